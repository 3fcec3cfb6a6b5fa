#!/usr/bin/env python3
"""What a sampling query costs: dppr_group_sample against today's route, on the livejournal stand-in (BASELINE.json configs[2]),
10 sources in one group, eps = 1e-9, after the from-scratch solve and a few batches, all in one session.

  sample     torch_bridge.group_sample with a device destination for S = 0 (the tree build alone), S = 65 536 and S = 2^20 / 10
             draws per lane, NULL spec and DEG + seeds,in. Device time: events around the first and the last kernel of the library
             call (dppr_debug_query_ms, profiling on); the draw pass is the difference to S = 0.
  dot        dppr_group_dot_dense_dev with F = 1 over the same group: the yardstick of the build, which reads the state once by
             external id as the dot pass does and, beyond it, writes 8 n Vt bytes of leaves: about twice the bytes.
  route      today's: dppr_group_export_dense_dev (source-major float64), a torch clamp, one torch.multinomial per lane (V must not
             exceed 2^24 for it). Host clock around all of it with a device synchronisation, and the export's device time.

Median (min .. max) over CALLS calls after WARMUP warm-up calls. The bytes of a draw are counted by formula (2 KB of leaves, 16 bytes
per stored level, 12 bytes out) and set against the streaming copy the library calibrates (dppr_bench_stream_copy, 1 GiB). A run
without a GPU fails (there is no CPU path). Writes profiles/sample_times.md, stamped with the library's build id.

    python tools/sample_times.py [--out profiles/sample_times.md] [--batches 3] [--calls 20]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dynamicppr_amd import datagen, engine as eng, stream as st, torch_bridge as tb  # noqa: E402

DATA = "/tmp/dppr_data"
EPS = 1e-9
WARMUP = 3
TILE = 2048


def stand_in(key, batches):
    cfg = datagen.STAND_INS[key]
    f = cfg.flags.split()
    opt = {f[i]: f[i + 1] for i in range(0, len(f), 2)}
    wl = st.workload_config(cfg.edges, 0.1, int(opt.get("-n", 0)), float(opt.get("-r", -1.0)), int(opt.get("-b", 0)),
                            int(opt.get("-c", 0)), int(opt.get("-l", 0)))
    V, e1, e2, _ = datagen.stand_in_stream(key, DATA, limit=wl.window + batches * wl.per_batch)
    return V, e1, e2, cfg, wl


def summary(xs):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} .. {max(xs):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_times.md"))
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()

    V, e1, e2, cfg, wl = stand_in("livejournal", a.batches)
    heads = np.asarray(e2[:wl.window], dtype=np.int64)
    if not cfg.directed:
        heads = np.concatenate([heads, np.asarray(e1[:wl.window], dtype=np.int64)])
    ranked = np.lexsort((np.arange(V), -np.bincount(heads, minlength=V)))   # in-degree descending, id ascending
    copy_ms = eng.bench_stream_copy(1 << 30)
    copy_gbs = 2 * (1 << 30) / copy_ms / 1e6
    n = 10
    e = eng.Engine(V, wl.window, cfg.directed, wl.per_batch)
    ss = st.SlidingStream(V, e1, e2, cfg.directed, wl)
    e.load_window(*ss.serialize_edge_stream())
    gid = e.add_source_group([int(x) for x in ranked[:n]])
    e.group_init_solve(gid, EPS)
    for _ in range(a.batches):
        assert not ss.stream_updates()
        e.set_batch(*ss.batch_arrays())
        e.slide(*ss.new_arrays())
        e.group_update(gid, EPS)
    e.set_profiling(1)
    dev = torch.device("cuda", e.device)
    Vt = -(-V // TILE) * TILE
    levels = max((V - 1).bit_length(), 11) - 8          # stored levels a draw descends before its subtile
    draw_bytes = 2048 + 16 * levels + 12

    # the yardstick of the build: the dense dot pass with F = 1
    h = torch.ones((1, V), dtype=torch.float64, device=dev)
    dot_ms = []
    for k in range(WARMUP + a.calls):
        tb.group_dot(e, gid, h)
        if k >= WARMUP:
            dot_ms.append(e.query_ms())
    dot_med = statistics.median(dot_ms)

    lines, route_lines = [], []
    for what, kw in (("NULL", {}), ("DEG + seeds,in", dict(factor="deg", exclude=("seeds", "in")))):
        build_med = None
        for S in (0, 65536, (1 << 20) // n):
            dev_ms, call_ms = [], []
            for k in range(WARMUP + a.calls):
                t0 = time.perf_counter()
                ids, w, total, support, status = tb.group_sample(e, gid, S, seed=k, **kw)
                t1 = time.perf_counter()
                if k >= WARMUP:
                    dev_ms.append(e.query_ms())
                    call_ms.append(1e3 * (t1 - t0))
            med = statistics.median(dev_ms)
            if S == 0:
                build_med = med
                note = f"build / dot = {med / dot_med:.2f}; {8 * n * Vt * (1 + 1 / 128) / 1e6:.1f} MB written, {8 * n * Vt * (1 + 1 / 128) / med / 1e6:.0f} GB/s of writes"
            else:
                draw_ms = med - build_med
                gbs = n * S * draw_bytes / draw_ms / 1e6
                note = f"draw pass {draw_ms:.3f} ms, {n * S / draw_ms / 1e3:.1f} M draws/s, {n * S * draw_bytes / 1e6:.1f} MB, {gbs:.0f} GB/s, {100 * gbs / copy_gbs:.0f} % of the copy rate"
            lines.append(f"| {what} | {S} | {summary(dev_ms)} | {summary(call_ms)} | {int(support.min())} .. {int(support.max())} | {note} |")
            print(lines[-1], flush=True)
            if what == "NULL" and S > 0 and V <= (1 << 24):
                r_ms, ex_ms = [], []
                for k in range(WARMUP + a.calls):
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    dense = tb.group_dense(e, gid)                     # [n, V] float64
                    q = e.query_ms()
                    dense.clamp_(min=0.0)
                    got = [torch.multinomial(dense[i], S, replacement=True) for i in range(n)]
                    torch.cuda.synchronize(dev)
                    t1 = time.perf_counter()
                    if k >= WARMUP:
                        r_ms.append(1e3 * (t1 - t0))
                        ex_ms.append(q)
                    del got, dense
                route_lines.append(f"| {S} | {summary(ex_ms)} | {summary(r_ms)} | {8 * n * V / 1e6:.1f} MB | {statistics.median(r_ms) / statistics.median(call_ms):.1f} x |")
                print(route_lines[-1], flush=True)
    e.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# Vertices drawn in proportion to a lane's score (`dppr_group_sample`) against today's route: times\n\n")
        f.write(f"Library build `{eng.build_id()}`. livejournal stand-in, window of {wl.window} edges, V = {V} (Vt = {Vt}, {levels} stored levels above a "
                f"subtile), {n} sources in one group, eps = {EPS:g}, after the from-scratch solve and {a.batches} batches. `tools/sample_times.py`: "
                f"median (min .. max) in ms over {a.calls} calls after {WARMUP} warm-up calls, device destination. device time = events around the "
                "first and the last kernel of the library call, call time = host clock around the Python call (with the allocation of the "
                "result tensors). S = 0 is the tree build alone; the draw pass is the difference to it. Bytes of a draw by formula: "
                f"2048 of leaves + 16 per stored level + 12 out = {draw_bytes}. `dppr_group_dot_dense_dev`, F = 1, same group, same run: "
                f"{summary(dot_ms)} ms device. Stream copy of 1 GiB in the same process: {copy_ms:.3f} ms, {copy_gbs:.0f} GB/s read + write.\n\n")
        f.write("| spec | S per lane | sample device ms | sample call ms | support per lane | |\n|---|---|---|---|---|---|\n")
        f.write("\n".join(lines) + "\n")
        if route_lines:
            f.write("\nToday's route in the same session: `dppr_group_export_dense_dev` (source-major float64), `clamp_(min=0)`, one "
                    "`torch.multinomial(replacement=True)` per lane; host clock around all of it, synchronised.\n\n")
            f.write("| S per lane | export device ms | route call ms | bytes out of the engine | route call / sample call |\n|---|---|---|---|---|\n")
            f.write("\n".join(route_lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
