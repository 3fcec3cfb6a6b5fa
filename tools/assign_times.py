#!/usr/bin/env python3
"""What a labelling costs: dppr_assign against the recipe it replaces, on the livejournal stand-in (BASELINE.json configs[2]),
eps = 1e-9, after the from-scratch solve and a few batches, all in one session.

  10 sources     one group of the 10 vertices of largest in-degree (rows of 10 doubles)
  20 set lanes   two groups (16 + 4 lanes, as ./pagerank --target-sets deals 20 lines) of sets of 64 seeds each

  assign   torch_bridge.assign: labels + margin at a device destination, profiling on. Device time: events around the first and
           the last kernel of the library call (dppr_debug_query_ms); call time: host clock around the Python call.
  recipe   the label-propagation recipe of before: group_dense (dppr_group_export_dense_dev, [V][n] f64) per group, torch.cat over
           the groups, argmax(1) and -- where the margin is asked for -- topk(2) and a subtraction. Timed with events around the whole recipe, and by the host clock.

Median (min .. max) over CALLS calls after WARMUP warm-up calls. The bytes each path moves are counted by formula (below) and set
against the streaming copy the library calibrates (dppr_bench_stream_copy, 1 GiB). A run without a GPU fails (there is no CPU
path). Writes profiles/assign_times.md, stamped with the library's build id.

    python tools/assign_times.py [--out profiles/assign_times.md] [--batches 3] [--calls 15]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the library: one HIP runtime, dynamicppr_amd/torch_bridge.py)
from dynamicppr_amd import torch_bridge as tb  # noqa: E402
from dynamicppr_amd import datagen, engine as eng, stream as st  # noqa: E402

DATA = "/tmp/dppr_data"
EPS = 1e-9
WARMUP = 3


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


def recipe(e, groups, margin):
    D = [tb.group_dense(e, g, "p", torch.float64, "vertex_major") for g in groups]
    D = D[0] if len(D) == 1 else torch.cat(D, dim=1)
    label = D.argmax(1)
    if not margin:
        return label, None
    top = torch.topk(D, 2, dim=1).values
    return label, top[:, 0] - top[:, 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assign_times.md"))
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--calls", type=int, default=15)
    a = ap.parse_args()

    V, e1, e2, cfg, wl = stand_in("livejournal", a.batches)
    heads = np.asarray(e2[:wl.window], dtype=np.int64)
    if not cfg.directed:
        heads = np.concatenate([heads, np.asarray(e1[:wl.window], dtype=np.int64)])
    ranked = np.lexsort((np.arange(V), -np.bincount(heads, minlength=V)))   # in-degree descending, id ascending
    copy_ms = eng.bench_stream_copy(1 << 30)
    copy_gbs = 2 * (1 << 30) / copy_ms / 1e6
    dev = torch.device("cuda", 0)
    lines = []
    for name, make in (("10 sources, one group", lambda e: [e.add_source_group([int(x) for x in ranked[:10]])]),
                       ("20 set lanes of 64 seeds, groups of 16 + 4",
                        lambda e: [e.add_target_group([(ranked[i:20 * 64:20].astype(np.int32), np.full(64, 1.0 / 64)) for i in lanes])
                                   for lanes in (range(16), range(16, 20))])):
        e = eng.Engine(V, wl.window, cfg.directed, wl.per_batch)
        ss = st.SlidingStream(V, e1, e2, cfg.directed, wl)
        e.load_window(*ss.serialize_edge_stream())
        groups = make(e)
        for g in groups:
            e.group_init_solve(g, EPS)
        for _ in range(a.batches):
            assert not ss.stream_updates()
            e.set_batch(*ss.batch_arrays())
            e.slide(*ss.new_arrays())
            for g in groups:
                e.group_update(g, EPS)
        e.set_profiling(1)
        sp = e.id_space()
        rows = sp["ids"] + sp["parked"]
        widths = [2 * ((len(e.group_sources(g)) + 1) // 2) for g in groups]     # doubles per row: the lanes, padded to an even count
        n_classes = sum(len(e.group_sources(g)) for g in groups)
        state = sum(8 * w * rows for w in widths)
        for margin in (False, True):
            dev_ms, call_ms, rec_ev, rec_call = [], [], [], []
            for k in range(WARMUP + a.calls):
                t0 = time.perf_counter()
                tb.assign(e, groups, want=("margin",) if margin else ())
                t1 = time.perf_counter()
                q = e.query_ms()
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                t2 = time.perf_counter()
                ev0.record()
                recipe(e, groups, margin)
                ev1.record()
                torch.cuda.synchronize(dev)
                t3 = time.perf_counter()
                if k >= WARMUP:
                    dev_ms.append(q)
                    call_ms.append(1e3 * (t1 - t0))
                    rec_ev.append(ev0.elapsed_time(ev1))
                    rec_call.append(1e3 * (t3 - t2))
            a_bytes = state + 4 * V + 4 * V + (8 * V if margin else 0)    # rows once, the id map, labels (and margins) out
            r_bytes = state + 4 * V * len(groups) + 8 * V * n_classes     # the exports: rows, the id map per group, [V][n] out
            r_bytes += (2 * 8 * V * n_classes if len(groups) > 1 else 0)  # torch.cat: read and written again
            r_bytes += 8 * V * n_classes + 8 * V                          # argmax reads it, int64 labels out
            if margin:
                r_bytes += 8 * V * n_classes + 2 * 8 * V + 2 * 8 * V + 8 * V  # topk(2) reads it, two values out; read again, the margin out
            ad, rd = statistics.median(dev_ms), statistics.median(rec_ev)
            lines.append(f"| {name} | {'labels + margin' if margin else 'labels'} | {n_classes} | {rows} | {summary(dev_ms)} | {summary(call_ms)} | "
                         f"{a_bytes / 1e6:.1f} MB, {a_bytes / ad / 1e6:.0f} GB/s, {100 * a_bytes / ad / 1e6 / copy_gbs:.0f} % | {summary(rec_ev)} | "
                         f"{summary(rec_call)} | {r_bytes / 1e6:.1f} MB, {r_bytes / rd / 1e6:.0f} GB/s, {100 * r_bytes / rd / 1e6 / copy_gbs:.0f} % | {rd / ad:.1f} x |")
            print(lines[-1], flush=True)
        e.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# Every vertex to its best lane (`dppr_assign`) against the dense-export recipe: times\n\n")
        f.write(f"Library build `{eng.build_id()}`. livejournal stand-in, window of {wl.window} edges, V = {V}, eps = {EPS:g}, after the from-scratch "
                f"solve and {a.batches} batches. `tools/assign_times.py`: median (min .. max) in ms over {a.calls} calls after {WARMUP} warm-up calls. "
                "assign: labels, or labels + margin, at a device destination (`torch_bridge.assign`), device time = events around the first and the last "
                "kernel of the library call, call time = host clock around the Python call. recipe: `group_dense` per group, `torch.cat`, "
                "`argmax(1)` and, for the margin, `topk(2)` and the subtraction, events around the whole recipe and the host clock around it. Bytes by formula "
                "(rows that hold a vertex x row width x 8 read once per path; 4 V of id map per pass over the external ids; what each step "
                f"writes and reads back), against the stream copy of 1 GiB measured in the same process: {copy_ms:.3f} ms, {copy_gbs:.0f} GB/s "
                "read + write.\n\n")
        f.write("| case | asked for | classes | rows that hold a vertex | assign device ms | assign call ms | assign bytes, rate, of the copy rate | recipe event ms | "
                "recipe call ms | recipe bytes, rate, of the copy rate | recipe / assign |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
        f.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
