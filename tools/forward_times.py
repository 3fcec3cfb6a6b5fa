#!/usr/bin/env python3
"""What a forward query costs: dppr_forward against what a caller has today, on the livejournal stand-in (BASELINE.json
configs[2]), after the window is loaded and a few batches have slid, all in one session.

  forward    Engine.forward with m in {1, 10, 16} starts (vertices of largest out-degree, so that no column dies), iters = 64,
             tol = 0, iters_used and rem alone (no part that copies f out). Device time: events around the first kernel and the
             last check of the library call (dppr_debug_query_ms, profiling on), so the 8 read-backs of the freeze word are
             inside; per sweep = that time / 64. Call time: host clock around the Python call. Then the same call with a top 100.
  today      dppr_read_graph to the host (the in-CSR by external id), then the plain numpy power iteration of the definition for
             ONE start: y = 0.85 x / (d + 1), x = bincount(heads, y[tails]), f += 0.15 x, 64 times. (Not the fold: the order of
             the additions is numpy's. It is the cost that is measured.) Host clock.

Median (min .. max) over CALLS calls after WARMUP warm-up calls. The bytes of a sweep are counted by formula -- 8 per entry, one
row of 8 gw bytes gathered per entry, 8 gw read and 16 gw written per live row -- and set against the streaming copy the library
calibrates (dppr_bench_stream_copy, 1 GiB). A run without a GPU fails (there is no CPU path). Writes profiles/forward_times.md,
stamped with the library's build id.

    python tools/forward_times.py [--out profiles/forward_times.md] [--batches 3] [--calls 10]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dynamicppr_amd import datagen, engine as eng, stream as st  # noqa: E402

DATA = "/tmp/dppr_data"
WARMUP = 2
ITERS = 64


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


def row_width(m):
    return 2 if m <= 2 else (m + 1) // 2 * 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forward_times.md"))
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()

    V, e1, e2, cfg, wl = stand_in("livejournal", a.batches)
    copy_ms = eng.bench_stream_copy(1 << 30)
    copy_gbs = 2 * (1 << 30) / copy_ms / 1e6
    e = eng.Engine(V, wl.window, cfg.directed, wl.per_batch)
    ss = st.SlidingStream(V, e1, e2, cfg.directed, wl)
    e.load_window(*ss.serialize_edge_stream())
    for _ in range(a.batches):
        assert not ss.stream_updates()
        e.set_batch(*ss.batch_arrays())
        e.slide(*ss.new_arrays())
    e.set_profiling(1)

    # today's route, and the shape of the window
    t_read, t_iter = [], []
    for k in range(3):
        t0 = time.perf_counter()
        row, col, deg = e.read_graph()
        t1 = time.perf_counter()
        t_read.append(1e3 * (t1 - t0))
    row64 = row.astype(np.int64)
    Ed = int(row64[-1])
    tails = col[:Ed].astype(np.int64)
    heads = np.repeat(np.arange(V, dtype=np.int64), np.diff(row64))
    d = np.bincount(tails, minlength=V).astype(np.float64)
    live = int(np.count_nonzero(e.id_map() >= 0))
    starts = np.lexsort((np.arange(V), -d))[:16].astype(np.int32)   # out-degree descending, id ascending
    for k in range(2):
        t0 = time.perf_counter()
        x = np.zeros(V)
        x[starts[0]] = 1.0
        f = 0.15 * x
        for _ in range(ITERS):
            y = (0.85 * x) / (d + 1.0)
            x = np.bincount(heads, weights=y[tails], minlength=V)
            f = f + 0.15 * x
        t_iter.append(1e3 * (time.perf_counter() - t0))
    probe = np.argsort(-f)[:eng.FORWARD_AT_MAX].astype(np.int32)   # the 4096 largest entries
    got = e.forward(starts[:1], ITERS, at=probe)
    apart = float(np.max(np.abs(got["at"][0] - f[probe])))

    lines = []
    for m in (1, 10, 16):
        gw = row_width(m)
        sweep_bytes = Ed * (8 + 8 * gw) + live * 24 * gw
        for what, kw in (("iters_used, rem", {}), ("+ top 100", dict(k=100))):
            dev_ms, call_ms = [], []
            for k in range(WARMUP + a.calls):
                t0 = time.perf_counter()
                res = e.forward(starts[:m], ITERS, 0.0, **kw)
                t1 = time.perf_counter()
                if k >= WARMUP:
                    dev_ms.append(e.query_ms())
                    call_ms.append(1e3 * (t1 - t0))
            assert np.all(res["iters_used"] == ITERS), res["iters_used"]
            per = statistics.median(dev_ms) / ITERS
            gbs = sweep_bytes / per / 1e6
            lines.append(f"| {m} | {gw} | {what} | {summary(dev_ms)} | {1e3 * per:.1f} | {summary(call_ms)} | {sweep_bytes / 1e6:.0f} MB, {gbs:.0f} GB/s, "
                         f"{100 * gbs / copy_gbs:.0f} % of the copy rate | {float(res['rem'].max()):.2e} |")
            print(lines[-1], flush=True)
    e.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write("# The forward sweep (`dppr_forward`) against what a caller has today: times\n\n")
        fo.write(f"Library build `{eng.build_id()}`. livejournal stand-in, window of {wl.window} edges ({Ed} stored entries of the in-CSR), V = {V}, "
                 f"{live} vertices hold an id, after the load and {a.batches} slides. `tools/forward_times.py`: median (min .. max) in ms over {a.calls} "
                 f"calls after {WARMUP} warm-up calls; iters = {ITERS}, tol = 0, the starts are the vertices of largest out-degree (every column runs all "
                 f"{ITERS} iterations). device time = events around the first kernel and the last check of the library call, the 8 read-backs of the "
                 f"freeze word inside; per sweep = device time / {ITERS} (the checks and the read-backs are spread over the sweeps). call time = host "
                 "clock around the Python call, with the memset of the planes and the selection of the top 100 where asked for. Bytes of a sweep by "
                 f"formula: 8 per entry + one gathered row of 8 gw per entry + 24 gw per live row. Stream copy of 1 GiB in the same process: "
                 f"{copy_ms:.3f} ms, {copy_gbs:.0f} GB/s read + write.\n\n")
        fo.write("| m | row width | parts | device ms per call | us per sweep | call ms | bytes of a sweep by formula | largest rem |\n|---|---|---|---|---|---|---|---|\n")
        fo.write("\n".join(lines) + "\n")
        fo.write(f"\nToday's route in the same session, ONE start: `dppr_read_graph` to the host {summary(t_read)} ms ({(4 * (V + 1) + 4 * Ed + 4 * V) / 1e6:.0f} MB), "
                 f"then {ITERS} iterations of the definition in numpy (`bincount` over the entries) {summary(t_iter)} ms: "
                 f"{(statistics.median(t_read) + statistics.median(t_iter)) / 1e3:.2f} s per start. Its f and the device's differ by at most {apart:.2e} over its 4096 largest entries "
                 "(numpy's order of additions against the fold's).\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
