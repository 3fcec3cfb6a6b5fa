#!/usr/bin/env python3
"""What a local forward query costs: dppr_forward_push against dppr_forward at the iteration count that leaves the same mass, on
the livejournal stand-in (BASELINE.json configs[2]), after the window is loaded and a few batches have slid, all in one session.

  cases      three start sets -- the hub (largest out-degree), a vertex of median out-degree among those with an out-edge, and a
             16-column call (the 16 vertices of largest out-degree) -- at eps in {1e-6, 1e-7, 1e-8}, max_rounds = 256.
  push       Engine.forward_push, the per-column statistics and work alone (no part that copies p out). Device time: events
             around the first kernel and the fold of rem of the library call (dppr_debug_query_ms, profiling on), so the
             read-backs of the chunk word are inside. Call time: host clock around the Python call (memsets included).
  sweep      Engine.forward with tol = 0 and iters = K = ceil(ln rem / ln 0.85), rem the LARGEST rem of the push's columns (the
             fewest sweeps that leave no more mass in that column: the comparison favours the sweep), clamped to [1, 256].
             The two calls alternate inside one loop.

Median (min .. max) over CALLS calls after WARMUP warm-up calls of each. A run without a GPU fails (there is no CPU path). Writes
profiles/fpush_times.md, stamped with the library's build id.

    python tools/fpush_times.py [--out profiles/fpush_times.md] [--batches 3] [--calls 10]
"""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dynamicppr_amd import engine as eng, stream as st  # noqa: E402
from tools.forward_times import WARMUP, stand_in, summary  # noqa: E402

EPSS = (1e-6, 1e-7, 1e-8)
MAX_ROUNDS = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpush_times.md"))
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()

    V, e1, e2, cfg, wl = stand_in("livejournal", a.batches)
    e = eng.Engine(V, wl.window, cfg.directed, wl.per_batch)
    ss = st.SlidingStream(V, e1, e2, cfg.directed, wl)
    e.load_window(*ss.serialize_edge_stream())
    for _ in range(a.batches):
        assert not ss.stream_updates()
        e.set_batch(*ss.batch_arrays())
        e.slide(*ss.new_arrays())
    e.set_profiling(1)
    row, col, _ = e.read_graph()
    Ed = int(row[-1])
    d = np.bincount(col[:Ed].astype(np.int64), minlength=V)
    live = int(np.count_nonzero(e.id_map() >= 0))
    by_deg = np.lexsort((np.arange(V), -d))   # out-degree descending, id ascending
    with_out = by_deg[:int(np.count_nonzero(d > 0))]
    median = int(with_out[len(with_out) // 2])
    cases = (("hub", [int(by_deg[0])]), ("median out-degree", [median]), ("16 columns", [int(x) for x in by_deg[:16]]))

    lines = []
    for name, starts in cases:
        for eps in EPSS:
            push_dev, push_call, fw_dev, fw_call = [], [], [], []
            res = e.forward_push(starts, eps, MAX_ROUNDS)
            rem = float(res["rem"].max())
            K = min(256, max(1, math.ceil(math.log(rem) / math.log(0.85)))) if 0.0 < rem < 1.0 else 1
            for k in range(WARMUP + a.calls):
                t0 = time.perf_counter()
                res = e.forward_push(starts, eps, MAX_ROUNDS)
                t1 = time.perf_counter()
                ms = e.query_ms()
                t2 = time.perf_counter()
                fw = e.forward(np.array(starts, dtype=np.int32), K, 0.0)
                t3 = time.perf_counter()
                if k >= WARMUP:
                    push_dev.append(ms)
                    push_call.append(1e3 * (t1 - t0))
                    fw_dev.append(e.query_ms())
                    fw_call.append(1e3 * (t3 - t2))
            assert np.all(fw["iters_used"] == K), fw["iters_used"]
            speedup = statistics.median(fw_dev) / statistics.median(push_dev)
            lines.append(f"| {name} (d = {', '.join(str(int(d[s])) for s in starts[:3])}{' ..' if len(starts) > 3 else ''}) | {eps:g} | "
                         f"{int(res['rounds_used'].max())} | {int(res['converged'].min())} | {int(res['pushes'].sum())} | "
                         f"{' / '.join(str(int(x)) for x in res['work'])} | {rem:.3g} | {summary(push_dev)} | {summary(push_call)} | {K} | "
                         f"{summary(fw_dev)} | {float(fw['rem'].max()):.3g} | {speedup:.2f} |")
            print(lines[-1], flush=True)
    e.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write("# The forward push (`dppr_forward_push`) against the forward sweep (`dppr_forward`) at the same remaining mass: times\n\n")
        fo.write(f"Library build `{eng.build_id()}`. livejournal stand-in, window of {wl.window} edges ({Ed} stored entries of the in-CSR), V = {V}, "
                 f"{live} vertices hold an id, after the load and {a.batches} slides. `tools/fpush_times.py`: median (min .. max) in ms over {a.calls} "
                 f"calls after {WARMUP} warm-up calls, the push and the sweep alternating in one loop; max_rounds = {MAX_ROUNDS}. device time = events "
                 "around the first kernel and the last kernel before the parts of the library call, the read-backs of the chunk word (every 8 rounds) "
                 "or of the freeze word (every 8 sweeps) inside; call time = host clock around the Python call, the memsets of the planes included. "
                 "work = rows pushed / rows gathered / in-edges of those rows over the union frontier, summed over the rounds; the dense sweep walks "
                 f"{Ed} entries per iteration. K = ceil(ln rem / ln 0.85) with the largest rem of the push's columns: the fewest sweeps that leave "
                 "no more mass. speed-up = sweep device ms / push device ms (below 1: the push is slower).\n\n")
        fo.write("| start | eps | rounds | all converged | pushes | work | rem (push) | push device ms | push call ms | K | sweep device ms | rem (sweep) | speed-up |\n")
        fo.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        fo.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
