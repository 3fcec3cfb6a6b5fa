#!/usr/bin/env python3
"""Times of the conductance sweep of a source group (dppr_group_cluster) on the livejournal stand-in, 10-source group, eps = 1e-9,
after the from-scratch solve -- and, in the same run and on the same state, of dppr_group_topk at the same (k, min_p), the
selection the sweep starts with.

  group_cluster   k in {1024, 8192}, min_p = 0, min_size = 1: the records alone, and with the four arrays
  group_topk      the same k
  host route      what a caller without the call moves: Ed x 4 bytes of out-CSR (dppr_read_out_graph), besides the top-k

  device ms  events around the first and the last kernel of the library call (dppr_set_profiling, dppr_debug_query_ms)
  call ms    host clock around the Python call, which ends in a synchronisation of the solver stream
Every figure is the median of REPEATS calls after WARMUP calls, with the spread (min .. max). Also counted, from one copy of the
window to the host: how many out-row and in-row entries the orders' rows hold, which is what the row walk reads, and how many of those
rows are longer than CL_SPLIT entries and are walked in pieces. A run without a GPU fails (there is no CPU path). Writes
profiles/cluster_times.md, stamped with the library's build id.

    python tools/cluster_times.py [--out profiles/cluster_times.md] [--repeats 15] [--warmup 3]
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
EPS = 1e-9
N_SOURCES = 10
KS = (1024, 8192)
CL_SPLIT = 2048  # dynamicppr_amd/csrc/dppr_cluster_plan.hpp


def stand_in(key):
    cfg = datagen.STAND_INS[key]
    f = cfg.flags.split()
    opt = {f[i]: f[i + 1] for i in range(0, len(f), 2)}
    wl = st.workload_config(cfg.edges, 0.1, int(opt.get("-n", 0)), float(opt.get("-r", -1.0)), int(opt.get("-b", 0)),
                            int(opt.get("-c", 0)), int(opt.get("-l", 0)))
    V, e1, e2, _ = datagen.stand_in_stream(key, DATA, limit=wl.window + wl.per_batch)
    return V, e1, e2, cfg, wl


def summary(xs):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} .. {max(xs):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_times.md"))
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    reps = a.warmup + a.repeats

    V, e1, e2, cfg, wl = stand_in("livejournal")
    sources = [int(x) for x in datagen.ranked_sources(V, e1, e2, wl.window, cfg.directed, N_SOURCES, 1000, 10)]
    e = eng.Engine(V, wl.window, cfg.directed, wl.per_batch)
    ss = st.SlidingStream(V, e1, e2, cfg.directed, wl)
    a1, a2 = ss.serialize_edge_stream()
    e.load_window(a1, a2)
    gid = e.add_source_group(sources)
    e.group_init_solve(gid, EPS)
    e.set_profiling(1)
    sp = e.id_space()
    rows = sp["ids"] + sp["parked"]
    w1, w2 = np.asarray(a1, dtype=np.int64), np.asarray(a2, dtype=np.int64)
    if not cfg.directed:
        w1, w2 = np.concatenate([w1, w2]), np.concatenate([w2, w1])
    outdeg, indeg = np.bincount(w1, minlength=V), np.bincount(w2, minlength=V)
    Ed = len(w1)
    lines, counts = [], []

    def timed(name, fn, note=""):
        d, c = [], []
        for rep in range(reps):
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            if rep >= a.warmup:
                d.append(e.query_ms())
                c.append((t1 - t0) * 1e3)
        lines.append(f"| {name} | {summary(d)} | {summary(c)} | {note} |")
        print(lines[-1], flush=True)
        return statistics.median(d)

    for k in KS:
        best, ids, cut_out, cut_in, vol = e.group_cluster(gid, k, profile=True)
        entries_out = sum(int(outdeg[ids[i][ids[i] >= 0]].sum()) for i in range(N_SOURCES))
        entries_in = sum(int(indeg[ids[i][ids[i] >= 0]].sum()) for i in range(N_SOURCES))
        assert entries_out == sum(int(vol[i][b["count"] - 1]) for i, b in enumerate(best))  # (the window's degrees are the epoch's)
        split = sum(int((outdeg[ids[i][ids[i] >= 0]] > CL_SPLIT).sum() + (indeg[ids[i][ids[i] >= 0]] > CL_SPLIT).sum()) for i in range(N_SOURCES))
        counts.append(f"k = {k}: the {N_SOURCES} orders hold {sum(b['count'] for b in best)} vertices, {entries_out} out-row and {entries_in} in-row "
                      f"entries ({(entries_out + entries_in) / N_SOURCES / 1e6:.2f} M per source, {100.0 * (entries_out + entries_in) / N_SOURCES / (2 * Ed):.1f} % "
                      f"of the window's 2 x {Ed}), {split} rows longer than {CL_SPLIT} entries; best prefixes: "
                      + ", ".join(f"{b['best_size']} ({b['best_phi']:.4f})" for b in best) + ".")
        print(counts[-1], flush=True)
        t_cl = timed(f"group_cluster, k = {k}, records alone", lambda: e.group_cluster(gid, k), f"{4 * (entries_out + 2 * entries_in) / 1e6:.1f} MB of row entries")
        timed(f"group_cluster, k = {k}, with the four arrays", lambda: e.group_cluster(gid, k, profile=True), f"{28 * N_SOURCES * k / 1e6:.2f} MB copied back")
        t_tk = timed(f"group_topk, k = {k}", lambda: e.group_topk(gid, k))
        lines.append(f"| host route, k = {k} | - | - | {4 * Ed / 1e6:.1f} MB of out-CSR to the host, besides the top-k; the sweep adds "
                     f"{t_cl - t_tk:.3f} ms of device time to the selection |")
    e.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# Local clusters of the tracked sources (`dppr_group_cluster`): times\n\n")
        f.write(f"Library build `{eng.build_id()}`. livejournal stand-in, window of {wl.window} edges ({Ed} stored), V = {V}, {rows} rows "
                f"hold a vertex; {N_SOURCES}-source group (rows of 16 doubles), eps = {EPS:g}, after the from-scratch solve. "
                f"`tools/cluster_times.py`: median (min .. max) in ms over {a.repeats} calls after {a.warmup} warm-up calls. Device time: events "
                "around the first and the last kernel of the library call (the clearing of the rank table included); call time: host clock "
                "around the Python call (each ends in a synchronisation).\n\n")
        f.write("\n\n".join(counts) + "\n\n")
        f.write("| route | device ms | call ms | note |\n|---|---|---|---|\n")
        f.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
