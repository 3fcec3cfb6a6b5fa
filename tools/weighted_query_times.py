#!/usr/bin/env python3
"""Times of the weighted query of a source group (Engine.group_topk_weighted) on the livejournal stand-in, 10-source group,
eps = 1e-9, after the from-scratch solve -- and, in the same run, of the two yardsticks this change does not touch:
Engine.group_topk at the same k, and the dense route (group_read of the ten columns, the numpy fold, filter and sort).

Per k in {100, 8192} and q in {1, 16}:
  device ms  events around the first and the last kernel of the query (dppr_set_profiling, dppr_debug_query_ms)
  call ms    host clock around the Python call, which ends in a synchronisation of the solver stream
Every figure is the median of REPEATS calls after WARMUP calls of the same shape, with the spread (min .. max); the three
routes alternate inside one repeat. A run without a GPU fails (there is no CPU path). Writes profiles/weighted_query_times.md,
stamped with the library's build id.

    python tools/weighted_query_times.py [--out profiles/weighted_query_times.md] [--repeats 15] [--warmup 3]
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


def stand_in(key):
    cfg = datagen.STAND_INS[key]
    f = cfg.flags.split()
    opt = {f[i]: f[i + 1] for i in range(0, len(f), 2)}
    wl = st.workload_config(cfg.edges, 0.1, int(opt.get("-n", 0)), float(opt.get("-r", -1.0)), int(opt.get("-b", 0)),
                            int(opt.get("-c", 0)), int(opt.get("-l", 0)))
    V, e1, e2, _ = datagen.stand_in_stream(key, DATA, limit=wl.window + wl.per_batch)
    return V, e1, e2, cfg, wl


def fold(cols, w):
    acc = w[0] * cols[0]
    for i in range(1, len(cols)):
        acc = acc + w[i] * cols[i]
    return acc


def dense_route(e, gid, w, k):
    cols = [e.group_read(gid, i)[0] for i in range(N_SOURCES)]
    out = []
    for wj in w:
        score = fold(cols, wj)
        ids = np.nonzero(score > 0.0)[0]
        ids = ids[np.lexsort((ids, -score[ids]))[:k]]
        out.append((ids.astype(np.int32), score[ids]))
    return out


def summary(xs):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} .. {max(xs):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_query_times.md"))
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    V, e1, e2, cfg, wl = stand_in("livejournal")
    sources = [int(x) for x in datagen.ranked_sources(V, e1, e2, wl.window, cfg.directed, N_SOURCES, 1000, 10)]
    e = eng.Engine(V, wl.window, cfg.directed, wl.per_batch)
    ss = st.SlidingStream(V, e1, e2, cfg.directed, wl)
    e.load_window(*ss.serialize_edge_stream())
    gid = e.add_source_group(sources)
    e.group_init_solve(gid, EPS)
    e.set_profiling(1)  # (after the solve: only the queries below are timed by events)
    sp = e.id_space()
    rows = sp["ids"] + sp["parked"]
    rng = np.random.default_rng(1)

    lines = []
    for k in (100, 8192):
        for q in (1, 16):
            w = np.ones((1, N_SOURCES)) if q == 1 else rng.standard_normal((q, N_SOURCES))
            t = {name: [] for name in ("w_dev", "w_call", "t_dev", "t_call", "d_call")}
            for rep in range(a.warmup + a.repeats):
                t0 = time.perf_counter()
                got = e.group_topk_weighted(gid, w, k)
                t1 = time.perf_counter()
                w_dev = e.query_ms()
                t2 = time.perf_counter()
                e.group_topk(gid, k)
                t3 = time.perf_counter()
                t_dev = e.query_ms()
                t4 = time.perf_counter()
                want = dense_route(e, gid, w, k)
                t5 = time.perf_counter()
                if rep == 0:  # the routes agree (ids, and scores bit for bit) before anything is timed
                    for (gi, gs), (wi, ws) in zip(got, want):
                        assert np.array_equal(gi, wi) and np.array_equal(gs.view(np.uint64), ws.view(np.uint64))
                if rep >= a.warmup:
                    for name, v in (("w_dev", w_dev), ("w_call", (t1 - t0) * 1e3), ("t_dev", t_dev), ("t_call", (t3 - t2) * 1e3),
                                    ("d_call", (t5 - t4) * 1e3)):
                        t[name].append(v)
            lines.append(f"| {k} | {q} | {summary(t['w_dev'])} | {summary(t['w_call'])} | {summary(t['t_dev'])} | "
                         f"{summary(t['t_call'])} | {summary(t['d_call'])} |")
            print(lines[-1], flush=True)
    e.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# Weighted query of a source group: times\n\n")
        f.write(f"Library build `{eng.build_id()}`. livejournal stand-in, window of {wl.window} edges, V = {V}, {rows} rows hold a vertex; "
                f"{N_SOURCES}-source group, eps = {EPS:g}, after the from-scratch solve. `tools/weighted_query_times.py`: median "
                f"(min .. max) in ms over {a.repeats} calls after {a.warmup} warm-up calls, the three routes alternating inside a repeat. "
                "Device time: events around the first and the last kernel of a query; call time: host clock around the Python call "
                "(ends in a stream synchronisation; allocation of the outputs and the copy back included).\n\n")
        f.write("| k | q | weighted: device | weighted: call | group_topk (10 lanes): device | group_topk: call | "
                "dense: 10 x group_read + numpy fold, filter, sort (q vectors): call |\n|---|---|---|---|---|---|---|\n")
        f.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
