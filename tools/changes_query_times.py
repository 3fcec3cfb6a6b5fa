#!/usr/bin/env python3
"""Times of the change query of a source group (Engine.group_changes) on the livejournal stand-in, 10-source group, eps = 1e-9,
one batch after the mark -- and, in the same run, of the two yardsticks this query is held against: Engine.group_topk at the
same k, and the dense route it replaces (group_read of the ten columns at mark time and again now, the numpy subtraction,
filter and sort).

Per k in {100, 8192}, without and with remark:
  device ms  events around the first and the last kernel of the query (dppr_set_profiling, dppr_debug_query_ms)
  call ms    host clock around the Python call, which ends in a synchronisation of the solver stream
Every figure is the median of REPEATS calls after WARMUP calls of the same shape, with the spread (min .. max); the routes
alternate inside one repeat. Without remark the mark stays where it is and every repeat asks the same question. With remark a
query leaves the mark at the current p, so every repeat first takes ONE MORE BATCH (slide + group_update, untimed) and then
asks what that batch moved -- the per-batch feed; its dense route keeps the previous read and reads every source once. A run
without a GPU fails (there is no CPU path). Writes profiles/changes_query_times.md, stamped with the library's build id.

    python tools/changes_query_times.py [--out profiles/changes_query_times.md] [--repeats 15] [--warmup 3]
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


def stand_in(key, n_batches):
    cfg = datagen.STAND_INS[key]
    f = cfg.flags.split()
    opt = {f[i]: f[i + 1] for i in range(0, len(f), 2)}
    wl = st.workload_config(cfg.edges, 0.1, int(opt.get("-n", 0)), float(opt.get("-r", -1.0)), int(opt.get("-b", 0)),
                            int(opt.get("-c", 0)), int(opt.get("-l", 0)))
    V, e1, e2, _ = datagen.stand_in_stream(key, DATA, limit=wl.window + (1 + n_batches) * wl.per_batch)
    return V, e1, e2, cfg, wl


def diff_route(marks, nows, k):
    out = []
    for m, p in zip(marks, nows):
        d = p - m
        ids = np.nonzero(np.abs(d) > 0.0)[0]
        moved = len(ids)
        ids = ids[np.lexsort((ids, -np.abs(d[ids])))[:k]]
        out.append((ids.astype(np.int32), d[ids], p[ids], moved))
    return out


def summary(xs):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} .. {max(xs):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "changes_query_times.md"))
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    reps = a.warmup + a.repeats

    V, e1, e2, cfg, wl = stand_in("livejournal", 1 + 2 * reps)
    sources = [int(x) for x in datagen.ranked_sources(V, e1, e2, wl.window, cfg.directed, N_SOURCES, 1000, 10)]
    e = eng.Engine(V, wl.window, cfg.directed, wl.per_batch)
    ss = st.SlidingStream(V, e1, e2, cfg.directed, wl)
    e.load_window(*ss.serialize_edge_stream())
    gid = e.add_source_group(sources)
    e.group_init_solve(gid, EPS)

    def dense():
        return [e.group_read(gid, i)[0] for i in range(N_SOURCES)]

    def batch():
        assert not ss.stream_updates()
        e.set_batch(*ss.batch_arrays())
        e.slide(*ss.new_arrays())
        e.group_update(gid, EPS)

    def agree(got, want):  # ids, deltas and p bit for bit, moved
        for (gi, gd, gp, gm), (wi, wd, wp, wm) in zip(got, want):
            assert np.array_equal(gi, wi) and gm == wm
            assert np.array_equal(gd.view(np.uint64), wd.view(np.uint64)) and np.array_equal(gp.view(np.uint64), wp.view(np.uint64))

    e.group_mark(gid)
    marks = dense()
    batch()
    e.set_profiling(1)  # (only the queries below are timed by events)
    lines = []
    for remark in (False, True):
        for k in (100, 8192):
            t = {name: [] for name in ("c_dev", "c_call", "t_dev", "t_call", "d_call")}
            for rep in range(reps):
                if remark:
                    batch()
                t0 = time.perf_counter()
                got = e.group_changes(gid, k, 0.0, remark)
                t1 = time.perf_counter()
                c_dev = e.query_ms()
                t2 = time.perf_counter()
                e.group_topk(gid, k)
                t3 = time.perf_counter()
                t_dev = e.query_ms()
                t4 = time.perf_counter()
                if not remark:
                    dense()      # the dense route reads every source twice: at mark time ...
                nows = dense()   # ... and now (a feed keeps the previous read)
                want = diff_route(marks, nows, k)
                t5 = time.perf_counter()
                agree(got, want)
                if remark:
                    marks = nows
                if rep >= a.warmup:
                    for name, v in (("c_dev", c_dev), ("c_call", (t1 - t0) * 1e3), ("t_dev", t_dev), ("t_call", (t3 - t2) * 1e3),
                                    ("d_call", (t5 - t4) * 1e3)):
                        t[name].append(v)
            moved = [m for _, _, _, m in got]
            lines.append(f"| {k} | {int(remark)} | {summary(t['c_dev'])} | {summary(t['c_call'])} | {summary(t['t_dev'])} | "
                         f"{summary(t['t_call'])} | {summary(t['d_call'])} | {min(moved)} .. {max(moved)} |")
            print(lines[-1], flush=True)
        if not remark:  # the feed starts from a mark that is the current state
            e.group_mark(gid)
            marks = dense()
    sp = e.id_space()
    rows = sp["ids"] + sp["parked"]
    e.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# What a batch moved (`dppr_group_changes`): times\n\n")
        f.write(f"Library build `{eng.build_id()}`. livejournal stand-in, window of {wl.window} edges, batches of {wl.per_batch}, V = {V}, "
                f"{rows} rows hold a vertex at the end; {N_SOURCES}-source group, eps = {EPS:g}. `tools/changes_query_times.py`: median "
                f"(min .. max) in ms over {a.repeats} calls after {a.warmup} warm-up calls, the routes alternating inside a repeat. "
                "remark 0: marked after the from-scratch solve, every repeat asks what the one batch since then moved. remark 1: the "
                "per-batch feed, every repeat takes one more batch (untimed) and asks what it moved. Device time: events around the "
                "first and the last kernel of a query; call time: host clock around the Python call (ends in a stream "
                "synchronisation; allocation of the outputs and the copy back included). Dense route: group_read of the ten sources "
                "(twice for remark 0 -- at mark time and now; once for remark 1, where the previous read is kept), numpy subtraction, "
                "filter and lexsort. Every repeat checks that the two routes agree bit for bit.\n\n")
        f.write("| k | remark | group_changes: device | group_changes: call | group_topk (10 lanes): device | group_topk: call | "
                "dense reads + numpy diff, filter, sort: call | moved per source (last repeat) |\n|---|---|---|---|---|---|---|---|\n")
        f.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
