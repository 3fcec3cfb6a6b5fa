#!/usr/bin/env python3
"""What an explain query costs: dppr_group_explain_at against the recipe of before, on the livejournal stand-in
(BASELINE.json configs[2]), 10 sources in one group, eps = 1e-9, after the from-scratch solve and a few batches, all in one session.

  explain   Engine.group_explain_at(ids, f, depth) for m = 16, 1024, 4096 ids and (f, depth) = (3, 16), (16, 64), with the memo of
            next hops off, on, and as the plan chooses (dppr_debug_explain). Device time: events around the first and the last
            kernel of the library call (dppr_debug_query_ms, profiling on); call time: host clock around the Python call.
  recipe    group_read of every column and read_out_graph -- the window over PCIe -- then tests/explain_ref.py (np.unique over the
            edges, the three-operation contribution, np.lexsort, a Python loop for the paths). It takes seconds, so it is timed
            once per (f, depth), at the largest m; the dense reads and the group-by are timed apart from the per-id work.

Half of the ids are drawn from the vertices that qualify in lane 0 (p > 0), half from all of [0, V). Median (min .. max) over CALLS
calls after WARMUP warm-up calls. Every answer of the three memo settings is compared with the others', and at the largest m with
the recipe's. --skip-recipe, --m, --shapes and --memos leave some calls alone, for a kernel trace of one shape. A run without a GPU fails (there is no
CPU path). Writes profiles/explain_times.md, stamped with the library's build id.

    python tools/explain_times.py [--out profiles/explain_times.md] [--batches 3] [--calls 15] [--m 16,1024,4096] [--shapes 3x16,16x64]
                                    [--memos off,on,plan] [--skip-recipe]
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
from tests import explain_ref as xr  # noqa: E402

DATA = "/tmp/dppr_data"
EPS = 1e-9
WARMUP = 3
SHAPES = ((3, 16), (16, 64))
MEMOS = (("off", 0), ("on", 1), ("plan", -1))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explain_times.md"))
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--m", default="16,1024,4096")
    ap.add_argument("--shapes", default=",".join(f"{f}x{d}" for f, d in SHAPES), help="f x depth, comma separated")
    ap.add_argument("--memos", default=",".join(w for w, _ in MEMOS), help="off, on, plan")
    ap.add_argument("--skip-recipe", action="store_true")
    a = ap.parse_args()
    ms_list = [int(x) for x in a.m.split(",")]
    shapes = [tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",")]
    memos = [(w, v) for w, v in MEMOS if w in a.memos.split(",")]

    V, e1, e2, cfg, wl = stand_in("livejournal", a.batches)
    heads = np.asarray(e2[:wl.window], dtype=np.int64)
    if not cfg.directed:
        heads = np.concatenate([heads, np.asarray(e1[:wl.window], dtype=np.int64)])
    ranked = np.lexsort((np.arange(V), -np.bincount(heads, minlength=V)))   # in-degree descending, id ascending
    n = 10
    sources = [int(x) for x in ranked[:n]]
    e = eng.Engine(V, wl.window, cfg.directed, wl.per_batch)
    ss = st.SlidingStream(V, e1, e2, cfg.directed, wl)
    e.load_window(*ss.serialize_edge_stream())
    gid = e.add_source_group(sources)
    e.group_init_solve(gid, EPS)
    for _ in range(a.batches):
        assert not ss.stream_updates()
        e.set_batch(*ss.batch_arrays())
        e.slide(*ss.new_arrays())
        e.group_update(gid, EPS)
    e.set_profiling(1)
    sp = e.id_space()
    rng = np.random.default_rng(3)
    lane0 = np.nonzero(e.group_read(gid, 0)[0] > 0)[0]
    lines, recipe_lines = [], []
    graph = cols = None
    read_ms = group_ms = 0.0
    for f, depth in shapes:
        for m in ms_list:
            ids = np.concatenate([rng.choice(lane0, m // 2, replace=False), rng.integers(0, V, m - m // 2)]).astype(np.int32)
            cells, first, res = [], None, None
            for what, memo in memos:
                e.debug_explain(memo, 64)
                dev_ms, call_ms = [], []
                for k in range(WARMUP + a.calls):
                    t0 = time.perf_counter()
                    res = e.group_explain_at(gid, ids, f, depth)
                    t1 = time.perf_counter()
                    if k >= WARMUP:
                        dev_ms.append(e.query_ms())
                        call_ms.append(1e3 * (t1 - t0))
                first = first or res
                xr.same(res, first, ("memo", what, m, f, depth))
                cells.append(f"{summary(dev_ms)} | {summary(call_ms)}")
            e.debug_explain(-1, 64)
            ends = np.bincount(first["end"].ravel(), minlength=4)
            lines.append(f"| {f}, {depth} | {m} | " + " | ".join(cells) + f" | {int(first['deg'].max())} | {int(first['len'].max())} | "
                         f"{ends[0]} / {ends[1]} / {ends[2]} / {ends[3]} |")
            print(lines[-1], flush=True)
            if m == ms_list[-1] and not a.skip_recipe:
                t0 = time.perf_counter()
                cols = [e.group_read(gid, i)[0] for i in range(n)]
                row, col = e.read_out_graph()
                t1 = time.perf_counter()
                graph = xr.from_csr(row, col)
                t2 = time.perf_counter()
                want = xr.explain(graph, cols, sources, ids, f, depth)
                t3 = time.perf_counter()
                xr.same(first, want, ("recipe", m, f, depth))
                read_ms, group_ms = 1e3 * (t1 - t0), 1e3 * (t2 - t1)
                call = float(cells[-1].split("|")[1].split("(")[0])
                recipe_lines.append(f"| {f}, {depth} | {m} | {read_ms:.0f} | {group_ms:.0f} | {1e3 * (t3 - t2):.0f} | {1e3 * (t3 - t0):.0f} | "
                                    f"{(8 * V * n + 4 * (V + 1) + 4 * len(col)) / 1e6:.1f} MB | {1e3 * (t3 - t0) / call:.0f} x |")
                print(recipe_lines[-1], flush=True)
    e.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        out.write("# Explain a score (`dppr_group_explain_at`) against the recipe of before: times\n\n")
        out.write(f"Library build `{eng.build_id()}`. livejournal stand-in, window of {wl.window} edges, V = {V}, {sp['ids']} live rows, {n} sources "
                  f"in one group, eps = {EPS:g}, after the from-scratch solve and {a.batches} batches. `tools/explain_times.py`: median (min .. max) "
                  f"in ms over {a.calls} calls after {WARMUP} warm-up calls. Half of the ids have p > 0 in lane 0, half are drawn from all of "
                  "[0, V). device = events around the first and the last kernel of the library call (with the memo on: its memset too), "
                  "call = host clock around the Python call, which allocates and fills the twelve output arrays. memo off / on: "
                  "`dppr_debug_explain(0 | 1)`; memo plan: what `ex_memo_on` of `dppr_explain_plan.hpp` chooses. The results of the three "
                  "settings were compared: equal. ends = (query, lane) pairs that end at a seed / at the depth / dead / in a cycle.\n\n")
        out.write("| f, depth | m | " + " | ".join(f"memo {w} device ms | memo {w} call ms" for w, _ in memos) + " | longest row | longest path | ends |\n"
                  + "|---" * (5 + 2 * len(memos)) + "|\n")
        out.write("\n".join(lines) + "\n")
        if recipe_lines:
            out.write("\nThe recipe it replaces, once per (f, depth) at the largest m: `group_read` of every column and `read_out_graph`, the "
                      "group-by of `tests/explain_ref.py` (np.unique over the edges), then its contributors and paths of the m ids. Every "
                      "answer was compared with the call's: equal.\n\n")
            out.write("| f, depth | m | dense reads + out-CSR ms | group-by ms | contributors and paths ms | recipe ms | bytes over PCIe | recipe / plan call |\n"
                      "|---|---|---|---|---|---|---|---|\n")
            out.write("\n".join(recipe_lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
