#!/usr/bin/env python3
"""What a position query costs: dppr_group_position_at against the two recipes of before, on the livejournal stand-in
(BASELINE.json configs[2]), 10 sources in one group, eps = 1e-9, after the from-scratch solve and a few batches, all in one session.

  position   Engine.group_position_at(ids) for m = 16, 1024, 4096 ids, NULL spec and DEG + seeds,in. Device time: events around
             the first and the last kernel of the library call (dppr_debug_query_ms, profiling on); call time: host clock around
             the Python call.
  recipe i   group_topk_ranked(k = 8192) and a search of the returned lists on the host (a dict per lane). It cannot answer a
             query whose position is 8192 or more: the share of (id, lane) pairs with a position that it misses is reported.
  recipe ii  group_rank_score_at(arange(V)) -- every column over PCIe -- and the numpy order of tests/position_ref.py. It does not
             depend on m beyond the final lookup and takes seconds, so it is timed once per spec, at the 4096 ids.

Half of the ids are drawn from the vertices that qualify in lane 0, half from all of [0, V). Median (min .. max) over CALLS calls
after WARMUP warm-up calls. The bytes of the count pass are counted by formula (below) and set against the streaming copy the
library calibrates (dppr_bench_stream_copy, 1 GiB); --skip-recipes and --m leave the position calls alone, for a kernel trace of
one shape. A run without a GPU fails (there is no CPU path). Writes profiles/position_times.md, stamped with the library's build id.

    python tools/position_times.py [--out profiles/position_times.md] [--batches 3] [--calls 15] [--m 16,1024,4096] [--skip-recipes]
                                     [--dense-calls N]
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
from tests import position_ref  # noqa: E402

DATA = "/tmp/dppr_data"
EPS = 1e-9
WARMUP = 3
K_MAX = 8192
LDS_QUERIES = 4096   # (lane, query) pairs a workgroup of the count pass holds: dppr_position_plan.hpp


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


def shape(n, m):
    """pos_shape of dppr_position_plan.hpp without a cap: (tile, lanes, lane blocks, passes)."""
    tile = min(max(m, 1), LDS_QUERIES)
    lanes = min(LDS_QUERIES // tile, n)
    return tile, lanes, -(-n // lanes), max(-(-m // tile), 1)


def recipe_topk(e, gid, ids, spec):
    """Recipe i: (pos [m][n] with -2 where the lists do not tell, device ms of the selection)."""
    lists = e.group_topk_ranked(gid, K_MAX, 0.0, spec)
    q = e.query_ms()
    pos = np.empty((len(ids), len(lists)), dtype=np.int32)
    for i, (gi, _) in enumerate(lists):
        where = {int(v): t for t, v in enumerate(gi)}
        full = len(gi) == K_MAX   # (a shorter list is the whole order: what is not in it does not qualify)
        pos[:, i] = [where.get(int(v), -2 if full else -1) for v in ids]
    return pos, q


def recipe_dense(e, gid, ids, spec, V):
    """Recipe ii: every column to the host, the numpy order."""
    sc = e.group_rank_score_at(gid, np.arange(V, dtype=np.int32), spec)
    q = e.query_ms()
    return position_ref.group_positions([sc[:, i] for i in range(sc.shape[1])], ids), q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "position_times.md"))
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--m", default="16,1024,4096")
    ap.add_argument("--skip-recipes", action="store_true")
    ap.add_argument("--dense-calls", type=int, default=None, help="calls of recipe ii (default: --calls)")
    a = ap.parse_args()
    ms_list = [int(x) for x in a.m.split(",")]
    dense_calls = a.calls if a.dense_calls is None else a.dense_calls

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
    sp = e.id_space()
    rows = sp["ids"] + sp["parked"]
    rng = np.random.default_rng(3)
    lane0 = np.nonzero(e.group_read(gid, 0)[0] > 0)[0]
    specs = (("NULL", None), ("DEG + seeds,in", eng.Engine.rank_spec(eng.FACTOR_DEG, exclude=eng.EXCLUDE_SEEDS | eng.EXCLUDE_IN_NEIGHBOURS)))
    lines, dense_lines = [], []
    for what, spec in specs:
        for m in ms_list:
            ids = np.concatenate([rng.choice(lane0, m // 2, replace=False), rng.integers(0, V, m - m // 2)]).astype(np.int32)
            dev_ms, call_ms, r1_dev, r1_call = [], [], [], []
            pos = cnt = None
            for k in range(WARMUP + a.calls):
                t0 = time.perf_counter()
                pos, cnt = e.group_position_at(gid, ids, spec)
                t1 = time.perf_counter()
                q = e.query_ms()
                if k >= WARMUP:
                    dev_ms.append(q)
                    call_ms.append(1e3 * (t1 - t0))
                if a.skip_recipes:
                    continue
                t2 = time.perf_counter()
                got, q1 = recipe_topk(e, gid, ids, spec)
                t3 = time.perf_counter()
                if k >= WARMUP:
                    r1_dev.append(q1)
                    r1_call.append(1e3 * (t3 - t2))
                told = got != -2
                assert np.array_equal(got[told], pos[told]) and np.all((pos[~told] >= K_MAX) | (pos[~told] == -1))   # (a full list does not tell "beyond it" from "never")
            tile, lanes, blocks, passes = shape(n, m)
            # the count pass: every lane block reads its lanes' doubles of every row and the row's id, once per pass; the keys and
            # ids of a workgroup's tile (12 bytes a position) are small beside it
            c_bytes = passes * rows * (8 * n + 4 * blocks)
            missed = ""
            if not a.skip_recipes:
                answered = pos >= 0
                blind = int(np.count_nonzero(pos >= K_MAX))
                missed = f"{summary(r1_dev)} | {summary(r1_call)} | {blind} of {int(np.count_nonzero(answered))} ({100.0 * blind / max(int(np.count_nonzero(answered)), 1):.1f} %)"
            lines.append(f"| {what} | {m} | {tile} x {lanes}, {blocks} x {passes} | {summary(dev_ms)} | {summary(call_ms)} | {c_bytes / 1e6:.1f} MB | "
                         f"{int(cnt.min())} .. {int(cnt.max())} | {missed or '- | - | -'} |")
            print(lines[-1], flush=True)
            if m == ms_list[-1] and not a.skip_recipes:
                r2_dev, r2_call = [], []
                for k in range(WARMUP + dense_calls):
                    t0 = time.perf_counter()
                    (wp, wc), q2 = recipe_dense(e, gid, ids, spec, V)
                    t1 = time.perf_counter()
                    assert np.array_equal(wp, pos) and np.array_equal(wc, cnt)
                    if k >= WARMUP:
                        r2_dev.append(q2)
                        r2_call.append(1e3 * (t1 - t0))
                dense_lines.append(f"| {what} | {m} | {summary(r2_dev)} | {summary(r2_call)} | {8 * V * n / 1e6:.1f} MB | "
                                   f"{statistics.median(r2_call) / statistics.median(call_ms):.0f} x |")
                print(dense_lines[-1], flush=True)
    e.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# Positions of given vertices in a lane's order (`dppr_group_position_at`) against the two recipes of before: times\n\n")
        f.write(f"Library build `{eng.build_id()}`. livejournal stand-in, window of {wl.window} edges, V = {V}, {rows} rows hold a vertex, {n} sources in "
                f"one group, eps = {EPS:g}, after the from-scratch solve and {a.batches} batches. `tools/position_times.py`: median (min .. max) in ms "
                f"over {a.calls} calls after {WARMUP} warm-up calls. Half of the ids qualify in lane 0, half are drawn from all of [0, V). position: "
                "device time = events around the first and the last kernel of the library call, call time = host clock around the Python "
                "call. shape = queries x lanes a workgroup of the count pass holds, lane blocks x passes of its grid. count pass bytes by "
                "formula: passes x rows x (8 n + 4 lane blocks). Recipe i: `group_topk_ranked(k = 8192)` and a host search of its lists (device "
                "time of the selection, host clock around selection + search); blind = (id, lane) pairs with a position of 8192 or more, "
                "which it cannot give, of the pairs that have a position. Recipe ii: `group_rank_score_at(arange(V))` and the numpy order "
                "(device time of the point read, host clock around all of it), once per spec"
                f"{'' if dense_calls == a.calls else f', {dense_calls} calls after {WARMUP}'}. Every recipe result that exists was compared "
                f"with the call's: equal. Stream copy of 1 GiB in the same process: {copy_ms:.3f} ms, {copy_gbs:.0f} GB/s read + write.\n\n")
        f.write("| spec | m | shape | position device ms | position call ms | count pass bytes | qualifying per lane | recipe i device ms | "
                "recipe i call ms | recipe i blind |\n|---|---|---|---|---|---|---|---|---|---|\n")
        f.write("\n".join(lines) + "\n")
        if dense_lines:
            f.write("\n| spec | m | recipe ii device ms | recipe ii call ms | bytes over PCIe | recipe ii call / position call |\n|---|---|---|---|---|---|\n")
            f.write("\n".join(dense_lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
