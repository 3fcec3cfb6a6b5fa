#!/usr/bin/env python3
"""What the ranked, position and sample queries over a forward track cost on the device (dppr_ftrack_topk_ranked /
dppr_ftrack_position_at / dppr_ftrack_sample) against the host path a caller had before them: a dense copy of the track's p, the
out-rows of the epoch, and numpy -- on the livejournal stand-in (BASELINE.json configs[2]) with the tracks of
profiles/fcluster_times.md, all in one session.

  cases      three start sets -- the hub (largest out-degree), a vertex of median out-degree among those with an out-edge, and a
             64-seed set -- at eps in {1e-6, 1e-8}, max_rounds = 256, as a track of m = 1 column and as one of m = 16 (the hub and
             the 15 next vertices by out-degree; the median vertex and its 15 neighbours in the degree order; 16 different 64-seed
             sets). The spec is DPPR_FACTOR_DEG with the seeds and their out-neighbours excluded, min_score 0.
  device     ForwardTrack.topk_ranked(k = 100), .position_at(4096 ids), .sample(S = 65536, into device memory). Device ms: events
             around the first and the last kernel of the library call (dppr_debug_query_ms, profiling on; the host's reads lie
             between them); wall ms: the call as Python sees it. One warm call of each, then REPEATS calls: the median.
  host       wall ms of the path each call replaces: copy = ftrack_read of the dense p into device memory of the caller and from
             there to the host; then, in numpy over p and the out-rows, per column: score = p * (outdeg + 1) with the seeds and
             their out-neighbours set to 0; top = np.argpartition + a sort of the 100; position = a sort of the qualifying scores
             and np.searchsorted for the 4096 ids (ties by id through np.lexsort); sample = np.cumsum + np.searchsorted for 65536
             uniforms (the natural host sampler, not the tree of the definition). read_out_graph is per epoch, not per call: it is
             timed apart. One warm pass, then REPEATS_HOST: the median.
  tiles      once, at m = 16 from the hub, eps 1e-8: the top k with the count / fill tile at its extremes (dppr_debug_ftrack_rank 64
             and 1024), at 256 and at the plan's choice: one warm call, then TILE_REPEATS (30), the median with its spread.

The top k of the two paths is asserted equal (ids and score bits) in the run. A run without a GPU fails (there is no CPU path).
Writes profiles/ftrack_rank_times.md, stamped with the library's build id.

    python tools/ftrack_rank_times.py [--out profiles/ftrack_rank_times.md] [--repeats 5] [--host-repeats 2] [--tile-repeats 30]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dynamicppr_amd import engine as eng, stream as st  # noqa: E402
from tools.fcluster_times import hip_runtime, median  # noqa: E402
from tools.forward_times import stand_in  # noqa: E402

EPSS = (1e-6, 1e-8)
MAX_ROUNDS = 256
WARM = 2
K, N_IDS, S = 100, 4096, 65536
FLAGS = eng.EXCLUDE_SEEDS | eng.EXCLUDE_OUT_NEIGHBOURS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ftrack_rank_times.md"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--tile-repeats", type=int, default=30)
    a = ap.parse_args()

    V, e1, e2, cfg, wl = stand_in("livejournal", WARM)
    e = eng.Engine(V, wl.window, cfg.directed, wl.per_batch)
    ss = st.SlidingStream(V, e1, e2, cfg.directed, wl)
    e.load_window(*ss.serialize_edge_stream())
    for _ in range(WARM):
        assert not ss.stream_updates()
        e.set_batch(*ss.batch_arrays())
        e.slide(*ss.new_arrays())
    e.set_profiling(1)
    hip = hip_runtime()
    d_p, d_ids, d_w = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_p), 8 * V * 16) == 0 and hip.hipMalloc(C.byref(d_ids), 4 * 16 * S) == 0 and hip.hipMalloc(C.byref(d_w), 8 * 16 * S) == 0

    def timed(f):
        t0 = time.perf_counter()
        out = f()
        return out, (time.perf_counter() - t0) * 1e3

    graph_ms = []
    for _ in range(a.repeats + 1):
        (row, col), ms = timed(e.read_out_graph)
        graph_ms.append(ms)
    row = row.astype(np.int64)
    Ed = int(row[-1])
    col = col[:Ed].astype(np.int64)
    d = np.diff(row)
    factor = (d + 1).astype(np.float64)
    live = int(np.count_nonzero(e.id_map() >= 0))
    by_deg = np.lexsort((np.arange(V), -d))
    with_out = by_deg[:int(np.count_nonzero(d > 0))]
    mid = len(with_out) // 2
    rng = np.random.default_rng(64)
    many = [(np.sort(rng.choice(with_out, 64, replace=False)).astype(np.int32), rng.random(64) + 0.05) for _ in range(16)]
    cases = (("hub (d = %d)" % d[by_deg[0]], [int(x) for x in by_deg[:16]]),
             ("median out-degree (d = %d)" % d[with_out[mid]], [int(x) for x in with_out[mid:mid + 16]]), ("64 seeds", many))
    spec = eng.Engine.rank_spec(eng.FACTOR_DEG, exclude=FLAGS)
    ids = np.random.default_rng(7).integers(0, V, N_IDS).astype(np.int32)
    u = np.random.default_rng(8).random(S)

    def dense_p(t, m):
        t.read(dense_p_ptr=d_p.value, dtype=eng.F64, layout=eng.SOURCE_MAJOR)
        p = np.empty((m, V))
        assert hip.hipMemcpy(p.ctypes.data, d_p, 8 * V * m, 2) == 0   # hipMemcpyDeviceToHost
        return p

    def host_scores(p, sets):
        out = []
        for pc, s in zip(p, sets):
            seeds = np.atleast_1d(np.asarray(s if np.isscalar(s) else s[0], dtype=np.int64))
            sc = pc * factor
            sc[seeds] = 0.0
            for v in seeds:
                sc[col[row[v]:row[v + 1]]] = 0.0
            out.append(sc)
        return out

    def host_top(scores):
        res = []
        for sc in scores:
            q = np.flatnonzero(sc > 0.0)
            if len(q) > K:
                q = q[np.argpartition(-sc[q], K - 1)[:K]]
                q = np.flatnonzero(sc >= sc[q].min())   # (every tie of the boundary, then the order decides)
            q = q[np.lexsort((q, -sc[q]))][:K]
            res.append((q.astype(np.int32), sc[q]))
        return res

    def host_positions(scores):
        pos = np.full((N_IDS, len(scores)), -1, dtype=np.int32)
        for i, sc in enumerate(scores):
            q = np.flatnonzero(sc > 0.0)
            order = q[np.lexsort((q, -sc[q]))]
            inv = np.full(V, -1, dtype=np.int32)
            inv[order] = np.arange(len(order), dtype=np.int32)
            pos[:, i] = inv[ids]
        return pos

    def host_sample(scores):
        out = np.empty((len(scores), S), dtype=np.int32)
        for i, sc in enumerate(scores):
            w = np.where(sc > 0.0, sc, 0.0)
            cdf = np.cumsum(w)
            out[i] = np.searchsorted(cdf, u * cdf[-1], side="right") if cdf[-1] > 0 else -1
        return out

    lines, tile_lines = [], []
    for name, pool in cases:
        for eps in EPSS:
            for m in (1, 16):
                sets = pool[:m]
                t = e.ftrack(sets, eps, MAX_ROUNDS)
                dev = {k: [] for k in ("top", "pos", "smp")}
                wall = {k: [] for k in ("top", "pos", "smp")}
                for rep in range(a.repeats + 1):
                    top, w_ = timed(lambda: t.topk_ranked(K, 0.0, spec))
                    dev["top"].append(e.query_ms())
                    wall["top"].append(w_)
                    (pos, cnt), w_ = timed(lambda: t.position_at(ids, spec))
                    dev["pos"].append(e.query_ms())
                    wall["pos"].append(w_)
                    _, w_ = timed(lambda: t.sample(S, spec, device_ptrs=dict(ids=d_ids.value, w=d_w.value)))
                    dev["smp"].append(e.query_ms())
                    wall["smp"].append(w_)
                host = {k: [] for k in ("copy", "score", "top", "pos", "smp")}
                for rep in range(a.host_repeats + 1):
                    p, c = timed(lambda: dense_p(t, m))
                    scores, sc_ms = timed(lambda: host_scores(p, sets))
                    htop, t_ms = timed(lambda: host_top(scores))
                    hpos, p_ms = timed(lambda: host_positions(scores))
                    _, s_ms = timed(lambda: host_sample(scores))
                    for k, v in zip(("copy", "score", "top", "pos", "smp"), (c, sc_ms, t_ms, p_ms, s_ms)):
                        host[k].append(v)
                for (gi, gs), (hi, hs) in zip(top, htop):   # (the two paths agree: ids and score bits)
                    assert np.array_equal(gi, hi) and gs.tobytes() == hs.tobytes(), (name, eps, m)
                assert np.array_equal(pos, hpos), (name, eps, m)
                support = int(max(cnt))
                med = lambda xs: median(xs[1:])
                base = med(host["copy"]) + med(host["score"])
                lines.append(f"| {name} | {eps:g} | {m} | {support} | {med(dev['top']):.3f} | {med(wall['top']):.3f} | {base + med(host['top']):.1f} | "
                             f"{med(dev['pos']):.3f} | {med(wall['pos']):.3f} | {base + med(host['pos']):.1f} | {med(dev['smp']):.3f} | {med(wall['smp']):.3f} | "
                             f"{base + med(host['smp']):.1f} | {med(host['copy']):.1f} | {med(host['score']):.1f} |")
                print(lines[-1], flush=True)
                if name.startswith("hub") and eps == 1e-8 and m == 16:
                    for tile in (64, 256, 0, 1024):
                        e.debug_ftrack_rank(tile)
                        ms = []
                        for rep in range(a.tile_repeats + 1):
                            again = t.topk_ranked(K, 0.0, spec)
                            ms.append(e.query_ms())
                        assert all(np.array_equal(x[0], y[0]) and x[1].tobytes() == y[1].tobytes() for x, y in zip(again, top))
                        plan = 1024 if V >= 1 << 20 else 256
                        tile_lines.append(f"| {tile if tile else 'the plan: %d' % plan} | {-(-V // (tile or plan))} | {median(ms[1:]):.3f} | "
                                          f"{min(ms[1:]):.3f} .. {max(ms[1:]):.3f} |")
                        print(tile_lines[-1], flush=True)
                    e.debug_ftrack_rank(0)
                t.close()
    for ptr in (d_p, d_ids, d_w):
        hip.hipFree(ptr)
    e.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write("# Ranked, position and sample queries over a forward track against the host path: times\n\n")
        fo.write(f"Library build `{eng.build_id()}`. livejournal stand-in, window of {wl.window} edges ({Ed} stored out-edges), V = {V}, {live} vertices hold an "
                 f"id, after the load and {WARM} slides. `tools/ftrack_rank_times.py`: tracks of m = 1 and m = 16 columns per case (max_rounds = {MAX_ROUNDS}); "
                 f"the spec is DPPR_FACTOR_DEG with the seeds and their out-neighbours excluded, min_score 0; top = `dppr_ftrack_topk_ranked` k = {K}, "
                 f"pos = `dppr_ftrack_position_at` with {N_IDS} ids, smp = `dppr_ftrack_sample` S = {S} per column into device memory. One warm call of each, "
                 f"then {a.repeats}: the median. dev = device ms, events around the first and the last kernel of the library call (the host's reads of "
                 "the seeds' row lengths and of the kept rows lie between them); wall = the call as Python sees it, ms. host = wall ms of the path the call "
                 "replaces: the dense copy of p (`ftrack_read` into device memory, then to the host: `copy`), the scores in numpy over p and the out-rows "
                 f"(`score`), and the top k / the positions / the draws in numpy (one warm pass, then {a.host_repeats}: the median); `read_out_graph`, per "
                 f"epoch and not per call, is apart: median {median(graph_ms[1:]):.1f} ms. support = the largest count of qualifying vertices of a column. "
                 "The two paths agree on every top k (ids, score bits) and every position (asserted in the run). No ratio was fixed in advance: the table "
                 "is the result.\n\n")
        fo.write("| start | eps | m | support | top dev | top wall | top host | pos dev | pos wall | pos host | smp dev | smp wall | smp host | host copy | host score |\n")
        fo.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        fo.write("\n".join(lines) + "\n\n")
        fo.write("The count / scan / fill split of the compacted scratch state, top k at m = 16 from the hub, eps 1e-8, device ms by the ids per tile "
                 f"(`dppr_debug_ftrack_rank`), one warm call, then {a.tile_repeats}: the median and the spread:\n\n| tile_rows | tiles | top dev | "
                 "min .. max |\n|---|---|---|---|\n")
        fo.write("\n".join(tile_lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
