#!/usr/bin/env python3
"""Times of the subgraph a top-k order induces (dppr_group_subgraph) on the livejournal stand-in, 10-source group, eps = 1e-9, after
the from-scratch solve -- and, in the same run and on the same state, of dppr_group_cluster and dppr_group_topk at the same k and of
the host route the call replaces.

  group_subgraph  k in {1024, 8192}, min_p = 0: the size query (cap = 0), and the fill into device memory (DPPR_DEST_DEVICE, cap =
                  the entries), the fill once per setting of dppr_debug_subgraph_wave_max in WAVE_MAXES (0: every row by the
                  histogram kernel) -- the crossover between the two fill kernels is chosen from these lines
  group_cluster   the same k, the records alone
  group_topk      the same k
  host route      group_topk + read_out_graph + the numpy filter of tests/subgraph_ref.py in vectorised form: host clock alone

  device ms  events around the first and the last kernel of the library call (dppr_set_profiling, dppr_debug_query_ms); for the
             fill this spans the one read of the counts by the host that lies between the scan and the fill
  call ms    host clock around the Python call, which ends in a synchronisation of the solver stream
Every figure is the median of REPEATS calls after WARMUP calls, with the spread (min .. max). Also counted, from the result: the
subgraph's edges per source, how many rows hold more than 64 / 128 / 256 entries of the order, how many are longer than CL_SPLIT
stored entries, and with them how many rows the histogram kernel places at the default setting; and the bytes each route moves to or
from the host. The stand-in's rows hold few entries of an order, so the crossover is timed on a second shape: CLIQUES disjoint complete
directed graphs of M + 1 vertices, one source in each, where every row holds exactly M entries of its order -- the fill with every
row placed by its wave (wave_max = 256) against every row placed by the histogram kernel (wave_max = 0), for M in CLIQUE_MS. A run
without a GPU fails (there is no CPU path). Writes profiles/subgraph_times.md, stamped with the library's build id.

    python tools/subgraph_times.py [--out profiles/subgraph_times.md] [--repeats 15] [--warmup 3]
"""
import argparse
import ctypes as C
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
CL_SPLIT = 2048   # dynamicppr_amd/csrc/dppr_cluster_plan.hpp
SG_WAVE_MAX = 256  # dynamicppr_amd/csrc/dppr_subgraph_plan.hpp: the default of dppr_debug_subgraph_wave_max
WAVE_MAXES = (256, 128, 64, 0)
CLIQUES = 10
CLIQUE_MS = (32, 64, 96, 128, 192, 256)


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


def device_alloc(nbytes):
    """Device memory from the HIP runtime the library is linked to (no second runtime is loaded)."""
    eng.lib()
    paths = {l.rsplit(" ", 1)[-1].strip() for l in open("/proc/self/maps") if "libamdhip64" in l}
    assert len(paths) == 1, paths
    hip = C.CDLL(paths.pop())
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), max(int(nbytes), 8)) == 0
    return p.value


def host_route(e, gid, k, V):
    """What a caller without the call does: the orders, the whole out-CSR to the host, the filter in numpy."""
    tops = e.group_topk(gid, k)
    row, col = e.read_out_graph()
    row = row.astype(np.int64)
    out = []
    for ids, _, _ in tops:
        pos = np.full(V, -1, dtype=np.int32)
        pos[ids] = np.arange(len(ids), dtype=np.int32)
        lens = row[ids + 1] - row[ids]
        at = np.repeat(row[ids] - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens) + np.arange(int(lens.sum()))
        tail, head = np.repeat(np.arange(len(ids), dtype=np.int32), lens), pos[col[at]]
        keep = head >= 0
        tail, head = tail[keep], head[keep]
        o = np.lexsort((head, tail))
        out.append((np.concatenate([[0], np.cumsum(np.bincount(tail, minlength=len(ids)))]), head[o]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subgraph_times.md"))
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
    w1 = np.asarray(a1, dtype=np.int64)
    if not cfg.directed:
        w1 = np.concatenate([w1, np.asarray(a2, dtype=np.int64)])
    outdeg = np.bincount(w1, minlength=V)
    Ed = len(w1)
    lines, counts = [], []

    def timed(name, fn, note="", device=True):
        d, c = [], []
        for rep in range(reps):
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            if rep >= a.warmup:
                d.append(e.query_ms())
                c.append((t1 - t0) * 1e3)
        lines.append(f"| {name} | {summary(d) if device else '-'} | {summary(c)} | {note} |")
        print(lines[-1], flush=True)
        return statistics.median(d)

    for k in KS:
        cnt, off, ids, p, row_ptr, col = e.group_subgraph(gid, k)
        total = int(off[N_SOURCES])
        want = host_route(e, gid, k, V)
        for i in range(N_SOURCES):  # (the two routes give the same CSR)
            L = int(cnt[i])
            assert np.array_equal(row_ptr[i, :L + 1] - off[i], want[i][0]) and np.array_equal(col[off[i]:off[i + 1]], want[i][1]), i
        m = np.concatenate([np.diff(row_ptr[i, :int(cnt[i]) + 1]) for i in range(N_SOURCES)])
        lens = np.concatenate([outdeg[ids[i, :int(cnt[i])]] for i in range(N_SOURCES)])
        long_rows = int(np.sum((m > 0) & ((lens > CL_SPLIT) | (m > SG_WAVE_MAX))))
        counts.append(f"k = {k}: the {N_SOURCES} orders hold {int(cnt.sum())} vertices and {int(lens.sum())} out-row entries; the subgraphs hold "
                      f"{total} edges ({', '.join(str(int(x)) for x in np.diff(off))} per source); rows with more than 64 / 128 / 256 entries of "
                      f"the order: {int(np.sum(m > 64))} / {int(np.sum(m > 128))} / {int(np.sum(m > 256))}, the longest {int(m.max())}; rows longer than "
                      f"{CL_SPLIT} stored entries: {int(np.sum(lens > CL_SPLIT))}; rows placed by the histogram kernel at the default "
                      f"({SG_WAVE_MAX}): {long_rows} of {int(np.sum(m > 0))} that hold an entry.")
        print(counts[-1], flush=True)
        d_ids, d_p = device_alloc(4 * N_SOURCES * k), device_alloc(8 * N_SOURCES * k)
        d_rp, d_col = device_alloc(8 * N_SOURCES * (k + 1)), device_alloc(4 * total)
        timed(f"group_subgraph, k = {k}, the size query", lambda: e.group_subgraph_dev(gid, k, 0.0, 0, None, None, None, None),
              "136 B of offsets and 64 B of counts to the host")
        t_sg = None
        for wm in WAVE_MAXES:
            e.set_subgraph_wave_max(wm)
            t = timed(f"group_subgraph, k = {k}, the fill to the device, wave_max = {wm}",
                      lambda: e.group_subgraph_dev(gid, k, 0.0, total, d_ids, d_p, d_rp, d_col),
                      f"{(12 * N_SOURCES * k + 8 * N_SOURCES * (k + 1) + 4 * total) / 1e6:.2f} MB written in place, 200 B to the host")
            t_sg = t if t_sg is None else t_sg
        e.set_subgraph_wave_max(SG_WAVE_MAX)
        t_cl = timed(f"group_cluster, k = {k}, records alone", lambda: e.group_cluster(gid, k))
        t_tk = timed(f"group_topk, k = {k}", lambda: e.group_topk(gid, k), f"{20 * N_SOURCES * k / 1e6:.2f} MB copied back")
        timed(f"host route, k = {k}: group_topk + read_out_graph + numpy filter", lambda: host_route(e, gid, k, V),
              f"{(4 * Ed + 4 * (V + 1) + 20 * N_SOURCES * k) / 1e6:.1f} MB to the host, {4 * total / 1e6:.2f} MB of col back to the device", device=False)
        lines.append(f"| k = {k} | - | - | the fill adds {t_sg - t_tk:.3f} ms of device time to the selection, the conductance sweep {t_cl - t_tk:.3f} ms |")
    e.close()

    # the crossover between the two fill kernels: rows of exactly M entries of the order
    for M in CLIQUE_MS:
        size = M + 1
        u, w = np.divmod(np.arange(size * size), size)
        keep = u != w
        c1 = np.concatenate([u[keep] + q * size for q in range(CLIQUES)]).astype(np.int32)
        c2 = np.concatenate([w[keep] + q * size for q in range(CLIQUES)]).astype(np.int32)
        e = eng.Engine(CLIQUES * size, len(c1), 1, 1)
        e.load_window(c1, c2)
        gid = e.add_source_group([q * size for q in range(CLIQUES)])
        e.group_init_solve(gid, EPS)
        e.set_profiling(1)
        k = 8192
        cnt, off, ids, p, row_ptr, col = e.group_subgraph(gid, k)
        total = int(off[CLIQUES])
        assert np.all(cnt == size) and total == CLIQUES * size * M and all(np.all(np.diff(row_ptr[i, :size + 1]) == M) for i in range(CLIQUES))
        d_col, d_rp = device_alloc(4 * total), device_alloc(8 * CLIQUES * (k + 1))
        t = {}
        for wm in (256, 0):
            e.set_subgraph_wave_max(wm)
            t[wm] = timed(f"cliques, {CLIQUES} x {size} rows of {M} entries, the fill, wave_max = {wm}",
                          lambda: e.group_subgraph_dev(gid, k, 0.0, total, None, None, d_rp, d_col), "every row by " + ("its wave" if wm else "the histogram kernel"))
        lines.append(f"| rows of {M} entries | - | - | by waves {t[256] - t[0]:+.3f} ms against the histogram kernel, {CLIQUES * size} rows |")
        e.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# The subgraph around the tracked sources (`dppr_group_subgraph`): times\n\n")
        f.write(f"Library build `{eng.build_id()}`. livejournal stand-in, window of {wl.window} edges ({Ed} stored), V = {V}, {rows} rows "
                f"hold a vertex; {N_SOURCES}-source group (rows of 16 doubles), eps = {EPS:g}, after the from-scratch solve. "
                f"`tools/subgraph_times.py`: median (min .. max) in ms over {a.repeats} calls after {a.warmup} warm-up calls. Device time: events "
                "around the first and the last kernel of the library call (the clearing of the rank table and, for the fill, the one read of "
                "the counts by the host included); call time: host clock around the Python call (each ends in a synchronisation).\n\n")
        f.write("\n\n".join(counts) + "\n\n")
        f.write("| route | device ms | call ms | note |\n|---|---|---|---|\n")
        f.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
