#!/usr/bin/env python3
"""What the full-length conductance sweep of a forward track costs on the device (dppr_ftrack_cluster) against the host path a caller
had before it: the dense p of the track copied to the host, dppr_read_out_graph, and the sweep in numpy -- on the livejournal
stand-in (BASELINE.json configs[2]), all in one session.

  cases      three start sets -- the hub (largest out-degree), a vertex of median out-degree among those with an out-edge, and a
             64-seed set -- at eps in {1e-6, 1e-7, 1e-8}, max_rounds = 256. Each case is a track of one column, created after the
             load and WARM slides; the sweep is by p / (outdeg + 1), min_score 0, the whole support.
  device     ForwardTrack.cluster, the records alone (cap = 0: nothing but 40 bytes per column comes back). Device ms: events
             around the first and the last kernel of the library call (dppr_debug_query_ms, profiling on; the one read of the
             counts lies between them); wall ms: the call as Python sees it. One warm call, then REPEATS calls: the median.
  host       wall ms of: the dense copy of p into device memory of the caller and from there to the host; read_out_graph; the
             order by np.lexsort and tests/cluster_ref.prefix_arrays; the best prefix vectorised in numpy (cluster_ref.best is a
             Python loop over the positions: its time would say nothing). Each part is listed; the graph read is per epoch, not per
             track, and is listed apart. One warm pass, then REPEATS: the median.

A run without a GPU fails (there is no CPU path). Writes profiles/fcluster_times.md, stamped with the library's build id.

    python tools/fcluster_times.py [--out profiles/fcluster_times.md] [--repeats 5]
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
from tests import cluster_ref as cr  # noqa: E402
from tests import fcluster_ref as fcr  # noqa: E402
from tools.forward_times import stand_in  # noqa: E402

EPSS = (1e-6, 1e-7, 1e-8)
MAX_ROUNDS = 256
WARM = 2


def hip_runtime():
    eng.lib()
    paths = {l.rsplit(" ", 1)[-1].strip() for l in open("/proc/self/maps") if "libamdhip64" in l}
    assert len(paths) == 1, paths
    hip = C.CDLL(paths.pop())
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


def best_numpy(cut_out, vol, Ed, min_size=1):
    """cluster_ref.best, vectorised: the first minimum of cut_out / min(vol, Ed - vol) over the eligible prefixes."""
    den = np.minimum(vol, Ed - vol)
    ok = (den > 0) & (np.arange(len(vol)) + 1 >= min_size)
    if not ok.any():
        return dict(count=len(vol), best_size=0, best_cut=0, best_vol=0, best_phi=float("inf"))
    phi = np.full(len(vol), np.inf)
    phi[ok] = cut_out[ok].astype(np.float64) / den[ok].astype(np.float64)
    j = int(np.flatnonzero(ok & (phi == phi[ok].min()))[0])
    return dict(count=len(vol), best_size=j + 1, best_cut=int(cut_out[j]), best_vol=int(vol[j]), best_phi=float(phi[j]))


def median(xs):
    return float(np.median(np.asarray(xs)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fcluster_times.md"))
    ap.add_argument("--repeats", type=int, default=5)
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
    d_p = C.c_void_p()
    assert hip.hipMalloc(C.byref(d_p), 8 * V) == 0

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
    live = int(np.count_nonzero(e.id_map() >= 0))
    by_deg = np.lexsort((np.arange(V), -d))
    with_out = by_deg[:int(np.count_nonzero(d > 0))]
    rng = np.random.default_rng(64)
    many = (np.sort(rng.choice(with_out, 64, replace=False)).astype(np.int32), rng.random(64) + 0.05)
    cases = (("hub (d = %d)" % d[by_deg[0]], int(by_deg[0])), ("median out-degree (d = %d)" % d[with_out[len(with_out) // 2]], int(with_out[len(with_out) // 2])),
             ("64 seeds", many))

    def dense_p(t):
        t.read(dense_p_ptr=d_p.value, dtype=eng.F64, layout=eng.SOURCE_MAJOR)
        p = np.empty(V)
        assert hip.hipMemcpy(p.ctypes.data, d_p, 8 * V, 2) == 0   # hipMemcpyDeviceToHost
        return p

    def host_sweep(p):
        ids, _ = fcr.ordered(p, row, col, "deg")
        co, _, vol = cr.prefix_arrays(V, row, col, ids)
        return best_numpy(co, vol, Ed)

    lines = []
    for name, s in cases:
        for eps in EPSS:
            t = e.ftrack([s], eps, MAX_ROUNDS)
            dev_ms, wall_ms, copy_ms, sweep_ms = [], [], [], []
            for rep in range(a.repeats + 1):
                got, w = timed(lambda: t.cluster("deg")[0])
                dev_ms.append(e.query_ms())
                wall_ms.append(w)
                p, c = timed(lambda: dense_p(t))
                want, sw = timed(lambda: host_sweep(p))
                copy_ms.append(c)
                sweep_ms.append(sw)
                assert got == want, (name, eps, got, want)   # (the two paths agree, the conductance to the bit)
            dev, wall, cp, sw = median(dev_ms[1:]), median(wall_ms[1:]), median(copy_ms[1:]), median(sweep_ms[1:])
            host = cp + sw
            lines.append(f"| {name} | {eps:g} | {int(t.created['rounds_used'][0])} / {int(t.created['converged'][0])} | {got['count']} | {got['best_size']} | "
                         f"{got['best_phi']:.6g} | {dev:.3f} | {wall:.3f} | {cp:.3f} | {sw:.3f} | {host:.3f} | {host / wall:.1f} |")
            print(lines[-1], flush=True)
            t.close()
    hip.hipFree(d_p)
    e.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write("# The full-length conductance sweep of a forward track (`dppr_ftrack_cluster`) against the host path: times\n\n")
        fo.write(f"Library build `{eng.build_id()}`. livejournal stand-in, window of {wl.window} edges ({Ed} stored out-edges), V = {V}, {live} vertices hold an "
                 f"id, after the load and {WARM} slides. `tools/fcluster_times.py`: a track of one column per case (max_rounds = {MAX_ROUNDS}), order by "
                 f"p / (outdeg + 1), min_score 0, max_len 0 (the whole support L), the records alone. One warm call of each kind, then {a.repeats}: the "
                 "median. device ms = events around the first and the last kernel of the library call, the one read of the counts inside; wall ms = the "
                 "call as Python sees it. Host path, wall ms: copy = the dense p of the track into the caller's device memory and to the host; sweep = "
                 "np.lexsort + tests/cluster_ref.prefix_arrays + the first minimum in numpy; the graph read (`read_out_graph`, per epoch, not per track) "
                 f"is listed apart: median {median(graph_ms[1:]):.3f} ms. host = copy + sweep; ratio = host / device wall. The two paths agree on every "
                 "record, the conductance to the bit (asserted in the run).\n\n")
        fo.write("| start | eps | create rounds / converged | support L | best size | best phi | device ms | device wall ms | host copy ms | host sweep ms | "
                 "host ms | ratio |\n")
        fo.write("|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        fo.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
