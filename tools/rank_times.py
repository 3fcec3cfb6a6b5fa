#!/usr/bin/env python3
"""Times of the ranked query of a source group (Engine.group_topk_ranked) on the livejournal stand-in, 10-source group,
eps = 1e-9, after the from-scratch solve, k = 100 -- and, in the same run, of the yardstick this change does not touch:
Engine.group_topk at the same k.

Four shapes:
  group_topk                      the plain query (code untouched by the ranked queries)
  ranked, NULL spec               the same order through the scratch state: one more streaming pass
  ranked, DEG + all exclusions    degrees from out_row_ptr, the seeds' rows marked (one read of their lengths by the host)
  ranked, DEV f64 + deny mask     one gather of 8 bytes and one of 1 byte per row, by external id
Per shape:
  device ms  events around the first and the last kernel of the query (dppr_set_profiling, dppr_debug_query_ms)
  call ms    host clock around the Python call, which ends in a synchronisation of the solver stream
Every figure is the median of REPEATS calls after WARMUP calls of the same shape, with the spread (min .. max); the four
shapes alternate inside one repeat. A run without a GPU fails (there is no CPU path). Writes profiles/rank_times.md, stamped
with the library's build id.

    python tools/rank_times.py [--out profiles/rank_times.md] [--repeats 15] [--warmup 3]
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
K = 100


def stand_in(key):
    cfg = datagen.STAND_INS[key]
    f = cfg.flags.split()
    opt = {f[i]: f[i + 1] for i in range(0, len(f), 2)}
    wl = st.workload_config(cfg.edges, 0.1, int(opt.get("-n", 0)), float(opt.get("-r", -1.0)), int(opt.get("-b", 0)),
                            int(opt.get("-c", 0)), int(opt.get("-l", 0)))
    V, e1, e2, _ = datagen.stand_in_stream(key, DATA, limit=wl.window + wl.per_batch)
    return V, e1, e2, cfg, wl


def device_copy(a):
    """A host array in device memory of the runtime the library brought in: (address, free)."""
    eng.lib()
    paths = {l.rsplit(" ", 1)[-1].strip() for l in open("/proc/self/maps") if "libamdhip64" in l}
    assert len(paths) == 1, paths
    hip = C.CDLL(paths.pop())
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    a = np.ascontiguousarray(a)
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), a.nbytes) == 0
    assert hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0  # hipMemcpyHostToDevice
    return p.value, lambda: hip.hipFree(p)


def summary(xs):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} .. {max(xs):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_times.md"))
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
    g = rng.random(V) + 0.5
    deny = (rng.random(V) < 0.5).astype(np.uint8)
    d_g, free_g = device_copy(g)
    d_deny, free_deny = device_copy(deny)
    spec = eng.Engine.rank_spec
    everything = eng.EXCLUDE_SEEDS | eng.EXCLUDE_IN_NEIGHBOURS | eng.EXCLUDE_OUT_NEIGHBOURS
    shapes = [("group_topk (10 lanes)", lambda: e.group_topk(gid, K)),
              ("ranked, NULL spec", lambda: e.group_topk_ranked(gid, K)),
              ("ranked, DEG + seeds, in and out neighbours", lambda: e.group_topk_ranked(gid, K, 0.0, spec(eng.FACTOR_DEG, exclude=everything))),
              ("ranked, DEV f64 + deny mask", lambda: e.group_topk_ranked(gid, K, 0.0, spec(eng.FACTOR_DEV, d_g, eng.F64, eng.MASK_DENY, d_deny)))]
    # the anchor holds here too, before anything is timed
    plain, ranked = shapes[0][1](), shapes[1][1]()
    for (pi, pp, _), (ri, rs) in zip(plain, ranked):
        assert np.array_equal(pi, ri) and np.array_equal(pp.view(np.uint64), rs.view(np.uint64))
    t = {name: ([], []) for name, _ in shapes}
    for rep in range(a.warmup + a.repeats):
        for name, call in shapes:
            t0 = time.perf_counter()
            call()
            t1 = time.perf_counter()
            dev = e.query_ms()
            if rep >= a.warmup:
                t[name][0].append(dev)
                t[name][1].append((t1 - t0) * 1e3)
    lines = [f"| {name} | {summary(t[name][0])} | {summary(t[name][1])} |" for name, _ in shapes]
    print("\n".join(lines), flush=True)
    e.close()
    free_g()
    free_deny()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# Ranked query of a source group: times\n\n")
        f.write(f"Library build `{eng.build_id()}`. livejournal stand-in, window of {wl.window} edges, V = {V}, {rows} rows hold a vertex; "
                f"{N_SOURCES}-source group, eps = {EPS:g}, after the from-scratch solve, k = {K}. `tools/rank_times.py`: median "
                f"(min .. max) in ms over {a.repeats} calls after {a.warmup} warm-up calls, the four shapes alternating inside a repeat. "
                "Device time: events around the first and the last kernel of a query (with neighbour flags the host's read of the "
                "seeds' row lengths lies between them); call time: host clock around the Python call (ends in a stream "
                "synchronisation; allocation of the outputs and the copy back included). One box, one run.\n\n")
        f.write("| shape | device | call |\n|---|---|---|\n")
        f.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
