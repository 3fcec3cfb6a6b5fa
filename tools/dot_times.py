#!/usr/bin/env python3
"""Times of the dot products over the vertex axis of a source group on the livejournal stand-in, 10-source group, eps = 1e-9,
after the from-scratch solve -- and, in the same run, of the dense route they replace (group_dense plus torch.matmul).

  group_dot_dense_dev   F in {1, 16, 64}, f64 / f32, feature-major / vertex-major, device destination
  group_dot_sparse      one query of 10^3 and of 10^6 entries, ids and weights in host and in device memory
  dense route           torch_bridge.group_dense ([n][V], f64) and torch.matmul(H, D.T), F in {1, 16, 64}

  device ms  events around the first and the last kernel of the library call (dppr_set_profiling, dppr_debug_query_ms)
  call ms    host clock around the Python call, which ends in a synchronisation (of the solver stream; of the device for torch)
Every figure is the median of REPEATS calls after WARMUP calls, with the spread (min .. max). torch is imported first (one HIP
runtime) and provides the device memory. A run without a GPU fails (there is no CPU path). Writes profiles/dot_times.md, stamped
with the library's build id.

    python tools/dot_times.py [--out profiles/dot_times.md] [--repeats 15] [--warmup 3]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the library: dynamicppr_amd/torch_bridge.py, the loading rule)

from dynamicppr_amd import datagen, engine as eng, stream as st, torch_bridge as tb  # noqa: E402

DATA = "/tmp/dppr_data"
EPS = 1e-9
N_SOURCES = 10
FS = (1, 16, 64)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dot_times.md"))
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    reps = a.warmup + a.repeats

    V, e1, e2, cfg, wl = stand_in("livejournal")
    sources = [int(x) for x in datagen.ranked_sources(V, e1, e2, wl.window, cfg.directed, N_SOURCES, 1000, 10)]
    e = eng.Engine(V, wl.window, cfg.directed, wl.per_batch)
    ss = st.SlidingStream(V, e1, e2, cfg.directed, wl)
    e.load_window(*ss.serialize_edge_stream())
    gid = e.add_source_group(sources)
    e.group_init_solve(gid, EPS)
    e.set_profiling(1)
    dev = torch.device("cuda", e.device)
    sp = e.id_space()
    rows = sp["ids"] + sp["parked"]
    lines = []

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

    gen = torch.Generator(device=dev).manual_seed(5)
    dense_ms = {}
    for F in FS:
        H64 = torch.randn((F, V), dtype=torch.float64, device=dev, generator=gen)
        out = torch.empty((F, N_SOURCES), dtype=torch.float64, device=dev)

        def route():
            D = tb.group_dense(e, gid, "p", torch.float64, "source_major")
            r = torch.matmul(H64, D.T)
            torch.cuda.synchronize(dev)
            return r

        ref = route()
        for tdt, dtype, name in ((torch.float64, eng.F64, "f64"), (torch.float32, eng.F32, "f32")):
            H = H64.to(tdt)
            for layout, lname in ((eng.H_FEATURE_MAJOR, "feature-major"), (eng.H_VERTEX_MAJOR, "vertex-major")):
                Hl = H if layout == eng.H_FEATURE_MAJOR else H.T.contiguous()
                torch.cuda.synchronize(dev)
                moved = V * (H.element_size() * F + 4) + rows * 128 * -(-F // 16)
                ms = timed(f"group_dot_dense_dev, F = {F}, {name}, {lname}",
                           lambda: e.group_dot_dense_dev(gid, Hl.data_ptr(), F, eng.DENSE_P, dtype, layout, out_ptr=out.data_ptr()),
                           f"{moved / 1e6:.1f} MB by the byte count of DESIGN 9f")
                dense_ms[(F, name, lname)] = (ms, moved)
                if tdt == torch.float64:  # the two routes agree to rounding (the orders of the sums differ)
                    assert torch.allclose(out, ref, rtol=1e-9, atol=1e-12), (F, lname)
        timed(f"dense route: group_dense + torch.matmul, F = {F}", route, f"{8 * N_SOURCES * V / 1e6:.1f} MB written and read back", device=False)
        del H64, H, Hl, out, ref
    rng = np.random.default_rng(6)
    for m in (10 ** 3, 10 ** 6):
        ids = rng.integers(0, V, m).astype(np.int32)
        w = rng.standard_normal(m)
        off = np.array([0, m], dtype=np.int64)
        timed(f"group_dot_sparse, one query of {m} entries, host", lambda: e.group_dot_sparse(gid, off, ids, w), "ids and weights uploaded by the call")
        d_ids, d_w = torch.from_numpy(ids).to(dev), torch.from_numpy(w).to(dev)
        torch.cuda.synchronize(dev)
        timed(f"group_dot_sparse, one query of {m} entries, device", lambda: e.group_dot_sparse_dev(gid, off, d_ids.data_ptr(), d_w.data_ptr()))
        del d_ids, d_w
    fills = eng.bench_line_fills()
    copy = eng.bench_stream_copy()
    e.close()
    copy_gbs = 2 * (1 << 30) / copy / 1e6
    ms16, moved16 = dense_ms[(16, "f64", "feature-major")]

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# The sources scored under seed distributions (`dppr_group_dot_dense_dev`, `dppr_group_dot_sparse`): times\n\n")
        f.write(f"Library build `{eng.build_id()}`. livejournal stand-in, window of {wl.window} edges, V = {V}, {rows} rows hold a "
                f"vertex; {N_SOURCES}-source group (rows of 16 doubles), eps = {EPS:g}, after the from-scratch solve. `tools/dot_times.py`: "
                f"median (min .. max) in ms over {a.repeats} calls after {a.warmup} warm-up calls. Device time: events around the first and the "
                "last kernel of the library call (the zeroing of the partials included); call time: host clock around the Python call (each "
                "ends in a synchronisation). In the same process: "
                f"2^26 random 128-B line fills out of 1 GiB take {fills:.3f} ms ({(1 << 26) / fills / 1e6:.1f} G lines/s), a stream copy of 1 GiB "
                f"takes {copy:.3f} ms ({copy_gbs:.0f} GB/s read + write).\n\n")
        f.write(f"Against the expectation of DESIGN 9f: F = 16, f64, feature-major moves {moved16 / 1e6:.1f} MB by the byte count there in "
                f"{ms16:.3f} ms, {moved16 / ms16 / 1e6:.0f} GB/s, {100 * moved16 / ms16 / 1e6 / copy_gbs:.0f} % of the stream-copy rate "
                "(expected: no less than 50 %).\n\n")
        f.write("| route | device ms | call ms | note |\n|---|---|---|---|\n")
        f.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
