#!/usr/bin/env python3
"""Times of the exports of a source group on the livejournal stand-in, 10-source group, eps = 1e-9, after the from-scratch
solve -- and, in the same run, of the dense route they replace (group_read of the ten sources plus the numpy filter).

  group_support                                   min_p = 1e-6
  group_export_sparse   min_p in {1e-4, 1e-6, 0}  host destination (size call + fill, as Engine.group_export_sparse makes them)
                                                  and device destination (the fill alone, into memory of exactly the count)
  group_export_dense_dev  f64 / f32, vertex-major / source-major
  dense route           ten group_reads, np.nonzero(p > min_p) and the values per source

  device ms  events around the first and the last kernel of the LAST library call of the route (dppr_set_profiling,
             dppr_debug_query_ms): for a host export that is the fill
  call ms    host clock around the Python call(s), which end in a synchronisation of the solver stream
Every figure is the median of REPEATS calls after WARMUP calls, with the spread (min .. max). torch is imported first (one HIP
runtime) and provides the device memory. A run without a GPU fails (there is no CPU path). Writes profiles/export_times.md,
stamped with the library's build id.

    python tools/export_times.py [--out profiles/export_times.md] [--repeats 15] [--warmup 3]
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


def summary(xs):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} .. {max(xs):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "export_times.md"))
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
    lines = []

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

    def dense_route(min_p):
        out = []
        for i in range(N_SOURCES):
            p = e.group_read(gid, i)[0]
            ids = np.nonzero(p > min_p)[0]
            out.append((ids.astype(np.int32), p[ids]))
        return out

    timed("group_support, min_p 1e-6", lambda: e.group_support(gid, 1e-6))
    for min_p in (1e-4, 1e-6, 0.0):
        total = int(e.group_support(gid, min_p).sum())
        off, ids, p = e.group_export_sparse(gid, min_p)
        want = dense_route(min_p)
        for i, (wi, wp) in enumerate(want):  # the two routes agree bit for bit
            assert np.array_equal(ids[off[i]:off[i + 1]], wi) and np.array_equal(p[off[i]:off[i + 1]].view(np.uint64), wp.view(np.uint64))
        timed(f"group_export_sparse, host, min_p {min_p:g}", lambda: e.group_export_sparse(gid, min_p), f"{total} entries; size call + fill")
        d_ids = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        d_p = torch.empty(max(total, 1), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        timed(f"group_export_sparse, device, min_p {min_p:g}", lambda: e.group_export_sparse_dev(gid, min_p, total, d_ids.data_ptr(), d_p.data_ptr()),
              f"{total} entries; the fill alone")
        assert np.array_equal(d_ids[:total].cpu().numpy(), ids)
        t = []
        for rep in range(reps):
            t0 = time.perf_counter()
            dense_route(min_p)
            if rep >= a.warmup:
                t.append((time.perf_counter() - t0) * 1e3)
        lines.append(f"| dense route (10 group_reads + numpy filter), min_p {min_p:g} | - | {summary(t)} | {total} entries |")
        print(lines[-1], flush=True)
        del d_ids, d_p
    for dtype, tdt, name in ((eng.F64, torch.float64, "f64"), (eng.F32, torch.float32, "f32")):
        for layout, lname in ((eng.VERTEX_MAJOR, "vertex-major"), (eng.SOURCE_MAJOR, "source-major")):
            dst = torch.empty(N_SOURCES * V, dtype=tdt, device=dev)
            torch.cuda.synchronize(dev)
            timed(f"group_export_dense_dev, {name}, {lname}", lambda: e.group_export_dense_dev(gid, dst.data_ptr(), eng.DENSE_P, dtype, layout),
                  f"{dst.numel() * dst.element_size() / 1e6:.1f} MB written")
            del dst
    fills = eng.bench_line_fills()
    copy = eng.bench_stream_copy()
    e.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# The exports of a source group (`dppr_group_support`, `dppr_group_export_sparse`, `dppr_group_export_dense_dev`): times\n\n")
        f.write(f"Library build `{eng.build_id()}`. livejournal stand-in, window of {wl.window} edges, V = {V}, {sp['ids'] + sp['parked']} rows hold a "
                f"vertex; {N_SOURCES}-source group (rows of 16 doubles), eps = {EPS:g}, after the from-scratch solve. `tools/export_times.py`: "
                f"median (min .. max) in ms over {a.repeats} calls after {a.warmup} warm-up calls. Device time: events around the first and the "
                "last kernel of the last library call of the route; call time: host clock around the Python call(s) (each ends in a stream "
                "synchronisation; allocation of numpy outputs and the copy back included). In the same process: "
                f"2^26 random 128-B line fills out of 1 GiB take {fills:.3f} ms ({(1 << 26) / fills / 1e6:.1f} G lines/s), a stream copy of 1 GiB "
                f"takes {copy:.3f} ms ({2 * (1 << 30) / copy / 1e6:.0f} GB/s read + write).\n\n")
        f.write("| route | device ms | call ms | note |\n|---|---|---|---|\n")
        f.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
