#!/usr/bin/env python3
"""What a patch costs: dppr_group_patch against the way of before, on the livejournal stand-in, 10-source group, eps = 1e-9, as
the per-batch feed (min_p = 1e-6, min_delta = 0, the emitted-only re-mark): every repeat takes one more batch (untimed), then
the routes below; after that the patch alone over as many batches with min_delta = 1e-8, and again with 1e-6.

  patch            the size call and the sized call to the host, as Engine.group_patch makes them
  export + diff    what it replaces: group_export_sparse(min_p) to the host and the numpy diff against the previous export
  export, device   group_export_sparse(min_p) into device memory of exactly the count: the fill alone

  device ms  events around the first and the last kernel of ONE library call (dppr_set_profiling, dppr_debug_query_ms)
  call ms    host clock around the Python call(s), which end in a synchronisation of the solver stream
Every repeat checks that the patch IS the diff of the two exports (min_delta = 0: the replica is exact), bit for bit. Every figure
is the median of REPEATS repeats after WARMUP warm batches, with the spread (min .. max). torch is imported first (one HIP runtime)
and provides the device memory. A run without a GPU fails (there is no CPU path). Writes profiles/patch_times.md, stamped with
the library's build id.

    python tools/patch_times.py [--out profiles/patch_times.md] [--repeats 25] [--warmup 3]
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

import torch  # noqa: E402  (before the library: dynamicppr_amd/torch_bridge.py, the loading rule)

from dynamicppr_amd import datagen, engine as eng, stream as st  # noqa: E402

DATA = "/tmp/dppr_data"
EPS = 1e-9
N_SOURCES = 10
MIN_P = 1e-6
DELTAS = (1e-8, 1e-6)


def stand_in(key, n_batches):
    cfg = datagen.STAND_INS[key]
    f = cfg.flags.split()
    opt = {f[i]: f[i + 1] for i in range(0, len(f), 2)}
    wl = st.workload_config(cfg.edges, 0.1, int(opt.get("-n", 0)), float(opt.get("-r", -1.0)), int(opt.get("-b", 0)),
                            int(opt.get("-c", 0)), int(opt.get("-l", 0)))
    V, e1, e2, _ = datagen.stand_in_stream(key, DATA, limit=wl.window + (1 + n_batches) * wl.per_batch)
    return V, e1, e2, cfg, wl


def diff_route(old, new):
    """The patch that takes the export `old` to the export `new`, by numpy: per lane, the ids of `new` that `old` lacks or holds with
    other bits, and the ids of `old` that `new` lacks."""
    n = len(old[0]) - 1
    uo, do = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
    ui, up, di = [], [], []
    for i in range(n):
        oi, op = old[1][old[0][i]:old[0][i + 1]], old[2][old[0][i]:old[0][i + 1]]
        ni, np_ = new[1][new[0][i]:new[0][i + 1]], new[2][new[0][i]:new[0][i + 1]]
        at = np.searchsorted(oi, ni)
        at[at == len(oi)] = 0
        held = (oi[at] == ni) if len(oi) else np.zeros(len(ni), dtype=bool)
        same = held & (op[at].view(np.uint64) == np_.view(np.uint64)) if len(oi) else held
        ui.append(ni[~same])
        up.append(np_[~same])
        di.append(oi[~np.isin(oi, ni, assume_unique=True)])
        uo[i + 1], do[i + 1] = uo[i] + len(ui[-1]), do[i] + len(di[-1])
    return {"up_offsets": uo, "up_ids": np.concatenate(ui), "up_p": np.concatenate(up), "del_offsets": do, "del_ids": np.concatenate(di)}


def summary(xs):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} .. {max(xs):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patch_times.md"))
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    reps = a.warmup + a.repeats

    V, e1, e2, cfg, wl = stand_in("livejournal", (1 + len(DELTAS)) * reps)
    sources = [int(x) for x in datagen.ranked_sources(V, e1, e2, wl.window, cfg.directed, N_SOURCES, 1000, 10)]
    e = eng.Engine(V, wl.window, cfg.directed, wl.per_batch)
    ss = st.SlidingStream(V, e1, e2, cfg.directed, wl)
    e.load_window(*ss.serialize_edge_stream())
    gid = e.add_source_group(sources)
    e.group_init_solve(gid, EPS)
    dev = torch.device("cuda", e.device)
    L, n = eng.lib(), N_SOURCES
    i64p = C.POINTER(C.c_int64)

    def batch():
        assert not ss.stream_updates()
        e.set_batch(*ss.batch_arrays())
        e.slide(*ss.new_arrays())
        e.group_update(gid, EPS)

    def patch_two_calls(delta=0.0):
        """Engine.group_patch with the device time of either call read in between."""
        uo, do = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
        out = eng.PatchOut(uo.ctypes.data_as(i64p), None, None, do.ctypes.data_as(i64p), None, -1)
        assert L.dppr_group_patch(e._h, gid, MIN_P, delta, 0, 0, eng.DEST_HOST, eng.PATCH_KEEP_MARK, C.byref(out)) == 0
        size_ms = e.query_ms()
        ups, dels = int(uo[n]), int(do[n])
        up_ids, up_p, del_ids = np.empty(max(ups, 1), dtype=np.int32), np.empty(max(ups, 1)), np.empty(max(dels, 1), dtype=np.int32)
        out = eng.PatchOut(uo.ctypes.data_as(i64p), up_ids.ctypes.data, up_p.ctypes.data, do.ctypes.data_as(i64p), del_ids.ctypes.data, -1)
        assert L.dppr_group_patch(e._h, gid, MIN_P, delta, ups, dels, eng.DEST_HOST, eng.PATCH_REMARK_EMITTED, C.byref(out)) == 0
        assert out.written == 1
        return {"up_offsets": uo, "up_ids": up_ids[:ups], "up_p": up_p[:ups], "del_offsets": do, "del_ids": del_ids[:dels]}, size_ms, e.query_ms()

    held = eng.live_bytes()[0]
    e.group_mark(gid)  # the initial sync: the mark, then the export
    gw = (eng.live_bytes()[0] - held) // (8 * V)  # doubles per row of the state and of the mark
    prev = e.group_export_sparse(gid, MIN_P)
    e.set_profiling(1)  # (only the queries below are timed by events)
    t = {name: [] for name in ("size_dev", "fill_dev", "patch_call", "exp_dev", "exp_call", "diff_call", "expd_dev", "expd_call")}
    sizes = []
    for rep in range(reps):
        batch()
        t0 = time.perf_counter()
        pt, size_ms, fill_ms = patch_two_calls()
        t1 = time.perf_counter()
        now = e.group_export_sparse(gid, MIN_P)
        t2 = time.perf_counter()
        exp_ms = e.query_ms()
        t3 = time.perf_counter()
        want = diff_route(prev, now)
        t4 = time.perf_counter()
        for key in want:  # the patch is the diff of the two exports, bit for bit
            assert np.array_equal(np.asarray(pt[key]).view(np.uint8), np.asarray(want[key]).view(np.uint8)), (rep, key)
        total = int(now[0][n])
        d_ids = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        d_p = torch.empty(max(total, 1), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        t5 = time.perf_counter()
        e.group_export_sparse_dev(gid, MIN_P, total, d_ids.data_ptr(), d_p.data_ptr())
        t6 = time.perf_counter()
        expd_ms = e.query_ms()
        prev = now
        if rep >= a.warmup:
            for name, v in (("size_dev", size_ms), ("fill_dev", fill_ms), ("patch_call", (t1 - t0) * 1e3), ("exp_dev", exp_ms),
                            ("exp_call", (t2 - t1) * 1e3), ("diff_call", (t4 - t3) * 1e3), ("expd_dev", expd_ms), ("expd_call", (t6 - t5) * 1e3)):
                t[name].append(v)
            sizes.append((int(pt["up_offsets"][n]), int(pt["del_offsets"][n]), total))
        del d_ids, d_p
    # the same feed with a min_delta above 0: sizes and times alone (tests/test_patch_gpu.py holds such a feed to its bound)
    with_delta = []
    for delta in DELTAS:
        e.group_mark(gid)
        td = {name: [] for name in ("size_dev", "fill_dev", "patch_call")}
        sizes_d = []
        for rep in range(reps):
            batch()
            t0 = time.perf_counter()
            pt, size_ms, fill_ms = patch_two_calls(delta)
            t1 = time.perf_counter()
            if rep >= a.warmup:
                for name, v in (("size_dev", size_ms), ("fill_dev", fill_ms), ("patch_call", (t1 - t0) * 1e3)):
                    td[name].append(v)
                sizes_d.append((int(pt["up_offsets"][n]), int(pt["del_offsets"][n])))
        with_delta.append((delta, td, sizes_d))
    sp = e.id_space()
    rows = sp["ids"] + sp["parked"]
    fills = eng.bench_line_fills()
    copy = eng.bench_stream_copy()
    e.close()

    # what the three kernels of the sized call must move at least: ext2int, the mark rows and the mask (written, then read) of every
    # external id, one gathered p row per occupied row, and the entries themselves
    ups_med, dels_med = statistics.median(s[0] for s in sizes), statistics.median(s[1] for s in sizes)
    stream_bytes = V * (4 + 8 * gw + 4 + 4) + rows * 8 * gw + 12 * ups_med + 4 * dels_med
    fill_med = statistics.median(t["fill_dev"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# The patch feed (`dppr_group_patch`): times\n\n")
        f.write(f"Library build `{eng.build_id()}`. livejournal stand-in, window of {wl.window} edges, batches of {wl.per_batch}, V = {V}, "
                f"{rows} rows hold a vertex at the end; {N_SOURCES}-source group (rows of {gw} doubles), eps = {EPS:g}, min_p = {MIN_P:g}, min_delta = 0, the "
                f"emitted-only re-mark. `tools/patch_times.py`: median (min .. max) in ms over {a.repeats} repeats after {a.warmup} warm "
                "batches; every repeat takes one more batch (untimed), then runs the routes in turn and checks that the patch is the numpy "
                "diff of the two exports bit for bit. Device time: events around the first and the last kernel of one library call; call "
                "time: host clock around the Python call(s) (each ends in a stream synchronisation; allocation of the numpy outputs and "
                f"the copy back included). In the same process: 2^26 random 128-B line fills out of 1 GiB take {fills:.3f} ms "
                f"({(1 << 26) / fills / 1e6:.1f} G lines/s), a stream copy of 1 GiB takes {copy:.3f} ms ({2 * (1 << 30) / copy / 1e6:.0f} GB/s "
                "read + write).\n\n")
        f.write(f"Sizes over the repeats (min .. median .. max): upserts {min(s[0] for s in sizes)} .. {ups_med:.0f} .. {max(s[0] for s in sizes)}, "
                f"deletes {min(s[1] for s in sizes)} .. {dels_med:.0f} .. {max(s[1] for s in sizes)}, support "
                f"{min(s[2] for s in sizes)} .. {statistics.median(s[2] for s in sizes):.0f} .. {max(s[2] for s in sizes)} entries.\n\n")
        f.write("| route | device ms | call ms |\n|---|---|---|\n")
        f.write(f"| patch: the size call (classify, scan) | {summary(t['size_dev'])} | |\n")
        f.write(f"| patch: the sized call (classify, scan, fill + re-mark) | {summary(t['fill_dev'])} | |\n")
        f.write(f"| patch: both calls, host destination | | {summary(t['patch_call'])} |\n")
        f.write(f"| group_export_sparse to the host (device: its fill call) | {summary(t['exp_dev'])} | {summary(t['exp_call'])} |\n")
        f.write(f"| numpy diff of two exports | | {summary(t['diff_call'])} |\n")
        f.write(f"| group_export_sparse to the device, the fill call alone | {summary(t['expd_dev'])} | {summary(t['expd_call'])} |\n\n")
        for delta, td, sizes_d in with_delta:
            f.write(f"With min_delta = {delta:g} over {a.repeats} further batches: upserts {min(s[0] for s in sizes_d)} .. "
                    f"{statistics.median(s[0] for s in sizes_d):.0f} .. {max(s[0] for s in sizes_d)}, deletes {min(s[1] for s in sizes_d)} .. "
                    f"{statistics.median(s[1] for s in sizes_d):.0f} .. {max(s[1] for s in sizes_d)}; the size call {summary(td['size_dev'])} ms, the "
                    f"sized call {summary(td['fill_dev'])} ms on the device, both calls {summary(td['patch_call'])} ms on the host clock.\n\n")
        f.write(f"The sized call moves at least {stream_bytes / 1e6:.1f} MB (ext2int, the mark rows, the mask written and read, one p row per "
                f"occupied row, the entries): {stream_bytes / fill_med / 1e6:.0f} GB/s at its median device time.\n")
    print(open(a.out).read())


if __name__ == "__main__":
    main()
