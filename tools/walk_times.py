#!/usr/bin/env python3
"""Times of the forward walks and of the refined point queries on the livejournal stand-in, 10-source group, eps = 1e-9, after
the from-scratch solve.

  walks                 both kernel forms (lane refill, one walk per thread), W in {2^10, 2^16} x m in {1, 256}, device destination:
                        walks/s and steps/s (a step: one Philox draw with its two dependent loads; the mean number of draws per walk
                        comes from the numpy restatement of tests/walk_ref.py over a sample of the same starts)
  ceiling               dppr_bench_line_fills in the same process: random 128-byte line fills per second, at TWO lines per step
  group_refine_at       the whole call (walks, fold, finish, copy back), m = 256, both W
  group_read            the dense reads of p and r of all sources: what a finish on the CPU would need first

  device ms  events around the first and the last kernel of the library call (dppr_set_profiling, dppr_debug_query_ms)
  call ms    host clock around the Python call, which ends in a synchronisation of the solver stream
Every figure is the median of REPEATS calls after WARMUP calls, with the spread (min .. max). A run without a GPU fails (there is
no CPU path). Writes profiles/walk_times.md, stamped with the library's build id.

    python tools/walk_times.py [--out profiles/walk_times.md] [--repeats 9] [--warmup 2]
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
from tests import walk_ref  # noqa: E402

DATA = "/tmp/dppr_data"
EPS = 1e-9
N_SOURCES = 10
SEED = 0x5EED5EED5EED
FORMS = ((eng.WALK_REFILL, "lane refill"), (eng.WALK_PER_THREAD, "one walk per thread"))


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


class DeviceInts:
    """m * W int32 of device memory through the HIP runtime the library brought in."""

    def __init__(self, count):
        paths = {l.rsplit(" ", 1)[-1].strip() for l in open("/proc/self/maps") if "libamdhip64" in l}
        self.L = C.CDLL(paths.pop())
        self.L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.L.hipFree.argtypes = [C.c_void_p]
        self.p = C.c_void_p()
        assert self.L.hipMalloc(C.byref(self.p), 4 * count) == 0

    def free(self):
        assert self.L.hipFree(self.p) == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "walk_times.md"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
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
    sp = e.id_space()
    x2i = e.id_map()
    named = np.nonzero(x2i >= 0)[0]
    starts = named[np.random.default_rng(9).permutation(len(named))[:256]].astype(np.int32)
    # draws per walk: the restatement over the device's rows, 64 walks from each of the 256 starts
    row, col = e.read_out_graph()
    rp, cl, i2e = walk_ref.internal_csr(V, row, col, x2i)
    _, steps = walk_ref.walks(rp, cl, x2i.astype(np.int64), i2e, starts, 64, SEED, with_steps=True)
    draws = float(steps.mean())
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
        return statistics.median(d)

    buf = DeviceInts(256 << 16)
    rate = {}
    for W in (1 << 10, 1 << 16):
        for m in (1, 256):
            for form, fname in FORMS:
                e.set_walk_form(form)
                ms = timed(f"walks, {fname}, W = 2^{W.bit_length() - 1}, m = {m}", lambda: e.walks_dev(starts[:m], W, SEED, buf.p.value))
                rate[(W, m, form)] = m * W / ms / 1e3  # M walks/s
                lines[-1] = lines[-1][:-2] + f"{rate[(W, m, form)]:.1f} M walks/s, {rate[(W, m, form)] * draws / 1e3:.2f} G steps/s |"
    e.set_walk_form(eng.WALK_REFILL)
    buf.free()
    for W in (1 << 10, 1 << 16):
        timed(f"group_refine_at, W = 2^{W.bit_length() - 1}, m = 256, {N_SOURCES} sources", lambda: e.group_refine_at(gid, starts, W, SEED),
              "walks + fold + finish; the call time includes the copy back")
    t = []
    for rep in range(reps):
        t0 = time.perf_counter()
        for i in range(N_SOURCES):
            e.group_read(gid, i)
        if rep >= a.warmup:
            t.append((time.perf_counter() - t0) * 1e3)
    lines.append(f"| group_read of p and r, {N_SOURCES} sources | - | {summary(t)} | {16 * N_SOURCES * V / 1e6:.1f} MB to the host |")
    fills = eng.bench_line_fills()
    e.close()
    fill_rate = (1 << 26) / fills / 1e6  # G lines/s
    big = {form: rate[(1 << 16, 256, form)] for form, _ in FORMS}

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# Forward walks and refined point queries (`dppr_walks`, `dppr_group_refine_at`): times\n\n")
        f.write(f"Library build `{eng.build_id()}`. livejournal stand-in, window of {wl.window} edges, V = {V}, {sp['ids'] + sp['parked']} rows "
                f"hold a vertex; {N_SOURCES}-source group, eps = {EPS:g}, after the from-scratch solve; 256 starts drawn from the vertices "
                f"with an id. `tools/walk_times.py`: median (min .. max) in ms over {a.repeats} calls after {a.warmup} warm-up calls. A walk "
                f"takes {draws:.2f} draws on average here (the numpy restatement over 64 walks from each start). In the same process: 2^26 "
                f"random 128-B line fills out of 1 GiB take {fills:.3f} ms ({fill_rate:.2f} G lines/s): at two lines per step the ceiling is "
                f"{fill_rate / 2:.2f} G steps/s.\n\n")
        f.write(f"Against the expectation of DESIGN 9g: at W = 2^16, m = 256 the lane-refill form runs {big[eng.WALK_REFILL] * draws / 1e3:.2f} G "
                f"steps/s, {100 * big[eng.WALK_REFILL] * draws / 1e3 / (fill_rate / 2):.0f} % of the ceiling, and "
                f"{big[eng.WALK_REFILL] / big[eng.WALK_PER_THREAD]:.2f} x the one-walk-per-thread form. (The ceiling is that of lines which miss "
                "every cache; the W walks of one start share the rows of their first steps, so a figure above it says the loads hit.)\n\n")
        f.write("| route | device ms | call ms | note |\n|---|---|---|---|\n")
        f.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
