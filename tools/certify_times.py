#!/usr/bin/env python3
"""What a certificate costs: dppr_group_certify against the way of before, on the livejournal stand-in (BASELINE.json configs[2]),
10 sources in one group, eps = 1e-9, after the from-scratch solve and a few batches, the same state in one process, alternating.

  certify   Engine.group_certify with both parts, with the residual part alone and with the invariant part alone. Device time:
            events around the first and the last kernel of the library call (dppr_debug_query_ms, profiling on); call time: host
            clock around the Python call.
  before    what tools/soak.py and tests/test_fullsize_gpu.py do: ten group_reads (V x 10 x 2 doubles over PCIe), then per lane the
            scan of |r| and tests/util.invariant_max_err_np over the window's edges (which the host holds already: they are read
            once, outside the timing). Host clock; every group_read ends with a synchronisation.

Every CALLS / RECIPES-th certificate is followed by one pass of the way of before. The two answers are compared: max |r| equal, the
invariant errors apart by less than 1e-13. Beside the times: the algorithmic bytes of the invariant pass -- per stored edge one
4-byte head and one row of gw doubles of p (the (8 + 4/S)-bytes-per-edge-and-source model of the sweeps with gw for S), plus the
state read and the sums written and read, 2 x V x gw x 8 -- and the share of the random-line-fill ceiling measured in this run
(dppr_bench_line_fills, 1 GiB table). A run without a GPU fails (there is no CPU path). Writes profiles/certify_times.md, stamped
with the library's build id.

    python tools/certify_times.py [--out profiles/certify_times.md] [--batches 3] [--calls 25] [--recipes 5]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dynamicppr_amd import engine as eng, stream as st  # noqa: E402
from tests.util import invariant_max_err_np  # noqa: E402
from tools.explain_times import stand_in  # noqa: E402

EPS = 1e-9
WARMUP = 3


def summary(xs):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} .. {max(xs):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "certify_times.md"))
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--recipes", type=int, default=5)
    a = ap.parse_args()
    assert a.calls >= 20 and a.recipes >= 1

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
    row, col = e.read_out_graph()                   # the window by external id, as the host of the way of before holds it
    tails, heads = np.repeat(np.arange(V), np.diff(row)), col.astype(np.int64)
    Ed, gw = len(col), 10                           # (a 10-source group: rows of 10 doubles)

    def before():
        t0 = time.perf_counter()
        worst_r, worst_inv = np.zeros(n), np.zeros(n)
        for i in range(n):
            p, r = e.group_read(gid, i)
            worst_r[i] = np.max(np.abs(r))
            worst_inv[i] = invariant_max_err_np(p, r, tails, heads, V, sources[i])
        return 1e3 * (time.perf_counter() - t0), worst_r, worst_inv

    times = {"both": ([], []), "residual": ([], []), "invariant": ([], [])}
    before_ms, cert, was = [], None, None
    every = max(1, a.calls // a.recipes)
    for k in range(WARMUP + a.calls):
        for what, kw in (("both", {}), ("residual", dict(invariant=False)), ("invariant", dict(residual=False))):
            t0 = time.perf_counter()
            res = e.group_certify(gid, EPS, **kw)
            t1 = time.perf_counter()
            if k >= WARMUP:
                times[what][0].append(e.query_ms())
                times[what][1].append(1e3 * (t1 - t0))
            if what == "both":
                assert cert is None or all(np.asarray(cert[x]).tobytes() == np.asarray(res[x]).tobytes() for x in res), "two calls differ"
                cert = res
        if k >= WARMUP and (k - WARMUP) % every == 0 and len(before_ms) < a.recipes:
            ms, worst_r, worst_inv = before()
            before_ms.append(ms)
            was = (worst_r, worst_inv)
            print(f"call {k - WARMUP}: certify {times['both'][0][-1]:.3f} ms on the device, the way of before {ms:.0f} ms", flush=True)
    assert np.array_equal(cert["max_abs_r"], was[0]), (cert["max_abs_r"], was[0])
    assert np.all(np.abs(cert["inv_max_err"] - was[1]) < 1e-13), (cert["inv_max_err"], was[1])
    assert not cert["n_pos"].any() and not cert["n_neg"].any() and not cert["n_nonfinite"].any()

    lines = 1 << 26
    fills_per_s = lines / (eng.bench_line_fills(1 << 30, lines, reps=3) * 1e-3)
    e.close()

    dev = statistics.median(times["both"][0])
    inv = statistics.median(times["invariant"][0])
    rows = sp["ids"] + sp["parked"]                 # the occupied rows: the passes read ext2int for all of [0, V) and a row only where there is one
    edge_bytes, state_bytes, touched = Ed * (8 * gw + 4), 2 * V * gw * 8, 3 * rows * gw * 8 + 4 * V
    old = statistics.median(before_ms)
    text = [
        "# Certify a state (`dppr_group_certify`) against the dense reads of before: times\n",
        f"Library build `{eng.build_id()}`. livejournal stand-in, window of {wl.window} edges ({Ed} stored out-edges), V = {V}, {sp['ids']} live rows, "
        f"{n} sources in one group (rows of {gw} doubles), eps = {EPS:g}, after the from-scratch solve and {a.batches} batches. "
        f"`tools/certify_times.py`: median (min .. max) in ms over {a.calls} calls after {WARMUP} warm-up calls, the three forms and the way of "
        f"before alternating on the same state in one process. device = events around the first and the last kernel of the library call, "
        "call = host clock around the Python call. Every call returned identical bits; max |r| equals the dense reads', the invariant "
        f"errors agree to 1e-13 (largest: {cert['inv_max_err'].max():.3e} on the device, {was[1].max():.3e} in numpy).\n",
        "| form | device ms | call ms |\n|---|---|---|",
        f"| residual + invariant | {summary(times['both'][0])} | {summary(times['both'][1])} |",
        f"| residual alone | {summary(times['residual'][0])} | {summary(times['residual'][1])} |",
        f"| invariant alone | {summary(times['invariant'][0])} | {summary(times['invariant'][1])} |",
        f"\nThe way of before -- ten `group_read`s ({2 * 8 * V * n / 1e6:.0f} MB over PCIe), then per lane max |r| and `invariant_max_err_np` "
        f"over the window's edges, host clock: {summary(before_ms)} ms over {len(before_ms)} passes. Ratio of the medians, before / device: "
        f"**{old / dev:.0f} x** ({old / statistics.median(times['both'][1]):.0f} x against the call on the host clock).\n",
        f"Run-to-run spread of the device time of both parts over {a.calls} calls: min {min(times['both'][0]):.3f}, median {dev:.3f}, max "
        f"{max(times['both'][0]):.3f} ms ({100 * (max(times['both'][0]) - min(times['both'][0])) / dev:.1f} % of the median).\n",
        f"Algorithmic bytes of the invariant pass: {Ed} edges x ({8 * gw} + 4) B = {edge_bytes / 1e6:.1f} MB of heads and gathered rows, plus "
        f"2 x V x {gw} x 8 B = {state_bytes / 1e6:.1f} MB of state: {(edge_bytes + state_bytes) / 1e6:.1f} MB in {inv:.3f} ms = "
        f"{(edge_bytes + state_bytes) / (inv * 1e-3) / 1e9:.0f} GB/s. That model counts a state row for every one of the V ids; only "
        f"{rows} rows are occupied, so what the pass touches beside the edges is p, r and S of those rows and the id map, "
        f"{touched / 1e6:.1f} MB: {(edge_bytes + touched) / 1e6:.1f} MB = {(edge_bytes + touched) / (inv * 1e-3) / 1e9:.0f} GB/s. The gather is one random row per edge: {Ed / (inv * 1e-3) / 1e9:.2f} G rows/s "
        f"against {fills_per_s / 1e9:.2f} G random 128-byte line fills/s measured in this run (1 GiB table): "
        f"{100 * Ed / (inv * 1e-3) / fills_per_s:.0f} % of that ceiling (rows of hubs are served by L2, so the share may pass 100 %).\n",
    ]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        out.write("\n".join(text))
    print("\n".join(text))
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
