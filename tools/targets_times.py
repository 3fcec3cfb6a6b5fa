#!/usr/bin/env python3
"""What set lanes cost a batch: dppr_group_update on the livejournal stand-in, 10 lanes, eps = 1e-9, for lanes of 1, 64 and 4096
seeds each against the plain 10-source group, all in one session.

  plain      add_source_group of the 10 vertices of largest in-degree: k_su_apply, no seed table
  sets of m  add_target_group, lane i holding the m vertices of in-degree rank i, i + 10, i + 20, .. (so the 10 lanes together
             hold the 10 m vertices of largest in-degree), weight 1 / m each: k_su_apply_seeded with a binary search of at most
             log2(m) + 1 steps per tail run. m = 1 gives lanes of weight 1.0 -- source lanes, and the plain path: lane 0
             receives weight 0.5 instead so that the group keeps a table and the seeded kernel is what is timed

Every configuration follows the same stream from its own from-scratch solve: WARMUP batches, then BATCHES timed ones with
dppr_set_profiling on. Per batch: the event time of the whole timed region (what dppr_group_update returns), the sweeps' share of
it (dppr_stats_t.sweep_ms) and the rest -- the stream update, seeding, the push tail and launch gaps --, and, counted on the
host, the batch's records whose tail is a seed of some lane (lane x record pairs: the lookups that find a weight). A run without a
GPU fails (there is no CPU path). Writes profiles/targets_times.md, stamped with the library's build id.

    python tools/targets_times.py [--out profiles/targets_times.md] [--batches 20] [--warmup 3]
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dynamicppr_amd import datagen, engine as eng, stream as st  # noqa: E402

DATA = "/tmp/dppr_data"
EPS = 1e-9
LANES = 10
SIZES = (1, 64, 4096)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "targets_times.md"))
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    total = a.warmup + a.batches

    V, e1, e2, cfg, wl = stand_in("livejournal", total)
    heads = np.asarray(e2[:wl.window], dtype=np.int64)
    if not cfg.directed:
        heads = np.concatenate([heads, np.asarray(e1[:wl.window], dtype=np.int64)])
    indeg = np.bincount(heads, minlength=V)
    ranked = np.lexsort((np.arange(V), -indeg))  # in-degree descending, id ascending

    configs = [("plain 10-source group", None)]
    for m in SIZES:
        lanes = [(ranked[i:LANES * m:LANES].astype(np.int32), np.full(m, 1.0 / m)) for i in range(LANES)]
        if m == 1:
            lanes[0] = (lanes[0][0], np.array([0.5]))
        configs.append((f"sets of {m}", lanes))

    lines = []
    for name, lanes in configs:
        e = eng.Engine(V, wl.window, cfg.directed, wl.per_batch)
        ss = st.SlidingStream(V, e1, e2, cfg.directed, wl)
        e.load_window(*ss.serialize_edge_stream())
        if lanes is None:
            gid = e.add_source_group([int(x) for x in ranked[:LANES]])
            seed_of = [np.zeros(V, dtype=bool) for _ in range(LANES)]
            for i in range(LANES):
                seed_of[i][ranked[i]] = True
        else:
            gid = e.add_target_group(lanes)
            seed_of = []
            for ids, _ in lanes:
                s = np.zeros(V, dtype=bool)
                s[ids] = True
                seed_of.append(s)
        init_ms = e.group_init_solve(gid, EPS)
        e.set_profiling(1)
        ms, sweep, hits, records = [], [], [], 0
        for k in range(total):
            assert not ss.stream_updates()
            b1, b2, ins = ss.batch_arrays()
            e.set_batch(b1, b2, ins)
            e.slide(*ss.new_arrays())
            before = e.group_stats(gid)["sweep_ms"]
            t = e.group_update(gid, EPS)
            if k >= a.warmup:
                ms.append(t)
                sweep.append(e.group_stats(gid)["sweep_ms"] - before)
                tails = np.asarray(b1, dtype=np.int64)
                hits.append(int(sum(int(s[tails].sum()) for s in seed_of)))
                records = len(tails)
        rest = [x - y for x, y in zip(ms, sweep)]
        lines.append(f"| {name} | {init_ms:.2f} | {summary(ms)} | {summary(sweep)} | {summary(rest)} | {statistics.mean(hits):.1f} of {LANES * records} |")
        print(lines[-1], flush=True)
        e.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# Weighted vertex sets as targets (`dppr_add_target_group`): what a batch costs\n\n")
        f.write(f"Library build `{eng.build_id()}`. livejournal stand-in, window of {wl.window} edges, {wl.per_batch} stream edges per batch, "
                f"V = {V}; {LANES} lanes (rows of 16 doubles), eps = {EPS:g}. `tools/targets_times.py`: every configuration follows the same "
                f"stream from its own from-scratch solve, {a.warmup} warm-up batches, then {a.batches} timed ones with profiling on (an event "
                "pair around every sweep). Per batch, median (min .. max) in ms: the event time of `dppr_group_update`'s timed region, the "
                "sweeps' share of it, and the rest (stream update, seeding, push tail, gaps). Seeds are the vertices of largest in-degree in "
                "the initial window, dealt round-robin over the lanes. Last column: lane x record pairs of a batch whose tail is a seed of "
                "that lane (mean), of all pairs.\n\n")
        f.write("| lanes | init solve ms | group_update ms per batch | of that: sweeps | the rest | records that hit a seed |\n|---|---|---|---|---|---|\n")
        f.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
