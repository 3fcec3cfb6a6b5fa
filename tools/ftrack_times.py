#!/usr/bin/env python3
"""What it costs to keep a forward vector current: dppr_ftrack_update against a fresh dppr_forward_push on the same epoch at the same
eps -- what a caller had to do before the track existed --, on the livejournal stand-in (BASELINE.json configs[2]), batch by batch,
all in one session.

  cases      three start sets -- the hub (largest out-degree), a vertex of median out-degree among those with an out-edge, and a
             64-seed set (64 vertices drawn from those with an out-edge, weights in [0.05, 1.05)) -- at eps in {1e-6, 1e-8},
             max_rounds = 256. Each case is a track of one column, created after the load and WARM slides.
  update     ForwardTrack.update to the new epoch, the statistics alone (no part that copies p out). Device time: events around
             the first and the last kernel of the library call (dppr_debug_query_ms, profiling on), cut by three more events into
             load | fix-up | rounds | store (dppr_debug_ftrack_ms): the load and the store are the two whole-V copies (the store
             with the fold of rem), the fix-up holds the two device sorts of the records.
  fresh      Engine.forward_push of the same set on the same epoch with the same eps and cap, right after the update.

One call of each per batch and case (an update cannot be repeated): the table lists every batch, nothing is averaged. A run without
a GPU fails (there is no CPU path). Writes profiles/ftrack_times.md, stamped with the library's build id.

    python tools/ftrack_times.py [--out profiles/ftrack_times.md] [--batches 5]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dynamicppr_amd import engine as eng, stream as st  # noqa: E402
from tools.forward_times import row_width, stand_in  # noqa: E402

EPSS = (1e-6, 1e-8)
MAX_ROUNDS = 256
WARM = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ftrack_times.md"))
    ap.add_argument("--batches", type=int, default=5)
    a = ap.parse_args()

    V, e1, e2, cfg, wl = stand_in("livejournal", WARM + a.batches)
    e = eng.Engine(V, wl.window, cfg.directed, wl.per_batch)
    ss = st.SlidingStream(V, e1, e2, cfg.directed, wl)
    e.load_window(*ss.serialize_edge_stream())

    def slide():
        assert not ss.stream_updates()
        e.set_batch(*ss.batch_arrays())
        return e.slide(*ss.new_arrays())

    for _ in range(WARM):
        slide()
    e.set_profiling(1)
    row, col, _ = e.read_graph()
    Ed = int(row[-1])
    d = np.bincount(col[:Ed].astype(np.int64), minlength=V)
    live = int(np.count_nonzero(e.id_map() >= 0))
    by_deg = np.lexsort((np.arange(V), -d))   # out-degree descending, id ascending
    with_out = by_deg[:int(np.count_nonzero(d > 0))]
    rng = np.random.default_rng(64)
    many = (np.sort(rng.choice(with_out, 64, replace=False)).astype(np.int32), rng.random(64) + 0.05)
    cases = (("hub (d = %d)" % d[by_deg[0]], int(by_deg[0])), ("median out-degree (d = %d)" % d[with_out[len(with_out) // 2]], int(with_out[len(with_out) // 2])),
             ("64 seeds", many))
    tracks = [(name, s, eps, e.ftrack([s], eps, MAX_ROUNDS)) for name, s in cases for eps in EPSS]
    for name, s, eps, t in tracks:   # (a warm call of each kind: the work space is sized)
        e.forward_push([s], eps, MAX_ROUNDS)

    lines = []
    for b in range(a.batches):
        ep = slide()
        for name, s, eps, t in tracks:
            got = t.update(ep, MAX_ROUNDS)
            total, cut = e.query_ms(), t.times_ms()
            fresh = e.forward_push([s], eps, MAX_ROUNDS)
            fresh_ms = e.query_ms()
            lines.append(f"| {b + 1} | {name} | {eps:g} | {int(got['rounds_used'][0])} / {int(got['converged'][0])} | {' / '.join(str(int(x)) for x in got['fix'])} | "
                         f"{' / '.join(str(int(x)) for x in got['work'])} | {total:.3f} | {cut[0]:.3f} | {cut[1]:.3f} | {cut[2]:.3f} | {cut[3]:.3f} | "
                         f"{int(fresh['rounds_used'][0])} / {int(fresh['converged'][0])} | {' / '.join(str(int(x)) for x in fresh['work'])} | {fresh_ms:.3f} | "
                         f"{fresh_ms / total:.2f} | {float(got['rem'][0]):.3g} / {float(fresh['rem'][0]):.3g} |")
            print(lines[-1], flush=True)
    e.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write("# Keeping a forward vector current (`dppr_ftrack_update`) against a fresh push per batch (`dppr_forward_push`): times\n\n")
        fo.write(f"Library build `{eng.build_id()}`. livejournal stand-in, window of {wl.window} edges ({Ed} stored entries of the in-CSR), V = {V}, "
                 f"{live} vertices hold an id, {wl.per_batch} deletes and {wl.per_batch} inserts per batch, after the load and {WARM} slides. "
                 f"`tools/ftrack_times.py`: ONE call of each kind per batch and case (an update cannot be repeated), every batch listed; "
                 f"max_rounds = {MAX_ROUNDS}; each track has one column (row width {row_width(1)}: a whole-V copy moves {2 * 8 * row_width(1)} bytes per "
                 f"vertex and plane pair, V x m = {V}). device ms = events around the first and the last kernel of the library call, the "
                 "read-backs of the chunk word inside; load | fix-up | rounds | store cut it by three more events (the store includes the fold of "
                 "rem; the fix-up includes the two device sorts of the records). work = rows pushed / rows gathered / in-edges of those rows, "
                 "summed over the rounds. fix = records / distinct tails / distinct heads. speed-up = fresh device ms / update device ms.\n\n")
        fo.write("| batch | start | eps | update rounds / converged | fix | update work | update device ms | load | fix-up | rounds | store | "
                 "fresh rounds / converged | fresh work | fresh device ms | speed-up | rem update / fresh |\n")
        fo.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        fo.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
