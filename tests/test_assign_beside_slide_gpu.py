"""dppr_assign / dppr_assign_at beside the graph update of the NEXT batch, on the rig and by the method of
tests/test_queries_beside_slide_gpu.py (churn stream, W = 600, c = 60, two resident epochs, renumbering at 8 % / 8 parked; a
3-source group, a 10-source group and a 5-lane set group on ONE engine). A graph update changes no solver state, so -- in the
caller's ids -- the labels, best, margin, counts and the flips against a fixed previous labelling over all three groups are, bit
for bit, the quiet result BEFORE, DURING and AFTER the concurrent slide of batch k + 1, also at a parked vertex that batch revives
(its id changes, its rows move); and they are still answered after an exclusive slide that renumbers, because the query reads no
epoch. The quiet result is the numpy restatement (tests/assign_ref.py) over the dense reads.

BATCHES = 20. Measured on an MI355X with this rig: a concurrent set_batch + slide takes 0.53 to 0.56 ms, a quiet pass of the family
(two assign and two assign_at calls) 0.31 to 0.33 ms, and 5 of the 19 slides are exclusive (all 5 renumber). 20 batches gave 21
(undirected) and 27 (directed) passes of the family beside the 14 concurrent slides, 12 vertices revived beside a pass, 14 probes of
a revived vertex by assign_at; with 40 batches the figures were 36 / 38 passes beside 27 slides and 31 revivals. At least 6 passes
beside a slide, one revival, one revived vertex probed and one renumbering are asked for."""
import threading
import time

import numpy as np
import pytest

from tests import assign_ref as ref
from tests.test_queries_beside_slide_gpu import Rig, V, eq, hip  # noqa: F401  (hip: the fixture of that module)

pytestmark = pytest.mark.gpu

BATCHES = 20


def family(rig, prev):
    """The calls of the family over (g3, g10, tg): dict of lists of arrays, as the families of the rig."""
    e = rig.e
    groups = [rig.g3, rig.g10, rig.tg]
    scale = rig.assign_scale
    out = {}
    for what, sc, ms in (("plain", None, 0.0), ("scaled", scale, 1e-6)):
        a = e.assign(groups, sc, ms, prev=prev)
        out[what] = [a["label"], a["best"], a["margin"], a["counts"], np.array([a["n_flips"]])] + list(a["flips"])
        out[(what, "at")] = list(e.assign_at(groups, rig.ids, sc, ms))
    return out


def same(got, want, tag):
    assert got.keys() == want.keys(), tag
    for key in got:
        assert len(got[key]) == len(want[key]), (tag, key)
        for j, (a, b) in enumerate(zip(got[key], want[key])):
            assert eq(a, b), (tag, key, j, np.asarray(a).ravel()[:6], np.asarray(b).ravel()[:6])


def restated(rig, prev):
    D = rig.dense()
    P = np.stack([p for h in ("g3", "g10", "tg") for p in D[h][0]], axis=1)
    out = {}
    for what, sc, ms in (("plain", None, 0.0), ("scaled", rig.assign_scale, 1e-6)):
        label, best, second, second_label, margin = ref.assign(P, sc, ms)
        fl = ref.flips(prev, label)
        out[what] = [label, best, margin, ref.counts(label, P.shape[1]), np.array([len(fl[0])])] + list(fl)
        out[(what, "at")] = [label[rig.ids], best[rig.ids], second_label[rig.ids], margin[rig.ids]]
    return out


@pytest.mark.parametrize("directed", [1, 0])
def test_assign_before_during_and_after_a_concurrent_slide(hip, directed):
    rig = Rig(directed, hip, BATCHES)
    e = rig.e
    rig.assign_scale = np.random.default_rng(12).random(18) + 0.25
    rig.assign_scale[4] = 0.0
    box = []
    rig.build(1, False, box)
    epoch = rig.built(box)[0]
    prev = np.full(V, -1, dtype=np.int32)
    beside = slides = revived_beside = revived_probed = exclusive = renumbered = 0
    t_slide = t_pass = 0.0
    for k in range(1, BATCHES):
        rig.update(epoch)
        ids = rig.probe(k)
        t0 = time.perf_counter()
        R0 = family(rig, prev)
        t_pass += time.perf_counter() - t0
        if k in (1, 2, 10, BATCHES - 1):
            same(R0, restated(rig, prev), (directed, k, "numpy"))
        box = []
        m0, sp0 = e.id_map(), e.id_space()
        if e.renumbering_due():
            rig.build(k + 1, False, box)
            renumbered += e.id_space()["renumberings"] - sp0["renumberings"]
            exclusive += 1
            same(family(rig, prev), R0, (directed, k, "after the exclusive slide"))   # (no resident epoch is needed)
        else:
            th = threading.Thread(target=rig.build, args=(k + 1, True, box))
            calls = []
            th.start()
            try:
                while th.is_alive():
                    q0 = time.perf_counter()
                    got = family(rig, prev)
                    calls.append((q0, time.perf_counter()))
                    same(got, R0, (directed, k, "beside"))
            finally:
                th.join()
            _, b0, b1 = rig.built(box)
            beside += sum(1 for q0, q1 in calls if q0 < b1 and q1 > b0)
            same(family(rig, prev), R0, (directed, k, "after the join"))
            slides += 1
            t_slide += b1 - b0
            revived_beside += e.id_space()["revivals"] - sp0["revivals"]
            moved = np.nonzero((m0 >= 0) & (e.id_map() != m0))[0]     # vertices the slide revived: they had an id, and it changed
            revived_probed += int(np.count_nonzero(np.isin(moved, ids)))
        prev = R0["plain"][0]             # the labels of this batch are the next one's previous labelling
        epoch = rig.built(box)[0]
    print(f"directed={directed}: {beside} passes of the family beside {slides} concurrent slides of {1e3 * t_slide / max(slides, 1):.2f} ms, "
          f"a quiet pass {1e3 * t_pass / (BATCHES - 1):.2f} ms, {exclusive} exclusive slides ({renumbered} renumbered), revivals beside {revived_beside}, "
          f"of them probed by assign_at {revived_probed}, {e.id_space()}")
    assert beside >= 6 and revived_beside >= 1 and revived_probed >= 1 and renumbered >= 1, (beside, revived_beside, revived_probed, renumbered)
    e.close()
