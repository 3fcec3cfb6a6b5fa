"""dppr_patch / dppr_group_patch beside the graph update of the NEXT batch, on the rig of tests/test_queries_beside_slide_gpu.py
(churn stream, W = 600, c = 60, two resident epochs, renumbering at 8 % / 8 parked; a slot and a 10-source group on ONE engine) and
in the shape of tests/test_certify_beside_slide_gpu.py. A graph update changes no solver state and no mark, and a patch holds the
id-map lock as dppr_read does, so -- in the caller's ids -- a patch taken BEFORE, DURING and AFTER the concurrent slide of batch
k + 1 is, bit for bit, the quiet result, also when that batch names a new vertex or revives a parked one, and after an exclusive
slide that renumbers (a patch names no epoch). The quiet result is held to tests/patch_ref.py over the dense reads. Every patch
here keeps the mark (a re-mark would make the next call a different question); the mark is taken once, after the first update."""
import threading
import time

import numpy as np
import pytest

from dynamicppr_amd import engine as eng
from tests import patch_ref as ref
from tests.test_queries_beside_slide_gpu import Rig, hip  # noqa: F401  (hip: the fixture of that module)

pytestmark = pytest.mark.gpu

BATCHES = 20
DELTA = 1e-9


def family(rig, taus):
    """{handle: the patch at each of its thresholds, as a flat list of arrays}"""
    out = {}
    for h, (kind, hd, _, _) in rig.handles.items():
        out[h] = []
        for tau in taus[h]:
            pt = rig.e.patch(hd, tau, DELTA) if kind == "slot" else rig.e.group_patch(hd, tau, DELTA)
            out[h].append(pt)
    return out


def same(got, want, tag):
    assert got.keys() == want.keys(), tag
    for h in got:
        for a, b in zip(got[h], want[h]):
            assert ref.same_patch(a, b), (tag, h)


@pytest.mark.parametrize("directed", [1, 0])
def test_patches_before_during_and_after_a_concurrent_slide(hip, directed):
    rig = Rig(directed, hip, BATCHES, full=False)
    e = rig.e
    box = []
    rig.build(1, False, box)
    epoch = rig.built(box)[0]
    rig.update(epoch)
    rig.mark()
    taus = {}
    for h, marks in rig.marks.items():
        pos = np.concatenate([m[m > 0] for m in marks])
        taus[h] = (0.0, float(np.quantile(pos, 0.5)))
    beside = slides = revived_beside = exclusive = renumbered = entries = 0
    for k in range(1, BATCHES):
        if k > 1:
            rig.update(epoch)
        R0 = family(rig, taus)
        if k in (2, 3, 10, BATCHES - 1):  # the quiet result is the reference's
            D = rig.dense()
            for h in R0:
                for tau, pt in zip(taus[h], R0[h]):
                    want = ref.patch(D[h][0], rig.marks[h], tau, DELTA)
                    assert ref.same_patch(pt, want), (directed, k, h, tau)
                    entries += int(want["up_offsets"][-1] + want["del_offsets"][-1])
        box = []
        sp0 = e.id_space()
        if e.renumbering_due():
            rig.build(k + 1, False, box)
            renumbered += e.id_space()["renumberings"] - sp0["renumberings"]
            exclusive += 1
            same(family(rig, taus), R0, (directed, k, "after the exclusive slide"))
        else:
            th = threading.Thread(target=rig.build, args=(k + 1, True, box))
            calls = []
            th.start()
            try:
                while th.is_alive():
                    q0 = time.perf_counter()
                    got = family(rig, taus)
                    calls.append((q0, time.perf_counter()))
                    same(got, R0, (directed, k, "beside"))
            finally:
                th.join()
            _, b0, b1 = rig.built(box)
            beside += sum(1 for q0, q1 in calls if q0 < b1 and q1 > b0)
            same(family(rig, taus), R0, (directed, k, "after the next slide"))
            slides += 1
            revived_beside += e.id_space()["revivals"] - sp0["revivals"]
        epoch = rig.built(box)[0]
    print(f"directed={directed}: {beside} passes of the family beside {slides} concurrent slides, {exclusive} exclusive slides "
          f"({renumbered} renumbered), revivals beside {revived_beside}, {entries} entries held to numpy, {e.id_space()}")
    assert beside >= 3 and revived_beside >= 1 and renumbered >= 1 and entries > 0, (beside, revived_beside, renumbered, entries)
    e.close()
