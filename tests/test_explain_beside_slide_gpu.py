"""dppr_explain_at / dppr_group_explain_at beside the graph update of the NEXT batch, on the rig and by the method of
tests/test_position_beside_slide_gpu.py (churn stream, W = 600, c = 60, two resident epochs, renumbering at 8 % / 8 parked; a slot, a
10-source group and a 5-lane set group on ONE engine). A graph update changes no solver state and the epoch the states stand on
stays resident, so -- in the caller's ids -- contributors and paths are, value for value, the quiet result BEFORE, DURING and AFTER
the concurrent slide of batch k + 1, also at a parked vertex that batch revives (its id changes, its rows move). After an exclusive
slide that renumbers, every call is refused as "epoch not resident": the call always reads the epoch's out-CSR. The quiet result is
the numpy restatement (tests/explain_ref.py) over the dense reads and the epoch's out-CSR by external id. The epoch of the last
update is always named.

BATCHES = 20, as tests/test_position_beside_slide_gpu.py: at least 3 passes of the family beside a slide, one revival beside a pass
and one renumbering are asked for (conditions on the rig, not on the call)."""
import threading
import time

import numpy as np
import pytest

from tests import explain_ref as xr
from tests.test_queries_beside_slide_gpu import Rig, V, eq, hip, refused  # noqa: F401  (hip: the fixture of that module)

pytestmark = pytest.mark.gpu

BATCHES = 20
SHAPES = ((3, 16), (16, 2))   # (f, depth)
KEYS = ("deg", "distinct", "self", "nbr_count", "nbr", "nbr_mult", "nbr_c", "len", "end", "path", "path_p", "path_c")


def handles(rig):
    return ["slot"] + rig.wide


def family(rig, epoch, resident=True):
    """{(handle, f, depth): [the twelve arrays]}; after a renumbering (resident False) every call is refused."""
    e, out = rig.e, {}
    for h in handles(rig):
        kind, hd, _, _ = rig.handles[h]
        for f, depth in SHAPES:
            if kind == "slot":
                call = lambda: e.explain_at(hd, rig.ids, f, depth, epoch)   # noqa: E731
            else:
                call = lambda: e.group_explain_at(hd, rig.ids, f, depth, epoch)   # noqa: E731
            if resident:
                res = call()
                out[(h, f, depth)] = [res[k] for k in KEYS]
            else:
                refused(call)
    return out


def same(got, want, tag):
    assert got.keys() == want.keys(), tag
    for key in got:
        for k, a, b in zip(KEYS, got[key], want[key]):
            assert eq(a, b), (tag, key, k, np.asarray(a).ravel()[:6], np.asarray(b).ravel()[:6])


def seeds_of(rig, h):
    if h == "tg":
        return [list(zip(ids.tolist(), np.asarray(w, dtype=np.float64).tolist())) for ids, w in rig.sets]
    return [s[0] for s in rig.handles[h][3]]


def restated(rig, epoch):
    D = rig.dense()
    g = xr.from_csr(*rig.e.read_out_graph(epoch))
    out = {}
    for h in handles(rig):
        for f, depth in SHAPES:
            res = xr.explain(g, D[h][0], seeds_of(rig, h), rig.ids, f, depth)
            if h == "slot":
                res = xr.slot_form(res)
            out[(h, f, depth)] = [res[k] for k in KEYS]
    return out


@pytest.mark.parametrize("directed", [1, 0])
def test_explanations_before_during_and_after_a_concurrent_slide(hip, directed):
    rig = Rig(directed, hip, BATCHES)
    e = rig.e
    box = []
    rig.build(1, False, box)
    epoch = rig.built(box)[0]
    beside = slides = revived_beside = exclusive = renumbered = 0
    for k in range(1, BATCHES):
        rig.update(epoch)
        rig.probe(k)
        R0 = family(rig, epoch)
        if k in (1, 2, 10, BATCHES - 1):
            same(R0, restated(rig, epoch), (directed, k, "numpy"))
        box = []
        sp0 = e.id_space()
        if e.renumbering_due():
            rig.build(k + 1, False, box)
            moved = e.id_space()["renumberings"] - sp0["renumberings"]
            renumbered += moved
            exclusive += 1
            R1 = family(rig, epoch, resident=not moved)
            if moved:
                assert not R1
            else:
                same(R1, R0, (directed, k, "after the exclusive slide"))
        else:
            th = threading.Thread(target=rig.build, args=(k + 1, True, box))
            calls = []
            th.start()
            try:
                while th.is_alive():
                    q0 = time.perf_counter()
                    got = family(rig, epoch)
                    calls.append((q0, time.perf_counter()))
                    same(got, R0, (directed, k, "beside"))
            finally:
                th.join()
            _, b0, b1 = rig.built(box)
            beside += sum(1 for q0, q1 in calls if q0 < b1 and q1 > b0)
            same(family(rig, epoch), R0, (directed, k, "after the next slide"))
            slides += 1
            revived_beside += e.id_space()["revivals"] - sp0["revivals"]
        epoch = rig.built(box)[0]
    print(f"directed={directed}: {beside} passes of the family beside {slides} concurrent slides, {exclusive} exclusive slides "
          f"({renumbered} renumbered), revivals beside {revived_beside}, {e.id_space()}")
    assert beside >= 3 and revived_beside >= 1 and renumbered >= 1, (beside, revived_beside, renumbered)
    e.close()
