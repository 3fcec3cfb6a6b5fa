"""dppr_certify / dppr_group_certify beside the graph update of the NEXT batch, on the rig and by the method of
tests/test_explain_beside_slide_gpu.py (churn stream, W = 600, c = 60, two resident epochs, renumbering at 8 % / 8 parked; a slot, a
10-source group and a 5-lane set group on ONE engine). A graph update changes no solver state and the epoch the states stand on
stays resident, so every output of the certificate over the explicitly named epoch k is, bit for bit, the quiet result BEFORE,
DURING and AFTER the concurrent slide of batch k + 1 -- also when that batch names a new vertex or revives a parked one (the row
gets an id, or moves; it holds no edge in epoch k). After an exclusive slide that renumbers, every call is refused as "epoch not
resident": the call always names an epoch. The quiet result is held to the numpy restatement (tests/certify_ref.py) over the dense
reads and the epoch's out-edges by external id.

BATCHES = 20, as tests/test_explain_beside_slide_gpu.py: at least 3 passes of the family beside a slide, one revival beside a pass
and one renumbering are asked for (conditions on the rig, not on the call)."""
import threading
import time

import numpy as np
import pytest

from tests import certify_ref as cr
from tests.test_certify_gpu import INVARIANT_TOL, RESIDUAL, bits, edges_of
from tests.test_explain_beside_slide_gpu import seeds_of
from tests.test_queries_beside_slide_gpu import EPS, Rig, V, eq, hip, refused  # noqa: F401  (hip: the fixture of that module)

pytestmark = pytest.mark.gpu

BATCHES = 20
KEYS = RESIDUAL + ("inv_max_err", "inv_argmax", "state_epoch", "converged", "conv_eps")


def handles(rig):
    return ["slot"] + rig.wide


def family(rig, epoch, resident=True):
    """{handle: [the outputs]}; after a renumbering (resident False) every call is refused."""
    e, out = rig.e, {}
    for h in handles(rig):
        kind, hd, _, _ = rig.handles[h]
        call = (lambda: e.certify(hd, EPS, epoch)) if kind == "slot" else (lambda: e.group_certify(hd, EPS, epoch))
        if resident:
            res = call()
            out[h] = [np.asarray(res[k]) for k in KEYS]
        else:
            refused(call)
    return out


def same(got, want, tag):
    assert got.keys() == want.keys(), tag
    for key in got:
        for k, a, b in zip(KEYS, got[key], want[key]):
            assert eq(a, b), (tag, key, k, a, b)


def held_to_numpy(rig, R0, epoch, tag):
    D = rig.dense()
    tails, heads = edges_of(rig.e, epoch)
    has_id = rig.e.id_map() >= 0
    for h in handles(rig):
        want = cr.certify(V, tails, heads, D[h][0], D[h][1], seeds_of(rig, h), EPS, has_id)
        got = dict(zip(KEYS, R0[h]))
        for k in RESIDUAL:
            if want[k].dtype == np.float64:
                assert np.array_equal(bits(got[k]), bits(want[k])), (tag, h, k, got[k], want[k])
            else:
                assert np.array_equal(got[k], want[k]), (tag, h, k, got[k], want[k])
        assert np.all(np.abs(got["inv_max_err"] - want["inv_max_err"]) < INVARIANT_TOL), (tag, h, got["inv_max_err"], want["inv_max_err"])
        assert np.all(got["inv_max_err"] < INVARIANT_TOL) and np.all(got["n_pos"] == 0) and np.all(got["n_neg"] == 0), (tag, h)
        assert got["state_epoch"] == epoch and got["converged"] == 1


@pytest.mark.parametrize("directed", [1, 0])
def test_certificates_before_during_and_after_a_concurrent_slide(hip, directed):
    rig = Rig(directed, hip, BATCHES)
    e = rig.e
    box = []
    rig.build(1, False, box)
    epoch = rig.built(box)[0]
    beside = slides = revived_beside = exclusive = renumbered = 0
    for k in range(1, BATCHES):
        rig.update(epoch)
        rig.probe(k)
        e.debug_certify(*((0, 0), (7, 1), (64, 4))[k % 3])   # (every setting: the order of the additions is a function of it alone)
        R0 = family(rig, epoch)
        if k in (1, 2, 10, BATCHES - 1):
            held_to_numpy(rig, R0, epoch, (directed, k, "numpy"))
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
