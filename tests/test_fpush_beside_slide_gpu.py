"""The forward push (dppr_forward_push) beside the graph update of the NEXT batch, on the rig of
tests/test_queries_beside_slide_gpu.py: the result over the explicitly named epoch k is, bit for bit, the quiet result before, during
and after the concurrent slide of batch k + 1 -- also for a parked seed that the batch revives (its row moves) --, it is the numpy
restatement over the rows of epoch k, and after an exclusive slide that renumbers the call is refused as "epoch not resident"."""
import threading
import time

import numpy as np
import pytest

from dynamicppr_amd import engine as eng
from tests import forward_ref as fr
from tests import fpush_ref as pr
from tests.test_forward_gpu import rows_of
from tests.test_queries_beside_slide_gpu import Rig, V, hip, refused, same  # noqa: F401  (hip: the fixture)

pytestmark = pytest.mark.gpu

BATCHES = 36
EPS, ROUNDS, K, M = 1e-6, 24, 64, 5


def sets_of(rig):
    """The first two probed ids (vertices the next batch revives come first), a weighted set of four probed ids (they are
    distinct), one from the interleaved tail, and a live source."""
    ids = rig.ids
    return [int(ids[0]), int(ids[1]), (np.array([ids[0], ids[-1], ids[2], ids[5]]), np.array([0.5, 1.0, 2.0, 0.25])), int(ids[-2]), 0]


def push_all(rig, epoch):
    e, hp = rig.e, rig.hip
    got = e.forward_push(sets_of(rig), EPS, ROUNDS, k=K, at=rig.ids, epoch=epoch, dense_p_ptr=rig.d_dense, dtype=eng.F64, layout=eng.SOURCE_MAJOR)
    return {"meta": [got[x] for x in ("rounds_used", "converged", "rem", "pushes", "left", "work")], "at": [got["at_p"], got["at_r"]],
            "topk": [x for t in got["topk"] for x in t], "dense": [hp.read(rig.d_dense, 8 * M * V, np.float64)]}


def restated(rig, epoch):
    e = rig.e
    rows = rows_of(e, epoch)
    rowless = pr.rowless_mask(rows)
    want = [pr.push(rows, rowless, *((s, 1.0) if np.isscalar(s) else s), EPS, ROUNDS) for s in sets_of(rig)]
    meta = [np.array([getattr(w, x) for w in want], dtype=t) for x, t in (("rounds_used", np.int32), ("converged", np.int32), ("rem", np.float64),
                                                                          ("pushes", np.int64), ("left", np.int64))]
    return {"meta": meta + [pr.work(rows, want)],
            "at": [np.stack([w.p[rig.ids] for w in want]), np.stack([w.r[rig.ids] for w in want])],
            "topk": [x for w in want for x in fr.topk(w.p, K)],
            "dense": [np.stack([w.p for w in want]).reshape(-1)]}


@pytest.mark.parametrize("directed", [1, 0])
def test_forward_push_beside_a_concurrent_slide(hip, directed):
    rig = Rig(directed, hip, BATCHES, full=False)
    e = rig.e
    box = []
    rig.build(1, False, box)
    epoch = rig.built(box)[0]
    beside = slides = refusals = revived_beside = 0
    for k in range(1, BATCHES):
        rig.update(epoch)
        rig.probe(k)
        R0 = push_all(rig, epoch)
        if k in (1, 2, 9, BATCHES - 1):
            same(R0, restated(rig, epoch), (directed, k, "numpy"))
        box = []
        if e.renumbering_due():
            before = e.id_space()["renumberings"]
            rig.build(k + 1, False, box)
            if e.id_space()["renumberings"] > before:
                refused(lambda: push_all(rig, epoch))
                refusals += 1
            else:
                same(push_all(rig, epoch), R0, (directed, k, "after the exclusive slide"))
        else:
            before = e.id_space()["revivals"]
            th = threading.Thread(target=rig.build, args=(k + 1, True, box))
            calls = []
            th.start()
            try:
                while th.is_alive():
                    q0 = time.perf_counter()
                    got = push_all(rig, epoch)
                    calls.append((q0, time.perf_counter()))
                    same(got, R0, (directed, k, "beside"))
            finally:
                th.join()
            _, b0, b1 = rig.built(box)
            beside += sum(1 for q0, q1 in calls if q0 < b1 and q1 > b0)
            same(push_all(rig, epoch), R0, (directed, k, "after the join"))
            revived_beside += e.id_space()["revivals"] - before
            slides += 1
        epoch = rig.built(box)[0]
    print(f"directed={directed}: {beside} calls beside {slides} concurrent slides, revivals beside {revived_beside}, refused after {refusals} renumberings")
    assert beside >= 3 and refusals >= 1, (beside, slides, refusals)
    e.close()
