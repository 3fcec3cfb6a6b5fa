"""The forward sweep (dppr_forward) beside the graph update of the NEXT batch, on the rig of tests/test_queries_beside_slide_gpu.py:
the result over the explicitly named epoch k is, bit for bit, the quiet result before, during and after the concurrent slide of batch
k + 1 -- also for a parked start that the batch revives (its row moves) --, it is the numpy restatement over the rows of epoch k, and
after an exclusive slide that renumbers the call is refused as "epoch not resident"."""
import threading
import time

import numpy as np
import pytest

from dynamicppr_amd import engine as eng
from tests import forward_ref as fr
from tests.test_forward_gpu import Columns, rows_of
from tests.test_queries_beside_slide_gpu import Rig, V, hip, refused, same  # noqa: F401  (hip: the fixture)

pytestmark = pytest.mark.gpu

BATCHES = 36
ITERS, TOL, K, M = 24, 1e-6, 64, 5


def starts_of(rig):
    """The first two probed ids (vertices the next batch revives come first), two from the interleaved tail, and a live source."""
    return np.array([rig.ids[0], rig.ids[1], rig.ids[-1], rig.ids[-2], 0], dtype=np.int32)


def forward_all(rig, epoch):
    e, hp = rig.e, rig.hip
    starts = starts_of(rig)
    got = e.forward(starts, ITERS, TOL, k=K, at=rig.ids, epoch=epoch, dense_ptr=rig.d_dense, dtype=eng.F64, layout=eng.SOURCE_MAJOR)
    return {"meta": [got["iters_used"], got["rem"]], "at": [got["at"]], "topk": [x for t in got["topk"] for x in t],
            "dense": [hp.read(rig.d_dense, 8 * M * V, np.float64)]}


def restated(rig, epoch):
    cols = Columns(rows_of(rig.e, epoch))
    want = [cols(q, ITERS, TOL) for q in starts_of(rig)]
    return {"meta": [np.array([w[2] for w in want], dtype=np.int32), np.array([w[1] for w in want])],
            "at": [np.stack([w[0][rig.ids] for w in want])],
            "topk": [x for w in want for x in fr.topk(w[0], K)],
            "dense": [np.stack([w[0] for w in want]).reshape(-1)]}


@pytest.mark.parametrize("directed", [1, 0])
def test_forward_beside_a_concurrent_slide(hip, directed):
    rig = Rig(directed, hip, BATCHES, full=False)
    e = rig.e
    box = []
    rig.build(1, False, box)
    epoch = rig.built(box)[0]
    beside = slides = refusals = revived_beside = 0
    for k in range(1, BATCHES):
        rig.update(epoch)
        rig.probe(k)
        R0 = forward_all(rig, epoch)
        if k in (1, 2, 9, BATCHES - 1):
            same(R0, restated(rig, epoch), (directed, k, "numpy"))
        box = []
        if e.renumbering_due():
            before = e.id_space()["renumberings"]
            rig.build(k + 1, False, box)
            if e.id_space()["renumberings"] > before:
                refused(lambda: forward_all(rig, epoch))
                refusals += 1
            else:
                same(forward_all(rig, epoch), R0, (directed, k, "after the exclusive slide"))
        else:
            before = e.id_space()["revivals"]
            th = threading.Thread(target=rig.build, args=(k + 1, True, box))
            calls = []
            th.start()
            try:
                while th.is_alive():
                    q0 = time.perf_counter()
                    got = forward_all(rig, epoch)
                    calls.append((q0, time.perf_counter()))
                    same(got, R0, (directed, k, "beside"))
            finally:
                th.join()
            _, b0, b1 = rig.built(box)
            beside += sum(1 for q0, q1 in calls if q0 < b1 and q1 > b0)
            same(forward_all(rig, epoch), R0, (directed, k, "after the join"))
            revived_beside += e.id_space()["revivals"] - before
            slides += 1
        epoch = rig.built(box)[0]
    print(f"directed={directed}: {beside} calls beside {slides} concurrent slides, revivals beside {revived_beside}, refused after {refusals} renumberings")
    assert beside >= 3 and refusals >= 1, (beside, slides, refusals)
    e.close()
