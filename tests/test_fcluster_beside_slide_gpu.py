"""The full-length conductance sweep of a forward track (dppr_ftrack_cluster) beside the graph update of the NEXT batch, on the rig of
tests/test_queries_beside_slide_gpu.py: a track stands on epoch k; its sweep under both orders is taken while nothing else runs --
and is the numpy definition over the rows of epoch k --, then again and again while dppr_slide_concurrent builds epoch k + 1. Bit for
bit the calls beside the slide equal the quiet one."""
import threading
import time

import numpy as np
import pytest

from tests import fcluster_ref as fcr
from tests.test_forward_gpu import rows_of
from tests.test_ftrack_gpu import RefTrack
from tests.test_queries_beside_slide_gpu import Rig, V, hip, same  # noqa: F401  (hip: the fixture)

pytestmark = pytest.mark.gpu

BATCHES = 30
EPS, ROUNDS = 1e-6, 24
SETS = [0, 1, (np.array([2, 3, 5, 8]), np.array([0.5, 1.0, 2.0, 0.25])), V // 2, V - 1]


def sweep(t):
    out = {}
    for order in ("deg", "p"):
        best, off, *arrays = t.cluster(order, profile=True)
        out[order] = [np.array([[b[k] for k in ("count", "best_size", "best_cut", "best_vol")] for b in best], dtype=np.int64),
                      np.array([b["best_phi"] for b in best]), off] + arrays
    return out


def restated(e, epoch, ref):
    row, col = e.read_out_graph(epoch)
    out = {}
    for order in ("deg", "p"):
        res = [fcr.cluster(c.p, row, col, order) for c in ref.cols]
        off = np.concatenate([[0], np.cumsum([len(r[1]) for r in res])]).astype(np.int64)
        out[order] = [np.array([[r[0][k] for k in ("count", "best_size", "best_cut", "best_vol")] for r in res], dtype=np.int64),
                      np.array([r[0]["best_phi"] for r in res]), off] + [np.concatenate([r[i] for r in res]) for i in range(1, 6)]
    return out


@pytest.mark.parametrize("directed", [1, 0])
def test_a_sweep_beside_a_concurrent_slide(hip, directed):
    rig = Rig(directed, hip, BATCHES, full=False)
    e = rig.e
    t = e.ftrack(SETS, EPS, ROUNDS)
    ref = RefTrack(rows_of(e, 0), SETS, EPS, ROUNDS)
    box = []
    rig.build(1, False, box)
    epoch = rig.built(box)[0]
    beside = slides = 0
    for k in range(1, BATCHES):
        rig.update(epoch)
        ref.rows = rows_of(e, epoch)
        ref.update(ref.rows, rig.stage[k - 1]["b"], ROUNDS)
        t.update(epoch, ROUNDS)
        R0 = sweep(t)
        same(R0, restated(e, epoch, ref), (directed, k, "numpy"))
        box = []
        if e.renumbering_due():
            rig.build(k + 1, False, box)
        else:
            th = threading.Thread(target=rig.build, args=(k + 1, True, box))
            calls = []
            th.start()
            try:
                first = True
                while th.is_alive() or first:
                    q0 = time.perf_counter()
                    got = sweep(t)
                    calls.append((q0, time.perf_counter()))
                    same(got, R0, (directed, k, "beside"))
                    first = False
            finally:
                th.join()
            _, b0, b1 = rig.built(box)
            beside += sum(1 for q0, q1 in calls if q0 < b1 and q1 > b0)
            same(sweep(t), R0, (directed, k, "after the join"))
            slides += 1
        epoch = rig.built(box)[0]
    print(f"directed={directed}: {beside} sweeps beside {slides} concurrent slides")
    assert beside >= 3, (beside, slides)
    e.close()
