"""The ranked, position and sample queries over a forward track (dppr_ftrack_topk_ranked / _position_at / _sample, with
dppr_ftrack_rank_score_at) beside the graph update of the NEXT batch, on the rig of tests/test_queries_beside_slide_gpu.py: a track
stands on epoch k; the three calls under a spec that reads degrees and both neighbour rows are taken while nothing else runs -- and
are the numpy definition over the rows of epoch k --, then again and again while dppr_slide_concurrent builds epoch k + 1. Bit for
bit the calls beside the slide equal the quiet ones."""
import threading
import time

import numpy as np
import pytest

from dynamicppr_amd import engine as eng
from tests import ftrack_rank_ref as frr
from tests.test_forward_gpu import rows_of
from tests.test_fpush_gpu import as_set
from tests.test_ftrack_gpu import RefTrack
from tests.test_queries_beside_slide_gpu import Rig, V, hip, same  # noqa: F401  (hip: the fixture)

pytestmark = pytest.mark.gpu

BATCHES = 30
EPS, ROUNDS = 1e-6, 24
SETS = [0, 1, (np.array([2, 3, 5, 8]), np.array([0.5, 1.0, 2.0, 0.25])), V // 2, V - 1]
FLAGS = eng.EXCLUDE_SEEDS | eng.EXCLUDE_IN_NEIGHBOURS | eng.EXCLUDE_OUT_NEIGHBOURS
IDS = np.arange(0, V, 3, dtype=np.int32)[:4096]
NS, SEED, FIRST = 200, 77, 2 ** 32 - 9


def queries(t):
    spec = eng.Engine.rank_spec(eng.FACTOR_DEG, exclude=FLAGS)
    top = t.topk_ranked(50, 0.0, spec)
    pos, cnt = t.position_at(IDS, spec)
    ids, w, total, support, status = t.sample(NS, spec, 0.0, SEED, FIRST)
    m = len(top)
    tid, tsc = np.full((m, 50), -1, dtype=np.int32), np.zeros((m, 50))
    for i, (a, b) in enumerate(top):
        tid[i, :len(a)], tsc[i, :len(a)] = a, b
    return {"topk": [tid, tsc], "position": [pos, cnt], "sample": [ids, w, total, support, status], "score_at": [t.rank_score_at(IDS, spec)]}


def restated(e, epoch, ref):
    graph = frr.Graph(V, *e.read_out_graph(epoch))
    want = frr.scores([c.p for c in ref.cols], [as_set(s)[0] for s in SETS], graph, factor=frr.DEG, exclude=FLAGS)
    m = len(want)
    tid, tsc = np.full((m, 50), -1, dtype=np.int32), np.zeros((m, 50))
    for i, s in enumerate(want):
        a, b = frr.topk(s, 50)
        tid[i, :len(a)], tsc[i, :len(a)] = a, b
    return {"topk": [tid, tsc], "position": list(frr.positions(want, IDS)), "sample": list(frr.sample(want, NS, 0.0, SEED, FIRST)),
            "score_at": [np.stack(want, axis=1)[IDS]]}


@pytest.mark.parametrize("directed", [1, 0])
def test_the_three_calls_beside_a_concurrent_slide(hip, directed):
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
        R0 = queries(t)
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
                    got = queries(t)
                    calls.append((q0, time.perf_counter()))
                    same(got, R0, (directed, k, "beside"))
                    first = False
            finally:
                th.join()
            _, b0, b1 = rig.built(box)
            beside += sum(1 for q0, q1 in calls if q0 < b1 and q1 > b0)
            same(queries(t), R0, (directed, k, "after the join"))
            slides += 1
        epoch = rig.built(box)[0]
    print(f"directed={directed}: {beside} query rounds beside {slides} concurrent slides")
    assert beside >= 3, (beside, slides)
    e.close()
