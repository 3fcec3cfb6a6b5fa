"""A forward track (dppr_ftrack_update) beside the graph update of the NEXT batch, on the rig of
tests/test_queries_beside_slide_gpu.py: two tracks with the same sets stand on epoch k - 1; one is moved to the explicitly named
epoch k while nothing else runs, the other while dppr_slide_concurrent builds epoch k + 1 -- further updates on its own epoch and
reads follow for as long as the slide runs. Bit for bit the two agree, and they are the numpy definition over the rows of epoch k
and the batch's records. After an exclusive slide that renumbers, both tracks follow to the new epoch all the same (the state is by
external id)."""
import threading
import time

import numpy as np
import pytest

from dynamicppr_amd import engine as eng
from tests import forward_ref as fr
from tests.test_forward_gpu import rows_of
from tests.test_ftrack_gpu import RefTrack
from tests.test_queries_beside_slide_gpu import Rig, V, hip, same  # noqa: F401  (hip: the fixture)

pytestmark = pytest.mark.gpu

BATCHES = 36
EPS, ROUNDS, K, M = 1e-6, 24, 64, 5
SETS = [0, 1, (np.array([2, 3, 5, 8]), np.array([0.5, 1.0, 2.0, 0.25])), V // 2, V - 1]


def shaped(rig, got, meta=True):
    out = {"at": [got["at_p"], got["at_r"]], "topk": [x for t in got["topk"] for x in t], "dense": [rig.hip.read(rig.d_dense, 8 * M * V, np.float64)]}
    if meta:
        out["meta"] = [got[x] for x in ("rounds_used", "converged", "rem", "pushes", "left", "work", "fix")]
    return out


def advance(rig, t, epoch, meta=True):
    return shaped(rig, t.update(epoch, ROUNDS, k=K, at=rig.ids, dense_p_ptr=rig.d_dense, dtype=eng.F64, layout=eng.SOURCE_MAJOR), meta)


def restated(rig, ref):
    cols = ref.cols
    last = [c.last for c in cols]
    meta = [np.array([getattr(l, x) for l in last], dtype=t) for x, t in (("rounds_used", np.int32), ("converged", np.int32), ("rem", np.float64),
                                                                          ("pushes", np.int64), ("left", np.int64))]
    from tests import ftrack_ref as tr
    return {"meta": meta + [tr.work(ref.rows, last), np.array(last[0].fix, dtype=np.int64)],
            "at": [np.stack([c.p[rig.ids] for c in cols]), np.stack([c.r[rig.ids] for c in cols])],
            "topk": [x for c in cols for x in fr.topk(c.p, K)],
            "dense": [np.stack([c.p for c in cols]).reshape(-1)]}


@pytest.mark.parametrize("directed", [1, 0])
def test_a_track_update_beside_a_concurrent_slide(hip, directed):
    rig = Rig(directed, hip, BATCHES, full=False)
    e = rig.e
    quiet, busy = e.ftrack(SETS, EPS, ROUNDS), e.ftrack(SETS, EPS, ROUNDS)
    ref = RefTrack(rows_of(e, 0), SETS, EPS, ROUNDS)
    box = []
    rig.build(1, False, box)
    epoch = rig.built(box)[0]
    beside = slides = followed = 0
    for k in range(1, BATCHES):
        rig.update(epoch)
        rig.probe(k)
        ref.rows = rows_of(e, epoch)
        ref.update(ref.rows, rig.stage[k - 1]["b"], ROUNDS)
        R0 = advance(rig, quiet, epoch)
        same(R0, restated(rig, ref), (directed, k, "numpy"))
        box = []
        if e.renumbering_due():
            before = e.id_space()["renumberings"]
            same(advance(rig, busy, epoch), R0, (directed, k, "before the exclusive slide"))
            rig.build(k + 1, False, box)
            followed += int(e.id_space()["renumberings"] > before)
        else:
            th = threading.Thread(target=rig.build, args=(k + 1, True, box))
            calls = []
            th.start()
            try:
                first = True
                while th.is_alive() or first:
                    q0 = time.perf_counter()
                    got = advance(rig, busy, epoch, meta=first)   # (later calls: more rounds on the own epoch -- none is left to do)
                    calls.append((q0, time.perf_counter()))
                    same(got, R0 if first else {x: R0[x] for x in got}, (directed, k, "beside"))
                    first = False
            finally:
                th.join()
            _, b0, b1 = rig.built(box)
            beside += sum(1 for q0, q1 in calls if q0 < b1 and q1 > b0)
            after = shaped(rig, busy.read(k=K, at=rig.ids, dense_p_ptr=rig.d_dense, dtype=eng.F64, layout=eng.SOURCE_MAJOR))
            same({x: after[x] for x in ("at", "topk", "dense")}, {x: R0[x] for x in ("at", "topk", "dense")}, (directed, k, "after the join"))
            slides += 1
        epoch = rig.built(box)[0]
        assert quiet.info()["epoch"] == busy.info()["epoch"] == epoch - 1
    print(f"directed={directed}: {beside} track calls beside {slides} concurrent slides, followed {followed} renumberings")
    assert beside >= 3 and followed >= 1, (beside, slides, followed)
    e.close()
