"""dppr_sample / dppr_group_sample beside the graph update of the NEXT batch, on the rig and by the method of
tests/test_position_beside_slide_gpu.py (churn stream, W = 600, c = 60, two resident epochs, renumbering at 8 % / 8 parked; a slot, a
10-source group and a 5-lane set group on ONE engine, the four specs of its ranked family). A graph update changes no solver state,
so -- in the caller's ids -- the draws, their weights, the totals, supports and statuses are, bit for bit, the quiet result BEFORE,
DURING and AFTER the concurrent slide of batch k + 1, also where that batch revives a parked vertex (its internal id changes, its
rows move: the tree is in EXTERNAL id order). After an exclusive slide that renumbers, the specs that read the epoch's CSR are
refused as "epoch not resident" and the others still give the quiet result. The quiet result is the numpy restatement
(tests/sample_ref.py) over the dense reads and the epoch's out-CSR by external id. The epoch of the last update is always named."""
import threading
import time

import numpy as np
import pytest

from tests import rank_ref, sample_ref
from tests.test_queries_beside_slide_gpu import IN, OUT, S, Rig, V, eq, hip, refused  # noqa: F401  (hip: the fixture of that module)

pytestmark = pytest.mark.gpu

BATCHES = 20
DRAWS = 300
MIN_SCORES = (0.0, 1e-6)
SEED, FIRST = 0x1234567800000007, 2 ** 32 - 100


def handles(rig):
    return ["slot"] + rig.wide


def family(rig, epoch, resident=True):
    """{(spec, handle, min_score): [ids, w, total, support, status]}; after a renumbering (resident False) the specs that read the
    CSR are refused."""
    e, out = rig.e, {}
    for what, spec in rig.specs.items():
        for h in handles(rig):
            kind, hd, _, _ = rig.handles[h]
            for ms in MIN_SCORES:
                if kind == "slot":
                    call = lambda: [np.asarray(x) for x in e.sample(hd, DRAWS, spec, ms, SEED, FIRST, True, epoch)]   # noqa: E731
                else:
                    call = lambda: list(e.group_sample(hd, DRAWS, spec, ms, SEED, FIRST, True, epoch))   # noqa: E731
                if resident or what not in rig.graph_specs:
                    out[(what, h, ms)] = call()
                else:
                    refused(call)
    return out


def same(got, want, tag, partial=False):
    assert got.keys() <= want.keys() if partial else got.keys() == want.keys(), tag
    for key in got:
        for j, (a, b) in enumerate(zip(got[key], want[key])):
            assert eq(a, b), (tag, key, j, np.asarray(a).ravel()[:6], np.asarray(b).ravel()[:6])


def restated(rig, epoch):
    D = rig.dense()
    row, col = rig.e.read_out_graph(epoch)
    tails, heads = rank_ref.edges(row, col)
    deg = rank_ref.out_degree(V, tails)
    out = {}
    for what in rig.specs:
        for h in handles(rig):
            cols = D[h][0]
            if what == "null":
                sc = rank_ref.scores(cols)
            elif what == "deg, every exclusion":
                sc = rank_ref.scores(cols, rank_ref.DEG, outdeg=deg, excl=rank_ref.excluded(V, tails, heads, rig.handles[h][3], S | IN | OUT))
            elif what == "inv_deg, deny":
                sc = rank_ref.scores(cols, rank_ref.INV_DEG, outdeg=deg, deny=rig.mask)
            else:
                assert what == "dev f32, allow"
                sc = rank_ref.scores(cols, rank_ref.DEV, g=rig.g32, allow=rig.mask)
            for ms in MIN_SCORES:
                ids, w, total, support, status = sample_ref.group_sample(np.stack(sc, axis=1), DRAWS, ms, SEED, FIRST)
                if h == "slot":
                    out[(what, h, ms)] = [ids[0], w[0], np.asarray(total[0]), np.asarray(int(support[0])), np.asarray(int(status[0]))]
                else:
                    out[(what, h, ms)] = [ids, w, total, support, status]
    return out


def test_draws_before_during_and_after_a_concurrent_slide(hip):
    directed = 1
    rig = Rig(directed, hip, BATCHES)
    e = rig.e
    box = []
    rig.build(1, False, box)
    epoch = rig.built(box)[0]
    beside = slides = exclusive = renumbered = 0
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
            same(R1, R0, (directed, k, "after the exclusive slide"), partial=bool(moved))
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
        epoch = rig.built(box)[0]
    print(f"{beside} passes of the family beside {slides} concurrent slides, {exclusive} exclusive slides ({renumbered} renumbered), {e.id_space()}")
    assert beside >= 1 and slides >= 1, (beside, slides)
    e.close()
