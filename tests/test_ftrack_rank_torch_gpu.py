"""dynamicppr_amd/torch_bridge.py, ftrack_topk_ranked / ftrack_position_at / ftrack_sample: factor and mask tensors on the engine's
device handed to the ranked queries over a forward track, against the binding's own calls with the spec the bridge builds, bit for
bit, and against numpy (tests/ftrack_rank_ref.py) after a create and after two batches; the samples come back as tensors on the
engine's device; arguments the calls cannot take raise before the engine is called. The GPU test runs in ONE fresh child process
(torch first, then the engine: one HIP runtime)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import numpy as np
import torch
from dynamicppr_amd import torch_bridge as tb
from dynamicppr_amd import datagen, engine as eng
from dynamicppr_amd.stream import SlidingStream, Workload
from tests import forward_ref as fr
from tests import ftrack_ref as tr
from tests import ftrack_rank_ref as frr
from tests.ftrack_rank_ref import bits

V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
W, c, S = 600, 20, 300
g = SlidingStream(V, e1, e2, 1, Workload(W, c, 0, 0))
e = eng.Engine(V, W, 1, c)
e.load_window(*g.serialize_edge_stream())
dev = torch.device("cuda", e.device)
rows_now = lambda: fr.Rows(V, *e.read_graph()[:2], e.id_map())
rows = rows_now()
x2i = e.id_map()
named = np.nonzero((x2i >= 0) & (rows.d > 0))[0]
unnamed = int(np.nonzero(x2i < 0)[0][0])
sets = [int(named[0]), (np.array([named[7], unnamed, named[2]]), np.array([0.5, 1.5, 2.0])), unnamed, int(named[-1]), int(np.argmax(rows.d))]
as_set = lambda s: ((np.array([s]), np.ones(1)) if np.isscalar(s) else s)
seeds = [np.asarray(as_set(s)[0], dtype=np.int64) for s in sets]
m = len(sets)
t = e.ftrack(sets, 1e-6, 64)
cols = [tr.Column(rows, *as_set(s), 1e-6, 64) for s in sets]
rng = np.random.default_rng(4)
allow = rng.random(V) < 0.6
deny = (rng.random(V) < 0.3).astype(np.uint8) * 9
g32 = (rng.random(V) * 3.0 - 0.5).astype(np.float32)
g32[rng.random(V) < 0.1] = 0.0
to = lambda a: torch.from_numpy(a).to(dev)
d_allow, d_deny, d_g32 = to(allow), to(deny), to(g32)
both = ((d_allow != 0) & (d_deny == 0)).to(torch.uint8).contiguous()
spec = eng.Engine.rank_spec
ids = np.concatenate([np.arange(V), [unnamed, unnamed, 3]]).astype(np.int32)
for step in range(3):
    if step:
        assert not g.stream_updates()
        rec = tuple(x.copy() for x in g.batch_arrays())
        e.set_batch(*rec)
        ep = e.slide(*g.new_arrays())
        rows = rows_now()
        for col in cols:
            col.update(rows, rec, 64)
        t.update(ep, 64)
    graph = frr.Graph(V, *e.read_out_graph())
    p = [col.p for col in cols]
    cases = [(dict(), None, dict()),
             (dict(allow=d_allow, deny=d_deny), spec(mask=eng.MASK_ALLOW, mask_dev=both.data_ptr()), dict(allow=allow, deny=deny)),
             (dict(factor=d_g32, deny=d_deny, exclude=("seeds",)), spec(eng.FACTOR_DEV, d_g32.data_ptr(), eng.F32, eng.MASK_DENY, d_deny.data_ptr(), 1),
              dict(factor=frr.DEV, g=g32, deny=deny, exclude=1)),
             (dict(factor="deg", exclude=("seeds", "out")), spec(eng.FACTOR_DEG, exclude=5), dict(factor=frr.DEG, exclude=5)),
             (dict(factor="inv_deg", allow=d_allow, exclude=("seeds", "in", "out")), spec(eng.FACTOR_INV_DEG, mask=eng.MASK_ALLOW, mask_dev=d_allow.view(torch.uint8).data_ptr(), exclude=7),
              dict(factor=frr.INV_DEG, allow=allow, exclude=7))]
    for kw, sp, ref_kw in cases:
        want = frr.scores(p, seeds, graph, **ref_kw)
        for ms in (0.0, 1e-4):
            top = tb.ftrack_topk_ranked(e, t, 25, ms, **kw)
            mine = t.topk_ranked(25, ms, sp)
            assert len(top) == m
            for i in range(m):
                wi, ws = frr.topk(want[i], 25, ms)
                assert np.array_equal(top[i][0], wi) and np.array_equal(bits(top[i][1]), bits(ws)), (step, list(kw), ms, i)
                assert np.array_equal(top[i][0], mine[i][0]) and np.array_equal(bits(top[i][1]), bits(mine[i][1]))
            pos, cnt = tb.ftrack_position_at(e, t, torch.from_numpy(ids).to(dev), ms, **kw)
            assert pos.dtype == torch.int32 and cnt.dtype == torch.int32 and pos.device.type == "cpu" and tuple(pos.shape) == (len(ids), m)
            wpos, wcnt = frr.positions(want, ids, ms)
            assert np.array_equal(pos.numpy(), wpos) and np.array_equal(cnt.numpy(), wcnt), (step, list(kw), ms)
            hpos, hcnt = t.position_at(ids, sp, ms)
            assert np.array_equal(pos.numpy(), hpos) and np.array_equal(cnt.numpy(), hcnt)
            sid, sw, total, support, status = tb.ftrack_sample(e, t, S, ms, 0xABCDEF0123456789, 2 ** 32 - 3, **kw)
            assert isinstance(sid, torch.Tensor) and sid.dtype == torch.int32 and sid.device == dev and tuple(sid.shape) == (m, S)
            assert isinstance(sw, torch.Tensor) and sw.dtype == torch.float64 and sw.device == dev and tuple(sw.shape) == (m, S)
            assert total.dtype == torch.float64 and support.dtype == torch.int32 and status.dtype == torch.int32 and total.device.type == "cpu"
            rid, rw, rt, rs, rst = frr.sample(want, S, ms, 0xABCDEF0123456789, 2 ** 32 - 3)
            assert np.array_equal(sid.cpu().numpy(), rid) and np.array_equal(bits(sw.cpu().numpy()), bits(rw)), (step, list(kw), ms)
            assert np.array_equal(bits(total.numpy()), bits(rt)) and np.array_equal(support.numpy(), rs) and np.array_equal(status.numpy(), rst)
            hid, hw, ht, hs, hst = t.sample(S, sp, ms, 0xABCDEF0123456789, 2 ** 32 - 3)   # the host-destination call with the spec the bridge builds
            assert np.array_equal(sid.cpu().numpy(), hid) and np.array_equal(bits(sw.cpu().numpy()), bits(hw)) and np.array_equal(bits(total.numpy()), bits(ht))
    assert tb.ftrack_topk_ranked(e, t, 5)[2][0].tolist() == [unnamed] and len(tb.ftrack_topk_ranked(e, t, 5, exclude="seeds")[2][0]) == 0
sid, sw, total, support, status = tb.ftrack_sample(e, t, S, with_w=False)
assert sw is None and np.array_equal(sid.cpu().numpy(), t.sample(S)[0])
sid, sw, total, support, status = tb.ftrack_sample(e, t, 0)
assert tuple(sid.shape) == (m, 0) and np.array_equal(bits(total.numpy()), bits(t.sample(0)[2]))
closed = e.ftrack([int(named[0])], 1e-4, 4)
closed.close()
for fn, args, kw in ((tb.ftrack_topk_ranked, (closed, 5), {}), (tb.ftrack_topk_ranked, (3, 5), {}), (tb.ftrack_position_at, (closed, [1]), {}),
                     (tb.ftrack_sample, (closed, 4), {}), (tb.ftrack_sample, (t, -1), {}), (tb.ftrack_sample, (t, eng.SAMPLE_MAX + 1), {}),
                     (tb.ftrack_topk_ranked, (t, 5), dict(factor="degree")), (tb.ftrack_topk_ranked, (t, 5), dict(exclude=("up",))),
                     (tb.ftrack_topk_ranked, (t, 5), dict(allow=d_allow.cpu())), (tb.ftrack_position_at, (t, torch.zeros(3, device=dev)), {}),
                     (tb.ftrack_sample, (t, 4), dict(factor=d_g32[:-1]))):
    try:
        fn(e, *args, **kw)
    except (eng.DpprError, ValueError) as err:
        assert fn.__name__ in str(err), err
        continue
    raise AssertionError(f"{fn.__name__} {args} {kw} was accepted")
t.close()
e.close()
print("forward rank bridge ok")
"""


@pytest.mark.gpu
def test_ftrack_rank_bridge_in_a_fresh_process():
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "forward rank bridge ok" in r.stdout, r.stdout[-3000:]
