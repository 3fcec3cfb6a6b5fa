"""dynamicppr_amd/torch_bridge.py, group_position_at: factor and mask tensors on the engine's device handed to
dppr_group_position_at, against the engine call with the same spec and against the numpy restatement of tests/position_ref.py,
integer for integer; int32 CPU tensors come back; a tensor that is not what the call can read raises ValueError before the engine
is called. The GPU test runs in ONE fresh child process (torch first, then the engine: one HIP runtime)."""
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
from tests import position_ref, rank_ref

V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
W, c, directed, eps, n = 600, 20, 0, 1e-9, 10
sources = [int(x) for x in datagen.top_sources(V, e1, e2, W, directed, n)]
e = eng.Engine(V, W, directed, c)
e.load_window(e1[:W], e2[:W])
gid = e.add_source_group(sources)
e.group_init_solve(gid, eps)
dev = torch.device("cuda", e.device)
cols = [e.group_read(gid, i)[0] for i in range(n)]
tails, heads = rank_ref.edges(*e.read_out_graph())
deg = rank_ref.out_degree(V, tails)
seeds = [[s] for s in sources]
rng = np.random.default_rng(4)
allow = rng.random(V) < 0.5
deny = (rng.random(V) < 0.3).astype(np.uint8) * 9
g64 = rng.random(V) * 3.0
g64[rng.random(V) < 0.1] = 0.0
g32 = g64.astype(np.float32)
ids = rng.integers(0, V, 300).astype(np.int32)
t = lambda a: torch.from_numpy(a).to(dev)

def same(got, want, spec, ms, what):
    pos, cnt = got
    assert isinstance(pos, torch.Tensor) and pos.dtype == torch.int32 and pos.device.type == "cpu" and tuple(pos.shape) == (len(ids), n), what
    assert isinstance(cnt, torch.Tensor) and cnt.dtype == torch.int32 and cnt.device.type == "cpu" and tuple(cnt.shape) == (n,), what
    wp, wc = position_ref.group_positions(want, ids, ms)
    assert np.array_equal(pos.numpy(), wp) and np.array_equal(cnt.numpy(), wc), what
    ep, ec = e.group_position_at(gid, ids, spec, ms)   # the engine call with the spec the bridge builds
    assert np.array_equal(pos.numpy(), ep) and np.array_equal(cnt.numpy(), ec), what

d_allow, d_deny, d_g64, d_g32 = t(allow), t(deny), t(g64), t(g32)
both = ((d_allow != 0) & (d_deny == 0)).to(torch.uint8).contiguous()
ex_all = rank_ref.excluded(V, tails, heads, seeds, 7)
ex_seeds = rank_ref.excluded(V, tails, heads, seeds, 1)
spec = eng.Engine.rank_spec
for ms in (0.0, 1e-4):
    same(tb.group_position_at(e, gid, ids, ms), rank_ref.scores(cols), None, ms, "plain")
    same(tb.group_position_at(e, gid, torch.from_numpy(ids), ms, allow=d_allow), rank_ref.scores(cols, allow=allow),
         spec(mask=eng.MASK_ALLOW, mask_dev=d_allow.view(torch.uint8).data_ptr()), ms, "bool allow, ids as a tensor")
    same(tb.group_position_at(e, gid, t(ids).to(torch.int64), ms, allow=d_allow, deny=d_deny), rank_ref.scores(cols, allow=allow, deny=deny),
         spec(mask=eng.MASK_ALLOW, mask_dev=both.data_ptr()), ms, "both masks, ids on the device")
    same(tb.group_position_at(e, gid, ids.tolist(), ms, factor=d_g64), rank_ref.scores(cols, rank_ref.DEV, g=g64),
         spec(eng.FACTOR_DEV, d_g64.data_ptr()), ms, "float64 factor, ids as a list")
    same(tb.group_position_at(e, gid, ids, ms, factor=d_g32, deny=d_deny, exclude=("seeds",)),
         rank_ref.scores(cols, rank_ref.DEV, g=g32, deny=deny, excl=ex_seeds),
         spec(eng.FACTOR_DEV, d_g32.data_ptr(), eng.F32, eng.MASK_DENY, d_deny.data_ptr(), 1), ms, "float32 factor, deny, seeds")
    same(tb.group_position_at(e, gid, ids, ms, factor="deg", exclude=("seeds", "in", "out")),
         rank_ref.scores(cols, rank_ref.DEG, outdeg=deg, excl=ex_all), spec(eng.FACTOR_DEG, exclude=7), ms, "deg, all flags")
    same(tb.group_position_at(e, gid, ids, ms, factor="inv_deg", exclude="in"),
         rank_ref.scores(cols, rank_ref.INV_DEG, outdeg=deg, excl=rank_ref.excluded(V, tails, heads, seeds, 2)),
         spec(eng.FACTOR_INV_DEG, exclude=2), ms, "inv_deg, in")
pos, cnt = tb.group_position_at(e, gid, [])
assert tuple(pos.shape) == (0, n) and np.array_equal(cnt.numpy(), position_ref.group_positions(cols, [])[1])

bad = [dict(factor=torch.from_numpy(g64)),                       # a CPU tensor
       dict(allow=torch.from_numpy(allow)), dict(deny=torch.from_numpy(deny)),
       dict(factor=t(g64[:-1])), dict(allow=t(allow[:-1])),      # the wrong length
       dict(factor=t(np.repeat(g64, 2))[::2]),                   # not contiguous
       dict(factor=t(g64).to(torch.float16)), dict(allow=t(g64)),   # the wrong dtype
       dict(factor="degree"), dict(exclude=("seeds", "both")), dict(allow=allow)]
for kw in bad:
    try:
        tb.group_position_at(e, gid, ids, **kw)
    except ValueError as err:
        assert "group_position_at" in str(err), err
        continue
    raise AssertionError(f"{list(kw)} was accepted")
for wrong in (torch.from_numpy(ids.astype(np.float32)), torch.from_numpy(ids.reshape(2, -1))):
    try:
        tb.group_position_at(e, gid, wrong)
    except ValueError:
        continue
    raise AssertionError("ids that are no 1-D integer tensor were accepted")
e.close()
print("position bridge ok")
"""


@pytest.mark.gpu
def test_group_position_at_in_a_fresh_process():
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "position bridge ok" in r.stdout, r.stdout[-3000:]
