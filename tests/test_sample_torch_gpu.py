"""dynamicppr_amd/torch_bridge.py, group_sample: factor and mask tensors on the engine's device handed to dppr_group_sample with a
device destination, against the host-destination engine call with the same spec and against the numpy restatement of
tests/sample_ref.py, bit for bit; ids (int32) and w (float64) come back as tensors on the engine's device; a tensor that is not
what the call can read raises ValueError before the engine is called, and a device out_ids that is too small is refused by the
engine with nothing written. The GPU test runs in ONE fresh child process (torch first, then the engine: one HIP runtime)."""
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
from tests import rank_ref, sample_ref
from tests.sample_ref import bits

V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
W, c, directed, eps, n, S = 600, 20, 0, 1e-9, 10, 500
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
g32 = (rng.random(V) * 3.0).astype(np.float32)
g32[rng.random(V) < 0.1] = 0.0
t = lambda a: torch.from_numpy(a).to(dev)

def same(got, want, spec, ms, seed, first, what):
    ids, w, total, support, status = got
    assert isinstance(ids, torch.Tensor) and ids.dtype == torch.int32 and ids.device == dev and tuple(ids.shape) == (n, S), what
    assert isinstance(w, torch.Tensor) and w.dtype == torch.float64 and w.device == dev and tuple(w.shape) == (n, S), what
    assert total.dtype == torch.float64 and support.dtype == torch.int32 and status.dtype == torch.int32 and total.device.type == "cpu", what
    rid, rw, rt, rs, rst = sample_ref.group_sample(np.stack(want, axis=1), S, ms, seed, first)
    assert np.array_equal(ids.cpu().numpy(), rid) and np.array_equal(bits(w.cpu().numpy()), bits(rw)), what
    assert np.array_equal(bits(total.numpy()), bits(rt)) and np.array_equal(support.numpy(), rs) and np.array_equal(status.numpy(), rst), what
    hid, hw, ht, hs, hst = e.group_sample(gid, S, spec, ms, seed, first)   # the host-destination call with the spec the bridge builds
    assert np.array_equal(ids.cpu().numpy(), hid) and np.array_equal(bits(w.cpu().numpy()), bits(hw)) and np.array_equal(bits(total.numpy()), bits(ht)), what

d_allow, d_deny, d_g32 = t(allow), t(deny), t(g32)
both = ((d_allow != 0) & (d_deny == 0)).to(torch.uint8).contiguous()
ex_all = rank_ref.excluded(V, tails, heads, seeds, 7)
spec = eng.Engine.rank_spec
for ms, seed, first in ((0.0, 0, 0), (1e-4, 0xABCDEF0123456789, 2 ** 32 - 3)):
    same(tb.group_sample(e, gid, S, ms, seed, first), rank_ref.scores(cols), None, ms, seed, first, "plain")
    same(tb.group_sample(e, gid, S, ms, seed, first, allow=d_allow, deny=d_deny), rank_ref.scores(cols, allow=allow, deny=deny),
         spec(mask=eng.MASK_ALLOW, mask_dev=both.data_ptr()), ms, seed, first, "both masks")
    same(tb.group_sample(e, gid, S, ms, seed, first, factor=d_g32, deny=d_deny, exclude=("seeds",)),
         rank_ref.scores(cols, rank_ref.DEV, g=g32, deny=deny, excl=rank_ref.excluded(V, tails, heads, seeds, 1)),
         spec(eng.FACTOR_DEV, d_g32.data_ptr(), eng.F32, eng.MASK_DENY, d_deny.data_ptr(), 1), ms, seed, first, "float32 factor, deny, seeds")
    same(tb.group_sample(e, gid, S, ms, seed, first, factor="deg", exclude=("seeds", "in", "out")),
         rank_ref.scores(cols, rank_ref.DEG, outdeg=deg, excl=ex_all), spec(eng.FACTOR_DEG, exclude=7), ms, seed, first, "deg, all flags")
ids, w, total, support, status = tb.group_sample(e, gid, S, with_w=False)
assert w is None and np.array_equal(ids.cpu().numpy(), e.group_sample(gid, S)[0])
ids, w, total, support, status = tb.group_sample(e, gid, 0)
assert tuple(ids.shape) == (n, 0) and np.array_equal(bits(total.numpy()), bits(e.group_sample(gid, 0)[2]))

# a device out_ids that is too small is refused, and nothing is written
# (torch carves small tensors out of larger allocations; one of 12 MiB is an allocation of its own, of exactly that size)
cap = 12 * 1024 * 1024 // 4
S_big = cap // n + 1
assert n * S_big > cap and S_big <= eng.SAMPLE_MAX and n * S_big <= eng.SAMPLE_MAX_TOTAL
small = torch.full((cap,), 77, dtype=torch.int32, device=dev)
torch.cuda.synchronize(dev)
try:
    e.group_sample_dev(gid, S_big, small.data_ptr())
except eng.DpprError:
    pass
else:
    raise AssertionError("a device destination two elements short of n * S was accepted")
assert bool((small == 77).all())
del small
exact = torch.full((n * S,), 77, dtype=torch.int32, device=dev)
torch.cuda.synchronize(dev)
e.group_sample_dev(gid, S, exact.data_ptr())
assert np.array_equal(exact.cpu().numpy().reshape(n, S), e.group_sample(gid, S)[0])

bad = [dict(factor=torch.from_numpy(g32)), dict(allow=torch.from_numpy(allow)),   # CPU tensors
       dict(factor=t(g32[:-1])), dict(allow=t(allow[:-1])),                         # the wrong length
       dict(factor=t(np.repeat(g32, 2))[::2]),                                      # not contiguous
       dict(factor=t(g32).to(torch.float16)), dict(allow=t(g32)),                   # the wrong dtype
       dict(factor="degree"), dict(exclude=("seeds", "both")), dict(allow=allow)]
for kw in bad:
    try:
        tb.group_sample(e, gid, S, **kw)
    except ValueError as err:
        assert "group_sample" in str(err), err
        continue
    raise AssertionError(f"{list(kw)} was accepted")
e.close()
print("sample bridge ok")
"""


@pytest.mark.gpu
def test_group_sample_in_a_fresh_process():
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "sample bridge ok" in r.stdout, r.stdout[-3000:]
