"""dynamicppr_amd/torch_bridge.py, group_topk_ranked: factor and mask tensors on the engine's device handed to
dppr_group_topk_ranked, against the numpy restatement of tests/rank_ref.py, exactly; a tensor that is not what the call can read
raises ValueError before the engine is called. The GPU test runs in ONE fresh child process (torch first, then the engine: one HIP
runtime)."""
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
from tests import rank_ref

V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
W, c, directed, eps, n = 600, 20, 0, 1e-9, 10
sources = [int(x) for x in datagen.top_sources(V, e1, e2, W, directed, n)]
e = eng.Engine(V, W, directed, c)
e.load_window(e1[:W], e2[:W])
gid = e.add_source_group(sources)
e.group_init_solve(gid, eps)
dev = torch.device("cuda", e.device)
bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
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

def same(got, want, k, what):
    assert len(got) == n, what
    for i, (gi, gs) in enumerate(got):
        wi, ws = rank_ref.topk(want[i], k)
        assert np.array_equal(gi, wi) and np.array_equal(bits(gs), bits(ws)), (what, i, k)

t = lambda a: torch.from_numpy(a).to(dev)
ex_all = rank_ref.excluded(V, tails, heads, seeds, 7)
ex_seeds = rank_ref.excluded(V, tails, heads, seeds, 1)
for k in (10, 8192):
    same(tb.group_topk_ranked(e, gid, k), rank_ref.scores(cols), k, "plain")
    same(tb.group_topk_ranked(e, gid, k, allow=t(allow)), rank_ref.scores(cols, allow=allow), k, "bool allow")
    same(tb.group_topk_ranked(e, gid, k, deny=t(deny)), rank_ref.scores(cols, deny=deny), k, "uint8 deny")
    same(tb.group_topk_ranked(e, gid, k, allow=t(allow), deny=t(deny)), rank_ref.scores(cols, allow=allow, deny=deny), k, "both masks")
    same(tb.group_topk_ranked(e, gid, k, factor=t(g64)), rank_ref.scores(cols, rank_ref.DEV, g=g64), k, "float64 factor")
    same(tb.group_topk_ranked(e, gid, k, factor=t(g32), deny=t(deny), exclude=("seeds",)),
         rank_ref.scores(cols, rank_ref.DEV, g=g32, deny=deny, excl=ex_seeds), k, "float32 factor, deny, seeds")
    same(tb.group_topk_ranked(e, gid, k, factor="deg", exclude=("seeds", "in", "out")),
         rank_ref.scores(cols, rank_ref.DEG, outdeg=deg, excl=ex_all), k, "deg, all flags")
    same(tb.group_topk_ranked(e, gid, k, factor="inv_deg", exclude="in", min_score=0.0),
         rank_ref.scores(cols, rank_ref.INV_DEG, outdeg=deg, excl=rank_ref.excluded(V, tails, heads, seeds, 2)), k, "inv_deg, in")

bad = [dict(factor=torch.from_numpy(g64)),                       # a CPU tensor
       dict(allow=torch.from_numpy(allow)), dict(deny=torch.from_numpy(deny)),
       dict(factor=t(g64[:-1])), dict(allow=t(allow[:-1])),      # the wrong length
       dict(factor=t(np.stack([g64, g64]))),                     # the wrong shape
       dict(factor=t(np.repeat(g64, 2))[::2]),                   # not contiguous
       dict(factor=t(g64).to(torch.float16)), dict(allow=t(g64)), dict(deny=t(deny).to(torch.int32)),   # the wrong dtype
       dict(factor="degree"), dict(factor=3), dict(exclude=("seeds", "both")), dict(allow=allow)]
for kw in bad:
    try:
        tb.group_topk_ranked(e, gid, 10, **kw)
    except ValueError:
        continue
    raise AssertionError(f"{list(kw)} was accepted")
e.close()
print("rank bridge ok")
"""


@pytest.mark.gpu
def test_group_topk_ranked_in_a_fresh_process():
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "rank bridge ok" in r.stdout, r.stdout[-3000:]
