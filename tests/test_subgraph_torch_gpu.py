"""dynamicppr_amd/torch_bridge.py, group_subgraph: the top-k orders of a group and the stored edges among them as torch tensors on
the engine's device, against the host-destination call of the binding, exactly, and row_ptr / col indexing consistently. The GPU test
runs in ONE fresh child process (torch first, then the engine: one HIP runtime)."""
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

V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
W, c, directed, eps, n = 600, 20, 1, 1e-9, 10
sources = [int(x) for x in datagen.top_sources(V, e1, e2, W, directed, n)]
e = eng.Engine(V, W, directed, c)
e.load_window(e1[:W], e2[:W])
gid = e.add_source_group(sources)
e.group_init_solve(gid, eps)
dev = torch.device("cuda", e.device)
bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)

for k, min_p in ((1, 0.0), (65, 0.0), (8192, 0.0), (300, 1e-6)):
    h_cnt, h_off, h_ids, h_p, h_rp, h_col = e.group_subgraph(gid, k, min_p)
    out = tb.group_subgraph(e, gid, k, min_p)
    assert len(out) == 5 and all(isinstance(t, torch.Tensor) and t.device == dev for t in out), k
    cnt, ids, p, row_ptr, col = out
    assert (cnt.dtype, ids.dtype, p.dtype, row_ptr.dtype, col.dtype) == (torch.int32, torch.int32, torch.float64, torch.int64, torch.int32)
    assert tuple(cnt.shape) == (n,) and tuple(ids.shape) == (n, k) and tuple(p.shape) == (n, k) and tuple(row_ptr.shape) == (n, k + 1)
    assert np.array_equal(cnt.cpu().numpy(), h_cnt) and np.array_equal(ids.cpu().numpy(), h_ids)
    assert np.array_equal(bits(p.cpu().numpy()), bits(h_p)) and np.array_equal(row_ptr.cpu().numpy(), h_rp)
    assert np.array_equal(col.cpu().numpy(), h_col) and col.numel() == int(h_off[n])
    # row_ptr and col index consistently: rows follow each other without a gap, source by source, and hold positions below the count
    flat = row_ptr.cpu().numpy()
    assert flat[0, 0] == 0 and flat[-1, -1] == col.numel() and np.all(np.diff(flat, axis=1) >= 0) and np.all(flat[1:, 0] == flat[:-1, -1])
    if col.numel():
        owner = torch.bucketize(torch.arange(col.numel(), device=dev), row_ptr[:, -1].contiguous(), right=True)
        assert int(owner.max()) < n and bool(torch.all(col < cnt[owner])) and bool(torch.all(col >= 0))
    if k == 8192:
        assert col.numel() > 50 and int(cnt.max()) < k

for bad_k in (0, 8193):
    try:
        tb.group_subgraph(e, gid, bad_k)
    except eng.DpprError:
        continue
    raise AssertionError(f"k = {bad_k} was accepted")
e.close()
print("subgraph bridge ok")
"""


@pytest.mark.gpu
def test_group_subgraph_in_a_fresh_process():
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "subgraph bridge ok" in r.stdout, r.stdout[-3000:]
