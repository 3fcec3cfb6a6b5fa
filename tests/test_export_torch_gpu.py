"""dynamicppr_amd/torch_bridge.py: the state as torch tensors on the engine's device. The GPU test runs in ONE fresh child
process (torch first, then the engine: one HIP runtime); the CPU test holds that the engine binding stays torch-free."""
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
cols = [e.group_read(gid, i) for i in range(n)]
P, R = np.stack([x[0] for x in cols]), np.stack([x[1] for x in cols])
bits = lambda a, u: np.ascontiguousarray(a).view(u)
for min_p in (0.0, 1e-4):
    t = tb.group_sparse_csr(e, gid, min_p)
    assert t.layout == torch.sparse_csr and tuple(t.shape) == (n, V) and t.device.type == "cuda"
    assert t.col_indices().dtype == torch.int32 and t.values().dtype == torch.float64
    want = np.where(P > min_p, P, 0.0)
    assert np.array_equal(bits(t.to_dense().cpu().numpy(), np.uint64), bits(want, np.uint64)), min_p
    assert t.values().numel() == np.count_nonzero(P > min_p)
tp, tr = tb.group_sparse_csr(e, gid, 1e-6, with_r=True)
assert np.array_equal(bits(tr.to_dense().cpu().numpy(), np.uint64), bits(np.where(P > 1e-6, R, 0.0), np.uint64))
for which, M in (("p", P), ("r", R)):
    for dtype, np_t, np_u in ((torch.float64, np.float64, np.uint64), (torch.float32, np.float32, np.uint32)):
        for layout in ("source_major", "vertex_major"):
            d = tb.group_dense(e, gid, which, dtype, layout)
            want = (M if layout == "source_major" else M.T).astype(np_t)
            assert tuple(d.shape) == want.shape and d.dtype == dtype and d.device.type == "cuda"
            assert np.array_equal(bits(d.cpu().numpy(), np_u), bits(want, np_u)), (which, dtype, layout)
e.close()
print("bridge ok")
"""


@pytest.mark.gpu
def test_group_tensors_in_a_fresh_process():
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "bridge ok" in r.stdout, r.stdout[-3000:]


def test_the_bridge_keeps_torch_out_of_the_engine():
    """Importing the engine alone leaves torch unloaded; importing the bridge puts no torch into the engine module. (No GPU.)"""
    code = ("import sys\n"
            "from dynamicppr_amd import engine\n"
            "assert 'torch' not in sys.modules, 'engine.py imported torch'\n"
            "from dynamicppr_amd import torch_bridge\n"
            "assert 'torch' in sys.modules and not hasattr(engine, 'torch')\n"
            "assert callable(torch_bridge.group_sparse_csr) and callable(torch_bridge.group_dense)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:]
    text = open(os.path.join(ROOT, "dynamicppr_amd", "engine.py")).read()
    assert "torch" not in text
