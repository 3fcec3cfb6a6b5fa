"""dynamicppr_amd/torch_bridge.py, forward: the dense result of dppr_forward as a tensor on the engine's device, float64 bit for bit
and float32 rounded once, in both layouts, against Engine.forward's point reads over every id and against the numpy restatement of
tests/forward_ref.py; iters_used and rem come back as CPU tensors; arguments the call cannot take raise DpprError before the
engine is called. The GPU test runs in ONE fresh child process (torch first, then the engine: one HIP runtime)."""
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
from tests import forward_ref as fr

bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
W, c = 600, 20
e = eng.Engine(V, W, 1, c)
e.load_window(e1[:W], e2[:W])
dev = torch.device("cuda", e.device)
row, col, _ = e.read_graph()
x2i = e.id_map()
rows = fr.Rows(V, row, col, x2i)
named = np.nonzero((x2i >= 0) & (rows.d > 0))[0]
starts = np.array([named[0], named[7], np.nonzero(x2i < 0)[0][0], named[0], named[-1]], dtype=np.int32)
every = np.arange(V, dtype=np.int32)
for iters, tol in ((64, 0.0), (20, 1e-4)):
    host = e.forward(starts, iters, tol, at=every)
    want = [fr.forward(rows, int(q), iters, tol) for q in starts]
    full = np.stack([w[0] for w in want])
    assert np.array_equal(bits(host["at"]), bits(full))
    for layout in ("source_major", "vertex_major"):
        f, used, rem = tb.forward(e, starts, iters, tol, layout=layout)
        assert isinstance(f, torch.Tensor) and f.dtype == torch.float64 and f.device == dev
        assert tuple(f.shape) == ((5, V) if layout == "source_major" else (V, 5))
        got = f.cpu().numpy() if layout == "source_major" else f.cpu().numpy().T
        assert np.array_equal(bits(got), bits(host["at"])), layout
        assert used.dtype == torch.int32 and rem.dtype == torch.float64 and used.device.type == "cpu"
        assert np.array_equal(used.numpy(), host["iters_used"]) and np.array_equal(bits(rem.numpy()), bits(host["rem"]))
        assert used.numpy().tolist() == [w[2] for w in want] and np.array_equal(bits(rem.numpy()), bits([w[1] for w in want]))
        f32, _, _ = tb.forward(e, starts, iters, tol, dtype=torch.float32, layout=layout)
        assert f32.dtype == torch.float32 and f32.device == dev
        got32 = f32.cpu().numpy() if layout == "source_major" else f32.cpu().numpy().T
        assert np.array_equal(got32.view(np.uint32), full.astype(np.float32).view(np.uint32)), layout
one, used, rem = tb.forward(e, [int(named[3])], 8)
assert tuple(one.shape) == (1, V) and float(one.sum()) > 0.15
for kw in (dict(dtype=torch.float16), dict(layout="rows"), dict(starts=[]), dict(starts=list(range(17)))):
    args = dict(starts=starts)
    args.update(kw)
    try:
        tb.forward(e, args.pop("starts"), **args)
    except eng.DpprError as err:
        assert "forward" in str(err), err
        continue
    raise AssertionError(f"{list(kw)} was accepted")
e.close()
print("forward bridge ok")
"""


@pytest.mark.gpu
def test_forward_in_a_fresh_process():
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "forward bridge ok" in r.stdout, r.stdout[-3000:]
