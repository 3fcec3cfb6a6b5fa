"""dynamicppr_amd/torch_bridge.py, forward_push: the dense p and r of dppr_forward_push as tensors on the engine's device, float64
bit for bit and float32 rounded once, in both layouts, against the numpy restatement of tests/fpush_ref.py; the statistics come
back as CPU tensors; r goes straight into group_dot; arguments the call cannot take raise DpprError before the engine is called.
The GPU test runs in ONE fresh child process (torch first, then the engine: one HIP runtime)."""
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
from tests import fpush_ref as pr

bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
W, c = 600, 20
e = eng.Engine(V, W, 1, c)
e.load_window(e1[:W], e2[:W])
dev = torch.device("cuda", e.device)
row, col, _ = e.read_graph()
x2i = e.id_map()
rows = fr.Rows(V, row, col, x2i)
rowless = pr.rowless_mask(rows)
named = np.nonzero((x2i >= 0) & (rows.d > 0))[0]
unnamed = int(np.nonzero(x2i < 0)[0][0])
sets = [int(named[0]), (np.array([named[7], unnamed, named[2]]), np.array([0.5, 1.5, 2.0])), unnamed, int(named[-1]), int(named[0])]
for eps, max_rounds in ((1e-5, 64), (1e-7, 5)):
    want = [pr.push(rows, rowless, *((s, 1.0) if np.isscalar(s) else s), eps, max_rounds) for s in sets]
    full = {"p": np.stack([w.p for w in want]), "r": np.stack([w.r for w in want])}
    for layout in ("source_major", "vertex_major"):
        p, r, info = tb.forward_push(e, sets, eps, max_rounds, layout=layout)
        for name, t in (("p", p), ("r", r)):
            assert isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.device == dev
            assert tuple(t.shape) == ((5, V) if layout == "source_major" else (V, 5))
            got = t.cpu().numpy() if layout == "source_major" else t.cpu().numpy().T
            assert np.array_equal(bits(got), bits(full[name])), (name, layout)
        assert info["rounds_used"].dtype == torch.int32 and info["pushes"].dtype == torch.int64 and info["rem"].device.type == "cpu"
        for key in ("rounds_used", "converged", "pushes", "left"):
            assert info[key].numpy().tolist() == [getattr(w, key) for w in want], key
        assert np.array_equal(bits(info["rem"].numpy()), bits([w.rem for w in want]))
        assert info["work"].numpy().tolist() == pr.work(rows, want).tolist()
        p32, r32, _ = tb.forward_push(e, sets, eps, max_rounds, dtype=torch.float32, layout=layout)
        for name, t in (("p", p32), ("r", r32)):
            assert t.dtype == torch.float32 and t.device == dev
            got32 = t.cpu().numpy() if layout == "source_major" else t.cpu().numpy().T
            assert np.array_equal(got32.view(np.uint32), full[name].astype(np.float32).view(np.uint32)), (name, layout)
# r is the seed distribution of the bidirectional estimate
gid = e.add_source_group([int(named[0]), int(named[5])])
e.group_init_solve(gid, 1e-9)
p, r, info = tb.forward_push(e, sets, 1e-5, 64)
dot = tb.group_dot(e, gid, r)
assert tuple(dot.shape) == (5, 2) and float(dot.min()) >= 0.0
for kw in (dict(dtype=torch.float16), dict(layout="rows"), dict(sets=[]), dict(sets=list(range(17)))):
    args = dict(sets=sets)
    args.update(kw)
    try:
        tb.forward_push(e, args.pop("sets"), 1e-5, **args)
    except eng.DpprError as err:
        assert "forward_push" in str(err), err
        continue
    raise AssertionError(f"{list(kw)} was accepted")
e.close()
print("forward push bridge ok")
"""


@pytest.mark.gpu
def test_forward_push_in_a_fresh_process():
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "forward push bridge ok" in r.stdout, r.stdout[-3000:]
