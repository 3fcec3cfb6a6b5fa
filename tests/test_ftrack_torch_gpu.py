"""dynamicppr_amd/torch_bridge.py, ftrack_read: the dense p and r of a forward track as tensors on the engine's device, float64 bit for
bit and float32 rounded once, in both layouts, against the numpy definition of tests/ftrack_ref.py after a create and after two
batches; the counts of the last call come back as CPU tensors; r goes straight into group_dot; arguments the call cannot take raise
DpprError before the engine is called. The GPU test runs in ONE fresh child process (torch first, then the engine: one HIP runtime)."""
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

bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
W, c = 600, 20
g = SlidingStream(V, e1, e2, 1, Workload(W, c, 0, 0))
e = eng.Engine(V, W, 1, c)
e.load_window(*g.serialize_edge_stream())
dev = torch.device("cuda", e.device)
rows_now = lambda: fr.Rows(V, *e.read_graph()[:2], e.id_map())
rows = rows_now()
x2i = e.id_map()
named = np.nonzero((x2i >= 0) & (rows.d > 0))[0]
unnamed = int(np.nonzero(x2i < 0)[0][0])
sets = [int(named[0]), (np.array([named[7], unnamed, named[2]]), np.array([0.5, 1.5, 2.0])), unnamed, int(named[-1]), int(named[0])]
as_set = lambda s: ((s, 1.0) if np.isscalar(s) else s)
t = e.ftrack(sets, 1e-6, 64)
cols = [tr.Column(rows, *as_set(s), 1e-6, 64) for s in sets]
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
    full = {"p": np.stack([w.p for w in cols]), "r": np.stack([w.r for w in cols])}
    for layout in ("source_major", "vertex_major"):
        p, r, info = tb.ftrack_read(e, t, layout=layout)
        for name, x in (("p", p), ("r", r)):
            assert isinstance(x, torch.Tensor) and x.dtype == torch.float64 and x.device == dev
            assert tuple(x.shape) == ((5, V) if layout == "source_major" else (V, 5))
            got = x.cpu().numpy() if layout == "source_major" else x.cpu().numpy().T
            assert np.array_equal(bits(got), bits(full[name])), (step, name, layout)
        assert info["rounds_used"].dtype == torch.int32 and info["pushes"].dtype == torch.int64 and info["rem"].device.type == "cpu"
        for key in ("rounds_used", "converged", "pushes", "left"):
            assert info[key].numpy().tolist() == [getattr(w.last, key) for w in cols], (step, key)
        assert np.array_equal(bits(info["rem"].numpy()), bits([w.last.rem for w in cols]))
        assert info["work"].numpy().tolist() == tr.work(rows, [w.last for w in cols]).tolist()
        assert info["fix"].numpy().tolist() == cols[0].last.fix
        p32, r32, _ = tb.ftrack_read(e, t, dtype=torch.float32, layout=layout)
        for name, x in (("p", p32), ("r", r32)):
            assert x.dtype == torch.float32 and x.device == dev
            got32 = x.cpu().numpy() if layout == "source_major" else x.cpu().numpy().T
            assert np.array_equal(got32.view(np.uint32), full[name].astype(np.float32).view(np.uint32)), (step, name, layout)
assert any(np.any(w.r < 0) for w in cols)   # a tracked r holds both signs
gid = e.add_source_group([int(named[0]), int(named[5])])
e.group_init_solve(gid, 1e-9)
p, r, info = tb.ftrack_read(e, t)
dot = tb.group_dot(e, gid, r)
assert tuple(dot.shape) == (5, 2)
closed = e.ftrack([int(named[0])], 1e-4, 4)
closed.close()
for args in ((t, dict(dtype=torch.float16)), (t, dict(layout="rows")), (closed, {}), (3, {})):
    try:
        tb.ftrack_read(e, args[0], **args[1])
    except eng.DpprError as err:
        assert "ftrack_read" in str(err), err
        continue
    raise AssertionError(f"{args} was accepted")
t.close()
e.close()
print("forward track bridge ok")
"""


@pytest.mark.gpu
def test_ftrack_read_in_a_fresh_process():
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "forward track bridge ok" in r.stdout, r.stdout[-3000:]
