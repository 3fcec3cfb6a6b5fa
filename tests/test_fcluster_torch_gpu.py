"""dynamicppr_amd/torch_bridge.py, ftrack_cluster: the full-length conductance sweep of a forward track as tensors on the engine's
device (DPPR_DEST_DEVICE), against the numpy definition of tests/fcluster_ref.py after a create and after two batches, both orders;
arguments the call cannot take raise DpprError before the engine is called. The GPU test runs in ONE fresh child process (torch
first, then the engine: one HIP runtime)."""
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
from tests import fcluster_ref as fcr
from tests import forward_ref as fr
from tests import ftrack_ref as tr

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
    row, col_ = e.read_out_graph()
    for order in ("deg", "p"):
        for kw in (dict(), dict(max_len=9, min_size=2), dict(min_score=1e-4)):
            best, off, ids, score, cut_out, cut_in, vol = tb.ftrack_cluster(e, t, order, **kw)
            assert off.dtype == torch.int64 and off.device.type == "cpu" and len(off) == 6 and len(best) == 5
            for x, d in ((ids, torch.int32), (score, torch.float64), (cut_out, torch.int64), (cut_in, torch.int64), (vol, torch.int64)):
                assert isinstance(x, torch.Tensor) and x.dtype == d and x.device == dev and len(x) == int(off[-1])
            arrays = [x.cpu().numpy() for x in (ids, score, cut_out, cut_in, vol)]
            o = off.numpy()
            for i, w in enumerate(cols):
                want = fcr.cluster(w.p, row, col_, order, **kw)
                fcr.same((best[i], *[a[o[i]:o[i + 1]] for a in arrays]), want, (step, order, i))
            assert best[2]["count"] == 0   # the column of the vertex that no edge names
            assert best == t.cluster(order, **kw)
closed = e.ftrack([int(named[0])], 1e-4, 4)
closed.close()
for args in ((t, dict(order="degree")), (closed, {}), (3, {})):
    try:
        tb.ftrack_cluster(e, args[0], **args[1])
    except eng.DpprError as err:
        assert "ftrack_cluster" in str(err), err
        continue
    raise AssertionError(f"{args} was accepted")
t.close()
e.close()
print("forward cluster bridge ok")
"""


@pytest.mark.gpu
def test_ftrack_cluster_in_a_fresh_process():
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "forward cluster bridge ok" in r.stdout, r.stdout[-3000:]
