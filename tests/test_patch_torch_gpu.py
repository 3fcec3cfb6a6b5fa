"""dynamicppr_amd/torch_bridge.py: the patch feed with a replica held as torch tensors on the engine's device -- group_patch
writes the patch in place, apply_patch merges it from torch ops. The chain of tests/test_patch_gpu.py (mark, export, six batches
with the emitted-only re-mark) runs in ONE fresh child process (torch first, then the engine: one HIP runtime)."""
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
from oracle import oracle as orc
from tests import patch_ref as ref

V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
W, c, directed, eps, n = 600, 20, 0, 1e-9, 10
sources = [int(x) for x in datagen.top_sources(V, e1, e2, W, directed, n)]
g = orc.Graph(V, e1, e2, directed, W, c)
e = eng.Engine(V, W, directed, c)
e.load_window(*g.window_edges())
gid = e.add_source_group(sources)
e.group_init_solve(gid, eps)
dev = torch.device("cuda", e.device)
dense = lambda: [e.group_read(gid, i)[0] for i in range(n)]
pos = np.concatenate([p[p > 0] for p in dense()])
tau = float(np.quantile(pos, 0.5))
for delta in (0.0, 1e-7):
    e.group_mark(gid)                       # the initial sync: the mark, then the export
    mark = dense()
    off, ids, p = e.group_export_sparse(gid, tau)
    replica = (torch.from_numpy(off), torch.from_numpy(ids).to(dev), torch.from_numpy(p).to(dev))
    sent = 0
    for batch in range(6):
        assert not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        e.slide(*g.new_stream())
        e.group_update(gid, eps)
        now = dense()
        pt = tb.group_patch(e, gid, tau, delta)   # (the emitted-only re-mark is the default of the bridge)
        assert pt["up_ids"].device == dev and pt["up_p"].device == dev and pt["del_ids"].device == dev
        assert pt["up_ids"].dtype == torch.int32 and pt["up_p"].dtype == torch.float64 and pt["up_offsets"].dtype == torch.int64
        got = {k: v.cpu().numpy() for k, v in pt.items()}
        assert ref.same_patch(got, ref.patch(now, mark, tau, delta)), (delta, batch)
        mark = ref.remark(now, mark, tau, delta, ref.REMARK_EMITTED)
        sent += len(got["up_ids"]) + len(got["del_ids"])
        replica = tb.apply_patch(replica, pt, V)
        assert replica[1].device == dev and replica[2].device == dev and replica[1].dtype == torch.int32
        mine = (replica[0].numpy(), replica[1].cpu().numpy(), replica[2].cpu().numpy())
        want = e.group_export_sparse(gid, tau)
        assert np.array_equal(mine[0], want[0]) and np.array_equal(mine[1], want[1]), (delta, batch)
        if delta == 0.0:
            assert np.array_equal(ref.bits(mine[2]), ref.bits(want[2])), batch
        else:
            assert np.all(np.abs(mine[2] - want[2]) <= delta), batch
    assert sent > 0
e.close()
print("patch bridge ok")
"""


@pytest.mark.gpu
def test_the_replica_as_tensors_in_a_fresh_process():
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "patch bridge ok" in r.stdout, r.stdout[-3000:]
