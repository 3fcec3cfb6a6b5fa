"""dynamicppr_amd/torch_bridge.py, group_dot: the sources of a group scored under seed distributions held in torch tensors, against
the fold of tests/dot_ref.py over group_dense copied to the host, bit for bit. The GPU test runs in ONE fresh child process (torch
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
from tests import dot_ref

V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
W, c, directed, eps, n = 600, 20, 1, 1e-9, 10
sources = [int(x) for x in datagen.top_sources(V, e1, e2, W, directed, n)]
e = eng.Engine(V, W, directed, c)
e.load_window(e1[:W], e2[:W])
gid = e.add_source_group(sources)
e.group_init_solve(gid, eps)
dev = torch.device("cuda", e.device)
bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
rng = np.random.default_rng(31)
F = 17
h = rng.standard_normal((F, V))


def check(out, want, what):
    assert isinstance(out, torch.Tensor) and out.dtype == torch.float64 and tuple(out.shape) == (F, n) and out.device == dev, what
    assert np.array_equal(bits(out.cpu().numpy()), bits(want)), what


for which in ("p", "r"):
    cols = list(tb.group_dense(e, gid, which, torch.float64, "source_major").cpu().numpy())
    for dtype, np_t in ((torch.float64, np.float64), (torch.float32, np.float32)):
        ht = h.astype(np_t)
        want = dot_ref.dense(ht.astype(np.float64), cols)
        H = torch.from_numpy(ht).to(dev)
        check(tb.group_dot(e, gid, H, which), want, (which, dtype, "feature_major"))
        check(tb.group_dot(e, gid, H.T.contiguous(), which, "vertex_major"), want, (which, dtype, "vertex_major"))
        check(tb.group_dot(e, gid, H.T.contiguous().T, which), want, (which, dtype, "a view that is not contiguous"))
    ids = [np.nonzero(np.abs(row) > 0.9)[0] for row in h]
    off = np.concatenate([[0], np.cumsum([len(i) for i in ids])])
    col, val = np.concatenate(ids), np.concatenate([row[i] for row, i in zip(h, ids)])
    S = torch.sparse_csr_tensor(torch.from_numpy(off.astype(np.int32)), torch.from_numpy(col.astype(np.int32)), torch.from_numpy(val),
                                size=(F, V)).to(dev)
    assert S.col_indices().dtype == torch.int32 and S.values().dtype == torch.float64
    check(tb.group_dot(e, gid, S, which), dot_ref.sparse(off, col, val, cols), (which, "sparse"))

H = torch.from_numpy(h).to(dev)
S64 = torch.sparse_csr_tensor(torch.from_numpy(off.astype(np.int64)), torch.from_numpy(col.astype(np.int64)), torch.from_numpy(val), size=(F, V)).to(dev)
S32 = torch.sparse_csr_tensor(torch.from_numpy(off.astype(np.int32)), torch.from_numpy(col.astype(np.int32)), torch.from_numpy(val.astype(np.float32)),
                              size=(F, V)).to(dev)
Swide = torch.sparse_csr_tensor(torch.from_numpy(off.astype(np.int32)), torch.from_numpy(col.astype(np.int32)), torch.from_numpy(val), size=(F, V + 1)).to(dev)
bad = [(H.to(torch.float16), "p", "feature_major"), (H.to(torch.int64), "p", "feature_major"),   # a wrong dtype
       (H.cpu(), "p", "feature_major"), (S.cpu(), "p", "feature_major"),                           # a wrong device
       (H, "p", "vertex_major"), (H[:, :-1], "p", "feature_major"), (H[0], "p", "feature_major"), (H.T.contiguous(), "p", "feature_major"),  # a wrong shape
       (H[:0], "p", "feature_major"), (S64, "p", "feature_major"), (S32, "p", "feature_major"), (Swide, "p", "feature_major"),
       (H, "q", "feature_major"), (H, "p", "source_major"), (h, "p", "feature_major")]
for k, (t, which, layout) in enumerate(bad):
    try:
        tb.group_dot(e, gid, t, which, layout)
    except eng.DpprError:
        continue
    raise AssertionError(f"bad call {k} was accepted")
check(tb.group_dot(e, gid, H), dot_ref.dense(h, list(tb.group_dense(e, gid).cpu().numpy())), "a valid call after the rejections")
e.close()
print("dot bridge ok")
"""


@pytest.mark.gpu
def test_group_dot_in_a_fresh_process():
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "dot bridge ok" in r.stdout, r.stdout[-3000:]
