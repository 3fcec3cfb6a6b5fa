"""torch_bridge.assign against the recipe it replaces -- group_dense(...) of every group, concatenated, argmax(1) / topk(2) in torch --
in ONE fresh child process (torch first, then the engine: one HIP runtime). Where the maximum over the classes is positive and
unique the label IS torch's argmax; elsewhere the stated rule holds: the smallest class of a tied maximum, -1 where no score is
positive. The prev tensor is updated in place."""
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
W, c, directed, eps = 600, 20, 1, 1e-9
src = [int(x) for x in datagen.top_sources(V, e1, e2, W, directed, 13)]
e = eng.Engine(V, W, directed, c)
e.load_window(e1[:W], e2[:W])
g10, g3 = e.add_source_group(src[:10]), e.add_source_group(src[10:])
tg = e.add_target_group([(np.array(src[:4], dtype=np.int32), np.full(4, 0.25)), (np.array([src[5]], dtype=np.int32), np.array([1.0]))])
for g in (g10, g3, tg):
    e.group_init_solve(g, eps)
dev = torch.device("cuda", e.device)

def recipe(groups):
    return torch.cat([tb.group_dense(e, g, "p", torch.float64, "vertex_major") for g in groups], dim=1)

def check(groups, scale=None, some_clear=True):
    D = recipe(groups)
    C = D.shape[1]
    S = D if scale is None else D * torch.tensor(scale, dtype=torch.float64, device=dev)[None, :]
    out = tb.assign(e, groups, scale)
    label, best, margin = out["label"], out["best"], out["margin"]
    assert label.dtype == torch.int32 and best.dtype == torch.float64 and label.device == dev and tuple(label.shape) == (V,)
    top = torch.topk(S, min(2, C), dim=1).values
    mx = top[:, 0]
    unique = (S == mx[:, None]).sum(1) == 1
    clear = (mx > 0) & unique
    assert int(clear.sum()) > 0 or not some_clear
    assert torch.equal(label[clear].long(), S.argmax(1)[clear])
    # the tie rule: the smallest class that holds the maximum; -1 where no score is positive
    first = (S == mx[:, None]).to(torch.int32).argmax(1)
    want = torch.where(mx > 0, first, torch.full_like(first, -1)).to(torch.int32)
    assert torch.equal(label, want)
    assert torch.equal(best.view(torch.int64), torch.where(mx > 0, mx, torch.zeros_like(mx)).view(torch.int64))
    second = torch.clamp(top[:, 1], min=0.0) if C > 1 else torch.zeros_like(mx)
    assert torch.equal(margin.view(torch.int64), torch.where(mx > 0, mx - second, torch.zeros_like(mx)).view(torch.int64))
    counts = out["counts"]
    assert counts.dtype == np.int64 and counts.sum() == V and counts[C] == int((label < 0).sum())
    assert np.array_equal(counts[:C], torch.bincount(label[label >= 0].long(), minlength=C).cpu().numpy())
    assert out["n_flips"] == 0 and out["flips"] is None
    return out

a = check([g10])
check([g3, g10])
check([g10, tg, g3], scale=[1.0] * 10 + [0.25, 1.0] + [2.0, 0.0, 0.5])
t = check([g10, g10], some_clear=False)   # (every positive maximum is a tie)
assert int((t["label"] >= 10).sum()) == 0 and not bool(t["margin"][t["label"] >= 0].any())
only = tb.assign(e, [g3], want=())
assert only["best"] is None and only["margin"] is None
# prev is updated in place, and the flips are those against it
prev = a["label"].clone()
prev[::7] = 3
before = prev.clone()
out = tb.assign(e, [g10], prev=prev, want=("margin",))
assert out["label"] is prev and torch.equal(prev, a["label"]) and out["best"] is None
ids = torch.nonzero(before != a["label"]).flatten().to(torch.int32)
assert out["n_flips"] == ids.numel() > 0
fid, fold, fnew = out["flips"]
assert torch.equal(fid, ids) and torch.equal(fold, before[ids.long()]) and torch.equal(fnew, a["label"][ids.long()])
again = tb.assign(e, [g10], prev=prev)
assert again["n_flips"] == 0 and all(x.numel() == 0 for x in again["flips"])
for bad in (prev.cpu(), prev.long(), prev[:-1], prev[::2]):
    try:
        tb.assign(e, [g10], prev=bad)
    except ValueError:
        pass
    else:
        raise AssertionError("a prev that is not a contiguous int32 [V] tensor on the device must be refused")
e.close()
print("assign bridge ok")
"""


@pytest.mark.gpu
def test_assign_tensors_in_a_fresh_process():
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "assign bridge ok" in r.stdout, r.stdout[-3000:]
