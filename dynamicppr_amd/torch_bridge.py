"""The engine's state as torch tensors on the engine's device: the device-side exports of include/dppr.h
(dppr_group_export_sparse / dppr_group_export_dense_dev) written straight into memory that torch allocated.

The engine binding itself (``engine.py``) stays torch-free: nothing there imports torch, and importing this module puts no
torch into it.

Loading rule (the one ``bench.py`` lives by). torch bundles a HIP runtime of its own, and that runtime and the one
libdppr_hip.so links to share one SONAME: whichever is loaded first serves the whole process. A pointer is only meaningful to
the runtime that allocated it, so torch must be imported BEFORE the library is loaded -- import torch (or this module) first,
then create the engine. If the library is already loaded when this module is imported and the HIP runtime mapped into the
process is not torch's, the import raises instead of passing pointers between two runtimes.
"""
from __future__ import annotations

import os

from . import engine as _eng

_lib_was_loaded = _eng._lib is not None

import torch  # noqa: E402  (after the look at the library: the check below is about the order of the two loads)


def _mapped_hip_runtimes():
    """Paths of every libamdhip64 mapped into this process."""
    paths = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                path = line.rsplit(" ", 1)[-1].strip()
                if "libamdhip64" in os.path.basename(path):
                    paths.add(os.path.realpath(path))
    except OSError:
        pass
    return paths


def _check_one_runtime():
    torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    names = os.listdir(torch_lib) if os.path.isdir(torch_lib) else []
    bundled = {os.path.realpath(os.path.join(torch_lib, n)) for n in names if n.startswith("libamdhip64")}
    foreign = sorted(_mapped_hip_runtimes() - bundled)
    if _lib_was_loaded and bundled and foreign:
        raise ImportError("dynamicppr_amd.torch_bridge: libdppr_hip.so was loaded before torch, and the HIP runtime mapped into "
                          f"this process ({', '.join(foreign)}) is not torch's: import torch (or this module) before the first "
                          "engine call, so that both use one runtime")


_check_one_runtime()

_DTYPES = {torch.float64: _eng.F64, torch.float32: _eng.F32}
_LAYOUTS = {"vertex_major": _eng.VERTEX_MAJOR, "source_major": _eng.SOURCE_MAJOR}
_WHICH = {"p": _eng.DENSE_P, "r": _eng.DENSE_R}


def _device(engine):
    return torch.device("cuda", engine.device)


def group_sparse_csr(engine, gid, min_p, with_r=False):
    """The sparse vectors of every source of group `gid` (p > min_p) as a torch.sparse_csr_tensor of shape [n, V] on the engine's
    device: int32 col_indices (external ids ascending), float64 values, crow_indices uploaded from the host offsets. with_r: a pair
    (p tensor, r tensor) over the same indices."""
    n = len(engine.group_sources(gid))
    dev = _device(engine)
    total = int(engine.group_support(gid, min_p).sum())
    ids = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    p = torch.empty(max(total, 1), dtype=torch.float64, device=dev)
    r = torch.empty(max(total, 1), dtype=torch.float64, device=dev) if with_r else None
    torch.cuda.synchronize(dev)   # (the allocations are torch's; nothing of torch's is in flight on them when the engine writes)
    off = engine.group_export_sparse_dev(gid, min_p, total, ids.data_ptr(), p.data_ptr(), r.data_ptr() if with_r else None)
    if int(off[n]) != total:
        raise _eng.DpprError("group_sparse_csr: the state changed between the size call and the fill")
    if total >= 2 ** 31:
        raise _eng.DpprError("group_sparse_csr: more than 2^31 - 1 entries do not fit int32 indices")
    crow = torch.from_numpy(off.astype("int32")).to(dev)   # (one index dtype for crow_indices and col_indices)

    def csr(values):
        return torch.sparse_csr_tensor(crow, ids[:total], values[:total], size=(n, engine.V))

    return (csr(p), csr(r)) if with_r else csr(p)


def group_dense(engine, gid, which="p", dtype=torch.float64, layout="source_major"):
    """p (or r) of every source of group `gid` by external id as a dense tensor on the engine's device: [n, V] (source_major) or
    [V, n] (vertex_major), float64 or float32 (round to nearest even)."""
    if dtype not in _DTYPES or layout not in _LAYOUTS or which not in _WHICH:
        raise _eng.DpprError(f"group_dense: which in {sorted(_WHICH)}, dtype float64 or float32, layout in {sorted(_LAYOUTS)}")
    n = len(engine.group_sources(gid))
    shape = (n, engine.V) if layout == "source_major" else (engine.V, n)
    out = torch.empty(shape, dtype=dtype, device=_device(engine))
    torch.cuda.synchronize(out.device)
    engine.group_export_dense_dev(gid, out.data_ptr(), _WHICH[which], _DTYPES[dtype], _LAYOUTS[layout])
    return out
