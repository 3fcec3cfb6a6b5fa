"""The engine's state as torch tensors on the engine's device: the device-side exports of include/dppr.h
(dppr_group_export_sparse / dppr_group_export_dense_dev, dppr_group_subgraph, dppr_assign, dppr_group_patch) written straight into memory that torch
allocated.

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


def forward(engine, starts, iters=64, tol=0.0, dtype=torch.float64, layout="source_major", epoch=-1):
    """dppr_forward over torch tensors: f^K of the walk from each of the external ids `starts` (at most 16) as a dense tensor on
    the engine's device, [m, V] (source_major) or [V, m] (vertex_major), float64 (bit for bit) or float32 (rounded once). Returns
    (f, iters_used, rem), the last two as CPU tensors [m]."""
    if dtype not in _DTYPES or layout not in _LAYOUTS:
        raise _eng.DpprError(f"forward: dtype float64 or float32, layout in {sorted(_LAYOUTS)}")
    m = len(starts)
    if not 1 <= m <= _eng.FORWARD_MAX_M:
        raise _eng.DpprError(f"forward: 1 <= len(starts) <= {_eng.FORWARD_MAX_M}, not {m}")
    shape = (m, engine.V) if layout == "source_major" else (engine.V, m)
    out = torch.empty(shape, dtype=dtype, device=_device(engine))
    torch.cuda.synchronize(out.device)   # (the tensor is torch's; nothing of torch's is in flight on it when the engine writes)
    res = engine.forward(starts, iters, tol, epoch=epoch, dense_ptr=out.data_ptr(), dtype=_DTYPES[dtype], layout=_LAYOUTS[layout])
    return out, torch.from_numpy(res["iters_used"].copy()), torch.from_numpy(res["rem"].copy())


def forward_push(engine, sets, eps, max_rounds=64, dtype=torch.float64, layout="source_major", epoch=-1):
    """dppr_forward_push over torch tensors: p and r of the forward push from each of the start sets `sets` (at most 16; a vertex
    id or a pair (ids, weights)) as dense tensors on the engine's device, [m, V] (source_major) or [V, m] (vertex_major), float64
    (bit for bit) or float32 (rounded once). r is what group_dot takes for the bidirectional estimate. Returns (p, r, info): info
    holds rounds_used, converged, rem, pushes, left [m] and work [3] as CPU tensors."""
    if dtype not in _DTYPES or layout not in _LAYOUTS:
        raise _eng.DpprError(f"forward_push: dtype float64 or float32, layout in {sorted(_LAYOUTS)}")
    m = len(sets)
    if not 1 <= m <= _eng.FORWARD_MAX_M:
        raise _eng.DpprError(f"forward_push: 1 <= len(sets) <= {_eng.FORWARD_MAX_M}, not {m}")
    shape = (m, engine.V) if layout == "source_major" else (engine.V, m)
    p = torch.empty(shape, dtype=dtype, device=_device(engine))
    r = torch.empty(shape, dtype=dtype, device=p.device)
    torch.cuda.synchronize(p.device)   # (the tensors are torch's; nothing of torch's is in flight on them when the engine writes)
    res = engine.forward_push(sets, eps, max_rounds, epoch=epoch, dense_p_ptr=p.data_ptr(), dense_r_ptr=r.data_ptr(), dtype=_DTYPES[dtype],
                              layout=_LAYOUTS[layout])
    return p, r, {k: torch.from_numpy(v.copy()) for k, v in res.items()}


def ftrack_read(engine, track, dtype=torch.float64, layout="source_major"):
    """dppr_ftrack_read over torch tensors: p and r of the forward track `track` (Engine.ftrack) as it stands, dense tensors on the
    engine's device, [m, V] (source_major) or [V, m] (vertex_major), float64 (bit for bit) or float32 (rounded once). Returns
    (p, r, info): info holds rounds_used, converged, rem, pushes, left [m], work and fix [3] of the last create or update call as
    CPU tensors."""
    if dtype not in _DTYPES or layout not in _LAYOUTS:
        raise _eng.DpprError(f"ftrack_read: dtype float64 or float32, layout in {sorted(_LAYOUTS)}")
    if not isinstance(track, _eng.ForwardTrack) or track.handle < 0:
        raise _eng.DpprError("ftrack_read: an open ForwardTrack of Engine.ftrack")
    shape = (track.m, engine.V) if layout == "source_major" else (engine.V, track.m)
    p = torch.empty(shape, dtype=dtype, device=_device(engine))
    r = torch.empty(shape, dtype=dtype, device=p.device)
    torch.cuda.synchronize(p.device)   # (the tensors are torch's; nothing of torch's is in flight on them when the engine writes)
    res = track.read(dense_p_ptr=p.data_ptr(), dense_r_ptr=r.data_ptr(), dtype=_DTYPES[dtype], layout=_LAYOUTS[layout])
    return p, r, {k: torch.from_numpy(v.copy()) for k, v in res.items()}


def ftrack_cluster(engine, track, order="deg", min_score=0.0, max_len=0, min_size=1):
    """dppr_ftrack_cluster over torch tensors: the full-length conductance sweep of every column of the forward track `track`, one CSR
    over the columns on the engine's device, filled in place (DPPR_DEST_DEVICE). Returns (best, offsets, ids, score, cut_out, cut_in,
    vol): best a list of dicts (count, best_size, best_cut, best_vol, best_phi), offsets [m + 1] int64 on the CPU, ids int32, score
    float64, the three prefix arrays int64. The best cluster of column c is ids[offsets[c]:offsets[c] + best[c]["best_size"]]. Two
    calls: the size query, then the fill with exactly that many entries."""
    if order not in _eng.FCLUSTER_ORDERS:
        raise _eng.DpprError(f"ftrack_cluster: order in {sorted(_eng.FCLUSTER_ORDERS)}")
    if not isinstance(track, _eng.ForwardTrack) or track.handle < 0:
        raise _eng.DpprError("ftrack_cluster: an open ForwardTrack of Engine.ftrack")
    dev = _device(engine)
    kw = dict(order=order, min_score=min_score, max_len=max_len, min_size=min_size)
    best, off = track.cluster(device_ptrs={}, cap=0, **kw)
    total = int(off[-1])
    dtypes = (torch.int32, torch.float64, torch.int64, torch.int64, torch.int64)
    arrays = [torch.empty(max(total, 1), dtype=d, device=dev) for d in dtypes]
    if total:
        torch.cuda.synchronize(dev)   # (the allocations are torch's; nothing of torch's is in flight on them when the engine writes)
        names = ("ids", "score", "cut_out", "cut_in", "vol")
        best, off = track.cluster(device_ptrs={n: a.data_ptr() for n, a in zip(names, arrays)}, cap=total, **kw)
        if int(off[-1]) != total:
            raise _eng.DpprError("ftrack_cluster: the state changed between the size call and the fill")
    return (best, torch.from_numpy(off.copy()), *[a[:total] for a in arrays])


_H_LAYOUTS = {"feature_major": _eng.H_FEATURE_MAJOR, "vertex_major": _eng.H_VERTEX_MAJOR}


def group_dot(engine, gid, H, which="p", layout="feature_major"):
    """The sources of group `gid` scored under F seed distributions (dppr_group_dot_dense_dev / dppr_group_dot_sparse): a float64
    tensor [F, n] on the engine's device, written in place. H is a dense float64 / float32 tensor on the engine's device, [F, V]
    (feature_major) or [V, F] (vertex_major), or a torch.sparse_csr_tensor of shape [F, V] with int32 col_indices and float64
    values there (its crow_indices go to the host as the offsets). Anything else raises DpprError."""
    if not isinstance(H, torch.Tensor) or which not in _WHICH or layout not in _H_LAYOUTS:
        raise _eng.DpprError(f"group_dot: H a tensor, which in {sorted(_WHICH)}, layout in {sorted(_H_LAYOUTS)}")
    dev = _device(engine)
    n = len(engine.group_sources(gid))
    if H.layout == torch.sparse_csr:
        crow, col, val = H.crow_indices(), H.col_indices(), H.values()
        if H.dim() != 2 or H.shape[1] != engine.V or not 1 <= H.shape[0] <= _eng.DOT_MAX_F:
            raise _eng.DpprError(f"group_dot: a sparse H is [F, V] with 1 <= F <= {_eng.DOT_MAX_F} and V = {engine.V}, not {tuple(H.shape)}")
        if col.dtype != torch.int32 or val.dtype != torch.float64:
            raise _eng.DpprError(f"group_dot: a sparse H has int32 col_indices and float64 values, not {col.dtype} / {val.dtype}")
        if col.device != dev or val.device != dev:
            raise _eng.DpprError(f"group_dot: H must be on the engine's device {dev}, not {col.device}")
        col, val = col.contiguous(), val.contiguous()
        off = crow.to("cpu", torch.int64).numpy()
        out = torch.empty((H.shape[0], n), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)   # (H and out are torch's; nothing of torch's is in flight on them when the engine reads and writes)
        engine.group_dot_sparse_dev(gid, off, col.data_ptr(), val.data_ptr(), _WHICH[which], out_ptr=out.data_ptr())
        return out
    if H.layout != torch.strided or H.dtype not in _DTYPES:
        raise _eng.DpprError(f"group_dot: H is dense float64 / float32 or sparse CSR, not {H.layout} of {H.dtype}")
    if H.device != dev:
        raise _eng.DpprError(f"group_dot: H must be on the engine's device {dev}, not {H.device}")
    vdim = 1 if layout == "feature_major" else 0   # (the axis of the vertices)
    if H.dim() != 2 or H.shape[vdim] != engine.V:
        raise _eng.DpprError(f"group_dot: a {layout} H is {'[F, V]' if vdim else '[V, F]'} with V = {engine.V}, not {tuple(H.shape)}")
    F = H.shape[1 - vdim]
    if not 1 <= F <= _eng.DOT_MAX_F:
        raise _eng.DpprError(f"group_dot: 1 <= F <= {_eng.DOT_MAX_F}, not {F}")
    H = H.contiguous()
    out = torch.empty((F, n), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    engine.group_dot_dense_dev(gid, H.data_ptr(), F, _WHICH[which], _DTYPES[H.dtype], _H_LAYOUTS[layout], out_ptr=out.data_ptr())
    return out


def group_subgraph(engine, gid, k, min_p=0.0, epoch=-1):
    """The top-k order of every source of group `gid` and the stored edges among its vertices (dppr_group_subgraph) as tensors on the
    engine's device, filled in place: (counts [n] int32, ids [n, k] int32, p [n, k] float64, row_ptr [n, k + 1] int64, col int32).
    Row j of source i is col[row_ptr[i, j]:row_ptr[i, j + 1]]: positions in source i's order, ascending; ids are -1 and p is 0 past
    counts[i]. Two calls: the size query, then the fill with exactly that many entries."""
    if not 1 <= int(k) <= _eng.SUBGRAPH_MAX:
        raise _eng.DpprError(f"group_subgraph: 1 <= k <= {_eng.SUBGRAPH_MAX}, not {k}")
    n = len(engine.group_sources(gid))
    dev = _device(engine)
    k = int(k)
    ids = torch.empty((n, k), dtype=torch.int32, device=dev)
    p = torch.empty((n, k), dtype=torch.float64, device=dev)
    row_ptr = torch.empty((n, k + 1), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)   # (the allocations are torch's; nothing of torch's is in flight on them when the engine writes)
    cnt, off = engine.group_subgraph_dev(gid, k, min_p, 0, ids.data_ptr(), p.data_ptr(), row_ptr.data_ptr(), None, epoch)
    total = int(off[n])
    col = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    if total:
        torch.cuda.synchronize(dev)
        cnt, off = engine.group_subgraph_dev(gid, k, min_p, total, None, None, None, col.data_ptr(), epoch)
        if int(off[n]) != total:
            raise _eng.DpprError("group_subgraph: the state changed between the size call and the fill")
    return torch.from_numpy(cnt).to(dev), ids, p, row_ptr, col[:total]


_RANK_FACTORS = {None: _eng.FACTOR_NONE, "none": _eng.FACTOR_NONE, "deg": _eng.FACTOR_DEG, "inv_deg": _eng.FACTOR_INV_DEG}
_RANK_EXCLUDE = {"seeds": _eng.EXCLUDE_SEEDS, "in": _eng.EXCLUDE_IN_NEIGHBOURS, "out": _eng.EXCLUDE_OUT_NEIGHBOURS}


def _rank_vector(engine, t, what, dtypes, who="group_topk_ranked"):
    """A per-vertex tensor of a ranked query: on the engine's device, V elements, contiguous, of one of `dtypes`."""
    if not isinstance(t, torch.Tensor) or t.layout != torch.strided:
        raise ValueError(f"{who}: {what} is a dense tensor")
    if t.device != _device(engine):
        raise ValueError(f"{who}: {what} must be on the engine's device {_device(engine)}, not {t.device}")
    if t.dim() != 1 or t.numel() != engine.V:
        raise ValueError(f"{who}: {what} holds V = {engine.V} elements, not {tuple(t.shape)}")
    if t.dtype not in dtypes:
        raise ValueError(f"{who}: {what} is one of {[str(d) for d in dtypes]}, not {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{who}: {what} must be contiguous")
    return t


def _rank_spec(engine, factor, allow, deny, exclude, who):
    """The dppr_rank_spec_t of a ranked call over torch tensors, and the tensors it points into (to be kept until the engine has
    returned)."""
    flags = 0
    for name in ([exclude] if isinstance(exclude, str) else exclude):
        if name not in _RANK_EXCLUDE:
            raise ValueError(f"{who}: exclude holds any of {sorted(_RANK_EXCLUDE)}, not {name!r}")
        flags |= _RANK_EXCLUDE[name]
    kind, g_ptr, g_dtype = _eng.FACTOR_NONE, 0, _eng.F64
    keep = []   # (what the engine reads stays referenced until it has returned)
    if isinstance(factor, torch.Tensor):
        g = _rank_vector(engine, factor, "factor", (torch.float64, torch.float32), who)
        kind, g_ptr, g_dtype = _eng.FACTOR_DEV, g.data_ptr(), _DTYPES[g.dtype]
        keep.append(g)
    elif factor in _RANK_FACTORS:
        kind = _RANK_FACTORS[factor]
    else:
        raise ValueError(f"{who}: factor is None, 'deg', 'inv_deg' or a tensor, not {factor!r}")
    masks = {"allow": allow, "deny": deny}
    for what, m in masks.items():
        if m is not None:
            m = _rank_vector(engine, m, what, (torch.bool, torch.uint8), who)
            masks[what] = m.view(torch.uint8) if m.dtype == torch.bool else m
    mode, m_ptr = _eng.MASK_NONE, 0
    if masks["allow"] is not None and masks["deny"] is not None:
        both = ((masks["allow"] != 0) & (masks["deny"] == 0)).to(torch.uint8).contiguous()
        mode, m_ptr = _eng.MASK_ALLOW, both.data_ptr()
        keep.append(both)
    elif masks["allow"] is not None:
        mode, m_ptr = _eng.MASK_ALLOW, masks["allow"].data_ptr()
        keep.append(masks["allow"])
    elif masks["deny"] is not None:
        mode, m_ptr = _eng.MASK_DENY, masks["deny"].data_ptr()
        keep.append(masks["deny"])
    return _eng.Engine.rank_spec(kind, g_ptr, g_dtype, mode, m_ptr, flags), keep


def group_topk_ranked(engine, gid, k, min_score=0.0, factor=None, allow=None, deny=None, exclude=(), epoch=-1):
    """dppr_group_topk_ranked over torch tensors: a list of (ids, scores) numpy pairs, one per lane, as Engine.group_topk_ranked
    returns them. factor: None, "deg", "inv_deg" or a float64 / float32 tensor g (score = p * g[v]); allow / deny: bool or uint8
    tensors (nonzero = set; with both, a vertex takes part if it is allowed and not denied); exclude: any of "seeds", "in", "out".
    Every tensor lives on the engine's device, is contiguous and holds V elements by external id: anything else raises ValueError
    before the engine is called."""
    spec, keep = _rank_spec(engine, factor, allow, deny, exclude, "group_topk_ranked")
    torch.cuda.synchronize(_device(engine))   # (the tensors are torch's; nothing of torch's is in flight on them when the engine reads)
    return engine.group_topk_ranked(gid, k, min_score, spec, epoch)


def group_position_at(engine, gid, ids, min_score=0.0, factor=None, allow=None, deny=None, exclude=(), epoch=-1):
    """dppr_group_position_at over torch tensors: where the external ids `ids` (a host sequence or an integer tensor, at most 4096)
    stand in every lane's order under the factor, masks and exclusions of group_topk_ranked, which it takes in the same form.
    Returns (pos, counts): int32 CPU tensors [len(ids)][n] (-1: the id does not qualify in the lane) and [n]."""
    spec, keep = _rank_spec(engine, factor, allow, deny, exclude, "group_position_at")
    if isinstance(ids, torch.Tensor):
        if ids.is_floating_point() or ids.dtype == torch.bool or ids.dim() != 1:
            raise ValueError(f"group_position_at: ids is a 1-D integer tensor or a sequence, not {ids.dtype} {tuple(ids.shape)}")
        ids = ids.detach().cpu().numpy()
    torch.cuda.synchronize(_device(engine))   # (the tensors are torch's; nothing of torch's is in flight on them when the engine reads)
    pos, counts = engine.group_position_at(gid, ids, spec, min_score, epoch)
    return torch.from_numpy(pos), torch.from_numpy(counts)


def group_sample(engine, gid, S, min_score=0.0, seed=0, first=0, factor=None, allow=None, deny=None, exclude=(), with_w=True, epoch=-1):
    """dppr_group_sample over torch tensors: S external ids per lane drawn with replacement in proportion to the lane's score under
    the factor, masks and exclusions of group_topk_ranked, which it takes in the same form. Returns (ids, w, total, support,
    status): ids int32 [n, S] and w float64 [n, S] (None without with_w) on the engine's device, filled in place; total float64
    [n], support int32 [n] and status int32 [n] as CPU tensors. ids are -1 where a lane's status is not SAMPLE_OK."""
    spec, keep = _rank_spec(engine, factor, allow, deny, exclude, "group_sample")
    S = int(S)
    if not 0 <= S <= _eng.SAMPLE_MAX:
        raise _eng.DpprError(f"group_sample: 0 <= S <= {_eng.SAMPLE_MAX}, not {S}")
    n = len(engine.group_sources(gid))
    dev = _device(engine)
    ids = torch.empty((n, S), dtype=torch.int32, device=dev)
    w = torch.empty((n, S), dtype=torch.float64, device=dev) if with_w else None
    torch.cuda.synchronize(dev)   # (the tensors are torch's; nothing of torch's is in flight on them when the engine reads or writes)
    total, support, status = engine.group_sample_dev(gid, S, ids.data_ptr() if S else None, w.data_ptr() if with_w and S else None, spec,
                                                     min_score, seed, first, epoch)
    return ids, w, torch.from_numpy(total), torch.from_numpy(support), torch.from_numpy(status)


def _open_track(track, who):
    if not isinstance(track, _eng.ForwardTrack) or track.handle < 0:
        raise _eng.DpprError(f"{who}: an open ForwardTrack of Engine.ftrack")
    return track


def ftrack_topk_ranked(engine, track, k, min_score=0.0, factor=None, allow=None, deny=None, exclude=()):
    """dppr_ftrack_topk_ranked over torch tensors: a list of (ids, scores) numpy pairs, one per column of the forward track `track`,
    as ForwardTrack.topk_ranked returns them. factor, allow, deny and exclude are those of group_topk_ranked, in the same form; the
    seeds of a column are its start set, the degrees and neighbours those of the epoch the track stands on."""
    _open_track(track, "ftrack_topk_ranked")
    spec, keep = _rank_spec(engine, factor, allow, deny, exclude, "ftrack_topk_ranked")
    torch.cuda.synchronize(_device(engine))   # (the tensors are torch's; nothing of torch's is in flight on them when the engine reads)
    return track.topk_ranked(k, min_score, spec)


def ftrack_position_at(engine, track, ids, min_score=0.0, factor=None, allow=None, deny=None, exclude=()):
    """dppr_ftrack_position_at over torch tensors: where the external ids `ids` (a host sequence or an integer tensor, at most 4096)
    stand in every column's order under the factor, masks and exclusions of ftrack_topk_ranked. Returns (pos, counts): int32 CPU
    tensors [len(ids)][m] (-1: the id does not qualify in the column) and [m]."""
    _open_track(track, "ftrack_position_at")
    spec, keep = _rank_spec(engine, factor, allow, deny, exclude, "ftrack_position_at")
    if isinstance(ids, torch.Tensor):
        if ids.is_floating_point() or ids.dtype == torch.bool or ids.dim() != 1:
            raise ValueError(f"ftrack_position_at: ids is a 1-D integer tensor or a sequence, not {ids.dtype} {tuple(ids.shape)}")
        ids = ids.detach().cpu().numpy()
    torch.cuda.synchronize(_device(engine))   # (the tensors are torch's; nothing of torch's is in flight on them when the engine reads)
    pos, counts = track.position_at(ids, spec, min_score)
    return torch.from_numpy(pos.copy()), torch.from_numpy(counts.copy())


def ftrack_sample(engine, track, S, min_score=0.0, seed=0, first=0, factor=None, allow=None, deny=None, exclude=(), with_w=True):
    """dppr_ftrack_sample over torch tensors: S external ids per column drawn with replacement in proportion to the column's score
    under the factor, masks and exclusions of ftrack_topk_ranked. Returns (ids, w, total, support, status): ids int32 [m, S] and w
    float64 [m, S] (None without with_w) on the engine's device, filled in place; total float64 [m], support int32 [m] and status
    int32 [m] as CPU tensors. ids are -1 where a column's status is not SAMPLE_OK."""
    _open_track(track, "ftrack_sample")
    spec, keep = _rank_spec(engine, factor, allow, deny, exclude, "ftrack_sample")
    S = int(S)
    if not 0 <= S <= _eng.SAMPLE_MAX:
        raise _eng.DpprError(f"ftrack_sample: 0 <= S <= {_eng.SAMPLE_MAX}, not {S}")
    dev = _device(engine)
    ids = torch.empty((track.m, S), dtype=torch.int32, device=dev)
    w = torch.empty((track.m, S), dtype=torch.float64, device=dev) if with_w else None
    torch.cuda.synchronize(dev)   # (the tensors are torch's; nothing of torch's is in flight on them when the engine reads or writes)
    total, support, status = track.sample(S, spec, min_score, seed, first,
                                          device_ptrs=dict(ids=ids.data_ptr() if S else None, w=w.data_ptr() if with_w and S else None))
    return ids, w, torch.from_numpy(total.copy()), torch.from_numpy(support.copy()), torch.from_numpy(status.copy())


def assign(engine, groups, scale=None, min_score=0.0, prev=None, want=("best", "margin")):
    """dppr_assign over torch tensors on the engine's device: every external id gets the smallest class of largest score =
    scale[c] * p_c above min_score, or -1; the classes are the lanes of `groups` (handles of this engine) in call order. Returns a
    dict: label [V] int32, best / margin [V] float64 (those named in `want`, else None), counts [C + 1] int64 on the host (the last:
    unassigned), n_flips, and flips = (id, old, new) int32 tensors against `prev`, ascending by id (None without prev).
    prev: an int32 tensor of V labels on the engine's device, contiguous; it is UPDATED IN PLACE and returned as label. scale: a
    host sequence of C finite values >= 0, or None. Anything else raises ValueError before the engine is called."""
    dev = _device(engine)
    unknown = set(want) - {"best", "margin"}
    if unknown:
        raise ValueError(f"assign: want holds any of 'best', 'margin', not {sorted(unknown)}")
    V = engine.V
    if prev is not None:
        if not isinstance(prev, torch.Tensor) or prev.layout != torch.strided or prev.dtype != torch.int32:
            raise ValueError("assign: prev is a dense int32 tensor")
        if prev.device != dev:
            raise ValueError(f"assign: prev must be on the engine's device {dev}, not {prev.device}")
        if prev.dim() != 1 or prev.numel() != V or not prev.is_contiguous():
            raise ValueError(f"assign: prev holds V = {V} labels, contiguous, not {tuple(prev.shape)}")
    label = prev if prev is not None else torch.empty(V, dtype=torch.int32, device=dev)
    best = torch.empty(V, dtype=torch.float64, device=dev) if "best" in want else None
    margin = torch.empty(V, dtype=torch.float64, device=dev) if "margin" in want else None
    lists = tuple(torch.empty(V, dtype=torch.int32, device=dev) for _ in range(3)) if prev is not None else (None, None, None)
    torch.cuda.synchronize(dev)   # (the tensors are torch's; nothing of torch's is in flight on them when the engine reads and writes)
    counts, n_flips = engine.assign_dev(groups, label.data_ptr(), scale, min_score, best.data_ptr() if best is not None else None,
                                        margin.data_ptr() if margin is not None else None, label.data_ptr() if prev is not None else None,
                                        V if prev is not None else 0, tuple(t.data_ptr() if t is not None else None for t in lists))
    flips = tuple(t[:n_flips] for t in lists) if prev is not None else None
    return {"label": label, "best": best, "margin": margin, "counts": counts, "n_flips": n_flips, "flips": flips}


def group_patch(engine, gid, min_p, min_delta=0.0, remark=_eng.PATCH_REMARK_EMITTED):
    """dppr_group_patch with tensors on the engine's device, written in place: a dict of up_offsets / del_offsets (int64 CPU
    tensors [n + 1]), up_ids (int32), up_p (float64) and del_ids (int32). Two calls: the size query, which leaves the mark alone,
    then the fill with exactly those caps, which applies `remark`."""
    n = len(engine.group_sources(gid))
    dev = _device(engine)
    uo, do, _ = engine.group_patch_dev(gid, min_p, min_delta, 0, 0, None, None, None, _eng.PATCH_KEEP_MARK)
    ups, dels = int(uo[n]), int(do[n])
    up_ids = torch.empty(max(ups, 1), dtype=torch.int32, device=dev)
    up_p = torch.empty(max(ups, 1), dtype=torch.float64, device=dev)
    del_ids = torch.empty(max(dels, 1), dtype=torch.int32, device=dev)
    if ups or dels or int(remark) != _eng.PATCH_KEEP_MARK:
        torch.cuda.synchronize(dev)   # (the allocations are torch's; nothing of torch's is in flight on them when the engine writes)
        uo, do, written = engine.group_patch_dev(gid, min_p, min_delta, ups, dels, up_ids.data_ptr() if ups else None,
                                                 up_p.data_ptr() if ups else None, del_ids.data_ptr() if dels else None, remark)
        if written != 1 or int(uo[n]) != ups or int(do[n]) != dels:
            raise _eng.DpprError("group_patch: the state changed between the size call and the fill")
    return {"up_offsets": torch.from_numpy(uo), "up_ids": up_ids[:ups], "up_p": up_p[:ups], "del_offsets": torch.from_numpy(do),
            "del_ids": del_ids[:dels]}


def _lanes(offsets, dev):
    """The lane of every entry of a CSR over the lanes, from its host offsets."""
    counts = (offsets[1:] - offsets[:-1]).to(dev)
    return torch.repeat_interleave(torch.arange(len(counts), dtype=torch.int64, device=dev), counts)


def apply_patch(replica, patch, V):
    """Merge a patch of group_patch into a replica held as tensors -- (offsets int64 CPU [n + 1], ids int32, p float64), the
    form of group_export_sparse with ids and p on one device -- from torch ops alone: every entry gets the key lane * V + id, the
    replica's entries whose key is deleted or upserted leave, the upserts enter, one sort puts the keys back in order. Returns a
    new (offsets, ids, p)."""
    off, ids, p = replica
    dev = ids.device
    n = len(off) - 1
    key = _lanes(off, dev) * V + ids.to(torch.int64)
    up_key = _lanes(patch["up_offsets"], dev) * V + patch["up_ids"].to(torch.int64)
    del_key = _lanes(patch["del_offsets"], dev) * V + patch["del_ids"].to(torch.int64)
    keep = ~torch.isin(key, torch.cat([up_key, del_key]))
    all_key, all_p = torch.cat([key[keep], up_key]), torch.cat([p[keep], patch["up_p"]])
    all_key, order = torch.sort(all_key)   # (the keys are distinct: the order is total)
    lane = torch.div(all_key, V, rounding_mode="floor")
    counts = torch.bincount(lane, minlength=n).cpu()
    new_off = torch.zeros(n + 1, dtype=torch.int64)
    new_off[1:] = torch.cumsum(counts, 0)
    return new_off, (all_key - lane * V).to(torch.int32), all_p[order]
