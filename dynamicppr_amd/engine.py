"""ctypes binding of libdppr_hip.so (the C ABI of include/dppr.h).

This is plumbing for tests and bench.py; the product's host side is the C++
program under dynamicppr_amd/host/ (``./pagerank``), which calls the same C ABI.
There is no CPU fallback: if the HIP library is missing or no device is present
every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DPPR_LIB") or os.path.join(_HERE, "libdppr_hip.so")  # DPPR_LIB: diagnostic builds only

SCHEDULE_EAGER = 0
SCHEDULE_SYNC = 1


class DpprError(RuntimeError):
    pass


class Stats(C.Structure):
    _fields_ = [("iterations", C.c_int64), ("sum_F", C.c_int64), ("sum_E", C.c_int64), ("sum_N", C.c_int64),
                ("records", C.c_int64), ("inspected", C.c_int64), ("batches", C.c_int64),
                ("pull_iterations", C.c_int64),
                ("algorithmic_bytes", C.c_int64), ("gpu_ms", C.c_double), ("push_ms", C.c_double),
                ("push_launches", C.c_int64), ("persist_launches", C.c_int64), ("persist_aborts", C.c_int64),
                ("binned_sweeps", C.c_int64), ("sweep_F", C.c_int64), ("sweep_E", C.c_int64), ("sweep_ms", C.c_double),
                ("sweep_launches", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def build(force: bool = False) -> str:
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".hpp"))]
    srcs.append(os.path.join(os.path.dirname(_HERE), "include", "dppr.h"))
    stale = (not os.path.exists(LIB_PATH)) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", csrc, "-s", "all"])
    return LIB_PATH


_lib = None
EXPORTS = [
    "dppr_abi_version", "dppr_strerror", "dppr_last_error", "dppr_create", "dppr_destroy", "dppr_set_schedule", "dppr_set_profiling", "dppr_set_tuning", "dppr_set_persistent", "dppr_set_incremental_graph",
    "dppr_load_window", "dppr_set_batch", "dppr_slide", "dppr_add_source", "dppr_init_solve", "dppr_update",
    "dppr_incremental_batch_update", "dppr_execute_main_loop", "dppr_read", "dppr_write", "dppr_stats",
    "dppr_reset_stats", "dppr_inspect", "dppr_read_graph", "dppr_graph_edges", "dppr_read_out_graph", "dppr_trace_enable",
    "dppr_trace_get", "dppr_synchronize", "dppr_bench_atomics",
    "dppr_add_source_group", "dppr_group_init_solve", "dppr_group_update", "dppr_group_read", "dppr_group_stats",
    "dppr_group_reset_stats", "dppr_set_group_seeding", "dppr_seed_lists", "dppr_set_sweep_bitmap", "dppr_set_group_resident", "dppr_set_resident_slots", "dppr_set_resident_update",
    "dppr_set_renumbering", "dppr_id_space", "dppr_set_group_push", "dppr_set_binned_sweep", "dppr_device_count", "dppr_set_phase_merge", "dppr_init_solve_at", "dppr_group_init_solve_at", "dppr_set_variant", "dppr_set_batch_grouping",
    "dppr_time_batch_grouping", "dppr_debug_dump", "dppr_hint_next_batch",
    "dppr_bench_line_fills", "dppr_bench_stream_copy", "dppr_build_id", "dppr_heartbeat", "dppr_slide_concurrent", "dppr_renumbering_due", "dppr_debug_bin_tables",
    "dppr_debug_grouping", "dppr_topk", "dppr_group_topk", "dppr_read_at", "dppr_group_read_at", "dppr_debug_live_bytes",
    "dppr_group_sources", "dppr_group_replace_source", "dppr_group_add_source", "dppr_group_remove_source",
    "dppr_group_topk_weighted", "dppr_group_score_at", "dppr_debug_query_ms",
    "dppr_mark", "dppr_group_mark", "dppr_unmark", "dppr_group_unmark", "dppr_changes", "dppr_group_changes",
    "dppr_support", "dppr_group_support", "dppr_export_sparse", "dppr_group_export_sparse", "dppr_export_dense_dev",
    "dppr_group_export_dense_dev",
    "dppr_patch", "dppr_group_patch",
    "dppr_dot_dense_dev", "dppr_group_dot_dense_dev", "dppr_dot_sparse", "dppr_group_dot_sparse",
    "dppr_walks", "dppr_refine_at", "dppr_group_refine_at", "dppr_debug_id_map", "dppr_debug_walk_form",
    "dppr_cluster", "dppr_group_cluster",
    "dppr_subgraph", "dppr_group_subgraph", "dppr_debug_subgraph_wave_max",
    "dppr_add_target_group", "dppr_group_replace_target", "dppr_group_targets",
    "dppr_topk_ranked", "dppr_group_topk_ranked", "dppr_rank_score_at", "dppr_group_rank_score_at", "dppr_debug_rank_piece",
    "dppr_assign", "dppr_assign_at",
    "dppr_position_at", "dppr_group_position_at", "dppr_debug_position_tile",
    "dppr_explain_at", "dppr_group_explain_at", "dppr_debug_explain",
    "dppr_certify", "dppr_group_certify", "dppr_debug_certify",
    "dppr_sample", "dppr_group_sample", "dppr_debug_sample_form",
    "dppr_forward", "dppr_debug_forward",
    "dppr_forward_push", "dppr_debug_forward_push",
    "dppr_ftrack_create", "dppr_ftrack_update", "dppr_ftrack_read", "dppr_ftrack_info", "dppr_ftrack_destroy", "dppr_debug_ftrack_ms",
    "dppr_ftrack_cluster", "dppr_debug_ftrack_cluster",
    "dppr_ftrack_topk_ranked", "dppr_ftrack_rank_score_at", "dppr_ftrack_position_at", "dppr_ftrack_sample", "dppr_debug_ftrack_rank",
]

DEST_HOST, DEST_DEVICE = 0, 1
DENSE_P, DENSE_R = 0, 1
F64, F32 = 0, 1
VERTEX_MAJOR, SOURCE_MAJOR = 0, 1
DOT_MAX_F = 4096
H_FEATURE_MAJOR, H_VERTEX_MAJOR = 0, 1
WALK_MAX_M, WALK_MAX_W, WALK_MAX_TOTAL = 4096, 1 << 20, 1 << 26
WALK_REFILL, WALK_PER_THREAD = 0, 1
CLUSTER_MAX = 8192
SUBGRAPH_MAX = 8192
TARGET_SET_MAX = 65536
FACTOR_NONE, FACTOR_DEV, FACTOR_DEG, FACTOR_INV_DEG = 0, 1, 2, 3
MASK_NONE, MASK_ALLOW, MASK_DENY = 0, 1, 2
EXCLUDE_SEEDS, EXCLUDE_IN_NEIGHBOURS, EXCLUDE_OUT_NEIGHBOURS = 1, 2, 4
RANK_PIECE = 512
ASSIGN_GROUPS_MAX, ASSIGN_CLASSES_MAX = 16, 256
POSITION_MAX = 4096
EXPLAIN_MAX_M, EXPLAIN_MAX_F, EXPLAIN_MAX_DEPTH = 4096, 16, 64
END_SEED, END_DEPTH, END_DEAD, END_CYCLE = 0, 1, 2, 3
CERT_RESIDUAL, CERT_INVARIANT = 1, 2
PATCH_KEEP_MARK, PATCH_REMARK_ALL, PATCH_REMARK_EMITTED = 0, 1, 2
SAMPLE_MAX, SAMPLE_MAX_TOTAL = 1 << 20, 1 << 24
SAMPLE_OK, SAMPLE_EMPTY, SAMPLE_NONFINITE = 0, 1, 2
SAMPLE_WAVE, SAMPLE_PER_THREAD = 0, 1
FORWARD_MAX_M, FORWARD_MAX_ITERS, FORWARD_CHECK, FORWARD_AT_MAX = 16, 256, 8, 4096
FPUSH_SET_MAX, FPUSH_MAX_ROUNDS = 4096, 256
FTRACK_MAX = 16


class RankSpec(C.Structure):
    """dppr_rank_spec_t: the factor, the mask and the exclusions of a ranked query."""
    _fields_ = [("factor", C.c_int32), ("factor_dtype", C.c_int32), ("factor_dev", C.c_void_p), ("mask", C.c_int32),
                ("mask_dev", C.c_void_p), ("exclude", C.c_uint32)]


class ExplainOut(C.Structure):
    """dppr_explain_out_t: where the outputs of an explain call go (host memory; a NULL is not computed)."""
    _ip, _dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    _fields_ = [("deg", _ip), ("distinct", _ip), ("self", _dp), ("nbr_count", _ip), ("nbr", _ip), ("nbr_mult", _ip), ("nbr_c", _dp),
                ("len", _ip), ("end", _ip), ("path", _ip), ("path_p", _dp), ("path_c", _dp)]


class CertifyOut(C.Structure):
    """dppr_certify_out_t: where the outputs of a certify call go (host memory, [n]; a NULL is not computed), and what the last
    solve left, written by the call."""
    _ip, _dp, _lp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
    _fields_ = [("max_abs_r", _dp), ("argmax_r", _ip), ("sum_abs_r", _dp), ("sum_p", _dp), ("n_pos", _lp), ("n_neg", _lp),
                ("n_nonfinite", _lp), ("n_p_nonzero", _lp), ("inv_max_err", _dp), ("inv_argmax", _ip),
                ("state_epoch", C.c_int32), ("converged", C.c_int32), ("conv_eps", C.c_double)]


class ForwardOut(C.Structure):
    """dppr_forward_out_t: where the parts of a forward call go (a part whose pointers are all NULL is not run)."""
    _ip, _dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    _fields_ = [("iters_used", _ip), ("rem", _dp), ("k", C.c_int32), ("min_f", C.c_double), ("topk_ids", _ip), ("topk_f", _dp),
                ("topk_counts", _ip), ("at_ids", _ip), ("n_at", C.c_int32), ("at_f", _dp), ("dense_dev", C.c_void_p),
                ("dense_dtype", C.c_int32), ("dense_layout", C.c_int32)]


class ForwardPushOut(C.Structure):
    """dppr_forward_push_out_t: where the parts of a forward push go (a part whose pointers are all NULL is not run)."""
    _ip, _dp, _lp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
    _fields_ = [("rounds_used", _ip), ("converged", _ip), ("rem", _dp), ("pushes", _lp), ("left", _lp), ("work", _lp),
                ("k", C.c_int32), ("min_p", C.c_double), ("topk_ids", _ip), ("topk_p", _dp), ("topk_counts", _ip),
                ("at_ids", _ip), ("n_at", C.c_int32), ("at_p", _dp), ("at_r", _dp), ("dense_p_dev", C.c_void_p),
                ("dense_r_dev", C.c_void_p), ("dense_dtype", C.c_int32), ("dense_layout", C.c_int32)]


class FtrackOut(C.Structure):
    """dppr_ftrack_out_t: dppr_forward_push_out_t with fix [3] behind it."""
    _fields_ = ForwardPushOut._fields_ + [("fix", C.POINTER(C.c_int64))]


class PatchOut(C.Structure):
    """dppr_patch_out_t: where the two CSRs of a patch go (the offsets in host memory, the arrays where `dest` says), and whether
    the call wrote them."""
    _fields_ = [("up_offsets", C.POINTER(C.c_int64)), ("up_ids", C.c_void_p), ("up_p", C.c_void_p),
                ("del_offsets", C.POINTER(C.c_int64)), ("del_ids", C.c_void_p), ("written", C.c_int32)]


def apply_patch(replica, patch):
    """Merge a patch (the dict Engine.patch / Engine.group_patch returns) into a replica held in the (offsets, ids, p) form of
    group_export_sparse: per lane the deletes leave, the upserts overwrite or enter, the ids stay ascending. Pure numpy; returns a
    new (offsets, ids, p)."""
    off, ids, p = (np.asarray(a) for a in replica[:3])
    n = len(off) - 1
    uo, do = patch["up_offsets"], patch["del_offsets"]
    if len(uo) != n + 1 or len(do) != n + 1:
        raise ValueError(f"apply_patch: the replica has {n} lanes, the patch {len(uo) - 1}")
    out_ids, out_p, out_off = [], [], np.zeros(n + 1, dtype=np.int64)
    for i in range(n):
        li, lp = ids[off[i]:off[i + 1]], p[off[i]:off[i + 1]]
        ui, up = patch["up_ids"][uo[i]:uo[i + 1]], patch["up_p"][uo[i]:uo[i + 1]]
        di = patch["del_ids"][do[i]:do[i + 1]]
        keep = ~np.isin(li, di) & ~np.isin(li, ui)
        mi, mp = np.concatenate([li[keep], ui]), np.concatenate([lp[keep], up])
        order = np.argsort(mi, kind="stable")
        out_ids.append(mi[order])
        out_p.append(mp[order])
        out_off[i + 1] = out_off[i] + len(mi)
    return out_off, np.concatenate(out_ids).astype(np.int32), np.concatenate(out_p).astype(np.float64)


class Cluster(C.Structure):
    """dppr_cluster_t: the best prefix of one source's order."""
    _fields_ = [("count", C.c_int32), ("best_size", C.c_int32), ("best_cut", C.c_int64), ("best_vol", C.c_int64),
                ("best_phi", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def lib():
    """Load the HIP library; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DpprError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(the HIP extension is mandatory, there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    vp, ip, dp, u8p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    i64p, fp = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    L.dppr_abi_version.restype = C.c_int
    L.dppr_strerror.argtypes = [C.c_int]
    L.dppr_strerror.restype = C.c_char_p
    L.dppr_last_error.argtypes = [vp]
    L.dppr_last_error.restype = C.c_char_p
    L.dppr_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int32, C.c_int32, C.c_int, C.c_int32, C.c_int32]
    L.dppr_destroy.argtypes = [vp]
    L.dppr_destroy.restype = None
    L.dppr_set_schedule.argtypes = [vp, C.c_int]
    L.dppr_set_profiling.argtypes = [vp, C.c_int]
    L.dppr_set_incremental_graph.argtypes = [vp, C.c_int]
    L.dppr_set_renumbering.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.dppr_set_group_push.argtypes = [vp, C.c_int, C.c_int, C.c_int64]
    L.dppr_id_space.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.dppr_set_tuning.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.dppr_set_persistent.argtypes = [vp, C.c_int, C.c_int64]
    L.dppr_load_window.argtypes = [vp, ip, ip, C.c_int32]
    L.dppr_set_batch.argtypes = [vp, ip, ip, u8p, C.c_int32]
    L.dppr_slide.argtypes = [vp, ip, ip, C.c_int32, ip]
    L.dppr_add_source.argtypes = [vp, C.c_int32, ip]
    L.dppr_init_solve.argtypes = [vp, C.c_int32, C.c_double, fp]
    L.dppr_init_solve_at.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, fp]
    L.dppr_group_init_solve_at.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, fp]
    L.dppr_update.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, fp]
    L.dppr_incremental_batch_update.argtypes = [vp, C.c_int32, C.c_int32]
    L.dppr_execute_main_loop.argtypes = [vp, C.c_int32, C.c_int32, C.c_int, C.c_double]
    L.dppr_read.argtypes = [vp, C.c_int32, dp, dp]
    L.dppr_write.argtypes = [vp, C.c_int32, dp, dp]
    L.dppr_stats.argtypes = [vp, C.c_int32, C.POINTER(Stats)]
    L.dppr_reset_stats.argtypes = [vp, C.c_int32]
    L.dppr_inspect.argtypes = [vp, C.c_int32, C.c_int, C.c_double, ip, ip]
    L.dppr_read_graph.argtypes = [vp, C.c_int32, ip, ip, ip]
    L.dppr_graph_edges.argtypes = [vp, C.c_int32, ip]
    L.dppr_read_out_graph.argtypes = [vp, C.c_int32, ip, ip]
    L.dppr_trace_enable.argtypes = [vp, C.c_int32, C.c_int]
    L.dppr_trace_get.argtypes = [vp, C.c_int32, i64p, i64p, i64p, ip]
    L.dppr_synchronize.argtypes = [vp]
    L.dppr_add_source_group.argtypes = [vp, ip, C.c_int32, ip]
    L.dppr_group_init_solve.argtypes = [vp, C.c_int32, C.c_double, fp]
    L.dppr_group_update.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, fp]
    L.dppr_group_read.argtypes = [vp, C.c_int32, C.c_int32, dp, dp]
    L.dppr_group_stats.argtypes = [vp, C.c_int32, C.POINTER(Stats)]
    L.dppr_set_sweep_bitmap.argtypes = [vp, C.c_int]
    L.dppr_set_phase_merge.argtypes = [vp, C.c_int, C.c_int]
    L.dppr_set_variant.argtypes = [vp, C.c_int]
    L.dppr_set_batch_grouping.argtypes = [vp, C.c_int]
    L.dppr_set_binned_sweep.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64]
    L.dppr_set_group_resident.argtypes = [vp, C.c_int]
    L.dppr_set_resident_slots.argtypes = [vp, C.c_int]
    L.dppr_set_resident_update.argtypes = [vp, C.c_int]
    L.dppr_seed_lists.argtypes = [vp, C.c_int32, C.c_int, ip, ip]
    L.dppr_group_reset_stats.argtypes = [vp, C.c_int32]
    L.dppr_set_group_seeding.argtypes = [vp, C.c_int]
    L.dppr_bench_atomics.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, fp]
    L.dppr_time_batch_grouping.argtypes = [vp, C.c_int32, C.c_int32, fp]
    L.dppr_debug_dump.argtypes = [vp, C.c_char_p, C.c_int32]
    L.dppr_hint_next_batch.argtypes = [vp, ip, ip, C.c_int32, ip, ip, C.c_int32]
    L.dppr_bench_line_fills.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int, fp]
    L.dppr_bench_stream_copy.argtypes = [C.c_int, C.c_int64, C.c_int, fp]
    L.dppr_build_id.restype = C.c_char_p
    L.dppr_heartbeat.argtypes = [vp]
    L.dppr_slide_concurrent.argtypes = [vp, ip, ip, C.c_int32, ip]
    L.dppr_renumbering_due.argtypes = [vp]
    u16p = C.POINTER(C.c_uint16)
    L.dppr_debug_bin_tables.argtypes = [vp, C.c_int32, ip, ip, ip, ip, ip, ip, ip, u16p, ip, ip, u16p, ip, i64p, i64p]
    u32p = C.POINTER(C.c_uint32)
    L.dppr_debug_grouping.argtypes = [vp, C.c_int32, C.c_int32, u32p, u32p, ip, ip, ip]
    L.dppr_heartbeat.restype = C.c_ulonglong
    L.dppr_topk.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, ip, dp, dp, ip]
    L.dppr_group_topk.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, ip, dp, dp, ip]
    L.dppr_read_at.argtypes = [vp, C.c_int32, ip, C.c_int32, dp, dp]
    L.dppr_group_read_at.argtypes = [vp, C.c_int32, ip, C.c_int32, dp, dp]
    L.dppr_debug_live_bytes.argtypes = [i64p, i64p]
    L.dppr_group_sources.argtypes = [vp, C.c_int32, ip, ip]
    L.dppr_group_replace_source.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, fp]
    L.dppr_group_add_source.argtypes = [vp, C.c_int32, C.c_int32, ip, fp]
    L.dppr_group_remove_source.argtypes = [vp, C.c_int32, C.c_int32]
    L.dppr_group_topk_weighted.argtypes = [vp, C.c_int32, dp, C.c_int32, C.c_int32, C.c_double, ip, dp, ip]
    L.dppr_group_score_at.argtypes = [vp, C.c_int32, dp, C.c_int32, ip, C.c_int32, dp]
    L.dppr_debug_query_ms.argtypes = [vp, fp]
    for name in ("dppr_mark", "dppr_group_mark", "dppr_unmark", "dppr_group_unmark"):
        getattr(L, name).argtypes = [vp, C.c_int32]
    L.dppr_changes.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, C.c_int, ip, dp, dp, ip, ip]
    L.dppr_group_changes.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, C.c_int, ip, dp, dp, ip, ip]
    L.dppr_support.argtypes = [vp, C.c_int32, C.c_double, i64p]
    L.dppr_group_support.argtypes = [vp, C.c_int32, C.c_double, i64p]
    # (ids / p / r as plain addresses: host arrays or device memory, as `dest` says)
    L.dppr_export_sparse.argtypes = [vp, C.c_int32, C.c_double, C.c_int64, C.c_int, i64p, vp, vp, vp]
    L.dppr_group_export_sparse.argtypes = [vp, C.c_int32, C.c_double, C.c_int64, C.c_int, i64p, vp, vp, vp]
    L.dppr_export_dense_dev.argtypes = [vp, C.c_int32, C.c_int, C.c_int, vp]
    L.dppr_patch.argtypes = [vp, C.c_int32, C.c_double, C.c_double, C.c_int64, C.c_int64, C.c_int, C.c_int, vp]
    L.dppr_group_patch.argtypes = [vp, C.c_int32, C.c_double, C.c_double, C.c_int64, C.c_int64, C.c_int, C.c_int, vp]
    L.dppr_group_export_dense_dev.argtypes = [vp, C.c_int32, C.c_int, C.c_int, C.c_int, vp]
    L.dppr_dot_dense_dev.argtypes = [vp, C.c_int32, C.c_int, vp, C.c_int, C.c_int, C.c_int32, C.c_int, vp]
    L.dppr_group_dot_dense_dev.argtypes = [vp, C.c_int32, C.c_int, vp, C.c_int, C.c_int, C.c_int32, C.c_int, vp]
    L.dppr_dot_sparse.argtypes = [vp, C.c_int32, C.c_int, i64p, vp, vp, C.c_int, C.c_int32, C.c_int, vp]
    L.dppr_group_dot_sparse.argtypes = [vp, C.c_int32, C.c_int, i64p, vp, vp, C.c_int, C.c_int32, C.c_int, vp]
    # (out_ends as a plain address: a host array or device memory, as `dest` says; corr / sumsq may be NULL)
    L.dppr_walks.argtypes = [vp, C.c_int32, ip, C.c_int32, C.c_int32, C.c_uint64, C.c_int, vp]
    L.dppr_refine_at.argtypes = [vp, C.c_int32, C.c_int32, ip, C.c_int32, C.c_int32, C.c_uint64, vp, vp, vp]
    L.dppr_group_refine_at.argtypes = [vp, C.c_int32, C.c_int32, ip, C.c_int32, C.c_int32, C.c_uint64, vp, vp, vp]
    L.dppr_debug_id_map.argtypes = [vp, ip]
    # (best as a plain address: one record, or n of a group; ids / cut_out / cut_in / vol may be NULL)
    L.dppr_cluster.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, vp, vp, vp, vp, vp]
    L.dppr_group_cluster.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, vp, vp, vp, vp, vp]
    # (counts / offsets are host arrays; ids / p / row_ptr / col as plain addresses, host or device by `dest`, NULL allowed)
    L.dppr_subgraph.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int64, C.c_int, vp, vp, vp, vp, vp, vp]
    L.dppr_group_subgraph.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int64, C.c_int, vp, vp, vp, vp, vp, vp]
    L.dppr_debug_subgraph_wave_max.argtypes = [vp, C.c_int]
    L.dppr_debug_walk_form.argtypes = [vp, C.c_int]
    L.dppr_add_target_group.argtypes = [vp, i64p, ip, dp, C.c_int32, ip]
    L.dppr_group_replace_target.argtypes = [vp, C.c_int32, C.c_int32, ip, dp, C.c_int32, fp]
    L.dppr_group_targets.argtypes = [vp, C.c_int32, i64p, ip, dp, C.c_int64]
    L.dppr_topk_ranked.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_int32, C.c_double, ip, dp, ip]
    L.dppr_group_topk_ranked.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_int32, C.c_double, ip, dp, ip]
    L.dppr_rank_score_at.argtypes = [vp, C.c_int32, C.c_int32, vp, ip, C.c_int32, dp]
    L.dppr_group_rank_score_at.argtypes = [vp, C.c_int32, C.c_int32, vp, ip, C.c_int32, dp]
    L.dppr_debug_rank_piece.argtypes = [vp, C.c_int]
    L.dppr_position_at.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_double, ip, C.c_int32, ip, ip]
    L.dppr_group_position_at.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_double, ip, C.c_int32, ip, ip]
    L.dppr_debug_position_tile.argtypes = [vp, C.c_int]
    # (out_ids / out_w as plain addresses: host arrays or device memory, as `dest` says; out_w and out_support may be NULL)
    L.dppr_sample.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_double, C.c_uint64, C.c_uint64, C.c_int32, C.c_int, vp, vp, dp, ip, ip]
    L.dppr_group_sample.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_double, C.c_uint64, C.c_uint64, C.c_int32, C.c_int, vp, vp, dp, ip, ip]
    L.dppr_debug_sample_form.argtypes = [vp, C.c_int]
    L.dppr_explain_at.argtypes = [vp, C.c_int32, C.c_int32, ip, C.c_int32, C.c_int32, C.c_int32, vp]
    L.dppr_group_explain_at.argtypes = [vp, C.c_int32, C.c_int32, ip, C.c_int32, C.c_int32, C.c_int32, vp]
    L.dppr_debug_explain.argtypes = [vp, C.c_int, C.c_int]
    L.dppr_certify.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, C.c_int, vp]
    L.dppr_group_certify.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, C.c_int, vp]
    L.dppr_debug_certify.argtypes = [vp, C.c_int, C.c_int]
    L.dppr_forward.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_double, vp]
    L.dppr_forward_push.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int32,
                                    C.c_double, C.c_int32, vp]
    L.dppr_debug_forward_push.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.dppr_ftrack_create.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int32,
                                     C.c_double, C.c_int32, vp, C.POINTER(C.c_int32)]
    L.dppr_ftrack_update.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, vp]
    L.dppr_ftrack_read.argtypes = [vp, C.c_int32, vp]
    L.dppr_ftrack_info.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                   C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int64]
    L.dppr_ftrack_destroy.argtypes = [vp, C.c_int32]
    L.dppr_debug_ftrack_ms.argtypes = [vp, C.POINTER(C.c_float)]
    # (the five arrays as plain addresses: host arrays or device memory, as `dest` says; each may be NULL)
    L.dppr_ftrack_cluster.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, C.c_int64, C.c_int32, C.c_int64, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.dppr_debug_ftrack_cluster.argtypes = [vp, C.c_int, C.c_int]
    L.dppr_ftrack_topk_ranked.argtypes = [vp, C.c_int32, vp, C.c_int32, C.c_double, ip, dp, ip]
    L.dppr_ftrack_rank_score_at.argtypes = [vp, C.c_int32, vp, ip, C.c_int32, dp]
    L.dppr_ftrack_position_at.argtypes = [vp, C.c_int32, vp, C.c_double, ip, C.c_int32, ip, ip]
    # (out_ids / out_w as plain addresses, as dppr_group_sample)
    L.dppr_ftrack_sample.argtypes = [vp, C.c_int32, vp, C.c_double, C.c_uint64, C.c_uint64, C.c_int32, C.c_int, vp, vp, dp, ip, ip]
    L.dppr_debug_ftrack_rank.argtypes = [vp, C.c_int]
    L.dppr_debug_forward.argtypes = [vp, C.c_int, C.c_int]
    L.dppr_assign.argtypes = [vp, ip, C.c_int32, dp, C.c_double, C.c_int, vp, vp, vp, i64p, vp, C.c_int64, i64p, vp, vp, vp]
    L.dppr_assign_at.argtypes = [vp, ip, C.c_int32, dp, C.c_double, ip, C.c_int32, ip, dp, ip, dp]
    for name in EXPORTS:
        if name not in ("dppr_strerror", "dppr_last_error", "dppr_destroy", "dppr_build_id", "dppr_heartbeat"):
            getattr(L, name).restype = C.c_int
    _lib = L
    return L


def rank_metrics(pos_column, ks):
    """MRR and Hits@K of one column of positions (Engine.position_at / group_position_at): (mrr, {K: hits}). A position p >= 0
    contributes 1 / (p + 1) to the mean reciprocal rank and a hit to every K > p; -1 is a miss for both. Host arithmetic, summed
    in input order; an empty column gives zeros."""
    pos = [int(p) for p in np.asarray(pos_column).reshape(-1)]
    ks = [int(k) for k in ks]
    rr, hits = 0.0, {k: 0 for k in ks}
    for p in pos:
        if p < 0:
            continue
        rr += 1.0 / (p + 1)
        for k in ks:
            if p < k:
                hits[k] += 1
    m = len(pos)
    if m == 0:
        return 0.0, {k: 0.0 for k in ks}
    return rr / m, {k: hits[k] / m for k in ks}


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.POINTER(C.c_int32))


FCLUSTER_BY_P, FCLUSTER_BY_P_OVER_DEG = 0, 1
FCLUSTER_ORDERS = {"p": FCLUSTER_BY_P, "deg": FCLUSTER_BY_P_OVER_DEG}


class FCluster(C.Structure):
    """dppr_fcluster_t"""
    _fields_ = [("count", C.c_int64), ("best_size", C.c_int64), ("best_cut", C.c_int64), ("best_vol", C.c_int64), ("best_phi", C.c_double)]

    def as_dict(self):
        return {"count": int(self.count), "best_size": int(self.best_size), "best_cut": int(self.best_cut), "best_vol": int(self.best_vol),
                "best_phi": float(self.best_phi)}


class ForwardTrack:
    """A forward track of an Engine (dppr_ftrack_*). update / read return the dict of Engine.forward_push plus fix [3] int64
    (records applied, distinct tails, distinct heads); the counts are those of the last create or update call."""

    def __init__(self, engine, handle, m):
        self._e, self.handle, self.m, self.created = engine, handle, m, None

    def _out(self, k, min_p, at, dense_p_ptr, dense_r_ptr, dtype, layout):
        """(the FtrackOut of a call, a function that returns the call's dict once it has run)"""
        ip, dp, lp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
        m, n = self.m, max(self.m, 1)
        res = {"rounds_used": np.full(n, -1, dtype=np.int32), "converged": np.full(n, -1, dtype=np.int32), "rem": np.full(n, np.nan),
               "pushes": np.full(n, -1, dtype=np.int64), "left": np.full(n, -1, dtype=np.int64), "work": np.full(3, -1, dtype=np.int64),
               "fix": np.full(3, -1, dtype=np.int64)}
        out = FtrackOut()
        out.rounds_used, out.converged, out.rem = res["rounds_used"].ctypes.data_as(ip), res["converged"].ctypes.data_as(ip), res["rem"].ctypes.data_as(dp)
        out.pushes, out.left, out.work = res["pushes"].ctypes.data_as(lp), res["left"].ctypes.data_as(lp), res["work"].ctypes.data_as(lp)
        out.fix = res["fix"].ctypes.data_as(lp)
        keep = [res]
        if k:
            kk = max(int(k), 1)
            tid, tp, cnt = np.empty((n, kk), dtype=np.int32), np.empty((n, kk)), np.empty(n, dtype=np.int32)
            out.k, out.min_p = int(k), float(min_p)
            out.topk_ids, out.topk_p, out.topk_counts = tid.ctypes.data_as(ip), tp.ctypes.data_as(dp), cnt.ctypes.data_as(ip)
        if at is not None:
            b, _ = _i32(at)
            at_p, at_r = np.empty((max(len(b), 1), n)), np.empty((max(len(b), 1), n))
            out.at_ids, out.n_at, out.at_p, out.at_r = b.ctypes.data_as(ip), len(b), at_p.ctypes.data_as(dp), at_r.ctypes.data_as(dp)
            keep.append(b)
        if dense_p_ptr or dense_r_ptr:
            out.dense_p_dev, out.dense_r_dev, out.dense_dtype, out.dense_layout = dense_p_ptr, dense_r_ptr, int(dtype), int(layout)

        def finish():
            for key in ("rounds_used", "converged", "rem", "pushes", "left"):
                res[key] = res[key][:m]
            if k:
                res["topk"] = [(tid[i, :c].copy(), tp[i, :c].copy()) for i, c in enumerate(cnt[:m])]
            if at is not None:
                res["at_p"] = np.ascontiguousarray(at_p[:len(b), :m].T)
                res["at_r"] = np.ascontiguousarray(at_r[:len(b), :m].T)
            return res
        return out, finish

    def update(self, epoch=-1, max_rounds=64, k=0, min_p=0.0, at=None, dense_p_ptr=None, dense_r_ptr=None, dtype=F64, layout=VERTEX_MAJOR):
        """dppr_ftrack_update: to `epoch`, the track's own (more rounds) or the next one (fix-up, then rounds)."""
        out, finish = self._out(k, min_p, at, dense_p_ptr, dense_r_ptr, dtype, layout)
        self._e._ck(self._e._L.dppr_ftrack_update(self._e._h, self.handle, int(epoch), int(max_rounds), C.byref(out)), "ftrack_update")
        return finish()

    def read(self, k=0, min_p=0.0, at=None, dense_p_ptr=None, dense_r_ptr=None, dtype=F64, layout=VERTEX_MAJOR):
        """dppr_ftrack_read: the outputs of the state as it stands."""
        out, finish = self._out(k, min_p, at, dense_p_ptr, dense_r_ptr, dtype, layout)
        self._e._ck(self._e._L.dppr_ftrack_read(self._e._h, self.handle, C.byref(out)), "ftrack_read")
        return finish()

    def info(self):
        """dict(epoch=, m=, eps=, sets=[(ids, weights), ..])"""
        ep, m, eps = C.c_int32(), C.c_int32(), C.c_double()
        off = np.zeros(FTRACK_MAX + 1, dtype=np.int64)
        L, h = self._e._L, self._e._h
        self._e._ck(L.dppr_ftrack_info(h, self.handle, C.byref(ep), C.byref(m), C.byref(eps), off.ctypes.data_as(C.POINTER(C.c_int64)), None, None, 0),
                    "ftrack_info")
        n = int(off[m.value])
        ids, w = np.empty(max(n, 1), dtype=np.int32), np.empty(max(n, 1))
        self._e._ck(L.dppr_ftrack_info(h, self.handle, None, None, None, None, ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                       w.ctypes.data_as(C.POINTER(C.c_double)), n), "ftrack_info")
        return {"epoch": ep.value, "m": m.value, "eps": eps.value,
                "sets": [(ids[off[i]:off[i + 1]].copy(), w[off[i]:off[i + 1]].copy()) for i in range(m.value)]}

    def cluster(self, order="deg", min_score=0.0, max_len=0, min_size=1, profile=False, device_ptrs=None, cap=None):
        """dppr_ftrack_cluster: the lowest-conductance prefix of every column's FULL order (order "deg": p / (outdeg + 1), "p": raw p;
        score > min_score, at most max_len positions, 0 = all): a list of dicts (count, best_size, best_cut, best_vol, best_phi) in
        column order. profile=True: (that list, offsets [m + 1], ids, score, cut_out, cut_in, vol), the five arrays one CSR over the
        columns; the members of column c's best cluster are ids[offsets[c]:offsets[c] + best_size]. device_ptrs: a dict of raw
        device addresses (ids, score, cut_out, cut_in, vol; each optional) with `cap` entries each: (that list, offsets); nothing is
        written there if offsets[m] > cap."""
        m = self.m
        best, off = (FCluster * max(m, 1))(), np.zeros(max(m, 1) + 1, dtype=np.int64)
        head = (self._e._h, self.handle, FCLUSTER_ORDERS.get(order, order), float(min_score), int(max_len), int(min_size))
        fn, ck = self._e._L.dppr_ftrack_cluster, self._e._ck
        names = ("ids", "score", "cut_out", "cut_in", "vol")
        if device_ptrs is not None:
            ck(fn(*head, int(cap or 0), DEST_DEVICE, C.addressof(best), off.ctypes.data, *[device_ptrs.get(k) for k in names]), "ftrack_cluster")
            return [b.as_dict() for b in best[:m]], off[:m + 1]
        if not profile:
            ck(fn(*head, 0, DEST_HOST, C.addressof(best), off.ctypes.data, None, None, None, None, None), "ftrack_cluster")
            return [b.as_dict() for b in best[:m]]
        ck(fn(*head, 0, DEST_HOST, C.addressof(best), off.ctypes.data, None, None, None, None, None), "ftrack_cluster")  # the size call
        total = int(off[m])
        arrays = [np.empty(total, dtype=dt) for dt in (np.int32, np.float64, np.int64, np.int64, np.int64)]
        if total:   # the fill (the state does not change between the two calls of one thread)
            ck(fn(*head, total, DEST_HOST, C.addressof(best), off.ctypes.data, *[a.ctypes.data for a in arrays]), "ftrack_cluster")
            if int(off[m]) != total:
                raise DpprError("ftrack_cluster: the state changed between the size call and the fill")
        return ([b.as_dict() for b in best[:m]], off[:m + 1].copy(), *arrays)

    # ---- ranked, position and sample queries over the track's p (include/dppr.h: dppr_ftrack_topk_ranked ..) ----
    def topk_ranked(self, k, min_score=0.0, spec=None):
        """Engine.group_topk_ranked over the track's columns: a list of (ids, scores), one per column, trimmed to the count. The score
        is THE SCORE of topk_ranked from the track's own p (a seed without a row included), the degrees and neighbours those of the
        track's epoch, the seeds of a column its start set. spec: Engine.rank_spec()."""
        m, kk = max(self.m, 1), max(int(k), 1)
        ids, sc, cnt = np.empty((m, kk), dtype=np.int32), np.empty((m, kk), dtype=np.float64), np.empty(m, dtype=np.int32)
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        self._e._ck(self._e._L.dppr_ftrack_topk_ranked(self._e._h, self.handle, C.byref(spec) if spec is not None else None, int(k), float(min_score),
                                                       ids.ctypes.data_as(ip), sc.ctypes.data_as(dp), cnt.ctypes.data_as(ip)), "ftrack_topk_ranked")
        return [(ids[i, :c].copy(), sc[i, :c].copy()) for i, c in enumerate(cnt[:self.m])]

    def rank_score_at(self, ids, spec=None):
        """The scores of every column at the given external ids: a [len(ids)][m] array (vertex-major, as Engine.group_rank_score_at)."""
        a, pa = _i32(ids)
        out = np.empty((len(a), max(self.m, 1)), dtype=np.float64)
        self._e._ck(self._e._L.dppr_ftrack_rank_score_at(self._e._h, self.handle, C.byref(spec) if spec is not None else None, pa, len(a),
                                                         out.ctypes.data_as(C.POINTER(C.c_double))), "ftrack_rank_score_at")
        return out[:, :self.m]

    def position_at(self, ids, spec=None, min_score=0.0):
        """Where the given external ids stand in every column's order: (pos int32 [len(ids)][m], counts int32 [m]), as
        Engine.group_position_at; rank_metrics takes a column of pos."""
        a, pa = _i32(ids)
        pos, cnt = np.empty((len(a), max(self.m, 1)), dtype=np.int32), np.empty(max(self.m, 1), dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        self._e._ck(self._e._L.dppr_ftrack_position_at(self._e._h, self.handle, C.byref(spec) if spec is not None else None, float(min_score), pa, len(a),
                                                       pos.ctypes.data_as(ip), cnt.ctypes.data_as(ip)), "ftrack_position_at")
        return pos[:, :self.m], cnt[:self.m]

    def sample(self, S, spec=None, min_score=0.0, seed=0, first=0, with_w=True, device_ptrs=None):
        """S external ids per column drawn with replacement in proportion to the column's score, as Engine.group_sample with the lane
        index = the column: (ids int32 [m][S], w float64 [m][S] or None, total [m], support [m], status [m]). device_ptrs: a dict of
        raw device addresses (ids: m * S int32; w: m * S float64, optional) that take the draws instead: (total, support, status)."""
        m = max(self.m, 1)
        total, support, status = np.empty(m, dtype=np.float64), np.empty(m, dtype=np.int32), np.empty(m, dtype=np.int32)
        head = (self._e._h, self.handle, C.byref(spec) if spec is not None else None, float(min_score), int(seed), int(first), int(S))
        tail = (total.ctypes.data_as(C.POINTER(C.c_double)), support.ctypes.data_as(C.POINTER(C.c_int32)), status.ctypes.data_as(C.POINTER(C.c_int32)))
        fn = self._e._L.dppr_ftrack_sample
        if device_ptrs is not None:
            self._e._ck(fn(*head, DEST_DEVICE, device_ptrs.get("ids"), device_ptrs.get("w"), *tail), "ftrack_sample")
            return total[:self.m], support[:self.m], status[:self.m]
        ids = np.empty((m, max(int(S), 0)), dtype=np.int32)
        w = np.empty((m, max(int(S), 0)), dtype=np.float64) if with_w else None
        self._e._ck(fn(*head, DEST_HOST, ids.ctypes.data, w.ctypes.data if with_w else None, *tail), "ftrack_sample")
        return ids[:self.m], None if w is None else w[:self.m], total[:self.m], support[:self.m], status[:self.m]

    def times_ms(self):
        """With Engine.set_profiling(1): device ms of the engine's last track create / update: [load, fix-up, rounds, store]."""
        out = (C.c_float * 4)()
        self._e._ck(self._e._L.dppr_debug_ftrack_ms(self._e._h, out), "debug_ftrack_ms")
        return [float(x) for x in out]

    def close(self):
        if self.handle >= 0:
            self._e._ck(self._e._L.dppr_ftrack_destroy(self._e._h, self.handle), "ftrack_destroy")
            self.handle = -1


class Engine:
    """One device-resident window graph plus any number of source slots.

    Method names follow the reference's driver interface (gpu/PPRGPU.cuh:179-182,
    gpu/PPRRevPushGPU.cuh): ``GPUBuildSlidingGraph`` -> :meth:`slide`,
    ``IncrementalBatchUpdate`` -> :meth:`incremental_batch_update`,
    ``ExecuteMainLoop(phase)`` -> :meth:`execute_main_loop`; :meth:`update` is the
    whole timed region of ``SlidingWindowExecuteMainLoop``.
    """

    def __init__(self, V, W, directed, max_batch, n_epochs=1, device=0, schedule=SCHEDULE_EAGER,
                 hub_min_degree=None, big_row_edges=None, pull_min_frontier=None, chunk_iters=None, pull_block=None,
                 persistent=None, persist_timeout_us=None, sweep_bitmap=None, binned=None, merge_phases=None, variant=None, group_at_slide=None, resident_slots=None, resident_update=None):
        self._L = lib()
        self._h = C.c_void_p()
        self._batch_len, self._staged_len = {0: 0}, 0
        self._group_n = {}  # group -> number of sources
        self.V, self.W, self.directed, self.c = int(V), int(W), int(directed), int(max_batch)
        self.device = int(device)
        rc = self._L.dppr_create(C.byref(self._h), int(device), self.V, self.W, self.directed, self.c, int(n_epochs))
        if rc:
            self._h = C.c_void_p()
            raise DpprError(f"dppr_create: {self._L.dppr_strerror(rc).decode()}")
        self.set_schedule(schedule)
        if variant is not None:   # the reference's -o: sets the schedule too (1, 3: synchronous)
            self._ck(self._L.dppr_set_variant(self._h, int(variant)), "set_variant")
        if any(v is not None for v in (hub_min_degree, big_row_edges, pull_min_frontier, chunk_iters, pull_block)):
            self._ck(self._L.dppr_set_tuning(self._h, int(hub_min_degree or 256), int(big_row_edges or 512),
                                             int(pull_min_frontier or 0), int(chunk_iters or 0),
                                             int(pull_block or 0)), "set_tuning")
        if sweep_bitmap is not None:
            self._ck(self._L.dppr_set_sweep_bitmap(self._h, int(sweep_bitmap)), "set_sweep_bitmap")
        if group_at_slide is not None:
            self._ck(self._L.dppr_set_batch_grouping(self._h, int(group_at_slide)), "set_batch_grouping")
        if resident_slots is not None:
            self.set_resident_slots(resident_slots)
        if resident_update is not None:
            self._ck(self._L.dppr_set_resident_update(self._h, int(resident_update)), "set_resident_update")
        if merge_phases is not None:   # True / divisor
            self.set_phase_merge(bool(merge_phases), 0 if merge_phases is True or not merge_phases else int(merge_phases))
        if binned is not None:   # int mode, or (mode, ha_tiles, hb_tiles, target_edges, min_ids, chunk_edges, target_a_edges)
            args = (binned,) if isinstance(binned, int) else tuple(binned)
            args = tuple(int(a) for a in args) + (0,) * (7 - len(args))
            self._ck(self._L.dppr_set_binned_sweep(self._h, *args), "set_binned_sweep")
        if persistent is not None or persist_timeout_us is not None:
            self._ck(self._L.dppr_set_persistent(self._h, 1 if persistent is None else int(persistent),
                                                 int(persist_timeout_us or 0)), "set_persistent")

    def _ck(self, rc, what):
        if rc:
            raise DpprError(f"{what}: {self._L.dppr_strerror(rc).decode()} ({self._L.dppr_last_error(self._h).decode()})")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.dppr_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_schedule(self, schedule):
        self._ck(self._L.dppr_set_schedule(self._h, int(schedule)), "set_schedule")

    def set_phase_merge(self, on, eps_divisor=0):
        """One loop for residuals of both signs, run to eps / eps_divisor (include/dppr.h); eager schedule only."""
        self._ck(self._L.dppr_set_phase_merge(self._h, int(on), int(eps_divisor)), "set_phase_merge")

    def bin_tables(self, epoch=-1, arrays=True):
        """Test hook: the binned-sweep tables of an epoch (dppr_debug_bin_tables) as a dict; None when the epoch has none."""
        na, nb, ne, nr, nt, pa, rb = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        rc = self._L.dppr_debug_bin_tables(self._h, int(epoch), C.byref(na), C.byref(nb), C.byref(ne), C.byref(nr), C.byref(nt),
                                           None, None, None, None, None, None, None, C.byref(pa), C.byref(rb))
        out = {"patched": pa.value, "rebuilt": rb.value}
        if rc:
            return None if not arrays else dict(out, valid=False)
        out.update(valid=True, n_a=na.value, n_b=nb.value, n_edges=ne.value, n_runs=nr.value, n_tiles=nt.value)
        if arrays:
            n_blk, n_rb = (ne.value + 63) // 64, (nr.value + 63) // 64
            acut, bcut = np.empty(na.value + 1, np.int32), np.empty(nb.value + 1, np.int32)
            hl, dl = np.empty(max(nr.value, 1), np.uint16), np.empty(max(ne.value, 1), np.uint16)
            tdelta, tb, vb = np.empty(max(nt.value, 1), np.int32), np.empty(n_rb + 1, np.int32), np.empty(n_blk + 1, np.int32)
            i32, u16 = C.POINTER(C.c_int32), C.POINTER(C.c_uint16)
            self._ck(self._L.dppr_debug_bin_tables(self._h, int(epoch), None, None, None, None, None, acut.ctypes.data_as(i32), bcut.ctypes.data_as(i32),
                                                   hl.ctypes.data_as(u16), tdelta.ctypes.data_as(i32), tb.ctypes.data_as(i32), dl.ctypes.data_as(u16),
                                                   vb.ctypes.data_as(i32), None, None), "debug_bin_tables")
            out.update(acut=acut, bcut=bcut, hl=hl[:nr.value], tdelta=tdelta[:nt.value], tb=tb, dl=dl[:ne.value], vb=vb)
        return out

    def renumbering_due(self):
        return bool(self._L.dppr_renumbering_due(self._h))

    def set_batch_grouping(self, at_slide):
        """0 (default): CopyOutDegree + the grouping of a batch's records run inside the timed region, as the reference times them;
        1: at slide time (for epochs already built: on entry to the next update, before its event bracket opens)."""
        self._ck(self._L.dppr_set_batch_grouping(self._h, int(at_slide)), "set_batch_grouping")

    def set_incremental_graph(self, on):
        self._ck(self._L.dppr_set_incremental_graph(self._h, int(on)), "set_incremental_graph")

    def set_group_push(self, enter_pairs=-1, list_cap=0, max_edges=0):
        """Tail of a source group's loop as pushes: -1 automatic threshold, 0 never, N below N frontier pairs."""
        self._ck(self._L.dppr_set_group_push(self._h, int(enter_pairs), int(list_cap), int(max_edges)), "set_group_push")

    def set_renumbering(self, on, growth_pct=0, min_parked=0):
        """Renumbering of the internal ids at slide time (include/dppr.h); 0 keeps a threshold as it is."""
        self._ck(self._L.dppr_set_renumbering(self._h, int(on), int(growth_pct), int(min_parked)), "set_renumbering")

    def id_space(self):
        """dict(ids=swept ids, parked=ids parked with their state, renumberings=, revivals=)"""
        a, b, c, d = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        self._ck(self._L.dppr_id_space(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)), "id_space")
        return {"ids": a.value, "parked": b.value, "renumberings": c.value, "revivals": d.value}

    def set_profiling(self, on):
        self._ck(self._L.dppr_set_profiling(self._h, int(on)), "set_profiling")

    def load_window(self, e1, e2):
        a, pa = _i32(e1)
        b, pb = _i32(e2)
        self._ck(self._L.dppr_load_window(self._h, pa, pb, len(a)), "load_window")
        self._batch_len = {0: 0}   # epoch -> records of its batch (debug_grouping sizes its arrays with it)
        self._staged_len = 0

    def set_batch(self, b1, b2, ins):
        a, pa = _i32(b1)
        b, pb = _i32(b2)
        i = np.ascontiguousarray(ins, dtype=np.uint8)
        self._ck(self._L.dppr_set_batch(self._h, pa, pb, i.ctypes.data_as(C.POINTER(C.c_uint8)), len(a)), "set_batch")
        self._staged_len = len(a)

    def hint_next_batch(self, b1, b2, n1, n2):
        """Lookahead (dppr_hint_next_batch): the id lookups of the next set_batch(b1, b2, ..) / slide(n1, n2) run on helper
        threads from now on. Returns the four arrays as contiguous int32 -- pass THESE objects to set_batch / slide (the
        engine matches the hint by pointer and length) and leave them untouched until then."""
        arrs = [_i32(x) for x in (b1, b2, n1, n2)]
        if len(arrs[0][0]) != len(arrs[1][0]) or len(arrs[2][0]) != len(arrs[3][0]):
            raise DpprError("hint_next_batch: b1 / b2 and n1 / n2 must have equal lengths")
        self._hint_keep = [a for a, _ in arrs]   # (keeps the memory alive until the next hint)
        self._ck(self._L.dppr_hint_next_batch(self._h, arrs[0][1], arrs[1][1], len(arrs[0][0]), arrs[2][1], arrs[3][1], len(arrs[2][0])),
                 "hint_next_batch")
        return tuple(self._hint_keep)

    def slide(self, n1, n2, concurrent=False):
        """GPUBuildSlidingGraph. concurrent=True: dppr_slide_concurrent -- may run (from another thread) beside an update on an older,
        explicitly named epoch; needs n_epochs >= 2."""
        a, pa = _i32(n1)
        b, pb = _i32(n2)
        ep = C.c_int32(-1)
        fn = self._L.dppr_slide_concurrent if concurrent else self._L.dppr_slide
        self._ck(fn(self._h, pa, pb, len(a), C.byref(ep)), "slide")
        self._batch_len[ep.value] = self._staged_len
        self._staged_len = 0
        return ep.value

    def add_source(self, s):
        slot = C.c_int32(-1)
        self._ck(self._L.dppr_add_source(self._h, int(s), C.byref(slot)), "add_source")
        return slot.value

    def init_solve(self, slot, eps, epoch=-1):
        ms = C.c_float(0)
        self._ck(self._L.dppr_init_solve_at(self._h, slot, int(epoch), float(eps), C.byref(ms)), "init_solve")
        return ms.value

    def update(self, slot, eps, epoch=-1):
        ms = C.c_float(0)
        self._ck(self._L.dppr_update(self._h, slot, int(epoch), float(eps), C.byref(ms)), "update")
        return ms.value

    def incremental_batch_update(self, slot, epoch=-1):
        self._ck(self._L.dppr_incremental_batch_update(self._h, slot, int(epoch)), "incremental_batch_update")

    def execute_main_loop(self, slot, phase, eps, epoch=-1):
        self._ck(self._L.dppr_execute_main_loop(self._h, slot, int(epoch), int(phase), float(eps)), "execute_main_loop")

    def read(self, slot):
        p = np.empty(self.V, dtype=np.float64)
        r = np.empty(self.V, dtype=np.float64)
        dp = C.POINTER(C.c_double)
        self._ck(self._L.dppr_read(self._h, slot, p.ctypes.data_as(dp), r.ctypes.data_as(dp)), "read")
        return p, r

    def write(self, slot, p, r):
        p = np.ascontiguousarray(p, dtype=np.float64)
        r = np.ascontiguousarray(r, dtype=np.float64)
        dp = C.POINTER(C.c_double)
        self._ck(self._L.dppr_write(self._h, slot, p.ctypes.data_as(dp), r.ctypes.data_as(dp)), "write")

    def stats(self, slot):
        st = Stats()
        self._ck(self._L.dppr_stats(self._h, slot, C.byref(st)), "stats")
        return st.as_dict()

    def reset_stats(self, slot):
        self._ck(self._L.dppr_reset_stats(self._h, slot), "reset_stats")

    def inspect(self, slot, phase, eps):
        out = np.empty(self.V, dtype=np.int32)
        n = C.c_int32(0)
        self._ck(self._L.dppr_inspect(self._h, slot, int(phase), float(eps),
                                      out.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n)), "inspect")
        return out[:n.value].copy()

    def seed_lists(self, slot, phase):
        out = np.empty(max(4 * self.c, 1), dtype=np.int32)
        n = C.c_int32(0)
        self._ck(self._L.dppr_seed_lists(self._h, slot, int(phase), out.ctypes.data_as(C.POINTER(C.c_int32)),
                                         C.byref(n)), "seed_lists")
        return out[:n.value].copy()

    def read_graph(self, epoch=-1):
        ne = C.c_int32(0)
        self._ck(self._L.dppr_graph_edges(self._h, int(epoch), C.byref(ne)), "graph_edges")
        row = np.empty(self.V + 1, dtype=np.int32)
        col = np.empty(max(ne.value, 1), dtype=np.int32)
        deg = np.empty(self.V, dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        self._ck(self._L.dppr_read_graph(self._h, int(epoch), row.ctypes.data_as(ip), col.ctypes.data_as(ip),
                                         deg.ctypes.data_as(ip)), "read_graph")
        return row, col[:ne.value], deg

    def read_out_graph(self, epoch=-1):
        ne = C.c_int32(0)
        self._ck(self._L.dppr_graph_edges(self._h, int(epoch), C.byref(ne)), "graph_edges")
        row = np.empty(self.V + 1, dtype=np.int32)
        col = np.empty(max(ne.value, 1), dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        self._ck(self._L.dppr_read_out_graph(self._h, int(epoch), row.ctypes.data_as(ip), col.ctypes.data_as(ip)),
                 "read_out_graph")
        return row, col[:ne.value]

    def trace_enable(self, slot, on=True):
        self._ck(self._L.dppr_trace_enable(self._h, slot, int(on)), "trace_enable")

    def trace_get(self, slot):
        ni, nd = C.c_int64(0), C.c_int64(0)
        self._ck(self._L.dppr_trace_get(self._h, slot, C.byref(ni), C.byref(nd), None, None), "trace_get")
        off = np.zeros(ni.value + 1, dtype=np.int64)
        ids = np.zeros(max(nd.value, 1), dtype=np.int32)
        self._ck(self._L.dppr_trace_get(self._h, slot, None, None, off.ctypes.data_as(C.POINTER(C.c_int64)),
                                        ids.ctypes.data_as(C.POINTER(C.c_int32))), "trace_get")
        return [ids[off[i]:off[i + 1]].copy() for i in range(ni.value)]

    # ---- source groups (multi-source batched sweeps) ----
    def add_source_group(self, sources):
        a, pa = _i32(sources)
        gid = C.c_int32(-1)
        self._ck(self._L.dppr_add_source_group(self._h, pa, len(a), C.byref(gid)), "add_source_group")
        self._group_n[gid.value] = len(a)
        return gid.value

    def group_init_solve(self, group, eps, epoch=-1):
        ms = C.c_float(0)
        self._ck(self._L.dppr_group_init_solve_at(self._h, group, int(epoch), float(eps), C.byref(ms)), "group_init_solve")
        return ms.value

    def group_update(self, group, eps, epoch=-1):
        ms = C.c_float(0)
        self._ck(self._L.dppr_group_update(self._h, group, int(epoch), float(eps), C.byref(ms)), "group_update")
        return ms.value

    def group_read(self, group, index):
        p = np.empty(self.V, dtype=np.float64)
        r = np.empty(self.V, dtype=np.float64)
        dp = C.POINTER(C.c_double)
        self._ck(self._L.dppr_group_read(self._h, group, int(index), p.ctypes.data_as(dp), r.ctypes.data_as(dp)),
                 "group_read")
        return p, r

    # ---- sources of a running group (exclusive calls, like add_source_group; include/dppr.h) ----
    def group_sources(self, group):
        """The external ids of the group's sources in lane order."""
        out = np.empty(16, dtype=np.int32)
        n = C.c_int32(0)
        self._ck(self._L.dppr_group_sources(self._h, int(group), out.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n)), "group_sources")
        self._group_n[group] = n.value
        return [int(v) for v in out[:n.value]]

    def group_replace_source(self, group, index, source):
        """Lane `index` of a converged group becomes `source`, solved from scratch at the group's tolerance: ms of the device work."""
        ms = C.c_float(0)
        self._ck(self._L.dppr_group_replace_source(self._h, int(group), int(index), int(source), C.byref(ms)), "group_replace_source")
        return ms.value

    def group_add_source(self, group, source):
        """One more source for a converged group: (its index, ms of the device work)."""
        idx, ms = C.c_int32(-1), C.c_float(0)
        self._ck(self._L.dppr_group_add_source(self._h, int(group), int(source), C.byref(idx), C.byref(ms)), "group_add_source")
        self._group_n[group] = idx.value + 1
        return idx.value, ms.value

    def group_remove_source(self, group, index):
        """Drops source `index`; the sources behind it move down by one."""
        self._ck(self._L.dppr_group_remove_source(self._h, int(group), int(index)), "group_remove_source")
        self.group_sources(group)   # (keeps _group_n in step: group_topk / group_read_at size their outputs from it)

    # ---- weighted vertex sets as the targets of a group (include/dppr.h) ----
    @staticmethod
    def _seed_set(s):
        """(ids, weights) of one lane: a vertex, a sequence of vertices (weight 1.0 each) or a pair (ids, weights)."""
        if np.isscalar(s):
            return np.array([s], dtype=np.int32), np.ones(1)
        if isinstance(s, tuple) and len(s) == 2 and not np.isscalar(s[0]):
            ids, w = np.ascontiguousarray(s[0], dtype=np.int32).ravel(), np.ascontiguousarray(s[1], dtype=np.float64).ravel()
            if len(ids) != len(w):
                raise ValueError("a seed set needs one weight per id")
            return ids, w
        ids = np.ascontiguousarray(s, dtype=np.int32).ravel()
        return ids, np.ones(len(ids))

    def add_target_group(self, sets):
        """A group whose lane i tracks the PPR towards the weighted vertex set sets[i] (see _seed_set); a lane of one seed of
        weight 1.0 is a source lane. Returns the group id."""
        lanes = [self._seed_set(s) for s in sets]
        off = np.zeros(len(lanes) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(i) for i, _ in lanes])
        ids = np.ascontiguousarray(np.concatenate([i for i, _ in lanes]) if lanes else np.zeros(0), dtype=np.int32)
        w = np.ascontiguousarray(np.concatenate([x for _, x in lanes]) if lanes else np.zeros(0), dtype=np.float64)
        gid = C.c_int32(-1)
        self._ck(self._L.dppr_add_target_group(self._h, off.ctypes.data_as(C.POINTER(C.c_int64)), ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                               w.ctypes.data_as(C.POINTER(C.c_double)), len(lanes), C.byref(gid)), "add_target_group")
        self._group_n[gid.value] = len(lanes)
        return gid.value

    def group_replace_target(self, group, index, ids, weights=None):
        """Lane `index` of a converged group becomes the weighted set (ids, weights; weight 1.0 each without weights), solved from
        scratch at the group's tolerance: ms of the device work."""
        ids, w = self._seed_set(ids if weights is None else (ids, weights))
        ms = C.c_float(0)
        self._ck(self._L.dppr_group_replace_target(self._h, int(group), int(index), ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                                   w.ctypes.data_as(C.POINTER(C.c_double)), len(ids), C.byref(ms)), "group_replace_target")
        return ms.value

    def group_targets(self, group, cap=None):
        """The seed sets of the group in lane order, external ids ascending: a list of (ids, weights). With cap: the raw call,
        (offsets[17], ids[cap], weights[cap]) -- the arrays untouched when offsets[16] > cap."""
        off = np.zeros(17, dtype=np.int64)
        i64p, ip, dp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
        if cap is None:
            self._ck(self._L.dppr_group_targets(self._h, int(group), off.ctypes.data_as(i64p), None, None, 0), "group_targets")
            total = int(off[16])
        else:
            total = int(cap)
        ids, w = np.full(max(total, 1), -7, dtype=np.int32), np.full(max(total, 1), -7.0)
        self._ck(self._L.dppr_group_targets(self._h, int(group), off.ctypes.data_as(i64p), ids.ctypes.data_as(ip), w.ctypes.data_as(dp), total),
                 "group_targets")
        if cap is not None:
            return off, ids[:total], w[:total]
        n = len(self.group_sources(group))
        return [(ids[off[i]:off[i + 1]].copy(), w[off[i]:off[i + 1]].copy()) for i in range(n)]

    # ---- queries of a state (top-k and point reads on the device) ----
    def topk(self, slot, k, min_p=0.0):
        """The k vertices of largest p with p > min_p, by p descending then id ascending: (ids, p, r), trimmed to the count."""
        ids, p, r, cnt = self._topk(self._L.dppr_topk, slot, 1, k, min_p, "topk")
        return ids[0, :cnt[0]].copy(), p[0, :cnt[0]].copy(), r[0, :cnt[0]].copy()

    def group_topk(self, group, k, min_p=0.0):
        """topk for every source of a group at once: a list of (ids, p, r), one per source in group order."""
        ids, p, r, cnt = self._topk(self._L.dppr_group_topk, group, self._group_n.get(group, 1), k, min_p, "group_topk")
        return [(ids[i, :c].copy(), p[i, :c].copy(), r[i, :c].copy()) for i, c in enumerate(cnt)]

    def _topk(self, fn, which, n, k, min_p, what):
        kk = max(int(k), 1)
        ids = np.empty((n, kk), dtype=np.int32)
        p = np.empty((n, kk), dtype=np.float64)
        r = np.empty((n, kk), dtype=np.float64)
        cnt = np.empty(n, dtype=np.int32)
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        self._ck(fn(self._h, int(which), int(k), float(min_p), ids.ctypes.data_as(ip), p.ctypes.data_as(dp),
                    r.ctypes.data_as(dp), cnt.ctypes.data_as(ip)), what)
        return ids, p, r, cnt

    def read_at(self, slot, ids):
        """p and r at the given external ids (0.0 where a vertex has no id): two arrays of len(ids)."""
        a, pa = _i32(ids)
        p = np.empty(len(a), dtype=np.float64)
        r = np.empty(len(a), dtype=np.float64)
        dp = C.POINTER(C.c_double)
        self._ck(self._L.dppr_read_at(self._h, int(slot), pa, len(a), p.ctypes.data_as(dp), r.ctypes.data_as(dp)), "read_at")
        return p, r

    def group_read_at(self, group, ids):
        """p and r of every source of a group at the given ids: two [len(ids)][n] arrays (vertex-major, as the state)."""
        a, pa = _i32(ids)
        n = self._group_n.get(group, 1)
        p = np.empty((len(a), n), dtype=np.float64)
        r = np.empty((len(a), n), dtype=np.float64)
        dp = C.POINTER(C.c_double)
        self._ck(self._L.dppr_group_read_at(self._h, int(group), pa, len(a), p.ctypes.data_as(dp), r.ctypes.data_as(dp)),
                 "group_read_at")
        return p, r

    # ---- a group as a weighted set of targets ----
    def _weights(self, group, weights, what):
        """weights as a contiguous [q][n] array, checked here (before the library is called)."""
        w = np.array(weights, dtype=np.float64, order="C", ndmin=2)
        n = self._group_n.get(group, 1)
        if w.ndim != 2 or w.shape[1] != n:
            raise DpprError(f"{what}: weights must be [n] or [q][n] with n = {n} sources, got shape {np.shape(weights)}")
        if not 1 <= w.shape[0] <= 16:
            raise DpprError(f"{what}: 1 to 16 weight vectors per call, got {w.shape[0]}")
        if not np.all(np.isfinite(w)):
            raise DpprError(f"{what}: weights must be finite")
        return w

    def group_topk_weighted(self, group, weights, k, min_score=0.0):
        """The k vertices of largest score = sum_i w_i * p_i (folded in lane order, include/dppr.h) with score > min_score, by score
        descending then id ascending, for every weight vector: a list of (ids, scores), trimmed to the counts. `weights` is [n] or [q][n]."""
        w = self._weights(group, weights, "group_topk_weighted")
        q, kk = w.shape[0], max(int(k), 1)
        ids = np.empty((q, kk), dtype=np.int32)
        sc = np.empty((q, kk), dtype=np.float64)
        cnt = np.empty(q, dtype=np.int32)
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        self._ck(self._L.dppr_group_topk_weighted(self._h, int(group), w.ctypes.data_as(dp), q, int(k), float(min_score),
                                                  ids.ctypes.data_as(ip), sc.ctypes.data_as(dp), cnt.ctypes.data_as(ip)),
                 "group_topk_weighted")
        return [(ids[j, :c].copy(), sc[j, :c].copy()) for j, c in enumerate(cnt)]

    def group_score_at(self, group, weights, ids):
        """The scores of every weight vector at the given external ids: a [len(ids)][q] array."""
        w = self._weights(group, weights, "group_score_at")
        a, pa = _i32(ids)
        out = np.empty((len(a), w.shape[0]), dtype=np.float64)
        dp = C.POINTER(C.c_double)
        self._ck(self._L.dppr_group_score_at(self._h, int(group), w.ctypes.data_as(dp), w.shape[0], pa, len(a),
                                             out.ctypes.data_as(dp)), "group_score_at")
        return out

    # ---- ranked candidates: factor, mask and neighbour exclusion before the selection ----
    @staticmethod
    def rank_spec(factor=FACTOR_NONE, factor_dev=0, factor_dtype=F64, mask=MASK_NONE, mask_dev=0, exclude=0):
        """A dppr_rank_spec_t. factor_dev / mask_dev are integer device addresses ([V] by external id) that the caller keeps alive."""
        return RankSpec(int(factor), int(factor_dtype), int(factor_dev) or None, int(mask), int(mask_dev) or None, int(exclude))

    def _topk_ranked(self, fn, which, n, spec, k, min_score, epoch, what):
        kk = max(int(k), 1)
        ids = np.empty((n, kk), dtype=np.int32)
        sc = np.empty((n, kk), dtype=np.float64)
        cnt = np.empty(n, dtype=np.int32)
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        self._ck(fn(self._h, int(which), int(epoch), C.byref(spec) if spec is not None else None, int(k), float(min_score),
                    ids.ctypes.data_as(ip), sc.ctypes.data_as(dp), cnt.ctypes.data_as(ip)), what)
        return [(ids[i, :c].copy(), sc[i, :c].copy()) for i, c in enumerate(cnt)]

    def topk_ranked(self, slot, k, min_score=0.0, spec=None, epoch=-1):
        """The k vertices of largest score (include/dppr.h: p times or over the spec's factor, +0.0 where masked out or excluded)
        with score > min_score, by score descending then id ascending: (ids, scores), trimmed to the count. spec: rank_spec()."""
        return self._topk_ranked(self._L.dppr_topk_ranked, slot, 1, spec, k, min_score, epoch, "topk_ranked")[0]

    def group_topk_ranked(self, group, k, min_score=0.0, spec=None, epoch=-1):
        """topk_ranked for every lane of a group at once: a list of (ids, scores), one per lane in group order."""
        return self._topk_ranked(self._L.dppr_group_topk_ranked, group, self._group_n.get(group, 1), spec, k, min_score, epoch,
                                 "group_topk_ranked")

    def _rank_score_at(self, fn, which, n, spec, ids, epoch, what):
        a, pa = _i32(ids)
        out = np.empty((len(a), n), dtype=np.float64)
        self._ck(fn(self._h, int(which), int(epoch), C.byref(spec) if spec is not None else None, pa, len(a),
                    out.ctypes.data_as(C.POINTER(C.c_double))), what)
        return out

    def rank_score_at(self, slot, ids, spec=None, epoch=-1):
        """The score of topk_ranked at the given external ids: an array of len(ids)."""
        return self._rank_score_at(self._L.dppr_rank_score_at, slot, 1, spec, ids, epoch, "rank_score_at")[:, 0]

    def group_rank_score_at(self, group, ids, spec=None, epoch=-1):
        """The scores of every lane of a group at the given external ids: a [len(ids)][n] array (vertex-major, as the state)."""
        return self._rank_score_at(self._L.dppr_group_rank_score_at, group, self._group_n.get(group, 1), spec, ids, epoch,
                                   "group_rank_score_at")

    def debug_rank_piece(self, edges):
        """Test hook (dppr_debug_rank_piece): the rows of the seeds are marked in pieces of at most `edges` entries, one wave each;
        1 .. 512, default 512. The results do not depend on it."""
        self._ck(self._L.dppr_debug_rank_piece(self._h, int(edges)), "debug_rank_piece")

    # ---- positions of given vertices in a lane's order ----
    def _position_at(self, fn, which, n, ids, spec, min_score, epoch, what):
        a, pa = _i32(ids)
        pos = np.empty((len(a), n), dtype=np.int32)
        cnt = np.empty(n, dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        self._ck(fn(self._h, int(which), int(epoch), C.byref(spec) if spec is not None else None, float(min_score), pa, len(a),
                    pos.ctypes.data_as(ip), cnt.ctypes.data_as(ip)), what)
        return pos, cnt

    def position_at(self, slot, ids, spec=None, min_score=0.0, epoch=-1):
        """Where the given external ids stand in the order of topk_ranked (include/dppr.h: the number of vertices of larger score,
        or of equal score and smaller id; -1 where the id does not qualify): (pos int32 [len(ids)], the count of qualifying
        vertices)."""
        pos, cnt = self._position_at(self._L.dppr_position_at, slot, 1, ids, spec, min_score, epoch, "position_at")
        return pos[:, 0].copy(), int(cnt[0])

    def group_position_at(self, group, ids, spec=None, min_score=0.0, epoch=-1):
        """position_at for every lane of a group at once: (pos int32 [len(ids)][n], vertex-major as the state, counts int32 [n])."""
        return self._position_at(self._L.dppr_group_position_at, group, self._group_n.get(group, 1), ids, spec, min_score, epoch,
                                 "group_position_at")

    def debug_position_tile(self, queries):
        """Test hook (dppr_debug_position_tile): the count pass holds at most `queries` positions of a lane's order per workgroup and
        pass; 1 .. 4096, 0 (default): the plan's choice. The results do not depend on it."""
        self._ck(self._L.dppr_debug_position_tile(self._h, int(queries)), "debug_position_tile")

    # ---- explain a score: top contributing out-edges and the path to the seeds ----
    def _explain_at(self, fn, which, n, ids, f, depth, epoch, what, want=None):
        a, pa = _i32(ids)
        m, f, depth = len(a), int(f), int(depth)
        shapes = {"deg": ((m,), np.int32), "distinct": ((m,), np.int32), "self": ((m, n), np.float64),
                  "nbr_count": ((m, n), np.int32), "nbr": ((m, n, max(f, 0)), np.int32), "nbr_mult": ((m, n, max(f, 0)), np.int32),
                  "nbr_c": ((m, n, max(f, 0)), np.float64), "len": ((m, n), np.int32), "end": ((m, n), np.int32),
                  "path": ((m, n, max(depth, 0) + 1), np.int32), "path_p": ((m, n, max(depth, 0) + 1), np.float64),
                  "path_c": ((m, n, max(depth, 0)), np.float64)}
        if want is not None:   # (only what is asked for is computed and copied back: the other pointers stay NULL)
            want = [want] if isinstance(want, str) else list(want)
            unknown = [k for k in want if k not in shapes]
            if unknown:
                raise ValueError(f"{what}: unknown outputs {unknown}; the outputs are {list(shapes)}")
            shapes = {k: v for k, v in shapes.items() if k in want}
        res = {k: np.zeros(shape, dtype=dt) for k, (shape, dt) in shapes.items()}
        out = ExplainOut()
        for k, arr in res.items():
            ptr = C.POINTER(C.c_int32 if arr.dtype == np.int32 else C.c_double)
            setattr(out, k, arr.ctypes.data_as(ptr))
        self._ck(fn(self._h, int(which), int(epoch), pa, m, f, depth, C.byref(out)), what)
        return res

    def explain_at(self, slot, ids, f=4, depth=16, epoch=-1, want=None):
        """Why the given external ids have the score they have (include/dppr.h: dppr_explain_at): a dict of numpy arrays -- deg,
        distinct [m]; self, nbr_count, len, end [m]; nbr, nbr_mult, nbr_c [m][f]; path, path_p [m][depth + 1]; path_c [m][depth].
        want: the names of the outputs to compute and return (default: all twelve)."""
        res = self._explain_at(self._L.dppr_explain_at, slot, 1, ids, f, depth, epoch, "explain_at", want)
        return {k: (v if v.ndim == 1 else v[:, 0].copy()) for k, v in res.items()}

    def group_explain_at(self, group, ids, f=4, depth=16, epoch=-1, want=None):
        """explain_at for every lane of a group at once: the same dict with a lane axis after the vertex axis -- self, nbr_count,
        len, end [m][n]; nbr, nbr_mult, nbr_c [m][n][f]; path, path_p [m][n][depth + 1]; path_c [m][n][depth]; deg, distinct [m].
        want: the names of the outputs to compute and return (default: all twelve)."""
        return self._explain_at(self._L.dppr_group_explain_at, group, self._group_n.get(group, 1), ids, f, depth, epoch, "group_explain_at",
                                want)

    def debug_explain(self, memo=-1, wave_rows=64):
        """Test hook (dppr_debug_explain): memo -1 the plan's choice, 0 off, 1 on; wave_rows 1 .. 64 entries of a row per wave and
        step. The results depend on neither."""
        self._ck(self._L.dppr_debug_explain(self._h, int(memo), int(wave_rows)), "debug_explain")

    # ---- certify a state: residual norms and the loop invariant ----
    _CERT_RESIDUAL = {"max_abs_r": np.float64, "argmax_r": np.int32, "sum_abs_r": np.float64, "sum_p": np.float64, "n_pos": np.int64,
                      "n_neg": np.int64, "n_nonfinite": np.int64, "n_p_nonzero": np.int64}
    _CERT_INVARIANT = {"inv_max_err": np.float64, "inv_argmax": np.int32}

    def _certify(self, fn, which, n, eps, epoch, residual, invariant, what):
        names = dict(self._CERT_RESIDUAL if residual else {})
        names.update(self._CERT_INVARIANT if invariant else {})
        res = {k: np.zeros(n, dtype=dt) for k, dt in names.items()}
        out = CertifyOut()
        for k, arr in res.items():
            ctype = {np.dtype(np.float64): C.c_double, np.dtype(np.int32): C.c_int32, np.dtype(np.int64): C.c_int64}[arr.dtype]
            setattr(out, k, arr.ctypes.data_as(C.POINTER(ctype)))
        flags = (CERT_RESIDUAL if residual else 0) | (CERT_INVARIANT if invariant else 0)
        self._ck(fn(self._h, int(which), int(epoch), float(eps), flags, C.byref(out)), what)
        res.update(state_epoch=int(out.state_epoch), converged=int(out.converged), conv_eps=float(out.conv_eps))
        return res

    def certify(self, slot, eps, epoch=-1, residual=True, invariant=True):
        """Whether a slot's state is still right, decided on the device (include/dppr.h: dppr_certify): a dict of numpy arrays of
        one entry -- max_abs_r, argmax_r, sum_abs_r, sum_p, n_pos, n_neg, n_nonfinite, n_p_nonzero (residual), inv_max_err,
        inv_argmax (invariant, against the out-edges of `epoch`) -- plus state_epoch, converged and conv_eps of the last solve."""
        return self._certify(self._L.dppr_certify, slot, 1, eps, epoch, residual, invariant, "certify")

    def group_certify(self, group, eps, epoch=-1, residual=True, invariant=True):
        """certify for every lane of a group at once: the same dict, every array with one entry per lane."""
        return self._certify(self._L.dppr_group_certify, group, self._group_n.get(group, 1), eps, epoch, residual, invariant, "group_certify")

    def debug_certify(self, piece_edges=0, wave_rows=0):
        """Test hook (dppr_debug_certify): out-rows longer than piece_edges are summed in pieces; wave_rows short rows share a wave
        (a power of two up to 64); 0: the plan's choice. Both change the order of the additions inside the invariant's sums only."""
        self._ck(self._L.dppr_debug_certify(self._h, int(piece_edges), int(wave_rows)), "debug_certify")

    # ---- vertices drawn in proportion to a lane's score ----
    def _sample(self, fn, which, n, S, spec, min_score, seed, first, epoch, dest, ids_ptr, w_ptr, what):
        total = np.empty(n, dtype=np.float64)
        support = np.empty(n, dtype=np.int32)
        status = np.empty(n, dtype=np.int32)
        self._ck(fn(self._h, int(which), int(epoch), C.byref(spec) if spec is not None else None, float(min_score), int(seed), int(first),
                    int(S), dest, ids_ptr, w_ptr, total.ctypes.data_as(C.POINTER(C.c_double)), support.ctypes.data_as(C.POINTER(C.c_int32)),
                    status.ctypes.data_as(C.POINTER(C.c_int32))), what)
        return total, support, status

    def _sample_host(self, fn, which, n, S, spec, min_score, seed, first, with_w, epoch, what):
        ids = np.empty((n, max(int(S), 0)), dtype=np.int32)
        w = np.empty((n, max(int(S), 0)), dtype=np.float64) if with_w else None
        total, support, status = self._sample(fn, which, n, S, spec, min_score, seed, first, epoch, DEST_HOST, ids.ctypes.data,
                                              w.ctypes.data if with_w else None, what)
        return ids, w, total, support, status

    def sample(self, slot, S, spec=None, min_score=0.0, seed=0, first=0, with_w=True, epoch=-1):
        """S external ids drawn with replacement in proportion to the slot's score (include/dppr.h: THE SCORE of topk_ranked above
        min_score, a sum tree in external-id order, Philox draws number first .. first + S - 1): (ids int32 [S], w float64 [S] or
        None, total, support, status). ids are -1 where status is not SAMPLE_OK."""
        ids, w, total, support, status = self._sample_host(self._L.dppr_sample, slot, 1, S, spec, min_score, seed, first, with_w, epoch, "sample")
        return ids[0], None if w is None else w[0], float(total[0]), int(support[0]), int(status[0])

    def group_sample(self, group, S, spec=None, min_score=0.0, seed=0, first=0, with_w=True, epoch=-1):
        """sample for every lane of a group at once: (ids int32 [n][S], w float64 [n][S] or None, total [n], support [n], status [n]).
        A lane's draws depend on its own weights, its lane index, seed and the draw number alone."""
        return self._sample_host(self._L.dppr_group_sample, group, self._group_n.get(group, 1), S, spec, min_score, seed, first, with_w, epoch,
                                 "group_sample")

    def group_sample_dev(self, group, S, ids_ptr, w_ptr=None, spec=None, min_score=0.0, seed=0, first=0, epoch=-1):
        """... into device memory of the caller: n * S int32 at the raw address ids_ptr and, unless w_ptr is None, n * S float64 at
        w_ptr, lane-major. Returns (total, support, status)."""
        return self._sample(self._L.dppr_group_sample, group, self._group_n.get(group, 1), S, spec, min_score, seed, first, epoch, DEST_DEVICE,
                            ids_ptr, w_ptr, "group_sample")

    def debug_sample_form(self, form):
        """Test hook (dppr_debug_sample_form): SAMPLE_WAVE (default) or SAMPLE_PER_THREAD. The results do not depend on it."""
        self._ck(self._L.dppr_debug_sample_form(self._h, int(form)), "debug_sample_form")

    # ---- forward PPR of any vertex on the resident window ----
    def forward(self, starts, iters=64, tol=0.0, k=0, min_f=0.0, at=None, epoch=-1, dense_ptr=None, dtype=F64, layout=VERTEX_MAJOR):
        """f^K of the walk from each of the external ids `starts` (at most 16) over the in-CSR of `epoch` (include/dppr.h:
        dppr_forward). Returns a dict: iters_used [m] int32 and rem [m]; with k > 0, topk = a list of (ids, f) per start, f
        descending, ties by id ascending, f > min_f; with `at`, at = f at those external ids, [m][len(at)]. dense_ptr: a raw
        device address that takes f by external id, [V][m] (VERTEX_MAJOR) or [m][V] (SOURCE_MAJOR) elements of `dtype`."""
        a, pa = _i32(starts)
        m = len(a)
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        res = {"iters_used": np.full(max(m, 1), -1, dtype=np.int32), "rem": np.full(max(m, 1), np.nan)}
        out = ForwardOut()
        out.iters_used, out.rem = res["iters_used"].ctypes.data_as(ip), res["rem"].ctypes.data_as(dp)
        if k:
            kk = max(int(k), 1)
            ids, f, cnt = np.empty((max(m, 1), kk), dtype=np.int32), np.empty((max(m, 1), kk)), np.empty(max(m, 1), dtype=np.int32)
            out.k, out.min_f = int(k), float(min_f)
            out.topk_ids, out.topk_f, out.topk_counts = ids.ctypes.data_as(ip), f.ctypes.data_as(dp), cnt.ctypes.data_as(ip)
        if at is not None:
            b, _ = _i32(at)
            at_f = np.empty((max(len(b), 1), max(m, 1)))
            out.at_ids, out.n_at, out.at_f = b.ctypes.data_as(ip), len(b), at_f.ctypes.data_as(dp)
        if dense_ptr:
            out.dense_dev, out.dense_dtype, out.dense_layout = dense_ptr, int(dtype), int(layout)
        self._ck(self._L.dppr_forward(self._h, int(epoch), pa, m, int(iters), float(tol), C.byref(out)), "forward")
        res["iters_used"], res["rem"] = res["iters_used"][:m], res["rem"][:m]
        if k:
            res["topk"] = [(ids[i, :c].copy(), f[i, :c].copy()) for i, c in enumerate(cnt[:m])]
        if at is not None:
            res["at"] = np.ascontiguousarray(at_f[:len(b), :m].T)
        return res

    def debug_forward(self, piece_edges=0, team=0):
        """Test hook (dppr_debug_forward): in-rows longer than piece_edges are summed in pieces; `team` lanes share a gathered
        row. 0: the plan's choice. The results do not depend on either."""
        self._ck(self._L.dppr_debug_forward(self._h, int(piece_edges), int(team)), "debug_forward")

    # ---- forward push: local forward PPR from weighted start sets ----
    def forward_push(self, sets, eps, max_rounds=64, k=0, min_p=0.0, at=None, epoch=-1, dense_p_ptr=None, dense_r_ptr=None, dtype=F64,
                     layout=VERTEX_MAJOR):
        """The frontier-driven forward push from each of the start sets `sets` (at most 16) over `epoch` (include/dppr.h:
        dppr_forward_push). A set is a vertex id (one seed of weight 1.0) or a pair (ids, weights). Returns a dict: rounds_used,
        converged [m] int32, rem [m], pushes, left [m] int64, work [3] int64; with k > 0, topk = a list of (ids, p) per set; with
        `at`, at_p and at_r = p and r at those external ids, [m][len(at)]. dense_p_ptr / dense_r_ptr: raw device addresses that
        take p / r by external id, [V][m] (VERTEX_MAJOR) or [m][V] (SOURCE_MAJOR) elements of `dtype`."""
        lanes = [(np.array([s], dtype=np.int32), np.ones(1)) if np.isscalar(s) else s for s in sets]
        m = len(lanes)
        off = np.zeros(m + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(np.atleast_1d(l[0])) for l in lanes])
        ids = np.ascontiguousarray(np.concatenate([np.atleast_1d(l[0]) for l in lanes]) if m else [], dtype=np.int32)
        w = np.ascontiguousarray(np.concatenate([np.atleast_1d(l[1]) for l in lanes]) if m else [], dtype=np.float64)
        if len(w) != len(ids):
            raise ValueError("forward_push: a set needs one weight per id")
        ip, dp, lp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
        n = max(m, 1)
        res = {"rounds_used": np.full(n, -1, dtype=np.int32), "converged": np.full(n, -1, dtype=np.int32), "rem": np.full(n, np.nan),
               "pushes": np.full(n, -1, dtype=np.int64), "left": np.full(n, -1, dtype=np.int64), "work": np.full(3, -1, dtype=np.int64)}
        out = ForwardPushOut()
        out.rounds_used, out.converged, out.rem = res["rounds_used"].ctypes.data_as(ip), res["converged"].ctypes.data_as(ip), res["rem"].ctypes.data_as(dp)
        out.pushes, out.left, out.work = res["pushes"].ctypes.data_as(lp), res["left"].ctypes.data_as(lp), res["work"].ctypes.data_as(lp)
        if k:
            kk = max(int(k), 1)
            tid, tp, cnt = np.empty((n, kk), dtype=np.int32), np.empty((n, kk)), np.empty(n, dtype=np.int32)
            out.k, out.min_p = int(k), float(min_p)
            out.topk_ids, out.topk_p, out.topk_counts = tid.ctypes.data_as(ip), tp.ctypes.data_as(dp), cnt.ctypes.data_as(ip)
        if at is not None:
            b, _ = _i32(at)
            at_p, at_r = np.empty((max(len(b), 1), n)), np.empty((max(len(b), 1), n))
            out.at_ids, out.n_at, out.at_p, out.at_r = b.ctypes.data_as(ip), len(b), at_p.ctypes.data_as(dp), at_r.ctypes.data_as(dp)
        if dense_p_ptr or dense_r_ptr:
            out.dense_p_dev, out.dense_r_dev, out.dense_dtype, out.dense_layout = dense_p_ptr, dense_r_ptr, int(dtype), int(layout)
        self._ck(self._L.dppr_forward_push(self._h, int(epoch), off.ctypes.data_as(lp), ids.ctypes.data_as(ip), w.ctypes.data_as(dp), m,
                                           float(eps), int(max_rounds), C.byref(out)), "forward_push")
        for key in ("rounds_used", "converged", "rem", "pushes", "left"):
            res[key] = res[key][:m]
        if k:
            res["topk"] = [(tid[i, :c].copy(), tp[i, :c].copy()) for i, c in enumerate(cnt[:m])]
        if at is not None:
            res["at_p"] = np.ascontiguousarray(at_p[:len(b), :m].T)
            res["at_r"] = np.ascontiguousarray(at_r[:len(b), :m].T)
        return res

    def debug_ftrack_cluster(self, scan_tile=0, piece_edges=0):
        """Test hook of ForwardTrack.cluster: positions per tile of the prefix sum and entries per piece of a long row (0 or a power of
        two in [64, 4096]; 0: the plan decides). Every setting gives the same bits."""
        self._ck(self._L.dppr_debug_ftrack_cluster(self._h, int(scan_tile), int(piece_edges)), "debug_ftrack_cluster")

    def debug_ftrack_rank(self, tile_rows=0):
        """Test hook of ForwardTrack.topk_ranked / position_at: external ids per tile of the count / fill passes (0 or a power of two in
        [64, 1024]; 0: the plan decides). Every setting gives the same bits."""
        self._ck(self._L.dppr_debug_ftrack_rank(self._h, int(tile_rows)), "debug_ftrack_rank")

    def debug_forward_push(self, piece_edges=0, team=0, chunk_rounds=0):
        """Test hook (dppr_debug_forward_push): piece_edges and team as debug_forward; chunk_rounds rounds are enqueued between
        two read-backs. 0: the plan's choice. The results do not depend on any of them."""
        self._ck(self._L.dppr_debug_forward_push(self._h, int(piece_edges), int(team), int(chunk_rounds)), "debug_forward_push")

    # ---- forward track: forward PPR of weighted start sets kept current under the stream ----
    def ftrack(self, sets, eps, max_rounds=64, k=0, min_p=0.0, at=None, epoch=-1, dense_p_ptr=None, dense_r_ptr=None, dtype=F64,
               layout=VERTEX_MAJOR):
        """A forward track over the start sets `sets` (include/dppr.h: dppr_ftrack_create), created on `epoch`: the arguments of
        forward_push. Returns a ForwardTrack; its `.created` is the result dict of the create call (that of forward_push, plus fix)."""
        lanes = [(np.array([s], dtype=np.int32), np.ones(1)) if np.isscalar(s) else s for s in sets]
        m = len(lanes)
        off = np.zeros(m + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(np.atleast_1d(l[0])) for l in lanes])
        ids = np.ascontiguousarray(np.concatenate([np.atleast_1d(l[0]) for l in lanes]) if m else [], dtype=np.int32)
        w = np.ascontiguousarray(np.concatenate([np.atleast_1d(l[1]) for l in lanes]) if m else [], dtype=np.float64)
        if len(w) != len(ids):
            raise ValueError("ftrack: a set needs one weight per id")
        ip, dp, lp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
        tr = ForwardTrack(self, -1, m)
        out, finish = tr._out(k, min_p, at, dense_p_ptr, dense_r_ptr, dtype, layout)
        handle = C.c_int32(-1)
        self._ck(self._L.dppr_ftrack_create(self._h, int(epoch), off.ctypes.data_as(lp), ids.ctypes.data_as(ip), w.ctypes.data_as(dp), m,
                                            float(eps), int(max_rounds), C.byref(out), C.byref(handle)), "ftrack_create")
        tr.handle = handle.value
        tr.created = finish()
        return tr

    # ---- every vertex to its best lane, across groups ----
    def _assign_classes(self, groups, scale, what):
        """The groups of a call as an int32 array, and its scales as a contiguous [C] array (or None), checked against the class count."""
        g = np.ascontiguousarray(groups, dtype=np.int32).ravel()
        n_classes = sum(self._group_n.get(int(x), 0) for x in g)
        sc = None
        if scale is not None:
            sc = np.ascontiguousarray(scale, dtype=np.float64).ravel()
            if len(sc) != n_classes:
                raise DpprError(f"{what}: scale must hold one entry per class ({n_classes}), got {len(sc)}")
        return g, n_classes, sc

    def assign(self, groups, scale=None, min_score=0.0, prev=None, cap=None, best=True, margin=True, inplace=False, lists=None):
        """dppr_assign with a host destination. The classes are the lanes of `groups` (group handles of this engine, in call
        order); every external id gets the smallest class of largest score = scale[c] * p_c above min_score, or -1. Returns a dict:
        label [V] int32, best / margin [V] (None where not asked for), counts [C + 1] int64 (the last: unassigned), n_flips and
        flips = (id, old, new) against `prev` ([V] int32), ascending by id; flips is None without prev or when n_flips > cap
        (cap defaults to V: everything fits). inplace: the labels are written into `prev` itself (a contiguous int32 array).
        lists: three preallocated int32 arrays of at least cap entries to take the flips."""
        g, n_classes, sc = self._assign_classes(groups, scale, "assign")
        V = self.V
        if prev is not None:
            if inplace and not (isinstance(prev, np.ndarray) and prev.dtype == np.int32 and prev.flags.c_contiguous):
                raise DpprError("assign: an in-place prev must be a contiguous int32 array")
            prev = np.ascontiguousarray(prev, dtype=np.int32)
            if prev.shape != (V,):
                raise DpprError(f"assign: prev must hold V = {V} labels, got shape {prev.shape}")
        label = prev if (inplace and prev is not None) else np.empty(V, dtype=np.int32)
        b = np.empty(V, dtype=np.float64) if best else None
        mg = np.empty(V, dtype=np.float64) if margin else None
        counts = np.zeros(n_classes + 1, dtype=np.int64)
        cap = 0 if prev is None else V if cap is None else int(cap)
        if lists is None and cap > 0:
            lists = tuple(np.full(min(cap, V), -1, dtype=np.int32) for _ in range(3))
        fl = lists if cap > 0 else (None, None, None)
        nf = C.c_int64(0)
        dp, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int64)
        self._ck(self._L.dppr_assign(self._h, g.ctypes.data_as(C.POINTER(C.c_int32)), len(g), sc.ctypes.data_as(dp) if sc is not None else None,
                                     float(min_score), DEST_HOST, label.ctypes.data, b.ctypes.data if best else None,
                                     mg.ctypes.data if margin else None, counts.ctypes.data_as(i64p),
                                     prev.ctypes.data if prev is not None else None, cap, C.byref(nf),
                                     *(a.ctypes.data if a is not None else None for a in fl)), "assign")
        n = int(nf.value)
        flips = tuple(a[:n].copy() for a in fl) if prev is not None and cap > 0 and n <= cap else None
        if prev is not None and cap == 0 and n == 0:
            flips = tuple(np.empty(0, dtype=np.int32) for _ in range(3))
        return {"label": label, "best": b, "margin": mg, "counts": counts, "n_flips": n, "flips": flips}

    def assign_dev(self, groups, label_ptr, scale=None, min_score=0.0, best_ptr=None, margin_ptr=None, prev_ptr=None, cap=0,
                   flip_ptrs=(None, None, None)):
        """dppr_assign into device memory at the given raw addresses ([V] each; prev_ptr may equal label_ptr; the three flip
        lists hold cap entries): (counts [C + 1], n_flips) on the host. Nothing is written to the lists if n_flips > cap."""
        g, n_classes, sc = self._assign_classes(groups, scale, "assign_dev")
        counts = np.zeros(n_classes + 1, dtype=np.int64)
        nf = C.c_int64(0)
        dp, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int64)
        self._ck(self._L.dppr_assign(self._h, g.ctypes.data_as(C.POINTER(C.c_int32)), len(g), sc.ctypes.data_as(dp) if sc is not None else None,
                                     float(min_score), DEST_DEVICE, label_ptr or None, best_ptr or None, margin_ptr or None,
                                     counts.ctypes.data_as(i64p), prev_ptr or None, int(cap), C.byref(nf),
                                     *(a or None for a in flip_ptrs)), "assign_dev")
        return counts, int(nf.value)

    def assign_at(self, groups, ids, scale=None, min_score=0.0):
        """dppr_assign_at: (label, best, second_label, margin) at the given external ids, arrays of len(ids)."""
        g, _, sc = self._assign_classes(groups, scale, "assign_at")
        a, pa = _i32(ids)
        m = len(a)
        label, second = np.empty(m, dtype=np.int32), np.empty(m, dtype=np.int32)
        b, mg = np.empty(m, dtype=np.float64), np.empty(m, dtype=np.float64)
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        self._ck(self._L.dppr_assign_at(self._h, g.ctypes.data_as(ip), len(g), sc.ctypes.data_as(dp) if sc is not None else None,
                                        float(min_score), pa, m, label.ctypes.data_as(ip), b.ctypes.data_as(dp), second.ctypes.data_as(ip),
                                        mg.ctypes.data_as(dp)), "assign_at")
        return label, b, second, mg

    # ---- what a batch moved: marks and the top k of |p - mark| ----
    def mark(self, slot):
        """Keep a copy of the slot's p as it is now (one mark per slot; marking again overwrites it)."""
        self._ck(self._L.dppr_mark(self._h, int(slot)), "mark")

    def group_mark(self, group):
        """Keep a copy of p of every source of the group as it is now (dropped when the group's sources change)."""
        self._ck(self._L.dppr_group_mark(self._h, int(group)), "group_mark")

    def unmark(self, slot):
        self._ck(self._L.dppr_unmark(self._h, int(slot)), "unmark")

    def group_unmark(self, group):
        self._ck(self._L.dppr_group_unmark(self._h, int(group)), "group_unmark")

    def changes(self, slot, k, min_delta=0.0, remark=False):
        """The k vertices of largest |d|, d = p - mark, with |d| > min_delta, by |d| descending then id ascending:
        (ids, delta, p, moved), the arrays trimmed to the count; moved is the number of qualifying vertices whatever k is.
        remark=True: the mark is the current p afterwards (the per-batch feed)."""
        ids, d, p, cnt, moved = self._changes(self._L.dppr_changes, slot, 1, k, min_delta, remark, "changes")
        return ids[0, :cnt[0]].copy(), d[0, :cnt[0]].copy(), p[0, :cnt[0]].copy(), int(moved[0])

    def group_changes(self, group, k, min_delta=0.0, remark=False):
        """changes for every source of a group at once: a list of (ids, delta, p, moved), one per source in group order."""
        ids, d, p, cnt, moved = self._changes(self._L.dppr_group_changes, group, self._group_n.get(group, 1), k, min_delta, remark,
                                              "group_changes")
        return [(ids[i, :c].copy(), d[i, :c].copy(), p[i, :c].copy(), int(moved[i])) for i, c in enumerate(cnt)]

    def _changes(self, fn, which, n, k, min_delta, remark, what):
        kk = max(int(k), 1)
        ids = np.empty((n, kk), dtype=np.int32)
        d = np.empty((n, kk), dtype=np.float64)
        p = np.empty((n, kk), dtype=np.float64)
        cnt = np.zeros(n, dtype=np.int32)
        moved = np.zeros(n, dtype=np.int32)
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        self._ck(fn(self._h, int(which), int(k), float(min_delta), int(bool(remark)), ids.ctypes.data_as(ip), d.ctypes.data_as(dp),
                    p.ctypes.data_as(dp), cnt.ctypes.data_as(ip), moved.ctypes.data_as(ip)), what)
        return ids, d, p, cnt, moved

    # ---- the state leaves the engine: sparse vectors and dense device copies ----
    def support(self, slot, min_p=0.0):
        """How many vertices of the slot have p > min_p."""
        cnt = C.c_int64(-1)
        self._ck(self._L.dppr_support(self._h, int(slot), float(min_p), C.byref(cnt)), "support")
        return cnt.value

    def group_support(self, group, min_p=0.0):
        """How many vertices of every source of the group have p > min_p: an int64 array in lane order."""
        cnt = np.zeros(self._group_n.get(group, 1), dtype=np.int64)
        self._ck(self._L.dppr_group_support(self._h, int(group), float(min_p), cnt.ctypes.data_as(C.POINTER(C.c_int64))), "group_support")
        return cnt

    def export_sparse(self, slot, min_p=0.0, with_r=False):
        """Every vertex of the slot with p > min_p, by id ascending: (offsets [2], ids, p[, r])."""
        return self._export_sparse(self._L.dppr_export_sparse, slot, 1, min_p, with_r, "export_sparse")

    def group_export_sparse(self, group, min_p=0.0, with_r=False):
        """The sparse vectors of every source of a group as one CSR over the sources: (offsets [n + 1], ids, p[, r]); source i's
        entries are [offsets[i], offsets[i + 1]), by id ascending."""
        return self._export_sparse(self._L.dppr_group_export_sparse, group, self._group_n.get(group, 1), min_p, with_r, "group_export_sparse")

    def _export_sparse(self, fn, which, n, min_p, with_r, what):
        i64p = C.POINTER(C.c_int64)
        off = np.zeros(n + 1, dtype=np.int64)
        self._ck(fn(self._h, int(which), float(min_p), 0, DEST_HOST, off.ctypes.data_as(i64p), None, None, None), what)   # the size call
        total = int(off[n])
        ids = np.empty(total, dtype=np.int32)
        p = np.empty(total, dtype=np.float64)
        r = np.empty(total, dtype=np.float64) if with_r else None
        if total:   # the fill (the state does not change between the two calls of one thread)
            self._ck(fn(self._h, int(which), float(min_p), total, DEST_HOST, off.ctypes.data_as(i64p), ids.ctypes.data,
                        p.ctypes.data, r.ctypes.data if with_r else None), what)
            if int(off[n]) != total:
                raise DpprError(f"{what}: the state changed between the size call and the fill")
        return (off, ids, p, r) if with_r else (off, ids, p)

    def export_sparse_dev(self, slot, min_p, cap, ids_ptr, p_ptr, r_ptr=None):
        """dppr_export_sparse into device memory at the given raw addresses (cap entries each; r_ptr may be None): the host
        offsets [2]. Nothing is written if offsets[1] > cap."""
        return self._export_sparse_dev(self._L.dppr_export_sparse, slot, 1, min_p, cap, ids_ptr, p_ptr, r_ptr, "export_sparse_dev")

    def group_export_sparse_dev(self, group, min_p, cap, ids_ptr, p_ptr, r_ptr=None):
        """dppr_group_export_sparse into device memory at the given raw addresses: the host offsets [n + 1]."""
        return self._export_sparse_dev(self._L.dppr_group_export_sparse, group, self._group_n.get(group, 1), min_p, cap, ids_ptr, p_ptr,
                                       r_ptr, "group_export_sparse_dev")

    def _export_sparse_dev(self, fn, which, n, min_p, cap, ids_ptr, p_ptr, r_ptr, what):
        off = np.zeros(n + 1, dtype=np.int64)
        self._ck(fn(self._h, int(which), float(min_p), int(cap), DEST_DEVICE, off.ctypes.data_as(C.POINTER(C.c_int64)),
                    ids_ptr or None, p_ptr or None, r_ptr or None), what)
        return off

    def export_dense_dev(self, slot, dst_ptr, which=DENSE_P, dtype=F64):
        """p (or r) of the slot by external id, V elements of `dtype`, into device memory at the raw address dst_ptr."""
        self._ck(self._L.dppr_export_dense_dev(self._h, int(slot), int(which), int(dtype), dst_ptr or None), "export_dense_dev")

    def group_export_dense_dev(self, group, dst_ptr, which=DENSE_P, dtype=F64, layout=VERTEX_MAJOR):
        """p (or r) of every source of the group by external id, [V][n] or [n][V] elements of `dtype`, into device memory at dst_ptr."""
        self._ck(self._L.dppr_group_export_dense_dev(self._h, int(group), int(which), int(dtype), int(layout), dst_ptr or None),
                 "group_export_dense_dev")

    # ---- the patch feed: what to write into and remove from a replica of {p > min_p} ----
    def patch(self, slot, min_p, min_delta=0.0, remark=PATCH_KEEP_MARK):
        """The patch of a slot against its mark (include/dppr.h: dppr_patch): a dict of up_offsets [2], up_ids, up_p, del_offsets
        [2], del_ids. remark: PATCH_KEEP_MARK, PATCH_REMARK_ALL or PATCH_REMARK_EMITTED (the per-batch feed)."""
        return self._patch(self._L.dppr_patch, slot, 1, min_p, min_delta, remark, "patch")

    def group_patch(self, group, min_p, min_delta=0.0, remark=PATCH_KEEP_MARK):
        """patch for every source of a group at once: two CSRs over the lanes, every lane by id ascending."""
        return self._patch(self._L.dppr_group_patch, group, self._group_n.get(group, 1), min_p, min_delta, remark, "group_patch")

    def _patch(self, fn, which, n, min_p, min_delta, remark, what):
        i64p = C.POINTER(C.c_int64)
        uo, do = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
        out = PatchOut(uo.ctypes.data_as(i64p), None, None, do.ctypes.data_as(i64p), None, -1)
        self._ck(fn(self._h, int(which), float(min_p), float(min_delta), 0, 0, DEST_HOST, PATCH_KEEP_MARK, C.byref(out)), what)   # the size call
        ups, dels = int(uo[n]), int(do[n])
        up_ids, up_p = np.empty(ups, dtype=np.int32), np.empty(ups, dtype=np.float64)
        del_ids = np.empty(dels, dtype=np.int32)
        if ups or dels or int(remark) != PATCH_KEEP_MARK:   # the fill and the re-mark (the state does not change between the two calls of one thread)
            out = PatchOut(uo.ctypes.data_as(i64p), up_ids.ctypes.data if ups else None, up_p.ctypes.data if ups else None,
                           do.ctypes.data_as(i64p), del_ids.ctypes.data if dels else None, -1)
            self._ck(fn(self._h, int(which), float(min_p), float(min_delta), ups, dels, DEST_HOST, int(remark), C.byref(out)), what)
            if out.written != 1 or int(uo[n]) != ups or int(do[n]) != dels:
                raise DpprError(f"{what}: the state changed between the size call and the fill")
        return {"up_offsets": uo, "up_ids": up_ids, "up_p": up_p, "del_offsets": do, "del_ids": del_ids}

    def patch_dev(self, slot, min_p, min_delta, cap_up, cap_del, up_ids_ptr, up_p_ptr, del_ids_ptr, remark=PATCH_KEEP_MARK):
        """dppr_patch into device memory at the given raw addresses (cap_up / cap_del entries): (up_offsets [2], del_offsets [2],
        written). Nothing is written and the mark is not touched if a total exceeds its cap."""
        return self._patch_dev(self._L.dppr_patch, slot, 1, min_p, min_delta, cap_up, cap_del, up_ids_ptr, up_p_ptr, del_ids_ptr, remark,
                               "patch_dev")

    def group_patch_dev(self, group, min_p, min_delta, cap_up, cap_del, up_ids_ptr, up_p_ptr, del_ids_ptr, remark=PATCH_KEEP_MARK):
        """dppr_group_patch into device memory at the given raw addresses: (up_offsets [n + 1], del_offsets [n + 1], written)."""
        return self._patch_dev(self._L.dppr_group_patch, group, self._group_n.get(group, 1), min_p, min_delta, cap_up, cap_del, up_ids_ptr,
                               up_p_ptr, del_ids_ptr, remark, "group_patch_dev")

    def _patch_dev(self, fn, which, n, min_p, min_delta, cap_up, cap_del, up_ids_ptr, up_p_ptr, del_ids_ptr, remark, what):
        i64p = C.POINTER(C.c_int64)
        uo, do = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
        out = PatchOut(uo.ctypes.data_as(i64p), up_ids_ptr or None, up_p_ptr or None, do.ctypes.data_as(i64p), del_ids_ptr or None, -1)
        self._ck(fn(self._h, int(which), float(min_p), float(min_delta), int(cap_up), int(cap_del), DEST_DEVICE, int(remark), C.byref(out)),
                 what)
        return uo, do, int(out.written)

    # ---- the sources scored under a seed distribution: h . p over the vertex axis ----
    def dot_dense_dev(self, slot, h_ptr, F, which=DENSE_P, dtype=F64, layout=H_FEATURE_MAJOR, out_ptr=None):
        """dppr_dot_dense_dev: h ([F][V] or [V][F] elements of `dtype`) in device memory at the raw address h_ptr. The scores [F]
        as a numpy array, or, with out_ptr (a raw device address of F doubles), written there (returns None)."""
        return self._dot_dense(self._L.dppr_dot_dense_dev, slot, 1, h_ptr, F, which, dtype, layout, out_ptr, True, "dot_dense_dev")

    def group_dot_dense_dev(self, group, h_ptr, F, which=DENSE_P, dtype=F64, layout=H_FEATURE_MAJOR, out_ptr=None):
        """dppr_group_dot_dense_dev: the scores [F][n] of every source of the group, as dot_dense_dev."""
        return self._dot_dense(self._L.dppr_group_dot_dense_dev, group, self._group_n.get(group, 1), h_ptr, F, which, dtype, layout,
                               out_ptr, False, "group_dot_dense_dev")

    def _dot_dense(self, fn, handle, n, h_ptr, F, which, dtype, layout, out_ptr, flat, what):
        if out_ptr is not None:
            self._ck(fn(self._h, int(handle), int(which), h_ptr or None, int(dtype), int(layout), int(F), DEST_DEVICE, out_ptr or None), what)
            return None
        out = np.empty((max(int(F), 0), n), dtype=np.float64)
        self._ck(fn(self._h, int(handle), int(which), h_ptr or None, int(dtype), int(layout), int(F), DEST_HOST, out.ctypes.data), what)
        return out[:, 0] if flat else out

    def dot_sparse(self, slot, offsets, ids, w, which=DENSE_P, out_ptr=None):
        """dppr_dot_sparse over a CSR of seed sets in host memory (offsets [F + 1], external ids, weights): the scores [F], or, with
        out_ptr (a raw device address of F doubles), written there (returns None)."""
        return self._dot_sparse(self._L.dppr_dot_sparse, slot, 1, offsets, ids, w, which, out_ptr, True, "dot_sparse")

    def group_dot_sparse(self, group, offsets, ids, w, which=DENSE_P, out_ptr=None):
        """dppr_group_dot_sparse: the scores [F][n] of every source of the group, as dot_sparse."""
        return self._dot_sparse(self._L.dppr_group_dot_sparse, group, self._group_n.get(group, 1), offsets, ids, w, which, out_ptr, False,
                                "group_dot_sparse")

    def dot_sparse_dev(self, slot, offsets, ids_ptr, w_ptr, which=DENSE_P, out_ptr=None):
        """dot_sparse with ids (int32) and w (f64) in device memory at raw addresses; the offsets stay a host array."""
        return self._dot_sparse(self._L.dppr_dot_sparse, slot, 1, offsets, ids_ptr, w_ptr, which, out_ptr, True, "dot_sparse_dev", DEST_DEVICE)

    def group_dot_sparse_dev(self, group, offsets, ids_ptr, w_ptr, which=DENSE_P, out_ptr=None):
        """group_dot_sparse with ids (int32) and w (f64) in device memory at raw addresses; the offsets stay a host array."""
        return self._dot_sparse(self._L.dppr_group_dot_sparse, group, self._group_n.get(group, 1), offsets, ids_ptr, w_ptr, which, out_ptr,
                                False, "group_dot_sparse_dev", DEST_DEVICE)

    def _dot_sparse(self, fn, handle, n, offsets, ids, w, which, out_ptr, flat, what, src=DEST_HOST):
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        F = len(off) - 1
        if src == DEST_HOST:
            ids = np.ascontiguousarray(ids, dtype=np.int32)
            w = np.ascontiguousarray(w, dtype=np.float64)
            if len(off) == 0 or len(ids) != len(w) or len(ids) < int(off[-1]):
                raise DpprError(f"{what}: offsets [F + 1]; ids and w must hold offsets[F] entries each")
            ids_ptr, w_ptr = ids.ctypes.data, w.ctypes.data  # (ids and w stay alive until the call returns)
        else:
            ids_ptr, w_ptr = ids or None, w or None
        offp = off.ctypes.data_as(C.POINTER(C.c_int64))
        if out_ptr is not None:
            self._ck(fn(self._h, int(handle), int(which), offp, ids_ptr, w_ptr, int(src), F, DEST_DEVICE, out_ptr or None), what)
            return None
        out = np.empty((max(F, 0), n), dtype=np.float64)
        self._ck(fn(self._h, int(handle), int(which), offp, ids_ptr, w_ptr, int(src), F, DEST_HOST, out.ctypes.data), what)
        return out[:, 0] if flat else out

    def walks(self, starts, W, seed=0, epoch=-1):
        """Endpoints of W forward walks from each of the external ids `starts` over the out-CSR of `epoch` (dppr_walks):
        int32 [m][W], an external id or -1 for a walk that died. A walk is a function of (start, walk number, seed) alone."""
        a, pa = _i32(starts)
        out = np.empty((len(a), max(int(W), 0)), dtype=np.int32)
        self._ck(self._L.dppr_walks(self._h, int(epoch), pa, len(a), int(W), int(seed), DEST_HOST, out.ctypes.data), "walks")
        return out

    def walks_dev(self, starts, W, seed, out_ptr, epoch=-1):
        """... into device memory of the caller: m * W int32 at the raw address out_ptr."""
        a, pa = _i32(starts)
        self._ck(self._L.dppr_walks(self._h, int(epoch), pa, len(a), int(W), int(seed), DEST_DEVICE, out_ptr), "walks")

    def refine_at(self, slot, ids, W, seed=0, epoch=-1, corr=True, sumsq=True):
        """p refined by W walks from each of `ids` (dppr_refine_at): (est, corr, sumsq), each [m]; corr / sumsq None when not asked for.
        est = p[v] + corr is an unbiased estimate of the fixed point; its standard error is sqrt((sumsq / W - corr^2) / (W - 1))."""
        return self._refine(self._L.dppr_refine_at, slot, 1, ids, W, seed, epoch, corr, sumsq, True, "refine_at")

    def group_refine_at(self, group, ids, W, seed=0, epoch=-1, corr=True, sumsq=True):
        """... for every source of a group from ONE set of walks: each [m][n]."""
        return self._refine(self._L.dppr_group_refine_at, group, self._group_n[group], ids, W, seed, epoch, corr, sumsq, False, "group_refine_at")

    def _refine(self, fn, handle, n, ids, W, seed, epoch, corr, sumsq, flat, what):
        a, pa = _i32(ids)
        outs = [np.empty((len(a), n), dtype=np.float64) if want else None for want in (True, corr, sumsq)]
        self._ck(fn(self._h, int(handle), int(epoch), pa, len(a), int(W), int(seed), *[None if o is None else o.ctypes.data for o in outs]), what)
        return tuple(None if o is None else (o[:, 0] if flat else o) for o in outs)

    def cluster(self, slot, k, min_p=0.0, min_size=1, epoch=-1, profile=False):
        """The lowest-conductance prefix of the slot's top-k order (dppr_cluster): a dict of count, best_size, best_cut, best_vol,
        best_phi. profile=True: (that dict, ids, cut_out, cut_in, vol), the four arrays [k] (ids -1 and counts 0 past `count`)."""
        best, arrays = self._cluster(self._L.dppr_cluster, slot, 1, k, min_p, min_size, epoch, profile, "cluster")
        return (best[0], *[a[0] for a in arrays]) if profile else best[0]

    def group_cluster(self, group, k, min_p=0.0, min_size=1, epoch=-1, profile=False):
        """... for every source of a group at once: a list of dicts in group order; profile=True: (that list, ids, cut_out, cut_in,
        vol), the four arrays [n][k]."""
        best, arrays = self._cluster(self._L.dppr_group_cluster, group, self._group_n.get(group, 1), k, min_p, min_size, epoch, profile,
                                     "group_cluster")
        return (best, *arrays) if profile else best

    def _cluster(self, fn, which, n, k, min_p, min_size, epoch, profile, what):
        kk = max(int(k), 1)
        best = (Cluster * n)()
        arrays = [np.empty((n, kk), dtype=dt) for dt in (np.int32, np.int64, np.int64, np.int64)] if profile else []
        self._ck(fn(self._h, int(which), int(epoch), int(k), float(min_p), int(min_size), C.addressof(best),
                    *([a.ctypes.data for a in arrays] if profile else [None] * 4)), what)
        return [b.as_dict() for b in best], arrays

    def subgraph(self, slot, k, min_p=0.0, epoch=-1):
        """The slot's top-k order and every stored edge among its vertices (dppr_subgraph): (count, ids [k], p [k], row_ptr [k + 1],
        col). Row j holds the positions, ascending, of the heads of v_j's out-edges that lie in the order; ids -1 / p 0 past count."""
        cnt, _, ids, p, row_ptr, col = self._subgraph(self._L.dppr_subgraph, slot, 1, k, min_p, epoch, "subgraph")
        return int(cnt[0]), ids[0], p[0], row_ptr[0], col

    def group_subgraph(self, group, k, min_p=0.0, epoch=-1):
        """... for every source of a group as one CSR over the sources: (counts [n], offsets [n + 1], ids [n][k], p [n][k],
        row_ptr [n][k + 1], col). row_ptr holds absolute indices into col; source i's entries are [offsets[i], offsets[i + 1])."""
        return self._subgraph(self._L.dppr_group_subgraph, group, self._group_n.get(group, 1), k, min_p, epoch, "group_subgraph")

    def _subgraph(self, fn, which, n, k, min_p, epoch, what):
        kk = max(int(k), 1)
        cnt, off = np.zeros(n, dtype=np.int32), np.zeros(n + 1, dtype=np.int64)
        ids, p = np.empty((n, kk), dtype=np.int32), np.empty((n, kk), dtype=np.float64)
        row_ptr = np.empty((n, kk + 1), dtype=np.int64)
        head = (self._h, int(which), int(epoch), int(k), float(min_p))
        self._ck(fn(*head, 0, DEST_HOST, cnt.ctypes.data, off.ctypes.data, ids.ctypes.data, p.ctypes.data, row_ptr.ctypes.data, None), what)  # the size call
        total = int(off[n])
        col = np.empty(total, dtype=np.int32)
        if total:   # the fill (the state does not change between the two calls of one thread)
            self._ck(fn(*head, total, DEST_HOST, cnt.ctypes.data, off.ctypes.data, None, None, None, col.ctypes.data), what)
            if int(off[n]) != total:
                raise DpprError(f"{what}: the state changed between the size call and the fill")
        return cnt, off, ids, p, row_ptr, col

    def group_subgraph_dev(self, group, k, min_p, cap, ids_ptr, p_ptr, row_ptr_ptr, col_ptr, epoch=-1):
        """dppr_group_subgraph into device memory at the given raw addresses (ids / p [n][k], row_ptr [n][k + 1], col cap entries;
        each of the first three may be None): the host (counts [n], offsets [n + 1]). Nothing is written to col if offsets[n] > cap."""
        return self._subgraph_dev(self._L.dppr_group_subgraph, group, self._group_n.get(group, 1), k, min_p, cap, ids_ptr, p_ptr,
                                  row_ptr_ptr, col_ptr, epoch, "group_subgraph_dev")

    def subgraph_dev(self, slot, k, min_p, cap, ids_ptr, p_ptr, row_ptr_ptr, col_ptr, epoch=-1):
        """dppr_subgraph into device memory at the given raw addresses: the host (counts [1], offsets [2])."""
        return self._subgraph_dev(self._L.dppr_subgraph, slot, 1, k, min_p, cap, ids_ptr, p_ptr, row_ptr_ptr, col_ptr, epoch, "subgraph_dev")

    def _subgraph_dev(self, fn, which, n, k, min_p, cap, ids_ptr, p_ptr, row_ptr_ptr, col_ptr, epoch, what):
        cnt, off = np.zeros(n, dtype=np.int32), np.zeros(n + 1, dtype=np.int64)
        self._ck(fn(self._h, int(which), int(epoch), int(k), float(min_p), int(cap), DEST_DEVICE, cnt.ctypes.data, off.ctypes.data,
                    ids_ptr or None, p_ptr or None, row_ptr_ptr or None, col_ptr or None), what)
        return cnt, off

    def set_subgraph_wave_max(self, wave_max):
        """Test and measurement hook (dppr_debug_subgraph_wave_max): rows of the subgraph calls with at most this many entries in
        the order are placed by one wave, the others by a workgroup; 0 .. 256, default 256. The results do not depend on it."""
        self._ck(self._L.dppr_debug_subgraph_wave_max(self._h, int(wave_max)), "set_subgraph_wave_max")

    def id_map(self):
        """Test hook (dppr_debug_id_map): the internal id of every external id, -1 without one."""
        out = np.empty(self.V, dtype=np.int32)
        self._ck(self._L.dppr_debug_id_map(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))), "debug_id_map")
        return out

    def set_walk_form(self, form):
        """Test hook (dppr_debug_walk_form): WALK_REFILL (default) or WALK_PER_THREAD; the same results bit for bit."""
        self._ck(self._L.dppr_debug_walk_form(self._h, int(form)), "debug_walk_form")

    def query_ms(self):
        """With set_profiling on: device ms of the last top-k, changes or export call, first to last kernel (dppr_debug_query_ms)."""
        ms = C.c_float(0)
        self._ck(self._L.dppr_debug_query_ms(self._h, C.byref(ms)), "debug_query_ms")
        return ms.value

    def group_stats(self, group):
        st = Stats()
        self._ck(self._L.dppr_group_stats(self._h, group, C.byref(st)), "group_stats")
        return st.as_dict()

    def group_reset_stats(self, group):
        self._ck(self._L.dppr_group_reset_stats(self._h, group), "group_reset_stats")

    def set_resident_slots(self, sorted_slots):
        """Edge slots of the single-source resident sweep: sorted by gather position (default), or CSR order."""
        self._ck(self._L.dppr_set_resident_slots(self._h, int(sorted_slots)), "set_resident_slots")

    def set_group_resident(self, on):
        self._ck(self._L.dppr_set_group_resident(self._h, int(on)), "set_group_resident")

    def set_group_seeding(self, from_tails):
        self._ck(self._L.dppr_set_group_seeding(self._h, int(from_tails)), "set_group_seeding")

    def synchronize(self):
        self._ck(self._L.dppr_synchronize(self._h), "synchronize")

    def time_batch_grouping(self, epoch=-1, reps=5):
        """ms per batch of CopyOutDegree + the grouping of the records by tail, run on their own as the timed region runs them."""
        ms = C.c_float(0)
        self._ck(self._L.dppr_time_batch_grouping(self._h, int(epoch), int(reps), C.byref(ms)), "time_batch_grouping")
        return ms.value

    def debug_grouping(self, epoch=-1, path=0):
        """Test hook (dppr_debug_grouping): the grouping of the epoch's records by tail on `path` (0: what the timed region runs,
        1: rank, 2: bucket, 3: radix, 4: grouped at slide). Returns (tails, index, raw_tails, path_taken, nb): the grouped tails and
        record indices (uint32), the epoch's tails in batch order (int32, internal ids), the path that ran, and the buckets of path 2."""
        L = self._batch_len.get(max(self._batch_len) if epoch < 0 else int(epoch), 0)   # (an epoch that is not resident: refused below)
        cap = max(4 * self.c, 1)   # (room for the longest batch there can be, whatever L is)
        tails, index = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        raw = np.zeros(cap, np.int32)
        taken, nb = C.c_int32(0), C.c_int32(0)
        u32p = C.POINTER(C.c_uint32)
        self._ck(self._L.dppr_debug_grouping(self._h, int(epoch), int(path), tails.ctypes.data_as(u32p), index.ctypes.data_as(u32p),
                                             raw.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(taken), C.byref(nb)), "debug_grouping")
        return tails[:L].copy(), index[:L].copy(), raw[:L].copy(), taken.value, nb.value

    def debug_dump(self):
        """Post-mortem text of the engine (dppr_debug_dump): callable from another thread than the one stuck in a call."""
        buf = C.create_string_buffer(1 << 16)
        n = self._L.dppr_debug_dump(self._h, buf, len(buf))
        return buf.raw[:max(n, 0)].decode(errors="replace")


def bench_atomics(table_elems, n, scope=0, reps=5, device=0):
    ms = C.c_float(0)
    rc = lib().dppr_bench_atomics(int(device), int(table_elems), int(n), int(scope), int(reps), C.byref(ms))
    if rc:
        raise DpprError(f"bench_atomics: {lib().dppr_strerror(rc).decode()}")
    return ms.value


def bench_line_fills(table_bytes=1 << 30, lines=1 << 26, reps=3, device=0):
    """ms for `lines` random 128-byte line fetches out of a table of table_bytes (dppr_bench_line_fills)."""
    ms = C.c_float(0)
    rc = lib().dppr_bench_line_fills(int(device), int(table_bytes), int(lines), int(reps), C.byref(ms))
    if rc:
        raise DpprError(f"bench_line_fills: {lib().dppr_strerror(rc).decode()}")
    return ms.value


def bench_stream_copy(nbytes=1 << 30, reps=5, device=0):
    """ms per streaming copy of nbytes (read + write)."""
    ms = C.c_float(0)
    rc = lib().dppr_bench_stream_copy(int(device), int(nbytes), int(reps), C.byref(ms))
    if rc:
        raise DpprError(f"bench_stream_copy: {lib().dppr_strerror(rc).decode()}")
    return ms.value


def live_bytes():
    """(device bytes, pinned host bytes) this process holds through the library right now (dppr_debug_live_bytes): the leak check."""
    dev, pin = C.c_int64(0), C.c_int64(0)
    rc = lib().dppr_debug_live_bytes(C.byref(dev), C.byref(pin))
    if rc:
        raise DpprError(f"debug_live_bytes: {lib().dppr_strerror(rc).decode()}")
    return dev.value, pin.value


def build_id():
    """Identity of the loaded library's sources (dppr_build_id; tools/build_id.py computes the tree's)."""
    return lib().dppr_build_id().decode()
