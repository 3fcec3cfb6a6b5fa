// dppr_host_ftrack_rank.hpp -- host side of the ranked, position and sample queries over a forward track (dppr_ftrack_topk_ranked /
// dppr_ftrack_rank_score_at / dppr_ftrack_position_at / dppr_ftrack_sample): the checks that need no device, those of a spec's and
// a destination's device pointers, and the launch sequences of dppr_ftrack_rank.hpp (called with map_mu held, on the solver
// stream, as every query). The track's plane is read in place by external id, never written; no field of an Epoch is written and
// nothing here is reached from the update path. The back halves are the group forms' own: run_select, position_finish,
// sample_finish (dppr_host_query.hpp); the exclusion words, the seeds' row lengths and the piece list live in the ranked family's
// buffers (QueryWork::Rank), the scores in the one scratch state.
#pragma once

namespace {

struct FrCall { // a checked call: the track, its epoch where the spec reads the graph (else NULL), the spec
    const FTrack &tk;
    const Epoch *ep;
    RkSpec sp;
    FrSeeds seeds;
};

FrTrack fr_track(const dppr_engine *e, const FTrack &tk) { return {tk.state.get(), tk.gw, tk.m, e->V, e->d_ext2int.get()}; }

// What every form checks after its own arguments: the track's epoch, where the spec needs one, and the spec's device pointers.
// NULL: fine; otherwise the words of the rejection.
const char *ftrack_rank_refused(dppr_engine *e, const FTrack &tk, const dppr_rank_spec_t *spec, const Epoch **out_ep) {
    *out_ep = nullptr;
    if (fr_needs_epoch(spec)) {
        const Epoch *ep = tk.epoch >= 0 ? find_epoch(e, tk.epoch) : nullptr;
        if (!ep) return "ftrack ranked: the spec reads degrees or neighbours and the track's epoch is no longer resident (update the track or create a new one)";
        *out_ep = ep;
    }
    return rank_spec_ptrs_refused(e, spec);
}

// the maps a call's kernels read: ext2int always (the degree, the seeds' rows), int2ext where neighbours are marked
unsigned fr_maps(const RkSpec &sp) { return MAP_E2I | ((sp.exclude & RK_EXCLUDE_ROWS) ? MAP_I2E : 0u); }

// the exclusion words by external id, the seed table, the seeds' row lengths and the piece list by its bound: in place before the
// first kernel
int fr_mark_workspace(dppr_engine *e, Grow &grow, const FrCall &c) {
    if (!c.sp.exclude) return DPPR_OK;
    QueryWork::Rank &rk = e->q.rk;
    int rc = grow(rk.excl, fr_excl_elems(e->V));
    if (!rc) rc = grow(e->q.fr.seeds, fr_seed_elems(c.seeds.total()));
    if (rc || !(c.sp.exclude & RK_EXCLUDE_ROWS)) return rc;
    const size_t len = rk_len_elems((size_t)c.seeds.total());
    rc = grow(rk.len, len);
    if (!rc) rc = grow(rk.len_pin, len);
    if (!rc) rc = grow(rk.list, std::max<size_t>(rk_piece_cap(fr_rk_seeds(c.seeds), c.ep->Ed, c.sp.exclude, e->rk_piece), 1));
    return rc;
}

// The marking stage, enqueued (its workspace is in place): the words zeroed, the seed table up, the seeds' row lengths read back --
// the one wait of the stage, as in rank_mark_enqueue -- and cut into pieces on the host, one wave of k_fr_mark per piece.
// Returns the words, or NULL: nothing is excluded.
int fr_mark_enqueue(dppr_engine *e, const FrCall &c, const RkGraph &g, const unsigned **out_excl) {
    *out_excl = nullptr;
    if (!c.sp.exclude) return DPPR_OK;
    QueryWork::Rank &rk = e->q.rk;
    const int total = c.seeds.total();
    int *d_seeds = e->q.fr.seeds.get();
    HIP_TRY(hipMemsetAsync(rk.excl, 0, sizeof(unsigned) * fr_excl_elems(e->V), e->stream));
    if (total > 0) HIP_TRY(hipMemcpyAsync(d_seeds, c.tk.ids.data(), sizeof(int32_t) * (size_t)total, hipMemcpyHostToDevice, e->stream));
    size_t n_items = 0;
    if ((c.sp.exclude & RK_EXCLUDE_ROWS) && total > 0) {
        hipLaunchKernelGGL(k_fr_rowlen, dim3(grid_for(total, FR_BLOCK)), dim3(FR_BLOCK), 0, e->stream, c.seeds, d_seeds, e->d_ext2int.get(), g,
                           rk.len.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(rk.len_pin, rk.len, sizeof(int) * 2 * (size_t)total, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        rk_pieces(rk.len_pin.get(), total, c.sp.exclude, e->rk_piece, rk.items);
        n_items = rk.items.size();
        if (n_items > rk.list.capacity()) // (rk_piece_cap bounds what a call can have: a dropped piece would under-exclude)
            return fail(e, DPPR_ERR_HIP, "ftrack ranked: the piece list was too short (rk_piece_cap)");
        if (n_items > 0)
            HIP_TRY(hipMemcpyAsync(rk.list, rk.items.data(), sizeof(unsigned long long) * n_items, hipMemcpyHostToDevice, e->stream));
    }
    const int64_t blocks = std::max<int64_t>(((int64_t)n_items + FR_WAVES - 1) / FR_WAVES, ((int64_t)total + FR_BLOCK - 1) / FR_BLOCK);
    hipLaunchKernelGGL(k_fr_mark, dim3(grid_for(blocks, 1)), dim3(FR_BLOCK), 0, e->stream, c.seeds, d_seeds, e->d_ext2int.get(), e->d_int2ext.get(), g,
                       c.sp.exclude, e->rk_piece, rk.list.get(), (unsigned)n_items, rk.excl.get());
    HIP_TRY(hipGetLastError());
    *out_excl = rk.excl.get();
    return DPPR_OK;
}

// the counts and bases of the tiles, the head of the scan and its pinned twin, the selection's own buffers: in place before the
// first kernel (the scratch state follows the ONE read)
int fr_compact_workspace(dppr_engine *e, Grow &grow, int m, int64_t tiles) {
    QueryWork::FtrackRank &fr = e->q.fr;
    int rc = grow(fr.cnt, fr_cnt_elems(tiles), with_slack(fr_cnt_elems(tiles)));
    if (!rc) rc = grow(fr.base, fr_cnt_elems(tiles), with_slack(fr_cnt_elems(tiles)));
    if (!rc) rc = grow(fr.head, EX_HEAD_BYTES);
    if (!rc) rc = grow(fr.head_pin, EX_HEAD_BYTES);
    if (!rc) rc = topk_workspace(e, grow, m, 1);
    return rc;
}

// The compacted scratch state of a call, enqueued inside the caller's bracket: count, scan, THE read of the call (the kept rows
// size the scratch state and what follows), fill. *out_rows: the rows of the scratch state (0: no vertex qualifies in any column,
// and nothing was filled).
int fr_compact_enqueue(dppr_engine *e, Grow &grow, const FrCall &c, const RkGraph &g, const unsigned *excl, double min_score, int *out_rows) {
    QueryWork::FtrackRank &fr = e->q.fr;
    QueryWork::Scratch &sc = e->q.sc;
    const int m = c.tk.m, tile_rows = fr_tile_rows(e->fr_tile, e->V);
    const int64_t tiles = fr_tiles(e->V, tile_rows);
    const FrTrack tk = fr_track(e, c.tk);
    const RkRule rule = rank_rule(c.sp);
    const dim3 grid((unsigned)fr_grid(tiles)), block(FR_BLOCK);
    ExHead *head = reinterpret_cast<ExHead *>(fr.head.get());
    by_factor(c.sp, [&](auto kind, auto elem) -> int {
        using T = decltype(elem);
        hipLaunchKernelGGL((k_fr_count<decltype(kind)::value, T>), grid, block, 0, e->stream, tk, excl, rule, g, min_score, tile_rows, fr.cnt.get());
        return DPPR_OK;
    });
    if (!fr_scan_fits(tiles)) return fail(e, DPPR_ERR_INVALID, "ftrack ranked: more tiles than the scan counts");
    hipLaunchKernelGGL(k_ex_scan, dim3(1), dim3(EX_LANES * WAVE), 0, e->stream, fr.cnt.get(), 1, (int)tiles, std::numeric_limits<long long>::max(),
                       fr.base.get(), head);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(fr.head_pin, fr.head, sizeof(ExHead), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const long long rows = reinterpret_cast<const ExHead *>(fr.head_pin.get())->offsets[1];
    *out_rows = (int)rows; // (<= V < 2^31)
    if (rows == 0) return DPPR_OK;
    if (int rc = scratch_workspace(e, grow, (size_t)rows, m, 1)) return rc;
    by_factor(c.sp, [&](auto kind, auto elem) -> int {
        using T = decltype(elem);
        hipLaunchKernelGGL((k_fr_fill<decltype(kind)::value, T>), grid, block, 0, e->stream, tk, excl, rule, g, min_score, tile_rows, fr.cnt.get(),
                           fr.base.get(), sc.a.get(), sc.ext.get());
        return DPPR_OK;
    });
    HIP_TRY(hipGetLastError());
    return DPPR_OK;
}

// Top k of every column by the spec's score (arguments, the spec's device pointers and the epoch validated by the caller).
// Results are column-major: [m][k].
int run_ftrack_topk_ranked(dppr_engine *e, const FrCall &c, int k, double min_score, int32_t *out_ids, double *out_score, int32_t *out_counts) {
    if (int rc = query_begin(e, fr_maps(c.sp))) return rc;
    QueryWork::Scratch &sc = e->q.sc;
    const int m = c.tk.m;
    Grow grow{e};
    if (int rc = fr_mark_workspace(e, grow, c)) return rc;
    if (int rc = fr_compact_workspace(e, grow, m, fr_tiles(e->V, fr_tile_rows(e->fr_tile, e->V)))) return rc;
    const RkGraph g = rank_graph(e, c.ep);
    if (int rc = DeviceTime{e}.open()) return rc;
    const unsigned *excl = nullptr;
    if (int rc = fr_mark_enqueue(e, c, g, &excl)) return rc;
    int rows = 0;
    if (int rc = fr_compact_enqueue(e, grow, c, g, excl, min_score, &rows)) return rc;
    if (rows == 0) { // no vertex qualifies in any column: what the selection writes past a count
        if (int rc = DeviceTime{e}.close()) return rc;
        if (int rc = run_end(e)) return rc;
        std::fill(out_counts, out_counts + m, 0);
        std::fill(out_ids, out_ids + (size_t)m * (size_t)k, -1);
        std::fill(out_score, out_score + (size_t)m * (size_t)k, 0.0);
        return DPPR_OK;
    }
    return run_select(e, scratch_state(sc.a, sc.a, m, rows), sc.ext, k, min_score, out_ids, out_score, nullptr, out_counts);
}

// the launch of the point kernel over a call's uploaded ids
int fr_score_at_enqueue(dppr_engine *e, const FrCall &c, const RkGraph &g, const unsigned *excl, const int *d_ids, int n_ids, double *d_out) {
    const FrTrack tk = fr_track(e, c.tk);
    const RkRule rule = rank_rule(c.sp);
    by_factor(c.sp, [&](auto kind, auto elem) -> int {
        using T = decltype(elem);
        hipLaunchKernelGGL((k_fr_score_at<decltype(kind)::value, T>), dim3(grid_for((int64_t)n_ids * tk.m, FR_BLOCK)), dim3(FR_BLOCK), 0, e->stream, tk,
                           d_ids, n_ids, excl, rule, g, d_out);
        return DPPR_OK;
    });
    HIP_TRY(hipGetLastError());
    return DPPR_OK;
}

// the scores at n_ids external ids (validated by the caller like the rest, n_ids > 0), [n_ids][m]
int run_ftrack_rank_score_at(dppr_engine *e, const FrCall &c, const int32_t *ids, int n_ids, double *out_score) {
    if (int rc = query_begin(e, fr_maps(c.sp))) return rc;
    Grow grow{e};
    if (int rc = fr_mark_workspace(e, grow, c)) return rc;
    const RkGraph g = rank_graph(e, c.ep);
    return point_read(e, grow, ids, n_ids, c.tk.m, 1, out_score, nullptr, [&](const int *d_ids, double *d_out, double *) {
        const unsigned *excl = nullptr;
        if (int rc = fr_mark_enqueue(e, c, g, &excl)) return rc;
        return fr_score_at_enqueue(e, c, g, excl, d_ids, n_ids, d_out);
    });
}

// Positions of n_ids external ids in every column's order, and every column's count of qualifying vertices (n_ids == 0: the
// counts alone): the marking, the compacted scratch state, the scores at the ids, then the back half of run_position.
int run_ftrack_position(dppr_engine *e, const FrCall &c, double min_score, const int32_t *ids, int n_ids, int32_t *out_pos, int32_t *out_counts) {
    if (int rc = query_begin(e, fr_maps(c.sp))) return rc;
    QueryWork::Position &ps = e->q.pos;
    const int m = c.tk.m;
    Grow grow{e};
    if (int rc = fr_mark_workspace(e, grow, c)) return rc;
    if (int rc = fr_compact_workspace(e, grow, m, fr_tiles(e->V, fr_tile_rows(e->fr_tile, e->V)))) return rc;
    if (int rc = position_workspace(e, grow, m, n_ids)) return rc;
    const RkGraph g = rank_graph(e, c.ep);
    const PosWork w = pos_work(m, n_ids);
    const RaLayout ra = ra_layout(n_ids, m, 1);
    int *d_ids = reinterpret_cast<int *>(e->q.ra.buf + ra.off_ids);
    double *d_qs = reinterpret_cast<double *>(e->q.ra.buf + ra.off_a);
    if (n_ids > 0) HIP_TRY(hipMemcpyAsync(d_ids, ids, sizeof(int) * (size_t)n_ids, hipMemcpyHostToDevice, e->stream));
    if (int rc = DeviceTime{e}.open()) return rc;
    const unsigned *excl = nullptr;
    if (int rc = fr_mark_enqueue(e, c, g, &excl)) return rc;
    int rows = 0;
    if (int rc = fr_compact_enqueue(e, grow, c, g, excl, min_score, &rows)) return rc;
    if (rows == 0) { // no vertex qualifies in any column: no id has a position
        if (int rc = DeviceTime{e}.close()) return rc;
        if (int rc = run_end(e)) return rc;
        if (out_counts) std::fill(out_counts, out_counts + m, 0);
        if (n_ids > 0) std::fill(out_pos, out_pos + (size_t)n_ids * (size_t)m, -1);
        return DPPR_OK;
    }
    HIP_TRY(hipMemsetAsync(ps.slots, 0, sizeof(unsigned) * w.slot_elems, e->stream));
    if (n_ids > 0)
        if (int rc = fr_score_at_enqueue(e, c, g, excl, d_ids, n_ids, d_qs)) return rc;
    return position_finish(e, rows, m, min_score, n_ids, out_pos, out_counts);
}

// S draws of every column by the spec's score: the marking, the leaves straight from the track's plane (they are in external id
// order: nothing is compacted), then the back half of run_sample.
int run_ftrack_sample(dppr_engine *e, const FrCall &c, double min_score, uint64_t seed, uint64_t first, int S, int dest, int32_t *out_ids, double *out_w,
                      double *out_total, int32_t *out_support, int32_t *out_status) {
    if (int rc = query_begin(e, fr_maps(c.sp))) return rc;
    QueryWork::Sample &sm = e->q.sm;
    const int m = c.tk.m;
    const SmTree t = sample_tree(e->V);
    const SmLayout lay = sample_layout(m, S, dest == DPPR_DEST_HOST, out_w != nullptr);
    Grow grow{e};
    if (int rc = fr_mark_workspace(e, grow, c)) return rc;
    if (int rc = sample_workspace(e, grow, m, t, lay.total_bytes)) return rc;
    const RkGraph g = rank_graph(e, c.ep);
    const RkRule rule = rank_rule(c.sp);
    const FrTrack tk = fr_track(e, c.tk);
    const SmOut head = sample_head(e, lay);
    const bool plain = e->sample_form == 1;
    if (int rc = DeviceTime{e}.open()) return rc;
    const unsigned *excl = nullptr;
    if (int rc = fr_mark_enqueue(e, c, g, &excl)) return rc;
    HIP_TRY(hipMemsetAsync(sm.blk, 0, SM_HEAD_BYTES, e->stream));
    by_factor(c.sp, [&](auto kind, auto elem) -> int {
        using T = decltype(elem);
        hipLaunchKernelGGL((k_fr_leaves<decltype(kind)::value, T>), dim3(t.tiles), dim3(SM_BLOCK), 0, e->stream, tk, excl, rule, g, min_score, t,
                           sm.leaves.get(), sm.nodes.get(), plain ? sm.low.get() : nullptr, head.support);
        return DPPR_OK;
    });
    return sample_finish(e, m, t, seed, first, S, dest, out_ids, out_w, out_total, out_support, out_status);
}

const char *const FR_SPEC_WORDS = "factor 0..3, factor_dtype 0 or 1, mask 0..2, exclude bits 1 | 2 | 4";

int ftrack_topk_ranked_call(dppr_engine *e, int32_t track, const dppr_rank_spec_t *spec, int32_t k, double min_score, int32_t *out_ids,
                            double *out_score, int32_t *out_counts) {
    const FTrack *tk = find_ftrack(e, track);
    if (!tk) return fail(e, DPPR_ERR_INVALID, "ftrack_topk_ranked: no such track");
    if (!fr_topk_args_ok(spec, k, min_score, out_ids, out_score, out_counts))
        return fail(e, DPPR_ERR_INVALID, (std::string("ftrack_topk_ranked: ") + FR_SPEC_WORDS + ", k in [1, DPPR_TOPK_MAX], min_score >= 0, non-null ids / score / counts").c_str());
    HIP_TRY(hipSetDevice(e->device));
    const Epoch *ep = nullptr;
    if (const char *why = ftrack_rank_refused(e, *tk, spec, &ep)) return fail(e, DPPR_ERR_INVALID, why);
    std::lock_guard<std::mutex> map_lk(e->map_mu); // (as dppr_ftrack_read: one state of the id space for the whole call)
    return run_ftrack_topk_ranked(e, FrCall{*tk, ep, rank_spec(spec), fr_seeds(tk->offsets.data(), tk->m)}, k, min_score, out_ids, out_score, out_counts);
}

int ftrack_rank_score_at_call(dppr_engine *e, int32_t track, const dppr_rank_spec_t *spec, const int32_t *ids, int32_t n_ids, double *out_score) {
    const FTrack *tk = find_ftrack(e, track);
    if (!tk) return fail(e, DPPR_ERR_INVALID, "ftrack_rank_score_at: no such track");
    if (!fr_score_at_args_ok(spec, ids, n_ids, e->V, out_score))
        return fail(e, DPPR_ERR_INVALID, (std::string("ftrack_rank_score_at: ") + FR_SPEC_WORDS + ", ids in [0, V), non-null score").c_str());
    HIP_TRY(hipSetDevice(e->device));
    const Epoch *ep = nullptr;
    if (const char *why = ftrack_rank_refused(e, *tk, spec, &ep)) return fail(e, DPPR_ERR_INVALID, why);
    if (n_ids == 0) return DPPR_OK;
    std::lock_guard<std::mutex> map_lk(e->map_mu);
    return run_ftrack_rank_score_at(e, FrCall{*tk, ep, rank_spec(spec), fr_seeds(tk->offsets.data(), tk->m)}, ids, n_ids, out_score);
}

int ftrack_position_call(dppr_engine *e, int32_t track, const dppr_rank_spec_t *spec, double min_score, const int32_t *ids, int32_t n_ids,
                         int32_t *out_pos, int32_t *out_counts) {
    const FTrack *tk = find_ftrack(e, track);
    if (!tk) return fail(e, DPPR_ERR_INVALID, "ftrack_position_at: no such track");
    if (!fr_position_args_ok(spec, min_score, ids, n_ids, e->V, out_pos))
        return fail(e, DPPR_ERR_INVALID, (std::string("ftrack_position_at: ") + FR_SPEC_WORDS + ", min_score >= 0, n_ids in [0, DPPR_POSITION_MAX], ids in [0, V), non-null ids / pos when n_ids > 0").c_str());
    HIP_TRY(hipSetDevice(e->device));
    const Epoch *ep = nullptr;
    if (const char *why = ftrack_rank_refused(e, *tk, spec, &ep)) return fail(e, DPPR_ERR_INVALID, why);
    if (n_ids == 0 && !out_counts) return DPPR_OK;
    std::lock_guard<std::mutex> map_lk(e->map_mu);
    return run_ftrack_position(e, FrCall{*tk, ep, rank_spec(spec), fr_seeds(tk->offsets.data(), tk->m)}, min_score, ids, n_ids, out_pos, out_counts);
}

int ftrack_sample_call(dppr_engine *e, int32_t track, const dppr_rank_spec_t *spec, double min_score, uint64_t seed, uint64_t first, int32_t S, int dest,
                       int32_t *out_ids, double *out_w, double *out_total, int32_t *out_support, int32_t *out_status) {
    const FTrack *tk = find_ftrack(e, track);
    if (!tk) return fail(e, DPPR_ERR_INVALID, "ftrack_sample: no such track");
    if (!fr_sample_args_ok(spec, min_score, tk->m, first, S, dest, out_ids, out_total, out_status))
        return fail(e, DPPR_ERR_INVALID, (std::string("ftrack_sample: ") + FR_SPEC_WORDS + ", min_score >= 0, S in [0, DPPR_SAMPLE_MAX], m * S <= DPPR_SAMPLE_MAX_TOTAL, first + S without a wrap, dest 0 or 1, non-null ids when S > 0, non-null total / status").c_str());
    HIP_TRY(hipSetDevice(e->device));
    const Epoch *ep = nullptr;
    if (const char *why = ftrack_rank_refused(e, *tk, spec, &ep)) return fail(e, DPPR_ERR_INVALID, why);
    if (dest == DPPR_DEST_DEVICE && S > 0 &&
        (!dev_range_ok(e, out_ids, sample_ids_bytes(tk->m, S), sizeof(int32_t)) || (out_w && !dev_range_ok(e, out_w, sample_w_bytes(tk->m, S), sizeof(double)))))
        return fail(e, DPPR_ERR_INVALID, "ftrack_sample: a device destination is aligned device memory of the engine's device, m * S elements inside one allocation");
    std::lock_guard<std::mutex> map_lk(e->map_mu);
    return run_ftrack_sample(e, FrCall{*tk, ep, rank_spec(spec), fr_seeds(tk->offsets.data(), tk->m)}, min_score, seed, first, S, dest, out_ids, out_w,
                             out_total, out_support, out_status);
}

} // namespace
