// dppr_host_fcluster.hpp -- host side of the full-length conductance sweep of a forward track (dppr_ftrack_cluster): the checks that
// need no device, those of a caller's device pointers, and run_ftrack_cluster, the launch sequence of dppr_fcluster.hpp (called with
// map_mu held, on the solver stream, as every query). It stands beside run_ftrack and shares its planes and the track table, not a
// skeleton: the track is read, never written, and no field of an Epoch is written. Nothing here is reached from the update path.
#pragma once

namespace {

// every array a device destination names: aligned device memory of the engine's device, capc entries inside one allocation
bool fc_dest_ok(const dppr_engine *e, int64_t capc, const int32_t *ids, const double *score, const int64_t *cut_out, const int64_t *cut_in,
                const int64_t *vol) {
    const size_t n = (size_t)capc;
    return (!ids || dev_range_ok(e, ids, sizeof(int32_t) * n, sizeof(int32_t))) && (!score || dev_range_ok(e, score, sizeof(double) * n, sizeof(double))) &&
           (!cut_out || dev_range_ok(e, cut_out, sizeof(int64_t) * n, sizeof(int64_t))) &&
           (!cut_in || dev_range_ok(e, cut_in, sizeof(int64_t) * n, sizeof(int64_t))) && (!vol || dev_range_ok(e, vol, sizeof(int64_t) * n, sizeof(int64_t)));
}

// The order of every column and its sweep (arguments, the track, its epoch and a device destination validated by the caller).
// load, count and scan run without a read-back; the qualifying offsets come to the host once and size the sort; fill, sort, rank,
// the edge pass and the multi-tile scan follow; the records come back with the head, the arrays where they are wanted.
int run_ftrack_cluster(dppr_engine *e, const FTrack &tk, const Epoch &ep, int order, double min_score, int64_t max_len, int min_size, int64_t cap,
                       int dest, dppr_fcluster_t *out_best, int64_t *out_offsets, int32_t *out_ids, double *out_score, int64_t *out_cut_out,
                       int64_t *out_cut_in, int64_t *out_vol) {
    if (int rc = query_begin(e, MAP_E2I)) return rc;
    QueryWork::Forward &fq = e->q.fw;
    QueryWork::FCluster &fc = e->q.fc;
    const int V = e->V, m = tk.m, gw = tk.gw, n_int = e->n_int;
    const int S = fc_scan_tile(e->fc_tile), piece = fc_piece(e->fc_piece);
    const bool host = dest == DPPR_DEST_HOST;
    const size_t plane = fw_plane_elems(V, gw);
    const int tiles = (V + FC_TILE - 1) / FC_TILE;
    const size_t tm = (size_t)std::max(tiles, 1) * (size_t)m, rank_elems = (size_t)std::max(n_int, 1) * (size_t)m;
    const size_t list_cap_z = fc_list_cap(m, ep.Ed, piece);
    const unsigned list_cap = (unsigned)std::min<size_t>(list_cap_z, 0xffffffffu);
    Grow grow{e};
    int rc = grow(fq.planes, 2 * plane);
    if (!rc) rc = grow(fc.mask, (size_t)std::max(V, 1));
    if (!rc) rc = grow(fc.cnt, tm);
    if (!rc) rc = grow(fc.base, tm);
    if (!rc) rc = grow(fc.head, FC_HEAD_BYTES);
    if (!rc) rc = grow(fc.head_pin, FC_HEAD_BYTES);
    if (!rc) rc = grow(fc.rank, rank_elems, with_slack(rank_elems));
    if (!rc) rc = grow(fc.list, sizeof(FcItem) * (size_t)list_cap);
    if (rc) return rc;
    double *p = fq.planes.get(), *r = p + plane;
    const double *sp = tk.state.get(), *sr = sp + (size_t)V * gw;
    const int *x2i = e->d_ext2int.get();
    const FcGraph g{ep.out_row_ptr.get(), ep.out_col.get(), ep.row_ptr.get(), ep.adj.get(), n_int};
    ExHead *head = reinterpret_cast<ExHead *>(fc.head.get());
    FcCtl *ctl = reinterpret_cast<FcCtl *>(fc.head.get() + FC_HEAD_OFF_CTL);
    dppr_fcluster_t *d_best = reinterpret_cast<dppr_fcluster_t *>(fc.head.get() + FC_HEAD_OFF_BEST);
    const dim3 tile_grid((unsigned)std::min(std::max(tiles, 1), 2048)), tile_block(FC_TILE), block(FC_BLOCK);

    HIP_TRY(hipMemsetAsync(fc.head, 0, FC_HEAD_BYTES, e->stream));
    if (int rc2 = DeviceTime{e}.open()) return rc2;
    hipLaunchKernelGGL(k_ft_load, dim3((unsigned)grid_for((int64_t)V * gw, FW_BLOCK, 4 * FP_GRID_MAX)), dim3(FW_BLOCK), 0, e->stream, sp, sr, x2i, V, gw, p,
                       r);
    hipLaunchKernelGGL(k_fc_count, tile_grid, tile_block, 0, e->stream, p, gw, m, x2i, V, g, order, min_score, fc.mask.get(), fc.cnt.get());
    hipLaunchKernelGGL(k_ex_scan, dim3(1), dim3(EX_LANES * WAVE), 0, e->stream, fc.cnt.get(), m, tiles, std::numeric_limits<long long>::max(),
                       fc.base.get(), head);
    HIP_TRY(hipGetLastError());
    // THE read of the call: the qualifying offsets size the sort, the order and the scan
    HIP_TRY(hipMemcpyAsync(fc.head_pin, fc.head, sizeof(ExHead), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const FcCols cols = fc_cols(reinterpret_cast<const ExHead *>(fc.head_pin.get())->offsets, m, max_len, S);
    const long long Q = cols.qoff[m], T = cols.off[m], n_tiles = cols.tile0[m];
    const bool fits = fc_fits(T, cap), any = out_ids || out_score || out_cut_out || out_cut_in || out_vol;
    const FcLayout lay = fc_layout(T);
    size_t sort_bytes = 0;
    for (int c = 0; c < m; ++c) {
        const size_t n = (size_t)(cols.qoff[c + 1] - cols.qoff[c]);
        size_t b = 0;
        if (n > 0)
            HIP_TRY(rocprim::radix_sort_pairs_desc(nullptr, b, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int *)nullptr, (int *)nullptr, n,
                                                   0u, 64u, e->stream));
        sort_bytes = std::max(sort_bytes, b);
    }
    const size_t qz = (size_t)std::max(Q, 1ll), tz = (size_t)std::max(T, 1ll), ntz = (size_t)std::max(n_tiles, 1ll);
    rc = grow(fc.keys, 2 * qz, with_slack(2 * qz));
    if (!rc) rc = grow(fc.vals, 2 * qz, with_slack(2 * qz));
    if (!rc) rc = grow(fc.tmp, std::max<size_t>(sort_bytes, 1));
    if (!rc) rc = grow(fc.d, 3 * tz + 6 * ntz, with_slack(3 * tz + 6 * ntz));
    if (!rc) rc = grow(fc.tbest, sizeof(FcBest) * ntz);
    if (!rc) rc = grow(fc.blk, std::max<size_t>(lay.total_bytes, 8), with_slack(std::max<size_t>(lay.total_bytes, 8)));
    if (!rc && host && fits && any) rc = grow(fc.pin, std::max<size_t>(lay.total_bytes, 8), with_slack(std::max<size_t>(lay.total_bytes, 8)));
    if (rc) return rc;
    unsigned long long *keys = fc.keys.get(), *keys2 = keys + qz;
    int *vals = fc.vals.get(), *vals2 = vals + qz;
    long long *d = fc.d.get(), *tsum = d + 3 * tz, *carry = tsum + 3 * ntz;
    FcBest *tbest = reinterpret_cast<FcBest *>(fc.tbest.get());
    unsigned char *blk = fc.blk.get();
    const bool direct = !host && fits; // a device destination that holds the entries is written in place
    int *d_ids = direct && out_ids ? out_ids : reinterpret_cast<int *>(blk + lay.off_ids);
    double *d_score = direct && out_score ? out_score : reinterpret_cast<double *>(blk + lay.off_score);
    long long *d_cut_out = direct && out_cut_out ? reinterpret_cast<long long *>(out_cut_out) : reinterpret_cast<long long *>(blk + lay.off_cut_out);
    long long *d_cut_in = direct && out_cut_in ? reinterpret_cast<long long *>(out_cut_in) : reinterpret_cast<long long *>(blk + lay.off_cut_in);
    long long *d_vol = direct && out_vol ? reinterpret_cast<long long *>(out_vol) : reinterpret_cast<long long *>(blk + lay.off_vol);
    if (Q > 0) {
        hipLaunchKernelGGL(k_fc_fill, tile_grid, tile_block, 0, e->stream, p, gw, m, x2i, V, g, order, fc.mask.get(), fc.base.get(), keys, vals);
        HIP_TRY(hipGetLastError());
        for (int c = 0; c < m; ++c) {
            const size_t n = (size_t)(cols.qoff[c + 1] - cols.qoff[c]);
            if (n == 0) continue;
            size_t tmp = fc.tmp.capacity();
            HIP_TRY(rocprim::radix_sort_pairs_desc(fc.tmp.get(), tmp, keys + cols.qoff[c], keys2 + cols.qoff[c], vals + cols.qoff[c], vals2 + cols.qoff[c],
                                                   n, 0u, 64u, e->stream));
        }
    }
    if (T > 0) {
        HIP_TRY(hipMemsetAsync(fc.rank, 0xff, sizeof(int) * (size_t)n_int * (size_t)m, e->stream));
        hipLaunchKernelGGL(k_fc_rank, dim3((unsigned)grid_for(T, FC_BLOCK, 8192)), block, 0, e->stream, cols, keys2, vals2, x2i, n_int, fc.rank.get(), d_ids,
                           d_score);
        hipLaunchKernelGGL(k_fc_rows, dim3((unsigned)grid_for(T, FC_WAVES, 1 << 16)), block, 0, e->stream, cols, g, x2i, d_ids, fc.rank.get(), piece, d, ctl,
                           reinterpret_cast<FcItem *>(fc.list.get()), list_cap);
        hipLaunchKernelGGL(k_fc_big, dim3((unsigned)grid_for((int64_t)list_cap, FC_WAVES, 1024)), block, 0, e->stream, cols, g, x2i, d_ids, fc.rank.get(),
                           piece, d, ctl, reinterpret_cast<const FcItem *>(fc.list.get()), list_cap);
        const dim3 scan_grid((unsigned)std::min(n_tiles, 4096ll));
        hipLaunchKernelGGL(k_fc_sums, scan_grid, block, 0, e->stream, cols, d, S, tsum);
        hipLaunchKernelGGL(k_fc_carry, dim3((unsigned)m), block, 0, e->stream, cols, tsum, carry);
        hipLaunchKernelGGL(k_fc_apply, scan_grid, block, 0, e->stream, cols, d, carry, S, (long long)ep.Ed, min_size, d_cut_out, d_cut_in, d_vol, tbest);
    }
    hipLaunchKernelGGL(k_fc_best, dim3((unsigned)m), block, 0, e->stream, cols, tbest, d_best);
    HIP_TRY(hipGetLastError());
    if (int rc2 = DeviceTime{e}.close()) return rc2;
    HIP_TRY(hipMemcpyAsync(fc.head_pin, fc.head, FC_HEAD_BYTES, hipMemcpyDeviceToHost, e->stream));
    const bool copy = host && fits && any && T > 0;
    if (copy) {
        const struct { const void *want; size_t off, bytes; } sec[5] = {{out_ids, lay.off_ids, sizeof(int32_t) * (size_t)T},
                                                                        {out_score, lay.off_score, sizeof(double) * (size_t)T},
                                                                        {out_cut_out, lay.off_cut_out, sizeof(int64_t) * (size_t)T},
                                                                        {out_cut_in, lay.off_cut_in, sizeof(int64_t) * (size_t)T},
                                                                        {out_vol, lay.off_vol, sizeof(int64_t) * (size_t)T}};
        for (const auto &s : sec)
            if (s.want) HIP_TRY(hipMemcpyAsync(fc.pin + s.off, blk + s.off, s.bytes, hipMemcpyDeviceToHost, e->stream));
    }
    if (int rc2 = run_end(e)) return rc2; // (a device destination is complete here: any stream of the caller may read it)
    const FcCtl *h_ctl = reinterpret_cast<const FcCtl *>(fc.head_pin.get() + FC_HEAD_OFF_CTL);
    if (h_ctl->n_items > list_cap) return fail(e, DPPR_ERR_HIP, "ftrack_cluster: the piece list was too short (fc_list_cap)");
    for (int c = 0; c <= m; ++c) out_offsets[c] = cols.off[c];
    memcpy(out_best, fc.head_pin.get() + FC_HEAD_OFF_BEST, sizeof(dppr_fcluster_t) * (size_t)m);
    if (copy) {
        if (out_ids) memcpy(out_ids, fc.pin + lay.off_ids, sizeof(int32_t) * (size_t)T);
        if (out_score) memcpy(out_score, fc.pin + lay.off_score, sizeof(double) * (size_t)T);
        if (out_cut_out) memcpy(out_cut_out, fc.pin + lay.off_cut_out, sizeof(int64_t) * (size_t)T);
        if (out_cut_in) memcpy(out_cut_in, fc.pin + lay.off_cut_in, sizeof(int64_t) * (size_t)T);
        if (out_vol) memcpy(out_vol, fc.pin + lay.off_vol, sizeof(int64_t) * (size_t)T);
    }
    return DPPR_OK;
}

int ftrack_cluster_call(dppr_engine *e, int32_t track, int32_t order, double min_score, int64_t max_len, int32_t min_size, int64_t cap, int dest,
                        dppr_fcluster_t *out_best, int64_t *out_offsets, int32_t *out_ids, double *out_score, int64_t *out_cut_out, int64_t *out_cut_in,
                        int64_t *out_vol) {
    const FTrack *tk = find_ftrack(e, track);
    if (!tk) return fail(e, DPPR_ERR_INVALID, "ftrack_cluster: no such track");
    if (!fc_args_ok(order, min_score, max_len, e->V, min_size, cap, dest, out_best, out_offsets, out_ids, out_score, out_cut_out, out_cut_in, out_vol))
        return fail(e, DPPR_ERR_INVALID,
                    "ftrack_cluster: order 0 or 1, min_score >= 0, max_len in [0, V], min_size >= 1, cap >= 0, dest 0 or 1, non-null best / offsets, an array when cap > 0");
    const Epoch *ep = find_epoch(e, tk->epoch);
    if (!ep || tk->epoch < 0) return fail(e, DPPR_ERR_INVALID, "ftrack_cluster: the track's epoch is no longer resident (update the track or create a new one)");
    HIP_TRY(hipSetDevice(e->device));
    if (dest == DPPR_DEST_DEVICE && cap > 0 && !fc_dest_ok(e, fc_cap_clamped(cap, e->V, tk->m), out_ids, out_score, out_cut_out, out_cut_in, out_vol))
        return fail(e, DPPR_ERR_INVALID, "ftrack_cluster: ids / score / cut_out / cut_in / vol must be aligned device memory of the engine's device, cap entries inside one allocation");
    std::lock_guard<std::mutex> map_lk(e->map_mu); // (as dppr_ftrack_read: one state of the id space for the whole call)
    return run_ftrack_cluster(e, *tk, *ep, order, min_score, max_len, min_size, cap, dest, out_best, out_offsets, out_ids, out_score, out_cut_out,
                              out_cut_in, out_vol);
}

} // namespace
