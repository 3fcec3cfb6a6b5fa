// dppr_host_ftrack.hpp -- host side of the forward track (dppr_ftrack_create / _update / _read / _info / _destroy): the checks that
// need no device, the track table of the engine, and run_ftrack, the launch sequence of dppr_ftrack.hpp over the rounds of
// dppr_fpush.hpp (called with map_mu held, on the solver stream, as every query). Nothing here is reached from the update path, and
// no field of an Epoch is written. The forward push's own host side (run_fpush, dppr_host_query.hpp) is left as it is: the two
// share the device pieces and the work space, not a skeleton.
#pragma once

namespace {

enum FtMode { FT_CREATE = 0, FT_MORE = 1, FT_ADVANCE = 2, FT_READ = 3 };

// the per-column figures and the counts of the last create or update call
void ftrack_meta_out(const FTrack &tk, const dppr_ftrack_out_t &out) {
    for (int c = 0; c < tk.m; ++c) {
        if (out.rounds_used) out.rounds_used[c] = tk.rounds_used[c];
        if (out.converged) out.converged[c] = tk.left[c] == 0 ? 1 : 0;
        if (out.rem) out.rem[c] = tk.rem[c];
        if (out.pushes) out.pushes[c] = (int64_t)tk.pushes[c];
        if (out.left) out.left[c] = (int64_t)tk.left[c];
    }
    for (int i = 0; i < 3; ++i) {
        if (out.work) out.work[i] = (int64_t)tk.work[i];
        if (out.fix) out.fix[i] = (int64_t)tk.fix[i];
    }
}

// One call on a track whose ext planes exist: load, (fix-up,) (rounds,) (store,) then the parts `which` names. CREATE: tk.state is
// zero. The track's fields are written only after the device work has succeeded.
int run_ftrack(dppr_engine *e, FTrack &tk, const Epoch &ep, FtMode mode, int max_rounds, uint32_t which, const dppr_ftrack_out_t &out) {
    if (int rc = query_begin(e, MAP_E2I | ((which & FP_TOPK) ? MAP_I2E : 0u))) return rc;
    QueryWork::Forward &fq = e->q.fw;
    const int V = e->V, m = tk.m, gw = tk.gw, n_seeds = (int)tk.offsets[(size_t)m];
    const double eps = tk.eps;
    const int piece = fw_piece(e->fp_piece), T = fw_team(gw, e->fp_team), PP = fw_lane_pieces(gw, T), levels = fw_levels(piece);
    const int chunk = fp_chunk(e->fp_chunk);
    const bool rounds = mode != FT_READ, fixup = mode == FT_ADVANCE && ep.L > 0;
    const int L = fixup ? ep.L : 0;
    const size_t plane = fw_plane_elems(V, gw), part_elems = fw_part_elems(V, m);
    const size_t item_cap = fw_item_cap(ep.Ed, piece), long_cap = fw_long_cap(ep.Ed, piece);
    const size_t list_cap = fp_list_cap(V), mark_cap = fp_mark_cap(V, ep.Ed), words = fp_bitmap_words(V);
    const long long stride = fw_part_stride(V);
    size_t sort_bytes = 0;
    if (fixup)
        HIP_TRY(rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                          (size_t)L, 0u, 32u, e->stream));
    Grow grow{e};
    int rc = grow(fq.planes, 4 * plane);
    if (!rc) rc = grow(fq.fp_head, sizeof(FpHead) + 4 * sizeof(unsigned long long));
    if (!rc) rc = grow(fq.fp_pin, sizeof(FpHead) + 4 * sizeof(unsigned long long));
    if (!rc) rc = grow(fq.fp_seeds, sizeof(FpSeed) * (size_t)n_seeds);
    if (!rc) rc = grow(fq.fp_seeds_pin, sizeof(FpSeed) * (size_t)n_seeds);
    if (!rc) rc = grow(fq.fp_lists, 4 * list_cap);
    if (!rc) rc = grow(fq.fp_bits, words);
    if (!rc) rc = grow(fq.fp_mark, mark_cap);
    if (!rc) rc = grow(fq.part, part_elems);
    if (!rc) rc = grow(fq.items, item_cap);
    if (!rc) rc = grow(fq.longs, sizeof(FwLong) * long_cap);
    if (!rc) rc = grow(fq.pp, item_cap * (size_t)gw);
    if (!rc && fixup) rc = grow(fq.ft_sort, ft_sort_words(L));
    if (!rc && fixup) rc = grow(fq.ft_tmp, sort_bytes ? sort_bytes : 1);
    if (!rc && fixup) rc = grow(fq.ft_c, ft_c_elems(L, gw));
    if (!rc && (which & FP_TOPK)) rc = topk_workspace(e, grow, m, (size_t)(e->n_int + e->n_parked));
    if (!rc && (which & FP_AT)) rc = grow(e->q.ra.buf, ra_layout(out.n_at, m, 2).total_bytes);
    if (rc) return rc;
    double *p = fq.planes.get(), *r = p + plane, *y[2] = {r + plane, r + 2 * plane};
    double *sp = tk.state.get(), *sr = sp + (size_t)V * gw;
    FpHead *head = reinterpret_cast<FpHead *>(fq.fp_head.get());
    unsigned long long *d_fix = reinterpret_cast<unsigned long long *>(fq.fp_head.get() + sizeof(FpHead)); // [3] behind the head
    const FpHead *pin = reinterpret_cast<const FpHead *>(fq.fp_pin.get());
    const unsigned long long *pin_fix = reinterpret_cast<const unsigned long long *>(fq.fp_pin.get() + sizeof(FpHead));
    FpSeed *seeds = reinterpret_cast<FpSeed *>(fq.fp_seeds.get()), *h_seeds = reinterpret_cast<FpSeed *>(fq.fp_seeds_pin.get());
    FwLong *longs = reinterpret_cast<FwLong *>(fq.longs.get());
    const unsigned icap = (unsigned)std::min<size_t>(item_cap, 0xffffffffu), lcap = (unsigned)std::min<size_t>(long_cap, 0xffffffffu);
    const FwGraph g{ep.row_ptr.get(), ep.adj.get(), ep.out_row_ptr.get(), e->n_int, V};
    FpLists ls;
    for (int i = 0; i < 2; ++i) {
        ls.front[i] = fq.fp_lists.get() + (size_t)i * list_cap;
        ls.recv[i] = fq.fp_lists.get() + (size_t)(2 + i) * list_cap;
    }
    ls.bits = fq.fp_bits.get();
    ls.mark = fq.fp_mark.get();
    ls.list_cap = (unsigned)std::min<size_t>(list_cap, 0xffffffffu);
    ls.mark_cap = (unsigned)std::min<size_t>(mark_cap, 0xffffffffu);
    const int *x2i = e->d_ext2int.get();
    const dim3 block(FW_BLOCK);
    const dim3 thread_grid((unsigned)fp_grid(e->n_int, FW_BLOCK)), mark_grid((unsigned)fp_grid(e->n_int, FW_WAVES * (WAVE / FP_MARK_LANES)));
    const dim3 rows_grid((unsigned)std::min(fw_units_grid(e->n_int, T), FP_GRID_MAX));
    const dim3 piece_grid((unsigned)std::min(fw_units_grid((long long)std::min<size_t>(item_cap, 1u << 20), T), FP_GRID_MAX));
    const dim3 long_grid((unsigned)grid_for((int64_t)std::min<size_t>(long_cap, 1u << 16) * m, FW_BLOCK, FP_GRID_MAX));
    const dim3 copy_grid((unsigned)grid_for((int64_t)V * gw, FW_BLOCK, 4 * FP_GRID_MAX));

    HIP_TRY(hipMemsetAsync(head, 0, sizeof(FpHead) + 4 * sizeof(unsigned long long), e->stream));
    HIP_TRY(hipMemsetAsync(y[0], 0, sizeof(double) * 2 * plane, e->stream));
    if (rounds) {
        HIP_TRY(hipMemsetAsync(fq.fp_bits, 0, sizeof(unsigned) * words, e->stream));
        HIP_TRY(hipMemsetAsync(fq.part, 0, sizeof(double) * part_elems, e->stream)); // (+0.0: the tiles of padding)
    }
    if (mode == FT_CREATE) {
        for (int c = 0; c < m; ++c)
            for (int64_t j = tk.offsets[(size_t)c]; j < tk.offsets[(size_t)c + 1]; ++j)
                h_seeds[j] = FpSeed{tk.ids[(size_t)j], c, tk.weights[(size_t)j], -1, 0};
        HIP_TRY(hipMemcpyAsync(seeds, h_seeds, sizeof(FpSeed) * (size_t)n_seeds, hipMemcpyHostToDevice, e->stream));
    }
    if (int rc2 = DeviceTime{e}.open()) return rc2;
    hipLaunchKernelGGL(k_ft_load, copy_grid, block, 0, e->stream, sp, sr, x2i, V, gw, p, r);
    HIP_TRY(hipGetLastError());
    // (profiling: events 2, 3, 4 cut the bracket into load | fix-up | rounds | store)
    if (int rc2 = DeviceTime{e}.record(2)) return rc2;
    int k = 0;
    if (rounds) {
        const bool from_records = ft_candidates_from_records(mode == FT_ADVANCE ? FT_STEP_NEXT : FT_STEP_SAME, tk.converged);
        if (mode == FT_CREATE)
            hipLaunchKernelGGL(k_fp_init, dim3((unsigned)grid_for(n_seeds, FW_BLOCK, FP_GRID_MAX)), block, 0, e->stream, head, seeds, n_seeds, x2i, g, r, gw,
                               ls);
        if (fixup) {
            uint32_t *kt = fq.ft_sort.get(), *kh = kt + L, *idx = kh + L, *st = idx + L, *sh = st + L, *sv = sh + L; // sv: by tail, then by head
            hipLaunchKernelGGL(k_ft_keys, dim3((unsigned)grid_for(L, FW_BLOCK, FP_GRID_MAX)), block, 0, e->stream, ep.b1.get(), ep.b2.get(), L, kt, kh, idx);
            HIP_TRY(hipGetLastError());
            const dim3 rec_grid((unsigned)grid_for((int64_t)L * m, FW_BLOCK, FP_GRID_MAX));
            size_t tmp = fq.ft_tmp.capacity();
            HIP_TRY(rocprim::radix_sort_pairs(fq.ft_tmp.get(), tmp, kt, st, idx, sv, (size_t)L, 0u, 32u, e->stream));
            hipLaunchKernelGGL(k_ft_tails, rec_grid, block, 0, e->stream, head, g, st, sv, ep.ins.get(), L, p, r, gw, m, fq.ft_c.get(), ls,
                               from_records ? 1 : 0, d_fix);
            tmp = fq.ft_tmp.capacity();
            HIP_TRY(rocprim::radix_sort_pairs(fq.ft_tmp.get(), tmp, kh, sh, idx, sv, (size_t)L, 0u, 32u, e->stream)); // (sv of step T is done with)
            hipLaunchKernelGGL(k_ft_heads, rec_grid, block, 0, e->stream, head, g, sh, sv, ep.ins.get(), L, r, gw, m, fq.ft_c.get(), ls,
                               from_records ? 1 : 0, d_fix);
        }
        if (int rc2 = DeviceTime{e}.record(3)) return rc2;
        if (mode != FT_CREATE && !from_records) hipLaunchKernelGGL(k_ft_scan, thread_grid, block, 0, e->stream, head, g, eps, r, gw, m, ls);
        HIP_TRY(hipGetLastError());
        while (k < max_rounds) {
            const int end = fp_chunk_end(k, max_rounds, chunk);
            for (++k; k <= end; ++k) {
                const int b = k & 1;
                hipLaunchKernelGGL(k_fp_select<true>, thread_grid, block, 0, e->stream, head, g, eps, p, r, y[b], y[b ^ 1], gw, m, ls, b);
                hipLaunchKernelGGL(k_fp_mark, mark_grid, block, 0, e->stream, head, g, ep.out_col.get(), ls, b, piece, fq.items.get(), icap, longs, lcap);
                by_fw_shape(PP, levels, [&](auto pp_c, auto lv_c) -> int {
                    constexpr int P = decltype(pp_c)::value, LV = decltype(lv_c)::value;
                    hipLaunchKernelGGL((k_fp_gather<P, LV>), rows_grid, block, 0, e->stream, head, g, y[b], r, gw, m, T, piece, ls, b);
                    hipLaunchKernelGGL((k_fw_pieces<P, LV>), piece_grid, block, 0, e->stream, g, y[b], gw, m, T, piece, &head->fw, fq.items.get(), icap,
                                       fq.pp.get());
                    return DPPR_OK;
                });
                hipLaunchKernelGGL(k_fp_long, long_grid, block, 0, e->stream, head, r, gw, m, piece, longs, lcap, fq.pp.get());
            }
            k = end;
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(fq.fp_pin.get() + offsetof(FpHead, last_act), reinterpret_cast<unsigned char *>(head) + offsetof(FpHead, last_act),
                                   sizeof(unsigned), hipMemcpyDeviceToHost, e->stream)); // THE word of the chunk
            HIP_TRY(loop_wait(e));
            if (!pin->last_act) break; // (no column pushed: every later round is empty)
        }
        hipLaunchKernelGGL(k_fp_left<true>, thread_grid, block, 0, e->stream, head, g, eps, r, gw, m, ls, k & 1);
        HIP_TRY(hipGetLastError());
        if (int rc2 = DeviceTime{e}.record(4)) return rc2;
    }
    if (mode == FT_CREATE) { // the seeds without a row: p = 0.15 w, in the planes where the seed has an id, else in the ext plane below
        HIP_TRY(hipMemcpyAsync(h_seeds, seeds, sizeof(FpSeed) * (size_t)n_seeds, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        for (int j = 0; j < n_seeds; ++j) {
            if (h_seeds[j].row >= 0) continue;
            const int row = e->ext2int[(size_t)h_seeds[j].id];
            if (row >= 0)
                hipLaunchKernelGGL(k_fp_poke<double>, dim3(1), dim3(WAVE), 0, e->stream, p, (long long)row * gw + h_seeds[j].col, fp_rowless_p(h_seeds[j].w));
        }
    }
    if (rounds) {
        // back to the ext planes; |r| into y[0] (the rounds are over), folded by external id as dppr_forward_push folds r
        hipLaunchKernelGGL(k_ft_store, copy_grid, block, 0, e->stream, p, r, x2i, V, gw, sp, sr, y[0]);
        if (mode == FT_CREATE)
            for (int j = 0; j < n_seeds; ++j)
                if (h_seeds[j].row < 0 && e->ext2int[(size_t)h_seeds[j].id] < 0)
                    hipLaunchKernelGGL(k_fp_poke<double>, dim3(1), dim3(WAVE), 0, e->stream, sp, (long long)h_seeds[j].id * gw + h_seeds[j].col,
                                       fp_rowless_p(h_seeds[j].w));
        hipLaunchKernelGGL(k_fw_rem, dim3((unsigned)fw_rem_grid(V)), block, dot_lds_bytes(gw, 1), e->stream, y[0], gw, m, x2i, V, fq.part.get(), stride);
        hipLaunchKernelGGL(k_dot_combine, dim3((m + DOT_CB_WAVES - 1) / DOT_CB_WAVES), dim3(DOT_CB_WAVES * WAVE), 0, e->stream, fq.part.get(),
                           (const long long *)nullptr, stride, m, m, &head->fw.dot, head->rem);
        HIP_TRY(hipGetLastError());
    }
    if (int rc2 = DeviceTime{e}.close()) return rc2;
    HIP_TRY(hipMemcpyAsync(fq.fp_pin, head, sizeof(FpHead) + 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
    if (int rc2 = run_end(e)) return rc2;
    if (e->profiling && rounds) {
        const int cut[5] = {0, 2, 3, 4, 1};
        for (int i = 0; i < 4; ++i) HIP_TRY(hipEventElapsedTime(&e->ft_ms[i], e->evpool[cut[i]], e->evpool[cut[i + 1]]));
    }
    const float call_ms = e->query_ms;
    if (pin->overflow || pin->fw.overflow) return fail(e, DPPR_ERR_HIP, "ftrack: a list was too short (fp_list_cap, fp_mark_cap, fw_item_cap)");
    if (rounds) { // the call has succeeded: the track moves
        const FpHead hd = *pin;
        bool all = true;
        for (int c = 0; c < m; ++c) {
            tk.rounds_used[c] = hd.rounds_used[c];
            tk.pushes[c] = (long long)hd.pushes[c];
            tk.left[c] = (long long)hd.left[c];
            tk.rem[c] = hd.rem[c];
            all = all && hd.left[c] == 0;
        }
        for (int i = 0; i < 3; ++i) tk.work[i] = (long long)hd.work[i];
        tk.fix[0] = L;
        tk.fix[1] = (long long)pin_fix[1];
        tk.fix[2] = (long long)pin_fix[2];
        tk.converged = all;
        tk.epoch = ep.id;
    }
    ftrack_meta_out(tk, out);
    // the seeds that have no id even now: no row of the planes holds them; the host answers p = 0.15 w (r = +0.0), as the push does
    struct Rowless { int id, col; double p; };
    std::vector<Rowless> rowless;
    if (which & (FP_DENSE | FP_AT | FP_TOPK))
        for (int c = 0; c < m; ++c)
            for (int64_t j = tk.offsets[(size_t)c]; j < tk.offsets[(size_t)c + 1]; ++j)
                if (e->ext2int[(size_t)tk.ids[(size_t)j]] < 0) rowless.push_back({tk.ids[(size_t)j], c, fp_rowless_p(tk.weights[(size_t)j])});
    if (which & FP_DENSE) {
        const bool sm = out.dense_layout == DPPR_SOURCE_MAJOR;
        const dim3 grid(sm ? std::min((int)ex_tiles(V), 2048) : grid_for((int64_t)V * m, EX_TILE));
        by_dtype_layout(out.dense_dtype, sm, [&](auto elem, auto source_major) -> int {
            using E = decltype(elem);
            if (out.dense_p_dev) {
                hipLaunchKernelGGL((k_ex_dense<E, decltype(source_major)::value>), grid, dim3(EX_TILE), 0, e->stream, p, gw, m, x2i, V,
                                   static_cast<E *>(out.dense_p_dev));
                for (const Rowless &s : rowless)
                    hipLaunchKernelGGL(k_fp_poke<E>, dim3(1), dim3(WAVE), 0, e->stream, static_cast<E *>(out.dense_p_dev),
                                       (long long)ex_dense_index(out.dense_layout, m, V, s.id, s.col), s.p);
            }
            if (out.dense_r_dev)
                hipLaunchKernelGGL((k_ex_dense<E, decltype(source_major)::value>), grid, dim3(EX_TILE), 0, e->stream, r, gw, m, x2i, V,
                                   static_cast<E *>(out.dense_r_dev));
            return DPPR_OK;
        });
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(e->stream)); // (the destinations are complete here: any stream of the caller may read them)
    }
    if (which & FP_AT) {
        const int n_at = out.n_at;
        std::vector<double> spare(out.at_p && out.at_r ? 0 : (size_t)n_at * m);
        double *at_p = out.at_p ? out.at_p : spare.data(), *at_r = out.at_r ? out.at_r : spare.data();
        if (int rc2 = point_read(e, grow, out.at_ids, n_at, m, 2, at_p, at_r, [&](const int *d_ids, double *d_a, double *d_b) {
                hipLaunchKernelGGL(k_read_at, dim3(grid_for((int64_t)n_at * m)), dim3(BLOCK), 0, e->stream, p, r, gw, m, x2i, d_ids, n_at, d_a, d_b);
                return DPPR_OK;
            }))
            return rc2;
        if (out.at_p)
            for (const Rowless &s : rowless)
                for (int j = 0; j < n_at; ++j)
                    if (out.at_ids[j] == s.id) out.at_p[(size_t)j * m + s.col] = s.p;
    }
    if (which & FP_TOPK) {
        const TkState st = tk_state(e, p, p, gw, m);
        if (int rc2 = run_select(e, st, e->d_int2ext, out.k, out.min_p, out.topk_ids, out.topk_p, nullptr, out.topk_counts)) return rc2;
        for (const Rowless &s : rowless)
            out.topk_counts[s.col] = fp_topk_insert(out.topk_ids + (size_t)s.col * out.k, out.topk_p + (size_t)s.col * out.k, out.topk_counts[s.col],
                                                    out.k, out.min_p, s.id, s.p);
    }
    if (e->profiling) e->query_ms = call_ms; // (the parts opened brackets of their own)
    return DPPR_OK;
}

// the checks of a call's outputs that dppr_forward_push makes, before any device work
int ftrack_out_check(dppr_engine *e, const dppr_ftrack_out_t *out, int m, const char *what) {
    if (!out) return DPPR_OK;
    if (!ft_parts_ok(out))
        return fail(e, DPPR_ERR_INVALID,
                    (std::string(what) + ": a part asked for needs its pointers; k in [1, DPPR_TOPK_MAX], min_p >= 0; n_at in [1, DPPR_FORWARD_AT_MAX]; dtype 0 or 1, layout 0 or 1").c_str());
    if ((ft_which(out) & FP_AT) && !dppr::ids_in_range(out->at_ids, out->n_at, e->V))
        return fail(e, DPPR_ERR_INVALID, (std::string(what) + ": at_ids in [0, V)").c_str());
    HIP_TRY(hipSetDevice(e->device));
    for (void *dst : {out->dense_p_dev, out->dense_r_dev})
        if (dst && !dev_range_ok(e, dst, ex_dense_bytes(out->dense_dtype, m, e->V), ex_elem_bytes(out->dense_dtype)))
            return fail(e, DPPR_ERR_INVALID,
                        (std::string(what) + ": a dense destination must be aligned device memory of the engine's device, m x V elements inside one allocation").c_str());
    return DPPR_OK;
}

FTrack *find_ftrack(dppr_engine *e, int32_t track) { return ft_handle_ok(track) && e->ftracks[track].used ? &e->ftracks[track] : nullptr; }

int ftrack_create_call(dppr_engine *e, int32_t epoch, const int64_t *offsets, const int32_t *ids, const double *weights, int32_t m, double eps,
                       int32_t max_rounds, const dppr_ftrack_out_t *out, int32_t *out_track) {
    if (!out_track || !ft_create_args_ok(m, eps, max_rounds))
        return fail(e, DPPR_ERR_INVALID, "ftrack_create: m in [1, 16], eps > 0 and finite, max_rounds in [1, 256], non-null out_track");
    if (TgCheck c = fp_csr_check(offsets, ids, weights, m, e->V)) return fail(e, DPPR_ERR_INVALID, (std::string("ftrack_create: ") + tg_check_text(c)).c_str());
    if (int rc = ftrack_out_check(e, out, m, "ftrack_create")) return rc;
    const Epoch *ep = find_epoch(e, epoch);
    if (!ep) return fail(e, DPPR_ERR_INVALID, "ftrack_create: epoch not resident (evicted or never built)");
    int slot = -1;
    for (int i = 0; i < FT_MAX && slot < 0; ++i)
        if (!e->ftracks[i].used) slot = i;
    if (slot < 0) return fail(e, DPPR_ERR_INVALID, "ftrack_create: DPPR_FTRACK_MAX tracks exist");
    HIP_TRY(hipSetDevice(e->device));
    std::lock_guard<std::mutex> map_lk(e->map_mu); // (as dppr_read: one state of the id space for the whole call)
    FTrack &tk = e->ftracks[slot];
    tk = FTrack();
    tk.m = m;
    tk.gw = fw_row_width(m);
    tk.eps = eps;
    tk.offsets.assign(offsets, offsets + m + 1);
    tk.ids.assign(ids, ids + offsets[m]);
    tk.weights.assign(weights, weights + offsets[m]);
    const size_t elems = ft_state_elems(e->V, tk.gw);
    if (tk.state.alloc(elems) != 0) {
        tk = FTrack();
        return fail(e, DPPR_ERR_NOMEM, "ftrack_create: the track's planes");
    }
    int rc = DPPR_OK;
    if (hipMemsetAsync(tk.state.get(), 0, sizeof(double) * elems, e->stream) != hipSuccess) rc = fail(e, DPPR_ERR_HIP, "ftrack_create: hipMemsetAsync");
    const dppr_ftrack_out_t none{};
    if (!rc) rc = run_ftrack(e, tk, *ep, FT_CREATE, max_rounds, ft_which(out), out ? *out : none);
    if (rc) {
        (void)hipStreamSynchronize(e->stream);
        tk.state.reset();
        tk = FTrack();
        return rc;
    }
    tk.used = true;
    *out_track = slot;
    return DPPR_OK;
}

int ftrack_update_call(dppr_engine *e, int32_t track, int32_t epoch, int32_t max_rounds, const dppr_ftrack_out_t *out) {
    FTrack *tk = find_ftrack(e, track);
    if (!tk) return fail(e, DPPR_ERR_INVALID, "ftrack_update: no such track");
    if (!ft_rounds_ok(max_rounds)) return fail(e, DPPR_ERR_INVALID, "ftrack_update: max_rounds in [1, 256]");
    if (int rc = ftrack_out_check(e, out, tk->m, "ftrack_update")) return rc;
    const Epoch *ep = find_epoch(e, epoch);
    if (!ep) return fail(e, DPPR_ERR_INVALID, "ftrack_update: epoch not resident (evicted or never built)");
    const FtStep step = ft_step(tk->epoch, ep->id);
    if (step == FT_STEP_BAD) return fail(e, DPPR_ERR_INVALID, "ftrack_update: the track takes its own epoch or the next one (create a new track)");
    HIP_TRY(hipSetDevice(e->device));
    std::lock_guard<std::mutex> map_lk(e->map_mu);
    const dppr_ftrack_out_t none{};
    return run_ftrack(e, *tk, *ep, step == FT_STEP_NEXT ? FT_ADVANCE : FT_MORE, max_rounds, ft_which(out), out ? *out : none);
}

int ftrack_read_call(dppr_engine *e, int32_t track, const dppr_ftrack_out_t *out) {
    FTrack *tk = find_ftrack(e, track);
    if (!tk) return fail(e, DPPR_ERR_INVALID, "ftrack_read: no such track");
    if (!out) return fail(e, DPPR_ERR_INVALID, "ftrack_read: non-null out");
    if (int rc = ftrack_out_check(e, out, tk->m, "ftrack_read")) return rc;
    const uint32_t which = ft_which(out);
    if (!(which & (FP_DENSE | FP_AT | FP_TOPK))) { // (no device work at all)
        ftrack_meta_out(*tk, *out);
        return DPPR_OK;
    }
    // the planes are loaded over the rows of ANY resident epoch: a read walks no edge
    const Epoch *ep = find_epoch(e, -1);
    if (!ep) return fail(e, DPPR_ERR_INVALID, "ftrack_read: no epoch is resident");
    HIP_TRY(hipSetDevice(e->device));
    std::lock_guard<std::mutex> map_lk(e->map_mu);
    return run_ftrack(e, *tk, *ep, FT_READ, 1, which, *out);
}

} // namespace
