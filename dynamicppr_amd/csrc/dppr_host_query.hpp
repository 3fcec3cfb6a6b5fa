// dppr_host_query.hpp -- host side of the state queries (dppr_topk / dppr_group_topk / dppr_read_at / dppr_group_read_at, and
// dppr_group_topk_weighted / dppr_group_score_at, dppr_mark / dppr_changes, dppr_support / dppr_export_sparse /
// dppr_export_dense_dev and their group forms, dppr_dot_dense_dev / dppr_dot_sparse and theirs, dppr_walks / dppr_refine_at /
// dppr_group_refine_at): workspace, the device copy of int2ext, the check of a caller's device pointer and
// the launch sequences of dppr_topk.hpp, dppr_wquery.hpp, dppr_changes.hpp, dppr_export.hpp, dppr_dot.hpp and dppr_walk.hpp. Called with map_mu held, on the solver
// stream; nothing here is reached from the update path.
#pragma once

namespace {

constexpr size_t TK_RES_IDS = 64; // byte offset of the ids in a result block (the 16 counts come first)

size_t tk_res_bytes(int n, int k, bool with_r) {
    const size_t nk = (size_t)n * (size_t)k;
    return TK_RES_IDS + ((sizeof(int) * nk + 7) & ~(size_t)7) + sizeof(double) * nk * (with_r ? 2 : 1);
}

// int2ext on the device, for the tie order (ids are compared in external numbering). Only the occupied zones are copied.
int sync_int2ext(dppr_engine *e) {
    const unsigned gen = e->map_gen.load(std::memory_order_acquire);
    if (e->d_int2ext && gen == e->i2e_gen_on_device) return DPPR_OK;
    if (!e->d_int2ext) HIP_TRY(e->d_int2ext.alloc((size_t)e->V));
    if (e->n_int > 0)
        HIP_TRY(hipMemcpyAsync(e->d_int2ext, e->int2ext.data(), sizeof(int) * (size_t)e->n_int, hipMemcpyHostToDevice, e->stream));
    if (e->n_parked > 0) {
        const size_t lo = (size_t)(e->V - e->n_parked);
        HIP_TRY(hipMemcpyAsync(e->d_int2ext + lo, e->int2ext.data() + lo, sizeof(int) * (size_t)e->n_parked, hipMemcpyHostToDevice,
                               e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream)); // (the host map may change once map_mu is released)
    e->i2e_gen_on_device = gen;
    return DPPR_OK;
}

int topk_workspace(dppr_engine *e, int n, size_t rows) {
    if (!e->tk_pin) { // (the last of the set: one that failed half way is made again)
        HIP_TRY(e->tk_ws.regrow(sizeof(unsigned) * GS_MAX * (TK_BINS1 + TK_BINS2) + sizeof(TkLane) * GS_MAX));
        HIP_TRY(e->tk_out_key.regrow((size_t)GS_MAX * DPPR_TOPK_MAX));
        HIP_TRY(e->tk_out_row.regrow((size_t)GS_MAX * DPPR_TOPK_MAX));
        HIP_TRY(e->tk_res.regrow(tk_res_bytes(GS_MAX, DPPR_TOPK_MAX, true)));
        HIP_TRY(e->tk_pin.regrow(tk_res_bytes(GS_MAX, DPPR_TOPK_MAX, true)));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_tk_hist1), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(sizeof(unsigned) * GS_MAX * TK_BINS1)));
    }
    // a candidate list can hold every occupied row of its lane (the boundary bin of a state whose values crowd one exponent)
    const size_t need = (size_t)n * std::max<size_t>(rows, 1);
    if (e->tk_cand.capacity() < need) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(e->tk_cand.regrow(std::min<size_t>((size_t)GS_MAX * (size_t)e->V, need + need / 4)));
    }
    return DPPR_OK;
}

// The kernels of one selection of dppr_topk.hpp over a state whose workspace is in place (topk_workspace), enqueued. i2e: the
// external id of every row of `st`. Ordered counts, ids, p and r of all lanes, lane-major [n][k], go where the four res_ pointers say.
int select_enqueue(dppr_engine *e, const TkState &st, const int *i2e, int k, double min_p, int *res_cnt, int *res_id, double *res_p,
                   double *res_r) {
    const int n = st.n;
    unsigned *hist1 = reinterpret_cast<unsigned *>(e->tk_ws.get()), *hist2 = hist1 + GS_MAX * TK_BINS1;
    TkLane *ctl = reinterpret_cast<TkLane *>(hist2 + GS_MAX * TK_BINS2);
    const int cand_cap = (int)std::max<size_t>(st.rows, 1);
    HIP_TRY(hipMemsetAsync(e->tk_ws, 0, sizeof(unsigned) * GS_MAX * (TK_BINS1 + TK_BINS2) + sizeof(TkLane) * GS_MAX, e->stream));
    const int n_chunks = std::max((st.rows + TK_ROWS - 1) / TK_ROWS, 1);
    const int grid1 = std::min(n_chunks, 512); // (<= 2 workgroups of 1024 threads per CU)
    hipLaunchKernelGGL(k_tk_hist1, dim3(grid1), dim3(TK_BLOCK), sizeof(unsigned) * n * TK_BINS1, e->stream, st, min_p, hist1);
    hipLaunchKernelGGL(k_tk_select1, dim3(n), dim3(256), 0, e->stream, hist1, k, ctl);
    hipLaunchKernelGGL(k_tk_compact, dim3(grid1), dim3(TK_BLOCK), 0, e->stream, st, min_p, ctl, k, e->tk_out_key, e->tk_out_row,
                       e->tk_cand, cand_cap);
    const int grid2 = std::min(std::max(st.rows / 4096, 1), 64);
    for (int round = 0; round < TK_ROUNDS; ++round) {
        const int s = TK_SHIFT1 - TK_DIGIT * (round + 1);
        hipLaunchKernelGGL(k_tk_hist2, dim3(grid2, n), dim3(256), 0, e->stream, st, i2e, ctl, e->tk_cand, cand_cap, s, hist2);
        hipLaunchKernelGGL(k_tk_select2, dim3(n), dim3(256), 0, e->stream, hist2, s, ctl);
    }
    hipLaunchKernelGGL(k_tk_take, dim3(grid2, n), dim3(256), 0, e->stream, st, i2e, ctl, e->tk_cand, cand_cap, k,
                       e->tk_out_key, e->tk_out_row);
    hipLaunchKernelGGL(k_tk_rank, dim3((k + 255) / 256, n), dim3(256), 0, e->stream, st, i2e, ctl, k, e->tk_out_key,
                       e->tk_out_row, res_cnt, res_id, res_p, res_r);
    HIP_TRY(hipGetLastError());
    return DPPR_OK;
}

// The selection and its copy to the host. With dppr_set_profiling on, the device time from the first to the last kernel is kept
// (query_ms; `opened`: the caller recorded the opening event before kernels of its own).
int run_select(dppr_engine *e, const TkState &st, const int *i2e, int k, double min_p, int32_t *out_ids, double *out_p,
               double *out_r, int32_t *out_counts, bool opened = false) {
    const int n = st.n;
    if (e->profiling && !opened) HIP_TRY(hipEventRecord(e->evpool[0], e->stream));
    const size_t nk = (size_t)n * (size_t)k;
    int *res_cnt = reinterpret_cast<int *>(e->tk_res.get()), *res_id = reinterpret_cast<int *>(e->tk_res.get() + TK_RES_IDS);
    const size_t off_p = TK_RES_IDS + ((sizeof(int) * nk + 7) & ~(size_t)7), off_r = off_p + sizeof(double) * nk;
    double *res_p = reinterpret_cast<double *>(e->tk_res + off_p), *res_r = reinterpret_cast<double *>(e->tk_res + off_r);
    if (int rc = select_enqueue(e, st, i2e, k, min_p, res_cnt, res_id, res_p, res_r)) return rc;
    if (e->profiling) HIP_TRY(hipEventRecord(e->evpool[1], e->stream));
    HIP_TRY(hipMemcpyAsync(e->tk_pin, e->tk_res, tk_res_bytes(n, k, out_r != nullptr), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->profiling) HIP_TRY(hipEventElapsedTime(&e->query_ms, e->evpool[0], e->evpool[1]));
    memcpy(out_counts, e->tk_pin, sizeof(int) * (size_t)n);
    memcpy(out_ids, e->tk_pin + TK_RES_IDS, sizeof(int) * nk);
    memcpy(out_p, e->tk_pin + off_p, sizeof(double) * nk);
    if (out_r) memcpy(out_r, e->tk_pin + off_r, sizeof(double) * nk);
    return DPPR_OK;
}

TkState tk_state(const dppr_engine *e, const double *p, const double *r, int gw, int n) {
    TkState st;
    st.p = p;
    st.r = r;
    st.gw = gw;
    st.n = n;
    st.n_int = e->n_int;
    st.lo_parked = e->V - e->n_parked;
    st.rows = e->n_int + e->n_parked;
    return st;
}

// Top k of every lane of a state (p / r rows gw doubles wide, n lanes). Results are lane-major: [n][k].
int run_topk(dppr_engine *e, const double *p, const double *r, int gw, int n, int k, double min_p, int32_t *out_ids,
             double *out_p, double *out_r, int32_t *out_counts) {
    HIP_TRY(hipSetDevice(e->device));
    const TkState st = tk_state(e, p, r, gw, n);
    int rc = sync_int2ext(e);
    if (rc) return rc;
    rc = topk_workspace(e, n, (size_t)st.rows);
    if (rc) return rc;
    return run_select(e, st, e->d_int2ext, k, min_p, out_ids, out_p, out_r, out_counts);
}

// ---- a group as a weighted set of targets (dppr_wquery.hpp) ---------------------------------------------------------------
// the weights of a call on the device: [q][n] (one small upload; wq_w is in place)
int wq_upload(dppr_engine *e, const double *weights, int q, int n) {
    HIP_TRY(hipMemcpyAsync(e->wq_w, weights, sizeof(double) * (size_t)q * (size_t)n, hipMemcpyHostToDevice, e->stream));
    return DPPR_OK;
}

// Top k of q weighted combinations of a group's lanes (weights [q][n], validated by the caller). Results are query-major: [q][k].
// Every buffer is in place before the first kernel; the scratch state is 8 q + 4 bytes per occupied row.
int run_topk_weighted(dppr_engine *e, const double *p, int gw, int n, const double *weights, int q, int k, double min_score,
                      int32_t *out_ids, double *out_score, int32_t *out_counts) {
    HIP_TRY(hipSetDevice(e->device));
    const TkState st = tk_state(e, p, p, gw, n);
    int rc = sync_int2ext(e);
    if (rc) return rc;
    rc = topk_workspace(e, q, (size_t)st.rows);
    if (rc) return rc;
    const size_t rows = std::max<size_t>((size_t)st.rows, 1);
    if (e->wq_score.capacity() < rows * (size_t)q || e->wq_ext.capacity() < rows) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (e->wq_score.capacity() < rows * (size_t)q) HIP_TRY(e->wq_score.regrow(rows * (size_t)q + rows * (size_t)q / 4));
        if (e->wq_ext.capacity() < rows) HIP_TRY(e->wq_ext.regrow(rows + rows / 4));
    }
    if (!e->wq_w) HIP_TRY(e->wq_w.alloc((size_t)GS_MAX * GS_MAX));
    rc = wq_upload(e, weights, q, n);
    if (rc) return rc;
    if (e->profiling) HIP_TRY(hipEventRecord(e->evpool[0], e->stream));
    const int n_tiles = std::max((st.rows + WQ_ROWS - 1) / WQ_ROWS, 1);
    hipLaunchKernelGGL(k_wq_scores, dim3(std::min(n_tiles, 2048)), dim3(WQ_BLOCK), 0, e->stream, st, e->d_int2ext, e->wq_w, q,
                       e->wq_score, e->wq_ext);
    HIP_TRY(hipGetLastError());
    TkState sc; // the scratch: q lanes, rows q doubles wide, compacted (no parked zone)
    sc.p = sc.r = e->wq_score;
    sc.gw = sc.n = q;
    sc.n_int = sc.lo_parked = sc.rows = st.rows;
    return run_select(e, sc, e->wq_ext, k, min_score, out_ids, out_score, nullptr, out_counts, true);
}

// p / r at m external ids (validated by the caller), [m][n]
int run_read_at(dppr_engine *e, const double *p, const double *r, int gw, int n, const int32_t *ids, int m, double *out_p,
                double *out_r) {
    HIP_TRY(hipSetDevice(e->device));
    int rc = sync_map(e);
    if (rc) return rc;
    const size_t mn = (size_t)m * (size_t)n;
    const size_t ids_bytes = (sizeof(int) * (size_t)m + 7) & ~(size_t)7, need = ids_bytes + 2 * sizeof(double) * mn;
    if (e->ra_buf.capacity() < need) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(e->ra_buf.regrow(need));
    }
    int *d_ids = reinterpret_cast<int *>(e->ra_buf.get());
    double *d_p = reinterpret_cast<double *>(e->ra_buf + ids_bytes), *d_r = d_p + mn;
    HIP_TRY(hipMemcpyAsync(d_ids, ids, sizeof(int) * (size_t)m, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_read_at, dim3(grid_for((int64_t)mn)), dim3(BLOCK), 0, e->stream, p, r, gw, n, e->d_ext2int, d_ids, m,
                       d_p, d_r);
    HIP_TRY(hipGetLastError());
    if (out_p) HIP_TRY(hipMemcpyAsync(out_p, d_p, sizeof(double) * mn, hipMemcpyDeviceToHost, e->stream));
    if (out_r) HIP_TRY(hipMemcpyAsync(out_r, d_r, sizeof(double) * mn, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return DPPR_OK;
}

// scores of q weighted combinations at m external ids (ids and weights validated by the caller, m > 0), [m][q]
int run_score_at(dppr_engine *e, const double *p, int gw, int n, const double *weights, int q, const int32_t *ids, int m,
                 double *out_score) {
    HIP_TRY(hipSetDevice(e->device));
    int rc = sync_map(e);
    if (rc) return rc;
    const size_t mq = (size_t)m * (size_t)q;
    const size_t ids_bytes = (sizeof(int) * (size_t)m + 7) & ~(size_t)7, need = ids_bytes + sizeof(double) * mq;
    if (e->ra_buf.capacity() < need) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(e->ra_buf.regrow(need));
    }
    if (!e->wq_w) HIP_TRY(e->wq_w.alloc((size_t)GS_MAX * GS_MAX));
    rc = wq_upload(e, weights, q, n);
    if (rc) return rc;
    int *d_ids = reinterpret_cast<int *>(e->ra_buf.get());
    double *d_out = reinterpret_cast<double *>(e->ra_buf + ids_bytes);
    HIP_TRY(hipMemcpyAsync(d_ids, ids, sizeof(int) * (size_t)m, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_score_at, dim3(grid_for((int64_t)mq, WQ_BLOCK)), dim3(WQ_BLOCK), 0, e->stream, p, gw, n, e->d_ext2int, d_ids,
                       m, e->wq_w, q, d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_score, d_out, sizeof(double) * mq, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return DPPR_OK;
}

// ---- what a batch moved (dppr_changes.hpp) ---------------------------------------------------------------------------------
static_assert(CH_LANES == GS_MAX && CH_K_MAX == DPPR_TOPK_MAX, "dppr_changes_plan.hpp restates GS_MAX and DPPR_TOPK_MAX");

// mark = p of every source as it is now, by external id ([V][gw]). The buffer is obtained before anything is written; a second
// mark of the same width overwrites the first in place.
int run_mark(dppr_engine *e, const double *p, int gw, DevBuf<double> &mark) {
    HIP_TRY(hipSetDevice(e->device));
    const size_t need = (size_t)e->V * (size_t)gw;
    DevBuf<double> fresh;
    if (mark.capacity() != need) HIP_TRY(fresh.alloc(need));
    int rc = sync_map(e);
    if (rc) return rc;
    if (fresh) mark.swap(fresh); // (what `fresh` holds now goes when this call returns, after the stream has drained)
    hipLaunchKernelGGL(k_ch_mark, dim3(grid_for((int64_t)need, CH_BLOCK)), dim3(CH_BLOCK), 0, e->stream, p, gw, e->d_ext2int.get(), e->V,
                       mark.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    return DPPR_OK;
}

// Top k of |p - mark| of every lane (arguments validated by the caller, the mark exists and is [V][gw]). Results are lane-major:
// [n][k]. Every buffer is in place before the first kernel; the scratch is 16 n + 4 bytes per occupied row; nothing is read back
// between the kernels and one copy brings counts, moved, ids, deltas and p to the host.
int run_changes(dppr_engine *e, const double *p, int gw, int n, double *mark, int k, double min_delta, int remark, int32_t *out_ids,
                double *out_delta, double *out_p, int32_t *out_counts, int32_t *out_moved) {
    HIP_TRY(hipSetDevice(e->device));
    const TkState st = tk_state(e, p, p, gw, n);
    int rc = sync_int2ext(e);
    if (rc) return rc;
    rc = sync_map(e);
    if (rc) return rc;
    rc = topk_workspace(e, n, (size_t)st.rows);
    if (rc) return rc;
    const size_t rows = std::max<size_t>((size_t)st.rows, 1);
    if (e->ch_abs.capacity() < rows * (size_t)n || e->ch_d.capacity() < rows * (size_t)n || e->ch_ext.capacity() < rows) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        const size_t want = rows * (size_t)n + rows * (size_t)n / 4;
        if (e->ch_abs.capacity() < rows * (size_t)n) HIP_TRY(e->ch_abs.regrow(want));
        if (e->ch_d.capacity() < rows * (size_t)n) HIP_TRY(e->ch_d.regrow(want));
        if (e->ch_ext.capacity() < rows) HIP_TRY(e->ch_ext.regrow(rows + rows / 4));
    }
    if (!e->ch_pin) { // (the last of the pair: one that failed half way is made again)
        HIP_TRY(e->ch_res.regrow(ch_layout(GS_MAX, DPPR_TOPK_MAX).total_bytes));
        HIP_TRY(e->ch_pin.regrow(ch_layout(GS_MAX, DPPR_TOPK_MAX).copy_bytes));
    }
    const ChLayout lay = ch_layout(n, k);
    unsigned char *res = e->ch_res.get();
    int *res_cnt = reinterpret_cast<int *>(res + lay.off_cnt), *res_moved = reinterpret_cast<int *>(res + lay.off_moved);
    int *res_id = reinterpret_cast<int *>(res + lay.off_ids);
    double *res_d = reinterpret_cast<double *>(res + lay.off_delta), *res_p = reinterpret_cast<double *>(res + lay.off_p);
    double *res_abs = reinterpret_cast<double *>(res + lay.off_abs);
    if (e->profiling) HIP_TRY(hipEventRecord(e->evpool[0], e->stream));
    HIP_TRY(hipMemsetAsync(res_moved, 0, sizeof(int) * GS_MAX, e->stream));
    const int n_tiles = std::max((st.rows + CH_ROWS - 1) / CH_ROWS, 1);
    hipLaunchKernelGGL(k_ch_delta, dim3(std::min(n_tiles, 2048)), dim3(CH_BLOCK), 0, e->stream, st, e->d_int2ext.get(), mark, e->V,
                       min_delta, remark, e->ch_abs.get(), e->ch_d.get(), e->ch_ext.get(), res_moved);
    HIP_TRY(hipGetLastError());
    TkState sc; // the scratch: n lanes, rows n doubles wide, compacted (no parked zone); p = |d|, r = d
    sc.p = e->ch_abs;
    sc.r = e->ch_d;
    sc.gw = sc.n = n;
    sc.n_int = sc.lo_parked = sc.rows = st.rows;
    rc = select_enqueue(e, sc, e->ch_ext, k, min_delta, res_cnt, res_id, res_abs, res_d);
    if (rc) return rc;
    hipLaunchKernelGGL(k_ch_gather, dim3(grid_for((int64_t)n * k, CH_BLOCK)), dim3(CH_BLOCK), 0, e->stream, p, gw, n, k,
                       e->d_ext2int.get(), res_id, res_p);
    HIP_TRY(hipGetLastError());
    if (e->profiling) HIP_TRY(hipEventRecord(e->evpool[1], e->stream));
    HIP_TRY(hipMemcpyAsync(e->ch_pin, e->ch_res, lay.copy_bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->profiling) HIP_TRY(hipEventElapsedTime(&e->query_ms, e->evpool[0], e->evpool[1]));
    const size_t nk = (size_t)n * (size_t)k;
    memcpy(out_counts, e->ch_pin + lay.off_cnt, sizeof(int) * (size_t)n);
    if (out_moved) memcpy(out_moved, e->ch_pin + lay.off_moved, sizeof(int) * (size_t)n);
    memcpy(out_ids, e->ch_pin + lay.off_ids, sizeof(int) * nk);
    memcpy(out_delta, e->ch_pin + lay.off_delta, sizeof(double) * nk);
    if (out_p) memcpy(out_p, e->ch_pin + lay.off_p, sizeof(double) * nk);
    return DPPR_OK;
}

// ---- the exports (dppr_export.hpp, dppr_export_plan.hpp) --------------------------------------------------------------------
static_assert(EX_LANES == GS_MAX, "dppr_export_plan.hpp restates GS_MAX");
static_assert(EX_DEST_HOST == DPPR_DEST_HOST && EX_DEST_DEVICE == DPPR_DEST_DEVICE && EX_DENSE_P == DPPR_DENSE_P &&
                  EX_DENSE_R == DPPR_DENSE_R && EX_F64 == DPPR_F64 && EX_F32 == DPPR_F32 && EX_VERTEX_MAJOR == DPPR_VERTEX_MAJOR &&
                  EX_SOURCE_MAJOR == DPPR_SOURCE_MAJOR,
              "dppr_export_plan.hpp restates the constants of include/dppr.h");

// A destination in the caller's device memory: device memory of the engine's device, [ptr, ptr + bytes) inside one allocation,
// aligned. Asked of the runtime's tables alone: no device work, and a pointer the runtime does not know is a `false`, not an error.
bool ex_dev_dest_ok(const dppr_engine *e, const void *ptr, size_t bytes, size_t align) {
    if (!ptr || ((uintptr_t)ptr & (uintptr_t)(align - 1))) return false;
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof(a));
    if (hipPointerGetAttributes(&a, ptr) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    if (a.type != hipMemoryTypeDevice || a.device != e->device) return false;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void *>(ptr)) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return ex_range_ok((uintptr_t)ptr, bytes, align, (uintptr_t)base, size);
}

// The three arrays of a sparse export to the device (cap > 0; out_r may be NULL)
bool ex_sparse_dest_ok(const dppr_engine *e, int64_t cap, const int32_t *ids, const double *p, const double *r) {
    return ex_dev_dest_ok(e, ids, sizeof(int32_t) * (size_t)cap, sizeof(int32_t)) &&
           ex_dev_dest_ok(e, p, sizeof(double) * (size_t)cap, sizeof(double)) &&
           (!r || ex_dev_dest_ok(e, r, sizeof(double) * (size_t)cap, sizeof(double)));
}

// workspace by V, the block by what the call copies back: in place before anything is written
int export_workspace(dppr_engine *e, size_t block_bytes) {
    const ExWork w = ex_workspace(e->V);
    if (e->ex_mask.capacity() >= w.mask_elems && e->ex_cnt.capacity() >= w.cnt_elems && e->ex_base.capacity() >= w.base_elems &&
        e->ex_blk.capacity() >= block_bytes && e->ex_pin.capacity() >= block_bytes)
        return DPPR_OK;
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->ex_mask.capacity() < w.mask_elems) HIP_TRY(e->ex_mask.regrow(w.mask_elems));
    if (e->ex_cnt.capacity() < w.cnt_elems) HIP_TRY(e->ex_cnt.regrow(w.cnt_elems));
    if (e->ex_base.capacity() < w.base_elems) HIP_TRY(e->ex_base.regrow(w.base_elems));
    if (e->ex_blk.capacity() < block_bytes) HIP_TRY(e->ex_blk.regrow(block_bytes));
    if (e->ex_pin.capacity() < block_bytes) HIP_TRY(e->ex_pin.regrow(block_bytes));
    return DPPR_OK;
}

// The sparse vectors of every lane of a state (arguments and a device destination validated by the caller). cap = 0: the counts
// alone (dppr_support, the size query). The offsets are decided on the device and so is whether the fill runs: nothing is read
// back between the kernels; one copy brings the head -- and a host destination's ids, p and r -- back.
int run_export_sparse(dppr_engine *e, const double *p, const double *r, int gw, int n, double min_p, int64_t cap, int dest,
                      int64_t *out_offsets, int32_t *out_ids, double *out_p, double *out_r) {
    HIP_TRY(hipSetDevice(e->device));
    int rc = sync_map(e);
    if (rc) return rc;
    const bool host = dest == DPPR_DEST_HOST;
    const int64_t capc = ex_cap_clamped(cap, e->V, n);
    const ExLayout lay = ex_layout(host ? capc : 0, host && out_r);
    rc = export_workspace(e, lay.total_bytes);
    if (rc) return rc;
    unsigned char *blk = e->ex_blk.get();
    ExHead *head = reinterpret_cast<ExHead *>(blk);
    int *d_ids = host ? reinterpret_cast<int *>(blk + lay.off_ids) : out_ids;
    double *d_p = host ? reinterpret_cast<double *>(blk + lay.off_p) : out_p;
    double *d_r = !out_r ? nullptr : host ? reinterpret_cast<double *>(blk + lay.off_r) : out_r;
    const int tiles = (int)ex_tiles(e->V), grid = std::min(tiles, 2048);
    if (e->profiling) HIP_TRY(hipEventRecord(e->evpool[0], e->stream));
    hipLaunchKernelGGL(k_ex_mask, dim3(grid), dim3(EX_TILE), 0, e->stream, p, gw, n, e->d_ext2int.get(), e->V, min_p,
                       e->ex_mask.get(), e->ex_cnt.get());
    hipLaunchKernelGGL(k_ex_scan, dim3(1), dim3(EX_LANES * WAVE), 0, e->stream, e->ex_cnt.get(), n, tiles, (long long)capc,
                       e->ex_base.get(), head);
    if (capc > 0)
        hipLaunchKernelGGL(k_ex_fill, dim3(grid), dim3(EX_TILE), 0, e->stream, p, r, gw, n, e->d_ext2int.get(), e->V,
                           e->ex_mask.get(), e->ex_base.get(), head, d_ids, d_p, d_r);
    HIP_TRY(hipGetLastError());
    if (e->profiling) HIP_TRY(hipEventRecord(e->evpool[1], e->stream));
    HIP_TRY(hipMemcpyAsync(e->ex_pin, e->ex_blk, lay.total_bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream)); // (a device destination is complete here: any stream of the caller may read it)
    if (e->profiling) HIP_TRY(hipEventElapsedTime(&e->query_ms, e->evpool[0], e->evpool[1]));
    const ExHead *h = reinterpret_cast<const ExHead *>(e->ex_pin.get());
    for (int i = 0; i <= n; ++i) out_offsets[i] = h->offsets[i];
    const size_t total = (size_t)h->offsets[n];
    if (host && capc > 0 && h->go && total > 0) {
        memcpy(out_ids, e->ex_pin + lay.off_ids, sizeof(int32_t) * total);
        memcpy(out_p, e->ex_pin + lay.off_p, sizeof(double) * total);
        if (out_r) memcpy(out_r, e->ex_pin + lay.off_r, sizeof(double) * total);
    }
    return DPPR_OK;
}

// p or r of every lane by external id into the caller's device memory (arguments and the destination validated by the caller)
int run_export_dense(dppr_engine *e, const double *src, int gw, int n, int dtype, int layout, void *dst) {
    HIP_TRY(hipSetDevice(e->device));
    int rc = sync_map(e);
    if (rc) return rc;
    const int V = e->V;
    const int *x2i = e->d_ext2int.get();
    if (e->profiling) HIP_TRY(hipEventRecord(e->evpool[0], e->stream));
    if (layout == DPPR_SOURCE_MAJOR) {
        const dim3 grid(std::min((int)ex_tiles(V), 2048)), block(EX_TILE);
        if (dtype == DPPR_F32)
            hipLaunchKernelGGL((k_ex_dense<float, true>), grid, block, 0, e->stream, src, gw, n, x2i, V, static_cast<float *>(dst));
        else
            hipLaunchKernelGGL((k_ex_dense<double, true>), grid, block, 0, e->stream, src, gw, n, x2i, V, static_cast<double *>(dst));
    } else {
        const dim3 grid(grid_for((int64_t)V * n, EX_TILE)), block(EX_TILE);
        if (dtype == DPPR_F32)
            hipLaunchKernelGGL((k_ex_dense<float, false>), grid, block, 0, e->stream, src, gw, n, x2i, V, static_cast<float *>(dst));
        else
            hipLaunchKernelGGL((k_ex_dense<double, false>), grid, block, 0, e->stream, src, gw, n, x2i, V, static_cast<double *>(dst));
    }
    HIP_TRY(hipGetLastError());
    if (e->profiling) HIP_TRY(hipEventRecord(e->evpool[1], e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->profiling) HIP_TRY(hipEventElapsedTime(&e->query_ms, e->evpool[0], e->evpool[1]));
    return DPPR_OK;
}

// What the six entry points share: the checks that need no device and those of a device destination, the id-map lock, the run.
int export_sparse_call(dppr_engine *e, const double *p, const double *r, int gw, int n, double min_p, int64_t cap, int dest,
                       int64_t *out_offsets, int32_t *out_ids, double *out_p, double *out_r) {
    if (!ex_sparse_args_ok(min_p, cap, dest, out_offsets, out_ids, out_p))
        return fail(e, DPPR_ERR_INVALID, "export_sparse: min_p >= 0, cap >= 0, dest 0 or 1, non-null offsets, non-null ids / p when cap > 0");
    HIP_TRY(hipSetDevice(e->device));
    if (cap > 0 && dest == DPPR_DEST_DEVICE && !ex_sparse_dest_ok(e, ex_cap_clamped(cap, e->V, n), out_ids, out_p, out_r))
        return fail(e, DPPR_ERR_INVALID, "export_sparse: ids / p / r must be aligned device memory of the engine's device, cap entries inside one allocation");
    std::lock_guard<std::mutex> map_lk(e->map_mu); // (as dppr_read)
    return run_export_sparse(e, p, r, gw, n, min_p, cap, dest, out_offsets, out_ids, out_p, out_r);
}

int support_call(dppr_engine *e, const double *p, int gw, int n, double min_p, int64_t *out_counts) {
    if (!ex_support_args_ok(min_p, out_counts)) return fail(e, DPPR_ERR_INVALID, "support: min_p >= 0, non-null counts");
    int64_t offsets[GS_MAX + 1];
    int rc;
    {
        std::lock_guard<std::mutex> map_lk(e->map_mu);
        rc = run_export_sparse(e, p, nullptr, gw, n, min_p, 0, DPPR_DEST_HOST, offsets, nullptr, nullptr, nullptr);
    }
    if (rc) return rc;
    for (int i = 0; i < n; ++i) out_counts[i] = offsets[i + 1] - offsets[i];
    return DPPR_OK;
}

int export_dense_call(dppr_engine *e, const double *p, const double *r, int gw, int n, int which, int dtype, int layout, void *dst) {
    if (!ex_dense_args_ok(which, dtype, layout)) return fail(e, DPPR_ERR_INVALID, "export_dense_dev: which 0 or 1, dtype 0 or 1, layout 0 or 1");
    HIP_TRY(hipSetDevice(e->device));
    if (!ex_dev_dest_ok(e, dst, ex_dense_bytes(dtype, n, e->V), ex_elem_bytes(dtype)))
        return fail(e, DPPR_ERR_INVALID, "export_dense_dev: dst must be aligned device memory of the engine's device, n x V elements inside one allocation");
    std::lock_guard<std::mutex> map_lk(e->map_mu);
    return run_export_dense(e, which == DPPR_DENSE_R ? r : p, gw, n, dtype, layout, dst);
}

// ---- the state folded over the vertex axis (dppr_dot.hpp, dppr_dot_plan.hpp) ----------------------------------------------------
static_assert(DOT_LANES == GS_MAX && DOT_MAX_F == DPPR_DOT_MAX_F, "dppr_dot_plan.hpp restates GS_MAX and DPPR_DOT_MAX_F");
static_assert(DOT_DEST_HOST == DPPR_DEST_HOST && DOT_DEST_DEVICE == DPPR_DEST_DEVICE && DOT_P == DPPR_DENSE_P && DOT_R == DPPR_DENSE_R &&
                  DOT_F64 == DPPR_F64 && DOT_F32 == DPPR_F32 && DOT_FEATURE_MAJOR == DPPR_H_FEATURE_MAJOR &&
                  DOT_VERTEX_MAJOR == DPPR_H_VERTEX_MAJOR,
              "dppr_dot_plan.hpp restates the constants of include/dppr.h");

// partials, the device input of a sparse call, the block and its pinned twin: in place before the first kernel
int dot_workspace(dppr_engine *e, size_t part_elems, size_t in_bytes, size_t block_bytes) {
    if (!e->dot_lds_set) { // (the widest dense pass stages more than the 64 KiB a kernel has without asking)
        const int lds = (int)dot_lds_bytes(GS_MAX, DOT_FCHUNK);
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_dot_dense<double, false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_dot_dense<double, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_dot_dense<float, false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_dot_dense<float, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        e->dot_lds_set = true;
    }
    part_elems = std::max<size_t>(part_elems, 1);
    if (e->dot_part.capacity() >= part_elems && e->dot_in.capacity() >= in_bytes && e->dot_blk.capacity() >= block_bytes &&
        e->dot_pin.capacity() >= block_bytes)
        return DPPR_OK;
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->dot_part.capacity() < part_elems) HIP_TRY(e->dot_part.regrow(part_elems));
    if (e->dot_in.capacity() < in_bytes) HIP_TRY(e->dot_in.regrow(in_bytes));
    if (e->dot_blk.capacity() < block_bytes) HIP_TRY(e->dot_blk.regrow(block_bytes));
    if (e->dot_pin.capacity() < block_bytes) HIP_TRY(e->dot_pin.regrow(block_bytes));
    return DPPR_OK;
}

// the end of both runs: one copy brings the head -- and a host destination's results -- back; a raised head is a rejected call
int dot_finish(dppr_engine *e, size_t block_bytes, size_t out_bytes, int dest, double *out) {
    if (e->profiling) HIP_TRY(hipEventRecord(e->evpool[1], e->stream));
    HIP_TRY(hipMemcpyAsync(e->dot_pin, e->dot_blk, block_bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream)); // (a device destination is complete here: any stream of the caller may read it)
    if (e->profiling) HIP_TRY(hipEventElapsedTime(&e->query_ms, e->evpool[0], e->evpool[1]));
    if (reinterpret_cast<const DotHead *>(e->dot_pin.get())->bad) return fail(e, DPPR_ERR_INVALID, "dot_sparse: an id in device memory lies outside [0, V)");
    if (dest == DPPR_DEST_HOST) memcpy(out, e->dot_pin + DOT_HEAD_BYTES, out_bytes);
    return DPPR_OK;
}

// out[f][i] over dense h in the caller's device memory (arguments, h and a device destination validated by the caller)
int run_dot_dense(dppr_engine *e, const double *x, int gw, int n, const void *h, int dtype, int layout, int F, int dest, double *out) {
    HIP_TRY(hipSetDevice(e->device));
    int rc = sync_map(e);
    if (rc) return rc;
    const int V = e->V;
    const size_t blk_bytes = dot_block_bytes(F, n, dest), part_elems = dot_dense_part_elems(V, n, F);
    rc = dot_workspace(e, part_elems, 0, blk_bytes);
    if (rc) return rc;
    DotHead *head = reinterpret_cast<DotHead *>(e->dot_blk.get());
    double *d_out = dest == DPPR_DEST_HOST ? reinterpret_cast<double *>(e->dot_blk + DOT_HEAD_BYTES) : out;
    const long long stride = dot_cols(V);
    const int per_launch = dot_launch_features(V, n, F);
    const int *x2i = e->d_ext2int.get();
    if (e->profiling) HIP_TRY(hipEventRecord(e->evpool[0], e->stream));
    HIP_TRY(hipMemsetAsync(head, 0, DOT_HEAD_BYTES, e->stream));
    HIP_TRY(hipMemsetAsync(e->dot_part, 0, sizeof(double) * part_elems, e->stream)); // (+0.0: the tiles of padding)
    for (int f0 = 0; f0 < F; f0 += per_launch) {
        const int f1 = std::min(F, f0 + per_launch), fcm = std::min(DOT_FCHUNK, f1 - f0);
        const dim3 grid((unsigned)std::min<int64_t>(dot_tiles(V), 2048), (unsigned)((f1 - f0 + DOT_FCHUNK - 1) / DOT_FCHUNK)), block(DOT_TILE);
        const size_t lds = dot_lds_bytes(gw, fcm);
        const bool vm = layout == DPPR_H_VERTEX_MAJOR;
        if (dtype == DPPR_F32) {
            const float *hf = static_cast<const float *>(h);
            if (vm) hipLaunchKernelGGL((k_dot_dense<float, true>), grid, block, lds, e->stream, x, gw, n, x2i, V, hf, F, f0, f1, fcm, e->dot_part.get(), stride);
            else hipLaunchKernelGGL((k_dot_dense<float, false>), grid, block, lds, e->stream, x, gw, n, x2i, V, hf, F, f0, f1, fcm, e->dot_part.get(), stride);
        } else {
            const double *hd = static_cast<const double *>(h);
            if (vm) hipLaunchKernelGGL((k_dot_dense<double, true>), grid, block, lds, e->stream, x, gw, n, x2i, V, hd, F, f0, f1, fcm, e->dot_part.get(), stride);
            else hipLaunchKernelGGL((k_dot_dense<double, false>), grid, block, lds, e->stream, x, gw, n, x2i, V, hd, F, f0, f1, fcm, e->dot_part.get(), stride);
        }
        const int nout = (f1 - f0) * n;
        hipLaunchKernelGGL(k_dot_combine, dim3((nout + DOT_CB_WAVES - 1) / DOT_CB_WAVES), dim3(DOT_CB_WAVES * WAVE), 0, e->stream,
                           e->dot_part.get(), (const long long *)nullptr, stride, nout, n, head, d_out + (size_t)f0 * n);
        HIP_TRY(hipGetLastError());
    }
    return dot_finish(e, blk_bytes, dot_out_bytes(F, n), dest, out);
}

// out[f][i] over the CSR of F queries (arguments, host ids, device ids' / w's range and a device destination validated by the caller)
int run_dot_sparse(dppr_engine *e, const double *x, int gw, int n, const int64_t *offsets, const int32_t *ids, const double *w, int src,
                   int F, int dest, double *out) {
    HIP_TRY(hipSetDevice(e->device));
    int rc = sync_map(e);
    if (rc) return rc;
    const bool host_src = src == DPPR_DEST_HOST;
    const int64_t m = offsets[F];
    dot_tile_table(offsets, F, e->dot_tb);
    const long long n_tiles = (long long)e->dot_tb.tiles.size(), cols = e->dot_tb.cols();
    const DotSparseWork wk = dot_sparse_work(n_tiles, F, m, host_src);
    const size_t blk_bytes = dot_block_bytes(F, n, dest), part_elems = std::max<size_t>((size_t)cols * (size_t)n, 1);
    rc = dot_workspace(e, part_elems, wk.bytes, blk_bytes);
    if (rc) return rc;
    unsigned char *in = e->dot_in.get();
    DotTile *d_tiles = reinterpret_cast<DotTile *>(in);
    long long *d_col = reinterpret_cast<long long *>(in + wk.off_col);
    const int *d_ids = host_src ? reinterpret_cast<const int *>(in + wk.off_ids) : ids;
    const double *d_w = host_src ? reinterpret_cast<const double *>(in + wk.off_w) : w;
    DotHead *head = reinterpret_cast<DotHead *>(e->dot_blk.get());
    double *d_out = dest == DPPR_DEST_HOST ? reinterpret_cast<double *>(e->dot_blk + DOT_HEAD_BYTES) : out;
    if (n_tiles > 0) HIP_TRY(hipMemcpyAsync(d_tiles, e->dot_tb.tiles.data(), sizeof(DotTile) * (size_t)n_tiles, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(d_col, e->dot_tb.col.data(), sizeof(long long) * ((size_t)F + 1), hipMemcpyHostToDevice, e->stream));
    if (host_src && m > 0) {
        HIP_TRY(hipMemcpyAsync(in + wk.off_ids, ids, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(in + wk.off_w, w, sizeof(double) * (size_t)m, hipMemcpyHostToDevice, e->stream));
    }
    if (e->profiling) HIP_TRY(hipEventRecord(e->evpool[0], e->stream));
    HIP_TRY(hipMemsetAsync(head, 0, DOT_HEAD_BYTES, e->stream));
    HIP_TRY(hipMemsetAsync(e->dot_part, 0, sizeof(double) * part_elems, e->stream)); // (+0.0: the tiles of padding)
    if (n_tiles > 0)
        hipLaunchKernelGGL(k_dot_sparse, dim3((unsigned)std::min<long long>(n_tiles, 2048)), dim3(DOT_TILE), dot_lds_bytes(gw, 1), e->stream, x,
                           gw, n, e->d_ext2int.get(), e->V, d_ids, d_w, d_tiles, n_tiles, head, e->dot_part.get(), cols);
    const int nout = F * n;
    hipLaunchKernelGGL(k_dot_combine, dim3((nout + DOT_CB_WAVES - 1) / DOT_CB_WAVES), dim3(DOT_CB_WAVES * WAVE), 0, e->stream,
                       e->dot_part.get(), (const long long *)d_col, cols, nout, n, head, d_out);
    HIP_TRY(hipGetLastError());
    return dot_finish(e, blk_bytes, dot_out_bytes(F, n), dest, out);
}

// What the four entry points share: the checks that need no device, those of the device pointers, the id-map lock, the run.
int dot_dense_call(dppr_engine *e, const double *p, const double *r, int gw, int n, int which, const void *h, int dtype, int layout,
                   int F, int dest, double *out) {
    if (!dot_dense_args_ok(which, h, dtype, layout, F, dest, out))
        return fail(e, DPPR_ERR_INVALID, "dot_dense_dev: which 0 or 1, dtype 0 or 1, h_layout 0 or 1, F in [1, DPPR_DOT_MAX_F], dest 0 or 1, non-null h / out");
    HIP_TRY(hipSetDevice(e->device));
    if (!ex_dev_dest_ok(e, h, dot_dense_h_bytes(dtype, F, e->V), dot_elem_bytes(dtype)))
        return fail(e, DPPR_ERR_INVALID, "dot_dense_dev: h must be aligned device memory of the engine's device, F x V elements inside one allocation");
    if (dest == DPPR_DEST_DEVICE && !ex_dev_dest_ok(e, out, dot_out_bytes(F, n), sizeof(double)))
        return fail(e, DPPR_ERR_INVALID, "dot_dense_dev: out must be aligned device memory of the engine's device, F x n doubles inside one allocation");
    std::lock_guard<std::mutex> map_lk(e->map_mu); // (as dppr_read)
    return run_dot_dense(e, which == DPPR_DENSE_R ? r : p, gw, n, h, dtype, layout, F, dest, out);
}

int dot_sparse_call(dppr_engine *e, const double *p, const double *r, int gw, int n, int which, const int64_t *offsets, const int32_t *ids,
                    const double *w, int src, int F, int dest, double *out) {
    if (!dot_sparse_args_ok(which, offsets, ids, w, src, F, dest, out))
        return fail(e, DPPR_ERR_INVALID, "dot_sparse: which 0 or 1, src 0 or 1, F in [1, DPPR_DOT_MAX_F], dest 0 or 1, non-null ids / w / out, offsets[0] = 0 and non-decreasing");
    HIP_TRY(hipSetDevice(e->device));
    const int64_t m = offsets[F];
    if (src == DPPR_DEST_DEVICE) {
        if (!ex_dev_dest_ok(e, ids, sizeof(int32_t) * (size_t)m, sizeof(int32_t)) || !ex_dev_dest_ok(e, w, sizeof(double) * (size_t)m, sizeof(double)))
            return fail(e, DPPR_ERR_INVALID, "dot_sparse: ids / w must be aligned device memory of the engine's device, offsets[F] entries inside one allocation");
    } else if (!dot_ids_ok(ids, m, e->V)) {
        return fail(e, DPPR_ERR_INVALID, "dot_sparse: ids in [0, V)");
    }
    if (dest == DPPR_DEST_DEVICE && !ex_dev_dest_ok(e, out, dot_out_bytes(F, n), sizeof(double)))
        return fail(e, DPPR_ERR_INVALID, "dot_sparse: out must be aligned device memory of the engine's device, F x n doubles inside one allocation");
    std::lock_guard<std::mutex> map_lk(e->map_mu);
    return run_dot_sparse(e, which == DPPR_DENSE_R ? r : p, gw, n, offsets, ids, w, src, F, dest, out);
}

// ---- forward walks and the refinement of point queries (dppr_walk.hpp, dppr_walk_plan.hpp) ------------------------------------------
static_assert(WALK_MAX_M == DPPR_WALK_MAX_M && WALK_MAX_W == DPPR_WALK_MAX_W && WALK_DEST_HOST == DPPR_DEST_HOST &&
                  WALK_DEST_DEVICE == DPPR_DEST_DEVICE,
              "dppr_walk_plan.hpp restates the constants of include/dppr.h");

// starts, endpoints and the results of a refine call: in place before the first kernel
int walk_workspace(dppr_engine *e, size_t m, size_t ends_elems, size_t res_elems) {
    if (e->wk_starts.capacity() >= m && e->wk_ends.capacity() >= ends_elems && e->wk_res.capacity() >= res_elems) return DPPR_OK;
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->wk_starts.capacity() < m) HIP_TRY(e->wk_starts.regrow(m));
    if (e->wk_ends.capacity() < ends_elems) HIP_TRY(e->wk_ends.regrow(ends_elems));
    if (e->wk_res.capacity() < res_elems) HIP_TRY(e->wk_res.regrow(res_elems));
    return DPPR_OK;
}

// the walk kernel in the engine's form over the m starts in wk_starts (both id maps are on the device)
int walk_enqueue(dppr_engine *e, const Epoch &ep, int m, int W, uint64_t seed, int *d_ends) {
    const long long total = walk_total(m, W), per_wave = walk_per_wave(total);
    const unsigned k0 = (unsigned)(seed & 0xffffffffu), k1 = (unsigned)(seed >> 32);
    if (e->walk_form == 0)
        hipLaunchKernelGGL(k_walk<true>, dim3((unsigned)walk_blocks_refill(total)), dim3(WALK_BLOCK), 0, e->stream, ep.out_row_ptr.get(),
                           ep.out_col.get(), e->d_ext2int.get(), e->d_int2ext.get(), e->wk_starts.get(), (unsigned)W, total, per_wave, k0, k1, d_ends);
    else
        hipLaunchKernelGGL(k_walk<false>, dim3((unsigned)walk_blocks_simple(total)), dim3(WALK_BLOCK), 0, e->stream, ep.out_row_ptr.get(),
                           ep.out_col.get(), e->d_ext2int.get(), e->d_int2ext.get(), e->wk_starts.get(), (unsigned)W, total, per_wave, k0, k1, d_ends);
    HIP_TRY(hipGetLastError());
    return DPPR_OK;
}

// the endpoints of W walks from each of m starts (arguments, ids and a device destination validated by the caller), [m][W]
int run_walks(dppr_engine *e, const Epoch &ep, const int32_t *starts, int m, int W, uint64_t seed, int dest, int32_t *out_ends) {
    HIP_TRY(hipSetDevice(e->device));
    int rc = sync_map(e);
    if (rc) return rc;
    rc = sync_int2ext(e);
    if (rc) return rc;
    const bool host = dest == DPPR_DEST_HOST;
    rc = walk_workspace(e, (size_t)m, host ? (size_t)walk_total(m, W) : 0, 0);
    if (rc) return rc;
    int *d_ends = host ? e->wk_ends.get() : out_ends;
    HIP_TRY(hipMemcpyAsync(e->wk_starts, starts, sizeof(int) * (size_t)m, hipMemcpyHostToDevice, e->stream));
    if (e->profiling) HIP_TRY(hipEventRecord(e->evpool[0], e->stream));
    rc = walk_enqueue(e, ep, m, W, seed, d_ends);
    if (rc) return rc;
    if (e->profiling) HIP_TRY(hipEventRecord(e->evpool[1], e->stream));
    if (host) HIP_TRY(hipMemcpyAsync(out_ends, d_ends, walk_ends_bytes(m, W), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream)); // (a device destination is complete here: any stream of the caller may read it)
    if (e->profiling) HIP_TRY(hipEventElapsedTime(&e->query_ms, e->evpool[0], e->evpool[1]));
    return DPPR_OK;
}

// est / corr / sumsq at m ids, [m][n]: the walks, the fold of r at their endpoints over the pieces of the dot products, the finish
int run_refine(dppr_engine *e, const Epoch &ep, const double *p, const double *r, int gw, int n, const int32_t *ids, int m, int W,
               uint64_t seed, double *out_est, double *out_corr, double *out_sumsq) {
    HIP_TRY(hipSetDevice(e->device));
    int rc = sync_map(e);
    if (rc) return rc;
    rc = sync_int2ext(e);
    if (rc) return rc;
    e->wk_off.resize((size_t)m + 1);
    for (int q = 0; q <= m; ++q) e->wk_off[(size_t)q] = (int64_t)q * W;
    dot_tile_table(e->wk_off.data(), m, e->dot_tb);
    const long long n_tiles = (long long)e->dot_tb.tiles.size(), cols = e->dot_tb.cols();
    const DotSparseWork wk = dot_sparse_work(n_tiles, m, 0, false);
    const size_t mn = (size_t)m * (size_t)n, part_elems = (size_t)cols * 2 * (size_t)n;
    rc = walk_workspace(e, (size_t)m, (size_t)walk_total(m, W), 2 * mn + walk_result_elems(m, n));
    if (rc) return rc;
    rc = dot_workspace(e, part_elems, wk.bytes, DOT_HEAD_BYTES);
    if (rc) return rc;
    unsigned char *in = e->dot_in.get();
    DotTile *d_tiles = reinterpret_cast<DotTile *>(in);
    long long *d_col = reinterpret_cast<long long *>(in + wk.off_col);
    DotHead *head = reinterpret_cast<DotHead *>(e->dot_blk.get());
    double *d_folded = e->wk_res.get(), *d_res = d_folded + 2 * mn;
    HIP_TRY(hipMemcpyAsync(e->wk_starts, ids, sizeof(int) * (size_t)m, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(d_tiles, e->dot_tb.tiles.data(), sizeof(DotTile) * (size_t)n_tiles, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(d_col, e->dot_tb.col.data(), sizeof(long long) * ((size_t)m + 1), hipMemcpyHostToDevice, e->stream));
    if (e->profiling) HIP_TRY(hipEventRecord(e->evpool[0], e->stream));
    rc = walk_enqueue(e, ep, m, W, seed, e->wk_ends.get());
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(head, 0, DOT_HEAD_BYTES, e->stream));
    HIP_TRY(hipMemsetAsync(e->dot_part, 0, sizeof(double) * part_elems, e->stream)); // (+0.0: the tiles of padding)
    hipLaunchKernelGGL(k_walk_fold, dim3((unsigned)std::min<long long>(n_tiles, 2048)), dim3(DOT_TILE), dot_lds_bytes(gw, 1), e->stream, r, gw, n,
                       e->d_ext2int.get(), e->wk_ends.get(), d_tiles, n_tiles, e->dot_part.get(), cols);
    const int nout = m * 2 * n;
    hipLaunchKernelGGL(k_dot_combine, dim3((nout + DOT_CB_WAVES - 1) / DOT_CB_WAVES), dim3(DOT_CB_WAVES * WAVE), 0, e->stream,
                       e->dot_part.get(), (const long long *)d_col, cols, nout, 2 * n, head, d_folded);
    hipLaunchKernelGGL(k_refine_finish, dim3(grid_for((int64_t)mn)), dim3(BLOCK), 0, e->stream, p, gw, n, e->d_ext2int.get(),
                       e->wk_starts.get(), m, W, d_folded, d_res);
    HIP_TRY(hipGetLastError());
    if (e->profiling) HIP_TRY(hipEventRecord(e->evpool[1], e->stream));
    HIP_TRY(hipMemcpyAsync(out_est, d_res, sizeof(double) * mn, hipMemcpyDeviceToHost, e->stream));
    if (out_corr) HIP_TRY(hipMemcpyAsync(out_corr, d_res + mn, sizeof(double) * mn, hipMemcpyDeviceToHost, e->stream));
    if (out_sumsq) HIP_TRY(hipMemcpyAsync(out_sumsq, d_res + 2 * mn, sizeof(double) * mn, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->profiling) HIP_TRY(hipEventElapsedTime(&e->query_ms, e->evpool[0], e->evpool[1]));
    return DPPR_OK;
}

// What the entry points share: the checks that need no device, that of a device destination, the id-map lock, the run.
int walks_call(dppr_engine *e, const Epoch &ep, const int32_t *starts, int32_t m, int32_t W, uint64_t seed, int dest, int32_t *out_ends) {
    if (!walk_args_ok(starts, m, W, dest, out_ends))
        return fail(e, DPPR_ERR_INVALID, "walks: m in [1, DPPR_WALK_MAX_M], W in [1, DPPR_WALK_MAX_W], m * W <= 2^26, dest 0 or 1, non-null starts / out_ends");
    if (!walk_ids_ok(starts, m, e->V)) return fail(e, DPPR_ERR_INVALID, "walks: starts in [0, V)");
    HIP_TRY(hipSetDevice(e->device));
    if (dest == DPPR_DEST_DEVICE && !ex_dev_dest_ok(e, out_ends, walk_ends_bytes(m, W), sizeof(int32_t)))
        return fail(e, DPPR_ERR_INVALID, "walks: out_ends must be aligned device memory of the engine's device, m x W ints inside one allocation");
    std::lock_guard<std::mutex> map_lk(e->map_mu); // (as dppr_read)
    return run_walks(e, ep, starts, m, W, seed, dest, out_ends);
}

int refine_call(dppr_engine *e, const SolveState &st, const Epoch &ep, const double *p, const double *r, int gw, int n, const int32_t *ids,
                int32_t m, int32_t W, uint64_t seed, double *out_est, double *out_corr, double *out_sumsq) {
    if (!refine_args_ok(ids, m, W, out_est))
        return fail(e, DPPR_ERR_INVALID, "refine_at: m in [1, DPPR_WALK_MAX_M], W in [1, DPPR_WALK_MAX_W], m * W <= 2^26, non-null ids / out_est");
    if (!walk_ids_ok(ids, m, e->V)) return fail(e, DPPR_ERR_INVALID, "refine_at: ids in [0, V)");
    if (!st.converged) return fail(e, DPPR_ERR_INVALID, "refine_at: the state is not converged (solve or update it first)");
    if (!refine_epoch_ok(st.last_epoch, ep.id))
        return fail(e, DPPR_ERR_INVALID, "refine_at: the state stands on another epoch than the one given: walks over another graph would give a biased estimate");
    std::lock_guard<std::mutex> map_lk(e->map_mu); // (as dppr_read)
    return run_refine(e, ep, p, r, gw, n, ids, m, W, seed, out_est, out_corr, out_sumsq);
}

} // namespace
