// dppr_host_query.hpp -- host side of the state queries: every dppr_* entry point that reads a state without changing it, from
// dppr_topk to dppr_group_rank_score_at. Nothing here is reached from the update path. A state reaches a query as a StateView
// (dppr_host_state.hpp); a family has a run_* (the launch sequence of its kernel header, called with map_mu held, on the solver
// stream) and a *_call (the checks that need no device, those of the caller's device pointers, map_mu, the run). Shared, each
// written once: query_begin (the device, the id maps), Grow / with_slack (room in a buffer before anything is written), DeviceTime
// (the bracket around a call's kernels), run_end and fetch_block (the end of a run), dev_range_ok (a caller's device pointer),
// topk_workspace / select_enqueue / run_select (the selection over a state or a scratch state), scratch_workspace (the one scratch
// state of the weighted, changes and ranked queries), point_read (read_at, score_at, rank_score_at), cl_graph / order_workspace /
// order_enqueue (the top-k order and its rank table: the opening of cluster and subgraph).
#pragma once

namespace {

static_assert(Q_LANES == GS_MAX, "dppr_query_plan.hpp restates GS_MAX");

// ---- what the families share ------------------------------------------------------------------------------------------------
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

// The opening of a run: the engine's device, and the device copies of the id maps its kernels read brought up to date
enum : unsigned { MAP_E2I = 1, MAP_I2E = 2 };
int query_begin(dppr_engine *e, unsigned maps) {
    HIP_TRY(hipSetDevice(e->device));
    if (maps & MAP_E2I)
        if (int rc = sync_map(e)) return rc;
    if (maps & MAP_I2E)
        if (int rc = sync_int2ext(e)) return rc;
    return DPPR_OK;
}

// Room in a buffer before anything is written: one that holds fewer than `need` elements is released and made again with `want`.
// A release waits for the device, so the solver stream is drained first: once per call (a Grow lives for one), whatever grows.
struct Grow {
    dppr_engine *e;
    bool drained = false;
    template <class B> int operator()(B &buf, size_t need, size_t want) {
        if (buf.capacity() >= need) return DPPR_OK;
        if (!drained) HIP_TRY(hipStreamSynchronize(e->stream));
        drained = true;
        HIP_TRY(buf.regrow(want));
        return DPPR_OK;
    }
    template <class B> int operator()(B &buf, size_t need) { return (*this)(buf, need, need); }
};
constexpr size_t with_slack(size_t need) { return need + need / 4; } // the scratch that follows the occupied rows grows a quarter ahead

// The device time of a call, first to last kernel (dppr_set_profiling; query_ms): opened by whoever launches the first kernel,
// closed before the copy back, read after the synchronisation that follows
struct DeviceTime {
    dppr_engine *e;
    int record(int i) {
        if (e->profiling) HIP_TRY(hipEventRecord(e->evpool[i], e->stream));
        return DPPR_OK;
    }
    int open() { return record(0); }
    int close() { return record(1); }
    int read() {
        if (e->profiling) HIP_TRY(hipEventElapsedTime(&e->query_ms, e->evpool[0], e->evpool[1]));
        return DPPR_OK;
    }
};

// The end of every run, after the bracket has closed and the copies back are enqueued: the wait, then the bracket's reading
int run_end(dppr_engine *e) {
    HIP_TRY(hipStreamSynchronize(e->stream));
    return DeviceTime{e}.read();
}
// ... of a run whose results come back in a block: the bracket closes, one copy takes `bytes` of the block to its pinned twin
int fetch_block(dppr_engine *e, const DevBuf<unsigned char> &blk, PinBuf<unsigned char> &pin, size_t bytes) {
    if (int rc = DeviceTime{e}.close()) return rc;
    HIP_TRY(hipMemcpyAsync(pin, blk, bytes, hipMemcpyDeviceToHost, e->stream));
    return run_end(e);
}

// One of the four instantiations of a kernel template <T, bool> by a call's dtype and layout flag: f(T(), std::bool_constant<flag>())
template <class F> int by_dtype_layout(int dtype, bool flag, F &&f) {
    if (dtype == DPPR_F32) return flag ? f(float(), std::true_type()) : f(float(), std::false_type());
    return flag ? f(double(), std::true_type()) : f(double(), std::false_type());
}

// A caller's pointer into device memory: device memory of the engine's device, [ptr, ptr + bytes) inside one allocation, aligned.
// Asked of the runtime's tables alone: no device work, and a pointer the runtime does not know is a `false`, not an error.
bool dev_range_ok(const dppr_engine *e, const void *ptr, size_t bytes, size_t align) {
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

// ---- top k and point reads (dppr_topk.hpp) -------------------------------------------------------------------------------------
int topk_workspace(dppr_engine *e, Grow &grow, int n, size_t rows) {
    QueryWork::TopK &tk = e->q.tk;
    if (!tk.pin) { // (the last of the set: one that failed half way is made again)
        HIP_TRY(tk.ws.regrow(sizeof(unsigned) * GS_MAX * (TK_BINS1 + TK_BINS2) + sizeof(TkLane) * GS_MAX));
        HIP_TRY(tk.out_key.regrow((size_t)GS_MAX * DPPR_TOPK_MAX));
        HIP_TRY(tk.out_row.regrow((size_t)GS_MAX * DPPR_TOPK_MAX));
        HIP_TRY(tk.res.regrow(tk_layout(GS_MAX, DPPR_TOPK_MAX, true).total_bytes));
        HIP_TRY(tk.pin.regrow(tk_layout(GS_MAX, DPPR_TOPK_MAX, true).total_bytes));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_tk_hist1), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(sizeof(unsigned) * GS_MAX * TK_BINS1)));
    }
    // a candidate list can hold every occupied row of its lane (the boundary bin of a state whose values crowd one exponent)
    const size_t need = (size_t)n * std::max<size_t>(rows, 1);
    return grow(tk.cand, need, std::min<size_t>((size_t)GS_MAX * (size_t)e->V, with_slack(need)));
}

// The kernels of one selection of dppr_topk.hpp over a state whose workspace is in place (topk_workspace), enqueued. i2e: the
// external id of every row of `st`. Ordered counts, ids, p and r of all lanes, lane-major [n][k], go where the four res_ pointers say.
int select_enqueue(dppr_engine *e, const TkState &st, const int *i2e, int k, double min_p, int *res_cnt, int *res_id, double *res_p,
                   double *res_r) {
    QueryWork::TopK &tk = e->q.tk;
    const int n = st.n;
    unsigned *hist1 = reinterpret_cast<unsigned *>(tk.ws.get()), *hist2 = hist1 + GS_MAX * TK_BINS1;
    TkLane *ctl = reinterpret_cast<TkLane *>(hist2 + GS_MAX * TK_BINS2);
    const int cand_cap = (int)std::max<size_t>(st.rows, 1);
    HIP_TRY(hipMemsetAsync(tk.ws, 0, sizeof(unsigned) * GS_MAX * (TK_BINS1 + TK_BINS2) + sizeof(TkLane) * GS_MAX, e->stream));
    const int n_chunks = std::max((st.rows + TK_ROWS - 1) / TK_ROWS, 1);
    const int grid1 = std::min(n_chunks, 512); // (<= 2 workgroups of 1024 threads per CU)
    hipLaunchKernelGGL(k_tk_hist1, dim3(grid1), dim3(TK_BLOCK), sizeof(unsigned) * n * TK_BINS1, e->stream, st, min_p, hist1);
    hipLaunchKernelGGL(k_tk_select1, dim3(n), dim3(256), 0, e->stream, hist1, k, ctl);
    hipLaunchKernelGGL(k_tk_compact, dim3(grid1), dim3(TK_BLOCK), 0, e->stream, st, min_p, ctl, k, tk.out_key, tk.out_row,
                       tk.cand, cand_cap);
    const int grid2 = std::min(std::max(st.rows / 4096, 1), 64);
    for (int round = 0; round < TK_ROUNDS; ++round) {
        const int s = TK_SHIFT1 - TK_DIGIT * (round + 1);
        hipLaunchKernelGGL(k_tk_hist2, dim3(grid2, n), dim3(256), 0, e->stream, st, i2e, ctl, tk.cand, cand_cap, s, hist2);
        hipLaunchKernelGGL(k_tk_select2, dim3(n), dim3(256), 0, e->stream, hist2, s, ctl);
    }
    hipLaunchKernelGGL(k_tk_take, dim3(grid2, n), dim3(256), 0, e->stream, st, i2e, ctl, tk.cand, cand_cap, k, tk.out_key,
                       tk.out_row);
    hipLaunchKernelGGL(k_tk_rank, dim3((k + 255) / 256, n), dim3(256), 0, e->stream, st, i2e, ctl, k, tk.out_key, tk.out_row,
                       res_cnt, res_id, res_p, res_r);
    HIP_TRY(hipGetLastError());
    return DPPR_OK;
}

// The selection and its copy to the host, inside the bracket its caller opened
int run_select(dppr_engine *e, const TkState &st, const int *i2e, int k, double min_p, int32_t *out_ids, double *out_p,
               double *out_r, int32_t *out_counts) {
    QueryWork::TopK &tk = e->q.tk;
    const TkLayout lay = tk_layout(st.n, k, out_r != nullptr);
    unsigned char *res = tk.res.get();
    if (int rc = select_enqueue(e, st, i2e, k, min_p, reinterpret_cast<int *>(res + lay.off_cnt), reinterpret_cast<int *>(res + lay.off_ids),
                                reinterpret_cast<double *>(res + lay.off_p), reinterpret_cast<double *>(res + lay.off_r)))
        return rc;
    if (int rc = fetch_block(e, tk.res, tk.pin, lay.copy_bytes)) return rc;
    const size_t nk = (size_t)st.n * (size_t)k;
    memcpy(out_counts, tk.pin + lay.off_cnt, sizeof(int) * (size_t)st.n);
    memcpy(out_ids, tk.pin + lay.off_ids, sizeof(int) * nk);
    memcpy(out_p, tk.pin + lay.off_p, sizeof(double) * nk);
    if (out_r) memcpy(out_r, tk.pin + lay.off_r, sizeof(double) * nk);
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

// Room for the scratch state of a call and the selection over it: topk_workspace, `planes` (1 or 2) of [rows][lanes] doubles and
// the external id of every row, a quarter ahead
int scratch_workspace(dppr_engine *e, Grow &grow, size_t rows, int lanes, int planes) {
    QueryWork::Scratch &sc = e->q.sc;
    const size_t plane = scratch_plane_elems(rows, lanes), ext = scratch_ext_elems(rows);
    int rc = topk_workspace(e, grow, lanes, rows);
    if (!rc) rc = grow(sc.a, plane, with_slack(plane));
    if (!rc && planes == 2) rc = grow(sc.b, plane, with_slack(plane));
    if (!rc) rc = grow(sc.ext, ext, with_slack(ext));
    return rc;
}
// the grid of a kernel that fills it: one workgroup per tile of dppr_topk.hpp, 2048 at the most
int tile_grid(int rows) { return std::min(std::max((rows + TK_TILE_ROWS - 1) / TK_TILE_ROWS, 1), 2048); }
// ... as the selection reads it: q lanes, rows q doubles wide, compacted (no parked zone)
TkState scratch_state(const double *p, const double *r, int q, int rows) {
    TkState sc;
    sc.p = p;
    sc.r = r;
    sc.gw = sc.n = q;
    sc.n_int = sc.lo_parked = sc.rows = rows;
    return sc;
}

// Top k of every lane of a state (p / r rows gw doubles wide, n lanes). Results are lane-major: [n][k].
int run_topk(dppr_engine *e, const StateView &v, int k, double min_p, int32_t *out_ids, double *out_p, double *out_r,
             int32_t *out_counts) {
    if (int rc = query_begin(e, MAP_I2E)) return rc;
    const TkState st = tk_state(e, v.p, v.r, v.gw, v.n);
    Grow grow{e};
    if (int rc = topk_workspace(e, grow, v.n, (size_t)st.rows)) return rc;
    if (int rc = DeviceTime{e}.open()) return rc;
    return run_select(e, st, e->d_int2ext, k, min_p, out_ids, out_p, out_r, out_counts);
}

int topk_call(dppr_engine *e, const StateView &v, int32_t k, double min_p, int32_t *out_ids, double *out_p, double *out_r,
              int32_t *out_counts) {
    if (!topk_args_ok(k, min_p, out_ids, out_p, out_counts))
        return fail(e, DPPR_ERR_INVALID, v.group ? "topk: k in [1, DPPR_TOPK_MAX], min_p >= 0, non-null ids / p / counts"
                                                 : "topk: k in [1, DPPR_TOPK_MAX], min_p >= 0, non-null ids / p / count");
    std::lock_guard<std::mutex> map_lk(e->map_mu); // (as dppr_read: one state of the id space for the whole query)
    return run_topk(e, v, k, min_p, out_ids, out_p, out_r, out_counts);
}

// The point reads: m external ids (validated by the caller, m > 0) up, `outs` (1 or 2) outputs of [m][cols] doubles written by
// what launch(d_ids, d_a, d_b) enqueues inside the bracket, those the caller wants (out_a / out_b not NULL) back. The caller's
// own buffers are in place before the call.
template <class Launch>
int point_read(dppr_engine *e, Grow &grow, const int32_t *ids, int m, int cols, int outs, double *out_a, double *out_b, Launch &&launch) {
    const size_t bytes = sizeof(double) * (size_t)m * (size_t)cols;
    const RaLayout lay = ra_layout(m, cols, outs);
    if (int rc = grow(e->q.ra.buf, lay.total_bytes)) return rc;
    unsigned char *buf = e->q.ra.buf.get();
    int *d_ids = reinterpret_cast<int *>(buf + lay.off_ids);
    double *d_a = reinterpret_cast<double *>(buf + lay.off_a), *d_b = outs == 2 ? reinterpret_cast<double *>(buf + lay.off_b) : nullptr;
    HIP_TRY(hipMemcpyAsync(d_ids, ids, sizeof(int) * (size_t)m, hipMemcpyHostToDevice, e->stream));
    if (int rc = DeviceTime{e}.open()) return rc;
    if (int rc = launch(d_ids, d_a, d_b)) return rc;
    HIP_TRY(hipGetLastError());
    if (int rc = DeviceTime{e}.close()) return rc;
    if (out_a) HIP_TRY(hipMemcpyAsync(out_a, d_a, bytes, hipMemcpyDeviceToHost, e->stream));
    if (out_b) HIP_TRY(hipMemcpyAsync(out_b, d_b, bytes, hipMemcpyDeviceToHost, e->stream));
    return run_end(e);
}

// p / r at m external ids, [m][n]
int run_read_at(dppr_engine *e, const StateView &v, const int32_t *ids, int m, double *out_p, double *out_r) {
    if (int rc = query_begin(e, MAP_E2I)) return rc;
    Grow grow{e};
    return point_read(e, grow, ids, m, v.n, 2, out_p, out_r, [&](const int *d_ids, double *d_p, double *d_r) {
        hipLaunchKernelGGL(k_read_at, dim3(grid_for((int64_t)m * v.n)), dim3(BLOCK), 0, e->stream, v.p, v.r, v.gw, v.n, e->d_ext2int, d_ids, m, d_p,
                           d_r);
        return DPPR_OK;
    });
}

int read_at_call(dppr_engine *e, const StateView &v, const int32_t *ids, int32_t m, double *out_p, double *out_r) {
    if (!read_at_args_ok(ids, m, e->V)) return fail(e, DPPR_ERR_INVALID, "read_at: ids in [0, V)");
    if (m == 0 || (!out_p && !out_r)) return DPPR_OK;
    std::lock_guard<std::mutex> map_lk(e->map_mu);
    return run_read_at(e, v, ids, m, out_p, out_r);
}

// ---- a group as a weighted set of targets (dppr_wquery.hpp) ---------------------------------------------------------------
// the weights of a call on the device: [q][n] (one small upload)
int wq_upload(dppr_engine *e, const double *weights, int q, int n) {
    if (!e->q.wq.w) HIP_TRY(e->q.wq.w.alloc((size_t)GS_MAX * GS_MAX));
    HIP_TRY(hipMemcpyAsync(e->q.wq.w, weights, sizeof(double) * (size_t)q * (size_t)n, hipMemcpyHostToDevice, e->stream));
    return DPPR_OK;
}

// Top k of q weighted combinations of a group's lanes (weights [q][n], validated by the caller). Results are query-major: [q][k].
// Every buffer is in place before the first kernel; the scratch state is 8 q + 4 bytes per occupied row.
int run_topk_weighted(dppr_engine *e, const StateView &v, const double *weights, int q, int k, double min_score, int32_t *out_ids,
                      double *out_score, int32_t *out_counts) {
    if (int rc = query_begin(e, MAP_I2E)) return rc;
    QueryWork::Scratch &sc = e->q.sc;
    const TkState st = tk_state(e, v.p, v.p, v.gw, v.n);
    Grow grow{e};
    if (int rc = scratch_workspace(e, grow, (size_t)st.rows, q, 1)) return rc;
    if (int rc = wq_upload(e, weights, q, v.n)) return rc;
    if (int rc = DeviceTime{e}.open()) return rc;
    hipLaunchKernelGGL(k_wq_scores, dim3(tile_grid(st.rows)), dim3(TK_TILE_BLOCK), 0, e->stream, st, e->d_int2ext, e->q.wq.w, q, sc.a, sc.ext);
    HIP_TRY(hipGetLastError());
    return run_select(e, scratch_state(sc.a, sc.a, q, st.rows), sc.ext, k, min_score, out_ids, out_score, nullptr, out_counts);
}

// scores of q weighted combinations at m external ids (ids and weights validated by the caller, m > 0), [m][q]
int run_score_at(dppr_engine *e, const StateView &v, const double *weights, int q, const int32_t *ids, int m, double *out_score) {
    if (int rc = query_begin(e, MAP_E2I)) return rc;
    if (int rc = wq_upload(e, weights, q, v.n)) return rc;
    Grow grow{e};
    return point_read(e, grow, ids, m, q, 1, out_score, nullptr, [&](const int *d_ids, double *d_out, double *) {
        hipLaunchKernelGGL(k_score_at, dim3(grid_for((int64_t)m * q, WQ_BLOCK)), dim3(WQ_BLOCK), 0, e->stream, v.p, v.gw, v.n, e->d_ext2int, d_ids,
                           m, e->q.wq.w, q, d_out);
        return DPPR_OK;
    });
}

int topk_weighted_call(dppr_engine *e, const StateView &v, const double *weights, int32_t q, int32_t k, double min_score,
                       int32_t *out_ids, double *out_score, int32_t *out_counts) {
    if (!weights_ok(weights, q, v.n) || !topk_args_ok(k, min_score, out_ids, out_score, out_counts))
        return fail(e, DPPR_ERR_INVALID,
                    "group_topk_weighted: q in [1, 16], finite weights, k in [1, DPPR_TOPK_MAX], min_score >= 0, non-null ids / score / counts");
    std::lock_guard<std::mutex> map_lk(e->map_mu);
    return run_topk_weighted(e, v, weights, q, k, min_score, out_ids, out_score, out_counts);
}

int score_at_call(dppr_engine *e, const StateView &v, const double *weights, int32_t q, const int32_t *ids, int32_t m, double *out_score) {
    if (!weights_ok(weights, q, v.n) || !out_score || !read_at_args_ok(ids, m, e->V))
        return fail(e, DPPR_ERR_INVALID, "group_score_at: q in [1, 16], finite weights, ids in [0, V), non-null score");
    if (m == 0) return DPPR_OK;
    std::lock_guard<std::mutex> map_lk(e->map_mu);
    return run_score_at(e, v, weights, q, ids, m, out_score);
}

// ---- what a batch moved (dppr_changes.hpp, dppr_changes_plan.hpp) ------------------------------------------------------------
// mark = p of every source as it is now, by external id ([V][gw]). The buffer is obtained before anything is written; a second
// mark of the same width overwrites the first in place.
int run_mark(dppr_engine *e, const StateView &v) {
    HIP_TRY(hipSetDevice(e->device));
    const size_t need = (size_t)e->V * (size_t)v.gw;
    DevBuf<double> fresh;
    if (v.mark.capacity() != need) HIP_TRY(fresh.alloc(need));
    if (int rc = query_begin(e, MAP_E2I)) return rc;
    if (fresh) v.mark.swap(fresh); // (what `fresh` holds now goes when this call returns, after the stream has drained)
    hipLaunchKernelGGL(k_ch_mark, dim3(grid_for((int64_t)need, CH_BLOCK)), dim3(CH_BLOCK), 0, e->stream, v.p, v.gw, e->d_ext2int.get(), e->V,
                       v.mark.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    return DPPR_OK;
}

int mark_call(dppr_engine *e, const StateView &v) {
    std::lock_guard<std::mutex> map_lk(e->map_mu);
    return run_mark(e, v);
}

// Top k of |p - mark| of every lane (arguments validated by the caller, the mark exists and is [V][gw]). Results are lane-major:
// [n][k]. Every buffer is in place before the first kernel; the scratch is 16 n + 4 bytes per occupied row; nothing is read back
// between the kernels and one copy brings counts, moved, ids, deltas and p to the host.
int run_changes(dppr_engine *e, const StateView &v, int k, double min_delta, int remark, int32_t *out_ids, double *out_delta,
                double *out_p, int32_t *out_counts, int32_t *out_moved) {
    if (int rc = query_begin(e, MAP_E2I | MAP_I2E)) return rc;
    QueryWork::Changes &ch = e->q.ch;
    QueryWork::Scratch &sc = e->q.sc;
    const int n = v.n;
    const TkState st = tk_state(e, v.p, v.p, v.gw, n);
    Grow grow{e};
    if (int rc = scratch_workspace(e, grow, (size_t)st.rows, n, 2)) return rc;
    if (!ch.pin) { // (the last of the pair: one that failed half way is made again)
        HIP_TRY(ch.res.regrow(ch_layout(GS_MAX, DPPR_TOPK_MAX).total_bytes));
        HIP_TRY(ch.pin.regrow(ch_layout(GS_MAX, DPPR_TOPK_MAX).copy_bytes));
    }
    const ChLayout lay = ch_layout(n, k);
    unsigned char *res = ch.res.get();
    int *res_cnt = reinterpret_cast<int *>(res + lay.off_cnt), *res_moved = reinterpret_cast<int *>(res + lay.off_moved);
    int *res_id = reinterpret_cast<int *>(res + lay.off_ids);
    double *res_d = reinterpret_cast<double *>(res + lay.off_delta), *res_p = reinterpret_cast<double *>(res + lay.off_p);
    double *res_abs = reinterpret_cast<double *>(res + lay.off_abs);
    if (int rc = DeviceTime{e}.open()) return rc;
    HIP_TRY(hipMemsetAsync(res_moved, 0, sizeof(int) * GS_MAX, e->stream));
    hipLaunchKernelGGL(k_ch_delta, dim3(tile_grid(st.rows)), dim3(TK_TILE_BLOCK), 0, e->stream, st, e->d_int2ext.get(), v.mark.get(), e->V,
                       min_delta, remark, sc.a.get(), sc.b.get(), sc.ext.get(), res_moved);
    HIP_TRY(hipGetLastError());
    // (the scratch: p = |d|, r = d)
    if (int rc = select_enqueue(e, scratch_state(sc.a, sc.b, n, st.rows), sc.ext, k, min_delta, res_cnt, res_id, res_abs, res_d)) return rc;
    hipLaunchKernelGGL(k_ch_gather, dim3(grid_for((int64_t)n * k, CH_BLOCK)), dim3(CH_BLOCK), 0, e->stream, v.p, v.gw, n, k,
                       e->d_ext2int.get(), res_id, res_p);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_block(e, ch.res, ch.pin, lay.copy_bytes)) return rc;
    const size_t nk = (size_t)n * (size_t)k;
    memcpy(out_counts, ch.pin + lay.off_cnt, sizeof(int) * (size_t)n);
    if (out_moved) memcpy(out_moved, ch.pin + lay.off_moved, sizeof(int) * (size_t)n);
    memcpy(out_ids, ch.pin + lay.off_ids, sizeof(int) * nk);
    memcpy(out_delta, ch.pin + lay.off_delta, sizeof(double) * nk);
    if (out_p) memcpy(out_p, ch.pin + lay.off_p, sizeof(double) * nk);
    return DPPR_OK;
}

int changes_call(dppr_engine *e, const StateView &v, int32_t k, double min_delta, int remark, int32_t *out_ids, double *out_delta,
                 double *out_p, int32_t *out_counts, int32_t *out_moved) {
    if (!ch_args_ok(k, min_delta, out_ids, out_delta, out_counts))
        return fail(e, DPPR_ERR_INVALID, v.group ? "changes: k in [1, DPPR_TOPK_MAX], min_delta >= 0, non-null ids / delta / counts"
                                                 : "changes: k in [1, DPPR_TOPK_MAX], min_delta >= 0, non-null ids / delta / count");
    if (!v.mark)
        return fail(e, DPPR_ERR_INVALID, v.group ? "changes: the group has no mark (dppr_group_mark; a change of the sources drops it)"
                                                 : "changes: the slot has no mark (dppr_mark)");
    std::lock_guard<std::mutex> map_lk(e->map_mu);
    return run_changes(e, v, k, min_delta, remark, out_ids, out_delta, out_p, out_counts, out_moved);
}

// ---- the exports (dppr_export.hpp, dppr_export_plan.hpp) --------------------------------------------------------------------
// The three arrays of a sparse export to the device (cap > 0; out_r may be NULL)
bool ex_sparse_dest_ok(const dppr_engine *e, int64_t cap, const int32_t *ids, const double *p, const double *r) {
    return dev_range_ok(e, ids, sizeof(int32_t) * (size_t)cap, sizeof(int32_t)) &&
           dev_range_ok(e, p, sizeof(double) * (size_t)cap, sizeof(double)) &&
           (!r || dev_range_ok(e, r, sizeof(double) * (size_t)cap, sizeof(double)));
}

// workspace by V, the block by what the call copies back: in place before anything is written
int export_workspace(dppr_engine *e, size_t block_bytes) {
    QueryWork::Export &ex = e->q.ex;
    const ExWork w = ex_workspace(e->V);
    Grow grow{e};
    int rc = grow(ex.mask, w.mask_elems);
    if (!rc) rc = grow(ex.cnt, w.cnt_elems);
    if (!rc) rc = grow(ex.base, w.base_elems);
    if (!rc) rc = grow(ex.blk, block_bytes);
    if (!rc) rc = grow(ex.pin, block_bytes);
    return rc;
}

// The sparse vectors of every lane of a state (arguments and a device destination validated by the caller). cap = 0: the counts
// alone (dppr_support, the size query). The offsets are decided on the device and so is whether the fill runs: nothing is read
// back between the kernels; one copy brings the head -- and a host destination's ids, p and r -- back.
int run_export_sparse(dppr_engine *e, const StateView &v, double min_p, int64_t cap, int dest, int64_t *out_offsets, int32_t *out_ids,
                      double *out_p, double *out_r) {
    if (int rc = query_begin(e, MAP_E2I)) return rc;
    QueryWork::Export &ex = e->q.ex;
    const int n = v.n;
    const bool host = dest == DPPR_DEST_HOST;
    const int64_t capc = ex_cap_clamped(cap, e->V, n);
    const ExLayout lay = ex_layout(host ? capc : 0, host && out_r);
    if (int rc = export_workspace(e, lay.total_bytes)) return rc;
    unsigned char *blk = ex.blk.get();
    ExHead *head = reinterpret_cast<ExHead *>(blk);
    int *d_ids = host ? reinterpret_cast<int *>(blk + lay.off_ids) : out_ids;
    double *d_p = host ? reinterpret_cast<double *>(blk + lay.off_p) : out_p;
    double *d_r = !out_r ? nullptr : host ? reinterpret_cast<double *>(blk + lay.off_r) : out_r;
    const int tiles = (int)ex_tiles(e->V), grid = std::min(tiles, 2048);
    if (int rc = DeviceTime{e}.open()) return rc;
    hipLaunchKernelGGL(k_ex_mask, dim3(grid), dim3(EX_TILE), 0, e->stream, v.p, v.gw, n, e->d_ext2int.get(), e->V, min_p, ex.mask.get(),
                       ex.cnt.get());
    hipLaunchKernelGGL(k_ex_scan, dim3(1), dim3(EX_LANES * WAVE), 0, e->stream, ex.cnt.get(), n, tiles, (long long)capc, ex.base.get(),
                       head);
    if (capc > 0)
        hipLaunchKernelGGL(k_ex_fill, dim3(grid), dim3(EX_TILE), 0, e->stream, v.p, v.r, v.gw, n, e->d_ext2int.get(), e->V, ex.mask.get(),
                           ex.base.get(), head, d_ids, d_p, d_r);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_block(e, ex.blk, ex.pin, lay.total_bytes)) return rc; // (a device destination is complete here: any stream of the caller may read it)
    const ExHead *h = reinterpret_cast<const ExHead *>(ex.pin.get());
    for (int i = 0; i <= n; ++i) out_offsets[i] = h->offsets[i];
    const size_t total = (size_t)h->offsets[n];
    if (host && capc > 0 && h->go && total > 0) {
        memcpy(out_ids, ex.pin + lay.off_ids, sizeof(int32_t) * total);
        memcpy(out_p, ex.pin + lay.off_p, sizeof(double) * total);
        if (out_r) memcpy(out_r, ex.pin + lay.off_r, sizeof(double) * total);
    }
    return DPPR_OK;
}

// p or r of every lane by external id into the caller's device memory (arguments and the destination validated by the caller)
int run_export_dense(dppr_engine *e, const StateView &v, int which, int dtype, int layout, void *dst) {
    if (int rc = query_begin(e, MAP_E2I)) return rc;
    const int V = e->V;
    const bool sm = layout == DPPR_SOURCE_MAJOR;
    const dim3 grid(sm ? std::min((int)ex_tiles(V), 2048) : grid_for((int64_t)V * v.n, EX_TILE)), block(EX_TILE);
    if (int rc = DeviceTime{e}.open()) return rc;
    by_dtype_layout(dtype, sm, [&](auto elem, auto source_major) -> int {
        using T = decltype(elem);
        hipLaunchKernelGGL((k_ex_dense<T, decltype(source_major)::value>), grid, block, 0, e->stream, which == DPPR_DENSE_R ? v.r : v.p, v.gw,
                           v.n, e->d_ext2int.get(), V, static_cast<T *>(dst));
        return DPPR_OK;
    });
    HIP_TRY(hipGetLastError());
    if (int rc = DeviceTime{e}.close()) return rc;
    return run_end(e);
}

int export_sparse_call(dppr_engine *e, const StateView &v, double min_p, int64_t cap, int dest, int64_t *out_offsets, int32_t *out_ids,
                       double *out_p, double *out_r) {
    if (!ex_sparse_args_ok(min_p, cap, dest, out_offsets, out_ids, out_p))
        return fail(e, DPPR_ERR_INVALID, "export_sparse: min_p >= 0, cap >= 0, dest 0 or 1, non-null offsets, non-null ids / p when cap > 0");
    HIP_TRY(hipSetDevice(e->device));
    if (cap > 0 && dest == DPPR_DEST_DEVICE && !ex_sparse_dest_ok(e, ex_cap_clamped(cap, e->V, v.n), out_ids, out_p, out_r))
        return fail(e, DPPR_ERR_INVALID, "export_sparse: ids / p / r must be aligned device memory of the engine's device, cap entries inside one allocation");
    std::lock_guard<std::mutex> map_lk(e->map_mu); // (as dppr_read)
    return run_export_sparse(e, v, min_p, cap, dest, out_offsets, out_ids, out_p, out_r);
}

int support_call(dppr_engine *e, const StateView &v, double min_p, int64_t *out_counts) {
    if (!ex_support_args_ok(min_p, out_counts)) return fail(e, DPPR_ERR_INVALID, "support: min_p >= 0, non-null counts");
    int64_t offsets[GS_MAX + 1];
    int rc;
    {
        std::lock_guard<std::mutex> map_lk(e->map_mu);
        rc = run_export_sparse(e, v, min_p, 0, DPPR_DEST_HOST, offsets, nullptr, nullptr, nullptr);
    }
    if (rc) return rc;
    for (int i = 0; i < v.n; ++i) out_counts[i] = offsets[i + 1] - offsets[i];
    return DPPR_OK;
}

int export_dense_call(dppr_engine *e, const StateView &v, int which, int dtype, int layout, void *dst) {
    if (!ex_dense_args_ok(which, dtype, layout)) return fail(e, DPPR_ERR_INVALID, "export_dense_dev: which 0 or 1, dtype 0 or 1, layout 0 or 1");
    HIP_TRY(hipSetDevice(e->device));
    if (!dev_range_ok(e, dst, ex_dense_bytes(dtype, v.n, e->V), ex_elem_bytes(dtype)))
        return fail(e, DPPR_ERR_INVALID, "export_dense_dev: dst must be aligned device memory of the engine's device, n x V elements inside one allocation");
    std::lock_guard<std::mutex> map_lk(e->map_mu);
    return run_export_dense(e, v, which, dtype, layout, dst);
}

// ---- the patch feed (dppr_patch.hpp, dppr_patch_plan.hpp) ---------------------------------------------------------------------
// workspace by V, the block by what the call copies back: in place before anything is written
int patch_workspace(dppr_engine *e, size_t block_bytes) {
    QueryWork::Patch &pt = e->q.pt;
    const PtWork w = pt_workspace(e->V);
    Grow grow{e};
    int rc = grow(pt.mask, w.mask_elems);
    if (!rc) rc = grow(pt.cnt, w.cnt_elems);
    if (!rc) rc = grow(pt.base, w.base_elems);
    if (!rc) rc = grow(pt.blk, block_bytes);
    if (!rc) rc = grow(pt.pin, block_bytes);
    return rc;
}

// The patch of every lane of a state against its mark (arguments, the mark and a device destination validated by the caller).
// The offsets are decided on the device and so is whether the fill and the re-mark run: nothing is read back between the kernels;
// one copy brings the head -- and a host destination's ids and p -- back.
int run_patch(dppr_engine *e, const StateView &v, double min_p, double min_delta, int64_t cap_up, int64_t cap_del, int dest, int remark,
              dppr_patch_out_t *out) {
    if (int rc = query_begin(e, MAP_E2I)) return rc;
    QueryWork::Patch &pt = e->q.pt;
    const int n = v.n;
    const bool host = dest == DPPR_DEST_HOST;
    const int64_t cu = ex_cap_clamped(cap_up, e->V, n), cd = ex_cap_clamped(cap_del, e->V, n);
    const PtLayout lay = pt_layout(host ? cu : 0, host ? cd : 0);
    if (int rc = patch_workspace(e, lay.total_bytes)) return rc;
    unsigned char *blk = pt.blk.get();
    PtHead *head = reinterpret_cast<PtHead *>(blk);
    int *d_up_ids = host ? reinterpret_cast<int *>(blk + lay.off_up_ids) : out->up_ids;
    double *d_up_p = host ? reinterpret_cast<double *>(blk + lay.off_up_p) : out->up_p;
    int *d_del_ids = host ? reinterpret_cast<int *>(blk + lay.off_del_ids) : out->del_ids;
    const int tiles = (int)ex_tiles(e->V), grid = std::min(tiles, 2048);
    if (int rc = DeviceTime{e}.open()) return rc;
    hipLaunchKernelGGL(k_pt_classify, dim3(grid), dim3(EX_TILE), 0, e->stream, v.p, v.gw, n, e->d_ext2int.get(), e->V, v.mark.get(), min_p,
                       min_delta, pt.mask.get(), pt.cnt.get());
    hipLaunchKernelGGL(k_pt_scan, dim3(1), dim3(PT_LANES * WAVE), 0, e->stream, pt.cnt.get(), n, tiles, (long long)cu, (long long)cd,
                       pt.base.get(), head);
    if (cu > 0 || cd > 0 || remark != DPPR_PATCH_KEEP_MARK) // (the size query has nothing to fill and nothing to mark)
        hipLaunchKernelGGL(k_pt_fill, dim3(grid), dim3(EX_TILE), 0, e->stream, v.p, v.gw, n, e->d_ext2int.get(), e->V, v.mark.get(),
                           pt.mask.get(), pt.base.get(), head, remark, d_up_ids, d_up_p, d_del_ids);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_block(e, pt.blk, pt.pin, lay.total_bytes)) return rc; // (a device destination is complete here: any stream of the caller may read it)
    const PtHead *h = reinterpret_cast<const PtHead *>(pt.pin.get());
    for (int i = 0; i <= n; ++i) {
        out->up_offsets[i] = h->up_offsets[i];
        out->del_offsets[i] = h->del_offsets[i];
    }
    out->written = h->written;
    if (host && h->go) {
        const size_t ups = (size_t)h->up_offsets[n], dels = (size_t)h->del_offsets[n];
        if (ups > 0) {
            memcpy(out->up_ids, pt.pin + lay.off_up_ids, sizeof(int32_t) * ups);
            memcpy(out->up_p, pt.pin + lay.off_up_p, sizeof(double) * ups);
        }
        if (dels > 0) memcpy(out->del_ids, pt.pin + lay.off_del_ids, sizeof(int32_t) * dels);
    }
    return DPPR_OK;
}

int patch_call(dppr_engine *e, const StateView &v, double min_p, double min_delta, int64_t cap_up, int64_t cap_del, int dest, int remark,
               dppr_patch_out_t *out) {
    if (!pt_args_ok(min_p, min_delta, cap_up, cap_del, dest, remark, out))
        return fail(e, DPPR_ERR_INVALID, "patch: min_p >= 0, min_delta >= 0, caps >= 0, dest 0 or 1, remark 0, 1 or 2, non-null out and offsets, "
                                         "non-null up_ids / up_p when cap_up > 0, non-null del_ids when cap_del > 0");
    if (!v.mark)
        return fail(e, DPPR_ERR_INVALID, v.group ? "patch: the group has no mark (dppr_group_mark; a change of the sources drops it)"
                                                 : "patch: the slot has no mark (dppr_mark)");
    HIP_TRY(hipSetDevice(e->device));
    if (dest == DPPR_DEST_DEVICE) {
        const size_t cu = (size_t)ex_cap_clamped(cap_up, e->V, v.n), cd = (size_t)ex_cap_clamped(cap_del, e->V, v.n);
        const bool up_ok = cap_up == 0 || (dev_range_ok(e, out->up_ids, sizeof(int32_t) * cu, sizeof(int32_t)) &&
                                           dev_range_ok(e, out->up_p, sizeof(double) * cu, sizeof(double)));
        const bool del_ok = cap_del == 0 || dev_range_ok(e, out->del_ids, sizeof(int32_t) * cd, sizeof(int32_t));
        if (!up_ok || !del_ok)
            return fail(e, DPPR_ERR_INVALID, "patch: up_ids / up_p / del_ids must be aligned device memory of the engine's device, cap entries inside one allocation");
    }
    std::lock_guard<std::mutex> map_lk(e->map_mu); // (as dppr_read)
    return run_patch(e, v, min_p, min_delta, cap_up, cap_del, dest, remark, out);
}

// ---- the state folded over the vertex axis (dppr_dot.hpp, dppr_dot_plan.hpp) ----------------------------------------------------
// partials, the device input of a sparse call, the block and its pinned twin: in place before the first kernel
int dot_workspace(dppr_engine *e, Grow &grow, size_t part_elems, size_t in_bytes, size_t block_bytes) {
    QueryWork::Dot &dot = e->q.dot;
    if (!dot.lds_set) { // (the widest dense pass stages more than the 64 KiB a kernel has without asking)
        const int lds = (int)dot_lds_bytes(GS_MAX, DOT_FCHUNK);
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_dot_dense<double, false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_dot_dense<double, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_dot_dense<float, false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_dot_dense<float, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        dot.lds_set = true;
    }
    int rc = grow(dot.part, std::max<size_t>(part_elems, 1));
    if (!rc) rc = grow(dot.in, in_bytes);
    if (!rc) rc = grow(dot.blk, block_bytes);
    if (!rc) rc = grow(dot.pin, block_bytes);
    return rc;
}

// the end of both runs: one copy brings the head -- and a host destination's results -- back; a raised head is a rejected call
int dot_finish(dppr_engine *e, size_t block_bytes, size_t out_bytes, int dest, double *out) {
    QueryWork::Dot &dot = e->q.dot;
    if (int rc = fetch_block(e, dot.blk, dot.pin, block_bytes)) return rc; // (a device destination is complete here: any stream of the caller may read it)
    if (reinterpret_cast<const DotHead *>(dot.pin.get())->bad) return fail(e, DPPR_ERR_INVALID, "dot_sparse: an id in device memory lies outside [0, V)");
    if (dest == DPPR_DEST_HOST) memcpy(out, dot.pin + DOT_HEAD_BYTES, out_bytes);
    return DPPR_OK;
}

// out[f][i] over dense h in the caller's device memory (arguments, h and a device destination validated by the caller)
int run_dot_dense(dppr_engine *e, const StateView &v, int which, const void *h, int dtype, int layout, int F, int dest, double *out) {
    if (int rc = query_begin(e, MAP_E2I)) return rc;
    QueryWork::Dot &dot = e->q.dot;
    const double *x = which == DPPR_DENSE_R ? v.r : v.p;
    const int V = e->V, gw = v.gw, n = v.n;
    const size_t blk_bytes = dot_block_bytes(F, n, dest), part_elems = dot_dense_part_elems(V, n, F);
    Grow grow{e};
    if (int rc = dot_workspace(e, grow, part_elems, 0, blk_bytes)) return rc;
    DotHead *head = reinterpret_cast<DotHead *>(dot.blk.get());
    double *d_out = dest == DPPR_DEST_HOST ? reinterpret_cast<double *>(dot.blk + DOT_HEAD_BYTES) : out;
    const long long stride = dot_cols(V);
    const int per_launch = dot_launch_features(V, n, F);
    const int *x2i = e->d_ext2int.get();
    if (int rc = DeviceTime{e}.open()) return rc;
    HIP_TRY(hipMemsetAsync(head, 0, DOT_HEAD_BYTES, e->stream));
    HIP_TRY(hipMemsetAsync(dot.part, 0, sizeof(double) * part_elems, e->stream)); // (+0.0: the tiles of padding)
    for (int f0 = 0; f0 < F; f0 += per_launch) {
        const int f1 = std::min(F, f0 + per_launch), fcm = std::min(DOT_FCHUNK, f1 - f0);
        const dim3 grid((unsigned)std::min<int64_t>(dot_tiles(V), 2048), (unsigned)((f1 - f0 + DOT_FCHUNK - 1) / DOT_FCHUNK)), block(DOT_TILE);
        const size_t lds = dot_lds_bytes(gw, fcm);
        by_dtype_layout(dtype, layout == DPPR_H_VERTEX_MAJOR, [&](auto elem, auto vertex_major) -> int {
            using T = decltype(elem);
            hipLaunchKernelGGL((k_dot_dense<T, decltype(vertex_major)::value>), grid, block, lds, e->stream, x, gw, n, x2i, V,
                               static_cast<const T *>(h), F, f0, f1, fcm, dot.part.get(), stride);
            return DPPR_OK;
        });
        const int nout = (f1 - f0) * n;
        hipLaunchKernelGGL(k_dot_combine, dim3((nout + DOT_CB_WAVES - 1) / DOT_CB_WAVES), dim3(DOT_CB_WAVES * WAVE), 0, e->stream,
                           dot.part.get(), (const long long *)nullptr, stride, nout, n, head, d_out + (size_t)f0 * n);
        HIP_TRY(hipGetLastError());
    }
    return dot_finish(e, blk_bytes, dot_out_bytes(F, n), dest, out);
}

// What run_dot_sparse and run_refine share: a fold of `lanes` outputs per query over the tile table in q.dot.tb (F queries).
struct Fold {
    DotSparseWork wk;
    long long n_tiles = 0, cols = 0;
    size_t part_elems = 0;
    DotTile *tiles = nullptr;
    long long *col = nullptr;
    DotHead *head = nullptr;
};

// ... its set-up: the partials, the input (the table, and m ids / w of a host source) and the block in place, the table on the device
int fold_setup(dppr_engine *e, Grow &grow, int F, int64_t m, bool host_src, int lanes, size_t blk_bytes, Fold &f) {
    QueryWork::Dot &dot = e->q.dot;
    f.n_tiles = (long long)dot.tb.tiles.size();
    f.cols = dot.tb.cols();
    f.wk = dot_sparse_work(f.n_tiles, F, m, host_src);
    f.part_elems = std::max<size_t>((size_t)f.cols * (size_t)lanes, 1);
    if (int rc = dot_workspace(e, grow, f.part_elems, f.wk.bytes, blk_bytes)) return rc;
    f.tiles = reinterpret_cast<DotTile *>(dot.in.get());
    f.col = reinterpret_cast<long long *>(dot.in + f.wk.off_col);
    f.head = reinterpret_cast<DotHead *>(dot.blk.get());
    if (f.n_tiles > 0) HIP_TRY(hipMemcpyAsync(f.tiles, dot.tb.tiles.data(), sizeof(DotTile) * (size_t)f.n_tiles, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(f.col, dot.tb.col.data(), sizeof(long long) * ((size_t)F + 1), hipMemcpyHostToDevice, e->stream));
    return DPPR_OK;
}

// ... and its finish: head and partials zeroed, the caller's pass over the tiles, the combine into d_out [F][lanes]
template <class Pass> int fold_finish(dppr_engine *e, const Fold &f, int F, int lanes, double *d_out, Pass &&pass) {
    HIP_TRY(hipMemsetAsync(f.head, 0, DOT_HEAD_BYTES, e->stream));
    HIP_TRY(hipMemsetAsync(e->q.dot.part, 0, sizeof(double) * f.part_elems, e->stream)); // (+0.0: the tiles of padding)
    if (f.n_tiles > 0) pass(dim3((unsigned)std::min<long long>(f.n_tiles, 2048)));
    const int nout = F * lanes;
    hipLaunchKernelGGL(k_dot_combine, dim3((nout + DOT_CB_WAVES - 1) / DOT_CB_WAVES), dim3(DOT_CB_WAVES * WAVE), 0, e->stream,
                       e->q.dot.part.get(), (const long long *)f.col, f.cols, nout, lanes, f.head, d_out);
    HIP_TRY(hipGetLastError());
    return DPPR_OK;
}

// out[f][i] over the CSR of F queries (arguments, host ids, device ids' / w's range and a device destination validated by the caller)
int run_dot_sparse(dppr_engine *e, const StateView &v, int which, const int64_t *offsets, const int32_t *ids, const double *w, int src,
                   int F, int dest, double *out) {
    if (int rc = query_begin(e, MAP_E2I)) return rc;
    QueryWork::Dot &dot = e->q.dot;
    const double *x = which == DPPR_DENSE_R ? v.r : v.p;
    const int gw = v.gw, n = v.n;
    const bool host_src = src == DPPR_DEST_HOST;
    const int64_t m = offsets[F];
    dot_tile_table(offsets, F, dot.tb);
    const size_t blk_bytes = dot_block_bytes(F, n, dest);
    Grow grow{e};
    Fold f;
    if (int rc = fold_setup(e, grow, F, m, host_src, n, blk_bytes, f)) return rc;
    unsigned char *in = dot.in.get();
    const int *d_ids = host_src ? reinterpret_cast<const int *>(in + f.wk.off_ids) : ids;
    const double *d_w = host_src ? reinterpret_cast<const double *>(in + f.wk.off_w) : w;
    double *d_out = dest == DPPR_DEST_HOST ? reinterpret_cast<double *>(dot.blk + DOT_HEAD_BYTES) : out;
    if (host_src && m > 0) {
        HIP_TRY(hipMemcpyAsync(in + f.wk.off_ids, ids, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(in + f.wk.off_w, w, sizeof(double) * (size_t)m, hipMemcpyHostToDevice, e->stream));
    }
    if (int rc = DeviceTime{e}.open()) return rc;
    if (int rc = fold_finish(e, f, F, n, d_out, [&](dim3 grid) {
            hipLaunchKernelGGL(k_dot_sparse, grid, dim3(DOT_TILE), dot_lds_bytes(gw, 1), e->stream, x, gw, n, e->d_ext2int.get(), e->V, d_ids,
                               d_w, f.tiles, f.n_tiles, f.head, dot.part.get(), f.cols);
        }))
        return rc;
    return dot_finish(e, blk_bytes, dot_out_bytes(F, n), dest, out);
}

int dot_dense_call(dppr_engine *e, const StateView &v, int which, const void *h, int dtype, int layout, int F, int dest, double *out) {
    if (!dot_dense_args_ok(which, h, dtype, layout, F, dest, out))
        return fail(e, DPPR_ERR_INVALID, "dot_dense_dev: which 0 or 1, dtype 0 or 1, h_layout 0 or 1, F in [1, DPPR_DOT_MAX_F], dest 0 or 1, non-null h / out");
    HIP_TRY(hipSetDevice(e->device));
    if (!dev_range_ok(e, h, dot_dense_h_bytes(dtype, F, e->V), dot_elem_bytes(dtype)))
        return fail(e, DPPR_ERR_INVALID, "dot_dense_dev: h must be aligned device memory of the engine's device, F x V elements inside one allocation");
    if (dest == DPPR_DEST_DEVICE && !dev_range_ok(e, out, dot_out_bytes(F, v.n), sizeof(double)))
        return fail(e, DPPR_ERR_INVALID, "dot_dense_dev: out must be aligned device memory of the engine's device, F x n doubles inside one allocation");
    std::lock_guard<std::mutex> map_lk(e->map_mu); // (as dppr_read)
    return run_dot_dense(e, v, which, h, dtype, layout, F, dest, out);
}

int dot_sparse_call(dppr_engine *e, const StateView &v, int which, const int64_t *offsets, const int32_t *ids, const double *w, int src,
                    int F, int dest, double *out) {
    if (!dot_sparse_args_ok(which, offsets, ids, w, src, F, dest, out))
        return fail(e, DPPR_ERR_INVALID, "dot_sparse: which 0 or 1, src 0 or 1, F in [1, DPPR_DOT_MAX_F], dest 0 or 1, non-null ids / w / out, offsets[0] = 0 and non-decreasing");
    HIP_TRY(hipSetDevice(e->device));
    const int64_t m = offsets[F];
    if (src == DPPR_DEST_DEVICE) {
        if (!dev_range_ok(e, ids, sizeof(int32_t) * (size_t)m, sizeof(int32_t)) || !dev_range_ok(e, w, sizeof(double) * (size_t)m, sizeof(double)))
            return fail(e, DPPR_ERR_INVALID, "dot_sparse: ids / w must be aligned device memory of the engine's device, offsets[F] entries inside one allocation");
    } else if (!dppr::ids_in_range(ids, m, e->V)) {
        return fail(e, DPPR_ERR_INVALID, "dot_sparse: ids in [0, V)");
    }
    if (dest == DPPR_DEST_DEVICE && !dev_range_ok(e, out, dot_out_bytes(F, v.n), sizeof(double)))
        return fail(e, DPPR_ERR_INVALID, "dot_sparse: out must be aligned device memory of the engine's device, F x n doubles inside one allocation");
    std::lock_guard<std::mutex> map_lk(e->map_mu);
    return run_dot_sparse(e, v, which, offsets, ids, w, src, F, dest, out);
}

// ---- forward walks and the refinement of point queries (dppr_walk.hpp, dppr_walk_plan.hpp) ------------------------------------------
// starts, endpoints and the results of a refine call: in place before the first kernel
int walk_workspace(dppr_engine *e, Grow &grow, size_t m, size_t ends_elems, size_t res_elems) {
    int rc = grow(e->q.wk.starts, m);
    if (!rc) rc = grow(e->q.wk.ends, ends_elems);
    if (!rc) rc = grow(e->q.wk.res, res_elems);
    return rc;
}

// the walk kernel in the engine's form over the m starts in wk.starts (both id maps are on the device)
int walk_enqueue(dppr_engine *e, const Epoch &ep, int m, int W, uint64_t seed, int *d_ends) {
    const long long total = walk_total(m, W), per_wave = walk_per_wave(total);
    const unsigned k0 = (unsigned)(seed & 0xffffffffu), k1 = (unsigned)(seed >> 32);
    const bool refill = e->walk_form == 0;
    hipLaunchKernelGGL(refill ? k_walk<true> : k_walk<false>, dim3((unsigned)(refill ? walk_blocks_refill(total) : walk_blocks_simple(total))),
                       dim3(WALK_BLOCK), 0, e->stream, ep.out_row_ptr.get(), ep.out_col.get(), e->d_ext2int.get(), e->d_int2ext.get(),
                       e->q.wk.starts.get(), (unsigned)W, total, per_wave, k0, k1, d_ends);
    HIP_TRY(hipGetLastError());
    return DPPR_OK;
}

// the endpoints of W walks from each of m starts (arguments, ids and a device destination validated by the caller), [m][W]
int run_walks(dppr_engine *e, const Epoch &ep, const int32_t *starts, int m, int W, uint64_t seed, int dest, int32_t *out_ends) {
    if (int rc = query_begin(e, MAP_E2I | MAP_I2E)) return rc;
    const bool host = dest == DPPR_DEST_HOST;
    Grow grow{e};
    if (int rc = walk_workspace(e, grow, (size_t)m, host ? (size_t)walk_total(m, W) : 0, 0)) return rc;
    int *d_ends = host ? e->q.wk.ends.get() : out_ends;
    HIP_TRY(hipMemcpyAsync(e->q.wk.starts, starts, sizeof(int) * (size_t)m, hipMemcpyHostToDevice, e->stream));
    if (int rc = DeviceTime{e}.open()) return rc;
    if (int rc = walk_enqueue(e, ep, m, W, seed, d_ends)) return rc;
    if (int rc = DeviceTime{e}.close()) return rc;
    if (host) HIP_TRY(hipMemcpyAsync(out_ends, d_ends, walk_ends_bytes(m, W), hipMemcpyDeviceToHost, e->stream));
    return run_end(e); // (a device destination is complete here: any stream of the caller may read it)
}

// est / corr / sumsq at m ids, [m][n]: the walks, the fold of r at their endpoints over the pieces of the dot products, the finish
int run_refine(dppr_engine *e, const Epoch &ep, const StateView &v, const int32_t *ids, int m, int W, uint64_t seed, double *out_est,
               double *out_corr, double *out_sumsq) {
    if (int rc = query_begin(e, MAP_E2I | MAP_I2E)) return rc;
    QueryWork::Walk &wk = e->q.wk;
    const int gw = v.gw, n = v.n;
    wk.off.resize((size_t)m + 1);
    for (int q = 0; q <= m; ++q) wk.off[(size_t)q] = (int64_t)q * W;
    dot_tile_table(wk.off.data(), m, e->q.dot.tb);
    const size_t mn = (size_t)m * (size_t)n;
    Grow grow{e};
    Fold f;
    if (int rc = walk_workspace(e, grow, (size_t)m, (size_t)walk_total(m, W), 2 * mn + walk_result_elems(m, n))) return rc;
    if (int rc = fold_setup(e, grow, m, 0, false, 2 * n, DOT_HEAD_BYTES, f)) return rc;
    double *d_folded = wk.res.get(), *d_res = d_folded + 2 * mn;
    HIP_TRY(hipMemcpyAsync(wk.starts, ids, sizeof(int) * (size_t)m, hipMemcpyHostToDevice, e->stream));
    if (int rc = DeviceTime{e}.open()) return rc;
    if (int rc = walk_enqueue(e, ep, m, W, seed, wk.ends.get())) return rc;
    if (int rc = fold_finish(e, f, m, 2 * n, d_folded, [&](dim3 grid) {
            hipLaunchKernelGGL(k_walk_fold, grid, dim3(DOT_TILE), dot_lds_bytes(gw, 1), e->stream, v.r, gw, n, e->d_ext2int.get(), wk.ends.get(),
                               f.tiles, f.n_tiles, e->q.dot.part.get(), f.cols);
        }))
        return rc;
    hipLaunchKernelGGL(k_refine_finish, dim3(grid_for((int64_t)mn)), dim3(BLOCK), 0, e->stream, v.p, gw, n, e->d_ext2int.get(), wk.starts.get(),
                       m, W, d_folded, d_res);
    HIP_TRY(hipGetLastError());
    if (int rc = DeviceTime{e}.close()) return rc;
    HIP_TRY(hipMemcpyAsync(out_est, d_res, sizeof(double) * mn, hipMemcpyDeviceToHost, e->stream));
    if (out_corr) HIP_TRY(hipMemcpyAsync(out_corr, d_res + mn, sizeof(double) * mn, hipMemcpyDeviceToHost, e->stream));
    if (out_sumsq) HIP_TRY(hipMemcpyAsync(out_sumsq, d_res + 2 * mn, sizeof(double) * mn, hipMemcpyDeviceToHost, e->stream));
    return run_end(e);
}

int walks_call(dppr_engine *e, const Epoch &ep, const int32_t *starts, int32_t m, int32_t W, uint64_t seed, int dest, int32_t *out_ends) {
    if (!walk_args_ok(starts, m, W, dest, out_ends))
        return fail(e, DPPR_ERR_INVALID, "walks: m in [1, DPPR_WALK_MAX_M], W in [1, DPPR_WALK_MAX_W], m * W <= 2^26, dest 0 or 1, non-null starts / out_ends");
    if (!dppr::ids_in_range(starts, m, e->V)) return fail(e, DPPR_ERR_INVALID, "walks: starts in [0, V)");
    HIP_TRY(hipSetDevice(e->device));
    if (dest == DPPR_DEST_DEVICE && !dev_range_ok(e, out_ends, walk_ends_bytes(m, W), sizeof(int32_t)))
        return fail(e, DPPR_ERR_INVALID, "walks: out_ends must be aligned device memory of the engine's device, m x W ints inside one allocation");
    std::lock_guard<std::mutex> map_lk(e->map_mu); // (as dppr_read)
    return run_walks(e, ep, starts, m, W, seed, dest, out_ends);
}

int refine_call(dppr_engine *e, const StateView &v, const Epoch &ep, const int32_t *ids, int32_t m, int32_t W, uint64_t seed,
                double *out_est, double *out_corr, double *out_sumsq) {
    if (!refine_args_ok(ids, m, W, out_est))
        return fail(e, DPPR_ERR_INVALID, "refine_at: m in [1, DPPR_WALK_MAX_M], W in [1, DPPR_WALK_MAX_W], m * W <= 2^26, non-null ids / out_est");
    if (!dppr::ids_in_range(ids, m, e->V)) return fail(e, DPPR_ERR_INVALID, "refine_at: ids in [0, V)");
    if (!v.st.converged) return fail(e, DPPR_ERR_INVALID, "refine_at: the state is not converged (solve or update it first)");
    if (!refine_epoch_ok(v.st.last_epoch, ep.id))
        return fail(e, DPPR_ERR_INVALID, "refine_at: the state stands on another epoch than the one given: walks over another graph would give a biased estimate");
    std::lock_guard<std::mutex> map_lk(e->map_mu); // (as dppr_read)
    return run_refine(e, ep, v, ids, m, W, seed, out_est, out_corr, out_sumsq);
}

// ---- the conductance sweep over a top-k order (dppr_cluster.hpp, dppr_cluster_plan.hpp) -------------------------------------------
// The ORDER STAGE, the opening cluster and subgraph share: the top-k order of every lane and the rank table that says where a
// vertex stands in it. cl_graph: the epoch's two CSRs and the zones of the state, as the kernels of both families read them.
ClGraph cl_graph(const Epoch &ep, const TkState &st) {
    return {ep.out_row_ptr.get(), ep.out_col.get(), ep.row_ptr.get(), ep.adj.get(), st.n_int, st.lo_parked, st.rows};
}

// ... its workspace: the selection's, the rank table by the occupied rows, the chunk list of the later kernels by the epoch's edges
int order_workspace(dppr_engine *e, Grow &grow, int n, size_t rows, long long Ed) {
    int rc = topk_workspace(e, grow, n, rows);
    if (!rc) rc = grow(e->q.cl.rank, cl_rank_elems(rows, n), with_slack(cl_rank_elems(rows, n)));
    if (!rc) rc = grow(e->q.cl.list, cl_list_cap(n, Ed));
    return rc;
}
unsigned order_list_cap(int n, long long Ed) { return (unsigned)std::min<size_t>(cl_list_cap(n, Ed), 0xffffffffu); }

// ... and its kernels, enqueued: the rank table cleared, the selection with its ids and p where the caller says (p NULL: to the
// top-k block, which nobody copies, like the counts -- *out_cnt -- and r), k_cl_rank
int order_enqueue(dppr_engine *e, const ClGraph &g, const TkState &st, int k, double min_p, int *ids, double *p, const int **out_cnt) {
    const TkLayout tkl = tk_layout(st.n, k, true);
    unsigned char *tkres = e->q.tk.res.get();
    int *cnt = reinterpret_cast<int *>(tkres + tkl.off_cnt);
    const int stride = cl_stride(st.n), nk = st.n * k;
    if (st.rows > 0) HIP_TRY(hipMemsetAsync(e->q.cl.rank, 0xff, sizeof(unsigned short) * (size_t)st.rows * (size_t)stride, e->stream));
    if (int rc = select_enqueue(e, st, e->d_int2ext, k, min_p, cnt, ids, p ? p : reinterpret_cast<double *>(tkres + tkl.off_p),
                                reinterpret_cast<double *>(tkres + tkl.off_r)))
        return rc;
    hipLaunchKernelGGL(k_cl_rank, dim3((nk + CL_BLOCK - 1) / CL_BLOCK), dim3(CL_BLOCK), 0, e->stream, g, e->d_ext2int.get(), cnt, ids, st.n, k, stride,
                       e->q.cl.rank.get());
    HIP_TRY(hipGetLastError());
    *out_cnt = cnt;
    return DPPR_OK;
}

// the per-position values and the block of the sweep: in place before the first kernel
int cluster_workspace(dppr_engine *e) {
    QueryWork::Cluster &cl = e->q.cl;
    if (!cl.pin) { // (the last of the set: one that failed half way is made again)
        const size_t block = cl_layout(GS_MAX, DPPR_CLUSTER_MAX, true, true, true, true).total_bytes;
        HIP_TRY(cl.d.regrow(sizeof(ClCtl) / sizeof(int) + (size_t)3 * GS_MAX * DPPR_CLUSTER_MAX));
        HIP_TRY(cl.blk.regrow(block));
        HIP_TRY(cl.pin.regrow(block));
    }
    return DPPR_OK;
}

// The best prefix of every lane's top-k order and, where asked for, the order and its prefix arrays (arguments and the epoch
// validated by the caller). Results are lane-major: best [n], the arrays [n][k]. The selection writes its ids straight into the
// block; nothing is read back between the kernels.
int run_cluster(dppr_engine *e, const Epoch &ep, const StateView &v, int k, double min_p, int min_size, dppr_cluster_t *out_best,
                int32_t *out_ids, int64_t *out_cut_out, int64_t *out_cut_in, int64_t *out_vol) {
    if (int rc = query_begin(e, MAP_E2I | MAP_I2E)) return rc;
    QueryWork::Cluster &cl = e->q.cl;
    const int n = v.n, stride = cl_stride(n);
    const TkState st = tk_state(e, v.p, v.r, v.gw, n);
    Grow grow{e};
    if (int rc = order_workspace(e, grow, n, (size_t)st.rows, ep.Ed)) return rc;
    if (int rc = cluster_workspace(e)) return rc;
    const ClLayout lay = cl_layout(n, k, out_ids != nullptr, out_cut_out != nullptr, out_cut_in != nullptr, out_vol != nullptr);
    unsigned char *blk = cl.blk.get();
    int *ids = reinterpret_cast<int *>(blk + lay.off_ids);
    ClCtl *ctl = reinterpret_cast<ClCtl *>(cl.d.get());
    int *d = cl.d + sizeof(ClCtl) / sizeof(int);
    const ClGraph g = cl_graph(ep, st);
    const unsigned list_cap = order_list_cap(n, ep.Ed);
    const int nk = n * k;
    const int *cnt = nullptr, *x2i = e->d_ext2int.get();
    if (int rc = DeviceTime{e}.open()) return rc;
    HIP_TRY(hipMemsetAsync(ctl, 0, sizeof(ClCtl), e->stream));
    if (int rc = order_enqueue(e, g, st, k, min_p, ids, nullptr, &cnt)) return rc;
    hipLaunchKernelGGL(k_cl_rows, dim3((nk + CL_WAVES - 1) / CL_WAVES), dim3(CL_BLOCK), 0, e->stream, g, x2i, cnt, ids, n, k, stride,
                       cl.rank.get(), d, ctl, cl.list.get(), list_cap);
    hipLaunchKernelGGL(k_cl_big, dim3(grid_for((int64_t)list_cap, CL_WAVES, 1024)), dim3(CL_BLOCK), 0, e->stream, g, x2i, ids, n, k, stride,
                       cl.rank.get(), d, ctl, cl.list.get(), list_cap);
    hipLaunchKernelGGL(k_cl_scan, dim3(n), dim3(CL_SCAN_BLOCK), 0, e->stream, cnt, d, n, k, (long long)ep.Ed, min_size,
                       reinterpret_cast<dppr_cluster_t *>(blk + lay.off_best), reinterpret_cast<long long *>(blk + lay.off_cut_out),
                       reinterpret_cast<long long *>(blk + lay.off_cut_in), reinterpret_cast<long long *>(blk + lay.off_vol));
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_block(e, cl.blk, cl.pin, lay.copy_bytes)) return rc;
    const size_t nks = (size_t)n * (size_t)k;
    memcpy(out_best, cl.pin + lay.off_best, sizeof(dppr_cluster_t) * (size_t)n);
    if (out_ids) memcpy(out_ids, cl.pin + lay.off_ids, sizeof(int32_t) * nks);
    if (out_cut_out) memcpy(out_cut_out, cl.pin + lay.off_cut_out, sizeof(int64_t) * nks);
    if (out_cut_in) memcpy(out_cut_in, cl.pin + lay.off_cut_in, sizeof(int64_t) * nks);
    if (out_vol) memcpy(out_vol, cl.pin + lay.off_vol, sizeof(int64_t) * nks);
    return DPPR_OK;
}

int cluster_call(dppr_engine *e, const StateView &v, const Epoch &ep, int32_t k, double min_p, int32_t min_size, dppr_cluster_t *out_best,
                 int32_t *out_ids, int64_t *out_cut_out, int64_t *out_cut_in, int64_t *out_vol) {
    if (!cluster_args_ok(k, min_p, min_size, out_best))
        return fail(e, DPPR_ERR_INVALID, "cluster: k in [1, DPPR_CLUSTER_MAX], min_p >= 0, min_size in [1, k], non-null out_best");
    if (!refine_epoch_ok(v.st.last_epoch, ep.id))
        return fail(e, DPPR_ERR_INVALID, "cluster: the state stands on another epoch than the one given: a cut of another graph says nothing about it");
    std::lock_guard<std::mutex> map_lk(e->map_mu); // (as dppr_read: one state of the id space for the whole query)
    return run_cluster(e, ep, v, k, min_p, min_size, out_best, out_ids, out_cut_out, out_cut_in, out_vol);
}

// ---- the subgraph a top-k order induces (dppr_subgraph.hpp, dppr_subgraph_plan.hpp) ------------------------------------------------
// the per-position work and the block with its pinned twin: in place before the first kernel
int subgraph_workspace(dppr_engine *e, Grow &grow, size_t block_bytes) {
    QueryWork::Subgraph &sg = e->q.sg;
    int rc = grow(sg.work, sg_work_elems(GS_MAX, DPPR_SUBGRAPH_MAX));
    if (!rc) rc = grow(sg.blk, block_bytes);
    if (!rc) rc = grow(sg.pin, block_bytes);
    return rc;
}

// every section a device destination names: aligned device memory of the engine's device, inside one allocation
bool sg_dest_ok(const dppr_engine *e, int n, int k, int64_t capc, const int32_t *ids, const double *p, const int64_t *row_ptr, const int32_t *col) {
    return (!ids || dev_range_ok(e, ids, sg_ids_bytes(n, k), sizeof(int32_t))) && (!p || dev_range_ok(e, p, sg_p_bytes(n, k), sizeof(double))) &&
           (!row_ptr || dev_range_ok(e, row_ptr, sg_row_ptr_bytes(n, k), sizeof(int64_t))) &&
           (capc <= 0 || dev_range_ok(e, col, sg_col_bytes(capc), sizeof(int32_t)));
}

// The order of every lane and the CSR of the stored edges among its vertices (arguments, the epoch and a device destination
// validated by the caller). The selection writes ids and p where they are wanted; count, chunks and scan follow without a read
// back; the head comes to the host once, the offsets and counts are written, and the fill runs if the entries fit cap.
int run_subgraph(dppr_engine *e, const Epoch &ep, const StateView &v, int k, double min_p, int64_t cap, int dest, int32_t *out_counts,
                 int64_t *out_offsets, int32_t *out_ids, double *out_p, int64_t *out_row_ptr, int32_t *out_col) {
    if (int rc = query_begin(e, MAP_E2I | MAP_I2E)) return rc;
    QueryWork::Subgraph &sg = e->q.sg;
    const int n = v.n, stride = cl_stride(n);
    const bool host = dest == DPPR_DEST_HOST;
    const int64_t capc = sg_cap_clamped(cap, ep.Ed, n);
    const TkState st = tk_state(e, v.p, v.r, v.gw, n);
    const SgLayout lay = sg_layout(n, k, host ? capc : 0, out_ids != nullptr, out_p != nullptr, out_row_ptr != nullptr, out_col != nullptr);
    Grow grow{e};
    if (int rc = order_workspace(e, grow, n, (size_t)st.rows, ep.Ed)) return rc;
    if (int rc = subgraph_workspace(e, grow, lay.total_bytes)) return rc;
    unsigned char *blk = sg.blk.get();
    SgHead *head = reinterpret_cast<SgHead *>(blk + lay.off_head);
    int *d_ids = !host && out_ids ? out_ids : reinterpret_cast<int *>(blk + lay.off_ids);
    double *d_p = !host && out_p ? out_p : reinterpret_cast<double *>(blk + lay.off_p);
    long long *d_row_ptr = !host && out_row_ptr ? reinterpret_cast<long long *>(out_row_ptr) : reinterpret_cast<long long *>(blk + lay.off_row_ptr);
    int *d_col = host ? reinterpret_cast<int *>(blk + lay.off_col) : out_col;
    SgCtl *ctl = reinterpret_cast<SgCtl *>(sg.work.get());
    const int nk = n * k;
    int *m = sg.work + sizeof(SgCtl) / sizeof(int), *long_list = m + nk;
    const ClGraph g = cl_graph(ep, st);
    const unsigned list_cap = order_list_cap(n, ep.Ed);
    const int *cnt = nullptr, *x2i = e->d_ext2int.get();
    const unsigned short *rank = e->q.cl.rank.get();
    if (int rc = DeviceTime{e}.open()) return rc;
    HIP_TRY(hipMemsetAsync(ctl, 0, sizeof(SgCtl), e->stream));
    if (int rc = order_enqueue(e, g, st, k, min_p, d_ids, d_p, &cnt)) return rc;
    hipLaunchKernelGGL(k_sg_count, dim3((nk + CL_WAVES - 1) / CL_WAVES), dim3(CL_BLOCK), 0, e->stream, g, x2i, cnt, d_ids, n, k, stride, rank, m,
                       ctl, e->q.cl.list.get(), list_cap);
    hipLaunchKernelGGL(k_sg_big, dim3(grid_for((int64_t)list_cap, CL_WAVES, 1024)), dim3(CL_BLOCK), 0, e->stream, g, x2i, d_ids, k, stride, rank, m,
                       ctl, e->q.cl.list.get(), list_cap);
    hipLaunchKernelGGL(k_sg_scan, dim3(n), dim3(CL_SCAN_BLOCK), 0, e->stream, cnt, m, n, k, head, d_row_ptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(sg.pin, blk + lay.off_head, SG_HEAD_BYTES, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const SgHead *h = reinterpret_cast<const SgHead *>(sg.pin.get());
    for (int i = 0; i <= n; ++i) out_offsets[i] = h->offsets[i];
    for (int i = 0; i < n; ++i) out_counts[i] = h->count[i];
    const int64_t total = h->offsets[n];
    const bool fill = capc > 0 && total > 0 && total <= capc;
    if (fill) {
        hipLaunchKernelGGL(k_sg_fill, dim3((nk + CL_WAVES - 1) / CL_WAVES), dim3(CL_BLOCK), 0, e->stream, g, x2i, cnt, d_ids, n, k, stride, rank,
                           d_row_ptr, e->sg_wave_max, d_col, ctl, long_list);
        hipLaunchKernelGGL(k_sg_long, dim3(SG_LONG_GRID), dim3(SG_LONG_BLOCK), 0, e->stream, g, x2i, d_ids, k, stride, rank, d_row_ptr, d_col, ctl,
                           long_list, (unsigned)nk);
        HIP_TRY(hipGetLastError());
    }
    if (int rc = DeviceTime{e}.close()) return rc;
    // a host destination: one copy from the first to the last section asked for (col by the entries it holds, not by cap)
    size_t hi = lay.copy_hi;
    if (host && out_col && capc > 0) hi = fill ? lay.off_col + sg_col_bytes(total) : std::min(hi, lay.off_col);
    const bool copy = host && hi > lay.copy_lo;
    if (copy) HIP_TRY(hipMemcpyAsync(sg.pin + lay.copy_lo, blk + lay.copy_lo, hi - lay.copy_lo, hipMemcpyDeviceToHost, e->stream));
    if (int rc = run_end(e)) return rc; // (a device destination is complete here: any stream of the caller may read it)
    if (host) {
        if (out_ids) memcpy(out_ids, sg.pin + lay.off_ids, sg_ids_bytes(n, k));
        if (out_p) memcpy(out_p, sg.pin + lay.off_p, sg_p_bytes(n, k));
        if (out_row_ptr) memcpy(out_row_ptr, sg.pin + lay.off_row_ptr, sg_row_ptr_bytes(n, k));
        if (fill) memcpy(out_col, sg.pin + lay.off_col, sg_col_bytes(total));
    }
    return DPPR_OK;
}

int subgraph_call(dppr_engine *e, const StateView &v, const Epoch &ep, int32_t k, double min_p, int64_t cap, int dest, int32_t *out_counts,
                  int64_t *out_offsets, int32_t *out_ids, double *out_p, int64_t *out_row_ptr, int32_t *out_col) {
    if (!subgraph_args_ok(k, min_p, cap, dest, out_offsets, out_counts, out_col))
        return fail(e, DPPR_ERR_INVALID, "subgraph: k in [1, DPPR_SUBGRAPH_MAX], min_p >= 0, cap >= 0, dest 0 or 1, non-null offsets / counts, non-null col when cap > 0");
    if (!refine_epoch_ok(v.st.last_epoch, ep.id))
        return fail(e, DPPR_ERR_INVALID, "subgraph: the state stands on another epoch than the one given: the edges of another graph are not those its order was computed on");
    HIP_TRY(hipSetDevice(e->device));
    if (dest == DPPR_DEST_DEVICE && !sg_dest_ok(e, v.n, k, sg_cap_clamped(cap, ep.Ed, v.n), out_ids, out_p, out_row_ptr, out_col))
        return fail(e, DPPR_ERR_INVALID, "subgraph: ids / p / row_ptr / col must be aligned device memory of the engine's device, n x k (row_ptr: n x (k + 1), col: cap) entries inside one allocation");
    std::lock_guard<std::mutex> map_lk(e->map_mu); // (as dppr_read: one state of the id space for the whole query)
    return run_subgraph(e, ep, v, k, min_p, cap, dest, out_counts, out_offsets, out_ids, out_p, out_row_ptr, out_col);
}

// ---- ranked candidates (dppr_rank.hpp, dppr_rank_plan.hpp) ----------------------------------------------------------------------
// the seeds of a state's lanes as the kernels read them: a slot's source, a group's sources and the seed table of its set lanes
RkLanes rank_lanes(const Slot &s) {
    RkLanes l{};
    for (int i = 0; i < GS_MAX; ++i) l.src.s[i] = -1;
    l.src.s[0] = s.source;
    l.seeds = rk_seeds(l.src.s, nullptr, 1);
    return l;
}
RkLanes rank_lanes(const Group &g) {
    RkLanes l{};
    l.src = g.src;
    const bool table = (bool)g.tg;
    if (table) l.tg = tg_dev(g);
    l.seeds = rk_seeds(g.src.s, table ? g.ttab.off : nullptr, g.n);
    return l;
}

// the epoch's CSRs (ep NULL: the spec reads none) and the live zone
RkGraph rank_graph(const dppr_engine *e, const Epoch *ep) {
    RkGraph g{};
    if (ep) {
        g.out_row_ptr = ep->out_row_ptr.get();
        g.out_col = ep->out_col.get();
        g.in_row_ptr = ep->row_ptr.get();
        g.in_adj = ep->adj.get();
    }
    g.n_int = e->n_int;
    g.V = e->V;
    return g;
}

RkRule rank_rule(const RkSpec &sp) { return {sp.mask_dev, sp.mask == DPPR_MASK_DENY ? 1 : 0, sp.factor_dev}; }

// One of the instantiations of a kernel template <KIND, T> by a spec's factor and the dtype of g: f(integral_constant<int, KIND>(), T())
template <class F> int by_factor(const RkSpec &sp, F &&f) {
    switch (sp.factor) {
    case DPPR_FACTOR_DEV:
        return sp.factor_dtype == DPPR_F32 ? f(std::integral_constant<int, DPPR_FACTOR_DEV>(), float())
                                           : f(std::integral_constant<int, DPPR_FACTOR_DEV>(), double());
    case DPPR_FACTOR_DEG: return f(std::integral_constant<int, DPPR_FACTOR_DEG>(), double());
    case DPPR_FACTOR_INV_DEG: return f(std::integral_constant<int, DPPR_FACTOR_INV_DEG>(), double());
    default: return f(std::integral_constant<int, DPPR_FACTOR_NONE>(), double());
    }
}

// the exclusion words by the live rows, the seeds' row lengths and the piece list by its bound: in place before the first kernel
int rank_mark_workspace(dppr_engine *e, Grow &grow, const RkLanes &l, const RkSpec &sp, const Epoch *ep) {
    if (!sp.exclude) return DPPR_OK;
    QueryWork::Rank &rk = e->q.rk;
    const size_t live = rk_excl_elems((size_t)e->n_int);
    int rc = grow(rk.excl, live, std::min<size_t>((size_t)e->V, with_slack(live)));
    if (rc || !(sp.exclude & RK_EXCLUDE_ROWS)) return rc;
    const size_t len = rk_len_elems((size_t)l.seeds.total());
    rc = grow(rk.len, len);
    if (!rc) rc = grow(rk.len_pin, len);
    if (!rc) rc = grow(rk.list, std::max<size_t>(rk_piece_cap(l.seeds, ep->Ed, sp.exclude, e->rk_piece), 1));
    return rc;
}

// The marking stage, enqueued (its workspace is in place): the words zeroed, the seeds' row lengths read back -- the one wait of
// the stage -- and cut into pieces on the host, one wave of k_rk_mark per piece. Returns the words, or NULL: nothing is excluded.
int rank_mark_enqueue(dppr_engine *e, const RkLanes &l, const RkSpec &sp, const RkGraph &g, const unsigned **out_excl) {
    *out_excl = nullptr;
    if (!sp.exclude) return DPPR_OK;
    QueryWork::Rank &rk = e->q.rk;
    const int total = l.seeds.total();
    HIP_TRY(hipMemsetAsync(rk.excl, 0, sizeof(unsigned) * rk_excl_elems((size_t)e->n_int), e->stream));
    size_t n_items = 0;
    if ((sp.exclude & RK_EXCLUDE_ROWS) && total > 0) {
        hipLaunchKernelGGL(k_rk_rowlen, dim3(grid_for(total, RK_BLOCK)), dim3(RK_BLOCK), 0, e->stream, l, g, rk.len.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(rk.len_pin, rk.len, sizeof(int) * 2 * (size_t)total, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        rk_pieces(rk.len_pin.get(), total, sp.exclude, e->rk_piece, rk.items);
        n_items = std::min(rk.items.size(), rk.list.capacity()); // (rk_piece_cap bounds what a call can have)
        if (n_items > 0)
            HIP_TRY(hipMemcpyAsync(rk.list, rk.items.data(), sizeof(unsigned long long) * n_items, hipMemcpyHostToDevice, e->stream));
    }
    const int64_t blocks = std::max<int64_t>(((int64_t)n_items + RK_WAVES - 1) / RK_WAVES, ((int64_t)total + RK_BLOCK - 1) / RK_BLOCK);
    hipLaunchKernelGGL(k_rk_mark, dim3(grid_for(blocks, 1)), dim3(RK_BLOCK), 0, e->stream, l, g, sp.exclude, e->rk_piece, rk.list.get(),
                       (unsigned)n_items, rk.excl.get());
    HIP_TRY(hipGetLastError());
    *out_excl = rk.excl.get();
    return DPPR_OK;
}

// Top k of every lane by the spec's score (arguments, the spec's device pointers and the epoch validated by the caller; ep NULL:
// the spec reads no CSR). Results are lane-major: [n][k]. Every buffer is in place before the first kernel; the scratch state is
// 8 n + 4 bytes per occupied row.
int run_topk_ranked(dppr_engine *e, const StateView &v, const RkLanes &l, const Epoch *ep, const RkSpec &sp, int k, double min_score,
                    int32_t *out_ids, double *out_score, int32_t *out_counts) {
    if (int rc = query_begin(e, MAP_I2E)) return rc;
    QueryWork::Scratch &sc = e->q.sc;
    const TkState st = tk_state(e, v.p, v.p, v.gw, v.n);
    Grow grow{e};
    if (int rc = scratch_workspace(e, grow, (size_t)st.rows, v.n, 1)) return rc;
    if (int rc = rank_mark_workspace(e, grow, l, sp, ep)) return rc;
    const RkGraph g = rank_graph(e, ep);
    const RkRule rule = rank_rule(sp);
    if (int rc = DeviceTime{e}.open()) return rc;
    const unsigned *excl = nullptr;
    if (int rc = rank_mark_enqueue(e, l, sp, g, &excl)) return rc;
    by_factor(sp, [&](auto kind, auto elem) -> int {
        using T = decltype(elem);
        hipLaunchKernelGGL((k_rk_scores<decltype(kind)::value, T>), dim3(tile_grid(st.rows)), dim3(TK_TILE_BLOCK), 0, e->stream, st,
                           e->d_int2ext.get(), excl, rule, g, sc.a.get(), sc.ext.get());
        return DPPR_OK;
    });
    HIP_TRY(hipGetLastError());
    return run_select(e, scratch_state(sc.a, sc.a, v.n, st.rows), sc.ext, k, min_score, out_ids, out_score, nullptr, out_counts);
}

// the scores at m external ids (validated by the caller like the rest, m > 0), [m][n]
int run_rank_score_at(dppr_engine *e, const StateView &v, const RkLanes &l, const Epoch *ep, const RkSpec &sp, const int32_t *ids, int m,
                      double *out_score) {
    if (int rc = query_begin(e, MAP_E2I)) return rc;
    Grow grow{e};
    if (int rc = rank_mark_workspace(e, grow, l, sp, ep)) return rc;
    const RkGraph g = rank_graph(e, ep);
    const RkRule rule = rank_rule(sp);
    return point_read(e, grow, ids, m, v.n, 1, out_score, nullptr, [&](const int *d_ids, double *d_out, double *) {
        const unsigned *excl = nullptr;
        if (int rc = rank_mark_enqueue(e, l, sp, g, &excl)) return rc;
        return by_factor(sp, [&](auto kind, auto elem) -> int {
            using T = decltype(elem);
            hipLaunchKernelGGL((k_rk_score_at<decltype(kind)::value, T>), dim3(grid_for((int64_t)m * v.n, RK_BLOCK)), dim3(RK_BLOCK), 0, e->stream,
                               v.p, v.gw, v.n, e->d_ext2int.get(), d_ids, m, excl, rule, g, d_out);
            return DPPR_OK;
        });
    });
}

// the spec's device pointers (shared with the forms over a forward track). NULL: fine; otherwise the words of the rejection.
const char *rank_spec_ptrs_refused(dppr_engine *e, const dppr_rank_spec_t *spec) {
    if (rank_needs_factor_dev(spec) &&
        !dev_range_ok(e, spec->factor_dev, rank_factor_bytes(spec->factor_dtype, e->V), rank_factor_elem_bytes(spec->factor_dtype)))
        return "ranked: factor_dev must be aligned device memory of the engine's device, V elements inside one allocation";
    if (rank_needs_mask_dev(spec) && !dev_range_ok(e, spec->mask_dev, rank_mask_bytes(e->V), 1))
        return "ranked: mask_dev must be device memory of the engine's device, V bytes inside one allocation";
    return nullptr;
}

// What both forms check after their own arguments: the epoch, where the spec needs one (*out_ep stays NULL otherwise), and the
// spec's device pointers. NULL: fine; otherwise the words of the rejection.
const char *rank_spec_refused(dppr_engine *e, const StateView &v, int32_t epoch, const dppr_rank_spec_t *spec, const Epoch **out_ep) {
    *out_ep = nullptr;
    if (rank_needs_epoch(spec)) {
        const Epoch *ep = find_epoch(e, epoch);
        if (!ep) return "ranked: epoch not resident (evicted or never built)";
        if (!refine_epoch_ok(v.st.last_epoch, ep->id))
            return "ranked: the state stands on another epoch than the one given: the degrees and neighbours of another graph are not those its order was computed on";
        *out_ep = ep;
    }
    return rank_spec_ptrs_refused(e, spec);
}

// (Owner: a Slot or a Group. Its seeds are read under map_mu: a renumbering beside the call renames them)
template <class Owner>
int topk_ranked_call(dppr_engine *e, Owner &o, int32_t epoch, const dppr_rank_spec_t *spec, int32_t k, double min_score, int32_t *out_ids,
                     double *out_score, int32_t *out_counts) {
    const StateView v = view(o);
    if (!rank_topk_args_ok(spec, k, min_score, out_ids, out_score, out_counts))
        return fail(e, DPPR_ERR_INVALID, "topk_ranked: factor 0..3, factor_dtype 0 or 1, mask 0..2, exclude bits 1 | 2 | 4, k in [1, DPPR_TOPK_MAX], min_score >= 0, non-null ids / score / counts");
    HIP_TRY(hipSetDevice(e->device));
    const Epoch *ep = nullptr;
    if (const char *why = rank_spec_refused(e, v, epoch, spec, &ep)) return fail(e, DPPR_ERR_INVALID, why);
    std::lock_guard<std::mutex> map_lk(e->map_mu); // (as dppr_read: one state of the id space for the whole query)
    return run_topk_ranked(e, v, rank_lanes(o), ep, rank_spec(spec), k, min_score, out_ids, out_score, out_counts);
}

template <class Owner>
int rank_score_at_call(dppr_engine *e, Owner &o, int32_t epoch, const dppr_rank_spec_t *spec, const int32_t *ids, int32_t m, double *out_score) {
    const StateView v = view(o);
    if (!rank_score_at_args_ok(spec, ids, m, e->V, out_score))
        return fail(e, DPPR_ERR_INVALID, "rank_score_at: factor 0..3, factor_dtype 0 or 1, mask 0..2, exclude bits 1 | 2 | 4, ids in [0, V), non-null score");
    HIP_TRY(hipSetDevice(e->device));
    const Epoch *ep = nullptr;
    if (const char *why = rank_spec_refused(e, v, epoch, spec, &ep)) return fail(e, DPPR_ERR_INVALID, why);
    if (m == 0) return DPPR_OK;
    std::lock_guard<std::mutex> map_lk(e->map_mu);
    return run_rank_score_at(e, v, rank_lanes(o), ep, rank_spec(spec), ids, m, out_score);
}

// ---- positions of given vertices in a lane's order (dppr_position.hpp, dppr_position_plan.hpp) -----------------------------------
// the ids and the query scores (the buffer of the point reads), keys and places, slots, the block and its pinned twin: in place
// before the first kernel
int position_workspace(dppr_engine *e, Grow &grow, int n, int m) {
    QueryWork::Position &ps = e->q.pos;
    if (!ps.lds_set) { // (a lane's 4096 queries take 64 bytes more than the 64 KiB a kernel has without asking)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_pos_count), hipFuncAttributeMaxDynamicSharedMemorySize, (int)POS_LDS_MAX));
        ps.lds_set = true;
    }
    const PosWork w = pos_work(n, m);
    const size_t blk = pos_layout(n, m).total_bytes;
    int rc = grow(e->q.ra.buf, ra_layout(m, n, 1).total_bytes);
    if (!rc) rc = grow(ps.keys, std::max<size_t>(w.key_bytes, 1));
    if (!rc) rc = grow(ps.slots, w.slot_elems);
    if (!rc) rc = grow(ps.blk, blk);
    if (!rc) rc = grow(ps.pin, blk);
    return rc;
}

// The back half of a position call, from the filled scratch state (sc: `rows` rows of n scores with their external ids) and the
// query scores at the uploaded ids (the buffer of the point reads) to the caller's arrays: the order of the queries, the count
// pass, the sums, the one copy back. Its workspace is in place (position_workspace), the slots are zeroed, the bracket is open.
int position_finish(dppr_engine *e, int rows, int n, double min_score, int m, int32_t *out_pos, int32_t *out_counts) {
    QueryWork::Scratch &sc = e->q.sc;
    QueryWork::Position &ps = e->q.pos;
    const PosShape shape = pos_shape(n, m, e->pos_tile);
    const PosWork w = pos_work(n, m);
    const PosLayout lay = pos_layout(n, m);
    const RaLayout ra = ra_layout(m, n, 1);
    int *d_ids = reinterpret_cast<int *>(e->q.ra.buf + ra.off_ids);
    double *d_qs = reinterpret_cast<double *>(e->q.ra.buf + ra.off_a);
    unsigned long long *d_key = reinterpret_cast<unsigned long long *>(ps.keys + w.off_key);
    int *d_place = reinterpret_cast<int *>(ps.keys + w.off_place);
    int *res_cnt = reinterpret_cast<int *>(ps.blk + lay.off_cnt), *res_pos = reinterpret_cast<int *>(ps.blk + lay.off_pos);
    if (m > 0)
        hipLaunchKernelGGL(k_pos_order, dim3((m + POS_ORDER_BLOCK - 1) / POS_ORDER_BLOCK, n), dim3(POS_ORDER_BLOCK), 0, e->stream, d_qs, d_ids, m, n,
                           min_score, d_key, d_place);
    hipLaunchKernelGGL(k_pos_count, dim3(pos_grid_x(rows, shape), shape.lane_blocks, shape.passes), dim3(POS_BLOCK),
                       pos_lds_bytes(shape.lanes, shape.tile), e->stream, sc.a.get(), sc.ext.get(), rows, n, min_score, d_key, d_place, d_ids, m,
                       shape.tile, shape.lanes, ps.slots.get());
    hipLaunchKernelGGL(k_pos_finish, dim3(n), dim3(POS_BLOCK), 0, e->stream, ps.slots.get(), d_key, d_place, m, n, shape.tile, res_cnt, res_pos);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_block(e, ps.blk, ps.pin, lay.total_bytes)) return rc;
    if (out_counts) memcpy(out_counts, ps.pin + lay.off_cnt, sizeof(int32_t) * (size_t)n);
    if (m > 0) memcpy(out_pos, ps.pin + lay.off_pos, sizeof(int32_t) * (size_t)m * (size_t)n);
    return DPPR_OK;
}

// Positions of m external ids in every lane's order by the spec's score, and every lane's count of qualifying vertices (arguments,
// the spec's device pointers and the epoch validated by the caller; m == 0: the counts alone). Every buffer is in place before the
// first kernel, every stage is enqueued before the one copy back: the marking and the scratch state of run_topk_ranked, the scores
// at the ids of run_rank_score_at, the order of the queries, the count pass, the sums.
int run_position(dppr_engine *e, const StateView &v, const RkLanes &l, const Epoch *ep, const RkSpec &sp, double min_score, const int32_t *ids,
                 int m, int32_t *out_pos, int32_t *out_counts) {
    if (int rc = query_begin(e, MAP_E2I | MAP_I2E)) return rc;
    QueryWork::Scratch &sc = e->q.sc;
    QueryWork::Position &ps = e->q.pos;
    const int n = v.n;
    const TkState st = tk_state(e, v.p, v.p, v.gw, n);
    Grow grow{e};
    if (int rc = scratch_workspace(e, grow, (size_t)st.rows, n, 1)) return rc;
    if (int rc = rank_mark_workspace(e, grow, l, sp, ep)) return rc;
    if (int rc = position_workspace(e, grow, n, m)) return rc;
    const RkGraph g = rank_graph(e, ep);
    const RkRule rule = rank_rule(sp);
    const PosWork w = pos_work(n, m);
    const RaLayout ra = ra_layout(m, n, 1);
    int *d_ids = reinterpret_cast<int *>(e->q.ra.buf + ra.off_ids);
    double *d_qs = reinterpret_cast<double *>(e->q.ra.buf + ra.off_a);
    if (m > 0) HIP_TRY(hipMemcpyAsync(d_ids, ids, sizeof(int) * (size_t)m, hipMemcpyHostToDevice, e->stream));
    if (int rc = DeviceTime{e}.open()) return rc;
    const unsigned *excl = nullptr;
    if (int rc = rank_mark_enqueue(e, l, sp, g, &excl)) return rc;
    HIP_TRY(hipMemsetAsync(ps.slots, 0, sizeof(unsigned) * w.slot_elems, e->stream));
    by_factor(sp, [&](auto kind, auto elem) -> int {
        using T = decltype(elem);
        hipLaunchKernelGGL((k_rk_scores<decltype(kind)::value, T>), dim3(tile_grid(st.rows)), dim3(TK_TILE_BLOCK), 0, e->stream, st,
                           e->d_int2ext.get(), excl, rule, g, sc.a.get(), sc.ext.get());
        if (m > 0)
            hipLaunchKernelGGL((k_rk_score_at<decltype(kind)::value, T>), dim3(grid_for((int64_t)m * n, RK_BLOCK)), dim3(RK_BLOCK), 0, e->stream,
                               v.p, v.gw, n, e->d_ext2int.get(), d_ids, m, excl, rule, g, d_qs);
        return DPPR_OK;
    });
    return position_finish(e, st.rows, n, min_score, m, out_pos, out_counts);
}

template <class Owner>
int position_call(dppr_engine *e, Owner &o, int32_t epoch, const dppr_rank_spec_t *spec, double min_score, const int32_t *ids, int32_t m,
                  int32_t *out_pos, int32_t *out_counts) {
    const StateView v = view(o);
    if (!position_args_ok(spec, min_score, ids, m, e->V, out_pos))
        return fail(e, DPPR_ERR_INVALID, "position_at: factor 0..3, factor_dtype 0 or 1, mask 0..2, exclude bits 1 | 2 | 4, min_score >= 0, m in [0, DPPR_POSITION_MAX], ids in [0, V), non-null ids / pos when m > 0");
    HIP_TRY(hipSetDevice(e->device));
    const Epoch *ep = nullptr;
    if (const char *why = rank_spec_refused(e, v, epoch, spec, &ep)) return fail(e, DPPR_ERR_INVALID, why);
    if (m == 0 && !out_counts) return DPPR_OK;
    std::lock_guard<std::mutex> map_lk(e->map_mu); // (as dppr_read: one state of the id space for the whole query)
    return run_position(e, v, rank_lanes(o), ep, rank_spec(spec), min_score, ids, m, out_pos, out_counts);
}

// ---- vertices drawn in proportion to a lane's score (dppr_sample.hpp, dppr_sample_plan.hpp) ---------------------------------------
// the leaves, the nodes, the low levels of the plain form, the block and its pinned twin: in place before the first kernel
int sample_workspace(dppr_engine *e, Grow &grow, int n, const SmTree &t, size_t blk_bytes) {
    QueryWork::Sample &sm = e->q.sm;
    int rc = grow(sm.leaves, sample_leaf_elems(n, t.Vt));
    if (!rc) rc = grow(sm.nodes, sample_node_elems(n, t));
    if (!rc && e->sample_form == 1) rc = grow(sm.low, sample_leaf_elems(n, t.Vt));
    if (!rc) rc = grow(sm.blk, blk_bytes);
    if (!rc) rc = grow(sm.pin, blk_bytes);
    return rc;
}

// the head of a call's result block
SmOut sample_head(dppr_engine *e, const SmLayout &lay) {
    QueryWork::Sample &sm = e->q.sm;
    return {reinterpret_cast<double *>(sm.blk + lay.off_total), reinterpret_cast<int *>(sm.blk + lay.off_support), reinterpret_cast<int *>(sm.blk + lay.off_status)};
}

// The back half of a sample call, from the written leaves and tiles' nodes of n lanes to the caller's arrays: the upper levels,
// the draws of the form in force, the one copy back. Its workspace is in place (sample_workspace), the head of the block is zeroed,
// the bracket is open.
int sample_finish(dppr_engine *e, int n, const SmTree &t, uint64_t seed, uint64_t first, int S, int dest, int32_t *out_ids, double *out_w,
                  double *out_total, int32_t *out_support, int32_t *out_status) {
    QueryWork::Sample &sm = e->q.sm;
    const bool host = dest == DPPR_DEST_HOST;
    const SmLayout lay = sample_layout(n, S, host, out_w != nullptr);
    const SmOut head = sample_head(e, lay);
    int *d_ids = host ? reinterpret_cast<int *>(sm.blk + lay.off_ids) : out_ids;
    double *d_w = !out_w ? nullptr : host ? reinterpret_cast<double *>(sm.blk + lay.off_w) : out_w;
    const bool plain = e->sample_form == 1;
    hipLaunchKernelGGL(k_sm_upper, dim3(n), dim3(SM_BLOCK), 0, e->stream, sm.nodes.get(), t, head);
    if (S > 0) {
        const int64_t total = (int64_t)n * S;
        if (plain)
            hipLaunchKernelGGL(k_sm_draw_plain, dim3((unsigned)sample_plain_blocks(total)), dim3(SM_BLOCK), 0, e->stream, sm.leaves.get(),
                               sm.nodes.get(), sm.low.get(), t, head.total, head.status, (int64_t)S, total, first, seed, d_ids, d_w);
        else
            hipLaunchKernelGGL(k_sm_draw, dim3((unsigned)sample_draw_blocks(total)), dim3(SM_BLOCK), 0, e->stream, sm.leaves.get(), sm.nodes.get(), t,
                               head.total, head.status, (int64_t)S, total, first, seed, d_ids, d_w);
    }
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_block(e, sm.blk, sm.pin, lay.total_bytes)) return rc; // (a device destination is complete here: any stream of the caller may read it)
    memcpy(out_total, sm.pin + lay.off_total, sizeof(double) * (size_t)n);
    if (out_support) memcpy(out_support, sm.pin + lay.off_support, sizeof(int32_t) * (size_t)n);
    memcpy(out_status, sm.pin + lay.off_status, sizeof(int32_t) * (size_t)n);
    if (host && S > 0) {
        memcpy(out_ids, sm.pin + lay.off_ids, sample_ids_bytes(n, S));
        if (out_w) memcpy(out_w, sm.pin + lay.off_w, sample_w_bytes(n, S));
    }
    return DPPR_OK;
}

// S draws of every lane by the spec's score, with the totals, supports and statuses (arguments, the spec's device pointers, the
// epoch and a device destination validated by the caller; S == 0: the tree alone). Every buffer is in place before the first
// kernel, every stage is enqueued before the one copy back: the marking of run_topk_ranked, the leaves and the tiles' nodes, the
// upper levels, the draws.
int run_sample(dppr_engine *e, const StateView &v, const RkLanes &l, const Epoch *ep, const RkSpec &sp, double min_score, uint64_t seed,
               uint64_t first, int S, int dest, int32_t *out_ids, double *out_w, double *out_total, int32_t *out_support, int32_t *out_status) {
    if (int rc = query_begin(e, MAP_E2I)) return rc;
    QueryWork::Sample &sm = e->q.sm;
    const int n = v.n;
    const bool host = dest == DPPR_DEST_HOST;
    const SmTree t = sample_tree(e->V);
    const SmLayout lay = sample_layout(n, S, host, out_w != nullptr);
    Grow grow{e};
    if (int rc = rank_mark_workspace(e, grow, l, sp, ep)) return rc;
    if (int rc = sample_workspace(e, grow, n, t, lay.total_bytes)) return rc;
    const RkGraph g = rank_graph(e, ep);
    const RkRule rule = rank_rule(sp);
    const SmOut head = sample_head(e, lay);
    const bool plain = e->sample_form == 1;
    if (int rc = DeviceTime{e}.open()) return rc;
    const unsigned *excl = nullptr;
    if (int rc = rank_mark_enqueue(e, l, sp, g, &excl)) return rc;
    HIP_TRY(hipMemsetAsync(sm.blk, 0, SM_HEAD_BYTES, e->stream));
    by_factor(sp, [&](auto kind, auto elem) -> int {
        using T = decltype(elem);
        hipLaunchKernelGGL((k_sm_leaves<decltype(kind)::value, T>), dim3(t.tiles), dim3(SM_BLOCK), 0, e->stream, v.p, v.gw, n, e->d_ext2int.get(),
                           excl, rule, g, min_score, t, sm.leaves.get(), sm.nodes.get(), plain ? sm.low.get() : nullptr, head.support);
        return DPPR_OK;
    });
    return sample_finish(e, n, t, seed, first, S, dest, out_ids, out_w, out_total, out_support, out_status);
}

template <class Owner>
int sample_call(dppr_engine *e, Owner &o, int32_t epoch, const dppr_rank_spec_t *spec, double min_score, uint64_t seed, uint64_t first, int32_t S,
                int dest, int32_t *out_ids, double *out_w, double *out_total, int32_t *out_support, int32_t *out_status) {
    const StateView v = view(o);
    if (!sample_args_ok(spec, min_score, v.n, first, S, dest, out_ids, out_total, out_status))
        return fail(e, DPPR_ERR_INVALID, "sample: factor 0..3, factor_dtype 0 or 1, mask 0..2, exclude bits 1 | 2 | 4, min_score >= 0, S in [0, DPPR_SAMPLE_MAX], n * S <= DPPR_SAMPLE_MAX_TOTAL, first + S without a wrap, dest 0 or 1, non-null ids when S > 0, non-null total / status");
    HIP_TRY(hipSetDevice(e->device));
    const Epoch *ep = nullptr;
    if (const char *why = rank_spec_refused(e, v, epoch, spec, &ep)) return fail(e, DPPR_ERR_INVALID, why);
    if (dest == DPPR_DEST_DEVICE && S > 0 &&
        (!dev_range_ok(e, out_ids, sample_ids_bytes(v.n, S), sizeof(int32_t)) || (out_w && !dev_range_ok(e, out_w, sample_w_bytes(v.n, S), sizeof(double)))))
        return fail(e, DPPR_ERR_INVALID, "sample: a device destination is aligned device memory of the engine's device, n * S elements inside one allocation");
    std::lock_guard<std::mutex> map_lk(e->map_mu); // (as dppr_read: one state of the id space for the whole query)
    return run_sample(e, v, rank_lanes(o), ep, rank_spec(spec), min_score, seed, first, S, dest, out_ids, out_w, out_total, out_support, out_status);
}

// ---- every vertex to its best lane, across groups (dppr_assign.hpp, dppr_assign_plan.hpp) --------------------------------------
static_assert(AS_TEAM_MAX * 2 == GS_MAX, "the widest row of a group is one step of the widest team");

// The groups of a call, looked up under the checks GET_GROUP makes, as the kernels' descriptors and the team that reads them.
// NULL: fine; otherwise the words of the rejection.
const char *assign_desc(dppr_engine *e, const int32_t *groups, int n_groups, AsDesc &d, int &team) {
    int n[AS_GROUPS_MAX], max_gw = 0;
    for (int i = 0; i < n_groups; ++i) {
        if (groups[i] < 0 || groups[i] >= (int)e->groups.size()) return "assign: bad group";
        n[i] = e->groups[(size_t)groups[i]].n;
    }
    const AsTable tb = as_table(n, n_groups);
    if (!tb.ok) return "assign: more than DPPR_ASSIGN_CLASSES_MAX classes";
    memset(&d, 0, sizeof(d));
    for (int i = 0; i < n_groups; ++i) {
        const Group &g = e->groups[(size_t)groups[i]];
        d.g[i] = AsGroup{g.p.get(), g.gw, g.n, tb.base[i]};
        max_gw = std::max(max_gw, g.gw);
    }
    d.n_groups = n_groups;
    d.C = tb.C;
    team = as_team(max_gw);
    return nullptr;
}

// One of the four instantiations of a kernel template <TEAM>: f(std::integral_constant<int, TEAM>())
template <class F> int by_team(int team, F &&f) {
    switch (team) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 4: return f(std::integral_constant<int, 4>());
    default: return f(std::integral_constant<int, 8>());
    }
}

struct AsCall { // (arguments, the groups and a device destination validated by the caller)
    AsDesc d;
    int team;
    const double *scale;
    double min_score;
    int dest;
    int32_t *out_label;
    double *out_best, *out_margin;
    int64_t *out_counts;
    const int32_t *prev;
    int64_t cap;
    int64_t *out_n_flips;
    int32_t *flip_id, *flip_old, *flip_new;
};

// Labels, best, margin, counts and flips of every external id. Every buffer is in place before anything is written; the flip
// positions are decided on the device and so is whether the fill runs: nothing is read back between the kernels; one copy brings
// the head -- and a host destination's arrays -- back. A host destination's prev_label goes into the label section and is updated there.
int run_assign(dppr_engine *e, const AsCall &c) {
    if (int rc = query_begin(e, MAP_E2I)) return rc;
    QueryWork::Assign &as = e->q.as;
    const int V = e->V;
    const bool host = c.dest == DPPR_DEST_HOST;
    const int64_t capc = c.prev ? as_cap_clamped(c.cap, V) : 0;
    const AsLayout lay = as_layout(V, capc, c.out_best != nullptr, c.out_margin != nullptr, host);
    const AsWork wk = as_workspace(V);
    Grow grow{e};
    int rc = grow(as.scale, wk.scale_elems);
    if (!rc) rc = grow(as.cnt, wk.cnt_elems);
    if (!rc) rc = grow(as.base, wk.base_elems);
    if (!rc) rc = grow(as.ws, wk.ws_elems);
    if (!rc) rc = grow(as.blk, lay.total_bytes);
    if (!rc) rc = grow(as.pin, lay.total_bytes);
    if (rc) return rc;
    unsigned char *blk = as.blk.get();
    AsHead *head = reinterpret_cast<AsHead *>(blk);
    int *d_label = host ? reinterpret_cast<int *>(blk + lay.off_label) : c.out_label;
    double *d_best = !c.out_best ? nullptr : host ? reinterpret_cast<double *>(blk + lay.off_best) : c.out_best;
    double *d_margin = !c.out_margin ? nullptr : host ? reinterpret_cast<double *>(blk + lay.off_margin) : c.out_margin;
    int *d_fid = host ? reinterpret_cast<int *>(blk + lay.off_fid) : c.flip_id;
    int *d_fold = host ? reinterpret_cast<int *>(blk + lay.off_fold) : c.flip_old;
    int *d_fnew = host ? reinterpret_cast<int *>(blk + lay.off_fnew) : c.flip_new;
    const int *d_prev = !c.prev ? nullptr : host ? d_label : c.prev;
    const double *d_scale = c.scale ? as.scale.get() : nullptr;
    if (c.scale) HIP_TRY(hipMemcpyAsync(as.scale, c.scale, sizeof(double) * (size_t)c.d.C, hipMemcpyHostToDevice, e->stream));
    if (host && c.prev) HIP_TRY(hipMemcpyAsync(d_label, c.prev, sizeof(int32_t) * (size_t)V, hipMemcpyHostToDevice, e->stream));
    const int tiles = (int)as_tiles(V), grid = std::min(tiles, 2048);
    if (int rc2 = DeviceTime{e}.open()) return rc2;
    HIP_TRY(hipMemsetAsync(head, 0, AS_HEAD_BYTES, e->stream));
    by_team(c.team, [&](auto team) -> int {
        hipLaunchKernelGGL((k_as_label<decltype(team)::value>), dim3(grid), dim3(AS_TILE), 0, e->stream, c.d, d_scale, c.min_score,
                           e->d_ext2int.get(), V, d_prev, d_label, d_best, d_margin, as.cnt.get(), as.ws.get(), wk.ws_plane,
                           reinterpret_cast<unsigned long long *>(head->counts));
        return DPPR_OK;
    });
    if (d_prev) {
        hipLaunchKernelGGL(k_as_scan, dim3(1), dim3(AS_TILE), 0, e->stream, as.cnt.get(), tiles, (long long)capc, as.base.get(), head);
        if (capc > 0)
            hipLaunchKernelGGL(k_as_fill, dim3(grid), dim3(AS_TILE), 0, e->stream, as.cnt.get(), as.base.get(), as.ws.get(), wk.ws_plane,
                               tiles, head, d_fid, d_fold, d_fnew);
    }
    HIP_TRY(hipGetLastError());
    if (int rc2 = fetch_block(e, as.blk, as.pin, lay.total_bytes)) return rc2; // (a device destination is complete here: any stream of the caller may read it)
    const AsHead *h = reinterpret_cast<const AsHead *>(as.pin.get());
    for (int i = 0; i <= c.d.C; ++i) c.out_counts[i] = h->counts[i];
    if (c.out_n_flips) *c.out_n_flips = h->n_flips;
    if (host) {
        memcpy(c.out_label, as.pin + lay.off_label, sizeof(int32_t) * (size_t)V);
        if (c.out_best) memcpy(c.out_best, as.pin + lay.off_best, sizeof(double) * (size_t)V);
        if (c.out_margin) memcpy(c.out_margin, as.pin + lay.off_margin, sizeof(double) * (size_t)V);
        if (capc > 0 && h->go && h->n_flips > 0) {
            const size_t bytes = sizeof(int32_t) * (size_t)h->n_flips;
            memcpy(c.flip_id, as.pin + lay.off_fid, bytes);
            memcpy(c.flip_old, as.pin + lay.off_fold, bytes);
            memcpy(c.flip_new, as.pin + lay.off_fnew, bytes);
        }
    }
    return DPPR_OK;
}

// the same values at m external ids (validated by the caller like the rest, m > 0)
int run_assign_at(dppr_engine *e, const AsDesc &d, int team, const double *scale, double min_score, const int32_t *ids, int m,
                  int32_t *out_label, double *out_best, int32_t *out_second_label, double *out_margin) {
    if (int rc = query_begin(e, MAP_E2I)) return rc;
    QueryWork::Assign &as = e->q.as;
    Grow grow{e};
    if (int rc = grow(as.scale, as_workspace(e->V).scale_elems)) return rc;
    if (int rc = grow(e->q.ra.buf, ra_layout(m, AS_AT_COLS, 2).total_bytes)) return rc;
    if (scale) HIP_TRY(hipMemcpyAsync(as.scale, scale, sizeof(double) * (size_t)d.C, hipMemcpyHostToDevice, e->stream));
    const double *d_scale = scale ? as.scale.get() : nullptr;
    std::vector<double> val((size_t)m * AS_AT_COLS), lab((size_t)m * AS_AT_COLS);
    const int rc = point_read(e, grow, ids, m, AS_AT_COLS, 2, val.data(), lab.data(), [&](const int *d_ids, double *d_val, double *d_lab) {
        return by_team(team, [&](auto tm) -> int {
            constexpr int T = decltype(tm)::value;
            hipLaunchKernelGGL((k_as_at<T>), dim3(grid_for((int64_t)m * T, AS_TILE)), dim3(AS_TILE), 0, e->stream, d, d_scale, min_score,
                               e->d_ext2int.get(), d_ids, m, d_val, reinterpret_cast<int *>(d_lab));
            return DPPR_OK;
        });
    });
    if (rc) return rc;
    const int32_t *li = reinterpret_cast<const int32_t *>(lab.data());
    for (int i = 0; i < m; ++i) {
        out_label[i] = li[4 * (size_t)i];
        if (out_second_label) out_second_label[i] = li[4 * (size_t)i + 1];
        if (out_best) out_best[i] = val[2 * (size_t)i];
        if (out_margin) out_margin[i] = val[2 * (size_t)i + 1];
    }
    return DPPR_OK;
}

int assign_call(dppr_engine *e, const int32_t *groups, int32_t n_groups, const double *scale, double min_score, int dest, int32_t *out_label,
                double *out_best, double *out_margin, int64_t *out_counts, const int32_t *prev_label, int64_t cap, int64_t *out_n_flips,
                int32_t *flip_id, int32_t *flip_old, int32_t *flip_new) {
    if (!e) return fail(e, DPPR_ERR_INVALID, "assign: no engine");
    if (e->broken) return fail(e, DPPR_ERR_INVALID, "engine unusable after a failed renumbering");
    if (const AsCheck ck = as_check(groups, n_groups, min_score, dest, out_label, out_counts, cap, flip_id, flip_old, flip_new))
        return fail(e, DPPR_ERR_INVALID, (std::string("assign: ") + as_check_text(ck)).c_str());
    AsCall c{};
    if (const char *why = assign_desc(e, groups, n_groups, c.d, c.team)) return fail(e, DPPR_ERR_INVALID, why);
    if (!as_scale_ok(scale, c.d.C)) return fail(e, DPPR_ERR_INVALID, (std::string("assign: ") + as_check_text(AS_BAD_SCALE)).c_str());
    HIP_TRY(hipSetDevice(e->device));
    if (dest == DPPR_DEST_DEVICE) {
        const size_t V = (size_t)e->V, capc = (size_t)as_cap_clamped(cap, e->V);
        bool ok = dev_range_ok(e, out_label, sizeof(int32_t) * V, sizeof(int32_t)) &&
                  (!out_best || dev_range_ok(e, out_best, sizeof(double) * V, sizeof(double))) &&
                  (!out_margin || dev_range_ok(e, out_margin, sizeof(double) * V, sizeof(double))) &&
                  (!prev_label || dev_range_ok(e, prev_label, sizeof(int32_t) * V, sizeof(int32_t)));
        if (ok && capc > 0)
            ok = dev_range_ok(e, flip_id, sizeof(int32_t) * capc, sizeof(int32_t)) && dev_range_ok(e, flip_old, sizeof(int32_t) * capc, sizeof(int32_t)) &&
                 dev_range_ok(e, flip_new, sizeof(int32_t) * capc, sizeof(int32_t));
        if (!ok)
            return fail(e, DPPR_ERR_INVALID, "assign: label / best / margin / prev_label / flip lists must be aligned device memory of the engine's device, V (the lists: cap) entries inside one allocation");
    }
    c.scale = scale, c.min_score = min_score, c.dest = dest;
    c.out_label = out_label, c.out_best = out_best, c.out_margin = out_margin, c.out_counts = out_counts;
    c.prev = prev_label, c.cap = cap, c.out_n_flips = out_n_flips;
    c.flip_id = flip_id, c.flip_old = flip_old, c.flip_new = flip_new;
    std::lock_guard<std::mutex> map_lk(e->map_mu); // (as dppr_read: one state of the id space for the whole query)
    return run_assign(e, c);
}

int assign_at_call(dppr_engine *e, const int32_t *groups, int32_t n_groups, const double *scale, double min_score, const int32_t *ids, int32_t m,
                   int32_t *out_label, double *out_best, int32_t *out_second_label, double *out_margin) {
    if (!e) return fail(e, DPPR_ERR_INVALID, "assign_at: no engine");
    if (e->broken) return fail(e, DPPR_ERR_INVALID, "engine unusable after a failed renumbering");
    if (const AsCheck ck = as_at_check(groups, n_groups, min_score, ids, m, e->V, out_label))
        return fail(e, DPPR_ERR_INVALID, (std::string("assign_at: ") + as_check_text(ck)).c_str());
    AsDesc d;
    int team = 1;
    if (const char *why = assign_desc(e, groups, n_groups, d, team)) return fail(e, DPPR_ERR_INVALID, why);
    if (!as_scale_ok(scale, d.C)) return fail(e, DPPR_ERR_INVALID, (std::string("assign_at: ") + as_check_text(AS_BAD_SCALE)).c_str());
    if (m == 0) return DPPR_OK;
    std::lock_guard<std::mutex> map_lk(e->map_mu);
    return run_assign_at(e, d, team, scale, min_score, ids, m, out_label, out_best, out_second_label, out_margin);
}

// ---- explain a score: top contributors and the path to the seeds (dppr_explain.hpp, dppr_explain_plan.hpp) -------------------------
// Contributors and paths of m external ids in every lane (arguments and the epoch validated by the caller, m > 0, `which` names at
// least one output). Every buffer is in place before the first kernel -- the block, its pinned twin and, with the memo on, the
// first plane of the scratch state of the ranked family -- and both kernels are enqueued before the one copy back.
int run_explain(dppr_engine *e, const StateView &v, const RkLanes &l, const Epoch &ep, const int32_t *ids, int m, int f, int depth,
                uint32_t which, const dppr_explain_out_t &out) {
    if (int rc = query_begin(e, MAP_E2I | MAP_I2E)) return rc;
    QueryWork::Explain &xq = e->q.exq;
    const int n = v.n;
    const ExplainLayout lay = ex_layout(m, n, f, depth, which);
    const bool memo = ex_memo_on(m, n, depth, which, e->ex_memo);
    const size_t memo_elems = ex_memo_elems((size_t)e->n_int, n);
    Grow grow{e};
    int rc = grow(xq.blk, lay.total_bytes);
    if (!rc) rc = grow(xq.pin, lay.total_bytes);
    if (!rc && memo) rc = grow(e->q.sc.a, memo_elems, with_slack(memo_elems));
    if (rc) return rc;
    unsigned char *blk = xq.blk.get();
    auto ints = [&](uint32_t bit, size_t off) { return (which & bit) ? reinterpret_cast<int *>(blk + off) : nullptr; };
    auto dbls = [&](uint32_t bit, size_t off) { return (which & bit) ? reinterpret_cast<double *>(blk + off) : nullptr; };
    int *d_ids = reinterpret_cast<int *>(blk + lay.off_ids);
    const ExIn in{v.p, v.gw, n, e->d_ext2int.get(), e->d_int2ext.get(), d_ids, m, rank_graph(e, &ep), l};
    const ExFirstOut fo{ints(EX_DEG, lay.off_deg),     ints(EX_DISTINCT, lay.off_distinct), dbls(EX_SELF, lay.off_self), ints(EX_NBR_COUNT, lay.off_nbr_count),
                        ints(EX_NBR, lay.off_nbr),     ints(EX_NBR_MULT, lay.off_nbr_mult), dbls(EX_NBR_C, lay.off_nbr_c)};
    const ExPathOut po{ints(EX_LEN, lay.off_len), ints(EX_END, lay.off_end), ints(EX_PATH, lay.off_path), dbls(EX_PATH_P, lay.off_path_p),
                       dbls(EX_PATH_C, lay.off_path_c)};
    HIP_TRY(hipMemcpyAsync(d_ids, ids, sizeof(int) * (size_t)m, hipMemcpyHostToDevice, e->stream));
    if (int rc2 = DeviceTime{e}.open()) return rc2;
    const dim3 grid((unsigned)ex_grid(m, n)), block(EX_BLOCK);
    if (which & EX_FIRST) hipLaunchKernelGGL(k_ex_first, grid, block, 0, e->stream, in, f, e->ex_wave_rows, fo);
    if (which & EX_WALK) {
        unsigned long long *d_memo = memo ? reinterpret_cast<unsigned long long *>(e->q.sc.a.get()) : nullptr;
        if (memo) HIP_TRY(hipMemsetAsync(d_memo, 0xff, sizeof(unsigned long long) * memo_elems, e->stream)); // (every entry: unknown)
        hipLaunchKernelGGL(k_ex_path, grid, block, 0, e->stream, in, depth, e->ex_wave_rows, d_memo, po);
    }
    HIP_TRY(hipGetLastError());
    if (int rc2 = fetch_block(e, xq.blk, xq.pin, lay.copy_bytes)) return rc2;
    const size_t mn = (size_t)m * (size_t)n;
    auto back = [&](uint32_t bit, void *dst, size_t off, size_t bytes) {
        if (which & bit) memcpy(dst, xq.pin + off, bytes);
    };
    back(EX_DEG, out.deg, lay.off_deg, sizeof(int32_t) * (size_t)m);
    back(EX_DISTINCT, out.distinct, lay.off_distinct, sizeof(int32_t) * (size_t)m);
    back(EX_SELF, out.self, lay.off_self, sizeof(double) * mn);
    back(EX_NBR_COUNT, out.nbr_count, lay.off_nbr_count, sizeof(int32_t) * mn);
    back(EX_NBR, out.nbr, lay.off_nbr, sizeof(int32_t) * mn * (size_t)f);
    back(EX_NBR_MULT, out.nbr_mult, lay.off_nbr_mult, sizeof(int32_t) * mn * (size_t)f);
    back(EX_NBR_C, out.nbr_c, lay.off_nbr_c, sizeof(double) * mn * (size_t)f);
    back(EX_LEN, out.len, lay.off_len, sizeof(int32_t) * mn);
    back(EX_END, out.end, lay.off_end, sizeof(int32_t) * mn);
    back(EX_PATH, out.path, lay.off_path, sizeof(int32_t) * mn * ((size_t)depth + 1));
    back(EX_PATH_P, out.path_p, lay.off_path_p, sizeof(double) * mn * ((size_t)depth + 1));
    back(EX_PATH_C, out.path_c, lay.off_path_c, sizeof(double) * mn * (size_t)depth);
    return DPPR_OK;
}

// (Owner: a Slot or a Group. Its seeds are read under map_mu: a renumbering beside the call renames them)
template <class Owner>
int explain_call(dppr_engine *e, Owner &o, int32_t epoch, const int32_t *ids, int32_t m, int32_t f, int32_t depth, const dppr_explain_out_t *out) {
    const StateView v = view(o);
    if (!ex_args_ok(ids, m, f, depth, e->V, out))
        return fail(e, DPPR_ERR_INVALID, "explain_at: m in [0, DPPR_EXPLAIN_MAX_M], f in [0, DPPR_EXPLAIN_MAX_F], depth in [0, DPPR_EXPLAIN_MAX_DEPTH], f + depth >= 1, ids in [0, V), non-null ids / out when m > 0");
    const Epoch *ep = find_epoch(e, epoch);
    if (!ep) return fail(e, DPPR_ERR_INVALID, "explain_at: epoch not resident (evicted or never built)");
    if (!refine_epoch_ok(v.st.last_epoch, ep->id))
        return fail(e, DPPR_ERR_INVALID, "explain_at: the state stands on another epoch than the one given: the out-edges of another graph do not decompose its scores");
    const uint32_t which = ex_which(out, f, depth);
    if (m == 0 || !which) return DPPR_OK;
    std::lock_guard<std::mutex> map_lk(e->map_mu); // (as dppr_read: one state of the id space for the whole query)
    return run_explain(e, v, rank_lanes(o), *ep, ids, m, f, depth, which, *out);
}

// ---- the certificate of a state: residual norms and the loop invariant (dppr_certify.hpp, dppr_certify_plan.hpp) ----------------
// The parts `which` names (arguments and the epoch validated by the caller, at least one output). Every buffer is in place before
// the first kernel -- the block, its pinned twin, the head and the partials, and for the invariant the queue of pieces, their
// partials and the first plane of the scratch state of the ranked family for S -- and every kernel is enqueued before the one
// copy back.
int run_certify(dppr_engine *e, const StateView &v, const RkLanes &l, const Epoch &ep, double eps, uint32_t which, dppr_certify_out_t &out) {
    if (int rc = query_begin(e, MAP_E2I)) return rc;
    QueryWork::Certify &cq = e->q.cert;
    const int n = v.n, gw = v.gw, V = e->V;
    const bool res = (which & CERT_RES) != 0, inv = (which & CERT_INV) != 0;
    const CertLayout lay = cert_layout(n, which);
    const CertWork wk = cert_work();
    const int piece = cert_piece(e->cert_piece), wave_rows = cert_wave_rows(gw, e->cert_wave_rows);
    const size_t part_elems = cert_part_elems(V, n), s_elems = scratch_plane_elems((size_t)e->n_int, gw);
    const size_t cap = cert_list_cap(ep.Ed, piece);
    Grow grow{e};
    int rc = grow(cq.blk, lay.total_bytes);
    if (!rc) rc = grow(cq.pin, lay.total_bytes);
    if (!rc) rc = grow(cq.ws, wk.bytes);
    if (!rc && res) rc = grow(cq.part, part_elems);
    if (!rc && inv) rc = grow(e->q.sc.a, s_elems, with_slack(s_elems));
    if (!rc && inv) rc = grow(cq.list, cap);
    if (!rc && inv) rc = grow(cq.pp, cap * (size_t)gw);
    if (rc) return rc;
    unsigned char *blk = cq.blk.get();
    CertHead *head = reinterpret_cast<CertHead *>(cq.ws + wk.off_head);
    double *sums = reinterpret_cast<double *>(cq.ws + wk.off_sums);
    CertMax *max_r = reinterpret_cast<CertMax *>(cq.ws + wk.off_max_r), *max_inv = reinterpret_cast<CertMax *>(cq.ws + wk.off_max_inv);
    auto dbls = [&](uint32_t bit, size_t off) { return (which & bit) ? reinterpret_cast<double *>(blk + off) : nullptr; };
    auto i64s = [&](uint32_t bit, size_t off) { return (which & bit) ? reinterpret_cast<long long *>(blk + off) : nullptr; };
    auto ints = [&](uint32_t bit, size_t off) { return (which & bit) ? reinterpret_cast<int *>(blk + off) : nullptr; };
    const CertOut co{dbls(CERT_MAX_R, lay.off_max_r),      dbls(CERT_SUM_R, lay.off_sum_r),  dbls(CERT_SUM_P, lay.off_sum_p),
                     dbls(CERT_INV_ERR, lay.off_inv_err),  i64s(CERT_N_POS, lay.off_n_pos),  i64s(CERT_N_NEG, lay.off_n_neg),
                     i64s(CERT_N_NONFINITE, lay.off_n_nonfinite), i64s(CERT_N_P_NONZERO, lay.off_n_p_nonzero),
                     ints(CERT_ARGMAX_R, lay.off_argmax_r), ints(CERT_INV_ARG, lay.off_inv_arg)};
    const int *x2i = e->d_ext2int.get();
    const dim3 block(CERT_BLOCK);
    int nwg_r = 0, nwg_inv = 0;
    if (int rc2 = DeviceTime{e}.open()) return rc2;
    HIP_TRY(hipMemsetAsync(head, 0, sizeof(CertHead), e->stream));
    if (res) {
        const long long stride = dot_cols(V) > 0 ? dot_cols(V) : DOT_TPB;
        nwg_r = cert_stream_grid(V);
        HIP_TRY(hipMemsetAsync(cq.part, 0, sizeof(double) * part_elems, e->stream)); // (+0.0: the tiles of padding)
        hipLaunchKernelGGL(k_cert_residual, dim3((unsigned)nwg_r), block, dot_lds_bytes(n, 1), e->stream, v.p, v.r, gw, n, x2i, V, eps,
                           cq.part.get(), stride, head, max_r);
        hipLaunchKernelGGL(k_dot_combine, dim3((2 * n + DOT_CB_WAVES - 1) / DOT_CB_WAVES), dim3(DOT_CB_WAVES * WAVE), 0, e->stream,
                           cq.part.get(), (const long long *)nullptr, stride, 2 * n, n, &head->dot, sums);
    }
    if (inv) {
        const CertGraph g{ep.out_row_ptr.get(), ep.out_col.get(), e->n_int, V};
        double *S = e->q.sc.a.get();
        const unsigned ucap = (unsigned)std::min<size_t>(cap, 0xffffffffu);
        const int rows_per_wg = CERT_BLOCK / cert_lane_stride(n);
        nwg_inv = (int)std::max<long long>(1, std::min<long long>(((long long)V + rows_per_wg - 1) / rows_per_wg, CERT_GRID_MAX));
        hipLaunchKernelGGL(k_cert_rows, dim3((unsigned)cert_rows_grid(e->n_int, wave_rows)), block, 0, e->stream, v.p, gw, g, piece, wave_rows, S,
                           head, cq.list.get(), ucap);
        hipLaunchKernelGGL(k_cert_pieces, dim3((unsigned)std::min<size_t>((cap + CERT_WAVES - 1) / CERT_WAVES, 4096)), block, 0, e->stream, v.p,
                           gw, g, piece, head, cq.list.get(), ucap, cq.pp.get());
        hipLaunchKernelGGL(k_cert_long, dim3((unsigned)std::min<size_t>((cap * (size_t)gw + CERT_BLOCK - 1) / CERT_BLOCK, 4096)), block, 0,
                           e->stream, gw, g, piece, head, cq.list.get(), ucap, cq.pp.get(), S);
        hipLaunchKernelGGL(k_cert_err, dim3((unsigned)nwg_inv), block, 0, e->stream, v.p, v.r, gw, n, x2i, V, g, l, S, max_inv);
    }
    hipLaunchKernelGGL(k_cert_finish, dim3((unsigned)n), dim3(WAVE), 0, e->stream, head, sums, n, max_r, nwg_r, max_inv, nwg_inv, co);
    HIP_TRY(hipGetLastError());
    if (int rc2 = fetch_block(e, cq.blk, cq.pin, lay.copy_bytes)) return rc2;
    auto back = [&](uint32_t bit, void *dst, size_t off, size_t elem_bytes) {
        if (which & bit) memcpy(dst, cq.pin + off, elem_bytes * (size_t)n);
    };
    back(CERT_MAX_R, out.max_abs_r, lay.off_max_r, sizeof(double));
    back(CERT_SUM_R, out.sum_abs_r, lay.off_sum_r, sizeof(double));
    back(CERT_SUM_P, out.sum_p, lay.off_sum_p, sizeof(double));
    back(CERT_INV_ERR, out.inv_max_err, lay.off_inv_err, sizeof(double));
    back(CERT_N_POS, out.n_pos, lay.off_n_pos, sizeof(int64_t));
    back(CERT_N_NEG, out.n_neg, lay.off_n_neg, sizeof(int64_t));
    back(CERT_N_NONFINITE, out.n_nonfinite, lay.off_n_nonfinite, sizeof(int64_t));
    back(CERT_N_P_NONZERO, out.n_p_nonzero, lay.off_n_p_nonzero, sizeof(int64_t));
    back(CERT_ARGMAX_R, out.argmax_r, lay.off_argmax_r, sizeof(int32_t));
    back(CERT_INV_ARG, out.inv_argmax, lay.off_inv_arg, sizeof(int32_t));
    return DPPR_OK;
}

// (Owner: a Slot or a Group. Its seeds are read under map_mu: a renumbering beside the call renames them)
template <class Owner>
int certify_call(dppr_engine *e, Owner &o, int32_t epoch, double eps, int flags, dppr_certify_out_t *out) {
    const StateView v = view(o);
    if (!cert_args_ok(eps, flags, out))
        return fail(e, DPPR_ERR_INVALID, "certify: non-null out, flags DPPR_CERT_RESIDUAL | DPPR_CERT_INVARIANT (1 .. 3), eps > 0");
    const Epoch *ep = find_epoch(e, epoch);
    if (!ep) return fail(e, DPPR_ERR_INVALID, "certify: epoch not resident (evicted or never built)");
    out->state_epoch = v.st.last_epoch;
    out->converged = v.st.converged ? 1 : 0;
    out->conv_eps = v.st.conv_eps;
    const uint32_t which = cert_which(out, flags);
    if (!which) return DPPR_OK;
    std::lock_guard<std::mutex> map_lk(e->map_mu); // (as dppr_read: one state of the id space for the whole query)
    return run_certify(e, v, rank_lanes(o), *ep, eps, which, *out);
}

// ---- the forward sweep of any vertex (dppr_forward.hpp, dppr_forward_plan.hpp) -----------------------------------------------------
// One of the four instantiations of a sweep kernel template <PP, LEVELS>: f(pieces of a row per lane, levels of the counter)
template <class F> int by_fw_shape(int lane_pieces, int levels, F &&f) {
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using LS = std::integral_constant<int, FW_LEVELS_SHORT>;
    using LL = std::integral_constant<int, FW_LEVELS_LONG>;
    if (lane_pieces == 1) return levels == FW_LEVELS_SHORT ? f(I1(), LS()) : f(I1(), LL());
    return levels == FW_LEVELS_SHORT ? f(I2(), LS()) : f(I2(), LL());
}

// The sweeps and the parts `which` names (arguments, ids, a device destination and the epoch validated by the caller). Every buffer
// is in place before the first kernel. Per chunk the host enqueues up to 8 sweeps, the rem fold and the freeze update and reads
// back the freeze word; the whole head comes back once, after the last chunk.
int run_forward(dppr_engine *e, const Epoch &ep, const int32_t *starts, int m, int iters, double tol, uint32_t which,
                const dppr_forward_out_t &out) {
    if (int rc = query_begin(e, MAP_E2I | ((which & FW_TOPK) ? MAP_I2E : 0u))) return rc;
    QueryWork::Forward &fq = e->q.fw;
    const int V = e->V, gw = fw_row_width(m);
    const int piece = fw_piece(e->fw_piece), T = fw_team(gw, e->fw_team), PP = fw_lane_pieces(gw, T), levels = fw_levels(piece);
    const size_t plane = fw_plane_elems(V, gw), part_elems = fw_part_elems(V, m);
    const size_t item_cap = fw_item_cap(ep.Ed, piece), long_cap = fw_long_cap(ep.Ed, piece);
    const long long stride = fw_part_stride(V);
    Grow grow{e};
    int rc = grow(fq.planes, 4 * plane);
    if (!rc) rc = grow(fq.head, sizeof(FwHead));
    if (!rc) rc = grow(fq.pin, sizeof(FwHead));
    if (!rc) rc = grow(fq.part, part_elems);
    if (!rc) rc = grow(fq.items, item_cap);
    if (!rc) rc = grow(fq.longs, sizeof(FwLong) * long_cap);
    if (!rc) rc = grow(fq.pp, item_cap * (size_t)gw);
    if (!rc && (which & FW_TOPK)) rc = topk_workspace(e, grow, m, (size_t)(e->n_int + e->n_parked));
    if (!rc && (which & FW_AT)) rc = grow(e->q.ra.buf, ra_layout(out.n_at, m, 2).total_bytes);
    if (rc) return rc;
    double *y = fq.planes.get(), *yn = y + plane, *f = yn + plane, *x = f + plane;
    FwHead *head = reinterpret_cast<FwHead *>(fq.head.get());
    const FwHead *pin = reinterpret_cast<const FwHead *>(fq.pin.get());
    FwLong *longs = reinterpret_cast<FwLong *>(fq.longs.get());
    const unsigned icap = (unsigned)std::min<size_t>(item_cap, 0xffffffffu), lcap = (unsigned)std::min<size_t>(long_cap, 0xffffffffu);
    const FwGraph g{ep.row_ptr.get(), ep.adj.get(), ep.out_row_ptr.get(), e->n_int, V};
    const int *x2i = e->d_ext2int.get();
    const dim3 block(FW_BLOCK);
    const dim3 rows_grid((unsigned)fw_units_grid(e->n_int, T)), piece_grid((unsigned)fw_units_grid((long long)std::min<size_t>(item_cap, 1u << 20), T));
    const dim3 long_grid((unsigned)grid_for((int64_t)std::min<size_t>(long_cap, 1u << 16) * m, FW_BLOCK, 1024));

    HIP_TRY(hipMemsetAsync(head, 0, sizeof(FwHead), e->stream));
    HIP_TRY(hipMemcpyAsync(head->starts, starts, sizeof(int) * (size_t)m, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemsetAsync(fq.planes, 0, sizeof(double) * 4 * plane, e->stream));
    HIP_TRY(hipMemsetAsync(fq.part, 0, sizeof(double) * part_elems, e->stream)); // (+0.0: the tiles of padding)
    if (int rc2 = DeviceTime{e}.open()) return rc2;
    hipLaunchKernelGGL(k_fw_init, dim3(1), dim3(WAVE), 0, e->stream, head, m, iters, x2i, g, y, f, gw);
    hipLaunchKernelGGL(k_fw_list, dim3((unsigned)grid_for(e->n_int, FW_BLOCK, 1024)), block, 0, e->stream, g, piece, head, fq.items.get(), icap,
                       longs, lcap);
    HIP_TRY(hipGetLastError());
    unsigned frozen = 0;
    for (int k = 0; k < iters && (frozen & fw_all(m)) != fw_all(m);) {
        const int end = fw_next_check(k, iters);
        for (++k; k <= end; ++k) {
            const FwPlanes pl{y, yn, f, x, gw, m, k == end ? 1 : 0};
            by_fw_shape(PP, levels, [&](auto pp_c, auto lv_c) -> int {
                constexpr int P = decltype(pp_c)::value, L = decltype(lv_c)::value;
                hipLaunchKernelGGL((k_fw_sweep<P, L>), rows_grid, block, 0, e->stream, g, pl, T, piece, head);
                hipLaunchKernelGGL((k_fw_pieces<P, L>), piece_grid, block, 0, e->stream, g, pl.y, gw, m, T, piece, head, fq.items.get(), icap,
                                   fq.pp.get());
                return DPPR_OK;
            });
            hipLaunchKernelGGL(k_fw_long, long_grid, block, 0, e->stream, g, pl, piece, head, longs, lcap, fq.pp.get());
            std::swap(y, yn);
        }
        k = end;
        hipLaunchKernelGGL(k_fw_rem, dim3((unsigned)fw_rem_grid(V)), block, dot_lds_bytes(gw, 1), e->stream, x, gw, m, x2i, V, fq.part.get(), stride);
        hipLaunchKernelGGL(k_dot_combine, dim3((m + DOT_CB_WAVES - 1) / DOT_CB_WAVES), dim3(DOT_CB_WAVES * WAVE), 0, e->stream, fq.part.get(),
                           (const long long *)nullptr, stride, m, m, &head->dot, head->cur);
        hipLaunchKernelGGL(k_fw_check, dim3(1), dim3(WAVE), 0, e->stream, head, m, k, tol, k == iters ? 1 : 0);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(fq.pin, head, sizeof(unsigned), hipMemcpyDeviceToHost, e->stream)); // THE word of the chunk
        HIP_TRY(loop_wait(e));
        frozen = pin->frozen;
    }
    if (int rc2 = DeviceTime{e}.close()) return rc2;
    HIP_TRY(hipMemcpyAsync(fq.pin, head, sizeof(FwHead), hipMemcpyDeviceToHost, e->stream));
    if (int rc2 = run_end(e)) return rc2;
    const float sweep_ms = e->query_ms;
    if (pin->overflow) return fail(e, DPPR_ERR_HIP, "forward: the list of the long rows' pieces was too short (fw_item_cap)");
    const FwHead hd = *pin; // (the parts below reuse nothing of it, but the pinned twin is the engine's)
    if (out.iters_used) memcpy(out.iters_used, hd.iters_used, sizeof(int32_t) * (size_t)m);
    if (out.rem) memcpy(out.rem, hd.rem, sizeof(double) * (size_t)m);

    if (which & FW_DENSE) {
        const bool sm = out.dense_layout == DPPR_SOURCE_MAJOR;
        const dim3 grid(sm ? std::min((int)ex_tiles(V), 2048) : grid_for((int64_t)V * m, EX_TILE));
        by_dtype_layout(out.dense_dtype, sm, [&](auto elem, auto source_major) -> int {
            using E = decltype(elem);
            hipLaunchKernelGGL((k_ex_dense<E, decltype(source_major)::value>), grid, dim3(EX_TILE), 0, e->stream, f, gw, m, x2i, V,
                               static_cast<E *>(out.dense_dev));
            for (int c = 0; c < m; ++c)
                if (hd.rowless[c])
                    hipLaunchKernelGGL(k_fw_poke<E>, dim3(1), dim3(WAVE), 0, e->stream, static_cast<E *>(out.dense_dev),
                                       (long long)ex_dense_index(out.dense_layout, m, V, starts[c], c));
            return DPPR_OK;
        });
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(e->stream)); // (the destination is complete here: any stream of the caller may read it)
    }
    if (which & FW_AT) {
        const int n_at = out.n_at;
        if (int rc2 = point_read(e, grow, out.at_ids, n_at, m, 2, out.at_f, nullptr, [&](const int *d_ids, double *d_a, double *d_b) {
                hipLaunchKernelGGL(k_read_at, dim3(grid_for((int64_t)n_at * m)), dim3(BLOCK), 0, e->stream, f, f, gw, m, x2i, d_ids, n_at, d_a, d_b);
                return DPPR_OK;
            }))
            return rc2;
        for (int c = 0; c < m; ++c)
            if (hd.rowless[c])
                for (int j = 0; j < n_at; ++j)
                    if (out.at_ids[j] == starts[c]) out.at_f[(size_t)j * m + c] = FW_ALPHA;
    }
    if (which & FW_TOPK) {
        const TkState st = tk_state(e, f, f, gw, m);
        if (int rc2 = run_select(e, st, e->d_int2ext, out.k, out.min_f, out.topk_ids, out.topk_f, nullptr, out.topk_counts)) return rc2;
        for (int c = 0; c < m; ++c)
            if (hd.rowless[c] && FW_ALPHA > out.min_f) { // (the column holds nothing else)
                out.topk_counts[c] = 1;
                out.topk_ids[(size_t)c * out.k] = starts[c];
                out.topk_f[(size_t)c * out.k] = FW_ALPHA;
            }
    }
    if (e->profiling) e->query_ms = sweep_ms; // (the parts opened brackets of their own)
    return DPPR_OK;
}

int forward_call(dppr_engine *e, int32_t epoch, const int32_t *starts, int32_t m, int32_t iters, double tol, const dppr_forward_out_t *out) {
    if (!fw_args_ok(starts, m, iters, tol, out))
        return fail(e, DPPR_ERR_INVALID, "forward: m in [1, 16], iters in [1, 256], tol >= 0 and finite, non-null starts / out");
    if (!fw_parts_ok(out))
        return fail(e, DPPR_ERR_INVALID,
                    "forward: a part asked for needs all its pointers; k in [1, DPPR_TOPK_MAX], min_f >= 0; n_at in [1, DPPR_FORWARD_AT_MAX]; dtype 0 or 1, layout 0 or 1");
    const uint32_t which = fw_which(out);
    if (!dppr::ids_in_range(starts, m, e->V)) return fail(e, DPPR_ERR_INVALID, "forward: starts in [0, V)");
    if ((which & FW_AT) && !dppr::ids_in_range(out->at_ids, out->n_at, e->V)) return fail(e, DPPR_ERR_INVALID, "forward: at_ids in [0, V)");
    const Epoch *ep = find_epoch(e, epoch);
    if (!ep) return fail(e, DPPR_ERR_INVALID, "forward: epoch not resident (evicted or never built)");
    HIP_TRY(hipSetDevice(e->device));
    if ((which & FW_DENSE) && !dev_range_ok(e, out->dense_dev, ex_dense_bytes(out->dense_dtype, m, e->V), ex_elem_bytes(out->dense_dtype)))
        return fail(e, DPPR_ERR_INVALID, "forward: dense_dev must be aligned device memory of the engine's device, m x V elements inside one allocation");
    if (!which) return DPPR_OK;
    std::lock_guard<std::mutex> map_lk(e->map_mu); // (as dppr_read: one state of the id space for the whole call)
    return run_forward(e, *ep, starts, m, iters, tol, which, *out);
}

// ---- the forward push from weighted start sets (dppr_fpush.hpp, dppr_fpush_plan.hpp) -----------------------------------------------
// The rounds and the parts `which` names (arguments, the CSR, ids, device destinations and the epoch validated by the caller).
// Every buffer is in place before the first kernel. Per chunk the host enqueues a few rounds -- select, mark, gather, the pieces
// of the long receivers and their sums -- and reads back ONE word: the columns that pushed in the chunk's last round.
int run_fpush(dppr_engine *e, const Epoch &ep, const int64_t *offsets, const int32_t *ids, const double *weights, int m, double eps, int max_rounds,
              uint32_t which, const dppr_forward_push_out_t &out) {
    if (int rc = query_begin(e, MAP_E2I | ((which & FP_TOPK) ? MAP_I2E : 0u))) return rc;
    QueryWork::Forward &fq = e->q.fw;
    const int V = e->V, gw = fw_row_width(m), n_seeds = (int)offsets[m];
    const int piece = fw_piece(e->fp_piece), T = fw_team(gw, e->fp_team), PP = fw_lane_pieces(gw, T), levels = fw_levels(piece);
    const int chunk = fp_chunk(e->fp_chunk);
    const size_t plane = fw_plane_elems(V, gw), part_elems = fw_part_elems(V, m);
    const size_t item_cap = fw_item_cap(ep.Ed, piece), long_cap = fw_long_cap(ep.Ed, piece);
    const size_t list_cap = fp_list_cap(V), mark_cap = fp_mark_cap(V, ep.Ed), words = fp_bitmap_words(V);
    const long long stride = fw_part_stride(V);
    Grow grow{e};
    int rc = grow(fq.planes, 4 * plane);
    if (!rc) rc = grow(fq.fp_head, sizeof(FpHead));
    if (!rc) rc = grow(fq.fp_pin, sizeof(FpHead));
    if (!rc) rc = grow(fq.fp_seeds, sizeof(FpSeed) * (size_t)n_seeds);
    if (!rc) rc = grow(fq.fp_seeds_pin, sizeof(FpSeed) * (size_t)n_seeds);
    if (!rc) rc = grow(fq.fp_lists, 4 * list_cap);
    if (!rc) rc = grow(fq.fp_bits, words);
    if (!rc) rc = grow(fq.fp_mark, mark_cap);
    if (!rc) rc = grow(fq.part, part_elems);
    if (!rc) rc = grow(fq.items, item_cap);
    if (!rc) rc = grow(fq.longs, sizeof(FwLong) * long_cap);
    if (!rc) rc = grow(fq.pp, item_cap * (size_t)gw);
    if (!rc && (which & FP_TOPK)) rc = topk_workspace(e, grow, m, (size_t)(e->n_int + e->n_parked));
    if (!rc && (which & FP_AT)) rc = grow(e->q.ra.buf, ra_layout(out.n_at, m, 2).total_bytes);
    if (rc) return rc;
    double *p = fq.planes.get(), *r = p + plane, *y[2] = {r + plane, r + 2 * plane};
    FpHead *head = reinterpret_cast<FpHead *>(fq.fp_head.get());
    const FpHead *pin = reinterpret_cast<const FpHead *>(fq.fp_pin.get());
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

    for (int c = 0; c < m; ++c)
        for (int64_t j = offsets[c]; j < offsets[c + 1]; ++j) h_seeds[j] = FpSeed{ids[j], c, weights[j], -1, 0};
    HIP_TRY(hipMemsetAsync(head, 0, sizeof(FpHead), e->stream));
    HIP_TRY(hipMemcpyAsync(seeds, h_seeds, sizeof(FpSeed) * (size_t)n_seeds, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemsetAsync(fq.planes, 0, sizeof(double) * 4 * plane, e->stream));
    HIP_TRY(hipMemsetAsync(fq.fp_bits, 0, sizeof(unsigned) * words, e->stream));
    HIP_TRY(hipMemsetAsync(fq.part, 0, sizeof(double) * part_elems, e->stream)); // (+0.0: the tiles of padding)
    if (int rc2 = DeviceTime{e}.open()) return rc2;
    hipLaunchKernelGGL(k_fp_init, dim3((unsigned)grid_for(n_seeds, FW_BLOCK, FP_GRID_MAX)), block, 0, e->stream, head, seeds, n_seeds, x2i, g, r, gw, ls);
    HIP_TRY(hipGetLastError());
    int k = 0;
    while (k < max_rounds) {
        const int end = fp_chunk_end(k, max_rounds, chunk);
        for (++k; k <= end; ++k) {
            const int b = k & 1;
            hipLaunchKernelGGL(k_fp_select<false>, thread_grid, block, 0, e->stream, head, g, eps, p, r, y[b], y[b ^ 1], gw, m, ls, b);
            hipLaunchKernelGGL(k_fp_mark, mark_grid, block, 0, e->stream, head, g, ep.out_col.get(), ls, b, piece, fq.items.get(), icap, longs, lcap);
            by_fw_shape(PP, levels, [&](auto pp_c, auto lv_c) -> int {
                constexpr int P = decltype(pp_c)::value, L = decltype(lv_c)::value;
                hipLaunchKernelGGL((k_fp_gather<P, L>), rows_grid, block, 0, e->stream, head, g, y[b], r, gw, m, T, piece, ls, b);
                hipLaunchKernelGGL((k_fw_pieces<P, L>), piece_grid, block, 0, e->stream, g, y[b], gw, m, T, piece, &head->fw, fq.items.get(), icap,
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
    hipLaunchKernelGGL(k_fp_left<false>, thread_grid, block, 0, e->stream, head, g, eps, r, gw, m, ls, k & 1);
    hipLaunchKernelGGL(k_fw_rem, dim3((unsigned)fw_rem_grid(V)), block, dot_lds_bytes(gw, 1), e->stream, r, gw, m, x2i, V, fq.part.get(), stride);
    hipLaunchKernelGGL(k_dot_combine, dim3((m + DOT_CB_WAVES - 1) / DOT_CB_WAVES), dim3(DOT_CB_WAVES * WAVE), 0, e->stream, fq.part.get(),
                       (const long long *)nullptr, stride, m, m, &head->fw.dot, head->rem);
    HIP_TRY(hipGetLastError());
    if (int rc2 = DeviceTime{e}.close()) return rc2;
    HIP_TRY(hipMemcpyAsync(fq.fp_pin, head, sizeof(FpHead), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(h_seeds, seeds, sizeof(FpSeed) * (size_t)n_seeds, hipMemcpyDeviceToHost, e->stream));
    if (int rc2 = run_end(e)) return rc2;
    const float push_ms = e->query_ms;
    if (pin->overflow || pin->fw.overflow) return fail(e, DPPR_ERR_HIP, "forward_push: a list was too short (fp_list_cap, fp_mark_cap, fw_item_cap)");
    const FpHead hd = *pin;
    struct Rowless { int id, col; double p; };
    std::vector<Rowless> rowless; // the seeds the host answers: p = 0.15 w
    for (int j = 0; j < n_seeds; ++j)
        if (h_seeds[j].row < 0) rowless.push_back({h_seeds[j].id, h_seeds[j].col, fp_rowless_p(h_seeds[j].w)});
    for (int c = 0; c < m; ++c) {
        if (out.rounds_used) out.rounds_used[c] = hd.rounds_used[c];
        if (out.converged) out.converged[c] = hd.left[c] == 0 ? 1 : 0;
        if (out.rem) out.rem[c] = hd.rem[c];
        if (out.pushes) out.pushes[c] = (int64_t)hd.pushes[c];
        if (out.left) out.left[c] = (int64_t)hd.left[c];
    }
    if (out.work)
        for (int i = 0; i < 3; ++i) out.work[i] = (int64_t)hd.work[i];

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
        for (const Rowless &s : rowless) // (a row of the device holds +0.0 there: the seed is not in the column's list yet)
            out.topk_counts[s.col] = fp_topk_insert(out.topk_ids + (size_t)s.col * out.k, out.topk_p + (size_t)s.col * out.k, out.topk_counts[s.col],
                                                    out.k, out.min_p, s.id, s.p);
    }
    if (e->profiling) e->query_ms = push_ms; // (the parts opened brackets of their own)
    return DPPR_OK;
}

int forward_push_call(dppr_engine *e, int32_t epoch, const int64_t *offsets, const int32_t *ids, const double *weights, int32_t m, double eps,
                      int32_t max_rounds, const dppr_forward_push_out_t *out) {
    if (!fp_args_ok(m, eps, max_rounds, out))
        return fail(e, DPPR_ERR_INVALID, "forward_push: m in [1, 16], eps > 0 and finite, max_rounds in [1, 256], non-null out");
    if (!fp_parts_ok(out))
        return fail(e, DPPR_ERR_INVALID,
                    "forward_push: a part asked for needs its pointers; k in [1, DPPR_TOPK_MAX], min_p >= 0; n_at in [1, DPPR_FORWARD_AT_MAX]; dtype 0 or 1, layout 0 or 1");
    if (TgCheck c = fp_csr_check(offsets, ids, weights, m, e->V)) return fail(e, DPPR_ERR_INVALID, (std::string("forward_push: ") + tg_check_text(c)).c_str());
    const uint32_t which = fp_which(out);
    if ((which & FP_AT) && !dppr::ids_in_range(out->at_ids, out->n_at, e->V)) return fail(e, DPPR_ERR_INVALID, "forward_push: at_ids in [0, V)");
    const Epoch *ep = find_epoch(e, epoch);
    if (!ep) return fail(e, DPPR_ERR_INVALID, "forward_push: epoch not resident (evicted or never built)");
    HIP_TRY(hipSetDevice(e->device));
    for (void *dst : {out->dense_p_dev, out->dense_r_dev})
        if (dst && !dev_range_ok(e, dst, ex_dense_bytes(out->dense_dtype, m, e->V), ex_elem_bytes(out->dense_dtype)))
            return fail(e, DPPR_ERR_INVALID,
                        "forward_push: a dense destination must be aligned device memory of the engine's device, m x V elements inside one allocation");
    if (!which) return DPPR_OK;
    std::lock_guard<std::mutex> map_lk(e->map_mu); // (as dppr_read: one state of the id space for the whole call)
    return run_fpush(e, *ep, offsets, ids, weights, m, eps, max_rounds, which, *out);
}

} // namespace
