// dppr_host_state.hpp -- host side of libdppr_hip.so, part 1 of 4: what an engine OWNS (replaces gpu/DeviceMemory.cuh,
// gpu/GPUEdgeBatch.cuh and the members of gpu/SlidingGraphBuilder.cuh) -- the resident graph epochs, the per-source slots and source
// groups (what both carry with the same meaning: SolveState), the two HIP streams (solver / builder) and their scratch -- plus the
// small helpers every other part uses (error reporting, the bounded stream wait, the event bracket of a timed region and the end of
// a solve, the id lookahead of dppr_hint_next_batch).
// Every device or pinned-host allocation is a DevBuf / PinBuf (dppr_devbuf.hpp) that is a member of its owner -- Epoch, Slot, Group,
// dppr_engine -- or a local of the function that needs it: memory goes when its owner goes, dppr_destroy lists nothing, and a call
// that fails half way leaves nothing behind. The HIP runtime's allocation calls appear in the two policies below and nowhere else.
// Included by dppr_engine.hip only, after the kernel headers (one translation unit: the kernels are templates).
#pragma once

// Slot::cnt: [0..2] rotating frontier counters, [3] phase-1 candidates, [4] scratch, [5..6] big-row
// counters, [7] list scratch / status word of a resident launch; the log of a launch (up to
// 2 x MAX_CHUNK entries, dppr_loop_plan.hpp: a whole batch) follows the header
static constexpr int CNT_HDR = 16;
static constexpr int PERSIST_RETRY_BATCHES = 64; // after a failed roll-call: batches on per-iteration launches before the next try
static constexpr int GQ_PAD = 32;               // ints between the rotating group counters of k_gsweep (own 128-byte line each)
static constexpr int BIN_MAX_BLOCKS = 1 << 16, BIN_MAX_BIG = 4096, BIN_SMALL_INTS = BIN_MAX_BLOCKS + BIN_MAX_BIG + 1 + 64; // bin_cut scratch
static constexpr int SU_SPLIT_MIN = 1 << 16;  // batch records from which IncrementalBatchUpdate runs as k_su_terms + k_su_apply (stream_update)
static constexpr int MERGE_MISS_WORD = 44; // word of hub_hist (64 ints) that counts the retired keys a slide's merge did not find

namespace dppr {

// bytes this PROCESS holds through the two policies (dppr_debug_live_bytes: a leak check that ignores the device's other tenants)
inline std::atomic<long long> g_device_bytes{0}, g_pinned_bytes{0};

struct DeviceAlloc {
    static int alloc(void **p, size_t bytes) {
        const hipError_t rc = hipMalloc(p, bytes);
        if (rc == hipSuccess) g_device_bytes.fetch_add((long long)bytes, std::memory_order_relaxed);
        return (int)rc;
    }
    static int free(void *p, size_t bytes) {
        g_device_bytes.fetch_sub((long long)bytes, std::memory_order_relaxed);
        return (int)hipFree(p);
    }
};

struct PinnedAlloc {
    static int alloc(void **p, size_t bytes) {
        const hipError_t rc = hipHostMalloc(p, bytes, hipHostMallocDefault);
        if (rc == hipSuccess) g_pinned_bytes.fetch_add((long long)bytes, std::memory_order_relaxed);
        return (int)rc;
    }
    static int free(void *p, size_t bytes) {
        g_pinned_bytes.fetch_sub((long long)bytes, std::memory_order_relaxed);
        return (int)hipHostFree(p);
    }
};

template <class T> using DevBuf = Buf<T, DeviceAlloc>;
template <class T> using PinBuf = Buf<T, PinnedAlloc>;

} // namespace dppr

namespace {

struct Epoch {
    DevBuf<int> row_ptr; // V+1   in-CSR (push)
    DevBuf<Adj> adj;     // Ed
    DevBuf<int> out_row_ptr; // V+1  out-CSR (pull)
    DevBuf<int> out_col;     // Ed
    int Ed = 0;
    // batch that produced this epoch (empty for epoch 0)
    DevBuf<int> b1, b2, deg_after; // 4c each
    DevBuf<uint8_t> ins;
    int L = 0;
    DevBuf<uint32_t> sk, sv; // the batch's records grouped by tail at slide time: tails ascending, record indices (stable)
    int max_bucket = 0; // records in the fullest bucket of the bucket path (largest_bucket, dppr_grouping.hpp), counted at upload
    bool grouped = false;
    int id = -1; // global epoch number stored in this ring entry
    // sweep groups: tiles [grp_tile[g], grp_tile[g+1]) per workgroup, about equal edges each
    DevBuf<int> grp_tile; // V/64 + 2
    int n_groups = 0;
    int grp_n_int = 0;       // internal ids covered by the table
    // the same for the source-group sweeps (k_gsweep), cut once a source group exists: many small groups --
    // two workgroups per CU and an even spread matter there, a bound on the group count does not; at
    // most 512 vertices each when a 16-wide source group exists
    DevBuf<int> ggrp_tile;
    int n_ggroups = 0;
    int ggrp_max_tiles = 0;
    DevBuf<int> gtab;     // row tables of those groups (k_gtables): GT_STRIDE(512 | 1024) ints per group
    // hub directory of this epoch (vertices whose pushes are aggregated in LDS)
    DevBuf<int> hub_v, hub_degp1;
    int n_hubs = 0;
    // binned sweep (dppr_binned.hpp): block cuts (first tile of every A- / B-block), per edge the head index inside
    // its A-block + B-major position (A-major order) and the row index inside its B-block (B-major order)
    DevBuf<int> acut; int *bcut = nullptr; // first vertex of every A- / B-block (one allocation; bcut points into it)
    int n_a = 0, n_b = 0;
    DevBuf<BinChunk> chunks;           // work items of k_bin_scatter
    int n_chunks = 0;
    DevBuf<uint16_t> hl, dl; // hl: per RUN (A-major), head index + first-of-tile bit; dl: per edge (B-major), row index + first-of-run bit
    DevBuf<int> vb, tb;      // per aligned block of 64 edges: run that holds its first edge; per 64 runs: tile that holds the first run
    DevBuf<int> tdelta;                 // per tile (A-major order): B-major run index - A-major run index of its runs
    int n_runs = 0, n_tiles = 0;
    bool bin_valid = false;
    int bin_n_int = 0; // internal ids the tables cover (<= grp_n_int: later ids have no edge in this epoch)
    // slot table of the resident sweep (dppr_resident.hpp: k_res_slots), rebuilt with every group cut
    DevBuf<uint32_t> res_pk; // Ed entries, group by group, sorted by gather position
    bool res_valid = false;
    // the batch's records (sk / sv) cut into the sweep groups' ranges, for IncrementalBatchUpdate inside a resident launch
    DevBuf<int> su_rng;      // n_groups + 1 first-record indices, then two result words of k_res_rec_ranges
    bool su_inline = false;     // every group's range fits the launch's workgroup and no tail lies beyond the groups
};

// What a Slot and a Group carry with the same meaning: the state a solve leaves, its statistics and the loops' histories
struct SolveState {
    bool converged = false; // |r| <= conv_eps everywhere, for every source (state after a completed solve)
    double conv_eps = 0.0;
    double park_eps = 0.0;  // parked rows satisfy |r| <= park_eps (0: they are exactly zero)
    int last_epoch = -2;    // epoch whose batch was applied last (-2: unknown, e.g. after dppr_write: anything goes)
    dppr_stats_t st{};
    LoopHistory hist;       // iterations the last loops of each phase took; groups: also before the push form took over (dppr_loop_plan.hpp)
    DevBuf<IterStats> dstats; // two blocks: [0] push iterations (and resident launches), [1] dense sweeps -- the roofline of the sweep kernel counts its own edges
};

struct Slot : SolveState {
    int source = 0;     // internal id
    int source_ext = 0; // id the caller gave
    DevBuf<double> p, r;
    DevBuf<double> mark;  // dppr_mark: p as it was then, [V] by EXTERNAL id (empty: no mark; dppr_changes.hpp)
    DevBuf<double> x, x2; // dense per-iteration push amounts (x) and pull output (x2)
    DevBuf<uint32_t> act[2]; // activity bitmaps of x / x2 for sweeps on windows that cannot run resident
    size_t act_bytes = 0;
    DevBuf<int> ft[2];
    DevBuf<int> neg;     // phase-1 candidates
    DevBuf<int> status;  // status-array duplicate filter (variants EAGER / VANILLA): launch number that queued the vertex last; allocated on first use
    DevBuf<int> cnt;     // [0..2] rotating frontier counters, [3] neg candidates, [4] scratch, [5..6] big-row counters
    DevBuf<BigItem> big; // deferred big rows of the current iteration
    int *log = nullptr;     // per-chunk log: frontier size seen by each enqueued iteration
    long long iter_seq = 0; // running iteration number (selects the big-row counter)
    double sweep_us = 0;       // binned windows: running mean of a sweep's time (the push / sweep decision)
    double atomic_ns = 1.0 / 23.5; // ... and of a push iteration's time per in-edge (starts at the chip's rate of returning f64 atomics)
    bool start_dense[2] = {false, false}; // the last loop of each phase began with a frontier worth a sweep
    int last_F0[2] = {0, 0};   // ... and its size
    bool seed_lists_valid = false; // ft[0]/cnt[0] and neg/cnt[3] hold the lists of the last dppr_incremental_batch_update
    bool phase0_done = false; // ExecuteMainLoop(0) completed since the last modification
    double phase0_eps = 0.0;
    bool trace = false;
    std::vector<int64_t> trace_off;
    std::vector<int32_t> trace_ids;
};

// f2: up to 16 sources solved together on interleaved state (dppr_multi.hpp)
struct Group : SolveState {
    int n = 0;                 // sources in use (1..16)
    int spl = 1;               // doubles per lane of an octet: 1 (rows of <= 8 doubles) or 2
    int gw = OCT;              // doubles per vertex = row_width(n): 2, 4, .. 16 (dppr_multi.hpp)
    int src_ext[GS_MAX] = {0}; // ids the caller gave
    SrcN src{};                // internal ids, -1 = unused lane (and a lane whose target is a vertex set: src_ext -1 too)
    TargetSets tsets;          // the lanes' seed sets by external id (dppr_targets_plan.hpp); n == 0: every lane is a plain source
    TgTable ttab;              // ... as the device holds them: internal ids ascending within a lane (host copy, remapped by a renumbering)
    DevBuf<unsigned char> tg;  // ... the seed table on the device (dppr_targets.hpp; empty without a set lane)
    DevBuf<double> p, r, x, x2; // [V][gw]
    DevBuf<double> mark;       // dppr_group_mark: p as it was then, [V][gw] by EXTERNAL id (empty: no mark; dropped when the sources change)
    DevBuf<uint32_t> act[2]; // activity bitmaps that go with x / x2
    size_t act_bytes = 0;
    DevBuf<int> cnt;        // [3][GS_MAX] rotating frontier sizes, then the per-chunk log [MAX][GS_MAX]
    DevBuf<int> gq;         // one-sweep launches: three rotating group counters (a launch takes tickets from one and zeroes the next), GQ_PAD ints apart
    unsigned gq_seq = 0;       // one-sweep launches enqueued so far
    DevBuf<int> mlog;       // multi-sweep launches: [GS_MAX] status word + padding, then one row of frontier sizes per sweep
    // the tail of a loop as pushes (dppr_gpush.hpp): vertex lists, scan, control block; allocated on first use
    DevBuf<int> plist[2];
    DevBuf<int> ppre;
    DevBuf<GPushCtl> pctl;
};

// What a query needs of a state, slot or group alike (dppr_host_query.hpp): p / r rows gw doubles wide, n lanes, the state's mark
// and what its last solve left
struct StateView {
    const double *p, *r;
    int gw, n;
    DevBuf<double> &mark;
    const SolveState &st;
    bool group; // (the words of a rejection name a slot or a group)
};
// the three sections of a group's seed table (dppr_targets_plan.hpp lays the block out)
inline TgDev tg_dev(const Group &g) {
    const int64_t total = g.ttab.total();
    return {reinterpret_cast<const double *>(g.tg.get() + tg_w_at()), reinterpret_cast<const int *>(g.tg.get() + tg_off_at(total)),
            reinterpret_cast<const int *>(g.tg.get() + tg_ids_at(total))};
}
inline StateView view(Slot &s) { return {s.p, s.r, 1, 1, s.mark, s, false}; }
inline StateView view(Group &g) { return {g.p, g.r, g.gw, g.n, g.mark, g, true}; }

// The workspace of the state queries, family by family: all of it allocated on a family's first call and grown on demand
struct QueryWork {
    struct TopK { // dppr_topk.hpp
        DevBuf<unsigned char> ws;           // pass-1 and refinement histograms, per-lane control words (zeroed per query)
        DevBuf<unsigned long long> out_key; // [16][DPPR_TOPK_MAX] result lists before ordering
        DevBuf<int> out_row;
        DevBuf<int> cand;                   // candidate lists: [n][cap] internal rows
        DevBuf<unsigned char> res; PinBuf<unsigned char> pin; // ordered results (device / pinned host): counts, ids, p, r
    } tk;
    struct ReadAt {
        DevBuf<unsigned char> buf; // point reads: ids, then p and r outputs (dppr_group_score_at: ids, then the scores)
    } ra;
    struct Scratch { // the compacted scratch state of the weighted, changes and ranked queries (one call at a time: map_mu, the solver stream)
        DevBuf<double> a, b; // [occupied rows][lanes] each: the scores of a weighted or ranked call (a alone), |p - mark| and p - mark of changes
        DevBuf<int> ext;     // the external id of every row of it
    } sc;
    struct Weighted { // a group as a weighted set of targets (dppr_wquery.hpp); its scores: sc
        DevBuf<double> w; // [16][16] weights of the call
    } wq;
    struct Changes { // what a batch moved (dppr_changes.hpp); |p - mark| and p - mark: sc
        DevBuf<unsigned char> res; PinBuf<unsigned char> pin; // counts, moved, ids, deltas, p (dppr_changes_plan.hpp): device / pinned host
    } ch;
    struct Export { // dppr_export.hpp, dppr_export_plan.hpp; the block grows with a host destination's cap
        DevBuf<unsigned short> mask; // [V] which lanes qualify at every external id
        DevBuf<int> cnt;             // [tiles][16] qualifying ids per tile and lane
        DevBuf<long long> base;      // [tiles][16] first output position of a tile's entries of a lane
        DevBuf<unsigned char> blk; PinBuf<unsigned char> pin; // head (offsets, go), then ids / p / r of a host destination: device / pinned host
    } ex;
    struct Patch { // dppr_patch.hpp, dppr_patch_plan.hpp; the block grows with a host destination's caps
        DevBuf<unsigned> mask;  // [V] upserts (low half) and deletes (high half) of every lane at every external id
        DevBuf<int> cnt;        // [tiles][2][16] upserts and deletes per tile and lane
        DevBuf<long long> base; // [tiles][2][16] first output position of a tile's entries of a kind and lane
        DevBuf<unsigned char> blk; PinBuf<unsigned char> pin; // head (offsets, go, written), then up_ids / up_p / del_ids of a host destination
    } pt;
    struct Dot { // the state folded over the vertex axis (dppr_dot.hpp, dppr_dot_plan.hpp)
        DevBuf<double> part;      // one partial per (tile, output), output-major
        DevBuf<unsigned char> in; // a sparse call: its tile table and columns, and the ids / w of a host source
        DevBuf<unsigned char> blk; PinBuf<unsigned char> pin; // head (the flag), then the results of a host destination: device / pinned host
        dppr::DotTable tb;        // host side of the tile table (kept for its capacity)
        bool lds_set = false;     // the dense pass was given its dynamic LDS limit
    } dot;
    struct Walk { // forward walks and the refinement of point queries (dppr_walk.hpp, dppr_walk_plan.hpp)
        DevBuf<int> starts;       // [m] the starts / queried ids of the call
        DevBuf<int> ends;         // [m][W] endpoints of a host destination and of a refine call
        DevBuf<double> res;       // a refine call: folded [m][2 n], then est | corr | sumsq [m][n] each
        std::vector<int64_t> off; // a refine call: the offsets q * W of its m queries (kept for its capacity)
    } wk;
    struct Cluster { // the conductance sweep over a top-k order (dppr_cluster.hpp, dppr_cluster_plan.hpp)
        DevBuf<unsigned short> rank;     // [occupied rows][cl_stride(n)] position of a vertex in every lane's order (0xffff: absent)
        DevBuf<int> d;                   // the control words (ClCtl), then d_out | d_in | deg, each [n][k]
        DevBuf<unsigned long long> list; // chunk items of the rows walked in pieces (cl_list_cap)
        DevBuf<unsigned char> blk; PinBuf<unsigned char> pin; // the records, ids, cut_out, cut_in, vol: device / pinned host
    } cl;
    struct Subgraph { // the subgraph a top-k order induces (dppr_subgraph.hpp, dppr_subgraph_plan.hpp); the rank table and the chunk list are cl's
        DevBuf<int> work;                                     // the control words (SgCtl), the matches of every position [n][k], the rows queued for k_sg_long [n][k]
        DevBuf<unsigned char> blk; PinBuf<unsigned char> pin; // the head, ids, p, row_ptr and a host destination's col: device / pinned host
    } sg;
    struct Rank { // ranked candidates (dppr_rank.hpp, dppr_rank_plan.hpp); its scores: sc
        DevBuf<unsigned> excl; // bit i: excluded for lane i (zeroed per call). A slot / group call: [live rows] by internal id; a call over a forward track: [V] by EXTERNAL id, bit c for column c
        DevBuf<int> len; PinBuf<int> len_pin;     // [seeds][2] out-row and in-row length of every seed: device / pinned host
        DevBuf<unsigned long long> list;          // the piece list of the call (rk_piece_cap)
        std::vector<unsigned long long> items;    // ... as the host builds it (kept for its capacity)
    } rk;
    struct Position { // positions of given vertices in a lane's order (dppr_position.hpp, dppr_position_plan.hpp); its scores: sc, its ids and query scores: ra
        DevBuf<unsigned char> keys; // [n][m] keys of the queries by position in the lane's order, then [n][m] their places in `ids`
        DevBuf<unsigned> slots;     // [n][m + 1] entries per first preceded position, the lane's count last (zeroed per call)
        DevBuf<unsigned char> blk; PinBuf<unsigned char> pin; // counts, positions: device / pinned host
        bool lds_set = false;       // the count pass was given its dynamic LDS limit
    } pos;
    struct Sample { // vertices drawn in proportion to a lane's score (dppr_sample.hpp, dppr_sample_plan.hpp); its exclusion words: rk
        DevBuf<double> leaves; // [n][Vt] the weights by external id, lane-major
        DevBuf<double> nodes;  // [n][node_stride] the levels 8 .. top of every lane's tree
        DevBuf<double> low;    // [n][Vt] the levels 1 .. 7 (dppr_debug_sample_form(1) alone)
        DevBuf<unsigned char> blk; PinBuf<unsigned char> pin; // head (totals, supports, statuses), then ids / w of a host destination: device / pinned host
    } sm;
    struct Explain { // top contributors and the path to the seeds (dppr_explain.hpp, dppr_explain_plan.hpp); its memo: the first plane of sc
        DevBuf<unsigned char> blk; PinBuf<unsigned char> pin; // the planes asked for, then the queried ids: device / pinned host
    } exq;
    struct Certify { // the certificate of a state (dppr_certify.hpp, dppr_certify_plan.hpp); the gathered sums S: the first plane of sc
        DevBuf<unsigned char> blk; PinBuf<unsigned char> pin; // the planes asked for: device / pinned host
        DevBuf<unsigned char> ws;        // the head (counters, queued pieces), the two sums, the workgroups' (word, id) partials (cert_work)
        DevBuf<double> part;             // the partials of the two sums, as the dot family lays them out
        DevBuf<unsigned long long> list; // the queued pieces of the long rows (cert_list_cap)
        DevBuf<double> pp;               // [queued pieces][gw] one partial per piece
    } cert;
    struct Forward { // the forward sweep of any vertex (dppr_forward.hpp, dppr_forward_plan.hpp); its selection: tk, its point reads: ra
        DevBuf<double> planes;            // y | y' | f | x, each [V][row width]
        DevBuf<unsigned char> head; PinBuf<unsigned char> pin; // FwHead: device / pinned host (the freeze word per chunk, the whole head at the end)
        DevBuf<double> part;              // the partials of the rem fold, as the dot family lays them out
        DevBuf<unsigned long long> items; // the queued pieces of the long in-rows (fw_item_cap)
        DevBuf<unsigned char> longs;      // the long rows (FwLong, fw_long_cap)
        DevBuf<double> pp;                // [queued pieces][row width] one partial per piece
        // the forward push (dppr_fpush.hpp, dppr_fpush_plan.hpp) shares everything above (its planes: p | r | y0 | y1) and adds:
        DevBuf<unsigned char> fp_head; PinBuf<unsigned char> fp_pin; // FpHead: device / pinned host (one word per chunk, the whole head at the end)
        DevBuf<unsigned char> fp_seeds; PinBuf<unsigned char> fp_seeds_pin; // the seed table (FpSeed): device / pinned host (the rows come back)
        DevBuf<int> fp_lists;             // front[2] | recv[2], each fp_list_cap rows
        DevBuf<unsigned> fp_bits;         // a bit per row: already a receiver of the round
        DevBuf<unsigned long long> fp_mark; // the queued pieces of the frontier's out-rows (fp_mark_cap)
        // the forward track (dppr_ftrack.hpp, dppr_ftrack_plan.hpp) runs the rounds of the push over all of the above and adds:
        DevBuf<uint32_t> ft_sort;         // the records' keys and indices, in and sorted by tail and by head (ft_sort_words)
        DevBuf<unsigned char> ft_tmp;     // the device radix sort's own scratch
        DevBuf<double> ft_c;              // [records][row width] c of step T, by record
    } fw;
    struct FCluster { // the full-length conductance sweep of a forward track (dppr_fcluster.hpp, dppr_fcluster_plan.hpp); its planes: fw
        DevBuf<unsigned short> mask;     // [V] which columns qualify at every external id
        DevBuf<int> cnt;                 // [tiles][m] qualifying ids per tile and column
        DevBuf<long long> base;          // [tiles][m] first position of a tile's entries of a column
        DevBuf<unsigned char> head; PinBuf<unsigned char> head_pin; // ExHead (the qualifying offsets), the control words, the records: device / pinned host
        DevBuf<unsigned long long> keys; // the score bits of the qualifying entries, in | sorted
        DevBuf<int> vals;                // their external ids, in | sorted
        DevBuf<unsigned char> tmp;       // the device radix sort's own scratch
        DevBuf<int> rank;                // [live rows][m] position of a vertex in every column's order (-1: absent)
        DevBuf<long long> d;             // d_out | d_in | deg by position, then the tiles' sums and carries
        DevBuf<unsigned char> tbest;     // the tiles' first minima (FcBest)
        DevBuf<unsigned char> list;      // the queued pieces of the long rows (FcItem, fc_list_cap)
        DevBuf<unsigned char> blk; PinBuf<unsigned char> pin; // ids, score, cut_out, cut_in, vol by position: device / pinned host
    } fc;
    struct FtrackRank { // the ranked, position and sample queries over a forward track (dppr_ftrack_rank.hpp, dppr_ftrack_rank_plan.hpp); its exclusion words, row lengths and pieces: rk (the words by EXTERNAL id here), its scores: sc
        DevBuf<int> seeds;      // the flat table of the track's seeds, external ids
        DevBuf<int> cnt;        // [tiles] kept ids per tile
        DevBuf<long long> base; // [tiles] first row of a tile in the compacted scratch state
        DevBuf<unsigned char> head; PinBuf<unsigned char> head_pin; // ExHead (offsets[1]: the kept rows): device / pinned host
    } fr;
    struct Assign { // every vertex to its best lane across groups (dppr_assign.hpp, dppr_assign_plan.hpp); the block grows with a host destination
        DevBuf<double> scale; // [256] the scales of the call
        DevBuf<int> cnt;      // [tiles] flips per tile
        DevBuf<int> base;     // [tiles] first output position of a tile's flips
        DevBuf<int> ws;       // [3][tiles x 256] id | old | new of every tile's flips, compacted inside the tile
        DevBuf<unsigned char> blk; PinBuf<unsigned char> pin; // head (n_flips, go, counts), then label / best / margin / flips of a host destination: device / pinned host
    } as;
};

} // namespace

namespace dppr {
// A forward track (dppr_ftrack_*): the push state of up to 16 weighted start sets, by EXTERNAL id, and what the last create or
// update call counted. Owned by the engine; touched by the track calls alone.
struct FTrack {
    bool used = false;
    int epoch = -1, m = 0, gw = 0;
    double eps = 0.0;
    std::vector<int64_t> offsets;
    std::vector<int32_t> ids;
    std::vector<double> weights;
    DevBuf<double> state;   // p | r, each [V][gw]
    bool converged = false; // every column of the last call
    int rounds_used[Q_LANES] = {};
    long long pushes[Q_LANES] = {}, left[Q_LANES] = {}, work[3] = {}, fix[3] = {};
    double rem[Q_LANES] = {};
};
} // namespace dppr

struct dppr_engine : dppr::IdSpace { // (the id maps, the parked zone and the pending row moves: dppr_idspace.hpp)
    int device = 0;
    int V = 0, W = 0, c = 0, directed = 1, n_epochs = 1;
    int Ed = 0;   // directed edges in the window
    int bits = 1; // bits of a vertex id
    int schedule = DPPR_SCHEDULE_EAGER;
    // the reference's variants (-o, gpu/PPRRevPushGPUVariants.cuh) as mechanisms of the push iterations: dppr_set_variant
    bool status_dedup = false; // duplicate filter of a push iteration: status array (EAGER 2, VANILLA 3) instead of the threshold crossing
    bool pre_extract = false;  // synchronous push iterations zero residual[u] at the snapshot (InspectExtra: FAST_FRONTIER 1, VANILLA 3) instead of repairing
    bool group_at_slide = false; // dppr_set_batch_grouping(1): the batch's records are grouped by tail (and CopyOutDegree done) when the batch is uploaded
                                 // (dppr_slide); default since round 5: inside dppr_update, where the reference times them (gpu/PPRGPU.cuh:138-164)
    int merge_miss_host = 0;        // retired keys the last slide's merge did not find (read back with the build's synchronisations)
    long long merge_fallbacks = 0;  // slides that re-sorted the window because of that
    bool test_force_merge_miss = false; // (test hook, DPPR_TEST_MERGE_MISS=1: every incremental slide takes the fallback)
    int raw_backoff = 0;         // batches for which a resident launch does not take the records raw (after one called itself off: a group with more records than threads)
    bool merge_phases = false; // dppr_set_phase_merge: one loop for residuals of both signs (eager schedule only)
    int merge_div = 4;         // ... run to eps / merge_div
    hipStream_t stream = nullptr; // the SOLVER's stream: IncrementalBatchUpdate, the frontier loops, reads and writes of p / r
    hipStream_t bs = nullptr;     // the graph BUILDER's stream (lowest priority): window ring, key merge, CSRs, group cuts and tables, binned tables,
                                  // id-space row moves. Every builder entry point ends with a host synchronisation of bs, every solver call with one of
                                  // `stream`, so calls made one after the other need no cross-stream event; dppr_slide_concurrent runs beside a solver call.
    bool build_concurrent = false; // (builder thread only) the slide in progress may run beside dppr_update / dppr_group_update on an OLDER epoch
    std::mutex err_mu;             // `err` is written by whichever of the two threads fails
    std::mutex map_mu;             // the id maps and the pending row moves: held by the builder from the first id it assigns to the end of the row
                                   // moves (dppr_set_batch; the id-assigning head of a slide), and by a reader on the solver thread (dppr_read,
                                   // dppr_group_read, settle_parked) from its copy of the map to the end of its gathers -- a read beside a
                                   // concurrent slide sees either the maps and rows of before a revival or those of after it
    unsigned map_gen_on_device = 0; // IdSpace::map_gen the device copy of ext2int was taken at
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t evpool[2 * 64] = {};
    bool profiling = false;
    int pull_block = 0;   // sweep workgroup size pinned by dppr_set_tuning (0: 1024)
    int chunk_iters = 24; // iterations enqueued between two host read-backs of the frontier size
    bool chunk_explicit = false; // set by dppr_set_tuning: then it also caps what a resident launch is given
    // resident sweeps (dppr_resident.hpp)
    int persist_mode = 1;              // 1: use resident sweeps when an epoch's groups fit the chip at once
    bool persist_ok = true;            // cleared when a roll-call gives up: per-iteration launches until re-armed
    int persist_retry = 0;             // dppr_update calls until resident launches are tried again (0: not pending)
    int persist_cap = 0;               // co-resident workgroups of k_pull_resident at the sweep's block size
    int res_slots = 1;                 // 1: resident launches take their edge slots from the sorted slot table (0: CSR order)
    int res_update = 1;                // 1: a whole-batch resident launch applies the batch's records itself (PLAN_UPDATE)
    DevBuf<double> res_arena;       // snapshot vectors of a resident launch (resident_arena)
    long long res_arena_stride = 0;    // doubles per vector
    unsigned long long persist_ticks = 5000000ull; // roll-call time limit in 100 MHz ticks (50 ms)
    int persist_rollcall_extra = 0;    // tests: the roll-call waits for a workgroup that does not exist
    DevBuf<GridBar> bar;
    // window ring, stream order
    DevBuf<int> w1, w2;
    int head = 0;
    bool loaded = false;
    bool broken = false; // a renumbering failed half way (HIP error after the host maps changed): every call but dppr_destroy is refused
    DevBuf<int> outdeg;
    DevBuf<int> hub_slot_of; // V, scratch of the CSR build (k_assign_hubs: ~hub slot, or out-degree + 1)
    DevBuf<int> hub_hist;    // 32 + 1 ints (histogram, hub counter)
    int hub_min_degree = HUB_MIN_DEGREE_DEFAULT;
    int big_row = BIG_ROW_DEFAULT;
    int pull_min_frontier = 0; // 0: auto (max(1024, Ed/192)); < 0: never pull; > 0: pull when F >= value
    // CSR build: persistent sorted key arrays (in-orientation dst<<bits|src, out-orientation
    // src<<bits|dst; undirected graphs share one) + scratch of the same size
    DevBuf<uint64_t> in_sorted, out_sorted;
    DevBuf<uint64_t> keys_a, keys_b;
    DevBuf<unsigned char> sort_tmp;
    size_t sort_tmp_bytes = 0;
    DevBuf<int> su_grp; // hand-written grouping of a large batch (dppr_update.hpp k_su_grp_*): histogram | cursors | bucket starts + slice starts
    // incremental maintenance (f1): batch keys, positions of the retired keys
    DevBuf<uint64_t> bk[4]; // del-in, ins-in, del-out, ins-out (unsorted)
    DevBuf<uint64_t> bks[4]; // the same, sorted
    DevBuf<int> delpos; // positions of a slide's retired keys in the persistent sorted keys (2 * max_batch)
    struct Pre { // dppr_hint_next_batch
        std::future<bool> task;
        const int32_t *src[4] = {nullptr, nullptr, nullptr, nullptr};
        int n[4] = {0, 0, 0, 0};
        std::vector<int32_t> out[4];
        std::vector<uint32_t> miss[4]; // positions the lookup left at -1 (no id yet / parked), in array order
        unsigned long long epoch = 0;
        bool armed = false, ok = false;
    } pre;
    long long pre_hits = 0, pre_misses = 0; // id arrays that dppr_set_batch / dppr_slide took from the lookahead; entries resolved at the call
    bool incremental = true; // dppr_slide merges the batch into the sorted keys (false: full re-sort)
    bool sweep_bits = false;        // per-iteration single-source sweeps test an activity bitmap before each gather (dppr_set_sweep_bitmap;
                                    // measured slower on every stand-in, DESIGN.md section 6: off unless asked for)
    bool hot_blocks = true;         // vertex numbering in blocks of falling in-degree (DPPR_HOT_BLOCKS=0: two blocks, hot | rest)
    int gsweep_hot_rows = 24576;    // k_gsweep: rows below this id are gathered with the default cache policy, the others non-temporal (DPPR_GSWEEP_HOT)
    int gsweep_grid_cap = 0;        // workgroups of a one-sweep launch of k_gsweep: 0 = two per CU, what is resident at once (the groups beyond
                                    // the grid are dealt by a device counter; LiveJournal stand-in, 10 sources: 12.40 ms per batch at 512, 13.1-13.2 at
                                    // 768 / 1024 / 2048; DPPR_GSWEEP_GRID: tuning runs)
    bool group_resident = true;     // source groups on windows whose sweep groups are all resident run a loop as multi-sweep launches
    int gmulti_cap[2] = {-1, -1};   // co-resident workgroups of k_gsweep<.., true> per state width (-1: not queried yet)
    bool any_groups = false;        // a source group exists: epochs carry the second group table
    int ggroups_min = 256;          // ... of at least this many groups (DPPR_GGROUPS_MIN: tuning runs; 512 / 1008 measured slower on
                                    // the configs[1] stand-in, equal on the LiveJournal one)
    bool force_radix_grouping = false; // (A/B, tests: DPPR_GROUPING_RADIX=1 -- the in-region grouping always as key kernel + device radix sort)
    bool cost_model = true;         // binned windows: push or sweep by estimated cost (DPPR_COST_MODEL=0: by the vertex-count threshold)
    bool group_full_rows = false;   // (A/B, DPPR_GROUP_FULL_ROWS=1: rows of 64 / 128 bytes whatever the source count, as until round 3)
    bool wide_groups = false;       // ... one of more than 8 sources: its groups hold at most 512 vertices
    bool group_tail_seeding = true; // source groups seed from the batch tails after a converged solve (false: dense Inspect)
    int gpush_enter_pairs = -1;     // a group's loop switches to the push form below this many frontier pairs (-1: automatic,
                                    // max(64, gpush_auto_factor pairs per sweep group); 0: never) -- dppr_set_group_push
    int gpush_list_cap = 1 << 20;   // vertices a frontier list of that form holds
    long long gpush_max_edges = 0;  // in-edges one iteration of that form may have (0: from the sweep's floor, 20 per sweep group)
    int gpush_auto_factor = 2;      // automatic threshold: this many pairs per sweep group (DPPR_GROUP_PUSH_FACTOR: tuning runs)
    // binned sweep of single-source loops on windows far beyond the L2s (dppr_binned.hpp, dppr_set_binned_sweep)
    int bin_mode = 1;               // 0: never, 1: when a source slot exists and the window has >= bin_min_ids vertices, 2: always
    int bin_ha_tiles = 128, bin_hb_tiles = 60; // an A-block holds at most 64 x ha_tiles heads (8 B of LDS each), a B-block 64 x hb_tiles rows (20 B each: 77 KB, two workgroups per CU)
    long long bin_target = 0;       // edges a B-block is cut for (one workgroup of k_bin_reduce); 0: from the window, clamp(Ed / 256, 16 K, 384 K)
                                    // (measured: LiveJournal stand-in best at 16-32 K, twitter / friendster at 192 K)
    long long bin_target_a = 4ll << 20; // ... an A-block (its edges are dealt to workgroups of k_bin_scatter in chunks: large, so that tiles are long runs)
    long long bin_min_ids = 1ll << 19; // (smaller windows run resident or gather: R-MAT window of 2 M edges, ~0.65 M ids, single source: binned 2.66 ms per batch
                                       // against 3.26 gathering; window of 1 M edges, ~0.38 M ids: 2.45 against 1.47 -- tools/r04/midsize_probe.sh)
    DevBuf<int> bin_vblk_a;      // vertex -> A-block (V ints; the B-block of a row is found by bisection, k_bin_keys)
    DevBuf<unsigned long long> bin_scan; // counts and scans of the tables' tail (4 x (Ed / 64 + 3) words)
    DevBuf<int> bin_small;       // quantile vertices | big rows | counter (bin_cut)
    long long bin_chunk = 32768;    // edges per workgroup of k_bin_scatter
    DevBuf<double> bin_vals;     // the values in B-major order: what pass 1 hands to pass 2 (one loop runs at a time)
    // the tables PATCHED per slide (dppr_binned.hpp, round 5): both orders persistent as sorted words under frozen block cuts
    DevBuf<uint64_t> bin_wb, bin_wa; // B-major / A-major words of the NEWEST epoch (rotate with keys_a / keys_b at a merge)
    DevBuf<int> bin_first;       // B-major run index of every block pair's first run: n_b x n_a ints (scratch of the tables' tail)
    std::vector<int32_t> bin_cut_a, bin_cut_b; // the cuts in use (first vertex of every block; frozen between re-cuts, extended by new ids)
    int bin_abits = 0, bin_bbits = 0;   // width of the block-number fields of the words (with room for appended blocks)
    int bin_cut_ids = 0;            // ids the cuts cover
    bool bin_words_valid = false;   // bin_wb / bin_wa describe the newest epoch under bin_cut_a / bin_cut_b
    int bin_slides_since_cut = 0;
    bool bin_incremental = true;    // DPPR_BIN_INCREMENTAL=0: every epoch's tables by the two sorts (rounds 3-4)
    int bin_recut_every = 32;       // slides between two fresh cuts (DPPR_BIN_RECUT_EVERY)
    bool bin_frozen_rebuild = false; // (tests, DPPR_BIN_FROZEN_REBUILD=1: the sorts, but under the frozen cuts -- what the patched tables must equal bit for bit)
    bool bin_force_full = false;    // the next build sorts afresh (a merge missed a key)
    int bin_miss_host = 0;
    long long bin_patched = 0, bin_rebuilt = 0; // epochs whose tables were patched / built by the sorts
    DevBuf<unsigned char> bin_tmp;
    size_t bin_tmp_bytes = 0;
    bool bin_ready = false;         // scratch allocated, kernels' LDS sizes registered
    std::vector<int32_t> h_tiles_in;
    // stream-update scratch
    DevBuf<uint32_t> su_k[2], su_v[2];
    DevBuf<double> su_term;
    DevBuf<uint8_t> su_ins;
    DevBuf<unsigned char> su_tmp;
    size_t su_tmp_bytes = 0;
    // staged batch (set_batch before slide)
    std::vector<int32_t> st_b1, st_b2;
    std::vector<uint8_t> st_ins;
    bool batch_staged = false;
    // epochs
    std::vector<Epoch> epochs;
    int newest = -1; // global id of newest epoch
    std::vector<Slot> slots;
    std::vector<Group> groups;
    PinBuf<int> pinned; // host-pinned readback words
    std::atomic<unsigned long long> heartbeat{0}; // bumped at every read-back of a frontier loop and every stage of a graph build (dppr_heartbeat)
    PinBuf<char> dump_pin;     // host-pinned landing area of dppr_debug_dump's device reads, owned by the engine for its whole life
    static constexpr size_t DUMP_PIN_BYTES = sizeof(GridBar) + 4096;
    // vertex compaction: external id <-> internal id (assigned on first appearance), live zone [0, n_int) and parked
    // zone [V - n_parked, V): IdSpace. Renumbering (dppr_builder.hpp) is decided here:
    bool renumber_on = true;       // dppr_set_renumbering
    int renumber_growth_pct = 15;  // a slide considers it once n_int has grown by this much since the last numbering ...
    int renumber_min_parked = 1024; // ... and does it if at least this many ids (and growth_pct / 2 % of the live ones) would be parked
    int renumber_next = 0;         // n_int at which the next slide looks at the live count
    int renumberings = 0;
    std::vector<int32_t> mv_src, mv_dst, mv_zero; // row moves of revived vertices being applied (flush_moves)
    DevBuf<int> mv_idx;         // device: src | dst | zero lists
    DevBuf<double> mv_tmp;      // device: the rows in flight
    DevBuf<int> d_ext2int;  // device copy of ext2int, refreshed on demand
    DevBuf<double> d_xfer;  // V doubles: staging of p / r in external order
    // queries of a state (dppr_host_query.hpp)
    DevBuf<int> d_int2ext;          // device copy of int2ext (live and parked zones), refreshed by the queries only
    unsigned i2e_gen_on_device = 0;    // IdSpace::map_gen that copy was taken at
    QueryWork q;                    // their workspace
    int walk_form = 0;              // 0: lane refill, 1: one walk per thread (dppr_debug_walk_form)
    int sg_wave_max = SG_WAVE_MAX;  // matched entries of a row up to which the wave that owns it places them (dppr_debug_subgraph_wave_max)
    int rk_piece = RK_PIECE;        // entries of a seed's row one wave of k_rk_mark walks (dppr_debug_rank_piece)
    int sample_form = 0;            // 0: a wave rebuilds a draw's lowest 8 levels, 1: one draw per thread over a fully stored tree (dppr_debug_sample_form)
    int pos_tile = 0;               // queries of a lane's order a workgroup of k_pos_count holds per pass; 0: the plan's choice (dppr_debug_position_tile)
    int ex_memo = -1;               // the memo of k_ex_path: -1 the plan's choice, 0 off, 1 on (dppr_debug_explain)
    int ex_wave_rows = EX_WAVE_ROWS; // entries of a row a wave of dppr_explain.hpp takes per step (dppr_debug_explain)
    int cert_piece = 0;             // edges of a piece of a long row in k_cert_rows; 0: the plan's choice (dppr_debug_certify)
    int cert_wave_rows = 0;         // short rows that share a wave of k_cert_rows; 0: the plan's choice (dppr_debug_certify)
    int fw_piece = 0;               // entries of a piece of a long in-row of the forward sweep; 0: the plan's choice (dppr_debug_forward)
    int fw_team = 0;                // lanes that share a gathered row there; 0: the plan's choice (dppr_debug_forward)
    int fp_piece = 0, fp_team = 0;  // the same two for the forward push (dppr_debug_forward_push)
    int fc_tile = 0, fc_piece = 0;  // the scan tile and the row piece of the forward track's sweep (dppr_debug_ftrack_cluster; 0: the plan decides)
    int fr_tile = 0;                // ids of a tile of the count / fill passes of the ranked queries over a forward track (dppr_debug_ftrack_rank; 0: the plan decides)
    int fp_chunk = 0;               // rounds of the forward push between two read-backs; 0: the plan's choice (dppr_debug_forward_push)
    dppr::FTrack ftracks[16];       // the forward tracks (DPPR_FTRACK_MAX)
    float ft_ms[4] = {-1.0f, -1.0f, -1.0f, -1.0f}; // dppr_set_profiling: device time of the last track call's load, fix-up, rounds, store (dppr_debug_ftrack_ms)
    float query_ms = -1.0f;         // dppr_set_profiling: device time of the last top-k, changes, export or dot call, first to last kernel (dppr_debug_query_ms)
    std::vector<int32_t> h_tmp1, h_tmp2;
    std::vector<int32_t> h_tiles; // host copy of the tile edge prefix / group table
    int max_iters = 1 << 20;
    std::string err;
};

namespace {

inline void set_err(dppr_engine *e, const char *msg) {
    std::lock_guard<std::mutex> lk(e->err_mu);
    e->err = msg;
}

// (`call`: a HIP call, or a buffer's alloc / regrow, whose int status is the policy's hipError_t)
#define HIP_TRY(call)                                                                                   \
    do {                                                                                                \
        const hipError_t _e = static_cast<hipError_t>(call);                                            \
        if (_e != hipSuccess) {                                                                         \
            char _b[512];                                                                               \
            snprintf(_b, sizeof(_b), "%s in %s at line %d", hipGetErrorString(_e), __FILE__, __LINE__); \
            set_err(e, _b);                                                                             \
            return _e == hipErrorOutOfMemory ? DPPR_ERR_NOMEM : DPPR_ERR_HIP;                           \
        }                                                                                               \
    } while (0)

// the same for calls whose message is "<prefix><HIP's words>" (no file / line): what a caller of those entry points reads today
#define HIP_TRY_MSG(prefix, call)                                                 \
    do {                                                                          \
        const hipError_t _e = static_cast<hipError_t>(call);                      \
        if (_e != hipSuccess) {                                                   \
            set_err(e, (std::string(prefix) + hipGetErrorString(_e)).c_str());    \
            return _e == hipErrorOutOfMemory ? DPPR_ERR_NOMEM : DPPR_ERR_HIP;     \
        }                                                                         \
    } while (0)

inline int grid_for(int64_t n, int per_block = BLOCK, int cap = 2048) {
    int64_t g = (n + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

// Wait for the engine's stream from inside a frontier loop (the read-back at the end of a chunk of iterations): polling the
// stream's completion instead of a blocking hipStreamSynchronize, whose wake-up is part of every chunk boundary's gap
// (DPPR_SYNC_SPIN=0: the blocking call, for A/B runs).
// The poll is bounded: a chunk of sweeps is over within a millisecond or two; after LOOP_SPIN_US the
// thread gives its core back and blocks -- N engines driven by N host threads (./pagerank -g N, two engines on one
// device) must not hold N cores at 100 % for a wait that has turned long.
constexpr long LOOP_SPIN_US = 2000; // (covers a resident launch of a configs[1]-size batch, ~0.4 ms: at 200 the blocking call's wake-up cost that path 6 %)
inline hipError_t loop_sync(hipStream_t st) {
    static const bool spin = !(getenv("DPPR_SYNC_SPIN") && atoi(getenv("DPPR_SYNC_SPIN")) == 0);
    if (!spin) return hipStreamSynchronize(st);
    timespec t0;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    hipError_t r;
    unsigned polls = 0;
    while ((r = hipStreamQuery(st)) == hipErrorNotReady) {
        if ((++polls & 15u) == 0) {
            timespec now;
            clock_gettime(CLOCK_MONOTONIC, &now);
            if ((now.tv_sec - t0.tv_sec) * 1000000L + (now.tv_nsec - t0.tv_nsec) / 1000L > LOOP_SPIN_US) return hipStreamSynchronize(st);
        }
        __builtin_ia32_pause();
    }
    return r;
}

inline hipError_t loop_wait(dppr_engine *e) { // a read-back of a frontier loop: a sign of life for a watchdog (dppr_heartbeat)
    e->heartbeat.fetch_add(1, std::memory_order_relaxed);
    return loop_sync(e->stream);
}

int fail(dppr_engine *e, int code, const char *msg) {
    if (e) set_err(e, msg);
    return code;
}

// The event bracket of a timed region on the solver's stream: what is enqueued between the two calls is what *ms reports, after
// ONE synchronisation at the close. (An error return between them leaves nothing to undo.)
inline int bracket_open(dppr_engine *e) {
    HIP_TRY(hipEventRecord(e->ev0, e->stream));
    return DPPR_OK;
}
inline int bracket_close(dppr_engine *e, float *ms) {
    HIP_TRY(hipEventRecord(e->ev1, e->stream));
    HIP_TRY(hipEventSynchronize(e->ev1));
    HIP_TRY(hipEventElapsedTime(ms, e->ev0, e->ev1));
    return DPPR_OK;
}
// ... closed at the end of a solve: converged at eps on that epoch; `counted`: the solve is a batch of the statistics
inline int solve_finished(dppr_engine *e, SolveState &o, double eps, int epoch_id, bool counted, float *out_ms) {
    float ms = 0;
    if (int rc = bracket_close(e, &ms)) return rc;
    if (out_ms) *out_ms = ms;
    if (counted) {
        o.st.gpu_ms += ms;
        o.st.batches++;
    }
    o.converged = true;
    o.conv_eps = eps;
    o.last_epoch = epoch_id;
    return DPPR_OK;
}

// dppr_hint_next_batch: the lookups of the NEXT batch's ids run on helper threads while dppr_update waits for the device. They
// only read the id maps; every path that changes the maps waits for them first (pre_join).
inline void pre_join(dppr_engine *e) {
    if (e->pre.task.valid()) e->pre.ok = e->pre.task.get();
}

inline int to_int(dppr_engine *e, int ext) { // (IdSpace: assigns, or revives a parked vertex)
    pre_join(e);
    return e->to_int(ext);
}

// a finished, still valid lookahead for exactly this array? (its index in e->pre, or -1)
int pre_find(dppr_engine *e, const int32_t *src, int n) {
    pre_join(e);
    if (!e->pre.armed || !e->pre.ok || e->pre.epoch != e->renumber_epoch || n <= 0) return -1;
    for (int k = 0; k < 4; ++k)
        if (e->pre.src[k] == src && e->pre.n[k] == n) {
            // same pointer, same length -- and still the same CONTENTS? (a caller that refilled the buffer without hinting again would get
            // the ids of the old contents: ADVICE r04.) First, last and strided samples: an id the lookup resolved maps back to src[i].
            const std::vector<int32_t> &o = e->pre.out[k];
            const int step = std::max(1, n / 64);
            for (int i = 0; i < n; i = (i + step < n || i == n - 1) ? i + step : n - 1) {
                const int m = o[(size_t)i];
                if (m >= 0 && (m >= (int)e->int2ext.size() || e->int2ext[(size_t)m] != src[i])) {
                    e->pre.armed = false; // stale: everything the hint holds is dropped
                    return -1;
                }
                if (i == n - 1) break;
            }
            return k;
        }
    return -1;
}

// ids inside [0, V)? (no side effect: a rejected call must not assign ids, revive parked vertices or queue row moves)
bool ids_in_range(dppr_engine *e, const int32_t *src, int n) {
    if (pre_find(e, src, n) >= 0) return true; // (the lookahead checked every id)
    for (int i = 0; i < n; ++i)
        if (src[i] < 0 || src[i] >= e->V) return false;
    return true;
}

// translate an id array; returns false (nothing changed) if any id is outside [0, V)
bool translate(dppr_engine *e, const int32_t *src, int n, std::vector<int32_t> &dst) {
    // looked up ahead of time (dppr_hint_next_batch) and still valid: no renumbering since (ids assigned or revived in between only
    // concern entries the lookup left at -1: those are resolved now, in array order, exactly as IdSpace::translate does)
    const int k = pre_find(e, src, n);
    if (k >= 0) {
        e->pre.src[k] = nullptr; // (consumed)
        dst.swap(e->pre.out[k]);
        e->resolve(src, dst.data(), e->pre.miss[k]);
        e->pre_hits++;
        e->pre_misses += (long long)e->pre.miss[k].size();
        return true;
    }
    // an array the lookahead does not cover: whatever it still holds is for calls that did not come -- drop it rather than let a
    // later call match a reused buffer by pointer and length alone
    if (n > 0) e->pre.armed = false;
    dst.resize((size_t)std::max(n, 1));
    return e->translate(src, (size_t)std::max(n, 0), dst.data());
}

} // namespace
