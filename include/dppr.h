/*
 * dppr.h -- C ABI of libdppr_hip.so: the MI355X-native dynamic reverse-push PPR
 * engine (hot path of guowentian/dynamicppr, gpu/ tree).
 *
 * Drop-in boundary. The reference has no FFI layer; its seam is the C++ virtual
 * interface PPRGPU::{GPUBuildSlidingGraph, IncrementalBatchUpdate,
 * ExecuteMainLoop(phase), ValidateResult} (gpu/PPRGPU.cuh:179-182) plus the data
 * handed across it (DeviceMemory, GPUEdgeBatch, SlidingGraphBuilder). Each entry
 * point below names the reference interface it replaces. The host program
 * (./pagerank, dynamicppr_amd/host/) and any other binding call only this.
 *
 * Conventions: plain pointers and sizes, no C++ or torch types. Every function
 * returns 0 (DPPR_OK) or a negative dppr_status; nothing exits the process (the
 * reference prints and exit(-1)s, gpu/GPUUtil.cuh:7-19). An engine is confined to
 * one host thread -- except for the builder / solver pair of dppr_slide_concurrent and the
 * helper of dppr_hint_next_batch --; engines on different devices are independent. Host buffers are
 * borrowed for the duration of the call only (as EdgeBatch arrays are,
 * SlidingGraphVec.h:17-26). All device memory is owned by the engine
 * (DeviceMemory / SlidingGraphBuilder ownership, gpu/DeviceMemory.cuh:31-50).
 *
 * Index type int32, value type double, ALPHA = 0.15 (Meta.h:25-31).
 */
#ifndef DPPR_H
#define DPPR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPPR_ABI_VERSION 6

typedef struct dppr_engine dppr_engine; /* opaque */

typedef enum dppr_status {
    DPPR_OK = 0,
    DPPR_ERR_INVALID = -1,   /* bad argument / call order */
    DPPR_ERR_HIP = -2,       /* a HIP runtime call failed (see dppr_last_error) */
    DPPR_ERR_NOMEM = -3,
    DPPR_ERR_NO_DEVICE = -4, /* no usable gfx950 device: the HIP path is mandatory, no CPU fallback */
    DPPR_ERR_NOT_CONVERGED = -5 /* iteration cap hit */
} dppr_status;

/* Push schedule. Both are legal interleavings of the reference kernels
 * (gpu/ExpandRev.cuh:8-183 + :708-743); see DESIGN.md "Schedules".
 *   EAGER : sparse (push) iterations take a frontier vertex's residual with an atomic
 *           exchange at the moment it is pushed (reads whatever has arrived, like the
 *           racy `ru = residual[u]` of ExpandUnifiedRev); dense iterations run as pull
 *           sweeps, which are synchronous by construction. Production mode.
 *   SYNC  : every frontier residual is snapshotted before any push of the iteration
 *           lands, in sparse iterations too; results are independent of thread
 *           scheduling up to the rounding of the sums, and the per-iteration frontier
 *           SETS equal the oracle's synchronous schedule exactly. Validation mode. */
#define DPPR_SCHEDULE_EAGER 0
#define DPPR_SCHEDULE_SYNC 1

typedef struct dppr_stats_t {
    int64_t iterations;   /* frontier-loop iterations (both phases) since last reset */
    int64_t sum_F;        /* sum of frontier sizes */
    int64_t sum_E;        /* traversed in-edges */
    int64_t sum_N;        /* vertices enqueued into next frontiers */
    int64_t records;      /* batch records applied by IncrementalBatchUpdate */
    int64_t inspected;    /* vertices scanned by full Inspect passes */
    int64_t batches;      /* dppr_update calls */
    int64_t pull_iterations; /* iterations evaluated as a dense pull sweep (subset of iterations) */
    int64_t algorithmic_bytes; /* 8 * inspected + 45 * records + sum(72F + 24E + 4N) */
    double gpu_ms;        /* sum of event-timed regions */
    double push_ms;       /* sum of per-launch event times of the push kernel (profiling on only) */
    int64_t push_launches; /* push-kernel launches timed into push_ms */
    int64_t persist_launches; /* launches of the resident multi-iteration sweep (k_pull_resident) */
    int64_t persist_aborts;   /* of those, launches that stopped at a grid-barrier time-out */
    int64_t binned_sweeps;    /* pull iterations evaluated as a binned sweep (k_bin_scatter + k_bin_reduce; subset of pull_iterations) */
    /* ABI 3: the dense sweeps on their own (one launch per sweep: k_pull_iter, k_bin_scatter + k_bin_reduce, k_gsweep), so that
     * the roofline of the sweep kernel is its own bytes over its own time, reproducible from a rocprofv3 kernel-stats file */
    int64_t sweep_F;          /* sum of the frontier sizes the sweeps pushed (subset of sum_F) */
    int64_t sweep_E;          /* in-edges the sweeps traversed (subset of sum_E) */
    double sweep_ms;          /* sum of the sweeps' event times (profiling on only; subset of push_ms) */
    int64_t sweep_launches;   /* sweeps timed into sweep_ms */
} dppr_stats_t;

/* ---- lifetime ----------------------------------------------------------- */

/* HIP devices visible to the process (0 when there is none or the runtime fails): lets a host program that has no HIP of
 * its own map `-g N` device threads onto the devices that exist. No reference counterpart (single implicit device 0). */
int dppr_device_count(void);

/* IncrementalBatchUpdate replays a batch's records tail by tail, each tail's records in batch order (lock-free; the
 * reference serialises them with a spin lock per tail, gpu/StreamUpdate.cuh:50-72), after CopyOutDegree (gpu/StreamUpdate.cuh:7-17).
 * at_slide = 0 (DEFAULT since ABI 4): both run inside dppr_update / dppr_group_update / dppr_incremental_batch_update -- the
 * reference's bracket (gpu/PPRGPU.cuh:138-164 times all of IncrementalBatchUpdate). The grouping's contract: equal tails are
 * contiguous and keep batch order; the order of the tails depends on the path. Up to 4 Ki records (SU_RANK_MAX) it is one ranking
 * launch (k_su_group_rank; tails ascending); up to 4 Mi records (SU_GRP_MAX_RECORDS) records go into buckets by the low bits of the
 * tail and are ranked inside them (tails ascending only inside a bucket), unless one bucket would hold more than 16 Ki records
 * (SU_GRP_MAX_BUCKET: a hot tail); those batches and longer ones go through the device radix sort (tails ascending). A whole-batch
 * resident launch takes the records raw and groups them itself (dppr_resident.hpp). at_slide = 1 (rounds 3-4): the grouping and the degree gather, functions of the batch
 * alone, are done when the batch is uploaded (dppr_slide; for epochs that already exist: on entry to the next call, BEFORE its
 * event bracket opens) and the timed region holds only the replay. Same results bit for bit. */
int dppr_set_batch_grouping(dppr_engine *e, int at_slide);

/* The reference's four variants (-o, Meta.h; gpu/PPRRevPushGPUVariants.cuh:6-150) as MECHANISMS of the push iterations:
 *   0 OPTIMIZED     eager residual read + threshold-crossing duplicate filter (ExpandUnifiedRev + RepairFrontierRev)      [default]
 *   1 FAST_FRONTIER residuals pre-extracted and zeroed at the snapshot (InspectExtra, gpu/Inspect.cuh:51-65), crossing filter, no repair
 *   2 EAGER         eager read + STATUS-ARRAY filter: legal(curr) && atomicExch(status[v], level) < level (gpu/ExpandRev.cuh:255,298,340)
 *   3 VANILLA       pre-extracted + status-array filter (gpu/ExpandRev.cuh:603,646,688)
 * 1 and 3 imply the synchronous schedule, 0 and 2 the eager one (dppr_set_schedule may be called afterwards). Dense iterations
 * run as sweeps in every variant (a sweep computes the next frontier directly and needs neither filter): to time the four
 * mechanisms against each other, as the paper's ablation does, pin the push form (dppr_set_tuning pull_min_frontier = -1,
 * ./pagerank --push-only). Results: the variants' frontier SETS per iteration equal the oracle's restatements of the reference's
 * variants (tests); p / r as for the two schedules. */
int dppr_set_variant(dppr_engine *e, int variant);

/* MERGED LOOP (off by default; not the reference's schedule). The reference pushes the positive residuals of a batch to
 * convergence (ExecuteMainLoop(0)) and then the negative ones (ExecuteMainLoop(1), gpu/PPRGPU.cuh:138-164). Both loops
 * spread the same batch's disturbance over the same part of the graph, and most of what they move cancels: with
 * on != 0, dppr_update / dppr_group_update (eager schedule) run ONE loop that pushes every residual with |r| > eps',
 * eps' = eps / eps_divisor (0 keeps the divisor; default 4). Every push is the reference's push (gpu/ExpandRev.cuh:70-77,
 * :708-743), the loop invariant of SURVEY.md section 0 holds after every iteration, and the state it ends in satisfies
 * |r| <= eps' < eps -- a state the reference's own Validate() accepts (cpu/PPRCPUMTCilkRev.h:291-309), closer to the
 * fixed point than the reference's result (LiveJournal stand-in, eps 1e-9: max |p - p_cilk| 4.8e-10 with divisor 4;
 * 7.7e-10 with divisor 1) in a third to a half of the sweeps. The split interface (dppr_incremental_batch_update +
 * dppr_execute_main_loop(0 / 1)) and the synchronous schedule always run the reference's two loops. */
int dppr_set_phase_merge(dppr_engine *e, int on, int eps_divisor);

/* Replaces: DeviceMemory ctor + CudaAllocAppData + InitForDynamicGraph
 * (gpu/DeviceMemory.cuh:9-74) and SlidingGraphBuilder ctor
 * (gpu/SlidingGraphBuilder.cuh:64-76), as called from PPRGPU ctor
 * (gpu/PPRGPU.cuh:23-34).
 *   window_edges : W, the sliding window size in STREAM edges (undirected streams
 *                  are mirrored inside, as InitWindowStream does)
 *   max_batch    : c, stream edges per batch (edge batches hold up to 4c records)
 *   n_epochs     : how many graph epochs (CSR + batch records) stay resident in
 *                  HBM; 1 = rebuild in place like the reference, K+1 lets a caller
 *                  pre-stage K batches and then run the timed path back to back. */
int dppr_create(dppr_engine **out, int device, int32_t vertex_count, int32_t window_edges,
                int directed, int32_t max_batch, int32_t n_epochs);
void dppr_destroy(dppr_engine *e);
const char *dppr_strerror(int status);
const char *dppr_last_error(const dppr_engine *e); /* detail of the last failure */
int dppr_abi_version(void);
int dppr_set_schedule(dppr_engine *e, int schedule);
/* When on, every launch of the push kernel (the dominant kernel) is bracketed by its own
 * hipEvent pair on the engine's stream and summed into dppr_stats_t.push_ms. Off by default
 * (the extra events perturb the whole-batch time slightly). */
int dppr_set_profiling(dppr_engine *e, int on);
/* Execution-path knobs (defaults 256 / 512 / 0); only valid right after dppr_create.
 * hub_min_degree: out-degree from which a vertex's incoming pushes are aggregated in LDS (at
 * most 2048 hubs per epoch); big_row_edges: in-degree from which a frontier vertex's row is
 * expanded by the whole grid; pull_min_frontier: frontier size from which an iteration is
 * evaluated as a dense pull sweep instead of push atomics (0 = auto: max(1024, edges/192),
 * negative = never); chunk_iters: iterations enqueued per host read-back of the frontier size
 * (default 24, 1 = read back every iteration like the reference, <= 0 keeps the default; an
 * explicit value also caps the sweeps a resident launch may run before the host looks);
 * pull_block: workgroup size of the sweep, 256 / 512 / 1024 (0 = chosen from the graph size).
 * Results never depend on them beyond floating-point summation order; tests set them so
 * small graphs exercise every path. */
int dppr_set_tuning(dppr_engine *e, int hub_min_degree, int big_row_edges, int pull_min_frontier,
                    int chunk_iters, int pull_block);
/* Resident sweeps: when a window's sweep groups all fit on the chip at once, a run of dense
 * iterations is ONE launch that keeps the per-vertex state on chip; workgroups exchange the
 * per-iteration snapshot through memory and wait for each other's values, not for the host (no
 * counterpart in the reference, whose loop reads the frontier size back after every iteration,
 * gpu/PPRRevPushGPU.cuh:107). mode 1 = automatic (default; in the steady
 * state of a stream the launches of BOTH phases of a batch are enqueued ahead, without a
 * read-back in between), 2 = resident launches but one host read-back per launch, 0 = never
 * (every iteration its own launch). Such a launch first checks that all its workgroups are
 * running (waiting on one another needs that); timeout_us is how long that roll-call may take before the
 * launch gives up WITHOUT having changed anything and the engine continues with per-iteration
 * launches, trying resident ones again 64 batches later (0 keeps the default, 50 ms; negative = a roll-call that cannot succeed, which tests
 * use to exercise that path; the results are the same either way).
 * Only valid right after dppr_create. */
int dppr_set_persistent(dppr_engine *e, int mode, int64_t timeout_us);

/* Single-source per-iteration sweeps (windows too large for a resident launch) can test an activity
 * bitmap of the snapshot (1 bit per vertex, L2-resident) before each 8-byte gather of x[u], so that
 * heads outside the frontier cost no random sector (k_pull_iter<.., true>). Off by default: on the
 * LiveJournal and twitter stand-ins it fetches 30 % / 0 % fewer bytes and is 0 % / 23 % SLOWER (the
 * extra dependent L2 round trip per edge costs more than the sectors it saves; profiles/r02_pmc_*_bits*).
 * Source groups always use their bitmap (dppr_multi.hpp). Results are identical either way. */
int dppr_set_sweep_bitmap(dppr_engine *e, int on);

/* Single-source dense iterations on windows whose snapshot vector is far beyond the L2s run as a BINNED
 * (propagation-blocked) sweep: two streaming passes over a per-epoch layout of the window's edges instead of one
 * random 64-byte sector per edge (dppr_binned.hpp: k_bin_scatter + k_bin_reduce replace k_pull_iter; the per-edge
 * term is still gpu/ExpandRev.cuh:72's expression, results equal k_pull_iter's up to the order of each row's sum).
 *   mode         : 0 never, 1 (default) when a source slot exists and the window has at least min_ids vertices with
 *                  an id, 2 always (tests: tiny windows)
 *   ha_tiles     : an A-block holds at most 64 x ha_tiles heads (8 bytes of LDS per head; 0 keeps the default, 128)
 *   hb_tiles     : a B-block holds at most 64 x hb_tiles rows (20 bytes of LDS per row; 0 keeps 60 = 77 KB, two workgroups per CU)
 *   target_edges : edges a B-block is cut for (0 keeps the automatic choice, clamp(window edges / 256, 16 Ki, 384 Ki): twitter stand-in,
 *                  single source, 192 Ki / 384 Ki / 768 Ki: 74.6 / 70.2 / 77.7 ms per batch); a row of a quarter of that is a block of its own
 *   min_ids      : mode 1 threshold (0 keeps 1 Mi vertices with an id: smaller windows run resident or cannot fill the chip with blocks)
 *   chunk_edges  : runs (one head into one B-block: the unit x[u] travels in since ABI 5) per workgroup of k_bin_scatter (0 keeps 32768)
 *   target_a_edges : edges an A-block is cut for (0 keeps 4 Mi: large, the longer the runs a tile's values are written in)
 * The layout costs at most 4 bytes per window edge and epoch (2 per edge + 2 per run + 4 per tile) plus 32 bytes per window edge of engine
 * state (the values of pass 1, and both orders of the window's edges as sorted words), and is built in dppr_load_window and PATCHED by
 * dppr_slide (untimed, like the CSRs):
 * a slide merges the words of its retired and inserted edges into the two orders instead of sorting the window twice; the block
 * cuts are renewed every 32 slides (DPPR_BIN_RECUT_EVERY; DPPR_BIN_INCREMENTAL=0: the sorts every epoch). Only valid right after dppr_create. */
int dppr_set_binned_sweep(dppr_engine *e, int mode, int ha_tiles, int hb_tiles, int64_t target_edges, int64_t min_ids,
                          int64_t chunk_edges, int64_t target_a_edges);

/* ---- graph side (UNTIMED in the reference's metric) --------------------- */

/* Replaces: SlidingGraphBuilder::InitWindowStream (gpu/SlidingGraphBuilder.cuh:182-192)
 * + BuildInGraph (:137-153) / DeviceMemory::CudaMemcpyGraph (gpu/DeviceMemory.cuh:76-112).
 * e1/e2: the n == W window edges in stream order, NOT mirrored. Builds epoch 0. */
int dppr_load_window(dppr_engine *e, const int32_t *e1, const int32_t *e2, int32_t n);

/* Replaces: GPUEdgeBatch::CudaMemcpy(EdgeBatch*, HostToDevice) (gpu/GPUEdgeBatch.cuh:20-26).
 * The L = 2c (directed) or 4c (undirected) records exactly as
 * SlidingGraphVec::StreamUpdates lays them out (SlidingGraphVec.h:241-272):
 * [c deletes][c inserts] then the mirrored copy. Stages them for the NEXT epoch. */
int dppr_set_batch(dppr_engine *e, const int32_t *edge1, const int32_t *edge2,
                   const uint8_t *is_insert, int32_t length);

/* Replaces: SlidingGraphBuilder::IncBuildInGraph(new_stream, ...)
 * (gpu/SlidingGraphBuilder.cuh:117-133, :163-181, :193-221) = PPRGPU::GPUBuildSlidingGraph.
 * Drops the c oldest window edges, appends the c new ones, rebuilds the in-CSR
 * (rows sorted ascending like the reference's pair sort) and the out-degrees, and
 * makes the result the newest epoch. Call after dppr_set_batch. *out_epoch (may be
 * NULL) receives the new epoch id. */
int dppr_slide(dppr_engine *e, const int32_t *new_e1, const int32_t *new_e2, int32_t c,
               int32_t *out_epoch);

/* The same graph update, allowed to run CONCURRENTLY with one solver call on an OLDER epoch (ABI 4; the overlap of the reference's
 * untimed region, gpu/PPRGPU.cuh:114-135, with its timed one). Contract: ONE builder thread (dppr_set_batch +
 * dppr_slide_concurrent for batch k + 1) beside ONE solver thread (dppr_update / dppr_group_update / dppr_incremental_batch_update /
 * dppr_execute_main_loop / dppr_read / dppr_stats with an EXPLICIT epoch id <= k; never -1 = "newest", which the builder is
 * changing); the solver must not be given epoch k + 1 before this call has returned; n_epochs >= 2 (epoch k + 1 takes the ring
 * entry of epoch k + 1 - n_epochs, which nothing may still be solving on). The builder works on its own HIP stream and scratch;
 * what it shares with the solver are the state rows of vertices that are NEW or REVIVED in batch k + 1, which no older epoch
 * touches. Such a slide never renumbers the id space and never grows the resident-launch arena: when dppr_renumbering_due(e)
 * says so, make the next graph update an exclusive dppr_slide (after the solver call has returned). Same results.
 * dppr_read / dppr_group_read beside the builder (ABI 5): the engine holds its id-map lock from the first id a batch assigns or revives
 * to the end of the row moves that go with it, and a read holds it from its copy of the map to the end of its gathers -- a read sees
 * the id space of before a revival or of after it, never a mixture (it may wait for the builder's id-assigning head, never for the
 * graph build itself). */
int dppr_slide_concurrent(dppr_engine *e, const int32_t *new_e1, const int32_t *new_e2, int32_t c, int32_t *out_epoch);
int dppr_renumbering_due(const dppr_engine *e);

/* How dppr_slide maintains the device CSR. on (default): the previous epoch's sorted edge keys
 * are kept and the batch is merged in (sort of the 2c batch keys + mark + select + merge, O(Ed)
 * streaming). off: the whole window is re-sorted every batch, which is what the reference does
 * (thrust::sort in BuildCSRGraph, gpu/SlidingGraphBuilder.cuh:203-221). Same CSR either way. */
int dppr_set_incremental_graph(dppr_engine *e, int on);

/* Renumbering of the internal vertex ids (no counterpart in the reference, whose kernels scan all V ids every
 * iteration: gpu/Inspect.cuh:8-48). The engine numbers vertices by first appearance and sweeps only those ids; a
 * vertex whose last edge left the window keeps p / r, so on a long stream the id space outgrows the vertices that
 * still have edges. on (default): a dppr_slide that finds EVERY source slot / group converged on the newest epoch,
 * the id space grown by growth_pct % (default 15) since the last numbering and at least min_parked (default 1024,
 * and growth_pct / 2 % of the live vertices) ids without an edge, renumbers: live vertices first, the others parked at the top
 * of the id capacity with their state rows, outside of every sweep; a parked vertex that shows up in a later batch
 * gets a fresh id and its rows back. Results are those of a run without renumbering; older epochs become
 * unavailable at that slide (they are in the old numbering), which is why slots that lag behind block it.
 * growth_pct / min_parked = 0 keep their current values. */
int dppr_set_renumbering(dppr_engine *e, int on, int growth_pct, int min_parked);
/* ids in use by sweeps and scans, parked ids, renumberings so far, parked vertices that came back (any may be NULL) */
int dppr_id_space(dppr_engine *e, int32_t *n_ids, int32_t *n_parked, int32_t *renumberings, int64_t *revivals);

/* ---- per-source state ---------------------------------------------------- */

/* Allocates pagerank/residual/frontier state for one source vertex
 * (DeviceMemory::CudaAllocAppData, gpu/DeviceMemory.cuh:51-63). */
int dppr_add_source(dppr_engine *e, int32_t source_vertex, int32_t *out_slot);

/* Replaces: Init<<<>>> + ExecuteMainLoop(0) of PPRGPU::DynamicExecute
 * (gpu/PPRGPU.cuh:85-89, gpu/PPRCommon.cuh:12-22). Runs on the newest epoch. */
int dppr_init_solve(dppr_engine *e, int32_t slot, double eps, float *out_ms);
/* ... on a given resident epoch (-1: the newest, as dppr_init_solve): a source added after several epochs were pre-staged starts
 * from the first of them and follows them with dppr_update in sequence. */
int dppr_init_solve_at(dppr_engine *e, int32_t slot, int32_t epoch, double eps, float *out_ms);

/* THE TIMED REGION of the reference (gpu/PPRGPU.cuh:138-164):
 * IncrementalBatchUpdate + ExecuteMainLoop(0) + ExecuteMainLoop(1) for one batch.
 * epoch < 0 means the newest epoch. *out_ms = hipEvent time of exactly that region
 * (batch upload and CSR rebuild excluded, as in the reference). */
int dppr_update(dppr_engine *e, int32_t slot, int32_t epoch, double eps, float *out_ms);
/* (Epochs must be applied to a source in sequence: after the solve / update on epoch k only epoch
 * k + 1 is accepted, DPPR_ERR_INVALID otherwise -- with several epochs resident a skipped or replayed
 * batch would otherwise go unnoticed. dppr_write resets that memory. The same holds for
 * dppr_incremental_batch_update and dppr_group_update.) */

/* The same region split along the reference's virtual interface, for callers that
 * keep the reference's driver loop and for kernel-level parity tests:
 *   PPRRevPushGPU::IncrementalBatchUpdate (gpu/PPRRevPushGPU.cuh:21-28,
 *     gpu/StreamUpdate.cuh:7-76)
 *   PPRRevPushGPU::ExecuteMainLoop(phase) (gpu/PPRRevPushGPU.cuh:97-131): full
 *     Inspect over V, then the Expand/Repair frontier loop. */
int dppr_incremental_batch_update(dppr_engine *e, int32_t slot, int32_t epoch);
/* Test hook: the frontier seeds dppr_incremental_batch_update derived from the batch when the state
 * was converged before it -- phase 0: tails with r > eps, phase 1: tails with r < -eps (eps = that of
 * the completed solve). This is what cpu/PPRCPUMTCilkRev.h:126-156 (DynPushInit) builds from the batch
 * endpoints; unordered. Valid only between that call and the next main loop / update. */
int dppr_seed_lists(dppr_engine *e, int32_t slot, int phase, int32_t *out_ids, int32_t *out_count);
int dppr_execute_main_loop(dppr_engine *e, int32_t slot, int32_t epoch, int phase, double eps);

/* Replaces: the cudaMemcpy D2H of pagerank/residual in ValidateResult
 * (gpu/PPRRevPushGPU.cuh:136-139). p and r each hold vertex_count doubles. */
int dppr_read(dppr_engine *e, int32_t slot, double *p, double *r);
/* Overwrite p/r (test hook: lets a kernel be checked from an arbitrary state). */
int dppr_write(dppr_engine *e, int32_t slot, const double *p, const double *r);

int dppr_stats(dppr_engine *e, int32_t slot, dppr_stats_t *out);
int dppr_reset_stats(dppr_engine *e, int32_t slot);

/* ---- source groups (multi-source batched sweeps) ---------------------------------------
 * Up to 16 sources that share the engine's graph are solved TOGETHER: their p / r / x vectors are
 * interleaved (8 doubles = one 64-byte sector per vertex for up to 8 sources, 16 doubles = one
 * 128-byte line for 9..16), so one pass over the out-CSR serves all of them (BASELINE.json configs
 * 3 and 5 run 10 sources over the same stream). Per source the arithmetic and the results are those
 * of the single-source calls; group iterations are always sweeps, and an activity bitmap keeps a
 * sweep's cost proportional to what the frontiers touch (dppr_multi.hpp). The reference has no
 * counterpart (one source per process, gpu/PPRGPU.cuh:24). */
int dppr_add_source_group(dppr_engine *e, const int32_t *sources, int32_t n /* 1..16 */, int32_t *out_group);
int dppr_group_init_solve(dppr_engine *e, int32_t group, double eps, float *out_ms);
int dppr_group_init_solve_at(dppr_engine *e, int32_t group, int32_t epoch, double eps, float *out_ms); /* (as dppr_init_solve_at) */
/* timed region for all sources of the group at once (same scope as dppr_update) */
int dppr_group_update(dppr_engine *e, int32_t group, int32_t epoch, double eps, float *out_ms);
int dppr_group_read(dppr_engine *e, int32_t group, int32_t index, double *p, double *r);
int dppr_group_stats(dppr_engine *e, int32_t group, dppr_stats_t *out); /* summed over the sources */
int dppr_group_reset_stats(dppr_engine *e, int32_t group);

/* ---- sources of a running group: replace, add, drop (backward-compatible additions, ABI 6) ----
 * A group's set of sources may change while the stream runs, without a second group and without re-solving the
 * sources that stay. The reference has no counterpart (one source per process, gpu/PPRGPU.cuh:24).
 *
 * Common contract. The group must be converged (a completed dppr_group_init_solve / dppr_group_update) and the
 * epoch it was last solved on must still be resident, DPPR_ERR_INVALID otherwise. A new source's column is solved
 * from scratch ON THAT EPOCH -- Init + ExecuteMainLoop(0) for that source, exactly as dppr_group_init_solve_at runs
 * them (gpu/PPRCommon.cuh:12-22, gpu/PPRRevPushGPU.cuh:97-131) -- with the tolerance the group is converged to:
 * there is no eps argument, any other value would either move the other columns or leave the group with two
 * tolerances. The other sources are not changed by value: p and r as dppr_group_read returns them are equal
 * before and after, element for element (their columns fail the legal-push test in every sweep of the loop).
 * Afterwards the group is converged at the same tolerance on the same epoch, and the next dppr_group_update
 * seeds from the batch tails as before.
 * EXCLUSIVE calls, like dppr_add_source_group: they assign or revive vertex ids, move state rows and may re-cut
 * the sweep groups of every resident epoch -- never beside dppr_slide_concurrent or any other call on the engine.
 * Every argument is checked first and a rejected call touches nothing (no id assigned, no parked vertex revived,
 * no row moved): a bad group or index, a source outside [0, V), a group that is not converged, an epoch that is
 * gone, add at 16 sources, remove at 1 source -- all DPPR_ERR_INVALID. Every buffer a call needs is obtained
 * before anything changes: after DPPR_ERR_NOMEM the group is exactly as before.
 * *out_ms (may be NULL): hipEvent time of the device work -- the column's init, the re-interleaving of the rows
 * where the row width changes, the column's frontier loop; the sweep-group re-cut that a fresh vertex id or the
 * first group of more than 8 sources needs is builder work and stays outside, as everywhere else. dppr_group_stats:
 * the loop's iterations, sum_F, sum_E, sum_N, inspected and sweep fields are added; batches, records and gpu_ms
 * describe dppr_group_update and are not. */
/* The external ids of the group's sources in lane order (the `index` of dppr_group_read) and their number. */
int dppr_group_sources(dppr_engine *e, int32_t group, int32_t *out_sources /* [16], may be NULL */, int32_t *out_n);
/* Lane `index` becomes new_source; the row width stays, nothing is re-interleaved. The vertex the lane had before, or
 * one another lane has, is allowed and means a re-solve of that lane. Drops the group's mark (dppr_group_mark): a
 * lane changes meaning. */
int dppr_group_replace_source(dppr_engine *e, int32_t group, int32_t index, int32_t new_source, float *out_ms);
/* One more source; it takes index n (*out_index, may be NULL). An odd group's padding double is taken into use as it
 * is (re-initialised), otherwise p / r are re-interleaved to rows of two more doubles in one streaming pass each
 * (the old and the new rows exist side by side during the call). The ninth source makes the group a wide one
 * (16-byte lanes; sweep groups of at most 512 vertices on this engine from then on). Drops the group's mark
 * (dppr_group_mark): the rows change width. */
int dppr_group_add_source(dppr_engine *e, int32_t group, int32_t new_source, int32_t *out_index, float *out_ms);
/* Drops source `index`. The sources behind it move down by one -- the order is kept, THE CALLER'S HIGHER INDICES
 * DECREASE BY 1 -- and the rows are re-interleaved to the width of n - 1 sources, which gives the memory back.
 * The dropped vertex no longer counts as in use when the ids are renumbered. No loop runs. Drops the group's mark
 * (dppr_group_mark): the lanes behind the dropped one change meaning. */
int dppr_group_remove_source(dppr_engine *e, int32_t group, int32_t index);

/* ---- weighted vertex sets as the targets of a group (backward-compatible additions, ABI 6) ----
 * A lane of a group need not stand for one vertex: it may track the PPR towards a WEIGHTED SET of vertices (a community,
 * a labelled class -- one lane per class, the argmax over the lanes is label propagation on a live stream --, a block
 * list, a topic) with up to DPPR_TARGET_SET_MAX seeds, solved and kept current by the same sweeps as a source lane. The
 * reference has no counterpart (one source vertex per process, gpu/PPRGPU.cuh:24).
 *
 * THE LANE. With the seed vector h (h[v] = the weight of seed v, 0.0 elsewhere) the lane keeps the engine's invariant
 * with the indicator of the source replaced by h:
 *     p[u] + ALPHA * r[u] == ALPHA * h[u] + (1 - ALPHA) / (outdeg(u) + 1) * sum over v in out(u) of p[v]
 * Init is p = 0, r = h (gpu/PPRCommon.cuh:12-22 with h for e_s) and the stream update's source term is ALPHA * h[u]
 * (gpu/StreamUpdate.cuh:50-72 with h[u] for [u == s]). PPR IS LINEAR IN THE TARGET: the lane converges to
 * sum_v h[v] * p_v, p_v being the column a source lane of v would hold, and a converged lane (max|r| <= eps) satisfies
 * |p - exact| < eps FOR ANY h -- with e = p - exact and M the row-substochastic operator of the invariant,
 * e = M e - ALPHA r, hence |e|_inf <= |r|_inf --, so the weights need not sum to 1 and the tolerance means what it
 * means for a source. Weights must be finite and > 0: Init leaves r = h >= 0 and dppr_group_init_solve_at runs the
 * loop of the positive residuals only. Every query of a group (top-k, weighted top-k, changes, export, dot, refine,
 * cluster, subgraph, point reads) reads p / r rows and works on a set lane unchanged.
 * Every seed vertex receives an internal id when the set is given (a seed outside the window too; a parked one is
 * revived) and counts as in use when the ids are renumbered, like a source: it is never parked while its lane has it.
 *
 * A lane of ONE seed of weight exactly 1.0 is a source lane. A group made only of such lanes IS a group of
 * dppr_add_source_group: the same state, the same kernels, the same results bit for bit.
 *
 * dppr_add_target_group: n lanes, lane i with the seeds ids[offsets[i] .. offsets[i + 1]) and their weights; offsets is
 * [n + 1], HOST memory like the arrays. Otherwise as dppr_add_source_group (an EXCLUSIVE call).
 * dppr_group_replace_target: the contract of dppr_group_replace_source (the group converged, its epoch resident, an
 * EXCLUSIVE call; no eps argument) with a seed set for the vertex: lane `index` is re-initialised to p = 0, r = h and
 * solved on that epoch at the group's tolerance. The other lanes are not changed by value, bit for bit. Drops the
 * group's mark. The seeds the lane had before no longer count as in use.
 * dppr_group_targets: the seed sets in lane order, external ids ascending within a lane: lane i occupies
 * [out_offsets[i], out_offsets[i + 1]) of out_ids and out_weights. out_offsets is [17], HOST memory, and is ALWAYS written
 * with the true offsets (entries beyond the group's lanes repeat the total). Capacity as for the sparse exports: if
 * out_offsets[16] > cap nothing is written to out_ids / out_weights and the call still returns DPPR_OK; cap = 0 with
 * NULL arrays is the size query. A source lane is listed as its vertex with weight 1.0.
 * dppr_group_sources reports -1 for a lane that is not a single seed of weight 1.0. dppr_group_replace_source may
 * replace a set lane (it becomes a source lane); dppr_group_add_source and dppr_group_remove_source carry the other
 * lanes' sets along, a removal moving the sets behind the dropped lane down by one with their lanes.
 *
 * Rejected with DPPR_ERR_INVALID before any device work or id assignment, nothing touched: n outside [1, 16]; a NULL
 * offsets, ids or weights; offsets that do not start at 0 or decrease; a lane with no seed or more than
 * DPPR_TARGET_SET_MAX; an id outside [0, V); an id twice within a lane (the same id in different lanes is fine); a
 * weight that is not finite or not > 0; and what dppr_group_replace_source rejects. dppr_group_targets: a NULL
 * out_offsets, cap < 0, cap > 0 with a NULL array. Every buffer a call needs -- the seed table of 12 bytes per seed
 * included -- is obtained before anything changes: after DPPR_ERR_NOMEM the engine is as it was before the call. */
#define DPPR_TARGET_SET_MAX 65536
int dppr_add_target_group(dppr_engine *e, const int64_t *offsets /* [n + 1], HOST */, const int32_t *ids, const double *weights,
                          int32_t n /* 1..16 */, int32_t *out_group);
int dppr_group_replace_target(dppr_engine *e, int32_t group, int32_t index, const int32_t *ids, const double *weights,
                              int32_t m /* 1..DPPR_TARGET_SET_MAX */, float *out_ms);
int dppr_group_targets(dppr_engine *e, int32_t group, int64_t *out_offsets /* [17], HOST */, int32_t *out_ids, double *out_weights,
                       int64_t cap);

/* ---- queries of a state: top-k and point reads (added in ABI 6, backward compatible) ----
 * The answer a dense dppr_read / dppr_group_read would give, without moving V doubles per source to the
 * host: a radix select runs on the device over the rows that hold a vertex (the live and the parked
 * zone), two streaming passes over p for all sources of a group at once (dppr_topk.hpp), and one copy of
 * the n x k results comes back.
 *
 * dppr_topk / dppr_group_topk: for each source the qualifying vertices are the external ids v with
 * p[v] > min_p, p being exactly what dppr_read / dppr_group_read returns. They are ordered by p
 * descending, then external id ascending, and the first min(k, #qualifying) are returned with their
 * count: ids, the stored p (bit for bit, not recomputed) and, if out_r is not NULL, r at those vertices.
 * Entries of a row past its count hold id -1 and 0.0. Group outputs are source-major: [n][k], counts [n].
 * Since min_p >= 0, a vertex without an internal id (p exactly 0.0) never qualifies, nor a negative p,
 * -0.0 or NaN.
 *
 * dppr_read_at / dppr_group_read_at: p and r at m caller-given external ids (0.0 for a vertex without an
 * id), as a dense read would return them. Group outputs are vertex-major, [m][n] like the state; either
 * output may be NULL.
 *
 * Rejected with DPPR_ERR_INVALID before any device work, nothing written: k outside [1, DPPR_TOPK_MAX],
 * min_p negative or NaN, a bad slot / group, a NULL out_ids, out_p or count pointer, an id outside
 * [0, V) (read_at). All four hold the id-map lock as dppr_read does (safe beside dppr_slide_concurrent),
 * run on the solver stream, work on any state (converged or not, or set by dppr_write) and are never
 * part of the update path. */
#define DPPR_TOPK_MAX 8192
int dppr_topk(dppr_engine *e, int32_t slot, int32_t k, double min_p,
              int32_t *out_ids, double *out_p, double *out_r /* may be NULL */, int32_t *out_count);
int dppr_group_topk(dppr_engine *e, int32_t group, int32_t k, double min_p,
                    int32_t *out_ids /* [n][k] */, double *out_p /* [n][k] */, double *out_r /* [n][k] or NULL */,
                    int32_t *out_counts /* [n] */);
int dppr_read_at(dppr_engine *e, int32_t slot, const int32_t *ids, int32_t m, double *out_p, double *out_r);
int dppr_group_read_at(dppr_engine *e, int32_t group, const int32_t *ids, int32_t m,
                       double *out_p /* [m][n] */, double *out_r /* [m][n] */); /* either output may be NULL */

/* ---- a source group as a weighted set of targets (backward-compatible additions, ABI 6) ----
 * PPR is linear in the target: with p_i[v] the PPR of v towards source s_i, sum_i w_i * p_i[v] is the PPR of v
 * towards the weighted target set {(s_i, w_i)}. These two calls rank and read that combination on the device,
 * for up to 16 weight vectors at once, instead of dppr_group_read of every column and host arithmetic.
 *
 * weights is [q][n], q in [1, 16]; n is the group's current source count and the columns follow its lane order,
 * as dppr_group_sources reports both. Weights may be negative (contrast queries) or zero.
 *
 * THE SCORE of query j at vertex v is defined exactly. With p_i[v] exactly what dppr_group_read returns:
 *     acc = w[j][0] * p_0[v];
 *     for i = 1 .. n-1 in that order: acc = acc + w[j][i] * p_i[v];
 * Every product and every sum is rounded to double (round to nearest even); nothing is fused into a
 * multiply-add. A vertex without an internal id takes part with all p_i = 0.0 (its score is +0.0 or -0.0 as
 * the signs of the weights make it). Two consequences: a one-hot weight vector (w[j][i] = 1.0, the rest 0.0)
 * gives, bit for bit, the ids and values dppr_group_topk returns for source i; and the same loop over the dense
 * reads on the host reproduces every score bit for bit.
 *
 * dppr_group_topk_weighted: the qualifying vertices of query j are the external ids with score > min_score
 * (min_score >= 0), ordered by score descending, then external id ascending; the first min(k, #qualifying) are
 * returned with their count, entries past the count hold id -1 and 0.0. Outputs are query-major: ids [q][k],
 * scores [q][k], counts [q]. A NaN score (an overflow of opposite signs can make one) never qualifies, nor a
 * negative or zero one; +inf orders above every finite score.
 *
 * dppr_group_score_at: the q scores at m caller-given external ids, vertex-major [m][q]. m == 0 is a valid no-op.
 *
 * Rejected with DPPR_ERR_INVALID before any device work, nothing written: q outside [1, 16], k outside
 * [1, DPPR_TOPK_MAX], min_score negative or NaN, a weight that is NaN or infinite, a NULL weights, out_ids,
 * out_score or out_counts, a bad group; for dppr_group_score_at a NULL ids with m > 0, m < 0, or an id outside
 * [0, V). Both hold the id-map lock as dppr_read does (safe beside dppr_slide_concurrent), run on the solver
 * stream, work on any state (converged or not), scan the live and the parked zone, and are never part of the
 * update path. The top-k query keeps a device scratch of 8 q + 4 bytes per row that holds a vertex (not per V),
 * obtained -- like every other buffer of the call -- before anything is written: after DPPR_ERR_NOMEM the states
 * and the engine are as before. The scratch is ONE, shared with dppr_changes and dppr_topk_ranked and their group
 * forms: an engine holds the largest any call of the three families has needed, not one per family. */
int dppr_group_topk_weighted(dppr_engine *e, int32_t group, const double *weights /* [q][n] */, int32_t q /* 1..16 */,
                             int32_t k, double min_score, int32_t *out_ids /* [q][k] */, double *out_score /* [q][k] */,
                             int32_t *out_counts /* [q] */);
int dppr_group_score_at(dppr_engine *e, int32_t group, const double *weights /* [q][n] */, int32_t q,
                        const int32_t *ids, int32_t m, double *out_score /* [m][q] */);
/* Measurement aid: with dppr_set_profiling on, *out_ms is the device time of the last dppr_topk / dppr_group_topk /
 * dppr_group_topk_weighted / dppr_read_at / dppr_group_read_at / dppr_group_score_at call on this engine, from the first
 * to the last kernel (the copy back not included); -1 before the first such call. */
int dppr_debug_query_ms(dppr_engine *e, float *out_ms);

/* ---- what a batch moved: marks and per-source top-k of |delta p| (backward-compatible additions, ABI 6) ----
 * The question a consumer of a DYNAMIC PPR asks after a batch -- which vertices moved, by how much, how many moved by
 * more than min_delta -- answered on the device instead of by two dense reads per source and a diff on the host.
 *
 * MARK. dppr_mark / dppr_group_mark keep a copy of p of every source of the slot / group as it is now, exactly
 * what dppr_read / dppr_group_read would return. There is one mark per slot or group; marking again overwrites
 * it. A vertex that has no internal id at mark time has mark 0.0. The mark belongs to EXTERNAL vertex ids (it is
 * stored by external id, V doubles per row lane): a renumbering of the id space, the parking of a vertex or its
 * revival between mark and query changes no result. dppr_write leaves a mark alone.
 *
 * DELTA. For source i and external id v: d_i[v] = p_i[v] - mark_i[v], p_i being exactly what dppr_read /
 * dppr_group_read returns now (0.0 for a vertex without an id) -- ONE double subtraction, rounded to nearest even,
 * so the same subtraction over two dense reads on the host reproduces every value bit for bit.
 *
 * dppr_changes / dppr_group_changes: the qualifying vertices of source i are the external ids v with
 * |d_i[v]| > min_delta (min_delta >= 0, so a delta of +0.0 or -0.0 never qualifies, nor a NaN). They are ordered by
 * |d| descending, then external id ascending, and the first min(k, #qualifying) are returned:
 *     out_ids   [n][k]  the vertices
 *     out_delta [n][k]  d, signed
 *     out_p     [n][k]  the current p at those vertices (may be NULL)
 *     out_counts [n]    min(k, moved_i); entries of a row past its count hold id -1 and 0.0 (delta and p)
 *     out_moved  [n]    the number of qualifying vertices of source i, whatever k is (may be NULL)
 * Group outputs are source-major (lane order, as dppr_group_sources reports it); a slot is n = 1.
 *
 * RE-MARK. With remark != 0 the mark equals the current p once the call returns, as if dppr_mark / dppr_group_mark
 * had followed -- done in the same pass over the state, without another buffer. Calling with remark != 0 after
 * every batch is the per-batch feed: each call reports what that batch moved. (If a call with remark != 0 fails
 * with DPPR_ERR_HIP the mark is undefined: mark again.)
 *
 * UNMARK. dppr_unmark / dppr_group_unmark release the mark's memory (8 V bytes per row lane). Unmarking something
 * that has no mark returns DPPR_OK. A mark also goes with its engine, and dppr_group_replace_source,
 * dppr_group_add_source and dppr_group_remove_source drop the group's mark.
 *
 * Rejected with DPPR_ERR_INVALID before any device work, nothing written: a slot or group without a mark, k
 * outside [1, DPPR_TOPK_MAX], min_delta negative or NaN, a NULL out_ids, out_delta or out_counts, a bad slot /
 * group. Every buffer a call needs -- the mark itself (dppr_mark), the scratch of 16 n + 4 bytes per row that
 * holds a vertex (the one of dppr_group_topk_weighted) and the result block (dppr_changes) -- is obtained before anything is written: after
 * DPPR_ERR_NOMEM the state and any earlier mark are as before.
 * Threading and stream as dppr_topk: mark and query hold the id-map lock as dppr_read does (safe beside
 * dppr_slide_concurrent), run on the solver stream, work on any state (converged or not, or set by dppr_write),
 * scan the live and the parked zone and are never part of the update path or of a timed region. With
 * dppr_set_profiling on, dppr_debug_query_ms also reports the device time of the last dppr_changes /
 * dppr_group_changes, first to last kernel. */
int dppr_mark(dppr_engine *e, int32_t slot);
int dppr_group_mark(dppr_engine *e, int32_t group);
int dppr_unmark(dppr_engine *e, int32_t slot);
int dppr_group_unmark(dppr_engine *e, int32_t group);
int dppr_changes(dppr_engine *e, int32_t slot, int32_t k, double min_delta, int remark,
                 int32_t *out_ids, double *out_delta, double *out_p /* may be NULL */, int32_t *out_count,
                 int32_t *out_moved /* may be NULL */);
int dppr_group_changes(dppr_engine *e, int32_t group, int32_t k, double min_delta, int remark,
                       int32_t *out_ids /* [n][k] */, double *out_delta /* [n][k] */, double *out_p /* [n][k] or NULL */,
                       int32_t *out_counts /* [n] */, int32_t *out_moved /* [n] or NULL */);

/* ---- the state leaves the engine: thresholded sparse vectors and dense device copies (backward-compatible additions, ABI 6) ----
 * What a consumer takes beyond "the best k": the whole support of every source above a threshold, in id order (a CSR over the
 * sources: PPR-sparsified adjacency, candidate generation, a join), and p / r by external id in device memory the caller owns.
 *
 * SPARSE (dppr_support / dppr_group_support / dppr_export_sparse / dppr_group_export_sparse).
 * Qualifying entries: for source i (lane order as dppr_group_sources reports it) the external ids v with p_i[v] > min_p,
 * min_p >= 0, p_i[v] exactly what dppr_group_read returns. A vertex without an internal id, a negative p, -0.0 and NaN never
 * qualify (the rule of dppr_topk).
 * Order: by external id ascending.
 * Layout: source i's entries occupy [offsets[i], offsets[i + 1]) of out_ids, out_p and out_r; offsets[0] = 0. Values are the
 * stored doubles bit for bit; out_r holds r at the same vertices. A slot is n = 1 (out_offsets [2]).
 * Offsets: out_offsets is always HOST memory and is always written with the TRUE counts. dppr_support / dppr_group_support
 * return the differences offsets[i + 1] - offsets[i] alone.
 * Capacity: if offsets[n] > cap nothing is written to out_ids, out_p or out_r and the call still returns DPPR_OK -- the caller
 * compares offsets[n] with cap. cap = 0 with NULL arrays is the size query; the pattern is two calls, the second with
 * cap = offsets[n] of the first (a host destination is staged and copied by cap entries: an exact cap copies nothing spare).
 * Determinism: the result is a function of the state alone; it does not depend on grid size or scheduling, and no output
 * position comes from an atomic.
 * dest: where out_ids, out_p and out_r live. For DPPR_DEST_DEVICE the call returns after the solver stream has finished
 * writing, so any stream of the caller may read afterwards.
 *
 * DENSE (dppr_export_dense_dev / dppr_group_export_dense_dev): dst[v * n + i] (DPPR_VERTEX_MAJOR) or dst[i * V + v]
 * (DPPR_SOURCE_MAJOR) is p_i[v] (DPPR_DENSE_P) or r_i[v] (DPPR_DENSE_R) for every external id v in [0, V), 0.0 for a vertex
 * without an id. DPPR_F64: bit for bit. DPPR_F32: converted with round-to-nearest-even, what numpy's astype(float32) of the
 * dense read gives. A slot is n = 1. There is no host destination: dppr_read and dppr_group_read are that.
 *
 * A device destination is checked before any device work (hipPointerGetAttributes, hipMemGetAddressRange): the pointer must
 * be device memory on the ENGINE'S device, [dst, dst + bytes needed) must lie wholly inside one allocation (sparse: cap
 * entries of each array, cap taken as at most n * V; dense: n * V elements) and it must be aligned to its element size.
 * Anything else is DPPR_ERR_INVALID with nothing written: a wrong pointer is a rejected call, never a fault.
 * Also rejected with DPPR_ERR_INVALID before any device work, nothing written: min_p negative or NaN, cap < 0, a NULL
 * out_offsets / out_counts, cap > 0 with a NULL out_ids or out_p, dest / which / dtype / layout outside its values, a bad
 * slot / group.
 *
 * Threading and stream as dppr_topk: every call holds the id-map lock as dppr_read does (safe beside dppr_slide_concurrent),
 * runs on the solver stream, works on any state (converged or not, or set by dppr_write), sees the live and the parked zone
 * and is never part of the update path or of a timed region. The work space is 2 bytes per external id plus 192 bytes per
 * 256 external ids, and the block of a host destination 12 (20 with out_r) bytes per entry of cap, device and pinned host;
 * all of it is the engine's, obtained before anything is written, grown on demand and released with the engine: after
 * DPPR_ERR_NOMEM the state and the engine are as before. With dppr_set_profiling on, dppr_debug_query_ms also reports
 * the device time of the last of these calls, first to last kernel. */
#define DPPR_DEST_HOST 0
#define DPPR_DEST_DEVICE 1
#define DPPR_DENSE_P 0
#define DPPR_DENSE_R 1
#define DPPR_F64 0
#define DPPR_F32 1
#define DPPR_VERTEX_MAJOR 0 /* [V][n] */
#define DPPR_SOURCE_MAJOR 1 /* [n][V] */
int dppr_support(dppr_engine *e, int32_t slot, double min_p, int64_t *out_count);
int dppr_group_support(dppr_engine *e, int32_t group, double min_p, int64_t *out_counts /* [n] */);
int dppr_export_sparse(dppr_engine *e, int32_t slot, double min_p, int64_t cap, int dest, int64_t *out_offsets /* [2], HOST */,
                       int32_t *out_ids, double *out_p, double *out_r /* may be NULL */);
int dppr_group_export_sparse(dppr_engine *e, int32_t group, double min_p, int64_t cap, int dest,
                             int64_t *out_offsets /* [n + 1], HOST */, int32_t *out_ids, double *out_p,
                             double *out_r /* may be NULL */);
int dppr_export_dense_dev(dppr_engine *e, int32_t slot, int which, int dtype, void *dst_device);
int dppr_group_export_dense_dev(dppr_engine *e, int32_t group, int which, int dtype, int layout, void *dst_device);

/* ---- the sources scored under any seed distribution: h . p over the vertex axis (backward-compatible additions, ABI 6) ----
 * p_i[v] approximates pi_v(s_i), the PPR a walk started at v gives to the tracked source s_i, and PPR is linear in the start
 * distribution: for a seed distribution h over the vertices, pi_h(s_i) = sum_v h[v] pi_v(s_i) ~ sum_v h[v] p_i[v], with an error
 * of at most max|r_i| * |h|_1. One dot product scores a tracked source under any personalisation (a follow set, a set of
 * flagged accounts, a column of a feature matrix) without leaving the device: this is the dual of dppr_group_topk_weighted,
 * which folds over the sources.
 *
 *     out[f][i] = fold_j ( h_f[slot j] (x) x_i[vertex of slot j] )        f in [0, F), i in [0, n); out is [F][n], a slot is n = 1
 * x_i[v] is p_i[v] (DPPR_DENSE_P) or r_i[v] (DPPR_DENSE_R) by EXTERNAL id, exactly what dppr_group_read returns, +0.0 for a
 * vertex without a row. The padding lane of an odd group never reaches a result.
 *
 * THE FOLD. The result is a function of the state and of h alone: equal on every run, and reproducible bit for bit.
 * Slots.  Dense: slot j is external id j, j = 0 .. V - 1; h is [F][V] (DPPR_H_FEATURE_MAJOR) or [V][F] (DPPR_H_VERTEX_MAJOR) in
 *         DEVICE memory of the caller, DPPR_F64 or DPPR_F32 (f32 is widened to f64, exactly, before anything else).
 *         Sparse: one CSR over the F queries; slot j of query f is its j-th entry, at offsets[f] + j: external id ids[..],
 *         weight w[..]. Ids may repeat and come in any order; every occurrence is a slot of its own.
 * Term.   t_j = h_j * x_i[v_j], rounded to double, never fused with an addition. The product is computed even where x is +0.0
 *         for want of a row: a negative h gives -0.0 there.
 * Block.  Slots are taken in blocks of 2^16 consecutive slots, the last one padded with +0.0. A block is summed by the
 *         balanced binary tree that adds neighbours: level 1 is t_{2j} + t_{2j+1}, level 2 adds neighbouring level-1 sums, and
 *         so on for 16 levels, every sum rounded to double. Padding is added as +0.0 (-0.0 + +0.0 = +0.0).
 * Blocks. acc = B_0, then acc = acc + B_b for b = 1, 2, .. in ascending order. A query without slots is +0.0.
 * The order does not depend on grid size, on F, on n or on any internal chunking. In numpy, over terms t[..., slots]:
 *         pad to whole blocks, reshape to [..., blocks, 65536], y = y[..., 0::2] + y[..., 1::2] until one column is left, then
 *         add the columns from left to right.
 * A one-hot h therefore returns x_i[v] bit for bit. Non-finite h is outside this contract: IEEE arithmetic decides.
 *
 * Sparse offsets [F + 1] are always HOST memory: int64, offsets[0] = 0, non-decreasing. ids and w lie where `src` says
 * (DPPR_DEST_HOST or DPPR_DEST_DEVICE); out lies where `dest` says. For DPPR_DEST_DEVICE the call returns after the solver
 * stream has finished writing, so any stream of the caller may read afterwards.
 *
 * Rejected with DPPR_ERR_INVALID, nothing written and nothing read through a bad pointer: F outside [1, DPPR_DOT_MAX_F];
 * which / dtype / h_layout / src / dest outside its values; a NULL pointer; offsets that do not begin at 0 or decrease; a
 * pointer given as device memory (h, ids / w with src = DPPR_DEST_DEVICE, out with dest = DPPR_DEST_DEVICE) that is not device
 * memory of the ENGINE'S device, whose needed bytes (F * V elements; offsets[F] entries; F * n doubles) do not lie wholly
 * inside one allocation, or that is not aligned to its element; a sparse id outside [0, V) -- ids in host memory are checked
 * before any device work, ids in device memory by the kernel that gathers them, which then keeps the result from being
 * written: either way the call returns DPPR_ERR_INVALID with out untouched; a bad slot / group.
 *
 * Threading and stream as dppr_export_dense_dev: the id-map lock of dppr_read, the solver stream, any state, live and parked
 * zone, never part of the update path or of a timed region. Work space: at most 1 byte per external id and 16 features of a
 * launch (64 MiB at the most: a launch takes fewer features instead), 8 n bytes per 2048 entries of a sparse call plus the ids
 * and weights of a host source, and the block of a host destination (8 F n bytes, device and pinned host); all of it is the
 * engine's, obtained before the first kernel, grown on demand and released with the engine. With dppr_set_profiling on,
 * dppr_debug_query_ms also reports the device time of the last of these calls, first to last kernel. */
#define DPPR_DOT_MAX_F 4096
#define DPPR_H_FEATURE_MAJOR 0 /* h[f][v], F rows of V */
#define DPPR_H_VERTEX_MAJOR 1  /* h[v][f], V rows of F */
int dppr_dot_dense_dev(dppr_engine *e, int32_t slot, int which, const void *h_device, int dtype, int h_layout, int32_t F, int dest,
                       double *out /* [F] */);
int dppr_group_dot_dense_dev(dppr_engine *e, int32_t group, int which, const void *h_device, int dtype, int h_layout, int32_t F,
                             int dest, double *out /* [F][n] */);
int dppr_dot_sparse(dppr_engine *e, int32_t slot, int which, const int64_t *offsets /* [F + 1], HOST */, const int32_t *ids,
                    const double *w, int src, int32_t F, int dest, double *out /* [F] */);
int dppr_group_dot_sparse(dppr_engine *e, int32_t group, int which, const int64_t *offsets /* [F + 1], HOST */, const int32_t *ids,
                          const double *w, int src, int32_t F, int dest, double *out /* [F][n] */);

/* ---- point queries refined by random walks on the device: unbiased pi beyond eps (backward-compatible additions, ABI 6) ----
 * Every other query is bounded by the solve tolerance: p_i[v] is within about max|r_i| of pi_v(s_i). The state is one half of a
 * bidirectional estimator. With pi^ the fixed point the loop invariant defines (cpu/PPRCPUPowVec.h),
 *     pi^[u] = ALPHA [u == s] + (1 - ALPHA) / (outdeg(u) + 1) * sum_{x in out(u)} pi^[x],
 * the error e = pi^ - p satisfies e[u] = ALPHA r[u] + (1 - ALPHA) / (outdeg(u) + 1) * sum_{x in out(u)} e[x], so e[v] = E[t], t the
 * residual at the endpoint of a short forward walk from v (0 for a walk that dies): p_i[v] + mean_w r_i[X_w] is an unbiased
 * estimate of pi^_v(s_i) whose error shrinks as max|r_i| / sqrt(W), and ONE set of walks from v serves every source of a group,
 * because a walk does not depend on the source. The endpoints are also samples of the forward PPR distribution of v.
 *
 * THE WALK is identified by (start EXTERNAL id v, walk number w, seed) and by nothing else: not by the grid, the lane that ran it,
 * the position of v in the call, m or W. It runs over the out-CSR of the given epoch, the one the pull sweep reads.
 * Random numbers: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85; a round is
 *     c' = (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), then the key is incremented).
 * Step t = 0 .. 255 at internal vertex u (u_0 the internal id of v):
 *     1. (x0, x1, x2, x3) = philox(counter = (w, v, t, 0), key = (seed & 0xffffffff, seed >> 32)).
 *     2. x0 < 0x26666666 = floor(0.15 * 2^32): the walk STOPS; its endpoint is the external id of u.
 *     3. d = out_row_ptr[u + 1] - out_row_ptr[u] in that epoch; d = 0 for a vertex with no row there, a parked vertex, and a
 *        start without an internal id (which stops at itself or dies).
 *     4. j = floor(((x1 * 2^32 + x2) * (d + 1)) / 2^64).
 *     5. j == d: the walk DIES (the `+ 1` of the reference's denominator is this slot); its endpoint is -1.
 *        Otherwise u = out_col[out_row_ptr[u] + j].
 *     6. A walk still alive after step 255 dies.
 * Row order: the row the device holds -- neighbours by ascending INTERNAL id, duplicates kept. Results are reproducible for a
 * given engine history and seed. A renumbering of the id space changes which neighbour an index j selects, NOT the
 * distribution; it invalidates every older epoch, so a resident epoch is always in the current numbering.
 * Bias: the stop probability is 0.15 - 9.3e-11, a neighbour's probability is off by at most d / 2^64, truncation at 256 steps
 * loses at most 0.85^256 = 8.5e-19. With about 6.7 expected steps the endpoint distribution is within 1e-8 of the ideal one in
 * total variation: the bias of an estimate is at most 1e-8 * max|r_i|.
 *
 * dppr_walks: out_ends[q * W + w] = endpoint (external id, or -1) of walk w from starts[q]; starts are HOST memory and may
 * repeat; out_ends lies where dest says (DPPR_DEST_HOST / DPPR_DEST_DEVICE; a device pointer is checked as a destination of
 * dppr_export_dense_dev is). The epoch must be resident (-1: the newest).
 *
 * dppr_refine_at / dppr_group_refine_at, for source i (lane order) and query q, v = ids[q]; outputs [m][n], a slot is n = 1:
 *     t_w   = r_i[X_w] by external id, exactly what dppr_group_read returns (+0.0 without a row); +0.0 for a walk that died
 *     S     = fold_w t_w: THE FOLD of dppr_dot_dense_dev above over the slots w = 0 .. W - 1 (blocks of 2^16, the balanced tree
 *             that adds neighbours, padding +0.0, blocks added in ascending order)
 *     corr  = S / (double)W                  one division, rounded to nearest
 *     est   = p_i[v] + corr                  one addition; p_i[v] what dppr_group_read returns (+0.0 without a row)
 *     sumsq = fold_w (t_w * t_w)             every product rounded to double, never fused
 * out_corr and out_sumsq may be NULL. The standard error of est is sqrt((sumsq / W - corr^2) / (W - 1)).
 * The state must be converged, and if the epoch it stands on is known (anything but a state set by dppr_write) that must be
 * the epoch given: against another graph the estimate is biased, and the call is refused.
 *
 * Rejected with DPPR_ERR_INVALID, nothing written: m outside [1, DPPR_WALK_MAX_M], W outside [1, DPPR_WALK_MAX_W], m * W > 2^26;
 * a NULL starts / ids / out_ends / out_est; a start outside [0, V) (checked on the host before any launch); a bad dest; a device
 * pointer that is not aligned device memory of the engine's device with m * W ints inside one allocation; a bad slot / group;
 * an epoch that is not resident; for the refine calls a state that is not converged or stands on another epoch.
 * Threading and stream as dppr_dot_sparse: the id-map lock of dppr_read (safe beside dppr_slide_concurrent), the solver stream,
 * live and parked zone, never part of the update path or of a timed region. Work space: 4 bytes per walk for a host destination
 * and for a refine call, whose fold adds 16 n bytes per 2048 walks (at least 512 n bytes per query); all of it is the engine's,
 * obtained before the first kernel, grown on demand and released with the engine. With dppr_set_profiling on,
 * dppr_debug_query_ms also reports the device time of the last of these calls, first to last kernel. */
#define DPPR_WALK_MAX_M 4096
#define DPPR_WALK_MAX_W (1 << 20)
int dppr_walks(dppr_engine *e, int32_t epoch, const int32_t *starts /* [m] external, HOST */, int32_t m, int32_t W, uint64_t seed,
               int dest, int32_t *out_ends /* [m][W] external id or -1 */);
int dppr_refine_at(dppr_engine *e, int32_t slot, int32_t epoch, const int32_t *ids, int32_t m, int32_t W, uint64_t seed,
                   double *out_est /* [m] */, double *out_corr /* [m], may be NULL */, double *out_sumsq /* [m], may be NULL */);
int dppr_group_refine_at(dppr_engine *e, int32_t group, int32_t epoch, const int32_t *ids, int32_t m, int32_t W, uint64_t seed,
                         double *out_est /* [m][n] */, double *out_corr /* [m][n], may be NULL */,
                         double *out_sumsq /* [m][n], may be NULL */);
/* Test hooks. dppr_debug_id_map: the internal id of every external id ([V]; -1 without one), with which a test rebuilds the
 * rows the walks index from dppr_read_out_graph. dppr_debug_walk_form: 0 (default) the lane-refill kernel, 1 one walk per
 * thread -- the same results bit for bit, kept for the measurement (tools/walk_times.py). */
int dppr_debug_id_map(dppr_engine *e, int32_t *out_ext2int /* [V], -1 without an internal id */);
int dppr_debug_walk_form(dppr_engine *e, int form);

/* ---- local clusters of the tracked sources: a conductance sweep over the top-k order (backward-compatible additions, ABI 6) ----
 * Every other query reads the state; this one asks the graph about it. The vertices are ordered by p, the order is walked, and the
 * cut is made where the conductance of the prefix is lowest (Andersen, Chung, Lang: "Local graph partitioning using PageRank
 * vectors", FOCS 2006) -- on the device, next to the state, instead of dppr_group_topk + dppr_read_out_graph + a sweep on the host.
 * The loop invariant normalises by outdeg + 1, and on a window that stores both directions (d(v) + 1) pi_v(s) = (d(s) + 1) pi_s(v):
 * p_i[v] is proportional to the forward PPR of s_i at v divided by d(v) + 1, the degree-normalised vector the ACL sweep orders by.
 * On a directed window the order is by contribution to s_i and the cut is the out-boundary of the prefix.
 *
 * For source i (lane order; a slot is n = 1), every output is defined exactly:
 *   ORDER   v_0 .. v_{L-1}: exactly what dppr_topk / dppr_group_topk return for (k, min_p) -- p > min_p, p descending, external
 *           id ascending, live and parked zone -- with L = count = min(k, #qualifying). out_ids[i][j] = v_j; entries past L are -1.
 *   GRAPH   the out-CSR of `epoch` with multiplicity: a duplicate edge counts as often as it is stored, a self loop never crosses
 *           a cut. Ed is what dppr_graph_edges returns for the epoch. A vertex without a row in that epoch (parked, or never
 *           named) has degree 0.
 *   PREFIX  with S_j = {v_0 .. v_j}:
 *             vol[j]     = sum over u in S_j of outdeg(u)
 *             cut_out[j] = #{stored edges u -> w : u in S_j, w not in S_j}
 *             cut_in[j]  = #{stored edges u -> w : u not in S_j, w in S_j}
 *           Entries past L are 0. (directed = 0: both directions are stored and cut_in == cut_out.)
 *   BEST    den[j] = min(vol[j], Ed - vol[j]). Prefix j is ELIGIBLE if j + 1 >= min_size and den[j] > 0.
 *           phi[j] = (double)cut_out[j] / (double)den[j]: one IEEE division of two exactly converted integers.
 *           The best prefix is the eligible j of smallest phi, the smallest j among equal values:
 *           best_size = j + 1, best_cut = cut_out[j], best_vol = vol[j], best_phi = phi[j].
 *           No eligible prefix: best_size = 0, best_cut = best_vol = 0, best_phi = +infinity.
 * A prefix's values do not depend on what follows it: the arrays of a smaller k are the head of those of a larger one.
 * Group outputs are source-major: out_best [n], the four arrays [n][k]; each of the four may be NULL (only what is asked for is
 * copied back).
 *
 * The epoch must be resident (-1: the newest). If the epoch the state stands on is known (anything but a state set by dppr_write)
 * it must be the one given: a cut of another graph says nothing about this state, and the call is refused. Convergence is NOT
 * required: like dppr_topk the call works on any state.
 *
 * Rejected with DPPR_ERR_INVALID before any device work, nothing written: k outside [1, DPPR_CLUSTER_MAX], min_p negative or NaN,
 * min_size outside [1, k], a NULL out_best, a bad slot / group, an epoch that is not resident or not the state's.
 * Threading and stream as dppr_topk: the id-map lock of dppr_read (safe beside dppr_slide_concurrent), the solver stream, never
 * part of the update path or of a timed region. Work space beyond dppr_topk's: a rank table of 2 bytes per source (rounded up to
 * a power of two) and row that holds a vertex, 8 bytes per 512 edges of the epoch and source for the rows that are walked in
 * pieces, and the result block; all of it is the engine's, obtained before the first kernel, grown on demand and released with
 * the engine: after DPPR_ERR_NOMEM the states and the engine are as before. With dppr_set_profiling on, dppr_debug_query_ms also
 * reports the device time of the last of these calls, first to last kernel. */
#define DPPR_CLUSTER_MAX DPPR_TOPK_MAX      /* 8192: the sweep walks the order dppr_topk defines */
typedef struct {
    int32_t count;      /* L: vertices of the order, min(k, #qualifying)                         */
    int32_t best_size;  /* j*+1, 0 if no prefix is eligible                                      */
    int64_t best_cut;   /* cut_out of that prefix                                                */
    int64_t best_vol;   /* vol of that prefix                                                    */
    double  best_phi;   /* its conductance; +infinity if best_size == 0                          */
} dppr_cluster_t;
int dppr_cluster(dppr_engine *e, int32_t slot, int32_t epoch, int32_t k, double min_p, int32_t min_size,
                 dppr_cluster_t *out_best,
                 int32_t *out_ids /* [k] or NULL */, int64_t *out_cut_out /* [k] or NULL */,
                 int64_t *out_cut_in /* [k] or NULL */, int64_t *out_vol /* [k] or NULL */);
int dppr_group_cluster(dppr_engine *e, int32_t group, int32_t epoch, int32_t k, double min_p, int32_t min_size,
                       dppr_cluster_t *out_best /* [n] */,
                       int32_t *out_ids /* [n][k] or NULL */, int64_t *out_cut_out /* [n][k] or NULL */,
                       int64_t *out_cut_in /* [n][k] or NULL */, int64_t *out_vol /* [n][k] or NULL */);

/* ---- the subgraph around a source: its top-k order and every stored edge among it (backward-compatible additions, ABI 6) ----
 * What a PPR index is most often kept for downstream: the k vertices of largest p and the edges among them as a CSR in LOCAL
 * numbering (vertex = its position in the order) -- the input of a PPR-neighbourhood sampler or of a plot -- built on the device,
 * next to the state, instead of dppr_group_topk + dppr_read_out_graph + a filter on the host and a copy back.
 *
 * For source i (lane order; a slot is n = 1), every output is defined exactly:
 *   ORDER   v_0 .. v_{L-1}: exactly what dppr_topk / dppr_group_topk return for (k, min_p) -- p > min_p, p descending, external
 *           id ascending, live and parked zone -- with L = min(k, #qualifying). out_counts[i] = L; out_ids[i][j] = v_j and -1
 *           past L; out_p[i][j] is the stored double and 0.0 past L.
 *   GRAPH   the out-CSR of `epoch` with multiplicity: a duplicate edge appears as often as it is stored. A self loop of a vertex
 *           of the order IS an edge of the subgraph (tail position = head position); dppr_cluster differs here, because a self
 *           loop never crosses a cut. A vertex without a row in that epoch (parked, or never named) has an empty row and is
 *           nobody's head.
 *   ROWS    with rho_i(w) the position of w in the order, row j of source i holds rho_i(w) for every stored out-edge v_j -> w
 *           whose head lies in the order, in ascending position; equal positions are adjacent. The order in which the device
 *           stores a row's entries is no part of this: the rule does not depend on it.
 *   LAYOUT  one CSR over all sources. out_offsets [n + 1]: source i's entries occupy [offsets[i], offsets[i + 1]) of out_col;
 *           offsets[0] = 0. out_row_ptr [n][k + 1] holds ABSOLUTE indices into out_col: row j of source i is
 *           [row_ptr[i][j], row_ptr[i][j + 1]), row_ptr[i][0] = offsets[i], and row_ptr[i][j] = offsets[i + 1] for j >= L.
 *           out_col [cap] holds local positions in [0, L).
 * Prefix property: with k' < k and both orders longer than k', row j < k' of the smaller call is row j of the larger one
 * restricted to positions < k'.
 * Capacity: out_offsets and out_counts are always HOST memory and are always written with the TRUE counts. If offsets[n] > cap
 * nothing is written to out_col and the call still returns DPPR_OK -- the caller compares offsets[n] with cap; out_ids, out_p and
 * out_row_ptr are written either way. cap = 0 with a NULL out_col is the size query; the pattern is two calls, the second with
 * cap = offsets[n] of the first.
 * dest (DPPR_DEST_HOST / DPPR_DEST_DEVICE): where out_ids, out_p, out_row_ptr and out_col live; each of the first three may be
 * NULL. A device destination is checked as the exports check theirs, before any device work: device memory of the ENGINE'S
 * device, the bytes needed (n * k ids / p, n * (k + 1) row_ptr, cap entries of col, cap taken as at most n * Ed) wholly inside
 * one allocation, aligned to the element size; and the call returns after the solver stream has finished writing, so any stream
 * of the caller may read afterwards.
 * Determinism: the result is a function of the state and the epoch alone; no output position comes from the return value of an
 * atomic (integer sums are used to count).
 *
 * Epoch rule as dppr_cluster: the epoch must be resident (-1: the newest) and, if the epoch the state stands on is known
 * (anything but a state set by dppr_write), it must be the one given. Convergence is NOT required.
 * Rejected with DPPR_ERR_INVALID before any device work, nothing written: k outside [1, DPPR_SUBGRAPH_MAX], min_p negative or
 * NaN, cap < 0, cap > 0 with a NULL out_col, a NULL out_offsets or out_counts, dest outside its values, a bad slot / group, an
 * epoch that is not resident or not the state's, a bad device pointer.
 * Threading and stream as dppr_cluster: the id-map lock of dppr_read (safe beside dppr_slide_concurrent), the solver stream, never
 * part of the update path or of a timed region. Work space beyond dppr_cluster's rank table and chunk list: 1 MiB of per-position
 * counters and the block (ids, p, row_ptr; a host destination's col by cap, device and pinned host); all of it is the engine's,
 * obtained before the first kernel, grown on demand and released with the engine: after DPPR_ERR_NOMEM the states and the engine
 * are as before. With dppr_set_profiling on, dppr_debug_query_ms also reports the device time of the last of these calls, first
 * to last kernel (the one read of the counts by the host lies between them).
 * dppr_debug_subgraph_wave_max: a test and measurement hook. A row with at most this many entries in the order (default and largest
 * value 256; and at most 2048 stored entries) is placed by the wave that owns it, any other by a workgroup with a histogram; 0
 * sends every row there. The results do not depend on it. */
#define DPPR_SUBGRAPH_MAX DPPR_TOPK_MAX     /* 8192: the subgraph is induced by the order dppr_topk defines */
int dppr_subgraph(dppr_engine *e, int32_t slot, int32_t epoch, int32_t k, double min_p, int64_t cap, int dest,
                  int32_t *out_count /* HOST */, int64_t *out_offsets /* [2], HOST */,
                  int32_t *out_ids /* [k] or NULL */, double *out_p /* [k] or NULL */,
                  int64_t *out_row_ptr /* [k + 1] or NULL */, int32_t *out_col /* [cap]; NULL with cap = 0 */);
int dppr_group_subgraph(dppr_engine *e, int32_t group, int32_t epoch, int32_t k, double min_p, int64_t cap, int dest,
                        int32_t *out_counts /* [n], HOST */, int64_t *out_offsets /* [n + 1], HOST */,
                        int32_t *out_ids /* [n][k] or NULL */, double *out_p /* [n][k] or NULL */,
                        int64_t *out_row_ptr /* [n][k + 1] or NULL */, int32_t *out_col /* [cap]; NULL with cap = 0 */);
int dppr_debug_subgraph_wave_max(dppr_engine *e, int wave_max);

/* ---- ranked candidates: factor, mask and neighbour exclusion before the selection (backward-compatible additions, ABI 6) ----
 * dppr_topk / dppr_group_topk return the k best of ALL vertices by raw p. What a consumer ranks is rarely that: the head of every
 * source's order is the source itself and the vertices with a stored edge to it, the candidates are one type of vertex or what is
 * outside a block list, and the order wanted is often p times a per-vertex factor. These calls apply all three on the device,
 * between the state and the selection, instead of a large k or a dense read finished on the host.
 *
 * THE SCORE of lane i (lane order; a slot is n = 1) at vertex v is defined exactly. With p = p_i[v] exactly what dppr_read /
 * dppr_group_read returns (0.0 for a vertex without an internal id), and outdeg(v) the out-degree of v in `epoch` with
 * multiplicity as stored (0 for a parked vertex or one without a row):
 *     DPPR_FACTOR_NONE      score = p
 *     DPPR_FACTOR_DEV       score = p * g[v]                  g = factor_dev[v] by EXTERNAL id; an f32 g is converted to double exactly
 *     DPPR_FACTOR_DEG       score = p * (double)(outdeg(v) + 1)
 *     DPPR_FACTOR_INV_DEG   score = p / (double)(outdeg(v) + 1)
 * Each is ONE rounding to double (round to nearest even), nothing fused: numpy's `*` and `/` over the dense read reproduce every
 * score bit for bit. On a window that stores both directions (d(v) + 1) p_i[v] = (d(s_i) + 1) pi_{s_i}(v), so DPPR_FACTOR_DEG
 * ranks by the FORWARD PPR of the source, the vector this reverse-push engine does not hold.
 *   MASKED OUT   DPPR_MASK_ALLOW: only vertices with mask_dev[v] != 0 take part; DPPR_MASK_DENY: vertices with mask_dev[v] != 0
 *                do not. mask_dev is [V] by external id, one byte per vertex. A vertex that is masked out scores exactly +0.0.
 *   EXCLUDED     per lane, by the OR of DPPR_EXCLUDE_*: SEEDS -- the lane's source, or every seed of its set
 *                (dppr_add_target_group); IN_NEIGHBOURS -- v with a stored edge v -> seed in `epoch`, for any seed of the lane;
 *                OUT_NEIGHBOURS -- v with a stored edge seed -> v. A vertex excluded for the lane scores +0.0 IN THAT LANE: the
 *                same vertex may be excluded for lane 2 and rank first for lane 3. On an undirected window the two neighbour
 *                flags mean the same set. Self loops and duplicate edges need no special case (a self loop makes the seed its
 *                own neighbour).
 *   NO ID        a vertex without an internal id has no row and no edge: it scores +0.0 if it is masked out, otherwise its score
 *                follows the formula from p = 0.0 (DPPR_FACTOR_DEV: 0.0 * g[v], which is -0.0 for a negative and NaN for an
 *                infinite or NaN g[v]).
 *
 * dppr_topk_ranked / dppr_group_topk_ranked: THE ORDER is as in dppr_group_topk. The qualifying vertices of lane i are the external
 * ids with score > min_score (min_score >= 0: a score of +-0, a negative or a NaN score never qualifies, +inf orders first), ordered
 * by score descending, then external id ascending; the first min(k, #qualifying) are returned with their count and their scores,
 * entries past the count hold id -1 and 0.0. Group outputs are lane-major: ids [n][k], scores [n][k], counts [n]. The live and the
 * parked zone are scanned.
 * ANCHOR: with spec == NULL, or a spec of DPPR_FACTOR_NONE / DPPR_MASK_NONE / exclude 0, ids and scores equal the ids and p of
 * dppr_topk / dppr_group_topk(k, min_p = min_score) bit for bit.
 *
 * dppr_rank_score_at / dppr_group_rank_score_at: the same score at m caller-given external ids, vertex-major [m][n] like the state.
 * m == 0 is a valid no-op.
 *
 * EPOCH. A spec that needs neither degrees nor neighbours (no DPPR_FACTOR_DEG / _INV_DEG, no neighbour flag) does not look at
 * `epoch`. Otherwise the epoch rule of dppr_cluster: the epoch must be resident (-1: the newest) and, if the epoch the state stands
 * on is known (anything but a state set by dppr_write), it must be the one given. Convergence is NOT required.
 *
 * Rejected with DPPR_ERR_INVALID before any device work, nothing written: an unknown factor, factor_dtype (read only for
 * DPPR_FACTOR_DEV) or mask value, unknown exclude bits; a factor_dev (DPPR_FACTOR_DEV) or mask_dev (a mask) that is not device
 * memory of the ENGINE'S device, whose V elements do not lie inside one allocation, or that is not aligned to its element size; k
 * outside [1, DPPR_TOPK_MAX]; min_score negative or NaN; a NULL out_ids, out_score or count pointer; a bad slot / group; for the
 * score_at forms a NULL out_score, a NULL ids with m > 0, m < 0 or an id outside [0, V); an epoch that is not resident or not the
 * state's, where the spec needs one. factor_dev and mask_dev are only read, on the solver stream, before the call returns.
 * Threading and stream as dppr_topk: the id-map lock of dppr_read (safe beside dppr_slide_concurrent), the solver stream, any state
 * (converged or not), never part of the update path or of a timed region. Work space beyond dppr_topk's: a scratch state of
 * 8 n + 4 bytes per row that holds a vertex (the one of dppr_group_topk_weighted), 4 bytes per live row for the exclusion words, and for the neighbour flags 8 bytes per
 * seed and 8 bytes per piece of 512 entries of the seeds' rows (bounded by the epoch's edges per lane and direction); all of it is
 * the engine's, obtained before the first kernel, grown on demand and released with the engine: after DPPR_ERR_NOMEM the states and
 * the engine are as before. With dppr_set_profiling on, dppr_debug_query_ms also reports the device time of the last of these
 * calls, first to last kernel (with a neighbour flag the one read of the seeds' row lengths by the host lies between them).
 * OUT OF SCOPE: weight vectors as in dppr_group_topk_weighted. A set lane IS the combined target; "the neighbours of a combination"
 * of lanes has no single meaning.
 * dppr_debug_rank_piece: a test hook, as dppr_debug_subgraph_wave_max. The rows of the seeds are walked in pieces of at most `edges`
 * entries, one wave each (default and largest value 512, smallest 1). The results do not depend on it. */
#define DPPR_FACTOR_NONE      0   /* score = p                                                        */
#define DPPR_FACTOR_DEV       1   /* score = p * g[v], g = factor_dev[v] by EXTERNAL id, [V], f64/f32 */
#define DPPR_FACTOR_DEG       2   /* score = p * (double)(outdeg(v) + 1)   (forward PPR order on a    */
                                  /*                                        window of both directions)*/
#define DPPR_FACTOR_INV_DEG   3   /* score = p / (double)(outdeg(v) + 1)                              */
#define DPPR_MASK_NONE  0
#define DPPR_MASK_ALLOW 1         /* only vertices with mask_dev[v] != 0 take part */
#define DPPR_MASK_DENY  2         /* vertices with mask_dev[v] != 0 do not         */
#define DPPR_EXCLUDE_SEEDS          1u  /* the lane's source / every seed of its set                  */
#define DPPR_EXCLUDE_IN_NEIGHBOURS  2u  /* v with a stored edge v -> seed, for any seed of the lane   */
#define DPPR_EXCLUDE_OUT_NEIGHBOURS 4u  /* v with a stored edge seed -> v                             */
typedef struct {
    int32_t factor, factor_dtype;      /* DPPR_FACTOR_*, DPPR_F64 | DPPR_F32 (read only for _DEV) */
    const void *factor_dev;            /* [V] by external id, device memory of the engine's device */
    int32_t mask;                      /* DPPR_MASK_* */
    const uint8_t *mask_dev;           /* [V] by external id, one byte per vertex, device memory  */
    uint32_t exclude;                  /* OR of DPPR_EXCLUDE_* */
} dppr_rank_spec_t;
int dppr_topk_ranked(dppr_engine *e, int32_t slot, int32_t epoch, const dppr_rank_spec_t *spec, int32_t k, double min_score,
                     int32_t *out_ids, double *out_score, int32_t *out_count);
int dppr_group_topk_ranked(dppr_engine *e, int32_t group, int32_t epoch, const dppr_rank_spec_t *spec, int32_t k, double min_score,
                           int32_t *out_ids /* [n][k] */, double *out_score /* [n][k] */, int32_t *out_counts /* [n] */);
int dppr_rank_score_at(dppr_engine *e, int32_t slot, int32_t epoch, const dppr_rank_spec_t *spec, const int32_t *ids, int32_t m,
                       double *out_score /* [m] */);
int dppr_group_rank_score_at(dppr_engine *e, int32_t group, int32_t epoch, const dppr_rank_spec_t *spec, const int32_t *ids, int32_t m,
                             double *out_score /* [m][n] */);
int dppr_debug_rank_piece(dppr_engine *e, int edges);

/* ---- positions of given vertices in a lane's order (backward-compatible additions, ABI 6) ----
 * dppr_topk_ranked returns the head of every lane's order. These calls answer the inverse question: WHERE DOES VERTEX v STAND in
 * lane i's order -- the input of MRR, Hits@K and the percentile of a held-out edge, and the "rank of item v for user s" shown
 * beside a score. Without them the answer is a selection at k = DPPR_TOPK_MAX searched on the host, blind below position 8192, or
 * a dense read of every column and a host sort.
 *
 * THE SCORE score_i[v] is THE SCORE of dppr_topk_ranked for lane i, unchanged: the same factor, mask and exclusion, the same NO ID
 * rule, the same EPOCH rule (a spec that reads no degree and no neighbour does not look at `epoch`); spec == NULL means the score
 * is p.
 * QUALIFYING. A vertex qualifies in lane i iff score_i[v] > min_score, with min_score >= 0: a score of +-0, a negative or a NaN
 * score never qualifies, +inf does.
 * POSITION. pos[j][i] = -1 if ids[j] does not qualify in lane i. Otherwise it is the number of external ids u with
 * score_i[u] > score_i[v], or score_i[u] == score_i[v] and u < v: the 0-based position of v in the order of dppr_topk_ranked.
 * Every such u qualifies by itself. Every output is an integer defined by comparisons alone.
 * COUNTS. out_counts[i] is the number of qualifying vertices of lane i, the denominator of a percentile: the count
 * dppr_group_topk_ranked would report at unlimited k.
 * ZONES. The live and the parked zone are both counted. A vertex without an internal id never qualifies and never precedes
 * anything.
 * DUPLICATE IDS. A duplicate id gives the same answer in each of its places.
 * ANCHORS. (a) For every (i, j) with 0 <= pos[j][i] < k, dppr_group_topk_ranked(k, min_score, spec) returns ids[j] at
 * [i][pos[j][i]]. (b) Conversely, the positions of the ids that call returns for lane i are 0, 1, .., count - 1 in column i.
 * (c) With spec == NULL the same holds against dppr_group_topk(k, min_p = min_score).
 *
 * Outputs: dppr_position_at out_pos [m] and one count; dppr_group_position_at out_pos [m][n], vertex-major like the state, and
 * out_counts [n]. The count pointer may be NULL. m == 0 is valid: only the counts are computed if asked, a no-op if they are not.
 *
 * Rejected with DPPR_ERR_INVALID before any device work, nothing written: m < 0 or m > DPPR_POSITION_MAX; a NULL ids or a NULL
 * out_pos with m > 0; an id outside [0, V); min_score negative or NaN; every spec and epoch rejection of dppr_topk_ranked; a bad
 * slot / group.
 * Threading and stream as dppr_topk_ranked: the id-map lock for the whole call (safe beside dppr_slide_concurrent), the solver
 * stream, any state (converged or not), never part of the update path or of a timed region. Every stage is enqueued before the
 * single copy back of 64 + 4 m n bytes. Work space beyond dppr_topk_ranked's (whose scratch state it is, not a second one):
 * 12 m n bytes of keys and permutation, 4 (m + 1) n bytes of slots, the result block and its pinned twin; all of it is the
 * engine's, obtained before the first kernel, grown on demand and released with the engine: after DPPR_ERR_NOMEM the states and the
 * engine are as before. With dppr_set_profiling on, dppr_debug_query_ms reports the device time of the last of these calls.
 * OUT OF SCOPE: weight vectors (the scores of dppr_group_topk_weighted), positions by |p - mark|, device-resident ids or outputs,
 * more than DPPR_POSITION_MAX ids per call.
 * dppr_debug_position_tile: a test hook, as dppr_debug_rank_piece. The count pass holds at most `queries` consecutive positions of
 * a lane's order per workgroup and pass (smallest value 1, largest 4096; 0, the default: the plan's choice), so a small m can be
 * made to take several passes and lane blocks. The results do not depend on it. */
#define DPPR_POSITION_MAX 4096   /* ids per call, the limit of dppr_refine_at */
int dppr_position_at(dppr_engine *e, int32_t slot, int32_t epoch, const dppr_rank_spec_t *spec, double min_score,
                     const int32_t *ids, int32_t m, int32_t *out_pos /* [m] */, int32_t *out_count /* [1], may be NULL */);
int dppr_group_position_at(dppr_engine *e, int32_t group, int32_t epoch, const dppr_rank_spec_t *spec, double min_score,
                           const int32_t *ids, int32_t m, int32_t *out_pos /* [m][n], vertex-major like the state */,
                           int32_t *out_counts /* [n], may be NULL */);
int dppr_debug_position_tile(dppr_engine *e, int queries);

/* ---- explain a score: top contributing out-edges and the path to the seeds (backward-compatible additions, ABI 6) ----
 * The queries above answer WHAT is near a lane's target. These answer WHY a vertex has the score it has. The invariant every lane
 * keeps,
 *     p_i[u] + alpha r_i[u] = alpha h_i[u] + sum over stored out-edges u -> w of (1 - alpha) p_i[w] / (outdeg(u) + 1),
 * is an exact decomposition of p_i[u] into its own seed term and one term per out-neighbour; following the largest term hop by
 * hop gives the strongest chain from u to the lane's seeds. Without these calls the answer is dppr_group_read of every column,
 * dppr_read_out_graph and a group-by on the host. Every value below is reproducible by numpy bit for bit.
 *
 * For lane i and a vertex u with a row in `epoch`:
 *   DEGREE        d(u) is the stored out-degree, duplicates counted, as dppr_read_out_graph shows it. A vertex without an internal
 *                 id, or parked, has d = 0 and no heads.
 *   HEADS         the DISTINCT heads w of u's out-row; mult(u, w) is the number of stored copies. A self loop is a head like any
 *                 other.
 *   CONTRIBUTION  c_i(u, w) = (((1.0 - 0.15) * p_i[w]) * (double)mult) / (double)(d(u) + 1): two multiplications and one IEEE
 *                 division, in this order, never contracted. 1.0 - 0.15 is the double 0x1.b333333333333p-1 (the literal 0.85).
 *   CONTRIBUTOR ORDER of (u, i): the heads with c > 0 (false for a NaN and for negatives), c descending, external id of the head
 *                 ascending.
 *   OWN TERM      self_i[u] = 0.15 * h_i[u]: h is the indicator of the source for a source lane, the seed weight for a set lane,
 *                 0.0 otherwise.
 * Outputs are vertex-major [m][n] as the state and as dppr_position_at (a slot is n = 1). Per query id ids[j]:
 *   deg[j], distinct[j]   d and the number of distinct heads (they do not depend on the lane)
 *   self[j][i]            the own term
 *   TOP f CONTRIBUTORS    nbr_count[j][i] = min(f, #heads with c > 0); nbr[j][i][0..f) holds external ids, -1 past the count;
 *                         nbr_mult holds 0 and nbr_c 0.0 past the count; all three follow the contributor order.
 *   PATH of at most `depth` hops. path[j][i][0] = ids[j] always. At u = path[t] the first rule that applies decides:
 *       1. h_i[u] > 0                                  -> DPPR_EXPLAIN_END_SEED (0)
 *       2. t == depth                                  -> DPPR_EXPLAIN_END_DEPTH (1)
 *       3. the contributor order of (u, i) is empty    -> DPPR_EXPLAIN_END_DEAD (2)
 *       4. its first head is already on the path (u itself included: a self loop) -> DPPR_EXPLAIN_END_CYCLE (3)
 *       5. otherwise that head becomes path[t + 1], path_c[j][i][t] is its contribution, and t advances.
 *     len[j][i] = t + 1 in [1, depth + 1]; end[j][i] the code above; path is -1 past len; path_c is 0.0 past len - 1;
 *     path_p[j][i][t] = p_i[path[t]] is the stored double (0.0 for a vertex without a row), 0.0 past len.
 * A duplicate id gives the same answer in each of its places. Prefix property: the path for depth' < depth is the head of the
 * longer one, with END_DEPTH where it was cut.
 *
 * Limits: m in [0, DPPR_EXPLAIN_MAX_M], f in [0, DPPR_EXPLAIN_MAX_F], depth in [0, DPPR_EXPLAIN_MAX_DEPTH], f + depth >= 1.
 * m == 0 is valid and writes nothing. Every pointer of dppr_explain_out_t may be NULL: only what is asked for is computed and
 * copied back; all of them are HOST memory.
 * Epoch rule as dppr_cluster: the epoch must be resident (-1: the newest) and must be the one the state stands on, if that is
 * known. Convergence is NOT required: the decomposition holds for every state the solver leaves, with r in it.
 * Rejected with DPPR_ERR_INVALID before any device work, nothing written: m, f or depth outside the limits, f + depth == 0, a NULL
 * ids or a NULL out with m > 0, an id outside [0, V), a bad slot / group, an epoch that is not resident or not the state's.
 * Threading and stream as dppr_read: the id-map lock for the whole call (safe beside dppr_slide_concurrent), the solver stream,
 * never part of the update path or of a timed region. Determinism: the result is a function of the state and the epoch alone; no
 * output position comes from an atomic. Work space: the result block and its pinned twin, and -- with the memo on -- the one
 * scratch state of the ranked family; all of it is the engine's, obtained before the first kernel, grown on demand and released
 * with the engine: after DPPR_ERR_NOMEM the states and the engine are as before. With dppr_set_profiling on, dppr_debug_query_ms
 * reports the device time of the last of these calls.
 * dppr_debug_explain: a test hook. memo: -1 the plan decides, 0 off, 1 on -- the table of next hops the path waves share;
 * wave_rows in [1, 64]: the entries of a row a wave takes per step. The results depend on neither.
 * OUT OF SCOPE: device destinations, contributors at hops beyond the first, the whole next-hop forest, the in-CSR. */
#define DPPR_EXPLAIN_MAX_M 4096
#define DPPR_EXPLAIN_MAX_F 16
#define DPPR_EXPLAIN_MAX_DEPTH 64
#define DPPR_EXPLAIN_END_SEED 0
#define DPPR_EXPLAIN_END_DEPTH 1
#define DPPR_EXPLAIN_END_DEAD 2
#define DPPR_EXPLAIN_END_CYCLE 3
typedef struct { /* every pointer may be NULL: only what is asked for is copied back; HOST memory */
    int32_t *deg, *distinct;                /* [m]                 */
    double *self;                           /* [m][n]              */
    int32_t *nbr_count;                     /* [m][n]              */
    int32_t *nbr, *nbr_mult; double *nbr_c; /* [m][n][f]           */
    int32_t *len, *end;                     /* [m][n]              */
    int32_t *path; double *path_p;          /* [m][n][depth + 1]   */
    double *path_c;                         /* [m][n][depth] (depth 0: unused) */
} dppr_explain_out_t;
int dppr_explain_at(dppr_engine *e, int32_t slot, int32_t epoch, const int32_t *ids, int32_t m, int32_t f, int32_t depth,
                    const dppr_explain_out_t *out);
int dppr_group_explain_at(dppr_engine *e, int32_t group, int32_t epoch, const int32_t *ids, int32_t m, int32_t f, int32_t depth,
                          const dppr_explain_out_t *out);
int dppr_debug_explain(dppr_engine *e, int memo /* -1 plan decides, 0 off, 1 on */, int wave_rows /* 1 .. 64 */);

/* ---- certify a state: residual norms and the loop invariant (backward-compatible additions, ABI 6) ----
 * The queries above read a state. These say whether it is still RIGHT, without a dense read: any state that keeps the invariant
 *     p_i + alpha r_i = alpha h_i + M p_i
 * satisfies |p - p*|inf <= max_abs_r (p* = alpha h + M p* is the fixed point, so p - p* = M (p - p*) - alpha r; M has
 * non-negative entries and row sums <= 1 - alpha, hence |p - p*|inf <= (1 - alpha) |p - p*|inf + alpha |r|inf). "max |r| per
 * lane" plus "the invariant holds to rounding" is therefore a complete certificate of accuracy; no fixed point is computed and
 * the state is only read.
 *
 * ROWS. Every external id that has an internal id takes part, in the live zone and the parked zone, as dppr_topk sees them. A
 * vertex without an id has p = r = 0 and contributes nothing. Outputs are [n], one entry per lane (a slot: n = 1).
 * RESIDUAL PART (DPPR_CERT_RESIDUAL).
 *   n_pos[i], n_neg[i]   rows with r > eps and with r < -eps. The inequalities are strict: the test of the solver's loops (phase 0
 *                        and phase 1), so r == eps is not counted.
 *   n_nonfinite[i]       rows where p or r is NaN or +-inf. Such a row counts here only: it takes no part in any other output
 *                        of this part, and its slot in the two sums holds +0.0.
 *   max_abs_r[i]         the largest |r_i[v]|; 0.0 with argmax_r[i] = -1 if the lane has no finite row. argmax_r[i] is the
 *                        SMALLEST external id that attains it.
 *   sum_abs_r[i], sum_p[i]  the fold of the dot family (section dot above): the term |r_i[v]| (respectively p_i[v]) sits at slot
 *                        v, blocks of 2^16 slots, a block summed by the balanced tree that adds neighbours, the blocks added in
 *                        ascending order; the slot of a vertex without an id holds +0.0. sum_p[i] is bit for bit what
 *                        dppr_dot_dense_dev returns for h = 1, and numpy reproduces both sums bit for bit.
 *   n_p_nonzero[i]       rows with p != 0.
 * INVARIANT PART (DPPR_CERT_INVARIANT), against the out-CSR of `epoch` (-1: the newest). For every row u and lane i
 *     err_i[u] = | (p_i[u] + 0.15 * r_i[u]) - (0.15 * h_i[u] + (0.85 * S_i[u]) / (double)(d(u) + 1)) |
 *   S_i[u] is the sum of p_i[w] over the STORED out-edges u -> w: duplicates count as stored, self loops count. d(u) is the number
 *   of stored out-edges. h_i is the lane's seed vector: 1.0 at the source of a source lane, the seed weights of a set lane. A
 *   parked row has d = 0 and S = 0. inv_max_err[i] is the largest err_i[u] (an err that is not finite takes no part; 0.0 and
 *   inv_argmax[i] = -1 if there is none); inv_argmax[i] is the smallest external id among the rows that attain the device's own
 *   maximum. The ORDER of the additions inside S is the device's and is not part of the contract (rows are stored by internal id):
 *   two calls on the same state with the same dppr_debug_certify setting return identical bits, and any setting agrees with the
 *   plain sum to rounding. The call does NOT require that the state stands on `epoch`: state_epoch tells which epoch it stands on
 *   (-2: unknown, e.g. after dppr_write); against another epoch the result is simply the violation that graph implies.
 *   Convergence is not required.
 * state_epoch, converged and conv_eps are written by every accepted call: what the last solve left.
 * Rejected with DPPR_ERR_INVALID before any device work, nothing written: a NULL out, flags outside 1..3, an eps that is not
 * positive (a NaN is not), a bad slot / group, an epoch that is not resident, an engine that is broken. Every pointer of
 * dppr_certify_out_t may be NULL; a part all of whose pointers are NULL is simply not run.
 * Threading and stream as dppr_explain_at: the id-map lock for the whole call (safe beside dppr_slide_concurrent with an explicit
 * epoch <= k), the solver stream, never part of the update path or of a timed region. Work space: the result block, its pinned
 * twin, the partials and the queue of pieces, and the one scratch state of the ranked family for S; all of it is the engine's,
 * obtained before the first kernel, grown on demand and released with the engine: after DPPR_ERR_NOMEM the states and the engine
 * are as before. With dppr_set_profiling on, dppr_debug_query_ms reports the device time. Results do not depend on the grid size
 * or on scheduling; no output value comes from a floating-point atomic.
 * dppr_debug_certify: a test hook. piece_edges in [0, 2^20]: out-rows longer than this are summed in pieces of this many edges;
 * wave_rows in {0, 1, 2, 4, .. 64}: the short rows that share a wave (never more than the wave has teams). 0: the plan decides.
 * OUT OF SCOPE: the fixed point or any power iteration, repairing a state, several groups in one call. */
#define DPPR_CERT_RESIDUAL  1
#define DPPR_CERT_INVARIANT 2
typedef struct {            /* every pointer is HOST memory, [n] (a slot: n = 1), any may be NULL */
    double  *max_abs_r;   int32_t *argmax_r;    /* external id; -1 if the lane has no finite r */
    double  *sum_abs_r;   double  *sum_p;
    int64_t *n_pos;       int64_t *n_neg;       /* r > eps, r < -eps: dppr::legal, phase 0 and phase 1 */
    int64_t *n_nonfinite;                       /* rows where p or r is NaN or +-inf */
    int64_t *n_p_nonzero;
    double  *inv_max_err; int32_t *inv_argmax;  /* DPPR_CERT_INVARIANT only */
    int32_t state_epoch;  int32_t converged;  double conv_eps;   /* written by the call: what the last solve left (SolveState) */
} dppr_certify_out_t;
int dppr_certify(dppr_engine *e, int32_t slot, int32_t epoch, double eps, int flags, dppr_certify_out_t *out);
int dppr_group_certify(dppr_engine *e, int32_t group, int32_t epoch, double eps, int flags, dppr_certify_out_t *out);
int dppr_debug_certify(dppr_engine *e, int piece_edges /* 0: the plan decides */, int wave_rows /* 0: the plan decides */);

/* ---- every vertex to its best lane, across groups (backward-compatible additions, ABI 6) ----
 * The queries above answer per lane. With one lane per class -- sources or target sets -- the question per VERTEX is which lane
 * holds it best: label propagation on a live stream. dppr_assign reduces over the lane axis in one pass over the states, across
 * groups, and reports what a batch changed against a previous labelling (what dppr_changes is for p).
 *
 * CLASSES are the lanes of the n_groups groups of ONE engine named in `groups`, concatenated in call order: n_groups in
 * [1, DPPR_ASSIGN_GROUPS_MAX], C = sum of the groups' lane counts <= DPPR_ASSIGN_CLASSES_MAX. A group may be named twice; its
 * lanes are then two sets of classes. Source lanes and set lanes are alike.
 * For every external id v in [0, V):
 *     score_c[v] = scale[c] * p_c[v]     ONE multiplication (nothing fused); p_c[v] is exactly what dppr_group_read returns, 0.0
 *                                        for a vertex without an internal id. scale: HOST memory, [C], every entry finite and
 *                                        >= 0. scale == NULL: the scores are the stored p bit for bit, no multiplication.
 *     label[v]   the SMALLEST class whose score is the maximum of the scores that are > min_score (min_score >= 0, not NaN); -1
 *                if no score is. A negative score, +-0.0 and a class scaled by 0 never win.
 *     best[v]    score_label[v].
 *     second[v]  starts at +0.0 and is replaced only by a strictly greater score of a class other than label[v], classes taken in
 *                ascending order (so the class that set it is the smallest of those that hold it).
 *     margin[v]  best[v] - second[v], ONE subtraction.
 *     Where label[v] = -1: best[v] = margin[v] = +0.0 (no class is left out of second, which dppr_assign_at still reports).
 *     out_counts HOST memory, int64 [C + 1]: counts[c] = vertices labelled c, counts[C] = vertices labelled -1.
 *     FLIPS      with prev_label given ([V] int32, where `dest` says): the ids with prev_label[v] != label[v], in ascending id
 *                order, as three int32 arrays flip_id / flip_old / flip_new. *out_n_flips (HOST, may be NULL) is always the TRUE
 *                number of flips (0 without prev_label). The lists are written only if n_flips <= cap; otherwise NOTHING is
 *                written to them and the call is still DPPR_OK: the capacity rule of dppr_export_sparse. cap = 0 with NULL lists
 *                counts only. prev_label may BE out_label: an update in place (every element is read by the thread that then
 *                writes it). Arrays that overlap in any other way are not supported.
 * No output position comes from an atomic: the result is a function of the states alone, whatever the grid or the scheduling.
 * dest (DPPR_DEST_HOST / DPPR_DEST_DEVICE) governs every [V] array (out_label, out_best, out_margin -- the latter two may be NULL --,
 * prev_label) and the flip lists; counts and n_flips are always host memory. For DPPR_DEST_DEVICE the call returns after the solver
 * stream has finished: any stream of the caller may read the arrays.
 *
 * dppr_assign_at: the same values at m caller-given external ids (duplicates allowed), host memory, plus out_second_label: the
 * class that set second, or -1. out_best / out_second_label / out_margin may be NULL. m == 0 is a valid no-op.
 *
 * Rejected with DPPR_ERR_INVALID before any device work, nothing written: a bad handle or group; n_groups out of range or a NULL
 * groups; more than DPPR_ASSIGN_CLASSES_MAX classes; a scale that is not finite or is negative; min_score negative or NaN; a dest
 * that is neither; a NULL out_label or out_counts; cap < 0; cap > 0 with a NULL list; for DPPR_DEST_DEVICE an array that is not
 * device memory of the ENGINE'S device, is not aligned to its element size, or whose V (the lists: min(cap, V)) entries do not lie
 * inside one allocation; for dppr_assign_at m < 0, a NULL ids with m > 0, an id outside [0, V), a NULL out_label.
 * Threading and stream as dppr_topk: the id-map lock of dppr_read for the whole call (safe beside dppr_slide_concurrent), the
 * solver stream, the live and the parked zone, any state (converged or not); needs no resident epoch; never part of the update
 * path or of a timed region. Work space: 12 bytes per external id rounded up to tiles of 256, 8 bytes per tile, 2 KiB of scales
 * and a block of 2072 bytes -- for a host destination plus the arrays asked for --, with its pinned twin; all of it is the
 * engine's, obtained before anything is written, grown on demand and released with the engine: after DPPR_ERR_NOMEM the states
 * and the engine are as before. With dppr_set_profiling on, dppr_debug_query_ms reports the device time of the last of these
 * calls, first to last kernel.
 * OUT OF SCOPE: single-source slots (a group of one source serves); classes spread over several engines. */
#define DPPR_ASSIGN_GROUPS_MAX  16
#define DPPR_ASSIGN_CLASSES_MAX 256
int dppr_assign(dppr_engine *e, const int32_t *groups, int32_t n_groups, const double *scale /* [C], NULL ok */, double min_score, int dest,
                int32_t *out_label /* [V] */, double *out_best /* [V], NULL ok */, double *out_margin /* [V], NULL ok */,
                int64_t *out_counts /* host [C + 1] */, const int32_t *prev_label /* [V], NULL ok */, int64_t cap,
                int64_t *out_n_flips /* host */, int32_t *flip_id, int32_t *flip_old, int32_t *flip_new);
int dppr_assign_at(dppr_engine *e, const int32_t *groups, int32_t n_groups, const double *scale, double min_score, const int32_t *ids,
                   int32_t m, int32_t *out_label /* [m] */, double *out_best /* [m] */, int32_t *out_second_label /* [m] */,
                   double *out_margin /* [m] */);

/* ---- the patch feed: keep a replica of the thresholded state current, batch by batch (backward-compatible additions, ABI 6) ----
 * A consumer holds a copy of the thresholded vectors {p_i[v] > min_p} downstream (a feature store, a candidate index, a tensor
 * beside a model). dppr_group_export_sparse costs the whole support whatever a batch moved, and dppr_group_changes knows neither
 * the threshold nor which entries left the support. A PATCH is the entries to write and the entries to remove that make the
 * replica equal to the thresholded state; its size follows the change, not the support. It is the first query about the step
 * from one state to the next: it compares the state with the MARK of dppr_mark / dppr_group_mark (the same mark dppr_changes uses).
 *
 * For lane i (lane order as dppr_group_sources reports it) and external id v in [0, V):
 *     p   = p_i[v], exactly what dppr_read / dppr_group_read returns now (0.0 for a vertex without an internal id)
 *     m   = mark_i[v]
 *     d   = p - m, ONE double subtraction rounded to nearest even (the delta of dppr_changes)
 *     now = (p > min_p), then = (m > min_p), min_p >= 0: a negative value, -0.0 and NaN never qualify (the rule of
 *           dppr_export_sparse)
 *     UPSERT (v, i):  now && (!then || |d| > min_delta), min_delta >= 0.   Carries the id and p, bit for bit.
 *     DELETE (v, i):  then && !now.                                       Carries the id.
 * So a NaN p over a qualifying mark is a delete, a qualifying p over a NaN mark is an upsert, and |d| == min_delta is suppressed.
 * r is not part of a patch: it can move where p does not.
 *
 * Layout: two CSRs over the lanes in a dppr_patch_out_t -- up_offsets [n + 1], up_ids, up_p and del_offsets [n + 1], del_ids.
 * Lane i's upserts occupy [up_offsets[i], up_offsets[i + 1]) of up_ids and up_p, its deletes [del_offsets[i], del_offsets[i + 1])
 * of del_ids; each lane is in ascending external id. A slot is n = 1 (offsets [2]).
 * Offsets: up_offsets and del_offsets are always HOST memory and are always written with the TRUE counts.
 * Capacity: the caller gives cap_up and cap_del (entries). If up_offsets[n] > cap_up or del_offsets[n] > cap_del nothing is
 * written to the arrays, the mark is not touched, and the call returns DPPR_OK with written = 0; otherwise written = 1. Caps of 0
 * with NULL arrays are the size query; the pattern is two calls, the first with DPPR_PATCH_KEEP_MARK.
 * dest: where up_ids, up_p and del_ids live, DPPR_DEST_HOST or DPPR_DEST_DEVICE, with the device-pointer checks of the exports
 * (cap_up entries of up_ids and up_p, cap_del entries of del_ids, each cap taken as at most n * V).
 * Determinism: no output position and no value comes from an atomic. The result is a function of the state, the mark, min_p and
 * min_delta alone.
 *
 * RE-MARK, applied in the same call and only when written = 1:
 *     DPPR_PATCH_KEEP_MARK      leaves the mark alone.
 *     DPPR_PATCH_REMARK_ALL     sets the mark to p everywhere, as dppr_mark / dppr_group_mark would.
 *     DPPR_PATCH_REMARK_EMITTED sets mark_i[v] = p_i[v] only at the emitted upserts and deletes (v, i).
 * DPPR_PATCH_REMARK_EMITTED is the mode that BOUNDS DRIFT. Under it the mark is what the replica holds: where the replica has an
 * entry the mark is the value last sent, where it has none the mark does not qualify. After every applied patch the replica's
 * support equals {p > min_p} exactly, and every value it holds is within min_delta of the current p -- for any number of
 * batches, because a value is suppressed only while |p - (the value the replica holds)| <= min_delta. Under
 * DPPR_PATCH_REMARK_ALL with min_delta > 0 the mark follows p where nothing was sent, so moves below min_delta accumulate
 * unseen: the support stays exact, the values may drift without bound. With min_delta = 0 the replica is exact under either mode.
 * (If a call with a re-mark fails with DPPR_ERR_HIP the mark is undefined: mark again.)
 *
 * The initial sync is dppr_group_mark followed by dppr_group_export_sparse(min_p). A call on a slot or group without a mark is
 * DPPR_ERR_INVALID; dppr_group_replace_source, dppr_group_add_source and dppr_group_remove_source drop the mark, the consumer
 * then marks and exports again.
 *
 * Rejected with DPPR_ERR_INVALID before any device work, nothing written and the mark untouched: min_p or min_delta negative or
 * NaN, a negative cap, cap_up > 0 with a NULL up_ids or up_p, cap_del > 0 with a NULL del_ids, dest or remark outside its
 * values, a NULL out, up_offsets or del_offsets, a device destination that fails the checks, no mark, a bad slot / group.
 * Threading and stream as dppr_export_sparse: the call holds the id-map lock as dppr_read does (safe beside
 * dppr_slide_concurrent), runs on the solver stream, works on any state, sees the live and the parked zone and is never part of
 * the update path or of a timed region. The work space is 4 bytes per external id plus 384 bytes per 256 external ids, and the
 * block of a host destination 12 bytes per entry of cap_up and 4 per entry of cap_del, device and pinned host; all of it is the
 * engine's, obtained before anything is written, grown on demand and released with the engine. With dppr_set_profiling on,
 * dppr_debug_query_ms also reports the device time of the last of these calls, first to last kernel. */
#define DPPR_PATCH_KEEP_MARK 0
#define DPPR_PATCH_REMARK_ALL 1
#define DPPR_PATCH_REMARK_EMITTED 2
typedef struct {
    int64_t *up_offsets;  /* [n + 1], HOST */
    int32_t *up_ids;      /* cap_up entries, dest */
    double *up_p;         /* cap_up entries, dest */
    int64_t *del_offsets; /* [n + 1], HOST */
    int32_t *del_ids;     /* cap_del entries, dest */
    int32_t written;      /* set by the call: 1 the arrays hold the patch and the re-mark was applied, 0 a cap was too small */
} dppr_patch_out_t;
int dppr_patch(dppr_engine *e, int32_t slot, double min_p, double min_delta, int64_t cap_up, int64_t cap_del, int dest, int remark,
               dppr_patch_out_t *out);
int dppr_group_patch(dppr_engine *e, int32_t group, double min_p, double min_delta, int64_t cap_up, int64_t cap_del, int dest,
                     int remark, dppr_patch_out_t *out);

/* ---- vertices drawn in proportion to a lane's score (backward-compatible additions, ABI 6) ----
 * Every query above is a deterministic read. Consumers that TRAIN on the index need draws: negative and candidate sampling for a
 * recommender or a link predictor (vertices in proportion to p_i[v], the lane's seeds and their neighbours left out, one vertex
 * type allowed), importance sampling of a GNN mini-batch, Monte Carlo estimates of a sum over a lane's distribution. These calls
 * draw S external ids per lane WITH replacement, in proportion to a weight that is THE SCORE of the ranked queries, from a sum
 * tree built on the device; nothing of size V leaves the engine.
 *
 * THE DEFINITION. Lane i is in lane order; a slot is n = 1, lane 0. Every step is one addition, one subtraction, one
 * multiplication or one comparison of IEEE doubles, so a host program reproduces every draw exactly.
 * 1. WEIGHT. score_i[v] is THE SCORE of dppr_topk_ranked, unchanged: the same factor, mask and exclusion, the same NO ID rule,
 *    the same EPOCH rule (a spec that reads no degree and no neighbour does not look at `epoch`); spec == NULL means the score is
 *    p. w_i[v] = score_i[v] if score_i[v] > min_score (min_score >= 0), otherwise w_i[v] = +0.0: a NaN, a negative or a zero score
 *    weighs nothing.
 * 2. TREE. P is the smallest power of two >= V. Level 0 is y0[j] = w_i[j] for j < V and +0.0 for V <= j < P, in EXTERNAL id
 *    order. Level l + 1 is y[j] = y_l[2j] + y_l[2j + 1], one rounding. The root is out_total[i]; out_support[i] is the number of
 *    positive leaves. A root == 0 gives status DPPR_SAMPLE_EMPTY, a root that is not finite DPPR_SAMPLE_NONFINITE: in both
 *    cases every draw of the lane is -1 and its out_w is +0.0. Otherwise the status is DPPR_SAMPLE_OK.
 * 3. UNIFORM. Draw number j = first + 0 .. first + S - 1, in 64-bit arithmetic (first + S must not wrap):
 *    (x0, x1, x2, x3) = Philox4x32-10(counter = (lo32 j, hi32 j, i, 0x53414D50), key = (lo32 seed, hi32 seed)),
 *    u = ((x0 * 2^32 + x1) >> 11) * 2^-53, x = u * root, one rounding.
 * 4. DESCENT. From the root to a leaf. At a node with children L (even) and R (odd): if x >= L and R > 0 then x = x - L (one
 *    rounding) and go right; otherwise go left. The draw is the leaf's external id and out_w is that leaf's weight.
 * CONSEQUENCES. The descent only ever enters a node of positive value: a draw never returns a masked, excluded or
 * below-threshold vertex, whatever the roundings did (x may even be rounded up to the root itself). A lane's draws are a function
 * of its own leaves, its lane index, seed and j alone: not of n, S, the other lanes, or the form of the kernels. The contract is
 * the definition: the probability of v is w[v] / total up to the rounding of the sums, of relative order log2(P) * 2^-52.
 * ANCHORS. (a) Every drawn id v has dppr_group_rank_score_at(v) in that lane equal to out_w bit for bit, and > min_score.
 * (b) The draws of (first, S = a + b) are those of (first, a) followed by those of (first + a, b). (c) A lane with one positive
 * leaf returns it S times. (d) S == 0 is valid: only totals, supports and statuses are computed.
 *
 * dest (DPPR_DEST_HOST / DPPR_DEST_DEVICE) governs out_ids and out_w: a device pointer is checked as the destinations of the
 * exports are (aligned device memory of the engine's device, n * S elements inside one allocation), and is complete when the call
 * returns. out_w and out_support may be NULL. out_total, out_support and out_status are always host memory. Outputs:
 * dppr_sample out_ids [S], out_w [S], one total, support and status; dppr_group_sample out_ids [n][S] and out_w [n][S],
 * lane-major, out_total [n], out_support [n], out_status [n].
 *
 * Rejected with DPPR_ERR_INVALID before any device work, nothing written: every spec and epoch rejection of dppr_topk_ranked;
 * min_score negative or NaN; S < 0, S > DPPR_SAMPLE_MAX or n * S > DPPR_SAMPLE_MAX_TOTAL; first + S wrapping; an unknown dest;
 * a NULL out_ids with S > 0; a NULL out_total or out_status; a device out_ids or out_w that the range check refuses; a bad slot
 * / group.
 * Threading and stream as dppr_topk_ranked: the id-map lock for the whole call (safe beside dppr_slide_concurrent), the solver
 * stream, any state (converged or not), never part of the update path or of a timed region. Every stage is enqueued before the
 * single copy back. WORK SPACE: 8 n Vt bytes of leaves (Vt = V rounded up to 2048) and 8 n (Vt / 128 + 2 per level) bytes of
 * nodes -- about 8 n V (1 + 1/128) --, dppr_topk_ranked's exclusion words where the spec excludes, and the result block with its
 * pinned twin: 256 bytes, and 12 n S more for a host destination. All of it is the engine's, obtained before the first kernel,
 * grown on demand and released with the engine: after DPPR_ERR_NOMEM the states and the engine are as before. With
 * dppr_set_profiling on, dppr_debug_query_ms reports the device time of the last of these calls.
 * OUT OF SCOPE: sampling without replacement; weight vectors across lanes (the scores of dppr_group_topk_weighted); sampling by r
 * or by |delta p|; alias tables.
 * dppr_debug_sample_form: a test hook, as dppr_debug_walk_form. 0 (default): a wave rebuilds the lowest 8 levels of a draw from
 * the 256 leaves under it; 1: one thread per draw reads every level from a fully stored tree (8 n Vt bytes more). The results do
 * not depend on the form. */
#define DPPR_SAMPLE_MAX        (1 << 20)  /* draws per lane and call */
#define DPPR_SAMPLE_MAX_TOTAL  (1 << 24)  /* n * S per call */
#define DPPR_SAMPLE_OK         0
#define DPPR_SAMPLE_EMPTY      1          /* no vertex has a positive weight: every draw is -1 */
#define DPPR_SAMPLE_NONFINITE  2          /* the lane's total is not finite: every draw is -1 */
int dppr_sample(dppr_engine *e, int32_t slot, int32_t epoch, const dppr_rank_spec_t *spec, double min_score, uint64_t seed,
                uint64_t first, int32_t S, int dest, int32_t *out_ids /* [S] */, double *out_w /* [S], may be NULL */,
                double *out_total /* [1] */, int32_t *out_support /* [1], may be NULL */, int32_t *out_status /* [1] */);
int dppr_group_sample(dppr_engine *e, int32_t group, int32_t epoch, const dppr_rank_spec_t *spec, double min_score, uint64_t seed,
                      uint64_t first, int32_t S, int dest, int32_t *out_ids /* [n][S], lane-major */,
                      double *out_w /* [n][S], may be NULL */, double *out_total /* [n] */,
                      int32_t *out_support /* [n], may be NULL */, int32_t *out_status /* [n] */);
int dppr_debug_sample_form(dppr_engine *e, int form);

/* ---- forward PPR of any vertex on the resident window (backward-compatible additions, ABI 6) ----
 * Every score above is a column of the reverse problem: p_i[v] ~ pi_v(s_i) for a tracked target s_i. dppr_forward answers the
 * other direction, "where does the walk from q go?", for up to 16 starts q that need not be tracked: a ROW of the PPR matrix,
 * swept on the device over the in-CSR of a resident epoch. Read side only: no state is read or changed.
 *
 * DEFINITION. M[u][w] = 0.85 * mult(u -> w) / (d(u) + 1) over the STORED out-edges of epoch `epoch` (-1: the newest): d(u) is
 * the number of stored out-edges of u, duplicates count as stored, self loops count, the + 1 is death. For a start q
 *     x_0 = e_q,   x_{k+1}[w] = sum over the stored edges u -> w of x_k[u] * M[u][w],   f^K = 0.15 * sum_{k = 0 .. K} x_k
 * so that pihat_q(t) = lim f^K[t] and 0 <= pihat_q(t) - f^K[t] <= |x_{K+1}|_1 =: rem (0.15 * sum_{j > K} 0.85^(j-K-1) <= 1).
 * Every rounding is fixed; numpy reproduces every output bit for bit (tests/forward_ref.py):
 *   per-vertex term  y_k[u] = (0.85 * x_k[u]) / (double)(d(u) + 1): one multiplication, one division, once per vertex and
 *                    iteration.
 *   row sum          x_{k+1}[w] is THE FOLD of the dot family (section dot above) over the terms y_k[tail] of w's in-row in the
 *                    order the device stores it -- ascending internal tail id, duplicates as stored, self loops kept: blocks of
 *                    2^16 slots, a block summed by the balanced tree that adds neighbours (missing slots +0.0), the blocks added
 *                    in ascending order. Every term is >= +0.0, so padding is exact.
 *   accumulation     f[w] = f[w] + 0.15 * x_{k+1}[w]: one multiplication and one addition, k ascending; f starts as 0.15 * e_q.
 *   remaining mass   rem is the same fold of the last computed x over the external ids 0 .. V - 1; the slot of a vertex without
 *                    an internal id holds +0.0.
 *   stopping         iters in [1, 256], tol >= 0. After the iterations 8, 16, 24, .. below iters and after iteration iters every
 *                    column's rem is evaluated; a column whose rem <= tol is FROZEN at that check: its f and rem stand, its
 *                    iters_used is that k, it takes no further part. tol = 0 stops only a column whose mass has died out. After
 *                    iteration iters every column still running stops with iters_used = iters and the rem it has.
 *   independence     a column is a function of the epoch's rows, q, iters and tol alone: not of the other starts of the call, of
 *                    m, of the grid, of a team or piece size (dppr_debug_forward), or of what the solver has done.
 *   no internal id   a start without an internal id, and a parked one, has d = 0: f = 0.15 * e_q, rem = 0.0, iters_used =
 *                    min(8, iters).
 *   renumberings     results are by external id; like a walk, the order of a row's terms follows the rows the device holds, so a
 *                    renumbering may move last bits (it invalidates older epochs anyway).
 * OUTPUTS (dppr_forward_out_t; a part whose pointers are all NULL is not run):
 *   iters_used[m], rem[m]          HOST memory, either may be NULL.
 *   top k per start                topk_ids / topk_f [m][k], topk_counts [m], HOST memory: the vertices with f > min_f, f
 *                                  descending, ties by external id ascending (the order of dppr_topk); entries past a count: id
 *                                  -1, f 0.0. Asked for when any of the three is not NULL; then all three, k in
 *                                  [1, DPPR_TOPK_MAX] and min_f >= 0 are required.
 *   f at given ids                 at_f[j * m + i] = f_i[at_ids[j]], HOST memory, n_at in [1, DPPR_FORWARD_AT_MAX]. Asked for
 *                                  when at_ids or at_f is not NULL; then both are required.
 *   dense copy                     dense_dev: DEVICE memory of the caller, f by external id, dense_dtype DPPR_F64 (bit for bit)
 *                                  or DPPR_F32 (rounded once, to nearest even), dense_layout DPPR_VERTEX_MAJOR [V][m] or
 *                                  DPPR_SOURCE_MAJOR [m][V]; the pointer is checked as dppr_export_dense_dev checks its own.
 * starts: m in [1, DPPR_FORWARD_MAX_M] external ids in HOST memory; a start may repeat. The columns are interleaved as a group's
 * state is ([rows][row width of m]), so one gathered row serves every start.
 * Rejected with DPPR_ERR_INVALID before any device work, nothing written: m outside [1, 16], iters outside [1, 256], a tol that
 * is negative or not finite, a NULL starts or out, a start or an at id outside [0, V), a part asked for with a pointer missing
 * or a bad k / min_f / n_at / dtype / layout / device pointer, an epoch that is not resident, an engine that is broken.
 * Threading and stream as dppr_certify: the id-map lock for the whole call (safe beside dppr_slide_concurrent with an explicit
 * epoch <= k), the solver stream, never part of the update path or of a timed region. The host enqueues up to 8 sweeps, the rem
 * fold and the freeze update and then reads back ONE word; nothing is read back between sweeps. Work space: four planes of
 * [V][row width] doubles, the partials of the fold and the queue of the long rows' pieces; all of it is the engine's, obtained
 * before the first kernel, grown on demand and released with the engine: after DPPR_ERR_NOMEM the engine is as before. With
 * dppr_set_profiling on, dppr_debug_query_ms reports the time from the first sweep to the last check (read-backs included).
 * No output value comes from a floating-point atomic.
 * dppr_debug_forward: a test hook. piece_edges 0 or a power of two in [64, 4096]: in-rows longer than this are summed in pieces
 * of this many entries; team in {0, 1, 2, 4, 8}: the lanes that share one gathered row (raised to the fewest the row width
 * allows). 0: the plan decides. Every setting gives the same bits.
 * OUT OF SCOPE: the ranked or subgraph families over f. (Weighted start sets and a push with a frontier: dppr_forward_push;
 * a forward vector kept current under the stream: dppr_ftrack_create / dppr_ftrack_update; the conductance sweep of a track's p:
 * dppr_ftrack_cluster.) */
#define DPPR_FORWARD_MAX_M 16
#define DPPR_FORWARD_MAX_ITERS 256
#define DPPR_FORWARD_CHECK 8          /* iterations between two evaluations of rem */
#define DPPR_FORWARD_AT_MAX 4096
typedef struct {
    int32_t *iters_used; double *rem;                                   /* [m], HOST; either may be NULL */
    int32_t k; double min_f; int32_t *topk_ids; double *topk_f; int32_t *topk_counts; /* [m][k], [m][k], [m], HOST */
    const int32_t *at_ids; int32_t n_at; double *at_f;                  /* [n_at], [n_at][m], HOST */
    void *dense_dev; int32_t dense_dtype, dense_layout;                 /* DEVICE; DPPR_F64 | DPPR_F32; DPPR_VERTEX_MAJOR | DPPR_SOURCE_MAJOR */
} dppr_forward_out_t;
int dppr_forward(dppr_engine *e, int32_t epoch, const int32_t *starts /* [m] external, HOST */, int32_t m, int32_t iters, double tol,
                 const dppr_forward_out_t *out);
int dppr_debug_forward(dppr_engine *e, int piece_edges /* 0: the plan decides */, int team /* 0: the plan decides */);

/* ---- forward push: local forward PPR from a weighted start set (backward-compatible additions, ABI 6) ----
 * dppr_forward sweeps the whole window whatever the answer looks like. dppr_forward_push is the frontier-driven forward push of
 * Andersen, Chung and Lang on the device: its work follows the mass, not the window. Read side only: no state is read or changed,
 * no id is assigned.
 *
 * DEFINITION. M, d(u), stored edges, duplicates, self loops and epochs are exactly those of dppr_forward. A call has m in
 * [1, DPPR_FORWARD_MAX_M] columns. Column c starts from a weighted set h_c, a CSR in HOST memory (offsets[m + 1], ids, weights)
 * under the rules of dppr_add_target_group: offsets start at 0 and never decrease, a column has 1 .. DPPR_FPUSH_SET_MAX seeds, no
 * id twice within a column, every weight finite and > 0, weights are not normalised. A single vertex is one seed of weight 1.0.
 * Per column, by the device's rows: p = 0, r = h_c, thr[u] = eps * (double)(d(u) + 1) (one multiplication). Round k = 1, 2, ..:
 *   frontier         F = { u : r[u] > thr[u] }, a strict comparison. If F is empty the column is CONVERGED, rounds_used = k - 1,
 *                    and it never changes again.
 *   push             for u in F: p[u] = p[u] + 0.15 * r[u] (one multiplication, one addition), y[u] = (0.85 * r[u]) /
 *                    (double)(d(u) + 1) (the per-vertex term of dppr_forward), r[u] = +0.0. For u not in F: y[u] = +0.0.
 *   gather           for every vertex w: r[w] = r[w] + s[w], s[w] the row sum of dppr_forward: THE FOLD of the dot family over
 *                    y[tail] along w's whole in-row in stored order. Every term is >= +0.0: a row with no tail in F has
 *                    s = +0.0 and r[w] keeps its bits, so the device skips every row without a frontier in-neighbour. The
 *                    definition stays the dense one that numpy runs (tests/fpush_ref.py), bit for bit.
 *   stopping         max_rounds in [1, DPPR_FPUSH_MAX_ROUNDS]. After round max_rounds F is evaluated once more: a column whose F
 *                    is empty then is converged with rounds_used = max_rounds; any other stops with converged = 0 and
 *                    rounds_used = max_rounds.
 *   rowless seeds    a seed without an internal id, or a parked one, has no row: it is settled exactly whatever eps is,
 *                    p[q] = 0.15 * w and r[q] = +0.0; it takes no part in the rounds and counts in no statistic (the host
 *                    answers it, as dppr_forward answers a start without a row). So that a column is a function of the epoch
 *                    alone -- whether a vertex without an edge is parked is not one -- the same holds for every seed that no
 *                    stored edge of the epoch names.
 *   independence     a column is a function of the epoch's rows, its set, eps and max_rounds alone: not of the other columns,
 *                    of m, of the grid, of the chunking of rounds or of dppr_debug_forward_push.
 * GUARANTEE. With pihat_h = sum_q h[q] * pihat_q and rem = sum r: 0 <= pihat_h[t] - p[t] <= rem entrywise; a converged column
 * has r[u] <= eps * (d(u) + 1) everywhere; pihat_h(s) = p[s] + sum_u r[u] * pihat_u(s) exactly, so r handed to
 * dppr_group_dot_dense_dev over a solved group gives the bidirectional estimate of pihat_h(s_i) with error <= rem * max|r_reverse|.
 * OUTPUTS (dppr_forward_push_out_t; a part whose pointers are all NULL is not run):
 *   per column, HOST, each may be NULL   rounds_used[m], converged[m], rem[m] (the fold of r over the external ids 0 .. V - 1,
 *                                  as dppr_forward's rem), pushes[m] (int64: the sum of |F_k| over the rounds), left[m] (int64:
 *                                  the vertices with r > thr at the end; 0 if and only if converged).
 *   work[3]                        int64, HOST, over the UNION of the columns' frontiers per round, summed over the rounds: rows
 *                                  pushed; rows gathered (vertices with at least one in-neighbour in the union frontier); the
 *                                  in-edges of those rows. Exact integers: what the device walked.
 *   top k of p per column          topk_ids / topk_p [m][k], topk_counts [m], HOST: order and layout of dppr_forward's top k.
 *   p and r at given ids           at_p / at_r [j * m + i], HOST, n_at in [1, DPPR_FORWARD_AT_MAX]. Asked for when at_ids, at_p
 *                                  or at_r is not NULL; then at_ids and at least one of the two are required.
 *   dense copies                   dense_p_dev and / or dense_r_dev: DEVICE memory of the caller, by external id, one dtype and
 *                                  layout for both under the rules of dppr_forward's dense copy.
 * Rejected with DPPR_ERR_INVALID before any device work, nothing written: what dppr_forward rejects, an eps that is not finite or
 * not > 0, max_rounds outside [1, DPPR_FPUSH_MAX_ROUNDS], a bad CSR (NULL, offsets, sizes, an id outside [0, V), an id twice in a
 * column, a bad weight).
 * Threading, stream, work-space ownership and DPPR_ERR_NOMEM behave as for dppr_forward; the planes are shared with it. Nothing is
 * read back between the rounds of a chunk: the host enqueues a few rounds, then reads ONE word. Every kernel takes its counts from
 * device memory, so a round after convergence is a few empty launches. No output value comes from a floating-point atomic; the
 * order of the frontier and receiver lists enters no value.
 * dppr_debug_forward_push: a test hook. piece_edges and team as dppr_debug_forward; chunk_rounds in [0, 256]: the rounds enqueued
 * between two read-backs. 0: the plan decides. Every setting gives the same bits.
 * OUT OF SCOPE: a true scatter push (a hub that receives anything is gathered whole: the price of determinism), dense start
 * vectors, the subgraph family over p. (A forward vector kept current under the stream: dppr_ftrack_*; the
 * conductance sweep of a track's p, and a fresh track is the push bit for bit: dppr_ftrack_cluster.) (The ranked, position and
 * sample queries over a track's p: dppr_ftrack_topk_ranked and its siblings.) */
#define DPPR_FPUSH_SET_MAX 4096
#define DPPR_FPUSH_MAX_ROUNDS 256
typedef struct {
    int32_t *rounds_used; int32_t *converged; double *rem; int64_t *pushes; int64_t *left; /* [m], HOST; each may be NULL */
    int64_t *work;                                                      /* [3], HOST; may be NULL */
    int32_t k; double min_p; int32_t *topk_ids; double *topk_p; int32_t *topk_counts; /* [m][k], [m][k], [m], HOST */
    const int32_t *at_ids; int32_t n_at; double *at_p; double *at_r;    /* [n_at], [n_at][m], [n_at][m], HOST */
    void *dense_p_dev; void *dense_r_dev; int32_t dense_dtype, dense_layout; /* DEVICE; as dppr_forward_out_t */
} dppr_forward_push_out_t;
int dppr_forward_push(dppr_engine *e, int32_t epoch, const int64_t *offsets /* [m + 1], HOST */, const int32_t *ids, const double *weights,
                      int32_t m, double eps, int32_t max_rounds, const dppr_forward_push_out_t *out);
int dppr_debug_forward_push(dppr_engine *e, int piece_edges, int team, int chunk_rounds /* 0: the plan decides */);

/* ---- forward track: forward PPR of weighted start sets kept current under the stream (backward-compatible additions, ABI 6) ----
 * dppr_forward_push starts from zero on every call. A FORWARD TRACK keeps the push state (p, r) of up to DPPR_FORWARD_MAX_M weighted
 * start sets inside the engine and moves it from epoch k to epoch k + 1 by a fix-up over that epoch's batch records and signed push
 * rounds over the rows the fix-up disturbed. Read side only with respect to the solver: no slot or group state is read or changed,
 * the call takes no part in dppr_update / dppr_group_update or in a timed region, no id is assigned. An engine holds at most
 * DPPR_FTRACK_MAX tracks.
 *
 * DEFINITION. M, d(u), stored edges, duplicates, self loops, the per-vertex term, THE FOLD and the row order are those of
 * dppr_forward / dppr_forward_push. Write P = p / 0.15 for the mass pushed at a vertex. The state of a column keeps
 *     r[w] = h[w] - P[w] + sum over stored edges u -> w of 0.85 * P[u] * mult / (d(u) + 1)                                  (I)
 * on the epoch it stands on, to rounding. (I) alone gives pihat_h = p + sum_u r[u] * pihat_u exactly, so
 * |pihat_h[t] - p[t]| <= sum |r| entrywise; a converged column has |r[u]| <= eps * (d(u) + 1) everywhere.
 *   create, on epoch k   p = 0, r = h, then the rounds below; the rowless-seed rule of dppr_forward_push applies (p = 0.15 * w,
 *                    r = +0.0 at a seed that no stored edge of the epoch names). With non-negative r the signed test is the
 *                    unsigned one: a fresh track equals dppr_forward_push with the same sets, eps and max_rounds bit for bit in
 *                    p, r, rem, rounds_used, converged, pushes, left, work.
 *   fix-up, k -> k + 1   over the records i = 0 .. L - 1 of epoch k + 1's batch as dppr_set_batch staged them (tail, head,
 *                    is_insert; the mirrored copies of an undirected window are records like any other), per column, by
 *                    external id.
 *                    STEP T, for every vertex u that is the tail of at least one record: n_ins, n_del its insert and delete
 *                    records, d1 = d(u) on epoch k + 1, d0 = d1 - n_ins + n_del. g[u] = p[u] / (0.15 * (double)(d0 + 1)) (one
 *                    multiplication, one division, from p before any change), c[u] = 0.85 * g[u]. Only if d1 != d0:
 *                    p[u] = (p[u] * (double)(d1 + 1)) / (double)(d0 + 1) and r[u] = r[u] - (double)(d1 - d0) * g[u] (one
 *                    multiplication, one subtraction). A tail with d1 == d0 keeps p[u] and r[u] to the bit.
 *                    STEP H, after step T is complete, for every vertex w that is the head of at least one record, the records
 *                    in ascending i: r[w] = r[w] + c[tail_i] for an insert, r[w] = r[w] - c[tail_i] for a delete. The sum is
 *                    sequential, one rounding per record.
 *                    Rescaling P[u] by (d1 + 1) / (d0 + 1) leaves 0.85 * P[u] / (d(u) + 1) unchanged on every kept edge, so (I)
 *                    changes only at u and at the heads of the changed edges. A vertex new in the batch has p = r = 0; a vertex
 *                    whose last edge leaves gets d1 = 0 and keeps its values (the state is by external id).
 *   rounds           those of dppr_forward_push with the frontier F = { u : |r[u]| > thr[u] }, strict; the push is the same three
 *                    assignments, r, y and the fold's terms may be negative. r is never -0.0, so a row without a frontier
 *                    in-neighbour keeps its bits and is skipped; the definition stays the dense one (tests/ftrack_ref.py).
 *   rem              THE FOLD of |r| over the external ids 0 .. V - 1; dppr_forward_push's rem bit for bit while r >= 0.
 *   independence     a column is a function of the epochs' rows, the batches, its own set, eps and the max_rounds of each call:
 *                    not of the other columns, of m, of the grid, of the chunking, of dppr_debug_forward_push, of a renumbering
 *                    of the internal ids beyond the row order the fold already follows, or of anything the solver did.
 * CALLS. dppr_ftrack_create validates as dppr_forward_push does, runs the create step on `epoch` and hands out a track id in
 * [0, DPPR_FTRACK_MAX); `out` may be NULL. dppr_ftrack_update accepts exactly two epochs: the track's own (no fix-up, up to
 * max_rounds more rounds, for a column that stopped unconverged) and the next one (fix-up, then rounds): the sequence rule of
 * dppr_update. Anything else -- a skipped epoch, an older one, one that is not resident (for instance after a renumbering slide
 * the track did not follow: create a new track) -- is DPPR_ERR_INVALID with the track unchanged. dppr_ftrack_read writes the
 * outputs of the state as it stands; dppr_ftrack_info returns the epoch, m, eps and the start sets (offsets [m + 1]; ids and
 * weights when `cap` holds them all, else DPPR_ERR_INVALID with the size in offsets[m]); dppr_ftrack_destroy frees the track.
 * OUTPUTS: dppr_ftrack_out_t is dppr_forward_push_out_t with rem as defined above and fix[3] (int64, HOST): records applied,
 * distinct tails, distinct heads. rounds_used, pushes, left, work and fix are those of the last create or update call;
 * dppr_ftrack_read returns them unchanged.
 * The state is held as [V][row width] planes by EXTERNAL id: a renumbering, a parking or a revival never touches it, and a track
 * never blocks a renumbering. Every call loads it into the planes of the forward family through the id map and stores it back:
 * two whole-V copies, the fixed cost of a call.
 * Input rules, rejection before any device work, the id-map lock, stream, work-space ownership and DPPR_ERR_NOMEM behave as for
 * dppr_forward_push; dppr_debug_forward_push applies to the rounds unchanged, and every setting gives the same bits. No output
 * value comes from a floating-point atomic; no output position or value depends on the order of a list.
 * OUT OF SCOPE: changing a track's sets in place, tracks that span engines, the subgraph family over a track's p, any change
 * to the reverse update path. (The conductance sweep of a track's p: dppr_ftrack_cluster.) (Ranked candidates, positions and
 * samples over a track's p: dppr_ftrack_topk_ranked / _rank_score_at / _position_at / _sample.) */
#define DPPR_FTRACK_MAX 16
typedef struct {
    int32_t *rounds_used; int32_t *converged; double *rem; int64_t *pushes; int64_t *left; /* [m], HOST; each may be NULL */
    int64_t *work;                                                      /* [3], HOST; may be NULL */
    int32_t k; double min_p; int32_t *topk_ids; double *topk_p; int32_t *topk_counts; /* [m][k], [m][k], [m], HOST */
    const int32_t *at_ids; int32_t n_at; double *at_p; double *at_r;    /* [n_at], [n_at][m], [n_at][m], HOST */
    void *dense_p_dev; void *dense_r_dev; int32_t dense_dtype, dense_layout; /* DEVICE; as dppr_forward_out_t */
    int64_t *fix;                                                       /* [3], HOST; may be NULL */
} dppr_ftrack_out_t;
int dppr_ftrack_create(dppr_engine *e, int32_t epoch, const int64_t *offsets /* [m + 1], HOST */, const int32_t *ids, const double *weights,
                       int32_t m, double eps, int32_t max_rounds, const dppr_ftrack_out_t *out /* may be NULL */, int32_t *out_track);
int dppr_ftrack_update(dppr_engine *e, int32_t track, int32_t epoch, int32_t max_rounds, const dppr_ftrack_out_t *out /* may be NULL */);
int dppr_ftrack_read(dppr_engine *e, int32_t track, const dppr_ftrack_out_t *out);
int dppr_ftrack_info(dppr_engine *e, int32_t track, int32_t *epoch, int32_t *m, double *eps, int64_t *offsets /* [17] */, int32_t *ids,
                     double *weights, int64_t cap);
int dppr_ftrack_destroy(dppr_engine *e, int32_t track);
/* With dppr_set_profiling on: the device time in ms of the last create or update call, cut into [4]: the load, the fix-up, the
 * rounds (the scan of the candidates and the count of `left` with them), the store with the fold of rem. -1 before the first. */
int dppr_debug_ftrack_ms(dppr_engine *e, float *out_ms /* [4] */);

/* ---- local cluster of a forward track: a full-length conductance sweep over p (backward-compatible additions, ABI 6) ----
 * The forward push vector of a start set is what PageRank-Nibble sweeps for a low-conductance cut (Andersen, Chung, Lang, FOCS
 * 2006), and the guarantee is about the sweep over the WHOLE support. dppr_cluster cannot be pointed at a track: its order is raw
 * p where ACL needs p / degree, and it ends at DPPR_CLUSTER_MAX positions. dppr_ftrack_cluster orders every qualifying vertex of
 * the window -- up to V per column -- and sweeps the order on the device, next to the state, instead of a dense read of p +
 * dppr_read_out_graph + a sweep on the host. Read side only: the track, the solver's states and the epoch are not changed.
 *
 * For column c of the track, on the epoch the track stands on, every output is defined exactly:
 *   SCORE     p[v] is what dppr_ftrack_read returns at v; outdeg(v) is the stored out-degree with multiplicity.
 *             DPPR_FCLUSTER_BY_P: score = p[v]. DPPR_FCLUSTER_BY_P_OVER_DEG: score = p[v] / (double)(outdeg(v) + 1), ONE division,
 *             nothing fused.
 *   QUALIFIES v qualifies if at least one stored edge of the epoch names it as tail or head and score > min_score (min_score >= 0).
 *             A track's p can be negative after deletes: a negative score, a +-0 score and a NaN score never qualify; +infinity
 *             orders first. A seed that no stored edge names is in no order, whether or not it has an internal id (the
 *             rowless-seed rule of dppr_forward_push: such a seed has no edge to cut, and the result stays a function of the
 *             epoch alone).
 *   ORDER     v_0 .. v_{L-1}: score descending, external id ascending. L = #qualifying if max_len == 0, else
 *             min(max_len, #qualifying). count = L.
 *   GRAPH, PREFIX, BEST   word for word those of dppr_cluster: the out-CSR of the epoch with multiplicity, a self loop never
 *             crosses a cut, Ed is what dppr_graph_edges returns; with S_j = {v_0 .. v_j}: vol[j] = sum of outdeg over S_j,
 *             cut_out[j] = #{stored edges u -> w : u in S_j, w not in S_j}, cut_in[j] = #{stored edges u -> w : u not in S_j,
 *             w in S_j}; den[j] = min(vol[j], Ed - vol[j]); prefix j is eligible iff j + 1 >= min_size and den[j] > 0;
 *             phi[j] = (double)cut_out[j] / (double)den[j], one IEEE division; the best prefix is the first minimum (the smallest
 *             j among equal values); with no eligible prefix: best_size = 0, best_cut = best_vol = 0, best_phi = +infinity.
 *   Prefix property: the arrays of a smaller max_len are the head of those of a larger one.
 *   LAYOUT    one CSR over the columns under the capacity rule of dppr_export_sparse / dppr_subgraph: column c's entries occupy
 *             [offsets[c], offsets[c + 1]) of the five arrays, offsets[0] = 0, offsets[c + 1] - offsets[c] = L of column c.
 *             out_offsets [m + 1] and out_best [m] are HOST memory and are always written, with the TRUE counts. If
 *             offsets[m] > cap nothing is written to the five arrays and the call still returns DPPR_OK. cap = 0 with all five
 *             arrays NULL is the size-and-best query. dest (DPPR_DEST_HOST / DPPR_DEST_DEVICE): where the five arrays live; each
 *             may be NULL. A device destination is checked as the exports check theirs, before any device work (cap entries of
 *             the element type, cap taken as at most m * V, inside one allocation of the engine's device, aligned), and the call
 *             returns after the solver stream has finished writing. out_score holds the scores the order was made by. The members
 *             of the best cluster of column c are ids[offsets[c] .. offsets[c] + best_size).
 *   Determinism: the result is a function of the track's state and the epoch alone: not of the other columns, of the grid or of
 *             dppr_debug_ftrack_cluster. No output value or position comes from a floating-point atomic, and none from the return
 *             value of an atomic (integer sums count; the order in which the pieces of a long row are queued enters nothing).
 * Rejected with DPPR_ERR_INVALID before any device work, nothing written: no such track, an unknown order, min_score negative or
 * NaN, max_len < 0 or > V, min_size < 1, cap < 0, cap > 0 with every array NULL, a bad dest, a NULL out_best or out_offsets, a
 * bad device pointer, the track's epoch no longer resident, a broken engine.
 * Threading and stream as dppr_ftrack_read: the id-map lock for the whole call (safe beside dppr_slide_concurrent), the solver
 * stream, never part of an update or of a timed region. ONE read of the per-column counts by the host lies between the kernels,
 * as in dppr_subgraph, to size the sort. Work space: the p | r planes of the forward family, a 16-bit mask per external id, and
 * per qualifying (vertex, column) 24 bytes of sort keys and ids (in and out), per ordered position 60 bytes (ids, score, three
 * differences, three prefix sums), 4 bytes per (live row, column) of rank table, the sort's own scratch and the list of the
 * long rows' pieces; all of it is the engine's, grown on demand and released with the engine: after DPPR_ERR_NOMEM the track and
 * the engine are as before. With dppr_set_profiling on, dppr_debug_query_ms reports the call, first to last kernel (the one read
 * of the counts lies between them).
 * dppr_debug_ftrack_cluster: a test hook. scan_tile 0 or a power of two in [64, 4096]: positions of a tile of the multi-tile
 * prefix sum; piece_edges 0 or a power of two in [64, 4096]: rows longer than this are walked in pieces of this many entries.
 * 0: the plan decides. Every setting gives the same bits.
 * OUT OF SCOPE: masks and exclusions inside the sweep, the subgraph family over a track, the full-length sweep for slot and
 * group states, sweeps over dppr_forward / dppr_forward_push results that are not tracks (a fresh track is the push bit for
 * bit). (Factors, masks and exclusions over a track's p, as a ranked order: dppr_ftrack_topk_ranked and its siblings.) */
#define DPPR_FCLUSTER_BY_P           0   /* score = p[v]                              */
#define DPPR_FCLUSTER_BY_P_OVER_DEG  1   /* score = p[v] / (double)(outdeg(v) + 1)    */
typedef struct { int64_t count, best_size, best_cut, best_vol; double best_phi; } dppr_fcluster_t;
int dppr_ftrack_cluster(dppr_engine *e, int32_t track, int32_t order, double min_score, int64_t max_len, int32_t min_size,
                        int64_t cap, int dest,
                        dppr_fcluster_t *out_best   /* [m], HOST */,
                        int64_t *out_offsets        /* [m + 1], HOST */,
                        int32_t *out_ids, double *out_score,
                        int64_t *out_cut_out, int64_t *out_cut_in, int64_t *out_vol /* [cap] each, each may be NULL */);
int dppr_debug_ftrack_cluster(dppr_engine *e, int scan_tile, int piece_edges);

/* ---- rank, locate and sample over a forward track's p (backward-compatible additions, ABI 6) ----
 * A track is the engine's answer to "where does the walk from this user or this set go, kept current per batch": the recommender
 * and link-prediction vector. The head of its raw order is its own start set and what that set already links to; "who to follow"
 * is the forward vector with the seeds and their out-neighbours excluded and one vertex type allowed, and a held-out edge is
 * evaluated by the position of its head in that order. These calls point the ranked family -- dppr_rank_spec_t, the top k, the
 * score at given ids, the positions (MRR / Hits@K / percentile) and the samples (negatives, candidates) -- at a track, on the
 * device, instead of a dense copy of p + dppr_read_out_graph + numpy per batch. There is no `epoch` argument: as in
 * dppr_ftrack_cluster the graph is the epoch the track stands on. Read side only: the track and every solver state are unchanged.
 *
 * For column c of the track and external id v, every output is defined exactly:
 *   P            p = p_c[v] is exactly what dppr_ftrack_read returns at v (at_p). The track's state is by external id and
 *                complete: a seed that no stored edge names holds 0.15 * w, a parked vertex keeps its value, and after deletes p
 *                may be negative.
 *   OUTDEG       outdeg(v) is the stored out-degree of v on the track's epoch, with multiplicity; 0 for a vertex without a live
 *                row (no internal id, or parked).
 *   THE SCORE    word for word THE SCORE of dppr_topk_ranked: DPPR_FACTOR_NONE / _DEV / _DEG / _INV_DEG are one explicit rounding
 *                each, nothing fused; an f32 g is converted to double exactly; mask_dev and factor_dev are [V] by external id; a
 *                vertex that is masked out scores exactly +0.0.
 *   SEEDS        the seeds of column c are the ids dppr_ftrack_info lists for it, whatever their weights.
 *   EXCLUDED     DPPR_EXCLUDE_SEEDS excludes the seeds; DPPR_EXCLUDE_IN_NEIGHBOURS / _OUT_NEIGHBOURS exclude v with a stored edge
 *                v -> seed / seed -> v on the track's epoch, for any seed of the column. Exclusion is per column: a vertex
 *                excluded in column 2 may rank first in column 3. An excluded vertex scores +0.0 in that column.
 *   NO ID        THE ONE PLACE this differs from the NO ID rule of dppr_topk_ranked: a vertex without an internal id is not
 *                p = 0. Its score follows the formula from the track's own p_c[v] with outdeg = 0, so a rowless seed is in the
 *                raw order exactly as it is in dppr_ftrack_read's top k, and DPPR_EXCLUDE_SEEDS takes it out although it has
 *                no row.
 *   QUALIFIES, ORDER, POSITION, COUNTS, DUPLICATE IDS   those of dppr_group_topk_ranked / dppr_group_position_at with "lane" read
 *                as "column" and n as the track's m: score > min_score (min_score >= 0; a +-0, negative or NaN score never
 *                qualifies, +inf orders first), score descending then external id ascending, entries past a count hold id -1 and
 *                0.0, pos = -1 where the id does not qualify, every external id 0 .. V - 1 takes part.
 *   WEIGHT, TREE, UNIFORM, DESCENT, statuses   those of dppr_group_sample with the lane index i = the column; the limits are
 *                DPPR_SAMPLE_MAX and m * S <= DPPR_SAMPLE_MAX_TOTAL.
 *   EPOCH        a spec that reads no degree and no neighbour never looks at the graph: it works even when the track's epoch has
 *                left the ring. Otherwise the track's epoch must be resident, else DPPR_ERR_INVALID.
 *   INDEPENDENCE a column's outputs are a function of its own p, its seeds, the spec and the epoch: not of m, of the other columns,
 *                of the grid or of any debug hook.
 * Outputs: dppr_ftrack_topk_ranked ids [m][k], scores [m][k], counts [m]; dppr_ftrack_rank_score_at [n_ids][m], vertex-major;
 * dppr_ftrack_position_at pos [n_ids][m] and counts [m] (may be NULL); dppr_ftrack_sample as dppr_group_sample with n = m.
 * n_ids == 0 and S == 0 behave as in the group forms.
 * ANCHORS. (a) With spec == NULL, or the all-zero spec, the ids and scores equal the top k of dppr_ftrack_read(k, min_p =
 * min_score) bit for bit, a column whose only seed is rowless included. (b) dppr_ftrack_rank_score_at at any id equals the score
 * that places it in (a), bit for bit. (c) With DPPR_FACTOR_INV_DEG and nothing else, on a track with no rowless seed, the first k
 * ids and scores equal the first k of dppr_ftrack_cluster(DPPR_FCLUSTER_BY_P_OVER_DEG, min_score, max_len = k): two independent
 * device paths, a radix sort against a selection, agreeing to the bit. (d) The position anchors (a) - (b) of
 * dppr_group_position_at, taken against dppr_ftrack_topk_ranked. (e) The sample anchors (a) - (d) of dppr_group_sample, taken
 * against dppr_ftrack_rank_score_at.
 *
 * Rejected with DPPR_ERR_INVALID before any device work, nothing written: no such track; every spec rejection of dppr_topk_ranked
 * (enum values, exclude bits, the device-pointer range checks); k outside [1, DPPR_TOPK_MAX]; min_score negative or NaN; NULL
 * outputs where the group forms refuse them; n_ids < 0, an id outside [0, V), n_ids > DPPR_POSITION_MAX for positions; the sample
 * limits and a bad device destination; the epoch rule above; a broken engine.
 * Threading and stream as dppr_ftrack_read: the id-map lock for the whole call (safe beside dppr_slide_concurrent), the solver
 * stream, never part of an update or of a timed region.
 * SHAPE. The track's [V][row width] plane is read in place by external id; nothing is loaded into the forward family's planes. A
 * spec that excludes marks one 32-bit word per external id, bit c for column c (with a neighbour flag the one read of the seeds'
 * row lengths by the host lies between the kernels, as in dppr_topk_ranked). The top k and the positions then run over a
 * COMPACTED scratch state that holds a row only for an external id at which at least one column has score > min_score, in
 * ascending external id: a count per tile, a scan over the tiles, ONE read of the row count by the host (as in dppr_subgraph and
 * dppr_ftrack_cluster) and a fill that recomputes the scores and places each row by its rank inside its tile; no position comes
 * from an atomic. A dropped row qualifies in no column, so it is in no top k, precedes no position and joins no count: the
 * compaction cannot change a result. Zero kept rows is a valid result: every count is 0, ids are -1, positions are -1. A sample's
 * leaves are in external-id order already; nothing is compacted there.
 * Work space: 4 V bytes of exclusion words and 4 bytes per seed where the spec excludes, the row lengths and pieces of
 * dppr_topk_ranked, 12 bytes per tile, 8 m + 4 bytes per kept row of scratch state (the one of dppr_group_topk_ranked, not a second
 * one), then what the group forms take behind it; all of it is the engine's, obtained before the first kernel that uses it, grown
 * on demand and released with the engine: after DPPR_ERR_NOMEM the track and the engine are as before. With dppr_set_profiling
 * on, dppr_debug_query_ms reports the call, first to last kernel.
 * dppr_debug_ftrack_rank: a test hook. tile_rows 0 (the plan decides) or a power of two in [64, 1024]: external ids per tile of
 * the count / fill passes. Every setting gives the same bits.
 * OUT OF SCOPE: the subgraph, patch and changes families over a track; ranked queries over one-shot dppr_forward /
 * dppr_forward_push results (a fresh track is the push bit for bit); weight vectors across columns. */
int dppr_ftrack_topk_ranked(dppr_engine *e, int32_t track, const dppr_rank_spec_t *spec, int32_t k, double min_score,
                            int32_t *out_ids /* [m][k] */, double *out_score /* [m][k] */, int32_t *out_counts /* [m] */);
int dppr_ftrack_rank_score_at(dppr_engine *e, int32_t track, const dppr_rank_spec_t *spec, const int32_t *ids, int32_t n_ids,
                              double *out_score /* [n_ids][m] */);
int dppr_ftrack_position_at(dppr_engine *e, int32_t track, const dppr_rank_spec_t *spec, double min_score, const int32_t *ids,
                            int32_t n_ids, int32_t *out_pos /* [n_ids][m] */, int32_t *out_counts /* [m], may be NULL */);
int dppr_ftrack_sample(dppr_engine *e, int32_t track, const dppr_rank_spec_t *spec, double min_score, uint64_t seed, uint64_t first,
                       int32_t S, int dest, int32_t *out_ids /* [m][S] */, double *out_w /* may be NULL */,
                       double *out_total /* [m] */, int32_t *out_support /* may be NULL */, int32_t *out_status /* [m] */);
int dppr_debug_ftrack_rank(dppr_engine *e, int tile_rows);

/* Windows whose sweep groups are all resident at once run a frontier loop of a source group as
 * multi-sweep launches (grid barrier between sweeps, row tables kept in LDS; dppr_multi.hpp). on by
 * default; 0 = one launch per sweep everywhere. The roll-call / time-out rules are those of
 * dppr_set_persistent. Same results. */
int dppr_set_group_resident(dppr_engine *e, int on);
/* Edge slots of the single-source resident sweep (dppr_resident.hpp). sorted = 1 (default): every sweep group's edges are
 * dealt to the threads in the order of their gather position, so that the lanes of one gather instruction read the same
 * or neighbouring 64-byte sectors (table built with the group cut, untimed -- the reference builds its CSR untimed as well,
 * gpu/PPRGPU.cuh:131-135). sorted = 0: slots in CSR order (the form of rounds 1-2). Same pushes, same sums up to the order
 * of the additions. 1 takes effect with the next epoch built, 0 at once. */
int dppr_set_resident_slots(dppr_engine *e, int sorted);
/* IncrementalBatchUpdate inside the resident launch of a whole batch (dppr_resident.hpp, PLAN_UPDATE; on by default): the
 * workgroup that owns a tail applies its records -- same terms, same order per tail as the separate kernel
 * (gpu/StreamUpdate.cuh:34-76), bit-identical residuals -- before it seeds the frontier. dppr_update only (the split calls
 * dppr_incremental_batch_update + dppr_execute_main_loop always run the update as its own kernel). 0 = always a kernel of its own. */
int dppr_set_resident_update(dppr_engine *e, int on);
/* The tail of a source group's frontier loop as pushes. A sweep costs at least its floor (every out_col entry, every
 * sweep group's tables) however few (vertex, source) pairs are still being pushed; below enter_pairs frontier pairs
 * the loop's remaining iterations run as what the reference does for every iteration (gpu/ExpandRev.cuh:34-77,
 * :708-743: per frontier vertex and in-neighbour a returning atomic add, all sources of the group at once), same
 * synchronous schedule, same results up to the order of the sums. enter_pairs: -1 (default) = automatic: below
 * max(64, 2 pairs per sweep group) -- the factor 2 can be changed for tuning runs with the environment variable
 * DPPR_GROUP_PUSH_FACTOR, read in dppr_create --, 0 = never, N = below N pairs; an iteration with more in-edges than the floor is worth sends
 * the loop back to sweeps (max_edges: that bound on an iteration's in-edges; 0 = automatic, 20 per sweep group), to
 * try again on a much smaller frontier. list_cap: vertices a frontier list holds (0: keep; default 2^20). Windows
 * whose groups run as multi-sweep launches do not use it. */
int dppr_set_group_push(dppr_engine *e, int enter_pairs, int list_cap, int64_t max_edges);

/* How dppr_group_update seeds its two frontier loops. from_tails (default): after a converged solve
 * only tails of the batch's records can be legal (the argument of cpu/PPRCPUMTCilkRev.h:126-156), so
 * the frontier is read off the batch; 0: a full Inspect pass over all vertices per phase like
 * PPRRevPushGPU::ExecuteMainLoop (gpu/PPRRevPushGPU.cuh:97-104). Same frontier either way. */
int dppr_set_group_seeding(dppr_engine *e, int from_tails);

/* ---- validation / test hooks -------------------------------------------- */

/* Replaces: InspectPureRev alone (gpu/Inspect.cuh:8-48). Writes the legal vertices
 * (unordered) to out_ids (capacity vertex_count) and their count to *out_count. */
int dppr_inspect(dppr_engine *e, int32_t slot, int phase, double eps, int32_t *out_ids, int32_t *out_count);

/* Replaces: the D2H copies of in_row_ptr/in_col_ind in the -DVALIDATE CSR check
 * (gpu/PPRRevPushGPU.cuh:69-72). row_ptr: V+1, col: directed-edge count, out_degree: V
 * (any may be NULL). */
int dppr_read_graph(dppr_engine *e, int32_t epoch, int32_t *row_ptr, int32_t *col, int32_t *out_degree);
int dppr_graph_edges(dppr_engine *e, int32_t epoch, int32_t *out_directed_edges);
/* The out-CSR the pull sweep reads (rows sorted ascending). row_ptr: V+1, col: directed edges. */
int dppr_read_out_graph(dppr_engine *e, int32_t epoch, int32_t *row_ptr, int32_t *col);

/* Frontier trace (test hook): when enabled the host loop copies every iteration's
 * frontier back. dppr_trace_get returns them concatenated: offsets has n_iters+1
 * entries. Pass NULL buffers to query sizes. */
int dppr_trace_enable(dppr_engine *e, int32_t slot, int on);
int dppr_trace_get(dppr_engine *e, int32_t slot, int64_t *n_iters, int64_t *n_ids,
                   int64_t *offsets, int32_t *ids);

/* Waits for everything the engine has enqueued (the solver's and the builder's HIP streams). */
int dppr_synchronize(dppr_engine *e);

/* Lookahead for the untimed region (no reference counterpart: its graph update is serial,
 * gpu/PPRGPU.cuh:114-135). Tells the engine which id arrays the NEXT dppr_set_batch (b1, b2: L records) and dppr_slide
 * (n1, n2: c new edges) will be called with -- the SAME pointers and lengths, contents final and untouched until those
 * calls. Their external -> internal lookups (the dominant host cost of a large batch: 18 + 5 ms of a twitter-size
 * slide) then run on helper threads while the caller is inside dppr_update / dppr_group_update, and the two calls only
 * resolve what the lookups could not (ids without an internal id yet, parked vertices). Read-only on the engine: every
 * call that changes the id maps waits for the lookups first; after a renumbering, or when the pointers / lengths differ,
 * the hint is ignored. Results are identical with and without it.
 * Threads: this is the ONE call that may also come from another host thread than the engine's while that one is inside
 * dppr_update / dppr_group_update / dppr_incremental_batch_update / dppr_execute_main_loop (none of which touches the id maps) --
 * so a host can advance its own stream and hint from a helper while the update runs (./pagerank does) -- provided the helper
 * has returned from it before the engine's thread makes its next call. */
int dppr_hint_next_batch(dppr_engine *e, const int32_t *b1, const int32_t *b2, int32_t L, const int32_t *n1, const int32_t *n2, int32_t c);

/* What dppr_set_batch_grouping(at_slide = 1) and the batch upload move out of the reference's timed region
 * (gpu/PPRGPU.cuh:138-164 times CopyOutDegree + the whole IncrementalBatchUpdate): the post-batch out-degree gather and the
 * grouping of epoch `epoch`'s L records by tail (on the path the timed region takes), run `reps` times on the engine's stream between two
 * events; *out_ms = milliseconds per repetition. bench.py adds it to the measured batch time and reports both accountings
 * (config.timed_region). Touches scratch only. */
int dppr_time_batch_grouping(dppr_engine *e, int32_t epoch, int32_t reps, float *out_ms);
/* Test hook (ABI 6): the grouping of epoch `epoch`'s L records by tail, read back. path 0 = what the timed region would use for
 * this epoch (4 when it was grouped at slide; DPPR_GROUPING_RADIX counts), 1 = rank (L <= 64 Ki), 2 = bucket (L <= 4 Mi),
 * 3 = radix, 4 = the arrays grouped at slide (error when the epoch was not). Paths 0-3 run as dppr_time_batch_grouping does
 * (degrees into scratch; no solver state changes). tails_out / index_out: the L grouped (tail, record index) pairs (internal ids);
 * raw_tails_out: the epoch's L tails in batch order; *path_taken: 1-4; *nb_out: the buckets of path 2, else 0. Any pointer may be NULL. */
int dppr_debug_grouping(dppr_engine *e, int32_t epoch, int32_t path, uint32_t *tails_out, uint32_t *index_out, int32_t *raw_tails_out,
                        int32_t *path_taken, int32_t *nb_out);

/* Diagnostics for a call that does not come back (one unexplained 300-second guard in 13 suite runs). Writes a
 * text report into buf (at most cap bytes, NUL-terminated; returns the length written): last error, epoch / id-space
 * state, resident-launch settings, per slot and group the host-side loop state and statistics, and -- read through a
 * SEPARATE stream with a bounded wait, so that it works while the engine's own stream is stuck in a kernel -- the
 * GridBar words (roll-call outcome, check-ins, per-sweep arrivals) and the status words of resident / multi-sweep
 * launches. Callable from another host thread than the one inside the engine (it takes no lock: the host-side fields
 * are read racily, which is what a post-mortem wants). No reference counterpart (its loop is host-driven,
 * gpu/PPRRevPushGPU.cuh:106-130, and cannot wait on a device-side barrier). */
int dppr_debug_dump(dppr_engine *e, char *buf, int32_t cap);
/* Test hook (ABI 5): the binned-sweep tables of an epoch (dppr_binned.hpp) -- block cuts (n_a + 1 / n_b + 1 first vertices, internal
 * ids); the RUN list in A-major order (n_runs entries: head index inside its A-block, top bit = first run of its tile), per tile
 * (n_tiles, A-major order) the difference between its runs' B-major and A-major indices, per 64 runs the tile that holds the first of
 * them (n_runs / 64 + 1 entries, rounded up); the EDGE list in B-major order (n_edges entries: row index inside its B-block, top bit =
 * first edge of its run) and per 64 edges the run that holds the first of them (n_edges / 64 + 1 entries, rounded up); how many epochs
 * had their tables patched by the slide's merge and how many built by the sorts. Any pointer may be NULL. The patched tables must
 * equal, bit for bit, what the sorts produce under the same cuts (tests/test_binned_tables_gpu.py). */
int dppr_debug_bin_tables(dppr_engine *e, int32_t epoch, int32_t *n_a, int32_t *n_b, int32_t *n_edges, int32_t *n_runs, int32_t *n_tiles,
                          int32_t *acut, int32_t *bcut, uint16_t *hl, int32_t *tdelta, int32_t *tb, uint16_t *dl, int32_t *vb,
                          int64_t *patched, int64_t *rebuilt);
/* Leak check (backward-compatible addition, ABI 6): bytes of device memory and of pinned host memory that THIS PROCESS holds through
 * the library at the moment of the call, all engines together -- the library's own count, so other tenants of a shared device do
 * not show in it. Needs no engine; callable from any thread; either pointer may be NULL. After every engine has been destroyed both
 * are what they were before the first was created (0 in a process that made no other call that is still running). */
int dppr_debug_live_bytes(int64_t *device_bytes, int64_t *pinned_bytes);

/* A counter that advances at every host read-back of a frontier loop and every stage of a graph build (ABI 4): a watchdog
 * samples it so that ONE long call (the first solve on a large window, a group's from-scratch solve) is told from a hang
 * (ADVICE r04). Callable from any thread. */
unsigned long long dppr_heartbeat(const dppr_engine *e);

/* Microbenchmark used to calibrate the roofline ceiling of the push kernel
 * (SURVEY.md 8d): n returning f64 atomic adds per launch at pseudo-random
 * addresses of a table of table_elems doubles; scope 0 = agent, 1 = workgroup.
 * Returns the average kernel time in ms over reps launches. */
int dppr_bench_atomics(int device, int64_t table_elems, int64_t n, int scope, int reps, float *out_ms);
/* The other two calibrated ceilings of SURVEY.md 8(d), measured by bench.py in the run that prints the line (ABI 4):
 * dppr_bench_line_fills -- `lines` random 128-byte line fetches (one request per 8 lanes, the access shape of the group
 * sweep's row gathers) out of a table of table_bytes (a power of two; 1 GiB = beyond every cache); *out_ms = time for
 * `lines` fetches. dppr_bench_stream_copy -- a streaming copy of `bytes` (read + write): *out_ms per copy. */
int dppr_bench_line_fills(int device, int64_t table_bytes, int64_t lines, int reps, float *out_ms);
int dppr_bench_stream_copy(int device, int64_t bytes, int reps, float *out_ms);

/* Identity of the build: the first 16 hex digits of the SHA-256 over the kernel / engine sources the library was compiled
 * from (the .hpp files of csrc in name order, csrc/dppr_engine.hip, include/dppr.h; see csrc/Makefile). Profiles under profiles/ carry the id of
 * the library that produced them; bench.py refuses counter traffic measured on another build. */
const char *dppr_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* DPPR_H */
