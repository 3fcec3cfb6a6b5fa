// ppr_gpu.hpp -- driver classes of ./pagerank over the C ABI (include/dppr.h).
//
// PPRGPU keeps the reference's driver shape (gpu/PPRGPU.cuh:21-198): DynamicExecute(),
// SlidingWindowExecuteMainLoop() and the four virtuals GPUBuildSlidingGraph /
// IncrementalBatchUpdate / ExecuteMainLoop(phase) / ValidateResult, the same timed scope
// (gpu/PPRGPU.cuh:138-164) and the same stdout contract (:116-124, :170-176). What differs:
//   * one engine (= one device, one window-graph replica) serves SEVERAL source vertices;
//   * no CUDA types here -- everything device-side sits behind libdppr_hip.so;
//   * validation is a run-time flag (--validate) instead of -DVALIDATE;
//   * errors come back as status codes; this layer prints and exits like CUDA_ERROR did
//     (gpu/GPUUtil.cuh:7-19).
#pragma once

#include <atomic>
#include <future>
#include <thread>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/dppr.h"
#include "graph_vec.hpp"
#include "meta.hpp"

#define DPPR_CHECK(eng, call)                                                                       \
    do {                                                                                            \
        int _rc = (call);                                                                           \
        if (_rc != DPPR_OK) {                                                                       \
            std::cout << dppr_strerror(_rc) << " (" << dppr_last_error(eng) << ") in " << __FILE__  \
                      << " at line " << __LINE__ << std::endl;                                      \
            std::exit(-1);                                                                          \
        }                                                                                           \
    } while (0)

// --profile: what the reference prints when it is compiled with -DPROFILE (ProfileCommon.h:6-31 phase and counter
// names, GPUProfiler::ReportProfile gpu/GPUProfiler.cuh:42-55, the per-iteration line of gpu/PPRRevPushGPU.cuh:109-111).
// Phases are timed on the host clock around calls that synchronise the stream, scoped as gpu/PPRGPU.cuh:47-163 scopes
// them. Inspect, Expand and RepairFrontier are ONE kernel per iteration here: their event-timed total is reported as
// expand_time, inspect_time / repair_frontier_time stay 0 (as do the phases the reference's GPU path never starts).
struct HostProfile {
    enum Phase { INSPECT, EXPAND, INIT_GRAPH_CALC, DYNA_GRAPH_CALC, EXCLUDE_GRAPH_UPDATE, SORT, REDUCE, REPAIR_FRONTIER,
                 INC_UPDATE, PUSH, TOTAL, PPR, PPR_UPDATE, PPR_QUERY, N_PHASES };
    double ms[N_PHASES] = {0};
    timespec t0[N_PHASES];
    void Start(Phase p) { clock_gettime(CLOCK_MONOTONIC, &t0[p]); }
    void End(Phase p) {
        timespec b;
        clock_gettime(CLOCK_MONOTONIC, &b);
        ms[p] += (b.tv_sec - t0[p].tv_sec) * 1e3 + (b.tv_nsec - t0[p].tv_nsec) * 1e-6;
    }
    static const char *Name(int p) {
        static const char *names[N_PHASES] = {"inspect_time", "expand_time", "init_graph_calculation_time",
                                              "dynamic_graph_calculation_time", "exclude_graph_update_time", "sort_time",
                                              "reduce_time", "repair_frontier_time", "inc_update_time", "push_time",
                                              "total_time", "ppr_time", "ppr_update_time", "ppr_query_time"};
        return names[p];
    }
};

class PPRGPU {
public:
    PPRGPU(SlidingGraphVec *g, int device, const std::vector<IndexType> &sources, bool quiet)
        : graph(g), device_id(device), source_vertex_ids(sources), quiet_(quiet) {
        if (!quiet_)
            for (IndexType s : sources) std::cout << "choose " << s << " as source vertex id" << std::endl;
        // two resident epochs: the graph of batch k + 1 is built (dppr_slide_concurrent) while batch k is being solved
        overlap_ = !gValidate && !gSplitInterface && std::getenv("DPPR_NO_OVERLAP") == nullptr;
        int rc = dppr_create(&engine, device, g->vertex_count, g->sliding_window_size, g->directed ? 1 : 0,
                             (int32_t)gStreamUpdateCountPerBatch, overlap_ ? 2 : 1);
        if (rc != DPPR_OK) {
            std::cout << "dppr_create: " << dppr_strerror(rc) << std::endl;
            std::exit(-1);
        }
        DPPR_CHECK(engine, dppr_set_variant(engine, gVariant)); // (-o: the variant's mechanisms and its schedule)
        if (gSchedule) DPPR_CHECK(engine, dppr_set_schedule(engine, gSchedule)); // (--sync on an eager variant)
        if (gPushOnly) DPPR_CHECK(engine, dppr_set_tuning(engine, 256, 512, -1, 0, 0)); // (--push-only: every iteration through the push kernels)
        if (gMergePhases) DPPR_CHECK(engine, dppr_set_phase_merge(engine, 1, 0)); // (--merge-phases: include/dppr.h; not the reference's schedule)
        ppr_time.assign(sources.size(), 0.0f);
    }
    virtual ~PPRGPU() { dppr_destroy(engine); }

    // gpu/PPRGPU.cuh:64-108
    virtual void DynamicExecute() {
        prof.Start(HostProfile::TOTAL);
        prof.Start(HostProfile::INIT_GRAPH_CALC);
        {
            EdgeBatch init_stream(graph->sliding_window_size);
            graph->SerializeEdgeStream(&init_stream);
            DPPR_CHECK(engine, dppr_load_window(engine, init_stream.edge1, init_stream.edge2, init_stream.length));
        }
        // several sources on one device are solved together, up to 16 per group (multi-source batched
        // sweeps); --split keeps the reference's one-source-at-a-time driver flow
        use_groups = (source_vertex_ids.size() > 1 && !gSplitInterface && !gNoGroups) || !target_lanes.empty(); // (set lanes exist in groups only)
        // two or three sources on a large window: one after the other on the single-source path (binned sweeps) beats a group, whose
        // sweep costs about the same for 2 as for 8 sources (friendster stand-in, 3 sources: 422 ms per batch as a group, 3 x 100 in series)
        // (--topk-weights asks for the group)
        if (use_groups && source_vertex_ids.size() <= 3 && graph->sliding_window_size >= 4000000 && !gTopKWeightsGiven && !gAssign && target_lanes.empty()) use_groups = false;
        if (gProfile) DPPR_CHECK(engine, dppr_set_profiling(engine, 1));
        if (!quiet_) std::cout << "start..." << std::endl;
        if (use_groups) {
            for (size_t i = 0; i < source_vertex_ids.size(); i += kGroupMax) {
                const int32_t n = (int32_t)std::min<size_t>(kGroupMax, source_vertex_ids.size() - i);
                int32_t gid = -1;
                if (target_lanes.empty()) {
                    DPPR_CHECK(engine, dppr_add_source_group(engine, source_vertex_ids.data() + i, n, &gid));
                } else { // --target-sets: lanes i .. i + n of this device as one group of weighted vertex sets
                    std::vector<int64_t> off(1, 0);
                    std::vector<int32_t> ids;
                    std::vector<double> w;
                    for (int32_t j = 0; j < n; ++j) {
                        for (const auto &sd : gTargetSets[target_lanes[i + (size_t)j]]) {
                            ids.push_back(sd.first);
                            w.push_back(sd.second);
                        }
                        off.push_back((int64_t)ids.size());
                    }
                    DPPR_CHECK(engine, dppr_add_target_group(engine, off.data(), ids.data(), w.data(), n, &gid));
                }
                groups.push_back(gid);
            }
            ppr_time.assign(groups.size(), 0.0f);
            for (size_t k = 0; k < groups.size(); ++k) {
                float ms = 0;
                DPPR_CHECK(engine, dppr_group_init_solve(engine, groups[k], gTolerance, &ms));
                progress++;
                if (!quiet_) std::cout << "elapsed time=" << ms << "ms" << std::endl;
            }
            if (gValidate)
                for (size_t i = 0; i < source_vertex_ids.size(); ++i) ValidateResult(i);
        } else {
            slots.resize(source_vertex_ids.size());
            for (size_t i = 0; i < slots.size(); ++i)
                DPPR_CHECK(engine, dppr_add_source(engine, source_vertex_ids[i], &slots[i]));
            for (size_t i = 0; i < slots.size(); ++i) { // Init + ExecuteMainLoop(0)
                float ms = 0;
                if (gProfile) DPPR_CHECK(engine, dppr_trace_enable(engine, slots[i], 1));
                DPPR_CHECK(engine, dppr_init_solve(engine, slots[i], gTolerance, &ms));
                progress++;
                if (gProfile) PrintIterations(i, 0);
                if (!quiet_) std::cout << "elapsed time=" << ms << "ms" << std::endl;
                if (gValidate) ValidateResult(i);
            }
        }
        if (gChangesK > 0) { // --changes: the from-scratch solution is the first mark
            for (int32_t gid : groups) DPPR_CHECK(engine, dppr_group_mark(engine, gid));
            for (int32_t sl : slots) DPPR_CHECK(engine, dppr_mark(engine, sl));
        }
        if (gPatchGiven) { // --patch-min: the from-scratch solution is the mark the first patch is taken against
            for (int32_t gid : groups) DPPR_CHECK(engine, dppr_group_mark(engine, gid));
            for (int32_t sl : slots) DPPR_CHECK(engine, dppr_mark(engine, sl));
        }
        if (gCertify > 0) PrintCertify(-1); // --certify: the from-scratch solution first
        if (!gTrackSets.empty()) PrintForwardTrack(-1, true); // --forward-track: created on the window the initial solve ran on
        prof.End(HostProfile::INIT_GRAPH_CALC);
        prof.Start(HostProfile::DYNA_GRAPH_CALC);
        if (overlap_) SlidingWindowExecuteOverlapped();
        else SlidingWindowExecuteMainLoop();
        prof.End(HostProfile::DYNA_GRAPH_CALC);
        prof.End(HostProfile::TOTAL);
        if (!quiet_) std::cout << "finish!" << std::endl;
        if (std::getenv("DPPR_HOST_TIMES")) // (stderr, not a line of the reference: the loop's wall time beside the ppr_time it reports)
            std::cerr << "host_times batches=" << batches_done << " dynamic_ms=" << prof.ms[HostProfile::DYNA_GRAPH_CALC]
                      << " graph_update_ms=" << prof.ms[HostProfile::EXCLUDE_GRAPH_UPDATE] << " ppr_ms=" << prof.ms[HostProfile::PPR]
                      << " graph_update_beside_ppr_ms=" << build_beside_ms << " overlap=" << (overlap_ ? 1 : 0) << std::endl;
        if (gProfile && !quiet_) ReportProfile();
    }

    // gpu/PPRRevPushGPU.cuh:109-111: one line per frontier iteration of the loop that just ran (the engine's iteration
    // trace holds the frontier of every iteration; it is cleared for the next loop)
    void PrintIterations(size_t i, size_t phase_id) {
        int64_t n_iters = 0, n_ids = 0;
        DPPR_CHECK(engine, dppr_trace_get(engine, slots[i], &n_iters, &n_ids, nullptr, nullptr));
        std::vector<int64_t> off((size_t)n_iters + 1, 0);
        if (n_iters > 0) DPPR_CHECK(engine, dppr_trace_get(engine, slots[i], nullptr, nullptr, off.data(), nullptr));
        if (!quiet_)
            for (int64_t it = 0; it < n_iters; ++it)
                std::cout << "phase_id=" << phase_id << ",iteration_id=" << it << ",frontier_count=" << off[(size_t)it + 1] - off[(size_t)it]
                          << std::endl;
        DPPR_CHECK(engine, dppr_trace_enable(engine, slots[i], 1)); // (clears it)
    }

    // GPUProfiler::ReportProfile (gpu/GPUProfiler.cuh:42-55)
    void ReportProfile() {
        long long traverse = 0, expand = 0;
        for (size_t i = 0; i < slots.size(); ++i) {
            dppr_stats_t st;
            DPPR_CHECK(engine, dppr_stats(engine, slots[i], &st));
            prof.ms[HostProfile::EXPAND] += st.push_ms;
            traverse += st.sum_E;
            expand += st.sum_F;
        }
        std::cout << "****************** profile time **********************" << std::endl;
        for (int j = 0; j < HostProfile::N_PHASES; ++j) std::cout << "[" << HostProfile::Name(j) << "]=" << prof.ms[j] << "ms ";
        std::cout << std::endl;
        std::cout << "[traverse_count]=" << traverse << " [expand_count]=" << expand
                  << " [update_pos_residual_count]=0 [update_neg_residual_count]=0 [update_random_walk_count]=0 " << std::endl;
        std::cout << "****************** end profile  **********************" << std::endl;
    }

    // gpu/PPRGPU.cuh:109-177
    virtual void SlidingWindowExecuteMainLoop() {
        size_t stream_batch_count = 0;
        if (std::getenv("DPPR_TEST_STALL")) // (test hook: a driver that stops making progress -- the watchdog's post-mortem path)
            for (;;) std::this_thread::sleep_for(std::chrono::seconds(1));
        // Lookahead (include/dppr.h dppr_hint_next_batch): once batch k's graph is built, a helper thread advances the host stream to
        // batch k+1 and tells the engine which id arrays it will get next -- the stream advance and the id lookups then run while
        // this thread waits for batch k's update (the reference's untimed region, gpu/PPRGPU.cuh:114-135, is serial). Not with
        // --validate (its power iteration reads the host graph at batch k); DPPR_NO_LOOKAHEAD=1 for A/B runs. Results are identical.
        const bool lookahead = !gValidate && std::getenv("DPPR_NO_LOOKAHEAD") == nullptr;
        bool ahead = false, ahead_end = false; // the next batch is staged in graph->edge_batch / new_stream already | the stream ended there
        std::future<int> ahead_task;
        while (stream_batch_count++ < gStreamBatchCount) {
            if (!quiet_ && (gStreamUpdateCountPerBatch > 100 || stream_batch_count % 100 == 0))
                Report(stream_batch_count);
            progress++;
            prof.Start(HostProfile::EXCLUDE_GRAPH_UPDATE);
            if (ahead ? ahead_end : graph->StreamUpdates(gStreamUpdateCountPerBatch)) break; // partial batch: dropped
            ahead = false;
            // ---- untimed: batch upload + device graph rebuild ----
            DPPR_CHECK(engine, dppr_set_batch(engine, graph->edge_batch->edge1, graph->edge_batch->edge2,
                                              graph->edge_batch->is_insert, graph->edge_batch->length));
            GPUBuildSlidingGraph();
            progress++;
            prof.End(HostProfile::EXCLUDE_GRAPH_UPDATE);
            if (lookahead && stream_batch_count < gStreamBatchCount) { // (both calls above have consumed the host arrays of batch k)
                ahead = true;
                ahead_task = std::async(std::launch::async, [this, &ahead_end] {
                    ahead_end = graph->StreamUpdates(gStreamUpdateCountPerBatch);
                    if (ahead_end) return (int)DPPR_OK;
                    return dppr_hint_next_batch(engine, graph->edge_batch->edge1, graph->edge_batch->edge2, graph->edge_batch->length,
                                                graph->new_stream->edge1, graph->new_stream->edge2, graph->new_stream->length);
                });
            }
            prof.Start(HostProfile::PPR);
            // ---- timed: IncrementalBatchUpdate + ExecuteMainLoop(0) + (1), per source or per group ----
            for (size_t k = 0; k < groups.size(); ++k) {
                float ms = 0;
                DPPR_CHECK(engine, dppr_group_update(engine, groups[k], -1, gTolerance, &ms));
                ppr_time[k] += ms;
            }
            if (use_groups && gValidate)
                for (size_t i = 0; i < source_vertex_ids.size(); ++i) ValidateResult(i);
            for (size_t i = 0; i < slots.size(); ++i) {
                float ms = 0;
                if (gSplitInterface) {
                    // timed on the host: the three calls each synchronise the stream
                    struct timespec a, b;
                    clock_gettime(CLOCK_MONOTONIC, &a);
                    prof.Start(HostProfile::INC_UPDATE);
                    IncrementalBatchUpdate(i);
                    prof.End(HostProfile::INC_UPDATE);
                    prof.Start(HostProfile::PUSH);
                    ExecuteMainLoop(i, 0);
                    if (gProfile) PrintIterations(i, 0);
                    ExecuteMainLoop(i, 1);
                    if (gProfile) PrintIterations(i, 1);
                    prof.End(HostProfile::PUSH);
                    clock_gettime(CLOCK_MONOTONIC, &b);
                    ms = (float)((b.tv_sec - a.tv_sec) * 1e3 + (b.tv_nsec - a.tv_nsec) * 1e-6);
                } else {
                    DPPR_CHECK(engine, dppr_update(engine, slots[i], -1, gTolerance, &ms));
                }
                ppr_time[i] += ms;
                if (gValidate) ValidateResult(i);
            }
            prof.End(HostProfile::PPR);
            if (ahead_task.valid()) {
                const int ahead_rc = ahead_task.get();
                DPPR_CHECK(engine, ahead_rc);
            }
            if (gChangesK > 0) PrintChanges(stream_batch_count);
            if (gPatchGiven) PrintPatch(stream_batch_count);
            if (gAssign) PrintAssign(stream_batch_count);
            if (!gRefineIds.empty()) PrintRefined(-1);
            if (!gPositionIds.empty()) PrintPositions(-1);
            if (gSample > 0) PrintSamples(-1);
            if (!gForwardIds.empty()) PrintForward(-1);
            if (!gPushSets.empty()) PrintForwardPush(-1);
            if (!gTrackSets.empty()) PrintForwardTrack(-1, false);
            if (!gExplainIds.empty()) PrintExplained(-1);
            if (gCertify > 0 && stream_batch_count % (size_t)gCertify == 0) PrintCertify(-1);
            if (gClusterK > 0) PrintClusters(-1);
            if (gSubgraphK > 0) PrintSubgraphs(-1);
        }
        batches_done = stream_batch_count - 1;
        if (!quiet_) Report(stream_batch_count);
        if (!quiet_) { // (not a line of the reference: how far the engine's internal id space is from the window's vertices)
            int32_t ids = 0, parked = 0, renumberings = 0;
            int64_t revivals = 0;
            DPPR_CHECK(engine, dppr_id_space(engine, &ids, &parked, &renumberings, &revivals));
            std::cout << "id_space ids=" << ids << " parked=" << parked << " renumberings=" << renumberings
                      << " revivals=" << revivals << std::endl;
        }
    }

    // The same loop with the untimed region of batch k + 1 (host stream advance, batch upload, device graph build: gpu/PPRGPU.cuh:114-135)
    // running on a helper thread WHILE batch k is solved. The engine keeps two epochs; the helper builds epoch
    // k + 1 through dppr_set_batch + dppr_slide_concurrent (own HIP stream and scratch inside the engine), this thread solves the
    // explicitly named epoch k. What this thread still waits for -- the first batch's graph, the remainder of a build that outlasts
    // its solve, and any slide that has to be exclusive (a renumbering of the id space moves every state row: dppr_renumbering_due)
    // -- is what exclude_graph_update_time reports; the helper's own time is reported beside it. Same stdout lines, same results
    // (DPPR_NO_OVERLAP=1: the serial loop above with its id lookahead; --validate and --split use that one too).
    struct Built {
        bool end = false;      // the stream ended: no such batch (a partial last batch is dropped, like the reference's)
        bool deferred = false; // host stream advanced, but batch upload + slide wait for the solver (exclusive slide)
        int32_t epoch = -1;
        double ms = 0;
    };
    Built BuildNext(bool concurrent) {
        Built b;
        timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        b.end = graph->StreamUpdates(gStreamUpdateCountPerBatch);
        if (!b.end) {
            if (concurrent && dppr_renumbering_due(engine)) {
                b.deferred = true;
            } else {
                DPPR_CHECK(engine, dppr_set_batch(engine, graph->edge_batch->edge1, graph->edge_batch->edge2, graph->edge_batch->is_insert,
                                                  graph->edge_batch->length));
                if (concurrent)
                    DPPR_CHECK(engine, dppr_slide_concurrent(engine, graph->new_stream->edge1, graph->new_stream->edge2, graph->new_stream->length, &b.epoch));
                else
                    DPPR_CHECK(engine, dppr_slide(engine, graph->new_stream->edge1, graph->new_stream->edge2, graph->new_stream->length, &b.epoch));
            }
        }
        clock_gettime(CLOCK_MONOTONIC, &t1);
        b.ms = (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6;
        progress++;
        return b;
    }

    virtual void SlidingWindowExecuteOverlapped() {
        size_t stream_batch_count = 0;
        if (std::getenv("DPPR_TEST_STALL")) // (test hook, as in the serial loop)
            for (;;) std::this_thread::sleep_for(std::chrono::seconds(1));
        prof.Start(HostProfile::EXCLUDE_GRAPH_UPDATE);
        Built nxt = gStreamBatchCount > 0 ? BuildNext(false) : Built(); // batch 1's graph: nothing to run beside
        prof.End(HostProfile::EXCLUDE_GRAPH_UPDATE);
        if (gStreamBatchCount == 0) nxt.end = true;
        while (stream_batch_count++ < gStreamBatchCount) {
            if (!quiet_ && (gStreamUpdateCountPerBatch > 100 || stream_batch_count % 100 == 0))
                Report(stream_batch_count);
            progress++;
            if (nxt.end) break;
            if (nxt.deferred) { // the host arrays hold this batch; the solver is idle now
                prof.Start(HostProfile::EXCLUDE_GRAPH_UPDATE);
                DPPR_CHECK(engine, dppr_set_batch(engine, graph->edge_batch->edge1, graph->edge_batch->edge2, graph->edge_batch->is_insert,
                                                  graph->edge_batch->length));
                DPPR_CHECK(engine, dppr_slide(engine, graph->new_stream->edge1, graph->new_stream->edge2, graph->new_stream->length, &nxt.epoch));
                prof.End(HostProfile::EXCLUDE_GRAPH_UPDATE);
                progress++;
            }
            const int32_t epoch = nxt.epoch;
            const bool more = stream_batch_count < gStreamBatchCount;
            std::future<Built> task;
            if (more) task = std::async(std::launch::async, [this] { return BuildNext(true); });
            prof.Start(HostProfile::PPR);
            for (size_t k = 0; k < groups.size(); ++k) {
                float ms = 0;
                DPPR_CHECK(engine, dppr_group_update(engine, groups[k], epoch, gTolerance, &ms));
                ppr_time[k] += ms;
            }
            for (size_t i = 0; i < slots.size(); ++i) {
                float ms = 0;
                DPPR_CHECK(engine, dppr_update(engine, slots[i], epoch, gTolerance, &ms));
                ppr_time[i] += ms;
            }
            prof.End(HostProfile::PPR);
            if (more) {
                prof.Start(HostProfile::EXCLUDE_GRAPH_UPDATE); // (what is left of the build once the solve is over)
                nxt = task.get();
                prof.End(HostProfile::EXCLUDE_GRAPH_UPDATE);
                build_beside_ms += nxt.ms;
            }
            if (gChangesK > 0) PrintChanges(stream_batch_count);
            if (gPatchGiven) PrintPatch(stream_batch_count);
            if (gAssign) PrintAssign(stream_batch_count);
            if (!gRefineIds.empty()) PrintRefined(epoch); // (the epoch the states stand on: the helper may have built the next one)
            if (!gPositionIds.empty()) PrintPositions(epoch);
            if (gSample > 0) PrintSamples(epoch);
            if (!gForwardIds.empty()) PrintForward(epoch);
            if (!gPushSets.empty()) PrintForwardPush(epoch);
            if (!gTrackSets.empty()) PrintForwardTrack(epoch, false);
            if (!gExplainIds.empty()) PrintExplained(epoch);
            if (gCertify > 0 && stream_batch_count % (size_t)gCertify == 0) PrintCertify(epoch); // (the explicit epoch: the helper may have built the next one)
            if (gClusterK > 0) PrintClusters(epoch);
            if (gSubgraphK > 0) PrintSubgraphs(epoch);
        }
        batches_done = stream_batch_count - 1;
        if (!quiet_) Report(stream_batch_count);
        if (!quiet_) {
            int32_t ids = 0, parked = 0, renumberings = 0;
            int64_t revivals = 0;
            DPPR_CHECK(engine, dppr_id_space(engine, &ids, &parked, &renumberings, &revivals));
            std::cout << "id_space ids=" << ids << " parked=" << parked << " renumberings=" << renumberings
                      << " revivals=" << revivals << std::endl;
        }
    }

    // the reference's four virtuals (gpu/PPRGPU.cuh:179-182), per source slot
    virtual void GPUBuildSlidingGraph() {
        DPPR_CHECK(engine, dppr_slide(engine, graph->new_stream->edge1, graph->new_stream->edge2,
                                      graph->new_stream->length, nullptr));
    }
    virtual void IncrementalBatchUpdate(size_t i) { DPPR_CHECK(engine, dppr_incremental_batch_update(engine, slots[i], -1)); }
    virtual void ExecuteMainLoop(size_t i, size_t phase_id) {
        DPPR_CHECK(engine, dppr_execute_main_loop(engine, slots[i], -1, (int)phase_id, gTolerance));
    }

    // gpu/PPRRevPushGPU.cuh:134-164: residual bound, then |p - p_pow| < 100 eps with the
    // power iteration of cpu/PPRCPUPowVec.h:55-83 on the current window graph.
    void ReadSource(size_t i, double *p, double *r) {
        if (use_groups) DPPR_CHECK(engine, dppr_group_read(engine, groups[i / kGroupMax], (int32_t)(i % kGroupMax), p, r));
        else DPPR_CHECK(engine, dppr_read(engine, slots[i], p, r));
    }

    virtual void ValidateResult(size_t i) {
        const IndexType V = graph->vertex_count, s = source_vertex_ids[i];
        std::vector<double> p((size_t)V), r((size_t)V);
        ReadSource(i, p.data(), r.data());
        for (IndexType u = 0; u < V; ++u) {
            if (!(r[u] < gTolerance && r[u] > -gTolerance)) {
                std::cout << "VALIDATE FAILED: residual[" << u << "]=" << r[u] << std::endl;
                std::exit(-1);
            }
        }
        std::vector<IndexType> row, col;
        graph->ConstructGraph(row, col);
        if (!target_lanes.empty()) {
            // a lane of --target-sets: the residual bound above, then the invariant with the lane's seed vector h,
            //   p[u] + ALPHA r[u] == ALPHA h[u] + (1 - ALPHA) / (outdeg(u) + 1) * sum over v in out(u) of p[v],
            // to rounding (1e-13 for sum(h) <= 1, as the tests hold it; p scales with sum(h)). |p - exact| < eps follows from
            // the two (include/dppr.h).
            std::vector<double> h((size_t)V, 0.0);
            double total = 0.0;
            for (const auto &sd : gTargetSets[target_lanes[i]]) {
                h[(size_t)sd.first] = sd.second;
                total += sd.second;
            }
            const double bound = 1e-13 * std::max(1.0, total);
            double worst = 0.0;
            for (IndexType u = 0; u < V; ++u) {
                double acc = 0.0;
                for (IndexType j = row[u]; j < row[u + 1]; ++j) acc += p[col[j]];
                const double rhs = ALPHA * h[u] + (1.0 - ALPHA) / (double)(row[u + 1] - row[u] + 1) * acc;
                const double err = std::fabs(p[u] + ALPHA * r[u] - rhs);
                worst = std::max(worst, err);
                if (!(err < bound)) {
                    std::cout << "VALIDATE FAILED: invariant " << err << "," << bound << " at vertex " << u << std::endl;
                    std::exit(-1);
                }
            }
            if (!quiet_) std::cout << "validate ok (set lane of " << gTargetSets[target_lanes[i]].size() << " seeds: residual bound + invariant with h, max error=" << worst << ")" << std::endl;
            return;
        }
        std::vector<double> a((size_t)V), b((size_t)V);
        for (IndexType u = 0; u < V; ++u) a[u] = (u == s) ? 1 : 0;
        size_t iters = 0;
        for (;;) { // Jacobi sweep until no component moves by more than 1e-14
            bool stop = true;
            for (IndexType u = 0; u < V; ++u) {
                double acc = 0.0;
                const size_t d = (size_t)(row[u + 1] - row[u]);
                for (IndexType j = row[u]; j < row[u + 1]; ++j) acc += a[col[j]] / (d + 1);
                acc = (1.0 - ALPHA) * acc;
                if (u == s) acc += ALPHA * 1.0;
                b[u] = acc;
                if (std::fabs(acc - a[u]) > 1e-14) stop = false;
            }
            if (stop) break;
            a.swap(b);
            ++iters;
        }
        const double bound = gTolerance * 100;
        for (IndexType u = 0; u < V; ++u) {
            const double err = std::fabs(a[u] - p[u]);
            if (!(err < bound)) {
                std::cout << "VALIDATE FAILED: " << err << "," << bound << " at vertex " << u << std::endl;
                std::exit(-1);
            }
        }
        if (!quiet_) std::cout << "validate ok (power iterations=" << iters << ")" << std::endl;
    }

    void Dump(const std::string &path) {
        FILE *f = std::fopen(path.c_str(), "wb");
        if (!f) return;
        const IndexType V = graph->vertex_count;
        std::vector<double> p((size_t)V), r((size_t)V);
        for (size_t i = 0; i < source_vertex_ids.size(); ++i) {
            ReadSource(i, p.data(), r.data());
            std::fwrite(&source_vertex_ids[i], sizeof(IndexType), 1, f);
            std::fwrite(&V, sizeof(IndexType), 1, f);
            std::fwrite(p.data(), sizeof(double), (size_t)V, f);
            std::fwrite(r.data(), sizeof(double), (size_t)V, f);
        }
        std::fclose(f);
    }

    // --topk: the k vertices of largest p of every source of this device, in this device's source order, through the device-side
    // selection (dppr_topk / dppr_group_topk: one call per slot or per group of up to 16)
    struct TopEntry {
        int32_t vertex;
        double p;
    };
    std::vector<std::vector<TopEntry>> TopK(int k) {
        const size_t n_src = source_vertex_ids.size();
        std::vector<std::vector<TopEntry>> out(n_src);
        std::vector<int32_t> ids, cnt;
        std::vector<double> p;
        for (size_t first = 0; first < n_src; first += use_groups ? kGroupMax : 1) {
            const size_t n = use_groups ? std::min(kGroupMax, n_src - first) : 1;
            ids.assign(n * (size_t)k, -1);
            p.assign(n * (size_t)k, 0.0);
            cnt.assign(n, 0);
            if (use_groups)
                DPPR_CHECK(engine, dppr_group_topk(engine, groups[first / kGroupMax], k, 0.0, ids.data(), p.data(), nullptr, cnt.data()));
            else
                DPPR_CHECK(engine, dppr_topk(engine, slots[first], k, 0.0, ids.data(), p.data(), nullptr, cnt.data()));
            for (size_t j = 0; j < n; ++j)
                for (int32_t t = 0; t < cnt[j]; ++t) out[first + j].push_back({ids[j * (size_t)k + t], p[j * (size_t)k + t]});
        }
        return out;
    }

    // --rank-factor / --rank-exclude: the same lists by the ranked query on the newest epoch (dppr_topk_ranked /
    // dppr_group_topk_ranked; TopEntry::p holds the score). No mask: the program owns no device memory.
    std::vector<std::vector<TopEntry>> TopKRanked(int k, int factor, unsigned exclude) {
        const size_t n_src = source_vertex_ids.size();
        std::vector<std::vector<TopEntry>> out(n_src);
        std::vector<int32_t> ids, cnt;
        std::vector<double> score;
        dppr_rank_spec_t spec{};
        spec.factor = factor;
        spec.exclude = exclude;
        for (size_t first = 0; first < n_src; first += use_groups ? kGroupMax : 1) {
            const size_t n = use_groups ? std::min(kGroupMax, n_src - first) : 1;
            ids.assign(n * (size_t)k, -1);
            score.assign(n * (size_t)k, 0.0);
            cnt.assign(n, 0);
            if (use_groups)
                DPPR_CHECK(engine, dppr_group_topk_ranked(engine, groups[first / kGroupMax], -1, &spec, k, 0.0, ids.data(), score.data(), cnt.data()));
            else
                DPPR_CHECK(engine, dppr_topk_ranked(engine, slots[first], -1, &spec, k, 0.0, ids.data(), score.data(), cnt.data()));
            for (size_t j = 0; j < n; ++j)
                for (int32_t t = 0; t < cnt[j]; ++t) out[first + j].push_back({ids[j * (size_t)k + t], score[j * (size_t)k + t]});
        }
        return out;
    }

    // --sparse-min: every vertex with p > min_p of every source of this device, in this device's source order and by id, through
    // the device-side compaction (dppr_export_sparse / dppr_group_export_sparse: the size call, then the fill)
    struct SparseVec {
        std::vector<int32_t> ids;
        std::vector<double> p;
    };
    std::vector<SparseVec> SparseExport(double min_p) {
        const size_t n_src = source_vertex_ids.size();
        std::vector<SparseVec> out(n_src);
        std::vector<int32_t> ids;
        std::vector<double> p;
        for (size_t first = 0; first < n_src; first += use_groups ? kGroupMax : 1) {
            const size_t n = use_groups ? std::min(kGroupMax, n_src - first) : 1;
            std::vector<int64_t> off(n + 1, 0);
            auto call = [&](int64_t cap) {
                if (use_groups)
                    DPPR_CHECK(engine, dppr_group_export_sparse(engine, groups[first / kGroupMax], min_p, cap, DPPR_DEST_HOST, off.data(), ids.data(), p.data(), nullptr));
                else
                    DPPR_CHECK(engine, dppr_export_sparse(engine, slots[first], min_p, cap, DPPR_DEST_HOST, off.data(), ids.data(), p.data(), nullptr));
            };
            call(0);
            ids.assign((size_t)off[n] + 1, -1);
            p.assign((size_t)off[n] + 1, 0.0);
            if (off[n] > 0) call(off[n]);
            for (size_t j = 0; j < n; ++j) {
                out[first + j].ids.assign(ids.begin() + off[j], ids.begin() + off[j + 1]);
                out[first + j].p.assign(p.begin() + off[j], p.begin() + off[j + 1]);
            }
        }
        return out;
    }

    // --seeds: the score of every source of this device under every seed set (one CSR over the lines, host memory), through the
    // device-side fold (dppr_dot_sparse / dppr_group_dot_sparse), DPPR_DOT_MAX_F lines a call: [source of this device][line]
    std::vector<std::vector<double>> SeedScores(const std::vector<int64_t> &off, const std::vector<int32_t> &ids, const std::vector<double> &w) {
        const size_t n_src = source_vertex_ids.size(), lines = off.size() - 1;
        std::vector<std::vector<double>> out(n_src, std::vector<double>(lines, 0.0));
        const int32_t none_id = 0;
        const double none_w = 0.0;
        std::vector<int64_t> rel;
        std::vector<double> res;
        for (size_t first = 0; first < n_src; first += use_groups ? kGroupMax : 1) {
            const size_t n = use_groups ? std::min(kGroupMax, n_src - first) : 1;
            for (size_t l0 = 0; l0 < lines; l0 += DPPR_DOT_MAX_F) {
                const size_t F = std::min<size_t>(DPPR_DOT_MAX_F, lines - l0);
                rel.resize(F + 1);
                for (size_t f = 0; f <= F; ++f) rel[f] = off[l0 + f] - off[l0];
                const int32_t *pi = ids.empty() ? &none_id : ids.data() + off[l0]; // (a file of blank lines: no entry, and no NULL)
                const double *pw = w.empty() ? &none_w : w.data() + off[l0];
                res.assign(F * n, 0.0);
                if (use_groups)
                    DPPR_CHECK(engine, dppr_group_dot_sparse(engine, groups[first / kGroupMax], DPPR_DENSE_P, rel.data(), pi, pw, DPPR_DEST_HOST, (int32_t)F, DPPR_DEST_HOST, res.data()));
                else
                    DPPR_CHECK(engine, dppr_dot_sparse(engine, slots[first], DPPR_DENSE_P, rel.data(), pi, pw, DPPR_DEST_HOST, (int32_t)F, DPPR_DEST_HOST, res.data()));
                for (size_t f = 0; f < F; ++f)
                    for (size_t j = 0; j < n; ++j) out[first + j][l0 + f] = res[f * n + j];
            }
        }
        return out;
    }

    // --changes: what batch `batch` (from 1) moved, per source of this device in this device's source order, and the new mark in the
    // same pass (dppr_changes / dppr_group_changes with remark = 1). Outside the timed region: ppr_time is the hipEvent time the
    // update calls return. One device's lines of a batch are printed as one block (-g N: the device threads take turns).
    void PrintChanges(size_t batch) {
        const int k = gChangesK;
        const size_t n_src = source_vertex_ids.size();
        std::vector<int32_t> ids, cnt, moved;
        std::vector<double> d, p;
        std::string out;
        char line[200];
        for (size_t first = 0; first < n_src; first += use_groups ? kGroupMax : 1) {
            const size_t n = use_groups ? std::min(kGroupMax, n_src - first) : 1;
            ids.assign(n * (size_t)k, -1);
            d.assign(n * (size_t)k, 0.0);
            p.assign(n * (size_t)k, 0.0);
            cnt.assign(n, 0);
            moved.assign(n, 0);
            if (use_groups)
                DPPR_CHECK(engine, dppr_group_changes(engine, groups[first / kGroupMax], k, gChangesMin, 1, ids.data(), d.data(), p.data(), cnt.data(), moved.data()));
            else
                DPPR_CHECK(engine, dppr_changes(engine, slots[first], k, gChangesMin, 1, ids.data(), d.data(), p.data(), cnt.data(), moved.data()));
            for (size_t j = 0; j < n; ++j) {
                std::snprintf(line, sizeof(line), "moved %zu %d %d\n", batch, (int)source_vertex_ids[first + j], (int)moved[j]);
                out += line;
                for (int32_t t = 0; t < cnt[j]; ++t) {
                    const size_t at = j * (size_t)k + (size_t)t;
                    std::snprintf(line, sizeof(line), "changes %zu %d %d %d %.17g %.17g\n", batch, (int)source_vertex_ids[first + j], (int)t + 1, (int)ids[at], d[at], p[at]);
                    out += line;
                }
            }
        }
        progress++;
        static std::mutex print_mu;
        std::lock_guard<std::mutex> lk(print_mu);
        std::cout << out << std::flush;
    }

    // --patch-min: the patch of batch `batch` (from 1) that brings a replica of {p > gPatchMin} up to date, per source of this device in
    // this device's source order (dppr_patch / dppr_group_patch: the size call, which leaves the mark alone, then the fill with
    // DPPR_PATCH_REMARK_EMITTED, so that the mark is what the replica holds). Outside the timed region, printed as one block like
    // --changes; the entries are appended to --patch-out under the same lock.
    void PrintPatch(size_t batch) {
        const size_t n_src = source_vertex_ids.size();
        std::vector<int32_t> up_ids, del_ids;
        std::vector<double> up_p;
        std::string out, file;
        char line[200];
        for (size_t first = 0; first < n_src; first += use_groups ? kGroupMax : 1) {
            const size_t n = use_groups ? std::min(kGroupMax, n_src - first) : 1;
            std::vector<int64_t> uo(n + 1, 0), dl(n + 1, 0);
            dppr_patch_out_t po{uo.data(), nullptr, nullptr, dl.data(), nullptr, 0};
            auto call = [&](int64_t cap_up, int64_t cap_del, int remark) {
                if (use_groups)
                    DPPR_CHECK(engine, dppr_group_patch(engine, groups[first / kGroupMax], gPatchMin, gPatchDelta, cap_up, cap_del, DPPR_DEST_HOST, remark, &po));
                else
                    DPPR_CHECK(engine, dppr_patch(engine, slots[first], gPatchMin, gPatchDelta, cap_up, cap_del, DPPR_DEST_HOST, remark, &po));
            };
            call(0, 0, DPPR_PATCH_KEEP_MARK);
            up_ids.assign((size_t)uo[n] + 1, -1);
            up_p.assign((size_t)uo[n] + 1, 0.0);
            del_ids.assign((size_t)dl[n] + 1, -1);
            po.up_ids = up_ids.data();
            po.up_p = up_p.data();
            po.del_ids = del_ids.data();
            call(uo[n], dl[n], DPPR_PATCH_REMARK_EMITTED);
            if (po.written != 1) {
                std::cout << "patch: the state changed between the size call and the fill" << std::endl;
                std::exit(-1);
            }
            for (size_t j = 0; j < n; ++j) {
                const int src = (int)source_vertex_ids[first + j];
                std::snprintf(line, sizeof(line), "patch %d upserts %lld deletes %lld\n", src, (long long)(uo[j + 1] - uo[j]), (long long)(dl[j + 1] - dl[j]));
                out += line;
                if (gPatchOut.empty()) continue;
                for (int64_t t = uo[j]; t < uo[j + 1]; ++t) {
                    std::snprintf(line, sizeof(line), "U %zu %d %d %.17g\n", batch, src, (int)up_ids[(size_t)t], up_p[(size_t)t]);
                    file += line;
                }
                for (int64_t t = dl[j]; t < dl[j + 1]; ++t) {
                    std::snprintf(line, sizeof(line), "D %zu %d %d\n", batch, src, (int)del_ids[(size_t)t]);
                    file += line;
                }
            }
        }
        progress++;
        static std::mutex print_mu;
        std::lock_guard<std::mutex> lk(print_mu);
        std::cout << out << std::flush;
        if (!gPatchOut.empty()) {
            std::FILE *f = std::fopen(gPatchOut.c_str(), "a");
            if (!f || std::fwrite(file.data(), 1, file.size(), f) != file.size() || std::fclose(f) != 0) {
                std::cout << "cannot write " << gPatchOut << std::endl;
                std::exit(-1);
            }
        }
    }

    // --assign: after a batch, every vertex to the lane that holds it best over ALL groups of this device (dppr_assign, host
    // destination, no scale), the flips counted against the labels of the batch before, which the host keeps and passes back in
    // place (the first batch: against all -1). Outside the timed region, one line per batch.
    void PrintAssign(size_t batch) {
        const size_t V = (size_t)graph->vertex_count, n_classes = source_vertex_ids.size();
        if (assign_label.size() != V) assign_label.assign(V, -1);
        std::vector<int64_t> counts(n_classes + 1, 0);
        int64_t flips = 0;
        DPPR_CHECK(engine, dppr_assign(engine, groups.data(), (int32_t)groups.size(), nullptr, gAssignMin, DPPR_DEST_HOST, assign_label.data(), nullptr,
                                       nullptr, counts.data(), assign_label.data(), 0, &flips, nullptr, nullptr, nullptr));
        std::string out = "assign " + std::to_string(batch) + " classes=" + std::to_string(n_classes) + " unassigned=" + std::to_string(counts[n_classes]) +
                          " flips=" + std::to_string(flips) + " counts=";
        for (size_t c = 0; c < n_classes; ++c) out += (c ? "," : "") + std::to_string(counts[c]);
        progress++;
        std::cout << out << std::endl;
    }
    // --assign-out: the labels of the last batch, raw int32 [V] (all -1 if no batch ran)
    bool WriteAssign(const std::string &path) {
        if (assign_label.size() != (size_t)graph->vertex_count) assign_label.assign((size_t)graph->vertex_count, -1);
        std::FILE *f = std::fopen(path.c_str(), "wb");
        if (!f) return false;
        const bool ok = std::fwrite(assign_label.data(), sizeof(int32_t), assign_label.size(), f) == assign_label.size();
        return std::fclose(f) == 0 && ok;
    }

    // --refine: after a batch, the pagerank of every listed vertex towards every source of this device refined by gWalks forward
    // walks over `epoch` (dppr_refine_at / dppr_group_refine_at: one set of walks serves all sources of a group), with the
    // standard error a caller derives from sumsq. Outside the timed region, printed as one block like --changes.
    void PrintRefined(int32_t epoch) {
        const size_t n_src = source_vertex_ids.size(), m = gRefineIds.size();
        const double W = (double)gWalks;
        std::vector<double> est, corr, sumsq;
        std::string out;
        char line[200];
        for (size_t first = 0; first < n_src; first += use_groups ? kGroupMax : 1) {
            const size_t n = use_groups ? std::min(kGroupMax, n_src - first) : 1;
            est.assign(m * n, 0.0);
            corr.assign(m * n, 0.0);
            sumsq.assign(m * n, 0.0);
            if (use_groups)
                DPPR_CHECK(engine, dppr_group_refine_at(engine, groups[first / kGroupMax], epoch, gRefineIds.data(), (int32_t)m, gWalks, gWalkSeed, est.data(), corr.data(), sumsq.data()));
            else
                DPPR_CHECK(engine, dppr_refine_at(engine, slots[first], epoch, gRefineIds.data(), (int32_t)m, gWalks, gWalkSeed, est.data(), corr.data(), sumsq.data()));
            for (size_t q = 0; q < m; ++q)
                for (size_t j = 0; j < n; ++j) {
                    const size_t at = q * n + j;
                    const double var = std::max(sumsq[at] / W - corr[at] * corr[at], 0.0);
                    const double se = gWalks > 1 ? std::sqrt(var / (W - 1.0)) : std::nan("");
                    std::snprintf(line, sizeof(line), "refined %d %zu %.17g %.17g %.17g\n", (int)gRefineIds[q], first + j, est[at], corr[at], se);
                    out += line;
                }
        }
        progress++;
        static std::mutex print_mu;
        std::lock_guard<std::mutex> lk(print_mu);
        std::cout << out << std::flush;
    }

    // --positions: after a batch, where every listed vertex stands in the order of every source of this device (dppr_position_at /
    // dppr_group_position_at: by pagerank, or by the score of --rank-factor / --rank-exclude over `epoch`), and how many vertices have
    // a position at all. Outside the timed region, printed as one block like --changes.
    void PrintPositions(int32_t epoch) {
        const size_t n_src = source_vertex_ids.size(), m = gPositionIds.size();
        std::vector<int32_t> pos, cnt;
        dppr_rank_spec_t spec{};
        spec.factor = gRankGiven ? gRankFactor : DPPR_FACTOR_NONE;
        spec.exclude = gRankGiven ? (unsigned)gRankExclude : 0u;
        std::string out;
        char line[200];
        for (size_t first = 0; first < n_src; first += use_groups ? kGroupMax : 1) {
            const size_t n = use_groups ? std::min(kGroupMax, n_src - first) : 1;
            pos.assign(m * n, -1);
            cnt.assign(n, 0);
            if (use_groups)
                DPPR_CHECK(engine, dppr_group_position_at(engine, groups[first / kGroupMax], epoch, &spec, 0.0, gPositionIds.data(), (int32_t)m, pos.data(), cnt.data()));
            else
                DPPR_CHECK(engine, dppr_position_at(engine, slots[first], epoch, &spec, 0.0, gPositionIds.data(), (int32_t)m, pos.data(), cnt.data()));
            for (size_t j = 0; j < n; ++j) {
                for (size_t q = 0; q < m; ++q) {
                    std::snprintf(line, sizeof(line), "position %d %d %d\n", (int)source_vertex_ids[first + j], (int)gPositionIds[q], (int)pos[q * n + j]);
                    out += line;
                }
                std::snprintf(line, sizeof(line), "positions %d qualifying %d\n", (int)source_vertex_ids[first + j], (int)cnt[j]);
                out += line;
            }
        }
        progress++;
        static std::mutex print_mu;
        std::lock_guard<std::mutex> lk(print_mu);
        std::cout << out << std::flush;
    }

    // --explain: after a batch, per source of this device and per listed vertex, the path of largest contributions towards the source
    // and the out-neighbours that contribute most (dppr_explain_at / dppr_group_explain_at over `epoch`). Outside the timed region,
    // printed as one block like --changes.
    void PrintExplained(int32_t epoch) {
        const size_t n_src = source_vertex_ids.size(), m = gExplainIds.size();
        const size_t f = (size_t)gExplainTop, dp = (size_t)gExplainDepth + 1;
        std::vector<int32_t> cnt, nbr, mult, len, end, path;
        std::vector<double> c;
        std::string out;
        char line[200];
        for (size_t first = 0; first < n_src; first += use_groups ? kGroupMax : 1) {
            const size_t n = use_groups ? std::min(kGroupMax, n_src - first) : 1;
            cnt.assign(m * n, 0), len.assign(m * n, 0), end.assign(m * n, 0);
            nbr.assign(m * n * f + 1, -1), mult.assign(m * n * f + 1, 0), c.assign(m * n * f + 1, 0.0), path.assign(m * n * dp, -1);
            dppr_explain_out_t o{};
            o.nbr_count = cnt.data(), o.nbr = nbr.data(), o.nbr_mult = mult.data(), o.nbr_c = c.data();
            o.len = len.data(), o.end = end.data(), o.path = path.data();
            if (use_groups)
                DPPR_CHECK(engine, dppr_group_explain_at(engine, groups[first / kGroupMax], epoch, gExplainIds.data(), (int32_t)m, gExplainTop, gExplainDepth, &o));
            else
                DPPR_CHECK(engine, dppr_explain_at(engine, slots[first], epoch, gExplainIds.data(), (int32_t)m, gExplainTop, gExplainDepth, &o));
            for (size_t j = 0; j < n; ++j)
                for (size_t q = 0; q < m; ++q) {
                    const size_t at = q * n + j;
                    const int src = (int)source_vertex_ids[first + j], v = (int)gExplainIds[q];
                    std::snprintf(line, sizeof(line), "explain %d %d %d %d", src, v, (int)end[at], (int)len[at]);
                    out += line;
                    for (int t = 0; t < len[at]; ++t) {
                        std::snprintf(line, sizeof(line), " %d", (int)path[at * dp + (size_t)t]);
                        out += line;
                    }
                    out += "\n";
                    for (int k = 0; k < cnt[at]; ++k) {
                        std::snprintf(line, sizeof(line), "because %d %d %d %d %.17g\n", src, v, (int)nbr[at * f + (size_t)k], (int)mult[at * f + (size_t)k], c[at * f + (size_t)k]);
                        out += line;
                    }
                }
        }
        progress++;
        static std::mutex print_mu;
        std::lock_guard<std::mutex> lk(print_mu);
        std::cout << out << std::flush;
    }

    // --certify: the certificate of every source's state over `epoch` (dppr_certify / dppr_group_certify, both parts): one line per
    // source in source order; legal > 0, nonfinite > 0 or inv >= 1e-13 * max(1, sum of the lane's seed weights) -- the bound
    // ValidateResult holds set lanes to -- ends the program. Outside the timed region, printed as one block like --changes.
    void PrintCertify(int32_t epoch) {
        const size_t n_src = source_vertex_ids.size();
        std::string out, failed;
        char line[400];
        for (size_t first = 0; first < n_src; first += use_groups ? kGroupMax : 1) {
            const size_t n = use_groups ? std::min(kGroupMax, n_src - first) : 1;
            std::vector<double> max_r(n), sum_r(n), inv(n);
            std::vector<int32_t> at(n), inv_at(n);
            std::vector<int64_t> pos(n), neg(n), nonfinite(n);
            dppr_certify_out_t o{};
            o.max_abs_r = max_r.data(), o.argmax_r = at.data(), o.sum_abs_r = sum_r.data();
            o.n_pos = pos.data(), o.n_neg = neg.data(), o.n_nonfinite = nonfinite.data();
            o.inv_max_err = inv.data(), o.inv_argmax = inv_at.data();
            const int flags = DPPR_CERT_RESIDUAL | DPPR_CERT_INVARIANT;
            if (use_groups) DPPR_CHECK(engine, dppr_group_certify(engine, groups[first / kGroupMax], epoch, gTolerance, flags, &o));
            else DPPR_CHECK(engine, dppr_certify(engine, slots[first], epoch, gTolerance, flags, &o));
            for (size_t j = 0; j < n; ++j) {
                double total = 1.0; // (sum of h: a source lane's indicator)
                if (!target_lanes.empty()) {
                    total = 0.0;
                    for (const auto &sd : gTargetSets[target_lanes[first + j]]) total += sd.second;
                }
                const double bound = 1e-13 * std::max(1.0, total);
                const long long legal = (long long)(pos[j] + neg[j]);
                std::snprintf(line, sizeof(line), "certify %d epoch=%d max_r=%.17g at=%d sum_r=%.17g legal=%lld nonfinite=%lld inv=%.17g inv_at=%d\n",
                              (int)source_vertex_ids[first + j], (int)o.state_epoch, max_r[j], (int)at[j], sum_r[j], legal, (long long)nonfinite[j],
                              inv[j], (int)inv_at[j]);
                out += line;
                if (failed.empty() && (legal > 0 || nonfinite[j] > 0 || !(inv[j] < bound))) {
                    std::snprintf(line, sizeof(line), "CERTIFY FAILED: source %d legal=%lld nonfinite=%lld inv=%.17g bound=%.17g\n",
                                  (int)source_vertex_ids[first + j], legal, (long long)nonfinite[j], inv[j], bound);
                    failed = line;
                }
            }
        }
        progress++;
        static std::mutex print_mu;
        std::lock_guard<std::mutex> lk(print_mu);
        std::cout << out << failed << std::flush;
        if (!failed.empty()) std::exit(-1);
    }

    // --sample: after a batch, gSample vertices drawn in proportion to the score of every source of this device (dppr_sample /
    // dppr_group_sample: by pagerank, or by the score of --rank-factor / --rank-exclude over `epoch`). Outside the timed region,
    // printed as one block like --changes.
    void PrintSamples(int32_t epoch) {
        const size_t n_src = source_vertex_ids.size(), S = (size_t)gSample;
        std::vector<int32_t> ids, support, status, seen;
        std::vector<double> total;
        dppr_rank_spec_t spec{};
        spec.factor = gRankGiven ? gRankFactor : DPPR_FACTOR_NONE;
        spec.exclude = gRankGiven ? (unsigned)gRankExclude : 0u;
        std::string out;
        char line[200];
        for (size_t first = 0; first < n_src; first += use_groups ? kGroupMax : 1) {
            const size_t n = use_groups ? std::min(kGroupMax, n_src - first) : 1;
            ids.assign(n * S, -1);
            total.assign(n, 0.0);
            support.assign(n, 0);
            status.assign(n, 0);
            if (use_groups)
                DPPR_CHECK(engine, dppr_group_sample(engine, groups[first / kGroupMax], epoch, &spec, 0.0, gSampleSeed, 0, (int32_t)S, DPPR_DEST_HOST, ids.data(),
                                                     nullptr, total.data(), support.data(), status.data()));
            else
                DPPR_CHECK(engine, dppr_sample(engine, slots[first], epoch, &spec, 0.0, gSampleSeed, 0, (int32_t)S, DPPR_DEST_HOST, ids.data(), nullptr,
                                               total.data(), support.data(), status.data()));
            for (size_t j = 0; j < n; ++j) {
                seen.assign(ids.begin() + (long)(j * S), ids.begin() + (long)((j + 1) * S));
                std::sort(seen.begin(), seen.end());
                size_t distinct = 0;
                for (size_t q = 0; q < S; ++q) distinct += seen[q] >= 0 && (q == 0 || seen[q] != seen[q - 1]) ? 1 : 0;
                std::snprintf(line, sizeof(line), "sample %d lane %d total %.17g support %d status %d distinct %zu ids", (int)source_vertex_ids[first + j], (int)j,
                              total[j], (int)support[j], (int)status[j], distinct);
                out += line;
                for (size_t q = 0; q < std::min<size_t>(S, 8); ++q) {
                    std::snprintf(line, sizeof(line), " %d", (int)ids[j * S + q]);
                    out += line;
                }
                out += "\n";
            }
        }
        progress++;
        static std::mutex print_mu;
        std::lock_guard<std::mutex> lk(print_mu);
        std::cout << out << std::flush;
    }

    // --forward: after a batch, the forward sweep from every id of the file over `epoch` (dppr_forward: any vertex, tracked or not), in
    // calls of at most 16 starts. Outside the timed region, printed as one block like --changes.
    void PrintForward(int32_t epoch) {
        const size_t n_ids = gForwardIds.size(), K = (size_t)gForwardTopK;
        std::vector<int32_t> used(DPPR_FORWARD_MAX_M), ids(DPPR_FORWARD_MAX_M * std::max<size_t>(K, 1)), counts(DPPR_FORWARD_MAX_M);
        std::vector<double> rem(DPPR_FORWARD_MAX_M), f(DPPR_FORWARD_MAX_M * std::max<size_t>(K, 1));
        std::string out;
        char line[200];
        for (size_t first = 0; first < n_ids; first += DPPR_FORWARD_MAX_M) {
            const size_t m = std::min<size_t>(DPPR_FORWARD_MAX_M, n_ids - first);
            dppr_forward_out_t o{};
            o.iters_used = used.data();
            o.rem = rem.data();
            std::fill(counts.begin(), counts.end(), 0);
            if (K > 0) {
                o.k = (int32_t)K;
                o.min_f = 0.0;
                o.topk_ids = ids.data();
                o.topk_f = f.data();
                o.topk_counts = counts.data();
            }
            DPPR_CHECK(engine, dppr_forward(engine, epoch, gForwardIds.data() + first, (int32_t)m, gForwardIters, gForwardTol, &o));
            for (size_t j = 0; j < m; ++j) {
                std::snprintf(line, sizeof(line), "forward %d iters %d rem %.17g top %d", (int)gForwardIds[first + j], (int)used[j], rem[j], (int)counts[j]);
                out += line;
                for (size_t q = 0; q < (size_t)counts[j]; ++q) {
                    std::snprintf(line, sizeof(line), " %d:%.17g", (int)ids[j * K + q], f[j * K + q]);
                    out += line;
                }
                out += "\n";
            }
        }
        progress++;
        static std::mutex print_mu;
        std::lock_guard<std::mutex> lk(print_mu);
        std::cout << out << std::flush;
    }

    // --forward-push: after a batch, the forward push from every set of the file over `epoch` (dppr_forward_push), in calls of at most
    // 16 sets. Outside the timed region, printed as one block like --changes.
    void PrintForwardPush(int32_t epoch) {
        const size_t n_sets = gPushSets.size(), K = (size_t)gForwardTopK;
        std::vector<int32_t> used(DPPR_FORWARD_MAX_M), conv(DPPR_FORWARD_MAX_M), ids(DPPR_FORWARD_MAX_M * std::max<size_t>(K, 1)), counts(DPPR_FORWARD_MAX_M);
        std::vector<int64_t> pushes(DPPR_FORWARD_MAX_M), left(DPPR_FORWARD_MAX_M);
        std::vector<double> rem(DPPR_FORWARD_MAX_M), p(DPPR_FORWARD_MAX_M * std::max<size_t>(K, 1));
        std::string out;
        char line[240];
        for (size_t first = 0; first < n_sets; first += DPPR_FORWARD_MAX_M) {
            const size_t m = std::min<size_t>(DPPR_FORWARD_MAX_M, n_sets - first);
            std::vector<int64_t> off(1, 0);
            std::vector<int32_t> sid;
            std::vector<double> sw;
            for (size_t j = 0; j < m; ++j) {
                for (const auto &s : gPushSets[first + j]) {
                    sid.push_back(s.first);
                    sw.push_back(s.second);
                }
                off.push_back((int64_t)sid.size());
            }
            dppr_forward_push_out_t o{};
            o.rounds_used = used.data();
            o.converged = conv.data();
            o.rem = rem.data();
            o.pushes = pushes.data();
            o.left = left.data();
            std::fill(counts.begin(), counts.end(), 0);
            if (K > 0) {
                o.k = (int32_t)K;
                o.min_p = 0.0;
                o.topk_ids = ids.data();
                o.topk_p = p.data();
                o.topk_counts = counts.data();
            }
            DPPR_CHECK(engine, dppr_forward_push(engine, epoch, off.data(), sid.data(), sw.data(), (int32_t)m, gPushEps, gPushRounds, &o));
            for (size_t j = 0; j < m; ++j) {
                std::snprintf(line, sizeof(line), "fpush %d seeds %d rounds %d converged %d rem %.17g pushes %lld left %lld top %d",
                              (int)gPushSets[first + j][0].first, (int)gPushSets[first + j].size(), (int)used[j], (int)conv[j], rem[j], (long long)pushes[j],
                              (long long)left[j], (int)counts[j]);
                out += line;
                for (size_t q = 0; q < (size_t)counts[j]; ++q) {
                    std::snprintf(line, sizeof(line), " %d:%.17g", (int)ids[j * K + q], p[j * K + q]);
                    out += line;
                }
                out += "\n";
            }
        }
        progress++;
        static std::mutex print_mu;
        std::lock_guard<std::mutex> lk(print_mu);
        std::cout << out << std::flush;
    }

    // --forward-track: a forward track per 16 sets of the file (dppr_ftrack_*). create: on the loaded window, after the initial solve;
    // else the tracks move to `epoch`, the batch's graph, by the fix-up and the signed rounds. Outside the timed region, printed as one
    // block like --changes.
    std::vector<int32_t> ftracks;
    void PrintForwardTrack(int32_t epoch, bool create) {
        const size_t n_sets = gTrackSets.size(), K = (size_t)gForwardTopK;
        std::vector<int32_t> used(DPPR_FORWARD_MAX_M), conv(DPPR_FORWARD_MAX_M), ids(DPPR_FORWARD_MAX_M * std::max<size_t>(K, 1)), counts(DPPR_FORWARD_MAX_M);
        std::vector<int64_t> pushes(DPPR_FORWARD_MAX_M), fix(3);
        std::vector<double> rem(DPPR_FORWARD_MAX_M), p(DPPR_FORWARD_MAX_M * std::max<size_t>(K, 1));
        std::string out;
        char line[280];
        for (size_t first = 0, t = 0; first < n_sets; first += DPPR_FORWARD_MAX_M, ++t) {
            const size_t m = std::min<size_t>(DPPR_FORWARD_MAX_M, n_sets - first);
            dppr_ftrack_out_t o{};
            o.rounds_used = used.data();
            o.converged = conv.data();
            o.rem = rem.data();
            o.pushes = pushes.data();
            o.fix = fix.data();
            std::fill(counts.begin(), counts.end(), 0);
            if (K > 0) {
                o.k = (int32_t)K;
                o.min_p = 0.0;
                o.topk_ids = ids.data();
                o.topk_p = p.data();
                o.topk_counts = counts.data();
            }
            if (create) {
                std::vector<int64_t> off(1, 0);
                std::vector<int32_t> sid;
                std::vector<double> sw;
                for (size_t j = 0; j < m; ++j) {
                    for (const auto &s : gTrackSets[first + j]) {
                        sid.push_back(s.first);
                        sw.push_back(s.second);
                    }
                    off.push_back((int64_t)sid.size());
                }
                int32_t handle = -1;
                DPPR_CHECK(engine, dppr_ftrack_create(engine, epoch, off.data(), sid.data(), sw.data(), (int32_t)m, gPushEps, gPushRounds, &o, &handle));
                ftracks.push_back(handle);
            } else {
                DPPR_CHECK(engine, dppr_ftrack_update(engine, ftracks[t], epoch, gPushRounds, &o));
            }
            int32_t at = -1;
            DPPR_CHECK(engine, dppr_ftrack_info(engine, ftracks[t], &at, nullptr, nullptr, nullptr, nullptr, nullptr, 0));
            for (size_t j = 0; j < m; ++j) {
                std::snprintf(line, sizeof(line), "ftrack %d seeds %d epoch %d rounds %d converged %d rem %.17g pushes %lld fix %lld %lld %lld top %d",
                              (int)gTrackSets[first + j][0].first, (int)gTrackSets[first + j].size(), (int)at, (int)used[j], (int)conv[j], rem[j],
                              (long long)pushes[j], (long long)fix[0], (long long)fix[1], (long long)fix[2], (int)counts[j]);
                out += line;
                for (size_t q = 0; q < (size_t)counts[j]; ++q) {
                    std::snprintf(line, sizeof(line), " %d:%.17g", (int)ids[j * K + q], p[j * K + q]);
                    out += line;
                }
                out += "\n";
            }
        }
        // --forward-cluster: the full-length sweep of every set's p on the epoch the tracks stand on now (the records alone)
        if (!gTrackCluster.empty()) {
            const int32_t order = gTrackCluster == "p" ? DPPR_FCLUSTER_BY_P : DPPR_FCLUSTER_BY_P_OVER_DEG;
            for (size_t first = 0, t = 0; first < n_sets; first += DPPR_FORWARD_MAX_M, ++t) {
                const size_t m = std::min<size_t>(DPPR_FORWARD_MAX_M, n_sets - first);
                dppr_fcluster_t best[DPPR_FORWARD_MAX_M];
                int64_t offsets[DPPR_FORWARD_MAX_M + 1];
                DPPR_CHECK(engine, dppr_ftrack_cluster(engine, ftracks[t], order, 0.0, 0, 1, 0, DPPR_DEST_HOST, best, offsets, nullptr, nullptr, nullptr,
                                                       nullptr, nullptr));
                for (size_t j = 0; j < m; ++j) {
                    std::snprintf(line, sizeof(line), "fcluster %d size %lld of %lld cut %lld vol %lld phi %.17g\n", (int)gTrackSets[first + j][0].first,
                                  (long long)best[j].best_size, (long long)best[j].count, (long long)best[j].best_cut, (long long)best[j].best_vol,
                                  best[j].best_phi);
                    out += line;
                }
            }
        }
        // --forward-rank: the K best of every set by the ranked query over the track's own p, on the epoch the tracks stand on now
        // (under --rank-factor / --rank-exclude if given; no mask: the program owns no device memory)
        if (gTrackRankGiven) {
            const size_t RK = (size_t)gTrackRank;
            dppr_rank_spec_t spec{};
            spec.factor = gRankGiven ? gRankFactor : DPPR_FACTOR_NONE;
            spec.exclude = gRankGiven ? (unsigned)gRankExclude : 0u;
            std::vector<int32_t> rids(DPPR_FORWARD_MAX_M * RK), rcnt(DPPR_FORWARD_MAX_M);
            std::vector<double> rscore(DPPR_FORWARD_MAX_M * RK);
            for (size_t first = 0, t = 0; first < n_sets; first += DPPR_FORWARD_MAX_M, ++t) {
                const size_t m = std::min<size_t>(DPPR_FORWARD_MAX_M, n_sets - first);
                int32_t at = -1;
                DPPR_CHECK(engine, dppr_ftrack_info(engine, ftracks[t], &at, nullptr, nullptr, nullptr, nullptr, nullptr, 0));
                DPPR_CHECK(engine, dppr_ftrack_topk_ranked(engine, ftracks[t], &spec, gTrackRank, 0.0, rids.data(), rscore.data(), rcnt.data()));
                for (size_t j = 0; j < m; ++j) {
                    std::snprintf(line, sizeof(line), "franked %d epoch %d count %d", (int)(first + j), (int)at, (int)rcnt[j]);
                    out += line;
                    for (size_t q = 0; q < (size_t)rcnt[j]; ++q) {
                        std::snprintf(line, sizeof(line), " %d:%.17g", (int)rids[j * RK + q], rscore[j * RK + q]);
                        out += line;
                    }
                    out += "\n";
                }
            }
        }
        progress++;
        static std::mutex print_mu;
        std::lock_guard<std::mutex> lk(print_mu);
        std::cout << out << std::flush;
    }

    // --cluster: after a batch, the prefix of lowest conductance of every source's top-K order over `epoch` (dppr_cluster /
    // dppr_group_cluster: the records alone, no array comes back). Outside the timed region, printed as one block like --changes.
    void PrintClusters(int32_t epoch) {
        const size_t n_src = source_vertex_ids.size();
        std::vector<dppr_cluster_t> best;
        std::string out;
        char line[200];
        for (size_t first = 0; first < n_src; first += use_groups ? kGroupMax : 1) {
            const size_t n = use_groups ? std::min(kGroupMax, n_src - first) : 1;
            best.assign(n, dppr_cluster_t{});
            if (use_groups)
                DPPR_CHECK(engine, dppr_group_cluster(engine, groups[first / kGroupMax], epoch, gClusterK, gClusterMin, gClusterMinSize, best.data(), nullptr, nullptr, nullptr, nullptr));
            else
                DPPR_CHECK(engine, dppr_cluster(engine, slots[first], epoch, gClusterK, gClusterMin, gClusterMinSize, best.data(), nullptr, nullptr, nullptr, nullptr));
            for (size_t j = 0; j < n; ++j) {
                std::snprintf(line, sizeof(line), "cluster %d size %d cut %lld vol %lld phi %.17g\n", (int)source_vertex_ids[first + j], (int)best[j].best_size,
                              (long long)best[j].best_cut, (long long)best[j].best_vol, best[j].best_phi);
                out += line;
            }
        }
        progress++;
        static std::mutex print_mu;
        std::lock_guard<std::mutex> lk(print_mu);
        std::cout << out << std::flush;
    }

    // --subgraph: after a batch, every source's top-K order and the stored edges of `epoch` among its vertices (dppr_subgraph /
    // dppr_group_subgraph: the size query, then the fill). Outside the timed region, printed as one block like --changes; the file
    // of --subgraph-out is written anew after every batch, so it holds the last one's.
    void PrintSubgraphs(int32_t epoch) {
        const size_t n_src = source_vertex_ids.size(), k = (size_t)gSubgraphK;
        std::string out, file;
        char line[200];
        std::vector<int32_t> cnt, ids, col;
        std::vector<int64_t> off, row_ptr;
        std::vector<double> p;
        for (size_t first = 0; first < n_src; first += use_groups ? kGroupMax : 1) {
            const size_t n = use_groups ? std::min(kGroupMax, n_src - first) : 1;
            cnt.assign(n, 0), off.assign(n + 1, 0), ids.assign(n * k, -1), p.assign(n * k, 0.0), row_ptr.assign(n * (k + 1), 0);
            auto call = [&](int64_t cap) {
                if (use_groups)
                    DPPR_CHECK(engine, dppr_group_subgraph(engine, groups[first / kGroupMax], epoch, gSubgraphK, 0.0, cap, DPPR_DEST_HOST, cnt.data(), off.data(), ids.data(),
                                                           p.data(), row_ptr.data(), cap ? col.data() : nullptr));
                else
                    DPPR_CHECK(engine, dppr_subgraph(engine, slots[first], epoch, gSubgraphK, 0.0, cap, DPPR_DEST_HOST, cnt.data(), off.data(), ids.data(), p.data(),
                                                     row_ptr.data(), cap ? col.data() : nullptr));
            };
            call(0);
            col.assign((size_t)off[n], 0);
            if (off[n] > 0) call(off[n]);
            for (size_t j = 0; j < n; ++j) {
                const int src = (int)source_vertex_ids[first + j];
                std::snprintf(line, sizeof(line), "subgraph %d vertices %d edges %lld\n", src, (int)cnt[j], (long long)(off[j + 1] - off[j]));
                out += line;
                if (gSubgraphOut.empty()) continue;
                for (int32_t t = 0; t < cnt[j]; ++t) {
                    std::snprintf(line, sizeof(line), "v %d %d %d %.17g\n", src, (int)t, (int)ids[j * k + (size_t)t], p[j * k + (size_t)t]);
                    file += line;
                }
                for (int32_t t = 0; t < cnt[j]; ++t)
                    for (int64_t x = row_ptr[j * (k + 1) + (size_t)t]; x < row_ptr[j * (k + 1) + (size_t)t + 1]; ++x) {
                        std::snprintf(line, sizeof(line), "e %d %d %d\n", src, (int)t, (int)col[(size_t)x]);
                        file += line;
                    }
            }
        }
        if (!gSubgraphOut.empty()) {
            const std::string path = gSubgraphOut + (n_drivers > 1 ? "." + std::to_string(driver_index) : "");
            std::FILE *f = std::fopen(path.c_str(), "w");
            if (!f) {
                std::cout << "cannot write " << path << std::endl;
                std::exit(-1);
            }
            std::fwrite(file.data(), 1, file.size(), f);
            std::fclose(f);
        }
        progress++;
        static std::mutex print_mu;
        std::lock_guard<std::mutex> lk(print_mu);
        std::cout << out << std::flush;
    }

    // --topk-weights: the k vertices of largest sum_i w_i * p_i over this device's sources, which are one group (checked in main)
    std::vector<TopEntry> TopKWeighted(int k, const std::vector<double> &w) {
        std::vector<int32_t> ids((size_t)k, -1);
        std::vector<double> score((size_t)k, 0.0);
        int32_t cnt = 0;
        DPPR_CHECK(engine, dppr_group_topk_weighted(engine, groups[0], w.data(), 1, k, 0.0, ids.data(), score.data(), &cnt));
        std::vector<TopEntry> out;
        for (int32_t t = 0; t < cnt; ++t) out.push_back({ids[(size_t)t], score[(size_t)t]});
        return out;
    }

    double TotalPprTime() const {
        double t = 0;
        for (float x : ppr_time) t += x;
        return t;
    }

    SlidingGraphVec *graph;
    dppr_engine *engine = nullptr;
    int device_id;
    int driver_index = 0, n_drivers = 1; // which of the -g N drivers this is (the suffix of a per-driver file)
    std::vector<IndexType> source_vertex_ids;
    std::vector<size_t> target_lanes; // --target-sets: the lines of gTargetSets this device tracks, in the order of source_vertex_ids (empty: sources)
    std::vector<int32_t> slots;  // one per source (single-source mode)
    static constexpr size_t kGroupMax = 16; // sources per group (dppr_add_source_group)
    std::vector<int32_t> assign_label; // --assign: the labels of the batch before, by external id
    std::vector<int32_t> groups; // one per 16 sources (group mode: several sources per device)
    bool use_groups = false;
    std::vector<float> ppr_time; // ms per source (single mode) or per group, timed region only
    HostProfile prof;
    size_t batches_done = 0;
    bool overlap_ = false;       // the graph of batch k + 1 is built while batch k is solved (SlidingWindowExecuteOverlapped)
    double build_beside_ms = 0;  // ... time the helper thread spent on those builds
    std::atomic<unsigned long long> progress{0}; // bumped after every engine call that can take long (the watchdog of pagerank_main.cpp looks at it)

protected:
    // the progress / summary lines scripts/extract_gpu.py scrapes (gpu/PPRGPU.cuh:116-124,170-176);
    // with several sources, time is summed over sources and edges counted once per source
    void Report(size_t stream_batch_count) const {
        const double t = TotalPprTime();
        long long cur_edge_num = (long long)gStreamUpdateCountPerBatch * (long long)(stream_batch_count - 1) *
                                 (long long)source_vertex_ids.size();
        const size_t solves = (stream_batch_count - 1) * source_vertex_ids.size();
        std::cout << "coming stream_batch_count=" << stream_batch_count << std::endl;
        std::cout << "ppr_time " << t << std::endl;
        std::cout << "edge_num " << cur_edge_num << std::endl;
        std::cout << "ppr_latency " << (solves > 0 ? t / solves : 0) << std::endl;
        std::cout << "ppr_throughput " << cur_edge_num / t * 1000.0 << std::endl;
        // which loop produced the two figures above: with the graph of batch k + 1 built BESIDE the solve of batch k the
        // builder shares the device with the timed region, and ppr_latency comes out a few per cent above the serial loop's
        // (DPPR_NO_OVERLAP=1: the reference's loop shape, what tools/sweep.py and bench.py measure)
        std::cout << "graph_update " << (overlap_ ? "overlapped" : "serial") << std::endl;
    }
    bool quiet_;
};

// The reference has one driver class per variant (gpu/PPRRevPushGPU.cuh, gpu/PPRRevPushGPUVariants.cuh); here all four variants
// (-o 0 OPTIMIZED, 1 FAST_FRONTIER, 2 EAGER, 3 VANILLA) are mechanisms of one engine, selected by dppr_set_variant in the base
// class's constructor (gVariant): the duplicate filter (threshold crossing | status array) and the residual read (eager | pre-extracted)
// of the push kernels. One class therefore serves every -o.
class PPRRevPushGPU : public PPRGPU {
public:
    using PPRGPU::PPRGPU;
};
