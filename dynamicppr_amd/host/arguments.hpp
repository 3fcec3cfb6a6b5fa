// arguments.hpp -- flag parsing for ./pagerank. Same flags and defaults as the reference
// (Arguments.h:66-86); unlike it, a flag at the end of argv without a value is an error instead
// of an out-of-bounds read (util/CommandLine.h:52-55), and -a is range-checked exactly.
#pragma once

#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/dppr.h" // (DPPR_TOPK_MAX)
#include "meta.hpp"

namespace args_detail {
inline const char *find(int argc, char **argv, const char *flag) {
    for (int i = 1; i < argc; ++i) {
        if (std::strcmp(argv[i], flag) == 0) {
            if (i + 1 >= argc) {
                std::cout << "missing value after " << flag << std::endl;
                std::exit(-1);
            }
            return argv[i + 1];
        }
    }
    return nullptr;
}
inline bool has(int argc, char **argv, const char *flag) {
    for (int i = 1; i < argc; ++i)
        if (std::strcmp(argv[i], flag) == 0) return true;
    return false;
}
inline int as_int(int argc, char **argv, const char *flag, int dflt) {
    const char *v = find(argc, argv, flag);
    return v ? std::atoi(v) : dflt;
}
inline double as_double(int argc, char **argv, const char *flag, double dflt) {
    const char *v = find(argc, argv, flag);
    if (!v) return dflt;
    char *end = nullptr;
    const double x = std::strtod(v, &end);
    if (end == v) {
        std::cout << "bad number after " << flag << std::endl;
        std::exit(-1);
    }
    return x;
}
// a flag whose value must be a number and nothing else: NaN for a missing or non-numeric value (rejected by ArgumentsChecker)
inline double as_whole_double(int argc, char **argv, const char *flag, double dflt) {
    if (!has(argc, argv, flag)) return dflt;
    const char *v = find(argc, argv, flag);
    char *end = nullptr;
    const double x = v ? std::strtod(v, &end) : 0.0;
    return v && end != v && *end == '\0' ? x : std::nan("");
}
// "w1,w2,..": finite numbers separated by commas; anything else gives an empty list (rejected by ArgumentsChecker)
inline std::vector<double> parse_weights(const char *v) {
    std::vector<double> w;
    for (const char *p = v;;) {
        char *end = nullptr;
        const double x = std::strtod(p, &end);
        if (end == p || !std::isfinite(x)) return {};
        w.push_back(x);
        if (*end == '\0') return w;
        if (*end != ',') return {};
        p = end + 1;
    }
}
// --rank-factor: none | deg | inv-deg as DPPR_FACTOR_*; anything else -1 (rejected by ArgumentsChecker)
inline int parse_rank_factor(const char *v) {
    if (std::strcmp(v, "none") == 0) return DPPR_FACTOR_NONE;
    if (std::strcmp(v, "deg") == 0) return DPPR_FACTOR_DEG;
    if (std::strcmp(v, "inv-deg") == 0) return DPPR_FACTOR_INV_DEG;
    return -1;
}
// --rank-exclude: a comma-separated list of seeds | in | out as the OR of DPPR_EXCLUDE_*; an empty or unknown token gives -1
inline int parse_rank_exclude(const char *v) {
    int flags = 0;
    const std::string s(v);
    for (size_t at = 0;;) {
        const size_t end = s.find(',', at);
        const std::string tok = s.substr(at, end == std::string::npos ? std::string::npos : end - at);
        if (tok == "seeds") flags |= (int)DPPR_EXCLUDE_SEEDS;
        else if (tok == "in") flags |= (int)DPPR_EXCLUDE_IN_NEIGHBOURS;
        else if (tok == "out") flags |= (int)DPPR_EXCLUDE_OUT_NEIGHBOURS;
        else return -1;
        if (end == std::string::npos) return flags;
        at = end + 1;
    }
}
// --seeds: every line of `path` is one seed set `id[:weight] id[:weight] ...` (weight 1 where none is given; a blank line is an
// empty set). false: unreadable, no line at all, or a token that is not a non-negative id with an optional finite weight.
inline bool load_seeds(const char *path, std::vector<int64_t> &off, std::vector<int32_t> &ids, std::vector<double> &w) {
    std::ifstream in(path);
    if (!in) return false;
    off.assign(1, 0);
    ids.clear();
    w.clear();
    std::string line, tok;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        while (ls >> tok) {
            char *end = nullptr;
            errno = 0;
            const long long id = std::strtoll(tok.c_str(), &end, 10);
            if (end == tok.c_str() || errno || id < 0 || id > INT32_MAX) return false;
            double weight = 1.0;
            if (*end == ':') {
                const char *ws = end + 1;
                weight = std::strtod(ws, &end);
                if (end == ws || !std::isfinite(weight)) return false;
            }
            if (*end != '\0') return false;
            ids.push_back((int32_t)id);
            w.push_back(weight);
        }
        off.push_back((int64_t)ids.size());
    }
    return off.size() > 1;
}
// --target-sets: the format of --seeds, one lane per line. false: what load_seeds rejects, or a blank line (a lane has a seed).
// The weights' sign, the ids' range and an id twice in a lane are the engine's to reject (dppr_add_target_group).
inline bool load_target_sets(const char *path, std::vector<std::vector<std::pair<int32_t, double>>> &lanes) {
    std::vector<int64_t> off;
    std::vector<int32_t> ids;
    std::vector<double> w;
    lanes.clear();
    if (!load_seeds(path, off, ids, w)) return false;
    for (size_t i = 0; i + 1 < off.size(); ++i) {
        if (off[i + 1] == off[i]) return false;
        lanes.emplace_back();
        for (int64_t k = off[i]; k < off[i + 1]; ++k) lanes.back().emplace_back(ids[(size_t)k], w[(size_t)k]);
    }
    return !lanes.empty();
}
// --refine, --positions, --explain: one external vertex id per line (blank lines are skipped). false: unreadable, no id, or a token that is not an id >= 0.
inline bool load_ids(const char *path, std::vector<int32_t> &ids) {
    std::ifstream in(path);
    if (!in) return false;
    ids.clear();
    std::string tok;
    while (in >> tok) {
        char *end = nullptr;
        errno = 0;
        const long long id = std::strtoll(tok.c_str(), &end, 10);
        if (end == tok.c_str() || *end != '\0' || errno || id < 0 || id > INT32_MAX) return false;
        ids.push_back((int32_t)id);
    }
    return !ids.empty();
}
} // namespace args_detail

inline void PrintUsage() {
    std::cout << "==========[USAGE]==========\n"
              << "-d: gDataFileName\n-a: gAppType\n" << REVERSE_PUSH << ":rev push\n"
              << "-i: gIsDirected\n-y: gIsDynamic\n-w: gWindowRatio\n-n: gWorkloadConfigType\n"
              << SLIDE_WINDOW_RATIO << ": SLIDE_WINDOW_RATIO, " << SLIDE_BATCH_SIZE << ": SLIDE_BATCH_SIZE\n"
              << "-r: gStreamUpdateCountVersusWindowRatio\n-b: gStreamBatchCount\n"
              << "-c: gStreamUpdateCountPerBatch\n-l: gStreamUpdateCountTotal\n"
              << "-s: gSourceVertexId\n-t: gThreadNum (ignored on the GPU)\n-o: gVariant\n-e: error tolerance\n"
              << "-g: number of GPUs (sources are dealt round-robin)\n"
              << "--sources <file>: one source vertex id per line (overrides -s)\n"
              << "--target-sets <file>: instead of --sources / -s: one weighted vertex set per line, tokens `id` or `id:weight` (a bare id\n"
              << "            weighs 1.0; weights finite and > 0, no id twice in a line). Every line is one lane that tracks the pagerank\n"
              << "            towards its set; lanes are dealt into groups of up to 16 like sources (not with --split / --no-groups /\n"
              << "            --topk-weights). A lane is named by its first id in the outputs; --validate checks the residual bound and the\n"
              << "            invariant with the lane's seed vector\n"
              << "--dump <path>: write pagerank/residual of every source after the last batch\n"
              << "--topk <K>: after the last batch print the K vertices of largest pagerank of every source (1 <= K <= 8192),\n"
              << "            one line each, in source order: topk <source> <rank from 1> <vertex> <pagerank>\n"
              << "--topk-weights <w1,w2,...>: with --topk and all sources in one group (one GPU, 2 to 16 sources, no --no-groups / --split),\n"
              << "            one finite weight per source: after the topk lines, the K vertices of largest sum_i w_i * pagerank_i,\n"
              << "            one line each: topkw <rank from 1> <vertex> <score>\n"
              << "--rank-factor <none|deg|inv-deg> [--rank-exclude <seeds,in,out>]: with --topk, after the topk lines the K best of every source\n"
              << "            by pagerank * (outdeg + 1) (deg: the forward-PPR order on an undirected window), / (outdeg + 1) (inv-deg) or as it\n"
              << "            is (none), without the source itself (seeds), the vertices with an edge to it (in) or from it (out), one line each:\n"
              << "            ranked <source> <rank from 1> <vertex> <score>   (either flag alone is enough; not with --split)\n"
              << "--changes <K> [--changes-min <D>]: after every batch print, per source in source order, what the batch moved (1 <= K <= 8192, D >= 0):\n"
              << "            moved <batch> <source> <vertices with |delta pagerank| > D>, then the K largest of them by |delta|, one line each:\n"
              << "            changes <batch> <source> <rank from 1> <vertex> <delta> <pagerank>\n"
              << "--sparse-min <P> [--sparse-out <file>]: after the last batch print, per source in source order, the number of vertices\n"
              << "            with pagerank > P (P >= 0): support <source> <count>; with --sparse-out also write them to <file>,\n"
              << "            one line each, by source then vertex id: <source> <vertex> <pagerank>\n"
              << "--patch-min <P> [--patch-delta <D>] [--patch-out <file>]: after every batch print, per source in source order, the size of the patch\n"
              << "            that brings a replica of {pagerank > P} up to date (P >= 0, D >= 0; not with --changes): patch <source> upserts <a> deletes <b>;\n"
              << "            an entry that stays above P is sent again only once it has moved by more than D since it was last sent. With --patch-out\n"
              << "            also append the entries to <file>, by source then vertex id: U <batch> <source> <vertex> <pagerank> / D <batch> <source> <vertex>\n"
              << "--seeds <file>: every line of <file> is one seed set `id[:weight] id[:weight] ...` (weight 1 by default, ids in [0, V));\n"
              << "            after the last batch print, per line (from 1) and per source in source order, the source's PPR under that seed\n"
              << "            distribution, sum_v weight[v] * pagerank_source[v]: seedscore <line> <source> <score>\n"
              << "--refine <file> --walks <W> [--walk-seed <S>]: <file> holds one vertex id per line (ids in [0, V), at most 4096, W in [1, 2^20],\n"
              << "            ids x W <= 2^26); after every batch print, per id and per source (index from 0, in source order), the pagerank\n"
              << "            refined by W random walks, its correction and its standard error: refined <vertex> <source index> <est> <corr> <stderr>\n"
              << "--positions <file>: <file> holds one vertex id per line (ids in [0, V), at most 4096); after every batch print, per source in source\n"
              << "            order, where every id stands in the source's order by pagerank -- by the score of --rank-factor / --rank-exclude if\n"
              << "            given (no --topk needed) --, from 0, -1 if its score is not > 0: position <source> <vertex> <pos>, then the number\n"
              << "            of vertices that have a position: positions <source> qualifying <count>   (not with --split)\n"
              << "--explain <file> [--explain-top <F>] [--explain-depth <D>]: <file> holds one vertex id per line (ids in [0, V), at most 4096); after every\n"
              << "            batch print, per source in source order and per id, the path of largest contributions towards the source, at most D hops\n"
              << "            (0 <= D <= 64, default 16): explain <source> <vertex> <end> <len> <v0> <v1> ...  (end 0 seed, 1 depth, 2 dead end, 3 cycle),\n"
              << "            then the F out-neighbours that contribute most to its pagerank (0 <= F <= 16, default 3, F + D >= 1):\n"
              << "            because <source> <vertex> <neighbour> <stored copies> <contribution>   (not with --split)\n"
              << "--certify <N>: after the initial solve and after every N-th batch (N >= 1) certify every source's state on the device, against the\n"
              << "            batch's own graph: certify <source> epoch=<id> max_r=<largest |r|> at=<vertex> sum_r=<sum of |r|> legal=<vertices still\n"
              << "            legal to push> nonfinite=<rows with a NaN or inf> inv=<largest violation of the invariant> inv_at=<vertex>; the program\n"
              << "            prints CERTIFY FAILED: ... and exits non-zero if legal > 0, nonfinite > 0 or inv >= 1e-13 * max(1, sum of the lane's\n"
              << "            seed weights)   (not with --split)\n"
              << "--forward <file> [--forward-iters <N>] [--forward-tol <T>] [--forward-topk <K>]: <file> holds one vertex id per line; after every\n"
              << "            batch sweep the walk FROM each of them forward over the batch's own graph (any vertex, tracked or not; 1 <= N <= 256\n"
              << "            iterations, default 64; a start stops at a check -- every 8 iterations -- once less than T of its mass remains, default\n"
              << "            0; the K vertices it reaches most, 0 <= K <= 64, default 5): forward <vertex> iters <used> rem <mass remaining> top <found>\n"
              << "            <v0>:<f0> <v1>:<f1> ...   (starts beyond 16 go in calls of 16; not with --split)\n"
              << "--forward-push <file> --push-eps <E> [--push-rounds <N>]: <file> holds one weighted vertex set per line as --target-sets; after\n"
              << "            every batch run the frontier-driven forward push from each set over the batch's own graph (E > 0: a vertex is pushed\n"
              << "            while its residual exceeds E * (outdeg + 1); at most N rounds, 1 <= N <= 256, default 64; the --forward-topk K vertices\n"
              << "            it reaches most): fpush <first id> seeds <count> rounds <used> converged <0|1> rem <mass remaining> pushes <count> left\n"
              << "            <count> top <found> <v0>:<p0> ...   (sets beyond 16 go in calls of 16; not with --split)\n"
              << "--forward-track <file> --push-eps <E> [--push-rounds <N>]: <file> as --forward-push (at most 256 sets); a forward track per 16\n"
              << "            sets is created after the initial solve and moved to every batch's graph by a fix-up over the batch's records and\n"
              << "            signed push rounds, instead of a push from zero: ftrack <first id> seeds <count> epoch <e> rounds <used> converged <0|1>\n"
              << "            rem <fold of |r|> pushes <count> fix <records> <tails> <heads> top <found> <v0>:<p0> ...   (not with --split)\n"
              << "--forward-cluster deg|p: with --forward-track, after the create and after every batch sweep every set's WHOLE order -- every vertex an\n"
              << "            edge names with a score > 0, by p / (outdeg + 1) (deg) or by p -- for its prefix of lowest conductance (dppr_ftrack_cluster):\n"
              << "            fcluster <first id> size <best_size> of <count> cut <cut_out> vol <vol> phi <conductance, %.17g>\n"
              << "--forward-rank <K>: with --forward-track, after the create and after every batch print the K best of every set by the ranked query\n"
              << "            over the track's own p (dppr_ftrack_topk_ranked; 1 <= K <= 8192) -- by the score of --rank-factor / --rank-exclude if given (the\n"
              << "            seeds are the set's, the degrees and neighbours those of the epoch the track stands on; no --topk needed):\n"
              << "            franked <set index> epoch <e> count <found> <v0>:<score0, %.17g> ...\n"
              << "--sample <S> [--sample-seed <X>]: after every batch draw, per source in source order, S vertices with replacement in proportion to\n"
              << "            the source's pagerank -- to the score of --rank-factor / --rank-exclude if given (no --topk needed) -- (1 <= S <= 2^20;\n"
              << "            the draws are a function of the scores, the source's lane, X and the draw number alone): sample <source> lane <lane>\n"
              << "            total <sum of the weights> support <vertices of positive weight> status <0 ok, 1 empty, 2 not finite> distinct <ids drawn>\n"
              << "            ids <the first 8>   (not with --split)\n"
              << "--cluster <K> [--cluster-min <P>] [--cluster-min-size <M>]: after every batch print, per source in source order, the prefix of\n"
              << "            lowest conductance of the source's K vertices of largest pagerank > P (1 <= K <= 8192, P >= 0, 1 <= M <= K vertices\n"
              << "            at least): cluster <source> size <vertices> cut <edges leaving it> vol <its out-degrees> phi <conductance>\n"
              << "--subgraph <K> [--subgraph-out <file>]: after every batch print, per source in source order, the size of the subgraph its K\n"
              << "            vertices of largest pagerank induce (1 <= K <= 8192): subgraph <source> vertices <L> edges <stored edges among them>;\n"
              << "            with --subgraph-out also write it to <file> (the last batch's; with -g N one file per device, <file>.<device>):\n"
              << "            v <source> <position> <vertex> <pagerank> per vertex, e <source> <tail position> <head position> per edge\n"
              << "--assign [--assign-min <S>] [--assign-out <file>]: one class per source (or per line of --target-sets), in source order;\n"
              << "            after every batch print the label propagation over them -- every vertex goes to the class of its largest\n"
              << "            pagerank > S (S >= 0, default 0; ties to the first class; none: unassigned) --, flips counted against the batch before\n"
              << "            (the first against all unassigned): assign <batch> classes=<C> unassigned=<n> flips=<n> counts=c0,c1,...\n"
              << "            with --assign-out also write the last labels to <file>, raw int32 [V], -1 = unassigned. Needs the sources in groups\n"
              << "            on ONE device (2 to 256 sources or --target-sets; not with -g N > 1, --no-groups, --split)\n"
              << "--validate: residual bound + power-iteration check after every solve\n"
              << "--split: drive each batch through IncrementalBatchUpdate/ExecuteMainLoop(0)/(1)\n"
              << "--sync: synchronous (deterministic) push schedule\n"
              << "--share-device: with -g N on a node of fewer devices, device thread d uses device d % (devices present) (also DPPR_DEVICE_ALIAS=1)\n"
              << "--push-only: every iteration as a push iteration (no pull sweeps): what the -o variants differ in\n"
              << "--merge-phases: push the residuals of both signs in ONE loop, to eps / 4 (not the reference's schedule; same pushes, |p - p_reference| < 1e-9)\n"
              << "--no-groups: with several sources per GPU, solve them one at a time (default: up to 16 together)\n"
              << "--profile: per-iteration frontier lines and the phase-time report of the reference's -DPROFILE build (implies --split)\n"
              << "EXAMPLE: ./pagerank -d ../data/com-dblp.ungraph.bin -a 0 -i 0 -y 1 -w 0.1 -n 0 -r 0.01 -b 1000 -s 1\n"
              << "EXAMPLE: ./pagerank -d ../data/com-dblp.ungraph.bin -a 0 -i 0 -y 1 -w 0.1 -n 1 -c 100 -l 10000 -s 1"
              << std::endl;
}

inline void PrintArguments() {
    std::cout << "gAppType=" << gAppType << ",gIsDirected=" << gIsDirected << ",gIsDynamic=" << gIsDynamic << std::endl;
    std::cout << "gWindowRatio=" << gWindowRatio << ",gWorkloadConfigType=" << gWorkloadConfigType
              << ",gStreamUpdateCountVersusWindowRatio=" << gStreamUpdateCountVersusWindowRatio
              << ",gStreamBatchCount=" << gStreamBatchCount << ",gStreamUpdateCountPerBatch="
              << gStreamUpdateCountPerBatch << ",gStreamUpdateCountTotal=" << gStreamUpdateCountTotal << std::endl;
    std::cout << "gSourceVertexId=" << gSourceVertexId << std::endl;
    std::cout << "gThreadNum=" << gThreadNum << ",gVariant=" << gVariant << std::endl;
    std::cout << "error=" << gTolerance << ",ALPHA=" << ALPHA << std::endl;
}

inline void ArgumentsChecker() {
    bool ok = gAppType >= 0 && gAppType < kAlgoTypeSize && gIsDirected >= 0 && gIsDynamic >= 0 &&
              !gDataFileName.empty() && gTolerance > 0 && gNumGpus >= 1;
    if (gWorkloadConfigType == SLIDE_WINDOW_RATIO)
        ok = ok && gStreamUpdateCountVersusWindowRatio >= 0.0 && gStreamBatchCount != 0;
    else if (gWorkloadConfigType == SLIDE_BATCH_SIZE)
        ok = ok && gStreamUpdateCountPerBatch != 0 && gStreamUpdateCountTotal != 0;
    else
        ok = false;
    if (gIsDynamic == 0) {
        std::cout << "-y 0 (static mode) is deprecated in the reference (README.md:82) and not supported" << std::endl;
        ok = false;
    }
    if (gVariant < 0 || gVariant >= kVariantTypeSize) ok = false;
    if (gTopK < 0 || gTopK > DPPR_TOPK_MAX) ok = false;
    if (gChangesK < 0 || gChangesK > DPPR_TOPK_MAX || !(gChangesMin >= 0.0) || (gChangesMinGiven && gChangesK == 0)) ok = false;
    if ((gSparseGiven && !(gSparseMin >= 0.0)) || (!gSparseOut.empty() && !gSparseGiven)) ok = false;
    // (a value that is no number was read as NaN and fails `>=`; --patch-min and --changes would share one mark)
    if ((gPatchGiven && (!(gPatchMin >= 0.0) || !(gPatchDelta >= 0.0) || gChangesK > 0)) || ((gPatchDeltaGiven || !gPatchOut.empty()) && !gPatchGiven)) ok = false;
    if (gSeedsBad) ok = false;
    if (gRefineBad || gRefineFile.empty() != !gWalksGiven) ok = false;
    if (!gRefineFile.empty() && !gRefineBad &&
        (gWalks < 1 || gWalks > DPPR_WALK_MAX_W || gRefineIds.size() > (size_t)DPPR_WALK_MAX_M || (long long)gRefineIds.size() * gWalks > (1ll << 26)))
        ok = false;
    if (gPositionsBad || (!gPositionsFile.empty() && (gPositionIds.size() > (size_t)DPPR_POSITION_MAX || gSplitInterface))) ok = false;
    if (gExplainBad || (gExplainOptsGiven && gExplainFile.empty())) ok = false;
    if (!gExplainFile.empty() && (gExplainIds.size() > (size_t)DPPR_EXPLAIN_MAX_M || gSplitInterface || gExplainTop < 0 || gExplainTop > DPPR_EXPLAIN_MAX_F ||
                                  gExplainDepth < 0 || gExplainDepth > DPPR_EXPLAIN_MAX_DEPTH || gExplainTop + gExplainDepth < 1))
        ok = false;
    if (gCertifyGiven && (gCertifyBad || gCertify < 1 || gSplitInterface)) ok = false;
    if (gClusterGiven && (gClusterK < 1 || gClusterK > DPPR_CLUSTER_MAX || !(gClusterMin >= 0.0) || gClusterMinSize < 1 || gClusterMinSize > gClusterK))
        ok = false;
    if (gClusterOptsGiven && !gClusterGiven) ok = false;
    if ((gSubgraphGiven && (gSubgraphK < 1 || gSubgraphK > DPPR_SUBGRAPH_MAX)) || (!gSubgraphOut.empty() && !gSubgraphGiven)) ok = false;
    if (gTopKWeightsGiven && (gTopK == 0 || gTopKWeights.empty())) ok = false; // (the count is checked against the sources in main)
    if (gForwardBad || (gForwardOptsGiven && gForwardFile.empty())) ok = false;
    if (!gForwardFile.empty() && (gSplitInterface || gForwardIters < 1 || gForwardIters > DPPR_FORWARD_MAX_ITERS || !(gForwardTol >= 0.0) ||
                                  !std::isfinite(gForwardTol) || gForwardTopK < 0 || gForwardTopK > 64))
        ok = false;
    if (!gTrackCluster.empty() && (gTrackFile.empty() || (gTrackCluster != "deg" && gTrackCluster != "p"))) ok = false;
    if (gTrackRankGiven && (gTrackFile.empty() || gTrackRank < 1 || gTrackRank > DPPR_TOPK_MAX)) ok = false;
    if (gPushBad || gTrackBad || (gPushOptsGiven && gPushFile.empty() && gTrackFile.empty())) ok = false;
    if (!gTrackFile.empty() && (gSplitInterface || !(gPushEps > 0.0) || !std::isfinite(gPushEps) || gPushRounds < 1 || gPushRounds > DPPR_FPUSH_MAX_ROUNDS ||
                                gForwardTopK < 0 || gForwardTopK > 64 || gTrackSets.size() > (size_t)DPPR_FTRACK_MAX * DPPR_FORWARD_MAX_M))
        ok = false;
    if (!gPushFile.empty() && (gSplitInterface || !(gPushEps > 0.0) || !std::isfinite(gPushEps) || gPushRounds < 1 || gPushRounds > DPPR_FPUSH_MAX_ROUNDS ||
                               gForwardTopK < 0 || gForwardTopK > 64))
        ok = false;
    if ((gSampleGiven && (gSample < 1 || gSample > DPPR_SAMPLE_MAX || gSplitInterface)) || (gSampleSeedGiven && !gSampleGiven)) ok = false;
    if (gRankGiven && ((gTopK == 0 && gPositionsFile.empty() && !gSampleGiven && !gTrackRankGiven) || gRankFactor < 0 || gRankExclude < 0 || gSplitInterface)) ok = false;
    if (!gTargetSetsFile.empty() && (gTargetSetsBad || gTargetSets.empty() || !gSourcesFile.empty() || gSplitInterface || gNoGroups || gTopKWeightsGiven)) ok = false;
    if ((gAssignMinGiven || !gAssignOut.empty()) && !gAssign) ok = false;
    if (gAssign && (!(gAssignMin >= 0.0) || gSplitInterface || gNoGroups)) ok = false; // (one device, groups in use: checked against the sources in main)
    if (!ok) {
        std::cout << "invalid arguments" << std::endl;
        PrintUsage();
        std::exit(-1);
    }
}

inline void ArgumentsParser(int argc, char **argv) {
    using namespace args_detail;
    if (const char *d = find(argc, argv, "-d")) gDataFileName = d;
    gAppType = as_int(argc, argv, "-a", 0);
    gIsDirected = as_int(argc, argv, "-i", -1);
    gIsDynamic = as_int(argc, argv, "-y", -1);
    gWindowRatio = as_double(argc, argv, "-w", 0.1);
    gWorkloadConfigType = as_int(argc, argv, "-n", SLIDE_WINDOW_RATIO);
    gStreamUpdateCountVersusWindowRatio = as_double(argc, argv, "-r", -1.0);
    gStreamBatchCount = (size_t)as_int(argc, argv, "-b", 0);
    gStreamUpdateCountPerBatch = (size_t)as_int(argc, argv, "-c", 0);
    gStreamUpdateCountTotal = (size_t)as_int(argc, argv, "-l", 0);
    gSourceVertexId = as_int(argc, argv, "-s", 1);
    gThreadNum = as_int(argc, argv, "-t", 1);
    gVariant = as_int(argc, argv, "-o", 0);
    gTolerance = as_double(argc, argv, "-e", 1e-9);
    gNumGpus = as_int(argc, argv, "-g", 1);
    if (const char *f = find(argc, argv, "--sources")) gSourcesFile = f;
    if (const char *f = find(argc, argv, "--target-sets")) {
        gTargetSetsFile = f;
        gTargetSetsBad = !load_target_sets(f, gTargetSets);
    }
    if (const char *f = find(argc, argv, "--dump")) gDumpPath = f;
    gTopK = as_int(argc, argv, "--topk", 0);
    if (const char *w = find(argc, argv, "--topk-weights")) {
        gTopKWeightsGiven = true;
        gTopKWeights = parse_weights(w);
    }
    if (const char *f = find(argc, argv, "--rank-factor")) {
        gRankGiven = true;
        gRankFactor = parse_rank_factor(f);
    }
    if (const char *x = find(argc, argv, "--rank-exclude")) {
        gRankGiven = true;
        gRankExclude = parse_rank_exclude(x);
    }
    gChangesK = as_int(argc, argv, "--changes", 0);
    gChangesMinGiven = find(argc, argv, "--changes-min") != nullptr;
    gChangesMin = as_double(argc, argv, "--changes-min", 0.0);
    gSparseGiven = find(argc, argv, "--sparse-min") != nullptr;
    gSparseMin = as_double(argc, argv, "--sparse-min", 0.0);
    if (const char *f = find(argc, argv, "--sparse-out")) gSparseOut = f;
    gPatchGiven = has(argc, argv, "--patch-min");
    gPatchDeltaGiven = has(argc, argv, "--patch-delta");
    gPatchMin = as_whole_double(argc, argv, "--patch-min", 0.0);
    gPatchDelta = as_whole_double(argc, argv, "--patch-delta", 0.0);
    if (const char *f = find(argc, argv, "--patch-out")) gPatchOut = f;
    if (const char *f = find(argc, argv, "--seeds")) {
        gSeedsFile = f;
        gSeedsBad = !load_seeds(f, gSeedOff, gSeedIds, gSeedW);
    }
    if (const char *f = find(argc, argv, "--refine")) {
        gRefineFile = f;
        gRefineBad = !load_ids(f, gRefineIds);
    }
    if (const char *f = find(argc, argv, "--positions")) {
        gPositionsFile = f;
        gPositionsBad = !load_ids(f, gPositionIds);
    }
    if (const char *f = find(argc, argv, "--explain")) {
        gExplainFile = f;
        gExplainBad = !load_ids(f, gExplainIds);
    }
    gExplainOptsGiven = find(argc, argv, "--explain-top") != nullptr || find(argc, argv, "--explain-depth") != nullptr;
    gExplainTop = as_int(argc, argv, "--explain-top", 3);
    gExplainDepth = as_int(argc, argv, "--explain-depth", 16);
    if (const char *v = find(argc, argv, "--certify")) { // (a whole number, all of the token)
        gCertifyGiven = true;
        char *end = nullptr;
        const long x = std::strtol(v, &end, 10);
        gCertifyBad = end == v || *end != '\0' || x > 1000000000l;
        gCertify = gCertifyBad || x < 0 ? 0 : (int)x;
    }
    if (const char *f = find(argc, argv, "--forward")) {
        gForwardFile = f;
        gForwardBad = !load_ids(f, gForwardIds);
    }
    if (const char *f = find(argc, argv, "--forward-push")) {
        gPushFile = f;
        gPushBad = !load_target_sets(f, gPushSets);
    }
    if (const char *f = find(argc, argv, "--forward-track")) {
        gTrackFile = f;
        gTrackBad = !load_target_sets(f, gTrackSets);
    }
    if (has(argc, argv, "--forward-cluster")) {
        const char *v = find(argc, argv, "--forward-cluster");
        gTrackCluster = v && *v ? v : "?"; // (no value, or an empty one: refused with the usage)
    }
    gTrackRankGiven = has(argc, argv, "--forward-rank");
    gTrackRank = as_int(argc, argv, "--forward-rank", 0);
    gPushOptsGiven = has(argc, argv, "--push-eps") || has(argc, argv, "--push-rounds");
    gPushEps = as_whole_double(argc, argv, "--push-eps", 0.0);
    gPushRounds = as_int(argc, argv, "--push-rounds", 64);
    gForwardOptsGiven = has(argc, argv, "--forward-iters") || has(argc, argv, "--forward-tol") || (has(argc, argv, "--forward-topk") && gPushFile.empty() && gTrackFile.empty());
    gForwardIters = as_int(argc, argv, "--forward-iters", 64);
    gForwardTol = as_whole_double(argc, argv, "--forward-tol", 0.0);
    gForwardTopK = as_int(argc, argv, "--forward-topk", 5);
    gSampleGiven = has(argc, argv, "--sample");
    gSample = as_int(argc, argv, "--sample", 0);
    gSampleSeedGiven = has(argc, argv, "--sample-seed");
    if (const char *v = find(argc, argv, "--sample-seed")) gSampleSeed = std::strtoull(v, nullptr, 0);
    gWalksGiven = find(argc, argv, "--walks") != nullptr;
    gWalks = as_int(argc, argv, "--walks", 0);
    if (const char *v = find(argc, argv, "--walk-seed")) gWalkSeed = std::strtoull(v, nullptr, 0);
    gClusterGiven = find(argc, argv, "--cluster") != nullptr;
    gClusterK = as_int(argc, argv, "--cluster", 0);
    gClusterOptsGiven = find(argc, argv, "--cluster-min") != nullptr || find(argc, argv, "--cluster-min-size") != nullptr;
    gClusterMin = as_double(argc, argv, "--cluster-min", 0.0);
    gClusterMinSize = as_int(argc, argv, "--cluster-min-size", 1);
    gSubgraphGiven = find(argc, argv, "--subgraph") != nullptr;
    gSubgraphK = as_int(argc, argv, "--subgraph", 0);
    if (const char *f = find(argc, argv, "--subgraph-out")) gSubgraphOut = f;
    gAssign = has(argc, argv, "--assign");
    gAssignMinGiven = find(argc, argv, "--assign-min") != nullptr;
    gAssignMin = as_double(argc, argv, "--assign-min", 0.0);
    if (const char *f = find(argc, argv, "--assign-out")) gAssignOut = f;
    gValidate = has(argc, argv, "--validate");
    gSplitInterface = has(argc, argv, "--split");
    gSchedule = has(argc, argv, "--sync") ? 1 : 0;
    gNoGroups = has(argc, argv, "--no-groups");
    gMergePhases = has(argc, argv, "--merge-phases");
    gPushOnly = has(argc, argv, "--push-only");
    gShareDevice = has(argc, argv, "--share-device") || (getenv("DPPR_DEVICE_ALIAS") && atoi(getenv("DPPR_DEVICE_ALIAS")) != 0);
    gProfile = has(argc, argv, "--profile");
    if (gProfile) gSplitInterface = true; // the phases are timed and traced around the three virtual calls
    // -o: the reference's four variants (gpu/PPRRevPushGPUVariants.cuh) = {eager residual read | pre-extracted residuals
    // (InspectExtra)} x {threshold-crossing | status-array duplicate filter}; the engine has both mechanisms of both kinds
    // (dppr_set_variant). The pre-extracting variants (1 FAST_FRONTIER, 3 VANILLA) run the synchronous schedule.
    if (gVariant == FAST_FRONTIER || gVariant == VANILLA) gSchedule = 1;
    ArgumentsChecker();
}
