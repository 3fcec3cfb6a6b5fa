// meta.hpp -- constants, flag globals and small helpers of the host program.
//
// The names of the flag globals (gDataFileName ... gTolerance) and of the enums are the
// reference's CLI contract (Meta.h:5-67, Meta.cpp); everything else is new code.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

using IndexType = int32_t; // Meta.h:26
using ValueType = double;  // Meta.h:25

enum AlgoType { REVERSE_PUSH = 0, kAlgoTypeSize };
enum VariantType { OPTIMIZED = 0, FAST_FRONTIER = 1, EAGER = 2, VANILLA = 3, kVariantTypeSize };
enum WorkloadConfigType {
    SLIDE_WINDOW_RATIO, // batch = ratio of the window (-r, -b)
    SLIDE_BATCH_SIZE    // batch = fixed number of edges (-c, -l)
};

constexpr ValueType ALPHA = 0.15; // Meta.h:31

// ---- flags (same letters and defaults as Arguments.h:66-86) -------------------------------
inline std::string gDataFileName;
inline int gAppType = -1;
inline int gIsDirected = -1;
inline int gIsDynamic = -1;
inline double gWindowRatio = 0.1;
inline int gWorkloadConfigType = SLIDE_WINDOW_RATIO;
inline double gStreamUpdateCountVersusWindowRatio = -1.0;
inline size_t gStreamBatchCount = 0;
inline size_t gStreamUpdateCountPerBatch = 0;
inline size_t gStreamUpdateCountTotal = 0;
inline int gSourceVertexId = 1;
inline int gThreadNum = 1;
inline int gVariant = OPTIMIZED;
inline ValueType gTolerance = 1e-9;
// ---- additions of this build ------------------------------------------------------------
inline int gNumGpus = 1;              // -g : devices; sources are dealt round-robin over them
inline std::string gSourcesFile;      // --sources : file with one source vertex id per line
inline std::string gTargetSetsFile;   // --target-sets : file with one weighted vertex set per line (a lane each; instead of --sources)
inline std::vector<std::vector<std::pair<int32_t, double>>> gTargetSets; // ... its lanes: (vertex, weight)
inline bool gTargetSetsBad = false;   // ... unreadable, or a token that is no `id` / `id:weight`
inline std::string gDumpPath;         // --dump : write p/r of every source after the last batch
inline int gTopK = 0;                 // --topk K : print the K vertices of largest p of every source after the last batch (0: off)
inline std::vector<double> gTopKWeights; // --topk-weights w1,w2,.. : also rank the weighted combination of the sources (one weight per source, all in one group)
inline bool gTopKWeightsGiven = false;
inline bool gRankGiven = false;       // --rank-factor / --rank-exclude : with --topk, also print the K best by the ranked query (ranked <source> ...)
inline int gRankFactor = 0;           // --rank-factor none|deg|inv-deg : DPPR_FACTOR_NONE / _DEG / _INV_DEG (-1: not one of them)
inline int gRankExclude = 0;          // --rank-exclude seeds,in,out : OR of DPPR_EXCLUDE_* (-1: a token that is none of the three)
inline int gChangesK = 0;             // --changes K : after every batch print, per source, how many vertices moved and the K largest |delta p| (0: off)
inline double gChangesMin = 0.0;      // --changes-min D : only vertices with |delta p| > D count and are printed
inline bool gSparseGiven = false;     // --sparse-min P : after the last batch print, per source, how many vertices have pagerank > P (support <source> <count>)
inline double gSparseMin = 0.0;
inline std::string gSparseOut;        // --sparse-out FILE : ... and write them, one text line `source id pagerank` each, by source then id
inline bool gChangesMinGiven = false;
inline bool gPatchGiven = false;      // --patch-min P : after every batch print, per source, the size of the patch of {pagerank > P} (patch <source> upserts <a> deletes <b>)
inline double gPatchMin = 0.0;
inline bool gPatchDeltaGiven = false; // --patch-delta D : an entry that stays above P is sent again only once it has moved by more than D since it was last sent
inline double gPatchDelta = 0.0;
inline std::string gPatchOut;         // --patch-out FILE : ... and append the patch, one text line `U batch source id pagerank` or `D batch source id` per entry
inline std::string gSeedsFile;        // --seeds FILE : every line one seed set `id[:weight] ...`; after the last batch print seedscore <line> <source> <score>
inline bool gSeedsBad = false;        //   FILE could not be read, holds no line, or a token is not id[:weight] with id >= 0
inline std::vector<int64_t> gSeedOff; //   the seed sets as one CSR over the lines: offsets [lines + 1], external ids, weights
inline std::vector<int32_t> gSeedIds;
inline std::vector<double> gSeedW;
inline std::string gRefineFile;       // --refine FILE : one external vertex id per line; after every batch print refined <v> <source index> <est> <corr> <stderr>
inline bool gRefineBad = false;       //   FILE could not be read, holds no id, or a token is not an id >= 0
inline std::vector<int32_t> gRefineIds;
inline std::string gPositionsFile;    // --positions FILE : one external vertex id per line; after every batch print position <source> <v> <pos> and positions <source> qualifying <count>
inline bool gPositionsBad = false;    //   FILE could not be read, holds no id, or a token is not an id >= 0
inline std::vector<int32_t> gPositionIds;
inline std::string gExplainFile;      // --explain FILE : one external vertex id per line; after every batch print explain <source> <v> <end> <len> <v0> <v1> ... and because <source> <v> <w> <mult> <c>
inline bool gExplainBad = false;      //   FILE could not be read, holds no id, or a token is not an id >= 0
inline std::vector<int32_t> gExplainIds;
inline int gExplainTop = 3;           // --explain-top F : contributors listed per id and source
inline int gExplainDepth = 16;        // --explain-depth D : hops of the path at the most
inline bool gExplainOptsGiven = false;
inline int gCertify = 0;              // --certify N : after the initial solve and after every N-th batch print certify <source> epoch=.. max_r=.. ... (dppr_certify / dppr_group_certify)
inline bool gCertifyGiven = false;
inline bool gCertifyBad = false;      //   N is not a whole number
inline std::string gForwardFile;      // --forward FILE : one external vertex id per line; after every batch print one forward line per start (dppr_forward)
inline bool gForwardBad = false;      //   FILE could not be read, holds no id, or a token is not an id >= 0
inline std::vector<int32_t> gForwardIds;
inline bool gForwardOptsGiven = false; // --forward-iters / --forward-tol / --forward-topk
inline int gForwardIters = 64;        // --forward-iters N (1 <= N <= 256)
inline double gForwardTol = 0.0;      // --forward-tol T (T >= 0)
inline std::string gPushFile;         // --forward-push FILE : one weighted vertex set per line (the format of --target-sets); after every batch print one fpush line per set (dppr_forward_push)
inline bool gPushBad = false;         //   FILE could not be read, holds no set, or a token is not `id` or `id:weight`
inline std::vector<std::vector<std::pair<int32_t, double>>> gPushSets;
inline bool gPushOptsGiven = false;   // --push-eps / --push-rounds
inline double gPushEps = 0.0;         // --push-eps E (E > 0; required with --forward-push and --forward-track)
inline int gPushRounds = 64;          // --push-rounds N (1 <= N <= 256)
inline std::string gTrackFile;        // --forward-track FILE : sets as --forward-push; a forward track per 16 sets is created after the initial solve and updated after every batch (dppr_ftrack_*; --push-eps, --push-rounds)
inline bool gTrackBad = false;        //   FILE could not be read, holds no set or more than 256, or a token is not `id` or `id:weight`
inline std::vector<std::vector<std::pair<int32_t, double>>> gTrackSets;
inline std::string gTrackCluster;     // --forward-cluster deg|p : with --forward-track, the full-length conductance sweep of every set's p after the create and after every batch (dppr_ftrack_cluster)
inline bool gTrackRankGiven = false;  // --forward-rank K : with --forward-track, the K best of every set by the ranked query over the track's p after the create and after every batch (dppr_ftrack_topk_ranked; under --rank-factor / --rank-exclude if given)
inline int gTrackRank = 0;
inline int gForwardTopK = 5;          // --forward-topk K (0 <= K <= 64: 0 prints no vertex)
inline int gSample = 0;               // --sample S : after every batch print one sample line per source (S draws in proportion to its score)
inline bool gSampleGiven = false;
inline bool gSampleSeedGiven = false;
inline unsigned long long gSampleSeed = 0; // --sample-seed X
inline int gWalks = 0;                // --walks W : walks per refined vertex (with --refine)
inline bool gWalksGiven = false;
inline unsigned long long gWalkSeed = 0; // --walk-seed S
inline int gClusterK = 0;             // --cluster K : after every batch print cluster <source> size <n> cut <c> vol <v> phi <phi>, the best prefix of the top-K order (0: off)
inline bool gClusterGiven = false;
inline double gClusterMin = 0.0;      // --cluster-min P : the order holds the vertices with pagerank > P
inline int gClusterMinSize = 1;       // --cluster-min-size M : the smallest prefix that may be the cluster
inline bool gClusterOptsGiven = false; //   --cluster-min or --cluster-min-size was given
inline int gSubgraphK = 0;            // --subgraph K : after every batch print subgraph <source> vertices <L> edges <m>, the top-K order and the stored edges among it (0: off)
inline bool gSubgraphGiven = false;
inline std::string gSubgraphOut;      // --subgraph-out FILE : ... and write the CSR of the last batch, text lines `v source position id pagerank` and `e source tail head`
inline bool gAssign = false;          // --assign : after every batch print assign <batch> classes=<C> unassigned=<n> flips=<n> counts=c0,c1,.. (dppr_assign over this device's groups)
inline double gAssignMin = 0.0;       // --assign-min S : a class labels a vertex only with a score > S
inline bool gAssignMinGiven = false;
inline std::string gAssignOut;        // --assign-out FILE : ... and write the last labels, raw int32 [V]
inline bool gValidate = false;        // --validate : the reference's -DVALIDATE checks at run time
inline bool gShareDevice = false;     // --share-device (or DPPR_DEVICE_ALIAS=1): the -g N device threads share the devices that exist (d % count)
inline bool gPushOnly = false;        // --push-only : no pull sweeps (the ablation of the -o variants times their push mechanisms)
inline bool gMergePhases = false;     // --merge-phases : one loop for residuals of both signs, to eps / 4 (dppr_set_phase_merge; off: the reference's two loops)
inline bool gSplitInterface = false;  // --split : drive the timed region through the 3 virtual calls
inline int gSchedule = 0;             // --sync : deterministic synchronous schedule
inline bool gProfile = false;         // --profile : the reference's -DPROFILE output (per-iteration frontier lines, phase times)
inline bool gNoGroups = false;        // --no-groups : solve several sources one at a time instead of up to 16 together
