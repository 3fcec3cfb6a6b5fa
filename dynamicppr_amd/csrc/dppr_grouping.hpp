// dppr_grouping.hpp -- which implementation groups a batch's L records by tail for IncrementalBatchUpdate (dppr_update.hpp kernels,
// enqueue_grouping in dppr_host_loop.hpp). Pure host code: the engine calls it when a batch is uploaded and when the grouping is
// enqueued; tests/native/grouping_test.cpp drives it on the CPU.
//
// The contract every path keeps: equal tails are contiguous, and the records of one tail are in batch order. The order of the
// TAILS depends on the path -- ascending for rank, radix and at-slide; for bucket, bucket by bucket (tail & (nb - 1)), ascending
// inside a bucket. A consumer may find a tail's run by comparing neighbours, not by bisecting the whole array.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace dppr {

// rank  : k_su_group_rank, one launch, every record compared with every record (L^2)
// bucket: k_su_grp_hist / _scatter / _rank, nb low-bit buckets, every record compared with the records of its bucket
// radix : k_su_keys + the device radix sort (beyond SU_GRP_MAX_RECORDS, a bucket above SU_GRP_MAX_BUCKET, or DPPR_GROUPING_RADIX=1)
// at slide: epoch_group_records, the device radix sort when the batch is uploaded (dppr_set_batch_grouping(1))
enum GroupingPath { GROUPING_AUTO = 0, GROUPING_RANK = 1, GROUPING_BUCKET = 2, GROUPING_RADIX = 3, GROUPING_AT_SLIDE = 4 };

constexpr int SU_RANK_MAX = 4096;
constexpr int SU_GRP_MAX_BUCKETS = 4096, SU_GRP_MAX_RECORDS = 1 << 22;
// The ranking launch of the bucket path costs every record of a bucket the size of that bucket: a bucket of more records than this
// (one hot tail -- low bits cannot split it -- or several that share their low bits) sends the batch to the radix sort instead.
// With it the ranking does at most SU_GRP_MAX_BUCKET comparisons per record.
constexpr int SU_GRP_MAX_BUCKET = 1 << 14;

// Buckets of the bucket path for L records: the first power of two from 64 on with nb * 512 >= L, at most SU_GRP_MAX_BUCKETS.
inline int grouping_buckets(int L) {
    int nb = 64;
    while (nb < SU_GRP_MAX_BUCKETS && (long long)nb * 512 < L) nb *= 2;
    return nb;
}

// Records in the fullest bucket of the bucket path for these (internal) tails; 0 for a batch the bucket path does not take by length.
inline int largest_bucket(const int32_t *tails, int L) {
    if (L <= SU_RANK_MAX || L > SU_GRP_MAX_RECORDS) return 0;
    const int nb = grouping_buckets(L);
    std::vector<int> h((size_t)nb, 0);
    for (int i = 0; i < L; ++i) h[(size_t)(tails[i] & (nb - 1))]++;
    return *std::max_element(h.begin(), h.end());
}

// The path the timed region runs for a batch that was not grouped at slide.
inline GroupingPath grouping_path(int L, int max_bucket, bool force_radix) {
    if (force_radix) return GROUPING_RADIX;
    if (L <= SU_RANK_MAX) return GROUPING_RANK;
    if (L <= SU_GRP_MAX_RECORDS && max_bucket <= SU_GRP_MAX_BUCKET) return GROUPING_BUCKET;
    return GROUPING_RADIX;
}

} // namespace dppr
