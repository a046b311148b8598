// sufr_shared_scan.h -- the arithmetic behind the sequence counts of repeats and the k-common substrings
// (include/sufr_shared.h): the sequence of a text position, the sort key of a rank, the decision of
// one pair (prev[r], r) and the count of an interval from the prefix sums.  Plain integer code that the kernels of
// sufr_shared.inc, the host path of sufr_query.cpp and tests/shared_shim.cpp all compile (SUFR_HD, the way of
// sufr_lz_scan.h); there is no second copy of it.
//
// The pyramid is that of sufr_repeat_scan.h over the clipped LCP l; an accessor is that of its searches.  A pair costs one
// lz_range_min and one rep_search_right, each bounded by 2 x 64 x levels reads however far apart its two ranks are.
#pragma once
#include <stdint.h>

#include "sufr_lz_scan.h"

namespace sufr {

static constexpr uint32_t SHR_RANK_BITS = 40;           // a sort key is doc << 40 | rank
static constexpr uint32_t SHR_DOC_BITS = 24;

// doc(p): the index of the last sequence start <= p (starts ascending from 0; num <= 1: one sequence)
SUFR_HD uint64_t shr_doc(const uint64_t* starts, uint64_t num, uint64_t p)
{
    if (num <= 1) return 0;
    uint64_t a = 1, b = num;                             // the first i with starts[i] > p (starts[0] = 0 <= p)
    while (a < b) {
        const uint64_t m = a + (b - a) / 2;
        if (starts[m] > p) b = m; else a = m + 1;
    }
    return a - 1;
}

SUFR_HD uint64_t shr_key(uint64_t doc, uint64_t r) { return (doc << SHR_RANK_BITS) | r; }
SUFR_HD uint64_t shr_key_doc(uint64_t key) { return key >> SHR_RANK_BITS; }
SUFR_HD uint64_t shr_key_rank(uint64_t key) { return key & (((uint64_t)1 << SHR_RANK_BITS) - 1); }

// the key bits above the rank that vary: bits(num - 1)
SUFR_HD uint32_t shr_doc_bits(uint64_t num)
{
    uint32_t b = 0;
    while (num > 1 && ((num - 1) >> b)) b++;
    return b;
}

// q(r) of the pair (prev, r), prev < r < s: the smallest j in (prev, r] with l[j] == min l(prev, r]
template <typename A>
SUFR_HD uint64_t shr_pair(const A& acc, uint64_t s, uint64_t prev, uint64_t r)
{
    const uint64_t m = lz_range_min(acc, s, prev + 1, r + 1);
    return rep_search_right(acc, s, prev, m + 1);        // (the first l[j] <= m: none is smaller, so it is == m, and j <= r)
}

// seqs([a, b)) from the exclusive prefix P of H (s + 1 entries)
template <typename P>
SUFR_HD uint64_t shr_seqs(const P* prefix, uint64_t a, uint64_t b) { return (b - a) - ((uint64_t)prefix[b] - (uint64_t)prefix[a + 1]); }

// min_seqs <= seqs <= max_seqs (min_seqs 0 means 1 and filters nothing; max_seqs 0: off)
SUFR_HD bool shr_keep(uint64_t seqs, uint64_t min_seqs, uint64_t max_seqs) { return seqs >= min_seqs && (!max_seqs || seqs <= max_seqs); }

}  // namespace sufr
