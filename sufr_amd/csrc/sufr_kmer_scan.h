// sufr_kmer_scan.h -- the segmented count behind the k-mer spectra and occurrence maps (include/sufr_kmer.h, DESIGN.md
// section 18): the summary of a stretch of ranks, its combine operator, the carries between stretches and the count of one
// rank of a 64-rank word.  Plain integer code that the kernels of sufr_kmer.inc, the host path of sufr_query.cpp and
// tests/kmer_shim.cpp all compile (SUFR_HD, the way of sufr_trace.h and sufr_runkey.h); there is no second copy of it.
//
// Every rank carries two flags: head (rank 0, or LCP[r] < k: a k-interval begins here) and whole (its k-mer crosses no
// break).  The count of a rank is the number of whole ranks between the last head at or before it and the next head after
// it.  A stretch of consecutive ranks is summarised by
//   has    it holds a head
//   pre    whole ranks before its first head (all of its whole ranks when it holds none)
//   post   whole ranks from its last head on (all of its whole ranks when it holds none)
// and two adjacent stretches combine into the summary of their union.  The operator is associative with KmerSum{0, 0, 0}
// as its identity, so summaries can be folded in any grouping: 64 ranks to a word, words to a tile, tiles to the array.
// What a stretch needs from outside is two numbers: carry_in, the whole ranks of the interval that is open at its start,
// and carry_out, the whole ranks after its end up to the next head.
#pragma once
#include <stdint.h>

#ifndef SUFR_HD
#if defined(__HIPCC__)
#define SUFR_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SUFR_HD static inline
#endif
#endif
// SUFR_HD for a member function defined in its class (there `static` would mean something else, and `inline` is implied)
#ifndef SUFR_HD_MEMBER
#if defined(__HIPCC__)
#define SUFR_HD_MEMBER __host__ __device__ inline __attribute__((always_inline))
#else
#define SUFR_HD_MEMBER
#endif
#endif

namespace sufr {

struct KmerSum { uint64_t pre, post; uint32_t has; };

SUFR_HD KmerSum kmer_identity() { return KmerSum{0, 0, 0}; }

// the summary of stretch a followed by stretch b
SUFR_HD KmerSum kmer_combine(const KmerSum& a, const KmerSum& b)
{
    KmerSum c;
    c.has = a.has | b.has;
    c.pre = a.has ? a.pre : a.pre + b.pre;
    c.post = b.has ? b.post : a.post + b.pre;          // (b without a head: b.pre is all of its whole ranks)
    return c;
}

// up to 64 consecutive ranks as two masks, bit i = rank i, bits beyond the ranks clear: H heads, W whole ranks
SUFR_HD KmerSum kmer_word_sum(uint64_t H, uint64_t W)
{
    if (!H) { const uint64_t c = (uint64_t)__builtin_popcountll(W); return KmerSum{c, c, 0}; }
    const int first = __builtin_ctzll(H), last = 63 - __builtin_clzll(H);
    return KmerSum{(uint64_t)__builtin_popcountll(W & (((uint64_t)1 << first) - 1)), (uint64_t)__builtin_popcountll(W >> last), 1};
}

// `before`: everything between the start of an enclosing stretch and this one; outer: the carry_in of the enclosing stretch
SUFR_HD uint64_t kmer_carry_in(const KmerSum& before, uint64_t outer) { return before.has ? before.post : before.post + outer; }
// `after`: everything between the end of this stretch and the end of the enclosing one; outer: the enclosing carry_out
SUFR_HD uint64_t kmer_carry_out(const KmerSum& after, uint64_t outer) { return after.has ? after.pre : after.pre + outer; }

// the whole ranks of the interval that holds rank i of a word (its count when it is whole; the count of the k-mer when it
// is a head), given the carries of the word
SUFR_HD uint64_t kmer_rank_count(uint64_t H, uint64_t W, uint32_t i, uint64_t carry_in, uint64_t carry_out)
{
    const uint64_t upto = i >= 63 ? ~(uint64_t)0 : (((uint64_t)2 << i) - 1);        // ranks 0 .. i
    const uint64_t hb = H & upto, ha = H & ~upto;
    uint64_t c;
    if (hb) c = (uint64_t)__builtin_popcountll(W & upto & ~(((uint64_t)1 << (63 - __builtin_clzll(hb))) - 1));
    else c = carry_in + (uint64_t)__builtin_popcountll(W & upto);
    if (ha) c += (uint64_t)__builtin_popcountll(W & ~upto & (((uint64_t)1 << __builtin_ctzll(ha)) - 1));
    else c += carry_out + (uint64_t)__builtin_popcountll(W & ~upto);
    return c;
}

// brk(p): the smallest break >= p.  Breaks are starts[i] - 1 for i >= 1 and n - 1; starts ascending from 0 (num <= 1: one
// sequence).  p < n.
SUFR_HD uint64_t kmer_brk(const uint64_t* starts, uint64_t num, uint64_t n, uint64_t p)
{
    if (num <= 1) return n - 1;
    uint64_t a = 1, b = num;                             // the first i with starts[i] > p (starts[0] = 0 <= p)
    while (a < b) {
        const uint64_t m = a + (b - a) / 2;
        if (starts[m] > p) b = m; else a = m + 1;
    }
    return a < num ? starts[a] - 1 : n - 1;
}

// whole: p + k <= brk(p), without the sum (k is any u64)
SUFR_HD bool kmer_whole(const uint64_t* starts, uint64_t num, uint64_t n, uint64_t p, uint64_t k)
{
    return kmer_brk(starts, num, n, p) - p >= k;
}

// the bin of a k-mer of count c >= 1
SUFR_HD uint64_t kmer_bin(uint64_t c, uint64_t bins) { return (c < bins ? c : bins) - 1; }

}  // namespace sufr
