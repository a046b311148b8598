// sufr_repeat_scan.h -- the arithmetic behind the repeats of the indexed text (include/sufr_repeat.h):
// the clipped LCP, the index arithmetic of a min pyramid over it, the two nearest-smaller-value searches that walk the
// pyramid, the decision "is this rank the representative of an interval, and of which" (rep_interval), the popcount-prefix
// count of flagged ranks, the supermaximal walk and the reduction of a find pass's candidates (RepBest).  Plain integer
// code that the kernels of sufr_repeat.inc, the host path of sufr_query.cpp and tests/repeat_shim.cpp all compile (SUFR_HD,
// the way of sufr_kmer_scan.h); there is no second copy of it.
//
// The pyramid.  Level 0 is l[0..s), the clipped LCP.  Entry i of level k >= 1 is the minimum of entries [64 i, 64 i + 64) of
// level k - 1, so level k has ceil(s / 64^k) entries; levels are kept while the one below has more than 64 entries, and the
// levels 1, 2, ... lie one after the other in one array.  A search for the nearest entry left (right) of rank r that is
// <= v (< v) scans the rest of r's 64-block, then climbs: at every level it scans the rest of the parent's block, until an
// entry qualifies (some rank below it does, and everything between it and r does not) or the array ends; then it descends
// into the qualifying child that is nearest to r, level by level.  It reads at most 64 entries per level on the way up and
// 64 on the way down: the cost of one search is bounded by 2 x 64 x levels, whatever the distance to the answer.
//
// An accessor `acc` gives the searches their data: acc.at(0, 0, i) is l[i], acc.at(k, off, i) entry i of level k >= 1, where
// off = rep_level_offset(s, k) is where that level begins in the array of the coarser levels (a search computes it once per
// level, not per read), and acc.sa(r) the suffix array (the supermaximal walk only).
#pragma once
#include <stdint.h>

#include "sufr_kmer_scan.h"

namespace sufr {

static constexpr uint64_t REP_NONE = ~(uint64_t)0;      // rep_search_left: nothing qualifies
static constexpr uint32_t REP_LAMBDA_MAX = 256;         // different left symbols that are bytes: a supermaximal repeat has no more non-start occurrences

// d(p) = brk(p) - p: the symbols from p on that a repeat may cover
SUFR_HD uint64_t rep_room(const uint64_t* starts, uint64_t num, uint64_t n, uint64_t p) { return kmer_brk(starts, num, n, p) - p; }

// l[r] for r >= 1, from LCP[r] and the rooms of SA[r-1] and SA[r]
SUFR_HD uint64_t rep_clip(uint64_t lcp, uint64_t room_prev, uint64_t room_cur)
{
    const uint64_t m = room_prev < room_cur ? room_prev : room_cur;
    return lcp < m ? lcp : m;
}

// p begins a sequence: its left symbol is one of its own (p == 0, or p - 1 is a break)
SUFR_HD bool rep_is_start(const uint64_t* starts, uint64_t num, uint64_t n, uint64_t p)
{
    if (p == 0) return true;
    if (num <= 1) return false;
    return kmer_brk(starts, num, n, p - 1) == p - 1;
}

// entries of level k: ceil(s / 64^k)
SUFR_HD uint64_t rep_level_size(uint64_t s, uint32_t k)
{
    const uint32_t sh = 6 * k;
    if (sh >= 64) return s ? 1 : 0;
    return (s >> sh) + ((s & (((uint64_t)1 << sh) - 1)) ? 1 : 0);
}

// the number of levels above level 0
SUFR_HD uint32_t rep_levels(uint64_t s)
{
    uint32_t k = 0;
    while (rep_level_size(s, k) > 64) k++;
    return k;
}

// where level k >= 1 begins in the array of the coarser levels; rep_level_offset(s, rep_levels(s) + 1) is its length
SUFR_HD uint64_t rep_level_offset(uint64_t s, uint32_t k)
{
    uint64_t off = 0;
    for (uint32_t j = 1; j < k; j++) off += rep_level_size(s, j);
    return off;
}

// the largest j < r with l[j] <= v, or REP_NONE
template <typename A>
SUFR_HD uint64_t rep_search_left(const A& acc, uint64_t s, uint64_t r, uint64_t v)
{
    uint64_t pos = r, j = 0, off = 0;                    // off: where level lev begins (levels >= 1)
    uint32_t lev = 0;
    for (;;) {                                           // up: entries [block start, pos) of level lev, nearest first
        const uint64_t base = pos & ~(uint64_t)63;
        bool found = false;
        for (j = pos; j > base;) {
            j--;
            if (acc.at(lev, off, j) <= v) { found = true; break; }
        }
        if (found) break;
        if (base == 0) return REP_NONE;
        pos = base >> 6;                                 // the parent of this block: its left siblings are next
        if (lev) off += rep_level_size(s, lev);
        lev++;
    }
    while (lev > 0) {                                    // down: the last qualifying child
        lev--;
        const uint64_t lo = j << 6, n = rep_level_size(s, lev);
        if (lev) off -= n;
        j = lo + 64 < n ? lo + 64 : n;
        while (j > lo) {
            j--;
            if (acc.at(lev, off, j) <= v) break;
        }
    }
    return j;
}

// the smallest j > r with l[j] < v, or s
template <typename A>
SUFR_HD uint64_t rep_search_right(const A& acc, uint64_t s, uint64_t r, uint64_t v)
{
    uint64_t pos = r, j = 0, off = 0;                    // off: where level lev begins (levels >= 1)
    uint32_t lev = 0;
    for (;;) {                                           // up: entries (pos, block end) of level lev, nearest first
        const uint64_t n = rep_level_size(s, lev), base = pos & ~(uint64_t)63, end = base + 64 < n ? base + 64 : n;
        bool found = false;
        for (j = pos + 1; j < end; j++)
            if (acc.at(lev, off, j) < v) { found = true; break; }
        if (found) break;
        if (end == n) return s;
        pos = base >> 6;
        if (lev) off += n;
        lev++;
    }
    while (lev > 0) {                                    // down: the first qualifying child
        lev--;
        const uint64_t n = rep_level_size(s, lev), hi = (j << 6) + 64 < n ? (j << 6) + 64 : n;
        if (lev) off -= n;
        for (j <<= 6; j + 1 < hi; j++)
            if (acc.at(lev, off, j) < v) break;
    }
    return j;
}

// flagged ranks among [0, x): words holds one bit per rank, prefix[i] the flagged ranks before word i
SUFR_HD uint64_t rep_rank(const uint64_t* words, const uint64_t* prefix, uint64_t x)
{
    if (!x) return 0;
    const uint64_t i = (x - 1) >> 6;
    const uint32_t m = (uint32_t)((x - 1) & 63) + 1;     // 1 .. 64 bits of word i
    return prefix[i] + (uint64_t)__builtin_popcountll(words[i] & (m == 64 ? ~(uint64_t)0 : (((uint64_t)1 << m) - 1)));
}

// flagged ranks among [lo, hi)
SUFR_HD uint64_t rep_flagged(const uint64_t* words, const uint64_t* prefix, uint64_t lo, uint64_t hi)
{
    return hi > lo ? rep_rank(words, prefix, hi) - rep_rank(words, prefix, lo) : 0;
}

// some rank in (a, b) differs from its predecessor in the left symbol (dw, dp: the "differs from the previous rank" flags)
SUFR_HD bool rep_left_diverse(const uint64_t* dw, const uint64_t* dp, uint64_t a, uint64_t b) { return rep_flagged(dw, dp, a + 1, b) > 0; }

// [a, b) of value v is supermaximal: l[j] == v inside it and the left symbols of its occurrences are pairwise different.
// sw, sp: the "is a sequence start" flags.  Two refusals cost no walk: neighbours that share a left symbol, and more than
// 256 occurrences that are not sequence starts (their left symbols are bytes).  Otherwise the ranks are walked, up to the
// first l[j] != v or the first repeated byte: at most 257 ranks that are not sequence starts, plus the sequence starts
// between them -- a text of many identical whole sequences makes this walk as long as their number.
template <typename A>
SUFR_HD bool rep_supermaximal(const A& acc, const uint8_t* text, const uint64_t* dw, const uint64_t* dp, const uint64_t* sw,
                              const uint64_t* sp, uint64_t a, uint64_t b, uint64_t v)
{
    const uint64_t count = b - a;
    if (rep_flagged(dw, dp, a + 1, b) != count - 1) return false;
    if (count - rep_flagged(sw, sp, a, b) > REP_LAMBDA_MAX) return false;
    uint64_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;             // the bytes seen
    for (uint64_t j = a; j < b; j++) {
        if (j > a && acc.at(0, 0, j) != v) return false;
        if ((sw[j >> 6] >> (j & 63)) & 1) continue;
        const uint32_t c = text[acc.sa(j) - 1], q = c >> 6;
        const uint64_t bit = (uint64_t)1 << (c & 63);
        const uint64_t have = q == 0 ? s0 : q == 1 ? s1 : q == 2 ? s2 : s3;
        if (have & bit) return false;
        s0 |= q == 0 ? bit : 0; s1 |= q == 1 ? bit : 0; s2 |= q == 2 ? bit : 0; s3 |= q == 3 ? bit : 0;
    }
    return true;
}

// the kind and count filters of one interval [a, b) of value v (v >= min_len is checked before the searches)
template <typename A>
SUFR_HD bool rep_keep(const A& acc, const uint8_t* text, const uint64_t* dw, const uint64_t* dp, const uint64_t* sw, const uint64_t* sp,
                      uint32_t kind, uint64_t min_count, uint64_t max_count, uint64_t a, uint64_t b, uint64_t v)
{
    const uint64_t count = b - a;
    if (count < min_count || (max_count && count > max_count)) return false;
    if (kind == 0) return true;
    if (kind == 1) return rep_left_diverse(dw, dp, a, b);
    return rep_supermaximal(acc, text, dw, dp, sw, sp, a, b, v);
}

// If rank r, 1 <= r < s, is the representative of an interval of value v = l[r] >= min_len -- the nearest l <= v on its left
// is smaller (an equal one is an earlier rank of the same interval, and the representative) -- then fn(a, z, v) with that
// interval [a, z).  What is done with an interval is a callable and not code behind a returned flag so that in a kernel it
// stays inside the branch that found the interval: behind a flag the lanes of a wave meet again first, and the writing
// form of k_rep_find was 4 % slower for it.
template <typename A, typename F>
SUFR_HD void rep_interval(const A& acc, uint64_t s, uint64_t r, uint64_t min_len, F fn)
{
    const uint64_t v = acc.at(0, 0, r);
    if (v >= min_len) {
        const uint64_t a = rep_search_left(acc, s, r, v);
        if (a != REP_NONE && acc.at(0, 0, a) < v) fn(a, rep_search_right(acc, s, r, v), v);
    }
}

// out[i] = min of in[64 i .. 64 i + 64): one coarser level of a pyramid, serially (the device has k_rep_level)
SUFR_HD void rep_level_up(const uint64_t* in, uint64_t n_in, uint64_t* out, uint64_t n_out)
{
    for (uint64_t i = 0; i < n_out; i++) {
        uint64_t low = ~(uint64_t)0;
        for (uint64_t j = i * 64; j < n_in && j < i * 64 + 64; j++) if (in[j] < low) low = in[j];
        out[i] = low;
    }
}

// the better of two "longest" candidates (len, rep): longer wins, ties go to the smaller representative; len 0: none
SUFR_HD bool rep_better(uint64_t len, uint64_t rep, uint64_t than_len, uint64_t than_rep)
{
    return len > than_len || (len == than_len && len && rep < than_rep);
}

// what a find pass keeps of the intervals it met: the longest (len, its representative, its first rank), the largest count
// and the largest number of sequences (0 where the call has no such column).  All zero: nothing met.  merge is commutative
// and associative -- rep_better is a strict order on (len, rep) and the other two are maxima -- so lanes, waves, tiles and
// chunks may be combined in any order.
struct RepBest {
    uint64_t len, rep, rank, cnt, seq;
    SUFR_HD_MEMBER void merge(const RepBest& o)
    {
        if (rep_better(o.len, o.rep, len, rep)) { len = o.len; rep = o.rep; rank = o.rank; }
        if (o.cnt > cnt) cnt = o.cnt;
        if (o.seq > seq) seq = o.seq;
    }
    // the interval [a, a + count) of value v with representative r, seen in `seqs` sequences
    SUFR_HD_MEMBER void take(uint64_t v, uint64_t r, uint64_t a, uint64_t count, uint64_t seqs) { merge(RepBest{v, r, a, count, seqs}); }
};

}  // namespace sufr
