// sufr_lz_scan.h -- the arithmetic behind the longest previous factor and the LZ77 parse (include/sufr_lz.h, DESIGN.md
// section 20): the range minimum over a min pyramid, the decision of one rank (its two neighbours with a smaller text
// position, the two minima, the clip and the tie rule) and the packed entry of the parse tables.  Plain integer code that
// the kernels of sufr_lz.inc, the host path of sufr_query.cpp and tests/lz_shim.cpp all compile (SUFR_HD, the way of
// sufr_repeat_scan.h); there is no second copy of it.
//
// The pyramids are those of sufr_repeat_scan.h (fan-out 64, rep_level_size, rep_level_offset), built twice: over the
// suffix array's values, where rep_search_left / rep_search_right find the nearest rank on either side whose suffix starts
// earlier in the text, and over the raw LCP array -- not the clipped l of section 19; the two differ where sequence starts
// are positional only -- where lz_range_min answers min LCP[lo, hi).  Level 0 of either is the array itself, with no copy.
// An accessor is that of the searches: acc.at(0, 0, i) is entry i of the array, acc.at(k, off, i) entry i of level k >= 1.
#pragma once
#include <stdint.h>

#include "sufr_repeat_scan.h"

namespace sufr {

static constexpr uint64_t LZ_NONE = ~(uint64_t)0;       // no source: LPF is 0

// the minimum of entries [lo, hi) of level 0, ~0 when lo >= hi.  At every level the part of the range before the first and
// after the last 64-block boundary is scanned (at most 63 entries each), and the whole blocks between them are their
// parents' range one level up: at most 2 x 64 reads per level whatever hi - lo is.
template <typename A>
SUFR_HD uint64_t lz_range_min(const A& acc, uint64_t s, uint64_t lo, uint64_t hi)
{
    uint64_t m = ~(uint64_t)0, off = 0;                  // off: where level lev begins (levels >= 1)
    uint32_t lev = 0;
    while (lo < hi) {
        const uint64_t le = (lo + 63) & ~(uint64_t)63, hb = hi & ~(uint64_t)63;
        if (le >= hb || rep_level_size(s, lev) <= 64) {  // no whole block between them, or the top level: it has no parent
            for (uint64_t j = lo; j < hi; j++) { const uint64_t x = acc.at(lev, off, j); if (x < m) m = x; }
            break;
        }
        for (uint64_t j = lo; j < le; j++) { const uint64_t x = acc.at(lev, off, j); if (x < m) m = x; }
        for (uint64_t j = hb; j < hi; j++) { const uint64_t x = acc.at(lev, off, j); if (x < m) m = x; }
        lo = le >> 6; hi = hb >> 6;
        if (lev) off += rep_level_size(s, lev);
        lev++;
    }
    return m;
}

struct LzEntry { uint64_t lpf, src; };

// The decision of one position of room d(p): has1 / has2 say whether j1 / j2 exist, m1 / m2 are the minima and q1 / q2 the
// text positions SA[j1] / SA[j2].  The one place where the clip and the tie rule (m1 >= m2 -> j1) are written down.
SUFR_HD LzEntry lz_pick(bool has1, uint64_t m1, uint64_t q1, bool has2, uint64_t m2, uint64_t q2, uint64_t room)
{
    if (!has1 && !has2) return LzEntry{0, LZ_NONE};
    const bool first = has1 && (!has2 || m1 >= m2);
    uint64_t m = first ? m1 : m2;
    if (m > room) m = room;
    if (!m) return LzEntry{0, LZ_NONE};
    return LzEntry{m, first ? q1 : q2};
}

// LPF and SRC of p = SA[r].  sa: the accessor over the suffix array's values and their min pyramid; lcp: the one over the
// raw LCP and its min pyramid.  Two searches and two range minima, each bounded by 2 x 64 x levels reads.
template <typename S, typename L>
SUFR_HD LzEntry lz_rank(const S& sa, const L& lcp, uint64_t s, uint64_t r, uint64_t p, uint64_t room)
{
    if (!room) return LzEntry{0, LZ_NONE};               // (a break position: whatever the neighbours say, the clip leaves 0)
    bool has1 = false, has2 = false;
    uint64_t m1 = 0, m2 = 0, q1 = 0, q2 = 0;
    if (p) {                                             // SA[j] < p as SA[j] <= p - 1
        const uint64_t j1 = rep_search_left(sa, s, r, p - 1);
        if (j1 != REP_NONE) { has1 = true; q1 = sa.at(0, 0, j1); m1 = lz_range_min(lcp, s, j1 + 1, r + 1); }
    }
    const uint64_t j2 = rep_search_right(sa, s, r, p);
    if (j2 < s) { has2 = true; q2 = sa.at(0, 0, j2); m2 = lz_range_min(lcp, s, r + 1, j2 + 1); }
    return lz_pick(has1, m1, q1, has2, m2, q2, room);
}

// the length of the factor that starts at a position of that LPF
SUFR_HD uint64_t lz_step(uint64_t lpf) { return lpf ? lpf : 1; }

// An entry of the parse table of a tile: the last in-tile position on the chain from this one (tile-relative, below 2^16)
// and the hops to it.
SUFR_HD uint32_t lz_tab_pack(uint32_t last, uint32_t hops) { return last | (hops << 16); }
SUFR_HD uint32_t lz_tab_last(uint32_t e) { return e & 0xFFFFu; }
SUFR_HD uint32_t lz_tab_hops(uint32_t e) { return e >> 16; }

}  // namespace sufr
