// sufr_bwt_scan.h -- the arithmetic behind the BWT of the indexed text, its runs and the LF mapping (include/sufr_bwt.h,
// DESIGN.md section 22): where the byte of a rank comes from, the summary of a tile of ranks, the carry that tells a tile
// how far its open run goes on beyond its end, and the length and the filter of a run.  The longest run is chosen by
// rep_better of sufr_repeat_scan.h on (length, rank): longer wins, ties go to the smaller rank.  Plain integer code that
// the kernels of sufr_bwt.inc and the host path of sufr_query.cpp both compile (SUFR_HD, the way of sufr_lz_scan.h); there
// is no second copy of it.
//
// Tiles.  The ranks are cut into tiles of a fixed size (the last may be shorter).  A run is reported by the tile that holds
// its head; the only thing such a tile cannot see is how far the run that is open at its right end goes on.  That is the
// carry: ext[t], the ranks beyond the end of tile t that continue its last run.  With the summaries (first, last, pre, suf)
// of the tiles -- pre / suf: the length of the run at the left / right end, both the tile's length where it is one run --
//     ext[t] = 0                                   where t is the last tile or last[t] != first[t + 1]
//            = pre[t + 1]                          where tile t + 1 is not one whole run
//            = pre[t + 1] + ext[t + 1]             where it is,
// that is ext[t] = add + pass * ext[t + 1] with pass 0 or 1 (BwtLink).  Links compose (bwt_chain), so a sweep from the last
// tile to the first may take many tiles at a time as a scan; a run may cover any number of whole tiles.
#pragma once
#include <stdint.h>

#include "sufr_repeat_scan.h"

namespace sufr {

// the text position of BWT[r] for p = SA[r] (cyclic at the text's start)
SUFR_HD uint64_t bwt_source(uint64_t p, uint64_t n) { return p ? p - 1 : n - 1; }

// a min_len of 0 counts as 1
SUFR_HD uint64_t bwt_min_len(uint64_t min_len) { return min_len ? min_len : 1; }

// x -> add + pass * x, pass 0 or 1
struct BwtLink { uint64_t add, pass; };

// what tile t + 1 (first symbol, pre, length) gives the run that is open at the end of a tile whose last symbol is `last`
SUFR_HD BwtLink bwt_link(uint32_t last, uint32_t next_first, uint64_t next_pre, uint64_t next_len)
{
    if (last != next_first) return BwtLink{0, 0};
    return BwtLink{next_pre, next_pre == next_len ? (uint64_t)1 : 0};
}

// near(far(x)): `near` is the link of the tile nearer to the start of the array
SUFR_HD BwtLink bwt_chain(const BwtLink& near, const BwtLink& far) { return BwtLink{near.add + near.pass * far.add, near.pass * far.pass}; }

// The length of the run whose head is at tile-relative rank i: next is the tile-relative rank of the next head in the tile,
// len (the tile's length) where there is none; only then the run goes on beyond the tile, by ext.
SUFR_HD uint64_t bwt_run_length(uint64_t i, uint64_t next, uint64_t len, uint64_t ext) { return next - i + (next == len ? ext : 0); }

}  // namespace sufr
