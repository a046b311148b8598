// sufr_tiepairs.h -- tie pairs in the tie bitmaps, shared by the device kernels and the host-side unit test.
// The leaf sorts describe tie runs (equal whole keys) by two bits per output position, 128 positions per window: member (M0 M1)
// and run head (H0 H1).  A run is a head and the members without a head bit that follow it; it may cross a window's end -- the
// member in slot 0 of the next window then has no head bit.  A tie PAIR is a run of exactly two members.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SUFR_TP_HD __host__ __device__ __forceinline__
#else
#define SUFR_TP_HD static inline
#endif

namespace sufr {

struct TieMask128 { uint64_t lo, hi; };      // a bit per slot of a window: slots 0-63, 64-127

// "continues a run": a member that is not a head
SUFR_TP_HD TieMask128 tie_continues(uint64_t M0, uint64_t M1, uint64_t H0, uint64_t H1)
{
    return TieMask128{M0 & ~H0, M1 & ~H1};
}

// The first two slots of the next window, as tie_pair_heads wants them: bit 0 / 1 set when slot 0 / 1 of that window continues a
// run.  (No next window: 0.)
SUFR_TP_HD uint32_t tie_next_bits(uint64_t nextM0, uint64_t nextH0)
{
    return (uint32_t)((nextM0 & ~nextH0) & 3ull);
}

// The slots of this window that head a run of exactly two: a head whose successor continues the run and whose successor's
// successor does not.  `next`: tie_next_bits of the window behind this one.
SUFR_TP_HD TieMask128 tie_pair_heads(uint64_t M0, uint64_t M1, uint64_t H0, uint64_t H1, uint32_t next)
{
    const TieMask128 T = tie_continues(M0, M1, H0, H1);
    const uint64_t n0 = (uint64_t)(next & 1u), n1 = (uint64_t)((next >> 1) & 1u);
    const uint64_t T1lo = (T.lo >> 1) | (T.hi << 63), T1hi = (T.hi >> 1) | (n0 << 63);                  // slot + 1 continues
    const uint64_t T2lo = (T.lo >> 2) | (T.hi << 62), T2hi = (T.hi >> 2) | (n0 << 62) | (n1 << 63);     // slot + 2 continues
    return TieMask128{M0 & H0 & T1lo & ~T2lo, M1 & H1 & T1hi & ~T2hi};
}

SUFR_TP_HD uint32_t tie_mask_count(TieMask128 m)
{
    return (uint32_t)(__builtin_popcountll(m.lo) + __builtin_popcountll(m.hi));
}

}  // namespace sufr
