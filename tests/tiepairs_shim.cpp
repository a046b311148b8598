// Host-side shim around sufr_amd/csrc/sufr_tiepairs.h (the tie-pair masks of the pair path in front of the tie level), so that
// tests/test_tiepairs_cpu.py can hold the very code the kernels run to a brute-force scan of the bit strings, without a GPU.
#include <stddef.h>
#include "../sufr_amd/csrc/sufr_tiepairs.h"

// wmask: nwin windows of four words (M0 M1 H0 H1), the layout of the tie bitmaps; out: two words per window, a bit per slot
// that heads a run of exactly two.  Returns the number of such slots.
extern "C" uint64_t shim_tie_pair_heads(const uint64_t* wmask, uint32_t nwin, uint64_t* out)
{
    uint64_t total = 0;
    for (uint32_t w = 0; w < nwin; w++) {
        const uint64_t* m = wmask + (size_t)w * 4;
        const uint32_t next = w + 1 < nwin ? sufr::tie_next_bits(m[4], m[6]) : 0u;
        const sufr::TieMask128 p = sufr::tie_pair_heads(m[0], m[1], m[2], m[3], next);
        out[(size_t)w * 2] = p.lo; out[(size_t)w * 2 + 1] = p.hi;
        total += sufr::tie_mask_count(p);
    }
    return total;
}
