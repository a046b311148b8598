// Host-side shim around sufr_amd/csrc/sufr_trace.h (the banded rows and the walk the trace kernels run per lane), so that the
// device's arithmetic can be held to a full-table witness on the CPU.  Test infrastructure.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../sufr_amd/csrc/sufr_trace.h"

namespace {
// what edit_load8 (sufr_edit.inc) gives: eight bytes from idx on, 0 where outside [0, n); ok: bit j set when byte j is inside
uint64_t load8(const uint8_t* T, uint64_t n, int64_t idx, uint32_t& ok)
{
    uint64_t w = 0;
    ok = 0;
    for (int j = 0; j < 8; j++)
        if (idx + j >= 0 && (uint64_t)(idx + j) < n) { w |= (uint64_t)T[idx + j] << (8 * j); ok |= 1u << j; }
    return w;
}
}

extern "C" {

// One record (end, edits) of the query Q against T.  Returns 0 when the banded value of the end cell is not `edits` (nothing
// else is written then), else 1 with *start, *nruns and the runs in forward order, BAM encoded, the first `cap` of them.
int shim_trace(const uint8_t* T, uint64_t n, const uint8_t* Q, uint64_t m, uint64_t end, uint32_t edits, uint64_t* start,
               uint32_t* nruns, uint32_t* cigar, uint32_t cap)
{
    const uint32_t v = edits;
    const int64_t g = (int64_t)(end + 1) - (int64_t)m;
    std::vector<uint32_t> d0(m + 1), vp(m + 1);
    const uint32_t score = sufr::trace_forward(
        m, v, g, [&](int64_t idx, uint32_t& ok) { return load8(T, n, idx, ok); }, [&](int64_t idx, uint32_t& ok) { return load8(Q, m, idx, ok); },
        [&](uint64_t r, uint32_t D0, uint32_t VP) { d0[r] = D0; vp[r] = VP; });
    if (score != v) return 0;
    std::vector<uint32_t> runs;
    uint32_t nr = 0;
    *start = sufr::trace_walk(
        m, v, g, [&](uint64_t r, uint32_t& D0, uint32_t& VP) { D0 = d0[r]; VP = vp[r]; }, [&](uint64_t i) { return Q[i]; },
        [&](uint64_t j) { return T[j]; }, [&](uint32_t op, uint32_t len) { runs.push_back(len << 4 | op); }, nr);
    *nruns = nr;
    for (uint32_t t = 0; t < nr && t < cap; t++) cigar[t] = runs[nr - 1 - t];
    return 1;
}

}
