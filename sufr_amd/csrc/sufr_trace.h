// sufr_trace.h -- the banded table of one alignment traceback and the walk over it: the arithmetic k_trace_rows and
// k_trace_write (sufr_trace.inc) run per lane, as plain integer code that also compiles on the host (SUFR_HD, the way of
// sufr_runkey.h; tests/trace_shim.cpp holds it to a full-table witness without a GPU).  include/sufr_align.h has the
// contract, DESIGN.md section 17 the argument for the band.
//
// The band of a record with v = edits, e = end + 1, m query bytes, g = e - m.  Row r (r query bytes consumed) holds the
// W = 2v + 1 cells of the columns r + g - v + k, k = 0 .. W - 1: cell k of every row lies on the diagonal g - v + k, the end
// cell (m, e) is cell v of row m.  A cell reads its diagonal neighbour (r - 1, k), the cell above it (r - 1, k + 1) and the
// cell to its left (r, k - 1); outside the band is +inf, row 0 is 0.  Myers' recurrences in Hyyro's banded form, as in
// edit_band (sufr_edit.inc), on 32-bit words: P / N bit k is the delta between the cells k and k + 1 of a row (+1 / -1).
//   the top cell (k = W - 1) has no cell above it: P bit W - 1 is kept set, which says "the cell above is one more than the
//       diagonal neighbour", so that it never gives the minimum: the same as +inf
//   the bottom cell (k = 0) has no cell to its left: the addition that carries the left neighbours along starts without a
//       carry, which gives D0 bit 0 = match | N bit 0: the minimum of the diagonal and the upper neighbour alone
// Text bytes outside [0, n) match nothing: the table is the one of the text with junk on both sides, which agrees with the
// real one on every column 0 .. n (column 0 holds r); the walk handles column 0 itself.
// A row leaves two words: D0 (bit k: cell k equals its diagonal neighbour) and VP (bit k: cell k is one more than the cell
// above it).  The walk needs nothing else.
#pragma once
#include <stdint.h>

#ifndef SUFR_HD
#if defined(__HIPCC__)
#define SUFR_HD __host__ __device__ __forceinline__
#else
#define SUFR_HD static inline
#endif
#endif

namespace sufr {

// BAM op codes of the four ops
static constexpr uint32_t TRACE_OP_I = 1, TRACE_OP_D = 2, TRACE_OP_EQ = 7, TRACE_OP_X = 8;
enum { TRACE_DIAG = 0, TRACE_UP = 1, TRACE_LEFT = 2 };

struct TraceBand {
    uint32_t pl[8], valid;      // sliding bit-planes of the text window of the row: bit k is the text byte of cell k
    uint32_t P, N;              // horizontal deltas of the row
    uint32_t top, wmask;        // bit W - 1, the W low bits
    uint32_t score;             // the value of cell v: the diagonal of the end cell
};

SUFR_HD void trace_init(TraceBand& b, uint32_t v)
{
    b.top = 1u << (2 * v);
    b.wmask = b.top | (b.top - 1);
#pragma unroll
    for (int i = 0; i < 8; i++) b.pl[i] = 0;
    b.valid = 0;
    b.P = b.top;
    b.N = 0;
    b.score = 0;
}

// the window moves one column: `byte` (ok: inside the text) becomes the text byte of the top cell
SUFR_HD void trace_push(TraceBand& b, uint32_t byte, uint32_t ok)
{
#pragma unroll
    for (int i = 0; i < 8; i++) b.pl[i] = (b.pl[i] >> 1) | ((byte >> i) & 1u ? b.top : 0u);
    b.valid = (b.valid >> 1) | (ok ? b.top : 0u);
}

// one row: the query byte qc against the window; D0 and VP of the new row
SUFR_HD void trace_row(TraceBand& b, uint32_t qc, uint32_t v, uint32_t& D0_out, uint32_t& VP_out)
{
    uint32_t eq = b.valid;
#pragma unroll
    for (int i = 0; i < 8; i++) eq &= ~(b.pl[i] ^ (0u - ((qc >> i) & 1u)));
    const uint32_t P = b.P, N = b.N;
    const uint32_t X = eq | N;
    const uint32_t D0 = ((((X & P) + P) ^ P) | X) & b.wmask;
    const uint32_t VP = (N | ~(D0 | P)) & b.wmask, VN = D0 & P, Xs = D0 >> 1;
    b.N = Xs & VP;
    b.P = (VN | ~(Xs | VP)) & b.wmask;           // (bit W - 1 comes out set: Xs and VP are 0 there)
    b.score += (~D0 >> v) & 1u;
    D0_out = D0;
    VP_out = VP;
}

// the move out of cell k of a row with these two words; match: the query byte of the row equals the text byte of the cell.
// A match always has D0 = 1; a mismatch is a diagonal move iff the diagonal delta is 1.
SUFR_HD int trace_move(uint32_t D0, uint32_t VP, uint32_t k, uint32_t match)
{
    if (((D0 >> k) & 1u) == match) return TRACE_DIAG;
    return (VP >> k) & 1u ? TRACE_UP : TRACE_LEFT;
}

// The rows of one record, r = 1 .. m in order.  loadT(idx, ok) / loadQ(idx, ok): eight bytes of the text / the query from the
// signed index idx on, ok bit j set when byte j exists; store(r, D0, VP) keeps row r.  Returns the banded value of the end cell:
// it equals v iff v = D(e) (a band narrower than D(e) reads above v, a wider one reads D(e)).
template <typename LoadT, typename LoadQ, typename Store>
SUFR_HD uint32_t trace_forward(uint64_t m, uint32_t v, int64_t g, LoadT loadT, LoadQ loadQ, Store store)
{
    TraceBand b;
    trace_init(b, v);
    const uint32_t W = 2 * v + 1;
    // the window of row 1 but for its last byte: T[g - v .. g + v)
    for (uint32_t k = 0; k + 1 < W; k += 8) {
        uint32_t ok;
        const uint64_t w = loadT(g - (int64_t)v + (int64_t)k, ok);
#pragma unroll
        for (uint32_t j = 0; j < 8; j++)
            if (k + j + 1 < W) trace_push(b, (uint32_t)(w >> (8 * j)) & 0xFFu, (ok >> j) & 1u);
    }
    for (uint64_t r0 = 0; r0 < m; r0 += 8) {
        uint32_t ok, qok;
        const uint64_t tw = loadT(g + (int64_t)v + (int64_t)r0, ok);
        const uint64_t qw = loadQ((int64_t)r0, qok);
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) {
            if (r0 + j < m) {
                trace_push(b, (uint32_t)(tw >> (8 * j)) & 0xFFu, (ok >> j) & 1u);
                uint32_t D0, VP;
                trace_row(b, (uint32_t)(qw >> (8 * j)) & 0xFFu, v, D0, VP);
                store(r0 + j + 1, D0, VP);
            }
        }
    }
    return b.score;
}

// The walk back from (m, e) over the kept rows.  row(r, D0, VP) reads row r, qbyte(i) / tbyte(j) one byte of the query / the
// text (j is in [0, e)), emit(op, len) takes the runs, last run first.  Returns the start; nruns: the number of runs.
// In column 0 the only move is up (the junk table left of the text would offer a diagonal one).
template <typename Row, typename QByte, typename TByte, typename Emit>
SUFR_HD uint64_t trace_walk(uint64_t m, uint32_t v, int64_t g, Row row, QByte qbyte, TByte tbyte, Emit emit, uint32_t& nruns)
{
    uint64_t i = m;
    int64_t j = g + (int64_t)m;                   // the column; the cell index is k = j - i - g + v
    uint32_t k = v, op = 0, len = 0, runs = 0;
    while (i > 0) {
        int mv = TRACE_UP;
        uint32_t o = TRACE_OP_I;
        if (j > 0) {
            uint32_t D0, VP;
            row(i, D0, VP);
            const uint32_t match = qbyte(i - 1) == tbyte((uint64_t)(j - 1)) ? 1u : 0u;
            mv = trace_move(D0, VP, k, match);
            o = mv == TRACE_DIAG ? (match ? TRACE_OP_EQ : TRACE_OP_X) : mv == TRACE_UP ? TRACE_OP_I : TRACE_OP_D;
        }
        if (o != op) {
            if (len) { emit(op, len); runs++; }
            op = o;
            len = 0;
        }
        len++;
        if (mv == TRACE_DIAG) { i--; j--; }
        else if (mv == TRACE_UP) { i--; k++; }
        else { j--; k--; }
    }
    if (len) { emit(op, len); runs++; }
    nruns = runs;
    return (uint64_t)j;
}

}  // namespace sufr
