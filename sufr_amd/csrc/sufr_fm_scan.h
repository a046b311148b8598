// sufr_fm_scan.h -- the layout and the arithmetic of the FM-index over the BWT of the indexed text (include/sufr_fm.h,
// DESIGN.md section 23): the shape of a block, the count of a byte value in the front of a block, occ, the backward search
// of one query, the walk from a rank to a sampled suffix, the chunk walk of extract (section 25), the backtracking walk of the k-mismatch search (section 24) and the walk of the matching statistics on a pair of indexes (section 26).  Plain integer code that the kernels of sufr_fm.inc and the host
// path of sufr_query.cpp both compile (SUFR_HD, the way of sufr_bwt_scan.h); there is no second copy of it.  The kernels read
// a block with wider loads than fm_occ does and count with the same fm_eq_bytes.
//
// Blocks.  Block j serves the ranks [j B, (j + 1) B): `cbytes` bytes of checkpoints -- for every byte value that occurs, in
// the order of the values, the number of ranks before j B with that BWT byte, w bytes each (w: the index width) -- and behind
// them the B bytes BWT[j B ..], zero where the array has ended.  There are s / B + 1 blocks, so that occ(c, s) has its
// checkpoints where s is a multiple of B.  With cbytes = K w rounded up to 32,
//     stride = the power of two that holds two cbytes, 128 at least;   B = stride - cbytes:
// K <= 8 at w = 4 gives 32 + 96 in one aligned 128-byte line, the granularity of a gather, so an occ is
// one line; 23 amino acids at w = 4 give 96 + 160 in 256, all 256 byte values 1024 + 1024 (w = 4) or 2048 + 2048 (w = 8).  B is
// a multiple of 32 and never below cbytes: the BWT bytes are at least half of every block.
//
// Marks.  One FmMark per 64 ranks: bit i of `bits` says that SA[64 k + i] is a multiple of the sampling rate and was kept,
// `before` is the number of kept values in front of rank 64 k.  16 bytes per 64 ranks at both index widths.
#pragma once
#include <stdint.h>

#include "sufr_bwt_scan.h"

namespace sufr {

static constexpr uint32_t FM_NO_COL = 0xFFFFFFFFu;      // the column of a byte value that does not occur (BWT_NO_COL of sufr_bwt.inc)

struct FmShape { uint32_t K, w, cbytes, B, stride; };

SUFR_HD FmShape fm_shape(uint32_t K, uint32_t w)
{
    FmShape sh{K, w, (K * w + 31u) & ~31u, 0, 128};
    if (sh.cbytes == 0) sh.cbytes = 32;                  // (an empty array: one block of no counts)
    while (sh.stride < 2 * sh.cbytes) sh.stride *= 2;
    sh.B = sh.stride - sh.cbytes;
    return sh;
}

// The ranks of a tile of the build: whole blocks and whole mark words, `ranks` at most and one of each at least
SUFR_HD uint64_t fm_tile(uint32_t B, uint64_t ranks)
{
    const uint64_t unit = B % 64 ? 2 * (uint64_t)B : B;  // (B is a multiple of 32)
    return ranks < unit ? unit : ranks / unit * unit;
}

SUFR_HD uint64_t fm_blocks(uint64_t s, uint32_t B) { return s / B + 1; }
SUFR_HD uint64_t fm_mark_words(uint64_t s) { return (s + 63) / 64; }

struct FmMark { uint64_t bits, before; };

// How many of the first `have` bytes of a dword (in memory order; 4 and more: all) equal the byte whose four copies are pat
SUFR_HD uint32_t fm_eq_bytes(uint32_t word, uint32_t pat, uint32_t have)
{
    const uint32_t x = word ^ pat;
    const uint32_t zero = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);        // 0x80 in every byte of x that is 0
    return (uint32_t)__builtin_popcount(zero & (have >= 4 ? 0xFFFFFFFFu : (1u << (8 * have)) - 1u));
}

SUFR_HD uint64_t fm_rd(const uint8_t* p, uint32_t w)
{
    if (w == 4) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
    uint64_t v; __builtin_memcpy(&v, p, 8); return v;
}

// What a query reads.  C: 257 entries, C[c] the ranks with a smaller BWT byte, C[256] = s; col: 256 entries
struct FmView {
    const uint8_t* blocks;
    const FmMark* marks;
    const uint8_t* kept;                                 // the kept suffixes in rank order, w bytes each
    const uint64_t* C;
    const uint32_t* col;
    uint64_t s, q;                                       // q: the sampling rate, 0 where there are no samples
    FmShape sh;
    uint32_t e;                                          // T[n - 1]
};

// occ(c, r) = #{ j < r : BWT[j] == c } for a byte value c that occurs and r <= s; nothing behind the block of r is read
SUFR_HD uint64_t fm_occ(const FmView& V, uint32_t c, uint64_t r)
{
    const uint8_t* p = V.blocks + r / V.sh.B * V.sh.stride;
    const uint32_t rem = (uint32_t)(r % V.sh.B), pat = c * 0x01010101u;
    uint64_t n = fm_rd(p + V.col[c] * V.sh.w, V.sh.w);
    p += V.sh.cbytes;
    for (uint32_t i = 0; i < rem; i += 4) {
        uint32_t word;
        __builtin_memcpy(&word, p + i, 4);
        n += fm_eq_bytes(word, pat, rem - i);
    }
    return n;
}

// May byte c stand at place i of a query of m bytes?  Not where it does not occur, and the end byte only at the last place:
// the one row whose BWT byte is the end byte is the cyclic one
SUFR_HD bool fm_byte_ok(const FmView& V, uint32_t c, uint64_t i, uint64_t m) { return V.col[c] != FM_NO_COL && (c != V.e || i + 1 == m); }

// The rank range of P[0..m): lo == hi == 0 where it does not occur; every rank for the empty query, which every suffix
// begins with (the answer of sufr_file_search)
SUFR_HD void fm_search(const FmView& V, const uint8_t* P, uint64_t m, uint64_t& lo, uint64_t& hi)
{
    lo = hi = 0;
    if (!m) { hi = V.s; return; }
    if (!fm_byte_ok(V, P[m - 1], m - 1, m)) return;
    uint64_t a = V.C[P[m - 1]], b = V.C[P[m - 1] + 1u];
    for (uint64_t i = m - 1; i-- > 0 && a < b;) {
        const uint32_t c = P[i];
        if (!fm_byte_ok(V, c, i, m)) return;
        a = V.C[c] + fm_occ(V, c, a);
        b = V.C[c] + fm_occ(V, c, b);
    }
    if (a < b) { lo = a; hi = b; }
}

SUFR_HD bool fm_marked(const FmMark& mk, uint64_t r) { return (mk.bits >> (r & 63u)) & 1u; }
SUFR_HD uint64_t fm_slot(const FmMark& mk, uint64_t r) { return mk.before + (uint64_t)__builtin_popcountll(mk.bits & (((uint64_t)1 << (r & 63u)) - 1)); }

// SA[r] for r < s of an index with samples: LF steps to a kept rank, fewer than q of them (position 0 is kept, so the cyclic
// row is never stepped through); ~0 where q steps find none, which only arrays that are no suffix array can cause
SUFR_HD uint64_t fm_position(const FmView& V, uint64_t r)
{
    for (uint64_t k = 0; k < V.q; k++) {
        const FmMark mk = V.marks[r >> 6];
        if (fm_marked(mk, r)) return fm_rd(V.kept + fm_slot(mk, r) * V.sh.w, V.sh.w) + k;
        const uint32_t c = V.blocks[r / V.sh.B * V.sh.stride + V.sh.cbytes + r % V.sh.B];
        r = V.C[c] + fm_occ(V, c, r);
    }
    return ~(uint64_t)0;
}

// ---- extract: a range of the text read back from the BWT (include/sufr_fm_text.h) ------------------
// One LF step from rank r < s: c = BWT[r], the byte in front of the suffix of rank r, and the rank of the suffix that begins
// with it.  On the cyclic row (SA[r] == 0) c is the end byte and the step gives C[e], the rank of suffix n - 1: the row stands
// for position n there (include/sufr_fm_text.h), which is the one use extract makes of it.
SUFR_HD uint64_t fm_lf(const FmView& V, uint64_t r, uint32_t& c)
{
    c = V.blocks[r / V.sh.B * V.sh.stride + V.sh.cbytes + r % V.sh.B];
    return V.C[c] + fm_occ(V, c, r);
}

// A clipped request [start, end) with start < end <= n holds the chunks first .. first + count - 1 of q positions each
SUFR_HD void fm_extract_clip(uint64_t n, uint64_t& start, uint64_t& end)
{
    if (end > n) end = n;
    if (start > end) start = end;
}
SUFR_HD uint64_t fm_extract_chunks(uint64_t q, uint64_t start, uint64_t end) { return start < end ? (end - 1) / q - start / q + 1 : 0; }

// The entry of text_kept that chunk k of an index of n positions starts from: k + 1, the rank of position (k + 1) q, where
// that is a position of the text; else 0, the cyclic row, which stands for position n
SUFR_HD uint64_t fm_extract_slot(uint64_t q, uint64_t n, uint64_t k) { return (k + 1) * q < n ? k + 1 : 0; }

// Chunk k of the clipped request [start, end): from r, the rank text_kept[fm_extract_slot(q, n, k)], top - min(end, top) silent
// steps and then one emit(p, T[p]) per step for p = min(end, top) - 1 down to max(start, k q); top = min((k + 1) q, n).  q steps
// at most.  lf(r, c) is one LF step: it sets c = BWT[r] and returns the next rank (fm_lf, or the kernel's wider loads).
template <class Lf, class Emit>
SUFR_HD void fm_extract_chunk(uint64_t q, uint64_t n, uint64_t k, uint64_t start, uint64_t end, uint64_t r, Lf&& lf, Emit&& emit)
{
    const uint64_t top = (k + 1) * q < n ? (k + 1) * q : n;
    const uint64_t hi = end < top ? end : top, lo = start > k * q ? start : k * q;
    uint32_t c = 0;
    for (uint64_t p = top; p > hi; p--) r = lf(r, c);
    for (uint64_t p = hi; p > lo; p--) {
        r = lf(r, c);
        emit(p - 1, c);
    }
}

// ---- k-mismatch search by backtracking (include/sufr_fm.h) ---------------------------------------
static constexpr uint32_t FM_APPROX_MAX = 3;             // SUFR_FM_APPROX_MAX_MISMATCHES: the walk keeps FM_APPROX_MAX suspended frames

// One step for every byte value: at_lo[k] = occ(c_k, lo) and at_hi[k] = occ(c_k, hi) for the byte value c_k of every column
// k < K, lo <= hi <= s, from the blocks of lo and of hi; where they are one block its bytes are counted once
SUFR_HD void fm_occ_all(const FmView& V, uint64_t lo, uint64_t hi, uint64_t* at_lo, uint64_t* at_hi)
{
    const uint64_t ja = lo / V.sh.B, jb = hi / V.sh.B;
    const uint8_t* pa = V.blocks + ja * V.sh.stride;
    const uint8_t* pb = V.blocks + jb * V.sh.stride;
    const uint32_t ra = (uint32_t)(lo % V.sh.B), rb = (uint32_t)(hi % V.sh.B);
    for (uint32_t k = 0; k < V.sh.K; k++) at_lo[k] = fm_rd(pa + k * V.sh.w, V.sh.w);
    for (uint32_t i = 0; i < ra; i++) at_lo[V.col[pa[V.sh.cbytes + i]]]++;
    uint32_t from = 0;
    if (ja == jb) { for (uint32_t k = 0; k < V.sh.K; k++) at_hi[k] = at_lo[k]; from = ra; }
    else for (uint32_t k = 0; k < V.sh.K; k++) at_hi[k] = fm_rd(pb + k * V.sh.w, V.sh.w);
    for (uint32_t i = from; i < rb; i++) at_hi[V.col[pb[V.sh.cbytes + i]]]++;
}

// A frame of the walk: the rank range [lo, hi) of X[t..m), the places 0 .. t - 1 still to go, and what its Ops made of the
// columns it has yet to try as substitutions at place t - 1
struct FmFrame { uint64_t t, lo, hi; uint32_t next; };

// The walk of one query Q[0..m) with at most d <= FM_APPROX_MAX substitutions: leaf(lo, hi, h) for every leaf, in the order
// of include/sufr_fm.h (at every place the substitutions in ascending byte order, each expanded completely, then the exact
// continuation).  The frame at work is `f`, with h substitutions behind it; the h frames it descends from are suspended in
// `st` (st.put(depth, frame), st.get(depth), depth < d).  A frame moves along its exact path once its substitutions are done,
// so there are never more than d suspended frames, whatever m is, and no range is computed twice.
//   Ops   col(c)               the column of byte value c, FM_NO_COL where it does not occur (V.col, from wherever it is kept)
//         sym(k)               the byte value of column k
//         begin(h, lo, hi)     called once when the frame of depth h < d arrives at a place with the range [lo, hi): prepares
//                              the step of every column and returns the state of the columns to try
//         next(state, k, lo, hi)   takes the next column to try out of the state of the frame with the range [lo, hi); false
//                              when there is none left
//         child(h, c, k, a, b) the step of [a, b) with byte c of column k, for a frame that begin(h, ..) prepared
//         exact(h, prepared, c, k, a, b)   the same for the query's own byte; prepared: begin(h, ..) saw this range
// Termination.  Every iteration of the loop does one of four things: it takes a column out of a frame's state (at most K
// times between two moves of that frame), it pushes (h grows, h <= d), it moves the frame one place down (t shrinks; t is
// never raised, a pushed frame starts below its parent), or it pops.  A frame is popped once and only frames that were
// pushed are; pushes happen only at a (frame, place, column) triple, of which there are finitely many below every frame.
template <class Ops, class Stack, class Leaf>
SUFR_HD void fm_approx_walk(const FmView& V, const uint8_t* Q, uint64_t m, uint32_t d, Ops& ops, Stack& st, Leaf&& leaf)
{
    if (!m) return;
    uint32_t h = 0;
    FmFrame f{m, 0, V.s, d ? ops.begin(0, 0, V.s) : 0};
    for (;;) {
        bool alive = f.t != 0;
        if (!alive) leaf(f.lo, f.hi, h);
        else {
            const uint64_t i = f.t - 1;                  // the place of this step
            const uint32_t q = Q[i];
            uint32_t k;
            if (h < d && ops.next(f.next, k, f.lo, f.hi)) {
                const uint32_t c = ops.sym(k);
                if (c == q || (c == V.e && f.t != m)) continue;      // (fm_byte_ok: the end byte only at the last place)
                uint64_t a = f.lo, b = f.hi;
                ops.child(h, c, k, a, b);
                if (a >= b) continue;
                st.put(h, f);
                h++;
                f = FmFrame{i, a, b, h < d && i ? ops.begin(h, a, b) : 0};
                continue;
            }
            const uint32_t kq = ops.col(q);
            alive = kq != FM_NO_COL && (q != V.e || f.t == m);
            if (alive) {
                ops.exact(h, h < d, q, kq, f.lo, f.hi);
                f.t = i;
                alive = f.lo < f.hi;
                if (alive && h < d && i) f.next = ops.begin(h, f.lo, f.hi);
            }
        }
        if (!alive) {
            if (!h) return;
            f = st.get(--h);
        }
    }
}

// ---- matching statistics on a pair of indexes (include/sufr_fm_match.h) ----------------------------
// May byte c of column k stand inside a match?  Not where it does not occur, and never the end byte: X leaves it out
SUFR_HD bool fm_ms_byte_ok(uint32_t k, uint32_t c, uint32_t e) { return k != FM_NO_COL && c != e; }

// The walk of include/sufr_fm_match.h over the offsets [a, b) of the query Q[0..m), a <= b <= m: out(j, ms[j]) once for every
// a <= j < b, in descending order of j.  F is the index of T, R that of the reversed text; the two agree in C and in the
// columns (sufr_fm_pair_check), which tab.C(c) and tab.col(c) read from wherever they are kept.  step(V, c, k, lo, hi) moves
// the range [lo, hi) of V by the byte c of column k: lo = C[c] + occ(c, lo), hi = C[c] + occ(c, hi).  The extension of an
// offset reads the query up to m, beyond b; the search back stops at a, where the offsets of this piece end -- Q[a..end)
// occurs then, which is all that the offsets a .. x need (fact (a) of the header).  Returns the steps: the bytes looked at.
// Arrays that are no pair of a text and its reversal may end a search back above the offset it came from; the walk then
// gives that one offset its extension and goes on below it, so that it ends, and it reads only what each index reads alone.
template <class Tab, class Step, class Out>
SUFR_HD uint64_t fm_ms_walk(const FmView& F, const FmView& R, const Tab& tab, const uint8_t* Q, uint64_t m, uint64_t a, uint64_t b, Step&& step, Out&& out)
{
    uint64_t steps = 0;
    for (uint64_t x1 = b; x1 > a;) {                     // x1 - 1: the offset at work, x of the header
        const uint64_t x = x1 - 1;
        uint64_t end = x, lo = 0, hi = 0;
        for (; end < m; end++) {                         // forwards on R: ms[x] = end - x
            const uint32_t c = Q[end], k = tab.col(c);
            steps++;
            if (!fm_ms_byte_ok(k, c, F.e)) break;
            uint64_t ua = lo, ub = hi;
            if (end == x) { ua = tab.C(c); ub = tab.C(c + 1u); } else step(R, c, k, ua, ub);
            if (ua >= ub) break;
            lo = ua; hi = ub;
        }
        if (end == x) { out(x, (uint32_t)0); x1 = x; continue; }
        uint64_t start = end;
        for (; start > a; start--) {                     // backwards on F from end: Q[start..end) occurs
            const uint32_t c = Q[start - 1], k = tab.col(c);
            steps++;
            if (!fm_ms_byte_ok(k, c, F.e)) break;
            uint64_t ua = lo, ub = hi;
            if (start == end) { ua = tab.C(c); ub = tab.C(c + 1u); } else step(F, c, k, ua, ub);
            if (ua >= ub) break;
            lo = ua; hi = ub;
        }
        if (start > x) start = x;                        // (only arrays that are no pair)
        for (uint64_t j = x1; j-- > start;) out(j, (uint32_t)(end - j));
        x1 = start;
    }
    return steps;
}

}  // namespace sufr
