// sufr_fm.inc -- the FM-index over the BWT of a device-resident index: its build, the backward search and the locate that
// reads neither the text nor the suffix array (included by sufr_kernels.hip after sufr_bwt.inc; include/sufr_fm.h and
// sufr_fm_approx.h, DESIGN.md sections 23 and 24).  The layout and the arithmetic are sufr_fm_scan.h, which the host path compiles too.
//
// Build.  The BWT goes to scratch of the context by k_bwt_gather, which also counts the bytes; one synchronisation reads the
// counts and the end byte, which decide the refusal, K and with it the shape of a block.  The tiles of the build are those of
// sufr_hip_set_bwt_tile cut down to whole blocks and whole mark words (fm_tile); there is one tile more than the ranks need
// where they fill the last one, for the trailing block.  k_bwt_cols, k_bwt_tile_hist and k_bwt_col_scan (sufr_bwt.inc) leave the
// number of ranks of every occurring byte value before every tile.  Then
// k_fm_blocks      a workgroup per tile, the tile's bytes in LDS: a lane per (block, byte value) counts the value in the block
//                  with fm_eq_bytes, a lane per byte value adds the counts up from the tile's base and writes the checkpoints
//                  of every block, all lanes copy the bytes.  With samples: the marks SA[r] % q == 0 as ballot words, and the
//                  number of marks of the tile (an LDS sum: no order in it).
// k_locate_scan    (sufr_search.inc) the tiles' mark counts into bases and the number of samples: the second synchronisation.
// k_fm_samples     a workgroup per tile: the marks before every word (a popcount prefix over the tile's words behind the
//                  tile's base) and the kept values in rank order -- the count and write passes of the runs of sufr_bwt.inc.
// No result comes from the arrival order of an atomic: two builds give the same bytes.
//
// k_fm_search      a lane per query.  A step needs occ at lo and at hi, two independent blocks: in the one-line shape (32 bytes
//                  of counts and 96 of BWT in 128) both blocks are loaded whole, twelve 16-byte loads and the two counts in
//                  flight before any is used; in the wide shapes the two blocks are read side by side, 16 bytes at a time, up
//                  to the rank.  C and the columns are in LDS.  The steps of a query depend on each other; nothing is read
//                  behind the query or behind a block.
// k_fm_locate      k_locate_counts / k_locate_scan / k_locate_apply size the output as for sufr_hip_locate_batch_device; then a
//                  lane per hit walks LF steps to a marked rank and stores kept + steps.
// k_fm_approx      k-mismatch search by backtracking (include/sufr_fm_approx.h, DESIGN.md section 24): a lane per (query, strand)
//                  runs fm_approx_walk of sufr_fm_scan.h, the frame at work in registers and the at most three suspended
//                  ones in LDS; a count pass (leaves and records of every item, scanned in the workgroup), k_locate_scan over
//                  the workgroups' sums (the one synchronisation), a fill pass that stores every leaf at its slot, then
//                  k_fm_locate with the leaves as its queries and k_fm_approx_expand for the other record columns.
// k_fm_text_samples  with SUFR_FM_TEXT (include/sufr_fm_text.h, DESIGN.md section 25), behind k_fm_samples on the same tiles: the
//                  rank of every kept position, text_kept[SA[r] / q] = r.  One writer per entry, no atomics.
// k_fm_extract     k_fm_extract_counts (a lane per request: its clipped length and its chunks, scanned in the workgroup),
//                  k_locate_scan over both sums (the one synchronisation, for the two totals), k_fm_extract_apply; then a lane
//                  per chunk runs fm_extract_chunk of sufr_fm_scan.h: at most q LF steps from a text sample, each one fm_occ_one
//                  in the block that also holds the step's BWT byte, the bytes gathered in a register and stored as dwords.
// k_fm_ms          matching statistics on a pair of indexes, that of the text and that of its reversal (include/sufr_fm_match.h,
//                  DESIGN.md section 26): a lane per slab of G bytes of the batch runs fm_ms_walk of sufr_fm_scan.h for the part of
//                  every query in it; the SMEMs then come from the kernels of sufr_match.inc and k_fm_search on the slices.
// The copies (sufr_hip_fm_upload / _download) are allocations and copies.
// No scratch.  LDS: k_fm_blocks 34 KB, k_fm_samples 4 KB, k_fm_search, k_fm_locate, k_fm_extract and k_fm_ms 3 KB, k_fm_approx 25 KB.

#include "../../include/sufr_fm_text.h"
#include "../../include/sufr_fm_match.h"
#include "sufr_fm_host.h"

struct sufr_hip_fm {
    int device = 0;
    sufr::FmView V{};                  // device addresses
    uint64_t samples = 0;
    void *blocks = nullptr, *marks = nullptr, *kept = nullptr, *tabs = nullptr;      // the allocations: tabs = C (257 u64), col (256 u32)
    void* text_kept = nullptr;         // SUFR_FM_TEXT: the rank of every kept position, `samples` entries of w bytes (sufr_fm_text.h)
    uint8_t h_tabs[257 * 8 + 256 * 4] = {0};       // what tabs holds, on the host: the pair check of sufr_fm_match.h reads no device memory
};

namespace sufr {

static constexpr uint32_t FM_PAIRS_MAX = BWT_TILE_MAX / 4;            // (block, byte value) pairs of a tile: B >= K w >= 4 K

// the one-line shape: the constants the compiler may fold
template <bool LINE> __device__ __forceinline__ uint32_t fm_B(const FmShape& sh) { return LINE ? 96u : sh.B; }
template <bool LINE> __device__ __forceinline__ uint32_t fm_stride(const FmShape& sh) { return LINE ? 128u : sh.stride; }
template <bool LINE> __device__ __forceinline__ uint32_t fm_cbytes(const FmShape& sh) { return LINE ? 32u : sh.cbytes; }
static inline bool fm_is_line(const FmShape& sh) { return sh.B == 96 && sh.stride == 128 && sh.cbytes == 32 && sh.w == 4; }

__device__ __forceinline__ uint64_t fm_ld(const uint8_t* p, uint32_t w) { return w == 4 ? (uint64_t)*(const uint32_t*)p : *(const uint64_t*)p; }

// how many of the bytes [at, at + 16) of a block's BWT, of which the first rem count, equal the byte of pat
__device__ __forceinline__ uint32_t fm_eq16(const uint4& x, uint32_t pat, uint32_t rem, uint32_t at)
{
    const uint32_t have = rem > at ? rem - at : 0;
    return fm_eq_bytes(x.x, pat, have) + fm_eq_bytes(x.y, pat, have > 4 ? have - 4 : 0) + fm_eq_bytes(x.z, pat, have > 8 ? have - 8 : 0) +
           fm_eq_bytes(x.w, pat, have > 12 ? have - 12 : 0);
}

// a = C[c] + occ(c, a) and b = C[c] + occ(c, b) for the byte value c of column k; base = C[c]
template <bool LINE>
__device__ __forceinline__ void fm_occ_pair(const FmView& V, uint32_t c, uint32_t k, uint64_t base, uint64_t& a, uint64_t& b)
{
    const uint32_t B = fm_B<LINE>(V.sh), pat = c * 0x01010101u;
    const uint8_t* pa = V.blocks + a / B * fm_stride<LINE>(V.sh);
    const uint8_t* pb = V.blocks + b / B * fm_stride<LINE>(V.sh);
    const uint32_t ra = (uint32_t)(a % B), rb = (uint32_t)(b % B), w = LINE ? 4u : V.sh.w;
    uint64_t na = fm_ld(pa + k * w, w), nb = fm_ld(pb + k * w, w);
    const uint4* va = (const uint4*)(pa + fm_cbytes<LINE>(V.sh));
    const uint4* vb = (const uint4*)(pb + fm_cbytes<LINE>(V.sh));
    if (LINE) {
        uint4 xa[6], xb[6];
#pragma unroll
        for (int i = 0; i < 6; i++) { xa[i] = va[i]; xb[i] = vb[i]; }
#pragma unroll
        for (int i = 0; i < 6; i++) { na += fm_eq16(xa[i], pat, ra, 16u * i); nb += fm_eq16(xb[i], pat, rb, 16u * i); }
    } else {
        const uint32_t far = ra > rb ? ra : rb;
        for (uint32_t at = 0; at < far; at += 16) {      // (at < rem <= B: inside the block)
            const uint4 zero = make_uint4(0, 0, 0, 0);
            const uint4 xa = at < ra ? va[at / 16] : zero, xb = at < rb ? vb[at / 16] : zero;
            na += fm_eq16(xa, pat, ra, at);
            nb += fm_eq16(xb, pat, rb, at);
        }
    }
    a = base + na;
    b = base + nb;
}

// base + occ(c, r) for the byte value c of column k, r = the block at p plus rem ranks: the one occ of an LF step
template <bool LINE>
__device__ __forceinline__ uint64_t fm_occ_one(const FmView& V, uint32_t c, uint32_t k, uint64_t base, const uint8_t* p, uint32_t rem)
{
    const uint32_t pat = c * 0x01010101u, w = LINE ? 4u : V.sh.w;
    uint64_t n = fm_ld(p + k * w, w);
    const uint4* v = (const uint4*)(p + fm_cbytes<LINE>(V.sh));
    if (LINE) {
        uint4 x[6];
#pragma unroll
        for (int i = 0; i < 6; i++) x[i] = v[i];
#pragma unroll
        for (int i = 0; i < 6; i++) n += fm_eq16(x[i], pat, rem, 16u * i);
    } else {
        for (uint32_t at = 0; at < rem; at += 16) n += fm_eq16(v[at / 16], pat, rem, at);      // (at < rem <= B: inside the block)
    }
    return base + n;
}

// C and the columns of an index into LDS (257 and 256 entries), by the 256 lanes of a workgroup
__device__ __forceinline__ void fm_stage_tables(const FmView& V, uint64_t* s_C, uint32_t* s_col)
{
    s_C[threadIdx.x] = V.C[threadIdx.x];
    s_col[threadIdx.x] = V.col[threadIdx.x];
    if (threadIdx.x == 0) s_C[256] = V.C[256];
    __syncthreads();
}

template <bool LINE>
__global__ __launch_bounds__(256) void k_fm_search(FmView V, const uint8_t* __restrict__ queries, const uint64_t* __restrict__ qoff, uint64_t nq,
                                                   uint64_t* __restrict__ lo_out, uint64_t* __restrict__ hi_out)
{
    __shared__ uint64_t s_C[257];
    __shared__ uint32_t s_col[256];
    fm_stage_tables(V, s_C, s_col);
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    const uint8_t* P = queries + qoff[i];
    const uint64_t m = qoff[i + 1] - qoff[i];
    uint64_t a = 0, b = m ? 0 : V.s;                                 // (the empty query: every rank)
    if (m) {
        uint32_t c = P[m - 1], next = m > 1 ? P[m - 2] : 0;
        if (s_col[c] != FM_NO_COL) { a = s_C[c]; b = s_C[c + 1]; }
        for (uint64_t j = m - 1; j-- > 0 && a < b;) {
            c = next;
            next = j ? P[j - 1] : 0;                              // (the byte of the next step is under way while this one's blocks are)
            const uint32_t k = s_col[c];
            if (k == FM_NO_COL || c == V.e) { a = b = 0; break; }      // (the end byte stands only at the last place)
            fm_occ_pair<LINE>(V, c, k, s_C[c], a, b);
        }
    }
    const bool found = a < b;
    lo_out[i] = found ? a : 0;
    hi_out[i] = found ? b : 0;
}

template <bool LINE>
__global__ __launch_bounds__(256) void k_fm_locate(FmView V, const uint64_t* __restrict__ lo, const uint64_t* __restrict__ off, uint64_t nq,
                                                   uint64_t total, uint32_t* __restrict__ positions, uint64_t* __restrict__ positions64)
{
    __shared__ uint64_t s_C[257];
    __shared__ uint32_t s_col[256];
    fm_stage_tables(V, s_C, s_col);
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= total) return;
    const uint64_t q = last_le(off, 0, nq, j);                       // the query whose slice holds output j
    uint64_t r = lo[q] + (j - off[q]), p = ~(uint64_t)0;
    const uint32_t B = fm_B<LINE>(V.sh);
    if (r < V.s) {
        for (uint64_t k = 0; k < V.q; k++) {
            const FmMark mk = V.marks[r >> 6];
            const uint8_t* pb = V.blocks + r / B * fm_stride<LINE>(V.sh);
            const uint32_t rem = (uint32_t)(r % B);
            const uint32_t c = pb[fm_cbytes<LINE>(V.sh) + rem];
            if (fm_marked(mk, r)) { p = fm_ld(V.kept + fm_slot(mk, r) * V.sh.w, V.sh.w) + k; break; }
            r = fm_occ_one<LINE>(V, c, s_col[c], s_C[c], pb, rem);
        }
    }
    if (positions64) positions64[j] = p; else positions[j] = (uint32_t)p;
}

// ---- k-mismatch search by backtracking (DESIGN.md section 24) --------------------------------------------------------------
// What fm_approx_walk (sufr_fm_scan.h) asks of a lane.  One-line shape: the state of a frame is the set of columns whose child
// range is not empty, a bit each (K <= 8), and next takes the lowest; wide shapes: the state is the next column, every column
// is tried while the range is wide, and only the columns of the bytes BWT[lo .. hi) once it holds FM_FEW_RANKS ranks or fewer.
// A child and an exact step are one fm_occ_pair.
static constexpr uint64_t FM_FEW_RANKS = 16;
template <bool LINE>
struct FmLaneOps {
    const FmView& V;
    const uint64_t* s_C;
    const uint32_t* s_col;
    const uint8_t* s_sym;

    __device__ __forceinline__ uint32_t col(uint32_t c) const { return s_col[c]; }
    __device__ __forceinline__ uint32_t sym(uint32_t k) const { return s_sym[k]; }
    __device__ __forceinline__ bool next(uint32_t& state, uint32_t& k, uint64_t lo, uint64_t hi) const
    {
        if (LINE) {
            if (!state) return false;
            k = (uint32_t)__builtin_ctz(state);
            state &= state - 1;
            return true;
        }
        k = state;
        if (hi - lo <= FM_FEW_RANKS) {                   // only a byte of BWT[lo .. hi) has a child: the lowest such column from `state` on
            k = FM_NO_COL;
            const uint8_t* p = V.blocks + lo / V.sh.B * V.sh.stride + V.sh.cbytes;
            const uint32_t rem = (uint32_t)(lo % V.sh.B), last = (uint32_t)(hi - lo) - 1;
#pragma unroll
            for (uint32_t j = 0; j < FM_FEW_RANKS; j++) {      // every load is of a rank of the range (the last one again behind it), none waits for another
                const uint32_t at = rem + (j < last ? j : last);              // (FM_FEW_RANKS <= B: one block edge at most)
                const uint32_t kr = s_col[p[at < V.sh.B ? at : at - V.sh.B + V.sh.stride]];
                if (kr >= state && kr < k) k = kr;
            }
        }
        if (k >= V.sh.K) return false;
        state = k + 1;
        return true;
    }
    __device__ __forceinline__ void child(uint32_t, uint32_t c, uint32_t k, uint64_t& a, uint64_t& b) const { fm_occ_pair<LINE>(V, c, k, s_C[c], a, b); }
    __device__ __forceinline__ void exact(uint32_t, bool, uint32_t c, uint32_t k, uint64_t& a, uint64_t& b) const { fm_occ_pair<LINE>(V, c, k, s_C[c], a, b); }
    // the columns with occ(c, lo) < occ(c, hi), lo < hi <= s.  A short range: the columns of the bytes BWT[lo .. hi) themselves;
    // else the counts of the two lines, every column counted from the same twelve loads
    __device__ __forceinline__ uint32_t begin(uint32_t, uint64_t lo, uint64_t hi) const
    {
        if (!LINE) return 0;
        uint32_t mask = 0;
        if (hi - lo <= FM_FEW_RANKS / 2) {
            const uint8_t* p = V.blocks + lo / 96u * 128u + 32u;
            const uint32_t rem = (uint32_t)(lo % 96u), last = (uint32_t)(hi - lo) - 1;
#pragma unroll
            for (uint32_t j = 0; j < FM_FEW_RANKS / 2; j++) {  // every load is of a rank of the range (the last one again behind it), none waits for another
                const uint32_t at = rem + (j < last ? j : last);
                mask |= 1u << s_col[p[at < 96u ? at : at + 32u]];           // (a byte of the array, which occurs; one block edge at most)
            }
            return mask;
        }
        const uint8_t* pa = V.blocks + lo / 96u * 128u;
        const uint8_t* pb = V.blocks + hi / 96u * 128u;
        const uint32_t ra = (uint32_t)(lo % 96u), rb = (uint32_t)(hi % 96u);
        // the two lines 16 bytes at a time, every column counted from the same loads; the loop is kept rolled: unrolled, its
        // 64 registers of line and the eight columns in flight brought the kernel to 203 VGPRs and 2 waves a SIMD
        const uint4 ca0 = ((const uint4*)pa)[0], ca1 = ((const uint4*)pa)[1], cb0 = ((const uint4*)pb)[0], cb1 = ((const uint4*)pb)[1];
        uint32_t diff[8] = {cb0.x - ca0.x, cb0.y - ca0.y, cb0.z - ca0.z, cb0.w - ca0.w, cb1.x - ca1.x, cb1.y - ca1.y, cb1.z - ca1.z, cb1.w - ca1.w};
        uint32_t pat[8];
#pragma unroll
        for (int k = 0; k < 8; k++) pat[k] = s_sym[k] * 0x01010101u;      // (columns behind K: counts of 0 on both sides, any byte)
#pragma unroll 1
        for (uint32_t at = 0; at < 96u; at += 16u) {
            const uint4 xa = *(const uint4*)(pa + 32u + at), xb = *(const uint4*)(pb + 32u + at);
#pragma unroll
            for (int k = 0; k < 8; k++) diff[k] += fm_eq16(xb, pat[k], rb, at) - fm_eq16(xa, pat[k], ra, at);
        }
#pragma unroll
        for (int k = 0; k < 8; k++) if ((uint32_t)k < V.sh.K && diff[k]) mask |= 1u << k;
        return mask;
    }
};

// the suspended frames of the 256 lanes of a workgroup, by depth
struct FmLaneStack {
    uint64_t* s_t;
    uint64_t* s_lo;
    uint64_t* s_hi;
    uint32_t* s_next;
    __device__ __forceinline__ void put(uint32_t h, const FmFrame& f) const
    {
        const uint32_t at = h * 256 + threadIdx.x;
        s_t[at] = f.t; s_lo[at] = f.lo; s_hi[at] = f.hi; s_next[at] = f.next;
    }
    __device__ __forceinline__ FmFrame get(uint32_t h) const
    {
        const uint32_t at = h * 256 + threadIdx.x;
        return FmFrame{s_t[at], s_lo[at], s_hi[at], s_next[at]};
    }
};

// What the two passes of k_fm_approx exchange.  item_*: for every item the leaves and the records of the items before it in
// its workgroup; wg_*: per workgroup, after k_locate_scan those of the workgroups before it.  A leaf: its first rank, the
// offset of its first record, item << 8 | substitutions
struct FmApproxBufs {
    uint64_t *item_leaf, *item_rec, *wg_leaf, *wg_rec;
    uint64_t *leaf_lo, *leaf_off, *leaf_tag;
    uint64_t nleaves;
};

// A lane per item (a query, or a strand of one).  Count pass: the leaves and the records of every item, scanned in the
// workgroup.  Fill pass: the same walk, every leaf stored at its slot -- no order comes from an atomic.
template <bool LINE, bool FILL>
__global__ __launch_bounds__(256) void k_fm_approx(FmView V, const uint8_t* __restrict__ queries, const uint64_t* __restrict__ qoff, uint64_t nq,
                                                   uint32_t d, FmApproxBufs o)
{
    __shared__ uint64_t s_C[257], s_w[8];
    __shared__ uint32_t s_col[256];
    __shared__ uint8_t s_sym[256];
    __shared__ uint64_t s_t[FM_APPROX_MAX * 256], s_lo[FM_APPROX_MAX * 256], s_hi[FM_APPROX_MAX * 256];
    __shared__ uint32_t s_next[FM_APPROX_MAX * 256];
    s_sym[threadIdx.x] = 0;                              // (the columns behind K are read, masked, by FmLaneOps::begin)
    __syncthreads();
    if (V.col[threadIdx.x] != FM_NO_COL) s_sym[V.col[threadIdx.x]] = (uint8_t)threadIdx.x;
    fm_stage_tables(V, s_C, s_col);
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const FmLaneOps<LINE> ops{V, s_C, s_col, s_sym};
    const FmLaneStack st{s_t, s_lo, s_hi, s_next};
    uint64_t cnt[2] = {0, 0}, tot[2];                    // leaves, records
    if (FILL) {
        if (i < nq) { cnt[0] = o.wg_leaf[blockIdx.x] + o.item_leaf[i]; cnt[1] = o.wg_rec[blockIdx.x] + o.item_rec[i]; }
    }
    if (i < nq) {
        fm_approx_walk(V, queries + qoff[i], qoff[i + 1] - qoff[i], d, ops, st, [&](uint64_t lo, uint64_t hi, uint32_t h) {
            if (FILL && cnt[0] < o.nleaves) { o.leaf_lo[cnt[0]] = lo; o.leaf_off[cnt[0]] = cnt[1]; o.leaf_tag[cnt[0]] = i << 8 | h; }
            cnt[0]++;
            cnt[1] += hi - lo;
        });
    }
    if (FILL) return;
    wg_scan(cnt, tot, s_w);
    if (i < nq) { o.item_leaf[i] = cnt[0]; o.item_rec[i] = cnt[1]; }
    if (threadIdx.x == 0) { o.wg_leaf[blockIdx.x] = tot[0]; o.wg_rec[blockIdx.x] = tot[1]; }
}

// query, strand and mismatches of record j from the leaf whose slice holds it (the positions are k_fm_locate's)
__global__ __launch_bounds__(256) void k_fm_approx_expand(const uint64_t* __restrict__ leaf_off, const uint64_t* __restrict__ leaf_tag, uint64_t nleaves,
                                                          uint64_t total, uint32_t both, uint64_t* __restrict__ out_query,
                                                          uint8_t* __restrict__ out_strand, uint8_t* __restrict__ out_mism)
{
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= total) return;
    const uint64_t tag = leaf_tag[last_le(leaf_off, 0, nleaves, j)], a = tag >> 8;
    out_query[j] = both ? a >> 1 : a;
    out_strand[j] = (uint8_t)(both ? a & 1 : 0);
    out_mism[j] = (uint8_t)tag;
}

// ---- matching statistics on a pair of indexes (include/sufr_fm_match.h, DESIGN.md section 26) --------------------------------
// C and the columns in LDS: the tables of fm_ms_walk.  The pair agrees in them (fm_pair_check), so one copy serves both views
struct FmLaneTab {
    const uint64_t* s_C;
    const uint32_t* s_col;
    __device__ __forceinline__ uint32_t col(uint32_t c) const { return s_col[c]; }
    __device__ __forceinline__ uint64_t C(uint32_t c) const { return s_C[c]; }
};

// A lane per slab of G consecutive bytes of the concatenated batch (grid-stride: the grid does not depend on the batch).  The
// part of every query that the slab touches is one fm_ms_walk of sufr_fm_scan.h over the offsets the slab owns; the walk
// reads the query beyond the slab, up to its end, and writes ms only inside the slab.  No atomics, no per-lane array.
template <bool LINE, uint32_t G>
__global__ __launch_bounds__(256) void k_fm_ms(FmView F, FmView R, const uint8_t* __restrict__ queries, const uint64_t* __restrict__ qoff, uint64_t nq,
                                               uint32_t* __restrict__ ms)
{
    __shared__ uint64_t s_C[257];
    __shared__ uint32_t s_col[256];
    fm_stage_tables(F, s_C, s_col);
    const FmLaneTab tab{s_C, s_col};
    const uint64_t g0 = qoff[0], g_end = qoff[nq], nslabs = (g_end - g0 + G - 1) / G, stride = (uint64_t)gridDim.x * 256;
    for (uint64_t slab = (uint64_t)blockIdx.x * 256 + threadIdx.x; slab < nslabs; slab += stride) {
        const uint64_t lo = g0 + slab * G, hi = lo + G < g_end ? lo + G : g_end;
        uint64_t a = last_le(qoff, 0, nq, lo);
        for (uint64_t g = lo; g < hi;) {
            while (qoff[a + 1] <= g) a++;                  // (g < g_end == qoff[nq]: a stays below nq)
            const uint64_t qb = qoff[a], qe = qoff[a + 1], pe = qe < hi ? qe : hi;
            uint32_t* out = ms + qb;
            fm_ms_walk(F, R, tab, queries + qb, qe - qb, g - qb, pe - qb,
                       [&](const FmView& V, uint32_t c, uint32_t k, uint64_t& x, uint64_t& y) { fm_occ_pair<LINE>(V, c, k, s_C[c], x, y); },
                       [&](uint64_t j, uint32_t v) { out[j] = v; });
            g = pe;
        }
    }
}

// The blocks of tile t and, with a sampling rate q, its mark words and t_cnt[t], the number of its marks.  tab: the ranks of
// every column before the tile (k_bwt_col_scan)
template <typename T>
__global__ __launch_bounds__(256) void k_fm_blocks(const T* __restrict__ sa, const uint8_t* __restrict__ bwt, uint64_t s, uint32_t tile, uint64_t ntiles,
                                                   FmShape sh, const uint32_t* __restrict__ col, const uint64_t* __restrict__ tab, uint64_t q,
                                                   uint8_t* __restrict__ blocks, FmMark* __restrict__ marks, uint64_t* __restrict__ t_cnt)
{
    __shared__ uint32_t s_w[BWT_TILE_MAX / 4], s_cnt[FM_PAIRS_MAX], s_sym[256], s_marks;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t K = sh.K, B = sh.B, bw = B / 4;
    if (col[threadIdx.x] != FM_NO_COL) s_sym[col[threadIdx.x]] = threadIdx.x;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t base = t * tile;
        const uint32_t len = (uint32_t)(s - base < tile ? s - base : tile);
        const uint32_t nblk = t + 1 < ntiles ? tile / B : len / B + 1;             // (the last tile is short: its last block is the trailing one)
        const uint32_t* src = (const uint32_t*)(bwt + base);                         // (base is a multiple of 32, the array padded to a dword)
        if (threadIdx.x == 0) s_marks = 0;
        for (uint32_t i = threadIdx.x; i < nblk * bw; i += 256) {
            uint32_t word = 4 * i < len ? src[i] : 0;
            if (4 * i < len && len - 4 * i < 4) word &= (1u << (8 * (len - 4 * i))) - 1u;      // zero behind the array's end
            s_w[i] = word;
        }
        __syncthreads();
        for (uint32_t p = threadIdx.x; p < nblk * K; p += 256) {
            const uint32_t j = p / K, pat = s_sym[p % K] * 0x01010101u;
            const uint32_t have = len > j * B ? (len - j * B < B ? len - j * B : B) : 0;
            uint32_t n = 0;
            for (uint32_t i = 0; 4 * i < have; i++) n += fm_eq_bytes(s_w[j * bw + i], pat, have - 4 * i);
            s_cnt[p] = n;
        }
        __syncthreads();
        uint8_t* out = blocks + base / B * sh.stride;
        if (threadIdx.x < sh.cbytes / sh.w) {             // a lane per count of a block, the unused ones behind the K zero
            uint64_t run = threadIdx.x < K ? tab[t * K + threadIdx.x] : 0;
            for (uint32_t j = 0; j < nblk; j++) {
                uint8_t* at = out + (uint64_t)j * sh.stride + threadIdx.x * sh.w;
                if (sh.w == 4) *(uint32_t*)at = (uint32_t)run; else *(uint64_t*)at = run;
                if (threadIdx.x < K) run += s_cnt[j * K + threadIdx.x];
            }
        }
        for (uint32_t i = threadIdx.x; i < nblk * bw; i += 256)
            ((uint32_t*)(out + (uint64_t)(i / bw) * sh.stride + sh.cbytes))[i % bw] = s_w[i];
        if (q) {
            for (uint32_t it = 0; it < len; it += 256) {    // (uniform: every lane of a wave takes part in the ballot)
                const uint32_t i = it + threadIdx.x;
                const uint64_t m = __ballot(i < len && (uint64_t)sa[base + (i < len ? i : 0)] % q == 0);
                if (lane == 0 && it + 64 * wave < len) {
                    marks[(base >> 6) + (it >> 6) + wave].bits = m;
                    atomicAdd(&s_marks, (uint32_t)__builtin_popcountll(m));           // (a sum: any order)
                }
            }
            __syncthreads();
            if (threadIdx.x == 0) t_cnt[t] = s_marks;
        }
        __syncthreads();                                 // (the LDS arrays are the next tile's)
    }
}

// t_cnt[t]: the marks before tile t (k_locate_scan).  The marks before every word of the tile, and the kept suffixes
template <typename T>
__global__ __launch_bounds__(256) void k_fm_samples(const T* __restrict__ sa, uint64_t s, uint32_t tile, uint64_t ntiles, const uint64_t* __restrict__ t_cnt,
                                                    FmMark* __restrict__ marks, T* __restrict__ kept)
{
    __shared__ uint64_t s_bits[BWT_TILE_MAX / 64], s_pf[BWT_TILE_MAX / 64], s_sc[4];
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t base = t * tile;
        const uint32_t len = (uint32_t)(s - base < tile ? s - base : tile), nwords = (len + 63) / 64;
        const uint64_t bits = threadIdx.x < nwords ? marks[(base >> 6) + threadIdx.x].bits : 0;
        uint64_t v[1] = {(uint64_t)__builtin_popcountll(bits)}, tot[1];
        wg_scan(v, tot, s_sc);
        const uint64_t before = t_cnt[t] + v[0];
        if (threadIdx.x < nwords) marks[(base >> 6) + threadIdx.x].before = before;
        s_bits[threadIdx.x] = bits;
        s_pf[threadIdx.x] = before;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < len; i += 256) {
            const FmMark mk{s_bits[i >> 6], s_pf[i >> 6]};
            if (fm_marked(mk, i)) kept[fm_slot(mk, i)] = sa[base + i];
        }
        __syncthreads();                                 // (the LDS arrays are the next tile's)
    }
}

// ---- text samples and extract (include/sufr_fm_text.h, DESIGN.md section 25) ------------------------------------------------
// text_kept[SA[r] / q] = r for the marked ranks of every tile: every entry has one writer, so there is no order in it
template <typename T>
__global__ __launch_bounds__(256) void k_fm_text_samples(const T* __restrict__ sa, uint64_t s, uint32_t tile, uint64_t ntiles, uint64_t q, uint64_t samples,
                                                         T* __restrict__ text_kept)
{
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t base = t * tile;
        const uint32_t len = (uint32_t)(s - base < tile ? s - base : tile);
        for (uint32_t i = threadIdx.x; i < len; i += 256) {
            const uint64_t p = sa[base + i];
            if (p % q == 0 && p / q < samples) text_kept[p / q] = (T)(base + i);      // (p < n in a suffix array: the guard keeps any array inside)
        }
    }
}

// A lane per request: its clipped length and its chunks, scanned in the workgroup; wg_*: the workgroup's sums
__global__ __launch_bounds__(256) void k_fm_extract_counts(const uint64_t* __restrict__ starts, const uint64_t* __restrict__ ends, uint64_t num, uint64_t n,
                                                           uint64_t q, uint64_t* __restrict__ off, uint64_t* __restrict__ choff,
                                                           uint64_t* __restrict__ wg_bytes, uint64_t* __restrict__ wg_chunks)
{
    __shared__ uint64_t s_w[8];
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint64_t v[2] = {0, 0}, tot[2];                       // bytes, chunks
    if (i < num) {
        uint64_t a = starts[i], b = ends[i];
        fm_extract_clip(n, a, b);
        v[0] = b - a;
        v[1] = fm_extract_chunks(q, a, b);
    }
    wg_scan(v, tot, s_w);
    if (i < num) { off[i] = v[0]; choff[i] = v[1]; }
    if (threadIdx.x == 0) { wg_bytes[blockIdx.x] = tot[0]; wg_chunks[blockIdx.x] = tot[1]; }
}

// the workgroups' bases (k_locate_scan) onto the offsets of every request, and the two totals behind them
__global__ __launch_bounds__(256) void k_fm_extract_apply(uint64_t* __restrict__ off, uint64_t* __restrict__ choff, uint64_t num,
                                                          const uint64_t* __restrict__ wg_bytes, const uint64_t* __restrict__ wg_chunks,
                                                          const uint64_t* __restrict__ totals)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < num) { off[i] += wg_bytes[i / 256]; choff[i] += wg_chunks[i / 256]; }
    if (i == num) { off[num] = totals[0]; choff[num] = totals[1]; }
}

// the low cnt <= 3 bytes of acc to a[0 .. cnt)
__device__ __forceinline__ void fm_put_bytes(uint8_t* a, uint32_t acc, uint32_t cnt)
{
    if (cnt > 0) a[0] = (uint8_t)acc;
    if (cnt > 1) a[1] = (uint8_t)(acc >> 8);
    if (cnt > 2) a[2] = (uint8_t)(acc >> 16);
}

// A lane per chunk: fm_extract_chunk of sufr_fm_scan.h with a step that reads the block once, for the byte and for its occ.
// The lane's bytes go to consecutive addresses, downwards: they are gathered in one register, the byte of the lower address
// shifted in below the others, and stored as a dword whenever an aligned address is reached with four of them, as single
// bytes at the two edges of the lane's slice (a neighbouring lane owns the rest of those dwords).
template <bool LINE>
__global__ __launch_bounds__(256) void k_fm_extract(FmView V, const uint8_t* __restrict__ text_kept, const uint64_t* __restrict__ starts,
                                                    const uint64_t* __restrict__ ends, uint64_t num, const uint64_t* __restrict__ off,
                                                    const uint64_t* __restrict__ choff, uint64_t nchunks, uint8_t* __restrict__ bytes)
{
    __shared__ uint64_t s_C[257];
    __shared__ uint32_t s_col[256];
    fm_stage_tables(V, s_C, s_col);
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nchunks) return;
    const uint64_t i = last_le(choff, 0, num, j);                    // the request whose chunks hold chunk j
    uint64_t lo = starts[i], hi = ends[i];
    fm_extract_clip(V.s, lo, hi);
    const uint64_t k = lo / V.q + (j - choff[i]);
    const uint64_t r0 = fm_ld(text_kept + fm_extract_slot(V.q, V.s, k) * V.sh.w, V.sh.w);
    const uint32_t B = fm_B<LINE>(V.sh);
    uint8_t* const dst = bytes + off[i];                             // of position lo
    uint32_t acc = 0, cnt = 0;
    uint8_t* a = dst;
    fm_extract_chunk(V.q, V.s, k, lo, hi, r0,
        [&](uint64_t r, uint32_t& c) {
            const uint8_t* pb = V.blocks + r / B * fm_stride<LINE>(V.sh);
            const uint32_t rem = (uint32_t)(r % B);
            c = pb[fm_cbytes<LINE>(V.sh) + rem];
            return fm_occ_one<LINE>(V, c, s_col[c], s_C[c], pb, rem);
        },
        [&](uint64_t p, uint32_t c) {
            a = dst + (p - lo);
            acc = acc << 8 | c;
            cnt++;
            if (((uintptr_t)a & 3u) == 0) {
                if (cnt == 4) *(uint32_t*)a = acc; else fm_put_bytes(a, acc, cnt);
                cnt = 0;
            }
        });
    fm_put_bytes(a, acc, cnt);                                       // (the lower edge: a is the lane's lowest address, cnt <= 3)
}

}  // namespace sufr

namespace {

uint64_t fm_device_bytes(const sufr_hip_fm* fm)
{
    const sufr::FmView& V = fm->V;
    return sufr::fm_blocks(V.s, V.sh.B) * V.sh.stride + (V.q ? sufr::fm_mark_words(V.s) * sizeof(sufr::FmMark) + fm->samples * V.sh.w : 0) + 257 * 8 + 256 * 4;
}

int fm_alloc(sufr::Pipeline& pl, void** p, uint64_t bytes, const char* what)
{
    if (hipMalloc(p, bytes ? bytes : 1) == hipSuccess) return 0;
    *p = nullptr;
    (void)hipGetLastError();
    pl.set_error(std::string("fm_build: hipMalloc of the ") + what + " (" + std::to_string(bytes) + " bytes) failed");
    return SUFR_HIP_E_NOMEM;
}

template <typename T>
int fm_build_run(sufr_hip_ctx* ctx, const sufr_hip_index* ix, uint64_t sample, uint32_t flags, sufr_hip_fm* fm)
{
    sufr::Pipeline& pl = ctx->pl;
    const uint64_t s = ix->ix.s, n = ix->ix.n;
    int rc;
    // bwtsum: the 256 counts, the number of samples, then the tiles' mark counts (fm_tile gives more than half of the tile it
    // is given, so there are 2 s / bwt_tile + 1 tiles at most)
    if ((rc = pl.ensure(ctx->bwtbytes, s + 8)) || (rc = pl.ensure(ctx->bwtsum, (257 + 2 * s / bwt_tile(ctx) + 2) * 8))) return rc;
    uint8_t* bwt = (uint8_t*)ctx->bwtbytes.p;
    unsigned long long* counts = (unsigned long long*)ctx->bwtsum.p;
    if (hipMemsetAsync(counts, 0, 256 * 8, pl.stream) != hipSuccess) { pl.set_error("fm_build: memset failed"); return SUFR_HIP_E_HIP; }
    bwt_gather<T>(ctx, ix, bwt, counts, nullptr);
    unsigned long long h[256];
    uint8_t e = 0;
    const bool copied = hipMemcpyAsync(&e, ix->ix.text + (n - 1), 1, hipMemcpyDeviceToHost, pl.stream) == hipSuccess &&
                        hipMemcpyAsync(h, counts, 256 * 8, hipMemcpyDeviceToHost, pl.stream) == hipSuccess;
    if (hipStreamSynchronize(pl.stream) != hipSuccess || !copied) { pl.set_error("fm_build: reading the byte counts and the end byte failed"); return SUFR_HIP_E_HIP; }
    if ((rc = launch_status(pl, "fm_build"))) return rc;
    if (h[e] != 1) {
        pl.set_error("fm_build: the last byte of the text occurs " + std::to_string(h[e]) + " times among the indexed positions, not once");
        return SUFR_HIP_E_UNSUPPORTED;
    }
    uint32_t K = 0;
    for (int c = 0; c < 256; c++) K += h[c] ? 1 : 0;
    sufr::FmView& V = fm->V;
    V.s = s; V.q = sample; V.e = e; V.sh = sufr::fm_shape(K, (uint32_t)ix->sa_width);
    const sufr::FmShape sh = V.sh;
    const uint32_t tile = (uint32_t)sufr::fm_tile(sh.B, bwt_tile(ctx));
    const uint64_t ntiles = s / tile + 1, nblocks = sufr::fm_blocks(s, sh.B), nwords = sufr::fm_mark_words(s);
    if ((rc = pl.ensure(ctx->bwttab, ntiles * K * 8))) return rc;
    uint64_t* d_total = (uint64_t*)ctx->bwtsum.p + 256;
    uint64_t* t_cnt = d_total + 1;
    if ((rc = fm_alloc(pl, &fm->blocks, nblocks * sh.stride, "blocks")) || (rc = fm_alloc(pl, &fm->tabs, 257 * 8 + 256 * 4, "tables")) ||
        (sample && (rc = fm_alloc(pl, &fm->marks, nwords * sizeof(sufr::FmMark), "marks")))) return rc;
    uint64_t* d_C = (uint64_t*)fm->tabs;
    uint32_t* d_col = (uint32_t*)(d_C + 257);
    V.blocks = (const uint8_t*)fm->blocks; V.marks = (const sufr::FmMark*)fm->marks; V.C = d_C; V.col = d_col;
    if (hipMemcpyAsync(d_C + 256, &V.s, 8, hipMemcpyHostToDevice, pl.stream) != hipSuccess) { pl.set_error("fm_build: copying C[256] failed"); return SUFR_HIP_E_HIP; }
    const uint64_t wgs = batch_grid(pl);
    const uint32_t grid = (uint32_t)(ntiles < wgs ? ntiles : wgs);
    const T* sa = index_sa<T>(ix);
    uint64_t* tab = (uint64_t*)ctx->bwttab.p;
    hipLaunchKernelGGL(sufr::k_bwt_cols, dim3(1), dim3(256), 0, pl.stream, (const unsigned long long*)counts, d_C, d_col);
    hipLaunchKernelGGL(sufr::k_bwt_tile_hist, dim3(grid), dim3(256), 0, pl.stream, (const uint8_t*)bwt, s, tile, ntiles, (const uint32_t*)d_col, K, tab);
    hipLaunchKernelGGL(sufr::k_bwt_col_scan, dim3(K), dim3(1024), 0, pl.stream, tab, ntiles, K);
    hipLaunchKernelGGL(sufr::k_fm_blocks<T>, dim3(grid), dim3(256), 0, pl.stream, sa, (const uint8_t*)bwt, s, tile, ntiles, sh, (const uint32_t*)d_col,
                       (const uint64_t*)tab, sample, (uint8_t*)fm->blocks, (sufr::FmMark*)fm->marks, t_cnt);
    if (sample) {
        hipLaunchKernelGGL(sufr::k_locate_scan, dim3(1), dim3(1024), 0, pl.stream, t_cnt, ntiles, d_total);
        unsigned long long total = 0;
        if ((rc = launch_status(pl, "fm_build")) || (rc = read_totals(pl, d_total, 1, &total, "fm_build", "counting the samples failed"))) return rc;
        fm->samples = total;
        if ((rc = fm_alloc(pl, &fm->kept, total * sh.w, "samples"))) return rc;
        V.kept = (const uint8_t*)fm->kept;
        hipLaunchKernelGGL(sufr::k_fm_samples<T>, dim3(grid), dim3(256), 0, pl.stream, sa, s, tile, ntiles, (const uint64_t*)t_cnt, (sufr::FmMark*)fm->marks,
                           (T*)fm->kept);
        if (flags & SUFR_FM_TEXT) {
            if ((rc = fm_alloc(pl, &fm->text_kept, total * sh.w, "text samples"))) return rc;
            // (a suffix array writes every entry; rank 0 where an array that is none leaves one out, so that every walk stays inside)
            if (hipMemsetAsync(fm->text_kept, 0, total * sh.w, pl.stream) != hipSuccess) { pl.set_error("fm_build: memset failed"); return SUFR_HIP_E_HIP; }
            hipLaunchKernelGGL(sufr::k_fm_text_samples<T>, dim3(grid), dim3(256), 0, pl.stream, sa, s, tile, ntiles, sample, (uint64_t)total,
                               (T*)fm->text_kept);
        }
    }
    if ((rc = launch_status(pl, "fm_build"))) return rc;
    const bool tabs_back = hipMemcpyAsync(fm->h_tabs, fm->tabs, sizeof fm->h_tabs, hipMemcpyDeviceToHost, pl.stream) == hipSuccess;
    if (hipStreamSynchronize(pl.stream) != hipSuccess || !tabs_back) { pl.set_error("fm_build: the build failed"); return SUFR_HIP_E_HIP; }      // nothing reads ix from here on
    return 0;
}

int fm_check(sufr_hip_ctx* ctx, const sufr_hip_fm* fm)
{
    ctx->pl.err.clear();
    if (fm->device != ctx->pl.device) { ctx->pl.set_error("the FM-index lives on another device"); return SUFR_HIP_E_INVALID; }
    if (hipSetDevice(ctx->pl.device) != hipSuccess) { ctx->pl.set_error("hipSetDevice failed"); return SUFR_HIP_E_HIP; }
    return 0;
}

// sufr_hip_fm_build_flags (include/sufr_fm_text.h); flags == 0: sufr_hip_fm_build
int fm_build_device(sufr_hip_ctx* ctx, const sufr_hip_index* ix, uint64_t sample, uint32_t flags, sufr_hip_fm** out)
{
    if (!ctx || !ix || !out) return SUFR_HIP_E_INVALID;
    *out = nullptr;
    ctx->pl.err.clear();
    if ((flags & ~SUFR_FM_TEXT) || ((flags & SUFR_FM_TEXT) && !sample)) {
        ctx->pl.set_error("fm_build: unknown flags, or SUFR_FM_TEXT with sample == 0");
        return SUFR_HIP_E_INVALID;
    }
    if (const int rc = query_check(ctx, ix)) return rc;
    const char* why = !ix->ix.n || ix->ix.s != ix->ix.n ? "the index leaves text positions out"
                      : ix->ix.maskpos                 ? "the index was built with a seed mask"
                      : ix->built_mql                  ? "the index was built with a max_query_len"
                                                       : nullptr;
    if (why) { ctx->pl.set_error(std::string("fm_build: ") + why); return SUFR_HIP_E_UNSUPPORTED; }
    sufr_hip_fm* fm = new sufr_hip_fm;
    fm->device = ctx->pl.device;
    const int rc = by_width(ix, [&](auto w) { return fm_build_run<decltype(w)>(ctx, ix, sample, flags, fm); });
    if (rc) {
        (void)hipStreamSynchronize(ctx->pl.stream);                 // (nothing in flight writes what is freed)
        sufr_hip_fm_free(fm);
        return rc;
    }
    *out = fm;
    return 0;
}

}  // namespace

extern "C" {

void sufr_hip_fm_free(sufr_hip_fm* fm)
{
    if (!fm) return;
    (void)hipSetDevice(fm->device);
    for (void* p : {fm->blocks, fm->marks, fm->kept, fm->tabs, fm->text_kept}) if (p) (void)hipFree(p);
    delete fm;
}

int sufr_hip_fm_build(sufr_hip_ctx* ctx, const sufr_hip_index* ix, uint64_t sample, sufr_hip_fm** out) { return fm_build_device(ctx, ix, sample, 0, out); }

int sufr_hip_fm_get_info(const sufr_hip_fm* fm, sufr_fm_info* info)
{
    if (!fm || !info) return SUFR_HIP_E_INVALID;
    const sufr::FmView& V = fm->V;
    *info = sufr_fm_info{V.s, V.sh.K, V.sh.B, V.sh.stride, V.q, fm->samples, fm_device_bytes(fm), V.sh.w, V.e};
    return 0;
}

int sufr_hip_fm_search_batch_device(sufr_hip_ctx* ctx, const sufr_hip_fm* fm, const void* d_queries, const void* d_offsets, uint64_t num_queries,
                                    void* d_rank_lo, void* d_rank_hi)
{
    if (!ctx || !fm || (num_queries && (!d_queries || !d_offsets || !d_rank_lo || !d_rank_hi))) return SUFR_HIP_E_INVALID;
    if (const int rc = fm_check(ctx, fm)) return rc;
    if (!num_queries) return 0;
    const uint64_t blocks = (num_queries + 255) / 256;
    if (blocks > 0x7fffffffull) { ctx->pl.set_error("fm_search: too many queries in one batch"); return SUFR_HIP_E_INVALID; }
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(256), 0, ctx->pl.stream, fm->V, (const uint8_t*)d_queries, (const uint64_t*)d_offsets,
                           num_queries, (uint64_t*)d_rank_lo, (uint64_t*)d_rank_hi);
    };
    if (sufr::fm_is_line(fm->V.sh)) launch(sufr::k_fm_search<true>); else launch(sufr::k_fm_search<false>);
    return launch_status(ctx->pl, "fm_search");
}

int sufr_hip_fm_locate_batch_device(sufr_hip_ctx* ctx, const sufr_hip_fm* fm, const void* d_rank_lo, const void* d_rank_hi, uint64_t num_queries,
                                    uint64_t max_hits, void* d_offsets, void* d_positions, uint64_t cap, uint64_t* total_out)
{
    if (total_out) *total_out = 0;
    if (!ctx || !fm || !d_offsets || (num_queries && (!d_rank_lo || !d_rank_hi))) return SUFR_HIP_E_INVALID;
    sufr::Pipeline& pl = ctx->pl;
    int rc;
    if ((rc = fm_check(ctx, fm))) return rc;
    if (!fm->V.q) { pl.set_error("fm_locate: the index was built without samples (sample == 0)"); return SUFR_HIP_E_UNSUPPORTED; }
    const uint64_t nblk = (num_queries + sufr::LOC_BLK - 1) / sufr::LOC_BLK;
    if ((rc = pl.ensure(pl.scalars, sufr::Pipeline::SC_N * 8)) || (rc = pl.ensure(pl.partials, (size_t)(nblk + 1) * 8))) return rc;
    unsigned long long total = 0;
    uint64_t* off = (uint64_t*)d_offsets;
    if (num_queries) {
        hipLaunchKernelGGL(sufr::k_locate_counts, dim3((uint32_t)nblk), dim3(256), 0, pl.stream, (const uint64_t*)d_rank_lo, (const uint64_t*)d_rank_hi,
                           num_queries, max_hits, off, (uint64_t*)pl.partials.p);
        hipLaunchKernelGGL(sufr::k_locate_scan, dim3(1), dim3(1024), 0, pl.stream, (uint64_t*)pl.partials.p, nblk, (uint64_t*)pl.sc(sufr::Pipeline::SC_TOTAL));
        hipLaunchKernelGGL(sufr::k_locate_apply, dim3((uint32_t)((num_queries + 256) / 256)), dim3(256), 0, pl.stream, off, num_queries,
                           (const uint64_t*)pl.partials.p, (const uint64_t*)pl.sc(sufr::Pipeline::SC_TOTAL));
        if ((rc = read_totals(pl, pl.sc(sufr::Pipeline::SC_TOTAL), 1, &total, "fm_locate", "counting the matches failed"))) return rc;
    } else if (hipMemsetAsync(d_offsets, 0, 8, pl.stream) != hipSuccess) { pl.set_error("fm_locate: memset failed"); return SUFR_HIP_E_HIP; }
    if (total_out) *total_out = total;
    if (total > cap) {
        pl.set_error("fm_locate: " + std::to_string(total) + " positions, room for " + std::to_string(cap) + " (raise the capacity or set max_hits)");
        return SUFR_HIP_E_CAPACITY;
    }
    if (!total) return 0;
    if (!d_positions) return SUFR_HIP_E_INVALID;
    const uint64_t blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffull) { pl.set_error("fm_locate: too many positions for one launch"); return SUFR_HIP_E_INVALID; }
    const bool wide = fm->V.sh.w == 8;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(256), 0, pl.stream, fm->V, (const uint64_t*)d_rank_lo, (const uint64_t*)off, num_queries,
                           (uint64_t)total, wide ? (uint32_t*)nullptr : (uint32_t*)d_positions, wide ? (uint64_t*)d_positions : (uint64_t*)nullptr);
    };
    if (sufr::fm_is_line(fm->V.sh)) launch(sufr::k_fm_locate<true>); else launch(sufr::k_fm_locate<false>);
    return launch_status(pl, "fm_locate");
}

int sufr_hip_fm_approx_device(sufr_hip_ctx* ctx, const sufr_hip_fm* fm, const void* d_queries, const void* d_offsets, uint64_t num_queries,
                              uint32_t max_mismatches, uint32_t flags, uint64_t cap, void* d_query, void* d_strand, void* d_position,
                              void* d_mismatches, uint64_t* total_out)
{
    if (total_out) *total_out = 0;
    if (!ctx || !fm || (num_queries && (!d_queries || !d_offsets))) return SUFR_HIP_E_INVALID;
    sufr::Pipeline& pl = ctx->pl;
    int rc;
    if ((rc = fm_check(ctx, fm))) return rc;
    if (max_mismatches > SUFR_FM_APPROX_MAX_MISMATCHES) {
        pl.set_error("fm_approx: max_mismatches must be at most " + std::to_string(SUFR_FM_APPROX_MAX_MISMATCHES));
        return SUFR_HIP_E_INVALID;
    }
    if (!fm->V.q) { pl.set_error("fm_approx: the index was built without samples (sample == 0)"); return SUFR_HIP_E_UNSUPPORTED; }
    if (!num_queries) return 0;
    // one strand: the batch as it was given, nothing of it read here; both: the doubled batch of the seeded searches
    QueryBatch b{(const uint8_t*)d_queries, (const uint64_t*)d_offsets, num_queries, 1, 0, false};
    if ((flags & SUFR_FM_APPROX_BOTH_STRANDS) && ((rc = take_batch(ctx, nullptr, d_queries, d_offsets, num_queries, true, "fm_approx", b)) || !b.nb)) return rc;
    const uint64_t wgs = (b.nq + 255) / 256;
    if (wgs > 0x7fffffffull) { pl.set_error("fm_approx: too many queries in one batch"); return SUFR_HIP_E_INVALID; }
    // xlo, xhi: per item; xsum: the workgroups' leaves, their records, the two totals
    if ((rc = pl.ensure(ctx->xlo, b.nq * 8)) || (rc = pl.ensure(ctx->xhi, b.nq * 8)) || (rc = pl.ensure(ctx->xsum, (2 * wgs + 2) * 8))) return rc;
    uint64_t* sums = (uint64_t*)ctx->xsum.p;
    sufr::FmApproxBufs o{(uint64_t*)ctx->xlo.p, (uint64_t*)ctx->xhi.p, sums, sums + wgs, nullptr, nullptr, nullptr, 0};
    const bool line = sufr::fm_is_line(fm->V.sh);
    auto walk = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((uint32_t)wgs), dim3(256), 0, pl.stream, fm->V, b.q, b.qoff, b.nq, max_mismatches, o);
    };
    if (line) walk(sufr::k_fm_approx<true, false>); else walk(sufr::k_fm_approx<false, false>);
    hipLaunchKernelGGL(sufr::k_locate_scan, dim3(1), dim3(1024), 0, pl.stream, o.wg_leaf, wgs, sums + 2 * wgs);
    hipLaunchKernelGGL(sufr::k_locate_scan, dim3(1), dim3(1024), 0, pl.stream, o.wg_rec, wgs, sums + 2 * wgs + 1);
    unsigned long long totals[2] = {0, 0};               // leaves, records
    if ((rc = launch_status(pl, "fm_approx")) || (rc = read_totals(pl, sums + 2 * wgs, 2, totals, "fm_approx", "counting the records failed"))) return rc;
    if ((rc = records_fit(pl, "fm_approx", "records", totals[1], cap, total_out)) || !totals[1]) return rc;
    if (any_null({d_query, d_strand, d_position, d_mismatches})) return SUFR_HIP_E_INVALID;
    const uint64_t nleaves = totals[0], nrec = totals[1], blocks = (nrec + 255) / 256;
    if (blocks > 0x7fffffffull) { pl.set_error("fm_approx: too many records for one launch"); return SUFR_HIP_E_INVALID; }
    if ((rc = pl.ensure(ctx->xcand, 3 * nleaves * 8))) return rc;
    o.leaf_off = (uint64_t*)ctx->xcand.p; o.leaf_lo = o.leaf_off + nleaves; o.leaf_tag = o.leaf_lo + nleaves; o.nleaves = nleaves;
    if (line) walk(sufr::k_fm_approx<true, true>); else walk(sufr::k_fm_approx<false, true>);
    // the leaves are the queries of the locate, their record offsets its offsets; the positions are stored as u64
    auto locate = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(256), 0, pl.stream, fm->V, (const uint64_t*)o.leaf_lo, (const uint64_t*)o.leaf_off, nleaves,
                           nrec, (uint32_t*)nullptr, (uint64_t*)d_position);
    };
    if (line) locate(sufr::k_fm_locate<true>); else locate(sufr::k_fm_locate<false>);
    hipLaunchKernelGGL(sufr::k_fm_approx_expand, dim3((uint32_t)blocks), dim3(256), 0, pl.stream, (const uint64_t*)o.leaf_off, (const uint64_t*)o.leaf_tag,
                       nleaves, nrec, (uint32_t)b.both, (uint64_t*)d_query, (uint8_t*)d_strand, (uint8_t*)d_mismatches);
    return launch_status(pl, "fm_approx");
}

int sufr_hip_fm_approx(sufr_hip_ctx* ctx, const sufr_hip_fm* fm, const uint8_t* queries, const uint64_t* offsets, uint64_t num_queries,
                       uint32_t max_mismatches, uint32_t flags, uint64_t cap, uint64_t* query, uint8_t* strand, uint64_t* position,
                       uint8_t* mismatches, uint64_t* total_out)
{
    if (total_out) *total_out = 0;
    if (!ctx || !fm || (num_queries && !offsets)) return SUFR_HIP_E_INVALID;
    if (const int rc = fm_check(ctx, fm)) return rc;
    if (!num_queries) return sufr_hip_fm_approx_device(ctx, fm, nullptr, nullptr, 0, max_mismatches, flags, cap, nullptr, nullptr, nullptr, nullptr, total_out);
    return staged_records(ctx, "FM k-mismatch", queries, offsets, num_queries, cap, {{query, 8}, {strand, 1}, {position, 8}, {mismatches, 1}}, 0, total_out,
                          [&](const void* d_q, const void* d_off, void* const* col, uint64_t* total) {
        return sufr_hip_fm_approx_device(ctx, fm, d_q, d_off, num_queries, max_mismatches, flags, cap, col[0], col[1], col[2], col[3], total);
    });
}

// ---- include/sufr_fm_text.h: text samples, extract and the copies between host and device (DESIGN.md section 25) ----------
int sufr_hip_fm_build_flags(sufr_hip_ctx* ctx, const sufr_hip_index* ix, uint64_t sample, uint32_t flags, sufr_hip_fm** out)
{
    return fm_build_device(ctx, ix, sample, flags, out);
}

int sufr_hip_fm_get_text_info(const sufr_hip_fm* fm, sufr_fm_text_info* info)
{
    if (!fm || !info) return SUFR_HIP_E_INVALID;
    const sufr::FmView& V = fm->V;
    const uint64_t ts = fm->text_kept ? fm->samples : 0;
    *info = sufr_fm_text_info{ts, ts * V.sh.w, sufr::fm_file_layout(V.sh, V.s, V.q, fm->samples, fm->text_kept != nullptr, 0, 0).bytes};
    return 0;
}

int sufr_hip_fm_extract_batch_device(sufr_hip_ctx* ctx, const sufr_hip_fm* fm, const void* d_starts, const void* d_ends, uint64_t num,
                                     void* d_offsets, void* d_bytes, uint64_t cap, uint64_t* total_out)
{
    if (total_out) *total_out = 0;
    if (!ctx || !fm || !d_offsets || (num && (!d_starts || !d_ends))) return SUFR_HIP_E_INVALID;
    sufr::Pipeline& pl = ctx->pl;
    int rc;
    if ((rc = fm_check(ctx, fm))) return rc;
    if (!fm->text_kept) { pl.set_error("fm_extract: the index was built without SUFR_FM_TEXT"); return SUFR_HIP_E_UNSUPPORTED; }
    if (!num) {
        if (hipMemsetAsync(d_offsets, 0, 8, pl.stream) != hipSuccess) { pl.set_error("fm_extract: memset failed"); return SUFR_HIP_E_HIP; }
        return 0;
    }
    const uint64_t wgs = (num + 255) / 256;
    if (wgs > 0x7fffffffull) { pl.set_error("fm_extract: too many requests in one batch"); return SUFR_HIP_E_INVALID; }
    // xlo: the chunks in front of every request; xsum: the workgroups' bytes, their chunks, the two totals
    if ((rc = pl.ensure(ctx->xlo, (num + 1) * 8)) || (rc = pl.ensure(ctx->xsum, (2 * wgs + 2) * 8))) return rc;
    uint64_t* off = (uint64_t*)d_offsets;
    uint64_t* choff = (uint64_t*)ctx->xlo.p;
    uint64_t* sums = (uint64_t*)ctx->xsum.p;
    const sufr::FmView& V = fm->V;
    hipLaunchKernelGGL(sufr::k_fm_extract_counts, dim3((uint32_t)wgs), dim3(256), 0, pl.stream, (const uint64_t*)d_starts, (const uint64_t*)d_ends, num,
                       V.s, V.q, off, choff, sums, sums + wgs);
    hipLaunchKernelGGL(sufr::k_locate_scan, dim3(1), dim3(1024), 0, pl.stream, sums, wgs, sums + 2 * wgs);
    hipLaunchKernelGGL(sufr::k_locate_scan, dim3(1), dim3(1024), 0, pl.stream, sums + wgs, wgs, sums + 2 * wgs + 1);
    hipLaunchKernelGGL(sufr::k_fm_extract_apply, dim3((uint32_t)((num + 256) / 256)), dim3(256), 0, pl.stream, off, choff, num, (const uint64_t*)sums,
                       (const uint64_t*)(sums + wgs), (const uint64_t*)(sums + 2 * wgs));
    unsigned long long totals[2] = {0, 0};               // bytes, chunks
    if ((rc = launch_status(pl, "fm_extract")) || (rc = read_totals(pl, sums + 2 * wgs, 2, totals, "fm_extract", "counting the bytes failed"))) return rc;
    if ((rc = records_fit(pl, "fm_extract", "bytes", totals[0], cap, total_out)) || !totals[0]) return rc;
    if (!d_bytes) return SUFR_HIP_E_INVALID;
    const uint64_t blocks = (totals[1] + 255) / 256;
    if (blocks > 0x7fffffffull) { pl.set_error("fm_extract: too many chunks for one launch"); return SUFR_HIP_E_INVALID; }
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(256), 0, pl.stream, V, (const uint8_t*)fm->text_kept, (const uint64_t*)d_starts,
                           (const uint64_t*)d_ends, num, (const uint64_t*)off, (const uint64_t*)choff, (uint64_t)totals[1], (uint8_t*)d_bytes);
    };
    if (sufr::fm_is_line(V.sh)) launch(sufr::k_fm_extract<true>); else launch(sufr::k_fm_extract<false>);
    return launch_status(pl, "fm_extract");
}

int sufr_hip_fm_extract_batch(sufr_hip_ctx* ctx, const sufr_hip_fm* fm, const uint64_t* starts, const uint64_t* ends, uint64_t num, uint64_t* offsets,
                              uint8_t* bytes, uint64_t cap, uint64_t* total_out)
{
    if (total_out) *total_out = 0;
    if (!ctx || !fm || !offsets || (num && (!starts || !ends))) return SUFR_HIP_E_INVALID;
    if (const int rc = fm_check(ctx, fm)) return rc;
    if (!fm->text_kept) { ctx->pl.set_error("fm_extract: the index was built without SUFR_FM_TEXT"); return SUFR_HIP_E_UNSUPPORTED; }
    if (!num) { offsets[0] = 0; return 0; }
    // the requests are the staged bytes: starts | ends, one "query" of 16 num bytes; the offsets come back from the extra room
    std::vector<uint64_t> req(2 * num);
    memcpy(req.data(), starts, num * 8);
    memcpy(req.data() + num, ends, num * 8);
    const uint64_t req_bytes[1] = {16 * num};
    return staged_records(ctx, "FM extract", (const uint8_t*)req.data(), req_bytes, 0, cap, {{bytes, 1}}, (num + 1) * 8, total_out,
                          [&](const void* d_req, const void*, void* const* col, uint64_t* total) {
        int rc = sufr_hip_fm_extract_batch_device(ctx, fm, d_req, (const uint64_t*)d_req + num, num, col[1], col[0], cap, total);
        if ((!rc || rc == SUFR_HIP_E_CAPACITY) && (hipMemcpyAsync(offsets, col[1], (num + 1) * 8, hipMemcpyDeviceToHost, ctx->pl.stream) != hipSuccess ||
                                                   hipStreamSynchronize(ctx->pl.stream) != hipSuccess)) rc = SUFR_HIP_E_HIP;
        return rc;
    });
}

int sufr_hip_fm_upload(sufr_hip_ctx* ctx, const sufr_fm* h, sufr_hip_fm** out)
{
    if (!ctx || !h || !out) return SUFR_HIP_E_INVALID;
    *out = nullptr;
    sufr::Pipeline& pl = ctx->pl;
    pl.err.clear();
    if (hipSetDevice(pl.device) != hipSuccess) { pl.set_error("hipSetDevice failed"); return SUFR_HIP_E_HIP; }
    sufr_hip_fm* fm = new sufr_hip_fm;
    fm->device = pl.device;
    fm->samples = h->samples;
    std::vector<uint8_t> tabs(sufr::FM_TABLE_BYTES);
    memcpy(tabs.data(), h->C, 257 * 8);
    memcpy(tabs.data() + 257 * 8, h->col, 256 * 4);
    struct Part { void** d; const void* src; uint64_t bytes; const char* what; bool have; };
    const Part parts[] = {{&fm->blocks, h->blocks.data(), h->blocks.size(), "blocks", true},
                          {&fm->tabs, tabs.data(), tabs.size(), "tables", true},
                          {&fm->marks, h->marks.data(), h->marks.size() * sizeof(sufr::FmMark), "marks", h->q != 0},
                          {&fm->kept, h->kept.data(), h->kept.size(), "samples", h->q != 0},
                          {&fm->text_kept, h->text_kept.data(), h->text_kept.size(), "text samples", !h->text_kept.empty()}};
    int rc = 0;
    for (const Part& p : parts) {
        if (!p.have) continue;
        if ((rc = fm_alloc(pl, p.d, p.bytes, p.what))) break;
        if (p.bytes && hipMemcpy(*p.d, p.src, p.bytes, hipMemcpyHostToDevice) != hipSuccess) {
            pl.set_error(std::string("fm_upload: copying the ") + p.what + " failed");
            rc = SUFR_HIP_E_HIP;
            break;
        }
    }
    if (rc) { sufr_hip_fm_free(fm); return rc; }
    memcpy(fm->h_tabs, tabs.data(), sizeof fm->h_tabs);
    uint64_t* d_C = (uint64_t*)fm->tabs;
    fm->V = sufr::FmView{(const uint8_t*)fm->blocks, (const sufr::FmMark*)fm->marks, (const uint8_t*)fm->kept, d_C, (const uint32_t*)(d_C + 257),
                         h->s, h->q, h->sh, h->e};
    *out = fm;
    return 0;
}

int sufr_hip_fm_download(sufr_hip_ctx* ctx, const sufr_hip_fm* fm, sufr_fm** out)
{
    if (!ctx || !fm || !out) return SUFR_HIP_E_INVALID;
    *out = nullptr;
    if (const int rc = fm_check(ctx, fm)) return rc;
    sufr::Pipeline& pl = ctx->pl;
    if (hipStreamSynchronize(pl.stream) != hipSuccess) { pl.set_error("fm_download: the stream failed"); return SUFR_HIP_E_HIP; }
    const sufr::FmView& V = fm->V;
    const sufr::FmShape sh = V.sh;
    sufr_fm* h = new sufr_fm;
    h->sh = sh; h->s = V.s; h->q = V.q; h->samples = fm->samples; h->e = V.e;
    std::vector<uint8_t> tabs(sufr::FM_TABLE_BYTES);
    h->blocks.resize(sufr::fm_blocks(V.s, sh.B) * sh.stride);
    if (V.q) { h->marks.resize(sufr::fm_mark_words(V.s)); h->kept.resize(fm->samples * sh.w); }
    if (fm->text_kept) h->text_kept.resize(fm->samples * sh.w);
    struct Part { void* dst; const void* d; uint64_t bytes; };
    const Part parts[] = {{h->blocks.data(), fm->blocks, h->blocks.size()}, {tabs.data(), fm->tabs, tabs.size()},
                          {h->marks.data(), fm->marks, h->marks.size() * sizeof(sufr::FmMark)}, {h->kept.data(), fm->kept, h->kept.size()},
                          {h->text_kept.data(), fm->text_kept, h->text_kept.size()}};
    for (const Part& p : parts)
        if (p.bytes && hipMemcpy(p.dst, p.d, p.bytes, hipMemcpyDeviceToHost) != hipSuccess) {
            pl.set_error("fm_download: copying the index failed");
            delete h;
            return SUFR_HIP_E_HIP;
        }
    memcpy(h->C, tabs.data(), 257 * 8);
    memcpy(h->col, tabs.data() + 257 * 8, 256 * 4);
    // what the file format wants zero, whoever built the index: the checkpoint bytes behind K w, the BWT bytes behind s and
    // the mark bits behind s
    const uint64_t nblocks = h->blocks.size() / sh.stride;
    if (sh.K * sh.w < sh.cbytes)
        for (uint64_t j = 0; j < nblocks; j++) memset(h->blocks.data() + j * sh.stride + sh.K * sh.w, 0, sh.cbytes - sh.K * sh.w);
    memset(h->blocks.data() + (nblocks - 1) * sh.stride + sh.cbytes + V.s % sh.B, 0, sh.B - V.s % sh.B);
    if (V.q && (V.s & 63u)) h->marks.back().bits &= ((uint64_t)1 << (V.s & 63u)) - 1;
    *out = h;
    return 0;
}

}  // extern "C"

// ---- include/sufr_fm_match.h: matching statistics and SMEMs on a pair of indexes (DESIGN.md section 26) ---------------------
namespace {

static constexpr uint32_t FM_MS_SLAB = 32;               // the bytes of a lane of k_fm_ms (profiles/fm_match_bench.txt)

// both indexes on the context's device, and a pair (sufr_fm_match.h): from the host copies of the tables
int fm_pair_check(sufr_hip_ctx* ctx, const sufr_hip_fm* fwd, const sufr_hip_fm* rev)
{
    int rc;
    if ((rc = fm_check(ctx, fwd)) || (rc = fm_check(ctx, rev))) return rc;
    const sufr::FmView &F = fwd->V, &R = rev->V;
    if (F.s == R.s && F.sh.w == R.sh.w && F.e == R.e && !memcmp(fwd->h_tabs, rev->h_tabs, sizeof fwd->h_tabs)) return 0;
    ctx->pl.set_error("not an index of the reversed text");
    return SUFR_HIP_E_INVALID;
}

template <uint32_t G>
void fm_ms_launch(sufr_hip_ctx* ctx, const sufr_hip_fm* fwd, const sufr_hip_fm* rev, const void* d_queries, const void* d_offsets, uint64_t nq, void* d_ms)
{
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(batch_grid(ctx->pl)), dim3(256), 0, ctx->pl.stream, fwd->V, rev->V, (const uint8_t*)d_queries,
                           (const uint64_t*)d_offsets, nq, (uint32_t*)d_ms);
    };
    if (sufr::fm_is_line(fwd->V.sh)) launch(sufr::k_fm_ms<true, G>); else launch(sufr::k_fm_ms<false, G>);
}

}  // namespace

extern "C" {

int sufr_hip_fm_matching_stats_device(sufr_hip_ctx* ctx, const sufr_hip_fm* fwd, const sufr_hip_fm* rev, const void* d_queries, const void* d_offsets,
                                      uint64_t num_queries, void* d_ms)
{
    if (!ctx || !fwd || !rev || (num_queries && (!d_queries || !d_offsets || !d_ms))) return SUFR_HIP_E_INVALID;
    if (const int rc = fm_pair_check(ctx, fwd, rev)) return rc;
    if (!num_queries) return 0;
#ifdef SUFR_HIP_PROBES
    // the probes build has the other slabs too, for the table FM_MS_SLAB was chosen from; no result depends on the slab
    const char* v = getenv("SUFR_PROBE_FM_MS_SLAB");
    switch (v ? atoi(v) : 0) {
        case 64: fm_ms_launch<64>(ctx, fwd, rev, d_queries, d_offsets, num_queries, d_ms); break;
        case 128: fm_ms_launch<128>(ctx, fwd, rev, d_queries, d_offsets, num_queries, d_ms); break;
        case 256: fm_ms_launch<256>(ctx, fwd, rev, d_queries, d_offsets, num_queries, d_ms); break;
        default: fm_ms_launch<FM_MS_SLAB>(ctx, fwd, rev, d_queries, d_offsets, num_queries, d_ms); break;
    }
#else
    fm_ms_launch<FM_MS_SLAB>(ctx, fwd, rev, d_queries, d_offsets, num_queries, d_ms);
#endif
    return launch_status(ctx->pl, "fm_matching_stats");
}

int sufr_hip_fm_smems_device(sufr_hip_ctx* ctx, const sufr_hip_fm* fwd, const sufr_hip_fm* rev, const void* d_queries, const void* d_offsets,
                             uint64_t num_queries, uint32_t min_len, void* d_ms, uint64_t cap, void* d_query, void* d_query_offset, void* d_length,
                             void* d_rank_lo, void* d_rank_hi, uint64_t* total_out)
{
    if (total_out) *total_out = 0;
    if (!ctx || !fwd || !rev || (num_queries && (!d_queries || !d_offsets || !d_ms))) return SUFR_HIP_E_INVALID;
    int rc;
    if ((rc = fm_pair_check(ctx, fwd, rev))) return rc;
    if (min_len == 0) { ctx->pl.set_error("fm_smems: min_len must be at least 1"); return SUFR_HIP_E_INVALID; }
    if (!num_queries) return 0;
    if ((rc = sufr_hip_fm_matching_stats_device(ctx, fwd, rev, d_queries, d_offsets, num_queries, d_ms))) return rc;
    // the rank range of every SMEM: the backward search of the packed slices on the index of the text
    return smems_from_stats(ctx, d_queries, d_offsets, num_queries, min_len, d_ms, cap, d_query, d_query_offset, d_length, d_rank_lo, d_rank_hi, total_out,
                            [&](const void* packed, const uint64_t* slice_off, uint64_t nsm) {
        return sufr_hip_fm_search_batch_device(ctx, fwd, packed, slice_off, nsm, d_rank_lo, d_rank_hi);
    });
}

int sufr_hip_fm_smems(sufr_hip_ctx* ctx, const sufr_hip_fm* fwd, const sufr_hip_fm* rev, const uint8_t* queries, const uint64_t* offsets,
                      uint64_t num_queries, uint32_t min_len, uint64_t cap, uint64_t* query, uint32_t* query_offset, uint32_t* length, uint64_t* rank_lo,
                      uint64_t* rank_hi, uint64_t* total_out)
{
    if (total_out) *total_out = 0;
    if (!ctx || !fwd || !rev || (num_queries && !offsets)) return SUFR_HIP_E_INVALID;
    if (const int rc = fm_pair_check(ctx, fwd, rev)) return rc;
    if (min_len == 0) { ctx->pl.set_error("fm_smems: min_len must be at least 1"); return SUFR_HIP_E_INVALID; }
    if (!num_queries) return 0;
    // the matching statistics (4 bytes per query byte) stay on the device: they ride behind the record columns
    return staged_records(ctx, "FM SMEM", queries, offsets, num_queries, cap, {{query, 8}, {query_offset, 4}, {length, 4}, {rank_lo, 8}, {rank_hi, 8}},
                          offsets[num_queries] * 4, total_out, [&](const void* d_q, const void* d_off, void* const* col, uint64_t* total) {
        return sufr_hip_fm_smems_device(ctx, fwd, rev, d_q, d_off, num_queries, min_len, col[5], cap, col[0], col[1], col[2], col[3], col[4], total);
    });
}

}  // extern "C"
