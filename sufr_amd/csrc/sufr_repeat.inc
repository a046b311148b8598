// sufr_repeat.inc -- maximal and supermaximal repeats from the SA, the LCP and the text of a device-resident index (included
// by sufr_kernels.hip after sufr_kmer.inc; include/sufr_repeat.h, DESIGN.md section 19).
//
// An interval [a, b) is found from its representative rank by two nearest-smaller-value searches over the clipped LCP l.
// Intervals may be as long as the array (all-A, the N^21 bucket of a genome), so nothing is local to a tile: the searches
// walk a min pyramid of fan-out 64 over l, and the "are the left symbols all one" question is a difference of two popcount
// prefixes.  The arithmetic -- the clip, the pyramid's indices, the searches, the prefix test, the supermaximal walk -- is
// sufr_repeat_scan.h, which the host path and tests/repeat_shim.cpp compile too; this file only moves the data.
//
// k_rep_fold     one pass over SA, LCP and the text.  A wave takes 64 consecutive ranks: l[r] (stored only when there are
//                several sequences; with one, l is the LCP array), the gather of T[SA[r] - 1] (one byte per rank, the one
//                random access), the "left symbol differs from the previous rank's" and "is a sequence start" words by
//                __ballot, the wave's minimum of l (level 1 of the pyramid) and, per tile, the exclusive popcount prefix
//                of the words with the tile's totals.  The rank before a wave's first is loaded by its lane 0.
// k_locate_scan  (sufr_search.inc) one workgroup: the tile totals to bases, twice.
// k_rep_addbase  the tile bases onto the word prefixes (s / 64 entries).
// k_rep_level    one launch per level >= 2: a wave per entry, 64 entries of the level below.
// k_rep_find     <T, MODE, SEQS>, the one find pass of repeats (SEQS false) and of shared and common (sufr_shared.inc, SEQS
//                true).  A lane per rank: rep_interval -- l[r] >= min_len, the left search with <= (the rank is the
//                representative iff the value found is smaller, and that index is a), the right search for b -- then the
//                count filter and the kind (rep_keep) and, with SEQS, seqs from two reads of P and its filter.  The l of up
//                to 4096 ranks of the tile, and their level-1 entries, are staged in LDS and searched there first
//                (RepStaged::stage over rep_tile_window); a search that leaves the window reads the pyramid in memory and
//                descends again.  REP_COUNT: kept ranks per tile and the tile's RepBest (longest / largest count / largest
//                seqs), reduced over the workgroup by wg_reduce_op over RepBestOp.  REP_WRITE: the same decisions,
//                compacted in rank order behind the tile's base.  REP_PROFILE (SEQS only): an atomic max per interval that
//                raises its entry.  The cost of a rank is bounded by 2 x 64 x levels reads per search whatever b - a is; only
//                the supermaximal walk (rep_supermaximal) is longer, and says when.
// k_tile_best    <Op> one workgroup: the stats from the tiles' candidates by tile_reduce -- RepBestOp<4 or 5> here,
//                SumBestOp<1> for sufr_lz.inc and sufr_bwt.inc.
// The scans and reductions are those of sufr_scan.inc (DESIGN.md section 10.2).
// A workgroup takes tiles t = blockIdx.x, blockIdx.x + gridDim.x, ...; no scratch; k_rep_find holds 16.4 KB of LDS (32-bit
// arrays) or 32.7 KB (64-bit) without SEQS, 16.8 / 33.5 KB with it; k_tile_best 16 candidates.
// Host: repeats_prepare (the fold, the scans, the levels: RepPrep, which also owns the scratch of the find pass) and
// repeats_find<T, SEQS> (counting launch, k_locate_scan, k_tile_best, report_total, writing launch), which sufr_shared.inc
// calls with SEQS set.

#include "sufr_repeat_scan.h"
#include "sufr_shared_scan.h"

namespace sufr {

static constexpr uint32_t REP_TILE_MAX = 16384;         // ranks of a tile at most: 256 words, one per lane
static constexpr uint32_t REP_STAGE = 4096;             // ranks of l a workgroup keeps in LDS at a time: one block of level 1

template <typename T>
struct RepAcc {
    const T *l0, *up, *sa_;                             // l (LCP or its clipped copy), the coarser levels, the suffix array
    uint64_t s;
    __device__ __forceinline__ uint64_t at(uint32_t level, uint64_t off, uint64_t i) const      // off: rep_level_offset(s, level)
    {
        if (level) return (uint64_t)up[off + i];
        return i ? (uint64_t)l0[i] : 0;
    }
    __device__ __forceinline__ uint64_t sa(uint64_t r) const { return (uint64_t)sa_[r]; }
};

// a window of level 0 and of the level-1 entries above it: ranks [w0, w0 + len), w0 a multiple of 64, and vlen words
struct RepWindow { uint64_t w0, len, vlen; };

// len ranks from w0 on of an array of s (level 1 exists when s > 64)
__device__ __forceinline__ RepWindow rep_window(uint64_t w0, uint64_t len, uint64_t s) { return RepWindow{w0, len, s > 64 ? (len + 63) / 64 : 0}; }

// the window of tile t at step `it` (a multiple of `stage`): `stage` ranks, or what is left of the tile or of the array
__device__ __forceinline__ RepWindow rep_tile_window(uint64_t t, uint32_t tile, uint32_t it, uint32_t stage, uint64_t s)
{
    const uint64_t w0 = t * tile + it, left = tile - it < stage ? tile - it : stage;
    return rep_window(w0, w0 + left < s ? left : s - w0, s);
}

// RepAcc behind a window of l and of level 1 in LDS.  A search reads the window first -- a scan step is then an LDS read,
// not a dependent global load -- and what lies outside it from memory.
template <typename T, typename G = RepAcc<T>>         // (G: what lies behind the window; sufr_lz.inc stages its own arrays)
struct RepStaged {
    G g;
    T *s_l, *s_l1;
    uint64_t w0, len, v0, vlen;                         // the window of level 0 and of level 1: first index and entries
    // fills the window, all 256 lanes of the workgroup; the caller's barriers stand before and after
    __device__ __forceinline__ void stage(const RepWindow& win)
    {
        for (uint64_t i = threadIdx.x; i < win.len; i += 256) s_l[i] = (T)g.at(0, 0, win.w0 + i);
        if (threadIdx.x < win.vlen) s_l1[threadIdx.x] = (T)g.at(1, 0, (win.w0 >> 6) + threadIdx.x);
        w0 = win.w0; len = win.len; v0 = win.w0 >> 6; vlen = win.vlen;
    }
    __device__ __forceinline__ uint64_t at(uint32_t level, uint64_t off, uint64_t i) const
    {
        // (the empty asm keeps the compiler from folding the LDS read and the global read into one flat load of a selected
        // pointer)
        if (level == 0 && i - w0 < len) { T x = s_l[i - w0]; asm volatile("" : "+v"(x)); return (uint64_t)x; }
        if (level == 1 && i - v0 < vlen) { T x = s_l1[i - v0]; asm volatile("" : "+v"(x)); return (uint64_t)x; }
        return g.at(level, off, i);
    }
    __device__ __forceinline__ uint64_t sa(uint64_t r) const { return g.sa(r); }
};

struct RepBits { const uint64_t *dw, *dp, *sw, *sp; };   // "differs" words and prefix, "sequence start" words and prefix

template <typename T>
__global__ __launch_bounds__(256) void k_rep_fold(const T* __restrict__ sa, const T* __restrict__ lcp, const uint8_t* __restrict__ text,
                                                  uint64_t s, KmerSeqs q, uint32_t tile, uint64_t ntiles, T* __restrict__ ell,
                                                  T* __restrict__ lv1, uint64_t* __restrict__ dw, uint64_t* __restrict__ sw,
                                                  uint64_t* __restrict__ dp, uint64_t* __restrict__ sp, uint64_t* __restrict__ t_d,
                                                  uint64_t* __restrict__ t_s)
{
    __shared__ uint32_t s_pd[256], s_ps[256], s_w[4];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, nw = tile >> 6;      // (tile: a multiple of 256)
    const uint64_t n1 = (s + 63) / 64;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        for (uint32_t j = w; j < nw; j += 4) {
            const uint64_t r = t * tile + (uint64_t)j * 64 + lane;
            uint64_t v = ~(uint64_t)0, room = 0;
            uint32_t lam = 256;                          // 256: a symbol of its own (a sequence start); ranks past the end too
            bool start = false;
            if (r < s) {
                const uint64_t p = (uint64_t)sa[r];
                start = rep_is_start(q.starts, q.num, q.n, p);
                if (!start) lam = text[p - 1];
                if (ell) room = rep_room(q.starts, q.num, q.n, p);
            }
            uint32_t plam = __shfl_up(lam, 1);
            uint64_t proom = __shfl_up(room, 1);
            if (lane == 0 && r >= 1 && r < s) {          // the previous rank is another wave's: load it
                const uint64_t pp = (uint64_t)sa[r - 1];
                plam = rep_is_start(q.starts, q.num, q.n, pp) ? 256 : text[pp - 1];
                if (ell) proom = rep_room(q.starts, q.num, q.n, pp);
            }
            if (r < s) {
                v = r == 0 ? 0 : ell ? rep_clip((uint64_t)lcp[r], proom, room) : (uint64_t)lcp[r];
                if (ell) ell[r] = (T)v;
            }
            const bool diff = r >= 1 && r < s && (lam == 256 || plam == 256 || lam != plam);
            const uint64_t D = __ballot(diff), S = __ballot(start);
            for (int o = 32; o > 0; o >>= 1) { const uint64_t u = __shfl_xor(v, o); if (u < v) v = u; }
            if (lane == 0) {
                const uint64_t word = t * nw + j;
                dw[word] = D; sw[word] = S;
                s_pd[j] = (uint32_t)__builtin_popcountll(D); s_ps[j] = (uint32_t)__builtin_popcountll(S);
                if (lv1 && word < n1) lv1[word] = (T)v;
            }
        }
        __syncthreads();
        const uint32_t cd = threadIdx.x < nw ? s_pd[threadIdx.x] : 0, cs = threadIdx.x < nw ? s_ps[threadIdx.x] : 0;
        const WgScan<uint32_t> d = wg_scan_op<SumOp<uint32_t>, 4>(cd, s_w), e = wg_scan_op<SumOp<uint32_t>, 4>(cs, s_w);
        if (threadIdx.x < nw) { dp[t * nw + threadIdx.x] = d.before; sp[t * nw + threadIdx.x] = e.before; }
        if (threadIdx.x == 0) { t_d[t] = d.total; t_s[t] = e.total; }
    }
}

__global__ __launch_bounds__(256) void k_rep_addbase(uint64_t* __restrict__ dp, uint64_t* __restrict__ sp, uint64_t nwords, uint32_t nw,
                                                     const uint64_t* __restrict__ t_d, const uint64_t* __restrict__ t_s)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nwords; i += stride) { dp[i] += t_d[i / nw]; sp[i] += t_s[i / nw]; }
}

// out[i] = min of in[64 i .. 64 i + 64), a wave per entry
template <typename T>
__global__ __launch_bounds__(256) void k_rep_level(const T* __restrict__ in, uint64_t n_in, T* __restrict__ out, uint64_t n_out)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * 4;
    for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n_out; i += stride) {
        const uint64_t j = i * 64 + lane;
        uint64_t v = j < n_in ? (uint64_t)in[j] : ~(uint64_t)0;
        for (int o = 32; o > 0; o >>= 1) { const uint64_t u = __shfl_xor(v, o); if (u < v) v = u; }
        if (lane == 0) out[i] = (T)v;
    }
}

// kind, min_len and the count filter of sufr_repeat.h; min_seqs / max_seqs: the filter of sufr_shared.h (0, 0 where no
// sequences are counted)
struct RepFilter { uint32_t kind; uint64_t min_len, min_count, max_count, min_seqs, max_seqs; };
enum { REP_COUNT = 0, REP_WRITE = 1, REP_PROFILE = 2 };

// a RepBest as NCOL words `stride` apart: len, rep, rank, cnt and, with 5 columns, seq
template <int NCOL>
__device__ __forceinline__ RepBest rep_best_get(const uint64_t* p, uint32_t stride = 1)
{
    return RepBest{p[0], p[stride], p[2 * stride], p[3 * stride], NCOL > 4 ? p[4 * stride] : 0};
}
template <int NCOL>
__device__ __forceinline__ void rep_best_put(uint64_t* p, const RepBest& b, uint32_t stride = 1)
{
    p[0] = b.len; p[stride] = b.rep; p[2 * stride] = b.rank; p[3 * stride] = b.cnt;
    if (NCOL > 4) p[4 * stride] = b.seq;
}

// RepBest::merge over the NCOL words of a candidate (commutative: sufr_repeat_scan.h).  get / stats: what k_tile_best reads
// of a tile and writes behind the total -- {longest, longest_rank, max_count (, max_seqs)}
template <int NCOL>
struct RepBestOp {
    static constexpr int COLS = NCOL;
    struct V { uint64_t c[NCOL]; };
    static __device__ __forceinline__ V make(const RepBest& b) { V v; rep_best_put<NCOL>(v.c, b); return v; }
    static __device__ __forceinline__ V identity() { return make(RepBest{0, 0, 0, 0, 0}); }
    static __device__ __forceinline__ V combine(const V& a, const V& b)
    {
        RepBest x = rep_best_get<NCOL>(a.c);
        x.merge(rep_best_get<NCOL>(b.c));
        return make(x);
    }
    static __device__ __forceinline__ V get(const uint64_t* p) { return make(rep_best_get<NCOL>(p)); }
    static __device__ __forceinline__ void stats(uint64_t* out, const V& v)
    {
        out[0] = v.c[0]; out[1] = v.c[2]; out[2] = v.c[3];
        if (NCOL > 4) out[3] = v.c[4];
    }
};

// NSUM sums and the best (length, at) by rep_better: longer wins, ties go to the smaller `at` -- a total order on the
// candidates of length > 0.  rep_better never prefers a length of 0, so between two values of length 0 combine keeps the
// left one's `at`: the operator is commutative as long as every value of length 0 carries at = 0, like the identity.  The
// lane loops of k_lz_emit and k_bwt_runs set `at` only together with a length > 0, so that holds for them and for the
// tiles they write.  The tails of those two kernels, and with one sum their candidates per tile.
template <int NSUM>
struct SumBestOp {
    static constexpr int COLS = NSUM + 2;
    struct V { uint64_t sum[NSUM], len, at; };
    static __device__ __forceinline__ V identity() { V v; for (int n = 0; n < NSUM; n++) v.sum[n] = 0; v.len = v.at = 0; return v; }
    static __device__ __forceinline__ V combine(const V& a, const V& b)
    {
        V v = a;
        for (int n = 0; n < NSUM; n++) v.sum[n] += b.sum[n];
        if (rep_better(b.len, b.at, a.len, a.at)) { v.len = b.len; v.at = b.at; }
        return v;
    }
    static __device__ __forceinline__ V get(const uint64_t* p) { V v; for (int n = 0; n < NSUM; n++) v.sum[n] = p[n]; v.len = p[NSUM]; v.at = p[NSUM + 1]; return v; }
    static __device__ __forceinline__ void stats(uint64_t* out, const V& v) { for (int n = 0; n < NSUM; n++) out[n] = v.sum[n]; out[NSUM] = v.len; out[NSUM + 1] = v.at; }
};

// The find pass of repeats (SEQS false: 4 columns; P, o_seqs, best and the seqs filter are not looked at) and of shared and
// common (SEQS true: 5 columns; seqs from two reads of P, then its filter).
// REP_COUNT: t_cnt[t] = kept ranks of tile t, t_best[NCOL t ..] = the tile's RepBest.  REP_WRITE: t_cnt[t] is the tile's
// base; the records go to o_rank / o_count / o_len (/ o_seqs) in rank order.  REP_PROFILE (SEQS only): best[k - 1] = the
// longest interval of exactly k sequences (nbest entries, zeroed before the launch) -- the entry is read first and the atomic
// max issued only when v is larger: the value only grows, so a stale read costs at most an atomic that changes nothing.
template <typename T, int MODE, bool SEQS>
__global__ __launch_bounds__(256) void k_rep_find(RepAcc<T> gacc, const uint8_t* __restrict__ text, RepBits bits, const T* __restrict__ P,
                                                  RepFilter flt, uint32_t tile, uint64_t ntiles, uint64_t* __restrict__ t_cnt,
                                                  uint64_t* __restrict__ t_best, uint64_t* __restrict__ o_rank, uint64_t* __restrict__ o_count,
                                                  uint64_t* __restrict__ o_len, uint64_t* __restrict__ o_seqs, uint64_t* __restrict__ best, uint64_t nbest)
{
    static_assert(MODE != REP_PROFILE || SEQS, "the profile is one of sequence counts");
    constexpr int NCOL = SEQS ? 5 : 4;
    using Best = RepBestOp<NCOL>;
    __shared__ uint32_t s_w[4];
    __shared__ typename Best::V s_b[4];
    __shared__ T s_l[REP_STAGE], s_l1[REP_STAGE / 64];
    RepStaged<T> acc{gacc, s_l, s_l1, 0, 0, 0, 0};
    const uint64_t s = gacc.s;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        uint64_t running = MODE == REP_WRITE ? t_cnt[t] : 0;
        RepBest b{0, 0, 0, 0, 0};
        for (uint32_t it = 0; it < tile; it += 256) {
            const uint64_t r = t * tile + it + threadIdx.x;
            if (r - threadIdx.x >= s) break;             // (uniform: past the end of the array)
            if (it % REP_STAGE == 0) {                   // (uniform) the next window of the tile
                __syncthreads();                         // (the lanes are done with the window before)
                acc.stage(rep_tile_window(t, tile, it, REP_STAGE, s));
                __syncthreads();
            }
            bool keep = false;
            uint64_t a = 0, z = 0, v = 0, q = 0;
            if (r >= 1 && r < s)
                rep_interval(acc, s, r, flt.min_len, [&](uint64_t ia, uint64_t iz, uint64_t iv) {
                    a = ia; z = iz; v = iv;
                    keep = rep_keep(acc, text, bits.dw, bits.dp, bits.sw, bits.sp, flt.kind, flt.min_count, flt.max_count, a, z, v);
                    if (SEQS && keep) { q = shr_seqs(P, a, z); keep = shr_keep(q, flt.min_seqs, flt.max_seqs); }
                });
            if (MODE == REP_PROFILE) {
                if (keep && q - 1 < nbest && __hip_atomic_load(&best[q - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v)
                    atomicMax((unsigned long long*)&best[q - 1], (unsigned long long)v);
                continue;
            }
            const WgScan<uint32_t> sc = wg_scan_op<SumOp<uint32_t>, 4>(keep ? 1u : 0u, s_w);
            if (keep) {
                if (MODE == REP_WRITE) {
                    const uint64_t o = running + sc.before;
                    o_rank[o] = a; o_count[o] = z - a; o_len[o] = v;
                    if (SEQS) o_seqs[o] = q;
                } else b.take(v, r, a, z - a, q);
            }
            running += sc.total;
        }
        if (MODE == REP_COUNT) {
            const typename Best::V best = wg_reduce_op<Best, 4>(Best::make(b), s_b);
            if (threadIdx.x == 0) {
                t_cnt[t] = running;
                for (int c = 0; c < NCOL; c++) t_best[NCOL * t + c] = best.c[c];
            }
        }
    }
}

// stats[0] = *total (the sum of the tile counts), then Op::stats of the combination of the tiles' candidates (Op::COLS
// words per tile): comparisons and sums, no atomics, so nothing depends on an order
template <typename Op>
__global__ __launch_bounds__(1024) void k_tile_best(const uint64_t* __restrict__ t_best, uint64_t ntiles, const uint64_t* __restrict__ total,
                                                    uint64_t* __restrict__ stats)
{
    __shared__ typename Op::V s_v[16];
    const typename Op::V v = tile_reduce<Op>(ntiles, [&](uint64_t t) { return Op::get(t_best + Op::COLS * t); }, s_v);
    if (threadIdx.x == 0) { stats[0] = *total; Op::stats(stats + 1, v); }
}

}  // namespace sufr

namespace {

// what the calls that search the clipped LCP share (repeats; sufr_shared.inc): the tiling, the accessor over l and its
// pyramid, the flag words with their prefixes, and the tile sums of the search pass
template <typename T>
struct RepPrep {
    uint32_t tile, nw, levels, grid;
    uint64_t ntiles, nwords, wgs;
    sufr::RepAcc<T> acc;
    sufr::RepBits bits;
    uint64_t *t_cnt, *t_best, *d_stats;                  // ntiles + 1 kept counts (then bases), 5 columns per tile, 5 stats
};

// the fold, the scans of the popcount totals and the coarser levels, enqueued on the context's stream
template <typename T>
int repeats_prepare(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_lcp, const sufr::KmerSeqs& q, RepPrep<T>& P)
{
    sufr::Pipeline& pl = ctx->pl;
    const uint64_t s = ix->ix.s;
    const uint32_t tile = ctx->repeat_tile ? ctx->repeat_tile : sufr::REP_TILE_MAX, nw = tile / 64;
    const uint64_t ntiles = (s + tile - 1) / tile, nwords = ntiles * nw;
    const uint32_t levels = sufr::rep_levels(s);
    const bool clipped = q.num > 1;
    int rc;
    // rbits: the "differs" words, the "start" words and their prefixes; rsum: per tile the two popcount totals (each with
    // its grand total behind it), the kept counts (and their total), the five columns of a candidate (repeats uses four of
    // them); then the five stats
    if ((rc = pl.ensure(ctx->rbits, nwords * 32)) || (rc = pl.ensure(ctx->rsum, (ntiles * 8 + 3 + 5) * 8)) ||
        (rc = pl.ensure(ctx->rpyr, (sufr::rep_level_offset(s, levels + 1) + 1) * sizeof(T))) ||
        (clipped && (rc = pl.ensure(ctx->rell, s * sizeof(T))))) return rc;
    uint64_t* dw = (uint64_t*)ctx->rbits.p;
    uint64_t *sw = dw + nwords, *dp = sw + nwords, *sp = dp + nwords;
    uint64_t* t_d = (uint64_t*)ctx->rsum.p;
    uint64_t *t_s = t_d + ntiles + 1, *t_cnt = t_s + ntiles + 1, *t_best = t_cnt + ntiles + 1, *d_stats = t_best + 5 * ntiles;
    T* up = (T*)ctx->rpyr.p;
    T* ell = clipped ? (T*)ctx->rell.p : nullptr;
    const T* sa = index_sa<T>(ix);
    const uint64_t wgs = batch_grid(pl);
    const uint32_t grid = (uint32_t)(ntiles < wgs ? ntiles : wgs);
    hipLaunchKernelGGL(sufr::k_rep_fold<T>, dim3(grid), dim3(256), 0, pl.stream, sa, (const T*)d_lcp, ix->ix.text, s, q, tile, ntiles, ell,
                       levels ? up : (T*)nullptr, dw, sw, dp, sp, t_d, t_s);
    hipLaunchKernelGGL(sufr::k_locate_scan, dim3(1), dim3(1024), 0, pl.stream, t_d, ntiles, t_d + ntiles);
    hipLaunchKernelGGL(sufr::k_locate_scan, dim3(1), dim3(1024), 0, pl.stream, t_s, ntiles, t_s + ntiles);
    {
        const uint64_t need = (nwords + 255) / 256;
        hipLaunchKernelGGL(sufr::k_rep_addbase, dim3((uint32_t)(need < wgs ? need : wgs)), dim3(256), 0, pl.stream, dp, sp, nwords, nw,
                           (const uint64_t*)t_d, (const uint64_t*)t_s);
    }
    for (uint32_t k = 2; k <= levels; k++) {
        const uint64_t n_in = sufr::rep_level_size(s, k - 1), n_out = sufr::rep_level_size(s, k), need = (n_out + 3) / 4;
        hipLaunchKernelGGL(sufr::k_rep_level<T>, dim3((uint32_t)(need < wgs ? need : wgs)), dim3(256), 0, pl.stream,
                           (const T*)(up + sufr::rep_level_offset(s, k - 1)), n_in, up + sufr::rep_level_offset(s, k), n_out);
    }
    P = RepPrep<T>{tile, nw, levels, grid, ntiles, nwords, wgs, sufr::RepAcc<T>{clipped ? (const T*)ell : (const T*)d_lcp, (const T*)up, sa, s},
                   sufr::RepBits{dw, dp, sw, sp}, t_cnt, t_best, d_stats};
    return 0;
}

// The counted find of repeats (SEQS false) and shared (SEQS true, P the prefix of sufr_shared.inc): the counting launch, the
// tile counts to bases, the stats, the report (one synchronisation), the writing launch.  h: the NCOL stats as read, zeros
// when they were not.
template <typename T, bool SEQS>
int repeats_find(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const RepPrep<T>& R, const T* P, const sufr::RepFilter& flt, const char* tag,
                 uint64_t cap, void* d_rank, void* d_count, void* d_length, void* d_seqs, uint64_t* total_out, unsigned long long* h)
{
    constexpr int NCOL = SEQS ? 5 : 4;
    sufr::Pipeline& pl = ctx->pl;
    uint64_t* const none = nullptr;
    hipLaunchKernelGGL((sufr::k_rep_find<T, sufr::REP_COUNT, SEQS>), dim3(R.grid), dim3(256), 0, pl.stream, R.acc, ix->ix.text, R.bits, P, flt, R.tile,
                       R.ntiles, R.t_cnt, R.t_best, none, none, none, none, none, (uint64_t)0);
    hipLaunchKernelGGL(sufr::k_locate_scan, dim3(1), dim3(1024), 0, pl.stream, R.t_cnt, R.ntiles, R.t_cnt + R.ntiles);
    hipLaunchKernelGGL(sufr::k_tile_best<sufr::RepBestOp<NCOL>>, dim3(1), dim3(1024), 0, pl.stream, (const uint64_t*)R.t_best, R.ntiles,
                       (const uint64_t*)(R.t_cnt + R.ntiles), R.d_stats);
    const int rc = report_total(pl, tag, "records", R.d_stats, NCOL, h, cap, total_out, d_rank && d_count && d_length && (!SEQS || d_seqs));
    if (rc || !h[0]) return rc;
    hipLaunchKernelGGL((sufr::k_rep_find<T, sufr::REP_WRITE, SEQS>), dim3(R.grid), dim3(256), 0, pl.stream, R.acc, ix->ix.text, R.bits, P, flt, R.tile,
                       R.ntiles, R.t_cnt, R.t_best, (uint64_t*)d_rank, (uint64_t*)d_count, (uint64_t*)d_length, (uint64_t*)d_seqs, none, (uint64_t)0);
    return launch_status(pl, tag);
}

template <typename T>
int repeats_run(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_lcp, const sufr::KmerSeqs& q, const sufr::RepFilter& flt,
                uint64_t cap, void* d_rank, void* d_count, void* d_length, uint64_t* total_out, sufr_repeat_stats* stats_out)
{
    RepPrep<T> R;
    if (const int rc = repeats_prepare<T>(ctx, ix, d_lcp, q, R)) return rc;
    unsigned long long h[4];
    const int rc = repeats_find<T, false>(ctx, ix, R, (const T*)nullptr, flt, "repeats", cap, d_rank, d_count, d_length, nullptr, total_out, h);
    if (stats_out) *stats_out = sufr_repeat_stats{h[0], h[1], h[2], h[3]};
    return rc;
}

}  // namespace

extern "C" {

int sufr_hip_set_repeat_tile(sufr_hip_ctx* ctx, uint64_t ranks)
{
    if (!ctx) return SUFR_HIP_E_INVALID;
    if (ranks > sufr::REP_TILE_MAX) ranks = sufr::REP_TILE_MAX;
    ctx->repeat_tile = (uint32_t)((ranks + 255) / 256 * 256);        // (0 stays 0: the default)
    return 0;
}

int sufr_hip_repeats_device(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_lcp, const uint64_t* seq_starts,
                            uint64_t num_sequences, uint32_t kind, uint64_t min_len, uint64_t min_count, uint64_t max_count, uint64_t cap,
                            void* d_rank, void* d_count, void* d_length, uint64_t* total_out, sufr_repeat_stats* stats_out)
{
    if (stats_out) *stats_out = sufr_repeat_stats{0, 0, 0, 0};
    if (total_out) *total_out = 0;
    if (!ctx || !ix) return SUFR_HIP_E_INVALID;
    sufr::Pipeline& pl = ctx->pl;
    int rc;
    if ((rc = lcp_refusals(ctx, ix, "repeats", "repeats"))) return rc;
    if (min_len == 0) { pl.set_error("repeats: min_len must be at least 1"); return SUFR_HIP_E_INVALID; }
    if (kind > SUFR_REPEAT_SUPERMAXIMAL) { pl.set_error("repeats: unknown kind " + std::to_string(kind)); return SUFR_HIP_E_INVALID; }
    if (!ix->ix.s) return 0;
    sufr::KmerSeqs q;
    if ((rc = kmer_prepare(ctx, ix, d_lcp, seq_starts, num_sequences, "repeats", q))) return rc;
    const sufr::RepFilter flt{kind, min_len, min_count < 2 ? 2 : min_count, max_count, 0, 0};
    return by_width(ix, [&](auto w) { return repeats_run<decltype(w)>(ctx, ix, d_lcp, q, flt, cap, d_rank, d_count, d_length, total_out, stats_out); });
}

}  // extern "C"
