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
// k_rep_find     a lane per rank with l[r] >= min_len: the left search with <= (the rank is the representative iff the
//                value found is smaller, and that index is a), then the right search for b, the count filter and the kind.
//                The l of up to 4096 ranks of the tile, and their level-1 entries, are staged in LDS and searched there
//                first (RepStaged); a search that leaves the window reads the pyramid in memory and descends again.
//                Counting run: kept ranks per tile and the tile's longest / largest count.  Writing run: the same decisions,
//                compacted in rank order behind the tile's base.  The cost of a rank is bounded by 2 x 64 x levels reads per
//                search whatever b - a is; only the supermaximal walk (rep_supermaximal) is longer, and says when.
// k_rep_best     one workgroup: the stats from the tiles' candidates -- comparisons of (length, representative), no atomics,
//                so nothing depends on an order.
// A workgroup takes tiles t = blockIdx.x, blockIdx.x + gridDim.x, ...; no scratch; k_rep_find holds 16.4 KB of LDS (32-bit
// arrays) or 32.7 KB (64-bit), the others under 33 KB.

#include "sufr_repeat_scan.h"

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

// RepAcc behind a window of l and of level 1 in LDS: ranks [w0, w1) and their words (w0 a multiple of 64).  A search reads
// the window first -- a scan step is then an LDS read, not a dependent global load -- and what lies outside it from memory.
template <typename T, typename G = RepAcc<T>>         // (G: what lies behind the window; sufr_lz.inc stages its own arrays)
struct RepStaged {
    G g;
    const T *s_l, *s_l1;
    uint64_t w0, len, v0, vlen;                         // the window of level 0 and of level 1: first index and entries
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

// exclusive prefix of x over the 256 lanes of a workgroup and its total; s_w: 4 words of LDS, free again on return
__device__ __forceinline__ uint32_t rep_wg_exscan(uint32_t x, uint32_t* s_w, uint32_t& total)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t inc = x;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(inc, o); if (lane >= (uint32_t)o) inc += u; }
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
    for (uint32_t k = 0; k < 4; k++) { const uint32_t t = s_w[k]; if (k < w) base += t; total += t; }
    __syncthreads();
    return base + inc - x;
}

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
        uint32_t td, ts;
        const uint32_t cd = threadIdx.x < nw ? s_pd[threadIdx.x] : 0, cs = threadIdx.x < nw ? s_ps[threadIdx.x] : 0;
        const uint32_t ed = rep_wg_exscan(cd, s_w, td), es = rep_wg_exscan(cs, s_w, ts);
        if (threadIdx.x < nw) { dp[t * nw + threadIdx.x] = ed; sp[t * nw + threadIdx.x] = es; }
        if (threadIdx.x == 0) { t_d[t] = td; t_s[t] = ts; }
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

struct RepFilter { uint32_t kind; uint64_t min_len, min_count, max_count; };

// WRITE false: t_cnt[t] = kept ranks of tile t, t_best[4 t ..] = {longest, its representative, its rank, largest count}.
// WRITE true: t_cnt[t] is the tile's base; the records go to o_rank / o_count / o_len in rank order.
template <typename T, bool WRITE>
__global__ __launch_bounds__(256) void k_rep_find(RepAcc<T> gacc, const uint8_t* __restrict__ text, RepBits bits, RepFilter flt, uint32_t tile,
                                                  uint64_t ntiles, uint64_t* __restrict__ t_cnt, uint64_t* __restrict__ t_best,
                                                  uint64_t* __restrict__ o_rank, uint64_t* __restrict__ o_count, uint64_t* __restrict__ o_len)
{
    __shared__ uint32_t s_w[4];
    __shared__ uint64_t s_b[4][4];
    __shared__ T s_l[REP_STAGE], s_l1[REP_STAGE / 64];
    RepStaged<T> acc{gacc, s_l, s_l1, 0, 0, 0, 0};
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t s = gacc.s;
    const bool has_l1 = s > 64;                          // (level 1 exists)
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        uint64_t running = WRITE ? t_cnt[t] : 0;
        uint64_t b_len = 0, b_rep = 0, b_rank = 0, b_cnt = 0;
        for (uint32_t it = 0; it < tile; it += 256) {
            const uint64_t r = t * tile + it + threadIdx.x;
            if (r - threadIdx.x >= s) break;             // (uniform: past the end of the array)
            if (it % REP_STAGE == 0) {                   // (uniform) the next window of the tile: REP_STAGE ranks, or what is left
                const uint64_t w0 = t * tile + it, left = tile - it < REP_STAGE ? tile - it : REP_STAGE,
                               len = w0 + left < s ? left : s - w0, vlen = has_l1 ? (len + 63) / 64 : 0;
                __syncthreads();                         // (the lanes are done with the window before)
                for (uint64_t i = threadIdx.x; i < len; i += 256) s_l[i] = (T)gacc.at(0, 0, w0 + i);
                if (threadIdx.x < vlen) s_l1[threadIdx.x] = (T)gacc.at(1, 0, (w0 >> 6) + threadIdx.x);
                acc.w0 = w0; acc.len = len; acc.v0 = w0 >> 6; acc.vlen = vlen;
                __syncthreads();
            }
            bool keep = false;
            uint64_t a = 0, z = 0, v = 0;
            if (r >= 1 && r < s) {
                v = acc.at(0, 0, r);
                if (v >= flt.min_len) {
                    a = rep_search_left(acc, s, r, v);
                    if (a != REP_NONE && acc.at(0, 0, a) < v) {
                        z = rep_search_right(acc, s, r, v);
                        keep = rep_keep(acc, text, bits.dw, bits.dp, bits.sw, bits.sp, flt.kind, flt.min_count, flt.max_count, a, z, v);
                    }
                }
            }
            uint32_t tot;
            const uint32_t at = rep_wg_exscan(keep ? 1u : 0u, s_w, tot);
            if (keep) {
                if (WRITE) { const uint64_t o = running + at; o_rank[o] = a; o_count[o] = z - a; o_len[o] = v; }
                else {
                    if (v > b_len) { b_len = v; b_rep = r; b_rank = a; }      // (a lane's ranks ascend: ties keep the first)
                    if (z - a > b_cnt) b_cnt = z - a;
                }
            }
            running += tot;
        }
        if (!WRITE) {
            for (int o = 32; o > 0; o >>= 1) {
                const uint64_t l2 = __shfl_down(b_len, o), r2 = __shfl_down(b_rep, o), a2 = __shfl_down(b_rank, o), c2 = __shfl_down(b_cnt, o);
                if (rep_better(l2, r2, b_len, b_rep)) { b_len = l2; b_rep = r2; b_rank = a2; }
                if (c2 > b_cnt) b_cnt = c2;
            }
            if (lane == 0) { s_b[w][0] = b_len; s_b[w][1] = b_rep; s_b[w][2] = b_rank; s_b[w][3] = b_cnt; }
            __syncthreads();
            if (threadIdx.x == 0) {
                for (uint32_t k = 1; k < 4; k++) {
                    if (rep_better(s_b[k][0], s_b[k][1], b_len, b_rep)) { b_len = s_b[k][0]; b_rep = s_b[k][1]; b_rank = s_b[k][2]; }
                    if (s_b[k][3] > b_cnt) b_cnt = s_b[k][3];
                }
                t_cnt[t] = running;
                t_best[4 * t] = b_len; t_best[4 * t + 1] = b_rep; t_best[4 * t + 2] = b_rank; t_best[4 * t + 3] = b_cnt;
            }
            __syncthreads();                             // (s_b is reused by the next tile)
        }
    }
}

// stats = {records, longest, longest_rank, max_count}; *total: the sum of the tile counts
__global__ __launch_bounds__(1024) void k_rep_best(const uint64_t* __restrict__ t_best, uint64_t ntiles, const uint64_t* __restrict__ total,
                                                   uint64_t* __restrict__ stats)
{
    __shared__ uint64_t s_l[1024], s_r[1024], s_a[1024], s_c[1024];
    const uint32_t i = threadIdx.x;
    uint64_t b_len = 0, b_rep = 0, b_rank = 0, b_cnt = 0;
    for (uint64_t t = i; t < ntiles; t += 1024) {
        if (rep_better(t_best[4 * t], t_best[4 * t + 1], b_len, b_rep)) { b_len = t_best[4 * t]; b_rep = t_best[4 * t + 1]; b_rank = t_best[4 * t + 2]; }
        if (t_best[4 * t + 3] > b_cnt) b_cnt = t_best[4 * t + 3];
    }
    s_l[i] = b_len; s_r[i] = b_rep; s_a[i] = b_rank; s_c[i] = b_cnt;
    __syncthreads();
    for (uint32_t o = 512; o > 0; o >>= 1) {
        if (i < o) {
            if (rep_better(s_l[i + o], s_r[i + o], s_l[i], s_r[i])) { s_l[i] = s_l[i + o]; s_r[i] = s_r[i + o]; s_a[i] = s_a[i + o]; }
            if (s_c[i + o] > s_c[i]) s_c[i] = s_c[i + o];
        }
        __syncthreads();
    }
    if (i == 0) { stats[0] = *total; stats[1] = s_l[0]; stats[2] = s_a[0]; stats[3] = s_c[0]; }
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
    uint64_t *t_cnt, *t_best, *d_stats;                  // ntiles + 1 kept counts (then bases), 4 candidates per tile, 4 stats
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
    // its grand total behind it), the kept counts (and their total), the four candidates; then the four stats
    if ((rc = pl.ensure(ctx->rbits, nwords * 32)) || (rc = pl.ensure(ctx->rsum, (ntiles * 7 + 3 + 4) * 8)) ||
        (rc = pl.ensure(ctx->rpyr, (sufr::rep_level_offset(s, levels + 1) + 1) * sizeof(T))) ||
        (clipped && (rc = pl.ensure(ctx->rell, s * sizeof(T))))) return rc;
    uint64_t* dw = (uint64_t*)ctx->rbits.p;
    uint64_t *sw = dw + nwords, *dp = sw + nwords, *sp = dp + nwords;
    uint64_t* t_d = (uint64_t*)ctx->rsum.p;
    uint64_t *t_s = t_d + ntiles + 1, *t_cnt = t_s + ntiles + 1, *t_best = t_cnt + ntiles + 1, *d_stats = t_best + 4 * ntiles;
    T* up = (T*)ctx->rpyr.p;
    T* ell = clipped ? (T*)ctx->rell.p : nullptr;
    const T* sa = (const T*)(ix->ix.sa64 ? (const void*)ix->ix.sa64 : (const void*)ix->ix.sa);
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

template <typename T>
int repeats_run(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_lcp, const sufr::KmerSeqs& q, const sufr::RepFilter& flt,
                uint64_t cap, void* d_rank, void* d_count, void* d_length, uint64_t* total_out, sufr_repeat_stats* stats_out)
{
    sufr::Pipeline& pl = ctx->pl;
    RepPrep<T> P;
    int rc;
    if ((rc = repeats_prepare<T>(ctx, ix, d_lcp, q, P))) return rc;
    const uint32_t tile = P.tile, grid = P.grid;
    const uint64_t ntiles = P.ntiles;
    const sufr::RepAcc<T> acc = P.acc;
    const sufr::RepBits bits = P.bits;
    uint64_t *t_cnt = P.t_cnt, *t_best = P.t_best, *d_stats = P.d_stats;
    hipLaunchKernelGGL((sufr::k_rep_find<T, false>), dim3(grid), dim3(256), 0, pl.stream, acc, ix->ix.text, bits, flt, tile, ntiles, t_cnt, t_best,
                       (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr);
    hipLaunchKernelGGL(sufr::k_locate_scan, dim3(1), dim3(1024), 0, pl.stream, t_cnt, ntiles, t_cnt + ntiles);
    hipLaunchKernelGGL(sufr::k_rep_best, dim3(1), dim3(1024), 0, pl.stream, (const uint64_t*)t_best, ntiles, (const uint64_t*)(t_cnt + ntiles), d_stats);
    if ((rc = launch_status(pl, "repeats"))) return rc;
    unsigned long long h[4];
    if ((rc = read_totals(pl, d_stats, 4, h, "repeats", "reading the total failed"))) return rc;
    if (total_out) *total_out = h[0];
    if (stats_out) *stats_out = sufr_repeat_stats{h[0], h[1], h[2], h[3]};
    if (h[0] > cap) {
        pl.set_error("repeats: " + std::to_string(h[0]) + " records, room for " + std::to_string(cap));
        return SUFR_HIP_E_CAPACITY;
    }
    if (!h[0]) return 0;
    if (!d_rank || !d_count || !d_length) { pl.set_error("repeats: no output arrays"); return SUFR_HIP_E_INVALID; }
    hipLaunchKernelGGL((sufr::k_rep_find<T, true>), dim3(grid), dim3(256), 0, pl.stream, acc, ix->ix.text, bits, flt, tile, ntiles, t_cnt, t_best,
                       (uint64_t*)d_rank, (uint64_t*)d_count, (uint64_t*)d_length);
    return launch_status(pl, "repeats");
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
    pl.err.clear();
    int rc;
    if ((rc = query_check(ctx, ix, "repeats"))) return rc;
    if (ix->built_mql > 0) {
        pl.set_error("repeats: the index was built with max_query_len " + std::to_string(ix->built_mql) + ", its LCP is capped");
        return SUFR_HIP_E_UNSUPPORTED;
    }
    if (min_len == 0) { pl.set_error("repeats: min_len must be at least 1"); return SUFR_HIP_E_INVALID; }
    if (kind > SUFR_REPEAT_SUPERMAXIMAL) { pl.set_error("repeats: unknown kind " + std::to_string(kind)); return SUFR_HIP_E_INVALID; }
    if (!ix->ix.s) return 0;
    sufr::KmerSeqs q;
    if ((rc = kmer_prepare(ctx, ix, d_lcp, seq_starts, num_sequences, "repeats", q))) return rc;
    const sufr::RepFilter flt{kind, min_len, min_count < 2 ? 2 : min_count, max_count};
    return ix->sa_width == 8 ? repeats_run<uint64_t>(ctx, ix, d_lcp, q, flt, cap, d_rank, d_count, d_length, total_out, stats_out)
                             : repeats_run<uint32_t>(ctx, ix, d_lcp, q, flt, cap, d_rank, d_count, d_length, total_out, stats_out);
}

}  // extern "C"
