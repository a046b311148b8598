// sufr_lz.inc -- the longest previous factor of every text position and the LZ77 parse, from the SA and the LCP of a
// device-resident index (included by sufr_kernels.hip after sufr_repeat.inc; include/sufr_lz.h, DESIGN.md section 20).
//
// LPF[SA[r]] needs the nearest rank on either side of r whose suffix starts earlier in the text and the minimum of the LCP
// between them.  Both may be as far away as the array is long (all-A: SA descends, every left search runs to rank 0), so
// nothing is local to a tile: the searches of sufr_repeat_scan.h walk a min pyramid over the suffix array's values, and
// lz_range_min walks one over the raw LCP.  The arithmetic is sufr_lz_scan.h, which the host path and tests/lz_shim.cpp
// compile too; this file moves the data and turns n "next position" pointers into one ordered factor list.
//
// k_lz_fold      one pass over SA and LCP: level 1 of both pyramids, a wave per 64 ranks.
// k_rep_level    (sufr_repeat.inc) one launch per level >= 2 and pyramid.
// k_lz_lpf       a lane per rank: two searches, two range minima, the binary search of the sequence starts for d(p), then
//                the scatter of LPF and SRC to position SA[r] (the buffers are zeroed / NONE-filled first, so positions that
//                are not indexed read as defined).  The SA and the LCP of up to LZ_STAGE ranks of the tile and their level-1
//                entries are staged in LDS (RepStaged over LzAcc, the window by rep_tile_window; one loop fills both
//                arrays), so that a scan step is an LDS read.
// k_lz_table     the parse, table phase.  A workgroup per tile of B text positions: every position's entry (the last
//                in-tile position on its chain, the hops to it) by pointer doubling in LDS -- one 32-bit word per position,
//                updated in place: a word is always a true (position on the chain, hops to it) pair, a round composes two
//                of them, and a reader that meets a word already advanced in this round only gets further: ceil(log2 B)
//                rounds.  4 bytes per position go to scratch of the context.
// k_lz_chain     the parse, chain phase: one lane walks from tile to tile -- the entry of the next tile is last +
//                step[last], the factor base of an entered tile the running sum of hops + 1 -- two dependent loads per
//                entered tile.  Tiles that a long factor jumps over keep the "no entry" mark.  The one serial part.
// k_lz_emit      the parse, emit phase.  A workgroup per entered tile: the steps of the tile in LDS (16 bits each, held to
//                B), one lane walks the chain from the tile's entry and leaves the list of its positions in the same array
//                (entry k is written after entry k was read: k never runs ahead of the chain), then a lane per factor.
//                Counting run: the tile's literals and its longest factor.  Writing run: (start, length, source) behind the
//                tile's base, in text order.
// k_tile_best    (sufr_repeat.inc, over SumBestOp<1>) one workgroup: the stats from the tiles' candidates -- the sum of the
//                literals, the best (length, start); no atomics.  The tail of k_lz_emit is wg_reduce_op over the same
//                operator (sufr_scan.inc, DESIGN.md section 10.2).  The host tail of the counted call is report_total.
// No scratch; LDS: k_lz_lpf 16.5 KB (32-bit arrays) or 33 KB (64-bit), k_lz_table 64 KB, k_lz_emit 32 KB.

#include "sufr_lz_scan.h"

namespace sufr {

static constexpr uint32_t LZ_TILE_MAX = 16384;          // ranks of an LPF tile and positions of a parse tile at most
static constexpr uint32_t LZ_STAGE = 2048;              // ranks of SA and LCP a workgroup keeps in LDS at a time
static constexpr uint32_t LZ_NO_ENTRY = 0xFFFFFFFFu;    // t_entry of a tile the chain does not enter

// an array and the coarser levels of its min pyramid
template <typename T>
struct LzAcc {
    const T *l0, *up;
    __device__ __forceinline__ uint64_t at(uint32_t level, uint64_t off, uint64_t i) const { return level ? (uint64_t)up[off + i] : (uint64_t)l0[i]; }
};

// sa1[i] = min SA[64 i .. 64 i + 64), lcp1[i] = min LCP[64 i .. 64 i + 64): a wave per entry
template <typename T>
__global__ __launch_bounds__(256) void k_lz_fold(const T* __restrict__ sa, const T* __restrict__ lcp, uint64_t s, T* __restrict__ sa1,
                                                 T* __restrict__ lcp1, uint64_t n1)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * 4;
    for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n1; i += stride) {
        const uint64_t r = i * 64 + lane;
        uint64_t a = r < s ? (uint64_t)sa[r] : ~(uint64_t)0, b = r < s ? (uint64_t)lcp[r] : ~(uint64_t)0;
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t ua = __shfl_xor(a, o), ub = __shfl_xor(b, o);
            if (ua < a) a = ua;
            if (ub < b) b = ub;
        }
        if (lane == 0) { sa1[i] = (T)a; lcp1[i] = (T)b; }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_lz_lpf(LzAcc<T> gsa, LzAcc<T> glcp, uint64_t s, KmerSeqs q, uint32_t tile, uint64_t ntiles,
                                                T* __restrict__ lpf, T* __restrict__ src)
{
    __shared__ T s_sa[LZ_STAGE], s_lcp[LZ_STAGE], s_sa1[LZ_STAGE / 64], s_lcp1[LZ_STAGE / 64];
    RepStaged<T, LzAcc<T>> sa{gsa, s_sa, s_sa1, 0, 0, 0, 0}, lcp{glcp, s_lcp, s_lcp1, 0, 0, 0, 0};
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        for (uint32_t it = 0; it < tile; it += 256) {
            const uint64_t r = t * tile + it + threadIdx.x;
            if (r - threadIdx.x >= s) break;             // (uniform: past the end of the array)
            if (it % LZ_STAGE == 0) {                    // (uniform) the next window of the tile, of both arrays
                const RepWindow win = rep_tile_window(t, tile, it, LZ_STAGE, s);
                __syncthreads();                         // (the lanes are done with the window before)
                // (one loop fills both arrays: two calls of RepStaged::stage cost the 64-bit kernel four VGPRs)
                for (uint64_t i = threadIdx.x; i < win.len; i += 256) { s_sa[i] = gsa.l0[win.w0 + i]; s_lcp[i] = glcp.l0[win.w0 + i]; }
                if (threadIdx.x < win.vlen) { s_sa1[threadIdx.x] = gsa.up[(win.w0 >> 6) + threadIdx.x]; s_lcp1[threadIdx.x] = glcp.up[(win.w0 >> 6) + threadIdx.x]; }
                sa.w0 = lcp.w0 = win.w0; sa.len = lcp.len = win.len; sa.v0 = lcp.v0 = win.w0 >> 6; sa.vlen = lcp.vlen = win.vlen;
                __syncthreads();
            }
            if (r < s) {
                const uint64_t p = sa.at(0, 0, r);
                const LzEntry e = lz_rank(sa, lcp, s, r, p, rep_room(q.starts, q.num, q.n, p));
                if (lpf) lpf[p] = (T)e.lpf;
                if (src) src[p] = (T)e.src;              // (LZ_NONE is all ones of either width)
            }
        }
    }
}

// tab[p]: lz_tab_pack(the last position of p's tile on the chain from p, the hops to it)
template <typename T>
__global__ __launch_bounds__(256) void k_lz_table(const T* __restrict__ lpf, uint64_t n, uint32_t B, uint64_t ntiles, uint32_t* __restrict__ tab)
{
    __shared__ uint32_t s_e[LZ_TILE_MAX];
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t base = t * B;
        const uint32_t len = (uint32_t)(n - base < B ? n - base : B);
        for (uint32_t i = threadIdx.x; i < len; i += 256) {
            const uint64_t nx = i + lz_step((uint64_t)lpf[base + i]);
            s_e[i] = nx < len ? lz_tab_pack((uint32_t)nx, 1) : lz_tab_pack(i, 0);
        }
        __syncthreads();
        for (uint32_t reach = 1; reach < len; reach <<= 1) {        // (after k rounds an entry is 2^k hops on, or at its chain's end)
            for (uint32_t i = threadIdx.x; i < len; i += 256) {
                // (one 32-bit LDS access each: whichever of this round's versions of an entry a lane meets, it is a whole one)
                const uint32_t e = __hip_atomic_load(&s_e[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP), j = lz_tab_last(e);
                if (j == i) continue;
                const uint32_t e2 = __hip_atomic_load(&s_e[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP), j2 = lz_tab_last(e2);
                if (j2 == j) continue;
                __hip_atomic_store(&s_e[i], lz_tab_pack(j2, lz_tab_hops(e) + lz_tab_hops(e2)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            __syncthreads();
        }
        for (uint32_t i = threadIdx.x; i < len; i += 256) tab[base + i] = s_e[i];
        __syncthreads();                                 // (s_e is the next tile's)
    }
}

// t_entry[t] (LZ_NO_ENTRY before the launch): the tile-relative position at which the parse enters tile t; t_base[t]: the
// factors before it; *total: z
template <typename T>
__global__ __launch_bounds__(64) void k_lz_chain(const T* __restrict__ lpf, const uint32_t* __restrict__ tab, uint64_t n, uint32_t B,
                                                 uint32_t* __restrict__ t_entry, uint64_t* __restrict__ t_base, uint64_t* __restrict__ total)
{
    if (threadIdx.x || blockIdx.x) return;
    uint64_t pos = 0, count = 0;
    while (pos < n) {
        const uint64_t t = pos / B;
        const uint32_t e = tab[pos];
        t_entry[t] = (uint32_t)(pos - t * B);
        t_base[t] = count;
        count += (uint64_t)lz_tab_hops(e) + 1;
        const uint64_t last = t * B + lz_tab_last(e);
        pos = last + lz_step((uint64_t)lpf[last]);
    }
    *total = count;
}

// WRITE false: t_stat[3 t ..] = {literals, longest, longest_start} of the factors that start in tile t (zeros for a tile
// without an entry).  WRITE true: the records of tile t go behind t_base[t].
template <typename T, bool WRITE>
__global__ __launch_bounds__(256) void k_lz_emit(const T* __restrict__ lpf, const T* __restrict__ src, uint64_t n, uint32_t B, uint64_t ntiles,
                                                 const uint32_t* __restrict__ t_entry, const uint64_t* __restrict__ t_base,
                                                 uint64_t* __restrict__ t_stat, uint64_t* __restrict__ o_start, uint64_t* __restrict__ o_len,
                                                 uint64_t* __restrict__ o_src)
{
    __shared__ uint16_t s_st[LZ_TILE_MAX];
    __shared__ uint32_t s_cnt;
    using Stat = SumBestOp<1>;
    __shared__ Stat::V s_b[4];
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint32_t e0 = t_entry[t];                  // (uniform)
        if (e0 == LZ_NO_ENTRY) {
            if (!WRITE && threadIdx.x < 3) t_stat[3 * t + threadIdx.x] = 0;
            continue;
        }
        const uint64_t base = t * B;
        const uint32_t len = (uint32_t)(n - base < B ? n - base : B);
        for (uint32_t i = threadIdx.x; i < len; i += 256) {
            const uint64_t st = lz_step((uint64_t)lpf[base + i]);
            s_st[i] = (uint16_t)(st < B ? st : B);       // (B and more leave the tile alike)
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t c = e0, k = 0;
            while (c < len) {                            // (k <= c: entry k is free once the step at c is read)
                const uint32_t st = s_st[c];
                s_st[k++] = (uint16_t)c;
                c += st;
            }
            s_cnt = k;
        }
        __syncthreads();
        const uint32_t cnt = s_cnt;
        const uint64_t out = t_base[t];
        Stat::V b = Stat::identity();                    // {literals, longest, longest_start}
        for (uint32_t k = threadIdx.x; k < cnt; k += 256) {
            const uint64_t p = base + s_st[k], l = (uint64_t)lpf[p];
            if (WRITE) { o_start[out + k] = p; o_len[out + k] = lz_step(l); o_src[out + k] = l ? (uint64_t)src[p] : LZ_NONE; }
            else {
                if (!l) b.sum[0]++;
                if (lz_step(l) > b.len) { b.len = lz_step(l); b.at = p; }      // (a lane's positions ascend: ties keep the first)
            }
        }
        if (!WRITE) {
            b = wg_reduce_op<Stat, 4>(b, s_b);
            if (threadIdx.x == 0) Stat::stats(t_stat + 3 * t, b);
        }
        __syncthreads();                                 // (s_st and s_cnt are the next tile's)
    }
}

}  // namespace sufr

namespace {

// LPF and SRC of every position into lpf / src (n entries of T each; either may be null): the fills, the pyramids, k_lz_lpf
template <typename T>
int lz_lpf_run(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_lcp, const sufr::KmerSeqs& q, T* lpf, T* src, const char* what)
{
    sufr::Pipeline& pl = ctx->pl;
    const uint64_t s = ix->ix.s, n = ix->ix.n;
    if ((lpf && n && hipMemsetAsync(lpf, 0, n * sizeof(T), pl.stream) != hipSuccess) ||
        (src && n && hipMemsetAsync(src, 0xFF, n * sizeof(T), pl.stream) != hipSuccess)) { pl.set_error(std::string(what) + ": memset failed"); return SUFR_HIP_E_HIP; }
    if (!s || !n || (!lpf && !src)) return 0;
    const uint32_t tile = ctx->lz_rank_tile ? ctx->lz_rank_tile : sufr::LZ_TILE_MAX, levels = sufr::rep_levels(s);
    const uint64_t ntiles = (s + tile - 1) / tile, plen = sufr::rep_level_offset(s, levels + 1) + 1;
    // lzpyr: the coarser levels of the pyramid over SA, then those of the pyramid over the LCP
    if (const int rc = pl.ensure(ctx->lzpyr, 2 * plen * sizeof(T))) return rc;
    T* up_sa = (T*)ctx->lzpyr.p;
    T* up_lcp = up_sa + plen;
    const T* sa = index_sa<T>(ix);
    const uint64_t wgs = batch_grid(pl);
    if (levels) {
        const uint64_t n1 = sufr::rep_level_size(s, 1), need = (n1 + 3) / 4;
        hipLaunchKernelGGL(sufr::k_lz_fold<T>, dim3((uint32_t)(need < wgs ? need : wgs)), dim3(256), 0, pl.stream, sa, (const T*)d_lcp, s, up_sa, up_lcp, n1);
    }
    for (uint32_t k = 2; k <= levels; k++) {
        const uint64_t n_in = sufr::rep_level_size(s, k - 1), n_out = sufr::rep_level_size(s, k), need = (n_out + 3) / 4;
        const uint64_t o_in = sufr::rep_level_offset(s, k - 1), o_out = sufr::rep_level_offset(s, k);
        for (T* up : {up_sa, up_lcp})
            hipLaunchKernelGGL(sufr::k_rep_level<T>, dim3((uint32_t)(need < wgs ? need : wgs)), dim3(256), 0, pl.stream, (const T*)(up + o_in), n_in,
                               up + o_out, n_out);
    }
    const sufr::LzAcc<T> asa{sa, (const T*)up_sa}, alcp{(const T*)d_lcp, (const T*)up_lcp};
    hipLaunchKernelGGL(sufr::k_lz_lpf<T>, dim3((uint32_t)(ntiles < wgs ? ntiles : wgs)), dim3(256), 0, pl.stream, asa, alcp, s, q, tile, ntiles, lpf, src);
    return launch_status(pl, what);
}

template <typename T>
int lz_run(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_lcp, const sufr::KmerSeqs& q, uint64_t cap, void* d_start, void* d_length,
           void* d_source, uint64_t* total_out, sufr_lz_stats* stats_out)
{
    sufr::Pipeline& pl = ctx->pl;
    const uint64_t n = ix->ix.n;
    const uint32_t B = ctx->lz_pos_tile ? ctx->lz_pos_tile : sufr::LZ_TILE_MAX;
    const uint64_t ntiles = (n + B - 1) / B;
    int rc;
    // lzarr: LPF, then SRC (2 n w); lztab: the parse tables (4 n); lzsum: per tile the base (8), the three candidates (24)
    // and the entry (4), then the total and the four stats
    if ((rc = pl.ensure(ctx->lzarr, 2 * n * sizeof(T))) || (rc = pl.ensure(ctx->lztab, n * 4)) ||
        (rc = pl.ensure(ctx->lzsum, ntiles * 36 + 5 * 8 + 8))) return rc;
    T* lpf = (T*)ctx->lzarr.p;
    T* src = lpf + n;
    uint32_t* tab = (uint32_t*)ctx->lztab.p;
    uint64_t* t_base = (uint64_t*)ctx->lzsum.p;
    uint64_t *t_stat = t_base + ntiles, *d_total = t_stat + 3 * ntiles, *d_stats = d_total + 1;
    uint32_t* t_entry = (uint32_t*)(d_stats + 4);
    if ((rc = lz_lpf_run<T>(ctx, ix, d_lcp, q, lpf, src, "lz"))) return rc;
    if (hipMemsetAsync(t_entry, 0xFF, ntiles * 4, pl.stream) != hipSuccess) { pl.set_error("lz: memset failed"); return SUFR_HIP_E_HIP; }
    const uint64_t wgs = batch_grid(pl);
    const uint32_t grid = (uint32_t)(ntiles < wgs ? ntiles : wgs);
    hipLaunchKernelGGL(sufr::k_lz_table<T>, dim3(grid), dim3(256), 0, pl.stream, (const T*)lpf, n, B, ntiles, tab);
#ifdef SUFR_HIP_PROBES
    hipEvent_t ev[2] = {nullptr, nullptr};                // (probes build: the chain kernel's own time, to standard error)
    const bool stamp = hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess && hipEventRecord(ev[0], pl.stream) == hipSuccess;
#endif
    hipLaunchKernelGGL(sufr::k_lz_chain<T>, dim3(1), dim3(64), 0, pl.stream, (const T*)lpf, (const uint32_t*)tab, n, B, t_entry, t_base, d_total);
#ifdef SUFR_HIP_PROBES
    if (stamp) (void)hipEventRecord(ev[1], pl.stream);
#endif
    hipLaunchKernelGGL((sufr::k_lz_emit<T, false>), dim3(grid), dim3(256), 0, pl.stream, (const T*)lpf, (const T*)src, n, B, ntiles,
                       (const uint32_t*)t_entry, (const uint64_t*)t_base, t_stat, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr);
    hipLaunchKernelGGL(sufr::k_tile_best<sufr::SumBestOp<1>>, dim3(1), dim3(1024), 0, pl.stream, (const uint64_t*)t_stat, ntiles, (const uint64_t*)d_total, d_stats);
    unsigned long long h[4];
    rc = report_total(pl, "lz", "factors", d_stats, 4, h, cap, total_out, d_start && d_length && d_source);
#ifdef SUFR_HIP_PROBES
    float ms = 0;
    if (stamp && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) fprintf(stderr, "lz: chain kernel %.3f ms (%llu tiles of %u positions)\n", ms, (unsigned long long)ntiles, B);
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
#endif
    if (stats_out) *stats_out = sufr_lz_stats{h[0], h[1], h[2], h[3]};
    if (rc || !h[0]) return rc;
    hipLaunchKernelGGL((sufr::k_lz_emit<T, true>), dim3(grid), dim3(256), 0, pl.stream, (const T*)lpf, (const T*)src, n, B, ntiles,
                       (const uint32_t*)t_entry, (const uint64_t*)t_base, t_stat, (uint64_t*)d_start, (uint64_t*)d_length, (uint64_t*)d_source);
    return launch_status(pl, "lz");
}

// the refusals both calls share, then the sequence starts of the call on the device (q)
int lz_prepare(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_lcp, const uint64_t* seq_starts, uint64_t num_sequences, const char* what,
               sufr::KmerSeqs& q)
{
    if (const int rc = lcp_refusals(ctx, ix, "longest previous factors", what)) return rc;
    return kmer_prepare(ctx, ix, d_lcp, seq_starts, num_sequences, what, q);
}

}  // namespace

extern "C" {

int sufr_hip_set_lz_tile(sufr_hip_ctx* ctx, uint64_t ranks, uint64_t positions)
{
    if (!ctx) return SUFR_HIP_E_INVALID;
    if (ranks > sufr::LZ_TILE_MAX) ranks = sufr::LZ_TILE_MAX;
    if (positions > sufr::LZ_TILE_MAX) positions = sufr::LZ_TILE_MAX;
    ctx->lz_rank_tile = (uint32_t)((ranks + 255) / 256 * 256);       // (0 stays 0: the default)
    ctx->lz_pos_tile = (uint32_t)((positions + 255) / 256 * 256);
    return 0;
}

int sufr_hip_lpf_device(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_lcp, const uint64_t* seq_starts, uint64_t num_sequences,
                        void* d_lpf, void* d_src)
{
    if (!ctx || !ix) return SUFR_HIP_E_INVALID;
    sufr::KmerSeqs q;
    if (const int rc = lz_prepare(ctx, ix, d_lcp, seq_starts, num_sequences, "lpf", q)) return rc;
    return by_width(ix, [&](auto w) { return lz_lpf_run(ctx, ix, d_lcp, q, (decltype(w)*)d_lpf, (decltype(w)*)d_src, "lpf"); });
}

int sufr_hip_lz_device(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_lcp, const uint64_t* seq_starts, uint64_t num_sequences,
                       uint64_t cap, void* d_start, void* d_length, void* d_source, uint64_t* total_out, sufr_lz_stats* stats_out)
{
    if (stats_out) *stats_out = sufr_lz_stats{0, 0, 0, 0};
    if (total_out) *total_out = 0;
    if (!ctx || !ix) return SUFR_HIP_E_INVALID;
    sufr::KmerSeqs q;
    if (const int rc = lz_prepare(ctx, ix, d_lcp, seq_starts, num_sequences, "lz", q)) return rc;
    if (!ix->ix.n) return 0;
    return by_width(ix, [&](auto w) { return lz_run<decltype(w)>(ctx, ix, d_lcp, q, cap, d_start, d_length, d_source, total_out, stats_out); });
}

}  // extern "C"
