// sufr_bwt.inc -- the BWT of the indexed text, its runs and the LF mapping, from the text and the SA of a device-resident
// index (included by sufr_kernels.hip after sufr_shared.inc; include/sufr_bwt.h, DESIGN.md section 22).
//
// Everything is cut into tiles of ranks (BWT_TILE_MAX at most, a multiple of 256), one tile per workgroup of 256 lanes at a
// time.  A run may cover any number of tiles and the stable rank of a symbol depends on every tile before it, so the passes
// over the tiles are joined by small serial sweeps over per-tile summaries; the arithmetic of the run carry is
// sufr_bwt_scan.h, which the host path compiles too.  All rank and position arithmetic is 64-bit.
//
// k_bwt_gather     a lane per rank: SA[r] coalesced, the one text byte in front of it (a random read), the tile's bytes in
//                  LDS and from there to memory as whole dwords.  A 256-bin histogram of the tile by LDS atomics (counts do
//                  not depend on the order) goes to the global counts; the tile's run summary (first and last symbol, the
//                  length of the run at either end) by LDS atomic min / max.
// k_bwt_carry      one workgroup sweeps the summaries from the last tile to the first (a backward tile_sweep of BwtLinkOp;
//                  sufr_scan.inc, DESIGN.md section 10.2): ext[t], the ranks beyond tile t that continue its last run.
// k_bwt_runs       a workgroup per tile over the BWT bytes: the run heads as ballot words in LDS, the next head of a head by a
//                  walk over those words, its length by bwt_run_length -- no lane reads beyond its tile.  Counting run: the
//                  tile's heads, kept heads and longest run.  Writing run: the kept heads' records behind the tile's base (a
//                  popcount prefix over the kept words).  Between the two, k_locate_scan (sufr_search.inc) turns the kept
//                  counts into bases and k_tile_best (sufr_repeat.inc) the candidates into the stats.
// k_bwt_cols       the 256 counts into C[c] and the column of every byte value that occurs.
// k_bwt_tile_hist  a workgroup per tile: the counts of the tile, one table column per occurring byte value.
// k_bwt_col_scan   a workgroup per column: the exclusive scan of the column down the tiles, a forward tile_sweep.
// k_bwt_rank       a workgroup per tile, a wave per quarter of it: the quarters' histograms give every wave its bases in LDS,
//                  then each wave takes 64 ranks at a time -- the lanes with the same symbol by eight ballots over the symbol
//                  bits, the rank from the base and the popcount of the lanes below, the base advanced by the group's lowest
//                  lane.  No rank comes from the arrival order of an atomic: the output is the same bits on every run.
// No scratch; LDS: k_bwt_gather 17 KB, k_bwt_runs 18 KB (counting) or 22 KB (writing), k_bwt_tile_hist 17 KB, k_bwt_rank 28 KB.

#include "sufr_bwt_scan.h"

namespace sufr {

static constexpr uint32_t BWT_TILE_MAX = 16384;         // ranks of a tile at most
static constexpr uint32_t BWT_NO_COL = 0xFFFFFFFFu;     // the column of a byte value that does not occur

struct BwtTile { uint32_t syms, pre, suf; };            // first | last << 8; the length of the run at the left / right end

// the bytes of tile [base, base + len) of the BWT into LDS, as dwords (base is a multiple of 256, the array padded to one)
__device__ __forceinline__ void bwt_stage(const uint8_t* __restrict__ bwt, uint64_t base, uint32_t len, uint32_t* s_w)
{
    const uint32_t* src = (const uint32_t*)(bwt + base);
    for (uint32_t i = threadIdx.x; i < (len + 3) / 4; i += 256) s_w[i] = src[i];
}

template <typename T>
__global__ __launch_bounds__(256) void k_bwt_gather(const T* __restrict__ sa, const uint8_t* __restrict__ text, uint64_t n, uint64_t s, uint32_t tile,
                                                    uint64_t ntiles, uint8_t* __restrict__ bwt, unsigned long long* __restrict__ counts,
                                                    BwtTile* __restrict__ sums)
{
    __shared__ uint32_t s_w[BWT_TILE_MAX / 4], s_h[256], s_pre, s_suf;
    uint8_t* s_b = (uint8_t*)s_w;
    s_h[threadIdx.x] = 0;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t base = t * tile;
        const uint32_t len = (uint32_t)(s - base < tile ? s - base : tile);
        if (threadIdx.x == 0) { s_pre = len; s_suf = 0; }
        __syncthreads();                                 // (s_h is zero, s_w is free)
        for (uint32_t i = threadIdx.x; i < len; i += 256) {
            const uint8_t c = text[bwt_source((uint64_t)sa[base + i], n)];
            s_b[i] = c;
            atomicAdd(&s_h[c], 1u);
        }
        __syncthreads();
        const uint32_t first = s_b[0], last = s_b[len - 1];
        if (sums) {
            for (uint32_t i = threadIdx.x; i < len; i += 256) {
                const uint32_t c = s_b[i];
                if (c != first) atomicMin(&s_pre, i);           // the first rank that is not the first symbol
                if (c != last) atomicMax(&s_suf, i + 1);        // behind the last rank that is not the last symbol
            }
        }
        if (bwt) {
            uint32_t* dst = (uint32_t*)(bwt + base);             // (base is a multiple of 256 and bwt of 4)
            for (uint32_t i = threadIdx.x; i < len / 4; i += 256) dst[i] = s_w[i];
            if (threadIdx.x < (len & 3u)) bwt[base + (len & ~3u) + threadIdx.x] = s_b[(len & ~3u) + threadIdx.x];
        }
        const uint32_t mine = s_h[threadIdx.x];
        if (mine) {
            if (counts) atomicAdd(&counts[threadIdx.x], (unsigned long long)mine);
            s_h[threadIdx.x] = 0;
        }
        __syncthreads();
        if (sums && threadIdx.x == 0) sums[t] = BwtTile{first | (last << 8), s_pre, len - s_suf};
    }
}

struct BwtLinkOp {
    using V = BwtLink;
    static __device__ __forceinline__ V identity() { return BwtLink{0, 1}; }
    static __device__ __forceinline__ V combine(const V& near, const V& far) { return bwt_chain(near, far); }
};

// ext[t]: the ranks beyond the end of tile t that continue its last run
__global__ __launch_bounds__(1024) void k_bwt_carry(const BwtTile* __restrict__ sums, uint64_t ntiles, uint32_t tile, uint64_t s, uint64_t* __restrict__ ext)
{
    __shared__ BwtLink s_l[16];
    // the link of tile t: what tile t + 1 gives its open run (behind the last tile there is nothing: ext = 0 passes through)
    const auto link = [&](uint64_t t) {
        if (t + 1 >= ntiles) return BwtLinkOp::identity();
        const BwtTile cur = sums[t], nx = sums[t + 1];
        const uint64_t nb = (t + 1) * tile;
        return bwt_link(cur.syms >> 8, nx.syms & 255u, nx.pre, s - nb < tile ? s - nb : tile);
    };
    tile_sweep<BwtLinkOp, true>(ntiles, link, [&](uint64_t t, const BwtLink& own, const BwtLink& after) { ext[t] = bwt_chain(own, after).add; }, s_l);
}

// WRITE false: t_cnt[t] = the kept heads of tile t, t_stat[3 t ..] = {heads, longest, longest_rank} of the runs that start in
// it.  WRITE true: t_cnt[t] is the tile's base (the exclusive scan of the counts); the records of its kept heads go behind it.
template <typename T, bool WRITE>
__global__ __launch_bounds__(256) void k_bwt_runs(const T* __restrict__ sa, const uint8_t* __restrict__ bwt, uint64_t s, uint32_t tile, uint64_t ntiles,
                                                  const uint64_t* __restrict__ ext, uint64_t min_len, uint64_t* __restrict__ t_cnt,
                                                  uint64_t* __restrict__ t_stat, uint64_t* __restrict__ o_rank, uint64_t* __restrict__ o_len,
                                                  uint64_t* __restrict__ o_sym, uint64_t* __restrict__ o_first)
{
    __shared__ uint32_t s_w[BWT_TILE_MAX / 4];
    using Stat = SumBestOp<2>;
    __shared__ uint64_t s_hd[BWT_TILE_MAX / 64], s_kp[BWT_TILE_MAX / 64], s_pf[BWT_TILE_MAX / 64], s_sc[4];
    __shared__ Stat::V s_b4[4];
    const uint8_t* s_b = (const uint8_t*)s_w;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t base = t * tile;
        const uint32_t len = (uint32_t)(s - base < tile ? s - base : tile), span = (len + 255u) & ~255u, nwords = (len + 63) / 64;
        const uint32_t prev = base ? bwt[base - 1] : 256u;      // (256 is no byte: rank 0 is a head)
        const uint64_t beyond = ext[t];
        bwt_stage(bwt, base, len, s_w);
        __syncthreads();
        for (uint32_t it = 0; it < span; it += 256) {     // (uniform: every lane of a wave takes part in the ballot)
            const uint32_t i = it + threadIdx.x;
            const uint64_t m = __ballot(i < len && (uint32_t)s_b[i] != (i ? (uint32_t)s_b[i - 1] : prev));
            if (lane == 0) s_hd[(it >> 6) + w] = m;
        }
        __syncthreads();
        Stat::V b = Stat::identity();                    // {heads, kept heads, longest, longest_rank}
        // the length of the run whose head is at i
        auto run_length = [&](uint32_t i) {
            uint32_t word = i >> 6;
            uint64_t m = (i & 63u) == 63u ? 0 : s_hd[word] & (~(uint64_t)0 << ((i & 63u) + 1));
            while (!m && ++word < nwords) m = s_hd[word];
            return bwt_run_length(i, m ? word * 64 + (uint32_t)__builtin_ctzll(m) : len, len, beyond);
        };
        for (uint32_t it = 0; it < span; it += 256) {
            const uint32_t i = it + threadIdx.x;
            const bool head = (s_hd[i >> 6] >> (i & 63u)) & 1;
            uint64_t l = 0;
            if (head) {
                l = run_length(i);
                b.sum[0]++;
                if (rep_better(l, base + i, b.len, b.at)) { b.len = l; b.at = base + i; }      // (a lane's ranks ascend: ties keep the first)
            }
            const uint64_t m = __ballot(head && l >= min_len);
            if (WRITE) { if (lane == 0) s_kp[(it >> 6) + w] = m; }
            else if (lane == 0) b.sum[1] += (uint64_t)__builtin_popcountll(m);
        }
        if (!WRITE) {
            b = wg_reduce_op<Stat, 4>(b, s_b4);
            if (threadIdx.x == 0) { t_cnt[t] = b.sum[1]; t_stat[3 * t] = b.sum[0]; t_stat[3 * t + 1] = b.len; t_stat[3 * t + 2] = b.at; }
        } else {
            __syncthreads();
            uint64_t v[1] = {threadIdx.x < nwords ? (uint64_t)__builtin_popcountll(s_kp[threadIdx.x]) : 0}, tot[1];
            wg_scan(v, tot, s_sc);
            s_pf[threadIdx.x] = v[0];
            __syncthreads();
            const uint64_t out = t_cnt[t];
            for (uint32_t it = 0; it < span; it += 256) {
                const uint32_t i = it + threadIdx.x;
                const uint64_t m = s_kp[i >> 6];
                if (!((m >> (i & 63u)) & 1)) continue;
                const uint64_t o = out + s_pf[i >> 6] + (uint64_t)__builtin_popcountll(m & (((uint64_t)1 << (i & 63u)) - 1));
                o_rank[o] = base + i; o_len[o] = run_length(i); o_sym[o] = s_b[i]; o_first[o] = (uint64_t)sa[base + i];
            }
        }
        __syncthreads();                                 // (the LDS arrays are the next tile's)
    }
}

// cbase[c] = C[c]; col[c]: the number of occurring byte values below c where c occurs, BWT_NO_COL where it does not
__global__ __launch_bounds__(256) void k_bwt_cols(const unsigned long long* __restrict__ counts, uint64_t* __restrict__ cbase, uint32_t* __restrict__ col)
{
    __shared__ uint64_t s_sc[8];
    const uint64_t c = counts[threadIdx.x];
    uint64_t v[2] = {c, c ? (uint64_t)1 : 0}, tot[2];
    wg_scan(v, tot, s_sc);
    cbase[threadIdx.x] = v[0];
    col[threadIdx.x] = c ? (uint32_t)v[1] : BWT_NO_COL;
}

// tab[t K + col[c]] = the ranks of tile t with BWT[r] == c
__global__ __launch_bounds__(256) void k_bwt_tile_hist(const uint8_t* __restrict__ bwt, uint64_t s, uint32_t tile, uint64_t ntiles,
                                                       const uint32_t* __restrict__ col, uint32_t K, uint64_t* __restrict__ tab)
{
    __shared__ uint32_t s_w[BWT_TILE_MAX / 4], s_h[256];
    const uint8_t* s_b = (const uint8_t*)s_w;
    const uint32_t my_col = col[threadIdx.x];
    s_h[threadIdx.x] = 0;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t base = t * tile;
        const uint32_t len = (uint32_t)(s - base < tile ? s - base : tile);
        __syncthreads();                                 // (s_h is zero, s_w is free)
        bwt_stage(bwt, base, len, s_w);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < len; i += 256) atomicAdd(&s_h[s_b[i]], 1u);
        __syncthreads();
        if (my_col != BWT_NO_COL) tab[t * K + my_col] = s_h[threadIdx.x];
        s_h[threadIdx.x] = 0;
    }
}

// column blockIdx.x of tab, in place: the exclusive scan down the tiles
__global__ __launch_bounds__(1024) void k_bwt_col_scan(uint64_t* __restrict__ tab, uint64_t ntiles, uint32_t K)
{
    __shared__ uint64_t s_sc[16];
    uint64_t* col = tab + blockIdx.x;
    tile_sweep<SumOp<uint64_t>, false>(
        ntiles, [&](uint64_t t) { return col[t * K]; }, [&](uint64_t t, uint64_t, uint64_t before) { col[t * K] = before; }, s_sc);
}

// lf[r] = C[c] + the ranks before r with the symbol c of r: cbase, the tile's row of tab, the quarters before r's and the
// lanes below r's
template <typename T>
__global__ __launch_bounds__(256) void k_bwt_rank(const uint8_t* __restrict__ bwt, uint64_t s, uint32_t tile, uint64_t ntiles,
                                                  const uint64_t* __restrict__ cbase, const uint32_t* __restrict__ col, uint32_t K,
                                                  const uint64_t* __restrict__ tab, T* __restrict__ lf)
{
    __shared__ uint32_t s_w[BWT_TILE_MAX / 4], s_h[4][256];
    __shared__ uint64_t s_run[4][256];
    const uint8_t* s_b = (const uint8_t*)s_w;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t my_col = col[threadIdx.x];
    const uint64_t my_c = cbase[threadIdx.x];
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t base = t * tile;
        const uint32_t len = (uint32_t)(s - base < tile ? s - base : tile);
        const uint32_t quarter = ((len + 3) / 4 + 63u) & ~63u;                  // ranks of a wave: whole groups of 64
        const uint32_t lo = w * quarter < len ? w * quarter : len, hi = lo + quarter < len ? lo + quarter : len;
        bwt_stage(bwt, base, len, s_w);
        for (uint32_t k = 0; k < 4; k++) s_h[k][threadIdx.x] = 0;
        __syncthreads();
        for (uint32_t i = lo + lane; i < hi; i += 64) atomicAdd(&s_h[w][s_b[i]], 1u);
        __syncthreads();
        uint64_t b = my_c + (my_col != BWT_NO_COL ? tab[t * K + my_col] : 0);
        for (uint32_t k = 0; k < 4; k++) { s_run[k][threadIdx.x] = b; b += s_h[k][threadIdx.x]; }
        __syncthreads();
        for (uint32_t i0 = lo; i0 < hi; i0 += 64) {       // (uniform in the wave; only this wave touches s_run[w])
            const uint32_t i = i0 + lane;
            const bool act = i < hi;
            const uint32_t c = act ? s_b[i] : 0;
            uint64_t same = __ballot(act);                // the lanes with this lane's symbol
            for (uint32_t bit = 0; bit < 8; bit++) {
                const uint64_t m = __ballot(act && ((c >> bit) & 1));
                same &= (c >> bit) & 1 ? m : ~m;
            }
            const uint32_t below = (uint32_t)__builtin_popcountll(same & (((uint64_t)1 << lane) - 1));
            const uint64_t at = __hip_atomic_load(&s_run[w][c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            if (act) lf[base + i] = (T)(at + below);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");             // (every lane has read its base before a base moves)
            if (act && !below)
                __hip_atomic_store(&s_run[w][c], at + (uint64_t)__builtin_popcountll(same), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");             // (... and the next 64 ranks read the moved ones)
        }
        __syncthreads();                                 // (the LDS arrays are the next tile's)
    }
}

}  // namespace sufr

namespace {

uint32_t bwt_tile(const sufr_hip_ctx* ctx) { return ctx->bwt_tile ? ctx->bwt_tile : sufr::BWT_TILE_MAX; }

// the gather of all three calls: the BWT into bwt, the counts added to counts, the tile summaries into sums (each may be null)
template <typename T>
void bwt_gather(sufr_hip_ctx* ctx, const sufr_hip_index* ix, uint8_t* bwt, unsigned long long* counts, sufr::BwtTile* sums)
{
    sufr::Pipeline& pl = ctx->pl;
    const uint32_t tile = bwt_tile(ctx);
    const uint64_t ntiles = (ix->ix.s + tile - 1) / tile, wgs = batch_grid(pl);
    hipLaunchKernelGGL(sufr::k_bwt_gather<T>, dim3((uint32_t)(ntiles < wgs ? ntiles : wgs)), dim3(256), 0, pl.stream, index_sa<T>(ix), ix->ix.text,
                       ix->ix.n, ix->ix.s, tile, ntiles, bwt, counts, sums);
}

template <typename T>
int bwt_runs_run(sufr_hip_ctx* ctx, const sufr_hip_index* ix, uint64_t min_len, uint64_t cap, void* d_rank, void* d_length, void* d_symbol,
                 void* d_first, uint64_t* total_out, sufr_bwt_stats* stats_out)
{
    sufr::Pipeline& pl = ctx->pl;
    const uint64_t s = ix->ix.s;
    const uint32_t tile = bwt_tile(ctx);
    const uint64_t ntiles = (s + tile - 1) / tile;
    int rc;
    // bwtbytes: the BWT (padded to a dword); bwtsum: per tile ext (8), the kept count, then base (8) and the three candidates
    // (24), then the total and the four stats, then the tile summaries (12 each)
    if ((rc = pl.ensure(ctx->bwtbytes, s + 8)) || (rc = pl.ensure(ctx->bwtsum, ntiles * (40 + sizeof(sufr::BwtTile)) + 5 * 8))) return rc;
    uint8_t* bwt = (uint8_t*)ctx->bwtbytes.p;
    uint64_t* ext = (uint64_t*)ctx->bwtsum.p;
    uint64_t *t_cnt = ext + ntiles, *d_total = t_cnt + ntiles, *t_stat = d_total + 1, *d_stats = t_stat + 3 * ntiles;
    sufr::BwtTile* sums = (sufr::BwtTile*)(d_stats + 4);
    bwt_gather<T>(ctx, ix, bwt, nullptr, sums);
    hipLaunchKernelGGL(sufr::k_bwt_carry, dim3(1), dim3(1024), 0, pl.stream, (const sufr::BwtTile*)sums, ntiles, tile, s, ext);
    const uint64_t wgs = batch_grid(pl);
    const uint32_t grid = (uint32_t)(ntiles < wgs ? ntiles : wgs);
    const T* sa = index_sa<T>(ix);
    hipLaunchKernelGGL((sufr::k_bwt_runs<T, false>), dim3(grid), dim3(256), 0, pl.stream, sa, (const uint8_t*)bwt, s, tile, ntiles, (const uint64_t*)ext,
                       min_len, t_cnt, t_stat, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr);
    hipLaunchKernelGGL(sufr::k_locate_scan, dim3(1), dim3(1024), 0, pl.stream, t_cnt, ntiles, d_total);
    // {the total, the sum of the first column, the best (length, rank)} = {records, runs, longest, longest_rank}
    hipLaunchKernelGGL(sufr::k_tile_best<sufr::SumBestOp<1>>, dim3(1), dim3(1024), 0, pl.stream, (const uint64_t*)t_stat, ntiles, (const uint64_t*)d_total, d_stats);
    unsigned long long h[4];
    rc = report_total(pl, "bwt_runs", "records", d_stats, 4, h, cap, total_out, d_rank && d_length && d_symbol && d_first);
    if (stats_out) *stats_out = sufr_bwt_stats{h[1], h[0], h[2], h[3]};
    if (rc || !h[0]) return rc;
    hipLaunchKernelGGL((sufr::k_bwt_runs<T, true>), dim3(grid), dim3(256), 0, pl.stream, sa, (const uint8_t*)bwt, s, tile, ntiles, (const uint64_t*)ext,
                       min_len, t_cnt, t_stat, (uint64_t*)d_rank, (uint64_t*)d_length, (uint64_t*)d_symbol, (uint64_t*)d_first);
    return launch_status(pl, "bwt_runs");
}

template <typename T>
int bwt_lf_run(sufr_hip_ctx* ctx, const sufr_hip_index* ix, T* lf)
{
    sufr::Pipeline& pl = ctx->pl;
    const uint64_t s = ix->ix.s;
    const uint32_t tile = bwt_tile(ctx);
    const uint64_t ntiles = (s + tile - 1) / tile;
    int rc;
    // bwtsum: the 256 counts, C (256 u64), the columns (256 u32); bwttab: a row of K bases per tile
    if ((rc = pl.ensure(ctx->bwtbytes, s + 8)) || (rc = pl.ensure(ctx->bwtsum, 256 * 20))) return rc;
    uint8_t* bwt = (uint8_t*)ctx->bwtbytes.p;
    unsigned long long* counts = (unsigned long long*)ctx->bwtsum.p;
    uint64_t* cbase = (uint64_t*)(counts + 256);
    uint32_t* col = (uint32_t*)(cbase + 256);
    if (hipMemsetAsync(counts, 0, 256 * 8, pl.stream) != hipSuccess) { pl.set_error("lf: memset failed"); return SUFR_HIP_E_HIP; }
    bwt_gather<T>(ctx, ix, bwt, counts, nullptr);
    unsigned long long h[256];
    if ((rc = launch_status(pl, "lf")) || (rc = read_totals(pl, counts, 256, h, "lf", "reading the byte counts failed"))) return rc;
    uint32_t K = 0;
    for (int c = 0; c < 256; c++) K += h[c] ? 1 : 0;
    if ((rc = pl.ensure(ctx->bwttab, ntiles * K * 8))) return rc;
    uint64_t* tab = (uint64_t*)ctx->bwttab.p;
    const uint64_t wgs = batch_grid(pl);
    const uint32_t grid = (uint32_t)(ntiles < wgs ? ntiles : wgs);
    hipLaunchKernelGGL(sufr::k_bwt_cols, dim3(1), dim3(256), 0, pl.stream, (const unsigned long long*)counts, cbase, col);
    hipLaunchKernelGGL(sufr::k_bwt_tile_hist, dim3(grid), dim3(256), 0, pl.stream, (const uint8_t*)bwt, s, tile, ntiles, (const uint32_t*)col, K, tab);
    hipLaunchKernelGGL(sufr::k_bwt_col_scan, dim3(K), dim3(1024), 0, pl.stream, tab, ntiles, K);
    hipLaunchKernelGGL(sufr::k_bwt_rank<T>, dim3(grid), dim3(256), 0, pl.stream, (const uint8_t*)bwt, s, tile, ntiles, (const uint64_t*)cbase,
                       (const uint32_t*)col, K, (const uint64_t*)tab, lf);
    return launch_status(pl, "lf");
}

// what all three calls check before they touch the device (there are no refusals: a seed-mask index is as good as any)
int bwt_prepare(sufr_hip_ctx* ctx, const sufr_hip_index* ix)
{
    ctx->pl.err.clear();
    return query_check(ctx, ix);
}

}  // namespace

extern "C" {

int sufr_hip_set_bwt_tile(sufr_hip_ctx* ctx, uint64_t ranks)
{
    if (!ctx) return SUFR_HIP_E_INVALID;
    if (ranks > sufr::BWT_TILE_MAX) ranks = sufr::BWT_TILE_MAX;
    ctx->bwt_tile = (uint32_t)((ranks + 255) / 256 * 256);           // (0 stays 0: the default)
    return 0;
}

int sufr_hip_bwt_device(sufr_hip_ctx* ctx, const sufr_hip_index* ix, void* d_bwt, void* d_counts)
{
    if (!ctx || !ix) return SUFR_HIP_E_INVALID;
    if (const int rc = bwt_prepare(ctx, ix)) return rc;
    if ((uintptr_t)d_bwt & 3) { ctx->pl.set_error("bwt: the output is not aligned to 4 bytes"); return SUFR_HIP_E_INVALID; }
    if (d_counts && hipMemsetAsync(d_counts, 0, 256 * 8, ctx->pl.stream) != hipSuccess) { ctx->pl.set_error("bwt: memset failed"); return SUFR_HIP_E_HIP; }
    if (!ix->ix.s || (!d_bwt && !d_counts)) return 0;
    by_width(ix, [&](auto w) { bwt_gather<decltype(w)>(ctx, ix, (uint8_t*)d_bwt, (unsigned long long*)d_counts, nullptr); return 0; });
    return launch_status(ctx->pl, "bwt");
}

int sufr_hip_bwt_runs_device(sufr_hip_ctx* ctx, const sufr_hip_index* ix, uint64_t min_len, uint64_t cap, void* d_rank, void* d_length, void* d_symbol,
                             void* d_first, uint64_t* total_out, sufr_bwt_stats* stats_out)
{
    if (stats_out) *stats_out = sufr_bwt_stats{0, 0, 0, 0};
    if (total_out) *total_out = 0;
    if (!ctx || !ix) return SUFR_HIP_E_INVALID;
    if (const int rc = bwt_prepare(ctx, ix)) return rc;
    if (!ix->ix.s) return 0;
    return by_width(ix, [&](auto w) {
        return bwt_runs_run<decltype(w)>(ctx, ix, sufr::bwt_min_len(min_len), cap, d_rank, d_length, d_symbol, d_first, total_out, stats_out);
    });
}

int sufr_hip_lf_device(sufr_hip_ctx* ctx, const sufr_hip_index* ix, void* d_lf)
{
    if (!ctx || !ix) return SUFR_HIP_E_INVALID;
    if (const int rc = bwt_prepare(ctx, ix)) return rc;
    if (!ix->ix.s || !d_lf) return 0;
    return by_width(ix, [&](auto w) { return bwt_lf_run(ctx, ix, (decltype(w)*)d_lf); });
}

}  // extern "C"
