// sufr_kmer.inc -- k-mer spectra, occurrence maps and unique lengths from the SA and the LCP of a device-resident index
// (included by sufr_kernels.hip after sufr_trace.inc; include/sufr_kmer.h, DESIGN.md section 18).
//
// The count of a rank is a segmented sum whose segments (k-intervals) may be as long as the array, so no rank may assume
// that its interval ends inside its tile.  The arithmetic -- the summary of a stretch of ranks, its combine operator, the
// carries, the count of one rank of a 64-rank word -- is sufr_kmer_scan.h, which the host path and tests/kmer_shim.cpp
// compile too; this file only moves the data.
//
// The scans and the sweep are those of sufr_scan.inc (DESIGN.md section 10.2) over KmerOp.
// k_kmer_fold    one pass over SA and LCP.  A wave takes 64 consecutive ranks: head = (r == 0 or LCP[r] < k), whole =
//                (brk(SA[r]) - SA[r] >= k, a binary search of the sequence starts), two __ballot words per wave, stored
//                (s / 4 bytes in all).  A tile is up to 256 words, one per lane: the total of wg_scan_op over their
//                summaries is the tile's.
// k_kmer_carry   two tile_sweeps over the tile summaries: forward, carry_in[t] = whole ranks of the interval open at the
//                start of tile t; backward, carry_out[t] = whole ranks after its end up to the next head.
// k_kmer_apply   one pass over the words (no SA, no LCP).  The same workgroup scan gives every word its carries; after that
//                a rank's count is bit arithmetic on the two words of its wave.  occ goes out by rank, or through SA into a
//                zeroed by-position buffer (non-zero values only).  Every interval is credited once, by the lane of its
//                head: count 1 by a ballot per wave, the rest by integer atomics on private LDS bins (up to KMER_LDS_BINS,
//                merged into the global bins at the end) or, with more bins, on the global bins.  Nothing is a float, so
//                the result does not depend on the order.
// k_unique_len   elementwise: LCP[r], LCP[r+1], SA[r], brk.
// A workgroup takes tiles t = blockIdx.x, blockIdx.x + gridDim.x, ...; no scratch, 20 KB of LDS at most.

#include "sufr_kmer_scan.h"

namespace sufr {

static constexpr uint32_t KMER_TILE_MAX = 16384;        // ranks of a tile at most: 256 words, one per lane
static constexpr uint32_t KMER_LDS_BINS = 1024;         // histogram bins a workgroup keeps in LDS; more go to the global bins

struct KmerSeqs { const uint64_t* starts; uint64_t num, n; };

struct KmerOp {
    using V = KmerSum;
    static __device__ __forceinline__ V identity() { return kmer_identity(); }
    static __device__ __forceinline__ V combine(const V& a, const V& b) { return kmer_combine(a, b); }
};

template <typename T>
__global__ __launch_bounds__(256) void k_kmer_fold(const T* __restrict__ sa, const T* __restrict__ lcp, uint64_t s, KmerSeqs q, uint64_t k,
                                                   uint32_t tile, uint64_t ntiles, uint64_t* __restrict__ hbits, uint64_t* __restrict__ wbits,
                                                   uint64_t* __restrict__ t_pre, uint64_t* __restrict__ t_post, uint64_t* __restrict__ t_has)
{
    __shared__ uint64_t s_h[256], s_w[256];
    __shared__ KmerSum s_k[4];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, nw = tile >> 6;      // (tile: a multiple of 256)
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        for (uint32_t j = w; j < nw; j += 4) {
            const uint64_t r = t * tile + (uint64_t)j * 64 + lane;
            bool head = false, whole = false;
            if (r < s) {
                head = r == 0 || (uint64_t)lcp[r] < k;
                whole = kmer_whole(q.starts, q.num, q.n, (uint64_t)sa[r], k);
            }
            const uint64_t H = __ballot(head), W = __ballot(whole);
            if (lane == 0) { s_h[j] = H; s_w[j] = W; hbits[t * nw + j] = H; wbits[t * nw + j] = W; }
        }
        __syncthreads();
        const KmerSum mine = threadIdx.x < nw ? kmer_word_sum(s_h[threadIdx.x], s_w[threadIdx.x]) : kmer_identity();
        const WgScan<KmerSum> sc = wg_scan_op<KmerOp, 4>(mine, s_k);
        if (threadIdx.x == 0) { t_pre[t] = sc.total.pre; t_post[t] = sc.total.post; t_has[t] = sc.total.has; }
    }
}

__global__ __launch_bounds__(1024) void k_kmer_carry(const uint64_t* __restrict__ t_pre, const uint64_t* __restrict__ t_post,
                                                     const uint64_t* __restrict__ t_has, uint64_t ntiles, uint64_t* __restrict__ cin,
                                                     uint64_t* __restrict__ cout)
{
    __shared__ KmerSum s_k[16];
    const auto load = [&](uint64_t t) { return KmerSum{t_pre[t], t_post[t], (uint32_t)t_has[t]}; };
    tile_sweep<KmerOp, false>(ntiles, load, [&](uint64_t t, const KmerSum&, const KmerSum& before) { cin[t] = kmer_carry_in(before, 0); }, s_k);
    tile_sweep<KmerOp, true>(ntiles, load, [&](uint64_t t, const KmerSum&, const KmerSum& after) { cout[t] = kmer_carry_out(after, 0); }, s_k);
}

// stats: whole, distinct, unique, max_count
template <typename T>
__global__ __launch_bounds__(256) void k_kmer_apply(const T* __restrict__ sa, uint64_t s, uint32_t tile, uint64_t ntiles,
                                                    const uint64_t* __restrict__ hbits, const uint64_t* __restrict__ wbits,
                                                    const uint64_t* __restrict__ cin, const uint64_t* __restrict__ cout,
                                                    T* __restrict__ occ, uint32_t by_position, uint64_t bins,
                                                    unsigned long long* __restrict__ hist, unsigned long long* __restrict__ stats)
{
    __shared__ uint64_t s_h[256], s_w[256], s_ci[256], s_co[256];
    __shared__ KmerSum s_k[4];
    __shared__ unsigned long long s_bins[KMER_LDS_BINS];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, nw = tile >> 6;
    const bool private_bins = hist && bins <= KMER_LDS_BINS;
    if (private_bins) for (uint32_t i = threadIdx.x; i < bins; i += 256) s_bins[i] = 0;
    __syncthreads();
    uint64_t n_whole = 0, n_distinct = 0, n_unique = 0;  // the same in every lane of a wave
    uint64_t c_max = 0;                                  // per lane
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        uint64_t H = 0, W = 0;
        if (threadIdx.x < nw) { H = hbits[t * nw + threadIdx.x]; W = wbits[t * nw + threadIdx.x]; }
        const WgScan<KmerSum> sc = wg_scan_op<KmerOp, 4, true>(threadIdx.x < nw ? kmer_word_sum(H, W) : kmer_identity(), s_k);
        s_h[threadIdx.x] = H; s_w[threadIdx.x] = W;
        s_ci[threadIdx.x] = kmer_carry_in(sc.before, cin[t]);
        s_co[threadIdx.x] = kmer_carry_out(sc.after, cout[t]);
        __syncthreads();
        for (uint32_t j = w; j < nw; j += 4) {
            const uint64_t r = t * tile + (uint64_t)j * 64 + lane;
            if (r - lane >= s) break;                    // (uniform: the words past the end of the array)
            const uint64_t Hj = s_h[j], Wj = s_w[j];
            const uint64_t c = kmer_rank_count(Hj, Wj, lane, s_ci[j], s_co[j]);
            const bool whole = (Wj >> lane) & 1, head = (Hj >> lane) & 1;
            if (occ && r < s) {
                if (!by_position) occ[r] = (T)(whole ? c : 0);
                else if (whole) occ[(uint64_t)sa[r]] = (T)c;
            }
            const bool credit = head && c > 0;
            const uint64_t ones = __ballot(credit && c == 1), any = __ballot(credit);
            n_whole += (uint64_t)__builtin_popcountll(Wj);
            n_distinct += (uint64_t)__builtin_popcountll(any);
            n_unique += (uint64_t)__builtin_popcountll(ones);
            if (credit && c > 1) {
                if (c > c_max) c_max = c;
                if (private_bins) atomicAdd(&s_bins[kmer_bin(c, bins)], 1ull);
                else if (hist) atomicAdd(&hist[kmer_bin(c, bins)], 1ull);
            }
        }
        __syncthreads();                                 // (the words are replaced by the next tile)
    }
    if (n_unique && c_max == 0) c_max = 1;
    for (int o = 32; o > 0; o >>= 1) { const uint64_t u = __shfl_down(c_max, o); if (u > c_max) c_max = u; }
    if (lane == 0) {
        if (n_unique) {
            if (private_bins) atomicAdd(&s_bins[0], (unsigned long long)n_unique);
            else if (hist) atomicAdd(&hist[0], (unsigned long long)n_unique);
        }
        if (stats) {
            if (n_whole) atomicAdd(&stats[0], (unsigned long long)n_whole);
            if (n_distinct) atomicAdd(&stats[1], (unsigned long long)n_distinct);
            if (n_unique) atomicAdd(&stats[2], (unsigned long long)n_unique);
            if (c_max) atomicMax(&stats[3], (unsigned long long)c_max);
        }
    }
    if (private_bins) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < bins; i += 256) if (s_bins[i]) atomicAdd(&hist[i], s_bins[i]);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_unique_len(const T* __restrict__ sa, const T* __restrict__ lcp, uint64_t s, KmerSeqs q,
                                                    uint32_t by_position, T* __restrict__ out)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < s; r += stride) {
        const uint64_t a = (uint64_t)lcp[r], b = r + 1 < s ? (uint64_t)lcp[r + 1] : 0, p = (uint64_t)sa[r];
        const uint64_t u = 1 + (a > b ? a : b);
        const uint64_t v = kmer_whole(q.starts, q.num, q.n, p, u) ? u : 0;
        if (!by_position) out[r] = (T)v;
        else if (v) out[p] = (T)v;
    }
}

}  // namespace sufr

namespace {

// the refusals both calls share, then the sequence starts of the call on the device (q); `what` names the call
int kmer_prepare(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_lcp, const uint64_t* seq_starts, uint64_t num_sequences,
                 const char* what, sufr::KmerSeqs& q)
{
    sufr::Pipeline& pl = ctx->pl;
    const uint64_t n = ix->ix.n;
    q = sufr::KmerSeqs{nullptr, 0, n};
    if (!ix->ix.s) return 0;
    if (!d_lcp) { pl.set_error(std::string(what) + ": no LCP array"); return SUFR_HIP_E_INVALID; }
    if (!seq_starts || !num_sequences) return 0;
    bool ok = seq_starts[0] == 0;
    for (uint64_t i = 0; ok && i < num_sequences; i++) ok = seq_starts[i] < n && (i == 0 || seq_starts[i] > seq_starts[i - 1]);
    if (!ok) { pl.set_error(std::string(what) + ": the sequence starts must ascend from 0 and stay below the text length"); return SUFR_HIP_E_INVALID; }
    if (num_sequences < 2) return 0;
    // the copy on the device is kept while the starts stay the same; before it is replaced, what may still read it ends
    std::vector<uint64_t>& have = ctx->kmer_starts;
    if (have.size() != num_sequences || memcmp(have.data(), seq_starts, num_sequences * 8) != 0 || !ctx->kstarts.p) {
        if (hipStreamSynchronize(pl.stream) != hipSuccess) { pl.set_error(std::string(what) + ": waiting for the stream failed"); return SUFR_HIP_E_HIP; }
        have.assign(seq_starts, seq_starts + num_sequences);
        if (const int rc = pl.ensure(ctx->kstarts, num_sequences * 8)) { have.clear(); return rc; }
        if (hipMemcpyAsync(ctx->kstarts.p, have.data(), num_sequences * 8, hipMemcpyHostToDevice, pl.stream) != hipSuccess) {
            have.clear();
            pl.set_error(std::string(what) + ": copying the sequence starts failed");
            return SUFR_HIP_E_HIP;
        }
    }
    q.starts = (const uint64_t*)ctx->kstarts.p;
    q.num = num_sequences;
    return 0;
}

// an empty array: a by-position output is all zeros, there is nothing else to do
int kmer_nothing(sufr::Pipeline& pl, void* d_by_position, uint64_t bytes)
{
    if (d_by_position && bytes && hipMemsetAsync(d_by_position, 0, bytes, pl.stream) != hipSuccess) { pl.set_error("kmers: memset failed"); return SUFR_HIP_E_HIP; }
    return 0;
}

template <typename T>
int kmers_run(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_lcp, const sufr::KmerSeqs& q, uint64_t k, bool by_position,
              uint64_t bins, void* d_hist, void* d_occ, sufr_kmer_stats* stats_out)
{
    sufr::Pipeline& pl = ctx->pl;
    const uint64_t s = ix->ix.s;
    const uint32_t tile = ctx->kmer_tile ? ctx->kmer_tile : sufr::KMER_TILE_MAX;
    const uint64_t ntiles = (s + tile - 1) / tile, nwords = ntiles * (tile / 64);
    int rc;
    // kbits: the head words, then the whole words; ksum: pre, post, has, carry_in, carry_out per tile, then the four stats
    if ((rc = pl.ensure(ctx->kbits, nwords * 16)) || (rc = pl.ensure(ctx->ksum, (ntiles * 5 + 4) * 8))) return rc;
    uint64_t* hbits = (uint64_t*)ctx->kbits.p;
    uint64_t* wbits = hbits + nwords;
    uint64_t* t_pre = (uint64_t*)ctx->ksum.p;
    uint64_t *t_post = t_pre + ntiles, *t_has = t_post + ntiles, *cin = t_has + ntiles, *cout = cin + ntiles;
    unsigned long long* d_stats = (unsigned long long*)(cout + ntiles);
    bool ok = hipMemsetAsync(d_stats, 0, 32, pl.stream) == hipSuccess;
    if (by_position && d_occ) ok = ok && hipMemsetAsync(d_occ, 0, q.n * sizeof(T), pl.stream) == hipSuccess;
    if (!ok) { pl.set_error("kmers: memset failed"); return SUFR_HIP_E_HIP; }
    const T* sa = index_sa<T>(ix);
    const uint64_t wgs = batch_grid(pl);
    const uint32_t grid = (uint32_t)(ntiles < wgs ? ntiles : wgs);
    hipLaunchKernelGGL(sufr::k_kmer_fold<T>, dim3(grid), dim3(256), 0, pl.stream, sa, (const T*)d_lcp, s, q, k, tile, ntiles, hbits, wbits,
                       t_pre, t_post, t_has);
    hipLaunchKernelGGL(sufr::k_kmer_carry, dim3(1), dim3(1024), 0, pl.stream, (const uint64_t*)t_pre, (const uint64_t*)t_post,
                       (const uint64_t*)t_has, ntiles, cin, cout);
    hipLaunchKernelGGL(sufr::k_kmer_apply<T>, dim3(grid), dim3(256), 0, pl.stream, sa, s, tile, ntiles, (const uint64_t*)hbits,
                       (const uint64_t*)wbits, (const uint64_t*)cin, (const uint64_t*)cout, (T*)d_occ, (uint32_t)by_position, bins,
                       (unsigned long long*)d_hist, d_stats);
    if ((rc = launch_status(pl, "kmers"))) return rc;
    if (stats_out) {
        unsigned long long h[4];
        if ((rc = read_totals(pl, d_stats, 4, h, "kmers", "reading the stats failed"))) return rc;
        *stats_out = sufr_kmer_stats{h[0], h[1], h[2], h[3]};
    }
    return 0;
}

}  // namespace

extern "C" {

int sufr_hip_set_kmer_tile(sufr_hip_ctx* ctx, uint64_t ranks)
{
    if (!ctx) return SUFR_HIP_E_INVALID;
    if (ranks > sufr::KMER_TILE_MAX) ranks = sufr::KMER_TILE_MAX;
    ctx->kmer_tile = (uint32_t)((ranks + 255) / 256 * 256);          // (0 stays 0: the default)
    return 0;
}

int sufr_hip_kmers_device(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_lcp, const uint64_t* seq_starts,
                          uint64_t num_sequences, uint64_t k, uint32_t flags, uint64_t bins, void* d_hist, void* d_occ,
                          sufr_kmer_stats* stats_out)
{
    if (stats_out) *stats_out = sufr_kmer_stats{0, 0, 0, 0};
    if (!ctx || !ix) return SUFR_HIP_E_INVALID;
    sufr::Pipeline& pl = ctx->pl;
    pl.err.clear();
    int rc;
    if ((rc = query_check(ctx, ix, "k-mer counts"))) return rc;
    if (ix->built_mql > 0 && k > ix->built_mql) {
        pl.set_error("kmers: the index was built with max_query_len " + std::to_string(ix->built_mql) + ", its LCP says nothing about k = " + std::to_string(k));
        return SUFR_HIP_E_UNSUPPORTED;
    }
    if (k == 0) { pl.set_error("kmers: k must be at least 1"); return SUFR_HIP_E_INVALID; }
    if (d_hist && bins == 0) { pl.set_error("kmers: a histogram needs at least one bin"); return SUFR_HIP_E_INVALID; }
    if (d_hist && hipMemsetAsync(d_hist, 0, bins * 8, pl.stream) != hipSuccess) { pl.set_error("kmers: memset failed"); return SUFR_HIP_E_HIP; }
    sufr::KmerSeqs q;
    const bool by_position = (flags & SUFR_KMER_BY_POSITION) != 0;
    if (!ix->ix.s) return kmer_nothing(pl, by_position ? d_occ : nullptr, ix->ix.n * (uint64_t)ix->sa_width);
    if ((rc = kmer_prepare(ctx, ix, d_lcp, seq_starts, num_sequences, "kmers", q))) return rc;
    return by_width(ix, [&](auto w) { return kmers_run<decltype(w)>(ctx, ix, d_lcp, q, k, by_position, bins, d_hist, d_occ, stats_out); });
}

int sufr_hip_unique_lengths_device(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_lcp, const uint64_t* seq_starts,
                                   uint64_t num_sequences, uint32_t flags, void* d_out)
{
    if (!ctx || !ix) return SUFR_HIP_E_INVALID;
    sufr::Pipeline& pl = ctx->pl;
    int rc;
    if ((rc = lcp_refusals(ctx, ix, "unique lengths", "unique_lengths"))) return rc;
    sufr::KmerSeqs q;
    const bool by_position = (flags & SUFR_KMER_BY_POSITION) != 0;
    if (!ix->ix.s) return kmer_nothing(pl, by_position ? d_out : nullptr, ix->ix.n * (uint64_t)ix->sa_width);
    if ((rc = kmer_prepare(ctx, ix, d_lcp, seq_starts, num_sequences, "unique_lengths", q))) return rc;
    if (!d_out) { pl.set_error("unique_lengths: no output"); return SUFR_HIP_E_INVALID; }
    const uint64_t s = ix->ix.s, wgs = batch_grid(pl), need = (s + 255) / 256;
    const uint32_t grid = (uint32_t)(need < wgs ? need : wgs);
    if (by_position && hipMemsetAsync(d_out, 0, q.n * (uint64_t)ix->sa_width, pl.stream) != hipSuccess) { pl.set_error("unique_lengths: memset failed"); return SUFR_HIP_E_HIP; }
    by_width(ix, [&](auto w) {
        using T = decltype(w);
        hipLaunchKernelGGL(sufr::k_unique_len<T>, dim3(grid), dim3(256), 0, pl.stream, index_sa<T>(ix), (const T*)d_lcp, s, q, (uint32_t)by_position,
                           (T*)d_out);
        return 0;
    });
    return launch_status(pl, "unique_lengths");
}

}  // extern "C"
