// sufr_shared.inc -- the number of different sequences behind every repeat, and the k-common substrings, from the SA, the
// LCP and the sequence starts of a device-resident index (included by sufr_kernels.hip after sufr_lz.inc;
// include/sufr_shared.h, DESIGN.md section 21).
//
// "Distinct sequences among the ranks [a, b)" is (b - a) minus the ranks that are not the first of their sequence there,
// and those are the H mass strictly inside the interval (the identity of sufr_shared.h): a difference of two prefix sums
// per interval, whatever b - a is.  The intervals, the clipped LCP l, its min pyramid and the flag words are those of
// sufr_repeat.inc, built by the same kernels (repeats_prepare); the arithmetic of this file -- the sequence of a position,
// the decision of one pair, the count -- is sufr_shared_scan.h, which the host path and tests/shared_shim.cpp compile too.
//
// k_shr_keys     a lane per rank: the binary search of the sequence starts, one 64-bit key doc << 40 | r.
// sort_keys      (sufr_edit.inc) over the bits [40, 40 + bits(num - 1)): the keys arrive in rank order and the sort is stable,
//                so the ranks of every sequence come out ascending.  One sequence: no pass.
// k_shr_pairs    a lane per sorted key j: if key j - 1 has the same sequence the pair is (prev, r); q = shr_pair (one range
//                minimum, one search, each bounded by 2 x 64 x levels reads) and H[q] += 1 by a global atomic add -- integer
//                adds commute, the result depends on no order; the one atomic add of this file.  Per 256 keys the l of up to
//                REP_STAGE ranks from the first pair's prev on is staged in LDS (RepStaged::stage) when the keys of the step
//                are near enough for that to serve them (one sequence: always; many sequences: the ranks of one sequence lie
//                far apart and nothing is staged); a pair whose range leaves the window reads the pyramid in memory.  The
//                window is a copy: it changes no result.
// k_shr_scan     the exclusive prefix of H inside every tile, in place, and the tile totals; k_locate_scan (sufr_search.inc)
//                turns the totals into bases; k_shr_addbase adds them: P, s + 1 entries of the index width.
// k_rep_find     (sufr_repeat.inc) with SEQS set: the find pass of repeats with seqs from two reads of P, its filter and its
//                column; counting, writing, or the profile (every representative raises best[seqs - 1] to v).  The counted
//                find is repeats_find<T, true>; k_tile_best over RepBestOp<5> gives its stats.
// k_shr_suffix   one workgroup: the suffix maximum of best into d_common, a backward tile_sweep (sufr_scan.inc, DESIGN.md
//                section 10.2) of MaxOp.
// A workgroup takes tiles t = blockIdx.x, blockIdx.x + gridDim.x, ...; no scratch, no MFMA.  LDS: k_shr_pairs 16.6 KB (32-bit
// arrays) or 33.2 KB (64-bit), k_shr_suffix 128 bytes, k_shr_scan 32 bytes.

#include "sufr_shared_scan.h"

namespace sufr {

__device__ __forceinline__ void shr_add_one(uint32_t* p) { atomicAdd(p, 1u); }
__device__ __forceinline__ void shr_add_one(uint64_t* p) { atomicAdd((unsigned long long*)p, 1ull); }

template <typename T>
__global__ __launch_bounds__(256) void k_shr_keys(const T* __restrict__ sa, uint64_t s, KmerSeqs q, uint64_t* __restrict__ keys)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < s; r += stride) keys[r] = shr_key(shr_doc(q.starts, q.num, (uint64_t)sa[r]), r);
}

// H[q(r)] += 1 for every pair (prev[r], r); keys: the s keys sorted by sequence, H zeroed
template <typename T>
__global__ __launch_bounds__(256) void k_shr_pairs(RepAcc<T> gacc, const uint64_t* __restrict__ keys, uint32_t tile, uint64_t ntiles, T* __restrict__ H)
{
    __shared__ T s_l[REP_STAGE], s_l1[REP_STAGE / 64];
    RepStaged<T> acc{gacc, s_l, s_l1, 0, 0, 0, 0};
    const uint64_t s = gacc.s;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        for (uint32_t it = 0; it < tile; it += 256) {
            const uint64_t j0 = t * tile + it, j = j0 + threadIdx.x;
            if (j0 >= s) break;                          // (uniform: past the end of the array)
            {                                            // (uniform) the window of these 256 keys
                const uint64_t jl = j0 + 255 < s ? j0 + 255 : s - 1, k0 = keys[j0], kl = keys[jl];
                uint64_t lo = shr_key_rank(k0);
                if (j0) { const uint64_t kp = keys[j0 - 1]; if (shr_key_doc(kp) == shr_key_doc(k0)) lo = shr_key_rank(kp); }
                const uint64_t w0 = lo & ~(uint64_t)63;
                // one sequence from the first key to the last: the ranks ascend and the last one bounds what is read;
                // staging pays while that is a few windows at most
                const uint64_t span = shr_key_doc(kl) == shr_key_doc(k0) ? shr_key_rank(kl) + 1 - w0 : REP_STAGE;
                uint64_t len = span > 4 * (uint64_t)REP_STAGE ? 0 : span < REP_STAGE ? span : REP_STAGE;
                if (len > s - w0) len = s - w0;
                __syncthreads();                         // (the lanes are done with the window before)
                acc.stage(rep_window(w0, len, s));
                __syncthreads();
            }
            if (j >= 1 && j < s) {
                const uint64_t key = keys[j], pk = keys[j - 1];
                if (shr_key_doc(pk) == shr_key_doc(key)) shr_add_one(&H[shr_pair(acc, s, shr_key_rank(pk), shr_key_rank(key))]);
            }
        }
    }
}

// x[0..n): the exclusive prefix inside every tile, in place; t_sum[t]: the tile's total
template <typename T>
__global__ __launch_bounds__(256) void k_shr_scan(T* __restrict__ x, uint64_t n, uint32_t tile, uint64_t ntiles, uint64_t* __restrict__ t_sum)
{
    __shared__ uint64_t s_w[4];
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        uint64_t run = 0;
        for (uint32_t it = 0; it < tile; it += 256) {
            const uint64_t i = t * tile + it + threadIdx.x;
            if (i - threadIdx.x >= n) break;             // (uniform)
            uint64_t v[1] = {i < n ? (uint64_t)x[i] : 0}, tot[1];
            wg_scan(v, tot, s_w);
            if (i < n) x[i] = (T)(run + v[0]);
            run += tot[0];
        }
        if (threadIdx.x == 0) t_sum[t] = run;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_shr_addbase(T* __restrict__ x, uint64_t n, uint32_t tile, const uint64_t* __restrict__ t_base)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) x[i] = (T)((uint64_t)x[i] + t_base[i / tile]);
}

// common[k] = max best[k ..)
__global__ __launch_bounds__(1024) void k_shr_suffix(const uint64_t* __restrict__ best, uint64_t num, uint64_t* __restrict__ common)
{
    __shared__ uint64_t s_m[16];
    tile_sweep<MaxOp, true>(
        num, [&](uint64_t k) { return best[k]; }, [&](uint64_t k, uint64_t own, uint64_t after) { common[k] = own > after ? own : after; }, s_m);
}

}  // namespace sufr

namespace {

template <typename T>
struct ShrPrep {
    const T* P;                                          // the exclusive prefix of H, s + 1 entries
    uint64_t* best;                                      // the profile's maxima, num entries
#ifdef SUFR_HIP_PROBES
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};      // (probes build: before the sort, between the sort and the pairs, after the pairs)
    bool stamp = false;
#endif
};

// Scratch of the context, grown on demand and freed with it: shkeys, the two key buffers (16 s bytes); shhist, the digit
// counts of a radix pass (256 * SCAN_WGS + 1 words); shpre, H and then P ((s + 1) entries of the index width); shsum, the
// tile sums of the prefix and the profile's maxima (the find pass has its sums in RepPrep).
// Enqueues the passes of repeats_prepare, the keys, the sort, the pairs and the prefix.
template <typename T>
int shared_prepare(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_lcp, const sufr::KmerSeqs& q, uint64_t num, RepPrep<T>& R, ShrPrep<T>& S)
{
    sufr::Pipeline& pl = ctx->pl;
    const uint64_t s = ix->ix.s;
    int rc;
    if ((rc = repeats_prepare<T>(ctx, ix, d_lcp, q, R))) return rc;
    const uint64_t ntiles = R.ntiles, np = s + 1, nptiles = (np + R.tile - 1) / R.tile;
    if ((rc = pl.ensure(ctx->shkeys, s * 16)) || (rc = pl.ensure(ctx->shhist, ((uint64_t)256 * sufr::SCAN_WGS + 1) * 8)) ||
        (rc = pl.ensure(ctx->shpre, np * sizeof(T))) || (rc = pl.ensure(ctx->shsum, (nptiles + 1 + num) * 8))) return rc;
    uint64_t* ka = (uint64_t*)ctx->shkeys.p;
    uint64_t* kb = ka + s;
    T* H = (T*)ctx->shpre.p;
    uint64_t* t_h = (uint64_t*)ctx->shsum.p;
    S.P = H;
    S.best = t_h + nptiles + 1;
    if (hipMemsetAsync(H, 0, np * sizeof(T), pl.stream) != hipSuccess) { pl.set_error("shared: memset failed"); return SUFR_HIP_E_HIP; }
    {
        const uint64_t need = (s + 255) / 256;
        hipLaunchKernelGGL(sufr::k_shr_keys<T>, dim3((uint32_t)(need < R.wgs ? need : R.wgs)), dim3(256), 0, pl.stream, index_sa<T>(ix), s, q, ka);
    }
#ifdef SUFR_HIP_PROBES
    S.stamp = hipEventCreate(&S.ev[0]) == hipSuccess && hipEventCreate(&S.ev[1]) == hipSuccess && hipEventCreate(&S.ev[2]) == hipSuccess &&
              hipEventRecord(S.ev[0], pl.stream) == hipSuccess;
#endif
    const uint64_t* sorted = sufr::sort_keys(pl.stream, ka, kb, s, sufr::SHR_RANK_BITS, sufr::SHR_RANK_BITS + sufr::shr_doc_bits(q.num),
                                             (uint64_t*)ctx->shhist.p);
#ifdef SUFR_HIP_PROBES
    if (S.stamp) (void)hipEventRecord(S.ev[1], pl.stream);
#endif
    hipLaunchKernelGGL(sufr::k_shr_pairs<T>, dim3(R.grid), dim3(256), 0, pl.stream, R.acc, sorted, R.tile, ntiles, H);
#ifdef SUFR_HIP_PROBES
    if (S.stamp) (void)hipEventRecord(S.ev[2], pl.stream);
#endif
    const uint32_t pgrid = (uint32_t)(nptiles < R.wgs ? nptiles : R.wgs);
    hipLaunchKernelGGL(sufr::k_shr_scan<T>, dim3(pgrid), dim3(256), 0, pl.stream, H, np, R.tile, nptiles, t_h);
    hipLaunchKernelGGL(sufr::k_locate_scan, dim3(1), dim3(1024), 0, pl.stream, t_h, nptiles, t_h + nptiles);
    {
        const uint64_t need = (np + 255) / 256;
        hipLaunchKernelGGL(sufr::k_shr_addbase<T>, dim3((uint32_t)(need < R.wgs ? need : R.wgs)), dim3(256), 0, pl.stream, H, np, R.tile, (const uint64_t*)t_h);
    }
    return 0;
}

template <typename T>
int shared_run(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_lcp, const sufr::KmerSeqs& q, const sufr::RepFilter& flt, uint64_t cap,
               void* d_rank, void* d_count, void* d_length, void* d_seqs, uint64_t* total_out, sufr_shared_stats* stats_out)
{
    RepPrep<T> R;
    ShrPrep<T> S;
    if (const int rc = shared_prepare<T>(ctx, ix, d_lcp, q, 0, R, S)) return rc;
    unsigned long long h[5];
    const int rc = repeats_find<T, true>(ctx, ix, R, S.P, flt, "shared", cap, d_rank, d_count, d_length, d_seqs, total_out, h);
#ifdef SUFR_HIP_PROBES
    float ms_sort = 0, ms_pairs = 0;                      // (probes build: the sort's and the pair pass's own times, to standard error)
    if (S.stamp && hipEventElapsedTime(&ms_sort, S.ev[0], S.ev[1]) == hipSuccess && hipEventElapsedTime(&ms_pairs, S.ev[1], S.ev[2]) == hipSuccess)
        fprintf(stderr, "shared: sort %.3f ms, pairs %.3f ms (%llu ranks)\n", ms_sort, ms_pairs, (unsigned long long)ix->ix.s);
    for (hipEvent_t e : S.ev) if (e) (void)hipEventDestroy(e);
#endif
    if (stats_out) *stats_out = sufr_shared_stats{h[0], h[1], h[2], h[3], h[4]};
    return rc;
}

template <typename T>
int common_run(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_lcp, const sufr::KmerSeqs& q, uint64_t num, void* d_common)
{
    sufr::Pipeline& pl = ctx->pl;
    RepPrep<T> R;
    ShrPrep<T> S;
    int rc;
    if ((rc = shared_prepare<T>(ctx, ix, d_lcp, q, num, R, S))) return rc;
    if (hipMemsetAsync(S.best, 0, num * 8, pl.stream) != hipSuccess) { pl.set_error("common: memset failed"); return SUFR_HIP_E_HIP; }
    const sufr::RepFilter flt{SUFR_REPEAT_BRANCHING, 1, 2, 0, 0, 0};
    uint64_t* const none = nullptr;
    hipLaunchKernelGGL((sufr::k_rep_find<T, sufr::REP_PROFILE, true>), dim3(R.grid), dim3(256), 0, pl.stream, R.acc, ix->ix.text, R.bits, S.P, flt, R.tile,
                       R.ntiles, R.t_cnt, R.t_best, none, none, none, none, S.best, num);
    hipLaunchKernelGGL(sufr::k_shr_suffix, dim3(1), dim3(1024), 0, pl.stream, (const uint64_t*)S.best, num, (uint64_t*)d_common);
#ifdef SUFR_HIP_PROBES
    for (hipEvent_t e : S.ev) if (e) (void)hipEventDestroy(e);      // (only sufr_hip_shared_device prints the stamps)
#endif
    return launch_status(pl, "common");
}

// what both calls refuse whatever their other arguments are
int shared_refusals(sufr_hip_ctx* ctx, const sufr_hip_index* ix, uint64_t num_sequences, const char* what)
{
    sufr::Pipeline& pl = ctx->pl;
    if (const int rc = lcp_refusals(ctx, ix, what, what)) return rc;
    if (ix->ix.s >> sufr::SHR_RANK_BITS || num_sequences >> sufr::SHR_DOC_BITS) {
        pl.set_error(std::string(what) + ": 2^40 suffixes or 2^24 sequences, or more");
        return SUFR_HIP_E_UNSUPPORTED;
    }
    return 0;
}

}  // namespace

extern "C" {

int sufr_hip_shared_device(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_lcp, const uint64_t* seq_starts, uint64_t num_sequences,
                           uint32_t kind, uint64_t min_len, uint64_t min_count, uint64_t max_count, uint64_t min_seqs, uint64_t max_seqs,
                           uint64_t cap, void* d_rank, void* d_count, void* d_length, void* d_seqs, uint64_t* total_out,
                           sufr_shared_stats* stats_out)
{
    if (stats_out) *stats_out = sufr_shared_stats{0, 0, 0, 0, 0};
    if (total_out) *total_out = 0;
    if (!ctx || !ix) return SUFR_HIP_E_INVALID;
    sufr::Pipeline& pl = ctx->pl;
    int rc;
    if ((rc = shared_refusals(ctx, ix, num_sequences, "shared"))) return rc;
    if (min_len == 0) { pl.set_error("shared: min_len must be at least 1"); return SUFR_HIP_E_INVALID; }
    if (kind > SUFR_REPEAT_SUPERMAXIMAL) { pl.set_error("shared: unknown kind " + std::to_string(kind)); return SUFR_HIP_E_INVALID; }
    if (max_seqs && min_seqs > max_seqs) { pl.set_error("shared: min_seqs is larger than max_seqs"); return SUFR_HIP_E_INVALID; }
    if (!ix->ix.s) return 0;
    sufr::KmerSeqs q;
    if ((rc = kmer_prepare(ctx, ix, d_lcp, seq_starts, num_sequences, "shared", q))) return rc;
    const sufr::RepFilter flt{kind, min_len, min_count < 2 ? 2 : min_count, max_count, min_seqs, max_seqs};
    return by_width(ix, [&](auto w) { return shared_run<decltype(w)>(ctx, ix, d_lcp, q, flt, cap, d_rank, d_count, d_length, d_seqs, total_out, stats_out); });
}

int sufr_hip_common_device(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_lcp, const uint64_t* seq_starts, uint64_t num_sequences,
                           void* d_common)
{
    if (!ctx || !ix) return SUFR_HIP_E_INVALID;
    sufr::Pipeline& pl = ctx->pl;
    int rc;
    if ((rc = shared_refusals(ctx, ix, num_sequences, "common"))) return rc;
    sufr::KmerSeqs q;
    if ((rc = kmer_prepare(ctx, ix, d_lcp, seq_starts, num_sequences, "common", q))) return rc;
    if (!d_common) { pl.set_error("common: no output array"); return SUFR_HIP_E_INVALID; }
    const uint64_t num = num_sequences && seq_starts ? num_sequences : 1;
    if (!ix->ix.s) {
        if (hipMemsetAsync(d_common, 0, num * 8, pl.stream) != hipSuccess) { pl.set_error("common: memset failed"); return SUFR_HIP_E_HIP; }
        return 0;
    }
    return by_width(ix, [&](auto w) { return common_run<decltype(w)>(ctx, ix, d_lcp, q, num, d_common); });
}

}  // extern "C"
