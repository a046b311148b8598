// sufr_match.inc -- matching statistics and SMEMs of a query batch on a device-resident index (included by sufr_kernels.hip
// after sufr_search.inc; include/sufr_match.h, DESIGN.md section 13).
//
// k_matching_stats   one lane per query byte: the lower bound of the query's remainder Q[j..m) (search_seed + search_lower of
//                    sufr_search.inc), then ms[j] = the longer common prefix with the suffixes at ranks lo - 1 and lo.
//                    The lane -> query map is a binary search of the offsets (last_le; grid-stride loop: the grid does not
//                    depend on the batch, so the launch needs nothing from the device).
// k_smem_count       SMEM flags (ms[j] >= k and (j == 0 or ms[j-1] <= ms[j])) counted per workgroup, with the summed lengths
// k_locate_scan      (sufr_search.inc) exclusive scan of both per-workgroup sums; one synchronisation reads the totals
// k_smem_emit        the flags again, scanned inside the workgroup: records in (query, offset) order + packed slice offsets
// k_smem_gather      the SMEM slices packed into one query batch, searched by the unchanged sufr_hip_search_batch_device
// No MFMA, no LDS beyond the scan words, no scratch.
// Its own: match_stat, the SMEM rule (match_flags8), the three SMEM kernels and smems_from_stats, the SMEMs of statistics that
// are there, which sufr_fm.inc calls too (include/sufr_fm_match.h).  The search, last_le, wg_scan, scan_chunk
// (SCAN_WGS workgroups), query_check, read_totals, the record epilogue and staged_records are sufr_search.inc's.

namespace sufr {

// ms of Q[0..qlen) (qlen >= 1).  Prefix table: an entry narrows the search to the suffixes that share the first pk symbols;
// a missing entry (s.none) only says ms < pk, so the whole array is searched, which is what the seed then holds.  The l / r
// that search_lower seeds with pk are lower bounds inside the table range, not LCPs with probed neighbours: ms is taken
// from explicit comparisons with ranks lo - 1 and lo.
__device__ __forceinline__ uint32_t match_stat(const SearchIndex& ix, const uint8_t* __restrict__ q, uint32_t qlen, uint64_t mql)
{
    const SearchSeed s = search_seed(ix, q, qlen, mql);
    const uint64_t lo = search_lower(ix, q, qlen, mql, s.lo, s.hi, s.shared).first;
    uint32_t best = 0;
    if (lo > 0) best = search_compare(ix, q, qlen, mql, ix.suffix(lo - 1), 0).lcp;
    if (lo < ix.s) { const uint32_t v = search_compare(ix, q, qlen, mql, ix.suffix(lo), 0).lcp; best = v > best ? v : best; }
    return best;
}

__global__ __launch_bounds__(256) void k_matching_stats(SearchIndex ix, const uint8_t* __restrict__ queries,
                                                        const uint64_t* __restrict__ qoff, uint64_t nq, uint64_t mql,
                                                        uint32_t* __restrict__ ms)
{
    const uint64_t g_end = qoff[nq], stride = (uint64_t)gridDim.x * 256;
    for (uint64_t g = qoff[0] + (uint64_t)blockIdx.x * 256 + threadIdx.x; g < g_end; g += stride) {
        const uint64_t a = last_le(qoff, 0, nq, g);
        ms[g] = match_stat(ix, queries + g, (uint32_t)(qoff[a + 1] - g), mql);
    }
}

// flags (bit k: byte g + k starts an SMEM), count and summed lengths of the 8 bytes of a lane
__device__ __forceinline__ void match_flags8(const uint32_t* __restrict__ ms, const uint64_t* __restrict__ qoff, uint64_t nq,
                                             uint64_t g, uint64_t g_hi, uint32_t min_len, uint32_t& fl, uint64_t& cnt, uint64_t& lsum)
{
    fl = 0; cnt = 0; lsum = 0;
    if (g >= g_hi) return;
    uint64_t a = last_le(qoff, 0, nq, g);
    for (uint32_t k = 0; k < 8 && g + k < g_hi; k++) {
        while (qoff[a + 1] <= g + k) a++;
        const uint32_t v = ms[g + k];
        if (v >= min_len && (g + k == qoff[a] || ms[g + k - 1] <= v)) { fl |= 1u << k; cnt++; lsum += v; }
    }
}

__global__ __launch_bounds__(256) void k_smem_count(const uint32_t* __restrict__ ms, const uint64_t* __restrict__ qoff, uint64_t nq,
                                                    uint32_t min_len, uint64_t* __restrict__ cnt_sum, uint64_t* __restrict__ len_sum)
{
    __shared__ uint64_t s_w[8];
    const uint64_t g0 = qoff[0], g_end = qoff[nq], chunk = scan_chunk(g_end - g0);
    const uint64_t lo = g0 + (uint64_t)blockIdx.x * chunk, hi = lo + chunk < g_end ? lo + chunk : g_end;
    uint64_t c_acc = 0, l_acc = 0;
    for (uint64_t t = lo; t < hi; t += LOC_BLK) {
        uint64_t v[2], tot[2];                         // count, summed lengths
        uint32_t fl;
        match_flags8(ms, qoff, nq, t + (uint64_t)threadIdx.x * 8, hi, min_len, fl, v[0], v[1]);
        wg_scan(v, tot, s_w);
        c_acc += tot[0]; l_acc += tot[1];
    }
    if (threadIdx.x == 0) { cnt_sum[blockIdx.x] = c_acc; len_sum[blockIdx.x] = l_acc; }
}

__global__ __launch_bounds__(256) void k_smem_emit(const uint32_t* __restrict__ ms, const uint64_t* __restrict__ qoff, uint64_t nq,
                                                   uint32_t min_len, const uint64_t* __restrict__ cnt_base,
                                                   const uint64_t* __restrict__ len_base, uint64_t* __restrict__ out_query,
                                                   uint32_t* __restrict__ out_qoff, uint32_t* __restrict__ out_len,
                                                   uint64_t* __restrict__ slice_off)
{
    __shared__ uint64_t s_w[8];
    const uint64_t g0 = qoff[0], g_end = qoff[nq], chunk = scan_chunk(g_end - g0);
    const uint64_t lo = g0 + (uint64_t)blockIdx.x * chunk, hi = lo + chunk < g_end ? lo + chunk : g_end;
    uint64_t c_run = cnt_base[blockIdx.x], l_run = len_base[blockIdx.x];
    for (uint64_t t = lo; t < hi; t += LOC_BLK) {
        const uint64_t g = t + (uint64_t)threadIdx.x * 8;
        uint64_t v[2], tot[2];                         // count, summed lengths
        uint32_t fl;
        match_flags8(ms, qoff, nq, g, hi, min_len, fl, v[0], v[1]);
        wg_scan(v, tot, s_w);
        uint64_t at = c_run + v[0], bytes = l_run + v[1];
        uint64_t a = fl ? last_le(qoff, 0, nq, g) : 0;
        for (uint32_t k = 0; fl; k++, fl >>= 1) {
            if (!(fl & 1u)) continue;
            while (qoff[a + 1] <= g + k) a++;
            const uint32_t len = ms[g + k];
            out_query[at] = a; out_qoff[at] = (uint32_t)(g + k - qoff[a]); out_len[at] = len; slice_off[at] = bytes;
            at++; bytes += len;
        }
        c_run += tot[0]; l_run += tot[1];
    }
}

// one wavefront per SMEM (grid-stride): its slice of the query bytes, packed at slice_off
__global__ __launch_bounds__(256) void k_smem_gather(const uint8_t* __restrict__ queries, const uint64_t* __restrict__ qoff,
                                                     const uint64_t* __restrict__ sq, const uint32_t* __restrict__ sqoff,
                                                     const uint32_t* __restrict__ slen, uint64_t* __restrict__ slice_off,
                                                     uint64_t nsm, uint64_t nbytes, uint8_t* __restrict__ packed)
{
    const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (uint64_t)gridDim.x * 4;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t t = wave; t < nsm; t += nwaves) {
        const uint8_t* src = queries + qoff[sq[t]] + sqoff[t];
        uint8_t* dst = packed + slice_off[t];
        for (uint32_t k = lane; k < slen[t]; k += 64) dst[k] = src[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) slice_off[nsm] = nbytes;
}

}  // namespace sufr

namespace {

// The SMEMs of a batch whose statistics are in d_ms: flags, the one synchronisation for the totals, records and the packed
// slices; search(packed, slice_off, nsm) then enqueues the rank range of every slice
template <typename Search>
int smems_from_stats(sufr_hip_ctx* ctx, const void* d_queries, const void* d_offsets, uint64_t num_queries, uint32_t min_len, const void* d_ms,
                     uint64_t cap, void* d_query, void* d_query_offset, void* d_length, void* d_rank_lo, void* d_rank_hi, uint64_t* total_out,
                     Search search)
{
    sufr::Pipeline& pl = ctx->pl;
    int rc;
    // blocksums of the counts and of the lengths, then their two totals
    const uint64_t G = sufr::SCAN_WGS;
    if ((rc = pl.ensure(ctx->mtmp, (2 * G + 2) * 8))) return rc;
    uint64_t* cnt_sum = (uint64_t*)ctx->mtmp.p;
    uint64_t* len_sum = cnt_sum + G;
    uint64_t* tot = len_sum + G;
    const uint64_t* off = (const uint64_t*)d_offsets;
    const uint32_t* ms = (const uint32_t*)d_ms;
    hipLaunchKernelGGL(sufr::k_smem_count, dim3((uint32_t)G), dim3(256), 0, pl.stream, ms, off, num_queries, min_len, cnt_sum, len_sum);
    hipLaunchKernelGGL(sufr::k_locate_scan, dim3(1), dim3(1024), 0, pl.stream, cnt_sum, G, tot);
    hipLaunchKernelGGL(sufr::k_locate_scan, dim3(1), dim3(1024), 0, pl.stream, len_sum, G, tot + 1);
    unsigned long long totals[2] = {0, 0};
    if ((rc = read_totals(pl, tot, 2, totals, "smems", "counting the SMEMs failed"))) return rc;
    const uint64_t nsm = totals[0], nbytes = totals[1];
    if ((rc = records_fit(pl, "smems", "SMEMs", nsm, cap, total_out)) || !nsm) return rc;
    if (any_null({d_query, d_query_offset, d_length, d_rank_lo, d_rank_hi})) return SUFR_HIP_E_INVALID;
    if ((rc = pl.ensure(ctx->mpoff, (nsm + 1) * 8)) || (rc = pl.ensure(ctx->mbytes, nbytes))) return rc;
    uint64_t* slice_off = (uint64_t*)ctx->mpoff.p;
    hipLaunchKernelGGL(sufr::k_smem_emit, dim3((uint32_t)G), dim3(256), 0, pl.stream, ms, off, num_queries, min_len,
                       (const uint64_t*)cnt_sum, (const uint64_t*)len_sum, (uint64_t*)d_query, (uint32_t*)d_query_offset,
                       (uint32_t*)d_length, slice_off);
    uint64_t gw = (nsm + 3) / 4;
    if (gw > 16384) gw = 16384;
    hipLaunchKernelGGL(sufr::k_smem_gather, dim3((uint32_t)gw), dim3(256), 0, pl.stream, (const uint8_t*)d_queries, off,
                       (const uint64_t*)d_query, (const uint32_t*)d_query_offset, (const uint32_t*)d_length, slice_off, nsm, nbytes,
                       (uint8_t*)ctx->mbytes.p);
    if ((rc = launch_status(pl, "smems"))) return rc;
    return search(ctx->mbytes.p, slice_off, nsm);
}

}  // namespace

extern "C" {

int sufr_hip_matching_stats_device(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_queries, const void* d_offsets,
                                   uint64_t num_queries, void* d_ms)
{
    if (!ctx || !ix || (num_queries && (!d_queries || !d_offsets || !d_ms))) return SUFR_HIP_E_INVALID;
    ctx->pl.err.clear();
    if (const int rc = query_check(ctx, ix, "matching statistics")) return rc;
    if (!num_queries) return 0;
    // latency-bound lanes: 8 workgroups of 4 waves per CU, looping over the batch
    const uint32_t grid = batch_grid(ctx->pl);
    hipLaunchKernelGGL(sufr::k_matching_stats, dim3(grid), dim3(256), 0, ctx->pl.stream, ix->ix, (const uint8_t*)d_queries,
                       (const uint64_t*)d_offsets, num_queries, effective_mql(ix, 0, 0), (uint32_t*)d_ms);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { ctx->pl.set_error(std::string("k_matching_stats: ") + hipGetErrorString(e)); return SUFR_HIP_E_HIP; }
    return 0;
}

int sufr_hip_smems_device(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_queries, const void* d_offsets,
                          uint64_t num_queries, uint32_t min_len, void* d_ms, uint64_t cap, void* d_query, void* d_query_offset,
                          void* d_length, void* d_rank_lo, void* d_rank_hi, uint64_t* total_out)
{
    if (total_out) *total_out = 0;
    if (!ctx || !ix || (num_queries && (!d_queries || !d_offsets || !d_ms))) return SUFR_HIP_E_INVALID;
    sufr::Pipeline& pl = ctx->pl;
    pl.err.clear();
    if (const int rc = query_check(ctx, ix, "matching statistics")) return rc;
    if (min_len == 0) { pl.set_error("smems: min_len must be at least 1"); return SUFR_HIP_E_INVALID; }
    if (!num_queries) return 0;
    int rc;
    if ((rc = sufr_hip_matching_stats_device(ctx, ix, d_queries, d_offsets, num_queries, d_ms))) return rc;
    // the rank range of every SMEM: the unchanged batched search of the packed slices (the build's cap applies as in count)
    return smems_from_stats(ctx, d_queries, d_offsets, num_queries, min_len, d_ms, cap, d_query, d_query_offset, d_length, d_rank_lo, d_rank_hi, total_out,
                            [&](const void* packed, const uint64_t* slice_off, uint64_t nsm) {
        return sufr_hip_search_batch_device(ctx, ix, packed, slice_off, nsm, 0, 0, d_rank_lo, d_rank_hi);
    });
}

int sufr_hip_smems(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const uint8_t* queries, const uint64_t* offsets,
                   uint64_t num_queries, uint32_t min_len, uint64_t cap, uint64_t* query, uint32_t* query_offset,
                   uint32_t* length, uint64_t* rank_lo, uint64_t* rank_hi, uint64_t* total_out)
{
    if (total_out) *total_out = 0;
    if (!ctx || !ix || (num_queries && !offsets)) return SUFR_HIP_E_INVALID;
    ctx->pl.err.clear();
    if (const int rc = query_check(ctx, ix, "matching statistics")) return rc;
    if (min_len == 0) { ctx->pl.set_error("smems: min_len must be at least 1"); return SUFR_HIP_E_INVALID; }
    if (!num_queries) return 0;
    // the matching statistics (4 bytes per query byte) stay on the device: they ride behind the record columns
    return staged_records(ctx, "SMEM", queries, offsets, num_queries, cap, {{query, 8}, {query_offset, 4}, {length, 4}, {rank_lo, 8}, {rank_hi, 8}},
                          offsets[num_queries] * 4, total_out, [&](const void* d_q, const void* d_off, void* const* col, uint64_t* total) {
        return sufr_hip_smems_device(ctx, ix, d_q, d_off, num_queries, min_len, col[5], cap, col[0], col[1], col[2], col[3], col[4], total);
    });
}

}  // extern "C"
