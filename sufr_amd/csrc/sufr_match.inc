// sufr_match.inc -- matching statistics and SMEMs of a query batch on a device-resident index (included by sufr_kernels.hip
// after sufr_search.inc; include/sufr_match.h, DESIGN.md section 13).
//
// k_matching_stats   one lane per query byte: the lower bound of the query's remainder Q[j..m) under search_compare (the
//                    loop of k_search_batch), then ms[j] = the longer common prefix with the suffixes at ranks lo - 1 and lo.
//                    The lane -> query map is a binary search of the offsets (grid-stride loop: the grid does not depend on
//                    the batch, so the launch needs nothing from the device).
// k_smem_count       SMEM flags (ms[j] >= k and (j == 0 or ms[j-1] <= ms[j])) counted per workgroup, with the summed lengths
// k_locate_scan      (sufr_search.inc) exclusive scan of both per-workgroup sums; one synchronisation reads the totals
// k_smem_emit        the flags again, scanned inside the workgroup: records in (query, offset) order + packed slice offsets
// k_smem_gather      the SMEM slices packed into one query batch, searched by the unchanged sufr_hip_search_batch_device
// No MFMA, no LDS beyond the scan words, no scratch.

namespace sufr {

static constexpr uint32_t SMEM_WGS = 1024;      // workgroups of k_smem_count / k_smem_emit (fixed: blocksums of k_locate_scan)

// the query that holds byte g of the batch: the last a < nq with off[a] <= g (off[0] <= g < off[nq])
__device__ __forceinline__ uint64_t match_query_of(const uint64_t* __restrict__ off, uint64_t nq, uint64_t g)
{
    uint64_t a = 0, b = nq;
    while (b - a > 1) { const uint64_t m = a + (b - a) / 2; if (off[m] <= g) a = m; else b = m; }
    return a;
}

// ms of Q[0..qlen) (qlen >= 1).  Prefix table: an entry narrows the search to the suffixes that share the first pk symbols;
// a missing entry only says ms < pk, so the whole array is searched.  l / r seeded with pk are lower bounds inside the table
// range, not LCPs with probed neighbours: ms is taken from explicit comparisons with ranks lo - 1 and lo.
__device__ __forceinline__ uint32_t match_stat(const SearchIndex& ix, const uint8_t* __restrict__ q, uint32_t qlen, uint64_t mql)
{
    uint64_t lo = 0, hi = ix.s;
    uint32_t l = 0, r = 0;
    if (ix.ptab && qlen >= ix.pk && (mql == 0 || mql >= ix.pk)) {
        uint64_t code = 0;
        bool ok = true;
        for (uint32_t k = 0; k < ix.pk; k++) {
            const uint32_t c = ix.pcode[q[k]];
            ok = ok && c != 0xFFu;
            code = code * ix.pradix + (c & 0x7Fu);
        }
        if (ok) {
            const uint2 e = ix.ptab[code];
            if (e.x != 0xFFFFFFFFu) { lo = e.x; hi = ~e.y; l = r = ix.pk; }
        }
    }
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        const SearchCmp c = search_compare(ix, q, qlen, mql, ix.suffix(mid), l < r ? l : r);
        if (c.cmp > 0) { lo = mid + 1; l = c.lcp; }
        else { hi = mid; r = c.lcp; }
    }
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
        const uint64_t a = match_query_of(qoff, nq, g);
        ms[g] = match_stat(ix, queries + g, (uint32_t)(qoff[a + 1] - g), mql);
    }
}

// exclusive workgroup scan of two per-lane values (256 lanes); tx / ty: the workgroup totals
__device__ __forceinline__ void match_wg_scan2(uint64_t& x, uint64_t& y, uint64_t& tx, uint64_t& ty, uint64_t* s_w)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint64_t ix = x, iy = y;
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t vx = __shfl_up(ix, o), vy = __shfl_up(iy, o);
        if (lane >= (uint32_t)o) { ix += vx; iy += vy; }
    }
    if (lane == 63) { s_w[w] = ix; s_w[4 + w] = iy; }
    __syncthreads();
    uint64_t bx = 0, by = 0;
    tx = 0; ty = 0;
    for (uint32_t k = 0; k < 4; k++) {
        if (k < w) { bx += s_w[k]; by += s_w[4 + k]; }
        tx += s_w[k]; ty += s_w[4 + k];
    }
    __syncthreads();                                   // (s_w is reused by the next tile)
    x = bx + ix - x; y = by + iy - y;
}

// workgroup b owns bytes [g0 + b * chunk, g0 + (b + 1) * chunk), in tiles of LOC_BLK (8 consecutive bytes per lane)
__device__ __forceinline__ uint64_t match_chunk(uint64_t g0, uint64_t g_end)
{
    const uint64_t c = (g_end - g0 + SMEM_WGS - 1) / SMEM_WGS;
    return (c + LOC_BLK - 1) / LOC_BLK * LOC_BLK;
}

// flags (bit k: byte g + k starts an SMEM), count and summed lengths of the 8 bytes of a lane
__device__ __forceinline__ void match_flags8(const uint32_t* __restrict__ ms, const uint64_t* __restrict__ qoff, uint64_t nq,
                                             uint64_t g, uint64_t g_hi, uint32_t min_len, uint32_t& fl, uint64_t& cnt, uint64_t& lsum)
{
    fl = 0; cnt = 0; lsum = 0;
    if (g >= g_hi) return;
    uint64_t a = match_query_of(qoff, nq, g);
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
    const uint64_t g0 = qoff[0], g_end = qoff[nq], chunk = match_chunk(g0, g_end);
    const uint64_t lo = g0 + (uint64_t)blockIdx.x * chunk, hi = lo + chunk < g_end ? lo + chunk : g_end;
    uint64_t c_acc = 0, l_acc = 0;
    for (uint64_t t = lo; t < hi; t += LOC_BLK) {
        uint64_t c, l, tc, tl;
        uint32_t fl;
        match_flags8(ms, qoff, nq, t + (uint64_t)threadIdx.x * 8, hi, min_len, fl, c, l);
        match_wg_scan2(c, l, tc, tl, s_w);
        c_acc += tc; l_acc += tl;
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
    const uint64_t g0 = qoff[0], g_end = qoff[nq], chunk = match_chunk(g0, g_end);
    const uint64_t lo = g0 + (uint64_t)blockIdx.x * chunk, hi = lo + chunk < g_end ? lo + chunk : g_end;
    uint64_t c_run = cnt_base[blockIdx.x], l_run = len_base[blockIdx.x];
    for (uint64_t t = lo; t < hi; t += LOC_BLK) {
        const uint64_t g = t + (uint64_t)threadIdx.x * 8;
        uint64_t c, l, tc, tl;
        uint32_t fl;
        match_flags8(ms, qoff, nq, g, hi, min_len, fl, c, l);
        match_wg_scan2(c, l, tc, tl, s_w);
        uint64_t at = c_run + c, bytes = l_run + l;
        uint64_t a = fl ? match_query_of(qoff, nq, g) : 0;
        for (uint32_t k = 0; fl; k++, fl >>= 1) {
            if (!(fl & 1u)) continue;
            while (qoff[a + 1] <= g + k) a++;
            const uint32_t v = ms[g + k];
            out_query[at] = a; out_qoff[at] = (uint32_t)(g + k - qoff[a]); out_len[at] = v; slice_off[at] = bytes;
            at++; bytes += v;
        }
        c_run += tc; l_run += tl;
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

int match_check(sufr_hip_ctx* ctx, const sufr_hip_index* ix)
{
    if (ix->device != ctx->pl.device) { ctx->pl.set_error("the index lives on another device"); return SUFR_HIP_E_INVALID; }
    if (ix->ix.maskpos) { ctx->pl.set_error("matching statistics of a seed-mask index are not supported"); return SUFR_HIP_E_UNSUPPORTED; }
    if (hipSetDevice(ctx->pl.device) != hipSuccess) { ctx->pl.set_error("hipSetDevice failed"); return SUFR_HIP_E_HIP; }
    return 0;
}

}  // namespace

extern "C" {

int sufr_hip_matching_stats_device(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_queries, const void* d_offsets,
                                   uint64_t num_queries, void* d_ms)
{
    if (!ctx || !ix || (num_queries && (!d_queries || !d_offsets || !d_ms))) return SUFR_HIP_E_INVALID;
    ctx->pl.err.clear();
    if (const int rc = match_check(ctx, ix)) return rc;
    if (!num_queries) return 0;
    // latency-bound lanes: 8 workgroups of 4 waves per CU, looping over the batch
    const uint32_t grid = (ctx->pl.num_cus ? ctx->pl.num_cus : 256u) * 8u;
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
    if (const int rc = match_check(ctx, ix)) return rc;
    if (min_len == 0) { pl.set_error("smems: min_len must be at least 1"); return SUFR_HIP_E_INVALID; }
    if (!num_queries) return 0;
    int rc;
    if ((rc = sufr_hip_matching_stats_device(ctx, ix, d_queries, d_offsets, num_queries, d_ms))) return rc;
    // blocksums of the counts and of the lengths, then their two totals
    const uint64_t G = sufr::SMEM_WGS;
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
    if (hipMemcpyAsync(totals, tot, 16, hipMemcpyDeviceToHost, pl.stream) != hipSuccess || hipStreamSynchronize(pl.stream) != hipSuccess) {
        pl.set_error("smems: counting the SMEMs failed");
        return SUFR_HIP_E_HIP;
    }
    const uint64_t nsm = totals[0], nbytes = totals[1];
    if (total_out) *total_out = nsm;
    if (nsm > cap) {
        pl.set_error("smems: " + std::to_string(nsm) + " SMEMs, room for " + std::to_string(cap));
        return SUFR_HIP_E_CAPACITY;
    }
    if (!nsm) return 0;
    if (!d_query || !d_query_offset || !d_length || !d_rank_lo || !d_rank_hi) return SUFR_HIP_E_INVALID;
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
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { pl.set_error(std::string("smems: ") + hipGetErrorString(e)); return SUFR_HIP_E_HIP; }
    // the rank range of every SMEM: the unchanged batched search of the packed slices (the build's cap applies as in count)
    return sufr_hip_search_batch_device(ctx, ix, ctx->mbytes.p, slice_off, nsm, 0, 0, d_rank_lo, d_rank_hi);
}

int sufr_hip_smems(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const uint8_t* queries, const uint64_t* offsets,
                   uint64_t num_queries, uint32_t min_len, uint64_t cap, uint64_t* query, uint32_t* query_offset,
                   uint32_t* length, uint64_t* rank_lo, uint64_t* rank_hi, uint64_t* total_out)
{
    if (total_out) *total_out = 0;
    if (!ctx || !ix || (num_queries && !offsets)) return SUFR_HIP_E_INVALID;
    ctx->pl.err.clear();
    if (const int rc = match_check(ctx, ix)) return rc;
    if (min_len == 0) { ctx->pl.set_error("smems: min_len must be at least 1"); return SUFR_HIP_E_INVALID; }
    if (!num_queries) return 0;
    const uint64_t qbytes = offsets[num_queries], obytes = (num_queries + 1) * 8;
    // one allocation: queries | offsets | ms | records (cap of each)
    const uint64_t o_at = (qbytes + 7) / 8 * 8, ms_at = o_at + obytes, q_at = ms_at + (qbytes * 4 + 7) / 8 * 8;
    const uint64_t qo_at = q_at + cap * 8, len_at = qo_at + cap * 4, lo_at = len_at + cap * 4, hi_at = lo_at + cap * 8;
    uint8_t* d = nullptr;
    if (hipMalloc((void**)&d, hi_at + cap * 8 + 8) != hipSuccess) { ctx->pl.set_error("hipMalloc of the SMEM batch failed"); return SUFR_HIP_E_NOMEM; }
    hipStream_t st = ctx->pl.stream;
    int rc = 0;
    if ((qbytes && hipMemcpyAsync(d, queries, qbytes, hipMemcpyHostToDevice, st) != hipSuccess) ||
        hipMemcpyAsync(d + o_at, offsets, obytes, hipMemcpyHostToDevice, st) != hipSuccess) rc = SUFR_HIP_E_HIP;
    uint64_t total = 0;
    if (!rc) rc = sufr_hip_smems_device(ctx, ix, d, d + o_at, num_queries, min_len, d + ms_at, cap, d + q_at, d + qo_at, d + len_at,
                                        d + lo_at, d + hi_at, &total);
    if (total_out) *total_out = total;
    if (!rc && total && (hipMemcpyAsync(query, d + q_at, total * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
                         hipMemcpyAsync(query_offset, d + qo_at, total * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                         hipMemcpyAsync(length, d + len_at, total * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                         hipMemcpyAsync(rank_lo, d + lo_at, total * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
                         hipMemcpyAsync(rank_hi, d + hi_at, total * 8, hipMemcpyDeviceToHost, st) != hipSuccess)) rc = SUFR_HIP_E_HIP;
    if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = SUFR_HIP_E_HIP;
    if (rc == SUFR_HIP_E_HIP && ctx->pl.err.empty()) ctx->pl.set_error("copying the SMEM batch failed");
    (void)hipFree(d);
    return rc;
}

}  // extern "C"
