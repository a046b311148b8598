// sufr_mem.inc -- maximal exact matches (MEMs) of a query batch on a device-resident index (included by sufr_kernels.hip
// after sufr_match.inc; include/sufr_mem.h, DESIGN.md section 14).
//
// k_mem_bitmap       once per index whose array leaves positions out: one lane per rank sets bit SA[r] (atomicOr on u32 words)
// k_mem_revcomp      both strands: the doubled batch, query i as it is then its reverse complement, with the new offsets
// k_mem_ranges       one lane per query offset (grid-stride): the rank range of the k'-prefix Q[j..j+k') found in place by
//                    search_range (sufr_search.inc, what k_search_batch runs); an empty range when j + k > m or the range
//                    holds more than max_occ suffixes
// k_locate_counts / k_locate_scan / k_locate_apply (sufr_search.inc) exclusive scan of the range sizes: the candidate starts;
//                    one synchronisation reads the candidate total
// k_mem_count        1024 workgroups over the candidates, 8 per lane: candidate -> offset by binary search of the starts,
//                    p = SA[lo + ...], the left condition (one query byte, one text byte, one bitmap bit); counts per workgroup
// k_locate_scan      the MEM total (second synchronisation) and the workgroup bases
// k_mem_emit         the flags again, scanned in the workgroup; every MEM is extended with 8-byte compares and written
// No MFMA, no LDS beyond the scan words, no scratch.
// From sufr_search.inc: search_range, common_prefix, last_le (offset -> query, candidate -> offset), wg_scan and scan_chunk
// (SCAN_WGS workgroups), query_check, read_totals and the staging of the host-pointer entry point.

namespace sufr {

struct MemBatch {
    const uint8_t* q;           // query bytes (the doubled batch with both strands)
    const uint64_t* qoff;       // nq + 1 offsets
    uint64_t nq;
    const uint64_t* rlo;        // per offset g - qoff[0]: first rank of its k'-prefix
    const uint64_t* cand;       // per offset: first candidate (exclusive scan of the range sizes), nb + 1 entries
    uint64_t nb;                // offsets in the batch
    const uint32_t* bits;       // indexed positions, or nullptr: every position is indexed
    uint32_t min_len, kk;       // k and k' = min(k, L)
};

__global__ __launch_bounds__(256) void k_mem_bitmap(SearchIndex ix, uint32_t* __restrict__ bits)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < ix.s; r += stride) {
        const uint64_t p = ix.suffix(r);
        atomicOr(&bits[p >> 5], 1u << (p & 31));
    }
}

__device__ __forceinline__ uint8_t mem_complement(uint8_t c)
{
    return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
}

__global__ __launch_bounds__(256) void k_mem_revcomp(const uint8_t* __restrict__ queries, const uint64_t* __restrict__ qoff, uint64_t nq,
                                                     uint8_t* __restrict__ dst, uint64_t* __restrict__ doff)
{
    const uint64_t g0 = qoff[0], g_end = qoff[nq], stride = (uint64_t)gridDim.x * 256;
    const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    for (uint64_t i = tid; i <= nq; i += stride) {
        if (i < nq) { doff[2 * i] = 2 * (qoff[i] - g0); doff[2 * i + 1] = qoff[i] + qoff[i + 1] - 2 * g0; }
        else doff[2 * nq] = 2 * (g_end - g0);
    }
    for (uint64_t g = g0 + tid; g < g_end; g += stride) {
        const uint64_t a = last_le(qoff, 0, nq, g), b = qoff[a], e = qoff[a + 1];
        const uint8_t c = queries[g];
        dst[2 * (b - g0) + (g - b)] = c;
        dst[b + e - 2 * g0 + (e - 1 - g)] = mem_complement(c);
    }
}

__global__ __launch_bounds__(256) void k_mem_ranges(SearchIndex ix, const uint8_t* __restrict__ queries, const uint64_t* __restrict__ qoff,
                                                    uint64_t nq, uint64_t mql, uint32_t min_len, uint32_t kk, uint64_t max_occ,
                                                    uint64_t* __restrict__ lo_out, uint64_t* __restrict__ hi_out)
{
    const uint64_t g0 = qoff[0], g_end = qoff[nq], stride = (uint64_t)gridDim.x * 256;
    for (uint64_t g = g0 + (uint64_t)blockIdx.x * 256 + threadIdx.x; g < g_end; g += stride) {
        const uint64_t a = last_le(qoff, 0, nq, g);
        uint64_t lo = 0, hi = 0;
        if (g + min_len <= qoff[a + 1]) {
            search_range(ix, queries + g, kk, mql, lo, hi);      // (kk <= the build's cap)
            if (max_occ && hi - lo > max_occ) hi = lo;
        }
        lo_out[g - g0] = lo; hi_out[g - g0] = hi;
    }
}

// walks the (up to) 8 candidates [c, c_hi) of a lane: f(k, g, a, p) for every one that starts a MEM (g: offset index, a: query)
template <typename F>
__device__ __forceinline__ void mem_walk8(const SearchIndex& ix, const MemBatch& B, uint64_t c, uint64_t c_hi, F f)
{
    if (c >= c_hi) return;
    const uint64_t g0 = B.qoff[0];
    uint64_t g = last_le(B.cand, 0, B.nb, c);
    uint64_t a = last_le(B.qoff, 0, B.nq, g0 + g);
    for (uint32_t k = 0; k < 8 && c + k < c_hi; k++) {
        if (B.cand[g + 1] <= c + k) {
            g = last_le(B.cand, g + 1, B.nb, c + k);
            while (B.qoff[a + 1] <= g0 + g) a++;
        }
        const uint64_t G = g0 + g;
        const uint64_t p = ix.suffix(B.rlo[g] + (c + k - B.cand[g]));
        if (G > B.qoff[a] && p > 0 && B.q[G - 1] == ix.text[p - 1] && (!B.bits || ((B.bits[(p - 1) >> 5] >> ((p - 1) & 31)) & 1u))) continue;
        if (B.kk < B.min_len) {                        // capped build, k > L: the slice matched L symbols, the text must go on to k
            if (p + B.min_len > ix.n) continue;
            bool ok = true;
            for (uint32_t t = B.kk; t < B.min_len && ok; t++) ok = B.q[G + t] == ix.text[p + t];
            if (!ok) continue;
        }
        f(k, g, a, p);
    }
}

__global__ __launch_bounds__(256) void k_mem_count(SearchIndex ix, MemBatch B, uint64_t* __restrict__ cnt_sum)
{
    __shared__ uint64_t s_w[4];
    const uint64_t total = B.cand[B.nb], chunk = scan_chunk(total);
    const uint64_t lo = (uint64_t)blockIdx.x * chunk, hi = lo + chunk < total ? lo + chunk : total;
    uint64_t acc = 0;
    for (uint64_t t = lo; t < hi; t += LOC_BLK) {
        uint64_t cnt[1] = {0}, tot[1];
        mem_walk8(ix, B, t + (uint64_t)threadIdx.x * 8, hi, [&](uint32_t, uint64_t, uint64_t, uint64_t) { cnt[0]++; });
        wg_scan(cnt, tot, s_w);
        acc += tot[0];
    }
    if (threadIdx.x == 0) cnt_sum[blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void k_mem_emit(SearchIndex ix, MemBatch B, const uint64_t* __restrict__ cnt_base, uint32_t both,
                                                  uint64_t* __restrict__ out_query, uint32_t* __restrict__ out_qoff,
                                                  uint8_t* __restrict__ out_strand, uint32_t* __restrict__ out_len,
                                                  uint64_t* __restrict__ out_pos)
{
    __shared__ uint64_t s_w[4];
    const uint64_t total = B.cand[B.nb], chunk = scan_chunk(total);
    const uint64_t lo = (uint64_t)blockIdx.x * chunk, hi = lo + chunk < total ? lo + chunk : total;
    uint64_t run = cnt_base[blockIdx.x];
    for (uint64_t t = lo; t < hi; t += LOC_BLK) {
        const uint64_t c = t + (uint64_t)threadIdx.x * 8;
        uint32_t fl = 0;
        uint64_t cnt[1] = {0}, tot[1];
        mem_walk8(ix, B, c, hi, [&](uint32_t k, uint64_t, uint64_t, uint64_t) { fl |= 1u << k; cnt[0]++; });
        wg_scan(cnt, tot, s_w);
        uint64_t at = run + cnt[0];
        if (fl) {
            mem_walk8(ix, B, c, hi, [&](uint32_t, uint64_t g, uint64_t a, uint64_t p) {
                // the exact length: on from the k' already matched, to the end of the query or of the text
                const uint64_t G = B.qoff[0] + g, qe = B.qoff[a + 1];
                const uint64_t lim = qe - G < ix.n - p ? qe - G : ix.n - p;
                const uint64_t l = common_prefix<uint64_t>(B.q + G, ix.text + p, B.kk, lim);
                out_query[at] = both ? a >> 1 : a;
                out_qoff[at] = (uint32_t)(G - B.qoff[a]);
                out_strand[at] = (uint8_t)(both ? a & 1 : 0);
                out_len[at] = (uint32_t)l;
                out_pos[at] = p;
                at++;
            });
        }
        run += tot[0];
    }
}

}  // namespace sufr

namespace {

// the bitmap of the indexed positions, once per index (none when every position is indexed)
int mem_bitmap(sufr_hip_ctx* ctx, const sufr_hip_index* ix)
{
    if (ix->ix.s >= ix->ix.n) return 0;
    std::lock_guard<std::mutex> lock(ix->mem_mu);
    if (ix->mem_bits_done) return 0;
    sufr::Pipeline& pl = ctx->pl;
    const uint64_t words = (ix->ix.n + 31) / 32;
    void* bits = nullptr;
    if (hipMalloc(&bits, words * 4) != hipSuccess) {
        (void)hipGetLastError();
        pl.set_error("mems: hipMalloc of the indexed-position bitmap (" + std::to_string(words * 4) + " bytes) failed");
        return SUFR_HIP_E_NOMEM;
    }
    const uint32_t grid = (pl.num_cus ? pl.num_cus : 256u) * 8u;
    bool ok = hipMemsetAsync(bits, 0, words * 4, pl.stream) == hipSuccess;
    if (ok) hipLaunchKernelGGL(sufr::k_mem_bitmap, dim3(grid), dim3(256), 0, pl.stream, ix->ix, (uint32_t*)bits);
    ok = ok && hipGetLastError() == hipSuccess && hipStreamSynchronize(pl.stream) == hipSuccess;   // other streams may use it next
    if (!ok) { (void)hipFree(bits); pl.set_error("mems: building the indexed-position bitmap failed"); return SUFR_HIP_E_HIP; }
    ix->mem_bits = bits;
    ix->mem_bits_done = true;
    return 0;
}

}  // namespace

extern "C" {

int sufr_hip_mems_device(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_queries, const void* d_offsets,
                         uint64_t num_queries, uint32_t min_len, uint64_t max_occ, uint32_t flags, uint64_t cap,
                         void* d_query, void* d_query_offset, void* d_strand, void* d_length, void* d_position,
                         uint64_t* total_out)
{
    if (total_out) *total_out = 0;
    if (!ctx || !ix || (num_queries && (!d_queries || !d_offsets))) return SUFR_HIP_E_INVALID;
    sufr::Pipeline& pl = ctx->pl;
    pl.err.clear();
    if (const int rc = query_check(ctx, ix, "MEMs")) return rc;
    if (min_len == 0) { ctx->pl.set_error("mems: min_len must be at least 1"); return SUFR_HIP_E_INVALID; }
    if (!num_queries) return 0;
    int rc;
    if ((rc = mem_bitmap(ctx, ix))) return rc;
    // the byte count of the batch sizes the scratch
    unsigned long long ends[2] = {0, 0};
    const uint64_t* uoff = (const uint64_t*)d_offsets;
    if (hipMemcpyAsync(&ends[0], uoff, 8, hipMemcpyDeviceToHost, pl.stream) != hipSuccess ||
        hipMemcpyAsync(&ends[1], uoff + num_queries, 8, hipMemcpyDeviceToHost, pl.stream) != hipSuccess ||
        hipStreamSynchronize(pl.stream) != hipSuccess) { pl.set_error("mems: reading the batch offsets failed"); return SUFR_HIP_E_HIP; }
    if (ends[1] <= ends[0]) return 0;
    const bool both = (flags & SUFR_MEM_BOTH_STRANDS) != 0;
    const uint64_t nb = (ends[1] - ends[0]) * (both ? 2 : 1), nq = num_queries * (both ? 2 : 1);
    const uint32_t grid = (pl.num_cus ? pl.num_cus : 256u) * 8u;
    const uint8_t* q = (const uint8_t*)d_queries;
    const uint64_t* qoff = uoff;
    if (both) {
        if ((rc = pl.ensure(ctx->xq, nb + 8)) || (rc = pl.ensure(ctx->xoff, (nq + 1) * 8))) return rc;
        hipLaunchKernelGGL(sufr::k_mem_revcomp, dim3(grid), dim3(256), 0, pl.stream, q, uoff, num_queries, (uint8_t*)ctx->xq.p,
                           (uint64_t*)ctx->xoff.p);
        q = (const uint8_t*)ctx->xq.p;
        qoff = (const uint64_t*)ctx->xoff.p;
    }
    // rank range of every offset's k'-prefix, then the exclusive scan of the range sizes
    const uint64_t L = ix->built_mql;
    const uint32_t kk = L > 0 && L < min_len ? (uint32_t)L : min_len;
    const uint64_t nblk = (nb + sufr::LOC_BLK - 1) / sufr::LOC_BLK;
    if ((rc = pl.ensure(ctx->xlo, nb * 8)) || (rc = pl.ensure(ctx->xhi, nb * 8)) || (rc = pl.ensure(ctx->xcand, (nb + 1) * 8)) ||
        (rc = pl.ensure(ctx->xsum, (nblk + 1 + sufr::SCAN_WGS + 1) * 8))) return rc;
    uint64_t* rlo = (uint64_t*)ctx->xlo.p;
    uint64_t* cand = (uint64_t*)ctx->xcand.p;
    uint64_t* bsum = (uint64_t*)ctx->xsum.p;
    uint64_t* cnt_sum = bsum + nblk + 1;
    hipLaunchKernelGGL(sufr::k_mem_ranges, dim3(grid), dim3(256), 0, pl.stream, ix->ix, q, qoff, nq, effective_mql(ix, 0, 0), min_len, kk,
                       max_occ, rlo, (uint64_t*)ctx->xhi.p);
    hipLaunchKernelGGL(sufr::k_locate_counts, dim3((uint32_t)nblk), dim3(256), 0, pl.stream, (const uint64_t*)rlo,
                       (const uint64_t*)ctx->xhi.p, nb, (uint64_t)0, cand, bsum);
    hipLaunchKernelGGL(sufr::k_locate_scan, dim3(1), dim3(1024), 0, pl.stream, bsum, nblk, bsum + nblk);
    hipLaunchKernelGGL(sufr::k_locate_apply, dim3((uint32_t)((nb + 256) / 256)), dim3(256), 0, pl.stream, cand, nb, (const uint64_t*)bsum,
                       (const uint64_t*)(bsum + nblk));
    unsigned long long ncand = 0;
    if ((rc = read_totals(pl, bsum + nblk, 1, &ncand, "mems: counting the candidates failed"))) return rc;
    if (!ncand) return 0;
    // the left condition per candidate, counted per workgroup, then the MEM total
    const sufr::MemBatch B{q, qoff, nq, rlo, cand, nb, (const uint32_t*)ix->mem_bits, min_len, kk};
    hipLaunchKernelGGL(sufr::k_mem_count, dim3(sufr::SCAN_WGS), dim3(256), 0, pl.stream, ix->ix, B, cnt_sum);
    hipLaunchKernelGGL(sufr::k_locate_scan, dim3(1), dim3(1024), 0, pl.stream, cnt_sum, (uint64_t)sufr::SCAN_WGS, cnt_sum + sufr::SCAN_WGS);
    unsigned long long nmem = 0;
    if ((rc = read_totals(pl, cnt_sum + sufr::SCAN_WGS, 1, &nmem, "mems: counting the MEMs failed"))) return rc;
    if (total_out) *total_out = nmem;
    if (nmem > cap) {
        pl.set_error("mems: " + std::to_string(nmem) + " MEMs, room for " + std::to_string(cap));
        return SUFR_HIP_E_CAPACITY;
    }
    if (!nmem) return 0;
    if (!d_query || !d_query_offset || !d_strand || !d_length || !d_position) return SUFR_HIP_E_INVALID;
    hipLaunchKernelGGL(sufr::k_mem_emit, dim3(sufr::SCAN_WGS), dim3(256), 0, pl.stream, ix->ix, B, (const uint64_t*)cnt_sum, (uint32_t)both,
                       (uint64_t*)d_query, (uint32_t*)d_query_offset, (uint8_t*)d_strand, (uint32_t*)d_length, (uint64_t*)d_position);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { pl.set_error(std::string("mems: ") + hipGetErrorString(e)); return SUFR_HIP_E_HIP; }
    return 0;
}

int sufr_hip_mems(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const uint8_t* queries, const uint64_t* offsets, uint64_t num_queries,
                  uint32_t min_len, uint64_t max_occ, uint32_t flags, uint64_t cap, uint64_t* query, uint32_t* query_offset,
                  uint8_t* strand, uint32_t* length, uint64_t* position, uint64_t* total_out)
{
    if (total_out) *total_out = 0;
    if (!ctx || !ix || (num_queries && !offsets)) return SUFR_HIP_E_INVALID;
    ctx->pl.err.clear();
    if (const int rc = query_check(ctx, ix, "MEMs")) return rc;
    if (min_len == 0) { ctx->pl.set_error("mems: min_len must be at least 1"); return SUFR_HIP_E_INVALID; }
    if (!num_queries) return 0;
    const uint64_t qbytes = offsets[num_queries], obytes = (num_queries + 1) * 8;
    // one allocation: queries | offsets | records (cap of each)
    const uint64_t o_at = (qbytes + 7) / 8 * 8, q_at = o_at + obytes, pos_at = q_at + cap * 8, qo_at = pos_at + cap * 8;
    const uint64_t len_at = qo_at + cap * 4, st_at = len_at + cap * 4;
    uint8_t* d;
    int rc = stage_batch(ctx, "MEM", queries, offsets, num_queries, o_at, st_at + cap + 8, &d);
    uint64_t total = 0;
    if (!rc) rc = sufr_hip_mems_device(ctx, ix, d, d + o_at, num_queries, min_len, max_occ, flags, cap, d + q_at, d + qo_at, d + st_at,
                                       d + len_at, d + pos_at, &total);
    if (total_out) *total_out = total;
    return unstage_batch(ctx, "MEM", d, rc, {{query, q_at, total * 8}, {query_offset, qo_at, total * 4}, {strand, st_at, total},
                                             {length, len_at, total * 4}, {position, pos_at, total * 8}});
}

}  // extern "C"
