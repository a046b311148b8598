// sufr_mem.inc -- maximal exact matches (MEMs) of a query batch on a device-resident index (included by sufr_kernels.hip
// after sufr_match.inc; include/sufr_mem.h, DESIGN.md section 14).
//
// take_batch         (sufr_search.inc) the bitmap of the index (k_mem_bitmap, once), the two ends of the batch (a
//                    synchronisation of its own) and, with both strands, the doubled batch (k_mem_revcomp)
// k_mem_ranges       one lane per query offset (grid-stride): the rank range of the k'-prefix Q[j..j+k') found in place by
//                    search_range (what k_search_batch runs); an empty range when j + k > m or the range holds more than
//                    max_occ suffixes
// candidate_starts   (sufr_search.inc) k_locate_counts / k_locate_scan / k_locate_apply: the exclusive scan of the range sizes
//                    is the candidate starts; one synchronisation reads the candidate total
// k_mem_count        1024 workgroups over the candidates, 8 per lane: candidate -> offset by binary search of the starts,
//                    p = SA[lo + ...], the left condition (one query byte, one text byte, one bitmap bit); counts per workgroup
// scan_total         (sufr_search.inc) k_locate_scan: the MEM total (second synchronisation) and the workgroup bases
// k_mem_emit         the flags again, scanned in the workgroup; every MEM is extended with 8-byte compares and written
// No MFMA, no LDS beyond the scan words, no scratch.
// From sufr_search.inc: search_range, common_prefix, last_le (offset -> query, candidate -> offset), wg_scan and scan_chunk
// (SCAN_WGS workgroups); the host side of the driver (query_check, take_batch, candidate_starts, scan_total, records_fit,
// any_null, launch_status) and staged_records for the host-pointer entry point.

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
    int rc;
    if ((rc = query_check(ctx, ix, "MEMs"))) return rc;
    if (min_len == 0) { pl.set_error("mems: min_len must be at least 1"); return SUFR_HIP_E_INVALID; }
    QueryBatch b;
    if ((rc = take_batch(ctx, ix, d_queries, d_offsets, num_queries, (flags & SUFR_MEM_BOTH_STRANDS) != 0, "mems", b)) || !b.nb) return rc;
    // rank range of every offset's k'-prefix: the candidates
    const uint64_t L = ix->built_mql;
    const uint32_t kk = L > 0 && L < min_len ? (uint32_t)L : min_len;
    Candidates c;
    rc = candidate_starts(ctx, b.nb, "mems", [&](uint64_t* rlo, uint64_t* rhi) {
        hipLaunchKernelGGL(sufr::k_mem_ranges, dim3(b.grid), dim3(256), 0, pl.stream, ix->ix, b.q, b.qoff, b.nq, effective_mql(ix, 0, 0), min_len,
                           kk, max_occ, rlo, rhi);
    }, c);
    if (rc || !c.ncand) return rc;
    // the left condition per candidate, counted per workgroup, then the MEM total
    const sufr::MemBatch B{b.q, b.qoff, b.nq, c.rlo, c.cand, b.nb, (const uint32_t*)ix->mem_bits, min_len, kk};
    hipLaunchKernelGGL(sufr::k_mem_count, dim3(sufr::SCAN_WGS), dim3(256), 0, pl.stream, ix->ix, B, c.cnt_sum);
    unsigned long long nmem = 0;
    if ((rc = scan_total(pl, c.cnt_sum, sufr::SCAN_WGS, &nmem, "mems", "counting the MEMs failed"))) return rc;
    if ((rc = records_fit(pl, "mems", "MEMs", nmem, cap, total_out)) || !nmem) return rc;
    if (any_null({d_query, d_query_offset, d_strand, d_length, d_position})) return SUFR_HIP_E_INVALID;
    hipLaunchKernelGGL(sufr::k_mem_emit, dim3(sufr::SCAN_WGS), dim3(256), 0, pl.stream, ix->ix, B, (const uint64_t*)c.cnt_sum, (uint32_t)b.both,
                       (uint64_t*)d_query, (uint32_t*)d_query_offset, (uint8_t*)d_strand, (uint32_t*)d_length, (uint64_t*)d_position);
    return launch_status(pl, "mems");
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
    return staged_records(ctx, "MEM", queries, offsets, num_queries, cap, {{query, 8}, {query_offset, 4}, {strand, 1}, {length, 4}, {position, 8}},
                          0, total_out, [&](const void* d_q, const void* d_off, void* const* col, uint64_t* total) {
        return sufr_hip_mems_device(ctx, ix, d_q, d_off, num_queries, min_len, max_occ, flags, cap, col[0], col[1], col[2], col[3], col[4], total);
    });
}

}  // extern "C"
