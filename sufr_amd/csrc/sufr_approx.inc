// sufr_approx.inc -- k-mismatch search of a query batch on a device-resident index: seed and verify with the pigeonhole
// filter (included by sufr_kernels.hip after sufr_mem.inc; include/sufr_approx.h, DESIGN.md section 15).
//
// take_batch         (sufr_search.inc) the bitmap of the index, the two ends of the batch (a synchronisation of its own), the
//                    doubled batch with both strands
// k_approx_seeds     one lane per seed g = a * (d + 1) + i (grid-stride): the rank range of the first k' bytes of piece i of
//                    query a, found in place by search_range; empty when the query is shorter than d + 1, marked dead
//                    (APPROX_DEAD in the low bound) when it holds more than max_occ suffixes
// candidate_starts   (sufr_search.inc) the exclusive scan of the range sizes: the candidate starts; one synchronisation
//                    reads the candidate total.  pigeonhole_candidates (below) is these two steps, shared with sufr_edit.inc
// k_approx_count     SCAN_WGS workgroups over the candidates, 8 per lane: candidate -> seed by binary search of the starts,
//                    p = SA[lo + ...] - o_i, the window bounds, the rest of a capped piece, the anchors of the lower pieces
//                    (piece bytes, one bitmap bit, liveness), the Hamming distance 8 bytes a step with an exit at d + 1;
//                    counts per workgroup
// scan_total         (sufr_search.inc) k_locate_scan: the record total (second synchronisation) and the workgroup bases
// k_approx_emit      the verdicts again (one byte per candidate, kept in a register), scanned in the workgroup; the records
// No MFMA, no LDS beyond the scan words, no scratch.
// From sufr_search.inc: search_range, common_prefix, last_le, wg_scan and scan_chunk (SCAN_WGS workgroups); the host side of
// the driver (query_check, take_batch, candidate_starts, scan_total, records_fit, any_null, launch_status) and
// staged_records for the host-pointer entry points.

namespace sufr {

static constexpr uint64_t APPROX_DEAD = ~0ull;        // rlo of a seed that starts more than max_occ suffixes
static constexpr uint32_t APPROX_NO = 0xFFu;          // verdict of a candidate that gives no record (else: its distance)

struct ApproxBatch {
    const uint8_t* q;           // query bytes (the doubled batch with both strands)
    const uint64_t* qoff;       // nq + 1 offsets
    uint64_t nq;
    const uint64_t* rlo;        // per seed g = a * np + i: first rank of its range, APPROX_DEAD for a dead piece
    const uint64_t* cand;       // per seed: first candidate (exclusive scan of the range sizes), ns + 1 entries
    uint64_t ns;                // seeds in the batch: nq * np
    const uint32_t* bits;       // indexed positions, or nullptr: every position is indexed
    uint64_t L;                 // the build's max_query_len (0: none): a seed is the first min(len, L) bytes of its piece
    uint32_t np, d;             // pieces per query (d + 1) and the distance bound
};

__device__ __forceinline__ uint64_t approx_piece(uint64_t i, uint64_t m, uint32_t np) { return i * m / np; }

__global__ __launch_bounds__(256) void k_approx_seeds(SearchIndex ix, const uint8_t* __restrict__ queries, const uint64_t* __restrict__ qoff,
                                                      uint64_t nq, uint64_t L, uint32_t np, uint64_t max_occ,
                                                      uint64_t* __restrict__ lo_out, uint64_t* __restrict__ hi_out)
{
    const uint64_t ns = nq * np, stride = (uint64_t)gridDim.x * 256;
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < ns; g += stride) {
        const uint64_t a = g / np, i = g - a * np, b = qoff[a], m = qoff[a + 1] - b;
        uint64_t lo = 0, hi = 0;
        if (m >= np) {
            const uint64_t o = approx_piece(i, m, np), len = approx_piece(i + 1, m, np) - o;
            search_range(ix, queries + b + o, (uint32_t)(L > 0 && L < len ? L : len), L, lo, hi);
            if (max_occ && hi - lo > max_occ) lo = hi = APPROX_DEAD;
        }
        lo_out[g] = lo; hi_out[g] = hi;
    }
}

// differing bytes of two 8-byte words
__device__ __forceinline__ uint32_t approx_diff8(uint64_t x, uint64_t y)
{
    const uint64_t v = x ^ y, lo7 = 0x7F7F7F7F7F7F7F7Full;
    return (uint32_t)__popcll((((v & lo7) + lo7) | v) & ~lo7);       // bit 7 of every byte that is not 0
}

// candidate c of seed g: APPROX_NO, or the distance of the window it stands for; p_out: the window start
__device__ __forceinline__ uint32_t approx_verify(const SearchIndex& ix, const ApproxBatch& B, uint64_t g, uint64_t c, uint64_t& p_out)
{
    const uint64_t a = g / B.np, i = g - a * B.np, b = B.qoff[a], m = B.qoff[a + 1] - b;
    const uint64_t o = approx_piece(i, m, B.np), len = approx_piece(i + 1, m, B.np) - o;
    const uint64_t sp = ix.suffix(B.rlo[g] + (c - B.cand[g]));
    if (sp < o) return APPROX_NO;                                    // the window would start before the text
    const uint64_t p = sp - o;
    p_out = p;
    if (p + m > ix.n) return APPROX_NO;
    const uint8_t* __restrict__ Q = B.q + b;
    const uint8_t* __restrict__ T = ix.text + p;
    if (B.L > 0 && B.L < len && common_prefix<uint64_t>(Q + o, T + o, B.L, len) < len) return APPROX_NO;   // capped build: the rest of the piece
    // a lower piece that anchors p reports the window: its bytes, then its start in the bitmap, then its liveness
    uint64_t oj = 0;
    for (uint64_t j = 0; j < i; j++) {
        const uint64_t on = approx_piece(j + 1, m, B.np), pj = p + oj;
        if (common_prefix<uint64_t>(Q + oj, T + oj, 0, on - oj) == on - oj && (!B.bits || ((B.bits[pj >> 5] >> (pj & 31)) & 1u)) &&
            B.rlo[g - i + j] != APPROX_DEAD) return APPROX_NO;
        oj = on;
    }
    uint32_t h = 0;
    uint64_t t = 0;
    for (; t + 8 <= m && h <= B.d; t += 8) {
        uint64_t x, y;
        __builtin_memcpy(&x, Q + t, 8);
        __builtin_memcpy(&y, T + t, 8);
        h += approx_diff8(x, y);
    }
    for (; t < m && h <= B.d; t++) h += Q[t] != T[t];
    return h <= B.d ? h : APPROX_NO;
}

// walks the (up to) 8 candidates [c, c_hi) of a lane: f(k, g) for candidate c + k of seed g
template <typename F>
__device__ __forceinline__ void approx_walk8(const ApproxBatch& B, uint64_t c, uint64_t c_hi, F f)
{
    if (c >= c_hi) return;
    uint64_t g = last_le(B.cand, 0, B.ns, c);
    for (uint32_t k = 0; k < 8 && c + k < c_hi; k++) {
        if (B.cand[g + 1] <= c + k) g = last_le(B.cand, g + 1, B.ns, c + k);
        f(k, g);
    }
}

__global__ __launch_bounds__(256) void k_approx_count(SearchIndex ix, ApproxBatch B, uint64_t* __restrict__ cnt_sum)
{
    __shared__ uint64_t s_w[4];
    const uint64_t total = B.cand[B.ns], chunk = scan_chunk(total);
    const uint64_t lo = (uint64_t)blockIdx.x * chunk, hi = lo + chunk < total ? lo + chunk : total;
    uint64_t acc = 0;
    for (uint64_t t = lo; t < hi; t += LOC_BLK) {
        const uint64_t c = t + (uint64_t)threadIdx.x * 8;
        uint64_t cnt[1] = {0}, tot[1];
        approx_walk8(B, c, hi, [&](uint32_t k, uint64_t g) { uint64_t p; cnt[0] += approx_verify(ix, B, g, c + k, p) != APPROX_NO; });
        wg_scan(cnt, tot, s_w);
        acc += tot[0];
    }
    if (threadIdx.x == 0) cnt_sum[blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void k_approx_emit(SearchIndex ix, ApproxBatch B, const uint64_t* __restrict__ cnt_base, uint32_t both,
                                                     uint64_t* __restrict__ out_query, uint8_t* __restrict__ out_strand,
                                                     uint64_t* __restrict__ out_pos, uint8_t* __restrict__ out_mism)
{
    __shared__ uint64_t s_w[4];
    const uint64_t total = B.cand[B.ns], chunk = scan_chunk(total);
    const uint64_t lo = (uint64_t)blockIdx.x * chunk, hi = lo + chunk < total ? lo + chunk : total;
    uint64_t run = cnt_base[blockIdx.x];
    for (uint64_t t = lo; t < hi; t += LOC_BLK) {
        const uint64_t c = t + (uint64_t)threadIdx.x * 8;
        uint64_t verdicts = ~0ull;                                   // byte k: the verdict of candidate c + k
        uint64_t cnt[1] = {0}, tot[1];
        approx_walk8(B, c, hi, [&](uint32_t k, uint64_t g) {
            uint64_t p;
            const uint32_t v = approx_verify(ix, B, g, c + k, p);
            if (v != APPROX_NO) { verdicts ^= (uint64_t)(v ^ APPROX_NO) << (8 * k); cnt[0]++; }
        });
        wg_scan(cnt, tot, s_w);
        uint64_t at = run + cnt[0];
        if (verdicts != ~0ull) {
            approx_walk8(B, c, hi, [&](uint32_t k, uint64_t g) {
                const uint32_t v = (uint32_t)(verdicts >> (8 * k)) & 0xFFu;
                if (v == APPROX_NO) return;
                const uint64_t a = g / B.np, i = g - a * B.np;
                out_query[at] = both ? a >> 1 : a;
                out_strand[at] = (uint8_t)(both ? a & 1 : 0);
                out_pos[at] = ix.suffix(B.rlo[g] + (c + k - B.cand[g])) - approx_piece(i, B.qoff[a + 1] - B.qoff[a], B.np);
                out_mism[at] = (uint8_t)v;
                at++;
            });
        }
        run += tot[0];
    }
}

}  // namespace sufr

namespace {

int approx_args(sufr_hip_ctx* ctx, const sufr_hip_index* ix, uint32_t max_mismatches)
{
    if (const int rc = query_check(ctx, ix, "k-mismatch searches")) return rc;
    if (max_mismatches > SUFR_APPROX_MAX_MISMATCHES) {
        ctx->pl.set_error("approx: max_mismatches must be at most " + std::to_string(SUFR_APPROX_MAX_MISMATCHES));
        return SUFR_HIP_E_INVALID;
    }
    return 0;
}

// The pigeonhole candidates of a batch (k-mismatch and k-difference): d + 1 seeds per query, the rank range of every seed
// (k_approx_seeds), the exclusive scan of the live range sizes.  B: what the count and emit kernels read.
int pigeonhole_candidates(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const QueryBatch& b, uint32_t d, uint64_t max_occ, const char* tag,
                          sufr::ApproxBatch& B, Candidates& c)
{
    const uint32_t np = d + 1;
    const uint64_t ns = b.nq * np;
    if (const int rc = candidate_starts(ctx, ns, tag, [&](uint64_t* rlo, uint64_t* rhi) {
        hipLaunchKernelGGL(sufr::k_approx_seeds, dim3(b.grid), dim3(256), 0, ctx->pl.stream, ix->ix, b.q, b.qoff, b.nq, (uint64_t)ix->built_mql, np,
                           max_occ, rlo, rhi);
    }, c)) return rc;                                                // (c is not set when the scratch could not be had)
    B = sufr::ApproxBatch{b.q, b.qoff, b.nq, c.rlo, c.cand, ns, (const uint32_t*)ix->mem_bits, ix->built_mql, np, d};
    return 0;
}

// The host-pointer entry point of a pigeonhole search: `limits` checks the arguments, `device` is the *_device twin; the
// record columns are query, strand, where (position / end) and distance (mismatches / edits).
using PigeonholeDevice = int (*)(sufr_hip_ctx*, const sufr_hip_index*, const void*, const void*, uint64_t, uint32_t, uint64_t, uint32_t, uint64_t,
                                 void*, void*, void*, void*, uint64_t*);

int pigeonhole_host(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const uint8_t* queries, const uint64_t* offsets, uint64_t num_queries, uint32_t d,
                    uint64_t max_occ, uint32_t flags, uint64_t cap, uint64_t* query, uint8_t* strand, uint64_t* where, uint8_t* distance,
                    uint64_t* total_out, const char* what, int (*limits)(sufr_hip_ctx*, const sufr_hip_index*, uint32_t), PigeonholeDevice device)
{
    if (total_out) *total_out = 0;
    if (!ctx || !ix || (num_queries && !offsets)) return SUFR_HIP_E_INVALID;
    ctx->pl.err.clear();
    if (const int rc = limits(ctx, ix, d)) return rc;
    if (!num_queries) return 0;
    return staged_records(ctx, what, queries, offsets, num_queries, cap, {{query, 8}, {strand, 1}, {where, 8}, {distance, 1}}, 0, total_out,
                          [&](const void* d_q, const void* d_off, void* const* col, uint64_t* total) {
        return device(ctx, ix, d_q, d_off, num_queries, d, max_occ, flags, cap, col[0], col[1], col[2], col[3], total);
    });
}

}  // namespace

extern "C" {

int sufr_hip_approx_device(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_queries, const void* d_offsets,
                           uint64_t num_queries, uint32_t max_mismatches, uint64_t max_occ, uint32_t flags, uint64_t cap,
                           void* d_query, void* d_strand, void* d_position, void* d_mismatches, uint64_t* total_out)
{
    if (total_out) *total_out = 0;
    if (!ctx || !ix || (num_queries && (!d_queries || !d_offsets))) return SUFR_HIP_E_INVALID;
    sufr::Pipeline& pl = ctx->pl;
    pl.err.clear();
    int rc;
    if ((rc = approx_args(ctx, ix, max_mismatches))) return rc;
    QueryBatch b;
    if ((rc = take_batch(ctx, ix, d_queries, d_offsets, num_queries, (flags & SUFR_APPROX_BOTH_STRANDS) != 0, "approx", b)) || !b.nb) return rc;
    sufr::ApproxBatch B;
    Candidates c;
    if ((rc = pigeonhole_candidates(ctx, ix, b, max_mismatches, max_occ, "approx", B, c)) || !c.ncand) return rc;
    // the verdict of every candidate, counted per workgroup, then the record total
    hipLaunchKernelGGL(sufr::k_approx_count, dim3(sufr::SCAN_WGS), dim3(256), 0, pl.stream, ix->ix, B, c.cnt_sum);
    unsigned long long nrec = 0;
    if ((rc = scan_total(pl, c.cnt_sum, sufr::SCAN_WGS, &nrec, "approx", "counting the records failed"))) return rc;
    if ((rc = records_fit(pl, "approx", "records", nrec, cap, total_out)) || !nrec) return rc;
    if (any_null({d_query, d_strand, d_position, d_mismatches})) return SUFR_HIP_E_INVALID;
    hipLaunchKernelGGL(sufr::k_approx_emit, dim3(sufr::SCAN_WGS), dim3(256), 0, pl.stream, ix->ix, B, (const uint64_t*)c.cnt_sum, (uint32_t)b.both,
                       (uint64_t*)d_query, (uint8_t*)d_strand, (uint64_t*)d_position, (uint8_t*)d_mismatches);
    return launch_status(pl, "approx");
}

int sufr_hip_approx(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const uint8_t* queries, const uint64_t* offsets, uint64_t num_queries,
                    uint32_t max_mismatches, uint64_t max_occ, uint32_t flags, uint64_t cap, uint64_t* query, uint8_t* strand,
                    uint64_t* position, uint8_t* mismatches, uint64_t* total_out)
{
    return pigeonhole_host(ctx, ix, queries, offsets, num_queries, max_mismatches, max_occ, flags, cap, query, strand, position, mismatches,
                           total_out, "k-mismatch", approx_args, sufr_hip_approx_device);
}

}  // extern "C"
