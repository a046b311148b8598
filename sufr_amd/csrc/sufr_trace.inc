// sufr_trace.inc -- alignment traceback of k-difference records on a device-resident text: for every record (query, strand,
// end, edits) the start of its alignment and its CIGAR (included by sufr_kernels.hip after sufr_edit.inc;
// include/sufr_align.h, DESIGN.md section 17).
//
// k_trace_check      one lane per record: the five checks that need no table (query, strand, end, edits, query length); the
//                    first offending record (atomicMin), the longest query of the records (atomicMax), whether a record is on
//                    strand 1, the byte range of the batch.  First synchronisation: it sizes the chunks.
// k_mem_revcomp      (double_batch, sufr_search.inc) only when a record is on strand 1: the doubled batch
// per chunk of records (as many as the row storage holds at 8 bytes per row of the longest query):
//   k_trace_rows     one record per lane: the rows of the 2 * edits + 1 band (trace_forward, sufr_trace.h), two words per row to
//                    rows[(r - 1) * chunk_records + lane_record]; the banded value of the end cell against `edits` (the sixth
//                    check); the walk (trace_walk) for the start and the number of runs; wg_scan: the offsets inside the
//                    workgroup, the workgroup's sum
//   k_locate_scan    (sufr_search.inc) the workgroup bases and the total of the chunk
//   k_trace_write    the walk again over the rows of the chunk, which are still there: cigar_off and the runs, last run first
//                    from the end of the record's slice, nothing at or beyond cigar_cap; the running base of the next chunk
// Second synchronisation: the CIGAR total and the first record whose edits is not D(end + 1).
//
// Ops are not carried from the first walk to the second: a chunk's rows stay in place until its runs are written, the offsets
// are local to the chunk and a running base, kept on the device in two words that the chunks use in turn, makes them global.
// Packing the ops (2 bits each) for a write after the last chunk would cost (m + edits) / 4 bytes per record of the whole call
// and a third kernel; walking twice costs a second read of at most m + edits rows per record and no memory.
// No MFMA, no scratch; LDS: the scan words.

#include "sufr_trace.h"

namespace sufr {

static constexpr uint64_t TRACE_SCRATCH_DEFAULT = (uint64_t)256 << 20;      // bytes of row storage unless set_trace_scratch says otherwise
static constexpr uint64_t TRACE_CHUNK_MAX = (uint64_t)1 << 20;              // records of a chunk at most

// scalars of a call (u64 words)
enum { TR_BASE0 = 0, TR_BASE1 = 1, TR_BAD = 2, TR_MAXM = 3, TR_STRAND1 = 4, TR_G0 = 5, TR_GEND = 6, TR_CHUNK = 7, TR_N = 8 };

struct TraceRecs {
    const uint64_t* query;
    const uint8_t* strand;
    const uint64_t* end;
    const uint8_t* edits;
    uint64_t num;
};

__global__ __launch_bounds__(256) void k_trace_check(TraceRecs R, const uint64_t* __restrict__ qoff, uint64_t nq, uint64_t n,
                                                     unsigned long long* __restrict__ sc)
{
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t == 0) { sc[TR_G0] = qoff[0]; sc[TR_GEND] = qoff[nq]; }
    uint64_t longest = 0;                                           // of the wave: one atomic per wave, not per record
    if (t < R.num) {
        const uint64_t a = R.query[t], e = R.end[t];
        const uint32_t s = R.strand[t], v = R.edits[t];
        bool ok = a < nq && s <= 1 && e < n && v <= SUFR_EDIT_MAX_EDITS;
        if (ok) {
            const uint64_t m = qoff[a + 1] - qoff[a];
            ok = m >= (uint64_t)v + 1;
            if (ok) longest = m;
            if (ok && s) sc[TR_STRAND1] = 1;
        }
        if (!ok) atomicMin(&sc[TR_BAD], (unsigned long long)t);
    }
    for (int o = 32; o > 0; o >>= 1) { const uint64_t u = __shfl_xor(longest, o); longest = u > longest ? u : longest; }
    if ((threadIdx.x & 63u) == 0 && longest) atomicMax(&sc[TR_MAXM], (unsigned long long)longest);
}

// the query of record t in the batch (q, qoff): the doubled batch (query 2 a + strand) when both
struct TraceQuery { const uint8_t* Q; uint64_t m; uint32_t v; int64_t g; };
__device__ __forceinline__ TraceQuery trace_query(const TraceRecs& R, uint64_t t, const uint8_t* __restrict__ q,
                                                  const uint64_t* __restrict__ qoff, uint64_t g0, uint32_t both)
{
    const uint64_t a = both ? 2 * R.query[t] + R.strand[t] : R.query[t];
    const uint64_t b = qoff[a] - g0, m = qoff[a + 1] - qoff[a];
    return {q + b, m, (uint32_t)R.edits[t], (int64_t)(R.end[t] + 1) - (int64_t)m};
}

// records [c0, c0 + cr): rows, start, the runs of every record (nruns, chunk-local), the exclusive offsets inside the workgroup
// (to cigar_off) and the workgroup sums
__global__ __launch_bounds__(256) void k_trace_rows(const uint8_t* __restrict__ T, uint64_t n, TraceRecs R, const uint8_t* __restrict__ q,
                                                    const uint64_t* __restrict__ qoff, uint64_t g0, uint32_t both, uint64_t c0, uint64_t cr,
                                                    uint2* __restrict__ rows, uint64_t* __restrict__ start, uint32_t* __restrict__ nruns,
                                                    uint64_t* __restrict__ cigar_off, uint64_t* __restrict__ wgsum,
                                                    unsigned long long* __restrict__ sc)
{
    __shared__ uint64_t s_w[4];
    const uint64_t lr = (uint64_t)blockIdx.x * 256 + threadIdx.x, t = c0 + lr;
    uint64_t cnt[1] = {0}, tot[1];
    if (lr < cr) {
        const TraceQuery A = trace_query(R, t, q, qoff, g0, both);
        uint2* __restrict__ mine = rows + lr;
        const uint32_t score = trace_forward(
            A.m, A.v, A.g, [&](int64_t idx, uint32_t& ok) { return edit_load8(T, n, idx, ok); },
            [&](int64_t idx, uint32_t& ok) { return edit_load8(A.Q, A.m, idx, ok); },
            [&](uint64_t r, uint32_t D0, uint32_t VP) { mine[(r - 1) * cr] = make_uint2(D0, VP); });
        uint32_t nr = 0;
        uint64_t st = 0;
        if (score != A.v) atomicMin(&sc[TR_BAD], (unsigned long long)t);
        else
            st = trace_walk(
                A.m, A.v, A.g, [&](uint64_t r, uint32_t& D0, uint32_t& VP) { const uint2 w = mine[(r - 1) * cr]; D0 = w.x; VP = w.y; },
                [&](uint64_t i) { return A.Q[i]; }, [&](uint64_t j) { return T[j]; }, [&](uint32_t, uint32_t) {}, nr);
        start[t] = st;
        nruns[lr] = nr;
        cnt[0] = nr;
    }
    wg_scan(cnt, tot, s_w);
    if (lr < cr) cigar_off[t] = cnt[0];
    if (threadIdx.x == 0) wgsum[blockIdx.x] = tot[0];
}

// the same records after k_locate_scan over wgsum: the offsets made global, the runs; chunk c reads the base of word c & 1 and
// leaves the next chunk's in the other word
__global__ __launch_bounds__(256) void k_trace_write(const uint8_t* __restrict__ T, TraceRecs R, const uint8_t* __restrict__ q,
                                                     const uint64_t* __restrict__ qoff, uint64_t g0, uint32_t both, uint64_t c0, uint64_t cr,
                                                     const uint2* __restrict__ rows, const uint32_t* __restrict__ nruns,
                                                     const uint64_t* __restrict__ wgbase, uint32_t slot, uint64_t* __restrict__ cigar_off,
                                                     uint32_t* __restrict__ cigar, uint64_t cap, unsigned long long* __restrict__ sc)
{
    const uint64_t lr = (uint64_t)blockIdx.x * 256 + threadIdx.x, t = c0 + lr;
    const uint64_t base = sc[TR_BASE0 + slot];
    if (lr == 0) sc[TR_BASE0 + (slot ^ 1u)] = base + sc[TR_CHUNK];
    if (lr >= cr) return;
    const uint64_t off = base + wgbase[blockIdx.x] + cigar_off[t];
    cigar_off[t] = off;
    const uint32_t nr = nruns[lr];
    if (!cigar || !nr || off >= cap) return;
    const TraceQuery A = trace_query(R, t, q, qoff, g0, both);
    const uint2* __restrict__ mine = rows + lr;
    uint64_t at = off + nr;
    uint32_t again;
    (void)trace_walk(
        A.m, A.v, A.g, [&](uint64_t r, uint32_t& D0, uint32_t& VP) { const uint2 w = mine[(r - 1) * cr]; D0 = w.x; VP = w.y; },
        [&](uint64_t i) { return A.Q[i]; }, [&](uint64_t j) { return T[j]; },
        [&](uint32_t op, uint32_t len) { at--; if (at < cap) cigar[at] = len << 4 | op; }, again);
}

}  // namespace sufr

extern "C" {

int sufr_hip_set_trace_scratch(sufr_hip_ctx* ctx, uint64_t bytes)
{
    if (!ctx) return SUFR_HIP_E_INVALID;
    ctx->trace_scratch = bytes;
    return 0;
}

int sufr_hip_edit_trace_device(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_queries, const void* d_offsets,
                               uint64_t num_queries, uint64_t num_records, const void* d_query, const void* d_strand, const void* d_end,
                               const void* d_edits, uint64_t cigar_cap, void* d_start, void* d_cigar_off, void* d_cigar,
                               uint64_t* total_out)
{
    if (total_out) *total_out = 0;
    if (!ctx || !ix || !d_cigar_off || (cigar_cap && !d_cigar)) return SUFR_HIP_E_INVALID;
    if (num_records && (!d_query || !d_strand || !d_end || !d_edits || !d_start)) return SUFR_HIP_E_INVALID;
    sufr::Pipeline& pl = ctx->pl;
    pl.err.clear();
    int rc;
    if ((rc = query_check(ctx, ix))) return rc;                      // (the text alone is read: a seed-mask index is as good as any)
    if (!num_records) {
        if (hipMemsetAsync(d_cigar_off, 0, 8, pl.stream) != hipSuccess) { pl.set_error("trace: hipMemsetAsync failed"); return SUFR_HIP_E_HIP; }
        return 0;
    }
    if (!num_queries || !d_queries || !d_offsets) {
        pl.set_error("trace: record 0 names a query of an empty batch");
        return SUFR_HIP_E_INVALID;
    }
    const sufr::TraceRecs R{(const uint64_t*)d_query, (const uint8_t*)d_strand, (const uint64_t*)d_end, (const uint8_t*)d_edits, num_records};
    const uint64_t* uoff = (const uint64_t*)d_offsets;
    // the scalars; the checks that need no table, the longest query, the byte range of the batch
    if ((rc = pl.ensure(ctx->tsc, sufr::TR_N * 8))) return rc;
    unsigned long long* sc = (unsigned long long*)ctx->tsc.p;
    if (hipMemsetAsync(sc, 0, sufr::TR_N * 8, pl.stream) != hipSuccess || hipMemsetAsync(sc + sufr::TR_BAD, 0xFF, 8, pl.stream) != hipSuccess) {
        pl.set_error("trace: hipMemsetAsync failed");
        return SUFR_HIP_E_HIP;
    }
    hipLaunchKernelGGL(sufr::k_trace_check, dim3((uint32_t)((num_records + 255) / 256)), dim3(256), 0, pl.stream, R, uoff, num_queries,
                       ix->ix.n, sc);
    unsigned long long h[sufr::TR_N];
    if ((rc = read_totals(pl, sc, sufr::TR_N, h, "trace", "checking the records failed"))) return rc;
    if (h[sufr::TR_BAD] != ~0ull) {
        pl.set_error("trace: record " + std::to_string(h[sufr::TR_BAD]) + " is no record of this batch and text (query, strand, end, edits "
                     "or the length of its query out of range)");
        return SUFR_HIP_E_INVALID;
    }
    // the chunks: 8 bytes per row of the longest query and record
    const uint64_t max_m = h[sufr::TR_MAXM], budget = ctx->trace_scratch ? ctx->trace_scratch : sufr::TRACE_SCRATCH_DEFAULT;
    uint64_t cr = budget / (8 * max_m) / 64 * 64;
    if (cr < 64) {
        pl.set_error("trace: the rows of 64 records of a query of " + std::to_string(max_m) + " bytes take " + std::to_string(64 * 8 * max_m) +
                     " bytes; the row storage is " + std::to_string(budget) + " bytes (sufr_hip_set_trace_scratch)");
        return SUFR_HIP_E_NOMEM;
    }
    if (cr > sufr::TRACE_CHUNK_MAX) cr = sufr::TRACE_CHUNK_MAX;
    if (cr > (num_records + 63) / 64 * 64) cr = (num_records + 63) / 64 * 64;
    const uint64_t max_wgs = (cr + 255) / 256;
    if ((rc = pl.ensure(ctx->trows, cr * 8 * max_m)) || (rc = pl.ensure(ctx->tmisc, cr * 4 + (max_wgs + 1) * 8))) return rc;
    uint64_t* wgsum = (uint64_t*)ctx->tmisc.p;
    uint32_t* nruns = (uint32_t*)(wgsum + max_wgs + 1);
    // strand 1: the doubled batch (offsets from 0); else the batch as it is, read from its first byte
    QueryBatch b{(const uint8_t*)d_queries, uoff, num_queries, h[sufr::TR_GEND] - h[sufr::TR_G0], batch_grid(pl), false};
    uint64_t g0 = 0;
    if (h[sufr::TR_STRAND1]) { if ((rc = double_batch(ctx, b))) return rc; }
    else { g0 = h[sufr::TR_G0]; b.q += g0; }
    uint32_t slot = 0;
    for (uint64_t c0 = 0; c0 < num_records; c0 += cr, slot ^= 1u) {
        const uint64_t n_here = num_records - c0 < cr ? num_records - c0 : cr;
        const uint32_t wgs = (uint32_t)((n_here + 255) / 256);
        hipLaunchKernelGGL(sufr::k_trace_rows, dim3(wgs), dim3(256), 0, pl.stream, ix->ix.text, ix->ix.n, R, b.q, b.qoff, g0, (uint32_t)b.both, c0, n_here,
                           (uint2*)ctx->trows.p, (uint64_t*)d_start, nruns, (uint64_t*)d_cigar_off, wgsum, sc);
        hipLaunchKernelGGL(sufr::k_locate_scan, dim3(1), dim3(1024), 0, pl.stream, wgsum, (uint64_t)wgs, (uint64_t*)(sc + sufr::TR_CHUNK));
        hipLaunchKernelGGL(sufr::k_trace_write, dim3(wgs), dim3(256), 0, pl.stream, ix->ix.text, R, b.q, b.qoff, g0, (uint32_t)b.both, c0, n_here,
                           (const uint2*)ctx->trows.p, (const uint32_t*)nruns, (const uint64_t*)wgsum, slot, (uint64_t*)d_cigar_off,
                           (uint32_t*)d_cigar, cigar_cap, sc);
    }
    if ((rc = launch_status(pl, "trace"))) return rc;
    if (hipMemcpyAsync((uint64_t*)d_cigar_off + num_records, sc + sufr::TR_BASE0 + slot, 8, hipMemcpyDeviceToDevice, pl.stream) != hipSuccess) {
        pl.set_error("trace: hipMemcpyAsync failed");
        return SUFR_HIP_E_HIP;
    }
    if ((rc = read_totals(pl, sc, sufr::TR_N, h, "trace", "reading the CIGAR total failed"))) return rc;
    if (h[sufr::TR_BAD] != ~0ull) {
        pl.set_error("trace: record " + std::to_string(h[sufr::TR_BAD]) + ": edits is not D(end + 1)");
        return SUFR_HIP_E_INVALID;
    }
    const uint64_t total = h[sufr::TR_BASE0 + slot];
    if (pl.debug) fprintf(stderr, "[sufr_hip debug] trace: %llu records, longest query %llu, %llu per chunk, %llu runs\n",
                          (unsigned long long)num_records, (unsigned long long)max_m, (unsigned long long)cr, (unsigned long long)total);
    return records_fit(pl, "trace", "CIGAR runs", total, cigar_cap, total_out);
}

int sufr_hip_edit_trace(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const uint8_t* queries, const uint64_t* offsets, uint64_t num_queries,
                        uint64_t num_records, const uint64_t* query, const uint8_t* strand, const uint64_t* end, const uint8_t* edits,
                        uint64_t cigar_cap, uint64_t* start, uint64_t* cigar_off, uint32_t* cigar, uint64_t* total_out)
{
    if (total_out) *total_out = 0;
    if (!ctx || !ix || !cigar_off || (cigar_cap && !cigar) || (num_queries && !offsets)) return SUFR_HIP_E_INVALID;
    if (num_records && (!query || !strand || !end || !edits || !start)) return SUFR_HIP_E_INVALID;
    ctx->pl.err.clear();
    if (const int rc = query_check(ctx, ix)) return rc;
    cigar_off[0] = 0;
    if (!num_records) return 0;
    if (!num_queries) { ctx->pl.set_error("trace: record 0 names a query of an empty batch"); return SUFR_HIP_E_INVALID; }
    const uint64_t qbytes = offsets[num_queries], obytes = (num_queries + 1) * 8, nr = num_records;
    // one allocation: queries | offsets | query, end | start, cigar_off | cigar | strand, edits
    const uint64_t o_at = (qbytes + 7) / 8 * 8, q_at = o_at + obytes, end_at = q_at + nr * 8, s_at = end_at + nr * 8, co_at = s_at + nr * 8,
                   cg_at = co_at + (nr + 1) * 8, st_at = cg_at + (cigar_cap + 1) / 2 * 8, ed_at = st_at + nr;
    uint8_t* d;
    hipStream_t s = ctx->pl.stream;
    int rc = stage_batch(ctx, "trace", queries, offsets, num_queries, o_at, ed_at + nr + 8, &d);
    if (!rc && (hipMemcpyAsync(d + q_at, query, nr * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
                hipMemcpyAsync(d + end_at, end, nr * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
                hipMemcpyAsync(d + st_at, strand, nr, hipMemcpyHostToDevice, s) != hipSuccess ||
                hipMemcpyAsync(d + ed_at, edits, nr, hipMemcpyHostToDevice, s) != hipSuccess)) rc = SUFR_HIP_E_HIP;
    uint64_t total = 0;
    if (!rc) rc = sufr_hip_edit_trace_device(ctx, ix, d, d + o_at, num_queries, nr, d + q_at, d + st_at, d + end_at, d + ed_at, cigar_cap,
                                             d + s_at, d + co_at, cigar_cap ? d + cg_at : nullptr, &total);
    if (total_out) *total_out = total;
    // start and cigar_off are complete with a capacity error too; the runs only when they all fit
    if (rc == SUFR_HIP_E_CAPACITY) {
        if (hipMemcpyAsync(start, d + s_at, nr * 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipMemcpyAsync(cigar_off, d + co_at, (nr + 1) * 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess) { ctx->pl.set_error("copying the trace batch failed"); rc = SUFR_HIP_E_HIP; }
        (void)hipFree(d);
        return rc;
    }
    return unstage_batch(ctx, "trace", d, rc, {{start, s_at, nr * 8}, {cigar_off, co_at, (nr + 1) * 8}, {cigar, cg_at, total * 4}});
}

}  // extern "C"
