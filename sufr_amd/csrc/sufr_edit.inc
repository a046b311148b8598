// sufr_edit.inc -- k-difference (edit distance) search of a query batch on a device-resident index: pigeonhole seeds, a
// bit-parallel banded Sellers table per candidate, a radix sort and a unique step over the reported ends (included by
// sufr_kernels.hip after sufr_approx.inc; include/sufr_edit.h, DESIGN.md section 16).
//
// batch_extent / double_batch (sufr_search.inc) the ends of the batch (a synchronisation of its own); the sort-key check sits between
//                    the two; the doubled batch with both strands
// pigeonhole_candidates (sufr_approx.inc) k_approx_seeds, then the candidate starts; first synchronisation: their total
// k_edit_count       SCAN_WGS workgroups over the candidates, 8 per lane (approx_walk8): candidate -> seed, diagonal
//                    p = SA[..] - o_i; the pre-filter (a lower live piece whose seed matches at an indexed position on the
//                    same diagonal has the same band: it reports); the band; the ends of [p + m - d, p + m + d] that pass,
//                    counted per candidate (one byte each) and per workgroup
// scan_total         (sufr_search.inc) k_locate_scan: the emission total (second synchronisation) and the workgroup bases
// k_edit_emit        the band again for the candidates that counted an end; the packed keys
// sort_keys          (below) LSD radix sort over the key bits that vary
// k_key_count / k_key_compact <KEY_UNIQUE>   the first key of every run of equal (query, strand, end): third synchronisation
// k_key_count / k_key_compact <KEY_MINIMA>   SUFR_EDIT_LOCAL_MINIMA: the keys no neighbour beats; one more synchronisation
// k_edit_records     the four record arrays from the keys
// No MFMA, no scratch; LDS: the scan words, the 256 counters and offsets of a radix pass.
//
// A key is ((a << eb) | e) << 4 | D(e): a the query (2 * query + strand with both strands), e the exclusive end (1 .. n, so
// that e - 1 and e + 1 of a key never collide with a key of another query), eb the bit width of n.

namespace sufr {

static constexpr uint32_t EDIT_VAL_BITS = 4;           // D(e) <= 15

// ---- the band of one candidate -----------------------------------------------------------------------------------------
// Row r (r query bytes consumed) holds the W = 4d + 1 cells of the columns p + r - 2d + k (text bytes consumed), k = 0 .. W - 1.
// A cell reads its diagonal neighbour (r - 1, k), the cell above (r - 1, k + 1) and the cell to its left (r, k - 1); outside
// the band is +inf.  Myers' recurrences on the horizontal deltas of a row, bit k: the delta between cells k and k + 1
// (P: +1, N: -1); the band moves one column per row, so the diagonal vector is shifted down instead of the deltas being
// shifted up (Hyyro's banded form).  s0 is the value of cell 0.  Text bytes outside [0, n) match nothing, which gives column
// 0 its value r and the columns beyond n values nobody reads.  The match vector comes from nine sliding bit-planes of the
// text window (eight byte bits and `valid`), one push per row.
struct EditBand { uint64_t P, N; uint32_t s0; };

// eight bytes of T from idx on (0 where outside [0, n)); ok: bit j set when byte j is inside
__device__ __forceinline__ uint64_t edit_load8(const uint8_t* __restrict__ T, uint64_t n, int64_t idx, uint32_t& ok)
{
    uint64_t w = 0;
    if (idx >= 0 && (uint64_t)idx + 8 <= n) { __builtin_memcpy(&w, T + idx, 8); ok = 0xFFu; return w; }
    ok = 0;
#pragma unroll
    for (int j = 0; j < 8; j++)
        if ((uint64_t)(idx + j) < n) { w |= (uint64_t)T[idx + j] << (8 * j); ok |= 1u << j; }
    return w;
}

// false: every cell of some row is above d, so no end of this band passes
__device__ __forceinline__ bool edit_band(const uint8_t* __restrict__ Q, uint64_t m, const uint8_t* __restrict__ T, uint64_t n, int64_t p,
                                          uint32_t d, EditBand& out)
{
    const uint32_t W = 4 * d + 1;
    const uint64_t top = 1ull << (W - 1), wmask = top | (top - 1);
    uint64_t pl[8] = {0, 0, 0, 0, 0, 0, 0, 0}, valid = 0;
    auto push = [&](uint32_t byte, uint32_t ok) {
#pragma unroll
        for (int b = 0; b < 8; b++) pl[b] = (pl[b] >> 1) | ((byte >> b) & 1u ? top : 0ull);
        valid = (valid >> 1) | (ok ? top : 0ull);
    };
    // the window of row 1 but for its last byte: T[p - 2d .. p + 2d)
    for (uint32_t k = 0; k + 1 < W; k += 8) {
        uint32_t ok;
        const uint64_t w = edit_load8(T, n, p - 2 * (int64_t)d + k, ok);
#pragma unroll
        for (uint32_t j = 0; j < 8; j++)
            if (k + j + 1 < W) push((uint32_t)(w >> (8 * j)) & 0xFFu, (ok >> j) & 1u);
    }
    uint64_t P = 0, N = 0;
    uint32_t s0 = 0;
    for (uint64_t r0 = 0; r0 < m; r0 += 8) {
        uint32_t ok, qok;
        const uint64_t tw = edit_load8(T, n, p + (int64_t)r0 + 2 * (int64_t)d, ok);
        const uint64_t qw = edit_load8(Q, m, (int64_t)r0, qok);
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) {
            if (r0 + j < m) {
                push((uint32_t)(tw >> (8 * j)) & 0xFFu, (ok >> j) & 1u);
                const uint32_t qc = (uint32_t)(qw >> (8 * j)) & 0xFFu;
                uint64_t eq = valid;
#pragma unroll
                for (int b = 0; b < 8; b++) eq &= ~(pl[b] ^ (0ull - (uint64_t)((qc >> b) & 1u)));
                const uint64_t X = eq | N;
                const uint64_t D0 = ((((X & P) + P) ^ P) | X) & wmask;
                const uint64_t VP = N | ~(D0 | P), VN = D0 & P, Xs = D0 >> 1;
                N = Xs & VP;
                P = (VN | ~(Xs | VP)) & wmask;
                s0 += (uint32_t)(~D0 & 1ull);
            }
        }
        // every cell of the row above d: so is every later row (values do not fall along a diagonal)
        uint32_t v = s0, mn = s0;
        for (uint32_t k = 0; k + 1 < W; k++) { v += (uint32_t)((P >> k) & 1ull) - (uint32_t)((N >> k) & 1ull); mn = v < mn ? v : mn; }
        if (mn > d) return false;
    }
    out.P = P; out.N = N; out.s0 = s0;
    return true;
}

// candidate c of seed g: bit j of the result is set when the exclusive end e0 + j passes (j = 0 .. 2d), vals: 4 bits per
// passing end, in order of j (at most 31 ends: two words)
__device__ __forceinline__ uint32_t edit_verify(const SearchIndex& ix, const ApproxBatch& B, uint64_t g, uint64_t c, int64_t& e0,
                                                uint64_t (&vals)[2])
{
    const uint64_t a = g / B.np, i = g - a * B.np, b = B.qoff[a], m = B.qoff[a + 1] - b;
    const uint64_t o = approx_piece(i, m, B.np);
    const int64_t p = (int64_t)ix.suffix(B.rlo[g] + (c - B.cand[g])) - (int64_t)o;
    const uint8_t* __restrict__ Q = B.q + b;
    // a lower live piece whose seed matches at an indexed position of this diagonal walks the same band: it reports
    uint64_t oj = 0;
    for (uint64_t j = 0; j < i; j++) {
        const uint64_t on = approx_piece(j + 1, m, B.np), len = on - oj, kk = B.L > 0 && B.L < len ? B.L : len;
        const int64_t pj = p + (int64_t)oj;
        if (pj >= 0 && (uint64_t)pj + kk <= ix.n && B.rlo[g - i + j] != APPROX_DEAD &&
            (!B.bits || ((B.bits[(uint64_t)pj >> 5] >> ((uint64_t)pj & 31)) & 1u)) &&
            common_prefix<uint64_t>(Q + oj, ix.text + pj, 0, kk) == kk) return 0;
        oj = on;
    }
    EditBand band;
    if (!edit_band(Q, m, ix.text, ix.n, p, B.d, band)) return 0;
    e0 = p + (int64_t)m - (int64_t)B.d;
    const uint64_t lowd = (1ull << B.d) - 1;
    uint32_t v = band.s0 + (uint32_t)__popcll(band.P & lowd) - (uint32_t)__popcll(band.N & lowd), mask = 0, at = 0;
    vals[0] = vals[1] = 0;
    for (uint32_t j = 0; j <= 2 * B.d; j++) {                        // cell d + j of the last row
        const int64_t e = e0 + j;
        if (e >= 1 && (uint64_t)e <= ix.n && v <= B.d) {
            mask |= 1u << j;
            if (at < 16) vals[0] |= (uint64_t)v << (4 * at); else vals[1] |= (uint64_t)v << (4 * (at - 16));
            at++;
        }
        v += (uint32_t)((band.P >> (B.d + j)) & 1ull) - (uint32_t)((band.N >> (B.d + j)) & 1ull);
    }
    return mask;
}

__global__ __launch_bounds__(256) void k_edit_count(SearchIndex ix, ApproxBatch B, uint8_t* __restrict__ cnt8, uint64_t* __restrict__ cnt_sum)
{
    __shared__ uint64_t s_w[4];
    const uint64_t total = B.cand[B.ns], chunk = scan_chunk(total);
    const uint64_t lo = (uint64_t)blockIdx.x * chunk, hi = lo + chunk < total ? lo + chunk : total;
    uint64_t acc = 0;
    for (uint64_t t = lo; t < hi; t += LOC_BLK) {
        const uint64_t c = t + (uint64_t)threadIdx.x * 8;
        uint64_t cnt[1] = {0}, tot[1];
        approx_walk8(B, c, hi, [&](uint32_t k, uint64_t g) {
            int64_t e0;
            uint64_t vals[2];
            const uint32_t n1 = (uint32_t)__popc(edit_verify(ix, B, g, c + k, e0, vals));
            cnt8[c + k] = (uint8_t)n1;
            cnt[0] += n1;
        });
        wg_scan(cnt, tot, s_w);
        acc += tot[0];
    }
    if (threadIdx.x == 0) cnt_sum[blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void k_edit_emit(SearchIndex ix, ApproxBatch B, const uint8_t* __restrict__ cnt8,
                                                   const uint64_t* __restrict__ cnt_base, uint32_t eb, uint64_t* __restrict__ keys)
{
    __shared__ uint64_t s_w[4];
    const uint64_t total = B.cand[B.ns], chunk = scan_chunk(total);
    const uint64_t lo = (uint64_t)blockIdx.x * chunk, hi = lo + chunk < total ? lo + chunk : total;
    uint64_t run = cnt_base[blockIdx.x];
    for (uint64_t t = lo; t < hi; t += LOC_BLK) {
        const uint64_t c = t + (uint64_t)threadIdx.x * 8;
        uint64_t cnt[1] = {0}, tot[1];
        for (uint32_t k = 0; k < 8 && c + k < hi; k++) cnt[0] += cnt8[c + k];
        const bool any = cnt[0] != 0;
        wg_scan(cnt, tot, s_w);
        uint64_t at = run + cnt[0];
        if (any) {
            approx_walk8(B, c, hi, [&](uint32_t k, uint64_t g) {
                if (!cnt8[c + k]) return;
                int64_t e0;
                uint64_t vals[2];
                const uint32_t mask = edit_verify(ix, B, g, c + k, e0, vals);
                const uint64_t a = g / B.np;
                uint32_t nth = 0;
                for (uint32_t j = 0; j <= 2 * B.d; j++) {
                    if (!((mask >> j) & 1u)) continue;
                    const uint64_t v = (nth < 16 ? vals[0] >> (4 * nth) : vals[1] >> (4 * (nth - 16))) & 15u;
                    keys[at++] = (((a << eb) | (uint64_t)(e0 + j)) << EDIT_VAL_BITS) | v;
                    nth++;
                }
            });
        }
        run += tot[0];
    }
}

// ---- sort_keys: LSD radix sort of 64-bit keys over the bits [lo_bit, hi_bit) --------------------------------------------
// A general key sort (the k_group_sort_* kernels of the build sort suffix records in place and know what a suffix is).  One
// pass per 8-bit digit, stable, between two buffers of n keys:
//   k_sort_hist     SCAN_WGS workgroups, workgroup b over keys [b * chunk, (b + 1) * chunk): its 256 digit counts, in LDS,
//                   then digit-major into hist[digit * SCAN_WGS + b]
//   k_locate_scan   the exclusive scan of hist in that order: where every workgroup's keys of every digit go
//   k_sort_scatter  the same chunks in tiles of 256 keys, one per lane: a lane finds the lanes of its wave with its digit by
//                   eight ballots, its rank among them by a popcount; the waves' counts go through LDS, so that a tile keeps
//                   its order; the offsets of the workgroup advance tile by tile
// hist: 256 * SCAN_WGS + 1 words.  Returns the buffer that holds the sorted keys (a or b); the passes are enqueued on the
// stream, nothing is synchronised.
__global__ __launch_bounds__(256) void k_sort_hist(const uint64_t* __restrict__ keys, uint64_t n, uint32_t shift, uint32_t dmask,
                                                   uint64_t* __restrict__ hist)
{
    __shared__ uint32_t s_h[256];
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t chunk = scan_chunk(n), lo = (uint64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    for (uint64_t j = lo + threadIdx.x; j < hi; j += 256) atomicAdd(&s_h[(uint32_t)(keys[j] >> shift) & dmask], 1u);
    __syncthreads();
    hist[(uint64_t)threadIdx.x * SCAN_WGS + blockIdx.x] = s_h[threadIdx.x];
}

__global__ __launch_bounds__(256) void k_sort_scatter(const uint64_t* __restrict__ in, uint64_t n, uint32_t shift, uint32_t dmask,
                                                      const uint64_t* __restrict__ hist, uint64_t* __restrict__ out)
{
    __shared__ uint64_t s_off[256];
    __shared__ uint32_t s_cnt[4][256];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    s_off[threadIdx.x] = hist[(uint64_t)threadIdx.x * SCAN_WGS + blockIdx.x];
    for (int k = 0; k < 4; k++) s_cnt[k][threadIdx.x] = 0;
    __syncthreads();
    const uint64_t chunk = scan_chunk(n), lo = (uint64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    for (uint64_t t = lo; t < hi; t += 256) {
        const uint64_t j = t + threadIdx.x;
        const bool act = j < hi;
        const uint64_t key = act ? in[j] : 0;
        const uint32_t dg = (uint32_t)(key >> shift) & dmask;
        uint64_t peers = __ballot(act);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool bit = (dg >> b) & 1u;
            const uint64_t bal = __ballot(act && bit);
            peers &= bit ? bal : ~bal;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1));
        if (act && rank == 0) s_cnt[w][dg] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (act) {
            uint64_t base = s_off[dg];
            for (uint32_t k = 0; k < w; k++) base += s_cnt[k][dg];
            out[base + rank] = key;
        }
        __syncthreads();
        uint32_t sum = 0;
        for (int k = 0; k < 4; k++) { sum += s_cnt[k][threadIdx.x]; s_cnt[k][threadIdx.x] = 0; }
        s_off[threadIdx.x] += sum;
        __syncthreads();
    }
}

static uint64_t* sort_keys(hipStream_t stream, uint64_t* a, uint64_t* b, uint64_t n, uint32_t lo_bit, uint32_t hi_bit, uint64_t* hist)
{
    for (uint32_t shift = lo_bit; shift < hi_bit; shift += 8) {
        const uint32_t bits = hi_bit - shift < 8 ? hi_bit - shift : 8, dmask = (1u << bits) - 1;
        hipLaunchKernelGGL(k_sort_hist, dim3(SCAN_WGS), dim3(256), 0, stream, (const uint64_t*)a, n, shift, dmask, hist);
        hipLaunchKernelGGL(k_locate_scan, dim3(1), dim3(1024), 0, stream, hist, (uint64_t)256 * SCAN_WGS, hist + 256 * SCAN_WGS);
        hipLaunchKernelGGL(k_sort_scatter, dim3(SCAN_WGS), dim3(256), 0, stream, (const uint64_t*)a, n, shift, dmask, (const uint64_t*)hist, b);
        uint64_t* t = a; a = b; b = t;
    }
    return a;
}

// ---- what stays of the sorted keys --------------------------------------------------------------------------------------
enum { KEY_UNIQUE = 0, KEY_MINIMA = 1 };

// KEY_UNIQUE: key j opens a run of equal (a, e).  KEY_MINIMA (unique keys): D(e - 1) > D(e) and D(e + 1) >= D(e), a
// neighbour that is no key counting as d + 1
template <int MODE>
__device__ __forceinline__ bool key_keep(const uint64_t* __restrict__ keys, uint64_t j, uint64_t n, uint32_t d)
{
    const uint64_t sk = keys[j] >> EDIT_VAL_BITS;
    if (MODE == KEY_UNIQUE) return j == 0 || (keys[j - 1] >> EDIT_VAL_BITS) != sk;
    const uint32_t v = (uint32_t)keys[j] & 15u;
    uint32_t vl = d + 1, vr = d + 1;
    if (j > 0 && (keys[j - 1] >> EDIT_VAL_BITS) + 1 == sk) vl = (uint32_t)keys[j - 1] & 15u;
    if (j + 1 < n && (keys[j + 1] >> EDIT_VAL_BITS) == sk + 1) vr = (uint32_t)keys[j + 1] & 15u;
    return vl > v && vr >= v;
}

template <int MODE>
__global__ __launch_bounds__(256) void k_key_count(const uint64_t* __restrict__ keys, uint64_t n, uint32_t d, uint64_t* __restrict__ sums)
{
    __shared__ uint64_t s_w[4];
    const uint64_t chunk = scan_chunk(n), lo = (uint64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    uint64_t acc = 0;
    for (uint64_t t = lo; t < hi; t += LOC_BLK) {
        const uint64_t c = t + (uint64_t)threadIdx.x * 8;
        uint64_t cnt[1] = {0}, tot[1];
        for (uint32_t k = 0; k < 8 && c + k < hi; k++) cnt[0] += key_keep<MODE>(keys, c + k, n, d);
        wg_scan(cnt, tot, s_w);
        acc += tot[0];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = acc;
}

template <int MODE>
__global__ __launch_bounds__(256) void k_key_compact(const uint64_t* __restrict__ keys, uint64_t n, uint32_t d,
                                                     const uint64_t* __restrict__ bases, uint64_t* __restrict__ out)
{
    __shared__ uint64_t s_w[4];
    const uint64_t chunk = scan_chunk(n), lo = (uint64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    uint64_t run = bases[blockIdx.x];
    for (uint64_t t = lo; t < hi; t += LOC_BLK) {
        const uint64_t c = t + (uint64_t)threadIdx.x * 8;
        uint32_t keep = 0;
        for (uint32_t k = 0; k < 8 && c + k < hi; k++) keep |= (uint32_t)key_keep<MODE>(keys, c + k, n, d) << k;
        uint64_t cnt[1] = {(uint64_t)__popc(keep)}, tot[1];
        wg_scan(cnt, tot, s_w);
        uint64_t at = run + cnt[0];
        for (uint32_t k = 0; k < 8; k++) if ((keep >> k) & 1u) out[at++] = keys[c + k];
        run += tot[0];
    }
}

__global__ __launch_bounds__(256) void k_edit_records(const uint64_t* __restrict__ keys, uint64_t n, uint32_t eb, uint32_t both,
                                                      uint64_t* __restrict__ out_query, uint8_t* __restrict__ out_strand,
                                                      uint64_t* __restrict__ out_end, uint8_t* __restrict__ out_edits)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += stride) {
        const uint64_t key = keys[j], sk = key >> EDIT_VAL_BITS, a = sk >> eb;
        out_query[j] = both ? a >> 1 : a;
        out_strand[j] = (uint8_t)(both ? a & 1 : 0);
        out_end[j] = (sk & ((1ull << eb) - 1)) - 1;
        out_edits[j] = (uint8_t)(key & 15u);
    }
}

}  // namespace sufr

namespace {

int edit_args(sufr_hip_ctx* ctx, const sufr_hip_index* ix, uint32_t max_edits)
{
    if (const int rc = query_check(ctx, ix, "k-difference searches")) return rc;
    if (max_edits > SUFR_EDIT_MAX_EDITS) {
        ctx->pl.set_error("edit: max_edits must be at most " + std::to_string(SUFR_EDIT_MAX_EDITS));
        return SUFR_HIP_E_INVALID;
    }
    return 0;
}

uint32_t bit_width_u64(uint64_t v) { uint32_t b = 0; while (v) { b++; v >>= 1; } return b; }

}  // namespace

extern "C" {

int sufr_hip_edit_device(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_queries, const void* d_offsets,
                         uint64_t num_queries, uint32_t max_edits, uint64_t max_occ, uint32_t flags, uint64_t cap, void* d_query,
                         void* d_strand, void* d_end, void* d_edits, uint64_t* total_out)
{
    if (total_out) *total_out = 0;
    if (!ctx || !ix || (num_queries && (!d_queries || !d_offsets))) return SUFR_HIP_E_INVALID;
    sufr::Pipeline& pl = ctx->pl;
    pl.err.clear();
    int rc;
    if ((rc = edit_args(ctx, ix, max_edits))) return rc;
    QueryBatch b;
    if ((rc = batch_extent(ctx, ix, d_queries, d_offsets, num_queries, "edit", b)) || !b.nb) return rc;
    // the sort key: query (and strand) above the exclusive end above the distance; checked before the batch is doubled
    const bool both = (flags & SUFR_EDIT_BOTH_STRANDS) != 0;
    const uint64_t nq = num_queries * (both ? 2 : 1);
    const uint32_t eb = bit_width_u64(ix->ix.n), ab = bit_width_u64(nq - 1);
    if (eb + ab + sufr::EDIT_VAL_BITS > 64) {
        pl.set_error("edit: " + std::to_string(nq) + " queries on a text of " + std::to_string(ix->ix.n) + " bytes need a sort key of " +
                     std::to_string(eb + ab + sufr::EDIT_VAL_BITS) + " bits; 64 are sorted");
        return SUFR_HIP_E_UNSUPPORTED;
    }
    if (both && (rc = double_batch(ctx, b))) return rc;
    sufr::ApproxBatch B;
    Candidates c;
    if ((rc = pigeonhole_candidates(ctx, ix, b, max_edits, max_occ, "edit", B, c)) || !c.ncand) return rc;
    // the ends every candidate reports, counted per candidate and per workgroup, then the emission total
    if ((rc = pl.ensure(ctx->ecnt, c.ncand))) return rc;
    uint64_t* cnt_sum = c.cnt_sum;
    hipLaunchKernelGGL(sufr::k_edit_count, dim3(sufr::SCAN_WGS), dim3(256), 0, pl.stream, ix->ix, B, (uint8_t*)ctx->ecnt.p, cnt_sum);
    unsigned long long nemit = 0;
    if ((rc = scan_total(pl, cnt_sum, sufr::SCAN_WGS, &nemit, "edit", "counting the reported ends failed")) || !nemit) return rc;
    // the keys, sorted over the bits that vary, and the first of every run
    if ((rc = pl.ensure(ctx->ekeys, nemit * 8)) || (rc = pl.ensure(ctx->ekeys2, nemit * 8)) ||
        (rc = pl.ensure(ctx->ehist, ((uint64_t)256 * sufr::SCAN_WGS + 1) * 8))) return rc;
    uint64_t* ka = (uint64_t*)ctx->ekeys.p;
    uint64_t* kb = (uint64_t*)ctx->ekeys2.p;
    hipLaunchKernelGGL(sufr::k_edit_emit, dim3(sufr::SCAN_WGS), dim3(256), 0, pl.stream, ix->ix, B, (const uint8_t*)ctx->ecnt.p,
                       (const uint64_t*)cnt_sum, eb, ka);
    uint64_t* sorted = sufr::sort_keys(pl.stream, ka, kb, nemit, sufr::EDIT_VAL_BITS, sufr::EDIT_VAL_BITS + eb + ab, (uint64_t*)ctx->ehist.p);
    uint64_t* other = sorted == ka ? kb : ka;
    hipLaunchKernelGGL(sufr::k_key_count<sufr::KEY_UNIQUE>, dim3(sufr::SCAN_WGS), dim3(256), 0, pl.stream, (const uint64_t*)sorted,
                       (uint64_t)nemit, max_edits, cnt_sum);
    unsigned long long nrec = 0;
    if ((rc = scan_total(pl, cnt_sum, sufr::SCAN_WGS, &nrec, "edit", "counting the records failed"))) return rc;
    const uint64_t* recs = sorted;                                   // (all of them distinct: nothing to move)
    if (nrec < nemit) {
        hipLaunchKernelGGL(sufr::k_key_compact<sufr::KEY_UNIQUE>, dim3(sufr::SCAN_WGS), dim3(256), 0, pl.stream, (const uint64_t*)sorted,
                           (uint64_t)nemit, max_edits, (const uint64_t*)cnt_sum, other);
        recs = other;
        other = sorted;
    }
    if (flags & SUFR_EDIT_LOCAL_MINIMA) {
        const uint64_t nuniq = nrec;
        hipLaunchKernelGGL(sufr::k_key_count<sufr::KEY_MINIMA>, dim3(sufr::SCAN_WGS), dim3(256), 0, pl.stream, recs, nuniq, max_edits, cnt_sum);
        if ((rc = scan_total(pl, cnt_sum, sufr::SCAN_WGS, &nrec, "edit", "counting the local minima failed"))) return rc;
        if (nrec <= cap && nrec) {
            hipLaunchKernelGGL(sufr::k_key_compact<sufr::KEY_MINIMA>, dim3(sufr::SCAN_WGS), dim3(256), 0, pl.stream, recs, nuniq, max_edits,
                               (const uint64_t*)cnt_sum, other);
            recs = other;
        }
    }
    if (pl.debug) fprintf(stderr, "[sufr_hip debug] edit: d=%u max_occ=%llu flags=%u: %llu seeds, %llu candidates, %llu reported ends, %llu records\n",
                          max_edits, (unsigned long long)max_occ, flags, (unsigned long long)B.ns, c.ncand, nemit, nrec);
    if ((rc = records_fit(pl, "edit", "records", nrec, cap, total_out)) || !nrec) return rc;
    if (any_null({d_query, d_strand, d_end, d_edits})) return SUFR_HIP_E_INVALID;
    hipLaunchKernelGGL(sufr::k_edit_records, dim3(b.grid), dim3(256), 0, pl.stream, recs, (uint64_t)nrec, eb, (uint32_t)both, (uint64_t*)d_query,
                       (uint8_t*)d_strand, (uint64_t*)d_end, (uint8_t*)d_edits);
    return launch_status(pl, "edit");
}

int sufr_hip_edit(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const uint8_t* queries, const uint64_t* offsets, uint64_t num_queries,
                  uint32_t max_edits, uint64_t max_occ, uint32_t flags, uint64_t cap, uint64_t* query, uint8_t* strand, uint64_t* end,
                  uint8_t* edits, uint64_t* total_out)
{
    return pigeonhole_host(ctx, ix, queries, offsets, num_queries, max_edits, max_occ, flags, cap, query, strand, end, edits, total_out,
                           "k-difference", edit_args, sufr_hip_edit_device);
}

}  // extern "C"
