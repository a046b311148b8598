// sufr_search.inc -- batched search of a device-resident index (included by sufr_kernels.hip after sufr_capi.inc).
//
// What it replaces: the per-query work of SuffixArray::count / locate (libsufr/src/suffix_array.rs:181-236, 340-366),
// which the reference spreads over a rayon pool with one SufrSearch per thread (sufr_file.rs:760-800): two binary
// searches over the suffix array with SufrSearch::compare (sufr_search.rs:171-343).  Here the text and the suffix
// array stay in HBM and one launch answers a whole batch, one lane per query.
//
// The rank range is found as lower bound / upper bound of the same three-way comparison instead of the reference's
// "equal and the neighbour differs" probes: the comparison is monotone over the ranks of a sorted array, so both give
// the first and the last rank that compare equal; the bound form does one comparison per step instead of two.
//
// Cost model (DESIGN.md section 10): a step is two dependent loads, SA[mid] and the text at that position.  The first
// ~20 steps of every query fall on the same 2^20 array cells and stay in L2 / MALL; the last log2(s) - 20 steps of both
// searches are random 64-byte HBM sectors.  The kernel is latency bound per lane and sector-rate bound per device,
// nowhere near the byte rate of HBM.
//
// This file owns what every query kernel shares; sufr_match.inc, sufr_mem.inc, sufr_approx.inc, sufr_edit.inc and
// sufr_trace.inc, included after it, add only their own rules (DESIGN.md section 10, "The shared front end").
// Device: search_compare / common_prefix, the range search (search_seed, search_lower, search_range), last_le, scan_chunk
// (wg_scan and the sweep behind k_locate_scan are sufr_scan.inc), the locate scan (k_locate_counts / k_locate_scan / k_locate_apply), k_mem_bitmap and k_mem_revcomp.
// Host: query_check, lcp_refusals, index_sa, by_width, read_totals, scan_total; the batch of a call (take_batch =
// batch_extent + double_batch, mem_bitmap); candidate_starts; the record epilogue (records_fit, any_null, launch_status,
// report_total); the staging of the host-pointer entry points (stage_batch / unstage_batch, staged_records).

namespace sufr {

struct SearchIndex {
    const uint8_t* text;       // normalized text, n bytes
    uint64_t n;
    const uint32_t* sa;        // s ranks (32-bit arrays: text_len < 2^32 - 1, suffix_array.rs:460-470) ...
    const uint64_t* sa64;      // ... or 64-bit ones (exactly one of the two is set)
    uint64_t s;
    __device__ __forceinline__ uint64_t suffix(uint64_t r) const { return sa64 ? sa64[r] : (uint64_t)sa[r]; }
    const uint32_t* maskpos;   // offsets of the 1s of the seed mask (weight of them), or nullptr
    uint32_t weight, mask_len;
    // prefix table (optional): for every string of `pk` symbols over the table alphabet the rank range of the suffixes
    // that start with it, as (first rank, ~(last rank + 1)); 0xFFFFFFFF in .x: no such suffix
    const uint2* ptab;
    const uint8_t* pcode;      // 256 entries: code of a byte in the table alphabet, 0xFF outside it
    uint32_t pk, pradix;
};

struct SearchCmp { uint32_t lcp; int cmp; };          // cmp: -1 query < suffix, 0 equal, +1 query > suffix

// find_lcp_full_offset (util.rs:19-37)
__device__ __forceinline__ uint64_t search_full_offset(const SearchIndex& ix, uint32_t lcp)
{
    if (!ix.maskpos || lcp == 0 || lcp > ix.mask_len) return lcp;
    const uint32_t off = ix.maskpos[lcp - 1];
    const uint32_t next = lcp < ix.weight ? ix.maskpos[lcp] : 0;
    return (next > off && next - off > 1) ? next : off + 1;
}

// symbols a and b share from `from` on, `lim` at most: 8 per step (a byte loop pays one L2 round trip per symbol)
template <typename T>
__device__ __forceinline__ T common_prefix(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, T from, T lim)
{
    T k = from;
    bool diff = false;
    while (k + 8 <= lim) {
        uint64_t x, y;
        __builtin_memcpy(&x, a + k, 8);
        __builtin_memcpy(&y, b + k, 8);
        if (x != y) { k += (T)(__builtin_ctzll(x ^ y) >> 3); diff = true; break; }
        k += 8;
    }
    if (!diff) while (k < lim && a[k] == b[k]) k++;
    return k;
}

// SufrSearch::compare (sufr_search.rs:241-343); mql = the effective max_query_len (0: none), resolved on the host
__device__ __forceinline__ SearchCmp search_compare(const SearchIndex& ix, const uint8_t* __restrict__ q, uint32_t qlen, uint64_t mql,
                                                    uint64_t sp, uint32_t skip)
{
    uint32_t lcp;
    if (!ix.maskpos) {
        if (mql > 0 && skip >= mql) lcp = skip;
        else {
            const uint64_t ts = sp + skip;
            uint64_t te = mql > 0 ? ts + mql : ts + qlen;
            if (te > ix.n) te = ix.n;
            const uint32_t room = te > ts ? (uint32_t)(te - ts) : 0;
            const uint32_t lim = qlen - skip < room ? qlen - skip : room;      // skip <= qlen: it is an lcp with the query
            lcp = skip + common_prefix<uint32_t>(q + skip, ix.text + ts, 0, lim);
        }
    } else {
        const uint32_t weight = ix.weight;
        if (skip >= weight || (mql > 0 && skip >= mql)) lcp = skip;
        else {
            const uint32_t end = mql > 0 ? (mql < weight ? (uint32_t)mql : weight) : weight;
            uint32_t k = skip;                          // care positions are ascending: both length bounds are prefixes
            while (k < end) {
                const uint32_t off = ix.maskpos[k];
                if (off >= qlen || sp + off >= ix.n || q[off] != ix.text[sp + off]) break;
                k++;
            }
            lcp = k;
        }
    }
    int cmp;
    if (mql > 0 && lcp >= mql) cmp = 0;
    else {
        const uint64_t fo = search_full_offset(ix, lcp);
        if (fo >= qlen) cmp = 0;
        else if (sp + fo >= ix.n) cmp = 1;
        else {
            const uint8_t a = q[fo], b = ix.text[sp + fo];
            cmp = a < b ? -1 : (a > b ? 1 : 0);
        }
    }
    return {lcp, cmp};
}

// ---- the range search every query kernel shares (k_search_batch, k_matching_stats, k_mem_ranges) ------------------
// Returned by value: reference parameters for l / above / r_above cost these kernels 12 bytes of scratch per lane.
struct SearchSeed { uint64_t lo, hi; uint32_t shared; bool none; };               // [lo, hi) holds every suffix that can match
struct SearchLower { uint64_t first, above; uint32_t l, r_above; };

// Prefix table: the suffixes that start with the query's first pk symbols are one rank range, looked up instead of
// searched (`shared` = pk), or there are none (`none`).  Without a table, for a shorter query or cap, and for symbols
// outside the table alphabet: the whole array with nothing shared.
__device__ __forceinline__ SearchSeed search_seed(const SearchIndex& ix, const uint8_t* __restrict__ q, uint32_t qlen, uint64_t mql)
{
    SearchSeed s{0, ix.s, 0, false};
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
            if (e.x == 0xFFFFFFFFu) s.none = true;
            else { s.lo = e.x; s.hi = ~e.y; s.shared = ix.pk; }
        }
    }
    return s;
}

// Lower bound in [lo, hi), whose suffixes all share `shared` symbols with the query: `first` = the first rank whose
// suffix is not below the query, `above` = the lowest rank seen above it (hi if none), l = symbols shared with the
// suffix just below `first` (or with the whole range), r_above = those shared with `above`.
__device__ __forceinline__ SearchLower search_lower(const SearchIndex& ix, const uint8_t* __restrict__ q, uint32_t qlen, uint64_t mql,
                                                    uint64_t lo, uint64_t hi, uint32_t shared)
{
    uint64_t above = hi;
    uint32_t l = shared, r = shared, r_above = shared;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        const SearchCmp c = search_compare(ix, q, qlen, mql, ix.suffix(mid), l < r ? l : r);
        if (c.cmp > 0) { lo = mid + 1; l = c.lcp; }
        else {
            hi = mid; r = c.lcp;
            if (c.cmp < 0) { above = mid; r_above = c.lcp; }
        }
    }
    return {lo, above, l, r_above};
}

// The half-open rank range of the suffixes that match q[0..qlen); lo == hi == 0 when there are none.
__device__ __forceinline__ void search_range(const SearchIndex& ix, const uint8_t* __restrict__ q, uint32_t qlen, uint64_t mql,
                                             uint64_t& lo_out, uint64_t& hi_out)
{
    lo_out = hi_out = 0;
    const SearchSeed s = search_seed(ix, q, qlen, mql);
    if (s.none) return;
    const SearchLower b = search_lower(ix, q, qlen, mql, s.lo, s.hi, s.shared);
    // upper bound inside [first, above): the first rank whose suffix is above the query
    uint64_t ulo = b.first, uhi = b.above;
    uint32_t ul = b.l, ur = b.r_above;
    while (ulo < uhi) {
        const uint64_t mid = ulo + (uhi - ulo) / 2;
        const SearchCmp c = search_compare(ix, q, qlen, mql, ix.suffix(mid), ul < ur ? ul : ur);
        if (c.cmp >= 0) { ulo = mid + 1; ul = c.lcp; }
        else { uhi = mid; ur = c.lcp; }
    }
    if (ulo > b.first) { lo_out = b.first; hi_out = ulo; }
}

// byte histogram of the text (the table alphabet is chosen from it)
__global__ __launch_bounds__(256) void k_byte_hist(const uint8_t* __restrict__ text, uint64_t n, unsigned long long* __restrict__ hist)
{
    __shared__ uint32_t s_cnt[256];
    s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t at = (uint64_t)blockIdx.x * 256 + threadIdx.x; at < n; at += stride) atomicAdd(&s_cnt[text[at]], 1u);
    __syncthreads();
    if (s_cnt[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

// ranks are contiguous per prefix: first rank by atomicMin, last rank + 1 by atomicMin of its complement
__global__ __launch_bounds__(256) void k_prefix_table(SearchIndex ix, uint2* __restrict__ tab)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= ix.s) return;
    const uint64_t pos = ix.suffix(r);
    if (pos + ix.pk > ix.n) return;
    uint64_t code = 0;
    for (uint32_t k = 0; k < ix.pk; k++) {
        const uint32_t c = ix.pcode[ix.text[pos + k]];
        if (c == 0xFFu) return;
        code = code * ix.pradix + c;
    }
    atomicMin(&tab[code].x, (uint32_t)r);
    atomicMin(&tab[code].y, ~(uint32_t)(r + 1));
}

// One lane per query.  lo[i], hi[i]: the half-open rank range, lo == hi == 0 when the query does not occur.
__global__ __launch_bounds__(256) void k_search_batch(SearchIndex ix, const uint8_t* __restrict__ queries,
                                                      const uint64_t* __restrict__ qoff, uint64_t nq, uint64_t mql,
                                                      uint64_t* __restrict__ lo_out, uint64_t* __restrict__ hi_out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    uint64_t lo, hi;
    search_range(ix, queries + qoff[i], (uint32_t)(qoff[i + 1] - qoff[i]), mql, lo, hi);
    lo_out[i] = lo;
    hi_out[i] = hi;
}

// ---- locate: the positions behind the rank ranges ----------------------------------------------------------------
// counts (capped) -> exclusive scan in three small kernels -> one lane per output position
static constexpr int LOC_BLK = 2048;       // counts per workgroup of the scan (256 lanes x 8)
// k_locate_scan scans 1024 sums in one launch: the kernels that walk a whole batch with a scan of their own (SMEMs, MEMs)
// run this many workgroups, workgroup b over items [b * chunk, (b + 1) * chunk) in tiles of LOC_BLK (8 per lane)
static constexpr uint32_t SCAN_WGS = 1024;
__device__ __forceinline__ uint64_t scan_chunk(uint64_t total)
{
    const uint64_t c = (total + SCAN_WGS - 1) / SCAN_WGS;
    return (c + LOC_BLK - 1) / LOC_BLK * LOC_BLK;
}

// the last i in [a, b) with arr[i] <= v (arr ascending, arr[a] <= v): the slice of an exclusive scan that holds item v
__device__ __forceinline__ uint64_t last_le(const uint64_t* __restrict__ arr, uint64_t a, uint64_t b, uint64_t v)
{
    while (b - a > 1) { const uint64_t m = a + (b - a) / 2; if (arr[m] <= v) a = m; else b = m; }
    return a;
}

__global__ __launch_bounds__(256) void k_locate_counts(const uint64_t* __restrict__ lo, const uint64_t* __restrict__ hi, uint64_t nq,
                                                       uint64_t max_hits, uint64_t* __restrict__ off, uint64_t* __restrict__ blocksum)
{
    __shared__ uint64_t s_w[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * LOC_BLK + (uint64_t)threadIdx.x * 8;
    uint64_t c[8], sum = 0;
    for (int k = 0; k < 8; k++) {
        uint64_t v = i0 + k < nq ? hi[i0 + k] - lo[i0 + k] : 0;
        if (max_hits && v > max_hits) v = max_hits;
        c[k] = sum; sum += v;                                      // exclusive inside the lane
    }
    uint64_t base[1] = {sum}, tot[1];
    wg_scan(base, tot, s_w);
    for (int k = 0; k < 8; k++) if (i0 + k < nq) off[i0 + k] = base[0] + c[k];
    if (threadIdx.x == 0) blocksum[blockIdx.x] = tot[0];
}

// blocksum[0 .. nblk): the exclusive scan, in place; *total: the sum (tile_sweep of sufr_scan.inc)
__global__ __launch_bounds__(1024) void k_locate_scan(uint64_t* __restrict__ blocksum, uint64_t nblk, uint64_t* __restrict__ total)
{
    __shared__ uint64_t s_p[16];
    const uint64_t sum = tile_sweep<SumOp<uint64_t>, false>(
        nblk, [&](uint64_t b) { return blocksum[b]; }, [&](uint64_t b, uint64_t, uint64_t before) { blocksum[b] = before; }, s_p);
    if (threadIdx.x == 0) *total = sum;
}

__global__ __launch_bounds__(256) void k_locate_apply(uint64_t* __restrict__ off, uint64_t nq, const uint64_t* __restrict__ blocksum,
                                                      const uint64_t* __restrict__ total)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nq) off[i] += blocksum[i / LOC_BLK];
    if (i == nq) off[nq] = *total;
}

__global__ __launch_bounds__(256) void k_locate_gather(SearchIndex ix, const uint64_t* __restrict__ lo, const uint64_t* __restrict__ off,
                                                       uint64_t nq, uint64_t total, uint32_t* __restrict__ positions,
                                                       uint64_t* __restrict__ positions64)
{
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= total) return;
    const uint64_t a = last_le(off, 0, nq, j);                     // the query whose slice holds output j
    const uint64_t p = ix.suffix(lo[a] + (j - off[a]));
    if (positions64) positions64[j] = p; else positions[j] = (uint32_t)p;
}

// ---- what the seeded searches (MEMs, k-mismatch, k-difference, traceback) share on the device ----------------------
// once per index whose array leaves positions out: one lane per rank sets bit SA[r] (atomicOr on u32 words)
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

// both strands: the doubled batch, query i as it is then its reverse complement, with the new offsets (from 0)
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

}  // namespace sufr

struct sufr_hip_index {
    sufr::SearchIndex ix{};
    uint64_t built_mql = 0;
    int device = 0;
    int sa_width = 4;              // bytes per entry of the suffix array
    void* own_text = nullptr;      // allocations this object made (index_load); wrap() leaves them null
    void* own_sa = nullptr;
    void* own_mask = nullptr;
    void* ptab = nullptr;          // prefix table and its byte -> code map
    void* pcode = nullptr;
    mutable std::mutex mem_mu;     // MEMs (sufr_mem.inc): bitmap of the indexed positions, built by the first call that needs it
    mutable void* mem_bits = nullptr;
    mutable bool mem_bits_done = false;
};

namespace {

int index_set_mask(sufr_hip_ctx* ctx, sufr_hip_index* ix, const uint8_t* mask, uint64_t mask_len)
{
    std::vector<uint32_t> pos;
    for (uint64_t i = 0; i < mask_len; i++) if (mask[i] == 1 || mask[i] == '1') pos.push_back((uint32_t)i);
    if (pos.empty()) return 0;
    if (hipMalloc(&ix->own_mask, pos.size() * 4) != hipSuccess ||
        hipMemcpy(ix->own_mask, pos.data(), pos.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        ctx->pl.set_error("hipMalloc / hipMemcpy of the seed mask failed");
        return SUFR_HIP_E_HIP;
    }
    ix->ix.maskpos = (const uint32_t*)ix->own_mask;
    ix->ix.weight = (uint32_t)pos.size();
    ix->ix.mask_len = (uint32_t)mask_len;
    return 0;
}

// Prefix table of the index (DESIGN.md section 10).  Alphabet: ACGT for DNA, otherwise the byte values that make up at
// least 1 % of the text (32 at most); pk = the most symbols whose table stays within 2^28 entries and 4 entries per
// suffix.  Not built for seed-mask indexes and for max-query-len builds shorter than pk (their order is not the order
// of the first pk symbols).
int index_build_table(sufr_hip_ctx* ctx, sufr_hip_index* ix, bool is_dna)
{
    sufr::Pipeline& pl = ctx->pl;
    sufr::SearchIndex& X = ix->ix;
    if (X.maskpos || X.s < 2) return 0;
    if (X.s >= 0xFFFFFFFFull) return 0;                  // (the table holds 32-bit ranks: a longer array is searched without it)
    uint8_t map[256];
    memset(map, 0xFF, sizeof map);
    uint32_t radix = 0;
    if (is_dna) { for (const char* p = "ACGT"; *p; p++) map[(uint8_t)*p] = (uint8_t)radix++; }
    else {
        unsigned long long* d_hist = nullptr;
        unsigned long long hist[256];
        if (hipMalloc((void**)&d_hist, sizeof hist) != hipSuccess) { pl.set_error("hipMalloc failed"); return SUFR_HIP_E_NOMEM; }
        uint64_t grid = (X.n + 256 * 64 - 1) / (256 * 64);
        if (grid > 4096) grid = 4096;
        bool ok = hipMemsetAsync(d_hist, 0, sizeof hist, pl.stream) == hipSuccess;
        if (ok) hipLaunchKernelGGL(sufr::k_byte_hist, dim3((uint32_t)grid), dim3(256), 0, pl.stream, X.text, X.n, d_hist);
        ok = ok && hipMemcpyAsync(hist, d_hist, sizeof hist, hipMemcpyDeviceToHost, pl.stream) == hipSuccess &&
             hipStreamSynchronize(pl.stream) == hipSuccess;
        (void)hipFree(d_hist);
        if (!ok) { pl.set_error("byte histogram of the text failed"); return SUFR_HIP_E_HIP; }
        for (int c = 0; c < 256 && radix < 32; c++) if (hist[c] * 100 >= X.n) map[c] = (uint8_t)radix++;
    }
    if (radix < 2) return 0;
    uint64_t budget = X.s * 4 < ((uint64_t)1 << 28) ? X.s * 4 : ((uint64_t)1 << 28);
    if (budget < 256) budget = 256;
    uint32_t pk = 0;
    uint64_t entries = 1;
    while (entries * radix <= budget) { entries *= radix; pk++; }
    if (pk < 2 || (ix->built_mql > 0 && ix->built_mql < pk)) return 0;
    if (hipMalloc(&ix->ptab, entries * 8) != hipSuccess || hipMalloc(&ix->pcode, 256) != hipSuccess) {
        pl.set_error("hipMalloc of the prefix table (" + std::to_string(entries * 8) + " bytes) failed");
        return SUFR_HIP_E_NOMEM;
    }
    X.pk = pk; X.pradix = radix; X.pcode = (const uint8_t*)ix->pcode;
    if (hipMemcpyAsync(ix->pcode, map, 256, hipMemcpyHostToDevice, pl.stream) != hipSuccess ||
        hipMemsetAsync(ix->ptab, 0xFF, entries * 8, pl.stream) != hipSuccess) { pl.set_error("prefix table: setup failed"); return SUFR_HIP_E_HIP; }
    hipLaunchKernelGGL(sufr::k_prefix_table, dim3((uint32_t)((X.s + 255) / 256)), dim3(256), 0, pl.stream, X, (uint2*)ix->ptab);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(pl.stream) != hipSuccess) { pl.set_error("prefix table: kernel failed"); return SUFR_HIP_E_HIP; }
    X.ptab = (const uint2*)ix->ptab;
    return 0;
}

// the effective max_query_len of SufrSearch::compare (sufr_search.rs:251-262 for MaxQueryLen, 288-291 for Mask)
uint64_t effective_mql(const sufr_hip_index* ix, int has_mql, uint64_t mql)
{
    if (ix->ix.maskpos) return has_mql ? mql : 0;
    if (ix->built_mql > 0 && has_mql) return ix->built_mql < mql ? ix->built_mql : mql;
    return has_mql ? mql : ix->built_mql;
}

// what every query entry point checks before it touches the device; `masked`: what a seed-mask index does not support
// (nullptr: it does)
int query_check(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const char* masked = nullptr)
{
    if (ix->device != ctx->pl.device) { ctx->pl.set_error("the index lives on another device"); return SUFR_HIP_E_INVALID; }
    if (masked && ix->ix.maskpos) { ctx->pl.set_error(std::string(masked) + " of a seed-mask index are not supported"); return SUFR_HIP_E_UNSUPPORTED; }
    if (hipSetDevice(ctx->pl.device) != hipSuccess) { ctx->pl.set_error("hipSetDevice failed"); return SUFR_HIP_E_HIP; }
    return 0;
}

// the preamble of the calls that read the whole LCP (repeats, shared and common, lpf and lz, unique lengths): query_check,
// then the refusal of an index whose LCP was capped by max_query_len; `what` names the call in that text
int lcp_refusals(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const char* masked_name, const char* what)
{
    ctx->pl.err.clear();
    if (const int rc = query_check(ctx, ix, masked_name)) return rc;
    if (ix->built_mql > 0) {
        ctx->pl.set_error(std::string(what) + ": the index was built with max_query_len " + std::to_string(ix->built_mql) + ", its LCP is capped");
        return SUFR_HIP_E_UNSUPPORTED;
    }
    return 0;
}

// the suffix array in the width the index has
template <typename T>
const T* index_sa(const sufr_hip_index* ix) { return (const T*)(ix->ix.sa64 ? (const void*)ix->ix.sa64 : (const void*)ix->ix.sa); }

// fn(uint32_t()) or fn(uint64_t()), by the width of the index: fn is a generic lambda that takes its T from the argument
template <typename F>
int by_width(const sufr_hip_index* ix, F fn) { return ix->sa_width == 8 ? fn(uint64_t()) : fn(uint32_t()); }

// the workgroups of the kernels that loop over a batch (latency-bound lanes: 8 workgroups of 4 waves per CU)
uint32_t batch_grid(const sufr::Pipeline& pl) { return (pl.num_cus ? pl.num_cus : 256u) * 8u; }

// n totals of the device to the host, complete on return (one synchronisation); the error text is "<tag>: <what>"
int read_totals(sufr::Pipeline& pl, const void* d_src, int n, unsigned long long* dst, const char* tag, const char* what)
{
    if (hipMemcpyAsync(dst, d_src, (size_t)n * 8, hipMemcpyDeviceToHost, pl.stream) == hipSuccess &&
        hipStreamSynchronize(pl.stream) == hipSuccess) return 0;
    pl.set_error(std::string(tag) + ": " + what);
    return SUFR_HIP_E_HIP;
}

// k_locate_scan over n workgroup sums (in place: the exclusive bases) and their total, read to the host: one
// synchronisation.  The error text is "<tag>: <what>".
int scan_total(sufr::Pipeline& pl, uint64_t* sums, uint64_t n, unsigned long long* total, const char* tag, const char* what)
{
    hipLaunchKernelGGL(sufr::k_locate_scan, dim3(1), dim3(1024), 0, pl.stream, sums, n, sums + n);
    return read_totals(pl, sums + n, 1, total, tag, what);
}

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
    const uint32_t grid = batch_grid(pl);
    bool ok = hipMemsetAsync(bits, 0, words * 4, pl.stream) == hipSuccess;
    if (ok) hipLaunchKernelGGL(sufr::k_mem_bitmap, dim3(grid), dim3(256), 0, pl.stream, ix->ix, (uint32_t*)bits);
    ok = ok && hipGetLastError() == hipSuccess && hipStreamSynchronize(pl.stream) == hipSuccess;   // other streams may use it next
    if (!ok) { (void)hipFree(bits); pl.set_error("mems: building the indexed-position bitmap failed"); return SUFR_HIP_E_HIP; }
    ix->mem_bits = bits;
    ix->mem_bits_done = true;
    return 0;
}

// ---- the batch of a call (MEMs, k-mismatch, k-difference, traceback) -------------------------------------------------
// q / qoff: the bytes and the nq + 1 offsets the kernels read (the doubled batch with both strands), nb: its byte count
// (0: an empty batch, nothing to do), grid: the workgroups of the kernels that loop over it
struct QueryBatch { const uint8_t* q; const uint64_t* qoff; uint64_t nq, nb; uint32_t grid; bool both; };

// the batch as the caller gave it: the bitmap of the index, then the two ends of the offsets (one synchronisation).  ix may
// be null: a caller without text and suffix array (the FM-index of sufr_fm.inc), for which no bitmap is made
int batch_extent(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_queries, const void* d_offsets, uint64_t num_queries,
                 const char* tag, QueryBatch& b)
{
    sufr::Pipeline& pl = ctx->pl;
    b = QueryBatch{(const uint8_t*)d_queries, (const uint64_t*)d_offsets, num_queries, 0, batch_grid(pl), false};
    if (!num_queries) return 0;
    if (ix) if (const int rc = mem_bitmap(ctx, ix)) return rc;
    unsigned long long ends[2] = {0, 0};                             // offsets[0] and offsets[num_queries]
    bool ok = true;
    for (int k = 0; k < 2; k++)
        ok = ok && hipMemcpyAsync(&ends[k], b.qoff + k * num_queries, 8, hipMemcpyDeviceToHost, pl.stream) == hipSuccess;
    if (!ok || hipStreamSynchronize(pl.stream) != hipSuccess) { pl.set_error(std::string(tag) + ": reading the batch offsets failed"); return SUFR_HIP_E_HIP; }
    if (ends[1] > ends[0]) b.nb = ends[1] - ends[0];
    return 0;
}

// both strands: k_mem_revcomp of the batch as given (nb bytes) into the context's xq / xoff, which b then names
int double_batch(sufr_hip_ctx* ctx, QueryBatch& b)
{
    sufr::Pipeline& pl = ctx->pl;
    int rc;
    if ((rc = pl.ensure(ctx->xq, 2 * b.nb + 8)) || (rc = pl.ensure(ctx->xoff, (2 * b.nq + 1) * 8))) return rc;
    hipLaunchKernelGGL(sufr::k_mem_revcomp, dim3(b.grid), dim3(256), 0, pl.stream, b.q, b.qoff, b.nq, (uint8_t*)ctx->xq.p, (uint64_t*)ctx->xoff.p);
    b = QueryBatch{(const uint8_t*)ctx->xq.p, (const uint64_t*)ctx->xoff.p, 2 * b.nq, 2 * b.nb, b.grid, true};
    return 0;
}

// batch_extent, then with both strands double_batch; ix may be null as for batch_extent
int take_batch(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_queries, const void* d_offsets, uint64_t num_queries, bool both,
               const char* tag, QueryBatch& b)
{
    if (const int rc = batch_extent(ctx, ix, d_queries, d_offsets, num_queries, tag, b)) return rc;
    return both && b.nb ? double_batch(ctx, b) : 0;
}

// ---- candidate starts ---------------------------------------------------------------------------------------------------
// n items (the offsets of MEMs, the seeds of the pigeonhole searches) each with a rank range: ranges(rlo, rhi) launches the
// kernel that fills them, then k_locate_counts / k_locate_scan / k_locate_apply make cand[0 .. n] the exclusive scan of the
// range sizes and one synchronisation reads their total.  cnt_sum: SCAN_WGS + 1 words for the count kernel that follows.
struct Candidates { uint64_t* rlo; uint64_t* cand; uint64_t* cnt_sum; unsigned long long ncand; };

template <typename Ranges>
int candidate_starts(sufr_hip_ctx* ctx, uint64_t n, const char* tag, Ranges ranges, Candidates& c)
{
    sufr::Pipeline& pl = ctx->pl;
    const uint64_t nblk = (n + sufr::LOC_BLK - 1) / sufr::LOC_BLK;
    int rc;
    if ((rc = pl.ensure(ctx->xlo, n * 8)) || (rc = pl.ensure(ctx->xhi, n * 8)) || (rc = pl.ensure(ctx->xcand, (n + 1) * 8)) ||
        (rc = pl.ensure(ctx->xsum, (nblk + 1 + sufr::SCAN_WGS + 1) * 8))) return rc;
    uint64_t* rhi = (uint64_t*)ctx->xhi.p;
    uint64_t* bsum = (uint64_t*)ctx->xsum.p;
    c = Candidates{(uint64_t*)ctx->xlo.p, (uint64_t*)ctx->xcand.p, bsum + nblk + 1, 0};
    ranges(c.rlo, rhi);
    hipLaunchKernelGGL(sufr::k_locate_counts, dim3((uint32_t)nblk), dim3(256), 0, pl.stream, (const uint64_t*)c.rlo, (const uint64_t*)rhi, n,
                       (uint64_t)0, c.cand, bsum);
    hipLaunchKernelGGL(sufr::k_locate_scan, dim3(1), dim3(1024), 0, pl.stream, bsum, nblk, bsum + nblk);
    hipLaunchKernelGGL(sufr::k_locate_apply, dim3((uint32_t)((n + 256) / 256)), dim3(256), 0, pl.stream, c.cand, n, (const uint64_t*)bsum,
                       (const uint64_t*)(bsum + nblk));
    return read_totals(pl, bsum + nblk, 1, &c.ncand, tag, "counting the candidates failed");
}

// ---- the record epilogue ------------------------------------------------------------------------------------------------
// the total of a call against the room of its caller: "<tag>: N <noun>, room for M"
int records_fit(sufr::Pipeline& pl, const char* tag, const char* noun, uint64_t total, uint64_t cap, uint64_t* total_out)
{
    if (total_out) *total_out = total;
    if (total <= cap) return 0;
    pl.set_error(std::string(tag) + ": " + std::to_string(total) + " " + noun + ", room for " + std::to_string(cap));
    return SUFR_HIP_E_CAPACITY;
}

bool any_null(std::initializer_list<const void*> ptrs)
{
    for (const void* p : ptrs) if (!p) return true;
    return false;
}

// what the launches of a call left behind
int launch_status(sufr::Pipeline& pl, const char* tag)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    pl.set_error(std::string(tag) + ": " + hipGetErrorString(e));
    return SUFR_HIP_E_HIP;
}

// The report of a counted call between its counting and its writing launches: what the launches left behind, the ncols
// stats of the device into h (h[0] the total; one synchronisation; zeros when it fails), the total against the caller's room
// and, when there is something to write, the caller's arrays.  0: h[0] records are to be written (none: nothing is left to do).
int report_total(sufr::Pipeline& pl, const char* tag, const char* noun, const void* d_stats, int ncols, unsigned long long* h, uint64_t cap,
                 uint64_t* total_out, bool have_outputs)
{
    for (int k = 0; k < ncols; k++) h[k] = 0;
    int rc;
    if ((rc = launch_status(pl, tag)) || (rc = read_totals(pl, d_stats, ncols, h, tag, "reading the total failed")) ||
        (rc = records_fit(pl, tag, noun, h[0], cap, total_out))) return rc;
    if (h[0] && !have_outputs) { pl.set_error(std::string(tag) + ": no output arrays"); return SUFR_HIP_E_INVALID; }
    return 0;
}

// The host-pointer entry points stage their batch in one allocation, queries | offsets (at o_at) | what the caller lays
// out behind them, and call their *_device twin on it.  `what` names the batch in the error texts.
int stage_batch(sufr_hip_ctx* ctx, const char* what, const uint8_t* queries, const uint64_t* offsets, uint64_t nq, uint64_t o_at,
                uint64_t bytes, uint8_t** d)
{
    if (hipMalloc((void**)d, bytes) != hipSuccess) {
        *d = nullptr;
        ctx->pl.set_error(std::string("hipMalloc of the ") + what + " batch failed");
        return SUFR_HIP_E_NOMEM;
    }
    if ((offsets[nq] && hipMemcpyAsync(*d, queries, offsets[nq], hipMemcpyHostToDevice, ctx->pl.stream) != hipSuccess) ||
        hipMemcpyAsync(*d + o_at, offsets, (nq + 1) * 8, hipMemcpyHostToDevice, ctx->pl.stream) != hipSuccess) return SUFR_HIP_E_HIP;
    return 0;
}

struct StageBack { void* dst; uint64_t at, bytes; };             // to the host: `bytes` from offset `at` of the allocation

// rc: what staging and the device call gave; when that is 0 the results are copied back, complete on return
int unstage_batch(sufr_hip_ctx* ctx, const char* what, uint8_t* d, int rc, const StageBack* back, size_t n)
{
    for (size_t k = 0; k < n; k++)
        if (!rc && back[k].bytes && hipMemcpyAsync(back[k].dst, d + back[k].at, back[k].bytes, hipMemcpyDeviceToHost, ctx->pl.stream) != hipSuccess)
            rc = SUFR_HIP_E_HIP;
    if (!rc && hipStreamSynchronize(ctx->pl.stream) != hipSuccess) rc = SUFR_HIP_E_HIP;
    if (rc == SUFR_HIP_E_HIP && ctx->pl.err.empty()) ctx->pl.set_error(std::string("copying the ") + what + " batch failed");
    (void)hipFree(d);
    return rc;
}

int unstage_batch(sufr_hip_ctx* ctx, const char* what, uint8_t* d, int rc, std::initializer_list<StageBack> back)
{
    return unstage_batch(ctx, what, d, rc, back.begin(), back.size());
}

// A host-pointer entry point whose results are record columns: one allocation, queries | offsets | every column at `cap`
// elements of its width | `extra` bytes, each part on an 8-byte boundary.  call(d_queries, d_offsets, col, &total) runs the
// *_device twin on it (col[k]: column k, col[number of columns]: the extra bytes); `total` elements of every column go back.
struct Column { void* host; uint32_t width; };
static constexpr size_t STAGE_MAX_COLUMNS = 6;

template <typename Call>
int staged_records(sufr_hip_ctx* ctx, const char* what, const uint8_t* queries, const uint64_t* offsets, uint64_t nq, uint64_t cap,
                   std::initializer_list<Column> cols, uint64_t extra, uint64_t* total_out, Call call)
{
    const uint64_t o_at = (offsets[nq] + 7) / 8 * 8;
    uint64_t at[STAGE_MAX_COLUMNS + 1], end = o_at + (nq + 1) * 8;
    size_t k = 0;
    for (const Column& c : cols) { at[k++] = end; end += (cap * c.width + 7) / 8 * 8; }
    at[k] = end;
    uint8_t* d;
    int rc = stage_batch(ctx, what, queries, offsets, nq, o_at, end + extra + 8, &d);
    uint64_t total = 0;
    if (!rc) {
        void* col[STAGE_MAX_COLUMNS + 1];
        for (size_t j = 0; j <= k; j++) col[j] = d + at[j];
        rc = call(d, d + o_at, col, &total);
    }
    if (total_out) *total_out = total;
    StageBack back[STAGE_MAX_COLUMNS];
    k = 0;
    for (const Column& c : cols) { back[k] = StageBack{c.host, at[k], total * c.width}; k++; }
    return unstage_batch(ctx, what, d, rc, back, k);
}

}  // namespace

extern "C" {

int sufr_hip_index_wrap(sufr_hip_ctx* ctx, const void* d_text, uint64_t text_len, const void* d_sa, uint64_t num_suffixes,
                        uint32_t flags, uint64_t built_max_query_len, const char* seed_mask, sufr_hip_index** out)
{
    if (!ctx || !out || !d_text || (!d_sa && num_suffixes)) return SUFR_HIP_E_INVALID;
    *out = nullptr;
    ctx->pl.err.clear();
    // the width of the array: the file format's rule (suffix_array.rs:460-470: u32 iff text_len < u32::MAX), or the flag
    const bool wide = text_len >= 0xFFFFFFFFull || (flags & SUFR_HIP_FLAG_SA_U64);
    if (hipSetDevice(ctx->pl.device) != hipSuccess) { ctx->pl.set_error("hipSetDevice failed"); return SUFR_HIP_E_HIP; }
    if (num_suffixes) {
        // a u32 array handed over for a text that takes u64 entries (or the flag set on a u32 array) would be read past its
        // end: what the runtime knows about the allocation behind d_sa must cover num_suffixes entries of the assumed width
        void* abase = nullptr; size_t asize = 0;
        if (hipMemGetAddressRange((hipDeviceptr_t*)&abase, &asize, (hipDeviceptr_t)d_sa) == hipSuccess && abase) {
            const size_t off = (size_t)((const uint8_t*)d_sa - (const uint8_t*)abase);
            if (off > asize || (asize - off) / (wide ? 8u : 4u) < num_suffixes) {
                ctx->pl.set_error(std::string("index_wrap: d_sa is shorter than num_suffixes entries of ") + (wide ? "8" : "4") + " bytes");
                return SUFR_HIP_E_INVALID;
            }
        } else (void)hipGetLastError();
    }
    sufr_hip_index* ix = new sufr_hip_index;
    ix->device = ctx->pl.device;
    ix->ix.text = (const uint8_t*)d_text; ix->ix.n = text_len;
    ix->ix.sa = wide ? nullptr : (const uint32_t*)d_sa; ix->ix.sa64 = wide ? (const uint64_t*)d_sa : nullptr; ix->ix.s = num_suffixes;
    ix->sa_width = wide ? 8 : 4;
    ix->built_mql = built_max_query_len;
    if (seed_mask) {
        const int rc = index_set_mask(ctx, ix, (const uint8_t*)seed_mask, strlen(seed_mask));
        if (rc) { sufr_hip_index_free(ix); return rc; }
    }
    if (!(flags & SUFR_HIP_FLAG_NO_PREFIX_TABLE))
        if (const int rc = index_build_table(ctx, ix, (flags & SUFR_HIP_FLAG_DNA) != 0)) { sufr_hip_index_free(ix); return rc; }
    *out = ix;
    return 0;
}

int sufr_hip_index_load(sufr_hip_ctx* ctx, const sufr_file* f, sufr_hip_index** out)
{
    if (!ctx || !f || !out) return SUFR_HIP_E_INVALID;
    *out = nullptr;
    ctx->pl.err.clear();
    sufr_file_meta m;
    sufr_file_metadata(f, &m);
    const bool wide = m.index_width != 4;
    if (hipSetDevice(ctx->pl.device) != hipSuccess) { ctx->pl.set_error("hipSetDevice failed"); return SUFR_HIP_E_HIP; }
    sufr_hip_index* ix = new sufr_hip_index;
    ix->device = ctx->pl.device;
    const uint64_t sa_bytes = m.len_suffixes * (wide ? 8 : 4);
    if (hipMalloc(&ix->own_text, m.text_len ? m.text_len : 1) != hipSuccess || hipMalloc(&ix->own_sa, sa_bytes ? sa_bytes : 4) != hipSuccess) {
        ctx->pl.set_error("hipMalloc of the index (" + std::to_string(m.text_len + sa_bytes) + " bytes) failed");
        sufr_hip_index_free(ix);
        return SUFR_HIP_E_NOMEM;
    }
    // the mapping is pageable memory: parallel_copy stages it through pinned pieces
    if (parallel_copy(ctx->pl.device, ix->own_text, sufr_file_text(f), m.text_len, false) ||
        parallel_copy(ctx->pl.device, ix->own_sa, sufr_file_suffix_array(f), sa_bytes, false)) {
        ctx->pl.set_error("copying the index to the device failed");
        sufr_hip_index_free(ix);
        return SUFR_HIP_E_HIP;
    }
    ix->ix.text = (const uint8_t*)ix->own_text; ix->ix.n = m.text_len;
    ix->ix.sa = wide ? nullptr : (const uint32_t*)ix->own_sa; ix->ix.sa64 = wide ? (const uint64_t*)ix->own_sa : nullptr;
    ix->sa_width = wide ? 8 : 4;
    ix->ix.s = m.len_suffixes;
    ix->built_mql = m.max_query_len;
    if (m.seed_mask_len) {
        const int rc = index_set_mask(ctx, ix, sufr_file_seed_mask(f), m.seed_mask_len);
        if (rc) { sufr_hip_index_free(ix); return rc; }
    }
    if (const int rc = index_build_table(ctx, ix, m.is_dna != 0)) { sufr_hip_index_free(ix); return rc; }
    *out = ix;
    return 0;
}

int sufr_hip_index_width(const sufr_hip_index* ix) { return ix ? ix->sa_width : 0; }

void sufr_hip_index_free(sufr_hip_index* ix)
{
    if (!ix) return;
    (void)hipSetDevice(ix->device);
    if (ix->own_text) (void)hipFree(ix->own_text);
    if (ix->own_sa) (void)hipFree(ix->own_sa);
    if (ix->own_mask) (void)hipFree(ix->own_mask);
    if (ix->ptab) (void)hipFree(ix->ptab);
    if (ix->pcode) (void)hipFree(ix->pcode);
    if (ix->mem_bits) (void)hipFree(ix->mem_bits);
    delete ix;
}

int sufr_hip_search_batch_device(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_queries, const void* d_offsets,
                                 uint64_t num_queries, int has_max_query_len, uint64_t max_query_len, void* d_rank_lo,
                                 void* d_rank_hi)
{
    if (!ctx || !ix || (num_queries && (!d_queries || !d_offsets || !d_rank_lo || !d_rank_hi))) return SUFR_HIP_E_INVALID;
    ctx->pl.err.clear();
    if (!num_queries) return 0;
    if (const int rc = query_check(ctx, ix)) return rc;
    const uint64_t blocks = (num_queries + 255) / 256;
    if (blocks > 0x7fffffffull) { ctx->pl.set_error("too many queries in one batch"); return SUFR_HIP_E_INVALID; }
    sufr::k_search_batch<<<(unsigned)blocks, 256, 0, ctx->pl.stream>>>(ix->ix, (const uint8_t*)d_queries, (const uint64_t*)d_offsets,
                                                                     num_queries, effective_mql(ix, has_max_query_len, max_query_len),
                                                                     (uint64_t*)d_rank_lo, (uint64_t*)d_rank_hi);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { ctx->pl.set_error(std::string("k_search_batch: ") + hipGetErrorString(e)); return SUFR_HIP_E_HIP; }
    return 0;
}

int sufr_hip_locate_batch_device(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const void* d_rank_lo, const void* d_rank_hi,
                                 uint64_t num_queries, uint64_t max_hits, void* d_offsets, void* d_positions, uint64_t cap,
                                 uint64_t* total_out)
{
    if (!ctx || !ix || !d_offsets || (num_queries && (!d_rank_lo || !d_rank_hi))) return SUFR_HIP_E_INVALID;
    sufr::Pipeline& pl = ctx->pl;
    pl.err.clear();
    if (total_out) *total_out = 0;
    int rc;
    if ((rc = query_check(ctx, ix))) return rc;
    const uint64_t nblk = (num_queries + sufr::LOC_BLK - 1) / sufr::LOC_BLK;
    if ((rc = pl.ensure(pl.scalars, sufr::Pipeline::SC_N * 8)) || (rc = pl.ensure(pl.partials, (size_t)(nblk + 1) * 8))) return rc;
    unsigned long long total = 0;
    uint64_t* off = (uint64_t*)d_offsets;
    if (num_queries) {
        hipLaunchKernelGGL(sufr::k_locate_counts, dim3((uint32_t)nblk), dim3(256), 0, pl.stream, (const uint64_t*)d_rank_lo,
                           (const uint64_t*)d_rank_hi, num_queries, max_hits, off, (uint64_t*)pl.partials.p);
        hipLaunchKernelGGL(sufr::k_locate_scan, dim3(1), dim3(1024), 0, pl.stream, (uint64_t*)pl.partials.p, nblk,
                           (uint64_t*)pl.sc(sufr::Pipeline::SC_TOTAL));
        hipLaunchKernelGGL(sufr::k_locate_apply, dim3((uint32_t)((num_queries + 256) / 256)), dim3(256), 0, pl.stream, off, num_queries,
                           (const uint64_t*)pl.partials.p, (const uint64_t*)pl.sc(sufr::Pipeline::SC_TOTAL));
        if ((rc = read_totals(pl, pl.sc(sufr::Pipeline::SC_TOTAL), 1, &total, "locate", "counting the matches failed"))) return rc;
    } else if (hipMemsetAsync(d_offsets, 0, 8, pl.stream) != hipSuccess) { pl.set_error("memset failed"); return SUFR_HIP_E_HIP; }
    if (total_out) *total_out = total;
    if (total > cap) {
        pl.set_error("locate: " + std::to_string(total) + " positions, room for " + std::to_string(cap) + " (raise the capacity or set max_hits)");
        return SUFR_HIP_E_CAPACITY;
    }
    if (total) {
        if (!d_positions) return SUFR_HIP_E_INVALID;
        const uint64_t blocks = (total + 255) / 256;
        if (blocks > 0x7fffffffull) { pl.set_error("locate: too many positions for one launch"); return SUFR_HIP_E_INVALID; }
        hipLaunchKernelGGL(sufr::k_locate_gather, dim3((uint32_t)blocks), dim3(256), 0, pl.stream, ix->ix, (const uint64_t*)d_rank_lo,
                           (const uint64_t*)off, num_queries, (uint64_t)total, ix->ix.sa64 ? (uint32_t*)nullptr : (uint32_t*)d_positions,
                           ix->ix.sa64 ? (uint64_t*)d_positions : (uint64_t*)nullptr);
        if (hipGetLastError() != hipSuccess) { pl.set_error("k_locate_gather failed to launch"); return SUFR_HIP_E_HIP; }
    }
    return 0;
}

int sufr_hip_search_batch(sufr_hip_ctx* ctx, const sufr_hip_index* ix, const uint8_t* queries, const uint64_t* offsets,
                          uint64_t num_queries, int has_max_query_len, uint64_t max_query_len, uint64_t* rank_lo,
                          uint64_t* rank_hi)
{
    if (!ctx || !ix || (num_queries && (!offsets || !rank_lo || !rank_hi))) return SUFR_HIP_E_INVALID;
    ctx->pl.err.clear();
    if (!num_queries) return 0;
    if (hipSetDevice(ctx->pl.device) != hipSuccess) { ctx->pl.set_error("hipSetDevice failed"); return SUFR_HIP_E_HIP; }
    // one allocation: queries | offsets | rank_lo | rank_hi
    const uint64_t obytes = (num_queries + 1) * 8, rbytes = num_queries * 8;
    const uint64_t o_at = (offsets[num_queries] + 7) / 8 * 8, lo_at = o_at + obytes, hi_at = lo_at + rbytes;
    uint8_t* d;
    int rc = stage_batch(ctx, "query", queries, offsets, num_queries, o_at, hi_at + rbytes, &d);
    if (!rc) rc = sufr_hip_search_batch_device(ctx, ix, d, d + o_at, num_queries, has_max_query_len, max_query_len, d + lo_at, d + hi_at);
    return unstage_batch(ctx, "query", d, rc, {{rank_lo, lo_at, rbytes}, {rank_hi, hi_at, rbytes}});
}

}  // extern "C"
