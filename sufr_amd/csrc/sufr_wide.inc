// sufr_wide.inc -- texts the 32-bit record indices of the pipeline cannot address (included by sufr_kernels.hip
// after sufr_launch.inc): n >= 2^32 - 2^24, the u64 arm of SuffixArray::write (libsufr/src/suffix_array.rs:460-470,
// types.rs:288-345 `Int`), SURVEY.md section 8 row f4.
//
// The text is cut into windows of H positions.  Window i is an ordinary 32-bit build of text[i*H, i*H + H + M): its
// own H positions plus a margin of M that only serves as comparison context.  The suffixes that start in the margin are
// dropped from the result (LCP of the survivors = minimum over the dropped run), and the window is accepted when no
// comparison between two surviving neighbours ran into the end of the window:
//         max(a, b) + lcp(a, b) < window length          for every surviving neighbour pair (a, b),
// which says that their order was decided by a real mismatch, the same one the whole text shows.  A repeat longer than
// the margin fails the test; the window is then rebuilt with the largest margin that fits 32 bits (or the caller's cap,
// sufr_hip_set_window_retry).  If that fails too (round 5; rounds 2-4 stopped with SUFR_HIP_E_UNSUPPORTED here), the
// suffixes whose comparison with their successor ran into the end of the window -- "short" suffixes: the window saw a
// proper prefix of them -- are taken OUT of the window's arrays (the others are in whole-text order among themselves,
// with exact LCPs: see repair_window), ordered by comparisons over the WHOLE text with 64-bit positions (a bitonic
// network over wide_compare; LCPs from one comparison per neighbour pair) and handed to the merge as a list of their
// own, which the rank merge places like any other window's.  Comparisons over the whole text walk the repeat symbol by
// symbol: this is the correct slow path for the rare window, not a fast one; more than 2^22 such suffixes in one
// window are refused.
//
// The windows are then merged by rank: every suffix x of window i finds, by binary search with whole-text comparison,
// how many suffixes of every other window are smaller, and its LCP with its predecessor there (the last probe that
// compared below x).  Its place in the output is its own rank plus those counts; its LCP is the largest LCP with any of
// the candidate predecessors (its own window's included), because the true predecessor is the largest candidate and the
// LCP with x grows as a candidate gets closer to x.  Suffixes are distinct, so there are no ties to break.
//
// --max-query-len / --seed-mask builds (find_lcp's other arms, sufr_builder.rs:272-314): the windows are built with the
// option and merged under the same order (WideOrder) -- the first L symbols / the care symbols of the mask decide, equal
// ones come in descending position (the canonical member of the reference's family, see apply_max_query_len and
// sort_masked), the LCP is the capped / care-symbol count.  A tie in one window and a tie across windows are the same
// rule, so the merge stays a merge of strictly ordered lists.

namespace sufr {

static constexpr int WIDE_MAX_WINDOWS = 32;     // (windows of the text + the lists of repaired suffixes, one per window that needed it)
struct WideWindow { const uint32_t* sa; const uint32_t* lcp; uint64_t base, count; };
struct WideWindows { WideWindow w[WIDE_MAX_WINDOWS]; int num; };

// sufr_builder.rs:144-160 on a byte stream, 16 bytes per lane
__global__ void __launch_bounds__(256)
k_wide_normalize(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint64_t n, int raw, int softmask)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256 * 16;
    for (uint64_t at = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 16; at < n; at += stride) {
        const int m = n - at < 16 ? (int)(n - at) : 16;
        uint8_t v[16];
        if (m == 16) *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(in + at);
        else for (int k = 0; k < m; k++) v[k] = in[at + k];
        if (raw)
            for (int k = 0; k < 16; k++) if (v[k] >= 97 && v[k] <= 122) v[k] = softmask ? (uint8_t)'N' : (uint8_t)(v[k] & 0x5F);
        if (m == 16) *reinterpret_cast<uint4*>(out + at) = *reinterpret_cast<const uint4*>(v);
        else for (int k = 0; k < m; k++) out[at + k] = v[k];
    }
}

static constexpr int WIDE_BLK = 4096;          // ranks per workgroup of the filter kernels (256 lanes x 16)

// survivors per workgroup: suffixes that start inside the window's own H positions (drop == nullptr), or -- the repair of
// a window, below -- the ranks whose drop flag is not set
__global__ void __launch_bounds__(256)
k_wide_count(const uint32_t* __restrict__ sa, uint64_t s, uint32_t own, uint32_t* __restrict__ blockcnt,
             const uint8_t* __restrict__ drop = nullptr, uint32_t skip = 0 /* ranks below it do not count (shards: an aligned start) */)
{
    __shared__ uint32_t s_sum[4];
    const uint64_t r0 = (uint64_t)blockIdx.x * WIDE_BLK + (uint64_t)threadIdx.x * 16;
    uint32_t c = 0;
    for (int k = 0; k < 16; k++) if (r0 + k < s && r0 + k >= skip && (drop ? !drop[r0 + k] : sa[r0 + k] < own)) c++;
    for (int o = 32; o; o >>= 1) c += __shfl_down(c, o);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) blockcnt[blockIdx.x] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

// exclusive scan of the workgroup counts, one workgroup; total -> *total
__global__ void __launch_bounds__(1024)
k_wide_scan(uint32_t* __restrict__ blockcnt, uint32_t nblk, unsigned long long* __restrict__ total)
{
    __shared__ uint32_t s_part[1024];
    const uint32_t per = (nblk + 1023) / 1024;
    const uint32_t lo = threadIdx.x * per, hi = lo + per < nblk ? lo + per : nblk;
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; i++) sum += blockcnt[i];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const uint32_t v = threadIdx.x >= (unsigned)o ? s_part[threadIdx.x - o] : 0;
        __syncthreads();
        s_part[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = s_part[threadIdx.x] - sum;
    for (uint32_t i = lo; i < hi; i++) { const uint32_t c = blockcnt[i]; blockcnt[i] = run; run += c; }
    if (threadIdx.x == 1023) *total = s_part[1023];
}

// survivors in rank order; their LCP is the minimum over the dropped suffixes between them and the previous survivor.
// A lane holds its 16 ranks in registers; only a dropped run that reaches back over the lane's first rank is walked
// in memory (margin suffixes are a few per cent of a window).
__global__ void __launch_bounds__(256)
k_wide_compact(const uint32_t* __restrict__ sa, const uint32_t* __restrict__ lcp, uint64_t s, uint32_t own,
               const uint32_t* __restrict__ blockoff, uint32_t* __restrict__ out_sa, uint32_t* __restrict__ out_lcp,
               const uint8_t* __restrict__ drop = nullptr, uint32_t skip = 0)
{
    __shared__ uint32_t s_wave[4];
    const uint64_t r0 = (uint64_t)blockIdx.x * WIDE_BLK + (uint64_t)threadIdx.x * 16;
    uint32_t v[16], l[16];
    if (r0 + 16 <= s) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint4 a = reinterpret_cast<const uint4*>(sa + r0)[q], b = reinterpret_cast<const uint4*>(lcp + r0)[q];
            v[4 * q] = a.x; v[4 * q + 1] = a.y; v[4 * q + 2] = a.z; v[4 * q + 3] = a.w;
            l[4 * q] = b.x; l[4 * q + 1] = b.y; l[4 * q + 2] = b.z; l[4 * q + 3] = b.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 16; k++) { v[k] = r0 + k < s ? sa[r0 + k] : 0xFFFFFFFFu; l[k] = r0 + k < s ? lcp[r0 + k] : 0; }
    }
    uint32_t keep = 0, c = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) if (r0 + k < s && r0 + k >= skip && (drop ? !drop[r0 + k] : v[k] < own)) { keep |= 1u << k; c++; }
    uint32_t incl = c;                                   // inclusive scan over the workgroup
    for (int o = 1; o < 64; o <<= 1) { const uint32_t w = __shfl_up(incl, o); if ((threadIdx.x & 63) >= (unsigned)o) incl += w; }
    if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t at = blockoff[blockIdx.x] + incl - c;
    for (unsigned w = 0; w < (threadIdx.x >> 6); w++) at += s_wave[w];
    uint32_t run = 0xFFFFFFFFu;                          // minimum LCP over the dropped ranks since the last survivor of this lane
    bool seen = false;                                   // a survivor of this lane came before
#pragma unroll
    for (int k = 0; k < 16; k++) {
        if (!(keep & (1u << k))) { run = l[k] < run ? l[k] : run; continue; }
        uint32_t m = l[k] < run ? l[k] : run;
        bool prev = seen;
        if (!seen) {                                     // the run reaches back over the lane's first rank
            uint64_t j = r0;
            while (j > skip) {
                j--;
                if (drop ? !drop[j] : sa[j] < own) { prev = true; break; }
                const uint32_t w = lcp[j];
                m = w < m ? w : m;
            }
        }
        out_sa[at] = v[k];
        out_lcp[at] = prev ? m : 0;
        at++;
        run = 0xFFFFFFFFu; seen = true;
    }
}

// the acceptance test of a window: the farthest text position any comparison between surviving neighbours touched
__global__ void __launch_bounds__(256)
k_wide_reach(const uint32_t* __restrict__ sa, const uint32_t* __restrict__ lcp, uint64_t k, unsigned long long* __restrict__ reach)
{
    __shared__ unsigned long long s_max[4];
    unsigned long long v = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < k; r += (uint64_t)gridDim.x * 256) {
        if (r == 0) continue;
        const uint32_t a = sa[r - 1], b = sa[r];
        const unsigned long long w = (unsigned long long)(a > b ? a : b) + lcp[r];
        v = w > v ? w : v;
    }
    for (int o = 32; o; o >>= 1) { const unsigned long long w = __shfl_down(v, o); v = w > v ? w : v; }
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) v = s_max[w] > v ? s_max[w] : v;
        if (v) atomicMax(reach, v);
    }
}

// the order the windows were built under
struct WideOrder {
    int mode;                    // 0 plain suffix order, 1 max_query_len, 2 seed mask
    uint32_t L;                  // mode 1: symbols compared
    const uint32_t* offs;        // mode 2: care offsets, ascending (device)
    uint32_t weight;             // mode 2: how many
};

// x against y on the whole text from `l` matched symbols on; returns x < y ? -1 : +1 and the LCP in l.  x != y.
__device__ __forceinline__ int wide_compare_plain(const uint8_t* __restrict__ t, uint64_t n, uint64_t x, uint64_t y, uint64_t& l)
{
    const uint64_t room = n - (x > y ? x : y);           // symbols of the suffix that starts later
    uint64_t k = l;
    bool diff = false;
    while (k + 8 <= room) {
        uint64_t a, b;
        __builtin_memcpy(&a, t + x + k, 8);
        __builtin_memcpy(&b, t + y + k, 8);
        if (a != b) { k += (uint64_t)(__builtin_ctzll(a ^ b) >> 3); diff = true; break; }
        k += 8;
    }
    if (!diff) while (k < room && t[x + k] == t[y + k]) k++;
    l = k;
    if (k == room) return x > y ? -1 : 1;                // the later start ran out of text: it is the smaller suffix
    return t[x + k] < t[y + k] ? -1 : 1;
}

// the same under the order of the build; `l` (symbols known to match) is a hint of the plain order only
__device__ __forceinline__ int wide_compare(const WideOrder& wo, const uint8_t* __restrict__ t, uint64_t n, uint64_t x, uint64_t y,
                                            uint64_t& l)
{
    if (wo.mode == 0) return wide_compare_plain(t, n, x, y, l);
    if (wo.mode == 1) {                                  // the first L symbols; equal ones in descending position
        const uint64_t room = n - (x > y ? x : y);
        const uint64_t lim = room < wo.L ? room : wo.L;
        uint64_t k = 0;
        while (k < lim && t[x + k] == t[y + k]) k++;
        l = k;
        if (k >= wo.L || k == room) return x > y ? -1 : 1;
        return t[x + k] < t[y + k] ? -1 : 1;
    }
    // mode 2: care symbols (k_mask_keys / k_mask_lcp; the symbols themselves stand in for the codes of a window's build --
    // same order, and one table for all windows; 0 = past the end, below every symbol)
    uint32_t c = 0, inside = 0xffffffffu;
    for (; c < wo.weight; c++) {
        const uint64_t qx = x + wo.offs[c], qy = y + wo.offs[c];
        const uint32_t cx = qx < n ? (uint32_t)t[qx] : 0u, cy = qy < n ? (uint32_t)t[qy] : 0u;
        if ((qx >= n || qy >= n) && inside == 0xffffffffu) inside = c;
        if (cx != cy) { l = c < inside ? c : inside; return cx < cy ? -1 : 1; }
    }
    l = c < inside ? c : inside;
    return x > y ? -1 : 1;
}

// number of suffixes of window `ot` below x, known to lie in [lo, hi], and the LCP of x with the last of them (0 when none)
__device__ __forceinline__ uint64_t wide_rank(const WideOrder& wo, const uint8_t* __restrict__ text, uint64_t n, const WideWindow& ot,
                                             uint64_t x, uint64_t lo, uint64_t hi, uint64_t& pred_lcp)
{
    const uint64_t lo0 = lo;
    uint64_t l = 0, rr = 0;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        uint64_t m = l < rr ? l : rr;
        if (wide_compare(wo, text, n, x, ot.base + ot.sa[mid], m) > 0) { lo = mid + 1; l = m; }
        else { hi = mid; rr = m; }
    }
    if (lo == lo0 && lo > 0) {                           // the predecessor was never probed: one comparison for its LCP
        l = 0;
        (void)wide_compare(wo, text, n, x, ot.base + ot.sa[lo - 1], l);
    }
    pred_lcp = lo > 0 ? l : 0;
    return lo;
}

static constexpr int WIDE_SAMPLE = 64;        // every 64th suffix of a window is ranked over the whole of the other windows

// coarse[o * nsamp + j]: suffixes of window o below the suffix of rank j * WIDE_SAMPLE of window `self` (o != self)
__global__ void __launch_bounds__(256)
k_wide_coarse(WideOrder wo, const uint8_t* __restrict__ text, uint64_t n, WideWindows ws, int self, uint64_t nsamp,
              uint32_t* __restrict__ coarse)
{
    const WideWindow me = ws.w[self];
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const int o = (int)blockIdx.y;
    if (j >= nsamp || o == self) return;
    const uint64_t x = me.base + me.sa[j * WIDE_SAMPLE];
    uint64_t unused;
    coarse[(uint64_t)o * nsamp + j] = (uint32_t)wide_rank(wo, text, n, ws.w[o], x, 0, ws.w[o].count, unused);
}

// place and LCP of every suffix of window `self` in the merged order; OUT = uint32_t or uint64_t.  The ranks in the
// other windows grow with the rank in this one: a suffix searches only between the counts of the two samples around it.
template <typename OUT>
__global__ void __launch_bounds__(256)
k_wide_merge(WideOrder wo, const uint8_t* __restrict__ text, uint64_t n, WideWindows ws, int self, uint64_t nsamp,
             const uint32_t* __restrict__ coarse,
             OUT* __restrict__ out_sa, OUT* __restrict__ out_lcp)
{
    const WideWindow me = ws.w[self];
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= me.count) return;
    const uint64_t x = me.base + me.sa[r];
    const uint64_t j = r / WIDE_SAMPLE;
    uint64_t place = r, best = me.lcp[r];
    for (int o = 0; o < ws.num; o++) {
        if (o == self) continue;
        const uint64_t lo = coarse[(uint64_t)o * nsamp + j];
        const uint64_t hi = j + 1 < nsamp ? coarse[(uint64_t)o * nsamp + j + 1] : ws.w[o].count;
        uint64_t l;
        place += wide_rank(wo, text, n, ws.w[o], x, lo, hi, l);
        if (l > best) best = l;
    }
    out_sa[place] = (OUT)x;
    out_lcp[place] = (OUT)best;
}

// ---- shards of a windowed build (round 5) -------------------------------------------------------------------------
// A shard is a range of the suffixes' first 8 bytes (big-endian, zeros past the end of the text): monotone in the suffix
// order (and in the order of a -m L build with L >= 8), so a shard is a contiguous range of ranks in every window and the
// shards concatenate to the whole arrays.  The range bounds are quantiles of a FIXED sample of the text (every (n / 2^20)-th
// position that starts a suffix): every rank computes the same ones from its own copy of the text, no communication.
__device__ __forceinline__ uint64_t wide_prefix8(const uint8_t* __restrict__ t, uint64_t pos, uint64_t end)
{
    uint64_t v = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) v = (v << 8) | (pos + (uint64_t)k < end ? (uint64_t)t[pos + k] : 0ull);
    return v;
}

__global__ void __launch_bounds__(256)
k_wide_sample(const uint8_t* __restrict__ t, uint64_t n, uint64_t stride, uint64_t ns, unsigned long long* __restrict__ out)
{
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < ns) out[j] = wide_prefix8(t, j * stride, n);
}

// ranks [out[0], out[1]) of a window's suffix array hold the prefixes in [lo, hi); wt = the window's text, len = its length
// (a survivor has its 8 bytes inside the window: the margin is at least 8)
__global__ void __launch_bounds__(64)
k_wide_shard_bounds(const uint8_t* __restrict__ wt, uint64_t len, const uint32_t* __restrict__ sa, uint64_t s, uint64_t lo, uint64_t hi,
                    int has_hi, unsigned long long* __restrict__ out_lo, unsigned long long* __restrict__ out_hi)
{
    if (threadIdx.x > 1) return;
    const uint64_t v = threadIdx.x ? hi : lo;
    uint64_t a = 0, b = s;                                  // first rank whose prefix is >= v
    if (threadIdx.x && !has_hi) a = s;
    while (a < b) {
        const uint64_t mid = a + (b - a) / 2;
        if (wide_prefix8(wt, sa[mid], len) < v) a = mid + 1; else b = mid;
    }
    *(threadIdx.x ? out_hi : out_lo) = a;
}

// ---- repair of a window whose comparisons ran into its end (round 5) ---------------------------------------------
// The window's build ordered the truncated suffixes text[a, len): where a's truncated suffix is a proper PREFIX of its
// successor's, the build put a first ("past the end sorts first", 372-379) although the whole text may say otherwise.
// Such a survivor is "short":   short(r)  <=>  sa[r] + lcp[r + 1] >= len   (its successor matches it up to the window's end;
// every later suffix that a is a prefix of lies between the two in the window's order, so the successor decides).
// Without the short suffixes the survivors are in whole-text order with exact LCPs: for neighbours u, v of the remaining
// list, u is not short, so u has a symbol at offset lcp(u, v) <= lcp(u, successor of u) inside the window; if v had none, v
// would be a prefix of u and stand before it.  Both have one: a real mismatch, the one the whole text shows.
__global__ void __launch_bounds__(256)
k_wide_short_mark(const uint32_t* __restrict__ sa, const uint32_t* __restrict__ lcp, uint64_t kept, uint64_t len,
                  uint8_t* __restrict__ is_short, uint8_t* __restrict__ not_short)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= kept) return;
    const bool sh = r + 1 < kept && (uint64_t)sa[r] + (uint64_t)lcp[r + 1] >= len;
    is_short[r] = sh ? 1 : 0;
    not_short[r] = sh ? 0 : 1;
}

static constexpr uint32_t WIDE_PAD = 0xFFFFFFFFu;         // padding of the bitonic network: above every suffix

// one compare-exchange stage of a bitonic network over window-local positions, ordered by whole-text comparison
__global__ void __launch_bounds__(256)
k_wide_bitonic(WideOrder wo, const uint8_t* __restrict__ text, uint64_t n, uint64_t base, uint32_t* __restrict__ v, uint32_t P,
               uint32_t k, uint32_t j)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const uint32_t l = i ^ j;
    if (l <= i) return;
    const uint32_t a = v[i], b = v[l];
    auto above = [&](uint32_t x, uint32_t y) -> bool {    // x > y in the order of the build (padding above everything)
        if (x == y || y == WIDE_PAD) return false;
        if (x == WIDE_PAD) return true;
        uint64_t m = 0;
        return wide_compare(wo, text, n, base + x, base + y, m) > 0;
    };
    const bool up = (i & k) == 0;
    if (up ? above(a, b) : above(b, a)) { v[i] = b; v[l] = a; }
}

// LCPs of the sorted list: one whole-text comparison per neighbour pair.  The list's LCP column is 32 bits wide like a window's:
// two repaired suffixes that share 2^32 - 1 symbols or more report 2^32 - 1 (the merge then takes the larger of that and the
// other windows' values: a common prefix of >= 2^32 symbols between neighbours of the merged order is under-reported).  The
// repair is exact for every repeat below 4 Gi symbols; a text with a longer exact duplicate is outside what this path claims.
__global__ void __launch_bounds__(256)
k_wide_list_lcp(WideOrder wo, const uint8_t* __restrict__ text, uint64_t n, uint64_t base, const uint32_t* __restrict__ v, uint64_t cnt,
                uint32_t* __restrict__ lcp)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= cnt) return;
    uint64_t m = 0;
    if (i > 0) (void)wide_compare(wo, text, n, base + v[i - 1], base + v[i], m);
    lcp[i] = (uint32_t)(m > 0xFFFFFFFFull ? 0xFFFFFFFFull : m);
}

// ---- two windows: one sequential merge per sample interval -------------------------------------------------------
// With two windows A and B the sample counts cut B into the ranges [c_j, c_j+1) that lie between consecutive samples
// of A: interval j of A (WIDE_SAMPLE suffixes, the sample first) and range j of B merge among themselves and with
// nothing else.  One lane merges one interval: one comparison per output suffix instead of ~7 probes.  The place of an
// output is the number of suffixes of both windows before it; its LCP is its own array's value when its predecessor
// comes from the same window, and the LCP of the comparison it just lost when the predecessor comes from the other one
// (that comparison was against exactly this suffix: it was the head of its list then).  Ranges of B above WIDE_HEAVY
// (a repeat family that lives in one window only) are queued and ranked by binary search by a workgroup each.
static constexpr uint32_t WIDE_HEAVY = 1024;

// The first 24 symbols of a list head stay in registers while it waits: a comparison that is decided inside them (the
// usual case: neighbours in the merged order of a few 10^9 suffixes share ~16 symbols) does not touch the text again.
struct WideHead { uint64_t w[3]; };
__device__ __forceinline__ WideHead wide_head_load(const uint8_t* __restrict__ t, uint64_t pos)      // the text copy is padded
{
    WideHead h;
    __builtin_memcpy(&h.w[0], t + pos, 8); __builtin_memcpy(&h.w[1], t + pos + 8, 8); __builtin_memcpy(&h.w[2], t + pos + 16, 8);
    return h;
}
// like wide_compare from 0 matched symbols, with the heads' first 24 symbols at hand
__device__ __forceinline__ int wide_compare_heads(const WideOrder& wo, const uint8_t* __restrict__ t, uint64_t n, uint64_t x,
                                                  const WideHead& hx, uint64_t y, const WideHead& hy, uint64_t& l)
{
    if (wo.mode != 0) { l = 0; return wide_compare(wo, t, n, x, y, l); }
    const uint64_t room = n - (x > y ? x : y);
    uint64_t k = 24;
#pragma unroll
    for (int i = 2; i >= 0; i--) if (hx.w[i] != hy.w[i]) k = (uint64_t)(8 * i) + (uint64_t)(__builtin_ctzll(hx.w[i] ^ hy.w[i]) >> 3);
    if (k < 24 && k < room) {                               // a real mismatch inside the text
        l = k;
        return ((hx.w[k >> 3] >> (8 * (k & 7))) & 0xFFu) < ((hy.w[k >> 3] >> (8 * (k & 7))) & 0xFFu) ? -1 : 1;
    }
    l = k < room ? k : 0;                                   // 24 equal symbols: walk on from there; near the end of the text: from 0
    return wide_compare_plain(t, n, x, y, l);
}

// A lane reads its four arrays front to back, one 4-byte element at a time, with 65 k lanes per XCD doing the same:
// every such load is its own L2 miss.  Stream4 fetches the aligned 16 bytes around an element once and serves the next
// three elements from registers.  (The blocks may start before or end after the window's part of the shared arrays:
// both sides lie inside the allocation.)
struct Stream4 {
    const uint32_t* base;
    const uint32_t* cur;             // start of the block in `blk` (16-byte aligned), nullptr: none yet
    uint4 blk;
    __device__ __forceinline__ explicit Stream4(const uint32_t* b) : base(b), cur(nullptr), blk(make_uint4(0, 0, 0, 0)) {}
    __device__ __forceinline__ uint32_t at(uint64_t idx)
    {
        // the block pointer is derived from the element pointer by arithmetic, so that it stays a global-memory pointer
        // for the compiler (a pointer rebuilt from an integer becomes generic and loads through FLAT instructions)
        const uint32_t* p = base + idx;
        const uint32_t q = (uint32_t)(reinterpret_cast<uintptr_t>(p) >> 2) & 3u;
        const uint32_t* bp = p - q;
        if (bp != cur) { blk = *reinterpret_cast<const uint4*>(bp); cur = bp; }
        return q == 0 ? blk.x : q == 1 ? blk.y : q == 2 ? blk.z : blk.w;
    }
};

// outputs leave in aligned pairs: the places of a lane are consecutive
template <typename OUT>
struct PairOut {
    OUT* sa; OUT* lcp;
    OUT psa, plcp; bool pending, paired;
    uint64_t last;
    // paired: both arrays start on a 16-byte boundary (the caller's pointers decide)
    __device__ __forceinline__ PairOut(OUT* s, OUT* l, bool p) : sa(s), lcp(l), psa(0), plcp(0), pending(false), paired(p), last(0) {}
    __device__ __forceinline__ void put(uint64_t place, OUT v, OUT w)
    {
        if (!paired) { sa[place] = v; lcp[place] = w; return; }
        if (pending) {                                   // place is odd: its even neighbour waits
            if constexpr (sizeof(OUT) == 8) {
                *reinterpret_cast<ulonglong2*>(sa + place - 1) = make_ulonglong2(psa, v);
                *reinterpret_cast<ulonglong2*>(lcp + place - 1) = make_ulonglong2(plcp, w);
            } else {
                *reinterpret_cast<uint2*>(sa + place - 1) = make_uint2(psa, v);
                *reinterpret_cast<uint2*>(lcp + place - 1) = make_uint2(plcp, w);
            }
            pending = false;
        } else if ((place & 1) == 0) { psa = v; plcp = w; pending = true; last = place; }
        else { sa[place] = v; lcp[place] = w; }
    }
    __device__ __forceinline__ void flush() { if (pending) { sa[last] = psa; lcp[last] = plcp; pending = false; } }
};

// the suffixes of B below the first sample of A keep their ranks
template <typename OUT>
__global__ void __launch_bounds__(256)
k_wide_head(WideWindow b, uint64_t count, OUT* __restrict__ out_sa, OUT* __restrict__ out_lcp)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= count) return;
    out_sa[k] = (OUT)(b.base + b.sa[k]);
    out_lcp[k] = (OUT)b.lcp[k];
}

template <typename OUT>
__global__ void __launch_bounds__(256)
k_wide_seqmerge(WideOrder wo, const uint8_t* __restrict__ text, uint64_t n, WideWindow a, WideWindow b, uint64_t nsamp,
                const uint32_t* __restrict__ coarse, uint32_t* __restrict__ heavy, unsigned long long* __restrict__ nheavy,
                OUT* __restrict__ out_sa, OUT* __restrict__ out_lcp)
{
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nsamp) return;
    uint64_t i = j * WIDE_SAMPLE;
    const uint64_t a_hi = i + WIDE_SAMPLE < a.count ? i + WIDE_SAMPLE : a.count;
    uint64_t k = coarse[j];
    const uint64_t b_hi = j + 1 < nsamp ? coarse[j + 1] : b.count;
    if (b_hi - k > WIDE_HEAVY) { heavy[atomicAdd(nheavy, 1ull)] = (uint32_t)j; return; }
    // the sample opens the interval: every suffix of the range is above it; its predecessor is the suffix of A before
    // it or the last suffix of B below it
    Stream4 asa(a.sa), alcp(a.lcp), bsa(b.sa), blcp(b.lcp);
    PairOut<OUT> out(out_sa, out_lcp, (((uintptr_t)out_sa | (uintptr_t)out_lcp) & 15u) == 0);
    uint64_t x = a.base + asa.at(i);
    {
        uint64_t best = alcp.at(i);
        if (k > 0) {
            uint64_t l = 0;
            (void)wide_compare(wo, text, n, x, b.base + b.sa[k - 1], l);
            best = l > best ? l : best;
        }
        out.put(i + k, (OUT)x, (OUT)best);
        i++;
    }
    bool prev_a = true;               // which window the previous output came from
    uint64_t cross = 0;               // LCP of the last comparison: loser (still a head) against winner (the previous output)
    uint64_t y = k < b_hi ? b.base + bsa.at(k) : 0;
    WideHead hx = wide_head_load(text, x), hy = wide_head_load(text, y);
    if (k < b_hi) (void)wide_compare_heads(wo, text, n, x, hx, y, hy, cross);      // the sample against the head of the range
    if (i < a_hi) { x = a.base + asa.at(i); hx = wide_head_load(text, x); }
    while (i < a_hi || k < b_hi) {
        bool take_a;
        uint64_t h = 0;
        if (i == a_hi) take_a = false;
        else if (k == b_hi) take_a = true;
        else take_a = wide_compare_heads(wo, text, n, x, hx, y, hy, h) < 0;
        if (take_a) {
            out.put(i + k, (OUT)x, (OUT)(prev_a ? (uint64_t)alcp.at(i) : cross));
            i++;
            if (i < a_hi) { x = a.base + asa.at(i); hx = wide_head_load(text, x); }
            prev_a = true;
        } else {
            out.put(i + k, (OUT)y, (OUT)(prev_a ? cross : (uint64_t)blcp.at(k)));
            k++;
            if (k < b_hi) { y = b.base + bsa.at(k); hy = wide_head_load(text, y); }
            prev_a = false;
        }
        cross = h;                    // (0 when one list was exhausted: the next output then follows its own window)
    }
    out.flush();
}

// a queued interval: its suffixes of A rank themselves in the range of B, the range of B ranks itself among them
template <typename OUT>
__global__ void __launch_bounds__(256)
k_wide_heavy(WideOrder wo, const uint8_t* __restrict__ text, uint64_t n, WideWindow a, WideWindow b, uint64_t nsamp,
             const uint32_t* __restrict__ coarse, const uint32_t* __restrict__ heavy, OUT* __restrict__ out_sa, OUT* __restrict__ out_lcp)
{
    const uint64_t j = heavy[blockIdx.x];
    const uint64_t a_lo = j * WIDE_SAMPLE, a_hi = a_lo + WIDE_SAMPLE < a.count ? a_lo + WIDE_SAMPLE : a.count;
    const uint64_t b_lo = coarse[j], b_hi = j + 1 < nsamp ? coarse[j + 1] : b.count;
    for (uint64_t i = a_lo + threadIdx.x; i < a_hi; i += 256) {
        const uint64_t x = a.base + a.sa[i];
        uint64_t l;
        const uint64_t c = wide_rank(wo, text, n, b, x, b_lo, b_hi, l);
        const uint64_t own = a.lcp[i];
        out_sa[i + c] = (OUT)x; out_lcp[i + c] = (OUT)(l > own ? l : own);
    }
    for (uint64_t k = b_lo + threadIdx.x; k < b_hi; k += 256) {
        const uint64_t y = b.base + b.sa[k];
        uint64_t l;
        const uint64_t c = wide_rank(wo, text, n, a, y, a_lo + 1, a_hi, l);      // the sample itself is below the whole range
        const uint64_t own = b.lcp[k];
        out_sa[k + c] = (OUT)y; out_lcp[k + c] = (OUT)(l > own ? l : own);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
struct WidePlan { uint64_t H; uint64_t margin; int num; };

// windows of equal size, as few as fit; the margin is what the caller set or 2^26
inline WidePlan wide_plan(uint64_t n, uint64_t window, uint64_t margin)
{
    const uint64_t limit = SUFR_MAX_TEXT_LEN - 1;
    WidePlan p;
    p.margin = margin ? margin : ((uint64_t)1 << 26);
    if (window) { if (window > limit - 1) window = limit - 1; if (p.margin > limit - window) p.margin = limit - window; }
    else {
        if (p.margin > limit / 2) p.margin = limit / 2;
        window = limit - p.margin;
    }
    const uint64_t cnt = (n + window - 1) / window;
    p.H = (n + cnt - 1) / cnt;                               // equal windows: H <= window
    p.H = (p.H + 15) & ~(uint64_t)15;                        // window bases stay 16-byte aligned (vector loads of the text)
    const uint64_t num = (n + p.H - 1) / p.H;
    p.num = num > (uint64_t)WIDE_MAX_WINDOWS ? -1 : (int)num;
    return p;
}

// The repair of one window (header comment): out_sa / out_lcp hold its `kept` survivors; on return they hold the *nrest
// that are not short (in whole-text order, exact LCPs) and *l_sa / *l_lcp the *nshort short ones, sorted over the whole text.
template <typename ORPH>
int repair_window(Pipeline& pl, const WideOrder& wo, const uint8_t* t, uint64_t n, uint64_t base, uint64_t len, uint32_t* out_sa,
                  uint32_t* out_lcp, uint64_t kept, DevBuf& wblk, ORPH& orphans, uint32_t** l_sa, uint32_t** l_lcp, uint64_t* nshort,
                  uint64_t* nrest)
{
    hipStream_t st = pl.stream;
    int rc;
    // scratch: the survivors as they are (the window's raw arrays are not needed any more), two flag arrays
    if ((rc = pl.ensure(pl.sa32, kept * 4 + 4)) || (rc = pl.ensure(pl.lcp32, kept * 4 + 4))) return rc;
    uint8_t* flags = nullptr;
    if (hipMalloc((void**)&flags, kept * 2 + 16) != hipSuccess) { pl.set_error("out of device memory (window repair)"); return SUFR_HIP_E_NOMEM; }
    orphans.bufs.push_back(flags);
    uint8_t *is_short = flags, *not_short = flags + kept;
    if (hipMemcpyAsync(pl.sa32.p, out_sa, kept * 4, hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemcpyAsync(pl.lcp32.p, out_lcp, kept * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) { pl.set_error("window repair: copy failed"); return SUFR_HIP_E_HIP; }
    hipLaunchKernelGGL(k_wide_short_mark, dim3((uint32_t)((kept + 255) / 256)), dim3(256), 0, st, (const uint32_t*)pl.sa32.p,
                       (const uint32_t*)pl.lcp32.p, kept, len, is_short, not_short);
    const uint32_t nblk = (uint32_t)((kept + WIDE_BLK - 1) / WIDE_BLK);
    if ((rc = pl.ensure(wblk, (size_t)nblk * 4))) return rc;
    // how many are short
    unsigned long long cnt = 0;
    hipLaunchKernelGGL(k_wide_count, dim3(nblk), dim3(256), 0, st, (const uint32_t*)pl.sa32.p, kept, 0u, (uint32_t*)wblk.p, (const uint8_t*)not_short);
    hipLaunchKernelGGL(k_wide_scan, dim3(1), dim3(1024), 0, st, (uint32_t*)wblk.p, nblk, pl.sc(Pipeline::SC_TOTAL));
    if (hipMemcpyAsync(&cnt, pl.sc(Pipeline::SC_TOTAL), 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        pl.set_error("window repair: counting failed"); return SUFR_HIP_E_HIP;
    }
    *nshort = cnt; *nrest = kept - cnt;
    if (cnt > ((uint64_t)1 << 22)) return SUFR_HIP_E_UNSUPPORTED;
    uint32_t P = 1;
    while (P < cnt) P <<= 1;
    uint32_t* list = nullptr;
    if (hipMalloc((void**)&list, ((size_t)P * 2 + 4) * 4) != hipSuccess) { pl.set_error("out of device memory (window repair)"); return SUFR_HIP_E_NOMEM; }
    orphans.bufs.push_back(list);
    *l_sa = list; *l_lcp = list + P;
    if (hipMemsetAsync(list, 0xFF, (size_t)P * 4, st) != hipSuccess) { pl.set_error("memset failed"); return SUFR_HIP_E_HIP; }
    // the short ones -> list (their LCP column is recomputed below); the others -> back to out_sa / out_lcp, LCP = minimum over
    // the ranks taken out between two of them
    hipLaunchKernelGGL(k_wide_compact, dim3(nblk), dim3(256), 0, st, (const uint32_t*)pl.sa32.p, (const uint32_t*)pl.lcp32.p, kept, 0u,
                       (const uint32_t*)wblk.p, *l_sa, *l_lcp, (const uint8_t*)not_short);
    hipLaunchKernelGGL(k_wide_count, dim3(nblk), dim3(256), 0, st, (const uint32_t*)pl.sa32.p, kept, 0u, (uint32_t*)wblk.p, (const uint8_t*)is_short);
    hipLaunchKernelGGL(k_wide_scan, dim3(1), dim3(1024), 0, st, (uint32_t*)wblk.p, nblk, pl.sc(Pipeline::SC_TOTAL));
    hipLaunchKernelGGL(k_wide_compact, dim3(nblk), dim3(256), 0, st, (const uint32_t*)pl.sa32.p, (const uint32_t*)pl.lcp32.p, kept, 0u,
                       (const uint32_t*)wblk.p, out_sa, out_lcp, (const uint8_t*)is_short);
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1)
            hipLaunchKernelGGL(k_wide_bitonic, dim3((P + 255) / 256), dim3(256), 0, st, wo, t, n, base, *l_sa, P, k, j);
    if (cnt) hipLaunchKernelGGL(k_wide_list_lcp, dim3((uint32_t)((cnt + 255) / 256)), dim3(256), 0, st, wo, t, n, base, (const uint32_t*)*l_sa, (uint64_t)cnt, *l_lcp);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { pl.set_error("window repair failed"); return SUFR_HIP_E_HIP; }
    return 0;
}

template <typename OUT>
int sort_device_wide(Pipeline& pl, const void* d_in, uint64_t n, uint32_t flags, uint64_t window, uint64_t margin, OUT* d_sa,
                     OUT* d_lcp, uint64_t cap, uint64_t* num_suffixes_out, sufr_hip_stats* st_out, DevBuf& wtext, DevBuf& wsa,
                     DevBuf& wlcp, DevBuf& wblk)
{
    if (num_suffixes_out) *num_suffixes_out = 0;
    if (!d_in) { pl.set_error("null text"); return SUFR_HIP_E_INVALID; }
    if (hipSetDevice(pl.device) != hipSuccess) { pl.set_error("hipSetDevice failed"); return SUFR_HIP_E_HIP; }
    struct NotResident { Pipeline& p; ~NotResident() { p.resident_text_len = 0; } } not_resident{pl};   // (pl.text ends up holding a window)
    pl.wide_text_len = 0;                                    // (set again when the build succeeds: what the shard stitch checks)
    // (sufr_hip_overlapped / sufr_hip_doublings speak of the whole build: every window's build adds to them)
    // (so do sufr_hip_exc_retry -- the largest over the windows -- and sufr_hip_exc_taken -- the last window that took ranks out)
    struct Chains { Pipeline& p; uint32_t overlapped = 0; uint64_t doublings = 0; uint32_t exc_retry = 0; uint64_t exc_taken = 0, pairs_resolved = 0, pairs_left = 0;
                    ~Chains() { p.last_pairs_resolved = pairs_resolved; p.last_pairs_left = pairs_left; p.last_overlapped = overlapped; p.last_doublings = doublings; p.last_exc_retry = exc_retry; p.last_exc_taken = exc_taken; } } chains{pl};
    WidePlan plan = wide_plan(n, window, margin);
    // the order of the build: a window must hold every symbol a comparison of its own suffixes looks at
    WideOrder wo = {0, 0u, nullptr, 0u};
    if (!pl.opt_mask_offsets.empty()) {
        wo.mode = 2; wo.weight = (uint32_t)pl.opt_mask_offsets.size();
        const uint64_t span = (uint64_t)pl.opt_mask_offsets.back() + 1;
        if (plan.margin < span) {
            // a window must hold the care symbols of every suffix it owns: H + span symbols.  wide_plan clamped the margin to what
            // 32 bits leave beside the window; where the span does not fit there, the windows shrink instead (a clipped window
            // would compare its last suffixes against padding, and the masked LCP cannot tell: it counts care symbols, not text).
            // Equal windows reach that size only for texts of ~2 x 2^32 bytes and more: beyond what one device holds today.
            const uint64_t limit = SUFR_MAX_TEXT_LEN - 1;
            if (span + 64 > limit) { pl.set_error("seed mask spans more symbols than a window holds"); return SUFR_HIP_E_UNSUPPORTED; }
            if (plan.H + span > limit) plan = wide_plan(n, limit - span - 16, span);
            if (plan.margin < span) plan.margin = span;
        }
    } else if (pl.opt_max_query_len > 0) {
        // (an L beyond 32 bits never ties two suffixes of a window: the plain order)
        if (pl.opt_max_query_len < 0xFFFFFFFFull) { wo.mode = 1; wo.L = (uint32_t)pl.opt_max_query_len; }
    }
    if (plan.num < 1) { pl.set_error("text too long for " + std::to_string(WIDE_MAX_WINDOWS) + " windows"); return SUFR_HIP_E_UNSUPPORTED; }
    hipStream_t st = pl.stream;
    int rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { pl.set_error("hipEventCreate failed"); return SUFR_HIP_E_HIP; }
    struct Ev { hipEvent_t a, b; ~Ev() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } evguard{e0, e1};
    (void)hipEventRecord(e0, st);
    // the normalised text, padded: every window and the merge read this copy
    if ((rc = pl.ensure(wtext, n + TEXT_PAD))) return rc;
    uint8_t* t = (uint8_t*)wtext.p;
    {
        uint64_t grid = (n / 16 + 255) / 256;
        if (grid > 8192) grid = 8192;
        if (grid < 1) grid = 1;
        if ((uintptr_t)d_in & 15u) {                         // vector loads want an aligned source: copy, then map in place
            if (hipMemcpyAsync(t, d_in, n, hipMemcpyDeviceToDevice, st) != hipSuccess) { pl.set_error("text copy failed"); return SUFR_HIP_E_HIP; }
            d_in = t;
        }
        hipLaunchKernelGGL(k_wide_normalize, dim3((uint32_t)grid), dim3(256), 0, st, (const uint8_t*)d_in, t, n,
                           (flags & SUFR_HIP_FLAG_RAW_TEXT) ? 1 : 0, (flags & SUFR_HIP_FLAG_IGNORE_SOFTMASK) ? 1 : 0);
        if (hipMemsetAsync(t + n, 0, TEXT_PAD, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
            pl.set_error("normalising the text failed"); return SUFR_HIP_E_HIP;
        }
    }
    const uint32_t wflags = flags & ~(uint32_t)SUFR_HIP_FLAG_RAW_TEXT;
    // the windows' surviving ranks, all windows behind one another: n entries for a whole build, about a shard's share for a shard
    // (round 5: 8 n bytes per shard were the ceiling of the out-of-core create); grown, contents kept, when a window needs more
    uint64_t wcap = n;
    if (pl.wide_num_shards > 1) {
        wcap = n / pl.wide_num_shards + n / (2ull * pl.wide_num_shards) + ((uint64_t)1 << 20);
        if (wcap > n) wcap = n;
    }
    if ((rc = pl.ensure(wsa, wcap * 4 + 16)) || (rc = pl.ensure(wlcp, wcap * 4 + 16))) return rc;
    if ((rc = pl.ensure(pl.scalars, Pipeline::SC_N * 8))) return rc;
    // ---- the shard of this call: a range [sh_lo, sh_hi) of 8-byte prefixes (k_wide_sample, above) ----
    const bool sharded = pl.wide_num_shards > 1;
    uint64_t sh_lo = 0, sh_hi = 0;
    bool sh_has_hi = false;
    if (sharded) {
        if (wo.mode == 2) { pl.set_error("seed-mask builds in windows are built on one GPU"); return SUFR_HIP_E_UNSUPPORTED; }
        if (wo.mode == 1 && wo.L < 8) { pl.set_error("a max_query_len below 8 symbols ties suffixes across shards: built on one GPU"); return SUFR_HIP_E_UNSUPPORTED; }
        if (pl.opt_max_query_len > 0 && pl.opt_max_query_len < 8) { pl.set_error("a max_query_len below 8 symbols ties suffixes across shards: built on one GPU"); return SUFR_HIP_E_UNSUPPORTED; }
        if (plan.margin < 8) plan.margin = 8;                // a survivor's 8 bytes lie inside its window
        const uint64_t ns = n < ((uint64_t)1 << 20) ? n : ((uint64_t)1 << 20), stride = n / ns;
        if ((rc = pl.ensure(wblk, (size_t)ns * 8))) return rc;
        hipLaunchKernelGGL(k_wide_sample, dim3((uint32_t)((ns + 255) / 256)), dim3(256), 0, st, (const uint8_t*)t, n, stride, ns, (unsigned long long*)wblk.p);
        std::vector<uint64_t> smp(ns);
        if (hipMemcpyAsync(smp.data(), wblk.p, (size_t)ns * 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
            pl.set_error("sampling the text failed"); return SUFR_HIP_E_HIP;
        }
        if ((flags & SUFR_HIP_FLAG_DNA) && !(flags & SUFR_HIP_FLAG_ALLOW_AMBIGUITY)) {       // eligibility 446-449: a property of the first byte
            size_t k = 0;
            for (uint64_t v : smp) { const uint8_t c = (uint8_t)(v >> 56); if (c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == '$') smp[k++] = v; }
            smp.resize(k);
        }
        std::sort(smp.begin(), smp.end());
        auto cut = [&](uint32_t k) -> uint64_t { return smp.empty() ? 0ull : smp[(size_t)((unsigned __int128)smp.size() * k / pl.wide_num_shards)]; };
        sh_lo = pl.wide_shard_index ? cut(pl.wide_shard_index) : 0ull;
        sh_has_hi = pl.wide_shard_index + 1 < pl.wide_num_shards;
        sh_hi = sh_has_hi ? cut(pl.wide_shard_index + 1) : 0ull;
    }
    WideWindows ws;
    ws.num = plan.num;
    pl.wide_orphans = 0;
    struct Orphans { std::vector<void*> bufs; ~Orphans() { for (void* q : bufs) (void)hipFree(q); } } orphans;     // the repair lists live until the merge is done
    uint64_t kept_total = 0;
    uint64_t woff[WIDE_MAX_WINDOWS] = {0};
    sufr_hip_stats acc;
    memset(&acc, 0, sizeof acc);
    for (int i = 0; i < plan.num; i++) {
        const uint64_t base = (uint64_t)i * plan.H;
        const uint64_t own = n - base < plan.H ? n - base : plan.H;
        const uint64_t limit = SUFR_MAX_TEXT_LEN - 1;
        uint64_t m = plan.margin;
        for (int attempt = 0;; attempt++) {
            uint64_t len = own + m;
            if (len > n - base) len = n - base;
            if (len > limit) len = limit;
            const bool to_end = base + len == n;
            if ((rc = pl.ensure(pl.sa32, len * 4 + 4)) || (rc = pl.ensure(pl.lcp32, len * 4 + 4))) return rc;
            uint64_t s = 0;
            sufr_hip_stats wst;
            rc = pl.sort_device_u32(t + base, len, wflags, 0, 1, (uint32_t*)pl.sa32.p, (uint32_t*)pl.lcp32.p, len, &s, &wst);
            chains.overlapped |= pl.last_overlapped; chains.doublings += pl.last_doublings;
            chains.pairs_resolved += pl.last_pairs_resolved; chains.pairs_left += pl.last_pairs_left;
            if (pl.last_exc_retry > chains.exc_retry) chains.exc_retry = pl.last_exc_retry;
            if (pl.last_exc_taken) chains.exc_taken = pl.last_exc_taken;
            if (rc) return rc;
            if (i == 0 && attempt == 0) acc = wst;
            else { acc.ms_total += wst.ms_total; acc.ms_normalize += wst.ms_normalize; acc.ms_hist_text += wst.ms_hist_text;
                   acc.ms_partition += wst.ms_partition; acc.ms_passes += wst.ms_passes; acc.ms_finish += wst.ms_finish;
                   acc.ms_deep += wst.ms_deep; acc.deep_records += wst.deep_records; acc.num_large_groups += wst.num_large_groups;
                   if (wst.num_levels > acc.num_levels) acc.num_levels = wst.num_levels; }
            unsigned long long kept = 0, reach = 0;
            // a shard keeps the ranks whose 8-byte prefix lies in its range; the filter starts at the 16-byte boundary below them
            const uint32_t* fsa = (const uint32_t*)pl.sa32.p;
            const uint32_t* flcp = (const uint32_t*)pl.lcp32.p;
            uint32_t skip = 0;
            if (sharded && s) {
                unsigned long long rb[2] = {0, 0};
                hipLaunchKernelGGL(k_wide_shard_bounds, dim3(1), dim3(64), 0, st, (const uint8_t*)(t + base), len, fsa, s, sh_lo, sh_hi,
                                   sh_has_hi ? 1 : 0, pl.sc(Pipeline::SC_TOTAL), pl.sc(Pipeline::SC_BAD));
                if (hipMemcpyAsync(&rb[0], pl.sc(Pipeline::SC_TOTAL), 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
                    hipMemcpyAsync(&rb[1], pl.sc(Pipeline::SC_BAD), 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
                    hipStreamSynchronize(st) != hipSuccess) { pl.set_error("finding the shard's ranks failed"); return SUFR_HIP_E_HIP; }
                if (rb[1] < rb[0]) rb[1] = rb[0];
                const uint64_t a0 = rb[0] & ~(uint64_t)3;
                skip = (uint32_t)(rb[0] - a0);
                fsa += a0; flcp += a0;
                s = rb[1] - a0;
                if (s <= skip) s = 0;
            }
            // room for this window's survivors (at most s of them) behind those of the windows before it
            if ((kept_total + s) * 4 + 16 > wsa.cap || (kept_total + s) * 4 + 16 > wlcp.cap) {
                const uint64_t want = kept_total + s + ((kept_total + s) >> 3);
                if ((rc = pl.ensure_keep(wsa, (want < n ? want : n) * 4 + 16)) || (rc = pl.ensure_keep(wlcp, (want < n ? want : n) * 4 + 16))) return rc;
            }
            uint32_t* out_sa = (uint32_t*)wsa.p + kept_total;
            uint32_t* out_lcp = (uint32_t*)wlcp.p + kept_total;
            if (s) {
                const uint32_t nblk = (uint32_t)((s + WIDE_BLK - 1) / WIDE_BLK);
                if ((rc = pl.ensure(wblk, (size_t)nblk * 4))) return rc;
                hipLaunchKernelGGL(k_wide_count, dim3(nblk), dim3(256), 0, st, fsa, s, (uint32_t)own, (uint32_t*)wblk.p, (const uint8_t*)nullptr, skip);
                hipLaunchKernelGGL(k_wide_scan, dim3(1), dim3(1024), 0, st, (uint32_t*)wblk.p, nblk, pl.sc(Pipeline::SC_TOTAL));
                hipLaunchKernelGGL(k_wide_compact, dim3(nblk), dim3(256), 0, st, fsa, flcp, s,
                                   (uint32_t)own, (const uint32_t*)wblk.p, out_sa, out_lcp, (const uint8_t*)nullptr, skip);
                if (hipMemcpyAsync(&kept, pl.sc(Pipeline::SC_TOTAL), 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
                    hipStreamSynchronize(st) != hipSuccess) { pl.set_error("filtering a window failed"); return SUFR_HIP_E_HIP; }
                if (!to_end && kept > 1) {
                    if (hipMemsetAsync(pl.sc(Pipeline::SC_BAD), 0, 8, st) != hipSuccess) { pl.set_error("memset failed"); return SUFR_HIP_E_HIP; }
                    const uint64_t rblk = (kept + 255) / 256;
                    hipLaunchKernelGGL(k_wide_reach, dim3((uint32_t)(rblk < 4096 ? rblk : 4096)), dim3(256), 0, st, (const uint32_t*)out_sa,
                                       (const uint32_t*)out_lcp, (uint64_t)kept, pl.sc(Pipeline::SC_BAD));
                    if (hipMemcpyAsync(&reach, pl.sc(Pipeline::SC_BAD), 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
                        hipStreamSynchronize(st) != hipSuccess) { pl.set_error("checking a window failed"); return SUFR_HIP_E_HIP; }
                }
            }
            if (!to_end && reach >= len) {                   // a comparison ran into the end of the window
                uint64_t widest = limit - own < n - base - own ? limit - own : n - base - own;
                if (pl.opt_wide_retry && widest > pl.opt_wide_retry) widest = pl.opt_wide_retry;
                if (attempt == 0 && widest > m) { m = widest; continue; }
                // the widest margin did not reach over the repeat: the short suffixes leave the window's arrays and come back
                // as a list of their own, ordered over the whole text (header comment; k_wide_short_mark)
                if (wo.mode == 2) {
                    pl.set_error("a seed-mask window ran into its end (the margin covers the mask's span: this cannot happen)");
                    return SUFR_HIP_E_HIP;
                }
                if (ws.num >= WIDE_MAX_WINDOWS) { pl.set_error("too many windows need a repair list"); return SUFR_HIP_E_UNSUPPORTED; }
                uint32_t *l_sa = nullptr, *l_lcp = nullptr;
                uint64_t nshort = 0, nrest = 0;
                if ((rc = repair_window(pl, wo, t, n, base, len, out_sa, out_lcp, (uint64_t)kept, wblk, orphans, &l_sa, &l_lcp, &nshort, &nrest))) {
                    if (rc == SUFR_HIP_E_UNSUPPORTED)
                        pl.set_error("a repeat of " + std::to_string(reach - own) + " or more symbols crosses the end of window " + std::to_string(i) +
                                     " and ties " + std::to_string(nshort) + " suffixes through it: more than the whole-text repair takes (2^22)");
                    return rc;
                }
                ws.w[ws.num++] = {l_sa, l_lcp, base, nshort};
                pl.wide_orphans += nshort;
                kept = nrest;
            }
            ws.w[i] = {nullptr, nullptr, base, (uint64_t)kept};      // (its place in wsa / wlcp: woff[i]; the arrays may still move)
            woff[i] = kept_total;
            kept_total += kept;
            break;
        }
    }
    for (int i = 0; i < plan.num; i++) { ws.w[i].sa = (const uint32_t*)wsa.p + woff[i]; ws.w[i].lcp = (const uint32_t*)wlcp.p + woff[i]; }
    for (int i = plan.num; i < ws.num; i++) kept_total += ws.w[i].count;      // (the repair lists are suffixes of the output too)
    if (num_suffixes_out) *num_suffixes_out = kept_total;
    if (kept_total > cap) {
        pl.set_error("output capacity " + std::to_string(cap) + " < num_suffixes " + std::to_string(kept_total));
        return SUFR_HIP_E_CAPACITY;
    }
    if (wo.mode == 2) {
        if ((rc = pl.ensure(pl.wideoffs, (size_t)wo.weight * 4))) return rc;
        if (hipMemcpyAsync(pl.wideoffs.p, pl.opt_mask_offsets.data(), (size_t)wo.weight * 4, hipMemcpyHostToDevice, st) != hipSuccess) {
            pl.set_error("uploading the mask offsets failed"); return SUFR_HIP_E_HIP;
        }
        wo.offs = (const uint32_t*)pl.wideoffs.p;
    }
    if (ws.num == 2 && ws.w[0].count && ws.w[1].count) {
        // two windows: sample ranks of A in B, then one sequential merge per interval (heavy ranges queued)
        const WideWindow A = ws.w[0], B = ws.w[1];
        const uint64_t nsamp = (A.count + WIDE_SAMPLE - 1) / WIDE_SAMPLE;
        if ((rc = pl.ensure(wblk, (size_t)nsamp * 2 * 4 * 2))) return rc;
        uint32_t* coarse = (uint32_t*)wblk.p;                 // [2][nsamp]: k_wide_coarse writes row 1 (window 1 seen from window 0)
        uint32_t* heavy = coarse + 2 * nsamp;
        if (hipMemsetAsync(pl.sc(Pipeline::SC_TOTAL), 0, 8, st) != hipSuccess) { pl.set_error("memset failed"); return SUFR_HIP_E_HIP; }
        hipLaunchKernelGGL(k_wide_coarse, dim3((uint32_t)((nsamp + 255) / 256), 2u), dim3(256), 0, st, wo, (const uint8_t*)t, n, ws, 0, nsamp, coarse);
        hipLaunchKernelGGL((k_wide_seqmerge<OUT>), dim3((uint32_t)((nsamp + 255) / 256)), dim3(256), 0, st, wo, (const uint8_t*)t, n, A, B, nsamp,
                           (const uint32_t*)(coarse + nsamp), heavy, pl.sc(Pipeline::SC_TOTAL), d_sa, d_lcp);
        uint32_t first = 0;                                   // suffixes of B below the first sample of A
        unsigned long long nheavy = 0;
        if (hipMemcpyAsync(&first, coarse + nsamp, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(&nheavy, pl.sc(Pipeline::SC_TOTAL), 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) { pl.set_error("merging the windows failed"); return SUFR_HIP_E_HIP; }
        if (first) hipLaunchKernelGGL((k_wide_head<OUT>), dim3((first + 255u) / 256u), dim3(256), 0, st, B, (uint64_t)first, d_sa, d_lcp);
        if (nheavy) hipLaunchKernelGGL((k_wide_heavy<OUT>), dim3((uint32_t)nheavy), dim3(256), 0, st, wo, (const uint8_t*)t, n, A, B, nsamp,
                                       (const uint32_t*)(coarse + nsamp), (const uint32_t*)heavy, d_sa, d_lcp);
    } else
    for (int i = 0; i < ws.num; i++) {
        if (!ws.w[i].count) continue;
        const uint64_t nsamp = (ws.w[i].count + WIDE_SAMPLE - 1) / WIDE_SAMPLE;
        if ((rc = pl.ensure(wblk, (size_t)nsamp * ws.num * 4))) return rc;
        hipLaunchKernelGGL(k_wide_coarse, dim3((uint32_t)((nsamp + 255) / 256), (uint32_t)ws.num), dim3(256), 0, st, wo, (const uint8_t*)t, n, ws, i,
                           nsamp, (uint32_t*)wblk.p);
        hipLaunchKernelGGL((k_wide_merge<OUT>), dim3((uint32_t)((ws.w[i].count + 255) / 256)), dim3(256), 0, st, wo, (const uint8_t*)t, n, ws, i,
                           nsamp, (const uint32_t*)wblk.p, d_sa, d_lcp);
    }
    (void)hipEventRecord(e1, st);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { pl.set_error("merging the windows failed"); return SUFR_HIP_E_HIP; }
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    acc.text_len = n; acc.num_suffixes = kept_total; acc.ms_total = ms;
    if (st_out) *st_out = acc;
    pl.wide_text_len = n;                                    // wtext holds the normalised text of this build
    return 0;
}

}  // namespace sufr
