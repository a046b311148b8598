// sufr_exc.inc -- DNA texts with a few bytes outside {$ % A C G N T} stay on the fixed 3-bit code table (round 6; included by
// sufr_kernels.hip after sufr_wide.inc, whose whole-text comparison kernels it shares).
//
// An NCBI GRCh38 carries IUPAC ambiguity codes at a few dozen positions, and any `-D` delimiter other than '%' is such a byte
// too.  Until round 5 one of them sent the whole build to the general code table: 4- or 5-bit codes, 16 or 12 characters per
// key, the text-staging partition kernels -- 64 ms ('#' delimiters) to 278 ms (ten IUPAC letters) against 52 ms on the 3.1 Gb
// stand-in (profiles/r06_input_classes.txt).  Now k_text_pass_dna writes 'N' in their place and lists them: the pipeline builds
// the exact arrays SA', LCP' of that text T' (same eligibility: 'N' starts a suffix iff the foreign byte does,
// sufr_builder.rs:446-449), the bytes are put back, and the suffixes whose comparisons REACHED a listed position are re-placed:
//
//   * rank r is AFFECTED iff [SA'[r], SA'[r] + max(LCP'[r], LCP'[r + 1])] holds a listed position: the comparisons of T' with its
//     two neighbours (hence with every other suffix: the common prefix with anything farther is no longer) read only positions
//     at which T and T' agree otherwise;
//   * two unaffected suffixes x, y compare in T as in T': lcp'(x, y) <= min(reach(x), reach(y)), no listed position in either
//     window, the mismatch is the same byte pair.  Without the affected ranks SA' is therefore in the order of T, and the LCP of
//     two survivors is the minimum over the ranks taken out between them (k_exc_merge);
//   * the affected suffixes are sorted by comparisons on T itself (k_wide_bitonic / wide_compare_plain of sufr_wide.inc) and
//     each finds its place among the survivors by binary search (k_exc_rank); one streaming pass writes the final arrays,
//     shifted by the insertions before them, with the LCPs at the seams from one direct comparison each.
//
// Finding the affected ranks without reading the arrays (single-shard builds; k_exc_pmin / k_exc_expand): a suffix is affected
// iff its longest common prefix with ANY other suffix of T' reaches the first listed position f at or after it, M(p) >= f - p.
// Going down from f over the positions that start a suffix this is MONOTONE: if some q shares f - p symbols with suffix p, then
// q + d shares f - p - d symbols with suffix p + d, and q + d starts a suffix because it starts with the byte p + d starts with
// (eligibility is a property of the first byte, sufr_builder.rs:446-449) -- the argument of Kasai's LCP algorithm.  So the
// affected suffixes before f are the suffix starts in [p*(f), f]: p* by a galloping + binary search over positions, each probe
// one binary search of the suffix in SA' (its rank; comparisons on T', run-aware) and two LCP' reads.  A few thousand probes
// for 50 listed bytes instead of a pass over 12 GB (k_exc_mark: 3.4 ms, still used by sharded builds, whose arrays hold only
// their own suffixes).
//
// Which byte T' carries at a listed position does not matter for correctness (no surviving comparison looks at it).  Cost on the
// 3.1 Gb stand-in with 50 IUPAC bytes: one read of SA' / LCP' to mark, one read + one write to merge (~8 ms); nothing when the
// text has no such byte.  More than EXC_MAX_LIST listed positions or more than 2^22 affected suffixes take the general code
// table as before.  The second limit can be lowered (sufr_hip_set_exc_max_affected; never raised: the list and the whole-text
// sort are sized for 2^22): exc_reinsert compares against it in three places -- (1) the position ranges of k_exc_pmin, 16 x the
// limit, before the listed bytes are put back; (2) the ranks taken out; (3) in a shard, the suffixes left to place -- and
// records which one gave up (Pipeline::last_exc_retry, last_exc_taken).  Pipeline::reinsert_listed then puts back what is still
// 'N' and builds the text again from the caller's pointer.
//
// Shards (first-digit ranges, identical on every rank): a suffix with a listed byte among its first D characters may belong to
// another shard than the one its 'N' form was built in.  Every rank takes ALL suffixes with a listed byte among their first D
// characters out of its arrays (k_exc_mark: a reach of at least D - 1), keeps of the taken ones those whose TRUE first D bytes
// lie in its range, and adds the ones of the other shards' that do (k_exc_shard_add: at most D per listed byte, found from the
// list alone): every suffix ends up in exactly one shard, no communication.  That holds for a rank that takes the retry, too:
// it builds the whole text with the general table and hands out the ranks whose true first D bytes lie in its range
// (Pipeline::retry_whole_text) -- a range chosen again on the general table's digits would not fit between its neighbours'.

namespace sufr {

static constexpr uint32_t EXC_BLK = 1024;            // ranks per workgroup of the mark / merge kernels (256 lanes x 4)
static constexpr uint32_t EXC_LDS_LIST = 8192;       // listed positions / insertion points kept in LDS

// affected ranks: one bit per rank (bit i of word w <-> rank 64 w + i), their number per block of EXC_BLK ranks, and the suffixes
// themselves appended to `list` (any order: they are sorted next; *nlist counts all of them, list holds the first list_cap).
// exc: the listed positions, ascending.  Up to EXC_LDS_LIST of them are searched in LDS; a longer list through every
// `stride`-th entry in LDS and the rest in memory.  coarse: one bit per 2^cshift text positions, set where a listed position
// lies -- almost every suffix starts and ends its comparisons inside one block without one: a single LDS read.
static constexpr uint32_t EXC_COARSE_WORDS = 2048;   // 65 536 bits
__global__ void __launch_bounds__(256)
k_exc_mark(const uint32_t* __restrict__ sa, const uint32_t* __restrict__ lcp, uint32_t s, const uint32_t* __restrict__ exc, uint32_t E,
           int cshift, uint32_t min_reach /* shards: D - 1, else 0 */, uint32_t cap /* capped builds: symbols compared, else 0 */,
           unsigned long long* __restrict__ affbits, uint32_t* __restrict__ blkcnt, uint32_t nblk,
           uint32_t* __restrict__ list, uint32_t list_cap, unsigned int* __restrict__ nlist)
{
    extern __shared__ __align__(16) uint32_t s_dyn[];
    uint32_t* s_coarse = s_dyn;                          // EXC_COARSE_WORDS
    uint32_t* s_exc = s_dyn + EXC_COARSE_WORDS;          // the list, or every stride-th entry of it
    __shared__ uint32_t s_cnt[4];
    const uint32_t stride = (E + EXC_LDS_LIST - 1) / EXC_LDS_LIST;          // 1: the whole list
    const uint32_t ns = (E + stride - 1) / stride;
    for (uint32_t i = threadIdx.x; i < EXC_COARSE_WORDS; i += 256) s_coarse[i] = 0;
    for (uint32_t i = threadIdx.x; i < ns; i += 256) s_exc[i] = exc[i * stride];
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < E; i += 256) { const uint32_t q = exc[i] >> cshift; atomicOr(&s_coarse[q >> 5], 1u << (q & 31u)); }
    __syncthreads();
    for (uint32_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const uint32_t r0 = blk * EXC_BLK;
        uint32_t c = 0;
        uint32_t pv[4], av[4], bv[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t r = r0 + (uint32_t)k * 256 + threadIdx.x;
            pv[k] = r < s ? sa[r] : 0u;
            av[k] = r < s ? lcp[r] : 0u;
            bv[k] = r + 1 < s ? lcp[r + 1] : 0u;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t r = r0 + (uint32_t)k * 256 + threadIdx.x;
            bool aff = false;
            if (r < s) {
                const uint32_t p = pv[k];
                uint32_t reach = av[k] > bv[k] ? av[k] : bv[k];
                reach = reach > min_reach ? reach : min_reach;
                const uint64_t last = (uint64_t)p + reach;                              // the farthest position a comparison of p read
                const uint32_t q0 = p >> cshift, q1 = (uint32_t)(last >> cshift);
                bool maybe = q1 != q0 || ((s_coarse[q0 >> 5] >> (q0 & 31u)) & 1u) != 0u;
                if (maybe) {
                    // the first listed position >= p
                    uint32_t lo = 0, hi = ns;
                    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (s_exc[mid] < p) lo = mid + 1; else hi = mid; }
                    if (stride == 1) aff = lo < ns && (uint64_t)s_exc[lo] <= last && (cap == 0u || s_exc[lo] - p < cap);
                    else {
                        // entries (lo - 1) stride + 1 .. lo stride of the list lie in (sample lo - 1, sample lo]
                        uint32_t a = lo ? (lo - 1) * stride + 1 : 0u, b = lo < ns ? lo * stride + 1 : E;
                        if (b > E) b = E;
                        while (a < b) { const uint32_t mid = (a + b) >> 1; if (exc[mid] < p) a = mid + 1; else b = mid; }
                        aff = a < E && (uint64_t)exc[a] <= last && (cap == 0u || exc[a] - p < cap);
                    }
                }
                if (aff) { const unsigned int at = atomicAdd(nlist, 1u); if (at < list_cap) list[at] = p; }
            }
            const unsigned long long bal = __ballot(aff);
            if ((threadIdx.x & 63u) == 0u && r0 + (uint32_t)k * 256 + (threadIdx.x & ~63u) < s)
                affbits[(size_t)(r0 >> 6) + (uint32_t)k * 4 + (threadIdx.x >> 6)] = bal;
            c += (uint32_t)__popcll(bal);
        }
        if ((threadIdx.x & 63u) == 0u) s_cnt[threadIdx.x >> 6] = c;        // (c is wave-uniform)
        __syncthreads();
        if (threadIdx.x == 0) blkcnt[blk] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        __syncthreads();
    }
}

// affected ranks before rank r (blkoff: exclusive scan of the block counts)
__device__ __forceinline__ uint32_t exc_aff_before(const unsigned long long* __restrict__ affbits, const uint32_t* __restrict__ blkoff, uint32_t r)
{
    uint32_t c = blkoff[r / EXC_BLK];
    const uint32_t w0 = (r / EXC_BLK) * (EXC_BLK / 64), w1 = r >> 6;
    for (uint32_t w = w0; w < w1; w++) c += (uint32_t)__popcll(affbits[w]);
    if (r & 63u) c += (uint32_t)__popcll(affbits[w1] & ((1ull << (r & 63u)) - 1ull));
    return c;
}

// first unaffected rank >= r below `lim` (lim if none); last unaffected rank < r (0xffffffff if none)
__device__ __forceinline__ uint32_t exc_next_kept(const unsigned long long* __restrict__ affbits, uint32_t r, uint32_t lim)
{
    while (r < lim) {
        const unsigned long long free = ~affbits[r >> 6] & (~0ull << (r & 63u));
        if (free) { const uint32_t q = (r & ~63u) + (uint32_t)__builtin_ctzll(free); return q < lim ? q : lim; }
        r = (r & ~63u) + 64u;
    }
    return lim;
}
__device__ __forceinline__ uint32_t exc_prev_kept(const unsigned long long* __restrict__ affbits, uint32_t r)
{
    while (r > 0) {
        const uint32_t q = r - 1;                                          // candidates: ranks <= q
        const unsigned long long free = ~affbits[q >> 6] & ((q & 63u) == 63u ? ~0ull : ((2ull << (q & 63u)) - 1ull));
        if (free) return (q & ~63u) + 63u - (uint32_t)__builtin_clzll(free);
        r = q & ~63u;
    }
    return 0xffffffffu;
}

// x against y on the whole text T from `l` matched symbols on: returns x < y ? -1 : +1 and the common prefix in l (x != y).
// wide_compare_plain (sufr_wide.inc) with one addition: a run of equal bytes is crossed in one step.  The affected suffixes of a
// genome are the ones in front of an 'N' run that holds a listed byte (a '#' between two sequences sits between the telomere
// runs of both): every comparison among them walks 10^4 .. 10^7 'N' otherwise.  The run-end table is that of the BUILD's text
// (listed bytes as 'N'), so a step also stops at the next listed position of either suffix.
// cap (capped builds, --max-query-len L built directly): only the first `cap` symbols count; suffixes that agree on them come in
// descending position (sufr_builder.rs:668-712) -- the rule of a suffix that runs out of text, so one return serves both.
struct ExcText { const uint8_t* t; uint64_t n; RunTable rt; const uint32_t* exc; uint32_t E; uint32_t cap; };
__device__ __forceinline__ int exc_compare(const ExcText& X, uint64_t x, uint64_t y, uint64_t& l)
{
    const uint8_t* __restrict__ t = X.t;
    uint64_t room = X.n - (x > y ? x : y);               // symbols of the suffix that starts later
    if (X.cap && (uint64_t)X.cap < room) room = X.cap;   // ... or the cap
    uint64_t k = l < room ? l : room;
    for (;;) {
        bool diff = false;
        uint32_t steps = 0;
        while (k + 8 <= room && steps < 8u) {
            uint64_t a, b;
            __builtin_memcpy(&a, t + x + k, 8);
            __builtin_memcpy(&b, t + y + k, 8);
            if (a != b) { k += (uint64_t)(__builtin_ctzll(a ^ b) >> 3); diff = true; break; }
            k += 8; steps++;
        }
        if (diff) break;
        if (k + 8 > room) { while (k < room && t[x + k] == t[y + k]) k++; break; }
        // 64 symbols matched: inside a run?  (the last two symbols of x's side are equal; y's are the same symbols)
        if (k >= 2 && t[x + k - 1] == t[x + k - 2] && t[x + k] == t[x + k - 1] && t[y + k] == t[x + k]) {
            auto clipped_run = [&](uint64_t q) -> uint64_t {
                uint64_t r = run_len_exact(q, X.rt);                               // symbols equal to T'[q] from q on
                uint32_t lo = 0, hi = X.E;                                         // the first listed position >= q
                while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((uint64_t)X.exc[mid] < q) lo = mid + 1; else hi = mid; }
                if (lo < X.E) { const uint64_t d = (uint64_t)X.exc[lo] - q; r = d < r ? d : r; }
                return r;
            };
            const uint64_t rx = clipped_run(x + k), ry = clipped_run(y + k);
            uint64_t skip = rx < ry ? rx : ry;
            if (skip > room - k) skip = room - k;
            if (skip > 1) k += skip - 1;                                           // (the symbol at the end of the step is compared as usual)
        }
    }
    l = k < room ? k : room;
    if (k >= room) return x > y ? -1 : 1;                // the later start ran out of text (or both agree up to the cap): it comes first
    return t[x + k] < t[y + k] ? -1 : 1;
}

static constexpr uint32_t EXC_PAD = 0xFFFFFFFFu;         // padding of the bitonic network: above every suffix

// one compare-exchange stage of a bitonic network over text positions (k_wide_bitonic with the run-aware comparison)
__global__ void __launch_bounds__(256)
k_exc_bitonic(ExcText X, uint32_t* __restrict__ v, uint32_t P, uint32_t k, uint32_t j)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const uint32_t l = i ^ j;
    if (l <= i) return;
    const uint32_t a = v[i], b = v[l];
    auto above = [&](uint32_t p, uint32_t q) -> bool {
        if (p == q || q == EXC_PAD) return false;
        if (p == EXC_PAD) return true;
        uint64_t m = 0;
        return exc_compare(X, (uint64_t)p, (uint64_t)q, m) > 0;
    };
    const bool up = (i & k) == 0;
    if (up ? above(a, b) : above(b, a)) { v[i] = b; v[l] = a; }
}

// LCPs of the sorted list
__global__ void __launch_bounds__(256)
k_exc_list_lcp(ExcText X, const uint32_t* __restrict__ v, uint32_t cnt, uint32_t* __restrict__ lcp)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= cnt) return;
    uint64_t m = 0;
    if (i > 0) (void)exc_compare(X, (uint64_t)v[i - 1], (uint64_t)v[i], m);
    lcp[i] = (uint32_t)m;
}

// ---- the affected ranks from the listed positions alone (single-shard builds) -----------------------------------------
__device__ __forceinline__ bool exc_starts_suffix(uint32_t b, int allow_amb)
{
    return allow_amb || b == 0x24u || b == 0x41u || b == 0x43u || b == 0x47u || b == 0x54u;      // sufr_builder.rs:446-449 (DNA)
}
// rank of suffix p in sa (sorted in the order of the text X.t -- the BUILD's text, listed bytes as 'N'); 0xffffffff if it is not there
__device__ __forceinline__ uint32_t exc_rank_of(const ExcText& X, const uint32_t* __restrict__ sa, uint32_t s, uint64_t p)
{
    uint32_t lo = 0, hi = s;
    uint64_t ll = 0, lr = 0;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        const uint64_t q = sa[mid];
        if (q == p) return mid;
        uint64_t l = ll < lr ? ll : lr;
        if (exc_compare(X, p, q, l) > 0) { lo = mid + 1; ll = l; } else { hi = mid; lr = l; }
    }
    return 0xffffffffu;
}
// first position >= p that starts a suffix (runs of bytes that start none -- 'N', '%' -- are crossed in one run-table lookup)
__device__ __forceinline__ uint64_t exc_next_start(const ExcText& X, uint64_t p, int allow_amb)
{
    while (p < X.n && !exc_starts_suffix(X.t[p], allow_amb)) p += run_len_exact(p, X.rt);
    return p;
}
// does every suffix start in [p, f] reach the listed position f (vacuously true when there is none)?  monotone in p
__device__ __forceinline__ bool exc_reaches(const ExcText& X, const uint32_t* __restrict__ sa, const uint32_t* __restrict__ lcp, uint32_t s,
                                            uint64_t p, uint64_t f, int allow_amb)
{
    const uint64_t e = exc_next_start(X, p, allow_amb);
    if (e > f) return true;
    const uint32_t r = exc_rank_of(X, sa, s, e);
    if (r == 0xffffffffu) return true;                                      // (cannot happen in a single-shard build)
    const uint32_t a = lcp[r], b = r + 1 < s ? lcp[r + 1] : 0u;
    return (uint64_t)(a > b ? a : b) >= f - e && (X.cap == 0u || f - e < (uint64_t)X.cap);     // (a capped comparison reads cap symbols at most)
}
// pmin[e]: the smallest position p > the listed position before exc[e] such that every suffix start in [p, exc[e]] is affected
// (exc[e] + 1: none).  One WAVE per listed position: a probe is a binary search of a suffix in SA' -- ~31 dependent random reads
// --, so the 64 lanes probe 64 positions at a time: first the 64 positions right below the listed one (where the boundary
// almost always lies: one round), then 64-ary over what is left (a lane per listed position, galloping: 2.45 ms for 50 of them).
__global__ void __launch_bounds__(256)
k_exc_pmin(ExcText X /* the build's text: E = 0 */, const uint32_t* __restrict__ exc, uint32_t E, const uint32_t* __restrict__ sa,
           const uint32_t* __restrict__ lcp, uint32_t s, int allow_amb, uint32_t* __restrict__ pmin)
{
    const uint32_t e = (blockIdx.x * 256 + threadIdx.x) >> 6;
    if (e >= E) return;
    const uint32_t ln = lane_id();
    const uint64_t f = exc[e];
    const uint64_t floor_p = e ? (uint64_t)exc[e - 1] + 1 : 0ull;          // (positions at or below the listed position before have it as theirs)
    // invariant: reaches(good) is true (good = f + 1: vacuously); the answer lies in [lo, good]
    uint64_t lo = floor_p, good = f + 1;
    bool dense = true;
    while (lo < good) {
        const uint64_t span = good - lo;
        uint64_t stride = dense ? 1ull : (span + 63) / 64;
        uint64_t base = dense ? (span > 64 ? good - 64 : lo) : lo;         // dense: the 64 positions right below `good`
        const uint64_t c = base + stride * ln;
        const bool in = c < good;
        const bool r = in ? exc_reaches(X, sa, lcp, s, c, f, allow_amb) : true;
        const unsigned long long T = __ballot(r);
        // monotone: false ... false true ... true over the lanes; k = first lane that reaches
        const int k = T ? __builtin_ctzll(T) : 64;                         // (64: none of the probed positions reaches; `good` still does)
        if (k == 0) {
            if (base == lo) { good = lo; break; }                          // the whole interval reaches
            good = base;                                                   // all 64 reach: go on below them
        } else {
            if (k < 64 && base + stride * (uint64_t)k < good) good = base + stride * (uint64_t)k;
            lo = base + stride * (uint64_t)(k - 1) + 1;
        }
        dense = false;
        if (good - lo <= 64) dense = true;
    }
    if (ln == 0) pmin[e] = (uint32_t)good;
}
// the suffix starts of the ranges [pmin[e], exc[e]] -> their ranks marked (bit per rank, count per block) and listed;
// roff: exclusive prefix sums of the range lengths, total T
__global__ void __launch_bounds__(256)
k_exc_expand(ExcText X, const uint32_t* __restrict__ exc, uint32_t E, const uint32_t* __restrict__ pmin, const unsigned long long* __restrict__ roff,
             unsigned long long T, const uint32_t* __restrict__ sa, uint32_t s, int allow_amb, unsigned long long* __restrict__ affbits,
             uint32_t* __restrict__ blkcnt, uint32_t* __restrict__ list, uint32_t list_cap, unsigned int* __restrict__ nlist)
{
    const unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    uint32_t lo = 0, hi = E;                                               // last e with roff[e] <= t
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (roff[mid] <= t) lo = mid; else hi = mid; }
    const uint64_t p = (uint64_t)pmin[lo] + (t - roff[lo]);
    if (p > (uint64_t)exc[lo] || !exc_starts_suffix(X.t[p], allow_amb)) return;
    const uint32_t r = exc_rank_of(X, sa, s, p);
    if (r == 0xffffffffu) return;
    atomicOr(&affbits[r >> 6], 1ull << (r & 63u));
    atomicAdd(&blkcnt[r / EXC_BLK], 1u);
    const unsigned int at = atomicAdd(nlist, 1u);
    if (at < list_cap) list[at] = (uint32_t)p;
}

// place of every listed suffix among the survivors: ins_rank[j] = the first unaffected rank whose suffix is above list[j] (s if
// none), ins_u[j] = survivors below it.  The list is sorted, so both are non-decreasing in j.
__global__ void __launch_bounds__(256)
k_exc_rank(ExcText X, const uint32_t* __restrict__ sa, uint32_t s,
           const unsigned long long* __restrict__ affbits, const uint32_t* __restrict__ blkoff, const uint32_t* __restrict__ list, uint32_t A,
           uint32_t* __restrict__ ins_rank, uint32_t* __restrict__ ins_u)
{
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= A) return;
    const uint64_t x = list[j];
    uint32_t lo = 0, hi = s;
    uint64_t ll = 0, lr = 0;                                               // symbols matched with the probes below / above x
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        const uint32_t m = exc_next_kept(affbits, mid, hi);
        if (m == hi) { hi = mid; continue; }                               // [mid, hi) holds no survivor
        uint64_t l = ll < lr ? ll : lr;
        if (exc_compare(X, x, (uint64_t)sa[m], l) > 0) { lo = m + 1; ll = l; }
        else { hi = mid; lr = l; }
    }
    const uint32_t at = exc_next_kept(affbits, lo, s);
    ins_rank[j] = at;
    ins_u[j] = at - exc_aff_before(affbits, blkoff, at < s ? at : s);
}
// (at == s: every affected rank counts) -- blkoff has one entry past the last block for that
// the listed suffixes into the output: place = survivors below + listed suffixes below
__global__ void __launch_bounds__(256)
k_exc_place(ExcText X, const uint32_t* __restrict__ sa, const unsigned long long* __restrict__ affbits,
            const uint32_t* __restrict__ list, const uint32_t* __restrict__ list_lcp, uint32_t A, const uint32_t* __restrict__ ins_rank,
            const uint32_t* __restrict__ ins_u, uint32_t* __restrict__ out_sa, uint32_t* __restrict__ out_lcp)
{
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= A) return;
    const uint32_t place = ins_u[j] + j;
    uint32_t l = 0;
    if (j > 0 && ins_u[j - 1] == ins_u[j]) l = list_lcp[j];               // the listed suffix before it sits right before it
    else {
        const uint32_t pr = exc_prev_kept(affbits, ins_rank[j]);
        if (pr != 0xffffffffu) { uint64_t m = 0; (void)exc_compare(X, (uint64_t)list[j], (uint64_t)sa[pr], m); l = (uint32_t)m; }
    }
    out_sa[place] = list[j];
    out_lcp[place] = l;
}

// listed suffixes placed at or before the first rank of every block of EXC_BLK ranks (were it a survivor): cblk[b], b = 0 .. nblk
__global__ void __launch_bounds__(256)
k_exc_block_counts(const uint32_t* __restrict__ blkoff, uint32_t nblk, const uint32_t* __restrict__ ins_u, uint32_t A, uint32_t* __restrict__ cblk)
{
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b > nblk) return;
    if (b == nblk) { cblk[b] = A; return; }
    const uint32_t u0 = b * EXC_BLK - blkoff[b];
    uint32_t lo = 0, hi = A;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (ins_u[mid] <= u0) lo = mid + 1; else hi = mid; }
    cblk[b] = lo;
}

// the survivors into the output, shifted by the affected ranks before them and the insertions at or before them.  A block
// without an affected rank and without an insertion inside it -- all but a few hundred of 1.5 million -- is a shifted copy.
__global__ void __launch_bounds__(256)
k_exc_merge(ExcText X, const uint32_t* __restrict__ sa, const uint32_t* __restrict__ lcp, uint32_t s,
            const unsigned long long* __restrict__ affbits, const uint32_t* __restrict__ blkoff, const uint32_t* __restrict__ cblk,
            const uint32_t* __restrict__ list, const uint32_t* __restrict__ ins_u, uint32_t nblk, uint32_t* __restrict__ out_sa,
            uint32_t* __restrict__ out_lcp)
{
    __shared__ uint32_t s_pre[EXC_BLK / 64];
    for (uint32_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const uint32_t r0 = blk * EXC_BLK;
        const uint32_t off0 = blkoff[blk], naff = blkoff[blk + 1] - off0;
        // listed suffixes at or before a survivor of this block: between the counts of this block's and the next block's first rank
        const uint32_t c_lo = cblk[blk], c_hi = cblk[blk + 1];
        const uint32_t u0 = r0 - off0;                                     // survivor index of the block's first rank (c_lo counts up to it)
        uint32_t sv[4], lv[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t r = r0 + (uint32_t)k * 256 + threadIdx.x;
            sv[k] = r < s ? sa[r] : 0u;
            lv[k] = r < s ? lcp[r] : 0u;
        }
        if (naff == 0 && c_lo == c_hi) {
            // only the block's first rank can follow a listed suffix or an affected rank
            if (threadIdx.x == 0) {
                if (c_lo > 0 && ins_u[c_lo - 1] == u0) {
                    uint64_t m = 0;
                    (void)exc_compare(X, (uint64_t)sv[0], (uint64_t)list[c_lo - 1], m);
                    lv[0] = (uint32_t)m;
                } else if (r0 > 0 && ((affbits[(r0 >> 6) - 1u] >> 63) & 1ull)) {
                    uint32_t l = lv[0], q = r0;
                    bool found = false;
                    while (q > 0) {
                        q--;
                        if (!((affbits[q >> 6] >> (q & 63u)) & 1ull)) { found = true; break; }
                        const uint32_t v = lcp[q];
                        l = v < l ? v : l;
                    }
                    lv[0] = found ? l : 0u;
                }
            }
            const uint32_t shift = c_lo - off0;                            // (mod 2^32: the sum r + shift is what counts)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t r = r0 + (uint32_t)k * 256 + threadIdx.x;
                if (r < s) { out_sa[r + shift] = sv[k]; out_lcp[r + shift] = lv[k]; }
            }
            continue;
        }
        __syncthreads();                                                   // (s_pre of the block before: read by all by now)
        if (threadIdx.x < 64u) {
            // affected ranks before every 64-rank word of the block
            const uint32_t w = threadIdx.x;
            uint32_t c = (w < EXC_BLK / 64 && r0 + w * 64 < s) ? (uint32_t)__popcll(affbits[(r0 >> 6) + w]) : 0u;
            uint32_t incl = c;
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) { const uint32_t v = __shfl_up(incl, o, WAVE); if ((int)w >= o) incl += v; }
            if (w < EXC_BLK / 64) s_pre[w] = off0 + incl - c;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t r = r0 + (uint32_t)k * 256 + threadIdx.x;
            if (r >= s) continue;
            const uint32_t w = (uint32_t)k * 4 + (threadIdx.x >> 6);
            const unsigned long long bits = affbits[(r0 >> 6) + w];
            if ((bits >> (r & 63u)) & 1ull) continue;                      // affected: placed by k_exc_place
            const uint32_t u = r - (s_pre[w] + (uint32_t)__popcll(bits & ((1ull << (r & 63u)) - 1ull)));
            uint32_t c = c_lo;                                             // listed suffixes with ins_u <= u
            if (c_hi != c_lo) {
                uint32_t lo = c_lo, hi = c_hi;
                while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (ins_u[mid] <= u) lo = mid + 1; else hi = mid; }
                c = lo;
            }
            uint32_t l = lv[k];
            const bool after_listed = c > c_lo ? ins_u[c - 1] == u : (c > 0 && u == u0 && ins_u[c - 1] == u);
            const bool prev_out = r > 0 && (r & 63u ? ((bits >> ((r & 63u) - 1u)) & 1ull) != 0ull : ((affbits[(r >> 6) - 1u] >> 63) & 1ull) != 0ull);
            if (after_listed) {                                            // a listed suffix sits right before this one
                uint64_t m = 0;
                (void)exc_compare(X, (uint64_t)sv[k], (uint64_t)list[c - 1], m);
                l = (uint32_t)m;
            } else if (prev_out) {
                // minimum over the ranks taken out since the survivor before
                uint32_t q = r;
                bool found = false;
                while (q > 0) {
                    q--;
                    if (!((affbits[q >> 6] >> (q & 63u)) & 1ull)) { found = true; break; }
                    const uint32_t v = lcp[q];
                    l = v < l ? v : l;
                }
                if (!found) l = 0;                                         // the first survivor of all, nothing listed before it
            }
            out_sa[u + c] = sv[k];
            out_lcp[u + c] = l;
        }
    }
}

// ---- shards ---------------------------------------------------------------------------------------------------------
// (ExcShard: sufr_launch.inc -- first digits of D characters in [raw_lo, raw_hi); raw_hi = 8^D: no upper bound)

// D symbols as one integer in text order: 9 bits each, byte + 1, 0 past the end of the text
__device__ __forceinline__ uint64_t exc_true_prefix(const ExcText& X, uint64_t p, int D)
{
    uint64_t v = 0;
    for (int i = 0; i < D; i++) v = (v << 9) | (p + (uint64_t)i < X.n ? (uint64_t)X.t[p + i] + 1ull : 0ull);
    return v;
}
// the same for a digit of the fixed codes {0 pad, 1 '$', 2 '%', 3 A, 4 C, 5 G, 6 N, 7 T}
__device__ __forceinline__ uint64_t exc_digit_prefix(uint32_t raw, int D)
{
    const uint32_t bytes = 0x544e4743u;                  // codes 4..7: C G N T
    uint64_t v = 0;
    for (int i = D - 1; i >= 0; i--) {
        const uint32_t c = (raw >> (3 * i)) & 7u;
        const uint32_t b = c == 0 ? 0u : (c == 1 ? 0x25u : (c == 2 ? 0x26u : (c == 3 ? 0x42u : ((bytes >> (8 * (c - 4))) & 0xffu) + 1u)));
        v = (v << 9) | b;
    }
    return v;
}
// does the suffix at p belong to the shard by its TRUE first D bytes / by the codes it was built with ('N' for listed bytes)?
__device__ __forceinline__ bool exc_true_in(const ExcText& X, const ExcShard& S, uint64_t p)
{
    const uint64_t v = exc_true_prefix(X, p, S.D);
    if (v < exc_digit_prefix(S.raw_lo, S.D)) return false;
    return (S.raw_hi >> (3 * S.D)) != 0u || v < exc_digit_prefix(S.raw_hi, S.D);
}
__device__ __forceinline__ bool exc_built_in(const ExcText& X, const ExcShard& S, uint64_t p)
{
    uint32_t raw = 0;
    for (int i = 0; i < S.D; i++) {
        const uint64_t q = p + (uint64_t)i;
        uint32_t c = 0;
        if (q < X.n) {
            uint32_t lo = 0, hi = X.E;
            while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((uint64_t)X.exc[mid] < q) lo = mid + 1; else hi = mid; }
            c = (lo < X.E && (uint64_t)X.exc[lo] == q) ? 6u : dna_fixed_code(X.t[q]);
        }
        raw = (raw << 3) | c;
    }
    return raw >= S.raw_lo && raw < S.raw_hi;
}

// of the suffixes taken out of this shard's arrays: the ones that stay in this shard
__global__ void __launch_bounds__(256)
k_exc_shard_filter(ExcText X, ExcShard S, const uint32_t* __restrict__ list, uint32_t A, uint32_t* __restrict__ out, unsigned int* __restrict__ nout)
{
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= A) return;
    const uint32_t p = list[j];
    if (exc_true_in(X, S, p)) out[atomicAdd(nout, 1u)] = p;
}
// the suffixes the other shards were built with that belong here: a listed byte among their first D characters moved them
__global__ void __launch_bounds__(256)
k_exc_shard_add(ExcText X, ExcShard S, uint32_t* __restrict__ out, uint32_t out_cap, unsigned int* __restrict__ nout)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= X.E * (uint32_t)S.D) return;
    const uint32_t e = t / (uint32_t)S.D, d = t % (uint32_t)S.D;
    const uint32_t f = X.exc[e];
    if (f < d) return;
    const uint32_t p = f - d;
    // (once per suffix: from the first listed byte at or after p)
    if (e > 0 && X.exc[e - 1] >= p) return;
    const uint32_t b = X.t[p];
    if (!(S.allow_amb || b == 0x24u || b == 0x41u || b == 0x43u || b == 0x47u || b == 0x54u)) return;     // sufr_builder.rs:446-449
    if (exc_true_in(X, S, p) && !exc_built_in(X, S, p)) { const unsigned int at = atomicAdd(nout, 1u); if (at < out_cap) out[at] = p; }
}

// ---------------------------------------------------------------------------------------------------------------
// host side.  bsa / blcp: the arrays of the build on T' (s ranks), out_sa / out_lcp: the caller's.  Returns
// SUFR_HIP_E_UNSUPPORTED (no error text) when more suffixes are affected than the whole-text sort takes or the context allows
// (pl.exc_max_affected()): the caller builds the text again with the general code table.
// ---------------------------------------------------------------------------------------------------------------
static constexpr uint64_t EXC_MAX_AFFECTED = Pipeline::EXC_MAX_AFFECTED_DEFAULT;     // what the list and the whole-text sort are sized for

int exc_reinsert(Pipeline& pl, uint8_t* d_text, uint64_t n, const uint32_t* bsa, const uint32_t* blcp, uint32_t s,
                 const uint32_t* d_exc, uint32_t E, uint32_t* out_sa, uint32_t* out_lcp, uint64_t out_cap, uint64_t* affected_out,
                 const ExcShard& shard, uint64_t* s_out)
{
    // d_text: still the BUILD's text ('N' for the listed bytes) on entry; the bytes are put back once the affected ranks are known
    *s_out = s;
    hipStream_t st = pl.stream;
    int rc;
    *affected_out = 0;
    // the limit of all three comparisons below (sufr_hip_set_exc_max_affected: EXC_MAX_AFFECTED or less; the buffers keep their sizes);
    // the one that gives up says so in last_exc_retry
    const uint64_t max_affected = pl.exc_max_affected();
    auto give_up = [&pl](uint32_t way) { if (way > pl.last_exc_retry) pl.last_exc_retry = way; return SUFR_HIP_E_UNSUPPORTED; };
    const uint32_t nblk = (s + EXC_BLK - 1) / EXC_BLK;
    const size_t nwords = (size_t)nblk * (EXC_BLK / 64);
    if ((rc = pl.ensure(pl.exc_bits, nwords * 8 + 64)) || (rc = pl.ensure(pl.exc_blk, ((size_t)nblk + 4) * 4)) ||
        (rc = pl.ensure(pl.exc_off, ((size_t)nblk + 4) * 4))) return rc;
    unsigned long long* bits = (unsigned long long*)pl.exc_bits.p;
    uint32_t* blkcnt = (uint32_t*)pl.exc_blk.p;
    uint32_t* blkoff = (uint32_t*)pl.exc_off.p;
    // the affected suffixes are appended to the list as they are found: room for the most the whole-text sort takes
    const uint32_t list_cap = (uint32_t)EXC_MAX_AFFECTED;
    if ((rc = pl.ensure(pl.exc_list, ((size_t)list_cap * 4 + (size_t)nblk + 64) * 4))) return rc;
    uint32_t* list = (uint32_t*)pl.exc_list.p;                             // P entries, then: LCPs (P), ranks (A), survivor counts (A), block counts
    if (hipMemsetAsync(blkcnt + nblk, 0, 16, st) != hipSuccess || hipMemsetAsync(pl.sc(Pipeline::SC_TMP0), 0, 8, st) != hipSuccess) { pl.set_error("memset failed"); return SUFR_HIP_E_HIP; }
    if (!shard.sharded) {
        // from the listed positions alone (header comment): no pass over the arrays
        ExcText XB;
        XB.t = d_text; XB.n = n; XB.rt = pl.rtab; XB.exc = d_exc; XB.E = 0; XB.cap = shard.cap;          // the build's text: nothing to clip at
        if ((rc = pl.ensure(pl.exc_pmin, (size_t)E * 4 + 64)) || (rc = pl.ensure(pl.exc_roff, ((size_t)E + 1) * 8 + 64))) return rc;
        if (hipMemsetAsync(bits, 0, nwords * 8, st) != hipSuccess || hipMemsetAsync(blkcnt, 0, (size_t)nblk * 4, st) != hipSuccess) { pl.set_error("memset failed"); return SUFR_HIP_E_HIP; }
        hipLaunchKernelGGL(k_exc_pmin, dim3((E + 3) / 4), dim3(256), 0, st, XB, d_exc, E, bsa, blcp, s, shard.allow_amb, (uint32_t*)pl.exc_pmin.p);
        std::vector<uint32_t> hp(E), he(E);
        if (hipMemcpyAsync(hp.data(), pl.exc_pmin.p, (size_t)E * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(he.data(), d_exc, (size_t)E * 4, hipMemcpyDeviceToHost, st) != hipSuccess || pl.sync_reads() != hipSuccess) { pl.set_error("finding the affected suffixes failed"); return SUFR_HIP_E_HIP; }
        std::vector<unsigned long long> ro((size_t)E + 1, 0ull);
        for (uint32_t e = 0; e < E; e++) ro[e + 1] = ro[e] + (hp[e] <= he[e] ? (unsigned long long)he[e] - hp[e] + 1ull : 0ull);
        const unsigned long long T = ro[E];
        if (T > ((unsigned long long)max_affected << 4)) return give_up(1);       // (ranges of positions: most start a suffix; the text still holds 'N')
        if (T) {
            if (hipMemcpyAsync(pl.exc_roff.p, ro.data(), ((size_t)E + 1) * 8, hipMemcpyHostToDevice, st) != hipSuccess) { pl.set_error("copy failed"); return SUFR_HIP_E_HIP; }
            hipLaunchKernelGGL(k_exc_expand, dim3((uint32_t)((T + 255) / 256)), dim3(256), 0, st, XB, d_exc, E, (const uint32_t*)pl.exc_pmin.p,
                               (const unsigned long long*)pl.exc_roff.p, T, bsa, s, shard.allow_amb, bits, blkcnt, list, list_cap,
                               (unsigned int*)pl.sc(Pipeline::SC_TMP0));
            if (pl.sync_reads() != hipSuccess) { pl.set_error("marking the affected suffixes failed"); return SUFR_HIP_E_HIP; }     // (ro: a host vector)
        }
    } else {
    int cshift = 0;
    while (((n - 1) >> cshift) >= (uint64_t)EXC_COARSE_WORDS * 32) cshift++;
    {
        const uint32_t stride = (E + EXC_LDS_LIST - 1) / EXC_LDS_LIST, ns = (E + stride - 1) / stride;
        const size_t lds = ((size_t)EXC_COARSE_WORDS + ns) * 4;
        const uint32_t grid = nblk < 8192u ? nblk : 8192u;
        if (nblk)                                                          // (an empty shard: nothing to mark, the suffixes of its range are added below)
        hipLaunchKernelGGL(k_exc_mark, dim3(grid), dim3(256), lds, st, bsa, blcp, s, d_exc, E, cshift,
                           shard.sharded ? (uint32_t)(shard.D - 1) : 0u, shard.cap, bits, blkcnt, nblk, list, list_cap,
                           (unsigned int*)pl.sc(Pipeline::SC_TMP0));
    }
    }
    // the listed bytes back into the text: every comparison from here on is on the caller's text
    hipLaunchKernelGGL(k_exc_restore, dim3((E + 255) / 256), dim3(256), 0, st, d_text, (const uint32_t*)pl.exc_pos.p, (const uint8_t*)pl.exc_byte.p, E);
    pl.exc_pending = 0;
    if ((rc = pl.scan_u32(blkcnt, nblk + 1, blkoff))) return rc;          // (one entry past the last block: the total)
    unsigned long long tot = 0;
    if (pl.read_at_sync(&tot, pl.sc(Pipeline::SC_SCANTOTAL), 8) != hipSuccess || pl.sync_reads() != hipSuccess) { pl.set_error("marking the affected suffixes failed"); return SUFR_HIP_E_HIP; }
    const uint64_t A_out = tot;                                            // ranks taken out of the arrays
    pl.last_exc_taken = A_out;
    if (A_out > max_affected) return give_up(2);
    ExcText X;
    X.t = d_text; X.n = n; X.rt = pl.rtab; X.exc = d_exc; X.E = E; X.cap = shard.cap;
    uint64_t A = A_out;                                                    // suffixes placed by whole-text comparison
    if (shard.sharded) {
        // the taken suffixes that stay + the other shards' suffixes that belong here -> a list of their own
        if ((rc = pl.ensure(pl.exc_list2, ((size_t)list_cap * 4 + (size_t)nblk + 64) * 4))) return rc;
        uint32_t* list2 = (uint32_t*)pl.exc_list2.p;
        if (hipMemsetAsync(pl.sc(Pipeline::SC_TMP1), 0, 8, st) != hipSuccess) { pl.set_error("memset failed"); return SUFR_HIP_E_HIP; }
        if (A_out) hipLaunchKernelGGL(k_exc_shard_filter, dim3((uint32_t)((A_out + 255) / 256)), dim3(256), 0, st, X, shard, (const uint32_t*)list,
                                      (uint32_t)A_out, list2, (unsigned int*)pl.sc(Pipeline::SC_TMP1));
        hipLaunchKernelGGL(k_exc_shard_add, dim3((E * (uint32_t)shard.D + 255) / 256), dim3(256), 0, st, X, shard, list2, list_cap,
                           (unsigned int*)pl.sc(Pipeline::SC_TMP1));
        unsigned long long cnt = 0;
        if (pl.read_at_sync(&cnt, pl.sc(Pipeline::SC_TMP1), 8) != hipSuccess || pl.sync_reads() != hipSuccess) { pl.set_error("re-sharding the affected suffixes failed"); return SUFR_HIP_E_HIP; }
        A = (uint32_t)cnt;
        if (A > max_affected) return give_up(3);
        list = list2;
    }
    *affected_out = A;
    *s_out = (uint64_t)s - A_out + A;
    if (pl.debug) fprintf(stderr, "[sufr_hip debug] %u bytes outside the DNA table: %llu of %u suffixes taken out, %llu re-placed\n", E,
                          (unsigned long long)A_out, s, (unsigned long long)A);
    if (*s_out > out_cap) { pl.set_error("output capacity " + std::to_string(out_cap) + " < num_suffixes " + std::to_string(*s_out)); return SUFR_HIP_E_CAPACITY; }
    if (A == 0 && A_out == 0) {
        if (s == 0) return 0;
        if (hipMemcpyAsync(out_sa, bsa, (size_t)s * 4, hipMemcpyDeviceToDevice, st) != hipSuccess ||
            hipMemcpyAsync(out_lcp, blcp, (size_t)s * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) { pl.set_error("copy failed"); return SUFR_HIP_E_HIP; }
        return 0;
    }
    uint32_t P = 1;
    while (P < A) P <<= 1;
    if (P < 2) P = 2;
    uint32_t* list_lcp = list + P;
    uint32_t* ins_rank = list_lcp + P;
    uint32_t* ins_u = ins_rank + A;
    uint32_t* cblk = ins_u + A;                                            // nblk + 1
    if (P > A && hipMemsetAsync(list + A, 0xFF, (size_t)(P - A) * 4, st) != hipSuccess) { pl.set_error("memset failed"); return SUFR_HIP_E_HIP; }
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1)
            hipLaunchKernelGGL(k_exc_bitonic, dim3((P + 255) / 256), dim3(256), 0, st, X, list, P, k, j);
    if (A) {
    hipLaunchKernelGGL(k_exc_list_lcp, dim3((uint32_t)((A + 255) / 256)), dim3(256), 0, st, X, (const uint32_t*)list, (uint32_t)A, list_lcp);
    hipLaunchKernelGGL(k_exc_rank, dim3((uint32_t)((A + 255) / 256)), dim3(256), 0, st, X, bsa, s, (const unsigned long long*)bits,
                       (const uint32_t*)blkoff, (const uint32_t*)list, (uint32_t)A, ins_rank, ins_u);
    }
    hipLaunchKernelGGL(k_exc_block_counts, dim3((nblk + 1 + 255) / 256), dim3(256), 0, st, (const uint32_t*)blkoff, nblk, (const uint32_t*)ins_u, (uint32_t)A, cblk);
    if (nblk)
    hipLaunchKernelGGL(k_exc_merge, dim3(nblk < 8192u ? nblk : 8192u), dim3(256), 0, st, X, bsa, blcp, s, (const unsigned long long*)bits,
                       (const uint32_t*)blkoff, (const uint32_t*)cblk, (const uint32_t*)list, (const uint32_t*)ins_u, nblk, out_sa, out_lcp);
    if (A)
    hipLaunchKernelGGL(k_exc_place, dim3((uint32_t)((A + 255) / 256)), dim3(256), 0, st, X, bsa, (const unsigned long long*)bits,
                       (const uint32_t*)list, (const uint32_t*)list_lcp, (uint32_t)A, (const uint32_t*)ins_rank, (const uint32_t*)ins_u, out_sa, out_lcp);
    if (hipGetLastError() != hipSuccess) { pl.set_error("re-placing the affected suffixes failed"); return SUFR_HIP_E_HIP; }
    return 0;
}

}  // namespace sufr
