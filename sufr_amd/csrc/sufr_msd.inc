// sufr_msd.inc -- MSD radix partition of the suffixes on k-character prefixes, then an in-LDS sort of
// every leaf bucket (included by sufr_kernels.hip).
//
// Replaces phase 1 of the reference builder -- partition(): every suffix is binary-searched among sampled
// pivots with cold find_lcp calls and appended to its bucket under a mutex (sufr_builder.rs:404-487,
// upper_bound/is_less 346-394) -- and the top of phase 2 (merge_sort 601-631 inside a bucket):
//
//   level 1   k_msd_hist_text + k_msd_part_text      stream the bit-packed text once; (key, index) records
//                                                    land in the bucket of their first D characters
//   level l   k_msd_hist + k_msd_scatter             buckets too large for the LDS are partitioned again on
//                                                    their next D characters (segment by segment)
//   leaves    k_leaf_sort                            a workgroup takes consecutive small buckets (<= CAP
//                                                    records in all), sorts them in LDS on the remaining
//                                                    key bits (stable LSD passes, wave-level ballot ranking)
//                                                    and writes them to their final place
//
// MSD partitioning needs no stable order (the next level / the leaf sort orders a bucket completely), so a
// workgroup claims the output slots of a tile with one atomicAdd per digit on a cursor shared by all the
// workgroups of its group (group = blockIdx % G, i.e. one XCD under round-robin dispatch -- a placement
// that only matters for speed).  Consecutive claims on a digit are adjacent in memory, so the partly
// filled 128-byte line at the end of one workgroup's run is completed by the next claimer while it is
// still in that XCD's L2: HBM sees whole lines however short the per-tile runs are.
//
// Dense digits: of the 2^dbits nominal values of a D-character digit only those that occur in the text are
// numbered (monotone), see DigitMap.

namespace sufr {

static constexpr uint32_t MSD_MAX_BINS = 4096;    // dense digit values per level (LDS counters of the kernels)

// rank of a raw digit value among the raw values that occur in the text (absent values take the rank of the
// next present one): rowbase[raw / 64] + popcount(pres[raw / 64] below bit raw % 64)
struct DigitMap {
    const uint64_t* pres;       // [rows]  bit i of pres[r] set: raw value 64 r + i occurs
    const uint16_t* rowbase;    // [rows]  number of occurring raw values below 64 r
    uint32_t rows;              // raw_bins / 64
    uint32_t raw_mask;          // raw_bins - 1
    uint32_t nbins;             // occurring values (dense range)
    int dbits;                  // bits per digit = b * D
};

struct LdsMap {
    const uint64_t* pres;
    const uint16_t* rowbase;
};

__device__ __forceinline__ size_t msd_map_bytes(uint32_t rows) { return (size_t)rows * 8 + (((size_t)rows * 2 + 15) & ~(size_t)15); }

// area: 8-byte aligned LDS of msd_map_bytes(rows); callers synchronise before the first lookup
template <int NT>
__device__ __forceinline__ LdsMap msd_load_map(const DigitMap& dm, uint8_t* area)
{
    uint64_t* sp = reinterpret_cast<uint64_t*>(area);
    uint16_t* sr = reinterpret_cast<uint16_t*>(area + (size_t)dm.rows * 8);
    for (uint32_t i = threadIdx.x; i < dm.rows; i += NT) { sp[i] = dm.pres[i]; sr[i] = dm.rowbase[i]; }
    LdsMap m; m.pres = sp; m.rowbase = sr;
    return m;
}

__device__ __forceinline__ uint32_t dense_digit(uint32_t raw, const LdsMap& m)
{
    const uint32_t hi = raw >> 6, lo = raw & 63u;
    const uint64_t below = m.pres[hi] & ((1ull << lo) - 1ull);
    return (uint32_t)m.rowbase[hi] + (uint32_t)__popcll(below);
}

// The key of a record read with the non-temporal hint (k_msd_hist streams its input once; measured on the 3.1 Gb stand-in:
// 3.51 -> 3.34 ms.  The same hint on the record loads of k_msd_scatter and k_leaf_sort, whose stores depend on those
// loads in order, cost 12.4 -> 13.8 ms and 14.2 -> 22.6 ms: profiles/r04_nt_loads.txt).
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint2 load_key_nt(const Rec* p)
{
    const u32x2_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(p));
    return make_uint2(v.x, v.y);
}

// ---------------------------------------------------------------------------------------------
// Level 1 histogram over the bit-packed text: dense first digit of every suffix start whose raw first digit
// lies in [raw_lo, raw_hi) (the shard filter of a multi-GPU build).  One row of counters per group.
// ---------------------------------------------------------------------------------------------
template <int B>
__global__ void __launch_bounds__(THREADS)
k_msd_hist_text(uint64_t n, KeyParams kp, DigitMap dm, uint64_t chunk, uint32_t raw_lo, uint32_t raw_hi,
                uint32_t ngroups, uint32_t* __restrict__ grouptab)
{
    extern __shared__ __align__(16) uint8_t smem[];
    const LdsMap map = msd_load_map<THREADS>(dm, smem);
    uint32_t* s_cnt = reinterpret_cast<uint32_t*>(smem + msd_map_bytes(dm.rows));     // nbins
    for (uint32_t i = threadIdx.x; i < dm.nbins; i += THREADS) s_cnt[i] = 0;
    __syncthreads();
    const int shift = 64 - dm.dbits;
    const uint64_t c0 = (uint64_t)blockIdx.x * chunk;
    const uint64_t c1 = min(c0 + chunk, n);
    for (uint64_t tile0 = c0; tile0 < c1; tile0 += TILE) {
        uint64_t key[EPT];
        uint32_t elig;
        build_keys_packed_t<B, EPT>(kp.packed, tile0 + (uint64_t)threadIdx.x * EPT, kp.elig_codes, key, elig);
#pragma unroll
        for (int e = 0; e < EPT; e++) {
            const uint32_t raw = (uint32_t)(key[e] >> shift);
            if ((elig & (1u << e)) && raw >= raw_lo && raw < raw_hi) atomicAdd(&s_cnt[dense_digit(raw, map)], 1u);
        }
    }
    __syncthreads();
    uint32_t* row = grouptab + (size_t)(blockIdx.x % ngroups) * dm.nbins;
    for (uint32_t i = threadIdx.x; i < dm.nbins; i += THREADS) {
        const uint32_t c = s_cnt[i];
        if (c) atomicAdd(&row[i], c);
    }
}

// leafbase[d] = first slot of bucket d (bins outside [bin_lo, bin_hi) count as empty), leafbase[NB] = total;
// cursor of group g on bucket d = leafbase[d] + records of the groups before g.
// (1 024 threads, the groups' counts of a bin read once, side by side: 17 -> ~6 us -- the kernel sits on the critical path of every
// build, and of a 4.6 Mb one it was 2.5 %)
static constexpr int CUR0_NT = 1024;
__global__ void __launch_bounds__(CUR0_NT)
k_msd_cursors0(const uint32_t* __restrict__ grouptab, uint32_t G, uint32_t NB, uint32_t bin_lo, uint32_t bin_hi,
               uint32_t* __restrict__ leafbase, uint32_t* __restrict__ gcur, unsigned long long* __restrict__ total)
{
    constexpr int NW = CUR0_NT / WAVE;
    __shared__ uint32_t s_w[NW];
    __shared__ uint32_t s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < NB; b0 += CUR0_NT) {
        const uint32_t d = b0 + threadIdx.x;
        const bool live = d < NB && d >= bin_lo && d < bin_hi;
        uint32_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0};        // the first eight groups' counts (msd_groups = 8: all of them)
        uint32_t v = 0;
        if (live) {
#pragma unroll
            for (int g = 0; g < 8; g++) if ((uint32_t)g < G) c[g] = grouptab[(size_t)g * NB + d];
#pragma unroll
            for (int g = 0; g < 8; g++) v += c[g];
            for (uint32_t g = 8; g < G; g++) v += grouptab[(size_t)g * NB + d];
        }
        uint32_t incl = v;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const uint32_t t = __shfl_up(incl, o, WAVE);
            if ((int)lane_id() >= o) incl += t;
        }
        if (lane_id() == 63) s_w[threadIdx.x >> 6] = incl;
        __syncthreads();
        uint32_t wbase = 0, all = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) { const uint32_t x = s_w[w]; if ((uint32_t)w < (threadIdx.x >> 6)) wbase += x; all += x; }
        const uint32_t carry = s_carry;
        if (d < NB) {
            uint32_t run = carry + wbase + incl - v;
            leafbase[d] = run;
#pragma unroll
            for (int g = 0; g < 8; g++) if ((uint32_t)g < G) { gcur[(size_t)g * NB + d] = run; run += c[g]; }
            for (uint32_t g = 8; g < G; g++) {
                gcur[(size_t)g * NB + d] = run;
                if (live) run += grouptab[(size_t)g * NB + d];
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) s_carry = carry + all;
        __syncthreads();
    }
    if (threadIdx.x == 0) { leafbase[NB] = s_carry; *total = (unsigned long long)s_carry; }
}

// ---------------------------------------------------------------------------------------------
// Bin scan of one tile + claim of its output slots.  On entry s_cnt[d] = records of the tile with digit d.
// msd_claim_begin leaves the exclusive prefix in s_cnt (visible after its barrier) and issues one returning
// atomicAdd per non-empty digit on the shared cursors; the caller places its records in LDS meanwhile and
// then calls msd_claim_end, which replaces the prefix by  gdelta[d] = claimed base - prefix  (a record staged
// at slot j with digit d goes to global slot j + gdelta[d]) between two barriers.
// Bins per thread: PB = MSD_MAX_BINS / NT consecutive ones.
// ---------------------------------------------------------------------------------------------
template <int NT>
struct MsdClaim {
    static constexpr int PB = (int)MSD_MAX_BINS / NT;
    uint32_t base[PB];
};

// The scan gives every thread PB consecutive bins; the claims are issued the other way round -- bin
// k * NT + thread, so that one wave instruction touches 64 consecutive cursors (scattered single-dword atomics
// run ~17x slower at the memory side than contiguous ones) -- with the count of a bin taken as the difference
// of neighbouring prefixes.
template <int NT>
__device__ __forceinline__ void msd_claim_begin(uint32_t* s_cnt, uint32_t NB, uint32_t* __restrict__ cur,
                                                uint32_t* s_wsum, uint32_t* s_total, MsdClaim<NT>& cl)
{
    constexpr int PB = MsdClaim<NT>::PB;
    const uint32_t d0 = threadIdx.x * PB;
    uint32_t c[PB];
    uint32_t local = 0;
#pragma unroll
    for (int k = 0; k < PB; k++) { c[k] = (d0 + k < NB) ? s_cnt[d0 + k] : 0u; local += c[k]; }
    uint32_t incl = local;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const uint32_t t = __shfl_up(incl, o, WAVE);
        if ((int)lane_id() >= o) incl += t;
    }
    const int wv = threadIdx.x >> 6;
    if (lane_id() == 63) s_wsum[wv] = incl;
    __syncthreads();
    uint32_t wbase = 0;
    for (int w = 0; w < wv; w++) wbase += s_wsum[w];
    if (threadIdx.x == NT - 1) *s_total = wbase + incl;
    uint32_t run = wbase + incl - local;
#pragma unroll
    for (int k = 0; k < PB; k++) {
        if (d0 + k < NB) s_cnt[d0 + k] = run;
        run += c[k];
    }
    __syncthreads();
    const uint32_t total = *s_total;
#pragma unroll
    for (int k = 0; k < PB; k++) {
        const uint32_t d = (uint32_t)k * NT + threadIdx.x;
        cl.base[k] = 0;
        if (d < NB) {
            const uint32_t cnt = (d + 1 < NB ? s_cnt[d + 1] : total) - s_cnt[d];
            if (cnt) cl.base[k] = atomicAdd(&cur[d], cnt);
        }
    }
}

template <int NT>
__device__ __forceinline__ void msd_claim_end(uint32_t* s_cnt, uint32_t NB, const MsdClaim<NT>& cl)
{
    constexpr int PB = MsdClaim<NT>::PB;
    __syncthreads();                                       // every record has read its prefix, every bin its count
#pragma unroll
    for (int k = 0; k < PB; k++) {
        const uint32_t d = (uint32_t)k * NT + threadIdx.x;
        if (d < NB) s_cnt[d] = cl.base[k] - s_cnt[d];
    }
    __syncthreads();
}

__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, uint32_t lane)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)lane);
    return ((uint64_t)hi << 32) | lo;
}

#ifdef SUFR_HIP_PROBES
// ---------------------------------------------------------------------------------------------
// k_msd_part_text_r3: the radix-partition kernel as round 3 shipped it (probes build only: the A/B partner of the
// k_msd_part_text of sufr_part.inc, SUFR_PROBE_PART_R3=1).  Streams the bit-packed text once (3/8 byte per base for DNA) and
// writes the (key, index) record of every suffix start to the bucket of its first D characters.
// Algorithmic bytes (SURVEY 8d, first partition pass): n (text) + 4 s (indices); the 8-byte key travels with the
// index so that no later pass gathers from the text.
//
// Big tiles with two bytes of staging per record.  A tile is NT * ITER positions (65536 for DNA).  Its packed text
// is copied to LDS as big-endian dwords (24 KB).  Suffix starts come from a bitmap (one bit per position, written
// by the text pass: eligibility 446-449 is a property of the first character).  A wave walks the tile 64 consecutive
// positions at a time (iteration e of wave w: bitmap word e * waves + w, lane l its bit l): the bitmap word of an
// iteration is wave-uniform (one lane holds it, v_readlane hands it round), so stretches that start no suffix --
// masked repeats, N runs: half of a soft-masked genome, in runs of hundreds of bases -- cost a scalar test per 64
// positions instead of 64 predicated lanes' worth of work (round 2 gave a lane 32 consecutive positions: every
// iteration then had some lane with a suffix start, and the kernel paid for all positions of the text).
// A lane cuts the first digit of its position out of the LDS text (two dwords, one funnel shift), looks the dense
// digit up and takes its rank inside the tile from a returning LDS atomic (digit | rank stay in registers).  After
// the bin scan and the claims (one returning atomicAdd per non-empty digit on the shared cursor of its bucket) a
// record's staging slot is start[digit] + rank: the slot takes the record's 16-bit POSITION, nothing else.  The
// copy-out walks the slots in order, cuts every record's K-character key out of the LDS text again and stores
// key + index as one 12-byte record -- consecutive lanes write consecutive records of a digit run.  What that buys
// over staging whole records (12 bytes each, tiles of 8192 positions): eight times the records per digit run and
// claim, an eighth of the per-tile bin work (scan, claims, barriers) per record.
// The text (and bitmap words) of the next tile are fetched into registers before the copy-out and consumed before
// the stores are issued: loads and stores retire in order on this hardware, a load issued behind the stores would
// wait for them.  A tile with more than CAP suffix starts (texts without masked stretches) is flushed as two halves.
// ---------------------------------------------------------------------------------------------
template <int B, int NT, int RNDS>
struct PartGeomR3 {
    static constexpr int PPT = (B == 4) ? 16 : 32;         // (positions per thread and round: a whole number of dwords)
    static constexpr int ITER = PPT * RNDS;                // positions per thread = iterations of a wave over the tile
    static constexpr int P = NT * ITER;                    // positions per tile
    static constexpr int TW = P * B / 32;                  // dwords of packed text per tile
    static constexpr int CAP = P / 16 * 9;                 // records staged per flush (>= P / 2)
    static constexpr size_t lds_bytes(uint32_t map_bytes, uint32_t nbins)
    {
        return (size_t)(TW + 4) * 8 + map_bytes + (size_t)((nbins + 3u) & ~3u) * 8 + 128 + (size_t)CAP * 2;
    }
};

// (SUFR_STAMP*: phase stamps of the probes build, defined in sufr_kernels.hip)

// The kernel is a two-stage software pipeline over "units" (a tile, or half of one that holds more than CAP suffix
// starts):  ranking of unit u  ||  copy-out of unit u - 1.   Stamped per phase (probes build), round 2's version
// spent 54 % of a tile's time computing with an idle store queue and 36 % issuing stores with idle ALUs, one after
// the other: with one workgroup per CU nothing else fills either gap, and smaller tiles for a second workgroup
// shorten the digit runs (measured: 6.9 -> 9.4 ms).  Here the stores of a unit are issued one record per lane
// between the ranking steps of the next unit -- its text stays in the other one of two LDS text buffers, its
// bucket deltas in the array the next unit uses for its bin starts only after the joint loop.
// A returning memory operation queues behind the OLDER stores of its own wave (one in-order vmcnt per wave), so the
// claims -- returning atomics whose results are needed microseconds later -- belong to waves that never store: the
// first quarter of the waves claim and rank, the others rank and copy out.
template <int B, int NT, int RNDS, bool SHARDED>
__global__ void __launch_bounds__(NT)
k_msd_part_text_r3(uint64_t n, KeyParams kp, DigitMap dm, uint64_t chunk, uint32_t raw_lo, uint32_t raw_hi,
                uint32_t ngroups, uint32_t* __restrict__ gcur, Rec* __restrict__ out,
                const uint64_t* __restrict__ startbits, uint32_t keep_lo)
{
    using Geom = PartGeomR3<B, NT, RNDS>;
    constexpr int ITER = Geom::ITER, P = Geom::P, TW = Geom::TW, CAP = Geom::CAP;
    constexpr int PB = (int)MSD_MAX_BINS / NT;             // bins per thread of the scan
    constexpr int K = 64 / B;
    constexpr int NWORDS = P / 64;                         // bitmap words of a tile
    constexpr uint32_t NW = NT / 64;                       // iteration e of wave w covers bitmap word e NW + w of the tile: the
                                                           // waves sample the tile evenly (a wave with a span of its own idles
                                                           // at the barriers whenever its span is a masked stretch)
    constexpr uint32_t NCW = NW >= 4 ? NW / 4 : 1;         // waves that claim (and never store)
    constexpr uint32_t NCT = NCW * 64;                     // their threads
    constexpr uint32_t NC = NT - NCT;                      // threads that copy out
    constexpr int PBC = ((int)MSD_MAX_BINS + (int)NCT - 1) / (int)NCT;     // bins per claiming thread
    // keep_lo: the key's low word keeps the bits of kp.K characters ((uint32_t)(~0ull << (64 - K * B)) for the K = 64 / B a
    // key holds; the probes build can shorten the key)
    static_assert(K * B >= 32, "the key's high word is all characters");
    static_assert(B >= 2 && B <= 4 && P <= 65536 && CAP >= P / 2 && CAP <= 65536 && ITER % 2 == 0 && ITER <= 64 && PB >= 1 &&
                  NWORDS <= NT && (uint64_t)ITER * NC >= (uint64_t)CAP, "tile geometry");
    extern __shared__ __align__(16) uint8_t smem[];
    const uint32_t NB = dm.nbins, NBa = (NB + 3u) & ~3u;
    uint32_t* s_textb = reinterpret_cast<uint32_t*>(smem);                                // 2 x (TW + 4)
    const LdsMap map = msd_load_map<NT>(dm, smem + (size_t)(TW + 4) * 8);
    uint32_t* s_arr = reinterpret_cast<uint32_t*>(smem + (size_t)(TW + 4) * 8 + msd_map_bytes(dm.rows));   // 2 x NBa
    uint32_t* s_misc = s_arr + 2 * NBa;                                                   // 32
    uint16_t* s_pos = reinterpret_cast<uint16_t*>(s_misc + 32);                           // CAP
    uint32_t* cur = gcur + (size_t)(blockIdx.x % ngroups) * NB;
    const int dshift = 64 - dm.dbits;
    const uint64_t c0 = (uint64_t)blockIdx.x * chunk, c1 = min(c0 + chunk, n);
    if (c0 >= c1) return;
    const uint32_t wv = threadIdx.x >> 6;
    const uint32_t ln = lane_id();
    const bool claimer = threadIdx.x < NCT;
    constexpr int NV = TW / 4 + 1;                         // 16-byte vectors of a tile's text (+ one of halo)
    constexpr int NPRE = (NV + NT - 1) / NT;
    uint4 nxt[NPRE];
    uint64_t nxtbits = 0;                                  // lane l of wave w: bitmap word l NW + w of the next tile
    const uint64_t nbw = (n + 63) / 64;                    // words of the bitmap
    auto fetch = [&](uint64_t t0) {
        const uint4* src = reinterpret_cast<const uint4*>(kp.packed + ((t0 * B) >> 3));
#pragma unroll
        for (int u = 0; u < NPRE; u++) { const int v = threadIdx.x + u * NT; nxt[u] = v < NV ? src[v] : make_uint4(0, 0, 0, 0); }
        const uint64_t wi = t0 / 64 + (uint64_t)ln * NW + wv;
        nxtbits = (ln < (uint32_t)ITER && wi < nbw) ? startbits[wi] : 0ull;
    };
    // the fetched text as big-endian dwords into text buffer `tb`, the tile's suffix starts counted (s_misc[8 + wave])
    auto land = [&](uint32_t tb) {
        uint4* dst = reinterpret_cast<uint4*>(s_textb + (size_t)tb * (TW + 4));
#pragma unroll
        for (int u = 0; u < NPRE; u++) {
            const int v = threadIdx.x + u * NT;
            uint4 q = nxt[u];
            q.x = __builtin_bswap32(q.x); q.y = __builtin_bswap32(q.y); q.z = __builtin_bswap32(q.z); q.w = __builtin_bswap32(q.w);
            if (v < NV) dst[v] = q;
        }
        uint32_t c = (uint32_t)__popcll(nxtbits);
        uint32_t l2 = ln;                                  // (opaque: the shuffle addresses are formed here, not kept in
        asm volatile("" : "+v"(l2));                       //  registers across the tile loop)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            c += (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((l2 + (uint32_t)o) & 63u) << 2), (int)c);
        if (ln == 0) s_misc[8 + wv] = c;
    };
    // one record of a copy-out: slot j of the unit whose text is in buffer `tb`, whose deltas are in `delta`
    auto copy_one = [&](uint32_t j, const uint32_t* T, const uint32_t* delta, uint64_t t0) {
        const uint32_t pos = s_pos[j];
        const uint32_t i = (pos * B) >> 5, sh = (pos * B) & 31u;
        const uint32_t w0 = T[i], w1 = T[i + 1], w2 = T[i + 2];
        Rec rr;
        rr.khi = (uint32_t)((((uint64_t)w0 << 32) | w1) >> (32u - sh));
        rr.klo = (uint32_t)((((uint64_t)w1 << 32) | w2) >> (32u - sh)) & keep_lo;
        rr.idx = (uint32_t)(t0 + pos);
        out[j + delta[dense_digit(rr.khi >> (dshift - 32), map)]] = rr;
    };
    uint32_t unit = 0;                                     // parity: which array counts, which one takes the bin starts
    uint32_t p_total = 0, p_tb = 0;                        // the unit to copy out: records, text buffer,
    uint64_t p_tile0 = 0;                                  //   first position of its tile
    SUFR_STAMP_DECL(8)
    fetch(c0);
    land(0);
    for (uint32_t i = threadIdx.x; i < NB; i += NT) s_arr[i] = 0;
    uint64_t mybits = nxtbits;                             // suffix starts of iteration l of this wave (lanes < ITER)
    __syncthreads();
    uint32_t tb = 0;
    for (uint64_t tile0 = c0; tile0 < c1; tile0 += P, tb ^= 1u) {
        uint32_t kept = 0;                                 // (a sharded build keeps a part of them: an upper bound is all this decides)
#pragma unroll
        for (uint32_t w = 0; w < NW; w++) kept += s_misc[8 + w];
        const bool more = tile0 + P < c1;
        const uint32_t* T = s_textb + (size_t)tb * (TW + 4);
        // one unit: the suffix starts of iterations [E0, E1) ranked (while the unit before it is copied out), claimed
        // and staged; `last`: the tile's last unit (the next tile's text is fetched under it)
        auto run_unit = [&](auto e0c, auto e1c, const bool last) {
            constexpr int E0 = decltype(e0c)::value, E1 = decltype(e1c)::value;
            constexpr int CS = ITER / (E1 - E0);           // copy-out steps per ranking step
            uint32_t* CNT = s_arr + (size_t)(unit & 1u) * NBa;            // counts, then slot deltas of this unit
            uint32_t* START = s_arr + (size_t)((unit & 1u) ^ 1u) * NBa;   // deltas of the unit before, then this unit's bin starts
            const uint32_t* PT = s_textb + (size_t)p_tb * (TW + 4);
            if (last && more) fetch(tile0 + P);            // (before this unit's stores: loads behind them would wait for them)
            // digit | rank << 12 of the suffix start this lane meets in every iteration (~0: none)
            uint32_t dr[E1 - E0];
            uint32_t q0 = wv * 64u + ln;                   // (opaque: the 64 text offsets of a lane are formed here, per tile,
            asm volatile("" : "+v"(q0));                   //  not hoisted out of the tile loop into 128 live registers)
            uint32_t cj = threadIdx.x - NCT;               // copy-out slot of this thread in the step at hand
            asm volatile("" : "+v"(cj));
#pragma unroll
            for (int e = E0; e < E1; e++) {
                dr[e - E0] = 0xffffffffu;
                const uint64_t wbits = readlane_u64(mybits, (uint32_t)e);
                // (wbits == 0: a wave-uniform skip of 64 positions that start no suffix)
                if (wbits != 0ull && ((wbits >> ln) & 1ull)) {
                    const uint32_t o = (q0 + (uint32_t)e * (64u * NW)) * (uint32_t)B;
                    const uint32_t i = o >> 5, sh = o & 31u;
                    const uint64_t W = ((uint64_t)T[i] << 32) | T[i + 1];
                    const uint32_t raw = (uint32_t)((W << sh) >> dshift);
                    bool ok = true;
                    if constexpr (SHARDED) ok = raw >= raw_lo && raw < raw_hi;
                    if (ok) {
                        const uint32_t d = dense_digit(raw, map);
                        dr[e - E0] = d | (atomicAdd(&CNT[d], 1u) << 12);
                    }
                }
                if (!claimer) {
#pragma unroll
                    for (int c = 0; c < CS; c++) {
                        if (cj < p_total) copy_one(cj, PT, START, p_tile0);
                        cj += NC;
                    }
                }
                if ((e & 1) == 1) __builtin_amdgcn_sched_barrier(0);         // the look-ups of 2 iterations in flight, not of 64
            }
            SUFR_STAMP(ph__, 0)                            // 0: ranking || copy-out (this wave)
            __syncthreads();                               // the counts are complete, the unit before is copied out
            SUFR_STAMP(ph__, 1)                            // 1: ... waiting for the other waves
            // exclusive scan of the counts (PB consecutive bins per thread) -> START
            {
                const uint32_t d0 = threadIdx.x * PB;
                uint32_t c[PB];
                uint32_t local = 0;
#pragma unroll
                for (int k = 0; k < PB; k++) { c[k] = (d0 + k < NB) ? CNT[d0 + k] : 0u; local += c[k]; }
                uint32_t incl = local;
#pragma unroll
                for (int o = 1; o < WAVE; o <<= 1) {
                    const uint32_t t = __shfl_up(incl, o, WAVE);
                    if ((int)ln >= o) incl += t;
                }
                if (ln == 63) s_misc[wv] = incl;
                __syncthreads();
                uint32_t wsum = 0;
                for (uint32_t w = 0; w < wv; w++) wsum += s_misc[w];
                if (threadIdx.x == NT - 1) s_misc[24] = wsum + incl;
                uint32_t run = wsum + incl - local;
#pragma unroll
                for (int k = 0; k < PB; k++) { if (d0 + k < NB) START[d0 + k] = run; run += c[k]; }
                __syncthreads();
            }
            SUFR_STAMP(ph__, 2)                            // 2: bin scan
            const uint32_t total = s_misc[24];
            // claims on bins k * NCT + thread (one wave instruction touches 64 consecutive cursors), by the waves that
            // never store: the first PBH bins of a thread before the staging pass (their latency hides under it), the
            // others (more than NCT * PBH dense digits: rare) after it
            constexpr int PBH = PBC < 8 ? PBC : 8;
            uint32_t base[PBH];
            auto claim = [&](int k0) {
#pragma unroll
                for (int k = 0; k < PBH; k++) {
                    uint32_t d = (uint32_t)(k0 + k) * NCT + threadIdx.x;
                    asm volatile("" : "+v"(d));            // the cursor's address is formed here, not kept across the tile loop
                    base[k] = 0;
                    if (d < NB) { const uint32_t cnt = CNT[d]; if (cnt) base[k] = atomicAdd(&cur[d], cnt); }
                }
            };
            auto settle = [&](int k0) {
#pragma unroll
                for (int k = 0; k < PBH; k++) {
                    const uint32_t d = (uint32_t)(k0 + k) * NCT + threadIdx.x;
                    if (d < NB) CNT[d] = base[k] - START[d];                 // staging slot -> slot of the bucket
                }
            };
            if (claimer) claim(0);
            // staging: a record's slot takes its position
#pragma unroll
            for (int e = E0; e < E1; e++) {
                const uint32_t v = dr[e - E0];
                if (v != 0xffffffffu) s_pos[START[v & 0xfffu] + (v >> 12)] = (uint16_t)(q0 + (uint32_t)e * (64u * NW));
            }
            if (claimer) {
                settle(0);
                for (int k0 = PBH; k0 < PBC && (uint32_t)k0 * NCT < NB; k0 += PBH) { claim(k0); settle(k0); }
            }
            SUFR_STAMP(ph__, 3)                            // 3: claims, staging pass, deltas
            if (last && more) {
                land(tb ^ 1u);                             // (its loads were issued before this unit's stores)
                mybits = nxtbits;
            }
            SUFR_STAMP(ph__, 4)                            // 4: next tile's text to LDS
            __syncthreads();                               // staged; nobody reads the bin starts any more
            {
                uint32_t i0 = threadIdx.x;                 // (opaque, as above)
                asm volatile("" : "+v"(i0));
                for (uint32_t i = i0; i < NB; i += NT) START[i] = 0;        // the next unit counts here
            }
            p_total = total; p_tb = tb; p_tile0 = tile0;
            unit++;
            __syncthreads();
            SUFR_STAMP(ph__, 5)                            // 5: barriers, zeroing
        };
        using I0 = std::integral_constant<int, 0>;
        using IH = std::integral_constant<int, ITER / 2>;
        using IR = std::integral_constant<int, ITER>;
        if (kept <= (uint32_t)CAP) {
            run_unit(I0{}, IR{}, true);
        } else {
            const uint64_t keepbits = mybits;              // (the tile's last unit replaces mybits by the next tile's)
            run_unit(I0{}, IH{}, false);
            mybits = keepbits;
            run_unit(IH{}, IR{}, true);
        }
    }
    // the last unit's copy-out (the LDS addresses are formed again, from an opaque copy of the map size: kept from
    // the prologue they would sit in registers -- or scratch -- across the whole tile loop)
    if (!claimer) {
        uint32_t rows2 = dm.rows;
        asm volatile("" : "+s"(rows2));
        uint32_t* arr2 = reinterpret_cast<uint32_t*>(smem + (size_t)(TW + 4) * 8 + msd_map_bytes(rows2));
        const uint16_t* pos2 = reinterpret_cast<const uint16_t*>(arr2 + 2 * NBa + 32);
        const uint32_t* PT = s_textb + (size_t)p_tb * (TW + 4);
        const uint32_t* delta = arr2 + (size_t)((unit & 1u) ^ 1u) * NBa;
        uint32_t j0 = threadIdx.x - NCT;
        asm volatile("" : "+v"(j0));
        for (uint32_t j = j0; j < p_total; j += NC) {
            const uint32_t pos = pos2[j];
            const uint32_t i = (pos * B) >> 5, sh = (pos * B) & 31u;
            const uint32_t w0 = PT[i], w1 = PT[i + 1], w2 = PT[i + 2];
            Rec rr;
            rr.khi = (uint32_t)((((uint64_t)w0 << 32) | w1) >> (32u - sh));
            rr.klo = (uint32_t)((((uint64_t)w1 << 32) | w2) >> (32u - sh)) & keep_lo;
            rr.idx = (uint32_t)(p_tile0 + pos);
            out[j + delta[dense_digit(rr.khi >> (dshift - 32), map)]] = rr;
        }
    }
    SUFR_STAMP(ph__, 6)
    SUFR_STAMP_FLUSH(0, 8)
}

#endif  // SUFR_HIP_PROBES

// suffix-start bitmap from a bit-packed code stream (alphabets that do not go through k_text_pass_dna): bit i of
// word w <-> position 64 w + i starts a suffix (its code is in elig_codes; positions past the end have code 0)
template <int B>
__global__ void __launch_bounds__(256)
k_startbits_packed(const uint8_t* __restrict__ packed, uint64_t n, uint32_t elig_codes, uint64_t* __restrict__ startbits)
{
    const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= (n + 63) / 64) return;
    const uint8_t* pp = packed + ((w * 64 * B) >> 3);       // 64 * B bits: a whole number of bytes
    uint64_t bits = 0;
    for (int e = 0; e < 64; e++) {
        const uint32_t o = (uint32_t)e * B;
        const uint32_t two = ((uint32_t)pp[o >> 3] << 8) | pp[(o >> 3) + 1];
        const uint32_t code = (two >> (16 - B - (o & 7u))) & ((1u << B) - 1u);
        if (w * 64 + e < n && ((elig_codes >> code) & 1u)) bits |= 1ull << e;
    }
    startbits[w] = bits;
}

// ---------------------------------------------------------------------------------------------
// Segment plans.  A level works on a list of segments (start, size): the buckets of the previous level that
// are too large for the leaf sort.  Segments are dealt to G groups (segment k -> group k % G) so that the
// workgroups of one group (one XCD) fill the same buckets at the same time; slot q = (k % G) * SG + k / G of
// the permuted list holds segment k, SG = ceil(nseg / G).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_seg_units(const uint32_t* __restrict__ seg_size, uint32_t nseg, uint32_t G, uint32_t SG, uint32_t unit,
            uint32_t* __restrict__ units)
{
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q >= G * SG) return;
    const uint32_t k = (q % SG) * G + q / SG;
    units[q] = k < nseg ? (seg_size[k] + unit - 1) / unit : 0u;
}

// tile t of the permuted list: tdesc[t] = {first record, records, segment, 0}
__global__ void __launch_bounds__(256)
k_msd_tiles(const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ seg_size, uint32_t G,
            uint32_t SG, uint32_t unit, const uint32_t* __restrict__ upre /* G*SG exclusive */,
            const unsigned long long* __restrict__ utotal, uint4* __restrict__ tdesc)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint32_t)*utotal) return;
    uint32_t lo = 0, hi = G * SG;                // last q with upre[q] <= t
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (upre[mid] <= t) lo = mid; else hi = mid;
    }
    const uint32_t q = lo;
    const uint32_t k = (q % SG) * G + q / SG;
    const uint32_t i = t - upre[q];
    const uint32_t off = i * unit;
    const uint32_t cnt = min(unit, seg_size[k] - off);
    tdesc[t] = make_uint4(seg_start[k] + off, cnt, k, 0u);
}

// ---------------------------------------------------------------------------------------------
// k_msd_hist: digit counts of every segment (leafcnt[k * NB + d]).  A workgroup takes a contiguous range of
// the tile list and flushes its LDS counters whenever the segment changes.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(THREADS)
k_msd_hist(const Rec* __restrict__ recs, const uint4* __restrict__ tdesc,
           const unsigned long long* __restrict__ utotal, int shift, DigitMap dm, uint32_t* __restrict__ leafcnt)
{
    extern __shared__ __align__(16) uint8_t smem[];
    const LdsMap map = msd_load_map<THREADS>(dm, smem);
    uint32_t* s_cnt = reinterpret_cast<uint32_t*>(smem + msd_map_bytes(dm.rows));     // nbins
    const uint32_t NB = dm.nbins;
    for (uint32_t i = threadIdx.x; i < NB; i += THREADS) s_cnt[i] = 0;
    __syncthreads();
    const uint32_t T = (uint32_t)*utotal;
    const uint32_t per = (T + gridDim.x - 1) / gridDim.x;
    const uint32_t t0 = blockIdx.x * per, t1 = min(t0 + per, T);
    uint32_t seg = 0xffffffffu;
    auto flush = [&](uint32_t k) {
        __syncthreads();
        uint32_t* row = leafcnt + (size_t)k * NB;
        for (uint32_t i = threadIdx.x; i < NB; i += THREADS) {
            const uint32_t c = s_cnt[i];
            if (c) { atomicAdd(&row[i], c); s_cnt[i] = 0; }
        }
        __syncthreads();
    };
    for (uint32_t t = t0; t < t1; t++) {
        const uint4 td = tdesc[t];
        if (td.z != seg) { if (seg != 0xffffffffu) flush(seg); seg = td.z; }
        const Rec* kp = recs + td.x;
        // four keys in flight per lane (the key is the first 8 bytes of a record)
        uint32_t i = threadIdx.x;
        for (; i + 3u * THREADS < td.y; i += 4u * THREADS) {
            uint2 q[4];
#pragma unroll
            for (int u = 0; u < 4; u++) q[u] = load_key_nt(&kp[i + (uint32_t)u * THREADS]);
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint64_t k = ((uint64_t)q[u].y << 32) | q[u].x;
                const uint32_t d = dense_digit((uint32_t)(k >> shift) & dm.raw_mask, map);
                const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)d);
                if (__ballot(d == d0) == ~0ull) { if (lane_id() == 0) atomicAdd(&s_cnt[d0], 64u); }   // (one long run: see k_msd_scatter)
                else atomicAdd(&s_cnt[d], 1u);
            }
        }
        for (; i < td.y; i += THREADS) {
            const uint2 q = load_key_nt(&kp[i]);
            const uint64_t k = ((uint64_t)q.y << 32) | q.x;
            atomicAdd(&s_cnt[dense_digit((uint32_t)(k >> shift) & dm.raw_mask, map)], 1u);
        }
    }
    if (seg != 0xffffffffu) flush(seg);
}

// absolute first slot of every sub-bucket: leafbase[k * NB + d] = seg_start[k] + (off[k * NB + d] - off[k * NB]),
// where off = exclusive scan of leafcnt over the whole table; the cursors start there
__global__ void __launch_bounds__(256)
k_msd_leafbase(const uint32_t* __restrict__ off, const uint32_t* __restrict__ seg_start, uint32_t nseg, uint32_t NB,
               uint32_t* __restrict__ leafbase, uint32_t* __restrict__ leafcur)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint64_t)nseg * NB) return;
    const uint32_t k = (uint32_t)(i / NB);
    const uint32_t v = seg_start[k] + (off[i] - off[(size_t)k * NB]);
    leafbase[i] = v;
    leafcur[i] = v;
}

// ---------------------------------------------------------------------------------------------
// k_msd_scatter: one MSD level over (key, idx) records.  Workgroup w belongs to group w % G and takes every
// R-th tile of its group's part of the tile list (R = workgroups per group), so that the workgroups that run
// together fill the same segment's sub-buckets.  Ranking by LDS atomics, slots claimed on the sub-bucket
// cursors, records staged in LDS in digit order and written as runs.
// ---------------------------------------------------------------------------------------------
template <int NT, int E>
__global__ void __launch_bounds__(NT)
k_msd_scatter(const Rec* __restrict__ in, const uint4* __restrict__ tdesc, const uint32_t* __restrict__ upre,
              uint32_t G, uint32_t SG, const unsigned long long* __restrict__ utotal, int shift, DigitMap dm,
              uint32_t* __restrict__ leafcur, Rec* __restrict__ out)
{
    constexpr int TILEB = NT * E;
    extern __shared__ __align__(16) uint8_t smem[];
    const uint32_t NB = dm.nbins;
    const uint32_t NBa = (NB + 3u) & ~3u;
    uint64_t* s_key = reinterpret_cast<uint64_t*>(smem);                          // TILEB, in digit order
    const LdsMap map = msd_load_map<NT>(dm, smem + (size_t)TILEB * 8);
    uint32_t* s_idx = reinterpret_cast<uint32_t*>(smem + (size_t)TILEB * 8 + msd_map_bytes(dm.rows));   // TILEB
    uint32_t* s_cnt = s_idx + TILEB;                                              // NB: counts -> prefix -> slot delta
    uint32_t* s_misc = s_cnt + NBa;                                               // 32
    uint16_t* s_dig = reinterpret_cast<uint16_t*>(s_misc + 32);                   // TILEB

    const uint32_t g = blockIdx.x % G, r = blockIdx.x / G, R = gridDim.x / G;     // gridDim.x is a multiple of G
    const uint32_t lo = upre[(size_t)g * SG];
    const uint32_t hi = (g + 1 < G) ? upre[(size_t)(g + 1) * SG] : (uint32_t)*utotal;
    // The records of the next tile are loaded before the copy-out of the current one and consumed (pinned) before
    // its stores are issued: loads and stores retire in order, a load issued behind the stores would wait for them.
    uint32_t nlo[E], nhi[E], nix[E];
    uint4 ntd = make_uint4(0u, 0u, 0u, 0u);
    auto fetch = [&](uint32_t t) {
        ntd = tdesc[t];
#pragma unroll
        for (int e = 0; e < E; e++) {
            const uint32_t j = (uint32_t)e * NT + threadIdx.x;
            nlo[e] = 0; nhi[e] = 0; nix[e] = 0;
            if (j < ntd.y) { const Rec rr = in[ntd.x + j]; nlo[e] = rr.klo; nhi[e] = rr.khi; nix[e] = rr.idx; }
        }
    };
    auto pin = [&]() {
#pragma unroll
        for (int e = 0; e < E; e++) asm volatile("" : "+v"(nlo[e]), "+v"(nhi[e]), "+v"(nix[e]));
    };
    if (lo + r < hi) { fetch(lo + r); pin(); }
    SUFR_STAMP_DECL(8)
    for (uint32_t t = lo + r; t < hi; t += R) {
        const uint4 td = ntd;
        __syncthreads();                                   // the previous copy-out is done with the staging area
        SUFR_STAMP(ph__, 0)
        for (uint32_t i = threadIdx.x; i < NB; i += NT) s_cnt[i] = 0;
        uint64_t key[E];
        uint32_t idx[E], dig[E], rank[E];
        uint32_t valid = 0;
#pragma unroll
        for (int e = 0; e < E; e++) {
            const uint32_t j = (uint32_t)e * NT + threadIdx.x;
            key[e] = ((uint64_t)nhi[e] << 32) | nlo[e]; idx[e] = nix[e];
            if (j < td.y) valid |= 1u << e;
        }
#pragma unroll
        for (int e = 0; e < E; e++) dig[e] = dense_digit((uint32_t)(key[e] >> shift) & dm.raw_mask, map);
        __syncthreads();
        SUFR_STAMP(ph__, 1)
#pragma unroll
        for (int e = 0; e < E; e++) {
            // (a bucket that is one long run -- N^k under --allow-ambiguity, poly-A -- puts the same digit in every lane:
            // 64 returning atomics on one LDS address are served one by one; the wave then counts itself instead)
            const bool v = valid & (1u << e);
            const uint64_t vm = __ballot(v);
            const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)dig[e]);
            if (vm == ~0ull && __ballot(dig[e] == d0) == ~0ull) {
                uint32_t b = 0;
                if (lane_id() == 0) b = atomicAdd(&s_cnt[d0], 64u);
                rank[e] = (uint32_t)__builtin_amdgcn_readfirstlane((int)b) + lane_id();
            } else {
                rank[e] = v ? atomicAdd(&s_cnt[dig[e]], 1u) : 0u;
            }
        }
        __syncthreads();
        SUFR_STAMP(ph__, 2)
        MsdClaim<NT> cl;
        msd_claim_begin<NT>(s_cnt, NB, leafcur + (size_t)td.z * NB, s_misc, s_misc + 24, cl);
        SUFR_STAMP(ph__, 3)
        const bool more = t + R < hi;
        if (more) fetch(t + R);
#pragma unroll
        for (int e = 0; e < E; e++) {
            if (valid & (1u << e)) {
                const uint32_t pos = s_cnt[dig[e]] + rank[e];
                s_key[pos] = key[e];
                s_idx[pos] = idx[e];
                s_dig[pos] = (uint16_t)dig[e];
            }
        }
        SUFR_STAMP(ph__, 4)
        msd_claim_end<NT>(s_cnt, NB, cl);
        SUFR_STAMP(ph__, 5)
        if (more) pin();
        SUFR_STAMP(ph__, 6)
        for (uint32_t j = threadIdx.x; j < td.y; j += NT) {
            const uint32_t o = j + s_cnt[s_dig[j]];
            out[o] = make_rec(s_key[j], s_idx[j]);
        }
        SUFR_STAMP(ph__, 7)
    }
    SUFR_STAMP_FLUSH(1, 8)
}

// copy of whole segments (the buckets still too large after the last level): tile by tile
__global__ void __launch_bounds__(256)
k_copy_tiles(const Rec* __restrict__ in, const uint4* __restrict__ tdesc,
             const unsigned long long* __restrict__ utotal, Rec* __restrict__ out)
{
    const uint32_t T = (uint32_t)*utotal;
    for (uint32_t t = blockIdx.x; t < T; t += gridDim.x) {
        const uint4 td = tdesc[t];
        for (uint32_t j = threadIdx.x; j < td.y; j += 256) out[td.x + j] = in[td.x + j];
    }
}

// ---------------------------------------------------------------------------------------------
// Windows of the leaf sort: consecutive sub-buckets ("leaves") of one segment, packed greedily -- a window takes
// leaves while its records stay within CAP.  A leaf of more than BIG <= CAP records is flagged for the next
// MSD level and left out (it also ends the window before it).  Two consecutive windows of an uninterrupted
// stretch hold more than CAP records together, so windows are > 1/2 full on average and ~ CAP - (mean leaf) / 2
// in practice (round 2 cut windows every G = CAP / 2 slots: half-empty workgroups, twice the per-window work).
// One wave per segment walks its leaves 64 at a time: with the window start known, "first leaf that does not
// fit / is big" is a ballot.  EMIT = false counts the windows of every segment (and sets the big flags),
// EMIT = true writes  wdesc[wpre[k] + i] = {first record, records, first leaf's digit, leaves}.
// ---------------------------------------------------------------------------------------------
template <bool EMIT>
__global__ void __launch_bounds__(256)
k_pack_windows(const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ seg_size, uint32_t nseg,
               const uint32_t* __restrict__ leafbase, uint32_t NB, uint32_t CAP, uint32_t BIG,
               uint32_t* __restrict__ wcount, const uint32_t* __restrict__ wpre, uint4* __restrict__ wdesc,
               uint32_t* __restrict__ bigflag)
{
    const uint32_t k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= nseg) return;
    const uint32_t ln = lane_id();
    const uint32_t* lb = leafbase + (size_t)k * NB;
    const uint32_t s0 = seg_start[k], s1 = s0 + seg_size[k];
    (void)s0;
    bool open = false;                   // uniform state: a window is open, its first record / first leaf
    uint32_t wpos = 0, wleaf = 0, nw = 0;
    const uint32_t wbase = EMIT ? wpre[k] : 0u;
    auto close = [&](uint32_t endpos, uint32_t endleaf) {
        if (endpos > wpos) {
            if (EMIT && ln == 0u) wdesc[wbase + nw] = make_uint4(wpos, endpos - wpos, wleaf, endleaf - wleaf);
            nw++;
        }
        open = false;
    };
    for (uint32_t c = 0; c < NB; c += 64) {
        const uint32_t d = c + ln;
        const bool valid = d < NB;
        const uint32_t b = valid ? lb[d] : s1;
        const uint32_t e = (d + 1 < NB) ? lb[d + 1] : s1;
        const bool big = valid && e - b > BIG;
        if (!EMIT && big) bigflag[(size_t)k * NB + d] = 1u;
        const uint32_t nv = min(64u, NB - c);
        uint32_t cur = 0;
        while (cur < nv) {
            if (!open) {
                // leaves from `cur` on: big ones are skipped, the first other one opens a window
                const uint64_t nb = __ballot(valid && !big) & (~0ull << cur);
                if (!nb) break;
                cur = (uint32_t)__builtin_ctzll(nb);
                wpos = (uint32_t)__builtin_amdgcn_readlane((int)b, (int)cur);
                wleaf = c + cur;
                open = true;
            }
            // first leaf from `cur` on that is big or does not fit (the window's own first leaf is neither)
            const uint64_t stop = __ballot(valid && (big || e - wpos > CAP)) & (~0ull << cur);
            if (!stop) break;
            cur = (uint32_t)__builtin_ctzll(stop);
            close((uint32_t)__builtin_amdgcn_readlane((int)b, (int)cur), c + cur);
        }
    }
    if (open) close(s1, NB);
    if (!EMIT && ln == 0u) wcount[k] = nw;
}

// the flagged leaves, in order, as the segment list of the next level
__global__ void __launch_bounds__(256)
k_compact_big(const uint32_t* __restrict__ bigflag, const uint32_t* __restrict__ bigoff,
              const uint32_t* __restrict__ leafbase, const uint32_t* __restrict__ seg_start,
              const uint32_t* __restrict__ seg_size, uint32_t nseg, uint32_t NB,
              uint32_t* __restrict__ new_start, uint32_t* __restrict__ new_size,
              unsigned long long* __restrict__ big_records /* [0] records in all, [1] the largest */)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint64_t)nseg * NB || !bigflag[i]) return;
    const uint32_t k = (uint32_t)(i / NB), d = (uint32_t)(i % NB);
    const uint32_t a = leafbase[i];
    const uint32_t b = d + 1 < NB ? leafbase[i + 1] : seg_start[k] + seg_size[k];
    new_start[bigoff[i]] = a;
    new_size[bigoff[i]] = b - a;
    atomicAdd(big_records, (unsigned long long)(b - a));
    atomicMax(big_records + 1, (unsigned long long)(b - a));
}

// ---------------------------------------------------------------------------------------------
// Finishing a window (replaces the LCP-merge of the reference, sufr_builder.rs:634-767, for suffixes that
// differ inside their K-character keys; the boundary LCP of write(), 893-902, is k_fix_window_lcp below).
// The window's records lie in LDS ordered by their whole key.  Every slot takes its suffix index to SA; a
// record whose key differs from its predecessor's gets  LCP = common characters of the two keys  (exact: the
// keys hold the first K characters of both suffixes and differ).  Records that share their whole key with a
// neighbour form tie runs -- their order and the LCPs inside the run need text beyond the key: they are
// marked in two bitmaps over the output positions (members / run heads; layout of k_build_ties: per 128
// positions M0 M1 H0 H1) for the tie level.  The LCP of the window's first record needs the record before
// it, which another workgroup places: the window leaves its first and last key in out_key and its start in
// `fixlist` for k_fix_window_lcp (at the window's own index: one shared atomic counter serialises ~10^5
// windows per launch on one address).
// ---------------------------------------------------------------------------------------------
struct FinishOut {
    uint32_t* SA;
    uint32_t* LCP;
    unsigned long long* wmask;      // zeroed; 4 words per 128 output positions
    uint32_t* fixlist;              // window starts: window `win` of a level writes entry *nfix + win
    const uint32_t* nfix;           // entries of the levels before this one (advanced between the levels)
    uint32_t fixcap;
    int b, K;                       // bits per character, characters per key
};

// lane i takes the value of lane i - 1 / i + 1 of its wave (lane 0 / 63 keep their own): whole-wave DPP shifts
__device__ __forceinline__ uint64_t wave_shr1_u64(uint64_t v)
{
    const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
    const uint32_t a = (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xf, 0xf, false);
    const uint32_t b = (uint32_t)__builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xf, 0xf, false);
    return ((uint64_t)b << 32) | a;
}
__device__ __forceinline__ uint64_t wave_shl1_u64(uint64_t v)
{
    const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
    const uint32_t a = (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, 0x130, 0xf, 0xf, false);
    const uint32_t b = (uint32_t)__builtin_amdgcn_update_dpp(hi, hi, 0x130, 0xf, 0xf, false);
    return ((uint64_t)b << 32) | a;
}

template <int NT>
__device__ __forceinline__ void leaf_finish(const uint64_t* s_key, const uint32_t* s_idx, unsigned long long* s_bits,
                                            uint32_t start, uint32_t cnt, Rec* __restrict__ out_rec,
                                            const FinishOut& fo, uint32_t win)
{
    // s_bits: 2 * nwords u64 (members, heads) for the positions from start & ~63 on
    const uint32_t p0 = start & ~63u;
    const uint32_t nwords = ((start + cnt - p0) + 63u) / 64u;
    unsigned long long* s_M = s_bits;
    unsigned long long* s_H = s_bits + nwords;
    for (uint32_t i = threadIdx.x; i < 2u * nwords; i += NT) s_bits[i] = 0ull;
    __syncthreads();
    // consecutive lanes hold consecutive slots: the neighbours' keys come over the wave (DPP shifts), only the
    // first and the last lane of a wave read theirs from the LDS
    const uint32_t ln = lane_id();
    for (uint32_t j0 = 0; j0 < cnt; j0 += NT) {
        const uint32_t j = j0 + threadIdx.x;
        const bool in = j < cnt;
        const uint64_t k = in ? s_key[j] : 0ull;
        uint64_t kp = wave_shr1_u64(k), kn = wave_shl1_u64(k);
        if (ln == 0u) kp = (in && j > 0) ? s_key[j - 1] : 0ull;
        if (ln == 63u) kn = (j + 1 < cnt) ? s_key[j + 1] : 0ull;
        if (in) {
            const bool tie_prev = j > 0 && kp == k;
            const bool tie_next = j + 1 < cnt && kn == k;
            fo.SA[start + j] = s_idx[j];
            if (j > 0 && !tie_prev) fo.LCP[start + j] = plain_key_common(kp, k, fo.b, fo.K);
            if (tie_prev || tie_next) {
                const uint32_t rel = start + j - p0;
                atomicOr(&s_M[rel >> 6], 1ull << (rel & 63u));
                if (!tie_prev) atomicOr(&s_H[rel >> 6], 1ull << (rel & 63u));
            }
        }
    }
    if (threadIdx.x == 0) {
        out_rec[start] = make_rec(s_key[0], s_idx[0]);
        out_rec[start + cnt - 1] = make_rec(s_key[cnt - 1], s_idx[cnt - 1]);
        const uint32_t i = *fo.nfix + win;
        if (i < fo.fixcap) fo.fixlist[i] = start;
    }
    __syncthreads();
    for (uint32_t wi = threadIdx.x; wi < nwords; wi += NT) {
        const uint32_t gw = (p0 >> 6) + wi;                 // 64-position word -> M at 4 (gw / 2) + gw % 2, H two further
        const size_t at = (size_t)(gw >> 1) * 4 + (gw & 1u);
        const unsigned long long M = s_M[wi], H = s_H[wi];
        if (M) {
            // the first and the last word may be shared with a neighbouring window
            if (wi == 0 || wi + 1 == nwords) { atomicOr(&fo.wmask[at], M); if (H) atomicOr(&fo.wmask[at + 2], H); }
            else { fo.wmask[at] = M; fo.wmask[at + 2] = H; }
        }
    }
}

// LCP of the first record of every finished window (and of every group left to the deeper levels) with the
// record before it: both keys are in `keys` -- a window leaves its first and last key there, a group all of
// its records -- and differ, because the two records lie in different buckets.
__global__ void __launch_bounds__(256)
k_fix_window_lcp(const uint32_t* __restrict__ fixlist, const uint32_t* __restrict__ nfix, uint32_t fixcap,
                 const Rec* __restrict__ recs, uint32_t* __restrict__ LCP, int b, int K)
{
    const uint32_t n = min(*nfix, fixcap);
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const uint32_t p = fixlist[i];
        LCP[p] = p ? plain_key_common(rec_key(recs[p - 1]), rec_key(recs[p]), b, K) : 0u;
    }
}

// starts of the groups that go to the deeper levels as they are, appended to the fix list
__global__ void __launch_bounds__(256)
k_append_starts(const uint32_t* __restrict__ seg_start, uint32_t nseg, uint32_t* __restrict__ fixlist,
                const uint32_t* __restrict__ nfix, uint32_t fixcap)
{
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nseg) return;
    const uint32_t i = *nfix + k;
    if (i < fixcap) fixlist[i] = seg_start[k];
}

// *nfix += *add (+ extra): the fix list grows by the windows of a level
__global__ void k_advance_fix(uint32_t* __restrict__ nfix, const unsigned long long* __restrict__ add, uint32_t extra)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) *nfix += (add ? (uint32_t)*add : 0u) + extra;
}

// records / runs per 128 positions from the tie bitmaps (the counts k_build_ties' offsets are scanned from)
__global__ void __launch_bounds__(256)
k_tie_counts(const unsigned long long* __restrict__ wmask, uint32_t nwin, uint32_t* __restrict__ wcnt, uint32_t stride /* second row: a multiple of 4, for the one-launch scans */)
{
    const uint32_t w = blockIdx.x * 256 + threadIdx.x;
    if (w >= nwin) return;
    wcnt[w] = (uint32_t)(__popcll(wmask[(size_t)w * 4]) + __popcll(wmask[(size_t)w * 4 + 1]));
    wcnt[(size_t)stride + w] = (uint32_t)(__popcll(wmask[(size_t)w * 4 + 2]) + __popcll(wmask[(size_t)w * 4 + 3]));
}

// groups handed to the re-keying levels without a finisher pass before them: size, depth and period of every
// segment (what k_group_extent derives from sorted keys)
__global__ void __launch_bounds__(256)
k_groups_from_segments(const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ seg_size, uint32_t L,
                       uint32_t depth, const uint32_t* __restrict__ idxs, uint32_t istride, const uint8_t* __restrict__ text,
                       int detect_period, uint32_t* __restrict__ heads, uint32_t* __restrict__ sizes,
                       uint32_t* __restrict__ newdepth, uint8_t* __restrict__ newperiod, uint32_t* __restrict__ maxsize,
                       const uint32_t* __restrict__ depth_of = nullptr)
{
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= L) return;
    const uint32_t h = seg_start[k];
    heads[k] = h;
    sizes[k] = seg_size[k];
    if (depth_of) depth = depth_of[k];                 // (groups of different depths: run buckets taken out after the first level)
    newdepth[k] = depth;
    uint32_t pi = 1;
    if (depth >= 12 && detect_period) {
        const uint8_t* e = text + (uint64_t)idxs[(size_t)h * istride] + depth;    // one past the common prefix
        const uint32_t win = depth < 16 ? depth : 16;
        for (uint32_t c = 1; c <= 8 && c * 2 <= win; c++) {
            bool ok = true;
            for (uint32_t i = 1; i + c <= win && ok; i++) ok = e[-(int)i] == e[-(int)(i + c)];
            if (ok) { pi = c; break; }
        }
    }
    newperiod[k] = (uint8_t)pi;
    if (seg_size[k] > __hip_atomic_load(maxsize, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(maxsize, seg_size[k]);
}

// ---------------------------------------------------------------------------------------------
// Counting digit of the leaf sort: the first characters below a leaf's prefix, range-coded with the
// character frequencies of the text (cum[v] = share of suffix starts whose character code is below v, as a
// 32-bit fraction).  Like any arithmetic code it is monotone in the lexicographic order of the characters --
// the interval of a string lies inside its prefix's, intervals of different characters do not overlap -- and
// it spreads ordinary text evenly over the 2^k buckets whatever the code width (DNA: 6 bases fill 4096
// buckets, the rare '$' '%' 'N' take slivers).  Any monotone function of the key may define the buckets,
// because the members of a bucket are then ranked by their whole key.
// ---------------------------------------------------------------------------------------------
struct CharModel {
    const uint32_t* cum;   // [2^b + 1] cumulative shares, cum[0] = 0, cum[2^b] = 0xffffffff
    int b;                 // bits per character code
    int lastbit;           // lowest key bit that belongs to a character: 64 - K * b
    int mchars;            // characters worth coding (more cannot move a record to another bucket by much)
};

// k_leaf_sort_lsd: the fallback of k_leaf_sort for the windows it flagged (a bucket of more than bmax
// records, or more leaves than the counting digit has values): stable LSD passes of <= 8 bits over
//     leaf ordinal | key bits [lowbit, hibit)          (lowbit = the key's last character: the whole key)
// Wave w holds slots w * E * 64 + e * 64 + lane, so rank order == slot order: per pass every wave ranks its strip
// with ballots (match-any on the digit) and a per-wave LDS counter row, a prefix over waves and bins gives the
// final slots.  Sorted in LDS, written once.
template <int NT, int E>
__global__ void __launch_bounds__(NT)
k_leaf_sort_lsd(const Rec* __restrict__ in, Rec* __restrict__ out_rec, const uint4* __restrict__ wdesc,
                const unsigned long long* __restrict__ wtotal, const uint32_t* __restrict__ wslow, int hibit,
                int lowbit, DigitMap dm, FinishOut fo)
{
    constexpr int CAP = NT * E;
    extern __shared__ __align__(16) uint8_t smem[];
    const uint32_t W = (uint32_t)*wtotal;
    uint64_t* s_key = reinterpret_cast<uint64_t*>(smem);                                  // CAP
    const LdsMap map = msd_load_map<NT>(dm, smem + (size_t)CAP * 8);
    uint32_t* s_idx = reinterpret_cast<uint32_t*>(smem + (size_t)CAP * 8 + msd_map_bytes(dm.rows));   // CAP
    uint32_t* s_misc = s_idx + CAP;                                                       // 32
    uint32_t* s_tot = s_misc + 32;                                                        // 256
    uint16_t* s_wcnt = reinterpret_cast<uint16_t*>(s_tot + 256);                          // NW * 256
    unsigned long long* s_bits = reinterpret_cast<unsigned long long*>(s_tot);            // tie bitmaps (same area, afterwards)
    const int nlow = hibit > lowbit ? hibit - lowbit : 0;
    for (uint32_t win = blockIdx.x; win < W; win += gridDim.x) {
    if (!wslow[win]) continue;
    const uint4 wd = wdesc[win];
    const uint32_t start = wd.x, cnt = wd.y, d0 = wd.z, nleaves = wd.w;
    const int ordbits = nleaves > 1u ? 32 - __clz((int)(nleaves - 1u)) : 0;
    __syncthreads();                                        // tables loaded; the previous window is out of the LDS
    constexpr int NW = NT / WAVE;
    constexpr int BINS = 256;
    const int wv = threadIdx.x >> 6;
    const uint32_t ln = lane_id();
    const uint32_t strip0 = (uint32_t)wv * (E * WAVE);
    const int tbits = nlow + ordbits;
    uint64_t key[E];
    uint32_t idx[E];
    auto leaf_ord = [&](uint64_t k) -> uint32_t {
        return ordbits ? dense_digit((uint32_t)(k >> hibit) & dm.raw_mask, map) - d0 : 0u;
    };
    // ---- fallback: stable LSD passes on  ordinal | key bits [lowbit, hibit) ---------------------
    // (strip layout: wave w holds slots w * E * 64 + e * 64 + lane, so rank order == slot order)
    uint32_t valid = 0;
#pragma unroll
    for (int e = 0; e < E; e++) {
        const uint32_t j = strip0 + (uint32_t)e * WAVE + ln;
        key[e] = 0; idx[e] = 0;
        if (j < cnt) { valid |= 1u << e; const Rec r = in[start + j]; key[e] = rec_key(r); idx[e] = r.idx; }
    }
    const int npass = (tbits + 7) / 8;
    const int w = npass ? (tbits + npass - 1) / npass : 1;  // digit width of every pass (the top one may be narrower)
    const uint32_t nb = 1u << w;
    const uint64_t lowmask = nlow ? ((1ull << nlow) - 1ull) : 0ull;
    auto sort_word = [&](uint64_t k) -> uint64_t {
        uint64_t sw = nlow ? ((k >> lowbit) & lowmask) : 0ull;
        if (ordbits) sw |= (uint64_t)leaf_ord(k) << nlow;
        return sw;
    };
    __syncthreads();
    for (int p = 0; p < npass; p++) {
        for (uint32_t i = threadIdx.x; i < (uint32_t)NW * nb / 2u; i += NT) reinterpret_cast<uint32_t*>(s_wcnt)[i] = 0;
        __syncthreads();
        uint32_t dig[E], rank[E];
#pragma unroll
        for (int e = 0; e < E; e++) dig[e] = (uint32_t)(sort_word(key[e]) >> (p * w)) & (nb - 1u);
        auto my = SUFR_LDS_VOLATILE(uint16_t, s_wcnt + (size_t)wv * nb);
#pragma unroll
        for (int e = 0; e < E; e++) {
            const bool v = valid & (1u << e);
            const uint32_t d = v ? dig[e] : 0u;
            uint32_t mlo, mhi;
            match_digit_t<0>(d, w, v, mlo, mhi);
            const uint32_t before = my[d];
            const uint32_t lower = __builtin_amdgcn_mbcnt_hi(mhi, __builtin_amdgcn_mbcnt_lo(mlo, 0u));
            rank[e] = before + lower;
            if (v && lower == 0) my[d] = (uint16_t)(before + __popc(mlo) + __popc(mhi));
        }
        __syncthreads();
        // per digit: exclusive prefix over the waves (in place) and the window's count
        for (uint32_t d = threadIdx.x; d < nb; d += NT) {
            uint32_t run = 0;
#pragma unroll
            for (int x = 0; x < NW; x++) {
                const uint32_t c = s_wcnt[(size_t)x * nb + d];
                s_wcnt[(size_t)x * nb + d] = (uint16_t)run;
                run += c;
            }
            s_tot[d] = run;
        }
        __syncthreads();
        // exclusive scan of the <= 256 digit counts (first four waves, one value per lane)
        uint32_t sv = 0, sincl = 0;
        if (threadIdx.x < BINS) {
            sv = threadIdx.x < nb ? s_tot[threadIdx.x] : 0u;
            sincl = sv;
#pragma unroll
            for (int o = 1; o < WAVE; o <<= 1) {
                const uint32_t t = __shfl_up(sincl, o, WAVE);
                if ((int)ln >= o) sincl += t;
            }
            if (ln == 63) s_misc[wv] = sincl;
        }
        __syncthreads();
        if (threadIdx.x < nb) {
            uint32_t wbase = 0;
            for (int x = 0; x < wv; x++) wbase += s_misc[x];
            s_tot[threadIdx.x] = wbase + sincl - sv;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < E; e++)
            if (valid & (1u << e)) rank[e] += s_tot[dig[e]] + my[dig[e]];
        // records are in registers: the staging area takes them at their new slots
#pragma unroll
        for (int e = 0; e < E; e++) {
            if (valid & (1u << e)) { s_key[rank[e]] = key[e]; s_idx[rank[e]] = idx[e]; }
        }
        __syncthreads();
        if (p + 1 < npass) {
#pragma unroll
            for (int e = 0; e < E; e++) {
                const uint32_t j = strip0 + (uint32_t)e * WAVE + ln;
                if (j < cnt) { key[e] = s_key[j]; idx[e] = s_idx[j]; }
            }
        }
    }
    if (npass == 0) {                                       // nothing to sort on: the window is one run of equal keys
#pragma unroll
        for (int e = 0; e < E; e++) {
            const uint32_t j = strip0 + (uint32_t)e * WAVE + ln;
            if (j < cnt) { s_key[j] = key[e]; s_idx[j] = idx[e]; }
        }
        __syncthreads();
    }
    leaf_finish<NT>(s_key, s_idx, s_bits, start, cnt, out_rec, fo, win);
    }
}

// ---------------------------------------------------------------------------------------------
// Sorting the groups of a re-keying level (the records of the large tie groups, keyed with run keys).
// Round 2 sorted a level with ~8 stable LSD passes over all its (key, index, group) records -- five on key
// digits, three on the group ordinal to bring the groups back together: 512 bytes of HBM traffic per record and level,
// although the records of a group never leave the group's own range and a typical group holds 10^3 records.
// Here a group is sorted where it lies:
//   k_group_psegs        the groups (start[g], size[g]) as "leaves" of pseudo-segments of GS_PS groups, so that
//                        k_pack_windows packs consecutive groups of <= CAP records into windows and flags the others;
//   k_group_sort_small   a window is loaded once, sorted in LDS by  group ordinal | key bits [lowbit, 64)  with stable
//                        8-bit passes (ballot ranking, as k_leaf_sort_lsd) and written once: 24 bytes per record;
//   k_group_sort_big     a flagged group (> CAP records, up to `giant` = 16 384) is sorted by ONE workgroup with stable
//                        LSD passes over its own range, ping-pong between the two key / index arrays: 200 KB that stay
//                        in the L2 between the passes.  (Groups come off a work queue.)
//   k_large_*            larger groups: copied side by side, sorted by the whole-device passes on (group, key), copied
//                        back (one workgroup would be a long tail; sufr_launch.inc, group_sort_run).
// The group array (seg) is not moved at all.  Also used for the tie runs of --max-query-len builds (apply_max_query_len).
// ---------------------------------------------------------------------------------------------
static constexpr uint32_t GS_PS = 512;         // groups per pseudo-segment (one wave packs the windows of one)

// leafbase[k * GS_PS + d] = start of group k * GS_PS + d (m for the padding), pseudo-segment k = its groups' range
__global__ void __launch_bounds__(256)
k_group_psegs(const uint32_t* __restrict__ start, uint32_t L, uint32_t m, uint32_t npseg, uint32_t* __restrict__ leafbase,
              uint32_t* __restrict__ pst, uint32_t* __restrict__ psz)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < npseg * GS_PS) leafbase[i] = i < L ? start[i] : m;
    if (i < npseg) {
        const uint32_t a = start[i * GS_PS];
        const uint32_t b = (i + 1) * GS_PS < L ? start[(i + 1) * GS_PS] : m;
        pst[i] = a; psz[i] = b - a;
    }
}

// groups above `giant` records, in any order: lg[slot] = g, lsz[slot] = size[g]; count[0] = how many, count[1] = their records
__global__ void __launch_bounds__(256)
k_group_large(const uint32_t* __restrict__ size, uint32_t L, uint32_t giant, unsigned long long* __restrict__ count,
              uint32_t* __restrict__ lg, uint32_t* __restrict__ lsz)
{
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= L || size[g] <= giant) return;
    const uint32_t slot = (uint32_t)atomicAdd(count, 1ull);
    atomicAdd(count + 1, (unsigned long long)size[g]);
    lg[slot] = g; lsz[slot] = size[g];
}

// their records side by side: compact position t of large group q = lg slot holds record start[lg[q]] + (t - loff[q]), keyed
// (q, key) for whole-device passes ...
__global__ void __launch_bounds__(256)
k_large_gather(const uint64_t* __restrict__ kA, const uint32_t* __restrict__ iA, const uint32_t* __restrict__ gstart,
               const uint32_t* __restrict__ lg, const uint32_t* __restrict__ loff, uint32_t nlarge, uint32_t mlarge,
               uint64_t* __restrict__ kC, uint32_t* __restrict__ iC, uint32_t* __restrict__ sC)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= mlarge) return;
    uint32_t lo = 0, hi = nlarge;                      // last q with loff[q] <= t
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (loff[mid] <= t) lo = mid; else hi = mid; }
    const uint32_t src = gstart[lg[lo]] + (t - loff[lo]);
    kC[t] = kA[src]; iC[t] = iA[src]; sC[t] = lo;
}
// ... and back: sorted by (q, key), position t is the (t - loff[q])-th record of its group
__global__ void __launch_bounds__(256)
k_large_return(const uint64_t* __restrict__ kC, const uint32_t* __restrict__ iC, const uint32_t* __restrict__ sC,
               const uint32_t* __restrict__ gstart, const uint32_t* __restrict__ lg, const uint32_t* __restrict__ loff,
               uint32_t mlarge, uint64_t* __restrict__ kB, uint32_t* __restrict__ iB)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= mlarge) return;
    const uint32_t q = sC[t];
    const uint32_t dst = gstart[lg[q]] + (t - loff[q]);
    kB[dst] = kC[t]; iB[dst] = iC[t];
}

// list of the flagged groups: big[off[g]] = g
__global__ void __launch_bounds__(256)
k_group_biglist(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ off, uint32_t L, uint32_t* __restrict__ big)
{
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g < L && flag[g]) big[off[g]] = g;
}

template <int NT, int E>
__global__ void __launch_bounds__(NT)
k_group_sort_small(const uint64_t* __restrict__ kin, const uint32_t* __restrict__ iin, const uint32_t* __restrict__ seg,
                   uint64_t* __restrict__ kout, uint32_t* __restrict__ iout, const uint4* __restrict__ wdesc,
                   const unsigned long long* __restrict__ wtotal, int lowbit)
{
    constexpr int CAP = NT * E;
    constexpr int NW = NT / WAVE;
    constexpr int BINS = 256;
    extern __shared__ __align__(16) uint8_t smem[];
    uint64_t* s_key = reinterpret_cast<uint64_t*>(smem);                                  // CAP
    uint32_t* s_idx = reinterpret_cast<uint32_t*>(smem + (size_t)CAP * 8);                // CAP
    uint16_t* s_ord = reinterpret_cast<uint16_t*>(s_idx + CAP);                           // CAP
    uint32_t* s_misc = reinterpret_cast<uint32_t*>(s_ord + CAP);                          // 32
    uint32_t* s_tot = s_misc + 32;                                                        // 256
    uint16_t* s_wcnt = reinterpret_cast<uint16_t*>(s_tot + BINS);                         // NW * 256
    const uint32_t W = (uint32_t)*wtotal;
    const int wv = threadIdx.x >> 6;
    const uint32_t ln = lane_id();
    const uint32_t strip0 = (uint32_t)wv * (E * WAVE);
    const int nlow = 64 - lowbit;                           // key bits to sort
    const int npk = (nlow + 7) / 8;                         // passes on key bits (8 bits each, the top one may be narrower)
    for (uint32_t win = blockIdx.x; win < W; win += gridDim.x) {
        const uint4 wd = wdesc[win];
        const uint32_t start = wd.x, cnt = wd.y;
        const uint32_t g0 = seg[start];                     // the window's first group
        const uint32_t nleaves = seg[start + cnt - 1u] - g0 + 1u;
        const int ordbits = nleaves > 1u ? 32 - __clz((int)(nleaves - 1u)) : 0;
        const int npo = (ordbits + 7) / 8;                  // passes on the group ordinal
        __syncthreads();                                    // the previous window is out of the LDS
        // strip layout: wave w holds slots w * E * 64 + e * 64 + lane, so rank order == slot order
        uint64_t key[E];
        uint32_t idx[E], ord[E];
        uint32_t valid = 0;
#pragma unroll
        for (int e = 0; e < E; e++) {
            const uint32_t j = strip0 + (uint32_t)e * WAVE + ln;
            key[e] = 0; idx[e] = 0; ord[e] = 0;
            if (j < cnt) { valid |= 1u << e; key[e] = kin[start + j]; idx[e] = iin[start + j]; ord[e] = seg[start + j] - g0; }
        }
        auto my = SUFR_LDS_VOLATILE(uint16_t, s_wcnt + (size_t)wv * BINS);
        for (int p = 0; p < npk + npo; p++) {
            for (uint32_t i = threadIdx.x; i < (uint32_t)NW * BINS / 2u; i += NT) reinterpret_cast<uint32_t*>(s_wcnt)[i] = 0;
            __syncthreads();
            const bool onkey = p < npk;
            const int sh = onkey ? lowbit + 8 * p : 8 * (p - npk);
            const int w = onkey ? (p == npk - 1 ? nlow - 8 * p : 8) : (p - npk == npo - 1 ? ordbits - 8 * (p - npk) : 8);
            const uint32_t nb = 1u << w;
            uint32_t dig[E], rank[E];
#pragma unroll
            for (int e = 0; e < E; e++)
                dig[e] = onkey ? (uint32_t)(key[e] >> sh) & (nb - 1u) : (ord[e] >> sh) & (nb - 1u);
#pragma unroll
            for (int e = 0; e < E; e++) {
                const bool v = valid & (1u << e);
                const uint32_t d = v ? dig[e] : 0u;
                uint32_t mlo, mhi;
                match_digit_t<0>(d, w, v, mlo, mhi);
                const uint32_t before = my[d];
                const uint32_t lower = __builtin_amdgcn_mbcnt_hi(mhi, __builtin_amdgcn_mbcnt_lo(mlo, 0u));
                rank[e] = before + lower;
                if (v && lower == 0) my[d] = (uint16_t)(before + __popc(mlo) + __popc(mhi));
            }
            __syncthreads();
            for (uint32_t d = threadIdx.x; d < nb; d += NT) {       // per digit: exclusive prefix over the waves, window count
                uint32_t run = 0;
#pragma unroll
                for (int x = 0; x < NW; x++) {
                    const uint32_t c = s_wcnt[(size_t)x * BINS + d];
                    s_wcnt[(size_t)x * BINS + d] = (uint16_t)run;
                    run += c;
                }
                s_tot[d] = run;
            }
            __syncthreads();
            uint32_t sv = 0, sincl = 0;                             // exclusive scan of the <= 256 digit counts
            if (threadIdx.x < BINS) {
                sv = threadIdx.x < nb ? s_tot[threadIdx.x] : 0u;
                sincl = sv;
#pragma unroll
                for (int o = 1; o < WAVE; o <<= 1) {
                    const uint32_t t = __shfl_up(sincl, o, WAVE);
                    if ((int)ln >= o) sincl += t;
                }
                if (ln == 63) s_misc[wv] = sincl;
            }
            __syncthreads();
            if (threadIdx.x < nb) {
                uint32_t wbase = 0;
                for (int x = 0; x < wv; x++) wbase += s_misc[x];
                s_tot[threadIdx.x] = wbase + sincl - sv;
            }
            __syncthreads();
#pragma unroll
            for (int e = 0; e < E; e++)
                if (valid & (1u << e)) rank[e] += s_tot[dig[e]] + my[dig[e]];
            // the records are in registers: the staging area takes them at their new slots
#pragma unroll
            for (int e = 0; e < E; e++)
                if (valid & (1u << e)) { s_key[rank[e]] = key[e]; s_idx[rank[e]] = idx[e]; s_ord[rank[e]] = (uint16_t)ord[e]; }
            __syncthreads();
            if (p + 1 < npk + npo) {
#pragma unroll
                for (int e = 0; e < E; e++) {
                    const uint32_t j = strip0 + (uint32_t)e * WAVE + ln;
                    if (j < cnt) { key[e] = s_key[j]; idx[e] = s_idx[j]; ord[e] = s_ord[j]; }
                }
            }
        }
        // (npk + npo >= 1: nlow >= 1) -- sorted in LDS, written once, in order
        for (uint32_t j = threadIdx.x; j < cnt; j += NT) { kout[start + j] = s_key[j]; iout[start + j] = s_idx[j]; }
    }
}

// A group too large for a window: stable LSD passes of D bits on key bits [lowbit, 64) over the group's own range, by one
// workgroup (ballot ranking per wave, running cursors per digit across the tiles of a pass).  NP passes, NP odd: the
// records start in (kA, iA) and end in (kB, iB).
template <int NT, int E>
__global__ void __launch_bounds__(NT)
k_group_sort_big(uint64_t* kA, uint32_t* iA, uint64_t* kB, uint32_t* iB,
                 const uint32_t* __restrict__ gstart, const uint32_t* __restrict__ gsize, const uint32_t* __restrict__ biglist,
                 const unsigned long long* __restrict__ nbig, unsigned int* __restrict__ queue, int lowbit, int D, int NP,
                 uint32_t giant /* groups above this are sorted by whole-device passes (k_large_*) */)
{
    constexpr int TILEB = NT * E;
    constexpr int NW = NT / WAVE;
    extern __shared__ __align__(16) uint8_t smem[];
    const uint32_t NB = 1u << D;
    uint32_t* s_gbase = reinterpret_cast<uint32_t*>(smem);  // NB: running output cursor of a digit
    uint32_t* s_gdelta = s_gbase + NB;                      // NB
    uint32_t* s_tot = s_gdelta + NB;                        // NB   tile count -> tile prefix
    uint32_t* s_misc = s_tot + NB;                          // 32
    uint8_t* s_union = reinterpret_cast<uint8_t*>(s_misc + 32);
    uint16_t* s_wcnt = reinterpret_cast<uint16_t*>(s_union); // NW * NB u16 during ranking, then the staging arrays
    uint64_t* s_key = reinterpret_cast<uint64_t*>(s_union);
    uint32_t* s_idx = reinterpret_cast<uint32_t*>(s_key + TILEB);
    const int wv = threadIdx.x >> 6;
    const uint32_t ln = lane_id();
    const uint32_t total_big = (uint32_t)*nbig;
    const int nlow = 64 - lowbit;
    for (;;) {
        __syncthreads();
        if (threadIdx.x == 0) s_misc[31] = atomicAdd(queue, 1u);
        __syncthreads();
        const uint32_t q = s_misc[31];
        if (q >= total_big) break;
        const uint32_t g = biglist[q];
        const uint32_t c0 = gstart[g], c1 = c0 + gsize[g];
        if (c1 - c0 > giant) continue;
        for (int p = 0; p < NP; p++) {
            const uint64_t* in_key = (p & 1) ? kB : kA; const uint32_t* in_idx = (p & 1) ? iB : iA;
            uint64_t* out_key = (p & 1) ? kA : kB; uint32_t* out_idx = (p & 1) ? iA : iB;
            // digit of this pass: D bits from lowbit + p D on; passes beyond the key's top sort on nothing (a copy)
            const int sh = lowbit + p * D;
            const int w = sh >= 64 ? 0 : (64 - sh < D ? 64 - sh : D);
            const uint32_t mask = w ? (1u << w) - 1u : 0u;
            (void)nlow;
            // histogram of the group on this digit -> starting cursors
            for (uint32_t i = threadIdx.x; i < NB; i += NT) s_tot[i] = 0;
            __syncthreads();
            for (uint32_t j = c0 + threadIdx.x; j < c1; j += NT)
                atomicAdd(&s_tot[w ? (uint32_t)(in_key[j] >> sh) & mask : 0u], 1u);
            __syncthreads();
            for (uint32_t i = threadIdx.x; i < NB; i += NT) s_gbase[i] = c0;
            __syncthreads();
            block_scan_bins_t<NT>(s_tot, s_gbase, s_gdelta, NB, s_misc, s_misc + 24);     // s_tot: exclusive prefix
            for (uint32_t i = threadIdx.x; i < NB; i += NT) s_gbase[i] = c0 + s_tot[i];
            __syncthreads();
            for (uint32_t tile0 = c0; tile0 < c1; tile0 += TILEB) {
                __syncthreads();  // previous tile's copy-out done before the union region is reused
                for (uint32_t i = threadIdx.x; i < (NW * NB + 1) / 2; i += NT) reinterpret_cast<uint32_t*>(s_wcnt)[i] = 0;
                __syncthreads();
                uint64_t key[E];
                uint32_t idx[E], dig[E], rank[E];
                uint32_t valid = 0;
                const uint32_t strip0 = tile0 + wv * (E * WAVE);
#pragma unroll
                for (int e = 0; e < E; e++) {
                    const uint32_t j = strip0 + e * WAVE + ln;
                    key[e] = 0; idx[e] = 0;
                    if (j < c1) { valid |= 1u << e; key[e] = in_key[j]; idx[e] = in_idx[j]; }
                }
                auto my = SUFR_LDS_VOLATILE(uint16_t, s_wcnt + (size_t)wv * NB);
#pragma unroll
                for (int e = 0; e < E; e++) dig[e] = w ? (uint32_t)(key[e] >> sh) & mask : 0u;
#pragma unroll
                for (int e = 0; e < E; e++) {
                    const bool v = valid & (1u << e);
                    const uint32_t d = v ? dig[e] : 0u;
                    uint32_t mlo, mhi;
                    match_digit_t<0>(d, D, v, mlo, mhi);
                    const uint32_t before = my[d];
                    const uint32_t lower = __builtin_amdgcn_mbcnt_hi(mhi, __builtin_amdgcn_mbcnt_lo(mlo, 0u));
                    rank[e] = before + lower;
                    if (v && lower == 0) my[d] = (uint16_t)(before + __popc(mlo) + __popc(mhi));
                }
                __syncthreads();
                for (uint32_t d = threadIdx.x; d < NB; d += NT) {
                    uint32_t run = 0;
#pragma unroll
                    for (int x = 0; x < NW; x++) {
                        const uint32_t c = s_wcnt[(size_t)x * NB + d];
                        s_wcnt[(size_t)x * NB + d] = (uint16_t)run;
                        run += c;
                    }
                    s_tot[d] = run;
                }
                __syncthreads();
                block_scan_bins_t<NT>(s_tot, s_gbase, s_gdelta, NB, s_misc, s_misc + 24);   // advances the cursors
                const uint32_t total = s_misc[24];
#pragma unroll
                for (int e = 0; e < E; e++)
                    if (valid & (1u << e)) rank[e] += s_tot[dig[e]] + my[dig[e]];
                __syncthreads();
#pragma unroll
                for (int e = 0; e < E; e++)
                    if (valid & (1u << e)) { s_key[rank[e]] = key[e]; s_idx[rank[e]] = idx[e]; }
                __syncthreads();
                for (uint32_t j = threadIdx.x; j < total; j += NT) {
                    const uint64_t k = s_key[j];
                    const uint32_t o = j + s_gdelta[w ? (uint32_t)(k >> sh) & mask : 0u];
                    out_key[o] = k;
                    out_idx[o] = s_idx[j];
                }
            }
            __syncthreads();   // (workgroup scope: the next pass reads what this one wrote)
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_leaf_sort: the wave-level sort inside a bucket (replaces merge_sort of a partition,
// sufr_builder.rs:601-631).  Workgroups loop over the windows: <= CAP records of consecutive leaves are
// loaded once, sorted in LDS and written once, in order, to their place in the output arrays.
//   fast path   one counting pass (LDS atomics) on  leaf ordinal | a monotone digest of the next characters
//               (<= LEAF_T1 bits), then every record ranks itself inside its bucket by comparing whole keys --
//               buckets hold one to three records on ordinary text, so the window ends up ordered by the entire
//               64-bit key.  The digest: DNA3 (the fixed 3-bit code table): A C G T -> 0 1 2 3 of six characters,
//               as two reads of a table of three-character halves in LDS (dna3_digest12 and dna3_half_entry,
//               sufr_runkey.h); otherwise the range coder of CharModel (table look-ups in LDS).  Any monotone
//               function of the key will do: the members of a bucket are ranked by their whole keys.
//               Every record reads the four key slots from its bucket's start, RB records of a thread in flight
//               together (a loop per record paid an LDS round trip per member), and counts the members before
//               it (leaf_rank4, sufr_runkey.h) -- unclamped and unmasked: what follows a bucket is larger;
//   fallback    a window with a bucket of more than `bmax` records (long repeats) is left to k_leaf_sort_lsd.
// Either way the window is ordered by at least the key bits above `lowbit`, which is what k_finish needs.
// The loads of the next window are issued before the current one is copied out.
// ---------------------------------------------------------------------------------------------
static constexpr int LEAF_CS_MAX = 1024;       // entries of the combined-character table of the range coder
static constexpr int LEAF_KEY_PAD = 4;         // key slots behind a window: the ranking reads up to three past its last record

template <int NT, int E, int LEAF_T1, bool DNA3>          // LEAF_T1: bits of the counting digit (2^T1 LDS counters)
__global__ void __launch_bounds__(NT)
k_leaf_sort(const Rec* __restrict__ in, Rec* __restrict__ out_rec, const uint4* __restrict__ wdesc,
            const unsigned long long* __restrict__ wtotal, uint32_t* __restrict__ wslow, int hibit, DigitMap dm,
            CharModel cm, FinishOut fo, uint32_t bmax)
{
    constexpr int CAP = NT * E;
    constexpr int NW = NT / WAVE;
    constexpr int NB1 = 1 << LEAF_T1;
    constexpr int PB1 = NB1 / NT;
    extern __shared__ __align__(16) uint8_t smem[];
    const uint32_t W = (uint32_t)*wtotal;
    uint32_t win = blockIdx.x;
    if (win >= W) return;
    constexpr int KEYS = CAP + LEAF_KEY_PAD;
    uint64_t* s_key = reinterpret_cast<uint64_t*>(smem);                                  // KEYS: the window + the ranking's sentinels
    const LdsMap map = msd_load_map<NT>(dm, smem + (size_t)KEYS * 8);
    // range coder over `cs` characters at a time: s_cum[v] = interval {low, high} of the cs-character string v
    const int cs = cm.b * 3 <= 10 ? 3 : (cm.b * 2 <= 10 ? 2 : 1);
    const uint32_t ncomb = 1u << (cm.b * cs);
    uint2* s_cum = reinterpret_cast<uint2*>(smem + (size_t)KEYS * 8 + msd_map_bytes(dm.rows));   // ncomb <= LEAF_CS_MAX
    uint32_t* s_idx = reinterpret_cast<uint32_t*>(s_cum + (DNA3 ? 0 : LEAF_CS_MAX));     // CAP
    uint32_t* s_misc = s_idx + CAP;                                                       // 32
    uint32_t* s_cnt = s_misc + 32;                                                        // NB1 (fast path)
    uint16_t* s_dg = reinterpret_cast<uint16_t*>(s_cnt + NB1);                            // DNA3_HALF_ENTRIES (DNA3)
    if constexpr (DNA3) {
        for (uint32_t v = threadIdx.x; v < DNA3_HALF_ENTRIES; v += NT) s_dg[v] = dna3_half_entry(v);
    }
    if constexpr (!DNA3) {
        for (uint32_t v = threadIdx.x; v < ncomb; v += NT) {
            uint32_t lo = 0, wd32 = 0xffffffffu;
            for (int i = cs - 1; i >= 0; i--) {
                const uint32_t c = (v >> (cm.b * i)) & ((1u << cm.b) - 1u);
                const uint32_t a = __umulhi(wd32, cm.cum[c]), bnd = __umulhi(wd32, cm.cum[c + 1]);
                lo += a; wd32 = bnd - a;
            }
            s_cum[v] = make_uint2(lo, lo + wd32);
        }
    }

    const int wv = threadIdx.x >> 6;
    const uint32_t ln = lane_id();
    const uint32_t cmask = ncomb - 1u;
    unsigned long long* s_bits = reinterpret_cast<unsigned long long*>(s_cnt);            // tie bitmaps (after the ranking)
    int avail = (hibit - cm.lastbit) / (cm.b * cs);         // cs-character steps the key holds below the leaf prefix
    if (avail > (cm.mchars + cs - 1) / cs) avail = (cm.mchars + cs - 1) / cs;
    if (avail < 0) avail = 0;
    const int stepbits = cm.b * cs;

#ifdef SUFR_HIP_PROBES
    const uint32_t abl = bmax >> 24;                        // phase ablation (timing probes only: results are wrong)
    bmax &= 0xffffffu;
#else
    constexpr uint32_t abl = 0;
#endif
    uint64_t key[E];
    uint32_t idx[E];
    uint4 wd = wdesc[win];
    // records of a window are dealt to the threads round-robin: slot e * NT + thread
    auto load_window = [&](const uint4& d) {
#pragma unroll
        for (int e = 0; e < E; e++) {
            const uint32_t j = (uint32_t)e * NT + threadIdx.x;
            if (j < d.y) { const Rec r = in[d.x + j]; key[e] = rec_key(r); idx[e] = r.idx; }
        }
    };
    load_window(wd);
    for (;;) {
        const uint32_t start = wd.x, cnt = wd.y, d0 = wd.z, nleaves = wd.w;
        const int ordbits = nleaves > 1u ? 32 - __clz((int)(nleaves - 1u)) : 0;
        bool staged = false;                                // the window lies sorted in LDS
        auto leaf_ord = [&](uint64_t k) -> uint32_t {
            return ordbits ? dense_digit((uint32_t)(k >> hibit) & dm.raw_mask, map) - d0 : 0u;
        };
        if (cnt != 0 && abl != 4) {
            staged = true;
            // ---- fast path: counting pass on  ordinal | digest of the next characters -----------------------
            const int kbits = ordbits <= LEAF_T1 ? LEAF_T1 - ordbits : 0;
            const uint32_t nb1 = ordbits <= LEAF_T1 ? (uint32_t)NB1 : 0u;
            __syncthreads();                                // tables loaded; the previous window is out of the LDS
            for (uint32_t i = threadIdx.x; i < nb1; i += NT) s_cnt[i] = 0;
            __syncthreads();
            bool fast = nb1 != 0;
            uint32_t dr[E];
            if (fast) {
#pragma unroll
                for (int e = 0; e < E; e++) {
                    dr[e] = 0;
                    if ((uint32_t)e * NT + threadIdx.x < cnt) {
                        uint32_t dg;
                        if constexpr (DNA3) {
                            // the six characters below the leaf prefix (zeros below the key's last character)
                            const uint32_t t = (uint32_t)((key[e] << (64 - hibit)) >> 46);
                            // (two table reads, sufr_runkey.h; a digit of six bits or fewer takes the first three characters only)
                            const uint32_t hi = s_dg[t >> 9];
                            const uint32_t d12 = kbits > 6 ? dna3_digest12_halves(hi, s_dg[t & 511u]) : (hi & 63u) << 6;
                            dg = abl == 1 ? 0u : d12 >> (12 - (kbits > 12 ? 12 : kbits));
                            if (kbits > 12) dg <<= kbits - 12;
                        } else {
                            uint32_t lo = 0, wd32 = 0xffffffffu;
                            int sh = hibit;
                            for (int i = 0; i < (abl == 1 ? 0 : avail); i++) {
                                sh -= stepbits;
                                const uint2 cu = s_cum[(uint32_t)(key[e] >> sh) & cmask];
                                const uint32_t a = __umulhi(wd32, cu.x), bnd = __umulhi(wd32, cu.y);
                                lo += a; wd32 = bnd - a;
                            }
                            dg = kbits ? lo >> (32 - kbits) : 0u;
                        }
                        const uint32_t d = (leaf_ord(key[e]) << kbits) | (kbits ? dg : 0u);
                        dr[e] = d | (atomicAdd(&s_cnt[d], 1u) << LEAF_T1);
                    }
                }
                __syncthreads();
                // exclusive scan of the counters (PB1 consecutive ones per thread) and the largest bucket
                const uint32_t b0 = threadIdx.x * PB1;
                uint32_t c[PB1];
                uint32_t local = 0, big = 0;
#pragma unroll
                for (int k = 0; k < PB1; k++) { c[k] = s_cnt[b0 + k]; local += c[k]; big = max(big, c[k]); }
                uint32_t incl = local;
#pragma unroll
                for (int o = 1; o < WAVE; o <<= 1) {
                    const uint32_t t = __shfl_up(incl, o, WAVE);
                    if ((int)ln >= o) incl += t;
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) big = max(big, (uint32_t)__shfl_xor((int)big, o, WAVE));
                if (ln == 63) s_misc[wv] = incl;
                if (ln == 0) s_misc[16 + (wv & 15)] = big;
                __syncthreads();
                uint32_t wbase = 0;
                for (int x = 0; x < wv; x++) wbase += s_misc[x];
                uint32_t run = wbase + incl - local;
#pragma unroll
                for (int k = 0; k < PB1; k++) { s_cnt[b0 + k] = run; run += c[k]; }
                uint32_t mx = 0;
#pragma unroll
                for (int x = 0; x < NW; x++) mx = max(mx, s_misc[16 + x]);
                fast = mx <= bmax;
                __syncthreads();
            }
            if (fast) {
                // every record goes to its bucket's range in arrival order; a bucket of one record (most of them) is
                // final, the members of a larger one rank themselves by their whole keys and move once more
                // (kept per record: ls = the bucket's start | its size << 16 -- a window holds fewer than 2^14 records -- and dr,
                // whose high bits are the arrival rank)
                uint32_t ls[E];
#pragma unroll
                for (int e = 0; e < E; e++) {
                    ls[e] = 0;
                    if ((uint32_t)e * NT + threadIdx.x < cnt) {
                        const uint32_t d = dr[e] & (NB1 - 1u);
                        const uint32_t lo = s_cnt[d];
                        const uint32_t sz = (d + 1u < (uint32_t)NB1 ? s_cnt[d + 1u] : cnt) - lo;
                        ls[e] = lo | (sz << 16);
                        const uint32_t p = lo + (dr[e] >> LEAF_T1);
                        s_key[p] = key[e]; s_idx[p] = idx[e];
                    }
                }
                // the ranking reads four slots at a time from a bucket's start whatever its size, unclamped and unmasked.  That is
                // right only while every key past a bucket is LARGER AS A WHOLE 64-BIT KEY than the bucket's members, which rests on
                // three things together: (1) k_pack_windows keeps a window inside one segment, so all records of a window agree on
                // the key bits above `hibit`; (2) below them the counting digit is  leaf ordinal | digest,  and dense_digit is
                // monotone in the raw digit at `hibit`, the digest monotone in the bits below it -- a larger digit means a larger
                // key; (3) past the window's last record lie these sentinels, the largest key, which a slot past its bucket tests
                // with `less` only (leaf_mate_before: a < sz <= i).  A window that spanned two segments would break (1) and with it
                // the ranking, silently.  The reads stay inside the key area: lo + 3 <= cnt + 2 < CAP + LEAF_KEY_PAD
                if (threadIdx.x < LEAF_KEY_PAD - 1) s_key[cnt + threadIdx.x] = ~0ull;
                __syncthreads();
                uint32_t cr[E];                             // rank inside the bucket
                if (abl != 2) {
                    // the first four slots, RB records' reads in flight together.  Straight-line: a bucket of one record ranks itself
                    // first (nothing in its four slots is before it).  A slot of a row past the window's end (ls == 0) reads the
                    // window's first four keys and compares them with a key[e] that load_window never assigned (whatever the
                    // register holds, the previous window's key at most): a rank that nothing below uses, since ls == 0 fails both
                    // size tests
                    constexpr int RB = NT >= 1024 ? 2 : 4;          // (1024 threads: 128 registers per lane)
#pragma unroll
                    for (int h = 0; h < E; h += RB) {
                        uint64_t kt[RB][4];
#pragma unroll
                        for (int q = 0; q < RB; q++) {
                            if (h + q < E) {
#pragma unroll
                                for (int i = 0; i < 4; i++) kt[q][i] = s_key[(ls[h + q] & 0xffffu) + (uint32_t)i];
                            }
                        }
#pragma unroll
                        for (int q = 0; q < RB; q++) {
                            const int e = h + q;
                            if (e < E) cr[e] = leaf_rank4(kt[q], key[e], 0u, dr[e] >> LEAF_T1);
                            // (one record's compares at a time: interleaved, their lane masks outnumber the scalar registers)
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                    // larger buckets: the rest of their members, four at a time (1024 threads: one, for the registers)
                    constexpr uint32_t TB = NT >= 1024 ? 1 : 4;
#pragma unroll
                    for (int e = 0; e < E; e++) {
                        if (ls[e] > (4u << 16 | 0xffffu)) {
                            const uint32_t lo = ls[e] & 0xffffu, sz = ls[e] >> 16, a = dr[e] >> LEAF_T1;
                            uint32_t c = 0;
                            for (uint32_t i = 4u; i < sz; i += TB) {
                                uint64_t kb[TB];
#pragma unroll
                                for (uint32_t j = 0; j < TB; j++) kb[j] = s_key[lo + i + j];
#pragma unroll
                                for (uint32_t j = 0; j < TB; j++) c += leaf_mate_before(kb[j], key[e], i + j, a);
                            }
                            cr[e] += c;
                        }
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < E; e++) cr[e] = dr[e] >> LEAF_T1;
                }
                __syncthreads();
#pragma unroll
                for (int e = 0; e < E; e++) {
                    if ((uint32_t)(ls[e] > (1u << 16 | 0xffffu)) & (uint32_t)(cr[e] != dr[e] >> LEAF_T1)) {
                        const uint32_t p = (ls[e] & 0xffffu) + cr[e];
                        s_key[p] = key[e]; s_idx[p] = idx[e];
                    }
                }
                __syncthreads();
            } else {
                if (threadIdx.x == 0) wslow[win] = 1u;      // k_leaf_sort_lsd takes this window
                staged = false;
            }
        }
        // next window: its loads fly while this one is finished out of the LDS
        const uint32_t cur_win = win;
        win += gridDim.x;
        const bool more = win < W;
        if (more) { wd = wdesc[win]; load_window(wd); }
        if (staged && abl != 3) leaf_finish<NT>(s_key, s_idx, s_bits, start, cnt, out_rec, fo, cur_win);
        if (!more) break;
    }
}

}  // namespace sufr
