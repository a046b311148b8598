// sufr_scan.inc -- the scan and the reduction over the lanes of a workgroup, and the sweep of per-tile summaries by one
// workgroup (included by sufr_kernels.hip before sufr_search.inc; DESIGN.md section 10.2).  Device only.
//
// The analysis passes (k-mers, repeats, LZ, shared, BWT) cut the ranks into tiles, leave a summary per tile, let one
// workgroup sweep the summaries and use the result in a second pass.  What is combined differs -- sums, maxima, KmerSum,
// BwtLink, RepBest -- and lives in the *_scan.h headers; how it moves across lanes and tiles is the same and is written here
// once, with its barriers.
//
// An operator Op is a struct with
//   V                  the value: trivially copyable, made of 32- or 64-bit words
//   identity()         combine(identity(), x) == combine(x, identity()) == x
//   combine(left, right)   associative; `left` is what lies nearer to rank 0.  Not assumed commutative, except by
//                      wg_reduce_op and tile_reduce, which say so.
// A wave has 64 lanes, here as everywhere in this build.

#include <type_traits>

namespace sufr {

template <typename T>
struct SumOp {
    using V = T;
    static __device__ __forceinline__ V identity() { return 0; }
    static __device__ __forceinline__ V combine(V a, V b) { return a + b; }
};

struct MaxOp {
    using V = uint64_t;
    static __device__ __forceinline__ V identity() { return 0; }
    static __device__ __forceinline__ V combine(V a, V b) { return a > b ? a : b; }
};

// v of the lane `o` below (DOWN false) or above (DOWN true) this one in its wave, word by word
template <bool DOWN, typename V>
__device__ __forceinline__ V lane_shift(const V& v, int o)
{
    static_assert(std::is_trivially_copyable<V>::value && sizeof(V) % 4 == 0, "a value is made of 32-bit words");
    uint32_t w[sizeof(V) / 4];
    __builtin_memcpy(w, &v, sizeof(V));
#pragma unroll
    for (uint32_t k = 0; k < sizeof(V) / 4; k++) w[k] = DOWN ? __shfl_down(w[k], o) : __shfl_up(w[k], o);
    V r;
    __builtin_memcpy(&r, w, sizeof(V));
    return r;
}

// before: the lanes below this one, in lane order; after (BOTH only): the lanes above it; total: all of them
template <typename V>
struct WgScan { V before, after, total; };

// The scan over the 64 * WAVES lanes of a workgroup.  Inside a wave the values move by shuffles; the wave totals pass
// through lds (WAVES values, free again on return; the total of a wave is the same in both directions).
template <typename Op, int WAVES, bool BOTH = false>
__device__ __forceinline__ WgScan<typename Op::V> wg_scan_op(const typename Op::V& mine, typename Op::V* lds)
{
    using V = typename Op::V;
    static_assert(WAVES == 4 || WAVES == 16, "256 or 1024 lanes");
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    V f = mine, b = mine;                               // inclusive: lanes 0 .. lane, lanes lane .. 63
    for (int o = 1; o < 64; o <<= 1) {
        const V u = lane_shift<false>(f, o);
        if (lane >= (uint32_t)o) f = Op::combine(u, f);
        if (BOTH) { const V d = lane_shift<true>(b, o); if (lane + (uint32_t)o < 64u) b = Op::combine(b, d); }
    }
    if (lane == 63) lds[w] = f;
    V fe = lane_shift<false>(f, 1), be = BOTH ? lane_shift<true>(b, 1) : Op::identity();
    if (lane == 0) fe = Op::identity();
    if (lane == 63) be = Op::identity();
    __syncthreads();                                    // every wave's total is in lds before any lane reads one
    V pw = Op::identity(), sw = Op::identity(), tot = Op::identity();
    for (uint32_t k = 0; k < (uint32_t)WAVES; k++) {
        const V t = lds[k];
        if (k < w) pw = Op::combine(pw, t);
        if (BOTH && k > w) sw = Op::combine(sw, t);
        tot = Op::combine(tot, t);
    }
    __syncthreads();                                    // every lane has read the totals before the caller's next scan writes lds
    return WgScan<V>{Op::combine(pw, fe), Op::combine(be, sw), tot};
}

// The scan of the query kernels: the exclusive scan of N per-lane sums over the 256 lanes of a workgroup (v: in place), tot:
// the workgroup totals; s_w: 4 * N words of LDS, free again on return.  wg_scan_op over N sum columns gives the same numbers;
// this form, which takes the exclusive value as inclusive - own instead of one more shuffle, is kept because the generic one
// cost k_smem_emit 12 VGPRs (44 -> 56; profiles/scan_refactor_ab.txt).  The barriers are those of wg_scan_op.
template <int N>
__device__ __forceinline__ void wg_scan(uint64_t (&v)[N], uint64_t (&tot)[N], uint64_t* s_w)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint64_t inc[N];
#pragma unroll
    for (int n = 0; n < N; n++) inc[n] = v[n];
    for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
        for (int n = 0; n < N; n++) { const uint64_t u = __shfl_up(inc[n], o); if (lane >= (uint32_t)o) inc[n] += u; }
    }
    if (lane == 63) {
#pragma unroll
        for (int n = 0; n < N; n++) s_w[4 * n + w] = inc[n];
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < N; n++) { inc[n] -= v[n]; v[n] = 0; tot[n] = 0; }
    for (uint32_t k = 0; k < 4; k++) {
#pragma unroll
        for (int n = 0; n < N; n++) { if (k < w) v[n] += s_w[4 * n + k]; tot[n] += s_w[4 * n + k]; }
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < N; n++) v[n] += inc[n];
}

// The combination over the 64 * WAVES lanes of a workgroup, valid in lane 0.  For COMMUTATIVE operators only: the lanes
// are folded as a tree, not in lane order.  lds: WAVES values, free again on return.
template <typename Op, int WAVES>
__device__ __forceinline__ typename Op::V wg_reduce_op(typename Op::V v, typename Op::V* lds)
{
    for (int o = 32; o > 0; o >>= 1) v = Op::combine(v, lane_shift<true>(v, o));
    if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();                                    // every wave's value is in lds before lane 0 reads it
    if (threadIdx.x == 0) for (uint32_t k = 1; k < (uint32_t)WAVES; k++) v = Op::combine(v, lds[k]);
    __syncthreads();                                    // lane 0 has read them before the caller's next reduction writes lds
    return v;
}

// One workgroup of 1024 lanes sweeps ntiles elements.  Lane i folds its block [i per, (i + 1) per), per = ceil(ntiles /
// 1024) (the upper lanes may have none), one scan joins the lanes, then every lane walks its block again:
// store(t, own, exclusive) with own = load(t) and exclusive = everything before t in array order, or after t when
// BACKWARD.  load(t) may read what store(t, ..) of the same t overwrites, and nothing else that any store writes: the lanes
// are not ordered against each other after the scan, so a load that looks beyond its own element (k_bwt_carry reads
// sums[t + 1], which may lie in the next lane's block) needs a store that writes another array.  Returns the total; lds: 16
// values.
template <typename Op, bool BACKWARD, typename Load, typename Store>
__device__ __forceinline__ typename Op::V tile_sweep(uint64_t ntiles, Load load, Store store, typename Op::V* lds)
{
    using V = typename Op::V;
    const uint64_t per = (ntiles + 1023) / 1024, i0 = (uint64_t)threadIdx.x * per, b0 = i0 < ntiles ? i0 : ntiles,
                   b1 = b0 + per < ntiles ? b0 + per : ntiles;
    V mine = Op::identity();
    for (uint64_t t = b0; t < b1; t++) mine = Op::combine(mine, load(t));
    const WgScan<V> sc = wg_scan_op<Op, 16, BACKWARD>(mine, lds);
    if (!BACKWARD) {
        V run = sc.before;
        for (uint64_t t = b0; t < b1; t++) { const V own = load(t); store(t, own, run); run = Op::combine(run, own); }
    } else {
        V run = sc.after;
        for (uint64_t t = b1; t > b0; t--) { const V own = load(t - 1); store(t - 1, own, run); run = Op::combine(own, run); }
    }
    return sc.total;
}

// The combination of ntiles elements by one workgroup of 1024 lanes, valid in lane 0.  For COMMUTATIVE operators only:
// lane i takes elements i, i + 1024, ...  lds: 16 values.
template <typename Op, typename Load>
__device__ __forceinline__ typename Op::V tile_reduce(uint64_t ntiles, Load load, typename Op::V* lds)
{
    typename Op::V v = Op::identity();
    for (uint64_t t = threadIdx.x; t < ntiles; t += 1024) v = Op::combine(v, load(t));
    return wg_reduce_op<Op, 16>(v, lds);
}

}  // namespace sufr
