// Host-side shim around sufr_amd/csrc/sufr_lz_scan.h (the range minimum over a min pyramid, the searches of
// sufr_repeat_scan.h over a pyramid of the suffix array's values, the decision of one rank and the packed table entry that
// the LPF / LZ77 kernels run), so that the device's arithmetic can be held to linear scans on the CPU.  With -DLZ_SHIM_MAIN
// it is a stand-alone program that runs the same comparison by itself (built with -fsanitize=address,undefined by
// tests/test_lz_host.py).  Test infrastructure.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../sufr_amd/csrc/sufr_lz_scan.h"

namespace {
struct ShimAcc {
    const uint64_t *a, *up;
    mutable uint64_t reads;
    uint64_t at(uint32_t level, uint64_t off, uint64_t i) const { reads++; return level ? up[off + i] : a[i]; }
};
}

extern "C" {

// entries of the array of the coarser levels (at least 1, so that a caller can always allocate)
uint64_t shim_lz_pyramid_size(uint64_t s) { return sufr::rep_level_offset(s, sufr::rep_levels(s) + 1) + 1; }
uint32_t shim_lz_levels(uint64_t s) { return sufr::rep_levels(s); }

// the coarser levels of a[0..s) into up (shim_lz_pyramid_size(s) entries)
void shim_lz_pyramid(const uint64_t* a, uint64_t s, uint64_t* up)
{
    const uint32_t levels = sufr::rep_levels(s);
    for (uint32_t k = 1; k <= levels; k++) {
        const uint64_t* in = k == 1 ? a : up + sufr::rep_level_offset(s, k - 1);
        uint64_t* out = up + sufr::rep_level_offset(s, k);
        const uint64_t n_in = sufr::rep_level_size(s, k - 1), n_out = sufr::rep_level_size(s, k);
        for (uint64_t i = 0; i < n_out; i++) {
            uint64_t low = ~(uint64_t)0;
            for (uint64_t j = i * 64; j < n_in && j < i * 64 + 64; j++) if (in[j] < low) low = in[j];
            out[i] = low;
        }
    }
}

// min a[lo, hi); *reads (may be null) receives the entries it read
uint64_t shim_lz_range_min(const uint64_t* a, const uint64_t* up, uint64_t s, uint64_t lo, uint64_t hi, uint64_t* reads)
{
    const ShimAcc acc{a, up, 0};
    const uint64_t m = sufr::lz_range_min(acc, s, lo, hi);
    if (reads) *reads = acc.reads;
    return m;
}

// n ranges at once: out[i] = min a[lo[i], hi[i]); returns the largest number of reads of one of them
uint64_t shim_lz_range_min_many(const uint64_t* a, const uint64_t* up, uint64_t s, const uint64_t* lo, const uint64_t* hi, uint64_t n, uint64_t* out)
{
    uint64_t most = 0;
    for (uint64_t i = 0; i < n; i++) {
        const ShimAcc acc{a, up, 0};
        out[i] = sufr::lz_range_min(acc, s, lo[i], hi[i]);
        if (acc.reads > most) most = acc.reads;
    }
    return most;
}

// the two searches of every rank over the values sa[0..s) as the LPF pass runs them: left[r] the largest j < r with
// sa[j] < sa[r] (REP_NONE if none), right[r] the smallest j > r with sa[j] < sa[r] (s if none)
void shim_lz_neighbours(const uint64_t* sa, const uint64_t* up, uint64_t s, uint64_t* left, uint64_t* right)
{
    const ShimAcc acc{sa, up, 0};
    for (uint64_t r = 0; r < s; r++) {
        left[r] = sa[r] ? sufr::rep_search_left(acc, s, r, sa[r] - 1) : sufr::REP_NONE;
        right[r] = sufr::rep_search_right(acc, s, r, sa[r]);
    }
}

// LPF and SRC by rank (lpf[r], src[r] belong to position sa[r]) with the room of every rank handed in
void shim_lz_rank_all(const uint64_t* sa, const uint64_t* up_sa, const uint64_t* lcp, const uint64_t* up_lcp, uint64_t s, const uint64_t* room,
                      uint64_t* lpf, uint64_t* src)
{
    const ShimAcc a{sa, up_sa, 0}, l{lcp, up_lcp, 0};
    for (uint64_t r = 0; r < s; r++) {
        const sufr::LzEntry e = sufr::lz_rank(a, l, s, r, sa[r], room[r]);
        lpf[r] = e.lpf; src[r] = e.src;
    }
}

void shim_lz_pick(int has1, uint64_t m1, uint64_t q1, int has2, uint64_t m2, uint64_t q2, uint64_t room, uint64_t* out)
{
    const sufr::LzEntry e = sufr::lz_pick(has1 != 0, m1, q1, has2 != 0, m2, q2, room);
    out[0] = e.lpf; out[1] = e.src;
}

uint32_t shim_lz_tab_pack(uint32_t last, uint32_t hops) { return sufr::lz_tab_pack(last, hops); }
uint32_t shim_lz_tab_last(uint32_t e) { return sufr::lz_tab_last(e); }
uint32_t shim_lz_tab_hops(uint32_t e) { return sufr::lz_tab_hops(e); }

}

#ifdef LZ_SHIM_MAIN
int main()
{
    uint64_t x = 88172645463325252ull, cases = 0;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    const uint64_t lens[] = {1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 8192, 262143, 262144, 262145, 300000};
    for (const uint64_t s : lens)
        for (int kind = 0; kind < 4; kind++) {
            // 0: random; 1: constant; 2: ascending; 3: descending
            std::vector<uint64_t> a(s);
            for (uint64_t r = 0; r < s; r++) a[r] = kind == 0 ? rnd() % 1000 : kind == 1 ? 5 : kind == 2 ? r : s - r;
            std::vector<uint64_t> up(shim_lz_pyramid_size(s));
            shim_lz_pyramid(a.data(), s, up.data());
            const uint64_t bound = 2 * 64 * ((uint64_t)sufr::rep_levels(s) + 1);
            for (int q = 0; q < 400; q++) {
                uint64_t lo = rnd() % s, hi = lo + 1 + rnd() % (s - lo);
                if (q == 0) { lo = 0; hi = s; }
                if (q == 1 && s > 64) { lo = 64; hi = s - s % 64; }
                if (q == 2 && s > 4096) { lo = 4096; hi = s; }
                if (q == 3) hi = lo + 1;
                if (hi <= lo) continue;
                uint64_t want = ~(uint64_t)0, reads = 0;
                for (uint64_t j = lo; j < hi; j++) if (a[j] < want) want = a[j];
                if (shim_lz_range_min(a.data(), up.data(), s, lo, hi, &reads) != want || reads > bound) {
                    printf("range_min: s %llu kind %d [%llu, %llu) reads %llu\n", (unsigned long long)s, kind, (unsigned long long)lo, (unsigned long long)hi, (unsigned long long)reads);
                    return 1;
                }
                cases++;
            }
            if (shim_lz_range_min(a.data(), up.data(), s, 3, 3, nullptr) != ~(uint64_t)0) return 1;
            // the neighbours with a smaller value, by two stack passes
            std::vector<uint64_t> left(s), right(s), st;
            shim_lz_neighbours(a.data(), up.data(), s, left.data(), right.data());
            for (uint64_t r = 0; r < s; r++) {
                while (!st.empty() && a[st.back()] >= a[r]) st.pop_back();
                if (left[r] != (st.empty() ? sufr::REP_NONE : st.back())) { printf("left: s %llu kind %d rank %llu\n", (unsigned long long)s, kind, (unsigned long long)r); return 1; }
                st.push_back(r);
            }
            st.clear();
            for (uint64_t r = s; r > 0; r--) {
                while (!st.empty() && a[st.back()] >= a[r - 1]) st.pop_back();
                if (right[r - 1] != (st.empty() ? s : st.back())) { printf("right: s %llu kind %d rank %llu\n", (unsigned long long)s, kind, (unsigned long long)(r - 1)); return 1; }
                st.push_back(r - 1);
            }
            cases += 2 * s;
        }
    uint64_t o[2];
    shim_lz_pick(1, 5, 10, 1, 5, 20, 9, o); if (o[0] != 5 || o[1] != 10) return 1;      // the tie goes to j1
    shim_lz_pick(1, 4, 10, 1, 5, 20, 9, o); if (o[0] != 5 || o[1] != 20) return 1;
    shim_lz_pick(1, 7, 10, 0, 0, 0, 3, o); if (o[0] != 3 || o[1] != 10) return 1;       // the clip
    shim_lz_pick(0, 0, 0, 1, 7, 20, 0, o); if (o[0] != 0 || o[1] != sufr::LZ_NONE) return 1;
    shim_lz_pick(0, 0, 0, 0, 0, 0, 9, o); if (o[0] != 0 || o[1] != sufr::LZ_NONE) return 1;
    shim_lz_pick(1, 0, 10, 1, 0, 20, 9, o); if (o[0] != 0 || o[1] != sufr::LZ_NONE) return 1;
    if (shim_lz_tab_last(shim_lz_tab_pack(16383, 16383)) != 16383 || shim_lz_tab_hops(shim_lz_tab_pack(16383, 16383)) != 16383) return 1;
    printf("ok %llu\n", (unsigned long long)cases);
    return 0;
}
#endif
