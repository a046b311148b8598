// Host-side shim around sufr_amd/csrc/sufr_repeat_scan.h (the min pyramid's index arithmetic, the two nearest-smaller-value
// searches and the popcount-prefix count the repeat kernels run), so that the device's arithmetic can be held to a linear
// scan on the CPU.  With -DREPEAT_SHIM_MAIN it is a stand-alone program that runs the same comparison by itself (built with
// -fsanitize=address,undefined by tests/test_repeat_host.py).  Test infrastructure.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../sufr_amd/csrc/sufr_repeat_scan.h"

namespace {
struct ShimAcc {
    const uint64_t *ell, *up;
    uint64_t s;
    uint64_t at(uint32_t level, uint64_t off, uint64_t i) const { return level ? up[off + i] : ell[i]; }
    uint64_t sa(uint64_t r) const { return r; }
};
}

extern "C" {

// entries of the array of the coarser levels (at least 1, so that a caller can always allocate)
uint64_t shim_rep_pyramid_size(uint64_t s) { return sufr::rep_level_offset(s, sufr::rep_levels(s) + 1) + 1; }
uint32_t shim_rep_levels(uint64_t s) { return sufr::rep_levels(s); }
uint64_t shim_rep_level_size(uint64_t s, uint32_t k) { return sufr::rep_level_size(s, k); }

// the coarser levels of ell[0..s) into up (shim_rep_pyramid_size(s) entries)
void shim_rep_pyramid(const uint64_t* ell, uint64_t s, uint64_t* up)
{
    const uint32_t levels = sufr::rep_levels(s);
    for (uint32_t k = 1; k <= levels; k++) {
        const uint64_t* in = k == 1 ? ell : up + sufr::rep_level_offset(s, k - 1);
        uint64_t* out = up + sufr::rep_level_offset(s, k);
        const uint64_t n_in = sufr::rep_level_size(s, k - 1), n_out = sufr::rep_level_size(s, k);
        for (uint64_t i = 0; i < n_out; i++) {
            uint64_t low = ~(uint64_t)0;
            for (uint64_t j = i * 64; j < n_in && j < i * 64 + 64; j++) if (in[j] < low) low = in[j];
            out[i] = low;
        }
    }
}

uint64_t shim_rep_search_left(const uint64_t* ell, const uint64_t* up, uint64_t s, uint64_t r, uint64_t v)
{
    return sufr::rep_search_left(ShimAcc{ell, up, s}, s, r, v);
}
uint64_t shim_rep_search_right(const uint64_t* ell, const uint64_t* up, uint64_t s, uint64_t r, uint64_t v)
{
    return sufr::rep_search_right(ShimAcc{ell, up, s}, s, r, v);
}
// both searches of every rank with v = ell[r]
void shim_rep_search_all(const uint64_t* ell, const uint64_t* up, uint64_t s, uint64_t* left, uint64_t* right)
{
    const ShimAcc acc{ell, up, s};
    for (uint64_t r = 0; r < s; r++) { left[r] = sufr::rep_search_left(acc, s, r, ell[r]); right[r] = sufr::rep_search_right(acc, s, r, ell[r]); }
}

// flags[0..s) (bytes 0 / 1) as words and their exclusive popcount prefix ((s + 63) / 64 entries each)
void shim_rep_words(const uint8_t* flags, uint64_t s, uint64_t* words, uint64_t* prefix)
{
    uint64_t run = 0;
    for (uint64_t i = 0; i < (s + 63) / 64; i++) {
        uint64_t w = 0;
        for (uint64_t r = i * 64; r < s && r < i * 64 + 64; r++) if (flags[r]) w |= (uint64_t)1 << (r - i * 64);
        words[i] = w; prefix[i] = run;
        run += (uint64_t)__builtin_popcountll(w);
    }
}
uint64_t shim_rep_flagged(const uint64_t* words, const uint64_t* prefix, uint64_t lo, uint64_t hi) { return sufr::rep_flagged(words, prefix, lo, hi); }
int shim_rep_left_diverse(const uint64_t* words, const uint64_t* prefix, uint64_t a, uint64_t b) { return sufr::rep_left_diverse(words, prefix, a, b) ? 1 : 0; }
uint64_t shim_rep_clip(uint64_t lcp, uint64_t room_prev, uint64_t room_cur) { return sufr::rep_clip(lcp, room_prev, room_cur); }
uint64_t shim_rep_room(const uint64_t* starts, uint64_t num, uint64_t n, uint64_t p) { return sufr::rep_room(starts, num, n, p); }
int shim_rep_is_start(const uint64_t* starts, uint64_t num, uint64_t n, uint64_t p) { return sufr::rep_is_start(starts, num, n, p) ? 1 : 0; }

}

#ifdef REPEAT_SHIM_MAIN
int main()
{
    uint64_t x = 88172645463325252ull, cases = 0;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    const uint64_t lens[] = {0, 1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 8192, 262143, 262144, 262145, 300000};
    for (const uint64_t s : lens)
        for (int kind = 0; kind < 5; kind++) {
            if (s > 10000 && kind > 2) continue;
            // 0: random small values; 1: one plateau; 2: ascending (every left answer next door, every right answer s);
            // 3: descending; 4: plateaus of 64 and 4096 with dips exactly on the boundaries
            std::vector<uint64_t> ell(s + 1);
            for (uint64_t r = 0; r < s; r++)
                ell[r] = kind == 0 ? rnd() % 7 : kind == 1 ? 5 : kind == 2 ? r : kind == 3 ? s - r : (r % 4096 == 0 ? 1 : r % 64 == 0 ? 2 : 3);
            if (s) ell[0] = 0;
            std::vector<uint64_t> up(shim_rep_pyramid_size(s)), left(s + 1), right(s + 1);
            shim_rep_pyramid(ell.data(), s, up.data());
            shim_rep_search_all(ell.data(), up.data(), s, left.data(), right.data());
            // the linear scan, by a stack (ascending values): nearest j < r with ell[j] <= ell[r]
            std::vector<uint64_t> st;
            for (uint64_t r = 0; r < s; r++) {
                while (!st.empty() && ell[st.back()] > ell[r]) st.pop_back();
                const uint64_t want = st.empty() ? sufr::REP_NONE : st.back();
                if (left[r] != want) { printf("left: s %llu kind %d rank %llu\n", (unsigned long long)s, kind, (unsigned long long)r); return 1; }
                st.push_back(r);
            }
            st.clear();
            for (uint64_t r = s; r > 0; r--) {               // nearest j > r-1 with ell[j] < ell[r-1]
                while (!st.empty() && ell[st.back()] >= ell[r - 1]) st.pop_back();
                const uint64_t want = st.empty() ? s : st.back();
                if (right[r - 1] != want) { printf("right: s %llu kind %d rank %llu\n", (unsigned long long)s, kind, (unsigned long long)(r - 1)); return 1; }
                st.push_back(r - 1);
            }
            cases += 2 * s + 1;
        }
    for (const uint64_t s : {0ull, 1ull, 63ull, 64ull, 65ull, 128ull, 1000ull}) {
        std::vector<uint8_t> flags(s + 1);
        for (uint64_t r = 0; r < s; r++) flags[r] = rnd() % 3 == 0;
        std::vector<uint64_t> words(s / 64 + 1), prefix(s / 64 + 1);
        shim_rep_words(flags.data(), s, words.data(), prefix.data());
        for (uint64_t lo = 0; lo <= s; lo += 1 + (s > 200 ? rnd() % 7 : 0))
            for (uint64_t hi = 0; hi <= s; hi += 1 + (s > 200 ? rnd() % 7 : 0)) {
                uint64_t want = 0;
                for (uint64_t r = lo; r < hi; r++) want += flags[r];
                if (shim_rep_flagged(words.data(), prefix.data(), lo, hi) != want) { printf("flagged: s %llu [%llu, %llu)\n", (unsigned long long)s, (unsigned long long)lo, (unsigned long long)hi); return 1; }
                cases++;
            }
    }
    const uint64_t starts[4] = {0, 5, 6, 20};
    for (uint64_t p = 0; p < 30; p++) {
        const bool want = p == 0 || p == 5 || p == 6 || p == 20;
        if ((shim_rep_is_start(starts, 4, 30, p) != 0) != want || (shim_rep_is_start(nullptr, 0, 30, p) != 0) != (p == 0)) { printf("is_start(%llu)\n", (unsigned long long)p); return 1; }
        if (shim_rep_room(nullptr, 0, 30, p) != 29 - p) return 1;
    }
    if (shim_rep_clip(9, 4, 7) != 4 || shim_rep_clip(3, 4, 7) != 3 || shim_rep_clip(9, 8, 7) != 7) return 1;
    printf("ok %llu\n", (unsigned long long)cases);
    return 0;
}
#endif
