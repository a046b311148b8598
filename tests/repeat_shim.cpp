// Host-side shim around sufr_amd/csrc/sufr_repeat_scan.h (the min pyramid's index arithmetic, the two nearest-smaller-value
// searches and the popcount-prefix count the repeat kernels run), so that the device's arithmetic can be held to a linear
// scan on the CPU.  With -DREPEAT_SHIM_MAIN it is a stand-alone program that runs the same comparison by itself (built with
// -fsanitize=address,undefined by tests/test_repeat_host.py).  Test infrastructure.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
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
    for (uint32_t k = 1; k <= levels; k++)
        sufr::rep_level_up(k == 1 ? ell : up + sufr::rep_level_offset(s, k - 1), sufr::rep_level_size(s, k - 1), up + sufr::rep_level_offset(s, k),
                           sufr::rep_level_size(s, k));
}
void shim_rep_level_up(const uint64_t* in, uint64_t n_in, uint64_t* out, uint64_t n_out) { sufr::rep_level_up(in, n_in, out, n_out); }

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

// rep_interval of every rank 1 <= r < s: is_rep[r] (0 / 1) and, for a representative, a[r], z[r], v[r]; rank 0 is none
void shim_rep_interval_all(const uint64_t* ell, const uint64_t* up, uint64_t s, uint64_t min_len, uint8_t* is_rep, uint64_t* a, uint64_t* z, uint64_t* v)
{
    const ShimAcc acc{ell, up, s};
    if (s) is_rep[0] = 0;
    for (uint64_t r = 1; r < s; r++) {
        is_rep[r] = 0;
        sufr::rep_interval(acc, s, r, min_len, [&](uint64_t ia, uint64_t iz, uint64_t iv) { is_rep[r] = 1; a[r] = ia; z[r] = iz; v[r] = iv; });
    }
}

// the RepBest of n candidates (5 words each: len, rep, rank, cnt, seq), merged as `parts` runs of take, then a merge of the
// runs from the last to the first; out: 5 words
void shim_rep_best(const uint64_t* cand, uint64_t n, uint64_t parts, uint64_t* out)
{
    if (!parts) parts = 1;
    std::vector<sufr::RepBest> part(parts, sufr::RepBest{0, 0, 0, 0, 0});
    for (uint64_t i = 0; i < n; i++) part[i % parts].take(cand[5 * i], cand[5 * i + 1], cand[5 * i + 2], cand[5 * i + 3], cand[5 * i + 4]);
    sufr::RepBest b{0, 0, 0, 0, 0};
    for (uint64_t k = parts; k > 0; k--) b.merge(part[k - 1]);
    out[0] = b.len; out[1] = b.rep; out[2] = b.rank; out[3] = b.cnt; out[4] = b.seq;
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
            // rep_interval: r is a representative iff the nearest <= on its left is strictly smaller (and ell[r] >= min_len)
            for (const uint64_t min_len : {(uint64_t)1, (uint64_t)3}) {
                std::vector<uint8_t> is_rep(s + 1);
                std::vector<uint64_t> ia(s + 1), iz(s + 1), iv(s + 1);
                shim_rep_interval_all(ell.data(), up.data(), s, min_len, is_rep.data(), ia.data(), iz.data(), iv.data());
                st.clear();
                for (uint64_t r = 0; r < s; r++) {
                    while (!st.empty() && ell[st.back()] > ell[r]) st.pop_back();
                    const bool want = r >= 1 && ell[r] >= min_len && !st.empty() && ell[st.back()] < ell[r];
                    if ((is_rep[r] != 0) != want || (want && (ia[r] != st.back() || iz[r] != right[r] || iv[r] != ell[r]))) {
                        printf("interval: s %llu kind %d min_len %llu rank %llu\n", (unsigned long long)s, kind, (unsigned long long)min_len, (unsigned long long)r);
                        return 1;
                    }
                    st.push_back(r);
                }
                cases += s;
            }
            // rep_level_up: every level of the pyramid is the 64-wise minimum of the one below, entry by entry
            for (uint32_t k = 1; k <= shim_rep_levels(s); k++) {
                const uint64_t* in = k == 1 ? ell.data() : up.data() + sufr::rep_level_offset(s, k - 1);
                const uint64_t n_in = shim_rep_level_size(s, k - 1), n_out = shim_rep_level_size(s, k);
                std::vector<uint64_t> got(n_out + 1, 77);
                shim_rep_level_up(in, n_in, got.data(), n_out);
                for (uint64_t i = 0; i < n_out; i++) {
                    const uint64_t want = *std::min_element(in + i * 64, in + std::min(n_in, i * 64 + 64));
                    if (got[i] != want || up[sufr::rep_level_offset(s, k) + i] != want) { printf("level_up: s %llu level %u entry %llu\n", (unsigned long long)s, k, (unsigned long long)i); return 1; }
                }
                if (got[n_out] != 77) { printf("level_up: wrote past the end\n"); return 1; }
                cases += n_out;
            }
            cases += 2 * s + 1;
        }
    // RepBest: the merge of random candidates, whatever their split into parts, is the first of a sort by (longer, smaller
    // representative) with the maxima of the counts and of the sequence counts; few different lengths, so ties abound
    for (int round = 0; round < 200; round++) {
        const uint64_t n = rnd() % 40;
        std::vector<uint64_t> cand(5 * n + 5);
        for (uint64_t i = 0; i < n; i++) {
            cand[5 * i] = rnd() % 4;
            cand[5 * i + 1] = 1 + i * 7 % 41 + 41 * (rnd() % 2);      // (every representative once)
            cand[5 * i + 2] = 1000 + i;                               // (every rank once: a rank from the wrong candidate shows)
            cand[5 * i + 3] = rnd() % 9; cand[5 * i + 4] = rnd() % 5;
        }
        std::vector<uint64_t> order(n);
        for (uint64_t i = 0; i < n; i++) order[i] = i;
        std::sort(order.begin(), order.end(), [&](uint64_t x, uint64_t y) {
            return cand[5 * x] != cand[5 * y] ? cand[5 * x] > cand[5 * y] : cand[5 * x + 1] < cand[5 * y + 1];
        });
        uint64_t want[5] = {0, 0, 0, 0, 0};
        if (n && cand[5 * order[0]]) { want[0] = cand[5 * order[0]]; want[1] = cand[5 * order[0] + 1]; want[2] = cand[5 * order[0] + 2]; }
        for (uint64_t i = 0; i < n; i++) { want[3] = std::max(want[3], cand[5 * i + 3]); want[4] = std::max(want[4], cand[5 * i + 4]); }
        for (const uint64_t parts : {(uint64_t)1, (uint64_t)3, (uint64_t)64}) {
            uint64_t got[5];
            shim_rep_best(cand.data(), n, parts, got);
            for (int c = 0; c < 5; c++)
                if (got[c] != want[c]) { printf("best: round %d parts %llu column %d\n", round, (unsigned long long)parts, c); return 1; }
            cases++;
        }
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
