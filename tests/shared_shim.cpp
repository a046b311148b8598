// Host-side shim around sufr_amd/csrc/sufr_shared_scan.h (the sequence of a position, the sort key, the decision of one pair
// over the min pyramid of the clipped LCP, and the sequence count of an interval from the prefix sums, as the kernels of
// sufr_shared.inc run them), so that the device's arithmetic can be held to linear scans and to a set count on the CPU.  With
// -DSHARED_SHIM_MAIN it is a stand-alone program that runs the same comparison by itself (built with
// -fsanitize=address,undefined by tests/test_shared_host.py).  Test infrastructure.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <set>
#include <vector>
#include "../sufr_amd/csrc/sufr_shared_scan.h"

namespace {
struct ShimAcc {
    const uint64_t *a, *up;
    mutable uint64_t reads;
    uint64_t at(uint32_t level, uint64_t off, uint64_t i) const { reads++; return level ? up[off + i] : a[i]; }
};
}

extern "C" {

// entries of the array of the coarser levels (at least 1, so that a caller can always allocate)
uint64_t shim_shr_pyramid_size(uint64_t s) { return sufr::rep_level_offset(s, sufr::rep_levels(s) + 1) + 1; }
uint32_t shim_shr_levels(uint64_t s) { return sufr::rep_levels(s); }

// the coarser levels of ell[0..s) into up (shim_shr_pyramid_size(s) entries)
void shim_shr_pyramid(const uint64_t* ell, uint64_t s, uint64_t* up)
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

uint64_t shim_shr_doc(const uint64_t* starts, uint64_t num, uint64_t p) { return sufr::shr_doc(starts, num, p); }
uint64_t shim_shr_key(uint64_t doc, uint64_t r) { return sufr::shr_key(doc, r); }
uint64_t shim_shr_key_doc(uint64_t key) { return sufr::shr_key_doc(key); }
uint64_t shim_shr_key_rank(uint64_t key) { return sufr::shr_key_rank(key); }
uint32_t shim_shr_doc_bits(uint64_t num) { return sufr::shr_doc_bits(num); }

// q of the pair (prev, r); *reads (may be null) receives the larger number of entries one of its two primitives read
uint64_t shim_shr_pair(const uint64_t* ell, const uint64_t* up, uint64_t s, uint64_t prev, uint64_t r, uint64_t* reads)
{
    const ShimAcc a{ell, up, 0}, b{ell, up, 0};
    const uint64_t m = sufr::lz_range_min(a, s, prev + 1, r + 1);
    (void)sufr::rep_search_right(b, s, prev, m + 1);
    if (reads) *reads = a.reads > b.reads ? a.reads : b.reads;
    const ShimAcc c{ell, up, 0};
    return sufr::shr_pair(c, s, prev, r);
}

// D[0..s): the sequence of every rank (below num).  prev (s entries, all ones: none), qs (s entries, all ones: no pair),
// H and P (s + 1 entries each) as the host and device paths build them.  Returns the largest number of reads of a primitive.
uint64_t shim_shr_prefix(const uint64_t* ell, const uint64_t* up, uint64_t s, const uint64_t* D, uint64_t num, uint64_t* prev, uint64_t* qs,
                         uint64_t* H, uint64_t* P)
{
    std::vector<uint64_t> last(num ? num : 1, ~(uint64_t)0);
    uint64_t most = 0;
    for (uint64_t j = 0; j <= s; j++) H[j] = 0;
    for (uint64_t r = 0; r < s; r++) {
        prev[r] = last[D[r]];
        last[D[r]] = r;
        qs[r] = ~(uint64_t)0;
        if (prev[r] == ~(uint64_t)0) continue;
        uint64_t reads = 0;
        qs[r] = shim_shr_pair(ell, up, s, prev[r], r, &reads);
        if (reads > most) most = reads;
        H[qs[r]]++;
    }
    uint64_t run = 0;
    for (uint64_t j = 0; j <= s; j++) { P[j] = run; run += H[j]; }
    return most;
}

uint64_t shim_shr_seqs(const uint64_t* P, uint64_t a, uint64_t b) { return sufr::shr_seqs(P, a, b); }
int shim_shr_keep(uint64_t seqs, uint64_t min_seqs, uint64_t max_seqs) { return sufr::shr_keep(seqs, min_seqs, max_seqs) ? 1 : 0; }

}

#ifdef SHARED_SHIM_MAIN
int main()
{
    uint64_t x = 88172645463325252ull, cases = 0;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    const uint64_t lens[] = {1, 2, 3, 63, 64, 65, 127, 128, 129, 700, 4095, 4096, 4097, 9000};
    for (const uint64_t s : lens)
        for (int kind = 0; kind < 5; kind++)
            for (const uint64_t num : {(uint64_t)1, (uint64_t)2, (uint64_t)5, (uint64_t)300}) {
                // l: 0 random small, 1 constant, 2 ascending, 3 descending, 4 dips on the block boundaries
                std::vector<uint64_t> ell(s), D(s);
                for (uint64_t r = 0; r < s; r++) {
                    ell[r] = kind == 0 ? rnd() % 6 : kind == 1 ? 4 : kind == 2 ? r : kind == 3 ? s - r : (r % 64 == 0 ? 1 : 3);
                    D[r] = rnd() % num;
                }
                ell[0] = 0;
                std::vector<uint64_t> up(shim_shr_pyramid_size(s)), prev(s), qs(s), H(s + 1), P(s + 1);
                shim_shr_pyramid(ell.data(), s, up.data());
                const uint64_t bound = 2 * 64 * ((uint64_t)sufr::rep_levels(s) + 1);
                if (shim_shr_prefix(ell.data(), up.data(), s, D.data(), num, prev.data(), qs.data(), H.data(), P.data()) > bound) { printf("reads: s %llu\n", (unsigned long long)s); return 1; }
                for (uint64_t r = 0; r < s; r++) {          // prev and q against linear scans
                    uint64_t p = ~(uint64_t)0;
                    for (uint64_t j = r; j > 0; j--) if (D[j - 1] == D[r]) { p = j - 1; break; }
                    if (p != prev[r]) { printf("prev: s %llu rank %llu\n", (unsigned long long)s, (unsigned long long)r); return 1; }
                    if (p == ~(uint64_t)0) continue;
                    uint64_t q = p + 1;
                    for (uint64_t j = p + 1; j <= r; j++) if (ell[j] < ell[q]) q = j;
                    if (q != qs[r]) { printf("pair: s %llu kind %d (%llu, %llu)\n", (unsigned long long)s, kind, (unsigned long long)p, (unsigned long long)r); return 1; }
                    cases++;
                }
                if (s > 2000 && kind != 0) continue;        // (the set count below is quadratic in the interval length)
                for (uint64_t r = 1; r < s; r++) {          // every interval, from every rank of it
                    const uint64_t v = ell[r];
                    if (!v) continue;
                    uint64_t a = r, b = r + 1;
                    while (ell[a] >= v) a--;                 // (l[0] = 0 ends it)
                    while (b < s && ell[b] >= v) b++;
                    if (b - a > 600) continue;
                    std::set<uint64_t> docs(D.begin() + a, D.begin() + b);
                    if (shim_shr_seqs(P.data(), a, b) != docs.size()) { printf("seqs: s %llu kind %d [%llu, %llu)\n", (unsigned long long)s, kind, (unsigned long long)a, (unsigned long long)b); return 1; }
                    cases++;
                }
            }
    const uint64_t starts[] = {0, 5, 6, 40};
    const uint64_t want[] = {0, 0, 1, 2, 2, 3, 3};
    const uint64_t at[] = {0, 4, 5, 6, 39, 40, 1000};
    for (int i = 0; i < 7; i++) if (shim_shr_doc(starts, 4, at[i]) != want[i]) return 1;
    if (shim_shr_doc(starts, 1, 77) != 0 || shim_shr_doc(nullptr, 0, 77) != 0) return 1;
    if (shim_shr_doc_bits(0) != 0 || shim_shr_doc_bits(1) != 0 || shim_shr_doc_bits(2) != 1 || shim_shr_doc_bits(256) != 8 || shim_shr_doc_bits(257) != 9) return 1;
    const uint64_t key = shim_shr_key(0xFFFFFF, ((uint64_t)1 << 40) - 1);
    if (shim_shr_key_doc(key) != 0xFFFFFF || shim_shr_key_rank(key) != ((uint64_t)1 << 40) - 1) return 1;
    printf("ok %llu\n", (unsigned long long)cases);
    return 0;
}
#endif
