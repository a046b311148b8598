// Host-side shim around sufr_amd/csrc/sufr_kmer_scan.h (the summaries, the combine operator, the carries and the per-rank
// count the k-mer kernels run), so that the device's arithmetic can be held to a direct per-interval count on the CPU.
// With -DKMER_SHIM_MAIN it is a stand-alone program that runs the same comparison by itself (built with
// -fsanitize=address,undefined by tests/test_kmer_host.py).  Test infrastructure.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../sufr_amd/csrc/sufr_kmer_scan.h"

extern "C" {

// The count of the interval of every rank of head[0..len) / whole[0..len) (bytes 0 / 1), the way the device gets it: words of
// `tile` ranks (1 .. 64), `group` words to a tile, tiles to the array; summaries folded at every level, carries handed down.
// Ranks before the first head form an interval of their own.  Returns 0, or -1 for a tile outside 1 .. 64 or group 0.
int shim_kmer_counts(const uint8_t* head, const uint8_t* whole, uint64_t len, uint32_t tile, uint32_t group, uint64_t* out)
{
    if (tile < 1 || tile > 64 || group < 1) return -1;
    const uint64_t nwords = (len + tile - 1) / tile, ngroups = (nwords + group - 1) / group;
    std::vector<uint64_t> H(nwords, 0), W(nwords, 0);
    for (uint64_t r = 0; r < len; r++) {
        if (head[r]) H[r / tile] |= (uint64_t)1 << (r % tile);
        if (whole[r]) W[r / tile] |= (uint64_t)1 << (r % tile);
    }
    // fold: words to group summaries
    std::vector<sufr::KmerSum> gs(ngroups, sufr::kmer_identity());
    for (uint64_t j = 0; j < nwords; j++) gs[j / group] = sufr::kmer_combine(gs[j / group], sufr::kmer_word_sum(H[j], W[j]));
    // carry: across the groups, both ways
    std::vector<uint64_t> gin(ngroups), gout(ngroups);
    sufr::KmerSum run = sufr::kmer_identity();
    for (uint64_t g = 0; g < ngroups; g++) { gin[g] = sufr::kmer_carry_in(run, 0); run = sufr::kmer_combine(run, gs[g]); }
    run = sufr::kmer_identity();
    for (uint64_t g = ngroups; g > 0; g--) { gout[g - 1] = sufr::kmer_carry_out(run, 0); run = sufr::kmer_combine(gs[g - 1], run); }
    // apply: the words of a group get their carries from the words before and after them in the group
    for (uint64_t g = 0; g < ngroups; g++) {
        const uint64_t j0 = g * group, j1 = j0 + group < nwords ? j0 + group : nwords;
        for (uint64_t j = j0; j < j1; j++) {
            sufr::KmerSum before = sufr::kmer_identity(), after = sufr::kmer_identity();
            for (uint64_t i = j0; i < j; i++) before = sufr::kmer_combine(before, sufr::kmer_word_sum(H[i], W[i]));
            for (uint64_t i = j1; i > j + 1; i--) after = sufr::kmer_combine(sufr::kmer_word_sum(H[i - 1], W[i - 1]), after);
            const uint64_t ci = sufr::kmer_carry_in(before, gin[g]), co = sufr::kmer_carry_out(after, gout[g]);
            for (uint64_t r = j * tile; r < (j + 1) * tile && r < len; r++) out[r] = sufr::kmer_rank_count(H[j], W[j], (uint32_t)(r % tile), ci, co);
        }
    }
    return 0;
}

uint64_t shim_kmer_brk(const uint64_t* starts, uint64_t num, uint64_t n, uint64_t p) { return sufr::kmer_brk(starts, num, n, p); }
int shim_kmer_whole(const uint64_t* starts, uint64_t num, uint64_t n, uint64_t p, uint64_t k) { return sufr::kmer_whole(starts, num, n, p, k) ? 1 : 0; }
uint64_t shim_kmer_bin(uint64_t c, uint64_t bins) { return sufr::kmer_bin(c, bins); }

}

#ifdef KMER_SHIM_MAIN
namespace {
void direct(const std::vector<uint8_t>& head, const std::vector<uint8_t>& whole, std::vector<uint64_t>& out)
{
    const size_t len = head.size();
    for (size_t a = 0; a < len;) {
        size_t z = a + 1;
        while (z < len && !head[z]) z++;
        uint64_t c = 0;
        for (size_t r = a; r < z; r++) c += whole[r];
        for (size_t r = a; r < z; r++) out[r] = c;
        a = z;
    }
}
}

int main()
{
    uint64_t x = 88172645463325252ull, cases = 0;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (size_t len = 0; len <= 40; len++)
        for (int kind = 0; kind < 8; kind++) {
            std::vector<uint8_t> head(len), whole(len);
            for (size_t r = 0; r < len; r++) {
                head[r] = kind == 0 ? 1 : kind == 1 ? 0 : kind == 2 ? r == len / 2 : kind == 3 ? r == 0 : (rnd() % (kind - 2)) == 0;
                whole[r] = kind < 4 ? (r % 3 != 1) : (rnd() % 4) != 0;
            }
            std::vector<uint64_t> want(len + 1), got(len + 1);
            direct(head, whole, want);
            for (uint32_t tile = 1; tile <= 9; tile++)
                for (uint32_t group : {1u, 2u, 3u, 64u}) {
                    if (shim_kmer_counts(head.data(), whole.data(), len, tile, group, got.data()) != 0) return 2;
                    for (size_t r = 0; r < len; r++)
                        if (got[r] != want[r]) { printf("mismatch len %zu kind %d tile %u group %u rank %zu\n", len, kind, tile, group, r); return 1; }
                    cases++;
                }
        }
    // whole 64-rank words, as the kernels use them
    for (int rep = 0; rep < 200; rep++) {
        const size_t len = 1 + rnd() % 700;
        std::vector<uint8_t> head(len), whole(len);
        const unsigned hd = 1 + rnd() % 90;
        for (size_t r = 0; r < len; r++) { head[r] = rnd() % hd == 0; whole[r] = rnd() % 5 != 0; }
        std::vector<uint64_t> want(len), got(len);
        direct(head, whole, want);
        if (shim_kmer_counts(head.data(), whole.data(), len, 64, 1 + rep % 5, got.data()) != 0) return 2;
        for (size_t r = 0; r < len; r++) if (got[r] != want[r]) { printf("mismatch at 64: len %zu rank %zu\n", len, r); return 1; }
        cases++;
    }
    const uint64_t starts[4] = {0, 5, 6, 20};
    for (uint64_t p = 0; p < 30; p++) {
        uint64_t want = 29;
        for (uint64_t b : {4ull, 5ull, 19ull}) if (b >= p && b < want) want = b;
        if (shim_kmer_brk(starts, 4, 30, p) != want || shim_kmer_brk(starts, 1, 30, p) != 29 || shim_kmer_brk(nullptr, 0, 30, p) != 29) { printf("brk(%llu)\n", (unsigned long long)p); return 1; }
        if (shim_kmer_whole(starts, 4, 30, p, ~(uint64_t)0)) return 1;
    }
    printf("ok %llu\n", (unsigned long long)cases);
    return 0;
}
#endif
