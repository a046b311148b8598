// Host-side shim around the leaf-sort helpers of sufr_amd/csrc/sufr_runkey.h (the digest table of k_leaf_sort and the
// ranking of the members of a counting bucket), so that both can be checked on the CPU.  Test infrastructure.
#include <stdint.h>
#include "../sufr_amd/csrc/sufr_runkey.h"

// A host model of how k_leaf_sort (sufr_msd.inc) puts those helpers together -- NOT the kernel's own loops, which read the LDS:
// the digest from the two table reads, and the rank of member `a` of the bucket keys[0 .. sz), four slots at a time with the
// kernel's sentinel 2^64 - 1 in the slots past the bucket.
static uint32_t model_digest12_tab(const uint16_t* tab, uint32_t t)
{
    return sufr::dna3_digest12_halves(tab[t >> 9], tab[t & 511u]);
}
static uint32_t model_rank_in_bucket(const uint64_t* keys, uint32_t sz, uint32_t a)
{
    uint32_t c = 0;
    for (uint32_t i0 = 0; i0 < sz; i0 += 4u) {
        uint64_t k[4];
        for (uint32_t j = 0; j < 4u; j++) k[j] = i0 + j < sz ? keys[i0 + j] : ~0ull;
        c += sufr::leaf_rank4(k, keys[a], i0, a);
    }
    return c;
}

extern "C" {

// direct[t] = dna3_digest12(t), table[t] = the composition from the table of halves, for all 2^18 six-character strings;
// high6[t] = what a digit of six bits or fewer takes (the first three characters alone), as 12 bits
void shim_leaf_digest_all(uint32_t* direct, uint32_t* table, uint32_t* high6)
{
    uint16_t tab[sufr::DNA3_HALF_ENTRIES];
    for (uint32_t x = 0; x < sufr::DNA3_HALF_ENTRIES; x++) tab[x] = sufr::dna3_half_entry(x);
    for (uint32_t t = 0; t < (1u << 18); t++) {
        direct[t] = sufr::dna3_digest12(t);
        table[t] = model_digest12_tab(tab, t);
        high6[t] = (tab[t >> 9] & 63u) << 6;
    }
}
void shim_leaf_half_table(uint16_t* out)
{
    for (uint32_t x = 0; x < sufr::DNA3_HALF_ENTRIES; x++) out[x] = sufr::dna3_half_entry(x);
}
// rank of every member of the bucket keys[0 .. sz) (arrival order): out[a]
void shim_leaf_ranks(const uint64_t* keys, uint32_t sz, uint32_t* out)
{
    for (uint32_t a = 0; a < sz; a++) out[a] = model_rank_in_bucket(keys, sz, a);
}
uint32_t shim_leaf_mate_before(uint64_t ki, uint64_t key, uint32_t i, uint32_t a) { return sufr::leaf_mate_before(ki, key, i, a); }
// the first-four form with slots past the bucket holding `junk` (the kernel reads them unclamped: keys of later buckets, which
// are larger, or its sentinel)
uint32_t shim_leaf_rank_first4(const uint64_t* keys, uint32_t sz, uint32_t a, uint64_t junk)
{
    uint64_t k[4];
    for (uint32_t i = 0; i < 4u; i++) k[i] = i < sz ? keys[i] : junk;
    return sufr::leaf_rank4(k, keys[a], 0u, a);
}
}
