// sufr_query.cpp -- the .sufr reader and the search of include/sufr_query.h (host C++, no device code).
//
// Replaces, for the query side of the reference: SufrFile::read (libsufr/src/sufr_file.rs:145-275),
// SufrSearch::search / suffix_search_first / suffix_search_last / compare (sufr_search.rs:104-350) and
// find_lcp_full_offset (util.rs:19-37).  The file is mapped, not read: text, SA and LCP are views into the mapping.
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/sufr_hip.h"
#include "../../include/sufr_query.h"
#include "../../include/sufr_match.h"
#include "../../include/sufr_mem.h"
#include "../../include/sufr_approx.h"
#include "../../include/sufr_edit.h"
#include "../../include/sufr_align.h"

struct sufr_file {
    std::string path;
    const uint8_t* map = nullptr;
    size_t map_len = 0;
    sufr_file_meta meta{};
    const uint8_t* text = nullptr;
    const uint8_t* sa = nullptr;
    const uint8_t* lcp = nullptr;
    const uint8_t* mask = nullptr;            // seed_mask_len bytes of 0 / 1
    std::vector<uint64_t> seq_starts;
    std::vector<std::string> seq_names;
    std::vector<uint64_t> mask_positions;     // offsets of the 1s: the "care" positions (types.rs:36-200)
    mutable std::once_flag indexed_once;      // MEMs: bit p of `indexed` = position p starts an indexed suffix, built on
    mutable std::vector<uint64_t> indexed;    // first use when the array leaves positions out (sufr_mem.h)
};

namespace {

void put_err(char* err, size_t errlen, const std::string& s)
{
    if (err && errlen) snprintf(err, errlen, "%s", s.c_str());
}

uint64_t rd64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }
uint64_t rdT(const uint8_t* p, int width, uint64_t i)
{
    if (width == 4) { uint32_t v; memcpy(&v, p + i * 4, 4); return v; }
    uint64_t v; memcpy(&v, p + i * 8, 8); return v;
}

struct Comparison { uint64_t lcp; int cmp; };          // cmp: -1 query < suffix, 0 equal, +1 query > suffix

// find_lcp_full_offset (util.rs:19-37): the text offset that follows `lcp` matched care positions
uint64_t full_offset(const sufr_file& f, uint64_t lcp)
{
    if (f.mask_positions.empty()) return lcp;
    if (lcp == 0 || lcp > f.meta.seed_mask_len) return lcp;
    // (lcp <= weight wherever compare() calls this: lcp counts care positions)
    const uint64_t offset = f.mask_positions[lcp - 1];
    const uint64_t next = lcp < f.mask_positions.size() ? f.mask_positions[lcp] : 0;
    return (next > offset && next - offset > 1) ? next : offset + 1;
}

// SufrSearch::compare (sufr_search.rs:241-343)
Comparison compare(const sufr_file& f, const uint8_t* q, size_t qlen, bool has_rt, uint64_t rt_mql, uint64_t suffix_pos,
                   uint64_t skip)
{
    const uint64_t n = f.meta.text_len;
    uint64_t lcp, max_query_len;
    if (f.mask_positions.empty()) {
        const uint64_t built = f.meta.max_query_len;
        max_query_len = (built > 0 && has_rt) ? (built < rt_mql ? built : rt_mql) : (has_rt ? rt_mql : built);
        if (max_query_len > 0 && skip >= max_query_len) lcp = skip;
        else {
            const uint64_t text_start = suffix_pos + skip;
            uint64_t text_end = max_query_len > 0 ? text_start + max_query_len : text_start + qlen;
            if (text_end > n) text_end = n;
            uint64_t k = 0;
            while (skip + k < qlen && text_start + k < text_end && q[skip + k] == f.text[text_start + k]) k++;
            lcp = skip + k;
        }
    } else {
        const uint64_t weight = f.mask_positions.size();
        max_query_len = has_rt ? rt_mql : 0;
        if (skip >= weight || (max_query_len > 0 && skip >= max_query_len)) lcp = skip;
        else {
            const uint64_t end = max_query_len > 0 ? (max_query_len < weight ? max_query_len : weight) : weight;
            uint64_t query_len = 0, suffix_len = 0;
            for (uint64_t i = skip; i < end; i++) {
                if (f.mask_positions[i] < qlen) query_len++;
                if (suffix_pos + f.mask_positions[i] < n) suffix_len++;
            }
            const uint64_t len = query_len < suffix_len ? query_len : suffix_len;
            uint64_t k = 0;
            while (k < len) {
                const uint64_t off = f.mask_positions[skip + k];
                if (suffix_pos + off >= n || q[off] != f.text[suffix_pos + off]) break;
                k++;
            }
            lcp = skip + k;
        }
    }
    int cmp;
    if (max_query_len > 0 && lcp >= max_query_len) cmp = 0;          // seen enough
    else {
        const uint64_t fo = full_offset(f, lcp);
        if (fo >= qlen) cmp = 0;                                      // the entire query matched
        else if (suffix_pos + fo >= n) cmp = 1;                       // (the reference has `unreachable!()` here)
        else cmp = q[fo] < f.text[suffix_pos + fo] ? -1 : (q[fo] > f.text[suffix_pos + fo] ? 1 : 0);
    }
    return {lcp, cmp};
}

// runs body(b, e) over [0, total) in chunks of `chunk`, `threads` workers (0: one per core), at most one per `least` items
// (0: one per chunk)
template <typename F>
void parallel_chunks(uint64_t total, uint64_t chunk, int threads, F body, uint64_t least = 0)
{
    if (least == 0) least = chunk;
    unsigned T = threads > 0 ? (unsigned)threads : std::thread::hardware_concurrency();
    if (T == 0) T = 1;
    if (T > total / least + 1) T = (unsigned)(total / least + 1);
    std::atomic<uint64_t> next{0};
    auto worker = [&]() {
        for (;;) {
            const uint64_t b = next.fetch_add(chunk);
            if (b >= total) return;
            body(b, b + chunk < total ? b + chunk : total);
        }
    };
    if (T == 1) { worker(); return; }
    std::vector<std::thread> th;
    for (unsigned t = 0; t < T; t++) th.emplace_back(worker);
    for (auto& t : th) t.join();
}

}  // namespace

extern "C" {

int sufr_file_open(const char* path, sufr_file** out, char* err, size_t errlen)
{
    if (!path || !out) return SUFR_HIP_E_INVALID;
    *out = nullptr;
    int fd = ::open(path, O_RDONLY);
    if (fd < 0) { put_err(err, errlen, std::string(path) + ": " + strerror(errno)); return SUFR_HIP_E_IO; }
    struct stat sb;
    if (fstat(fd, &sb) != 0 || sb.st_size < 68) {
        put_err(err, errlen, std::string(path) + ": not a .sufr file (too short)");
        ::close(fd);
        return SUFR_HIP_E_IO;
    }
    void* m = mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    ::close(fd);
    if (m == MAP_FAILED) { put_err(err, errlen, std::string(path) + ": mmap: " + strerror(errno)); return SUFR_HIP_E_IO; }
    sufr_file* f = new sufr_file;
    f->path = path; f->map = (const uint8_t*)m; f->map_len = (size_t)sb.st_size;
    auto fail = [&](const std::string& why) {
        put_err(err, errlen, std::string(path) + ": " + why);
        sufr_file_close(f);
        return SUFR_HIP_E_IO;
    };
    const uint8_t* p = f->map;
    sufr_file_meta& M = f->meta;
    M.version = p[0]; M.is_dna = p[1] == 1; M.allow_ambiguity = p[2] == 1; M.ignore_softmask = p[3] == 1;
    M.text_len = rd64(p + 4); M.text_pos = rd64(p + 12); M.suffix_array_pos = rd64(p + 20); M.lcp_pos = rd64(p + 28);
    M.len_suffixes = rd64(p + 36); M.max_query_len = rd64(p + 44); M.num_sequences = rd64(p + 52);
    M.index_width = M.text_len < 0xFFFFFFFFull ? 4 : 8;                // suffix_array.rs: u32 iff text_len < u32::MAX
    M.file_size = (uint64_t)sb.st_size; M.modified = (int64_t)sb.st_mtime;
    if (M.version != 6) return fail("unsupported .sufr version " + std::to_string(M.version) + " (this reader takes version 6)");
    const uint64_t W = (uint64_t)M.index_width;
    uint64_t at = 60;
    if (M.num_sequences > (f->map_len - at) / W) return fail("corrupt header (sequence starts)");
    f->seq_starts.resize(M.num_sequences);
    for (uint64_t i = 0; i < M.num_sequences; i++) f->seq_starts[i] = rdT(p + at, M.index_width, i);
    at += M.num_sequences * W;
    if (at + 8 > f->map_len) return fail("corrupt header (seed mask)");
    M.seed_mask_len = rd64(p + at); at += 8;
    if (M.seed_mask_len > f->map_len - at) return fail("corrupt header (seed mask)");
    if (M.seed_mask_len) {
        f->mask = p + at;
        for (uint64_t i = 0; i < M.seed_mask_len; i++) if (f->mask[i] == 1) f->mask_positions.push_back(i);
        at += M.seed_mask_len;
    }
    const uint64_t L = f->map_len;                                      // every bound without an overflowing product
    if (M.text_pos != at || M.text_len > L - at || M.len_suffixes > L / W || M.suffix_array_pos > L ||
        M.len_suffixes * W > L - M.suffix_array_pos || M.lcp_pos > L || M.len_suffixes * W > L - M.lcp_pos)
        return fail("corrupt header (section offsets)");
    f->text = p + M.text_pos; f->sa = p + M.suffix_array_pos; f->lcp = p + M.lcp_pos;
    // sequence names: bincode 1.x Vec<String> after the LCP section (u64 count, then u64 length + bytes each)
    uint64_t q = M.lcp_pos + M.len_suffixes * W;
    if (q + 8 > f->map_len) return fail("corrupt file (sequence names)");
    const uint64_t cnt = rd64(p + q); q += 8;
    for (uint64_t i = 0; i < cnt; i++) {
        if (q + 8 > f->map_len) return fail("corrupt file (sequence names)");
        const uint64_t len = rd64(p + q); q += 8;
        if (len > f->map_len - q) return fail("corrupt file (sequence names)");
        f->seq_names.emplace_back((const char*)p + q, (size_t)len);
        q += len;
    }
    if (f->seq_names.size() != M.num_sequences) return fail("corrupt file (sequence names do not match the header)");
    *out = f;
    return 0;
}

void sufr_file_close(sufr_file* f)
{
    if (!f) return;
    if (f->map) munmap((void*)f->map, f->map_len);
    delete f;
}

int sufr_file_metadata(const sufr_file* f, sufr_file_meta* meta)
{
    if (!f || !meta) return SUFR_HIP_E_INVALID;
    *meta = f->meta;
    return 0;
}

const uint8_t* sufr_file_text(const sufr_file* f) { return f ? f->text : nullptr; }
const uint8_t* sufr_file_seed_mask(const sufr_file* f) { return f ? f->mask : nullptr; }
const void* sufr_file_suffix_array(const sufr_file* f) { return f ? f->sa : nullptr; }
const void* sufr_file_lcp_array(const sufr_file* f) { return f ? f->lcp : nullptr; }
uint64_t sufr_file_suffix(const sufr_file* f, uint64_t rank) { return rdT(f->sa, f->meta.index_width, rank); }
uint64_t sufr_file_lcp(const sufr_file* f, uint64_t rank) { return rdT(f->lcp, f->meta.index_width, rank); }
uint64_t sufr_file_sequence_start(const sufr_file* f, uint64_t i) { return f->seq_starts[i]; }
const char* sufr_file_sequence_name(const sufr_file* f, uint64_t i) { return f->seq_names[i].c_str(); }

uint64_t sufr_file_sequence_of(const sufr_file* f, uint64_t pos)
{
    uint64_t lo = 0, hi = f->seq_starts.size();            // partition_point(|v| v <= pos)
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (f->seq_starts[mid] <= pos) lo = mid + 1; else hi = mid;
    }
    return lo ? lo - 1 : 0;
}

int sufr_file_search(const sufr_file* f, const uint8_t* q, size_t qlen, int has_mql, uint64_t mql, uint64_t* rank_lo,
                     uint64_t* rank_hi)
{
    if (!f || (!q && qlen) || !rank_lo || !rank_hi) return 0;
    const uint64_t n = f->meta.len_suffixes;
    if (n == 0) return 0;
    const bool rt = has_mql != 0;
    // suffix_search_first (sufr_search.rs:171-203), iteratively
    uint64_t first = 0;
    bool found = false;
    {
        uint64_t low = 0, high = n - 1, left = 0, right = 0;
        for (;;) {
            if (high < low) break;
            const uint64_t mid = low + (high - low) / 2;
            const uint64_t mv = sufr_file_suffix(f, mid);
            const Comparison c = compare(*f, q, qlen, rt, mql, mv, left < right ? left : right);
            if (c.cmp == 0 && (mid == 0 || compare(*f, q, qlen, rt, mql, sufr_file_suffix(f, mid - 1), 0).cmp > 0)) {
                first = mid; found = true; break;
            }
            if (c.cmp > 0) { low = mid + 1; left = c.lcp; }
            else { if (mid == 0) break; high = mid - 1; right = c.lcp; }
        }
    }
    if (!found) return 0;
    // suffix_search_last (206-238)
    uint64_t last = first;
    {
        uint64_t low = first, high = n - 1, left = 0, right = 0;
        for (;;) {
            if (high < low) break;
            const uint64_t mid = low + (high - low) / 2;
            const uint64_t mv = sufr_file_suffix(f, mid);
            const Comparison c = compare(*f, q, qlen, rt, mql, mv, left < right ? left : right);
            if (c.cmp == 0 && (mid == n - 1 || compare(*f, q, qlen, rt, mql, sufr_file_suffix(f, mid + 1), 0).cmp < 0)) {
                last = mid; break;
            }
            if (c.cmp < 0) { if (mid == 0) break; high = mid - 1; right = c.lcp; }
            else { low = mid + 1; left = c.lcp; }
        }
    }
    *rank_lo = first; *rank_hi = last + 1;
    return 1;
}

int sufr_file_search_batch(const sufr_file* f, const uint8_t* queries, const uint64_t* offsets, uint64_t nq, int has_mql,
                           uint64_t mql, uint64_t* rank_lo, uint64_t* rank_hi, int threads)
{
    if (!f || (nq && (!offsets || !rank_lo || !rank_hi))) return SUFR_HIP_E_INVALID;
    parallel_chunks(nq, 256, threads, [&](uint64_t b, uint64_t e) {
        for (uint64_t i = b; i < e; i++) {
            uint64_t lo = 0, hi = 0;
            const int hit = sufr_file_search(f, queries + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), has_mql, mql, &lo, &hi);
            rank_lo[i] = hit ? lo : 0; rank_hi[i] = hit ? hi : 0;
        }
    }, 64);                                                    // a worker is not worth fewer than 64 queries
    return 0;
}

}  // extern "C"

// ---- matching statistics and SMEMs (include/sufr_match.h) -------------------------------------
namespace {

// ms of one query offset: the lower bound of q[0..qlen) under compare(), then the longer of the prefixes it shares with
// the suffixes at the insertion point and just below it (the sorted order puts the longest shared prefix next to it).
// compare() caps at the build's max_query_len, so a capped file gives min(lcp, L).
uint32_t host_ms(const sufr_file& f, const uint8_t* q, size_t qlen)
{
    const uint64_t n = f.meta.len_suffixes;
    if (n == 0 || qlen == 0) return 0;
    uint64_t lo = 0, hi = n, l = 0, r = 0;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        const Comparison c = compare(f, q, qlen, false, 0, sufr_file_suffix(&f, mid), l < r ? l : r);
        if (c.cmp > 0) { lo = mid + 1; l = c.lcp; }
        else { hi = mid; r = c.lcp; }
    }
    uint64_t best = 0;
    if (lo > 0) best = compare(f, q, qlen, false, 0, sufr_file_suffix(&f, lo - 1), 0).lcp;
    if (lo < n) { const uint64_t v = compare(f, q, qlen, false, 0, sufr_file_suffix(&f, lo), 0).lcp; if (v > best) best = v; }
    return (uint32_t)best;
}

// the query that holds byte g of the batch: the last i < nq with offsets[i] <= g
uint64_t query_of(const uint64_t* offsets, uint64_t nq, uint64_t g)
{
    uint64_t a = 0, b = nq;
    while (b - a > 1) { const uint64_t m = a + (b - a) / 2; if (offsets[m] <= g) a = m; else b = m; }
    return a;
}

int match_args(const sufr_file* f, const uint8_t* queries, const uint64_t* offsets, uint64_t nq)
{
    if (!f || (nq && !offsets) || (nq && offsets[nq] > offsets[0] && !queries)) return SUFR_HIP_E_INVALID;
    for (uint64_t i = 0; i < nq; i++) if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > 0xFFFFFFFFull) return SUFR_HIP_E_INVALID;
    if (f->meta.seed_mask_len) return SUFR_HIP_E_UNSUPPORTED;
    return 0;
}

// ms of every byte of the batch: ms[g - base] for g in [offsets[0], offsets[nq])
void host_ms_batch(const sufr_file& f, const uint8_t* queries, const uint64_t* offsets, uint64_t nq, int threads, uint32_t* ms,
                   uint64_t base)
{
    const uint64_t g0 = offsets[0];
    parallel_chunks(offsets[nq] - g0, 4096, threads, [&](uint64_t b, uint64_t e) {
        uint64_t a = query_of(offsets, nq, g0 + b);
        for (uint64_t g = g0 + b; g < g0 + e; g++) {
            while (offsets[a + 1] <= g) a++;
            ms[g - base] = host_ms(f, queries + g, (size_t)(offsets[a + 1] - g));
        }
    });
}

// The SMEM rule over the statistics ms[g - g0] of a batch, in (query, offset) order: the records are counted, then written.
// total: their number, also where it exceeds cap (SUFR_HIP_E_CAPACITY, nothing written)
int smem_records(const uint32_t* ms, uint64_t g0, const uint64_t* offsets, uint64_t nq, uint32_t min_len, uint64_t cap, uint64_t* query,
                 uint32_t* qoff, uint32_t* len, const uint64_t* rank_lo, const uint64_t* rank_hi, uint64_t& total, uint64_t* total_out)
{
    auto each_smem = [&](auto emit) {
        for (uint64_t i = 0; i < nq; i++)
            for (uint64_t g = offsets[i]; g < offsets[i + 1]; g++) {
                const uint32_t v = ms[g - g0];
                if (v >= min_len && (g == offsets[i] || ms[g - g0 - 1] <= v)) emit(i, g, v);
            }
    };
    total = 0;
    each_smem([&](uint64_t, uint64_t, uint32_t) { total++; });
    if (total_out) *total_out = total;
    if (total > cap) return SUFR_HIP_E_CAPACITY;
    if (!total) return 0;
    if (!query || !qoff || !len || !rank_lo || !rank_hi) return SUFR_HIP_E_INVALID;
    uint64_t t = 0;
    each_smem([&](uint64_t i, uint64_t g, uint32_t v) { query[t] = i; qoff[t] = (uint32_t)(g - offsets[i]); len[t] = v; t++; });
    return 0;
}

}  // namespace

extern "C" {

int sufr_file_matching_stats(const sufr_file* f, const uint8_t* queries, const uint64_t* offsets, uint64_t nq, uint32_t* ms,
                             int threads)
{
    if (const int rc = match_args(f, queries, offsets, nq)) return rc;
    if (!nq || offsets[nq] == offsets[0]) return 0;
    if (!ms) return SUFR_HIP_E_INVALID;
    host_ms_batch(*f, queries, offsets, nq, threads, ms, 0);
    return 0;
}

int sufr_file_smems(const sufr_file* f, const uint8_t* queries, const uint64_t* offsets, uint64_t nq, uint32_t min_len,
                    uint64_t cap, uint64_t* query, uint32_t* qoff, uint32_t* len, uint64_t* rank_lo, uint64_t* rank_hi,
                    uint64_t* total_out, int threads)
{
    if (total_out) *total_out = 0;
    if (const int rc = match_args(f, queries, offsets, nq)) return rc;
    if (min_len == 0) return SUFR_HIP_E_INVALID;
    if (!nq || offsets[nq] == offsets[0]) return 0;
    const uint64_t g0 = offsets[0];
    std::vector<uint32_t> ms(offsets[nq] - g0);
    host_ms_batch(*f, queries, offsets, nq, threads, ms.data(), g0);
    uint64_t total = 0;
    if (const int rc = smem_records(ms.data(), g0, offsets, nq, min_len, cap, query, qoff, len, rank_lo, rank_hi, total, total_out)) return rc;
    if (!total) return 0;
    // the rank range of every SMEM: a plain search of its slice (it occurs: ms >= min_len >= 1)
    parallel_chunks(total, 256, threads, [&](uint64_t b, uint64_t e) {
        for (uint64_t k = b; k < e; k++) {
            uint64_t lo = 0, hi = 0;
            const int hit = sufr_file_search(f, queries + offsets[query[k]] + qoff[k], len[k], 0, 0, &lo, &hi);
            rank_lo[k] = hit ? lo : 0; rank_hi[k] = hit ? hi : 0;
        }
    });
    return 0;
}

}  // extern "C"

// ---- maximal exact matches (include/sufr_mem.h) -----------------------------------------------
namespace {

struct MemRec { uint64_t query; uint32_t qoff; uint8_t strand; uint32_t len; uint64_t pos; };

// the indexed positions as a bitmap, once per open file; empty when every position is indexed
const std::vector<uint64_t>& indexed_bits(const sufr_file& f)
{
    std::call_once(f.indexed_once, [&f]() {
        const uint64_t n = f.meta.text_len, s = f.meta.len_suffixes;
        if (s == n) return;
        f.indexed.assign((n + 63) / 64, 0);
        for (uint64_t r = 0; r < s; r++) { const uint64_t p = sufr_file_suffix(&f, r); f.indexed[p >> 6] |= 1ull << (p & 63); }
    });
    return f.indexed;
}

uint8_t revcomp_byte(uint8_t c)
{
    switch (c) { case 'A': return 'T'; case 'T': return 'A'; case 'C': return 'G'; case 'G': return 'C'; default: return c; }
}

// the batch in record order, offsets from 0: query i, then (both strands) its reverse complement as query 2i + 1, in `dbl`;
// one strand: the caller's bytes in place.  Returns the first byte of query 0.
const uint8_t* strand_batch(const uint8_t* queries, const uint64_t* offsets, uint64_t nq, bool both, std::vector<uint8_t>& dbl,
                            std::vector<uint64_t>& off)
{
    const uint64_t g0 = offsets[0], nb = offsets[nq] - g0;
    const uint8_t* qb = queries + g0;
    if (!both) {
        off.resize(nq + 1);
        for (uint64_t i = 0; i <= nq; i++) off[i] = offsets[i] - g0;
        return qb;
    }
    dbl.resize(2 * nb);
    off.resize(2 * nq + 1);
    for (uint64_t i = 0; i < nq; i++) {
        const uint64_t a = offsets[i] - g0, b = offsets[i + 1] - g0;
        off[2 * i] = 2 * a; off[2 * i + 1] = a + b;
        memcpy(dbl.data() + 2 * a, qb + a, (size_t)(b - a));
        for (uint64_t t = 0; t < b - a; t++) dbl[a + b + t] = revcomp_byte(qb[b - 1 - t]);
    }
    off[2 * nq] = 2 * nb;
    return dbl.data();
}

// query a of a strand batch as the records name it
struct QueryStrand { uint64_t query; uint8_t strand; };
QueryStrand query_strand(bool both, uint64_t a) { return {both ? a >> 1 : a, (uint8_t)(both ? a & 1 : 0)}; }

// piece i of the np pigeonhole pieces of a query of m bytes: its offset, its length, and how many of its bytes are searched
// (k' = min(len, L) on a build capped at L)
struct Piece { uint64_t o, len, kk; };
Piece piece_of(uint32_t i, uint64_t m, uint32_t np, uint64_t L)
{
    const uint64_t o = (uint64_t)i * m / np, len = (uint64_t)(i + 1) * m / np - o;
    return {o, len, L > 0 && L < len ? L : len};
}

// The records of the chunks, concatenated in order, against the room of the caller: the total, E_CAPACITY when it does not
// fit, nothing to write for 0, E_INVALID for a null column; else put(t, record) writes record t to the columns.
template <typename Rec, typename Put>
int collect_records(const std::vector<std::vector<Rec>>& recs, uint64_t cap, uint64_t* total_out, bool null_column, Put put)
{
    uint64_t total = 0;
    for (const auto& v : recs) total += v.size();
    if (total_out) *total_out = total;
    if (total > cap) return SUFR_HIP_E_CAPACITY;
    if (!total) return 0;
    if (null_column) return SUFR_HIP_E_INVALID;
    uint64_t t = 0;
    for (const auto& v : recs)
        for (const Rec& x : v) put(t++, x);
    return 0;
}

}  // namespace

extern "C" {

int sufr_file_mems(const sufr_file* f, const uint8_t* queries, const uint64_t* offsets, uint64_t nq, uint32_t min_len,
                   uint64_t max_occ, uint32_t flags, uint64_t cap, uint64_t* query, uint32_t* qoff, uint8_t* strand,
                   uint32_t* len, uint64_t* position, uint64_t* total_out, int threads)
{
    if (total_out) *total_out = 0;
    if (const int rc = match_args(f, queries, offsets, nq)) return rc;
    if (min_len == 0) return SUFR_HIP_E_INVALID;
    if (!nq || offsets[nq] == offsets[0]) return 0;
    const bool both = (flags & SUFR_MEM_BOTH_STRANDS) != 0;
    std::vector<uint8_t> dbl;
    std::vector<uint64_t> off;
    const uint8_t* qb = strand_batch(queries, offsets, nq, both, dbl, off);
    const uint64_t nq2 = off.size() - 1, nb2 = off[nq2];
    const std::vector<uint64_t>& bits = indexed_bits(*f);
    const uint64_t n = f->meta.text_len, L = f->meta.max_query_len;
    const uint32_t kk = L > 0 && L < min_len ? (uint32_t)L : min_len;                    // k' of the contract
    const uint8_t* text = f->text;
    // workers over chunks of query bytes; chunk c keeps its records, the chunks are concatenated in order
    const uint64_t chunk = 4096, nchunks = (nb2 + chunk - 1) / chunk;
    std::vector<std::vector<MemRec>> recs(nchunks);
    parallel_chunks(nb2, chunk, threads, [&](uint64_t b, uint64_t e) {
        std::vector<MemRec>& out = recs[b / chunk];
        uint64_t a = query_of(off.data(), nq2, b);
        for (uint64_t g = b; g < e; g++) {
            while (off[a + 1] <= g) a++;
            const uint64_t j = g - off[a], m = off[a + 1] - off[a];
            if (j + min_len > m) continue;
            uint64_t lo = 0, hi = 0;
            if (!sufr_file_search(f, qb + g, kk, 0, 0, &lo, &hi)) continue;
            if (max_occ && hi - lo > max_occ) continue;
            for (uint64_t r = lo; r < hi; r++) {
                const uint64_t p = sufr_file_suffix(f, r);
                if (j > 0 && p > 0 && qb[g - 1] == text[p - 1] && (bits.empty() || (bits[(p - 1) >> 6] >> ((p - 1) & 63) & 1))) continue;
                const uint64_t lim = m - j < n - p ? m - j : n - p;
                uint64_t l = kk;                                                         // the slice matched
                while (l < lim && qb[g + l] == text[p + l]) l++;
                if (l < min_len) continue;
                const QueryStrand qs = query_strand(both, a);
                out.push_back({qs.query, (uint32_t)j, qs.strand, (uint32_t)l, p});
            }
        }
    });
    return collect_records(recs, cap, total_out, !query || !qoff || !strand || !len || !position, [&](uint64_t t, const MemRec& x) {
        query[t] = x.query; qoff[t] = x.qoff; strand[t] = x.strand; len[t] = x.len; position[t] = x.pos;
    });
}

}  // extern "C"

// ---- k-mismatch search (include/sufr_approx.h) --------------------------------------------------
namespace {

struct ApproxRec { uint64_t query; uint8_t strand; uint64_t pos; uint8_t mism; };

}  // namespace

extern "C" {

int sufr_file_approx(const sufr_file* f, const uint8_t* queries, const uint64_t* offsets, uint64_t nq, uint32_t max_mismatches,
                     uint64_t max_occ, uint32_t flags, uint64_t cap, uint64_t* query, uint8_t* strand, uint64_t* position,
                     uint8_t* mismatches, uint64_t* total_out, int threads)
{
    if (total_out) *total_out = 0;
    if (const int rc = match_args(f, queries, offsets, nq)) return rc;
    if (max_mismatches > SUFR_APPROX_MAX_MISMATCHES) return SUFR_HIP_E_INVALID;
    if (!nq || offsets[nq] == offsets[0]) return 0;
    const bool both = (flags & SUFR_APPROX_BOTH_STRANDS) != 0;
    std::vector<uint8_t> dbl;
    std::vector<uint64_t> off;
    const uint8_t* qb = strand_batch(queries, offsets, nq, both, dbl, off);
    const uint64_t nq2 = off.size() - 1;
    const std::vector<uint64_t>& bits = indexed_bits(*f);
    const uint64_t n = f->meta.text_len, L = f->meta.max_query_len;
    const uint32_t d = max_mismatches, np = d + 1;
    const uint8_t* text = f->text;
    // workers over chunks of queries; chunk c keeps its records, the chunks are concatenated in order
    const uint64_t chunk = 16, nchunks = (nq2 + chunk - 1) / chunk;
    std::vector<std::vector<ApproxRec>> recs(nchunks);
    parallel_chunks(nq2, chunk, threads, [&](uint64_t b, uint64_t e) {
        std::vector<ApproxRec>& out = recs[b / chunk];
        Piece pc[SUFR_APPROX_MAX_MISMATCHES + 1];
        uint64_t lo[SUFR_APPROX_MAX_MISMATCHES + 1], hi[SUFR_APPROX_MAX_MISMATCHES + 1];
        bool live[SUFR_APPROX_MAX_MISMATCHES + 1];
        for (uint64_t a = b; a < e; a++) {
            const uint8_t* Q = qb + off[a];
            const uint64_t m = off[a + 1] - off[a];
            if (m < np || m > n) continue;
            for (uint32_t i = 0; i < np; i++) {                              // the rank range of every seed
                pc[i] = piece_of(i, m, np, L);
                lo[i] = hi[i] = 0;
                (void)sufr_file_search(f, Q + pc[i].o, (size_t)pc[i].kk, 0, 0, &lo[i], &hi[i]);
                live[i] = !max_occ || hi[i] - lo[i] <= max_occ;
            }
            for (uint32_t i = 0; i < np; i++) {
                if (!live[i]) continue;
                const uint64_t o = pc[i].o, len = pc[i].len, kk = pc[i].kk;
                for (uint64_t r = lo[i]; r < hi[i]; r++) {
                    const uint64_t sp = sufr_file_suffix(f, r);
                    if (sp < o) continue;                                    // the window would start before the text
                    const uint64_t p = sp - o;
                    if (p + m > n) continue;
                    if (kk < len && memcmp(Q + o + kk, text + sp + kk, (size_t)(len - kk)) != 0) continue;
                    bool lower = false;                                      // a lower piece anchors p: it reports the window
                    for (uint32_t j = 0; j < i && !lower; j++) {
                        const uint64_t pj = p + pc[j].o;
                        lower = live[j] && (bits.empty() || (bits[pj >> 6] >> (pj & 63) & 1)) &&
                                memcmp(Q + pc[j].o, text + pj, (size_t)pc[j].len) == 0;
                    }
                    if (lower) continue;
                    uint32_t h = 0;
                    for (uint64_t t = 0; t < m && h <= d; t++) h += Q[t] != text[p + t];
                    if (h > d) continue;
                    const QueryStrand qs = query_strand(both, a);
                    out.push_back({qs.query, qs.strand, p, (uint8_t)h});
                }
            }
        }
    }, 4);
    return collect_records(recs, cap, total_out, !query || !strand || !position || !mismatches, [&](uint64_t t, const ApproxRec& x) {
        query[t] = x.query; strand[t] = x.strand; position[t] = x.pos; mismatches[t] = x.mism;
    });
}

}  // extern "C"

// ---- k-difference search (include/sufr_edit.h) --------------------------------------------------
namespace {

struct EditRec { uint64_t query; uint8_t strand; uint64_t end; uint8_t edits; };

// The band of diagonal p: row r holds the cells of the columns p + r - 2d + k, k = 0 .. 4d; +inf outside the band and outside
// [0, n]; row 0 is free.  Plain cells, one row kept (the device walks the same band bit-parallel).  last: row m.
void edit_band_scalar(const uint8_t* Q, uint64_t m, const uint8_t* T, uint64_t n, int64_t p, uint32_t d, std::vector<uint32_t>& prev,
                      std::vector<uint32_t>& cur)
{
    const int64_t W = 4 * (int64_t)d + 1, sn = (int64_t)n;
    const uint32_t INF = 1u << 20;
    prev.assign((size_t)W + 2, INF);
    cur.assign((size_t)W + 2, INF);
    for (int64_t k = 0; k < W; k++) { const int64_t c = p - 2 * (int64_t)d + k; if (c >= 0 && c <= sn) prev[(size_t)k + 1] = 0; }
    for (uint64_t r = 1; r <= m; r++) {
        uint32_t low = INF;
        for (int64_t k = 0; k < W; k++) {
            const int64_t c = p + (int64_t)r - 2 * (int64_t)d + k;
            uint32_t v = INF;
            if (c >= 0 && c <= sn) {
                if (c >= 1) v = std::min(v, prev[(size_t)k + 1] + (Q[r - 1] != T[c - 1]));       // (r - 1, c - 1)
                v = std::min(v, prev[(size_t)k + 2] + 1);                                        // (r - 1, c)
                v = std::min(v, cur[(size_t)k] + 1);                                             // (r, c - 1)
            }
            cur[(size_t)k + 1] = std::min(v, INF);
            low = std::min(low, v);
        }
        prev.swap(cur);
        cur[0] = INF;
        if (low > d) { prev.assign((size_t)W + 2, INF); return; }                                // nothing below comes back under d
    }
}

}  // namespace

extern "C" {

int sufr_file_edit(const sufr_file* f, const uint8_t* queries, const uint64_t* offsets, uint64_t nq, uint32_t max_edits, uint64_t max_occ,
                   uint32_t flags, uint64_t cap, uint64_t* query, uint8_t* strand, uint64_t* end, uint8_t* edits, uint64_t* total_out,
                   int threads)
{
    if (total_out) *total_out = 0;
    if (const int rc = match_args(f, queries, offsets, nq)) return rc;
    if (max_edits > SUFR_EDIT_MAX_EDITS) return SUFR_HIP_E_INVALID;
    if (!nq || offsets[nq] == offsets[0]) return 0;
    const bool both = (flags & SUFR_EDIT_BOTH_STRANDS) != 0, minima = (flags & SUFR_EDIT_LOCAL_MINIMA) != 0;
    std::vector<uint8_t> dbl;
    std::vector<uint64_t> off;
    const uint8_t* qb = strand_batch(queries, offsets, nq, both, dbl, off);
    const uint64_t nq2 = off.size() - 1;
    const uint64_t n = f->meta.text_len, L = f->meta.max_query_len;
    const uint32_t d = max_edits, np = d + 1;
    const uint8_t* text = f->text;
    // workers over chunks of queries; chunk c keeps its records, the chunks are concatenated in order
    const uint64_t chunk = 16, nchunks = (nq2 + chunk - 1) / chunk;
    std::vector<std::vector<EditRec>> recs(nchunks);
    parallel_chunks(nq2, chunk, threads, [&](uint64_t b, uint64_t e) {
        std::vector<EditRec>& out = recs[b / chunk];
        std::vector<int64_t> diags;
        std::vector<std::pair<uint64_t, uint32_t>> ends;                     // (exclusive end, D)
        std::vector<uint32_t> row, tmp;
        for (uint64_t a = b; a < e; a++) {
            const uint8_t* Q = qb + off[a];
            const uint64_t m = off[a + 1] - off[a];
            if (m < np) continue;
            diags.clear();
            for (uint32_t i = 0; i < np; i++) {                              // the diagonals of every live seed
                const Piece pc = piece_of(i, m, np, L);
                uint64_t lo = 0, hi = 0;
                (void)sufr_file_search(f, Q + pc.o, (size_t)pc.kk, 0, 0, &lo, &hi);
                if (max_occ && hi - lo > max_occ) continue;
                for (uint64_t r = lo; r < hi; r++) diags.push_back((int64_t)sufr_file_suffix(f, r) - (int64_t)pc.o);
            }
            std::sort(diags.begin(), diags.end());
            diags.erase(std::unique(diags.begin(), diags.end()), diags.end());
            ends.clear();
            for (const int64_t p : diags) {
                edit_band_scalar(Q, m, text, n, p, d, row, tmp);
                for (uint32_t j = 0; j <= 2 * d; j++) {                      // cell d + j of the last row: the end p + m - d + j
                    const int64_t x = p + (int64_t)m - (int64_t)d + j;
                    if (x >= 1 && x <= (int64_t)n && row[(size_t)d + j + 1] <= d) ends.push_back({(uint64_t)x, row[(size_t)d + j + 1]});
                }
            }
            std::sort(ends.begin(), ends.end());
            ends.erase(std::unique(ends.begin(), ends.end()), ends.end());
            for (size_t t = 0; t < ends.size(); t++) {
                if (minima) {
                    const uint32_t v = ends[t].second;
                    const uint32_t vl = t > 0 && ends[t - 1].first + 1 == ends[t].first ? ends[t - 1].second : d + 1;
                    const uint32_t vr = t + 1 < ends.size() && ends[t + 1].first == ends[t].first + 1 ? ends[t + 1].second : d + 1;
                    if (!(vl > v && vr >= v)) continue;
                }
                const QueryStrand qs = query_strand(both, a);
                out.push_back({qs.query, qs.strand, ends[t].first - 1, (uint8_t)ends[t].second});
            }
        }
    }, 4);
    return collect_records(recs, cap, total_out, !query || !strand || !end || !edits, [&](uint64_t t, const EditRec& x) {
        query[t] = x.query; strand[t] = x.strand; end[t] = x.end; edits[t] = x.edits;
    });
}

}  // extern "C"

// ---- alignment traceback of k-difference records (include/sufr_align.h) ---------------------------
namespace {

// One record: the table of Q against T on the diagonals g - v .. g + v (g = e - m), every row kept: tab[r * W + k] is the cell
// of row r and column r + g - v + k, +inf outside the band and outside the columns 0 .. n; row 0 is free, column 0 holds r.
// Plain cells (the device keeps two bit vectors per row instead).  Then the walk of sufr_align.h, runs pushed last run first.
// false: the end cell does not hold v, so v is not D(e).
bool trace_scalar(const uint8_t* Q, uint64_t m, const uint8_t* T, uint64_t n, uint64_t e, uint32_t v, std::vector<uint32_t>& tab,
                  uint64_t& start, std::vector<uint32_t>& runs)
{
    const int64_t W = 2 * (int64_t)v + 1, sn = (int64_t)n, g = (int64_t)e - (int64_t)m;
    const uint32_t INF = 0x7FFFFFFFu;
    tab.assign((size_t)((m + 1) * (uint64_t)W), INF);
    auto col = [&](uint64_t r, int64_t k) { return (int64_t)r + g - (int64_t)v + k; };
    auto at = [&](uint64_t r, int64_t k) -> uint32_t { return k < 0 || k >= W ? INF : tab[(size_t)(r * (uint64_t)W + (uint64_t)k)]; };
    for (int64_t k = 0; k < W; k++) { const int64_t c = col(0, k); if (c >= 0 && c <= sn) tab[(size_t)k] = 0; }
    for (uint64_t r = 1; r <= m; r++)
        for (int64_t k = 0; k < W; k++) {
            const int64_t c = col(r, k);
            if (c < 0 || c > sn) continue;
            uint32_t x = INF;
            if (c >= 1 && at(r - 1, k) != INF) x = std::min(x, at(r - 1, k) + (Q[r - 1] != T[c - 1]));      // (r - 1, c - 1)
            if (at(r - 1, k + 1) != INF) x = std::min(x, at(r - 1, k + 1) + 1);                             // (r - 1, c)
            if (at(r, k - 1) != INF) x = std::min(x, at(r, k - 1) + 1);                                     // (r, c - 1)
            tab[(size_t)(r * (uint64_t)W + (uint64_t)k)] = x;
        }
    if (at(m, v) != v) return false;
    runs.clear();
    uint64_t i = m;
    int64_t k = v;
    uint32_t op = 0, len = 0;
    auto step = [&](uint32_t o) { if (o != op) { if (len) runs.push_back(len << 4 | op); op = o; len = 0; } len++; };
    while (i > 0) {
        const int64_t j = col(i, k);
        const uint32_t cur = at(i, k);
        if (j > 0 && at(i - 1, k) != INF && at(i - 1, k) + (Q[i - 1] != T[j - 1]) == cur) { step(Q[i - 1] == T[j - 1] ? 7u : 8u); i--; }
        else if (at(i - 1, k + 1) != INF && at(i - 1, k + 1) + 1 == cur) { step(1u); i--; k++; }
        else { step(2u); k--; }
    }
    if (len) runs.push_back(len << 4 | op);
    start = (uint64_t)col(0, k);
    return true;
}

}  // namespace

extern "C" {

int sufr_file_edit_trace(const sufr_file* f, const uint8_t* queries, const uint64_t* offsets, uint64_t nq, uint64_t num_records,
                         const uint64_t* query, const uint8_t* strand, const uint64_t* end, const uint8_t* edits, uint64_t cigar_cap,
                         uint64_t* start, uint64_t* cigar_off, uint32_t* cigar, uint64_t* total_out, int threads, char* err, size_t errlen)
{
    if (total_out) *total_out = 0;
    if (err && errlen) err[0] = 0;
    if (!f || !cigar_off || (cigar_cap && !cigar) || (nq && !offsets) || (nq && offsets[nq] > offsets[0] && !queries) ||
        (num_records && (!query || !strand || !end || !edits || !start))) {
        put_err(err, errlen, "trace: null argument");
        return SUFR_HIP_E_INVALID;
    }
    cigar_off[0] = 0;
    if (!num_records) return 0;
    const uint64_t n = f->meta.text_len;
    const uint8_t* text = f->text;
    // workers over chunks of records; a chunk keeps its runs, forward, record after record; cigar_off[t + 1]: the runs of t
    const uint64_t chunk = 64, nchunks = (num_records + chunk - 1) / chunk;
    std::vector<std::vector<uint32_t>> runs_of(nchunks);
    std::atomic<uint64_t> bad{~0ull};
    // the checks that need no table: record t names a query of the batch, a strand, an end of the text and a distance its query allows
    auto in_range = [&](uint64_t t) {
        return query[t] < nq && strand[t] <= 1 && end[t] < n && edits[t] <= SUFR_EDIT_MAX_EDITS &&
               offsets[query[t] + 1] >= offsets[query[t]] && offsets[query[t] + 1] - offsets[query[t]] >= (uint64_t)edits[t] + 1;
    };
    parallel_chunks(num_records, chunk, threads, [&](uint64_t b, uint64_t e) {
        std::vector<uint32_t>& out = runs_of[b / chunk];
        std::vector<uint32_t> tab, runs;
        std::vector<uint8_t> rc;
        for (uint64_t t = b; t < e; t++) {
            cigar_off[t + 1] = 0;
            start[t] = 0;
            bool ok = in_range(t);
            if (ok) {
                const uint8_t* Q = queries + offsets[query[t]];
                const uint64_t m = offsets[query[t] + 1] - offsets[query[t]];
                if (strand[t]) {
                    rc.resize((size_t)m);
                    for (uint64_t x = 0; x < m; x++) rc[(size_t)x] = revcomp_byte(Q[m - 1 - x]);
                    Q = rc.data();
                }
                ok = trace_scalar(Q, m, text, n, end[t] + 1, edits[t], tab, start[t], runs);
                if (ok) {
                    out.insert(out.end(), runs.rbegin(), runs.rend());
                    cigar_off[t + 1] = runs.size();
                }
            }
            if (!ok) { uint64_t cur = bad.load(); while (t < cur && !bad.compare_exchange_weak(cur, t)) {} }
        }
    }, 64);
    if (bad.load() != ~0ull) {
        const uint64_t t = bad.load();
        put_err(err, errlen, "trace: record " + std::to_string(t) + (!in_range(t) ? " is no record of this batch and text (query, strand, end, edits "
                             "or the length of its query out of range)" : ": edits is not D(end + 1)"));
        return SUFR_HIP_E_INVALID;
    }
    for (uint64_t t = 0; t < num_records; t++) cigar_off[t + 1] += cigar_off[t];
    const uint64_t total = cigar_off[num_records];
    if (total_out) *total_out = total;
    for (uint64_t c = 0; c < nchunks; c++) {
        const uint64_t at = cigar_off[c * chunk];
        if (at >= cigar_cap) break;
        const uint64_t cnt = std::min<uint64_t>(runs_of[c].size(), cigar_cap - at);
        if (cnt) memcpy(cigar + at, runs_of[c].data(), (size_t)cnt * 4);
    }
    if (total > cigar_cap) {
        put_err(err, errlen, "trace: " + std::to_string(total) + " CIGAR runs, room for " + std::to_string(cigar_cap));
        return SUFR_HIP_E_CAPACITY;
    }
    return 0;
}

}  // extern "C"

// ---- k-mer spectra, occurrence maps and unique lengths (include/sufr_kmer.h) ---------------------
#include "../../include/sufr_kmer.h"
#include "sufr_kmer_scan.h"

namespace {

// what both calls refuse, in the order of the device path
int kmer_args(const sufr_file* f, bool capped)
{
    if (!f) return SUFR_HIP_E_INVALID;
    if (f->meta.seed_mask_len) return SUFR_HIP_E_UNSUPPORTED;
    if (capped) return SUFR_HIP_E_UNSUPPORTED;
    return 0;
}

bool kmer_starts_ok(const sufr_file& f)
{
    const std::vector<uint64_t>& st = f.seq_starts;
    if (st.empty()) return true;
    bool ok = st[0] == 0;
    for (size_t i = 0; ok && i < st.size(); i++) ok = st[i] < f.meta.text_len && (i == 0 || st[i] > st[i - 1]);
    return ok;
}

void kmer_put(void* out, int width, uint64_t i, uint64_t v)
{
    if (width == 4) { const uint32_t x = (uint32_t)v; memcpy((uint8_t*)out + i * 4, &x, 4); }
    else memcpy((uint8_t*)out + i * 8, &v, 8);
}

}  // namespace

extern "C" {

int sufr_file_kmers(const sufr_file* f, uint64_t k, uint32_t flags, uint64_t bins, uint64_t* hist, void* occ, sufr_kmer_stats* stats,
                    int threads)
{
    if (stats) *stats = sufr_kmer_stats{0, 0, 0, 0};
    if (const int rc = kmer_args(f, f && f->meta.max_query_len > 0 && k > f->meta.max_query_len)) return rc;
    if (k == 0 || (hist && bins == 0)) return SUFR_HIP_E_INVALID;
    if (hist) memset(hist, 0, bins * 8);
    const uint64_t s = f->meta.len_suffixes, n = f->meta.text_len;
    const int width = f->meta.index_width;
    const bool by_position = (flags & SUFR_KMER_BY_POSITION) != 0;
    if (occ && by_position) memset(occ, 0, n * (uint64_t)width);
    if (!s) return 0;
    if (!kmer_starts_ok(*f)) return SUFR_HIP_E_INVALID;
    const uint64_t* starts = f->seq_starts.data();
    const uint64_t num = f->seq_starts.size();
    // pass 1: the whole flags (one bit per rank) and the summary of every chunk; the chunks hold whole words
    const uint64_t chunk = (uint64_t)1 << 16, nchunks = (s + chunk - 1) / chunk;
    std::vector<uint64_t> wbits((s + 63) / 64, 0);
    std::vector<sufr::KmerSum> sums(nchunks);
    auto head = [&](uint64_t r) { return r == 0 || rdT(f->lcp, width, r) < k; };
    parallel_chunks(s, chunk, threads, [&](uint64_t b, uint64_t e) {
        sufr::KmerSum run = sufr::kmer_identity();
        for (uint64_t r0 = b; r0 < e; r0 += 64) {
            uint64_t H = 0, W = 0;
            for (uint64_t r = r0; r < e && r < r0 + 64; r++) {
                if (head(r)) H |= (uint64_t)1 << (r - r0);
                if (sufr::kmer_whole(starts, num, n, rdT(f->sa, width, r), k)) W |= (uint64_t)1 << (r - r0);
            }
            wbits[r0 / 64] = W;
            run = sufr::kmer_combine(run, sufr::kmer_word_sum(H, W));
        }
        sums[b / chunk] = run;
    });
    // the carries of the chunks, in both directions
    std::vector<uint64_t> cin(nchunks), cout(nchunks);
    sufr::KmerSum run = sufr::kmer_identity();
    for (uint64_t c = 0; c < nchunks; c++) { cin[c] = sufr::kmer_carry_in(run, 0); run = sufr::kmer_combine(run, sums[c]); }
    run = sufr::kmer_identity();
    for (uint64_t c = nchunks; c > 0; c--) { cout[c - 1] = sufr::kmer_carry_out(run, 0); run = sufr::kmer_combine(sums[c - 1], run); }
    // pass 2: every chunk walks its intervals; an interval is credited by the chunk that holds its head
    std::mutex mu;
    sufr_kmer_stats total{0, 0, 0, 0};
    const uint64_t private_bins = hist ? (bins < 4096 ? bins : 4096) : 0;
    parallel_chunks(s, chunk, threads, [&](uint64_t b, uint64_t e) {
        const uint64_t c = b / chunk;
        std::vector<uint64_t> mine(private_bins, 0), big;
        sufr_kmer_stats st{0, 0, 0, 0};
        auto whole = [&](uint64_t r) { return (wbits[r / 64] >> (r & 63)) & 1; };
        uint64_t a = b;                                   // start of the interval piece being walked
        bool headed = head(b);                            // ... and whether its head is in this chunk
        while (a < e) {
            uint64_t z = a + 1, cnt = whole(a);
            while (z < e && !head(z)) { cnt += whole(z); z++; }
            uint64_t tot = cnt;
            if (!headed) tot += cin[c];
            if (z == e) tot += cout[c];
            if (occ) for (uint64_t r = a; r < z; r++) {
                if (!by_position) kmer_put(occ, width, r, whole(r) ? tot : 0);
                else if (whole(r)) kmer_put(occ, width, rdT(f->sa, width, r), tot);
            }
            if (headed && tot) {
                st.whole += tot; st.distinct++; st.unique += tot == 1;
                if (tot > st.max_count) st.max_count = tot;
                const uint64_t bin = hist ? sufr::kmer_bin(tot, bins) : 0;
                if (hist && bin < private_bins) mine[bin]++; else if (hist) big.push_back(bin);
            }
            a = z; headed = true;
        }
        std::lock_guard<std::mutex> g(mu);
        total.whole += st.whole; total.distinct += st.distinct; total.unique += st.unique;
        if (st.max_count > total.max_count) total.max_count = st.max_count;
        for (uint64_t i = 0; i < private_bins; i++) hist[i] += mine[i];
        for (const uint64_t bin : big) hist[bin]++;
    });
    if (stats) *stats = total;
    return 0;
}

int sufr_file_unique_lengths(const sufr_file* f, uint32_t flags, void* out, int threads)
{
    if (const int rc = kmer_args(f, f && f->meta.max_query_len > 0)) return rc;
    const uint64_t s = f->meta.len_suffixes, n = f->meta.text_len;
    const int width = f->meta.index_width;
    const bool by_position = (flags & SUFR_KMER_BY_POSITION) != 0;
    if (by_position && out) memset(out, 0, n * (uint64_t)width);
    if (!s) return 0;
    if (!kmer_starts_ok(*f) || !out) return SUFR_HIP_E_INVALID;
    const uint64_t* starts = f->seq_starts.data();
    const uint64_t num = f->seq_starts.size();
    parallel_chunks(s, (uint64_t)1 << 16, threads, [&](uint64_t b, uint64_t e) {
        for (uint64_t r = b; r < e; r++) {
            const uint64_t x = rdT(f->lcp, width, r), y = r + 1 < s ? rdT(f->lcp, width, r + 1) : 0, p = rdT(f->sa, width, r);
            const uint64_t u = 1 + (x > y ? x : y);
            const uint64_t v = sufr::kmer_whole(starts, num, n, p, u) ? u : 0;
            if (!by_position) kmer_put(out, width, r, v);
            else if (v) kmer_put(out, width, p, v);
        }
    });
    return 0;
}

}  // extern "C"

// ---- repeats of the indexed text (include/sufr_repeat.h) ----------------------------------------
#include "../../include/sufr_repeat.h"
#include "sufr_repeat_scan.h"
#include "sufr_shared_scan.h"

namespace {

// what the searches of sufr_repeat_scan.h read: l (the file's LCP with one sequence, a clipped copy otherwise), the coarser
// levels of the min pyramid and the suffix array
struct RepeatHostAcc {
    const uint8_t *sa_bytes, *lcp;
    int width;
    const uint64_t *ell, *up;
    uint64_t s;
    uint64_t at(uint32_t level, uint64_t off, uint64_t i) const          // off: rep_level_offset(s, level)
    {
        if (level) return up[off + i];
        return ell ? ell[i] : (i ? rdT(lcp, width, i) : 0);
    }
    uint64_t sa(uint64_t r) const { return rdT(sa_bytes, width, r); }
};

// pass 1 of the calls that search the clipped LCP (repeats, shared): l (several sequences only), the "differs from the
// previous rank" and "sequence start" flag words with their popcount prefixes, and the coarser levels of the min pyramid
struct RepeatHostPrep {
    std::vector<uint64_t> ell, dw, sw, dp, sp, up;
    RepeatHostAcc acc(const sufr_file* f) const
    {
        return RepeatHostAcc{f->sa, f->lcp, f->meta.index_width, f->seq_starts.size() > 1 ? ell.data() : nullptr, up.data(), f->meta.len_suffixes};
    }
};

void repeat_host_prepare(const sufr_file* f, int threads, RepeatHostPrep& P)
{
    const uint64_t* starts = f->seq_starts.data();
    const uint64_t num = f->seq_starts.size();
    const uint8_t* text = f->text;
    const uint64_t s = f->meta.len_suffixes, n = f->meta.text_len;
    const int width = f->meta.index_width;
    const uint64_t chunk = (uint64_t)1 << 16, nwords = (s + 63) / 64;
    const uint32_t levels = sufr::rep_levels(s);
    std::vector<uint64_t>&ell = P.ell, &dw = P.dw, &sw = P.sw, &dp = P.dp, &sp = P.sp, &up = P.up;
    ell.assign(num > 1 ? s : 0, 0); dw.assign(nwords, 0); sw.assign(nwords, 0); dp.assign(nwords, 0); sp.assign(nwords, 0);
    up.assign(sufr::rep_level_offset(s, levels + 1), 0);
    parallel_chunks(s, chunk, threads, [&](uint64_t b, uint64_t e) {
        bool pstart = false;
        uint8_t plam = 0;
        uint64_t proom = 0;
        if (b) {                                          // the rank before the chunk belongs to another chunk: load it
            const uint64_t pp = rdT(f->sa, width, b - 1);
            pstart = sufr::rep_is_start(starts, num, n, pp);
            plam = pstart ? 0 : text[pp - 1];
            proom = sufr::rep_room(starts, num, n, pp);
        }
        for (uint64_t r0 = b; r0 < e; r0 += 64) {
            uint64_t D = 0, S = 0, low = ~(uint64_t)0;
            for (uint64_t r = r0; r < e && r < r0 + 64; r++) {
                const uint64_t p = rdT(f->sa, width, r);
                const bool start = sufr::rep_is_start(starts, num, n, p);
                const uint8_t lam = start ? 0 : text[p - 1];
                const uint64_t room = sufr::rep_room(starts, num, n, p);
                const uint64_t v = r == 0 ? 0 : num > 1 ? sufr::rep_clip(rdT(f->lcp, width, r), proom, room) : rdT(f->lcp, width, r);
                if (num > 1) ell[r] = v;
                if (v < low) low = v;
                if (r && (start || pstart || lam != plam)) D |= (uint64_t)1 << (r - r0);
                if (start) S |= (uint64_t)1 << (r - r0);
                pstart = start; plam = lam; proom = room;
            }
            dw[r0 / 64] = D; sw[r0 / 64] = S;
            if (levels) up[r0 / 64] = low;
        }
    });
    uint64_t nd = 0, ns = 0;
    for (uint64_t i = 0; i < nwords; i++) {
        dp[i] = nd; sp[i] = ns;
        nd += (uint64_t)__builtin_popcountll(dw[i]); ns += (uint64_t)__builtin_popcountll(sw[i]);
    }
    for (uint32_t k = 2; k <= levels; k++)
        sufr::rep_level_up(up.data() + sufr::rep_level_offset(s, k - 1), sufr::rep_level_size(s, k - 1), up.data() + sufr::rep_level_offset(s, k),
                           sufr::rep_level_size(s, k));
}

struct RepeatHostFilter { uint32_t kind; uint64_t min_len, min_count, max_count, min_seqs, max_seqs; };

// where the find pass leaves its records (seqs: only with P), and what it met: the kept ranks and their RepBest
struct RepeatHostOut {
    uint64_t cap, *rank, *count, *length, *seqs;
    uint64_t records;
    sufr::RepBest best;
};

// pass 2 of repeats (P null: no sequences are counted, best.seq stays 0) and of shared: every chunk decides its own ranks;
// the records of the chunks, one after the other, are in representative order.  A counting call (fill false) keeps none.
// Then the capacity rule and the copy-out.
int repeat_host_find(const sufr_file* f, const RepeatHostPrep& prep, const uint64_t* P, const RepeatHostFilter& flt, bool fill, int threads,
                     RepeatHostOut& out)
{
    struct Rec { uint64_t rank, count, length, seqs; };
    const uint64_t s = f->meta.len_suffixes, chunk = (uint64_t)1 << 16, nchunks = (s + chunk - 1) / chunk;
    const RepeatHostAcc acc = prep.acc(f);
    std::vector<std::vector<Rec>> recs(nchunks);
    std::vector<uint64_t> kept(nchunks, 0);
    std::vector<sufr::RepBest> best(nchunks, sufr::RepBest{0, 0, 0, 0, 0});
    parallel_chunks(s, chunk, threads, [&](uint64_t b, uint64_t e) {
        for (uint64_t r = b ? b : 1; r < e; r++)
            sufr::rep_interval(acc, s, r, flt.min_len, [&](uint64_t a, uint64_t z, uint64_t v) {
                if (!sufr::rep_keep(acc, f->text, prep.dw.data(), prep.dp.data(), prep.sw.data(), prep.sp.data(), flt.kind, flt.min_count,
                                    flt.max_count, a, z, v)) return;
                const uint64_t q = P ? sufr::shr_seqs(P, a, z) : 0;
                if (P && !sufr::shr_keep(q, flt.min_seqs, flt.max_seqs)) return;
                kept[b / chunk]++;
                if (fill) recs[b / chunk].push_back(Rec{a, z - a, v, q});
                best[b / chunk].take(v, r, a, z - a, q);
            });
    });
    out.records = 0;
    out.best = sufr::RepBest{0, 0, 0, 0, 0};
    for (uint64_t c = 0; c < nchunks; c++) { out.records += kept[c]; out.best.merge(best[c]); }
    if (out.records > out.cap) return SUFR_HIP_E_CAPACITY;
    if (out.records && (!out.rank || !out.count || !out.length || (P && !out.seqs))) return SUFR_HIP_E_INVALID;
    uint64_t o = 0;
    for (uint64_t c = 0; c < nchunks; c++)
        for (const Rec& x : recs[c]) {
            out.rank[o] = x.rank; out.count[o] = x.count; out.length[o] = x.length;
            if (P) out.seqs[o] = x.seqs;
            o++;
        }
    return 0;
}

}  // namespace

extern "C" {

int sufr_file_repeats(const sufr_file* f, uint32_t kind, uint64_t min_len, uint64_t min_count, uint64_t max_count, uint64_t cap,
                      uint64_t* rank, uint64_t* count, uint64_t* length, uint64_t* total_out, sufr_repeat_stats* stats, int threads)
{
    if (stats) *stats = sufr_repeat_stats{0, 0, 0, 0};
    if (total_out) *total_out = 0;
    if (const int rc = kmer_args(f, f && f->meta.max_query_len > 0)) return rc;
    if (min_len == 0 || kind > SUFR_REPEAT_SUPERMAXIMAL) return SUFR_HIP_E_INVALID;
    if (!f->meta.len_suffixes) return 0;
    if (!kmer_starts_ok(*f)) return SUFR_HIP_E_INVALID;
    // pass 1: l (several sequences only), the "differs from the previous rank" and "sequence start" flags, the pyramid
    RepeatHostPrep prep;
    repeat_host_prepare(f, threads, prep);
    RepeatHostOut out{cap, rank, count, length, nullptr, 0, {}};
    const int rc = repeat_host_find(f, prep, nullptr, RepeatHostFilter{kind, min_len, min_count < 2 ? 2 : min_count, max_count, 0, 0}, cap > 0, threads, out);
    if (stats) *stats = sufr_repeat_stats{out.records, out.best.len, out.best.rank, out.best.cnt};
    if (total_out) *total_out = out.records;
    return rc;
}

}  // extern "C"

// ---- longest previous factors and the LZ77 parse (include/sufr_lz.h) ---------------------------
#include "../../include/sufr_lz.h"
#include "sufr_lz_scan.h"

namespace {

// what the searches and the range minimum of sufr_lz_scan.h read: a mapped array of the file and the coarser levels of its
// min pyramid
struct LzHostAcc {
    const uint8_t* bytes;
    int width;
    const uint64_t* up;
    uint64_t at(uint32_t level, uint64_t off, uint64_t i) const { return level ? up[off + i] : rdT(bytes, width, i); }
};

// the coarser levels of the min pyramid over a mapped array of s entries
std::vector<uint64_t> lz_pyramid(const uint8_t* bytes, int width, uint64_t s, int threads)
{
    const uint32_t levels = sufr::rep_levels(s);
    std::vector<uint64_t> up(sufr::rep_level_offset(s, levels + 1));
    if (!levels) return up;
    parallel_chunks(s, (uint64_t)1 << 16, threads, [&](uint64_t b, uint64_t e) {
        for (uint64_t r0 = b; r0 < e; r0 += 64) {
            uint64_t low = ~(uint64_t)0;
            for (uint64_t r = r0; r < e && r < r0 + 64; r++) { const uint64_t v = rdT(bytes, width, r); if (v < low) low = v; }
            up[r0 / 64] = low;
        }
    });
    for (uint32_t k = 2; k <= levels; k++)
        sufr::rep_level_up(up.data() + sufr::rep_level_offset(s, k - 1), sufr::rep_level_size(s, k - 1), up.data() + sufr::rep_level_offset(s, k),
                           sufr::rep_level_size(s, k));
    return up;
}

// the refusals of both calls
int lz_args(const sufr_file* f)
{
    if (const int rc = kmer_args(f, f && f->meta.max_query_len > 0)) return rc;
    if (f->meta.len_suffixes && !kmer_starts_ok(*f)) return SUFR_HIP_E_INVALID;
    return 0;
}

// LPF and SRC of every position, n entries of `width` bytes each (either may be null); put: kmer_put
void lz_host_lpf(const sufr_file& f, void* lpf, void* src, int width, int threads)
{
    const uint64_t s = f.meta.len_suffixes, n = f.meta.text_len;
    if (lpf) memset(lpf, 0, n * (uint64_t)width);
    if (src) memset(src, 0xFF, n * (uint64_t)width);
    if (!s || (!lpf && !src)) return;
    const int fw = f.meta.index_width;
    const std::vector<uint64_t> up_sa = lz_pyramid(f.sa, fw, s, threads), up_lcp = lz_pyramid(f.lcp, fw, s, threads);
    const LzHostAcc sa{f.sa, fw, up_sa.data()}, lcp{f.lcp, fw, up_lcp.data()};
    const uint64_t* starts = f.seq_starts.data();
    const uint64_t num = f.seq_starts.size();
    parallel_chunks(s, (uint64_t)1 << 14, threads, [&](uint64_t b, uint64_t e) {
        for (uint64_t r = b; r < e; r++) {
            const uint64_t p = rdT(f.sa, fw, r);
            const sufr::LzEntry x = sufr::lz_rank(sa, lcp, s, r, p, sufr::rep_room(starts, num, n, p));
            if (lpf) kmer_put(lpf, width, p, x.lpf);
            if (src) kmer_put(src, width, p, x.src);      // (LZ_NONE is all ones of either width)
        }
    });
}

}  // namespace

extern "C" {

int sufr_file_lpf(const sufr_file* f, void* lpf, void* src, int threads)
{
    if (const int rc = lz_args(f)) return rc;
    lz_host_lpf(*f, lpf, src, f->meta.index_width, threads);
    return 0;
}

int sufr_file_lz(const sufr_file* f, uint64_t cap, uint64_t* start, uint64_t* length, uint64_t* source, uint64_t* total_out,
                 sufr_lz_stats* stats, int threads)
{
    if (stats) *stats = sufr_lz_stats{0, 0, 0, 0};
    if (total_out) *total_out = 0;
    if (const int rc = lz_args(f)) return rc;
    const uint64_t n = f->meta.text_len;
    if (!n) return 0;
    std::vector<uint64_t> lpf(n), src(n);
    lz_host_lpf(*f, lpf.data(), src.data(), 8, threads);
    // the parse is a plain serial walk: once for the total and the stats, once more to fill
    sufr_lz_stats st{0, 0, 0, 0};
    for (uint64_t p = 0; p < n; p += sufr::lz_step(lpf[p])) {
        st.factors++;
        if (!lpf[p]) st.literals++;
        if (sufr::lz_step(lpf[p]) > st.longest) { st.longest = sufr::lz_step(lpf[p]); st.longest_start = p; }
    }
    if (stats) *stats = st;
    if (total_out) *total_out = st.factors;
    if (st.factors > cap) return SUFR_HIP_E_CAPACITY;
    if (!start || !length || !source) return SUFR_HIP_E_INVALID;
    uint64_t o = 0;
    for (uint64_t p = 0; p < n; p += sufr::lz_step(lpf[p]), o++) { start[o] = p; length[o] = sufr::lz_step(lpf[p]); source[o] = lpf[p] ? src[p] : sufr::LZ_NONE; }
    return 0;
}

}  // extern "C"

// ---- sequence counts of repeats and k-common substrings (include/sufr_shared.h) ------------------
#include "../../include/sufr_shared.h"
#include "sufr_shared_scan.h"

namespace {

// the refusals both calls share
int shared_args(const sufr_file* f)
{
    if (const int rc = kmer_args(f, f && f->meta.max_query_len > 0)) return rc;
    return 0;
}

// P[0..s]: the exclusive prefix of H, H[j] the pairs (prev[r], r) with q(r) = j.  D and prev by one serial pass with a
// last-seen table; the pairs threaded over chunks of ranks, added with atomics (integer adds commute); a serial prefix.
std::vector<uint64_t> shared_host_prefix(const sufr_file* f, const RepeatHostAcc& acc, int threads)
{
    const uint64_t s = f->meta.len_suffixes, num = f->seq_starts.size();
    const uint64_t* starts = f->seq_starts.data();
    const int width = f->meta.index_width;
    std::vector<uint64_t> prev(s), last(num ? num : 1, sufr::REP_NONE), P(s + 1, 0);
    for (uint64_t r = 0; r < s; r++) {
        const uint64_t d = sufr::shr_doc(starts, num, rdT(f->sa, width, r));
        prev[r] = last[d];
        last[d] = r;
    }
    uint64_t* H = P.data();
    parallel_chunks(s, (uint64_t)1 << 14, threads, [&](uint64_t b, uint64_t e) {
        for (uint64_t r = b; r < e; r++)
            if (prev[r] != sufr::REP_NONE) __atomic_fetch_add(&H[sufr::shr_pair(acc, s, prev[r], r)], (uint64_t)1, __ATOMIC_RELAXED);
    });
    uint64_t run = 0;
    for (uint64_t j = 0; j <= s; j++) { const uint64_t h = P[j]; P[j] = run; run += h; }
    return P;
}

}  // namespace

extern "C" {

int sufr_file_shared(const sufr_file* f, uint32_t kind, uint64_t min_len, uint64_t min_count, uint64_t max_count, uint64_t min_seqs,
                     uint64_t max_seqs, uint64_t cap, uint64_t* rank, uint64_t* count, uint64_t* length, uint64_t* seqs,
                     uint64_t* total_out, sufr_shared_stats* stats, int threads)
{
    if (stats) *stats = sufr_shared_stats{0, 0, 0, 0, 0};
    if (total_out) *total_out = 0;
    if (const int rc = shared_args(f)) return rc;
    if (min_len == 0 || kind > SUFR_REPEAT_SUPERMAXIMAL || (max_seqs && min_seqs > max_seqs)) return SUFR_HIP_E_INVALID;
    if (!f->meta.len_suffixes) return 0;
    if (!kmer_starts_ok(*f)) return SUFR_HIP_E_INVALID;
    RepeatHostPrep prep;
    repeat_host_prepare(f, threads, prep);
    const std::vector<uint64_t> P = shared_host_prefix(f, prep.acc(f), threads);
    RepeatHostOut out{cap, rank, count, length, seqs, 0, {}};
    const int rc = repeat_host_find(f, prep, P.data(), RepeatHostFilter{kind, min_len, min_count < 2 ? 2 : min_count, max_count, min_seqs, max_seqs},
                                    cap > 0, threads, out);
    if (stats) *stats = sufr_shared_stats{out.records, out.best.len, out.best.rank, out.best.cnt, out.best.seq};
    if (total_out) *total_out = out.records;
    return rc;
}

int sufr_file_common(const sufr_file* f, uint64_t* common, int threads)
{
    if (const int rc = shared_args(f)) return rc;
    if (!common) return SUFR_HIP_E_INVALID;
    const uint64_t s = f->meta.len_suffixes, num = f->seq_starts.size() ? f->seq_starts.size() : 1;
    for (uint64_t i = 0; i < num; i++) common[i] = 0;
    if (!s) return 0;
    if (!kmer_starts_ok(*f)) return SUFR_HIP_E_INVALID;
    RepeatHostPrep prep;
    repeat_host_prepare(f, threads, prep);
    const RepeatHostAcc acc = prep.acc(f);
    const std::vector<uint64_t> P = shared_host_prefix(f, acc, threads);
    // common[k - 1] first holds the longest interval of exactly k sequences (a maximum: the order of the updates is
    // immaterial), then the suffix maximum
    parallel_chunks(s, (uint64_t)1 << 16, threads, [&](uint64_t b, uint64_t e) {
        for (uint64_t r = b ? b : 1; r < e; r++)
            sufr::rep_interval(acc, s, r, 1, [&](uint64_t a, uint64_t z, uint64_t v) {
                uint64_t* at = &common[sufr::shr_seqs(P.data(), a, z) - 1];
                uint64_t cur = __atomic_load_n(at, __ATOMIC_RELAXED);
                while (v > cur && !__atomic_compare_exchange_n(at, &cur, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
            });
    });
    for (uint64_t i = num - 1; i > 0; i--) if (common[i] > common[i - 1]) common[i - 1] = common[i];
    return 0;
}

}  // extern "C"

// ---- the BWT of the indexed text, its runs and the LF mapping (include/sufr_bwt.h) --------------
#include "../../include/sufr_bwt.h"
#include "sufr_bwt_scan.h"

namespace {

// The ranks are cut into tiles of this many, whatever the number of workers: a worker takes whole tiles, what crosses a tile's
// end goes through per-tile summaries (sufr_bwt_scan.h), and so every result is the same for every thread count.
constexpr uint64_t BWT_HOST_TILE = (uint64_t)1 << 16;

// BWT[b, e) into out[b, e) (where out is not null) and its byte counts added to hist (256 entries, where not null)
void bwt_host_range(const sufr_file& f, uint64_t b, uint64_t e, uint8_t* out, uint64_t* hist)
{
    const uint64_t n = f.meta.text_len;
    const int fw = f.meta.index_width;
    for (uint64_t r = b; r < e; r++) {
        const uint8_t c = f.text[sufr::bwt_source(rdT(f.sa, fw, r), n)];
        if (out) out[r] = c;
        if (hist) hist[c]++;
    }
}

std::vector<uint8_t> bwt_host_bytes(const sufr_file& f, int threads)
{
    std::vector<uint8_t> bwt(f.meta.len_suffixes);
    parallel_chunks(bwt.size(), BWT_HOST_TILE, threads, [&](uint64_t b, uint64_t e) { bwt_host_range(f, b, e, bwt.data(), nullptr); });
    return bwt;
}

// ext[t] of sufr_bwt_scan.h for the tiles of BWT_HOST_TILE ranks: the summaries in parallel, then one sweep from the last tile
std::vector<uint64_t> bwt_host_carry(const std::vector<uint8_t>& bwt, int threads)
{
    const uint64_t s = bwt.size(), ntiles = (s + BWT_HOST_TILE - 1) / BWT_HOST_TILE;
    std::vector<uint64_t> pre(ntiles), ext(ntiles, 0);
    parallel_chunks(s, BWT_HOST_TILE, threads, [&](uint64_t b, uint64_t e) {
        uint64_t i = b + 1;
        while (i < e && bwt[i] == bwt[b]) i++;
        pre[b / BWT_HOST_TILE] = i - b;
    });
    for (uint64_t t = ntiles - 1; t-- > 0;) {
        const uint64_t nb = (t + 1) * BWT_HOST_TILE, nlen = s - nb < BWT_HOST_TILE ? s - nb : BWT_HOST_TILE;
        const sufr::BwtLink k = sufr::bwt_link(bwt[nb - 1], bwt[nb], pre[t + 1], nlen);
        ext[t] = k.add + k.pass * ext[t + 1];
    }
    return ext;
}

// fn(rank, length) for every run whose head lies in tile [b, e), in ascending rank; nothing beyond the tile is read but the
// byte in front of it
template <typename F>
void bwt_host_tile_runs(const std::vector<uint8_t>& bwt, uint64_t b, uint64_t e, uint64_t ext, F fn)
{
    uint64_t head = b;                                   // the head of the run the scan is in; a run that enters from the left is skipped
    bool mine = b == 0 || bwt[b] != bwt[b - 1];
    for (uint64_t i = b + 1; i <= e; i++) {
        if (i < e && bwt[i] == bwt[i - 1]) continue;
        if (mine) fn(head, sufr::bwt_run_length(head - b, i - b, e - b, ext));
        head = i; mine = true;
    }
}

}  // namespace

extern "C" {

int sufr_file_bwt(const sufr_file* f, uint8_t* bwt, uint64_t* counts, int threads)
{
    if (!f) return SUFR_HIP_E_INVALID;
    if (counts) memset(counts, 0, 256 * sizeof(uint64_t));
    if (!bwt && !counts) return 0;
    parallel_chunks(f->meta.len_suffixes, BWT_HOST_TILE, threads, [&](uint64_t b, uint64_t e) {
        uint64_t hist[256] = {0};
        bwt_host_range(*f, b, e, bwt, counts ? hist : nullptr);
        if (counts) for (int c = 0; c < 256; c++) if (hist[c]) __atomic_fetch_add(&counts[c], hist[c], __ATOMIC_RELAXED);      // (sums: any order)
    });
    return 0;
}

int sufr_file_bwt_runs(const sufr_file* f, uint64_t min_len, uint64_t cap, uint64_t* rank, uint64_t* length, uint64_t* symbol, uint64_t* first,
                       uint64_t* total_out, sufr_bwt_stats* stats, int threads)
{
    if (stats) *stats = sufr_bwt_stats{0, 0, 0, 0};
    if (total_out) *total_out = 0;
    if (!f) return SUFR_HIP_E_INVALID;
    const uint64_t s = f->meta.len_suffixes, ntiles = (s + BWT_HOST_TILE - 1) / BWT_HOST_TILE;
    if (!s) return 0;
    min_len = sufr::bwt_min_len(min_len);
    const std::vector<uint8_t> bwt = bwt_host_bytes(*f, threads);
    const std::vector<uint64_t> ext = bwt_host_carry(bwt, threads);
    // per tile: the kept heads (then their exclusive scan), the heads, the longest run and its rank
    std::vector<uint64_t> kept(ntiles + 1, 0), heads(ntiles, 0), b_len(ntiles, 0), b_at(ntiles, 0);
    parallel_chunks(s, BWT_HOST_TILE, threads, [&](uint64_t b, uint64_t e) {
        const uint64_t t = b / BWT_HOST_TILE;
        uint64_t n_heads = 0, n_kept = 0, best = 0, best_at = 0;     // (summed here, stored once: neighbouring tiles share cache lines)
        bwt_host_tile_runs(bwt, b, e, ext[t], [&](uint64_t a, uint64_t len) {
            n_heads++;
            if (len >= min_len) n_kept++;
            if (sufr::rep_better(len, a, best, best_at)) { best = len; best_at = a; }
        });
        heads[t] = n_heads; kept[t] = n_kept; b_len[t] = best; b_at[t] = best_at;
    });
    sufr_bwt_stats st{0, 0, 0, 0};
    for (uint64_t t = 0; t < ntiles; t++) {
        const uint64_t k = kept[t];
        kept[t] = st.records; st.records += k; st.runs += heads[t];
        if (sufr::rep_better(b_len[t], b_at[t], st.longest, st.longest_rank)) { st.longest = b_len[t]; st.longest_rank = b_at[t]; }
    }
    if (stats) *stats = st;
    if (total_out) *total_out = st.records;
    if (st.records > cap) return SUFR_HIP_E_CAPACITY;
    if (!st.records) return 0;
    if (!rank || !length || !symbol || !first) return SUFR_HIP_E_INVALID;
    const int fw = f->meta.index_width;
    parallel_chunks(s, BWT_HOST_TILE, threads, [&](uint64_t b, uint64_t e) {
        const uint64_t t = b / BWT_HOST_TILE;
        uint64_t o = kept[t];
        bwt_host_tile_runs(bwt, b, e, ext[t], [&](uint64_t a, uint64_t len) {
            if (len < min_len) return;
            rank[o] = a; length[o] = len; symbol[o] = bwt[a]; first[o] = rdT(f->sa, fw, a);
            o++;
        });
    });
    return 0;
}

int sufr_file_lf(const sufr_file* f, void* lf, int threads)
{
    if (!f) return SUFR_HIP_E_INVALID;
    const uint64_t s = f->meta.len_suffixes, ntiles = (s + BWT_HOST_TILE - 1) / BWT_HOST_TILE;
    if (!s || !lf) return 0;
    const std::vector<uint8_t> bwt = bwt_host_bytes(*f, threads);
    // a column per byte value that occurs; tab[t K + col]: the tile's count, then C[c] + the ranks of c before the tile
    // (a worker counts and ranks in arrays of its own and touches a row of the table once: neighbouring rows share cache lines)
    uint64_t counts[256] = {0};
    std::mutex mu;
    parallel_chunks(s, BWT_HOST_TILE, threads, [&](uint64_t b, uint64_t e) {
        uint64_t hist[256] = {0};
        for (uint64_t r = b; r < e; r++) hist[bwt[r]]++;
        std::lock_guard<std::mutex> g(mu);
        for (int c = 0; c < 256; c++) counts[c] += hist[c];
    });
    uint32_t col[256], K = 0;
    for (int c = 0; c < 256; c++) col[c] = counts[c] ? K++ : 0;
    std::vector<uint64_t> tab(ntiles * K, 0);
    parallel_chunks(s, BWT_HOST_TILE, threads, [&](uint64_t b, uint64_t e) {
        uint64_t hist[256] = {0};
        for (uint64_t r = b; r < e; r++) hist[bwt[r]]++;
        uint64_t* row = tab.data() + b / BWT_HOST_TILE * K;
        for (int c = 0; c < 256; c++) if (counts[c]) row[col[c]] = hist[c];
    });
    uint64_t below = 0;                                  // C[c]
    for (int c = 0; c < 256; c++) {
        if (!counts[c]) continue;
        uint64_t run = below;
        for (uint64_t t = 0; t < ntiles; t++) { const uint64_t k = tab[t * K + col[c]]; tab[t * K + col[c]] = run; run += k; }
        below += counts[c];
    }
    const int w = f->meta.index_width;
    parallel_chunks(s, BWT_HOST_TILE, threads, [&](uint64_t b, uint64_t e) {
        const uint64_t* row = tab.data() + b / BWT_HOST_TILE * K;
        uint64_t next[256];                              // the rank of the next occurrence of every byte value
        for (int c = 0; c < 256; c++) next[c] = counts[c] ? row[col[c]] : 0;
        for (uint64_t r = b; r < e; r++) kmer_put(lf, w, r, next[bwt[r]]++);
    });
    return 0;
}

}  // extern "C"

// ---- the FM-index over the BWT: backward search and locate without text and suffix array (include/sufr_fm.h, DESIGN.md
// section 23) ---------------------------------------------------------------------------------------------------------
#include "../../include/sufr_fm_approx.h"
#include "../../include/sufr_fm_text.h"
#include "../../include/sufr_fm_match.h"
#include "sufr_fm_host.h"

namespace {

// what sufr_fm_info says of an index of this shape: the blocks, the marks, the kept values, C (257 u64) and the columns (256 u32)
uint64_t fm_bytes(const sufr::FmShape& sh, uint64_t s, uint64_t q, uint64_t samples)
{
    return sufr::fm_blocks(s, sh.B) * sh.stride + (q ? sufr::fm_mark_words(s) * sizeof(sufr::FmMark) + samples * sh.w : 0) + 257 * 8 + 256 * 4;
}

// sufr_file_fm_build_flags (include/sufr_fm_text.h); flags == 0: sufr_file_fm_build
int fm_build_host(const sufr_file* f, uint64_t sample, uint32_t flags, sufr_fm** out, int threads)
{
    if (!f || !out) return SUFR_HIP_E_INVALID;
    *out = nullptr;
    if ((flags & ~SUFR_FM_TEXT) || ((flags & SUFR_FM_TEXT) && !sample)) return SUFR_HIP_E_INVALID;
    const uint64_t s = f->meta.len_suffixes, n = f->meta.text_len;
    if (!n || s != n || f->meta.seed_mask_len || f->meta.max_query_len) return SUFR_HIP_E_UNSUPPORTED;
    const std::vector<uint8_t> bwt = bwt_host_bytes(*f, threads);
    uint64_t counts[256] = {0};
    parallel_chunks(s, BWT_HOST_TILE, threads, [&](uint64_t b, uint64_t e) {
        uint64_t hist[256] = {0};
        for (uint64_t r = b; r < e; r++) hist[bwt[r]]++;
        for (int c = 0; c < 256; c++) if (hist[c]) __atomic_fetch_add(&counts[c], hist[c], __ATOMIC_RELAXED);      // (sums: any order)
    });
    sufr_fm* fm = new sufr_fm;
    fm->s = s; fm->q = sample; fm->e = f->text[n - 1];
    if (counts[fm->e] != 1) { delete fm; return SUFR_HIP_E_UNSUPPORTED; }
    uint32_t K = 0, sym[256];
    for (uint32_t c = 0; c < 256; c++) {
        fm->C[c + 1] = fm->C[c] + counts[c];
        fm->col[c] = counts[c] ? K : sufr::FM_NO_COL;
        if (counts[c]) sym[K++] = c;
    }
    const int w = f->meta.index_width;
    const sufr::FmShape sh = fm->sh = sufr::fm_shape(K, (uint32_t)w);
    // tiles of whole blocks and whole mark words, whatever the number of workers; the last one is short, or empty where s is
    // a multiple of the tile: it holds the trailing block.  tab[t K + k]: the ranks of tile t with byte sym[k], then of all
    // the tiles before it
    const uint64_t tile = sufr::fm_tile(sh.B, BWT_HOST_TILE), ntiles = s / tile + 1, nblocks = sufr::fm_blocks(s, sh.B);
    std::vector<uint64_t> tab(ntiles * K, 0);
    parallel_chunks(ntiles, 1, threads, [&](uint64_t t, uint64_t) {
        uint64_t hist[256] = {0};
        for (uint64_t r = t * tile, end = r + tile < s ? r + tile : s; r < end; r++) hist[bwt[r]]++;
        for (uint32_t k = 0; k < K; k++) tab[t * K + k] = hist[sym[k]];
    });
    for (uint32_t k = 0; k < K; k++) {
        uint64_t run = 0;
        for (uint64_t t = 0; t < ntiles; t++) { const uint64_t v = tab[t * K + k]; tab[t * K + k] = run; run += v; }
    }
    fm->blocks.assign(nblocks * sh.stride, 0);
    parallel_chunks(ntiles, 1, threads, [&](uint64_t t, uint64_t) {
        uint64_t run[256] = {0};                                     // by byte value: the ranks before the block
        for (uint32_t k = 0; k < K; k++) run[sym[k]] = tab[t * K + k];
        const uint64_t j1 = (t + 1) * tile / sh.B < nblocks ? (t + 1) * tile / sh.B : nblocks;
        for (uint64_t j = t * tile / sh.B; j < j1; j++) {
            uint8_t* p = fm->blocks.data() + j * sh.stride;
            for (uint32_t k = 0; k < K; k++) kmer_put(p, w, k, run[sym[k]]);
            const uint64_t b = j * sh.B, len = s - b < sh.B ? s - b : sh.B;
            memcpy(p + sh.cbytes, bwt.data() + b, len);
            for (uint64_t i = 0; i < len; i++) run[bwt[b + i]]++;
        }
    });
    if (sample) {
        const uint64_t nwords = sufr::fm_mark_words(s);
        fm->marks.assign(nwords, sufr::FmMark{0, 0});
        std::vector<uint64_t> kept(ntiles + 1, 0);                   // per tile: the kept ranks, then those of the tiles before it
        parallel_chunks(ntiles, 1, threads, [&](uint64_t t, uint64_t) {
            uint64_t cnt = 0;
            for (uint64_t r = t * tile, end = r + tile < s ? r + tile : s; r < end; r++)
                if (rdT(f->sa, w, r) % sample == 0) { fm->marks[r >> 6].bits |= (uint64_t)1 << (r & 63u); cnt++; }
            kept[t] = cnt;
        });
        for (uint64_t t = 0; t < ntiles; t++) { const uint64_t k = kept[t]; kept[t] = fm->samples; fm->samples += k; }
        fm->kept.assign(fm->samples * w, 0);
        const bool text = flags & SUFR_FM_TEXT;                       // (s == n: the kept positions are 0, q, 2 q, ..: one entry each)
        if (text) fm->text_kept.assign(fm->samples * w, 0);
        parallel_chunks(ntiles, 1, threads, [&](uint64_t t, uint64_t) {
            uint64_t o = kept[t];
            for (uint64_t r = t * tile, end = r + tile < s ? r + tile : s; r < end; r++) {
                if (!(r & 63u)) fm->marks[r >> 6].before = o;
                if (!sufr::fm_marked(fm->marks[r >> 6], r)) continue;
                const uint64_t p = rdT(f->sa, w, r);
                kmer_put(fm->kept.data(), w, o++, p);
                if (text) kmer_put(fm->text_kept.data(), w, p / sample, r);
            }
        });
    }
    fm->seq_starts = f->seq_starts;
    fm->seq_names = f->seq_names;
    *out = fm;
    return 0;
}

}  // namespace

extern "C" {

int sufr_file_fm_build(const sufr_file* f, uint64_t sample, sufr_fm** out, int threads) { return fm_build_host(f, sample, 0, out, threads); }

void sufr_fm_free(sufr_fm* fm) { delete fm; }

int sufr_fm_get_info(const sufr_fm* fm, sufr_fm_info* info)
{
    if (!fm || !info) return SUFR_HIP_E_INVALID;
    *info = sufr_fm_info{fm->s, fm->sh.K, fm->sh.B, fm->sh.stride, fm->q, fm->samples, fm_bytes(fm->sh, fm->s, fm->q, fm->samples), fm->sh.w, fm->e};
    return 0;
}

int sufr_fm_search_batch(const sufr_fm* fm, const uint8_t* queries, const uint64_t* offsets, uint64_t nq, uint64_t* rank_lo, uint64_t* rank_hi,
                         int threads)
{
    if (!fm || (nq && (!offsets || !rank_lo || !rank_hi)) || (nq && offsets[nq] > offsets[0] && !queries)) return SUFR_HIP_E_INVALID;
    for (uint64_t i = 0; i < nq; i++) if (offsets[i + 1] < offsets[i]) return SUFR_HIP_E_INVALID;
    const sufr::FmView V = fm->view();
    parallel_chunks(nq, 256, threads, [&](uint64_t b, uint64_t e) {
        for (uint64_t i = b; i < e; i++) sufr::fm_search(V, queries + offsets[i], offsets[i + 1] - offsets[i], rank_lo[i], rank_hi[i]);
    }, 64);
    return 0;
}

int sufr_fm_locate_batch(const sufr_fm* fm, const uint64_t* rank_lo, const uint64_t* rank_hi, uint64_t nq, uint64_t max_hits, uint64_t* offsets,
                         void* positions, uint64_t cap, uint64_t* total_out, int threads)
{
    if (total_out) *total_out = 0;
    if (!fm || !offsets || (nq && (!rank_lo || !rank_hi))) return SUFR_HIP_E_INVALID;
    if (!fm->q) return SUFR_HIP_E_UNSUPPORTED;
    uint64_t total = 0;
    for (uint64_t i = 0; i < nq; i++) {
        if (rank_lo[i] > rank_hi[i] || rank_hi[i] > fm->s) return SUFR_HIP_E_INVALID;
        const uint64_t hits = rank_hi[i] - rank_lo[i];
        offsets[i] = total;
        total += max_hits && hits > max_hits ? max_hits : hits;
    }
    offsets[nq] = total;
    if (total_out) *total_out = total;
    if (total > cap) return SUFR_HIP_E_CAPACITY;
    if (!total) return 0;
    if (!positions) return SUFR_HIP_E_INVALID;
    const sufr::FmView V = fm->view();
    parallel_chunks(total, 256, threads, [&](uint64_t b, uint64_t e) {
        uint64_t a = query_of(offsets, nq, b);
        for (uint64_t g = b; g < e; g++) {
            while (offsets[a + 1] <= g) a++;
            kmer_put(positions, (int)V.sh.w, g, sufr::fm_position(V, rank_lo[a] + (g - offsets[a])));
        }
    }, 64);
    return 0;
}

}  // extern "C"

// ---- k-mismatch search on the FM-index by backtracking (include/sufr_fm_approx.h)------------------------
namespace {

// What fm_approx_walk asks of the host: begin prepares the step of every column with one fm_occ_all, next tries the columns
// in order, child and a prepared exact step read what begin left
struct FmHostOps {
    const sufr::FmView& V;
    uint32_t sym_of[256];
    uint64_t at_lo[sufr::FM_APPROX_MAX][256], at_hi[sufr::FM_APPROX_MAX][256];      // by depth: occ of every column at lo and at hi
    uint64_t steps = 0;
    explicit FmHostOps(const sufr::FmView& v) : V(v)
    {
        for (uint32_t c = 0; c < 256; c++) if (V.col[c] != sufr::FM_NO_COL) sym_of[V.col[c]] = c;
    }
    uint32_t col(uint32_t c) const { return V.col[c]; }
    uint32_t sym(uint32_t k) const { return sym_of[k]; }
    uint32_t begin(uint32_t h, uint64_t lo, uint64_t hi) { steps++; sufr::fm_occ_all(V, lo, hi, at_lo[h], at_hi[h]); return 0; }
    bool next(uint32_t& state, uint32_t& k, uint64_t, uint64_t) const { k = state; return state < V.sh.K ? (state++, true) : false; }
    void child(uint32_t h, uint32_t c, uint32_t k, uint64_t& a, uint64_t& b) const { a = V.C[c] + at_lo[h][k]; b = V.C[c] + at_hi[h][k]; }
    void exact(uint32_t h, bool prepared, uint32_t c, uint32_t k, uint64_t& a, uint64_t& b)
    {
        if (prepared) { child(h, c, k, a, b); return; }
        steps++;
        a = V.C[c] + sufr::fm_occ(V, c, a);
        b = V.C[c] + sufr::fm_occ(V, c, b);
    }
};

struct FmHostStack {
    sufr::FmFrame fr[sufr::FM_APPROX_MAX];
    void put(uint32_t h, const sufr::FmFrame& f) { fr[h] = f; }
    sufr::FmFrame get(uint32_t h) const { return fr[h]; }
};

int fm_approx_args(const sufr_fm* fm, const uint8_t* queries, const uint64_t* offsets, uint64_t nq, uint32_t d)
{
    if (!fm || (nq && !offsets) || (nq && offsets[nq] > offsets[0] && !queries)) return SUFR_HIP_E_INVALID;
    for (uint64_t i = 0; i < nq; i++) if (offsets[i + 1] < offsets[i]) return SUFR_HIP_E_INVALID;
    if (d > SUFR_FM_APPROX_MAX_MISMATCHES) return SUFR_HIP_E_INVALID;
    return fm->q ? 0 : SUFR_HIP_E_UNSUPPORTED;
}

}  // namespace

extern "C" {

int sufr_fm_approx(const sufr_fm* fm, const uint8_t* queries, const uint64_t* offsets, uint64_t nq, uint32_t max_mismatches, uint32_t flags,
                   uint64_t cap, uint64_t* query, uint8_t* strand, uint64_t* position, uint8_t* mismatches, uint64_t* total_out, int threads)
{
    if (total_out) *total_out = 0;
    if (const int rc = fm_approx_args(fm, queries, offsets, nq, max_mismatches)) return rc;
    if (!nq || offsets[nq] == offsets[0]) return 0;
    const bool both = (flags & SUFR_FM_APPROX_BOTH_STRANDS) != 0;
    std::vector<uint8_t> dbl;
    std::vector<uint64_t> off;
    const uint8_t* qb = strand_batch(queries, offsets, nq, both, dbl, off);
    const uint64_t nq2 = off.size() - 1;
    const sufr::FmView V = fm->view();
    // Two passes of the same walk, as on the device.  Count: the records of every item (hi - lo of its leaves), no position
    // walked and nothing kept; their exclusive scan gives every item its slice and the total, which decides E_CAPACITY before
    // anything is filled.  Fill: every item writes its slice.  Workers take chunks of items in both.
    std::vector<uint64_t> at(nq2 + 1, 0);
    parallel_chunks(nq2, 16, threads, [&](uint64_t b, uint64_t e) {
        FmHostOps ops(V);
        FmHostStack st;
        for (uint64_t a = b; a < e; a++)
            sufr::fm_approx_walk(V, qb + off[a], off[a + 1] - off[a], max_mismatches, ops, st, [&](uint64_t lo, uint64_t hi, uint32_t) { at[a + 1] += hi - lo; });
    }, 4);
    for (uint64_t a = 0; a < nq2; a++) at[a + 1] += at[a];
    const uint64_t total = at[nq2];
    if (total_out) *total_out = total;
    if (total > cap) return SUFR_HIP_E_CAPACITY;
    if (!total) return 0;
    if (!query || !strand || !position || !mismatches) return SUFR_HIP_E_INVALID;
    parallel_chunks(nq2, 16, threads, [&](uint64_t b, uint64_t e) {
        FmHostOps ops(V);
        FmHostStack st;
        for (uint64_t a = b; a < e; a++) {
            if (at[a] == at[a + 1]) continue;
            const QueryStrand qs = query_strand(both, a);
            uint64_t t = at[a];
            sufr::fm_approx_walk(V, qb + off[a], off[a + 1] - off[a], max_mismatches, ops, st, [&](uint64_t lo, uint64_t hi, uint32_t h) {
                for (uint64_t r = lo; r < hi; r++, t++) {
                    query[t] = qs.query; strand[t] = qs.strand; position[t] = sufr::fm_position(V, r); mismatches[t] = (uint8_t)h;
                }
            });
        }
    }, 4);
    return 0;
}

int sufr_fm_approx_steps(const sufr_fm* fm, const uint8_t* queries, const uint64_t* offsets, uint64_t nq, uint32_t max_mismatches, uint32_t flags,
                         uint64_t* leaves, uint64_t* steps, int threads)
{
    if (const int rc = fm_approx_args(fm, queries, offsets, nq, max_mismatches)) return rc;
    if (!nq) return 0;
    if (!leaves || !steps) return SUFR_HIP_E_INVALID;
    const bool both = (flags & SUFR_FM_APPROX_BOTH_STRANDS) != 0;
    std::vector<uint8_t> dbl;
    std::vector<uint64_t> off;
    const uint8_t* qb = strand_batch(queries, offsets, nq, both, dbl, off);
    const sufr::FmView V = fm->view();
    parallel_chunks(off.size() - 1, 16, threads, [&](uint64_t b, uint64_t e) {
        FmHostOps ops(V);
        FmHostStack st;
        for (uint64_t a = b; a < e; a++) {
            ops.steps = leaves[a] = 0;
            sufr::fm_approx_walk(V, qb + off[a], off[a + 1] - off[a], max_mismatches, ops, st, [&](uint64_t, uint64_t, uint32_t) { leaves[a]++; });
            steps[a] = ops.steps;
        }
    }, 4);
    return 0;
}

}  // extern "C"

// ---- the FM-index as a self-contained object: extract, the index file, the sequences (include/sufr_fm_text.h, DESIGN.md
// section 25) ----------------------------------------------------------------------------------------------------------------
namespace {

uint64_t fm_name_bytes(const std::vector<std::string>& names)
{
    uint64_t b = 0;
    for (const std::string& s : names) b += strlen(s.c_str()) + 1;
    return b;
}

// the head of the index file; the rest of its first page is zero
struct FmFileHeader {
    char magic[8];
    uint32_t version, flags, w, e, K, B, stride, cbytes;
    uint64_t s, q, samples, sequences;
    uint64_t sec[2 * sufr::FM_FILE_SECTIONS];            // (offset, length) of every section
};
static_assert(sizeof(FmFileHeader) == 184, "the header of the index file is 184 bytes");
const char FM_FILE_MAGIC[8] = {'S', 'U', 'F', 'R', 'F', 'M', 'I', 0};

sufr::FmFileLayout fm_layout_of(const sufr_fm* fm, uint64_t sequences, uint64_t name_bytes)
{
    return sufr::fm_file_layout(fm->sh, fm->s, fm->q, fm->samples, !fm->text_kept.empty(), sequences, name_bytes);
}

bool fm_starts_fit(const uint64_t* starts, uint64_t num, uint64_t s)
{
    for (uint64_t i = 0; i < num; i++) if (starts[i] >= s || (i && starts[i] < starts[i - 1])) return false;
    return true;
}

// The checks of sufr_fm_load on the arrays of `fm`, whose header fields have been checked: "" or the check that failed
std::string fm_verify(const sufr_fm* fm, bool text, int threads)
{
    const sufr::FmShape sh = fm->sh;
    const uint64_t s = fm->s, q = fm->q;
    uint32_t K = 0, sym[256];
    if (fm->C[0] != 0) return "tables: C[0] is not 0";
    for (uint32_t c = 0; c < 256; c++) {
        if (fm->C[c + 1] < fm->C[c]) return "tables: C decreases at byte value " + std::to_string(c);
        const bool occurs = fm->C[c + 1] > fm->C[c];
        if (fm->col[c] != (occurs ? K : sufr::FM_NO_COL)) return "tables: the column of byte value " + std::to_string(c) + " is not its number among the occurring ones";
        if (occurs) { if (K < 256) sym[K] = c; K++; }
    }
    if (K != sh.K) return "tables: " + std::to_string(K) + " byte values occur, the header says " + std::to_string(sh.K);
    if (fm->C[256] != s) return "tables: C[256] is not the number of ranks";
    if (fm->C[fm->e + 1] - fm->C[fm->e] != 1) return "tables: the end byte does not occur exactly once";
    std::mutex mu;
    std::string bad;
    std::atomic<bool> failed{false};
    auto fail = [&](const std::string& why) {
        std::lock_guard<std::mutex> lock(mu);
        if (bad.empty()) bad = why;
        failed = true;
    };
    // blocks: every checkpoint against the one before it plus the bytes between them, so the tiles are independent
    const uint64_t nblocks = sufr::fm_blocks(s, sh.B);
    parallel_chunks(nblocks, 512, threads, [&](uint64_t b, uint64_t end) {
        uint64_t cnt[256];
        for (uint64_t j = b; j < end && !failed; j++) {
            const uint8_t* p = fm->blocks.data() + j * sh.stride;
            const uint64_t len = s - j * sh.B < sh.B ? s - j * sh.B : sh.B;
            const std::string at = "block " + std::to_string(j);
            for (uint32_t i = K * sh.w; i < sh.cbytes; i++) if (p[i]) return fail("blocks: " + at + " has a non-zero byte behind its checkpoints");
            for (uint32_t k = 0; k < K; k++) cnt[k] = 0;
            for (uint64_t i = 0; i < len; i++) {
                const uint32_t k = fm->col[p[sh.cbytes + i]];
                if (k == sufr::FM_NO_COL) return fail("blocks: " + at + " holds a byte value that has no column");
                cnt[k]++;
            }
            for (uint64_t i = len; i < sh.B; i++) if (p[sh.cbytes + i]) return fail("blocks: " + at + " has a non-zero byte behind the last rank");
            for (uint32_t k = 0; k < K; k++) {
                const uint64_t have = sufr::fm_rd(p + k * sh.w, sh.w);
                if (j == 0 && have != 0) return fail("blocks: a checkpoint of block 0 is not 0");
                const uint64_t next = j + 1 < nblocks ? sufr::fm_rd(p + sh.stride + k * sh.w, sh.w) : fm->C[sym[k] + 1] - fm->C[sym[k]];
                if (have + cnt[k] != next)
                    return fail(j + 1 < nblocks ? "blocks: a checkpoint of block " + std::to_string(j + 1) + " is not the running count"
                                                : std::string("blocks: the final counts are not the differences of C"));
            }
        }
    }, 512);
    if (failed) return bad;
    if (!q) return "";
    const uint64_t nwords = sufr::fm_mark_words(s);
    parallel_chunks(nwords, 4096, threads, [&](uint64_t b, uint64_t end) {
        for (uint64_t i = b; i < end; i++) {
            const sufr::FmMark mk = fm->marks[i];
            const uint64_t next = i + 1 < nwords ? fm->marks[i + 1].before : fm->samples;
            if ((i == 0 && mk.before != 0) || mk.before > next || next - mk.before != (uint64_t)__builtin_popcountll(mk.bits))
                return fail("marks: `before` of word " + std::to_string(i + 1 < nwords ? i + 1 : i) + " is not the running count (the total: the samples)");
            if (i + 1 == nwords && (s & 63u) && (mk.bits >> (s & 63u))) return fail("marks: a bit is set behind the last rank");
        }
    }, 4096);
    if (failed) return bad;
    std::atomic<bool> zero{false};
    parallel_chunks(fm->samples, 4096, threads, [&](uint64_t b, uint64_t end) {
        for (uint64_t i = b; i < end; i++) {
            const uint64_t v = rdT(fm->kept.data(), (int)sh.w, i);
            if (v % q || v >= s) return fail("kept: entry " + std::to_string(i) + " is not a multiple of the sample rate below the number of ranks");
            if (!v) zero = true;
        }
    }, 4096);
    if (failed) return bad;
    if (!zero) return "kept: position 0 is not among the kept values";
    if (!text) return "";
    parallel_chunks(fm->samples, 4096, threads, [&](uint64_t b, uint64_t end) {
        for (uint64_t k = b; k < end; k++) {
            const uint64_t r = rdT(fm->text_kept.data(), (int)sh.w, k);
            if (r >= s || !sufr::fm_marked(fm->marks[r >> 6], r)) return fail("text_kept: entry " + std::to_string(k) + " is not a marked rank");
            if (rdT(fm->kept.data(), (int)sh.w, sufr::fm_slot(fm->marks[r >> 6], r)) != k * q)
                return fail("text_kept: the kept value of entry " + std::to_string(k) + " is not its position");
        }
    }, 4096);
    return failed ? bad : "";
}

}  // namespace

extern "C" {

int sufr_file_fm_build_flags(const sufr_file* f, uint64_t sample, uint32_t flags, sufr_fm** out, int threads)
{
    return fm_build_host(f, sample, flags, out, threads);
}

int sufr_fm_get_text_info(const sufr_fm* fm, sufr_fm_text_info* info)
{
    if (!fm || !info) return SUFR_HIP_E_INVALID;
    const uint64_t ts = fm->text_kept.size() / fm->sh.w;
    *info = sufr_fm_text_info{ts, ts * fm->sh.w, fm_layout_of(fm, fm->seq_starts.size(), fm_name_bytes(fm->seq_names)).bytes};
    return 0;
}

uint64_t sufr_fm_num_sequences(const sufr_fm* fm) { return fm ? fm->seq_starts.size() : 0; }
uint64_t sufr_fm_sequence_start(const sufr_fm* fm, uint64_t i) { return fm && i < fm->seq_starts.size() ? fm->seq_starts[i] : 0; }
const char* sufr_fm_sequence_name(const sufr_fm* fm, uint64_t i) { return fm && i < fm->seq_names.size() ? fm->seq_names[i].c_str() : ""; }

int sufr_fm_set_sequences(sufr_fm* fm, const uint64_t* starts, const char* const* names, uint64_t num)
{
    if (!fm || (num && (!starts || !names)) || !fm_starts_fit(starts, num, fm->s)) return SUFR_HIP_E_INVALID;
    for (uint64_t i = 0; i < num; i++) if (!names[i]) return SUFR_HIP_E_INVALID;
    fm->seq_starts.assign(starts, starts + num);
    fm->seq_names.assign(names, names + num);
    return 0;
}

int sufr_fm_extract_batch(const sufr_fm* fm, const uint64_t* starts, const uint64_t* ends, uint64_t num, uint64_t* offsets, uint8_t* bytes,
                          uint64_t cap, uint64_t* total_out, int threads)
{
    if (total_out) *total_out = 0;
    if (!fm || !offsets || (num && (!starts || !ends))) return SUFR_HIP_E_INVALID;
    if (fm->text_kept.empty()) return SUFR_HIP_E_UNSUPPORTED;
    const uint64_t n = fm->s, q = fm->q;
    std::vector<uint64_t> choff(num + 1);                // the chunks in front of every request
    uint64_t total = 0, chunks = 0;
    for (uint64_t i = 0; i < num; i++) {
        uint64_t a = starts[i], b = ends[i];
        sufr::fm_extract_clip(n, a, b);
        offsets[i] = total;
        choff[i] = chunks;
        total += b - a;
        chunks += sufr::fm_extract_chunks(q, a, b);
    }
    offsets[num] = total;
    choff[num] = chunks;
    if (total_out) *total_out = total;
    if (total > cap) return SUFR_HIP_E_CAPACITY;
    if (!total) return 0;
    if (!bytes) return SUFR_HIP_E_INVALID;
    const sufr::FmView V = fm->view();
    const uint8_t* tk = fm->text_kept.data();
    parallel_chunks(chunks, 64, threads, [&](uint64_t b, uint64_t e) {
        uint64_t i = query_of(choff.data(), num, b);
        for (uint64_t g = b; g < e; g++) {
            while (choff[i + 1] <= g) i++;
            uint64_t lo = starts[i], hi = ends[i];
            sufr::fm_extract_clip(n, lo, hi);
            const uint64_t k = lo / q + (g - choff[i]);
            uint8_t* dst = bytes + offsets[i];
            sufr::fm_extract_chunk(q, n, k, lo, hi, rdT(tk, (int)V.sh.w, sufr::fm_extract_slot(q, n, k)),
                                   [&](uint64_t r, uint32_t& c) { return sufr::fm_lf(V, r, c); },
                                   [&](uint64_t p, uint32_t c) { dst[p - lo] = (uint8_t)c; });
        }
    }, 16);
    return 0;
}

int sufr_fm_save(const sufr_fm* fm, const char* path, const sufr_file* names_from, char* err, size_t errlen)
{
    if (!fm || !path) return SUFR_HIP_E_INVALID;
    const std::vector<uint64_t>& starts = names_from ? names_from->seq_starts : fm->seq_starts;
    const std::vector<std::string>& names = names_from ? names_from->seq_names : fm->seq_names;
    if (starts.size() != names.size() || !fm_starts_fit(starts.data(), starts.size(), fm->s)) {
        put_err(err, errlen, std::string(path) + ": the sequences to store are not those of the indexed text");
        return SUFR_HIP_E_INVALID;
    }
    const sufr::FmFileLayout L = fm_layout_of(fm, starts.size(), fm_name_bytes(names));
    std::vector<uint8_t> tables(sufr::FM_TABLE_BYTES), name_bytes;
    memcpy(tables.data(), fm->C, 257 * 8);
    memcpy(tables.data() + 257 * 8, fm->col, 256 * 4);
    for (const std::string& s : names) name_bytes.insert(name_bytes.end(), s.c_str(), s.c_str() + strlen(s.c_str()) + 1);
    FmFileHeader h{};
    memcpy(h.magic, FM_FILE_MAGIC, 8);
    h.version = 1; h.flags = fm->text_kept.empty() ? 0 : SUFR_FM_TEXT; h.w = fm->sh.w; h.e = fm->e; h.K = fm->sh.K; h.B = fm->sh.B;
    h.stride = fm->sh.stride; h.cbytes = fm->sh.cbytes; h.s = fm->s; h.q = fm->q; h.samples = fm->samples; h.sequences = starts.size();
    for (uint64_t i = 0; i < sufr::FM_FILE_SECTIONS; i++) { h.sec[2 * i] = L.off[i]; h.sec[2 * i + 1] = L.len[i]; }
    const void* data[sufr::FM_FILE_SECTIONS] = {tables.data(), starts.data(), name_bytes.data(), fm->blocks.data(), fm->marks.data(), fm->kept.data(),
                                                fm->text_kept.data()};
    FILE* fp = fopen(path, "wb");
    if (!fp) { put_err(err, errlen, std::string(path) + ": " + strerror(errno)); return SUFR_HIP_E_IO; }
    const std::vector<uint8_t> zeros(sufr::FM_FILE_PAGE, 0);
    uint64_t at = sizeof h;
    bool ok = fwrite(&h, sizeof h, 1, fp) == 1;
    for (uint64_t i = 0; i < sufr::FM_FILE_SECTIONS && ok; i++) {
        ok = fwrite(zeros.data(), 1, L.off[i] - at, fp) == L.off[i] - at && (!L.len[i] || fwrite(data[i], 1, L.len[i], fp) == L.len[i]);
        at = L.off[i] + L.len[i];
    }
    if (fclose(fp) != 0) ok = false;
    if (!ok) { put_err(err, errlen, std::string(path) + ": writing the index file failed: " + strerror(errno)); return SUFR_HIP_E_IO; }
    return 0;
}

int sufr_fm_load(const char* path, sufr_fm** out, int threads, char* err, size_t errlen)
{
    if (!path || !out) return SUFR_HIP_E_INVALID;
    *out = nullptr;
    FILE* fp = fopen(path, "rb");
    struct stat sb;
    if (!fp || fstat(fileno(fp), &sb) != 0) {
        put_err(err, errlen, std::string(path) + ": " + strerror(errno));
        if (fp) fclose(fp);
        return SUFR_HIP_E_IO;
    }
    sufr_fm* fm = nullptr;
    auto fail = [&](int rc, const std::string& why) {
        put_err(err, errlen, std::string(path) + ": " + why);
        fclose(fp);
        delete fm;
        return rc;
    };
    const uint64_t size = (uint64_t)sb.st_size;
    FmFileHeader h;
    if (size < sufr::FM_FILE_PAGE) return fail(SUFR_HIP_E_INVALID, "not an FM-index file (shorter than its header)");
    if (fread(&h, sizeof h, 1, fp) != 1) return fail(SUFR_HIP_E_IO, "reading the header failed");
    if (memcmp(h.magic, FM_FILE_MAGIC, 8) != 0) return fail(SUFR_HIP_E_INVALID, "header: not an FM-index file (wrong magic)");
    if (h.version != 1) return fail(SUFR_HIP_E_INVALID, "header: version " + std::to_string(h.version) + ", this library reads version 1");
    if (h.flags & ~SUFR_FM_TEXT) return fail(SUFR_HIP_E_INVALID, "header: unknown flags");
    const bool text = h.flags & SUFR_FM_TEXT;
    if (h.w != 4 && h.w != 8) return fail(SUFR_HIP_E_INVALID, "header: the index width is neither 4 nor 8");
    if (h.K < 1 || h.K > 256 || h.e > 255) return fail(SUFR_HIP_E_INVALID, "header: the number of byte values or the end byte is out of range");
    const sufr::FmShape sh = sufr::fm_shape(h.K, h.w);
    if (h.B != sh.B || h.stride != sh.stride || h.cbytes != sh.cbytes) return fail(SUFR_HIP_E_INVALID, "header: the block shape is not that of K and w");
    if (!h.s || h.s > size || (h.w == 4 && h.s > 0xFFFFFFFFull)) return fail(SUFR_HIP_E_INVALID, "header: the number of ranks does not fit the file or the width");
    if (h.samples != (h.q ? (h.s - 1) / h.q + 1 : 0) || (text && !h.q)) return fail(SUFR_HIP_E_INVALID, "header: the number of samples is not ceil(s / q)");
    const uint64_t name_len = h.sec[2 * sufr::FM_SEC_NAMES + 1];
    if (h.sequences > size / 8 || name_len > size) return fail(SUFR_HIP_E_INVALID, "header: the sequences do not fit the file");
    const sufr::FmFileLayout L = sufr::fm_file_layout(sh, h.s, h.q, h.samples, text, h.sequences, name_len);
    for (uint64_t i = 0; i < sufr::FM_FILE_SECTIONS; i++)
        if (h.sec[2 * i] != L.off[i] || h.sec[2 * i + 1] != L.len[i])
            return fail(SUFR_HIP_E_INVALID, "header: section " + std::to_string(i) + " is not where or as long as its formula says");
    if (L.bytes != size) return fail(SUFR_HIP_E_INVALID, "header: the file is " + std::to_string(size) + " bytes long, its sections end at " + std::to_string(L.bytes));
    fm = new sufr_fm;
    fm->sh = sh; fm->s = h.s; fm->q = h.q; fm->samples = h.samples; fm->e = h.e;
    std::vector<uint8_t> tables(sufr::FM_TABLE_BYTES), name_bytes(name_len);
    fm->seq_starts.resize(h.sequences);
    fm->blocks.resize(L.len[sufr::FM_SEC_BLOCKS]);
    fm->marks.resize(L.len[sufr::FM_SEC_MARKS] / sizeof(sufr::FmMark));
    fm->kept.resize(L.len[sufr::FM_SEC_KEPT]);
    fm->text_kept.resize(L.len[sufr::FM_SEC_TEXT]);
    void* data[sufr::FM_FILE_SECTIONS] = {tables.data(), fm->seq_starts.data(), name_bytes.data(), fm->blocks.data(), fm->marks.data(), fm->kept.data(),
                                          fm->text_kept.data()};
    for (uint64_t i = 0; i < sufr::FM_FILE_SECTIONS; i++)
        if (L.len[i] && (fseeko(fp, (off_t)L.off[i], SEEK_SET) != 0 || fread(data[i], 1, L.len[i], fp) != L.len[i]))
            return fail(SUFR_HIP_E_IO, "reading section " + std::to_string(i) + " failed");
    memcpy(fm->C, tables.data(), 257 * 8);
    memcpy(fm->col, tables.data() + 257 * 8, 256 * 4);
    if (!fm_starts_fit(fm->seq_starts.data(), h.sequences, h.s)) return fail(SUFR_HIP_E_INVALID, "sequences: the starts decrease or lie behind the text");
    for (uint64_t at = 0; at < name_len;) {
        const void* z = memchr(name_bytes.data() + at, 0, name_len - at);
        if (!z) return fail(SUFR_HIP_E_INVALID, "sequences: the last name does not end");
        fm->seq_names.emplace_back((const char*)name_bytes.data() + at);
        at = (uint64_t)((const uint8_t*)z - name_bytes.data()) + 1;
    }
    if (fm->seq_names.size() != h.sequences) return fail(SUFR_HIP_E_INVALID, "sequences: the names are not one per start");
    const std::string bad = fm_verify(fm, text, threads);
    if (!bad.empty()) return fail(SUFR_HIP_E_INVALID, bad);
    fclose(fp);
    *out = fm;
    return 0;
}

}  // extern "C"

// ---- matching statistics and SMEMs on a pair of indexes (include/sufr_fm_match.h) -----------------------
namespace {

// C and the columns of the pair, which agree (sufr_fm_pair_check), read from the index of the text
struct FmHostTab {
    const sufr::FmView& V;
    uint32_t col(uint32_t c) const { return V.col[c]; }
    uint64_t C(uint32_t c) const { return V.C[c]; }
};

void fm_host_step(const sufr::FmView& V, uint32_t c, uint32_t, uint64_t& a, uint64_t& b)
{
    a = V.C[c] + sufr::fm_occ(V, c, a);
    b = V.C[c] + sufr::fm_occ(V, c, b);
}

int fm_match_args(const sufr_fm* fwd, const sufr_fm* rev, const uint8_t* queries, const uint64_t* offsets, uint64_t nq)
{
    if (!fwd || !rev || (nq && !offsets) || (nq && offsets[nq] > offsets[0] && !queries)) return SUFR_HIP_E_INVALID;
    for (uint64_t i = 0; i < nq; i++) if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > 0xFFFFFFFFull) return SUFR_HIP_E_INVALID;
    return sufr_fm_pair_check(fwd, rev);
}

// The bytes of a piece of the batch that one call of a worker takes.  SUFR_FM_MS_HOST_SLAB sets it for the tests of the
// cuts; no result depends on it (fact (a) of the header)
uint64_t fm_ms_host_slab()
{
    const char* v = getenv("SUFR_FM_MS_HOST_SLAB");
    const long long k = v ? atoll(v) : 0;
    return k > 0 ? (uint64_t)k : 4096;
}

// ms[g - base] for every byte g of the batch: workers take slabs of the concatenated bytes, and in a slab the part of every
// query that it touches is one fm_ms_walk
void fm_ms_batch(const sufr_fm* fwd, const sufr_fm* rev, const uint8_t* queries, const uint64_t* offsets, uint64_t nq, int threads, uint32_t* ms,
                 uint64_t base)
{
    const sufr::FmView F = fwd->view(), R = rev->view();
    const FmHostTab tab{F};
    const uint64_t g0 = offsets[0];
    parallel_chunks(offsets[nq] - g0, fm_ms_host_slab(), threads, [&](uint64_t b, uint64_t e) {
        uint64_t a = query_of(offsets, nq, g0 + b);
        for (uint64_t g = g0 + b; g < g0 + e;) {
            while (offsets[a + 1] <= g) a++;
            const uint64_t qb = offsets[a], qe = offsets[a + 1], pe = qe < g0 + e ? qe : g0 + e;
            uint32_t* out = ms + (qb - base);
            sufr::fm_ms_walk(F, R, tab, queries + qb, qe - qb, g - qb, pe - qb, fm_host_step, [&](uint64_t j, uint32_t v) { out[j] = v; });
            g = pe;
        }
    });
}

}  // namespace

extern "C" {

int sufr_fm_pair_check(const sufr_fm* fwd, const sufr_fm* rev)
{
    if (!fwd || !rev) return SUFR_HIP_E_INVALID;
    const bool same = fwd->s == rev->s && fwd->sh.w == rev->sh.w && fwd->e == rev->e && !memcmp(fwd->col, rev->col, sizeof fwd->col) &&
                      !memcmp(fwd->C, rev->C, sizeof fwd->C);
    return same ? 0 : SUFR_HIP_E_INVALID;
}

int sufr_fm_matching_stats(const sufr_fm* fwd, const sufr_fm* rev, const uint8_t* queries, const uint64_t* offsets, uint64_t nq, uint32_t* ms,
                           int threads)
{
    if (const int rc = fm_match_args(fwd, rev, queries, offsets, nq)) return rc;
    if (!nq || offsets[nq] == offsets[0]) return 0;
    if (!ms) return SUFR_HIP_E_INVALID;
    fm_ms_batch(fwd, rev, queries, offsets, nq, threads, ms, 0);
    return 0;
}

int sufr_fm_smems(const sufr_fm* fwd, const sufr_fm* rev, const uint8_t* queries, const uint64_t* offsets, uint64_t nq, uint32_t min_len,
                  uint64_t cap, uint64_t* query, uint32_t* qoff, uint32_t* len, uint64_t* rank_lo, uint64_t* rank_hi, uint64_t* total_out,
                  int threads)
{
    if (total_out) *total_out = 0;
    if (const int rc = fm_match_args(fwd, rev, queries, offsets, nq)) return rc;
    if (min_len == 0) return SUFR_HIP_E_INVALID;
    if (!nq || offsets[nq] == offsets[0]) return 0;
    const uint64_t g0 = offsets[0];
    std::vector<uint32_t> ms(offsets[nq] - g0);
    fm_ms_batch(fwd, rev, queries, offsets, nq, threads, ms.data(), g0);
    uint64_t total = 0;
    if (const int rc = smem_records(ms.data(), g0, offsets, nq, min_len, cap, query, qoff, len, rank_lo, rank_hi, total, total_out)) return rc;
    if (!total) return 0;
    // the rank range of every SMEM: the backward search of its slice on the index of the text
    const sufr::FmView F = fwd->view();
    parallel_chunks(total, 256, threads, [&](uint64_t b, uint64_t e) {
        for (uint64_t k = b; k < e; k++) sufr::fm_search(F, queries + offsets[query[k]] + qoff[k], len[k], rank_lo[k], rank_hi[k]);
    }, 64);
    return 0;
}

int sufr_fm_matching_stats_steps(const sufr_fm* fwd, const sufr_fm* rev, const uint8_t* queries, const uint64_t* offsets, uint64_t nq,
                                 uint64_t* steps, int threads)
{
    if (const int rc = fm_match_args(fwd, rev, queries, offsets, nq)) return rc;
    if (!nq) return 0;
    if (!steps) return SUFR_HIP_E_INVALID;
    const sufr::FmView F = fwd->view(), R = rev->view();
    const FmHostTab tab{F};
    parallel_chunks(nq, 16, threads, [&](uint64_t b, uint64_t e) {
        for (uint64_t i = b; i < e; i++)
            steps[i] = sufr::fm_ms_walk(F, R, tab, queries + offsets[i], offsets[i + 1] - offsets[i], 0, offsets[i + 1] - offsets[i], fm_host_step,
                                        [](uint64_t, uint32_t) {});
    }, 4);
    return 0;
}

int sufr_file_write_reversed_fasta(const sufr_file* f, const char* path, char* err, size_t errlen)
{
    if (!f || !path) return SUFR_HIP_E_INVALID;
    const uint64_t n = f->meta.text_len, k = f->seq_starts.size();
    if (!n) { put_err(err, errlen, "the file holds no text"); return SUFR_HIP_E_INVALID; }
    FILE* fp = fopen(path, "wb");
    if (!fp) { put_err(err, errlen, std::string(path) + ": " + strerror(errno)); return SUFR_HIP_E_IO; }
    // sequence i is T[starts[i] .. the delimiter in front of starts[i + 1]), the last one ends in front of the end byte
    std::vector<uint8_t> line;
    bool ok = true;
    for (uint64_t i = k; i-- > 0 && ok;) {
        const uint64_t b = f->seq_starts[i], e = i + 1 < k ? f->seq_starts[i + 1] - 1 : n - 1;
        line.assign(1, (uint8_t)'>');
        line.insert(line.end(), f->seq_names[i].begin(), f->seq_names[i].end());
        line.push_back((uint8_t)'\n');
        for (uint64_t p = e; p-- > b;) line.push_back(f->text[p]);
        if (e > b) line.push_back((uint8_t)'\n');
        ok = fwrite(line.data(), 1, line.size(), fp) == line.size();
    }
    if (fclose(fp) != 0) ok = false;
    if (!ok) { put_err(err, errlen, std::string(path) + ": write failed"); return SUFR_HIP_E_IO; }
    return 0;
}

}  // extern "C"
