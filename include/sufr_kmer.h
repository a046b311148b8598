/*
 * sufr_kmer.h -- what the suffix array and the LCP array say about the indexed text itself: the k-mer spectrum, the
 * occurrence count of the k-mer at every rank or position, and the length at which the substring at every rank or position
 * becomes unique; on the host and on the GPU (part of libsufr_hip.so).  Single passes over SA and LCP:
 * no text access, no search.
 *
 * Definitions.
 *   Text and arrays   T is the text, n bytes.  SA[0..s) are the indexed positions in suffix order, LCP[0..s) is as in the
 *         file: LCP[0] = 0, otherwise the exact common prefix of SA[r-1] and SA[r]; LCP[s] := 0.  w is the index width, 4 or
 *         8 bytes: LCP and every per-rank or per-position output have width w.
 *   Breaks   the positions a k-mer may not contain: the last position n-1 (the '$'), and start_i - 1 for every sequence
 *         i >= 1 (the delimiter in front of it).  Breaks are positional, taken from the sequence starts, never from byte
 *         values.  brk(p) is the smallest break >= p.
 *   Whole    for k >= 1, position p is whole iff p + k <= brk(p).  A position that is itself a break is never whole.
 *   Interval a k-interval is a maximal rank range [a, b) with LCP[r] >= k for all a < r < b.
 *   Count    occ_k(r), the count of rank r, is 0 if SA[r] is not whole, otherwise the number of whole ranks in the
 *         k-interval of r.  It is defined per rank: a text whose delimiter byte also occurs inside sequences needs no rule
 *         of its own.
 *   Spectrum each k-interval with c >= 1 whole ranks is one distinct k-mer of count c.  For bins >= 1: hist[i], i < bins-1,
 *         is the number of distinct k-mers of count i+1; hist[bins-1] the number of count >= bins;
 *         stats = {whole = sum of c, distinct, unique = #(c == 1), max_count}.
 *   Unique length   u = 1 + max(LCP[r], LCP[r+1]); ul(r) = u if SA[r] + u <= brk(SA[r]), else 0: no substring that starts
 *         here is unique inside its sequence.
 *   SUFR_KMER_BY_POSITION   the output has n entries of width w: entry SA[r] holds the value of rank r, every unindexed
 *         position holds 0.  Without the flag it has s entries in rank order, parallel to SA.
 * Scope.  Counts are over INDEXED positions: an occurrence of a k-mer at a position the array leaves out (the Ns of a --dna
 * build, soft-masked stretches) is not counted.  Filtering by byte class (k-mers that contain N) is not done here.
 *
 * Refusals.  A seed-mask file or index: SUFR_HIP_E_UNSUPPORTED.  A build with max_query_len L > 0 has its LCP capped at L:
 * k <= L stays exact, k > L and unique lengths at all are SUFR_HIP_E_UNSUPPORTED.  k == 0, and bins == 0 with a histogram
 * asked for: SUFR_HIP_E_INVALID.  Sequence starts that do not ascend, do not begin at 0 or reach n: SUFR_HIP_E_INVALID.  An
 * empty array (s == 0) is a valid call: the histogram and the stats are all zero.
 */
#ifndef SUFR_KMER_H
#define SUFR_KMER_H
#include <stddef.h>
#include <stdint.h>

#include "sufr_query.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sufr_kmer_stats { uint64_t whole, distinct, unique, max_count; } sufr_kmer_stats;
#define SUFR_KMER_BY_POSITION 0x1u

/* ---- host: `threads` workers (0: one per core) over the mapped arrays; the sequence starts come from the file -------
 * hist (bins u64), occ (s or n entries of the file's index width) and stats may each be NULL. */
int sufr_file_kmers(const sufr_file *f, uint64_t k, uint32_t flags, uint64_t bins, uint64_t *hist, void *occ,
                    sufr_kmer_stats *stats, int threads);
int sufr_file_unique_lengths(const sufr_file *f, uint32_t flags, void *out, int threads);

/* ---- device: the index of sufr_hip_index_load / sufr_hip_index_wrap (its SA, n, s and build cap; the text is not read) --
 * d_lcp: s entries of the index's width (sufr_hip_index_width), e.g. what sufr_hip_sort_device_u32 left next to the SA.
 * seq_starts: a HOST array of num_sequences u64 (NULL / 0: one sequence).  d_hist: bins u64; d_occ / d_out: s or n entries
 * of the index's width; d_hist, d_occ and stats_out may each be NULL.
 * _kmers_device: a memset of d_hist, the fold (one pass over SA and LCP that leaves two bits per rank and a summary per
 * tile), the carry (one workgroup), the apply (one pass over the bits that writes d_occ and the histogram); with
 * SUFR_KMER_BY_POSITION a memset of d_occ comes first and the apply scatters through SA.  It synchronises once when
 * stats_out is given and otherwise only enqueues on the context's stream (complete after sufr_hip_synchronize).
 * _unique_lengths_device: one elementwise launch (after a memset with SUFR_KMER_BY_POSITION), enqueued only.
 * Both copy the sequence starts to the context when there are several; a call whose starts differ from those of the
 * context's previous call waits for that call first. */
int sufr_hip_kmers_device(sufr_hip_ctx *ctx, const sufr_hip_index *ix, const void *d_lcp, const uint64_t *seq_starts,
                          uint64_t num_sequences, uint64_t k, uint32_t flags, uint64_t bins, void *d_hist /* bins u64 */,
                          void *d_occ, sufr_kmer_stats *stats_out);
int sufr_hip_unique_lengths_device(sufr_hip_ctx *ctx, const sufr_hip_index *ix, const void *d_lcp,
                                   const uint64_t *seq_starts, uint64_t num_sequences, uint32_t flags, void *d_out);
/* Ranks one workgroup folds at a time (0: the default, 16384): rounded up to the workgroup size, 256, and held to 16384
 * at most.  It changes no result; small tiles put many tile boundaries into small arrays. */
int sufr_hip_set_kmer_tile(sufr_hip_ctx *ctx, uint64_t ranks);

#ifdef __cplusplus
}
#endif
#endif /* SUFR_KMER_H */
