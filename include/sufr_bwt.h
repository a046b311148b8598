/*
 * sufr_bwt.h -- the Burrows-Wheeler transform of the indexed text, its equal-letter runs and the LF mapping, from the suffix
 * array and the text alone; on the host and on the GPU (part of libsufr_hip.so).  The other analyses
 * (sufr_kmer.h, sufr_repeat.h, sufr_lz.h, sufr_shared.h) read SA + LCP; this header is the hand-over to FM-index tools,
 * run-length indexes and compressors: the arrays they are made of, and r, the number of runs, beside the z of sufr_lz.h.
 * The library's own FM-index over these arrays, with backward search and locate, is sufr_fm.h.
 *
 * Definitions.  T, n, SA[0..s) and the index width w are exactly as in sufr_kmer.h.  No LCP array and no sequence starts
 * are needed; nothing here assumes that SA is sorted, only that its entries are text positions.
 *   BWT[r] = T[SA[r] - 1], and T[n - 1] where SA[r] == 0 (cyclic): s bytes in rank order.  It is defined for every index,
 *         partial ones included (--dna without --allow-ambiguity, soft-mask, seed mask, --max-query-len): "the byte in front
 *         of every indexed suffix".
 *   counts[c], c < 256: the number of ranks with BWT[r] == c.  C[c]: the sum of counts[c'] over c' < c.
 *   Run       a maximal rank range [a, b) of equal BWT bytes.
 *   Records   four parallel arrays of `cap` entries, u64 for both index widths, in ascending rank: rank = a, length = b - a,
 *         symbol = the byte, first = SA[a].  Kept where length >= min_len; a min_len of 0 counts as 1.  *total_out always
 *         receives the number of kept records; when it exceeds cap the call returns SUFR_HIP_E_CAPACITY and fills nothing
 *         (the rule of sufr_lz.h).  cap == 0 with NULL arrays is a counting call.
 *   Stats     runs (= r, over all runs, whatever the filter); records (the kept ones); longest and longest_rank, the length
 *         and first rank of the longest run, ties to the smallest rank.  All zero for s == 0.
 *   LF[r] = C[BWT[r]] + #{ j < r : BWT[j] == BWT[r] }: s entries of the index width, a permutation of [0, s) -- the stable
 *         rank of every BWT symbol.  It is defined from the BWT alone, so it is valid on every index.
 *         Text-level meaning   where every position is indexed (s == n), the order is exact (no seed mask, no max_query_len)
 *         and the final '$' occurs once, SA[LF[r]] = (SA[r] - 1) mod n: LF walks the text backwards without the SA.
 *
 * Refusals.  None: every file and every index is a valid input.  An empty array (s == 0) is a valid call: empty outputs,
 * zero counts and zero stats.  NULL outputs are skipped.
 */
#ifndef SUFR_BWT_H
#define SUFR_BWT_H
#include <stddef.h>
#include <stdint.h>

#include "sufr_query.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sufr_bwt_stats { uint64_t runs, records, longest, longest_rank; } sufr_bwt_stats;

/* ---- host: `threads` workers (0: one per core) over rank ranges of the mapped arrays; the results do not depend on the
 * number of workers.  bwt: s bytes; counts: 256 entries; either may be NULL. */
int sufr_file_bwt(const sufr_file *f, uint8_t *bwt /* s */, uint64_t *counts /* 256 */, int threads);
/* rank, length, symbol, first: cap entries each (NULL with cap == 0); total_out and stats may be NULL. */
int sufr_file_bwt_runs(const sufr_file *f, uint64_t min_len, uint64_t cap, uint64_t *rank, uint64_t *length, uint64_t *symbol,
                       uint64_t *first, uint64_t *total_out, sufr_bwt_stats *stats, int threads);
/* lf: s entries of the file's index width (4 or 8 bytes). */
int sufr_file_lf(const sufr_file *f, void *lf /* s entries of the index width */, int threads);

/* ---- device: the index of sufr_hip_index_load / sufr_hip_index_wrap (its text, SA, n and s), with 32- or 64-bit entries.
 * d_bwt: s bytes on the device at an address that is a multiple of 4; d_counts: 256 u64 on the device; either may be NULL.
 * Enqueued only, on the context's stream (complete after sufr_hip_synchronize). */
int sufr_hip_bwt_device(sufr_hip_ctx *ctx, const sufr_hip_index *ix, void *d_bwt, void *d_counts /* 256 u64 */);
/* d_rank, d_length, d_symbol, d_first: cap u64 each on the device.  The BWT goes to scratch of the context; the gather, the
 * sweep over the tile summaries and a counting pass leave the total and the stats; the call synchronises once, for them, and
 * then enqueues the writing pass on the context's stream (complete after sufr_hip_synchronize).  Entries beyond the total
 * are not written. */
int sufr_hip_bwt_runs_device(sufr_hip_ctx *ctx, const sufr_hip_index *ix, uint64_t min_len, uint64_t cap, void *d_rank, void *d_length,
                             void *d_symbol, void *d_first, uint64_t *total_out, sufr_bwt_stats *stats_out);
/* d_lf: s entries of the index width on the device.  The call synchronises once, for the byte counts, which size the table
 * of the tiles' bases (one column per byte value that occurs); the ranking is enqueued on the context's stream (complete
 * after sufr_hip_synchronize).  The result is the same bits on every run. */
int sufr_hip_lf_device(sufr_hip_ctx *ctx, const sufr_hip_index *ix, void *d_lf);
/* Ranks one workgroup takes at a time in all three (0: the default, 16384): rounded up to the workgroup size, 256, and held
 * to 16384 at most.  It changes no result; small tiles put many tile boundaries into small arrays. */
int sufr_hip_set_bwt_tile(sufr_hip_ctx *ctx, uint64_t ranks);   /* 0: default 16384; rounded up to 256, at most 16384 */

#ifdef __cplusplus
}
#endif
#endif /* SUFR_BWT_H */
