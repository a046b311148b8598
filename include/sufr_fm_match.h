/*
 * sufr_fm_match.h -- matching statistics and super-maximal exact matches (SMEMs) of query batches on the FM-index alone: two
 * indexes of sufr_fm.h, one of the text and one of its reversal, and neither text nor suffix array in memory (part of
 * libsufr_hip.so).  T, n, s == n, e = T[n - 1], C, occ, w and K are exactly as in sufr_fm.h.
 *
 * Definitions.
 *   X = T[0 .. n - 1)           the text without its end byte.
 *   R = reverse(X) + e          the reversed text.
 *   fwd                         an FM-index of T.
 *   rev                         an FM-index of R at any sample rate, 0 included: it is never asked to locate.  A backward
 *         search on rev is a forward extension in the text.  Built with sample == 0 it takes 1.33 bytes per rank at DNA and
 *         32-bit positions; the pair takes 3.04 with every 32nd suffix of fwd kept.
 *   The reversed text as a FASTA.  For T = S1 % S2 % .. Sk e, R is the text of the FASTA that holds Sk^R, .., S1^R: every
 *         sequence reversed and the order of the sequences reversed, each under its own name, created with the flags that the
 *         forward file records.  sufr_file_write_reversed_fasta writes that file.
 *   Pair check.  fwd and rev must agree in ranks, width, end_byte, the byte values that occur and C[0..256]; anything else is
 *         SUFR_HIP_E_INVALID, on the device with the message "not an index of the reversed text".  The check is necessary,
 *         not sufficient: two indexes of different texts with equal byte counts pass it and give wrong answers.  They never
 *         read outside their arrays, since each index is valid alone, and every walk ends.  Producing the right pair is the
 *         job of sufr_file_write_reversed_fasta.
 *   Matching statistics.  For a query Q[0..m), ms[j] is the largest l <= m - j such that Q[j .. j + l) occurs in X.  A query
 *         byte equal to e matches nothing and no match crosses it; a byte that does not occur in the text behaves the same
 *         way.  For every query without the byte e this is sufr_file_matching_stats (sufr_match.h) on a file without
 *         max_query_len.  Batches have the layout of sufr_match.h: ms[offsets[i] + j]; a query is at most 2^32 - 1 bytes.
 *   SMEMs.  The rule of sufr_match.h: offset j starts one iff ms[j] >= min_len and (j == 0 or ms[j-1] <= ms[j]).  Records are
 *         (query, offset, length, rank_lo, rank_hi) in (query, offset) order, the range that of sufr_fm_search_batch on fwd
 *         for the slice.  min_len == 0 is SUFR_HIP_E_INVALID.  *total_out is always the count; over `cap` the call returns
 *         SUFR_HIP_E_CAPACITY and fills nothing.  The positions of an SMEM come from sufr_fm_locate_batch on fwd.
 *
 * The walk.  Let x = m - 1.  While x >= 0:
 *   1. Extend forwards from x on rev: start at [C[c], C[c + 1]) for c = Q[x], then step with Q[x + 1], Q[x + 2], .. until the
 *      range is empty or the query ends.  This gives l = ms[x].
 *   2. If l == 0, set x -= 1 and continue.
 *   3. Otherwise let end = x + l.  Search backwards from end on fwd with Q[end - 1], Q[end - 2], .. until the range is empty or
 *      the query begins.  This gives start <= x.
 *   4. Set ms[j] = end - j for j = start .. x.
 *   5. Set x = start - 1.
 * Two facts make this the whole algorithm.
 *   (a) Started from any x, the values the walk writes are correct: Q[j..end) occurs as a part of Q[start..end), and
 *       Q[j..end + 1) does not occur because Q[x..end + 1) does not.  So a query may be cut anywhere and each piece walked on
 *       its own: a piece that owns the offsets [a, b) starts at x = b - 1, stops its searches back at a, and writes only its
 *       own offsets.  ms is a function of the input, not of the cut, the number of workers or the slab of a GPU lane.
 *   (b) [start, end) is an SMEM, and no SMEM with a start in (start, x] exists, so nothing is skipped -- also where three or
 *       more SMEMs cover one query position.
 * Cost of a cut.  A piece that owns [a, b) pays its extension from b - 1, ms[b - 1] steps, and a search back of as many plus
 * b - a.  The host cuts at 4096 bytes; the device gives every lane 32.  A query that matches the text over a long stretch
 * therefore costs the device (m / 32) * ms steps, with up to 2 ms dependent steps in one lane: a query of a million bytes that
 * occurs whole is about 3e10 steps in one launch.  Callers with such queries (whole chromosomes against themselves, long runs
 * of one letter) should use sufr_match.h or the host path until a piece hands its extension on to its neighbour.
 * A step moves one range by one byte (two occ).  The whole-query walk takes at most 2 * (the summed lengths of the SMEMs at
 * min_len 1) + 2 m steps; sufr_fm_matching_stats_steps reports the number for every query.
 */
#ifndef SUFR_FM_MATCH_H
#define SUFR_FM_MATCH_H
#include <stddef.h>
#include <stdint.h>

#include "sufr_fm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- host.  `threads` as in sufr_fm.h: workers take pieces of the concatenated batch, whole queries and slabs of a long
 * one; no result depends on their number. */
int sufr_fm_pair_check(const sufr_fm *fwd, const sufr_fm *rev);
/* ms: offsets[num_queries] u32, as sufr_file_matching_stats fills them */
int sufr_fm_matching_stats(const sufr_fm *fwd, const sufr_fm *rev, const uint8_t *queries, const uint64_t *offsets,
                           uint64_t num_queries, uint32_t *ms, int threads);
int sufr_fm_smems(const sufr_fm *fwd, const sufr_fm *rev, const uint8_t *queries, const uint64_t *offsets, uint64_t num_queries,
                  uint32_t min_len, uint64_t cap, uint64_t *query, uint32_t *query_offset, uint32_t *length, uint64_t *rank_lo,
                  uint64_t *rank_hi, uint64_t *total_out, int threads);
/* for measurement: steps[i] = the steps of the whole-query walk of query i (num_queries u64) */
int sufr_fm_matching_stats_steps(const sufr_fm *fwd, const sufr_fm *rev, const uint8_t *queries, const uint64_t *offsets,
                                 uint64_t num_queries, uint64_t *steps, int threads);
/* The FASTA of the reversed text of an open .sufr (above).  Files with a seed mask, a max_query_len or positions left out
 * are written all the same: the file holds the text, not the index. */
int sufr_file_write_reversed_fasta(const sufr_file *f, const char *path, char *err, size_t errlen);

/* ---- device: fwd and rev live on the device of `ctx`.
 * _matching_stats_device only enqueues on the context's stream; d_ms holds offsets[num_queries] u32 entries.
 * _smems_device computes the statistics into d_ms (same size; the caller's scratch, it receives them), flags the SMEMs with
 * the kernels of sufr_hip_smems_device, synchronises once to read their total, then enqueues the records and their rank
 * ranges (sufr_hip_fm_search_batch_device on fwd over the SMEM slices) without further synchronisation.
 * _smems takes host buffers and returns when the records are there. */
int sufr_hip_fm_matching_stats_device(sufr_hip_ctx *ctx, const sufr_hip_fm *fwd, const sufr_hip_fm *rev, const void *d_queries,
                                      const void *d_offsets, uint64_t num_queries, void *d_ms);
int sufr_hip_fm_smems_device(sufr_hip_ctx *ctx, const sufr_hip_fm *fwd, const sufr_hip_fm *rev, const void *d_queries,
                             const void *d_offsets, uint64_t num_queries, uint32_t min_len, void *d_ms, uint64_t cap, void *d_query,
                             void *d_query_offset, void *d_length, void *d_rank_lo, void *d_rank_hi, uint64_t *total_out);
int sufr_hip_fm_smems(sufr_hip_ctx *ctx, const sufr_hip_fm *fwd, const sufr_hip_fm *rev, const uint8_t *queries,
                      const uint64_t *offsets, uint64_t num_queries, uint32_t min_len, uint64_t cap, uint64_t *query,
                      uint32_t *query_offset, uint32_t *length, uint64_t *rank_lo, uint64_t *rank_hi, uint64_t *total_out);

#ifdef __cplusplus
}
#endif
#endif /* SUFR_FM_MATCH_H */
