/*
 * sufr_shared.h -- the repeats of a collection with the number of different sequences each occurs in, and the longest
 * substring common to at least q of the sequences for every q (Gusfield's k-common substrings), from the suffix array, the
 * LCP array and the sequence starts; on the host and on the GPU (part of libsufr_hip.so).  It is
 * sufr_repeat.h with one more column: `count` says how often a repeat occurs, `seqs` in how many sequences -- what tells a
 * repeat found 40 times in one chromosome from one found once in each of 40.
 *
 * Definitions.  T, n, SA[0..s), LCP, w, breaks, brk(p), d(p), the clipped l, intervals [a, b) of value v, representatives,
 * lambda and the three kinds are exactly those of sufr_repeat.h; nothing is redefined.
 *   Sequence of a position   doc(p) is the index of the last sequence start <= p (a break belongs to the sequence it ends).
 *         D[r] = doc(SA[r]).
 *   Sequence count   seqs([a, b)) = |{ D[r] : a <= r < b }|, so 1 <= seqs <= min(count, num_sequences).  Where the delimiter
 *         byte occurs only at breaks this is the number of sequences in which the record's string has an indexed occurrence;
 *         otherwise the array definition stands, as in sufr_repeat.h.
 *   Previous rank   prev[r] is the largest j < r with D[j] == D[r]; it may be absent.
 *   The identity   for every r that has a prev[r] let m = min l(prev[r], r] and q(r) the smallest j in (prev[r], r] with
 *         l[j] == m.  H[j] = |{ r : q(r) = j }|, P the exclusive prefix sum of H with P[s] the total.  Then for every
 *         interval
 *                 seqs([a, b)) = (b - a) - (P[b] - P[a + 1]).
 *         A pair (prev[r], r) lies inside [a, b) exactly when q(r) lies in (a, b): if q is in (a, b) then l[q] >= v, and
 *         were prev[r] < a or r >= b the pair's range (prev[r], r] would hold a or b, where l < v <= m, against m being its
 *         minimum; the converse is immediate.  The ranks of [a, b) that are not the first of their sequence there -- the
 *         duplicates -- are therefore the H mass strictly inside the interval.
 *   Filters   kind, min_len, min_count, max_count as in sufr_repeat.h; min_seqs: 0 means 1; max_seqs: 0 means off.  A record
 *         is kept iff the conditions of sufr_repeat.h hold and min_seqs <= seqs <= max_seqs.
 *   Records   four parallel arrays of `cap` entries, u64 for both index widths: rank (= a), count, length (= v), seqs, in
 *         ascending order of the representative rank.  The capacity rule of sufr_repeat.h: *total_out always receives the
 *         number of kept records; when it exceeds cap the call returns SUFR_HIP_E_CAPACITY and fills nothing; cap == 0 with
 *         NULL arrays is a counting call.
 *   Stats     records; longest and longest_rank, ties to the smallest representative; max_count; max_seqs, the largest seqs
 *         of a kept record.  All zero when nothing is kept.  With kind 0, open count filters and min_seqs = num_sequences,
 *         `longest` is the longest common substring of all sequences.
 *   k-common profile   common[q - 1], q = 1 .. num_sequences, is the largest v over all intervals (kind 0, no filters) with
 *         seqs >= q, 0 if there is none.  It is non-increasing, and common[0] is the `longest` of repeats(kind 0, min_len 1).
 *
 * Refusals are those of sufr_repeat.h: a seed-mask file or index and a build with max_query_len > 0,
 * SUFR_HIP_E_UNSUPPORTED; min_len == 0, an unknown kind, sequence starts that do not ascend from 0 or reach n, and
 * min_seqs > max_seqs with max_seqs != 0, SUFR_HIP_E_INVALID.  An empty array (s == 0) is a valid call with no records and
 * an all-zero profile; one sequence is valid: every seqs is 1.  The device path also refuses s >= 2^40 and
 * num_sequences >= 2^24 (its sort keys hold a sequence and a rank in one word): SUFR_HIP_E_UNSUPPORTED.
 */
#ifndef SUFR_SHARED_H
#define SUFR_SHARED_H
#include <stddef.h>
#include <stdint.h>

#include "sufr_repeat.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sufr_shared_stats { uint64_t records, longest, longest_rank, max_count, max_seqs; } sufr_shared_stats;

/* ---- host: `threads` workers (0: one per core); the sequence starts come from the file.  rank, count, length, seqs: cap
 * entries each (NULL with cap == 0); total_out and stats may be NULL. */
int sufr_file_shared(const sufr_file *f, uint32_t kind, uint64_t min_len, uint64_t min_count, uint64_t max_count, uint64_t min_seqs,
                     uint64_t max_seqs, uint64_t cap, uint64_t *rank, uint64_t *count, uint64_t *length, uint64_t *seqs,
                     uint64_t *total_out, sufr_shared_stats *stats, int threads);
/* common: one entry per sequence of the file (sufr_file_meta.num_sequences). */
int sufr_file_common(const sufr_file *f, uint64_t *common, int threads);

/* ---- device: ctx, ix, d_lcp, seq_starts and num_sequences as in sufr_hip_repeats_device (NULL / 0 / 1: one sequence);
 * d_rank, d_count, d_length, d_seqs: cap u64 each on the device.  The passes of sufr_hip_repeats_device over SA, LCP and the
 * text, then one key per rank, a radix sort of the keys by sequence, a pass over the sorted keys that adds every pair to
 * H, the prefix of H, and the search pass, which counts; the call synchronises once, for the total and the stats, and then
 * enqueues the search pass again, which writes, on the context's stream (complete after sufr_hip_synchronize).  Entries
 * beyond the total are not written.  The tile of sufr_hip_set_repeat_tile applies and changes no result. */
int sufr_hip_shared_device(sufr_hip_ctx *ctx, const sufr_hip_index *ix, const void *d_lcp, const uint64_t *seq_starts,
                           uint64_t num_sequences, uint32_t kind, uint64_t min_len, uint64_t min_count, uint64_t max_count,
                           uint64_t min_seqs, uint64_t max_seqs, uint64_t cap, void *d_rank, void *d_count, void *d_length,
                           void *d_seqs, uint64_t *total_out, sufr_shared_stats *stats_out);
/* d_common: max(num_sequences, 1) u64 on the device, written on the context's stream (complete after sufr_hip_synchronize);
 * the call itself does not synchronise. */
int sufr_hip_common_device(sufr_hip_ctx *ctx, const sufr_hip_index *ix, const void *d_lcp, const uint64_t *seq_starts,
                           uint64_t num_sequences, void *d_common);

#ifdef __cplusplus
}
#endif
#endif /* SUFR_SHARED_H */
