/*
 * sufr_repeat.h -- the repeats of the indexed text from its suffix array and LCP array: the LCP intervals (the internal
 * nodes of the suffix tree, the right-maximal repeats), the left-diverse ones among them (the maximal repeats) and the
 * leaves of that hierarchy (the supermaximal repeats), each with its length, its occurrence count and the rank range of
 * its occurrences; on the host and on the GPU (part of libsufr_hip.so).  It is the variable-length
 * counterpart of sufr_kmer.h: which substrings repeat, how long they are, how often and where they occur, and which is the
 * longest.
 *
 * Definitions.  T, n, SA[0..s), LCP, w, breaks and brk(p) are exactly as in sufr_kmer.h; everything is defined from the
 * arrays alone.
 *   Clipped LCP   d(p) = brk(p) - p.  l[0] = 0, l[r] = min(LCP[r], d(SA[r-1]), d(SA[r])), l[s] := 0: two suffixes never
 *         agree "through" a break.  With one sequence l = LCP for r >= 1.
 *   Interval      for a rank r with v = l[r] >= 1 let a be the largest j < r with l[j] < v and b the smallest j > r with
 *         l[j] < v (s if there is none).  [a, b) is an interval of value v, count = b - a.  r is its representative iff no j
 *         in (a, r) has l[j] == v; every interval has exactly one.  The occurrences are SA[a..b); all have d >= v, so no
 *         occurrence contains a break.
 *   Left symbol   lambda(p) = T[p-1], unless p == 0 or p - 1 is a break: then lambda(p) is a symbol of its own, different
 *         from every byte and from that of every other sequence start.  It is read from the text whether or not p - 1 is
 *         indexed.
 *   Kinds   SUFR_REPEAT_BRANCHING: every interval.  SUFR_REPEAT_MAXIMAL: the intervals whose occurrences do not all share
 *         one lambda, i.e. some r in (a, b) has lambda(SA[r-1]) != lambda(SA[r]).  SUFR_REPEAT_SUPERMAXIMAL: l[j] == v for
 *         all j in (a, b), and the lambdas of the occurrences are pairwise different.
 *   Text-level meaning   where the delimiter byte occurs only at breaks, a record is a string without a break that has at
 *         least two indexed occurrences, and: kind 0, the occurrences are not all followed by one symbol; kind 1, they are
 *         also not all preceded by one symbol; kind 2, they are pairwise different in both the following and the preceding
 *         symbol -- a break counts as different from everything.  Where delimiter bytes also occur inside sequences, or the
 *         sequence starts are positional only (no delimiter byte in the text), the array definition stands: the suffixes
 *         are ordered by the bytes, the clip is positional, and the occurrences of one string may then come as more than one
 *         interval (an interval splits where a clipped rank lies between its ranks).  It is defined per interval of l and
 *         needs no rule of its own.
 *   Filters   min_len >= 1; min_count: 0 and 1 mean 2; max_count: 0 means off.  A record is kept iff v >= min_len and
 *         min_count <= count <= max_count.
 *   Records   three parallel arrays of `cap` entries, u64 for both index widths: rank (= a), count, length (= v), in
 *         ascending order of the representative rank -- one fixed order that needs no sort, the same on the host and on the
 *         device.  *total_out always receives the number of kept records; when it exceeds cap the call returns
 *         SUFR_HIP_E_CAPACITY and fills nothing (the rule of sufr_mem.h).  cap == 0 with NULL arrays is a counting call.
 *   Stats     records; longest and longest_rank, the length and rank of the longest kept record, ties to the smallest
 *         representative (the longest repeated substring when kind is 0 and the filters are open); max_count, the largest
 *         count of a kept record.  All zero when nothing is kept.
 * Scope.  Occurrences are INDEXED positions, as in sufr_kmer.h.
 *
 * Refusals.  A seed-mask file or index, and a build with max_query_len > 0 (its LCP is capped): SUFR_HIP_E_UNSUPPORTED.
 * min_len == 0, an unknown kind, sequence starts that do not ascend from 0 or reach n: SUFR_HIP_E_INVALID.  An empty array
 * (s == 0) is a valid call with no records.
 */
#ifndef SUFR_REPEAT_H
#define SUFR_REPEAT_H
#include <stddef.h>
#include <stdint.h>

#include "sufr_query.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sufr_repeat_stats { uint64_t records, longest, longest_rank, max_count; } sufr_repeat_stats;
#define SUFR_REPEAT_BRANCHING 0u
#define SUFR_REPEAT_MAXIMAL 1u
#define SUFR_REPEAT_SUPERMAXIMAL 2u

/* ---- host: `threads` workers (0: one per core) over the mapped arrays and text; the sequence starts come from the file.
 * rank, count, length: cap entries each (NULL with cap == 0); total_out and stats may be NULL. */
int sufr_file_repeats(const sufr_file *f, uint32_t kind, uint64_t min_len, uint64_t min_count, uint64_t max_count, uint64_t cap,
                      uint64_t *rank, uint64_t *count, uint64_t *length, uint64_t *total_out, sufr_repeat_stats *stats,
                      int threads);

/* ---- device: the index of sufr_hip_index_load / sufr_hip_index_wrap (its SA, n, s, build cap and its text, for lambda).
 * d_lcp and seq_starts are as in sufr_hip_kmers_device.  d_rank, d_count, d_length: cap u64 each on the device.
 * One pass over SA, LCP and the text leaves l (several sequences only), two flag bits per rank and the first level of the
 * min pyramid; small launches finish the pyramid and the popcount prefixes; a search pass counts the kept records per
 * tile and the stats; the call synchronises once, for the total and the stats, and then enqueues the same search pass
 * again, which writes the records, on the context's stream (complete after sufr_hip_synchronize).  Entries beyond the
 * total are not written. */
int sufr_hip_repeats_device(sufr_hip_ctx *ctx, const sufr_hip_index *ix, const void *d_lcp, const uint64_t *seq_starts,
                            uint64_t num_sequences, uint32_t kind, uint64_t min_len, uint64_t min_count, uint64_t max_count,
                            uint64_t cap, void *d_rank, void *d_count, void *d_length, uint64_t *total_out,
                            sufr_repeat_stats *stats_out);
/* Ranks one workgroup takes at a time (0: the default, 16384): rounded up to the workgroup size, 256, and held to 16384 at
 * most.  It changes no result; small tiles put many tile boundaries into small arrays. */
int sufr_hip_set_repeat_tile(sufr_hip_ctx *ctx, uint64_t ranks);

#ifdef __cplusplus
}
#endif
#endif /* SUFR_REPEAT_H */
