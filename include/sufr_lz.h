/*
 * sufr_lz.h -- the longest previous factor (LPF) of every text position, with a source position, and the Lempel-Ziv
 * (LZ77) factorization that follows from it, from the suffix array and the LCP array of the indexed text; on the host and
 * on the GPU (part of libsufr_hip.so).  sufr_kmer.h and sufr_repeat.h answer by rank; this header
 * answers by position and in text order: "this stretch is a copy of that earlier one", and how many such stretches (z) the
 * text is made of.
 *
 * Definitions.  T, n, SA[0..s), LCP, w, breaks, brk(p) and d(p) = brk(p) - p are exactly as in sufr_kmer.h and
 * sufr_repeat.h; everything is defined from the arrays alone.  NONE is all ones of the entry width.
 *   For a rank r with p = SA[r]
 *         j1 is the largest j < r with SA[j] < p and m1 = min LCP(j1, r]; both are absent when there is no such j.
 *         j2 is the smallest j > r with SA[j] < p and m2 = min LCP(r, j2]; both are absent when there is no such j.
 *         LPF[p] = min(d(p), max(m1, m2)), or 0 when both are absent.
 *         SRC[p] = SA[j1] if m1 exists and (m2 is absent or m1 >= m2), otherwise SA[j2]; SRC[p] = NONE whenever
 *         LPF[p] == 0.  The tie rule m1 >= m2 -> j1 is part of the contract: host and device agree entry for entry.
 *   A position that is not indexed has LPF = 0 and SRC = NONE.
 *   Text-level meaning   where the LCP is exact and delimiter bytes occur only at breaks, LPF[p] is the length of the
 *         longest string that starts at p, holds no break, and also starts at an indexed q < p; SRC[p] is such a q.  The
 *         copy may overlap p (q + LPF[p] > p).  A break position itself has d = 0, hence LPF = 0.
 *   Parse     p_0 = 0, p_{i+1} = p_i + max(1, LPF[p_i]), until n.  Factor i is (start = p_i, length = max(1, LPF[p_i]),
 *         source = SRC[p_i]); source == NONE marks a literal of length 1.  With every position indexed (s == n) this is
 *         the greedy, self-referential LZ77 parse per sequence: factors never span a break, sources may lie in earlier
 *         sequences.  With s < n it is still a valid parse: a factor that starts at a position that is not indexed is a
 *         literal, and copies start and are sourced at indexed positions only (a copy may run over positions that are
 *         not indexed when its source does).
 *   Records   three parallel arrays of `cap` entries, u64 for both index widths: start, length, source (NONE = ~0), in
 *         text order.  *total_out always receives z, the number of factors; when it exceeds cap the call returns
 *         SUFR_HIP_E_CAPACITY and fills nothing (the rule of sufr_mem.h and sufr_repeat.h).  cap == 0 with NULL arrays is
 *         a counting call.
 *   Stats     factors (= z); literals; longest and longest_start, the length and start of the longest factor, ties to the
 *         smallest start.  All zero for n == 0.
 * Scope.  Copies and sources are INDEXED positions, as in sufr_kmer.h and sufr_repeat.h.
 *
 * Refusals.  A seed-mask file or index, and a build with max_query_len > 0 (its LCP is capped): SUFR_HIP_E_UNSUPPORTED.
 * Sequence starts that do not ascend from 0 or reach n: SUFR_HIP_E_INVALID.  An empty array (s == 0) is a valid call: LPF is
 * all zero and the parse is n literals.
 */
#ifndef SUFR_LZ_H
#define SUFR_LZ_H
#include <stddef.h>
#include <stdint.h>

#include "sufr_query.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sufr_lz_stats { uint64_t factors, literals, longest, longest_start; } sufr_lz_stats;

/* ---- host: `threads` workers (0: one per core) over the mapped arrays; the sequence starts come from the file.
 * lpf, src: n entries each of the file's index width (4 or 8 bytes), by position; either may be NULL. */
int sufr_file_lpf(const sufr_file *f, void *lpf, void *src, int threads);
/* start, length, source: cap entries each (NULL with cap == 0); total_out and stats may be NULL. */
int sufr_file_lz(const sufr_file *f, uint64_t cap, uint64_t *start, uint64_t *length, uint64_t *source, uint64_t *total_out,
                 sufr_lz_stats *stats, int threads);

/* ---- device: the index of sufr_hip_index_load / sufr_hip_index_wrap (its SA, n, s and build cap).  d_lcp and seq_starts
 * are as in sufr_hip_kmers_device.  d_lpf, d_src: n entries each of the index width on the device; either may be NULL.
 * Enqueued only, on the context's stream (complete after sufr_hip_synchronize). */
int sufr_hip_lpf_device(sufr_hip_ctx *ctx, const sufr_hip_index *ix, const void *d_lcp, const uint64_t *seq_starts,
                        uint64_t num_sequences, void *d_lpf, void *d_src);
/* d_start, d_length, d_source: cap u64 each on the device.  LPF and SRC go to scratch of the context; a table pass, the
 * serial walk from tile to tile and a counting pass over the entered tiles leave the total and the stats; the call
 * synchronises once, for them, and then enqueues the writing pass on the context's stream (complete after
 * sufr_hip_synchronize).  Entries beyond the total are not written. */
int sufr_hip_lz_device(sufr_hip_ctx *ctx, const sufr_hip_index *ix, const void *d_lcp, const uint64_t *seq_starts,
                       uint64_t num_sequences, uint64_t cap, void *d_start, void *d_length, void *d_source,
                       uint64_t *total_out, sufr_lz_stats *stats_out);
/* Ranks one workgroup of the LPF pass takes at a time, and text positions one workgroup of the parse takes at a time (0:
 * the default, 16384 each): rounded up to the workgroup size, 256, and held to 16384 at most.  They change no result;
 * small tiles put many tile boundaries into small texts. */
int sufr_hip_set_lz_tile(sufr_hip_ctx *ctx, uint64_t ranks, uint64_t positions);

#ifdef __cplusplus
}
#endif
#endif /* SUFR_LZ_H */
