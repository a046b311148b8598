/*
 * sufr_edit.h -- k-difference search of query batches against the text: where a query ends in the text with at most d
 * substitutions, insertions and deletions (pigeonhole seeds, a banded Sellers table per candidate, sorted unique ends), on
 * one or both strands, on the host and on the GPU (part of libsufr_hip.so).
 *
 * Definitions.  The terms are those of sufr_approx.h: text T (n bytes), indexed positions I (the values of SA), the build's
 * max_query_len L (no cap when 0); queries are bytes, the sentinel and the sequence delimiter are ordinary bytes.  For a query
 * Q of length m and d = max_edits:
 *   piece     i (0 <= i <= d) is Q[o_i .. o_{i+1}) with o_i = floor(i * m / (d + 1)); its seed is its first
 *             k'_i = min(len_i, L) bytes (len_i when L == 0).
 *   live      a piece is live when max_occ == 0 or its seed starts at most max_occ indexed suffixes.
 *   D(e)      for an exclusive text end 0 <= e <= n: the minimum over b <= e of the unit-cost edit distance (substitution,
 *             insertion, deletion) between Q and T[b .. e): Sellers' semi-global distance.
 *   covers    piece i covers e when it is live, some t in I has T[t .. t + k'_i) equal to its seed, and
 *             |e - (t - o_i + m)| <= d in signed arithmetic (t - o_i may be negative).
 *   record    (query, strand, end = e - 1, edits = D(e)) is one iff D(e) <= d and some piece covers e.  A query with
 *             m < d + 1 has no records; m >= d + 1 also means that a match consumes at least one text byte, so `end` is a
 *             text position.
 *   SUFR_EDIT_BOTH_STRANDS   every query is also searched as its reverse complement (the rule of SUFR_APPROX_BOTH_STRANDS);
 *             those records carry strand 1 and `end` is where the reverse complement ends.
 *   SUFR_EDIT_LOCAL_MINIMA   a record at e stays only when D(e - 1) > D(e) and D(e + 1) >= D(e), a neighbour that is not a
 *             record counting as d + 1.  Without the flag an exact occurrence shows up as a hill of up to 2d + 1 ends, with
 *             it as one.
 * Records come sorted by (query, strand, end), each once, as four parallel arrays: query u64, strand u8, end u64, edits u8.
 *
 * Completeness.  An alignment with at most d edits leaves one of the d + 1 pieces unedited; that piece occurs exactly at some
 * t, and the alignment ends within d of t - o_i + m.  With max_occ == 0 on an index with s == n the records are all ends
 * with D(e) <= d.  Where the array leaves positions out, the ends that are lost are those whose unedited pieces all start on
 * unindexed positions.  A -m L build gives the records of the uncapped build of the same text when max_occ == 0.
 *
 * Out of scope: alignment starts, CIGAR strings, traceback.  The call is the "find the ends" phase; a caller traces back the
 * few ends it keeps (a backward banded table from `end` over at most m + d text bytes).  See sufr_align.h, which does that
 * for a list of records, on the host and on the GPU.
 *
 * Limits.  max_edits above SUFR_EDIT_MAX_EDITS is SUFR_HIP_E_INVALID; 0 is legal (exact occurrences, by their last byte).
 * Files and indexes built with a seed mask are refused (SUFR_HIP_E_UNSUPPORTED).  The device path sorts 64-bit keys that
 * hold the query number (doubled with both strands), the end and the distance: a batch with
 * bits(queries - 1) + bits(n) + 4 > 64 is refused (SUFR_HIP_E_UNSUPPORTED); it needs device memory for one byte per
 * candidate and 16 bytes per reported end before the unique step, and fails with SUFR_HIP_E_NOMEM when that is not there.
 *
 * Batches use the layout of sufr_file_search_batch.  Outputs hold `cap` records; *total_out receives the number of records
 * even when it exceeds cap (the call then returns SUFR_HIP_E_CAPACITY and fills nothing).
 */
#ifndef SUFR_EDIT_H
#define SUFR_EDIT_H
#include <stddef.h>
#include <stdint.h>

#include "sufr_query.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SUFR_EDIT_BOTH_STRANDS 0x1u
#define SUFR_EDIT_LOCAL_MINIMA 0x2u
#define SUFR_EDIT_MAX_EDITS 15u

/* ---- host: `threads` workers (0: one per core) share the query bytes ------------------------------------------- */
int sufr_file_edit(const sufr_file *f, const uint8_t *queries, const uint64_t *offsets, uint64_t num_queries,
                   uint32_t max_edits, uint64_t max_occ, uint32_t flags, uint64_t cap, uint64_t *query, uint8_t *strand,
                   uint64_t *end, uint8_t *edits, uint64_t *total_out, int threads);

/* ---- device: the index of sufr_hip_index_load / sufr_hip_index_wrap ---------------------------------------------
 * _edit_device reads the batch's byte count from d_offsets, then synchronises for the candidate total, the total of the
 * reported ends and the record total (once more with SUFR_EDIT_LOCAL_MINIMA); the records are enqueued on the context's
 * stream after that (complete after sufr_hip_synchronize).  It shares the bitmap of the indexed positions with
 * sufr_hip_mems_device and sufr_hip_approx_device.
 * _edit takes host buffers and returns when the records are there. */
int sufr_hip_edit_device(sufr_hip_ctx *ctx, const sufr_hip_index *ix, const void *d_queries, const void *d_offsets,
                         uint64_t num_queries, uint32_t max_edits, uint64_t max_occ, uint32_t flags, uint64_t cap,
                         void *d_query, void *d_strand, void *d_end, void *d_edits, uint64_t *total_out);
int sufr_hip_edit(sufr_hip_ctx *ctx, const sufr_hip_index *ix, const uint8_t *queries, const uint64_t *offsets,
                  uint64_t num_queries, uint32_t max_edits, uint64_t max_occ, uint32_t flags, uint64_t cap,
                  uint64_t *query, uint8_t *strand, uint64_t *end, uint8_t *edits, uint64_t *total_out);

#ifdef __cplusplus
}
#endif
#endif /* SUFR_EDIT_H */
