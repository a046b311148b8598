/*
 * sufr_approx.h -- k-mismatch search of query batches against the text (seed and verify with the pigeonhole filter), on one
 * or both strands, on the host and on the GPU (part of libsufr_hip.so).
 *
 * Definitions.  The index holds text T (n bytes) and its indexed suffixes SA[0..s); I is the set of indexed positions (the
 * values of SA); L is the build's max_query_len (no cap when 0).  Queries are bytes, compared byte for byte as
 * sufr_file_search compares them; the sentinel and the sequence delimiter are ordinary bytes, as they are for MEMs.  For a
 * query Q of length m and d = max_mismatches:
 *   piece     i (0 <= i <= d) is Q[o_i .. o_{i+1}) with o_i = floor(i * m / (d + 1)); its seed is its first
 *             k'_i = min(len_i, L) bytes (len_i when L == 0).  A query with m < d + 1 would have an empty piece: it has no
 *             records.
 *   live      a piece is live when max_occ == 0 or its seed starts at most max_occ indexed suffixes (the rule of
 *             sufr_mem.h, BWA's -c).
 *   alignment a window start p with p + m <= n; its distance is h(p) = #{t : Q[t] != T[p + t]}.  Piece i anchors p when it is
 *             live, p + o_i is in I and the whole piece equals T[p + o_i .. p + o_{i+1}).
 *   record    (query, strand, position = p, mismatches = h(p)) is one iff h(p) <= d and at least one piece anchors p.  It is
 *             reported once, by the lowest anchoring piece.
 *   SUFR_APPROX_BOTH_STRANDS  every query is also searched as its reverse complement Q' (the rule of
 *             SUFR_MEM_BOTH_STRANDS); those records carry strand 1 and position is where Q' aligns.
 * Records come in (query, strand, piece, rank) order, the rank being that of the suffix p + o_i in the seed's range, as four
 * parallel arrays: query u64, strand u8, position u64, mismatches u8.
 *
 * Completeness.  d mismatches fall into at most d of the d + 1 pieces, so every alignment with h(p) <= d has a piece that
 * matches exactly: with max_occ == 0 on an index with s == n the records are all alignments within distance d.  Where the
 * array leaves positions out (--dna builds: ambiguity codes, soft-masked stretches) the alignments that are lost are exactly
 * those whose exactly matching pieces all start on unindexed positions.  A -m L build gives the record set of the uncapped
 * build of the same text when max_occ == 0 (verification reads the text, not the array); only the order within a piece may
 * differ.
 *
 * Limits.  max_mismatches above SUFR_APPROX_MAX_MISMATCHES is SUFR_HIP_E_INVALID; 0 is legal (one piece: exact locate at
 * window starts).  Files and indexes built with a seed mask are refused (SUFR_HIP_E_UNSUPPORTED).
 *
 * Batches use the layout of sufr_file_search_batch: the concatenated query bytes plus num_queries + 1 offsets, query i =
 * bytes [offsets[i], offsets[i+1]).  Outputs hold `cap` records; *total_out receives the number of records even when it
 * exceeds cap (the call then returns SUFR_HIP_E_CAPACITY and fills nothing).
 */
#ifndef SUFR_APPROX_H
#define SUFR_APPROX_H
#include <stddef.h>
#include <stdint.h>

#include "sufr_query.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SUFR_APPROX_BOTH_STRANDS 0x1u
#define SUFR_APPROX_MAX_MISMATCHES 15u

/* ---- host: `threads` workers (0: one per core) share the query bytes ------------------------------------------- */
int sufr_file_approx(const sufr_file *f, const uint8_t *queries, const uint64_t *offsets, uint64_t num_queries,
                     uint32_t max_mismatches, uint64_t max_occ, uint32_t flags, uint64_t cap, uint64_t *query,
                     uint8_t *strand, uint64_t *position, uint8_t *mismatches, uint64_t *total_out, int threads);

/* ---- device: the index of sufr_hip_index_load / sufr_hip_index_wrap ---------------------------------------------
 * _approx_device reads the batch's byte count from d_offsets, then synchronises once for the candidate total and once for
 * the record total; the records are enqueued on the context's stream after that (complete after sufr_hip_synchronize).
 * It shares the bitmap of the indexed positions with sufr_hip_mems_device (n / 8 bytes, built by the first call of either
 * on an index whose array leaves text positions out, kept until sufr_hip_index_free).
 * _approx takes host buffers and returns when the records are there. */
int sufr_hip_approx_device(sufr_hip_ctx *ctx, const sufr_hip_index *ix, const void *d_queries, const void *d_offsets,
                           uint64_t num_queries, uint32_t max_mismatches, uint64_t max_occ, uint32_t flags, uint64_t cap,
                           void *d_query, void *d_strand, void *d_position, void *d_mismatches, uint64_t *total_out);
int sufr_hip_approx(sufr_hip_ctx *ctx, const sufr_hip_index *ix, const uint8_t *queries, const uint64_t *offsets,
                    uint64_t num_queries, uint32_t max_mismatches, uint64_t max_occ, uint32_t flags, uint64_t cap,
                    uint64_t *query, uint8_t *strand, uint64_t *position, uint8_t *mismatches, uint64_t *total_out);

#ifdef __cplusplus
}
#endif
#endif /* SUFR_APPROX_H */
