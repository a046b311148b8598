/*
 * sufr_match.h -- matching statistics and super-maximal exact matches (SMEMs) of query batches, on the host and on the GPU
 * (part of libsufr_hip.so).
 *
 * Definitions.  The index holds text T and the ranks SA[0..s) of its indexed suffixes; L is the build's max_query_len
 * (no cap when 0).  Queries are bytes, compared byte for byte as sufr_file_search compares them.  For a query Q of
 * length m:
 *   ms[j]  (0 <= j < m)  the largest l <= min(m - j, L) such that Q[j..j+l) is a prefix of some indexed suffix
 *                        (0 when no indexed suffix starts with Q[j]);
 *   SMEM   offset j starts one iff ms[j] >= min_len and (j == 0 or ms[j-1] <= ms[j]); it is the query interval
 *          [j, j + ms[j]), and [rank_lo, rank_hi) is the rank range of the indexed suffixes that start with it.
 * Records come in (query, offset) order.  Files and indexes built with a seed mask are refused (SUFR_HIP_E_UNSUPPORTED),
 * min_len 0 is SUFR_HIP_E_INVALID, an empty query has no statistics and no SMEMs.
 *
 * Batches use the layout of sufr_file_search_batch: the concatenated query bytes plus num_queries + 1 offsets, query i =
 * bytes [offsets[i], offsets[i+1]).  Matching statistics land in ms[offsets[i] + j].  SMEM outputs hold `cap` records;
 * *total_out receives the number of SMEMs even when it exceeds cap (the call then returns SUFR_HIP_E_CAPACITY and fills
 * nothing).  The positions of an SMEM are SA[rank_lo .. rank_hi): on the device, hand rank_lo / rank_hi to
 * sufr_hip_locate_batch_device.
 */
#ifndef SUFR_MATCH_H
#define SUFR_MATCH_H
#include <stddef.h>
#include <stdint.h>

#include "sufr_query.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- host: `threads` workers (0: one per core) share the query bytes ------------------------------------------- */
int sufr_file_matching_stats(const sufr_file *f, const uint8_t *queries, const uint64_t *offsets, uint64_t num_queries,
                             uint32_t *ms, int threads);
int sufr_file_smems(const sufr_file *f, const uint8_t *queries, const uint64_t *offsets, uint64_t num_queries,
                    uint32_t min_len, uint64_t cap, uint64_t *query, uint32_t *query_offset, uint32_t *length,
                    uint64_t *rank_lo, uint64_t *rank_hi, uint64_t *total_out, int threads);

/* ---- device: the index of sufr_hip_index_load / sufr_hip_index_wrap ---------------------------------------------
 * _matching_stats_device only enqueues on the context's stream; d_ms holds offsets[num_queries] u32 entries.
 * _smems_device computes the statistics into d_ms (same size; the caller's scratch, it receives them), flags the SMEMs,
 * synchronises once to read their total, then enqueues the records and their rank ranges (sufr_hip_search_batch_device
 * of the SMEM slices) without further synchronisation.
 * _smems takes host buffers and returns when the records are there. */
int sufr_hip_matching_stats_device(sufr_hip_ctx *ctx, const sufr_hip_index *ix, const void *d_queries, const void *d_offsets,
                                   uint64_t num_queries, void *d_ms);
int sufr_hip_smems_device(sufr_hip_ctx *ctx, const sufr_hip_index *ix, const void *d_queries, const void *d_offsets,
                          uint64_t num_queries, uint32_t min_len, void *d_ms, uint64_t cap, void *d_query, void *d_query_offset,
                          void *d_length, void *d_rank_lo, void *d_rank_hi, uint64_t *total_out);
int sufr_hip_smems(sufr_hip_ctx *ctx, const sufr_hip_index *ix, const uint8_t *queries, const uint64_t *offsets,
                   uint64_t num_queries, uint32_t min_len, uint64_t cap, uint64_t *query, uint32_t *query_offset,
                   uint32_t *length, uint64_t *rank_lo, uint64_t *rank_hi, uint64_t *total_out);

#ifdef __cplusplus
}
#endif
#endif /* SUFR_MATCH_H */
