/*
 * sufr_fm_approx.h -- k-mismatch search on the FM-index of sufr_fm.h by backtracking, on the host and on the GPU (part of
 * libsufr_hip.so).  It reads neither the text nor the suffix array.  The definition -- nodes, the order
 * of the leaves, records, special cases, errors -- is the block "k-mismatch search by backtracking" of sufr_fm.h.
 */
#ifndef SUFR_FM_APPROX_H
#define SUFR_FM_APPROX_H
#include <stddef.h>
#include <stdint.h>

#include "sufr_fm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SUFR_FM_APPROX_BOTH_STRANDS 0x1u
#define SUFR_FM_APPROX_MAX_MISMATCHES 3u

/* ---- host.  queries / offsets as for sufr_fm_search_batch; query, strand, position, mismatches: cap records each.  Workers
 * take (query, strand) items; no result depends on their number.  The records are counted before any position is walked, so a
 * call that ends in SUFR_HIP_E_CAPACITY costs the count alone. */
int  sufr_fm_approx(const sufr_fm *fm, const uint8_t *queries, const uint64_t *offsets, uint64_t num_queries, uint32_t max_mismatches,
                    uint32_t flags, uint64_t cap, uint64_t *query, uint8_t *strand, uint64_t *position, uint8_t *mismatches,
                    uint64_t *total_out, int threads);
/* For measurement only (profiles/fm_approx_bench.py): what the walk of a batch costs -- the leaves and the steps (one step: the
 * ranks of one range moved by one place, for one byte value or prepared for all of them) of every (query, strand) item,
 * num_queries entries each, twice as many with both strands. */
int  sufr_fm_approx_steps(const sufr_fm *fm, const uint8_t *queries, const uint64_t *offsets, uint64_t num_queries, uint32_t max_mismatches,
                          uint32_t flags, uint64_t *leaves, uint64_t *steps, int threads);

/* ---- device.  The records of sufr_fm_approx for a batch on the device, in the same order and with the same bytes on every
 * call.  One synchronisation, for the number of leaves and of records (with both strands the batch's byte count is read first, a
 * synchronisation of its own, as sufr_hip_approx_device does); the records are enqueued on the context's stream after it
 * (complete after sufr_hip_synchronize).  _approx takes host buffers and returns when the records are there. */
int  sufr_hip_fm_approx_device(sufr_hip_ctx *ctx, const sufr_hip_fm *fm, const void *d_queries, const void *d_offsets, uint64_t num_queries,
                               uint32_t max_mismatches, uint32_t flags, uint64_t cap, void *d_query, void *d_strand, void *d_position,
                               void *d_mismatches, uint64_t *total_out);
int  sufr_hip_fm_approx(sufr_hip_ctx *ctx, const sufr_hip_fm *fm, const uint8_t *queries, const uint64_t *offsets, uint64_t num_queries,
                        uint32_t max_mismatches, uint32_t flags, uint64_t cap, uint64_t *query, uint8_t *strand, uint64_t *position,
                        uint8_t *mismatches, uint64_t *total_out);

#ifdef __cplusplus
}
#endif
#endif /* SUFR_FM_APPROX_H */
