/*
 * sufr_mem.h -- maximal exact matches (MEMs) of query batches against the text, on one or both strands, on the host and on
 * the GPU (part of libsufr_hip.so).
 *
 * Definitions.  The index holds text T (n bytes) and its indexed suffixes SA[0..s); I is the set of indexed positions (the
 * values of SA); L is the build's max_query_len (no cap when 0).  Queries are bytes, compared byte for byte as
 * sufr_file_search compares them.  For a query Q of length m, an offset j, a position p in I and l(j, p) = lcp(Q[j..m), T[p..n)):
 *   MEM   (j, p, l) is one iff l(j, p) >= min_len and it cannot be extended to the left: j == 0, or p == 0, or
 *         Q[j-1] != T[p-1], or p-1 is not in I.  l is the exact, uncapped length (a MEM is right-maximal by construction).
 *   max_occ (0: off)  with k' = min(min_len, L) (min_len when L == 0): an offset j whose k'-prefix Q[j..j+k') starts more
 *         than max_occ indexed suffixes contributes no MEM.
 *   SUFR_MEM_BOTH_STRANDS  every query is also matched as its reverse complement Q' (Q reversed, uppercase A<->T and C<->G
 *         swapped, every other byte kept); records of Q' carry strand 1 and offsets in Q' coordinates.
 * Records come in (query, strand, offset, rank) order, as five parallel arrays: query u64, query_offset u32, strand u8,
 * length u32, position u64 (for both widths of the suffix array).  A -m L build gives the MEM set of the uncapped build of
 * the same text whenever max_occ == 0 or min_len <= L; only the rank order within an offset may differ.
 * Files and indexes built with a seed mask are refused (SUFR_HIP_E_UNSUPPORTED), min_len 0 is SUFR_HIP_E_INVALID, an empty
 * query or one shorter than min_len has no MEMs.
 *
 * Batches use the layout of sufr_file_search_batch: the concatenated query bytes plus num_queries + 1 offsets, query i =
 * bytes [offsets[i], offsets[i+1]).  Outputs hold `cap` records; *total_out receives the number of MEMs even when it exceeds
 * cap (the call then returns SUFR_HIP_E_CAPACITY and fills nothing).
 */
#ifndef SUFR_MEM_H
#define SUFR_MEM_H
#include <stddef.h>
#include <stdint.h>

#include "sufr_query.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SUFR_MEM_BOTH_STRANDS 0x1u

/* ---- host: `threads` workers (0: one per core) share the query bytes ------------------------------------------- */
int sufr_file_mems(const sufr_file *f, const uint8_t *queries, const uint64_t *offsets, uint64_t num_queries,
                   uint32_t min_len, uint64_t max_occ, uint32_t flags, uint64_t cap, uint64_t *query,
                   uint32_t *query_offset, uint8_t *strand, uint32_t *length, uint64_t *position,
                   uint64_t *total_out, int threads);

/* ---- device: the index of sufr_hip_index_load / sufr_hip_index_wrap ---------------------------------------------
 * _mems_device reads the batch's byte count from d_offsets, then synchronises once for the candidate total and once for
 * the MEM total; the records are enqueued on the context's stream after that (complete after sufr_hip_synchronize).
 * The first call on an index whose array leaves text positions out builds a bitmap of the indexed positions (n / 8
 * bytes, kept until sufr_hip_index_free).
 * _mems takes host buffers and returns when the records are there. */
int sufr_hip_mems_device(sufr_hip_ctx *ctx, const sufr_hip_index *ix, const void *d_queries, const void *d_offsets,
                         uint64_t num_queries, uint32_t min_len, uint64_t max_occ, uint32_t flags, uint64_t cap,
                         void *d_query, void *d_query_offset, void *d_strand, void *d_length, void *d_position,
                         uint64_t *total_out);
int sufr_hip_mems(sufr_hip_ctx *ctx, const sufr_hip_index *ix, const uint8_t *queries, const uint64_t *offsets,
                  uint64_t num_queries, uint32_t min_len, uint64_t max_occ, uint32_t flags, uint64_t cap, uint64_t *query,
                  uint32_t *query_offset, uint8_t *strand, uint32_t *length, uint64_t *position, uint64_t *total_out);

#ifdef __cplusplus
}
#endif
#endif /* SUFR_MEM_H */
