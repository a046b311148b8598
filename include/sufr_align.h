/*
 * sufr_align.h -- alignment traceback of k-difference records: for every record (query, strand, end, edits) that
 * sufr_file_edit / sufr_hip_edit(_device) reports, where its alignment starts in the text and its CIGAR, on the host and on
 * the GPU (part of libsufr_hip.so).
 *
 * Definitions.  The terms are those of sufr_edit.h: text T (n bytes), a query Q of m bytes; the sentinel and the sequence
 * delimiter are ordinary bytes.  C is Sellers' table of Q against T:
 *   C[0][j] = 0                                                      (0 <= j <= n)
 *   C[i][0] = i                                                      (0 <= i <= m)
 *   C[i][j] = min(C[i-1][j-1] + [Q[i-1] != T[j-1]], C[i-1][j] + 1, C[i][j-1] + 1)
 * and D(e) = C[m][e].  A strand-1 record aligns the reverse complement of its query exactly as SUFR_EDIT_BOTH_STRANDS forms it.
 *
 *   alignment  of a record (query, strand, end, edits): let e = end + 1 and walk back from (m, e).  At (i, j) with i > 0 take
 *              the first move that applies:
 *                1. diagonal, to (i-1, j-1), when j > 0 and C[i-1][j-1] + [Q[i-1] != T[j-1]] == C[i][j]; the op is '=' on
 *                   equal bytes and 'X' otherwise
 *                2. up, to (i-1, j), when C[i-1][j] + 1 == C[i][j]; the op is 'I': a query byte with no text byte
 *                3. left, to (i, j-1); the op is 'D': a text byte with no query byte
 *              and stop at i = 0.
 *   start      the j reached: the alignment covers T[start .. e).
 *   CIGAR      the ops in forward order (the last move made comes first), run-length encoded.
 * One rule and one path per record: the host, the device and any other implementation of the rule agree byte for byte.
 * What follows from the rule: the lengths of the X, I and D runs add up to `edits`; start plus the lengths of the =, X and D
 * runs is e; the =, X and I lengths add up to m; the first op is never D, and I only when start == 0; the last op is D only
 * where D(e - 1) < D(e): on a SUFR_EDIT_LOCAL_MINIMA record only when e - 1 is no record, which takes an array that leaves
 * positions out or a max_occ (with max_occ == 0 on an index with s == n, never).
 *
 * Outputs, for num_records records:
 *   start      u64[num_records]
 *   cigar_off  u64[num_records + 1], cigar_off[0] = 0: record t owns cigar[cigar_off[t] .. cigar_off[t + 1])
 *   cigar      u32[]: BAM encoding, len << 4 | op with the op codes I = 1, D = 2, '=' = 7, X = 8; adjacent runs of a record
 *              never share an op (a run longer than 2^28 - 1 does not fit the encoding: queries that long are not supported)
 *
 * Checks.  SUFR_HIP_E_INVALID, with the index of the first offending record in the error text, for a record with
 * query >= num_queries, strand > 1, end >= n, edits > SUFR_EDIT_MAX_EDITS, m < edits + 1 (the rule that gives such a query no
 * records) or edits != D(end + 1).  The last one costs nothing: the table is computed on the 2 * edits + 1 diagonals around
 * the end cell's, which is exact when edits == D(end + 1); a band narrower than the true D reads above `edits` in the end
 * cell and a wider one reads the true D.  Records need not be sorted and may repeat.
 *
 * Capacity.  With cigar_cap below the total the call returns SUFR_HIP_E_CAPACITY, *total_out is the total, start and
 * cigar_off are complete, and cigar is never written at or beyond cigar_cap (its contents are otherwise unspecified).
 * cigar_cap = 0 with a null cigar is the sizing call.
 *
 * The calls read the text only: files and indexes built with a seed mask or with -m are accepted.  Batches use the layout of
 * sufr_file_search_batch.
 */
#ifndef SUFR_ALIGN_H
#define SUFR_ALIGN_H
#include <stddef.h>
#include <stdint.h>

#include "sufr_edit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- host: `threads` workers (0: one per core) share the query bytes; err (errlen bytes, may be null) receives the text of
 * an error ------------------------------------------------------------------------------------------------------------- */
int sufr_file_edit_trace(const sufr_file *f, const uint8_t *queries, const uint64_t *offsets, uint64_t num_queries,
                         uint64_t num_records, const uint64_t *query, const uint8_t *strand, const uint64_t *end,
                         const uint8_t *edits, uint64_t cigar_cap, uint64_t *start, uint64_t *cigar_off, uint32_t *cigar,
                         uint64_t *total_out, int threads, char *err, size_t errlen);

/* ---- device: the index of sufr_hip_index_load / sufr_hip_index_wrap ---------------------------------------------
 * _edit_trace_device takes device pointers and enqueues on the context's stream.  It synchronises twice: once after the
 * checks that need no table, for the longest query among the records (it sizes the chunks the records are traced in),
 * and once for the CIGAR total and the validity flag; the outputs are complete on return.
 * One record per lane keeps two 32-bit words per query byte in the context's row storage; records are traced in chunks of as
 * many as fit.  m is limited only by 64 records having to fit: otherwise the call returns SUFR_HIP_E_NOMEM with the sizes in
 * the error text.
 * _edit_trace takes host buffers and returns when the outputs are there. */
int sufr_hip_edit_trace_device(sufr_hip_ctx *ctx, const sufr_hip_index *ix, const void *d_queries, const void *d_offsets,
                               uint64_t num_queries, uint64_t num_records, const void *d_query, const void *d_strand,
                               const void *d_end, const void *d_edits, uint64_t cigar_cap, void *d_start, void *d_cigar_off,
                               void *d_cigar, uint64_t *total_out);
int sufr_hip_edit_trace(sufr_hip_ctx *ctx, const sufr_hip_index *ix, const uint8_t *queries, const uint64_t *offsets,
                        uint64_t num_queries, uint64_t num_records, const uint64_t *query, const uint8_t *strand,
                        const uint64_t *end, const uint8_t *edits, uint64_t cigar_cap, uint64_t *start, uint64_t *cigar_off,
                        uint32_t *cigar, uint64_t *total_out);

/* the byte budget of the context's row storage (0: the default, 256 MiB); small values make a call take several chunks */
int sufr_hip_set_trace_scratch(sufr_hip_ctx *ctx, uint64_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* SUFR_ALIGN_H */
