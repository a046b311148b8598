/*
 * sufr_fm.h -- an FM-index over the BWT of the indexed text: backward search and locate without the text and without the
 * suffix array, on the host and on the GPU (part of libsufr_hip.so).  It is built from the arrays of
 * sufr_bwt.h and owns everything it reads afterwards: the file may be closed, the device index freed and wrapped tensors
 * overwritten.  At DNA and 32-bit positions it takes 1.71 bytes per rank with every 32nd suffix kept, against the 5 of text
 * and suffix array.
 *
 * Definitions.  T, n, SA[0..s), the index width w, BWT, counts and C are exactly as in sufr_bwt.h; e = T[n - 1], the end byte.
 *   Valid inputs   s == n (every position indexed), no seed mask, built without max_query_len, and counts[e] == 1.  Everything
 *         else is refused with SUFR_HIP_E_UNSUPPORTED: a --dna index that leaves positions out, a seed-mask index, a capped
 *         one, a text whose last byte occurs twice.  With e occurring once, any two suffixes differ at or before the first e
 *         either of them holds, so the order of the suffixes needs no wrap-around and cX < cY iff X < Y for every byte c:
 *         C[c] + occ(c, .) is exact for every byte value, whatever value e has.  The sequence delimiter is not special.  The
 *         one false statement of the BWT is the cyclic row (SA[r] == 0, BWT[r] == e); the rule on e below and the kept
 *         position 0 keep it out of every answer.
 *   occ(c, r) = #{ j < r : BWT[j] == c } for 0 <= r <= s.
 *   Search    the byte strings exactly as sufr_file_search_batch takes them.  For P[0..m): [C[P[m-1]], C[P[m-1]] + counts[P[m-1]]),
 *         then for i = m - 2 .. 0, with c = P[i]: lo = C[c] + occ(c, lo), hi = C[c] + occ(c, hi).  Empty as soon as lo == hi;
 *         empty for a byte that does not occur in the text, and where e stands anywhere in P but at its last place.  The empty
 *         answer is lo == hi == 0.  The range equals that of sufr_file_search_batch / sufr_hip_search_batch_device without a
 *         max_query_len, for every query; that includes the empty query (m == 0), whose range there is every rank, [0, s).
 *   Samples   sample = q >= 1 keeps SA[r] of the ranks with SA[r] % q == 0, in rank order, w bytes each.  A mark bit per rank
 *         and the number of marks in front of every 64 ranks turn a marked rank into its slot.  SA[r]: k = 0; while r is
 *         unmarked, r = C[BWT[r]] + occ(BWT[r], r) and k++; then kept[slot(r)] + k -- fewer than q steps.  sample == 0 keeps
 *         nothing, and locate on such an index is SUFR_HIP_E_UNSUPPORTED.
 *   Locate    the contract of sufr_hip_locate_batch_device (sufr_query.h): for query i the positions SA[lo_i .. min(hi_i, lo_i
 *         + max_hits)) in rank order (max_hits 0: all) in positions[offsets[i] .. offsets[i+1]); offsets holds num_queries + 1
 *         u64, positions up to `cap` entries of width w.  *total_out = offsets[num_queries] even when it exceeds cap; the
 *         call then returns SUFR_HIP_E_CAPACITY and fills no position.  The ranges are those a search returned.
 *   Layout    blocks of `stride` bytes: the K counts (w bytes each, K: the byte values that occur) at the block's first rank,
 *         then `block` = B bytes of the BWT; marks of 16 bytes per 64 ranks; the kept values (sufr_fm_scan.h).  K <= 8 at
 *         w == 4: 32 + 96 bytes in one aligned 128-byte line.  sufr_fm_info.bytes is all of it with the tables of C.
 *         The file it is saved to and loaded from, and the text samples it may also keep, are in sufr_fm_text.h.
 *
 * k-mismatch search by backtracking (declared in sufr_fm_approx.h).  For a query Q[0..m) and d = max_mismatches <=
 * SUFR_FM_APPROX_MAX_MISMATCHES; fm_byte_ok(c, t, m) says that byte c may stand at place t: it occurs in the text, and it is
 * e only where t == m - 1.
 *   Node      (t, lo, hi, h): [lo, hi) is the rank range of a string X[t+1..m) with X[j] == Q[j] at all but h places.  The root
 *         is (m - 1, 0, s, 0).  One step with byte c gives lo' = C[c] + occ(c, lo) and hi' = C[c] + occ(c, hi); from [0, s)
 *         that is [C[c], C[c + 1]).  An empty range ends the branch.
 *   Expanding a node with t >= 0.  If h < d: every byte value c != Q[t] that occurs and has fm_byte_ok(c, t, m), in ascending
 *         order; each child (t - 1, ., ., h + 1) is expanded completely before the next.  After them the exact child with
 *         c = Q[t], if fm_byte_ok(Q[t], t, m).  At every place the substitutions come before the exact continuation.
 *   Leaf      a node with t == -1: (lo, hi, h).  The leaf ranges of one query are disjoint, because different substitution
 *         sets spell different strings: every alignment appears once and nothing is deduplicated.  A leaf gives the records
 *         (query, strand, position = SA[r], mismatches = h) for r = lo .. hi - 1, SA[r] by the sampled walk of Samples.
 *   Order     (query, strand, leaf in the order above, rank), as four parallel arrays with the types of sufr_approx.h: query
 *         u64, strand u8, position u64, mismatches u8.
 *   Special   m == 0 gives no records.  m <= d is legal and allows up to m substitutions (sufr_file_approx refuses such
 *         queries).  e can be the substituted byte only at place m - 1: the window that ends at n.  A query byte that does not
 *         occur in the text can only be substituted.
 *   SUFR_FM_APPROX_BOTH_STRANDS  the rule of SUFR_MEM_BOTH_STRANDS: the query is searched again as its reverse complement and
 *         those records carry strand 1.
 *   Equality  for every query with m >= d + 1 the record set is that of sufr_file_approx with max_occ == 0 on the same file
 *         (complete there: s == n, no seed mask, no cap).
 *   Errors    d > SUFR_FM_APPROX_MAX_MISMATCHES: SUFR_HIP_E_INVALID.  An index built with sample == 0: SUFR_HIP_E_UNSUPPORTED.
 *         *total_out is always the record count; when it exceeds cap the call returns SUFR_HIP_E_CAPACITY and fills nothing.
 */
#ifndef SUFR_FM_H
#define SUFR_FM_H
#include <stddef.h>
#include <stdint.h>

#include "sufr_bwt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sufr_fm sufr_fm;             /* host */
typedef struct sufr_hip_fm sufr_hip_fm;     /* device */
typedef struct sufr_fm_info {
    uint64_t ranks, symbols /* K */, block /* B */, stride, sample, samples, bytes;
    uint32_t width, end_byte;
} sufr_fm_info;

/* ---- host: `threads` workers (0: one per core) take whole tiles of blocks for the build and queries or hits for the rest;
 * no result depends on the number of workers. */
int  sufr_file_fm_build(const sufr_file *f, uint64_t sample, sufr_fm **out, int threads);
void sufr_fm_free(sufr_fm *fm);
int  sufr_fm_get_info(const sufr_fm *fm, sufr_fm_info *info);
/* queries: the concatenated bytes, offsets: num_queries + 1; rank_lo, rank_hi: num_queries each */
int  sufr_fm_search_batch(const sufr_fm *fm, const uint8_t *queries, const uint64_t *offsets, uint64_t num_queries,
                          uint64_t *rank_lo, uint64_t *rank_hi, int threads);
/* offsets: num_queries + 1; positions: cap entries of the index width */
int  sufr_fm_locate_batch(const sufr_fm *fm, const uint64_t *rank_lo, const uint64_t *rank_hi, uint64_t num_queries, uint64_t max_hits,
                          uint64_t *offsets, void *positions, uint64_t cap, uint64_t *total_out, int threads);

/* ---- device.  The build runs on the context's stream with the tiles of sufr_hip_set_bwt_tile (cut down to whole blocks and
 * whole mark words) and synchronises three times: for the byte counts and the end byte, for the number of samples (not with
 * sample == 0), and at its end, after which nothing reads the index `ix` any more.  Two builds give the same bytes.  The
 * object lives on the device of `ctx` and is used with a context of that device. */
int  sufr_hip_fm_build(sufr_hip_ctx *ctx, const sufr_hip_index *ix, uint64_t sample, sufr_hip_fm **out);
void sufr_hip_fm_free(sufr_hip_fm *fm);
int  sufr_hip_fm_get_info(const sufr_hip_fm *fm, sufr_fm_info *info);
/* d_queries / d_offsets as sufr_hip_search_batch_device takes them; d_rank_lo, d_rank_hi: num_queries u64 each.  Enqueued only,
 * on the context's stream (complete after sufr_hip_synchronize). */
int  sufr_hip_fm_search_batch_device(sufr_hip_ctx *ctx, const sufr_hip_fm *fm, const void *d_queries, const void *d_offsets,
                                     uint64_t num_queries, void *d_rank_lo, void *d_rank_hi);
/* One synchronisation, for the total; the walk is enqueued on the context's stream. */
int  sufr_hip_fm_locate_batch_device(sufr_hip_ctx *ctx, const sufr_hip_fm *fm, const void *d_rank_lo, const void *d_rank_hi,
                                     uint64_t num_queries, uint64_t max_hits, void *d_offsets, void *d_positions, uint64_t cap,
                                     uint64_t *total_out);

#ifdef __cplusplus
}
#endif
#endif /* SUFR_FM_H */
