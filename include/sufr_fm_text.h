/*
 * sufr_fm_text.h -- the FM-index of sufr_fm.h as a self-contained object: text samples with which any range of the text is
 * read back from the BWT (extract), a file the index is saved to and loaded from without a .sufr, and copies between host and
 * device (part of libsufr_hip.so).  T, n, s == n, SA, BWT, C, occ, e = T[n - 1], w, q = sample, the
 * marks and `kept` are exactly as in sufr_fm.h.  ISA[p] is the rank r with SA[r] == p.
 *
 * Text samples.  SUFR_FM_TEXT asks the build to keep, beside everything else,
 *         text_kept[k] = the rank r with SA[r] == k q,   k = 0 .. samples - 1,   samples == ceil(n / q),   w bytes each.
 *         These are exactly the marked ranks: a rank that stores SA[r] into `kept` stores r into text_kept[SA[r] / q].  The
 *         cost is w / q bytes per rank (0.125 at w == 4, q == 32, which makes 1.83 bytes per rank at DNA).  SUFR_FM_TEXT with
 *         sample == 0 is SUFR_HIP_E_INVALID.  sufr_fm_info.bytes keeps its meaning and does not count them;
 *         sufr_fm_text_info does.  With flags == 0 the two *_build_flags calls are sufr_file_fm_build / sufr_hip_fm_build.
 *
 * Extract.
 *   Requests  request i is (starts[i], ends[i]), two u64 arrays.  It is clipped: end' = min(end, n), start' = min(start, end').
 *   Output    T[start' .. end') at bytes[offsets[i] .. offsets[i + 1]); offsets holds num + 1 u64 and offsets[0] == 0.
 *         *total_out = offsets[num] always; when it exceeds `cap` the call returns SUFR_HIP_E_CAPACITY and fills no byte (the
 *         offsets are filled, as locate does).  An index built without SUFR_FM_TEXT answers SUFR_HIP_E_UNSUPPORTED.
 *   Reading   the byte of position p is BWT[ISA[p + 1]], and one LF step, r -> C[BWT[r]] + occ(BWT[r], r), goes from
 *         ISA[p + 1] to ISA[p].  The range is cut at the multiples of q into chunks [k q, (k + 1) q).  Chunk k starts at rank
 *         text_kept[k + 1], which stands for position top = (k + 1) q, when (k + 1) q < n; otherwise at rank text_kept[0],
 *         which stands for position top = n (below).  From there the walk takes top - min(end', top) silent steps and then
 *         emits one byte per step down to max(start', k q).  No chunk walks more than q steps, whatever the length of the
 *         request, and chunks are independent.
 *   The cyclic row.  text_kept[0] is the rank r with SA[r] == 0, the one row whose BWT byte is a false statement about the
 *         suffixes: BWT[r] == e is T[n - 1], the byte in front of position n.  So the row stands for position n: its BWT byte
 *         is the byte of position n - 1, and its LF step, C[e] + occ(e, r) = C[e] (e occurs once, so no rank in front of r
 *         holds it), is the rank of the suffix n - 1, the only one that starts with e.  This is the one place where the
 *         cyclic row is stepped through on purpose; search and locate keep it out of every answer (sufr_fm.h).
 *
 * The index file (little-endian; every section starts on a multiple of 4096 bytes; all padding is zero).
 *   Header    0 "SUFRFMI\0" | 8 u32 version = 1 | 12 u32 flags (SUFR_FM_TEXT) | 16 u32 w | 20 u32 e | 24 u32 K | 28 u32 B |
 *         32 u32 stride | 36 u32 cbytes | 40 u64 s | 48 u64 q | 56 u64 samples | 64 u64 sequences | 72 seven (u64 offset,
 *         u64 length) pairs, one per section in the order below | zeros up to 4096.
 *   Sections  tables: C (257 u64) then the columns (256 u32, 0xFFFFFFFF: the byte value does not occur); sequence starts
 *         (u64 each); sequence names (each ended by a 0 byte); blocks ((s / B + 1) stride bytes); marks (ceil(s / 64) times
 *         (u64 bits, u64 before)); kept (samples w bytes); text_kept (samples w bytes with SUFR_FM_TEXT, else empty).
 *         offset[0] == 4096, offset[i + 1] == offset[i] + length[i] rounded up to 4096, and the file ends at offset[6] +
 *         length[6].  Checkpoint bytes behind K w and BWT bytes behind s are zero: the file of an index is one fixed byte
 *         string, whichever side built it.
 *   Names     sufr_fm_save with `names_from` stores the sequence starts and names of that .sufr; with NULL it stores those the
 *         index remembers -- an index built from a file or loaded from one remembers them, a downloaded one has none until
 *         sufr_fm_set_sequences gives it some (num == 0: none).
 *   Load      reads into owned memory and verifies the file, so that no later search or walk reads outside its arrays
 *         whatever the file holds.  I/O failures are SUFR_HIP_E_IO, everything else SUFR_HIP_E_INVALID with a message that
 *         names the failed check:
 *         header   magic, version, flags; w in {4, 8}; the shape equals fm_shape(K, w); every section's offset and length
 *                  equal their formulas; the file length equals the end of the last section;
 *         tables   the columns are the K occurring byte values numbered in ascending order; C[0] == 0, C is non-decreasing
 *                  and C[256] == s; C[e + 1] - C[e] == 1;
 *         sequences  the starts do not decrease and lie below s; there is one name per start;
 *         blocks   (one streaming pass, workers over tiles) every BWT byte in front of s has a column; every checkpoint equals
 *                  the running count; the final counts equal the differences of C; the bytes behind s and the checkpoint
 *                  bytes behind K w are zero;
 *         marks    `before` is the running popcount, its total equals samples, no bit is set behind s;
 *         kept     every value is a multiple of q and below s, and 0 is among them;
 *         text_kept  text_kept[k] is a marked rank below s and kept[slot(text_kept[k])] == k q.
 *         After these checks occ is exact for the stored bytes, every LF step lands in [0, s), and every walk is bounded by q.
 */
#ifndef SUFR_FM_TEXT_H
#define SUFR_FM_TEXT_H
#include <stddef.h>
#include <stdint.h>

#include "sufr_fm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SUFR_FM_TEXT 0x1u                   /* build flag: keep the text samples */

typedef struct sufr_fm_text_info {
    uint64_t text_samples;                  /* entries of text_kept (0 without SUFR_FM_TEXT) */
    uint64_t text_bytes;                    /* text_samples * w */
    uint64_t file_bytes;                    /* the length of the file sufr_fm_save writes with the names the index remembers */
} sufr_fm_text_info;

/* ---- host.  `threads` as in sufr_fm.h; no result depends on the number of workers. */
int  sufr_file_fm_build_flags(const sufr_file *f, uint64_t sample, uint32_t flags, sufr_fm **out, int threads);
int  sufr_fm_get_text_info(const sufr_fm *fm, sufr_fm_text_info *info);
/* starts, ends: num u64 each; offsets: num + 1 u64; bytes: cap bytes.  Workers take chunks. */
int  sufr_fm_extract_batch(const sufr_fm *fm, const uint64_t *starts, const uint64_t *ends, uint64_t num, uint64_t *offsets,
                           uint8_t *bytes, uint64_t cap, uint64_t *total_out, int threads);
int  sufr_fm_save(const sufr_fm *fm, const char *path, const sufr_file *names_from /* may be NULL */, char *err, size_t errlen);
int  sufr_fm_load(const char *path, sufr_fm **out, int threads, char *err, size_t errlen);
uint64_t sufr_fm_num_sequences(const sufr_fm *fm);
uint64_t sufr_fm_sequence_start(const sufr_fm *fm, uint64_t i);          /* i < sufr_fm_num_sequences */
const char *sufr_fm_sequence_name(const sufr_fm *fm, uint64_t i);        /* owned by the index */
/* replaces the sequences the index remembers: starts must not decrease and lie below the number of ranks */
int  sufr_fm_set_sequences(sufr_fm *fm, const uint64_t *starts, const char *const *names, uint64_t num);

/* ---- device.  The build is that of sufr_hip_fm_build with one more launch behind k_fm_samples when SUFR_FM_TEXT is set; it
 * uses no atomics, so two builds give the same bytes. */
int  sufr_hip_fm_build_flags(sufr_hip_ctx *ctx, const sufr_hip_index *ix, uint64_t sample, uint32_t flags, sufr_hip_fm **out);
int  sufr_hip_fm_get_text_info(const sufr_hip_fm *fm, sufr_fm_text_info *info);
/* d_starts, d_ends: num u64 each; d_offsets: num + 1 u64; d_bytes: cap bytes, all on the device.  One synchronisation, for the
 * totals; everything else is enqueued on the context's stream.  Two calls give the same bytes. */
int  sufr_hip_fm_extract_batch_device(sufr_hip_ctx *ctx, const sufr_hip_fm *fm, const void *d_starts, const void *d_ends, uint64_t num,
                                      void *d_offsets, void *d_bytes, uint64_t cap, uint64_t *total_out);
/* the same with host pointers; complete on return */
int  sufr_hip_fm_extract_batch(sufr_hip_ctx *ctx, const sufr_hip_fm *fm, const uint64_t *starts, const uint64_t *ends, uint64_t num,
                               uint64_t *offsets, uint8_t *bytes, uint64_t cap, uint64_t *total_out);
/* Allocations and copies only: neither the text nor a suffix array is ever on the device.  Complete on return. */
int  sufr_hip_fm_upload(sufr_hip_ctx *ctx, const sufr_fm *fm, sufr_hip_fm **out);
/* The downloaded index remembers no sequences.  Saved, it is the file of the host build of the same .sufr at the same sample
 * and flags saved without names. */
int  sufr_hip_fm_download(sufr_hip_ctx *ctx, const sufr_hip_fm *fm, sufr_fm **out);

#ifdef __cplusplus
}
#endif
#endif /* SUFR_FM_TEXT_H */
