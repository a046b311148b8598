"""Query answers at text positions beyond 2^31 and 2^32 without a multi-gigabyte build (a helper, not a test module).

A suffix array may index only some positions of its text (that is what a --dna build leaves behind, with the bitmap of the
indexed positions).  So a text can be a long filler of 0x00 that is not indexed, followed by a small indexed region that
ends in `$` at the end of the text.  Suffix comparisons never look left of a suffix's start and the region is the tail of the
text, so the order of its suffixes (and their LCPs) is that of the region alone: SA = SA(region) + filler.  Every query answer
is then translation-invariant: against a twin text of a short filler plus the same region, rank ranges, lengths, distances and
CIGARs are equal and every text position differs by the same constant.

The precondition is the twin's filler: TWIN_FILLER bytes exceed the longest query (MAX_QUERY) plus 15 edits plus the 8-byte
loads, so every window, left-extension check and traceback that reaches left of the region sees filler in both texts, never
the start of the text.  The filler byte is 0x00 because a file hole reads as zeros: on the host the filler is a hole in a
sparse file that the reader maps, on the device one torch.zeros.

  region()          the 40 000-byte region with its SA and LCP (the oracle's), built once
  GEOMETRIES        twin, u32_across_2_31, u32_top, u64_across_2_32: filler and index width; the boundary is the region's middle
  write_sparse()    the version-6 .sufr file of a geometry, the filler never written
  batch()           the queries, the same for every geometry
  answers()         every host operation on a SufrFile as a dict of plain lists, text positions shifted back to the twin's
  compare()         exact equality of two such dicts, the first difference in the message
  assert_witness_is_not_empty()   records on both sides of the boundary, spans over it, all four CIGAR operations

Repeats (include/sufr_repeat.h) get a region of their own.  The one place where the sequence starts enter a repeat is the
clip l[r] = min(LCP[r], d(SA[r-1]), d(SA[r])), d(p) = brk(p) - p, and the region above has no rank at which l[r] < LCP[r]: its two
`%` are followed by unrelated random text, so no two suffixes agree through a break and a wrong d() changes no answer there.
repeat_region() is the same text with the 61 bytes around the first `%` copied over those around the second, so that suffixes
on both sides of the boundary agree through a `%`, and the repeat files have two more sequence starts that no byte marks,
inside the first and the third copy of the planted segment (the sequence starts are positional: sufr_repeat.h), which cut
its 1200-byte repeat.  Every rank range, count, length and stat is translation-invariant as above; the left symbol of the
region's first position is the filler byte in every geometry.

  repeat_region()   that region with its SA and LCP (the oracle's), built once
  REPEAT_GEOMETRIES the four fillers and widths again, with the five sequence starts (REPEAT_NAMES)
  repeat_answers()  the records, stats and occurrences of every kind and filter of REPEAT_FILTERS as plain lists
  repeat_witness()  the twin's repeat answers, held to the serial witness of tests/test_repeat_host.py and shown not to be empty
  assert_repeat_witness_is_not_empty()   records on both sides of and across the boundary, clipped ranks decided from either side

The sequence counts and the k-common profile (include/sufr_shared.h) and the longest previous factors and the LZ77 parse
(include/sufr_lz.h) use the repeat region and its five sequences as they are: LPF is clipped by d(p), and seqs is only worth
comparing with several sequences on either side of the boundary.  Of all analyses these two depend most on absolute
positions: LPF compares them (SA[j] < p), scatters by them (lpf[p], src[p]) and returns them (src), the parse walks them, and
seqs is decided by doc(SA[r]), a bisection of the sequence starts.  Rank, count, length, seqs, the stats, the profile, LPF
and the parse's longest factor are translation-invariant; occurrences, SRC and longest_start differ by the shift, and every
filler position is one more literal: factors and literals grow by the shift.

Host LPF and LZ output by position is left out at the large geometries, for the reason given for k-mers in answers():
sufr_file_lpf fills n entries per array (17 to 34 GB) and sufr_file_lz walks two n-entry u64 vectors (69 GB).  What the host
and the kernels share of it, lz_rank of sufr_lz_scan.h, needs no n-entry array and is run on the shifted arrays through
tests/lz_shim.cpp (tests/test_query_high_positions.py); the n-entry outputs are checked on the device.

  SHARED_FILTERS    five filters on length, count and seqs; every one has records of kinds 0 and 1 on the twin
  shared_answers()  the records (with seqs), stats and occurrences of every kind and filter, and the profile under "common"
  shared_witness()  the twin's shared answers, held to the records of repeat_witness(), to len(set(docs)) and to a filter in Python
  lz_answers_by_rank()   LPF and SRC of the region's positions as plain lists, the shift off SRC, no source as -1
  lz_witness()      the twin's LPF, SRC and parse, held to the text alone (witness_lpf_at at lz_sample(), check_parse)
  assert_lz_shared_witness_is_not_empty()   targets, sources and copies on both sides of and across the boundary, positions that
                    the clip decides, every value of seqs, the records whose seqs a truncated position would change

The BWT, its runs and LF (include/sufr_bwt.h) accept every index, so they use the plain region and the four geometries as they
are: BWT[r] = T[SA[r] - 1] reads the filler byte in front of the region's first position, position 0 is never indexed (no
cyclic row), and only `first` = SA[a] of a run record takes the shift.

  bwt_answers()     the BWT bytes and counts, the run records and stats at min_len 1 and 8, LF, as plain lists
  bwt_witness()     the twin's, held to numpy on the arrays (witness() of tests/test_bwt_host.py) and shown not to be empty

The FM-index (include/sufr_fm.h, sufr_fm_approx.h, sufr_fm_text.h, sufr_fm_match.h) refuses an index that leaves positions out,
so there the filler is indexed, and its suffix order is known without sorting.  Let T = 0x00^F region, where the region ends
in `$` and holds no 0x00.  Suffix i < F is 0^(F-i) region: of two of them the one with the longer run of zeros is smaller,
because a zero meets region[0] > 0 there, so ranks 0 .. F-1 are positions 0 .. F-1 in order; the region's suffixes follow in the
order of SA(region), because they are the tail of the text:

  SA(T)   = [0, 1, .., F-1] ++ (SA(region) + F)             every position indexed, `$` once: a valid input with K = 8 byte
  BWT(T)  = `$`, 0^(F-1), then the region's BWT              values (0x00 $ % A C G N T), the one-line block shape at w == 4 and
  LF[0]   = F, LF[r] = r - 1 for 1 <= r < F                  the generic one (64 + 64) at w == 8; the run records start with
                                                             (0, 1, `$`, 0) and (1, F-1, 0x00, 1)

The reversed text of sufr_fm_match.h is reverse(region[:-1]) 0^F `$`, and SA of it is [(R-1)+i for i < F] ++ [n-1] ++
SA(reverse(region[:-1]) + `$`)[1:]: the zeros sort as above (the `$` behind them is larger than a zero), then the `$`, which is
smaller than every byte of the region, and two suffixes that start in the reversed region differ inside it or where the shorter
one meets its first zero, which is where it meets the `$` in the region alone -- the order does not depend on F >= 1.  Both
formulas are held to a sort of the suffixes at F = 1, 7, 500 (tests/test_query_high_positions.py), and SA(region) and
SA(reversed region) are the oracle's, every adjacent pair compared on the text in Python.

Against the twin (F = 4096, shift = F - 4096): every text position differs by the shift; every non-empty rank range of a
query that holds a non-zero byte differs by the shift (such a query occurs only where its non-zero byte meets the region, so
its ranks are F - k for k leading zeros, or the region's); matching statistics, SMEM lengths and offsets, mismatch counts and
extracted bytes are equal; the empty answer lo == hi == 0 is not shifted; a pure-zero query 0^k has the range [0, F - k + 1),
the empty query [0, n): both analytic and asserted apart.  k-mismatch records are translation-invariant for queries of more
than d bytes that fit the twin's filler and hold more than d non-zero bytes: a non-zero query byte then matches a region
byte, so the window starts within a query's length of the region and sees filler to its left in both texts.  Here ranks *and*
positions of the region straddle the boundary at its middle byte: rank F + r and the position of the region's r-th byte are
both 4096 + r on the twin.  symbols=9 sets three bytes of the region to R, which makes K = 9: the wide block shape (64 + 64 in
128) at w == 4.

  full_region()     the region's bytes, SA(region) with every position indexed and SA(reversed region), at 8 or 9 symbols
  FULL_GEOMETRIES   the four fillers and widths again; FULL_SYMBOLS: 9 symbols at twin and u32_across_2_31 only
  full_arrays_host()    text, SA, reversed text and its SA as numpy arrays, for small F; full_host_pair() builds the host pair
  full_sa_tail()    the last R entries of either suffix array at any F: what a device test copies behind an arange
  fm_batch()        about 400 queries and, apart, the pure-zero ones
  fm_answers()      every operation on a pair of indexes, host objects or adapters of device ones, as plain lists
  assert_fm_witness_is_not_empty()   ranges and positions on both sides of the boundary, windows and SMEMs over it, 0 to 3
                    mismatches on both strands, walks of 0 and q - 1 steps, the chunk of the cyclic row, zeros matched in the filler
"""
from __future__ import annotations

import functools
import os
import struct
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from sufr_amd import SufrFile, pack_queries

R = 40_000                      # the region
MID = R // 2                    # its middle byte: the boundary of every geometry lies here
TWIN_FILLER = 4096
MAX_QUERY = 1000
SEG_LEN, SEG_AT = 1200, (3_000, MID - 600, 30_000)      # the planted segment: before, across and after the middle
A_RUN = (MID - 3_000, MID - 2_000)                      # 1 000 A ending 2 000 before the middle
N_RUN = (MID + 5_000, MID + 5_400)                      # 400 N after it: positions that are not indexed
DELIMS = (10_000, 33_000)                               # one % on each side: three sequences
SEQ_NAMES = ("s0", "s1", "s2")
SPARSE_LIMIT = 64 << 20                                 # more blocks than this: the filesystem has no holes
assert TWIN_FILLER > MAX_QUERY + 15 + 8


@dataclass(frozen=True)
class Geometry:
    name: str
    filler: int
    width: int

    @property
    def n(self) -> int:
        return self.filler + R

    @property
    def shift(self) -> int:                             # what a text position is ahead of the twin's
        return self.filler - TWIN_FILLER

    @property
    def boundary(self) -> int:
        return self.filler + MID

    @property
    def seq_starts(self):
        return [0, self.filler + DELIMS[0] + 1, self.filler + DELIMS[1] + 1]


GEOMETRIES = {g.name: g for g in (
    Geometry("twin", TWIN_FILLER, 4),
    Geometry("u32_across_2_31", (1 << 31) - MID, 4),            # n = 2^31 + R/2: positions that are negative in int32
    Geometry("u32_top", (1 << 32) - 2 - R, 4),                  # n = 2^32 - 2: the largest 32-bit text
    Geometry("u64_across_2_32", (1 << 32) - MID, 8),            # n = 2^32 + R/2
)}
LARGE = [name for name in GEOMETRIES if name != "twin"]
WIDTH_FLIP = Geometry("first_64_bit_length", (1 << 32) - 1 - R, 8)   # n = 2^32 - 1: the shortest text with 64-bit arrays
assert GEOMETRIES["u32_across_2_31"].boundary == 1 << 31 and GEOMETRIES["u64_across_2_32"].boundary == 1 << 32
assert GEOMETRIES["u32_top"].n == (1 << 32) - 2 and GEOMETRIES["twin"].n == 44_096


@functools.lru_cache(maxsize=None)
def region(seed: int = 20):
    """text (uint8 array, R bytes ending in $), sa, lcp (uint64 arrays of the indexed positions: A C G T $), built once"""
    from oracle_helper import Oracle
    rng = np.random.default_rng(seed)
    t = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, R)].copy()
    seg = t[SEG_AT[0]:SEG_AT[0] + SEG_LEN].copy()
    for at in SEG_AT:
        t[at:at + SEG_LEN] = seg
    t[A_RUN[0]:A_RUN[1]] = ord("A")
    t[N_RUN[0]:N_RUN[1]] = ord("N")
    t[list(DELIMS)] = ord("%")
    t[-1] = ord("$")
    assert SEG_AT[1] < MID < SEG_AT[1] + SEG_LEN and A_RUN[1] == MID - 2000 and DELIMS[0] < MID < DELIMS[1] and N_RUN[0] > MID
    sa, lcp, _ = Oracle().build(t, is_dna=True)
    assert sa.size == R - (N_RUN[1] - N_RUN[0]) - len(DELIMS)
    t.setflags(write=False)
    return SimpleNamespace(text=t, sa=sa.astype(np.uint64), lcp=lcp.astype(np.uint64))


def arrays(geo: Geometry, reg=None):
    """SA + filler and LCP at the geometry's width (unsigned)"""
    reg = reg or region()
    dt = np.uint32 if geo.width == 4 else np.uint64
    sa = reg.sa + np.uint64(geo.filler)
    assert int(sa.max()) == geo.n - 1 and (geo.width == 8 or int(sa.max()) < 1 << 32)
    return sa.astype(dt), reg.lcp.astype(dt)


def write_sparse(path, geo: Geometry, indexed: bool = True, reg=None, names=SEQ_NAMES) -> int:
    """The version-6 file of the geometry as sufr_file_open parses it: the 60-byte header, the sequence starts at the index
    width, the mask length, text, SA, LCP, names.  Header, region, arrays and names are written at their offsets; the filler
    stays a hole.  indexed=False: the header and the names only (no suffixes).  reg, names: another region than region()
    and the names of the geometry's sequences.  Returns the bytes of disk blocks in use."""
    W = geo.width
    dt = "<u4" if W == 4 else "<u8"
    reg = reg or region()
    assert len(names) == len(geo.seq_starts)
    sa, lcp = arrays(geo, reg) if indexed else (np.zeros(0, dtype=dt), np.zeros(0, dtype=dt))
    starts = np.asarray(geo.seq_starts, dtype=dt)
    text_pos = 60 + starts.size * W + 8
    sa_pos = text_pos + geo.n
    lcp_pos = sa_pos + sa.size * W
    names = struct.pack("<Q", len(names)) + b"".join(struct.pack("<Q", len(s)) + s.encode() for s in names)
    header = bytes([6, 1, 0, 0]) + struct.pack("<7Q", geo.n, text_pos, sa_pos, lcp_pos, sa.size, 0, starts.size)
    assert len(header) == 60
    fd = os.open(str(path), os.O_CREAT | os.O_WRONLY | os.O_TRUNC, 0o644)
    try:
        os.ftruncate(fd, lcp_pos + lcp.size * W + len(names))
        os.pwrite(fd, header + starts.tobytes() + struct.pack("<Q", 0), 0)
        if indexed:
            os.pwrite(fd, reg.text.tobytes(), text_pos + geo.filler)
            os.pwrite(fd, sa.astype(dt).tobytes(), sa_pos)
            os.pwrite(fd, lcp.astype(dt).tobytes(), lcp_pos)
        os.pwrite(fd, names, lcp_pos + lcp.size * W)
    finally:
        os.close(fd)
    return os.stat(str(path)).st_blocks * 512


def open_checked(path, geo: Geometry, indexed: bool = True, reg=None, names=SEQ_NAMES) -> SufrFile:
    f = SufrFile(path)
    assert f.index_width == geo.width and f.text_len == geo.n and f.is_dna, (geo.name, f.index_width, f.text_len)
    assert f.len_suffixes == ((reg or region()).sa.size if indexed else 0)
    assert f.sequence_starts == geo.seq_starts and f.sequence_names == list(names)
    return f


# ---------------------------------------------------------------------------------------------------------------------
# the queries
# ---------------------------------------------------------------------------------------------------------------------
SMALL = 3                       # batch()[:SMALL]: the second batch size of the k-difference sort (its key has fewer bits)
ALIGN_SLICE = slice(0, 50)


def _substitute(rng, read: bytes, rate: float = 0.02) -> bytes:
    q = bytearray(read)
    for j in np.nonzero(rng.random(len(q)) < rate)[0]:
        q[j] = (b"ACGT".replace(bytes([q[j]]), b""))[int(rng.integers(0, 3))] if q[j] in b"ACGT" else ord("A")
    return bytes(q)


@functools.lru_cache(maxsize=None)
def batch(seed: int = 7):
    """About 700 queries: reads of 1-200 symbols cut from the region at 2 % substitutions (every one at least 12 long but
    for a handful, which keeps the records of d = 3 in the tens of thousands), reads over the middle, at both ends of the
    region and beyond the end of the text, reads with an inserted and a deleted symbol, A x 30, the empty query and a
    900-symbol prefix of the planted segment."""
    rng = np.random.default_rng(seed)
    text = region().text.tobytes()
    seg = text[SEG_AT[0]:SEG_AT[0] + SEG_LEN]
    qs = [seg[:900], b"A" * 30, _substitute(rng, text[MID - 60:MID + 70]), b""]            # the first SMALL: see above
    for length in (1, 2, 3, 4, 5, 6, 8, 10):
        at = int(rng.integers(0, R - length))
        qs.append(text[at:at + length])
    for _ in range(600):
        length = int(rng.integers(12, 201))
        at = int(rng.integers(0, R - length + 1))
        qs.append(_substitute(rng, text[at:at + length]))
    for _ in range(40):                                                                     # over the boundary byte
        length = int(rng.integers(20, 201))
        at = MID - int(rng.integers(1, length - 1))
        qs.append(_substitute(rng, text[at:at + length]))
    for length in (16, 40, 150):                                                            # the ends of the region
        qs += [text[:length], b"ACGT" + text[:length], text[R - length:], text[R - length:] + b"ACGT", text[R - length:R - 1]]
    for _ in range(12):                                                                     # I and D in the CIGARs
        length = int(rng.integers(60, 181))
        at = int(rng.integers(0, R - length + 1)) if _ % 3 else MID - length // 2
        q = bytearray(text[at:at + length])
        del q[length // 3]
        q.insert(2 * length // 3, b"ACGT"[(b"ACGT".index(q[2 * length // 3]) + 1) % 4] if q[2 * length // 3] in b"ACGT" else ord("C"))
        qs.append(bytes(q))
    assert max(len(q) for q in qs) <= MAX_QUERY
    return tuple(qs)


# ---------------------------------------------------------------------------------------------------------------------
# the answers
# ---------------------------------------------------------------------------------------------------------------------
SEARCH_MQL = (None, 6)
LOCATE_HITS = (0, 3)
SMEM_COMBOS = ((12, 4), (1, 0))                         # (min_len, max_hits)
MEM_COMBOS = ((15, 0, True), (15, 5, False))            # (min_len, max_occ, both strands)
APPROX_COMBOS = ((3, 0, True), (1, 50, False))          # (d, max_occ, both strands)
EDIT_COMBOS = ((3, 0, True, False), (3, 0, True, True)) # (d, max_occ, both strands, local minima)
KMER_KS = (1, 21, 64)
KMER_BINS = 64


def _ints(a, shift: int = 0):
    if hasattr(a, "cpu"):                               # (a torch tensor, wherever it lives)
        a = a.cpu().numpy()
    return (np.asarray(a).astype(np.int64) - shift).tolist()


def hit_ranges(lo, hi, max_hits: int):
    """(offsets, ranks) of the first max_hits ranks (0: all) of every range"""
    lo, hi = np.asarray(lo).astype(np.int64), np.asarray(hi).astype(np.int64)
    cnt = hi - lo
    if max_hits:
        cnt = np.minimum(cnt, max_hits)
    off = np.concatenate([[0], np.cumsum(cnt)])
    ranks = np.concatenate([np.arange(a, a + c) for a, c in zip(lo, cnt)] + [np.zeros(0, dtype=np.int64)])
    return off, ranks.astype(np.int64)


def answers(f: SufrFile, shift: int, queries=None) -> dict:
    """Every host operation on the file as plain lists; `shift` is taken off every text-position column (locate and SMEM
    positions, MEM and k-mismatch positions, k-difference ends, traceback starts) and off nothing else.  Output by position
    needs n entries on the host (17 to 34 GB at the large geometries) and is left to the device tests."""
    queries = list(batch() if queries is None else queries)
    qb, off = pack_queries(queries)
    sa = f.suffix_array
    out = {}
    for mql in SEARCH_MQL:
        lo, hi = f.search_batch(queries, mql)
        out[f"search mql={mql}"] = [_ints(lo), _ints(hi)]
        if mql is None:
            for max_hits in LOCATE_HITS:
                o, ranks = hit_ranges(lo, hi, max_hits)
                out[f"locate max_hits={max_hits}"] = [_ints(o), _ints(sa[ranks], shift)]
    out["locate api"] = [[(p.suffix - shift, p.rank, p.sequence_name, p.suffix - p.sequence_position == f.sequence_starts[SEQ_NAMES.index(p.sequence_name)])
                          for p in r.positions] for r in f.locate(queries[SMALL:SMALL + 30])]
    out["matching statistics"] = _ints(np.concatenate(f.matching_statistics(queries)))
    for min_len, max_hits in SMEM_COMBOS:
        qi, qo, ln, lo, hi = f.smem_arrays(qb, off, min_len)
        o, ranks = hit_ranges(lo, hi, max_hits)
        out[f"smems min_len={min_len} max_hits={max_hits}"] = [_ints(qi), _ints(qo), _ints(ln), _ints(lo), _ints(hi), _ints(o), _ints(sa[ranks], shift)]
    for min_len, occ, both in MEM_COMBOS:
        qi, qo, st, ln, pos = f.mem_arrays(qb, off, min_len, occ, both)
        out[f"mems min_len={min_len} max_occ={occ} both={both}"] = [_ints(qi), _ints(qo), _ints(st), _ints(ln), _ints(pos, shift)]
    for d, occ, both in APPROX_COMBOS:
        qi, st, pos, mm = f.approx_arrays(qb, off, d, occ, both)
        out[f"approx d={d} max_occ={occ} both={both}"] = [_ints(qi), _ints(st), _ints(pos, shift), _ints(mm)]
    for d, occ, both, minima in EDIT_COMBOS:
        for count in (len(queries), SMALL):
            sqb, soff = pack_queries(queries[:count])
            recs = f.edit_arrays(sqb, soff, d, occ, both, minima)
            start, coff, cigar = f.edit_trace_arrays(sqb, soff, *recs)
            tag = f"d={d} max_occ={occ} both={both} minima={minima} queries={'all' if count == len(queries) else count}"
            out["edit " + tag] = [_ints(recs[0]), _ints(recs[1]), _ints(recs[2], shift), _ints(recs[3])]
            out["trace " + tag] = [_ints(start, shift), _ints(coff), _ints(cigar)]
    out["align"] = [[(h.query, h.strand, h.end - shift, h.edits, h.start - shift, h.cigar) for h in hits]
                    for hits in f.align(queries[ALIGN_SLICE], 3, 0, True, True)]
    for k in KMER_KS:
        hist, stats, occ = f.kmers(k, KMER_BINS, "rank")
        out[f"kmers k={k}"] = [_ints(hist), sorted(stats.items()), _ints(occ)]
    out["unique lengths"] = _ints(f.unique_lengths())
    return out


def by_position(f: SufrFile, k: int) -> dict:
    """k-mer counts and unique lengths by text position over the region (the twin only: n entries each)"""
    assert f.text_len == GEOMETRIES["twin"].n
    return {f"kmers k={k} by position": _ints(f.kmers(k, KMER_BINS, "position")[2][TWIN_FILLER:]),
            "unique lengths by position": _ints(f.unique_lengths(True)[TWIN_FILLER:])}


def _first_difference(got, want, path=()):
    if isinstance(got, (list, tuple)) and isinstance(want, (list, tuple)):
        for i, (g, w) in enumerate(zip(got, want)):
            d = _first_difference(g, w, path + (i,))
            if d:
                return d
        return (path, f"{len(got)} entries", f"{len(want)} entries") if len(got) != len(want) else None
    return None if got == want else (path, got, want)


def compare(got: dict, want: dict, geometry: str, keys=None):
    """got == want, exactly, key by key; the message names the operation, the geometry, the index of the first difference and
    got / want there (text positions as the twin has them: the shift is already taken off)"""
    for key in (keys if keys is not None else want):
        assert key in got, f"{geometry}: no answer for {key!r}"
        if got[key] != want[key]:
            path, g, w = _first_difference(got[key], want[key])
            raise AssertionError(f"{key} at {geometry}: first difference at index {list(path)}: got {g!r}, want {w!r} (positions shifted to the twin's)")


def assert_witness_is_not_empty(want: dict, queries=None):
    """What keeps a comparison from being empty, decided by the twin's answers alone: every operation with a position column
    has records strictly on both sides of the boundary; MEMs, k-mismatch, k-difference and traceback have a record whose span
    [start, end) holds the boundary byte; the CIGARs hold all of = X I D."""
    from sufr_amd.sufr_file import cigar_string
    queries = list(batch() if queries is None else queries)
    B = GEOMETRIES["twin"].boundary
    lens = np.array([len(q) for q in queries], dtype=np.int64)

    def sides(name, pos):
        pos = np.asarray(pos, dtype=np.int64)
        assert (pos < B).any() and (pos > B).any(), f"{name}: no record on one side of the boundary"

    def spans(name, start, end):                                  # [start, end)
        start, end = np.asarray(start, dtype=np.int64), np.asarray(end, dtype=np.int64)
        assert ((start <= B) & (B < end)).any(), f"{name}: no record spans the boundary byte"

    for key, v in want.items():
        op = key.split()[0]
        if key.startswith("locate max_hits"):
            sides(key, v[1])
        elif op == "smems":
            sides(key, v[6])
        elif op == "mems":
            sides(key, v[4])
            spans(key, v[4], np.asarray(v[4]) + np.asarray(v[3]))
        elif op == "approx":
            sides(key, v[2])
            spans(key, v[2], np.asarray(v[2]) + lens[np.asarray(v[0], dtype=np.int64)])
        elif op == "edit":
            t = want["trace" + key[4:]]
            sides(key, v[2])
            sides("trace" + key[4:], t[0])
            spans(key, t[0], np.asarray(v[2]) + 1)
            if key.endswith("queries=all"):                       # (the slice of SMALL queries: sides and spans only)
                ops = set("".join(c for c in cigar_string(t[2]) if not c.isdigit()))
                assert ops == set("=XID"), (key, ops)
    flat = [h for hits in want["align"] for h in hits]
    assert flat and any(h[4] <= B <= h[2] for h in flat)
    assert any(h[2] < B for h in flat) and any(h[4] > B for h in flat), "align: no record on one side of the boundary"
    assert any(p[0] < B for r in want["locate api"] for p in r) and any(p[0] > B for r in want["locate api"] for p in r)
    assert all(p[3] for r in want["locate api"] for p in r)       # suffix = sequence start + sequence position
    assert {p[2] for r in want["locate api"] for p in r} == set(SEQ_NAMES)
    assert max(want["matching statistics"]) >= 900 and sum(want["kmers k=21"][0]) > 0


# ---------------------------------------------------------------------------------------------------------------------
# repeats: a region with clipped ranks, five sequences (two starts that no byte marks), the answers and their witness
# ---------------------------------------------------------------------------------------------------------------------
COPY = 30                                               # bytes on either side of the first % that also surround the second
POSITIONAL_STARTS = (SEG_AT[0] + 600, SEG_AT[2] + 900)  # inside the first and the third copy of the planted segment
REPEAT_NAMES = ("s0", "s1", "s2", "s3", "s4")
REPEAT_KINDS = (0, 1, 2)
REPEAT_FILTERS = ((1, 2, 0), (12, 2, 0), (25, 2, 0), (20, 3, 0), (1, 2, 2), (SEG_LEN, 2, 0))    # (min_len, min_count, max_count)
REPEAT_MAX_SHOWN = 16                                   # records of at most this many occurrences have a position column
SMALLEST_TILE = 256


@dataclass(frozen=True)
class RepeatGeometry(Geometry):
    @property
    def seq_starts(self):
        return [0] + [self.filler + x for x in (POSITIONAL_STARTS[0], DELIMS[0] + 1, POSITIONAL_STARTS[1], DELIMS[1] + 1)]


REPEAT_GEOMETRIES = {g.name: RepeatGeometry(g.name, g.filler, g.width) for g in GEOMETRIES.values()}
assert SEG_AT[0] < POSITIONAL_STARTS[0] < SEG_AT[0] + SEG_LEN < DELIMS[0] and DELIMS[0] + COPY < SEG_AT[1]
assert SEG_AT[2] < POSITIONAL_STARTS[1] < SEG_AT[2] + SEG_LEN < DELIMS[1] - COPY and N_RUN[1] < SEG_AT[2]


@functools.lru_cache(maxsize=None)
def repeat_region():
    """region() with text[DELIMS[0] - 30 : DELIMS[0] + 31] copied over text[DELIMS[1] - 30 : DELIMS[1] + 31]: text, sa, lcp as
    region() gives them, built once"""
    from oracle_helper import Oracle
    t = region().text.copy()
    t[DELIMS[1] - COPY:DELIMS[1] + COPY + 1] = t[DELIMS[0] - COPY:DELIMS[0] + COPY + 1]
    assert t[DELIMS[1]] == ord("%") and t[-1] == ord("$") and int((t == ord("%")).sum()) == len(DELIMS)
    sa, lcp, _ = Oracle().build(t, is_dna=True)
    assert sa.size == region().sa.size == R - (N_RUN[1] - N_RUN[0]) - len(DELIMS)
    t.setflags(write=False)
    return SimpleNamespace(text=t, sa=sa.astype(np.uint64), lcp=lcp.astype(np.uint64))


def write_repeat_file(path, geo: RepeatGeometry) -> int:
    return write_sparse(path, geo, reg=repeat_region(), names=REPEAT_NAMES)


def open_repeat_file(path, geo: RepeatGeometry) -> SufrFile:
    return open_checked(path, geo, reg=repeat_region(), names=REPEAT_NAMES)


def repeat_key(kind: int, min_len: int, min_count: int, max_count: int) -> str:
    return f"repeats kind={kind} min_len={min_len} min_count={min_count} max_count={max_count}"


def repeat_occurrences(rank, count, occurrences, shift: int):
    """[offsets, positions]: of every record with at most REPEAT_MAX_SHOWN occurrences, SA[rank : rank + count] - shift in
    ascending order; `occurrences` maps an int64 array of ranks to the suffix array's entries there"""
    rank, count = np.asarray(rank).astype(np.int64), np.asarray(count).astype(np.int64)
    shown = count <= REPEAT_MAX_SHOWN
    off, ranks = hit_ranges(rank[shown], rank[shown] + count[shown], 0)
    pos = np.asarray(occurrences(ranks)).astype(np.int64) - shift if ranks.size else np.zeros(0, dtype=np.int64)
    record = np.repeat(np.arange(off.size - 1), np.diff(off))
    return [_ints(off), pos[np.lexsort((pos, record))].tolist()]


def repeat_answers(source, shift: int, occurrences=None, threads: int = 0, filters=REPEAT_FILTERS) -> dict:
    """The repeats of every kind and filter as plain lists: rank, count, length, the stats as sorted items, and the position
    column of repeat_occurrences(), the only one that takes the shift.  source: a SufrFile, or a callable
    (kind, min_len, min_count, max_count) -> (rank, count, length, stats) together with `occurrences` (see above)."""
    if isinstance(source, SufrFile):
        f, sa = source, source.suffix_array
        source = lambda kind, ml, mc, xc: f.repeats(kind, ml, mc, xc, threads=threads)
        occurrences = lambda ranks: np.asarray(sa[ranks])
    out = {}
    for kind in REPEAT_KINDS:
        for ml, mc, xc in filters:
            rank, count, length, stats = source(kind, ml, mc, xc)
            out[repeat_key(kind, ml, mc, xc)] = [_ints(rank), _ints(count), _ints(length), sorted(stats.items())] + \
                repeat_occurrences(_ints(rank), _ints(count), occurrences, shift)
    return out


def clipped_ranks(f: SufrFile):
    """Of the twin: the ranks r >= 1 with l[r] < LCP[r], and for each the positions SA[r-1], SA[r] and their rooms
    brk(p) - p (int64 arrays), from the arrays and the sequence starts alone"""
    from test_repeat_host import brk_of, clipped
    sa = np.asarray(f.suffix_array).astype(np.int64)
    lcp = np.asarray(f.lcp).astype(np.int64)
    room = brk_of(f)[sa] - sa
    r = 1 + np.nonzero(clipped(f)[1:-1] < lcp[1:])[0]
    return r, sa[r - 1], sa[r], room[r - 1], room[r]


def assert_repeat_witness_is_not_empty(want: dict, f: SufrFile) -> dict:
    """What keeps a comparison of repeats from being empty, decided by the twin's file and answers alone (B is the twin's
    boundary).  Returns the counts it looked at."""
    from test_repeat_host import left_codes
    B = REPEAT_GEOMETRIES["twin"].boundary
    assert f.text_len == REPEAT_GEOMETRIES["twin"].n and f.sequence_starts == REPEAT_GEOMETRIES["twin"].seq_starts
    seen = {}
    for kind in REPEAT_KINDS:
        for flt in ((1, 2, 0), (12, 2, 0)):
            assert len(want[repeat_key(kind, *flt)][0]) > 0, (kind, flt)
        # the positional starts cut the planted 1200-byte repeat: the clip at work
        assert want[repeat_key(kind, SEG_LEN, 2, 0)][:3] == [[], [], []], kind
        assert dict(want[repeat_key(kind, SEG_LEN, 2, 0)][3]) == dict(records=0, longest=0, longest_rank=0, max_count=0), kind
        seen[f"records kind={kind}"] = len(want[repeat_key(kind, 1, 2, 0)][0])
        _, _, length, _, off, pos = want[repeat_key(kind, 1, 2, 0)]
        off, pos = np.asarray(off), np.asarray(pos, dtype=np.int64)
        first, last = pos[off[:-1]], pos[off[1:] - 1]                  # (the positions of a record ascend; none has no occurrence)
        assert ((first < B) & (last > B)).any(), f"kind {kind}: no record with occurrences on both sides of the boundary"
    spans = counts = False
    for key, (rank, count, length, _, off, pos) in want.items():
        shown = np.asarray(count) <= REPEAT_MAX_SHOWN
        lens = np.repeat(np.asarray(length, dtype=np.int64)[shown], np.diff(off))
        p = np.asarray(pos, dtype=np.int64)
        spans = spans or bool(((p <= B) & (B < p + lens)).any())
        counts = counts or max(count, default=0) > SMALLEST_TILE
    assert spans, "no occurrence whose span holds the boundary byte"
    assert counts, "no record with more occurrences than the smallest tile has ranks"
    r, p_prev, p_cur, room_prev, room_cur = clipped_ranks(f)
    low_decides = ((room_prev < room_cur) & (p_prev < B) & (p_cur > B)) | ((room_cur < room_prev) & (p_cur < B) & (p_prev > B))
    high_decides = ((room_prev < room_cur) & (p_prev > B) & (p_cur < B)) | ((room_cur < room_prev) & (p_cur > B) & (p_prev < B))
    straddle = (p_prev < B) != (p_cur < B)
    below = np.where(room_prev < room_cur, p_prev, p_cur) < B         # where the position of the smaller room lies
    seen.update({"clipped ranks": int(r.size), "equal rooms": int((room_prev == room_cur).sum()),
                 "the smaller room below the boundary": int((below & (room_prev != room_cur)).sum()),
                 "the smaller room above the boundary": int((~below & (room_prev != room_cur)).sum()),
                 "the smaller room below the boundary, the other position above": int(low_decides.sum()),
                 "the smaller room above the boundary, the other position below": int(high_decides.sum()),
                 "pairs that straddle the boundary": int(straddle.sum())})
    assert all(seen.values()), seen
    assert B not in p_prev and B not in p_cur
    lam = left_codes(f)
    starts = lam[lam >= 256] - 256
    assert 0x00 in lam and ord("N") in lam and np.unique(starts).size >= 4, "left symbols: no filler byte, no N or fewer than four sequence starts"
    seen["sequence starts among the left symbols"] = int(np.unique(starts).size)
    return seen


def repeat_witness(f: SufrFile):
    """(answers, counts): the twin's repeat answers, every key held exactly to the stack pass of tests/test_repeat_host.py
    (which reads nothing of the library but the arrays) and shown not to be empty, and the counts that
    assert_repeat_witness_is_not_empty() looked at"""
    from test_repeat_host import witness_serial
    want = repeat_answers(f, 0)
    sa = np.asarray(f.suffix_array)
    for kind in REPEAT_KINDS:
        for flt in REPEAT_FILTERS:
            rank, count, length, stats = witness_serial(f, kind, *flt)
            serial = [_ints(rank), _ints(count), _ints(length), sorted(stats.items())] + repeat_occurrences(rank, count, lambda ranks: sa[ranks], 0)
            compare(want, {repeat_key(kind, *flt): serial}, "the twin against the serial witness")
    counts = assert_repeat_witness_is_not_empty(want, f)
    return want, counts


# ---------------------------------------------------------------------------------------------------------------------
# sequence counts and the k-common profile, longest previous factors and the LZ77 parse: the repeat region again
# ---------------------------------------------------------------------------------------------------------------------
SHARED_FILTERS = ((1, 2, 0, 0, 0), (12, 2, 0, 2, 0), (20, 3, 0, 0, 1), (1, 2, 0, 5, 0), (8, 2, 0, 3, 4))   # (min_len, min_count, max_count, min_seqs, max_seqs)
LZ_SAMPLE_STEP = 40


def shared_key(kind: int, min_len: int, min_count: int, max_count: int, min_seqs: int, max_seqs: int) -> str:
    return f"shared kind={kind} min_len={min_len} min_count={min_count} max_count={max_count} min_seqs={min_seqs} max_seqs={max_seqs}"


def shared_answers(source, shift: int, occurrences=None, common=None, threads: int = 0, filters=SHARED_FILTERS) -> dict:
    """The shared records of every kind and filter as plain lists: rank, count, length, seqs, the stats as sorted items, and
    the position column of repeat_occurrences(), the only one that takes the shift; under "common" the profile.  source: a
    SufrFile, or a callable (kind, min_len, min_count, max_count, min_seqs, max_seqs) -> (rank, count, length, seqs, stats)
    together with `occurrences` (see repeat_occurrences) and `common`, a callable that returns the profile."""
    if isinstance(source, SufrFile):
        f, sa = source, source.suffix_array
        source = lambda kind, *flt: f.shared(kind, *flt, threads=threads)
        occurrences = lambda ranks: np.asarray(sa[ranks])
        common = lambda: f.common(threads=threads)
    out = {}
    for kind in REPEAT_KINDS:
        for flt in filters:
            rank, count, length, seqs, stats = source(kind, *flt)
            out[shared_key(kind, *flt)] = [_ints(rank), _ints(count), _ints(length), _ints(seqs), sorted(stats.items())] + \
                repeat_occurrences(_ints(rank), _ints(count), occurrences, shift)
    out["common"] = _ints(common())
    return out


def lz_answers_by_rank(lpf_of_region, src_of_region, shift: int) -> dict:
    """LPF and SRC of the region's positions (the last R entries of either array by position; numpy arrays or tensors of the
    index width, signed or not) as plain lists: SRC with the shift taken off, no source (all ones of the width) as -1"""
    def unsigned(a):
        a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
        return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
    lpf, src = unsigned(lpf_of_region), unsigned(src_of_region)
    assert lpf.size == src.size == R and lpf.dtype == src.dtype
    none = src == np.iinfo(src.dtype).max
    return {"lpf of the region": lpf.astype(np.int64).tolist(),
            "src of the region": np.where(none, -1, src.astype(np.int64) - shift).tolist()}


def docs_by_rank(f: SufrFile) -> np.ndarray:
    """the sequence of every rank's position, by bisection of the sequence starts"""
    return np.searchsorted(np.asarray(f.sequence_starts, dtype=np.int64), np.asarray(f.suffix_array).astype(np.int64), side="right") - 1


def _filter_shared(rows, ml, mc, xc, mq, xq):
    """rows of (rank, count, length, seqs) in record order -> the rows a filter keeps and their stats"""
    kept = [(a, c, ln, q) for a, c, ln, q in rows if ln >= ml and c >= max(mc, 2) and (xc == 0 or c <= xc) and q >= mq and (xq == 0 or q <= xq)]
    top = max((ln for _, _, ln, _ in kept), default=0)
    stats = dict(records=len(kept), longest=top, longest_rank=next((a for a, _, ln, _ in kept if ln == top), 0),
                 max_count=max((c for _, c, _, _ in kept), default=0), max_seqs=max((q for _, _, _, q in kept), default=0))
    return kept, stats


def shared_witness(f: SufrFile, repeats: dict = None) -> dict:
    """The twin's shared answers, held to what reads nothing of the library but the arrays: with open filters rank, count and
    length are the records that repeat_witness() has held to the serial stack pass (`repeats`: its answers, computed when
    not given); seqs of every record is len(set(docs[a : a + c])); every filter's answer is that list filtered here, with
    its stats and occurrences; common[q - 1] is the longest record of kind 0 in at least q sequences."""
    from test_shared_host import docs_of
    twin = REPEAT_GEOMETRIES["twin"]
    assert f.text_len == twin.n and f.sequence_starts == twin.seq_starts
    repeats = repeats if repeats is not None else repeat_witness(f)[0]
    want = shared_answers(f, 0)
    docs = docs_of(f)
    assert np.array_equal(docs, docs_by_rank(f))
    sa = np.asarray(f.suffix_array)
    for kind in REPEAT_KINDS:
        rank, count, length, seqs, _ = f.shared(kind, 1, 2, 0, 0, 0)
        rows = list(zip(_ints(rank), _ints(count), _ints(length), _ints(seqs)))
        assert [list(col) for col in zip(*rows)][:3] == repeats[repeat_key(kind, 1, 2, 0)][:3], f"kind {kind}: not the records of repeats"
        for a, c, _, q in rows:
            assert q == len(set(docs[a:a + c].tolist())), (kind, a, c, q)
        for flt in SHARED_FILTERS:
            kept, stats = _filter_shared(rows, *flt)
            cols = [[row[i] for row in kept] for i in range(4)]
            filtered = cols + [sorted(stats.items())] + repeat_occurrences(cols[0], cols[1], lambda ranks: sa[ranks], 0)
            compare(want, {shared_key(kind, *flt): filtered}, "the twin against its own records filtered in Python")
        if kind == 0:
            profile = [max((ln for _, _, ln, q in rows if q >= k), default=0) for k in range(1, len(twin.seq_starts) + 1)]
            assert want["common"] == profile == [1000, 600, 300, 10, 8], (want["common"], profile)
    return want


def lz_sample():
    """the twin's positions at which the text-only witness of LPF is asked: every 40th from 5 before the region on, the 600
    around the boundary, 50 on either side of each of the five sequence starts"""
    twin = REPEAT_GEOMETRIES["twin"]
    some = set(range(twin.filler - 5, twin.n, LZ_SAMPLE_STEP)) | set(range(twin.boundary - 300, twin.boundary + 300))
    for s in twin.seq_starts:
        some |= set(range(max(s - 50, 0), s + 50))
    return sorted(some)


def lz_witness(f: SufrFile) -> dict:
    """The twin's LPF, SRC and parse from the host path, held to the text alone: LPF at lz_sample() equals witness_lpf_at of
    tests/test_lz_host.py (no suffix order, no LCP); every source is an earlier indexed position that spells the same
    bytes, and there is none exactly where LPF is 0; check_parse holds the factors to the greedy walk over that LPF, to the
    text they rebuild and to the breaks.  Returns the answers of lz_answers_by_rank() and, under "lz", start, length,
    source (-1: a literal) and the stats as sorted items."""
    from test_lz_host import FF, check_parse, host_lpf, witness_lpf_at
    twin = REPEAT_GEOMETRIES["twin"]
    assert f.text_len == twin.n and f.sequence_starts == twin.seq_starts
    lpf, src = host_lpf(f)
    some = lz_sample()
    assert np.array_equal(lpf[some], witness_lpf_at(f, some)), "the host's LPF is not the text's at a sampled position"
    assert np.array_equal(src == -1, lpf == 0)
    tb = bytes(f.text)
    indexed = set(np.asarray(f.suffix_array).tolist())
    for p in np.nonzero(lpf)[0].tolist():
        q, ln = int(src[p]), int(lpf[p])
        assert 0 <= q < p and q in indexed and tb[q:q + ln] == tb[p:p + ln], (p, q, ln)
    start, length, source, st = check_parse(f, lpf)
    raw = f.lpf()
    want = lz_answers_by_rank(raw[0][twin.filler:], raw[1][twin.filler:], 0)
    assert want["lpf of the region"] == lpf[twin.filler:].tolist() and want["src of the region"] == src[twin.filler:].tolist()
    want["lz"] = [_ints(start), _ints(length), np.where(source == FF, -1, source.astype(np.int64)).tolist(), sorted(st.items())]
    want["lpf of the twin"], want["src of the twin"] = lpf.tolist(), src.tolist()
    return want


def assert_lz_shared_witness_is_not_empty(f: SufrFile, lz: dict, shared: dict) -> dict:
    """What keeps the comparisons of LPF, the parse and the shared records from being empty, decided by the twin's file and
    answers alone (B is the twin's boundary).  Returns the counts it looked at."""
    from test_repeat_host import brk_of
    twin = REPEAT_GEOMETRIES["twin"]
    B, F = twin.boundary, twin.filler
    assert f.text_len == twin.n and f.sequence_starts == twin.seq_starts
    lpf, src = np.array(lz["lpf of the twin"], dtype=np.int64), np.array(lz["src of the twin"], dtype=np.int64)
    p = np.nonzero(lpf)[0]
    q, ln = src[p], lpf[p]
    room = brk_of(f) - np.arange(twin.n)
    clip = p[ln == room[p]]
    seen = {"lpf nonzero": int(p.size), "lpf nonzero in the filler": int((p < F).sum()), "lpf max": int(lpf.max()),
            "lpf above the boundary, source below": int(((p > B) & (q < B)).sum()),
            "lpf and source above the boundary": int(((p > B) & (q > B)).sum()),
            "lpf and source below the boundary": int(((p < B) & (q < B)).sum()),
            "lpf targets that span the boundary byte": int(((p <= B) & (B < p + ln)).sum()),
            "lpf sources that span the boundary byte": int(((q <= B) & (B < q + ln)).sum()),
            "lpf self-overlapping copies": int((q + ln > p).sum()),
            "lpf decided by the clip": int(clip.size), "lpf decided by the clip above the boundary": int((clip > B).sum()),
            "lpf decided by the clip below the boundary": int((clip < B).sum())}
    start, length, source, st = lz["lz"]
    start, length, source, st = np.array(start, dtype=np.int64), np.array(length, dtype=np.int64), np.array(source, dtype=np.int64), dict(st)
    across = (start <= B) & (B < start + length)
    seen.update({"lz factors": st["factors"], "lz literals of the filler": int((start < F).sum()), "lz literals": st["literals"],
                 "lz longest": st["longest"], "lz longest_start": st["longest_start"], "lz factors that span the boundary byte": int(across.sum()),
                 "lz copies that start below the boundary": int(((source >= 0) & (start < B)).sum()),
                 "lz copies that start above the boundary": int(((source >= 0) & (start > B)).sum())})
    assert (source[start < F] == -1).all() and across.sum() == 1 and int(start[across][0]) == st["longest_start"] and int(length[across][0]) == st["longest"]
    rank, count, _, seqs = (np.array(col, dtype=np.int64) for col in shared[shared_key(0, *SHARED_FILTERS[0])][:4])
    for k in range(1, len(twin.seq_starts) + 1):
        seen[f"shared kind=0 records with seqs={k}"] = int((seqs == k).sum())
    seen["shared kind=0 records with 1 < seqs < count"] = int(((seqs > 1) & (seqs < count)).sum())
    for kind in (0, 1):
        for flt in SHARED_FILTERS:
            assert len(shared[shared_key(kind, *flt)][0]) > 0, (kind, flt)
    # a position of B and more that is truncated to 32 bits at u64_across_2_32 lands in the filler: sequence 0
    sa, docs = np.asarray(f.suffix_array).astype(np.int64), docs_by_rank(f)
    wrapped = np.where(sa >= B, 0, docs)
    seen["shared kind=0 records whose seqs changes if positions from the boundary on read as sequence 0"] = \
        sum(1 for a, c, k in zip(rank.tolist(), count.tolist(), seqs.tolist()) if len(set(wrapped[a:a + c].tolist())) != k)
    assert all(v for key, v in seen.items() if key != "lpf nonzero in the filler") and seen["lpf nonzero in the filler"] == 0, seen
    return seen


# ---------------------------------------------------------------------------------------------------------------------
# the BWT, its runs and LF on the partial-index geometries (include/sufr_bwt.h): the plain region
# ---------------------------------------------------------------------------------------------------------------------
BWT_MIN_LENS = (1, 8)


def bwt_answers(bwt, runs, lf, shift: int) -> dict:
    """The BWT bytes with their 256 counts, the run records at every min_len of BWT_MIN_LENS (rank, length, symbol, first with
    the shift taken off, the stats as sorted items) and LF as plain lists.  bwt() -> (bytes, counts), runs(min_len) -> (rank,
    length, symbol, first, stats) and lf() -> the array are callables over numpy arrays or tensors; everything but `first`
    is translation-invariant."""
    b, counts = bwt()
    out = {"bwt": [_ints(b), _ints(counts)]}
    for min_len in BWT_MIN_LENS:
        rank, length, symbol, first, stats = runs(min_len)
        out[f"bwt runs min_len={min_len}"] = [_ints(rank), _ints(length), _ints(symbol), _ints(first, shift), sorted(stats.items())]
    out["lf"] = _ints(lf())
    return out


def host_bwt_answers(f: SufrFile, shift: int, threads: int = 0) -> dict:
    return bwt_answers(lambda: f.bwt(threads), lambda min_len: f.bwt_runs(min_len, threads), lambda: f.lf(threads), shift)


def bwt_witness(f: SufrFile):
    """(answers, counts): the twin's BWT answers, held to numpy on the arrays (text[sa - 1], np.bincount, a run-length pass and
    a stable argsort: witness() of tests/test_bwt_host.py) and shown not to be empty: run records whose first position lies on
    either side of the boundary, the filler byte in front of the region's first position, N and % among the BWT bytes"""
    from test_bwt_host import witness
    twin = GEOMETRIES["twin"]
    assert f.text_len == twin.n and 0 not in np.asarray(f.suffix_array)           # position 0 is not indexed: no cyclic row
    want = host_bwt_answers(f, 0)
    text, sa = np.asarray(f.text), np.asarray(f.suffix_array)
    for min_len in BWT_MIN_LENS:
        bwt, counts, records, stats, lf = witness(text, sa, min_len)
        numpy = {"bwt": [_ints(bwt), _ints(counts)], "lf": _ints(lf),
                 f"bwt runs min_len={min_len}": [_ints(r) for r in records] + [sorted(stats.items())]}
        compare(want, numpy, "the twin against numpy")
    seen = {}
    for min_len in BWT_MIN_LENS:
        first = np.asarray(want[f"bwt runs min_len={min_len}"][3], dtype=np.int64)
        seen[f"runs min_len={min_len} first below the boundary"] = int((first < twin.boundary).sum())
        seen[f"runs min_len={min_len} first above the boundary"] = int((first > twin.boundary).sum())
    b = np.asarray(want["bwt"][0])
    seen.update({"bwt bytes 0x00": int((b == 0).sum()), "bwt bytes N": int((b == ord("N")).sum()), "bwt bytes %": int((b == ord("%")).sum())})
    assert all(seen.values()) and seen["bwt bytes 0x00"] == 1 and int(sa[np.nonzero(b == 0)[0][0]]) == twin.filler, seen
    return want, seen


# ---------------------------------------------------------------------------------------------------------------------
# the FM-index (include/sufr_fm.h and its companions): the filler is indexed, its suffix order is known without sorting
# ---------------------------------------------------------------------------------------------------------------------
FULL_GEOMETRIES = dict(GEOMETRIES)                      # the same fillers and widths; here ranks *and* positions straddle the boundary
FULL_SYMBOLS = {"twin": (8, 9), "u32_across_2_31": (8, 9), "u32_top": (8,), "u64_across_2_32": (8,)}
assert FULL_GEOMETRIES["u32_across_2_31"].boundary == 1 << 31 and FULL_GEOMETRIES["u64_across_2_32"].boundary == 1 << 32
R_AT = (7_000, MID + 37, 36_000)                        # symbols=9: three bytes set to R, one in each half and one by the middle
FM_SAMPLE = 32
FM_LOCATE_HITS = (0, 3)
FM_APPROX_COMBOS = ((2, True), (3, False))              # (d, both strands)
FM_SMEM_MIN_LENS = (1, 15)
ZERO_PREFIXES = ((1, 40), (5, 16), (37, 150), (100, 40))  # (k, j) of the queries 0^k region[:j]; j > 3: see fm_batch()


def check_suffix_order(t: bytes, sa):
    """every adjacent pair of the array is in the order of the text's suffixes (and the array is a permutation): the arrays
    rest on the text alone.  (4096 bytes decide all but a handful of pairs; the whole suffixes are compared where they do not)"""
    sa = np.asarray(sa).astype(np.int64)
    assert np.array_equal(np.sort(sa), np.arange(len(t)))
    prev = int(sa[0])
    for cur in sa[1:].tolist():
        x, y = t[prev:prev + 4096], t[cur:cur + 4096]
        assert x < y or (x == y and t[prev:] < t[cur:]), (prev, cur)
        prev = cur


@functools.lru_cache(maxsize=None)
def full_region(symbols: int = 8):
    """text (the bytes of region(); symbols=9: with the three bytes at R_AT set to R), sa = SA(text) with every position indexed,
    rtext = reverse(text[:-1]) + $ and rsa = SA(rtext): uint8 and int64 arrays, the order of either array checked pair by pair
    against the text in Python"""
    from oracle_helper import Oracle
    t = region().text.copy()
    if symbols == 9:
        assert all(t[p] in b"ACGT" for p in R_AT) and R_AT[0] < MID - 100 < R_AT[1] < MID + 100 < R_AT[2]
        t[list(R_AT)] = ord("R")
    assert t[-1] == ord("$") and 0 not in t and int((t == ord("$")).sum()) == 1 and np.unique(t).size == symbols - 1   # (0x00 is the filler's)
    rt = np.concatenate([t[:-1][::-1], t[-1:]])
    out = []
    for x in (t, rt):
        sa, _, _ = Oracle().build(x, is_dna=False)
        assert sa.size == R
        check_suffix_order(x.tobytes(), sa)
        out.append(np.asarray(sa).astype(np.int64))
    assert out[0][0] == out[1][0] == R - 1                          # the $ sorts first in both
    t.setflags(write=False); rt.setflags(write=False)
    return SimpleNamespace(text=t, sa=out[0], rtext=rt, rsa=out[1], symbols=symbols)


def full_sa_tail(F: int, symbols: int = 8):
    """(the last R entries of SA(T), the last R entries of SA(reversed T)) for T = 0x00^F region, as int64 arrays.  SA(T) =
    [0 .. F) ++ SA(region) + F; SA(reversed T) = [R - 1 .. R - 1 + F) ++ [n - 1] ++ SA(reversed region)[1:] (see the docstring)"""
    reg = full_region(symbols)
    return reg.sa + F, np.concatenate([[F + R - 1], reg.rsa[1:]]).astype(np.int64)


def full_arrays_host(F: int, symbols: int = 8):
    """text, sa, rtext, rsa of T = 0x00^F region as numpy arrays (uint8, uint32): small F only"""
    reg = full_region(symbols)
    assert 1 <= F < 1 << 24
    tail, rtail = full_sa_tail(F, symbols)
    text = np.concatenate([np.zeros(F, dtype=np.uint8), reg.text])
    rtext = np.concatenate([reg.rtext[:-1], np.zeros(F, dtype=np.uint8), reg.rtext[-1:]])
    sa = np.concatenate([np.arange(F, dtype=np.int64), tail]).astype(np.uint32)
    rsa = np.concatenate([np.arange(F, dtype=np.int64) + (R - 1), rtail]).astype(np.uint32)
    assert np.array_equal(rtext, np.concatenate([text[:-1][::-1], text[-1:]])) and sa.size == rsa.size == F + R
    return text, sa, rtext, rsa


def full_host_pair(directory, F: int, symbols: int = 8, sample: int = FM_SAMPLE, threads: int = 0):
    """(FmIndex of T with text samples, FmIndex of the reversed T without samples) built on the host from the files of
    full_arrays_host(), and the two open files"""
    from test_bwt_host import write_arrays
    text, sa, rtext, rsa = full_arrays_host(F, symbols)
    f = write_arrays(directory / f"full_{F}_{symbols}.sufr", text, sa)
    g = write_arrays(directory / f"full_{F}_{symbols}_rev.sufr", rtext, rsa)
    return f.fm(sample, threads, text=True), g.fm(0, threads), f, g


@functools.lru_cache(maxsize=None)
def fm_batch(symbols: int = 8, seed: int = 11):
    """(queries, pure-zero queries).  About 400 queries: reads of 12 to 200 bytes cut from the region at 2 % substitutions, 40
    of them over the middle byte; the region's first and last 16 / 40 / 150 bytes, with and without the $; 0^k region[:j] for
    ZERO_PREFIXES, plain and with the region's part substituted behind its first byte (so every piece that occurs and is all
    zeros can be extended to the right, and no SMEM is a pure-zero string; j > 3 keeps a non-zero byte matched at d = 3, so a
    window touches the region); $, %, N x 5, A x 30, the empty query; a 900-byte prefix of the planted segment.  The pure-zero
    queries 0^1, 0^5, 0^100 have ranges that are analytic, [0, F - k + 1), not the twin's plus a shift: a list of their own."""
    rng = np.random.default_rng(seed)
    text = full_region(symbols).text.tobytes()
    seg = text[SEG_AT[0]:SEG_AT[0] + SEG_LEN]
    qs = [seg[:900], b"A" * 30, b"", b"$", b"%", b"N" * 5]
    for _ in range(320):
        length = int(rng.integers(12, 201))
        at = int(rng.integers(0, R - length + 1))
        qs.append(_substitute(rng, text[at:at + length]))
    for _ in range(40):                                                                     # over the boundary byte
        length = int(rng.integers(20, 201))
        at = MID - int(rng.integers(1, length - 1))
        qs.append(_substitute(rng, text[at:at + length]))
    for length in (16, 40, 150):                                                            # the ends of the region
        qs += [text[:length], text[R - length:], text[R - length:R - 1]]
    for k, j in ZERO_PREFIXES:
        assert k <= 100 and j > 3
        qs += [bytes(k) + text[:j], bytes(k) + text[:1] + _substitute(rng, text[1:j], 0.05)]
    assert max(len(q) for q in qs) <= MAX_QUERY < TWIN_FILLER
    return tuple(qs), (bytes(1), bytes(5), bytes(100))


def fm_extract_requests(F: int, n: int):
    """(starts, ends) of the fixed extract requests, relative to F and n: across F, 1000 bytes over the middle, over the end of
    the text, behind it, an empty one, the first 64 bytes, 100 bytes deep in the filler, 3000 bytes inside the region, and
    where the text has them the 100 bytes around position 2^31"""
    req = [(F - 50, F + 50), (F + MID - 500, F + MID + 500), (n - 5, n + 5), (n + 3, n + 9), (F + 10, F + 10), (0, 64),
           (F // 2, F // 2 + 100), (F + 5_000, F + 8_000)]
    if n > (1 << 31) + 50:
        req.append(((1 << 31) - 50, (1 << 31) + 50))
    return np.array([a for a, _ in req], dtype=np.uint64), np.array([b for _, b in req], dtype=np.uint64)


FM_PARTS = ("info", "search", "locate", "approx", "ms", "smems", "extract")


def fm_answers(fwd, rev, shift: int, F: int, symbols: int = 8, parts=FM_PARTS, threads: int = 0) -> dict:
    """Every operation on the pair (fwd: the index of T = 0x00^F region with text samples, rev: that of the reversed T) as plain
    lists, for host FmIndex objects and for anything with their methods (tests/test_gpu_fm_high_positions.py wraps a
    DeviceFmIndex).  `shift` is taken off every text position and off both ends of every rank range that is not empty; the
    empty answer (0, 0) stays.  What is analytic is asserted here and not returned: the range of the empty query, [0, n);
    those of the pure-zero queries, [0, F - k + 1); the positions of the ranks [0, 3); every extracted byte."""
    queries, zeros = fm_batch(symbols)
    queries = list(queries)
    qb, off = pack_queries(queries)
    kw = {"threads": threads} if threads else {}
    n = F + R
    reg = full_region(symbols)
    out = {}

    def ranges(lo, hi):
        lo, hi = np.asarray(lo).astype(np.int64), np.asarray(hi).astype(np.int64)
        some = hi > lo
        return np.where(some, lo - shift, lo), np.where(some, hi - shift, hi)

    if "info" in parts:
        info = fwd.info
        assert info["ranks"] == n == rev.info["ranks"]
        out["info"] = [info["symbols"], info["sample"], info["end_byte"], info["ranks"] - shift]
    lo = hi = None
    if {"search", "locate"} & set(parts):
        lo, hi = (np.asarray(a).astype(np.int64) for a in fwd.search_batch(queries, **kw))
        empty = queries.index(b"")
        assert (int(lo[empty]), int(hi[empty])) == (0, n), "the empty query"
        lo[empty] = hi[empty] = 0                                    # (n ranks: not located)
        zlo, zhi = fwd.search_batch(list(zeros), **kw)
        assert _ints(zlo) == [0] * len(zeros) and _ints(zhi) == [F - len(z) + 1 for z in zeros], ("pure-zero queries", _ints(zlo), _ints(zhi))
        out["search"] = [a.tolist() for a in ranges(lo, hi)]
    if "locate" in parts:
        for max_hits in FM_LOCATE_HITS:
            o, pos = fwd.locate_ranges(lo.astype(np.uint64), hi.astype(np.uint64), max_hits, **kw)
            out[f"locate max_hits={max_hits}"] = [_ints(o), _ints(pos, shift)]
        elo, ehi = np.array([0, F - 40, n - 3], dtype=np.uint64), np.array([3, F + 40, n], dtype=np.uint64)
        o, pos = fwd.locate_ranges(elo, ehi, 0, **kw)
        assert _ints(o) == [0, 3, 83, 86] and _ints(pos[:3]) == [0, 1, 2], "the ranks [0, 3) are the positions [0, 3)"
        out["locate of explicit ranges"] = _ints(pos[3:], shift)
    if "approx" in parts:
        for d, both in FM_APPROX_COMBOS:
            keep = [i for i, q in enumerate(queries) if len(q) > d]
            sqb, soff = pack_queries([queries[i] for i in keep])
            qi, st, pos, mm = fwd.approx_arrays(sqb, soff, d, both, **kw)
            out[f"approx d={d} both={both}"] = [np.asarray(keep)[_ints(qi)].tolist() if len(qi) else [], _ints(st), _ints(pos, shift), _ints(mm)]
    if "ms" in parts:
        out["matching statistics"] = _ints(np.concatenate(fwd.matching_stats(queries, rev, **kw)))
    if "smems" in parts:
        for min_len in FM_SMEM_MIN_LENS:
            qi, qo, ln, slo, shi = (np.asarray(a).astype(np.int64) for a in fwd.smem_arrays(qb, off, rev, min_len, **kw))
            assert all(any(queries[i][o:o + l]) for i, o, l in zip(qi.tolist(), qo.tolist(), ln.tolist())), "an SMEM that is all zeros"
            assert (shi > slo).all()
            o, pos = fwd.locate_ranges(slo.astype(np.uint64), shi.astype(np.uint64), 0, **kw)
            out[f"smems min_len={min_len}"] = [_ints(qi), _ints(qo), _ints(ln), _ints(slo, shift), _ints(shi, shift), _ints(o), _ints(pos, shift)]
    if "extract" in parts:
        starts, ends = fm_extract_requests(F, n)
        o, data = fwd.extract_ranges(starts, ends, **kw)
        o, data = _ints(o), np.asarray(data)
        got = [data[o[i]:o[i + 1]] for i in range(starts.size)]
        for (a, b), g in zip(zip(starts.tolist(), ends.tolist()), got):
            a, b = min(a, n), min(b, n)
            want = np.concatenate([np.zeros(max(min(b, F) - a, 0), dtype=np.uint8), reg.text[max(a, F) - F:max(b, F) - F]])
            assert g.size == b - a and np.array_equal(g, want), f"extract [{a}, {b}) is not the text"
        out["extract"] = [g.tolist() for g in got[:8]]               # (the ninth is not in the twin: held to the text above)
    return out


def assert_fm_witness_is_not_empty(want: dict, symbols: int = 8) -> dict:
    """What keeps a comparison of the FM-index answers from being empty, decided by the twin's answers alone.  Rank F + r of the
    region's r-th byte and the byte's position are both 4096 + r on the twin, so the boundary rank and the boundary position
    are the twin's 4096 + MID.  Returns the counts it looked at."""
    twin = FULL_GEOMETRIES["twin"]
    B, F, q = twin.boundary, twin.filler, FM_SAMPLE
    queries = fm_batch(symbols)[0]
    lens = np.array([len(x) for x in queries], dtype=np.int64)
    seen = {}

    def sides(name, values):
        v = np.asarray(values, dtype=np.int64)
        seen[name + " below the boundary"], seen[name + " above the boundary"] = int(((v < B) & (v >= F)).sum()), int((v > B).sum())

    lo, hi = (np.asarray(a, dtype=np.int64) for a in want["search"])
    found = hi > lo
    sides("search ranges", lo[found])
    seen["queries not found"] = int((~found).sum())
    seen["queries whose leading zeros are matched in the filler"] = int(sum(1 for i, x in enumerate(queries) if x[:1] == b"\0" and found[i] and lo[i] < F))
    pos = np.asarray(want["locate max_hits=0"][1], dtype=np.int64)
    sides("located positions", pos)
    seen["located ranks q - 1 steps from their mark"] = int((pos % q == q - 1).sum())
    seen["located ranks that are marked"] = int((pos % q == 0).sum())
    for d, both in FM_APPROX_COMBOS:
        qi, st, p, mm = (np.asarray(a, dtype=np.int64) for a in want[f"approx d={d} both={both}"])
        tag = f"approx d={d} both={both} "
        sides(tag + "positions", p)
        seen[tag + "windows that hold the boundary byte"] = int(((p <= B) & (B < p + lens[qi])).sum())
        for k in range(d + 1):
            seen[tag + f"records with {k} mismatches"] = int((mm == k).sum())
        for s in (0, 1) if both else (0,):
            seen[tag + f"records on strand {s}"] = int((st == s).sum())
    for min_len in FM_SMEM_MIN_LENS:
        qi, qo, ln, slo, shi, o, p = (np.asarray(a, dtype=np.int64) for a in want[f"smems min_len={min_len}"])
        tag = f"smems min_len={min_len} "
        sides(tag + "ranges", slo)
        sides(tag + "positions", p)
        seen[tag + "occurrences that hold the boundary byte"] = int(((p <= B) & (B < p + np.repeat(ln, np.diff(o)))).sum())
    starts, ends = fm_extract_requests(F, twin.n)
    seen["extract requests over the boundary"] = int(((starts < B) & (ends > B + 1)).sum())
    seen["extract requests over the end of the text (the chunk of text_kept[0], the cyclic row)"] = int(((starts < twin.n) & (ends >= twin.n)).sum())
    seen["max ms"] = max(want["matching statistics"])
    assert all(seen.values()) and seen["max ms"] >= 900, seen
    return seen
