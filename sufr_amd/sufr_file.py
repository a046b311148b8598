"""Reading and searching a .sufr file: the host mirror of libsufr's query side.

`SufrFile` follows SufrFile<T> / SuffixArray of the reference (libsufr/src/sufr_file.rs, suffix_array.rs:181-440):
count / locate / extract / list / metadata / string_at with the reference's option and result names.  The work is done
by the C ABI of include/sufr_query.h (a mapped file, two binary searches per query).  `DeviceIndex` answers batches of
queries on the GPU from text + suffix array resident in HBM (sufr_hip_search_batch).  Both also give the matching
statistics and the super-maximal exact matches (SMEMs) of queries (include/sufr_match.h), and their
maximal exact matches (MEMs) on one or both strands (include/sufr_mem.h), and where they occur with
at most d mismatches (include/sufr_approx.h) or end with at most d edits (include/sufr_edit.h,
DESIGN.md section 16), with the start and the CIGAR of every such end (include/sufr_align.h)."""
from __future__ import annotations

import builtins
import ctypes as C
import datetime
import os
from dataclasses import dataclass, field
from functools import partial
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from ._lib import Context, FileMeta, SufrHipError, lib


@dataclass
class CountResult:                     # types.rs:365-374
    query_num: int
    query: str
    count: int


@dataclass
class LocatePosition:                  # types.rs:510-522
    suffix: int
    rank: int
    sequence_name: str
    sequence_position: int


@dataclass
class LocateResult:                    # types.rs:494-504
    query_num: int
    query: str
    positions: List[LocatePosition] = field(default_factory=list)


@dataclass
class ExtractSequence:                 # types.rs:423-444
    suffix: int
    rank: int
    sequence_name: str
    sequence_start: int
    sequence_range: Tuple[int, int]
    suffix_offset: int


@dataclass
class ExtractResult:                   # types.rs:400-409
    query_num: int
    query: str
    sequences: List[ExtractSequence] = field(default_factory=list)


@dataclass
class SmemHit:                         # one SMEM of a query (include/sufr_match.h)
    query_num: int
    query_offset: int                  # the SMEM is query[query_offset : query_offset + length]
    length: int
    rank_lo: int                       # the suffixes that start with it: ranks [rank_lo, rank_hi)
    rank_hi: int
    positions: np.ndarray              # SA[rank_lo : rank_lo + max_hits] (all with 0): absolute, rank order

    @property
    def count(self) -> int:
        return self.rank_hi - self.rank_lo


def _hit_end(lo: int, hi: int, max_hits: int) -> int:
    return lo + max_hits if max_hits and hi - lo > max_hits else hi


def _split(flat: np.ndarray, off: np.ndarray) -> list:
    o = off.astype(np.int64)
    return [flat[o[i] - o[0]:o[i + 1] - o[0]] for i in range(len(o) - 1)]


_SMEM_DTYPES = (np.uint64, np.uint32, np.uint32, np.uint64, np.uint64)     # query, query_offset, length, rank_lo, rank_hi


def _smem_hits(nq: int, recs, positions_of) -> List[List[SmemHit]]:
    """The SmemHit lists of `nq` queries from the five record columns; positions_of(t) are the positions of record t."""
    qi, qo, ln, lo, hi = recs
    out: List[List[SmemHit]] = [[] for _ in range(nq)]
    for t in range(len(qi)):
        out[int(qi[t])].append(SmemHit(int(qi[t]), int(qo[t]), int(ln[t]), int(lo[t]), int(hi[t]), positions_of(t).copy()))
    return out


@dataclass
class MemHit:                          # one MEM of a query (include/sufr_mem.h)
    query_offset: int                  # query[query_offset : query_offset + length] (strand 1: of the reverse complement) ...
    position: int                      # ... equals text[position : position + length], an indexed suffix
    length: int
    strand: int                        # 0: the query as given, 1: its reverse complement


_MEM_DTYPES = (np.uint64, np.uint32, np.uint8, np.uint32, np.uint64)        # query, query_offset, strand, length, position


def _mem_hits(nq: int, recs) -> List[List[MemHit]]:
    qi, qo, st, ln, pos = recs
    out: List[List[MemHit]] = [[] for _ in range(nq)]
    for t in range(len(qi)):
        out[int(qi[t])].append(MemHit(int(qo[t]), int(pos[t]), int(ln[t]), int(st[t])))
    return out


@dataclass
class ApproxHit:                       # one k-mismatch occurrence of a query (include/sufr_approx.h)
    query: int
    strand: int                        # 0: the query as given, 1: its reverse complement ...
    position: int                      # ... differs from text[position : position + len(query)] in `mismatches` bytes
    mismatches: int


_APPROX_DTYPES = (np.uint64, np.uint8, np.uint64, np.uint8)                 # query, strand, position, mismatches


def _approx_hits(nq: int, recs) -> List[List[ApproxHit]]:
    qi, st, pos, mm = recs
    out: List[List[ApproxHit]] = [[] for _ in range(nq)]
    for t in range(len(qi)):
        out[int(qi[t])].append(ApproxHit(int(qi[t]), int(st[t]), int(pos[t]), int(mm[t])))
    return out


@dataclass
class EditHit:                         # one k-difference occurrence of a query (include/sufr_edit.h)
    query: int
    strand: int                        # 0: the query as given, 1: its reverse complement ...
    end: int                           # ... is within `edits` substitutions, insertions and deletions of a piece of the text
    edits: int                         #     whose last byte is text[end]


def _edit_flags(both_strands: bool, local_minima: bool) -> int:
    from ._lib import EDIT_BOTH_STRANDS, EDIT_LOCAL_MINIMA
    return (EDIT_BOTH_STRANDS if both_strands else 0) | (EDIT_LOCAL_MINIMA if local_minima else 0)


def _edit_hits(nq: int, recs) -> List[List[EditHit]]:
    qi, st, end, ed = recs
    out: List[List[EditHit]] = [[] for _ in range(nq)]
    for t in range(len(qi)):
        out[int(qi[t])].append(EditHit(int(qi[t]), int(st[t]), int(end[t]), int(ed[t])))
    return out


@dataclass
class AlignHit:                        # a k-difference occurrence with its alignment (include/sufr_align.h)
    query: int
    strand: int
    end: int                           # the alignment covers text[start : end + 1] ...
    edits: int
    start: int
    cigar: str                         # ... with these ops ('=' 'X' 'I' 'D'), e.g. 37=1X12=2D98=


_CIGAR_OPS = {1: "I", 2: "D", 7: "=", 8: "X"}


def cigar_string(runs) -> str:
    """BAM-encoded runs (len << 4 | op) as text."""
    return "".join(f"{int(r) >> 4}{_CIGAR_OPS[int(r) & 15]}" for r in runs)


def _align_hits(nq: int, recs, trace) -> List[List[AlignHit]]:
    qi, st, end, ed = recs
    start, off, cigar = trace
    out: List[List[AlignHit]] = [[] for _ in range(nq)]
    for t in range(len(qi)):
        out[int(qi[t])].append(AlignHit(int(qi[t]), int(st[t]), int(end[t]), int(ed[t]), int(start[t]),
                                        cigar_string(cigar[int(off[t]):int(off[t + 1])])))
    return out


@dataclass
class SufrMetadata:                    # types.rs:587-626
    filename: str
    modified: datetime.datetime
    file_size: int
    file_version: int
    is_dna: bool
    allow_ambiguity: bool
    ignore_softmask: bool
    text_len: int
    len_suffixes: int
    num_sequences: int
    sequence_starts: List[int]
    sequence_names: List[str]
    max_query_len: int                 # sort_type: MaxQueryLen(n) ...
    seed_mask: Optional[str]           # ... or Mask(seed mask)


def _sized_to_fit(cap: Optional[int], guess: int, alloc, call, error):
    """The record arrays of an SMEM / MEM call, cut to the total it reports.  alloc(c) makes the outputs for c records and
    call(c, outputs, total) returns the library's code.  With a `cap` the call is made once; without one it starts at
    `guess` and, told -5 (capacity), once more with the total.  error(rc, total, c) makes the SufrHipError of a failure,
    which carries the total in `.total`."""
    c = cap if cap is not None else guess
    while True:
        out = alloc(max(c, 1))
        total = C.c_uint64(0)
        rc = call(c, out, total)
        if rc == -5 and cap is None:
            c = total.value
            continue
        if rc != 0:
            err = error(rc, total.value, c)
            err.total = total.value
            raise err
        return tuple(a[:total.value] for a in out)


def _file_error(fn: str, noun: str):
    def error(rc, total, c):
        msg = {-5: f"{total} {noun}, room for {c}", -6: "files built with a seed mask are not supported",
               -1: "invalid argument (min_len must be at least 1)"}.get(rc, "failed")
        return SufrHipError(rc, f"{fn}: " + msg)
    return error


_CAPPED = "files built with a seed mask or with a max_query_len (their LCP is capped) are not supported"
_LCP_ERRORS = {            # the analyses of the LCP array, by family: the text of every code the library gives a reason for
    "kmer": {-6: "files built with a seed mask are not supported, and a build with max_query_len has its LCP capped there",
             -1: "invalid argument (k and bins must be at least 1, the sequence starts must ascend from 0)"},
    "repeat": {-6: _CAPPED, -5: "more records than the arrays hold",
               -1: "invalid argument (min_len must be at least 1, the kind 0, 1 or 2, the sequence starts must ascend from 0)"},
    "shared": {-6: _CAPPED, -5: "more records than the arrays hold",
               -1: "invalid argument (min_len must be at least 1, the kind 0, 1 or 2, min_seqs at most max_seqs, the sequence starts "
                   "must ascend from 0)"},
    "lz": {-6: _CAPPED, -5: "more factors than the arrays hold", -1: "invalid argument (the sequence starts must ascend from 0)"},
}


def _lcp_check(family: str, fn: str, rc: int):
    """Raises the SufrHipError of the host call `fn` of a family of _LCP_ERRORS unless rc is 0."""
    if rc != 0:
        raise SufrHipError(rc, f"{fn}: " + _LCP_ERRORS[family].get(rc, "failed"))


def _bwt_check(fn: str, rc: int):
    """Raises the SufrHipError of the host call `fn` of include/sufr_bwt.h unless rc is 0 (it has no refusals)."""
    if rc != 0:
        raise SufrHipError(rc, f"{fn}: " + {-5: "more records than the arrays hold", -1: "invalid argument"}.get(rc, "failed"))


def _address(a):
    """Of a numpy array or a torch tensor, as the library takes it."""
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


def _counted(ncols: int, call, alloc, check, filled=lambda: None):
    """The `ncols` record columns of a call that counts, then fills, cut to the total.  call(cap, addresses, total) returns the
    library's code: made once with cap 0 and no columns (-5 there says only that there are records) and, unless the total is
    0, once more with the columns alloc(total) made.  check(rc) raises on a failure; filled() runs after a good fill."""
    total = C.c_uint64(0)
    rc = call(0, (None,) * ncols, total)
    if rc != -5:
        check(rc)
    out = alloc(max(total.value, 1))
    if total.value:
        check(call(total.value, [_address(a) for a in out], total))
        filled()
    return tuple(a[:total.value] for a in out)


def _host_columns(ncols: int):
    return lambda n: [np.zeros(n, dtype=np.uint64) for _ in range(ncols)]


def _as_bytes(q) -> bytes:
    return q.encode() if isinstance(q, str) else bytes(q)


def _packed_arrays(qbytes, offsets) -> Tuple[np.ndarray, np.ndarray]:
    """A packed batch as the host calls take it: contiguous uint8 bytes and uint64 offsets."""
    return np.ascontiguousarray(qbytes, dtype=np.uint8), np.ascontiguousarray(offsets, dtype=np.uint64)


class SufrFile:
    """An open version-6 .sufr file (SufrFile::read, sufr_file.rs:145-275).  The file is mapped, `low_memory` /
    `very_low_memory` of the reference only choose how much of it the reference copies to memory and are accepted
    and ignored here."""

    def __init__(self, filename: str, low_memory: bool = False):
        L = lib()
        h = C.c_void_p()
        err = C.create_string_buffer(512)
        rc = L.sufr_file_open(str(filename).encode(), C.byref(h), err, len(err))
        if rc != 0:
            raise SufrHipError(rc, err.value.decode())
        import threading
        self._view_lock = threading.RLock()       # re-entrant: a GC pass inside _view() can finalise a dead view of this file on the same thread
        self._live_views = 0
        self._close_pending = False
        self._h = h
        self.filename = str(filename)
        m = FileMeta()
        L.sufr_file_metadata(h, C.byref(m))
        self._meta = m
        self.text_len, self.len_suffixes, self.num_sequences = m.text_len, m.len_suffixes, m.num_sequences
        self.index_width = m.index_width
        self.is_dna, self.allow_ambiguity, self.ignore_softmask = bool(m.is_dna), bool(m.allow_ambiguity), bool(m.ignore_softmask)
        self.max_query_len = m.max_query_len
        self.sequence_starts = [L.sufr_file_sequence_start(h, i) for i in range(m.num_sequences)]
        self.sequence_names = [L.sufr_file_sequence_name(h, i).decode() for i in range(m.num_sequences)]
        self.seed_mask = None
        if m.seed_mask_len:
            raw = C.string_at(L.sufr_file_seed_mask(h), m.seed_mask_len)
            self.seed_mask = "".join("1" if b == 1 else "0" for b in raw)

    # -- views into the mapping --------------------------------------------------------------------------------------
    # Zero-copy: the arrays alias the mapped file, and every view PINS the mapping -- it holds a reference to this
    # object (so `SufrFile(p).suffix_array.tolist()` works).  close() (and leaving a `with` block) is therefore a
    # REQUEST while views are alive: the file stays mapped and open until the last view is gone (`pending_close` is
    # True meanwhile, `closed` only afterwards).  A caller that must release the file at a known point -- before
    # re-creating or truncating the same path, which would turn reads of a stale view into SIGBUS -- drops its views
    # first or takes copies (`copy=True` of array()).  The view count is guarded by a lock: finalisers run on
    # whichever thread drops the last reference.
    def _view(self, getter, count, dtype):
        import weakref
        with self._view_lock:
            if self._h is None:
                raise ValueError("SufrFile is closed")
            if count == 0:
                return np.empty(0, dtype=dtype)
            buf = (C.c_uint8 * (count * np.dtype(dtype).itemsize)).from_address(getter(self._h))
            self._live_views += 1
        buf._owner = self
        arr = np.frombuffer(buf, dtype=dtype)
        weakref.finalize(buf, SufrFile._view_gone, self)
        return arr

    @staticmethod
    def _view_gone(owner):
        with owner._view_lock:
            owner._live_views -= 1
            last = owner._live_views == 0 and owner._close_pending
        if last:
            owner.close()

    @property
    def closed(self) -> bool:
        """The mapping is gone (no view outstanding, close() done)."""
        return self._h is None

    @property
    def pending_close(self) -> bool:
        """close() was called while views were alive: the file is unmapped when the last of them goes."""
        return self._close_pending and self._h is not None

    def array(self, which: str, copy: bool = False) -> np.ndarray:
        """'text' | 'suffix_array' | 'lcp'; copy=True returns an array of its own (it does not pin the mapping)."""
        a = {"text": lambda: self.text, "suffix_array": lambda: self.suffix_array, "lcp": lambda: self.lcp}[which]()
        return a.copy() if copy else a

    @property
    def text(self) -> np.ndarray:
        return self._view(lib().sufr_file_text, self.text_len, np.uint8)

    @property
    def suffix_array(self) -> np.ndarray:
        return self._view(lib().sufr_file_suffix_array, self.len_suffixes, np.uint32 if self.index_width == 4 else np.uint64)

    @property
    def lcp(self) -> np.ndarray:
        return self._view(lib().sufr_file_lcp_array, self.len_suffixes, np.uint32 if self.index_width == 4 else np.uint64)

    def close(self):
        lock = getattr(self, "_view_lock", None)
        if lock is None:                                  # (__init__ failed before the mapping existed)
            return
        with lock:
            if self._live_views > 0:                      # arrays still alias the mapping: unmap when the last one goes
                self._close_pending = True
                return
            h, self._h = self._h, None
            self._close_pending = False
        if h:
            lib().sufr_file_close(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- the query API -------------------------------------------------------------------------------------------------
    def search(self, query, max_query_len: Optional[int] = None) -> Optional[Tuple[int, int]]:
        """Half-open rank range of the suffixes that match `query`, or None (SufrSearch::search, sufr_search.rs:104-168)."""
        q = _as_bytes(query)
        lo, hi = C.c_uint64(), C.c_uint64()
        hit = lib().sufr_file_search(self._h, q, len(q), int(max_query_len is not None), max_query_len or 0,
                                     C.byref(lo), C.byref(hi))
        return (lo.value, hi.value) if hit else None

    def search_batch(self, queries: Sequence, max_query_len: Optional[int] = None, threads: int = 0):
        """rank_lo, rank_hi (uint64 arrays, lo == hi == 0: not found) for a batch, `threads` host workers (0: one per core):
        the rayon loop of SufrFile::count / locate (sufr_file.rs:760-800)."""
        qb, off = pack_queries(queries)
        lo = np.zeros(len(off) - 1, dtype=np.uint64)
        hi = np.zeros(len(off) - 1, dtype=np.uint64)
        rc = lib().sufr_file_search_batch(self._h, qb.ctypes.data, off.ctypes.data, len(off) - 1, int(max_query_len is not None),
                                          max_query_len or 0, lo.ctypes.data, hi.ctypes.data, threads)
        if rc != 0:
            raise SufrHipError(rc, "sufr_file_search_batch failed")
        return lo, hi

    def count(self, queries: Sequence, max_query_len: Optional[int] = None, low_memory: bool = False) -> List[CountResult]:
        return _counts(queries, *self.search_batch(queries, max_query_len))

    def matching_statistics(self, queries: Sequence, threads: int = 0) -> List[np.ndarray]:
        """ms[j] per query (uint32 arrays): the longest prefix of query[j:] that starts an indexed suffix, capped at the
        build's max_query_len (include/sufr_match.h)."""
        qb, off = pack_queries(queries)
        ms = np.zeros(max(int(off[-1]), 1), dtype=np.uint32)
        rc = lib().sufr_file_matching_stats(self._h, qb.ctypes.data, off.ctypes.data, len(off) - 1, ms.ctypes.data, threads)
        if rc != 0:
            raise SufrHipError(rc, "sufr_file_matching_stats: " + ("files built with a seed mask are not supported" if rc == -6 else "failed"))
        return _split(ms, off)

    def smem_arrays(self, qbytes: np.ndarray, offsets: np.ndarray, min_len: int = 20, cap: Optional[int] = None, threads: int = 0):
        """(query, query_offset, length, rank_lo, rank_hi) of every SMEM of a packed batch, in (query, offset) order.  With a
        `cap` too small the SufrHipError (code -5) carries the total in `.total`; without one the arrays are sized to fit."""
        qbytes, offsets = _packed_arrays(qbytes, offsets)
        nq = len(offsets) - 1
        return _sized_to_fit(
            cap, int(offsets[-1] - offsets[0]) // 8 + 16, lambda c: [np.zeros(c, dtype=d) for d in _SMEM_DTYPES],
            lambda c, out, total: lib().sufr_file_smems(self._h, qbytes.ctypes.data, offsets.ctypes.data, nq, min_len, c,
                                                        *[a.ctypes.data for a in out], C.byref(total), threads),
            _file_error("sufr_file_smems", "SMEMs"))

    def smems(self, queries: Sequence, min_len: int = 20, max_hits: int = 0, threads: int = 0) -> List[List[SmemHit]]:
        """The SMEMs of every query (at least `min_len` long) with their rank ranges and up to `max_hits` positions each
        (0: all), on the host."""
        qb, off = pack_queries(queries)
        recs = self.smem_arrays(qb, off, min_len, threads=threads)
        sa, lo, hi = self.suffix_array, recs[3], recs[4]
        return _smem_hits(len(queries), recs, lambda t: sa[int(lo[t]):_hit_end(int(lo[t]), int(hi[t]), max_hits)])

    def write_reversed_fasta(self, path) -> None:
        """Writes the FASTA of the reversed text (include/sufr_fm_match.h): every sequence reversed and their order reversed,
        each under its name.  Created with this file's flags it gives the .sufr whose FM-index is the `rev` of a pair."""
        err = C.create_string_buffer(512)
        rc = lib().sufr_file_write_reversed_fasta(self._h, str(path).encode(), err, 512)
        if rc != 0:
            raise SufrHipError(rc, "sufr_file_write_reversed_fasta: " + (err.value.decode() or "failed"))

    def mem_arrays(self, qbytes: np.ndarray, offsets: np.ndarray, min_len: int = 20, max_occ: int = 0, both_strands: bool = False,
                   cap: Optional[int] = None, threads: int = 0):
        """(query, query_offset, strand, length, position) of every MEM of a packed batch, in (query, strand, offset, rank)
        order.  With a `cap` too small the SufrHipError (code -5) carries the total in `.total`; without one the arrays are
        sized to fit."""
        from ._lib import MEM_BOTH_STRANDS
        qbytes, offsets = _packed_arrays(qbytes, offsets)
        nq = len(offsets) - 1
        flags = MEM_BOTH_STRANDS if both_strands else 0
        return _sized_to_fit(
            cap, int(offsets[-1] - offsets[0]) // 4 + 16, lambda c: [np.zeros(c, dtype=d) for d in _MEM_DTYPES],
            lambda c, out, total: lib().sufr_file_mems(self._h, qbytes.ctypes.data, offsets.ctypes.data, nq, min_len, max_occ, flags, c,
                                                       *[a.ctypes.data for a in out], C.byref(total), threads),
            _file_error("sufr_file_mems", "MEMs"))

    def mems(self, queries: Sequence, min_len: int = 20, max_occ: int = 0, both_strands: bool = False,
             threads: int = 0) -> List[List[MemHit]]:
        """The MEMs of every query, at least `min_len` long, in (strand, offset, rank) order; offsets whose first min_len
        symbols start more than `max_occ` indexed suffixes give none (0: no limit).  On the host."""
        qb, off = pack_queries(queries)
        return _mem_hits(len(off) - 1, self.mem_arrays(qb, off, min_len, max_occ, both_strands, threads=threads))

    def approx_arrays(self, qbytes: np.ndarray, offsets: np.ndarray, max_mismatches: int = 2, max_occ: int = 0,
                      both_strands: bool = False, cap: Optional[int] = None, threads: int = 0):
        """(query, strand, position, mismatches) of every window of the text within `max_mismatches` substitutions of a query
        of a packed batch, in (query, strand, piece, rank) order.  With a `cap` too small the SufrHipError (code -5) carries
        the total in `.total`; without one the arrays are sized to fit."""
        from ._lib import APPROX_BOTH_STRANDS
        qbytes, offsets = _packed_arrays(qbytes, offsets)
        nq = len(offsets) - 1
        flags = APPROX_BOTH_STRANDS if both_strands else 0
        return _sized_to_fit(
            cap, 4 * nq + 16, lambda c: [np.zeros(c, dtype=d) for d in _APPROX_DTYPES],
            lambda c, out, total: lib().sufr_file_approx(self._h, qbytes.ctypes.data, offsets.ctypes.data, nq, max_mismatches, max_occ,
                                                         flags, c, *[a.ctypes.data for a in out], C.byref(total), threads),
            lambda rc, total, c: SufrHipError(rc, "sufr_file_approx: " + {
                -5: f"{total} records, room for {c}", -6: "files built with a seed mask are not supported",
                -1: "invalid argument (max_mismatches must be at most 15)"}.get(rc, "failed")))

    def approx(self, queries: Sequence, max_mismatches: int = 2, max_occ: int = 0, both_strands: bool = False,
               threads: int = 0) -> List[List[ApproxHit]]:
        """Where every query occurs with at most `max_mismatches` substitutions (seed and verify: the query is cut into
        max_mismatches + 1 pieces, pieces that start more than `max_occ` indexed suffixes seed nothing, 0: no limit), in
        (strand, piece, rank) order.  On the host."""
        qb, off = pack_queries(queries)
        return _approx_hits(len(off) - 1, self.approx_arrays(qb, off, max_mismatches, max_occ, both_strands, threads=threads))

    def edit_arrays(self, qbytes: np.ndarray, offsets: np.ndarray, max_edits: int = 2, max_occ: int = 0, both_strands: bool = False,
                    local_minima: bool = False, cap: Optional[int] = None, threads: int = 0):
        """(query, strand, end, edits) of every text position where a query of a packed batch ends with at most `max_edits`
        substitutions, insertions and deletions, sorted by (query, strand, end), each once.  With a `cap` too small the
        SufrHipError (code -5) carries the total in `.total`; without one the arrays are sized to fit."""
        qbytes, offsets = _packed_arrays(qbytes, offsets)
        nq = len(offsets) - 1
        flags = _edit_flags(both_strands, local_minima)
        return _sized_to_fit(
            cap, 4 * nq + 16, lambda c: [np.zeros(c, dtype=d) for d in _APPROX_DTYPES],
            lambda c, out, total: lib().sufr_file_edit(self._h, qbytes.ctypes.data, offsets.ctypes.data, nq, max_edits, max_occ,
                                                       flags, c, *[a.ctypes.data for a in out], C.byref(total), threads),
            lambda rc, total, c: SufrHipError(rc, "sufr_file_edit: " + {
                -5: f"{total} records, room for {c}", -6: "files built with a seed mask are not supported",
                -1: "invalid argument (max_edits must be at most 15)"}.get(rc, "failed")))

    def edit(self, queries: Sequence, max_edits: int = 2, max_occ: int = 0, both_strands: bool = False, local_minima: bool = False,
             threads: int = 0) -> List[List[EditHit]]:
        """Where every query ends in the text with at most `max_edits` edits (pigeonhole seeds as in `approx`, a banded
        Sellers table per candidate), by end; `local_minima` keeps one end per hill.  On the host."""
        qb, off = pack_queries(queries)
        return _edit_hits(len(off) - 1, self.edit_arrays(qb, off, max_edits, max_occ, both_strands, local_minima, threads=threads))

    def edit_trace_arrays(self, qbytes: np.ndarray, offsets: np.ndarray, query, strand, end, edits, cap: Optional[int] = None,
                          threads: int = 0):
        """(start, cigar_off, cigar) of the records (query, strand, end, edits) of `edit_arrays` on the same packed batch:
        record t starts at start[t] and owns the BAM-encoded runs cigar[cigar_off[t]:cigar_off[t + 1]] (include/sufr_align.h).
        With a `cap` (of runs) too small the SufrHipError (code -5) carries the total in `.total`; without one the runs are
        sized to fit.  A record that is none of this batch and text is code -1, with its index in the message."""
        qbytes, offsets = _packed_arrays(qbytes, offsets)
        recs = [np.ascontiguousarray(a, dtype=d) for a, d in zip((query, strand, end, edits), _APPROX_DTYPES)]
        nq, nr = len(offsets) - 1, len(recs[0])
        start = np.zeros(max(nr, 1), dtype=np.uint64)
        off = np.zeros(nr + 1, dtype=np.uint64)
        err = C.create_string_buffer(512)
        (cigar,) = _sized_to_fit(
            cap, 4 * nr + 16, lambda c: [np.zeros(c, dtype=np.uint32)],
            lambda c, out, total: lib().sufr_file_edit_trace(self._h, qbytes.ctypes.data, offsets.ctypes.data, nq, nr,
                                                             *[a.ctypes.data for a in recs], c, start.ctypes.data, off.ctypes.data,
                                                             out[0].ctypes.data, C.byref(total), threads, err, len(err)),
            lambda rc, total, c: SufrHipError(rc, "sufr_file_edit_trace: " + (err.value.decode() or "failed")))
        return start[:nr], off, cigar

    def align(self, queries: Sequence, max_edits: int = 2, max_occ: int = 0, both_strands: bool = False, local_minima: bool = False,
              threads: int = 0) -> List[List[AlignHit]]:
        """The hits of `edit` with the start and the CIGAR string of every one (`edit_arrays`, then `edit_trace_arrays`).  On
        the host."""
        qb, off = pack_queries(queries)
        recs = self.edit_arrays(qb, off, max_edits, max_occ, both_strands, local_minima, threads=threads)
        return _align_hits(len(off) - 1, recs, self.edit_trace_arrays(qb, off, *recs, threads=threads))

    # -- k-mer spectra, occurrence maps, unique lengths (include/sufr_kmer.h) -------------------------------------------
    def _index_dtype(self):
        return np.uint32 if self.index_width == 4 else np.uint64

    def kmers(self, k: int, bins: int = 256, occ: Optional[str] = None, threads: int = 0):
        """(hist, stats, occ) of the k-mers at the indexed positions: hist[i] distinct k-mers of count i + 1 (the last bin:
        `bins` and more), stats a dict of whole / distinct / unique / max_count, occ None or, with occ="rank" / "position",
        the count of the k-mer at every rank (parallel to the suffix array) or text position (0 where not indexed)."""
        from ._lib import KMER_BY_POSITION, KmerStats
        if occ not in (None, "rank", "position"):
            raise ValueError('occ is None, "rank" or "position"')
        hist = np.zeros(max(bins, 1), dtype=np.uint64)
        st = KmerStats()
        out = None if occ is None else np.zeros(max(self.text_len if occ == "position" else self.len_suffixes, 1), dtype=self._index_dtype())
        rc = lib().sufr_file_kmers(self._h, k, KMER_BY_POSITION if occ == "position" else 0, bins, hist.ctypes.data,
                                   out.ctypes.data if out is not None else None, C.byref(st), threads)
        _lcp_check("kmer", "sufr_file_kmers", rc)
        if out is not None:
            out = out[:self.text_len if occ == "position" else self.len_suffixes]
        return hist[:bins], st.as_dict(), out

    def unique_lengths(self, by_position: bool = False, threads: int = 0) -> np.ndarray:
        """The length at which the substring at every rank (or, by_position, text position) becomes unique: 1 + max(LCP[r],
        LCP[r + 1]), 0 where that runs over the end of its sequence (and, by position, where nothing is indexed)."""
        from ._lib import KMER_BY_POSITION
        count = self.text_len if by_position else self.len_suffixes
        out = np.zeros(max(count, 1), dtype=self._index_dtype())
        rc = lib().sufr_file_unique_lengths(self._h, KMER_BY_POSITION if by_position else 0, out.ctypes.data, threads)
        _lcp_check("kmer", "sufr_file_unique_lengths", rc)
        return out[:count]

    # -- repeats of the indexed text (include/sufr_repeat.h) ------------------------------------------------------------
    def repeats(self, kind="branching", min_len: int = 1, min_count: int = 2, max_count: int = 0, threads: int = 0):
        """(rank, count, length, stats): the repeats of the indexed text as three parallel uint64 arrays in ascending order of
        their representative rank -- the occurrences of record i are suffix_array[rank[i] : rank[i] + count[i]] -- and a
        dict of records / longest / longest_rank / max_count.  kind: "branching" (0, every LCP interval), "maximal" (1) or
        "super" (2).  One call counts, one fills."""
        from ._lib import REPEAT_KINDS, RepeatStats
        kind = REPEAT_KINDS.get(kind, kind)
        st = RepeatStats()
        cols = _counted(3, lambda cap, at, total: lib().sufr_file_repeats(self._h, kind, min_len, min_count, max_count, cap, *at,
                                                                          C.byref(total), C.byref(st), threads),
                        _host_columns(3), partial(_lcp_check, "repeat", "sufr_file_repeats"))
        return (*cols, st.as_dict())

    # -- longest previous factors and the LZ77 parse (include/sufr_lz.h) ------------------------------------------------
    def lpf(self, threads: int = 0):
        """(lpf, src): for every text position the length of the longest break-free string that also starts at an earlier
        indexed position, and such a position; arrays of the index width, src all ones where lpf is 0."""
        n = self.text_len
        out = [np.zeros(max(n, 1), dtype=self._index_dtype()) for _ in range(2)]
        rc = lib().sufr_file_lpf(self._h, out[0].ctypes.data, out[1].ctypes.data, threads)
        _lcp_check("lz", "sufr_file_lpf", rc)
        return out[0][:n], out[1][:n]

    def lz(self, threads: int = 0):
        """(start, length, source, stats): the LZ77 factors of the text in text order as three parallel uint64 arrays
        (source all ones: a literal of length 1) and a dict of factors / literals / longest / longest_start.  One call
        counts, one fills."""
        from ._lib import LzStats
        st = LzStats()
        cols = _counted(3, lambda cap, at, total: lib().sufr_file_lz(self._h, cap, *at, C.byref(total), C.byref(st), threads),
                        _host_columns(3), partial(_lcp_check, "lz", "sufr_file_lz"))
        return (*cols, st.as_dict())

    # -- sequence counts of repeats and k-common substrings (include/sufr_shared.h) --------------------------------------
    def shared(self, kind="branching", min_len: int = 1, min_count: int = 2, max_count: int = 0, min_seqs: int = 0, max_seqs: int = 0,
               threads: int = 0):
        """(rank, count, length, seqs, stats): the records of `repeats` with the number of different sequences among the
        occurrences of each, kept where min_seqs <= seqs <= max_seqs (0: open), and a dict of records / longest /
        longest_rank / max_count / max_seqs.  With min_seqs = num_sequences, `longest` is the longest substring common to all
        sequences; max_seqs = 1 keeps the repeats private to one sequence.  One call counts, one fills."""
        from ._lib import REPEAT_KINDS, SharedStats
        kind = REPEAT_KINDS.get(kind, kind)
        st = SharedStats()
        cols = _counted(4, lambda cap, at, total: lib().sufr_file_shared(self._h, kind, min_len, min_count, max_count, min_seqs, max_seqs,
                                                                         cap, *at, C.byref(total), C.byref(st), threads),
                        _host_columns(4), partial(_lcp_check, "shared", "sufr_file_shared"))
        return (*cols, st.as_dict())

    def common(self, threads: int = 0):
        """common[q - 1], q = 1 .. num_sequences: the length of the longest break-free string with indexed occurrences in at
        least q of the sequences (0: none); a uint64 array, non-increasing."""
        out = np.zeros(max(self.num_sequences, 1), dtype=np.uint64)
        rc = lib().sufr_file_common(self._h, out.ctypes.data, threads)
        _lcp_check("shared", "sufr_file_common", rc)
        return out

    # -- the BWT, its runs and the LF mapping (include/sufr_bwt.h) -------------------------------------------------------
    def bwt(self, threads: int = 0):
        """(bwt, counts): the byte in front of every indexed suffix in rank order (cyclic at the text's start) as a uint8
        array of len_suffixes entries, and how often each of the 256 byte values occurs in it (uint64).  Every file is a valid
        input."""
        s = self.len_suffixes
        out, counts = np.zeros(max(s, 1), dtype=np.uint8), np.zeros(256, dtype=np.uint64)
        _bwt_check("sufr_file_bwt", lib().sufr_file_bwt(self._h, out.ctypes.data, counts.ctypes.data, threads))
        return out[:s], counts

    def bwt_runs(self, min_len: int = 1, threads: int = 0):
        """(rank, length, symbol, first, stats): the maximal runs of equal BWT bytes of at least min_len ranks as four parallel
        uint64 arrays in ascending rank (first: suffix_array[rank]) and a dict of runs (r, whatever min_len) / records /
        longest / longest_rank.  One call counts, one fills."""
        from ._lib import BwtStats
        st = BwtStats()
        cols = _counted(4, lambda cap, at, total: lib().sufr_file_bwt_runs(self._h, min_len, cap, *at, C.byref(total), C.byref(st), threads),
                        _host_columns(4), partial(_bwt_check, "sufr_file_bwt_runs"))
        return (*cols, st.as_dict())

    def lf(self, threads: int = 0) -> np.ndarray:
        """LF[r] = C[bwt[r]] + the ranks before r with the same BWT byte: a permutation of the ranks, of the index width.
        Where every position is indexed and the order is exact, suffix_array[lf[r]] == (suffix_array[r] - 1) % text_len."""
        s = self.len_suffixes
        out = np.zeros(max(s, 1), dtype=self._index_dtype())
        _bwt_check("sufr_file_lf", lib().sufr_file_lf(self._h, out.ctypes.data, threads))
        return out[:s]

    # -- the FM-index over the BWT (include/sufr_fm.h) ---------------------------------------------------------------------
    def fm(self, sample: int = 32, threads: int = 0, text: bool = False) -> "FmIndex":
        """An FM-index of this file on the host: it answers search_batch and locate without the text and the suffix array and
        owns what it reads, so the file may be closed.  sample: every suffix at a multiple of it is kept for locate (0: none,
        no locate).  text: also keep the text samples, with which FmIndex.extract reads the text back (include/sufr_fm_text.h).
        Refused (-6) unless every position is indexed, there is no seed mask and no max_query_len, and the last byte of the
        text occurs once."""
        h = C.c_void_p()
        if text:
            from ._lib import FM_TEXT
            rc = lib().sufr_file_fm_build_flags(self._h, sample, FM_TEXT, C.byref(h), threads)
        else:
            rc = lib().sufr_file_fm_build(self._h, sample, C.byref(h), threads)
        if rc != 0:
            raise SufrHipError(rc, "sufr_file_fm_build: " + {-6: _FM_REFUSED, -1: "text=True needs a sample rate"}.get(rc, "failed"))
        return FmIndex(h, self.index_width)

    def _sequence_of(self, suffix: int) -> int:
        return lib().sufr_file_sequence_of(self._h, suffix)

    def locate(self, queries: Sequence, max_query_len: Optional[int] = None, low_memory: bool = False) -> List[LocateResult]:
        """SufrFile::locate (sufr_file.rs:1110-1175): positions in rank order."""
        sa = self.suffix_array
        out = []
        for i, q in enumerate(queries):
            res = LocateResult(i, q if isinstance(q, str) else bytes(q).decode("latin-1"))
            r = self.search(q, max_query_len)
            if r:
                for rank in range(r[0], r[1]):
                    sfx = int(sa[rank])
                    k = self._sequence_of(sfx)
                    res.positions.append(LocatePosition(sfx, rank, self.sequence_names[k], sfx - self.sequence_starts[k]))
            out.append(res)
        return out

    def extract(self, queries: Sequence, max_query_len: Optional[int] = None, low_memory: bool = False,
                prefix_len: Optional[int] = None, suffix_len: Optional[int] = None) -> List[ExtractResult]:
        """SufrFile::extract (sufr_file.rs:898-960)."""
        sa = self.suffix_array
        out = []
        for i, q in enumerate(queries):
            res = ExtractResult(i, q if isinstance(q, str) else bytes(q).decode("latin-1"))
            r = self.search(q, max_query_len)
            if r:
                for rank in range(r[0], r[1]):
                    sfx = int(sa[rank])
                    k = self._sequence_of(sfx)
                    start = self.sequence_starts[k]
                    end = self.sequence_starts[k + 1] if k + 1 < self.num_sequences else self.text_len
                    rel = sfx - start
                    cstart = max(rel - (prefix_len or 0), 0)
                    cend = min(rel + suffix_len, end) if suffix_len is not None else end
                    res.sequences.append(ExtractSequence(sfx, rank, self.sequence_names[k], start, (cstart, cend), rel - cstart))
            out.append(res)
        return out

    def string_at(self, pos: int, length: Optional[int] = None) -> str:
        """SufrFile::string_at (sufr_file.rs:399-411)."""
        end = min(pos + length, self.text_len) if length is not None else self.text_len
        return bytes(self.text[pos:end]).decode("latin-1")

    def list(self, ranks: Iterable[int] = (), show_rank=False, show_suffix=False, show_lcp=False, len: Optional[int] = None,
             number: Optional[int] = None) -> List[str]:
        """The lines `sufr list` prints (SufrFile::list, sufr_file.rs:1013-1077)."""
        width = builtins.len(str(self.text_len))
        sa, lcp = self.suffix_array, self.lcp
        n = self.text_len if len is None else len
        ranks = list(ranks)
        if not ranks:
            ranks = range(self.len_suffixes if not number else min(number, self.len_suffixes))
        lines = []
        for r in ranks:
            if r >= self.len_suffixes:
                continue
            sfx = int(sa[r])
            cols = []
            if show_rank:
                cols.append(f"{r:>{width}} ")
            if show_suffix:
                cols.append(f"{sfx:>{width}} ")
            if show_lcp:
                cols.append(f"{int(lcp[r]):>{width}} ")
            lines.append("".join(cols) + self.string_at(sfx, n))
        return lines

    def metadata(self) -> SufrMetadata:
        m = self._meta
        return SufrMetadata(self.filename, datetime.datetime.fromtimestamp(m.modified), m.file_size, m.version, self.is_dna,
                            self.allow_ambiguity, self.ignore_softmask, m.text_len, m.len_suffixes, m.num_sequences,
                            list(self.sequence_starts), list(self.sequence_names), m.max_query_len, self.seed_mask)



def pack_queries(queries: Sequence) -> Tuple[np.ndarray, np.ndarray]:
    """Concatenated query bytes + offsets, the batch layout of sufr_hip_search_batch."""
    bs = [_as_bytes(q) for q in queries]
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        off[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    return np.frombuffer(b"".join(bs), dtype=np.uint8).copy(), off


_FM_REFUSED = ("the FM-index takes an index of every text position (no --dna without --allow-ambiguity), built without a seed mask and "
               "without a max_query_len, over a text whose last byte occurs once")


def _fm_info(call, handle) -> dict:
    from ._lib import FmInfo
    info = FmInfo()
    rc = call(handle, C.byref(info))
    if rc != 0:
        raise SufrHipError(rc, "reading the info of the FM-index failed")
    return info.as_dict()


def _fm_text_info(call, handle) -> dict:
    from ._lib import FmTextInfo
    info = FmTextInfo()
    rc = call(handle, C.byref(info))
    if rc != 0:
        raise SufrHipError(rc, "reading the text info of the FM-index failed")
    return info.as_dict()


def _range_arrays(starts, ends) -> Tuple[np.ndarray, np.ndarray]:
    starts = np.ascontiguousarray(np.atleast_1d(starts), dtype=np.uint64)
    ends = np.ascontiguousarray(np.atleast_1d(ends), dtype=np.uint64)
    if starts.shape != ends.shape or starts.ndim != 1:
        raise ValueError("starts and ends must be one-dimensional and of one length")
    return starts, ends


def _clipped_total(starts: np.ndarray, ends: np.ndarray, n: int) -> int:
    e = np.minimum(ends, np.uint64(n))
    return int((e - np.minimum(starts, e)).sum())


_NO_TEXT = "the index was built without text samples (text=False)"


def _counts(queries: Sequence, lo, hi) -> List[CountResult]:
    return [CountResult(i, q if isinstance(q, str) else bytes(q).decode("latin-1"), int(hi[i] - lo[i])) for i, q in enumerate(queries)]


class FmIndex:
    """The FM-index of a .sufr file on the host (SufrFile.fm; include/sufr_fm.h): checkpointed BWT blocks, mark words and the
    kept suffixes.  It reads neither the file's text nor its suffix array."""

    def __init__(self, handle, index_width: int):
        self._h, self.index_width = handle, index_width

    @property
    def info(self) -> dict:
        """ranks, symbols (K), block (B), stride, sample, samples, bytes, width, end_byte (sufr_fm_info)"""
        return _fm_info(lib().sufr_fm_get_info, self._h)

    def close(self):
        if getattr(self, "_h", None):
            lib().sufr_fm_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def search_packed(self, qbytes: np.ndarray, offsets: np.ndarray, threads: int = 0):
        nq = len(offsets) - 1
        lo, hi = np.zeros(nq, dtype=np.uint64), np.zeros(nq, dtype=np.uint64)
        qbytes, offsets = _packed_arrays(qbytes, offsets)
        rc = lib().sufr_fm_search_batch(self._h, qbytes.ctypes.data, offsets.ctypes.data, nq, lo.ctypes.data, hi.ctypes.data, threads)
        if rc != 0:
            raise SufrHipError(rc, "sufr_fm_search_batch failed")
        return lo, hi

    def search_batch(self, queries: Sequence, threads: int = 0):
        """rank_lo, rank_hi (uint64 arrays, lo == hi == 0: not found): the ranges of SufrFile.search_batch."""
        return self.search_packed(*pack_queries(queries), threads)

    def count(self, queries: Sequence, threads: int = 0) -> List[CountResult]:
        return _counts(queries, *self.search_batch(queries, threads))

    def locate_ranges(self, lo: np.ndarray, hi: np.ndarray, max_hits: int = 0, threads: int = 0):
        """(offsets uint64[nq + 1], positions of the index width): query i owns positions[offsets[i]:offsets[i + 1]], the
        suffixes of ranks lo[i] .. min(hi[i], lo[i] + max_hits) in rank order (max_hits 0: all)."""
        lo, hi = np.ascontiguousarray(lo, dtype=np.uint64), np.ascontiguousarray(hi, dtype=np.uint64)
        cnt = hi - lo
        cap = int((np.minimum(cnt, np.uint64(max_hits)) if max_hits else cnt).sum())
        off = np.zeros(lo.size + 1, dtype=np.uint64)
        pos = np.zeros(max(cap, 1), dtype=np.uint64 if self.index_width == 8 else np.uint32)
        total = C.c_uint64(0)
        rc = lib().sufr_fm_locate_batch(self._h, lo.ctypes.data, hi.ctypes.data, lo.size, max_hits, off.ctypes.data, pos.ctypes.data, cap,
                                        C.byref(total), threads)
        if rc != 0:
            raise SufrHipError(rc, "sufr_fm_locate_batch: " + {-6: "the index was built without samples (sample == 0)",
                                                              -1: "invalid rank ranges"}.get(rc, "failed"))
        return off, pos[:total.value]

    def locate(self, queries: Sequence, max_hits: int = 0, threads: int = 0) -> List[np.ndarray]:
        """Text positions of every query's matches in rank order (unsigned arrays of the index's width)."""
        o, p = self.locate_ranges(*self.search_batch(queries, threads), max_hits, threads)
        return [p[int(o[i]):int(o[i + 1])] for i in range(len(queries))]

    # -- extract, the index file, the copies (include/sufr_fm_text.h) ---------------------------------------------------------
    @property
    def text_info(self) -> dict:
        """text_samples, text_bytes, file_bytes (sufr_fm_text_info)"""
        return _fm_text_info(lib().sufr_fm_get_text_info, self._h)

    def extract_ranges(self, starts, ends, threads: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """(offsets uint64[num + 1], bytes uint8): request i owns bytes[offsets[i]:offsets[i + 1]], the text from starts[i] to
        min(ends[i], text_len), read back from the BWT.  The index must have been built with text=True."""
        starts, ends = _range_arrays(starts, ends)
        cap = _clipped_total(starts, ends, self.info["ranks"])
        off = np.zeros(starts.size + 1, dtype=np.uint64)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        total = C.c_uint64(0)
        rc = lib().sufr_fm_extract_batch(self._h, starts.ctypes.data, ends.ctypes.data, starts.size, off.ctypes.data, out.ctypes.data, cap,
                                         C.byref(total), threads)
        if rc != 0:
            raise SufrHipError(rc, "sufr_fm_extract_batch: " + {-6: _NO_TEXT}.get(rc, "failed"))
        return off, out[:total.value]

    def extract(self, start: int, end: int) -> bytes:
        """The text from `start` to min(end, text_len)."""
        return self.extract_ranges([start], [end])[1].tobytes()

    def save(self, path, names_from: Optional["SufrFile"] = None) -> None:
        """Write the index to a file FmIndex.load reads without a .sufr (the layout: include/sufr_fm_text.h).  names_from: the
        open SufrFile whose sequence starts and names are stored; None stores those the index remembers (sequences())."""
        err = C.create_string_buffer(512)
        rc = lib().sufr_fm_save(self._h, os.fsencode(str(path)), names_from._h if names_from is not None else None, err, 512)
        if rc != 0:
            raise SufrHipError(rc, err.value.decode(errors="replace") or "sufr_fm_save failed")

    @classmethod
    def load(cls, path, threads: int = 0) -> "FmIndex":
        """The index FmIndex.save wrote, read into memory and verified: a damaged file is refused (-1, or -7 where it cannot be
        read) with the check that failed."""
        from ._lib import FmInfo
        h, err = C.c_void_p(), C.create_string_buffer(512)
        rc = lib().sufr_fm_load(os.fsencode(str(path)), C.byref(h), threads, err, 512)
        if rc != 0:
            raise SufrHipError(rc, err.value.decode(errors="replace") or "sufr_fm_load failed")
        info = FmInfo()
        lib().sufr_fm_get_info(h, C.byref(info))
        return cls(h, int(info.width))

    def sequences(self) -> Tuple[List[int], List[str]]:
        """(starts, names) of the sequences the index remembers: those of the file it was built from or loaded with."""
        L = lib()
        num = int(L.sufr_fm_num_sequences(self._h))
        return ([int(L.sufr_fm_sequence_start(self._h, i)) for i in range(num)],
                [L.sufr_fm_sequence_name(self._h, i).decode("latin-1") for i in range(num)])

    def set_sequences(self, starts: Sequence[int], names: Sequence[str]) -> None:
        """Replace the sequences the index remembers (none: save() then stores no names)."""
        st = np.ascontiguousarray(starts, dtype=np.uint64)
        arr = (C.c_char_p * max(len(names), 1))(*[n.encode("latin-1") for n in names])
        rc = lib().sufr_fm_set_sequences(self._h, st.ctypes.data, arr, len(names))
        if rc != 0 or st.size != len(names):
            raise SufrHipError(rc or -1, "sufr_fm_set_sequences: the starts must not decrease and must lie in the text, one name each")

    def to_device(self, ctx: Context) -> "DeviceFmIndex":
        """A copy of this index in the HBM of the context's device: allocations and copies only."""
        h = C.c_void_p()
        ctx.check(lib().sufr_hip_fm_upload(ctx.handle, self._h, C.byref(h)))
        return DeviceFmIndex(ctx, h, self.index_width)

    # -- k-mismatch search by backtracking (include/sufr_fm_approx.h) -------------------------------------------------------
    def approx_arrays(self, qbytes: np.ndarray, offsets: np.ndarray, max_mismatches: int = 2, both_strands: bool = False,
                      cap: Optional[int] = None, threads: int = 0):
        """(query, strand, position, mismatches) of every window of the text within `max_mismatches` (at most 3) substitutions
        of a query of a packed batch, as SufrFile.approx_arrays returns them, in (query, strand, leaf, rank) order.  With a `cap`
        too small the SufrHipError (code -5) carries the total in `.total`; without one the arrays are sized to fit."""
        from ._lib import FM_APPROX_BOTH_STRANDS
        qbytes, offsets = _packed_arrays(qbytes, offsets)
        nq = len(offsets) - 1
        flags = FM_APPROX_BOTH_STRANDS if both_strands else 0
        return _sized_to_fit(
            cap, 4 * nq + 16, lambda c: [np.zeros(c, dtype=d) for d in _APPROX_DTYPES],
            lambda c, out, total: lib().sufr_fm_approx(self._h, qbytes.ctypes.data, offsets.ctypes.data, nq, max_mismatches, flags, c,
                                                       *[a.ctypes.data for a in out], C.byref(total), threads),
            lambda rc, total, c: SufrHipError(rc, "sufr_fm_approx: " + {
                -5: f"{total} records, room for {c}", -6: "the index was built without samples (sample == 0)",
                -1: "invalid argument (max_mismatches must be at most 3)"}.get(rc, "failed")))

    def approx(self, queries: Sequence, max_mismatches: int = 2, both_strands: bool = False, threads: int = 0) -> List[List[ApproxHit]]:
        """Where every query occurs with at most `max_mismatches` substitutions, by backtracking on the index alone: all of
        them, each once, in (strand, leaf, rank) order."""
        qb, off = pack_queries(queries)
        return _approx_hits(len(off) - 1, self.approx_arrays(qb, off, max_mismatches, both_strands, threads=threads))

    def approx_steps(self, queries: Sequence, max_mismatches: int = 2, both_strands: bool = False, threads: int = 0):
        """(leaves, steps) of the walk of every (query, strand) item: what a batch costs (sufr_fm_approx_steps)."""
        qb, off = pack_queries(queries)
        items = (len(off) - 1) * (2 if both_strands else 1)
        leaves, steps = np.zeros(items, dtype=np.uint64), np.zeros(items, dtype=np.uint64)
        rc = lib().sufr_fm_approx_steps(self._h, qb.ctypes.data, off.ctypes.data, len(off) - 1, max_mismatches, 1 if both_strands else 0,
                                        leaves.ctypes.data, steps.ctypes.data, threads)
        if rc != 0:
            raise SufrHipError(rc, "sufr_fm_approx_steps failed")
        return leaves, steps

    # -- matching statistics and SMEMs on a pair of indexes (include/sufr_fm_match.h) ---------------------------------------
    @staticmethod
    def _pair_error(fn: str, noun: str = "records"):
        return lambda rc, total, c: SufrHipError(rc, f"{fn}: " + {
            -5: f"{total} {noun}, room for {c}",
            -1: "not an index of the reversed text, or an invalid argument (min_len must be at least 1)"}.get(rc, "failed"))

    def pair_check(self, rev: "FmIndex") -> None:
        """Raises unless `rev` agrees with this index in ranks, width, end byte, byte values and C: necessary for an index of
        the reversed text, not sufficient."""
        rc = lib().sufr_fm_pair_check(self._h, rev._h)
        if rc != 0:
            raise SufrHipError(rc, "sufr_fm_pair_check: not an index of the reversed text")

    def matching_stats(self, queries: Sequence, rev: "FmIndex", threads: int = 0) -> List[np.ndarray]:
        """ms[j] per query (uint32 arrays), as SufrFile.matching_statistics returns them, from this index and `rev`, the index
        of the reversed text, alone."""
        self.pair_check(rev)
        qb, off = pack_queries(queries)
        ms = np.zeros(max(int(off[-1]), 1), dtype=np.uint32)
        rc = lib().sufr_fm_matching_stats(self._h, rev._h, qb.ctypes.data, off.ctypes.data, len(off) - 1, ms.ctypes.data, threads)
        if rc != 0:
            raise SufrHipError(rc, "sufr_fm_matching_stats failed")
        return _split(ms, off)

    def smem_arrays(self, qbytes: np.ndarray, offsets: np.ndarray, rev: "FmIndex", min_len: int = 20, cap: Optional[int] = None,
                    threads: int = 0):
        """(query, query_offset, length, rank_lo, rank_hi) of every SMEM of a packed batch, as SufrFile.smem_arrays returns
        them.  With a `cap` too small the SufrHipError (code -5) carries the total in `.total`."""
        qbytes, offsets = _packed_arrays(qbytes, offsets)
        nq = len(offsets) - 1
        return _sized_to_fit(
            cap, int(offsets[-1] - offsets[0]) // 8 + 16, lambda c: [np.zeros(c, dtype=d) for d in _SMEM_DTYPES],
            lambda c, out, total: lib().sufr_fm_smems(self._h, rev._h, qbytes.ctypes.data, offsets.ctypes.data, nq, min_len, c,
                                                      *[a.ctypes.data for a in out], C.byref(total), threads),
            self._pair_error("sufr_fm_smems", "SMEMs"))

    def smems(self, queries: Sequence, rev: "FmIndex", min_len: int = 20, max_hits: int = 0, threads: int = 0) -> List[List[SmemHit]]:
        """The SMEMs of every query as SufrFile.smems returns them, the positions by locate_ranges."""
        qb, off = pack_queries(queries)
        recs = self.smem_arrays(qb, off, rev, min_len, threads=threads)
        po, pos = self.locate_ranges(recs[3], recs[4], max_hits, threads) if len(recs[0]) else (np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
        return _smem_hits(len(queries), recs, lambda t: pos[int(po[t]):int(po[t + 1])])

    def matching_stats_steps(self, queries: Sequence, rev: "FmIndex", threads: int = 0) -> np.ndarray:
        """The steps of the whole-query walk of every query (uint64): what the statistics of a batch cost."""
        qb, off = pack_queries(queries)
        steps = np.zeros(max(len(off) - 1, 1), dtype=np.uint64)
        rc = lib().sufr_fm_matching_stats_steps(self._h, rev._h, qb.ctypes.data, off.ctypes.data, len(off) - 1, steps.ctypes.data, threads)
        if rc != 0:
            raise SufrHipError(rc, "sufr_fm_matching_stats_steps: " + ("not an index of the reversed text" if rc == -1 else "failed"))
        return steps[:len(off) - 1]


class _DeviceBatch:
    """The batch path DeviceIndex and DeviceFmIndex share: an object with `ctx`, `_h` and `index_width` whose methods hand
    over the library call and the handles it takes after the context (the index; for a pair call of the FM-index the index
    and that of the reversed text).  Everything else about a call is the same on both."""

    def _packed(self, queries: Sequence):
        """The queries as a packed batch on the context's device: (uint8 bytes, int64 offsets)."""
        import torch
        qb, off = pack_queries(queries)
        dev = torch.device("cuda", self.ctx.device)
        return torch.from_numpy(qb).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev)

    @staticmethod
    def _device_bytes(qbytes):
        """The query bytes as the library takes them: a batch of empty queries still needs a device address."""
        import torch
        return qbytes if qbytes.numel() else torch.zeros(1, dtype=torch.uint8, device=qbytes.device)

    def _device_records(self, cap, guess, device, dtypes, call):
        """_sized_to_fit for torch outputs on `device`; the error text is the context's, the records are complete on return."""
        import torch
        out = _sized_to_fit(cap, guess, lambda c: [torch.empty(c, dtype=d, device=device) for d in dtypes], call,
                            lambda rc, total, c: SufrHipError(rc, lib().sufr_hip_last_error(self.ctx.handle).decode()))
        self.ctx.synchronize()
        return out

    def _search_device(self, call, qbytes, offsets, wait, *limit):
        """search_device: `limit` is what the call takes between the batch and the outputs."""
        import torch
        torch.cuda.current_stream(qbytes.device).synchronize()
        nq = offsets.numel() - 1
        lo = torch.empty(nq, dtype=torch.int64, device=qbytes.device)
        hi = torch.empty(nq, dtype=torch.int64, device=qbytes.device)
        self.ctx.check(call(self.ctx.handle, self._h, qbytes.data_ptr(), offsets.data_ptr(), nq, *limit, lo.data_ptr(), hi.data_ptr()))
        if wait:
            self.ctx.synchronize()
        return lo, hi

    def _locate_device(self, call, lo, hi, max_hits, capacity):
        import torch
        nq = lo.numel()
        off = torch.empty(nq + 1, dtype=torch.int64, device=lo.device)
        total = C.c_uint64(0)
        torch.cuda.current_stream(lo.device).synchronize()
        if capacity is None:                                   # size the output from the counts
            cnt = hi - lo
            capacity = int((cnt.clamp(max=max_hits) if max_hits else cnt).sum())
        pos = torch.empty(max(capacity, 1), dtype=torch.int64 if self.index_width == 8 else torch.int32, device=lo.device)
        self.ctx.check(call(self.ctx.handle, self._h, lo.data_ptr(), hi.data_ptr(), nq, max_hits, off.data_ptr(), pos.data_ptr(), capacity,
                            C.byref(total)))
        self.ctx.synchronize()
        return off, pos[:total.value]

    def _located(self, lo, hi, max_hits: int):
        """locate_device on the host: (offsets, positions as unsigned values of the index's width)."""
        o, p = self.locate_device(lo, hi, max_hits)
        return o.cpu().numpy(), p.cpu().numpy().view(np.uint64 if self.index_width == 8 else np.uint32)

    def _locate(self, n: int, lo, hi, max_hits: int) -> List[np.ndarray]:
        o, p = self._located(lo, hi, max_hits)
        return [p[o[i]:o[i + 1]] for i in range(n)]

    def _matching_stats_device(self, call, handles, qbytes, offsets, wait):
        import torch
        torch.cuda.current_stream(qbytes.device).synchronize()
        nq = offsets.numel() - 1
        qbytes = self._device_bytes(qbytes)
        ms = torch.zeros(max(int(offsets[-1]) if nq >= 0 and offsets.numel() else 0, 1), dtype=torch.int32, device=qbytes.device)
        self.ctx.check(call(self.ctx.handle, *handles, qbytes.data_ptr(), offsets.data_ptr(), max(nq, 0), ms.data_ptr()))
        if wait:
            self.ctx.synchronize()
        return ms

    def _smems_device(self, call, handles, qbytes, offsets, min_len, cap):
        import torch
        torch.cuda.current_stream(qbytes.device).synchronize()
        nq = offsets.numel() - 1
        dev = qbytes.device
        qbytes = self._device_bytes(qbytes)
        nbytes = int(offsets[-1] - offsets[0]) if nq > 0 else 0
        ms = torch.empty(max(int(offsets[-1]) if nq > 0 else 0, 1), dtype=torch.int32, device=dev)
        out = self._device_records(
            cap, nbytes // 8 + 16, dev, (torch.int64, torch.int32, torch.int32, torch.int64, torch.int64),
            lambda c, out, total: call(self.ctx.handle, *handles, qbytes.data_ptr(), offsets.data_ptr(), max(nq, 0), min_len, ms.data_ptr(), c,
                                       *[t.data_ptr() for t in out], C.byref(total)))
        self.last_ms = ms
        return out

    def _smems(self, nq: int, recs, max_hits: int) -> List[List[SmemHit]]:
        """The SmemHit lists of device records, the positions through locate_device."""
        po, pos = self._located(recs[3], recs[4], max_hits)
        return _smem_hits(nq, [t.cpu().numpy() for t in recs], lambda t: pos[po[t]:po[t + 1]])


class DeviceFmIndex(_DeviceBatch):
    """The FM-index of a DeviceIndex in HBM (DeviceIndex.fm_device; include/sufr_fm.h).  It owns everything it reads: the
    DeviceIndex may be closed and wrapped tensors overwritten.  The calls mirror DeviceIndex.search_device / locate_device."""

    def __init__(self, ctx: Context, handle, index_width: int):
        self.ctx, self._h, self.index_width = ctx, handle, index_width

    @property
    def info(self) -> dict:
        return _fm_info(lib().sufr_hip_fm_get_info, self._h)

    def close(self):
        if getattr(self, "_h", None):
            lib().sufr_hip_fm_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def search_device(self, qbytes, offsets, wait: bool = True):
        """torch CUDA tensors in (uint8 bytes, int64 offsets), int64 CUDA tensors (lo, hi) out; see DeviceIndex.search_device
        for `wait` and the streams."""
        return self._search_device(lib().sufr_hip_fm_search_batch_device, self._device_bytes(qbytes), offsets, wait)

    def locate_device(self, lo, hi, max_hits: int = 0, capacity: Optional[int] = None):
        """(offsets int64[nq + 1], positions) on the device for rank ranges on the device, as DeviceIndex.locate_device returns
        them: int32 holding u32 values, or int64 for a 64-bit index.  Complete on return."""
        return self._locate_device(lib().sufr_hip_fm_locate_batch_device, lo, hi, max_hits, capacity)

    def search(self, queries: Sequence) -> Tuple[np.ndarray, np.ndarray]:
        """rank_lo, rank_hi (uint64 arrays; lo == hi == 0 where the query does not occur)."""
        lo, hi = self.search_device(*self._packed(queries))
        return lo.cpu().numpy().view(np.uint64), hi.cpu().numpy().view(np.uint64)

    def count(self, queries: Sequence) -> List[CountResult]:
        return _counts(queries, *self.search(queries))

    # -- extract and the copies (include/sufr_fm_text.h) ------------------------------------------------------------------------
    @property
    def text_info(self) -> dict:
        """text_samples, text_bytes, file_bytes (sufr_fm_text_info; the file without names)"""
        return _fm_text_info(lib().sufr_hip_fm_get_text_info, self._h)

    def extract_device(self, starts, ends, cap: Optional[int] = None):
        """(offsets int64[num + 1], bytes uint8) on the device for int64 CUDA tensors of starts and ends: request i owns
        bytes[offsets[i]:offsets[i + 1]], the text from starts[i] to min(ends[i], text_len).  Complete on return.  With a `cap`
        too small the SufrHipError (code -5) carries the total in `.total`; without one the bytes are sized to fit."""
        import torch
        torch.cuda.current_stream(starts.device).synchronize()
        num = starts.numel()
        if cap is None:
            n = self.info["ranks"]
            e = ends.clamp(min=0, max=n) if num else ends
            cap = int((e - torch.minimum(starts.clamp(min=0), e)).sum()) if num else 0
        off = torch.empty(num + 1, dtype=torch.int64, device=starts.device)
        out = torch.empty(max(cap, 1), dtype=torch.uint8, device=starts.device)
        total = C.c_uint64(0)
        rc = lib().sufr_hip_fm_extract_batch_device(self.ctx.handle, self._h, starts.data_ptr(), ends.data_ptr(), num, off.data_ptr(), out.data_ptr(),
                                                    cap, C.byref(total))
        if rc != 0:
            err = SufrHipError(rc, lib().sufr_hip_last_error(self.ctx.handle).decode())
            err.total = int(total.value)
            raise err
        self.ctx.synchronize()
        return off, out[:total.value]

    def extract_ranges(self, starts, ends) -> Tuple[np.ndarray, np.ndarray]:
        """FmIndex.extract_ranges, read on the device: (offsets uint64[num + 1], bytes uint8) as numpy arrays."""
        import torch
        starts, ends = _range_arrays(starts, ends)
        dev = torch.device("cuda", self.ctx.device)
        # (positions beyond 2^63 mean "behind the text" and are held to int64's range)
        top = np.uint64(2**63 - 1)
        off, out = self.extract_device(torch.from_numpy(np.minimum(starts, top).astype(np.int64)).to(dev),
                                       torch.from_numpy(np.minimum(ends, top).astype(np.int64)).to(dev))
        return off.cpu().numpy().view(np.uint64), out.cpu().numpy()

    def extract(self, start: int, end: int) -> bytes:
        """The text from `start` to min(end, text_len)."""
        return self.extract_ranges([start], [end])[1].tobytes()

    def to_host(self) -> FmIndex:
        """A copy of this index in host memory (it remembers no sequences)."""
        h = C.c_void_p()
        self.ctx.check(lib().sufr_hip_fm_download(self.ctx.handle, self._h, C.byref(h)))
        return FmIndex(h, self.index_width)

    # -- k-mismatch search by backtracking (include/sufr_fm_approx.h) -------------------------------------------------------
    def approx_device(self, qbytes, offsets, max_mismatches: int = 2, both_strands: bool = False, cap: Optional[int] = None):
        """FmIndex.approx_arrays for a packed batch of torch CUDA tensors (uint8 bytes, int64 offsets): (query int64, strand
        uint8, position int64, mismatches uint8) tensors as DeviceIndex.approx_device returns them, in (query, strand, leaf,
        rank) order, complete on return.  With a `cap` too small the SufrHipError (code -5) carries the total in `.total`."""
        import torch
        from ._lib import FM_APPROX_BOTH_STRANDS
        torch.cuda.current_stream(qbytes.device).synchronize()
        nq = max(offsets.numel() - 1, 0)
        dev = qbytes.device
        qbytes = self._device_bytes(qbytes)
        flags = FM_APPROX_BOTH_STRANDS if both_strands else 0
        return self._device_records(
            cap, 4 * nq + 16, dev, (torch.int64, torch.uint8, torch.int64, torch.uint8),
            lambda c, out, total: lib().sufr_hip_fm_approx_device(self.ctx.handle, self._h, qbytes.data_ptr(), offsets.data_ptr(), nq,
                                                                  max_mismatches, flags, c, *[t.data_ptr() for t in out], C.byref(total)))

    def approx(self, queries: Sequence, max_mismatches: int = 2, both_strands: bool = False) -> List[List[ApproxHit]]:
        """The k-mismatch occurrences of every query (FmIndex.approx), found on the device."""
        qb, off = self._packed(queries)
        recs = self.approx_device(qb, off, max_mismatches, both_strands)
        return _approx_hits(off.numel() - 1, [t.cpu().numpy() for t in recs])

    def locate(self, queries: Sequence, max_hits: int = 0) -> List[np.ndarray]:
        """Text positions of every query's matches in rank order (unsigned arrays of the index's width)."""
        return self._locate(len(queries), *self.search_device(*self._packed(queries)), max_hits)

    # -- matching statistics and SMEMs on a pair of indexes (include/sufr_fm_match.h) ---------------------------------------
    def matching_stats_device(self, qbytes, offsets, rev: "DeviceFmIndex", wait: bool = True):
        """DeviceIndex.matching_statistics_device from this index and `rev`, the index of the reversed text, alone: an int32
        tensor (u32 values) indexed like the bytes.  wait=False: call ctx.synchronize() before reading it."""
        return self._matching_stats_device(lib().sufr_hip_fm_matching_stats_device, (self._h, rev._h), qbytes, offsets, wait)

    def matching_stats(self, queries: Sequence, rev: "DeviceFmIndex") -> List[np.ndarray]:
        """ms[j] per query (uint32 arrays), computed on the device."""
        qb, off = self._packed(queries)
        ms = self.matching_stats_device(qb, off, rev)
        return _split(ms.cpu().numpy().view(np.uint32), off.cpu().numpy().astype(np.uint64))

    def smems_device(self, qbytes, offsets, rev: "DeviceFmIndex", min_len: int = 20, cap: Optional[int] = None):
        """DeviceIndex.smems_device from the pair alone: (query int64, query_offset int32, length int32, rank_lo int64, rank_hi
        int64) tensors in (query, offset) order, complete on return; `last_ms` keeps the statistics.  With a `cap` too small
        the SufrHipError (code -5) carries the total in `.total`; without one the outputs are sized to fit."""
        return self._smems_device(lib().sufr_hip_fm_smems_device, (self._h, rev._h), qbytes, offsets, min_len, cap)

    def smems(self, queries: Sequence, rev: "DeviceFmIndex", min_len: int = 20, max_hits: int = 0) -> List[List[SmemHit]]:
        """The SMEMs of every query with their rank ranges and up to `max_hits` positions (0: all), as DeviceIndex.smems
        returns them (sufr_hip_fm_smems_device + sufr_hip_fm_locate_batch_device)."""
        return self._smems(len(queries), self.smems_device(*self._packed(queries), rev, min_len), max_hits)


class DeviceIndex(_DeviceBatch):
    """Text + suffix array resident in HBM, searched a batch at a time (include/sufr_query.h, device section).

    DeviceIndex.load(ctx, sufr_file)                              copies an open file to the GPU
    DeviceIndex.wrap(ctx, text_tensor, sa_tensor, ...)            wraps torch CUDA tensors (e.g. DeviceBuilder output)"""

    def __init__(self, ctx: Context, handle, keep=()):
        self.ctx, self._h, self._keep = ctx, handle, keep
        self.index_width = lib().sufr_hip_index_width(handle)      # 4 or 8: the width of the positions of this handle

    @classmethod
    def load(cls, ctx: Context, f: SufrFile) -> "DeviceIndex":
        h = C.c_void_p()
        ctx.check(lib().sufr_hip_index_load(ctx.handle, f._h, C.byref(h)))
        ix = cls(ctx, h)
        ix.text_len, ix.len_suffixes = f.text_len, f.len_suffixes
        assert ix.index_width == f.index_width              # (the file format's rule)
        return ix

    @classmethod
    def wrap(cls, ctx: Context, text, sa, max_query_len: int = 0, seed_mask: Optional[str] = None, is_dna: bool = False,
             prefix_table: bool = True) -> "DeviceIndex":
        import torch
        if not (text.is_cuda and sa.is_cuda and text.dtype == torch.uint8 and
                sa.dtype in (torch.int32, torch.uint32, torch.int64, torch.uint64)):
            raise ValueError("wrap() takes a uint8 text and a 32- or 64-bit suffix array on the GPU")
        wide = sa.dtype in (torch.int64, torch.uint64)
        if (text.numel() >= 0xFFFFFFFF) and not wide:
            raise ValueError("texts of 2^32 - 1 bytes and more have 64-bit suffix arrays (suffix_array.rs:460-470)")
        h = C.c_void_p()
        from ._lib import FLAG_DNA, FLAG_NO_PREFIX_TABLE, FLAG_SA_U64
        torch.cuda.current_stream(text.device).synchronize()      # the table is built from the arrays right away
        flags = (FLAG_DNA if is_dna else 0) | (0 if prefix_table else FLAG_NO_PREFIX_TABLE) | (FLAG_SA_U64 if wide else 0)
        ctx.check(lib().sufr_hip_index_wrap(ctx.handle, text.data_ptr(), text.numel(), sa.data_ptr(), sa.numel(), flags,
                                            max_query_len, seed_mask.encode() if seed_mask else None, C.byref(h)))
        ix = cls(ctx, h, keep=(text, sa))
        ix.text_len, ix.len_suffixes = text.numel(), sa.numel()
        # 8 iff the array was taken as 64-bit
        assert ix.index_width == (8 if wide else 4)
        return ix

    def close(self):
        if getattr(self, "_h", None):
            lib().sufr_hip_index_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def search(self, queries: Sequence, max_query_len: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """rank_lo, rank_hi (uint64 arrays; lo == hi == 0 where the query does not occur)."""
        qb, off = pack_queries(queries)
        return self.search_packed(qb, off, max_query_len)

    def search_packed(self, qbytes: np.ndarray, offsets: np.ndarray, max_query_len: Optional[int] = None):
        nq = len(offsets) - 1
        lo = np.zeros(nq, dtype=np.uint64)
        hi = np.zeros(nq, dtype=np.uint64)
        qbytes, offsets = _packed_arrays(qbytes, offsets)
        self.ctx.check(lib().sufr_hip_search_batch(self.ctx.handle, self._h, qbytes.ctypes.data, offsets.ctypes.data, nq,
                                                  int(max_query_len is not None), max_query_len or 0,
                                                  lo.ctypes.data, hi.ctypes.data))
        return lo, hi

    def search_device(self, qbytes, offsets, max_query_len: Optional[int] = None, wait: bool = True):
        """torch CUDA tensors in (uint8 bytes, int64 offsets), torch CUDA tensors out.  The launch goes to the context's
        stream, which is not ordered against torch's: the producer of the inputs is synchronised first, and with `wait`
        the answers are complete on return (wait=False: call ctx.synchronize() before reading them)."""
        return self._search_device(lib().sufr_hip_search_batch_device, qbytes, offsets, wait, int(max_query_len is not None), max_query_len or 0)

    def locate_device(self, lo, hi, max_hits: int = 0, capacity: Optional[int] = None):
        """Positions behind rank ranges that are on the device (torch int64 tensors from search_device): returns
        (offsets int64[nq + 1], positions); query i owns positions[offsets[i]:offsets[i + 1]], in rank order, at most max_hits
        of them (0: all).  The positions have the index's width: int32 holding u32 values, or int64 for a 64-bit index."""
        return self._locate_device(lib().sufr_hip_locate_batch_device, lo, hi, max_hits, capacity)

    def locate(self, queries: Sequence, max_query_len: Optional[int] = None, max_hits: int = 0) -> List[np.ndarray]:
        """Text positions of every query's matches in rank order (unsigned arrays of the index's width), searched and gathered
        on the device."""
        return self._locate(len(queries), *self.search_device(*self._packed(queries), max_query_len), max_hits)

    def count(self, queries: Sequence, max_query_len: Optional[int] = None) -> List[CountResult]:
        return _counts(queries, *self.search(queries, max_query_len))

    # -- matching statistics and SMEMs (include/sufr_match.h) ---------------------------------------------------------
    def matching_statistics_device(self, qbytes, offsets, wait: bool = True):
        """ms of a packed batch of torch CUDA tensors (uint8 bytes, int64 offsets): an int32 tensor (u32 values) indexed like
        the bytes.  wait=False: call ctx.synchronize() before reading it."""
        return self._matching_stats_device(lib().sufr_hip_matching_stats_device, (self._h,), qbytes, offsets, wait)

    def matching_statistics(self, queries: Sequence) -> List[np.ndarray]:
        """ms[j] per query (uint32 arrays), computed on the device."""
        qb, off = self._packed(queries)
        ms = self.matching_statistics_device(qb, off)
        return _split(ms.cpu().numpy().view(np.uint32), off.cpu().numpy().astype(np.uint64))

    def smems_device(self, qbytes, offsets, min_len: int = 20, cap: Optional[int] = None):
        """SMEMs of a packed batch of torch CUDA tensors: (query int64, query_offset int32, length int32, rank_lo int64,
        rank_hi int64) tensors in (query, offset) order, complete on return.  With a `cap` too small the SufrHipError
        (code -5) carries the total in `.total`; without one the outputs are sized to fit."""
        return self._smems_device(lib().sufr_hip_smems_device, (self._h,), qbytes, offsets, min_len, cap)

    def smems(self, queries: Sequence, min_len: int = 20, max_hits: int = 0) -> List[List[SmemHit]]:
        """The SMEMs of every query with their rank ranges and up to `max_hits` positions (0: all), searched and gathered
        on the device (sufr_hip_smems_device + sufr_hip_locate_batch_device)."""
        return self._smems(len(queries), self.smems_device(*self._packed(queries), min_len), max_hits)

    # -- k-mer spectra, occurrence maps, unique lengths (include/sufr_kmer.h) ------------------------------------------
    def _lcp_inputs(self, lcp, seq_starts):
        """What every *_device analysis takes: the LCP tensor checked (on the GPU, of the index's width, its producer
        finished) and the sequence starts as the library reads them.  Returns (dtype of the width, starts, their address, their
        count)."""
        import torch
        wide = self.index_width == 8
        if not lcp.is_cuda or lcp.dtype not in ((torch.int64, torch.uint64) if wide else (torch.int32, torch.uint32)):
            raise ValueError("the LCP array is a CUDA tensor of the index's width")
        torch.cuda.current_stream(lcp.device).synchronize()
        st = None if seq_starts is None else np.ascontiguousarray(seq_starts, dtype=np.uint64)
        return torch.int64 if wide else torch.int32, st, (st.ctypes.data if st is not None and st.size else None), (st.size if st is not None else 0)

    def _counted_device(self, lcp, ncols, call):
        """_counted for int64 columns on the LCP tensor's device; the error text is the context's, the records are complete on
        return."""
        import torch
        return _counted(ncols, call, lambda n: [torch.empty(n, dtype=torch.int64, device=lcp.device) for _ in range(ncols)],
                        self.ctx.check, self.ctx.synchronize)

    def kmers_device(self, lcp, k: int, bins: int = 256, occ: Optional[str] = None, seq_starts=None):
        """SufrFile.kmers on the device.  lcp: the LCP array as a torch CUDA tensor of the index's width (s entries);
        seq_starts: the sequence starts (host integers; None: one sequence).  Returns (hist int64 tensor, stats dict, occ
        tensor of the index's width or None), complete on return."""
        import torch
        from ._lib import KMER_BY_POSITION, KmerStats
        if occ not in (None, "rank", "position"):
            raise ValueError('occ is None, "rank" or "position"')
        dt, st, st_ptr, st_n = self._lcp_inputs(lcp, seq_starts)
        hist = torch.empty(max(bins, 1), dtype=torch.int64, device=lcp.device)
        count = None if occ is None else (lcp.numel() if occ == "rank" else self.text_len)
        out = None if occ is None else torch.empty(max(count, 1), dtype=dt, device=lcp.device)
        stats = KmerStats()
        self.ctx.check(lib().sufr_hip_kmers_device(self.ctx.handle, self._h, lcp.data_ptr(), st_ptr, st_n, k,
                                                   KMER_BY_POSITION if occ == "position" else 0, bins, hist.data_ptr(),
                                                   out.data_ptr() if out is not None else None, C.byref(stats)))
        self.ctx.synchronize()
        return hist[:bins], stats.as_dict(), (out[:count] if out is not None else None)

    def unique_lengths_device(self, lcp, by_position: bool = False, seq_starts=None):
        """SufrFile.unique_lengths on the device: a tensor of the index's width, complete on return."""
        import torch
        from ._lib import KMER_BY_POSITION
        dt, st, st_ptr, st_n = self._lcp_inputs(lcp, seq_starts)
        count = lcp.numel() if not by_position else self.text_len
        out = torch.empty(max(count, 1), dtype=dt, device=lcp.device)
        self.ctx.check(lib().sufr_hip_unique_lengths_device(self.ctx.handle, self._h, lcp.data_ptr(), st_ptr, st_n,
                                                            KMER_BY_POSITION if by_position else 0, out.data_ptr()))
        self.ctx.synchronize()
        return out[:count]

    # -- repeats of the indexed text (include/sufr_repeat.h) -----------------------------------------------------------
    def repeats_device(self, lcp, kind="branching", min_len: int = 1, min_count: int = 2, max_count: int = 0, seq_starts=None):
        """SufrFile.repeats on the device.  lcp and seq_starts as in kmers_device.  Returns (rank, count, length) as int64
        CUDA tensors and the stats dict, complete on return.  One call counts, one fills."""
        from ._lib import REPEAT_KINDS, RepeatStats
        kind = REPEAT_KINDS.get(kind, kind)
        _, st, st_ptr, st_n = self._lcp_inputs(lcp, seq_starts)
        stats = RepeatStats()
        cols = self._counted_device(lcp, 3, lambda cap, at, total: lib().sufr_hip_repeats_device(
            self.ctx.handle, self._h, lcp.data_ptr(), st_ptr, st_n, kind, min_len, min_count, max_count, cap, *at, C.byref(total), C.byref(stats)))
        return (*cols, stats.as_dict())

    # -- longest previous factors and the LZ77 parse (include/sufr_lz.h) -----------------------------------------------
    def lpf_device(self, lcp, seq_starts=None):
        """SufrFile.lpf on the device.  lcp and seq_starts as in kmers_device.  Returns (lpf, src) as CUDA tensors of the
        index's width, complete on return."""
        import torch
        dt, st, st_ptr, st_n = self._lcp_inputs(lcp, seq_starts)
        n = self.text_len
        out = [torch.empty(max(n, 1), dtype=dt, device=lcp.device) for _ in range(2)]
        self.ctx.check(lib().sufr_hip_lpf_device(self.ctx.handle, self._h, lcp.data_ptr(), st_ptr, st_n, out[0].data_ptr(), out[1].data_ptr()))
        self.ctx.synchronize()
        return out[0][:n], out[1][:n]

    def lz_device(self, lcp, seq_starts=None):
        """SufrFile.lz on the device.  Returns (start, length, source) as int64 CUDA tensors (source -1: a literal) and the
        stats dict, complete on return.  One call counts, one fills."""
        from ._lib import LzStats
        _, st, st_ptr, st_n = self._lcp_inputs(lcp, seq_starts)
        stats = LzStats()
        cols = self._counted_device(lcp, 3, lambda cap, at, total: lib().sufr_hip_lz_device(
            self.ctx.handle, self._h, lcp.data_ptr(), st_ptr, st_n, cap, *at, C.byref(total), C.byref(stats)))
        return (*cols, stats.as_dict())

    # -- sequence counts of repeats and k-common substrings (include/sufr_shared.h) -------------------------------------
    def shared_device(self, lcp, kind="branching", min_len: int = 1, min_count: int = 2, max_count: int = 0, min_seqs: int = 0,
                      max_seqs: int = 0, seq_starts=None):
        """SufrFile.shared on the device.  lcp and seq_starts as in kmers_device.  Returns (rank, count, length, seqs) as
        int64 CUDA tensors and the stats dict, complete on return.  One call counts, one fills."""
        from ._lib import REPEAT_KINDS, SharedStats
        kind = REPEAT_KINDS.get(kind, kind)
        _, st, st_ptr, st_n = self._lcp_inputs(lcp, seq_starts)
        stats = SharedStats()
        cols = self._counted_device(lcp, 4, lambda cap, at, total: lib().sufr_hip_shared_device(
            self.ctx.handle, self._h, lcp.data_ptr(), st_ptr, st_n, kind, min_len, min_count, max_count, min_seqs, max_seqs, cap, *at,
            C.byref(total), C.byref(stats)))
        return (*cols, stats.as_dict())

    def common_device(self, lcp, seq_starts=None):
        """SufrFile.common on the device: an int64 CUDA tensor of one entry per sequence, complete on return."""
        import torch
        _, st, st_ptr, st_n = self._lcp_inputs(lcp, seq_starts)
        out = torch.empty(max(st_n if st_ptr else 0, 1), dtype=torch.int64, device=lcp.device)
        self.ctx.check(lib().sufr_hip_common_device(self.ctx.handle, self._h, lcp.data_ptr(), st_ptr, st_n, out.data_ptr()))
        self.ctx.synchronize()
        return out

    # -- the BWT, its runs and the LF mapping (include/sufr_bwt.h) ------------------------------------------------------
    def _device(self):
        import torch
        return torch.device("cuda", self.ctx.device)

    def bwt_device(self):
        """SufrFile.bwt on the device: (bwt uint8 CUDA tensor, counts int64 CUDA tensor of 256 entries), complete on return."""
        import torch
        s = self.len_suffixes
        out = torch.empty(max(s, 4), dtype=torch.uint8, device=self._device())
        counts = torch.empty(256, dtype=torch.int64, device=self._device())
        self.ctx.check(lib().sufr_hip_bwt_device(self.ctx.handle, self._h, out.data_ptr(), counts.data_ptr()))
        self.ctx.synchronize()
        return out[:s], counts

    def bwt_runs_device(self, min_len: int = 1):
        """SufrFile.bwt_runs on the device: (rank, length, symbol, first) as int64 CUDA tensors and the stats dict, complete on
        return.  One call counts, one fills."""
        import torch
        from ._lib import BwtStats
        stats = BwtStats()
        cols = _counted(4, lambda cap, at, total: lib().sufr_hip_bwt_runs_device(self.ctx.handle, self._h, min_len, cap, *at, C.byref(total),
                                                                                 C.byref(stats)),
                        lambda n: [torch.empty(n, dtype=torch.int64, device=self._device()) for _ in range(4)], self.ctx.check, self.ctx.synchronize)
        return (*cols, stats.as_dict())

    def lf_device(self):
        """SufrFile.lf on the device: a CUDA tensor of the index's width, complete on return and the same bits on every run."""
        import torch
        s = self.len_suffixes
        out = torch.empty(max(s, 1), dtype=torch.int64 if self.index_width == 8 else torch.int32, device=self._device())
        self.ctx.check(lib().sufr_hip_lf_device(self.ctx.handle, self._h, out.data_ptr()))
        self.ctx.synchronize()
        return out[:s]

    # -- the FM-index over the BWT (include/sufr_fm.h) -------------------------------------------------------------------
    def fm_device(self, sample: int = 32, text: bool = False) -> "DeviceFmIndex":
        """SufrFile.fm on the device: the FM-index of this index in HBM, complete on return.  It owns everything it reads; this
        index may be closed afterwards.  text: also keep the text samples, for DeviceFmIndex.extract_device.  Refused (-6) as
        SufrFile.fm refuses."""
        import torch
        torch.cuda.current_stream(self._device()).synchronize()     # (wrapped tensors: their producer is done)
        h = C.c_void_p()
        if text:
            from ._lib import FM_TEXT
            self.ctx.check(lib().sufr_hip_fm_build_flags(self.ctx.handle, self._h, sample, FM_TEXT, C.byref(h)))
        else:
            self.ctx.check(lib().sufr_hip_fm_build(self.ctx.handle, self._h, sample, C.byref(h)))
        return DeviceFmIndex(self.ctx, h, self.index_width)

    # -- MEMs (include/sufr_mem.h) -----------------------------------------------------------------------------------
    def mems_device(self, qbytes, offsets, min_len: int = 20, max_occ: int = 0, both_strands: bool = False,
                    cap: Optional[int] = None):
        """MEMs of a packed batch of torch CUDA tensors (uint8 bytes, int64 offsets): (query int64, query_offset int32,
        strand uint8, length int32, position int64) tensors in (query, strand, offset, rank) order, complete on return.
        With a `cap` too small the SufrHipError (code -5) carries the total in `.total`; without one the outputs are sized
        to fit."""
        import torch
        from ._lib import MEM_BOTH_STRANDS
        torch.cuda.current_stream(qbytes.device).synchronize()
        nq = offsets.numel() - 1
        dev = qbytes.device
        qbytes = self._device_bytes(qbytes)
        nbytes = int(offsets[-1] - offsets[0]) if nq > 0 else 0
        flags = MEM_BOTH_STRANDS if both_strands else 0
        return self._device_records(
            cap, nbytes // 4 + 16, dev, (torch.int64, torch.int32, torch.uint8, torch.int32, torch.int64),
            lambda c, out, total: lib().sufr_hip_mems_device(self.ctx.handle, self._h, qbytes.data_ptr(), offsets.data_ptr(), max(nq, 0),
                                                             min_len, max_occ, flags, c, *[t.data_ptr() for t in out], C.byref(total)))

    def mems(self, queries: Sequence, min_len: int = 20, max_occ: int = 0, both_strands: bool = False) -> List[List[MemHit]]:
        """The MEMs of every query (SufrFile.mems), found on the device."""
        recs = self.mems_device(*self._packed(queries), min_len, max_occ, both_strands)
        return _mem_hits(len(queries), [t.cpu().numpy() for t in recs])

    # -- k-mismatch search (include/sufr_approx.h) -------------------------------------------------------------------
    def approx_device(self, qbytes, offsets, max_mismatches: int = 2, max_occ: int = 0, both_strands: bool = False,
                      cap: Optional[int] = None):
        """k-mismatch occurrences of a packed batch of torch CUDA tensors (uint8 bytes, int64 offsets): (query int64, strand
        uint8, position int64, mismatches uint8) tensors in (query, strand, piece, rank) order, complete on return.  With a
        `cap` too small the SufrHipError (code -5) carries the total in `.total`; without one the outputs are sized to fit."""
        import torch
        from ._lib import APPROX_BOTH_STRANDS
        torch.cuda.current_stream(qbytes.device).synchronize()
        nq = offsets.numel() - 1
        dev = qbytes.device
        qbytes = self._device_bytes(qbytes)
        flags = APPROX_BOTH_STRANDS if both_strands else 0
        return self._device_records(
            cap, 4 * max(nq, 0) + 16, dev, (torch.int64, torch.uint8, torch.int64, torch.uint8),
            lambda c, out, total: lib().sufr_hip_approx_device(self.ctx.handle, self._h, qbytes.data_ptr(), offsets.data_ptr(), max(nq, 0),
                                                               max_mismatches, max_occ, flags, c, *[t.data_ptr() for t in out],
                                                               C.byref(total)))

    def approx(self, queries: Sequence, max_mismatches: int = 2, max_occ: int = 0, both_strands: bool = False) -> List[List[ApproxHit]]:
        """The k-mismatch occurrences of every query (SufrFile.approx), found on the device."""
        recs = self.approx_device(*self._packed(queries), max_mismatches, max_occ, both_strands)
        return _approx_hits(len(queries), [t.cpu().numpy() for t in recs])

    # -- k-difference search (include/sufr_edit.h) -------------------------------------------------------------------
    def edit_device(self, qbytes, offsets, max_edits: int = 2, max_occ: int = 0, both_strands: bool = False,
                    local_minima: bool = False, cap: Optional[int] = None):
        """k-difference ends of a packed batch of torch CUDA tensors (uint8 bytes, int64 offsets): (query int64, strand uint8,
        end int64, edits uint8) tensors sorted by (query, strand, end), complete on return.  With a `cap` too small the
        SufrHipError (code -5) carries the total in `.total`; without one the outputs are sized to fit."""
        import torch
        torch.cuda.current_stream(qbytes.device).synchronize()
        nq = offsets.numel() - 1
        dev = qbytes.device
        qbytes = self._device_bytes(qbytes)
        flags = _edit_flags(both_strands, local_minima)
        return self._device_records(
            cap, 4 * max(nq, 0) + 16, dev, (torch.int64, torch.uint8, torch.int64, torch.uint8),
            lambda c, out, total: lib().sufr_hip_edit_device(self.ctx.handle, self._h, qbytes.data_ptr(), offsets.data_ptr(), max(nq, 0),
                                                             max_edits, max_occ, flags, c, *[t.data_ptr() for t in out],
                                                             C.byref(total)))

    def edit(self, queries: Sequence, max_edits: int = 2, max_occ: int = 0, both_strands: bool = False,
             local_minima: bool = False) -> List[List[EditHit]]:
        """The k-difference ends of every query (SufrFile.edit), found on the device."""
        recs = self.edit_device(*self._packed(queries), max_edits, max_occ, both_strands, local_minima)
        return _edit_hits(len(queries), [t.cpu().numpy() for t in recs])

    # -- alignment traceback (include/sufr_align.h) -------------------------------------------------------------------
    def edit_trace_device(self, qbytes, offsets, query, strand, end, edits, cap: Optional[int] = None):
        """Start and CIGAR of k-difference records on torch CUDA tensors (the batch and the four tensors of `edit_device`):
        (start int64, cigar_off int64[records + 1], cigar int32 holding BAM-encoded u32 runs), complete on return.  With a
        `cap` (of runs) too small the SufrHipError (code -5) carries the total in `.total`; without one the runs are sized to
        fit."""
        import torch
        torch.cuda.current_stream(qbytes.device).synchronize()
        nq, nr = offsets.numel() - 1, query.numel()
        dev = qbytes.device
        qbytes = self._device_bytes(qbytes)
        start = torch.zeros(max(nr, 1), dtype=torch.int64, device=dev)
        off = torch.zeros(nr + 1, dtype=torch.int64, device=dev)
        (cigar,) = self._device_records(
            cap, 4 * nr + 16, dev, (torch.int32,),
            lambda c, out, total: lib().sufr_hip_edit_trace_device(self.ctx.handle, self._h, qbytes.data_ptr(), offsets.data_ptr(), max(nq, 0),
                                                                   nr, query.data_ptr(), strand.data_ptr(), end.data_ptr(), edits.data_ptr(),
                                                                   c, start.data_ptr(), off.data_ptr(), out[0].data_ptr(), C.byref(total)))
        return start[:nr], off, cigar

    def edit_trace(self, qbytes: np.ndarray, offsets: np.ndarray, query, strand, end, edits, cap: Optional[int] = None):
        """`SufrFile.edit_trace_arrays` on host arrays through sufr_hip_edit_trace (staged, traced on the device, copied back)."""
        qbytes, offsets = _packed_arrays(qbytes, offsets)
        recs = [np.ascontiguousarray(a, dtype=d) for a, d in zip((query, strand, end, edits), _APPROX_DTYPES)]
        nq, nr = len(offsets) - 1, len(recs[0])
        start = np.zeros(max(nr, 1), dtype=np.uint64)
        off = np.zeros(nr + 1, dtype=np.uint64)
        (cigar,) = _sized_to_fit(
            cap, 4 * nr + 16, lambda c: [np.zeros(c, dtype=np.uint32)],
            lambda c, out, total: lib().sufr_hip_edit_trace(self.ctx.handle, self._h, qbytes.ctypes.data, offsets.ctypes.data, nq, nr,
                                                            *[a.ctypes.data for a in recs], c, start.ctypes.data, off.ctypes.data,
                                                            out[0].ctypes.data, C.byref(total)),
            lambda rc, total, c: SufrHipError(rc, lib().sufr_hip_last_error(self.ctx.handle).decode()))
        return start[:nr], off, cigar

    def align(self, queries: Sequence, max_edits: int = 2, max_occ: int = 0, both_strands: bool = False,
              local_minima: bool = False) -> List[List[AlignHit]]:
        """The hits of `edit` with the start and the CIGAR string of every one (SufrFile.align), searched and traced on the
        device."""
        dq, do = self._packed(queries)
        recs = self.edit_device(dq, do, max_edits, max_occ, both_strands, local_minima)
        recs = tuple(t.contiguous() for t in recs)
        st, co, cg = self.edit_trace_device(dq, do, *recs)
        return _align_hits(len(queries), [t.cpu().numpy() for t in recs],
                           (st.cpu().numpy(), co.cpu().numpy(), cg.cpu().numpy().view(np.uint32)))
