"""Alignment traceback of k-difference records on the host (include/sufr_align.h): no GPU.

The witness shares nothing with the library: the full (m + 1) x (n + 1) table of Sellers in numpy and the walk of
sufr_align.h over it, cell by cell.  The host path (a scalar banded table per record) and the device's arithmetic
(sufr_amd/csrc/sufr_trace.h through tests/trace_shim.cpp: bit-parallel rows, two words per row) are both held to it.
"""
import ctypes as C
import re
import subprocess
import zlib
from pathlib import Path

import numpy as np
import pytest

import sufr_amd
from sufr_amd import SufrFile, SufrHipError, pack_queries
from sufr_amd.sufr_file import cigar_string
from oracle_helper import GOLDEN
from test_match_host import run
from test_mem_host import ADVERSARIAL, BUILDS, _adversarial_body, _fasta_from, revcomp
from test_edit_host import with_indels

ROOT = Path(__file__).resolve().parent.parent
EXP = GOLDEN / "expected"
SUFR1 = EXP / "1.sufr"
DS = (0, 1, 2, 4)
OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8
GOLDEN_FILES = sorted(p.name for p in EXP.glob("*.sufr") if not SufrFile(p).seed_mask)


# ---------------------------------------------------------------------------------------------------------------------
# the witness
# ---------------------------------------------------------------------------------------------------------------------
def table(text: np.ndarray, q: bytes) -> np.ndarray:
    """C[i][j], i = 0 .. m, j = 0 .. n: row 0 is 0, column 0 is i."""
    n = text.size
    j = np.arange(n + 1, dtype=np.int64)
    tab = np.zeros((len(q) + 1, n + 1), dtype=np.int64)
    for r, c in enumerate(q, 1):
        cur = np.empty(n + 1, dtype=np.int64)
        cur[0] = r
        cur[1:] = np.minimum(tab[r - 1, :-1] + (text != c), tab[r - 1, 1:] + 1)
        tab[r] = np.minimum.accumulate(cur - j) + j                # the left neighbour: min over j' <= j of cur[j'] + j - j'
    return tab


def walk(tab: np.ndarray, text, q: bytes, end: int):
    """(start, runs) of the record that ends at `end`: diagonal first, then up, then left; runs as (len << 4 | op), forward."""
    i, j = len(q), end + 1
    ops = []
    while i > 0:
        c = tab[i, j]
        if j > 0 and tab[i - 1, j - 1] + (q[i - 1] != text[j - 1]) == c:
            ops.append(OP_EQ if q[i - 1] == text[j - 1] else OP_X)
            i, j = i - 1, j - 1
        elif tab[i - 1, j] + 1 == c:
            ops.append(OP_I)
            i -= 1
        else:
            assert j > 0 and tab[i, j - 1] + 1 == c
            ops.append(OP_D)
            j -= 1
    runs = []
    for o in reversed(ops):
        if runs and runs[-1][0] == o:
            runs[-1][1] += 1
        else:
            runs.append([o, 1])
    return j, [ln << 4 | o for o, ln in runs]


def witness(f: SufrFile, queries, recs, memo=None):
    """(start list, list of run lists, list of D(e - 1) < D(e)) of the records (query, strand, end, edits arrays), one table per
    (query, strand).  memo: tables and walks kept between calls on the same file and queries (a walk does not depend on d)."""
    text = np.asarray(f.text)
    memo = {} if memo is None else memo
    starts, cigars, falls = [], [], []
    for qi, st, end, ed in zip(*[a.tolist() for a in recs]):
        q = revcomp(queries[qi]) if st else bytes(queries[qi])
        if (qi, st) not in memo:
            memo[(qi, st)] = table(text, q)
        tab = memo[(qi, st)]
        assert tab[len(q), end + 1] == ed
        if (qi, st, end) not in memo:
            memo[(qi, st, end)] = walk(tab, text, q, end)
        s, runs = memo[(qi, st, end)]
        starts.append(s)
        cigars.append(runs)
        falls.append(bool(tab[len(q), end] < tab[len(q), end + 1]))
    return starts, cigars, falls


def test_witness_on_a_hand_checked_text():
    """T = ACGTACGA, Q = ACGA, d = 1.  The table (rows i = 0 .. 4 of Q, columns j = 0 .. 8 of T):

              -  A  C  G  T  A  C  G  A
           -  0  0  0  0  0  0  0  0  0
           A  1  0  1  1  1  0  1  1  0
           C  2  1  0  1  2  1  0  1  1
           G  3  2  1  0  1  2  1  0  1
           A  4  3  2  1  1  1  2  1  0

    end 7 (e = 8): four matches down the diagonal from (4, 8) to (0, 4): start 4, 4=.
    end 3 (e = 4, ACGT): (4, 4) = 1; A against T differs and C[3][3] + 1 = 1: diagonal, X; then G, C, A match: start 0, 3=1X.
    end 2 (e = 3, ACG): (4, 3) = 1; A against G differs and C[3][2] + 1 = 2: no diagonal; C[3][3] + 1 = 1: up, I; then three
        matches: start 0, 3=1I.
    end 4 (e = 5, ACGTA): (4, 5) = 1; A against A is equal and C[3][4] = 1: diagonal, =; at (3, 4) = 1 G against T differs and
        C[2][3] + 1 = 2: no diagonal; C[2][4] + 1 = 3: no up; left, D, to (3, 3) = 0; then three matches: start 0, 3=1D1=."""
    text = np.frombuffer(b"ACGTACGA", dtype=np.uint8)
    tab = table(text, b"ACGA")
    assert tab.tolist() == [[0, 0, 0, 0, 0, 0, 0, 0, 0], [1, 0, 1, 1, 1, 0, 1, 1, 0], [2, 1, 0, 1, 2, 1, 0, 1, 1],
                            [3, 2, 1, 0, 1, 2, 1, 0, 1], [4, 3, 2, 1, 1, 1, 2, 1, 0]]
    got = {end: walk(tab, text, b"ACGA", end) for end in (7, 3, 2, 4)}
    assert got[7] == (4, [4 << 4 | OP_EQ])
    assert got[3] == (0, [3 << 4 | OP_EQ, 1 << 4 | OP_X])
    assert got[2] == (0, [3 << 4 | OP_EQ, 1 << 4 | OP_I])
    assert got[4] == (0, [3 << 4 | OP_EQ, 1 << 4 | OP_D, 1 << 4 | OP_EQ])
    assert [cigar_string(got[e][1]) for e in (7, 3, 2, 4)] == ["4=", "3=1X", "3=1I", "3=1D1="]


# ---------------------------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_align_header_symbols_are_exported():
    inc = sufr_amd.LIB_PATH.parents[3] / "include"
    hdr = re.sub(r"/\*.*?\*/", "", (inc / "sufr_align.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(sufr_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(sufr_amd.ALIGN_EXPORTS), declared ^ set(sufr_amd.ALIGN_EXPORTS)
    L = sufr_amd.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(sufr_amd.LIB_PATH)], capture_output=True, text=True).stdout
    for name in declared:
        assert hasattr(L, name), name
        assert re.search(rf"\bT {name}\b", nm), name
    assert L.sufr_hip_abi_version() == 3
    # sufr_edit.h keeps its declarations and its three constants
    edit = (inc / "sufr_edit.h").read_text()
    assert "#define SUFR_EDIT_BOTH_STRANDS 0x1u" in edit and "#define SUFR_EDIT_LOCAL_MINIMA 0x2u" in edit and "#define SUFR_EDIT_MAX_EDITS 15u" in edit
    assert sufr_amd.EDIT_EXPORTS == ["sufr_file_edit", "sufr_hip_edit_device", "sufr_hip_edit"]


# ---------------------------------------------------------------------------------------------------------------------
# the host against the witness
# ---------------------------------------------------------------------------------------------------------------------
SEEN = dict(ops=set(), most_runs=0, start0=0, last_end=0, records=0)


def check_invariants(f: SufrFile, queries, recs, trace, minima, falls, all_ends):
    """What follows from the rule, on every record.  falls[t]: D(e - 1) < D(e); all_ends: the (query, strand, end) of the records
    without SUFR_EDIT_LOCAL_MINIMA.  A last D means D(e - 1) < D(e), so a local minimum ends on one only where e - 1 is no record
    (sufr_edit.h: such a neighbour counts as d + 1), which takes an array that leaves positions out."""
    start, off, cigar = trace
    lens = [len(q) for q in queries]
    assert off[0] == 0 and len(off) == len(recs[0]) + 1 and off[-1] == len(cigar)
    for t, (qi, st, end, ed) in enumerate(zip(*[a.tolist() for a in recs])):
        runs = cigar[int(off[t]):int(off[t + 1])].tolist()
        ops = [r & 15 for r in runs]
        by = {o: sum(r >> 4 for r in runs if r & 15 == o) for o in (OP_I, OP_D, OP_EQ, OP_X)}
        assert runs and set(ops) <= {OP_I, OP_D, OP_EQ, OP_X} and all(r >> 4 for r in runs)
        assert by[OP_X] + by[OP_I] + by[OP_D] == ed
        assert int(start[t]) + by[OP_EQ] + by[OP_X] + by[OP_D] == end + 1
        assert by[OP_EQ] + by[OP_X] + by[OP_I] == lens[qi]
        assert all(a != b for a, b in zip(ops, ops[1:]))
        assert ops[0] != OP_D and (ops[0] != OP_I or start[t] == 0)
        if ops[-1] == OP_D:
            assert falls[t]
            assert not minima or ((qi, st, end - 1) not in all_ends and f.len_suffixes < f.text_len)
        SEEN["ops"].update(ops)
        SEEN["most_runs"] = max(SEEN["most_runs"], len(runs))
        SEEN["start0"] += int(start[t] == 0)
        SEEN["last_end"] += int(end == f.text_len - 1)
        SEEN["records"] += 1


def check_file(f: SufrFile, queries, threads=0):
    """Host == witness for d in DS, both strands, minima on and off; the number of records."""
    qb, off = pack_queries(queries)
    n, memo = 0, {}
    for d in DS:
        for minima in (False, True):
            recs = f.edit_arrays(qb, off, d, 0, True, minima)
            if not minima:
                all_ends = set(zip(*[a.tolist() for a in recs[:3]]))
            trace = f.edit_trace_arrays(qb, off, *recs, threads=threads)
            want_start, want_cigar, falls = witness(f, queries, recs, memo)
            assert trace[0].tolist() == want_start, (d, minima)
            got_cigar = [trace[2][int(trace[1][t]):int(trace[1][t + 1])].tolist() for t in range(len(want_cigar))]
            assert got_cigar == want_cigar, (d, minima)
            check_invariants(f, queries, recs, trace, minima, falls, all_ends)
            n += len(want_start)
    return n


def golden_queries(name, f):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    big = f.text_len > 2000
    return with_indels(rng, f, 10 if big else 40, 60 if big else 16)


@pytest.mark.parametrize("name", GOLDEN_FILES)
def test_host_equals_witness_on_golden_files(name):
    f = SufrFile(EXP / name)
    assert check_file(f, golden_queries(name, f)) > 0


@pytest.mark.parametrize("kind", ADVERSARIAL)
@pytest.mark.parametrize("build", BUILDS)
def test_host_equals_witness_on_oracle_builds(oracle, tmp_path, kind, build):
    _fasta_from(_adversarial_body(kind), tmp_path / "x.fa")
    oracle.create(tmp_path / "x.fa", tmp_path / "x.sufr", **build)
    f = SufrFile(tmp_path / "x.sufr")
    rng = np.random.default_rng(zlib.crc32(f"{kind}{build}".encode()))
    queries = with_indels(rng, f, 10, 40) + [b"A" * 40, b"NACGTACGT", bytes(f.text)[-12:]]
    assert check_file(f, queries) > 0


def test_host_equals_witness_on_a_protein_build(oracle, tmp_path):
    rng = np.random.default_rng(8)
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    body = aa[rng.integers(0, 20, 1500)].copy()
    body[700:760] = body[100:160]
    body[[400, 900]] = ord("%")
    _fasta_from(body, tmp_path / "p.fa")
    oracle.create(tmp_path / "p.fa", tmp_path / "p.sufr", is_dna=False)
    f = SufrFile(tmp_path / "p.sufr")
    assert check_file(f, with_indels(rng, f, 30, 50)) > 0


def test_the_runs_cover_what_the_rule_can_give():
    """Over the golden files: each of the four ops, a CIGAR of five runs or more, a start at 0, an end at n - 1."""
    if not SEEN["records"]:                                        # (run on its own: the other tests fill SEEN)
        for name in GOLDEN_FILES:
            f = SufrFile(EXP / name)
            check_file(f, golden_queries(name, f))
    assert SEEN["ops"] == {OP_I, OP_D, OP_EQ, OP_X}, SEEN
    assert SEEN["most_runs"] >= 5 and SEEN["start0"] >= 1 and SEEN["last_end"] >= 1, SEEN


@pytest.mark.parametrize("threads", [1, 3, 16])
def test_threads_do_not_change_the_answer(threads):
    f = SufrFile(EXP / "long_dna_sequence.sufr")
    qb, off = pack_queries(with_indels(np.random.default_rng(4), f, 300, 150))
    recs = f.edit_arrays(qb, off, 3, 0, True, True)
    want = f.edit_trace_arrays(qb, off, *recs, threads=2)
    got = f.edit_trace_arrays(qb, off, *recs, threads=threads)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and len(want[0]) > 64


def test_seed_mask_and_capped_files_are_traced(oracle, tmp_path):
    """The call reads the text alone: the records of the plain file hold on the masked file of the same text."""
    p, k = SufrFile(EXP / "uniprot.sufr"), SufrFile(EXP / "uniprot-masked.sufr")
    assert k.seed_mask and bytes(p.text) == bytes(k.text)
    qb, off = pack_queries(with_indels(np.random.default_rng(2), p, 10, 40))
    recs = p.edit_arrays(qb, off, 2)
    assert len(recs[0]) > 0
    assert all(np.array_equal(a, b) for a, b in zip(p.edit_trace_arrays(qb, off, *recs), k.edit_trace_arrays(qb, off, *recs)))


def test_align_is_edit_with_start_and_cigar():
    f = SufrFile(SUFR1)                                            # ACGTNNACGT$, --dna
    hits = f.align([b"ACGA", b"GTNNAC"], 1, both_strands=True)
    assert [[(h.query, h.strand, h.end, h.edits) for h in hs] for hs in hits] == \
           [[(h.query, h.strand, h.end, h.edits) for h in hs] for hs in f.edit([b"ACGA", b"GTNNAC"], 1, both_strands=True)]
    assert [(h.end, h.start, h.cigar) for h in hits[1] if h.strand == 0 and h.edits == 0] == [(7, 2, "6=")]
    assert sufr_amd.SuffixArray.read(str(SUFR1)).align(["ACGA"], max_edits=1) == f.align([b"ACGA"], 1)
    assert f.align([], 1) == [] and f.align([b""], 0) == [[]]


# ---------------------------------------------------------------------------------------------------------------------
# the device's arithmetic (sufr_trace.h) against the witness
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    out = ROOT / "tests" / "_build" / "libtrace_shim.so"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "trace_shim.cpp"
    hdr = ROOT / "sufr_amd" / "csrc" / "sufr_trace.h"
    if not out.exists() or out.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(out), str(src)], check=True)
    L = C.CDLL(str(out))
    L.shim_trace.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.shim_trace.restype = C.c_int
    return L


def shim_trace(L, text, q, end, edits):
    st, nr = C.c_uint64(0), C.c_uint32(0)
    cg = np.zeros(len(q) + 40, dtype=np.uint32)
    qa = np.frombuffer(bytes(q), dtype=np.uint8)
    if not L.shim_trace(text.ctypes.data, text.size, qa.ctypes.data, qa.size, end, edits, C.byref(st), C.byref(nr), cg.ctypes.data, cg.size):
        return None
    return st.value, cg[:nr.value].tolist()


@pytest.mark.parametrize("sigma", [2, 3, 4, 5])
def test_device_step_equals_witness(shim, sigma):
    """Random texts over `sigma` symbols, slices with planted edits: every end with D(e) <= 15, the ends near 0 and near n among
    them, is traced with edits = D(e) and refused with D(e) - 1 and D(e) + 1."""
    rng = np.random.default_rng(sigma)
    widest, traced, refused, near = 0, 0, 0, set()
    for trial in range(60):
        n = int(rng.integers(20, 160))
        text = rng.integers(65, 65 + sigma, n).astype(np.uint8)
        at, m = int(rng.integers(0, n)), int(rng.integers(1, 70))
        q = bytearray(text[at:at + m].tobytes())
        for _ in range(int(rng.integers(0, 16))):
            kind, where, sym = int(rng.integers(0, 3)), int(rng.integers(0, max(len(q), 1))), int(rng.integers(65, 65 + sigma))
            if kind == 0 and q:
                q[where] = sym
            elif kind == 1:
                q.insert(where, sym)
            elif len(q) > 1:
                del q[where]
        q = bytes(q)
        if not q:
            continue
        tab = table(text, q)
        for e in range(1, n + 1):
            D = int(tab[len(q), e])
            for v in (D - 1, D, D + 1):
                if not 0 <= v <= 15 or len(q) < v + 1:
                    continue
                got = shim_trace(shim, text, q, e - 1, v)
                if v != D:
                    assert got is None, (trial, e, v, D)
                    refused += 1
                    continue
                assert got == walk(tab, text, q, e - 1), (trial, e, v)
                traced += 1
                widest = max(widest, v)
                if got[0] == 0:
                    near.add("start")
                if e == n:
                    near.add("end")
    assert traced > 1000 and refused > 1000 and widest == 15 and near == {"start", "end"}


# ---------------------------------------------------------------------------------------------------------------------
# rejections and capacity
# ---------------------------------------------------------------------------------------------------------------------
def _raw_trace(f, qb, off, recs, cap, cigar):
    L = sufr_amd.lib()
    nr = len(recs[0])
    start = np.zeros(max(nr, 1), dtype=np.uint64)
    coff = np.full(nr + 1, 0xAB, dtype=np.uint64)
    total = C.c_uint64(0)
    err = C.create_string_buffer(512)
    rc = L.sufr_file_edit_trace(f._h, qb.ctypes.data, off.ctypes.data, len(off) - 1, nr, *[a.ctypes.data for a in recs], cap,
                                start.ctypes.data, coff.ctypes.data, cigar.ctypes.data if cigar is not None else None,
                                C.byref(total), 1, err, len(err))
    return rc, total.value, start, coff, err.value.decode()


def test_records_that_are_none_are_refused():
    f = SufrFile(EXP / "3.sufr")
    text = bytes(f.text)
    queries = [text[10:30] + b"X" + text[31:50], text[50:58], text[0:3]]
    qb, off = pack_queries(queries)
    good = f.edit_arrays(qb, off, 2)
    assert len(good[0]) >= 3
    t = next(i for i in range(len(good[0])) if good[3][i] == 1 and good[0][i] == 0)       # a record with D = 1
    want = f.edit_trace_arrays(qb, off, *good)

    def broken(at, field, value):
        recs = [a.copy() for a in good]
        recs[field][at] = value
        with pytest.raises(SufrHipError) as e:
            f.edit_trace_arrays(qb, off, *recs)
        assert e.value.code == -1 and f"record {at}" in e.value.message, e.value.message
    broken(t, 0, len(queries))                                     # query >= num_queries
    broken(t, 1, 2)                                                # strand > 1
    broken(t, 2, f.text_len)                                       # end >= n
    broken(t, 3, 16)                                               # edits > SUFR_EDIT_MAX_EDITS
    recs = [a.copy() for a in good]                                # m < edits + 1: 3 edits on the 3-byte query
    recs[0][t], recs[3][t] = 2, 3
    with pytest.raises(SufrHipError) as e:
        f.edit_trace_arrays(qb, off, *recs)
    assert e.value.code == -1 and f"record {t}" in e.value.message
    broken(t, 3, 0)                                                # edits one below D
    broken(t, 3, 2)                                                # edits one above D
    # the first offending record is named
    recs = [a.copy() for a in good]
    recs[3][len(recs[3]) - 1], recs[3][1] = 9, 9
    with pytest.raises(SufrHipError) as e:
        f.edit_trace_arrays(qb, off, *recs, threads=4)
    assert re.search(r"record 1\b", e.value.message), e.value.message
    got = f.edit_trace_arrays(qb, off, *good)                      # and the file answers as before
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_capacity_and_empty_batches():
    f = SufrFile(EXP / "3.sufr")
    text = bytes(f.text)
    queries = [text[0:30] + b"X" + text[31:50] + text[52:70], text[50:90], b"QQ"]
    qb, off = pack_queries(queries)
    recs = f.edit_arrays(qb, off, 2, both_strands=True)
    start, coff, cigar = f.edit_trace_arrays(qb, off, *recs)
    total = len(cigar)
    assert total > len(recs[0]) >= 2 and coff[-1] == total
    for cap in (0, total - 1):
        with pytest.raises(SufrHipError) as e:
            f.edit_trace_arrays(qb, off, *recs, cap=cap)
        assert e.value.code == -5 and e.value.total == total
        buf = np.full(total + 8, 0xABABABAB, dtype=np.uint32)
        rc, tot, s2, c2, msg = _raw_trace(f, qb, off, recs, cap, buf)
        assert rc == -5 and tot == total and str(total) in msg
        assert np.array_equal(s2, start) and np.array_equal(c2, coff)
        assert (buf[cap:] == 0xABABABAB).all()                     # nothing at or beyond the cap
        assert np.array_equal(buf[:cap], cigar[:cap])              # (this implementation fills what fits)
    rc, tot, s2, c2, _ = _raw_trace(f, qb, off, recs, 0, None)     # the sizing call
    assert rc == -5 and tot == total and np.array_equal(c2, coff)
    got = f.edit_trace_arrays(qb, off, *recs, cap=total)
    assert np.array_equal(got[2], cigar)
    none = [np.zeros(0, dtype=d) for d in (np.uint64, np.uint8, np.uint64, np.uint8)]
    rc, tot, _, c2, _ = _raw_trace(f, qb, off, none, 0, None)
    assert rc == 0 and tot == 0 and c2.tolist() == [0]
    s0, c0, g0 = f.edit_trace_arrays(qb, off, *none)
    assert len(s0) == 0 and c0.tolist() == [0] and len(g0) == 0


# ---------------------------------------------------------------------------------------------------------------------
# sufr edit -c
# ---------------------------------------------------------------------------------------------------------------------
def _where(f, pos, absolute):
    if absolute:
        return str(pos)
    k = f._sequence_of(pos)
    return f"{f.sequence_names[k]}:{pos - f.sequence_starts[k]}"


def test_cli_appends_start_and_cigar(tmp_path):
    path = EXP / "long_dna_sequence.sufr"
    f = SufrFile(path)
    reads = [r for r in with_indels(np.random.default_rng(3), f, 60, 120, extra=b"N") if r and not set(r) & set(b"$%")]
    fa = tmp_path / "r.fa"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    for opts, kw in ((["-d", 2], dict(max_edits=2)), (["-d", 4, "-b", "-l"], dict(max_edits=4, both_strands=True, local_minima=True))):
        hits = [h for hs in f.align(reads, **kw) for h in hs]
        assert len(hits) > 0
        for absolute in (False, True):
            extra = ["-a"] if absolute else []
            plain = run("edit", *opts, *extra, "-q", fa, path).stdout
            traced = run("edit", *opts, *extra, "--cigar" if absolute else "-c", "-q", fa, path).stdout
            rows = [ln.split("\t") for ln in traced.splitlines()]
            assert all(len(r) == 6 for r in rows) and len(rows) == len(hits)
            assert "".join("\t".join(r[:4]) + "\n" for r in rows) == plain
            assert [(r[4], r[5]) for r in rows] == [(_where(f, h.start, absolute), h.cigar) for h in hits]
    assert "--cigar" in run("--help").stdout
    assert run("approx", "-c", SUFR1, "ACGT", check=False).returncode == 2
