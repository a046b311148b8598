"""Repeats of the indexed text on the host (include/sufr_repeat.h): no GPU.

Two witnesses.  The dictionary witness uses no suffix order and no LCP array: it groups the indexed positions by every
break-free prefix, one more symbol per round, and classifies each group of two or more by the text-level rules of the
header (following symbols, preceding symbols, a break different from everything).  The serial witness is a stack pass over
the clipped LCP in Python; it fixes the record order and the stats.  The shared arithmetic of the device path
(sufr_amd/csrc/sufr_repeat_scan.h through tests/repeat_shim.cpp) is held to a linear scan.
"""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sufr_amd
from sufr_amd import SufrFile, SufrHipError, synth
from oracle_helper import GOLDEN
from test_match_host import run
from test_mem_host import _fasta_from

ROOT = Path(__file__).resolve().parent.parent
EXP = GOLDEN / "expected"
GOLDEN_FILES = sorted(p.name for p in EXP.glob("*.sufr"))
KINDS = (0, 1, 2)
FILTERS = [(ml, mc, xc) for ml in (1, 2, 8) for mc in (2, 3) for xc in (0, 2)]


# ---------------------------------------------------------------------------------------------------------------------
# the witnesses
# ---------------------------------------------------------------------------------------------------------------------
def brk_of(f: SufrFile) -> np.ndarray:
    n = f.text_len
    breaks = np.array(sorted({n - 1} | {s - 1 for s in f.sequence_starts[1:]}), dtype=np.int64)
    return breaks[np.searchsorted(breaks, np.arange(n, dtype=np.int64), side="left")]


def witness_dictionary(f: SufrFile):
    """{kind: set of (length, frozenset of positions)} with open filters, from the text and the set of indexed positions"""
    tb = bytes(f.text)
    brk = brk_of(f).tolist()
    starts = set(f.sequence_starts) | {0}
    out = {k: set() for k in KINDS}
    groups = [sorted(set(np.asarray(f.suffix_array).tolist()))]
    length = 0
    while groups:
        length += 1
        nxt = []
        for g in groups:
            split = {}
            for p in g:
                if p + length <= brk[p]:                              # the prefix of `length` symbols holds no break
                    split.setdefault(tb[p + length - 1], []).append(p)
            nxt.extend(ps for ps in split.values() if len(ps) >= 2)
        groups = nxt
        for g in groups:
            fol = {tb[p + length] if p + length < brk[p] else ("break", p) for p in g}
            if len(fol) == 1:
                continue
            rec = (length, frozenset(g))
            out[0].add(rec)
            pre = {("start", p) if p in starts else tb[p - 1] for p in g}
            if len(pre) > 1:
                out[1].add(rec)
            if len(pre) == len(g) and len(fol) == len(g):
                out[2].add(rec)
    return out


def filtered(recs, min_len, min_count, max_count):
    return {(ln, ps) for ln, ps in recs if ln >= min_len and len(ps) >= max(min_count, 2) and (max_count == 0 or len(ps) <= max_count)}


def host_set(f: SufrFile, kind, min_len, min_count=2, max_count=0, threads=0):
    sa = np.asarray(f.suffix_array).astype(np.int64)
    rank, count, length, st = f.repeats(kind, min_len, min_count, max_count, threads=threads)
    recs = [(int(ln), frozenset(sa[int(a):int(a) + int(c)].tolist())) for a, c, ln in zip(rank, count, length)]
    assert len(set(recs)) == len(recs) == st["records"]
    return set(recs)


def clipped(f: SufrFile) -> np.ndarray:
    """l[0..s] (l[s] = 0) from the arrays and the sequence starts"""
    sa = np.asarray(f.suffix_array).astype(np.int64)
    lcp = np.asarray(f.lcp).astype(np.int64)
    ell = np.zeros(sa.size + 1, dtype=np.int64)
    if sa.size > 1:
        room = brk_of(f)[sa] - sa
        ell[1:-1] = np.minimum(lcp[1:], np.minimum(room[:-1], room[1:]))
    return ell


def left_codes(f: SufrFile) -> np.ndarray:
    """lambda of every rank as an integer: the byte, or 256 + p for a sequence start p"""
    sa = np.asarray(f.suffix_array).astype(np.int64)
    text = np.asarray(f.text)
    is_start = np.isin(sa, np.array(sorted(set(f.sequence_starts) | {0}), dtype=np.int64))
    return np.where(is_start, 256 + sa, text[np.maximum(sa - 1, 0)].astype(np.int64))


def witness_serial(f: SufrFile, kind, min_len, min_count=2, max_count=0):
    """(rank, count, length, stats) by a stack pass over the clipped LCP, records in representative order"""
    ell = clipped(f).tolist()
    s = len(ell) - 1
    lam = left_codes(f)
    diff = np.concatenate([[0], np.cumsum(np.concatenate([[0], lam[1:] != lam[:-1]]))]) if s else np.zeros(1, dtype=np.int64)
    prev_le, nxt_lt, stack = [-1] * s, [s] * s, []
    for r in range(s):                                                # nearest j < r with l[j] <= l[r]
        while stack and ell[stack[-1]] > ell[r]:
            stack.pop()
        prev_le[r] = stack[-1] if stack else -1
        stack.append(r)
    stack = []
    for r in range(s - 1, -1, -1):                                    # nearest j > r with l[j] < l[r]
        while stack and ell[stack[-1]] >= ell[r]:
            stack.pop()
        nxt_lt[r] = stack[-1] if stack else s
        stack.append(r)
    min_count = max(min_count, 2)
    ell_np = np.array(ell, dtype=np.int64)
    recs, best = [], (0, 0, 0)
    for r in range(1, s):
        v = ell[r]
        a = prev_le[r]
        if v < min_len or a < 0 or ell[a] == v:
            continue
        b = nxt_lt[r]
        c = b - a
        if c < min_count or (max_count and c > max_count):
            continue
        differing = int(diff[b] - diff[a + 1])                        # ranks in (a, b) that differ from their predecessor
        if kind == 1 and differing == 0:
            continue
        if kind == 2 and not (differing == c - 1 and (ell_np[a + 1:b] == v).all() and np.unique(lam[a:b]).size == c):
            continue
        recs.append((a, c, v))
        if v > best[0]:
            best = (v, a, r)
    stats = dict(records=len(recs), longest=best[0], longest_rank=best[1], max_count=max((c for _, c, _ in recs), default=0))
    cols = [np.array([x[i] for x in recs], dtype=np.uint64) for i in range(3)]
    return cols[0], cols[1], cols[2], stats


def same_as_serial(f: SufrFile, kind, min_len, min_count=2, max_count=0, threads=0):
    want = witness_serial(f, kind, min_len, min_count, max_count)
    got = f.repeats(kind, min_len, min_count, max_count, threads=threads)
    for i in range(3):
        assert got[i].dtype == np.uint64 and np.array_equal(got[i], want[i]), (kind, min_len, min_count, max_count, i)
    assert got[3] == want[3], (kind, min_len, min_count, max_count, got[3], want[3])
    return got


# ---------------------------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_repeat_header_symbols_are_exported():
    hdr = (ROOT / "include" / "sufr_repeat.h").read_text()
    for line in ("#define SUFR_REPEAT_BRANCHING 0u", "#define SUFR_REPEAT_MAXIMAL 1u", "#define SUFR_REPEAT_SUPERMAXIMAL 2u"):
        assert line in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(sufr_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(sufr_amd.REPEAT_EXPORTS), declared ^ set(sufr_amd.REPEAT_EXPORTS)
    L = sufr_amd.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(sufr_amd.LIB_PATH)], capture_output=True, text=True).stdout
    for name in declared:
        assert hasattr(L, name) and re.search(rf"\bT {name}\b", nm), name
    assert L.sufr_hip_abi_version() == 3
    assert C.sizeof(sufr_amd.RepeatStats) == 32


def test_host_stubs_define_the_device_entry_points():
    stubs = (ROOT / "sufr_amd" / "csrc" / "sufr_host_stubs.cpp").read_text()
    for name in sufr_amd.REPEAT_EXPORTS:
        if name.startswith("sufr_hip_"):
            assert re.search(rf"\bint {name}\(", stubs), name


# ---------------------------------------------------------------------------------------------------------------------
# against the dictionary witness
# ---------------------------------------------------------------------------------------------------------------------
def check_dictionary(f: SufrFile, seen):
    want = witness_dictionary(f)
    assert want[2] <= want[1] <= want[0]
    for kind in KINDS:
        for ml, mc, xc in FILTERS:
            exp = filtered(want[kind], ml, mc, xc)
            assert host_set(f, kind, ml, mc, xc) == exp, (kind, ml, mc, xc)
        seen[kind] += len(want[kind])
    if want[2] < want[1] < want[0]:
        seen["strict"] += 1
    same_as_serial(f, 0, 1)
    same_as_serial(f, 1, 2, 2, 5)
    same_as_serial(f, 2, 1)


def test_host_equals_dictionary_witness_on_golden_files():
    seen = {0: 0, 1: 0, 2: 0, "strict": 0}
    used = 0
    for name in GOLDEN_FILES:
        f = SufrFile(EXP / name)
        if f.seed_mask:
            for kind in KINDS:
                with pytest.raises(SufrHipError) as e:
                    f.repeats(kind, 3)
                assert e.value.code == -6
            continue
        check_dictionary(f, seen)
        used += 1
    assert used >= 10 and all(seen[k] > 0 for k in KINDS) and seen["strict"] > 0, seen


def oracle_file(oracle, tmp_path, body, name="x", **build):
    _fasta_from(body, tmp_path / f"{name}.fa")
    oracle.create(tmp_path / f"{name}.fa", tmp_path / f"{name}.sufr", **build)
    return SufrFile(tmp_path / f"{name}.sufr")


def small_bodies():
    """texts of at most ~600 symbols ('%' separates sequences)"""
    out = {kind: synth.adversarial(kind, 600, seed=3)[:-1] for kind in ("all_a", "tandem", "fib", "two_identical", "n_run", "acgt_k")}
    rng = np.random.default_rng(5)
    piece = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 90)]
    other = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, 120)]
    sep = np.frombuffer(b"%", dtype=np.uint8)
    # the same sequence twice and once more with a prefix cut off (sequence-start lambdas), N inside, a short last sequence
    out["several"] = np.concatenate([piece, sep, other, sep, piece, sep, piece[7:], sep, other[:30]])
    return out


@pytest.mark.parametrize("build", [dict(is_dna=True), dict(is_dna=True, allow_ambiguity=True), dict(is_dna=False)],
                         ids=["dna", "ambiguity", "bytes"])
def test_host_equals_dictionary_witness_on_oracle_builds(oracle, tmp_path, build):
    seen = {0: 0, 1: 0, 2: 0, "strict": 0}
    for kind, body in small_bodies().items():
        f = oracle_file(oracle, tmp_path, body, kind, **build)
        if kind in ("several", "two_identical"):
            assert f.num_sequences >= 2
        check_dictionary(f, seen)
        if kind == "several":
            # the twice-present sequence is one supermaximal repeat: both occurrences begin a sequence
            st = f.sequence_starts
            assert (90, frozenset({st[0], st[2]})) in host_set(f, 2, 1)
    assert all(seen[k] > 0 for k in KINDS) and seen["strict"] > 0, seen


# ---------------------------------------------------------------------------------------------------------------------
# against the serial witness: order, stats, chunks
# ---------------------------------------------------------------------------------------------------------------------
def test_chunks_threads_order_and_stats_on_a_larger_text(oracle, tmp_path):
    """150 000 symbols in five sequences with planted repeats: more than two chunks of the host passes, intervals that
    cross chunk ends, any number of workers"""
    rng = np.random.default_rng(11)
    body = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 150_000)].copy()
    body[20_000:90_000] = ord("A")                                   # nested intervals over more than a chunk of ranks
    for at in range(100_000, 140_000, 4_000):
        body[at:at + 300] = body[95_000:95_300]
    body[[30_000, 60_000, 99_000, 120_000]] = ord("%")
    f = oracle_file(oracle, tmp_path, body, is_dna=True, threads=4)
    assert f.num_sequences == 5 and f.len_suffixes > 1 << 17 == 2 * 65536
    ell = clipped(f)
    # an interval that spans a chunk boundary of the host path (2^16 ranks)
    assert ell[65536 - 5:65536 + 5].min() > 100
    for kind, ml, mc, xc in ((0, 12, 2, 0), (1, 12, 2, 0), (1, 20, 3, 50), (2, 12, 2, 0), (0, 250, 2, 0)):
        want = same_as_serial(f, kind, ml, mc, xc, threads=1)
        assert want[3]["records"] > 0
        for threads in (0, 2, 7):
            got = f.repeats(kind, ml, mc, xc, threads=threads)
            assert all(np.array_equal(got[i], want[i]) for i in range(3)) and got[3] == want[3]
    st = f.repeats(0, 1)[3]
    assert st["longest"] == int(ell.max()) > 20_000 and st["max_count"] > 20_000


def test_longest_ties_go_to_the_smallest_representative(oracle, tmp_path):
    # two different repeats of the same, longest length: TGATTACAGG twice and CCTTGGAAGC twice
    body = np.frombuffer(b"TGATTACAGGCTGATTACAGGAC%ACCTTGGAAGCTTCCTTGGAAGCA", dtype=np.uint8)
    f = oracle_file(oracle, tmp_path, body, is_dna=True)
    rank, count, length, st = same_as_serial(f, 0, 1)
    top = np.nonzero(length == length.max())[0]
    assert top.size >= 2 and st["longest"] == int(length.max()) and st["longest_rank"] == int(rank[top[0]])
    assert f.repeats(0, int(length.max()) + 1)[3] == dict(records=0, longest=0, longest_rank=0, max_count=0)


def test_positional_breaks_split_intervals(oracle, tmp_path):
    from test_kmer_host import positional_breaks_file
    f = positional_breaks_file(oracle, tmp_path)
    assert f.sequence_starts == [0, 700, 1500]
    for kind in KINDS:
        for ml, mc, xc in ((1, 2, 0), (600, 2, 0), (5, 3, 40)):
            same_as_serial(f, kind, ml, mc, xc)
    # in the text A^n every length has one repeat; with positional breaks the clipped ranks cut it into several intervals
    _, _, length, _ = f.repeats(0, 1)
    assert np.bincount(length.astype(np.int64)).max() > 1


def many_left_symbols_body(units=300):
    """L_i Q R_i, i < units: the R_i are different two-letter words in ascending order, so the suffixes that begin with Q
    stand in the order of i, and L_i alternates between A and B, so neighbouring occurrences of Q differ in their left symbol
    while only two left symbols exist: the interval of Q is a supermaximal candidate that passes the neighbour check and
    falls to the limit of 256 occurrences that are not sequence starts"""
    letters = b"CDEFGHIJKLMNOPRSTUVWXYZ"
    assert units <= len(letters) ** 2
    return np.frombuffer(b"".join(bytes([b"AB"[i % 2], ord("Q"), letters[i // len(letters)], letters[i % len(letters)]])
                                  for i in range(units)), dtype=np.uint8)


def crowded_candidate(f: SufrFile):
    """(a, b) of an interval of more than 256 occurrences, none a sequence start, whose neighbours all differ in lambda"""
    sa = np.asarray(f.suffix_array).astype(np.int64)
    text = np.asarray(f.text)
    a = int(np.nonzero(text[sa] == ord("Q"))[0].min())
    b = int(np.nonzero(text[sa] == ord("Q"))[0].max()) + 1
    lam = left_codes(f)
    ell = clipped(f)
    assert b - a > 256 and (text[sa[a:b]] == ord("Q")).all() and ell[a] < 1 and ell[b] < 1 and (ell[a + 1:b] >= 1).all()
    assert (lam[a:b] < 256).all() and (lam[a + 1:b] != lam[a:b - 1]).all() and np.unique(lam[a:b]).size == 2
    return a, b


def test_supermaximal_candidate_with_more_than_256_occurrences(oracle, tmp_path):
    f = oracle_file(oracle, tmp_path, many_left_symbols_body(), "q", is_dna=False)
    a, b = crowded_candidate(f)
    rank, count, length, _ = same_as_serial(f, 0, 1)
    assert ((rank == a) & (count == b - a) & (length == 1)).any()                 # the interval of Q itself
    for ml in (1, 2):
        got = same_as_serial(f, 2, ml)
        assert not ((got[0] == a) & (got[1] == b - a)).any()
    assert same_as_serial(f, 1, 1)[3]["records"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# capacity, refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_capacity_and_counting_calls():
    f = SufrFile(EXP / "long_dna_sequence.sufr")
    L = sufr_amd.lib()
    want = f.repeats(1, 3)
    total_want = want[3]["records"]
    assert total_want > 10
    total, st = C.c_uint64(0), sufr_amd.RepeatStats()
    assert L.sufr_file_repeats(f._h, 1, 3, 0, 0, 0, None, None, None, C.byref(total), C.byref(st), 1) == -5      # the counting call
    assert total.value == total_want and st.as_dict() == want[3]
    out = [np.full(total_want + 3, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64) for _ in range(3)]
    total.value = 0
    assert L.sufr_file_repeats(f._h, 1, 3, 0, 0, total_want - 1, *(a.ctypes.data for a in out), C.byref(total), None, 1) == -5
    assert total.value == total_want and all((a == 0xFFFFFFFFFFFFFFFF).all() for a in out)                      # nothing written
    assert L.sufr_file_repeats(f._h, 1, 3, 0, 0, total_want + 3, *(a.ctypes.data for a in out), C.byref(total), None, 1) == 0
    for i in range(3):
        assert np.array_equal(out[i][:total_want], want[i]) and (out[i][total_want:] == 0xFFFFFFFFFFFFFFFF).all()
    # min_count 0 and 1 mean 2; nothing kept: a counting call that succeeds
    assert L.sufr_file_repeats(f._h, 1, 3, 1, 0, 0, None, None, None, C.byref(total), None, 1) == -5 and total.value == total_want
    assert L.sufr_file_repeats(f._h, 0, 1 << 40, 0, 0, 0, None, None, None, C.byref(total), C.byref(st), 1) == 0
    assert total.value == 0 and st.as_dict() == dict(records=0, longest=0, longest_rank=0, max_count=0)
    assert L.sufr_file_repeats(None, 0, 1, 0, 0, 0, None, None, None, None, None, 1) == -1


def test_refusals(oracle, tmp_path):
    f = SufrFile(EXP / "uniprot-masked.sufr")
    assert f.seed_mask
    g = oracle_file(oracle, tmp_path, synth.adversarial("tandem", 600, seed=3)[:-1], is_dna=True, max_query_len=6)
    assert g.max_query_len == 6
    for h in (f, g):
        for kind in KINDS:
            with pytest.raises(SufrHipError) as e:
                h.repeats(kind, 3)
            assert e.value.code == -6
    h = SufrFile(EXP / "3.sufr")
    for call in (lambda: h.repeats(0, 0), lambda: h.repeats(3, 1)):
        with pytest.raises(SufrHipError) as e:
            call()
        assert e.value.code == -1


def _rewrite(f: SufrFile, path, starts, sa=None, lcp=None):
    text = np.asarray(f.text).copy()
    sa = np.asarray(f.suffix_array).copy() if sa is None else sa
    lcp = np.asarray(f.lcp).copy() if lcp is None else lcp
    st = np.array(starts, dtype=np.uint64)
    names = (C.c_char_p * len(starts))(*[b"s%d" % i for i in range(len(starts))])
    err = C.create_string_buffer(256)
    rc = sufr_amd.lib().sufr_write_file(str(path).encode(), 1, 0, 0, text.ctypes.data, text.size, 4, sa.ctypes.data, lcp.ctypes.data,
                                        sa.size, 0, 0, None, st.ctypes.data, len(starts), names, err, len(err))
    assert rc == 0, err.value
    return SufrFile(path)


def test_bad_starts_and_empty_arrays(tmp_path):
    f = SufrFile(EXP / "3.sufr")
    for i, bad in enumerate(([1, 5], [0, 9, 5], [0, f.text_len])):
        g = _rewrite(f, tmp_path / f"bad{i}.sufr", bad)
        with pytest.raises(SufrHipError) as e:
            g.repeats(0, 1)
        assert e.value.code == -1, bad
    none = _rewrite(f, tmp_path / "none.sufr", [0], sa=np.zeros(0, dtype=np.uint32), lcp=np.zeros(0, dtype=np.uint32))
    assert none.len_suffixes == 0
    for kind in KINDS:
        rank, count, length, st = none.repeats(kind, 1)
        assert rank.size == count.size == length.size == 0 and st == dict(records=0, longest=0, longest_rank=0, max_count=0)


# ---------------------------------------------------------------------------------------------------------------------
# the shared arithmetic (sufr_repeat_scan.h) on the CPU
# ---------------------------------------------------------------------------------------------------------------------
SHIM_SRC = ROOT / "tests" / "repeat_shim.cpp"
SHIM_DEPS = (SHIM_SRC, ROOT / "sufr_amd" / "csrc" / "sufr_repeat_scan.h", ROOT / "sufr_amd" / "csrc" / "sufr_kmer_scan.h")
NONE = (1 << 64) - 1


@pytest.fixture(scope="module")
def shim():
    out = ROOT / "tests" / "_build" / "librepeat_shim.so"
    out.parent.mkdir(exist_ok=True)
    if not out.exists() or any(out.stat().st_mtime < p.stat().st_mtime for p in SHIM_DEPS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", str(out), str(SHIM_SRC)], check=True)
    L = C.CDLL(str(out))
    vp, u64 = C.c_void_p, C.c_uint64
    L.shim_rep_pyramid_size.argtypes = [u64]; L.shim_rep_pyramid_size.restype = u64
    L.shim_rep_levels.argtypes = [u64]; L.shim_rep_levels.restype = C.c_uint32
    L.shim_rep_level_size.argtypes = [u64, C.c_uint32]; L.shim_rep_level_size.restype = u64
    L.shim_rep_pyramid.argtypes = [vp, u64, vp]; L.shim_rep_pyramid.restype = None
    L.shim_rep_search_left.argtypes = [vp, vp, u64, u64, u64]; L.shim_rep_search_left.restype = u64
    L.shim_rep_search_right.argtypes = [vp, vp, u64, u64, u64]; L.shim_rep_search_right.restype = u64
    L.shim_rep_search_all.argtypes = [vp, vp, u64, vp, vp]; L.shim_rep_search_all.restype = None
    L.shim_rep_words.argtypes = [vp, u64, vp, vp]; L.shim_rep_words.restype = None
    L.shim_rep_flagged.argtypes = [vp, vp, u64, u64]; L.shim_rep_flagged.restype = u64
    L.shim_rep_left_diverse.argtypes = [vp, vp, u64, u64]; L.shim_rep_left_diverse.restype = C.c_int
    return L


def linear_left(ell, r, v):
    for j in range(r - 1, -1, -1):
        if ell[j] <= v:
            return j
    return NONE


def linear_right(ell, r, v):
    for j in range(r + 1, len(ell)):
        if ell[j] < v:
            return j
    return len(ell)


def stack_answers(ell: np.ndarray):
    """the answers of both searches for every rank with v = l[r], by two stack passes"""
    e, s = ell.tolist(), ell.size
    left, right, stack = np.full(s, NONE, dtype=np.uint64), np.full(s, s, dtype=np.uint64), []
    for r in range(s):
        while stack and e[stack[-1]] > e[r]:
            stack.pop()
        if stack:
            left[r] = stack[-1]
        stack.append(r)
    stack = []
    for r in range(s - 1, -1, -1):
        while stack and e[stack[-1]] >= e[r]:
            stack.pop()
        if stack:
            right[r] = stack[-1]
        stack.append(r)
    return left, right


def pyramid(shim, ell):
    up = np.zeros(shim.shim_rep_pyramid_size(ell.size), dtype=np.uint64)
    shim.shim_rep_pyramid(ell.ctypes.data, ell.size, up.ctypes.data)
    return up


def test_pyramid_levels(shim):
    assert [shim.shim_rep_levels(s) for s in (0, 1, 64, 65, 4096, 4097, 262144, 262145, 64 ** 3 + 1)] == [0, 0, 0, 1, 1, 2, 2, 3, 3]
    assert [shim.shim_rep_level_size(4097, k) for k in (0, 1, 2, 3)] == [4097, 65, 2, 1]
    rng = np.random.default_rng(2)
    ell = rng.integers(0, 1000, 4097).astype(np.uint64)
    up = pyramid(shim, ell)
    assert np.array_equal(up[:65], [ell[i * 64:i * 64 + 64].min() for i in range(65)])
    assert up[65:67].tolist() == [int(ell[:4096].min()), int(ell[4096])]


@pytest.mark.parametrize("s", [1, 2, 63, 64, 65, 4095, 4096, 4097, 262143, 262144, 262145])
def test_searches_equal_a_linear_scan(shim, s):
    rng = np.random.default_rng(s)
    arrays = {"random": rng.integers(0, 9, s), "plateau": np.full(s, 4), "ascending": np.arange(s), "descending": np.arange(s, 0, -1),
              # dips exactly on word and level boundaries, plateaus between them
              "boundaries": np.where(np.arange(s) % 4096 == 0, 1, np.where(np.arange(s) % 64 == 0, 2, 3)),
              "last words": np.where(np.arange(s) % 64 == 63, 1, 3)}
    for what, a in arrays.items():
        ell = np.ascontiguousarray(a, dtype=np.uint64)
        ell[0] = 0
        up = pyramid(shim, ell)
        left, right = np.zeros(s, dtype=np.uint64), np.zeros(s, dtype=np.uint64)
        shim.shim_rep_search_all(ell.ctypes.data, up.ctypes.data, s, left.ctypes.data, right.ctypes.data)
        wl, wr = stack_answers(ell)
        assert np.array_equal(left, wl) and np.array_equal(right, wr), (s, what)
        assert left[0] == NONE and (what != "plateau" or s < 2 or (left[1:] == np.arange(s - 1)).all() and (right[1:] == s).all())
        # single searches with a v of their own, held to the linear scan itself; answers at index 0 and at s
        e = ell.tolist()
        for r in sorted({0, 1, s // 2, s - 1, min(64, s - 1), min(4096, s - 1), max(s - 65, 0)}):
            for v in (0, 1, 2, 3, 10 ** 9):
                assert shim.shim_rep_search_left(ell.ctypes.data, up.ctypes.data, s, r, v) == (linear_left(e, r, v) if s <= 5000 else
                                                                                              _np_left(ell, r, v)), (s, what, r, v)
                assert shim.shim_rep_search_right(ell.ctypes.data, up.ctypes.data, s, r, v) == (linear_right(e, r, v) if s <= 5000 else
                                                                                                _np_right(ell, r, v)), (s, what, r, v)
    if s > 1:
        ell = np.full(s, 7, dtype=np.uint64)
        ell[0] = 0
        up = pyramid(shim, ell)
        assert shim.shim_rep_search_left(ell.ctypes.data, up.ctypes.data, s, s - 1, 3) == 0          # the answer at index 0
        assert shim.shim_rep_search_right(ell.ctypes.data, up.ctypes.data, s, 0, 7) == s             # ... and at s


def _np_left(ell, r, v):
    hit = np.nonzero(ell[:r] <= v)[0]
    return int(hit[-1]) if hit.size else NONE


def _np_right(ell, r, v):
    hit = np.nonzero(ell[r + 1:] < v)[0]
    return int(hit[0]) + r + 1 if hit.size else ell.size


def test_popcount_prefix_equals_a_direct_count(shim):
    rng = np.random.default_rng(4)
    for s in (1, 63, 64, 65, 128, 129, 1000):
        flags = (rng.integers(0, 3, s) == 0).astype(np.uint8)
        words, prefix = np.zeros((s + 63) // 64, dtype=np.uint64), np.zeros((s + 63) // 64, dtype=np.uint64)
        shim.shim_rep_words(flags.ctypes.data, s, words.ctypes.data, prefix.ctypes.data)
        cum = np.concatenate([[0], np.cumsum(flags)])
        edges = sorted({0, 1, 63, 64, 65, 127, 128, s - 1, s} & set(range(s + 1))) + rng.integers(0, s + 1, 20).tolist()
        for lo in edges:
            for hi in edges:
                want = int(cum[hi] - cum[lo]) if hi > lo else 0
                assert shim.shim_rep_flagged(words.ctypes.data, prefix.ctypes.data, lo, hi) == want, (s, lo, hi)
                if hi > lo:
                    assert shim.shim_rep_left_diverse(words.ctypes.data, prefix.ctypes.data, lo, hi) == int(cum[hi] - cum[lo + 1] > 0 if hi > lo + 1 else 0)


def test_room_and_sequence_start_at_positions_beyond_2_31_and_2_32(shim):
    """rep_room and rep_is_start with the sequence starts of tests/high_positions.py, which lie beyond 2^31 and on both sides
    of 2^32, against a bisection in Python integers: at and next to every start, the boundary and both ends of the text"""
    import bisect
    from high_positions import REPEAT_GEOMETRIES
    vp, u64 = C.c_void_p, C.c_uint64
    shim.shim_rep_room.argtypes = [vp, u64, u64, u64]; shim.shim_rep_room.restype = u64
    shim.shim_rep_is_start.argtypes = [vp, u64, u64, u64]; shim.shim_rep_is_start.restype = C.c_int
    for geo in REPEAT_GEOMETRIES.values():
        starts = geo.seq_starts
        st = np.array(starts, dtype=np.uint64)
        for p in sorted({x + d for x in starts[1:] + [geo.filler, geo.boundary, geo.n - 2] for d in (-2, -1, 0, 1)} | {0, 1}):
            i = bisect.bisect_right(starts, p)
            room = (starts[i] - 1 if i < len(starts) else geo.n - 1) - p
            assert shim.shim_rep_room(st.ctypes.data, st.size, geo.n, p) == room, (geo.name, p)
            assert shim.shim_rep_is_start(st.ctypes.data, st.size, geo.n, p) == int(p in starts), (geo.name, p)
    top = REPEAT_GEOMETRIES["u64_across_2_32"].seq_starts
    assert top[2] < 1 << 32 < top[3]


def test_shared_arithmetic_under_the_sanitizers(tmp_path):
    """the same shim as a stand-alone program with AddressSanitizer and UBSan: host code, run as it is"""
    exe = tmp_path / "repeat_shim_main"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DREPEAT_SHIM_MAIN", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", str(exe), str(SHIM_SRC)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and re.fullmatch(r"ok \d+\n", r.stdout), r.stdout[-2000:] + r.stderr[-3000:]
    assert int(r.stdout.split()[1]) > 1_000_000


# ---------------------------------------------------------------------------------------------------------------------
# sufr repeats
# ---------------------------------------------------------------------------------------------------------------------
def repeats_text(f: SufrFile, recs, stats, max_positions=16):
    sa = np.asarray(f.suffix_array).astype(np.int64)
    starts = np.array(f.sequence_starts, dtype=np.int64)
    lines = []
    for a, c, ln in zip(*recs):
        pos = sorted(sa[int(a):int(a) + int(c)].tolist())
        shown = pos[:max_positions] if max_positions else pos
        where = []
        for p in shown:
            i = int(np.searchsorted(starts, p, side="right")) - 1
            where.append(f"{f.sequence_names[i]}:{p - int(starts[i])}")
        lines.append(f"{int(ln)}\t{int(c)}\t" + " ".join(where))
    lines += [f"# {key}\t{stats[key]}" for key in ("records", "longest", "longest_rank", "max_count")]
    return "\n".join(lines) + "\n"


def test_cli_repeats_prints_the_witness_records(tmp_path):
    f = SufrFile(EXP / "3.sufr")
    for kind, name in ((0, "branching"), (1, "maximal"), (2, "super")):
        w = witness_serial(f, kind, 2)
        assert filtered(witness_dictionary(f)[kind], 2, 2, 0) == {(int(ln), frozenset(np.asarray(f.suffix_array)[int(a):int(a) + int(c)].tolist()))
                                                                  for a, c, ln in zip(*w[:3])}
        assert run("repeats", "-l", 2, "--kind", name, EXP / "3.sufr").stdout == repeats_text(f, w[:3], w[3])
    w = witness_serial(f, 0, 1, 3, 9)
    assert w[3]["records"] > 0
    out = tmp_path / "r.tsv"
    assert run("rp", "-l", 1, "-c", 3, "-C", 9, "--max-positions", 2, "-o", out, EXP / "3.sufr").stdout == ""
    assert out.read_text() == repeats_text(f, w[:3], w[3], 2)
    r = run("repeats", "-l", 3, EXP / "uniprot-masked.sufr", check=False)
    assert r.returncode == 1 and r.stderr.startswith("Error: ") and "seed mask" in r.stderr
    assert run("repeats", EXP / "3.sufr", check=False).returncode == 2           # no -l
    assert run("repeats", "-l", 3, "--kind", "tandem", EXP / "3.sufr", check=False).returncode == 2
    assert "repeats|rp" in run("--help").stdout


def test_cli_repeats_without_records_and_refused(tmp_path):
    assert run("repeats", "-l", 100000, EXP / "uniprot.sufr").stdout == "# records\t0\n# longest\t0\n# longest_rank\t0\n# max_count\t0\n"
    out = tmp_path / "r.tsv"                                                     # the output is opened after the call: none after a refusal
    r = run("repeats", "-l", 3, "-o", out, EXP / "uniprot-masked.sufr", check=False)
    assert r.returncode == 1 and r.stderr.startswith("Error: ") and not out.exists()
