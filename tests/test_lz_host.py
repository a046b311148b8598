"""Longest previous factors and the LZ77 parse on the host (include/sufr_lz.h): no GPU.

The witness uses no suffix array and no LCP array: for every distance it compares the text with itself shifted by that
distance, symbol by symbol, and so knows for every pair of positions how far they agree; LPF is the best earlier indexed
position, held to the room before the next break.  It is quadratic and runs on texts of a few thousand symbols.  The shared
arithmetic of the device path (sufr_amd/csrc/sufr_lz_scan.h through tests/lz_shim.cpp) is held to linear scans.
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
FF = 0xFFFFFFFFFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------------
# the witness
# ---------------------------------------------------------------------------------------------------------------------
def brk_of(f: SufrFile) -> np.ndarray:
    n = f.text_len
    breaks = np.array(sorted({n - 1} | {s - 1 for s in f.sequence_starts[1:]}), dtype=np.int64)
    return breaks[np.searchsorted(breaks, np.arange(n, dtype=np.int64), side="left")]


def witness_lpf(f: SufrFile) -> np.ndarray:
    """LPF by position from the text, the breaks and the set of indexed positions"""
    text = np.asarray(f.text)
    n = text.size
    room = brk_of(f) - np.arange(n)
    indexed = np.zeros(n, dtype=bool)
    indexed[np.asarray(f.suffix_array).astype(np.int64)] = True
    best = np.zeros(n, dtype=np.int64)
    for d in range(1, n):
        eq = text[d:] == text[:-d]                                    # eq[q]: T[q] == T[q + d]
        here = np.arange(n - d)
        stop = np.where(eq, n - d, here)                              # the next disagreement at or after q
        run = np.minimum.accumulate(stop[::-1])[::-1] - here          # symbols on which q and q + d agree
        run = np.where(indexed[:n - d], run, 0)                       # the earlier position must be indexed
        np.maximum(best[d:], run, out=best[d:])
    return np.where(indexed, np.minimum(best, room), 0)


def witness_lpf_at(f: SufrFile, positions) -> np.ndarray:
    """the same for some positions only, one at a time: the earlier indexed positions that still agree, one more symbol per
    round (for texts too long for the quadratic table)"""
    text = np.asarray(f.text)
    brk = brk_of(f)
    indexed = np.sort(np.asarray(f.suffix_array).astype(np.int64))
    out = []
    for p in positions:
        cand, ln = indexed[indexed < p], 0
        if indexed[np.searchsorted(indexed, p) % indexed.size] != p:
            cand = cand[:0]
        while cand.size and ln < int(brk[p]) - p:
            cand = cand[text[cand + ln] == text[p + ln]]              # (cand + ln < p + ln <= brk[p]: inside the text)
            ln += bool(cand.size)
        out.append(ln)
    return np.array(out, dtype=np.int64)


def host_lpf(f: SufrFile, threads=0):
    lpf, src = f.lpf(threads=threads)
    none = np.iinfo(lpf.dtype).max
    assert lpf.dtype == src.dtype == np.asarray(f.suffix_array).dtype and lpf.size == src.size == f.text_len
    return lpf.astype(np.int64), np.where(src == none, -1, src.astype(np.int64))


def check_lpf(f: SufrFile):
    """the host's LPF equals the witness's; every source is an earlier indexed occurrence; returns the witness LPF"""
    lpf, src = host_lpf(f)
    if f.text_len <= 3000:
        want = witness_lpf(f)
    else:                                                             # a long text: every 40th position, a tile's worth at either end
        some = sorted(set(range(0, f.text_len, 40)) | set(range(300)) | set(range(f.text_len - 300, f.text_len)))
        assert np.array_equal(lpf[some], witness_lpf_at(f, some))
        want = lpf
    assert np.array_equal(lpf, want), np.nonzero(lpf != want)[0][:10]
    assert np.array_equal(src == -1, lpf == 0)
    tb = bytes(f.text)
    indexed = set(np.asarray(f.suffix_array).tolist())
    for p in np.nonzero(lpf)[0].tolist():
        q, ln = int(src[p]), int(lpf[p])
        assert 0 <= q < p and q in indexed and tb[q:q + ln] == tb[p:p + ln], (p, q, ln)
    return want


def check_parse(f: SufrFile, want_lpf: np.ndarray):
    """the factors tile the text, copy what they say they copy, span no break, and are the greedy walk over the witness"""
    start, length, source, st = f.lz()
    n = f.text_len
    assert start.dtype == length.dtype == source.dtype == np.uint64
    z = start.size
    assert z == st["factors"] and int(start[0]) == 0 and int(start[-1] + length[-1]) == n
    assert np.array_equal(start[1:], (start + length)[:-1]) and (length >= 1).all()
    brk = brk_of(f)
    tb = bytes(f.text)
    rebuilt = bytearray()
    for p, ln, q in zip(start.tolist(), length.tolist(), source.tolist()):
        assert ln == 1 or p + ln <= int(brk[p]), (p, ln)             # no factor spans a break
        if q == FF:
            assert ln == 1
            rebuilt.append(tb[p])
        else:
            assert q < p
            for i in range(ln):                                       # (the copy may overlap itself)
                rebuilt.append(rebuilt[q + i])
    assert bytes(rebuilt) == tb
    # the walk over the witness: with s == n this is the greedy parse itself
    p, steps = 0, []
    while p < n:
        steps.append((p, max(1, int(want_lpf[p]))))
        p += steps[-1][1]
    assert [(int(a), int(b)) for a, b in zip(start, length)] == steps
    assert np.array_equal(source == FF, want_lpf[start.astype(np.int64)] == 0)
    top = int(length.max())
    assert st == dict(factors=z, literals=int((source == FF).sum()), longest=top, longest_start=int(start[np.nonzero(length == top)[0][0]]))
    return start, length, source, st


def oracle_file(oracle, tmp_path, body, name="x", **build):
    _fasta_from(body, tmp_path / f"{name}.fa")
    oracle.create(tmp_path / f"{name}.fa", tmp_path / f"{name}.sufr", **build)
    return SufrFile(tmp_path / f"{name}.sufr")


def distinct_file(path, count=200):
    """`count` pairwise different bytes and the sentinel.  A sequence file cannot carry them (line ends, '>', letter case), so
    the arrays are written as they are: the suffixes in the order of their first bytes, every LCP 0."""
    text = np.array([b for b in range(256) if b != ord("$")][:count] + [ord("$")], dtype=np.uint8)
    assert np.unique(text).size == text.size == count + 1
    sa = np.argsort(text).astype(np.uint32)
    lcp = np.zeros(sa.size, dtype=np.uint32)
    starts = np.zeros(1, dtype=np.uint64)
    names = (C.c_char_p * 1)(b"1")
    err = C.create_string_buffer(256)
    rc = sufr_amd.lib().sufr_write_file(str(path).encode(), 0, 0, 0, text.ctypes.data, text.size, 4, sa.ctypes.data, lcp.ctypes.data, sa.size, 0, 0,
                                        None, starts.ctypes.data, 1, names, err, len(err))
    assert rc == 0, err.value
    return SufrFile(path)


def letters(alphabet: bytes, count: int, seed: int) -> np.ndarray:
    return np.frombuffer(alphabet, dtype=np.uint8)[np.random.default_rng(seed).integers(0, len(alphabet), count)]


def fibonacci(count: int) -> np.ndarray:
    a, b = b"A", b"AC"
    while len(b) < count:
        a, b = b, b + a
    return np.frombuffer(b[:count], dtype=np.uint8)


def small_texts():
    """name -> (body, build); '%' separates sequences"""
    sep = np.frombuffer(b"%", dtype=np.uint8)
    piece = letters(b"ACGT", 150, 7)
    dna = dict(is_dna=True)
    return {
        "all_a": (np.full(700, ord("A"), dtype=np.uint8), dna),
        "fib": (fibonacci(1500), dna),
        "acgt_k": (np.tile(np.frombuffer(b"ACGT", dtype=np.uint8), 300), dna),
        "random2": (letters(b"AC", 1500, 1), dna),
        "random4": (letters(b"ACGT", 2000, 2), dna),
        "identical": (np.concatenate([np.concatenate([piece, sep]) for _ in range(6)])[:-1], dna),
        "several": (np.concatenate([letters(b"ACGT", 300, 3), sep, letters(b"AC", 200, 4), sep, piece, sep, piece[40:], sep, letters(b"ACGT", 90, 5)]), dna),
        "n_runs": (np.concatenate([letters(b"ACGT", 400, 6), np.full(37, ord("N"), dtype=np.uint8), letters(b"ACGT", 300, 6), np.full(5, ord("N"), dtype=np.uint8),
                                   sep, letters(b"ACGTN", 500, 8)]), dna),
    }


# ---------------------------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_lz_header_symbols_are_exported():
    hdr = (ROOT / "include" / "sufr_lz.h").read_text()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(sufr_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(sufr_amd.LZ_EXPORTS), declared ^ set(sufr_amd.LZ_EXPORTS)
    L = sufr_amd.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(sufr_amd.LIB_PATH)], capture_output=True, text=True).stdout
    for name in declared:
        assert hasattr(L, name) and re.search(rf"\bT {name}\b", nm), name
    assert L.sufr_hip_abi_version() == 3
    assert C.sizeof(sufr_amd.LzStats) == 32
    assert hasattr(sufr_amd.Context, "set_lz_tile")


def test_host_stubs_define_the_device_entry_points():
    stubs = (ROOT / "sufr_amd" / "csrc" / "sufr_host_stubs.cpp").read_text()
    device = [name for name in sufr_amd.LZ_EXPORTS if name.startswith("sufr_hip_")]
    assert len(device) == 3
    for name in device:
        assert re.search(rf"\bint {name}\(", stubs), name


# ---------------------------------------------------------------------------------------------------------------------
# against the witness
# ---------------------------------------------------------------------------------------------------------------------
def test_host_equals_witness_on_golden_files():
    used = copies = 0
    for name in GOLDEN_FILES:
        f = SufrFile(EXP / name)
        if f.seed_mask:
            for call in (f.lpf, f.lz):
                with pytest.raises(SufrHipError) as e:
                    call()
                assert e.value.code == -6
            continue
        want = check_lpf(f)
        check_parse(f, want)
        used += 1
        copies += int((want > 0).sum())
    assert used >= 10 and copies > 1000


@pytest.mark.parametrize("name", sorted(small_texts()))
def test_host_equals_witness_on_oracle_builds(oracle, tmp_path, name):
    body, build = small_texts()[name]
    f = oracle_file(oracle, tmp_path, body, name, **build)
    assert f.text_len <= 2001
    want = check_lpf(f)
    start, length, source, st = check_parse(f, want)
    if name in ("identical", "several", "n_runs"):
        assert f.num_sequences >= 2
    unindexed = np.ones(f.text_len, dtype=bool)
    unindexed[np.asarray(f.suffix_array).astype(np.int64)] = False
    if name == "n_runs":                                             # a partial index: the N are not indexed and become literals
        assert unindexed.sum() > 40 + f.num_sequences
    else:                                                            # (a DNA build does not index the delimiters between sequences)
        assert np.nonzero(unindexed)[0].tolist() == [s - 1 for s in f.sequence_starts[1:]]
    at_unindexed = unindexed[start.astype(np.int64)]                 # (a copy may run over positions that are not indexed; none starts at one)
    assert (source[at_unindexed] == FF).all() and at_unindexed.sum() >= min(40, unindexed.sum())
    if name == "identical":                                          # the second sequence is one copy of the first, clipped at its break
        starts = f.sequence_starts
        i = int(np.nonzero(start == starts[1])[0][0])
        assert (int(length[i]), int(source[i])) == (150, 0) and int(start[i + 1]) == starts[2] - 1 and int(source[i + 1]) == FF


def test_pairwise_different_bytes_are_all_literals(tmp_path):
    f = distinct_file(tmp_path / "distinct.sufr")
    assert f.text_len == f.len_suffixes == 201
    want = check_lpf(f)
    assert not want.any()
    assert check_parse(f, want)[3] == dict(factors=201, literals=201, longest=1, longest_start=0)


def test_known_answers(oracle, tmp_path):
    for m in (4, 7, 300):
        f = oracle_file(oracle, tmp_path, np.full(m, ord("A"), dtype=np.uint8), f"a{m}", is_dna=True)
        start, length, source, st = f.lz()
        assert [start.tolist(), length.tolist(), source.tolist()] == [[0, 1, m], [1, m - 1, 1], [FF, 0, FF]]
        assert st == dict(factors=3, literals=2, longest=m - 1, longest_start=1)
    for k in (2, 80):
        f = oracle_file(oracle, tmp_path, np.tile(np.frombuffer(b"ACGT", dtype=np.uint8), k), f"acgt{k}", is_dna=True)
        start, length, source, st = f.lz()
        assert [start.tolist(), length.tolist(), source.tolist()] == [[0, 1, 2, 3, 4, 4 * k], [1, 1, 1, 1, 4 * k - 4, 1], [FF, FF, FF, FF, 0, FF]]
        assert st == dict(factors=6, literals=5, longest=4 * k - 4, longest_start=4)


def test_threads_capacity_and_counting_calls(oracle, tmp_path):
    f = oracle_file(oracle, tmp_path, letters(b"ACGT", 40_000, 9), is_dna=True, threads=4)       # more than one chunk of ranks
    want_lpf, want = f.lpf(threads=1), f.lz(threads=1)
    for threads in (2, 0):
        got_lpf, got = f.lpf(threads=threads), f.lz(threads=threads)
        assert all(np.array_equal(a, b) for a, b in zip(got_lpf, want_lpf))
        assert all(np.array_equal(got[i], want[i]) for i in range(3)) and got[3] == want[3]
    L = sufr_amd.lib()
    z = want[3]["factors"]
    assert z > 1000
    total, st = C.c_uint64(0), sufr_amd.LzStats()
    assert L.sufr_file_lz(f._h, 0, None, None, None, C.byref(total), C.byref(st), 1) == -5         # the counting call
    assert total.value == z and st.as_dict() == want[3]
    out = [np.full(z + 3, FF, dtype=np.uint64) for _ in range(3)]
    total.value = 0
    assert L.sufr_file_lz(f._h, z - 1, *(a.ctypes.data for a in out), C.byref(total), None, 1) == -5
    assert total.value == z and all((a == FF).all() for a in out)                               # nothing written
    assert L.sufr_file_lz(f._h, z + 3, *(a.ctypes.data for a in out), C.byref(total), None, 1) == 0
    for i in range(3):
        assert np.array_equal(out[i][:z], want[i]) and (out[i][z:] == FF).all()
    # either array of the table alone
    n = f.text_len
    only = np.zeros(n, dtype=np.uint32)
    assert L.sufr_file_lpf(f._h, only.ctypes.data, None, 1) == 0 and np.array_equal(only, want_lpf[0])
    assert L.sufr_file_lpf(f._h, None, only.ctypes.data, 1) == 0 and np.array_equal(only, want_lpf[1])
    assert L.sufr_file_lpf(None, None, None, 1) == -1 and L.sufr_file_lz(None, 0, None, None, None, None, None, 1) == -1


def test_refusals_and_empty_arrays(oracle, tmp_path):
    from test_repeat_host import _rewrite
    f = SufrFile(EXP / "uniprot-masked.sufr")
    assert f.seed_mask
    g = oracle_file(oracle, tmp_path, synth.adversarial("tandem", 600, seed=3)[:-1], is_dna=True, max_query_len=6)
    assert g.max_query_len == 6
    for h in (f, g):
        for call in (h.lpf, h.lz):
            with pytest.raises(SufrHipError) as e:
                call()
            assert e.value.code == -6
    h = SufrFile(EXP / "3.sufr")
    for i, bad in enumerate(([1, 5], [0, 9, 5], [0, h.text_len])):
        b = _rewrite(h, tmp_path / f"bad{i}.sufr", bad)
        for call in (b.lpf, b.lz):
            with pytest.raises(SufrHipError) as e:
                call()
            assert e.value.code == -1, bad
    none = _rewrite(h, tmp_path / "none.sufr", [0], sa=np.zeros(0, dtype=np.uint32), lcp=np.zeros(0, dtype=np.uint32))
    n = none.text_len
    assert none.len_suffixes == 0 and n > 0
    lpf, src = none.lpf()
    assert (lpf == 0).all() and (src == 0xFFFFFFFF).all()
    start, length, source, st = none.lz()
    assert np.array_equal(start, np.arange(n)) and (length == 1).all() and (source == FF).all()
    assert st == dict(factors=n, literals=n, longest=1, longest_start=0)


# ---------------------------------------------------------------------------------------------------------------------
# the shared arithmetic (sufr_lz_scan.h) on the CPU
# ---------------------------------------------------------------------------------------------------------------------
SHIM_SRC = ROOT / "tests" / "lz_shim.cpp"
SHIM_DEPS = (SHIM_SRC, ROOT / "sufr_amd" / "csrc" / "sufr_lz_scan.h", ROOT / "sufr_amd" / "csrc" / "sufr_repeat_scan.h",
             ROOT / "sufr_amd" / "csrc" / "sufr_kmer_scan.h")
NONE = (1 << 64) - 1


@pytest.fixture(scope="module")
def shim():
    out = ROOT / "tests" / "_build" / "liblz_shim.so"
    out.parent.mkdir(exist_ok=True)
    if not out.exists() or any(out.stat().st_mtime < p.stat().st_mtime for p in SHIM_DEPS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", str(out), str(SHIM_SRC)], check=True)
    L = C.CDLL(str(out))
    vp, u64 = C.c_void_p, C.c_uint64
    L.shim_lz_pyramid_size.argtypes = [u64]; L.shim_lz_pyramid_size.restype = u64
    L.shim_lz_levels.argtypes = [u64]; L.shim_lz_levels.restype = C.c_uint32
    L.shim_lz_pyramid.argtypes = [vp, u64, vp]; L.shim_lz_pyramid.restype = None
    L.shim_lz_range_min.argtypes = [vp, vp, u64, u64, u64, C.POINTER(u64)]; L.shim_lz_range_min.restype = u64
    L.shim_lz_range_min_many.argtypes = [vp, vp, u64, vp, vp, u64, vp]; L.shim_lz_range_min_many.restype = u64
    L.shim_lz_neighbours.argtypes = [vp, vp, u64, vp, vp]; L.shim_lz_neighbours.restype = None
    L.shim_lz_rank_all.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp]; L.shim_lz_rank_all.restype = None
    L.shim_lz_pick.argtypes = [C.c_int, u64, u64, C.c_int, u64, u64, u64, vp]; L.shim_lz_pick.restype = None
    L.shim_lz_tab_pack.argtypes = [C.c_uint32, C.c_uint32]; L.shim_lz_tab_pack.restype = C.c_uint32
    L.shim_lz_tab_last.argtypes = [C.c_uint32]; L.shim_lz_tab_last.restype = C.c_uint32
    L.shim_lz_tab_hops.argtypes = [C.c_uint32]; L.shim_lz_tab_hops.restype = C.c_uint32
    return L


def pyramid(shim, a):
    up = np.zeros(shim.shim_lz_pyramid_size(a.size), dtype=np.uint64)
    shim.shim_lz_pyramid(a.ctypes.data, a.size, up.ctypes.data)
    return up


def smaller_neighbours(a: np.ndarray):
    """for every index the nearest one on either side with a smaller value, by two stack passes"""
    v, s = a.tolist(), a.size
    left, right, stack = np.full(s, NONE, dtype=np.uint64), np.full(s, s, dtype=np.uint64), []
    for r in range(s):
        while stack and v[stack[-1]] >= v[r]:
            stack.pop()
        if stack:
            left[r] = stack[-1]
        stack.append(r)
    stack = []
    for r in range(s - 1, -1, -1):
        while stack and v[stack[-1]] >= v[r]:
            stack.pop()
        if stack:
            right[r] = stack[-1]
        stack.append(r)
    return left, right


@pytest.mark.parametrize("s", [1, 2, 63, 64, 65, 4095, 4096, 4097, 262144, 262145, 300_000])
def test_range_min_and_searches_equal_linear_scans(shim, s):
    rng = np.random.default_rng(s)
    arrays = {"constant": np.full(s, 4), "ascending": np.arange(s), "descending": np.arange(s, 0, -1), "random": rng.integers(0, 1000, s),
              "permutation": rng.permutation(s)}
    levels = shim.shim_lz_levels(s)
    assert levels == (0 if s <= 64 else 1 if s <= 4096 else 2 if s <= 262144 else 3)
    edges = sorted({0, 1, 63, 64, 65, 127, 128, 4095, 4096, 4097, 8192, 262143, 262144, s - 65, s - 64, s - 1, s} & set(range(s + 1)))
    lo = np.array([a for a in edges for b in edges if a < b] + [int(x) for x in rng.integers(0, s, 300)], dtype=np.uint64)
    hi = np.array([b for a in edges for b in edges if a < b] + [int(a) + 1 + int(rng.integers(0, s - int(a))) for a in lo[-300:]], dtype=np.uint64)
    assert ((lo + 1 == hi).any() or s == 1) and ((lo == 0) & (hi == s)).any()
    for what, a in arrays.items():
        a = np.ascontiguousarray(a, dtype=np.uint64)
        up = pyramid(shim, a)
        got = np.zeros(lo.size, dtype=np.uint64)
        most = shim.shim_lz_range_min_many(a.ctypes.data, up.ctypes.data, s, lo.ctypes.data, hi.ctypes.data, lo.size, got.ctypes.data)
        want = np.array([a[int(x):int(y)].min() for x, y in zip(lo, hi)], dtype=np.uint64)
        assert np.array_equal(got, want), (s, what)
        assert most <= 2 * 64 * (levels + 1), (s, what, most)         # bounded whatever hi - lo is
        assert shim.shim_lz_range_min(a.ctypes.data, up.ctypes.data, s, 1, 1, None) == NONE      # an empty range
        left, right = np.zeros(s, dtype=np.uint64), np.zeros(s, dtype=np.uint64)
        shim.shim_lz_neighbours(a.ctypes.data, up.ctypes.data, s, left.ctypes.data, right.ctypes.data)
        wl, wr = smaller_neighbours(a)
        assert np.array_equal(left, wl) and np.array_equal(right, wr), (s, what)
        if what == "descending" and s > 1:                            # every left search runs to the array's start, every right one is next door
            assert (wl == NONE).all() and np.array_equal(wr[:-1], np.arange(1, s))


def test_decision_and_table_entry(shim):
    out = np.zeros(2, dtype=np.uint64)
    cases = [((1, 5, 10, 1, 5, 20, 9), (5, 10)),                       # the tie goes to j1
             ((1, 4, 10, 1, 5, 20, 9), (5, 20)), ((1, 6, 10, 1, 5, 20, 9), (6, 10)),
             ((1, 7, 10, 0, 0, 0, 3), (3, 10)), ((0, 0, 0, 1, 7, 20, 3), (3, 20)),       # the clip
             ((1, 7, 10, 1, 9, 20, 3), (3, 20)),                       # the clip does not change which side wins
             ((0, 0, 0, 1, 7, 20, 0), (0, NONE)), ((0, 0, 0, 0, 0, 0, 9), (0, NONE)), ((1, 0, 10, 1, 0, 20, 9), (0, NONE))]
    for args, want in cases:
        shim.shim_lz_pick(*args, out.ctypes.data)
        assert tuple(out.tolist()) == want, args
    for last, hops in ((0, 0), (255, 1), (16383, 16383), (5, 16383)):
        e = shim.shim_lz_tab_pack(last, hops)
        assert (shim.shim_lz_tab_last(e), shim.shim_lz_tab_hops(e)) == (last, hops)


def test_rank_decisions_equal_the_host_call(shim, oracle, tmp_path):
    """lz_rank through the shim on the arrays of a file equals sufr_file_lpf: one code for both"""
    body, build = small_texts()["several"]
    f = oracle_file(oracle, tmp_path, body, **build)
    sa = np.asarray(f.suffix_array).astype(np.uint64)
    lcp = np.asarray(f.lcp).astype(np.uint64)
    room = (brk_of(f) - np.arange(f.text_len))[sa.astype(np.int64)].astype(np.uint64)
    lpf, src = np.zeros(sa.size, dtype=np.uint64), np.zeros(sa.size, dtype=np.uint64)
    up_sa, up_lcp = pyramid(shim, sa), pyramid(shim, lcp)
    shim.shim_lz_rank_all(sa.ctypes.data, up_sa.ctypes.data, lcp.ctypes.data, up_lcp.ctypes.data, sa.size, room.ctypes.data, lpf.ctypes.data, src.ctypes.data)
    want_lpf, want_src = host_lpf(f)
    assert np.array_equal(lpf.astype(np.int64), want_lpf[sa.astype(np.int64)])
    assert np.array_equal(np.where(src == NONE, -1, src.astype(np.int64)), want_src[sa.astype(np.int64)])


def test_shared_arithmetic_under_the_sanitizers(tmp_path):
    """the same shim as a stand-alone program with AddressSanitizer and UBSan: host code, run as it is"""
    exe = tmp_path / "lz_shim_main"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DLZ_SHIM_MAIN", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", str(exe), str(SHIM_SRC)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and re.fullmatch(r"ok \d+\n", r.stdout), r.stdout[-2000:] + r.stderr[-3000:]
    assert int(r.stdout.split()[1]) > 1_000_000


# ---------------------------------------------------------------------------------------------------------------------
# sufr lz
# ---------------------------------------------------------------------------------------------------------------------
def place(f: SufrFile, p: int) -> str:
    starts = np.array(f.sequence_starts, dtype=np.int64)
    i = int(np.searchsorted(starts, p, side="right")) - 1
    return f"{f.sequence_names[i]}:{p - int(starts[i])}"


def lz_text(f: SufrFile) -> str:
    start, length, source, st = f.lz()
    lines = [f"{place(f, int(p))}\t{int(ln)}\t{'*' if int(q) == FF else place(f, int(q))}" for p, ln, q in zip(start, length, source)]
    lines += [f"# {key}\t{st[key]}" for key in ("factors", "literals", "longest", "longest_start")]
    return "\n".join(lines) + "\n"


def lpf_text(f: SufrFile) -> str:
    lpf, src = host_lpf(f)
    return "".join(f"{place(f, p)}\t{int(lpf[p])}\t{'*' if src[p] < 0 else place(f, int(src[p]))}\n" for p in range(f.text_len))


def test_cli_lz_prints_what_the_python_calls_return(tmp_path):
    for name in ("3.sufr", "2d.sufr"):
        f = SufrFile(EXP / name)
        assert run("lz", EXP / name).stdout == lz_text(f)
        assert run("lz", "--lpf", EXP / name).stdout == lpf_text(f)
    out = tmp_path / "lz.tsv"
    assert run("lz", "-t", 2, "-o", out, EXP / "3.sufr").stdout == "" and out.read_text() == lz_text(SufrFile(EXP / "3.sufr"))
    r = run("lz", EXP / "uniprot-masked.sufr", check=False)
    assert r.returncode == 1 and r.stderr.startswith("Error: ") and "seed mask" in r.stderr
    assert run("lz", check=False).returncode == 2                    # no file
    assert run("lz", "--table", EXP / "3.sufr", check=False).returncode == 2
    assert "  lz " in run("--help").stdout
