"""Matching statistics and SMEMs on a pair of FM-indexes, on the host (include/sufr_fm_match.h, sufr_query.cpp): the index of the
text and the index of the reversed text against a brute-force witness in Python (substring tests on the text without its end
byte), against the backward search of the witness of tests/test_fm_host.py for the ranges, and against SufrFile.matching_statistics
/ SufrFile.smems of the same library on text and suffix array.  Every comparison is exact equality.  The query sets, the planted
texts and the witness are used by tests/test_fm_match_gpu.py too."""
import ctypes as C
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sufr_amd
from sufr_amd import FmIndex, SufrFile, SufrHipError, pack_queries
from oracle_helper import GOLDEN
from test_bwt_host import LF_FILES, write_arrays
from test_fm_host import Witness, sorted_sa
from test_lz_host import fibonacci, oracle_file
from test_match_host import run

ROOT = Path(__file__).resolve().parent.parent
EXP = GOLDEN / "expected"
INVALID, CAPACITY, NO_DEVICE = -1, -5, -2
SLAB_ENV = "SUFR_FM_MS_HOST_SLAB"


# ---------------------------------------------------------------------------------------------------------------------
# the witness
# ---------------------------------------------------------------------------------------------------------------------
def brute_ms(X: bytes, q: bytes) -> np.ndarray:
    """ms[j] = the largest l with q[j:j + l] in X, by substring tests alone.  ms[j] >= ms[j - 1] - 1, and whether q[j:j + l] occurs
    falls with l, so every offset is a doubling and a bisection above that bound."""
    m = len(q)
    ms = np.zeros(m, dtype=np.int64)
    prev = 0
    for j in range(m):
        lo, top = max(prev - 1, 0), m - j                             # q[j:j + lo] occurs
        step = 1
        hi = lo
        while hi < top and q[j:j + min(hi + step, top)] in X:
            hi = min(hi + step, top)
            step *= 2
        lo, hi = hi, min(hi + step, top)                              # occurs at lo; not at hi, unless hi == lo
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if q[j:j + mid] in X:
                lo = mid
            else:
                hi = mid - 1
        ms[j] = prev = lo
    return ms


def smems_of(ms: np.ndarray, min_len: int):
    return [(j, int(ms[j])) for j in range(len(ms)) if ms[j] >= min_len and (j == 0 or ms[j - 1] <= ms[j])]


def walk(X: bytes, q: bytes):
    """the walk of the header in Python with substring tests for its steps: (ms, the steps it takes)"""
    m = len(q)
    ms = np.zeros(m, dtype=np.int64)
    steps, x = 0, m - 1
    while x >= 0:
        l = 0
        while x + l < m and q[x:x + l + 1] in X:
            l += 1
        steps += l + (1 if x + l < m else 0)
        if l == 0:
            x -= 1
            continue
        end, b = x + l, 0
        while end - b > 0 and q[end - b - 1:end] in X:
            b += 1
        steps += b + (1 if end - b > 0 else 0)
        start = end - b
        assert start <= x
        ms[start:x + 1] = end - np.arange(start, x + 1)
        x = start - 1
    return ms, steps


class Pair:
    """a text T, its reversal R = reverse(T[:-1]) + e, their files and the witness of T"""

    def __init__(self, fwd_file: SufrFile, rev_file: SufrFile):
        self.f, self.g = fwd_file, rev_file
        self.text = np.asarray(fwd_file.text).copy()
        self.raw = self.text.tobytes()
        self.X = self.raw[:-1]
        self.e = self.raw[-1]
        self.w = Witness(self.text, np.asarray(fwd_file.suffix_array))
        self._ms, self._range = {}, {}
        assert np.array_equal(np.asarray(rev_file.text), reversal(self.text))

    def ms(self, q: bytes) -> np.ndarray:
        if q not in self._ms:
            self._ms[q] = brute_ms(self.X, q)
        return self._ms[q]

    def range_of(self, piece: bytes):
        if piece not in self._range:
            self._range[piece] = self.w.search(piece)[:2]
        return self._range[piece]

    def want(self, queries, min_len):
        """(the ms of every query, the five SMEM columns) from the witness"""
        ms = [self.ms(q) for q in queries]
        rows = []
        for i, q in enumerate(queries):
            for j, l in smems_of(ms[i], min_len):
                lo, hi = self.range_of(q[j:j + l])
                assert hi > lo
                rows.append((i, j, l, lo, hi))
        cols = [np.array([r[k] for r in rows], dtype=d) for k, d in enumerate((np.uint64, np.uint32, np.uint32, np.uint64, np.uint64))]
        return ms, cols


def reversal(text: np.ndarray) -> np.ndarray:
    return np.concatenate([text[:-1][::-1], text[-1:]])


def planted_pair(tmp_path, text: np.ndarray, name: str) -> Pair:
    """the files of a text and of its reversal from their arrays as they are"""
    text = np.ascontiguousarray(text, dtype=np.uint8)
    rev = reversal(text)
    return Pair(write_arrays(tmp_path / f"{name}.sufr", text, sorted_sa(text)), write_arrays(tmp_path / f"{name}_rev.sufr", rev, sorted_sa(rev)))


_PAIRS = {}


def golden_pair(name: str, oracle, tmp_path_factory) -> Pair:
    """a golden file and the oracle's .sufr of its reversed FASTA, built with its flags; once per run"""
    if name not in _PAIRS:
        d = tmp_path_factory.mktemp("pair")
        f = SufrFile(EXP / name)
        f.write_reversed_fasta(d / "rev.fa")
        oracle.create(d / "rev.fa", d / "rev.sufr", is_dna=f.is_dna, allow_ambiguity=f.allow_ambiguity, ignore_softmask=f.ignore_softmask)
        _PAIRS[name] = Pair(f, SufrFile(d / "rev.sufr"))
    return _PAIRS[name]


@pytest.fixture
def pairs(oracle, tmp_path_factory):
    return lambda name: golden_pair(name, oracle, tmp_path_factory)


def same_columns(got, want) -> bool:
    return len(got) == len(want) == 5 and all(g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want))


def query_set(p: Pair, seed: int = 0, count: int = 24, max_len: int = 90):
    """The empty query and one of a single byte; an absent byte; the end byte in the middle and at the end; X and T themselves;
    pieces of the text with substitutions, two and three distant pieces glued together (overlapping SMEMs), random strings over
    the text's bytes; on a file of several sequences a window across a delimiter"""
    rng = np.random.default_rng(seed)
    X, raw = p.X, p.raw
    n1 = len(X)
    absent = [c for c in range(255, -1, -1) if p.w.counts[c] == 0]
    symbols = sorted(set(X))
    qs = [b"", X[:1], X, raw, X[2:20] + raw[-1:] + X[4:19], X[3:17] + raw[-1:]]
    if absent:
        qs += [bytes([absent[0]]), X[1:30] + bytes([absent[0]]) + X[5:40]]
    for _ in range(count):
        kind = int(rng.integers(0, 4))
        L = int(rng.integers(1, max_len + 1))
        a, b, c = (int(v) for v in rng.integers(0, n1, 3))
        if kind == 0:
            q = bytearray(X[a:a + L])
            for _ in range(int(rng.integers(0, 3))):
                q[int(rng.integers(0, len(q)))] = symbols[int(rng.integers(0, len(symbols)))]
        elif kind == 1:
            q = bytearray(X[a:a + L // 2] + X[b:b + L - L // 2])
        elif kind == 2:
            q = bytearray(X[a:a + L // 3] + X[b:b + L // 3] + X[c:c + L // 3 + 1])
        else:
            q = bytearray(symbols[int(v)] for v in rng.integers(0, len(symbols), min(L, 24)))
        qs.append(bytes(q))
    starts = list(p.f.sequence_starts)
    if len(starts) > 1:
        s1 = int(starts[1])
        qs.append(raw[max(s1 - 9, 0):s1 + 8])                         # (the delimiter stands at s1 - 1)
    return qs


def conditions(p: Pair, qs, B: int):
    """what a query set does, from the witness"""
    c = set()
    for q in qs:
        ms = p.ms(q)
        if len(q) == 0:
            c.add("empty")
        if len(q) == 1:
            c.add("one_byte")
        if any(p.w.counts[b] == 0 for b in q):
            c.add("absent_byte")
        if p.e in q[:-1]:
            c.add("end_byte_inside")
        if q[-1:] == bytes([p.e]):
            c.add("end_byte_last")
        if q == p.X and ms[0] == len(p.X):
            c.add("is_X")
        if q == p.raw:
            c.add("is_T")
        sm = smems_of(ms, 1)
        depth = np.zeros(len(q) + 1, dtype=np.int64)
        for j, l in sm:
            depth[j] += 1
            depth[j + l] -= 1
        if len(q) and np.cumsum(depth).max() >= 3:
            c.add("three_cover")
        for j, l in sm:
            lo, hi = p.range_of(q[j:j + l])
            if hi - lo >= 2:
                c.add("two_ranks")
            if lo // B != (hi - 1) // B:
                c.add("two_blocks")
            if b"%" in q[j:j + l] and l >= 2:
                c.add("across_delimiter")
        if len(q) and not smems_of(ms, 20):
            c.add("none_at_20")
    return c


# ---------------------------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_match_header_symbols_are_exported():
    hdr = (ROOT / "include" / "sufr_fm_match.h").read_text()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(sufr_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(sufr_amd.FM_MATCH_EXPORTS), declared ^ set(sufr_amd.FM_MATCH_EXPORTS)
    L = sufr_amd.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(sufr_amd.LIB_PATH)], capture_output=True, text=True).stdout
    for name in declared:
        assert hasattr(L, name) and re.search(rf"\bT {name}\b", nm), name
    for cls, names in ((SufrFile, ("write_reversed_fasta",)), (FmIndex, ("matching_stats", "smems", "matching_stats_steps")),
                       (sufr_amd.DeviceFmIndex, ("matching_stats_device", "smems_device", "matching_stats", "smems"))):
        for name in names:
            assert hasattr(cls, name), (cls, name)


def test_host_stubs_answer_no_device(tmp_path):
    """a C++ program linked against the stubs alone gets SUFR_HIP_E_NO_DEVICE from the three device entry points"""
    stubs = ROOT / "sufr_amd" / "csrc" / "sufr_host_stubs.cpp"
    device = [name for name in sufr_amd.FM_MATCH_EXPORTS if name.startswith("sufr_hip_")]
    assert len(device) == 3
    for name in device:
        assert re.search(rf"\bint {name}\(", stubs.read_text()), name
    main = tmp_path / "main.cpp"
    main.write_text('#include "sufr_fm_match.h"\n#include <stdio.h>\nint main() {\n  uint64_t t = 7, u = 7;\n'
                    '  int rc[3] = {sufr_hip_fm_matching_stats_device(0, 0, 0, 0, 0, 0, 0),\n'
                    '    sufr_hip_fm_smems_device(0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, &t), sufr_hip_fm_smems(0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, &u)};\n'
                    '  printf("%d %d %d %llu %llu\\n", rc[0], rc[1], rc[2], (unsigned long long)t, (unsigned long long)u);\n  return 0;\n}\n')
    exe = tmp_path / "stubs"
    subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT / 'include'}", "-o", str(exe), str(main), str(stubs)],
                   check=True, capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == [str(NO_DEVICE)] * 3 + ["0", "0"], out


def test_the_header_is_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "sufr_fm_match.h"\nint main(void) { return sufr_fm_pair_check(0, 0) == 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", f"-I{ROOT / 'include'}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---------------------------------------------------------------------------------------------------------------------
# the reversed FASTA
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LF_FILES)
def test_reversed_fasta_through_the_oracle(oracle, tmp_path, name):
    """the oracle's .sufr of write_reversed_fasta, built with the forward file's flags: the text is reverse(T[:-1]) + e, the names
    are reversed and the starts mirrored"""
    f = SufrFile(EXP / name)
    fa, out = tmp_path / "rev.fa", tmp_path / "rev.sufr"
    f.write_reversed_fasta(fa)
    oracle.create(fa, out, is_dna=f.is_dna, allow_ambiguity=f.allow_ambiguity, ignore_softmask=f.ignore_softmask)
    g = SufrFile(out)
    text = np.asarray(f.text)
    assert np.array_equal(np.asarray(g.text), reversal(text))
    assert list(g.sequence_names) == list(f.sequence_names)[::-1]
    n, starts = text.size, [int(s) for s in f.sequence_starts]
    ends = starts[1:] + [n]                                           # sequence i is T[starts[i] : ends[i] - 1]
    assert [int(s) for s in g.sequence_starts] == [n - e for e in ends][::-1]
    assert (g.is_dna, g.allow_ambiguity, g.ignore_softmask) == (f.is_dna, f.allow_ambiguity, f.ignore_softmask)
    fwd, rev = f.fm(32), g.fm(0)
    fwd.pair_check(rev)
    qs = query_set(Pair(f, g), seed=3, count=6)
    assert [m.tolist() for m in fwd.matching_stats(qs, rev)] == [brute_ms(text.tobytes()[:-1], q).tolist() for q in qs]
    with pytest.raises(SufrHipError):
        f.write_reversed_fasta(tmp_path / "no" / "such" / "dir.fa")


# ---------------------------------------------------------------------------------------------------------------------
# against the witness and against text and suffix array
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LF_FILES)
def test_pair_equals_witness_and_suffix_array_on_golden_files(name, pairs):
    p = pairs(name)
    qs = query_set(p, seed=len(name))
    no_e = [q for q in qs if p.e not in q]                            # (sufr_file_matching_stats lets the end byte match itself)
    want = {k: p.want(qs, k) for k in (1, 5, 20)}
    rev = p.g.fm(0)
    assert rev.info["samples"] == 0
    for sample in (1, 7, 32):
        for threads in (1, 3, 0):
            fwd = p.f.fm(sample, threads)
            got = fwd.matching_stats(qs, rev, threads)
            assert all(g.dtype == np.uint32 for g in got)
            assert [g.tolist() for g in got] == [w.tolist() for w in want[1][0]], (sample, threads)
            for k in (1, 5, 20):
                assert same_columns(fwd.smem_arrays(*pack_queries(qs), rev, k, threads=threads), want[k][1]), (sample, threads, k)
    fwd = p.f.fm(7)
    assert [g.tolist() for g in fwd.matching_stats(no_e, rev)] == [g.tolist() for g in p.f.matching_statistics(no_e)]
    for k in (1, 5, 20):
        assert same_columns(fwd.smem_arrays(*pack_queries(no_e), rev, k), p.f.smem_arrays(*pack_queries(no_e), k)), k
        for max_hits in (0, 2):
            assert repr(fwd.smems(no_e, rev, k, max_hits)) == repr(p.f.smems(no_e, k, max_hits)), (k, max_hits)


def test_query_sets_meet_their_conditions(pairs):
    """over the six golden files the query sets hold every case the pair must get right; the small files cannot hold all"""
    seen = {}
    for name in LF_FILES:
        p = pairs(name)
        seen[name] = conditions(p, query_set(p, seed=len(name)), p.f.fm(0).info["block"])
        assert {"empty", "one_byte", "end_byte_inside", "end_byte_last", "is_X", "is_T", "two_ranks", "none_at_20"} <= seen[name], (name, seen[name])
    assert "absent_byte" in seen["abba.sufr"] and "absent_byte" in seen["long_dna_sequence_allow_ambiguity.sufr"]
    for name in ("long_dna_sequence_allow_ambiguity.sufr", "uniprot.sufr"):
        assert {"three_cover", "two_blocks"} <= seen[name], (name, seen[name])
    for name in ("2n.sufr", "2ns.sufr", "uniprot.sufr"):
        assert "across_delimiter" in seen[name], (name, seen[name])


def check_pair(p: Pair, qs, min_lens=(1, 5), samples=(7, 0), threads=(0, 2)):
    rev = p.g.fm(0)
    for k in min_lens:
        w_ms, w_cols = p.want(qs, k)
        for sample in samples:
            fwd = p.f.fm(sample)
            for t in threads:
                assert [g.tolist() for g in fwd.matching_stats(qs, rev, t)] == [w.tolist() for w in w_ms], (k, sample, t)
                assert same_columns(fwd.smem_arrays(*pack_queries(qs), rev, k, threads=t), w_cols), (k, sample, t)
    return rev


def planted_bodies():
    rng = np.random.default_rng(3)
    return {"a": np.full(1000, ord("A"), dtype=np.uint8), "fib": fibonacci(3000),
            "rnd": np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 959)]}


def test_planted_texts_through_the_oracle(oracle, tmp_path):
    """A^1000, a Fibonacci string of 3 000 and random DNA of 959, forward and reversed FASTA both through the oracle; fwd at
    sample 0 gives the statistics and the ranges too"""
    for name, body in planted_bodies().items():
        f = oracle_file(oracle, tmp_path, body, name, is_dna=True, allow_ambiguity=True)
        f.write_reversed_fasta(tmp_path / f"{name}_rev.fa")
        oracle.create(tmp_path / f"{name}_rev.fa", tmp_path / f"{name}_rev.sufr", is_dna=True, allow_ambiguity=True)
        p = Pair(f, SufrFile(tmp_path / f"{name}_rev.sufr"))
        qs = query_set(p, seed=7, count=16, max_len=300) + [b"A" * 2000, bytes(fibonacci(2584)), p.X[:500] + b"C" + p.X[400:]]
        check_pair(p, qs)


def test_all_byte_values_and_an_end_byte_that_is_not_the_smallest(tmp_path):
    rng = np.random.default_rng(11)
    text = rng.integers(0, 255, 5000).astype(np.uint8)
    text[:255] = np.arange(255)
    text[-1] = 255                                                    # the end byte is the largest byte value
    p = planted_pair(tmp_path, text, "bytes")
    rev = check_pair(p, query_set(p, seed=2, count=16), samples=(32,))
    assert (rev.info["symbols"], rev.info["block"], rev.info["stride"]) == (256, 1024, 2048)
    middle = np.frombuffer(b"TTGACCA$GATTACA$$ACGT" * 9 + b"M", dtype=np.uint8)      # 'M' ends the text: '$' and 'A'.. are smaller and larger
    p = planted_pair(tmp_path, middle, "middle")
    check_pair(p, query_set(p, seed=4, count=16) + [b"CCA$GATTACA$$ACGTTTGA", b"MTTGA", b"ACGTM"])


@pytest.mark.parametrize("n", [95, 96, 97, 191, 192, 193])
def test_sizes_around_the_block(tmp_path, n):
    rng = np.random.default_rng(n)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()
    text[-1] = ord("$")
    p = planted_pair(tmp_path, text, "s")
    rev = check_pair(p, query_set(p, seed=n, count=12))
    assert rev.info["block"] == 96 and rev.info["ranks"] == n


# ---------------------------------------------------------------------------------------------------------------------
# slabs and steps
# ---------------------------------------------------------------------------------------------------------------------
def with_slab(slab, call):
    """the host path cut at `slab` bytes: a knob of the library for this test, read at every call"""
    old = os.environ.get(SLAB_ENV)
    try:
        if slab is None:
            os.environ.pop(SLAB_ENV, None)
        else:
            os.environ[SLAB_ENV] = str(slab)
        return call()
    finally:
        if old is None:
            os.environ.pop(SLAB_ENV, None)
        else:
            os.environ[SLAB_ENV] = old


def test_slabs_give_the_arrays_of_the_uncut_walk(pairs):
    p = pairs("long_dna_sequence_allow_ambiguity.sufr")
    fwd, rev = p.f.fm(32), p.g.fm(0)
    long_query = p.X[1000:1150] + b"T" + p.X[3000:3100]              # longer than three slabs of 64, with SMEMs across their cuts
    qs = query_set(p, seed=9, count=20)[4:] + [long_query]
    ms = brute_ms(p.X, long_query)
    assert len(long_query) > 3 * 64 and any(j < cut < j + l for j, l in smems_of(ms, 1) for cut in (64, 128, 192))
    whole = with_slab(1 << 30, lambda: (fwd.matching_stats(qs, rev, 1), fwd.smem_arrays(*pack_queries(qs), rev, 5, threads=1)))
    assert [g.tolist() for g in whole[0]] == [brute_ms(p.X, q).tolist() for q in qs]
    for slab in (1, 7, 64, None):
        for threads in (1, 3):
            got = with_slab(slab, lambda: (fwd.matching_stats(qs, rev, threads), fwd.smem_arrays(*pack_queries(qs), rev, 5, threads=threads)))
            assert [g.tolist() for g in got[0]] == [g.tolist() for g in whole[0]], (slab, threads)
            assert same_columns(got[1], whole[1]), (slab, threads)


def test_steps_stay_below_their_bounds(pairs):
    """every query takes at most 2 * (the summed lengths of its SMEMs at min_len 1) + 2 m steps, and reads cut from the text
    with up to three substitutions take fewer than 3 steps per byte in all, which a search of every offset on its own does not
    (it takes about ms[j] per offset); the Python walk of the witness stays under the same cap and takes the same steps"""
    rng = np.random.default_rng(1)
    for _ in range(300):                                              # the Python walk, which the cap is taken from, is the brute force
        k = int(rng.integers(2, 5))
        X = bytes(rng.choice(list(b"ACGT"[:k]), int(rng.integers(1, 60))))
        q = bytes(rng.choice(list(b"ACGTN"[:k + 1]), int(rng.integers(0, 30))))
        assert np.array_equal(walk(X, q)[0], brute_ms(X, q)), (X, q)
    p = pairs("long_dna_sequence_allow_ambiguity.sufr")
    fwd, rev = p.f.fm(0), p.g.fm(0)
    qs = query_set(p, seed=5)
    steps = fwd.matching_stats_steps(qs, rev)
    assert steps.dtype == np.uint64 and steps.size == len(qs)
    for q, st in zip(qs, steps):
        ms = brute_ms(p.X, q)
        assert int(st) <= 2 * sum(l for _, l in smems_of(ms, 1)) + 2 * len(q), (q, st)
        if len(q) < 400:
            assert int(st) == walk(p.X, q)[1], q
    rng = np.random.default_rng(8)
    reads = []
    for a in rng.integers(0, len(p.X) - 150, 200):
        r = bytearray(p.X[a:a + 150])
        for at in rng.integers(0, 150, int(rng.integers(0, 4))):
            r[at] = b"ACGT"[(b"ACGT".index(r[at]) + 1) % 4] if r[at] in b"ACGT" else ord("A")
        reads.append(bytes(r))
    total = sum(len(r) for r in reads)
    witness_steps = sum(walk(p.X, r)[1] for r in reads[:40])
    assert witness_steps < 3 * sum(len(r) for r in reads[:40])
    got = fwd.matching_stats_steps(reads, rev, 2)
    assert int(got[:40].sum()) == witness_steps and int(got.sum()) < 3 * total
    assert sum(int(brute_ms(p.X, r).sum()) for r in reads[:40]) > 3 * sum(len(r) for r in reads[:40])      # the search of every offset on its own


# ---------------------------------------------------------------------------------------------------------------------
# refusals, capacity, lifetime
# ---------------------------------------------------------------------------------------------------------------------
def test_pairs_that_fail_the_check_are_refused(tmp_path):
    def pair(a: bytes, b: bytes, tag: str):
        ta, tb = (np.frombuffer(t, dtype=np.uint8) for t in (a, b))
        return (write_arrays(tmp_path / f"{tag}_a.sufr", ta, sorted_sa(ta)).fm(4), write_arrays(tmp_path / f"{tag}_b.sufr", tb, sorted_sa(tb)).fm(0))
    cases = {"length": (b"ACGTACGTAC$", b"ACGTACGTA$"), "end byte": (b"ACGTACGTAC$", b"ACGTACGTAC#"), "counts": (b"ACGTACGTAC$", b"ACGTACGTAA$")}
    for tag, (a, b) in cases.items():
        fwd, rev = pair(a, b, tag.replace(" ", "_"))
        with pytest.raises(SufrHipError) as err:
            fwd.matching_stats([b"ACGT"], rev)
        assert err.value.code == INVALID and "not an index of the reversed text" in str(err.value), tag
        with pytest.raises(SufrHipError) as err:
            fwd.smem_arrays(*pack_queries([b"ACGT"]), rev, 1)
        assert err.value.code == INVALID, tag
        with pytest.raises(SufrHipError) as err:
            fwd.matching_stats_steps([b"ACGT"], rev)
        assert err.value.code == INVALID, tag
    # equal counts, another text: the check passes (it is necessary, not sufficient) and every call ends inside its arrays
    fwd, rev = pair(b"ACGTACGTAC$", b"CCGTAAGTAC$", "other")
    fwd.pair_check(rev)
    qs = [b"ACGTACGTAC", b"GTAAG", b"TTTT", b"CATGCATGCA"]
    assert sum(m.size for m in fwd.matching_stats(qs, rev)) == sum(map(len, qs))
    fwd.smem_arrays(*pack_queries(qs), rev, 1)


def test_min_len_capacity_and_the_empty_batch(pairs):
    p = pairs("abba.sufr")
    fwd, rev = p.f.fm(2), p.g.fm(0)
    qs = [b"ABBA", b"BABAB", b"", b"AAB"]
    qb, off = pack_queries(qs)
    with pytest.raises(SufrHipError) as err:
        fwd.smem_arrays(qb, off, rev, 0)
    assert err.value.code == INVALID
    want = fwd.smem_arrays(qb, off, rev, 1)
    total = len(want[0])
    assert total >= 3 and same_columns(want, p.want(qs, 1)[1])
    with pytest.raises(SufrHipError) as err:
        fwd.smem_arrays(qb, off, rev, 1, cap=total - 1)
    assert err.value.code == CAPACITY and err.value.total == total
    # the C call itself: the total is set and nothing is filled
    cols = [np.full(total, 0xAB, dtype=d) for d in (np.uint64, np.uint32, np.uint32, np.uint64, np.uint64)]
    keep = [c.copy() for c in cols]
    t = C.c_uint64(0)
    rc = sufr_amd.lib().sufr_fm_smems(fwd._h, rev._h, qb.ctypes.data, off.ctypes.data, len(qs), 1, total - 1, *[c.ctypes.data for c in cols], C.byref(t), 0)
    assert rc == CAPACITY and t.value == total and all(np.array_equal(a, b) for a, b in zip(cols, keep))
    assert same_columns(fwd.smem_arrays(qb, off, rev, 1, cap=total), want)
    assert fwd.matching_stats([], rev) == [] and all(c.size == 0 for c in fwd.smem_arrays(*pack_queries([]), rev, 1))
    assert fwd.matching_stats([b""], rev)[0].size == 0 and fwd.smems([b"", b""], rev, 1) == [[], []]
    assert fwd.matching_stats_steps([], rev).size == 0


def test_the_pair_outlives_its_files_and_a_save_and_load(tmp_path):
    src, rsrc = tmp_path / "f.sufr", tmp_path / "r.sufr"
    shutil.copy(EXP / "long_dna_sequence_allow_ambiguity.sufr", src)
    f = SufrFile(src)
    p = Pair(f, write_arrays(rsrc, reversal(np.asarray(f.text)), sorted_sa(reversal(np.asarray(f.text)))))
    qs = query_set(p, seed=6, count=12)
    qb, off = pack_queries(qs)
    fwd, rev = p.f.fm(32), p.g.fm(0)
    want_ms, want = [m.tolist() for m in fwd.matching_stats(qs, rev)], fwd.smem_arrays(qb, off, rev, 5)
    assert same_columns(want, p.want(qs, 5)[1])
    no_e = [q for q in qs if p.e not in q]
    hits = repr(p.f.smems(no_e, 5))
    p.f.close(); p.g.close()
    src.unlink(); rsrc.unlink()
    assert [m.tolist() for m in fwd.matching_stats(qs, rev)] == want_ms and same_columns(fwd.smem_arrays(qb, off, rev, 5), want)
    assert repr(fwd.smems(no_e, rev, 5)) == hits
    fwd.save(tmp_path / "fwd.fm"); rev.save(tmp_path / "rev.fm")
    fwd2, rev2 = FmIndex.load(tmp_path / "fwd.fm"), FmIndex.load(tmp_path / "rev.fm")
    fwd.close(); rev.close()
    assert rev2.info["sample"] == 0
    assert [m.tolist() for m in fwd2.matching_stats(qs, rev2)] == want_ms and same_columns(fwd2.smem_arrays(qb, off, rev2, 5), want)
    assert repr(fwd2.smems(no_e, rev2, 5)) == hits


# ---------------------------------------------------------------------------------------------------------------------
# sufr fm --write-reverse / --smems --reverse
# ---------------------------------------------------------------------------------------------------------------------
def cli_files(oracle, tmp_path, name):
    """the forward file, the oracle's .sufr of `sufr fm --write-reverse`, and both saved as index files"""
    src, fa, rev = tmp_path / name, tmp_path / "rev.fa", tmp_path / "rev.sufr"
    shutil.copy(EXP / name, src)
    assert run("fm", src, "--write-reverse", fa).stdout == ""
    f = SufrFile(src)
    oracle.create(fa, rev, is_dna=f.is_dna, allow_ambiguity=f.allow_ambiguity, ignore_softmask=f.ignore_softmask)
    f.close()
    fwd_fm, rev_fm = tmp_path / "fwd.fm", tmp_path / "rev.fm"
    run("fm", src, "--save", fwd_fm, "-s", 8)
    run("fm", rev, "--save", rev_fm, "-s", 0)
    return src, rev, fwd_fm, rev_fm


CLI_QUERIES = {"long_dna_sequence_allow_ambiguity.sufr": ["ACGTACGTTTGACCAGTAGGACCATTTAGGAC", "GATTACA", "NNNNNNNNNNNNNNNNNNNNNNNNN", "TTTTTTTTTTTTTTTTTTTTTTTTTT"],
               "uniprot.sufr": ["MKVLAAGIVGLLLAQWCSAHKLEERYQ", "ACDEFGHIKLMNPQRSTVWY", "MMMMMMMMM"]}


def cli_queries(src, name):
    """with two windows of the text, one of them two distant pieces glued together: SMEMs at -k 20 too"""
    raw = SufrFile(src).text.tobytes()
    return CLI_QUERIES[name] + [raw[500:560].decode(), raw[900:930].decode() + raw[40:75].decode()]


@pytest.mark.parametrize("name", sorted(CLI_QUERIES))
def test_cli_prints_the_bytes_of_match(oracle, tmp_path, name):
    src, rev, fwd_fm, rev_fm = cli_files(oracle, tmp_path, name)
    queries = cli_queries(src, name)
    reads = tmp_path / "reads.fa"
    reads.write_text("".join(f">r{i}\n{q}\n" for i, q in enumerate(queries)))
    for k in (5, 20):
        want = run("match", "-k", k, src, *queries)
        assert want.stdout
        for args in (("fm", src, "--smems", "--reverse", rev), ("fm", src, "--smems", "--reverse", rev_fm, "-s", 7),
                     ("fm", "--index", fwd_fm, "--smems", "--reverse", rev_fm), ("fm", "--index", fwd_fm, "--smems", "--reverse", rev, "-t", 2)):
            assert run(*args, "-k", k, *queries).stdout == want.stdout, (k, args)
        assert run("fm", src, "--smems", "--reverse", rev, "-k", k, "-a", *queries).stdout == run("match", "-k", k, "-a", src, *queries).stdout
        assert run("fm", src, "--smems", "--reverse", rev, "-k", k, "--max-hits", 2, *queries).stdout == run("match", "-k", k, "-n", 2, src, *queries).stdout
    named = run("fm", "--index", fwd_fm, "--smems", "--reverse", rev_fm, "-k", 5, "-q", reads, "-o", tmp_path / "out.txt")
    assert named.stdout == "" and (tmp_path / "out.txt").read_text() == run("match", "-k", 5, "-q", reads, src).stdout != ""
    src.write_bytes(b""); rev.write_bytes(b"")                        # the index files answer without any .sufr
    assert run("fm", "--index", fwd_fm, "--smems", "--reverse", rev_fm, "-k", 20, *queries).stdout == want.stdout


def test_cli_error_exits(oracle, tmp_path):
    src, rev, fwd_fm, rev_fm = cli_files(oracle, tmp_path, "long_dna_sequence_allow_ambiguity.sufr")
    other = tmp_path / "abba.sufr"
    shutil.copy(EXP / "abba.sufr", other)
    bare = tmp_path / "bare.fm"
    run("fm", src, "--save", bare, "-s", 0)
    for args, word in ((("fm", src, "--smems", "ACGT"), "--reverse"), (("fm", src, "--smems", "--reverse", other, "ACGT"), "not an index of the reversed text"),
                       (("fm", src, "--smems", "--reverse", rev, "-s", 0, "ACGT"), "-s"), (("fm", "--index", bare, "--smems", "--reverse", rev_fm, "ACGT"), "samples"),
                       (("fm", src, "--smems", "--reverse", rev, "-k", 0, "ACGT"), "--min-len"), (("fm", src, "--smems", "--reverse", tmp_path / "none", "ACGT"), "none"),
                       (("fm", src, "--reverse", rev, "ACGT"), "--smems"), (("fm", "--index", fwd_fm, "--write-reverse", tmp_path / "x.fa"), "--write-reverse")):
        r = run(*args, check=False)
        assert r.returncode == 1 and r.stdout == "" and word in r.stderr, (args, r.stderr)


def test_cli_through_the_sanitizer_build(oracle, tmp_path):
    """the same commands through the stand-alone sanitizer build of the CLI (nothing preloaded) on two golden files: exit 0, the
    bytes of the plain build, and no report"""
    from test_fm_text_host import asan_cli
    exe = asan_cli()
    for name in sorted(CLI_QUERIES):
        d = tmp_path / name.split(".")[0]
        d.mkdir()
        src, rev, fwd_fm, rev_fm = cli_files(oracle, d, name)
        queries = cli_queries(src, name)
        r = subprocess.run([str(exe), "fm", str(src), "--write-reverse", str(d / "asan.fa")], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "" and (d / "asan.fa").read_bytes() == (d / "rev.fa").read_bytes()
        for args in ((str(src), "--smems", "--reverse", str(rev)), ("--index", str(fwd_fm), "--smems", "--reverse", str(rev_fm), "-t", "3")):
            for k in ("5", "20"):
                r = subprocess.run([str(exe), "fm", *args, "-k", k, *queries], capture_output=True, text=True)
                assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr and r.stderr == "", r.stderr[-2000:]
                assert r.stdout == run("match", "-k", k, src, *queries).stdout != ""
