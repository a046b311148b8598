"""Sequence counts of repeats and k-common substrings on the host (include/sufr_shared.h): no GPU.

The dictionary witness uses no suffix order and no LCP array: the repeats come from witness_dictionary of
tests/test_repeat_host.py, and the sequences of a repeat are counted by looking for its string in the text of every
sequence.  The identity behind the count -- seqs([a, b)) = (b - a) - (P[b] - P[a + 1]) -- is held to len(set(D[a:b])) on
every interval, through the shared arithmetic of the device path (sufr_amd/csrc/sufr_shared_scan.h, tests/shared_shim.cpp).
"""
import bisect
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
from test_repeat_host import KINDS, clipped, filtered, oracle_file, small_bodies, stack_answers, witness_dictionary, _rewrite

ROOT = Path(__file__).resolve().parent.parent
EXP = GOLDEN / "expected"
GOLDEN_FILES = sorted(p.name for p in EXP.glob("*.sufr"))
NOTHING = dict(records=0, longest=0, longest_rank=0, max_count=0, max_seqs=0)
# (min_len, min_count, max_count, min_seqs, max_seqs)
FILTERS = [(1, 2, 0, 0, 0), (1, 2, 0, 1, 1), (1, 2, 0, 2, 0), (2, 3, 0, 2, 3), (1, 2, 4, 0, 2), (3, 2, 0, 3, 0)]
FF = 0xFFFFFFFFFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------------
# the witness
# ---------------------------------------------------------------------------------------------------------------------
def sequence_texts(f: SufrFile):
    """the bytes of every sequence without its closing break"""
    tb, st, n = bytes(f.text), list(f.sequence_starts), f.text_len
    return [tb[st[i]:(st[i + 1] if i + 1 < len(st) else n) - 1] for i in range(len(st))]


def docs_of(f: SufrFile) -> np.ndarray:
    """D[r], by bisection of the sequence starts"""
    st = list(f.sequence_starts)
    return np.array([bisect.bisect_right(st, int(p)) - 1 for p in np.asarray(f.suffix_array)], dtype=np.int64)


def witness_shared(f: SufrFile):
    """{kind: set of (length, frozenset of positions, sequences that contain the string)}; the third by substring search in
    the sequences' own bytes, and -- where no delimiter byte lies inside a sequence -- equal to the sequences of the positions"""
    tb, seqs, st = bytes(f.text), sequence_texts(f), list(f.sequence_starts)
    out = {}
    for kind, recs in witness_dictionary(f).items():
        out[kind] = set()
        for length, ps in recs:
            p = min(ps)
            word = tb[p:p + length]
            holds = sum(1 for s in seqs if word in s)
            assert holds == len({bisect.bisect_right(st, q) - 1 for q in ps}), (word, sorted(ps))
            out[kind].add((length, ps, holds))
    return out


def filtered_shared(recs, ml, mc, xc, mq, xq):
    keep = filtered({(ln, ps) for ln, ps, _ in recs}, ml, mc, xc)
    return {(ln, ps, q) for ln, ps, q in recs if (ln, ps) in keep and q >= mq and (xq == 0 or q <= xq)}


def host_set(f: SufrFile, kind, ml, mc=2, xc=0, mq=0, xq=0, threads=0):
    sa = np.asarray(f.suffix_array).astype(np.int64)
    rank, count, length, seqs, st = f.shared(kind, ml, mc, xc, mq, xq, threads=threads)
    recs = [(int(ln), frozenset(sa[int(a):int(a) + int(c)].tolist()), int(q)) for a, c, ln, q in zip(rank, count, length, seqs)]
    assert len(set(recs)) == len(recs) == st["records"]
    assert st["max_seqs"] == max((q for _, _, q in recs), default=0) and st["max_count"] == max((len(ps) for _, ps, _ in recs), default=0)
    assert st["longest"] == max((ln for ln, _, _ in recs), default=0)
    return set(recs)


def common_brute(f: SufrFile) -> list:
    """common[q - 1] from a table of every break-free string that starts at an indexed position"""
    from test_repeat_host import brk_of
    tb, brk, st = bytes(f.text), brk_of(f).tolist(), list(f.sequence_starts)
    table = {}
    for p in sorted(set(np.asarray(f.suffix_array).tolist())):
        d = bisect.bisect_right(st, p) - 1
        for ln in range(1, brk[p] - p + 1):
            e = table.setdefault(tb[p:p + ln], [0, set()])
            e[0] += 1
            e[1].add(d)
    out = [0] * max(len(st), 1)
    for word, (count, docs) in table.items():
        if count >= 2:
            for q in range(len(docs)):
                out[q] = max(out[q], len(word))
    return out


def check_witness(f: SufrFile, seen):
    want = witness_shared(f)
    for kind in KINDS:
        for flt in FILTERS:
            assert host_set(f, kind, *flt) == filtered_shared(want[kind], *flt), (kind, flt)
        seen[kind] += len(want[kind])
    seen["shared"] += sum(1 for _, _, q in want[0] if q >= 2)
    seen["private"] += sum(1 for _, _, q in want[0] if q == 1)
    common = f.common()
    assert common.dtype == np.uint64 and common.tolist() == common_brute(f)
    assert (np.diff(common.astype(np.int64)) <= 0).all() and int(common[0]) == f.repeats(0, 1)[3]["longest"]


# ---------------------------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_shared_header_symbols_are_exported():
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "sufr_shared.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(sufr_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(sufr_amd.SHARED_EXPORTS), declared ^ set(sufr_amd.SHARED_EXPORTS)
    L = sufr_amd.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(sufr_amd.LIB_PATH)], capture_output=True, text=True).stdout
    for name in declared:
        assert hasattr(L, name) and re.search(rf"\bT {name}\b", nm), name
    assert L.sufr_hip_abi_version() == 3
    assert C.sizeof(sufr_amd.SharedStats) == 40
    stubs = (ROOT / "sufr_amd" / "csrc" / "sufr_host_stubs.cpp").read_text()
    for name in sufr_amd.SHARED_EXPORTS:
        if name.startswith("sufr_hip_"):
            assert re.search(rf"\bint {name}\(", stubs), name


# ---------------------------------------------------------------------------------------------------------------------
# against the dictionary witness
# ---------------------------------------------------------------------------------------------------------------------
def random_collection(rng):
    """1-8 sequences of up to ~60 symbols over 2 or 4 letters, as '%'-joined bytes and the build options: duplicated
    sequences, one-symbol sequences, empty ones in the middle (adjacent delimiters), N runs and lowercase runs"""
    letters = np.frombuffer(b"AC" if rng.integers(0, 2) else b"ACGT", dtype=np.uint8)
    k = int(rng.integers(1, 9))
    seqs = []
    for i in range(k):
        what = int(rng.integers(0, 10))
        if what == 0 and seqs:
            s = seqs[int(rng.integers(0, len(seqs)))].copy()          # a duplicate
        elif what == 1:
            s = letters[rng.integers(0, letters.size, 1)]             # one symbol
        elif what == 2 and 0 < i < k - 1:
            s = np.zeros(0, dtype=np.uint8)                           # empty: two delimiters side by side
        else:
            s = letters[rng.integers(0, letters.size, int(rng.integers(2, 61)))]
            if what == 3 and s.size > 6:                              # a piece of an earlier sequence: a shared repeat
                src = seqs[int(rng.integers(0, len(seqs)))] if seqs else s
                if src.size > 3:
                    piece = src[:int(rng.integers(2, min(src.size, 30)))]
                    at = int(rng.integers(0, s.size))
                    s = np.concatenate([s[:at], piece, s[at:]])[:70]
        seqs.append(s)
    mode = int(rng.integers(0, 4))                                    # 0 dna, 1 dna with N runs, 2 soft-masked, 3 bytes
    build = dict(is_dna=mode != 3)
    for s in seqs:
        if mode in (1, 2) and s.size > 8 and rng.integers(0, 2):
            a = int(rng.integers(0, s.size - 3))
            b = a + int(rng.integers(1, 6))
            if mode == 1:
                s[a:b] = ord("N")
            else:
                s[a:b] = s[a:b] + 32                                  # lowercase
    if mode == 2:
        build["ignore_softmask"] = True
    body = np.concatenate([np.concatenate([s, np.frombuffer(b"%", dtype=np.uint8)]) for s in seqs])[:-1]
    if body.size < 6:                                                 # (a text the builder can partition)
        body = np.concatenate([letters[rng.integers(0, letters.size, 6)], body])
    return body, build


def test_host_equals_dictionary_witness_on_random_collections(oracle, tmp_path):
    rng = np.random.default_rng(21)
    seen = {0: 0, 1: 0, 2: 0, "shared": 0, "private": 0}
    nums, unindexed = set(), 0
    for i in range(300):
        body, build = random_collection(rng)
        f = oracle_file(oracle, tmp_path, body, "c", **build)
        nums.add(f.num_sequences)
        unindexed += f.len_suffixes < f.text_len - f.num_sequences
        check_witness(f, seen)
        f.close()
    assert nums == set(range(1, 9)) and unindexed > 30, (nums, unindexed)
    assert all(seen[k] > 1000 for k in (0, 1, "shared", "private")) and seen[2] > 100, seen


def cut(body: np.ndarray, every: int) -> np.ndarray:
    """a delimiter over every `every`-th symbol of a body that has none"""
    out = body.copy()
    if not (out == ord("%")).any():
        out[every::every] = ord("%")
    return out


@pytest.mark.parametrize("build", [dict(is_dna=True), dict(is_dna=True, allow_ambiguity=True), dict(is_dna=False),
                                   dict(is_dna=True, ignore_softmask=True)], ids=["dna", "ambiguity", "bytes", "softmask"])
def test_host_equals_dictionary_witness_on_adversarial_bodies(oracle, tmp_path, build):
    seen = {0: 0, 1: 0, 2: 0, "shared": 0, "private": 0}
    for kind, body in small_bodies().items():
        body = cut(body, 97)
        if build.get("ignore_softmask"):
            body = body.copy()
            body[10:40] = np.where(body[10:40] == ord("%"), body[10:40], body[10:40] | 32)
        f = oracle_file(oracle, tmp_path, body, kind, **build)
        assert f.num_sequences >= 2
        check_witness(f, seen)
        if kind == "several" and not build.get("ignore_softmask"):
            # the twice-present sequence: one record of 90 symbols in two sequences
            st = f.sequence_starts
            assert (90, frozenset({st[0], st[2]}), 2) in host_set(f, 2, 1)
    assert all(v > 0 for v in seen.values()), seen


def test_host_equals_dictionary_witness_on_golden_files():
    seen = {0: 0, 1: 0, 2: 0, "shared": 0, "private": 0}
    for name in GOLDEN_FILES:
        f = SufrFile(EXP / name)
        if not f.seed_mask and f.text_len < 200:
            check_witness(f, seen)
    assert seen[0] > 0 and seen["shared"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# the identity itself and the pair primitive (sufr_shared_scan.h) on the CPU
# ---------------------------------------------------------------------------------------------------------------------
SHIM_SRC = ROOT / "tests" / "shared_shim.cpp"
SHIM_DEPS = (SHIM_SRC,) + tuple(ROOT / "sufr_amd" / "csrc" / h for h in ("sufr_shared_scan.h", "sufr_lz_scan.h", "sufr_repeat_scan.h", "sufr_kmer_scan.h"))
NONE = (1 << 64) - 1


@pytest.fixture(scope="module")
def shim():
    out = ROOT / "tests" / "_build" / "libshared_shim.so"
    out.parent.mkdir(exist_ok=True)
    if not out.exists() or any(out.stat().st_mtime < p.stat().st_mtime for p in SHIM_DEPS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", str(out), str(SHIM_SRC)], check=True)
    L = C.CDLL(str(out))
    vp, u64 = C.c_void_p, C.c_uint64
    L.shim_shr_pyramid_size.argtypes = [u64]; L.shim_shr_pyramid_size.restype = u64
    L.shim_shr_levels.argtypes = [u64]; L.shim_shr_levels.restype = C.c_uint32
    L.shim_shr_pyramid.argtypes = [vp, u64, vp]; L.shim_shr_pyramid.restype = None
    L.shim_shr_doc.argtypes = [vp, u64, u64]; L.shim_shr_doc.restype = u64
    L.shim_shr_key.argtypes = [u64, u64]; L.shim_shr_key.restype = u64
    L.shim_shr_key_doc.argtypes = [u64]; L.shim_shr_key_doc.restype = u64
    L.shim_shr_key_rank.argtypes = [u64]; L.shim_shr_key_rank.restype = u64
    L.shim_shr_doc_bits.argtypes = [u64]; L.shim_shr_doc_bits.restype = C.c_uint32
    L.shim_shr_pair.argtypes = [vp, vp, u64, u64, u64, C.POINTER(u64)]; L.shim_shr_pair.restype = u64
    L.shim_shr_prefix.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, vp]; L.shim_shr_prefix.restype = u64
    L.shim_shr_seqs.argtypes = [vp, u64, u64]; L.shim_shr_seqs.restype = u64
    L.shim_shr_keep.argtypes = [u64, u64, u64]; L.shim_shr_keep.restype = C.c_int
    return L


def shim_prefix(shim, ell: np.ndarray, docs: np.ndarray, num: int):
    """(prev, q, H, P, most reads of one primitive) of the arrays l[0..s) and D[0..s)"""
    s = ell.size
    ell = np.ascontiguousarray(ell, dtype=np.uint64)
    docs = np.ascontiguousarray(docs, dtype=np.uint64)
    up = np.zeros(shim.shim_shr_pyramid_size(s), dtype=np.uint64)
    shim.shim_shr_pyramid(ell.ctypes.data, s, up.ctypes.data)
    prev, qs, H, P = (np.zeros(s + 1, dtype=np.uint64) for _ in range(4))
    most = shim.shim_shr_prefix(ell.ctypes.data, up.ctypes.data, s, docs.ctypes.data, num, prev.ctypes.data, qs.ctypes.data, H.ctypes.data, P.ctypes.data)
    return prev[:s], qs[:s], H, P, most


def check_identity(shim, f: SufrFile):
    """every interval of the file: the formula over the shim's P equals len(set(D[a:b])); every pair equals a linear scan"""
    s = f.len_suffixes
    if s < 2:
        return 0
    ell, D = clipped(f)[:-1].astype(np.uint64), docs_of(f)
    prev, qs, H, P, most = shim_prefix(shim, ell, D, f.num_sequences)
    assert most <= 2 * 64 * (shim.shim_shr_levels(s) + 1)
    last = {}
    e = ell.tolist()
    for r in range(s):
        p = last.get(int(D[r]))
        last[int(D[r])] = r
        assert int(prev[r]) == (NONE if p is None else p)
        if p is not None:
            m = min(e[p + 1:r + 1])
            assert int(qs[r]) == p + 1 + e[p + 1:r + 1].index(m), (p, r)
    assert int(H.sum()) == s - len(last) and int(P[s]) == int(H.sum()) and np.array_equal(P[1:], np.cumsum(H)[:-1])
    left, right = stack_answers(ell)
    done = 0
    for r in range(1, s):
        if e[r] >= 1 and e[int(left[r])] < e[r]:                      # a representative
            a, b = int(left[r]), int(right[r])
            assert shim.shim_shr_seqs(P.ctypes.data, a, b) == len(set(D[a:b].tolist())), (a, b)
            done += 1
    return done


def test_identity_and_pair_primitive_through_the_shim(shim, oracle, tmp_path):
    rng = np.random.default_rng(33)
    done = 0
    for i in range(150):
        body, build = random_collection(rng)
        f = oracle_file(oracle, tmp_path, body, "c", **build)
        done += check_identity(shim, f)
        f.close()
    for kind, body in small_bodies().items():
        for every in (97, 13):
            done += check_identity(shim, oracle_file(oracle, tmp_path, cut(body, every), kind, is_dna=True))
    for name in GOLDEN_FILES:
        f = SufrFile(EXP / name)
        if not f.seed_mask and f.len_suffixes < 5000:
            done += check_identity(shim, f)
    assert done > 5000
    # pairs that are far apart: 300 000 ranks, three levels above l; dips on block boundaries, plateaus between them
    s = 300_000
    ell = np.where(np.arange(s) % 4096 == 0, 1, np.where(np.arange(s) % 64 == 0, 2, 3)).astype(np.uint64)
    ell[0] = 0
    ell[200_000] = 0
    D = (np.arange(s) % 7 == 0).astype(np.uint64)                     # sequence 1 on every 7th rank
    D[[5, s - 3]] = 2                                                 # a pair almost as long as the array
    prev, qs, H, P, most = shim_prefix(shim, ell, D, 3)
    assert shim.shim_shr_levels(s) == 3 and most <= 2 * 64 * 4
    assert int(prev[s - 3]) == 5 and int(qs[s - 3]) == 200_000        # the smallest, and of several the first
    assert int(qs[14]) == 8 and int(qs[4096 + 6]) == 4096 and int(qs[64 * 7]) == 64 * 7      # (7, 14]: all 3; a dip inside; a dip at r itself
    for a, b in ((0, 200_000), (200_000, s), (4096, 8192), (64, 128)):   # intervals of value 1, 1, 2 and 3
        assert ell[a + 1:b].min() > max(int(ell[a]), int(ell[b]) if b < s else 0)
        assert shim.shim_shr_seqs(P.ctypes.data, a, b) == len(set(D[a:b].tolist())), (a, b)
    # the sequence of a position, the key and its digits
    st = np.array([0, 5, 6, 40], dtype=np.uint64)
    assert [shim.shim_shr_doc(st.ctypes.data, 4, p) for p in (0, 4, 5, 6, 39, 40, 10 ** 12)] == [0, 0, 1, 2, 2, 3, 3]
    assert shim.shim_shr_doc(st.ctypes.data, 1, 77) == 0 and shim.shim_shr_doc(None, 0, 77) == 0
    assert [shim.shim_shr_doc_bits(k) for k in (0, 1, 2, 3, 256, 257, 300, 70_000, 1 << 24)] == [0, 0, 1, 2, 8, 9, 9, 17, 24]
    key = shim.shim_shr_key((1 << 24) - 1, (1 << 40) - 1)
    assert key == NONE and shim.shim_shr_key_doc(key) == (1 << 24) - 1 and shim.shim_shr_key_rank(key) == (1 << 40) - 1
    assert [shim.shim_shr_keep(q, lo, hi) for q, lo, hi in ((1, 0, 0), (1, 2, 0), (3, 2, 3), (4, 2, 3), (2, 0, 1))] == [1, 0, 1, 0, 0]


def test_shared_arithmetic_under_the_sanitizers(tmp_path):
    """the same shim as a stand-alone program with AddressSanitizer and UBSan: host code, run as it is"""
    exe = tmp_path / "shared_shim_main"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DSHARED_SHIM_MAIN", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", str(exe), str(SHIM_SRC)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and re.fullmatch(r"ok \d+\n", r.stdout), r.stdout[-2000:] + r.stderr[-3000:]
    assert int(r.stdout.split()[1]) > 400_000


# ---------------------------------------------------------------------------------------------------------------------
# against repeats; one sequence; chunks and threads
# ---------------------------------------------------------------------------------------------------------------------
def test_open_filters_equal_repeats_on_golden_files():
    used = 0
    for name in GOLDEN_FILES:
        f = SufrFile(EXP / name)
        if f.seed_mask:
            continue
        for kind, ml, mc, xc in ((0, 1, 2, 0), (1, 2, 2, 0), (2, 1, 2, 0), (0, 3, 3, 9)):
            want = f.repeats(kind, ml, mc, xc)
            got = f.shared(kind, ml, mc, xc)
            for i in range(3):
                assert got[i].dtype == np.uint64 and np.array_equal(got[i], want[i]), (name, kind, ml, i)
            assert {k: v for k, v in got[4].items() if k != "max_seqs"} == want[3], (name, kind, ml)
            assert got[3].size == want[0].size and (got[3] >= 1).all() and (got[3] <= np.minimum(got[1], f.num_sequences)).all()
            assert got[4]["max_seqs"] == (int(got[3].max()) if got[3].size else 0)
        common = f.common()
        assert common.size == f.num_sequences and int(common[0]) == f.repeats(0, 1)[3]["longest"] and (np.diff(common.astype(np.int64)) <= 0).all()
        # the longest common substring of all sequences, and the private repeats
        assert f.shared(0, 1, min_seqs=f.num_sequences)[4]["longest"] == int(common[-1])
        all_recs = f.shared(0, 1)
        private = f.shared(0, 1, max_seqs=1)
        assert np.array_equal(private[0], all_recs[0][all_recs[3] == 1]) and (private[3] == 1).all()
        used += 1
    assert used >= 10


def test_one_sequence():
    for name in ("1.sufr", "abba.sufr", "long_dna_sequence.sufr"):
        f = SufrFile(EXP / name)
        assert f.num_sequences == 1
        rank, count, length, seqs, st = f.shared(0, 1)
        assert seqs.size == st["records"] > 0 and (seqs == 1).all() and st["max_seqs"] == 1
        assert f.common().tolist() == [st["longest"]]
        assert f.shared(0, 1, min_seqs=2)[4] == NOTHING and f.shared(0, 1, min_seqs=2)[0].size == 0


def test_chunks_threads_and_counts_on_a_larger_text(oracle, tmp_path):
    """150 000 symbols in five sequences with planted repeats: more than two chunks of the host passes, pairs and intervals
    that cross chunk ends, any number of workers; seqs against per-sequence prefix counts in numpy"""
    rng = np.random.default_rng(11)
    body = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 150_000)].copy()
    body[20_000:90_000] = ord("A")
    for at in range(100_000, 140_000, 4_000):
        body[at:at + 300] = body[95_000:95_300]
    body[[30_000, 60_000, 99_000, 120_000]] = ord("%")
    f = oracle_file(oracle, tmp_path, body, is_dna=True, threads=4)
    assert f.num_sequences == 5 and f.len_suffixes > 1 << 17
    D = docs_of(f)
    cum = np.stack([np.concatenate([[0], np.cumsum(D == d)]) for d in range(5)])
    for kind, ml, mq, xq in ((0, 12, 0, 0), (1, 12, 2, 0), (0, 250, 0, 1), (0, 12, 3, 3)):
        want = f.shared(kind, ml, min_seqs=mq, max_seqs=xq, threads=1)
        a, b = want[0].astype(np.int64), (want[0] + want[1]).astype(np.int64)
        assert want[4]["records"] > 0 and np.array_equal(want[3], ((cum[:, b] - cum[:, a]) > 0).sum(axis=0))
        rep = f.repeats(kind, ml)
        keep = np.ones(rep[0].size, dtype=bool)
        full = ((cum[:, (rep[0] + rep[1]).astype(np.int64)] - cum[:, rep[0].astype(np.int64)]) > 0).sum(axis=0)
        keep = (full >= mq) & ((xq == 0) | (full <= xq))
        assert np.array_equal(want[0], rep[0][keep]) and np.array_equal(want[2], rep[2][keep])
        for threads in (0, 2, 7):
            got = f.shared(kind, ml, min_seqs=mq, max_seqs=xq, threads=threads)
            assert all(np.array_equal(got[i], want[i]) for i in range(4)) and got[4] == want[4]
    c1 = f.common(threads=1)
    assert c1[0] > 20_000 and all(np.array_equal(f.common(threads=t), c1) for t in (0, 3))
    rep = f.repeats(0, 1)
    full = ((cum[:, (rep[0] + rep[1]).astype(np.int64)] - cum[:, rep[0].astype(np.int64)]) > 0).sum(axis=0)
    assert c1.tolist() == [int(rep[2][full >= q].max()) if (full >= q).any() else 0 for q in range(1, 6)]


# ---------------------------------------------------------------------------------------------------------------------
# capacity, refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_capacity_and_counting_calls():
    f = SufrFile(EXP / "uniprot.sufr")
    L = sufr_amd.lib()
    want = f.shared(1, 3, min_seqs=2)
    n = want[4]["records"]
    assert n > 10
    total, st = C.c_uint64(0), sufr_amd.SharedStats()
    args = (f._h, 1, 3, 0, 0, 2, 0)
    assert L.sufr_file_shared(*args, 0, None, None, None, None, C.byref(total), C.byref(st), 1) == -5      # the counting call
    assert total.value == n and st.as_dict() == want[4]
    out = [np.full(n + 3, FF, dtype=np.uint64) for _ in range(4)]
    total.value = 0
    assert L.sufr_file_shared(*args, n - 1, *(a.ctypes.data for a in out), C.byref(total), None, 1) == -5
    assert total.value == n and all((a == FF).all() for a in out)                                          # nothing written
    assert L.sufr_file_shared(*args, n + 3, *(a.ctypes.data for a in out), C.byref(total), None, 1) == 0
    for i in range(4):
        assert np.array_equal(out[i][:n], want[i]) and (out[i][n:] == FF).all()
    assert L.sufr_file_shared(f._h, 0, 1 << 40, 0, 0, 0, 0, 0, None, None, None, None, C.byref(total), C.byref(st), 1) == 0
    assert total.value == 0 and st.as_dict() == NOTHING
    assert L.sufr_file_shared(f._h, 0, 1, 0, 0, f.num_sequences + 1, 0, 0, None, None, None, None, C.byref(total), C.byref(st), 1) == 0
    assert total.value == 0 and st.as_dict() == NOTHING
    assert L.sufr_file_shared(None, 0, 1, 0, 0, 0, 0, 0, None, None, None, None, None, None, 1) == -1
    assert L.sufr_file_common(None, None, 1) == -1 and L.sufr_file_common(f._h, None, 1) == -1


def test_refusals(oracle, tmp_path):
    f = SufrFile(EXP / "uniprot-masked.sufr")
    assert f.seed_mask
    g = oracle_file(oracle, tmp_path, synth.adversarial("tandem", 600, seed=3)[:-1], is_dna=True, max_query_len=6)
    assert g.max_query_len == 6
    for h in (f, g):
        for call in (lambda: h.shared(0, 3), lambda: h.shared(0, 0), lambda: h.common()):
            with pytest.raises(SufrHipError) as e:
                call()
            assert e.value.code == -6
    h = SufrFile(EXP / "3.sufr")
    for call in (lambda: h.shared(0, 0), lambda: h.shared(3, 1), lambda: h.shared(0, 1, min_seqs=3, max_seqs=2)):
        with pytest.raises(SufrHipError) as e:
            call()
        assert e.value.code == -1
    assert h.shared(0, 1, min_seqs=2, max_seqs=2)[4]["records"] > 0


def test_bad_starts_and_empty_arrays(tmp_path):
    f = SufrFile(EXP / "3.sufr")
    for i, bad in enumerate(([1, 5], [0, 9, 5], [0, f.text_len])):
        g = _rewrite(f, tmp_path / f"bad{i}.sufr", bad)
        for call in (lambda: g.shared(0, 1), lambda: g.common()):
            with pytest.raises(SufrHipError) as e:
                call()
            assert e.value.code == -1, bad
    none = _rewrite(f, tmp_path / "none.sufr", [0, 3], sa=np.zeros(0, dtype=np.uint32), lcp=np.zeros(0, dtype=np.uint32))
    assert none.len_suffixes == 0
    for kind in KINDS:
        out = none.shared(kind, 1)
        assert all(a.size == 0 for a in out[:4]) and out[4] == NOTHING
    assert none.common().tolist() == [0, 0]


# ---------------------------------------------------------------------------------------------------------------------
# sufr shared
# ---------------------------------------------------------------------------------------------------------------------
def shared_text(f: SufrFile, recs, stats, max_positions=16):
    sa = np.asarray(f.suffix_array).astype(np.int64)
    starts = np.array(f.sequence_starts, dtype=np.int64)
    lines = []
    for a, c, ln, q in zip(*recs):
        pos = sorted(sa[int(a):int(a) + int(c)].tolist())
        shown = pos[:max_positions] if max_positions else pos
        where = []
        for p in shown:
            i = int(np.searchsorted(starts, p, side="right")) - 1
            where.append(f"{f.sequence_names[i]}:{p - int(starts[i])}")
        lines.append(f"{int(ln)}\t{int(c)}\t{int(q)}\t" + " ".join(where))
    lines += [f"# {key}\t{stats[key]}" for key in ("records", "longest", "longest_rank", "max_count", "max_seqs")]
    return "\n".join(lines) + "\n"


def test_cli_shared_prints_the_python_records(tmp_path):
    for name in ("2.sufr", "3.sufr", "uniprot.sufr"):
        f = SufrFile(EXP / name)
        assert run("shared", "--common", EXP / name).stdout == "".join(f"{q + 1}\t{int(v)}\n" for q, v in enumerate(f.common()))
        got = f.shared(0, 3, min_seqs=2)
        assert got[4]["records"] > 0
        assert run("shared", "-q", 2, "-l", 3, EXP / name).stdout == shared_text(f, got[:4], got[4])
    f = SufrFile(EXP / "3.sufr")
    for kind, kname in ((1, "maximal"), (2, "super")):
        got = f.shared(kind, 1, 2, 9, 1, 2)
        out = tmp_path / "s.tsv"
        assert run("shared", "-l", 1, "-c", 2, "-C", 9, "--min-seqs", 1, "--max-seqs", 2, "--kind", kname, "--max-positions", 2, "-o", out,
                   EXP / "3.sufr").stdout == ""
        assert out.read_text() == shared_text(f, got[:4], got[4], 2)
    r = run("shared", "-l", 3, EXP / "uniprot-masked.sufr", check=False)
    assert r.returncode == 1 and r.stderr.startswith("Error: ") and "seed mask" in r.stderr
    assert run("shared", "--common", EXP / "uniprot-masked.sufr", check=False).returncode == 1
    assert run("shared", EXP / "3.sufr", check=False).returncode == 2                # no -l
    assert run("shared", "-l", 3, "--kind", "tandem", EXP / "3.sufr", check=False).returncode == 2
    assert run("shared", "-l", 3, "-q", 3, "--max-seqs", 2, EXP / "3.sufr", check=False).returncode == 2
    assert run("shared", "-l", 3, "--min-seq", 2, EXP / "3.sufr", check=False).returncode == 2
    assert run("shared", "-l", 3, "-q", check=False).returncode == 2
    assert "shared " in run("--help").stdout


def test_cli_shared_without_records():
    assert run("shared", "-l", 100000, "-q", 2, EXP / "uniprot.sufr").stdout == \
        "# records\t0\n# longest\t0\n# longest_rank\t0\n# max_count\t0\n# max_seqs\t0\n"
