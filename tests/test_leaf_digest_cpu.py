"""CPU checks of the leaf-sort helpers that host and device share (sufr_amd/csrc/sufr_runkey.h):
the DNA digest composed from the 512-entry table of halves must equal dna3_digest12 on all 2^18 inputs, and the ranking of the
members of a counting bucket (two orderings per member and its arrival rank; the first four slots read without a mask) must give the
position of every member in "sort by (key, arrival rank)"."""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
EDGE_KEYS = [0, 1, 2 ** 63 - 1, 2 ** 64 - 2, 2 ** 64 - 1]


@pytest.fixture(scope="module")
def shim():
    out = ROOT / "tests" / "_build" / "libleaf_digest_shim.so"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "leaf_digest_shim.cpp"
    hdr = ROOT / "sufr_amd" / "csrc" / "sufr_runkey.h"
    if not out.exists() or out.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(out), str(src)], check=True)
    L = C.CDLL(str(out))
    L.shim_leaf_digest_all.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.shim_leaf_half_table.argtypes = [C.c_void_p]
    L.shim_leaf_ranks.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.shim_leaf_mate_before.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]; L.shim_leaf_mate_before.restype = C.c_uint32
    L.shim_leaf_rank_first4.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64]; L.shim_leaf_rank_first4.restype = C.c_uint32
    return L


def test_table_composition_equals_the_digest_on_all_inputs(shim):
    direct = np.zeros(1 << 18, dtype=np.uint32); table = np.zeros_like(direct); high6 = np.zeros_like(direct)
    shim.shim_leaf_digest_all(direct.ctypes.data, table.ctypes.data, high6.ctypes.data)
    bad = np.nonzero(direct != table)[0]
    assert bad.size == 0, f"t = {bad[0]:#x}: digest {direct[bad[0]]:#x}, from the table {table[bad[0]]:#x} ({bad.size} inputs differ)"
    # a digit of six bits or fewer: the high lookup alone gives the top six bits
    assert np.array_equal(direct >> 6, high6 >> 6) and not (high6 & 63).any()
    assert direct.max() == 0xfff and direct[0] == 0


def test_half_table_entries(shim):
    """value in bits [5:0]; bits [13:8] are 63, or 0 where one of the three characters is pad, '$', '%' or 'N' (codes 0 1 2 6)"""
    tab = np.zeros(512, dtype=np.uint16)
    shim.shim_leaf_half_table(tab.ctypes.data)
    val = {3: 0, 4: 1, 5: 2, 7: 3}
    for x in range(512):
        chars = [(x >> 6) & 7, (x >> 3) & 7, x & 7]
        v = 0; cut = False
        for i, c in enumerate(chars):
            if cut:
                continue
            if c in val:
                v |= val[c] << (4 - 2 * i)
            else:
                v |= (3 if c == 6 else 0) << (4 - 2 * i)      # N sits at the left end of T's interval, the others at A's
                cut = True
        assert int(tab[x]) == v | ((0 if cut else 63) << 8), f"entry {x:#o}: {int(tab[x]):#x}"


def expected_ranks(keys):
    order = sorted(range(len(keys)), key=lambda a: (keys[a], a))
    want = [0] * len(keys)
    for r, a in enumerate(order):
        want[a] = r
    return want


def ranks(shim, keys):
    k = np.array(keys, dtype=np.uint64)
    out = np.zeros(len(keys), dtype=np.uint32)
    shim.shim_leaf_ranks(k.ctypes.data, len(keys), out.ctypes.data)
    return out.tolist()


def test_mate_predicate_on_the_edge_keys(shim):
    """every pair of edge keys, earlier and later arrival: (k_i, i) < (key, a) -- 2^64 - 1 against itself is where key + 1 wraps"""
    for ki, key in itertools.product(EDGE_KEYS, repeat=2):
        for i, a in [(0, 1), (1, 0), (3, 3), (2, 7), (7, 2)]:
            want = int((ki, i) < (key, a))
            assert shim.shim_leaf_mate_before(ki, key, i, a) == want, (ki, key, i, a)


def test_ranking_small_buckets_of_edge_keys_exhaustively(shim):
    """buckets of 1-5 members drawn from the edge keys, every combination with repetition, every arrival rank"""
    for sz in range(1, 6):
        for keys in itertools.product(EDGE_KEYS, repeat=sz):
            assert ranks(shim, keys) == expected_ranks(keys), keys


def test_ranking_random_buckets_with_duplicates(shim):
    """buckets of 1-9 members: random 64-bit keys, a few distinct values each so that duplicates are common, the edge keys mixed
    in; the ranks of all members (every arrival rank) are the permutation of the stable sort"""
    rng = np.random.default_rng(5)
    for trial in range(4000):
        sz = int(rng.integers(1, 10))
        pool = [int(x) for x in rng.integers(0, 2 ** 64, size=int(rng.integers(1, 4)), dtype=np.uint64)]
        pool += [EDGE_KEYS[int(j)] for j in rng.integers(0, 5, size=int(rng.integers(0, 3)))]
        near = pool[0]
        pool += [(near + 1) % 2 ** 64, (near - 1) % 2 ** 64]                  # neighbours: off-by-one orderings
        keys = [pool[int(j)] for j in rng.integers(0, len(pool), size=sz)]
        got = ranks(shim, keys)
        assert got == expected_ranks(keys), (keys, got)
        assert sorted(got) == list(range(sz))


def test_first_four_need_no_mask_for_larger_keys_past_the_bucket(shim):
    """the kernel reads four slots whatever the bucket's size, without a mask: what lies past the bucket is a key of a later
    bucket, larger than every member, or the sentinel 2^64 - 1 (which a member may equal: the test there is `less`)"""
    rng = np.random.default_rng(6)
    for sz in range(1, 5):
        for trial in range(200):
            keys = [EDGE_KEYS[int(j)] for j in rng.integers(0, 5, size=sz)]
            k = np.array(keys, dtype=np.uint64)
            want = expected_ranks(keys)
            for a in range(sz):
                for junk in {2 ** 64 - 1, min(max(keys) + 1, 2 ** 64 - 1)}:
                    assert shim.shim_leaf_rank_first4(k.ctypes.data, sz, a, junk) == want[a], (keys, a, junk)
