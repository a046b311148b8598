"""Paths through the leaf sort (k_leaf_sort / k_leaf_sort_lsd / leaf_finish, sufr_amd/csrc/sufr_msd.inc) at small sizes: the
DNA digest from its table with the tail-cutting characters at every offset, counting buckets of two to several hundred members
(the first-four ranking, its tail loop and the windows left to the LSD fallback), ragged last rows and windows of fewer records
than threads, the general code table (full-width keys) and a capped build (keys whose low bits hold positions).

Every case: whole SA and LCP equal the CPU oracle's.  The texts are built once."""
import functools

import numpy as np
import pytest
import torch

import sufr_amd

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
AMINO = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def text(name):
    """(text ending in '$', keyword arguments of the build)"""
    kw = dict(is_dna=True)
    if name in ("acgt", "acgt_n"):
        raw = ACGT[np.random.default_rng(21).integers(0, 4, 1_000_003)].copy()
        if name == "acgt_n":
            # single N and runs of 2-3 N about every 50 symbols (steps of 35..65: every offset within the six digest characters),
            # and 40 sequences
            rng = np.random.default_rng(22)
            at = np.cumsum(rng.integers(35, 66, raw.size // 50))
            at = at[at < raw.size - 4]
            ln = rng.integers(1, 4, at.size)
            for k in range(3):
                raw[at[ln > k] + k] = ord("N")
            raw[np.linspace(0, raw.size, 41, dtype=np.int64)[1:-1]] = ord("%")
    elif name == "repeats":
        # a two-letter half (few counting buckets, many members each), then tandem arrays of period 2-7 and 40 to 4 000 symbols
        # (equal keys by the hundred: buckets above four members, and above bmax = 256 -- the LSD fallback)
        rng = np.random.default_rng(23)
        raw = ACGT[rng.integers(0, 2, 300_000) * 2].copy()
        p = 150_000
        lengths = [40, 90, 200, 450, 1_000, 2_200, 4_000]
        while p < raw.size - 1:
            per = int(rng.integers(2, 8)); ln = min(lengths[int(rng.integers(0, len(lengths)))], raw.size - 1 - p)
            unit = ACGT[rng.integers(0, 4, per)]
            unit[0] = ACGT[(int(np.nonzero(ACGT == unit[-1])[0][0]) + 1) % 4]      # (not a homopolymer)
            raw[p:p + ln] = np.resize(unit, ln)
            p += ln
            gap = int(rng.integers(5, 60))
            raw[p:p + gap] = ACGT[rng.integers(0, 4, min(gap, raw.size - p))]
            p += gap
    elif name in ("len4097", "len70001"):
        raw = ACGT[np.random.default_rng(24).integers(0, 4, int(name[3:]))].copy()
    elif name == "protein":
        raw = AMINO[np.random.default_rng(25).integers(0, 20, 200_000)].copy(); kw = dict(is_dna=False)
    elif name == "capped":
        rng = np.random.default_rng(26)
        raw = ACGT[rng.integers(0, 4, 300_000)].copy()
        fam = ACGT[rng.integers(0, 4, 300)]
        for s in range(1_000, 290_000, 2_900):             # copies of one family: suffixes that agree on all 16 characters
            raw[s:s + 300] = fam
        kw = dict(is_dna=True, max_query_len=16)
    else:
        raise KeyError(name)
    raw[-1] = ord("$")
    raw.setflags(write=False)
    return raw, kw


def canonical(osa, olcp, cap):
    """the exact arrays -> the capped build's: runs of ranks with LCP >= cap re-ordered by descending position"""
    head = np.ones(osa.size, dtype=bool)
    head[1:] = olcp[1:] < cap
    order = np.lexsort((-osa.astype(np.int64), np.cumsum(head) - 1))
    return osa[order], np.minimum(olcp, cap).astype(np.uint32)


def equal_prefix_groups(olcp, k):
    """sizes of the groups of suffixes that agree on their first k characters (runs of ranks with LCP >= k)"""
    heads = np.nonzero(np.concatenate(([True], olcp[1:] < k)))[0]
    return np.diff(np.concatenate((heads, [olcp.size])))


def check(oracle, name, want_size):
    raw, kw = text(name)
    assert raw.size == want_size
    assert np.array_equal(oracle.normalize(raw, False), raw)
    cap = kw.get("max_query_len")
    osa, olcp, _ = oracle.build(raw, threads=8, **{k: v for k, v in kw.items() if k != "max_query_len"})
    if cap:             # the capped build's member of the reference's family, from the oracle's exact arrays (test_gpu_mql_fast)
        osa, olcp = canonical(osa, olcp, cap)
    db = sufr_amd.DeviceBuilder(0)
    try:
        sa, lcp = db.sort(torch.from_numpy(raw.copy()).cuda(), raw_text=True, **kw)
        gsa = sa.cpu().numpy().view(np.uint32); glcp = lcp.cpu().numpy().view(np.uint32)
        stats = db.stats.as_dict()
    finally:
        db.close()
    assert gsa.size == osa.size, f"{name}: {gsa.size} suffixes, want {osa.size}"
    bad = np.nonzero(gsa != osa)[0]
    assert bad.size == 0, f"{name}: SA differs at rank {bad[0]} of {osa.size}: got {gsa[bad[0]]} want {osa[bad[0]]} ({bad.size} ranks differ)"
    bad = np.nonzero(glcp != olcp)[0]
    assert bad.size == 0, f"{name}: LCP differs at rank {bad[0]} of {osa.size}: got {glcp[bad[0]]} want {olcp[bad[0]]} ({bad.size} ranks differ)"
    return raw, stats, olcp


def test_random_acgt(oracle):
    """1 000 003 symbols: several MSD levels, windows of many leaves (a digit of fewer than twelve digest bits)"""
    _, st, _ = check(oracle, "acgt", 1_000_003)
    assert st["bits_per_char"] == 3 and st["num_exceptions"] == 0


def test_acgt_with_n_and_sequences(oracle):
    """the same text with N, NN, NNN about every 50 symbols and 40 sequences: the characters that cut the digest's tail at
    every one of its six offsets, in both halves of the table"""
    raw, st, _ = check(oracle, "acgt_n", 1_000_003)
    assert int((raw == ord("%")).sum()) == 39
    s = raw.tobytes()
    assert s.count(b"NNN") > 1_000 and s.count(b"N") > 30_000
    assert st["bits_per_char"] == 3


def test_two_letters_and_tandem_repeats(oracle):
    """300 000 symbols: counting buckets of 2 to several hundred members, windows above bmax for the LSD fallback"""
    raw, st, olcp = check(oracle, "repeats", 300_000)
    assert set(np.unique(raw[:150_000]).tolist()) == {ord("A"), ord("G")}
    assert st["bits_per_char"] == 3
    # that the text still drives those paths: suffixes that agree on every character of the key have equal whole keys, so they
    # share a counting bucket whatever the digit; groups of 5 .. bmax of them run the tail loop of the ranking, a group above
    # bmax = 256 sends its window to k_leaf_sort_lsd
    groups = equal_prefix_groups(olcp, st["chars_per_key"])
    assert int(((groups > 4) & (groups <= 256)).sum()) >= 100, "no counting buckets of 5 .. 256 equal keys"
    assert int((groups > 256).sum()) >= 10 and int(groups.max()) >= 500, "no counting bucket above bmax"


@pytest.mark.parametrize("n", [4_097, 70_001])
def test_ragged_rows_and_short_windows(oracle, n):
    check(oracle, f"len{n}", n)


def test_protein_general_table(oracle):
    """twenty letters: the DNA3 = false instantiation (range-coder digest), keys that use every bit"""
    _, st, _ = check(oracle, "protein", 200_000)
    assert st["bits_per_char"] == 5 and st["alphabet_size"] == 21


def test_capped_dna_build(oracle):
    """-m 16: keys end in position bits, so whole keys differ and can have all 64 bits set; the copies of one family give runs
    of suffixes that agree on all 16 characters, which the position bits order (descending position)"""
    _, st, _ = check(oracle, "capped", 300_000)
    assert st["chars_per_key"] == 16                  # the capped build proper, not the exact build re-ordered
