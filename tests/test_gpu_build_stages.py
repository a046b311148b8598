"""Paths through the stages of the plain-order build (Pipeline::sort_build, sufr_amd/csrc/sufr_launch.inc)
that the other tests reach only at large sizes or not at all: a device text that is not 16-byte aligned (the staging copy in
front of the text stage), a DNA text pass whose list of bytes outside the table is given up (two of the ways back to the general
code table), and a first digit of fewer than five characters at small-tile size (first_digit_map, count_and_shard).

Every case: whole SA and LCP equal the CPU oracle's, the text the context keeps equals the reference's normalised text, and the
stats say which path the build took.  The oracle's arrays of a text are computed once and shared by its cases."""
import functools

import numpy as np
import pytest
import torch

import sufr_amd
from test_gpu_exceptions import _context_text

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
AMINO = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
# twenty letters of which two stand in the DNA table {$ % A C G N T}: 18 of 20 bytes of a random text lie outside it
MOSTLY_OUTSIDE = np.frombuffer(b"ACBDEFHIJKLMOPQRSUVW", dtype=np.uint8)
IUPAC = np.frombuffer(b"RYKMSWBDHV", dtype=np.uint8)
EXC_MAX_LIST = 1 << 20            # bytes outside the table a DNA build lists (sufr_launch.inc)


@functools.lru_cache(maxsize=None)
def text(name):
    """(raw text ending in '$', keyword arguments of the build)"""
    if name == "dna":
        raw = ACGT[np.random.default_rng(11).integers(0, 4, 70_001)].copy(); kw = dict(is_dna=True)
    elif name == "iupac":
        rng = np.random.default_rng(12)
        raw = ACGT[rng.integers(0, 4, 70_001)].copy(); kw = dict(is_dna=True)
        raw[rng.choice(70_000, 20, replace=False)] = IUPAC[rng.integers(0, 10, 20)]
    elif name == "protein":
        raw = AMINO[np.random.default_rng(13).integers(0, 20, 70_001)].copy(); kw = dict(is_dna=False)
    elif name == "amino_as_dna":
        raw = AMINO[np.random.default_rng(14).integers(0, 20, 1_200_000)].copy(); kw = dict(is_dna=True)
    elif name == "outside_as_dna":
        raw = MOSTLY_OUTSIDE[np.random.default_rng(15).integers(0, 20, 1_200_000)].copy(); kw = dict(is_dna=True)
    elif name == "six_symbols":
        raw = np.frombuffer(b"%ACGNT", dtype=np.uint8)[np.random.default_rng(16).integers(0, 6, 200_000)].copy()
        kw = dict(is_dna=True, allow_ambiguity=True)
    else:
        raise KeyError(name)
    raw[-1] = ord("$")
    raw.setflags(write=False)
    return raw, kw


@functools.lru_cache(maxsize=None)
def want(name):
    """the oracle's arrays of a text of this module (upper-case texts: normalising leaves them as they are)"""
    from oracle_helper import Oracle
    raw, kw = text(name)
    o = Oracle()
    assert np.array_equal(o.normalize(raw, False), raw)
    osa, olcp, _ = o.build(raw, threads=8, **kw)
    osa.setflags(write=False); olcp.setflags(write=False)
    return osa, olcp


def outside(raw):
    return int((~np.isin(raw, np.frombuffer(b"$%ACGNT", dtype=np.uint8))).sum())


def same(gsa, glcp, osa, olcp, what, skip_lcp_at=()):
    assert gsa.size == osa.size, f"{what}: {gsa.size} suffixes, want {osa.size}"
    bad = np.nonzero(gsa != osa)[0]
    assert bad.size == 0, f"{what}: SA differs at rank {bad[0]} of {osa.size}: got {gsa[bad[0]]} want {osa[bad[0]]} ({bad.size} ranks differ)"
    keep = np.ones(osa.size, dtype=bool)
    keep[[r for r in skip_lcp_at if r < osa.size]] = False
    bad = np.nonzero((glcp != olcp) & keep)[0]
    assert bad.size == 0, f"{what}: LCP differs at rank {bad[0]} of {osa.size}: got {glcp[bad[0]]} want {olcp[bad[0]]} ({bad.size} ranks differ)"


def build(db, x, **kw):
    """one build into zero-filled outputs through the 64-bit entry point (the context keeps its text: _context_text) -> SA, LCP"""
    out_sa = torch.zeros(x.numel(), dtype=torch.int64, device="cuda"); out_lcp = torch.zeros(x.numel(), dtype=torch.int64, device="cuda")
    sa, lcp = db.sort(x, raw_text=True, index_width=8, out_sa=out_sa, out_lcp=out_lcp, **kw)
    return sa.cpu().numpy().astype(np.uint32), lcp.cpu().numpy().astype(np.uint32)


def build_at_offset(db, raw, offset, **kw):
    """the text `offset` bytes into a device buffer (allocations are aligned to 256 bytes and more) -> SA, LCP, the context's text"""
    buf = torch.zeros(raw.size + offset, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    x = buf[offset:]
    x.copy_(torch.from_numpy(raw.copy()))
    assert x.data_ptr() % 16 == offset % 16 and x.is_contiguous()
    return build(db, x, **kw) + (_context_text(db.ctx, raw.size),)


@pytest.fixture()
def db():
    d = sufr_amd.DeviceBuilder(0)
    yield d
    d.close()


@pytest.mark.parametrize("offset", [1, 7])
@pytest.mark.parametrize("name", ["dna", "iupac", "protein"])
def test_misaligned_device_text(db, name, offset):
    """a text pointer that is not 16-byte aligned is staged into the workspace first: through the DNA table, the listed bytes
    (the context's text carries the letters afterwards, not the 'N' of the build) and the general table"""
    raw, kw = text(name)
    assert raw.size == 70_001
    osa, olcp = want(name)
    gsa, glcp, got = build_at_offset(db, raw, offset, **kw)
    same(gsa, glcp, osa, olcp, f"{name} at offset {offset}")
    assert np.array_equal(got, raw), f"{name} at offset {offset}: the context's text differs at {np.nonzero(got != raw)[0][:8]}"
    st = db.stats
    if name == "dna":
        assert st.bits_per_char == 3 and st.num_exceptions == 0
    elif name == "iupac":
        assert outside(raw) == 20
        assert st.bits_per_char == 3 and st.num_exceptions == 20 and st.num_reinserted >= 1
    else:
        assert st.bits_per_char == 5 and st.alphabet_size == 21 and st.num_exceptions == 0


@pytest.mark.parametrize("soft", [False, True])
def test_misaligned_soft_masked_text_is_normalised(db, oracle, soft):
    """the staging copy together with the text map: 70 001 symbols of ACGTacgtN at offset 1.  The text pass upper-cases the
    lower-case letters or, under --ignore-softmask, writes 'N' for them; the context's text is the reference's normalised text
    and the arrays are the oracle's of that text"""
    rng = np.random.default_rng(17 + soft)
    raw = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)[rng.integers(0, 9, 70_001)].copy()
    raw[-1] = ord("$")
    norm = oracle.normalize(raw, soft)
    assert not np.array_equal(norm, raw) and ((norm == ord("N")).sum() > (raw == ord("N")).sum()) == soft
    osa, olcp, _ = oracle.build(norm, is_dna=True, threads=8)
    gsa, glcp, got = build_at_offset(db, raw, 1, is_dna=True, ignore_softmask=soft)
    assert np.array_equal(got, norm), f"the context's text differs from the normalised text at {np.nonzero(got != norm)[0][:8]}"
    same(gsa, glcp, osa, olcp, f"soft-masked text at offset 1, ignore_softmask={soft}")
    assert db.stats.bits_per_char == 3 and db.stats.num_exceptions == 0


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("name", ["amino_as_dna", "outside_as_dna"])
def test_a_dna_build_that_gives_up_its_list(db, name, offset):
    """`is_dna` on 1 200 000 random symbols of twenty letters: the text pass lists bytes outside the table by the hundred
    thousand, and the build goes back to the general code table with nothing listed.
      amino_as_dna: the amino acids.  15 of the 20 are outside the table, ~900 000 bytes: fewer than the list holds (2^20), more
        than one in 64 -- the listed bytes are put back into the normalised text and that text is counted again.
      outside_as_dna: twenty letters with 18 outside the table, ~1 080 000 bytes: more than the list holds.  The list is cut
        short, so the build starts again from the caller's text (at offset 1: through the staging copy once more)."""
    raw, kw = text(name)
    assert raw.size == 1_200_000
    if name == "amino_as_dna":
        assert raw.size // 64 < outside(raw) <= EXC_MAX_LIST
    else:
        assert outside(raw) > EXC_MAX_LIST
    osa, olcp = want(name)
    gsa, glcp, got = build_at_offset(db, raw, offset, **kw)
    same(gsa, glcp, osa, olcp, f"{name} at offset {offset}")
    assert np.array_equal(got, raw), f"{name} at offset {offset}: the context's text differs at {np.nonzero(got != raw)[0][:8]}"
    assert db.stats.num_exceptions == 0 and db.stats.bits_per_char == 5 and db.stats.alphabet_size == 21


def test_fewer_characters_per_first_digit_at_small_tile_size(db):
    """`--dna --allow-ambiguity` on 200 000 symbols drawn from %ACGNT: all 6^5 = 7 776 five-mers occur, more than the 4 096
    first digits the partition takes, so the digit drops to four characters (12 bits) -- here with the 256-thread tiles of a
    small text.  No run of 1 000 'N' occurs (the reference's shortcut for those is not in play).  One shard against the oracle;
    three shards -- their first-digit counts are sums over the raw five-character counts of the text pass -- concatenate to the
    same arrays (a shard's first LCP is the stitch's)."""
    raw, kw = text("six_symbols")
    assert raw.size == 200_000
    five = np.lib.stride_tricks.sliding_window_view(raw[:-1], 5)
    assert np.unique(five, axis=0).shape[0] == 6 ** 5
    osa, olcp = want("six_symbols")
    x = torch.from_numpy(raw.copy()).cuda()
    one_sa, one_lcp = build(db, x, **kw)
    assert db.stats.digit_bits == 12 and db.stats.bits_per_char == 3
    same(one_sa, one_lcp, osa, olcp, "one shard")
    assert np.array_equal(_context_text(db.ctx, raw.size), raw)
    sas, lcps = [], []
    for k in range(3):
        sa, lcp = build(db, x, shard_index=k, num_shards=3, **kw)
        assert db.stats.digit_bits == 12
        sas.append(sa); lcps.append(lcp)
    sizes = [p.size for p in sas]
    assert min(sizes) > 0, f"shard sizes {sizes}"
    same(np.concatenate(sas), np.concatenate(lcps), one_sa, one_lcp, "three shards", skip_lcp_at=np.cumsum(sizes[:-1]).tolist())
