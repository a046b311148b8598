"""The two chains below the MSD levels side by side (sufr_launch.inc): the buckets whose suffixes agree on
all K key characters ("left-over" buckets) go through their re-keying levels on a helper pipeline -- a stream and a host thread of
its own -- while the build's pipeline takes the runs of equal keys; prefix doubling, which reads the ranks of ALL suffixes, joins
the helper first.  A build takes that path from 2^22 left-over records on; `Context.set_overlap_min(1)` sends these small texts
down it, and `Context.overlapped` / `Context.doublings` say what a build did.

Every case: whole SA and LCP equal the CPU oracle's, with the chains side by side (helper getter 1) and one after the other
(`set_overlap_min(2**64 - 1)`, helper getter 0), in the same context; the outputs are zero-filled before every build, so a rank
that is read before it was written is a valid position and shows as a wrong array.

The text: ~1.2 M symbols of random ACGT with
  * F, one exact unit of 60 bp, 6 000 times (random spacers between the copies): the suffixes that start in the unit's first
    40 symbols form ~40 buckets of 6 000 records and more -- above LEAF_BIG = 4 096 -- that agree on all 21 key characters;
  * S, a segment of 2 000 bp, 300 times (the recipe of test_many_copies_of_a_long_repeat): tie groups of 300 that stall the levels,
    so prefix doubling takes them over.  S holds five copies of F's unit: position p + d of a tied suffix lies in a left-over bucket.
A run of 6 000 'A' near the start gives the capped build -m 16 a bucket of its own kind (text_a).  4 300 of F's copies lie in the first 400 000 symbols, so that the first 420 000-symbol window of the windowed build has buckets
above LEAF_BIG too (6 000 copies spread evenly would leave ~2 600 per window: no window would reach the helper)."""
import functools

import numpy as np
import pytest
import torch

import sufr_amd

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
NEVER = 2**64 - 1


def _spaced(rng, pieces):
    out = []
    for p in pieces:
        out.append(p)
        out.append(ACGT[rng.integers(0, 4, int(rng.integers(8, 40)))])
    return out


@functools.lru_cache(maxsize=None)
def text_a():
    """(raw text, positions of F's stand-alone copies, positions of S's copies)"""
    rng = np.random.default_rng(2206)
    F = ACGT[rng.integers(0, 4, 60)]
    S = ACGT[rng.integers(0, 4, 2000)].copy()
    for at in (200, 600, 1000, 1400, 1800):
        S[at:at + 60] = F
    head = _spaced(rng, [F] * 4300)
    rest = [F] * 1700 + [S] * 300 + [ACGT[rng.integers(0, 4, 2000)] for _ in range(45)]
    order = rng.permutation(len(rest))
    tail = _spaced(rng, [rest[i] for i in order])
    # (a capped build keeps L characters and, below them, the top of the complemented position: only records whose positions
    # share those bits agree on the whole key -- -m 16: one aligned block of 65 536 positions.  A run of 6 000 'A' inside the
    # first block gives it one bucket above LEAF_BIG; the exact build takes A^21 as one more left-over bucket)
    parts = [ACGT[rng.integers(0, 4, 3000)], np.full(6000, ord("A"), np.uint8)] + head + tail + [np.frombuffer(b"$", dtype=np.uint8)]
    f_at, s_at, at = [], [], 0
    for p in parts:
        if p is F: f_at.append(at)
        if p is S: s_at.append(at)
        at += p.size
    raw = np.concatenate(parts)
    raw.setflags(write=False)
    assert len(f_at) == 6000 and len(s_at) == 300 and sum(a < 400_000 for a in f_at) >= 4300 and raw.size <= 2_500_000
    return raw, np.asarray(f_at), np.asarray(s_at)


@functools.lru_cache(maxsize=None)
def text_b():
    """text (a), then one bucket T^21 of at least RG_MIN_SIZE = 2^20 records: runs of T of 21 .. 599 symbols in random ACGT, the
    recipe of test_buckets_of_one_repeated_symbol_equal_oracle (a run of r symbols gives r - 20 records; ~290 each on average)"""
    rng = np.random.default_rng(2207)
    a = text_a()[0][:-1]
    lens = rng.integers(21, 600, 4300)
    assert int((lens - 20).sum()) >= (1 << 20) + 50_000
    parts = [a]
    for ln in lens.tolist():
        gap = ACGT[rng.integers(0, 4, int(rng.integers(2, 12)))].copy()
        gap[0] = ACGT[rng.integers(0, 3)]; gap[-1] = ACGT[rng.integers(0, 3)]      # (a run ends where it is said to)
        parts.append(gap); parts.append(np.full(ln, ord("T"), np.uint8))
    parts.append(np.frombuffer(b"A$", dtype=np.uint8))
    raw = np.concatenate(parts)
    raw.setflags(write=False)
    assert raw.size <= 2_600_000
    return raw


@functools.lru_cache(maxsize=None)
def text_d():
    """text (a) with 30 bytes replaced by R and Y: 12 inside copies of S (in front of, inside and behind the copies of F's unit in
    them), 12 inside stand-alone copies of F, 6 in the random stretches"""
    raw, f_at, s_at = text_a()
    raw = raw.copy()
    rng = np.random.default_rng(2208)
    at = [int(s_at[k]) + off for k, off in zip(rng.choice(300, 12, replace=False), (5, 150, 199, 230, 640, 999, 1003, 1390, 1500, 1799, 1861, 1999))]
    at += [int(f_at[k]) + int(off) for k, off in zip(rng.choice(6000, 12, replace=False), rng.integers(0, 60, 12))]
    at += [int(x) for x in rng.choice(2900, 6, replace=False)]
    assert len(set(at)) == 30
    raw[at] = np.frombuffer(b"RY", dtype=np.uint8)[rng.integers(0, 2, 30)]
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def want(name, allow_ambiguity=False):
    """the oracle's arrays of a text of this module: computed once, shared by the tests (here and in test_gpu_concurrent.py)"""
    from oracle_helper import Oracle
    raw = {"a": lambda: text_a()[0], "b": text_b, "d": text_d}[name]()
    osa, olcp, _ = Oracle().build(raw, is_dna=True, allow_ambiguity=allow_ambiguity, threads=8)
    osa.setflags(write=False); olcp.setflags(write=False)
    return osa, olcp


def build(db, x, *, overlap_min, shards=1, **kw):
    """one build (all shards behind one another) into zero-filled outputs -> SA, LCP, what the chains did, shard sizes, stats"""
    db.ctx.set_overlap_min(overlap_min)
    dt = torch.int64 if kw.get("index_width") == 8 else torch.int32
    sas, lcps, seen = [], [], []
    for k in range(shards):
        out_sa = torch.zeros(x.numel(), dtype=dt, device=x.device)
        out_lcp = torch.zeros(x.numel(), dtype=dt, device=x.device)
        sa, lcp = db.sort(x, raw_text=True, is_dna=True, shard_index=k, num_shards=shards, out_sa=out_sa, out_lcp=out_lcp, **kw)
        seen.append((db.ctx.overlapped, db.ctx.doublings))
        sas.append(sa.cpu().numpy().astype(np.uint32)); lcps.append(lcp.cpu().numpy().astype(np.uint32))
    return np.concatenate(sas), np.concatenate(lcps), seen, [p.size for p in sas]


def same(got, osa, olcp, what, sizes=None):
    gsa, glcp = got[0], got[1]
    assert gsa.size == osa.size, f"{what}: {gsa.size} suffixes, the oracle has {osa.size}"
    bad = np.nonzero(gsa != osa)[0]
    assert bad.size == 0, f"{what}: SA differs at rank {bad[0]} of {osa.size}: got {gsa[bad[0]]} want {osa[bad[0]]} ({bad.size} ranks differ)"
    keep = np.ones(osa.size, dtype=bool)
    if sizes is not None:
        starts = np.cumsum(sizes[:-1])
        keep[starts[starts < osa.size]] = False                    # (a shard's first LCP is the stitch's)
    bad = np.nonzero((glcp != olcp) & keep)[0]
    assert bad.size == 0, f"{what}: LCP differs at rank {bad[0]} of {osa.size}: got {glcp[bad[0]]} want {olcp[bad[0]]} ({bad.size} ranks differ)"


def both_orders(db, x, osa, olcp, what, *, shards=1, doubling=None, helper=1, **kw):
    """side by side, then one after the other: the same arrays, the oracle's.  doubling: True / False = the build must / must not
    enter prefix doubling (in every shard)"""
    side = build(db, x, overlap_min=1, shards=shards, **kw)
    print(f"{what}: side by side (helper, doublings) per shard {side[2]}, levels {db.stats.num_levels}, deep records {db.stats.deep_records}")
    assert all(h == helper for h, _ in side[2]), f"{what}: the left-over chain on the helper? want {helper}, got (helper, doublings) {side[2]}"
    if doubling is not None:
        assert all((d >= 1) == doubling for _, d in side[2]), f"{what}: entries into prefix doubling {side[2]}"
    same(side, osa, olcp, what + ", chains side by side", side[3] if shards > 1 else None)
    after = build(db, x, overlap_min=NEVER, shards=shards, **kw)
    assert all(h == 0 for h, _ in after[2]), f"{what}: set_overlap_min(2**64 - 1) and the helper ran: {after[2]}"
    assert [d for _, d in after[2]] == [d for _, d in side[2]]
    assert np.array_equal(side[0], after[0]) and np.array_equal(side[1], after[1]), f"{what}: the two orders of the chains give different arrays"
    return side


@pytest.fixture()
def db():
    d = sufr_amd.DeviceBuilder(0)
    yield d
    d.ctx.set_overlap_min(0)
    d.ctx.set_window(0, 0)
    d.close()


def test_setter_and_getters_of_a_fresh_context(db):
    assert db.ctx.overlapped == 0 and db.ctx.doublings == 0
    rng = np.random.default_rng(1)
    raw = ACGT[rng.integers(0, 4, 50_000)].copy(); raw[-1] = ord("$")
    for m in (1, 0, NEVER):                                      # (random text: no left-over bucket, nothing to overlap, no doubling)
        build(db, torch.from_numpy(raw).cuda(), overlap_min=m)
        assert db.ctx.overlapped == 0 and db.ctx.doublings == 0


def test_overlap_and_doubling_in_one_build(db):
    """(a) the tie chain enters prefix doubling while the left-over buckets are on the helper: it must wait for their ranks.
    Three builds in a context whose rank and key buffers are larger than n and hold the values of an earlier, larger build."""
    rng = np.random.default_rng(3)
    big = ACGT[rng.integers(0, 4, 2_000_000)].copy()
    seg = ACGT[rng.integers(0, 4, 2000)]
    for k in range(300): big[5 + k * 6600:5 + k * 6600 + 2000] = seg          # (doubling: the rank buffers take 2 M entries)
    big[-1] = ord("$")
    build(db, torch.from_numpy(big).cuda(), overlap_min=1)
    assert db.ctx.doublings >= 1
    raw = text_a()[0]
    x = torch.from_numpy(raw.copy()).cuda()
    osa, olcp = want("a")
    for rep in range(3):
        got = build(db, x, overlap_min=1)
        assert got[2] == [(1, got[2][0][1])] and got[2][0][1] >= 1, f"build {rep}: (helper, doublings) = {got[2]}"
        same(got, osa, olcp, f"build {rep}")
    both_orders(db, x, osa, olcp, "text (a)", doubling=True)
    db.ctx.set_overlap_min(0)                                    # the default threshold: far above this text's left-over records
    build(db, x, overlap_min=0)
    assert db.ctx.overlapped == 0


@pytest.mark.parametrize("amb", [False, True])
def test_with_a_run_bucket(db, amb):
    """(b) run_groups_find, the deferred run_groups_expand and doubling in one build: the run bucket's ranks are placed after the
    helper chain, and doubling reads them"""
    x = torch.from_numpy(text_b().copy()).cuda()
    osa, olcp = want("b", amb)
    both_orders(db, x, osa, olcp, f"text (b), allow_ambiguity={amb}", doubling=True, allow_ambiguity=amb)


@pytest.mark.parametrize("L", [12, 16])
def test_capped_builds(db, oracle, L):
    """(c) -m 12 / -m 16: no doubling; the left-over chain runs on the helper with position keys -- where a capped build can have
    one.  Its 64-bit key holds 3 L bits of characters and the top 64 - 3 L bits of the complemented 32-bit position, and the MSD
    levels go on over those: the records of a left-over bucket agree on all of it, so their positions lie in one aligned block of
    2^(3 L - 32) positions.  -m 16: 65 536 positions, the run of 'A' of text_a fills a bucket of 6 000.  -m 12: 16 positions -- no
    bucket can exceed LEAF_BIG, the capped build has no left-over chain at all, and the getter must say 0 for any text."""
    from test_gpu_mql_fast import canonical
    raw = text_a()[0]
    x = torch.from_numpy(raw.copy()).cuda()
    osa, olcp = want("a")
    wsa, wlcp = canonical(osa, olcp, L)
    side = both_orders(db, x, wsa, wlcp, f"text (a), max_query_len={L}", doubling=False, helper=1 if L == 16 else 0, max_query_len=L)
    # the oracle's own capped build (one member of the reference's family, test_max_query_len_canonical_form): min(LCP, L) and
    # the first L characters of every rank agree
    msa, mlcp, _ = oracle.build(raw, is_dna=True, max_query_len=L, threads=8)
    assert np.array_equal(np.minimum(mlcp, L), side[1])
    pad = np.concatenate([raw, np.zeros(L, dtype=np.uint8)])
    first = lambda sa: pad[sa.astype(np.int64)[:, None] + np.arange(L)[None, :]]
    assert np.array_equal(first(msa), first(side[0]))


@pytest.mark.parametrize("shards", [1, 2, 3])
def test_listed_bytes(db, shards):
    """(d) 30 IUPAC bytes inside copies of S and of F; the sharded builds run doubling with DblShard while the helper runs"""
    x = torch.from_numpy(text_d().copy()).cuda()
    osa, olcp = want("d")
    both_orders(db, x, osa, olcp, f"text (d), {shards} shards", shards=shards, doubling=True)
    assert db.stats.num_exceptions == 30 and db.stats.bits_per_char == 3


def test_windows(db):
    """(e) forced 32-bit windows: the window builds share the pipeline and its helper; the first window has left-over buckets"""
    x = torch.from_numpy(text_a()[0].copy()).cuda()
    osa, olcp = want("a")
    db.ctx.set_window(400_000, 20_000)
    try:
        both_orders(db, x, osa, olcp, "text (a) in windows", index_width=8)
    finally:
        db.ctx.set_window(0, 0)
