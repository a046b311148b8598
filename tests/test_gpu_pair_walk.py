"""The pair path in front of the tie level (sufr_launch.inc: tie_level): tie runs of exactly two
suffixes -- the two copies of a duplication -- are listed from the tie bitmaps and compared directly from character K on
(k_pair_walk), instead of being packed, keyed and ranked; a pair that does not part within WALK_CAP = 4096 characters is handed
back to the tie level.  `Context.set_pair_walk(1)` takes the path whatever the share of pairs, `(2)` never does, `(0)` decides by
the share; `Context.pairs_walked` says what the last build did.

Every case: whole SA and LCP equal the CPU oracle's with the path taken and with the path off, in one context, and the two builds
give the same arrays; the outputs are zero-filled before every build.  Texts of 30 000 - 100 000 symbols: a leaf window fills and
tie runs cross the 128-rank windows of the bitmaps."""
import functools

import numpy as np
import pytest
import torch

import sufr_amd
from sufr_amd import synth

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
WALK_CAP = 4096


def _acgt(rng, n):
    return ACGT[rng.integers(0, 4, n)].copy()


def _mutate(rng, seg, rate):
    """substitutions (always another base) at `rate` of the positions"""
    out = seg.copy()
    at = np.nonzero(rng.random(seg.size) < rate)[0]
    out[at] = ACGT[(np.searchsorted(ACGT, out[at]) + rng.integers(1, 4, at.size)) % 4]
    return out


@functools.lru_cache(maxsize=None)
def text(name):
    rng = np.random.default_rng({"subst": 1, "exact": 2, "tail": 3, "triples": 4, "nruns": 5, "few": 6, "protein": 7}[name])
    if name == "subst":                 # one 5 000-symbol segment copied at 1 % substitutions: walks of 0, 1, 2 and 3+ round trips
        t = _acgt(rng, 100_000)
        t[70_000:75_000] = _mutate(rng, t[10_000:15_000], 0.01)
    elif name == "exact":               # an exact copy of 10 000 symbols: pairs that share more than WALK_CAP characters
        t = _acgt(rng, 100_000)
        t[60_000:70_000] = t[20_000:30_000]
    elif name == "tail":                # the last 3 000 symbols repeat an earlier stretch: the later suffix of a pair ends first
        t = _acgt(rng, 40_000)
        t[-3_000:] = t[5_000:8_000]
    elif name == "triples":             # three copies of 2 000 symbols, a different base in front of and behind each copy:
        t = _acgt(rng, 50_000)          # every tie run has three members, at the segment's ends too
        seg = t[4_000:6_000].copy()
        for k, at in enumerate((4_000, 20_000, 36_000)):
            t[at:at + 2_000] = seg
            t[at - 1] = ACGT[k]; t[at + 2_000] = ACGT[k]
    elif name == "few":                 # the triples, and one copied stretch of 100 symbols: few pairs among the tie records
        t = text("triples")[:-1].copy()
        t[45_000:45_100] = t[12_000:12_100]
    elif name == "nruns":               # two copies of 500 symbols, each followed by 6 000 N and a tail of its own
        seg = _acgt(rng, 500)
        t = np.concatenate([_acgt(rng, 9_000), seg, np.full(6_000, ord("N"), np.uint8), _acgt(rng, 9_000),
                            seg, np.full(6_000, ord("N"), np.uint8), _acgt(rng, 9_000)])
    elif name == "protein":             # a 20-letter text with a copied stretch: 5-bit codes, no packed stream -- the byte walk
        aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
        t = aa[rng.integers(0, 20, 60_000)].copy()
        seg = t[8_000:11_000].copy()
        at = np.nonzero(rng.random(seg.size) < 0.01)[0]
        seg[at] = aa[rng.integers(0, 20, at.size)]
        t[40_000:43_000] = seg
    raw = np.concatenate([t, np.frombuffer(b"$", dtype=np.uint8)])
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def oracle():
    from oracle_helper import Oracle
    return Oracle()


def want(raw, *, is_dna=True, allow_ambiguity=False, ignore_softmask=False):
    osa, olcp, _ = oracle().build(oracle().normalize(np.ascontiguousarray(raw), ignore_softmask), is_dna=is_dna,
                                  allow_ambiguity=allow_ambiguity, threads=8)
    return osa, olcp


def build(db, x, mode, *, shards=1, **kw):
    """one build (all shards behind one another) into zero-filled outputs -> SA, LCP, (resolved, left_tied) summed, shard sizes"""
    db.ctx.set_pair_walk(mode)
    sas, lcps, res, left = [], [], 0, 0
    for k in range(shards):
        out_sa = torch.zeros(x.numel(), dtype=torch.int32, device=x.device)
        out_lcp = torch.zeros(x.numel(), dtype=torch.int32, device=x.device)
        sa, lcp = db.sort(x, raw_text=True, shard_index=k, num_shards=shards, out_sa=out_sa, out_lcp=out_lcp, **kw)
        r, l = db.ctx.pairs_walked
        res += r; left += l
        sas.append(sa.cpu().numpy().view(np.uint32).copy()); lcps.append(lcp.cpu().numpy().view(np.uint32).copy())
    return np.concatenate(sas), np.concatenate(lcps), (res, left), [p.size for p in sas]


def on_and_off(db, raw, osa, olcp, what, *, shards=1, **kw):
    """the path always, then never: the oracle's arrays both times -> (resolved, left_tied) of the build that took it"""
    from test_gpu_overlap import same
    x = torch.from_numpy(np.array(raw)).cuda()
    on = build(db, x, 1, shards=shards, **kw)
    print(f"{what}: pairs resolved {on[2][0]}, handed back {on[2][1]}, deep records {db.stats.deep_records}")
    same(on, osa, olcp, what + ", pair path on", on[3] if shards > 1 else None)
    off = build(db, x, 2, shards=shards, **kw)
    assert off[2] == (0, 0), f"{what}: set_pair_walk(2) and pairs were walked: {off[2]}"
    same(off, osa, olcp, what + ", pair path off", off[3] if shards > 1 else None)
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1]), f"{what}: the path on and off give different arrays"
    return on[2]


@pytest.fixture()
def db():
    d = sufr_amd.DeviceBuilder(0)
    yield d
    d.ctx.set_pair_walk(0)
    d.close()


def test_setter_and_getter(db):
    assert db.ctx.pairs_walked == (0, 0)
    with pytest.raises(sufr_amd.SufrHipError):
        db.ctx.set_pair_walk(3)
    db.ctx.set_pair_walk(0)


def test_duplicate_with_substitutions(db):
    raw = text("subst")
    osa, olcp = want(raw)
    # the walks this text asks for: common prefixes of the pairs beyond the K = 21 key characters, in round trips of 61 symbols
    trips = (olcp[olcp > 21].astype(np.int64) - 21) // 61
    assert {0, 1, 2}.issubset(set(trips.tolist())) and trips.max() >= 3
    resolved, left = on_and_off(db, raw, osa, olcp, "duplicate at 1 %", is_dna=True)
    assert resolved > 0 and left == 0


def test_exact_duplicate_longer_than_the_cap(db):
    raw = text("exact")
    osa, olcp = want(raw)
    assert olcp.max() > WALK_CAP + 21
    resolved, left = on_and_off(db, raw, osa, olcp, "exact duplicate of 10 000", is_dna=True)
    assert left > 0 and resolved > 0               # (the copies' last 4 096 suffixes part within the cap)


@pytest.mark.parametrize("name", ["two_identical", "tail"])
def test_ends_of_sequences(db, name):
    """pairs in which one suffix ends first: at '$', and '%' against '$'"""
    raw = synth.adversarial("two_identical", 40_000) if name == "two_identical" else text("tail")
    osa, olcp = want(raw)
    resolved, _ = on_and_off(db, raw, osa, olcp, name, is_dna=True)
    assert resolved > 0


def test_triples_have_no_pairs(db):
    raw = text("triples")
    osa, olcp = want(raw)
    resolved, left = on_and_off(db, raw, osa, olcp, "three copies", is_dna=True)
    assert (resolved, left) == (0, 0)


def test_pairs_that_run_into_n(db):
    """--dna -a: both members of every pair continue with 6 000 N -- more than the cap: all handed back, crossed by run keys"""
    raw = text("nruns")
    osa, olcp = want(raw, allow_ambiguity=True)
    resolved, left = on_and_off(db, raw, osa, olcp, "copies in front of N runs", is_dna=True, allow_ambiguity=True)
    assert left > 0


def test_ignore_softmask(db):
    raw = np.array(text("subst"))
    # half of the text in lower case, between the two copies: its suffixes are left out, the comparisons of the others read it
    raw[20_000:70_000] = raw[20_000:70_000] | 0x20
    osa, olcp = want(raw, ignore_softmask=True)
    resolved, _ = on_and_off(db, raw, osa, olcp, "ignore_softmask", is_dna=True, ignore_softmask=True)
    assert resolved > 0


def test_two_shards(db):
    raw = text("subst")
    osa, olcp = want(raw)
    resolved, _ = on_and_off(db, raw, osa, olcp, "two shards", shards=2, is_dna=True)
    assert resolved > 0


def test_listed_bytes(db):
    raw = np.array(text("subst"))
    raw[[10_700, 12_400, 73_900]] = np.frombuffer(b"RYK", dtype=np.uint8)     # inside the segment and inside its copy
    osa, olcp = want(raw)
    resolved, _ = on_and_off(db, raw, osa, olcp, "three IUPAC bytes", is_dna=True)
    assert resolved > 0 and db.stats.num_exceptions == 3


def test_protein_text(db):
    raw = text("protein")
    osa, olcp = want(raw, is_dna=False)
    resolved, _ = on_and_off(db, raw, osa, olcp, "protein", is_dna=False)
    assert resolved > 0 and db.stats.bits_per_char == 5


def test_capped_build_does_not_take_the_path(db):
    from test_gpu_mql_fast import canonical
    from test_gpu_overlap import same
    raw = text("subst")
    wsa, wlcp = canonical(*want(raw), 16)
    x = torch.from_numpy(np.array(raw)).cuda()
    for mode in (1, 2):
        got = build(db, x, mode, is_dna=True, max_query_len=16)
        assert got[2] == (0, 0)
        same(got, wsa, wlcp, f"max_query_len=16, mode {mode}")


def test_default_mode_decides_by_the_share_of_pairs(db):
    from test_gpu_overlap import same
    for name, taken in (("few", False), ("subst", True)):
        raw = text(name)
        osa, olcp = want(raw)
        got = build(db, torch.from_numpy(np.array(raw)).cuda(), 0, is_dna=True)
        same(got, osa, olcp, f"default mode, text {name}")
        assert (got[2][0] > 0) == taken, f"text {name}: pairs resolved {got[2]}"
