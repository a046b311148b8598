"""The retry of a `--dna` build whose listed bytes (bytes outside {$ % A C G N T}; sufr_amd/csrc/sufr_exc.inc) were looked at by
more suffixes than the whole-text sort takes: the text is built again with the general code table (Pipeline::reinsert_listed,
sufr_launch.inc).  The limit is 2^22 suffixes; `Context.set_exc_max_affected` lowers it so that a text of 120 001 symbols
reaches all three comparisons of exc_reinsert that give up (`Context.exc_retry` says which one did):

  1  one shard: the ranges of positions in front of the listed bytes hold more than 16 x limit positions.  Gives up BEFORE the
     listed bytes are put back into the context's text.
  2  more than `limit` ranks were taken out of the arrays (`Context.exc_taken`).  Gives up after the bytes are back.
  3  shards: more than `limit` suffixes are left to place once the other shards' suffixes that belong here are added
     (`stats.num_reinserted` of a build that does not retry).  Also from a shard that is empty as built.

Every case: whole SA and LCP equal the CPU oracle's arrays of the true text (outputs zero-filled before the call), the text the
context keeps equals the reference's normalised text, num_suffixes is right, exc_retry has the expected value, and the stats
speak of the build that made the arrays (after a retry: nothing listed and a code wider than 3 bits; without: listed bytes on
the 3-bit table).  A rank of a sharded build that retries must still fit between its neighbours, which may not have retried:
the shards concatenate to the oracle's arrays whichever of them do.

Limits are placed from the device's own counters of a build with the default limit, never from numbers written down here."""
import functools

import numpy as np
import pytest
import torch

import sufr_amd
from test_gpu_build_stages import build, build_at_offset, same
from test_gpu_exceptions import _context_text
from test_gpu_mql_fast import canonical

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
TABLE = np.frombuffer(b"$%ACGNT", dtype=np.uint8)
N_R = 120_001
SEG_AT = [10_000 + i * 13_000 for i in range(8)]
DEFAULT_LIMIT = 1 << 22


@functools.lru_cache(maxsize=None)
def text(name):
    """R: random ACGT with one 2 000-symbol segment (its first 1 500 symbols from {A, C} only) planted eight times, the copies
    differing in the symbol at 1 500 -- R N T R Y A G K: the comparisons of ~1 500 suffixes in front of each reach it --, six
    scattered bytes in the first 9 000 positions, '$' last.  Ten listed bytes.
    R_hash: R with 600 '#' between the copies ('#' sorts below '$': under --allow-ambiguity the suffixes that start at one are
    built in the shard of 'N' and belong to shard 0).  clean: R with 'A' for every listed byte."""
    rng = np.random.default_rng(41)
    raw = ACGT[rng.integers(0, 4, N_R)].copy()
    seg = ACGT[rng.integers(0, 4, 2_000)].copy()
    seg[:1_500] = ACGT[rng.integers(0, 2, 1_500)]
    for at, c in zip(SEG_AT, b"RNTRYAGK"):
        raw[at:at + 2_000] = seg
        raw[at + 1_500] = c
    raw[rng.choice(9_000, 6, replace=False)] = np.frombuffer(b"RYKW#!", dtype=np.uint8)
    raw[-1] = ord("$")
    if name == "R_hash":
        free = np.concatenate([np.arange(at + 2_100, at + 12_900) for at in SEG_AT[:-1]])
        raw[np.random.default_rng(42).choice(free, 600, replace=False)] = ord("#")
    elif name == "clean":
        raw[~np.isin(raw, TABLE)] = ord("A")
    elif name != "R":
        raise KeyError(name)
    raw.setflags(write=False)
    return raw


def listed(raw):
    return int((~np.isin(raw, TABLE)).sum())


@functools.lru_cache(maxsize=None)
def want(name, amb):
    """the oracle's arrays of a text of this module (upper-case: normalising leaves it as it is)"""
    from oracle_helper import Oracle
    raw = text(name)
    o = Oracle()
    assert np.array_equal(o.normalize(raw, False), raw)
    osa, olcp, _ = o.build(raw, is_dna=True, allow_ambiguity=amb, threads=8)
    assert osa.size == (raw.size if amb else int(np.isin(raw, np.frombuffer(b"$ACGT", dtype=np.uint8)).sum()))
    osa.setflags(write=False); olcp.setflags(write=False)
    return osa, olcp


@functools.lru_cache(maxsize=None)
def want_capped(name, amb, L):
    wsa, wlcp = canonical(*want(name, amb), L)
    wsa.setflags(write=False); wlcp.setflags(write=False)
    return wsa, wlcp


@functools.lru_cache(maxsize=None)
def device_text(name):
    return torch.from_numpy(text(name).copy()).cuda()


@pytest.fixture()
def db():
    d = sufr_amd.DeviceBuilder(0)
    yield d
    d.ctx.set_exc_max_affected(0)
    d.ctx.set_window(0, 0)
    d.close()


def check_state(db, raw, count, retry, what):
    """what a build leaves behind beside its arrays: the reason of the retry, the stats of the build that made the arrays, the
    count, the caller's text in the context"""
    st = db.stats
    assert db.ctx.exc_retry == retry, f"{what}: exc_retry {db.ctx.exc_retry}, want {retry} (exc_taken {db.ctx.exc_taken}, num_reinserted {st.num_reinserted})"
    if retry:
        assert st.num_exceptions == 0 and st.bits_per_char > 3, f"{what}: after the retry {st.num_exceptions} listed bytes, {st.bits_per_char} bits"
    elif listed(raw):
        assert st.num_exceptions == listed(raw) and st.bits_per_char == 3, f"{what}: {st.num_exceptions} listed bytes, {st.bits_per_char} bits"
    else:
        assert st.num_exceptions == 0 and st.bits_per_char == 3 and st.num_reinserted == 0 and db.ctx.exc_taken == 0, what
    assert db.num_suffixes == count and st.num_suffixes == count, f"{what}: num_suffixes {db.num_suffixes} / {st.num_suffixes}, want {count}"
    got = _context_text(db.ctx, raw.size)
    assert np.array_equal(got, raw), f"{what}: the context's text differs at {np.nonzero(got != raw)[0][:8]}: {bytes(got[got != raw][:8])}"


def one_shard(db, name, amb, limit, retry, what, *, offset=0, cap=None):
    """text `name` as one shard under `limit` against the oracle -> SA, LCP"""
    raw = text(name)
    db.ctx.set_exc_max_affected(limit)
    kw = dict(is_dna=True, allow_ambiguity=amb)
    if cap:
        kw["max_query_len"] = cap
    if offset:
        gsa, glcp, _ = build_at_offset(db, raw, offset, **kw)
    else:
        gsa, glcp = build(db, device_text(name), **kw)
    osa, olcp = want_capped(name, amb, cap) if cap else want(name, amb)
    same(gsa, glcp, osa, olcp, what)
    check_state(db, raw, osa.size, retry, what)
    return gsa, glcp


def affected(db, name, amb, what, **kw):
    """the suffixes a build with the default limit re-places: what the limits of a case are placed around"""
    one_shard(db, name, amb, 0, 0, f"{what}, default limit", **kw)
    A = int(db.stats.num_reinserted)
    assert db.ctx.exc_taken == A, f"{what}: one shard took {db.ctx.exc_taken} ranks out and re-placed {A}"
    assert A >= 64, f"{what}: {A} suffixes re-placed"
    print(f"{what}: default limit -> (exc_retry, exc_taken, num_reinserted) = (0, {A}, {A})")
    return A


def limit_for(way, A):
    """one shard: A itself is taken, A - 1 gives up on the count of ranks (2), A // 32 on the ranges of positions already (1: they
    hold at least A positions, more than 16 x (A // 32))"""
    return {0: A, 1: A // 32, 2: A - 1}[way]


# ---- a. the boundary, one shard ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("amb", [False, True])
def test_limit_at_and_below_the_affected_count(db, amb):
    A = affected(db, "R", amb, f"R, amb={amb}")
    arrays = []
    for way in (0, 2, 1):
        arrays.append(one_shard(db, "R", amb, limit_for(way, A), way, f"R, amb={amb}, limit {limit_for(way, A)}"))
        print(f"R amb={amb} limit {limit_for(way, A)}: (exc_retry, exc_taken, num_reinserted) = ({db.ctx.exc_retry}, {db.ctx.exc_taken}, {db.stats.num_reinserted})")
        assert db.ctx.exc_taken == (0 if way == 1 else A)           # (way 1 gives up before it counts the ranks)
    for sa, lcp in arrays[1:]:
        assert np.array_equal(sa, arrays[0][0]) and np.array_equal(lcp, arrays[0][1])


# ---- b. the same context afterwards -----------------------------------------------------------------------------------------
def chain_counters(db):
    return db.ctx.overlapped, db.ctx.doublings


def shard0_way3_limit(db, amb=True):
    """R_hash in three shards: shard 0 takes `taken` ranks out and places more than that, the '#' suffixes of the 'N' shard
    added -- a limit of `taken` passes the count of ranks and gives up on the count of suffixes to place"""
    db.ctx.set_exc_max_affected(0)
    build(db, device_text("R_hash"), is_dna=True, allow_ambiguity=amb, shard_index=0, num_shards=3)
    taken, placed = int(db.ctx.exc_taken), int(db.stats.num_reinserted)
    assert db.ctx.exc_retry == 0 and placed > taken >= 1, f"shard 0 of R_hash: {taken} ranks taken out, {placed} suffixes placed"
    return taken, placed


@pytest.mark.parametrize("way", [1, 2, 3])
def test_the_context_after_a_retry(db, way):
    """after a retry of each kind the same context builds a text without listed bytes (under the lowered limit) and text R (under
    the default limit) as a fresh context does: no retry, the 3-bit table, correct arrays, and the chain counters of those
    builds -- nothing of the retry (exc_disable, pending bytes, the counters of the inner build) is left behind"""
    fresh = sufr_amd.DeviceBuilder(0)
    try:
        one_shard(fresh, "clean", False, 0, 0, "clean, fresh context"); ref_clean = chain_counters(fresh)
        one_shard(fresh, "R", False, 0, 0, "R, fresh context"); ref_r = chain_counters(fresh)
    finally:
        fresh.close()
    if way == 3:
        limit, _ = shard0_way3_limit(db)
        db.ctx.set_exc_max_affected(limit)
        sa, _ = build(db, device_text("R_hash"), is_dna=True, allow_ambiguity=True, shard_index=0, num_shards=3)
        assert db.ctx.exc_retry == 3 and db.stats.num_exceptions == 0 and db.stats.bits_per_char > 3
        retried = chain_counters(db)
    else:
        A = affected(db, "R", False, "R")
        limit = limit_for(way, A)
        one_shard(db, "R", False, limit, way, f"R, way {way}")
        retried = chain_counters(db)
        one_shard(db, "R", False, limit, way, f"R, way {way} again")
        assert chain_counters(db) == retried, f"the same retry twice: chain counters {retried} then {chain_counters(db)}"
    one_shard(db, "clean", False, limit, 0, f"clean after way {way}")
    assert chain_counters(db) == ref_clean, f"clean after way {way}: chain counters {chain_counters(db)}, a fresh context's {ref_clean}"
    one_shard(db, "R", False, 0, 0, f"R after way {way}")
    assert chain_counters(db) == ref_r, f"R after way {way}: chain counters {chain_counters(db)}, a fresh context's {ref_r}"
    assert db.stats.num_reinserted >= 64


# ---- c. a caller's text that is not 16-byte aligned: the retry stages it a second time -------------------------------------------
@pytest.mark.parametrize("way", [1, 2])
def test_retry_of_a_misaligned_text(db, way):
    A = affected(db, "R", False, "R at offset 1", offset=1)
    one_shard(db, "R", False, limit_for(way, A), way, f"R at offset 1, way {way}", offset=1)


# ---- d. capped builds ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("way", [1, 2])
@pytest.mark.parametrize("L", [12, 17])
def test_retry_of_a_capped_build(db, L, way):
    """--max-query-len L built directly: the canonical form of the capped arrays (order of the first L symbols, ties in
    descending position, LCP = min(exact, L)), from the 3-bit build and from the retry alike"""
    A = affected(db, "R", False, f"R, -m {L}", cap=L)
    one_shard(db, "R", False, limit_for(way, A), way, f"R, -m {L}, way {way}", cap=L)
    print(f"R -m {L} way {way}: (exc_retry, exc_taken) = ({db.ctx.exc_retry}, {db.ctx.exc_taken})")


# ---- e. windows --------------------------------------------------------------------------------------------------------------
def test_retry_inside_windows(db):
    """three windows of 41 000 positions with a margin of 2 500 (above the 2 000 symbols of the planted segment): every window
    holds copies of the segment and listed bytes, and builds its text on its own.  A limit far below the count of the windows:
    windows retry, the merged arrays are the oracle's"""
    raw = text("R")
    osa, olcp = want("R", False)
    db.ctx.set_window(41_000, 2_500)
    assert -(-raw.size // 41_000) == 3
    gsa, glcp = build(db, device_text("R"), is_dna=True)
    same(gsa, glcp, osa, olcp, "three windows, default limit")
    assert db.ctx.exc_retry == 0 and db.num_suffixes == osa.size
    taken = int(db.ctx.exc_taken)                     # (of the last window that took ranks out)
    assert taken >= 64, f"the last window with listed bytes took {taken} ranks out"
    db.ctx.set_exc_max_affected(taken // 4)
    gsa, glcp = build(db, device_text("R"), is_dna=True)
    print(f"three windows, limit {taken // 4}: exc_retry {db.ctx.exc_retry}, exc_taken {db.ctx.exc_taken} (default limit: {taken})")
    same(gsa, glcp, osa, olcp, f"three windows, limit {taken // 4}")
    assert db.ctx.exc_retry > 0 and db.num_suffixes == osa.size
    db.ctx.set_window(0, 0)
    one_shard(db, "R", False, 0, 0, "one window again, default limit")


# ---- f. the host-buffer ABI ------------------------------------------------------------------------------------------------------
def test_host_buffers_after_a_retry_that_skipped_the_restore():
    """sufr_hip_build_u32 through way 1, which gives up while the context's text still holds 'N' for the listed bytes:
    norm_text_out carries the letters"""
    raw = text("R")
    osa, olcp = want("R", False)
    ctx = sufr_amd.Context(0)
    try:
        args = sufr_amd.SufrBuilderArgs(text=raw.copy(), is_dna=True)
        b = sufr_amd.SufrBuilder(args, index_width=4, ctx=ctx, write=False)
        A = int(b.stats.num_reinserted)
        assert ctx.exc_retry == 0 and A >= 64 and b.stats.num_exceptions == 10
        ctx.set_exc_max_affected(A // 32)
        b = sufr_amd.SufrBuilder(args, index_width=4, ctx=ctx, write=False)
        assert ctx.exc_retry == 1 and b.stats.num_exceptions == 0 and b.stats.bits_per_char > 3
        assert np.array_equal(b.text, raw), f"norm_text_out differs at {np.nonzero(b.text != raw)[0][:8]}"
        assert b.num_suffixes == osa.size
        same(np.asarray(b.suffix_array), np.asarray(b.lcp), osa, olcp, "host buffers, way 1")
    finally:
        ctx.set_exc_max_affected(0)
        ctx.close()


# ---- g, h. shards that disagree ------------------------------------------------------------------------------------------------
def shards(db, name, amb, limit, num=3):
    """every shard of the text under `limit` -> [(SA, LCP, exc_retry, exc_taken, num_reinserted)]"""
    raw = text(name)
    db.ctx.set_exc_max_affected(limit)
    out = []
    for k in range(num):
        sa, lcp = build(db, device_text(name), is_dna=True, allow_ambiguity=amb, shard_index=k, num_shards=num)
        st = db.stats
        retry = db.ctx.exc_retry
        what = f"{name}, amb={amb}, shard {k} of {num}, limit {limit}"
        assert db.num_suffixes == sa.size == st.num_suffixes, f"{what}: {sa.size} suffixes, num_suffixes {db.num_suffixes} / {st.num_suffixes}"
        if retry:
            assert st.num_exceptions == 0 and st.bits_per_char > 3, f"{what}: after the retry {st.num_exceptions} listed bytes, {st.bits_per_char} bits"
        else:
            assert st.num_exceptions == listed(raw) and st.bits_per_char == 3, f"{what}: {st.num_exceptions} listed bytes, {st.bits_per_char} bits"
        got = _context_text(db.ctx, raw.size)
        assert np.array_equal(got, raw), f"{what}: the context's text differs at {np.nonzero(got != raw)[0][:8]}"
        out.append((sa, lcp, retry, int(db.ctx.exc_taken), int(st.num_reinserted)))
    print(f"{name} amb={amb} limit {limit}: (exc_retry, exc_taken, num_reinserted), suffixes per shard = {[(p[2:], p[0].size) for p in out]}")
    return out


def predicted(base, limit):
    """which comparison gives up in every shard, from the counters of the build with the default limit"""
    return [2 if taken > limit else 3 if placed > limit else 0 for _, _, _, taken, placed in base]


def check_shards(parts, name, amb, what):
    """the shards concatenate to the oracle's arrays: no suffix lost, none twice (a shard's first LCP is the stitch's)"""
    osa, olcp = want(name, amb)
    sizes = [p[0].size for p in parts]
    gsa = np.concatenate([p[0] for p in parts]); glcp = np.concatenate([p[1] for p in parts])
    twice = gsa.size - np.unique(gsa).size
    lost = np.setdiff1d(osa, gsa).size
    assert sum(sizes) == osa.size and twice == 0 and lost == 0, \
        f"{what}: shard sizes {sizes} sum to {sum(sizes)}, the text has {osa.size} suffixes: {lost} lost, {twice} repeated (exc_retry {[p[2] for p in parts]})"
    same(gsa, glcp, osa, olcp, what, skip_lcp_at=np.cumsum(sizes[:-1]).tolist())


@pytest.mark.parametrize("amb", [False, True])
def test_shards_of_which_some_retry(db, amb):
    """three shards of text R.  The affected suffixes start with the segment's A and C: the shard of the low ranks takes
    thousands out, the shard of the high ranks a few dozen.  A limit that only the fullest shard exceeds, one that all but the
    emptiest exceed, and 1 (all retry): a rank that retries hands out the suffixes of the first-digit range its neighbours
    left to it, whatever code table it built them with"""
    base = shards(db, "R", amb, 0)
    assert [p[2] for p in base] == [0, 0, 0]
    check_shards(base, "R", amb, f"R, amb={amb}, default limit")
    need = [max(p[3], p[4]) for p in base]                  # the least limit under which the shard does not retry
    order = sorted(need)
    assert max(p[3] for p in base) >= 20 * max(1, min(p[3] for p in base)), f"ranks taken out per shard: {[p[3] for p in base]}"
    assert order[0] < order[1] < order[2] and order[0] >= 2, f"suffixes per shard to take out / place: {need}"
    for limit, retrying in ((order[2] - 1, 1), (order[0], 2), (1, 3)):
        want_retry = predicted(base, limit)
        assert sum(1 for w in want_retry if w) == retrying, (limit, want_retry, need)
        parts = shards(db, "R", amb, limit)
        assert [p[2] for p in parts] == want_retry, f"limit {limit}: exc_retry {[p[2] for p in parts]}, predicted {want_retry}"
        check_shards(parts, "R", amb, f"R, amb={amb}, limit {limit}")


def test_a_shard_that_gives_up_on_the_suffixes_added_to_it(db):
    """way 3: R_hash under --allow-ambiguity.  The 600 suffixes that start at a '#' are built as 'N...' in the last shard and
    belong to shard 0 ('#' < '$'): shard 0 places more suffixes than it took out.  A limit between the two"""
    assert listed(text("R_hash")) == 610 and 610 * 64 <= N_R
    base = shards(db, "R_hash", True, 0)
    assert [p[2] for p in base] == [0, 0, 0]
    check_shards(base, "R_hash", True, "R_hash, default limit")
    taken, placed = base[0][3], base[0][4]
    assert placed > taken >= 1, f"shard 0: {taken} ranks taken out, {placed} suffixes placed"
    limit = taken
    want_retry = predicted(base, limit)
    assert want_retry[0] == 3
    parts = shards(db, "R_hash", True, limit)
    assert [p[2] for p in parts] == want_retry, f"limit {limit}: exc_retry {[p[2] for p in parts]}, predicted {want_retry}"
    assert parts[0][3] == taken                       # (exc_taken is set when the build then gives up, too)
    check_shards(parts, "R_hash", True, f"R_hash, limit {limit}")


# ---- j. the setter -----------------------------------------------------------------------------------------------------------
def test_the_setter_refuses_more_than_the_buffers_take(db):
    L = sufr_amd.lib()
    assert L.sufr_hip_set_exc_max_affected(db.ctx.handle, DEFAULT_LIMIT + 1) == -1          # SUFR_HIP_E_INVALID
    msg = L.sufr_hip_last_error(db.ctx.handle).decode()
    assert str(DEFAULT_LIMIT + 1) in msg and "2^22" in msg, msg
    with pytest.raises(sufr_amd.SufrHipError) as e:
        db.ctx.set_exc_max_affected(1 << 40)
    assert e.value.code == -1
    one_shard(db, "R", False, DEFAULT_LIMIT, 0, "R, limit 2^22")          # (the refused values changed nothing; 2^22 itself is taken)
    one_shard(db, "R", False, 1, 1, "R, limit 1")
    one_shard(db, "R", False, 0, 0, "R, limit 0: the default again")
    assert db.stats.num_reinserted >= 64
