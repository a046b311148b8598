"""Sequence counts of repeats and k-common substrings on the GPU (include/sufr_shared.h, sufr_shared.inc) against the host path
of the same library, which tests/test_shared_host.py holds to its witnesses.  Every comparison is exact array equality: the
four record arrays, their order, the total, the stats and the whole profile."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import sufr_amd
from sufr_amd import DeviceIndex, SufrFile, synth
from oracle_helper import GOLDEN
from test_kmer_gpu import _dev, indexes, oracle_file
from test_repeat_host import clipped, stack_answers
from test_shared_host import NOTHING, docs_of

pytestmark = pytest.mark.gpu
EXP = GOLDEN / "expected"
KINDS = (0, 1, 2)
T = 256                                                               # the smallest tile: one workgroup of ranks
FF = 0xFFFFFFFFFFFFFFFF
# (min_count, max_count, min_seqs, max_seqs)
OPEN = ((2, 0, 0, 0),)


@pytest.fixture(scope="module")
def ctx():
    c = sufr_amd.Context(0)
    yield c
    c.close()


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def same_as_host(f: SufrFile, ix: DeviceIndex, lcp, kinds, min_lens, filters=OPEN, tag="", threads=0, common=True):
    """the device's records, order, total, stats and profile equal the host's; returns the number of records seen"""
    seen = 0
    for kind in kinds:
        for ml in min_lens:
            for mc, xc, mq, xq in filters:
                want = f.shared(kind, ml, mc, xc, mq, xq, threads=threads)
                got = ix.shared_device(lcp, kind, ml, mc, xc, mq, xq, f.sequence_starts)
                for i in range(4):
                    assert np.array_equal(_u64(got[i]), want[i]), (tag, kind, ml, mc, xc, mq, xq, i)
                assert got[4] == want[4], (tag, kind, ml, mc, xc, mq, xq, got[4], want[4])
                seen += want[4]["records"]
    if common:
        assert np.array_equal(_u64(ix.common_device(lcp, f.sequence_starts)), f.common(threads=threads)), tag
    return seen


def pairs_of(f: SufrFile):
    """(prev, q) of every rank that has a previous rank of its sequence, by linear scans over the clipped LCP"""
    ell, D = clipped(f)[:-1], docs_of(f)
    last, prev, qs = {}, [], []
    for r in range(D.size):
        p = last.get(int(D[r]))
        last[int(D[r])] = r
        if p is not None:
            prev.append(p)
            qs.append(p + 1 + int(np.argmin(ell[p + 1:r + 1])))
    return np.array(prev, dtype=np.int64), np.array(qs, dtype=np.int64)


def interval_starts(f: SufrFile):
    """a of every interval"""
    ell = clipped(f)[:-1].astype(np.uint64)
    left, _ = stack_answers(ell)
    reps = np.array([r for r in range(1, ell.size) if ell[r] >= 1 and ell[int(left[r])] < ell[r]], dtype=np.int64)
    return left[reps].astype(np.int64)


@pytest.mark.parametrize("name", sorted(p.name for p in EXP.glob("*.sufr")))
def test_device_equals_host_on_golden_files(ctx, name):
    f = SufrFile(EXP / name)
    for tag, ix, lcp in indexes(ctx, f):
        if f.seed_mask:
            if tag == "loaded":
                for call in (lambda: ix.shared_device(lcp, 0, 3), lambda: ix.common_device(lcp)):
                    with pytest.raises(sufr_amd.SufrHipError) as e:
                        call()
                    assert e.value.code == -6
            ix.close()
            continue
        top = max(int(clipped(f).max()), 1)
        k = f.num_sequences
        for tile in (0, T):
            ctx.set_repeat_tile(tile)
            seen = same_as_host(f, ix, lcp, KINDS, (1, 3, top), ((2, 0, 0, 0), (3, 4, 0, 0), (2, 0, 2, 0), (2, 0, 1, 1), (2, 0, k, k)), tag=(tag, tile))
            assert seen > 0 or f.len_suffixes < 12
            assert ix.shared_device(lcp, 0, top + 1, seq_starts=f.sequence_starts)[4] == NOTHING
            assert ix.shared_device(lcp, 0, 1, min_seqs=k + 1, seq_starts=f.sequence_starts)[4] == NOTHING
        ctx.set_repeat_tile(0)
        ix.close()


def test_refusals_return_the_host_codes(ctx, oracle, tmp_path):
    f = oracle_file(oracle, tmp_path, synth.adversarial("tandem", 1200, seed=3)[:-1], is_dna=True, max_query_len=6)
    ix = DeviceIndex.load(ctx, f)
    lcp = _dev(np.asarray(f.lcp))
    for call in (lambda: ix.shared_device(lcp, 0, 3), lambda: f.shared(0, 3), lambda: ix.shared_device(lcp, 0, 0), lambda: f.shared(0, 0),
                 lambda: ix.common_device(lcp), lambda: f.common()):
        with pytest.raises(sufr_amd.SufrHipError) as e:
            call()
        assert e.value.code == -6                                    # (the capped build is refused before min_len is looked at)
    ix.close()
    g = SufrFile(EXP / "3.sufr")
    ix = DeviceIndex.load(ctx, g)
    lcp = _dev(np.asarray(g.lcp))
    for call in (lambda: ix.shared_device(lcp, 0, 0), lambda: g.shared(0, 0), lambda: ix.shared_device(lcp, 3, 1), lambda: g.shared(3, 1),
                 lambda: ix.shared_device(lcp, 0, 1, min_seqs=3, max_seqs=2), lambda: g.shared(0, 1, min_seqs=3, max_seqs=2)):
        with pytest.raises(sufr_amd.SufrHipError) as e:
            call()
        assert e.value.code == -1
    L = sufr_amd.lib()
    total = C.c_uint64(7)
    out = torch.zeros(8, dtype=torch.int64, device="cuda")
    for bad in ([1, 5], [0, 5, 5], [0, 9, 5], [0, g.text_len]):
        st = np.array(bad, dtype=np.uint64)
        assert L.sufr_hip_shared_device(ctx.handle, ix._h, lcp.data_ptr(), st.ctypes.data, st.size, 0, 1, 0, 0, 0, 0, 0, None, None, None, None,
                                        C.byref(total), None) == -1, bad
        assert total.value == 0
        assert L.sufr_hip_common_device(ctx.handle, ix._h, lcp.data_ptr(), st.ctypes.data, st.size, out.data_ptr()) == -1, bad
    ctx.synchronize()
    ix.close()


# ---------------------------------------------------------------------------------------------------------------------
# tile and window boundaries, with the tile at its minimum
# ---------------------------------------------------------------------------------------------------------------------
def test_pairs_and_intervals_across_tiles(ctx, oracle, tmp_path):
    rng = np.random.default_rng(8)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    sep = np.frombuffer(b"%", dtype=np.uint8)
    ctx.set_repeat_tile(T)
    on_prev = on_q = on_a = False
    try:
        # 40 identical sequences of 80 symbols: every group of 40 equal suffixes collects its 39 pairs on few q
        piece = acgt[rng.integers(0, 4, 80)]
        f = oracle_file(oracle, tmp_path, np.concatenate([np.concatenate([piece, sep])] * 40)[:-1], "same", is_dna=True)
        assert f.num_sequences == 40 and f.len_suffixes > 12 * T
        prev, qs = pairs_of(f)
        assert np.bincount(qs).max() >= 39
        on_prev, on_q, on_a = on_prev or bool((prev % T == 0).any()), on_q or bool((qs % T == 0).any()), on_a or bool(((interval_starts(f) + 1) % T == 0).any())
        ix = DeviceIndex.load(ctx, f)
        lcp = _dev(np.asarray(f.lcp))
        assert same_as_host(f, ix, lcp, KINDS, (1, 40, 80), ((2, 0, 0, 0), (2, 0, 40, 0), (2, 0, 1, 39), (41, 0, 0, 0))) > 0
        assert ix.shared_device(lcp, 0, 80, seq_starts=f.sequence_starts)[4] == dict(records=1, longest=80, longest_rank=int(f.shared(0, 80)[0][0]),
                                                                                      max_count=40, max_seqs=40)
        assert _u64(ix.common_device(lcp, f.sequence_starts)).tolist() == [80] * 40
        ix.close()
        # one long sequence and one of two symbols whose two suffixes lie more than 8 tiles apart: one pair whose range
        # minimum and search leave every window
        long = np.frombuffer(b"CG", dtype=np.uint8)[rng.integers(0, 2, 3000)].copy()
        long[rng.integers(0, 3000, 60)] = ord("A")
        f = oracle_file(oracle, tmp_path, np.concatenate([np.frombuffer(b"AT%", dtype=np.uint8), long]), "far", is_dna=True)
        D = docs_of(f)
        two = np.nonzero(D == 0)[0]
        assert f.num_sequences == 2 and two.size == 2 and two[1] - two[0] > 8 * T
        prev, qs = pairs_of(f)
        on_prev, on_q, on_a = on_prev or bool((prev % T == 0).any()), on_q or bool((qs % T == 0).any()), on_a or bool(((interval_starts(f) + 1) % T == 0).any())
        ix = DeviceIndex.load(ctx, f)
        assert same_as_host(f, ix, _dev(np.asarray(f.lcp)), KINDS, (1, 2, 6), ((2, 0, 0, 0), (2, 0, 2, 0), (2, 0, 1, 1))) > 0
        ix.close()
        # A^3000 cut into 3 sequences: the intervals are nested, every b is far away, and seqs is at its ceiling
        body = np.full(3002, ord("A"), dtype=np.uint8)
        body[[1000, 2001]] = ord("%")
        f = oracle_file(oracle, tmp_path, body, "a3", is_dna=True)
        assert f.num_sequences == 3 and f.len_suffixes > 8 * T
        prev, qs = pairs_of(f)
        on_prev, on_q, on_a = on_prev or bool((prev % T == 0).any()), on_q or bool((qs % T == 0).any()), on_a or bool(((interval_starts(f) + 1) % T == 0).any())
        ix = DeviceIndex.load(ctx, f)
        lcp = _dev(np.asarray(f.lcp))
        assert same_as_host(f, ix, lcp, KINDS, (1, 5, 1000, 1001), ((2, 0, 0, 0), (2, 0, 3, 0), (100, 2000, 0, 2))) > 0
        rank, count, length, seqs, st = ix.shared_device(lcp, 0, 1, seq_starts=f.sequence_starts)
        assert st["max_seqs"] == 3 and (_u64(seqs) == np.minimum(_u64(count), 3)).all() and (_u64(count) > 8 * T).any()
        assert _u64(ix.common_device(lcp, f.sequence_starts)).tolist() == [1000, 1000, 1000]
        ix.close()
        assert on_prev and on_q and on_a
    finally:
        ctx.set_repeat_tile(0)


def test_shared_with_open_seqs_is_repeats_plus_a_column(ctx, oracle, tmp_path):
    """one find kernel serves both calls: with min_seqs = max_seqs = 0 shared keeps what repeats keeps, in its order, and the
    counting calls agree -- on the three indexes of uniprot.sufr (32- and 64-bit arrays) and on the two small collections of
    test_pairs_and_intervals_across_tiles, whose intervals cross the tiles and the staged windows"""
    rng = np.random.default_rng(8)
    piece = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 80)]
    same = oracle_file(oracle, tmp_path, np.concatenate([np.concatenate([piece, np.frombuffer(b"%", dtype=np.uint8)])] * 40)[:-1], "same", is_dna=True)
    body = np.full(3002, ord("A"), dtype=np.uint8)
    body[[1000, 2001]] = ord("%")
    a3 = oracle_file(oracle, tmp_path, body, "a3", is_dna=True)
    assert same.num_sequences == 40 and same.len_suffixes > 12 * T and a3.num_sequences == 3 and a3.len_suffixes > 8 * T
    uni = SufrFile(EXP / "uniprot.sufr")
    cases = [(f"uniprot {tag}", uni, ix, lcp) for tag, ix, lcp in indexes(ctx, uni)]
    cases += [(name, f, DeviceIndex.load(ctx, f), _dev(np.asarray(f.lcp))) for name, f in (("same", same), ("a3", a3))]
    L = sufr_amd.lib()
    seen = 0
    try:
        for name, f, ix, lcp in cases:
            st_h = np.array(f.sequence_starts, dtype=np.uint64)
            head = (ctx.handle, ix._h, lcp.data_ptr(), st_h.ctypes.data, st_h.size)
            for tile in (T, 0):
                ctx.set_repeat_tile(tile)
                for kind in KINDS:
                    for ml in (1, 5):
                        for mc, xc in ((2, 0), (3, 4)):
                            tag = (name, tile, kind, ml, mc, xc)
                            shr = ix.shared_device(lcp, kind, ml, mc, xc, 0, 0, f.sequence_starts)
                            rep = ix.repeats_device(lcp, kind, ml, mc, xc, f.sequence_starts)
                            for i in range(3):
                                assert np.array_equal(_u64(shr[i]), _u64(rep[i])), (tag, i)
                            assert _u64(shr[3]).size == _u64(rep[0]).size and {k: shr[4][k] for k in rep[3]} == rep[3], (tag, shr[4], rep[3])
                            # the counting calls: no room and no arrays
                            ts, tr = C.c_uint64(0), C.c_uint64(0)
                            rs = L.sufr_hip_shared_device(*head, kind, ml, mc, xc, 0, 0, 0, None, None, None, None, C.byref(ts), None)
                            rr = L.sufr_hip_repeats_device(*head, kind, ml, mc, xc, 0, None, None, None, C.byref(tr), None)
                            assert ts.value == tr.value == rep[3]["records"], (tag, ts.value, tr.value)
                            assert rs == rr == (-5 if tr.value else 0), (tag, rs, rr)       # (E_CAPACITY; nothing kept: nothing to refuse)
                            seen += tr.value
        assert seen > 0
    finally:
        ctx.set_repeat_tile(0)
        for _, _, ix, _ in cases:
            ix.close()


# ---------------------------------------------------------------------------------------------------------------------
# the digits of the sort
# ---------------------------------------------------------------------------------------------------------------------
def test_two_digits_the_second_partial(ctx, oracle, tmp_path):
    rng = np.random.default_rng(9)
    ac = np.frombuffer(b"ACGT", dtype=np.uint8)
    sep = np.frombuffer(b"%", dtype=np.uint8)
    family = ac[rng.integers(0, 4, 12)]
    parts = []
    for i in range(300):
        s = ac[rng.integers(0, 4, int(rng.integers(3, 30)))]
        if i % 3 == 0:
            s = np.concatenate([s[:2], family[:int(rng.integers(4, 13))], s[2:]])     # a family shared by a third of them
        parts += [s, sep]
    f = oracle_file(oracle, tmp_path, np.concatenate(parts[:-1]), "d300", is_dna=True)
    assert f.num_sequences == 300
    common = f.common()
    assert common[99] >= 4 and common[-1] <= 2
    ix = DeviceIndex.load(ctx, f)
    lcp = _dev(np.asarray(f.lcp))
    for tile in (T, 0):
        ctx.set_repeat_tile(tile)
        assert same_as_host(f, ix, lcp, KINDS, (1, 4), ((2, 0, 0, 0), (2, 0, 50, 0), (2, 0, 2, 99)), tag=tile) > 0
    ctx.set_repeat_tile(0)
    ix.close()


def test_more_sequences_than_the_suffix_sweep_has_lanes(ctx, oracle, tmp_path):
    """2050 short sequences: the profile has three entries to a lane of the suffix-maximum sweep (the upper lanes have none),
    and the maxima that set common[] for small and for large sequence counts lie in different lanes' blocks"""
    rng = np.random.default_rng(12)
    ac = np.frombuffer(b"ACGT", dtype=np.uint8)
    sep = np.frombuffer(b"%", dtype=np.uint8)
    families = [(2, ac[rng.integers(0, 4, 9)]), (5, ac[rng.integers(0, 4, 11)]), (41, ac[rng.integers(0, 4, 14)])]      # every 2nd, 5th, 41st
    parts = []
    for i in range(2050):
        s = ac[rng.integers(0, 4, int(rng.integers(3, 12)))]
        for every, fam in families:
            if i % every == 0:
                s = np.concatenate([s, fam, ac[rng.integers(0, 4, 2)]])
        parts += [s, sep]
    f = oracle_file(oracle, tmp_path, np.concatenate(parts[:-1]), "d2050", is_dna=True)
    num, per = f.num_sequences, (2050 + 1023) // 1024
    assert num == 2050 and per == 3 and (num + per - 1) // per < 1024
    common = f.common()
    steps = np.nonzero(common[:-1] != common[1:])[0]                 # common[k] > common[k + 1]: entry k of the profile is a maximum of its own
    assert common[49] >= 14 > common[409] >= 11 > common[1024] >= 9 and len(set((steps // per).tolist())) >= 3
    assert (steps % per != per - 1).any() and (steps >= 1024).any()  # (inside a lane's block, and beyond the lane count)
    for tag, ix, lcp in indexes(ctx, f):                               # loaded, wrapped, and wrapped with 64-bit arrays
        for tile in (T, 0):
            ctx.set_repeat_tile(tile)
            assert same_as_host(f, ix, lcp, (0,), (4,), ((2, 0, 0, 0), (2, 0, 400, 0)), tag=(tag, tile)) > 0
        ctx.set_repeat_tile(0)
        ix.close()


def _write_collection(path, text: np.ndarray, sa: np.ndarray, lcp: np.ndarray, starts: np.ndarray):
    err = C.create_string_buffer(256)
    st = np.ascontiguousarray(starts, dtype=np.uint64)
    names = (C.c_char_p * st.size)(*[b"s"] * st.size)
    rc = sufr_amd.lib().sufr_write_file(str(path).encode(), 1, 0, 0, text.ctypes.data, text.size, sa.dtype.itemsize, sa.ctypes.data, lcp.ctypes.data,
                                        sa.size, 0, 0, None, st.ctypes.data, st.size, names, err, len(err))
    assert rc == 0, err.value


def test_three_digits_and_three_coarser_levels(ctx, oracle, tmp_path):
    """70 000 sequences of 20 symbols, 1.47 M positions: three digit passes of the sort, three levels above the clipped LCP,
    and with the tile at 256 more tiles than the largest grid has workgroups"""
    rng = np.random.default_rng(10)
    k, m = 70_000, 20
    body = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (k, m + 1))]
    body[:, m] = ord("%")
    body[::7, 3:15] = body[0, 3:15]                                   # a 12-mer shared by every 7th sequence
    text = body.reshape(-1).copy()
    text[-1] = ord("$")
    starts = np.arange(k, dtype=np.uint64) * (m + 1)
    sa, lcp, _ = oracle.build(text, is_dna=True, threads=16)
    assert sa.size > 64 ** 3 and sa.size / T > 4096
    _write_collection(tmp_path / "x.sufr", text, sa, lcp, starts)
    f = SufrFile(tmp_path / "x.sufr")
    assert f.num_sequences == k
    ix = DeviceIndex.wrap(ctx, torch.from_numpy(text).cuda(), _dev(sa), is_dna=True, prefix_table=False)
    lcp = _dev(lcp)
    want = {kind: f.shared(kind, 8, threads=16) for kind in (0, 1)}
    common = f.common(threads=16)
    assert want[0][4]["records"] > 1000 and want[0][4]["max_seqs"] >= k // 7 and common[k // 7 - 1] >= 12 and common[-1] == 0
    for tile, kinds in ((T, (0, 1)), (0, (0,))):
        ctx.set_repeat_tile(tile)
        for kind in kinds:
            got = ix.shared_device(lcp, kind, 8, seq_starts=f.sequence_starts)
            assert all(np.array_equal(_u64(got[i]), want[kind][i]) for i in range(4)) and got[4] == want[kind][4], (tile, kind)
        assert np.array_equal(_u64(ix.common_device(lcp, f.sequence_starts)), common), tile
    ctx.set_repeat_tile(0)
    ix.close(); f.close()


# ---------------------------------------------------------------------------------------------------------------------
# the other cases
# ---------------------------------------------------------------------------------------------------------------------
def test_filters_and_capacity(ctx):
    f = SufrFile(EXP / "uniprot.sufr")
    k = f.num_sequences
    ix = DeviceIndex.load(ctx, f)
    lcp = _dev(np.asarray(f.lcp))
    L = sufr_amd.lib()
    # the longest substring common to all sequences, and the repeats private to one
    every = ix.shared_device(lcp, 0, 1, min_seqs=k, seq_starts=f.sequence_starts)
    common = _u64(ix.common_device(lcp, f.sequence_starts))
    assert every[4] == f.shared(0, 1, min_seqs=k)[4] and every[4]["longest"] == int(common[-1]) == int(f.common()[-1])
    private = ix.shared_device(lcp, 0, 3, max_seqs=1, seq_starts=f.sequence_starts)
    want = f.shared(0, 3, max_seqs=1)
    assert want[4]["records"] > 10 and private[4] == want[4] and (_u64(private[3]) == 1).all()
    assert all(np.array_equal(_u64(private[i]), want[i]) for i in range(4))
    # the capacity rule
    want = f.shared(1, 3, min_seqs=2)
    n = want[4]["records"]
    assert n > 10
    st_h = np.array(f.sequence_starts, dtype=np.uint64)
    out = [torch.full((n + 50,), -1, dtype=torch.int64, device="cuda") for _ in range(4)]           # 0xFF in every byte
    total, st = C.c_uint64(0), sufr_amd.SharedStats()
    args = (ctx.handle, ix._h, lcp.data_ptr(), st_h.ctypes.data, st_h.size, 1, 3, 0, 0, 2, 0)
    assert L.sufr_hip_shared_device(*args, 0, None, None, None, None, C.byref(total), C.byref(st)) == -5       # the counting call
    assert total.value == n and st.as_dict() == want[4]
    total.value = 0
    assert L.sufr_hip_shared_device(*args, n - 1, *(o.data_ptr() for o in out), C.byref(total), None) == -5
    ctx.synchronize()
    assert total.value == n and all((_u64(o) == FF).all() for o in out)                                 # nothing written
    ctx.check(L.sufr_hip_shared_device(*args, n + 50, *(o.data_ptr() for o in out), C.byref(total), C.byref(st)))
    ctx.synchronize()
    for i in range(4):
        assert np.array_equal(_u64(out[i])[:n], want[i]) and (_u64(out[i])[n:] == FF).all()
    assert total.value == n and st.as_dict() == want[4]
    ix.close()


def test_arrays_of_no_and_one_rank(ctx):
    for tile in (T, 0):
        ctx.set_repeat_tile(tile)
        text = torch.from_numpy(np.frombuffer(b"A$", dtype=np.uint8).copy()).cuda()
        for ranks in (1, 0):
            ix = DeviceIndex.wrap(ctx, text, torch.zeros(ranks, dtype=torch.int32, device="cuda"), prefix_table=False)
            lcp = torch.zeros(ranks, dtype=torch.int32, device="cuda")
            for kind in KINDS:
                out = ix.shared_device(lcp, kind, 1)
                assert all(t.numel() == 0 for t in out[:4]) and out[4] == NOTHING
            assert _u64(ix.common_device(lcp)).tolist() == [0]
            ix.close()
    ctx.set_repeat_tile(0)


def test_one_sequence_and_build_then_analyse_on_the_device(ctx, oracle, tmp_path):
    x, _ = synth.syn_ecoli(100_000, seed=9)
    text = x.numpy()
    f = oracle_file(oracle, tmp_path, text[:-1], is_dna=True, threads=4)
    assert np.array_equal(np.asarray(f.text), text) and f.num_sequences == 1
    db = sufr_amd.DeviceBuilder(0)
    t = torch.from_numpy(text).cuda()
    sa, lcp = db.sort(t, is_dna=True)
    ix = DeviceIndex.wrap(db.ctx, t, sa, is_dna=True)
    assert same_as_host(f, ix, lcp, KINDS, (8, 14), ((2, 0, 0, 0), (3, 20, 1, 1))) > 0
    rank, count, length, seqs, st = ix.shared_device(lcp, 0, 8)      # no sequence starts at all: one sequence
    assert (_u64(seqs) == 1).all() and st["max_seqs"] == 1 and _u64(ix.common_device(lcp)).tolist() == [st["longest"]] == [f.repeats(0, 1)[3]["longest"]]
    assert ix.shared_device(lcp, 0, 8, min_seqs=2)[4] == NOTHING
    ix.close(); db.close()


def test_two_contexts_on_two_threads_share_an_index(ctx):
    f = SufrFile(EXP / "uniprot.sufr")
    ix = DeviceIndex.load(ctx, f)
    lcp = _dev(np.asarray(f.lcp))
    other = sufr_amd.Context(0)
    twin = DeviceIndex(other, ix._h)                                 # the same index through the second context
    twin.text_len, twin.index_width = ix.text_len, ix.index_width
    want = {kind: f.shared(kind, 3, min_seqs=2) for kind in (1, 2)}
    common = f.common()
    results, errors = {}, []

    def work(name, index):
        try:
            out = []
            for _ in range(4):
                for kind in (1, 2):
                    got = index.shared_device(lcp, kind, 3, min_seqs=2, seq_starts=f.sequence_starts)
                    out.append((kind, [_u64(got[i]) for i in range(4)], got[4], _u64(index.common_device(lcp, f.sequence_starts))))
            results[name] = out
        except Exception as e:                                       # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=work, args=(nm, i)) for nm, i in (("a", ix), ("b", twin))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    twin._h = None                                                   # (the index is freed once, by ix)
    assert not errors, errors
    for name in ("a", "b"):
        for kind, cols, st, prof in results[name]:
            assert all(np.array_equal(cols[i], want[kind][i]) for i in range(4)) and st == want[kind][4] and np.array_equal(prof, common)
    ix.close(); other.close()


def test_cli_shared_on_the_device_prints_the_host_bytes():
    from test_match_host import run
    for name, opts in (("uniprot.sufr", ["-l", 6, "--kind", "maximal", "-q", 2]), ("uniprot.sufr", ["--common"]),
                       ("3.sufr", ["-l", 1, "--kind", "super", "--max-positions", 0, "--max-seqs", 2]), ("2.sufr", ["--common"])):
        host = run("shared", *opts, EXP / name).stdout
        assert host.count("\n") >= 2 and host == run("shared", *opts, "--device", 0, EXP / name).stdout


def test_cli_shared_on_the_device_without_records_to_a_file_and_refused(tmp_path):
    from test_match_host import run
    opts = ["-l", 100000, "-q", 2]
    host = run("shared", *opts, EXP / "uniprot.sufr").stdout
    assert host.count("\n") == 5 and host == run("shared", *opts, "--device", 0, EXP / "uniprot.sufr").stdout
    a, b = tmp_path / "host.tsv", tmp_path / "dev.tsv"
    opts = ["-l", 6, "-q", 2]
    assert run("shared", *opts, "-o", a, EXP / "uniprot.sufr").stdout == run("shared", *opts, "-o", b, "--device", 0, EXP / "uniprot.sufr").stdout == ""
    assert a.read_bytes() == b.read_bytes() != b""
    for opts in (["-l", 3], ["--common"]):
        r = run("shared", *opts, "--device", 0, EXP / "uniprot-masked.sufr", check=False)
        assert r.returncode == 1 and r.stderr.startswith("Error: ") and "uniprot-masked.sufr" in r.stderr
