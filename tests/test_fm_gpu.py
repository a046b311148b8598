"""The FM-index on the GPU (include/sufr_fm.h, sufr_fm.inc) against the host path of the same library and the numpy witness of
tests/test_fm_host.py.  Every comparison is exact array equality: the ranges, the offsets and the positions; on the loaded, the
wrapped and the 64-bit index, at the default BWT tile and with the tile at its minimum, 256."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import sufr_amd
from sufr_amd import DeviceIndex, SufrFile, SufrHipError, pack_queries
from oracle_helper import GOLDEN
from test_kmer_gpu import indexes, oracle_file
from test_lz_host import fibonacci
from test_bwt_host import LF_FILES, runs_of
from test_bwt_gpu import _unsigned, wrapped
from test_fm_host import SAMPLES, UNSUPPORTED, Witness, conditions, file_witness, query_set, random_text, sorted_sa, want_locate

pytestmark = pytest.mark.gpu
EXP = GOLDEN / "expected"
T = 256                                                               # the smallest tile
TILES = (0, T)


@pytest.fixture(scope="module")
def ctx():
    c = sufr_amd.Context(0)
    yield c
    c.set_bwt_tile(0)
    c.close()


def on_device(qs):
    qb, off = pack_queries(qs)
    return torch.from_numpy(qb).cuda(), torch.from_numpy(off.astype(np.int64)).cuda()


class Wanted:
    """the answers of a query set, once per text: the ranges and, per max_hits, the offsets and the positions"""

    def __init__(self, w: Witness, qs, width: int = 4):
        self.w, self.qs = w, qs
        got = [w.search(q)[:2] for q in qs]
        self.lo = np.array([g[0] for g in got], dtype=np.uint64)
        self.hi = np.array([g[1] for g in got], dtype=np.uint64)
        self.located = {m: want_locate(w, self.lo, self.hi, m, np.uint64) for m in (0, 3)}
        self.batch = on_device(qs)


def check_fm(dfm, want: Wanted, tag=""):
    """search and locate of a device FM-index equal the wanted arrays"""
    lo, hi = dfm.search_device(*want.batch)
    assert lo.dtype == torch.int64 and np.array_equal(_unsigned(lo), want.lo) and np.array_equal(_unsigned(hi), want.hi), tag
    if not dfm.info["sample"]:
        with pytest.raises(SufrHipError) as err:
            dfm.locate_device(lo, hi)
        assert err.value.code == UNSUPPORTED, tag
        return
    for max_hits, (w_off, w_pos) in want.located.items():
        off, pos = dfm.locate_device(lo, hi, max_hits)
        assert pos.dtype == (torch.int64 if dfm.index_width == 8 else torch.int32), tag
        assert np.array_equal(_unsigned(off), w_off) and np.array_equal(_unsigned(pos), w_pos), (tag, max_hits)


def check_index(ctx, ix: DeviceIndex, want: Wanted, samples=SAMPLES, tiles=TILES, host=None, tag=""):
    for tile in tiles:
        ctx.set_bwt_tile(tile)
        for sample in samples:
            dfm = ix.fm_device(sample)
            info = dfm.info
            assert info["ranks"] == want.w.s and info["sample"] == sample and info["width"] == ix.index_width, (tag, tile, sample)
            assert info["samples"] == (0 if not sample else int((want.w.sa % sample == 0).sum())) and info["end_byte"] == want.w.e
            if host is not None and ix.index_width == 4:
                assert info == host[sample], (tag, tile, sample)
            check_fm(dfm, want, (tag, tile, sample))
            dfm.close()
    ctx.set_bwt_tile(0)


# ---------------------------------------------------------------------------------------------------------------------
# the golden files: s from 11 (one partial block) to 63 220
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LF_FILES)
def test_device_equals_host_and_witness_on_golden_files(ctx, name):
    f, w = file_witness(name)
    host = {}
    for sample in SAMPLES:
        fm = f.fm(sample)
        host[sample] = fm.info
        B = host[sample]["block"]
    qs = query_set(w, B, seed=3)
    want = Wanted(w, qs)
    fm = f.fm(7)
    lo, hi = fm.search_batch(qs)
    assert np.array_equal(lo, want.lo) and np.array_equal(hi, want.hi)                # host == witness; below device == both
    for max_hits in (0, 3):
        off, pos = fm.locate_ranges(lo, hi, max_hits)
        assert np.array_equal(off, want.located[max_hits][0]) and np.array_equal(pos.astype(np.uint64), want.located[max_hits][1])
    for tag, ix, _ in indexes(ctx, f):
        check_index(ctx, ix, want, host=host, tag=(name, tag))      # every sample, both tiles, on all three indexes
        ix.close()


def test_query_sets_meet_their_conditions():
    """asserted on the CPU arrays so that no set goes vacuous: a third found, a third not, a range of two blocks, a bound equal
    to s, an occ argument that is a multiple of B, a located rank q - 1 steps from its mark, the rank with SA == 0 located"""
    for name, B in (("long_dna_sequence_allow_ambiguity.sufr", 96), ("uniprot.sufr", 160)):
        f, w = file_witness(name)
        assert f.fm(0).info["block"] == B
        qs = query_set(w, B, seed=3)
        for q in (7, 32):
            c = conditions(w, qs, B, q)
            total = c["found"] + c["missed"]
            assert 3 * c["found"] >= total and 3 * c["missed"] >= total and c["widest"] >= 2 * B, c
            assert c["ends"] and c["on_block"] and c["far"] and c["zero"], c


# ---------------------------------------------------------------------------------------------------------------------
# oracle-built texts with every position indexed, the tile at its minimum
# ---------------------------------------------------------------------------------------------------------------------
def test_locate_walks_a_run(ctx, oracle, tmp_path):
    """A^1000: AAA has 998 hits, and every LF step from a rank of the run stays in the run"""
    f = oracle_file(oracle, tmp_path, np.full(1000, ord("A"), dtype=np.uint8), "a", is_dna=True, allow_ambiguity=True)
    w = Witness(np.asarray(f.text), np.asarray(f.suffix_array))
    assert f.len_suffixes == f.text_len == 1001
    qs = query_set(w, 96) + [b"AAA", b"A" * 999 + b"$", b"A" * 1001]
    want = Wanted(w, qs)
    at = qs.index(b"AAA")
    assert int(want.hi[at] - want.lo[at]) == 998
    for tag, ix, _ in indexes(ctx, f):
        check_index(ctx, ix, want, samples=(32, 7, 1), tiles=(T,), tag=tag)
        ix.close()


def test_periodic_texts(ctx, oracle, tmp_path):
    for name, body in (("fib", fibonacci(3000)), ("long_runs", runs_of(b"AC", 3300, 300.0, seed=5))):
        f = oracle_file(oracle, tmp_path, body, name, is_dna=True, allow_ambiguity=True)
        w = Witness(np.asarray(f.text), np.asarray(f.suffix_array))
        assert f.len_suffixes == f.text_len > 3000
        want = Wanted(w, query_set(w, 96, seed=1))
        c = conditions(w, want.qs, 96, 32)
        assert c["widest"] >= 2 * 96 and c["on_block"] and c["far"] and c["zero"] and c["ends"], (name, c)
        for tag, ix, _ in indexes(ctx, f):
            check_index(ctx, ix, want, samples=(32, 2), tiles=(T,), tag=(name, tag))
            ix.close()


# ---------------------------------------------------------------------------------------------------------------------
# all 256 byte values: the wide stride
# ---------------------------------------------------------------------------------------------------------------------
def test_all_byte_values(ctx):
    rng = np.random.default_rng(11)
    text = rng.integers(0, 255, 5000).astype(np.uint8)
    text[:255] = np.arange(255)
    text[-1] = 255                                                   # the end byte occurs once
    sa = sorted_sa(text)
    w = Witness(text, sa)
    want = Wanted(w, query_set(w, 1024))
    c = conditions(w, want.qs, 1024, 32)
    assert c["on_block"] and c["far"] and c["zero"] and c["ends"], c
    for name, ix in wrapped(ctx, text, sa):
        ctx.set_bwt_tile(T)
        info = ix.fm_device(32).info
        assert (info["symbols"], info["block"], info["stride"]) == ((256, 1024, 2048) if name == "wrapped" else (256, 2048, 4096)), info
        check_index(ctx, ix, want, samples=(32, 1), tag=name)
        ix.close()


# ---------------------------------------------------------------------------------------------------------------------
# sizes around the block, the mark word and the tile
# ---------------------------------------------------------------------------------------------------------------------
def test_sizes_around_the_block_the_mark_word_and_the_tile(ctx):
    text = random_text(97, 1)
    probe = DeviceIndex.wrap(ctx, torch.from_numpy(text).cuda(), torch.from_numpy(sorted_sa(text).astype(np.int32)).cuda(), prefix_table=False)
    B = probe.fm_device(0).info["block"]
    probe.close()
    assert B == 96
    for s in (B - 1, B, B + 1, 2 * B, 64, 65, T, T + 1, 2 * B + T):
        text = random_text(s, s)
        sa = sorted_sa(text)
        w = Witness(text, sa)
        qs = query_set(w, B, seed=s, per_length=3)
        want = Wanted(w, qs)
        assert int(want.hi.max()) == s                               # occ(c, s) is asked for: the trailing block where s % B == 0
        for name, ix in wrapped(ctx, text, sa):
            check_index(ctx, ix, want, samples=(1, 5), tiles=(T,), tag=(s, name))
            everything = ix.fm_device(5)
            off, pos = everything.locate_device(torch.zeros(1, dtype=torch.int64, device="cuda"), torch.full((1,), s, dtype=torch.int64, device="cuda"))
            assert np.array_equal(_unsigned(pos), sa) and off.tolist() == [0, s], (s, name)       # every rank: the last mark word too
            ix.close()


# ---------------------------------------------------------------------------------------------------------------------
# the index owns what it reads
# ---------------------------------------------------------------------------------------------------------------------
def test_the_index_outlives_its_arrays(ctx):
    f, w = file_witness("long_dna_sequence_allow_ambiguity.sufr")
    want = Wanted(w, query_set(w, 96, seed=5))
    d_text = torch.from_numpy(np.array(f.text)).cuda()
    d_sa = torch.from_numpy(np.array(f.suffix_array).view(np.int32)).cuda()
    ix = DeviceIndex.wrap(ctx, d_text, d_sa, is_dna=True, prefix_table=False)
    a, b = ix.fm_device(32), ix.fm_device(32)
    assert a.info == b.info == f.fm(32).info                         # two builds, and the host's
    d_text.zero_()
    d_sa.zero_()
    torch.cuda.synchronize()
    check_fm(a, want, "zeroed a")
    check_fm(b, want, "zeroed b")
    ix.close()
    check_fm(a, want, "closed wrap")
    loaded = DeviceIndex.load(ctx, f)
    c = loaded.fm_device(7)
    loaded.close()
    f.close()
    check_fm(c, want, "closed load")


def test_partial_indexes_and_a_second_end_byte_are_refused(ctx):
    for name in ("long_dna_sequence.sufr", "uniprot-masked.sufr"):
        ix = DeviceIndex.load(ctx, SufrFile(EXP / name))
        with pytest.raises(SufrHipError) as err:
            ix.fm_device()
        assert err.value.code == UNSUPPORTED, name
        ix.close()
    text = np.frombuffer(b"ACGT$GATTACA$", dtype=np.uint8).copy()
    for name, ix in wrapped(ctx, text, sorted_sa(text)):
        with pytest.raises(SufrHipError) as err:
            ix.fm_device()
        assert err.value.code == UNSUPPORTED and "occurs 2 times" in str(err.value), name
        ix.close()
    capped = DeviceIndex.wrap(ctx, torch.from_numpy(text).cuda(), torch.from_numpy(sorted_sa(text).astype(np.int32)).cuda(), max_query_len=3,
                              prefix_table=False)
    with pytest.raises(SufrHipError) as err:
        capped.fm_device()
    assert err.value.code == UNSUPPORTED
    capped.close()


# ---------------------------------------------------------------------------------------------------------------------
# call shapes
# ---------------------------------------------------------------------------------------------------------------------
def test_capacity_max_hits_and_no_queries(ctx):
    f, w = file_witness("long_dna_sequence_allow_ambiguity.sufr")
    want = Wanted(w, query_set(w, 96))
    ix = DeviceIndex.load(ctx, f)
    dfm = ix.fm_device(7)
    ix.close()
    L = sufr_amd.lib()
    lo, hi = dfm.search_device(*want.batch)
    w_off, w_pos = want.located[3]
    z, nq = int(w_off[-1]), len(want.qs)
    assert z > 50
    FF = 0xFFFFFFFF
    off = torch.full((nq + 1,), -1, dtype=torch.int64, device="cuda")
    pos = torch.full((z + 9,), -1, dtype=torch.int32, device="cuda")
    total = C.c_uint64(0)
    args = (ctx.handle, dfm._h, lo.data_ptr(), hi.data_ptr(), nq, 3, off.data_ptr(), pos.data_ptr())
    assert L.sufr_hip_fm_locate_batch_device(*args, z - 1, C.byref(total)) == -5
    ctx.synchronize()
    assert total.value == z and (_unsigned(pos) == FF).all()         # no position written
    ctx.check(L.sufr_hip_fm_locate_batch_device(*args, z, C.byref(total)))
    ctx.synchronize()
    got = _unsigned(pos)
    assert total.value == z and np.array_equal(_unsigned(off), w_off) and np.array_equal(got[:z], w_pos) and (got[z:] == FF).all()
    # no queries: nothing is read, offsets[0] = 0
    ctx.check(L.sufr_hip_fm_search_batch_device(ctx.handle, dfm._h, None, None, 0, None, None))
    ctx.check(L.sufr_hip_fm_locate_batch_device(ctx.handle, dfm._h, None, None, 0, 0, off.data_ptr(), None, 0, C.byref(total)))
    ctx.synchronize()
    assert total.value == 0 and off[0].item() == 0 and off[1].item() == int(w_off[1])
    none = dfm.search_device(torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))
    assert none[0].numel() == 0
    # the convenience calls
    assert [p.tolist() for p in dfm.locate([b"ACGT", b""], max_hits=2)] == [w.sa[a:min(b, a + 2)].tolist() for a, b in (w.search(b"ACGT")[:2], (0, w.s))]
    assert [c.count for c in dfm.count([b"AC", b"ZZ"])] == [c.count for c in f.count([b"AC", b"ZZ"])]
    glo, ghi = dfm.search([b"AC"])
    assert (int(glo[0]), int(ghi[0])) == w.search(b"AC")[:2]


def test_two_contexts_on_two_threads(ctx):
    """two contexts, each with the FM-index of a different file, build and answer at once on two host threads"""
    names = ["uniprot.sufr", "long_dna_sequence_allow_ambiguity.sufr"]
    pairs = [file_witness(n) for n in names]
    wants = [Wanted(w, query_set(w, 96 if n.startswith("long") else 160, seed=2)) for n, (f, w) in zip(names, pairs)]
    other = sufr_amd.Context(0)
    other.set_bwt_tile(T)
    errors = []

    def work(c, f, want):
        try:
            for _ in range(3):
                ix = DeviceIndex.load(c, f)
                dfm = ix.fm_device(7)
                ix.close()
                check_fm(dfm, want)
                dfm.close()
        except BaseException as e:                                   # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=work, args=(c, f, want)) for c, (f, w), want in zip((ctx, other), pairs, wants)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    other.close()
    assert not errors, errors


def test_cli_fm_on_the_device_prints_the_host_lines():
    from test_match_host import run
    path = EXP / "long_dna_sequence_allow_ambiguity.sufr"
    queries = ["ACGT", "GATTACA", "N", "TTTTTTTTTTTTTTTTTTTTTTTTTT"]
    assert run("fm", "--device", 0, path, *queries).stdout == run("count", path, *queries).stdout != ""
    want, got = run("locate", path, *queries), run("fm", "--locate", "--device", 0, path, *queries)
    assert got.stdout == want.stdout != "" and got.stderr == want.stderr


def test_cli_fm_locate_with_max_hits_on_the_device_prints_the_host_lines():
    """the device locate that --locate and --smems share, cut at --max-hits"""
    from test_match_host import run
    path = EXP / "2ns.sufr"
    for flags in (("--max-hits", 2), ("--max-hits", 2, "-a", "-s", 3)):
        want, got = run("fm", "--locate", *flags, path, "N", "ACGT", "TTT"), run("fm", "--locate", *flags, "--device", 0, path, "N", "ACGT", "TTT")
        assert got.stdout == want.stdout != "" and got.stderr == want.stderr
