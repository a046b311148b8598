"""The BWT of the indexed text, its runs and the LF mapping on the GPU (include/sufr_bwt.h, sufr_bwt.inc) against the host path
of the same library and the numpy witness of tests/test_bwt_host.py.  Every comparison is exact array equality: the bytes,
the counts, the records and their order, the total, the stats and LF; on the loaded, the wrapped and the 64-bit index, at the
default tile and with the tile at its minimum, 256."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import sufr_amd
from sufr_amd import DeviceIndex, SufrFile, synth
from oracle_helper import GOLDEN, parse_sufr
from test_kmer_gpu import _dev, indexes, oracle_file
from test_lz_host import fibonacci
from test_bwt_host import STATS, edges, rotation, runs_of, text_for, witness

pytestmark = pytest.mark.gpu
EXP = GOLDEN / "expected"
T = 256                                                               # the smallest tile: one workgroup of ranks
TILES = (0, T)
LANES = 1024                                                          # lanes of the one workgroup that sweeps the tile summaries


@pytest.fixture(scope="module")
def ctx():
    c = sufr_amd.Context(0)
    yield c
    c.set_bwt_tile(0)
    c.close()


def _unsigned(t):
    a = t.cpu().numpy()
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).astype(np.uint64)


def check_index(ctx, ix: DeviceIndex, want, min_lens=(1,), tiles=TILES, tag=""):
    """bwt, counts, records, total, stats and lf of the device equal `want` (a witness at min_len 1) at every tile"""
    bwt, counts, records, stats, lf = want
    for tile in tiles:
        ctx.set_bwt_tile(tile)
        got_bwt, got_counts = ix.bwt_device()
        assert got_bwt.dtype == torch.uint8 and np.array_equal(got_bwt.cpu().numpy(), bwt), (tag, tile)
        assert np.array_equal(_unsigned(got_counts), counts), (tag, tile)
        for min_len in min_lens:
            keep = records[1] >= max(min_len, 1)
            got = ix.bwt_runs_device(min_len)
            for i in range(4):
                assert got[i].dtype == torch.int64 and np.array_equal(_unsigned(got[i]), records[i][keep]), (tag, tile, min_len, i)
            assert got[4] == dict(stats, records=int(keep.sum())), (tag, tile, min_len, got[4], stats)
        got_lf = ix.lf_device()
        assert got_lf.dtype == (torch.int64 if ix.index_width == 8 else torch.int32)
        assert np.array_equal(_unsigned(got_lf), lf), (tag, tile)
    ctx.set_bwt_tile(0)


def wrapped(ctx, text: np.ndarray, sa: np.ndarray):
    """(name, index) for the arrays wrapped with 32- and with 64-bit entries"""
    d_text = torch.from_numpy(np.ascontiguousarray(text, dtype=np.uint8)).cuda()
    yield "wrapped", DeviceIndex.wrap(ctx, d_text, _dev(sa.astype(np.uint32)), prefix_table=False)
    yield "wide", DeviceIndex.wrap(ctx, d_text, _dev(sa, True), prefix_table=False)


def check_arrays(ctx, text, sa, tag="", **kw):
    want = witness(text, sa)
    for name, ix in wrapped(ctx, text, sa):
        check_index(ctx, ix, want, tag=(tag, name), **kw)
        ix.close()
    return want


# ---------------------------------------------------------------------------------------------------------------------
# the golden files: s from 5 (one partial tile) to 63 220 (247 tiles of 256 with a ragged last one)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(p.name for p in EXP.glob("*.sufr")))
def test_device_equals_host_and_witness_on_golden_files(ctx, name):
    p = parse_sufr(EXP / name)
    want = witness(p.text, p.sa)
    f = SufrFile(EXP / name)
    host = f.bwt_runs()
    assert np.array_equal(f.bwt()[0], want[0]) and host[4] == want[3] and np.array_equal(f.lf().astype(np.uint64), want[4])
    for tag, ix, _ in indexes(ctx, f):                               # (the seed-mask file too: nothing is refused)
        check_index(ctx, ix, want, min_lens=(1, 0, 3), tag=(name, tag))
        ix.close()


def test_golden_sizes_cover_one_partial_tile_and_many_tiles():
    sizes = [parse_sufr(p).num_suffixes for p in EXP.glob("*.sufr")]
    assert min(sizes) < T and max(sizes) > 200 * T and max(sizes) % T != 0


# ---------------------------------------------------------------------------------------------------------------------
# runs against tile edges, with the tile at its minimum
# ---------------------------------------------------------------------------------------------------------------------
def test_one_run_over_several_whole_tiles(ctx, oracle, tmp_path):
    """A^1000 with every position indexed: the BWT is A^1000 $ -- one run over three whole tiles and a bit -- and the cyclic
    row is the last rank"""
    f = oracle_file(oracle, tmp_path, np.full(1000, ord("A"), dtype=np.uint8), "a", is_dna=True)
    sa = np.asarray(f.suffix_array)
    assert f.len_suffixes == f.text_len == 1001 and int(sa[0]) == 1000 and int(sa[1000]) == 0
    want = witness(np.asarray(f.text), sa)
    assert [a.tolist() for a in want[2]] == [[0, 1000], [1000, 1], [ord("A"), ord("$")], [1000, 0]] and edges(want[2], T)[2] == 3
    assert want[3] == dict(runs=2, records=2, longest=1000, longest_rank=0)
    for tag, ix, _ in indexes(ctx, f):
        check_index(ctx, ix, want, min_lens=(1, 2, 1000, 1001), tag=tag)
        ix.close()


def periodic_texts():
    fib = fibonacci(3000)
    return {"fib": fib, "tandem": synth.adversarial("tandem", 3000, seed=3)[:-1],
            "fib_a": np.concatenate([fib, np.full(700, ord("A"), dtype=np.uint8)]), "runs": runs_of(b"ACGT", 3000, 40.0, seed=2),
            "long_runs": runs_of(b"AC", 3300, 300.0, seed=5)}


def test_periodic_texts_put_runs_on_the_tile_edges(ctx, oracle, tmp_path):
    """The witness says what the runs do at the multiples of 256; over the texts some run must begin exactly at one, some run
    must end exactly at one and some run must cover two whole tiles -- a condition of the test, checked on the CPU arrays"""
    seen = [False, False, 0]
    for name, body in periodic_texts().items():
        f = oracle_file(oracle, tmp_path, body, name, is_dna=True)
        assert f.len_suffixes > 3000
        want = witness(np.asarray(f.text), np.asarray(f.suffix_array))
        begins, ends, whole = edges(want[2], T)
        seen = [seen[0] or begins, seen[1] or ends, max(seen[2], whole)]
        for tag, ix, _ in indexes(ctx, f):
            if tag != "wrapped":
                check_index(ctx, ix, want, min_lens=(1, 2, 64), tiles=(T,), tag=(name, tag))
            ix.close()
    assert seen[0] and seen[1] and seen[2] >= 2, seen


def test_planted_runs_on_the_tile_edges(ctx):
    """the BWT written down first: a run that begins exactly at a multiple of 256, one that ends exactly at one, one that
    covers two whole tiles and ends in the middle of a third, single-rank runs on both sides of an edge"""
    n = 12 * T + 99
    bwt = runs_of(b"ACGT$N", n, 3.0, seed=4)
    bwt[2 * T:2 * T + 40] = ord("A"); bwt[2 * T - 1] = ord("C"); bwt[2 * T + 40] = ord("G")          # begins at 2 T
    bwt[4 * T - 30:4 * T] = ord("C"); bwt[4 * T - 31] = ord("A"); bwt[4 * T] = ord("T")               # ends at 4 T
    bwt[6 * T - 5:8 * T + 100] = ord("G"); bwt[6 * T - 6] = ord("T"); bwt[8 * T + 100] = ord("A")     # tiles 6 and 7 whole
    bwt[10 * T - 2:10 * T + 2] = np.frombuffer(b"ACGT", dtype=np.uint8)                              # single ranks at an edge
    for zero_at in (0, n - 1, 5 * T, 5 * T - 1, 777):                # the cyclic row: first, last, on either side of an edge
        sa = rotation(n, zero_at)
        assert int(sa[zero_at]) == 0
        want = check_arrays(ctx, text_for(bwt, sa), sa, tag=zero_at, min_lens=(1, 2, 41), tiles=(T,) if zero_at else TILES)
        assert np.array_equal(want[0], bwt)
    begins, ends, whole = edges(want[2], T)
    assert begins and ends and whole >= 2 and want[3]["longest"] == 2 * T + 105 and want[3]["longest_rank"] == 6 * T - 5


# ---------------------------------------------------------------------------------------------------------------------
# all 256 byte values
# ---------------------------------------------------------------------------------------------------------------------
def test_all_byte_values_and_a_sorted_array(ctx):
    rng = np.random.default_rng(11)
    text = rng.integers(0, 256, 5000).astype(np.uint8)
    text[:256] = np.arange(256)
    sa = np.array(sorted(range(text.size), key=lambda p: text[p:].tobytes()), dtype=np.uint32)      # (numpy has no suffix sort; 5 000 slices do)
    want = check_arrays(ctx, text, sa, tag="bytes")
    assert (want[1] > 0).all() and np.array_equal(np.sort(want[4]), np.arange(text.size))           # every byte value; LF is a permutation
    # one tile of a single symbol, which the next tile does not hold at all
    bwt = rng.integers(0, 256, 5000).astype(np.uint8)
    bwt[3 * T:4 * T] = 200
    nxt = bwt[4 * T:5 * T]
    nxt[nxt == 200] = 201
    sa = rng.permutation(5000).astype(np.uint32)
    want = check_arrays(ctx, text_for(bwt, sa), sa, tag="single")
    assert np.array_equal(want[0], bwt) and (bwt[3 * T:4 * T] == 200).all() and not (bwt[4 * T:5 * T] == 200).any()
    assert np.array_equal(np.sort(want[4]), np.arange(5000)) and int((want[1] > 0).sum()) == 256


# ---------------------------------------------------------------------------------------------------------------------
# more tiles than the sweeps have lanes, and more than one tile per workgroup
# ---------------------------------------------------------------------------------------------------------------------
def per_lane(ntiles: int) -> int:
    """tiles in the block of one lane of a sweep (tile_sweep of sufr_scan.inc: lane i takes tiles [i per, (i + 1) per))"""
    return (ntiles + LANES - 1) // LANES


def test_more_tiles_than_lanes_of_the_carry_sweep(ctx):
    """2049 x 256 + 44 ranks at tile 256: 2050 tiles, three to a lane of the sweep, the upper lanes without any and the last
    tile ragged; a run over 200 whole tiles crosses the boundaries of more than 60 lanes' blocks, and a run of exactly one
    whole tile ends exactly where one lane's block hands over to the next"""
    n = 2049 * T + 44
    ntiles = (n + T - 1) // T
    per = per_lane(ntiles)
    assert ntiles == 2050 and per == 3 and n % T != 0 and (ntiles + per - 1) // per < LANES
    bwt = runs_of(b"ACGT", n, 6.0, seed=9)
    hand = 500 * per * T                                             # the first rank of lane 500's block
    bwt[hand - 200 * T - 7:hand + 3 * T + 9] = ord("T"); bwt[hand - 200 * T - 8] = ord("A"); bwt[hand + 3 * T + 9] = ord("C")
    hand2 = 100 * per * T
    bwt[hand2 - T:hand2] = ord("G"); bwt[hand2 - T - 1] = ord("A"); bwt[hand2] = ord("C")               # a whole tile up to the hand-over
    sa = rotation(n, hand)
    want = witness(text_for(bwt, sa), sa)
    assert np.array_equal(want[0], bwt) and want[3]["longest"] == 203 * T + 16 and edges(want[2], T)[2] >= 200
    rank, length = want[2][0].astype(np.int64), want[2][1].astype(np.int64)
    long_run = int(np.argmax(length))
    assert (rank[long_run] + length[long_run]) // (per * T) - rank[long_run] // (per * T) > 60       # block boundaries inside the long run
    assert ((rank == hand2 - T) & (length == T)).any() and hand2 % (per * T) == 0
    for name, ix in wrapped(ctx, text_for(bwt, sa), sa):
        check_index(ctx, ix, want, min_lens=(1, 3), tiles=(T,) if name == "wide" else TILES, tag=name)
        ix.close()


@pytest.mark.parametrize("ntiles,per", [(1023, 1), (1024, 1), (1025, 2), (2050, 3)])
def test_sweeps_at_the_lane_count_of_the_workgroup(ctx, ntiles, per):
    """as many tiles of 256 as the sweeps have lanes, one fewer, one more and twice as many and a bit (from 1025 on the upper
    lanes have no tile); the last tile ragged.  One run over every tile, one run per tile that ends exactly at the tile's
    edge, and random runs"""
    n = (ntiles - 1) * T + 77
    assert (n + T - 1) // T == ntiles and per_lane(ntiles) == per and (ntiles <= LANES or (ntiles + per - 1) // per < LANES)
    one = np.full(n, ord("A"), dtype=np.uint8)
    one[0] = ord("C")
    at_edges = np.repeat(np.frombuffer(b"AC", dtype=np.uint8)[np.arange(ntiles) % 2], T)[:n].copy()
    at_edges[::T] = ord("G")                                          # (a single rank at every tile's start, the rest of the tile one run)
    sa = rotation(n, 3 * T + 5)
    for tag, bwt in (("one", one), ("edges", at_edges), ("random", runs_of(b"ACGT$N", n, 40.0, seed=ntiles))):
        text = text_for(bwt, sa)
        want = witness(text, sa)
        assert np.array_equal(want[0], bwt)
        rank, length = want[2][0].astype(np.int64), want[2][1].astype(np.int64)
        if tag == "one":
            assert edges(want[2], T)[2] == ntiles - 2 and int(length.max()) == n - 1
        if tag == "edges":
            assert set(((rank + length)[(rank + length) % T == 0] // T).tolist()) == set(range(1, ntiles))
        for name, ix in wrapped(ctx, text, sa):
            check_index(ctx, ix, want, tiles=(T,), tag=(ntiles, tag, name))
            ix.close()


# ---------------------------------------------------------------------------------------------------------------------
# call shapes
# ---------------------------------------------------------------------------------------------------------------------
def test_arrays_of_no_and_one_rank(ctx):
    """(the golden empty.fa is no way to an empty array: oracle and builder refuse an empty sequence file)"""
    text = torch.from_numpy(np.frombuffer(b"ACGTACGTAC$", dtype=np.uint8).copy()).cuda()
    for tile in TILES:
        ctx.set_bwt_tile(tile)
        for dt in (torch.int32, torch.int64):
            none = DeviceIndex.wrap(ctx, text, torch.zeros(0, dtype=dt, device="cuda"), prefix_table=False)
            bwt, counts = none.bwt_device()
            assert bwt.numel() == 0 and not counts.any().item() and none.lf_device().numel() == 0
            got = none.bwt_runs_device()
            assert all(t.numel() == 0 for t in got[:4]) and got[4] == dict.fromkeys(STATS, 0)
            none.close()
            for p, c in ((0, "$"), (3, "G")):
                one = DeviceIndex.wrap(ctx, text, torch.full((1,), p, dtype=dt, device="cuda"), prefix_table=False)
                bwt, counts = one.bwt_device()
                assert bwt.tolist() == [ord(c)] and counts[ord(c)].item() == 1 and counts.sum().item() == 1
                got = one.bwt_runs_device()
                assert [t.tolist() for t in got[:4]] == [[0], [1], [ord(c)], [p]] and got[4] == dict(runs=1, records=1, longest=1, longest_rank=0)
                assert one.lf_device().tolist() == [0]
                one.close()
    ctx.set_bwt_tile(0)


def test_capacity_counting_and_null_outputs(ctx):
    f = SufrFile(EXP / "long_dna_sequence.sufr")
    p = parse_sufr(EXP / "long_dna_sequence.sufr")
    bwt, counts, records, stats, lf = witness(p.text, p.sa)
    ix = DeviceIndex.load(ctx, f)
    L = sufr_amd.lib()
    z = stats["records"]
    assert z > 100
    FF = 0xFFFFFFFFFFFFFFFF
    out = [torch.full((z + 50,), -1, dtype=torch.int64, device="cuda") for _ in range(4)]           # 0xFF in every byte
    total, st = C.c_uint64(0), sufr_amd.BwtStats()
    args = (ctx.handle, ix._h)
    assert L.sufr_hip_bwt_runs_device(*args, 1, 0, None, None, None, None, C.byref(total), C.byref(st)) == -5     # the counting call
    assert total.value == z and st.as_dict() == stats
    total.value = 0
    assert L.sufr_hip_bwt_runs_device(*args, 1, z - 1, *(o.data_ptr() for o in out), C.byref(total), None) == -5
    ctx.synchronize()
    assert total.value == z and all((_unsigned(o) == FF).all() for o in out)                        # nothing written
    ctx.check(L.sufr_hip_bwt_runs_device(*args, 1, z + 50, *(o.data_ptr() for o in out), C.byref(total), C.byref(st)))
    ctx.synchronize()
    for i in range(4):
        got = _unsigned(out[i])
        assert np.array_equal(got[:z], records[i]) and (got[z:] == FF).all()
    assert total.value == z and st.as_dict() == stats
    assert L.sufr_hip_bwt_runs_device(*args, stats["longest"] + 1, 0, None, None, None, None, C.byref(total), C.byref(st)) == 0
    assert total.value == 0 and st.as_dict() == dict(stats, records=0)
    # NULL outputs are skipped: either output of the gather alone, none at all
    s = f.len_suffixes
    only_bwt = torch.full((s + 3,), 7, dtype=torch.uint8, device="cuda")
    only_counts = torch.full((256,), 7, dtype=torch.int64, device="cuda")
    ctx.check(L.sufr_hip_bwt_device(*args, only_bwt.data_ptr(), None))
    ctx.check(L.sufr_hip_bwt_device(*args, None, only_counts.data_ptr()))
    ctx.check(L.sufr_hip_bwt_device(*args, None, None))
    ctx.check(L.sufr_hip_lf_device(*args, None))
    ctx.synchronize()
    got = only_bwt.cpu().numpy()
    assert np.array_equal(got[:s], bwt) and (got[s:] == 7).all() and np.array_equal(_unsigned(only_counts), counts)
    ix.close()


def test_two_contexts_on_two_threads(ctx):
    """two contexts, each with its own index of a different file, work at once on two host threads"""
    names = ["uniprot.sufr", "long_dna_sequence.sufr"]
    files = [SufrFile(EXP / n) for n in names]
    want = [witness(p.text, p.sa) for p in (parse_sufr(EXP / n) for n in names)]
    other = sufr_amd.Context(0)
    other.set_bwt_tile(T)
    work_on = [(ctx, files[0]), (other, files[1])]
    results, errors = {}, []

    def work(i, c, f):
        try:
            ix = DeviceIndex.load(c, f)
            out = []
            for _ in range(4):
                bwt, counts = ix.bwt_device()
                got = ix.bwt_runs_device()
                out.append((bwt.cpu().numpy(), _unsigned(counts), [_unsigned(got[k]) for k in range(4)], got[4], _unsigned(ix.lf_device())))
            ix.close()
            results[i] = out
        except Exception as e:                                       # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=work, args=(i, c, f)) for i, (c, f) in enumerate(work_on)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    other.close()
    assert not errors, errors
    for i in range(2):
        for bwt, counts, cols, st, lf in results[i]:
            assert np.array_equal(bwt, want[i][0]) and np.array_equal(counts, want[i][1]) and np.array_equal(lf, want[i][4])
            assert all(np.array_equal(cols[k], want[i][2][k]) for k in range(4)) and st == want[i][3]


def test_lf_is_the_same_bits_on_every_run(ctx):
    f = SufrFile(EXP / "uniprot.sufr")
    ix = DeviceIndex.load(ctx, f)
    ctx.set_bwt_tile(T)
    a, b = ix.lf_device(), ix.lf_device()
    ctx.set_bwt_tile(0)
    assert a.data_ptr() != b.data_ptr() and torch.equal(a, b) and np.array_equal(_unsigned(a), f.lf().astype(np.uint64))
    ix.close()


def test_cli_bwt_on_the_device_prints_the_host_bytes(tmp_path):
    from test_match_host import run
    for name in ("uniprot.sufr", "3.sufr", "uniprot-masked.sufr"):
        host = run("bwt", "--runs", "--min-len", 2, EXP / name).stdout
        assert host.count("\n") > 8 and host == run("bwt", "--runs", "--min-len", 2, "--device", 0, EXP / name).stdout
    files = [tmp_path / n for n in ("h.tsv", "h.bwt", "h.lf", "d.tsv", "d.bwt", "d.lf")]
    assert run("bwt", "-o", files[0], "--bwt", files[1], "--lf", files[2], EXP / "uniprot.sufr").stdout == ""
    assert run("bwt", "-o", files[3], "--bwt", files[4], "--lf", files[5], "--device", 0, EXP / "uniprot.sufr").stdout == ""
    for k in range(3):
        assert files[k].read_bytes() == files[k + 3].read_bytes() != b""
