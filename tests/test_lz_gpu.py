"""Longest previous factors and the LZ77 parse on the GPU (include/sufr_lz.h, sufr_lz.inc) against the host path of the same
library, which tests/test_lz_host.py holds to a quadratic witness without suffix array or LCP.  Every comparison is exact
array equality: LPF and SRC of every position, the records and their order, the total and the stats; on the loaded, the
wrapped and the 64-bit index, at the default tiles and with both tiles at their minimum, 256."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import sufr_amd
from sufr_amd import DeviceIndex, SufrFile, synth
from oracle_helper import GOLDEN
from test_gpu_match import _write
from test_kmer_gpu import _dev, indexes, oracle_file
from test_lz_host import FF, distinct_file, fibonacci, letters

pytestmark = pytest.mark.gpu
EXP = GOLDEN / "expected"
T = 256                                                               # the smallest tile: one workgroup of ranks or positions
TILES = ((0, 0), (T, T))


@pytest.fixture(scope="module")
def ctx():
    c = sufr_amd.Context(0)
    yield c
    c.set_lz_tile(0, 0)
    c.close()


def _unsigned(t, none_to_ff=False):
    a = t.cpu().numpy()
    a = a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)
    out = a.astype(np.uint64)
    if none_to_ff:
        out[a == np.iinfo(a.dtype).max] = FF
    return out


def host_results(f: SufrFile):
    lpf, src = f.lpf()
    return lpf.astype(np.uint64), np.where(src == np.iinfo(src.dtype).max, FF, src.astype(np.uint64)).astype(np.uint64), f.lz()


def same_as_host(ctx, f: SufrFile, want=None, tiles=TILES, which=("loaded", "wrapped", "wide"), tag=""):
    """LPF, SRC, records, total and stats of the device equal the host's on every index and tile; returns the host's"""
    want = want or host_results(f)
    for name, ix, lcp in indexes(ctx, f):
        if name in which:
            for tile in tiles:
                ctx.set_lz_tile(*tile)
                lpf, src = ix.lpf_device(lcp, f.sequence_starts)
                assert np.array_equal(_unsigned(lpf), want[0]), (tag, name, tile)
                assert np.array_equal(_unsigned(src, True), want[1]), (tag, name, tile)
                got = ix.lz_device(lcp, f.sequence_starts)
                for i in range(3):
                    assert np.array_equal(got[i].cpu().numpy().view(np.uint64), want[2][i]), (tag, name, tile, i)
                assert got[3] == want[2][3], (tag, name, tile, got[3], want[2][3])
        ix.close()
    ctx.set_lz_tile(0, 0)
    return want


@pytest.mark.parametrize("name", sorted(p.name for p in EXP.glob("*.sufr")))
def test_device_equals_host_on_golden_files(ctx, name):
    f = SufrFile(EXP / name)
    if f.seed_mask:                                                  # refusals return the host's codes
        ix = DeviceIndex.load(ctx, f)
        lcp = _dev(np.asarray(f.lcp))
        for call in (f.lpf, f.lz, lambda: ix.lpf_device(lcp, f.sequence_starts), lambda: ix.lz_device(lcp, f.sequence_starts)):
            with pytest.raises(sufr_amd.SufrHipError) as e:
                call()
            assert e.value.code == -6
        ix.close()
        return
    want = same_as_host(ctx, f, tag=name)
    assert want[2][3]["factors"] >= 3


def test_refusals_and_bad_starts(ctx, oracle, tmp_path):
    f = oracle_file(oracle, tmp_path, synth.adversarial("tandem", 1200, seed=3)[:-1], is_dna=True, max_query_len=6)
    ix = DeviceIndex.load(ctx, f)
    lcp = _dev(np.asarray(f.lcp))
    for call in (f.lpf, f.lz, lambda: ix.lpf_device(lcp), lambda: ix.lz_device(lcp)):
        with pytest.raises(sufr_amd.SufrHipError) as e:
            call()
        assert e.value.code == -6
    ix.close()
    g = SufrFile(EXP / "3.sufr")
    ix = DeviceIndex.load(ctx, g)
    lcp = _dev(np.asarray(g.lcp))
    L = sufr_amd.lib()
    total, st = C.c_uint64(7), sufr_amd.LzStats()
    out = torch.full((2 * g.text_len,), -1, dtype=torch.int32, device="cuda")
    for bad in ([1, 5], [0, 5, 5], [0, 9, 5], [0, g.text_len]):
        starts = np.array(bad, dtype=np.uint64)
        total.value = 7
        assert L.sufr_hip_lz_device(ctx.handle, ix._h, lcp.data_ptr(), starts.ctypes.data, starts.size, 0, None, None, None, C.byref(total),
                                    C.byref(st)) == -1, bad
        assert total.value == 0 and st.as_dict() == dict(factors=0, literals=0, longest=0, longest_start=0)
        assert L.sufr_hip_lpf_device(ctx.handle, ix._h, lcp.data_ptr(), starts.ctypes.data, starts.size, out.data_ptr(),
                                     out.data_ptr() + 4 * g.text_len) == -1, bad
    ctx.synchronize()
    ix.close()


# ---------------------------------------------------------------------------------------------------------------------
# tile boundaries, with both tiles at their minimum
# ---------------------------------------------------------------------------------------------------------------------
def test_all_a_searches_and_a_factor_over_many_tiles(ctx, oracle, tmp_path):
    """A^3000: the suffix array descends, so every left search runs to the array's start -- over more than 8 rank tiles from
    the far ranks -- and finds nothing, and every right search ends next door; the one long factor jumps over more than 8
    whole position tiles, which the chain leaves without an entry; the last tile of either kind is partial"""
    f = oracle_file(oracle, tmp_path, np.full(3000, ord("A"), dtype=np.uint8), "a", is_dna=True)
    sa = np.asarray(f.suffix_array).astype(np.int64)
    n = f.text_len
    assert f.len_suffixes == n == 3001 and n % T != 0 and n > 9 * T and np.array_equal(sa, np.arange(n)[::-1])
    want = same_as_host(ctx, f, tag="all_a")
    start, length, source, st = want[2]
    assert [start.tolist(), length.tolist(), source.tolist()] == [[0, 1, 3000], [1, 2999, 1], [FF, 0, FF]]
    entered = set((start // T).tolist())
    assert len(set(range(n // T + 1)) - entered) > 8 and entered == {0, n // T}
    assert st == dict(factors=3, literals=2, longest=2999, longest_start=1)
    assert np.array_equal(want[0][1:-1], np.arange(2999, 0, -1)) and (want[1][1:-1] == np.arange(2999)).all()


def test_short_text_and_exact_multiple_of_the_tile(ctx, oracle, tmp_path):
    short = oracle_file(oracle, tmp_path, letters(b"ACGT", 99, 1), "short", is_dna=True)
    assert short.text_len == 100 < T
    same_as_host(ctx, short, tag="short")
    exact = oracle_file(oracle, tmp_path, letters(b"ACGT", 4 * T - 1, 2), "exact", is_dna=True)
    assert exact.text_len == exact.len_suffixes == 4 * T
    want = same_as_host(ctx, exact, tag="exact")
    assert set((want[2][0] // T).tolist()) == {0, 1, 2, 3}


def planted_body():
    """A random four-letter text with symbols that occur nowhere before them (a first occurrence is a literal and no copy
    runs over it) and with copies of earlier stretches, so that the factors at the boundaries of the 256-position tiles are
    known exactly"""
    body = letters(b"ACGT", 1300, 12).copy()
    fresh = iter(b"DEFHIKLMNPQRSVWY")
    body[T] = next(fresh)                                            # a literal at a tile's first position
    body[2 * T - 1] = next(fresh)                                    # ... and at a tile's last
    body[699] = next(fresh)                                          # the factor after it starts at 700 ...
    body[700:3 * T] = body[100:168]                                  # ... is this copy of 68 symbols ...
    body[3 * T] = next(fresh)                                        # ... and ends exactly at the tile's end: the next entry is offset 0
    body[4 * T - 2] = next(fresh)                                    # the factor after it starts at the last position of a tile
    body[4 * T - 1:4 * T + 9] = body[200:210]
    body[4 * T + 9] = next(fresh)
    return body


def test_planted_factors_at_tile_boundaries(ctx, oracle, tmp_path):
    f = oracle_file(oracle, tmp_path, planted_body(), "planted", is_dna=False)
    assert f.len_suffixes == f.text_len == 1301
    want = same_as_host(ctx, f, tag="planted")
    start, length, source, _ = want[2]
    recs = {int(p): (int(ln), int(q)) for p, ln, q in zip(start, length, source)}
    assert recs[T] == (1, FF) and recs[2 * T - 1] == (1, FF)           # literals at a tile's first and last position
    assert recs[700][0] == 68 and recs[700][1] < 700 and recs[3 * T] == (1, FF)      # a copy that ends exactly at a tile end; the next entry is offset 0
    assert recs[4 * T - 1][0] == 10 and recs[4 * T - 1][1] < 4 * T - 1               # a copy that starts at the last position of a tile
    assert 4 * T not in recs                                         # (that tile is entered at offset 9)


def test_other_texts(ctx, oracle, tmp_path):
    sep = np.frombuffer(b"%", dtype=np.uint8)
    piece = letters(b"ACGT", 150, 7)
    n_runs = np.concatenate([letters(b"ACGT", 700, 6), np.full(300, ord("N"), dtype=np.uint8), letters(b"ACGT", 600, 6), np.full(5, ord("N"), dtype=np.uint8),
                             sep, letters(b"ACGTN", 500, 8)])
    texts = {"fib": fibonacci(3000), "acgt_k": np.tile(np.frombuffer(b"ACGT", dtype=np.uint8), 750), "random4": letters(b"ACGT", 5000, 2),
             "identical": np.concatenate([np.concatenate([piece, sep]) for _ in range(20)])[:-1], "n_runs": n_runs}
    seen = {}
    for name, body in texts.items():
        f = oracle_file(oracle, tmp_path, body, name, is_dna=True)
        want = same_as_host(ctx, f, which=("loaded", "wide"), tag=name)
        seen[name] = (f, want[2])
    f, (start, length, source, st) = seen["fib"]
    assert st["factors"] < 40 and st["longest"] > 900                # few, long, nested factors
    f, (start, length, source, st) = seen["acgt_k"]
    assert [start.tolist(), length.tolist(), source.tolist()] == [[0, 1, 2, 3, 4, 3000], [1, 1, 1, 1, 2996, 1], [FF, FF, FF, FF, 0, FF]]
    f, (start, length, source, st) = seen["random4"]
    assert st["factors"] > 700 and set((start // T).tolist()) == set(range(f.text_len // T + 1))      # many short factors, every tile entered
    f, (start, length, source, st) = seen["identical"]
    assert f.num_sequences == 20
    for i in range(1, 20):                                           # every later sequence is one copy out of an earlier one, clipped at its break
        k = int(np.nonzero(start == f.sequence_starts[i])[0][0])
        assert int(length[k]) == 150 and int(source[k]) < f.sequence_starts[i] and int(source[k]) % 151 == 0
    f, (start, length, source, st) = seen["n_runs"]
    unindexed = np.ones(f.text_len, dtype=bool)
    unindexed[np.asarray(f.suffix_array).astype(np.int64)] = False
    at = unindexed[start.astype(np.int64)]
    assert f.len_suffixes < f.text_len - 300 and at.sum() >= 300 and (source[at] == FF).all()      # a tile and more of literals at positions that are not indexed


def test_more_parse_tiles_than_the_stats_reduction_has_lanes(tmp_path):
    """524 621 bases sorted on the device, against the host path through a written file: 2050 parse tiles of 256 positions,
    two or three to every lane of the reduction that gives the stats (the last tile ragged), and as many rank tiles"""
    n = 2049 * T + 77
    x, _ = synth.syn_elegans(n - 1, seed=7, n_seqs=1, device="cuda")
    norm = torch.where((x >= 97) & (x <= 122), x - 32, x).contiguous()
    assert norm.numel() == n and (n + T - 1) // T == 2050
    db = sufr_amd.DeviceBuilder(0)
    sa, lcp = db.sort(norm, is_dna=True)
    _write(tmp_path / "x.sufr", norm.cpu().numpy(), sa.cpu().numpy().view(np.uint32).copy(), lcp.cpu().numpy().view(np.uint32).copy())
    f = SufrFile(tmp_path / "x.sufr")
    want = f.lz(threads=16)
    entered = set((want[0] // T).tolist())
    assert want[3]["factors"] > 2050 and 1024 < len(entered) and {0, 2049} <= entered          # more entered tiles than lanes, the last one too
    db.ctx.set_lz_tile(T, T)
    for wide, d_sa, d_lcp in ((False, sa, lcp), (True, sa.to(torch.int64), lcp.to(torch.int64))):      # (both are below 2^31)
        ix = DeviceIndex.wrap(db.ctx, norm, d_sa, is_dna=True, prefix_table=False)
        got = ix.lz_device(d_lcp, f.sequence_starts)
        for i in range(3):
            assert np.array_equal(got[i].cpu().numpy().view(np.uint64), want[i]), (wide, i)
        assert got[3] == want[3], (wide, got[3], want[3])
        ix.close()
    db.ctx.set_lz_tile(0, 0)
    f.close(); db.close()


def test_pairwise_different_bytes_are_all_literals(ctx, tmp_path):
    """255 pairwise different bytes and the sentinel: there are no more different bytes than that"""
    f = distinct_file(tmp_path / "distinct.sufr", 255)
    want = same_as_host(ctx, f, tag="distinct")
    assert want[2][3] == dict(factors=256, literals=256, longest=1, longest_start=0) and not want[0].any()


# ---------------------------------------------------------------------------------------------------------------------
# capacity and call shapes
# ---------------------------------------------------------------------------------------------------------------------
def test_capacity_and_untouched_outputs(ctx):
    f = SufrFile(EXP / "long_dna_sequence.sufr")
    ix = DeviceIndex.load(ctx, f)
    lcp = _dev(np.asarray(f.lcp))
    L = sufr_amd.lib()
    want = f.lz()
    z = want[3]["factors"]
    assert z > 100
    out = [torch.full((z + 50,), -1, dtype=torch.int64, device="cuda") for _ in range(3)]           # 0xFF in every byte
    total, st = C.c_uint64(0), sufr_amd.LzStats()
    args = (ctx.handle, ix._h, lcp.data_ptr(), None, 0)
    assert L.sufr_hip_lz_device(*args, 0, None, None, None, C.byref(total), C.byref(st)) == -5       # the counting call
    assert total.value == z and st.as_dict() == want[3]
    total.value = 0
    assert L.sufr_hip_lz_device(*args, z - 1, *(o.data_ptr() for o in out), C.byref(total), None) == -5
    ctx.synchronize()
    assert total.value == z and all((o.cpu().numpy().view(np.uint64) == FF).all() for o in out)     # nothing written
    ctx.check(L.sufr_hip_lz_device(*args, z + 50, *(o.data_ptr() for o in out), C.byref(total), C.byref(st)))
    ctx.synchronize()
    for i in range(3):
        got = out[i].cpu().numpy().view(np.uint64)
        assert np.array_equal(got[:z], want[i]) and (got[z:] == FF).all()
    assert total.value == z and st.as_dict() == want[3]
    # either array of the table alone
    n = f.text_len
    one = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                                         # (the fill runs on torch's stream, the call on the context's own)
    ctx.check(L.sufr_hip_lpf_device(*args, one.data_ptr(), None))
    ctx.synchronize()
    assert np.array_equal(_unsigned(one), f.lpf()[0].astype(np.uint64))
    ctx.check(L.sufr_hip_lpf_device(*args, None, one.data_ptr()))
    ctx.synchronize()
    assert np.array_equal(_unsigned(one), f.lpf()[1].astype(np.uint64))
    ix.close()


def test_an_empty_suffix_array_is_all_literals(ctx):
    text = torch.from_numpy(np.frombuffer(b"ACGTACGTAC" * 60 + b"$", dtype=np.uint8).copy()).cuda()
    n = text.numel()
    for tile in TILES:
        ctx.set_lz_tile(*tile)
        for wide in (False, True):
            dt = torch.int64 if wide else torch.int32
            ix = DeviceIndex.wrap(ctx, text, torch.zeros(0, dtype=dt, device="cuda"), prefix_table=False)
            lcp = torch.zeros(0, dtype=dt, device="cuda")
            lpf, src = ix.lpf_device(lcp)
            assert not _unsigned(lpf).any() and (_unsigned(src, True) == FF).all() and lpf.numel() == n
            start, length, source, st = ix.lz_device(lcp)
            assert np.array_equal(start.cpu().numpy(), np.arange(n)) and (length == 1).all() and (source == -1).all()
            assert st == dict(factors=n, literals=n, longest=1, longest_start=0)
            ix.close()
    ctx.set_lz_tile(0, 0)


def test_two_contexts_on_two_threads(ctx):
    """two contexts, each with its own index of a different file, parse at once on two host threads"""
    files = [SufrFile(EXP / "uniprot.sufr"), SufrFile(EXP / "long_dna_sequence.sufr")]
    want = [host_results(f) for f in files]
    other = sufr_amd.Context(0)
    other.set_lz_tile(T, T)
    work_on = [(ctx, files[0]), (other, files[1])]
    results, errors = {}, []

    def work(i, c, f):
        try:
            ix = DeviceIndex.load(c, f)
            lcp = _dev(np.asarray(f.lcp))
            out = []
            for _ in range(4):
                lpf, src = ix.lpf_device(lcp, f.sequence_starts)
                got = ix.lz_device(lcp, f.sequence_starts)
                out.append((_unsigned(lpf), _unsigned(src, True), [got[k].cpu().numpy().view(np.uint64) for k in range(3)], got[3]))
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
        for lpf, src, cols, st in results[i]:
            assert np.array_equal(lpf, want[i][0]) and np.array_equal(src, want[i][1])
            assert all(np.array_equal(cols[k], want[i][2][k]) for k in range(3)) and st == want[i][2][3]


def test_cli_lz_on_the_device_prints_the_host_bytes():
    from test_match_host import run
    for name in ("uniprot.sufr", "3.sufr"):
        host = run("lz", EXP / name).stdout
        assert host.count("\n") > 4 and host == run("lz", "--device", 0, EXP / name).stdout
    host = run("lz", "--lpf", EXP / "2d.sufr").stdout
    assert host.count("\n") > 4 and host == run("lz", "--lpf", "--device", 0, EXP / "2d.sufr").stdout


def test_cli_lz_on_the_device_to_a_file_and_refused(tmp_path):
    from test_match_host import run
    a, b = tmp_path / "host.tsv", tmp_path / "dev.tsv"
    assert run("lz", "-o", a, EXP / "uniprot.sufr").stdout == run("lz", "-o", b, "--device", 0, EXP / "uniprot.sufr").stdout == ""
    assert a.read_bytes() == b.read_bytes() != b""
    r = run("lz", "--device", 0, EXP / "uniprot-masked.sufr", check=False)
    assert r.returncode == 1 and r.stderr.startswith("Error: ") and "uniprot-masked.sufr" in r.stderr
