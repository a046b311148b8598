"""k-mer spectra, occurrence maps and unique lengths on the GPU (include/sufr_kmer.h, sufr_kmer.inc) against the host path of
the same library, which tests/test_kmer_host.py holds to a witness.  Every comparison is exact array equality."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import sufr_amd
from sufr_amd import DeviceIndex, SufrFile, synth
from oracle_helper import GOLDEN
from test_gpu_match import _write
from test_mem_host import _adversarial_body, _fasta_from

pytestmark = pytest.mark.gpu
EXP = GOLDEN / "expected"
KS = (1, 2, 3, 8, 21)
BINS = (1, 2, 256)
T = 256                                                               # the smallest tile: one workgroup of ranks
LDS_BINS = 1024                                                       # KMER_LDS_BINS of sufr_kmer.inc


@pytest.fixture(scope="module")
def ctx():
    c = sufr_amd.Context(0)
    yield c
    c.close()


def _dev(a: np.ndarray, wide=False):
    a = np.asarray(a)
    if wide or a.dtype.itemsize == 8:
        return torch.from_numpy(a.astype(np.int64)).cuda()
    return torch.from_numpy(a.astype(np.uint32).view(np.int32).copy()).cuda()


def _host(t):
    a = t.cpu().numpy()
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32).astype(np.uint64)


def indexes(ctx, f: SufrFile):
    """(index, lcp tensor) for the loaded file, the wrapped arrays, and the wrapped arrays widened to 64 bits"""
    text = torch.from_numpy(np.asarray(f.text).copy()).cuda()
    sa, lcp = np.asarray(f.suffix_array), np.asarray(f.lcp)
    yield "loaded", DeviceIndex.load(ctx, f), _dev(lcp)
    yield "wrapped", DeviceIndex.wrap(ctx, text, _dev(sa), max_query_len=f.max_query_len, is_dna=f.is_dna, prefix_table=False), _dev(lcp)
    yield "wide", DeviceIndex.wrap(ctx, text, _dev(sa, True), max_query_len=f.max_query_len, is_dna=f.is_dna, prefix_table=False), _dev(lcp, True)


def same_as_host(f: SufrFile, ix: DeviceIndex, lcp, ks, bins_list=(256,), unique=True, tag=""):
    starts = f.sequence_starts
    for k in ks:
        for bins in bins_list:
            for occ in ("rank", "position", None):
                h, st, o = f.kmers(k, bins, occ)
                dh, dst, do = ix.kmers_device(lcp, k, bins, occ, starts)
                assert np.array_equal(_host(dh), h), (tag, k, bins, occ)
                assert dst == st, (tag, k, bins, occ, dst, st)
                assert (o is None and do is None) or np.array_equal(_host(do), o.astype(np.uint64)), (tag, k, bins, occ)
    if unique:
        for by_pos in (False, True):
            assert np.array_equal(_host(ix.unique_lengths_device(lcp, by_pos, starts)), f.unique_lengths(by_pos).astype(np.uint64)), (tag, by_pos)


@pytest.mark.parametrize("name", sorted(p.name for p in EXP.glob("*.sufr")))
def test_device_equals_host_on_golden_files(ctx, name):
    f = SufrFile(EXP / name)
    above = int(np.asarray(f.lcp).max()) + 1
    for tag, ix, lcp in indexes(ctx, f):
        if f.seed_mask:
            if tag == "loaded":
                for call in (lambda: ix.kmers_device(lcp, 3), lambda: ix.unique_lengths_device(lcp)):
                    with pytest.raises(sufr_amd.SufrHipError) as e:
                        call()
                    assert e.value.code == -6
            ix.close()
            continue
        for tile in (0, T):
            ctx.set_kmer_tile(tile)
            same_as_host(f, ix, lcp, KS + (above,), BINS, tag=(tag, tile))
        ctx.set_kmer_tile(0)
        with pytest.raises(sufr_amd.SufrHipError) as e:
            ix.kmers_device(lcp, 0)
        assert e.value.code == -1
        ix.close()


def test_refusals_return_the_host_codes(ctx, oracle, tmp_path):
    _fasta_from(_adversarial_body("tandem"), tmp_path / "x.fa")
    oracle.create(tmp_path / "x.fa", tmp_path / "x.sufr", is_dna=True, max_query_len=6)
    f = SufrFile(tmp_path / "x.sufr")
    ix = DeviceIndex.load(ctx, f)
    lcp = _dev(np.asarray(f.lcp))
    same_as_host(f, ix, lcp, (1, 3, 6), unique=False)
    for call in (lambda: ix.kmers_device(lcp, 7), lambda: ix.unique_lengths_device(lcp), lambda: f.kmers(7), lambda: f.unique_lengths()):
        with pytest.raises(sufr_amd.SufrHipError) as e:
            call()
        assert e.value.code == -6
    ix.close()
    g = SufrFile(EXP / "3.sufr")
    ix = DeviceIndex.load(ctx, g)
    lcp = _dev(np.asarray(g.lcp))
    L = sufr_amd.lib()
    hist = torch.zeros(4, dtype=torch.int64, device="cuda")
    assert L.sufr_hip_kmers_device(ctx.handle, ix._h, lcp.data_ptr(), None, 0, 3, 0, 0, hist.data_ptr(), None, None) == -1     # no bins
    for bad in ([1, 5], [0, 5, 5], [0, 9, 5], [0, g.text_len]):
        st = np.array(bad, dtype=np.uint64)
        assert L.sufr_hip_kmers_device(ctx.handle, ix._h, lcp.data_ptr(), st.ctypes.data, st.size, 3, 0, 4, hist.data_ptr(), None, None) == -1, bad
        assert L.sufr_hip_unique_lengths_device(ctx.handle, ix._h, lcp.data_ptr(), st.ctypes.data, st.size, 0, hist.data_ptr()) == -1, bad
    ctx.synchronize()
    ix.close()


# ---------------------------------------------------------------------------------------------------------------------
# tile boundaries, with the tile at its minimum
# ---------------------------------------------------------------------------------------------------------------------
def oracle_file(oracle, tmp_path, body, name="x", **build):
    _fasta_from(body, tmp_path / f"{name}.fa")
    oracle.create(tmp_path / f"{name}.fa", tmp_path / f"{name}.sufr", **build)
    return SufrFile(tmp_path / f"{name}.sufr")


def longest_interval(lcp: np.ndarray, k: int) -> int:
    """ranks of the longest k-interval"""
    heads = np.concatenate([[0], np.nonzero(lcp[1:] < k)[0] + 1, [lcp.size]])
    return int(np.diff(heads).max())


def boundary_ks(lcp: np.ndarray, t: int):
    """(k of an interval that begins exactly at a tile boundary, k of one that ends exactly at one), None where there is none"""
    begin = end = None
    for j in range(1, (lcp.size - 2) // t + 1):
        b = j * t
        if begin is None and lcp[b] < lcp[b + 1]:
            begin = int(lcp[b + 1])                                  # LCP[jt] < k <= LCP[jt + 1]
        if end is None and lcp[b - 1] > lcp[b]:
            end = int(lcp[b - 1])                                    # LCP[jt - 1] >= k > LCP[jt]: ranks jt - 2, jt - 1 end there
    return begin, end


def test_intervals_across_tiles(ctx, oracle, tmp_path):
    ctx.set_kmer_tile(T)
    try:
        # one interval over at least 8 tiles; tiles without a head; a partial last tile
        body = np.full(3000, ord("A"), dtype=np.uint8)
        f = oracle_file(oracle, tmp_path, body, "a", is_dna=True)
        lcp = np.asarray(f.lcp).astype(np.int64)
        assert longest_interval(lcp, 5) >= 8 * T and f.len_suffixes % T != 0
        heads = np.concatenate([[True], lcp[1:] < 5])
        assert any(not heads[a:a + T].any() for a in range(0, lcp.size - T, T))
        ix = DeviceIndex.load(ctx, f)
        same_as_host(f, ix, _dev(np.asarray(f.lcp)), (5, 1, 2999, 3001), (2, 256, LDS_BINS + 3976))
        assert f.kmers(5, 2)[0].tolist() == [0, 1]                   # AAAAA alone, 2996 times: the saturating bin
        ix.close()
        # intervals that begin and end exactly at tile boundaries; tiles of heads only
        begun = ended = only_heads = False
        for kind in ("tandem", "acgt_k"):
            body = synth.adversarial(kind, 3000, seed=3)[:-1]
            f = oracle_file(oracle, tmp_path, body, kind, is_dna=True)
            lcp = np.asarray(f.lcp).astype(np.int64)
            kb, ke = boundary_ks(lcp, T)
            ks = sorted({k for k in (kb, ke) if k})
            for k in ks:
                h = np.concatenate([[True], lcp[1:] < k])
                only_heads = only_heads or any(h[a:a + T].all() for a in range(0, lcp.size - T, T))
            begun, ended = begun or kb is not None, ended or ke is not None
            ix = DeviceIndex.load(ctx, f)
            same_as_host(f, ix, _dev(np.asarray(f.lcp)), ks + [int(lcp.max()) + 1], (256,))
            ix.close()
        assert begun and ended and only_heads
    finally:
        ctx.set_kmer_tile(0)


def test_whole_and_other_ranks_of_an_interval_in_different_tiles(ctx, oracle, tmp_path):
    """an all-A text with positional sequence starts: the last k - 1 positions of every sequence are not whole and lie, tiles
    apart, in the one interval of the whole ranks"""
    from test_kmer_host import positional_breaks_file
    f = positional_breaks_file(oracle, tmp_path)
    k = 7
    lcp = np.asarray(f.lcp).astype(np.int64)
    occ = f.kmers(k, 256, "rank")[2]
    heads = np.concatenate([[0], np.nonzero(lcp[1:] < k)[0] + 1, [lcp.size]])
    a, b = max(zip(heads[:-1], heads[1:]), key=lambda ab: ab[1] - ab[0])
    tiles_zero = set(((np.nonzero(occ[a:b] == 0)[0] + a) // T).tolist())
    tiles_whole = set(((np.nonzero(occ[a:b] > 0)[0] + a) // T).tolist())
    assert len(tiles_zero) >= 2 and len(tiles_whole) >= 8 and f.num_sequences == 3
    ix = DeviceIndex.load(ctx, f)
    for tile in (T, 0):
        ctx.set_kmer_tile(tile)
        same_as_host(f, ix, _dev(np.asarray(f.lcp)), (k, 1, 2, 700), (1, 256))
    ctx.set_kmer_tile(0)
    ix.close()


def test_arrays_of_no_and_one_rank(ctx):
    for tile in (T, 0):
        ctx.set_kmer_tile(tile)
        text = torch.from_numpy(np.frombuffer(b"A$", dtype=np.uint8).copy()).cuda()
        one = DeviceIndex.wrap(ctx, text, torch.zeros(1, dtype=torch.int32, device="cuda"), prefix_table=False)
        lcp = torch.zeros(1, dtype=torch.int32, device="cuda")
        h, st, occ = one.kmers_device(lcp, 1, 3, "position")
        assert h.tolist() == [1, 0, 0] and st == dict(whole=1, distinct=1, unique=1, max_count=1) and occ.tolist() == [1, 0]
        h, st, occ = one.kmers_device(lcp, 2, 3, "rank")                # A$ holds the break
        assert h.tolist() == [0, 0, 0] and st == dict(whole=0, distinct=0, unique=0, max_count=0) and occ.tolist() == [0]
        assert one.unique_lengths_device(lcp).tolist() == [1]
        one.close()
        none = DeviceIndex.wrap(ctx, text, torch.zeros(0, dtype=torch.int32, device="cuda"), prefix_table=False)
        h, st, occ = none.kmers_device(torch.zeros(0, dtype=torch.int32, device="cuda"), 3, 4, None)
        assert h.tolist() == [0, 0, 0, 0] and st == dict(whole=0, distinct=0, unique=0, max_count=0) and occ is None
        none.close()
    ctx.set_kmer_tile(0)


def test_more_than_one_tile_per_workgroup(ctx, tmp_path):
    """1.5 M ranks with the tile at 256: more than twice as many tiles as the largest grid has workgroups"""
    wgs = torch.cuda.get_device_properties(0).multi_processor_count * 8
    n = 1_500_000
    assert n > 2 * wgs * T
    x, _ = synth.syn_elegans(n, seed=5, n_seqs=1, device="cuda")
    norm = torch.where((x >= 97) & (x <= 122), x - 32, x).contiguous()
    db = sufr_amd.DeviceBuilder(0)
    sa, lcp = db.sort(norm, is_dna=True)
    assert sa.numel() > 2 * wgs * T
    _write(tmp_path / "x.sufr", norm.cpu().numpy(), sa.cpu().numpy().view(np.uint32).copy(), lcp.cpu().numpy().view(np.uint32).copy())
    f = SufrFile(tmp_path / "x.sufr")
    ix = DeviceIndex.wrap(db.ctx, norm, sa, is_dna=True, prefix_table=False)
    for tile in (T, 0):
        db.ctx.set_kmer_tile(tile)
        for occ in ("rank", "position"):
            h, st, o = f.kmers(12, 256, occ, threads=16)
            dh, dst, do = ix.kmers_device(lcp, 12, 256, occ)
            assert np.array_equal(_host(dh), h) and dst == st and np.array_equal(_host(do), o.astype(np.uint64)), (tile, occ)
        assert st["max_count"] > 1 and st["unique"] > 0
    assert np.array_equal(_host(ix.unique_lengths_device(lcp, True)), f.unique_lengths(True, threads=16).astype(np.uint64))
    ix.close(); f.close(); db.close()


def kmer_witness(sa: np.ndarray, lcp: np.ndarray, n: int, k: int, bins: int):
    """(histogram, stats, occ by rank, occ by position) of one sequence of n symbols, by numpy"""
    sa, lcp = sa.astype(np.int64), lcp.astype(np.int64)
    interval = np.cumsum(np.concatenate([[True], lcp[1:] < k])) - 1
    whole = n - 1 - sa >= k
    count = np.bincount(interval, weights=whole).astype(np.int64)
    by_rank = np.where(whole, count[interval], 0).astype(np.uint64)
    by_pos = np.zeros(n, dtype=np.uint64)
    by_pos[sa] = by_rank
    seen = count[count > 0]
    hist = np.bincount(np.minimum(seen, bins) - 1, minlength=bins).astype(np.uint64)
    stats = dict(whole=int(whole.sum()), distinct=int(seen.size), unique=int((seen == 1).sum()), max_count=int(seen.max()) if seen.size else 0)
    return hist, stats, by_rank, by_pos


@pytest.mark.parametrize("ntiles,per", [(1023, 1), (1024, 1), (1025, 2), (2050, 3)])
def test_one_interval_over_every_block_of_the_sweep(ctx, ntiles, per):
    """A^n $ written down (SA descends, LCP = 0, 0, 1, ..., n - 1) with as many tiles of 256 as the carry sweep has lanes, one
    fewer, one more, and twice as many and a bit: at k = 1 one interval covers every tile but the first rank, so no tile
    but the first holds a head and both carries cross every boundary between two lanes' blocks; at k = 256 that interval
    begins exactly at a tile edge and a single rank ends there"""
    s = (ntiles - 1) * T + 77
    n = s - 1
    assert (s + T - 1) // T == ntiles and (ntiles + 1023) // 1024 == per
    text = np.concatenate([np.full(n, ord("A"), dtype=np.uint8), np.frombuffer(b"$", dtype=np.uint8)])
    sa = np.arange(n, -1, -1, dtype=np.int64)
    lcp = np.concatenate([[0], np.arange(n, dtype=np.int64)])
    heads = lcp[1:] < 1
    assert longest_interval(lcp, 1) == n and not heads[T - 1:].any()         # has == 0 in every tile but the first
    assert boundary_ks(lcp, T)[0] == T and longest_interval(lcp, T) == s - T and lcp[T - 1] < T and lcp[T] < T      # [T - 1, T) and [T, s)
    d_text = torch.from_numpy(text).cuda()
    ctx.set_kmer_tile(T)
    try:
        for wide in (False, True):
            ix = DeviceIndex.wrap(ctx, d_text, _dev(sa.astype(np.uint32), wide), prefix_table=False)
            d_lcp = _dev(lcp.astype(np.uint32), wide)
            for k in (1, T, 3):
                hist, stats, by_rank, by_pos = kmer_witness(sa, lcp, s, k, 256)
                assert stats["max_count"] == n - k + 1
                for occ, want in (("rank", by_rank), ("position", by_pos)):
                    dh, dst, do = ix.kmers_device(d_lcp, k, 256, occ)
                    assert np.array_equal(_host(dh), hist) and dst == stats and np.array_equal(_host(do), want), (wide, k, occ, dst, stats)
            ix.close()
    finally:
        ctx.set_kmer_tile(0)


def test_a_sorted_text_of_more_tiles_than_the_sweep_has_lanes(ctx, tmp_path):
    """525 000 bases sorted on the device, against the host path through a written file: 2051 tiles of 256, three to a lane"""
    x, _ = synth.syn_elegans(525_000, seed=6, n_seqs=1, device="cuda")
    norm = torch.where((x >= 97) & (x <= 122), x - 32, x).contiguous()
    db = sufr_amd.DeviceBuilder(0)
    sa, lcp = db.sort(norm, is_dna=True)
    assert ((sa.numel() + T - 1) // T + 1023) // 1024 == 3
    _write(tmp_path / "x.sufr", norm.cpu().numpy(), sa.cpu().numpy().view(np.uint32).copy(), lcp.cpu().numpy().view(np.uint32).copy())
    f = SufrFile(tmp_path / "x.sufr")
    want = {(k, occ): f.kmers(k, 256, occ, threads=16) for k in (3, 12) for occ in ("rank", "position")}
    db.ctx.set_kmer_tile(T)
    for wide, d_sa, d_lcp in ((False, sa, lcp), (True, sa.to(torch.int64), lcp.to(torch.int64))):      # (both are below 2^31)
        ix = DeviceIndex.wrap(db.ctx, norm, d_sa, is_dna=True, prefix_table=False)
        for (k, occ), (h, st, o) in want.items():
            dh, dst, do = ix.kmers_device(d_lcp, k, 256, occ)
            assert np.array_equal(_host(dh), h) and dst == st and np.array_equal(_host(do), o.astype(np.uint64)), (wide, k, occ)
        ix.close()
    db.ctx.set_kmer_tile(0)
    f.close(); db.close()


def test_outputs_are_left_untouched_outside_their_entries(ctx):
    f = SufrFile(EXP / "long_dna_sequence.sufr")
    assert f.len_suffixes < f.text_len                               # (the Ns are not indexed)
    ix = DeviceIndex.load(ctx, f)
    lcp = _dev(np.asarray(f.lcp))
    L = sufr_amd.lib()
    s, n = f.len_suffixes, f.text_len
    indexed = np.zeros(n, dtype=bool)
    indexed[np.asarray(f.suffix_array)] = True
    for unique in (False, True):
        pos = torch.full((n + 100,), -1, dtype=torch.int32, device="cuda")           # 0xFF in every byte
        rank = torch.full((s + 100,), -1, dtype=torch.int32, device="cuda")
        for out, flags in ((pos, 1), (rank, 0)):
            if unique:
                ctx.check(L.sufr_hip_unique_lengths_device(ctx.handle, ix._h, lcp.data_ptr(), None, 0, flags, out.data_ptr()))
            else:
                ctx.check(L.sufr_hip_kmers_device(ctx.handle, ix._h, lcp.data_ptr(), None, 0, 8, flags, 0, None, out.data_ptr(), None))
        ctx.synchronize()
        pos, rank = _host(pos), _host(rank)
        want_pos = f.unique_lengths(True) if unique else f.kmers(8, 256, "position")[2]
        want_rank = f.unique_lengths() if unique else f.kmers(8, 256, "rank")[2]
        assert np.array_equal(pos[:n], want_pos) and not pos[:n][~indexed].any() and (pos[n:] == 0xFFFFFFFF).all()
        assert np.array_equal(rank[:s], want_rank) and (rank[s:] == 0xFFFFFFFF).all()
    ix.close()


def test_build_then_analyse_without_leaving_the_device(ctx, oracle, tmp_path):
    x, _ = synth.syn_ecoli(100_000, seed=9)
    text = x.numpy()
    f = oracle_file(oracle, tmp_path, text[:-1], is_dna=True, threads=4)
    assert np.array_equal(np.asarray(f.text), text)
    db = sufr_amd.DeviceBuilder(0)
    t = torch.from_numpy(text).cuda()
    sa, lcp = db.sort(t, is_dna=True)                                # sufr_hip_sort_device_u32
    ix = DeviceIndex.wrap(db.ctx, t, sa, is_dna=True)
    same_as_host(f, ix, lcp, (8, 12, 21), (256,))
    ix.close(); db.close()


def test_two_contexts_on_two_threads_share_an_index(ctx):
    f = SufrFile(EXP / "uniprot.sufr")
    ix = DeviceIndex.load(ctx, f)
    lcp = _dev(np.asarray(f.lcp))
    other = sufr_amd.Context(0)
    twin = DeviceIndex(other, ix._h)                                 # the same index through the second context
    twin.text_len, twin.index_width = ix.text_len, ix.index_width
    want = f.kmers(3, 256, "position")
    want_u = f.unique_lengths()
    results, errors = {}, []

    def work(name, index):
        try:
            out = []
            for _ in range(6):
                h, st, o = index.kmers_device(lcp, 3, 256, "position", f.sequence_starts)
                out.append((_host(h), st, _host(o), _host(index.unique_lengths_device(lcp, False, f.sequence_starts))))
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
        for h, st, o, u in results[name]:
            assert np.array_equal(h, want[0]) and st == want[1] and np.array_equal(o, want[2]) and np.array_equal(u, want_u)
    ix.close(); other.close()


def test_cli_kmers_on_the_device_prints_the_host_bytes(tmp_path):
    from test_match_host import run
    for name, k in (("uniprot.sufr", 4), ("long_dna_sequence.sufr", 11)):
        outs = {}
        for where, opts in (("host", []), ("device", ["--device", 0])):
            occ, uniq = tmp_path / f"{where}.occ", tmp_path / f"{where}.uniq"
            outs[where] = (run("kmers", "-k", k, *opts, "--occ", occ, "--unique", uniq, EXP / name).stdout, occ.read_bytes(), uniq.read_bytes())
        assert outs["host"] == outs["device"] and outs["host"][0]


def test_cli_kmers_side_files_and_output_file_on_the_device(tmp_path):
    from test_match_host import run
    for asked in ((), ("occ",), ("unique",)):
        outs = {}
        for where, opts in (("host", []), ("device", ["--device", 0])):
            d = tmp_path / (where + "-" + "-".join(asked))
            d.mkdir()
            files = [x for name in asked for x in (f"--{name}", d / name)]
            outs[where] = (run("kmers", "-k", 4, *opts, *files, EXP / "uniprot.sufr").stdout, {p.name: p.read_bytes() for p in d.iterdir()})
        assert outs["host"] == outs["device"] and outs["host"][0] and sorted(outs["host"][1]) == sorted(asked)
    host, dev = tmp_path / "host.tsv", tmp_path / "dev.tsv"
    assert run("kmers", "-k", 4, "-o", host, EXP / "uniprot.sufr").stdout == run("kmers", "-k", 4, "-o", dev, "--device", 0, EXP / "uniprot.sufr").stdout == ""
    assert host.read_bytes() == dev.read_bytes() != b""


def test_cli_kmers_on_the_device_refuses_a_masked_file():
    from test_match_host import run
    r = run("kmers", "-k", 3, "--device", 0, EXP / "uniprot-masked.sufr", check=False)
    assert r.returncode == 1 and r.stderr.startswith("Error: ") and "uniprot-masked.sufr" in r.stderr
