"""Repeats of the indexed text on the GPU (include/sufr_repeat.h, sufr_repeat.inc) against the host path of the same library,
which tests/test_repeat_host.py holds to two witnesses.  Every comparison is exact array equality: records, their order,
the total and the stats."""
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
from test_repeat_host import clipped, crowded_candidate, many_left_symbols_body, small_bodies, stack_answers

pytestmark = pytest.mark.gpu
EXP = GOLDEN / "expected"
KINDS = (0, 1, 2)
T = 256                                                               # the smallest tile: one workgroup of ranks
NOTHING = dict(records=0, longest=0, longest_rank=0, max_count=0)
FF = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def ctx():
    c = sufr_amd.Context(0)
    yield c
    c.close()


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def same_as_host(f: SufrFile, ix: DeviceIndex, lcp, kinds, min_lens, filters=((2, 0),), tag="", threads=0):
    """the device's records, order, total and stats equal the host's; returns the number of records seen"""
    seen = 0
    for kind in kinds:
        for ml in min_lens:
            for mc, xc in filters:
                want = f.repeats(kind, ml, mc, xc, threads=threads)
                got = ix.repeats_device(lcp, kind, ml, mc, xc, f.sequence_starts)
                for i in range(3):
                    assert np.array_equal(_u64(got[i]), want[i]), (tag, kind, ml, mc, xc, i)
                assert got[3] == want[3], (tag, kind, ml, mc, xc, got[3], want[3])
                seen += want[3]["records"]
    return seen


def intervals(f: SufrFile):
    """(l, representatives, a, b) of every interval, from the arrays: two stack passes over the clipped LCP"""
    ell = clipped(f)[:-1].astype(np.uint64)
    left, right = stack_answers(ell)
    reps = np.array([r for r in range(1, ell.size) if ell[r] >= 1 and ell[int(left[r])] < ell[r]], dtype=np.int64)
    return ell, reps, left[reps].astype(np.int64), right[reps].astype(np.int64)


@pytest.mark.parametrize("name", sorted(p.name for p in EXP.glob("*.sufr")))
def test_device_equals_host_on_golden_files(ctx, name):
    f = SufrFile(EXP / name)
    for tag, ix, lcp in indexes(ctx, f):
        if f.seed_mask:
            if tag == "loaded":
                for kind in KINDS:
                    with pytest.raises(sufr_amd.SufrHipError) as e:
                        ix.repeats_device(lcp, kind, 3)
                    assert e.value.code == -6
            ix.close()
            continue
        top = max(int(clipped(f).max()), 1)
        for tile in (0, T):
            ctx.set_repeat_tile(tile)
            seen = same_as_host(f, ix, lcp, KINDS, (1, 3, top, top + 1), ((2, 0), (3, 4)), tag=(tag, tile))
            assert seen > 0 or f.len_suffixes < 12
            assert ix.repeats_device(lcp, 0, top + 1, seq_starts=f.sequence_starts)[3] == NOTHING
        ctx.set_repeat_tile(0)
        ix.close()


def test_refusals_return_the_host_codes(ctx, oracle, tmp_path):
    f = oracle_file(oracle, tmp_path, synth.adversarial("tandem", 1200, seed=3)[:-1], is_dna=True, max_query_len=6)
    ix = DeviceIndex.load(ctx, f)
    lcp = _dev(np.asarray(f.lcp))
    for call in (lambda: ix.repeats_device(lcp, 0, 3), lambda: f.repeats(0, 3), lambda: ix.repeats_device(lcp, 0, 0), lambda: f.repeats(0, 0)):
        with pytest.raises(sufr_amd.SufrHipError) as e:
            call()
        assert e.value.code == -6                                    # (the capped build is refused before min_len is looked at)
    ix.close()
    g = SufrFile(EXP / "3.sufr")
    ix = DeviceIndex.load(ctx, g)
    lcp = _dev(np.asarray(g.lcp))
    for call in (lambda: ix.repeats_device(lcp, 0, 0), lambda: g.repeats(0, 0), lambda: ix.repeats_device(lcp, 3, 1), lambda: g.repeats(3, 1)):
        with pytest.raises(sufr_amd.SufrHipError) as e:
            call()
        assert e.value.code == -1
    L = sufr_amd.lib()
    total = C.c_uint64(7)
    for bad in ([1, 5], [0, 5, 5], [0, 9, 5], [0, g.text_len]):
        st = np.array(bad, dtype=np.uint64)
        assert L.sufr_hip_repeats_device(ctx.handle, ix._h, lcp.data_ptr(), st.ctypes.data, st.size, 0, 1, 0, 0, 0, None, None, None,
                                         C.byref(total), None) == -1, bad
        assert total.value == 0
    ctx.synchronize()
    ix.close()


# ---------------------------------------------------------------------------------------------------------------------
# tile boundaries, with the tile at its minimum
# ---------------------------------------------------------------------------------------------------------------------
def test_intervals_across_tiles(ctx, oracle, tmp_path):
    ctx.set_repeat_tile(T)
    try:
        # A^3000: l ascends, so every interval is [r - 1, s): nested, all ending at s, every right search runs to the end of
        # the array over more than 8 tiles, the first rank of every tile finds its a in the tile before, the last tile is
        # partial
        f = oracle_file(oracle, tmp_path, np.full(3000, ord("A"), dtype=np.uint8), "a", is_dna=True)
        ell, reps, a, b = intervals(f)
        s = f.len_suffixes
        assert s % T != 0 and s > 8 * T and reps.size == s - 2
        assert (b == s).all() and (a == reps - 1).all() and (b - a).max() > 8 * T
        firsts = reps[reps % T == 0]
        assert firsts.size >= 8 and (a[reps % T == 0] // T == firsts // T - 1).all()
        ix = DeviceIndex.load(ctx, f)
        lcp = _dev(np.asarray(f.lcp))
        assert same_as_host(f, ix, lcp, KINDS, (1, 5, 2999, 3001), ((2, 0), (100, 2000))) > 0
        assert ix.repeats_device(lcp, 0, 1)[3] == dict(records=s - 2, longest=2999, longest_rank=s - 2, max_count=s - 1)
        # kind 2 on the all-A text: candidates of more than 256 occurrences that are not sequence starts
        assert (b - a).max() > 256 + 1 and ix.repeats_device(lcp, 2, 1)[3] == f.repeats(2, 1)[3]
        ix.close()
        # an a exactly on a tile boundary, a b exactly on one, a representative that is the first rank of a tile, and left
        # searches that leave their tile by more than a tile
        on_a = on_b = first = far = False
        for kind in ("tandem", "acgt_k", "fib"):
            f = oracle_file(oracle, tmp_path, synth.adversarial(kind, 3000, seed=3)[:-1], kind, is_dna=True)
            ell, reps, a, b = intervals(f)
            if kind != "fib":                                        # (these three are asked of tandem and acgt_k)
                on_a, on_b = on_a or bool(((a % T == 0) & (a > 0)).any()), on_b or bool(((b % T == 0) & (b < f.len_suffixes)).any())
                first = first or bool((reps % T == 0).any())
            far = far or bool((reps - a > T).any())
            if kind == "fib":
                # deep nesting: a rank that lies inside many intervals
                depth = np.zeros(f.len_suffixes + 1, dtype=np.int64)
                np.add.at(depth, a, 1)
                np.add.at(depth, b, -1)
                assert np.cumsum(depth).max() >= 12
            ix = DeviceIndex.load(ctx, f)
            assert same_as_host(f, ix, _dev(np.asarray(f.lcp)), KINDS, (1, 2, 8, int(ell.max())), ((2, 0), (3, 0), (2, 2)), tag=kind) > 0
            ix.close()
        assert on_a and on_b and first and far
    finally:
        ctx.set_repeat_tile(0)


def test_three_coarser_levels(tmp_path):
    """1.5 M ranks: three levels above the clipped LCP, and with the tile at 256 more tiles than the largest grid has
    workgroups"""
    n = 1_500_000
    x, _ = synth.syn_elegans(n, seed=5, n_seqs=1, device="cuda")
    norm = torch.where((x >= 97) & (x <= 122), x - 32, x).contiguous()
    db = sufr_amd.DeviceBuilder(0)
    sa, lcp = db.sort(norm, is_dna=True)
    assert sa.numel() > 64 ** 3
    _write(tmp_path / "x.sufr", norm.cpu().numpy(), sa.cpu().numpy().view(np.uint32).copy(), lcp.cpu().numpy().view(np.uint32).copy())
    f = SufrFile(tmp_path / "x.sufr")
    ix = DeviceIndex.wrap(db.ctx, norm, sa, is_dna=True, prefix_table=False)
    for tile in (T, 0):
        db.ctx.set_repeat_tile(tile)
        assert same_as_host(f, ix, lcp, (0, 1), (12,), tag=tile, threads=16) > 1000
    ix.close(); f.close(); db.close()


# ---------------------------------------------------------------------------------------------------------------------
# supermaximal repeats
# ---------------------------------------------------------------------------------------------------------------------
def test_supermaximal(ctx, oracle, tmp_path):
    f = oracle_file(oracle, tmp_path, small_bodies()["several"], "several", is_dna=True)
    assert f.num_sequences == 5
    g = SufrFile(EXP / "uniprot.sufr")
    for h in (f, g):
        for tag, ix, lcp in indexes(ctx, h):
            for tile in (T, 0):
                ctx.set_repeat_tile(tile)
                assert same_as_host(h, ix, lcp, (2,), (1, 4), ((2, 0), (3, 0))) > 0
            ix.close()
    ctx.set_repeat_tile(0)
    # the duplicated sequence: both occurrences are sequence starts
    rank, count, length, _ = f.repeats(2, 80)
    assert 90 in length.tolist()
    # a candidate whose neighbours all differ in the left symbol and that has more than 256 occurrences, none a sequence start
    q = oracle_file(oracle, tmp_path, many_left_symbols_body(), "q", is_dna=False)
    a, b = crowded_candidate(q)
    ix = DeviceIndex.load(ctx, q)
    lcp = _dev(np.asarray(q.lcp))
    for tile in (T, 0):
        ctx.set_repeat_tile(tile)
        assert same_as_host(q, ix, lcp, KINDS, (1, 2)) > 0
        got = ix.repeats_device(lcp, 2, 1)
        assert not ((_u64(got[0]) == a) & (_u64(got[1]) == b - a)).any()
    ctx.set_repeat_tile(0)
    ix.close()


# ---------------------------------------------------------------------------------------------------------------------
# the other cases
# ---------------------------------------------------------------------------------------------------------------------
def test_arrays_of_no_and_one_rank(ctx):
    for tile in (T, 0):
        ctx.set_repeat_tile(tile)
        text = torch.from_numpy(np.frombuffer(b"A$", dtype=np.uint8).copy()).cuda()
        for ranks in (1, 0):
            ix = DeviceIndex.wrap(ctx, text, torch.zeros(ranks, dtype=torch.int32, device="cuda"), prefix_table=False)
            lcp = torch.zeros(ranks, dtype=torch.int32, device="cuda")
            for kind in KINDS:
                rank, count, length, st = ix.repeats_device(lcp, kind, 1)
                assert rank.numel() == count.numel() == length.numel() == 0 and st == NOTHING
            ix.close()
    ctx.set_repeat_tile(0)


def test_capacity_and_untouched_outputs(ctx):
    f = SufrFile(EXP / "long_dna_sequence.sufr")
    ix = DeviceIndex.load(ctx, f)
    lcp = _dev(np.asarray(f.lcp))
    L = sufr_amd.lib()
    want = f.repeats(1, 3)
    n = want[3]["records"]
    assert n > 10
    out = [torch.full((n + 50,), -1, dtype=torch.int64, device="cuda") for _ in range(3)]           # 0xFF in every byte
    total, st = C.c_uint64(0), sufr_amd.RepeatStats()
    args = (ctx.handle, ix._h, lcp.data_ptr(), None, 0, 1, 3, 0, 0)
    assert L.sufr_hip_repeats_device(*args, 0, None, None, None, C.byref(total), C.byref(st)) == -5       # the counting call
    assert total.value == n and st.as_dict() == want[3]
    total.value = 0
    assert L.sufr_hip_repeats_device(*args, n - 1, *(o.data_ptr() for o in out), C.byref(total), None) == -5
    ctx.synchronize()
    assert total.value == n and all((_u64(o) == FF).all() for o in out)                                 # nothing written
    ctx.check(L.sufr_hip_repeats_device(*args, n + 50, *(o.data_ptr() for o in out), C.byref(total), C.byref(st)))
    ctx.synchronize()
    for i in range(3):
        assert np.array_equal(_u64(out[i])[:n], want[i]) and (_u64(out[i])[n:] == FF).all()
    assert total.value == n and st.as_dict() == want[3]
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
    assert same_as_host(f, ix, lcp, KINDS, (8, 14), ((2, 0), (3, 20))) > 0
    ix.close(); db.close()


def test_two_contexts_on_two_threads_share_an_index(ctx):
    f = SufrFile(EXP / "uniprot.sufr")
    ix = DeviceIndex.load(ctx, f)
    lcp = _dev(np.asarray(f.lcp))
    other = sufr_amd.Context(0)
    twin = DeviceIndex(other, ix._h)                                 # the same index through the second context
    twin.text_len, twin.index_width = ix.text_len, ix.index_width
    want = {kind: f.repeats(kind, 3) for kind in (1, 2)}
    results, errors = {}, []

    def work(name, index):
        try:
            out = []
            for _ in range(4):
                for kind in (1, 2):
                    got = index.repeats_device(lcp, kind, 3, seq_starts=f.sequence_starts)
                    out.append((kind, [_u64(got[i]) for i in range(3)], got[3]))
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
        for kind, cols, st in results[name]:
            assert all(np.array_equal(cols[i], want[kind][i]) for i in range(3)) and st == want[kind][3]
    ix.close(); other.close()


def test_cli_repeats_on_the_device_prints_the_host_bytes():
    from test_match_host import run
    for name, opts in (("uniprot.sufr", ["-l", 6, "--kind", "maximal"]), ("long_dna_sequence.sufr", ["-l", 9, "-c", 2, "-C", 5]),
                       ("3.sufr", ["-l", 1, "--kind", "super", "--max-positions", 0])):
        host = run("repeats", *opts, EXP / name).stdout
        assert host.count("\n") > 4 and host == run("repeats", *opts, "--device", 0, EXP / name).stdout


def test_cli_repeats_on_the_device_without_records_to_a_file_and_refused(tmp_path):
    from test_match_host import run
    host = run("repeats", "-l", 100000, EXP / "uniprot.sufr").stdout
    assert host.count("\n") == 4 and host == run("repeats", "-l", 100000, "--device", 0, EXP / "uniprot.sufr").stdout
    a, b = tmp_path / "host.tsv", tmp_path / "dev.tsv"
    assert run("repeats", "-l", 6, "-o", a, EXP / "uniprot.sufr").stdout == run("repeats", "-l", 6, "-o", b, "--device", 0, EXP / "uniprot.sufr").stdout == ""
    assert a.read_bytes() == b.read_bytes() != b""
    r = run("repeats", "-l", 3, "--device", 0, EXP / "uniprot-masked.sufr", check=False)
    assert r.returncode == 1 and r.stderr.startswith("Error: ") and "uniprot-masked.sufr" in r.stderr
