"""k-mismatch search on the FM-index by backtracking, on the GPU (include/sufr_fm_approx.h, sufr_fm.inc),
against the host path of the same library and the recursive witness of tests/test_fm_approx_host.py.  Every comparison is exact
equality of the four record arrays, order included: on the loaded, the wrapped and the 64-bit index (the one-line shape and
the wide one), built at the default BWT tile and at its minimum, with every suffix kept and every 32nd."""
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
from test_bwt_gpu import _unsigned, wrapped
from test_fm_host import Witness, sorted_sa
from test_fm_approx_host import (CAPACITY, CASES, DTYPES, INVALID, UNSUPPORTED, brute_set, case, check_conditions, planted, query_set, record_set,
                                 same_arrays, want_records)

pytestmark = pytest.mark.gpu
EXP = GOLDEN / "expected"
T = 256                                                               # the smallest tile
LONG = "long_dna_sequence_allow_ambiguity.sufr"


@pytest.fixture(scope="module")
def ctx():
    c = sufr_amd.Context(0)
    yield c
    c.set_bwt_tile(0)
    c.close()


def on_device(qs):
    qb, off = pack_queries(qs)
    return torch.from_numpy(qb).cuda(), torch.from_numpy(off.astype(np.int64)).cuda()


def records(dfm, batch, d, both, **kw):
    """the four arrays of a device call, with the types of the host's"""
    got = dfm.approx_device(*batch, d, both, **kw)
    assert [t.dtype for t in got] == [torch.int64, torch.uint8, torch.int64, torch.uint8]
    return tuple(_unsigned(t).astype(dt) for t, dt in zip(got, DTYPES))


def check_index(ctx, ix, qs, wants, ds, samples=(1, 32), tiles=(0, T), tag=""):
    """wants[(d, both)]: the arrays the device must give, for every d of ds, on the FM-index of ix at every tile and sample"""
    batch = on_device(qs)
    for tile in tiles:
        ctx.set_bwt_tile(tile)
        for sample in samples:
            dfm = ix.fm_device(sample)
            for d in ds:
                for both in (False, True):
                    assert same_arrays(records(dfm, batch, d, both), wants[(d, both)]), (tag, tile, sample, d, both)
            dfm.close()
    ctx.set_bwt_tile(0)


# ---------------------------------------------------------------------------------------------------------------------
# the golden files: device == host == witness
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,d", CASES)
def test_device_equals_host_and_witness_on_golden_files(ctx, name, d):
    f, w, qs, want = case(name, d)
    fm = f.fm(7)
    qb, off = pack_queries(qs)
    for both in (False, True):
        assert same_arrays(fm.approx_arrays(qb, off, d, both), want[both])                # host == witness; below device == both
    wants = {(d, both): want[both] for both in (False, True)}
    for tag, ix, _ in indexes(ctx, f):
        check_index(ctx, ix, qs, wants, (d,), tag=(name, tag))
        ix.close()


def test_batches_of_600_and_of_one(ctx):
    """three workgroups, the last partial; and one lane of one workgroup"""
    f, w, _, _ = case(LONG, 1)
    rng = np.random.default_rng(9)
    raw = w.text.tobytes()
    qs = [planted(rng, w, raw, int(a), 24, [int(t)] if k % 3 else []) for k, (a, t) in enumerate(zip(rng.integers(0, w.n - 24, 600), rng.integers(0, 24, 600)))]
    fm = f.fm(32)
    ix = DeviceIndex.load(ctx, f)
    dfm = ix.fm_device(32)
    ix.close()
    for d, both in ((1, True), (2, False)):
        want = fm.approx_arrays(*pack_queries(qs), d, both)
        assert len(set(want[0].tolist())) == 600 and record_set(want) == brute_set(w, qs, d, both)
        assert same_arrays(records(dfm, on_device(qs), d, both), want), (d, both)
    for q in (qs[0], b"", raw[-5:]):
        assert same_arrays(records(dfm, on_device([q]), 2, True), fm.approx_arrays(*pack_queries([q]), 2, True)), q
    hits = dfm.approx(qs[:3], 1)
    assert [[(h.position, h.mismatches) for h in hs] for hs in hits] == [[(h.position, h.mismatches) for h in hs] for hs in fm.approx(qs[:3], 1)]


# ---------------------------------------------------------------------------------------------------------------------
# oracle-built texts with every position indexed
# ---------------------------------------------------------------------------------------------------------------------
def test_a_run_and_a_fibonacci_string(ctx, oracle, tmp_path):
    """A^1000: every leaf of A^20 at d = 2 is a wide range; a Fibonacci string: few distinct substrings, ranges stay wide"""
    run = oracle_file(oracle, tmp_path, np.full(1000, ord("A"), dtype=np.uint8), "a", is_dna=True, allow_ambiguity=True)
    fib = oracle_file(oracle, tmp_path, fibonacci(3000), "fib", is_dna=True, allow_ambiguity=True)
    for name, f, qs in (("run", run, [b"A" * 20, b"A" * 19 + b"C", b"C" + b"A" * 19, b"A" * 600]), ("fib", fib, None)):
        w = Witness(np.asarray(f.text), np.asarray(f.suffix_array))
        assert f.len_suffixes == f.text_len
        qs = qs or query_set(w, 2, seed=4)
        wants = {(2, both): want_records(w, qs, 2, both) for both in (False, True)}
        assert record_set(wants[(2, True)]) == brute_set(w, qs, 2, True)
        if name == "run":
            assert len(wants[(2, False)][0]) > 3 * 900 and (wants[(2, False)][3] <= 2).all()
        fm = f.fm(32)
        assert same_arrays(fm.approx_arrays(*pack_queries(qs), 2, True), wants[(2, True)])
        for tag, ix, _ in indexes(ctx, f):
            check_index(ctx, ix, qs, wants, (2,), samples=(32, 7), tiles=(T,), tag=(name, tag))
            ix.close()


def test_all_byte_values(ctx):
    rng = np.random.default_rng(11)
    text = rng.integers(0, 255, 5000).astype(np.uint8)
    text[:255] = np.arange(255)
    text[-1] = 255                                                   # the end byte occurs once
    sa = sorted_sa(text)
    w = Witness(text, sa)
    qs = query_set(w, 1, seed=3) + [text[100:101].tobytes(), text[300:302].tobytes()]
    check_conditions("bytes", w, qs, 1, 1024)
    wants = {(1, both): want_records(w, qs, 1, both) for both in (False, True)}
    for name, ix in wrapped(ctx, text, sa):
        info = ix.fm_device(32).info
        assert (info["symbols"], info["stride"]) == ((256, 2048) if name == "wrapped" else (256, 4096)), info
        check_index(ctx, ix, qs, wants, (1,), samples=(32,), tiles=(T,), tag=name)
        ix.close()


# ---------------------------------------------------------------------------------------------------------------------
# lifetime, determinism, call shapes
# ---------------------------------------------------------------------------------------------------------------------
def test_the_index_outlives_its_arrays_and_two_calls_give_equal_bytes(ctx):
    f, w, qs, want = case(LONG, 2)
    batch = on_device(qs)
    d_text = torch.from_numpy(np.array(f.text)).cuda()
    d_sa = torch.from_numpy(np.array(f.suffix_array).view(np.int32)).cuda()
    ix = DeviceIndex.wrap(ctx, d_text, d_sa, is_dna=True, prefix_table=False)
    a = ix.fm_device(32)
    d_text.zero_()
    d_sa.zero_()
    torch.cuda.synchronize()
    assert same_arrays(records(a, batch, 2, True), want[True])
    ix.close()
    del d_text, d_sa
    first, second = a.approx_device(*batch, 2, True), a.approx_device(*batch, 2, True)
    assert all(torch.equal(x, y) for x, y in zip(first, second)) and same_arrays(records(a, batch, 2, True), want[True])
    loaded = DeviceIndex.load(ctx, f)
    b = loaded.fm_device(7)
    loaded.close()
    assert same_arrays(records(b, batch, 2, False), want[False])


def test_refusals_capacity_and_the_empty_batch(ctx):
    f, w, qs, want = case(LONG, 2)
    batch = on_device(qs)
    ix = DeviceIndex.load(ctx, f)
    dfm, none = ix.fm_device(7), ix.fm_device(0)
    ix.close()
    L = sufr_amd.lib()
    z, nq = len(want[False][0]), len(qs)
    assert z > 50
    out = [torch.full((z + 3,), 0x55, dtype=t, device="cuda") for t in (torch.int64, torch.uint8, torch.int64, torch.uint8)]
    total = C.c_uint64(0)
    call = lambda h, d, cap: L.sufr_hip_fm_approx_device(ctx.handle, h, batch[0].data_ptr(), batch[1].data_ptr(), nq, d, 0, cap,
                                                         *[t.data_ptr() for t in out], C.byref(total))
    assert call(dfm._h, 4, z) == INVALID and total.value == 0
    assert call(none._h, 2, z) == UNSUPPORTED and total.value == 0
    assert call(dfm._h, 2, z - 1) == CAPACITY
    ctx.synchronize()
    assert total.value == z and all((t == 0x55).all().item() for t in out)          # nothing written
    ctx.check(call(dfm._h, 2, z))
    ctx.synchronize()
    assert total.value == z and same_arrays([_unsigned(t[:z]).astype(dt) for t, dt in zip(out, DTYPES)], want[False])
    assert all((t[z:] == 0x55).all().item() for t in out)
    with pytest.raises(SufrHipError) as err:
        dfm.approx_device(*batch, 2, cap=z - 1)
    assert err.value.code == CAPACITY and err.value.total == z
    # no queries: nothing is read
    ctx.check(L.sufr_hip_fm_approx_device(ctx.handle, dfm._h, None, None, 0, 2, 1, 0, None, None, None, None, C.byref(total)))
    assert total.value == 0
    empty = (torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))
    assert all(t.numel() == 0 for t in dfm.approx_device(*empty, 2, True))
    assert all(t.numel() == 0 for t in dfm.approx_device(*on_device([b"", b""]), 3, True))
    assert dfm.approx([], 1) == [] and dfm.approx([b""], 1) == [[]]
    # the host-buffer entry point
    qb, off = pack_queries(qs)
    host = [np.zeros(z, dtype=dt) for dt in DTYPES]
    ctx.check(L.sufr_hip_fm_approx(ctx.handle, dfm._h, qb.ctypes.data, off.ctypes.data, nq, 2, 0, z, *[a.ctypes.data for a in host], C.byref(total)))
    assert total.value == z and same_arrays(host, want[False])


def test_two_contexts_on_two_threads(ctx):
    """two contexts, each with the FM-index of a different file, build and answer at once on two host threads"""
    cases = [case("uniprot.sufr", 1), case(LONG, 2)]
    ds = (1, 2)
    other = sufr_amd.Context(0)
    errors = []

    def work(c, f, qs, want, d):
        try:
            batch = on_device(qs)
            for _ in range(3):
                ix = DeviceIndex.load(c, f)
                dfm = ix.fm_device(7)
                ix.close()
                for both in (False, True):
                    assert same_arrays(records(dfm, batch, d, both), want[both])
                dfm.close()
        except BaseException as e:                                   # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=work, args=(c, f, qs, want, d)) for c, (f, w, qs, want), d in zip((ctx, other), cases, ds)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    other.close()
    assert not errors, errors


def test_cli_on_the_device_prints_the_host_lines():
    from test_match_host import run
    path = EXP / LONG
    reads = ["ACGTACGTAC", "GATTACAGATTACA", "NNNNNNNN", "ACGGT"]
    for extra in ((), ("-b", "-a")):
        assert run("fm", "-d", 2, "--device", 0, *extra, path, *reads).stdout == run("fm", "-d", 2, *extra, path, *reads).stdout != ""
