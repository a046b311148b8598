"""Matching statistics and SMEMs on the GPU (include/sufr_match.h, sufr_match.inc) against the host path of the same
library, which tests/test_match_host.py holds to a brute-force witness."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import sufr_amd
from sufr_amd import DeviceIndex, SufrFile, pack_queries, synth
from oracle_helper import GOLDEN
from test_match_host import random_queries, run

pytestmark = pytest.mark.gpu
EXP = GOLDEN / "expected"


@pytest.fixture(scope="module")
def ctx():
    c = sufr_amd.Context(0)
    yield c
    c.close()


def records(hits):
    return [[(h.query_offset, h.length, h.rank_lo, h.rank_hi, h.positions.tolist()) for h in q] for q in hits]


def same_as_host(f: SufrFile, ix: DeviceIndex, queries, min_lens=(1, 4, 20), max_hits=(0, 3)):
    dms = ix.matching_statistics(queries)
    hms = f.matching_statistics(queries)
    assert all(np.array_equal(a, b) for a, b in zip(dms, hms))
    n = 0
    for k in min_lens:
        for h in max_hits:
            want = records(f.smems(queries, k, h))
            got = records(ix.smems(queries, k, h))
            assert got == want, k
            n += sum(len(q) for q in want)
    return n


@pytest.mark.parametrize("name", sorted(p.name for p in EXP.glob("*.sufr")))
def test_device_equals_host_on_golden_files(ctx, name):
    f = SufrFile(EXP / name)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    queries = random_queries(rng, f, 1500, 150, extra=b"$%XN") + [b"", bytes(f.text)[:3000]]
    ix = DeviceIndex.load(ctx, f)
    if f.seed_mask:
        for call in (lambda: ix.matching_statistics(queries), lambda: ix.smems(queries, 3)):
            with pytest.raises(sufr_amd.SufrHipError) as e:
                call()
            assert e.value.code == -6
        ix.close()
        return
    assert same_as_host(f, ix, queries) > 0
    # without the prefix table: the same answers
    t = torch.from_numpy(np.asarray(f.text).copy()).cuda()
    s = torch.from_numpy(np.asarray(f.suffix_array).astype(np.int32 if f.index_width == 4 else np.int64)).cuda()
    for table in (True, False):
        w = DeviceIndex.wrap(ctx, t, s, max_query_len=f.max_query_len, is_dna=f.is_dna, prefix_table=table)
        assert records(w.smems(queries, 4, 2)) == records(f.smems(queries, 4, 2))
        w.close()
    ix.close()


def test_min_len_zero_and_empty_batches(ctx):
    f = SufrFile(EXP / "1.sufr")
    ix = DeviceIndex.load(ctx, f)
    with pytest.raises(sufr_amd.SufrHipError) as e:
        ix.smems([b"ACGT"], 0)
    assert e.value.code == -1
    assert ix.smems([], 3) == [] and ix.smems([b""], 3) == [[]] and ix.smems([b"", b"QQ"], 1) == [[], []]
    assert [m.tolist() for m in ix.matching_statistics([b"", b"ACGTA", b""])] == [[], [4, 3, 2, 1, 1], []]
    ix.close()


def _write(path, text: np.ndarray, sa: np.ndarray, lcp: np.ndarray, is_dna=True, max_query_len=0):
    err = C.create_string_buffer(256)
    starts = np.zeros(1, dtype=np.uint64)
    names = (C.c_char_p * 1)(b"1")
    w = sa.dtype.itemsize
    rc = sufr_amd.lib().sufr_write_file(str(path).encode(), int(is_dna), 0, 0, text.ctypes.data, text.size, w, sa.ctypes.data,
                                        lcp.ctypes.data, sa.size, int(max_query_len > 0), max_query_len, None, starts.ctypes.data, 1,
                                        names, err, len(err))
    assert rc == 0, err.value


def mutated_reads(rng, text: np.ndarray, nr: int, rl: int = 150, sub: float = 0.01, n_frac: float = 0.002):
    at = rng.integers(0, text.size - rl - 1, nr)
    qb = text[at[:, None] + np.arange(rl)[None, :]].reshape(-1).copy()
    hit = rng.random(qb.size) < sub
    qb[hit] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(hit.sum()))]
    qb[rng.random(qb.size) < n_frac] = ord("N")
    off = np.arange(nr + 1, dtype=np.uint64) * rl
    return qb, off


def compare_packed(f: SufrFile, ix: DeviceIndex, qb, off, min_len):
    want = f.smem_arrays(qb, off, min_len, threads=16)
    dq, dv = torch.from_numpy(qb).cuda(), torch.from_numpy(off.astype(np.int64)).cuda()
    got = ix.smems_device(dq, dv, min_len)
    for a, b in zip(got, want):
        assert np.array_equal(a.cpu().numpy().astype(np.int64), b.astype(np.int64))
    ms = np.zeros(qb.size, dtype=np.uint32)
    assert sufr_amd.lib().sufr_file_matching_stats(f._h, qb.ctypes.data, off.ctypes.data, len(off) - 1, ms.ctypes.data, 16) == 0
    assert np.array_equal(ix.last_ms.cpu().numpy().view(np.uint32)[:qb.size], ms)
    return got, len(want[0])


def test_built_and_wrapped_20mb_with_reads_and_a_long_query(ctx, tmp_path):
    """20 Mb syn_human built by DeviceBuilder and wrapped in place; 20 000 mutated 150-bp reads, queries shorter than the
    prefix table's k, queries with no table entry, a 1 Mb query; 32- and 64-bit arrays; the capacity path."""
    x, _ = synth.syn_human(20_000_000, seed=12, device="cuda")
    norm = torch.where((x >= 97) & (x <= 122), x - 32, x).contiguous()
    db = sufr_amd.DeviceBuilder(0)
    sa, lcp = db.sort(norm, is_dna=True)
    text = norm.cpu().numpy()
    sa_h, lcp_h = sa.cpu().numpy().view(np.uint32).copy(), lcp.cpu().numpy().view(np.uint32).copy()
    _write(tmp_path / "x.sufr", text, sa_h, lcp_h)
    f = SufrFile(tmp_path / "x.sufr")
    ix = DeviceIndex.wrap(db.ctx, norm, sa, is_dna=True)
    rng = np.random.default_rng(6)
    qb, off = mutated_reads(rng, text, 20_000)
    got, n = compare_packed(f, ix, qb, off, 20)
    assert n > 20_000
    # short queries (below pk = 13 here), queries whose first symbols have no table entry, one 1 Mb query
    extra = [bytes(text[i:i + int(L)]) for i, L in zip(rng.integers(0, text.size - 20, 2000), rng.integers(1, 13, 2000))]
    extra += [b"N" * 5 + bytes(text[i:i + 40]) for i in rng.integers(0, text.size - 50, 500)]
    extra += [b"ACGT" * 10 + b"TTTTTTTTTTTTTTTTTGA"]
    long_q = bytearray(text[3_000_000:4_000_000].tobytes())
    for p in rng.integers(0, len(long_q), 2000):
        long_q[int(p)] = ord("ACGT"[int(p) % 4])
    extra.append(bytes(long_q))
    eb, eo = pack_queries(extra)
    compare_packed(f, ix, eb, eo, 1)
    compare_packed(f, ix, eb, eo, 15)
    # the same arrays as a 64-bit index
    sa64 = sa.to(torch.int64) & 0xFFFFFFFF
    ix64 = DeviceIndex.wrap(db.ctx, norm, sa64, is_dna=True)
    assert ix64.index_width == 8
    small_b, small_o = qb[:150 * 2000], off[:2001]
    g32 = ix.smems(list(small_b.reshape(-1, 150)), 20, 5)
    g64 = ix64.smems(list(small_b.reshape(-1, 150)), 20, 5)
    assert records(g32) == records(g64)
    # capacity on the device: refused with the total, nothing else changes
    dq, dv = torch.from_numpy(small_b).cuda(), torch.from_numpy(small_o.astype(np.int64)).cuda()
    total = len(ix.smems_device(dq, dv, 20)[0])
    with pytest.raises(sufr_amd.SufrHipError) as e:
        ix.smems_device(dq, dv, 20, cap=total - 1)
    assert e.value.code == -5 and e.value.total == total
    assert len(ix.smems_device(dq, dv, 20, cap=total)[0]) == total
    ix64.close(); ix.close(); f.close(); db.close()


def test_200k_reads_on_the_100mb_stand_in(tmp_path):
    x, _ = synth.syn_human(100_000_000, seed=4, device="cuda")
    norm = torch.where((x >= 97) & (x <= 122), x - 32, x).contiguous()
    del x
    db = sufr_amd.DeviceBuilder(0)
    sa, lcp = db.sort(norm, is_dna=True)
    text = norm.cpu().numpy()
    _write(tmp_path / "h.sufr", text, sa.cpu().numpy().view(np.uint32), lcp.cpu().numpy().view(np.uint32))
    del lcp
    f = SufrFile(tmp_path / "h.sufr")
    ix = DeviceIndex.wrap(db.ctx, norm, sa, is_dna=True)
    qb, off = mutated_reads(np.random.default_rng(8), text, 200_000)
    _, n = compare_packed(f, ix, qb, off, 20)
    assert n > 200_000
    ix.close(); f.close(); db.close()


def test_cli_match_on_the_device_prints_the_host_bytes(tmp_path):
    f = SufrFile(EXP / "long_dna_sequence.sufr")
    rng = np.random.default_rng(3)
    reads = random_queries(rng, f, 400, 150)
    fa = tmp_path / "r.fa"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(reads) if r))
    for opts in ([], ["-k", 8], ["-k", 8, "-a"], ["-k", 5, "-n", 2]):
        host = run("match", *opts, "-q", fa, EXP / "long_dna_sequence.sufr").stdout
        dev = run("match", "--device", 0, *opts, "-q", fa, EXP / "long_dna_sequence.sufr").stdout
        assert dev == host and host
    assert run("match", "--device", 0, "-k", 3, EXP / "1.sufr", "ACGTA").stdout == "ACGTA\t0\t4\t2\t1:0,1:6\n"
