"""Maximal exact matches (MEMs) on the GPU (include/sufr_mem.h, sufr_mem.inc) against the host path of the same library,
which tests/test_mem_host.py holds to a brute-force witness."""
import zlib

import numpy as np
import pytest
import torch

import sufr_amd
from sufr_amd import DeviceIndex, SufrFile, pack_queries, synth
from oracle_helper import GOLDEN
from test_match_host import random_queries, run
from test_gpu_match import _write, mutated_reads
from test_mem_host import BUILDS, _adversarial_body, _fasta_from, stack

pytestmark = pytest.mark.gpu
EXP = GOLDEN / "expected"
COMBOS = [(k, occ, both) for k in (1, 3, 8) for occ in (0, 2) for both in (False, True)]


@pytest.fixture(scope="module")
def ctx():
    c = sufr_amd.Context(0)
    yield c
    c.close()


def same_as_host(f: SufrFile, ix: DeviceIndex, queries, combos=COMBOS):
    qb, off = pack_queries(queries)
    dq, dv = torch.from_numpy(qb).cuda(), torch.from_numpy(off.astype(np.int64)).cuda()
    n = 0
    for (k, occ, both) in combos:
        want = stack(f.mem_arrays(qb, off, k, occ, both))
        got = stack([t.cpu().numpy() for t in ix.mems_device(dq, dv, k, occ, both)])
        assert np.array_equal(got, want), (k, occ, both)
        n += len(want)
    return n


def _tensors(f: SufrFile, wide=False):
    t = torch.from_numpy(np.asarray(f.text).copy()).cuda()
    s = torch.from_numpy(np.asarray(f.suffix_array).astype(np.int64 if wide or f.index_width == 8 else np.int32)).cuda()
    return t, s


@pytest.mark.parametrize("name", sorted(p.name for p in EXP.glob("*.sufr")))
def test_device_equals_host_on_golden_files(ctx, name):
    f = SufrFile(EXP / name)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    queries = random_queries(rng, f, 800, 150, extra=b"$%XN") + [b"", bytes(f.text)[:3000]]
    ix = DeviceIndex.load(ctx, f)
    if f.seed_mask:
        with pytest.raises(sufr_amd.SufrHipError) as e:
            ix.mems(queries, 3)
        assert e.value.code == -6
        ix.close()
        return
    assert same_as_host(f, ix, queries) > 0
    # wrapped: without the prefix table, and as a 64-bit array
    t, s = _tensors(f)
    _, s64 = _tensors(f, wide=True)
    for sa, table in ((s, False), (s64, True), (s64, False)):
        w = DeviceIndex.wrap(ctx, t, sa, max_query_len=f.max_query_len, is_dna=f.is_dna, prefix_table=table)
        assert same_as_host(f, w, queries, [(3, 0, True), (8, 2, False)]) > 0
        w.close()
    ix.close()


@pytest.mark.parametrize("kind", ["all_a", "acgt_k", "tandem", "n_run", "many_short"])
def test_device_equals_host_on_oracle_builds(ctx, oracle, tmp_path, kind):
    _fasta_from(_adversarial_body(kind), tmp_path / "x.fa")
    for build in BUILDS:
        oracle.create(tmp_path / "x.fa", tmp_path / "x.sufr", **build)
        f = SufrFile(tmp_path / "x.sufr")
        rng = np.random.default_rng(zlib.crc32(f"{kind}{build}".encode()))
        queries = random_queries(rng, f, 200, 60, extra=b"N") + [b"A" * 150, b"NACGTACGT"]
        ix = DeviceIndex.load(ctx, f)
        same_as_host(f, ix, queries)
        ix.close()
        f.close()


def test_min_len_zero_capacity_and_empty_batches(ctx):
    f = SufrFile(EXP / "3.sufr")
    ix = DeviceIndex.load(ctx, f)
    with pytest.raises(sufr_amd.SufrHipError) as e:
        ix.mems([b"ACGT"], 0)
    assert e.value.code == -1
    assert ix.mems([], 3) == [] and ix.mems([b""], 3) == [[]] and ix.mems([b"", b"QQ"], 1, both_strands=True) == [[], []]
    text = bytes(f.text)
    qb, off = pack_queries([text[0:30] + b"X" + text[40:70], text[50:90], b"QQ"])
    dq, dv = torch.from_numpy(qb).cuda(), torch.from_numpy(off.astype(np.int64)).cuda()
    total = len(ix.mems_device(dq, dv, 5, 0, True)[0])
    assert total == len(f.mem_arrays(qb, off, 5, 0, True)[0]) >= 3
    for cap in (0, total - 1):
        with pytest.raises(sufr_amd.SufrHipError) as e:
            ix.mems_device(dq, dv, 5, 0, True, cap=cap)
        assert e.value.code == -5 and e.value.total == total
    assert len(ix.mems_device(dq, dv, 5, 0, True, cap=total)[0]) == total
    ix.close()


def test_reads_on_a_few_mb_dna_text_and_repeated_calls(tmp_path):
    """4 Mb syn_human built by DeviceBuilder and wrapped in place, 20 000 mutated 150-bp reads, half reverse-complemented;
    32- and 64-bit arrays; the same index asked again (the bitmap is built once) gives the same records."""
    x, _ = synth.syn_human(4_000_000, seed=12, device="cuda")
    norm = torch.where((x >= 97) & (x <= 122), x - 32, x).contiguous()
    db = sufr_amd.DeviceBuilder(0)
    sa, lcp = db.sort(norm, is_dna=True)
    text = norm.cpu().numpy()
    sa_h = sa.cpu().numpy().view(np.uint32).copy()
    assert sa_h.size < text.size                                  # (the N runs are not indexed: the bitmap is used)
    _write(tmp_path / "x.sufr", text, sa_h, lcp.cpu().numpy().view(np.uint32).copy())
    f = SufrFile(tmp_path / "x.sufr")
    ix = DeviceIndex.wrap(db.ctx, norm, sa, is_dna=True)
    rng = np.random.default_rng(6)
    qb, off = mutated_reads(rng, text, 20_000)
    rl = 150
    rc = bytes.maketrans(b"ACGT", b"TGCA")
    for i in range(0, 20_000, 2):
        qb[i * rl:(i + 1) * rl] = np.frombuffer(bytes(qb[i * rl:(i + 1) * rl])[::-1].translate(rc), dtype=np.uint8)
    dq, dv = torch.from_numpy(qb).cuda(), torch.from_numpy(off.astype(np.int64)).cuda()
    for (occ, both) in ((0, True), (500, True), (0, False)):
        want = stack(f.mem_arrays(qb, off, 20, occ, both, threads=16))
        for _ in range(3):
            got = stack([t.cpu().numpy() for t in ix.mems_device(dq, dv, 20, occ, both)])
            assert np.array_equal(got, want), (occ, both)
        assert len(want) > 20_000
    sa64 = sa.to(torch.int64) & 0xFFFFFFFF
    ix64 = DeviceIndex.wrap(db.ctx, norm, sa64, is_dna=True)
    small = list(qb[:150 * 2000].reshape(-1, 150))
    assert ix64.mems(small, 20, 0, True) == ix.mems(small, 20, 0, True) == f.mems(small, 20, 0, True)
    ix64.close(); ix.close(); f.close(); db.close()


def test_closed_form_run_of_a(ctx):
    """One run A^R in a text without any other A, query A^150, k = 20: offset 0 reports every p of the run with
    min(150, run_end - p) >= k (the longer run first: rank order), every j > 0 with 150 - j >= k only the run start.
    ~1.3e8 candidates: the candidate -> offset map and the 64-bit candidate count."""
    R, k, s = 1_000_000, 20, 1_234_567
    rng = np.random.default_rng(2)
    body = np.frombuffer(b"CGT", dtype=np.uint8)[rng.integers(0, 3, 3_000_000)]
    body[s:s + R] = ord("A")
    text = np.concatenate([body, np.frombuffer(b"$", dtype=np.uint8)])
    t = torch.from_numpy(text).cuda()
    db = sufr_amd.DeviceBuilder(0)
    sa, _ = db.sort(t, is_dna=True)
    ix = DeviceIndex.wrap(ctx, t, sa, is_dna=True)
    qb, off = pack_queries([b"A" * 150])
    qi, qo, st, ln, pos = (x.cpu().numpy().astype(np.int64) for x in
                           ix.mems_device(torch.from_numpy(qb).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), k))
    p0 = np.arange(s, s + R - k + 1)
    j1 = np.arange(1, 150 - k + 1)
    assert np.array_equal(qo, np.concatenate([np.zeros(p0.size), j1]))
    assert np.array_equal(pos, np.concatenate([p0, np.full(j1.size, s)]))
    assert np.array_equal(ln, np.concatenate([np.minimum(150, s + R - p0), 150 - j1]))
    assert not qi.any() and not st.any()
    ix.close(); db.close()


def test_cli_mems_on_the_device_prints_the_host_bytes(tmp_path):
    f = SufrFile(EXP / "long_dna_sequence.sufr")
    reads = random_queries(np.random.default_rng(3), f, 400, 150)
    fa = tmp_path / "r.fa"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(reads) if r))
    for opts in ([], ["-k", 8], ["-k", 8, "-b", "-a"], ["-k", 5, "--max-occ", 3, "-b"]):
        host = run("mems", *opts, "-q", fa, EXP / "long_dna_sequence.sufr").stdout
        dev = run("mems", "--device", 0, *opts, "-q", fa, EXP / "long_dna_sequence.sufr").stdout
        assert dev == host and host
    assert run("mems", "--device", 0, "-k", 3, "-b", EXP / "1.sufr", "ACGTA").stdout == \
        "ACGTA\t+\t0\t4\t1:6\nACGTA\t+\t0\t4\t1:0\nACGTA\t-\t1\t4\t1:6\nACGTA\t-\t1\t4\t1:0\n"
