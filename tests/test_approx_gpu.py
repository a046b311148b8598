"""k-mismatch search on the GPU (include/sufr_approx.h, sufr_approx.inc) against the host path of the same library, which
tests/test_approx_host.py holds to a brute-force witness; a closed form with millions of candidates and planted reads whose
origins must be found go through no host path at all."""
import threading
import zlib

import numpy as np
import pytest
import torch

import sufr_amd
from sufr_amd import DeviceIndex, SufrFile, pack_queries, synth
from oracle_helper import GOLDEN
from test_match_host import random_queries, run
from test_mem_host import ADVERSARIAL, BUILDS, _adversarial_body, _fasta_from
from test_approx_host import COMBOS, planted, stack

pytestmark = pytest.mark.gpu
EXP = GOLDEN / "expected"
C = sufr_amd._lib.C


@pytest.fixture(scope="module")
def ctx():
    c = sufr_amd.Context(0)
    yield c
    c.close()


def _dev(qb, off):
    return torch.from_numpy(qb).cuda(), torch.from_numpy(off.astype(np.int64)).cuda()


def _host_buffers(ctx, ix: DeviceIndex, qb, off, d, occ, both, cap):
    """sufr_hip_approx: host buffers in, host buffers out."""
    out = [np.zeros(max(cap, 1), dtype=dt) for dt in (np.uint64, np.uint8, np.uint64, np.uint8)]
    total = C.c_uint64(0)
    ctx.check(sufr_amd.lib().sufr_hip_approx(ctx.handle, ix._h, qb.ctypes.data, off.ctypes.data, len(off) - 1, d, occ, int(both), cap,
                                             *[a.ctypes.data for a in out], C.byref(total)))
    return [a[:total.value] for a in out]


def same_as_host(ctx, f: SufrFile, ix: DeviceIndex, queries, combos=COMBOS):
    qb, off = pack_queries(queries)
    dq, dv = _dev(qb, off)
    n = 0
    for (d, occ, both) in combos:
        want = stack(f.approx_arrays(qb, off, d, occ, both))
        got = stack([t.cpu().numpy() for t in ix.approx_device(dq, dv, d, occ, both)])
        assert np.array_equal(got, want), (d, occ, both)
        assert np.array_equal(stack(_host_buffers(ctx, ix, qb, off, d, occ, both, len(want))), want), (d, occ, both)
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
    queries = random_queries(rng, f, 400, 150, extra=b"$%XN") + planted(rng, f, 200, 150)
    ix = DeviceIndex.load(ctx, f)
    if f.seed_mask:
        with pytest.raises(sufr_amd.SufrHipError) as e:
            ix.approx(queries, 2)
        assert e.value.code == -6
        ix.close()
        return
    assert same_as_host(ctx, f, ix, queries) > 0
    # wrapped: without the prefix table, and as a 64-bit array
    t, s = _tensors(f)
    _, s64 = _tensors(f, wide=True)
    for sa, table in ((s, False), (s64, True), (s64, False)):
        w = DeviceIndex.wrap(ctx, t, sa, max_query_len=f.max_query_len, is_dna=f.is_dna, prefix_table=table)
        assert same_as_host(ctx, f, w, queries, [(2, 0, True), (4, 2, False), (0, 0, False)]) > 0
        w.close()
    ix.close()


@pytest.mark.parametrize("kind", ADVERSARIAL)
def test_device_equals_host_on_oracle_builds(ctx, oracle, tmp_path, kind):
    _fasta_from(_adversarial_body(kind), tmp_path / "x.fa")
    for build in BUILDS:
        oracle.create(tmp_path / "x.fa", tmp_path / "x.sufr", **build)
        f = SufrFile(tmp_path / "x.sufr")
        rng = np.random.default_rng(zlib.crc32(f"{kind}{build}".encode()))
        queries = planted(rng, f, 100, 60) + [b"A" * 150, b"NACGTACGT"]
        ix = DeviceIndex.load(ctx, f)
        assert same_as_host(ctx, f, ix, queries) > 0
        ix.close()
        f.close()


def test_device_equals_host_on_a_protein_build(ctx, oracle, tmp_path):
    rng = np.random.default_rng(8)
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    body = aa[rng.integers(0, 20, 5000)].copy()
    body[3000:3200] = body[500:700]
    body[[1400, 3900]] = ord("%")
    _fasta_from(body, tmp_path / "p.fa")
    oracle.create(tmp_path / "p.fa", tmp_path / "p.sufr", is_dna=False)
    f = SufrFile(tmp_path / "p.sufr")
    ix = DeviceIndex.load(ctx, f)
    assert same_as_host(ctx, f, ix, planted(rng, f, 200, 150)) > 0
    ix.close()


def test_limits_capacity_and_empty_batches(ctx):
    f = SufrFile(EXP / "3.sufr")
    ix = DeviceIndex.load(ctx, f)
    with pytest.raises(sufr_amd.SufrHipError) as e:
        ix.approx([b"ACGT"], 16)
    assert e.value.code == -1
    assert ix.approx([], 2) == [] and ix.approx([b""], 0) == [[]] and ix.approx([b"", b"QQ"], 2, both_strands=True) == [[], []]
    text = bytes(f.text)
    assert ix.approx([text[:40]], 15) == f.approx([text[:40]], 15) != [[]]
    qb, off = pack_queries([text[0:30] + b"X" + text[31:70], text[50:90], b"QQ"])
    dq, dv = _dev(qb, off)
    total = len(ix.approx_device(dq, dv, 2, 0, True)[0])
    assert total == len(f.approx_arrays(qb, off, 2, 0, True)[0]) >= 2
    for cap in (0, total - 1):
        with pytest.raises(sufr_amd.SufrHipError) as e:
            ix.approx_device(dq, dv, 2, 0, True, cap=cap)
        assert e.value.code == -5 and e.value.total == total
        # the outputs of a call that does not fit stay as they were
        out = [torch.full((total,), 0x5B, dtype=dt, device="cuda") for dt in (torch.int64, torch.uint8, torch.int64, torch.uint8)]
        n = C.c_uint64(0)
        rc = sufr_amd.lib().sufr_hip_approx_device(ctx.handle, ix._h, dq.data_ptr(), dv.data_ptr(), 3, 2, 0, 1, cap,
                                                   *[t.data_ptr() for t in out], C.byref(n))
        ctx.synchronize()
        assert rc == -5 and n.value == total and all(bool((t == 0x5B).all()) for t in out)
    assert len(ix.approx_device(dq, dv, 2, 0, True, cap=total)[0]) == total
    ix.close()


def test_closed_form_run_of_a(ctx):
    """Text A^1 000 000 (no sentinel), its suffixes in order (the shorter the smaller) with one position in seven left out
    of the array, queries A^100 with c = 0, 1, 3 bytes replaced by C, d = 3: every window is at distance c, so the records are
    the windows that have an all-A piece starting on an indexed position, once each, by the lowest such piece, in rank order
    (descending position).  About (4 - c) * 10^6 candidates per query: the lowest-anchor rule and the bitmap at scale."""
    n, m, d = 1_000_000, 100, 3
    pos = np.arange(n - 1, -1, -1, dtype=np.int64)
    sa = pos[pos % 7 != 3]
    t = torch.full((n,), ord("A"), dtype=torch.uint8, device="cuda")
    ix = DeviceIndex.wrap(ctx, t, torch.from_numpy(sa.astype(np.int32)).cuda(), is_dna=True)
    indexed = np.zeros(n, dtype=bool)
    indexed[sa] = True
    w = n - m + 1
    o = [i * m // (d + 1) for i in range(d + 2)]
    for swapped in ((), (10,), (10, 30, 60)):
        q = bytearray(b"A" * m)
        for at in swapped:
            q[at] = ord("C")
        good = [i for i in range(d + 1) if not any(o[i] <= at < o[i + 1] for at in swapped)]
        assert good
        lowest = np.full(w, -1, dtype=np.int64)
        for i in reversed(good):
            lowest[indexed[o[i]:o[i] + w]] = i
        want = []
        for i in good:
            p = sa - o[i]
            ok = (p >= 0) & (p < w)
            ok[ok] = lowest[p[ok]] == i
            want.append(p[ok])
        want = np.concatenate(want)
        assert want.size == int((lowest >= 0).sum()) >= 6 * w // 7        # (one good piece: the windows whose anchor is not left out)
        qb, off = pack_queries([bytes(q)])
        qi, st, ps, mm = (x.cpu().numpy().astype(np.int64) for x in ix.approx_device(*_dev(qb, off), d))
        assert np.array_equal(ps, want)
        assert (mm == len(swapped)).all() and not qi.any() and not st.any()
    ix.close()


def test_planted_reads_are_found_at_their_origin():
    """20 000 reads of 150 bp from windows of a 3 Mb syn_human text in which every position is indexed (--dna
    --ignore-softmask), exactly e = 0..3 substitutions each, every second read reverse-complemented; d = 3, both strands,
    max_occ 0: at most 3 of the 4 pieces carry a substitution, so every origin is a record, on the right strand."""
    x, _ = synth.syn_human(3_000_000, seed=21)
    norm = sufr_amd.normalize(x.numpy(), ignore_softmask=True)
    t = torch.from_numpy(norm).cuda()
    db = sufr_amd.DeviceBuilder(0)
    sa, _ = db.sort(t, is_dna=True)
    ix = DeviceIndex.wrap(db.ctx, t, sa, is_dna=True)
    n, rl, nr = norm.size, 150, 20_000
    indexed = np.zeros(n, dtype=bool)
    indexed[sa.cpu().numpy().view(np.uint32)] = True
    assert not indexed[norm == ord("N")].any()
    holes = np.concatenate([[0], np.cumsum(~indexed)])
    clean = np.nonzero(holes[rl:] - holes[:-rl] == 0)[0]          # window starts with 150 indexed positions
    clean = clean[norm[clean + rl - 1] != ord("$")]
    assert clean.size > nr
    rng = np.random.default_rng(17)
    at = rng.choice(clean, nr, replace=False)
    reads = norm[at[:, None] + np.arange(rl)[None, :]].copy()
    e = rng.integers(0, 4, nr)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for i in range(nr):
        where = rng.choice(rl, int(e[i]), replace=False)
        for j in where:
            reads[i, j] = rng.choice(acgt[acgt != reads[i, j]])
    comp = np.arange(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    reads[1::2] = comp[reads[1::2, ::-1]]
    strand = np.arange(nr) % 2
    qb, off = reads.reshape(-1).copy(), np.arange(nr + 1, dtype=np.uint64) * rl
    qi, st, ps, mm = (v.cpu().numpy().astype(np.int64) for v in ix.approx_device(*_dev(qb, off), 3, 0, True))
    assert (mm <= 3).all()
    key = (qi * 2 + st) * n + ps
    order = np.argsort(key)
    want = (np.arange(nr) * 2 + strand) * n + at
    slot = np.searchsorted(key[order], want)
    found = (slot < key.size) & (key[order][np.minimum(slot, key.size - 1)] == want)
    assert found.all(), (int((~found).sum()), np.nonzero(~found)[0][:10])
    assert (mm[order][slot] <= e).all()
    ix.close(); db.close()


def test_two_contexts_on_one_index_at_the_same_time():
    """One index (its array leaves the Ns out: the first calls race for the bitmap), two contexts on two threads, several
    calls each: the records of the sequential run."""
    f = SufrFile(EXP / "long_dna_sequence.sufr")
    rng = np.random.default_rng(23)
    batches = [pack_queries(planted(rng, f, 300, 150)) for _ in range(2)]
    want = [f.approx_arrays(qb, off, 3, 0, True) for qb, off in batches]
    ctxs = [sufr_amd.Context(0), sufr_amd.Context(0)]
    ix = DeviceIndex.load(ctxs[0], f)
    errors = []

    def work(k):
        mine = DeviceIndex(ctxs[k], ix._h)                         # the same index through this thread's context
        try:
            dq, dv = _dev(*batches[k])
            for rep in range(5):
                got = [t.cpu().numpy() for t in mine.approx_device(dq, dv, 3, 0, True)]
                if not all(np.array_equal(a.astype(np.int64), b.astype(np.int64)) for a, b in zip(got, want[k])):
                    errors.append(f"context {k}, call {rep}: records differ from the sequential run's")
                    break
        except Exception as e:                                     # noqa: BLE001 (reported below, in the main thread)
            errors.append(f"context {k}: {e!r}")
        finally:
            mine._h = None                                         # (ix owns the handle)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads: t.start()
    for t in threads: t.join(timeout=600)
    assert not any(t.is_alive() for t in threads), "a call did not return"
    assert not errors, errors
    assert len(want[0][0]) > 0 and len(want[1][0]) > 0
    ix.close()
    for c in ctxs: c.close()


def test_cli_on_the_device_prints_the_host_bytes(tmp_path):
    f = SufrFile(EXP / "long_dna_sequence.sufr")
    reads = [r for r in planted(np.random.default_rng(3), f, 300, 150, extra=b"N") if r and not set(r) & set(b"$%")]
    fa = tmp_path / "r.fa"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    for opts in ([], ["-d", 4], ["-d", 3, "-b", "-a"], ["-d", 1, "--max-occ", 3, "-b"]):
        host = run("approx", *opts, "-q", fa, EXP / "long_dna_sequence.sufr").stdout
        dev = run("approx", "--device", 0, *opts, "-q", fa, EXP / "long_dna_sequence.sufr").stdout
        assert dev == host and host
    assert run("approx", "--device", 0, "-d", 1, "-b", EXP / "1.sufr", "ACGA").stdout == \
        "ACGA\t+\t1:6\t1\nACGA\t+\t1:0\t1\nACGA\t-\t1:6\t1\nACGA\t-\t1:0\t1\n"
