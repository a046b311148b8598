"""k-difference search on the GPU (include/sufr_edit.h, sufr_edit.inc) against the host path of the same library, which
tests/test_edit_host.py holds to a brute-force witness; a closed form with millions of candidates and planted reads whose
origins must be found go through no host path at all."""
import threading
import zlib

import numpy as np
import pytest
import torch

import sufr_amd
from sufr_amd import DeviceIndex, SufrFile, pack_queries, synth
from oracle_helper import GOLDEN
from test_match_host import run
from test_mem_host import ADVERSARIAL, BUILDS, _adversarial_body, _fasta_from
from test_approx_host import stack
from test_edit_host import COMBOS, with_indels

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


def _host_buffers(ctx, ix: DeviceIndex, qb, off, d, occ, both, mi, cap):
    """sufr_hip_edit: host buffers in, host buffers out."""
    out = [np.zeros(max(cap, 1), dtype=dt) for dt in (np.uint64, np.uint8, np.uint64, np.uint8)]
    total = C.c_uint64(0)
    ctx.check(sufr_amd.lib().sufr_hip_edit(ctx.handle, ix._h, qb.ctypes.data, off.ctypes.data, len(off) - 1, d, occ,
                                           int(both) | 2 * int(mi), cap, *[a.ctypes.data for a in out], C.byref(total)))
    return [a[:total.value] for a in out]


def same_as_host(ctx, f: SufrFile, ix: DeviceIndex, queries, combos=COMBOS):
    qb, off = pack_queries(queries)
    dq, dv = _dev(qb, off)
    n = 0
    for (d, occ, both, mi) in combos:
        want = stack(f.edit_arrays(qb, off, d, occ, both, mi))
        got = stack([t.cpu().numpy() for t in ix.edit_device(dq, dv, d, occ, both, mi)])
        assert np.array_equal(got, want), (d, occ, both, mi, len(got), len(want))
        assert np.array_equal(stack(_host_buffers(ctx, ix, qb, off, d, occ, both, mi, len(want))), want), (d, occ, both, mi)
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
    queries = with_indels(rng, f, 200, 150)
    ix = DeviceIndex.load(ctx, f)
    if f.seed_mask:
        with pytest.raises(sufr_amd.SufrHipError) as e:
            ix.edit(queries, 2)
        assert e.value.code == -6
        ix.close()
        return
    assert same_as_host(ctx, f, ix, queries) > 0
    # wrapped: without the prefix table, and as a 64-bit array
    t, s = _tensors(f)
    _, s64 = _tensors(f, wide=True)
    for sa, table in ((s, False), (s64, True), (s64, False)):
        w = DeviceIndex.wrap(ctx, t, sa, max_query_len=f.max_query_len, is_dna=f.is_dna, prefix_table=table)
        assert same_as_host(ctx, f, w, queries, [(2, 0, True, False), (4, 2, False, True), (0, 0, False, False), (1, 0, True, True)]) > 0
        w.close()
    ix.close()


@pytest.mark.parametrize("kind", ADVERSARIAL)
def test_device_equals_host_on_oracle_builds(ctx, oracle, tmp_path, kind):
    _fasta_from(_adversarial_body(kind), tmp_path / "x.fa")
    for build in BUILDS:
        oracle.create(tmp_path / "x.fa", tmp_path / "x.sufr", **build)
        f = SufrFile(tmp_path / "x.sufr")
        rng = np.random.default_rng(zlib.crc32(f"{kind}{build}".encode()))
        queries = with_indels(rng, f, 60, 60) + [b"A" * 150, b"NACGTACGT", bytes(f.text)[-12:]]
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
    assert same_as_host(ctx, f, ix, with_indels(rng, f, 200, 150)) > 0
    ix.close()


def test_the_largest_distance_and_the_widest_band(ctx):
    """d = 15: 16 pieces, a band of 61 cells, 31 ends per candidate (both words of a candidate's values)."""
    f = SufrFile(EXP / "long_dna_sequence.sufr")
    queries = [q for q in with_indels(np.random.default_rng(15), f, 40, 150) if len(q) >= 60]
    ix = DeviceIndex.load(ctx, f)
    assert same_as_host(ctx, f, ix, queries, [(15, 0, True, False), (15, 0, False, True), (9, 3, True, True)]) > 0
    ix.close()


def test_limits_capacity_and_empty_batches(ctx):
    f = SufrFile(EXP / "3.sufr")
    ix = DeviceIndex.load(ctx, f)
    with pytest.raises(sufr_amd.SufrHipError) as e:
        ix.edit([b"ACGT"], 16)
    assert e.value.code == -1
    assert ix.edit([], 2) == [] and ix.edit([b""], 0) == [[]] and ix.edit([b"", b"QQ"], 2, both_strands=True) == [[], []]
    text = bytes(f.text)
    assert ix.edit([text[:40]], 15) == f.edit([text[:40]], 15) != [[]]
    assert ix.edit([text[:3]], 3) == [[]]
    qb, off = pack_queries([text[0:30] + b"X" + text[31:50] + text[52:70], text[50:90], b"QQ"])
    dq, dv = _dev(qb, off)
    for mi in (False, True):
        total = len(ix.edit_device(dq, dv, 2, 0, True, mi)[0])
        assert total == len(f.edit_arrays(qb, off, 2, 0, True, mi)[0]) >= (1 if mi else 2)     # (one query is 3 edits away: one hill)
        for cap in (0, total - 1):
            with pytest.raises(sufr_amd.SufrHipError) as e:
                ix.edit_device(dq, dv, 2, 0, True, mi, cap=cap)
            assert e.value.code == -5 and e.value.total == total
            # the outputs of a call that does not fit stay as they were
            out = [torch.full((total,), 0x5B, dtype=dt, device="cuda") for dt in (torch.int64, torch.uint8, torch.int64, torch.uint8)]
            n = C.c_uint64(0)
            rc = sufr_amd.lib().sufr_hip_edit_device(ctx.handle, ix._h, dq.data_ptr(), dv.data_ptr(), 3, 2, 0, 1 | 2 * int(mi), cap,
                                                     *[t.data_ptr() for t in out], C.byref(n))
            ctx.synchronize()
            assert rc == -5 and n.value == total and all(bool((t == 0x5B).all()) for t in out)
        assert len(ix.edit_device(dq, dv, 2, 0, True, mi, cap=total)[0]) == total
    ix.close()


def test_closed_form_run_of_a(ctx):
    """Text A^1 000 000 (no sentinel), queries A^100 with c = 0, 1, 3 bytes replaced by C, d = 3.  Against a piece A^l of the
    text the query pays for every C (substituted or deleted) and for every byte of the difference in length, and a piece
    that ends before e is at most e long: D(e) = max(c, m - e), reached by deleting the Cs first.  So the records are the
    ends e >= m - d, each with that value, wherever a piece covers them; about (4 - c) * 10^6 candidates per query, of which
    the pre-filter leaves one per diagonal, 7 ends each: 7 million keys through the sort for n - m + d + 1 records.

    A thinned array: the suffixes in order (the shorter the smaller) with one position in seven left out.  An all-A piece i
    covers e through the starts t in [e - m + o_i - d, e - m + o_i + d], cut to [0, n - len_i]: seven consecutive positions,
    of which one at most is left out.  The cut leaves fewer only at the two edges: at e = m - d, piece 0 keeps t = 0 alone
    (0 is indexed: 0 % 7 != 3) and a later piece keeps o_i - 2d .. o_i; at e = n the last piece keeps four.  Every window
    holds an indexed start, so thinning changes the candidates (6 in 7) and the emissions, not one record."""
    n, m, d = 1_000_000, 100, 3
    pos = np.arange(n - 1, -1, -1, dtype=np.int64)
    sa = pos[pos % 7 != 3]
    t = torch.full((n,), ord("A"), dtype=torch.uint8, device="cuda")
    full = DeviceIndex.wrap(ctx, t, torch.from_numpy(pos.astype(np.int32)).cuda(), is_dna=True)
    thin = DeviceIndex.wrap(ctx, t, torch.from_numpy(sa.astype(np.int32)).cuda(), is_dna=True)
    e = np.arange(m - d, n + 1, dtype=np.int64)
    for swapped in ((), (10,), (10, 30, 60)):
        q = bytearray(b"A" * m)
        for at in swapped:
            q[at] = ord("C")
        want = np.maximum(len(swapped), m - e)
        qb, off = pack_queries([bytes(q)])
        for ix in (full, thin):
            qi, st, end, ed = (x.cpu().numpy().astype(np.int64) for x in ix.edit_device(*_dev(qb, off), d))
            assert np.array_equal(end, e - 1) and np.array_equal(ed, want)
            assert not qi.any() and not st.any()
        # the minima: D falls to c at e = m - c, ties from there on (kept: the first), and nothing follows
        qi, st, end, ed = (x.cpu().numpy().astype(np.int64) for x in thin.edit_device(*_dev(qb, off), d, local_minima=True))
        assert end.tolist() == [m - len(swapped) - 1] and ed.tolist() == [len(swapped)]
    full.close(); thin.close()


def _planted_batch(norm, indexed, nr, rl, rng):
    """nr reads of rl bytes: a slice of the text that starts at `at`, with k = 0..3 edits drawn from substitutions,
    insertions and deletions, the slice sized so that the read comes out rl long; every second read reverse-complemented.
    Returns the reads, the exclusive end of every slice and k."""
    holes = np.concatenate([[0], np.cumsum(~indexed)])
    span = rl + 3
    clean = np.nonzero(holes[span:] - holes[:-span] == 0)[0]       # starts of rl + 3 indexed positions
    clean = clean[norm[clean + span - 1] != ord("$")]
    assert clean.size > nr
    at = rng.choice(clean, nr, replace=False)
    k = rng.integers(0, 4, nr)
    acgt = b"ACGT"
    reads = np.empty((nr, rl), dtype=np.uint8)
    ends = np.empty(nr, dtype=np.int64)
    for i in range(nr):
        kinds = rng.integers(0, 3, int(k[i]))                      # 0: substitution, 1: insertion, 2: deletion
        lt = rl - int((kinds == 1).sum()) + int((kinds == 2).sum())
        q = bytearray(norm[at[i]:at[i] + lt].tobytes())
        for kind in kinds:
            where = int(rng.integers(0, len(q)))
            if kind == 0:
                q[where] = acgt[(acgt.index(q[where]) + 1 + int(rng.integers(0, 3))) % 4] if q[where] in acgt else acgt[0]
            elif kind == 1:
                q.insert(where, acgt[int(rng.integers(0, 4))])
            else:
                del q[where]
        assert len(q) == rl
        reads[i] = np.frombuffer(bytes(q), dtype=np.uint8)
        ends[i] = at[i] + lt
    comp = np.arange(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    reads[1::2] = comp[reads[1::2, ::-1]]
    return reads, ends, k


def test_planted_reads_are_found_at_their_origin():
    """20 000 reads of 150 bp from a 3 Mb syn_human text in which every position is indexed (--dna --ignore-softmask), 0..3
    mixed edits each, every second read reverse-complemented; d = 3, both strands, max_occ 0: at most 3 of the 4 pieces
    carry an edit, so the end of every origin slice is a record, on the right strand, with at most the edits planted.  The
    approx records of the same batch are all there too (the inclusion, on the device)."""
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
    reads, ends, k = _planted_batch(norm, indexed, nr, rl, np.random.default_rng(17))
    strand = np.arange(nr) % 2
    qb, off = reads.reshape(-1).copy(), np.arange(nr + 1, dtype=np.uint64) * rl
    dq, dv = _dev(qb, off)
    qi, st, en, ed = (v.cpu().numpy().astype(np.int64) for v in ix.edit_device(dq, dv, 3, 0, True))
    assert (ed <= 3).all()
    key = (qi * 2 + st) * n + en
    assert (np.diff(key) > 0).all()                               # sorted by (query, strand, end), each once
    want = (np.arange(nr) * 2 + strand) * n + ends - 1
    slot = np.searchsorted(key, want)
    found = (slot < key.size) & (key[np.minimum(slot, key.size - 1)] == want)
    assert found.all(), (int((~found).sum()), np.nonzero(~found)[0][:10])
    assert (ed[slot] <= k).all()
    # The minima.  In the run of consecutive ends that holds an origin's end, the leftmost end of the least value has a larger
    # left neighbour and no smaller right one: it stays, with at most the edits planted.
    mq, ms, me, md = (v.cpu().numpy().astype(np.int64) for v in ix.edit_device(dq, dv, 3, 0, True, True))
    mkey = (mq * 2 + ms) * n + me
    assert (np.diff(mkey) > 0).all() and mkey.size < key.size
    mslot = np.searchsorted(key, mkey)
    assert (key[np.minimum(mslot, key.size - 1)] == mkey).all() and np.array_equal(ed[mslot], md)
    run_of = np.concatenate([[0], np.cumsum(np.diff(key) != 1)])
    least = np.full(run_of[-1] + 1, 99, dtype=np.int64)
    np.minimum.at(least, run_of[mslot], md)
    assert (least[run_of[slot]] <= k).all()
    # every approx record (q, s, p, h) is the edit record (q, s, p + m - 1, <= h)
    aq, as_, ap, ah = (v.cpu().numpy().astype(np.int64) for v in ix.approx_device(dq, dv, 3, 0, True))
    akey = (aq * 2 + as_) * n + ap + rl - 1
    aslot = np.searchsorted(key, akey)
    assert aq.size > nr // 8 and (key[np.minimum(aslot, key.size - 1)] == akey).all() and (ed[np.minimum(aslot, key.size - 1)] <= ah).all()
    ix.close(); db.close()


@pytest.mark.parametrize("name", ["long_dna_sequence.sufr", "uniprot.sufr"])
def test_every_approx_record_is_an_edit_record(ctx, name):
    f = SufrFile(EXP / name)
    qb, off = pack_queries(with_indels(np.random.default_rng(5), f, 300, 150))
    lens = np.diff(off.astype(np.int64))
    dq, dv = _dev(qb, off)
    ix = DeviceIndex.load(ctx, f)
    n = 0
    for d, occ, both in ((1, 0, True), (3, 2, True), (4, 0, False), (2, 5, False)):
        a = stack([t.cpu().numpy() for t in ix.approx_device(dq, dv, d, occ, both)])
        e = stack([t.cpu().numpy() for t in ix.edit_device(dq, dv, d, occ, both)])
        have = {(int(q), int(s), int(x)): int(v) for q, s, x, v in e}
        for q, s, p, h in a:
            key = (int(q), int(s), int(p + lens[q] - 1))
            assert key in have and have[key] <= h, (d, occ, both, q, s, p, h)
        n += len(a)
    assert n > 0
    ix.close()


def test_two_contexts_on_one_index_at_the_same_time():
    """One index (its array leaves the Ns out: the first calls race for the bitmap), two contexts on two threads, several
    calls each: the records of the sequential run."""
    f = SufrFile(EXP / "long_dna_sequence.sufr")
    rng = np.random.default_rng(23)
    batches = [pack_queries(with_indels(rng, f, 150, 150)) for _ in range(2)]
    want = [f.edit_arrays(qb, off, 3, 0, True, bool(k)) for k, (qb, off) in enumerate(batches)]
    ctxs = [sufr_amd.Context(0), sufr_amd.Context(0)]
    ix = DeviceIndex.load(ctxs[0], f)
    errors = []

    def work(k):
        mine = DeviceIndex(ctxs[k], ix._h)                         # the same index through this thread's context
        try:
            dq, dv = _dev(*batches[k])
            for rep in range(5):
                got = [t.cpu().numpy() for t in mine.edit_device(dq, dv, 3, 0, True, bool(k))]
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
    reads = [r for r in with_indels(np.random.default_rng(3), f, 200, 150, extra=b"N") if r and not set(r) & set(b"$%")]
    fa = tmp_path / "r.fa"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    for opts in ([], ["-d", 4, "-l"], ["-d", 3, "-b", "-a"], ["-d", 1, "--max-occ", 3, "-b", "-l"]):
        host = run("edit", *opts, "-q", fa, EXP / "long_dna_sequence.sufr").stdout
        dev = run("edit", "--device", 0, *opts, "-q", fa, EXP / "long_dna_sequence.sufr").stdout
        assert dev == host and host
    assert run("edit", "--device", 0, "-d", 1, "-b", "-l", EXP / "1.sufr", "ACGA").stdout == \
        run("edit", "-d", 1, "-b", "-l", EXP / "1.sufr", "ACGA").stdout != ""
