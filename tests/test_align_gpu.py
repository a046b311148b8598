"""Alignment traceback of k-difference records on the GPU (include/sufr_align.h, sufr_trace.inc) against the host path of
the same library, which tests/test_align_host.py holds to a full-table witness: starts, offsets and runs byte for byte,
through device tensors (sufr_hip_edit_trace_device) and through host buffers (sufr_hip_edit_trace)."""
import threading
import zlib

import numpy as np
import pytest
import torch

import sufr_amd
from sufr_amd import DeviceIndex, SufrFile, SufrHipError, pack_queries
from oracle_helper import GOLDEN
from test_match_host import run
from test_mem_host import _fasta_from
from test_edit_host import with_indels

pytestmark = pytest.mark.gpu
EXP = GOLDEN / "expected"
C = sufr_amd._lib.C
COMBOS4 = [(2, 0, True, False), (4, 2, False, True), (0, 0, False, False), (1, 0, True, True)]      # d, max_occ, both, minima
GOLDEN_FILES = sorted(p.name for p in EXP.glob("*.sufr") if not SufrFile(p).seed_mask)
DTYPES = (np.uint64, np.uint8, np.uint64, np.uint8)


@pytest.fixture(scope="module")
def ctx():
    c = sufr_amd.Context(0)
    yield c
    c.close()


def _dev(qb, off):
    return torch.from_numpy(qb).cuda(), torch.from_numpy(off.astype(np.int64)).cuda()


def _np(recs):
    return [t.cpu().numpy().astype(d) for t, d in zip(recs, DTYPES)]


def _to_dev(recs):
    return [torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else np.uint8)).cuda() for a in recs]


def trace_device(ix, dq, dv, drecs, cap=None):
    st, co, cg = ix.edit_trace_device(dq, dv, *drecs, cap=cap)
    return st.cpu().numpy().view(np.uint64), co.cpu().numpy().view(np.uint64), cg.cpu().numpy().view(np.uint32)


def same(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got, want))


def same_as_host(f: SufrFile, ix: DeviceIndex, queries, combos):
    """Records from edit_device, traced through both device entry points, against the host trace; the number of records."""
    qb, off = pack_queries(queries)
    dq, dv = _dev(qb, off)
    n = 0
    for (d, occ, both, mi) in combos:
        drecs = [t.contiguous() for t in ix.edit_device(dq, dv, d, occ, both, mi)]
        recs = _np(drecs)
        want = f.edit_trace_arrays(qb, off, *recs)
        assert same(trace_device(ix, dq, dv, drecs), want), (d, occ, both, mi)
        assert same(ix.edit_trace(qb, off, *recs), want), (d, occ, both, mi)
        n += len(recs[0])
    return n


def _tensors(f: SufrFile, wide=False):
    t = torch.from_numpy(np.asarray(f.text).copy()).cuda()
    s = torch.from_numpy(np.asarray(f.suffix_array).astype(np.int64 if wide or f.index_width == 8 else np.int32)).cuda()
    return t, s


@pytest.mark.parametrize("name", GOLDEN_FILES)
def test_device_equals_host_on_golden_files(ctx, name):
    """200 queries of up to 150 bytes, four (d, max_occ, strands, minima) combinations, then a 64-bit array."""
    f = SufrFile(EXP / name)
    queries = with_indels(np.random.default_rng(zlib.crc32(name.encode())), f, 200, 150)
    ix = DeviceIndex.load(ctx, f)
    assert same_as_host(f, ix, queries, COMBOS4) > 0
    t, s64 = _tensors(f, wide=True)
    w = DeviceIndex.wrap(ctx, t, s64, max_query_len=f.max_query_len, is_dna=f.is_dna)
    assert same_as_host(f, w, queries, COMBOS4) > 0
    w.close()
    ix.close()


def test_a_seed_mask_index_is_traced(ctx):
    p, k = SufrFile(EXP / "uniprot.sufr"), SufrFile(EXP / "uniprot-masked.sufr")
    qb, off = pack_queries(with_indels(np.random.default_rng(2), p, 50, 60))
    recs = p.edit_arrays(qb, off, 2)
    ix = DeviceIndex.load(ctx, k)
    assert len(recs[0]) > 0 and same(ix.edit_trace(qb, off, *recs), p.edit_trace_arrays(qb, off, *recs))
    ix.close()


def test_the_widest_band_d15_31_cells(ctx):
    f = SufrFile(EXP / "long_dna_sequence.sufr")
    queries = [q for q in with_indels(np.random.default_rng(15), f, 40, 150) if len(q) >= 60]
    ix = DeviceIndex.load(ctx, f)
    qb, off = pack_queries(queries)
    recs = f.edit_arrays(qb, off, 15, 0, True, False)
    assert int(recs[3].max()) == 15                               # records that use the whole band
    assert same_as_host(f, ix, queries, [(15, 0, True, False), (15, 0, False, True)]) > 0
    ix.close()


def test_a_protein_build(ctx, oracle, tmp_path):
    rng = np.random.default_rng(8)
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    body = aa[rng.integers(0, 20, 5000)].copy()
    body[3000:3200] = body[500:700]
    body[[1400, 3900]] = ord("%")
    _fasta_from(body, tmp_path / "p.fa")
    oracle.create(tmp_path / "p.fa", tmp_path / "p.sufr", is_dna=False)
    f = SufrFile(tmp_path / "p.sufr")
    ix = DeviceIndex.load(ctx, f)
    assert same_as_host(f, ix, with_indels(rng, f, 200, 150), COMBOS4) > 0
    ix.close()


# ---------------------------------------------------------------------------------------------------------------------
# a text without a sentinel: query lengths, the two ends of the text
# ---------------------------------------------------------------------------------------------------------------------
class Plain:
    """6 000 random bytes of ACGT, no sentinel, every position indexed; as a wrapped index, and as arrays for the checks (the
    host path of the library needs a file, so these tests check against what the rule says about planted queries)."""
    def __init__(self, ctx):
        rng = np.random.default_rng(31)
        self.text = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 6000)].copy()
        raw = self.text.tobytes()
        self.sa = np.array(sorted(range(len(raw)), key=lambda i: raw[i:]), dtype=np.int32)
        self.t = torch.from_numpy(self.text).cuda()
        self.ix = DeviceIndex.wrap(ctx, self.t, torch.from_numpy(self.sa).cuda(), is_dna=True)


@pytest.fixture(scope="module")
def plain(ctx):
    p = Plain(ctx)
    yield p
    p.ix.close()


def _witness(text, q, end, memo={}):
    from test_align_host import table, walk
    if memo.get("q") != q:
        memo.update(q=q, tab=table(text, q))
    return walk(memo["tab"], text, q, end)


@pytest.mark.parametrize("m", [1, 7, 8, 9, 63, 64, 65, 1000], ids=lambda m: f"m{m}")
def test_query_lengths_across_the_8_byte_loads(ctx, plain, m):
    """A slice of m bytes with one substitution, one insertion and one deletion where it is long enough (d = 1 below 63 bytes,
    3 from there on, 0 for a single byte); the records against the full-table witness."""
    raw = plain.text.tobytes()
    q = bytearray(raw[1500:1500 + m])
    d = 0
    if m >= 7:
        q[m // 2] = ord("A") if q[m // 2] != ord("A") else ord("C")
        d = 2 if m >= 63 else 1
    if m >= 63:
        q.insert(m // 4, ord("G") if q[m // 4] != ord("G") else ord("T"))
        del q[3 * m // 4]
        d = 3
    q = bytes(q)
    qb, off = pack_queries([q])
    dq, dv = _dev(qb, off)
    drecs = [t.contiguous() for t in plain.ix.edit_device(dq, dv, d, 0, False, m > 1)]
    recs = _np(drecs)
    assert len(recs[0]) > 0
    st, co, cg = trace_device(plain.ix, dq, dv, drecs)
    for t in range(len(recs[0])):
        assert (int(st[t]), cg[int(co[t]):int(co[t + 1])].tolist()) == _witness(plain.text, q, int(recs[2][t])), (m, t)
    assert same(plain.ix.edit_trace(qb, off, *recs), (st, co, cg))


def test_the_two_ends_of_a_text_without_a_sentinel(ctx, plain):
    """One query ends at n; the first two bytes of another are missing from the text's start: start 0 and a leading 2I."""
    raw = plain.text.tobytes()
    n = len(raw)
    head = b"TT" if raw[0:1] != b"T" else b"GG"
    queries = [raw[n - 40:n - 20] + b"N" + raw[n - 19:n], head + raw[0:30]]
    qb, off = pack_queries(queries)
    dq, dv = _dev(qb, off)
    drecs = [t.contiguous() for t in plain.ix.edit_device(dq, dv, 2)]
    recs = _np(drecs)
    st, co, cg = trace_device(plain.ix, dq, dv, drecs)
    got = {(int(recs[0][t]), int(recs[2][t])): (int(st[t]), sufr_amd.sufr_file.cigar_string(cg[int(co[t]):int(co[t + 1])])) for t in range(len(st))}
    assert got[(0, n - 1)] == (n - 40, "20=1X19=")
    assert got[(1, 29)] == (0, "2I30=")
    for t in range(len(st)):
        assert (int(st[t]), cg[int(co[t]):int(co[t + 1])].tolist()) == _witness(plain.text, queries[int(recs[0][t])], int(recs[2][t]))
    assert same(plain.ix.edit_trace(qb, off, *recs), (st, co, cg))


# ---------------------------------------------------------------------------------------------------------------------
# record counts and chunks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many(ctx):
    """About 5 000 records of 150-byte reads on both strands (records may repeat: the set is tiled up to 5 000), with the host's
    trace, computed once."""
    f = SufrFile(EXP / "long_dna_sequence.sufr")
    queries = [q for q in with_indels(np.random.default_rng(77), f, 400, 150) if q]
    qb, off = pack_queries(queries)
    recs = f.edit_arrays(qb, off, 3, 0, True, False)
    reps = -(-5000 // len(recs[0]))
    recs = [np.tile(a, reps)[:5000] for a in recs]
    ix = DeviceIndex.load(ctx, f)
    yield f, ix, qb, off, recs, f.edit_trace_arrays(qb, off, *recs)
    ix.close()


@pytest.mark.parametrize("count", [1, 63, 65, 257, 5000], ids=lambda c: f"records{c}")
def test_record_counts(ctx, many, count):
    f, ix, qb, off, recs, want = many
    some = [a[:count] for a in recs]
    runs = int(want[1][count])
    expect = (want[0][:count], want[1][:count + 1], want[2][:runs])
    assert same(trace_device(ix, *_dev(qb, off), _to_dev(some)), expect)
    assert same(ix.edit_trace(qb, off, *some), expect)


def test_chunks_5000_records_in_4_chunks_and_nomem_at_m1000(ctx, many, plain):
    f, ix, qb, off, recs, want = many
    longest = int(np.diff(off.astype(np.int64))[recs[0].astype(np.int64)].max())
    budget = 1664 * 8 * longest                                    # rows of 1 664 records
    assert -(-5000 // (budget // (8 * longest) // 64 * 64)) >= 3
    dq, dv = _dev(qb, off)
    try:
        ctx.set_trace_scratch(budget)
        assert same(trace_device(ix, dq, dv, _to_dev(recs)), want)
        ctx.set_trace_scratch(64 * 8 * longest)                    # one wave of records per chunk
        some = [a[:700] for a in recs]
        assert same(ix.edit_trace(qb, off, *some), (want[0][:700], want[1][:701], want[2][:int(want[1][700])]))
        # 64 records of a 1 000-byte query do not fit 64 * 8 * 1000 - 1 bytes
        q = plain.text.tobytes()[2000:3000]
        qb2, off2 = pack_queries([q])
        one = [np.array([0], dtype=np.uint64), np.array([0], dtype=np.uint8), np.array([2999], dtype=np.uint64), np.array([0], dtype=np.uint8)]
        ctx.set_trace_scratch(64 * 8 * 1000 - 1)
        with pytest.raises(SufrHipError) as e:
            plain.ix.edit_trace(qb2, off2, *one)
        assert e.value.code == -4 and "512000" in e.value.message
        ctx.set_trace_scratch(64 * 8 * 1000)
        st, co, cg = plain.ix.edit_trace(qb2, off2, *one)
        assert st.tolist() == [2000] and cg.tolist() == [1000 << 4 | 7]
    finally:
        ctx.set_trace_scratch(0)
    assert same(trace_device(ix, dq, dv, _to_dev(recs)), want)


# ---------------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------------
def test_invalid_records_and_capacity_as_on_the_host(ctx):
    f = SufrFile(EXP / "3.sufr")
    text = bytes(f.text)
    queries = [text[10:30] + b"X" + text[31:50], text[50:58], text[0:3]]
    qb, off = pack_queries(queries)
    dq, dv = _dev(qb, off)
    ix = DeviceIndex.load(ctx, f)
    good = f.edit_arrays(qb, off, 2, both_strands=True)
    want = f.edit_trace_arrays(qb, off, *good)
    t = next(i for i in range(len(good[0])) if good[3][i] == 1 and good[0][i] == 0)

    def broken(changes):
        recs = [a.copy() for a in good]
        for field, value in changes:
            recs[field][t] = value
        for call in (lambda: ix.edit_trace(qb, off, *recs), lambda: trace_device(ix, dq, dv, _to_dev(recs))):
            with pytest.raises(SufrHipError) as e:
                call()
            assert e.value.code == -1 and f"record {t}" in e.value.message, e.value.message
        assert same(ix.edit_trace(qb, off, *good), want)           # the next call on the context is right
    broken([(0, len(queries))])                                    # query >= num_queries
    broken([(1, 2)])                                               # strand > 1
    broken([(2, f.text_len)])                                      # end >= n
    broken([(3, 16)])                                              # edits > SUFR_EDIT_MAX_EDITS
    broken([(0, 2), (3, 3)])                                       # m < edits + 1
    broken([(3, 0)])                                               # edits one below D
    broken([(3, 2)])                                               # edits one above D
    # capacity
    total = len(want[2])
    nr = len(good[0])
    drecs = _to_dev(good)
    for cap in (0, total - 1):
        with pytest.raises(SufrHipError) as e:
            trace_device(ix, dq, dv, drecs, cap=cap)
        assert e.value.code == -5 and e.value.total == total
        with pytest.raises(SufrHipError) as e:
            ix.edit_trace(qb, off, *good, cap=cap)
        assert e.value.code == -5 and e.value.total == total
        start = torch.zeros(nr, dtype=torch.int64, device="cuda")
        coff = torch.full((nr + 1,), 0x5B, dtype=torch.int64, device="cuda")
        cigar = torch.full((total + 8,), 0x5B5B5B5B, dtype=torch.int32, device="cuda")
        n = C.c_uint64(0)
        rc = sufr_amd.lib().sufr_hip_edit_trace_device(ctx.handle, ix._h, dq.data_ptr(), dv.data_ptr(), len(queries), nr,
                                                       *[x.data_ptr() for x in drecs], cap, start.data_ptr(), coff.data_ptr(),
                                                       cigar.data_ptr() if cap else None, C.byref(n))
        ctx.synchronize()
        assert rc == -5 and n.value == total
        assert np.array_equal(start.cpu().numpy().view(np.uint64), want[0]) and np.array_equal(coff.cpu().numpy().view(np.uint64), want[1])
        assert bool((cigar[cap:] == 0x5B5B5B5B).all())             # nothing at or beyond the cap
        # the host-buffer twin: start and cigar_off come back with the capacity error
        hs, hc, hg = np.zeros(nr, dtype=np.uint64), np.zeros(nr + 1, dtype=np.uint64), np.full(total + 8, 0x5B5B5B5B, dtype=np.uint32)
        rc = sufr_amd.lib().sufr_hip_edit_trace(ctx.handle, ix._h, qb.ctypes.data, off.ctypes.data, len(queries), nr,
                                                *[a.ctypes.data for a in good], cap, hs.ctypes.data, hc.ctypes.data,
                                                hg.ctypes.data if cap else None, C.byref(n))
        assert rc == -5 and n.value == total and np.array_equal(hs, want[0]) and np.array_equal(hc, want[1])
        assert (hg[cap:] == 0x5B5B5B5B).all()
    assert same(trace_device(ix, dq, dv, drecs, cap=total), want)
    none = [a[:0] for a in good]
    st, co, cg = ix.edit_trace(qb, off, *none)
    assert len(st) == 0 and co.tolist() == [0] and len(cg) == 0
    st, co, cg = trace_device(ix, dq, dv, _to_dev(none))
    assert len(st) == 0 and co.tolist() == [0] and len(cg) == 0
    ix.close()


def test_align_on_the_device_is_align_on_the_host(ctx):
    f = SufrFile(EXP / "long_dna_sequence.sufr")
    queries = with_indels(np.random.default_rng(9), f, 30, 100)
    ix = DeviceIndex.load(ctx, f)
    got = ix.align(queries, 3, both_strands=True, local_minima=True)
    assert got == f.align(queries, 3, both_strands=True, local_minima=True) and sum(map(len, got)) > 0
    ix.close()


def test_two_contexts_on_one_index_at_the_same_time():
    f = SufrFile(EXP / "long_dna_sequence.sufr")
    rng = np.random.default_rng(23)
    batches = [pack_queries(with_indels(rng, f, 150, 150)) for _ in range(2)]
    recs = [f.edit_arrays(qb, off, 3, 0, True, bool(k)) for k, (qb, off) in enumerate(batches)]
    want = [f.edit_trace_arrays(qb, off, *r) for (qb, off), r in zip(batches, recs)]
    ctxs = [sufr_amd.Context(0), sufr_amd.Context(0)]
    longest = int(np.diff(batches[1][1].astype(np.int64))[recs[1][0].astype(np.int64)].max())
    ctxs[1].set_trace_scratch(64 * 8 * longest)                    # one of the two in chunks of 64 records
    assert len(recs[1][0]) > 3 * 64
    ix = DeviceIndex.load(ctxs[0], f)
    errors = []

    def work(k):
        mine = DeviceIndex(ctxs[k], ix._h)                         # the same index through this thread's context
        try:
            dq, dv = _dev(*batches[k])
            drecs = _to_dev(recs[k])
            for rep in range(5):
                if not same(trace_device(mine, dq, dv, drecs), want[k]):
                    errors.append(f"context {k}, call {rep}: the trace differs from the host's")
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
    for opts in (["-c"], ["-d", 4, "-l", "--cigar"], ["-d", 3, "-b", "-a", "-c"]):
        host = run("edit", *opts, "-q", fa, EXP / "long_dna_sequence.sufr").stdout
        dev = run("edit", "--device", 0, *opts, "-q", fa, EXP / "long_dna_sequence.sufr").stdout
        assert dev == host and host.count("\t") == 5 * host.count("\n") > 0
