"""Matching statistics and SMEMs on a pair of FM-indexes on the GPU (include/sufr_fm_match.h, k_fm_ms of sufr_fm.inc) against the
host path of the same library, which tests/test_fm_match_host.py holds to a brute-force witness.  Every comparison is exact array
equality: the statistics and all five record columns.  The answers of the host are computed once per text and shared."""
import ctypes as C
import subprocess
import sys
import threading
from pathlib import Path

import numpy as np
import pytest
import torch

import sufr_amd
from sufr_amd import DeviceIndex, SufrFile, SufrHipError, pack_queries
from test_bwt_gpu import _unsigned, wrapped
from test_fm_host import sorted_sa
from test_fm_match_host import EXP, Pair, golden_pair, planted_bodies, query_set, reversal
from test_kmer_gpu import indexes
from test_lz_host import fibonacci, oracle_file

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
INVALID, CAPACITY = -1, -5
SLAB = 32                                                             # FM_MS_SLAB of sufr_fm.inc: the bytes of a lane
MIN_LENS = (1, 20)
DNA = "long_dna_sequence_allow_ambiguity.sufr"


@pytest.fixture(scope="module")
def ctx():
    c = sufr_amd.Context(0)
    yield c
    c.close()


@pytest.fixture
def pairs(oracle, tmp_path_factory):
    return lambda name: golden_pair(name, oracle, tmp_path_factory)


class Wanted:
    """the answers of the host pair for a query set: the statistics of the whole batch and the record columns per min_len"""

    def __init__(self, fwd, rev, qs, min_lens=MIN_LENS):
        self.qs = qs
        self.qb, self.off = pack_queries(qs)
        ms = fwd.matching_stats(qs, rev)
        self.ms = np.concatenate(ms).astype(np.uint64) if ms else np.zeros(0, dtype=np.uint64)
        self.cols = {k: fwd.smem_arrays(self.qb, self.off, rev, k) for k in min_lens}
        self.batch = (torch.from_numpy(self.qb).cuda(), torch.from_numpy(self.off.astype(np.int64)).cuda())


def host_wanted(p: Pair, qs, min_lens=MIN_LENS) -> Wanted:
    return Wanted(p.f.fm(32), p.g.fm(0), qs, min_lens)


def check_pair(dfwd, drev, want: Wanted, tag=""):
    total = int(want.off[-1])
    ms = dfwd.matching_stats_device(*want.batch, drev)
    assert ms.dtype == torch.int32 and np.array_equal(_unsigned(ms)[:total], want.ms), tag
    for k, cols in want.cols.items():
        got = dfwd.smems_device(*want.batch, drev, k)
        assert [t.dtype for t in got] == [torch.int64, torch.int32, torch.int32, torch.int64, torch.int64], tag
        for g, w in zip(got, cols):
            assert np.array_equal(_unsigned(g), w.astype(np.uint64)), (tag, k)
        assert np.array_equal(_unsigned(dfwd.last_ms)[:total], want.ms), (tag, k)       # d_ms receives the statistics


def reads_of(X: bytes, count: int, length: int, seed: int, symbols: bytes = b"ACGT"):
    """windows of the text with 0 to 3 substitutions"""
    rng = np.random.default_rng(seed)
    out = []
    for a in rng.integers(0, len(X) - length, count):
        r = bytearray(X[a:a + length])
        for at in rng.integers(0, length, int(rng.integers(0, 4))):
            r[at] = symbols[int(rng.integers(0, len(symbols)))]
        out.append(bytes(r))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the index variants: loaded, wrapped and 64-bit; the one-line shape and the wide ones; built there and uploaded
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [DNA, "uniprot.sufr", "2ns.sufr"])
def test_device_equals_host_on_golden_files(ctx, pairs, name):
    """the one-line shape (DNA at w = 4), K = 23 at w = 4 (96 + 160 in 256) and their 64-bit forms; a batch of 600 reads and the
    query set of the host tests, with the empty query, X and T in it"""
    p = pairs(name)
    symbols = bytes(sorted(set(p.X) - {ord("%")}))
    # (a query that matches whole costs a lane per slab an extension to its end: X and T stay in at 22 000 bytes, not at 63 000)
    qs = [q for q in query_set(p, seed=4) if len(q) < 30_000] + (reads_of(p.X, 600, 100, 2, symbols) if len(p.X) > 1000 else [])
    want = host_wanted(p, qs)
    assert len(want.cols[1][0]) > len(qs) // 2
    shapes = set()
    for (tag, ix, _), (_, rix, _) in zip(indexes(ctx, p.f), indexes(ctx, p.g)):
        drev = rix.fm_device(0)
        rix.close()
        for sample in (1, 32):
            dfwd = ix.fm_device(sample)
            shapes.add((dfwd.info["symbols"], dfwd.info["width"], dfwd.info["block"], dfwd.info["stride"]))
            check_pair(dfwd, drev, want, (name, tag, sample))
            dfwd.close()
        ix.close()
        drev.close()
    if name == DNA:
        assert (6, 4, 96, 128) in shapes and any(s[1] == 8 for s in shapes), shapes
    if name == "uniprot.sufr":
        assert (23, 4, 160, 256) in shapes, shapes
    # the other route: host builds uploaded
    dfwd, drev = p.f.fm(32).to_device(ctx), p.g.fm(0).to_device(ctx)
    check_pair(dfwd, drev, want, (name, "uploaded"))
    no_e = [q for q in want.qs[:40] if p.e not in q]
    assert repr(dfwd.smems(no_e, drev, 5, 2)) == repr(p.f.smems(no_e, 5, 2))
    assert [m.tolist() for m in dfwd.matching_stats(no_e, drev)] == [m.tolist() for m in p.f.matching_statistics(no_e)]


def test_all_byte_values_at_both_widths(ctx, tmp_path):
    """K = 256: stride 2048 at w = 4 and 4096 at w = 8"""
    from test_fm_match_host import planted_pair
    rng = np.random.default_rng(11)
    text = rng.integers(0, 255, 5000).astype(np.uint8)
    text[:255] = np.arange(255)
    text[-1] = 255
    p = planted_pair(tmp_path, text, "bytes")
    qs = query_set(p, seed=2, count=40) + reads_of(p.X, 60, 40, 3, bytes(range(255)))
    want = host_wanted(p, qs)
    strides = []
    for (tag, ix), (_, rix) in zip(wrapped(ctx, p.text, np.asarray(p.f.suffix_array)), wrapped(ctx, np.asarray(p.g.text), np.asarray(p.g.suffix_array))):
        dfwd, drev = ix.fm_device(32), rix.fm_device(0)
        ix.close(); rix.close()
        strides.append((dfwd.info["width"], dfwd.info["stride"]))
        check_pair(dfwd, drev, want, tag)
    assert strides == [(4, 2048), (8, 4096)]


def test_uploaded_pair_in_a_process_without_a_device_index(tmp_path, pairs):
    """both indexes built on the host and uploaded; the child process never makes a DeviceIndex: neither the text nor a suffix
    array is ever on the device"""
    p = pairs(DNA)
    p.f.fm(32).save(tmp_path / "fwd.fm")
    p.g.fm(0).save(tmp_path / "rev.fm")
    np.save(tmp_path / "reads.npy", np.frombuffer(b"\n".join(reads_of(p.X, 50, 80, 6)), dtype=np.uint8))
    script = tmp_path / "child.py"
    script.write_text(
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {str(ROOT)!r})\n"
        "import sufr_amd\nfrom sufr_amd import FmIndex, pack_queries\n"
        "def never(*a, **k): raise AssertionError('a DeviceIndex was made')\n"
        "sufr_amd.DeviceIndex.__init__ = never\n"
        f"d = {str(tmp_path)!r}\n"
        "fwd, rev = FmIndex.load(d + '/fwd.fm'), FmIndex.load(d + '/rev.fm')\n"
        "qs = np.load(d + '/reads.npy').tobytes().split(b'\\n')\n"
        "ctx = sufr_amd.Context(0)\n"
        "dfwd, drev = fwd.to_device(ctx), rev.to_device(ctx)\n"
        "assert [m.tolist() for m in dfwd.matching_stats(qs, drev)] == [m.tolist() for m in fwd.matching_stats(qs, rev)]\n"
        "assert repr(dfwd.smems(qs, drev, 12)) == repr(fwd.smems(qs, rev, 12)) and any(dfwd.smems(qs, drev, 12))\n"
        "print('same')\n")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "same", r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------------------------------
# the inputs: one long query over many slabs, runs and periodic texts, batches on the cuts, a batch of one
# ---------------------------------------------------------------------------------------------------------------------
def random_pair(tmp_path, n: int, seed: int) -> Pair:
    """random DNA, where 64 bytes tell any two suffixes apart: the arrays of the text and of its reversal"""
    from test_bwt_host import write_arrays
    rng = np.random.default_rng(seed)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()
    text[-1] = ord("$")
    files = []
    for tag, t in (("f", text), ("r", reversal(text))):
        raw = t.tobytes()
        sa = np.array(sorted(range(n), key=lambda q: raw[q:q + 64]), dtype=np.uint32)
        files.append(write_arrays(tmp_path / f"{tag}.sufr", t, sa))
    return Pair(*files)


def test_one_long_query_over_many_slabs(ctx, tmp_path):
    """40 000 bytes cut from a random text of 50 000 with a substitution every 997 bytes: 1 250 slabs of 32, more than one
    workgroup; the statistics between two substitutions fall by one per byte from almost a thousand"""
    p = random_pair(tmp_path, 50_000, 13)
    q = bytearray(p.X[5000:45_000])
    for at in range(500, len(q), 997):
        q[at] = b"ACGT"[(b"ACGT".index(q[at]) + 1) % 4]
    want = host_wanted(p, [bytes(q), bytes(q[:1]), bytes(q[100:4000])], (1, 20, 500))
    assert len(q) // SLAB > 2 * 256 and int(want.ms.max()) > 900 and len(want.cols[500][0]) > 40
    dfwd, drev = p.f.fm(32).to_device(ctx), p.g.fm(0).to_device(ctx)
    check_pair(dfwd, drev, want)
    one = host_wanted(p, [bytes(q[:777])])                             # a batch of one
    check_pair(dfwd, drev, one)
    for (tag, ix), (_, rix) in zip(wrapped(ctx, p.text, np.asarray(p.f.suffix_array)), wrapped(ctx, np.asarray(p.g.text), np.asarray(p.g.suffix_array))):
        a, b = ix.fm_device(1), rix.fm_device(0)
        ix.close(); rix.close()
        check_pair(a, b, want, tag)


def test_runs_and_periodic_texts(ctx, oracle, tmp_path):
    """A^1000 and a Fibonacci string with queries of 2 000 A and a Fibonacci prefix: every lane's extension runs to the query's end"""
    for name, body in planted_bodies().items():
        f = oracle_file(oracle, tmp_path, body, name, is_dna=True, allow_ambiguity=True)
        f.write_reversed_fasta(tmp_path / f"{name}_rev.fa")
        oracle.create(tmp_path / f"{name}_rev.fa", tmp_path / f"{name}_rev.sufr", is_dna=True, allow_ambiguity=True)
        p = Pair(f, SufrFile(tmp_path / f"{name}_rev.sufr"))
        qs = query_set(p, seed=7, count=16, max_len=300) + [b"A" * 2000, bytes(fibonacci(2584)), p.X[:500] + b"C" + p.X[400:]]
        want = host_wanted(p, qs)
        for (tag, ix, _), (_, rix, _) in zip(indexes(ctx, p.f), indexes(ctx, p.g)):
            dfwd, drev = ix.fm_device(7), rix.fm_device(0)
            ix.close(); rix.close()
            check_pair(dfwd, drev, want, (name, tag))


def test_slab_cuts_on_and_beside_query_boundaries(ctx, pairs):
    """queries whose ends fall on a slab cut, one byte before it and one byte after it, and one longer than three slabs with a
    substitution behind its first cut"""
    p = pairs(DNA)
    lengths = [SLAB, SLAB - 1, 2, SLAB - 1, 0, SLAB + 1, SLAB - 2, 1, 3 * SLAB, 1, SLAB - 1, 7]
    ends = np.cumsum(lengths)
    assert {0, 1, SLAB - 1} <= {int(e) % SLAB for e in ends}
    rng = np.random.default_rng(4)
    qs = [p.X[int(a):int(a) + n] for a, n in zip(rng.integers(0, len(p.X) - 4 * SLAB, len(lengths)), lengths)]
    qs[8] = qs[8][:SLAB + 9] + b"T" + qs[8][SLAB + 10:]
    want = host_wanted(p, qs, (1, 5))
    check_pair(p.f.fm(32).to_device(ctx), p.g.fm(0).to_device(ctx), want)


# ---------------------------------------------------------------------------------------------------------------------
# call shapes, lifetime, refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_capacity_the_empty_batch_and_equal_bytes(ctx, pairs):
    p = pairs(DNA)
    want = host_wanted(p, query_set(p, seed=8)[4:] + reads_of(p.X, 40, 60, 1), (5,))
    cols = want.cols[5]
    z, nq = len(cols[0]), len(want.qs)
    assert z > 20
    dfwd, drev = p.f.fm(32).to_device(ctx), p.g.fm(0).to_device(ctx)
    L = sufr_amd.lib()
    qb, off = want.batch
    ms = torch.zeros(int(want.off[-1]), dtype=torch.int32, device="cuda")
    out = [torch.full((z + 3,), -1, dtype=d, device="cuda") for d in (torch.int64, torch.int32, torch.int32, torch.int64, torch.int64)]
    total = C.c_uint64(0)
    args = (ctx.handle, dfwd._h, drev._h, qb.data_ptr(), off.data_ptr(), nq, 5, ms.data_ptr())
    assert L.sufr_hip_fm_smems_device(*args, z - 1, *[t.data_ptr() for t in out], C.byref(total)) == CAPACITY
    ctx.synchronize()
    assert total.value == z and all((t == -1).all() for t in out)      # nothing filled
    assert "room for" in L.sufr_hip_last_error(ctx.handle).decode()
    ctx.check(L.sufr_hip_fm_smems_device(*args, z, *[t.data_ptr() for t in out], C.byref(total)))
    ctx.synchronize()
    first = [t.cpu().numpy().tobytes() for t in out] + [ms.cpu().numpy().tobytes()]
    assert total.value == z and all(np.array_equal(_unsigned(t)[:z], w.astype(np.uint64)) and (t[z:] == -1).all() for t, w in zip(out, cols))
    ctx.check(L.sufr_hip_fm_smems_device(*args, z, *[t.data_ptr() for t in out], C.byref(total)))
    ctx.synchronize()
    assert [t.cpu().numpy().tobytes() for t in out] + [ms.cpu().numpy().tobytes()] == first          # two calls, equal bytes
    assert L.sufr_hip_fm_smems_device(ctx.handle, dfwd._h, drev._h, qb.data_ptr(), off.data_ptr(), nq, 0, ms.data_ptr(), z, *[t.data_ptr() for t in out],
                                      C.byref(total)) == INVALID
    # the host-pointer entry point
    host = [np.full(z + 3, 0xAB, dtype=np.uint8).repeat(w.itemsize).view(w.dtype) for w in cols]
    hargs = (ctx.handle, dfwd._h, drev._h, want.qb.ctypes.data, want.off.ctypes.data, nq, 5)
    assert L.sufr_hip_fm_smems(*hargs, z - 1, *[a.ctypes.data for a in host], C.byref(total)) == CAPACITY and total.value == z
    assert all((a.view(np.uint8) == 0xAB).all() for a in host)
    ctx.check(L.sufr_hip_fm_smems(*hargs, z, *[a.ctypes.data for a in host], C.byref(total)))
    assert total.value == z and all(np.array_equal(a[:z], w) for a, w in zip(host, cols))
    # no queries, and queries of no bytes
    total.value = 9
    ctx.check(L.sufr_hip_fm_matching_stats_device(ctx.handle, dfwd._h, drev._h, None, None, 0, None))
    ctx.check(L.sufr_hip_fm_smems_device(ctx.handle, dfwd._h, drev._h, None, None, 0, 5, None, 0, None, None, None, None, None, C.byref(total)))
    assert total.value == 0
    total.value = 9
    ctx.check(L.sufr_hip_fm_smems(ctx.handle, dfwd._h, drev._h, None, None, 0, 5, 0, None, None, None, None, None, C.byref(total)))
    assert total.value == 0
    assert dfwd.matching_stats([b"", b""], drev)[0].size == 0 and dfwd.smems([b"", b""], drev, 1) == [[], []]
    none = dfwd.smems_device(torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"), drev, 1)
    assert all(t.numel() == 0 for t in none)


def test_the_pair_outlives_its_arrays(ctx, pairs):
    p = pairs(DNA)
    want = host_wanted(p, query_set(p, seed=5)[4:], (5,))
    held = []
    made = []
    for f in (p.f, p.g):
        d_text = torch.from_numpy(np.array(f.text)).cuda()
        d_sa = torch.from_numpy(np.array(f.suffix_array).view(np.int32)).cuda()
        ix = DeviceIndex.wrap(ctx, d_text, d_sa, is_dna=True, prefix_table=False)
        made.append(ix.fm_device(32 if f is p.f else 0))
        ix.close()
        d_text.zero_(); d_sa.zero_()
        held += [d_text, d_sa]
    torch.cuda.synchronize()
    check_pair(*made, want, "zeroed")
    del held[:]
    torch.cuda.empty_cache()
    check_pair(*made, want, "freed")


def test_a_mismatched_pair_is_refused(ctx, pairs):
    p, other = pairs(DNA), pairs("abba.sufr")
    dfwd, drev, wrong = p.f.fm(32).to_device(ctx), p.g.fm(0).to_device(ctx), other.g.fm(0).to_device(ctx)
    qb, off = (torch.from_numpy(a).cuda() for a in (np.frombuffer(b"ACGTACGT", dtype=np.uint8).copy(), np.array([0, 8], dtype=np.int64)))
    for call in (lambda: dfwd.matching_stats_device(qb, off, wrong), lambda: dfwd.smems_device(qb, off, wrong, 1), lambda: wrong.smems_device(qb, off, dfwd, 1)):
        with pytest.raises(SufrHipError) as err:
            call()
        assert err.value.code == INVALID and "not an index of the reversed text" in str(err.value)
    total = C.c_uint64(0)
    host = [np.zeros(8, dtype=d) for d in (np.uint64, np.uint32, np.uint32, np.uint64, np.uint64)]
    assert sufr_amd.lib().sufr_hip_fm_smems(ctx.handle, dfwd._h, wrong._h, b"ACGTACGT", np.array([0, 8], dtype=np.uint64).ctypes.data, 1, 1, 8,
                                            *[a.ctypes.data for a in host], C.byref(total)) == INVALID
    check_pair(dfwd, drev, host_wanted(p, [b"ACGTACGT", p.X[50:90]], (1,)))      # the context goes on working


def test_two_contexts_on_two_threads(ctx, pairs):
    """two contexts, each with the pair of a different file, answer at once on two host threads"""
    ps = [pairs("uniprot.sufr"), pairs(DNA)]
    wants = [host_wanted(p, query_set(p, seed=2)[4:] + reads_of(p.X, 100, 80, 3, bytes(sorted(set(p.X) - {ord("%")}))), (5,)) for p in ps]
    other = sufr_amd.Context(0)
    errors = []

    def work(c, p, want):
        try:
            for _ in range(3):
                dfwd, drev = p.f.fm(32).to_device(c), p.g.fm(0).to_device(c)
                check_pair(dfwd, drev, want)
                dfwd.close(); drev.close()
        except BaseException as e:                                   # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=work, args=(c, p, want)) for c, p, want in zip((ctx, other), ps, wants)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    other.close()
    assert not errors, errors


def test_cli_on_the_device_prints_the_host_lines(oracle, tmp_path):
    from test_fm_match_host import cli_files, cli_queries
    from test_match_host import run
    src, rev, fwd_fm, rev_fm = cli_files(oracle, tmp_path, DNA)
    queries = cli_queries(src, DNA)
    want = run("match", "-k", 5, src, *queries).stdout
    assert want and run("fm", src, "--smems", "--reverse", rev, "-k", 5, "--device", 0, *queries).stdout == want
    assert run("fm", "--index", fwd_fm, "--smems", "--reverse", rev_fm, "-k", 5, "--device", 0, *queries).stdout == want


def test_cli_smems_with_max_hits_on_the_device_prints_the_host_lines(oracle, tmp_path):
    """the positions of --smems come through the device locate of --locate, cut at --max-hits"""
    from test_fm_match_host import cli_files, cli_queries
    from test_match_host import run
    src, rev, fwd_fm, rev_fm = cli_files(oracle, tmp_path, DNA)
    queries = cli_queries(src, DNA)
    for args in ((src, "--smems", "--reverse", rev), ("--index", fwd_fm, "--smems", "--reverse", rev_fm, "-a")):
        want = run("fm", *args, "-k", 5, "--max-hits", 1, *queries).stdout
        assert want and run("fm", *args, "-k", 5, "--max-hits", 1, "--device", 0, *queries).stdout == want


def test_one_batch_through_both_device_classes(ctx, tmp_path):
    """DeviceIndex and DeviceFmIndex answer through one batch path: the same queries through both give the same counts,
    positions (cut at max_hits) and SMEMs, an empty query and one that does not occur among them"""
    from test_fm_match_host import planted_pair
    rng = np.random.default_rng(5)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 3001)].copy()
    text[-1] = ord("$")
    p = planted_pair(tmp_path, text, "both")
    qs = [p.X[a:a + n] for a, n in ((0, 40), (17, 3), (1500, 25), (2990, 10), (64, 1), (700, 60), (2000, 12), (333, 7))]
    qs += [b"", b"ACGTN", p.X[100:130] + p.X[2500:2530], p.X[5:25] + b"N" + p.X[900:920]]      # (no end byte: the pair matches in T[:-1])
    ix, rix = DeviceIndex.load(ctx, p.f), DeviceIndex.load(ctx, p.g)
    fm, rev = ix.fm_device(7), rix.fm_device(0)
    rix.close()
    counts = p.f.count(qs)                                            # the host file is the reference of both
    assert fm.count(qs) == ix.count(qs) == counts and counts[8].count == text.size and sum(c.count == 0 for c in counts) >= 2
    sa, (lo, hi) = np.asarray(p.f.suffix_array), p.f.search_batch(qs)
    for i, (a, b) in enumerate(zip(fm.locate(qs, max_hits=2), ix.locate(qs, max_hits=2))):
        want = sa[int(lo[i]):int(lo[i]) + min(int(hi[i] - lo[i]), 2)]
        assert a.dtype == b.dtype == want.dtype and np.array_equal(a, want) and np.array_equal(b, want), i
    for min_len in (1, 20):
        want = p.f.smems(qs, min_len, max_hits=1)
        assert repr(fm.smems(qs, rev, min_len, max_hits=1)) == repr(ix.smems(qs, min_len, max_hits=1)) == repr(want), min_len
        assert len(want) == len(qs) and any(want) and all(h.positions.size == 1 for hits in want for h in hits)
    for x in (fm, rev, ix):
        x.close()
