"""Matching statistics and SMEMs on the host (include/sufr_match.h): no GPU.

The witness depends on neither implementation: numpy over the file's own SA positions, R[j, p] = lcp(Q[j..], T[p..]) from
the query-by-text match matrix, ms[j] = max over the indexed p of R[j, p] capped at the build's max_query_len, the SMEM
rule applied to that, and the rank range of every SMEM read off the ranks whose suffix starts with its slice.
"""
import re
import subprocess
import zlib

import numpy as np
import pytest

import sufr_amd
from sufr_amd import SufrFile, SuffixArray, SufrHipError, pack_queries, synth
from oracle_helper import GOLDEN

EXP = GOLDEN / "expected"
SUFR1 = EXP / "1.sufr"


def run(*args, check=True):
    r = subprocess.run([str(sufr_amd.CLI_PATH), *map(str, args)], capture_output=True, text=True)
    if check:
        assert r.returncode == 0, r.stderr
    return r


# ---------------------------------------------------------------------------------------------------------------------
# the witness
# ---------------------------------------------------------------------------------------------------------------------
def lcp_matrix(q: bytes, text: np.ndarray) -> np.ndarray:
    """R[j, p] = lcp(q[j:], text[p:]) for every query offset j and text position p."""
    m, n = len(q), text.size
    R = np.zeros((m + 1, n + 1), dtype=np.int64)
    qa = np.frombuffer(q, dtype=np.uint8)
    for a in range(m - 1, -1, -1):
        R[a, :n] = (text == qa[a]) * (1 + R[a + 1, 1:n + 1])
    return R[:m, :n]


def witness(f: SufrFile, q: bytes, min_len: int):
    """(ms, [(offset, length, rank_lo, rank_hi)]) of one query."""
    text = np.asarray(f.text)
    sa = np.asarray(f.suffix_array).astype(np.int64)
    m = len(q)
    if m == 0:
        return np.zeros(0, dtype=np.int64), []
    R = lcp_matrix(q, text)[:, sa]                                # rows: offsets, columns: ranks
    ms = R.max(axis=1) if sa.size else np.zeros(m, dtype=np.int64)
    if f.max_query_len:
        ms = np.minimum(ms, f.max_query_len)
    hits = []
    for j in range(m):
        if ms[j] >= min_len and (j == 0 or ms[j - 1] <= ms[j]):
            ranks = np.nonzero(R[j] >= ms[j])[0]
            assert ranks.size and np.array_equal(ranks, np.arange(ranks[0], ranks[-1] + 1)), (q, j)   # one rank range
            hits.append((j, int(ms[j]), int(ranks[0]), int(ranks[-1]) + 1))
    return ms, hits


def check_file(f: SufrFile, queries, min_lens=(1, 3, 8), threads=0):
    got_ms = f.matching_statistics(queries, threads=threads)
    smems = 0
    for k in min_lens:
        qb, off = pack_queries(queries)
        qi, qo, ln, lo, hi = f.smem_arrays(qb, off, k, threads=threads)
        got = {}
        for t in range(len(qi)):
            got.setdefault(int(qi[t]), []).append((int(qo[t]), int(ln[t]), int(lo[t]), int(hi[t])))
        assert np.all(np.diff(qi.astype(np.int64)) >= 0)                                         # (query, offset) order
        for i, q in enumerate(queries):
            ms, hits = witness(f, q, k)
            assert np.array_equal(got_ms[i].astype(np.int64), ms), (q, got_ms[i], ms)
            assert got.get(i, []) == hits, (q, k, got.get(i), hits)
            smems += len(hits)
    return smems


def random_queries(rng, f: SufrFile, count, max_len, extra=b""):
    """Substrings of the text with substitutions, pairs of distant pieces glued together, random strings."""
    text = bytes(f.text)
    alphabet = sorted(set(text) | set(extra))
    pick = lambda: alphabet[int(rng.integers(0, len(alphabet)))]
    qs = []
    for _ in range(count):
        kind = int(rng.integers(0, 4))
        L = int(rng.integers(1, max_len + 1))
        if kind == 0:
            at = int(rng.integers(0, len(text)))
            q = bytearray(text[at:at + L])
            for _ in range(int(rng.integers(0, 3))):
                if q:
                    q[int(rng.integers(0, len(q)))] = pick()
        elif kind == 1:
            a, b = (int(x) for x in rng.integers(0, len(text), 2))
            q = bytearray(text[a:a + L // 2] + text[b:b + L - L // 2])
        elif kind == 2:
            q = bytearray(pick() for _ in range(L))
        else:
            at = int(rng.integers(0, len(text)))
            q = bytearray(text[at:at + L])
        qs.append(bytes(q))
    return qs


# ---------------------------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_match_header_symbols_are_exported():
    hdr = (sufr_amd.LIB_PATH.parents[3] / "include" / "sufr_match.h").read_text()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(sufr_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(sufr_amd.MATCH_EXPORTS), declared ^ set(sufr_amd.MATCH_EXPORTS)
    L = sufr_amd.lib()
    for name in declared:
        assert hasattr(L, name), name
    nm = subprocess.run(["nm", "-D", "--defined-only", str(sufr_amd.LIB_PATH)], capture_output=True, text=True).stdout
    for name in declared:
        assert re.search(rf"\bT {name}\b", nm), name


# ---------------------------------------------------------------------------------------------------------------------
# against the witness
# ---------------------------------------------------------------------------------------------------------------------
GOLDEN_FILES = sorted(p.name for p in EXP.glob("*.sufr"))


@pytest.mark.parametrize("name", GOLDEN_FILES)
def test_host_equals_witness_on_golden_files(name):
    f = SufrFile(EXP / name)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    big = f.text_len > 2000
    queries = random_queries(rng, f, 25 if big else 80, 60 if big else 16, extra=b"$%X")
    if f.seed_mask:
        with pytest.raises(SufrHipError) as e:
            f.matching_statistics(queries)
        assert e.value.code == -6
        with pytest.raises(SufrHipError) as e:
            f.smems(queries, 3)
        assert e.value.code == -6
        return
    assert check_file(f, queries) > 0


def _fasta_from(body: np.ndarray, path, width=60):
    """'%'-separated pieces of body -> one FASTA record each (the oracle joins them again)."""
    pieces = bytes(body).split(b"%")
    with open(path, "wb") as fh:
        for i, p in enumerate(pieces):
            fh.write(b">s%d\n" % i)
            for a in range(0, len(p), width):
                fh.write(p[a:a + width] + b"\n")


ADVERSARIAL = ["all_a", "acgt_k", "fib", "two_identical", "n_run", "tandem"]


@pytest.mark.parametrize("kind", ADVERSARIAL)
@pytest.mark.parametrize("build", [dict(is_dna=True), dict(is_dna=True, allow_ambiguity=True), dict(is_dna=False),
                                   dict(is_dna=True, max_query_len=5), dict(is_dna=False, max_query_len=11)])
def test_host_equals_witness_on_oracle_builds(oracle, tmp_path, kind, build):
    body = synth.adversarial(kind, 1500, seed=3)[:-1]
    _fasta_from(body, tmp_path / "x.fa")
    oracle.create(tmp_path / "x.fa", tmp_path / "x.sufr", **build)
    f = SufrFile(tmp_path / "x.sufr")
    assert f.max_query_len == build.get("max_query_len", 0)
    rng = np.random.default_rng(zlib.crc32(f"{kind}{build}".encode()))
    queries = random_queries(rng, f, 30, 40, extra=b"N")
    assert check_file(f, queries, min_lens=(1, 4, 12)) > 0
    if f.max_query_len:                                           # the cap is visible: a long repeat stops at L
        text = bytes(f.text)
        ms = f.matching_statistics([text[:30]])[0]
        assert ms.max() <= f.max_query_len


def test_host_equals_witness_on_protein_and_repeats(oracle, tmp_path):
    rng = np.random.default_rng(17)
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    prot = aa[rng.integers(0, aa.size, 2500)]
    prot[1200:1500] = prot[100:400]                               # a long exact repeat
    with open(tmp_path / "p.fa", "wb") as fh:
        fh.write(b">p1\n" + bytes(prot[:1300]) + b"\n>p2\n" + bytes(prot[1300:]) + b"\n")
    for mql in (None, 7):
        oracle.create(tmp_path / "p.fa", tmp_path / "p.sufr", is_dna=False, max_query_len=mql)
        f = SufrFile(tmp_path / "p.sufr")
        queries = random_queries(rng, f, 30, 80) + [bytes(prot[90:420])]
        assert check_file(f, queries, min_lens=(2, 20)) > 0
        f.close()


@pytest.mark.parametrize("threads", [1, 3, 0])
def test_threads_do_not_change_the_answer(threads):
    f = SufrFile(EXP / "long_dna_sequence.sufr")
    rng = np.random.default_rng(4)
    queries = random_queries(rng, f, 300, 150)
    want = f.smems(queries, 10, threads=1)
    got = f.smems(queries, 10, threads=threads)
    assert [[(h.query_offset, h.length, h.rank_lo, h.rank_hi) for h in q] for q in got] == \
           [[(h.query_offset, h.length, h.rank_lo, h.rank_hi) for h in q] for q in want]
    assert sum(len(q) for q in got) > 0


# ---------------------------------------------------------------------------------------------------------------------
# edge cases
# ---------------------------------------------------------------------------------------------------------------------
def test_edge_cases():
    f = SufrFile(SUFR1)                                           # ACGTNNACGT$, --dna: the N suffixes are not indexed
    text = bytes(f.text)
    ms = f.matching_statistics([b"", b"XYZ", b"ACGTA", text, b"T$", b"%ACG", b"NNAC", b"acgt"])
    assert [list(m) for m in ms] == [[], [0, 0, 0], [4, 3, 2, 1, 1],
                                     [11, 10, 9, 8, 0, 0, 5, 4, 3, 2, 1],   # the whole text; no indexed suffix starts with N
                                     [2, 1], [0, 3, 2, 1], [0, 0, 2, 1], [0, 0, 0, 0]]
    hits = f.smems([b"", b"XYZ", b"ACGTA", text, b"ACG"], min_len=4)
    assert hits[0] == [] and hits[1] == [] and hits[4] == []      # min_len above the query's length
    assert [(h.query_offset, h.length, h.count, list(h.positions)) for h in hits[2]] == [(0, 4, 2, [6, 0])]
    assert [(h.query_offset, h.length, h.count, list(h.positions)) for h in hits[3]] == [(0, 11, 1, [0]), (6, 5, 1, [6])]
    assert f.smems([b"ACGTA"], min_len=3, max_hits=1)[0][0].positions.tolist() == [6]
    assert f.smems([], 3) == [] and f.matching_statistics([]) == []


def test_seed_mask_and_min_len_zero_are_refused():
    f = SufrFile(EXP / "uniprot-masked.sufr")
    qb, off = pack_queries([b"RNELNNEEA"])
    L = sufr_amd.lib()
    ms = np.zeros(9, dtype=np.uint32)
    assert L.sufr_file_matching_stats(f._h, qb.ctypes.data, off.ctypes.data, 1, ms.ctypes.data, 1) == -6
    with pytest.raises(SufrHipError) as e:
        f.smem_arrays(qb, off, 3)
    assert e.value.code == -6
    g = SufrFile(SUFR1)
    with pytest.raises(SufrHipError) as e:
        g.smems([b"ACGT"], min_len=0)
    assert e.value.code == -1


def test_capacity_shortfall_returns_the_total():
    f = SufrFile(EXP / "3.sufr")
    text = bytes(f.text)
    queries = [text[0:30] + b"X" + text[40:70], text[50:90], b"QQ"]
    qb, off = pack_queries(queries)
    want = f.smem_arrays(qb, off, 5)
    n = len(want[0])
    assert n >= 3
    for cap in (0, 1, n - 1):
        with pytest.raises(SufrHipError) as e:
            f.smem_arrays(qb, off, 5, cap=cap)
        assert e.value.code == -5 and e.value.total == n
    got = f.smem_arrays(qb, off, 5, cap=n)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_suffix_array_facade():
    sa = SuffixArray.read(str(SUFR1))
    h = sa.smems(["ACGTA"], min_len=3)
    assert [(x.query_offset, x.length, x.rank_lo, x.rank_hi, x.count) for x in h[0]] == [(0, 4, 1, 3, 2)]


# ---------------------------------------------------------------------------------------------------------------------
# sufr match
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_match_hand_written_output(tmp_path):
    # 1.sufr: sequence "1" = ACGTNNACGT.  ACGTA: ms = 4 3 2 1 1, one SMEM of length >= 3 at offset 0 (ACGT, ranks 1..3:
    # ACGT$ at 6, then ACGTNNACGT$ at 0).  GTNNA: ms = 3 (GTN) ...: N starts no indexed suffix, but GTN is a prefix of one.
    assert run("match", "-k", 3, SUFR1, "ACGTA", "GTNNA", "XX").stdout == \
        "ACGTA\t0\t4\t2\t1:0,1:6\nGTNNA\t0\t5\t1\t1:2\n"
    assert run("ma", "-k", 3, "--abs", SUFR1, "ACGTA").stdout == "ACGTA\t0\t4\t2\t6,0\n"
    assert run("match", "-k", 3, "-n", 1, SUFR1, "ACGTA").stdout == "ACGTA\t0\t4\t2\t1:6\n"
    assert run("match", "-k", 3, "-n", 1, "-a", SUFR1, "ACGTA").stdout == "ACGTA\t0\t4\t2\t6\n"
    assert run("match", SUFR1, "ACGTA").stdout == ""                          # default min_len 20
    assert run("match", "-k", 2, SUFR1, "TTACG").stdout == "TTACG\t2\t3\t2\t1:0,1:6\n"      # ms = 1 1 3 2 1
    # named reads, gzip included
    import gzip
    fa = tmp_path / "r.fa.gz"
    with gzip.open(fa, "wb") as fh:
        fh.write(b">r1 first\nACGTA\n>r2\nTTACG\n>r3\nQQQ\n")
    out = tmp_path / "o.tsv"
    run("match", "-k", 2, "-q", fa, "-o", out, SUFR1)
    assert out.read_text() == "r1\t0\t4\t2\t1:0,1:6\nr2\t2\t3\t2\t1:0,1:6\n"


def test_cli_match_errors():
    r = run("match", "-k", 3, EXP / "uniprot-masked.sufr", "RNELNNEEA", check=False)
    assert r.returncode == 1 and r.stderr.startswith("Error: ") and "seed mask" in r.stderr
    r = run("match", "-k", 0, SUFR1, "ACGT", check=False)
    assert r.returncode == 1 and r.stderr.startswith("Error: ")
    r = run("match", SUFR1, check=False)
    assert r.returncode == 2
