"""Maximal exact matches (MEMs) on the host (include/sufr_mem.h): no GPU.

The witness depends on neither implementation: numpy over the file's own SA positions.  Row j of the query-by-text match
matrix (lcp_matrix of test_match_host, computed one row at a time from the last offset back) gives l(j, p) uncapped; a
position p of SA (rank order) is kept when l(j, p) >= k and the match does not extend left onto an indexed position; the
occurrence filter counts the p of SA with l(j, p) >= k' = min(k, L).  Strand 1 is the same on the reverse complement.
"""
import re
import subprocess
import zlib

import numpy as np
import pytest

import sufr_amd
from sufr_amd import SufrFile, SuffixArray, SufrHipError, pack_queries, synth
from oracle_helper import GOLDEN
from test_match_host import lcp_matrix, random_queries, run

EXP = GOLDEN / "expected"
SUFR1 = EXP / "1.sufr"
_RC = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(q: bytes) -> bytes:
    return bytes(q)[::-1].translate(_RC)


# ---------------------------------------------------------------------------------------------------------------------
# the witness
# ---------------------------------------------------------------------------------------------------------------------
def lcp_rows(q: bytes, text: np.ndarray):
    """Rows of lcp_matrix(q, text), from the last offset back: (j, R[j, :])."""
    n = text.size
    qa = np.frombuffer(q, dtype=np.uint8)
    prev = np.zeros(n + 1, dtype=np.int64)
    for j in range(len(q) - 1, -1, -1):
        cur = np.zeros(n + 1, dtype=np.int64)
        cur[:n] = (text == qa[j]) * (1 + prev[1:])
        yield j, cur[:n]
        prev = cur


def witness(f: SufrFile, queries, combos):
    """{(k, max_occ, both): (query, offset, strand, length, position) arrays in record order} for every combination."""
    text = np.asarray(f.text)
    sa = np.asarray(f.suffix_array).astype(np.int64)
    indexed = np.zeros(text.size, dtype=bool)
    indexed[sa] = True
    prev_ok = np.concatenate([[False], indexed[:-1]])[sa] if sa.size else np.zeros(0, dtype=bool)   # p > 0 and p - 1 indexed
    prev_byte = text[np.maximum(sa - 1, 0)]
    L = f.max_query_len
    recs = {c: [] for c in combos}
    for qi, q in enumerate(queries):
        for strand, qq in enumerate((bytes(q), revcomp(q))):
            per = {c: [] for c in combos if strand == 0 or c[2]}
            if not per:
                continue
            for j, row in lcp_rows(qq, text):
                r = row[sa]                                               # rank order
                ext = prev_ok & (prev_byte == qq[j - 1]) if j > 0 else np.zeros(sa.size, dtype=bool)
                for (k, occ, both) in per:
                    kk = min(k, L) if L else k
                    if j + k > len(qq) or (occ and int((r >= kk).sum()) > occ):
                        continue
                    ranks = np.nonzero((r >= k) & ~ext)[0]
                    if ranks.size:
                        per[(k, occ, both)].append((j, ranks, r[ranks]))
            for c, lst in per.items():
                for j, ranks, lens in reversed(lst):                      # (lcp_rows runs from the last offset back)
                    for rk, ln in zip(ranks, lens):
                        recs[c].append((qi, j, strand, int(ln), int(sa[rk])))
    return {c: np.array(v, dtype=np.int64).reshape(-1, 5) for c, v in recs.items()}


def stack(recs):
    return np.stack([np.asarray(a).astype(np.int64) for a in recs], axis=1) if len(recs[0]) else np.zeros((0, 5), dtype=np.int64)


COMBOS = [(k, occ, both) for k in (1, 3, 8) for occ in (0, 2) for both in (False, True)]


def check_file(f: SufrFile, queries, combos=COMBOS, threads=0):
    want = witness(f, queries, combos)
    qb, off = pack_queries(queries)
    n = 0
    for (k, occ, both) in combos:
        got = stack(f.mem_arrays(qb, off, k, occ, both, threads=threads))
        assert np.array_equal(got, want[(k, occ, both)]), (k, occ, both, got[:10], want[(k, occ, both)][:10])
        n += len(got)
    return n


def test_lcp_rows_are_lcp_matrix():
    rng = np.random.default_rng(1)
    text = np.frombuffer(b"ACGTTGCANNACGTACGT$", dtype=np.uint8)
    for q in (b"ACGT", b"TTGCANNAC", bytes(rng.choice(list(b"ACGTN"), 30).astype(np.uint8))):
        R = lcp_matrix(q, text)
        for j, row in lcp_rows(q, text):
            assert np.array_equal(row, R[j])


# ---------------------------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_mem_header_symbols_are_exported():
    hdr = (sufr_amd.LIB_PATH.parents[3] / "include" / "sufr_mem.h").read_text()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(sufr_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(sufr_amd.MEM_EXPORTS), declared ^ set(sufr_amd.MEM_EXPORTS)
    assert "#define SUFR_MEM_BOTH_STRANDS 0x1u" in hdr
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
    queries = random_queries(rng, f, 12 if big else 60, 60 if big else 16, extra=b"$%XN") + [b""]
    queries.append(bytes(f.text)[:3000])
    if f.seed_mask:
        with pytest.raises(SufrHipError) as e:
            f.mems(queries, 3)
        assert e.value.code == -6
        return
    combos = COMBOS if not big else [c for c in COMBOS if c[0] >= 3]
    assert check_file(f, queries, combos) > 0
    if big:                                                       # k = 1 on the short queries only (the slice has millions)
        assert check_file(f, queries[:-1], [c for c in COMBOS if c[0] == 1]) > 0


def _fasta_from(body: np.ndarray, path, width=60):
    """'%'-separated pieces of body -> one FASTA record each (the oracle joins them again)."""
    pieces = bytes(body).split(b"%")
    with open(path, "wb") as fh:
        for i, p in enumerate(pieces):
            fh.write(b">s%d\n" % i)
            for a in range(0, len(p), width):
                fh.write(p[a:a + width] + b"\n")


def _many_short(n=1500, seed=5):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGTN", dtype=np.uint8)
    parts = [acgt[rng.integers(0, 5 if i % 3 == 0 else 4, int(rng.integers(1, 30)))] for i in range(n // 15)]
    return np.concatenate([np.concatenate([p, np.frombuffer(b"%", dtype=np.uint8)]) for p in parts])[:-1]


ADVERSARIAL = ["all_a", "acgt_k", "tandem", "n_run", "many_short"]
BUILDS = [dict(is_dna=False), dict(is_dna=True), dict(is_dna=True, allow_ambiguity=True), dict(is_dna=True, ignore_softmask=True),
          dict(is_dna=True, max_query_len=3), dict(is_dna=True, max_query_len=6), dict(is_dna=False, max_query_len=11)]


def _adversarial_body(kind):
    if kind == "many_short":
        return _many_short()
    body = synth.adversarial(kind, 1200, seed=3)[:-1]
    if kind == "tandem":                                          # soft-masked stretches for --ignore-softmask
        body[100:300] = np.char.lower(body[100:300].view("S1")).view(np.uint8)
    return body


@pytest.mark.parametrize("kind", ADVERSARIAL)
@pytest.mark.parametrize("build", BUILDS)
def test_host_equals_witness_on_oracle_builds(oracle, tmp_path, kind, build):
    _fasta_from(_adversarial_body(kind), tmp_path / "x.fa")
    oracle.create(tmp_path / "x.fa", tmp_path / "x.sufr", **build)
    f = SufrFile(tmp_path / "x.sufr")
    rng = np.random.default_rng(zlib.crc32(f"{kind}{build}".encode()))
    queries = random_queries(rng, f, 12, 30, extra=b"N") + [b"A" * 40, b"NACGTACGT"]
    combos = [(k, occ, both) for k in (3, 8) for occ in (0, 2) for both in (False, True)]
    check_file(f, queries, combos)


def test_match_extends_left_onto_an_unindexed_n(oracle, tmp_path):
    (tmp_path / "n.fa").write_bytes(b">s\nGGGTTNACGTCCC\n")
    oracle.create(tmp_path / "n.fa", tmp_path / "n.sufr", is_dna=True)
    f = SufrFile(tmp_path / "n.sufr")
    assert 5 not in set(np.asarray(f.suffix_array).tolist())     # the N starts no indexed suffix
    hits = f.mems([b"NACGT"], min_len=4)
    assert [(h.query_offset, h.position, h.length, h.strand) for h in hits[0]] == [(1, 6, 4, 0)]
    plain = tmp_path / "p.sufr"
    oracle.create(tmp_path / "n.fa", plain, is_dna=False)         # indexed N: the match starts at the N instead
    assert [(h.query_offset, h.position, h.length) for h in SufrFile(plain).mems([b"NACGT"], min_len=4)[0]] == [(0, 5, 5)]


@pytest.mark.parametrize("L", [3, 6, 11])
def test_capped_build_gives_the_plain_mem_set(oracle, tmp_path, L):
    body = synth.adversarial("tandem", 2000, seed=9)[:-1]
    _fasta_from(body, tmp_path / "x.fa")
    oracle.create(tmp_path / "x.fa", tmp_path / "plain.sufr", is_dna=True)
    oracle.create(tmp_path / "x.fa", tmp_path / "cap.sufr", is_dna=True, max_query_len=L)
    p, c = SufrFile(tmp_path / "plain.sufr"), SufrFile(tmp_path / "cap.sufr")
    queries = random_queries(np.random.default_rng(L), p, 40, 60, extra=b"N")
    qb, off = pack_queries(queries)
    srt = lambda a: a[np.lexsort(a.T[::-1])]
    n = 0
    for k in (2, 4, 8, 15):
        for occ in (0, 3):
            if occ and k > L:
                continue
            for both in (False, True):
                a = stack(p.mem_arrays(qb, off, k, occ, both))
                b = stack(c.mem_arrays(qb, off, k, occ, both))
                assert np.array_equal(srt(a), srt(b)), (k, occ, both)
                n += len(a)
    assert n > 0


@pytest.mark.parametrize("threads", [0, 1, 2, 7])
def test_threads_do_not_change_the_answer(threads):
    f = SufrFile(EXP / "long_dna_sequence.sufr")
    queries = random_queries(np.random.default_rng(4), f, 300, 150)
    qb, off = pack_queries(queries)
    want = f.mem_arrays(qb, off, 10, 0, True, threads=1)
    got = f.mem_arrays(qb, off, 10, 0, True, threads=threads)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and len(want[0]) > 0


# ---------------------------------------------------------------------------------------------------------------------
# edge cases
# ---------------------------------------------------------------------------------------------------------------------
def test_capacity_min_len_and_empty_batches():
    f = SufrFile(EXP / "3.sufr")
    text = bytes(f.text)
    queries = [text[0:30] + b"X" + text[40:70], text[50:90], b"QQ"]
    qb, off = pack_queries(queries)
    want = f.mem_arrays(qb, off, 5, both_strands=True)
    n = len(want[0])
    assert n >= 3
    for cap in (0, 1, n - 1):
        with pytest.raises(SufrHipError) as e:
            f.mem_arrays(qb, off, 5, both_strands=True, cap=cap)
        assert e.value.code == -5 and e.value.total == n
    got = f.mem_arrays(qb, off, 5, both_strands=True, cap=n)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    with pytest.raises(SufrHipError) as e:
        f.mems([b"ACGT"], min_len=0)
    assert e.value.code == -1
    assert f.mems([], 3) == [] and f.mems([b""], 1) == [[]] and f.mems([b"", b"AC"], 3, both_strands=True) == [[], []]
    L = sufr_amd.lib()
    total = sufr_amd._lib.C.c_uint64(7)
    z = np.zeros(1, dtype=np.uint64)
    assert L.sufr_file_mems(f._h, None, z.ctypes.data, 0, 3, 0, 1, 0, None, None, None, None, None, sufr_amd._lib.C.byref(total), 1) == 0
    assert total.value == 0


def test_seed_mask_is_refused():
    f = SufrFile(EXP / "uniprot-masked.sufr")
    qb, off = pack_queries([b"RNELNNEEA"])
    with pytest.raises(SufrHipError) as e:
        f.mem_arrays(qb, off, 3)
    assert e.value.code == -6


def test_suffix_array_facade():
    sa = SuffixArray.read(str(SUFR1))
    h = sa.mems(["ACGTA"], min_len=3, both_strands=True)
    assert [(x.query_offset, x.position, x.length, x.strand) for x in h[0]] == [(0, 6, 4, 0), (0, 0, 4, 0), (1, 6, 4, 1), (1, 0, 4, 1)]


# ---------------------------------------------------------------------------------------------------------------------
# sufr mems
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_mems_hand_written_output(tmp_path):
    # 1.sufr: sequence "1" = ACGTNNACGT, --dna (the Ns start no indexed suffix).  ACGTA: ACGT at 6 (rank 1) and 0 (rank 2);
    # its reverse complement TACGT: ACGT from offset 1, both left-maximal (T != N at 5, T at -1).
    assert run("mems", "-k", 3, SUFR1, "ACGTA").stdout == "ACGTA\t+\t0\t4\t1:6\nACGTA\t+\t0\t4\t1:0\n"
    assert run("me", "-k", 3, "-b", SUFR1, "ACGTA").stdout == \
        "ACGTA\t+\t0\t4\t1:6\nACGTA\t+\t0\t4\t1:0\nACGTA\t-\t1\t4\t1:6\nACGTA\t-\t1\t4\t1:0\n"
    # NACGT: offset 1 (the N before it is not indexed); its reverse complement ACGTN runs on into the Ns at 0
    assert run("mems", "-k", 4, "-b", "--abs", SUFR1, "NACGT").stdout == \
        "NACGT\t+\t1\t4\t6\nNACGT\t+\t1\t4\t0\nNACGT\t-\t0\t4\t6\nNACGT\t-\t0\t5\t0\n"
    assert run("mems", "-k", 4, "--max-occ", 1, SUFR1, "ACGTA").stdout == ""   # ACGT starts 2 indexed suffixes
    assert run("mems", SUFR1, "ACGTA").stdout == ""                             # default min_len 20
    # named reads, -o.  CGTNN: CGT$ at 7 (rank order: '$' < 'N'), CGTNN at 1; its reverse complement NNACG: ACG from
    # offset 2 at 6 (the N before it at 5 is not indexed) and at 0
    fa = tmp_path / "r.fa"
    fa.write_bytes(b">r1 first\nACGTA\n>r2\nCGTNN\n")
    out = tmp_path / "o.tsv"
    run("mems", "-k", 3, "-b", "-q", fa, "-o", out, SUFR1)
    assert out.read_text() == ("r1\t+\t0\t4\t1:6\nr1\t+\t0\t4\t1:0\nr1\t-\t1\t4\t1:6\nr1\t-\t1\t4\t1:0\n"
                               "r2\t+\t0\t3\t1:7\nr2\t+\t0\t5\t1:1\nr2\t-\t2\t3\t1:6\nr2\t-\t2\t3\t1:0\n")


def test_cli_mems_errors():
    r = run("mems", "-k", 3, EXP / "uniprot-masked.sufr", "RNELNNEEA", check=False)
    assert r.returncode == 1 and r.stderr.startswith("Error: ") and "seed mask" in r.stderr
    r = run("mems", "-k", 0, SUFR1, "ACGT", check=False)
    assert r.returncode == 1 and r.stderr.startswith("Error: ")
    r = run("mems", SUFR1, check=False)
    assert r.returncode == 2
    r = run("mems", "-n", 2, SUFR1, "ACGT", check=False)                      # -n is match's
    assert r.returncode == 2
