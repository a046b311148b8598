"""k-mismatch search on the host (include/sufr_approx.h): no GPU.

The witness depends on neither implementation: numpy over the file's own text and SA.  One pass over the query bytes sums
text[p + t] != q[t] for every window start p, which gives h(p) and, from the running sums at the piece boundaries, which
pieces match exactly where; `indexed` comes from SA; a piece is live by the count of indexed positions that match its
k'-seed; records are ordered by walking SA once per piece.
"""
import re
import subprocess
import zlib

import numpy as np
import pytest

import sufr_amd
from sufr_amd import SufrFile, SuffixArray, SufrHipError, pack_queries, synth
from oracle_helper import GOLDEN
from test_match_host import random_queries, run
from test_mem_host import ADVERSARIAL, BUILDS, _adversarial_body, _fasta_from, revcomp

EXP = GOLDEN / "expected"
SUFR1 = EXP / "1.sufr"
DS = (0, 1, 2, 4)
COMBOS = [(d, occ, both) for d in DS for occ in (0, 2) for both in (False, True)]


# ---------------------------------------------------------------------------------------------------------------------
# the witness
# ---------------------------------------------------------------------------------------------------------------------
def occurrences(text: np.ndarray, s: bytes) -> np.ndarray:
    """ok[x] = text[x : x + len(s)] == s (False where it does not fit)."""
    ok = np.zeros(text.size, dtype=bool)
    w = text.size - len(s) + 1
    if w <= 0:
        return ok
    ok[:w] = True
    for t, c in enumerate(s):
        ok[:w] &= text[t:t + w] == c
    return ok


def witness_one(text, sa, indexed, L, q: bytes, ds, occs):
    """{(d, occ): [(position, mismatches)] in record order} of one query on one strand."""
    n, m = text.size, len(q)
    out = {(d, occ): [] for d in ds for occ in occs}
    w = n - m + 1
    if m == 0 or w <= 0:
        return out
    bounds = {i * m // (d + 1) for d in ds for i in range(d + 2)}
    cum = np.zeros(w, dtype=np.int32)
    snap = {0: cum.copy()}
    for t in range(m):
        cum += text[t:t + w] != q[t]
        if t + 1 in bounds:
            snap[t + 1] = cum.copy()
    h = cum
    for d in ds:
        if m < d + 1:
            continue
        o = [i * m // (d + 1) for i in range(d + 2)]
        exact = [(snap[o[i + 1]] - snap[o[i]]) == 0 for i in range(d + 1)]
        starts = [indexed[o[i]:o[i] + w] for i in range(d + 1)]
        seeds = [q[o[i]:o[i] + (min(o[i + 1] - o[i], L) if L else o[i + 1] - o[i])] for i in range(d + 1)]
        occ_of = [int((occurrences(text, s) & indexed).sum()) for s in seeds] if any(occs) else [0] * (d + 1)
        for occ in occs:
            lowest = np.full(w, -1, dtype=np.int64)
            for i in range(d, -1, -1):
                if occ == 0 or occ_of[i] <= occ:
                    lowest[exact[i] & starts[i]] = i
            lowest[h > d] = -1
            for i in range(d + 1):
                p = sa - o[i]
                ok = (p >= 0) & (p < w)
                ok[ok] = lowest[p[ok]] == i
                out[(d, occ)].extend((int(x), int(h[x])) for x in p[ok])
    return out


def witness(f: SufrFile, queries, combos):
    """{(d, occ, both): (query, strand, position, mismatches) rows in record order}."""
    text = np.asarray(f.text)
    sa = np.asarray(f.suffix_array).astype(np.int64)
    indexed = np.zeros(text.size, dtype=bool)
    indexed[sa] = True
    ds = sorted({c[0] for c in combos})
    occs = sorted({c[1] for c in combos})
    recs = {c: [] for c in combos}
    for qi, q in enumerate(queries):
        per = [witness_one(text, sa, indexed, f.max_query_len, qq, ds, occs) for qq in (bytes(q), revcomp(q))]
        for (d, occ, both) in combos:
            for strand in range(2 if both else 1):
                recs[(d, occ, both)].extend((qi, strand, p, hh) for p, hh in per[strand][(d, occ)])
    return {c: np.array(v, dtype=np.int64).reshape(-1, 4) for c, v in recs.items()}


def stack(recs):
    return np.stack([np.asarray(a).astype(np.int64) for a in recs], axis=1) if len(recs[0]) else np.zeros((0, 4), dtype=np.int64)


def check_file(f: SufrFile, queries, combos=COMBOS, threads=0):
    want = witness(f, queries, combos)
    qb, off = pack_queries(queries)
    n = 0
    for (d, occ, both) in combos:
        got = stack(f.approx_arrays(qb, off, d, occ, both, threads=threads))
        assert np.array_equal(got, want[(d, occ, both)]), (d, occ, both, got[:10], want[(d, occ, both)][:10])
        n += len(got)
    return n


def planted(rng, f: SufrFile, count, max_len, extra=b"$%XN"):
    """Slices of the text with 0..4 substitutions (bytes of the text and of `extra`), on top of random_queries; the empty
    query, slices of every length 0..5 (the lengths d and d + 1 of every d tested) and a 3 000-byte prefix."""
    text = bytes(f.text)
    alphabet = sorted(set(text) | set(extra))
    qs = random_queries(rng, f, count, max_len, extra=extra)
    for _ in range(count):
        m = int(rng.integers(1, max_len + 1))
        at = int(rng.integers(0, max(len(text) - m, 1)))
        q = bytearray(text[at:at + m])
        for _ in range(int(rng.integers(0, 5))):
            q[int(rng.integers(0, len(q)))] = alphabet[int(rng.integers(0, len(alphabet)))]
        qs.append(bytes(q))
    at = int(rng.integers(0, max(len(text) - 5, 1)))
    qs += [text[at:at + m] for m in range(6)] + [b"", b"$", b"N%", b"X" * 5, text[:3000]]
    return qs


def test_witness_on_a_hand_checked_text():
    # ACGTACGA: ACGA at 4 exactly; at 0 with one mismatch (T for A).  d = 1: pieces AC | GA; window 0 is anchored by AC,
    # window 4 by AC too (the lowest piece), in rank order of the suffixes that start with AC: ACGA (4) before ACGT (0)
    text = np.frombuffer(b"ACGTACGA", dtype=np.uint8)
    sa = np.array(sorted(range(8), key=lambda p: bytes(text[p:])), dtype=np.int64)
    got = witness_one(text, sa, np.ones(8, dtype=bool), 0, b"ACGA", (0, 1), (0, 1))
    assert got[(0, 0)] == [(4, 0)] and got[(1, 0)] == [(4, 0), (0, 1)]
    assert got[(1, 1)] == [(4, 0)]                                # AC starts two suffixes: dead; GA anchors window 4 only
    assert got[(0, 1)] == [(4, 0)]


# ---------------------------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_approx_header_symbols_are_exported():
    hdr = (sufr_amd.LIB_PATH.parents[3] / "include" / "sufr_approx.h").read_text()
    assert "#define SUFR_APPROX_BOTH_STRANDS 0x1u" in hdr and "#define SUFR_APPROX_MAX_MISMATCHES 15u" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(sufr_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(sufr_amd.APPROX_EXPORTS), declared ^ set(sufr_amd.APPROX_EXPORTS)
    L = sufr_amd.lib()
    for name in declared:
        assert hasattr(L, name), name
    nm = subprocess.run(["nm", "-D", "--defined-only", str(sufr_amd.LIB_PATH)], capture_output=True, text=True).stdout
    for name in declared:
        assert re.search(rf"\bT {name}\b", nm), name
    assert L.sufr_hip_abi_version() == 3


# ---------------------------------------------------------------------------------------------------------------------
# against the witness
# ---------------------------------------------------------------------------------------------------------------------
GOLDEN_FILES = sorted(p.name for p in EXP.glob("*.sufr"))


@pytest.mark.parametrize("name", GOLDEN_FILES)
def test_host_equals_witness_on_golden_files(name):
    f = SufrFile(EXP / name)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    big = f.text_len > 2000
    queries = planted(rng, f, 10 if big else 40, 60 if big else 16)
    if f.seed_mask:
        with pytest.raises(SufrHipError) as e:
            f.approx(queries, 2)
        assert e.value.code == -6
        return
    assert check_file(f, queries) > 0


@pytest.mark.parametrize("kind", ADVERSARIAL)
@pytest.mark.parametrize("build", BUILDS)
def test_host_equals_witness_on_oracle_builds(oracle, tmp_path, kind, build):
    _fasta_from(_adversarial_body(kind), tmp_path / "x.fa")
    oracle.create(tmp_path / "x.fa", tmp_path / "x.sufr", **build)
    f = SufrFile(tmp_path / "x.sufr")
    rng = np.random.default_rng(zlib.crc32(f"{kind}{build}".encode()))
    queries = planted(rng, f, 10, 40) + [b"A" * 40, b"NACGTACGT"]
    assert check_file(f, queries) > 0


def test_host_equals_witness_on_a_protein_build(oracle, tmp_path):
    rng = np.random.default_rng(8)
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    body = aa[rng.integers(0, 20, 1500)].copy()
    body[700:760] = body[100:160]                                  # a repeat, so that windows share pieces
    body[[400, 900]] = ord("%")
    _fasta_from(body, tmp_path / "p.fa")
    oracle.create(tmp_path / "p.fa", tmp_path / "p.sufr", is_dna=False)
    f = SufrFile(tmp_path / "p.sufr")
    assert check_file(f, planted(rng, f, 30, 50)) > 0


@pytest.mark.parametrize("L", [3, 6, 11])
def test_capped_build_gives_the_plain_record_set(oracle, tmp_path, L):
    body = synth.adversarial("tandem", 2000, seed=9)[:-1]
    _fasta_from(body, tmp_path / "x.fa")
    oracle.create(tmp_path / "x.fa", tmp_path / "plain.sufr", is_dna=True)
    oracle.create(tmp_path / "x.fa", tmp_path / "cap.sufr", is_dna=True, max_query_len=L)
    p, c = SufrFile(tmp_path / "plain.sufr"), SufrFile(tmp_path / "cap.sufr")
    qb, off = pack_queries(planted(np.random.default_rng(L), p, 40, 60))
    srt = lambda a: a[np.lexsort(a.T[::-1])]
    n = 0
    for d in DS:
        for both in (False, True):
            a = stack(p.approx_arrays(qb, off, d, 0, both))
            b = stack(c.approx_arrays(qb, off, d, 0, both))
            assert np.array_equal(srt(a), srt(b)), (d, both)
            n += len(a)
    assert n > 0


@pytest.mark.parametrize("name", ["3.sufr", "long_dna_sequence.sufr", "uniprot.sufr"])
def test_no_mismatch_is_locate(name):
    f = SufrFile(EXP / name)
    queries = [q for q in planted(np.random.default_rng(11), f, 30, 40) if 0 < len(q) <= f.text_len]
    hits = f.approx(queries, 0)
    n = 0
    for q, hs, loc in zip(queries, hits, f.locate(queries)):
        assert sorted(h.position for h in hs) == sorted(p.suffix for p in loc.positions), q
        assert all(h.mismatches == 0 and h.strand == 0 for h in hs)
        n += len(hs)
    assert n > 0


@pytest.mark.parametrize("threads", [3, 16])
def test_threads_do_not_change_the_answer(threads):
    f = SufrFile(EXP / "long_dna_sequence.sufr")
    qb, off = pack_queries(planted(np.random.default_rng(4), f, 300, 150))
    want = f.approx_arrays(qb, off, 3, 0, True, threads=1)
    got = f.approx_arrays(qb, off, 3, 0, True, threads=threads)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and len(want[0]) > 0


# ---------------------------------------------------------------------------------------------------------------------
# edge cases
# ---------------------------------------------------------------------------------------------------------------------
def test_limits_capacity_and_empty_batches():
    f = SufrFile(EXP / "3.sufr")
    text = bytes(f.text)
    queries = [text[0:30] + b"X" + text[31:70], text[50:90], b"QQ"]
    qb, off = pack_queries(queries)
    want = f.approx_arrays(qb, off, 2, both_strands=True)
    n = len(want[0])
    assert n >= 2
    C = sufr_amd._lib.C
    L = sufr_amd.lib()
    for cap in (0, 1, n - 1):
        with pytest.raises(SufrHipError) as e:
            f.approx_arrays(qb, off, 2, both_strands=True, cap=cap)
        assert e.value.code == -5 and e.value.total == n
        # the outputs of a call that does not fit stay as they were
        out = [np.full(n, 0xAB, dtype=dt) for dt in (np.uint64, np.uint8, np.uint64, np.uint8)]
        total = C.c_uint64(0)
        rc = L.sufr_file_approx(f._h, qb.ctypes.data, off.ctypes.data, len(queries), 2, 0, 1, cap, *[a.ctypes.data for a in out],
                                C.byref(total), 1)
        assert rc == -5 and total.value == n and all((a == 0xAB).all() for a in out)
    got = f.approx_arrays(qb, off, 2, both_strands=True, cap=n)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    with pytest.raises(SufrHipError) as e:
        f.approx([b"ACGT"], 16)
    assert e.value.code == -1
    assert len(f.approx([text[:40]], 15)[0]) >= 1
    assert f.approx([], 2) == [] and f.approx([b""], 0) == [[]] and f.approx([b"", b"AC"], 2, both_strands=True) == [[], []]
    total = C.c_uint64(7)
    z = np.zeros(1, dtype=np.uint64)
    assert L.sufr_file_approx(f._h, None, z.ctypes.data, 0, 2, 0, 1, 0, None, None, None, None, C.byref(total), 1) == 0
    assert total.value == 0


def test_seed_mask_is_refused():
    f = SufrFile(EXP / "uniprot-masked.sufr")
    qb, off = pack_queries([b"RNELNNEEA"])
    with pytest.raises(SufrHipError) as e:
        f.approx_arrays(qb, off, 1)
    assert e.value.code == -6


def test_unindexed_anchors_lose_the_window(oracle, tmp_path):
    # GGGTTNACGTCCC, --dna: the N at 5 starts no indexed suffix.  NACG with d = 1: pieces NA | CG; NA would anchor window 5
    # but starts unindexed, CG anchors it instead.  TNAC: pieces TN | AC, window 4: TN is indexed at 4.  NAAG (one
    # mismatch, in the second piece): only NA matches exactly, at an unindexed start: the window is lost.
    (tmp_path / "n.fa").write_bytes(b">s\nGGGTTNACGTCCC\n")
    oracle.create(tmp_path / "n.fa", tmp_path / "n.sufr", is_dna=True)
    f = SufrFile(tmp_path / "n.sufr")
    assert 5 not in set(np.asarray(f.suffix_array).tolist())
    rec = lambda q, d: [(h.position, h.mismatches) for h in f.approx([q], d)[0]]
    assert rec(b"NACG", 1) == [(5, 0)] and rec(b"TNAC", 1) == [(4, 0)] and rec(b"NAAG", 1) == [] and rec(b"NACG", 0) == []
    oracle.create(tmp_path / "n.fa", tmp_path / "p.sufr", is_dna=False)          # every position indexed: nothing is lost
    g = SufrFile(tmp_path / "p.sufr")
    assert [(h.position, h.mismatches) for h in g.approx([b"NAAG"], 1)[0]] == [(5, 1)]


def test_suffix_array_facade():
    sa = SuffixArray.read(str(SUFR1))                             # ACGTNNACGT$, --dna
    h = sa.approx(["ACGA"], max_mismatches=1, both_strands=True)
    assert [(x.query, x.strand, x.position, x.mismatches) for x in h[0]] == [(0, 0, 6, 1), (0, 0, 0, 1), (0, 1, 6, 1), (0, 1, 0, 1)]


# ---------------------------------------------------------------------------------------------------------------------
# sufr approx
# ---------------------------------------------------------------------------------------------------------------------
def _lines(f: SufrFile, names, hits, absolute):
    out = []
    for name, hs in zip(names, hits):
        for h in hs:
            if absolute:
                where = str(h.position)
            else:
                k = f._sequence_of(h.position)
                where = f"{f.sequence_names[k]}:{h.position - f.sequence_starts[k]}"
            out.append(f"{name}\t{'-' if h.strand else '+'}\t{where}\t{h.mismatches}\n")
    return "".join(out)


def test_cli_prints_the_python_records(tmp_path):
    path = EXP / "long_dna_sequence.sufr"
    f = SufrFile(path)
    reads = [r for r in planted(np.random.default_rng(3), f, 60, 120, extra=b"N") if r and not set(r) & set(b"$%")]
    fa = tmp_path / "r.fa"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    names = [f"r{i}" for i in range(len(reads))]
    for opts, kw in (([], dict(max_mismatches=2)), (["-d", 4, "-b"], dict(max_mismatches=4, both_strands=True)),
                     (["-d", 1, "--max-occ", 2, "-b"], dict(max_mismatches=1, max_occ=2, both_strands=True))):
        hits = f.approx(reads, **kw)
        assert sum(map(len, hits)) > 0
        assert run("approx", *opts, "-q", fa, path).stdout == _lines(f, names, hits, False)
        assert run("ap", *opts, "-a", "-q", fa, path).stdout == _lines(f, names, hits, True)
    out = tmp_path / "o.tsv"
    run("approx", "-d", 1, "-b", "-o", out, SUFR1, "ACGA")
    assert out.read_text() == "ACGA\t+\t1:6\t1\nACGA\t+\t1:0\t1\nACGA\t-\t1:6\t1\nACGA\t-\t1:0\t1\n"


def test_cli_errors():
    r = run("approx", EXP / "uniprot-masked.sufr", "RNELNNEEA", check=False)
    assert r.returncode == 1 and r.stderr.startswith("Error: ") and "seed mask" in r.stderr
    r = run("approx", "-d", 16, SUFR1, "ACGT", check=False)
    assert r.returncode == 1 and r.stderr.startswith("Error: ")
    assert run("approx", SUFR1, check=False).returncode == 2
    assert run("approx", "-k", 3, SUFR1, "ACGT", check=False).returncode == 2     # -k is match's and mems'
    assert "approx|ap" in run("--help").stdout
