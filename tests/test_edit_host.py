"""k-difference search on the host (include/sufr_edit.h): no GPU.

The witness depends on neither implementation: numpy over the file's own text and SA.  D(.) is the last row of the full
Sellers table, one vectorised row per query byte (no band); coverage comes from the occurrences of every seed at indexed
positions; the minima rule is applied to D itself, over all ends, with the ends that are no record set to d + 1.
"""
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

import sufr_amd
from sufr_amd import SufrFile, SuffixArray, SufrHipError, pack_queries, synth
from oracle_helper import GOLDEN
from test_match_host import run
from test_mem_host import ADVERSARIAL, BUILDS, _adversarial_body, _fasta_from, revcomp
from test_approx_host import occurrences, planted, stack

EXP = GOLDEN / "expected"
SUFR1 = EXP / "1.sufr"
DS = (0, 1, 2, 4)
COMBOS = [(d, occ, both, minima) for d in DS for occ in (0, 2) for both in (False, True) for minima in (False, True)]


# ---------------------------------------------------------------------------------------------------------------------
# the witness
# ---------------------------------------------------------------------------------------------------------------------
def sellers(text: np.ndarray, q: bytes) -> np.ndarray:
    """D[e], e = 0 .. n: the least edit distance between q and a piece of the text that ends before e."""
    n = text.size
    j = np.arange(n + 1, dtype=np.int64)
    row = np.zeros(n + 1, dtype=np.int64)
    for r, c in enumerate(q, 1):
        cur = np.empty(n + 1, dtype=np.int64)
        cur[0] = r
        cur[1:] = np.minimum(row[:-1] + (text != c), row[1:] + 1)
        row = np.minimum.accumulate(cur - j) + j                   # the left neighbour: min over j' <= j of cur[j'] + j - j'
    return row


def witness_one(text, indexed, L, q: bytes, ds, occs):
    """{(d, occ, minima): [(end, edits)] by end} of one query on one strand."""
    n, m = text.size, len(q)
    out = {(d, occ, mi): [] for d in ds for occ in occs for mi in (False, True)}
    if m == 0:
        return out
    D = sellers(text, q)
    for d in ds:
        if m < d + 1:
            continue
        o = [i * m // (d + 1) for i in range(d + 2)]
        seeds = [q[o[i]:o[i] + (min(o[i + 1] - o[i], L) if L else o[i + 1] - o[i])] for i in range(d + 1)]
        starts = [np.nonzero(occurrences(text, s) & indexed)[0] for s in seeds]
        for occ in occs:
            delta = np.zeros(n + 3, dtype=np.int64)
            for i in range(d + 1):
                if occ and starts[i].size > occ:
                    continue
                centre = starts[i] - o[i] + m
                np.add.at(delta, np.clip(centre - d, 0, n + 1), 1)
                np.add.at(delta, np.clip(centre + d + 1, 0, n + 1), -1)
            covered = np.cumsum(delta)[:n + 1] > 0
            rec = covered & (D <= d)
            val = np.full(n + 3, d + 1, dtype=np.int64)             # val[e + 1]: D(e) of a record, d + 1 of anything else
            val[1:n + 2][rec] = D[rec]
            keep = rec & (val[0:n + 1] > val[1:n + 2]) & (val[2:n + 3] >= val[1:n + 2])
            for mi, mask in ((False, rec), (True, keep)):
                e = np.nonzero(mask)[0]
                assert not e.size or e[0] >= 1
                out[(d, occ, mi)] = [(int(x) - 1, int(D[x])) for x in e]
    return out


def witness(f: SufrFile, queries, combos):
    """{(d, occ, both, minima): (query, strand, end, edits) rows in record order}."""
    text = np.asarray(f.text)
    indexed = np.zeros(text.size, dtype=bool)
    indexed[np.asarray(f.suffix_array).astype(np.int64)] = True
    ds = sorted({c[0] for c in combos})
    occs = sorted({c[1] for c in combos})
    recs = {c: [] for c in combos}
    for qi, q in enumerate(queries):
        strands = 2 if any(c[2] for c in combos) else 1
        per = [witness_one(text, indexed, f.max_query_len, qq, ds, occs) for qq in (bytes(q), revcomp(q))[:strands]]
        for (d, occ, both, mi) in combos:
            for strand in range(2 if both else 1):
                recs[(d, occ, both, mi)].extend((qi, strand, e, v) for e, v in per[strand][(d, occ, mi)])
    return {c: np.array(v, dtype=np.int64).reshape(-1, 4) for c, v in recs.items()}


def check_file(f: SufrFile, queries, combos=COMBOS, threads=0, nonzero=True):
    """Host == witness for every combination; the sum of the record totals, every one of which is above 0."""
    want = witness(f, queries, combos)
    qb, off = pack_queries(queries)
    n = 0
    for c in combos:
        d, occ, both, mi = c
        got = stack(f.edit_arrays(qb, off, d, occ, both, mi, threads=threads))
        assert np.array_equal(got, want[c]), (c, len(got), len(want[c]), got[:10], want[c][:10])
        # (a build that caps the seeds at L bytes may leave none of them alive under max_occ 2: -m 3 on 1 200 bytes)
        assert len(got) > 0 or not nonzero or (occ and f.max_query_len), c
        n += len(got)
    return n


def with_indels(rng, f: SufrFile, count, max_len, extra=b"$%XN"):
    """Slices of the text with 0..4 edits each, drawn from substitutions, insertions and deletions (bytes of the text and of
    `extra`), on top of `planted` (random queries, substituted slices, the short and odd ones)."""
    text = bytes(f.text)
    alphabet = sorted(set(text) | set(extra))
    qs = planted(rng, f, count, max_len, extra=extra)
    for _ in range(count):
        m = int(rng.integers(2, max_len + 1))
        at = int(rng.integers(0, max(len(text) - m, 1)))
        q = bytearray(text[at:at + m])
        for _ in range(int(rng.integers(0, 5))):
            kind, where = int(rng.integers(0, 3)), int(rng.integers(0, max(len(q), 1)))
            sym = alphabet[int(rng.integers(0, len(alphabet)))]
            if kind == 0 and q:
                q[where] = sym
            elif kind == 1:
                q.insert(where, sym)
            elif len(q) > 1:
                del q[where]
        qs.append(bytes(q))
    return qs


def test_witness_on_a_hand_checked_text():
    # ACGTACGA, query ACGA.  D(8) = 0 (ACGA at 4), D(7) = 1 (ACG), D(4) = 1 (ACGT), D(3) = 1 (ACG), D(5) = 1 (ACGTA, one
    # insertion), D(6) = D(2) = 2.  d = 1: pieces AC | GA; AC at 0 and 4 covers the ends 3..5 and 7..8, GA at 6 covers 7..8.
    # Minima: 3 (its left neighbour 2 is no record: 2 > 1; its right one ties) and 8; 4 and 5 tie with their left neighbour,
    # 7 has the smaller 8 to its right.
    text = np.frombuffer(b"ACGTACGA", dtype=np.uint8)
    assert sellers(text, b"ACGA").tolist() == [4, 3, 2, 1, 1, 1, 2, 1, 0]
    got = witness_one(text, np.ones(8, dtype=bool), 0, b"ACGA", (0, 1), (0, 1))
    assert got[(1, 0, False)] == [(2, 1), (3, 1), (4, 1), (6, 1), (7, 0)]
    assert got[(1, 0, True)] == [(2, 1), (7, 0)]
    assert got[(1, 1, False)] == [(6, 1), (7, 0)]                  # AC starts two suffixes: dead; GA covers 7..8
    assert got[(1, 1, True)] == [(7, 0)]                           # (6 is no record's right neighbour now, but 8 still beats 7)
    assert got[(0, 0, False)] == got[(0, 0, True)] == got[(0, 1, False)] == [(7, 0)]
    # the first position left out of the array: AC at 0 is gone, so are the ends only it covers
    indexed = np.ones(8, dtype=bool)
    indexed[0] = False
    assert witness_one(text, indexed, 0, b"ACGA", (1,), (0,))[(1, 0, False)] == [(6, 1), (7, 0)]


# ---------------------------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_edit_header_symbols_are_exported():
    hdr = (sufr_amd.LIB_PATH.parents[3] / "include" / "sufr_edit.h").read_text()
    assert "#define SUFR_EDIT_BOTH_STRANDS 0x1u" in hdr and "#define SUFR_EDIT_LOCAL_MINIMA 0x2u" in hdr
    assert "#define SUFR_EDIT_MAX_EDITS 15u" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(sufr_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(sufr_amd.EDIT_EXPORTS), declared ^ set(sufr_amd.EDIT_EXPORTS)
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
    queries = with_indels(rng, f, 10 if big else 40, 60 if big else 16)
    if f.seed_mask:
        with pytest.raises(SufrHipError) as e:
            f.edit(queries, 2)
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
    # (the text's last bytes: a seed that holds the sentinel starts one suffix, so max_occ 2 leaves records on a run of As)
    queries = with_indels(rng, f, 10, 40) + [b"A" * 40, b"NACGTACGT", bytes(f.text)[-12:]]
    assert check_file(f, queries) > 0


def test_host_equals_witness_on_a_protein_build(oracle, tmp_path):
    rng = np.random.default_rng(8)
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    body = aa[rng.integers(0, 20, 1500)].copy()
    body[700:760] = body[100:160]                                  # a repeat, so that ends are reported by several seeds
    body[[400, 900]] = ord("%")
    _fasta_from(body, tmp_path / "p.fa")
    oracle.create(tmp_path / "p.fa", tmp_path / "p.sufr", is_dna=False)
    f = SufrFile(tmp_path / "p.sufr")
    assert check_file(f, with_indels(rng, f, 30, 50)) > 0


@pytest.mark.parametrize("L", [3, 6, 11])
def test_capped_build_gives_the_plain_records(oracle, tmp_path, L):
    body = synth.adversarial("tandem", 2000, seed=9)[:-1]
    _fasta_from(body, tmp_path / "x.fa")
    oracle.create(tmp_path / "x.fa", tmp_path / "plain.sufr", is_dna=True)
    oracle.create(tmp_path / "x.fa", tmp_path / "cap.sufr", is_dna=True, max_query_len=L)
    p, c = SufrFile(tmp_path / "plain.sufr"), SufrFile(tmp_path / "cap.sufr")
    qb, off = pack_queries(with_indels(np.random.default_rng(L), p, 40, 60))
    for d in DS:
        for both in (False, True):
            for mi in (False, True):
                a = stack(p.edit_arrays(qb, off, d, 0, both, mi))
                b = stack(c.edit_arrays(qb, off, d, 0, both, mi))
                assert np.array_equal(a, b), (d, both, mi)         # the records are sorted: the order is equal too
                assert len(a) > 0
    # the capped file against the witness as well, occurrence filter included (its seeds are the capped ones)
    rng = np.random.default_rng(L + 100)
    assert check_file(c, with_indels(rng, c, 10, 40), nonzero=False) > 0     # (max_occ 2 leaves no 3-byte seed alive)


@pytest.mark.parametrize("name", ["3.sufr", "long_dna_sequence.sufr", "uniprot.sufr"])
def test_no_edit_is_locate_by_the_last_byte(name):
    f = SufrFile(EXP / name)
    queries = [q for q in with_indels(np.random.default_rng(11), f, 30, 40) if 0 < len(q) <= f.text_len]
    n = 0
    hits = f.edit(queries, 0)
    for q, hs, loc in zip(queries, hits, f.locate(queries)):
        assert [h.end for h in hs] == sorted(p.suffix + len(q) - 1 for p in loc.positions), q
        assert all(h.edits == 0 and h.strand == 0 for h in hs)
        n += len(hs)
    assert n > 0
    # the minima rule at d = 0: of a run of adjacent ends (all 0) the first stays
    for hs, ms in zip(hits, f.edit(queries, 0, local_minima=True)):
        ends = [h.end for h in hs]
        assert [h.end for h in ms] == [e for e in ends if e - 1 not in set(ends)]


@pytest.mark.parametrize("name", ["long_dna_sequence.sufr", "uniprot.sufr", "2.sufr"])
def test_every_approx_record_is_an_edit_record(name):
    """Both calls cut the same pieces, search the same seeds and call the same ones live, and a window within h
    substitutions ends at p + m with D <= h, on the window's own diagonal: (q, s, p, h) implies (q, s, p + m - 1, <= h), on any
    index and for any max_occ."""
    f = SufrFile(EXP / name)
    queries = with_indels(np.random.default_rng(5), f, 40, 60)
    qb, off = pack_queries(queries)
    lens = np.diff(off.astype(np.int64))
    n = 0
    for d in DS:
        for occ in (0, 2):
            for both in (False, True):
                a = stack(f.approx_arrays(qb, off, d, occ, both))
                e = stack(f.edit_arrays(qb, off, d, occ, both))
                have = {(int(q), int(s), int(x)): int(v) for q, s, x, v in e}
                for q, s, p, h in a:
                    key = (int(q), int(s), int(p + lens[q] - 1))
                    assert key in have and have[key] <= h, (d, occ, both, q, s, p, h)
                n += len(a)
    assert n > 0


@pytest.mark.parametrize("threads", [3, 16])
def test_threads_do_not_change_the_answer(threads):
    f = SufrFile(EXP / "long_dna_sequence.sufr")
    qb, off = pack_queries(with_indels(np.random.default_rng(4), f, 300, 150))
    for mi in (False, True):
        want = f.edit_arrays(qb, off, 3, 0, True, mi, threads=1)
        got = f.edit_arrays(qb, off, 3, 0, True, mi, threads=threads)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)) and len(want[0]) > 0


# ---------------------------------------------------------------------------------------------------------------------
# edge cases
# ---------------------------------------------------------------------------------------------------------------------
def test_limits_capacity_and_empty_batches():
    f = SufrFile(EXP / "3.sufr")
    text = bytes(f.text)
    queries = [text[0:30] + b"X" + text[31:50] + text[52:70], text[50:90], b"QQ"]
    qb, off = pack_queries(queries)
    want = f.edit_arrays(qb, off, 2, both_strands=True)
    n = len(want[0])
    assert n >= 2
    C = sufr_amd._lib.C
    L = sufr_amd.lib()
    for cap in (0, 1, n - 1):
        with pytest.raises(SufrHipError) as e:
            f.edit_arrays(qb, off, 2, both_strands=True, cap=cap)
        assert e.value.code == -5 and e.value.total == n
        # the outputs of a call that does not fit stay as they were
        out = [np.full(n, 0xAB, dtype=dt) for dt in (np.uint64, np.uint8, np.uint64, np.uint8)]
        total = C.c_uint64(0)
        rc = L.sufr_file_edit(f._h, qb.ctypes.data, off.ctypes.data, len(queries), 2, 0, 1, cap, *[a.ctypes.data for a in out],
                              C.byref(total), 1)
        assert rc == -5 and total.value == n and all((a == 0xAB).all() for a in out)
    got = f.edit_arrays(qb, off, 2, both_strands=True, cap=n)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    with pytest.raises(SufrHipError) as e:
        f.edit([b"ACGT"], 16)
    assert e.value.code == -1
    assert len(f.edit([text[:40]], 15)[0]) >= 1
    assert f.edit([], 2) == [] and f.edit([b""], 0) == [[]] and f.edit([b"", b"AC"], 2, both_strands=True) == [[], []]
    assert f.edit([text[:3]], 3) == [[]] and f.edit([text[:4]], 3) != [[]]      # m < d + 1: no records
    total = C.c_uint64(7)
    z = np.zeros(1, dtype=np.uint64)
    assert L.sufr_file_edit(f._h, None, z.ctypes.data, 0, 2, 0, 1, 0, None, None, None, None, C.byref(total), 1) == 0
    assert total.value == 0


def test_host_path_under_the_sanitizers():
    """The golden-file, capacity and threads tests of this file against the host-only AddressSanitizer + UBSan build
    (tests/test_sanitized_host.py has the scheme): the band's rows, the per-query vectors, the chunked workers."""
    from test_sanitized_host import ROOT, _asan_env, _clean
    env = _asan_env()
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_edit_host.py", "-q", "-p", "no:cacheprovider", "-k",
                        "golden_files or limits_capacity or threads_do_not or seed_mask"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1800)
    _clean(r.stdout + r.stderr)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]


def test_seed_mask_is_refused():
    f = SufrFile(EXP / "uniprot-masked.sufr")
    qb, off = pack_queries([b"RNELNNEEA"])
    with pytest.raises(SufrHipError) as e:
        f.edit_arrays(qb, off, 1)
    assert e.value.code == -6


def test_unindexed_anchors_lose_the_end(oracle, tmp_path):
    # GGGTTNACGTCCC, --dna: the N at 5 starts no indexed suffix.  NACG with d = 1: pieces NA | CG; NA starts unindexed, CG
    # (at 7, diagonal 5) covers the ends 8..10: D = 1 (NAC), 0, 1 (NACGT).  NAAG (one substitution, in the second piece):
    # only NA matches exactly, at an unindexed start: its end is lost.
    (tmp_path / "n.fa").write_bytes(b">s\nGGGTTNACGTCCC\n")
    oracle.create(tmp_path / "n.fa", tmp_path / "n.sufr", is_dna=True)
    f = SufrFile(tmp_path / "n.sufr")
    assert 5 not in set(np.asarray(f.suffix_array).tolist())
    rec = lambda g, q, d, mi=False: [(h.end, h.edits) for h in g.edit([q], d, local_minima=mi)[0]]
    assert rec(f, b"NACG", 1) == [(7, 1), (8, 0), (9, 1)] and rec(f, b"NACG", 1, True) == [(8, 0)]
    assert rec(f, b"NAAG", 1) == [] and rec(f, b"NACG", 0) == []
    oracle.create(tmp_path / "n.fa", tmp_path / "p.sufr", is_dna=False)          # every position indexed: nothing is lost
    g = SufrFile(tmp_path / "p.sufr")
    assert rec(g, b"NAAG", 1) == [(8, 1)] and rec(g, b"NACG", 0) == [(8, 0)]


def test_suffix_array_facade():
    sa = SuffixArray.read(str(SUFR1))                             # ACGTNNACGT$, --dna
    h = sa.edit(["ACGA"], max_edits=1, both_strands=True, local_minima=True)
    f = SufrFile(SUFR1)
    want = witness(f, [b"ACGA"], [(1, 0, True, True)])[(1, 0, True, True)]
    assert [[x.query, x.strand, x.end, x.edits] for x in h[0]] == want.tolist() and len(want) >= 2


# ---------------------------------------------------------------------------------------------------------------------
# sufr edit
# ---------------------------------------------------------------------------------------------------------------------
def _lines(f: SufrFile, names, hits, absolute):
    out = []
    for name, hs in zip(names, hits):
        for h in hs:
            if absolute:
                where = str(h.end)
            else:
                k = f._sequence_of(h.end)
                where = f"{f.sequence_names[k]}:{h.end - f.sequence_starts[k]}"
            out.append(f"{name}\t{'-' if h.strand else '+'}\t{where}\t{h.edits}\n")
    return "".join(out)


def test_cli_prints_the_python_records(tmp_path):
    path = EXP / "long_dna_sequence.sufr"
    f = SufrFile(path)
    reads = [r for r in with_indels(np.random.default_rng(3), f, 60, 120, extra=b"N") if r and not set(r) & set(b"$%")]
    fa = tmp_path / "r.fa"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    names = [f"r{i}" for i in range(len(reads))]
    for opts, kw in (([], dict(max_edits=2)), (["-d", 4, "-b", "-l"], dict(max_edits=4, both_strands=True, local_minima=True)),
                     (["--edits", 3, "--local-minima"], dict(max_edits=3, local_minima=True)),
                     (["-d", 1, "--max-occ", 2, "-b"], dict(max_edits=1, max_occ=2, both_strands=True))):
        hits = f.edit(reads, **kw)
        assert sum(map(len, hits)) > 0
        assert run("edit", *opts, "-q", fa, path).stdout == _lines(f, names, hits, False)
        assert run("ed", *opts, "-a", "-q", fa, path).stdout == _lines(f, names, hits, True)
    out = tmp_path / "o.tsv"
    run("edit", "-d", 1, "-l", "-o", out, SUFR1, "ACGA")
    g = SufrFile(SUFR1)
    assert out.read_text() == _lines(g, ["ACGA"], g.edit([b"ACGA"], 1, local_minima=True), False) != ""


def test_cli_errors():
    r = run("edit", EXP / "uniprot-masked.sufr", "RNELNNEEA", check=False)
    assert r.returncode == 1 and r.stderr.startswith("Error: ") and "seed mask" in r.stderr
    r = run("edit", "-d", 16, SUFR1, "ACGT", check=False)
    assert r.returncode == 1 and r.stderr.startswith("Error: ")
    assert run("edit", SUFR1, check=False).returncode == 2
    assert run("edit", "-k", 3, SUFR1, "ACGT", check=False).returncode == 2       # -k is match's and mems'
    assert run("edit", "--mismatches", 1, SUFR1, "ACGT", check=False).returncode == 2   # approx's name for -d
    assert run("approx", "--local-minima", SUFR1, "ACGT", check=False).returncode == 2
    assert "edit|ed" in run("--help").stdout
