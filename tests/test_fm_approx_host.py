"""k-mismatch search on the FM-index by backtracking, on the host (include/sufr_fm.h and sufr_fm_approx.h, sufr_query.cpp; DESIGN.md
section 24), against two witnesses: the Hamming distance of every window of the text in numpy, and a recursive transcription of the
definition over the Witness of tests/test_fm_host.py, which gives the leaves in order.  Every comparison is exact equality: of the
arrays with the transcription, of the record sets with the brute force and with SufrFile.approx(max_occ=0).  The query sets and their
conditions are built here and used by tests/test_fm_approx_gpu.py too."""
import ctypes as C
import functools
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sufr_amd
from sufr_amd import SufrFile, SufrHipError, pack_queries
from oracle_helper import GOLDEN
from test_bwt_host import LF_FILES, write_arrays
from test_fm_host import Witness, sorted_sa
from test_match_host import run

ROOT = Path(__file__).resolve().parent.parent
EXP = GOLDEN / "expected"
SMALLEST = "1n.sufr"
INVALID, CAPACITY, UNSUPPORTED = -1, -5, -6
DTYPES = (np.uint64, np.uint8, np.uint64, np.uint8)                  # query, strand, position, mismatches


def max_d(name: str) -> int:
    return 2 if name == "uniprot.sufr" else 3                        # (the wide shape: 22 substitutions a place)


CASES = [(name, d) for name in LF_FILES for d in range(max_d(name) + 1)]


# ---------------------------------------------------------------------------------------------------------------------
# the two witnesses
# ---------------------------------------------------------------------------------------------------------------------
def revcomp(q: bytes) -> bytes:
    return q[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def brute_force(w: Witness, q: bytes, d: int):
    """witness (a): {(position, mismatches)} of every window of the text within d substitutions of q; none for the empty query"""
    m, n = len(q), w.n
    if m == 0 or m > n:
        return set()
    dist = np.zeros(n - m + 1, dtype=np.int64)
    for j in range(m):
        dist += w.text[j:n - m + 1 + j] != q[j]
    at = np.nonzero(dist <= d)[0]
    return set(zip(at.tolist(), dist[at].tolist()))


def occ_lists(w: Witness):
    """occ(c, r) for every r in [0, s] as plain lists, from the witness's BWT (the recursion below asks many times)"""
    if not hasattr(w, "_occ_lists"):
        w._occ_lists = {int(c): np.concatenate([[0], np.cumsum(w.bwt == c)]).tolist() for c in np.nonzero(w.counts)[0]}
        w._C = [int(x) for x in w.C]
    return w._occ_lists, w._C


def leaves_of(w: Witness, q: bytes, d: int):
    """witness (b): the definition of include/sufr_fm.h transcribed -- the leaves (lo, hi, h) of one query in order"""
    occ, Cs = occ_lists(w)
    m, out, syms = len(q), [], sorted(occ)

    def ok(c, t):
        return c in occ and (c != w.e or t == m - 1)

    def expand(t, lo, hi, h):
        if lo >= hi:
            return
        if t < 0:
            out.append((lo, hi, h))
            return
        if h < d:
            for c in syms:
                if c != q[t] and ok(c, t):
                    expand(t - 1, Cs[c] + occ[c][lo], Cs[c] + occ[c][hi], h + 1)
        if ok(q[t], t):
            expand(t - 1, Cs[q[t]] + occ[q[t]][lo], Cs[q[t]] + occ[q[t]][hi], h)

    if m:
        expand(m - 1, 0, w.s, 0)
    return out


def items_of(qs, both: bool):
    """(query, strand, bytes) in record order"""
    return [(i, st, revcomp(q) if st else q) for i, q in enumerate(qs) for st in ((0, 1) if both else (0,))]


def want_records(w: Witness, qs, d: int, both: bool):
    """the four arrays from witness (b): (query, strand, leaf, rank) order"""
    cols = [[], [], [], []]
    for i, st, q in items_of(qs, both):
        for lo, hi, h in leaves_of(w, q, d):
            cols[0] += [i] * (hi - lo)
            cols[1] += [st] * (hi - lo)
            cols[2] += w.sa[lo:hi].tolist()
            cols[3] += [h] * (hi - lo)
    return tuple(np.array(c, dtype=t) for c, t in zip(cols, DTYPES))


def record_set(recs):
    return set(zip(*[np.asarray(c).astype(np.int64).tolist() for c in recs]))


def brute_set(w: Witness, qs, d: int, both: bool):
    return {(i, st, p, h) for i, st, q in items_of(qs, both) for p, h in brute_force(w, q, d)}


# ---------------------------------------------------------------------------------------------------------------------
# the query sets and their conditions
# ---------------------------------------------------------------------------------------------------------------------
def planted(rng, w: Witness, raw: bytes, a: int, m: int, places):
    """raw[a:a + m] with another occurring byte (not the end byte) at every one of `places`"""
    q = bytearray(raw[a:a + m])
    pool = [int(c) for c in np.nonzero(w.counts)[0] if c != w.e]
    for t in places:
        if t < len(q):
            q[t] = int(rng.choice([c for c in pool if c != q[t]] or pool))
    return bytes(q)


def query_set(w: Witness, d: int, seed: int = 0, per_length: int = 2, long_query: bool = True):
    """Pieces of the text with 0 .. d planted substitutions -- among them one at place 0, one at place m - 1, two at adjacent
    places --, the window that ends at n with another byte for the end byte, the end byte at an inner place, a byte that does
    not occur, d + 1 of them (no record), queries of 1 .. d bytes, the empty query, short queries (wide leaves) and, at d == 3,
    one of 300 bytes"""
    rng = np.random.default_rng(seed + 17 * d)
    raw, n = w.text.tobytes(), w.n
    absent = [c for c in range(255, -1, -1) if w.counts[c] == 0]
    qs = [b""]
    if n <= 64:                                                      # (where every window is a record that stays a short list)
        qs += [raw[int(rng.integers(0, n - m + 1)):][:m] for m in range(1, d + 1)]
    lengths = [m for m in (d + 2, 8, 12, 20, 31, 50) if d + 2 <= m <= n - 1]
    for m in lengths:
        for _ in range(per_length):
            for h in range(d + 1):
                a = int(rng.integers(0, n - m))
                qs.append(planted(rng, w, raw, a, m, rng.choice(m, h, replace=False).tolist()))
    m = lengths[-1] if len(lengths) < 3 else lengths[2]
    a = int(rng.integers(0, n - m))
    if d:
        qs += [planted(rng, w, raw, a, m, [0]), planted(rng, w, raw, a, m, [m - 1]), planted(rng, w, raw, n - m, m, [m - 1])]
        qs.append(raw[-3:] + raw[:max(m - 3, 1)])                    # the end byte at an inner place
    if d >= 2:
        qs.append(planted(rng, w, raw, a, m, [m // 2, m // 2 + 1]))
    if absent:
        qs.append(raw[a:a + m // 2] + bytes([absent[0]]) + raw[a + m // 2 + 1:a + m])
        qs.append(bytes([absent[0]]) * (d + 1) + raw[a:a + m])
        qs.append(raw[a:a + m] + bytes([absent[-1]]) * (d + 1))
    if d == 3 and long_query and n > 400:
        a = int(rng.integers(0, n - 300))
        qs.append(planted(rng, w, raw, a, 300, [1, 150, 298]))
    return qs


def conditions(w: Witness, qs, d: int, B: int):
    """what a query set does, from the two witnesses (one strand)"""
    c = dict(with_records=0, without=0, by_h=set(), wide_leaf=False, two_blocks=False, at_0=False, at_last=False, adjacent=False,
             end_window=False, inner_e=False, absent=False, empty=False, short=set(), long=False)
    raw, n = w.text.tobytes(), w.n
    for q in qs:
        m = len(q)
        leaves = leaves_of(w, q, d)
        c["with_records"] += bool(leaves)
        c["without"] += not leaves
        c["by_h"] |= {h for _, _, h in leaves}
        c["wide_leaf"] |= any(hi - lo >= 2 for lo, hi, _ in leaves)
        c["two_blocks"] |= any(lo // B != hi // B for lo, hi, _ in leaves)
        c["empty"] |= m == 0
        c["inner_e"] |= w.e in q[:-1]
        c["absent"] |= any(w.counts[b] == 0 for b in q)
        c["long"] |= m >= 300 and bool(leaves)
        if 1 <= m <= d and len(brute_force(w, q, d)) == n - m + 1:
            c["short"].add(m)
        for p, h in brute_force(w, q, d):                            # which places differ in the windows that are records
            diff = [t for t in range(m) if raw[p + t] != q[t]]
            c["at_0"] |= 0 in diff
            c["at_last"] |= m - 1 in diff
            c["adjacent"] |= any(t + 1 in diff for t in diff)
            c["end_window"] |= p == n - m and m - 1 in diff
    return c


def check_conditions(name: str, w: Witness, qs, d: int, B: int):
    c = conditions(w, qs, d, B)
    assert 3 * c["with_records"] >= len(qs) and c["without"] >= 1 and c["empty"], (name, d, c)
    assert c["by_h"] == set(range(d + 1)), (name, d, c)
    assert c["wide_leaf"], (name, d, c)
    if w.s > 20 * B:
        assert c["two_blocks"], (name, d, c)
    if d:
        assert c["at_0"] and c["at_last"] and c["end_window"] and c["inner_e"], (name, d, c)
    if d >= 2:
        assert c["adjacent"], (name, d, c)
    assert c["absent"] or (w.counts > 0).all(), (name, d, c)
    if name == SMALLEST:
        assert c["short"] == set(range(1, d + 1)), (name, d, c)
    if d == 3 and w.n > 400:
        assert c["long"], (name, d, c)
    return c


@functools.lru_cache(maxsize=None)
def case(name: str, d: int):
    """(file, witness, queries, the records of witness (b) with one strand and with both): computed once, never changed"""
    f = SufrFile(EXP / name)
    w = Witness(np.asarray(f.text), np.asarray(f.suffix_array))
    qs = query_set(w, d)
    return f, w, qs, {both: want_records(w, qs, d, both) for both in (False, True)}


def same_arrays(got, want):
    return all(g.dtype == x.dtype and np.array_equal(g, x) for g, x in zip(got, want))


# ---------------------------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_header_symbols_are_exported_and_stubbed():
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "sufr_fm_approx.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(sufr_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(sufr_amd.FM_APPROX_EXPORTS), declared ^ set(sufr_amd.FM_APPROX_EXPORTS)
    L = sufr_amd.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(sufr_amd.LIB_PATH)], capture_output=True, text=True).stdout
    for name in declared:
        assert hasattr(L, name) and re.search(rf"\bT {name}\b", nm), name
    stubs = (ROOT / "sufr_amd" / "csrc" / "sufr_host_stubs.cpp").read_text()
    device = [name for name in sufr_amd.FM_APPROX_EXPORTS if name.startswith("sufr_hip_")]
    assert len(device) == 2
    for name in device:
        assert re.search(rf"\bint {name}\(", stubs), name
    for cls in (sufr_amd.FmIndex, sufr_amd.DeviceFmIndex):
        assert hasattr(cls, "approx")
    assert hasattr(sufr_amd.FmIndex, "approx_arrays") and hasattr(sufr_amd.DeviceFmIndex, "approx_device")


# ---------------------------------------------------------------------------------------------------------------------
# the witnesses agree, the query sets meet their conditions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,d", CASES)
def test_witnesses_agree_and_query_sets_meet_their_conditions(name, d):
    f, w, qs, want = case(name, d)
    check_conditions(name, w, qs, d, f.fm(1).info["block"])
    for both in (False, True):
        assert record_set(want[both]) == brute_set(w, qs, d, both), (name, d, both)
        assert len(want[both][0]) == len(record_set(want[both]))    # every alignment once


# ---------------------------------------------------------------------------------------------------------------------
# the host path
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,d", CASES)
def test_host_equals_the_witnesses_and_approx(name, d):
    f, w, qs, want = case(name, d)
    qb, off = pack_queries(qs)
    long_enough = [i for i, q in enumerate(qs) if len(q) >= d + 1]
    for both in (False, True):
        brute = brute_set(w, qs, d, both)
        sv = record_set(f.approx_arrays(qb, off, d, 0, both))       # seed and verify: complete for m >= d + 1
        for sample in (1, 7, 32):
            fm = f.fm(sample)
            for threads in (1, 3, 0):
                got = fm.approx_arrays(qb, off, d, both, threads=threads)
                assert same_arrays(got, want[both]), (name, d, both, sample, threads)
                assert record_set(got) == brute
                assert {r for r in record_set(got) if r[0] in long_enough} == sv, (name, d, both, sample, threads)
            fm.close()
    assert sv and {r[0] for r in sv} <= set(long_enough)


@pytest.mark.parametrize("name", LF_FILES)
def test_no_mismatch_is_locate(name):
    f, w, qs, want = case(name, 0)
    fm = f.fm(7)
    hits = fm.approx(qs, 0)
    pos = fm.locate(qs)
    for i, q in enumerate(qs):
        assert [h.position for h in hits[i]] == (pos[i].tolist() if q else []), (name, i)
        assert all(h.mismatches == 0 and h.strand == 0 and h.query == i for h in hits[i])


def test_all_byte_values(tmp_path):
    """K = 256: 1024 bytes of counts and 1024 of BWT in a stride of 2048 (32-bit positions); one substitution tries 255 bytes a place"""
    rng = np.random.default_rng(11)
    text = rng.integers(0, 255, 5000).astype(np.uint8)
    text[:255] = np.arange(255)
    text[-1] = 255                                                   # the end byte occurs once
    sa = sorted_sa(text)
    f = write_arrays(tmp_path / "bytes.sufr", text, sa)
    w = Witness(text, sa)
    fm = f.fm(32)
    assert (fm.info["symbols"], fm.info["block"], fm.info["stride"]) == (256, 1024, 2048)
    qs = query_set(w, 1, seed=3) + [text[100:101].tobytes(), text[300:302].tobytes()]      # (short: leaves of many ranks)
    assert (w.counts > 0).all()
    c = check_conditions("bytes", w, qs, 1, 1024)
    assert c["by_h"] == {0, 1}
    qb, off = pack_queries(qs)
    for both in (False, True):
        want = want_records(w, qs, 1, both)
        got = fm.approx_arrays(qb, off, 1, both)
        assert same_arrays(got, want) and record_set(got) == brute_set(w, qs, 1, both)


def test_steps_and_leaves_of_the_walk():
    """sufr_fm_approx_steps: the leaves are those of the witness; with d == 0 a query of m bytes that occurs takes m steps"""
    f, w, qs, _ = case("long_dna_sequence_allow_ambiguity.sufr", 2)
    fm = f.fm(32)
    leaves, steps = fm.approx_steps(qs, 2, both_strands=True)
    assert leaves.tolist() == [len(leaves_of(w, q, 2)) for _, _, q in items_of(qs, True)]
    leaves0, steps0 = fm.approx_steps(qs, 0)
    found = [i for i, q in enumerate(qs) if q and w.search(q)[1] > 0]
    assert found and all(steps0[i] == len(qs[i]) and leaves0[i] == 1 for i in found)
    assert (steps[::2] >= steps0).all() and steps0[0] == 0


# ---------------------------------------------------------------------------------------------------------------------
# refusals, capacity, call shapes
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_capacity_and_the_empty_batch():
    f, w, qs, want = case("long_dna_sequence_allow_ambiguity.sufr", 2)
    L = sufr_amd.lib()
    fm = f.fm(7)
    qb, off = pack_queries(qs)
    z = len(want[False][0])
    assert z > 50
    out = [np.full(z + 3, 0xAA, dtype=t) for t in DTYPES]
    total = C.c_uint64(0)
    ptrs = [a.ctypes.data for a in out]
    call = lambda h, d, cap: L.sufr_fm_approx(h, qb.ctypes.data, off.ctypes.data, len(qs), d, 0, cap, *ptrs, C.byref(total), 0)
    assert call(fm._h, 4, z) == INVALID and total.value == 0
    assert call(fm._h, 2, z - 1) == CAPACITY and total.value == z and all((a == 0xAA).all() for a in out)
    assert call(fm._h, 2, z) == 0 and total.value == z and same_arrays([a[:z] for a in out], want[False])
    assert all((a[z:] == 0xAA).all() for a in out)
    none = f.fm(0)
    assert call(none._h, 2, z) == UNSUPPORTED and total.value == 0
    with pytest.raises(SufrHipError) as err:
        none.approx([b"ACGT"], 1)
    assert err.value.code == UNSUPPORTED
    with pytest.raises(SufrHipError) as err:
        fm.approx([b"ACGT"], 4)
    assert err.value.code == INVALID
    with pytest.raises(SufrHipError) as err:
        fm.approx_arrays(qb, off, 2, cap=z - 1)
    assert err.value.code == CAPACITY and err.value.total == z
    assert L.sufr_fm_approx(fm._h, None, None, 0, 2, 0, 0, None, None, None, None, C.byref(total), 0) == 0 and total.value == 0
    assert fm.approx([], 2) == [] and fm.approx([b""], 3, both_strands=True) == [[]]
    assert all(a.size == 0 for a in fm.approx_arrays(*pack_queries([b"", b""]), 1))


def test_the_index_outlives_the_file(tmp_path):
    import shutil
    path = tmp_path / "copy.sufr"
    shutil.copy(EXP / "long_dna_sequence_allow_ambiguity.sufr", path)
    _, w, qs, want = case("long_dna_sequence_allow_ambiguity.sufr", 2)
    f = SufrFile(path)
    fm = f.fm(32, 2)
    f.close()
    assert f.closed
    path.write_bytes(b"")                                            # the file is gone: the index owns what it reads
    assert same_arrays(fm.approx_arrays(*pack_queries(qs), 2, True), want[True])


# ---------------------------------------------------------------------------------------------------------------------
# sufr fm --mismatches
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_prints_the_lines_of_approx(tmp_path):
    for name, reads, d in (("long_dna_sequence_allow_ambiguity.sufr", ["ACGTACGTAC", "GATTACAGATTACA", "NNNNNNNN", "TTTTTTTTTTTTTT", "ACGGT"], 2),
                           ("uniprot.sufr", ["MKVLA", "LLLLLL", "WWPQR", "XQZJ"], 1), ("2ns.sufr", ["ACGT", "GTNN", "ACGTN"], 3)):
        path = EXP / name
        for extra in ((), ("-b",), ("-a", "-b")):
            want = run("approx", "-d", d, *extra, path, *reads).stdout
            for sample in (("-s", 5), ()):
                got = run("fm", "--mismatches", d, *extra, *sample, path, *reads).stdout
                assert sorted(got.splitlines()) == sorted(want.splitlines()) and want != "", (name, extra)
    path = EXP / "long_dna_sequence_allow_ambiguity.sufr"
    fa = tmp_path / "reads.fa"
    fa.write_text(">r1\nACGTACGTAC\n>r2\nGATTACAGATTACA\n")
    out = tmp_path / "out.txt"
    assert run("fm", "-d", 2, "-q", fa, "-t", 2, "-o", out, path).stdout == ""
    assert sorted(out.read_text().splitlines()) == sorted(run("approx", "-d", 2, "-q", fa, path).stdout.splitlines()) != []
    no_samples = run("fm", "--mismatches", 1, "-s", 0, path, "ACGT", check=False)
    assert no_samples.returncode == 1 and no_samples.stdout == "" and "-s" in no_samples.stderr and no_samples.stderr.count("\n") == 1
    too_many = run("fm", "--mismatches", 4, path, "ACGT", check=False)
    assert too_many.returncode == 1 and "at most 3" in too_many.stderr
    refused = run("fm", "-d", 1, EXP / "long_dna_sequence.sufr", "ACGT", check=False)
    assert refused.returncode == 1 and refused.stdout == "" and "positions" in refused.stderr
    assert "--mismatches" in run("--help").stdout
