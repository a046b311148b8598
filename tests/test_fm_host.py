"""The FM-index on the host (include/sufr_fm.h, sufr_query.cpp): backward search and locate without the text and the suffix array,
against the search of the same library on the suffix array and numpy slices of the arrays oracle_helper.parse_sufr reads.  Every
comparison is exact array equality.  The query sets and their conditions are built here and used by tests/test_fm_gpu.py too."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sufr_amd
from sufr_amd import SufrFile, SufrHipError, pack_queries
from oracle_helper import GOLDEN
from test_bwt_host import GOLDEN_FILES, LF_FILES, write_arrays
from test_match_host import run

ROOT = Path(__file__).resolve().parent.parent
EXP = GOLDEN / "expected"
SAMPLES = (1, 2, 7, 32, 0)
REFUSED = [n for n in GOLDEN_FILES if n not in LF_FILES]
UNSUPPORTED = -6


# ---------------------------------------------------------------------------------------------------------------------
# the witness and the query sets
# ---------------------------------------------------------------------------------------------------------------------
def sorted_sa(text: np.ndarray) -> np.ndarray:
    """the suffix array of a short text by sorting its suffixes as byte strings (a shorter suffix sorts first)"""
    raw = np.asarray(text, dtype=np.uint8).tobytes()
    return np.array(sorted(range(len(raw)), key=lambda p: raw[p:]), dtype=np.uint32)


class Witness:
    """occ and the backward search of a (text, suffix array) pair in numpy, with every occ argument a search meets"""

    def __init__(self, text, sa):
        self.text = np.asarray(text, dtype=np.uint8)
        self.sa = np.asarray(sa).astype(np.int64)
        self.n = self.s = self.text.size
        self.bwt = self.text[(self.sa - 1) % self.n]
        self.counts = np.bincount(self.bwt, minlength=256).astype(np.int64)
        self.C = np.concatenate([[0], np.cumsum(self.counts)])
        self.ranks_of = {c: np.nonzero(self.bwt == c)[0] for c in np.nonzero(self.counts)[0]}       # occ(c, r) = ranks_of[c] < r
        self.e = int(self.text[-1])

    def occ(self, c: int, r: int) -> int:
        return int(np.searchsorted(self.ranks_of[c], r, side="left"))

    def occ_by_cumsum(self, c: int) -> np.ndarray:
        """occ(c, r) for every r in [0, s], the way the issue names it"""
        return np.concatenate([[0], np.cumsum(self.bwt == c)])

    def search(self, q: bytes):
        """(lo, hi, the occ arguments met): the definition of include/sufr_fm.h, the empty query as sufr_file_search answers it"""
        m, args = len(q), []
        if m == 0:
            return 0, self.s, args
        if self.counts[q[-1]] == 0:
            return 0, 0, args
        lo, hi = int(self.C[q[-1]]), int(self.C[q[-1] + 1])
        for i in range(m - 2, -1, -1):
            c = q[i]
            if self.counts[c] == 0 or c == self.e:
                return 0, 0, args
            args += [lo, hi]
            lo, hi = int(self.C[c]) + self.occ(c, lo), int(self.C[c]) + self.occ(c, hi)
            if lo == hi:
                return 0, 0, args
        return lo, hi, args


def query_set(w: Witness, B: int, seed: int = 0, per_length: int = 8):
    """Substrings of the text at lengths 1, 2, 8, 31 and 200 and the same with one byte changed; queries that run over the
    text's end, that end in the end byte, that hold it inside; a byte that does not occur; the empty query; the whole text; the
    largest byte value (its range ends at s); and, where the array has more than one block, a query whose search meets an occ
    argument that is a multiple of B"""
    rng = np.random.default_rng(seed)
    raw, n = w.text.tobytes(), w.n
    absent = [c for c in range(255, -1, -1) if w.counts[c] == 0]
    other = absent[0] if absent else None                            # (all 256 values occur: nothing can be changed into an absent byte)
    qs = [b"", raw, raw[:8], raw[-1:], raw[-8:], raw[-4:] + raw[:3], raw[-5:] + b"AC", raw[-3:] + raw[-3:],
          bytes([int(w.text.max())]), bytes([int(w.text.min())])]
    if other is not None:
        qs += [bytes([other]), raw[:3] + bytes([other]), bytes([other]) + raw[:3]]
    for length in (1, 2, 8, 31, 200):
        for a in rng.integers(0, n, per_length):
            sub = raw[a:a + length]
            qs.append(sub)
            changed = bytearray(sub)
            at = int(rng.integers(0, len(changed)))
            pick = other if other is not None and length > 2 else int(w.text[int(rng.integers(0, n))])
            changed[at] = pick if pick != changed[at] else int(w.text[(a + 7) % n])
            qs.append(bytes(changed))
            qs.append(bytes(changed[::-1]) if length >= 8 else bytes(changed))
    for j in range(1, min((w.s - 1) // B, 3) + 1):                 # the suffix at rank j B, with the byte in front of it
        p = int(w.sa[j * B])
        if p > 0:
            qs.append(raw[p - 1:p + 200])
    return qs


def conditions(w: Witness, qs, B: int, q: int, max_hits: int = 0):
    """what a query set does, from the witness: (found, not found, the widest range, a final bound equal to s, an occ argument
    that is a positive multiple of B, a located position q - 1 steps from its mark, position 0 located)"""
    found = widest = 0
    ends = on_block = far = zero = False
    for query in qs:
        lo, hi, args = w.search(query)
        found += hi > lo
        widest = max(widest, hi - lo)
        ends = ends or (hi > lo and (hi == w.s or lo == w.s))
        on_block = on_block or any(a and a % B == 0 for a in args)
        pos = w.sa[lo:min(hi, lo + max_hits) if max_hits else hi]
        far = far or bool(q > 1 and (pos % q == q - 1).any())
        zero = zero or bool((pos == 0).any())
    return dict(found=int(found), missed=len(qs) - int(found), widest=int(widest), ends=ends, on_block=on_block, far=far, zero=zero)


def file_witness(name):
    f = SufrFile(EXP / name)
    return f, Witness(np.asarray(f.text), np.asarray(f.suffix_array))


def want_locate(w: Witness, lo, hi, max_hits, dtype):
    """(offsets, positions) as the locate contract lays them out"""
    parts = [w.sa[int(a):min(int(b), int(a) + max_hits) if max_hits else int(b)] for a, b in zip(lo, hi)]
    off = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)
    return off, (np.concatenate(parts) if parts else np.zeros(0)).astype(dtype)


# ---------------------------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_fm_header_symbols_are_exported():
    hdr = (ROOT / "include" / "sufr_fm.h").read_text()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(sufr_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(sufr_amd.FM_EXPORTS), declared ^ set(sufr_amd.FM_EXPORTS)
    L = sufr_amd.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(sufr_amd.LIB_PATH)], capture_output=True, text=True).stdout
    for name in declared:
        assert hasattr(L, name) and re.search(rf"\bT {name}\b", nm), name
    assert C.sizeof(sufr_amd.FmInfo) == 64
    assert hasattr(SufrFile, "fm") and hasattr(sufr_amd.DeviceIndex, "fm_device")


def test_host_stubs_define_the_device_entry_points():
    stubs = (ROOT / "sufr_amd" / "csrc" / "sufr_host_stubs.cpp").read_text()
    device = [name for name in sufr_amd.FM_EXPORTS if name.startswith("sufr_hip_")]
    assert len(device) == 5
    for name in device:
        assert re.search(rf"\b(int|void) {name}\(", stubs), name


# ---------------------------------------------------------------------------------------------------------------------
# against the search on the suffix array
# ---------------------------------------------------------------------------------------------------------------------
def test_the_witness_is_the_search_on_the_suffix_array():
    """the numpy backward search, which the conditions are taken from, gives the ranges of SufrFile.search_batch, and its occ
    is the cumulative sum"""
    for name in LF_FILES:
        f, w = file_witness(name)
        qs = query_set(w, 96)
        lo, hi = f.search_batch(qs)
        got = [w.search(q)[:2] for q in qs]
        assert [g[0] for g in got] == lo.tolist() and [g[1] for g in got] == hi.tolist(), name
        for c in list(w.ranks_of)[:3]:
            by_sum = w.occ_by_cumsum(int(c))
            assert all(w.occ(int(c), r) == by_sum[r] for r in (0, 1, w.s // 2, w.s - 1, w.s)), (name, c)


@pytest.mark.parametrize("name", LF_FILES)
def test_search_and_locate_equal_the_suffix_array(name):
    f, w = file_witness(name)
    dtype = np.uint64 if f.index_width == 8 else np.uint32
    B = None
    for sample in SAMPLES:
        for threads in (1, 3, 0):
            fm = f.fm(sample, threads)
            info = fm.info
            B = info["block"]
            assert info["ranks"] == w.s and info["sample"] == sample and info["width"] == f.index_width and info["end_byte"] == w.e
            assert info["symbols"] == int((w.counts > 0).sum()) and info["samples"] == (0 if not sample else int((w.sa % sample == 0).sum()))
            qs = query_set(w, B, seed=sample)
            want = f.search_batch(qs)
            lo, hi = fm.search_batch(qs, threads)
            assert lo.dtype == np.uint64 and np.array_equal(lo, want[0]) and np.array_equal(hi, want[1]), (sample, threads)
            if not sample:
                with pytest.raises(SufrHipError) as err:
                    fm.locate_ranges(lo, hi)
                assert err.value.code == UNSUPPORTED
                continue
            for max_hits in (0, 3):
                off, pos = fm.locate_ranges(lo, hi, max_hits, threads)
                w_off, w_pos = want_locate(w, lo, hi, max_hits, dtype)
                assert pos.dtype == dtype and np.array_equal(off, w_off) and np.array_equal(pos, w_pos), (sample, threads, max_hits)
            fm.close()
    # every rank at once: the whole suffix array comes back
    fm = f.fm(7)
    off, pos = fm.locate_ranges(np.zeros(1, dtype=np.uint64), np.array([w.s], dtype=np.uint64))
    assert np.array_equal(pos, w.sa.astype(dtype)) and off.tolist() == [0, w.s]
    by_query = fm.locate([w.text.tobytes()[:4], b""], max_hits=2)
    assert [p.tolist() for p in by_query] == [w.sa[a:min(b, a + 2)].tolist() for a, b in ([w.search(w.text.tobytes()[:4])[:2], (0, w.s)])]
    assert [c.count for c in fm.count([w.text.tobytes()[:2]])] == [c.count for c in f.count([w.text.tobytes()[:2]])]


def test_query_sets_meet_their_conditions():
    """a third found and a third not; on the files that have the ranks for it a range of two blocks and more, a bound equal to
    s, an occ argument on a block's first rank, a located rank q - 1 steps from its mark, and the cyclic row located"""
    for name in LF_FILES:
        f, w = file_witness(name)
        B = f.fm(0).info["block"]
        for q in (2, 7, 32):
            c = conditions(w, query_set(w, B, seed=q), B, q)
            total = c["found"] + c["missed"]
            assert 3 * c["found"] >= total and 3 * c["missed"] >= total, (name, c)
            assert c["ends"] and c["zero"], (name, q, c)
            if w.s > 20 * B:
                assert c["widest"] >= 2 * B and c["on_block"] and c["far"], (name, q, c)


def test_the_index_outlives_the_file_and_builds_are_equal(tmp_path):
    import shutil
    path = tmp_path / "copy.sufr"
    shutil.copy(EXP / "uniprot.sufr", path)
    f = SufrFile(path)
    w = Witness(np.array(f.text), np.array(f.suffix_array))          # (copies: a view would keep the file mapped)
    qs = query_set(w, 160)
    want = f.search_batch(qs)
    a, b = f.fm(32, 1), f.fm(32, 5)
    f.close()
    assert f.closed
    path.write_bytes(b"")                                            # the file is gone: the index owns what it reads
    assert a.info == b.info
    for fm in (a, b):
        lo, hi = fm.search_batch(qs)
        assert np.array_equal(lo, want[0]) and np.array_equal(hi, want[1])
        off, pos = fm.locate_ranges(lo, hi, 4)
        w_off, w_pos = want_locate(w, lo, hi, 4, np.uint32)
        assert np.array_equal(off, w_off) and np.array_equal(pos, w_pos)


# ---------------------------------------------------------------------------------------------------------------------
# refusals, sizes, call shapes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", REFUSED)
def test_partial_masked_and_capped_files_are_refused(name):
    assert len(REFUSED) == 8
    f = SufrFile(EXP / name)
    assert f.len_suffixes != f.text_len or f.seed_mask or f.max_query_len
    with pytest.raises(SufrHipError) as err:
        f.fm()
    assert err.value.code == UNSUPPORTED


def test_an_end_byte_that_occurs_twice_is_refused(tmp_path):
    text = np.frombuffer(b"ACGT$GATTACA$", dtype=np.uint8)
    f = write_arrays(tmp_path / "twice.sufr", text, sorted_sa(text))
    assert f.len_suffixes == f.text_len and not f.max_query_len and not f.seed_mask
    with pytest.raises(SufrHipError) as err:
        f.fm()
    assert err.value.code == UNSUPPORTED
    once = np.frombuffer(b"ACGT%GATTACA$", dtype=np.uint8)           # (the delimiter is not special; the last byte is)
    g = write_arrays(tmp_path / "once.sufr", once, sorted_sa(once))
    assert g.fm(2).locate([b"A", b"T%G", b"$", b"A$", b"$A"])[0].tolist() == [p for p in sorted_sa(once).tolist() if once[p] == ord("A")]


def test_bytes_meet_the_size_condition():
    """derived, not measured: K <= 8, w == 4 and sample == 32 take 128 / 96 + 16 / 64 + 4 / 32 = 1.71 bytes per rank"""
    f = SufrFile(EXP / "long_dna_sequence_allow_ambiguity.sufr")
    info = f.fm(32).info
    s = info["ranks"]
    assert info["symbols"] <= 8 and info["width"] == 4 and (info["block"], info["stride"]) == (96, 128)
    assert info["bytes"] <= 2 * s + 65536
    assert info["bytes"] == (s // 96 + 1) * 128 + (s + 63) // 64 * 16 + info["samples"] * 4 + 257 * 8 + 256 * 4
    assert info["samples"] == (s + 31) // 32 and info["bytes"] < 1.72 * s + 4096
    wide = SufrFile(EXP / "uniprot.sufr").fm(32).info               # 23 byte values: 96 bytes of counts, 160 of BWT
    assert (wide["symbols"], wide["block"], wide["stride"]) == (23, 160, 256)


def random_text(n: int, seed: int, alphabet: bytes = b"ACGT") -> np.ndarray:
    rng = np.random.default_rng(seed)
    text = np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)].copy()
    text[-1] = ord("$")
    return text


@pytest.mark.parametrize("s", [95, 96, 97, 192, 64, 65, 256, 257])
def test_sizes_around_the_block_and_the_mark_word(tmp_path, s):
    """B - 1, B, B + 1, 2 B, 64, 65 and 256, 257: the trailing block and the last mark word"""
    text = random_text(s, s)
    sa = sorted_sa(text)
    f = write_arrays(tmp_path / "s.sufr", text, sa)
    w = Witness(text, sa)
    for sample in (1, 5):
        fm = f.fm(sample)
        assert fm.info["block"] == 96
        qs = query_set(w, 96, seed=s)
        lo, hi = fm.search_batch(qs)
        want = f.search_batch(qs)
        assert np.array_equal(lo, want[0]) and np.array_equal(hi, want[1])
        off, pos = fm.locate_ranges(np.zeros(1, dtype=np.uint64), np.array([s], dtype=np.uint64))
        assert np.array_equal(pos, sa)
    assert w.search(bytes([int(text.max())]))[1] == s                # a bound equal to s: occ(c, s) reads the last block


def test_three_tiles_of_the_host_build(tmp_path):
    """140 001 ranks: the host build cuts them into tiles of 65 472 (whole blocks and mark words below 2^16), so the bases of the
    checkpoints, of the kept values and of the mark counts cross two tile edges, and workers share the tiles"""
    s = 140_001
    text = random_text(s, 21)
    raw = text.tobytes()
    sa = np.array(sorted(range(s), key=lambda p: raw[p:p + 64]), dtype=np.uint32)      # (random DNA: 64 bytes tell any two suffixes apart)
    f = write_arrays(tmp_path / "tiles.sufr", text, sa)
    tile = 65536 // 192 * 192
    assert 2 * tile < s < 3 * tile
    rng = np.random.default_rng(5)
    qs = [raw[a:a + m] for m in (1, 2, 8, 31) for a in rng.integers(0, s - 31, 40)] + [b"", raw[-9:], raw[:12], b"ACGTTGCAAC", b"T", b"$A"]
    qs += [raw[int(sa[r]) - 1:int(sa[r]) + 40] for r in (tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 63, s - 1) if sa[r] > 0]
    want = f.search_batch(qs)
    assert 3 * int((want[1] > want[0]).sum()) >= len(qs) and int(want[1].max()) == s
    infos = []
    for sample in (1, 7, 32):
        for threads in (1, 3, 0):
            fm = f.fm(sample, threads)
            infos.append(fm.info)
            assert infos[-1]["block"] == 96 and infos[-1]["samples"] == (s + sample - 1) // sample
            lo, hi = fm.search_batch(qs, threads)
            assert np.array_equal(lo, want[0]) and np.array_equal(hi, want[1]), (sample, threads)
            off, pos = fm.locate_ranges(np.zeros(1, dtype=np.uint64), np.array([s], dtype=np.uint64), 0, threads)
            assert np.array_equal(pos, sa), (sample, threads)
    assert infos[0] == infos[1] == infos[2] and infos[6] == infos[7] == infos[8]


def test_all_byte_values_take_the_wide_stride(tmp_path):
    rng = np.random.default_rng(11)
    text = rng.integers(0, 255, 5000).astype(np.uint8)
    text[:255] = np.arange(255)
    text[-1] = 255                                                   # the end byte occurs once
    sa = sorted_sa(text)
    f = write_arrays(tmp_path / "bytes.sufr", text, sa)
    w = Witness(text, sa)
    fm = f.fm(32)
    info = fm.info
    assert (info["symbols"], info["block"], info["stride"]) == (256, 1024, 2048)
    qs = query_set(w, 1024)
    lo, hi = fm.search_batch(qs)
    want = f.search_batch(qs)
    assert np.array_equal(lo, want[0]) and np.array_equal(hi, want[1])
    off, pos = fm.locate_ranges(lo, hi)
    w_off, w_pos = want_locate(w, lo, hi, 0, np.uint32)
    assert np.array_equal(off, w_off) and np.array_equal(pos, w_pos)
    c = conditions(w, qs, 1024, 32)
    assert c["on_block"] and c["far"] and c["zero"] and c["ends"], c


def test_capacity_max_hits_and_no_queries():
    f, w = file_witness("long_dna_sequence_allow_ambiguity.sufr")
    L = sufr_amd.lib()
    fm = f.fm(7)
    qs = query_set(w, 96)
    qb, qoff = pack_queries(qs)
    lo, hi = fm.search_batch(qs)
    w_off, w_pos = want_locate(w, lo, hi, 5, np.uint32)
    z = int(w_off[-1])
    assert z > 50
    off, pos = np.full(len(qs) + 1, 7, dtype=np.uint64), np.full(z + 9, 0xAAAAAAAA, dtype=np.uint32)
    total = C.c_uint64(0)
    args = (fm._h, lo.ctypes.data, hi.ctypes.data, len(qs), 5, off.ctypes.data, pos.ctypes.data)
    assert L.sufr_fm_locate_batch(*args, z - 1, C.byref(total), 0) == -5
    assert total.value == z and (pos == 0xAAAAAAAA).all()            # no position written
    assert L.sufr_fm_locate_batch(*args, z, C.byref(total), 2) == 0
    assert total.value == z and np.array_equal(off, w_off) and np.array_equal(pos[:z], w_pos) and (pos[z:] == 0xAAAAAAAA).all()
    assert L.sufr_fm_locate_batch(fm._h, None, None, 0, 0, off.ctypes.data, None, 0, C.byref(total), 0) == 0 and total.value == 0 and off[0] == 0
    assert L.sufr_fm_search_batch(fm._h, None, None, 0, None, None, 0) == 0
    bad = np.array([w.s + 1], dtype=np.uint64)
    assert L.sufr_fm_locate_batch(fm._h, lo.ctypes.data, bad.ctypes.data, 1, 0, off.ctypes.data, pos.ctypes.data, z, C.byref(total), 0) == -1
    assert qb.size == int(qoff[-1])


# ---------------------------------------------------------------------------------------------------------------------
# sufr fm
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_fm_prints_the_lines_of_count_and_locate(tmp_path):
    for name, queries in (("long_dna_sequence_allow_ambiguity.sufr", ["ACGT", "GATTACA", "N", "TTTTTTTTTTTTTTTTTTTTTTTTTT", "AC"]),
                          ("uniprot.sufr", ["MKV", "LLLL", "W", "XQZJ", "AAAAAA"]), ("2ns.sufr", ["AC", "GT", "N", "ACGTN"])):
        path = EXP / name
        assert run("fm", path, *queries).stdout == run("count", path, *queries).stdout != ""
        for extra in ((), ("-a",)):
            want, got = run("locate", *extra, path, *queries), run("fm", "--locate", *extra, "-s", 5, path, *queries)
            assert got.stdout == want.stdout != "" and got.stderr == want.stderr
    path = EXP / "uniprot.sufr"
    out = tmp_path / "fm.txt"
    assert run("fm", "--locate", "-t", 2, "-o", out, path, "MKV").stdout == "" and out.read_text() == run("locate", path, "MKV").stdout
    few = run("fm", "--locate", "-a", "--max-hits", 2, path, "LL").stdout.split()
    assert few == run("locate", "-a", path, "LL").stdout.split()[:3]
    reads = tmp_path / "reads.fa"
    reads.write_text(">r1\nMKV\n>r2\nLLLL\n")
    assert run("fm", "-q", reads, path).stdout.split() == ["r1", run("count", path, "MKV").stdout.split()[1], "r2", run("count", path, "LLLL").stdout.split()[1]]
    refused = run("fm", EXP / "long_dna_sequence.sufr", "ACGT", check=False)
    assert refused.returncode == 1 and refused.stdout == "" and refused.stderr.count("\n") == 1 and "positions" in refused.stderr
    masked = run("fm", EXP / "uniprot-masked.sufr", "MKV", check=False)
    assert masked.returncode == 1 and masked.stderr.count("\n") == 1 and "seed mask" in masked.stderr
    assert run("fm", check=False).returncode == 2 and run("fm", path, check=False).returncode == 2
    assert "  fm " in run("--help").stdout
