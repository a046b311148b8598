"""The BWT of the indexed text, its runs and the LF mapping on the host (include/sufr_bwt.h, sufr_query.cpp) against a numpy
witness on the arrays oracle_helper.parse_sufr reads: bwt = text[(sa - 1) % n], counts = bincount, the run heads from
bwt[1:] != bwt[:-1], lf as the inverse of a stable argsort.  Every comparison is exact array equality."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sufr_amd
from sufr_amd import SufrFile, SufrHipError
from oracle_helper import GOLDEN, parse_sufr
from test_match_host import run

ROOT = Path(__file__).resolve().parent.parent
EXP = GOLDEN / "expected"
GOLDEN_FILES = sorted(p.name for p in EXP.glob("*.sufr"))
LF_FILES = ("1n.sufr", "2n.sufr", "2ns.sufr", "abba.sufr", "long_dna_sequence_allow_ambiguity.sufr", "uniprot.sufr")
STATS = ("runs", "records", "longest", "longest_rank")


# ---------------------------------------------------------------------------------------------------------------------
# the witness
# ---------------------------------------------------------------------------------------------------------------------
def witness(text, sa, min_len=1):
    """(bwt, counts, (rank, length, symbol, first), stats, lf) of a text and a suffix array (any array of text positions)"""
    text = np.frombuffer(bytes(text), dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    sa = np.asarray(sa).astype(np.int64)
    n, s = text.size, sa.size
    if s == 0:
        empty = np.zeros(0, dtype=np.uint64)
        return np.zeros(0, dtype=np.uint8), np.zeros(256, dtype=np.uint64), (empty,) * 4, dict.fromkeys(STATS, 0), empty
    bwt = text[(sa - 1) % n]
    counts = np.bincount(bwt, minlength=256).astype(np.uint64)
    heads = np.concatenate([[0], np.nonzero(bwt[1:] != bwt[:-1])[0] + 1])
    length = np.diff(np.concatenate([heads, [s]]))
    longest = int(np.argmax(length))                                 # (the first of the longest)
    stats = dict(runs=int(heads.size), records=0, longest=int(length[longest]), longest_rank=int(heads[longest]))
    keep = length >= max(min_len, 1)
    stats["records"] = int(keep.sum())
    records = tuple(a[keep].astype(np.uint64) for a in (heads, length, bwt[heads], sa[heads]))
    lf = np.empty(s, dtype=np.uint64)
    lf[np.argsort(bwt, kind="stable")] = np.arange(s, dtype=np.uint64)
    return bwt, counts, records, stats, lf


def golden(name):
    p = parse_sufr(EXP / name)
    return p, witness(p.text, p.sa)


def check_host(f: SufrFile, want, min_len=1, threads=(0,)):
    """bwt, counts, records, total, stats and lf of the host equal the witness, in the dtypes of the index width"""
    bwt, counts, records, stats, lf = want
    width = np.uint64 if f.index_width == 8 else np.uint32
    for t in threads:
        got_bwt, got_counts = f.bwt(threads=t)
        assert got_bwt.dtype == np.uint8 and got_counts.dtype == np.uint64 and got_counts.size == 256
        assert np.array_equal(got_bwt, bwt) and np.array_equal(got_counts, counts), t
        got = f.bwt_runs(min_len, threads=t)
        for i in range(4):
            assert got[i].dtype == np.uint64 and np.array_equal(got[i], records[i]), (t, i)
        assert got[4] == stats and got[0].size == stats["records"], (t, got[4], stats)
        got_lf = f.lf(threads=t)
        assert got_lf.dtype == width and np.array_equal(got_lf.astype(np.uint64), lf), t


# ---------------------------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_bwt_header_symbols_are_exported():
    hdr = (ROOT / "include" / "sufr_bwt.h").read_text()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(sufr_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(sufr_amd.BWT_EXPORTS), declared ^ set(sufr_amd.BWT_EXPORTS)
    L = sufr_amd.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(sufr_amd.LIB_PATH)], capture_output=True, text=True).stdout
    for name in declared:
        assert hasattr(L, name) and re.search(rf"\bT {name}\b", nm), name
    assert C.sizeof(sufr_amd.BwtStats) == 32
    assert hasattr(sufr_amd.Context, "set_bwt_tile")


def test_host_stubs_define_the_device_entry_points():
    stubs = (ROOT / "sufr_amd" / "csrc" / "sufr_host_stubs.cpp").read_text()
    device = [name for name in sufr_amd.BWT_EXPORTS if name.startswith("sufr_hip_")]
    assert len(device) == 4
    for name in device:
        assert re.search(rf"\bint {name}\(", stubs), name


# ---------------------------------------------------------------------------------------------------------------------
# against the witness
# ---------------------------------------------------------------------------------------------------------------------
def test_there_are_fourteen_golden_files():
    assert len(GOLDEN_FILES) == 14 and "uniprot-masked.sufr" in GOLDEN_FILES


@pytest.mark.parametrize("name", GOLDEN_FILES)
def test_host_equals_witness_on_golden_files(name):
    p, want = golden(name)
    f = SufrFile(EXP / name)                                         # (the seed-mask file too: nothing is refused)
    assert f.len_suffixes == p.num_suffixes and f.index_width == p.width
    check_host(f, want, threads=(1, 3, 0))
    for min_len in (2, 5):
        bwt, counts, records, stats, lf = witness(p.text, p.sa, min_len)
        got = f.bwt_runs(min_len)
        assert all(np.array_equal(got[i], records[i]) for i in range(4)) and got[4] == stats, min_len


def test_lf_walks_the_text_backwards_where_every_position_is_indexed():
    ran = []
    for name in GOLDEN_FILES:
        p = parse_sufr(EXP / name)
        if p.num_suffixes != p.text_len or p.seed_mask or p.max_query_len:
            continue
        sa = p.sa.astype(np.int64)
        lf = SufrFile(EXP / name).lf().astype(np.int64)
        assert np.array_equal(sa[lf], (sa - 1) % p.text_len), name
        assert np.array_equal(np.sort(lf), np.arange(sa.size)), name
        ran.append(name)
    assert set(LF_FILES) <= set(ran), ran


def test_anchors_of_the_witness():
    """numbers of a numpy run on the golden files, so that the witness itself is pinned"""
    p, (bwt, counts, records, stats, lf) = golden("uniprot.sufr")
    assert stats["runs"] == 49332 and stats["longest"] == 58 and int((counts > 0).sum()) == 23
    p, (bwt, counts, records, stats, lf) = golden("long_dna_sequence_allow_ambiguity.sufr")
    assert stats["runs"] == 15040 and stats["longest"] == 1999
    p, (bwt, counts, records, stats, lf) = golden("abba.sufr")
    assert stats["runs"] == 8


def test_capacity_counting_and_min_len():
    name = "uniprot.sufr"
    p, (bwt, counts, records, stats, lf) = golden(name)
    f = SufrFile(EXP / name)
    L = sufr_amd.lib()
    z = stats["records"]
    total, st = C.c_uint64(0), sufr_amd.BwtStats()
    assert L.sufr_file_bwt_runs(f._h, 1, 0, None, None, None, None, C.byref(total), C.byref(st), 0) == -5      # the counting call
    assert total.value == z and st.as_dict() == stats
    out = [np.full(z, 7, dtype=np.uint64) for _ in range(4)]
    total.value = 0
    assert L.sufr_file_bwt_runs(f._h, 1, z - 1, *(o.ctypes.data for o in out), C.byref(total), None, 0) == -5
    assert total.value == z and all((o == 7).all() for o in out)      # nothing written
    assert L.sufr_file_bwt_runs(f._h, 1, z, *(o.ctypes.data for o in out), C.byref(total), C.byref(st), 2) == 0
    assert total.value == z and all(np.array_equal(out[i], records[i]) for i in range(4)) and st.as_dict() == stats
    zero, one = f.bwt_runs(0), f.bwt_runs(1)
    assert all(np.array_equal(zero[i], one[i]) for i in range(4)) and zero[4] == one[4] == stats       # min_len 0 counts as 1
    none = f.bwt_runs(stats["longest"] + 1)
    assert all(a.size == 0 for a in none[:4])
    assert none[4] == dict(stats, records=0) and none[4]["runs"] == stats["runs"] > 0
    # NULL outputs are skipped
    only = np.zeros(256, dtype=np.uint64)
    assert L.sufr_file_bwt(f._h, None, only.ctypes.data, 0) == 0 and np.array_equal(only, counts)
    assert L.sufr_file_bwt(f._h, None, None, 0) == 0 and L.sufr_file_lf(f._h, None, 0) == 0


def test_arrays_of_no_and_one_rank(tmp_path):
    """(the golden empty.fa is no way to an empty array: the oracle and the builder refuse an empty sequence file, which
    test_oracle_golden.py holds them to; the arrays are written as they are instead)"""
    from test_repeat_host import _rewrite
    h = SufrFile(EXP / "3.sufr")
    for count in (0, 1):
        sa = np.array([5][:count], dtype=np.uint32)
        f = _rewrite(h, tmp_path / f"s{count}.sufr", [0], sa=sa, lcp=np.zeros(count, dtype=np.uint32))
        assert f.len_suffixes == count and f.text_len > 5
        check_host(f, witness(np.asarray(f.text), sa), threads=(1, 0))
    assert f.bwt_runs()[4] == dict(runs=1, records=1, longest=1, longest_rank=0) and f.lf().tolist() == [0]
    none = SufrFile(tmp_path / "s0.sufr")
    assert none.bwt_runs()[4] == dict.fromkeys(STATS, 0) and not none.bwt()[1].any() and none.lf().size == 0


# ---------------------------------------------------------------------------------------------------------------------
# planted arrays: none of the three assumes that the suffix array is sorted, so any permutation is a legal input and the BWT
# can be written down first
# ---------------------------------------------------------------------------------------------------------------------
def text_for(bwt: np.ndarray, sa: np.ndarray) -> np.ndarray:
    """the text whose BWT under the permutation sa is bwt"""
    text = np.empty(bwt.size, dtype=np.uint8)
    text[(sa.astype(np.int64) - 1) % bwt.size] = bwt
    return text


def rotation(n: int, zero_at: int) -> np.ndarray:
    """a permutation of [0, n) with the 0 -- the cyclic row -- at rank zero_at"""
    return ((np.arange(n, dtype=np.int64) - zero_at) % n).astype(np.uint32)


def runs_of(alphabet: bytes, count: int, mean: float, seed: int) -> np.ndarray:
    """count bytes in runs of geometric lengths; neighbouring runs differ"""
    rng = np.random.default_rng(seed)
    lengths = rng.geometric(1.0 / mean, size=count)                  # (count runs of at least 1: enough)
    syms = rng.integers(0, len(alphabet) - 1, lengths.size)
    syms = (np.cumsum(syms + 1)) % len(alphabet)                     # (a step of 1 .. len - 1: never the symbol before)
    keep = int(np.searchsorted(np.cumsum(lengths), count)) + 1
    return np.repeat(np.frombuffer(alphabet, dtype=np.uint8)[syms[:keep]], lengths[:keep])[:count].copy()


def write_arrays(path, text: np.ndarray, sa: np.ndarray) -> SufrFile:
    """a 32-bit .sufr file of these arrays as they are (one sequence; the LCP is not read by anything here)"""
    text, sa = np.ascontiguousarray(text, dtype=np.uint8), np.ascontiguousarray(sa, dtype=np.uint32)
    lcp = np.zeros(sa.size, dtype=np.uint32)
    starts = np.zeros(1, dtype=np.uint64)
    names = (C.c_char_p * 1)(b"1")
    err = C.create_string_buffer(256)
    rc = sufr_amd.lib().sufr_write_file(str(path).encode(), 0, 0, 0, text.ctypes.data, text.size, 4, sa.ctypes.data, lcp.ctypes.data, sa.size, 0, 0,
                                        None, starts.ctypes.data, 1, names, err, len(err))
    assert rc == 0, err.value
    return SufrFile(path)


def edges(records, tile: int):
    """what the runs of a witness do at the multiples of `tile`: (one begins at a multiple other than 0, one ends at a
    multiple, the most whole tiles one run covers)"""
    rank, length = records[0].astype(np.int64), records[1].astype(np.int64)
    end = rank + length
    whole = end // tile - (rank + tile - 1) // tile
    return bool(((rank % tile == 0) & (rank > 0)).any()), bool((end % tile == 0).any()), int(whole.max())


HOST_TILE = 1 << 16                                                   # BWT_HOST_TILE of sufr_query.cpp


def test_runs_over_the_tiles_of_the_host_path(tmp_path):
    """six and a bit tiles of the host path: a run from just before the end of tile 0 to exactly the end of tile 2 (two whole
    tiles inside), short runs over the other edges, and the cyclic row in the middle of a tile"""
    n = 6 * HOST_TILE + 77
    bwt = runs_of(b"ACGT$N", n, 5.0, seed=1)
    bwt[HOST_TILE - 10:3 * HOST_TILE] = ord("A")
    bwt[HOST_TILE - 11], bwt[3 * HOST_TILE] = ord("C"), ord("G")
    sa = rotation(n, 4 * HOST_TILE + 123)
    f = write_arrays(tmp_path / "planted.sufr", text_for(bwt, sa), sa)
    want = witness(np.asarray(f.text), sa)
    assert np.array_equal(want[0], bwt)
    begins, ends, whole = edges(want[2], HOST_TILE)
    assert begins and ends and whole >= 2 and want[3]["longest"] == 2 * HOST_TILE + 10 and want[3]["longest_rank"] == HOST_TILE - 10
    check_host(f, want, threads=(1, 3, 0))
    want = witness(np.asarray(f.text), sa, 4)
    got = f.bwt_runs(4, threads=5)
    assert all(np.array_equal(got[i], want[2][i]) for i in range(4)) and got[4] == want[3] and 0 < got[4]["records"] < got[4]["runs"]


# ---------------------------------------------------------------------------------------------------------------------
# sufr bwt
# ---------------------------------------------------------------------------------------------------------------------
def shown(c: int) -> str:
    return chr(c) if 0x20 < c < 0x7F and c != 0x5C else f"\\x{c:02X}"


def place(f: SufrFile, p: int) -> str:
    starts = np.array(f.sequence_starts, dtype=np.int64)
    i = int(np.searchsorted(starts, p, side="right")) - 1
    return f"{f.sequence_names[i]}:{p - int(starts[i])}"


def bwt_text(f: SufrFile, runs=False, min_len=1) -> str:
    bwt, counts = f.bwt()
    rank, length, symbol, first, st = f.bwt_runs(min_len)
    lines = [f"{shown(c)}\t{int(counts[c])}" for c in range(256) if counts[c]]
    if runs:
        lines += [f"{int(r)}\t{int(ln)}\t{shown(int(c))}\t{place(f, int(p))}" for r, ln, c, p in zip(rank, length, symbol, first)]
    lines += [f"# ranks\t{f.len_suffixes}", f"# runs\t{st['runs']}", f"# longest\t{st['longest']}", f"# longest_rank\t{st['longest_rank']}"]
    return "\n".join(lines) + "\n"


def test_cli_bwt_prints_what_the_python_calls_return(tmp_path):
    for name in ("3.sufr", "abba.sufr", "uniprot-masked.sufr"):
        f = SufrFile(EXP / name)
        assert run("bwt", EXP / name).stdout == bwt_text(f)
        assert run("bwt", "--runs", EXP / name).stdout == bwt_text(f, True)
        assert run("bwt", "--runs", "--min-len", 3, EXP / name).stdout == bwt_text(f, True, 3)
    f = SufrFile(EXP / "3.sufr")
    text = bwt_text(f)
    assert text.startswith("$\t") and "# runs\t" in text and text.count("\n") >= 9
    out, raw, lf = tmp_path / "bwt.tsv", tmp_path / "bwt.bin", tmp_path / "lf.bin"
    assert run("bwt", "-t", 2, "-o", out, "--bwt", raw, "--lf", lf, EXP / "3.sufr").stdout == "" and out.read_text() == text
    assert raw.stat().st_size == f.len_suffixes and np.array_equal(np.frombuffer(raw.read_bytes(), dtype=np.uint8), f.bwt()[0])
    assert lf.stat().st_size == f.len_suffixes * f.index_width
    assert np.array_equal(np.frombuffer(lf.read_bytes(), dtype=np.uint32 if f.index_width == 4 else np.uint64), f.lf())
    assert run("bwt", check=False).returncode == 2                   # no file
    assert run("bwt", "--table", EXP / "3.sufr", check=False).returncode == 2
    assert "  bwt " in run("--help").stdout
