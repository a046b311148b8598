"""k-mer spectra, occurrence maps and unique lengths on the host (include/sufr_kmer.h): no GPU.

The witness uses neither implementation and no LCP array: a Python dictionary of the k-byte windows at the indexed, whole
positions of the file's text gives the counts; a shortest-unique-prefix search that groups the indexed positions by one more
byte per round gives the unique lengths.  Breaks come from the sequence starts alone.  The shared arithmetic of the device
path (sufr_amd/csrc/sufr_kmer_scan.h through tests/kmer_shim.cpp) is held to a direct per-interval count.
"""
import ctypes as C
import re
import subprocess
import zlib
from pathlib import Path

import numpy as np
import pytest

import sufr_amd
from sufr_amd import SufrFile, SufrHipError, synth
from oracle_helper import GOLDEN
from test_match_host import run
from test_mem_host import ADVERSARIAL, BUILDS, _adversarial_body, _fasta_from

ROOT = Path(__file__).resolve().parent.parent
EXP = GOLDEN / "expected"
GOLDEN_FILES = sorted(p.name for p in EXP.glob("*.sufr"))
KS = (1, 2, 3, 8, 21)
BINS = (1, 2, 256)


# ---------------------------------------------------------------------------------------------------------------------
# the witness
# ---------------------------------------------------------------------------------------------------------------------
def brk_of(f: SufrFile) -> np.ndarray:
    """brk[p] for every text position: the smallest break >= p; breaks are n - 1 and start_i - 1 for i >= 1."""
    n = f.text_len
    breaks = np.array(sorted({n - 1} | {s - 1 for s in f.sequence_starts[1:]}), dtype=np.int64)
    return breaks[np.searchsorted(breaks, np.arange(n, dtype=np.int64), side="left")]


def witness_kmers(f: SufrFile, k: int, bins: int):
    """(hist, stats, occ by rank, occ by position) from a dictionary of the windows."""
    tb = bytes(f.text)
    sa = np.asarray(f.suffix_array).astype(np.int64)
    brk = brk_of(f)
    whole = sa + k <= brk[sa] if sa.size else np.zeros(0, dtype=bool)
    d = {}
    for p in sa[whole].tolist():
        w = tb[p:p + k]
        d[w] = d.get(w, 0) + 1
    dt = np.uint32 if f.index_width == 4 else np.uint64
    rank = np.array([d[tb[p:p + k]] if wh else 0 for p, wh in zip(sa.tolist(), whole.tolist())], dtype=dt)
    pos = np.zeros(f.text_len, dtype=dt)
    pos[sa] = rank
    hist = np.zeros(bins, dtype=np.uint64)
    for c in d.values():
        hist[min(c, bins) - 1] += 1
    counts = list(d.values())
    stats = dict(whole=sum(counts), distinct=len(counts), unique=sum(c == 1 for c in counts), max_count=max(counts, default=0))
    return hist, stats, rank, pos


def witness_unique(f: SufrFile):
    """(by rank, by position): round u splits the groups of indexed positions that agree on u - 1 bytes by byte u; a position
    alone in its group has its shortest unique prefix, u.  A byte past the end of the text equals nothing."""
    tb = bytes(f.text)
    n = f.text_len
    sa = np.asarray(f.suffix_array).astype(np.int64)
    brk = brk_of(f)
    gid = {p: 0 for p in sa.tolist()}
    active = sa.tolist()
    ul = {}
    u = 0
    while active:
        u += 1
        buckets = {}
        for p in active:
            buckets.setdefault((gid[p], tb[p + u - 1] if p + u - 1 < n else -1 - p), []).append(p)
        active = []
        for i, ps in enumerate(buckets.values()):
            if len(ps) == 1:
                ul[ps[0]] = u
            else:
                for p in ps:
                    gid[p] = i
                active.extend(ps)
    dt = np.uint32 if f.index_width == 4 else np.uint64
    rank = np.array([ul[p] if p + ul[p] <= brk[p] else 0 for p in sa.tolist()], dtype=dt)
    pos = np.zeros(n, dtype=dt)
    pos[sa] = rank
    return rank, pos


def check_kmers(f: SufrFile, ks, bins_list=BINS, threads=0):
    for k in ks:
        for bins in bins_list:
            hist, stats, rank, pos = witness_kmers(f, k, bins)
            for occ, want in (("rank", rank), ("position", pos), (None, None)):
                h, st, got = f.kmers(k, bins, occ, threads=threads)
                assert np.array_equal(h, hist), (k, bins, occ, h[:8], hist[:8])
                assert st == stats, (k, bins, occ, st, stats)
                if occ is None:
                    assert got is None
                else:
                    assert got.dtype == want.dtype and np.array_equal(got, want), (k, bins, occ)


def check_unique(f: SufrFile):
    rank, pos = witness_unique(f)
    assert np.array_equal(f.unique_lengths(), rank)
    assert np.array_equal(f.unique_lengths(by_position=True), pos)
    return rank


# ---------------------------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_kmer_header_symbols_are_exported():
    hdr = (ROOT / "include" / "sufr_kmer.h").read_text()
    assert "#define SUFR_KMER_BY_POSITION 0x1u" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(sufr_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(sufr_amd.KMER_EXPORTS), declared ^ set(sufr_amd.KMER_EXPORTS)
    L = sufr_amd.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(sufr_amd.LIB_PATH)], capture_output=True, text=True).stdout
    for name in declared:
        assert hasattr(L, name) and re.search(rf"\bT {name}\b", nm), name
    assert L.sufr_hip_abi_version() == 3
    assert C.sizeof(sufr_amd.KmerStats) == 32


def test_host_stubs_define_the_device_entry_points():
    stubs = (ROOT / "sufr_amd" / "csrc" / "sufr_host_stubs.cpp").read_text()
    for name in sufr_amd.KMER_EXPORTS:
        if name.startswith("sufr_hip_"):
            assert re.search(rf"\bint {name}\(", stubs), name


# ---------------------------------------------------------------------------------------------------------------------
# against the witness
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN_FILES)
def test_host_equals_witness_on_golden_files(name):
    f = SufrFile(EXP / name)
    if f.seed_mask:
        for call in (lambda: f.kmers(3), lambda: f.unique_lengths(), lambda: f.kmers(0)):
            with pytest.raises(SufrHipError) as e:
                call()
            assert e.value.code == -6
        return
    above = int(np.asarray(f.lcp).max()) + 1 if f.len_suffixes else 30
    check_kmers(f, KS + (above,))
    # above the largest LCP every interval is one rank: every whole position has count 1
    _, st, occ = f.kmers(above, 4, "rank")
    assert set(np.unique(occ).tolist()) <= {0, 1} and st["max_count"] <= 1 and st["unique"] == st["distinct"] == st["whole"]
    check_unique(f)
    with pytest.raises(SufrHipError) as e:
        f.kmers(0)
    assert e.value.code == -1


def test_inputs_are_not_vacuous():
    """a golden file with several sequences has an indexed position that is not whole for k = 8 (and not only the '$')"""
    found = []
    for name in GOLDEN_FILES:
        f = SufrFile(EXP / name)
        if f.num_sequences < 2 or f.seed_mask:
            continue
        sa = np.asarray(f.suffix_array).astype(np.int64)
        brk = brk_of(f)
        short = sa[(sa + 8 > brk[sa]) & (brk[sa] < f.text_len - 1)]
        if short.size:
            found.append(name)
    assert found, "no multi-sequence golden file has an indexed position whose 8-mer crosses a delimiter"


def test_bins_zero_and_null_outputs():
    f = SufrFile(EXP / "3.sufr")
    L = sufr_amd.lib()
    hist = np.zeros(4, dtype=np.uint64)
    st = sufr_amd.KmerStats()
    assert L.sufr_file_kmers(f._h, 3, 0, 0, hist.ctypes.data, None, None, 1) == -1          # a histogram of no bins
    assert L.sufr_file_kmers(f._h, 3, 0, 0, None, None, C.byref(st), 1) == 0                # ... none asked for: fine
    assert st.as_dict() == witness_kmers(f, 3, 1)[1]
    assert L.sufr_file_kmers(f._h, 3, 0, 4, None, None, None, 1) == 0
    assert L.sufr_file_kmers(None, 3, 0, 4, None, None, None, 1) == -1


@pytest.mark.parametrize("kind", ADVERSARIAL)
@pytest.mark.parametrize("build", BUILDS)
def test_host_equals_witness_on_oracle_builds(oracle, tmp_path, kind, build):
    _fasta_from(_adversarial_body(kind), tmp_path / "x.fa")
    oracle.create(tmp_path / "x.fa", tmp_path / "x.sufr", **build)
    f = SufrFile(tmp_path / "x.sufr")
    L = build.get("max_query_len", 0)
    assert f.max_query_len == L
    if kind == "many_short":
        assert f.num_sequences > 50                                  # (the break lookup is a real search)
    if L:
        check_kmers(f, [k for k in (1, 2, 3, 6, 8, 11) if k <= L], bins_list=(2, 256))
        for call in (lambda: f.kmers(L + 1), lambda: f.kmers(21, occ="position"), lambda: f.unique_lengths(),
                     lambda: f.unique_lengths(by_position=True)):
            with pytest.raises(SufrHipError) as e:
                call()
            assert e.value.code == -6
        return
    check_kmers(f, (1, 3, 8, 21), bins_list=(2, 256))
    check_unique(f)
    if kind == "all_a":
        assert f.kmers(8)[1]["max_count"] > 1000


def test_chunks_and_threads_on_a_larger_text(oracle, tmp_path):
    """150 000 symbols in five sequences with planted repeats: more than one chunk of the host passes, intervals that cross
    chunk ends, any number of workers"""
    rng = np.random.default_rng(11)
    body = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 150_000)].copy()
    body[20_000:90_000] = ord("A")                                   # one interval over more than a chunk of ranks
    for at in range(100_000, 140_000, 4_000):
        body[at:at + 300] = body[95_000:95_300]
    body[[30_000, 60_000, 99_000, 120_000]] = ord("%")
    _fasta_from(body, tmp_path / "x.fa")
    oracle.create(tmp_path / "x.fa", tmp_path / "x.sufr", is_dna=True, threads=4)
    f = SufrFile(tmp_path / "x.sufr")
    assert f.num_sequences == 5 and f.len_suffixes > 2 * 65536
    check_kmers(f, (3, 12), bins_list=(256,), threads=1)
    want = f.kmers(12, 5000, "position", threads=1)
    assert want[1]["max_count"] > 20_000
    for threads in (0, 2, 7):
        got = f.kmers(12, 5000, "position", threads=threads)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1] and np.array_equal(got[2], want[2])
    # (the unique lengths are held to their witness on the small files: its rounds are quadratic in a run like this one)
    lcp = np.asarray(f.lcp).astype(np.int64)
    one = f.unique_lengths(threads=1)
    assert 20_000 < int(one.max()) <= 1 + int(lcp.max()) and np.array_equal(f.unique_lengths(threads=7), one)


def positional_breaks_file(oracle, tmp_path, n=2600, starts=(0, 700, 1500)):
    """A^n$ indexed as one text, written again with sequence starts that no byte marks: the breaks are positional, and the
    ranks whose k-mer runs over one lie in the same k-interval as the whole ranks"""
    _fasta_from(np.full(n, ord("A"), dtype=np.uint8), tmp_path / "a.fa")
    oracle.create(tmp_path / "a.fa", tmp_path / "a.sufr", is_dna=True)
    f = SufrFile(tmp_path / "a.sufr")
    text, sa, lcp = (np.asarray(a).copy() for a in (f.text, f.suffix_array, f.lcp))
    st = np.array(starts, dtype=np.uint64)
    names = (C.c_char_p * len(starts))(*[b"s%d" % i for i in range(len(starts))])
    err = C.create_string_buffer(256)
    rc = sufr_amd.lib().sufr_write_file(str(tmp_path / "b.sufr").encode(), 1, 0, 0, text.ctypes.data, text.size, 4, sa.ctypes.data,
                                        lcp.ctypes.data, sa.size, 0, 0, None, st.ctypes.data, len(starts), names, err, len(err))
    assert rc == 0, err.value
    return SufrFile(tmp_path / "b.sufr")


def test_breaks_are_positional(oracle, tmp_path):
    f = positional_breaks_file(oracle, tmp_path)
    assert f.sequence_starts == [0, 700, 1500]
    check_kmers(f, (1, 7, 700, 801), bins_list=(2, 256))
    _, st, occ = f.kmers(7, 256, "position")
    assert st == dict(whole=2601 - 3 * 7, distinct=1, unique=0, max_count=2601 - 3 * 7)
    assert not occ[693:700].any() and not occ[1493:1500].any() and occ[692] == occ[700] == st["whole"]
    check_unique(f)


# ---------------------------------------------------------------------------------------------------------------------
# the shared arithmetic (sufr_kmer_scan.h) on the CPU
# ---------------------------------------------------------------------------------------------------------------------
SHIM_SRC = ROOT / "tests" / "kmer_shim.cpp"
SHIM_DEPS = (SHIM_SRC, ROOT / "sufr_amd" / "csrc" / "sufr_kmer_scan.h")


def _stale(out: Path) -> bool:
    return not out.exists() or any(out.stat().st_mtime < p.stat().st_mtime for p in SHIM_DEPS)


@pytest.fixture(scope="module")
def shim():
    out = ROOT / "tests" / "_build" / "libkmer_shim.so"
    out.parent.mkdir(exist_ok=True)
    if _stale(out):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", str(out), str(SHIM_SRC)], check=True)
    L = C.CDLL(str(out))
    L.shim_kmer_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]
    L.shim_kmer_counts.restype = C.c_int
    L.shim_kmer_brk.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64]; L.shim_kmer_brk.restype = C.c_uint64
    L.shim_kmer_bin.argtypes = [C.c_uint64, C.c_uint64]; L.shim_kmer_bin.restype = C.c_uint64
    return L


def direct_counts(head: np.ndarray, whole: np.ndarray) -> np.ndarray:
    """the whole ranks of the interval of every rank; intervals begin at heads (and at rank 0)"""
    out = np.zeros(head.size, dtype=np.uint64)
    cuts = sorted({0, head.size} | set(np.nonzero(head)[0].tolist()))
    for a, b in zip(cuts[:-1], cuts[1:]):
        out[a:b] = int(whole[a:b].sum())
    return out


def shim_counts(L, head, whole, tile, group):
    head = np.ascontiguousarray(head, dtype=np.uint8)
    whole = np.ascontiguousarray(whole, dtype=np.uint8)
    out = np.zeros(max(head.size, 1), dtype=np.uint64)
    assert L.shim_kmer_counts(head.ctypes.data, whole.ctypes.data, head.size, tile, group, out.ctypes.data) == 0
    return out[:head.size]


def test_tile_summaries_and_carries_equal_a_direct_count(shim):
    rng = np.random.default_rng(7)
    n = 0
    for length in range(0, 41):
        cases = [(np.ones(length, dtype=np.uint8), "all heads"), (np.zeros(length, dtype=np.uint8), "no heads")]
        for at in {0, length // 2, max(length - 1, 0)}:
            h = np.zeros(length, dtype=np.uint8)
            h[at:at + 1] = 1
            cases.append((h, f"single head at {at}"))
        for dens in (2, 5, 13):
            for _ in range(3):
                cases.append(((rng.integers(0, dens, length) == 0).astype(np.uint8), f"random 1/{dens}"))
        for head, what in cases:
            for whole in (np.ones(length, dtype=np.uint8), (rng.integers(0, 3, length) > 0).astype(np.uint8), np.zeros(length, dtype=np.uint8)):
                want = direct_counts(head, whole)
                for tile in range(1, 10):
                    for group in (1, 2, 5):
                        got = shim_counts(shim, head, whole, tile, group)
                        assert np.array_equal(got, want), (length, what, tile, group, head, whole, got, want)
                        n += 1
    assert n > 10_000
    # whole 64-rank words, four to 256 words to a tile, as the kernels use them
    for length in (63, 64, 65, 1000, 16_384 + 70):
        head = (rng.integers(0, 97, length) == 0).astype(np.uint8)
        whole = (rng.integers(0, 4, length) > 0).astype(np.uint8)
        for group in (1, 4, 256):
            assert np.array_equal(shim_counts(shim, head, whole, 64, group), direct_counts(head, whole))
    assert shim.shim_kmer_counts(None, None, 0, 65, 1, None) == -1


def test_break_lookup_and_bins(shim):
    starts = np.array([0, 5, 6, 20], dtype=np.uint64)
    for p in range(30):
        want = min(b for b in (4, 5, 19, 29) if b >= p)
        assert shim.shim_kmer_brk(starts.ctypes.data, 4, 30, p) == want
        assert shim.shim_kmer_brk(starts.ctypes.data, 1, 30, p) == 29 == shim.shim_kmer_brk(None, 0, 30, p)
    assert [shim.shim_kmer_bin(c, 4) for c in (1, 2, 3, 4, 5, 1 << 40)] == [0, 1, 2, 3, 3, 3]
    assert [shim.shim_kmer_bin(c, 1) for c in (1, 9)] == [0, 0]


def test_shared_arithmetic_under_the_sanitizers(tmp_path):
    """the same shim as a stand-alone program with AddressSanitizer and UBSan: host code, run as it is"""
    exe = tmp_path / "kmer_shim_main"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DKMER_SHIM_MAIN", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", str(exe), str(SHIM_SRC)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and re.fullmatch(r"ok \d+\n", r.stdout), r.stdout[-2000:] + r.stderr[-3000:]
    assert int(r.stdout.split()[1]) > 10_000


# ---------------------------------------------------------------------------------------------------------------------
# sufr kmers
# ---------------------------------------------------------------------------------------------------------------------
def spectrum_text(hist, stats, bins):
    lines = [f"{'>=' + str(bins) if i + 1 == bins else i + 1}\t{int(c)}" for i, c in enumerate(hist) if c]
    lines += [f"# {key}\t{stats[key]}" for key in ("whole", "distinct", "unique", "max_count")]
    return "\n".join(lines) + "\n"


def test_cli_kmers_prints_the_witness_spectrum(tmp_path):
    f = SufrFile(EXP / "1.sufr")
    hist, stats, _, pos = witness_kmers(f, 3, 256)
    want = spectrum_text(hist, stats, 256)
    assert want == "1\t2\n2\t2\n# whole\t6\n# distinct\t4\n# unique\t2\n# max_count\t2\n"      # (ACG, CGT twice; GTN, TNN once)
    occ, uniq = tmp_path / "occ.bin", tmp_path / "uniq.bin"
    assert run("kmers", "-k", 3, "--occ", occ, "--unique", uniq, EXP / "1.sufr").stdout == want
    assert np.array_equal(np.fromfile(occ, dtype="<u4"), pos)
    assert np.array_equal(np.fromfile(uniq, dtype="<u4"), witness_unique(f)[1])
    hist2, stats2, _, _ = witness_kmers(f, 3, 2)
    assert run("km", "-k", 3, "-b", 2, EXP / "1.sufr").stdout == spectrum_text(hist2, stats2, 2) == \
        "1\t2\n>=2\t2\n# whole\t6\n# distinct\t4\n# unique\t2\n# max_count\t2\n"
    g = SufrFile(EXP / "uniprot.sufr")
    hist, stats, _, _ = witness_kmers(g, 4, 256)
    out = tmp_path / "spectrum.tsv"
    assert run("kmers", "-k", 4, "-o", out, EXP / "uniprot.sufr").stdout == ""
    assert out.read_text() == spectrum_text(hist, stats, 256)


def test_cli_kmers_writes_exactly_the_side_files_asked_for(tmp_path):
    f = SufrFile(EXP / "uniprot.sufr")
    hist, stats, occ_want = f.kmers(4, occ="position")
    uniq_want = f.unique_lengths(by_position=True)
    want = spectrum_text(hist, stats, 256)
    for asked in ((), ("occ",), ("unique",)):
        d = tmp_path / ("-".join(asked) or "neither")
        d.mkdir()
        opts = [x for name in asked for x in (f"--{name}", d / name)]
        assert run("kmers", "-k", 4, *opts, EXP / "uniprot.sufr").stdout == want
        assert sorted(p.name for p in d.iterdir()) == sorted(asked)
        if "occ" in asked:
            assert np.array_equal(np.fromfile(d / "occ", dtype="<u4"), occ_want)
        if "unique" in asked:
            assert np.array_equal(np.fromfile(d / "unique", dtype="<u4"), uniq_want)


def test_cli_kmers_errors_and_help():
    r = run("kmers", "-k", 3, EXP / "uniprot-masked.sufr", check=False)
    assert r.returncode == 1 and r.stderr.startswith("Error: ") and "seed mask" in r.stderr
    r = run("kmers", "-k", 0, EXP / "1.sufr", check=False)
    assert r.returncode == 1 and r.stderr.startswith("Error: ")
    assert run("kmers", EXP / "1.sufr", check=False).returncode == 2              # no -k
    assert run("kmers", "-k", 3, check=False).returncode == 2                     # no file
    h = run("--help").stdout
    assert "kmers|km" in h and "little-endian" in h and "--occ" in h and "--unique" in h
