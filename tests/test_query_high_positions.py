"""The host query paths at text positions beyond 2^31 and 2^32 (tests/high_positions.py has the construction and the
argument): every operation on a sparse file whose indexed region lies across 2^31, below 2^32 - 2 or across 2^32 must give
what it gives on the 44 KB twin, text positions shifted by the constant between the two.  Every comparison is exact.

Output by position (k-mer counts and unique lengths per text position) has n entries, 17 to 34 GB at these sizes, and is left
out on the host; tests/test_gpu_high_positions.py checks it on the device.

The repeats of the indexed text (include/sufr_repeat.h) have a region and five sequences of their own, in which sequence
starts clip the LCP on both sides of the boundary; tests/test_gpu_repeat_high_positions.py holds the device to the same
witness.

The sequence counts and the k-common profile (include/sufr_shared.h) use that region too, on the host and through the CLI.
LPF and the LZ77 parse by position have n entries on the host as well (sufr_file_lpf: 17 to 34 GB; sufr_file_lz: two n-entry
u64 vectors, 69 GB) and are left out; the decision of one rank that the host path and the kernels share (lz_rank of
sufr_lz_scan.h) runs on the shifted arrays through tests/lz_shim.cpp, and tests/test_gpu_lz_shared_high_positions.py holds
the device to the same witness.

The BWT, its runs and LF (include/sufr_bwt.h) have s-sized outputs and run on the three sparse files and through `sufr bwt`.
The FM-index refuses an index that leaves positions out, so its cases index the filler (T = 0x00^F region, whose suffix array
is known without a sort): the two suffix array formulas against a sort at small F, the host pair at F = 4096 against numpy and
the search on text and suffix array, and the host pair at F = 2^20 + 17 against the pair at 4096.  A host build at the large
geometries needs a 17 to 34 GB suffix array in a file that cannot be sparse; tests/test_gpu_fm_high_positions.py builds on the
device and runs the host query code on the downloaded index."""
import subprocess

import numpy as np
import pytest

import high_positions as hp
import sufr_amd
from high_positions import GEOMETRIES, LARGE, REPEAT_GEOMETRIES
from test_lz_host import NONE as LZ_NONE, pyramid, shim  # noqa: F401 (shim: the fixture that builds tests/lz_shim.cpp)


def run(*args):
    """the native CLI; its standard output"""
    r = subprocess.run([str(sufr_amd.CLI_PATH), *map(str, args)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """path and disk bytes of every geometry's file, in one directory that stays below a few MB of blocks"""
    d = tmp_path_factory.mktemp("high_positions")
    out = {name: (d / f"{name}.sufr", hp.write_sparse(d / f"{name}.sufr", geo)) for name, geo in GEOMETRIES.items()}
    yield out


def sparse_or_skip(files, name):
    path, used = files[name]
    if used > hp.SPARSE_LIMIT:
        pytest.skip(f"the filesystem has no holes: {name} takes {used} bytes of blocks for a {GEOMETRIES[name].n}-byte text")
    return path


@pytest.fixture(scope="module")
def witness(files):
    with hp.open_checked(files["twin"][0], GEOMETRIES["twin"]) as f:
        want = hp.answers(f, 0)
    hp.assert_witness_is_not_empty(want)
    return want


def test_the_witness_has_records_on_both_sides_of_and_across_the_boundary(witness):
    """(asserted in the fixture, on the twin's answers alone) and the counts are those of a batch that exercises the paths"""
    sizes = {k: len(v[0]) for k, v in witness.items() if k.split()[0] in ("mems", "approx", "edit")}
    print(sizes)
    assert all(sizes.values()), sizes
    reg = hp.region()
    assert reg.sa.size < hp.R and int(reg.lcp.max()) >= hp.SEG_LEN            # positions left out; the planted repeats


@pytest.mark.parametrize("name", LARGE)
def test_every_host_operation_equals_the_twin(files, witness, name):
    geo = GEOMETRIES[name]
    path = sparse_or_skip(files, name)
    with hp.open_checked(path, geo) as f:
        assert int(f.suffix_array.max()) == geo.n - 1 and int(f.suffix_array.min()) == geo.filler
        hp.compare(hp.answers(f, geo.shift), witness, name)


def test_the_width_rule_flips_at_2_32_minus_1(tmp_path, files):
    """u32 exactly when text_len < 2^32 - 1 (suffix_array.rs:460-470): the largest 32-bit text and, header only, the first
    64-bit one"""
    top = GEOMETRIES["u32_top"]
    assert top.n + 1 == hp.WIDTH_FLIP.n == 0xFFFFFFFF
    used = hp.write_sparse(tmp_path / "flip.sufr", hp.WIDTH_FLIP, indexed=False)
    if used > hp.SPARSE_LIMIT:
        pytest.skip(f"the filesystem has no holes: {used} bytes of blocks for a header")
    with hp.open_checked(tmp_path / "flip.sufr", hp.WIDTH_FLIP, indexed=False) as f:
        assert f.index_width == 8 and f.metadata().text_len == 0xFFFFFFFF
    with hp.open_checked(sparse_or_skip(files, "u32_top"), top) as f:
        assert f.index_width == 4 and f.metadata().text_len == 0xFFFFFFFE


def _shifted(stdout: str, shift: int):
    """`sufr locate --abs` lines (query, then absolute positions) with the shift taken off the positions"""
    return [[w[0]] + [int(x) - shift for x in w[1:]] for w in (line.split() for line in stdout.splitlines())]


def test_cli_locate_and_count_beyond_2_32(files):
    geo = GEOMETRIES["u64_across_2_32"]
    path = sparse_or_skip(files, geo.name)
    text = hp.region().text.tobytes()
    queries = [text[hp.MID - 9:hp.MID + 9].decode(), "A" * 30, text[hp.SEG_AT[0]:hp.SEG_AT[0] + 40].decode(), text[-13:-1].decode(), "ACGTAC"]
    got, want = (run("locate", "--abs", p, *queries).stdout for p in (path, files["twin"][0]))
    assert _shifted(got, geo.shift) == _shifted(want, 0) and want
    positions = [x for w in _shifted(want, 0) for x in w[1:]]
    assert min(positions) < GEOMETRIES["twin"].boundary < max(positions)
    assert max(int(x) for line in got.splitlines() for x in line.split()[1:]) > 1 << 32
    # by sequence: the names and the positions within the second and third sequence are the twin's
    got, want = (run("locate", p, *queries).stdout for p in (path, files["twin"][0]))
    keep = lambda s: [line for line in s.splitlines() if not line.startswith(hp.SEQ_NAMES[0] + " ")]
    assert keep(got) == keep(want) and any(line.startswith(hp.SEQ_NAMES[2] + " ") for line in keep(want))
    assert run("count", path, *queries).stdout == run("count", files["twin"][0], *queries).stdout != ""


# ---------------------------------------------------------------------------------------------------------------------
# repeats: the region with clipped ranks, five sequences
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def repeat_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("high_positions_repeats")
    return {name: (d / f"{name}.sufr", hp.write_repeat_file(d / f"{name}.sufr", geo)) for name, geo in REPEAT_GEOMETRIES.items()}


@pytest.fixture(scope="module")
def repeat_witness(repeat_files):
    """the twin's answers, held to the serial witness of tests/test_repeat_host.py and shown not to be empty, and the counts"""
    with hp.open_repeat_file(repeat_files["twin"][0], REPEAT_GEOMETRIES["twin"]) as f:
        return hp.repeat_witness(f)


def test_the_repeat_witness_equals_the_serial_pass_and_has_clipped_ranks_on_both_sides(repeat_witness, files):
    """(asserted in the fixture, from the twin alone)  The counts of the committed region are pinned, so that the region
    cannot drift unseen: the clip decides 1540 ranks, from the side below the boundary, from the side above it and with equal
    rooms; the plain region has none"""
    want, counts = repeat_witness
    print(counts)
    assert counts == {"records kind=0": 25113, "records kind=1": 20729, "records kind=2": 7459, "clipped ranks": 1540, "equal rooms": 30,
                      "the smaller room below the boundary": 1200, "the smaller room above the boundary": 310,
                      "the smaller room below the boundary, the other position above": 600,
                      "the smaller room above the boundary, the other position below": 305,
                      "pairs that straddle the boundary": 935, "sequence starts among the left symbols": 4}
    with hp.open_checked(files["twin"][0], GEOMETRIES["twin"]) as f:
        assert hp.clipped_ranks(f)[0].size == 0                      # why the plain region could not serve
    assert all(hp.repeat_key(kind, *flt) in want for kind in hp.REPEAT_KINDS for flt in hp.REPEAT_FILTERS) and len(want) == 18
    reg, rep = hp.region(), hp.repeat_region()
    assert rep.sa.size == reg.sa.size and (rep.text != reg.text).sum() <= 2 * hp.COPY and rep.text[hp.DELIMS[1]] == ord("%")


@pytest.mark.parametrize("name", LARGE)
def test_host_repeats_equal_the_twin(repeat_files, repeat_witness, name):
    geo = REPEAT_GEOMETRIES[name]
    path = sparse_or_skip(repeat_files, name)
    with hp.open_repeat_file(path, geo) as f:
        assert int(f.suffix_array.max()) == geo.n - 1 and int(f.suffix_array.min()) == geo.filler
        assert f.sequence_starts[1] > geo.filler and (name != "u64_across_2_32" or f.sequence_starts[3] > 1 << 32 > f.sequence_starts[2])
        for threads in (1, 0):
            hp.compare(hp.repeat_answers(f, geo.shift, threads=threads), repeat_witness[0], f"{name} (threads={threads})")


def _repeat_lines(stdout: str, shift: int):
    """`sufr repeats` and `sufr shared` output: (records, stats lines).  A record is (length, count, [(name, position) ...]),
    of `sufr shared` (length, count, seqs, [(name, position) ...]), with the shift taken
    off the positions within the first sequence, which begins at 0 and holds the filler, and off nothing else: the other
    sequences begin behind the filler, so the positions within them are printed as the twin's."""
    records, stats = [], []
    for line in stdout.splitlines():
        if line.startswith("#"):
            stats.append(line)
            continue
        *columns, where = line.split("\t")                            # (`sufr shared` has a third column, seqs, before the places)
        places = [w.rsplit(":", 1) for w in where.split(" ")]
        records.append((*columns, [(nm, str(int(x) - shift) if nm == hp.REPEAT_NAMES[0] else x) for nm, x in places]))
    return records, stats


REPEAT_CLI = (("-l", 12, "--kind", "maximal"), ("-l", 1, "--kind", "super", "-c", 3, "--max-positions", 0))


def test_cli_repeats_beyond_2_32(repeat_files):
    """The first sequence ends 3 600 bytes into the region, 16 400 below 2^32, so no position printed within it can exceed
    2^32 at this geometry; what lies beyond 2^32 are the fourth and fifth sequence.  Their records are found, named and
    placed from absolute positions of 2^32 and more, and must be printed byte for byte as the twin's; the positions within
    the first sequence are all beyond 2^32 - 20 000 and equal the twin's once the shift is off."""
    geo = REPEAT_GEOMETRIES["u64_across_2_32"]
    path = sparse_or_skip(repeat_files, geo.name)
    starts = dict(zip(hp.REPEAT_NAMES, geo.seq_starts))
    for opts in REPEAT_CLI:
        got, want = run("repeats", *opts, path).stdout, run("repeats", *opts, repeat_files["twin"][0]).stdout
        (g_rec, g_stats), (w_rec, w_stats) = _repeat_lines(got, geo.shift), _repeat_lines(want, 0)
        assert g_stats == w_stats and len(w_stats) == 4 and g_rec == w_rec and w_rec, opts
        printed = [(nm, int(x)) for _, _, places in _repeat_lines(got, 0)[0] for nm, x in places]
        first = [x for nm, x in printed if nm == hp.REPEAT_NAMES[0]]
        assert first and min(first) >= geo.filler == (1 << 32) - hp.MID and max(first) < starts["s1"]
        # the witness holds occurrences in every sequence, those that begin beyond 2^32 included.  (This line is decided by the
        # twin's records and the test's own starts: it keeps the comparison from being empty.  What fails for an error of the
        # library at such a position is the equality with the twin, above and below: a position of 2^32 and more that is
        # truncated lands in the filler and is printed within the first sequence.)
        assert max(starts[nm] + x for nm, x in printed) > 1 << 32 and {nm for nm, _ in printed} == set(hp.REPEAT_NAMES), opts
        # the other four sequences: byte-equal as printed
        keep = lambda s: [[w for w in line.split("\t")[2].split(" ") if not w.startswith(hp.REPEAT_NAMES[0] + ":")]
                          for line in s.splitlines() if not line.startswith("#")]
        assert keep(got) == keep(want)


# ---------------------------------------------------------------------------------------------------------------------
# sequence counts, the k-common profile, longest previous factors and the LZ77 parse: the repeat region again
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lz_shared_witness(repeat_files, repeat_witness):
    """(shared answers, LZ answers, counts) of the twin, each held to what reads only the arrays or only the text"""
    with hp.open_repeat_file(repeat_files["twin"][0], REPEAT_GEOMETRIES["twin"]) as f:
        shared = hp.shared_witness(f, repeat_witness[0])
        lz = hp.lz_witness(f)
        return shared, lz, hp.assert_lz_shared_witness_is_not_empty(f, lz, shared)


def test_the_lz_and_shared_witness_is_held_to_the_arrays_and_the_text_and_its_counts_are_pinned(lz_shared_witness):
    """(asserted in the fixture, from the twin alone)  The counts of the committed region are pinned, so that the region
    cannot drift unseen: LPF has targets and sources on either side of the boundary and spans over it, self-overlapping
    copies and positions that the clip decides on both sides; the one factor that spans the boundary byte is the longest;
    every value of seqs occurs, and 12 123 records of kind 0 would change their seqs if a position from the boundary on read
    as sequence 0, which is what a position of 2^32 and more truncated to 32 bits does at u64_across_2_32"""
    shared, lz, counts = lz_shared_witness
    print(counts)
    assert counts == {
        "lpf nonzero": 39591, "lpf nonzero in the filler": 0, "lpf max": 1200,
        "lpf above the boundary, source below": 13854, "lpf and source above the boundary": 5742, "lpf and source below the boundary": 19994,
        "lpf targets that span the boundary byte": 601, "lpf sources that span the boundary byte": 4, "lpf self-overlapping copies": 1020,
        "lpf decided by the clip": 950, "lpf decided by the clip above the boundary": 937, "lpf decided by the clip below the boundary": 13,
        "lz factors": 9934, "lz literals of the filler": 4096, "lz literals": 4505, "lz longest": 1197, "lz longest_start": 23499,
        "lz factors that span the boundary byte": 1, "lz copies that start below the boundary": 2987, "lz copies that start above the boundary": 2442,
        "shared kind=0 records with seqs=1": 4775, "shared kind=0 records with seqs=2": 11326, "shared kind=0 records with seqs=3": 4738,
        "shared kind=0 records with seqs=4": 2361, "shared kind=0 records with seqs=5": 1913, "shared kind=0 records with 1 < seqs < count": 12182,
        "shared kind=0 records whose seqs changes if positions from the boundary on read as sequence 0": 12123}
    sizes = [[len(shared[hp.shared_key(kind, *flt)][0]) for kind in hp.REPEAT_KINDS] for flt in hp.SHARED_FILTERS]
    assert sizes == [[25113, 20729, 7459], [1531, 25, 21], [980, 980, 0], [1913, 1913, 0], [1008, 628, 41]]
    assert shared["common"] == [1000, 600, 300, 10, 8] and len(shared) == 16
    # every factor is a literal or a copy that starts on one side of the boundary (none starts at the boundary byte)
    assert counts["lz copies that start below the boundary"] + counts["lz copies that start above the boundary"] == counts["lz factors"] - counts["lz literals"]
    assert REPEAT_GEOMETRIES["twin"].boundary == 24096 and len(hp.lz_sample()) > 1500


@pytest.mark.parametrize("name", LARGE)
def test_host_shared_and_common_equal_the_twin(repeat_files, lz_shared_witness, name):
    geo = REPEAT_GEOMETRIES[name]
    path = sparse_or_skip(repeat_files, name)
    with hp.open_repeat_file(path, geo) as f:
        assert int(f.suffix_array.max()) == geo.n - 1 and int(f.suffix_array.min()) == geo.filler
        assert f.sequence_starts[1] > geo.filler and (name != "u64_across_2_32" or f.sequence_starts[3] > 1 << 32 > f.sequence_starts[2])
        for threads in (1, 0):
            hp.compare(hp.shared_answers(f, geo.shift, threads=threads), lz_shared_witness[0], f"{name} (threads={threads})")


SHARED_CLI = (("-l", 12, "--kind", "maximal", "-q", 2), ("-l", 1, "--kind", "super", "-c", 3, "--max-positions", 0))


def test_cli_shared_beyond_2_32(repeat_files):
    """`sufr shared` on the u64_across_2_32 file against the twin, as test_cli_repeats_beyond_2_32 reads `sufr repeats`: the
    seqs column is found from absolute positions on both sides of 2^32 and must be the twin's; a position of 2^32 and more
    that is truncated lands in the filler, is counted for the first sequence and printed within it.  The profile of
    `--common` has no position at all: byte for byte the twin's."""
    geo = REPEAT_GEOMETRIES["u64_across_2_32"]
    path = sparse_or_skip(repeat_files, geo.name)
    starts = dict(zip(hp.REPEAT_NAMES, geo.seq_starts))
    for opts in SHARED_CLI:
        got, want = run("shared", *opts, path).stdout, run("shared", *opts, repeat_files["twin"][0]).stdout
        (g_rec, g_stats), (w_rec, w_stats) = _repeat_lines(got, geo.shift), _repeat_lines(want, 0)
        assert g_stats == w_stats and len(w_stats) == 5 and g_rec == w_rec and w_rec and all(len(rec) == 4 for rec in w_rec), opts
        assert {int(rec[2]) for rec in w_rec} >= {2, 3}, opts                       # records in two and in three sequences
        printed = [(nm, int(x)) for *_, places in _repeat_lines(got, 0)[0] for nm, x in places]
        first = [x for nm, x in printed if nm == hp.REPEAT_NAMES[0]]
        assert first and min(first) >= geo.filler == (1 << 32) - hp.MID and max(first) < starts["s1"]
        # (decided by the twin's records and the test's own starts: what keeps the comparison from being empty)
        assert max(starts[nm] + x for nm, x in printed) > 1 << 32 and {nm for nm, _ in printed} == set(hp.REPEAT_NAMES), opts
        keep = lambda s: [[w for w in line.split("\t")[3].split(" ") if not w.startswith(hp.REPEAT_NAMES[0] + ":")]
                          for line in s.splitlines() if not line.startswith("#")]
        assert keep(got) == keep(want)
    got, want = run("shared", "--common", path).stdout, run("shared", "--common", repeat_files["twin"][0]).stdout
    assert got == want == "1\t1000\n2\t600\n3\t300\n4\t10\n5\t8\n"


@pytest.mark.parametrize("name", LARGE)
def test_lpf_rank_decisions_at_shifted_positions(shim, repeat_files, lz_shared_witness, name):
    """lz_rank of sufr_lz_scan.h -- the arithmetic the host path and the kernels share -- on SA(region) + filler through
    tests/lz_shim.cpp: the min pyramid over the suffix array's values, the two searches by value (SA[j] <= p - 1, SA[j] < p),
    the two range minima and the clip by rooms computed here from the geometry's sequence starts.  No n-entry array is
    needed, so this holds at every large geometry; LPF by rank is the twin's, SRC the twin's plus the shift.  At the two
    32-bit geometries once more with the pyramid's entries narrowed to uint32 and widened again, which is what the device
    stores: a later failure of the device test is then not one of this arithmetic."""
    geo, twin = REPEAT_GEOMETRIES[name], REPEAT_GEOMETRIES["twin"]
    reg = hp.repeat_region()
    sa = np.ascontiguousarray(reg.sa + np.uint64(geo.filler))
    lcp = np.ascontiguousarray(reg.lcp)
    breaks = np.array(sorted({geo.n - 1} | {s - 1 for s in geo.seq_starts[1:]}), dtype=np.uint64)
    room = np.ascontiguousarray(breaks[np.searchsorted(breaks, sa, side="left")] - sa)
    assert int(sa.max()) == geo.n - 1 and int(room.min()) == 0 and int(room.max()) < hp.R
    lpf_twin = np.array(lz_shared_witness[1]["lpf of the twin"], dtype=np.int64)
    src_twin = np.array(lz_shared_witness[1]["src of the twin"], dtype=np.int64)
    at = (reg.sa + np.uint64(twin.filler)).astype(np.int64)
    want_lpf, want_src = lpf_twin[at], np.where(src_twin[at] < 0, -1, src_twin[at] + geo.shift)
    assert (want_lpf > 0).sum() == 39591 and (want_src >= geo.boundary).any() and ((want_src >= 0) & (want_src < geo.boundary)).any()
    up_sa, up_lcp = pyramid(shim, sa), pyramid(shim, lcp)
    narrowed = [up_sa] + ([up_sa.astype(np.uint32).astype(np.uint64)] if geo.width == 4 else [])
    for up in narrowed:
        lpf, src = np.zeros(sa.size, dtype=np.uint64), np.zeros(sa.size, dtype=np.uint64)
        shim.shim_lz_rank_all(sa.ctypes.data, up.ctypes.data, lcp.ctypes.data, up_lcp.ctypes.data, sa.size, room.ctypes.data, lpf.ctypes.data, src.ctypes.data)
        assert np.array_equal(lpf.astype(np.int64), want_lpf), name
        assert np.array_equal(np.where(src == LZ_NONE, -1, src.astype(np.int64)), want_src), name


# ---------------------------------------------------------------------------------------------------------------------
# the BWT, its runs and LF (include/sufr_bwt.h): the plain region, s-sized outputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bwt_witness(files):
    """the twin's BWT answers, held to numpy on the arrays and shown not to be empty, and the counts"""
    with hp.open_checked(files["twin"][0], GEOMETRIES["twin"]) as f:
        return hp.bwt_witness(f)


def test_the_bwt_witness_equals_numpy_and_its_counts_are_pinned(bwt_witness):
    """(asserted in the fixture, from the twin alone)  The counts of the committed region are pinned."""
    want, counts = bwt_witness
    print(counts)
    assert counts["bwt bytes 0x00"] == 1 and counts["bwt bytes %"] == 2 and counts["bwt bytes N"] == 1
    assert min(v for k, v in counts.items() if k.startswith("runs min_len=1")) > 10_000
    assert min(v for k, v in counts.items() if k.startswith("runs min_len=8")) >= 1
    assert len(want["lf"]) == hp.region().sa.size and sorted(want["lf"]) != want["lf"]


@pytest.mark.parametrize("name", LARGE)
def test_host_bwt_runs_and_lf_equal_the_twin(files, bwt_witness, name):
    """BWT[r] = T[SA[r] - 1] and first = SA[a] at positions that are negative as int32 or beyond 2^32; everything but `first`
    is the twin's"""
    geo = GEOMETRIES[name]
    path = sparse_or_skip(files, name)
    with hp.open_checked(path, geo) as f:
        for threads in (1, 0):
            hp.compare(hp.host_bwt_answers(f, geo.shift, threads), bwt_witness[0], f"{name} (threads={threads})")


def _bwt_lines(stdout: str, shift: int):
    """`sufr bwt --runs` output: (count lines and # lines, run records).  A record is (rank, length, symbol, name, position),
    the shift taken off the positions within the first sequence, which holds the filler (see _repeat_lines)."""
    other, records = [], []
    for line in stdout.splitlines():
        w = line.split("\t")
        if len(w) == 4:
            nm, x = w[3].rsplit(":", 1)
            records.append((w[0], w[1], w[2], nm, int(x) - shift if nm == hp.SEQ_NAMES[0] else int(x)))
        else:
            other.append(line)
    return other, records


def test_cli_bwt_runs_beyond_2_32(files):
    geo = GEOMETRIES["u64_across_2_32"]
    path = sparse_or_skip(files, geo.name)
    starts = dict(zip(hp.SEQ_NAMES, geo.seq_starts))
    for opts in (("--runs",), ("--runs", "--min-len", 8)):
        got, want = run("bwt", *opts, path).stdout, run("bwt", *opts, files["twin"][0]).stdout
        (g_other, g_rec), (w_other, w_rec) = _bwt_lines(got, geo.shift), _bwt_lines(want, 0)
        assert g_other == w_other and len(w_other) > 4 and g_rec == w_rec and w_rec, opts
        absolute = [starts[nm] + x for _, _, _, nm, x in _bwt_lines(got, 0)[1]]
        assert min(absolute) < 1 << 32 < max(absolute), opts                    # records first seen on both sides of 2^32
        assert {r[3] for r in w_rec} == set(hp.SEQ_NAMES) or len(opts) > 1
    assert run("bwt", path).stdout == run("bwt", files["twin"][0]).stdout != ""


# ---------------------------------------------------------------------------------------------------------------------
# the FM-index: the filler indexed, T = 0x00^F region (the construction: tests/high_positions.py)
# ---------------------------------------------------------------------------------------------------------------------
FM_BIG_FILLER = (1 << 20) + 17          # the region at odd places in blocks, mark words and tiles


@pytest.mark.parametrize("F", [1, 7, 500])
def test_the_suffix_array_formulas_equal_a_sort(F):
    """SA(0^F region) and SA(its reversal) as the helper writes them down, against the order of the suffixes themselves"""
    for symbols in (8, 9):
        text, sa, rtext, rsa = hp.full_arrays_host(F, symbols)
        hp.check_suffix_order(text.tobytes(), sa)
        hp.check_suffix_order(rtext.tobytes(), rsa)


@pytest.fixture(scope="module", params=[8, 9], ids=["8_symbols", "9_symbols"])
def fm_twin(request, tmp_path_factory):
    """the host pair on the twin, its files and its answers (the witness), shown not to be empty"""
    from types import SimpleNamespace
    symbols = request.param
    d = tmp_path_factory.mktemp("fm_high_positions")
    fwd, rev, f, g = hp.full_host_pair(d, hp.TWIN_FILLER, symbols)
    fwd.pair_check(rev)
    want = hp.fm_answers(fwd, rev, 0, hp.TWIN_FILLER, symbols)
    counts = hp.assert_fm_witness_is_not_empty(want, symbols)
    return SimpleNamespace(symbols=symbols, dir=d, fwd=fwd, rev=rev, f=f, g=g, want=want, counts=counts)


def test_the_fm_witness_is_held_to_the_arrays_and_is_not_empty(fm_twin):
    """the twin's search and locate against the numpy backward search of tests/test_fm_host.py, its matching statistics against
    the search on text and suffix array of the same file; the counts of assert_fm_witness_is_not_empty are printed"""
    from test_fm_host import Witness
    print(fm_twin.symbols, fm_twin.counts)
    info = fm_twin.fwd.info
    assert info["symbols"] == fm_twin.symbols and info["width"] == 4 and info["samples"] == -(-info["ranks"] // hp.FM_SAMPLE)
    assert (info["block"], info["stride"]) == ((96, 128) if fm_twin.symbols == 8 else (64, 128))
    w = Witness(np.asarray(fm_twin.f.text), np.asarray(fm_twin.f.suffix_array))
    queries = list(hp.fm_batch(fm_twin.symbols)[0])
    lo, hi = fm_twin.fwd.search_batch(queries)
    got = [w.search(q)[:2] for q in queries]
    assert [g[0] for g in got] == lo.tolist() and [g[1] for g in got] == hi.tolist()
    empty = queries.index(b"")
    lo[empty] = hi[empty] = 0
    off, pos = fm_twin.fwd.locate_ranges(lo, hi)
    assert np.array_equal(pos, np.concatenate([w.sa[int(a):int(b)] for a, b in zip(lo, hi)]))
    assert pos.tolist() == fm_twin.want["locate max_hits=0"][1]
    # (the pair matches in the text without its end byte, include/sufr_fm_match.h: the four queries that hold a $ are left out)
    ms = fm_twin.f.matching_statistics(queries)
    bounds = np.concatenate([[0], np.cumsum([len(q) for q in queries])])
    plain = [i for i, q in enumerate(queries) if b"$" not in q]
    assert len(plain) == len(queries) - 4
    for i in plain:
        assert ms[i].astype(np.int64).tolist() == fm_twin.want["matching statistics"][bounds[i]:bounds[i + 1]], i


def test_the_host_pair_at_an_odd_filler_equals_the_twin(fm_twin):
    F = FM_BIG_FILLER
    for threads in (1, 0):
        fwd, rev, f, g = hp.full_host_pair(fm_twin.dir, F, fm_twin.symbols, threads=threads)
        fwd.pair_check(rev)
        hp.compare(hp.fm_answers(fwd, rev, F - hp.TWIN_FILLER, F, fm_twin.symbols, threads=threads), fm_twin.want, f"F = {F} (threads={threads})")
        # the run records and LF of the full index: analytic in the filler, the twin's behind it
        rank, length, symbol, first, st = f.bwt_runs(1, threads)
        t_rank, t_length, t_symbol, t_first, t_st = fm_twin.f.bwt_runs(1)
        assert (rank[:2].tolist(), length[:2].tolist(), symbol[:2].tolist(), first[:2].tolist()) == ([0, 1], [1, F - 1], [36, 0], [0, 1])
        shift = F - hp.TWIN_FILLER
        assert np.array_equal(rank[2:] - shift, t_rank[2:]) and np.array_equal(first[2:] - shift, t_first[2:])
        assert np.array_equal(length[2:], t_length[2:]) and np.array_equal(symbol[2:], t_symbol[2:])
        assert st == dict(t_st, longest=F - 1) and st["longest_rank"] == 1
        lf, t_lf = f.lf(threads).astype(np.int64), fm_twin.f.lf().astype(np.int64)
        assert lf[0] == F and np.array_equal(lf[1:F], np.arange(F - 1)) and np.array_equal(lf[F:] - shift, t_lf[hp.TWIN_FILLER:])
        for x in (fwd, rev, f, g):
            x.close()
