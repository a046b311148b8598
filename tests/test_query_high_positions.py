"""The host query paths at text positions beyond 2^31 and 2^32 (tests/high_positions.py has the construction and the
argument): every operation on a sparse file whose indexed region lies across 2^31, below 2^32 - 2 or across 2^32 must give
what it gives on the 44 KB twin, text positions shifted by the constant between the two.  Every comparison is exact.

Output by position (k-mer counts and unique lengths per text position) has n entries, 17 to 34 GB at these sizes, and is left
out on the host; tests/test_gpu_high_positions.py checks it on the device.

The repeats of the indexed text (include/sufr_repeat.h) have a region and five sequences of their own, in which sequence
starts clip the LCP on both sides of the boundary; tests/test_gpu_repeat_high_positions.py holds the device to the same
witness."""
import subprocess

import pytest

import high_positions as hp
import sufr_amd
from high_positions import GEOMETRIES, LARGE, REPEAT_GEOMETRIES


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
    """`sufr repeats` output: (records, stats lines).  A record is (length, count, [(name, position) ...]) with the shift taken
    off the positions within the first sequence, which begins at 0 and holds the filler, and off nothing else: the other
    sequences begin behind the filler, so the positions within them are printed as the twin's."""
    records, stats = [], []
    for line in stdout.splitlines():
        if line.startswith("#"):
            stats.append(line)
            continue
        length, count, where = line.split("\t")
        places = [w.rsplit(":", 1) for w in where.split(" ")]
        records.append((length, count, [(nm, str(int(x) - shift) if nm == hp.REPEAT_NAMES[0] else x) for nm, x in places]))
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
