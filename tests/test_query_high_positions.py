"""The host query paths at text positions beyond 2^31 and 2^32 (tests/high_positions.py has the construction and the
argument): every operation on a sparse file whose indexed region lies across 2^31, below 2^32 - 2 or across 2^32 must give
what it gives on the 44 KB twin, text positions shifted by the constant between the two.  Every comparison is exact.

Output by position (k-mer counts and unique lengths per text position) has n entries, 17 to 34 GB at these sizes, and is left
out on the host; tests/test_gpu_high_positions.py checks it on the device."""
import subprocess

import pytest

import high_positions as hp
import sufr_amd
from high_positions import GEOMETRIES, LARGE


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
