"""Repeats of the indexed text on the device at text positions beyond 2^31 and 2^32 (tests/high_positions.py has the
construction, the repeat region and the argument).  The text on the device is one torch.zeros with the repeat region copied to
its end, the suffix array SA(region) + filler, and the five sequence starts lie behind the filler: beyond 2^31 at the two
32-bit geometries, on both sides of 2^32 at the 64-bit one.  The witness is always the host path on the 44 KB twin file, which
is held to the serial stack pass of tests/test_repeat_host.py first; tests/test_query_high_positions.py holds the host to it at
the same geometries.  No case compares the device with itself, every comparison is exact.

Which comparison depends on each read that only the device makes (sufr_repeat.inc, sufr_repeat_scan.h).  Kinds 1 and 2 are
decided by the left symbols alone, and at u64_across_2_32 an offset p - 1 that wraps at 2^32 lands in the filler: the left
symbol of every position above the boundary would read 0x00.  Counted on the twin's arrays, at open filters:
  lam = text[p - 1] of every rank       2 455 of the 20 729 records of kind 1 have all their occurrences above the boundary and
                                        would lose their left diversity: kind 1 of test_repeats_equal_the_twin[u64_across_2_32]
  the reload by lane 0 of a wave        45 intervals that are not left-diverse hold a rank r, r % 64 == 0, whose SA[r-1] lies above
                                        the boundary; a wrapped reload makes them records of kind 1 of the same test
  text[acc.sa(j) - 1] of the walk       2 054 of the 7 459 records of kind 2 have two or more occurrences above the boundary and
                                        would be refused for a repeated byte: kind 2 of the same test
  rep_room, rep_is_start                shared with the host; on the device kind 0 of every large geometry depends on them (the
                                        clipped ranks, the 1200-byte repeat that the positional starts cut)
"""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

import high_positions as hp
import sufr_amd
from high_positions import REPEAT_GEOMETRIES, compare
from sufr_amd import DeviceIndex
from test_gpu_high_positions import _memory_skip, _signed, _unsigned, place, release
from test_query_high_positions import _repeat_lines, sparse_or_skip

pytestmark = pytest.mark.gpu
TILES = (hp.SMALLEST_TILE, 0)                           # 155 tiles of one workgroup's ranks, and the default: 3 tiles
LOADED_FILTERS = ((12, 2, 0), (1, 2, 2))


@pytest.fixture(scope="module")
def ctx():
    c = sufr_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    """the twin file's path and its repeat answers: the witness"""
    path = tmp_path_factory.mktemp("high_positions_repeats_gpu") / "twin.sufr"
    geo = REPEAT_GEOMETRIES["twin"]
    hp.write_repeat_file(path, geo)
    with hp.open_repeat_file(path, geo) as f:
        want, counts = hp.repeat_witness(f)
    return path, want


@pytest.fixture(scope="module")
def u64_file(tmp_path_factory):
    """{name: (path, bytes of disk blocks)} of the sparse u64_across_2_32 repeat file, as sparse_or_skip takes it"""
    path = tmp_path_factory.mktemp("high_positions_repeats_u64") / "u64.sufr"
    return {"u64_across_2_32": (path, hp.write_repeat_file(path, REPEAT_GEOMETRIES["u64_across_2_32"]))}


@pytest.fixture(scope="module", params=list(REPEAT_GEOMETRIES))
def placed(request, ctx):
    geo = REPEAT_GEOMETRIES[request.param]
    try:
        p = place(ctx, geo, tables=(False,), reg=hp.repeat_region())       # repeats never touch the prefix table
    except (torch.OutOfMemoryError, sufr_amd.SufrHipError) as e:
        torch.cuda.empty_cache()
        _memory_skip(f"the {geo.n}-byte text of {geo.name}", e)
    yield p
    release(p)                                                              # the text goes before the next geometry comes


def device_answers(ix, lcp, sa, geo, filters=hp.REPEAT_FILTERS):
    """hp.repeat_answers through repeats_device; the occurrences are read from the suffix array on the device"""
    def call(kind, ml, mc, xc):
        rank, count, length, stats = ix.repeats_device(lcp, kind, ml, mc, xc, geo.seq_starts)
        assert rank.dtype == count.dtype == length.dtype == torch.int64
        return rank.cpu(), count.cpu(), length.cpu(), stats
    occurrences = lambda ranks: _unsigned(sa[torch.from_numpy(ranks).to(sa.device)])
    return hp.repeat_answers(call, geo.shift, occurrences, filters=filters)


def counting_call(ctx, placed, twin):
    """cap == 0 with no arrays: SUFR_HIP_E_CAPACITY, the twin's total and the twin's stats"""
    geo = placed.geo
    torch.cuda.synchronize()
    starts = np.array(geo.seq_starts, dtype=np.uint64)
    for kind in hp.REPEAT_KINDS:
        for ml, mc, xc in LOADED_FILTERS:
            want = twin[1][hp.repeat_key(kind, ml, mc, xc)]
            total, st = C.c_uint64(0), sufr_amd.RepeatStats()
            rc = sufr_amd.lib().sufr_hip_repeats_device(ctx.handle, placed.ix[False]._h, placed.lcp.data_ptr(), starts.ctypes.data, starts.size,
                                                        kind, ml, mc, xc, 0, None, None, None, C.byref(total), C.byref(st))
            assert rc == -5 and total.value == len(want[0]) > 0 and sorted(st.as_dict().items()) == want[3], (geo.name, kind, ml, mc, xc, rc)
    ctx.synchronize()


def test_repeats_equal_the_twin(ctx, placed, twin):
    """every kind and filter at both tile sizes; at u64_across_2_32 the counting call as well, on the same placement"""
    geo, ix = placed.geo, placed.ix[False]
    if geo.name in ("u32_across_2_31", "u32_top"):
        assert int(placed.sa.min()) < 0                                     # positions of 2^31 and more, negative as int32
    if geo.name == "u64_across_2_32":
        assert int(placed.sa.max()) >= 1 << 32 > int(placed.sa.min()) and geo.seq_starts[3] > 1 << 32 > geo.seq_starts[2]
    try:
        for tile in TILES:
            ctx.set_repeat_tile(tile)
            compare(device_answers(ix, placed.lcp, placed.sa, geo), twin[1], f"{geo.name} (tile {tile})")
    finally:
        ctx.set_repeat_tile(0)
    if geo.name == "u64_across_2_32":
        counting_call(ctx, placed, twin)


@pytest.mark.parametrize("name", ["u64_across_2_32"])
def test_a_loaded_sparse_file(ctx, twin, u64_file, name):
    """DeviceIndex.load of the u64_across_2_32 repeat file (the path of `sufr repeats --device 0`), the LCP from the file"""
    geo = REPEAT_GEOMETRIES[name]
    path = sparse_or_skip(u64_file, name)
    with hp.open_repeat_file(path, geo) as f:
        try:
            ix = DeviceIndex.load(ctx, f)
        except sufr_amd.SufrHipError as e:
            _memory_skip(f"the {geo.n}-byte file", e)
        try:
            assert ix.index_width == 8
            lcp = _signed(np.asarray(f.lcp), geo.width).cuda()
            sa = _signed(np.asarray(f.suffix_array), geo.width).cuda()
            assert f.sequence_starts == geo.seq_starts
            compare(device_answers(ix, lcp, sa, geo, LOADED_FILTERS), twin[1], geo.name + " (loaded)",
                    [hp.repeat_key(kind, *flt) for kind in hp.REPEAT_KINDS for flt in LOADED_FILTERS])
        finally:
            ix.close()


def test_cli_repeats_on_the_device_beyond_2_32(twin, u64_file):
    """`sufr repeats --device 0` on the u64_across_2_32 file prints the bytes of the host path on the same file, and the
    twin's once the shift is off the positions within the first sequence.  Only the failed allocation of the index skips
    (the message of sufr_hip_index_load's out-of-memory return); any other exit but 0, a device error included, fails."""
    geo = REPEAT_GEOMETRIES["u64_across_2_32"]
    path = sparse_or_skip(u64_file, geo.name)
    opts = ["repeats", "-l", "12", "--kind", "maximal"]
    cli = lambda *more: subprocess.run([str(sufr_amd.CLI_PATH), *opts, *more], capture_output=True, text=True, timeout=300)
    dev = cli("--device", "0", str(path))
    if dev.returncode != 0 and "hipMalloc of the index (" in dev.stderr:
        pytest.skip(f"not enough free HBM for the {geo.n}-byte file: {dev.stderr.strip()}")
    assert dev.returncode == 0, dev.stderr
    host, small = cli(str(path)), cli(str(twin[0]))
    assert host.returncode == 0 and small.returncode == 0, host.stderr + small.stderr
    assert dev.stdout == host.stdout and dev.stdout.count("\n") > 1000
    assert _repeat_lines(dev.stdout, geo.shift) == _repeat_lines(small.stdout, 0)
    assert f"# records\t{len(twin[1][hp.repeat_key(1, 12, 2, 0)][0])}\n" in dev.stdout
