"""Longest previous factors, the LZ77 parse, sequence counts and the k-common profile on the device at text positions beyond
2^31 and 2^32 (tests/high_positions.py has the construction, the repeat region and the argument).  The text on the device
is one torch.zeros with the repeat region copied to its end, the suffix array SA(region) + filler, and the five sequence
starts lie behind the filler: beyond 2^31 at the two 32-bit geometries, on both sides of 2^32 at the 64-bit one.  The witness
is always the host path on the 44 KB twin file, which is first held to what reads nothing of the library but the arrays
(shared_witness: the serial stack pass, len(set(docs))) or the text (lz_witness: witness_lpf_at, check_parse);
tests/test_query_high_positions.py holds the host's shared records and the rank decision of sufr_lz_scan.h to it at the same
geometries.  No case compares the device with itself, every comparison is exact.

Which comparison depends on each read that only the device makes (sufr_lz.inc, sufr_shared.inc), with its count from the
twin's arrays (B is the boundary: 2^31 or 2^32 at the large geometries):
  the SA-value pyramid and its pad      k_lz_fold stores min SA[64 i ..) at the index width and pads the last block with all ones.
                                        Every one of the 39 591 nonzero LPF entries is found by two searches over it (SA[j] < p):
                                        a signed compare at 2^31 turns the 13 854 entries above B with a source below it around,
                                        a pad that is not the largest value ends the searches of the last block at u32_top early:
                                        test_lpf_and_src_by_position, every large geometry
  the p - 1 of the left search          SA[j] <= p - 1 at p = B wraps in 32 bits; 5 742 entries have target and source above B,
                                        19 994 both below, and 601 targets and 4 sources span B: the same test
  the scatter index lpf[p], src[p]      n entries by position: an index truncated to 32 bits at u64_across_2_32 writes the 19 597
                                        entries above B into the filler, which the test reads whole: all 0 / all ones there
  rep_room at p >= 2^32                 950 entries are decided by the clip (lpf == d(p) > 0), 937 of them above B, by sequence
                                        starts on either side of 2^32: the same test
  base + i in k_lz_table / k_lz_emit    the parse walks n positions in tiles; its one factor over B is the longest (1 197 at
                                        B - 597) and 2 442 copies start above B, 2 987 below: total, literals, longest and
                                        longest_start of test_lz_totals_and_stats, where a 32-bit base + i or pos wraps the walk
                                        into the filler's literals
  shr_doc of SA[r]                      a position of 2^32 and more truncated to 32 bits reads as sequence 0: the seqs column of
                                        12 123 of the 25 113 records of kind 0 changes, and with it every filter on seqs and the
                                        profile: test_shared_equals_the_twin[u64_across_2_32]
"""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

import high_positions as hp
import sufr_amd
from high_positions import REPEAT_GEOMETRIES, _ints, compare
from sufr_amd import DeviceIndex
from test_gpu_high_positions import _all_zero, _memory_skip, _signed, _unsigned, place, release
from test_query_high_positions import _repeat_lines, sparse_or_skip

pytestmark = pytest.mark.gpu
TILES = (hp.SMALLEST_TILE, 0)                           # ranks: 155 tiles of one workgroup's ranks, and the default: 3 tiles
FEWER_FILTERS = (hp.SHARED_FILTERS[1], hp.SHARED_FILTERS[4])      # the counting call and the loaded file: a filter on seqs from below, one from both sides
LZ_CAP = 1000


@pytest.fixture(scope="module")
def ctx():
    c = sufr_amd.Context(0)
    yield c
    c.set_repeat_tile(0)
    c.set_lz_tile(0, 0)
    c.close()


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    """the twin file's path, its shared answers and its LZ answers: the witness"""
    path = tmp_path_factory.mktemp("high_positions_lz_shared_gpu") / "twin.sufr"
    geo = REPEAT_GEOMETRIES["twin"]
    hp.write_repeat_file(path, geo)
    with hp.open_repeat_file(path, geo) as f:
        shared = hp.shared_witness(f)
        lz = hp.lz_witness(f)
        hp.assert_lz_shared_witness_is_not_empty(f, lz, shared)
    return path, shared, lz


@pytest.fixture(scope="module")
def u64_file(tmp_path_factory):
    """{name: (path, bytes of disk blocks)} of the sparse u64_across_2_32 repeat file, as sparse_or_skip takes it"""
    path = tmp_path_factory.mktemp("high_positions_lz_shared_u64") / "u64.sufr"
    return {"u64_across_2_32": (path, hp.write_repeat_file(path, REPEAT_GEOMETRIES["u64_across_2_32"]))}


@pytest.fixture(scope="module", params=list(REPEAT_GEOMETRIES))
def placed(request, ctx):
    geo = REPEAT_GEOMETRIES[request.param]
    try:
        p = place(ctx, geo, tables=(False,), reg=hp.repeat_region())       # none of these analyses touches the prefix table
    except (torch.OutOfMemoryError, sufr_amd.SufrHipError) as e:
        torch.cuda.empty_cache()
        _memory_skip(f"the {geo.n}-byte text of {geo.name}", e)
    yield p
    release(p)                                                              # the text goes before the next geometry comes


def device_answers(ix, lcp, sa, geo, filters=hp.SHARED_FILTERS):
    """hp.shared_answers through shared_device and common_device; the occurrences are read from the suffix array on the device"""
    def call(kind, *flt):
        rank, count, length, seqs, stats = ix.shared_device(lcp, kind, *flt, geo.seq_starts)
        assert rank.dtype == count.dtype == length.dtype == seqs.dtype == torch.int64
        return rank.cpu(), count.cpu(), length.cpu(), seqs.cpu(), stats
    occurrences = lambda ranks: _unsigned(sa[torch.from_numpy(ranks).to(sa.device)])
    common = lambda: ix.common_device(lcp, geo.seq_starts).cpu()
    return hp.shared_answers(call, geo.shift, occurrences, common, filters=filters)


def shared_keys(filters):
    return [hp.shared_key(kind, *flt) for kind in hp.REPEAT_KINDS for flt in filters] + ["common"]


def shared_counting_call(ctx, placed, twin):
    """cap == 0 with no arrays: SUFR_HIP_E_CAPACITY, the twin's total and the twin's stats"""
    geo = placed.geo
    torch.cuda.synchronize()
    starts = np.array(geo.seq_starts, dtype=np.uint64)
    for kind in hp.REPEAT_KINDS:
        for flt in FEWER_FILTERS:
            want = twin[1][hp.shared_key(kind, *flt)]
            total, st = C.c_uint64(0), sufr_amd.SharedStats()
            rc = sufr_amd.lib().sufr_hip_shared_device(ctx.handle, placed.ix[False]._h, placed.lcp.data_ptr(), starts.ctypes.data, starts.size,
                                                       kind, *flt, 0, None, None, None, None, C.byref(total), C.byref(st))
            assert rc == -5 and total.value == len(want[0]) > 0 and sorted(st.as_dict().items()) == want[4], (geo.name, kind, flt, rc)
    ctx.synchronize()


def test_shared_equals_the_twin(ctx, placed, twin):
    """every kind and filter and the profile at both tile sizes; at u64_across_2_32 the counting call as well"""
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
        shared_counting_call(ctx, placed, twin)


def _all_ones(t: torch.Tensor) -> bool:
    step = 1 << 30
    return all(int(torch.count_nonzero(t[a:a + step] != -1)) == 0 for a in range(0, t.numel(), step))


def _one_array(ctx, placed, which: str):
    """sufr_hip_lpf_device with one output: the n entries of LPF ("lpf") or of SRC ("src") as a tensor of the index width"""
    geo = placed.geo
    starts = np.array(geo.seq_starts, dtype=np.uint64)
    try:
        out = torch.empty(geo.n, dtype=placed.lcp.dtype, device="cuda")
        torch.cuda.synchronize()
        ctx.check(sufr_amd.lib().sufr_hip_lpf_device(ctx.handle, placed.ix[False]._h, placed.lcp.data_ptr(), starts.ctypes.data, starts.size,
                                                     out.data_ptr() if which == "lpf" else None, out.data_ptr() if which == "src" else None))
        ctx.synchronize()
    except (torch.OutOfMemoryError, sufr_amd.SufrHipError) as e:
        out = None
        torch.cuda.empty_cache()
        _memory_skip(f"{geo.n} entries of {geo.width} bytes by position at {geo.name}", e)
    return out


def test_lpf_and_src_by_position(ctx, placed, twin):
    """The outputs have n entries of the index's width, so one of them is alive at a time (17 GB at u32_top, 34 GB at
    u64_across_2_32): the entries of the region are the twin's (SRC minus the shift, no source stays all ones of the width),
    the filler's are all 0 for LPF and all ones for SRC.  The rank tile at 256 and at its default."""
    geo = placed.geo
    want = {key: twin[2][key] for key in ("lpf of the region", "src of the region")}
    assert sum(1 for x in want["lpf of the region"] if x) == 39591 and max(want["src of the region"]) > REPEAT_GEOMETRIES["twin"].boundary
    try:
        for tile in TILES:
            ctx.set_lz_tile(tile, 0)
            region = {}
            for which, filler_is in (("lpf", _all_zero), ("src", _all_ones)):
                out = _one_array(ctx, placed, which)
                assert out.numel() == geo.n and out.dtype == placed.sa.dtype
                region[which] = out[geo.filler:].cpu()
                assert filler_is(out[:geo.filler]), f"{which} at {geo.name} (tile {tile}): an entry of the filler is not {'0' if which == 'lpf' else 'all ones'}"
                del out
                torch.cuda.empty_cache()                                    # (the next output takes its place)
            compare(hp.lz_answers_by_rank(region["lpf"], region["src"], geo.shift), want, f"{geo.name} (rank tile {tile})")
    finally:
        ctx.set_lz_tile(0, 0)
    if geo.name == "twin":                                                  # the wrapper: both arrays at once, of the index's dtype, every entry
        lpf, src = placed.ix[False].lpf_device(placed.lcp, geo.seq_starts)
        assert lpf.dtype == src.dtype == torch.int32
        assert _ints(_unsigned(lpf)) == twin[2]["lpf of the twin"]
        assert np.where(_unsigned(src) == 0xFFFFFFFF, -1, _unsigned(src)).tolist() == twin[2]["src of the twin"]


def test_lz_totals_and_stats(placed, twin):
    """The totals and the stats of the parse: every filler position is a literal, so factors and literals are the twin's
    plus the shift, `longest` is the twin's and `longest_start` the twin's plus the shift.  A call with room for 1000 records
    is refused and writes nothing.  On the twin the records themselves equal the host's, with both tiles at 256 and at their
    defaults.

    The position tile stays at its default at the large geometries: 256-position tiles would be 16 M serial tile hops of
    k_lz_chain.  Not reachable: the records at the large geometries would take 3 x 8 x 4.3e9 bytes, and even at
    u64_across_2_32 the total, 2^32 - 14 162, stays below 2^32, so record offsets of 2^32 and more are not exercised.

    The call's scratch is 2 n w + 4 n bytes (56 GB at the 32-bit geometries, 90 GB at u64_across_2_32); it belongs to a
    context of this test that is closed at its end."""
    geo, ix = placed.geo, placed.ix[False]
    shift = geo.shift
    want = dict(twin[2]["lz"][3])
    assert want == dict(factors=9934, literals=4505, longest=1197, longest_start=23499)
    want = dict(factors=want["factors"] + shift, literals=want["literals"] + shift, longest=want["longest"], longest_start=want["longest_start"] + shift)
    starts = np.array(geo.seq_starts, dtype=np.uint64)
    L = sufr_amd.lib()
    own = sufr_amd.Context(0)
    try:
        head = (own.handle, ix._h, placed.lcp.data_ptr(), starts.ctypes.data, starts.size)
        torch.cuda.synchronize()
        for tile in TILES:
            own.set_lz_tile(tile, 0)
            total, st = C.c_uint64(0), sufr_amd.LzStats()
            rc = L.sufr_hip_lz_device(*head, 0, None, None, None, C.byref(total), C.byref(st))
            if rc != -5:
                try:
                    own.check(rc)
                except sufr_amd.SufrHipError as e:
                    _memory_skip(f"the parse's scratch of {2 * geo.width + 4} bytes per position at {geo.name}", e)
            assert rc == -5 and total.value == want["factors"] and st.as_dict() == want, (geo.name, tile, rc, total.value, st.as_dict(), want)
        out = [torch.full((LZ_CAP,), -1, dtype=torch.int64, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        total = C.c_uint64(0)
        rc = L.sufr_hip_lz_device(*head, LZ_CAP, *(o.data_ptr() for o in out), C.byref(total), None)
        own.synchronize()
        assert rc == -5 and total.value == want["factors"] > LZ_CAP and all(int(torch.count_nonzero(o != -1)) == 0 for o in out), (geo.name, rc, total.value)
        if geo.name == "twin":
            mine = DeviceIndex(own, ix._h)                                  # the same index through this test's context
            try:
                for tile in ((hp.SMALLEST_TILE, hp.SMALLEST_TILE), (0, 0)):
                    own.set_lz_tile(*tile)
                    start, length, source, stats = mine.lz_device(placed.lcp, geo.seq_starts)
                    got = {"lz": [_ints(start), _ints(length), _ints(source), sorted(stats.items())]}
                    compare(got, twin[2], f"{geo.name} (tiles {tile})", ["lz"])
            finally:
                mine._h = None                                              # (placed owns the handle)
    finally:
        own.close()


def test_a_loaded_sparse_file(ctx, twin, u64_file):
    """DeviceIndex.load of the u64_across_2_32 repeat file (the path of `sufr shared --device 0`), the LCP from the file"""
    geo = REPEAT_GEOMETRIES["u64_across_2_32"]
    path = sparse_or_skip(u64_file, geo.name)
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
            compare(device_answers(ix, lcp, sa, geo, FEWER_FILTERS), twin[1], geo.name + " (loaded)", shared_keys(FEWER_FILTERS))
        finally:
            ix.close()


def test_cli_shared_on_the_device_beyond_2_32(twin, u64_file):
    """`sufr shared --device 0` on the u64_across_2_32 file prints the bytes of the host path on the same file, and the
    twin's once the shift is off the positions within the first sequence; the profile of `--common` has no position and is
    the twin's byte for byte.  Only the failed allocation of the index skips (the message of sufr_hip_index_load's
    out-of-memory return); any other exit but 0, a device error included, fails.  (`sufr lz` on this file would print
    4.3e9 lines and is not run.)"""
    geo = REPEAT_GEOMETRIES["u64_across_2_32"]
    path = sparse_or_skip(u64_file, geo.name)
    cli = lambda *args: subprocess.run([str(sufr_amd.CLI_PATH), "shared", *args], capture_output=True, text=True, timeout=300)
    for opts in (["-l", "12", "--kind", "maximal", "-q", "2"], ["--common"]):
        dev = cli(*opts, "--device", "0", str(path))
        if dev.returncode != 0 and "hipMalloc of the index (" in dev.stderr:
            pytest.skip(f"not enough free HBM for the {geo.n}-byte file: {dev.stderr.strip()}")
        assert dev.returncode == 0, dev.stderr
        host, small = cli(*opts, str(path)), cli(*opts, str(twin[0]))
        assert host.returncode == 0 and small.returncode == 0, host.stderr + small.stderr
        assert dev.stdout == host.stdout
        if opts == ["--common"]:
            assert dev.stdout == small.stdout == "".join(f"{q + 1}\t{v}\n" for q, v in enumerate(twin[1]["common"]))
        else:
            records = len(twin[1][hp.shared_key(1, 12, 2, 0, 2, 0)][0])
            assert _repeat_lines(dev.stdout, geo.shift) == _repeat_lines(small.stdout, 0)
            assert f"# records\t{records}\n" in dev.stdout and dev.stdout.count("\n") == records + 5
