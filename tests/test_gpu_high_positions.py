"""The device query paths at text positions beyond 2^31 and 2^32 (tests/high_positions.py has the construction and the
argument).  The text on the device is one torch.zeros with the 40 000-byte region copied to its end, the suffix array is
SA(region) + filler: as int32 it holds negative values at u32_across_2_31 and u32_top, as int64 values of 2^32 and more at
u64_across_2_32.  The witness is always the host path on the 44 KB twin file (tests/test_query_high_positions.py holds the
host to it at the same geometries); no case compares the device with itself, every comparison is exact.  The BWT, its runs
and LF run here too (they accept an index that leaves positions out); the FM-index does not, and has a module and a
construction of its own: tests/test_gpu_fm_high_positions.py."""
import ctypes as C
import threading
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import high_positions as hp
import sufr_amd
from high_positions import GEOMETRIES, _ints, compare
from sufr_amd import DeviceIndex, SufrFile, pack_queries

pytestmark = pytest.mark.gpu
KMER_K_BY_POSITION = 21


@pytest.fixture(scope="module")
def ctx():
    c = sufr_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    """the open twin file, its answers (the witness) and its outputs by position"""
    path = tmp_path_factory.mktemp("high_positions_gpu") / "twin.sufr"
    hp.write_sparse(path, GEOMETRIES["twin"])
    f = hp.open_checked(path, GEOMETRIES["twin"])
    want = hp.answers(f, 0)
    hp.assert_witness_is_not_empty(want)
    want.update(hp.by_position(f, KMER_K_BY_POSITION))
    B = GEOMETRIES["twin"].boundary - hp.TWIN_FILLER
    for key in (f"kmers k={KMER_K_BY_POSITION} by position", "unique lengths by position"):
        assert any(want[key][:B]) and any(want[key][B + 1:]) and 0 in want[key], key      # both sides; positions left out
    yield SimpleNamespace(file=f, want=want, path=path)
    f.close()


def _memory_skip(what, e):
    """only a failure to get the memory skips, loudly (conftest lists it); anything else fails"""
    if isinstance(e, sufr_amd.SufrHipError) and e.code != -4:
        raise e
    pytest.skip(f"not enough free HBM for {what}: {e}")


def _signed(a: np.ndarray, width: int) -> torch.Tensor:
    """an unsigned array as the tensor the device takes: uint32 -> the int32 view (negative from 2^31 on), uint64 -> int64"""
    return torch.from_numpy(a.astype(np.uint32).view(np.int32).copy() if width == 4 else a.astype(np.int64))


def _unsigned(t: torch.Tensor) -> np.ndarray:
    a = t.cpu().numpy()
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).astype(np.int64)


def place(ctx, geo: hp.Geometry, tables=(True, False), reg=None):
    """the geometry on the device: text, suffix array and LCP tensors and one wrapped index per entry of `tables` (with and
    without the prefix table); reg: another region than hp.region()"""
    reg = reg or hp.region()
    sa, lcp = hp.arrays(geo, reg)
    text = torch.zeros(geo.n, dtype=torch.uint8, device="cuda")
    text[geo.filler:] = torch.from_numpy(reg.text.copy()).cuda()
    d_sa, d_lcp = _signed(sa, geo.width).cuda(), _signed(lcp, geo.width).cuda()
    assert d_sa.dtype == (torch.int32 if geo.width == 4 else torch.int64)
    if geo.name in ("u32_across_2_31", "u32_top"):
        assert int(d_sa.min()) < 0                                          # positions of 2^31 and more, negative as int32
    if geo.name == "u64_across_2_32":
        assert int(d_sa.max()) >= 1 << 32 > int(d_sa.min())
    ix = {t: DeviceIndex.wrap(ctx, text, d_sa, is_dna=True, prefix_table=t) for t in tables}
    for i in ix.values():
        assert i.index_width == geo.width and i.text_len == geo.n
    return SimpleNamespace(geo=geo, text=text, sa=d_sa, lcp=d_lcp, ix=ix)


def release(p):
    for i in p.ix.values():
        i.close()
    p.ix.clear()
    p.text = p.sa = p.lcp = None
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", params=list(GEOMETRIES))
def placed(request, ctx):
    geo = GEOMETRIES[request.param]
    try:
        p = place(ctx, geo)
    except (torch.OutOfMemoryError, sufr_amd.SufrHipError) as e:
        torch.cuda.empty_cache()
        _memory_skip(f"the {geo.n}-byte text of {geo.name}", e)
    yield p
    release(p)                                                              # the text goes before the next geometry comes


@pytest.fixture(scope="module")
def queries():
    qs = list(hp.batch())
    qb, off = pack_queries(qs)
    small = pack_queries(qs[:hp.SMALL])
    dev = lambda b, o: (torch.from_numpy(b).cuda(), torch.from_numpy(o.astype(np.int64)).cuda())
    return SimpleNamespace(list=qs, qb=qb, off=off, dev=dev(qb, off), small=small, small_dev=dev(*small))


def _locate(ix, geo, lo, hi, max_hits):
    """offsets and shifted positions through locate_device; the dtype of the positions and the capacity refusal"""
    o, p = ix.locate_device(lo, hi, max_hits)
    assert p.dtype == (torch.int32 if geo.width == 4 else torch.int64)
    total = p.numel()
    assert total > 0
    with pytest.raises(sufr_amd.SufrHipError) as e:
        ix.locate_device(lo, hi, max_hits, capacity=total - 1)
    assert e.value.code == -5
    return _ints(o), _ints(_unsigned(p), geo.shift)                          # (int32 read back as uint32)


TABLES = pytest.mark.parametrize("table", [True, False], ids=["prefix_table", "no_table"])


@TABLES
def test_search_and_locate(placed, twin, queries, table):
    ix, geo, got = placed.ix[table], placed.geo, {}
    for mql in hp.SEARCH_MQL:
        lo, hi = ix.search_device(*queries.dev, mql)
        got[f"search mql={mql}"] = [_ints(lo.cpu()), _ints(hi.cpu())]
        if mql is None:
            for max_hits in hp.LOCATE_HITS:
                got[f"locate max_hits={max_hits}"] = list(_locate(ix, geo, lo, hi, max_hits))
    compare(got, twin.want, geo.name, got.keys())
    # the host-pointer entry points: sufr_hip_search_batch, and the search-and-gather of DeviceIndex.locate
    lo, hi = ix.search(queries.list)
    compare({"search mql=None": [_ints(lo), _ints(hi)]}, twin.want, geo.name + " (host buffers)", ["search mql=None"])
    per_query = ix.locate(queries.list, max_hits=3)
    flat = np.concatenate(per_query).astype(np.int64) if per_query else np.zeros(0, dtype=np.int64)
    compare({"locate max_hits=3": [_ints(np.concatenate([[0], np.cumsum([len(p) for p in per_query])])), _ints(flat, geo.shift)]},
            twin.want, geo.name + " (DeviceIndex.locate)", ["locate max_hits=3"])


@TABLES
def test_matching_statistics_and_smems(placed, twin, queries, table):
    ix, geo, got = placed.ix[table], placed.geo, {}
    got["matching statistics"] = _ints(_unsigned(ix.matching_statistics_device(*queries.dev))[:int(queries.off[-1])])
    for min_len, max_hits in hp.SMEM_COMBOS:
        qi, qo, ln, lo, hi = ix.smems_device(*queries.dev, min_len)
        got[f"smems min_len={min_len} max_hits={max_hits}"] = [_ints(t.cpu()) for t in (qi, qo, ln, lo, hi)] + list(_locate(ix, geo, lo, hi, max_hits))
    compare(got, twin.want, geo.name, got.keys())


def _host_records(ctx, fn, ix, qb, off, params, dtypes, cap):
    """a host-buffer entry point (sufr_hip_mems / _approx / _edit): the records are staged on the device and copied back"""
    out = [np.zeros(max(cap, 1), dtype=dt) for dt in dtypes]
    total = C.c_uint64(0)
    ctx.check(fn(ctx.handle, ix._h, qb.ctypes.data, off.ctypes.data, len(off) - 1, *params, cap, *[a.ctypes.data for a in out], C.byref(total)))
    assert total.value == cap
    return out


@TABLES
def test_mems(ctx, placed, twin, queries, table):
    ix, geo, got = placed.ix[table], placed.geo, {}
    for min_len, occ, both in hp.MEM_COMBOS:
        key = f"mems min_len={min_len} max_occ={occ} both={both}"
        qi, qo, st, ln, pos = (t.cpu() for t in ix.mems_device(*queries.dev, min_len, occ, both))
        got[key] = [_ints(qi), _ints(qo), _ints(st), _ints(ln), _ints(_unsigned(pos), geo.shift)]
        compare(got, twin.want, geo.name, [key])
        qi, qo, st, ln, pos = _host_records(ctx, sufr_amd.lib().sufr_hip_mems, ix, queries.qb, queries.off, (min_len, occ, int(both)),
                                            (np.uint64, np.uint32, np.uint8, np.uint32, np.uint64), len(twin.want[key][0]))
        compare({key: [_ints(qi), _ints(qo), _ints(st), _ints(ln), _ints(pos, geo.shift)]}, twin.want, geo.name + " (host buffers)", [key])


@TABLES
def test_k_mismatch(ctx, placed, twin, queries, table):
    ix, geo, got = placed.ix[table], placed.geo, {}
    for d, occ, both in hp.APPROX_COMBOS:
        key = f"approx d={d} max_occ={occ} both={both}"
        qi, st, pos, mm = (t.cpu() for t in ix.approx_device(*queries.dev, d, occ, both))
        got[key] = [_ints(qi), _ints(st), _ints(_unsigned(pos), geo.shift), _ints(mm)]
        compare(got, twin.want, geo.name, [key])
        qi, st, pos, mm = _host_records(ctx, sufr_amd.lib().sufr_hip_approx, ix, queries.qb, queries.off, (d, occ, int(both)),
                                        (np.uint64, np.uint8, np.uint64, np.uint8), len(twin.want[key][0]))
        compare({key: [_ints(qi), _ints(st), _ints(pos, geo.shift), _ints(mm)]}, twin.want, geo.name + " (host buffers)", [key])


def sort_passes(n: int, queries: int, both: bool) -> int:
    """the passes of the k-difference radix sort (include/sufr_edit.h): its key holds bit_width(n) bits of exclusive end and
    bit_width(queries - 1) bits of query (doubled with both strands), sorted eight bits a pass; an odd count leaves the
    sorted keys in the second of the two buffers"""
    return -(-(n.bit_length() + (queries * (2 if both else 1) - 1).bit_length()) // 8)


def test_the_end_field_of_the_k_difference_key():
    """32 bits at the largest 32-bit text, 33 across 2^32, and both parities of the pass count with the two batch sizes"""
    assert GEOMETRIES["u32_top"].n.bit_length() == 32 and GEOMETRIES["u64_across_2_32"].n.bit_length() == 33
    assert GEOMETRIES["u32_across_2_31"].n.bit_length() == 32 and GEOMETRIES["twin"].n.bit_length() == 16
    for name in GEOMETRIES:
        n = GEOMETRIES[name].n
        assert sort_passes(n, len(hp.batch()), True) % 2 == 0 and sort_passes(n, hp.SMALL, True) % 2 == 1, name


@TABLES
def test_k_difference_and_traceback(ctx, placed, twin, queries, table):
    ix, geo = placed.ix[table], placed.geo
    for d, occ, both, minima in hp.EDIT_COMBOS:
        for count, (qb, off), dev in ((len(queries.list), (queries.qb, queries.off), queries.dev), (hp.SMALL, queries.small, queries.small_dev)):
            tag = f"d={d} max_occ={occ} both={both} minima={minima} queries={'all' if count == len(queries.list) else count}"
            recs = tuple(t.contiguous() for t in ix.edit_device(*dev, d, occ, both, minima))
            start, coff, cigar = ix.edit_trace_device(*dev, *recs)
            qi, st, end, ed = (t.cpu() for t in recs)
            got = {"edit " + tag: [_ints(qi), _ints(st), _ints(_unsigned(end), geo.shift), _ints(ed)],
                   "trace " + tag: [_ints(_unsigned(start), geo.shift), _ints(coff.cpu()), _ints(_unsigned(cigar))]}
            compare(got, twin.want, geo.name, got.keys())
            # host buffers: the records (sufr_hip_edit) and their traceback (sufr_hip_edit_trace)
            want = twin.want["edit " + tag]
            hrecs = _host_records(ctx, sufr_amd.lib().sufr_hip_edit, ix, qb, off, (d, occ, int(both) | 2 * int(minima)),
                                  (np.uint64, np.uint8, np.uint64, np.uint8), len(want[0]))
            start, coff, cigar = ix.edit_trace(qb, off, *hrecs)
            got = {"edit " + tag: [_ints(hrecs[0]), _ints(hrecs[1]), _ints(hrecs[2], geo.shift), _ints(hrecs[3])],
                   "trace " + tag: [_ints(start, geo.shift), _ints(coff), _ints(cigar)]}
            compare(got, twin.want, geo.name + " (host buffers)", got.keys())


@TABLES
def test_align(placed, twin, queries, table):
    ix, geo = placed.ix[table], placed.geo
    got = {"align": [[(h.query, h.strand, h.end - geo.shift, h.edits, h.start - geo.shift, h.cigar) for h in hits]
                     for hits in ix.align(queries.list[hp.ALIGN_SLICE], 3, 0, True, True)]}
    compare(got, twin.want, geo.name, ["align"])


@TABLES
def test_kmers_and_unique_lengths_by_rank(placed, twin, table):
    ix, geo, got = placed.ix[table], placed.geo, {}
    for k in hp.KMER_KS:
        hist, stats, occ = ix.kmers_device(placed.lcp, k, hp.KMER_BINS, "rank", geo.seq_starts)
        assert occ.dtype == placed.lcp.dtype
        got[f"kmers k={k}"] = [_ints(hist.cpu()), sorted(stats.items()), _ints(_unsigned(occ))]
    got["unique lengths"] = _ints(_unsigned(ix.unique_lengths_device(placed.lcp, False, geo.seq_starts)))
    compare(got, twin.want, geo.name, got.keys())


@pytest.mark.parametrize("table", [True], ids=["prefix_table"])
def test_the_python_wrappers_read_positions_at_the_index_width(placed, twin, queries, table):
    """DeviceIndex.matching_statistics, .smems, .mems, .approx and .edit (the *_device calls with their results read back into
    numpy and dataclasses), one combination each"""
    ix, geo, qs, got = placed.ix[table], placed.geo, queries.list, {}
    got["matching statistics"] = _ints(np.concatenate(ix.matching_statistics(qs)))
    min_len, max_hits = hp.SMEM_COMBOS[0]
    hits = [h for per in ix.smems(qs, min_len, max_hits) for h in per]
    got[f"smems min_len={min_len} max_hits={max_hits}"] = [
        [h.query_num for h in hits], [h.query_offset for h in hits], [h.length for h in hits], [h.rank_lo for h in hits],
        [h.rank_hi for h in hits], _ints(np.concatenate([[0], np.cumsum([len(h.positions) for h in hits])])),
        _ints(np.concatenate([h.positions for h in hits]), geo.shift)]
    assert hits and hits[0].positions.dtype == (np.uint32 if geo.width == 4 else np.uint64)
    min_len, occ, both = hp.MEM_COMBOS[1]
    mems = [(i, h) for i, per in enumerate(ix.mems(qs, min_len, occ, both)) for h in per]
    got[f"mems min_len={min_len} max_occ={occ} both={both}"] = [[i for i, _ in mems], [h.query_offset for _, h in mems], [h.strand for _, h in mems],
                                                                 [h.length for _, h in mems], [h.position - geo.shift for _, h in mems]]
    d, occ, both = hp.APPROX_COMBOS[1]
    hits = [h for per in ix.approx(qs, d, occ, both) for h in per]
    got[f"approx d={d} max_occ={occ} both={both}"] = [[h.query for h in hits], [h.strand for h in hits], [h.position - geo.shift for h in hits],
                                                      [h.mismatches for h in hits]]
    d, occ, both, minima = hp.EDIT_COMBOS[1]
    hits = [h for per in ix.edit(qs, d, occ, both, minima) for h in per]
    got[f"edit d={d} max_occ={occ} both={both} minima={minima} queries=all"] = [[h.query for h in hits], [h.strand for h in hits],
                                                                               [h.end - geo.shift for h in hits], [h.edits for h in hits]]
    compare(got, twin.want, geo.name + " (Python wrappers)", got.keys())


@pytest.fixture(scope="module")
def bwt_want(twin):
    """the twin's BWT, runs and LF from the host path, held to numpy on the arrays and shown not to be empty"""
    return hp.bwt_witness(twin.file)[0]


@pytest.mark.parametrize("tile", [0, 256], ids=["default_tile", "tile_256"])
def test_bwt_runs_and_lf(ctx, placed, bwt_want, tile):
    """BWT[r] = T[SA[r] - 1] and first = SA[a] of the run records at positions that are negative as int32 or beyond 2^32:
    everything but `first` is the twin's.  The capacity refusal of the runs writes nothing."""
    ix, geo = placed.ix[False], placed.geo
    ctx.set_bwt_tile(tile)
    try:
        got = hp.bwt_answers(lambda: tuple(t.cpu() for t in ix.bwt_device()),
                             lambda min_len: tuple(t.cpu() for t in ix.bwt_runs_device(min_len)[:4]) + (ix.bwt_runs_device(min_len)[4],),
                             lambda: _unsigned(ix.lf_device()), geo.shift)
        compare(got, bwt_want, f"{geo.name} (tile {tile})")
        assert ix.lf_device().dtype == (torch.int32 if geo.width == 4 else torch.int64)
        z = len(bwt_want["bwt runs min_len=1"][0])
        out = [torch.full((z,), -1, dtype=torch.int64, device="cuda") for _ in range(4)]
        total = C.c_uint64(0)
        rc = sufr_amd.lib().sufr_hip_bwt_runs_device(ctx.handle, ix._h, 1, z - 1, *(o.data_ptr() for o in out), C.byref(total), None)
        ctx.synchronize()
        assert rc == -5 and total.value == z and all(bool((o == -1).all()) for o in out)
    finally:
        ctx.set_bwt_tile(0)


def _all_zero(t: torch.Tensor) -> bool:
    step = 1 << 30
    return all(int(torch.count_nonzero(t[a:a + step])) == 0 for a in range(0, t.numel(), step))


def test_kmers_and_unique_lengths_by_position(placed, twin):
    """The outputs have n entries of the index's width (17 GB at u32_top, 34 GB at u64_across_2_32): the entries of the
    region are the twin's, the filler's are all zero."""
    ix, geo = placed.ix[False], placed.geo
    for key, call in ((f"kmers k={KMER_K_BY_POSITION} by position",
                       lambda: ix.kmers_device(placed.lcp, KMER_K_BY_POSITION, hp.KMER_BINS, "position", geo.seq_starts)[2]),
                      ("unique lengths by position", lambda: ix.unique_lengths_device(placed.lcp, True, geo.seq_starts))):
        try:
            out = call()
        except (torch.OutOfMemoryError, sufr_amd.SufrHipError) as e:
            torch.cuda.empty_cache()
            _memory_skip(f"{geo.n} entries of {geo.width} bytes by position at {geo.name}", e)
        assert out.numel() == geo.n and out.dtype == placed.lcp.dtype
        compare({key: _ints(_unsigned(out[geo.filler:]))}, twin.want, geo.name, [key])
        assert _all_zero(out[:geo.filler]), f"{key} at {geo.name}: an entry of the filler is not zero"
        del out
        torch.cuda.empty_cache()


def test_the_width_rule_of_wrap(ctx):
    """u32 exactly when text_len < 2^32 - 1.  On the first 64-bit length the wrapper refuses a 32-bit tensor and the library
    reads the array as 64-bit whatever the flag says; one byte shorter (the largest 32-bit text) both take 32-bit entries."""
    n = hp.WIDTH_FLIP.n
    assert n == 0xFFFFFFFF == GEOMETRIES["u32_top"].n + 1
    try:
        text = torch.zeros(n, dtype=torch.uint8, device="cuda")
    except torch.OutOfMemoryError as e:
        _memory_skip(f"a {n}-byte text", e)
    sa = torch.zeros(4, dtype=torch.int32, device="cuda")                   # (room for one 64-bit entry and more)
    L = sufr_amd.lib()
    flags = sufr_amd._lib.FLAG_DNA | sufr_amd._lib.FLAG_NO_PREFIX_TABLE
    with pytest.raises(ValueError):
        DeviceIndex.wrap(ctx, text, sa, is_dna=True)
    for length, width in ((n, 8), (n - 1, 4)):
        h = C.c_void_p()
        ctx.check(L.sufr_hip_index_wrap(ctx.handle, text.data_ptr(), length, sa.data_ptr(), 1, flags, 0, None, C.byref(h)))
        assert L.sufr_hip_index_width(h) == width, (length, width)
        L.sufr_hip_index_free(h)
    ix = DeviceIndex.wrap(ctx, text[:n - 1], sa, is_dna=True, prefix_table=False)
    assert ix.index_width == 4
    ix.close()
    ix = DeviceIndex.wrap(ctx, text, sa.view(torch.int64), is_dna=True, prefix_table=False)
    assert ix.index_width == 8
    ix.close()
    del text
    torch.cuda.empty_cache()


def test_a_sparse_file_loaded_to_the_device(ctx, twin, queries, tmp_path):
    """DeviceIndex.load of the u64_across_2_32 file (the path of `sufr ... --device 0`): 4.3 GB of page-cache zeros go to the
    device, then search, locate and MEMs."""
    geo = GEOMETRIES["u64_across_2_32"]
    path = tmp_path / "u64.sufr"
    used = hp.write_sparse(path, geo)
    if used > hp.SPARSE_LIMIT:
        pytest.skip(f"the filesystem has no holes: {used} bytes of blocks for a {geo.n}-byte text")
    with hp.open_checked(path, geo) as f:
        try:
            ix = DeviceIndex.load(ctx, f)
        except sufr_amd.SufrHipError as e:
            _memory_skip(f"the {geo.n}-byte file", e)
        assert ix.index_width == 8
        lo, hi = ix.search_device(*queries.dev)
        got = {"search mql=None": [_ints(lo.cpu()), _ints(hi.cpu())], "locate max_hits=0": list(_locate(ix, geo, lo, hi, 0))}
        min_len, occ, both = hp.MEM_COMBOS[0]
        qi, qo, st, ln, pos = (t.cpu() for t in ix.mems_device(*queries.dev, min_len, occ, both))
        got[f"mems min_len={min_len} max_occ={occ} both={both}"] = [_ints(qi), _ints(qo), _ints(st), _ints(ln), _ints(_unsigned(pos), geo.shift)]
        compare(got, twin.want, geo.name + " (loaded)", got.keys())
        ix.close()


def test_two_contexts_share_the_index_beyond_2_32(twin, queries):
    """Two contexts on two host threads, one u64_across_2_32 index whose array leaves positions out: the first calls race for
    the bitmap of the indexed positions, 2^32 + 20 000 bits of it."""
    geo = GEOMETRIES["u64_across_2_32"]
    ctxs = [sufr_amd.Context(0), sufr_amd.Context(0)]
    p = None
    try:
        try:
            p = place(ctxs[0], geo, tables=(True,))
        except (torch.OutOfMemoryError, sufr_amd.SufrHipError) as e:
            torch.cuda.empty_cache()
            _memory_skip(f"the {geo.n}-byte text of {geo.name}", e)
        ix = p.ix[True]
        keys = [f"approx d={hp.APPROX_COMBOS[0][0]} max_occ={hp.APPROX_COMBOS[0][1]} both={hp.APPROX_COMBOS[0][2]}",
                "edit d=3 max_occ=0 both=True minima=True queries=all"]
        errors = []

        def work(k):
            mine = DeviceIndex(ctxs[k], ix._h)                     # the same index through this thread's context
            assert mine.index_width == 8
            try:
                for rep in range(3):
                    for which in ((0, 1) if k == 0 else (1, 0)):
                        if which == 0:
                            qi, st, pos, v = (t.cpu() for t in mine.approx_device(*queries.dev, *hp.APPROX_COMBOS[0]))
                        else:
                            qi, st, pos, v = (t.cpu() for t in mine.edit_device(*queries.dev, *hp.EDIT_COMBOS[1]))
                        compare({keys[which]: [_ints(qi), _ints(st), _ints(_unsigned(pos), geo.shift), _ints(v)]}, twin.want,
                                f"{geo.name} (context {k}, call {rep})", [keys[which]])
            except BaseException as e:                             # noqa: BLE001 (reported below, in the main thread)
                errors.append(f"context {k}: {e!r}")
            finally:
                mine._h = None                                     # (ix owns the handle)

        threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in threads: t.start()
        for t in threads: t.join(timeout=600)
        assert not any(t.is_alive() for t in threads), "a call did not return"
        assert not errors, errors
    finally:                                                       # a skip or a failure here holds no HBM for the rest of the module
        if p is not None:
            release(p)
        for c in ctxs: c.close()
