"""The FM-index on the device at ranks and text positions beyond 2^31 and 2^32 (tests/high_positions.py has the construction
and the argument).  The FM-index refuses an index that leaves positions out, so here the filler is indexed: T = 0x00^F region,
whose suffix array is [0 .. F) ++ SA(region) + F, is placed on the device without a sort (one torch.zeros and an arange) and
sufr_hip_fm_build runs on all n ranks, as does the index of the reversed text.  The ranks and the positions of the region
straddle 2^31 (u32_across_2_31), end at 2^32 - 2 (u32_top) or straddle 2^32 (u64_across_2_32) at the region's middle byte; at
u32_top and u64_across_2_32 the region's blocks lie beyond 4 GB of the block array.  The witness is always the host pair on
the 44 KB twin (tests/test_query_high_positions.py holds it to numpy); no case compares the device with itself, every
comparison is exact.

Deliberately out of scope: save / load at the large geometries (a 7 GB file per case; the section offsets beyond 2^32 in the
file stay untested), upload, a host *build* at large n (it needs a 17 to 34 GB suffix array in a file that cannot be sparse;
the host *query* code runs on a downloaded index, below) and a run longer than 2^32 ranks (the longest, F - 1, stays just
below)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import high_positions as hp
import sufr_amd
from high_positions import FULL_GEOMETRIES, R, compare
from sufr_amd import DeviceIndex, pack_queries
from test_gpu_high_positions import _memory_skip, _signed, _unsigned

pytestmark = pytest.mark.gpu
CASES = [(name, symbols) for name in FULL_GEOMETRIES for symbols in hp.FULL_SYMBOLS[name]]
PIECE = 1 << 30


@pytest.fixture(scope="module")
def ctx():
    c = sufr_amd.Context(0)
    c.set_bwt_tile(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    """symbols -> the host pair on the twin, its files and its answers (the witness), built once each"""
    d = tmp_path_factory.mktemp("fm_high_positions_gpu")
    made = {}

    def get(symbols):
        if symbols not in made:
            fwd, rev, f, g = hp.full_host_pair(d, hp.TWIN_FILLER, symbols)
            want = hp.fm_answers(fwd, rev, 0, hp.TWIN_FILLER, symbols)
            hp.assert_fm_witness_is_not_empty(want, symbols)
            made[symbols] = SimpleNamespace(fwd=fwd, rev=rev, f=f, g=g, want=want, dir=d)
        return made[symbols]
    return get


def _count_up(view: torch.Tensor, start: int):
    """view[i] = start + i at the tensor's width, unsigned: as int32 the values from 2^31 on are written as their negative
    twins, because int32 cannot count past 2^31 - 1.  In pieces, so that no temporary of the view's size is made."""
    for a in range(0, view.numel(), PIECE):
        b = min(a + PIECE, view.numel())
        lo, hi = start + a, start + b
        if view.dtype == torch.int64 or hi <= 1 << 31:
            torch.arange(lo, hi, dtype=view.dtype, device=view.device, out=view[a:b])
        elif lo >= 1 << 31:
            torch.arange(lo - (1 << 32), hi - (1 << 32), dtype=view.dtype, device=view.device, out=view[a:b])
        else:
            cut = (1 << 31) - lo
            torch.arange(lo, 1 << 31, dtype=view.dtype, device=view.device, out=view[a:a + cut])
            torch.arange(-(1 << 31), hi - (1 << 32), dtype=view.dtype, device=view.device, out=view[a + cut:b])


def place_full(ctx, geo: hp.Geometry, symbols: int, reverse: bool):
    """T = 0x00^F region (or its reversal, reverse(region[:-1]) 0x00^F $) and its suffix array on the device, wrapped: no
    n-entry array is built on the host"""
    reg = hp.full_region(symbols)
    F, n = geo.filler, geo.n
    tail, rtail = hp.full_sa_tail(F, symbols)
    text = torch.zeros(n, dtype=torch.uint8, device="cuda")
    sa = torch.empty(n, dtype=torch.int32 if geo.width == 4 else torch.int64, device="cuda")
    if reverse:
        text[:R - 1] = torch.from_numpy(reg.rtext[:-1].copy()).cuda()
        text[n - 1] = int(reg.rtext[-1])
        _count_up(sa[:F], R - 1)
        sa[F:] = _signed(rtail.astype(np.uint64), geo.width).cuda()
    else:
        text[F:] = torch.from_numpy(reg.text.copy()).cuda()
        _count_up(sa[:F], 0)
        sa[F:] = _signed(tail.astype(np.uint64), geo.width).cuda()
    # the ends of the counted part, read back unsigned
    first = 0 if not reverse else R - 1
    assert _unsigned(sa[:2]).tolist() == [first, first + 1] and _unsigned(sa[F - 2:F]).tolist() == [first + F - 2, first + F - 1]
    if geo.name in ("u32_across_2_31", "u32_top"):
        assert int(sa[F - 1]) < 0 or (not reverse and geo.name == "u32_across_2_31")        # negative as int32
    ix = DeviceIndex.wrap(ctx, text, sa, is_dna=False, prefix_table=False)
    assert ix.index_width == geo.width and ix.text_len == ix.len_suffixes == n
    return SimpleNamespace(text=text, sa=sa, ix=ix)


def release_full(p):
    if p is not None and p.ix is not None:
        p.ix.close()
        p.ix = p.text = p.sa = None
    torch.cuda.empty_cache()


class Dev:
    """a DeviceFmIndex with the methods of the host FmIndex that hp.fm_answers calls: numpy in, numpy out, through the
    *_device entry points"""

    def __init__(self, fm):
        self.fm = fm

    @property
    def info(self):
        return self.fm.info

    @staticmethod
    def _dev(qb, off):
        return torch.from_numpy(np.ascontiguousarray(qb)).cuda(), torch.from_numpy(np.asarray(off).astype(np.int64)).cuda()

    def search_batch(self, queries):
        lo, hi = self.fm.search_device(*self._dev(*pack_queries(list(queries))))
        return _unsigned(lo), _unsigned(hi)

    def locate_ranges(self, lo, hi, max_hits=0):
        lo, hi = (torch.from_numpy(np.asarray(a).astype(np.int64)).cuda() for a in (lo, hi))
        o, p = self.fm.locate_device(lo, hi, max_hits)
        assert p.dtype == (torch.int64 if self.fm.index_width == 8 else torch.int32)
        return _unsigned(o), _unsigned(p)                                       # (int32 read back as uint32)

    def approx_arrays(self, qb, off, d, both):
        qi, st, pos, mm = self.fm.approx_device(*self._dev(qb, off), d, both)
        return _unsigned(qi), _unsigned(st), _unsigned(pos), _unsigned(mm)

    def matching_stats(self, queries, rev):
        qb, off = pack_queries(list(queries))
        ms = self.fm.matching_stats_device(*self._dev(qb, off), rev.fm)
        return [_unsigned(ms)[:int(off[-1])]]

    def smem_arrays(self, qb, off, rev, min_len):
        out = self.fm.smems_device(*self._dev(qb, off), rev.fm, min_len)
        return tuple(_unsigned(t) for t in out)

    def extract_ranges(self, starts, ends):
        return self.fm.extract_ranges(starts, ends)


def build_pair(ctx, geo, symbols):
    """the pair of a geometry: the reversed text first (placed, built without samples, freed), then the text, whose placement
    stays for the cases that need the suffix array (the BWT, its runs, LF and a second build)"""
    rev = fwd = placed = None
    try:
        p = place_full(ctx, geo, symbols, reverse=True)
        try:
            rev = p.ix.fm_device(0)
        finally:
            release_full(p)
        placed = place_full(ctx, geo, symbols, reverse=False)
        fwd = placed.ix.fm_device(hp.FM_SAMPLE, text=True)
    except BaseException:
        for fm in (rev, fwd):
            if fm is not None:
                fm.close()
        release_full(placed)
        raise
    return SimpleNamespace(geo=geo, symbols=symbols, fwd=Dev(fwd), rev=Dev(rev), placed=placed)


@pytest.fixture(scope="module", params=CASES, ids=[f"{name}-{symbols}_symbols" for name, symbols in CASES])
def pair(request, ctx):
    name, symbols = request.param
    geo = FULL_GEOMETRIES[name]
    try:
        p = build_pair(ctx, geo, symbols)
    except (torch.OutOfMemoryError, sufr_amd.SufrHipError) as e:
        torch.cuda.empty_cache()
        _memory_skip(f"the {geo.n} ranks of {geo.name}", e)
    yield p
    p.fwd.fm.close()
    p.rev.fm.close()
    release_full(p.placed)                                                      # everything goes before the next geometry comes


def _check(pair, twins, parts, tag=""):
    geo = pair.geo
    got = hp.fm_answers(pair.fwd, pair.rev, geo.shift, geo.filler, pair.symbols, parts=parts)
    compare(got, twins(pair.symbols).want, f"{geo.name}, {pair.symbols} symbols{tag}", got.keys())
    return got


def fm_bytes(info: dict) -> int:
    """fm_device_bytes of sufr_fm.inc: the blocks, with samples the mark words and the kept values, C and the columns"""
    s, w = info["ranks"], info["width"]
    marks = ((s + 63) // 64 * 16 + info["samples"] * w) if info["sample"] else 0
    return (s // info["block"] + 1) * info["stride"] + marks + 257 * 8 + 256 * 4


def test_info(pair, twins):
    geo, n = pair.geo, pair.geo.n
    info, rinfo = pair.fwd.info, pair.rev.info
    shape = (96, 128) if (pair.symbols, geo.width) == (8, 4) else (64, 128)     # one line; 64 + 64 at K = 9 or w = 8
    for i in (info, rinfo):
        assert (i["ranks"], i["width"], i["symbols"], i["end_byte"]) == (n, geo.width, pair.symbols, 36)
        assert (i["block"], i["stride"]) == shape and i["bytes"] == fm_bytes(i)
    assert info["sample"] == hp.FM_SAMPLE and info["samples"] == -(-n // hp.FM_SAMPLE) and (rinfo["sample"], rinfo["samples"]) == (0, 0)
    assert pair.fwd.fm.text_info["text_samples"] == info["samples"]
    if geo.name in ("u32_top", "u64_across_2_32"):
        assert info["bytes"] > 1 << 32 and rinfo["bytes"] > 1 << 32              # the region's blocks lie beyond 4 GB
        assert (geo.filler // info["block"]) * info["stride"] > 1 << 32
    _check(pair, twins, ("info",))
    # the pair check passes (every call on the pair makes it); the text's index paired with itself is not refused by it, because
    # the check reads ranks, width, end byte, byte values and C, which an index shares with itself: left out


def test_search_locate(pair, twins):
    geo, fm = pair.geo, pair.fwd.fm
    got = _check(pair, twins, ("search", "locate"))
    want = twins(pair.symbols).want
    queries = list(hp.fm_batch(pair.symbols)[0])
    # the capacity refusal
    lo, hi = (np.asarray(a).copy() for a in pair.fwd.search_batch(queries))
    lo[queries.index(b"")] = hi[queries.index(b"")] = 0
    lo, hi = torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda()
    total = len(want["locate max_hits=3"][1])
    with pytest.raises(sufr_amd.SufrHipError) as e:
        fm.locate_device(lo, hi, 3, capacity=total - 1)
    assert e.value.code == -5
    # the host-pointer entry points
    keep = [q for q in queries if q]
    hlo, hhi = fm.search(keep)
    plain = [a for a, q in zip(zip(*got["search"]), queries) if q]
    shifted = lambda a, some: np.where(some, a.astype(np.int64) - geo.shift, a.astype(np.int64)).tolist()
    assert [shifted(hlo, hhi > hlo), shifted(hhi, hhi > hlo)] == [[a for a, _ in plain], [b for _, b in plain]]
    per_query = fm.locate(keep, max_hits=3)
    assert per_query[0].dtype == (np.uint64 if geo.width == 8 else np.uint32)
    flat = np.concatenate(per_query).astype(np.int64) - geo.shift
    assert flat.tolist() == want["locate max_hits=3"][1]                         # (the empty query holds no position there)


def test_approx(pair, twins):
    _check(pair, twins, ("approx",))
    d, both = hp.FM_APPROX_COMBOS[0]
    queries = [q for q in hp.fm_batch(pair.symbols)[0] if len(q) > d]
    total = len(twins(pair.symbols).want[f"approx d={d} both={both}"][0])
    with pytest.raises(sufr_amd.SufrHipError) as e:
        pair.fwd.fm.approx_device(*Dev._dev(*pack_queries(queries)), d, both, cap=total - 1)
    assert e.value.code == -5 and e.value.total == total


def test_extract(pair, twins):
    geo, fm = pair.geo, pair.fwd.fm
    _check(pair, twins, ("extract",))                                           # extract_ranges: against the text and the twin
    starts, ends = hp.fm_extract_requests(geo.filler, geo.n)
    d_starts, d_ends = (torch.from_numpy(a.astype(np.int64)).cuda() for a in (starts, ends))
    off, data = fm.extract_device(d_starts, d_ends)
    h_off, h_data = fm.extract_ranges(starts, ends)
    assert np.array_equal(_unsigned(off), h_off.astype(np.int64)) and np.array_equal(data.cpu().numpy(), h_data)
    with pytest.raises(sufr_amd.SufrHipError) as e:
        fm.extract_device(d_starts, d_ends, cap=int(h_off[-1]) - 1)
    assert e.value.code == -5 and e.value.total == int(h_off[-1])


def test_matching_stats_and_smems(pair, twins):
    geo, fm = pair.geo, pair.fwd.fm
    _check(pair, twins, ("ms", "smems"))                                        # smems_device and locate_device of its ranges
    want = twins(pair.symbols).want
    total = len(want["matching statistics"])
    assert _unsigned(fm.last_ms)[:total].tolist() == want["matching statistics"]
    queries = list(hp.fm_batch(pair.symbols)[0])
    hits = [h for per in fm.smems(queries, pair.rev.fm, 15, 4) for h in per]
    qi, qo, ln, lo, hi, o, pos = want["smems min_len=15"]
    assert [[h.query_num for h in hits], [h.query_offset for h in hits], [h.length for h in hits]] == [qi, qo, ln]
    assert [h.rank_lo - geo.shift for h in hits] == lo and [h.rank_hi - geo.shift for h in hits] == hi
    assert [(h.positions.astype(np.int64) - geo.shift).tolist() for h in hits] == [pos[o[t]:min(o[t + 1], o[t] + 4)] for t in range(len(qi))]


def test_bwt_runs_lf_full(pair, twins):
    """the BWT, the runs and LF of all n ranks, checked on the device: the filler's part is analytic, the tail is the twin's"""
    geo, ix, tw = pair.geo, pair.placed.ix, twins(pair.symbols)
    F, n, shift = geo.filler, geo.n, geo.shift
    t_bwt, t_counts = tw.f.bwt()
    bwt, counts = ix.bwt_device()
    assert int(bwt[0]) == 36 and all(int(torch.count_nonzero(bwt[a:min(a + PIECE, F)])) == 0 for a in range(1, F, PIECE))
    assert np.array_equal(bwt[F:].cpu().numpy(), t_bwt[hp.TWIN_FILLER:]) and int(counts[0]) == F
    assert np.array_equal(_unsigned(counts)[1:], t_counts[1:].astype(np.int64))
    del bwt
    t_runs = tw.f.bwt_runs(1)
    rank, length, symbol, first, st = ix.bwt_runs_device(1)
    rank, length, symbol, first = (_unsigned(t) for t in (rank, length, symbol, first))
    assert (rank[:2].tolist(), length[:2].tolist(), symbol[:2].tolist(), first[:2].tolist()) == ([0, 1], [1, F - 1], [36, 0], [0, 1])
    assert np.array_equal(rank[2:] - shift, t_runs[0][2:].astype(np.int64)) and np.array_equal(first[2:] - shift, t_runs[3][2:].astype(np.int64))
    assert np.array_equal(length[2:], t_runs[1][2:].astype(np.int64)) and np.array_equal(symbol[2:], t_runs[2][2:].astype(np.int64))
    assert st == dict(t_runs[4], longest=F - 1) and st["longest_rank"] == 1 and st["runs"] == t_runs[4]["runs"]
    try:
        lf = ix.lf_device()
    except (torch.OutOfMemoryError, sufr_amd.SufrHipError) as e:
        torch.cuda.empty_cache()
        _memory_skip(f"the {n} entries of LF at {geo.name}", e)
    assert lf.dtype == (torch.int64 if geo.width == 8 else torch.int32)
    assert _unsigned(lf[:1]).tolist() == [F]
    for a in range(1, F, PIECE):                                                # lf[r] = r - 1 in the filler
        b = min(a + PIECE, F)
        piece = lf[a:b].to(torch.int64)
        if geo.width == 4:
            piece &= 0xFFFFFFFF
        assert bool((piece == torch.arange(a - 1, b - 1, dtype=torch.int64, device="cuda")).all()), (geo.name, a)
        del piece
    assert np.array_equal(_unsigned(lf[F:]) - shift, tw.f.lf().astype(np.int64)[hp.TWIN_FILLER:])
    del lf
    torch.cuda.empty_cache()


def _pair_or_skip(ctx, geo, symbols, build):
    try:
        return build()
    except (torch.OutOfMemoryError, sufr_amd.SufrHipError) as e:
        torch.cuda.empty_cache()
        _memory_skip(f"the {geo.n} ranks of {geo.name}", e)


def test_sample_8_at_64_bits(ctx, twins):
    """an index of the text of u64_across_2_32 at sample 8, with text samples: samples * 8 > 2^32 bytes, so the kept values and
    the text samples of the region's upper half lie beyond 4 GB of `kept` and of `text_kept` (at sample 32 either array ends
    at 1 GB).  Locate and extract, against the twin built at sample 8 and against the text."""
    geo, symbols = FULL_GEOMETRIES["u64_across_2_32"], 8
    tw = twins(symbols)
    t8 = tw.f.fm(8, text=True)
    parts = ("search", "locate", "extract")
    want = hp.fm_answers(t8, None, 0, hp.TWIN_FILLER, symbols, parts=parts)
    assert want["locate max_hits=0"] == tw.want["locate max_hits=0"] and want["extract"] == tw.want["extract"]

    def build():
        p = place_full(ctx, geo, symbols, reverse=False)
        try:
            return p.ix.fm_device(8, text=True)
        finally:
            release_full(p)
    fm8 = _pair_or_skip(ctx, geo, symbols, build)
    try:
        assert fm8.info["samples"] * 8 > 1 << 32 and fm8.info["sample"] == 8 and fm8.text_info["text_bytes"] > 1 << 32
        got = hp.fm_answers(Dev(fm8), None, geo.shift, geo.filler, symbols, parts=parts)
        compare(got, want, f"{geo.name} at sample 8", got.keys())
    finally:
        fm8.close()
        torch.cuda.empty_cache()


def test_downloaded_index_on_the_host(ctx, twins):
    """sufr_hip_fm_download of both indexes of u32_top and every host operation on the copies, with all threads: the host query
    code of sufr_fm_scan.h at ranks beyond 2^31, which no host build can reach here"""
    geo, symbols = FULL_GEOMETRIES["u32_top"], 8
    p = _pair_or_skip(ctx, geo, symbols, lambda: build_pair(ctx, geo, symbols))
    release_full(p.placed)
    fwd = rev = None
    try:
        try:
            fwd, rev = p.fwd.fm.to_host(), p.rev.fm.to_host()
        except (MemoryError, sufr_amd.SufrHipError) as e:
            if isinstance(e, sufr_amd.SufrHipError) and e.code != -4:
                raise
            pytest.skip(f"not enough host memory for the downloaded pair of {geo.name}: {e}")
        assert fwd.info == p.fwd.info and rev.info == p.rev.info
        fwd.pair_check(rev)
        got = hp.fm_answers(fwd, rev, geo.shift, geo.filler, symbols)
        compare(got, twins(symbols).want, f"{geo.name} (downloaded, on the host)")
    finally:
        for fm in (fwd, rev, p.fwd.fm, p.rev.fm):
            if fm is not None:
                fm.close()
        torch.cuda.empty_cache()
