"""The --dna build paths at text positions beyond 2^31 and 2^32 (tests/high_build.py has the layout and the twin argument;
tests/test_build_high_witness.py checks its precondition on the CPU).

The text of every case is  N^F . X . N^T . $ : a filler that is not indexed, one of the regions of test_gpu_overlap.py (or a
soft-masked one), a tail.  The build costs a text pass over the filler plus the build of X, and its whole SA and LCP must equal
the oracle's arrays of the twin, shifted.  Outputs are caller-supplied, zero-filled, |X| + 64 entries.

  one window   across_2_31 (the boundary byte of X at 2^31) and top_single (n = SUFR_MAX_TEXT_LEN - 1, X at the end), index
               widths 4 and 8: left-over chain on the helper and behind, tie level and doubling, the run bucket, listed bytes,
               -m 12 / 16 (direct) and 30 (apply_max_query_len), the seed mask, three shards with the stitch, a soft-masked text at
               aligned and misaligned addresses, the host-buffer entry point
  windows      first_windowed (n = SUFR_MAX_TEXT_LEN: the shortest text that takes windows, 32-bit output), u32_cut_2_31
               (n = 2^32 - 2, the default plan cuts at 2^31), u64_cut_2_31 / u64_cut_2_32 (n = 3 * 2^31, three windows of 2^31):
               the cut on X's boundary byte; wide and short margins (repair), listed bytes, -m 16, the seed mask, two shards

Every case says from stats or context getters which path ran; that the path ran at a position >= 2^31 follows from the equality
itself (high_build.expected asserts that the expected positions reach n - 1 and lie on both sides of the boundary).

Cut products: widths and geometries are not multiplied with every region -- each (region, option) runs at both one-window
geometries with the widths alternating, and at every windowed geometry at the one width it has.

Memory: a one-window doubling case at n ~ 2^32 takes ~34 GB for ranks beside ~9 GB of text; a windowed case keeps the caller's
text, the normalised copy, the windows' rank arrays of n 32-bit entries each and one window's arrays and workspace: by the sizes
in sufr_wide.inc ~60 GB at n = 2^32 - 2 and ~85 GB at n = 3 * 2^31.  A case skips only when the device says it is out of memory.

Measured on an MI355X: 37 cases, none skipped, 23 s in all, 3.3 s the slowest (the first use of an oracle twin is in its case)."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import sufr_amd
import high_build as hb
from sufr_amd import shards
from test_gpu_mql_fast import canonical

pytestmark = pytest.mark.gpu

NEVER = 2**64 - 1
ONE_WINDOW = ("across_2_31", "top_single")
CUTS = ("u32_cut_2_31", "u64_cut_2_31", "u64_cut_2_32")
WIDE_MARGIN = 1 << 16                   # covers the longest LCP of the regions (5 999)


@pytest.fixture()
def db():
    d = sufr_amd.DeviceBuilder(0)
    t0 = time.perf_counter()
    yield d
    d.close()
    print(f"[{time.perf_counter() - t0:.2f} s]")


@pytest.fixture(scope="module")
def _window_builder():
    d = sufr_amd.DeviceBuilder(0)
    yield d
    d.close()


@pytest.fixture()
def wdb(_window_builder):
    """one context for all windowed cases, as a caller that builds text after text keeps one: its buffers (the windows' rank arrays
    take n entries each) are allocated once, and every build finds what the one before has left in them"""
    d = _window_builder
    t0 = time.perf_counter()
    yield d
    d.ctx.set_window(0, 0); d.ctx.set_window_retry(0); d.ctx.set_overlap_min(0)
    print(f"[{time.perf_counter() - t0:.2f} s]")


@pytest.fixture(scope="module", autouse=True)
def _buffer():
    yield
    hb.release()


def sort(db, x, lay, width, **kw):
    """one build into zero-filled outputs of |X| + 64 entries -> SA, LCP (unsigned numpy arrays)"""
    cap = lay.x_len + 64
    dt = torch.int32 if width == 4 else torch.int64
    try:
        out_sa = torch.zeros(cap, dtype=dt, device="cuda"); out_lcp = torch.zeros(cap, dtype=dt, device="cuda")
        sa, lcp = db.sort(x, is_dna=True, index_width=width, out_sa=out_sa, out_lcp=out_lcp, **kw)
    except (sufr_amd.SufrHipError, torch.OutOfMemoryError) as e:
        if isinstance(e, sufr_amd.SufrHipError) and e.code != -4:
            raise
        pytest.skip(f"not enough free HBM for a text of {lay.n} bytes: {e}")
    ut = np.uint32 if width == 4 else np.uint64
    assert db.stats.text_len == lay.n
    return sa.cpu().numpy().view(ut), lcp.cpu().numpy().view(ut)


def windows(db, geometry, lay, margin=0, retry=0):
    """the window settings of a windowed geometry; asserts in Python that the cut lies where the geometry says"""
    geo = hb.GEOMETRIES[geometry]
    window = geo.window or (1 << 31 if margin else 0)         # (a margin of the caller's needs a window of the caller's: the same cut)
    H, m, num = hb.check_plan(geo, lay, margin, window)
    if window:
        db.ctx.set_window(window, margin)
    db.ctx.set_window_retry(retry)
    assert lay.n >= hb.LIMIT or (window and lay.n > window)   # what sends a text to the windowed build
    return H, m, num


def context_text(ctx, lo, length):
    """bytes [lo, lo + length) of the normalised text the context keeps after a one-window build (test_gpu_exceptions._context_text
    reads all n bytes: 2 to 4 GB here)"""
    L = sufr_amd.lib()
    dev = C.c_int(-1); t = C.c_void_p(); sa = C.c_void_p(); lcp = C.c_void_p()
    L.sufr_hip_resident_arrays_.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.sufr_hip_resident_arrays_.restype = C.c_int
    ctx.check(L.sufr_hip_resident_arrays_(ctx.handle, C.byref(dev), C.byref(t), C.byref(sa), C.byref(lcp)))
    ctx.synchronize()
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]; hip.hipMemcpy.restype = C.c_int
    out = np.zeros(length, dtype=np.uint8)
    assert hip.hipMemcpy(out.ctypes.data, t.value + lo, length, 2) == 0      # hipMemcpyDeviceToHost
    return out


# ---------------------------------------------------------------------------------------------------------------------
# one window
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("geometry", ONE_WINDOW)
def test_left_over_chain_tie_level_and_doubling(db, geometry, width):
    """text (a): the left-over chain on the helper pipeline and behind the tie runs; prefix doubling (rank and position buffers
    indexed by position) in both"""
    hb.assert_region_is_not_empty("a")
    wsa, wlcp, lay = hb.expected("a", "plain", geometry, width)
    x, _ = hb.fill(geometry, "a")
    for overlap_min, helper in ((1, 1), (NEVER, 0)):
        db.ctx.set_overlap_min(overlap_min)
        sa, lcp = sort(db, x, lay, width)
        st = db.stats
        assert db.ctx.overlapped == helper and db.ctx.doublings >= 1, (db.ctx.overlapped, db.ctx.doublings)
        assert st.num_levels > 1 and st.partition_variant == 3 and st.bits_per_char == 3 and st.num_exceptions == 0
        assert lay.n >= 1 << 25                               # (the partition kernel's 1024-thread tiles)
        hb.same(sa, lcp, wsa, wlcp, f"text (a) at {geometry}, width {width}, helper {helper}")


@pytest.mark.parametrize("geometry,width", [("across_2_31", 4), ("top_single", 8)])
def test_run_bucket(db, geometry, width):
    """text (b): the bucket T^21 of 2^20 records and more, ordered in closed form; at across_2_31 its runs lie on both sides of 2^31"""
    hb.assert_region_is_not_empty("b")
    wsa, wlcp, lay = hb.expected("b", "plain", geometry, width)
    x, _ = hb.fill(geometry, "b")
    db.ctx.set_overlap_min(1)
    sa, lcp = sort(db, x, lay, width)
    # (no getter tells of the closed-form order: assert_region_is_not_empty has counted the bucket's 2^20 records, its threshold)
    assert db.ctx.doublings >= 1 and db.ctx.overlapped == 1 and db.stats.partition_variant == 3
    hb.same(sa, lcp, wsa, wlcp, f"text (b) at {geometry}, width {width}")


@pytest.mark.parametrize("geometry,width", [("across_2_31", 8), ("top_single", 4)])
def test_listed_bytes(db, geometry, width):
    """text (d): 30 bytes outside the DNA table on both sides of the boundary, re-placed by whole-text comparison"""
    hb.assert_region_is_not_empty("d")
    wsa, wlcp, lay = hb.expected("d", "plain", geometry, width)
    x, _ = hb.fill(geometry, "d")
    db.ctx.set_overlap_min(1)
    sa, lcp = sort(db, x, lay, width)
    st = db.stats
    assert st.num_exceptions == 30 and st.bits_per_char == 3 and st.num_reinserted >= 1 and db.ctx.exc_retry == 0
    hb.same(sa, lcp, wsa, wlcp, f"text (d) at {geometry}, width {width}")


@pytest.mark.parametrize("geometry,width,L", [("across_2_31", 4, 12), ("top_single", 8, 12), ("across_2_31", 8, 16), ("top_single", 4, 16),
                                              ("across_2_31", 4, 30), ("top_single", 8, 30)])
def test_capped_builds(db, geometry, width, L):
    """-m 12 and 16: built directly, keys of L characters and the top of the complemented 32-bit position; -m 30: the exact build,
    then apply_max_query_len.  Both: the canonical member of the family -- ties in descending position, which the shift keeps."""
    wsa, wlcp, lay = hb.expected("a", "plain", geometry, width)
    csa, clcp = canonical(wsa, wlcp, L)
    assert int((clcp >= L).sum()) > 100_000
    x, _ = hb.fill(geometry, "a")
    db.ctx.set_overlap_min(1)
    sa, lcp = sort(db, x, lay, width, max_query_len=L)
    if L <= 21:
        assert db.stats.chars_per_key == L and db.ctx.doublings == 0
    else:
        assert db.stats.chars_per_key < L and db.ctx.doublings >= 1
    hb.same(sa, lcp, csa, clcp, f"text (a) at {geometry}, width {width}, -m {L}")


@pytest.mark.parametrize("geometry,width", [("across_2_31", 4), ("top_single", 8)])
def test_seed_mask(db, geometry, width):
    """sort_masked: care symbols in order, equal ones in descending position"""
    hb.assert_region_is_not_empty("a", "mask")
    wsa, wlcp, lay = hb.expected("a", "mask", geometry, width)
    x, _ = hb.fill(geometry, "a")
    sa, lcp = sort(db, x, lay, width, seed_mask=hb.MASK)
    assert int(lcp.max()) == hb.MASK.count("1") and db.stats.num_suffixes == wsa.size
    hb.same(sa, lcp, wsa, wlcp, f"text (a) at {geometry}, width {width}, seed mask")


@pytest.mark.parametrize("geometry,width", [("across_2_31", 4), ("top_single", 8)])
def test_three_shards_and_the_stitch(db, geometry, width):
    """text (d) as three first-digit shards: they concatenate to the one-shard arrays, and the device stitch gives shards 1 and 2
    the oracle's LCP at their first rank (the rank the sharded tests elsewhere leave out)"""
    wsa, wlcp, lay = hb.expected("d", "plain", geometry, width)
    x, _ = hb.fill(geometry, "d")
    db.ctx.set_overlap_min(1)
    parts, rows, off = [], [], 0
    for r in range(3):
        cap = lay.x_len + 64
        dt = torch.int32 if width == 4 else torch.int64
        out_sa = torch.zeros(cap, dtype=dt, device="cuda"); out_lcp = torch.zeros(cap, dtype=dt, device="cuda")
        try:
            psa, plcp = db.sort(x, is_dna=True, index_width=width, shard_index=r, num_shards=3, out_sa=out_sa, out_lcp=out_lcp)
        except sufr_amd.SufrHipError as e:
            if e.code != -4:
                raise
            pytest.skip(f"not enough free HBM for a text of {lay.n} bytes: {e}")
        k = psa.numel()
        assert k > 0 and db.stats.num_exceptions == 30
        rows.append(shards.gather_boundaries_device(psa, k))
        if r:
            bounds = torch.cat(rows).contiguous()
            shards.stitch_device(db.ctx, lay.n, bounds, r, plcp)
            db.ctx.synchronize()
            assert int(plcp[0]) == int(wlcp[off]), f"shard {r}: stitched first LCP {int(plcp[0])}, the oracle has {int(wlcp[off])} at rank {off}"
        ut = np.uint32 if width == 4 else np.uint64
        parts.append((psa.cpu().numpy().view(ut), plcp.cpu().numpy().view(ut)))
        off += k
    hb.same(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), wsa, wlcp, f"text (d) in 3 shards at {geometry}")


@pytest.mark.parametrize("geometry", ONE_WINDOW)
def test_soft_masked_text_aligned_and_misaligned(db, geometry):
    """raw_text with and without --ignore-softmask, the device text at a 16-byte aligned address and one byte behind it (the
    staging copy in front of the text stage): the arrays at both widths, and the context's text over the region (the 64-bit entry
    point leaves it with the context)"""
    raw, _ = hb.region("soft")
    for soft in (False, True):
        hb.assert_region_is_not_empty("soft", "plain", False, soft)
        norm = hb.normalised("soft", soft)
        for offset, width in ((0, 8), (1, 8), (1, 4), (0, 4)):
            wsa, wlcp, lay = hb.expected("soft", "plain", geometry, width, soft)
            x, _ = hb.fill(geometry, "soft", offset)
            assert x.data_ptr() % 16 == offset
            sa, lcp = sort(db, x, lay, width, raw_text=True, ignore_softmask=soft)
            assert db.stats.num_exceptions == 0 and db.stats.bits_per_char == 3
            hb.same(sa, lcp, wsa, wlcp, f"soft-masked text at {geometry}, width {width}, ignore_softmask={soft}, offset {offset}")
            if width == 8:
                got = context_text(db.ctx, lay.F - 64, 64 + raw.size)
                assert np.array_equal(got[64:], norm) and bool((got[:64] == hb.N).all())


def test_host_buffer_entry_point():
    """sufr_hip_build_u32 on a host text whose region lies across 2^31: arrays, normalised text, and 'N' everywhere in front"""
    from sufr_amd.types import SufrBuilderArgs
    raw, at = hb.region("a")
    wsa, wlcp, lay = hb.expected("a", "plain", "across_2_31", 4)
    text = np.full(lay.n, hb.N, dtype=np.uint8)
    text[lay.F:] = raw
    try:
        b = sufr_amd.SufrBuilder(SufrBuilderArgs(text=text, is_dna=True), write=False)
    except sufr_amd.SufrHipError as e:
        if e.code != -4:
            raise
        pytest.skip(f"not enough free HBM for a text of {lay.n} bytes: {e}")
    assert b.index_width == 4 and b.num_suffixes == wsa.size and b.stats.partition_variant == 3
    hb.same(b.suffix_array, b.lcp, wsa, wlcp, "text (a) across 2^31 through the host-buffer entry point")
    assert np.array_equal(b.text[lay.F:], raw)
    step = 1 << 26
    for lo in range(0, lay.F, step):
        assert int(b.text[lo:min(lo + step, lay.F)].min()) == hb.N == int(b.text[lo:min(lo + step, lay.F)].max()), f"text[{lo}:] is not all 'N'"


# ---------------------------------------------------------------------------------------------------------------------
# windows
# ---------------------------------------------------------------------------------------------------------------------
def test_first_windowed_length(wdb):
    """n = SUFR_MAX_TEXT_LEN: one byte more than top_single, the default plan, 32-bit output; the first window holds no suffix"""
    wsa, wlcp, lay = hb.expected("a", "plain", "first_windowed", 4)
    x, _ = hb.fill("first_windowed", "a")
    H, m, num = windows(wdb, "first_windowed", lay)
    wdb.ctx.set_overlap_min(1)
    sa, lcp = sort(wdb, x, lay, 4)
    assert wdb.ctx.window_repairs == 0 and wdb.ctx.doublings >= 1 and wdb.ctx.overlapped == 1
    assert wdb.stats.partition_variant == 0                    # (the stats start from window 0's, which returned after its text pass)
    hb.same(sa, lcp, wsa, wlcp, "text (a) at first_windowed")


@pytest.mark.parametrize("geometry", CUTS)
def test_windows_with_a_margin_over_the_longest_lcp(wdb, geometry):
    width = hb.GEOMETRIES[geometry].width
    wsa, wlcp, lay = hb.expected("a", "plain", geometry, width)
    x, _ = hb.fill(geometry, "a")
    windows(wdb, geometry, lay, 0 if geometry == "u32_cut_2_31" else WIDE_MARGIN)       # (u32_cut_2_31: the default plan, margin 2^26)
    wdb.ctx.set_overlap_min(1)
    sa, lcp = sort(wdb, x, lay, width)
    assert wdb.ctx.window_repairs == 0 and wdb.ctx.doublings >= 1
    hb.same(sa, lcp, wsa, wlcp, f"text (a) at {geometry}")


@pytest.mark.parametrize("geometry", CUTS)
def test_windows_whose_margin_ends_inside_a_repeat(wdb, geometry):
    """margin 64 and a re-build margin capped at 500, inside the copy of S that the cut goes through: its suffixes are ordered by
    whole-text comparison with 64-bit positions and merged back"""
    width = hb.GEOMETRIES[geometry].width
    wsa, wlcp, lay = hb.expected("a", "plain", geometry, width)
    x, _ = hb.fill(geometry, "a")
    windows(wdb, geometry, lay, 64, 500)
    sa, lcp = sort(wdb, x, lay, width)
    assert wdb.ctx.window_repairs > 0
    hb.same(sa, lcp, wsa, wlcp, f"text (a) at {geometry}, margin 64, retry 500")


@pytest.mark.parametrize("geometry", CUTS)
def test_windows_with_listed_bytes(wdb, geometry):
    width = hb.GEOMETRIES[geometry].width
    wsa, wlcp, lay = hb.expected("d", "plain", geometry, width)
    x, _ = hb.fill(geometry, "d")
    windows(wdb, geometry, lay, WIDE_MARGIN)
    sa, lcp = sort(wdb, x, lay, width)
    assert wdb.ctx.window_repairs == 0 and wdb.ctx.exc_retry == 0 and wdb.ctx.exc_taken >= 1
    hb.same(sa, lcp, wsa, wlcp, f"text (d) at {geometry}")


@pytest.mark.parametrize("geometry", CUTS)
def test_windows_capped_and_masked(wdb, geometry):
    """-m 16 (ties in descending position over the WHOLE text) and the seed mask (windows built with it, merged under it)"""
    width = hb.GEOMETRIES[geometry].width
    wsa, wlcp, lay = hb.expected("a", "plain", geometry, width)
    csa, clcp = canonical(wsa, wlcp, 16)
    msa, mlcp, _ = hb.expected("a", "mask", geometry, width)
    x, _ = hb.fill(geometry, "a")
    windows(wdb, geometry, lay, WIDE_MARGIN)
    sa, lcp = sort(wdb, x, lay, width, max_query_len=16)
    assert wdb.ctx.doublings == 0
    hb.same(sa, lcp, csa, clcp, f"text (a) at {geometry}, -m 16")
    sa, lcp = sort(wdb, x, lay, width, seed_mask=hb.MASK)
    assert int(lcp.max()) == hb.MASK.count("1")
    hb.same(sa, lcp, msa, mlcp, f"text (a) at {geometry}, seed mask")


@pytest.mark.parametrize("geometry", CUTS)
def test_windows_in_two_shards(wdb, geometry):
    """two shards of the windowed build (ranges of the first 8 bytes): their concatenation, but for the second one's first LCP"""
    width = hb.GEOMETRIES[geometry].width
    wsa, wlcp, lay = hb.expected("a", "plain", geometry, width)
    x, _ = hb.fill(geometry, "a")
    windows(wdb, geometry, lay, WIDE_MARGIN)
    parts = [sort(wdb, x, lay, width, shard_index=r, num_shards=2) for r in range(2)]
    sizes = [p[0].size for p in parts]
    assert min(sizes) > 0
    hb.same(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), wsa, wlcp, f"text (a) at {geometry}, 2 shards", sizes)
