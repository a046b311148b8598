"""Build paths at text positions beyond 2^31 and 2^32 without a multi-gigabyte oracle run (a helper, not a test module).

A --dna build without --allow-ambiguity does not index 'N'.  So a text can be laid out as

    N^F . X . N^T . $        (T = 0: X itself ends in '$' and ends the text)

where X is one of the 1-3 MB regions that reach the deep paths at small size (test_gpu_overlap.py: left-over buckets, tie groups
and prefix doubling, a run bucket, listed bytes).  The build then costs a text pass over F + T bytes of 'N' plus the build of X;
the working arrays are sized by the number of suffixes.

The twin of the layout.  Suffix comparison never looks left of a suffix's start.  X ends in a byte other than 'N' and T >= |X|:
of two suffixes of X the later one reaches the tail first, and the earlier one has, inside those T tail bytes, X's last byte
against an 'N' -- every comparison between two suffixes of X is decided inside X or within its first |X| tail bytes.  So SA and
LCP of the layout are the CPU oracle's arrays of the twin  X . N^|X| . $  (T = 0: of X alone), every position below |X| shifted
by F and the one '$' suffix (rank 0, LCP 0) mapped to n - 1.  tests/test_build_high_witness.py checks exactly that on the CPU,
for every region and both orders; capped builds (-m) are compared with canonical(exact arrays, L), because the oracle's own -m
build is one member of the reference's family and not invariant, while "descending position" is.

  region(name)      raw bytes of a region and the byte of it that lands on a geometry's boundary
  GEOMETRIES        across_2_31, top_single (one window); first_windowed, u32_cut_2_31, u64_cut_2_32, u64_cut_2_31 (windows)
  layout()          F, T, n of a geometry for a region; plan()  the windows the build will cut, as sufr_wide.inc computes them
  twin_arrays()     the oracle's arrays of the twin, cached per region, order and tail; shifted()  the mapping of positions
  expected()        the shifted arrays at the index width
  fill()            the layout in one reusable device buffer
  same()            exact equality of whole arrays; names the first differing rank
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

N = ord("N")
MASK = "111010010100110111"
LIMIT = 0xFFFFFFFF - (1 << 24)          # SUFR_MAX_TEXT_LEN (sufr_launch.inc): texts of this length and more are built in windows
WIDE_MAX_WINDOWS = 64
MIN_TIES_ACROSS = 100                   # ranks with LCP >= 64 whose two neighbours lie on opposite sides of the boundary
ORDERS = ("plain", "mask")


# ---------------------------------------------------------------------------------------------------------------------
# the regions
# ---------------------------------------------------------------------------------------------------------------------
SOFT_LEN = 70_001
SOFT_SEG, SOFT_AT = 3_000, (2_000, 20_000, SOFT_LEN // 2 - 1_500, 50_000, 66_000)      # one segment: before, across, after the middle


@functools.lru_cache(maxsize=None)
def soft_text():
    """70 001 symbols of ACGTacgtN ending in '$', with five copies of a 3 000-symbol segment (bytes and case alike) of which
    one lies across the middle: with and without --ignore-softmask there are long ties on both sides of it"""
    rng = np.random.default_rng(2301)
    t = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)[rng.choice(9, SOFT_LEN, p=[.17, .17, .17, .17, .07, .07, .07, .07, .04])].copy()
    seg = np.frombuffer(b"ACGTacgt", dtype=np.uint8)[rng.choice(8, SOFT_SEG, p=[.2, .2, .2, .2, .05, .05, .05, .05])].copy()
    seg[:400] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 400)]           # (under --ignore-softmask lower case is 'N')
    for at in SOFT_AT:
        t[at:at + SOFT_SEG] = seg
    t[-2] = ord("C"); t[-1] = ord("$")
    t.setflags(write=False)
    return t


def _t_run_in_the_appended_part(raw, start):
    """the middle of the run of 'T' (21 symbols or more) nearest to the middle of raw[start:]"""
    is_t = np.concatenate([[0], (raw[start:] == ord("T")).astype(np.int8), [0]])
    d = np.diff(is_t)
    lo, hi = np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]
    long_runs = np.nonzero(hi - lo >= 100)[0]
    k = long_runs[np.argmin(np.abs((lo + hi)[long_runs] // 2 - (raw.size - start) // 2))]
    return start + int(lo[k] + hi[k]) // 2


@functools.lru_cache(maxsize=None)
def region(name):
    """(raw bytes ending in '$', the index of the byte that lands on the boundary).  "a", "b", "d": the texts of
    test_gpu_overlap.py; "soft": soft_text()."""
    if name == "soft":
        return soft_text(), SOFT_LEN // 2
    import test_gpu_overlap as ov
    raw_a, _, s_at = ov.text_a()
    mid_of_s = int(s_at[150]) + 1000                                   # the middle of a copy of S: copies of S and of F on both sides
    if name == "a":
        return raw_a, mid_of_s
    if name == "d":
        return ov.text_d(), mid_of_s
    if name == "b":
        raw = ov.text_b()
        at = _t_run_in_the_appended_part(raw, raw_a.size - 1)
        assert raw[at] == ord("T") and at > raw_a.size
        return raw, at
    raise KeyError(name)


def normalised(name, ignore_softmask=False):
    raw = region(name)[0]
    if name != "soft":
        return raw
    from oracle_helper import Oracle
    return Oracle().normalize(raw, ignore_softmask)


# ---------------------------------------------------------------------------------------------------------------------
# the geometries
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Geometry:
    name: str
    windowed: bool
    n: int | None               # None: the text ends with the region (n = boundary - at + |X|)
    boundary: int | None        # None: the region lies at the end of the text
    width: int | None           # None: both index widths
    window: int = 0             # set_window(window, margin): 0 = the default plan
    cut: int | None = None      # which window starts at the boundary


GEOMETRIES = {g.name: g for g in (
    Geometry("across_2_31", False, None, 1 << 31, None),
    Geometry("top_single", False, LIMIT - 1, None, None),
    Geometry("first_windowed", True, LIMIT, None, 4),
    Geometry("u32_cut_2_31", True, (1 << 32) - 2, 1 << 31, 4, 0, 1),
    Geometry("u64_cut_2_32", True, 3 << 31, 1 << 32, 8, 1 << 31, 2),
    Geometry("u64_cut_2_31", True, 3 << 31, 1 << 31, 8, 1 << 31, 1),
)}


@dataclass(frozen=True)
class Layout:
    F: int
    T: int
    n: int
    x_len: int                  # bytes of the region in the text: |X|, without its '$' when a tail follows

    @property
    def tailed(self):
        return self.T > 0


def layout(geo: Geometry, raw_len: int, at: int) -> Layout:
    """F, T, n: byte `at` of the region lies on the geometry's boundary; without a boundary the region ends the text"""
    if geo.boundary is None:
        lay = Layout(geo.n - raw_len, 0, geo.n, raw_len)
    elif geo.n is None:
        lay = Layout(geo.boundary - at, 0, geo.boundary - at + raw_len, raw_len)
    else:
        F = geo.boundary - at
        lay = Layout(F, geo.n - 1 - F - (raw_len - 1), geo.n, raw_len - 1)
        assert lay.T >= lay.x_len, "the tail is shorter than the region: the twin argument does not hold"
    assert lay.F > 0 and lay.F + lay.x_len + lay.T + (1 if lay.T else 0) == lay.n
    assert (lay.n >= LIMIT) == geo.windowed or geo.window, (geo.name, lay.n)
    return lay


def plan(n: int, window: int = 0, margin: int = 0):
    """(H, margin, windows) as wide_plan (sufr_wide.inc) cuts a text of n bytes: equal windows, as few as fit, bases 16-aligned"""
    limit = LIMIT - 1
    m = margin or 1 << 26
    if window:
        window = min(window, limit - 1)
        m = min(m, limit - window)
    else:
        m = min(m, limit // 2)
        window = limit - m
    cnt = -(-n // window)
    H = (-(-n // cnt) + 15) & ~15
    num = -(-n // H)
    assert num <= WIDE_MAX_WINDOWS
    return H, m, num


def check_plan(geo: Geometry, lay: Layout, margin: int = 0, window: int | None = None):
    """the plan arithmetic of a windowed geometry (window: what set_window is given, if not the geometry's): a change to
    wide_plan fails here instead of moving the cut into the filler"""
    H, m, num = plan(lay.n, geo.window if window is None else window, margin)
    if geo.cut is None:                                                # first_windowed: two windows, the first one all filler
        assert num == 2 and H <= lay.F, (geo.name, H, num, lay)
    else:
        assert num == (3 if lay.n == 3 << 31 else 2) and H == 1 << 31 and geo.cut * H == geo.boundary, (geo.name, H, num)
        assert lay.F < geo.boundary < lay.F + lay.x_len
    return H, m, num


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's arrays of the twin
# ---------------------------------------------------------------------------------------------------------------------
def twin_text(norm: np.ndarray, tailed: bool, filler: int = 0, tail: int | None = None) -> np.ndarray:
    """N^filler . X . N^tail . $ (tail: |X| unless given), or N^filler . X for a region that ends the text"""
    assert norm[-1] == ord("$") and norm[-2] != N
    if not tailed:
        return np.concatenate([np.full(filler, N, np.uint8), norm])
    x = norm[:-1]
    tail = x.size if tail is None else tail
    assert tail >= x.size
    return np.concatenate([np.full(filler, N, np.uint8), x, np.full(tail, N, np.uint8), np.frombuffer(b"$", dtype=np.uint8)])


def oracle_arrays(text: np.ndarray, order: str):
    from oracle_helper import Oracle
    sa, lcp, _ = Oracle().build(text, is_dna=True, seed_mask=MASK if order == "mask" else None, threads=8)
    return sa.astype(np.uint64), lcp.astype(np.uint64)


@functools.lru_cache(maxsize=None)
def twin_arrays(name: str, order: str, tailed: bool, ignore_softmask: bool = False):
    """the oracle's SA and LCP (uint64) of the region's twin, built once per region, order and tail.  The untailed plain arrays
    of "a", "b" and "d" are test_gpu_overlap.want's: one oracle run serves both modules."""
    assert order in ORDERS
    if name != "soft" and order == "plain" and not tailed:
        import test_gpu_overlap as ov
        sa, lcp = ov.want(name)
        sa, lcp = sa.astype(np.uint64), lcp.astype(np.uint64)
    else:
        sa, lcp = oracle_arrays(twin_text(normalised(name, ignore_softmask), tailed), order)
    sa.setflags(write=False); lcp.setflags(write=False)
    return sa, lcp


def shifted(sa: np.ndarray, x_len: int, F: int, n: int, tailed: bool, twin_filler: int = 0, twin_n: int | None = None):
    """positions of a twin -> positions of the layout: the region's by F (less the twin's own filler); with a tail, the '$'
    suffix -- the last byte of the twin, rank 0 -- to n - 1"""
    sa = sa.astype(np.uint64)
    out = sa - np.uint64(twin_filler) + np.uint64(F)
    if tailed:
        twin_n = 2 * x_len + 1 + twin_filler if twin_n is None else twin_n
        sentinel = sa == np.uint64(twin_n - 1)
        assert int(sentinel.sum()) == 1 and bool(sentinel[0]), "the twin's '$' suffix is not rank 0"
        assert bool((sa[~sentinel] < twin_filler + x_len).all())
        out[sentinel] = np.uint64(n - 1)
    return out


def ties_across(sa: np.ndarray, lcp: np.ndarray, at: int, min_lcp: int = 64) -> int:
    """ranks with LCP >= min_lcp whose suffix and the one before it start on opposite sides of byte `at` of the region"""
    left = sa < np.uint64(at)
    return int(((lcp[1:] >= np.uint64(min_lcp)) & (left[1:] != left[:-1])).sum())


def assert_region_is_not_empty(name: str, order: str = "plain", tailed: bool = False, ignore_softmask: bool = False):
    """from the oracle's arrays alone: more than 100 ranks tie over 64 symbols and more across the boundary byte; text (d) has
    listed bytes on both sides of it"""
    raw, at = region(name)
    sa, lcp = twin_arrays(name, order, tailed, ignore_softmask)
    k = ties_across(sa, lcp, at, 64 if order == "plain" else len([c for c in MASK if c == "1"]))
    assert k > MIN_TIES_ACROSS, f"region {name}, {order}: only {k} long ties across the boundary byte"
    if name == "d":
        listed = np.nonzero(~np.isin(raw, np.frombuffer(b"$ACGNT", dtype=np.uint8)))[0]
        assert listed.size == 30 and (listed < at).any() and (listed > at).any()
    if name == "b":                                                    # the T^21 bucket has its 2^20 records, on both sides
        t21 = np.convolve((raw == ord("T")).astype(np.int32), np.ones(21, np.int32), "valid") == 21
        assert int(t21.sum()) >= 1 << 20 and t21[:at - 21].sum() > 1000 and t21[at + 1:].sum() > 1000
    return k


def expected(name: str, order: str, geometry: str, width: int, ignore_softmask: bool = False):
    """(SA, LCP, layout) of the region in the geometry: the twin's arrays, shifted, at the index width"""
    geo = GEOMETRIES[geometry]
    raw, at = region(name)
    lay = layout(geo, raw.size, at)
    sa, lcp = twin_arrays(name, order, lay.tailed, ignore_softmask)
    sa = shifted(sa, lay.x_len, lay.F, lay.n, lay.tailed)
    assert int(sa.max()) == lay.n - 1 and int(sa.max()) >= 1 << 31
    if geo.boundary is not None:
        assert bool((sa < np.uint64(geo.boundary)).any()) and bool((sa >= np.uint64(geo.boundary)).any())
    assert geo.width in (None, width) and (width == 8 or lay.n < 0xFFFFFFFF)
    dt = np.uint32 if width == 4 else np.uint64
    return sa.astype(dt), lcp.astype(dt), lay


def same(got_sa, got_lcp, want_sa, want_lcp, what, sizes=None):
    """exact equality of whole arrays, the first differing rank in the message; sizes: shard sizes, whose first LCPs (the
    stitch's) are left out"""
    gsa, glcp = np.asarray(got_sa).astype(np.uint64), np.asarray(got_lcp).astype(np.uint64)
    wsa, wlcp = np.asarray(want_sa).astype(np.uint64), np.asarray(want_lcp).astype(np.uint64)
    assert gsa.size == wsa.size, f"{what}: {gsa.size} suffixes, the oracle has {wsa.size}"
    bad = np.nonzero(gsa != wsa)[0]
    assert bad.size == 0, f"{what}: SA differs at rank {bad[0]} of {wsa.size}: got {gsa[bad[0]]} want {wsa[bad[0]]} ({bad.size} ranks differ)"
    keep = np.ones(wsa.size, dtype=bool)
    if sizes is not None:
        starts = np.cumsum(sizes[:-1])
        keep[starts[starts < wsa.size]] = False
    bad = np.nonzero((glcp != wlcp) & keep)[0]
    assert bad.size == 0, f"{what}: LCP differs at rank {bad[0]} of {wsa.size}: got {glcp[bad[0]]} want {wlcp[bad[0]]} ({bad.size} ranks differ)"


# ---------------------------------------------------------------------------------------------------------------------
# the device text
# ---------------------------------------------------------------------------------------------------------------------
_slots = {}                             # text length -> [buffer, spans that are not 'N']; the two lengths used last are kept
SLACK = 64                              # room for a text that starts at a misaligned address


def fill(geometry: str, name: str, offset: int = 0):
    """(text of the layout as a device tensor of n bytes starting `offset` bytes into the buffer, layout).  A buffer of 'N' per
    text length (one torch.full); a later call writes 'N' over the region and '$' of the call before."""
    import torch
    geo = GEOMETRIES[geometry]
    raw, at = region(name)
    lay = layout(geo, raw.size, at)
    if lay.n not in _slots:
        while len(_slots) >= 2:
            del _slots[next(iter(_slots))]
            torch.cuda.empty_cache()
        _slots[lay.n] = [torch.full((lay.n + SLACK,), N, dtype=torch.uint8, device="cuda"), []]
    slot = _slots[lay.n] = _slots.pop(lay.n)                           # (the one used last goes to the end)
    buf = slot[0]
    for lo, hi in slot[1]:
        buf[lo:hi] = N
    x = torch.from_numpy(raw[:lay.x_len].copy()).cuda()
    buf[offset + lay.F:offset + lay.F + lay.x_len] = x
    slot[1] = [(offset + lay.F, offset + lay.F + lay.x_len)]
    if lay.tailed:
        buf[offset + lay.n - 1] = ord("$")
        slot[1].append((offset + lay.n - 1, offset + lay.n))
    torch.cuda.synchronize()
    return buf[offset:offset + lay.n], lay


def release():
    import torch
    _slots.clear()
    torch.cuda.empty_cache()
