"""The precondition of tests/test_gpu_build_high_positions.py, on the CPU (tests/high_build.py has the argument): the oracle's
arrays of a region X do not depend on how many 'N' stand in front of it or, beyond |X| of them, behind it.

For every region and for the plain order and the seed mask, the arrays of

    X . N^|X| . $        X . N^(2|X| + 37) . $        N^4096 . X . N^|X| . $

are equal after the shift (positions of X by the filler, the '$' suffix to the last byte), and those of N^4096 . X (X ending in
'$' and ending the text) equal those of X.  The first twin of each pair is the cached one the device tests expect from; the
other side is a fresh oracle run in its own coordinates, so a wrong `shifted` fails here."""
import time

import numpy as np
import pytest

import high_build as hb

CASES = [("a", False), ("d", False), ("b", False), ("soft", False), ("soft", True)]


@pytest.mark.parametrize("order", hb.ORDERS)
@pytest.mark.parametrize("name,ignore_softmask", CASES)
def test_arrays_are_invariant_under_filler_and_tail(name, ignore_softmask, order):
    t0 = time.perf_counter()
    norm = hb.normalised(name, ignore_softmask)
    x_len = norm.size - 1
    hb.assert_region_is_not_empty(name, order, True, ignore_softmask)
    hb.assert_region_is_not_empty(name, order, False, ignore_softmask)
    base_sa, base_lcp = hb.twin_arrays(name, order, True, ignore_softmask)
    assert int(base_lcp[0]) == 0 and int(base_sa[0]) == 2 * x_len
    for filler, tail in ((0, 2 * x_len + 37), (4096, x_len)):
        text = hb.twin_text(norm, True, filler, tail)
        sa, lcp = hb.oracle_arrays(text, order)
        want = hb.shifted(base_sa, x_len, filler, text.size, True)
        hb.same(sa, lcp, want, base_lcp, f"region {name}, {order}: filler {filler}, tail {tail}")
        assert int(sa[0]) == text.size - 1 and int(np.sort(sa)[-2]) < filler + x_len
    end_sa, end_lcp = hb.twin_arrays(name, order, False, ignore_softmask)
    text = hb.twin_text(norm, False, 4096)
    sa, lcp = hb.oracle_arrays(text, order)
    hb.same(sa, lcp, hb.shifted(end_sa, norm.size, 4096, text.size, False), end_lcp, f"region {name}, {order}: filler 4096, no tail")
    print(f"region {name} (ignore_softmask={ignore_softmask}), {order}: {time.perf_counter() - t0:.2f} s")


def test_every_geometry_lays_out_every_region():
    """F, T, n and the windows of every geometry x region: the boundary byte lies where the geometry says, the tail is at least
    as long as the region, and the windows are cut where the device tests expect them"""
    for geo in hb.GEOMETRIES.values():
        for name in ("a", "b", "d", "soft"):
            raw, at = hb.region(name)
            lay = hb.layout(geo, raw.size, at)
            assert lay.n < hb.LIMIT or geo.windowed
            if geo.boundary is not None:
                assert lay.F + at == geo.boundary
            if geo.windowed:
                hb.check_plan(geo, lay)
            if geo.window:
                hb.check_plan(geo, lay, 64)
    assert hb.plan((1 << 32) - 2) == (1 << 31, 1 << 26, 2) and hb.plan(3 << 31, 1 << 31, 1 << 16) == (1 << 31, 1 << 16, 3)
    assert hb.plan(hb.LIMIT)[2] == 2
