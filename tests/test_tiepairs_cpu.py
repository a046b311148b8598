"""CPU checks of the tie-pair masks shared with the device code (sufr_amd/csrc/sufr_tiepairs.h): the slots that head a tie run
of exactly two members, from the member / head bitmaps of 128-rank windows, must be the ones a position-by-position scan of the
bit strings finds -- also where the run crosses a window's end (its second member is slot 0 of the next window and has no head
bit there) and where a longer run does."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def shim():
    out = ROOT / "tests" / "_build" / "libtiepairs_shim.so"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "tiepairs_shim.cpp"
    hdr = ROOT / "sufr_amd" / "csrc" / "sufr_tiepairs.h"
    if not out.exists() or out.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(out), str(src)], check=True)
    L = C.CDLL(str(out))
    L.shim_tie_pair_heads.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.shim_tie_pair_heads.restype = C.c_uint64
    return L


def to_words(member, head):
    """bit strings over 128 * nwin positions -> the tie bitmaps: per window M0 M1 H0 H1"""
    nwin = member.size // 128
    w = np.zeros(nwin * 4, dtype=np.uint64)
    for bits, at in ((member, 0), (head, 2)):
        for p in np.nonzero(bits)[0].tolist():
            w[(p // 128) * 4 + at + (p % 128) // 64] |= np.uint64(1) << np.uint64(p % 64)
    return w


def scan(member, head):
    """positions that head a run of exactly two, one position at a time: a run is a head (a member with the head bit) and the
    members without a head bit right behind it"""
    n = member.size
    out = []
    for p in range(n):
        if not (member[p] and head[p]):
            continue
        q = p + 1
        while q < n and member[q] and not head[q]:
            q += 1
        if q - p == 2:
            out.append(p)
    return out


def from_shim(shim, member, head):
    nwin = member.size // 128
    w = to_words(member, head)
    out = np.zeros(nwin * 2, dtype=np.uint64)
    total = shim.shim_tie_pair_heads(w.ctypes.data, nwin, out.ctypes.data)
    got = [i * 64 + b for i in range(nwin * 2) for b in range(64) if (int(out[i]) >> b) & 1]
    assert total == len(got)
    return got


def runs_to_bits(nwin, runs):
    """runs: (first position, members)"""
    member = np.zeros(nwin * 128, dtype=bool); head = np.zeros(nwin * 128, dtype=bool)
    for at, ln in runs:
        member[at:at + ln] = True
        head[at] = True
    return member, head


HAND = {
    "pair at 126/127": (2, [(126, 2)], [126]),
    "pair at 127/128 (crossing)": (2, [(127, 2)], [127]),
    "pair at 63/64": (2, [(63, 2)], [63]),
    "two adjacent pairs": (2, [(10, 2), (12, 2)], [10, 12]),
    "two adjacent pairs across the end": (2, [(125, 2), (127, 2)], [125, 127]),
    "pair, then a pair in the next window's first slots": (2, [(126, 2), (128, 2)], [126, 128]),
    "a triple": (2, [(40, 3)], []),
    "a triple whose third member sits in the next window": (2, [(126, 3)], []),
    "a triple whose second and third members sit in the next window": (2, [(127, 3)], []),
    "a triple across the words of a window": (2, [(62, 3)], []),
    "a lone head at the array's last rank": (2, [(255, 1)], []),
    "a pair at the array's last two ranks": (2, [(254, 2)], [254]),
    "a pair behind a triple": (3, [(250, 3), (253, 2), (255, 2)], [253, 255]),
    "a long run over three windows": (4, [(100, 300)], []),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_cases(shim, name):
    nwin, runs, want = HAND[name]
    member, head = runs_to_bits(nwin, runs)
    assert scan(member, head) == want                    # (the scan itself, against what the case says)
    assert from_shim(shim, member, head) == want


@pytest.mark.parametrize("seed", range(40))
def test_random_runs_equal_the_scan(shim, seed):
    """runs of 2 .. 6 members (two thirds of them pairs), often back to back, over 3 .. 5 windows"""
    rng = np.random.default_rng(seed)
    nwin = int(rng.integers(3, 6))
    n = nwin * 128
    runs, at = [], int(rng.integers(0, 4))
    while at < n:
        ln = 2 if rng.random() < 0.66 else int(rng.integers(3, 7))
        ln = min(ln, n - at)
        runs.append((at, ln))
        at += ln + (0 if rng.random() < 0.5 else int(rng.integers(1, 6)))
    member, head = runs_to_bits(nwin, runs)
    want = scan(member, head)
    assert len(want) > 10
    assert from_shim(shim, member, head) == want


@pytest.mark.parametrize("seed", range(20))
def test_random_masks_equal_the_scan(shim, seed):
    """any member and head masks (heads among the members), dense and sparse: the masks and the scan read them the same way"""
    rng = np.random.default_rng(100 + seed)
    nwin = int(rng.integers(3, 6))
    member = rng.random(nwin * 128) < (0.2, 0.5, 0.8, 0.95)[seed % 4]
    head = member & (rng.random(nwin * 128) < (0.3, 0.5, 0.7)[seed % 3])
    assert from_shim(shim, member, head) == scan(member, head)
