"""Batches that do not start at byte 0 of their buffer.  The headers define query i as bytes [offsets[i], offsets[i + 1])
of the batch, so offsets[0] may be anything; the one place of the device drivers that reads offsets[0] is the shared batch
helper of sufr_search.inc (batch_extent / double_batch), and no other test passes such a batch.

The recipe: 24 reads of 60 .. 83 bytes cut from tests/golden/expected/long_dna_sequence.sufr, each with one substitution,
every third one also with one byte deleted; behind them the reverse complements of six of them, so that a search of both
strands has records on strand 1 (their traceback runs on the doubled batch; the records of strand 0 run on the batch as it
is, from g0 = offsets[0] != 0).  The reads are packed once from offset 0 and once behind 5 junk bytes.

Host half (no GPU): MEMs, k-mismatch, k-difference with every flag combination and the traceback of the k-difference
records give identical arrays for the two packings, and no leg is empty.  GPU half: the *_device entry points and the
host-buffer entry points on the shifted packing equal the host path."""
import ctypes as C

import numpy as np
import pytest

import sufr_amd
from sufr_amd import DeviceIndex, SufrFile
from oracle_helper import GOLDEN

SUFR = GOLDEN / "expected" / "long_dna_sequence.sufr"
JUNK = b"TTAGC"                                                  # offsets[0] == 5; DNA, so a driver that read it would find matches
MIN_LEN, D = 12, 2
_COMP = {65: 67, 67: 71, 71: 84, 84: 65}                          # the substitution: A -> C -> G -> T -> A
_RC = bytes.maketrans(b"ACGT", b"TGCA")


def _reads(text: np.ndarray):
    reads, at = [], 97
    for i in range(24):
        m = 60 + i
        while not all(c in b"ACGT" for c in bytes(text[at:at + m])):
            at += 1
        r = bytearray(bytes(text[at:at + m]))
        at += 811
        s = (7 * i + 11) % m
        r[s] = _COMP[r[s]]
        if i % 3 == 0:
            del r[m // 2]
        reads.append(bytes(r))
    return reads + [reads[i].translate(_RC)[::-1] for i in range(1, 24, 4)]


def _pack(reads, junk: bytes):
    qb = np.frombuffer(junk + b"".join(reads), dtype=np.uint8).copy()
    off = np.cumsum([len(junk)] + [len(r) for r in reads]).astype(np.uint64)
    return qb, off


@pytest.fixture(scope="module")
def case():
    """The file, the two packings and the host answers on the shifted one, computed once: legs[name] = arrays."""
    f = SufrFile(SUFR)
    reads = _reads(np.asarray(f.text))
    assert len(reads) == 30 and 59 <= min(map(len, reads)) and max(map(len, reads)) <= 83
    plain, shifted = _pack(reads, b""), _pack(reads, JUNK)
    assert plain[1][0] == 0 and shifted[1][0] == 5

    def legs(qb, off):
        out = {}
        for both in (False, True):
            out["mems", both] = f.mem_arrays(qb, off, MIN_LEN, 0, both)
            out["approx", both] = f.approx_arrays(qb, off, D, 0, both)
            for minima in (False, True):
                recs = f.edit_arrays(qb, off, D, 0, both, minima)
                out["edit", both, minima] = recs
                out["trace", both, minima] = f.edit_trace_arrays(qb, off, *recs)
        return out
    return f, shifted, legs(*plain), legs(*shifted)


def _same(got, want):
    return len(got) == len(want) and all(np.array_equal(np.asarray(a).view(np.asarray(b).dtype), b) for a, b in zip(got, want))


def test_host_answers_do_not_depend_on_where_the_batch_starts(case):
    _, _, plain, shifted = case
    assert plain.keys() == shifted.keys() and len(plain) == 12
    for leg, want in plain.items():
        print(leg, "records:", len(want[0]))
        assert len(want[0]) > 0, leg
        assert _same(shifted[leg], want), leg
    for minima in (False, True):                                 # both strands: records on either strand
        strand = shifted["edit", True, minima][1]
        assert (strand == 1).any() and (strand == 0).any()
    assert (shifted["approx", True][1] == 1).any() and (shifted["mems", True][2] == 1).any()


# ---- GPU half ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device(case):
    import torch
    f, (qb, off), _, _ = case
    ctx = sufr_amd.Context(0)
    ix = DeviceIndex.load(ctx, f)
    yield ctx, ix, torch.from_numpy(qb).cuda(), torch.from_numpy(off.astype(np.int64)).cuda()
    ix.close()
    ctx.close()


def _np(tensors):
    return [t.cpu().numpy() for t in tensors]


def _host_buffers(ctx, fn, qb, off, args, want):
    """A host-buffer entry point with room for exactly the records the host path found."""
    out = [np.zeros(max(len(a), 1), dtype=a.dtype) for a in want]
    total = C.c_uint64(0)
    ctx.check(fn(ctx.handle, qb.ctypes.data, off.ctypes.data, len(off) - 1, *args, len(want[0]), *[a.ctypes.data for a in out], C.byref(total)))
    return [a[:total.value] for a in out]


@pytest.mark.gpu
@pytest.mark.parametrize("both", [False, True])
def test_device_mems_and_approx_on_a_shifted_batch(case, device, both):
    _, (qb, off), _, want = case
    ctx, ix, dq, dv = device
    L = sufr_amd.lib()
    assert _same(_np(ix.mems_device(dq, dv, MIN_LEN, 0, both)), want["mems", both])
    assert _same(_np(ix.approx_device(dq, dv, D, 0, both)), want["approx", both])
    h = ix._h
    assert _same(_host_buffers(ctx, lambda c, *a: L.sufr_hip_mems(c, h, *a), qb, off, (MIN_LEN, 0, int(both)), want["mems", both]),
                 want["mems", both])
    assert _same(_host_buffers(ctx, lambda c, *a: L.sufr_hip_approx(c, h, *a), qb, off, (D, 0, int(both)), want["approx", both]),
                 want["approx", both])


@pytest.mark.gpu
@pytest.mark.parametrize("both,minima", [(False, False), (False, True), (True, False), (True, True)])
def test_device_edit_and_trace_on_a_shifted_batch(case, device, both, minima):
    _, (qb, off), _, want = case
    ctx, ix, dq, dv = device
    L = sufr_amd.lib()
    recs, trace = want["edit", both, minima], want["trace", both, minima]
    drecs = [t.contiguous() for t in ix.edit_device(dq, dv, D, 0, both, minima)]
    assert _same(_np(drecs), recs)
    assert _same(_np(ix.edit_trace_device(dq, dv, *drecs)), trace)          # strand 1 with both: the doubled batch; else g0 = 5
    h = ix._h
    assert _same(_host_buffers(ctx, lambda c, *a: L.sufr_hip_edit(c, h, *a), qb, off, (D, 0, int(both) | 2 * int(minima)), recs), recs)
    assert _same(ix.edit_trace(qb, off, *recs), trace)
