"""DNA texts with bytes outside {$ % A C G N T} (IUPAC ambiguity codes, another delimiter) keep the fixed 3-bit code table
(sufr_amd/csrc/sufr_exc.inc): the build runs on 'N' in their place and the suffixes whose comparisons reached such a byte are
re-placed by whole-text comparison.  Every case: whole SA and LCP equal the CPU oracle's (which compares raw bytes,
sufr_builder.rs:346-394), the normalised text handed back carries the original bytes, and the stats say the path was taken."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sufr_amd
from sufr_amd import synth

pytestmark = pytest.mark.gpu

IUPAC = np.frombuffer(b"RYKMSWBDHV", dtype=np.uint8)


def _acgt(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()


def _check(oracle, raw, *, expect_exceptions=True, shards=1, **kw):
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    db = sufr_amd.DeviceBuilder(0)
    x = torch.from_numpy(raw).cuda()
    sa, lcp = db.sort(x, raw_text=True, **kw)
    st = db.stats
    gsa = sa.cpu().numpy().view(np.uint32); glcp = lcp.cpu().numpy().view(np.uint32)
    norm = oracle.normalize(raw, kw.get("ignore_softmask", False))
    okw = {k: v for k, v in kw.items() if k in ("is_dna", "allow_ambiguity")}
    osa, olcp, _ = oracle.build(norm, threads=min(16, os.cpu_count() or 1), **okw)
    assert gsa.size == osa.size
    bad = np.nonzero(gsa != osa)[0]
    assert bad.size == 0, f"SA differs at rank {bad[0]} of {osa.size}: got {gsa[bad[0]]} want {osa[bad[0]]} ({bad.size} ranks differ)"
    bad = np.nonzero(glcp != olcp)[0]
    assert bad.size == 0, f"LCP differs at rank {bad[0]} of {osa.size}: got {glcp[bad[0]]} want {olcp[bad[0]]} ({bad.size} ranks differ)"
    if expect_exceptions:
        assert st.num_exceptions > 0 and st.bits_per_char == 3, (st.num_exceptions, st.bits_per_char)
    info = (st.num_exceptions, st.num_reinserted)
    db.close()
    return info


@pytest.mark.parametrize("n", [40, 1000, 70_000, 3_000_000])
@pytest.mark.parametrize("amb", [False, True])
def test_scattered_iupac_codes_equal_oracle(oracle, n, amb):
    rng = np.random.default_rng(n + amb)
    raw = _acgt(rng, n)
    k = max(1, min(60, n // 20))
    raw[rng.integers(0, n - 1, k)] = IUPAC[rng.integers(0, 10, k)]
    raw[-1] = ord("$")
    small = 64 * k > n                           # (more than one such byte in 64: the general table)
    exc, re = _check(oracle, raw, is_dna=True, allow_ambiguity=amb, expect_exceptions=not small)
    if not small:
        assert 0 < exc <= k and re >= (exc if amb else 1)


@pytest.mark.parametrize("soft", [False, True])
def test_softmasked_text_with_iupac_n_runs_and_delimiters(oracle, soft):
    """the shape of a real assembly: lowercase repeats (also lowercase IUPAC letters: upper-cased, or 'N' under
    --ignore-softmask), N runs, '%' between sequences, IUPAC codes next to all of them"""
    x, _ = synth.syn_human(2_000_000, seed=11)
    raw = x.numpy().copy()
    rng = np.random.default_rng(5)
    # (N runs stay below 1000: with two runs of >= 1000 'N' the reference's own --allow-ambiguity order is approximate,
    # sufr_builder.rs:302-307, and so is the oracle's -- DESIGN.md section 2)
    isn = np.nonzero((raw == ord("N")) | (raw >= 97))[0]      # (lowercase becomes 'N' under --ignore-softmask)
    raw[isn[::700]] = ord("A")
    at = rng.integers(100, raw.size - 100, 40)
    raw[at] = IUPAC[rng.integers(0, 10, 40)]
    raw[at[:10] + 1] = IUPAC[rng.integers(0, 10, 10)] | 0x20          # lowercase ones
    n_at = np.nonzero(raw == ord("N"))[0]
    raw[n_at[rng.integers(0, n_at.size, 5)]] = ord("R")               # inside N runs
    pc = np.nonzero(raw == ord("%"))[0]
    raw[pc[0] + 1] = ord("Y"); raw[pc[1] - 1] = ord("K")
    raw[0] = ord("M"); raw[-2] = ord("S")
    _check(oracle, raw, is_dna=True, ignore_softmask=soft)
    _check(oracle, raw, is_dna=True, ignore_softmask=soft, allow_ambiguity=True)


def test_other_delimiter_is_an_exception_byte(oracle):
    """`-D '#'`: every delimiter is a byte outside the table; also bytes below '$' and above 'T'"""
    rng = np.random.default_rng(8)
    raw = _acgt(rng, 500_000)
    raw[np.arange(5_000, raw.size - 1, 5_000)] = ord("#")
    raw[[17, 4_000, 250_000]] = [ord("!"), ord("Z"), ord("*")]
    raw[-1] = ord("$")
    exc, _ = _check(oracle, raw, is_dna=True)
    assert exc == 99 + 2                     # (250 000 is one of the delimiters)
    _check(oracle, raw, is_dna=True, allow_ambiguity=True)


def test_iupac_codes_inside_repeats_reach_far(oracle):
    """copies of a long segment that differ ONLY in an IUPAC letter (R in one, N in another, T in a third, the letter missing
    in the rest): the comparisons of thousands of suffixes before the letter reach it, and the order of the copies is decided
    by the raw byte ('N' < 'R' < 'T') -- the re-placed suffixes are most of the family"""
    rng = np.random.default_rng(21)
    raw = _acgt(rng, 1_500_000)
    seg = _acgt(rng, 6_000)
    for i, c in enumerate(b"RNTRYAGK"):
        s = seg.copy()
        s[4_000] = c
        raw[100_000 + i * 150_000:100_000 + i * 150_000 + 6_000] = s
    raw[-1] = ord("$")
    exc, re = _check(oracle, raw, is_dna=True)
    assert exc == 4 and re > 3 * 3_000
    _check(oracle, raw, is_dna=True, allow_ambiguity=True)


def test_runs_and_clusters_of_exception_bytes(oracle):
    """runs of one IUPAC letter (under -a every position of the run is a suffix; in the build they are a run of 'N': the
    closed-form run buckets), alternating letters, a run that ends the text"""
    rng = np.random.default_rng(33)
    raw = _acgt(rng, 800_000)
    raw[10_000:10_700] = ord("R")
    raw[300_000:300_050] = np.resize(np.frombuffer(b"RY", dtype=np.uint8), 50)
    raw[500_000:500_400] = ord("N"); raw[500_200] = ord("R")          # an N run broken by one letter
    raw[-40:-1] = ord("W")
    raw[-1] = ord("$")
    _check(oracle, raw, is_dna=True)
    exc, re = _check(oracle, raw, is_dna=True, allow_ambiguity=True)
    assert exc == 700 + 50 + 1 + 39 and re >= exc


def test_many_exception_bytes_fall_back_to_the_general_table(oracle):
    """more than one byte in 64 outside the table: not a DNA text with a few ambiguity codes -- the general code table as
    before (and the text handed back is still the caller's)"""
    rng = np.random.default_rng(2)
    raw = np.frombuffer(b"ACGTRYKM", dtype=np.uint8)[rng.integers(0, 8, 200_000)].copy()
    raw[-1] = ord("$")
    exc, _ = _check(oracle, raw, expect_exceptions=False, is_dna=True)
    assert exc == 0


@pytest.mark.parametrize("amb", [False, True])
@pytest.mark.parametrize("shards", [2, 3, 7])
def test_sharded_builds_with_exception_bytes_concatenate(oracle, shards, amb):
    """shards are first-digit ranges of the text as it was BUILT ('N' for the listed bytes); a suffix with a listed byte among
    its first five characters may truly belong to another shard: every rank takes all such suffixes out, keeps the ones whose
    true first bytes lie in its range and adds the other shards' that do -- the shards concatenate to the oracle's arrays,
    every suffix in exactly one of them.  Letters below 'A', between the table's letters and above 'T', clustered at the
    start of many suffixes."""
    rng = np.random.default_rng(4 + shards)
    raw = _acgt(rng, 400_000)
    raw[rng.integers(0, raw.size - 1, 60)] = np.frombuffer(b"RYKMSWBDHV*#Z!", dtype=np.uint8)[rng.integers(0, 14, 60)]
    raw[1000:1004] = np.frombuffer(b"RYRY", dtype=np.uint8)
    raw[-3] = ord("W")
    raw[-1] = ord("$")
    x = torch.from_numpy(raw).cuda()
    db = sufr_amd.DeviceBuilder(0)
    parts_sa, parts_lcp = [], []
    for k in range(shards):
        sa, lcp = db.sort(x, raw_text=True, is_dna=True, allow_ambiguity=amb, shard_index=k, num_shards=shards)
        assert db.stats.num_exceptions > 0 and db.stats.bits_per_char == 3
        assert db.stats.num_suffixes == sa.numel()
        parts_sa.append(sa.cpu().numpy().view(np.uint32).copy()); parts_lcp.append(lcp.cpu().numpy().view(np.uint32).copy())
    db.close()
    osa, olcp, _ = oracle.build(raw, is_dna=True, allow_ambiguity=amb, threads=8)
    gsa = np.concatenate(parts_sa); glcp = np.concatenate(parts_lcp)
    assert gsa.size == osa.size
    bad = np.nonzero(gsa != osa)[0]
    assert bad.size == 0, f"SA differs at rank {bad[0]}: got {gsa[bad[0]]} want {osa[bad[0]]} ({bad.size} ranks; shard sizes {[p.size for p in parts_sa]})"
    starts = np.cumsum([0] + [p.size for p in parts_sa[:-1]])
    keep = np.ones(osa.size, dtype=bool); keep[starts[1:]] = False      # (a shard's first LCP is the stitch's)
    assert np.array_equal(glcp[keep], olcp[keep])


def test_host_buffer_abi_returns_the_original_bytes(oracle):
    """sufr_hip_build_u32 (what the Rust shim binds): norm_text_out carries the IUPAC letters, not the 'N' of the build"""
    rng = np.random.default_rng(9)
    raw = _acgt(rng, 100_000)
    raw[[5, 50_000, 99_990]] = [ord("R"), ord("y"), ord("K")]
    raw[-1] = ord("$")
    ctx = sufr_amd.Context(0)
    args = sufr_amd.SufrBuilderArgs(text=raw, is_dna=True)
    b = sufr_amd.SufrBuilder(args, index_width=4, ctx=ctx, write=False)
    norm = oracle.normalize(raw, False)
    assert np.array_equal(b.text, norm) and norm[50_000] == ord("Y")
    osa, olcp, _ = oracle.build(norm, is_dna=True, threads=8)
    assert np.array_equal(b.suffix_array, osa) and np.array_equal(b.lcp, olcp)
    ctx.close()


def test_max_query_len_and_windows_with_exception_bytes(oracle):
    """-m L on top of the re-placed arrays (same canonical form as without exception bytes), and the windowed build"""
    rng = np.random.default_rng(12)
    raw = _acgt(rng, 300_000)
    raw[50_000:50_300] = raw[150_000:150_300]
    raw[rng.integers(0, raw.size - 1, 25)] = IUPAC[rng.integers(0, 10, 25)]
    raw[-1] = ord("$")
    x = torch.from_numpy(raw).cuda()
    osa, olcp, _ = oracle.build(raw, is_dna=True, threads=8)
    db = sufr_amd.DeviceBuilder(0)
    sa, lcp = db.sort(x, raw_text=True, is_dna=True, max_query_len=11)
    gsa = sa.cpu().numpy().view(np.uint32); glcp = lcp.cpu().numpy().view(np.uint32)
    assert np.array_equal(glcp, np.minimum(olcp, 11))
    assert np.array_equal(np.sort(gsa), np.sort(osa))
    pre = lambda p: bytes(raw[p:p + 11])
    assert [pre(p) for p in gsa[:20_000]] == [pre(p) for p in osa[:20_000]]
    db.ctx.set_window(70_000, 5_000)
    wsa, wlcp = db.sort(x, raw_text=True, is_dna=True, index_width=8)
    assert np.array_equal(wsa.cpu().numpy().astype(np.uint32), osa) and np.array_equal(wlcp.cpu().numpy().astype(np.uint32), olcp)
    db.ctx.set_window(0, 0)
    db.close()


def _long_n_run_text(seed, n=60_000):
    """two runs of >= 1000 'N' in the NORMALISED text (one of them made of 'N' and lowercase stretches that touch: 'N' under
    --ignore-softmask), further short ones, listed bytes inside, at the edges of and between the runs"""
    rng = np.random.default_rng(seed)
    raw = _acgt(rng, n)
    raw[5_000:6_300] = ord("N")
    raw[22_000:22_700] = ord("N"); raw[22_700:23_300] |= 0x20
    for _ in range(12):
        ln = int(rng.integers(1, 600)); at = int(rng.integers(24_000, n - ln))
        raw[at:at + ln] = ord("N") if rng.random() < 0.5 else (raw[at:at + ln] | 0x20)
    raw[[5_600, 6_299, 6_300, 22_000, 22_650, 23_299, 30_000]] = np.frombuffer(b"RYW#KSM", dtype=np.uint8)
    raw[-1] = ord("$")
    return raw


@pytest.mark.parametrize("shards", [1, 3])
@pytest.mark.parametrize("cap", [None, 17])
@pytest.mark.parametrize("planted", [False, True])
def test_long_n_runs_under_allow_ambiguity_are_exact(oracle, shards, cap, planted):
    """two runs of >= 1000 'N' with --allow-ambiguity: the reference's N-run shortcut (sufr_builder.rs:302-307) makes its own
    order approximate there ("known divergence"; found again by profiles/soak_round6.py, seed 7091), so the
    witness is the exact order: the oracle's byte-wise build of the same normalised text over all positions (is_dna=False keeps
    every suffix and has no N-run table; --allow-ambiguity keeps every suffix too).  With and without listed bytes, with and
    without a cap, one shard and three."""
    raw = _long_n_run_text(31 + shards)
    if not planted:
        raw[np.isin(raw, np.frombuffer(b"RYW#KSM", dtype=np.uint8))] = ord("A")
    norm = oracle.normalize(raw, True)
    osa, olcp, _ = oracle.build(norm, is_dna=False, threads=8)
    if cap:
        from test_gpu_mql_fast import canonical
        osa, olcp = canonical(osa, olcp, cap)
    db = sufr_amd.DeviceBuilder(0)
    x = torch.from_numpy(raw).cuda()
    sas, lcps = [], []
    for k in range(shards):
        sa, lcp = db.sort(x, raw_text=True, is_dna=True, allow_ambiguity=True, ignore_softmask=True, max_query_len=cap or 0,
                          shard_index=k, num_shards=shards)
        assert (db.stats.num_exceptions > 0) == planted
        sas.append(sa.cpu().numpy().view(np.uint32).copy()); lcps.append(lcp.cpu().numpy().view(np.uint32).copy())
    db.close()
    gsa = np.concatenate(sas); glcp = np.concatenate(lcps)
    assert gsa.size == osa.size
    bad = np.nonzero(gsa != osa)[0]
    assert bad.size == 0, f"SA differs at rank {bad[0]}: got {gsa[bad[0]]} want {osa[bad[0]]} ({bad.size} ranks)"
    starts = np.cumsum([0] + [p.size for p in sas[:-1]])
    keep = np.ones(osa.size, dtype=bool); keep[starts[1:]] = False
    bad = np.nonzero((glcp != olcp) & keep)[0]
    assert bad.size == 0, f"LCP differs at rank {bad[0]}: got {glcp[bad[0]]} want {olcp[bad[0]]} ({bad.size} ranks)"


# ---- the ways out of a build before the listed bytes are re-placed: the text handed out is the caller's all the same --------------
def _context_text(ctx, n):
    """the normalised text the context keeps on the device after a build through sufr_hip_sort_device_u64 (what the shard stitch
    and the device search read), copied to the host with the HIP runtime the process has loaded"""
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
    out = np.zeros(n, dtype=np.uint8)
    assert hip.hipMemcpy(out.ctypes.data, t, n, 2) == 0          # hipMemcpyDeviceToHost
    return out


def _listed(norm):
    return int((~np.isin(norm, np.frombuffer(b"$%ACGNT", dtype=np.uint8))).sum())


@pytest.mark.parametrize("soft", [False, True])
def test_an_empty_build_keeps_its_bytes(oracle, soft):
    """500 'N' with an 'R' and a 'y': --dna without --allow-ambiguity, no sentinel -- no position starts a suffix, the build
    returns right after the text pass, which has written 'N' over the listed bytes.  The text handed out is the reference's
    normalised text all the same (upper-cased: 'R' and 'Y', two listed bytes; under --ignore-softmask the reference turns the
    lowercase 'y' into 'N' itself, sufr_builder.rs:144-160, and one listed byte is left), and the stats count the listed bytes."""
    raw = np.full(500, ord("N"), np.uint8)
    raw[100] = ord("R"); raw[300] = ord("y")
    norm = oracle.normalize(raw, soft)
    assert _listed(norm) == (1 if soft else 2) and norm[100] == ord("R") and norm[300] == (ord("N") if soft else ord("Y"))
    ctx = sufr_amd.Context(0)
    b = sufr_amd.SufrBuilder(sufr_amd.SufrBuilderArgs(text=raw, is_dna=True, ignore_softmask=soft), index_width=4, ctx=ctx, write=False)
    assert b.num_suffixes == 0
    assert np.array_equal(b.text, norm), f"host buffers: text differs at {np.nonzero(b.text != norm)[0]}"
    assert b.stats.num_exceptions == _listed(norm)
    ctx.close()
    db = sufr_amd.DeviceBuilder(0)
    sa, lcp = db.sort(torch.from_numpy(raw).cuda(), raw_text=True, is_dna=True, ignore_softmask=soft, index_width=8)
    assert sa.numel() == 0 and lcp.numel() == 0 and db.stats.num_suffixes == 0
    got = _context_text(db.ctx, raw.size)
    assert np.array_equal(got, norm), f"device entry point: text differs at {np.nonzero(got != norm)[0]}"
    assert db.stats.num_exceptions == _listed(norm)
    db.close()


def test_a_build_that_does_not_fit_then_fits(oracle):
    """outputs of 10 entries: the capacity error and the number of suffixes the call needs -- and the context's text is the
    caller's, not the build's; the same context then builds the text into full-size outputs"""
    rng = np.random.default_rng(41)
    raw = _acgt(rng, 300_000)
    raw[40_000:40_400] = raw[200_000:200_400]
    raw[rng.choice(raw.size - 1, 20, replace=False)] = IUPAC[rng.integers(0, 10, 20)]
    raw[-1] = ord("$")
    norm = oracle.normalize(raw, False)
    assert _listed(norm) == 20
    osa, olcp, _ = oracle.build(norm, is_dna=True, threads=8)
    x = torch.from_numpy(raw).cuda()
    db = sufr_amd.DeviceBuilder(0)
    small_sa = torch.zeros(10, dtype=torch.int64, device="cuda"); small_lcp = torch.zeros(10, dtype=torch.int64, device="cuda")
    ns = C.c_uint64(0)
    rc = sufr_amd.lib().sufr_hip_sort_device_u64(db.ctx.handle, x.data_ptr(), x.numel(), 1 | 8, 0, None, 16, 42, 0, 1, small_sa.data_ptr(),
                                                small_lcp.data_ptr(), 10, C.byref(ns), C.byref(db.stats))
    assert rc == -5 and ns.value == osa.size, (rc, ns.value, osa.size)          # SUFR_HIP_E_CAPACITY
    got = _context_text(db.ctx, raw.size)
    assert np.array_equal(got, norm), f"after the capacity error: text differs at {np.nonzero(got != norm)[0][:8]}"
    out_sa = torch.zeros(raw.size, dtype=torch.int64, device="cuda"); out_lcp = torch.zeros(raw.size, dtype=torch.int64, device="cuda")
    sa, lcp = db.sort(x, raw_text=True, is_dna=True, index_width=8, out_sa=out_sa, out_lcp=out_lcp)
    assert db.stats.num_exceptions == 20
    assert np.array_equal(sa.cpu().numpy().astype(np.uint32), osa) and np.array_equal(lcp.cpu().numpy().astype(np.uint32), olcp)
    assert np.array_equal(_context_text(db.ctx, raw.size), norm)
    db.close()


def _empty_shard_text(case):
    if case == "a_runs":                         # 3 000 'A': the bucket AAAAA holds all but a few suffixes, the digits after it few
        raw = np.full(3001, ord("A"), np.uint8); at = [400, 1000, 1001, 1900, 2995]
    elif case == "t_runs":
        # 3 000 'T': TTTTT is the LAST digit of the built text, the ranks behind the first own the range above every digit of
        # the built text -- where the true first digits of the suffixes with a 'Y' (above 'T') among their first five bytes lie
        raw = np.full(3001, ord("T"), np.uint8); at = [0, 700, 1500, 1502, 2996]
    else:                                        # fewer suffixes than shards: ranks that own digits no suffix starts with
        raw = np.full(401, ord("N"), np.uint8); at = [150]; raw[149] = ord("A"); raw[300] = ord("C")
    raw[at] = ord("Y")
    raw[-1] = ord("$")
    return raw


@pytest.mark.parametrize("case", ["a_runs", "t_runs", "few_suffixes"])
def test_empty_shards_lose_and_repeat_no_suffix(oracle, case):
    """more shards than the built text has first digits to deal out: ranks whose own range is empty (top_hi <= top_lo) or holds
    no suffix.  Every rank still puts the listed bytes back and takes the suffixes whose TRUE first bytes lie in its range --
    those and no others: the shards concatenate to the oracle's arrays."""
    raw = _empty_shard_text(case)
    amb = case != "few_suffixes"
    shards = 7
    if amb:
        osa, olcp, _ = oracle.build(raw, is_dna=True, allow_ambiguity=True, threads=8)
    else:                                        # (three suffixes: the reference cannot draw its pivots; the naive witness)
        from oracle_helper import naive_sa_lcp
        osa, olcp = naive_sa_lcp(raw, True, False)
        osa = np.asarray(osa, dtype=np.uint32); olcp = np.asarray(olcp, dtype=np.uint32)
        assert osa.size == 3
    x = torch.from_numpy(raw).cuda()
    db = sufr_amd.DeviceBuilder(0)
    parts_sa, parts_lcp, ranges = [], [], []
    for k in range(shards):
        out_sa = torch.zeros(raw.size, dtype=torch.int32, device="cuda"); out_lcp = torch.zeros(raw.size, dtype=torch.int32, device="cuda")
        sa, lcp = db.sort(x, raw_text=True, is_dna=True, allow_ambiguity=amb, shard_index=k, num_shards=shards, out_sa=out_sa, out_lcp=out_lcp)
        assert db.stats.bits_per_char == 3 and db.stats.num_exceptions == _listed(raw), (k, db.stats.num_exceptions)
        assert db.stats.num_suffixes == sa.numel()
        ranges.append((db.stats.top_lo, db.stats.top_hi))
        parts_sa.append(sa.cpu().numpy().view(np.uint32).copy()); parts_lcp.append(lcp.cpu().numpy().view(np.uint32).copy())
    db.close()
    sizes = [p.size for p in parts_sa]
    print(f"{case}: first-digit ranges {ranges}, shard sizes {sizes}")
    assert any(hi <= lo for lo, hi in ranges), f"no rank's own range is empty: {ranges}"
    gsa = np.concatenate(parts_sa); glcp = np.concatenate(parts_lcp)
    assert np.unique(gsa).size == gsa.size, f"a suffix appears twice (shard sizes {sizes})"
    assert gsa.size == osa.size, f"{osa.size - gsa.size} suffixes lost (shard sizes {sizes})"
    bad = np.nonzero(gsa != osa)[0]
    assert bad.size == 0, f"SA differs at rank {bad[0]}: got {gsa[bad[0]]} want {osa[bad[0]]} ({bad.size} ranks; shard sizes {sizes})"
    keep = np.ones(osa.size, dtype=bool); keep[np.cumsum(sizes[:-1])[np.cumsum(sizes[:-1]) < osa.size]] = False      # (a shard's first LCP is the stitch's)
    assert np.array_equal(glcp[keep], olcp[keep])
