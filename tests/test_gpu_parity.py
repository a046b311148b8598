"""Parity tests proper (-m gpu): the HIP path, called through the C ABI, against
  * the reference's golden .sufr files (whole-file byte equality),
  * the CPU oracle on the same seeded inputs (bit-exact SA and LCP),
  * size-independent properties at larger sizes (permutation of the eligible positions, sortedness,
    exact LCP on sampled adjacent ranks)."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

import sufr_amd
from sufr_amd import synth
from oracle_helper import GOLDEN, GOLDEN_CASES, check_sa_lcp_properties, naive_sa_lcp, parse_sufr

pytestmark = pytest.mark.gpu

import os


@pytest.fixture(scope="module")
def ctx():
    c = sufr_amd.Context(0)
    yield c
    c.close()


def gpu_build(ctx, raw: np.ndarray, *, is_dna=True, allow_ambiguity=False, ignore_softmask=False, width=4,
              max_query_len=None, seed_mask=None):
    """sufr_hip_build_u32/u64 on a raw (un-normalised) host text."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    args = sufr_amd.SufrBuilderArgs(text=raw, is_dna=is_dna, allow_ambiguity=allow_ambiguity,
                                    ignore_softmask=ignore_softmask, max_query_len=max_query_len,
                                    seed_mask=seed_mask)
    b = sufr_amd.SufrBuilder(args, index_width=width, ctx=ctx, write=False)
    return b


def assert_matches_oracle(ctx, oracle, raw, *, is_dna=True, allow_ambiguity=False, ignore_softmask=False,
                          threads=8):
    b = gpu_build(ctx, raw, is_dna=is_dna, allow_ambiguity=allow_ambiguity, ignore_softmask=ignore_softmask)
    norm = oracle.normalize(np.ascontiguousarray(raw, dtype=np.uint8), ignore_softmask)
    assert np.array_equal(b.text, norm), "normalised text differs"
    if norm.size >= 4:
        sa, lcp, st = oracle.build(norm, is_dna=is_dna, allow_ambiguity=allow_ambiguity, threads=threads)
    else:  # the reference cannot build texts shorter than 4 (text_len/4 == 0 partitions): naive witness
        sa, lcp = naive_sa_lcp(norm, is_dna, allow_ambiguity)
    assert b.num_suffixes == sa.size
    bad = np.nonzero(b.suffix_array != sa)[0]
    assert bad.size == 0, f"SA differs at rank {bad[0]} of {sa.size}: got {b.suffix_array[bad[0]]} want {sa[bad[0]]}"
    bad = np.nonzero(b.lcp != lcp)[0]
    assert bad.size == 0, f"LCP differs at rank {bad[0]} of {sa.size}: got {b.lcp[bad[0]]} want {lcp[bad[0]]}"
    return b


# ---- the reference's golden files -----------------------------------------------------------------
GPU_GOLDEN = sorted(GOLDEN_CASES)


@pytest.mark.parametrize("name", GPU_GOLDEN)
def test_golden_file_bytes(tmp_path, name):
    case = dict(GOLDEN_CASES[name])
    fa = GOLDEN / "inputs" / case.pop("fa")
    out = tmp_path / name
    delim = case.pop("delimiter", b"%").decode()
    path, st = sufr_amd.create(str(fa), str(out), sequence_delimiter=delim, **case)
    assert path == str(out)
    assert out.read_bytes() == (GOLDEN / "expected" / name).read_bytes()


def test_native_cli_binary_golden(tmp_path):
    """`sufr create --dna -n 2 data/inputs/2.fa` (BASELINE config C1) through the native binary."""
    out = tmp_path / "2.sufr"
    r = subprocess.run([str(sufr_amd.CLI_PATH), "--log", "info", "create", "--dna", "-n", "2", "-o", str(out),
                        str(GOLDEN / "inputs" / "2.fa")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "Wrote 260 bytes" in r.stdout
    assert out.read_bytes() == (GOLDEN / "expected" / "2.sufr").read_bytes()
    # gzip input (needletail inflates it transparently in the reference)
    import gzip
    gz = tmp_path / "two.fa.gz"
    gz.write_bytes(gzip.compress((GOLDEN / "inputs" / "2.fa").read_bytes()))
    out_gz = tmp_path / "2gz.sufr"
    r = subprocess.run([str(sufr_amd.CLI_PATH), "create", "--dna", "-n", "2", "-o", str(out_gz), str(gz)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert out_gz.read_bytes() == (GOLDEN / "expected" / "2.sufr").read_bytes()
    # default output name: <input stem>.sufr in the CWD (sufr/src/lib.rs:334-340)
    r = subprocess.run([str(sufr_amd.CLI_PATH), "cr", "-d", str(GOLDEN / "inputs" / "1.fa")], cwd=tmp_path,
                       capture_output=True, text=True)
    assert r.returncode == 0 and (tmp_path / "1.sufr").read_bytes() == (GOLDEN / "expected" / "1.sufr").read_bytes()


@pytest.mark.parametrize("name", ["2.sufr", "long_dna_sequence.sufr", "uniprot.sufr", "uniprot-masked.sufr"])
def test_multi_device_create_is_byte_identical(tmp_path, name):
    """`sufr --devices 0,0,0 create` (three shards, here on one GPU): every shard writes its own range of the one
    file, the boundary LCPs are stitched on the device -- the bytes are those of the golden / single-GPU file.
    (--seed-mask builds shard on their own first key digit and stitch with the care-symbol LCP: uniprot-masked.sufr too
    comes out of three contexts.)"""
    case = dict(GOLDEN_CASES[name])
    fa = GOLDEN / "inputs" / case.pop("fa")
    delim = case.pop("delimiter", b"%").decode()
    want = (GOLDEN / "expected" / name).read_bytes()
    out = tmp_path / name
    path, sts = sufr_amd.create(str(fa), str(out), sequence_delimiter=delim, devices=[0, 0, 0], **case)
    assert path == str(out) and len(sts) == 3
    assert out.read_bytes() == want
    out2 = tmp_path / ("cli_" + name)
    cmd = [str(sufr_amd.CLI_PATH), "--devices", "0,0", "create", "-o", str(out2), str(fa), "-D", delim]
    for flag, opt in (("is_dna", "--dna"), ("allow_ambiguity", "-a"), ("ignore_softmask", "-i")):
        if case.get(flag):
            cmd.append(opt)
    if case.get("seed_mask"):
        cmd += ["-s", case["seed_mask"]]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert out2.read_bytes() == want


def test_multi_device_create_5mb_genome(tmp_path, oracle):
    """2, 5 and 8 shards of a 5 Mb soft-masked genome with N runs: the file equals the single-context file."""
    x, starts = synth.syn_human(5_000_000, seed=11)
    fa = tmp_path / "g.fa"
    body = x.numpy()[:-1]
    cuts = list(starts) + [body.size + 1]
    with open(fa, "wb") as f:
        for i in range(len(starts)):
            f.write(f">s{i}\n".encode() + body[cuts[i]:cuts[i + 1] - 1].tobytes() + b"\n")
    one = tmp_path / "one.sufr"
    sufr_amd.create(str(fa), str(one), is_dna=True, ignore_softmask=True)
    for k in (2, 5, 8):
        out = tmp_path / f"k{k}.sufr"
        sufr_amd.create(str(fa), str(out), is_dna=True, ignore_softmask=True, devices=[0] * k)
        assert out.read_bytes() == one.read_bytes(), k
    ref = tmp_path / "ref.sufr"
    oracle.create(str(fa), str(ref), is_dna=True, ignore_softmask=True)
    assert one.read_bytes() == ref.read_bytes()


def test_multi_device_create_with_a_run_bucket_and_stalling_repeats(tmp_path, oracle):
    """`sufr create --allow-ambiguity` over 1, 2 and 3 contexts on a text whose N bucket goes through the closed form and whose
    templated repeats hand a level to prefix doubling (in every shard since round 4): the files are byte-identical, and equal to
    the oracle's"""
    raw = _templated_runs_text(12, 5000, 6, 700, ntemplates=4, tlen=280)
    fa = tmp_path / "r.fa"
    with open(fa, "wb") as f:
        f.write(b">one\n" + raw[:-1].tobytes() + b"\n")
    one = tmp_path / "one.sufr"
    sufr_amd.create(str(fa), str(one), is_dna=True, allow_ambiguity=True)
    for k in (2, 3):
        out = tmp_path / f"k{k}.sufr"
        sufr_amd.create(str(fa), str(out), is_dna=True, allow_ambiguity=True, devices=[0] * k)
        assert out.read_bytes() == one.read_bytes(), k
    ref = tmp_path / "ref.sufr"
    oracle.create(str(fa), str(ref), is_dna=True, allow_ambiguity=True)
    assert one.read_bytes() == ref.read_bytes()


def test_create_reports_an_unwritable_output(tmp_path):
    """"{filename}: {io error}" like SufrBuilder::write (sufr_builder.rs:820), exit code 1 from the binary"""
    bad = tmp_path / "no_such_dir" / "x.sufr"
    with pytest.raises(sufr_amd.SufrHipError) as e:
        sufr_amd.create(str(GOLDEN / "inputs" / "1.fa"), str(bad), is_dna=True)
    assert str(bad) in str(e.value) and "No such file or directory" in str(e.value)
    r = subprocess.run([str(sufr_amd.CLI_PATH), "create", "-d", "-o", str(bad), str(GOLDEN / "inputs" / "1.fa")],
                       capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("Error: ") and str(bad) in r.stderr


def test_lib_rs_inline_vectors(ctx):  # libsufr/src/lib.rs:45-140
    d = sufr_amd.read_sequence_file(GOLDEN / "inputs" / "2.fa", b"N")
    b = gpu_build(ctx, np.frombuffer(d.seq, dtype=np.uint8))
    assert b.text.tobytes() == b"ACGTACGTNACGTACGT$"
    assert b.suffix_array.tolist() == [17, 13, 9, 0, 4, 14, 10, 1, 5, 15, 11, 2, 6, 16, 12, 3, 7]
    assert b.lcp.tolist() == [0, 0, 4, 8, 4, 0, 3, 7, 3, 0, 2, 6, 2, 0, 1, 5, 1]
    d = sufr_amd.read_sequence_file(GOLDEN / "inputs" / "1.fa", b"N")
    b = gpu_build(ctx, np.frombuffer(d.seq, dtype=np.uint8), allow_ambiguity=True, width=8)   # SufrBuilder<u64>
    assert b.suffix_array.dtype == np.uint64
    assert b.suffix_array.tolist() == [10, 6, 0, 7, 1, 8, 2, 5, 4, 9, 3]
    assert b.lcp.tolist() == [0, 0, 4, 0, 3, 0, 2, 0, 1, 0, 1]
    d = sufr_amd.read_sequence_file(GOLDEN / "inputs" / "smol.fa", b"N")
    b = gpu_build(ctx, np.frombuffer(d.seq, dtype=np.uint8))
    assert b.num_suffixes == 364


def test_option_errors_fail_loudly(ctx, tmp_path):
    with pytest.raises(sufr_amd.SufrHipError) as e:
        sufr_amd.create(str(GOLDEN / "inputs" / "uniprot.fa"), str(tmp_path / "m.sufr"), seed_mask="0110")
    assert e.value.code == -9 and "Invalid seed mask '0110'" in str(e.value)
    with pytest.raises(sufr_amd.SufrHipError) as e:        # sufr_builder.rs:163-165
        sufr_amd.create(str(GOLDEN / "inputs" / "1.fa"), str(tmp_path / "m.sufr"), max_query_len=3,
                        seed_mask="101", is_dna=True)
    assert "Cannot use max_query_len and seed_mask together" in str(e.value)
    # tie order of these builds crosses prefix buckets: the sharded device entry point refuses them
    t = torch.from_numpy(np.frombuffer(b"ACGTACGT$", dtype=np.uint8).copy()).cuda()
    db = sufr_amd.DeviceBuilder(0)
    with pytest.raises(sufr_amd.SufrHipError) as e:
        db.sort(t, is_dna=True, shard_index=0, num_shards=2, max_query_len=3)
    assert e.value.code == -6
    db.close()


# ---- --seed-mask and --max-query-len builds -------------------------------------------------------
def _lowent_dna(rng, n, sigma):
    body = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, sigma, size=n)]
    return np.concatenate([body, np.frombuffer(b"$", dtype=np.uint8)])


@pytest.mark.parametrize("mask", ["101", "1101", "10111011", "110000000011", "1" * 24 + "01",
                                  "1" + "01" * 30])
@pytest.mark.parametrize("n,sigma", [(5, 2), (700, 2), (5000, 4), (120_000, 3)])
def test_seed_mask_matches_oracle(ctx, oracle, mask, n, sigma):
    """Seed-mask builds are deterministic in the reference (ties resolved by position, 701-712)."""
    raw = _lowent_dna(np.random.default_rng(n + len(mask)), n, sigma)
    b = gpu_build(ctx, raw, seed_mask=mask)
    sa, lcp, st = oracle.build(raw, is_dna=True, seed_mask=mask, threads=8)
    assert np.array_equal(b.suffix_array, sa)
    assert np.array_equal(b.lcp, lcp)


def test_seed_mask_protein_and_inline_vectors(ctx, oracle):
    d = sufr_amd.read_sequence_file(GOLDEN / "inputs" / "uniprot.fa", b"%")
    raw = np.frombuffer(d.seq, dtype=np.uint8)
    for mask in ["10111011", "1001", "11011"]:
        b = gpu_build(ctx, raw, is_dna=False, seed_mask=mask)
        sa, lcp, st = oracle.build(oracle.normalize(raw, False), seed_mask=mask, threads=8)
        assert np.array_equal(b.suffix_array, sa) and np.array_equal(b.lcp, lcp)


def _first_chars(norm: np.ndarray, sa: np.ndarray, L: int) -> np.ndarray:
    """(len(sa), L) matrix of the first L characters of every listed suffix, 0 past the end."""
    pad = np.concatenate([norm, np.zeros(L, dtype=np.uint8)])
    return pad[sa.astype(np.int64)[:, None] + np.arange(L)[None, :]]


@pytest.mark.parametrize("L", [1, 2, 5, 12, 20, 21, 22, 40, 300])
@pytest.mark.parametrize("n,sigma", [(6, 1), (900, 2), (40_000, 4), (150_000, 2)])
def test_max_query_len_canonical_form(ctx, oracle, n, sigma, L):
    """The reference's -m builds depend on pivots and merge order (find_lcp overrides `len`, 310-314;
    tests/test_oracle_golden.py shows it): what every such build shares is the order of the first L
    characters and min(LCP, L).  The GPU emits the canonical member of that family: ties in descending
    position, LCP capped at L."""
    raw = _lowent_dna(np.random.default_rng(n * 31 + L), n, sigma)
    b = gpu_build(ctx, raw, max_query_len=L)
    full = gpu_build(ctx, raw)
    sa = b.suffix_array.astype(np.int64)
    assert np.array_equal(np.sort(sa), np.sort(full.suffix_array.astype(np.int64)))
    assert np.array_equal(b.lcp, np.minimum(full.lcp, L))
    tie = b.lcp >= L
    assert np.all(sa[1:][tie[1:]] < sa[:-1][tie[1:]]), "ties must come in descending position"
    assert np.array_equal(_first_chars(b.text, sa, min(L, 64)),
                          _first_chars(b.text, full.suffix_array, min(L, 64)))
    # the oracle (one member of the reference's family) agrees on both invariants
    osa, olcp, st = oracle.build(b.text, is_dna=True, max_query_len=L, threads=8)
    assert np.array_equal(np.minimum(olcp, L), b.lcp)
    assert np.array_equal(_first_chars(b.text, osa, min(L, 64)), _first_chars(b.text, sa, min(L, 64)))


def test_max_query_len_file_header(tmp_path):
    out = tmp_path / "m.sufr"
    sufr_amd.create(str(GOLDEN / "inputs" / "1.fa"), str(out), max_query_len=3, is_dna=True)
    g = parse_sufr(out)
    assert g.max_query_len == 3 and int(g.lcp.max()) <= 3


# ---- seeded inputs against the oracle -----------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 17, 63, 64, 65, 127, 128, 129, 255, 4095, 4096, 4097, 8191, 8193,
                               65_536, 300_000])
def test_random_dna_sizes(ctx, oracle, n):
    rng = np.random.default_rng(n)
    body = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n - 1)] if n > 1 else np.empty(0, np.uint8)
    raw = np.concatenate([body, np.frombuffer(b"$", dtype=np.uint8)])
    assert_matches_oracle(ctx, oracle, raw)


def test_sparse_partition_kernel_both_flush_modes(ctx, oracle):
    """The partition kernel takes 8192-position tiles: dense stretches overflow its record-sized staging area and
    are flushed as two half tiles; N-rich stretches fit in one."""
    rng = np.random.default_rng(77)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    parts = [acgt[rng.integers(0, 4, size=70_000)]]                         # dense: two flushes per tile
    mixed = acgt[rng.integers(0, 4, size=150_000)]
    for st in range(0, mixed.size, 900):                                     # ~45 % kept: one flush per tile
        mixed[st:st + int(rng.integers(300, 700))] = ord("N")
    parts += [mixed, np.full(60_000, ord("N"), dtype=np.uint8), acgt[rng.integers(0, 4, size=9_000)]]
    raw = np.concatenate(parts + [np.frombuffer(b"$", dtype=np.uint8)])
    b = assert_matches_oracle(ctx, oracle, raw)
    assert b.num_suffixes <= 0.55 * raw.size
    assert b.stats.partition_variant == 3          # k_msd_part_text (bit-packed stream)


def test_empty_text(ctx):
    b = gpu_build(ctx, np.empty(0, dtype=np.uint8))
    assert b.num_suffixes == 0


def _break_long_n_runs(raw: np.ndarray, soft: bool = False) -> np.ndarray:
    """Keep every N run of the NORMALISED text shorter than 1000: the reference's N-run shortcut
    (sufr_builder.rs:302-307, only active with allow_ambiguity) makes its own output approximate and
    merge-order dependent (hence thread-schedule dependent) once runs of >= 1000 N exist, so bit-exact
    comparison with it is only meaningful below that length.  With ignore_softmask, lowercase counts as N."""
    raw = raw.copy()
    isn = (raw == ord("N")) | (raw == ord("n"))
    if soft:
        isn |= (raw >= 97) & (raw <= 122)
    pos = np.nonzero(isn)[0]
    if pos.size:
        new_run = np.concatenate([[True], np.diff(pos) != 1])
        run_start = np.maximum.accumulate(np.where(new_run, np.arange(pos.size), 0))
        within = np.arange(pos.size) - run_start
        raw[pos[within % 500 == 499]] = ord("C")
    return raw


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("amb", [False, True])
def test_softmask_ambiguity_delimiters(ctx, oracle, soft, amb):
    x, starts = synth.syn_human(400_000, seed=11)
    raw = x.numpy()
    if amb:
        raw = _break_long_n_runs(raw, soft)
    assert_matches_oracle(ctx, oracle, raw, ignore_softmask=soft, allow_ambiguity=amb)


def test_allow_ambiguity_long_n_runs_are_exact(ctx):
    """With several N runs >= 1000 the reference is approximate (see above); the GPU path returns the exact
    order and exact LCP, checked against the naive witness."""
    rng = np.random.default_rng(4)
    body = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=9000)].copy()
    body[500:1700] = ord("N"); body[3000:4200] = ord("N"); body[6000:7500] = ord("N")
    raw = np.concatenate([body, np.frombuffer(b"$", dtype=np.uint8)])
    b = gpu_build(ctx, raw, allow_ambiguity=True)
    sa, lcp = naive_sa_lcp(raw, True, True)
    assert np.array_equal(b.suffix_array, sa) and np.array_equal(b.lcp, lcp)


def test_only_ineligible(ctx, oracle):
    raw = np.frombuffer(b"NNNNNNNNNNNNNNNNNNNNNNNN%NNNNNNNN", dtype=np.uint8)
    b = gpu_build(ctx, raw)
    assert b.num_suffixes == 0


def _rle_lcp_and_order(t: np.ndarray, starts: np.ndarray, a: int, b: int):
    """exact LCP of suffixes a, b and whether a < b, walking runs instead of bytes (t has few long runs)"""
    n = t.size
    k = 0
    while True:
        pa, pb = a + k, b + k
        if pa >= n or pb >= n:
            return k, pa >= n and pb < n
        if t[pa] != t[pb]:
            return k, t[pa] < t[pb]
        ea = starts[np.searchsorted(starts, pa, side="right")]      # end (exclusive) of pa's run
        eb = starts[np.searchsorted(starts, pb, side="right")]
        k += int(min(ea - pa, eb - pb))


def test_allow_ambiguity_runs_beyond_2_pow_16_bytes(ctx):
    """Runs of 2^16 bytes and more make run tokens longer than the 34 bits a re-keying level sorts by default;
    the level then sorts as many digits as its longest token needs.  Checked against an exact run-walking
    comparison on sampled adjacent ranks."""
    rng = np.random.default_rng(31)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    parts = [acgt[rng.integers(0, 4, 40)], np.full(300_000, ord("N"), np.uint8), acgt[rng.integers(0, 4, 25)],
             np.full(299_990, ord("N"), np.uint8), acgt[rng.integers(0, 4, 33)], np.full(70_000, ord("N"), np.uint8),
             acgt[rng.integers(0, 4, 12)], np.full(300_000, ord("N"), np.uint8), np.frombuffer(b"$", dtype=np.uint8)]
    raw = np.concatenate(parts)
    b = gpu_build(ctx, raw, allow_ambiguity=True)
    assert b.num_suffixes == raw.size
    sa = b.suffix_array.astype(np.int64); lcp = b.lcp.astype(np.int64)
    assert np.array_equal(np.sort(sa), np.arange(raw.size))
    change = np.flatnonzero(raw[1:] != raw[:-1]) + 1
    starts = np.concatenate([[0], change, [raw.size]])            # run starts, then n as the final end
    for r in rng.integers(1, sa.size, 40_000).tolist():
        k, less = _rle_lcp_and_order(raw, starts, int(sa[r - 1]), int(sa[r]))
        assert less and lcp[r] == k, (r, int(sa[r - 1]), int(sa[r]), k, int(lcp[r]))
    assert int(lcp.max()) >= 299_990


def _runs_text(seed, n, symbol, nruns, lo, hi, extra=()):
    """random ACGT with `nruns` runs of `symbol` (lengths uniform in [lo, hi)) and the runs of `extra` lengths, '$'-terminated"""
    rng = np.random.default_rng(seed)
    body = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].copy()
    lens = np.concatenate([rng.integers(lo, hi, nruns), np.asarray(extra, dtype=np.int64)]).astype(np.int64)
    rng.shuffle(lens)
    gap = (n - int(lens.sum())) // (lens.size + 1)
    assert gap >= 2
    at = 0
    for ln in lens.tolist():
        at += int(rng.integers(1, 2 * gap - 1))
        body[at:at + ln] = symbol
        at += ln
    return np.concatenate([body[:max(at + 5, n // 2)], np.frombuffer(b"$", dtype=np.uint8)])


def _templated_runs_text(seed, nruns, lo, hi, ntemplates=40, tlen=260):
    """runs of N whose TAILS come from a few templates (long tail LCPs: the order of two runs is decided hundreds of symbols behind
    them; many runs share a tail up to a late mutation), some runs back to back with one symbol between them, one at the very
    start of the text and one right before the final '$'"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    templates = [acgt[rng.integers(0, 4, tlen)] for _ in range(ntemplates)]
    parts = [np.full(int(rng.integers(lo, hi)), ord("N"), np.uint8)]          # a run at position 0
    for k in range(nruns):
        t = templates[int(rng.integers(0, ntemplates))].copy()
        if rng.random() < 0.7:                                               # a late mutation, or none at all
            t[int(rng.integers(tlen // 2, tlen))] = acgt[int(rng.integers(0, 4))]
        cut = tlen if rng.random() < 0.8 else int(rng.integers(1, tlen))     # some tails are cut short by the next run
        parts.append(t[:cut])
        if rng.random() < 0.05:
            parts.append(acgt[rng.integers(0, 4, int(rng.integers(300, 3000)))])
        parts.append(np.full(int(rng.integers(lo, hi)), ord("N"), np.uint8))
        if rng.random() < 0.03:                                              # two runs with ONE symbol between them
            parts.append(acgt[rng.integers(0, 4, 1)]); parts.append(np.full(int(rng.integers(lo, hi)), ord("N"), np.uint8))
    parts.append(np.frombuffer(b"$", dtype=np.uint8))                        # the last run ends at the end of the text
    return np.concatenate(parts)


@pytest.mark.parametrize("case", ["n_runs_amb", "g_runs_plain", "n_runs_amb_soft", "two_symbols", "n_runs_amb_3_shards", "templated_tails",
                                  "long_templated_tails"])
def test_buckets_of_one_repeated_symbol_equal_oracle(oracle, case):
    """A bucket c^21 of a million records and more is ordered in closed form (sufr_runs.inc): only the last member of every run
    goes through the levels, the others are placed by counting -- class 0 / class 1 blocks, the table of levels and the
    rectangles of the ~2 000 longest runs, the LCP inside a tile, across tiles, across blocks and across the two classes.
    Runs stay below 1 000 symbols so that the reference algorithm (byte walks) is the checker: whole arrays equal."""
    kw = dict(is_dna=True)
    if case in ("n_runs_amb", "n_runs_amb_3_shards"):
        raw = _runs_text(51, 6_000_000, ord("N"), 7000, 21, 900); kw["allow_ambiguity"] = True
    elif case == "templated_tails":
        raw = _templated_runs_text(55, 5200, 6, 760); kw["allow_ambiguity"] = True
    elif case == "long_templated_tails":
        # three templates of 3 000 symbols: neighbouring tails agree for 1 500 - 3 000 symbols, beyond the cap of k_rg_fix's walk
        # (the LCP of a tile's first entry then comes from the minimum of the tail LCPs between the two runs)
        raw = _templated_runs_text(56, 5200, 6, 760, ntemplates=3, tlen=3000); kw["allow_ambiguity"] = True
    elif case == "g_runs_plain":
        raw = _runs_text(52, 5_000_000, ord("G"), 5000, 18, 700)
    elif case == "n_runs_amb_soft":
        raw = _runs_text(53, 5_000_000, ord("a"), 6000, 25, 800); kw["allow_ambiguity"] = True; kw["ignore_softmask"] = True
    else:
        raw = _runs_text(54, 7_000_000, ord("T"), 5000, 21, 600)
        rng = np.random.default_rng(540)
        for _ in range(4500):                                     # a second symbol's runs in the gaps where they fit
            ln = int(rng.integers(21, 650)); at = int(rng.integers(0, raw.size - 700))
            if not (raw[at - 1:at + ln + 1] == ord("T")).any():
                raw[at:at + ln] = ord("C")
    soft = kw.pop("ignore_softmask", False)
    norm = oracle.normalize(raw, soft)
    osa, olcp, _ = oracle.build(norm, threads=min(32, os.cpu_count() or 1), **kw)
    db = sufr_amd.DeviceBuilder(0)
    x = torch.from_numpy(raw).cuda()
    if case.endswith("3_shards"):
        gsa, glcp, _ = _sharded_arrays(db, x, x.numel(), 3, raw_text=True, ignore_softmask=soft, **kw)
    else:
        sa, lcp = db.sort(x, raw_text=True, ignore_softmask=soft, **kw)
        gsa = sa.cpu().numpy().view(np.uint32); glcp = lcp.cpu().numpy().view(np.uint32)
    db.close()
    bad = np.nonzero(gsa != osa)[0]
    assert bad.size == 0, f"SA differs at rank {bad[0]} of {osa.size}: got {gsa[bad[0]]} want {osa[bad[0]]}"
    bad = np.nonzero(glcp != olcp)[0]
    assert bad.size == 0, f"LCP differs at rank {bad[0]} of {osa.size}: got {glcp[bad[0]]} want {olcp[bad[0]]} (SA {gsa[bad[0] - 1]}, {gsa[bad[0]]})"


def test_run_bucket_of_a_protein_text_equals_oracle(oracle):
    """masked protein: runs of X in a 20-letter text (5 bits per symbol, 12 symbols per key, no packed stream: the bucket X^12 is
    found among the left-over buckets of the last MSD level, not after the first)"""
    rng = np.random.default_rng(88)
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    n = 5_000_000
    t = aa[rng.integers(0, 20, n)].copy()
    at = 0
    while at < n - 2000:
        at += int(rng.integers(50, 1500)); ln = int(rng.integers(12, 900))
        t[at:at + ln] = ord("X"); at += ln
    t[np.arange(700, n, 50_000)] = ord("%")
    t[-1] = ord("$")
    norm = oracle.normalize(t, False)
    osa, olcp, _ = oracle.build(norm, is_dna=False, threads=min(32, os.cpu_count() or 1))
    db = sufr_amd.DeviceBuilder(0)
    sa, lcp = db.sort(torch.from_numpy(t).cuda(), is_dna=False, raw_text=True)
    gsa = sa.cpu().numpy().view(np.uint32); glcp = lcp.cpu().numpy().view(np.uint32)
    db.close()
    assert np.array_equal(gsa, osa) and np.array_equal(glcp, olcp)


@pytest.mark.parametrize("L", [7, 30, 400])
def test_max_query_len_on_a_text_with_a_run_bucket(L):
    """-m L after the closed-form bucket: the capped build is the canonical member of the reference's family (LCP = min(LCP, L),
    ties in descending position, the same first L characters rank by rank) of the uncapped one"""
    raw = _runs_text(71, 5_000_000, ord("N"), 6000, 21, 900)
    db = sufr_amd.DeviceBuilder(0)
    x = torch.from_numpy(raw).cuda()
    fsa, flcp = db.sort(x, is_dna=True, allow_ambiguity=True, raw_text=True)
    fsa = fsa.cpu().numpy().view(np.uint32).astype(np.int64); flcp = flcp.cpu().numpy().view(np.uint32).astype(np.int64)
    sa, lcp = db.sort(x, is_dna=True, allow_ambiguity=True, raw_text=True, max_query_len=L)
    sa = sa.cpu().numpy().view(np.uint32).astype(np.int64); lcp = lcp.cpu().numpy().view(np.uint32).astype(np.int64)
    db.close()
    assert np.array_equal(np.sort(sa), np.sort(fsa))
    assert np.array_equal(lcp, np.minimum(flcp, L))
    tie = lcp >= L
    assert np.all(sa[1:][tie[1:]] < sa[:-1][tie[1:]]), "ties must come in descending position"
    W = min(L, 48)
    assert np.array_equal(_first_chars(raw, sa, W), _first_chars(raw, fsa, W))


@pytest.mark.parametrize("letters", [b"AC", b"ACDEFGHIKLMN"])
def test_run_buckets_in_2_and_4_bit_alphabets_equal_oracle(oracle, letters):
    """the closed form with first digits of 7 symbols (2-bit codes) and of 3 symbols (4-bit codes): a generic alphabet, not the DNA
    table; the repeated symbol is the largest letter (every run is followed by a smaller one or the end: one class) or a middle
    one (both classes)"""
    rng = np.random.default_rng(len(letters))
    al = np.frombuffer(letters, dtype=np.uint8)
    n = 5_000_000
    t = al[rng.integers(0, al.size, n)].copy()
    sym = int(al[-1]) if al.size == 2 else int(al[al.size // 2])
    at = 0
    while at < n - 2000:
        at += int(rng.integers(30, 1200)); ln = int(rng.integers(8, 900))
        t[at:at + ln] = sym; at += ln
    t[-1] = ord("$")
    osa, olcp, _ = oracle.build(t, is_dna=False, threads=min(32, os.cpu_count() or 1))
    db = sufr_amd.DeviceBuilder(0)
    sa, lcp = db.sort(torch.from_numpy(t).cuda(), is_dna=False)
    gsa = sa.cpu().numpy().view(np.uint32); glcp = lcp.cpu().numpy().view(np.uint32)
    db.close()
    assert np.array_equal(gsa, osa) and np.array_equal(glcp, olcp)


@pytest.mark.parametrize("shards", [1, 2, 3])
def test_stalling_repeats_over_shards_equal_oracle(oracle, shards):
    """Thousands of copies of three 300-symbol templates: the re-keying levels stop shrinking and, on one GPU, prefix doubling takes
    over -- it keys a suffix by the RANK of a later position, which exists only if every suffix of the text is in the build.  A
    shard holds its own first-digit range only: there the build must stay with the levels (round 4's soak found 38 000 wrong ranks
    in such a text over two shards, and a memory fault)."""
    raw = _templated_runs_text(9, 6000, 6, 700, ntemplates=3, tlen=300)
    kw = dict(is_dna=True, allow_ambiguity=True)
    osa, olcp, _ = oracle.build(oracle.normalize(raw, False), threads=min(32, os.cpu_count() or 1), **kw)
    db = sufr_amd.DeviceBuilder(0)
    x = torch.from_numpy(raw).cuda()
    if shards == 1:
        sa, lcp = db.sort(x, raw_text=True, **kw)
        gsa = sa.cpu().numpy().view(np.uint32); glcp = lcp.cpu().numpy().view(np.uint32)
    else:
        gsa, glcp, _ = _sharded_arrays(db, x, x.numel(), shards, raw_text=True, **kw)
    db.close()
    assert np.array_equal(gsa, osa) and np.array_equal(glcp, olcp)


@pytest.mark.parametrize("case", ["long_n_runs", "all_a", "one_class"])
def test_buckets_of_one_repeated_symbol_with_very_long_runs_are_exact(case):
    """Runs of 10^5 - 10^6 symbols (the rectangles above the table; one run of 3 * 10^6 'A' is a single rectangle): the byte-walking
    reference cannot check these in reasonable time; an exact run-walking comparison of sampled adjacent ranks does, inside the
    bucket densely."""
    rng = np.random.default_rng(77)
    kw = dict(is_dna=True)
    if case == "long_n_runs":
        raw = _runs_text(61, 9_000_000, ord("N"), 2500, 21, 3000, extra=(1_500_000, 1_100_000, 300_000, 299_999, 70_000, 70_001, 5000))
        kw["allow_ambiguity"] = True
    elif case == "all_a":
        raw = np.concatenate([np.full(3_000_000, ord("A"), np.uint8), np.frombuffer(b"$", dtype=np.uint8)])
    else:                                                          # every run of T is followed by a smaller symbol: one class only
        raw = _runs_text(62, 6_000_000, ord("T"), 3000, 21, 1500, extra=(400_000, 90_000))
    db = sufr_amd.DeviceBuilder(0)
    sa, lcp = db.sort(torch.from_numpy(raw).cuda(), raw_text=True, **kw)
    sa = sa.cpu().numpy().view(np.uint32).astype(np.int64); lcp = lcp.cpu().numpy().view(np.uint32).astype(np.int64)
    db.close()
    elig = np.ones(raw.size, bool) if kw.get("allow_ambiguity") else np.isin(raw, np.frombuffer(b"ACGT$", dtype=np.uint8))
    assert sa.size == int(elig.sum()) and np.array_equal(np.sort(sa), np.flatnonzero(elig))
    change = np.flatnonzero(raw[1:] != raw[:-1]) + 1
    starts = np.concatenate([[0], change, [raw.size]])
    sym = {"long_n_runs": ord("N"), "all_a": ord("A"), "one_class": ord("T")}[case]
    inside = np.flatnonzero((raw[sa] == sym) & (lcp >= 21))       # ranks of the bucket (and a few of its neighbours)
    ranks = np.concatenate([rng.integers(1, sa.size, 15_000), inside[rng.integers(0, inside.size, 45_000)],
                            inside[:50], inside[-50:]])
    for r in ranks.tolist():
        if r == 0:
            continue
        k, less = _rle_lcp_and_order(raw, starts, int(sa[r - 1]), int(sa[r]))
        assert less and lcp[r] == k, (case, r, int(sa[r - 1]), int(sa[r]), k, int(lcp[r]))


@pytest.mark.parametrize("kind", ["all_a", "acgt_k", "fib", "two_identical", "n_run", "tandem"])
@pytest.mark.parametrize("n", [100, 5000])
def test_adversarial_micro_inputs(ctx, oracle, kind, n):
    assert_matches_oracle(ctx, oracle, synth.adversarial(kind, n, seed=n))


def test_long_repeats_need_deeper_levels(ctx, oracle):
    """Planted long exact repeats and tandem arrays: groups larger than a wave window, LCP >> key."""
    rng = np.random.default_rng(9)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    body = acgt[rng.integers(0, 4, size=200_000)]
    unit = acgt[rng.integers(0, 4, size=3000)]
    for k in range(150):                      # 150 exact copies of a 3 kb segment
        at = 1000 + k * 1300
        body[at:at + 1000] = unit[(k * 7) % 2000:(k * 7) % 2000 + 1000]
    body[150_000:160_000] = np.resize(acgt[rng.integers(0, 4, size=5)], 10_000)
    raw = np.concatenate([body, np.frombuffer(b"$", dtype=np.uint8)])
    b = assert_matches_oracle(ctx, oracle, raw)
    assert b.stats.num_levels > 1 and b.lcp.max() > 2000


def test_many_near_identical_copies(ctx, oracle):
    """40 copies of ten 1.5-4 kb families at 1 % divergence: tie groups of ~40 suffixes that split a few
    members at a time over dozens of finisher rounds and across window borders (regression test for an
    LDS-ordering race in the wave-private exchange)."""
    g = synth._gen("cpu", 5)
    text = synth._bases(g, 1_500_000, 0.645, "cpu")
    for f in range(10):
        synth._plant_family(g, text, synth._bases(g, 1500 + f * 300, 0.645, "cpu"), 40, 0.01, 0.01, lowercase=False)
    x, _ = synth._join(text, 3)
    for _ in range(2):
        assert_matches_oracle(ctx, oracle, x.numpy())


def _copies_text(seed, n, seg_len, copies, *, n_run=0, spacing=None, mutate=0.0):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    t = acgt[rng.integers(0, 4, n)]
    seg = acgt[rng.integers(0, 4, seg_len)].copy()
    if n_run:
        seg[seg_len // 3:seg_len // 3 + n_run] = ord("N")           # the copies share a masked stretch
    spacing = spacing or (n - seg_len - 10) // copies
    for k in range(copies):
        c = seg.copy()
        if mutate:
            hit = rng.random(seg_len) < mutate
            c[hit] = acgt[rng.integers(0, 4, int(hit.sum()))]
        at = 5 + k * spacing
        t[at:at + seg_len] = c
    return np.concatenate([t, np.frombuffer(b"$", dtype=np.uint8)])


@pytest.mark.parametrize("case", [
    dict(n=1_000_000, seg_len=20_000, copies=10),                   # groups of 10: walk keys inside k_finish
    dict(n=2_000_000, seg_len=2_000, copies=300),                   # groups of 300: prefix doubling takes the level over
    dict(n=2_000_000, seg_len=3_000, copies=200, n_run=50),         # ... with run keys among the rank keys (--dna: N starts no suffix)
    dict(n=1_500_000, seg_len=4_000, copies=150, mutate=0.002),     # near-identical copies: groups split round by round
    dict(n=600_000, seg_len=2_500, copies=200, spacing=2_500),      # a tandem array of a long unit (period >> 8)
])
def test_many_copies_of_a_long_repeat(ctx, oracle, case):
    """Copies of a long segment tie for thousands of characters: ~20 characters per re-keying level would take
    hundreds of levels.  Small groups are split by walk keys (common prefix with the group's first member), large
    ones by prefix doubling over ranks with the LCPs filled in by the text-order pass (sufr_dbl.inc)."""
    raw = _copies_text(77, **case)
    b = assert_matches_oracle(ctx, oracle, raw)
    assert int(b.lcp.max()) >= case["seg_len"] - 1 - case.get("n_run", 0) * 0 - (1 if case.get("mutate") else 0) * case["seg_len"]
    assert b.stats.num_levels < 60
    if case.get("n_run"):
        assert_matches_oracle(ctx, oracle, raw, allow_ambiguity=True)


def _families_text(seed, n, families):
    """random DNA with high-copy repeat families: (unit length, copies, mutation rate) each, copies placed at random"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    t = acgt[rng.integers(0, 4, n)]
    for unit, copies, mut in families:
        fam = acgt[rng.integers(0, 4, unit)]
        at = rng.integers(0, n - unit - 1, copies)
        for a in at:
            c = fam.copy()
            if mut:
                hit = rng.random(unit) < mut
                c[hit] = acgt[rng.integers(0, 4, int(hit.sum()))]
            t[a:a + unit] = c
    return np.concatenate([t, np.frombuffer(b"$", dtype=np.uint8)])


@pytest.mark.parametrize("families,n", [
    ([(300, 9_000, 0.01)], 4_000_000),                                  # groups of ~6 000 records: one workgroup each
    ([(300, 9_000, 0.01), (60, 30_000, 0.002)], 5_000_000),            # ... and groups of ~22 000 among them: side by side
    ([(150, 2_000, 0.02), (400, 900, 0.0), (40, 60_000, 0.0)], 4_000_000),   # small windows, an exact family, one of 60 000 copies
])
def test_high_copy_families_sort_their_groups_in_place(ctx, oracle, families, n):
    """Re-keying levels sort every group where it lies (k_group_sort_small / _big, k_large_*): families of thousands of
    near-identical copies give tie groups of every size class in the same level -- windows of small groups, groups above
    4 096 records, groups above 16 384 records next to them."""
    raw = _families_text(5, n, families)
    b = assert_matches_oracle(ctx, oracle, raw)
    assert b.stats.num_levels >= 3 and b.stats.deep_records > 1_000_000


def test_protein_alphabet(ctx, oracle):
    d = sufr_amd.read_sequence_file(GOLDEN / "inputs" / "uniprot.fa")
    assert_matches_oracle(ctx, oracle, np.frombuffer(d.seq, dtype=np.uint8), is_dna=False)


def test_text_without_sentinel_and_binary_bytes(ctx, oracle):
    rng = np.random.default_rng(21)
    raw = rng.integers(0, 256, size=50_000, dtype=np.uint8)          # all 256 byte values, zeros included
    raw[(raw >= 97) & (raw <= 122)] = 0                               # (lowercase would be case-folded)
    assert_matches_oracle(ctx, oracle, raw, is_dna=False)
    raw = np.frombuffer(b"ABABABABABABABABABABABAB" * 40, dtype=np.uint8)   # no '$': proper-prefix ties
    assert_matches_oracle(ctx, oracle, raw, is_dna=False)
    raw = np.zeros(3000, dtype=np.uint8)                              # a run of 0x00 bytes
    assert_matches_oracle(ctx, oracle, raw, is_dna=False)


def test_elegans_like_5m(ctx, oracle):
    x, _ = synth.syn_elegans(5_000_000, seed=2)
    assert_matches_oracle(ctx, oracle, x.numpy())


def test_ecoli_config_c2(ctx, oracle):
    """BASELINE config C2: E. coli-sized (4.64 Mb) --dna, bit-exact vs the CPU build."""
    x, _ = synth.syn_ecoli(4_641_652, seed=1)
    b = assert_matches_oracle(ctx, oracle, x.numpy())
    assert b.num_suffixes == 4_641_653


# ---- device-resident API, shards --------------------------------------------------------------------
def test_device_api_and_shards_concatenate(oracle):
    x, _ = synth.syn_human(3_000_000, seed=5)
    raw = x.numpy()
    norm = oracle.normalize(raw, True)
    sa, lcp, _ = oracle.build(norm, is_dna=True, threads=8)
    db = sufr_amd.DeviceBuilder(0)
    d_text = torch.from_numpy(raw).cuda()
    fsa, flcp = db.sort(d_text, is_dna=True, ignore_softmask=True, raw_text=True)
    assert np.array_equal(fsa.cpu().numpy().view(np.uint32), sa)
    assert np.array_equal(flcp.cpu().numpy().view(np.uint32), lcp)
    for shards in (2, 3, 8):
        parts_sa, parts_lcp = [], []
        for r in range(shards):
            psa, plcp = db.sort(d_text, is_dna=True, ignore_softmask=True, raw_text=True, shard_index=r,
                                num_shards=shards)
            assert db.stats.partition_variant == 3
            psa = psa.cpu().numpy().view(np.uint32).copy(); plcp = plcp.cpu().numpy().view(np.uint32).copy()
            if parts_sa and psa.size:      # boundary stitch: find_lcp(prev.last, this.first) (893-902)
                prev = next(p for p in reversed(parts_sa) if p.size)
                plcp[0] = sufr_amd.lcp_pair(norm, int(prev[-1]), int(psa[0]))
            parts_sa.append(psa); parts_lcp.append(plcp)
        assert np.array_equal(np.concatenate(parts_sa), sa)
        assert np.array_equal(np.concatenate(parts_lcp), lcp)
    db.close()


def test_device_stitch_sets_the_boundary_lcp_without_the_host(oracle):
    """sufr_hip_stitch_device_u32 (the timed N > 1 step of bench.py): {first, last, count} of every shard in ONE
    device tensor, LCP[0] of a shard set by a kernel on the context's text -- against the single build, with an
    empty shard between two others (the kernel looks for the nearest non-empty one)."""
    from sufr_amd import shards as sh
    x, _ = synth.syn_human(2_000_000, seed=21)
    raw = x.numpy()
    db = sufr_amd.DeviceBuilder(0)
    d_text = torch.from_numpy(raw).cuda()
    fsa, flcp = (t.clone() for t in db.sort(d_text, is_dna=True, ignore_softmask=True, raw_text=True))
    for world in (2, 4):
        parts, rows = [], []
        for r in range(world):
            psa, plcp = db.sort(d_text, is_dna=True, ignore_softmask=True, raw_text=True, shard_index=r, num_shards=world)
            parts.append((psa.clone(), plcp.clone()))
            rows.append(sh.gather_boundaries_device(psa, int(psa.numel())))
        # an empty shard squeezed in after shard 0: bounds rows {0, 0, 0}
        bounds = torch.cat([rows[0], torch.zeros(1, 3, dtype=torch.int64, device="cuda")] + rows[1:]).contiguous()
        off = 0
        for r in range(world):
            psa, plcp = parts[r]
            # (the context's text is the one of the last build: the same text for every shard)
            if r > 0:
                plcp[0] = -1
                sh.stitch_device(db.ctx, raw.size, bounds, r + 1, plcp)
            assert torch.equal(psa, fsa[off:off + psa.numel()])
            assert torch.equal(plcp, flcp[off:off + psa.numel()]), f"world {world} shard {r}"
            off += psa.numel()
        assert off == fsa.numel()
    db.close()


def test_options_on_a_5mb_genome(oracle, tmp_path):
    """-m and -s at a size where the tie runs fill many tiles (human-like repeats, 5 Mb)."""
    x, _ = synth.syn_human(5_000_000, seed=9)
    raw = x.numpy()
    db = sufr_amd.DeviceBuilder(0)
    d_text = torch.from_numpy(raw).cuda()
    fsa, flcp = (t.clone() for t in db.sort(d_text, is_dna=True, ignore_softmask=True, raw_text=True))
    for L in (8, 16, 33):
        msa, mlcp = db.sort(d_text, is_dna=True, ignore_softmask=True, raw_text=True, max_query_len=L)
        assert torch.equal(mlcp, torch.clamp(flcp, max=L))
        assert torch.equal(torch.sort(msa)[0], torch.sort(fsa)[0])
        tie = mlcp[1:] >= L
        assert bool(torch.all(msa[1:][tie] < msa[:-1][tie]))
        # same first L characters rank by rank as the exact build
        norm = torch.from_numpy(oracle.normalize(raw, True)).cuda()
        pad = torch.cat([norm, torch.zeros(L, dtype=torch.uint8, device="cuda")])
        pick = torch.randint(0, msa.numel(), (200_000,), device="cuda")
        ar = torch.arange(L, device="cuda")
        assert torch.equal(pad[(msa[pick].long()[:, None] + ar[None, :])],
                           pad[(fsa[pick].long()[:, None] + ar[None, :])])
    norm = oracle.normalize(raw, True)
    for mask in ("1101", "110110110110110110110110110110011"):
        ssa, slcp = db.sort(d_text, is_dna=True, ignore_softmask=True, raw_text=True, seed_mask=mask)
        osa, olcp, _ = oracle.build(norm, is_dna=True, seed_mask=mask, threads=8)
        assert np.array_equal(ssa.cpu().numpy().view(np.uint32), osa)
        assert np.array_equal(slcp.cpu().numpy().view(np.uint32), olcp)
    db.close()


def test_native_cli_seed_mask_and_max_query_len(tmp_path):
    out = tmp_path / "um.sufr"
    r = subprocess.run([str(sufr_amd.CLI_PATH), "create", "-s", "10111011", "-o", str(out),
                        str(GOLDEN / "inputs" / "uniprot.fa")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == (GOLDEN / "expected" / "uniprot-masked.sufr").read_bytes()
    out = tmp_path / "m.sufr"
    r = subprocess.run([str(sufr_amd.CLI_PATH), "create", "-d", "-m", "2", "-o", str(out),
                        str(GOLDEN / "inputs" / "2.fa")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    g = parse_sufr(out)
    assert g.max_query_len == 2 and g.lcp.tolist() == np.minimum(
        parse_sufr(GOLDEN / "expected" / "2.sufr").lcp, 2).tolist()


# ---- randomised differential test --------------------------------------------------------------------
def _fuzz_text(rng):
    """A small text with a random alphabet, repeat structure, case mix and terminator."""
    n = int(rng.choice([1, 2, 3, 5, 17, 64, 129, 700, 4097, 9000]) + rng.integers(0, 40))
    kind = int(rng.integers(0, 5))
    if kind == 0:      # DNA-like with IUPAC, N runs and lowercase
        alpha = np.frombuffer(b"ACGTNacgtnRY", dtype=np.uint8)
        p = np.array([20, 20, 20, 20, 6, 3, 3, 3, 3, 1, 0.5, 0.5]); p = p / p.sum()
        t = alpha[rng.choice(alpha.size, size=n, p=p)]
    elif kind == 1:    # tiny alphabet: long runs and deep ties
        sigma = int(rng.integers(1, 4))
        t = np.frombuffer(b"ACG", dtype=np.uint8)[rng.integers(0, sigma, size=n)]
    elif kind == 2:    # periodic with mutations
        unit = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(rng.integers(1, 9)))]
        t = np.resize(unit, n).copy()
        hit = rng.random(n) < 0.01
        t[hit] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(hit.sum()))]
    elif kind == 3:    # protein-like
        alpha = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYX", dtype=np.uint8)
        t = alpha[rng.integers(0, alpha.size, size=n)]
    else:              # arbitrary bytes from a random subset
        sub = rng.choice(256, size=int(rng.integers(2, 40)), replace=False).astype(np.uint8)
        t = sub[rng.integers(0, sub.size, size=n)]
    t = t.copy()
    if n > 40 and rng.random() < 0.5:      # a copied block: long common prefixes
        ln = int(rng.integers(5, n // 3)); a = int(rng.integers(0, n - ln)); b = int(rng.integers(0, n - ln))
        t[b:b + ln] = t[a:a + ln].copy()
    if n > 10 and rng.random() < 0.5:      # several sequences
        for c in rng.integers(1, n - 1, size=int(rng.integers(1, 4))):
            t[c] = ord("%")
    if rng.random() < 0.8:
        t = np.concatenate([t, np.frombuffer(b"$", dtype=np.uint8)])
    return t


@pytest.mark.parametrize("block", range(12))
def test_fuzz_small_texts_against_oracle(ctx, oracle, block):
    rng = np.random.default_rng(1000 + block)
    for case in range(60):
        raw = _fuzz_text(rng)
        is_dna = bool(rng.random() < 0.6)
        amb = bool(rng.random() < 0.3)
        soft = bool(rng.random() < 0.5)
        if amb:
            raw = _break_long_n_runs(raw, soft)
        mask = None
        if rng.random() < 0.15:
            ml = int(rng.integers(3, 12))
            mask = "1" + "".join(rng.choice(["0", "1"], size=ml - 2)) + "1"
            if "0" not in mask or not mask.startswith("1") or "10" not in mask and "0" in mask:
                mask = "1101"
            i = mask.index("0")
            mask = "1" * i + mask[i:]
        norm = oracle.normalize(np.ascontiguousarray(raw, dtype=np.uint8), soft)
        what = dict(is_dna=is_dna, allow_ambiguity=amb)
        try:
            b = gpu_build(ctx, raw, ignore_softmask=soft, seed_mask=mask, **what)
        except sufr_amd.SufrHipError as e:
            raise AssertionError(f"block {block} case {case}: {e} (n={raw.size}, {what}, mask={mask})")
        if norm.size >= 4:
            try:
                sa, lcp, st = oracle.build(norm, seed_mask=mask, threads=4, **what)
            except RuntimeError:       # fewer eligible positions than the pivots the reference wants to draw
                if mask is not None:   # (it would spin in select_pivots, 786-800): only the witness remains
                    continue
                sa, lcp = naive_sa_lcp(norm, is_dna, amb)
        elif mask is None:
            sa, lcp = naive_sa_lcp(norm, is_dna, amb)
        else:
            continue
        ctxt = f"block {block} case {case} n={raw.size} {what} soft={soft} mask={mask}"
        assert np.array_equal(b.text, norm), ctxt
        assert np.array_equal(b.suffix_array, sa), ctxt
        assert np.array_equal(b.lcp, lcp), ctxt


@pytest.mark.parametrize("block", range(4))
def test_fuzz_shards_concatenate_to_the_single_build(block):
    """Any number of prefix-bucket shards (empty ones included) concatenates to the one-GPU arrays once the
    first LCP of every non-empty shard but the first is stitched (sufr_builder.rs:893-902)."""
    rng = np.random.default_rng(5000 + block)
    db = sufr_amd.DeviceBuilder(0)
    for case in range(25):
        raw = _fuzz_text(rng)
        is_dna = bool(rng.random() < 0.6)
        soft = bool(rng.random() < 0.5)
        d_text = torch.from_numpy(raw).cuda()
        fsa, flcp = db.sort(d_text, is_dna=is_dna, ignore_softmask=soft, raw_text=True)
        fsa = fsa.cpu().numpy().view(np.uint32).copy(); flcp = flcp.cpu().numpy().view(np.uint32).copy()
        norm = sufr_amd.normalize(raw, soft)
        shards = int(rng.choice([2, 3, 5, 8]))
        parts_sa, parts_lcp = [], []
        for r in range(shards):
            psa, plcp = db.sort(d_text, is_dna=is_dna, ignore_softmask=soft, raw_text=True, shard_index=r,
                                num_shards=shards)
            psa = psa.cpu().numpy().view(np.uint32).copy(); plcp = plcp.cpu().numpy().view(np.uint32).copy()
            prev = next((p for p in reversed(parts_sa) if p.size), None)
            if prev is not None and psa.size:
                plcp[0] = sufr_amd.lcp_pair(norm, int(prev[-1]), int(psa[0]))
            parts_sa.append(psa); parts_lcp.append(plcp)
        ctxt = f"block {block} case {case} n={raw.size} shards={shards} dna={is_dna} soft={soft}"
        assert np.array_equal(np.concatenate(parts_sa), fsa), ctxt
        assert np.array_equal(np.concatenate(parts_lcp), flcp), ctxt
    db.close()


def _sharded_arrays(db, d_text, n, shards, **kw):
    """every shard built on the one context, its first LCP stitched on the device under the order of the build
    (sufr_hip_stitch_device_u32), concatenated"""
    from sufr_amd import shards as sh
    parts_sa, parts_lcp, bounds = [], [], torch.zeros(shards, 3, dtype=torch.int64, device="cuda")
    for r in range(shards):
        psa, plcp = db.sort(d_text, shard_index=r, num_shards=shards, **kw)
        cnt = psa.numel()
        if cnt:
            bounds[r, 0] = int(psa[0]) & 0xFFFFFFFF; bounds[r, 1] = int(psa[-1]) & 0xFFFFFFFF; bounds[r, 2] = cnt
            plcp = plcp.clone()
            sh.stitch_device(db.ctx, n, bounds[:r + 1].contiguous(), r, plcp)
            db.ctx.synchronize()
        parts_sa.append(psa.cpu().numpy().view(np.uint32).copy()); parts_lcp.append(plcp.cpu().numpy().view(np.uint32).copy())
    return np.concatenate(parts_sa), np.concatenate(parts_lcp), [p.size for p in parts_sa]


@pytest.mark.parametrize("block", range(3))
def test_fuzz_shards_of_masked_and_capped_builds_concatenate_to_the_single_build(block):
    """--seed-mask and --max-query-len builds over 2 / 3 / 5 / 8 shards (missing 2): a masked build is split on its
    own first key digit, a capped one on the first digit of the plain order; the boundary LCP is the care-symbol count /
    the capped count (k_lcp_stitch under the order of the build).  Concatenated, the shards are the one-GPU arrays."""
    rng = np.random.default_rng(8100 + block)
    db = sufr_amd.DeviceBuilder(0)
    for case in range(16):
        raw = _fuzz_text(rng)
        is_dna = bool(rng.random() < 0.6)
        soft = bool(rng.random() < 0.5)
        kw = dict(is_dna=is_dna, ignore_softmask=soft, raw_text=True)
        if rng.random() < 0.6:
            ones = int(rng.integers(1, 5))                   # regex ^1+0[01]*1$ (types.rs:163-166)
            kw["seed_mask"] = "1" * ones + "0" + "".join(rng.choice(["0", "1"], size=int(rng.integers(0, 16)))) + "1"
        else:
            kw["max_query_len"] = int(rng.choice([8, 9, 12, 16, 31, 100]))
        d_text = torch.from_numpy(raw).cuda()
        fsa, flcp = db.sort(d_text, **kw)
        fsa = fsa.cpu().numpy().view(np.uint32).copy(); flcp = flcp.cpu().numpy().view(np.uint32).copy()
        shards = int(rng.choice([2, 3, 5, 8]))
        csa, clcp, sizes = _sharded_arrays(db, d_text, raw.size, shards, **kw)
        ctxt = f"block {block} case {case} n={raw.size} shards={shards} sizes={sizes} {kw}"
        assert np.array_equal(csa, fsa), ctxt
        assert np.array_equal(clcp, flcp), ctxt
    with pytest.raises(sufr_amd.SufrHipError):              # a cap shorter than a first digit ties suffixes across shards
        db.sort(d_text, is_dna=True, max_query_len=3, shard_index=0, num_shards=2)
    db.close()


@pytest.mark.parametrize("kind", range(8))
def test_fuzz_structured_texts_against_oracle(ctx, oracle, kind):
    """20 k - 400 k texts with the structures that stress different parts of the pipeline: families of
    near-identical copies, tandem arrays of several periods, N runs with lowercase, long homopolymers, protein,
    exact duplicates of long segments, a two-letter alphabet."""
    rng = np.random.default_rng(700 + kind)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for case in range(5):
        n = int(rng.integers(20_000, 400_000))
        t = acgt[rng.integers(0, 4, n)]
        if kind == 1:
            fam = acgt[rng.integers(0, 4, int(rng.integers(200, 3000)))]
            for _ in range(int(rng.integers(5, 200))):
                at = int(rng.integers(0, n - fam.size)); c = fam.copy()
                hit = rng.random(fam.size) < rng.choice([0.0, 0.001, 0.02, 0.1])
                c[hit] = acgt[rng.integers(0, 4, int(hit.sum()))]
                t[at:at + fam.size] = c
        elif kind == 2:
            for _ in range(30):
                u = acgt[rng.integers(0, 4, int(rng.integers(1, 12)))]
                ln = int(rng.integers(50, 5000)); at = int(rng.integers(0, n - ln))
                t[at:at + ln] = np.resize(u, ln)
        elif kind == 3:
            t = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)[rng.integers(0, 9, n)]
            for _ in range(40):
                ln = int(rng.integers(1, 900)); at = int(rng.integers(0, n - ln)); t[at:at + ln] = ord("N")
        elif kind == 4:
            for _ in range(10):
                ln = int(rng.integers(100, 30000)); at = int(rng.integers(0, n - ln))
                t[at:at + ln] = acgt[rng.integers(0, 4)]
        elif kind == 5:
            t = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)[rng.integers(0, 20, n)]
        elif kind == 6:
            for _ in range(6):
                ln = int(rng.integers(500, 20000)); a = int(rng.integers(0, n - ln)); b = int(rng.integers(0, n - ln))
                t[b:b + ln] = t[a:a + ln].copy()
        elif kind == 7:
            t = acgt[rng.integers(0, 2, n)]
        t = t.copy()
        for c in rng.integers(1, n - 1, size=int(rng.integers(0, 5))):
            t[c] = ord("%")
        raw = np.concatenate([t, np.frombuffer(b"$", dtype=np.uint8)])
        soft = bool(rng.random() < 0.5)
        amb = bool(kind == 3 and rng.random() < 0.5)
        if amb:
            raw = _break_long_n_runs(raw, soft)
        assert_matches_oracle(ctx, oracle, raw, is_dna=kind != 5, allow_ambiguity=amb, ignore_softmask=soft)


# ---- BASELINE-sized property checks ---------------------------------------------------------------------
def test_elegans_config_c3_properties(oracle):
    """BASELINE config C3 size (100 Mb, 7 sequences): too big for the oracle in seconds, so check the
    size-independent properties: permutation of the eligible positions, order and exact LCP on 2e5 sampled
    adjacent ranks, plus the oracle on a prefix-range of the SA."""
    x, _ = synth.syn_elegans(100_286_401, seed=2, device="cuda")
    db = sufr_amd.DeviceBuilder(0)
    sa, lcp = db.sort(x, is_dna=True, raw_text=True)
    st = db.stats.as_dict()
    norm = oracle.normalize(x.cpu().numpy(), False)
    check_sa_lcp_properties(norm, sa.cpu().numpy().view(np.uint32), lcp.cpu().numpy().view(np.uint32),
                            is_dna=True, allow_ambiguity=False, sample=200_000, seed=1)
    assert st["num_suffixes"] == 100_286_402 - 6      # 6 delimiter positions are not suffix starts
    # the same text in 3 prefix-bucket shards (splitters from the sampled k-mer histogram): concatenation
    # must equal the unsharded arrays except for the first LCP entry of shards 1.., which is the stitch
    full_sa, full_lcp = sa.clone(), lcp.clone()
    off = 0
    for r in range(3):
        psa, plcp = db.sort(x, is_dna=True, raw_text=True, shard_index=r, num_shards=3)
        k = psa.numel()
        assert k > 0 and torch.equal(psa, full_sa[off:off + k])
        assert torch.equal(plcp[1:], full_lcp[off + 1:off + k])
        if r > 0:
            a, b = int(full_sa[off - 1]) & 0xFFFFFFFF, int(psa[0]) & 0xFFFFFFFF
            assert sufr_amd.lcp_pair(norm, a, b) == int(full_lcp[off])
        off += k
    assert off == full_sa.numel()
    db.close()


def test_elegans_config_c3_equals_oracle(oracle):
    """BASELINE config C3 (100 Mb, 7 sequences, --dna -n 64): the whole SA and the whole LCP array equal the
    oracle's, element for element (the oracle runs on all host cores: seconds on the GPU box)."""
    x, _ = synth.syn_elegans(100_286_401, seed=2, device="cuda")
    db = sufr_amd.DeviceBuilder(0)
    sa, lcp = db.sort(x, is_dna=True, raw_text=True, num_partitions=64)
    norm = oracle.normalize(x.cpu().numpy(), False)
    osa, olcp, _ = oracle.build(norm, is_dna=True, num_partitions=64, threads=os.cpu_count() or 1)
    assert np.array_equal(sa.cpu().numpy().view(np.uint32), osa)
    assert np.array_equal(lcp.cpu().numpy().view(np.uint32), olcp)
    db.close()


def test_seed_mask_build_at_100mb_equals_oracle(oracle):
    """--seed-mask at the size of the reference's own large masked build (Makefile:82, `-s 111010010100110111`): the
    100 Mb C3 stand-in, whole SA and whole LCP against the oracle (which orders by the care characters and breaks ties
    by descending position, sufr_builder.rs:272-300, 701-712)."""
    mask = "111010010100110111"
    x, _ = synth.syn_elegans(100_286_401, seed=2, device="cuda")
    db = sufr_amd.DeviceBuilder(0)
    sa, lcp = db.sort(x, is_dna=True, raw_text=True, num_partitions=64, seed_mask=mask)
    norm = oracle.normalize(x.cpu().numpy(), False)
    osa, olcp, _ = oracle.build(norm, is_dna=True, num_partitions=64, seed_mask=mask, threads=os.cpu_count() or 1)
    assert np.array_equal(sa.cpu().numpy().view(np.uint32), osa)
    assert np.array_equal(lcp.cpu().numpy().view(np.uint32), olcp)
    # ... and as eight shards (what eight GPUs build): split on the first key digit of the masked order, first LCPs stitched
    # with the care-symbol count, concatenated
    del sa, lcp
    csa, clcp, sizes = _sharded_arrays(db, x, x.numel(), 8, is_dna=True, raw_text=True, num_partitions=64, seed_mask=mask)
    assert min(sizes) > 0 and max(sizes) < 2 * (sum(sizes) // 8)
    assert np.array_equal(csa, osa) and np.array_equal(clcp, olcp)
    db.close()


def test_bench_reads_a_real_fasta_through_the_package_reader(tmp_path):
    """SUFR_BENCH_FASTA (real assemblies only if present on the box): bench.py must parse the file with
    the package's own reader, build it with the workload's flags and label the line `"data": "real"`."""
    import json
    import subprocess
    x, _ = synth.syn_human(300_000, seed=11)
    body = x.numpy()[:-1]
    fa = tmp_path / "tiny.fa"
    with open(fa, "wb") as f:
        f.write(b">chrA test\n")
        for i in range(0, 200_000, 70):
            f.write(body[i:min(i + 70, 200_000)].tobytes() + b"\n")
        f.write(b">chrB\n" + body[200_000:].tobytes() + b"\n")
    env = dict(os.environ, SUFR_BENCH_FASTA=str(fa))
    import sys
    from pathlib import Path
    r = subprocess.run([sys.executable, str(Path(__file__).resolve().parent.parent / "bench.py"), "--workload", "human", "--steps", "2", "--warmup", "1",
                        "--full", "--no-cpu-baseline", "--no-e2e", "--no-search", "--placement-trials", "1"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-400:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["data"] == "real" and "tiny.fa (2 sequences)" in line["config"]["workload"]
    assert line["config"]["text_len"] == body.size + 2            # the delimiter and the sentinel
    assert line["verified"]["ranks"] > 0               # the arrays of the timed step were checked against the text


def test_human_prefix_400mb_section_hashes_equal_oracle(oracle):
    """The first 400 Mb of the C4 stand-in (+ '$'), --dna --ignore-softmask -n 256: xxh64 of the SA section and of
    the LCP section (the bytes `sufr create` writes) equal the hashes of the oracle's arrays (SURVEY 8d gate)."""
    import xxhash
    x, _ = synth.syn_human(3_100_000_000, seed=4, device="cuda")
    x = x[:400_000_001].clone()
    x[-1] = ord("$")
    db = sufr_amd.DeviceBuilder(0)
    sa, lcp = db.sort(x, is_dna=True, ignore_softmask=True, raw_text=True, num_partitions=256)
    norm = oracle.normalize(x.cpu().numpy(), True)
    osa, olcp, _ = oracle.build(norm, is_dna=True, num_partitions=256, threads=os.cpu_count() or 1)
    gsa = sa.cpu().numpy().view(np.uint32); glcp = lcp.cpu().numpy().view(np.uint32)
    assert gsa.size == osa.size
    assert xxhash.xxh64(gsa.tobytes()).hexdigest() == xxhash.xxh64(osa.tobytes()).hexdigest()
    assert xxhash.xxh64(glcp.tobytes()).hexdigest() == xxhash.xxh64(olcp.tobytes()).hexdigest()
    db.close()


@pytest.mark.parametrize("mode", ["dna", "allow_ambiguity"])
def test_human_prefix_400mb_deep_modes_section_hashes_equal_oracle(oracle, mode):
    """The same 400 Mb prefix in the two modes that load the deep levels: `--dna` alone -- the soft-masked
    repeat families are indexed: 25 levels, 60 % of the suffixes tie beyond the 21-character key -- and `--dna
    --allow-ambiguity` (suffixes inside N runs indexed; the runs are broken below 1000, at random places, so that the
    reference's N-run shortcut, sufr_builder.rs:302-307, never fires and the reference is deterministic).  xxh64 of the SA and of the LCP
    section equal the oracle's."""
    import xxhash
    x, _ = synth.syn_human(3_100_000_000, seed=4, device="cuda")
    x = x[:400_000_001].clone()
    x[-1] = ord("$")
    amb = mode == "allow_ambiguity"
    if amb:
        # breaks at random places with random bases (and every 900th position, so that no run reaches 1000): a regular
        # N^899 A N^899 A ... would be a tandem array over megabases -- LCPs of 10^6 and more that the oracle's byte walk
        # (find_lcp 319-329) does not survive
        g = torch.Generator(device=x.device); g.manual_seed(5)
        isn = (x == ord("N")) | (x == ord("n"))
        brk = isn & ((torch.rand(x.numel(), generator=g, device=x.device) < 1 / 300) |
                     (torch.arange(x.numel(), device=x.device) % 900 == 0))
        bases = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=x.device)[
            torch.randint(0, 4, (x.numel(),), generator=g, device=x.device)]
        x[brk] = bases[brk]
        del isn, brk, bases
    db = sufr_amd.DeviceBuilder(0)
    sa, lcp = db.sort(x, is_dna=True, allow_ambiguity=amb, ignore_softmask=False, raw_text=True, num_partitions=256)
    assert db.stats.num_levels > 8                       # the deep path ran
    norm = oracle.normalize(x.cpu().numpy(), False)
    osa, olcp, _ = oracle.build(norm, is_dna=True, allow_ambiguity=amb, num_partitions=256, threads=os.cpu_count() or 1)
    gsa = sa.cpu().numpy().view(np.uint32); glcp = lcp.cpu().numpy().view(np.uint32)
    assert gsa.size == osa.size
    assert xxhash.xxh64(gsa.tobytes()).hexdigest() == xxhash.xxh64(osa.tobytes()).hexdigest()
    assert xxhash.xxh64(glcp.tobytes()).hexdigest() == xxhash.xxh64(olcp.tobytes()).hexdigest()
    db.close()


@pytest.mark.parametrize("kind", ["b2", "b4", "b3_many_digits", "b3_many_digits_sharded"])
def test_partition_kernel_geometries_at_40mb_equal_oracle(oracle, kind):
    """The instantiations of k_msd_part_text that the genome-shaped tests do not reach, at a size that takes the 1024-thread
    tiles (n >= 2^25): 2-bit codes (three symbols), 4-bit codes (twelve symbols), and 3-bit codes whose first digits are too
    many for a 65 536-position tile beside the counter arrays -- A C G T N mixing freely under --allow-ambiguity plus a few
    stray delimiters: ~3 500 five-mers, the half-size-tile fallback (RNDS = 1) --, the last one also as five shards.
    Whole SA and LCP against the oracle."""
    rng = np.random.default_rng({"b2": 1, "b4": 2}.get(kind, 3))
    n = 40_000_000
    if kind == "b2":
        raw = np.frombuffer(b"ACG", dtype=np.uint8)[rng.integers(0, 3, n)]
        kw = dict(is_dna=False)
    elif kind == "b4":
        raw = np.frombuffer(b"ACDEFGHIKLMN", dtype=np.uint8)[rng.integers(0, 12, n)]
        kw = dict(is_dna=False)
    else:
        # A C G T N mixing freely (5^5 = 3 125 five-mers) + 80 stray '%' (five new five-mers each): ~3 500 first digits
        raw = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, n)].copy()
        raw[rng.integers(0, n - 1, 80)] = ord("%")
        kw = dict(is_dna=True, allow_ambiguity=True)
    raw = raw.copy()
    raw[-1] = ord("$")
    x = torch.from_numpy(raw).cuda()
    db = sufr_amd.DeviceBuilder(0)
    if kind.endswith("sharded"):
        gsa, glcp, sizes = _sharded_arrays(db, x, n, 5, raw_text=True, **kw)
        assert min(sizes) > 0
    else:
        sa, lcp = db.sort(x, raw_text=True, **kw)
        gsa = sa.cpu().numpy().view(np.uint32); glcp = lcp.cpu().numpy().view(np.uint32)
        assert db.stats.partition_variant == (4 if kind.startswith("b3") else 3)     # the packed-stream kernel; half-size tiles for b3
    osa, olcp, _ = oracle.build(raw, threads=min(32, os.cpu_count() or 1), **kw)
    assert np.array_equal(gsa, osa)
    assert np.array_equal(glcp, olcp)
    db.close()


def test_human_config_c4_whole_arrays_hash_equal_to_the_oracle(oracle):
    """BASELINE config C4 at FULL size (3.1 Gb stand-in, --dna --ignore-softmask -n 256; 1.5 G suffixes): xxh64 of the whole SA
    and of the whole LCP array equal the hashes of the oracle's arrays (whole-array evidence used to stop
    at the 400 Mb prefix).  The oracle takes ~50 s on 32 host threads and ~70 GB of host memory: skipped on smaller hosts."""
    import xxhash
    mem_gb = os.sysconf("SC_PAGE_SIZE") * os.sysconf("SC_PHYS_PAGES") / 2**30
    if mem_gb < 200 or (os.cpu_count() or 1) < 16:
        pytest.skip(f"the oracle at 3.1 Gb needs ~70 GB of host memory and a minute of 32 threads (host: {mem_gb:.0f} GB, {os.cpu_count()} cores)")
    x, _ = synth.syn_human(3_100_000_000, seed=4, device="cuda")
    db = sufr_amd.DeviceBuilder(0)
    sa, lcp = db.sort(x, is_dna=True, ignore_softmask=True, raw_text=True, num_partitions=256)
    gsa = sa.cpu().numpy().view(np.uint32); glcp = lcp.cpu().numpy().view(np.uint32)
    raw = x.cpu().numpy()
    del x, sa, lcp
    db.close()
    torch.cuda.empty_cache()
    norm = oracle.normalize(raw, True)
    del raw
    osa, olcp, _ = oracle.build(norm, is_dna=True, num_partitions=256, threads=min(32, os.cpu_count() or 1))
    assert gsa.size == osa.size == 1_500_223_556
    assert xxhash.xxh64(gsa.tobytes()).hexdigest() == xxhash.xxh64(osa.tobytes()).hexdigest()
    assert xxhash.xxh64(glcp.tobytes()).hexdigest() == xxhash.xxh64(olcp.tobytes()).hexdigest()


def test_human_config_c4_properties():
    """BASELINE config C4 size (3.1 Gb stand-in, --dna --ignore-softmask): size-independent properties checked
    on the GPU itself (sufr_amd/verify.py) -- SA is a permutation of the eligible positions (count, sum, a
    weighted checksum and an xor of hashes against the eligibility mask); 10^6 sampled adjacent ranks plus 10^5
    sampled from the ranks with LCP >= 64 (the ones the levels beyond the packed key produce) are in order with
    the EXACT LCP, however long (walked through megabase N runs); 8 shards concatenate to the same arrays."""
    import gpu_verify as verify
    x, _ = synth.syn_human(3_100_000_000, seed=4, device="cuda")
    db = sufr_amd.DeviceBuilder(0)
    out_sa = torch.empty(1_530_000_000, dtype=torch.int32, device="cuda")
    out_lcp = torch.empty_like(out_sa)
    sa, lcp = db.sort(x, is_dna=True, ignore_softmask=True, raw_text=True, out_sa=out_sa, out_lcp=out_lcp)
    s = sa.numel()
    assert verify.check_permutation(x, sa, is_dna=True, ignore_softmask=True) == s
    lut = verify.normalize_lut("cuda", True)
    norm = torch.empty_like(x)
    for lo in range(0, x.numel(), 1 << 28):
        norm[lo:lo + (1 << 28)] = lut[x[lo:lo + (1 << 28)].long()]
    got = verify.check_sampled_ranks(norm, sa, lcp, samples=1_000_000, deep_samples=100_000, deep_min_lcp=64, seed=5)
    assert got["ranks"] == 1_100_000 and got["deep_ranks"] == 100_000 and got["max_lcp_checked"] > 10_000
    del norm
    # 8 prefix-bucket shards: identical arrays apart from the stitched first LCP of shards 1..7
    full_sa, full_lcp = sa.clone(), lcp.clone()
    off = 0
    for r in range(8):
        psa, plcp = db.sort(x, is_dna=True, ignore_softmask=True, raw_text=True, shard_index=r, num_shards=8)
        k = psa.numel()
        assert k > 0 and torch.equal(psa, full_sa[off:off + k]) and torch.equal(plcp[1:], full_lcp[off + 1:off + k])
        off += k
    assert off == s
    db.close()


def test_create_writes_through_links_and_keeps_plain_files_atomic(tmp_path):
    """`sufr create -o X` (advisor r4, medium): a NEW output and an existing plain file are written as `X.partial` and renamed
    (the existing file's mode survives, no `.partial` is left behind); a symlink, a hard-linked file and a device node are
    opened in place, as the reference's File::create does (sufr_builder.rs:819) -- the link stays a link, the other name of a
    hard-linked file sees the new bytes, `/dev/null` stays a character device."""
    import stat
    case = dict(GOLDEN_CASES["2.sufr"])
    fa = GOLDEN / "inputs" / case.pop("fa")
    want = (GOLDEN / "expected" / "2.sufr").read_bytes()

    def cli(out):
        r = subprocess.run([str(sufr_amd.CLI_PATH), "create", "--dna", "-o", str(out), str(fa)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr

    new = tmp_path / "new.sufr"
    cli(new)
    assert new.read_bytes() == want and not (tmp_path / "new.sufr.partial").exists()
    plain = tmp_path / "plain.sufr"
    plain.write_bytes(b"old contents")
    plain.chmod(0o600)
    cli(plain)
    assert plain.read_bytes() == want and stat.S_IMODE(plain.stat().st_mode) == 0o600
    assert not (tmp_path / "plain.sufr.partial").exists()
    target = tmp_path / "target.bin"
    target.write_bytes(b"x")
    link = tmp_path / "link.sufr"
    link.symlink_to(target)
    cli(link)
    assert link.is_symlink() and target.read_bytes() == want
    a, b = tmp_path / "a.sufr", tmp_path / "b.sufr"
    a.write_bytes(b"y")
    os.link(a, b)
    cli(a)
    assert a.read_bytes() == want and b.read_bytes() == want and a.stat().st_ino == b.stat().st_ino
    cli("/dev/null")
    assert stat.S_ISCHR(os.stat("/dev/null").st_mode) and not os.path.exists("/dev/null.partial")
