"""Matching statistics and SMEMs on a pair of FM-indexes (include/sufr_fm_match.h) against the path on text + suffix array
(include/sufr_match.h), in one session:
    python profiles/fm_match_bench.py [text_len] [reads]
Builds the index of a synthetic genome (synth.syn_human, --dna --allow-ambiguity: every position indexed, s == n) and the index
of its reversed text on the device, keeps the FM-index of the first at sample 32 and of the second at sample 0, and times, with
HIP events around the call on the context's stream (FM_BENCH_WARMUP warm-up calls, FM_BENCH_REPS timed ones: median, min, max),
for reads of 50, 100 and 150 bytes cut from the text (A, C, G, T only) with d planted substitutions, d = 0 .. 3, and for 64
queries of 100 000 bytes with a substitution every 997 bytes:
  DeviceFmIndex.matching_stats_device and smems_device (min_len 20) on the pair;
  DeviceIndex.matching_statistics_device and smems_device on text + suffix array -- equal statistics and equal records are
  asserted before anything is timed.
It prints the steps per read of the whole-query walk (sufr_fm_matching_stats_steps on the downloaded pair, the first
FM_BENCH_STEP_READS reads of every set), G steps/s, the resident bytes of the pair against text + suffix array, and the table
of the slab G of k_fm_ms on the reads of 150 and on the long queries, from which the shipped value is chosen: the best on the
reads unless it loses more than a factor of two on the long queries.  The table needs the probes build, which has the other
slabs (make -C sufr_amd/csrc probes; SUFR_AMD_PROBES_LIB=1; SUFR_PROBE_FM_MS_SLAB = 64, 128, 256); every other line is measured
at the slab that ships, in either build."""
import os
import statistics
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import sufr_amd
from sufr_amd import synth

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(float(args[0])) if args else 100_000_000
nq = int(float(args[1])) if len(args) > 1 else 100_000
REPS = int(os.environ.get("FM_BENCH_REPS", "7"))
WARM = int(os.environ.get("FM_BENCH_WARMUP", "2"))
step_reads = int(os.environ.get("FM_BENCH_STEP_READS", "2000"))
MIN_LEN = 20
SLAB_ENV = "SUFR_PROBE_FM_MS_SLAB"
os.environ.pop(SLAB_ENV, None)
t0 = time.time()
x, _ = synth.syn_human(n, seed=4, device="cuda")
norm = torch.where((x >= 97) & (x <= 122), x - 32, x).contiguous()
del x
db = sufr_amd.DeviceBuilder(0)
ctx = db.ctx
sa, lcp = db.sort(norm, is_dna=True, allow_ambiguity=True)
del lcp
ix = sufr_amd.DeviceIndex.wrap(ctx, norm, sa, is_dna=True)
s, N = sa.numel(), norm.numel()
assert s == N
fwd = ix.fm_device(32)
# the reversed text: reverse(T[:-1]) + e; its index is built, its FM-index kept at sample 0, text and suffix array freed
rtext = torch.cat([norm[:-1].flip(0), norm[-1:]]).contiguous()
db2 = sufr_amd.DeviceBuilder(0)                                    # (a builder of its own: the first one's arrays stay as they are)
rsa, rlcp = db2.sort(rtext, is_dna=True, allow_ambiguity=True)
del rlcp
rix = sufr_amd.DeviceIndex.wrap(ctx, rtext, rsa, is_dna=True)
rev = rix.fm_device(0)
rix.close()
db2.close()
del rtext, rsa
torch.cuda.empty_cache()
print(f"library {sufr_amd.LIB_PATH.name}; text {N:,} suffixes {s:,} (--allow-ambiguity): both indexes ready in {time.time() - t0:.1f} s; {nq:,} reads a set; "
      f"{WARM} warm-up + {REPS} timed calls each", flush=True)
pair_bytes = fwd.info["bytes"] + rev.info["bytes"]
print(f"FM pair: {fwd.info['bytes']:,} (sample 32) + {rev.info['bytes']:,} (sample 0) = {pair_bytes:,} bytes resident, {pair_bytes / s:.3f} a rank; "
      f"text + suffix array: {N + 4 * s:,} bytes, {(N + 4 * s) / s:.3f} a rank", flush=True)
stream = torch.cuda.Stream()                                       # the context's launches are timed on a stream of their own
L = sufr_amd.lib()
L.sufr_hip_set_stream(ctx.handle, stream.cuda_stream)
t0 = time.time()
h_fwd, h_rev = fwd.to_host(), rev.to_host()
print(f"host copies of the pair for the step counts ready in {time.time() - t0:.1f} s", flush=True)


def timed(call):
    ms = []
    for i in range(WARM + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        out = call()
        b.record(stream)
        b.synchronize()
        if i >= WARM:
            ms.append(a.elapsed_time(b))
    return out, ms


def line(name, ms, count, nbytes):
    med = statistics.median(ms)
    print(f"{name:46s} {med:10.3f} ms (min {min(ms):.3f} max {max(ms):.3f}, {len(ms)} calls)  {count / med / 1e3:9.3f} M queries/s  "
          f"{nbytes / med / 1e6:8.3f} G query bytes/s", flush=True)
    return med


g = torch.Generator(device="cuda").manual_seed(7)
nxt = torch.arange(256, dtype=torch.uint8, device="cuda")
for a, b in zip(b"ACGT", b"CGTA"):
    nxt[a] = b                                                     # a planted substitution: the next base (other bytes stay)


def reads(m, d, count):
    """`count` reads of m bytes cut from the text, of A, C, G, T only, then d planted substitutions"""
    at = torch.randint(0, N - m, (2 * count,), generator=g, device="cuda")
    q = norm[(at[:, None] + torch.arange(m, device="cuda")[None, :])]
    q = q[((q == 65) | (q == 67) | (q == 71) | (q == 84)).all(dim=1)][:count].contiguous()
    assert q.shape[0] == count, q.shape
    if d:
        places = torch.rand(count, m, generator=g, device="cuda").argsort(dim=1)[:, :d]
        q.scatter_(1, places, nxt[q.gather(1, places).long()])
    return q.reshape(-1).contiguous(), (torch.arange(count + 1, device="cuda", dtype=torch.int64) * m).contiguous()


def long_queries(count=64, m=100_000, every=997):
    at = torch.randint(0, N - m, (count,), generator=g, device="cuda")
    q = norm[(at[:, None] + torch.arange(m, device="cuda")[None, :])].contiguous()
    q[:, every // 2::every] = nxt[q[:, every // 2::every].long()]
    return q.reshape(-1).contiguous(), (torch.arange(count + 1, device="cuda", dtype=torch.int64) * m).contiguous()


def steps_of(qb, off, count):
    hq, ho = qb[:int(off[count])].cpu().numpy(), off[:count + 1].cpu().numpy().astype(np.uint64)
    steps = np.zeros(count, dtype=np.uint64)
    assert L.sufr_fm_matching_stats_steps(h_fwd._h, h_rev._h, hq.ctypes.data, ho.ctypes.data, count, steps.ctypes.data, 0) == 0
    return steps


def same_answers(qb, off, tag):
    """the statistics and the records of the pair equal those of text + suffix array, before anything is timed"""
    torch.cuda.synchronize()
    assert torch.equal(fwd.matching_stats_device(qb, off, rev), ix.matching_statistics_device(qb, off)), tag
    got, want = fwd.smems_device(qb, off, rev, MIN_LEN), ix.smems_device(qb, off, MIN_LEN)
    assert all(torch.equal(a, b) for a, b in zip(got, want)), tag
    return want[0].numel()


def measure(tag, qb, off, count, sample_steps):
    nbytes = qb.numel()
    total = same_answers(qb, off, tag)
    steps = steps_of(qb, off, sample_steps)
    per_byte = float(steps.sum()) / float(off[sample_steps])
    print(f"{tag}: {steps.mean():.1f} steps a query, {per_byte:.2f} a query byte (whole-query walk on the host, {sample_steps:,} queries); "
          f"{total / count:.2f} SMEMs a query at min_len {MIN_LEN}", flush=True)
    _, ms = timed(lambda: fwd.matching_stats_device(qb, off, rev, wait=False))
    t_ms = line(f"{tag}: FM pair, matching statistics", ms, count, nbytes)
    _, ms = timed(lambda: fwd.smems_device(qb, off, rev, MIN_LEN, cap=total))
    t_sm = line(f"{tag}: FM pair, SMEMs", ms, count, nbytes)
    _, ms = timed(lambda: ix.matching_statistics_device(qb, off, wait=False))
    t_ms0 = line(f"{tag}: text + SA, matching statistics", ms, count, nbytes)
    _, ms = timed(lambda: ix.smems_device(qb, off, MIN_LEN, cap=total))
    t_sm0 = line(f"{tag}: text + SA, SMEMs", ms, count, nbytes)
    print(f"    FM pair / text + SA time: statistics {t_ms / t_ms0:.2f}, SMEMs {t_sm / t_sm0:.2f}; {per_byte * nbytes / t_ms / 1e6:.2f} G steps/s "
          f"(slab walks take more steps than the whole-query walk that is counted)", flush=True)


for m in (50, 100, 150):
    for d in (0, 1, 2, 3):
        qb, off = reads(m, d, nq)
        measure(f"m={m} d={d}", qb, off, nq, min(step_reads, nq))
lq, loff = long_queries()
measure("64 x 100 000", lq, loff, 64, 8)

# ---- the slab of a lane ------------------------------------------------------------------------------------------------
if "probes" in sufr_amd.LIB_PATH.name:
    print("slab G of k_fm_ms: matching statistics, ms (median); G = 32 is the shipped slab", flush=True)
    rq, roff = reads(150, 1, nq)
    table = {}
    for G in (32, 64, 128, 256):
        os.environ[SLAB_ENV] = str(G)
        _, a = timed(lambda: fwd.matching_stats_device(rq, roff, rev, wait=False))
        _, b = timed(lambda: fwd.matching_stats_device(lq, loff, rev, wait=False))
        table[G] = (statistics.median(a), statistics.median(b))
        print(f"  G = {G:3d}: {nq:,} reads of 150 {table[G][0]:9.3f} ms   64 queries of 100 000 {table[G][1]:9.3f} ms", flush=True)
    os.environ.pop(SLAB_ENV, None)
    best_long = min(v[1] for v in table.values())
    ok = [G for G in table if table[G][1] <= 2 * best_long]
    choice = min(ok, key=lambda G: table[G][0])
    print(f"  choice: G = {choice} (the best on the reads among those within a factor of two of the best on the long queries)", flush=True)
else:
    print("slab G of k_fm_ms: not measured, this is not the probes build (make -C sufr_amd/csrc probes; SUFR_AMD_PROBES_LIB=1)", flush=True)
fwd.close(); rev.close(); ix.close(); db.close()
