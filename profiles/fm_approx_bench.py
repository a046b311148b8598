"""k-mismatch search by backtracking on the FM-index (include/sufr_fm_approx.h) against seed and verify on text + suffix array, in
one session:
    python profiles/fm_approx_bench.py [text_len] [reads]
Builds the index of a synthetic genome (synth.syn_human, --dna --allow-ambiguity: every position indexed, s == n) on the device,
wraps it in place, builds the FM-index at sample 8 and 32 and times, with HIP events around the call on the context's stream
(FM_BENCH_WARMUP warm-up calls, FM_BENCH_REPS timed ones, 1 and 3 where a call takes more than a second: median, min and max), for reads of 50, 100 and 150 bytes cut from the
text (A, C, G, T only, at most 16 exact occurrences) with d planted substitutions, d = 0 .. 3:
  DeviceFmIndex.approx_device at both samples;
  DeviceIndex.approx_device(max_occ=0) on text + suffix array -- equal record sets are asserted before anything is timed;
  at d == 0, search_device + locate_device of the same FM-index: what the frame machine costs over the plain backward search.
It also prints the occ steps and the leaves per read, counted by the host walk (sufr_fm_approx_steps) on the first
FM_BENCH_STEP_READS reads of every set -- the host FM-index is built from a .sufr file of the same arrays, written to a
temporary directory --, and the resident bytes of both structures."""
import ctypes as C
import os
import statistics
import sys
import tempfile
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import sufr_amd
from sufr_amd import synth

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(float(args[0])) if args else 100_000_000
nq = int(float(args[1])) if len(args) > 1 else 100_000
REPS = reps = int(os.environ.get("FM_BENCH_REPS", "7"))
WARM = warm = int(os.environ.get("FM_BENCH_WARMUP", "2"))
# FM_BENCH_SETS="100:2,150:3": only these (m, d) sets; a long measurement may be split over sessions
only = {tuple(map(int, x.split(":"))) for x in os.environ.get("FM_BENCH_SETS", "").split(",") if x}
step_reads = int(os.environ.get("FM_BENCH_STEP_READS", "2000"))
t0 = time.time()
x, _ = synth.syn_human(n, seed=4, device="cuda")
norm = torch.where((x >= 97) & (x <= 122), x - 32, x).contiguous()
del x
db = sufr_amd.DeviceBuilder(0)
sa, lcp = db.sort(norm, is_dna=True, allow_ambiguity=True)
ix = sufr_amd.DeviceIndex.wrap(db.ctx, norm, sa, is_dna=True)
s, N = sa.numel(), norm.numel()
assert s == N
print(f"text {N:,} suffixes {s:,} (--allow-ambiguity): index ready in {time.time() - t0:.1f} s; {nq:,} reads a set; "
      f"{warm} warm-up + {reps} timed calls each", flush=True)
stream = torch.cuda.Stream()                                       # the context's launches are timed on a stream of their own
L = sufr_amd.lib()
L.sufr_hip_set_stream(db.ctx.handle, stream.cuda_stream)
ctx = db.ctx


def timed(call, slow=False):
    """(result, ms of the timed calls); a call that takes more than a second gets 1 warm-up and 3 timed calls, like the build of
    fm_bench.py"""
    warm, reps = (1, min(3, REPS)) if slow else (WARM, REPS)
    ms = []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        out = call()
        b.record(stream)
        b.synchronize()
        if i >= warm:
            ms.append(a.elapsed_time(b))
    return out, ms


def line(name, ms, records):
    med = statistics.median(ms)
    print(f"{name:44s} {med:10.3f} ms (min {min(ms):.3f} max {max(ms):.3f}, {len(ms)} calls)  {nq / med / 1e3:9.3f} M reads/s  {records:,} records", flush=True)
    return med


# ---- the two structures ------------------------------------------------------------------------------------------------
fms = {sample: ix.fm_device(sample) for sample in (8, 32)}
for sample, fm in fms.items():
    print(f"FM-index sample {sample}: {fm.info['bytes']:,} bytes resident, {fm.info['bytes'] / s:.3f} a rank; text + suffix array: "
          f"{N + 4 * s:,} bytes, {(N + 4 * s) / s:.3f} a rank", flush=True)
# the host walk counts the steps: a .sufr file of the same arrays, then the host FM-index of it
t0 = time.time()
tmp = tempfile.TemporaryDirectory()
path = os.path.join(tmp.name, "bench.sufr")
h_text, h_sa, h_lcp = norm.cpu().numpy(), sa.cpu().numpy().view(np.uint32), lcp.cpu().numpy().view(np.uint32)
del lcp
starts = np.zeros(1, dtype=np.uint64)
names = (C.c_char_p * 1)(b"1")
err = C.create_string_buffer(256)
rc = L.sufr_write_file(path.encode(), 1, 1, 0, h_text.ctypes.data, h_text.size, 4, h_sa.ctypes.data, h_lcp.ctypes.data, h_sa.size, 0, 0, None,
                       starts.ctypes.data, 1, names, err, len(err))
assert rc == 0, err.value
del h_lcp, h_sa
host_file = sufr_amd.SufrFile(path)
host_fm = host_file.fm(32)
host_file.close()
tmp.cleanup()
print(f"host FM-index for the step counts ready in {time.time() - t0:.1f} s", flush=True)

# ---- the reads ---------------------------------------------------------------------------------------------------------
g = torch.Generator(device="cuda").manual_seed(7)
nxt = torch.arange(256, dtype=torch.uint8, device="cuda")
for a, b in zip(b"ACGT", b"CGTA"):
    nxt[a] = b                                                     # a planted substitution: the next base (other bytes stay)


def reads(m, d):
    """nq reads of m bytes cut from the text, of A, C, G, T only and with at most 16 exact occurrences (a read from a run of N or
    from a long repeat has millions of windows within d mismatches: that measures the output, not the search), then d planted
    substitutions"""
    at = torch.randint(0, N - m, (4 * nq,), generator=g, device="cuda")
    q = norm[(at[:, None] + torch.arange(m, device="cuda")[None, :])]
    q = q[((q == 65) | (q == 67) | (q == 71) | (q == 84)).all(dim=1)].contiguous()
    lo, hi = fms[32].search_device(q.reshape(-1), (torch.arange(q.shape[0] + 1, device="cuda", dtype=torch.int64) * m).contiguous())
    q = q[(hi - lo) <= 16][:nq].contiguous()
    assert q.shape[0] == nq, q.shape
    if d:
        places = torch.rand(nq, m, generator=g, device="cuda").argsort(dim=1)[:, :d]
        q.scatter_(1, places, nxt[q.gather(1, places).long()])
    return q.reshape(-1).contiguous(), (torch.arange(nq + 1, device="cuda", dtype=torch.int64) * m).contiguous()


def keyed(recs):
    """the records sorted by (query, position): the two paths give them in different orders"""
    key = (recs[0] << 32) | recs[2]
    key, order = torch.sort(key)
    return key, recs[1][order], recs[3][order]


for m in (50, 100, 150):
    for d in (0, 1, 2, 3):
        qb, off = reads(m, d)                                      # (drawn for every set, so that a split session sees the same reads)
        if only and (m, d) not in only:
            continue
        torch.cuda.synchronize()
        want = ix.approx_device(qb, off, d, 0, False)
        total = want[0].numel()
        slow = False
        for sample, fm in fms.items():
            t1 = time.time()
            got = fm.approx_device(qb, off, d, False)
            slow = slow or time.time() - t1 > 1.0
            assert all(torch.equal(a, b) for a, b in zip(keyed(got), keyed(want))), (m, d, sample)
        hq, ho = qb[:step_reads * m].cpu().numpy(), off[:step_reads + 1].cpu().numpy().astype(np.uint64)
        leaves, steps = np.zeros(step_reads, dtype=np.uint64), np.zeros(step_reads, dtype=np.uint64)
        assert L.sufr_fm_approx_steps(host_fm._h, hq.ctypes.data, ho.ctypes.data, step_reads, d, 0, leaves.ctypes.data, steps.ctypes.data, 0) == 0
        print(f"m={m} d={d}: {steps.mean():.1f} occ steps and {leaves.mean():.2f} leaves a read (host walk, {step_reads:,} reads), "
              f"{total / nq:.2f} records a read", flush=True)
        _, ms = timed(lambda: ix.approx_device(qb, off, d, 0, False, cap=total))
        t_sv = line(f"m={m} d={d}: seed and verify, text + SA", ms, total)
        for sample, fm in fms.items():
            _, ms = timed(lambda: fm.approx_device(qb, off, d, False, cap=total), slow)
            t_fm = line(f"m={m} d={d}: FM backtracking, sample {sample}", ms, total)
            print(f"    FM / seed-and-verify time {t_fm / t_sv:.2f}; {steps.mean() * nq / t_fm / 1e6:.2f} G occ steps/s", flush=True)
            if d == 0:
                def exact():
                    lo, hi = fm.search_device(qb, off, wait=False)
                    return fm.locate_device(lo, hi, capacity=total)
                (_, pos), ms = timed(exact)
                assert pos.numel() == total
                t_ex = line(f"m={m} d=0: FM search + locate, sample {sample}", ms, total)
                print(f"    frame machine / plain backward search time {t_fm / t_ex:.2f}", flush=True)
for fm in fms.values():
    fm.close()
ix.close(); db.close()
