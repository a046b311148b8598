"""Build, search and locate of the FM-index (include/sufr_fm.h) against the search and locate on text + suffix array, in one session:
    python profiles/fm_bench.py [text_len] [queries]
Builds the index of a synthetic genome (synth.syn_human, --dna --allow-ambiguity: every position indexed, s == n) on the device,
wraps it in place and times, with HIP events around the call on the context's stream (FM_BENCH_WARMUP warm-up calls,
FM_BENCH_REPS timed ones: median, min and max):
  the FM build at sample 32 and 8 (with info.bytes / s);
  for query sets of length 20, 50 and 150, one cut from the text and one random: sufr_hip_search_batch_device (prefix table on)
  and sufr_hip_fm_search_batch_device -- equal ranges are asserted before anything is timed;
  sufr_hip_locate_batch_device and sufr_hip_fm_locate_batch_device at sample 8 and 32 on the ranges of the cut queries of length
  20 (max_hits 16), equal positions asserted."""
import ctypes as C
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
nq = int(float(args[1])) if len(args) > 1 else 1_000_000
reps = int(os.environ.get("FM_BENCH_REPS", "7"))
warm = int(os.environ.get("FM_BENCH_WARMUP", "2"))
t0 = time.time()
x, _ = synth.syn_human(n, seed=4, device="cuda")
norm = torch.where((x >= 97) & (x <= 122), x - 32, x).contiguous()
del x
db = sufr_amd.DeviceBuilder(0)
sa, lcp = db.sort(norm, is_dna=True, allow_ambiguity=True)
del lcp
ix = sufr_amd.DeviceIndex.wrap(db.ctx, norm, sa, is_dna=True)
s, N = sa.numel(), norm.numel()
assert s == N
print(f"text {N:,} suffixes {s:,} (--allow-ambiguity): index ready in {time.time() - t0:.1f} s; {nq:,} queries a set; "
      f"{warm} warm-up + {reps} timed calls each", flush=True)
stream = torch.cuda.Stream()                                       # the context's launches are timed on a stream of their own
L = sufr_amd.lib()
L.sufr_hip_set_stream(db.ctx.handle, stream.cuda_stream)
ctx = db.ctx


def timed(call, reps=reps, warm=warm):
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


def line(name, ms, items, unit):
    med = statistics.median(ms)
    print(f"{name:44s} {med:10.3f} ms (min {min(ms):.3f} max {max(ms):.3f})  {items / med / 1e3:9.2f} M {unit}/s", flush=True)
    return med


# ---- build -------------------------------------------------------------------------------------------------------------
fms = {}
for sample in (32, 8):
    def build():
        h = C.c_void_p()
        ctx.check(L.sufr_hip_fm_build(ctx.handle, ix._h, sample, C.byref(h)))
        return h
    handles = []
    h, ms = timed(lambda: handles.append(build()) or handles[-1], reps=min(reps, 3), warm=1)
    for old in handles[:-1]:
        L.sufr_hip_fm_free(old)
    fms[sample] = sufr_amd.DeviceFmIndex(ctx, h, 4)
    info = fms[sample].info
    line(f"fm_build sample {sample}", ms, s, "ranks")
    print(f"    {info}  {info['bytes'] / s:.3f} bytes per rank (text + SA: 5)", flush=True)

# ---- search ------------------------------------------------------------------------------------------------------------
g = torch.Generator(device="cuda").manual_seed(7)
acgt = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device="cuda")
sets = {}
for m in (20, 50, 150):
    starts = torch.randint(0, N - m, (nq,), generator=g, device="cuda")
    cut = norm[(starts[:, None] + torch.arange(m, device="cuda")[None, :]).reshape(-1)].contiguous()
    rnd = acgt[torch.randint(0, 4, (nq * m,), generator=g, device="cuda")].contiguous()
    off = (torch.arange(nq + 1, device="cuda", dtype=torch.int64) * m).contiguous()
    sets[(m, "cut")] = (cut, off)
    sets[(m, "random")] = (rnd, off)
torch.cuda.synchronize()
lo_a, hi_a = (torch.empty(nq, dtype=torch.int64, device="cuda") for _ in range(2))
lo_b, hi_b = (torch.empty(nq, dtype=torch.int64, device="cuda") for _ in range(2))
fm = fms[32]
kept = {}
for (m, kind), (qb, off) in sets.items():
    sa_call = lambda: ctx.check(L.sufr_hip_search_batch_device(ctx.handle, ix._h, qb.data_ptr(), off.data_ptr(), nq, 0, 0, lo_a.data_ptr(), hi_a.data_ptr()))
    fm_call = lambda: ctx.check(L.sufr_hip_fm_search_batch_device(ctx.handle, fm._h, qb.data_ptr(), off.data_ptr(), nq, lo_b.data_ptr(), hi_b.data_ptr()))
    sa_call(); fm_call(); ctx.synchronize()
    assert torch.equal(lo_a, lo_b) and torch.equal(hi_a, hi_b), (m, kind)
    found = int((hi_a > lo_a).sum().item())
    _, ms = timed(sa_call)
    t_sa = line(f"search m={m} {kind}: text + SA", ms, nq, "queries")
    _, ms = timed(fm_call)
    t_fm = line(f"search m={m} {kind}: FM", ms, nq, "queries")
    print(f"    {found:,} of {nq:,} found; FM / SA time {t_fm / t_sa:.2f}", flush=True)
    if (m, kind) == (20, "cut"):
        kept = (lo_a.clone(), hi_a.clone())

# ---- locate ------------------------------------------------------------------------------------------------------------
lo, hi = kept
max_hits = 16
total = int((hi - lo).clamp(max=max_hits).sum().item())
off_a, off_b = (torch.empty(nq + 1, dtype=torch.int64, device="cuda") for _ in range(2))
pos_a, pos_b = (torch.empty(total + 1, dtype=torch.int32, device="cuda") for _ in range(2))
tot = C.c_uint64(0)
sa_loc = lambda: ctx.check(L.sufr_hip_locate_batch_device(ctx.handle, ix._h, lo.data_ptr(), hi.data_ptr(), nq, max_hits, off_a.data_ptr(), pos_a.data_ptr(), total, C.byref(tot)))
_, ms = timed(sa_loc)
t_sa = line(f"locate {total:,} hits: text + SA", ms, total, "hits")
for sample in (8, 32):
    f = fms[sample]
    fm_loc = lambda: ctx.check(L.sufr_hip_fm_locate_batch_device(ctx.handle, f._h, lo.data_ptr(), hi.data_ptr(), nq, max_hits, off_b.data_ptr(), pos_b.data_ptr(), total, C.byref(tot)))
    fm_loc(); ctx.synchronize()
    assert tot.value == total and torch.equal(off_a, off_b) and torch.equal(pos_a[:total], pos_b[:total]), sample
    _, ms = timed(fm_loc)
    t_fm = line(f"locate {total:,} hits: FM sample {sample}", ms, total, "hits")
    print(f"    FM / SA time {t_fm / t_sa:.2f}", flush=True)
for f in fms.values():
    f.close()
ix.close(); db.close()
