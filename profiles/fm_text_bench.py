"""Text samples, extract, the index file and the copies of the FM-index (include/sufr_fm_text.h), in one session:
    python profiles/fm_text_bench.py [text_len] [windows]
Builds the index of a synthetic genome (synth.syn_human, --dna --allow-ambiguity: every position indexed, s == n) on the device,
wraps it in place and times, with HIP events around the call on the context's stream (FM_BENCH_WARMUP warm-up calls,
FM_BENCH_REPS timed ones: median, min and max):
  the FM build at sample 32 and 8, with and without SUFR_FM_TEXT, with the bytes per rank of both;
  sufr_hip_fm_extract_batch_device of `windows` windows of 50 and of 150 bytes and of the whole text, as ms, bytes/s and LF
  steps/s -- equal bytes are asserted against the resident text before anything is timed -- beside the same requests gathered
  from the resident text by a plain indexed copy, and beside the step rate of k_fm_locate (sufr_hip_fm_locate_batch_device);
  on the host (wall clock): download, save, load (beside a plain read of the same file: the rest is the verification) and
  upload, with the file sizes."""
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
from sufr_amd._lib import FM_TEXT

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(float(args[0])) if args else 100_000_000
nw = int(float(args[1])) if len(args) > 1 else 1_000_000
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
print(f"text {N:,} suffixes {s:,} (--allow-ambiguity): index ready in {time.time() - t0:.1f} s; {nw:,} windows a set; "
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
    print(f"{name:52s} {med:10.3f} ms (min {min(ms):.3f} max {max(ms):.3f})  {items / med / 1e3:9.2f} M {unit}/s", flush=True)
    return med


# ---- build -------------------------------------------------------------------------------------------------------------
fms = {}
for sample in (32, 8):
    for flags in (0, FM_TEXT):
        def build():
            h = C.c_void_p()
            ctx.check(L.sufr_hip_fm_build_flags(ctx.handle, ix._h, sample, flags, C.byref(h)))
            return h
        handles = []
        h, ms = timed(lambda: handles.append(build()) or handles[-1], reps=min(reps, 3), warm=1)
        for old in handles[:-1]:
            L.sufr_hip_fm_free(old)
        fm = sufr_amd.DeviceFmIndex(ctx, h, 4)
        info, tinfo = fm.info, fm.text_info
        line(f"fm_build sample {sample}{' + text samples' if flags else ''}", ms, s, "ranks")
        print(f"    {info['bytes'] / s:.3f} bytes per rank + {tinfo['text_bytes'] / s:.3f} of text samples = {(info['bytes'] + tinfo['text_bytes']) / s:.3f}"
              f" (text + SA: 5); file {tinfo['file_bytes']:,} bytes", flush=True)
        if flags:
            fms[sample] = fm
        else:
            fm.close()

# ---- extract -----------------------------------------------------------------------------------------------------------
g = torch.Generator(device="cuda").manual_seed(7)
sets = {}
for m in (50, 150):
    st = torch.randint(0, N - m, (nw,), generator=g, device="cuda", dtype=torch.int64)
    sets[f"{nw:,} windows of {m}"] = (st, st + m)
sets["the whole text"] = (torch.zeros(1, dtype=torch.int64, device="cuda"), torch.full((1,), N, dtype=torch.int64, device="cuda"))
torch.cuda.synchronize()
tot = C.c_uint64(0)
for name, (st, en) in sets.items():
    num, nbytes = st.numel(), int((en - st).sum().item())
    off = torch.empty(num + 1, dtype=torch.int64, device="cuda")
    out = torch.empty(nbytes + 1, dtype=torch.uint8, device="cuda")
    # the same requests from the resident text: one indexed copy (the windows), or one copy (the whole text)
    if num > 1:
        m = nbytes // num
        idx = (st[:, None] + torch.arange(m, device="cuda")[None, :]).reshape(-1)
        with torch.cuda.stream(stream):
            plain = lambda: torch.index_select(norm, 0, idx)
            want, ms = timed(plain)
    else:
        with torch.cuda.stream(stream):
            plain = lambda: norm.clone()
            want, ms = timed(plain)
    t_copy = line(f"{name}: copy from the resident text", ms, nbytes, "bytes")
    for sample in (32, 8):
        fm = fms[sample]
        call = lambda: ctx.check(L.sufr_hip_fm_extract_batch_device(ctx.handle, fm._h, st.data_ptr(), en.data_ptr(), num, off.data_ptr(), out.data_ptr(),
                                                                    nbytes, C.byref(tot)))
        call(); ctx.synchronize(); stream.synchronize()
        assert tot.value == nbytes and torch.equal(out[:nbytes], want), (name, sample)
        # LF steps: every chunk walks from its top down to the lowest position it emits
        last = (en - 1) // sample
        steps = int((torch.clamp((last + 1) * sample, max=N) - st).sum().item())
        _, ms = timed(call)
        t_fm = line(f"{name}: FM extract sample {sample}", ms, nbytes, "bytes")
        print(f"    {steps:,} LF steps: {steps / statistics.median(ms) / 1e3:.1f} M steps/s; FM / copy time {t_fm / t_copy:.1f}", flush=True)
    del out, off, want

# ---- the step rate of locate, for comparison ----------------------------------------------------------------------------
nq = nw
lo = torch.randint(0, s - 1, (nq,), generator=g, device="cuda", dtype=torch.int64)
hi = lo + 1
off_b = torch.empty(nq + 1, dtype=torch.int64, device="cuda")
pos_b = torch.empty(nq + 1, dtype=torch.int32, device="cuda")
for sample in (32, 8):
    fm = fms[sample]
    loc = lambda: ctx.check(L.sufr_hip_fm_locate_batch_device(ctx.handle, fm._h, lo.data_ptr(), hi.data_ptr(), nq, 0, off_b.data_ptr(), pos_b.data_ptr(), nq, C.byref(tot)))
    loc(); ctx.synchronize()
    assert torch.equal(pos_b[:nq], sa[lo])
    steps = int((pos_b[:nq].to(torch.int64) % sample).sum().item())
    _, ms = timed(loc)
    line(f"locate {nq:,} ranks: FM sample {sample}", ms, nq, "hits")
    print(f"    {steps:,} LF steps: {steps / statistics.median(ms) / 1e3:.1f} M steps/s", flush=True)

# ---- the file and the copies (host, wall clock) ----------------------------------------------------------------------------
def wall(name, call, nbytes=None):
    t = time.perf_counter()
    out = call()
    dt = time.perf_counter() - t
    print(f"{name:52s} {dt * 1e3:10.1f} ms" + (f"  {nbytes / dt / 1e9:6.2f} GB/s" if nbytes else ""), flush=True)
    return out


with tempfile.TemporaryDirectory() as d:
    for sample in (32, 8):
        path = os.path.join(d, f"s{sample}.fm")
        host = wall(f"download sample {sample}", fms[sample].to_host)
        wall(f"save sample {sample}", lambda: host.save(path))
        size = os.path.getsize(path)
        assert size == host.text_info["file_bytes"]
        print(f"    file {size:,} bytes, {size / s:.3f} per rank", flush=True)
        wall(f"plain read of the file", lambda: np.fromfile(path, dtype=np.uint8), size)
        loaded = wall(f"load sample {sample} (read + verify)", lambda: sufr_amd.FmIndex.load(path), size)
        up = wall(f"upload sample {sample}", lambda: loaded.to_device(ctx), size)
        st, en = sets[f"{nw:,} windows of 50"]
        a = up.extract_device(st[:1000], en[:1000])
        b = fms[sample].extract_device(st[:1000], en[:1000])
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        up.close(); loaded.close(); host.close()
for f in fms.values():
    f.close()
ix.close(); db.close()
