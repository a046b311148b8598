"""Time of the repeat passes over a device-resident SA, LCP and text:   python profiles/repeat_bench.py [text_len] [min_len]
Builds the index of a synthetic genome (synth.syn_human) on the device, wraps it in place, hands the builder's LCP straight to
sufr_hip_repeats_device and times, per call, with HIP events around the call on the context's stream (REPEAT_BENCH_WARMUP
warm-up calls, REPEAT_BENCH_REPS timed ones: median, min and max):
  the counting call (fold, pyramid, prefixes, the counting search pass, one synchronisation) and the filling call (the same
  and the writing search pass) of the three kinds, and the k-mer spectrum of sufr_hip_kmers_device on the same arrays.
Beside every call: the bytes it moves by the model of DESIGN.md section 19 and the time of a plain device-to-device copy of
that many bytes in the same run -- the copy, not the code under test, is the yardstick.  Then, when the text is small enough to
write (<= 200 Mb), the host path of the written file on 16 threads, checked against the device results
(REPEAT_BENCH_NO_HOST=1 skips it)."""
import ctypes as C
import os
import statistics
import sys
import tempfile
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
import sufr_amd
from sufr_amd import synth

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
min_len = int(sys.argv[2]) if len(sys.argv) > 2 else 20
reps = int(os.environ.get("REPEAT_BENCH_REPS", "7"))
warm = int(os.environ.get("REPEAT_BENCH_WARMUP", "2"))
t0 = time.time()
x, _ = synth.syn_human(n, seed=4, device="cuda")
norm = torch.where((x >= 97) & (x <= 122), x - 32, x).contiguous()
del x
db = sufr_amd.DeviceBuilder(0)
sa, lcp = db.sort(norm, is_dna=True)
ix = sufr_amd.DeviceIndex.wrap(db.ctx, norm, sa, is_dna=True, prefix_table=False)
s, N, w = sa.numel(), norm.numel(), 4
print(f"text {N:,} suffixes {s:,} min_len {min_len}: index ready in {time.time() - t0:.1f} s; {warm} warm-up + {reps} timed calls each", flush=True)
stream = torch.cuda.Stream()                                       # the context's launches are timed on a stream of their own
L = sufr_amd.lib()
L.sufr_hip_set_stream(db.ctx.handle, stream.cuda_stream)


def timed(call):
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


def copy_ms(nbytes):
    """a device-to-device copy that reads and writes nbytes in all (nbytes / 2 each way)"""
    half = max(nbytes // 2, 1)
    src = torch.empty(half, dtype=torch.uint8, device="cuda")
    dst = torch.empty(half, dtype=torch.uint8, device="cuda")
    def copy():
        with torch.cuda.stream(stream):
            dst.copy_(src)
    return timed(copy)[1]


def count_call(kind):
    total, st = C.c_uint64(0), sufr_amd.RepeatStats()
    rc = L.sufr_hip_repeats_device(db.ctx.handle, ix._h, lcp.data_ptr(), None, 0, kind, min_len, 2, 0, 0, None, None, None, C.byref(total), C.byref(st))
    assert rc in (0, -5), rc
    return total.value, st.as_dict()


def fill_call(kind, out, cap):
    total, st = C.c_uint64(0), sufr_amd.RepeatStats()
    db.ctx.check(L.sufr_hip_repeats_device(db.ctx.handle, ix._h, lcp.data_ptr(), None, 0, kind, min_len, 2, 0, cap, out[0].data_ptr(),
                                           out[1].data_ptr(), out[2].data_ptr(), C.byref(total), C.byref(st)))
    return total.value, st.as_dict()


def report(name, ms, nbytes):
    cp = copy_ms(nbytes)
    med, cmed = statistics.median(ms), statistics.median(cp)
    print(f"{name:24s} {med:9.3f} ms (min {min(ms):.3f} max {max(ms):.3f})  model {nbytes / 1e9:7.3f} GB -> {nbytes / med / 1e6:7.1f} GB/s;"
          f"  copy of the same bytes {cmed:8.3f} ms (min {min(cp):.3f} max {max(cp):.3f})  ratio {med / cmed:5.2f}", flush=True)


# bytes by the model (one sequence: l is the LCP array, nothing is stored for it).  fold: SA and LCP read, one 64-byte line of
# the text per rank (the gather of T[SA[r] - 1]), two flag bits, two 8-byte prefixes per 64 ranks and level 1 written.
# search pass: l and the flag words and prefixes read; the counting call runs it once, the filling call twice and writes 24
# bytes per record
fold = 2 * s * w + 64 * s + s // 4 + s // 4 + s * w // 64
find = s * w + s // 2
results = {}
for kind, name in ((0, "branching"), (1, "maximal"), (2, "supermaximal")):
    (total, st), ms = timed(lambda: count_call(kind))
    report(f"{name}: count", ms, fold + find)
    out = [torch.empty(max(total, 1), dtype=torch.int64, device="cuda") for _ in range(3)]
    (total2, st2), ms = timed(lambda: fill_call(kind, out, total))
    assert total2 == total and st2 == st
    report(f"{name}: count + fill", ms, fold + 2 * find + 24 * total)
    results[kind] = (out, st)
    print(f"    {st}", flush=True)
_, ms = timed(lambda: ix.kmers_device(lcp, min_len, 256, None))
report(f"kmers spectrum k={min_len}", ms, 2 * s * w + s // 2)
if N <= 200_000_000 and not os.environ.get("REPEAT_BENCH_NO_HOST"):
    from test_gpu_match import _write
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "x.sufr")
        _write(path, norm.cpu().numpy(), sa.cpu().numpy().view(np.uint32).copy(), lcp.cpu().numpy().view(np.uint32).copy())
        f = sufr_amd.SufrFile(path)
        for kind, name in ((0, "branching"), (1, "maximal"), (2, "supermaximal")):
            t1 = time.time(); h = f.repeats(kind, min_len, threads=16); dt = time.time() - t1
            out, st = results[kind]
            same = all(np.array_equal(out[i].cpu().numpy().view(np.uint64), h[i]) for i in range(3)) and st == h[3]
            print(f"host, 16 threads: {name:14s} {dt * 1e3:9.1f} ms (count + fill)  equal to the device: {same}", flush=True)
            assert same
        f.close()
ix.close(); db.close()
