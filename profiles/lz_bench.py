"""Time of the LPF pass and of the LZ77 parse over a device-resident SA and LCP:   python profiles/lz_bench.py [text_len]
Builds the index of a synthetic genome (synth.syn_human) on the device, wraps it in place, hands the builder's LCP straight to
sufr_hip_lpf_device / sufr_hip_lz_device and times, per call, with HIP events around the call on the context's stream
(LZ_BENCH_WARMUP warm-up calls, LZ_BENCH_REPS timed ones: median, min and max):
  the LPF call (fills, pyramids, the search pass with its scatter), the counting LZ call (the same into scratch, table, chain,
  the counting emit pass, one synchronisation) and the filling LZ call (the same and the writing emit pass).
Beside every call: the bytes it moves by the model of DESIGN.md section 20 and the time of a plain device-to-device copy of
that many bytes in the same run -- the copy, not the code under test, is the yardstick.  The chain kernel's own time comes
from the probes build (make -C sufr_amd/csrc probes; SUFR_AMD_PROBES_LIB=1), which stamps it with two events and prints it
to standard error: it is collected here and shown with its share of the counting call.  Then, when the text is small enough
to write (<= 200 Mb), the host path of the written file on 16 threads, checked against the device results
(LZ_BENCH_NO_HOST=1 skips it)."""
import ctypes as C
import os
import re
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
reps = int(os.environ.get("LZ_BENCH_REPS", "7"))
warm = int(os.environ.get("LZ_BENCH_WARMUP", "2"))
t0 = time.time()
x, _ = synth.syn_human(n, seed=4, device="cuda")
norm = torch.where((x >= 97) & (x <= 122), x - 32, x).contiguous()
del x
db = sufr_amd.DeviceBuilder(0)
sa, lcp = db.sort(norm, is_dna=True)
ix = sufr_amd.DeviceIndex.wrap(db.ctx, norm, sa, is_dna=True, prefix_table=False)
s, N, w = sa.numel(), norm.numel(), 4
print(f"text {N:,} suffixes {s:,}: index ready in {time.time() - t0:.1f} s; {warm} warm-up + {reps} timed calls each", flush=True)
stream = torch.cuda.Stream()                                       # the context's launches are timed on a stream of their own
L = sufr_amd.lib()
L.sufr_hip_set_stream(db.ctx.handle, stream.cuda_stream)


class Stderr:
    """what the library writes to standard error while the block runs (the probes build's stamps)"""
    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


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
    """a device-to-device copy that reads and writes nbytes in all (nbytes / 2 each way), in pieces of at most 4 GB"""
    half = max(nbytes // 2, 1)
    piece = min(half, 1 << 32)
    src = torch.empty(piece, dtype=torch.uint8, device="cuda")
    dst = torch.empty(piece, dtype=torch.uint8, device="cuda")
    def copy():
        with torch.cuda.stream(stream):
            left = half
            while left > 0:
                k = min(left, piece)
                dst[:k].copy_(src[:k])
                left -= k
    ms = timed(copy)[1]
    del src, dst
    torch.cuda.empty_cache()
    return ms


def report(name, ms, nbytes):
    cp = copy_ms(nbytes)
    med, cmed = statistics.median(ms), statistics.median(cp)
    print(f"{name:24s} {med:9.3f} ms (min {min(ms):.3f} max {max(ms):.3f})  model {nbytes / 1e9:7.3f} GB -> {nbytes / med / 1e6:7.1f} GB/s;"
          f"  copy of the same bytes {cmed:8.3f} ms (min {min(cp):.3f} max {max(cp):.3f})  ratio {med / cmed:5.2f}", flush=True)
    return med


d_lpf = torch.empty(N, dtype=torch.int32, device="cuda")
d_src = torch.empty(N, dtype=torch.int32, device="cuda")


def lpf_call():
    db.ctx.check(L.sufr_hip_lpf_device(db.ctx.handle, ix._h, lcp.data_ptr(), None, 0, d_lpf.data_ptr(), d_src.data_ptr()))


def count_call():
    total, st = C.c_uint64(0), sufr_amd.LzStats()
    rc = L.sufr_hip_lz_device(db.ctx.handle, ix._h, lcp.data_ptr(), None, 0, 0, None, None, None, C.byref(total), C.byref(st))
    assert rc in (0, -5), rc
    return total.value, st.as_dict()


def fill_call(out, cap):
    total, st = C.c_uint64(0), sufr_amd.LzStats()
    db.ctx.check(L.sufr_hip_lz_device(db.ctx.handle, ix._h, lcp.data_ptr(), None, 0, cap, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                      C.byref(total), C.byref(st)))
    return total.value, st.as_dict()


# bytes by the model of section 20 (one sequence).  LPF call: two fills written, SA and LCP read by the fold and again by the
# search pass, LPF and SRC scattered -- one 64-byte line per rank and array where the line is not reused.  Parse: the table
# pass reads LPF and writes 4 bytes per position, an emit pass reads LPF again and LPF + SRC of every factor; the writing one
# adds 24 bytes per factor.
lpf_bytes = 2 * N * w + 4 * s * w + 2 * 64 * s
with Stderr() as err:
    _, ms = timed(lpf_call)
report("lpf", ms, lpf_bytes)
with Stderr() as err:
    (z, st), ms = timed(count_call)
chain = [float(v) for v in re.findall(r"lz: chain kernel ([0-9.]+) ms", err.text)][warm:]
count_med = report("lz: count", ms, lpf_bytes + N * w + 4 * N + N * w + 2 * w * z)
out = [torch.empty(max(z, 1), dtype=torch.int64, device="cuda") for _ in range(3)]
with Stderr() as err2:
    (z2, st2), ms = timed(lambda: fill_call(out, z))
assert z2 == z and st2 == st
report("lz: count + fill", ms, lpf_bytes + N * w + 4 * N + 2 * (N * w + 2 * w * z) + 24 * z)
print(f"    {st}  (n / z = {N / max(z, 1):.2f})", flush=True)
if chain:
    cmed = statistics.median(chain)
    print(f"chain kernel alone      {cmed:9.3f} ms (min {min(chain):.3f} max {max(chain):.3f}), {cmed / count_med * 100:5.1f} % of the counting call;"
          f" {(N + 16383) // 16384:,} tiles of 16384 positions -> {cmed * 1e3 / ((N + 16383) // 16384):.3f} us per tile", flush=True)
else:
    print("chain kernel alone      not stamped: this is not the probes build (make -C sufr_amd/csrc probes; SUFR_AMD_PROBES_LIB=1)", flush=True)
if N <= 200_000_000 and not os.environ.get("LZ_BENCH_NO_HOST"):
    from test_gpu_match import _write
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "x.sufr")
        _write(path, norm.cpu().numpy(), sa.cpu().numpy().view(np.uint32).copy(), lcp.cpu().numpy().view(np.uint32).copy())
        f = sufr_amd.SufrFile(path)
        t1 = time.time(); h = f.lz(threads=16); dt = time.time() - t1
        same = all(np.array_equal(out[i].cpu().numpy().view(np.uint64), h[i]) for i in range(3)) and st == h[3]
        print(f"host, 16 threads: lz {dt * 1e3:9.1f} ms (count + fill)  equal to the device: {same}", flush=True)
        assert same
        f.close()
ix.close(); db.close()
