"""Time of the BWT gather, the run report and the LF mapping over a device-resident text and SA:
    python profiles/bwt_bench.py [text_len] [--allow-ambiguity]
Builds the index of a synthetic genome (synth.syn_human, --dna --ignore-softmask; with --allow-ambiguity every position is
indexed, s == n) on the device, wraps it in place and times, per call, with HIP events around the call on the context's stream
(BWT_BENCH_WARMUP warm-up calls, BWT_BENCH_REPS timed ones: median, min and max):
  bwt (the gather with the counts), bwt_runs counting and counting + filling (min_len 1: every run is written), lf.
The yardstick is existing code with the same access shape, from the same session: unique_lengths_device(by_position=True), one
random 4-byte access per rank through SA.  Beside every call: ranks per second, the bytes it moves per rank by the model of
DESIGN.md section 22 (a random access counted as the 128-byte line it fetches) and its time against the yardstick's.  Then,
when the text is small enough to write (<= 200 Mb), the host paths of the written file on 16 threads, checked against the
device results (BWT_BENCH_NO_HOST=1 skips it)."""
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

args = [a for a in sys.argv[1:] if not a.startswith("--")]
ambiguity = "--allow-ambiguity" in sys.argv
n = int(float(args[0])) if args else 100_000_000
reps = int(os.environ.get("BWT_BENCH_REPS", "7"))
warm = int(os.environ.get("BWT_BENCH_WARMUP", "2"))
t0 = time.time()
x, _ = synth.syn_human(n, seed=4, device="cuda")
norm = torch.where((x >= 97) & (x <= 122), x - 32, x).contiguous()
del x
db = sufr_amd.DeviceBuilder(0)
sa, lcp = db.sort(norm, is_dna=True, allow_ambiguity=ambiguity)
ix = sufr_amd.DeviceIndex.wrap(db.ctx, norm, sa, is_dna=True, prefix_table=False)
s, N, w = sa.numel(), norm.numel(), 4
print(f"text {N:,} suffixes {s:,}{' (--allow-ambiguity)' if ambiguity else ''}: index ready in {time.time() - t0:.1f} s; "
      f"{warm} warm-up + {reps} timed calls each", flush=True)
stream = torch.cuda.Stream()                                       # the context's launches are timed on a stream of their own
L = sufr_amd.lib()
L.sufr_hip_set_stream(db.ctx.handle, stream.cuda_stream)
h = (db.ctx.handle, ix._h)


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


def report(name, ms, per_rank, yard=None):
    med = statistics.median(ms)
    print(f"{name:24s} {med:9.3f} ms (min {min(ms):.3f} max {max(ms):.3f})  {s / med / 1e6:7.2f} G ranks/s;  model {per_rank:6.1f} B/rank -> "
          f"{per_rank * s / med / 1e6:7.1f} GB/s" + (f";  {med / yard:5.2f} x the yardstick" if yard else ""), flush=True)
    return med


# the yardstick: SA and LCP read in order (2 w), one scattered 4-byte store per rank (a 128-byte line), the fill of the output
d_ul = torch.empty(N, dtype=torch.int32, device="cuda")
_, ms = timed(lambda: db.ctx.check(L.sufr_hip_unique_lengths_device(*h, lcp.data_ptr(), None, 0, sufr_amd._lib.KMER_BY_POSITION, d_ul.data_ptr())))
yard = report("unique_lengths by pos.", ms, 2 * w + 128 + w * N / s)
del d_ul

d_bwt = torch.empty(s + 8, dtype=torch.uint8, device="cuda")
d_counts = torch.empty(256, dtype=torch.int64, device="cuda")
d_lf = torch.empty(s, dtype=torch.int32, device="cuda")


def runs_call(cap, out):
    total, st = C.c_uint64(0), sufr_amd.BwtStats()
    rc = L.sufr_hip_bwt_runs_device(*h, 1, cap, *(o.data_ptr() if o is not None else None for o in out), C.byref(total), C.byref(st))
    assert rc == 0 or (rc == -5 and cap == 0), rc
    return total.value, st.as_dict()


# bytes per rank by the model of section 22.  The gather reads SA in order (w) and one text byte at random (a 128-byte line) and
# writes one byte; the run passes read that byte back (1 each) and the writing pass stores 32 bytes and fetches a line of SA per
# run; LF adds the histogram pass (1) and the ranking pass (1 read, w written).
_, ms = timed(lambda: db.ctx.check(L.sufr_hip_bwt_device(*h, d_bwt.data_ptr(), d_counts.data_ptr())))
report("bwt", ms, w + 128 + 1, yard)
(r, st), ms = timed(lambda: runs_call(0, (None,) * 4))
report("bwt_runs: count", ms, w + 128 + 1 + 1, yard)
out = [torch.empty(max(r, 1), dtype=torch.int64, device="cuda") for _ in range(4)]
(r2, st2), ms = timed(lambda: runs_call(r, out))
assert r2 == r and st2 == st
report("bwt_runs: count + fill", ms, w + 128 + 1 + 2 + (32 + 128) * r / s, yard)
print(f"    {st}  (n / r = {N / max(r, 1):.2f})", flush=True)
_, ms = timed(lambda: db.ctx.check(L.sufr_hip_lf_device(*h, d_lf.data_ptr())))
report("lf", ms, w + 128 + 1 + 2 + w, yard)
torch.cuda.synchronize()
occurring = int((d_counts > 0).sum().item())
print(f"    {occurring} byte values occur: {(s + 16383) // 16384:,} tiles of 16384 ranks x {occurring} bases of 8 bytes", flush=True)
if N <= 200_000_000 and not os.environ.get("BWT_BENCH_NO_HOST"):
    from test_gpu_match import _write
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "x.sufr")
        _write(path, norm.cpu().numpy(), sa.cpu().numpy().view(np.uint32).copy(), lcp.cpu().numpy().view(np.uint32).copy())
        f = sufr_amd.SufrFile(path)
        t1 = time.time(); hb, hc = f.bwt(threads=16); t_bwt = time.time() - t1
        t1 = time.time(); hr = f.bwt_runs(1, threads=16); t_runs = time.time() - t1
        t1 = time.time(); hl = f.lf(threads=16); t_lf = time.time() - t1
        same = (np.array_equal(d_bwt[:s].cpu().numpy(), hb) and np.array_equal(d_counts.cpu().numpy().view(np.uint64), hc) and
                all(np.array_equal(out[i].cpu().numpy().view(np.uint64), hr[i]) for i in range(4)) and st == hr[4] and
                np.array_equal(d_lf.cpu().numpy().view(np.uint32), hl))
        print(f"host, 16 threads: bwt {t_bwt * 1e3:8.1f} ms ({s / t_bwt / 1e9:.3f} G ranks/s)  bwt_runs (count + fill) {t_runs * 1e3:8.1f} ms "
              f"({s / t_runs / 1e9:.3f} G ranks/s)  lf {t_lf * 1e3:8.1f} ms ({s / t_lf / 1e9:.3f} G ranks/s)  equal to the device: {same}", flush=True)
        assert same
        f.close()
ix.close(); db.close()
