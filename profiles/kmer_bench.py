"""Time of the k-mer passes over a device-resident SA and LCP:   python profiles/kmer_bench.py [text_len] [k]
Builds the index of a synthetic genome (synth.syn_human) on the device, wraps it in place, hands the builder's LCP straight to
sufr_hip_kmers_device / sufr_hip_unique_lengths_device and times, per call, with HIP events around the call on the context's
stream (KMER_BENCH_WARMUP warm-up calls, KMER_BENCH_REPS timed ones: median, min and max):
  the spectrum alone, occ by rank, occ by position, unique lengths by rank and by position.
Beside every call: the bytes it moves by the model of DESIGN.md section 18 and the time of a plain device-to-device copy of
that many bytes in the same run -- the copy, not the code under test, is the yardstick.  Then, when the text is small enough to
write (<= 200 Mb), the host path of the written file on 16 threads, checked against the device results
(KMER_BENCH_NO_HOST=1 skips it)."""
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
k = int(sys.argv[2]) if len(sys.argv) > 2 else 21
reps = int(os.environ.get("KMER_BENCH_REPS", "7"))
warm = int(os.environ.get("KMER_BENCH_WARMUP", "2"))
t0 = time.time()
x, _ = synth.syn_human(n, seed=4, device="cuda")
norm = torch.where((x >= 97) & (x <= 122), x - 32, x).contiguous()
del x
db = sufr_amd.DeviceBuilder(0)
sa, lcp = db.sort(norm, is_dna=True)
ix = sufr_amd.DeviceIndex.wrap(db.ctx, norm, sa, is_dna=True, prefix_table=False)
s, N, w = sa.numel(), norm.numel(), 4
print(f"text {N:,} suffixes {s:,} k {k}: index ready in {time.time() - t0:.1f} s; {warm} warm-up + {reps} timed calls each", flush=True)
stream = torch.cuda.Stream()                                       # the context's launches are timed on a stream of their own
sufr_amd.lib().sufr_hip_set_stream(db.ctx.handle, stream.cuda_stream)


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


# bytes by the model: fold reads SA + LCP and writes two bits per rank; apply reads the bits and writes occ; by position
# adds the memset of n entries, the SA again and one 64-byte line per stored entry instead of w bytes
fold = 2 * s * w + s // 4
legs = [("spectrum", lambda: ix.kmers_device(lcp, k, 256, None), fold + s // 4),
        ("occ by rank", lambda: ix.kmers_device(lcp, k, 256, "rank"), fold + s // 4 + s * w),
        ("occ by position", lambda: ix.kmers_device(lcp, k, 256, "position"), fold + s // 4 + s * w + N * w + s * 64),
        ("unique by rank", lambda: ix.unique_lengths_device(lcp, False), 3 * s * w),
        ("unique by position", lambda: ix.unique_lengths_device(lcp, True), 2 * s * w + N * w + s * 64)]
results = {}
for name, call, nbytes in legs:
    out, ms = timed(call)
    cp = copy_ms(nbytes)
    results[name] = out
    med, cmed = statistics.median(ms), statistics.median(cp)
    print(f"{name:20s} {med:9.3f} ms (min {min(ms):.3f} max {max(ms):.3f})  model {nbytes / 1e9:7.3f} GB -> {nbytes / med / 1e6:7.1f} GB/s;"
          f"  copy of the same bytes {cmed:8.3f} ms (min {min(cp):.3f} max {max(cp):.3f})  ratio {med / cmed:5.2f}", flush=True)
st = results["spectrum"][1]
print(f"stats {st}")
if N <= 200_000_000 and not os.environ.get("KMER_BENCH_NO_HOST"):
    from test_gpu_match import _write
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "x.sufr")
        _write(path, norm.cpu().numpy(), sa.cpu().numpy().view(np.uint32).copy(), lcp.cpu().numpy().view(np.uint32).copy())
        f = sufr_amd.SufrFile(path)
        for name, call in (("spectrum", lambda: f.kmers(k, 256, None, threads=16)), ("occ by rank", lambda: f.kmers(k, 256, "rank", threads=16)),
                           ("occ by position", lambda: f.kmers(k, 256, "position", threads=16)),
                           ("unique by rank", lambda: f.unique_lengths(False, threads=16)), ("unique by position", lambda: f.unique_lengths(True, threads=16))):
            t = []
            for _ in range(3):
                t1 = time.time(); h = call(); t.append(time.time() - t1)
            dev_out = results[name]
            if name.startswith("unique"):
                same = np.array_equal(dev_out.cpu().numpy().view(np.uint32), h)
            else:
                same = np.array_equal(dev_out[0].cpu().numpy().view(np.uint64), h[0]) and dev_out[1] == h[1] and \
                    (h[2] is None or np.array_equal(dev_out[2].cpu().numpy().view(np.uint32), h[2]))
            print(f"host, 16 threads: {name:20s} {statistics.median(t) * 1e3:9.1f} ms (min {min(t) * 1e3:.1f} max {max(t) * 1e3:.1f})  equal to the device: {same}", flush=True)
            assert same
        f.close()
ix.close(); db.close()
