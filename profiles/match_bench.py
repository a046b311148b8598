"""Rate of the matching statistics and of the SMEMs on the device:   python profiles/match_bench.py [text_len] [reads] [min_len]
Builds the index of a synthetic genome (synth.syn_human) on the device, wraps it in place, simulates `reads` 150-bp reads
from the normalized text (1 % substitutions, 0.2 % N) and times, with HIP events on the context's stream:
  ms      sufr_hip_matching_stats_device alone (k_matching_stats),
  smems   sufr_hip_smems_device (k_matching_stats + flags + one synchronisation + records + slice search);
then, when the text is small enough to write (<= 200 Mb), the same batch through the host path of the written file on 16
threads (sufr_file_smems), and checks that both give the same records (MATCH_BENCH_NO_HOST=1 skips it).  The share of time per kernel comes from a
`rocprofv3 --kernel-trace --stats` run of this script."""
import ctypes as C
import os
import sys
import tempfile
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import sufr_amd
from sufr_amd import synth

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
nr = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
k = int(sys.argv[3]) if len(sys.argv) > 3 else 20
rl = 150
dev = "cuda"
t0 = time.time()
x, _ = synth.syn_human(n, seed=4, device=dev)
norm = torch.where((x >= 97) & (x <= 122), x - 32, x).contiguous()     # the text of a --dna build (soft-mask upper-cased)
del x
db = sufr_amd.DeviceBuilder(0)
sa, lcp = db.sort(norm, is_dna=True)
del lcp
ix = sufr_amd.DeviceIndex.wrap(db.ctx, norm, sa, is_dna=True)
print(f"text {n:,} suffixes {sa.numel():,}: index ready in {time.time() - t0:.1f} s", flush=True)
g = torch.Generator(device=dev); g.manual_seed(1)
at = torch.randint(0, n - rl - 1, (nr,), generator=g, device=dev)
qb = norm[(at[:, None] + torch.arange(rl, device=dev)[None, :]).reshape(-1)].contiguous()
sub = torch.rand(qb.numel(), generator=g, device=dev) < 0.01
qb[sub] = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[torch.randint(0, 4, (int(sub.sum()),), generator=g, device=dev)]
qb[torch.rand(qb.numel(), generator=g, device=dev) < 0.002] = ord("N")
off = (torch.arange(nr + 1, device=dev, dtype=torch.int64) * rl).contiguous()
nb = nr * rl
lib = sufr_amd.lib()
stream = torch.cuda.Stream()
lib.sufr_hip_set_stream(db.ctx.handle, stream.cuda_stream)
with torch.cuda.stream(stream):
    for rep in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        ms = ix.matching_statistics_device(qb, off, wait=False)
        e1.record(stream)
        stream.synchronize()
        t_ms = e0.elapsed_time(e1)
        print(f"ms:    {nr:,} reads x {rl} = {nb:,} offsets: {t_ms:.2f} ms  {nb / t_ms / 1e6:.3f} G offsets/s  "
              f"mean ms {ms.float().mean().item():.1f}", flush=True)
    for rep in range(3):
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        qi, qo, ln, lo, hi = ix.smems_device(qb, off, k)
        t_sm = (time.perf_counter() - w0) * 1e3
        nsm = qi.numel()
        print(f"smems: k={k}: {nsm:,} SMEMs ({nsm / nr:.2f} per read, mean length {ln.float().mean().item():.1f}, mean count "
              f"{(hi - lo).float().mean().item():.1f}): {t_sm:.2f} ms  {nb / t_sm / 1e6:.3f} G offsets/s  {nsm / t_sm / 1e3:.1f} M SMEMs/s",
              flush=True)
if n <= 200_000_000 and not os.environ.get("MATCH_BENCH_NO_HOST"):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "x.sufr")
        text_h = norm.cpu().numpy(); sa_h = sa.cpu().numpy().view(np.uint32); lcp_h = np.zeros_like(sa_h)
        starts = np.zeros(1, dtype=np.uint64); names = (C.c_char_p * 1)(b"1"); err = C.create_string_buffer(256)
        assert lib.sufr_write_file(path.encode(), 1, 0, 0, text_h.ctypes.data, n, 4, sa_h.ctypes.data, lcp_h.ctypes.data, sa_h.size,
                                   0, 0, None, starts.ctypes.data, 1, names, err, len(err)) == 0
        f = sufr_amd.SufrFile(path)
        qh = qb.cpu().numpy(); oh = off.cpu().numpy().astype(np.uint64)
        w0 = time.perf_counter()
        want = f.smem_arrays(qh, oh, k, threads=16)
        t_h = (time.perf_counter() - w0) * 1e3
        same = all(np.array_equal(a.cpu().numpy().astype(np.int64), b.astype(np.int64)) for a, b in zip((qi, qo, ln, lo, hi), want))
        print(f"host (16 threads): {t_h:.0f} ms  {nb / t_h / 1e6:.4f} G offsets/s; device smems is {t_h / t_sm:.1f}x the host; "
              f"records equal: {same}", flush=True)
        assert same
ix.close(); db.close()
