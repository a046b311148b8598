"""Rate of the MEMs of a read batch on the device:   python profiles/mem_bench.py [text_len] [reads] [min_len]
Builds the index of a synthetic genome (synth.syn_human) on the device, wraps it in place, simulates `reads` 150-bp reads
from the normalized text (1 % substitutions, 0.2 % N, every second read reverse-complemented) and times
sufr_hip_mems_device on both strands with max_occ 0 and 500 (wall clock around the call, which returns complete records).
Above 200 Mb the max_occ 0 records do not fit in device memory (syn_human's repeat families give thousands of MEMs per
read): that leg is timed as a call with cap 0, which counts the MEMs and stops before the records.
Then, when the text is small enough to write (<= 200 Mb), the same batch through the host path of the written file on 16
threads (sufr_file_mems), and checks that both give the same records (MEM_BENCH_NO_HOST=1 skips it).  The share of time
per kernel comes from a `rocprofv3 --kernel-trace --stats` run of this script."""
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
reps = int(os.environ.get("MEM_BENCH_REPS", "3"))
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
comp = torch.arange(256, dtype=torch.uint8, device=dev)
for a, b in (b"AT", b"TA", b"CG", b"GC"):
    comp[a] = b
r2 = qb.view(nr, rl)
r2[::2] = comp[r2[::2].flip(1).long()]                                 # half of the reads come from the other strand
off = (torch.arange(nr + 1, device=dev, dtype=torch.int64) * rl).contiguous()
offsets = 2 * nr * rl
results = {}
for occ in (0, 500):
    count_only = occ == 0 and n > 200_000_000
    for rep in range(reps):
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        if count_only:
            try:
                ix.mems_device(qb, off, k, occ, True, cap=0)
                nm = 0
            except sufr_amd.SufrHipError as e:
                assert e.code == -5
                nm = e.total
            t_m = (time.perf_counter() - w0) * 1e3
            print(f"mems: k={k} max_occ={occ} both strands, counted only: {offsets:,} offsets, {nm:,} MEMs ({nm / nr:.2f} per read): "
                  f"{t_m:.2f} ms  {offsets / t_m / 1e6:.3f} G offsets/s", flush=True)
            continue
        recs = ix.mems_device(qb, off, k, occ, True)
        t_m = (time.perf_counter() - w0) * 1e3
        nm = recs[0].numel()
        print(f"mems: k={k} max_occ={occ} both strands: {offsets:,} offsets, {nm:,} MEMs ({nm / nr:.2f} per read, mean length "
              f"{recs[3].float().mean().item():.1f}): {t_m:.2f} ms  {offsets / t_m / 1e6:.3f} G offsets/s", flush=True)
        results[occ] = (recs, t_m)
lib = sufr_amd.lib()
if n <= 200_000_000 and not os.environ.get("MEM_BENCH_NO_HOST"):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "x.sufr")
        text_h = norm.cpu().numpy(); sa_h = sa.cpu().numpy().view(np.uint32); lcp_h = np.zeros_like(sa_h)
        starts = np.zeros(1, dtype=np.uint64); names = (C.c_char_p * 1)(b"1"); err = C.create_string_buffer(256)
        assert lib.sufr_write_file(path.encode(), 1, 0, 0, text_h.ctypes.data, n, 4, sa_h.ctypes.data, lcp_h.ctypes.data, sa_h.size,
                                   0, 0, None, starts.ctypes.data, 1, names, err, len(err)) == 0
        f = sufr_amd.SufrFile(path)
        qh = qb.cpu().numpy(); oh = off.cpu().numpy().astype(np.uint64)
        for occ in (0, 500):
            w0 = time.perf_counter()
            want = f.mem_arrays(qh, oh, k, occ, True, threads=16)
            t_h = (time.perf_counter() - w0) * 1e3
            got, t_m = results[occ]
            same = all(np.array_equal(a.cpu().numpy().astype(np.int64), b.astype(np.int64)) for a, b in zip(got, want))
            print(f"host (16 threads) max_occ={occ}: {t_h:.0f} ms  {offsets / t_h / 1e6:.4f} G offsets/s; device is {t_h / t_m:.1f}x "
                  f"the host; records equal: {same}", flush=True)
            assert same
ix.close(); db.close()
