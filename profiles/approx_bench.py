"""Rate of the k-mismatch search of a read batch on the device:   python profiles/approx_bench.py [text_len] [reads] [d,d,...]
Builds the index of a synthetic genome (synth.syn_human) on the device, wraps it in place and simulates `reads` 150-bp
reads as profiles/mem_bench.py does (1 % substitutions, 0.2 % N, every second read reverse-complemented).  For every d and
max_occ 0 and 500, both strands:
  - the pieces of the doubled batch as plain queries through search_device (k_search_batch: the same search_range call as
    k_approx_seeds, on the same bytes), APPROX_BENCH_REPS times: the seeds, the candidates (sum of the live range sizes) and
    the run-to-run spread of the search;
  - approx_device, APPROX_BENCH_REPS times after a warm-up call that gives the record total: wall clock around one call with
    that capacity, which returns complete records;
Then one mems_device call (k = 20, max_occ 500) so that a kernel trace of this run holds k_mem_count next to the verify
passes, and, when the text is small enough to write (<= 200 Mb), the same batch through the host path of the written file on
16 threads (sufr_file_approx), checking that both give the same records (APPROX_BENCH_NO_HOST=1 skips it).  The share of time
per kernel comes from a `rocprofv3 --kernel-trace --stats` run of this script (never together with --pmc)."""
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
ds = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [1, 2, 3, 5]
reps = int(os.environ.get("APPROX_BENCH_REPS", "3"))
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
# the doubled batch (read, then its reverse complement): its pieces are plain queries over the same bytes
dbl = torch.stack([r2, comp[r2.flip(1).long()]], dim=1).reshape(-1).contiguous()
results = {}
for d in ds:
    o = torch.tensor([i * rl // (d + 1) for i in range(d + 1)], device=dev, dtype=torch.int64)
    poff = (torch.arange(2 * nr, device=dev, dtype=torch.int64)[:, None] * rl + o[None, :]).reshape(-1)
    poff = torch.cat([poff, torch.tensor([2 * nr * rl], device=dev, dtype=torch.int64)]).contiguous()
    seeds = poff.numel() - 1
    t_s = []
    ix.search_device(dbl, poff)                                        # (warm-up: not timed)
    for rep in range(reps):
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        lo, hi = ix.search_device(dbl, poff)
        t_s.append((time.perf_counter() - w0) * 1e3)
    size = hi - lo
    print(f"pieces: d={d} {seeds:,} seeds of {rl // (d + 1)}+ bytes through search_device: " + " ".join(f"{t:.2f}" for t in t_s) +
          f" ms (wall; spread {(max(t_s) - min(t_s)) / min(t_s) * 100:.2f} %)  {min(t_s) / seeds * 1e6:.3f} ns per seed", flush=True)
    for occ in (0, 500):
        cand = int((size if occ == 0 else torch.where(size <= occ, size, torch.zeros_like(size))).sum())
        total = ix.approx_device(qb, off, d, occ, True)[0].numel()     # (warm-up: the record total, so that a timed call runs once)
        for rep in range(reps):
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            recs = ix.approx_device(qb, off, d, occ, True, cap=total)
            t_m = (time.perf_counter() - w0) * 1e3
            nrec = recs[0].numel()
            print(f"approx: d={d} max_occ={occ} both strands: {seeds:,} seeds, {cand:,} candidates, {nrec:,} records "
                  f"({nrec / nr:.3f} per read, {cand / max(nrec, 1):.2f} candidates per record): {t_m:.2f} ms  "
                  f"{nr / t_m / 1e3:.3f} M reads/s", flush=True)
        results[(d, occ)] = (recs, t_m)
    del lo, hi, size, poff
torch.cuda.synchronize()
w0 = time.perf_counter()
m = ix.mems_device(qb, off, 20, 500, True)
print(f"mems: k=20 max_occ=500 both strands (for k_mem_count in the kernel trace): {m[0].numel():,} MEMs: "
      f"{(time.perf_counter() - w0) * 1e3:.2f} ms", flush=True)
del m
lib = sufr_amd.lib()
if n <= 200_000_000 and not os.environ.get("APPROX_BENCH_NO_HOST"):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "x.sufr")
        text_h = norm.cpu().numpy(); sa_h = sa.cpu().numpy().view(np.uint32); lcp_h = np.zeros_like(sa_h)
        starts = np.zeros(1, dtype=np.uint64); names = (C.c_char_p * 1)(b"1"); err = C.create_string_buffer(256)
        assert lib.sufr_write_file(path.encode(), 1, 0, 0, text_h.ctypes.data, n, 4, sa_h.ctypes.data, lcp_h.ctypes.data, sa_h.size,
                                   0, 0, None, starts.ctypes.data, 1, names, err, len(err)) == 0
        f = sufr_amd.SufrFile(path)
        qh = qb.cpu().numpy(); oh = off.cpu().numpy().astype(np.uint64)
        for (d, occ), (got, t_m) in results.items():
            w0 = time.perf_counter()
            want = f.approx_arrays(qh, oh, d, occ, True, threads=16)
            t_h = (time.perf_counter() - w0) * 1e3
            same = all(np.array_equal(a.cpu().numpy().astype(np.int64), b.astype(np.int64)) for a, b in zip(got, want))
            print(f"host (16 threads) d={d} max_occ={occ}: {t_h:.0f} ms  {nr / t_h / 1e3:.4f} M reads/s; device is {t_h / t_m:.1f}x "
                  f"the host; records equal: {same}", flush=True)
            assert same
ix.close(); db.close()
