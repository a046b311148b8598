"""Rate of the alignment traceback beside the search that feeds it:   python profiles/align_bench.py [text_len] [reads] [d,d,...]
Builds the index of a synthetic genome (synth.syn_human) on the device, wraps it in place and simulates the indel batch of
profiles/edit_bench.py: `reads` 150-bp reads with 1 % substitutions, 0.2 % N and 0.2 % indels, every second read
reverse-complemented.  For every d, with max_occ 500, both strands and SUFR_EDIT_LOCAL_MINIMA, after warm-up calls that give the
totals:
  - edit_device, ALIGN_BENCH_REPS times: wall clock around one call with that capacity, complete records;
  - edit_trace_device on those records, as often: wall clock around one call with the capacity of its runs; records/s, the bytes
    of row storage the call used (8 per query byte and record of a chunk) and the ratio to the search;
  - when the text is small enough to write (<= 200 Mb; ALIGN_BENCH_NO_HOST=1 skips it): sufr_file_edit_trace on 16 threads on
    the same records, checked to give the same starts, offsets and runs.
The share of time per kernel comes from a `rocprofv3 --kernel-trace --stats` run of this script (never together with --pmc)."""
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
ds = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [1, 3, 5]
reps = int(os.environ.get("ALIGN_BENCH_REPS", "3"))
occ, rl, dev = 500, 150, "cuda"
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
at = torch.randint(0, n - rl - 9, (nr,), generator=g, device=dev)
acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
comp = torch.arange(256, dtype=torch.uint8, device=dev)
for a, b in (b"AT", b"TA", b"CG", b"GC"):
    comp[a] = b
span = rl + 8
src = norm[(at[:, None] + torch.arange(span, device=dev)[None, :]).reshape(-1)].view(nr, span)
ev = torch.rand(nr, rl, generator=g, device=dev)
dele, ins = ev < 0.001, (ev >= 0.001) & (ev < 0.002)
col = (torch.arange(rl, device=dev)[None, :] + torch.cumsum(dele.long() - ins.long(), dim=1)).clamp_(0, span - 1)
r = torch.gather(src, 1, col)
r[ins] = acgt[torch.randint(0, 4, (int(ins.sum()),), generator=g, device=dev)]
qb = r.reshape(-1).contiguous()
sub = torch.rand(qb.numel(), generator=g, device=dev) < 0.01
qb[sub] = acgt[torch.randint(0, 4, (int(sub.sum()),), generator=g, device=dev)]
qb[torch.rand(qb.numel(), generator=g, device=dev) < 0.002] = ord("N")
r2 = qb.view(nr, rl)
r2[::2] = comp[r2[::2].flip(1).long()]                                 # half of the reads come from the other strand
off = (torch.arange(nr + 1, device=dev, dtype=torch.int64) * rl).contiguous()
budget = 256 << 20                                                     # the default row storage (sufr_trace.inc)
results = {}
for d in ds:
    total = ix.edit_device(qb, off, d, occ, True, True)[0].numel()
    t_e = []
    for rep in range(reps):
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        recs = ix.edit_device(qb, off, d, occ, True, True, cap=total)
        t_e.append((time.perf_counter() - w0) * 1e3)
    recs = [t.contiguous() for t in recs]
    runs = ix.edit_trace_device(qb, off, *recs)[2].numel()
    t_t = []
    for rep in range(reps):
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        tr = ix.edit_trace_device(qb, off, *recs, cap=runs)
        t_t.append((time.perf_counter() - w0) * 1e3)
    chunk = min(budget // (8 * rl) // 64 * 64, 1 << 20, -(-total // 64) * 64)
    print(f"align: d={d} max_occ={occ} both strands, minima: {total:,} records ({total / nr:.3f} per read), {runs:,} runs "
          f"({runs / max(total, 1):.2f} per record); edit_device: " + " ".join(f"{t:.2f}" for t in t_e) + " ms; edit_trace_device: "
          + " ".join(f"{t:.2f}" for t in t_t) + f" ms  {total / min(t_t) / 1e3:.3f} M records/s; rows: {chunk * 8 * rl:,} bytes a chunk of "
          f"{chunk:,} records, {total * 8 * rl:,} bytes over the call; trace / edit {min(t_t) / min(t_e):.3f}", flush=True)
    results[d] = (recs, tr, min(t_t))
if n <= 200_000_000 and not os.environ.get("ALIGN_BENCH_NO_HOST"):
    lib = sufr_amd.lib()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "x.sufr")
        text_h = norm.cpu().numpy(); sa_h = sa.cpu().numpy().view(np.uint32); lcp_h = np.zeros_like(sa_h)
        starts = np.zeros(1, dtype=np.uint64); names = (C.c_char_p * 1)(b"1"); err = C.create_string_buffer(256)
        assert lib.sufr_write_file(path.encode(), 1, 0, 0, text_h.ctypes.data, n, 4, sa_h.ctypes.data, lcp_h.ctypes.data, sa_h.size,
                                   0, 0, None, starts.ctypes.data, 1, names, err, len(err)) == 0
        f = sufr_amd.SufrFile(path)
        qh = qb.cpu().numpy(); oh = off.cpu().numpy().astype(np.uint64)
        for d, (recs, tr, t_m) in results.items():
            rh = [t.cpu().numpy().astype(dt) for t, dt in zip(recs, (np.uint64, np.uint8, np.uint64, np.uint8))]
            w0 = time.perf_counter()
            want = f.edit_trace_arrays(qh, oh, *rh, cap=tr[2].numel(), threads=16)
            t_h = (time.perf_counter() - w0) * 1e3
            same = all(np.array_equal(a.cpu().numpy().astype(np.int64), b.astype(np.int64)) for a, b in zip(tr, want))
            print(f"host trace (16 threads) d={d}: {t_h:.0f} ms  {len(rh[0]) / t_h / 1e3:.4f} M records/s; device is {t_h / t_m:.1f}x the host; "
                  f"outputs equal: {same}", flush=True)
            assert same
ix.close(); db.close()
