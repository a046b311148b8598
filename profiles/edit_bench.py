"""Rate of the k-difference search of a read batch on the device:   python profiles/edit_bench.py [text_len] [reads] [d,d,...]
Builds the index of a synthetic genome (synth.syn_human) on the device, wraps it in place and simulates two batches of
`reads` 150-bp reads: profiles/approx_bench.py's (1 % substitutions, 0.2 % N, every second read reverse-complemented) and
the same with 0.2 % indels on top (per base: half insertions, half deletions, the read cut or padded from the text back to
150 bp).  For every batch, every d and max_occ 0 and 500, both strands, after a warm-up call that gives the record total:
  - edit_device, EDIT_BENCH_REPS times: wall clock around one call with that capacity, which returns complete records;
  - approx_device at the same d on the same batch: what the band and the sort add;
  - one call through a second context made under SUFR_HIP_DEBUG=1, which prints seeds, candidates, reported ends and
    records on stderr.
A configuration whose scratch does not fit the device fails with an error that is printed, and the run goes on.  When the
text is small enough to write (<= 200 Mb), the indel batch also goes through the host path of the written file on 16
threads (sufr_file_edit; max_occ 0 only up to d = EDIT_BENCH_HOST_OCC0_D, 1 by default: the host walks every candidate's band
in full), checking that both give the same records (EDIT_BENCH_NO_HOST=1 skips it; EDIT_BENCH_OCCS picks the max_occ values).  The share of time per
kernel comes from a `rocprofv3 --kernel-trace --stats` run of this script (never together with --pmc)."""
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
reps = int(os.environ.get("EDIT_BENCH_REPS", "3"))
occs = [int(v) for v in os.environ.get("EDIT_BENCH_OCCS", "0,500").split(",")]
host_occ0_d = int(os.environ.get("EDIT_BENCH_HOST_OCC0_D", "1"))       # the host walks max_occ 0 up to this d (minutes beyond)
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
os.environ["SUFR_HIP_DEBUG"] = "1"
dbg_ctx = sufr_amd.Context(0)                                          # prints the counts of a call; never timed
del os.environ["SUFR_HIP_DEBUG"]
dbg = sufr_amd.DeviceIndex(dbg_ctx, ix._h)
print(f"text {n:,} suffixes {sa.numel():,}: index ready in {time.time() - t0:.1f} s", flush=True)
g = torch.Generator(device=dev); g.manual_seed(1)
at = torch.randint(0, n - rl - 9, (nr,), generator=g, device=dev)
acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
comp = torch.arange(256, dtype=torch.uint8, device=dev)
for a, b in (b"AT", b"TA", b"CG", b"GC"):
    comp[a] = b


def batch(indels: bool):
    span = rl + 8
    src = norm[(at[:, None] + torch.arange(span, device=dev)[None, :]).reshape(-1)].view(nr, span)
    if indels:
        # per read: the text offset of every read base moves by +1 after a deletion and by -1 after an insertion
        ev = torch.rand(nr, rl, generator=g, device=dev)
        dele, ins = ev < 0.001, (ev >= 0.001) & (ev < 0.002)
        shift = torch.cumsum(dele.long() - ins.long(), dim=1)
        col = (torch.arange(rl, device=dev)[None, :] + shift).clamp_(0, span - 1)
        r = torch.gather(src, 1, col)
        r[ins] = acgt[torch.randint(0, 4, (int(ins.sum()),), generator=g, device=dev)]
    else:
        r = src[:, :rl].clone()
    qb = r.reshape(-1).contiguous()
    sub = torch.rand(qb.numel(), generator=g, device=dev) < 0.01
    qb[sub] = acgt[torch.randint(0, 4, (int(sub.sum()),), generator=g, device=dev)]
    qb[torch.rand(qb.numel(), generator=g, device=dev) < 0.002] = ord("N")
    r2 = qb.view(nr, rl)
    r2[::2] = comp[r2[::2].flip(1).long()]                             # half of the reads come from the other strand
    return qb


off = (torch.arange(nr + 1, device=dev, dtype=torch.int64) * rl).contiguous()
results = {}
for name, qb in (("substitutions", batch(False)), ("indels", batch(True))):
    for d in ds:
        for occ in occs:
            try:
                total = ix.edit_device(qb, off, d, occ, True)[0].numel()   # (warm-up: the record total, so that a timed call runs once)
            except sufr_amd.SufrHipError as e:
                print(f"edit[{name}]: d={d} max_occ={occ}: refused: {e}", flush=True)
                continue
            t_e = []
            for rep in range(reps):
                torch.cuda.synchronize()
                w0 = time.perf_counter()
                recs = ix.edit_device(qb, off, d, occ, True, cap=total)
                t_e.append((time.perf_counter() - w0) * 1e3)
            ta = ix.approx_device(qb, off, d, occ, True)[0].numel()
            t_a = []
            for rep in range(reps):
                torch.cuda.synchronize()
                w0 = time.perf_counter()
                ar = ix.approx_device(qb, off, d, occ, True, cap=ta)
                t_a.append((time.perf_counter() - w0) * 1e3)
            sys.stdout.flush()
            dbg.edit_device(qb, off, d, occ, True, cap=total)
            sys.stderr.flush()
            mins = ix.edit_device(qb, off, d, occ, True, True)[0].numel()
            print(f"edit[{name}]: d={d} max_occ={occ} both strands: {total:,} records ({total / nr:.3f} per read; {mins:,} local minima): "
                  + " ".join(f"{t:.2f}" for t in t_e) + f" ms  {nr / min(t_e) / 1e3:.3f} M reads/s;  approx: {ta:,} records: "
                  + " ".join(f"{t:.2f}" for t in t_a) + f" ms;  edit / approx {min(t_e) / min(t_a):.2f}", flush=True)
            if name == "indels":
                results[(d, occ)] = (recs, min(t_e))
            del recs, ar
lib = sufr_amd.lib()
if n <= 200_000_000 and not os.environ.get("EDIT_BENCH_NO_HOST"):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "x.sufr")
        text_h = norm.cpu().numpy(); sa_h = sa.cpu().numpy().view(np.uint32); lcp_h = np.zeros_like(sa_h)
        starts = np.zeros(1, dtype=np.uint64); names = (C.c_char_p * 1)(b"1"); err = C.create_string_buffer(256)
        assert lib.sufr_write_file(path.encode(), 1, 0, 0, text_h.ctypes.data, n, 4, sa_h.ctypes.data, lcp_h.ctypes.data, sa_h.size,
                                   0, 0, None, starts.ctypes.data, 1, names, err, len(err)) == 0
        f = sufr_amd.SufrFile(path)
        qh = qb.cpu().numpy(); oh = off.cpu().numpy().astype(np.uint64)
        for (d, occ), (got, t_m) in results.items():
            if occ == 0 and d > host_occ0_d:
                continue
            w0 = time.perf_counter()
            want = f.edit_arrays(qh, oh, d, occ, True, threads=16)
            t_h = (time.perf_counter() - w0) * 1e3
            same = all(np.array_equal(a.cpu().numpy().astype(np.int64), b.astype(np.int64)) for a, b in zip(got, want))
            print(f"host (16 threads) d={d} max_occ={occ}: {t_h:.0f} ms  {nr / t_h / 1e3:.4f} M reads/s; device is {t_h / t_m:.1f}x "
                  f"the host; records equal: {same}", flush=True)
            assert same
dbg._h = None                                                          # (ix owns the handle)
dbg_ctx.close()
ix.close(); db.close()
