"""Time of the sequence-count passes over a device-resident SA, LCP and text:   python profiles/shared_bench.py [text_len] [min_len]
Builds the index of a synthetic genome (synth.syn_human, the stand-in of repeat_bench.py) on the device, wraps it in place and
cuts it into 1, 24 and 10 000 sequences by position (evenly spaced sequence starts; no delimiter byte is needed, the clip is
positional).  For every sequence count it times, with HIP events around the call on the context's stream (SHARED_BENCH_WARMUP
warm-up calls, SHARED_BENCH_REPS timed ones: median, min and max):
  sufr_hip_shared_device kind 0, the counting call and the filling call; sufr_hip_common_device; and sufr_hip_repeats_device
  kind 0, the counting call, on the same arrays and starts -- the yardstick: what shared costs beyond repeats is the keys, the
  sort, the pair pass and the prefix.
Beside every call: the bytes it moves by the model of DESIGN.md section 21 and the time of a plain device-to-device copy of
that many bytes in the same run.  The share of the counting call that is sort_keys and k_shr_pairs comes from the probes build
(make -C sufr_amd/csrc probes; SUFR_AMD_PROBES_LIB=1), which stamps both with events and prints them to standard error.
The lines go to standard output and to profiles/shared_bench.txt (SHARED_BENCH_OUT: another path)."""
import ctypes as C
import os
import re
import statistics
import sys
import tempfile
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import sufr_amd
from sufr_amd import synth

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
min_len = int(sys.argv[2]) if len(sys.argv) > 2 else 20
reps = int(os.environ.get("SHARED_BENCH_REPS", "7"))
warm = int(os.environ.get("SHARED_BENCH_WARMUP", "2"))
out_file = open(os.environ.get("SHARED_BENCH_OUT", os.path.join(ROOT, "profiles", "shared_bench.txt")), "w")


def say(line):
    print(line, flush=True)
    out_file.write(line + "\n")
    out_file.flush()


t0 = time.time()
x, _ = synth.syn_human(n, seed=4, device="cuda")
norm = torch.where((x >= 97) & (x <= 122), x - 32, x).contiguous()
del x
db = sufr_amd.DeviceBuilder(0)
sa, lcp = db.sort(norm, is_dna=True)
ix = sufr_amd.DeviceIndex.wrap(db.ctx, norm, sa, is_dna=True, prefix_table=False)
s, N, w = sa.numel(), norm.numel(), 4
say(f"text {N:,} suffixes {s:,} min_len {min_len}: index ready in {time.time() - t0:.1f} s; {warm} warm-up + {reps} timed calls each")
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
    return timed(copy)[1]


def report(name, ms, nbytes):
    cp = copy_ms(nbytes)
    med, cmed = statistics.median(ms), statistics.median(cp)
    say(f"{name:28s} {med:9.3f} ms (min {min(ms):.3f} max {max(ms):.3f})  model {nbytes / 1e9:7.3f} GB -> {nbytes / med / 1e6:7.1f} GB/s;"
        f"  copy of the same bytes {cmed:8.3f} ms (min {min(cp):.3f} max {max(cp):.3f})  ratio {med / cmed:5.2f}")
    return med


for num in (1, 24, 10_000):
    starts = (np.arange(num, dtype=np.uint64) * (N // num)).astype(np.uint64)
    st_ptr, st_n = (starts.ctypes.data, num) if num > 1 else (None, 0)
    base = (db.ctx.handle, ix._h, lcp.data_ptr(), st_ptr, st_n)

    def shared_call(cap, out):
        total, st = C.c_uint64(0), sufr_amd.SharedStats()
        rc = L.sufr_hip_shared_device(*base, 0, min_len, 2, 0, 0, 0, cap, *(o.data_ptr() if o is not None else None for o in out), C.byref(total), C.byref(st))
        assert rc in (0, -5), rc
        return total.value, st.as_dict()

    def repeats_call():
        total, st = C.c_uint64(0), sufr_amd.RepeatStats()
        rc = L.sufr_hip_repeats_device(*base, 0, min_len, 2, 0, 0, None, None, None, C.byref(total), C.byref(st))
        assert rc in (0, -5), rc
        return total.value, st.as_dict()

    # bytes by the model of DESIGN.md section 21 (w: the index width).  fold and find as in section 19 (with several
    # sequences l is written and read once more); keys: SA read, 8 bytes written; a digit pass: 8 read by the counts, 8 read
    # and 8 written by the scatter; pairs: the keys, one 64-byte line of l per pair, H zeroed and added to; prefix: H read and
    # written twice; find: P read once more
    clip = 2 * s * w if num > 1 else 0
    fold, find = 2 * s * w + 64 * s + s // 2 + s * w // 64 + clip, s * w + s // 2
    passes = (max(num - 1, 0).bit_length() + 7) // 8
    extra = (s * w + 8 * s) + 24 * s * passes + (8 * s + 64 * s + 3 * s * w) + 4 * s * w + s * w
    say(f"--- {num} sequence(s): {passes} digit pass(es) of the sort")
    with Stderr() as err:
        (total, st), ms = timed(lambda: shared_call(0, [None] * 4))
    count_med = report("shared: count", ms, fold + find + extra)
    sort_ms = [float(v) for v in re.findall(r"shared: sort ([0-9.]+) ms", err.text)][warm:]
    pair_ms = [float(v) for v in re.findall(r"pairs ([0-9.]+) ms", err.text)][warm:]
    if sort_ms and pair_ms:
        a, b = statistics.median(sort_ms), statistics.median(pair_ms)
        say(f"    sort_keys {a:9.3f} ms ({a / count_med * 100:4.1f} %)   k_shr_pairs {b:9.3f} ms ({b / count_med * 100:4.1f} %) of the counting call")
    else:
        say("    sort_keys / k_shr_pairs not stamped: this is not the probes build (make -C sufr_amd/csrc probes; SUFR_AMD_PROBES_LIB=1)")
    out = [torch.empty(max(total, 1), dtype=torch.int64, device="cuda") for _ in range(4)]
    (total2, st2), ms = timed(lambda: shared_call(total, out))
    assert total2 == total and st2 == st
    report("shared: count + fill", ms, fold + 2 * find + extra + s * w + 32 * total)
    say(f"    {st}")
    prof = torch.empty(num, dtype=torch.int64, device="cuda")
    _, ms = timed(lambda: db.ctx.check(L.sufr_hip_common_device(*base, prof.data_ptr())))
    report("common", ms, fold + find + extra)
    (rtotal, rst), ms = timed(repeats_call)
    rep_med = report("repeats kind 0: count", ms, fold + find)
    assert rtotal == total and all(rst[k] == st[k] for k in rst)
    say(f"    shared count / repeats count {count_med / rep_med:5.2f}")
ix.close(); db.close()
out_file.close()
