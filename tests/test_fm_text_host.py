"""The FM-index as a self-contained object on the host (include/sufr_fm_text.h, sufr_query.cpp): text samples and extract against
SufrFile.text, the index file (save, load and the checks of load on damaged files), the sequences it carries, and `sufr fm` with
--save, --index and --extract.  Every comparison is exact equality.  The request sets and their conditions are built here and
used by tests/test_fm_text_gpu.py too."""
import ctypes as C
import re
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sufr_amd
from sufr_amd import FmIndex, SufrFile, SufrHipError
from oracle_helper import GOLDEN
from test_bwt_host import LF_FILES, write_arrays
from test_fm_host import query_set, random_text, sorted_sa, Witness
from test_lz_host import fibonacci, oracle_file
from test_match_host import run

ROOT = Path(__file__).resolve().parent.parent
EXP = GOLDEN / "expected"
SAMPLES = (1, 2, 7, 32)
INVALID, IO, CAPACITY, UNSUPPORTED, NO_DEVICE = -1, -7, -5, -6, -2
PAGE = 4096
SECTIONS = ("tables", "starts", "names", "blocks", "marks", "kept", "text_kept")


# ---------------------------------------------------------------------------------------------------------------------
# the request sets
# ---------------------------------------------------------------------------------------------------------------------
def walked_ranks(sa: np.ndarray, n: int, q: int, start: int, end: int):
    """the ranks a request's chunks take their steps from: ISA[p + 1] for every position p the walk passes (silent steps too)"""
    isa = np.zeros(n + 1, dtype=np.int64)
    isa[sa] = np.arange(n)
    isa[n] = isa[0]                                                   # the cyclic row stands for position n
    out = []
    for k in range(start // q, (end - 1) // q + 1):
        top = min((k + 1) * q, n)
        out.append(isa[np.arange(max(start, k * q), top) + 1])
    return np.concatenate(out)


def request_set(n: int, q: int, B: int, sa=None, seed: int = 0, random: int = 600):
    """(starts, ends, conditions): the stated requests first, then `random` random ones.  The conditions name the index of the
    request that meets each of them, computed from n, q and B; None where the text is too short for it"""
    rng = np.random.default_rng(seed)
    reqs, cond = [], {}

    def add(name, a, b):
        cond[name] = len(reqs)
        reqs.append((a, b))

    add("empty", min(3, n), min(3, n))
    add("start_after_end", min(5, n), min(2, n - 1))
    add("end_after_n", max(n - 3, 0), n + 10)
    add("start_after_n", n + 1, n + 5)
    add("last_byte", n - 1, n)
    add("first_byte", 0, 1)
    add("whole", 0, n)
    huge = 2**64 - 1
    add("huge_end", max(n - 2, 0), huge)
    if q >= 4 and n > q:
        add("inside_a_chunk", 1, 3)                                  # [1, 3) lies in chunk 0
    if n > 3 * q + 1 and q > 1:
        for name, a, b in (("on_multiples", q, 3 * q), ("before_multiples", q - 1, 3 * q - 1), ("after_multiples", q + 1, 3 * q + 1)):
            add(name, a, b)
    elif n > 3:
        add("on_multiples", 1, 3)                                    # (q == 1: every position is a multiple)
    if n % q and n > q:
        add("last_short_chunk", n - n % q - 1, n - 1 if n % q > 1 else n)
    if sa is not None and n > B + 2:                                 # a chunk whose walk steps from ranks of two blocks
        for a in range(0, n - 1, max(q, 1)):
            b = min(a + max(q, 2), n)
            ranks = walked_ranks(sa, n, q, a, b)
            if np.unique(ranks // B).size > 1:
                add("crosses_a_block", a, b)
                break
    for _ in range(random):
        a = int(rng.integers(0, n + 2))
        b = a + int(rng.integers(0, min(n, 4 * max(q, 8)) + 1)) if rng.integers(0, 8) else int(rng.integers(0, n + 2))
        reqs.append((a, b))
    starts = np.array([r[0] for r in reqs], dtype=np.uint64)
    ends = np.array([r[1] for r in reqs], dtype=np.uint64)
    return starts, ends, cond


def want_extract(text: np.ndarray, starts, ends):
    """(offsets, bytes) as the extract contract lays them out"""
    n = text.size
    parts = []
    for a, b in zip(starts.tolist(), ends.tolist()):
        b = min(b, n)
        a = min(a, b)
        parts.append(text[a:b])
    off = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)
    return off, (np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)).astype(np.uint8)


def check_extract(fm, text, sa, q, threads=(0,), seed=0, random=600, tag=""):
    """extract of an index equals slices of the text, for the stated requests and the random ones; returns the conditions"""
    n, B = text.size, fm.info["block"]
    starts, ends, cond = request_set(n, q, B, sa, seed, random)
    w_off, w_bytes = want_extract(text, starts, ends)
    for t in threads:
        off, got = fm.extract_ranges(starts, ends, threads=t)
        assert off.dtype == np.uint64 and got.dtype == np.uint8, tag
        assert np.array_equal(off, w_off) and np.array_equal(got, w_bytes), (tag, t)
    return cond


# ---------------------------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_text_header_symbols_are_exported():
    hdr = (ROOT / "include" / "sufr_fm_text.h").read_text()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(sufr_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(sufr_amd.FM_TEXT_EXPORTS), declared ^ set(sufr_amd.FM_TEXT_EXPORTS)
    L = sufr_amd.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(sufr_amd.LIB_PATH)], capture_output=True, text=True).stdout
    for name in declared:
        assert hasattr(L, name) and re.search(rf"\bT {name}\b", nm), name
    assert C.sizeof(sufr_amd.FmTextInfo) == 24
    for cls, names in ((FmIndex, ("extract_ranges", "extract", "text_info", "save", "load", "sequences", "to_device")),
                       (sufr_amd.DeviceFmIndex, ("extract_device", "extract_ranges", "extract", "to_host", "text_info"))):
        for name in names:
            assert hasattr(cls, name), (cls, name)


def test_host_stubs_answer_no_device(tmp_path):
    """every device entry point of the header has a stub, and the stubs answer SUFR_HIP_E_NO_DEVICE: a C program linked against
    the stubs alone calls each of them"""
    stubs = ROOT / "sufr_amd" / "csrc" / "sufr_host_stubs.cpp"
    device = [name for name in sufr_amd.FM_TEXT_EXPORTS if name.startswith("sufr_hip_")]
    assert len(device) == 6
    for name in device:
        assert re.search(rf"\bint {name}\(", stubs.read_text()), name
    main = tmp_path / "main.cpp"
    main.write_text('#include "sufr_fm_text.h"\n#include <stdio.h>\nint main() {\n  uint64_t t = 7; sufr_hip_fm* d = (sufr_hip_fm*)1; sufr_fm* h = (sufr_fm*)1;\n'
                    '  sufr_fm_text_info ti;\n  int rc[6] = {sufr_hip_fm_build_flags(0, 0, 32, SUFR_FM_TEXT, &d), sufr_hip_fm_get_text_info(0, &ti),\n'
                    '    sufr_hip_fm_extract_batch_device(0, 0, 0, 0, 0, 0, 0, 0, &t), sufr_hip_fm_extract_batch(0, 0, 0, 0, 0, 0, 0, 0, &t),\n'
                    '    sufr_hip_fm_upload(0, 0, &d), sufr_hip_fm_download(0, 0, &h)};\n'
                    '  for (int i = 0; i < 6; i++) printf("%d ", rc[i]);\n  printf("%d %d %llu\\n", d == 0, h == 0, (unsigned long long)t);\n  return 0;\n}\n')
    exe = tmp_path / "stubs"
    subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT / 'include'}", "-o", str(exe), str(main), str(stubs)],
                   check=True, capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == [str(NO_DEVICE)] * 6 + ["1", "1", "0"], out


def test_the_header_is_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "sufr_fm_text.h"\nint main(void) { sufr_fm_text_info i = {0, 0, 0}; return (int)i.text_bytes + (int)(SUFR_FM_TEXT & 0); }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", f"-I{ROOT / 'include'}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---------------------------------------------------------------------------------------------------------------------
# extract against SufrFile.text
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LF_FILES)
def test_extract_equals_the_text_on_golden_files(name):
    f = SufrFile(EXP / name)
    text, sa = np.asarray(f.text).copy(), np.asarray(f.suffix_array).astype(np.int64)
    n = text.size
    for q in SAMPLES:
        plain = f.fm(q)
        fm = f.fm(q, 0, text=True)
        ti = fm.text_info
        assert fm.info == plain.info                                  # sufr_fm_info keeps its meaning
        assert ti["text_samples"] == (n + q - 1) // q and ti["text_bytes"] == (n + q - 1) // q * f.index_width
        assert plain.text_info["text_samples"] == 0 and plain.text_info["text_bytes"] == 0
        cond = check_extract(fm, text, sa, q, threads=(1, 3, 0), seed=q, tag=(name, q))
        for must in ("empty", "start_after_end", "end_after_n", "start_after_n", "last_byte", "first_byte", "whole", "on_multiples"):
            assert must in cond, (name, q, must)
        if n > 3 * q + 1 and q > 1:
            assert "before_multiples" in cond and "after_multiples" in cond
        if q >= 4 and n > q:
            assert "inside_a_chunk" in cond
        if n % q and n > q:
            assert "last_short_chunk" in cond
        if n > 20 * fm.info["block"]:
            assert "crosses_a_block" in cond, (name, q)
        assert fm.extract(0, n) == text.tobytes() and fm.extract(n - 1, n) == text[-1:].tobytes() and fm.extract(2, 1) == b""
        other = f.fm(q, 2, text=True)                                 # two builds, different workers: the same object
        assert other.text_info == ti
        fm.close(); plain.close(); other.close()


def planted(tmp_path, text: np.ndarray, name="p"):
    text = np.ascontiguousarray(text, dtype=np.uint8)
    sa = sorted_sa(text)
    return write_arrays(tmp_path / f"{name}.sufr", text, sa), text, sa.astype(np.int64)


@pytest.mark.parametrize("n", [31, 32, 33, 63, 64, 65, 95, 96, 97, 191, 192, 193])
def test_sizes_around_the_sample_rate_and_the_block(tmp_path, n):
    """n = 32 k - 1, 32 k, 32 k + 1 at q == 32 and n around B and 2 B: the last chunk full, one byte long and one short"""
    f, text, sa = planted(tmp_path, random_text(n, n))
    for q in (32, 1, 5):
        fm = f.fm(q, text=True)
        assert fm.info["block"] == 96 and fm.text_info["text_samples"] == (n + q - 1) // q
        check_extract(fm, text, sa, q, seed=n, random=200, tag=(n, q))
        for a in range(0, n, 7):                                      # every end from a few starts
            starts = np.full(n + 1 - a, a, dtype=np.uint64)
            ends = np.arange(a, n + 1, dtype=np.uint64)
            off, got = fm.extract_ranges(starts, ends)
            w_off, w_bytes = want_extract(text, starts, ends)
            assert np.array_equal(off, w_off) and np.array_equal(got, w_bytes), (n, q, a)


def test_oracle_built_texts(oracle, tmp_path):
    """texts through the oracle: A^1000, a Fibonacci string and random DNA of 96 k + 1 symbols"""
    rng = np.random.default_rng(3)
    bodies = {"a": np.full(1000, ord("A"), dtype=np.uint8), "fib": fibonacci(3000),
              "rnd": np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 959)]}
    for name, body in bodies.items():
        f = oracle_file(oracle, tmp_path, body, name, is_dna=True, allow_ambiguity=True)
        text, sa = np.asarray(f.text).copy(), np.asarray(f.suffix_array).astype(np.int64)
        assert f.len_suffixes == f.text_len == body.size + 1
        for q in (32, 7):
            fm = f.fm(q, text=True)
            check_extract(fm, text, sa, q, threads=(0, 2), seed=5, random=300, tag=(name, q))


def test_all_byte_values_and_an_end_byte_that_is_not_the_smallest(tmp_path):
    rng = np.random.default_rng(11)
    text = rng.integers(0, 255, 5000).astype(np.uint8)
    text[:255] = np.arange(255)
    text[-1] = 255                                                    # the end byte is the largest byte value
    f, text, sa = planted(tmp_path, text, "bytes")
    for q in (32, 3):
        fm = f.fm(q, text=True)
        assert (fm.info["symbols"], fm.info["block"], fm.info["stride"]) == (256, 1024, 2048)
        cond = check_extract(fm, text, sa, q, seed=q, random=300, tag=("bytes", q))
        assert "crosses_a_block" in cond
    middle = np.frombuffer(b"TTGACCA$GATTACA$$ACGT" * 9 + b"M", dtype=np.uint8)      # 'M' ends the text: '$' and 'A'.. are smaller and larger
    g, mtext, msa = planted(tmp_path, middle, "middle")
    for q in (1, 2, 4, 8, 32):
        check_extract(g.fm(q, text=True), mtext, msa, q, seed=q, random=200, tag=("middle", q))


def test_refusals_capacity_and_no_requests():
    f = SufrFile(EXP / "long_dna_sequence_allow_ambiguity.sufr")
    text = np.asarray(f.text).copy()
    L = sufr_amd.lib()
    plain = f.fm(32)
    with pytest.raises(SufrHipError) as err:
        plain.extract_ranges([0], [5])
    assert err.value.code == UNSUPPORTED
    h = C.c_void_p()
    assert L.sufr_file_fm_build_flags(f._h, 0, 1, C.byref(h), 0) == INVALID and not h.value      # SUFR_FM_TEXT with sample == 0
    assert L.sufr_file_fm_build_flags(f._h, 32, 2, C.byref(h), 0) == INVALID and not h.value     # an unknown flag
    with pytest.raises(SufrHipError) as err:
        f.fm(0, text=True)
    assert err.value.code == INVALID
    assert L.sufr_file_fm_build_flags(f._h, 32, 0, C.byref(h), 0) == 0                           # flags == 0: the old build
    same = FmIndex(h, f.index_width)
    assert same.info == plain.info and same.text_info == plain.text_info
    fm = f.fm(32, text=True)
    starts, ends, _ = request_set(text.size, 32, 96, None, seed=1, random=50)
    w_off, w_bytes = want_extract(text, starts, ends)
    z = int(w_off[-1])
    off, out = np.full(starts.size + 1, 7, dtype=np.uint64), np.full(z + 9, 0xAA, dtype=np.uint8)
    total = C.c_uint64(0)
    args = (fm._h, starts.ctypes.data, ends.ctypes.data, starts.size, off.ctypes.data, out.ctypes.data)
    assert L.sufr_fm_extract_batch(*args, z - 1, C.byref(total), 0) == CAPACITY
    assert total.value == z and (out == 0xAA).all() and np.array_equal(off, w_off)               # no byte written, the offsets are
    assert L.sufr_fm_extract_batch(*args, z, C.byref(total), 3) == 0
    assert total.value == z and np.array_equal(out[:z], w_bytes) and (out[z:] == 0xAA).all()
    off[0] = 9
    assert L.sufr_fm_extract_batch(fm._h, None, None, 0, off.ctypes.data, None, 0, C.byref(total), 0) == 0 and total.value == 0 and off[0] == 0
    o, b = fm.extract_ranges(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64))
    assert o.tolist() == [0] and b.size == 0


# ---------------------------------------------------------------------------------------------------------------------
# save and load
# ---------------------------------------------------------------------------------------------------------------------
def answers(fm, qs, reqs, text_on):
    lo, hi = fm.search_batch(qs)
    off, pos = fm.locate_ranges(lo, hi, 5)
    short = [q[:24] for q in qs if len(q) >= 3][:40]
    recs = fm.approx_arrays(*sufr_amd.pack_queries(short), 2)
    out = [lo, hi, off, pos, *recs]
    if text_on:
        out += list(fm.extract_ranges(*reqs))
    return out


@pytest.mark.parametrize("name", LF_FILES)
def test_load_of_save_answers_like_the_built_index(tmp_path, name):
    src = tmp_path / name
    shutil.copy(EXP / name, src)
    f = SufrFile(src)
    w = Witness(np.array(f.text), np.array(f.suffix_array))
    starts_names = (list(f.sequence_starts), list(f.sequence_names))
    built, want, paths = {}, {}, {}
    for text_on in (False, True):
        fm = built[text_on] = f.fm(7, text=text_on)
        qs = query_set(w, fm.info["block"], seed=2)
        reqs = request_set(w.n, 7, fm.info["block"], None, seed=4, random=100)[:2]
        want[text_on] = answers(fm, qs, reqs, text_on)
        a, b = tmp_path / f"a{int(text_on)}.fm", tmp_path / f"b{int(text_on)}.fm"
        fm.save(a)
        fm.save(b, names_from=f)
        assert a.read_bytes() == b.read_bytes()                       # two saves, and the remembered names are the file's
        assert a.stat().st_size == fm.text_info["file_bytes"] and a.stat().st_size % PAGE in (0, a.stat().st_size % PAGE)
        paths[text_on] = a
    f.close()
    src.write_bytes(b"")                                              # no .sufr in sight
    for text_on in (False, True):
        for threads in (1, 0):
            fm = FmIndex.load(paths[text_on], threads)
            assert fm.info == built[text_on].info and fm.text_info == built[text_on].text_info
            assert fm.sequences() == starts_names
            qs = query_set(w, fm.info["block"], seed=2)
            reqs = request_set(w.n, 7, fm.info["block"], None, seed=4, random=100)[:2]
            got = answers(fm, qs, reqs, text_on)
            assert len(got) == len(want[text_on]) and all(np.array_equal(x, y) for x, y in zip(got, want[text_on])), (name, text_on)
            again = tmp_path / "again.fm"
            fm.save(again)
            assert again.read_bytes() == paths[text_on].read_bytes()  # load(save(x)) saves the same file
        if not text_on:
            with pytest.raises(SufrHipError) as err:
                fm.extract_ranges([0], [1])
            assert err.value.code == UNSUPPORTED


def test_saving_without_names_and_with_other_names(tmp_path):
    f = SufrFile(EXP / "2ns.sufr")
    fm = f.fm(2, text=True)
    assert fm.sequences() == (list(f.sequence_starts), list(f.sequence_names)) and len(f.sequence_names) == 2
    named = tmp_path / "named.fm"
    fm.save(named)
    fm.set_sequences([], [])
    bare = tmp_path / "bare.fm"
    fm.save(bare)
    assert FmIndex.load(bare).sequences() == ([], []) and bare.stat().st_size == fm.text_info["file_bytes"] <= named.stat().st_size
    fm.save(bare, names_from=f)
    assert bare.read_bytes() == named.read_bytes()
    with pytest.raises(SufrHipError):
        fm.set_sequences([5, 2], ["a", "b"])                          # decreasing starts
    with pytest.raises(SufrHipError):
        fm.set_sequences([0, 10 ** 6], ["a", "b"])                    # behind the text


# ---------------------------------------------------------------------------------------------------------------------
# damaged files
# ---------------------------------------------------------------------------------------------------------------------
def sections(raw: bytes):
    """{name: (offset, length)} of an index file"""
    table = struct.unpack_from("<14Q", raw, 72)
    return {name: (table[2 * i], table[2 * i + 1]) for i, name in enumerate(SECTIONS)}


def header_field(raw: bytes, name: str) -> int:
    at = {"version": 8, "flags": 12, "w": 16, "e": 20, "K": 24, "B": 28, "stride": 32, "cbytes": 36}[name]
    return struct.unpack_from("<I", raw, at)[0]


def damaged_files(raw: bytes):
    """(tag, bytes) of every damage: truncations at and inside every section, and one targeted corruption per check of load"""
    sec = sections(raw)
    s, q = struct.unpack_from("<QQ", raw, 40)
    w, cbytes, stride, B = (header_field(raw, k) for k in ("w", "cbytes", "stride", "B"))
    out = []
    for name, (off, length) in sec.items():
        out.append((f"cut at {name}", raw[:off]))
        if length > 1:
            out.append((f"cut inside {name}", raw[:off + length // 2]))
    out.append(("cut inside the header", raw[:100]))
    out.append(("empty", b""))
    out.append(("one byte more", raw + b"\0"))

    def patched(tag, at, new: bytes):
        assert raw[at:at + len(new)] != new, tag
        out.append((tag, raw[:at] + new + raw[at + len(new):]))

    def bump(tag, at, width=8, by=1):
        v = int.from_bytes(raw[at:at + width], "little")
        patched(tag, at, ((v + by) % (1 << (8 * width))).to_bytes(width, "little"))

    patched("magic", 0, b"X")
    bump("version", 8, 4)
    patched("unknown flag", 12, (header_field(raw, "flags") | 4).to_bytes(4, "little"))
    patched("width", 16, (5).to_bytes(4, "little"))
    bump("K", 24, 4)
    bump("ranks", 40)
    bump("samples", 56)
    bump("a section offset", 72 + 16 * 3)
    blocks, marks, kept, text_kept, tables = sec["blocks"][0], sec["marks"][0], sec["kept"][0], sec["text_kept"][0], sec["tables"][0]
    col = tables + 257 * 8
    absent = next(c for c in range(256) if struct.unpack_from("<I", raw, col + 4 * c)[0] == 0xFFFFFFFF)
    patched("a BWT byte without a column", blocks + cbytes + min(5, s - 1), bytes([absent]))
    bump("a checkpoint off by one", blocks + stride, w)               # the first count of block 1
    patched("a checkpoint byte behind K w", blocks + cbytes - 1, b"\1")
    last = blocks + (s // B) * stride + cbytes + s % B
    patched("a non-zero byte behind s", last, b"A")
    bump("a `before` off by one", marks + 16 + 8)                     # of mark word 1
    if s % 64:
        patched("a mark bit behind s", marks + 16 * (s // 64) + 7, bytes([raw[marks + 16 * (s // 64) + 7] | 0x80]))
    bump("a kept value that is no multiple of q", kept + w, w)
    samples = struct.unpack_from("<Q", raw, 56)[0]
    zero = next(i for i in range(samples) if not int.from_bytes(raw[kept + w * i:kept + w * (i + 1)], "little"))
    patched("no kept value is 0", kept + w * zero, q.to_bytes(w, "little"))
    bump("C[256]", tables + 256 * 8)
    bump("C[1]: C decreases or a byte value without its column", tables + 8)
    bump("a column", col + 4 * raw[blocks + cbytes], 4)
    r = int.from_bytes(raw[text_kept + w:text_kept + 2 * w], "little")           # text_kept[1]: a marked rank
    bits = struct.unpack_from("<Q", raw, marks + 16 * (r // 64))[0]
    unmarked = next(x for x in range(64 * (r // 64), 64 * (r // 64) + 64) if not (bits >> (x % 64)) & 1)
    patched("a text_kept entry at an unmarked rank", text_kept + w, unmarked.to_bytes(w, "little"))
    patched("two text_kept entries swapped", text_kept, raw[text_kept + w:text_kept + 2 * w] + raw[text_kept:text_kept + w])
    patched("a text_kept entry behind s", text_kept + 2 * w, (s + 3).to_bytes(w, "little"))
    patched("a sequence start behind the text", sec["starts"][0], (s + 1).to_bytes(8, "little"))
    patched("a name that does not end", sec["names"][0] + sec["names"][1] - 1, b"x")
    assert q > 1
    return out


@pytest.fixture(scope="module")
def good_index(tmp_path_factory):
    d = tmp_path_factory.mktemp("fmfile")
    f = SufrFile(EXP / "long_dna_sequence_allow_ambiguity.sufr")
    path = d / "good.fm"
    f.fm(7, text=True).save(path)
    return d, path, path.read_bytes()


def test_damaged_files_are_refused_with_a_message(good_index):
    d, path, raw = good_index
    assert FmIndex.load(path).extract(0, 4) == SufrFile(EXP / "long_dna_sequence_allow_ambiguity.sufr").text[:4].tobytes()
    cases = damaged_files(raw)
    assert len(cases) > 35
    messages = set()
    for tag, data in cases:
        bad = d / "bad.fm"
        bad.write_bytes(data)
        with pytest.raises(SufrHipError) as err:
            FmIndex.load(bad)
        assert err.value.code in (INVALID, IO) and len(err.value.message) > len(str(bad)) + 2, (tag, err.value)
        messages.add(err.value.message.split(": ", 1)[1].split(":")[0])
    assert {"header", "tables", "blocks", "marks", "kept", "text_kept", "sequences"} <= messages, messages
    with pytest.raises(SufrHipError) as err:
        FmIndex.load(d / "missing.fm")
    assert err.value.code == IO


def asan_cli():
    r = subprocess.run(["make", "-C", str(ROOT / "sufr_amd" / "csrc"), "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return ROOT / "sufr_amd" / "csrc" / "_build" / "sufr_host_asan"


def test_damaged_files_through_the_sanitizer_build_of_the_cli(good_index):
    """the stand-alone sanitizer build of the CLI (nothing preloaded) on every damaged file and on seeded random byte flips:
    it exits 0 or 1 and the sanitizers report nothing"""
    d, path, raw = good_index
    exe = asan_cli()
    cases = damaged_files(raw)
    rng = np.random.default_rng(17)
    sec = sections(raw)
    spots = [0, 8, 12, 16, 24, 40, 48, 56, 64, 72] + [off for off, _ in sec.values()]
    for i in range(300):
        data = bytearray(raw)
        for _ in range(int(rng.integers(1, 4))):
            at = int(rng.integers(0, len(raw))) if i % 3 else min(int(rng.choice(spots)) + int(rng.integers(0, 40)), len(raw) - 1)
            data[at] ^= 1 << int(rng.integers(0, 8))
        cases.append((f"flip {i}", bytes(data)))
    good = subprocess.run([str(exe), "fm", "--index", str(path), "--locate", "ACGT"], capture_output=True, text=True)
    assert good.returncode == 0 and good.stdout and "Sanitizer" not in good.stderr
    seen = {0: 0, 1: 0}
    for tag, data in cases:
        bad = d / "asan.fm"
        bad.write_bytes(data)
        for args in (("--locate", "ACGT"), ("--extract", "--suffix-len", "9", "ACGT")):
            r = subprocess.run([str(exe), "fm", "--index", str(bad), *args], capture_output=True, text=True)
            assert r.returncode in (0, 1) and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (tag, r.returncode, r.stderr[-2000:])
            assert r.returncode == 0 or r.stderr.strip(), tag
            seen[r.returncode] += 1
    assert seen[1] > 100


# ---------------------------------------------------------------------------------------------------------------------
# sufr fm --save / --index / --extract
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_save_index_and_extract(tmp_path):
    name, queries = "long_dna_sequence_allow_ambiguity.sufr", ["ACGT", "GATTACA", "N", "TTTTTTTTTTTTTTTTTTTTTTTTTT", "AC"]
    src = tmp_path / name
    shutil.copy(EXP / name, src)
    raw = SufrFile(src).text.tobytes()
    near = [raw[100:114].decode(), raw[5000:5007].decode() + "A" + raw[5008:5016].decode()]      # windows of the text, one with a base changed
    want = {"count": run("count", src, *queries), "locate": run("locate", src, *queries), "locate_a": run("locate", "-a", src, *queries),
            "approx": run("approx", "-d", 1, src, *near),
            "extract": run("extract", src, "GATTACA", "ACGTT"), "extract_len": run("extract", "-p", 3, "-s", 11, src, "GATTACA", "ACGTT", "NNN")}
    from_sufr = run("fm", "--extract", "--prefix-len", 3, "--suffix-len", 11, src, "GATTACA", "ACGTT", "NNN")
    assert from_sufr.stdout == want["extract_len"].stdout != "" and from_sufr.stderr == want["extract_len"].stderr
    idx, bare = tmp_path / "x.fm", tmp_path / "bare.fm"
    assert run("fm", src, "--save", idx, "--text", "-s", 32).stdout == ""
    assert run("fm", src, "--save", bare, "-s", 5).stdout == ""
    f = SufrFile(src)
    assert idx.read_bytes() == _saved(f.fm(32, text=True), tmp_path) and bare.read_bytes() == _saved(f.fm(5), tmp_path)
    f.close()
    src.write_bytes(b"")                                              # the second command opens no .sufr
    assert run("fm", "--index", idx, *queries).stdout == want["count"].stdout != ""
    for index in (idx, bare):
        got = run("fm", "--index", index, "--locate", *queries)
        assert got.stdout == want["locate"].stdout != "" and got.stderr == want["locate"].stderr
        assert run("fm", "--index", index, "--locate", "-a", *queries).stdout == want["locate_a"].stdout
    got = run("fm", "--index", idx, "--mismatches", 1, *near)
    assert sorted(got.stdout.splitlines()) == sorted(want["approx"].stdout.splitlines()) and got.stdout
    assert run("fm", "--index", idx, "--extract", "GATTACA", "ACGTT").stdout == want["extract"].stdout != ""
    got = run("fm", "--index", idx, "--extract", "--prefix-len", 3, "--suffix-len", 11, "GATTACA", "ACGTT", "NNN")
    assert got.stdout == want["extract_len"].stdout and got.stderr == want["extract_len"].stderr
    refused = run("fm", "--index", bare, "--extract", "GATTACA", check=False)
    assert refused.returncode == 1 and refused.stdout == "" and "text" in refused.stderr
    broken = tmp_path / "broken.fm"
    broken.write_bytes(idx.read_bytes()[:-100])
    r = run("fm", "--index", broken, "ACGT", check=False)
    assert r.returncode == 1 and r.stdout == "" and r.stderr.strip()
    assert run("fm", "--index", tmp_path / "none.fm", "ACGT", check=False).returncode == 1


def _saved(fm, tmp_path) -> bytes:
    p = tmp_path / "py.fm"
    fm.save(p)
    return p.read_bytes()


# ---------------------------------------------------------------------------------------------------------------------
# sufr fm: one session behind count, --locate, --mismatches, --index, --save, --extract and --smems
# ---------------------------------------------------------------------------------------------------------------------
NS, NS_QUERIES = EXP / "2ns.sufr", ["AC", "GT", "N", "TTT"]


def test_cli_locate_at_sample_zero_prints_the_lines_of_locate():
    """--locate alone builds at sample 1 when told -s 0"""
    want, got = run("locate", NS, *NS_QUERIES), run("fm", "--locate", "-s", 0, NS, *NS_QUERIES)
    assert got.stdout == want.stdout != "" and got.stderr == want.stderr


def test_cli_index_without_samples_counts_and_refuses_the_rest(tmp_path):
    bare = tmp_path / "bare.fm"
    run("fm", NS, "--save", bare, "-s", 0)
    assert run("fm", "--index", bare, *NS_QUERIES).stdout == run("count", NS, *NS_QUERIES).stdout != ""
    for args in (("--locate",), ("-d", 1), ("--extract",)):
        r = run("fm", "--index", bare, *args, "ACGT", check=False)
        assert r.returncode == 1 and r.stdout == "" and len(r.stderr.splitlines()) == 1 and "counts only" in r.stderr, (args, r.stderr)


def test_cli_save_alone_writes_a_file_that_index_reads(tmp_path):
    idx = tmp_path / "x.fm"
    r = run("fm", NS, "--save", idx, check=False)
    assert r.returncode == 0 and r.stdout == "" and r.stderr == ""
    want, got = run("locate", NS, *NS_QUERIES), run("fm", "--index", idx, "--locate", *NS_QUERIES)
    assert got.stdout == want.stdout != "" and got.stderr == want.stderr


def test_cli_mismatches_from_an_index_file_prints_the_lines_of_the_sufr(tmp_path):
    idx = tmp_path / "x.fm"
    run("fm", NS, "--save", idx)
    for flags in ((), ("-b", "-a")):
        want, got = run("fm", "-d", 1, *flags, NS, "ACGA", "NNNT", "TTTTTT"), run("fm", "-d", 1, *flags, "--index", idx, "ACGA", "NNNT", "TTTTTT")
        assert got.stdout == want.stdout != "" and got.stderr == want.stderr


def test_cli_write_reverse_and_smems_in_one_run(oracle, tmp_path):
    from test_fm_match_host import cli_files, cli_queries
    name = "long_dna_sequence_allow_ambiguity.sufr"
    src, rev, _, _ = cli_files(oracle, tmp_path, name)
    queries, again = cli_queries(src, name), tmp_path / "again.fa"
    got = run("fm", src, "--write-reverse", again, "--smems", "--reverse", rev, "-k", 5, *queries)
    assert again.read_bytes() == (tmp_path / "rev.fa").read_bytes() != b""
    assert got.stdout == run("match", "-k", 5, src, *queries).stdout != ""
