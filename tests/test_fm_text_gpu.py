"""The self-contained FM-index on the GPU (include/sufr_fm_text.h, sufr_fm.inc): text samples and extract against the host path
of the same library and slices of the text; the copies between host and device and the index file.  Every comparison is exact
array equality, on the loaded, the wrapped and the 64-bit index, at the default BWT tile and with the tile at its minimum."""
import os
import subprocess
import sys
import threading
from pathlib import Path

import numpy as np
import pytest
import torch

import sufr_amd
from sufr_amd import DeviceIndex, FmIndex, SufrFile, SufrHipError, pack_queries
from oracle_helper import GOLDEN
from test_kmer_gpu import indexes
from test_lz_host import fibonacci, oracle_file
from test_bwt_gpu import _unsigned, wrapped
from test_fm_host import Witness, query_set, sorted_sa
from test_fm_text_host import CAPACITY, UNSUPPORTED, INVALID, request_set, want_extract

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
EXP = GOLDEN / "expected"
T = 256                                                               # the smallest tile
TILES = (0, T)
SAMPLES = (1, 32)


@pytest.fixture(scope="module")
def ctx():
    c = sufr_amd.Context(0)
    yield c
    c.set_bwt_tile(0)
    c.close()


class Wanted:
    """the requests of one text at one sample rate and their answers, computed once: slices of the text"""

    def __init__(self, text: np.ndarray, sa: np.ndarray, q: int, B: int, seed: int = 0):
        self.text, self.q = text, q
        self.starts, self.ends, self.cond = request_set(text.size, q, B, sa, seed, 600)
        self.off, self.bytes = want_extract(text, self.starts, self.ends)
        assert self.starts.size > 600 > 2 * 256                       # several workgroups of the count kernel


def check_extract(dfm, want: Wanted, tag=""):
    off, got = dfm.extract_ranges(want.starts, want.ends)
    assert off.dtype == np.uint64 and got.dtype == np.uint8, tag
    assert np.array_equal(off, want.off) and np.array_equal(got, want.bytes), tag
    one = want.cond["whole"]                                          # a batch of one: the whole text
    off, got = dfm.extract_ranges(want.starts[one:one + 1], want.ends[one:one + 1])
    assert off.tolist() == [0, want.text.size] and np.array_equal(got, want.text), tag


def check_file(ctx, f: SufrFile, tag, samples=SAMPLES, tiles=TILES, kinds=("loaded", "wrapped", "wide")):
    text, sa = np.asarray(f.text).copy(), np.asarray(f.suffix_array).astype(np.int64)
    shapes = set()
    for q in samples:
        host = f.fm(q, text=True)
        info, tinfo = host.info, host.text_info
        want = Wanted(text, sa, q, info["block"], seed=q)
        h_off, h_bytes = host.extract_ranges(want.starts, want.ends)
        assert np.array_equal(h_off, want.off) and np.array_equal(h_bytes, want.bytes)           # host == the text; below device == both
        host.set_sequences([], [])
        for kind, ix, _ in indexes(ctx, f):
            if kind not in kinds:
                ix.close()
                continue
            for tile in tiles:
                ctx.set_bwt_tile(tile)
                dfm = ix.fm_device(q, text=True)
                di = dfm.info
                if ix.index_width == 4:
                    assert di == info and dfm.text_info == host.text_info, (tag, kind, tile, q)
                assert dfm.text_info["text_samples"] == tinfo["text_samples"] == (text.size + q - 1) // q
                assert dfm.text_info["text_bytes"] == tinfo["text_samples"] * ix.index_width
                shapes.add((di["block"], di["stride"], di["width"]))
                check_extract(dfm, want, (tag, kind, tile, q))
                dfm.close()
            ix.close()
        ctx.set_bwt_tile(0)
    return shapes


# ---------------------------------------------------------------------------------------------------------------------
# device against host
# ---------------------------------------------------------------------------------------------------------------------
def test_the_one_line_shape_on_the_golden_dna_file(ctx):
    """22 001 ranks: the whole text spans several workgroups of chunks at both sample rates (688 chunks at q == 32)"""
    f = SufrFile(EXP / "long_dna_sequence_allow_ambiguity.sufr")
    assert (f.text_len + 31) // 32 > 2 * 256
    shapes = check_file(ctx, f, "dna")
    assert shapes == {(96, 128, 4), (64, 128, 8)}                     # the one-line shape, and its 64-bit form, which the wide kernel takes


def test_a_wide_shape_on_the_golden_protein_file(ctx):
    """63 220 ranks, the largest small input: 1 976 chunks at q == 32, eight workgroups"""
    shapes = check_file(ctx, SufrFile(EXP / "uniprot.sufr"), "uniprot", tiles=(T,))
    assert (160, 256, 4) in shapes


@pytest.mark.parametrize("name", ["1n.sufr", "2ns.sufr", "abba.sufr"])
def test_the_short_golden_files(ctx, name):
    check_file(ctx, SufrFile(EXP / name), name, tiles=(T,), kinds=("loaded", "wide"))


def test_all_byte_values_at_both_widths(ctx, tmp_path):
    """K == 256: stride 2048 at w == 4 and 4096 at w == 8; the end byte is the largest byte value"""
    from test_bwt_host import write_arrays
    rng = np.random.default_rng(11)
    text = rng.integers(0, 255, 5000).astype(np.uint8)
    text[:255] = np.arange(255)
    text[-1] = 255
    f = write_arrays(tmp_path / "bytes.sufr", text, sorted_sa(text))
    shapes = check_file(ctx, f, "bytes", tiles=(T,), kinds=("wrapped", "wide"))
    assert shapes == {(1024, 2048, 4), (2048, 4096, 8)}


def test_a_run_and_a_fibonacci_string(ctx, oracle, tmp_path):
    for name, body in (("a", np.full(1000, ord("A"), dtype=np.uint8)), ("fib", fibonacci(3000))):
        f = oracle_file(oracle, tmp_path, body, name, is_dna=True, allow_ambiguity=True)
        assert f.len_suffixes == f.text_len == body.size + 1
        check_file(ctx, f, name, samples=(32, 7), tiles=(T,), kinds=("loaded", "wide"))


def test_capacity_refusals_and_the_empty_batch(ctx):
    f = SufrFile(EXP / "long_dna_sequence_allow_ambiguity.sufr")
    text = np.asarray(f.text).copy()
    ix = DeviceIndex.load(ctx, f)
    plain, dfm = ix.fm_device(32), ix.fm_device(32, text=True)
    with pytest.raises(SufrHipError) as err:
        ix.fm_device(0, text=True)
    assert err.value.code == INVALID
    ix.close()
    assert plain.text_info["text_samples"] == 0 and plain.info == dfm.info
    starts, ends, _ = request_set(text.size, 32, 96, None, seed=1, random=50)
    w_off, w_bytes = want_extract(text, starts, ends)
    z = int(w_off[-1])
    top = np.uint64(2**63 - 1)
    d_starts = torch.from_numpy(np.minimum(starts, top).astype(np.int64)).cuda()
    d_ends = torch.from_numpy(np.minimum(ends, top).astype(np.int64)).cuda()
    with pytest.raises(SufrHipError) as err:
        plain.extract_device(d_starts, d_ends)
    assert err.value.code == UNSUPPORTED
    with pytest.raises(SufrHipError) as err:
        dfm.extract_device(d_starts, d_ends, cap=z - 1)
    assert err.value.code == CAPACITY and err.value.total == z
    off, got = dfm.extract_device(d_starts, d_ends, cap=z)
    assert np.array_equal(_unsigned(off), w_off) and np.array_equal(got.cpu().numpy(), w_bytes)
    off, got = dfm.extract_device(d_starts, d_ends, cap=z + 100)      # room to spare
    assert np.array_equal(_unsigned(off), w_off) and np.array_equal(got.cpu().numpy(), w_bytes)
    none = torch.zeros(0, dtype=torch.int64, device="cuda")
    off, got = dfm.extract_device(none, none)
    assert off.cpu().tolist() == [0] and got.numel() == 0
    assert dfm.extract(5, 25) == text[5:25].tobytes() and dfm.extract(text.size - 1, 2**64 - 1) == text[-1:].tobytes()
    # the host-pointer twin
    import ctypes as C
    L = sufr_amd.lib()
    h_off, h_out, total = np.full(starts.size + 1, 7, dtype=np.uint64), np.full(z + 9, 0xAA, dtype=np.uint8), C.c_uint64(0)
    args = (ctx.handle, dfm._h, starts.ctypes.data, ends.ctypes.data, starts.size, h_off.ctypes.data, h_out.ctypes.data)
    assert L.sufr_hip_fm_extract_batch(*args, z - 1, C.byref(total)) == CAPACITY and total.value == z and (h_out == 0xAA).all()
    assert np.array_equal(h_off, w_off)
    assert L.sufr_hip_fm_extract_batch(*args, z, C.byref(total)) == 0 and total.value == z
    assert np.array_equal(h_out[:z], w_bytes) and (h_out[z:] == 0xAA).all() and np.array_equal(h_off, w_off)
    assert L.sufr_hip_fm_extract_batch(ctx.handle, dfm._h, None, None, 0, h_off.ctypes.data, None, 0, C.byref(total)) == 0 and h_off[0] == 0


def test_the_index_answers_after_its_arrays_are_gone(ctx):
    f = SufrFile(EXP / "uniprot.sufr")
    text, sa = np.asarray(f.text).copy(), np.asarray(f.suffix_array).astype(np.int64)
    want = Wanted(text, sa, 32, 160, seed=9)
    d_text = torch.from_numpy(text).cuda()
    d_sa = torch.from_numpy(sa.astype(np.uint32).view(np.int32).copy()).cuda()
    ix = DeviceIndex.wrap(ctx, d_text, d_sa, prefix_table=False)
    dfm = ix.fm_device(32, text=True)
    ix.close()
    d_text.zero_(); d_sa.zero_()
    torch.cuda.synchronize()
    del d_text, d_sa
    torch.cuda.empty_cache()
    check_extract(dfm, want, "gone")


def test_two_calls_and_two_contexts_on_two_threads():
    f = SufrFile(EXP / "long_dna_sequence_allow_ambiguity.sufr")
    text, sa = np.asarray(f.text).copy(), np.asarray(f.suffix_array).astype(np.int64)
    want = Wanted(text, sa, 32, 96, seed=4)
    results, errors = {}, []

    def work(k):
        try:
            c = sufr_amd.Context(0)
            ix = DeviceIndex.load(c, f)
            dfm = ix.fm_device(32, text=True)
            ix.close()
            a = dfm.extract_ranges(want.starts, want.ends)
            b = dfm.extract_ranges(want.starts, want.ends)
            results[k] = (a, b)
            dfm.close()
            c.close()
        except Exception as e:                                        # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(2):
        (o1, b1), (o2, b2) = results[k]
        assert np.array_equal(o1, o2) and np.array_equal(b1, b2)      # two calls: the same bytes
        assert np.array_equal(o1, want.off) and np.array_equal(b1, want.bytes)


# ---------------------------------------------------------------------------------------------------------------------
# the copies and the file
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,q,text_on", [("long_dna_sequence_allow_ambiguity.sufr", 32, True), ("uniprot.sufr", 7, True), ("2ns.sufr", 2, True),
                                            ("long_dna_sequence_allow_ambiguity.sufr", 5, False), ("uniprot.sufr", 0, False)])
def test_a_downloaded_device_build_is_the_file_of_the_host_build(ctx, tmp_path, name, q, text_on):
    f = SufrFile(EXP / name)
    host = f.fm(q, text=text_on)
    host.set_sequences([], [])                                        # saved without names
    host.save(tmp_path / "host.fm")
    for tile in TILES:
        ctx.set_bwt_tile(tile)
        ix = DeviceIndex.load(ctx, f)
        dfm = ix.fm_device(q, text=text_on)
        ix.close()
        down = dfm.to_host()
        assert down.sequences() == ([], [])
        down.save(tmp_path / "down.fm")
        assert (tmp_path / "down.fm").read_bytes() == (tmp_path / "host.fm").read_bytes(), (name, tile)
        up = host.to_device(ctx)                                      # the four routes agree on info and text_info
        infos = [(x.info, x.text_info) for x in (host, dfm, down, up)]
        assert infos[0] == infos[1] == infos[2] == infos[3], infos
        assert infos[0][1]["file_bytes"] == (tmp_path / "host.fm").stat().st_size
        up.close(); dfm.close()
    ctx.set_bwt_tile(0)


CHILD = r"""
import sys
import numpy as np
import sufr_amd
from sufr_amd import FmIndex, pack_queries

def refuse(*a, **k):
    raise AssertionError("a DeviceIndex was created")
sufr_amd.DeviceIndex.__init__ = refuse
sufr_amd.DeviceIndex.load = refuse
sufr_amd.DeviceIndex.wrap = refuse
index, queries, requests, out = sys.argv[1:5]
ctx = sufr_amd.Context(0)
dfm = FmIndex.load(index).to_device(ctx)
qs = [bytes.fromhex(line) for line in open(queries).read().split("\n")]
lo, hi = dfm.search(qs)
located = dfm.locate(qs, 4)
short = [q[:20] for q in qs if len(q) >= 3][:30]
hits = dfm.approx(short, 2)
req = np.load(requests)
off, got = dfm.extract_ranges(req[0], req[1])
np.savez(out, lo=lo, hi=hi, pos=np.concatenate([p.astype(np.uint64) for p in located]), cnt=np.array([len(p) for p in located]),
         approx=np.array([(i, h.position, h.mismatches) for i, hs in enumerate(hits) for h in hs], dtype=np.int64).reshape(-1, 3),
         off=off, bytes=got, info=np.array(sorted(dfm.info.items()), dtype=object), allow_pickle=True)
dfm.close()
ctx.close()
"""


def test_a_loaded_file_on_the_device_answers_like_the_device_build(ctx, tmp_path):
    """the file of a host build, loaded and uploaded by a process that never creates a DeviceIndex (a child of this one), answers
    search, locate, approx and extract like the index built on the device from the resident text and suffix array"""
    f = SufrFile(EXP / "uniprot.sufr")
    w = Witness(np.asarray(f.text).copy(), np.asarray(f.suffix_array))
    f.fm(32, text=True).save(tmp_path / "u.fm")
    qs = [q for q in query_set(w, 160, seed=6)]
    starts, ends, _ = request_set(w.n, 32, 160, None, seed=2, random=200)
    (tmp_path / "q.txt").write_text("\n".join(q.hex() for q in qs))
    np.save(tmp_path / "r.npy", np.stack([np.minimum(starts, np.uint64(2**62)), np.minimum(ends, np.uint64(2**62))]))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(ROOT), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path / "u.fm"), str(tmp_path / "q.txt"), str(tmp_path / "r.npy"), str(tmp_path / "out.npz")],
                       capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.load(tmp_path / "out.npz", allow_pickle=True)
    ix = DeviceIndex.load(ctx, f)
    dfm = ix.fm_device(32, text=True)
    ix.close()
    lo, hi = dfm.search(qs)
    located = dfm.locate(qs, 4)
    short = [q[:20] for q in qs if len(q) >= 3][:30]
    hits = dfm.approx(short, 2)
    off, data = dfm.extract_ranges(starts, ends)
    assert np.array_equal(got["lo"], lo) and np.array_equal(got["hi"], hi) and int((hi > lo).sum()) > 10
    assert np.array_equal(got["cnt"], [len(p) for p in located]) and np.array_equal(got["pos"], np.concatenate([p.astype(np.uint64) for p in located]))
    want_hits = np.array([(i, h.position, h.mismatches) for i, hs in enumerate(hits) for h in hs], dtype=np.int64).reshape(-1, 3)
    assert np.array_equal(got["approx"], want_hits) and want_hits.shape[0] > 20
    assert np.array_equal(got["off"], off) and np.array_equal(got["bytes"], data) and data.size > 1000
    assert dict(got["info"].tolist()) == dfm.info


def test_cli_saves_on_the_device_and_answers_from_the_index_on_the_device(tmp_path):
    """`sufr fm --save --device` writes the file of the host build, and `sufr fm --index --device` prints the lines of locate,
    approx and extract with no .sufr opened"""
    import shutil
    from test_match_host import run
    name = "long_dna_sequence_allow_ambiguity.sufr"
    src = tmp_path / name
    shutil.copy(EXP / name, src)
    raw = SufrFile(src).text.tobytes()
    queries = ["ACGT", "GATTACA", "N", "TTTTTTTTTTTTTTTTTTTTTTTTTT", "AC"]
    near = [raw[100:114].decode(), raw[5000:5007].decode() + "A" + raw[5008:5016].decode()]
    want = {"count": run("count", src, *queries), "locate": run("locate", src, *queries), "approx": run("approx", "-d", 1, src, *near),
            "extract": run("extract", "-p", 3, "-s", 11, src, "GATTACA", "ACGTT", "NNN")}
    host, dev = tmp_path / "host.fm", tmp_path / "dev.fm"
    run("fm", src, "--save", host, "--text", "-s", 32)
    run("fm", src, "--save", dev, "--text", "-s", 32, "--device", 0)
    assert dev.read_bytes() == host.read_bytes()
    from_sufr = run("fm", "--extract", "--prefix-len", 3, "--suffix-len", 11, "--device", 0, src, "GATTACA", "ACGTT", "NNN")
    assert from_sufr.stdout == want["extract"].stdout != "" and from_sufr.stderr == want["extract"].stderr
    src.write_bytes(b"")
    assert run("fm", "--index", dev, "--device", 0, *queries).stdout == want["count"].stdout != ""
    got = run("fm", "--index", dev, "--locate", "--device", 0, *queries)
    assert got.stdout == want["locate"].stdout != "" and got.stderr == want["locate"].stderr
    got = run("fm", "--index", dev, "--mismatches", 1, "--device", 0, *near)
    assert sorted(got.stdout.splitlines()) == sorted(want["approx"].stdout.splitlines()) and got.stdout
    got = run("fm", "--index", dev, "--extract", "--prefix-len", 3, "--suffix-len", 11, "--device", 0, "GATTACA", "ACGTT", "NNN")
    assert got.stdout == want["extract"].stdout and got.stderr == want["extract"].stderr
