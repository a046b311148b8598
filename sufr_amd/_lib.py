"""ctypes binding of libsufr_hip.so (include/sufr_hip.h).  No CPU fallback: if the HIP library is
missing or no GPU is visible, every build entry point raises."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

CSRC = Path(__file__).resolve().parent / "csrc"
LIB_PATH = CSRC / "_build" / "libsufr_hip.so"
# profiles/*.sh may point the binding at the probes build (tuning knobs from SUFR_PROBE_*, phase stamps); the tests and
# the driver use the plain library, which reads no environment besides SUFR_HIP_DEBUG and SUFR_SERIAL_READER.  The
# switch is loud: a stray variable must not change a user's kernels silently.
if os.environ.get("SUFR_AMD_PROBES_LIB"):
    import sys as _sys
    LIB_PATH = CSRC / "_build" / "libsufr_hip_probes.so"
    print(f"sufr_amd: SUFR_AMD_PROBES_LIB is set -- loading the PROBES build {LIB_PATH.name} (tuning knobs from "
          "SUFR_PROBE_*; for profiling only)", file=_sys.stderr)
CLI_PATH = CSRC / "_build" / "sufr"
# tests/test_sanitized_host.py runs the host-side tests in a child process against the HOST-ONLY AddressSanitizer + UBSan
# build (`make asan`: reader, writer, query code; every device entry point answers "no device").  Loud, like the probes switch.
HOST_ASAN = bool(os.environ.get("SUFR_AMD_HOST_ASAN_LIB"))
if HOST_ASAN:
    import sys as _sys
    LIB_PATH = CSRC / "_build" / "libsufr_host_asan.so"
    CLI_PATH = CSRC / "_build" / "sufr_host_asan"
    print(f"sufr_amd: SUFR_AMD_HOST_ASAN_LIB is set -- loading the host-only sanitizer build {LIB_PATH.name} (no device code)",
          file=_sys.stderr)


class SufrHipError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"{message} (sufr_hip error {code})")
        self.code = code
        self.message = message


class Stats(C.Structure):
    """sufr_hip_stats"""
    _fields_ = [
        ("text_len", C.c_uint64), ("num_suffixes", C.c_uint64),
        ("alphabet_size", C.c_uint32), ("bits_per_char", C.c_uint32), ("chars_per_key", C.c_uint32),
        ("digit_bits", C.c_uint32), ("num_passes", C.c_uint32), ("num_levels", C.c_uint32),
        ("num_large_groups", C.c_uint64), ("deep_records", C.c_uint64),
        ("top_lo", C.c_uint32), ("top_hi", C.c_uint32), ("partition_workgroups", C.c_uint32),
        ("partition_variant", C.c_uint32),
        ("ms_total", C.c_float), ("ms_normalize", C.c_float), ("ms_hist_text", C.c_float),
        ("ms_partition", C.c_float), ("ms_passes", C.c_float), ("ms_finish", C.c_float),
        ("ms_deep", C.c_float), ("host_read_s", C.c_float), ("host_build_s", C.c_float),
        ("host_write_s", C.c_float),
        ("num_exceptions", C.c_uint32), ("ms_exceptions", C.c_float), ("num_reinserted", C.c_uint64),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class SequenceData(C.Structure):
    _fields_ = [("seq", C.POINTER(C.c_uint8)), ("seq_len", C.c_uint64),
                ("start_positions", C.POINTER(C.c_uint64)), ("sequence_names", C.POINTER(C.c_char_p)),
                ("num_sequences", C.c_uint64)]


class CreateArgs(C.Structure):
    _fields_ = [("input", C.c_char_p), ("output", C.c_char_p), ("num_partitions", C.c_uint64),
                ("has_max_query_len", C.c_int), ("max_query_len", C.c_uint64), ("is_dna", C.c_int),
                ("allow_ambiguity", C.c_int), ("ignore_softmask", C.c_int), ("sequence_delimiter", C.c_uint8),
                ("seed_mask", C.c_char_p), ("random_seed", C.c_uint64)]


class ShardInfo(C.Structure):
    _fields_ = [("num_suffixes", C.c_uint64), ("first_suffix", C.c_uint64), ("last_suffix", C.c_uint64)]


FLAG_DNA, FLAG_ALLOW_AMBIGUITY, FLAG_IGNORE_SOFTMASK, FLAG_RAW_TEXT = 1, 2, 4, 8
FLAG_NO_PREFIX_TABLE = 0x100      # sufr_hip_index_wrap only
FLAG_SA_U64 = 0x200               # sufr_hip_index_wrap only: 64-bit suffix array of a text below 2^32 - 1 bytes

# every symbol include/sufr_hip.h declares
EXPORTS = [
    "sufr_hip_abi_version", "sufr_hip_device_count", "sufr_hip_create", "sufr_hip_destroy",
    "sufr_hip_last_error", "sufr_hip_set_stream", "sufr_hip_synchronize", "sufr_hip_set_window", "sufr_hip_set_window_retry", "sufr_hip_set_array_budget", "sufr_hip_window_repairs", "sufr_hip_set_overlap_min", "sufr_hip_overlapped", "sufr_hip_doublings", "sufr_hip_set_pair_walk", "sufr_hip_pairs_walked", "sufr_hip_set_exc_max_affected", "sufr_hip_exc_retry", "sufr_hip_exc_taken", "sufr_hip_normalize", "sufr_hip_sort_device_u32",
    "sufr_hip_sort_device_u64", "sufr_hip_stitch_device_u32", "sufr_hip_stitch_device_u64", "sufr_hip_build_u32", "sufr_hip_build_u64", "sufr_hip_lcp_pair",
    "sufr_read_sequence_file", "sufr_sequence_data_free", "sufr_write_file", "sufr_hip_create_file", "sufr_hip_create_from_sequence",
    "sufr_hip_shard_build", "sufr_write_frame", "sufr_hip_shard_write", "sufr_hip_create_from_sequence_multi",
    "sufr_hip_create_file_multi",
]
# every symbol include/sufr_query.h declares
QUERY_EXPORTS = [
    "sufr_file_open", "sufr_file_close", "sufr_file_metadata", "sufr_file_text", "sufr_file_seed_mask",
    "sufr_file_suffix_array", "sufr_file_lcp_array", "sufr_file_suffix", "sufr_file_lcp", "sufr_file_sequence_start",
    "sufr_file_sequence_name", "sufr_file_sequence_of", "sufr_file_search", "sufr_file_search_batch",
    "sufr_hip_index_load", "sufr_hip_index_wrap", "sufr_hip_index_free", "sufr_hip_index_width", "sufr_hip_search_batch",
    "sufr_hip_search_batch_device", "sufr_hip_locate_batch_device",
]
# every symbol include/sufr_match.h declares
MATCH_EXPORTS = [
    "sufr_file_matching_stats", "sufr_file_smems", "sufr_hip_matching_stats_device", "sufr_hip_smems_device", "sufr_hip_smems",
]
# every symbol include/sufr_mem.h declares
MEM_EXPORTS = ["sufr_file_mems", "sufr_hip_mems_device", "sufr_hip_mems"]
MEM_BOTH_STRANDS = 0x1
# every symbol include/sufr_approx.h declares
APPROX_EXPORTS = ["sufr_file_approx", "sufr_hip_approx_device", "sufr_hip_approx"]
APPROX_BOTH_STRANDS = 0x1
# every symbol include/sufr_edit.h declares
EDIT_EXPORTS = ["sufr_file_edit", "sufr_hip_edit_device", "sufr_hip_edit"]
EDIT_BOTH_STRANDS = 0x1
EDIT_LOCAL_MINIMA = 0x2
# every symbol include/sufr_align.h declares
ALIGN_EXPORTS = ["sufr_file_edit_trace", "sufr_hip_edit_trace_device", "sufr_hip_edit_trace", "sufr_hip_set_trace_scratch"]
# every symbol include/sufr_kmer.h declares
KMER_EXPORTS = ["sufr_file_kmers", "sufr_file_unique_lengths", "sufr_hip_kmers_device", "sufr_hip_unique_lengths_device",
                "sufr_hip_set_kmer_tile"]
KMER_BY_POSITION = 0x1


class KmerStats(C.Structure):
    """sufr_kmer_stats"""
    _fields_ = [("whole", C.c_uint64), ("distinct", C.c_uint64), ("unique", C.c_uint64), ("max_count", C.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


# every symbol include/sufr_repeat.h declares
REPEAT_EXPORTS = ["sufr_file_repeats", "sufr_hip_repeats_device", "sufr_hip_set_repeat_tile"]
REPEAT_KINDS = {"branching": 0, "maximal": 1, "super": 2, "supermaximal": 2}


class RepeatStats(C.Structure):
    """sufr_repeat_stats"""
    _fields_ = [("records", C.c_uint64), ("longest", C.c_uint64), ("longest_rank", C.c_uint64), ("max_count", C.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


# every symbol include/sufr_lz.h declares
LZ_EXPORTS = ["sufr_file_lpf", "sufr_file_lz", "sufr_hip_lpf_device", "sufr_hip_lz_device", "sufr_hip_set_lz_tile"]


class LzStats(C.Structure):
    """sufr_lz_stats"""
    _fields_ = [("factors", C.c_uint64), ("literals", C.c_uint64), ("longest", C.c_uint64), ("longest_start", C.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


# every symbol include/sufr_shared.h declares
SHARED_EXPORTS = ["sufr_file_shared", "sufr_file_common", "sufr_hip_shared_device", "sufr_hip_common_device"]


class SharedStats(C.Structure):
    """sufr_shared_stats"""
    _fields_ = [("records", C.c_uint64), ("longest", C.c_uint64), ("longest_rank", C.c_uint64), ("max_count", C.c_uint64),
                ("max_seqs", C.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


# every symbol include/sufr_bwt.h declares
BWT_EXPORTS = ["sufr_file_bwt", "sufr_file_bwt_runs", "sufr_file_lf", "sufr_hip_bwt_device", "sufr_hip_bwt_runs_device", "sufr_hip_lf_device",
               "sufr_hip_set_bwt_tile"]


class BwtStats(C.Structure):
    """sufr_bwt_stats"""
    _fields_ = [("runs", C.c_uint64), ("records", C.c_uint64), ("longest", C.c_uint64), ("longest_rank", C.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


# every symbol include/sufr_fm.h declares
FM_EXPORTS = ["sufr_file_fm_build", "sufr_fm_free", "sufr_fm_get_info", "sufr_fm_search_batch", "sufr_fm_locate_batch", "sufr_hip_fm_build",
              "sufr_hip_fm_free", "sufr_hip_fm_get_info", "sufr_hip_fm_search_batch_device", "sufr_hip_fm_locate_batch_device"]
# every symbol include/sufr_fm_approx.h declares
FM_APPROX_EXPORTS = ["sufr_fm_approx", "sufr_fm_approx_steps", "sufr_hip_fm_approx_device", "sufr_hip_fm_approx"]
FM_APPROX_BOTH_STRANDS = 0x1
FM_APPROX_MAX_MISMATCHES = 3


# every symbol include/sufr_fm_text.h declares
FM_TEXT_EXPORTS = ["sufr_file_fm_build_flags", "sufr_fm_get_text_info", "sufr_fm_extract_batch", "sufr_fm_save", "sufr_fm_load",
                   "sufr_fm_num_sequences", "sufr_fm_sequence_start", "sufr_fm_sequence_name", "sufr_fm_set_sequences",
                   "sufr_hip_fm_build_flags", "sufr_hip_fm_get_text_info", "sufr_hip_fm_extract_batch_device", "sufr_hip_fm_extract_batch",
                   "sufr_hip_fm_upload", "sufr_hip_fm_download"]
FM_TEXT = 0x1
# every symbol include/sufr_fm_match.h declares
FM_MATCH_EXPORTS = ["sufr_fm_pair_check", "sufr_fm_matching_stats", "sufr_fm_smems", "sufr_fm_matching_stats_steps",
                    "sufr_file_write_reversed_fasta", "sufr_hip_fm_matching_stats_device", "sufr_hip_fm_smems_device", "sufr_hip_fm_smems"]


class FmTextInfo(C.Structure):
    """sufr_fm_text_info"""
    _fields_ = [("text_samples", C.c_uint64), ("text_bytes", C.c_uint64), ("file_bytes", C.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class FmInfo(C.Structure):
    """sufr_fm_info"""
    _fields_ = [("ranks", C.c_uint64), ("symbols", C.c_uint64), ("block", C.c_uint64), ("stride", C.c_uint64), ("sample", C.c_uint64),
                ("samples", C.c_uint64), ("bytes", C.c_uint64), ("width", C.c_uint32), ("end_byte", C.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class FileMeta(C.Structure):
    """sufr_file_meta"""
    _fields_ = [("version", C.c_uint8), ("is_dna", C.c_uint8), ("allow_ambiguity", C.c_uint8),
                ("ignore_softmask", C.c_uint8), ("index_width", C.c_int),
                ("text_len", C.c_uint64), ("text_pos", C.c_uint64), ("suffix_array_pos", C.c_uint64),
                ("lcp_pos", C.c_uint64), ("len_suffixes", C.c_uint64), ("max_query_len", C.c_uint64),
                ("num_sequences", C.c_uint64), ("seed_mask_len", C.c_uint64), ("file_size", C.c_uint64),
                ("modified", C.c_int64)]

_lib = None


def build_extension(verbose: bool = False) -> Path:
    """Compile the HIP library and the CLI for gfx950 (hipcc cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", str(CSRC)] + (["asan"] if HOST_ASAN else []), capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("building libsufr_hip.so failed:\n" + r.stdout + r.stderr)
    if verbose:
        print(r.stdout)
    return LIB_PATH


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise SufrHipError(-2, f"{LIB_PATH} is missing: build it with sufr_amd.build_extension() "
                               "(there is no CPU fallback)")
    # PyTorch wheels bundle their own HIP runtime; a process that loads this library first (/opt/rocm's runtime) and
    # torch afterwards ends up with two runtimes, and the second one to initialise finds no device.  Whoever uses the
    # Python binding next to torch gets torch's runtime for both: import it first when it is installed.
    import sys
    if "torch" not in sys.modules and not HOST_ASAN:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(str(LIB_PATH))
    vp, u64, u32, cp = C.c_void_p, C.c_uint64, C.c_uint32, C.c_char_p
    L.sufr_hip_abi_version.restype = C.c_int
    L.sufr_hip_device_count.restype = C.c_int
    L.sufr_hip_create.argtypes = [C.c_int]; L.sufr_hip_create.restype = vp
    L.sufr_hip_destroy.argtypes = [vp]; L.sufr_hip_destroy.restype = None
    L.sufr_hip_last_error.argtypes = [vp]; L.sufr_hip_last_error.restype = cp
    L.sufr_hip_set_stream.argtypes = [vp, vp]; L.sufr_hip_set_stream.restype = C.c_int
    L.sufr_hip_synchronize.argtypes = [vp]; L.sufr_hip_synchronize.restype = C.c_int
    L.sufr_hip_set_window.argtypes = [vp, u64, u64]; L.sufr_hip_set_window.restype = C.c_int
    L.sufr_hip_set_window_retry.argtypes = [vp, u64]; L.sufr_hip_set_window_retry.restype = C.c_int
    L.sufr_hip_set_array_budget.argtypes = [vp, u64]; L.sufr_hip_set_array_budget.restype = C.c_int
    L.sufr_hip_window_repairs.argtypes = [vp]; L.sufr_hip_window_repairs.restype = u64
    L.sufr_hip_set_overlap_min.argtypes = [vp, u64]; L.sufr_hip_set_overlap_min.restype = C.c_int
    L.sufr_hip_overlapped.argtypes = [vp]; L.sufr_hip_overlapped.restype = C.c_int
    L.sufr_hip_doublings.argtypes = [vp]; L.sufr_hip_doublings.restype = u64
    L.sufr_hip_set_pair_walk.argtypes = [vp, C.c_uint32]; L.sufr_hip_set_pair_walk.restype = C.c_int
    L.sufr_hip_pairs_walked.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]; L.sufr_hip_pairs_walked.restype = C.c_int
    L.sufr_hip_set_exc_max_affected.argtypes = [vp, u64]; L.sufr_hip_set_exc_max_affected.restype = C.c_int
    L.sufr_hip_exc_retry.argtypes = [vp]; L.sufr_hip_exc_retry.restype = C.c_int
    L.sufr_hip_exc_taken.argtypes = [vp]; L.sufr_hip_exc_taken.restype = u64
    L.sufr_hip_normalize.argtypes = [vp, vp, u64, C.c_int]; L.sufr_hip_normalize.restype = C.c_int
    dev_sig = [vp, vp, u64, u32, u64, cp, u64, u64, u32, u32, vp, vp, u64, C.POINTER(u64), C.POINTER(Stats)]
    L.sufr_hip_sort_device_u32.argtypes = dev_sig; L.sufr_hip_sort_device_u32.restype = C.c_int
    L.sufr_hip_sort_device_u64.argtypes = dev_sig; L.sufr_hip_sort_device_u64.restype = C.c_int
    host_sig = [vp, vp, u64, u32, u64, cp, u64, u64, vp, vp, vp, u64, C.POINTER(u64), C.POINTER(Stats)]
    L.sufr_hip_build_u32.argtypes = host_sig; L.sufr_hip_build_u32.restype = C.c_int
    L.sufr_hip_build_u64.argtypes = host_sig; L.sufr_hip_build_u64.restype = C.c_int
    L.sufr_hip_lcp_pair.argtypes = [vp, u64, u64, u64]; L.sufr_hip_lcp_pair.restype = u64
    L.sufr_hip_stitch_device_u32.argtypes = [vp, u64, vp, u32, u32, vp]; L.sufr_hip_stitch_device_u32.restype = C.c_int
    L.sufr_hip_stitch_device_u64.argtypes = [vp, u64, vp, u32, u32, vp]; L.sufr_hip_stitch_device_u64.restype = C.c_int
    L.sufr_read_sequence_file.argtypes = [cp, C.c_uint8, C.POINTER(SequenceData), cp, C.c_size_t]
    L.sufr_read_sequence_file.restype = C.c_int
    L.sufr_sequence_data_free.argtypes = [C.POINTER(SequenceData)]; L.sufr_sequence_data_free.restype = None
    L.sufr_write_file.argtypes = [cp, C.c_int, C.c_int, C.c_int, vp, u64, C.c_int, vp, vp, u64, C.c_int, u64, cp,
                                  vp, u64, C.POINTER(cp), cp, C.c_size_t]
    L.sufr_write_file.restype = C.c_int
    L.sufr_hip_create_file.argtypes = [vp, C.POINTER(CreateArgs), cp, C.c_size_t, C.POINTER(Stats)]
    L.sufr_hip_create_file.restype = C.c_int
    L.sufr_hip_create_from_sequence.argtypes = [vp, C.POINTER(SequenceData), C.POINTER(CreateArgs), cp, C.c_size_t,
                                                C.POINTER(Stats)]
    L.sufr_hip_create_from_sequence.restype = C.c_int
    L.sufr_hip_shard_build.argtypes = [vp, C.POINTER(SequenceData), C.POINTER(CreateArgs), u32, u32,
                                       C.POINTER(ShardInfo), C.POINTER(Stats)]
    L.sufr_hip_shard_build.restype = C.c_int
    L.sufr_write_frame.argtypes = [cp, C.POINTER(SequenceData), C.POINTER(CreateArgs), u64, cp, C.c_size_t]
    L.sufr_write_frame.restype = C.c_int
    L.sufr_hip_shard_write.argtypes = [vp, C.POINTER(SequenceData), C.POINTER(CreateArgs), cp, u64, u64, u64, C.c_int,
                                       u64, C.c_int]
    L.sufr_hip_shard_write.restype = C.c_int
    L.sufr_hip_create_from_sequence_multi.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(SequenceData),
                                                      C.POINTER(CreateArgs), cp, C.c_size_t, C.POINTER(Stats)]
    L.sufr_hip_create_from_sequence_multi.restype = C.c_int
    L.sufr_hip_create_file_multi.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(CreateArgs), cp, C.c_size_t,
                                             C.POINTER(Stats)]
    L.sufr_hip_create_file_multi.restype = C.c_int
    # include/sufr_query.h
    L.sufr_file_open.argtypes = [cp, C.POINTER(vp), cp, C.c_size_t]; L.sufr_file_open.restype = C.c_int
    L.sufr_file_close.argtypes = [vp]; L.sufr_file_close.restype = None
    L.sufr_file_metadata.argtypes = [vp, C.POINTER(FileMeta)]; L.sufr_file_metadata.restype = C.c_int
    for name in ("sufr_file_text", "sufr_file_seed_mask", "sufr_file_suffix_array", "sufr_file_lcp_array"):
        getattr(L, name).argtypes = [vp]; getattr(L, name).restype = vp
    for name in ("sufr_file_suffix", "sufr_file_lcp", "sufr_file_sequence_start", "sufr_file_sequence_of"):
        getattr(L, name).argtypes = [vp, u64]; getattr(L, name).restype = u64
    L.sufr_file_sequence_name.argtypes = [vp, u64]; L.sufr_file_sequence_name.restype = cp
    L.sufr_file_search.argtypes = [vp, cp, C.c_size_t, C.c_int, u64, C.POINTER(u64), C.POINTER(u64)]
    L.sufr_file_search.restype = C.c_int
    L.sufr_file_search_batch.argtypes = [vp, vp, vp, u64, C.c_int, u64, vp, vp, C.c_int]; L.sufr_file_search_batch.restype = C.c_int
    L.sufr_hip_index_load.argtypes = [vp, vp, C.POINTER(vp)]; L.sufr_hip_index_load.restype = C.c_int
    L.sufr_hip_index_wrap.argtypes = [vp, vp, u64, vp, u64, u32, u64, cp, C.POINTER(vp)]; L.sufr_hip_index_wrap.restype = C.c_int
    L.sufr_hip_index_free.argtypes = [vp]; L.sufr_hip_index_free.restype = None
    L.sufr_hip_index_width.argtypes = [vp]; L.sufr_hip_index_width.restype = C.c_int
    L.sufr_hip_search_batch.argtypes = [vp, vp, vp, vp, u64, C.c_int, u64, vp, vp]; L.sufr_hip_search_batch.restype = C.c_int
    L.sufr_hip_search_batch_device.argtypes = [vp, vp, vp, vp, u64, C.c_int, u64, vp, vp]
    L.sufr_hip_search_batch_device.restype = C.c_int
    L.sufr_hip_locate_batch_device.argtypes = [vp, vp, vp, vp, u64, u64, vp, vp, u64, C.POINTER(u64)]
    L.sufr_hip_locate_batch_device.restype = C.c_int
    # include/sufr_match.h
    L.sufr_file_matching_stats.argtypes = [vp, vp, vp, u64, vp, C.c_int]; L.sufr_file_matching_stats.restype = C.c_int
    L.sufr_file_smems.argtypes = [vp, vp, vp, u64, u32, u64, vp, vp, vp, vp, vp, C.POINTER(u64), C.c_int]
    L.sufr_file_smems.restype = C.c_int
    L.sufr_hip_matching_stats_device.argtypes = [vp, vp, vp, vp, u64, vp]; L.sufr_hip_matching_stats_device.restype = C.c_int
    L.sufr_hip_smems_device.argtypes = [vp, vp, vp, vp, u64, u32, vp, u64, vp, vp, vp, vp, vp, C.POINTER(u64)]
    L.sufr_hip_smems_device.restype = C.c_int
    L.sufr_hip_smems.argtypes = [vp, vp, vp, vp, u64, u32, u64, vp, vp, vp, vp, vp, C.POINTER(u64)]
    L.sufr_hip_smems.restype = C.c_int
    # include/sufr_mem.h
    L.sufr_file_mems.argtypes = [vp, vp, vp, u64, u32, u64, u32, u64, vp, vp, vp, vp, vp, C.POINTER(u64), C.c_int]
    L.sufr_file_mems.restype = C.c_int
    L.sufr_hip_mems_device.argtypes = [vp, vp, vp, vp, u64, u32, u64, u32, u64, vp, vp, vp, vp, vp, C.POINTER(u64)]
    L.sufr_hip_mems_device.restype = C.c_int
    L.sufr_hip_mems.argtypes = [vp, vp, vp, vp, u64, u32, u64, u32, u64, vp, vp, vp, vp, vp, C.POINTER(u64)]
    L.sufr_hip_mems.restype = C.c_int
    # include/sufr_approx.h
    L.sufr_file_approx.argtypes = [vp, vp, vp, u64, u32, u64, u32, u64, vp, vp, vp, vp, C.POINTER(u64), C.c_int]
    L.sufr_file_approx.restype = C.c_int
    L.sufr_hip_approx_device.argtypes = [vp, vp, vp, vp, u64, u32, u64, u32, u64, vp, vp, vp, vp, C.POINTER(u64)]
    L.sufr_hip_approx_device.restype = C.c_int
    L.sufr_hip_approx.argtypes = [vp, vp, vp, vp, u64, u32, u64, u32, u64, vp, vp, vp, vp, C.POINTER(u64)]
    L.sufr_hip_approx.restype = C.c_int
    # include/sufr_edit.h
    L.sufr_file_edit.argtypes = [vp, vp, vp, u64, u32, u64, u32, u64, vp, vp, vp, vp, C.POINTER(u64), C.c_int]
    L.sufr_file_edit.restype = C.c_int
    L.sufr_hip_edit_device.argtypes = [vp, vp, vp, vp, u64, u32, u64, u32, u64, vp, vp, vp, vp, C.POINTER(u64)]
    L.sufr_hip_edit_device.restype = C.c_int
    L.sufr_hip_edit.argtypes = [vp, vp, vp, vp, u64, u32, u64, u32, u64, vp, vp, vp, vp, C.POINTER(u64)]
    L.sufr_hip_edit.restype = C.c_int
    # include/sufr_align.h
    L.sufr_file_edit_trace.argtypes = [vp, vp, vp, u64, u64, vp, vp, vp, vp, u64, vp, vp, vp, C.POINTER(u64), C.c_int, cp, C.c_size_t]
    L.sufr_file_edit_trace.restype = C.c_int
    L.sufr_hip_edit_trace_device.argtypes = [vp, vp, vp, vp, u64, u64, vp, vp, vp, vp, u64, vp, vp, vp, C.POINTER(u64)]
    L.sufr_hip_edit_trace_device.restype = C.c_int
    L.sufr_hip_edit_trace.argtypes = [vp, vp, vp, vp, u64, u64, vp, vp, vp, vp, u64, vp, vp, vp, C.POINTER(u64)]
    L.sufr_hip_edit_trace.restype = C.c_int
    L.sufr_hip_set_trace_scratch.argtypes = [vp, u64]; L.sufr_hip_set_trace_scratch.restype = C.c_int
    # include/sufr_kmer.h
    L.sufr_file_kmers.argtypes = [vp, u64, u32, u64, vp, vp, C.POINTER(KmerStats), C.c_int]; L.sufr_file_kmers.restype = C.c_int
    L.sufr_file_unique_lengths.argtypes = [vp, u32, vp, C.c_int]; L.sufr_file_unique_lengths.restype = C.c_int
    L.sufr_hip_kmers_device.argtypes = [vp, vp, vp, vp, u64, u64, u32, u64, vp, vp, C.POINTER(KmerStats)]
    L.sufr_hip_kmers_device.restype = C.c_int
    L.sufr_hip_unique_lengths_device.argtypes = [vp, vp, vp, vp, u64, u32, vp]; L.sufr_hip_unique_lengths_device.restype = C.c_int
    L.sufr_hip_set_kmer_tile.argtypes = [vp, u64]; L.sufr_hip_set_kmer_tile.restype = C.c_int
    # include/sufr_repeat.h
    L.sufr_file_repeats.argtypes = [vp, u32, u64, u64, u64, u64, vp, vp, vp, C.POINTER(u64), C.POINTER(RepeatStats), C.c_int]
    L.sufr_file_repeats.restype = C.c_int
    L.sufr_hip_repeats_device.argtypes = [vp, vp, vp, vp, u64, u32, u64, u64, u64, u64, vp, vp, vp, C.POINTER(u64), C.POINTER(RepeatStats)]
    L.sufr_hip_repeats_device.restype = C.c_int
    L.sufr_hip_set_repeat_tile.argtypes = [vp, u64]; L.sufr_hip_set_repeat_tile.restype = C.c_int
    # include/sufr_lz.h
    L.sufr_file_lpf.argtypes = [vp, vp, vp, C.c_int]; L.sufr_file_lpf.restype = C.c_int
    L.sufr_file_lz.argtypes = [vp, u64, vp, vp, vp, C.POINTER(u64), C.POINTER(LzStats), C.c_int]; L.sufr_file_lz.restype = C.c_int
    L.sufr_hip_lpf_device.argtypes = [vp, vp, vp, vp, u64, vp, vp]; L.sufr_hip_lpf_device.restype = C.c_int
    L.sufr_hip_lz_device.argtypes = [vp, vp, vp, vp, u64, u64, vp, vp, vp, C.POINTER(u64), C.POINTER(LzStats)]
    L.sufr_hip_lz_device.restype = C.c_int
    L.sufr_hip_set_lz_tile.argtypes = [vp, u64, u64]; L.sufr_hip_set_lz_tile.restype = C.c_int
    # include/sufr_shared.h
    L.sufr_file_shared.argtypes = [vp, u32, u64, u64, u64, u64, u64, u64, vp, vp, vp, vp, C.POINTER(u64), C.POINTER(SharedStats), C.c_int]
    L.sufr_file_shared.restype = C.c_int
    L.sufr_file_common.argtypes = [vp, vp, C.c_int]; L.sufr_file_common.restype = C.c_int
    L.sufr_hip_shared_device.argtypes = [vp, vp, vp, vp, u64, u32, u64, u64, u64, u64, u64, u64, vp, vp, vp, vp, C.POINTER(u64),
                                         C.POINTER(SharedStats)]
    L.sufr_hip_shared_device.restype = C.c_int
    L.sufr_hip_common_device.argtypes = [vp, vp, vp, vp, u64, vp]; L.sufr_hip_common_device.restype = C.c_int
    # include/sufr_bwt.h
    L.sufr_file_bwt.argtypes = [vp, vp, vp, C.c_int]; L.sufr_file_bwt.restype = C.c_int
    L.sufr_file_bwt_runs.argtypes = [vp, u64, u64, vp, vp, vp, vp, C.POINTER(u64), C.POINTER(BwtStats), C.c_int]; L.sufr_file_bwt_runs.restype = C.c_int
    L.sufr_file_lf.argtypes = [vp, vp, C.c_int]; L.sufr_file_lf.restype = C.c_int
    L.sufr_hip_bwt_device.argtypes = [vp, vp, vp, vp]; L.sufr_hip_bwt_device.restype = C.c_int
    L.sufr_hip_bwt_runs_device.argtypes = [vp, vp, u64, u64, vp, vp, vp, vp, C.POINTER(u64), C.POINTER(BwtStats)]
    L.sufr_hip_bwt_runs_device.restype = C.c_int
    L.sufr_hip_lf_device.argtypes = [vp, vp, vp]; L.sufr_hip_lf_device.restype = C.c_int
    L.sufr_hip_set_bwt_tile.argtypes = [vp, u64]; L.sufr_hip_set_bwt_tile.restype = C.c_int
    # include/sufr_fm.h
    L.sufr_file_fm_build.argtypes = [vp, u64, C.POINTER(vp), C.c_int]; L.sufr_file_fm_build.restype = C.c_int
    L.sufr_fm_free.argtypes = [vp]; L.sufr_fm_free.restype = None
    L.sufr_fm_get_info.argtypes = [vp, C.POINTER(FmInfo)]; L.sufr_fm_get_info.restype = C.c_int
    L.sufr_fm_search_batch.argtypes = [vp, vp, vp, u64, vp, vp, C.c_int]; L.sufr_fm_search_batch.restype = C.c_int
    L.sufr_fm_locate_batch.argtypes = [vp, vp, vp, u64, u64, vp, vp, u64, C.POINTER(u64), C.c_int]; L.sufr_fm_locate_batch.restype = C.c_int
    L.sufr_hip_fm_build.argtypes = [vp, vp, u64, C.POINTER(vp)]; L.sufr_hip_fm_build.restype = C.c_int
    L.sufr_hip_fm_free.argtypes = [vp]; L.sufr_hip_fm_free.restype = None
    L.sufr_hip_fm_get_info.argtypes = [vp, C.POINTER(FmInfo)]; L.sufr_hip_fm_get_info.restype = C.c_int
    L.sufr_hip_fm_search_batch_device.argtypes = [vp, vp, vp, vp, u64, vp, vp]; L.sufr_hip_fm_search_batch_device.restype = C.c_int
    L.sufr_hip_fm_locate_batch_device.argtypes = [vp, vp, vp, vp, u64, u64, vp, vp, u64, C.POINTER(u64)]
    L.sufr_hip_fm_locate_batch_device.restype = C.c_int
    # include/sufr_fm_approx.h
    L.sufr_fm_approx.argtypes = [vp, vp, vp, u64, C.c_uint32, C.c_uint32, u64, vp, vp, vp, vp, C.POINTER(u64), C.c_int]
    L.sufr_fm_approx.restype = C.c_int
    L.sufr_fm_approx_steps.argtypes = [vp, vp, vp, u64, C.c_uint32, C.c_uint32, vp, vp, C.c_int]; L.sufr_fm_approx_steps.restype = C.c_int
    L.sufr_hip_fm_approx_device.argtypes = [vp, vp, vp, vp, u64, C.c_uint32, C.c_uint32, u64, vp, vp, vp, vp, C.POINTER(u64)]
    L.sufr_hip_fm_approx_device.restype = C.c_int
    L.sufr_hip_fm_approx.argtypes = [vp, vp, vp, vp, u64, C.c_uint32, C.c_uint32, u64, vp, vp, vp, vp, C.POINTER(u64)]
    L.sufr_hip_fm_approx.restype = C.c_int
    # include/sufr_fm_text.h
    L.sufr_file_fm_build_flags.argtypes = [vp, u64, u32, C.POINTER(vp), C.c_int]; L.sufr_file_fm_build_flags.restype = C.c_int
    L.sufr_fm_get_text_info.argtypes = [vp, C.POINTER(FmTextInfo)]; L.sufr_fm_get_text_info.restype = C.c_int
    L.sufr_fm_extract_batch.argtypes = [vp, vp, vp, u64, vp, vp, u64, C.POINTER(u64), C.c_int]; L.sufr_fm_extract_batch.restype = C.c_int
    L.sufr_fm_save.argtypes = [vp, cp, vp, cp, C.c_size_t]; L.sufr_fm_save.restype = C.c_int
    L.sufr_fm_load.argtypes = [cp, C.POINTER(vp), C.c_int, cp, C.c_size_t]; L.sufr_fm_load.restype = C.c_int
    L.sufr_fm_num_sequences.argtypes = [vp]; L.sufr_fm_num_sequences.restype = u64
    L.sufr_fm_sequence_start.argtypes = [vp, u64]; L.sufr_fm_sequence_start.restype = u64
    L.sufr_fm_sequence_name.argtypes = [vp, u64]; L.sufr_fm_sequence_name.restype = cp
    L.sufr_fm_set_sequences.argtypes = [vp, vp, C.POINTER(cp), u64]; L.sufr_fm_set_sequences.restype = C.c_int
    L.sufr_hip_fm_build_flags.argtypes = [vp, vp, u64, u32, C.POINTER(vp)]; L.sufr_hip_fm_build_flags.restype = C.c_int
    L.sufr_hip_fm_get_text_info.argtypes = [vp, C.POINTER(FmTextInfo)]; L.sufr_hip_fm_get_text_info.restype = C.c_int
    L.sufr_hip_fm_extract_batch_device.argtypes = [vp, vp, vp, vp, u64, vp, vp, u64, C.POINTER(u64)]
    L.sufr_hip_fm_extract_batch_device.restype = C.c_int
    L.sufr_hip_fm_extract_batch.argtypes = [vp, vp, vp, vp, u64, vp, vp, u64, C.POINTER(u64)]; L.sufr_hip_fm_extract_batch.restype = C.c_int
    L.sufr_hip_fm_upload.argtypes = [vp, vp, C.POINTER(vp)]; L.sufr_hip_fm_upload.restype = C.c_int
    L.sufr_hip_fm_download.argtypes = [vp, vp, C.POINTER(vp)]; L.sufr_hip_fm_download.restype = C.c_int
    # include/sufr_fm_match.h
    L.sufr_fm_pair_check.argtypes = [vp, vp]; L.sufr_fm_pair_check.restype = C.c_int
    L.sufr_fm_matching_stats.argtypes = [vp, vp, vp, vp, u64, vp, C.c_int]; L.sufr_fm_matching_stats.restype = C.c_int
    L.sufr_fm_smems.argtypes = [vp, vp, vp, vp, u64, u32, u64, vp, vp, vp, vp, vp, C.POINTER(u64), C.c_int]; L.sufr_fm_smems.restype = C.c_int
    L.sufr_fm_matching_stats_steps.argtypes = [vp, vp, vp, vp, u64, vp, C.c_int]; L.sufr_fm_matching_stats_steps.restype = C.c_int
    L.sufr_file_write_reversed_fasta.argtypes = [vp, cp, cp, C.c_size_t]; L.sufr_file_write_reversed_fasta.restype = C.c_int
    L.sufr_hip_fm_matching_stats_device.argtypes = [vp, vp, vp, vp, vp, u64, vp]; L.sufr_hip_fm_matching_stats_device.restype = C.c_int
    L.sufr_hip_fm_smems_device.argtypes = [vp, vp, vp, vp, vp, u64, u32, vp, u64, vp, vp, vp, vp, vp, C.POINTER(u64)]
    L.sufr_hip_fm_smems_device.restype = C.c_int
    L.sufr_hip_fm_smems.argtypes = [vp, vp, vp, vp, vp, u64, u32, u64, vp, vp, vp, vp, vp, C.POINTER(u64)]; L.sufr_hip_fm_smems.restype = C.c_int
    _lib = L
    return L


class Context:
    """sufr_hip_ctx: one per GPU."""

    def __init__(self, device: int = 0):
        L = lib()
        self._h = L.sufr_hip_create(device)
        if not self._h:
            raise SufrHipError(-2, L.sufr_hip_last_error(None).decode())
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            lib().sufr_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc: int):
        if rc != 0:
            raise SufrHipError(rc, lib().sufr_hip_last_error(self._h).decode())

    def set_window(self, window: int = 0, margin: int = 0):
        """Windowed builds (include/sufr_hip.h, sufr_hip_set_window); 0, 0 restores the defaults."""
        self.check(lib().sufr_hip_set_window(self._h, window, margin))

    def set_window_retry(self, widest_margin: int = 0):
        """Cap of the margin a window is re-built with when a repeat crosses its end (0: what 32 bits allow)."""
        self.check(lib().sufr_hip_set_window_retry(self._h, widest_margin))

    def set_array_budget(self, nbytes: int = 0):
        """Out-of-core windowed create: device bytes the SA + LCP arrays may take at once (sufr_hip_set_array_budget; 0: no limit)."""
        self.check(lib().sufr_hip_set_array_budget(self._h, nbytes))

    def set_trace_scratch(self, nbytes: int = 0):
        """Alignment traceback: device bytes the rows of a chunk of records may take (sufr_hip_set_trace_scratch; 0: the default)."""
        self.check(lib().sufr_hip_set_trace_scratch(self._h, nbytes))

    def set_kmer_tile(self, ranks: int = 0):
        """k-mer counts: ranks one workgroup folds at a time (sufr_hip_set_kmer_tile; 0: the default).  Rounded up to 256 and
        held to 16384; it changes no result."""
        self.check(lib().sufr_hip_set_kmer_tile(self._h, ranks))

    def set_repeat_tile(self, ranks: int = 0):
        """Repeats: ranks one workgroup takes at a time (sufr_hip_set_repeat_tile; 0: the default).  Rounded up to 256 and
        held to 16384; it changes no result."""
        self.check(lib().sufr_hip_set_repeat_tile(self._h, ranks))

    def set_lz_tile(self, ranks: int = 0, positions: int = 0):
        """LPF and LZ77: ranks one workgroup of the LPF pass takes at a time and text positions one workgroup of the parse
        takes at a time (sufr_hip_set_lz_tile; 0: the default).  Rounded up to 256 and held to 16384; they change no result."""
        self.check(lib().sufr_hip_set_lz_tile(self._h, ranks, positions))

    def set_bwt_tile(self, ranks: int = 0):
        """BWT, runs and LF: ranks one workgroup takes at a time (sufr_hip_set_bwt_tile; 0: the default).  Rounded up to 256
        and held to 16384; it changes no result."""
        self.check(lib().sufr_hip_set_bwt_tile(self._h, ranks))

    @property
    def window_repairs(self) -> int:
        """Suffixes of the last windowed build that were ordered by whole-text comparison."""
        return int(lib().sufr_hip_window_repairs(self._h))

    def set_overlap_min(self, min_records: int = 0):
        """Left-over records (buckets that agree on the whole key) from which their re-keying chain runs on the helper pipeline,
        beside the tie runs (sufr_hip_set_overlap_min; 0: the default of 2^22, 2^64 - 1: never)."""
        self.check(lib().sufr_hip_set_overlap_min(self._h, min_records))

    @property
    def overlapped(self) -> int:
        """1 if the last build ran the left-over chain on the helper pipeline (a windowed build: in one of its windows)."""
        return int(lib().sufr_hip_overlapped(self._h))

    @property
    def doublings(self) -> int:
        """How many times the last build handed a level to prefix doubling (both chains; a windowed build: all windows)."""
        return int(lib().sufr_hip_doublings(self._h))

    def set_pair_walk(self, mode: int = 0):
        """Tie runs of exactly two suffixes compared directly in front of the tie level (sufr_hip_set_pair_walk; 0: when the
        pairs hold a large enough share of the tie records, 1: always, 2: never).  The arrays do not depend on it."""
        self.check(lib().sufr_hip_set_pair_walk(self._h, mode))

    @property
    def pairs_walked(self):
        """(resolved, left_tied) of the last build: tie pairs the direct comparison finished, and pairs it handed back to the
        tie level because they agree for 4096 characters more (a windowed build: all windows)."""
        r, t = C.c_uint64(0), C.c_uint64(0)
        self.check(lib().sufr_hip_pairs_walked(self._h, C.byref(r), C.byref(t)))
        return int(r.value), int(t.value)

    def set_exc_max_affected(self, max_affected: int = 0):
        """Suffixes that may have looked at a byte outside the DNA table before a --dna build goes to the general code table
        instead of re-placing them (sufr_hip_set_exc_max_affected; 0: the default of 2^22, which is also the most)."""
        self.check(lib().sufr_hip_set_exc_max_affected(self._h, max_affected))

    @property
    def exc_retry(self) -> int:
        """Why the last build built its text again with the general code table: 0 it did not, 1 / 2 / 3 the limit it met
        (sufr_hip_exc_retry; a windowed build: the largest over its windows)."""
        return int(lib().sufr_hip_exc_retry(self._h))

    @property
    def exc_taken(self) -> int:
        """Ranks the last build took out of the arrays of the text with 'N' for the listed bytes (sufr_hip_exc_taken)."""
        return int(lib().sufr_hip_exc_taken(self._h))

    def synchronize(self):
        self.check(lib().sufr_hip_synchronize(self._h))

    @property
    def handle(self):
        return self._h
