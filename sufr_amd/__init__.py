"""sufr_amd: MI355X-native suffix-array + LCP construction behind the `sufr create` contract.

The construction path of TravisWheelerLab/sufr and, next to it, the reader / query side of
the files it writes (row f3); the compute is hand-written HIP for gfx950 in csrc/, reached through the C ABI of
include/sufr_hip.h, include/sufr_query.h, include/sufr_match.h, include/sufr_mem.h, include/sufr_approx.h, include/sufr_edit.h, include/sufr_align.h, include/sufr_kmer.h, include/sufr_repeat.h, include/sufr_lz.h, include/sufr_shared.h, include/sufr_bwt.h, include/sufr_fm.h and include/sufr_fm_approx.h."""
from ._lib import Context, Stats, SufrHipError, build_extension, lib, EXPORTS, QUERY_EXPORTS, MATCH_EXPORTS, MEM_EXPORTS, APPROX_EXPORTS, EDIT_EXPORTS, ALIGN_EXPORTS, KMER_EXPORTS, KmerStats, REPEAT_EXPORTS, RepeatStats, LZ_EXPORTS, LzStats, SHARED_EXPORTS, SharedStats, BWT_EXPORTS, BwtStats, FM_EXPORTS, FM_APPROX_EXPORTS, FM_TEXT_EXPORTS, FM_MATCH_EXPORTS, FmInfo, FmTextInfo, LIB_PATH, CLI_PATH
from .types import OUTFILE_VERSION, SENTINEL_CHARACTER, SequenceFileData, SufrBuilderArgs
from .util import lcp_pair, normalize, read_sequence_file
from .sufr_builder import DeviceBuilder, SufrBuilder
from .sufr_file import (AlignHit, ApproxHit, CountResult, DeviceFmIndex, DeviceIndex, FmIndex, EditHit, ExtractResult, ExtractSequence, LocatePosition, LocateResult, MemHit, SmemHit, SufrFile,
                        SufrMetadata, pack_queries)
from .suffix_array import SuffixArray
from .cli import create

__all__ = [
    "Context", "Stats", "SufrHipError", "build_extension", "lib", "EXPORTS", "LIB_PATH", "CLI_PATH",
    "OUTFILE_VERSION", "SENTINEL_CHARACTER", "SequenceFileData", "SufrBuilderArgs", "lcp_pair", "normalize",
    "read_sequence_file", "DeviceBuilder", "SufrBuilder", "SuffixArray", "create", "QUERY_EXPORTS", "SufrFile", "DeviceIndex",
    "CountResult", "LocateResult", "LocatePosition", "ExtractResult", "ExtractSequence", "SufrMetadata", "pack_queries",
    "MATCH_EXPORTS", "SmemHit", "MEM_EXPORTS", "MemHit", "APPROX_EXPORTS", "ApproxHit", "EDIT_EXPORTS", "EditHit", "ALIGN_EXPORTS", "AlignHit", "KMER_EXPORTS", "KmerStats", "REPEAT_EXPORTS", "RepeatStats", "LZ_EXPORTS", "LzStats",
    "SHARED_EXPORTS", "SharedStats", "BWT_EXPORTS", "BwtStats", "FM_EXPORTS", "FM_APPROX_EXPORTS", "FM_TEXT_EXPORTS", "FM_MATCH_EXPORTS", "FmInfo", "FmTextInfo", "FmIndex", "DeviceFmIndex",
]
