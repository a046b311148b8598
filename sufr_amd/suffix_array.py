"""SuffixArray facade (libsufr/src/suffix_array.rs): `write` builds on the GPU, `read` opens a file for queries."""
from __future__ import annotations

from typing import Optional

from .sufr_builder import SufrBuilder, U32_MAX
from .sufr_file import SufrFile
from .types import SufrBuilderArgs


class SuffixArray:
    """After `read`, count / extract / list / locate / smems / mems / approx / edit / align / metadata / string_at are SufrFile's (suffix_array.rs:181-440)."""

    def __init__(self, inner: SufrFile):
        self.inner = inner

    @staticmethod
    def write(args: SufrBuilderArgs) -> str:
        """Build and write the .sufr file; u32 indices iff len(text) < u32::MAX.  Returns the path."""
        width = 4 if len(args.text) < U32_MAX else 8
        return SufrBuilder(args, index_width=width).path

    @staticmethod
    def read(filename: str, low_memory: bool = False) -> "SuffixArray":
        return SuffixArray(SufrFile(filename, low_memory))

    def count(self, queries, max_query_len: Optional[int] = None, low_memory: bool = False):
        return self.inner.count(queries, max_query_len, low_memory)

    def locate(self, queries, max_query_len: Optional[int] = None, low_memory: bool = False):
        return self.inner.locate(queries, max_query_len, low_memory)

    def extract(self, queries, max_query_len: Optional[int] = None, low_memory: bool = False, prefix_len=None, suffix_len=None):
        return self.inner.extract(queries, max_query_len, low_memory, prefix_len, suffix_len)

    def smems(self, queries, min_len: int = 20, max_hits: int = 0):
        return self.inner.smems(queries, min_len, max_hits)

    def mems(self, queries, min_len: int = 20, max_occ: int = 0, both_strands: bool = False, threads: int = 0):
        return self.inner.mems(queries, min_len, max_occ, both_strands, threads)

    def approx(self, queries, max_mismatches: int = 2, max_occ: int = 0, both_strands: bool = False, threads: int = 0):
        return self.inner.approx(queries, max_mismatches, max_occ, both_strands, threads)

    def edit(self, queries, max_edits: int = 2, max_occ: int = 0, both_strands: bool = False, local_minima: bool = False,
             threads: int = 0):
        return self.inner.edit(queries, max_edits, max_occ, both_strands, local_minima, threads)

    def align(self, queries, max_edits: int = 2, max_occ: int = 0, both_strands: bool = False, local_minima: bool = False,
              threads: int = 0):
        return self.inner.align(queries, max_edits, max_occ, both_strands, local_minima, threads)

    def list(self, **opts):
        return self.inner.list(**opts)

    def metadata(self):
        return self.inner.metadata()

    def string_at(self, pos: int, len: Optional[int] = None) -> str:
        return self.inner.string_at(pos, len)
