// sufr_fm_host.h -- the FM-index on the host as an object (include/sufr_fm.h, sufr_fm_text.h): what sufr_query.cpp builds,
// loads, saves and queries, and what the copies between host and device of sufr_fm.inc read and fill.  Also the sizes of the
// index file's sections, which both sides report (sufr_fm_text_info.file_bytes).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "sufr_fm_scan.h"

struct sufr_fm {
    sufr::FmShape sh{};
    uint64_t s = 0, q = 0, samples = 0;
    uint32_t e = 0;
    uint64_t C[257] = {0};
    uint32_t col[256];
    std::vector<uint8_t> blocks, kept;
    std::vector<sufr::FmMark> marks;
    std::vector<uint8_t> text_kept;           // samples entries of w bytes with SUFR_FM_TEXT, else empty
    std::vector<uint64_t> seq_starts;         // the sequences the index remembers (sufr_fm_save)
    std::vector<std::string> seq_names;
    sufr::FmView view() const { return sufr::FmView{blocks.data(), marks.data(), kept.data(), C, col, s, q, sh, e}; }
};

namespace sufr {

static constexpr uint64_t FM_FILE_PAGE = 4096, FM_FILE_SECTIONS = 7, FM_TABLE_BYTES = 257 * 8 + 256 * 4;
enum { FM_SEC_TABLES, FM_SEC_STARTS, FM_SEC_NAMES, FM_SEC_BLOCKS, FM_SEC_MARKS, FM_SEC_KEPT, FM_SEC_TEXT };

// the (offset, length) of every section and the length of the file, from the lengths
struct FmFileLayout { uint64_t off[FM_FILE_SECTIONS], len[FM_FILE_SECTIONS], bytes; };

inline FmFileLayout fm_file_layout(const FmShape& sh, uint64_t s, uint64_t q, uint64_t samples, bool text, uint64_t sequences, uint64_t name_bytes)
{
    FmFileLayout L{};
    L.len[FM_SEC_TABLES] = FM_TABLE_BYTES;
    L.len[FM_SEC_STARTS] = sequences * 8;
    L.len[FM_SEC_NAMES] = name_bytes;
    L.len[FM_SEC_BLOCKS] = fm_blocks(s, sh.B) * sh.stride;
    L.len[FM_SEC_MARKS] = q ? fm_mark_words(s) * sizeof(FmMark) : 0;
    L.len[FM_SEC_KEPT] = q ? samples * sh.w : 0;
    L.len[FM_SEC_TEXT] = text ? samples * sh.w : 0;
    uint64_t at = FM_FILE_PAGE;
    for (uint64_t i = 0; i < FM_FILE_SECTIONS; i++) {
        L.off[i] = at;
        at = (at + L.len[i] + FM_FILE_PAGE - 1) / FM_FILE_PAGE * FM_FILE_PAGE;
    }
    L.bytes = L.off[FM_SEC_TEXT] + L.len[FM_SEC_TEXT];
    return L;
}

}  // namespace sufr
