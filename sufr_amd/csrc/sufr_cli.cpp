// sufr_cli.cpp -- `sufr create` on the MI355X build path.
//
// Command-line contract of the reference for this path: sufr/src/lib.rs:29-46 (global -t/--threads,
// -l/--log, --log-file), 83-125 (CreateArgs, alias `cr`), sufr/src/main.rs:8-40 (errors are printed as
// "Error: <msg>" and exit code 1).  The query sub-commands (count / locate / extract / list / summarize,
// sufr/src/lib.rs:129-271 for their arguments, 292-646 for their output) read the file through
// include/sufr_query.h; their output is the reference's, character for character.
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include <chrono>
#include <string>
#include <thread>
#include <unistd.h>
#include <vector>

#include "../../include/sufr_hip.h"
#include "../../include/sufr_query.h"
#include "../../include/sufr_match.h"
#include "../../include/sufr_mem.h"
#include "../../include/sufr_approx.h"
#include "../../include/sufr_edit.h"
#include "../../include/sufr_align.h"
#include "../../include/sufr_kmer.h"
#include "../../include/sufr_repeat.h"
#include "../../include/sufr_lz.h"
#include "../../include/sufr_bwt.h"
#include "../../include/sufr_fm_approx.h"
#include "../../include/sufr_fm_text.h"
#include "../../include/sufr_fm_match.h"
#include "../../include/sufr_shared.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <fstream>
#include <optional>
#include <sstream>
#include <time.h>

namespace {

struct Log {
    int level = 0;  // 0 off, 1 info, 2 debug
    FILE* out = stdout;
    void info(const std::string& s) const { if (level >= 1) { fprintf(out, "[INFO  sufr] %s\n", s.c_str()); fflush(out); } }
    void debug(const std::string& s) const { if (level >= 2) { fprintf(out, "[DEBUG sufr] %s\n", s.c_str()); fflush(out); } }
};

std::string with_commas(uint64_t v)
{
    std::string s = std::to_string(v), r;
    int c = 0;
    for (size_t i = s.size(); i-- > 0;) { r.insert(r.begin(), s[i]); if (++c % 3 == 0 && i) r.insert(r.begin(), ','); }
    return r;
}

int usage(FILE* f)
{
    fprintf(f,
            "Usage: sufr [OPTIONS] <COMMAND> ...\n\n"
            "Commands:\n"
            "  create|cr    <INPUT>                 Create sufr file (on the GPU)\n"
            "  count|co     <SUFR> <QUERY>...       Count occurrences of sequences [-m LEN] [-o OUT] [-l] [-v]\n"
            "  locate|lo    <SUFR> <QUERY>...       Locate sequences [-a] [-m LEN] [-o OUT] [-l] [-v]\n"
            "  extract|ex   <SUFR> <QUERY>...       Extract sequences [-p PREFIX_LEN] [-s SUFFIX_LEN] [-m LEN] [-o OUT] [-l] [-v]\n"
            "  list|ls      <FILE> [RANK]...        List the suffix array [-r] [-s] [-p] [--len LEN] [-n NUM] [-o OUT] [-v]\n"
            "  summarize|su <SUFR>                  Summarize sufr file\n"
            "  match|ma     <SUFR> [QUERY]...       Super-maximal exact matches of the queries: one line per SMEM,\n"
            "                                       name  offset  length  count  positions\n"
            "                                       [-k|--min-len N (20)] [-n|--max-hits N (0: all)] [-a|--abs]\n"
            "                                       [-q|--reads FASTA/FASTQ] [-o OUT]\n"
            "  mems|me      <SUFR> [QUERY]...       Maximal exact matches of the queries: one line per MEM,\n"
            "                                       name  strand(+/-)  offset  length  seq:pos\n"
            "                                       [-k|--min-len N (20)] [--max-occ N (0: no limit)] [-b|--both-strands]\n"
            "                                       [-a|--abs] [-q|--reads FASTA/FASTQ] [-o OUT]\n"
            "  approx|ap    <SUFR> [QUERY]...       Occurrences of the queries with at most N mismatches: one line per window,\n"
            "                                       name  strand(+/-)  seq:pos  mismatches\n"
            "                                       [-d|--mismatches N (2)] [--max-occ N (0: no limit)] [-b|--both-strands]\n"
            "                                       [-a|--abs] [-q|--reads FASTA/FASTQ] [-o OUT]\n"
            "  edit|ed      <SUFR> [QUERY]...       Where the queries end with at most N edits (substitutions, insertions,\n"
            "                                       deletions): one line per end, name  strand(+/-)  seq:end  edits\n"
            "                                       [-d|--edits N (2)] [--max-occ N (0: no limit)] [-b|--both-strands]\n"
            "                                       [-l|--local-minima] [-a|--abs] [-q|--reads FASTA/FASTQ] [-o OUT]\n"
            "                                       [-c|--cigar: two more columns, the start (as the end) and the CIGAR (= X I D)]\n"
            "  kmers|km     <SUFR>                  k-mer spectrum of the indexed text from its LCP array: one line per non-empty bin,\n"
            "                                       count  kmers (the last bin as >=BINS), then # whole, # distinct, # unique, # max_count\n"
            "                                       -k K [-b|--bins BINS (256)] [--device ID: on that GPU; otherwise on the host]\n"
            "                                       [--occ FILE: the count of the k-mer at every text position] [--unique FILE: the length\n"
            "                                       at which the substring at every text position becomes unique]; both files hold one raw\n"
            "                                       little-endian entry of the index width (4 or 8 bytes) per text position, 0 where the\n"
            "                                       position is not indexed or the k-mer / substring runs over the end of its sequence\n"
            "  repeats|rp   <SUFR>                  repeats of the indexed text from its LCP array, one line each in rank order:\n"
            "                                       length  count  occurrences (seq:pos, ascending by text position), then # records,\n"
            "                                       # longest, # longest_rank, # max_count\n"
            "                                       -l MINLEN [-c MINCOUNT (2)] [-C MAXCOUNT (0: no limit)] [--kind branching|maximal|super]\n"
            "                                       [--max-positions P (16; 0: all)] [--device ID: on that GPU; otherwise on the host] [-o OUT]\n"
            "  shared       <SUFR>                  the lines of repeats with one more column, the number of different sequences the\n"
            "                                       occurrences lie in: length  count  seqs  occurrences, then the # lines and # max_seqs\n"
            "                                       the options of repeats, [-q|--min-seqs Q (0: no limit)] [--max-seqs Q (0: no limit)]\n"
            "                                       [--common: instead one line q  length per q = 1 .. sequences, the longest substring\n"
            "                                       common to at least q sequences; takes only --device and -o]\n"
            "  lz           <SUFR>                  the LZ77 factors of the text from its SA and LCP, one line each in text order:\n"
            "                                       seq:offset  length  source-seq:offset (* for a literal), then # factors, # literals,\n"
            "                                       # longest, # longest_start\n"
            "                                       [--lpf: one line per text position instead: seq:offset  longest previous factor  source]\n"
            "                                       [--device ID: on that GPU; otherwise on the host] [-t THREADS] [-o OUT]\n"
            "  bwt          <SUFR>                  the Burrows-Wheeler transform of the indexed text from its SA (the byte in front of\n"
            "                                       every indexed suffix, in rank order): one line symbol  count per occurring byte\n"
            "                                       (printable bytes as themselves, others as \\xHH), then # ranks, # runs, # longest,\n"
            "                                       # longest_rank of its equal-letter runs\n"
            "                                       [--runs [--min-len L (1)]: in front of the # lines one line per run of at least L ranks:\n"
            "                                       rank  length  symbol  seq:offset of its first suffix]\n"
            "                                       [--bwt FILE: the raw bytes, one per rank] [--lf FILE: the LF mapping, one raw little-endian\n"
            "                                       entry of the index width (4 or 8 bytes) per rank]\n"
            "                                       [--device ID: on that GPU; otherwise on the host] [-t THREADS] [-o OUT]\n"
            "  fm           <SUFR> <QUERY>...       count, or with --locate locate, through an FM-index built from the file: backward\n"
            "                                       search over checkpointed BWT blocks and a sampled suffix array instead of text and\n"
            "                                       suffix array; the lines are those of count / locate.  Refused unless every text\n"
            "                                       position is indexed, without seed mask and max_query_len, and the last byte occurs once\n"
            "                                       [--locate [-a]] [-s|--sample Q (32): keep every suffix at a multiple of Q]\n"
            "                                       [--max-hits N (0: all)] [-q|--reads FILE] [--device ID] [-t THREADS] [-o OUT]\n"
            "                                       [-d|--mismatches D (at most 3) [-b|--both-strands] [-a]: instead every window of the\n"
            "                                       text within D mismatches of a query, by backtracking on the FM-index alone; the lines\n"
            "                                       are those of approx, in another order.  Needs samples: -s 0 is an error]\n"
            "                                       [--save OUT.fm [--text]: build the index (on the GPU with --device) and write it to a\n"
            "                                       file; --text keeps the text samples, with which the index gives the text back]\n"
            "                                       [--index IN.fm instead of <SUFR>: load such a file (verified) and answer from it alone,\n"
            "                                       on the GPU with --device; no .sufr is opened]\n"
            "                                       [--extract [--prefix-len N] [--suffix-len N]: the lines of extract for the hits of every\n"
            "                                       query, the bases read back from the BWT; implies --text]\n"
            "                                       [--write-reverse OUT.fa: write the FASTA of the reversed text (every sequence reversed, their\n"
            "                                       order reversed); `sufr create` it with the flags of <SUFR> for the .sufr of --reverse]\n"
            "                                       [--smems --reverse REV [-k MIN_LEN (20)] [--max-hits N] [-a]: the lines of match (name,\n"
            "                                       offset, length, count, positions) from two FM-indexes alone, that of <SUFR> or --index and\n"
            "                                       that of the reversed text; REV is the .sufr of the reversed FASTA (its index is built\n"
            "                                       without samples) or an index file saved from it.  Needs samples: -s 0 is an error]\n"
            "  count / locate / extract / match / mems / approx / edit take --device <ID>: the queries are searched as one batch on that GPU\n\n"
            "Global options:\n"
            "  -t, --threads <THREADS>   Host workers of count / locate / extract [default: one per core]; create runs on the GPU\n"
            "  -l, --log <LOG>           Log level [possible values: info, debug]\n"
            "      --log-file <FILE>     Log file\n"
            "      --device <ID>         HIP device ordinal [default: 0]\n"
            "      --devices <ID,ID,...> Build on several GPUs: the suffixes are split by first-digit range, every GPU\n"
            "                            sorts its range and writes its slice of the one output file\n\n"
            "create options:\n"
            "  -n, --num-partitions <NUM_PARTS>  Subproblem count [default: 16]\n"
            "  -m, --max-query-len <CONTEXT>     Max context\n"
            "  -o, --output <OUTPUT>             Output file\n"
            "  -d, --dna                         Input is DNA\n"
            "  -a, --allow-ambiguity             Allow suffixes starting with ambiguity codes\n"
            "  -i, --ignore-softmask             Ignore suffixes in soft-mask/lowercase regions\n"
            "  -D, --sequence-delimiter <DELIM>  Character to separate sequences [default: %%]\n"
            "  -s, --seed-mask <MASK>            Spaced seeds mask\n"
            "  -r, --random-seed <RANDSEED>      Random seed [default: 42]\n"
            "      --window <POSITIONS>          Build texts longer than this in overlapping windows merged on the device\n"
            "                                    [default: one window below 2^32 - 2^24 bytes, as few as fit above]\n"
            "      --margin <POSITIONS>          Comparison context after every window [default: 2^26]\n"
            "      --array-budget <BYTES>        Windowed builds: device memory the suffix + LCP arrays may take at once; the build\n"
            "                                    runs shard after shard and streams every slice to the file [default: no limit;\n"
            "                                    arrays that do not fit are split by themselves]\n\n"
            "Texts of 2^32 - 2^24 bytes and more are built in overlapping 32-bit windows merged on the device; with --devices every\n"
            "device builds its shard of the windows (a seed mask: on the first device).\n");
    return f == stderr ? 2 : 0;
}

// need(i, opt): the value of the option at argv[i], the argument behind it; without one the usage error and exit status 2
auto value_reader(int argc, char** argv)
{
    return [argc, argv](int& i, const char* opt) -> const char* {
        if (i + 1 >= argc) { fprintf(stderr, "error: a value is required for '%s'\n", opt); exit(2); }
        return argv[++i];
    };
}

// ---------------------------------------------------------------------------------------------------------------
// query sub-commands (sufr/src/lib.rs:292-646)
// ---------------------------------------------------------------------------------------------------------------
struct QueryArgs {
    std::string file, output;
    std::vector<std::string> positional;        // queries / ranks
    bool has_mql = false; uint64_t mql = 0;
    bool abs = false;
    bool has_prefix = false, has_suffix = false; uint64_t prefix_len = 0, suffix_len = 0;
    bool show_rank = false, show_suffix = false, show_lcp = false;
    bool has_len = false, has_number = false; uint64_t len = 0, number = 0;
    int device = -1;                            // --device N: the whole batch of queries is searched on that GPU
    int threads = 0;                            // -t/--threads (global option, sufr/src/lib.rs:29-46): host search workers
    uint64_t min_len = 20, max_hits = 0;        // match / mems: -k, match: -n
    std::string reads;                          // match / mems: -q FASTA / FASTQ of named queries
    uint64_t max_occ = 0;                       // mems / approx: --max-occ
    bool both_strands = false;                  // mems / approx: -b
    uint64_t mismatches = 2;                    // approx: -d
    uint64_t edits = 2;                         // edit: -d
    bool local_minima = false;                  // edit: -l
    bool cigar = false;                         // edit: -c
    bool locate = false;                        // fm: --locate
    uint64_t sample = 32;                       // fm: -s
    bool fm_approx = false;                     // fm: -d / --mismatches given (the distance is `mismatches`)
    std::string fm_save, fm_index;              // fm: --save OUT.fm, --index IN.fm
    bool fm_text = false, fm_extract = false;   // fm: --text, --extract
    bool fm_smems = false;                      // fm: --smems
    std::string fm_reverse, fm_write_reverse;   // fm: --reverse REV, --write-reverse OUT.fa
};

// parse_locate_queries (lib.rs:449-466): an argument that names an existing file is read as whitespace-separated queries
std::vector<std::string> expand_queries(const std::vector<std::string>& args)
{
    std::vector<std::string> out;
    for (const std::string& a : args) {
        struct stat sb;
        if (stat(a.c_str(), &sb) == 0) {
            // an argument that names something on disk is a file of queries (sufr/src/lib.rs: the path is opened and
            // read; a directory or an unreadable file is an error there too, not an empty query list)
            std::ifstream in(a);
            if (!S_ISREG(sb.st_mode) || !in) {
                fprintf(stderr, "Error: %s: %s\n", a.c_str(), S_ISDIR(sb.st_mode) ? "Is a directory" : "cannot read the query file");
                exit(1);
            }
            std::string w;
            while (in >> w) out.push_back(w);
        } else out.push_back(a);
    }
    return out;
}

struct OutFile {
    FILE* f = stdout;
    bool open(const std::string& name)
    {
        if (name.empty()) return true;
        f = fopen(name.c_str(), "w");
        return f != nullptr;
    }
    ~OutFile() { if (f && f != stdout) fclose(f); }
};

sufr_file* open_or_die(const std::string& path)
{
    char err[512] = {0};
    sufr_file* f = nullptr;
    if (sufr_file_open(path.c_str(), &f, err, sizeof err) != 0) { fprintf(stderr, "Error: %s\n", err); exit(1); }
    return f;
}

// an open .sufr file, closed on every way out
struct OpenFile {
    sufr_file* f;
    explicit OpenFile(const std::string& path) : f(open_or_die(path)) {}
    ~OpenFile() { sufr_file_close(f); }
    operator sufr_file*() const { return f; }
    OpenFile(const OpenFile&) = delete;
    OpenFile& operator=(const OpenFile&) = delete;
};

// A context on one device with the index of an open file on it: what every sub-command but create runs on with --device.
// Not up(): error() is the library's text.  Index, then context are released with the object.
struct DeviceIndex {
    sufr_hip_ctx* ctx;
    sufr_hip_index* ix = nullptr;
    int rc = SUFR_HIP_E_HIP;                    // of the load (the context did not come up: E_HIP)
    DeviceIndex(int device, sufr_file* f) : ctx(sufr_hip_create(device)) { if (ctx) rc = sufr_hip_index_load(ctx, f, &ix); }
    ~DeviceIndex()
    {
        if (ix) sufr_hip_index_free(ix);
        if (ctx) sufr_hip_destroy(ctx);
    }
    bool up() const { return ctx && rc == 0; }
    const char* error() const { return sufr_hip_last_error(ctx); }     // (no context: the text of the failed create)
    DeviceIndex(const DeviceIndex&) = delete;
    DeviceIndex& operator=(const DeviceIndex&) = delete;
};

// Rank range of every query: one by one on the host, or as one batch on a GPU (text + suffix array copied to HBM first:
// worth it for many queries; the answers are the same, tests/test_gpu_query.py).  false: an error, printed
struct Hit { bool found; uint64_t lo, hi; };
bool search_all(sufr_file* f, const QueryArgs& a, const std::vector<std::string>& queries, std::vector<Hit>& hits)
{
    std::string bytes;
    std::vector<uint64_t> off(queries.size() + 1, 0), lo(queries.size(), 0), hi(queries.size(), 0);
    for (size_t i = 0; i < queries.size(); i++) { bytes += queries[i]; off[i + 1] = bytes.size(); }
    if (a.device < 0)
        sufr_file_search_batch(f, (const uint8_t*)bytes.data(), off.data(), queries.size(), a.has_mql, a.mql, lo.data(), hi.data(), a.threads);
    else {
        DeviceIndex dev(a.device, f);
        if (!dev.up() || sufr_hip_search_batch(dev.ctx, dev.ix, (const uint8_t*)bytes.data(), off.data(), queries.size(), a.has_mql, a.mql,
                                               lo.data(), hi.data()) != 0) {
            fprintf(stderr, "Error: %s\n", dev.error());
            return false;
        }
    }
    hits.resize(queries.size());
    for (size_t i = 0; i < queries.size(); i++) hits[i] = Hit{hi[i] > lo[i], lo[i], hi[i]};
    return true;
}

int cmd_count(const QueryArgs& a)
{
    OpenFile f(a.file);
    OutFile out;
    if (!out.open(a.output)) { fprintf(stderr, "Error: %s: cannot create\n", a.output.c_str()); return 1; }
    const std::vector<std::string> queries = expand_queries(a.positional);
    std::vector<Hit> hits;
    if (!search_all(f, a, queries, hits)) return 1;
    for (size_t i = 0; i < queries.size(); i++)
        fprintf(out.f, "%s %llu\n", queries[i].c_str(), (unsigned long long)(hits[i].found ? hits[i].hi - hits[i].lo : 0));
    return 0;
}

// The lines of `sufr locate`: query qi has count(qi) hits (0: not found), suffix(qi, k) is the text position of hit k in rank
// order.  `sufr fm --locate` prints through here too, with positions that no suffix array was read for.
// the sequences of the text: of an open .sufr file, or those an FM-index file carries (SeqTable)
struct SeqTable {
    std::vector<uint64_t> starts;
    std::vector<std::string> names;
};
uint64_t seq_of(const sufr_file* f, uint64_t p) { return sufr_file_sequence_of(f, p); }
uint64_t seq_start(const sufr_file* f, uint64_t i) { return sufr_file_sequence_start(f, i); }
const char* seq_name(const sufr_file* f, uint64_t i) { return sufr_file_sequence_name(f, i); }
uint64_t seq_of(const SeqTable& t, uint64_t p)            // (sufr_file_sequence_of: the last sequence that starts at or before p)
{
    const size_t k = (size_t)(std::upper_bound(t.starts.begin(), t.starts.end(), p) - t.starts.begin());
    return k ? k - 1 : 0;
}
uint64_t seq_start(const SeqTable& t, uint64_t i) { return i < t.starts.size() ? t.starts[i] : 0; }
const char* seq_name(const SeqTable& t, uint64_t i) { return i < t.names.size() ? t.names[i].c_str() : ""; }

template <typename Seqs, typename Count, typename Suffix>
void print_located(const Seqs& f, FILE* out, bool abs, const std::vector<std::string>& queries, Count count, Suffix suffix)
{
    for (size_t qi = 0; qi < queries.size(); qi++) {
        const std::string& q = queries[qi];
        const uint64_t hits = count(qi);
        if (!hits) {
            fprintf(stderr, "%s not found\n", q.c_str());
            continue;
        }
        if (abs) {
            std::string line = q;
            for (uint64_t k = 0; k < hits; k++) line += " " + std::to_string(suffix(qi, k));
            fprintf(out, "%s\n", line.c_str());
            continue;
        }
        // by sequence name, then position inside the sequence (lib.rs:513-518)
        struct Pos { std::string name; uint64_t at; };
        std::vector<Pos> ps;
        for (uint64_t k = 0; k < hits; k++) {
            const uint64_t sfx = suffix(qi, k);
            const uint64_t i = seq_of(f, sfx);
            ps.push_back({seq_name(f, i), sfx - seq_start(f, i)});
        }
        std::stable_sort(ps.begin(), ps.end(), [](const Pos& x, const Pos& y) { return x.name != y.name ? x.name < y.name : x.at < y.at; });
        fprintf(out, "%s\n", q.c_str());
        std::string prev, buf;
        for (const Pos& p : ps) {
            if (p.name != prev) {
                if (!buf.empty()) fprintf(out, "%s %s\n", prev.c_str(), buf.c_str());
                prev = p.name; buf.clear();
            }
            if (!buf.empty()) buf += ",";
            buf += std::to_string(p.at);
        }
        if (!buf.empty()) fprintf(out, "%s %s\n", prev.c_str(), buf.c_str());
        fprintf(out, "//\n");
    }
}

int cmd_locate(const QueryArgs& a)
{
    OpenFile f(a.file);
    OutFile out;
    if (!out.open(a.output)) { fprintf(stderr, "Error: %s: cannot create\n", a.output.c_str()); return 1; }
    const std::vector<std::string> queries = expand_queries(a.positional);
    std::vector<Hit> hits;
    if (!search_all(f, a, queries, hits)) return 1;
    print_located(f.f, out.f, a.abs, queries, [&](size_t qi) { return hits[qi].found ? hits[qi].hi - hits[qi].lo : 0; },
                  [&](size_t qi, uint64_t k) { return sufr_file_suffix(f, hits[qi].lo + k); });
    return 0;
}

int cmd_extract(const QueryArgs& a)
{
    OpenFile f(a.file);
    OutFile out;
    if (!out.open(a.output)) { fprintf(stderr, "Error: %s: cannot create\n", a.output.c_str()); return 1; }
    sufr_file_meta m; sufr_file_metadata(f, &m);
    const uint8_t* text = sufr_file_text(f);
    const std::vector<std::string> queries = expand_queries(a.positional);
    std::vector<Hit> hits;
    if (!search_all(f, a, queries, hits)) return 1;
    for (size_t qi = 0; qi < queries.size(); qi++) {
        const std::string& q = queries[qi];
        const uint64_t lo = hits[qi].lo, hi = hits[qi].hi;
        if (!hits[qi].found) {
            fprintf(stderr, "%s not found\n", q.c_str());
            continue;
        }
        for (uint64_t r = lo; r < hi; r++) {          // SufrFile::extract (sufr_file.rs:898-960)
            const uint64_t sfx = sufr_file_suffix(f, r);
            const uint64_t i = sufr_file_sequence_of(f, sfx);
            const uint64_t seq_start = sufr_file_sequence_start(f, i);
            const uint64_t seq_end = i + 1 == m.num_sequences ? m.text_len : sufr_file_sequence_start(f, i + 1);
            const uint64_t rel = sfx - seq_start;
            const uint64_t cstart = rel > (a.has_prefix ? a.prefix_len : 0) ? rel - (a.has_prefix ? a.prefix_len : 0) : 0;
            uint64_t cend = a.has_suffix ? rel + a.suffix_len : seq_end;
            if (cend > seq_end) cend = seq_end;
            // string_at(sequence_start + range.start, Some(range.end - range.start)) (sufr_file.rs:399-411)
            const uint64_t from = seq_start + cstart;
            uint64_t to = from + (cend > cstart ? cend - cstart : 0);
            if (to > m.text_len) to = m.text_len;
            fprintf(out.f, ">%s:%llu-%llu %s %llu\n", sufr_file_sequence_name(f, i), (unsigned long long)cstart,
                    (unsigned long long)cend, q.c_str(), (unsigned long long)(rel - cstart));
            fwrite(text + from, 1, (size_t)(to > from ? to - from : 0), out.f);
            fputc('\n', out.f);
        }
    }
    return 0;
}

// parse_index / parse_pos (lib.rs:556-590): "3", "1,5", "2-4" (inclusive)
bool parse_ranks(const std::string& arg, std::vector<uint64_t>& out, std::string& err)
{
    size_t p = 0;
    while (p <= arg.size()) {
        size_t q = arg.find(',', p);
        if (q == std::string::npos) q = arg.size();
        const std::string val = arg.substr(p, q - p);
        auto is_num = [](const std::string& s) { return !s.empty() && s.find_first_not_of("0123456789") == std::string::npos; };
        const size_t dash = val.find('-');
        if (is_num(val)) out.push_back(strtoull(val.c_str(), nullptr, 10));
        else if (dash != std::string::npos && is_num(val.substr(0, dash)) && is_num(val.substr(dash + 1))) {
            const uint64_t n1 = strtoull(val.substr(0, dash).c_str(), nullptr, 10), n2 = strtoull(val.substr(dash + 1).c_str(), nullptr, 10);
            if (n1 >= n2) {
                err = "First number in range (" + std::to_string(n1) + ") must be lower than second number (" + std::to_string(n2) + ")";
                return false;
            }
            for (uint64_t v = n1; v <= n2; v++) out.push_back(v);
        } else { err = "illegal list value: \"" + val + "\""; return false; }
        p = q + 1;
    }
    return true;
}

int cmd_list(const QueryArgs& a)
{
    OpenFile f(a.file);
    OutFile out;
    if (!out.open(a.output)) { fprintf(stderr, "Error: %s: cannot create\n", a.output.c_str()); return 1; }
    std::vector<uint64_t> ranks;
    for (const std::string& r : a.positional) {
        std::string err;
        if (!parse_ranks(r, ranks, err)) { fprintf(stderr, "Error: %s\n", err.c_str()); return 1; }
    }
    sufr_file_meta m; sufr_file_metadata(f, &m);
    const uint8_t* text = sufr_file_text(f);
    const int width = (int)std::to_string(m.text_len).size();
    const uint64_t suffix_len = a.has_len ? a.len : m.text_len;
    auto print = [&](uint64_t rank) {                      // SufrFile::list (sufr_file.rs:1013-1077)
        const uint64_t sfx = sufr_file_suffix(f, rank);
        const uint64_t end = sfx + suffix_len > m.text_len ? m.text_len : sfx + suffix_len;
        if (a.show_rank) fprintf(out.f, "%*llu ", width, (unsigned long long)rank);
        if (a.show_suffix) fprintf(out.f, "%*llu ", width, (unsigned long long)sfx);
        if (a.show_lcp) fprintf(out.f, "%*llu ", width, (unsigned long long)sufr_file_lcp(f, rank));
        fwrite(text + sfx, 1, (size_t)(end - sfx), out.f);
        fputc('\n', out.f);
    };
    if (ranks.empty()) {
        const uint64_t number = a.has_number ? a.number : 0;
        for (uint64_t r = 0; r < m.len_suffixes; r++) {
            print(r);
            if (number > 0 && r == number - 1) break;
        }
    } else {
        for (uint64_t r : ranks) {
            if (r < m.len_suffixes) print(r);
            else fprintf(stderr, "Invalid rank: %llu\n", (unsigned long long)r);
        }
    }
    return 0;
}

// textwrap::wrap(s, width): greedy, breaks at spaces
std::vector<std::string> wrap_text(const std::string& s, size_t width)
{
    std::vector<std::string> lines;
    std::istringstream in(s);
    std::string w, cur;
    while (in >> w) {
        if (!cur.empty() && cur.size() + 1 + w.size() > width) { lines.push_back(cur); cur.clear(); }
        cur += (cur.empty() ? "" : " ") + w;
    }
    lines.push_back(cur);
    return lines;
}

int cmd_summarize(const QueryArgs& a)
{
    OpenFile f(a.file);
    sufr_file_meta m; sufr_file_metadata(f, &m);
    std::vector<std::pair<std::string, std::vector<std::string>>> rows;     // name, value lines
    auto row = [&](const std::string& k, const std::string& v) { rows.push_back({k, {v}}); };
    row("Filename", a.file);
    {
        char buf[64];
        time_t t = (time_t)m.modified;
        struct tm tmv;
        localtime_r(&t, &tmv);
        strftime(buf, sizeof buf, "%Y-%m-%d %H:%M", &tmv);
        row("Modified", buf);
    }
    row("File Size", with_commas(m.file_size) + " bytes");
    row("File Version", std::to_string(m.version));
    row("DNA", m.is_dna ? "true" : "false");
    row("Allow Ambiguity", m.allow_ambiguity ? "true" : "false");
    row("Ignore Softmask", m.ignore_softmask ? "true" : "false");
    row("Text Length", with_commas(m.text_len));
    row("Len Suffixes", with_commas(m.len_suffixes));
    if (m.seed_mask_len) {
        std::string mask;
        const uint8_t* mb = sufr_file_seed_mask(f);
        for (uint64_t i = 0; i < m.seed_mask_len; i++) mask += mb[i] ? '1' : '0';
        row("Seed mask", mask);
    } else row("Max query len", with_commas(m.max_query_len));
    row("Num sequences", with_commas(m.num_sequences));
    std::string starts, names;
    for (uint64_t i = 0; i < m.num_sequences; i++) {
        starts += (i ? ", " : "") + std::to_string(sufr_file_sequence_start(f, i));
        names += std::string(i ? ", " : "") + sufr_file_sequence_name(f, i);
    }
    rows.push_back({"Sequence starts", wrap_text(starts, 40)});
    rows.push_back({"Sequence names", wrap_text(names, 40)});
    // tabled's default style: +---+---+ between rows, cells padded by one blank
    size_t w0 = 0, w1 = 0;
    for (auto& r : rows) { w0 = std::max(w0, r.first.size()); for (auto& l : r.second) w1 = std::max(w1, l.size()); }
    const std::string rule = "+" + std::string(w0 + 2, '-') + "+" + std::string(w1 + 2, '-') + "+";
    printf("%s\n", rule.c_str());
    for (auto& r : rows) {
        for (size_t i = 0; i < r.second.size(); i++)
            printf("| %-*s | %-*s |\n", (int)w0, i == 0 ? r.first.c_str() : "", (int)w1, r.second[i].c_str());
        printf("%s\n", rule.c_str());
    }
    return 0;
}

// the queries of match / mems: the positional ones (named by themselves), then the records of -q FASTA / FASTQ
bool named_queries(const QueryArgs& a, std::vector<std::string>& names, std::vector<std::string>& seqs)
{
    names = expand_queries(a.positional);
    seqs = names;
    if (!a.reads.empty()) {
        sufr_sequence_data sd{};
        char err[512] = {0};
        if (sufr_read_sequence_file(a.reads.c_str(), '%', &sd, err, sizeof err) != 0) { fprintf(stderr, "Error: %s\n", err); return false; }
        for (uint64_t i = 0; i < sd.num_sequences; i++) {       // drop the delimiter after every sequence and the final sentinel
            const uint64_t b = sd.start_positions[i];
            const uint64_t e = i + 1 < sd.num_sequences ? sd.start_positions[i + 1] - 1 : (sd.seq_len ? sd.seq_len - 1 : 0);
            names.push_back(sd.sequence_names[i]);
            seqs.emplace_back((const char*)sd.seq + b, e > b ? e - b : 0);
        }
        sufr_sequence_data_free(&sd);
    }
    return true;
}

// The named queries of a command packed into one batch: what QuerySession and FmSession search
struct QueryBatch {
    std::vector<std::string> names;
    std::string bytes;                          // the queries, one after the other ...
    std::vector<uint64_t> off;                  // ... query i is bytes [off[i], off[i + 1])

    bool pack(const QueryArgs& a)
    {
        std::vector<std::string> seqs;
        if (!named_queries(a, names, seqs)) return false;
        off.assign(seqs.size() + 1, 0);
        for (size_t i = 0; i < seqs.size(); i++) { bytes += seqs[i]; off[i + 1] = bytes.size(); }
        return true;
    }
    const uint8_t* q() const { return (const uint8_t*)bytes.data(); }
    uint64_t nq() const { return off.size() - 1; }
};

// call(cap, &total) until the records fit: `cap` first, the exact count when that is short.  The code of the last call
template <typename Call>
int until_fits(uint64_t cap, uint64_t& total, Call call)
{
    for (;;) {
        const int rc = call(cap, &total);
        if (rc != SUFR_HIP_E_CAPACITY || total <= cap) return rc;
        cap = total;
    }
}

// What match, mems, approx and edit hold while they run: the .sufr file, the output, the named queries packed into one
// batch and, with --device, the index on that device.  Everything is released on every way out.
struct QuerySession : QueryBatch {
    sufr_file* f = nullptr;
    OutFile out;
    std::optional<DeviceIndex> dev;

    bool open(const QueryArgs& a)
    {
        f = open_or_die(a.file);
        if (!out.open(a.output)) { fprintf(stderr, "Error: %s: cannot create\n", a.output.c_str()); return false; }
        return true;
    }
    bool load(const QueryArgs& a)
    {
        if (!pack(a)) return false;
        if (a.device < 0) return true;
        dev.emplace(a.device, f);
        if (!dev->up()) { fprintf(stderr, "Error: %s\n", dev->error()); return false; }
        return true;
    }
    // the device is not held while the records are printed: the output may be large
    void release_device() { dev.reset(); }
    ~QuerySession() { release_device(); if (f) sufr_file_close(f); }
    QuerySession() = default;
    QuerySession(const QuerySession&) = delete;
    QuerySession& operator=(const QuerySession&) = delete;

    // ::until_fits with the report of a failure.  false: an error, printed
    // (`cmd` names the sub-command; ok_unsupported: an E_UNSUPPORTED whose text has it is no seed-mask refusal)
    template <typename Call>
    bool until_fits(const QueryArgs& a, const char* cmd, uint64_t cap, uint64_t& total, Call call, const char* ok_unsupported = nullptr)
    {
        const int rc = ::until_fits(cap, total, call);
        if (rc == SUFR_HIP_E_UNSUPPORTED && !(ok_unsupported && dev && strstr(dev->error(), ok_unsupported))) {
            fprintf(stderr, "Error: %s: %s does not support files built with a seed mask\n", a.file.c_str(), cmd);
            return false;
        }
        if (rc != 0) { fprintf(stderr, "Error: %s\n", dev ? dev->error() : (std::string(cmd) + " failed").c_str()); return false; }
        return true;
    }
};

// a text position as seq:pos (0-based inside the sequence), or absolute with --abs; the sequences are those of an open
// .sufr file or a SeqTable
template <typename Seqs>
std::string place(const Seqs& t, bool abs, uint64_t p)
{
    if (abs) return std::to_string(p);
    const uint64_t i = seq_of(t, p);
    return std::string(seq_name(t, i)) + ":" + std::to_string(p - seq_start(t, i));
}

// The lines of `sufr match` for `total` SMEM records: name, offset, length, count, positions.  positions(t) are the text
// positions of record t in rank order, at most max_hits of them: printed as they come with --abs, else as seq:pos ordered by
// sequence name, then position.  `sufr fm --smems` prints through here too, with the sequences of the index
template <typename Seqs, typename Positions>
void print_smems(const Seqs& seqs, FILE* out, bool abs, const std::vector<std::string>& names, uint64_t total, const std::vector<uint64_t>& qi,
                 const std::vector<uint32_t>& qo, const std::vector<uint32_t>& len, const std::vector<uint64_t>& lo, const std::vector<uint64_t>& hi,
                 Positions positions)
{
    for (uint64_t t = 0; t < total; t++) {
        const std::vector<uint64_t> where = positions(t);
        std::string pos;
        if (abs) for (size_t k = 0; k < where.size(); k++) pos += (k ? "," : "") + std::to_string(where[k]);
        else {
            struct Pos { uint64_t seq, at; };
            std::vector<Pos> ps;
            for (const uint64_t sfx : where) {
                const uint64_t i = seq_of(seqs, sfx);
                ps.push_back({i, sfx - seq_start(seqs, i)});
            }
            std::stable_sort(ps.begin(), ps.end(), [&](const Pos& x, const Pos& y) {
                const int c = x.seq == y.seq ? 0 : strcmp(seq_name(seqs, x.seq), seq_name(seqs, y.seq));
                return c ? c < 0 : x.at < y.at;
            });
            for (size_t k = 0; k < ps.size(); k++) pos += (k ? "," : "") + std::string(seq_name(seqs, ps[k].seq)) + ":" + std::to_string(ps[k].at);
        }
        fprintf(out, "%s\t%u\t%u\t%llu\t%s\n", names[qi[t]].c_str(), qo[t], len[t], (unsigned long long)(hi[t] - lo[t]), pos.c_str());
    }
}

// arguments of the query sub-commands (clap definitions of lib.rs:129-271)
// sufr match: the SMEMs of every query, one line each: name, offset, length, count, positions.
// Positions: SA[rank_lo .. rank_lo + max_hits) (all with 0), printed as seq:pos ordered by sequence name then position
// like locate's, or absolute in rank order with --abs.
int cmd_match(const QueryArgs& a)
{
    QuerySession s;
    if (!s.open(a)) return 1;
    if (a.min_len == 0 || a.min_len > 0xFFFFFFFFull) { fprintf(stderr, "Error: --min-len must be between 1 and 2^32 - 1\n"); return 1; }
    if (!s.load(a)) return 1;
    // records: room for one SMEM per 8 query bytes first, the exact count when that is short
    uint64_t total = 0;
    std::vector<uint64_t> qi, lo, hi;
    std::vector<uint32_t> qo, len;
    if (!s.until_fits(a, "match", s.bytes.size() / 8 + 16, total, [&](uint64_t cap, uint64_t* tot) {
            qi.resize(cap); lo.resize(cap); hi.resize(cap); qo.resize(cap); len.resize(cap);
            return s.dev ? sufr_hip_smems(s.dev->ctx, s.dev->ix, s.q(), s.off.data(), s.nq(), (uint32_t)a.min_len, cap, qi.data(), qo.data(), len.data(),
                                         lo.data(), hi.data(), tot)
                        : sufr_file_smems(s.f, s.q(), s.off.data(), s.nq(), (uint32_t)a.min_len, cap, qi.data(), qo.data(), len.data(), lo.data(),
                                          hi.data(), tot, a.threads);
        })) return 1;
    s.release_device();
    const sufr_file* f = s.f;
    print_smems(f, s.out.f, a.abs, s.names, total, qi, qo, len, lo, hi, [&](uint64_t t) {
        const uint64_t end = a.max_hits && hi[t] - lo[t] > a.max_hits ? lo[t] + a.max_hits : hi[t];
        std::vector<uint64_t> where;
        for (uint64_t r = lo[t]; r < end; r++) where.push_back(sufr_file_suffix(f, r));
        return where;
    });
    return 0;
}

// sufr mems: every MEM of every query, one line each in record order: name, strand (+ / -), offset (in
// the strand's coordinates), length, position as seq:pos (0-based) or absolute with --abs.
int cmd_mems(const QueryArgs& a)
{
    QuerySession s;
    if (!s.open(a)) return 1;
    if (a.min_len == 0 || a.min_len > 0xFFFFFFFFull) { fprintf(stderr, "Error: --min-len must be between 1 and 2^32 - 1\n"); return 1; }
    if (!s.load(a)) return 1;
    const uint32_t flags = a.both_strands ? SUFR_MEM_BOTH_STRANDS : 0;
    // records: room for one MEM per 4 query bytes first, the exact count when that is short
    uint64_t total = 0;
    std::vector<uint64_t> qi, pos;
    std::vector<uint32_t> qo, len;
    std::vector<uint8_t> st;
    if (!s.until_fits(a, "mems", s.bytes.size() / 4 + 16, total, [&](uint64_t cap, uint64_t* tot) {
            qi.resize(cap); pos.resize(cap); qo.resize(cap); len.resize(cap); st.resize(cap);
            return s.dev ? sufr_hip_mems(s.dev->ctx, s.dev->ix, s.q(), s.off.data(), s.nq(), (uint32_t)a.min_len, a.max_occ, flags, cap, qi.data(), qo.data(),
                                        st.data(), len.data(), pos.data(), tot)
                        : sufr_file_mems(s.f, s.q(), s.off.data(), s.nq(), (uint32_t)a.min_len, a.max_occ, flags, cap, qi.data(), qo.data(),
                                         st.data(), len.data(), pos.data(), tot, a.threads);
        })) return 1;
    s.release_device();
    for (uint64_t t = 0; t < total; t++)
        fprintf(s.out.f, "%s\t%c\t%u\t%u\t%s\n", s.names[qi[t]].c_str(), st[t] ? '-' : '+', qo[t], len[t], place(s.f, a.abs, pos[t]).c_str());
    return 0;
}

// sufr approx: every window of the text within -d mismatches of a query, one line each in record order:
// name, strand (+ / -), the window start as seq:pos (0-based) or absolute with --abs, mismatches.
int cmd_approx(const QueryArgs& a)
{
    if (a.mismatches > SUFR_APPROX_MAX_MISMATCHES) { fprintf(stderr, "Error: --mismatches must be at most %u\n", SUFR_APPROX_MAX_MISMATCHES); return 1; }
    QuerySession s;
    if (!s.open(a) || !s.load(a)) return 1;
    const uint32_t flags = a.both_strands ? SUFR_APPROX_BOTH_STRANDS : 0;
    // records: room for four windows per query first, the exact count when that is short
    uint64_t total = 0;
    std::vector<uint64_t> qi, pos;
    std::vector<uint8_t> st, mm;
    if (!s.until_fits(a, "approx", 4 * s.nq() + 16, total, [&](uint64_t cap, uint64_t* tot) {
            qi.resize(cap); pos.resize(cap); st.resize(cap); mm.resize(cap);
            return s.dev ? sufr_hip_approx(s.dev->ctx, s.dev->ix, s.q(), s.off.data(), s.nq(), (uint32_t)a.mismatches, a.max_occ, flags, cap, qi.data(),
                                          st.data(), pos.data(), mm.data(), tot)
                        : sufr_file_approx(s.f, s.q(), s.off.data(), s.nq(), (uint32_t)a.mismatches, a.max_occ, flags, cap, qi.data(), st.data(),
                                           pos.data(), mm.data(), tot, a.threads);
        })) return 1;
    s.release_device();
    for (uint64_t t = 0; t < total; t++)
        fprintf(s.out.f, "%s\t%c\t%s\t%u\n", s.names[qi[t]].c_str(), st[t] ? '-' : '+', place(s.f, a.abs, pos[t]).c_str(), (unsigned)mm[t]);
    return 0;
}

// What `sufr fm` holds while it runs (DESIGN.md sections 23 - 26): the output, the named queries packed into one batch, one
// FM-index or the pair of --smems (that of the text and that of the reversed text), the sequences of the text and, with
// --device, the context and every device allocation.  An index comes from an index file or is built from a .sufr, which is
// closed again at once: the index answers alone.  Everything is released on every way out.
struct FmSession : QueryBatch {
    struct Index {
        sufr_fm* host = nullptr;                // loaded, built on the host, or downloaded for --save
        sufr_hip_fm* dev = nullptr;             // with --device: uploaded or built there; it answers when it is there
        sufr_fm_info info{};
        sufr_fm_text_info text{};
    };
    const int device, threads;
    const bool pair;                            // --smems: the library checks the files and names all it asks in one text
    OutFile out;
    sufr_hip_ctx* ctx = nullptr;                // made by the first step that needs the device
    SeqTable seqs;
    Index ix[2];
    std::vector<void*> allocations;
    std::vector<uint64_t> loff;                 // of the last locate: range i has the positions loff[i] .. loff[i + 1] ...
    std::vector<uint8_t> pos;                   // ... of info.width bytes each

    FmSession(const QueryArgs& a, bool pair) : device(a.device), threads(a.threads), pair(pair) {}
    // the device is not held while the records are printed: the output may be large
    void release()
    {
        for (void* p : allocations) (void)hipFree(p);
        allocations.clear();
        for (Index& x : ix) {
            if (x.dev) sufr_hip_fm_free(x.dev);
            if (x.host) sufr_fm_free(x.host);
            x.dev = nullptr; x.host = nullptr;
        }
        if (ctx) sufr_hip_destroy(ctx);
        ctx = nullptr;
    }
    ~FmSession() { release(); }
    FmSession(const FmSession&) = delete;
    FmSession& operator=(const FmSession&) = delete;

    bool fail(const char* what) const { fprintf(stderr, "Error: %s\n", what); return false; }
    bool open(const std::string& output) { return out.open(output) || fail((output + ": cannot create").c_str()); }
    bool device_up() { return ctx || (ctx = sufr_hip_create(device)); }
    const char* device_error() const { return sufr_hip_last_error(ctx); }      // (no context: the text of the failed create)

    // Why a .sufr file gives no FM-index: by its metadata (nullptr: nothing against it), and for a build that refused
    const char* refusal(const sufr_file_meta& m) const
    {
        return pair                                          ? nullptr
               : m.len_suffixes != m.text_len || !m.text_len ? "the file leaves text positions out (every position must be indexed: --dna needs --allow-ambiguity)"
               : m.seed_mask_len                             ? "the file was built with a seed mask"
               : m.max_query_len                             ? "the file was built with a max_query_len"
                                                             : nullptr;
    }
    const char* refusal() const
    {
        return pair ? "every position must be indexed, without seed mask and max_query_len, and the last byte must occur once"
                    : "the last byte of the text occurs more than once";
    }

    // Index `slot` from `path`: an index file (loaded and verified; with --device uploaded), or a .sufr file whose index is
    // built at `sample` with `flags`, on the device with --device, and written to `save` unless that is empty.  want_names:
    // its sequences are those of the output.  false: an error, printed
    bool take(const std::string& path, bool index_file, uint64_t sample, uint32_t flags, bool want_names, const std::string& save, int slot)
    {
        Index& x = ix[slot];
        char err[512] = {0};
        if (index_file) {
            if (sufr_fm_load(path.c_str(), &x.host, threads, err, sizeof err) != 0) return fail(err);
            if (device >= 0 && (!device_up() || sufr_hip_fm_upload(ctx, x.host, &x.dev) != 0)) return fail(device_error());
            for (uint64_t i = 0; want_names && i < sufr_fm_num_sequences(x.host); i++) {
                seqs.starts.push_back(sufr_fm_sequence_start(x.host, i));
                seqs.names.push_back(sufr_fm_sequence_name(x.host, i));
            }
        } else {
            OpenFile f(path);
            sufr_file_meta m;
            sufr_file_metadata(f, &m);
            const char* why = refusal(m);
            if (!why && device >= 0) {
                sufr_hip_index* text_sa = nullptr;
                if (!device_up() || sufr_hip_index_load(ctx, f, &text_sa) != 0) return fail(device_error());
                const int rc = sufr_hip_fm_build_flags(ctx, text_sa, sample, flags, &x.dev);
                sufr_hip_index_free(text_sa);   // text and suffix array leave the device: the FM-index answers alone
                if (rc) why = rc == SUFR_HIP_E_UNSUPPORTED && !pair ? refusal() : device_error();
                else if (!save.empty() && sufr_hip_fm_download(ctx, x.dev, &x.host) != 0) return fail(device_error());
            } else if (!why) {
                const int rc = sufr_file_fm_build_flags(f, sample, flags, &x.host, threads);
                if (rc) why = rc == SUFR_HIP_E_UNSUPPORTED ? refusal() : "the build failed";
            }
            if (why) { fprintf(stderr, "Error: %s: no FM-index: %s\n", path.c_str(), why); return false; }
            for (uint64_t i = 0; want_names && i < m.num_sequences; i++) {
                seqs.starts.push_back(sufr_file_sequence_start(f, i));
                seqs.names.push_back(sufr_file_sequence_name(f, i));
            }
            if (!save.empty() && sufr_fm_save(x.host, save.c_str(), f, err, sizeof err) != 0) return fail(err);
        }
        if (x.dev ? sufr_hip_fm_get_info(x.dev, &x.info) || sufr_hip_fm_get_text_info(x.dev, &x.text)
                  : sufr_fm_get_info(x.host, &x.info) || sufr_fm_get_text_info(x.host, &x.text))
            return fail("reading the info of the FM-index failed");
        return true;
    }

    // device memory, released with the session.  nullptr: an error, printed
    uint8_t* alloc(uint64_t bytes)
    {
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) { fail("device memory for the batch"); return nullptr; }
        allocations.push_back(p);
        return (uint8_t*)p;
    }
    static bool copy(void* to, const void* from, uint64_t bytes, hipMemcpyKind kind) { return !bytes || hipMemcpy(to, from, bytes, kind) == hipSuccess; }
    bool copied(bool ok) const { return ok || fail("copying the batch"); }
    // after a device call: waits for it.  false: an error, printed
    bool done(int rc) const { return !(rc ? rc : sufr_hip_synchronize(ctx)) || fail(device_error()); }

    // The rank range of every query in index 0: lo, hi.  false: an error, printed
    bool search(std::vector<uint64_t>& lo, std::vector<uint64_t>& hi)
    {
        const uint64_t n = nq();
        lo.assign(n, 0); hi.assign(n, 0);
        if (!ix[0].dev) {
            const int rc = sufr_fm_search_batch(ix[0].host, q(), off.data(), n, lo.data(), hi.data(), threads);
            if (rc) fprintf(stderr, "Error: the FM-index search failed (%d)\n", rc);
            return !rc;
        }
        // one allocation: queries | offsets | lo | hi
        const uint64_t o_at = (bytes.size() + 7) / 8 * 8, lo_at = o_at + (n + 1) * 8, hi_at = lo_at + n * 8;
        uint8_t* d = alloc(hi_at + n * 8);
        if (!d) return false;
        return copied(copy(d, bytes.data(), bytes.size(), hipMemcpyHostToDevice) && copy(d + o_at, off.data(), (n + 1) * 8, hipMemcpyHostToDevice)) &&
               done(sufr_hip_fm_search_batch_device(ctx, ix[0].dev, d, d + o_at, n, d + lo_at, d + hi_at)) &&
               copied(copy(lo.data(), d + lo_at, n * 8, hipMemcpyDeviceToHost) && copy(hi.data(), d + hi_at, n * 8, hipMemcpyDeviceToHost));
    }

    // The text positions of the first `n` rank ranges lo[i] .. hi[i] in index 0, at most max_hits of each (0: all), in rank
    // order: loff and pos.  false: an error, printed
    bool locate(const std::vector<uint64_t>& lo, const std::vector<uint64_t>& hi, uint64_t n, uint64_t max_hits)
    {
        const uint64_t w = ix[0].info.width;
        uint64_t total = 0;
        for (uint64_t i = 0; i < n; i++) total += max_hits && hi[i] - lo[i] > max_hits ? max_hits : hi[i] - lo[i];
        loff.assign(n + 1, 0);
        pos.assign((total + 1) * w, 0);
        if (!n) return true;
        if (!ix[0].dev) {
            const int rc = sufr_fm_locate_batch(ix[0].host, lo.data(), hi.data(), n, max_hits, loff.data(), pos.data(), total, &total, threads);
            if (rc) fprintf(stderr, "Error: the FM-index locate failed (%d)\n", rc);
            return !rc;
        }
        // one allocation: lo | hi | the offsets | the positions
        const uint64_t hi_at = n * 8, l_at = 2 * n * 8, p_at = l_at + (n + 1) * 8;
        uint8_t* d = alloc(p_at + (total + 1) * w);
        if (!d) return false;
        return copied(copy(d, lo.data(), n * 8, hipMemcpyHostToDevice) && copy(d + hi_at, hi.data(), n * 8, hipMemcpyHostToDevice)) &&
               done(sufr_hip_fm_locate_batch_device(ctx, ix[0].dev, d, d + hi_at, n, max_hits, d + l_at, d + p_at, total, &total)) &&
               copied(copy(loff.data(), d + l_at, (n + 1) * 8, hipMemcpyDeviceToHost) && copy(pos.data(), d + p_at, total * w, hipMemcpyDeviceToHost));
    }
    // position `at` of the last locate (little-endian entries of 4 or 8 bytes)
    uint64_t position(uint64_t at) const
    {
        uint64_t p = 0;
        memcpy(&p, pos.data() + at * ix[0].info.width, ix[0].info.width);
        return p;
    }

    // call(cap, &total) until the records fit (::until_fits).  false: an error, printed
    template <typename Call>
    bool records(uint64_t cap, uint64_t& total, Call call)
    {
        return !::until_fits(cap, total, call) || fail(ctx ? device_error() : "the FM-index search failed");
    }
};

// sufr fm (include/sufr_fm.h, sufr_fm_approx.h, sufr_fm_text.h; DESIGN.md sections 23 - 25): count, with --locate locate, with
// --mismatches the windows within D mismatches by backtracking, with --extract the lines of extract (the hits through locate,
// the bases read back from the BWT), through an FM-index alone.  The index is built from the .sufr file (on the GPU with
// --device) or loaded from an index file (--index: no .sufr is opened, the sequence names are the file's; with --device it is
// uploaded); --save writes it.  The lines are those of count, locate, approx (in (query, strand, leaf, rank) order) and extract.
int cmd_fm(const QueryArgs& a)
{
    if (a.fm_approx && a.mismatches > SUFR_FM_APPROX_MAX_MISMATCHES) { fprintf(stderr, "Error: --mismatches must be at most %u\n", SUFR_FM_APPROX_MAX_MISMATCHES); return 1; }
    const bool want_text = a.fm_text || a.fm_extract, locate = a.locate || a.fm_extract;
    if (want_text && !a.sample) { fprintf(stderr, "Error: --text and --extract need the sampled suffixes: -s must be at least 1\n"); return 1; }
    if (a.fm_approx && !a.sample) { fprintf(stderr, "Error: --mismatches needs the sampled suffixes: -s must be at least 1\n"); return 1; }
    // An index that only counts keeps no suffixes.  -s 0 with --locate alone has always meant 1; with --index, --save, --text
    // or --extract it is taken as given, and an index without samples then refuses to locate
    const bool as_given = !a.fm_index.empty() || !a.fm_save.empty() || want_text;
    uint64_t sample = locate || a.fm_approx || !a.fm_save.empty() ? a.sample : 0;
    if (a.locate && !sample && !as_given) sample = 1;
    FmSession s(a, false);
    if (!s.open(a.output) || !s.take(a.file, !a.fm_index.empty(), sample, want_text ? SUFR_FM_TEXT : 0, true, a.fm_save, 0) || !s.pack(a)) return 1;
    const uint64_t nq = s.nq();
    if (!nq) return 0;                          // (--save alone)
    const FmSession::Index& x = s.ix[0];
    if ((locate || a.fm_approx) && !x.info.sample) {
        fprintf(stderr, "Error: %s: the index was saved without samples (-s 0): it counts only\n", a.file.c_str());
        return 1;
    }
    if (a.fm_extract && !x.text.text_samples) {
        fprintf(stderr, "Error: %s: the index was saved without --text: it cannot give the text back\n", a.file.c_str());
        return 1;
    }
    if (a.fm_approx) {
        const uint32_t flags = a.both_strands ? SUFR_FM_APPROX_BOTH_STRANDS : 0, d = (uint32_t)a.mismatches;
        // records: room for four windows per query first, the exact count when that is short
        uint64_t total = 0;
        std::vector<uint64_t> qi, pos;
        std::vector<uint8_t> st, mm;
        if (!s.records(4 * nq + 16, total, [&](uint64_t cap, uint64_t* tot) {
                qi.resize(cap); pos.resize(cap); st.resize(cap); mm.resize(cap);
                return x.dev ? sufr_hip_fm_approx(s.ctx, x.dev, s.q(), s.off.data(), nq, d, flags, cap, qi.data(), st.data(), pos.data(), mm.data(), tot)
                             : sufr_fm_approx(x.host, s.q(), s.off.data(), nq, d, flags, cap, qi.data(), st.data(), pos.data(), mm.data(), tot, a.threads);
            })) return 1;
        s.release();
        for (uint64_t t = 0; t < total; t++)
            fprintf(s.out.f, "%s\t%c\t%s\t%u\n", s.names[qi[t]].c_str(), st[t] ? '-' : '+', place(s.seqs, a.abs, pos[t]).c_str(), (unsigned)mm[t]);
        return 0;
    }
    std::vector<uint64_t> lo, hi;
    if (!s.search(lo, hi)) return 1;
    if (!locate) {
        for (size_t i = 0; i < nq; i++) fprintf(s.out.f, "%s %llu\n", s.names[i].c_str(), (unsigned long long)(hi[i] - lo[i]));
        return 0;
    }
    if (!s.locate(lo, hi, nq, a.fm_extract ? 0 : a.max_hits)) return 1;
    const std::vector<uint64_t>& loff = s.loff;
    if (!a.fm_extract) {
        s.release();
        print_located(s.seqs, s.out.f, a.abs, s.names, [&](size_t qi) { return loff[qi + 1] - loff[qi]; }, [&](size_t qi, uint64_t k) { return s.position(loff[qi] + k); });
        return 0;
    }
    // the lines of cmd_extract: the range of every hit, then all of them read back in one batch
    const uint64_t n = x.info.ranks, total = loff[nq];
    struct Line { uint64_t seq, cstart, cend, at; };
    std::vector<Line> lines(total);
    std::vector<uint64_t> starts(total), ends(total), boff(total + 1, 0);
    for (uint64_t t = 0; t < total; t++) {
        const uint64_t sfx = s.position(t), i = seq_of(s.seqs, sfx), s0 = seq_start(s.seqs, i);
        const uint64_t seq_end = i + 1 >= s.seqs.starts.size() ? n : s.seqs.starts[i + 1];
        const uint64_t rel = sfx - s0, pre = a.has_prefix ? a.prefix_len : 0;
        const uint64_t cstart = rel > pre ? rel - pre : 0;
        uint64_t cend = a.has_suffix ? rel + a.suffix_len : seq_end;
        if (cend > seq_end) cend = seq_end;
        lines[t] = Line{i, cstart, cend, rel - cstart};
        starts[t] = s0 + cstart;
        ends[t] = starts[t] + (cend > cstart ? cend - cstart : 0);
    }
    uint64_t nbytes = 0;
    for (uint64_t t = 0; t < total; t++) {      // (the clipping of the extract contract)
        const uint64_t e = ends[t] < n ? ends[t] : n;
        nbytes += e - (starts[t] < e ? starts[t] : e);
    }
    std::vector<uint8_t> text(nbytes + 1);
    const int rc = x.dev ? sufr_hip_fm_extract_batch(s.ctx, x.dev, starts.data(), ends.data(), total, boff.data(), text.data(), nbytes, &nbytes)
                         : sufr_fm_extract_batch(x.host, starts.data(), ends.data(), total, boff.data(), text.data(), nbytes, &nbytes, a.threads);
    if (rc) { s.fail(x.dev ? s.device_error() : "the FM-index extract failed"); return 1; }
    for (size_t qi = 0; qi < nq; qi++) {
        if (loff[qi + 1] == loff[qi]) { fprintf(stderr, "%s not found\n", s.names[qi].c_str()); continue; }
        for (uint64_t t = loff[qi]; t < loff[qi + 1]; t++) {
            fprintf(s.out.f, ">%s:%llu-%llu %s %llu\n", seq_name(s.seqs, lines[t].seq), (unsigned long long)lines[t].cstart, (unsigned long long)lines[t].cend,
                    s.names[qi].c_str(), (unsigned long long)lines[t].at);
            fwrite(text.data() + boff[t], 1, (size_t)(boff[t + 1] - boff[t]), s.out.f);
            fputc('\n', s.out.f);
        }
    }
    return 0;
}

// sufr fm <SUFR> --write-reverse OUT.fa (include/sufr_fm_match.h): the FASTA of the reversed text
int cmd_fm_write_reverse(const QueryArgs& a)
{
    if (!a.fm_index.empty()) { fprintf(stderr, "Error: --write-reverse needs the text: a .sufr file, not --index\n"); return 1; }
    char err[512] = {0};
    OpenFile f(a.file);
    if (sufr_file_write_reversed_fasta(f, a.fm_write_reverse.c_str(), err, sizeof err) != 0) { fprintf(stderr, "Error: %s\n", err); return 1; }
    return 0;
}

// sufr fm --smems --reverse REV: the lines of `sufr match` from two FM-indexes alone, the one of the
// text (built from <SUFR> at -s, or loaded with --index) and the one of the reversed text (REV: an index file, told by its
// magic, or the .sufr of the reversed FASTA, whose index is built at sample 0), on the GPU with --device.
int cmd_fm_smems(const QueryArgs& a)
{
    if (!a.fm_smems) { fprintf(stderr, "Error: --reverse goes with --smems\n"); return 1; }
    if (a.fm_reverse.empty()) { fprintf(stderr, "Error: --smems needs --reverse REV: the .sufr or the FM-index of the reversed text (sufr fm --write-reverse)\n"); return 1; }
    if (a.fm_index.empty() && !a.sample) { fprintf(stderr, "Error: --smems prints positions, which need the sampled suffixes: -s must be at least 1\n"); return 1; }
    if (a.min_len == 0 || a.min_len > 0xFFFFFFFFull) { fprintf(stderr, "Error: --min-len must be between 1 and 2^32 - 1\n"); return 1; }
    FmSession s(a, true);
    if (!s.open(a.output)) return 1;
    // an index file is told from a .sufr by its magic
    char magic[8] = {0};
    if (FILE* fp = fopen(a.fm_reverse.c_str(), "rb")) { if (fread(magic, 1, 8, fp) != 8) magic[0] = 0; fclose(fp); }
    else { fprintf(stderr, "Error: %s: %s\n", a.fm_reverse.c_str(), strerror(errno)); return 1; }
    if (!s.take(a.file, !a.fm_index.empty(), a.sample, 0, true, "", 0) || !s.take(a.fm_reverse, !memcmp(magic, "SUFRFMI\0", 8), 0, 0, false, "", 1)) return 1;
    const FmSession::Index &fwd = s.ix[0], &rev = s.ix[1];
    if (!fwd.info.sample) { fprintf(stderr, "Error: %s: the index was saved without samples (-s 0): it gives no positions\n", a.file.c_str()); return 1; }
    // (on the device the library checks the pair)
    if (a.device < 0 && sufr_fm_pair_check(fwd.host, rev.host) != 0) { fprintf(stderr, "Error: %s: not an index of the reversed text\n", a.fm_reverse.c_str()); return 1; }
    if (!s.pack(a)) return 1;
    // records: room for one SMEM per 8 query bytes first, the exact count when that is short
    uint64_t total = 0;
    std::vector<uint64_t> qi, lo, hi;
    std::vector<uint32_t> qo, len;
    if (!s.records(s.bytes.size() / 8 + 16, total, [&](uint64_t cap, uint64_t* tot) {
            qi.resize(cap); lo.resize(cap); hi.resize(cap); qo.resize(cap); len.resize(cap);
            return fwd.dev ? sufr_hip_fm_smems(s.ctx, fwd.dev, rev.dev, s.q(), s.off.data(), s.nq(), (uint32_t)a.min_len, cap, qi.data(), qo.data(), len.data(),
                                               lo.data(), hi.data(), tot)
                           : sufr_fm_smems(fwd.host, rev.host, s.q(), s.off.data(), s.nq(), (uint32_t)a.min_len, cap, qi.data(), qo.data(), len.data(), lo.data(),
                                           hi.data(), tot, a.threads);
        })) return 1;
    // the positions of every SMEM: locate on the index of the text
    if (!s.locate(lo, hi, total, a.max_hits)) return 1;
    s.release();
    print_smems(s.seqs, s.out.f, a.abs, s.names, total, qi, qo, len, lo, hi, [&](uint64_t t) {
        std::vector<uint64_t> where(s.loff[t + 1] - s.loff[t], 0);
        for (size_t k = 0; k < where.size(); k++) where[k] = s.position(s.loff[t] + k);
        return where;
    });
    return 0;
}

// sufr edit: every text position where a query ends with at most -d edits, one line each in record
// order (query, strand, end): name, strand (+ / -), the end as seq:offset (0-based) or absolute with --abs, edits.
// -c: the records are traced back (on the device with --device); two more columns, the start in the
// form of the end and the CIGAR.
int cmd_edit(const QueryArgs& a)
{
    if (a.edits > SUFR_EDIT_MAX_EDITS) { fprintf(stderr, "Error: --edits must be at most %u\n", SUFR_EDIT_MAX_EDITS); return 1; }
    QuerySession s;
    if (!s.open(a) || !s.load(a)) return 1;
    const uint32_t flags = (a.both_strands ? SUFR_EDIT_BOTH_STRANDS : 0) | (a.local_minima ? SUFR_EDIT_LOCAL_MINIMA : 0);
    // records: room for a hill of ends per query first, the exact count when that is short
    uint64_t total = 0;
    std::vector<uint64_t> qi, end;
    std::vector<uint8_t> st, ed;
    if (!s.until_fits(a, "edit", (2 * a.edits + 1) * s.nq() + 16, total, [&](uint64_t cap, uint64_t* tot) {
            qi.resize(cap); end.resize(cap); st.resize(cap); ed.resize(cap);
            return s.dev ? sufr_hip_edit(s.dev->ctx, s.dev->ix, s.q(), s.off.data(), s.nq(), (uint32_t)a.edits, a.max_occ, flags, cap, qi.data(), st.data(),
                                        end.data(), ed.data(), tot)
                        : sufr_file_edit(s.f, s.q(), s.off.data(), s.nq(), (uint32_t)a.edits, a.max_occ, flags, cap, qi.data(), st.data(), end.data(),
                                         ed.data(), tot, a.threads);
        }, "sort key")) return 1;
    // -c: the sizing call, then the runs
    std::vector<uint64_t> start(total + 1), coff(total + 1, 0);
    std::vector<uint32_t> cigar;
    if (a.cigar && total) {
        char err[512] = "";
        uint64_t runs = 0;
        for (int pass = 0; pass < 2; pass++) {
            const int rc = s.dev ? sufr_hip_edit_trace(s.dev->ctx, s.dev->ix, s.q(), s.off.data(), s.nq(), total, qi.data(), st.data(), end.data(), ed.data(),
                                                      cigar.size(), start.data(), coff.data(), cigar.empty() ? nullptr : cigar.data(), &runs)
                                : sufr_file_edit_trace(s.f, s.q(), s.off.data(), s.nq(), total, qi.data(), st.data(), end.data(), ed.data(),
                                                       cigar.size(), start.data(), coff.data(), cigar.empty() ? nullptr : cigar.data(), &runs,
                                                       a.threads, err, sizeof err);
            if (rc == SUFR_HIP_E_CAPACITY && pass == 0) { cigar.resize(runs); continue; }
            if (rc != 0) { fprintf(stderr, "Error: %s\n", s.dev ? s.dev->error() : err); return 1; }
            break;
        }
    }
    s.release_device();
    for (uint64_t t = 0; t < total; t++) {
        fprintf(s.out.f, "%s\t%c\t%s\t%u", s.names[qi[t]].c_str(), st[t] ? '-' : '+', place(s.f, a.abs, end[t]).c_str(), (unsigned)ed[t]);
        if (a.cigar) {
            fprintf(s.out.f, "\t%s\t", place(s.f, a.abs, start[t]).c_str());
            for (uint64_t r = coff[t]; r < coff[t + 1]; r++) {
                const uint32_t op = cigar[r] & 15u;
                fprintf(s.out.f, "%u%c", cigar[r] >> 4, op == 1 ? 'I' : op == 2 ? 'D' : op == 7 ? '=' : 'X');
            }
        }
        fputc('\n', s.out.f);
    }
    return 0;
}

int run_query(const std::string& cmd, int argc, char** argv, int first, int threads)
{
    QueryArgs a;
    a.threads = threads;
    std::vector<std::string> pos;
    auto need = value_reader(argc, argv);
    const bool is_list = cmd == "list", is_extract = cmd == "extract", is_locate = cmd == "locate", is_sum = cmd == "summarize";
    const bool is_edit = cmd == "edit", is_fm = cmd == "fm";
    const bool is_approx = cmd == "approx" || is_edit;
    const bool is_mems = cmd == "mems";
    const bool is_match = cmd == "match" || is_mems || is_approx;
    for (int i = first; i < argc; i++) {
        const std::string s = argv[i];
        if (s == "-h" || s == "--help") { usage(stdout); return 0; }
        else if (is_fm && s == "--locate") a.locate = true;
        else if (is_fm && (s == "-s" || s == "--sample")) a.sample = strtoull(need(i, "-s"), nullptr, 10);
        else if (is_fm && s == "--save") a.fm_save = need(i, "--save");
        else if (is_fm && s == "--index") a.fm_index = need(i, "--index");
        else if (is_fm && s == "--text") a.fm_text = true;
        else if (is_fm && s == "--extract") a.fm_extract = true;
        else if (is_fm && s == "--smems") a.fm_smems = true;
        else if (is_fm && s == "--reverse") a.fm_reverse = need(i, "--reverse");
        else if (is_fm && s == "--write-reverse") a.fm_write_reverse = need(i, "--write-reverse");
        else if (is_fm && (s == "-k" || s == "--min-len")) a.min_len = strtoull(need(i, "-k"), nullptr, 10);
        else if (is_fm && s == "--prefix-len") { a.has_prefix = true; a.prefix_len = strtoull(need(i, "--prefix-len"), nullptr, 10); }
        else if (is_fm && s == "--suffix-len") { a.has_suffix = true; a.suffix_len = strtoull(need(i, "--suffix-len"), nullptr, 10); }
        else if (is_fm && s == "--max-hits") a.max_hits = strtoull(need(i, "--max-hits"), nullptr, 10);
        else if (is_fm && (s == "-t" || s == "--threads")) a.threads = atoi(need(i, "-t"));
        else if (!is_list && !is_sum && !is_match && !is_fm && (s == "-m" || s == "--max-query-len")) { a.has_mql = true; a.mql = strtoull(need(i, "-m"), nullptr, 10); }
        else if (!is_sum && (s == "-o" || s == "--output")) a.output = need(i, "-o");
        else if (!is_list && !is_sum && ((s == "-l" && !is_edit) || s == "--low-memory")) {}   // access mode only: the file is mapped (edit: -l is --local-minima)
        else if (!is_sum && (s == "-v" || s == "--very-low-memory")) {}
        else if (!is_list && !is_sum && s == "--device") a.device = atoi(need(i, "--device"));
        else if ((is_locate || is_match || is_fm) && (s == "-a" || s == "--abs")) a.abs = true;
        else if (is_match && !is_approx && (s == "-k" || s == "--min-len")) a.min_len = strtoull(need(i, "-k"), nullptr, 10);
        else if ((is_mems || is_approx) && s == "--max-occ") a.max_occ = strtoull(need(i, "--max-occ"), nullptr, 10);
        else if ((is_mems || is_approx || is_fm) && (s == "-b" || s == "--both-strands")) a.both_strands = true;
        else if (is_fm && (s == "-d" || s == "--mismatches")) { a.fm_approx = true; a.mismatches = strtoull(need(i, "-d"), nullptr, 10); }
        else if (is_edit && (s == "-d" || s == "--edits")) a.edits = strtoull(need(i, "-d"), nullptr, 10);
        else if (is_edit && (s == "-l" || s == "--local-minima")) a.local_minima = true;
        else if (is_edit && (s == "-c" || s == "--cigar")) a.cigar = true;
        else if (is_approx && !is_edit && (s == "-d" || s == "--mismatches")) a.mismatches = strtoull(need(i, "-d"), nullptr, 10);
        else if (is_match && !is_mems && !is_approx && (s == "-n" || s == "--max-hits")) a.max_hits = strtoull(need(i, "-n"), nullptr, 10);
        else if ((is_match || is_fm) && (s == "-q" || s == "--reads")) a.reads = need(i, "-q");
        else if (is_extract && (s == "-p" || s == "--prefix-len")) { a.has_prefix = true; a.prefix_len = strtoull(need(i, "-p"), nullptr, 10); }
        else if (is_extract && (s == "-s" || s == "--suffix-len")) { a.has_suffix = true; a.suffix_len = strtoull(need(i, "-s"), nullptr, 10); }
        else if (is_list && (s == "-r" || s == "--show-rank")) a.show_rank = true;
        else if (is_list && (s == "-s" || s == "--show-suffix")) a.show_suffix = true;
        else if (is_list && (s == "-p" || s == "--show-lcp")) a.show_lcp = true;
        else if (is_list && s == "--len") { a.has_len = true; a.len = strtoull(need(i, "--len"), nullptr, 10); }
        else if (is_list && (s == "-n" || s == "--number")) { a.has_number = true; a.number = strtoull(need(i, "-n"), nullptr, 10); }
        else if (is_list && s.size() > 2 && s[0] == '-' && s[1] != '-' && s.find_first_not_of("rspv", 1) == std::string::npos) {
            for (size_t k = 1; k < s.size(); k++) {     // combined short flags: -rsp
                if (s[k] == 'r') a.show_rank = true; else if (s[k] == 's') a.show_suffix = true; else if (s[k] == 'p') a.show_lcp = true;
            }
        }
        else if (!s.empty() && s[0] == '-' && s.size() > 1) { fprintf(stderr, "error: unexpected argument '%s'\n", s.c_str()); return 2; }
        else pos.push_back(s);
    }
    if (!a.fm_index.empty()) pos.insert(pos.begin(), a.fm_index);      // (fm --index: the index file stands where the .sufr would)
    if (pos.empty()) { fprintf(stderr, "error: the following required arguments were not provided:\n  <%s>\n", is_list ? "FILE" : "SUFR"); return 2; }
    a.file = pos[0];
    a.positional.assign(pos.begin() + 1, pos.end());
    if (!is_list && !is_sum && a.positional.empty() && !((is_match || is_fm) && !a.reads.empty()) && a.fm_save.empty() && a.fm_write_reverse.empty()) {
        fprintf(stderr, "error: the following required arguments were not provided:\n  <QUERY>...\n");
        return 2;
    }
    if (cmd == "count") return cmd_count(a);
    if (is_locate) return cmd_locate(a);
    if (is_fm && !a.fm_write_reverse.empty()) {
        const int rc = cmd_fm_write_reverse(a);
        if (rc || !(a.fm_smems || !a.fm_reverse.empty())) return rc;
    }
    if (is_fm) return a.fm_smems || !a.fm_reverse.empty() ? cmd_fm_smems(a) : cmd_fm(a);
    if (is_edit) return cmd_edit(a);
    if (is_approx) return cmd_approx(a);
    if (is_mems) return cmd_mems(a);
    if (is_match) return cmd_match(a);
    if (is_extract) return cmd_extract(a);
    if (is_list) return cmd_list(a);
    return cmd_summarize(a);
}

// ---------------------------------------------------------------------------------------------------------------
// the analyses of the indexed text from its arrays: kmers, repeats, shared, lz (SA + LCP) and bwt (SA + text)
// ---------------------------------------------------------------------------------------------------------------
// What they hold while they run: the arguments they share, the .sufr file with its metadata and sequence starts, the
// output and, with --device, the index on that device and every device allocation (the LCP array is the first).  The
// first failure stays in `rc` (with a text of the session's own in `err` for allocations and copies) and turns the steps
// after it into no-ops, so a command reads top to bottom and asks once, in computed().  Everything is released on every
// way out.
struct AnalysisSession {
    std::string file, output;
    int device = -1;
    sufr_file* f = nullptr;
    sufr_file_meta m;
    std::vector<uint64_t> starts;               // of the sequences: what the *_device calls take beside the LCP array
    std::optional<DeviceIndex> dev;
    void* d_lcp = nullptr;
    bool need_lcp = true;                       // false: the command reads no LCP array (bwt), none is copied to the device
    std::vector<void*> allocations;
    OutFile out;
    int rc = 0;
    std::string err;

    // the arguments behind the sub-command: own(s, i, need) takes the command's options, the rest is the same for all.
    // Returns the exit status, or -1 to go on
    template <typename Own>
    int parse(int argc, char** argv, int first, Own own)
    {
        auto need = value_reader(argc, argv);
        for (int i = first; i < argc; i++) {
            const std::string s = argv[i];
            if (s == "-h" || s == "--help") { usage(stdout); return 0; }
            else if (own(s, i, need)) {}
            else if (s == "--device") device = atoi(need(i, "--device"));
            else if (s == "-o" || s == "--output") output = need(i, "-o");
            else if (s.size() > 1 && s[0] == '-') { fprintf(stderr, "error: unexpected argument '%s'\n", s.c_str()); return 2; }
            else if (file.empty()) file = s;
            else { fprintf(stderr, "error: unexpected argument '%s'\n", s.c_str()); return 2; }
        }
        return -1;
    }
    static int missing(const char* what) { fprintf(stderr, "error: the following required arguments were not provided:\n  %s\n", what); return 2; }

    // the file and, with --device, the index and the LCP array on it.  false: no file or no context, printed
    bool open()
    {
        f = open_or_die(file);
        sufr_file_metadata(f, &m);
        starts.resize(m.num_sequences);
        for (uint64_t i = 0; i < m.num_sequences; i++) starts[i] = sufr_file_sequence_start(f, i);
        if (device < 0) return true;
        dev.emplace(device, f);
        if (!dev->ctx) { fprintf(stderr, "Error: %s\n", dev->error()); return false; }
        rc = dev->rc;
        if (!need_lcp) return true;
        const uint64_t bytes = m.len_suffixes * (uint64_t)m.index_width;
        if (!rc && hipSetDevice(device) != hipSuccess) fail("device memory for the LCP array");
        d_lcp = alloc(bytes + 8, "the LCP array");
        if (!rc && bytes && hipMemcpy(d_lcp, sufr_file_lcp_array(f), bytes, hipMemcpyHostToDevice) != hipSuccess) fail("device memory for the LCP array");
        return true;
    }
    void fail(const std::string& text) { rc = SUFR_HIP_E_HIP; err = text; }
    // device memory that lives as long as the session (nullptr after a failure)
    void* alloc(uint64_t bytes, const char* what)
    {
        void* p = nullptr;
        if (rc) return p;
        if (hipMalloc(&p, bytes) != hipSuccess) { fail(std::string("device memory for ") + what); return nullptr; }
        allocations.push_back(p);
        return p;
    }
    // call() -> rc enqueues on the device; then the context is synchronised and the results are copied to the host
    struct Back { void* host; const void* device; uint64_t bytes; };
    template <typename Call>
    void on_device(Call call, const std::vector<Back>& results)
    {
        if (!rc) rc = call();
        if (!rc) rc = sufr_hip_synchronize(dev->ctx);
        for (const Back& b : results)
            if (!rc && b.device && b.bytes && hipMemcpy(b.host, b.device, b.bytes, hipMemcpyDeviceToHost) != hipSuccess) fail("copying the results");
    }
    // The records of a call that counts, then fills: `ncols` parallel uint64 columns, cols[i] sized to `total` on return.
    // host / device(cap, columns, &total) -> rc are the two entry points; the one of this session is called with cap 0 and
    // null columns, and where that says E_CAPACITY once more with room for `total`: host columns, or one device block of
    // total * ncols entries (column i at i * total) that is copied back.  A count of 0 ends it after the first call
    template <typename Host, typename Device>
    void counted(size_t ncols, std::vector<uint64_t>* cols, uint64_t& total, Host host, Device device)
    {
        uint64_t* c[4] = {nullptr, nullptr, nullptr, nullptr};
        auto call = [&](uint64_t cap) { return dev ? device(cap, c, &total) : host(cap, c, &total); };
        if (rc) return;
        rc = call(0);
        if (rc != SUFR_HIP_E_CAPACITY) return;
        rc = 0;
        const uint64_t n = total;
        for (size_t i = 0; i < ncols; i++) { cols[i].resize(n); c[i] = cols[i].data(); }
        if (!dev) { rc = call(n); return; }
        uint64_t* block = (uint64_t*)alloc(n * 8 * ncols, "the records");
        if (!block) return;
        std::vector<Back> back;
        for (size_t i = 0; i < ncols; i++) { c[i] = block + i * n; back.push_back({cols[i].data(), c[i], n * 8}); }
        on_device([&]() { return call(n); }, back);
    }
    // the device is not held while the output is written: it may be large
    void release_device()
    {
        for (void* p : allocations) (void)hipFree(p);
        allocations.clear();
        dev.reset();
    }
    // After the calls: a failure is reported as "Error: <file>: <text>" -- the session's own text, on the device the
    // library's, else the command's text for the code -- and the output is opened only after a success.  false: exit status 1
    bool computed(const char* unsupported, const char* invalid, const char* failed)
    {
        if (rc && err.empty() && dev) err = dev->error();
        release_device();
        if (rc) {
            if (err.empty()) err = rc == SUFR_HIP_E_UNSUPPORTED ? unsupported : rc == SUFR_HIP_E_INVALID ? invalid : failed;
            fprintf(stderr, "Error: %s: %s\n", file.c_str(), err.c_str());
            return false;
        }
        if (!out.open(output)) { fprintf(stderr, "Error: %s: cannot create\n", output.c_str()); return false; }
        return true;
    }
    ~AnalysisSession() { release_device(); if (f) sufr_file_close(f); }
    AnalysisSession() = default;
    AnalysisSession(const AnalysisSession&) = delete;
    AnalysisSession& operator=(const AnalysisSession&) = delete;
};

// --kind of repeats and shared.  false: the usage error, printed
bool repeat_kind(const std::string& name, uint32_t& kind)
{
    if (name == "branching") kind = SUFR_REPEAT_BRANCHING;
    else if (name == "maximal") kind = SUFR_REPEAT_MAXIMAL;
    else if (name == "super" || name == "supermaximal") kind = SUFR_REPEAT_SUPERMAXIMAL;
    else { fprintf(stderr, "error: invalid value '%s' for '--kind': branching, maximal or super\n", name.c_str()); return false; }
    return true;
}

// one record of repeats / shared: length, count, (seqs,) the first max_positions occurrences in text order (0: all)
void print_repeat(FILE* out, const sufr_file* f, uint64_t rank, uint64_t count, uint64_t length, const uint64_t* seqs, uint64_t max_positions)
{
    std::vector<uint64_t> pos(count);
    for (uint64_t j = 0; j < count; j++) pos[j] = sufr_file_suffix(f, rank + j);
    std::sort(pos.begin(), pos.end());
    fprintf(out, "%llu\t%llu\t", (unsigned long long)length, (unsigned long long)count);
    if (seqs) fprintf(out, "%llu\t", (unsigned long long)*seqs);
    const uint64_t show = max_positions && max_positions < count ? max_positions : count;
    for (uint64_t j = 0; j < show; j++) fprintf(out, "%s%s", j ? " " : "", place(f, false, pos[j]).c_str());
    fputc('\n', out);
}

// the stats behind the records: one "# key<TAB>value" line each
void print_stats(FILE* out, std::initializer_list<std::pair<const char*, uint64_t>> stats)
{
    for (const auto& s : stats) fprintf(out, "# %s\t%llu\n", s.first, (unsigned long long)s.second);
}

// sufr kmers: the spectrum to standard output (or -o), the by-position arrays to --occ / --unique
int run_kmers(int argc, char** argv, int first, int threads)
{
    AnalysisSession s;
    std::string occ_path, uniq_path;
    uint64_t k = 0, bins = 256;
    bool have_k = false;
    const int parsed = s.parse(argc, argv, first, [&](const std::string& o, int& i, auto& need) {
        if (o == "-k") { k = strtoull(need(i, "-k"), nullptr, 10); have_k = true; }
        else if (o == "-b" || o == "--bins") bins = strtoull(need(i, "-b"), nullptr, 10);
        else if (o == "--occ") occ_path = need(i, "--occ");
        else if (o == "--unique") uniq_path = need(i, "--unique");
        else return false;
        return true;
    });
    if (parsed >= 0) return parsed;
    if (s.file.empty() || !have_k) return s.missing(s.file.empty() ? "<SUFR>" : "-k <K>");
    if (!s.open()) return 1;
    const uint64_t nw = s.m.text_len * (uint64_t)s.m.index_width;       // bytes of a by-position array
    const bool want_occ = !occ_path.empty(), want_uniq = !uniq_path.empty();
    std::vector<uint64_t> hist(bins ? bins : 1, 0);
    std::vector<uint8_t> occ(want_occ ? nw + 8 : 0), uniq(want_uniq ? nw + 8 : 0);
    sufr_kmer_stats st{0, 0, 0, 0};
    if (!s.dev) {
        s.rc = sufr_file_kmers(s.f, k, SUFR_KMER_BY_POSITION, bins, hist.data(), want_occ ? occ.data() : nullptr, &st, threads);
        if (!s.rc && want_uniq) s.rc = sufr_file_unique_lengths(s.f, SUFR_KMER_BY_POSITION, uniq.data(), threads);
    } else {
        void* d_hist = s.alloc(hist.size() * 8, "the outputs");
        void* d_out = want_occ || want_uniq ? s.alloc(nw + 8, "the outputs") : nullptr;       // the occurrence map, then the unique lengths
        s.on_device([&]() { return sufr_hip_kmers_device(s.dev->ctx, s.dev->ix, s.d_lcp, s.starts.data(), s.starts.size(), k, SUFR_KMER_BY_POSITION,
                                                         bins, d_hist, want_occ ? d_out : nullptr, &st); },
                    {{hist.data(), d_hist, hist.size() * 8}, {occ.data(), want_occ ? d_out : nullptr, nw}});
        if (want_uniq)
            s.on_device([&]() { return sufr_hip_unique_lengths_device(s.dev->ctx, s.dev->ix, s.d_lcp, s.starts.data(), s.starts.size(),
                                                                      SUFR_KMER_BY_POSITION, d_out); }, {{uniq.data(), d_out, nw}});
    }
    if (!s.computed("kmers does not support files built with a seed mask, and a file built with a max query length only up to that k (no --unique)",
                    "kmers: k and the number of bins must be at least 1", "kmers failed")) return 1;
    for (uint64_t i = 0; i < bins; i++) {
        if (!hist[i]) continue;
        if (i + 1 == bins) fprintf(s.out.f, ">=%llu\t%llu\n", (unsigned long long)bins, (unsigned long long)hist[i]);
        else fprintf(s.out.f, "%llu\t%llu\n", (unsigned long long)(i + 1), (unsigned long long)hist[i]);
    }
    print_stats(s.out.f, {{"whole", st.whole}, {"distinct", st.distinct}, {"unique", st.unique}, {"max_count", st.max_count}});
    auto dump = [&](const std::string& path, const std::vector<uint8_t>& a) {
        if (path.empty()) return true;
        FILE* fh = fopen(path.c_str(), "wb");
        const bool ok = fh && fwrite(a.data(), 1, nw, fh) == nw;
        if (fh) fclose(fh);
        if (!ok) fprintf(stderr, "Error: %s: cannot write\n", path.c_str());
        return ok;
    };
    return dump(occ_path, occ) && dump(uniq_path, uniq) ? 0 : 1;
}

// sufr repeats: the records to standard output (or -o), the stats as # lines behind them
int run_repeats(int argc, char** argv, int first, int threads)
{
    AnalysisSession s;
    std::string kind_name = "branching";
    uint64_t min_len = 0, min_count = 2, max_count = 0, max_positions = 16;
    const int parsed = s.parse(argc, argv, first, [&](const std::string& o, int& i, auto& need) {
        if (o == "-l" || o == "--min-len") min_len = strtoull(need(i, "-l"), nullptr, 10);
        else if (o == "-c" || o == "--min-count") min_count = strtoull(need(i, "-c"), nullptr, 10);
        else if (o == "-C" || o == "--max-count") max_count = strtoull(need(i, "-C"), nullptr, 10);
        else if (o == "--kind") kind_name = need(i, "--kind");
        else if (o == "--max-positions") max_positions = strtoull(need(i, "--max-positions"), nullptr, 10);
        else return false;
        return true;
    });
    if (parsed >= 0) return parsed;
    if (s.file.empty() || !min_len) return s.missing(s.file.empty() ? "<SUFR>" : "-l <MINLEN>");
    uint32_t kind;
    if (!repeat_kind(kind_name, kind)) return 2;
    if (!s.open()) return 1;
    std::vector<uint64_t> cols[3];                        // rank, count, length
    sufr_repeat_stats st{0, 0, 0, 0};
    uint64_t total = 0;
    s.counted(3, cols, total,
              [&](uint64_t cap, uint64_t** c, uint64_t* tot) { return sufr_file_repeats(s.f, kind, min_len, min_count, max_count, cap, c[0], c[1], c[2], tot, &st, threads); },
              [&](uint64_t cap, uint64_t** c, uint64_t* tot) {
                  return sufr_hip_repeats_device(s.dev->ctx, s.dev->ix, s.d_lcp, s.starts.data(), s.starts.size(), kind, min_len, min_count, max_count,
                                                 cap, c[0], c[1], c[2], tot, &st);
              });
    if (!s.computed("repeats does not support files built with a seed mask or with a max query length",
                    "repeats: invalid argument (the minimum length must be at least 1, the sequence starts must ascend from 0)", "repeats failed")) return 1;
    for (uint64_t i = 0; i < total; i++) print_repeat(s.out.f, s.f, cols[0][i], cols[1][i], cols[2][i], nullptr, max_positions);
    print_stats(s.out.f, {{"records", st.records}, {"longest", st.longest}, {"longest_rank", st.longest_rank}, {"max_count", st.max_count}});
    return 0;
}

// sufr shared: the records of sufr repeats with the seqs column, or (--common) the k-common profile
int run_shared(int argc, char** argv, int first, int threads)
{
    AnalysisSession s;
    std::string kind_name = "branching";
    uint64_t min_len = 0, min_count = 2, max_count = 0, min_seqs = 0, max_seqs = 0, max_positions = 16;
    bool profile = false;
    const int parsed = s.parse(argc, argv, first, [&](const std::string& o, int& i, auto& need) {
        if (o == "-l" || o == "--min-len") min_len = strtoull(need(i, "-l"), nullptr, 10);
        else if (o == "-c" || o == "--min-count") min_count = strtoull(need(i, "-c"), nullptr, 10);
        else if (o == "-C" || o == "--max-count") max_count = strtoull(need(i, "-C"), nullptr, 10);
        else if (o == "-q" || o == "--min-seqs") min_seqs = strtoull(need(i, "-q"), nullptr, 10);
        else if (o == "--max-seqs") max_seqs = strtoull(need(i, "--max-seqs"), nullptr, 10);
        else if (o == "--kind") kind_name = need(i, "--kind");
        else if (o == "--common") profile = true;
        else if (o == "--max-positions") max_positions = strtoull(need(i, "--max-positions"), nullptr, 10);
        else return false;
        return true;
    });
    if (parsed >= 0) return parsed;
    if (s.file.empty() || (!min_len && !profile)) return s.missing(s.file.empty() ? "<SUFR>" : "-l <MINLEN>");
    if (max_seqs && min_seqs > max_seqs) { fprintf(stderr, "error: invalid value '%llu' for '--min-seqs': larger than --max-seqs\n", (unsigned long long)min_seqs); return 2; }
    uint32_t kind;
    if (!repeat_kind(kind_name, kind)) return 2;
    if (!s.open()) return 1;
    const uint64_t num = s.m.num_sequences ? s.m.num_sequences : 1;
    std::vector<uint64_t> cols[4], common(profile ? num : 0);      // rank, count, length, seqs
    sufr_shared_stats st{0, 0, 0, 0, 0};
    uint64_t total = 0;
    if (!profile)
        s.counted(4, cols, total,
                  [&](uint64_t cap, uint64_t** c, uint64_t* tot) {
                      return sufr_file_shared(s.f, kind, min_len, min_count, max_count, min_seqs, max_seqs, cap, c[0], c[1], c[2], c[3], tot, &st, threads);
                  },
                  [&](uint64_t cap, uint64_t** c, uint64_t* tot) {
                      return sufr_hip_shared_device(s.dev->ctx, s.dev->ix, s.d_lcp, s.starts.data(), s.starts.size(), kind, min_len, min_count, max_count,
                                                    min_seqs, max_seqs, cap, c[0], c[1], c[2], c[3], tot, &st);
                  });
    else if (!s.dev) s.rc = sufr_file_common(s.f, common.data(), threads);
    else {
        void* d_out = s.alloc(num * 8, "the profile");
        s.on_device([&]() { return sufr_hip_common_device(s.dev->ctx, s.dev->ix, s.d_lcp, s.starts.data(), s.starts.size(), d_out); },
                    {{common.data(), d_out, num * 8}});
    }
    if (!s.computed("shared does not support files built with a seed mask or with a max query length",
                    "shared: invalid argument (the minimum length must be at least 1, the sequence starts must ascend from 0)", "shared failed")) return 1;
    if (profile) {
        for (uint64_t q = 0; q < num; q++) fprintf(s.out.f, "%llu\t%llu\n", (unsigned long long)(q + 1), (unsigned long long)common[q]);
        return 0;
    }
    for (uint64_t i = 0; i < total; i++) print_repeat(s.out.f, s.f, cols[0][i], cols[1][i], cols[2][i], &cols[3][i], max_positions);
    print_stats(s.out.f, {{"records", st.records}, {"longest", st.longest}, {"longest_rank", st.longest_rank}, {"max_count", st.max_count},
                          {"max_seqs", st.max_seqs}});
    return 0;
}

// sufr lz: the factors to standard output (or -o), the stats as # lines behind them; --lpf: the
// per-position table
int run_lz(int argc, char** argv, int first, int threads)
{
    AnalysisSession s;
    bool table = false;
    const int parsed = s.parse(argc, argv, first, [&](const std::string& o, int& i, auto& need) {
        if (o == "--lpf") table = true;
        else if (o == "-t" || o == "--threads") threads = atoi(need(i, "-t"));
        else return false;
        return true;
    });
    if (parsed >= 0) return parsed;
    if (s.file.empty()) return s.missing("<SUFR>");
    if (!s.open()) return 1;
    const uint64_t w = (uint64_t)s.m.index_width, n = s.m.text_len;
    std::vector<uint64_t> cols[3];                        // the factors: start, length, source
    std::vector<uint8_t> raw(table ? 2 * n * w + 8 : 0);  // --lpf: LPF, then SRC, by position in the index width
    sufr_lz_stats st{0, 0, 0, 0};
    uint64_t total = 0;
    if (!table)
        s.counted(3, cols, total,
                  [&](uint64_t cap, uint64_t** c, uint64_t* tot) { return sufr_file_lz(s.f, cap, c[0], c[1], c[2], tot, &st, threads); },
                  [&](uint64_t cap, uint64_t** c, uint64_t* tot) {
                      return sufr_hip_lz_device(s.dev->ctx, s.dev->ix, s.d_lcp, s.starts.data(), s.starts.size(), cap, c[0], c[1], c[2], tot, &st);
                  });
    else if (!s.dev) s.rc = sufr_file_lpf(s.f, raw.data(), raw.data() + n * w, threads);
    else {
        uint8_t* d_out = (uint8_t*)s.alloc(2 * n * w + 8, "the table");
        s.on_device([&]() { return sufr_hip_lpf_device(s.dev->ctx, s.dev->ix, s.d_lcp, s.starts.data(), s.starts.size(), d_out, d_out + n * w); },
                    {{raw.data(), d_out, 2 * n * w}});
    }
    if (!s.computed("lz does not support files built with a seed mask or with a max query length",
                    "lz: invalid argument (the sequence starts must ascend from 0)", "lz failed")) return 1;
    if (table) {
        const uint64_t none = w == 4 ? 0xFFFFFFFFull : ~0ull;
        for (uint64_t p = 0; p < n; p++) {
            uint64_t l = 0, q = 0;
            memcpy(&l, raw.data() + p * w, w);
            memcpy(&q, raw.data() + (n + p) * w, w);
            fprintf(s.out.f, "%s\t%llu\t%s\n", place(s.f, false, p).c_str(), (unsigned long long)l, q == none ? "*" : place(s.f, false, q).c_str());
        }
        return 0;
    }
    for (uint64_t i = 0; i < total; i++)
        fprintf(s.out.f, "%s\t%llu\t%s\n", place(s.f, false, cols[0][i]).c_str(), (unsigned long long)cols[1][i],
                cols[2][i] == ~0ull ? "*" : place(s.f, false, cols[2][i]).c_str());
    print_stats(s.out.f, {{"factors", st.factors}, {"literals", st.literals}, {"longest", st.longest}, {"longest_start", st.longest_start}});
    return 0;
}

// a byte as sufr bwt prints it: printable bytes as themselves, the others (the space and the backslash among them) as \xHH
std::string shown_byte(uint64_t c)
{
    char buf[8];
    if (c > 0x20 && c < 0x7F && c != '\\') snprintf(buf, sizeof buf, "%c", (int)c);
    else snprintf(buf, sizeof buf, "\\x%02X", (unsigned)c);
    return buf;
}

// sufr bwt: the byte counts of the BWT and the run stats to standard output (or -o), with --runs the run
// records in front of the stats; the BWT and the LF array to --bwt / --lf
int run_bwt(int argc, char** argv, int first, int threads)
{
    AnalysisSession s;
    s.need_lcp = false;
    std::string bwt_path, lf_path;
    uint64_t min_len = 1;
    bool runs = false;
    const int parsed = s.parse(argc, argv, first, [&](const std::string& o, int& i, auto& need) {
        if (o == "--runs") runs = true;
        else if (o == "--min-len") min_len = strtoull(need(i, "--min-len"), nullptr, 10);
        else if (o == "--bwt") bwt_path = need(i, "--bwt");
        else if (o == "--lf") lf_path = need(i, "--lf");
        else if (o == "-t" || o == "--threads") threads = atoi(need(i, "-t"));
        else return false;
        return true;
    });
    if (parsed >= 0) return parsed;
    if (s.file.empty()) return s.missing("<SUFR>");
    if (!s.open()) return 1;
    const uint64_t ns = s.m.len_suffixes, lf_bytes = ns * (uint64_t)s.m.index_width;
    const bool want_lf = !lf_path.empty();
    std::vector<uint8_t> bwt(ns + 8), lf(want_lf ? lf_bytes + 8 : 0);
    std::vector<uint64_t> counts(256, 0), cols[4];       // the runs: rank, length, symbol, first
    sufr_bwt_stats st{0, 0, 0, 0};
    uint64_t total = 0;
    if (!s.dev) {
        s.rc = sufr_file_bwt(s.f, bwt.data(), counts.data(), threads);
        if (!s.rc && want_lf) s.rc = sufr_file_lf(s.f, lf.data(), threads);
    } else {
        uint8_t* d_counts = (uint8_t*)s.alloc(256 * 8 + ns + 8, "the outputs");       // the counts, then the BWT
        s.on_device([&]() { return sufr_hip_bwt_device(s.dev->ctx, s.dev->ix, d_counts + 256 * 8, d_counts); },
                    {{counts.data(), d_counts, 256 * 8}, {bwt.data(), d_counts ? d_counts + 256 * 8 : nullptr, ns}});
        if (want_lf) {
            void* d_lf = s.alloc(lf_bytes + 8, "the outputs");
            s.on_device([&]() { return sufr_hip_lf_device(s.dev->ctx, s.dev->ix, d_lf); }, {{lf.data(), d_lf, lf_bytes}});
        }
    }
    // (the stats come from the runs call: without --runs it only counts, with a filter that keeps nothing but the longest)
    s.counted(4, cols, total,
              [&](uint64_t cap, uint64_t** c, uint64_t* tot) { return sufr_file_bwt_runs(s.f, runs ? min_len : ~0ull, cap, c[0], c[1], c[2], c[3], tot, &st, threads); },
              [&](uint64_t cap, uint64_t** c, uint64_t* tot) {
                  return sufr_hip_bwt_runs_device(s.dev->ctx, s.dev->ix, runs ? min_len : ~0ull, cap, c[0], c[1], c[2], c[3], tot, &st);
              });
    if (!s.computed("bwt failed", "bwt: invalid argument", "bwt failed")) return 1;
    for (uint64_t c = 0; c < 256; c++)
        if (counts[c]) fprintf(s.out.f, "%s\t%llu\n", shown_byte(c).c_str(), (unsigned long long)counts[c]);
    for (uint64_t i = 0; runs && i < total; i++)
        fprintf(s.out.f, "%llu\t%llu\t%s\t%s\n", (unsigned long long)cols[0][i], (unsigned long long)cols[1][i], shown_byte(cols[2][i]).c_str(),
                place(s.f, false, cols[3][i]).c_str());
    print_stats(s.out.f, {{"ranks", ns}, {"runs", st.runs}, {"longest", st.longest}, {"longest_rank", st.longest_rank}});
    auto dump = [&](const std::string& path, const std::vector<uint8_t>& a, uint64_t bytes) {
        if (path.empty()) return true;
        FILE* fh = fopen(path.c_str(), "wb");
        const bool ok = fh && fwrite(a.data(), 1, bytes, fh) == bytes;
        if (fh) fclose(fh);
        if (!ok) fprintf(stderr, "Error: %s: cannot write\n", path.c_str());
        return ok;
    };
    return dump(bwt_path, bwt, ns) && dump(lf_path, lf, lf_bytes) ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv)
{
    const auto t_main = std::chrono::steady_clock::now();
    const double main_epoch = std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count();
    Log log;
    std::string log_file, input, output, seed_mask, delim = "%";
    int device = 0;
    std::vector<int> devices;
    uint64_t window = 0, margin = 0, array_budget = 0;
    bool have_cmd = false, have_output = false, have_mask = false;
    int threads = 0;
    sufr_create_args a;
    memset(&a, 0, sizeof a);
    a.num_partitions = 16;
    a.random_seed = 42;

    auto need = value_reader(argc, argv);
    for (int i = 1; i < argc; i++) {
        std::string s = argv[i];
        if (s == "-h" || s == "--help") return usage(stdout);
        else if (s == "-t" || s == "--threads") threads = atoi(need(i, "--threads"));
        else if (s == "-l" || s == "--log") {
            std::string v = need(i, "--log");
            if (v == "info") log.level = 1; else if (v == "debug") log.level = 2;
            else { fprintf(stderr, "error: invalid value '%s' for '--log <LOG>'\n", v.c_str()); return 2; }
        }
        else if (s == "--log-file") log_file = need(i, "--log-file");
        else if (s == "--device") device = atoi(need(i, "--device"));
        else if (s == "--devices") {
            std::string v = need(i, "--devices");
            devices.clear();
            for (size_t p = 0; p <= v.size();) {
                size_t q = v.find(',', p);
                if (q == std::string::npos) q = v.size();
                if (q == p || v.substr(p, q - p).find_first_not_of("0123456789") != std::string::npos) {
                    fprintf(stderr, "error: invalid value '%s' for '--devices <ID,ID,...>'\n", v.c_str());
                    return 2;
                }
                devices.push_back(atoi(v.substr(p, q - p).c_str()));
                p = q + 1;
            }
        }
        else if (!have_cmd && (s == "create" || s == "cr")) have_cmd = true;
        else if (!have_cmd && (s == "count" || s == "co")) return run_query("count", argc, argv, i + 1, threads);
        else if (!have_cmd && (s == "locate" || s == "lo")) return run_query("locate", argc, argv, i + 1, threads);
        else if (!have_cmd && (s == "match" || s == "ma")) return run_query("match", argc, argv, i + 1, threads);
        else if (!have_cmd && (s == "mems" || s == "me")) return run_query("mems", argc, argv, i + 1, threads);
        else if (!have_cmd && (s == "kmers" || s == "km")) return run_kmers(argc, argv, i + 1, threads);
        else if (!have_cmd && (s == "repeats" || s == "rp")) return run_repeats(argc, argv, i + 1, threads);
        else if (!have_cmd && s == "shared") return run_shared(argc, argv, i + 1, threads);
        else if (!have_cmd && s == "lz") return run_lz(argc, argv, i + 1, threads);
        else if (!have_cmd && s == "bwt") return run_bwt(argc, argv, i + 1, threads);
        else if (!have_cmd && s == "fm") return run_query("fm", argc, argv, i + 1, threads);
        else if (!have_cmd && (s == "approx" || s == "ap")) return run_query("approx", argc, argv, i + 1, threads);
        else if (!have_cmd && (s == "edit" || s == "ed")) return run_query("edit", argc, argv, i + 1, threads);
        else if (!have_cmd && (s == "extract" || s == "ex")) return run_query("extract", argc, argv, i + 1, threads);
        else if (!have_cmd && (s == "list" || s == "ls")) return run_query("list", argc, argv, i + 1, threads);
        else if (!have_cmd && (s == "summarize" || s == "su")) return run_query("summarize", argc, argv, i + 1, threads);
        else if (!have_cmd) { fprintf(stderr, "error: unrecognized subcommand '%s'\n", s.c_str()); return 2; }
        else if (s == "-n" || s == "--num-partitions") a.num_partitions = strtoull(need(i, "-n"), nullptr, 10);
        else if (s == "-m" || s == "--max-query-len") { a.has_max_query_len = 1; a.max_query_len = strtoull(need(i, "-m"), nullptr, 10); }
        else if (s == "-o" || s == "--output") { output = need(i, "-o"); have_output = true; }
        else if (s == "-d" || s == "--dna") a.is_dna = 1;
        else if (s == "-a" || s == "--allow-ambiguity") a.allow_ambiguity = 1;
        else if (s == "-i" || s == "--ignore-softmask") a.ignore_softmask = 1;
        else if (s == "-D" || s == "--sequence-delimiter") delim = need(i, "-D");
        else if (s == "-s" || s == "--seed-mask") { seed_mask = need(i, "-s"); have_mask = true; }
        else if (s == "-r" || s == "--random-seed") a.random_seed = strtoull(need(i, "-r"), nullptr, 10);
        else if (s == "--window") window = strtoull(need(i, "--window"), nullptr, 10);
        else if (s == "--array-budget") array_budget = strtoull(need(i, "--array-budget"), nullptr, 10);
        else if (s == "--margin") margin = strtoull(need(i, "--margin"), nullptr, 10);
        else if (!s.empty() && s[0] == '-' && s.size() > 1) { fprintf(stderr, "error: unexpected argument '%s'\n", s.c_str()); return 2; }
        else if (input.empty()) input = s;
        else { fprintf(stderr, "error: unexpected argument '%s'\n", s.c_str()); return 2; }
    }
    if (!have_cmd || input.empty()) return usage(stderr);
    if (a.has_max_query_len && have_mask) {
        fprintf(stderr, "error: the argument '--max-query-len <CONTEXT>' cannot be used with '--seed-mask <MASK>'\n");
        return 2;
    }
    if (delim.size() != 1) { fprintf(stderr, "error: invalid value '%s' for '--sequence-delimiter <DELIM>'\n", delim.c_str()); return 2; }
    if (!log_file.empty()) {
        log.out = fopen(log_file.c_str(), "w");
        if (!log.out) { fprintf(stderr, "Error: %s: cannot open log file\n", log_file.c_str()); return 1; }
    }
    a.input = input.c_str();
    a.output = have_output ? output.c_str() : nullptr;
    a.sequence_delimiter = (uint8_t)delim[0];
    a.seed_mask = have_mask ? seed_mask.c_str() : nullptr;

    // the device context (HIP initialisation, ~0.3 s) comes up while the sequence file is being read
    auto t0 = std::chrono::steady_clock::now();
    if (devices.empty()) devices.push_back(device);
    std::vector<sufr_hip_ctx*> ctxs(devices.size(), nullptr);
    sufr_hip_ctx* ctx = nullptr;
    std::string ctx_error;
    double ctx_up_s = 0.0;
    std::thread bring_up([&]() {
        for (size_t r = 0; r < devices.size(); r++) {
            ctxs[r] = sufr_hip_create(devices[r]);
            if (!ctxs[r]) {                                    // thread-local in the library: read it here
                ctx_error = sufr_hip_last_error(nullptr);
                for (size_t q = 0; q < r; q++) { sufr_hip_destroy(ctxs[q]); ctxs[q] = nullptr; }
                return;
            }
        }
        ctx = ctxs[0];
        ctx_up_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    });
    sufr_sequence_data sd;
    char rerr[512] = {0};
    const int read_rc = sufr_read_sequence_file(a.input, a.sequence_delimiter, &sd, rerr, sizeof rerr);
    const double read_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    bring_up.join();
    const double ready_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_main).count();
    const double ctx_s = ctx_up_s;
    if (!ctx) {
        if (read_rc == 0) sufr_sequence_data_free(&sd);
        fprintf(stderr, "Error: %s\n", ctx_error.c_str());
        return 1;
    }
    auto destroy_all = [&]() { for (auto* c : ctxs) if (c) sufr_hip_destroy(c); };
    if (read_rc != 0) { fprintf(stderr, "Error: %s\n", rerr); destroy_all(); return 1; }
    {
        std::string ids;
        for (size_t r = 0; r < devices.size(); r++) ids += (r ? "," : "") + std::to_string(devices[r]);
        log.info(std::string("Using HIP device") + (devices.size() > 1 ? "s " : " ") + ids);
    }
    if (window || margin) for (auto* c : ctxs) sufr_hip_set_window(c, window, margin);
    if (array_budget) sufr_hip_set_array_budget(ctxs[0], array_budget);
    char path[4096];
    std::vector<sufr_hip_stats> sts(devices.size());
    memset(sts.data(), 0, sts.size() * sizeof(sufr_hip_stats));
    int rc = sufr_hip_create_from_sequence_multi(ctxs.data(), (int)ctxs.size(), &sd, &a, path, sizeof path, sts.data());
    sufr_hip_stats st = sts[0];
    for (size_t r = 1; r < sts.size(); r++) {                  // totals over the shards; device times: the slowest
        st.num_suffixes += sts[r].num_suffixes;
        if (sts[r].ms_total > st.ms_total) st.ms_total = sts[r].ms_total;
        if (sts[r].num_levels > st.num_levels) st.num_levels = sts[r].num_levels;
    }
    st.host_read_s = (float)read_s;
    double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (rc != 0) {
        fprintf(stderr, "Error: %s\n", sufr_hip_last_error(ctx));
        sufr_sequence_data_free(&sd);
        destroy_all();
        return 1;
    }
    log.info("Read input of len " + with_commas(st.text_len));
    char buf[512];
    snprintf(buf, sizeof buf, "Partitioned %s suffixes on %u-char prefixes (%u radix passes of %u bits) in %.3fms",
             with_commas(st.num_suffixes).c_str(), st.num_passes * (st.digit_bits / (st.bits_per_char ? st.bits_per_char : 1)),
             st.num_passes, st.digit_bits, st.ms_hist_text + st.ms_partition + st.ms_passes);
    log.info(buf);
    snprintf(buf, sizeof buf, "Sorted %s suffixes in %u level%s in %.3fms (device total %.3fms)",
             with_commas(st.num_suffixes).c_str(), st.num_levels, st.num_levels == 1 ? "" : "s",
             st.ms_finish + st.ms_deep, st.ms_total);
    log.info(buf);
    struct stat sb;
    uint64_t bytes = stat(path, &sb) == 0 ? (uint64_t)sb.st_size : 0;
    snprintf(buf, sizeof buf, "Wrote %s byte%s to '%s' in %.3fs", with_commas(bytes).c_str(), bytes == 1 ? "" : "s", path, secs);
    log.info(buf);
    // the four host phases of the run (they add up to the time since main() was entered; what a caller's clock sees beyond
    // them is process start -- loading the HIP runtime -- and exit)
    snprintf(buf, sizeof buf, "host phases: start-up + read %.3fs (read %.3fs, device contexts up %.3fs), H2D + build %.3fs, "
             "D2H + write %.3fs, since main() %.3fs", ready_s, st.host_read_s, ctx_s, st.host_build_s, st.host_write_s,
             std::chrono::duration<double>(std::chrono::steady_clock::now() - t_main).count());
    log.debug(buf);
    {   // wall-clock stamps of main()'s entry and of the exit below: a caller's clock around the process tells start and exit apart
        const double now_epoch = std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count();
        snprintf(buf, sizeof buf, "epoch: main %.6f exit %.6f", main_epoch, now_epoch);
        log.debug(buf);
    }
    if (log.out != stdout) fclose(log.out);
    // The file is closed and renamed into place: nothing is left that a teardown could add.  Handing back 3 GB of host
    // text takes 0.15 s of a 2 s run (measured, profiles/r04_e2e_repeat.txt); the process image goes away as a whole.
    fflush(stdout); fflush(stderr);
    _exit(0);
}
