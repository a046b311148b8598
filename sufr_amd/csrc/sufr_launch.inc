// sufr_launch.inc -- host side of the build pipeline (included by sufr_kernels.hip).
//
// One Pipeline per context / GPU.  Replaces SufrBuilder::sort() (sufr_builder.rs:495-598):
//   pivots + partition()  ->  byte histogram -> dense character codes -> packed K-char keys,
//                             MSD partition levels on dense D-character digits (the first streams the text)
//   per-partition merge_sort -> leaf sort of the buckets, tie level + re-keying levels for long repeats,
//                             prefix doubling for levels that stop shrinking
// No temp files, no mutexes; every intermediate lives in HBM.

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <functional>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/sufr_hip.h"

namespace sufr {

#define HIP_TRY(call)                                                                        \
    do {                                                                                     \
        hipError_t e__ = (call);                                                             \
        if (e__ != hipSuccess) {                                                             \
            set_error(std::string(#call) + ": " + hipGetErrorString(e__));                   \
            return SUFR_HIP_E_HIP;                                                           \
        }                                                                                    \
    } while (0)

static constexpr uint64_t SUFR_MAX_TEXT_LEN = 0xFFFFFFFFull - (1ull << 24);   // largest text the device path takes

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

struct LevelArrays {
    DevBuf keyA, keyB, idxA, idxB, segA, segB, opos;
};

class Pipeline;
// sufr_exc.inc: the suffixes whose comparisons reached a byte outside the fixed DNA table, re-placed after the build
// The shard of a build: first digits (D characters of the fixed 3-bit codes) in [raw_lo, raw_hi); raw_hi = 8^D: no upper bound.
// cap: the symbols a capped build compares (--max-query-len L built directly), 0: the plain suffix order.
struct ExcShard { int sharded; uint32_t raw_lo, raw_hi; int D; int allow_amb; uint32_t cap; };
int exc_reinsert(Pipeline& pl, uint8_t* d_text, uint64_t n, const uint32_t* bsa, const uint32_t* blcp, uint32_t s,
                 const uint32_t* d_exc, uint32_t E, uint32_t* out_sa, uint32_t* out_lcp, uint64_t out_cap, uint64_t* affected_out,
                 const ExcShard& shard, uint64_t* s_out);
static constexpr uint32_t EXC_MAX_LIST = 1u << 20;     // bytes outside {$ % A C G N T} a DNA build lists (more: the general code table)

class Pipeline {
public:
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    uint64_t resident_text_len = 0;            // text of the last complete one-window build in `text` (0: none, or windows since)
    // the order of the last build, for the boundary LCP of its shards (k_lcp_pair / k_lcp_stitch): seed mask or length cap
    uint32_t stitch_weight = 0;                // care symbols of the mask (their offsets in `stitchoffs`), 0: no mask
    uint64_t stitch_cap = 0;                   // max_query_len, 0: none
    DevBuf stitchoffs;
    StitchOrder stitch_order() const { StitchOrder so; so.offs = stitch_weight ? (const uint32_t*)stitchoffs.p : nullptr; so.weight = stitch_weight; so.cap = stitch_cap; return so; }
    bool debug = false;

    // workspace (grown on demand, reused between builds)
    DevBuf text, bytehist, lut, table, bintot, binbase, scalars;
    DevBuf keyA, keyB, idxA, idxB;       // (key, idx) arrays of the masked / max-query-len passes
    DevBuf recA, recB;                   // 12-byte records of the MSD levels, ping-pong
    DevBuf rankbuf, dposbuf, deferbuf, unresbuf, posbitsbuf, dblf[7], dblg[6];   // prefix doubling (sufr_dbl.inc)
    DevBuf headsA, headsB, sizes, starts, partials;
    DevBuf tilefirst, runends, tileany, nexttile, nextblk, depthA, depthB, period, remapbuf, flagsbuf, packedbuf, wmaskbuf, wcntbuf, recoff, runoff, wlflag, wlhead, wloff, candbuf, keepbuf, plancnt, fixbuf, pairsc, pairbuf;
    DevBuf rg_misc, rg_blk, rg_blkoff, rg_rs, rg_rl, rg_E, rg_L, rg_V, rg_tab[2], rg_off[2], rg_long[2], rg_tmax[2], rg_hist, rg_depth;   // run buckets (sufr_runs.inc)
    // MSD levels: digit maps, group / sub-bucket tables, segment lists, tile and window plans
    DevBuf cumbuf, dmapbuf, identbuf[16], grouptab, gcur, leafcnt, leafoff, leafbase, leafcur, bigflag, bigoff;
    DevBuf rawtab, presbuf, rawtot, valsbuf, startbuf;   // k_text_pass_dna: raw first-digit histogram per group, 5-mer presence bits
    DevBuf exc_pos, exc_byte, exc_sorted, exc_sa, exc_lcp, exc_bits, exc_blk, exc_off, exc_list, exc_list2, exc_pmin, exc_roff;   // bytes outside the DNA table (sufr_exc.inc)
    // The left-over buckets (members agree on all K key characters) and the tie runs are two independent chains of re-keying
    // levels: latency-bound kernels and host round trips, level after level.  Round 6 runs the first chain on a helper pipeline
    // of its own (own stream, level arrays, scalars, read-back buffer; a host thread drives it) while this one does the tie runs:
    // the two write disjoint ranks of SA / LCP.  --dna on the 3.1 Gb stand-in: 0.297 -> 0.26 s (profiles/r06_input_classes.txt).
    // That holds for the text-keyed levels only: prefix doubling keys a suffix by the RANK of another one, which may lie in a
    // left-over bucket, so the tie chain joins the helper (and places the run buckets) before it enters run_doubling.
    std::unique_ptr<Pipeline> helper;
    bool overlap_chains = true;    // probes: off = one chain after the other (rounds 1-5)
    static constexpr uint64_t OVERLAP_MIN_DEFAULT = (uint64_t)1 << 22;
    uint64_t opt_overlap_min = 0;  // left-over records from which their chain runs on the helper (sufr_hip_set_overlap_min; 0: the default, ~0: never)
    // The pair path in front of the tie level (tie_level): tie runs of exactly two members are walked directly instead of being
    // keyed.  Taken when the pairs hold at least PAIR_MIN_PERMILLE thousandths of the tie records.
    // (the value: profiles/pair_walk_ab.txt, "threshold" -- measured on one MI355X: at ~15 per mille, the 100 Mb C. elegans stand-in,
    // the path costs 0.014 ms of 1.17; at 96, the --dna build of the human stand-in, it saves 3.4 ms of 153.8; 50 lies between)
    static constexpr uint32_t PAIR_MIN_PERMILLE = 50;
    uint32_t opt_pair_walk = 0;    // sufr_hip_set_pair_walk: 0 the default (by the share of pairs), 1 always, 2 never
    uint64_t last_pairs_resolved = 0, last_pairs_left = 0;   // the last build: pairs the path finished / walked and handed back (windowed builds: all windows)
    uint32_t last_overlapped = 0;  // the last build ran the left-over chain on the helper (windowed builds: one of the windows did)
    uint64_t dbl_entries = 0;      // entries into run_doubling by this pipeline in the current build
    uint64_t last_doublings = 0;   // ... of the last build, both chains (windowed builds: all windows)
    std::function<int()> before_doubling;      // run_levels calls it right before run_doubling (the join of the helper chain)
    uint32_t exc_pending = 0;      // listed bytes that are still 'N' in `text` (put back by exc_reinsert, or on the way out of the build)
    bool mql_fast_ok = true;       // probes: off = a capped build is the exact build + apply_max_query_len (rounds 1-5)
    bool exc_disable = false;      // this build takes the general code table whatever the text holds (the retry of a build that listed too much)
    static constexpr uint64_t EXC_MAX_AFFECTED_DEFAULT = (uint64_t)1 << 22;     // affected suffixes the whole-text sort and its buffers take
    uint64_t opt_exc_max_affected = 0;         // ... from which a build goes to the general code table (sufr_hip_set_exc_max_affected; 0: the default)
    uint64_t exc_max_affected() const { return opt_exc_max_affected ? opt_exc_max_affected : EXC_MAX_AFFECTED_DEFAULT; }
    uint32_t last_exc_retry = 0;   // why the last build took that retry: 0 it did not, 1 / 2 / 3 the comparison of exc_reinsert that gave up (windowed builds: the largest)
    uint64_t last_exc_taken = 0;   // ranks the last exc_reinsert took out of the arrays (also when it then gave up)
    DevBuf exc_all_sa, exc_all_lcp;            // the whole arrays of a sharded build's retry (retry_whole_text)
    bool no_exceptions = false;    // probes: every byte outside the table sends the build to the general code table (round 5)
    std::vector<uint32_t> rawtot_host, valshost;
    uint16_t h_lut[256];                       // code table of the build (host copy: uploaded asynchronously)
    uint32_t h_seg0[2];                        // the one segment level 1 starts from
    DevBuf segst[2], segsz[2], tunits, upre, tdesc, wunits, wpre, wdesc, wslow;
    std::vector<uint8_t> dmaphost, identhost[16];
    std::vector<uint16_t> remaphost;
    std::vector<uint32_t> cumhost;
    int segcur = 0;
    uint32_t text_wgs = 2048, pairs_wgs = 1024;
    uint32_t num_cus = 0;          // compute units of the device (chunking of the one-workgroup-per-CU text kernels)
    bool part_r3 = false;         // probes: round 3 form of the partition kernel (A/B partner)
    bool no_dna_table = false;    // always take the general code table
    bool detect_period = true;    // periodic run tokens for groups whose common prefix is periodic
    uint32_t msd_groups = 8;      // groups of workgroups sharing write cursors (one per XCD)
    int deep_digit_bits = 10;     // digit width of the passes of a re-keying level
    uint32_t dbl_min_share = 1;   // 0: prefix doubling off (probes)
    // re-keying levels: groups sorted where they lie (k_group_sort_*) instead of by whole-level LSD passes
    int mask_digit_bits = 10;         // digit width of the LSD passes of a seed-mask build (whole symbols)
    bool mask_lcp_from_keys = true;   // probes: off = the LCP of a seed-mask build is counted in the text (a sector per rank)
    bool group_sort = true;
    static constexpr uint32_t GS_CAP = 4096;        // records of a window of small groups (512 threads x 8)
    // groups above gs_giant: side by side, sorted by whole-device passes; up to it: ONE workgroup per group, ping-pong over the
    // group's own range (it stays in the L2).  With thousands of groups on a level (the left-over buckets of a --dna build:
    // 6 870 of up to 855 000 members) a workgroup per group of up to 131 072 records keeps the chip busy and takes two thirds of
    // the records out of the whole-device passes (--dna stand-in: 332 -> 318 ms, A/B); with a few dozen groups (the headline
    // build's) the same workgroups are a long tail (+3 ms): there the limit stays at 16 384.
    uint32_t gs_giant = 1u << 14;
    uint32_t gs_giant_knob = 0;                      // probes: a fixed limit
    DevBuf gs_leafbase, gs_pst, gs_psz, gs_wcnt, gs_wpre, gs_wdesc, gs_flag, gs_off, gs_big, gs_lg, gs_lsz, gs_loff;
    bool run_groups = true;       // probes: off = buckets of one repeated symbol go through the levels like any other
    bool key_carry = true;        // probes: off = the first level below the tie level reads its keys from the text again
    int p2min_knob = 0;           // probes: digits of a run key a re-keying level sorts at least
    int key_chars_knob = 0;       // probes: characters kept in the 64-bit key (packed alphabets)
    static bool packed_ok_for_knob(int b) { return b >= 2 && b <= 4; }
    uint32_t finish_opts = 0;     // probes build: k_finish phase switches in the top bits of its last argument
    LevelArrays lv[2];
    RunTable rtab{nullptr, nullptr, nullptr, nullptr, 0};
    DevBuf sa32, lcp32;  // used by the u64 / host wrappers
    DevBuf optA, optB, optC, optD, optE;   // --max-query-len / --seed-mask scratch
    DevBuf wideoffs;                       // care offsets of the mask for the merge of a windowed build (sufr_wide.inc)
    // build options set by the C entry points before sort_device_u32 (0 / empty = plain suffix order)
    uint64_t opt_max_query_len = 0;
    uint64_t opt_wide_retry = 0;              // windowed builds: cap of the retry margin (0: what 32 bits allow); sufr_hip_set_window_retry
    uint32_t wide_shard_index = 0, wide_num_shards = 1;   // windowed builds: the shard this call builds (set by the C ABI around the call)
    uint64_t wide_text_len = 0;               // length of the text the windows' normalised copy (ctx->wtext) holds; 0: none
    uint64_t wide_orphans = 0;                // ... of the last windowed build: suffixes ordered by whole-text comparison (sufr_wide.inc)
    std::vector<uint32_t> opt_mask_offsets;   // "care" offsets of the seed mask (types.rs:36-200)
    hipEvent_t ev[16];
    bool have_events = false;

    // geometry of the MSD kernels
    static constexpr int LEAF_E = 8;     // leaf sort: records per thread
    // its workgroup size: 1024 (windows of 8192 records).  512 (two workgroups per CU) sends every bucket above 2048
    // records through another MSD level: a third of the records of the 3.1 Gb stand-in
    int leaf_nt = 512;
    uint32_t LEAF_CAP = 4096;            // records per window = leaf_nt * LEAF_E
    uint32_t LEAF_BIG = 4096;            // leaves above this take another MSD level (BIG <= CAP)
    bool leaf_dna3 = false;              // keys of this build hold the fixed 3-bit DNA codes (k_leaf_sort<.., DNA3>)
    uint32_t leaf_bmax = 256;            // largest bucket the counting path of the leaf sort ranks by comparison (96: +3 ms, 2048: +2.5 ms)
    int leaf_t1 = 12;                    // bits of its counting digit (512 threads: 11 / 12, 1024 threads: 12 / 13)
    int ms_e = 8;                        // k_msd_scatter: records per thread
    static constexpr int ms_nt = 512;    // its workgroup size (tile = ms_nt * ms_e records)

    void set_error(const std::string& s) { err = s; }

    // Small results come back through a pinned staging buffer: a device-to-host copy into pageable memory (a stack variable, a
    // vector) costs ~9 us more per round trip -- 23 against 14 us for kernel + copy + synchronise, profiles/micro/readback.hip --
    // and a build makes 8 (4.6 Mb) to ~30 (3.1 Gb) of them.  d2h_at() queues the copy into the staging buffer, sync_reads() waits for
    // the stream and hands the bytes out; what does not fit the buffer is copied directly.  Every synchronisation of this file
    // goes through sync_reads(); a build that fails between the two leaves its queue to be dropped by the next one (reset_reads).
    static constexpr size_t PIN_CAP = (size_t)512 << 10;
    uint8_t* pin = nullptr;
    size_t pin_used = 0;
    struct PinItem { void* dst; size_t off, bytes; };
    std::vector<PinItem> pin_items;
    // d2h_at(): the copy is queued where the call stands (for sources that kernels launched before the synchronisation overwrite)
    hipError_t d2h_at(void* dst, const void* src, size_t bytes)
    {
        if (!pin || pin_used + bytes > PIN_CAP) { copies_queued = true; return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream); }
        const hipError_t e = hipMemcpyAsync(pin + pin_used, src, bytes, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) { pin_items.push_back({dst, pin_used, bytes}); pin_used += (bytes + 63) & ~(size_t)63; copies_queued = true; }
        return e;
    }
    // read_at_sync(): nothing is queued here -- the source is READ WHEN sync_reads() RUNS, so no kernel that writes it may be
    // launched between the two.  Nothing checks that: every read_at_sync() stands right in front of its sync_reads(), in the same
    // function (the stages of a build were cut so that no pair straddles two of them).  Up to eight small items go out through
    // ONE launch of k_publish into mapped pinned memory, and the host spins on the sequence number behind them: 7 us per round
    // trip against 16 (profiles/micro/readback.hip).  Larger ones, a ninth item, or a context without the mapped buffer take
    // the copies of d2h_at(), queued by sync_reads() itself.
    static constexpr size_t PUB_CAP = 8192;              // bytes of results per round trip through k_publish
    uint8_t* pub = nullptr;                              // mapped pinned memory: PUB_CAP bytes + the sequence word
    uint8_t* pub_dev = nullptr;
    unsigned long long pub_seq = 0;
    bool copies_queued = false;
    bool pub_broken = false;                             // a sequence word that never arrived: copies from then on
    bool pub_drop = false;                               // (probes build, SUFR_PROBE_PUBLISH_DROP: pretend it never arrives)
    struct PubItem { void* dst; const void* src; size_t bytes; };
    std::vector<PubItem> pub_items;
    hipError_t read_at_sync(void* dst, const void* src, size_t bytes)
    {
        pub_items.push_back({dst, src, bytes});
        return hipSuccess;
    }
    // ranges to clear, collected and cleared by one launch (k_zero_ranges)
    ZeroList zlist = {};
    // what a build that failed left queued is dropped (the destinations of its reads are gone)
    void reset_reads() { pin_items.clear(); pin_used = 0; pub_items.clear(); copies_queued = false; zlist.n = 0; }
    hipError_t zero_flush()
    {
        if (!zlist.n) return hipSuccess;
        unsigned long long units = 0;
        for (uint32_t r = 0; r < zlist.n; r++) units += zlist.bytes[r] / 16 + 2;
        uint64_t grid = (units + 256ull * 8 - 1) / (256ull * 8);
        if (grid < 1) grid = 1;
        if (grid > 4096) grid = 4096;
        ZeroSizes zs;
        uint8_t* zp[8];
        for (uint32_t r = 0; r < 8; r++) { zs.bytes[r] = r < zlist.n ? zlist.bytes[r] : 0ull; zp[r] = r < zlist.n ? (uint8_t*)(uintptr_t)zlist.p[r] : nullptr; }
        hipLaunchKernelGGL(k_zero_ranges, dim3((uint32_t)grid), dim3(256), 0, stream, zp[0], zp[1], zp[2], zp[3], zp[4], zp[5], zp[6], zp[7], zs);
        zlist.n = 0;
        return hipGetLastError();
    }
    hipError_t zero_later(void* p, size_t bytes)
    {
        if (!bytes) return hipSuccess;
        if (zlist.n == 8) { const hipError_t e = zero_flush(); if (e != hipSuccess) return e; }
        zlist.p[zlist.n] = (unsigned long long)(uintptr_t)p; zlist.bytes[zlist.n] = bytes; zlist.n++;
        return hipSuccess;
    }
    hipError_t sync_reads()
    {
        bool publish = pub && !pub_broken && !pub_items.empty() && pub_items.size() <= 8 && !copies_queued;
        size_t total = 0;
        for (const PubItem& it : pub_items) {
            if ((it.bytes & 3u) || ((uintptr_t)it.src & 3u)) publish = false;
            total += (it.bytes + 15) & ~(size_t)15;
        }
        if (total > PUB_CAP) publish = false;
        if (publish) {
            PubList pl;
            memset(&pl, 0, sizeof pl);
            uint32_t off = 0;
            for (const PubItem& it : pub_items) {
                pl.src[pl.n] = (const uint32_t*)it.src; pl.words[pl.n] = (uint32_t)(it.bytes / 4); pl.off[pl.n] = off; pl.n++;
                off += (uint32_t)(((it.bytes + 15) & ~(size_t)15) / 4);
            }
            const unsigned long long seq = ++pub_seq;
            unsigned long long* flag = (unsigned long long*)(pub + PUB_CAP);
            hipLaunchKernelGGL(k_publish, dim3(1), dim3(256), 0, stream, pl, (uint32_t*)pub_dev, (unsigned long long*)(pub_dev + PUB_CAP), seq);
            hipError_t e = hipGetLastError();
            if (e == hipSuccess) {
                // spin for a while (the kernels of a small build are microseconds long), then wait the ordinary way
                const auto t0 = std::chrono::steady_clock::now();
                uint32_t spins = 0;
                while (pub_drop || __atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq) {
                    if ((++spins & 255u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(150)) {
                        e = hipStreamSynchronize(stream);
                        break;
                    }
                }
            }
            if (e != hipSuccess) { pub_items.clear(); return e; }
            if (!pub_drop && __atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) {
                uint32_t r = 0;
                for (const PubItem& it : pub_items) { memcpy(it.dst, pub + (size_t)pl.off[r] * 4, it.bytes); r++; }
                pub_items.clear();
                return hipSuccess;
            }
            // The stream is done and the word is not there (host memory this device does not write through?): the values come by
            // copies, now and for the rest of this context's life.
            pub_broken = true;
        }
        for (const PubItem& it : pub_items) {
            const hipError_t e = d2h_at(it.dst, it.src, it.bytes);
            if (e != hipSuccess) { pub_items.clear(); pin_items.clear(); pin_used = 0; copies_queued = false; return e; }
        }
        pub_items.clear();
        const hipError_t e = hipStreamSynchronize(stream);
        if (e == hipSuccess) for (const PinItem& it : pin_items) memcpy(it.dst, pin + it.off, it.bytes);
        pin_items.clear();
        pin_used = 0;
        copies_queued = false;
        return e;
    }

    int init(int dev)
    {
        device = dev;
        int cnt = 0;
        if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) {
            set_error("no HIP device available (libsufr_hip has no CPU fallback)");
            return SUFR_HIP_E_NO_DEVICE;
        }
        if (dev < 0 || dev >= cnt) { set_error("device id out of range"); return SUFR_HIP_E_INVALID; }
        HIP_TRY(hipSetDevice(dev));
        {
            int cus = 0;
            if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) num_cus = (uint32_t)cus;
        }
        HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        own_stream = true;
        for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
        have_events = true;
        if (hipHostMalloc((void**)&pin, PIN_CAP, hipHostMallocDefault) != hipSuccess) { pin = nullptr; (void)hipGetLastError(); }    // (without it: direct copies)
        if (hipHostMalloc((void**)&pub, PUB_CAP + 64, hipHostMallocMapped) != hipSuccess ||
            hipHostGetDevicePointer((void**)&pub_dev, pub, 0) != hipSuccess) {
            if (pub) (void)hipHostFree(pub);
            pub = nullptr; pub_dev = nullptr; (void)hipGetLastError();                                                                // (without it: copies)
        } else {
            memset(pub, 0, PUB_CAP + 64);
        }
        read_env();
        return 0;
    }

    // The device pipeline reads one environment variable, SUFR_HIP_DEBUG (phase messages and order checks on
    // stderr).  Tuning knobs exist only in the probes build (-DSUFR_HIP_PROBES, profiles/*.py).
    void read_env()
    {
        const char* d = getenv("SUFR_HIP_DEBUG");
        debug = d && d[0] && d[0] != '0';
#ifdef SUFR_HIP_PROBES
        pub_drop = getenv("SUFR_PROBE_PUBLISH_DROP") && atoi(getenv("SUFR_PROBE_PUBLISH_DROP"));
        if (const char* e = getenv("SUFR_PROBE_TEXT_WGS")) if (atoi(e) > 0) text_wgs = (uint32_t)atoi(e);
        if (const char* e = getenv("SUFR_PROBE_PAIRS_WGS")) if (atoi(e) > 0) pairs_wgs = (uint32_t)atoi(e);
        if (const char* e = getenv("SUFR_PROBE_GROUPS")) if (atoi(e) > 0 && atoi(e) <= 64) msd_groups = (uint32_t)atoi(e);
        part_r3 = getenv("SUFR_PROBE_PART_R3") && atoi(getenv("SUFR_PROBE_PART_R3"));
        if (const char* e = getenv("SUFR_PROBE_DEEP_BITS")) { int v = atoi(e); if (v >= 4 && v <= 12) deep_digit_bits = v; }
        no_dna_table = getenv("SUFR_PROBE_NO_DNA_TABLE") && atoi(getenv("SUFR_PROBE_NO_DNA_TABLE"));
        no_exceptions = getenv("SUFR_PROBE_NO_EXCEPTIONS") && atoi(getenv("SUFR_PROBE_NO_EXCEPTIONS"));
        mql_fast_ok = !(getenv("SUFR_PROBE_NO_MQL_FAST") && atoi(getenv("SUFR_PROBE_NO_MQL_FAST")));
        overlap_chains = !(getenv("SUFR_PROBE_NO_OVERLAP") && atoi(getenv("SUFR_PROBE_NO_OVERLAP")));
        detect_period = !getenv("SUFR_PROBE_NO_PERIOD");
        if (const char* e = getenv("SUFR_PROBE_LEAF_NT")) if (atoi(e) == 512 || atoi(e) == 1024) leaf_nt = atoi(e);
        LEAF_CAP = (uint32_t)(leaf_nt * LEAF_E); LEAF_BIG = 4096;
        leaf_t1 = 12;
        if (const char* e = getenv("SUFR_PROBE_LEAF_BIG")) if (atoi(e) >= 64) LEAF_BIG = (uint32_t)atoi(e);
        if (LEAF_BIG > LEAF_CAP) LEAF_BIG = LEAF_CAP;
        if (const char* e = getenv("SUFR_PROBE_FINISH_OPTS")) finish_opts = (uint32_t)atoi(e) << 29;
        if (const char* e = getenv("SUFR_PROBE_DBL_SHARE")) dbl_min_share = (uint32_t)atoi(e);      // 0: never
        if (const char* e = getenv("SUFR_PROBE_P2MIN")) p2min_knob = atoi(e);
        key_carry = !getenv("SUFR_PROBE_NO_KEY_CARRY");
        run_groups = !getenv("SUFR_PROBE_NO_RUN_GROUPS");
        mask_lcp_from_keys = !getenv("SUFR_PROBE_MASK_LCP_TEXT");
        if (const char* e = getenv("SUFR_PROBE_MASK_DIGIT_BITS")) { int v = atoi(e); if (v >= 4 && v <= 12) mask_digit_bits = v; }
        if (const char* e = getenv("SUFR_PROBE_GROUP_SORT")) group_sort = atoi(e) != 0;
        if (const char* e = getenv("SUFR_PROBE_GIANT")) if (atoi(e) >= (int)GS_CAP) gs_giant_knob = (uint32_t)atoi(e);
        if (const char* e = getenv("SUFR_PROBE_KEY_CHARS")) key_chars_knob = atoi(e);
        if (const char* e = getenv("SUFR_PROBE_BMAX")) if (atoi(e) >= 1) leaf_bmax = (uint32_t)atoi(e);
        if (const char* e = getenv("SUFR_PROBE_LEAF_ABL")) leaf_bmax |= (uint32_t)atoi(e) << 24;
        if (const char* e = getenv("SUFR_PROBE_MS_E")) if (atoi(e) == 4 || atoi(e) == 6 || atoi(e) == 8) ms_e = atoi(e);
        if (const char* e = getenv("SUFR_PROBE_T1")) if (atoi(e) >= 11 && atoi(e) <= 13) leaf_t1 = atoi(e);
        if (leaf_nt == 512 && leaf_t1 == 13) leaf_t1 = 12;
        if (leaf_nt == 1024 && leaf_t1 == 11) leaf_t1 = 12;
#endif
        if (text_wgs > 16384u) text_wgs = 16384u;       // larger grids were never validated
        if (pairs_wgs > 16384u) pairs_wgs = 16384u;
    }

    void release(DevBuf& b) { if (b.p) (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }

    void destroy()
    {
        if (helper) { helper->destroy(); helper.reset(); }
        (void)hipSetDevice(device);
        DevBuf* all[] = {&text, &bytehist, &lut, &table, &bintot, &binbase, &scalars, &keyA, &keyB, &idxA,
                         &idxB, &recA, &recB, &headsA, &headsB, &sizes, &starts, &partials, &sa32, &lcp32,
                         &tilefirst, &runends, &tileany, &nexttile, &nextblk, &depthA, &depthB, &period, &remapbuf, &flagsbuf, &packedbuf, &wmaskbuf, &wcntbuf, &recoff, &runoff, &wlflag, &wlhead, &wloff, &candbuf, &keepbuf, &plancnt, &fixbuf, &pairsc, &pairbuf,
                         &rg_misc, &rg_blk, &rg_blkoff, &rg_rs, &rg_rl, &rg_E, &rg_L, &rg_V, &rg_tab[0], &rg_tab[1], &rg_off[0], &rg_off[1], &rg_long[0], &rg_long[1], &rg_tmax[0], &rg_tmax[1], &rg_hist, &rg_depth,
                         &exc_pos, &exc_byte, &exc_sorted, &exc_sa, &exc_lcp, &exc_bits, &exc_blk, &exc_off, &exc_list, &exc_list2, &exc_pmin, &exc_roff, &exc_all_sa, &exc_all_lcp,
                         &cumbuf, &dmapbuf, &rawtab, &presbuf, &rawtot, &valsbuf, &startbuf, &grouptab, &gcur, &leafcnt, &leafoff, &leafbase, &leafcur, &bigflag, &bigoff,
                         &segst[0], &segst[1], &segsz[0], &segsz[1], &tunits, &upre, &tdesc, &wunits, &wpre, &wdesc, &wslow,
                         &optA, &optB, &optC, &optD, &optE, &stitchoffs, &wideoffs,
                         &gs_leafbase, &gs_pst, &gs_psz, &gs_wcnt, &gs_wpre, &gs_wdesc, &gs_flag, &gs_off, &gs_big, &gs_lg, &gs_lsz, &gs_loff};
        for (auto& b : identbuf) release(b);
        for (auto& b : dblf) release(b);
        for (auto& b : dblg) release(b);
        release(rankbuf); release(dposbuf); release(deferbuf); release(unresbuf); release(posbitsbuf);
        for (auto* b : all) release(*b);
        for (auto& l : lv) { release(l.keyA); release(l.keyB); release(l.idxA); release(l.idxB);
                             release(l.segA); release(l.segB); release(l.opos); }
        if (have_events) for (auto& e : ev) (void)hipEventDestroy(e);
        if (pin) { (void)hipHostFree(pin); pin = nullptr; }
        if (pub) { (void)hipHostFree(pub); pub = nullptr; pub_dev = nullptr; }
        if (own_stream && stream) (void)hipStreamDestroy(stream);
    }

    // The large build-only arrays handed back while the outputs are still in use (sufr create: the records, packed text
    // and level arrays are ~40 of the ~55 GB of a human-sized build; returned here they leave under the D2H + write phase
    // instead of in the process's exit).  The text, SA / LCP and the small tables stay.
    void release_build_arrays(bool also_text)
    {
        if (helper) helper->release_build_arrays(false);
        (void)hipSetDevice(device);
        if (also_text) { release(text); resident_text_len = 0; }
        DevBuf* big[] = {&recA, &recB, &keyA, &keyB, &idxA, &idxB, &packedbuf, &runends, &startbuf, &wmaskbuf, &wcntbuf, &fixbuf, &exc_sa, &exc_lcp, &exc_bits, &exc_all_sa, &exc_all_lcp,
                         &headsA, &headsB, &rankbuf, &dposbuf, &deferbuf, &unresbuf, &posbitsbuf, &depthA, &depthB, &period,
                         &recoff, &runoff, &candbuf, &keepbuf, &pairbuf, &optA, &optB, &optC, &optD, &optE};
        for (auto* b : big) if (b->cap >= ((size_t)16 << 20)) release(*b);
        for (auto& b : dblf) release(b);
        for (auto& b : dblg) release(b);
        for (auto& l : lv) { release(l.keyA); release(l.keyB); release(l.idxA); release(l.idxB);
                             release(l.segA); release(l.segB); release(l.opos); }
    }

    // (grows like ensure, but what the buffer holds stays)
    int ensure_keep(DevBuf& b, size_t bytes)
    {
        if (b.cap >= bytes || !b.p) return ensure(b, bytes);
        DevBuf nb;
        int rc = ensure(nb, bytes + bytes / 2);
        if (rc) return rc;
        if (hipMemcpyAsync(nb.p, b.p, b.cap, hipMemcpyDeviceToDevice, stream) != hipSuccess || sync_reads() != hipSuccess) {
            (void)hipFree(nb.p);
            set_error("growing a buffer failed");
            return SUFR_HIP_E_HIP;
        }
        (void)hipFree(b.p);
        b = nb;
        return 0;
    }
    int ensure(DevBuf& b, size_t bytes)
    {
        if (bytes < 256) bytes = 256;
        if (b.cap >= bytes) return 0;
        if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
        size_t want = bytes + bytes / 16;
        hipError_t e = hipMalloc(&b.p, want);
        if (e != hipSuccess) {
            b.p = nullptr;
            (void)hipGetLastError();          // reported through the return code: a later launch check must not find it (a caller may go on with less: out-of-core create)
            set_error("hipMalloc(" + std::to_string(want) + " bytes): " + hipGetErrorString(e));
            return SUFR_HIP_E_NOMEM;
        }
        b.cap = want;
        return 0;
    }
    // scalars buffer layout (u64 slots)
    enum { SC_TOTAL = 0, SC_LARGE = 1, SC_MAXSIZE = 2, SC_SCANTOTAL = 3, SC_BAD = 4, SC_MAXTOK = 5, SC_WTOTAL = 6,
           SC_UTOTAL = 7, SC_NBIG = 8, SC_MBIG = 9, SC_MAXBIG = 10, SC_NFIX = 11, SC_TMP0 = 13, SC_TMP1 = 14, SC_GSBIG = 15, SC_GSLARGE = 16 /* and 17 */, SC_N = 24 };
    unsigned long long* sc(int i) { return reinterpret_cast<unsigned long long*>(scalars.p) + i; }

    static int ceil_log2_u64(uint64_t v) { int b = 0; while ((1ull << b) < v && b < 63) b++; return b; }

    // ---- one LSD pass over (key, idx[, seg]) records -------------------------------------------
    // nbins: digit values after the dense remap (remap == nullptr: identity, nbins == raw_bins)
    int radix_pass_pairs(const uint64_t* in_key, const uint32_t* in_idx, const uint32_t* in_seg, uint32_t m,
                         uint32_t nbins, uint32_t raw_bins, const uint16_t* remap, int shift, bool from_seg,
                         uint64_t* out_key, uint32_t* out_idx, uint32_t* out_seg)
    {
        const uint32_t tiles = (m + TILE - 1) / TILE;
        uint32_t nwg = tiles < pairs_wgs ? tiles : pairs_wgs;
        if (nwg < 1) nwg = 1;
        uint32_t tiles_per = (tiles + nwg - 1) / nwg;
        tiles_per = (tiles_per + 1u) & ~1u;            // chunks are multiples of every tile size (<= 8192)
        uint32_t chunk = tiles_per * TILE;
        nwg = (m + chunk - 1) / chunk;
        const int nbits = ceil_log2_u64(nbins) < 1 ? 1 : ceil_log2_u64(nbins);
        int rc;
        if ((rc = ensure(table, (size_t)nwg * nbins * 4))) return rc;
        if ((rc = ensure(bintot, (size_t)nbins * 4))) return rc;
        if ((rc = ensure(binbase, (size_t)nbins * 4))) return rc;
        const size_t rm_bytes = remap ? (size_t)((raw_bins + 7u) & ~7u) * 2 : 0;
        hipLaunchKernelGGL(k_hist_pairs, dim3(nwg), dim3(THREADS), (size_t)nbins * 4 + rm_bytes, stream, in_key,
                           from_seg ? in_seg : (const uint32_t*)nullptr, m, nbins, raw_bins, remap, shift, chunk,
                           (uint32_t*)table.p);
        hipLaunchKernelGGL(k_scan_table_cols, dim3((nbins + 255) / 256), dim3(256), 0, stream,
                           (uint32_t*)table.p, nwg, nbins, (uint32_t*)bintot.p);
        hipLaunchKernelGGL(k_scan_bins, dim3(1), dim3(256), 0, stream, (const uint32_t*)bintot.p, nbins,
                           (uint32_t*)binbase.p, (unsigned long long*)nullptr);
        const bool has_seg = in_seg != nullptr;
        const size_t nba = (nbins + 3u) & ~3u;
#define SUFR_LAUNCH_PAIRS_NB(SEG, NT_, E_, NB_)                                                                 \
        {                                                                                                      \
            size_t stage = (size_t)(NT_ * E_) * (SEG ? 16 : 12);                                              \
            size_t wc = ((size_t)(NT_ / 64) * nbins * 2 + 15) & ~(size_t)15;                                  \
            size_t lds = nba * 12 + 128 + rm_bytes + (stage > wc ? stage : wc);                               \
            HIP_TRY(hipFuncSetAttribute((const void*)k_scatter_pairs<SEG, NT_, E_, NB_>,                      \
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));               \
            hipLaunchKernelGGL((k_scatter_pairs<SEG, NT_, E_, NB_>), dim3(nwg), dim3(NT_), lds, stream, in_key, \
                               in_idx, in_seg, m, nbins, nbits, raw_bins, remap, shift, from_seg ? 1 : 0,     \
                               chunk, (const uint32_t*)table.p, (const uint32_t*)binbase.p, out_key, out_idx, \
                               out_seg);                                                                      \
        }
        // the ballot loop of the stable ranking is unrolled for the common digit widths
#define SUFR_LAUNCH_PAIRS(SEG, NT_, E_)                                                   \
        if (nbits == 10) SUFR_LAUNCH_PAIRS_NB(SEG, NT_, E_, 10)                            \
        else SUFR_LAUNCH_PAIRS_NB(SEG, NT_, E_, 0)
        if (has_seg) {
            SUFR_LAUNCH_PAIRS(true, 256, 16)
        } else {
            SUFR_LAUNCH_PAIRS(false, 512, 8)
        }
#undef SUFR_LAUNCH_PAIRS
#undef SUFR_LAUNCH_PAIRS_NB
        HIP_TRY(hipGetLastError());
        return 0;
    }

    // text kernels are compiled for the common character widths; anything else takes the generic path
#define SUFR_DISPATCH_B(bits, CALL)                 \
    switch (bits) {                                 \
        case 2: { constexpr int BB = 2; CALL; } break; \
        case 3: { constexpr int BB = 3; CALL; } break; \
        case 4: { constexpr int BB = 4; CALL; } break; \
        case 5: { constexpr int BB = 5; CALL; } break; \
        default: { constexpr int BB = 0; CALL; } break; \
    }

    int launch_hist_text(uint32_t grid, size_t lds, const uint8_t* d_text, uint64_t n, const KeyParams& kp,
                         const uint16_t* remap, int shift, uint64_t tchunk, uint32_t lo, uint32_t hi,
                         uint32_t tile_stride = 1)
    {
        SUFR_DISPATCH_B(kp.b, {
            HIP_TRY(hipFuncSetAttribute((const void*)k_hist_text<BB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(k_hist_text<BB>, dim3(grid), dim3(THREADS), lds, stream, d_text, n,
                               (const uint16_t*)lut.p, remap, kp, shift, tchunk, lo, hi, tile_stride, (uint32_t*)table.p);
        });
        HIP_TRY(hipGetLastError());
        return 0;
    }
    // level 1 for alphabets without a bit-packed stream (b = 1 or b >= 5): the text-staging partition kernel
    // on the top digit, per-workgroup slots from the [workgroup][bin] table
    int launch_scatter_text(uint32_t grid, const uint8_t* d_text, uint64_t n, const KeyParams& kp,
                            const uint16_t* remap, int shift, uint64_t tchunk, uint32_t lo, uint32_t hi,
                            bool sharded, Rec* orec)
    {
        const size_t nba = (kp.nbins + 3u) & ~3u;
        const size_t rm_bytes = remap ? (size_t)kp.raw_bins * 2 : 0;
#define SUFR_LAUNCH_ST(BB_, NT_, E_, SH_)                                                                      \
        {                                                                                                      \
            size_t lds = nba * 12 + (size_t)(NT_ * E_) * 13 + HALO + 512 + 128 + rm_bytes;                    \
            HIP_TRY(hipFuncSetAttribute((const void*)k_scatter_text<BB_, NT_, E_, SH_>,                       \
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));               \
            hipLaunchKernelGGL((k_scatter_text<BB_, NT_, E_, SH_>), dim3(grid), dim3(NT_), lds, stream,       \
                               d_text, n, (const uint16_t*)lut.p, remap, kp, shift, tchunk, lo, hi,           \
                               (const uint32_t*)table.p, (const uint32_t*)binbase.p, orec);                   \
        }
        if (kp.b == 5) { if (sharded) SUFR_LAUNCH_ST(5, 256, 16, true) else SUFR_LAUNCH_ST(5, 256, 16, false) }
        else { if (sharded) SUFR_LAUNCH_ST(0, 256, 16, true) else SUFR_LAUNCH_ST(0, 256, 16, false) }
#undef SUFR_LAUNCH_ST
        HIP_TRY(hipGetLastError());
        return 0;
    }
    int launch_presence(uint32_t grid, size_t lds, const uint8_t* d_text, uint64_t n, const KeyParams& kp,
                        uint64_t tchunk, uint32_t* flags, uint8_t* packed)
    {
        SUFR_DISPATCH_B(kp.b, {
            HIP_TRY(hipFuncSetAttribute((const void*)k_digit_presence<BB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(k_digit_presence<BB>, dim3(grid), dim3(THREADS), lds, stream, d_text, n,
                               (const uint16_t*)lut.p, kp, tchunk, flags, packed);
        });
        HIP_TRY(hipGetLastError());
        return 0;
    }

    int check_sorted(const char* what, const uint64_t* keys, const uint32_t* segs, uint32_t m, int shift)
    {
        if (!debug || m < 2) return 0;
        unsigned long long init = ~0ull;
        HIP_TRY(hipMemcpyAsync(sc(SC_BAD), &init, 8, hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(k_check_sorted, dim3((m + 255) / 256), dim3(256), 0, stream, keys, segs, m, shift,
                           (uint32_t*)sc(SC_BAD));
        unsigned long long got = 0;
        HIP_TRY(read_at_sync(&got, sc(SC_BAD), 8));
        HIP_TRY(sync_reads());
        uint32_t bad = (uint32_t)got;
        fprintf(stderr, "[sufr_hip debug] %s: m=%u shift=%d first_unsorted=%s%u\n", what, m, shift,
                bad == 0xffffffffu ? "none " : "", bad);
        if (bad != 0xffffffffu) { set_error(std::string("debug: records not sorted after ") + what); return SUFR_HIP_E_HIP; }
        return 0;
    }

    // ---- exclusive scan of `count` u32 values; total -> scalars[SC_SCANTOTAL] ---------------------
    // total_also: a second scalar that receives the total (besides SC_SCANTOTAL)
    int scan_u32(const uint32_t* in, uint32_t count, uint32_t* out, unsigned long long* total_also = nullptr)
    {
        if (count <= SCAN1_MAX) {
            hipLaunchKernelGGL(k_scan_small, dim3(1), dim3(1024), 0, stream, in, count, out, sc(SC_SCANTOTAL), total_also);
            HIP_TRY(hipGetLastError());
            return 0;
        }
        if (count <= SCANM_MAX && (((uintptr_t)in | (uintptr_t)out) & 15u) == 0) {
            hipLaunchKernelGGL(k_scan_medium, dim3(1), dim3(1024), 0, stream, in, count, out, sc(SC_SCANTOTAL), total_also);
            HIP_TRY(hipGetLastError());
            return 0;
        }
        uint32_t nb = (count + SCAN_ITEMS - 1) / SCAN_ITEMS;
        if (nb < 1) nb = 1;
        int rc;
        if ((rc = ensure(partials, (size_t)nb * 4))) return rc;
        hipLaunchKernelGGL(k_scan_reduce, dim3(nb), dim3(256), 0, stream, in, count, (uint32_t*)partials.p);
        hipLaunchKernelGGL(k_scan_partials, dim3(1), dim3(256), 0, stream, (uint32_t*)partials.p, nb,
                           sc(SC_SCANTOTAL), total_also);
        hipLaunchKernelGGL(k_scan_apply, dim3(nb), dim3(256), 0, stream, in, count,
                           (const uint32_t*)partials.p, out);
        HIP_TRY(hipGetLastError());
        return 0;
    }

    // ---- finishing a sorted level: k_plan_windows cuts it into windows of <= 128 records that start and end at group heads
    // and lists the groups above a window (the next level's groups, in heads_out); k_finish<PLANNED> orders every group of the
    // windows.  One host round trip for the two totals (rounds 2-3: fixed windows, a second launch for the groups that
    // crossed a window's end, two round trips).
    int finish_level(const uint64_t* k1, const uint32_t* i1, const uint32_t* s1, const uint32_t* op, const uint32_t* dn,
                     uint32_t m2, int sbits2, const uint8_t* d_text, uint64_t n, const KeyParams& kp, uint32_t* d_sa,
                     uint32_t* d_lcp, DevBuf* heads_out, uint32_t& L_out)
    {
        int rc;
        L_out = 0;
        const uint32_t nchunk = (m2 + PLAN_CH - 1) / PLAN_CH;
        const size_t ncnt = ((size_t)nchunk + 3) & ~(size_t)3;               // (the second half stays 16-byte aligned: one-launch scans)
        if ((rc = ensure(candbuf, (size_t)nchunk * PLAN_W * 8))) return rc;   // window slots of the chunks
        if ((rc = ensure(keepbuf, (size_t)nchunk * PLAN_L * 4))) return rc;   // large-group slots
        if ((rc = ensure(plancnt, ncnt * 2 * 4))) return rc;
        if ((rc = ensure(wloff, ncnt * 2 * 4))) return rc;
        uint32_t* wcnt = (uint32_t*)plancnt.p; uint32_t* lcnt = wcnt + ncnt;
        uint32_t* woff = (uint32_t*)wloff.p; uint32_t* loff = woff + ncnt;
        hipLaunchKernelGGL(k_plan_windows, dim3((nchunk + 3) / 4), dim3(256), 0, stream, k1, s1, op, dn, m2, sbits2, kp.b, d_lcp,
                           (uint2*)candbuf.p, (uint32_t*)keepbuf.p, wcnt, lcnt, nchunk);
        if ((rc = scan_u32(wcnt, nchunk, woff, sc(SC_TMP0)))) return rc;
        if ((rc = scan_u32(lcnt, nchunk, loff, sc(SC_TMP1)))) return rc;
        unsigned long long tot[2] = {0, 0};
        HIP_TRY(read_at_sync(tot, sc(SC_TMP0), 16));
        HIP_TRY(sync_reads());
        const uint32_t W = (uint32_t)tot[0], L1 = (uint32_t)tot[1];
        if ((rc = ensure(wlhead, ((size_t)W + 2) * 4))) return rc;
        if ((rc = ensure(wlflag, ((size_t)W + 2) * 4))) return rc;
        if ((rc = ensure(*heads_out, ((size_t)L1 + 2) * 4))) return rc;
        hipLaunchKernelGGL(k_plan_compact, dim3((uint32_t)(((uint64_t)nchunk * (PLAN_W + PLAN_L) + 255) / 256)), dim3(256), 0, stream,
                           (const uint2*)candbuf.p, (const uint32_t*)keepbuf.p, (const uint32_t*)wcnt, (const uint32_t*)lcnt,
                           (const uint32_t*)woff, (const uint32_t*)loff, nchunk, (uint32_t*)wlhead.p, (uint32_t*)wlflag.p,
                           (uint32_t*)heads_out->p);
        if (W)
            hipLaunchKernelGGL((k_finish<true, false, true>), dim3((W + 3) / 4), dim3(256), 0, stream, k1, i1, s1, op, dn, m2,
                               d_text, n, rtab, (const uint16_t*)lut.p, kp, sbits2, d_sa, d_lcp, (uint32_t*)wlflag.p,
                               (uint32_t*)wlhead.p, (uint32_t*)nullptr, (unsigned long long*)nullptr, (uint32_t*)nullptr,
                               W | finish_opts);
        HIP_TRY(hipGetLastError());
        L_out = L1;
        return 0;
    }


    // ---- buckets of one repeated symbol: closed-form order (sufr_runs.inc) ------------------------------------------------
    // prepare (before the re-keying levels take the left-over buckets): find the buckets c^K of at least RG_MIN_SIZE records,
    // list the runs of c that are at least K long, check that they account for the bucket record by record, and replace the
    // bucket's records by the last member of every run.  expand (after the levels): the bucket's first M places hold the
    // runs in tail order; every other member is placed by counting.
    DblShard dbl_shard{nullptr, 0, 0, 0u, 0u, 0};   // this build's place among the shards (run_doubling)
    struct RunGroupState { RunGroup g; uint32_t M, rcap, K; size_t run_off; };
    std::vector<RunGroupState> rg_active;
    size_t rg_run_off = 0;

    // K: characters the bucket's members share (all of the key; or the first digit's, `early`: then the records are seeded whole
    // into recs_dst and the caller takes the bucket off the list of the MSD levels).  Appends to rg_active.
    int run_groups_find(const uint8_t* d_text, uint64_t n, const KeyParams& kp, const Rec* recs_src, Rec* recs_dst,
                        const uint32_t* seg_start, uint32_t* seg_size, uint32_t nseg, uint32_t K, uint32_t min_size, bool early)
    {
        if (!run_groups || !rtab.ends || !nseg || K < 2) return 0;
        int rc;
        if ((rc = ensure(rg_misc, 65536))) return rc;
        uint32_t* misc = (uint32_t*)rg_misc.p;                 // [0] count, [16..] groups
        HIP_TRY(hipMemsetAsync(misc, 0, 64, stream));
        hipLaunchKernelGGL(k_rg_detect, dim3((nseg + 255) / 256), dim3(256), 0, stream, recs_src, seg_start,
                           (const uint32_t*)seg_size, nseg, kp.b, (int)K, min_size, d_text, (RunGroup*)(misc + 16), misc);
        uint32_t hostbuf[16 + 6 * RG_MAX_GROUPS];
        HIP_TRY(read_at_sync(hostbuf, misc, sizeof hostbuf));
        HIP_TRY(sync_reads());
        const uint32_t ng = hostbuf[0] < RG_MAX_GROUPS ? hostbuf[0] : RG_MAX_GROUPS;
        if (!ng) return 0;
        const uint64_t nwords = (n + 63) / 64;
        const uint32_t nblk = (uint32_t)((nwords + 255) / 256);
        if ((rc = ensure(rg_blk, (size_t)nblk * 4))) return rc;
        if ((rc = ensure(rg_blkoff, (size_t)nblk * 4))) return rc;
        for (uint32_t gi = 0; gi < ng; gi++) {
            RunGroup g;
            memcpy(&g, hostbuf + 16 + 6 * gi, sizeof g);
            const size_t run_off = rg_run_off;
            hipLaunchKernelGGL((k_rg_runs<0>), dim3(nblk), dim3(256), 0, stream, d_text, n, rtab, g.symbol, K,
                               (const uint32_t*)nullptr, (uint32_t*)rg_blk.p, (uint32_t*)nullptr, (uint32_t*)nullptr,
                               (uint32_t*)nullptr, (unsigned long long*)nullptr);
            if ((rc = scan_u32((const uint32_t*)rg_blk.p, nblk, (uint32_t*)rg_blkoff.p))) return rc;
            unsigned long long tot = 0;
            HIP_TRY(read_at_sync(&tot, sc(SC_SCANTOTAL), 8));
            HIP_TRY(sync_reads());
            const uint32_t M = (uint32_t)tot;
            if (!M || M > g.size) continue;
            if ((rc = ensure_keep(rg_rs, (run_off + M) * 4))) return rc;
            if ((rc = ensure_keep(rg_rl, (run_off + M) * 4))) return rc;
            if ((rc = ensure(rg_hist, ((size_t)RG_REPL * RG_HBINS + 2 * RG_REPL) * 4))) return rc;
            uint32_t* lhist = (uint32_t*)rg_hist.p;            // RG_REPL x RG_HBINS counters, then RG_REPL record sums
            HIP_TRY(hipMemsetAsync(lhist, 0, ((size_t)RG_REPL * RG_HBINS + 2 * RG_REPL) * 4, stream));
            hipLaunchKernelGGL((k_rg_runs<1>), dim3(nblk), dim3(256), 0, stream, d_text, n, rtab, g.symbol, K,
                               (const uint32_t*)rg_blkoff.p, (uint32_t*)nullptr, (uint32_t*)rg_rs.p + run_off,
                               (uint32_t*)rg_rl.p + run_off, lhist, (unsigned long long*)(lhist + (size_t)RG_REPL * RG_HBINS));
            std::vector<uint32_t> hr((size_t)RG_REPL * RG_HBINS + 2 * RG_REPL);
            HIP_TRY(read_at_sync(hr.data(), lhist, hr.size() * 4));
            HIP_TRY(sync_reads());
            std::vector<uint32_t> h(RG_HBINS, 0u);
            unsigned long long records = 0;
            for (uint32_t q = 0; q < RG_REPL; q++) {
                for (uint32_t i = 0; i < RG_HBINS; i++) h[i] += hr[(size_t)q * RG_HBINS + i];
                unsigned long long part; memcpy(&part, hr.data() + (size_t)RG_REPL * RG_HBINS + 2 * q, 8); records += part;
            }
            if (records != g.size) {                           // not what it looked like: the levels take it as it is
                if (debug) fprintf(stderr, "[sufr_hip debug] run bucket of '%c': %llu records by its runs, %u in the bucket -- left to the levels\n",
                                   (char)g.symbol, records, g.size);
                continue;
            }
            // levels up to rcap in the table, at most RG_NLONG longer runs beside it
            uint32_t cum = 0; int bin = (int)RG_HBINS - 1;
            for (; bin >= 1; bin--) { if (cum + h[bin] > RG_NLONG) break; cum += h[bin]; }
            if (bin == (int)RG_HBINS - 1) continue;           // thousands of runs beyond 65 535 symbols: not this way
            const uint32_t rcap = (uint32_t)(bin + 1) * 16u - 1u;
            if ((uint64_t)(rcap + 1) * ((M + 255) / 256 + 2) > RG_TABLE_MAX) continue;
            {
                // what run_groups_expand will allocate for this bucket (three arrays of M, a table and its scan per class): taken
                // NOW, while the bucket can still be left to the levels -- k_rg_seed overwrites its records, and an allocation
                // that fails afterwards would fail the whole build (advisor r4)
                const uint64_t cells = (uint64_t)(rcap + 1) * ((M + 255) / 256 + 2);
                DevBuf* need[] = {&rg_E, &rg_L, &rg_V, &rg_tab[0], &rg_tab[1], &rg_off[0], &rg_off[1]};
                const uint64_t want[] = {(uint64_t)M * 4, (uint64_t)M * 4, (uint64_t)M * 4, cells * 4, cells * 4, cells * 4, cells * 4};
                uint64_t missing = 0;
                for (int q = 0; q < 7; q++) if (need[q]->cap < want[q]) missing += want[q];
                size_t fr = 0, tot = 0;
                bool fits = missing == 0 || (hipMemGetInfo(&fr, &tot) == hipSuccess && missing + ((uint64_t)256 << 20) <= fr);
                for (int q = 0; fits && q < 7; q++) if (ensure(*need[q], want[q]) != 0) { fits = false; err.clear(); }
                if (!fits) {
                    if (debug) fprintf(stderr, "[sufr_hip debug] run bucket of '%c': %llu bytes of tables do not fit the free device memory -- left to the levels\n",
                                       (char)g.symbol, (unsigned long long)missing);
                    continue;
                }
            }
            hipLaunchKernelGGL(k_rg_seed, dim3((M + 255) / 256), dim3(256), 0, stream, (const uint32_t*)rg_rs.p + run_off,
                               (const uint32_t*)rg_rl.p + run_off, M, K, recs_dst, g.start, early ? (uint32_t*)nullptr : seg_size, g.seg,
                               early ? 1 : 0, g.klo, g.khi, g.size);
            if (debug) fprintf(stderr, "[sufr_hip debug] run bucket of '%c'%s: %u records in %u runs of %u and more, table levels 0..%u, %u longer runs\n",
                               (char)g.symbol, early ? " (after the first level)" : "", g.size, M, K, rcap, cum);
            rg_active.push_back(RunGroupState{g, M, rcap, K, run_off});
            rg_run_off += M;
        }
        HIP_TRY(hipGetLastError());
        return 0;
    }

    int run_groups_expand(const uint8_t* d_text, uint64_t n, const KeyParams& kp, uint32_t* d_sa, uint32_t* d_lcp)
    {
        int rc;
        (void)kp;
        for (const RunGroupState& S : rg_active) {
            const uint32_t M = S.M, start = S.g.start, rcap = S.rcap, K = S.K;
            const uint32_t* rs = (const uint32_t*)rg_rs.p + S.run_off;
            const uint32_t* rl = (const uint32_t*)rg_rl.p + S.run_off;
            if ((rc = ensure(rg_E, (size_t)M * 4)) || (rc = ensure(rg_L, (size_t)M * 4)) || (rc = ensure(rg_V, (size_t)M * 4))) return rc;
            uint32_t* misc = (uint32_t*)rg_misc.p;             // [0..7] scalars, [8] long count, [16..] long list, ...
            HIP_TRY(hipMemsetAsync(misc, 0, 64, stream));
            hipLaunchKernelGGL(k_rg_order, dim3((M + 255) / 256), dim3(256), 0, stream, (const uint32_t*)d_sa, (const uint32_t*)d_lcp,
                               start, M, rs, rl, K, d_text, n, S.g.symbol, (uint32_t*)rg_E.p, (uint32_t*)rg_L.p, (uint32_t*)rg_V.p, misc);
            hipLaunchKernelGGL(k_rg_long_list, dim3((M + 255) / 256), dim3(256), 0, stream, (const uint32_t*)rg_L.p, M, rcap,
                               misc + 16, misc + 8);
            std::vector<uint32_t> hb(16 + RG_NLONG);
            HIP_TRY(read_at_sync(hb.data(), misc, hb.size() * 4));
            HIP_TRY(sync_reads());
            if (hb[3] || hb[8] > RG_NLONG) { set_error("internal error: a run bucket did not come back in run order"); return SUFR_HIP_E_HIP; }
            const uint32_t M1 = hb[0], M0 = M - M1, R0max = hb[1], R1max = hb[2], nlong = hb[8];
            std::vector<uint32_t> tl(hb.begin() + 16, hb.begin() + 16 + nlong);
            std::sort(tl.begin(), tl.end());
            // the long runs: E, L, min V since the long run before
            std::vector<uint32_t> gap(nlong), el(2 * (size_t)nlong);
            uint32_t* d_tl = misc + 4096; uint32_t* d_gap = d_tl + RG_NLONG; uint32_t* d_el = d_gap + RG_NLONG;   // (64 KB: 16 K words)
            if (nlong) {
                HIP_TRY(hipMemcpyAsync(d_tl, tl.data(), (size_t)nlong * 4, hipMemcpyHostToDevice, stream));
                HIP_TRY(hipMemsetAsync(d_gap, 0xff, (size_t)nlong * 4, stream));
                hipLaunchKernelGGL(k_rg_long_gaps, dim3((M + 255) / 256), dim3(256), 0, stream, (const uint32_t*)rg_V.p,
                                   (const uint32_t*)rg_E.p, (const uint32_t*)rg_L.p, M, (const uint32_t*)d_tl, nlong, d_gap, d_el);
                HIP_TRY(d2h_at(gap.data(), d_gap, (size_t)nlong * 4));
                HIP_TRY(d2h_at(el.data(), d_el, (size_t)nlong * 8));
            }
            // the tables of the two classes: counts, one scan each
            RunRows R[2];
            uint64_t T[2] = {0, 0};
            for (int cls = 0; cls < 2; cls++) {
                RunRows& P = R[cls];
                P.ta = cls ? M0 : 0u; P.nt = cls ? M1 : M0; P.ntiles = (P.nt + 255) / 256; P.rcap = rcap; P.desc = (uint32_t)cls;
                P.K = K; P.base = 0; P.first_r = 0xffffffffu; P.first_lcp = RG_KEEP;
                if (!P.nt) continue;
                const size_t cells = (size_t)(rcap + 1) * P.ntiles;
                if ((rc = ensure(rg_tab[cls], cells * 4)) || (rc = ensure(rg_off[cls], cells * 4))) return rc;
                HIP_TRY(hipMemsetAsync(rg_tab[cls].p, 0, cells * 4, stream));
                if ((rc = ensure(rg_tmax[cls], (size_t)P.ntiles * 4))) return rc;
                hipLaunchKernelGGL((k_rg_rows<0>), dim3((P.ntiles + 3) / 4), dim3(256), 0, stream, P, (const uint32_t*)rg_E.p,
                                   (const uint32_t*)rg_L.p, (const uint32_t*)rg_V.p, (uint32_t*)rg_tab[cls].p, (uint32_t*)rg_tmax[cls].p,
                                   d_sa, d_lcp);
                if ((rc = scan_u32((const uint32_t*)rg_tab[cls].p, (uint32_t)cells, (uint32_t*)rg_off[cls].p, sc(cls ? SC_TMP1 : SC_TMP0)))) return rc;
            }
            unsigned long long tt[2] = {0, 0};
            HIP_TRY(read_at_sync(tt, sc(SC_TMP0), 16));
            HIP_TRY(sync_reads());
            if (R[0].nt) T[0] = tt[0];
            if (R[1].nt) T[1] = tt[1];
            // the rectangles above the table, per class: between two consecutive lengths of long runs the list of runs is fixed
            std::vector<uint32_t> desc[2], loff[2], lists[2];
            uint64_t Lg[2] = {0, 0};
            for (int cls = 0; cls < 2; cls++) {
                std::vector<uint32_t> ks;                      // long runs of the class, in tail order
                for (uint32_t k = 0; k < nlong; k++) if ((tl[k] < M0) == (cls == 0)) ks.push_back(k);
                if (ks.empty()) continue;
                std::vector<uint32_t> bps;
                for (uint32_t k : ks) bps.push_back(el[2 * k + 1]);
                std::sort(bps.begin(), bps.end());
                bps.erase(std::unique(bps.begin(), bps.end()), bps.end());
                struct Iv { uint32_t r_lo, nlev, a, lo; };
                std::vector<Iv> ivs;
                uint32_t prev = rcap;
                for (uint32_t b : bps) {
                    Iv iv{prev, b - prev, 0u, (uint32_t)(lists[cls].size() / 2)};
                    uint32_t running = 0xffffffffu;
                    for (uint32_t k : ks) {
                        running = gap[k] < running ? gap[k] : running;
                        if (el[2 * k + 1] >= b) { lists[cls].push_back(el[2 * k]); lists[cls].push_back(running); running = 0xffffffffu; iv.a++; }
                    }
                    ivs.push_back(iv);
                    prev = b;
                }
                if (cls) std::reverse(ivs.begin(), ivs.end());  // class 1: the longest first
                for (const Iv& iv : ivs) {
                    desc[cls].push_back((uint32_t)Lg[cls]); desc[cls].push_back(iv.r_lo); desc[cls].push_back(iv.nlev); desc[cls].push_back(iv.a);
                    loff[cls].push_back(iv.lo);
                    Lg[cls] += (uint64_t)iv.nlev * iv.a;
                }
            }
            const uint64_t S0 = T[0] + Lg[0];
            if (S0 + Lg[1] + T[1] != S.g.size) { set_error("internal error: a run bucket's blocks do not add up"); return SUFR_HIP_E_HIP; }
            const uint32_t boundary = S0 ? K + (R0max < R1max ? R0max : R1max) : RG_KEEP;
            R[0].base = start; R[0].first_r = 0u; R[0].first_lcp = RG_KEEP;
            R[1].base = start + (uint32_t)(S0 + Lg[1]);
            if (!Lg[1]) { R[1].first_r = R1max; R[1].first_lcp = boundary; }
            for (int cls = 0; cls < 2; cls++)
                if (R[cls].nt)
                    hipLaunchKernelGGL((k_rg_rows<1>), dim3((R[cls].ntiles + 3) / 4), dim3(256), 0, stream, R[cls], (const uint32_t*)rg_E.p,
                                       (const uint32_t*)rg_L.p, (const uint32_t*)rg_V.p, (uint32_t*)rg_off[cls].p,
                                       (uint32_t*)rg_tmax[cls].p, d_sa, d_lcp);
            for (int cls = 0; cls < 2; cls++) {
                if (!Lg[cls]) continue;
                const size_t nd = desc[cls].size(), nl = loff[cls].size(), ne = lists[cls].size();
                if ((rc = ensure(rg_long[cls], (nd + nl + ne) * 4))) return rc;
                uint32_t* dl = (uint32_t*)rg_long[cls].p;
                // (pageable host vectors: the copies are done when the calls return)
                HIP_TRY(hipMemcpyAsync(dl, desc[cls].data(), nd * 4, hipMemcpyHostToDevice, stream));
                HIP_TRY(hipMemcpyAsync(dl + nd, loff[cls].data(), nl * 4, hipMemcpyHostToDevice, stream));
                HIP_TRY(hipMemcpyAsync(dl + nd + nl, lists[cls].data(), ne * 4, hipMemcpyHostToDevice, stream));
                HIP_TRY(sync_reads());
                RunLong Q;
                Q.nint = (uint32_t)nl; Q.total = (uint32_t)Lg[cls]; Q.K = K; Q.desc_order = (uint32_t)cls;
                Q.base = cls ? start + (uint32_t)S0 : start + (uint32_t)T[0];
                Q.first_lcp = cls ? boundary : RG_KEEP;
                hipLaunchKernelGGL(k_rg_long_emit, dim3((Q.total + 255) / 256), dim3(256), 0, stream, Q, (const uint32_t*)dl,
                                   (const uint32_t*)(dl + nd), (const uint32_t*)(dl + nd + nl), d_sa, d_lcp);
            }
            for (int cls = 0; cls < 2; cls++)
                if (R[cls].nt)
                    hipLaunchKernelGGL(k_rg_fix, dim3((uint32_t)(((uint64_t)(rcap + 1) * R[cls].ntiles + 255) / 256)), dim3(256), 0, stream,
                                       R[cls], (const uint32_t*)rg_off[cls].p, (const uint32_t*)rg_tmax[cls].p, (const uint32_t*)d_sa, d_lcp,
                                       d_text, n, (const uint32_t*)rg_L.p, (const uint32_t*)rg_V.p);
            HIP_TRY(hipGetLastError());
        }
        rg_active.clear();
        rg_run_off = 0;
        return 0;
    }

    // Run buckets taken out after the FIRST level: a first digit c^D whose bucket is a good share of all suffixes (the N bucket of
    // an --allow-ambiguity build; a text of one symbol) would otherwise travel through every further MSD level as one segment of
    // one digit value -- 10 ps per record and level for nothing.  The bucket leaves the list of big leaves here (the list is a
    // few thousand entries after the first level: edited on the host), its places [start, start + size) are filled at the end.
    int run_groups_extract(const uint8_t* d_text, uint64_t n, const KeyParams& kp, const Rec* recs_src, Rec* recs_dst, uint32_t D,
                           uint64_t s_total, const FinishOut& fo, uint32_t& nseg, uint64_t& m, uint64_t& maxbig)
    {
        int rc;
        const size_t before = rg_active.size();
        uint64_t share = s_total / 32;
        const uint32_t min_size = share > RG_MIN_SIZE ? (uint32_t)(share < 0xffffffffull ? share : 0xffffffffull) : RG_MIN_SIZE;
        if (maxbig < min_size) return 0;                     // (no bucket of that size: no launch, no round trip)
        if ((rc = run_groups_find(d_text, n, kp, recs_src, recs_dst, (const uint32_t*)segst[segcur].p, (uint32_t*)segsz[segcur].p, nseg, D,
                                  min_size, true))) return rc;
        const size_t ne = rg_active.size() - before;
        if (!ne) return 0;
        std::vector<uint32_t> hs(nseg), hz(nseg);
        HIP_TRY(read_at_sync(hs.data(), segst[segcur].p, (size_t)nseg * 4));
        HIP_TRY(read_at_sync(hz.data(), segsz[segcur].p, (size_t)nseg * 4));
        HIP_TRY(sync_reads());
        std::vector<uint32_t> taken;
        for (size_t i = before; i < rg_active.size(); i++) taken.push_back(rg_active[i].g.start);
        uint32_t k2 = 0; uint64_t m2 = 0, mx = 0;
        for (uint32_t k = 0; k < nseg; k++) {
            if (std::find(taken.begin(), taken.end(), hs[k]) != taken.end()) continue;
            hs[k2] = hs[k]; hz[k2] = hz[k]; m2 += hz[k]; mx = hz[k] > mx ? hz[k] : mx; k2++;
        }
        if (k2) {
            HIP_TRY(hipMemcpyAsync(segst[segcur].p, hs.data(), (size_t)k2 * 4, hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemcpyAsync(segsz[segcur].p, hz.data(), (size_t)k2 * 4, hipMemcpyHostToDevice, stream));
        }
        // the buckets' first places join the list of boundary LCPs (k_fix_window_lcp), like the left-over buckets' do
        uint32_t* d_taken = (uint32_t*)rg_misc.p + 8192;
        HIP_TRY(hipMemcpyAsync(d_taken, taken.data(), taken.size() * 4, hipMemcpyHostToDevice, stream));
        HIP_TRY(sync_reads());               // (host vectors)
        hipLaunchKernelGGL(k_append_starts, dim3(1), dim3(256), 0, stream, (const uint32_t*)d_taken, (uint32_t)ne, fo.fixlist, fo.nfix, fo.fixcap);
        hipLaunchKernelGGL(k_advance_fix, dim3(1), dim3(64), 0, stream, (uint32_t*)sc(SC_NFIX), (const unsigned long long*)nullptr, (uint32_t)ne);
        HIP_TRY(hipGetLastError());
        nseg = k2; m = m2; maxbig = mx;
        return 0;
    }

    // ---- re-keying levels -----------------------------------------------------------------------------
    // ---- sorting groups of (key, suffix) records where they lie (sufr_msd.inc: k_group_sort_*, k_large_*) ------------
    // The groups are the ranges [start[g], start[g] + size[g]) of the arrays, in order and without gaps; grp[t] = g.
    // prepare: windows of consecutive groups of <= GS_CAP records, the list of the groups above that, the groups above
    // gs_giant and their records (read back asynchronously into the plan: the caller synchronises the stream before run).
    struct GroupPlan { uint32_t wub = 0; unsigned long long large[2] = {0, 0}; };
    int group_sort_prepare(const uint32_t* d_starts, const uint32_t* d_sizes, uint32_t L, uint32_t m2, uint32_t maxsize,
                           GroupPlan& gp)
    {
        int rc;
        gp.wub = 0; gp.large[0] = gp.large[1] = 0;
        if (!group_sort) return 0;
        gs_giant = gs_giant_knob ? gs_giant_knob : (L >= 2048u ? (1u << 17) : (1u << 14));
        const uint32_t npseg = (L + GS_PS - 1) / GS_PS;
        const uint64_t cells = (uint64_t)npseg * GS_PS;
        gp.wub = (uint32_t)(2 * ((uint64_t)m2 / GS_CAP) + npseg + (uint64_t)m2 / (GS_CAP + 1) + 2);
        if ((rc = ensure(gs_leafbase, cells * 4))) return rc;
        if ((rc = ensure(gs_pst, (size_t)npseg * 4))) return rc;
        if ((rc = ensure(gs_psz, (size_t)npseg * 4))) return rc;
        if ((rc = ensure(gs_wcnt, (size_t)npseg * 4))) return rc;
        if ((rc = ensure(gs_wpre, (size_t)npseg * 4))) return rc;
        if ((rc = ensure(gs_wdesc, (size_t)gp.wub * 16))) return rc;
        if ((rc = ensure(gs_flag, cells * 4))) return rc;
        if ((rc = ensure(gs_off, cells * 4))) return rc;
        if ((rc = ensure(gs_big, ((size_t)m2 / GS_CAP + 2) * 4))) return rc;
        const size_t lcap = (size_t)m2 / gs_giant + 2;
        if ((rc = ensure(gs_lg, lcap * 4))) return rc;
        if ((rc = ensure(gs_lsz, lcap * 4))) return rc;
        if ((rc = ensure(gs_loff, lcap * 4))) return rc;
        HIP_TRY(zero_later(gs_flag.p, cells * 4));
        HIP_TRY(zero_later(sc(SC_TMP0), 16));                       // SC_TMP0: work queue, SC_TMP1: windows
        HIP_TRY(zero_later(sc(SC_GSLARGE), 16));
        HIP_TRY(zero_flush());
        hipLaunchKernelGGL(k_group_psegs, dim3((uint32_t)((cells + 255) / 256)), dim3(256), 0, stream, d_starts, L, m2, npseg,
                           (uint32_t*)gs_leafbase.p, (uint32_t*)gs_pst.p, (uint32_t*)gs_psz.p);
        if (maxsize > gs_giant) {
            hipLaunchKernelGGL(k_group_large, dim3((L + 255) / 256), dim3(256), 0, stream, d_sizes, L, gs_giant, sc(SC_GSLARGE),
                               (uint32_t*)gs_lg.p, (uint32_t*)gs_lsz.p);
            HIP_TRY(d2h_at(gp.large, sc(SC_GSLARGE), 16));
        }
        hipLaunchKernelGGL(k_pack_windows<false>, dim3((npseg + 3) / 4), dim3(256), 0, stream,
                           (const uint32_t*)gs_pst.p, (const uint32_t*)gs_psz.p, npseg, (const uint32_t*)gs_leafbase.p,
                           GS_PS, (uint32_t)GS_CAP, (uint32_t)GS_CAP, (uint32_t*)gs_wcnt.p, (const uint32_t*)nullptr,
                           (uint4*)nullptr, (uint32_t*)gs_flag.p);
        if ((rc = scan_u32((const uint32_t*)gs_wcnt.p, npseg, (uint32_t*)gs_wpre.p, sc(SC_TMP1)))) return rc;
        hipLaunchKernelGGL(k_pack_windows<true>, dim3((npseg + 3) / 4), dim3(256), 0, stream,
                           (const uint32_t*)gs_pst.p, (const uint32_t*)gs_psz.p, npseg, (const uint32_t*)gs_leafbase.p,
                           GS_PS, (uint32_t)GS_CAP, (uint32_t)GS_CAP, (uint32_t*)nullptr, (const uint32_t*)gs_wpre.p,
                           (uint4*)gs_wdesc.p, (uint32_t*)nullptr);
        if (maxsize > GS_CAP) {
            if ((rc = scan_u32((const uint32_t*)gs_flag.p, (uint32_t)cells, (uint32_t*)gs_off.p, sc(SC_GSBIG)))) return rc;
            hipLaunchKernelGGL(k_group_biglist, dim3((L + 255) / 256), dim3(256), 0, stream, (const uint32_t*)gs_flag.p,
                               (const uint32_t*)gs_off.p, L, (uint32_t*)gs_big.p);
        }
        HIP_TRY(hipGetLastError());
        return 0;
    }

    // run: records (k1, i1) -> sorted inside every group by key bits [64 - sort_bits, 64) in (k2, i2); grp is not moved.
    // done = false: nothing was sorted (switched off, or the level is mostly large groups -- the first one, made of whole
    // left-over buckets, is better off with the whole-level passes than with being copied out and back).
    // Windows of small groups in LDS, groups up to gs_giant records by one workgroup each; larger ones side by side in
    // the arrays of C (idle scratch of at least their size), sorted by whole-device passes on (group, key), brought back.
    int group_sort_run(const GroupPlan& gp, uint64_t* k1, uint32_t* i1, const uint32_t* s1, uint64_t* k2, uint32_t* i2,
                       const uint32_t* d_starts, const uint32_t* d_sizes, uint32_t L, uint32_t m2, uint32_t maxsize,
                       int sort_bits, LevelArrays& C, bool& done)
    {
        int rc;
        (void)L;
        done = group_sort && gp.large[1] * 2 <= m2;
        if (!done) return 0;
        const int lowbit = 64 - sort_bits;
        int NP = (sort_bits + 9) / 10; if (!(NP & 1)) NP++;   // an odd number of passes: A -> B
        const int Dg = (sort_bits + NP - 1) / NP;              // <= 10 bits
        {
            const size_t lds = (size_t)GS_CAP * 14 + 128 + 1024 + (size_t)(512 / 64) * 256 * 2;
            const uint32_t grid = gp.wub < 2048u ? gp.wub : 2048u;
            HIP_TRY(hipFuncSetAttribute((const void*)k_group_sort_small<512, 8>,
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL((k_group_sort_small<512, 8>), dim3(grid), dim3(512), lds, stream, (const uint64_t*)k1,
                               (const uint32_t*)i1, (const uint32_t*)s1, k2, i2, (const uint4*)gs_wdesc.p,
                               (const unsigned long long*)sc(SC_TMP1), lowbit);
        }
        if (maxsize > GS_CAP) {
            const size_t nbw = (size_t)1 << Dg;
            // (tiles of 2 048 records: 36 KB of LDS, four workgroups per CU -- a workgroup is a chain of dependent passes;
            // 4 096-record tiles, two per CU: +2.5 ms on the --dna build, A/B on one box)
            const size_t stage = (size_t)2048 * 12, wc = 4 * nbw * 2;
            const size_t lds = nbw * 12 + 128 + (stage > wc ? stage : wc);
            HIP_TRY(hipFuncSetAttribute((const void*)k_group_sort_big<256, 8>,
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL((k_group_sort_big<256, 8>), dim3(1024), dim3(256), lds, stream, k1, i1, k2, i2,
                               d_starts, d_sizes, (const uint32_t*)gs_big.p,
                               (const unsigned long long*)sc(SC_GSBIG), (unsigned int*)sc(SC_TMP0), lowbit, Dg, NP,
                               gs_giant);
        }
        if (gp.large[0]) {
            const uint32_t nl = (uint32_t)gp.large[0], ml = (uint32_t)gp.large[1];
            if ((rc = ensure(C.keyA, (size_t)ml * 8))) return rc;
            if ((rc = ensure(C.keyB, (size_t)ml * 8))) return rc;
            if ((rc = ensure(C.idxA, (size_t)ml * 4))) return rc;
            if ((rc = ensure(C.idxB, (size_t)ml * 4))) return rc;
            if ((rc = ensure(C.segA, (size_t)ml * 4))) return rc;
            if ((rc = ensure(C.segB, (size_t)ml * 4))) return rc;
            uint64_t* kc = (uint64_t*)C.keyA.p; uint32_t* ic = (uint32_t*)C.idxA.p; uint32_t* sc1 = (uint32_t*)C.segA.p;
            uint64_t* kd = (uint64_t*)C.keyB.p; uint32_t* id = (uint32_t*)C.idxB.p; uint32_t* sd = (uint32_t*)C.segB.p;
            if ((rc = scan_u32((const uint32_t*)gs_lsz.p, nl, (uint32_t*)gs_loff.p))) return rc;
            hipLaunchKernelGGL(k_large_gather, dim3((ml + 255) / 256), dim3(256), 0, stream, (const uint64_t*)k1,
                               (const uint32_t*)i1, d_starts, (const uint32_t*)gs_lg.p,
                               (const uint32_t*)gs_loff.p, nl, ml, kc, ic, sc1);
            const int D = deep_digit_bits;
            const int PD = (sort_bits + D - 1) / D;
            for (int p = 0; p < PD; p++) {
                const int lo = lowbit + p * D;
                const int width = (p == PD - 1) ? sort_bits - p * D : D;
                if ((rc = radix_pass_pairs(kc, ic, sc1, ml, 1u << width, 1u << width, nullptr, lo, false, kd, id, sd)))
                    return rc;
                std::swap(kc, kd); std::swap(ic, id); std::swap(sc1, sd);
            }
            const int qbits = ceil_log2_u64(nl);
            for (int dq = 0; dq < qbits;) {
                int nb = qbits - dq; if (nb > D) nb = D;
                if ((rc = radix_pass_pairs(kc, ic, sc1, ml, 1u << nb, 1u << nb, nullptr, dq, true, kd, id, sd)))
                    return rc;
                std::swap(kc, kd); std::swap(ic, id); std::swap(sc1, sd);
                dq += nb;
            }
            hipLaunchKernelGGL(k_large_return, dim3((ml + 255) / 256), dim3(256), 0, stream, (const uint64_t*)kc,
                               (const uint32_t*)ic, (const uint32_t*)sc1, d_starts,
                               (const uint32_t*)gs_lg.p, (const uint32_t*)gs_loff.p, ml, k2, i2);
        }
        HIP_TRY(hipGetLastError());
        return 0;
    }

    struct LevelState {
        const uint64_t* k; const uint32_t* i; const uint32_t* s; const uint32_t* o;   // sorted records of the level
        uint32_t m; bool deep; int sbits; uint32_t L;                                 // L large groups in *heads_cur
        DevBuf *heads_cur, *heads_nxt, *depth_cur, *depth_nxt; int which;            // which: lv[] set to build into
        // groups given as segments instead of being read off sorted keys (first level only): depth in characters
        const uint32_t* seg_start = nullptr; const uint32_t* seg_size = nullptr; uint32_t seg_depth = 0;
        const uint32_t* seg_depth_of = nullptr;      // per group, when the groups are of different depths
        uint32_t istride = 1;          // 3: `i` points at the index field of 12-byte records (first level only)
        bool allow_doubling = false;   // groups that stay tied may be handed to run_doubling
        uint32_t s_total = 0;          // suffixes of the build (size of SA / LCP)
        bool pos_keys = false;         // capped build (mql_fast): the groups are ordered by descending position, not by their text
    };

    int run_levels(LevelState z, const uint8_t* d_text, uint64_t n, const KeyParams& kp, uint32_t* d_sa,
                   uint32_t* d_lcp, sufr_hip_stats& st)
    {
        int rc;
        const uint64_t* lk = z.k; const uint32_t* li = z.i; const uint32_t* ls = z.s; const uint32_t* lo = z.o;
        uint32_t m = z.m; bool deep = z.deep; int sbits = z.sbits; uint32_t L = z.L;
        DevBuf* heads_cur = z.heads_cur; DevBuf* heads_nxt = z.heads_nxt;
        DevBuf* depth_cur = z.depth_cur; DevBuf* depth_nxt = z.depth_nxt;
        int which = z.which;
        uint32_t istride = z.istride;
        uint32_t m_prev = 0, stalled = 0;
        // A level sorts as many whole digits of its run keys as 64 bits hold (DNA: five 12-bit digits, 19 characters behind a
        // 2-bit token).  Round 2 sorted three (the 34 bits a token can take, so that every level advances) to save whole-level
        // passes; since the sort happens inside the groups (LDS) the extra digits cost little and every level sheds more
        // records: --dna on the 3.1 Gb stand-in 25 -> 17 levels, 1.83 -> 1.60 G records in levels, 382 -> 360 ms (A/B, one box).
        const int P2max = 64 / kp.dbits;
        const int P2min = p2min_knob > 0 ? (p2min_knob < P2max ? p2min_knob : P2max) : P2max;
        while (L > 0) {
            if (st.num_levels > n / (uint64_t)kp.dchars + 8) {
                set_error("internal error: re-keying levels did not converge");
                return SUFR_HIP_E_HIP;
            }
            st.num_levels++;
            st.num_large_groups += L;
            if ((rc = ensure(sizes, (size_t)L * 4))) return rc;
            if ((rc = ensure(starts, (size_t)L * 4))) return rc;
            if ((rc = ensure(*depth_nxt, (size_t)L * 4))) return rc;
            if ((rc = ensure(period, (size_t)L))) return rc;
            HIP_TRY(zero_later(sc(SC_MAXSIZE), 8));
            HIP_TRY(zero_later(sc(SC_MAXTOK), 8));
            HIP_TRY(zero_flush());
            if (z.seg_start && !deep && lk == z.k) {
                if ((rc = ensure(*heads_cur, ((size_t)L + 2) * 4))) return rc;
                hipLaunchKernelGGL(k_groups_from_segments, dim3((L + 255) / 256), dim3(256), 0, stream, z.seg_start,
                                   z.seg_size, L, z.seg_depth, li, istride, (const uint8_t*)d_text, kp.detect_period,
                                   (uint32_t*)heads_cur->p, (uint32_t*)sizes.p, (uint32_t*)depth_nxt->p,
                                   (uint8_t*)period.p, (uint32_t*)sc(SC_MAXSIZE), z.seg_depth_of);
            } else if (deep) {
                if ((rc = ensure(plancnt, (size_t)L * 4))) return rc;         // (idle between two finish_level calls) periodic groups
                hipLaunchKernelGGL(k_group_extent<true>, dim3((L + 255) / 256), dim3(256), 0, stream, lk, ls,
                                   (const uint32_t*)depth_cur->p, m, sbits, kp, (const uint32_t*)heads_cur->p, li,
                                   (const uint8_t*)d_text, L, (uint32_t*)sizes.p, (uint32_t*)depth_nxt->p,
                                   (uint8_t*)period.p, (uint32_t*)sc(SC_MAXSIZE), (uint32_t*)plancnt.p);
            }
            else
                hipLaunchKernelGGL(k_group_extent<false>, dim3((L + 255) / 256), dim3(256), 0, stream, lk, ls,
                                   (const uint32_t*)nullptr, m, sbits, kp, (const uint32_t*)heads_cur->p, li,
                                   (const uint8_t*)d_text, L, (uint32_t*)sizes.p, (uint32_t*)depth_nxt->p,
                                   (uint8_t*)period.p, (uint32_t*)sc(SC_MAXSIZE));
            if ((rc = scan_u32((const uint32_t*)sizes.p, L, (uint32_t*)starts.p))) return rc;
            unsigned long long two[2] = {0, 0};
            HIP_TRY(read_at_sync(two, sc(SC_MAXSIZE), 16));
            HIP_TRY(sync_reads());
            const uint32_t maxsize = (uint32_t)two[0];
            const uint32_t nperiodic = (uint32_t)(two[0] >> 32);      // (k_group_extent only)
            const uint32_t m2 = (uint32_t)two[1];
            st.deep_records += m2;
            if (debug) {
                std::vector<uint32_t> hs(L);
                HIP_TRY(hipMemcpy(hs.data(), sizes.p, (size_t)L * 4, hipMemcpyDeviceToHost));
                uint64_t rs = 0, rm = 0, rg = 0; uint32_t nm = 0, ng = 0;
                for (uint32_t v : hs) { if (v <= GS_CAP) rs += v; else if (v <= gs_giant) { rm += v; nm++; } else { rg += v; ng++; } }
                fprintf(stderr, "[sufr_hip debug] level %u: groups=%u records=%u max=%u  (<=%u: %llu records; mid: %u groups %llu records; "
                                "giant: %u groups %llu records)\n", st.num_levels, L, m2, maxsize, GS_CAP, (unsigned long long)rs, nm,
                        (unsigned long long)rm, ng, (unsigned long long)rg);
            }
            LevelArrays& A = lv[which];
            if ((rc = ensure(A.keyA, (size_t)m2 * 8))) return rc;
            if ((rc = ensure(A.keyB, (size_t)m2 * 8))) return rc;
            if ((rc = ensure(A.idxA, (size_t)m2 * 4))) return rc;
            if ((rc = ensure(A.idxB, (size_t)m2 * 4))) return rc;
            if ((rc = ensure(A.segA, (size_t)m2 * 4))) return rc;
            if ((rc = ensure(A.segB, (size_t)m2 * 4))) return rc;
            if ((rc = ensure(A.opos, (size_t)m2 * 4))) return rc;
            if ((rc = ensure(*heads_nxt, ((size_t)m2 / 64 + 2) * 4))) return rc;
            // The tie level hands over whole runs (no key bits sorted yet): their members are re-keyed at the depth their keys
            // were taken at.  The keys travel with the records instead of being read from the text again (a random sector per
            // record: 9.5 ms for the 278 M records of the --dna stand-in); only groups found periodic since take new ones.
            const bool carry_keys = deep && sbits == 0 && lk != nullptr && key_carry;
            if (deep)
                hipLaunchKernelGGL(k_build_level<true>, dim3((m2 + 255) / 256), dim3(256), 0, stream, li, istride, lo,
                                   (const uint32_t*)heads_cur->p, (const uint32_t*)starts.p, L, m2,
                                   (uint32_t*)A.idxA.p, (uint32_t*)A.segA.p, (uint32_t*)A.opos.p,
                                   carry_keys ? lk : (const uint64_t*)nullptr, carry_keys ? (uint64_t*)A.keyA.p : (uint64_t*)nullptr);
            else
                hipLaunchKernelGGL(k_build_level<false>, dim3((m2 + 255) / 256), dim3(256), 0, stream, li, istride, lo,
                                   (const uint32_t*)heads_cur->p, (const uint32_t*)starts.p, L, m2,
                                   (uint32_t*)A.idxA.p, (uint32_t*)A.segA.p, (uint32_t*)A.opos.p);
            // Levels that stop shrinking: ordinary repeats diverge, and every level sheds a good part of its records; a
            // level that keeps more than 3/4 of the records of the one before it, twice in a row, is made of copies of
            // something long (~20 characters per level will not do) -- prefix doubling takes it over.  (Setting it up
            // costs a pass over all suffixes: not worth it for levels that converge by themselves.)
            stalled = (m_prev && (uint64_t)m2 * 4 > (uint64_t)m_prev * 3) ? stalled + 1 : 0;
            m_prev = m2;
            if (z.allow_doubling && dbl_min_share && stalled >= 2 && m2 >= 4096u) {
                st.deep_records -= m2;                    // (counted again by the rounds)
                st.num_levels--;
                st.num_large_groups -= L;
                if (before_doubling && (rc = before_doubling())) return rc;     // (every rank outside this chain is final from here on)
                return run_doubling((const uint32_t*)A.idxA.p, (const uint32_t*)A.segA.p, (const uint32_t*)A.opos.p,
                                    (const uint32_t*)starts.p, (const uint32_t*)depth_nxt->p, L, m2, d_text, n, kp, d_sa,
                                    d_lcp, z.s_total, lv[which ^ 1], st);
            }
            if (z.pos_keys)
                hipLaunchKernelGGL(k_pos_keys, dim3((m2 + 255) / 256), dim3(256), 0, stream, (const uint32_t*)A.idxA.p, m2, (uint64_t*)A.keyA.p);
            else if (carry_keys) {
                if (nperiodic)
                    hipLaunchKernelGGL(k_gather_keys_listed, dim3(nperiodic, 64), dim3(256), 0, stream, (const uint8_t*)d_text, n, rtab,
                                       (const uint16_t*)lut.p, (const uint32_t*)A.idxA.p, (const uint32_t*)plancnt.p,
                                       (const uint32_t*)starts.p, (const uint32_t*)sizes.p, (const uint32_t*)depth_nxt->p,
                                       (const uint8_t*)period.p, kp, (uint64_t*)A.keyA.p);
            } else
            hipLaunchKernelGGL(k_gather_keys, dim3((m2 + 255) / 256), dim3(256), 0, stream,
                               (const uint8_t*)d_text, n, rtab, (const uint16_t*)lut.p,
                               (const uint32_t*)A.idxA.p, (const uint32_t*)A.segA.p,
                               (const uint32_t*)depth_nxt->p, (const uint8_t*)period.p, m2, kp,
                               (uint64_t*)A.keyA.p, (uint32_t*)sc(SC_MAXTOK));
            HIP_TRY(hipGetLastError());
            // the groups as windows / mid-size groups / large groups, for the sort below (read back with the same sync)
            GroupPlan gp;
            if ((rc = group_sort_prepare((const uint32_t*)starts.p, (const uint32_t*)sizes.p, L, m2, maxsize, gp))) return rc;
            unsigned long long maxtok = 0;
            HIP_TRY(read_at_sync(&maxtok, sc(SC_MAXTOK), 8));
            HIP_TRY(sync_reads());
            // passes on the key digits (lowest sorted digit first), then on the segment ordinal; every token
            // of the level lies inside the sorted bits (tokens above 34 bits: runs of 2^16 bytes and more)
            int P2 = P2min + (maxsize > 4096 ? 1 : 0) + (maxsize > (1u << 20) ? 1 : 0);
            const int Ptok = ((int)(uint32_t)maxtok + kp.dbits - 1) / kp.dbits;
            if (P2 < Ptok) P2 = Ptok;
            if (P2 > P2max) P2 = P2max;
            uint64_t* k1 = (uint64_t*)A.keyA.p; uint32_t* i1 = (uint32_t*)A.idxA.p; uint32_t* s1 = (uint32_t*)A.segA.p;
            uint64_t* k2 = (uint64_t*)A.keyB.p; uint32_t* i2 = (uint32_t*)A.idxB.p; uint32_t* s2 = (uint32_t*)A.segB.p;
            const int sort_bits = P2 * kp.dbits;                  // key bits this level sorts
            bool by_group = false;
            if ((rc = group_sort_run(gp, k1, i1, s1, k2, i2, (const uint32_t*)starts.p, (const uint32_t*)sizes.p, L, m2, maxsize,
                                     sort_bits, lv[which ^ 1] /* read for the last time by k_build_level above */, by_group)))
                return rc;
            if (by_group) {
                HIP_TRY(hipGetLastError());
                std::swap(k1, k2); std::swap(i1, i2);            // sorted keys / suffixes in B, the groups where they were
            } else {
            // run-key bits are not character aligned, so there is no dense remap here: with 12-bit digits a
            // 4096-record tile holds about one record per digit value and every store is a lone 8-byte write.
            // Narrower digits mean more passes over better-filled sectors; 10 bits measured best (12: +15-35 %).
            const int D = deep_digit_bits;
            const int PD = (sort_bits + D - 1) / D;
            for (int p = 0; p < PD; p++) {
                const int lo = 64 - sort_bits + p * D;              // lowest digit first; the top one may be narrower
                const int width = (p == PD - 1) ? sort_bits - p * D : D;
                if ((rc = radix_pass_pairs(k1, i1, s1, m2, 1u << width, 1u << width, nullptr, lo, false, k2, i2, s2)))
                    return rc;
                std::swap(k1, k2); std::swap(i1, i2); std::swap(s1, s2);
            }
            int segbits = ceil_log2_u64(L);
            for (int done = 0; done < segbits;) {
                int nb = segbits - done; if (nb > D) nb = D;
                if ((rc = radix_pass_pairs(k1, i1, s1, m2, 1u << nb, 1u << nb, nullptr, done, true, k2, i2, s2)))
                    return rc;
                std::swap(k1, k2); std::swap(i1, i2); std::swap(s1, s2);
                done += nb;
            }
            }
            const int sbits2 = P2 * kp.dbits;
            if ((rc = check_sorted("deep level", k1, s1, m2, 64 - sbits2))) return rc;
            if ((rc = finish_level(k1, i1, s1, (const uint32_t*)A.opos.p, (const uint32_t*)depth_nxt->p, m2, sbits2, d_text, n, kp,
                                   d_sa, d_lcp, heads_nxt, L))) return rc;
            lk = k1; li = i1; ls = s1; lo = (const uint32_t*)A.opos.p; m = m2; deep = true; sbits = sbits2; istride = 1;
            std::swap(heads_cur, heads_nxt);
            std::swap(depth_cur, depth_nxt);
            which ^= 1;
        }

        return 0;
    }

    // ---- prefix doubling over ranks (sufr_dbl.inc) for the groups of one level, to the end -----------------
    // lev_*: the level's records in slot order (suffix, group, rank slot), start / depth per group
    int run_doubling(const uint32_t* lev_idx, const uint32_t* lev_seg, const uint32_t* lev_opos, const uint32_t* lev_start,
                     const uint32_t* lev_depth, uint32_t L, uint32_t m0, const uint8_t* d_text, uint64_t n,
                     const KeyParams& kp, uint32_t* d_sa, uint32_t* d_lcp, uint32_t s, LevelArrays& D,
                     sufr_hip_stats& st)
    {
        const DblShard dsh = dbl_shard;
        int rc;
        dbl_entries++;
        const size_t rwords = (size_t)s / 32 + 2;
        const size_t pwords = (size_t)(n / 64) + 2;
        if ((rc = ensure(rankbuf, (size_t)n * 4 + 64))) return rc;
        if ((rc = ensure(dposbuf, (size_t)n * 4 + 64))) return rc;
        if ((rc = ensure(deferbuf, rwords * 4))) return rc;
        if ((rc = ensure(unresbuf, rwords * 4))) return rc;
        if ((rc = ensure(posbitsbuf, pwords * 8))) return rc;
        if ((rc = ensure(D.keyA, (size_t)m0 * 8))) return rc;
        if ((rc = ensure(D.keyB, (size_t)m0 * 8))) return rc;
        if ((rc = ensure(D.idxA, (size_t)m0 * 4))) return rc;
        if ((rc = ensure(D.idxB, (size_t)m0 * 4))) return rc;
        if ((rc = ensure(D.segA, (size_t)m0 * 4))) return rc;
        if ((rc = ensure(D.segB, (size_t)m0 * 4))) return rc;
        for (auto& b : dblf) if ((rc = ensure(b, ((size_t)m0 + 2) * 4))) return rc;
        const size_t gmax = (size_t)(L > m0 / 2 ? L : m0 / 2) + 2;
        for (auto& b : dblg) if ((rc = ensure(b, gmax * 4))) return rc;
        uint32_t* R = (uint32_t*)rankbuf.p; uint32_t* Dpos = (uint32_t*)dposbuf.p;
        uint32_t* defer = (uint32_t*)deferbuf.p; uint32_t* unres = (uint32_t*)unresbuf.p;
        uint32_t *flag = (uint32_t*)dblf[0].p, *ordx = (uint32_t*)dblf[1].p, *first = (uint32_t*)dblf[2].p,
                 *adv = (uint32_t*)dblf[3].p, *keep = (uint32_t*)dblf[4].p, *keepoff = (uint32_t*)dblf[5].p,
                 *newhead = (uint32_t*)dblf[6].p;
        uint32_t* ngoff = flag;                       // the flags are dead once `first` exists ... (kept apart below)
        uint32_t *hd = (uint32_t*)dblg[0].p, *dp = (uint32_t*)dblg[1].p, *gst = (uint32_t*)dblg[2].p;
        uint32_t *hd2 = (uint32_t*)dblg[3].p, *dp2 = (uint32_t*)dblg[4].p, *gst2 = (uint32_t*)dblg[5].p;
        HIP_TRY(hipMemsetAsync(Dpos, 0xff, (size_t)n * 4, stream));
        if (dsh.sharded) HIP_TRY(hipMemsetAsync(R, 0xff, (size_t)n * 4, stream));   // DBL_NORANK: positions whose suffix lives in another shard
        HIP_TRY(hipMemsetAsync(defer, 0, rwords * 4, stream));
        HIP_TRY(hipMemsetAsync(unres, 0, rwords * 4, stream));
        hipLaunchKernelGGL(k_dbl_enter, dim3((m0 + 255) / 256), dim3(256), 0, stream, lev_idx, lev_seg, lev_opos, lev_start,
                           lev_depth, m0, R, Dpos, unres, hd, dp, gst);
        hipLaunchKernelGGL(k_dbl_init_ranks, dim3((s + 255) / 256), dim3(256), 0, stream, (const uint32_t*)d_sa, s,
                           (const uint32_t*)unres, R);
        HIP_TRY(hipMemcpyAsync(D.idxA.p, lev_idx, (size_t)m0 * 4, hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipMemcpyAsync(D.segA.p, lev_seg, (size_t)m0 * 4, hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipGetLastError());
        uint64_t* k1 = (uint64_t*)D.keyA.p; uint32_t* i1 = (uint32_t*)D.idxA.p; uint32_t* g1 = (uint32_t*)D.segA.p;
        uint64_t* k2 = (uint64_t*)D.keyB.p; uint32_t* i2 = (uint32_t*)D.idxB.p; uint32_t* g2 = (uint32_t*)D.segB.p;
        uint32_t m = m0, ng = L;
        const int Dg = deep_digit_bits;
        for (uint32_t round = 0; m > 0; round++) {
            if (round > 96) { set_error("internal error: prefix doubling did not converge"); return SUFR_HIP_E_HIP; }
            st.num_levels++;
            st.num_large_groups += ng;
            st.deep_records += m;
            HIP_TRY(hipMemsetAsync(sc(SC_MAXTOK), 0, 8, stream));
            hipLaunchKernelGGL(k_dbl_keys, dim3((m + 255) / 256), dim3(256), 0, stream, d_text, n, rtab,
                               (const uint16_t*)lut.p, kp, (const uint32_t*)i1, (const uint32_t*)g1, (const uint32_t*)dp, m,
                               (const uint32_t*)R, k1, (uint32_t*)sc(SC_MAXTOK), dsh);
            unsigned long long any = 0;
            HIP_TRY(read_at_sync(&any, sc(SC_MAXTOK), 8));
            HIP_TRY(sync_reads());
            if (debug) fprintf(stderr, "[sufr_hip debug] doubling round %u: groups=%u records=%u%s\n", round, ng, m,
                               any ? " (run keys among them)" : "");
            // stable LSD passes: key digits (lowest sorted digit first), then the group ordinal
            const int sort_bits = any ? 64 : DBL_CODE_BITS + DBL_KIND_BITS + 32;
            const int PD = (sort_bits + Dg - 1) / Dg;
            for (int p = 0; p < PD; p++) {
                const int lo = 64 - sort_bits + p * Dg;
                const int width = (p == PD - 1) ? sort_bits - p * Dg : Dg;
                if ((rc = radix_pass_pairs(k1, i1, g1, m, 1u << width, 1u << width, nullptr, lo, false, k2, i2, g2))) return rc;
                std::swap(k1, k2); std::swap(i1, i2); std::swap(g1, g2);
            }
            const int gbits = ceil_log2_u64(ng);
            for (int done = 0; done < gbits;) {
                int nb = gbits - done; if (nb > Dg) nb = Dg;
                if ((rc = radix_pass_pairs(k1, i1, g1, m, 1u << nb, 1u << nb, nullptr, done, true, k2, i2, g2))) return rc;
                std::swap(k1, k2); std::swap(i1, i2); std::swap(g1, g2);
                done += nb;
            }
            hipLaunchKernelGGL(k_dbl_flags, dim3((m + 255) / 256), dim3(256), 0, stream, (const uint64_t*)k1,
                               (const uint32_t*)g1, (const uint32_t*)i1, (const uint32_t*)dp, m, d_text, n,
                               (const uint16_t*)lut.p, kp.b, (const uint32_t*)Dpos, flag, adv);
            if ((rc = scan_u32(flag, m, ordx))) return rc;
            hipLaunchKernelGGL(k_dbl_first, dim3((m + 256) / 256), dim3(256), 0, stream, (const uint32_t*)flag,
                               (const uint32_t*)ordx, m, first);
            hipLaunchKernelGGL(k_dbl_apply, dim3((m + 255) / 256), dim3(256), 0, stream, (const uint32_t*)i1,
                               (const uint32_t*)g1, (const uint32_t*)flag, (const uint32_t*)ordx, (const uint32_t*)first,
                               (const uint32_t*)adv, (const uint32_t*)hd, (const uint32_t*)dp, (const uint32_t*)gst, m, d_sa,
                               d_lcp, R, Dpos, defer, keep, newhead);
            unsigned long long mk = 0, mg = 0;
            if ((rc = scan_u32(keep, m, keepoff))) return rc;
            HIP_TRY(read_at_sync(&mk, sc(SC_SCANTOTAL), 8));
            HIP_TRY(sync_reads());
            if (mk) {
                // new group ordinals: exclusive scan of the heads (into `keep`'s place: keep is read before by the
                // compaction through keepoff differences?  no -- a buffer of its own)
                if ((rc = ensure(wloff, ((size_t)m + 2) * 4))) return rc;
                ngoff = (uint32_t*)wloff.p;
                if ((rc = scan_u32(newhead, m, ngoff))) return rc;
                HIP_TRY(read_at_sync(&mg, sc(SC_SCANTOTAL), 8));
                HIP_TRY(sync_reads());
                hipLaunchKernelGGL(k_dbl_compact, dim3((m + 255) / 256), dim3(256), 0, stream, (const uint32_t*)i1,
                                   (const uint32_t*)g1, (const uint32_t*)flag, (const uint32_t*)ordx, (const uint32_t*)first,
                                   (const uint32_t*)adv, (const uint32_t*)hd, (const uint32_t*)dp, (const uint32_t*)gst,
                                   (const uint32_t*)keep, (const uint32_t*)keepoff, (const uint32_t*)ngoff, m, i2, g2, hd2,
                                   dp2, gst2);
                std::swap(i1, i2); std::swap(g1, g2);
                std::swap(hd, hd2); std::swap(dp, dp2); std::swap(gst, gst2);
            }
            HIP_TRY(hipGetLastError());
            m = (uint32_t)mk; ng = (uint32_t)mg;
        }
        // the LCP entries the rounds left open, in text order
        HIP_TRY(hipMemsetAsync(posbitsbuf.p, 0, pwords * 8, stream));
        hipLaunchKernelGGL(k_dbl_posbits, dim3((s + 255) / 256), dim3(256), 0, stream, (const uint32_t*)defer,
                           (const uint32_t*)d_sa, s, (unsigned long long*)posbitsbuf.p);
        const uint64_t nwords = n / 64 + 1;
        hipLaunchKernelGGL(k_dbl_phi, dim3((uint32_t)((nwords + 255) / 256)), dim3(256), 0, stream, d_text, n,
                           (const uint16_t*)lut.p, (const unsigned long long*)posbitsbuf.p, nwords, (const uint32_t*)R,
                           (const uint32_t*)d_sa, d_lcp, (const uint32_t*)defer);
        HIP_TRY(hipGetLastError());
        return 0;
    }

    // ---- --max-query-len: cap the LCP, order runs of equal L-prefixes by descending position -------
    int apply_max_query_len(uint64_t Lq, uint64_t n, uint32_t* d_sa, uint32_t* d_lcp, uint32_t s)
    {
        if (Lq == 0 || Lq >= n || s < 2) return 0;      // no two suffixes share n characters
        const uint32_t L = (uint32_t)Lq;
        int rc;
        if ((rc = ensure(optA, (size_t)s * 4))) return rc;
        if ((rc = ensure(optB, (size_t)s * 4))) return rc;
        hipLaunchKernelGGL(k_mql_flags, dim3((s + 255) / 256), dim3(256), 0, stream, d_lcp, s, L, (uint32_t*)optA.p);
        if ((rc = scan_u32((const uint32_t*)optA.p, s, (uint32_t*)optB.p))) return rc;
        unsigned long long tot = 0;
        HIP_TRY(read_at_sync(&tot, sc(SC_SCANTOTAL), 8));
        HIP_TRY(sync_reads());
        const uint32_t M = (uint32_t)tot;
        if (debug) fprintf(stderr, "[sufr_hip debug] max_query_len=%u: %u of %u ranks in tie runs\n", L, M, s);
        if (!M) return 0;
        if ((rc = ensure(keyA, (size_t)M * 8))) return rc;
        if ((rc = ensure(keyB, (size_t)M * 8))) return rc;
        if ((rc = ensure(idxA, (size_t)M * 4))) return rc;
        if ((rc = ensure(idxB, (size_t)M * 4))) return rc;
        if ((rc = ensure(optC, (size_t)M * 4))) return rc;   // slot (rank) of every compacted record
        if ((rc = ensure(optD, (size_t)M * 4))) return rc;   // 1 = first record of its run
        if ((rc = ensure(optE, (size_t)M * 4))) return rc;   // run ordinal (exclusive scan of the heads)
        hipLaunchKernelGGL(k_mql_compact, dim3((s + 255) / 256), dim3(256), 0, stream, (const uint32_t*)d_sa,
                           (const uint32_t*)d_lcp, (const uint32_t*)optA.p, (const uint32_t*)optB.p, s, L,
                           (uint32_t*)idxA.p, (uint32_t*)optC.p, (uint32_t*)optD.p);
        if ((rc = scan_u32((const uint32_t*)optD.p, M, (uint32_t*)optE.p))) return rc;
        HIP_TRY(read_at_sync(&tot, sc(SC_SCANTOTAL), 8));
        HIP_TRY(sync_reads());
        const int pos_bits = ceil_log2_u64(n) < 1 ? 1 : ceil_log2_u64(n);
        const int run_bits = ceil_log2_u64(tot + 1) < 1 ? 1 : ceil_log2_u64(tot + 1);
        const uint32_t R = (uint32_t)tot;                           // runs
        uint64_t* kcur = (uint64_t*)keyA.p; uint32_t* icur = (uint32_t*)idxA.p;
        uint64_t* kalt = (uint64_t*)keyB.p; uint32_t* ialt = (uint32_t*)idxB.p;
        // every run sorted where it lies, by descending position (k_group_sort_*: a run of `-m 12` on 100 Mb holds six
        // suffixes; the whole-array passes on (run, position) moved 54 key bits through six passes for them)
        bool done = false;
        if (group_sort && R) {
            if ((rc = ensure(starts, (size_t)R * 4))) return rc;
            if ((rc = ensure(sizes, (size_t)R * 4))) return rc;
            HIP_TRY(hipMemsetAsync(sc(SC_MAXSIZE), 0, 8, stream));
            hipLaunchKernelGGL(k_mql_groups, dim3((M + 255) / 256), dim3(256), 0, stream, (const uint32_t*)idxA.p,
                               (const uint32_t*)optD.p, (uint32_t*)optE.p, M, pos_bits, (uint32_t)(n - 1), kcur,
                               (uint32_t*)starts.p);
            hipLaunchKernelGGL(k_sizes_from_starts, dim3((R + 255) / 256), dim3(256), 0, stream, (const uint32_t*)starts.p, R, M,
                               (uint32_t*)sizes.p, sc(SC_MAXSIZE));
            GroupPlan gp;
            if ((rc = group_sort_prepare((const uint32_t*)starts.p, (const uint32_t*)sizes.p, R, M, M /* not known yet */, gp)))
                return rc;
            unsigned long long maxrun = 0;
            HIP_TRY(read_at_sync(&maxrun, sc(SC_MAXSIZE), 8));
            HIP_TRY(sync_reads());
            if ((rc = group_sort_run(gp, kcur, icur, (const uint32_t*)optE.p, kalt, ialt, (const uint32_t*)starts.p,
                                     (const uint32_t*)sizes.p, R, M, (uint32_t)maxrun, pos_bits, lv[0], done)))
                return rc;
            if (done) std::swap(icur, ialt);
        }
        if (!done) {
            if (group_sort && R)        // (the runs are known already: optE holds them)
                hipLaunchKernelGGL(k_mql_keys, dim3((M + 255) / 256), dim3(256), 0, stream, (const uint32_t*)idxA.p,
                                   (const uint32_t*)optE.p, M, pos_bits, (uint32_t)(n - 1), kcur);
            else {
                hipLaunchKernelGGL(k_mql_groups, dim3((M + 255) / 256), dim3(256), 0, stream, (const uint32_t*)idxA.p,
                                   (const uint32_t*)optD.p, (uint32_t*)optE.p, M, pos_bits, (uint32_t)(n - 1), kalt,
                                   (uint32_t*)optB.p /* run starts: unused here (optB is dead, s >= M entries) */);
                hipLaunchKernelGGL(k_mql_keys, dim3((M + 255) / 256), dim3(256), 0, stream, (const uint32_t*)idxA.p,
                                   (const uint32_t*)optE.p, M, pos_bits, (uint32_t)(n - 1), kcur);
            }
            HIP_TRY(hipGetLastError());
            // uniformly distributed digits: 10 bits keep a few records per digit value and tile (see run_levels)
            for (int shift = 0; shift < pos_bits + run_bits; shift += 10) {
                if ((rc = radix_pass_pairs(kcur, icur, nullptr, M, 1024u, 1024u, nullptr, shift, false, kalt, ialt,
                                           nullptr))) return rc;
                std::swap(kcur, kalt); std::swap(icur, ialt);
            }
        }
        hipLaunchKernelGGL(k_scatter_slots, dim3((M + 255) / 256), dim3(256), 0, stream, (const uint32_t*)icur,
                           (const uint32_t*)optC.p, M, d_sa);
        HIP_TRY(hipGetLastError());
        return 0;
    }

    // ---- --seed-mask: LSD sort of the eligible positions on the care characters -----------------------
    // s: eligible suffixes of the whole text.  num_shards > 1: this shard's are those whose first key digit lies in its range
    // (MaskShard, sufr_kernels.hip): ranges of ~s / N suffixes from the exact digit counts, identical on every rank.
    int sort_masked(const uint8_t* d_text, uint64_t n, const KeyParams& kp, uint64_t s, uint32_t shard_index, uint32_t num_shards,
                    uint32_t* d_sa, uint32_t* d_lcp, uint64_t cap, uint64_t* num_suffixes_out, sufr_hip_stats& st,
                    sufr_hip_stats* st_out)
    {
        int rc;
        const uint32_t tiles = (uint32_t)((n + TILE - 1) / TILE);
        const uint32_t weight = (uint32_t)opt_mask_offsets.size();
        const uint32_t mspan = opt_mask_offsets.back() + 1u;      // symbols a masked comparison reaches over
        // digits of whole characters, at most 10 bits: there is no dense remap here, and the per-wave counters
        // of a 4096-value digit would leave room for one workgroup per CU only
        const int mch = mask_digit_bits / kp.b > 0 ? mask_digit_bits / kp.b : 1;
        const int mbits = mch * kp.b;
        if ((rc = ensure(optA, (size_t)tiles * 4))) return rc;
        if ((rc = ensure(optB, (size_t)tiles * 4))) return rc;
        if ((rc = ensure(optC, (size_t)weight * 4))) return rc;
        if ((rc = ensure(stitchoffs, (size_t)weight * 4))) return rc;
        HIP_TRY(hipMemcpyAsync(optC.p, opt_mask_offsets.data(), (size_t)weight * 4, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(stitchoffs.p, opt_mask_offsets.data(), (size_t)weight * 4, hipMemcpyHostToDevice, stream));
        stitch_weight = weight;
        HIP_TRY(hipEventRecord(ev[4], stream));
        MaskShard ms;
        ms.offs = (const uint32_t*)optC.p; ms.mch = (int)weight < mch ? (int)weight : mch; ms.b = kp.b; ms.lo = 0; ms.hi = 0;
        if (num_shards > 1) {
            if ((rc = ensure(optD, 1024 * 4))) return rc;
            HIP_TRY(hipMemsetAsync(optD.p, 0, 1024 * 4, stream));
            hipLaunchKernelGGL(k_mask_top_hist, dim3(tiles), dim3(256), 0, stream, d_text, n, (const uint16_t*)lut.p, ms,
                               (uint32_t*)optD.p);
            std::vector<uint32_t> tot(1024);
            HIP_TRY(read_at_sync(tot.data(), optD.p, 1024 * 4));
            HIP_TRY(sync_reads());
            tot.resize((size_t)1 << (ms.mch * kp.b));
            uint64_t all = 0, cnt_shard = 0;
            for (uint32_t v : tot) all += v;
            uint32_t lo = 0, hi = 0;
            choose_shard(tot, all, shard_index, num_shards, lo, hi, cnt_shard);
            st.top_lo = lo; st.top_hi = hi;
            if (hi <= lo) { s = 0; }
            else { ms.lo = lo; ms.hi = hi; s = 0; for (uint32_t d = lo; d < hi; d++) s += tot[d]; }
        }
        st.num_suffixes = s;
        if (num_suffixes_out) *num_suffixes_out = s;
        if (s == 0) { st.num_levels = 1; if (st_out) *st_out = st; return 0; }
        if ((rc = check_capacity(s, cap, d_sa, d_lcp))) return rc;
        const uint32_t m = (uint32_t)s;
        if ((rc = ensure(keyA, (size_t)m * 8))) return rc;
        if ((rc = ensure(keyB, (size_t)m * 8))) return rc;
        if ((rc = ensure(idxA, (size_t)m * 4))) return rc;
        if ((rc = ensure(idxB, (size_t)m * 4))) return rc;
        hipLaunchKernelGGL(k_elig_count, dim3(tiles), dim3(256), 0, stream, d_text, n, (const uint16_t*)lut.p,
                           (uint32_t*)optA.p, ms);
        if ((rc = scan_u32((const uint32_t*)optA.p, tiles, (uint32_t*)optB.p))) return rc;
        hipLaunchKernelGGL(k_elig_emit_desc, dim3(tiles), dim3(256), 0, stream, d_text, n, (const uint16_t*)lut.p,
                           (const uint32_t*)optB.p, m, (uint32_t*)idxA.p, ms);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev[5], stream));
        uint64_t* kcur = (uint64_t*)keyA.p; uint32_t* icur = (uint32_t*)idxA.p;
        uint64_t* kalt = (uint64_t*)keyB.p; uint32_t* ialt = (uint32_t*)idxB.p;
        const int Kc = (kp.K / mch) * mch;                       // care characters per 64-bit key: whole digits
        const int rounds = ((int)weight + Kc - 1) / Kc;
        uint32_t passes = 0;
        for (int r = rounds - 1; r >= 0; r--) {
            const int c0 = r * Kc;
            const int cnt = (int)weight - c0 < Kc ? (int)weight - c0 : Kc;
            // (the care symbols picked out of registers instead of LDS rows -- a scalar choice of the word and a shift per symbol --
            // measured 28.5 against 24.6 ms on the hu-mask build: the select chains cost more than the conflicts they avoid)
            if (mspan <= (uint32_t)MASK_SPAN_MAX && cnt <= 64)
                hipLaunchKernelGGL(k_mask_keys_staged, dim3((m + 255) / 256), dim3(256), (size_t)256 * ((mspan + 7u) / 8u * 8u),
                                   stream, d_text, n, (const uint16_t*)lut.p, (const uint32_t*)icur, m,
                                   (const uint32_t*)optC.p + c0, cnt, kp.b, mspan, kcur);
            else
            hipLaunchKernelGGL(k_mask_keys, dim3((m + 255) / 256), dim3(256), 0, stream, d_text, n,
                               (const uint16_t*)lut.p, (const uint32_t*)icur, m, (const uint32_t*)optC.p + c0, cnt,
                               kp.b, kcur);
            HIP_TRY(hipGetLastError());
            const int ndig = (cnt + mch - 1) / mch;
            for (int d = ndig - 1; d >= 0; d--) {
                if ((rc = radix_pass_pairs(kcur, icur, nullptr, m, 1u << mbits, 1u << mbits, nullptr,
                                           64 - (d + 1) * mbits, false, kalt, ialt, nullptr))) return rc;
                std::swap(kcur, kalt); std::swap(icur, ialt);
                passes++;
            }
        }
        HIP_TRY(hipEventRecord(ev[6], stream));
        HIP_TRY(hipMemcpyAsync(d_sa, icur, (size_t)m * 4, hipMemcpyDeviceToDevice, stream));
        const uint32_t span = mspan;
        if (mask_lcp_from_keys && passes > 0)                      // (kcur: the sorted keys of the last round = the first care symbols)
            hipLaunchKernelGGL(k_mask_lcp_keys, dim3((m + 255) / 256), dim3(256), 0, stream, d_text, n, (const uint64_t*)kcur,
                               (const uint32_t*)d_sa, m, (const uint32_t*)optC.p, weight, (uint32_t)((int)weight < Kc ? (int)weight : Kc),
                               kp.b, span, d_lcp);
        else if (span <= (uint32_t)MASK_SPAN_MAX)                  // (the device text is the padded workspace copy)
            hipLaunchKernelGGL(k_mask_lcp_staged, dim3((m + 255) / 256), dim3(256), (size_t)257 * ((span + 7u) / 8u * 8u), stream,
                               d_text, n, (const uint32_t*)d_sa, m, (const uint32_t*)optC.p, weight, span, d_lcp);
        else
            hipLaunchKernelGGL(k_mask_lcp, dim3((m + 255) / 256), dim3(256), 0, stream, d_text, n, (const uint32_t*)d_sa,
                               m, (const uint32_t*)optC.p, weight, d_lcp);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev[7], stream));
        HIP_TRY(sync_reads());
        st.num_passes = passes; st.num_levels = 1;
        (void)hipEventElapsedTime(&st.ms_total, ev[0], ev[7]);
        (void)hipEventElapsedTime(&st.ms_normalize, ev[0], ev[1]);
        (void)hipEventElapsedTime(&st.ms_partition, ev[4], ev[5]);
        (void)hipEventElapsedTime(&st.ms_passes, ev[5], ev[6]);
        (void)hipEventElapsedTime(&st.ms_finish, ev[6], ev[7]);
        if (st_out) *st_out = st;
        return 0;
    }

    // ---- dense digit numbering of a level (DigitMap) from the presence flags of its raw digit values ----
    // present_vals (optional): raw value of every dense digit, ascending
    int upload_digit_map(const std::vector<uint32_t>& flags, int dbits, DevBuf& buf, std::vector<uint8_t>& host,
                         DigitMap& dm, std::vector<uint32_t>* present_vals)
    {
        const uint32_t raw_bins = 1u << dbits;
        const uint32_t rows = raw_bins >= 64u ? raw_bins / 64u : 1u;
        host.assign((size_t)rows * 10, 0);
        uint64_t* pres = reinterpret_cast<uint64_t*>(host.data());
        uint16_t* rb = reinterpret_cast<uint16_t*>(host.data() + (size_t)rows * 8);
        uint32_t dense = 0;
        if (present_vals) present_vals->clear();
        for (uint32_t r = 0; r < rows; r++) {
            rb[r] = (uint16_t)dense;
            for (uint32_t i = 0; i < 64u; i++) {
                const uint32_t v = r * 64u + i;
                if (v < raw_bins && flags[v]) {
                    pres[r] |= 1ull << i;
                    dense++;
                    if (present_vals) present_vals->push_back(v);
                }
            }
        }
        int rc;
        if ((rc = ensure(buf, host.size()))) return rc;
        HIP_TRY(hipMemcpyAsync(buf.p, host.data(), host.size(), hipMemcpyHostToDevice, stream));
        dm.pres = (const uint64_t*)buf.p;
        dm.rowbase = (const uint16_t*)((const uint8_t*)buf.p + (size_t)rows * 8);
        dm.rows = rows; dm.raw_mask = raw_bins - 1u; dm.nbins = dense; dm.dbits = dbits;
        return 0;
    }

    // the same map from presence WORDS (bit v & 63 of word v >> 6: the layout of DigitMap::pres itself)
    int upload_digit_map_words(const std::vector<uint64_t>& words, int dbits, DevBuf& buf, std::vector<uint8_t>& host,
                               DigitMap& dm, std::vector<uint32_t>& present_vals)
    {
        const uint32_t raw_bins = 1u << dbits;
        const uint32_t rows = raw_bins / 64u;
        if (raw_bins < 64u || words.size() != rows) { set_error("internal error: presence words do not fit the digit"); return SUFR_HIP_E_HIP; }
        host.assign((size_t)rows * 10, 0);
        uint64_t* pres = reinterpret_cast<uint64_t*>(host.data());
        uint16_t* rb = reinterpret_cast<uint16_t*>(host.data() + (size_t)rows * 8);
        uint32_t dense = 0;
        present_vals.clear();
        for (uint32_t r = 0; r < rows; r++) {
            uint64_t w = words[r];
            rb[r] = (uint16_t)dense;
            pres[r] = w;
            dense += (uint32_t)__builtin_popcountll(w);
            for (; w; w &= w - 1) present_vals.push_back(r * 64u + (uint32_t)__builtin_ctzll(w));
        }
        int rc;
        if ((rc = ensure(buf, host.size()))) return rc;
        HIP_TRY(hipMemcpyAsync(buf.p, host.data(), host.size(), hipMemcpyHostToDevice, stream));
        dm.pres = (const uint64_t*)buf.p;
        dm.rowbase = (const uint16_t*)((const uint8_t*)buf.p + (size_t)rows * 8);
        dm.rows = rows; dm.raw_mask = raw_bins - 1u; dm.nbins = dense; dm.dbits = dbits;
        return 0;
    }

    // every value of a w-bit digit numbered as it is (levels whose segment list is too long for the dense table)
    int identity_digit_map(int w, DigitMap& dm)
    {
        std::vector<uint32_t> all(1u << w, 1u);
        return upload_digit_map(all, w, identbuf[w], identhost[w], dm, nullptr);
    }

    static constexpr uint64_t SHARD_MIN_MQL = 8;             // smallest --max-query-len a sharded build takes (a first digit holds <= 7 symbols)
    static constexpr size_t PART_LDS_MAX = 160u * 1024u;     // LDS of a CU (one partition workgroup per CU)
    static size_t msd_map_bytes_host(uint32_t rows) { return (size_t)rows * 8 + (((size_t)rows * 2 + 15) & ~(size_t)15); }

    // ---- the leaf sort of one level + the list of buckets that need another level ---------------------
    // segments (seg_cur: start / size) hold `m` records in all; their sub-buckets start at leafbase[k * NB + d].
    // Windows of small buckets are sorted and finished (SA, LCP, tie bitmaps: `fo`; kdst takes their boundary
    // keys); flagged buckets become seg_nxt.  nbig / mbig: their number and records (read back: the caller
    // decides on the next level).
    int leaf_stage(const Rec* rsrc, Rec* rdst, uint32_t nseg, uint64_t m, const DigitMap& dm, const CharModel& cc,
                   const FinishOut& fo, int hibit, uint32_t& nbig, uint64_t& mbig, uint64_t& maxbig)
    {
        int rc;
        const uint32_t NB = dm.nbins;
        // windows: consecutive windows of an uninterrupted stretch of leaves hold more than CAP records together;
        // segments and big leaves (more than BIG records each) interrupt
        const uint64_t wub64 = 2 * (m / LEAF_CAP) + nseg + m / ((uint64_t)LEAF_BIG + 1) + 2;
        const uint64_t cells = (uint64_t)nseg * NB;
        if (wub64 >= (1ull << 31) || cells >= (1ull << 31)) { set_error("internal error: segment table too large"); return SUFR_HIP_E_HIP; }
        const uint32_t wub = (uint32_t)wub64;
        if ((rc = ensure(wunits, (size_t)nseg * 4))) return rc;
        if ((rc = ensure(wpre, (size_t)nseg * 4))) return rc;
        if ((rc = ensure(wdesc, (size_t)wub * 16))) return rc;
        if ((rc = ensure(bigflag, cells * 4))) return rc;
        if ((rc = ensure(bigoff, cells * 4))) return rc;
        if ((rc = ensure(wslow, (size_t)wub * 4))) return rc;
        HIP_TRY(zero_later(bigflag.p, cells * 4));
        HIP_TRY(zero_later(sc(SC_MBIG), 16));               // SC_MBIG, SC_MAXBIG
        HIP_TRY(zero_later(wslow.p, (size_t)wub * 4));
        HIP_TRY(zero_flush());
        hipLaunchKernelGGL(k_pack_windows<false>, dim3((nseg + 3) / 4), dim3(256), 0, stream,
                           (const uint32_t*)segst[segcur].p, (const uint32_t*)segsz[segcur].p, nseg,
                           (const uint32_t*)leafbase.p, NB, (uint32_t)LEAF_CAP, (uint32_t)LEAF_BIG, (uint32_t*)wunits.p,
                           (const uint32_t*)nullptr, (uint4*)nullptr, (uint32_t*)bigflag.p);
        if ((rc = scan_u32((const uint32_t*)wunits.p, nseg, (uint32_t*)wpre.p, sc(SC_WTOTAL)))) return rc;
        hipLaunchKernelGGL(k_pack_windows<true>, dim3((nseg + 3) / 4), dim3(256), 0, stream,
                           (const uint32_t*)segst[segcur].p, (const uint32_t*)segsz[segcur].p, nseg,
                           (const uint32_t*)leafbase.p, NB, (uint32_t)LEAF_CAP, (uint32_t)LEAF_BIG, (uint32_t*)nullptr,
                           (const uint32_t*)wpre.p, (uint4*)wdesc.p, (uint32_t*)nullptr);
        if ((rc = scan_u32((const uint32_t*)bigflag.p, (uint32_t)cells, (uint32_t*)bigoff.p, sc(SC_NBIG)))) return rc;
        const uint64_t bigcap = m / (LEAF_BIG + 1) + 1;            // every flagged bucket holds more than LEAF_BIG records
        if ((rc = ensure(segst[segcur ^ 1], bigcap * 4))) return rc;
        if ((rc = ensure(segsz[segcur ^ 1], bigcap * 4))) return rc;
        hipLaunchKernelGGL(k_compact_big, dim3((uint32_t)((cells + 255) / 256)), dim3(256), 0, stream,
                           (const uint32_t*)bigflag.p, (const uint32_t*)bigoff.p, (const uint32_t*)leafbase.p,
                           (const uint32_t*)segst[segcur].p, (const uint32_t*)segsz[segcur].p, nseg, NB,
                           (uint32_t*)segst[segcur ^ 1].p, (uint32_t*)segsz[segcur ^ 1].p, sc(SC_MBIG));
        unsigned long long two[3] = {0, 0, 0};
        {
            const uint32_t gmax = leaf_nt == 1024 ? 1024u : 2048u;
            const uint32_t grid = wub < gmax ? wub : gmax;       // workgroups loop over the windows
            const size_t lds = (size_t)LEAF_CAP * 12 + (size_t)LEAF_KEY_PAD * 8 + msd_map_bytes_host(dm.rows) +
                               (leaf_dna3 ? (size_t)DNA3_HALF_ENTRIES * 2 : (size_t)LEAF_CS_MAX * 8) +
                               128 + ((size_t)1 << leaf_t1) * 4;
#define SUFR_LEAF(NT_, T1_, D3_)                                                                                         \
            {                                                                                                            \
                HIP_TRY(hipFuncSetAttribute((const void*)k_leaf_sort<NT_, LEAF_E, T1_, D3_>,                            \
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                     \
                hipLaunchKernelGGL((k_leaf_sort<NT_, LEAF_E, T1_, D3_>), dim3(grid), dim3(NT_), lds, stream, rsrc,      \
                                   rdst, (const uint4*)wdesc.p, (const unsigned long long*)sc(SC_WTOTAL),              \
                                   (uint32_t*)wslow.p, hibit, dm, cc, fo, leaf_bmax);                                   \
            }
#define SUFR_LEAF_D(NT_, T1_) { if (leaf_dna3) SUFR_LEAF(NT_, T1_, true) else SUFR_LEAF(NT_, T1_, false) }
            if (leaf_nt == 1024) { if (leaf_t1 == 13) SUFR_LEAF_D(1024, 13) else SUFR_LEAF_D(1024, 12) }
            else { if (leaf_t1 == 11) SUFR_LEAF_D(512, 11) else SUFR_LEAF_D(512, 12) }
#undef SUFR_LEAF_D
#undef SUFR_LEAF
            const size_t lds2 = (size_t)LEAF_CAP * 12 + msd_map_bytes_host(dm.rows) + 128 + 256 * 4 +
                                (size_t)(leaf_nt / 64) * 256 * 2;
#define SUFR_LEAF_LSD(NT_)                                                                                               \
            {                                                                                                            \
                HIP_TRY(hipFuncSetAttribute((const void*)k_leaf_sort_lsd<NT_, LEAF_E>,                                  \
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));                    \
                hipLaunchKernelGGL((k_leaf_sort_lsd<NT_, LEAF_E>), dim3(grid), dim3(NT_), lds2, stream, rsrc, rdst,     \
                                   (const uint4*)wdesc.p, (const unsigned long long*)sc(SC_WTOTAL),                    \
                                   (const uint32_t*)wslow.p, hibit, cc.lastbit, dm, fo);                               \
            }
            if (leaf_nt == 1024) SUFR_LEAF_LSD(1024) else SUFR_LEAF_LSD(512)
#undef SUFR_LEAF_LSD
            // the fix list grows by this level's windows
            hipLaunchKernelGGL(k_advance_fix, dim3(1), dim3(64), 0, stream, (uint32_t*)sc(SC_NFIX),
                               (const unsigned long long*)sc(SC_WTOTAL), 0u);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(read_at_sync(two, sc(SC_NBIG), 24));                  // (the leaf kernels leave these three alone)
        HIP_TRY(sync_reads());
        nbig = (uint32_t)two[0];
        mbig = two[1];
        maxbig = two[2];
        return 0;
    }

    // tile list of the current segments (k_msd_tiles): G groups, `unit` records per tile
    int plan_tiles(uint32_t nseg, uint64_t m, uint32_t G, uint32_t unit, uint32_t& SG, uint32_t& tub)
    {
        int rc;
        SG = (nseg + G - 1) / G;
        const uint32_t slots = G * SG;
        tub = (uint32_t)(m / unit + nseg);
        if ((rc = ensure(tunits, (size_t)slots * 4))) return rc;
        if ((rc = ensure(upre, (size_t)slots * 4))) return rc;
        if ((rc = ensure(tdesc, (size_t)tub * 16))) return rc;
        hipLaunchKernelGGL(k_seg_units, dim3((slots + 255) / 256), dim3(256), 0, stream, (const uint32_t*)segsz[segcur].p,
                           nseg, G, SG, unit, (uint32_t*)tunits.p);
        if ((rc = scan_u32((const uint32_t*)tunits.p, slots, (uint32_t*)upre.p, sc(SC_UTOTAL)))) return rc;
        hipLaunchKernelGGL(k_msd_tiles, dim3((tub + 255) / 256), dim3(256), 0, stream, (const uint32_t*)segst[segcur].p,
                           (const uint32_t*)segsz[segcur].p, G, SG, unit, (const uint32_t*)upre.p,
                           (const unsigned long long*)sc(SC_UTOTAL), (uint4*)tdesc.p);
        HIP_TRY(hipGetLastError());
        return 0;
    }

    // ---- the build ------------------------------------------------------------------------------
    // Every way out of a build that listed bytes outside the DNA table -- an empty build, outputs that are too small, an
    // allocation that fails -- hands out the caller's text: what exc_reinsert has not put back yet is put back here (the helper
    // chain, which reads the text, has been joined by then).
    int sort_device_u32(const void* d_in, uint64_t n, uint32_t flags, uint32_t shard_index,
                        uint32_t num_shards, uint32_t* d_sa, uint32_t* d_lcp, uint64_t cap,
                        uint64_t* num_suffixes_out, sufr_hip_stats* st_out)
    {
        last_overlapped = 0; last_doublings = 0; dbl_entries = 0; last_pairs_resolved = 0; last_pairs_left = 0;
        if (helper) helper->dbl_entries = 0;
        if (!exc_disable) { last_exc_retry = 0; last_exc_taken = 0; }          // (the retry of a build keeps what that build recorded)
        const int rc = sort_build(d_in, n, flags, shard_index, num_shards, d_sa, d_lcp, cap, num_suffixes_out, st_out);
        before_doubling = nullptr;
        last_doublings = dbl_entries + (helper ? helper->dbl_entries : 0);       // (both chains: the helper has been joined)
        if (exc_pending) {
            const uint32_t E = exc_pending;
            exc_pending = 0;
            hipLaunchKernelGGL(k_exc_restore, dim3((E + 255) / 256), dim3(256), 0, stream, (uint8_t*)text.p,
                               (const uint32_t*)exc_pos.p, (const uint8_t*)exc_byte.p, E);
            if ((hipGetLastError() != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) && !rc) {
                set_error("putting the listed bytes back into the text failed");
                return SUFR_HIP_E_HIP;
            }
        }
        return rc;
    }

    // ---- the state of ONE plain-order build: lives on sort_build's stack and goes to its stages by reference.  A member is set
    // by the stage named above it and read by the stages after it.  Four are touched again, each in one place: kp (cut to the
    // digit by first_digit_map), d_sa / d_lcp (the caller's again once reinsert_listed has written them, in sort_build),
    // mql_count (m0 in sort_build, the final count in reinsert_listed).
    struct Build {
        // check_call: the call
        const void* d_in_caller = nullptr;                 // the caller's text as it was handed in
        uint64_t n = 0, cap = 0;
        uint32_t flags = 0, shard_index = 0, num_shards = 1;
        bool is_dna = false, allow_amb = false, raw = false, softmask = false, masked = false;
        uint32_t* caller_sa = nullptr; uint32_t* caller_lcp = nullptr;
        uint64_t* num_suffixes_out = nullptr;
        sufr_hip_stats* st_out = nullptr;
        sufr_hip_stats st;                                 // filled stage by stage; handed out by done()
        // open_text
        uint8_t* d_text = nullptr;                         // the normalised text (Pipeline::text)
        const void* d_in = nullptr;                        // what the text stage STARTS from: the caller's text, or its 16-byte aligned copy
        // plan_text_chunks: workgroup w of the streaming kernels takes chunk w (tchunk positions), group w % G1
        uint32_t ngrid = 0, G1 = 0;                        // (ngrid: the grid of k_normalize_bytehist)
        uint64_t nwg_t = 0, tchunk = 0;
        bool small_tiles = false;                          // 16384-position tiles of k_msd_part_text (256 threads), not 65536
        // text_stage
        bool dna_table = false;                            // the fixed 3-bit table {$ % A C G N T}; the packed stream is written
        uint32_t nexc = 0;                                 // listed bytes outside the table (the build then runs on 'N' in their place)
        unsigned long long hist[256];
        std::vector<uint64_t> pwords;                      // which raw first digits occur: a bit each (DNA text pass), or
        std::vector<uint32_t> pflags;                      // a flag each (first_digit_map: the presence pass, or fewer characters)
        // code_table
        KeyParams kp;
        uint64_t eligible_total = 0;
        // first_digit_map
        bool packed_path = false, mql_fast = false;
        int mql_charbits = 0, mbits = 0;                   // bits of the L characters of a capped key; of the first digit (D = mbits / kp.b)
        DigitMap dm;
        std::vector<uint32_t> present_vals;                // raw value of every dense first digit
        uint32_t NB = 0;
        const uint16_t* d_remap = nullptr;
        // char_model
        CharModel cc;
        // count_and_shard: this shard's first digits, raw [raw_lo, raw_hi) = dense [bin_lo, bin_hi) (all of them, then the shard's), its suffixes
        uint32_t raw_lo = 0, raw_hi = 0, bin_lo = 0, bin_hi = 0;
        uint64_t s = 0;
        // working_arrays: d_sa / d_lcp = the caller's, or the exception build's (exc_reinsert then writes the caller's)
        uint32_t m0 = 0;
        uint32_t* d_sa = nullptr; uint32_t* d_lcp = nullptr;
        Rec* xr[2] = {nullptr, nullptr};                   // records ping-pong between the levels; the sorted ones end up in [1]
        // msd_levels
        uint32_t nwin = 0, wcnt_stride = 0, fixcap = 0;    // 128-position windows of the tie bitmaps, a row of their counts, the fix list
        FinishOut fo;
        // reinsert_listed (else: m0)
        uint32_t mql_count = 0;                            // suffixes of the finished arrays
    };
    struct LeftOver { uint32_t groups = 0; uint64_t records = 0; uint32_t depth = 0; uint64_t maxbig = 0; };   // buckets whose members agree on every key character
    // the chain of the left-over buckets when it runs on the helper pipeline: joined after the tie runs, before prefix doubling
    // (before_doubling), and on every way out of sort_build
    struct LeftChain { std::thread th; int rc = 0; sufr_hip_stats st = {}; ~LeftChain() { if (th.joinable()) th.join(); } };

    int done(Build& B) { if (B.st_out) *B.st_out = B.st; return 0; }
    int check_capacity(uint64_t s, uint64_t cap, const uint32_t* d_sa, const uint32_t* d_lcp)
    {
        if (s > cap || !d_sa || !d_lcp) {
            set_error("output capacity " + std::to_string(cap) + " < num_suffixes " + std::to_string(s));
            return SUFR_HIP_E_CAPACITY;
        }
        return 0;
    }

    int sort_build(const void* d_in, uint64_t n, uint32_t flags, uint32_t shard_index,
                   uint32_t num_shards, uint32_t* d_sa, uint32_t* d_lcp, uint64_t cap,
                   uint64_t* num_suffixes_out, sufr_hip_stats* st_out)
    {
        Build B;
        LeftChain chain;                                       // (after B: joined before B goes)
        int rc;
        if ((rc = check_call(B, d_in, n, flags, shard_index, num_shards, d_sa, d_lcp, cap, num_suffixes_out, st_out))) return rc;
        if (n == 0) return done(B);
        if ((rc = open_text(B))) return rc;
        if ((rc = plan_text_chunks(B))) return rc;
        if ((rc = text_stage(B))) return rc;
        if ((rc = code_table(B))) return rc;
        if (B.eligible_total == 0) return done(B);
        if (B.masked) {
            if (num_suffixes_out) *num_suffixes_out = B.eligible_total;
            return sort_masked(B.d_text, n, B.kp, B.eligible_total, shard_index, num_shards, d_sa, d_lcp, cap, num_suffixes_out, B.st, st_out);
        }
        if ((rc = first_digit_map(B))) return rc;
        if ((rc = char_model(B))) return rc;
        if ((rc = count_and_shard(B))) return rc;
        if (B.s == 0) return empty_shard(B);
        if ((rc = check_capacity(B.s, cap, d_sa, d_lcp))) return rc;
        if ((rc = working_arrays(B))) return rc;
        if ((rc = launch_partition(B))) return rc;
        LeftOver left;
        if ((rc = msd_levels(B, left))) return rc;
        if ((rc = start_left_chain(B, left, chain))) return rc;
        if ((rc = tie_level(B, chain))) return rc;
        if ((rc = join_left_chain(B, chain))) return rc;
        B.mql_count = B.m0;
        if (B.mql_fast) {                                      // (before the listed bytes are dealt with: their pass compares under the cap)
            hipLaunchKernelGGL(k_mql_cap, dim3((B.m0 / 4 + 256) / 256), dim3(256), 0, stream, B.d_lcp, B.m0, (uint32_t)opt_max_query_len);
            HIP_TRY(hipGetLastError());
        }
        if (B.nexc) {
            bool rebuilt = false;
            rc = reinsert_listed(B, B.d_sa, B.d_lcp, B.m0, rebuilt);
            if (rc || rebuilt) return rc;
            B.d_sa = B.caller_sa; B.d_lcp = B.caller_lcp;
        }
        if (!B.mql_fast && opt_max_query_len > 0 && (rc = apply_max_query_len(opt_max_query_len, n, B.d_sa, B.d_lcp, B.mql_count))) return rc;
        HIP_TRY(hipEventRecord(ev[8], stream));
        HIP_TRY(sync_reads());
        HIP_TRY(hipGetLastError());
        return finish_stats(B);
    }

    int check_call(Build& B, const void* d_in, uint64_t n, uint32_t flags, uint32_t shard_index, uint32_t num_shards,
                   uint32_t* d_sa, uint32_t* d_lcp, uint64_t cap, uint64_t* num_suffixes_out, sufr_hip_stats* st_out)
    {
        memset(&B.st, 0, sizeof B.st);
        B.st.text_len = n;
        B.st_out = st_out;
        reset_reads();                                     // (reads a failed build queued: their destinations are gone)
        if (num_suffixes_out) *num_suffixes_out = 0;
        if (num_shards == 0 || shard_index >= num_shards) { set_error("bad shard index"); return SUFR_HIP_E_INVALID; }
        // 32-bit record indices with tile-sized strides: keep a margin below 2^32 so that no loop counter wraps
        if (n >= SUFR_MAX_TEXT_LEN) {
            set_error("text_len >= 2^32 - 2^24 does not fit one 32-bit window (sufr_wide.inc builds such texts in windows)");
            return SUFR_HIP_E_UNSUPPORTED;
        }
        read_env();
        B.masked = !opt_mask_offsets.empty();
        // Shards of the other two orders (find_lcp's other arms, 272-314: "a bounded key, then descending position"): a seed-mask
        // build is split on its own first key digit (sort_masked); a --max-query-len build on the first digit of the plain
        // order, which ties no two suffixes across a shard as long as the cap is at least a digit long (<= 7 symbols)
        if (num_shards > 1 && !B.masked && opt_max_query_len > 0 && opt_max_query_len < SHARD_MIN_MQL) {
            set_error("a max_query_len below " + std::to_string(SHARD_MIN_MQL) + " ties suffixes across first-digit shards: build it on one GPU");
            return SUFR_HIP_E_UNSUPPORTED;
        }
        stitch_weight = 0;
        stitch_cap = (!B.masked && opt_max_query_len > 0) ? opt_max_query_len : 0;
        B.d_in_caller = d_in; B.n = n; B.flags = flags; B.shard_index = shard_index; B.num_shards = num_shards;
        B.caller_sa = d_sa; B.caller_lcp = d_lcp; B.cap = cap; B.num_suffixes_out = num_suffixes_out;
        B.is_dna = flags & SUFR_HIP_FLAG_DNA; B.allow_amb = flags & SUFR_HIP_FLAG_ALLOW_AMBIGUITY;
        B.raw = flags & SUFR_HIP_FLAG_RAW_TEXT; B.softmask = flags & SUFR_HIP_FLAG_IGNORE_SOFTMASK;
        return 0;
    }

    // the workspace of every build, and the text where vector loads can read it
    int open_text(Build& B)
    {
        const uint64_t n = B.n;
        if (!B.d_in_caller) { set_error("null text"); return SUFR_HIP_E_INVALID; }
        HIP_TRY(hipSetDevice(device));
        int rc;
        resident_text_len = 0;
        if ((rc = ensure(text, n + TEXT_PAD))) return rc;
        resident_text_len = n;                             // (`text` takes the normalised text of THIS call from here on)
        if ((rc = ensure(bytehist, 256 * 8))) return rc;
        if ((rc = ensure(lut, 512))) return rc;
        if ((rc = ensure(scalars, SC_N * 8))) return rc;
        uint8_t* d_text = B.d_text = (uint8_t*)text.p;

        HIP_TRY(hipEventRecord(ev[0], stream));
        B.d_in = B.d_in_caller;
        if ((uintptr_t)B.d_in & 15u) {   // vector loads need a 16-byte aligned source: stage it first
            HIP_TRY(hipMemcpyAsync(d_text, B.d_in, n, hipMemcpyDeviceToDevice, stream));
            B.d_in = d_text;
        }
        HIP_TRY(zero_later(d_text + n, TEXT_PAD));
        HIP_TRY(zero_later(bytehist.p, 256 * 8));
        return 0;
    }

    // ---- text chunking for the streaming kernels: workgroup w takes chunk w, group w % G.  The one place that knows the tile units.
    int plan_text_chunks(Build& B)
    {
        const uint64_t n = B.n;
        int rc;
        {
            uint64_t nvec = n / 16;
            uint32_t grid = (uint32_t)((nvec + 255) / 256);
            if (grid > 2048) grid = 2048;
            if (grid < 1) grid = 1;
            const uint32_t rtiles0 = (uint32_t)((n + TILE - 1) / TILE);
            if ((rc = ensure(tilefirst, (size_t)rtiles0 * 4))) return rc;
            if ((rc = ensure(runends, (size_t)rtiles0 * 64 * 8))) return rc;
            if ((rc = ensure(tileany, (size_t)rtiles0 * 8))) return rc;
            if (grid > rtiles0) grid = rtiles0;
            B.ngrid = grid;
        }
        const uint64_t ttiles = (n + TILE - 1) / TILE;
        uint64_t nwg_t = ttiles < text_wgs ? ttiles : text_wgs;
        uint64_t tiles_per = (ttiles + nwg_t - 1) / nwg_t;
        // chunks are multiples of every tile size: 8192 positions for the text-staging kernels, the big tiles of
        // k_msd_part_text (65536 positions; 16384 for texts that would not give every CU a large one)
        const bool small_tiles = n < ((uint64_t)1 << 25);     // (below ~2 large tiles per CU)
        const uint64_t tile_unit = small_tiles ? 4 : 16;
        tiles_per = (tiles_per + tile_unit - 1) / tile_unit * tile_unit;
        if (!small_tiles && num_cus > 0) {
            // One 1024-thread workgroup per CU at a time: W workgroups of equal work run in ceil(W / CUs) rounds, the last one
            // partly empty (1971 workgroups on 256 CUs: 7.7 rounds paid as 8).  Among the chunk sizes that give between half and
            // one and a half times the workgroups asked for, take the one whose last round is fullest.
            const uint64_t big = (ttiles + tile_unit - 1) / tile_unit;          // text in 65536-position tiles
            const uint64_t lo = std::max<uint64_t>(1, big / (text_wgs + text_wgs / 2)), hi = std::max<uint64_t>(lo, 2 * big / text_wgs);
            double best = -1.0; uint64_t best_per = tiles_per / tile_unit;
            for (uint64_t per = lo; per <= hi; per++) {
                const uint64_t w = (big + per - 1) / per;
                const double fill = (double)w / (double)(((w + num_cus - 1) / num_cus) * num_cus);
                if (fill > best + 1e-9 || (fill > best - 1e-9 && per < best_per)) { best = fill; best_per = per; }
            }
            tiles_per = best_per * tile_unit;
        }
        B.small_tiles = small_tiles;
        B.tchunk = tiles_per * TILE;
        B.nwg_t = (n + B.tchunk - 1) / B.tchunk;
        B.st.partition_workgroups = (uint32_t)B.nwg_t;
        B.G1 = msd_groups;
        return ensure(startbuf, (size_t)ttiles * 64 * 8 + 64);     // suffix-start bitmap, whole tiles
    }

    // the bit-packed stream of b-bit codes: whole 4 KB tiles, then a tail (cleared by the caller) for the partition kernel's
    // tiles of 65536 positions, which read past the last of them
    int ensure_packed(uint64_t n, int b, size_t& pbytes, size_t& ptail)
    {
        pbytes = (size_t)((n + TILE - 1) / TILE) * (TILE * b / 8);
        ptail = (size_t)16 * TILE * b / 8 + 64;
        return ensure(packedbuf, pbytes + ptail);
    }

    // ---- the normalised text, its byte counts and run-end tables.  DNA builds first try the fixed 3-bit code table
    // {$ % A C G N T}: ONE pass over the text (k_text_pass_dna) then writes the normalised text, the bit-packed code stream
    // and the run-end tables, counts those symbols, the first digit of every suffix start and the 5-mers that occur; any
    // other byte falls back to the general path (the text is normalised by then, and normalising is idempotent)
    static const uint8_t* dna_table_bytes() { static const uint8_t t[8] = {0, '$', '%', 'A', 'C', 'G', 'N', 'T'}; return t; }
    int text_stage(Build& B)
    {
        const uint8_t* const dna_bytes = dna_table_bytes();
        const uint64_t n = B.n, nwg_t = B.nwg_t, tchunk = B.tchunk;
        const uint32_t G1 = B.G1, num_shards = B.num_shards;
        const bool raw = B.raw, softmask = B.softmask;
        uint8_t* const d_text = B.d_text; const void* d_in = B.d_in; unsigned long long* const hist = B.hist;
        int rc;
        if (B.is_dna && !B.masked && !no_dna_table && !exc_disable) {
            size_t pbytes, ptail;
            if ((rc = ensure_packed(n, 3, pbytes, ptail))) return rc;
            if ((rc = ensure(rawtab, (size_t)G1 * TP_RAW_BINS * 4))) return rc;
            if ((rc = ensure(presbuf, (size_t)TP_RAW_BINS / 8))) return rc;
            if ((rc = ensure(rawtot, (size_t)TP_RAW_BINS * 4))) return rc;
            if ((rc = ensure(flagsbuf, (size_t)TP_RAW_BINS * 4))) return rc;
            if ((rc = ensure(exc_pos, (size_t)EXC_MAX_LIST * 4)) || (rc = ensure(exc_byte, (size_t)EXC_MAX_LIST))) return rc;
            HIP_TRY(zero_later((uint8_t*)packedbuf.p + pbytes, ptail));
            HIP_TRY(zero_later(rawtab.p, (size_t)G1 * TP_RAW_BINS * 4));
            HIP_TRY(zero_later(presbuf.p, (size_t)TP_RAW_BINS / 8));
            HIP_TRY(zero_flush());                          // (with the text pad and the byte counts: one launch)
            const uint32_t fixed_elig = B.allow_amb ? 0xFEu : ((1u << 1) | (1u << 3) | (1u << 4) | (1u << 5) | (1u << 7));
            HIP_TRY(hipFuncSetAttribute((const void*)k_text_pass_dna, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TP_LDS));
            // one resident workgroup per CU (its 128 KB of LDS counters allow no second), each over every tp_grid-th chunk; a
            // multiple of the groups, so that a workgroup's chunks all count into one group's row
            uint32_t tp_grid = (uint32_t)nwg_t;
            {
                const uint32_t cus = num_cus ? num_cus : 256u;
                const uint32_t per = cus / G1 * G1;
                if (per >= G1 && tp_grid > per) tp_grid = per;
            }
            hipLaunchKernelGGL(k_text_pass_dna, dim3(tp_grid), dim3(TP_NT), TP_LDS, stream, (const uint8_t*)d_in,
                               d_text, n, raw ? 1 : 0, softmask ? 1 : 0, (unsigned long long*)bytehist.p,
                               (uint32_t*)tilefirst.p, (uint64_t*)runends.p, (uint64_t*)tileany.p,
                               (uint8_t*)packedbuf.p, fixed_elig, tchunk, G1, (uint32_t*)rawtab.p, (uint32_t*)presbuf.p,
                               (uint64_t*)startbuf.p, (uint32_t*)exc_pos.p, (uint8_t*)exc_byte.p, EXC_MAX_LIST);
            hipLaunchKernelGGL(k_fold_raw, dim3(TP_RAW_BINS / 256), dim3(256), 0, stream, (const uint32_t*)rawtab.p, G1,
                               (const uint32_t*)presbuf.p, (uint32_t*)rawtot.p, (unsigned long long*)flagsbuf.p);
            HIP_TRY(hipGetLastError());
            unsigned long long cnt9[10];                       // [1..7] the table's symbols, [9] bytes outside it
            unsigned long long occurs[TP_RAW_BINS / 64];
            rawtot_host.clear();
            HIP_TRY(read_at_sync(cnt9, bytehist.p, sizeof cnt9));
            HIP_TRY(read_at_sync(occurs, flagsbuf.p, sizeof occurs));
            if (num_shards > 1) {                          // (a single shard needs no counts: it holds every eligible suffix)
                rawtot_host.resize(TP_RAW_BINS);
                HIP_TRY(read_at_sync(rawtot_host.data(), rawtot.p, (size_t)TP_RAW_BINS * 4));
            }
            HIP_TRY(sync_reads());
            B.pwords.assign(occurs, occurs + TP_RAW_BINS / 64);    // (the digit map is built from the words: 5 us of host time, not 67)
            // Bytes outside the table (sufr_exc.inc): the text pass has written 'N' for them and listed them.  A handful -- the IUPAC
            // codes of a real assembly, a '#' between sequences -- stay on this path: the build runs on that text and
            // exc_reinsert re-places the suffixes that looked at them (a sharded build: also into the shard their true first
            // digit says).  A text with more of them than the list holds does not.
            const unsigned long long foreign = cnt9[9];
            if (foreign == 0 || (foreign <= EXC_MAX_LIST && foreign * 64 <= n && !no_exceptions)) {
                B.dna_table = true;
                B.nexc = (uint32_t)foreign;
                exc_pending = B.nexc; B.st.num_exceptions = B.nexc;
                memset(hist, 0, sizeof B.hist);
                for (int c = 1; c < 8; c++) hist[dna_bytes[c]] = cnt9[c];
            } else {
                HIP_TRY(hipMemsetAsync(bytehist.p, 0, 256 * 8, stream));
                if (foreign <= EXC_MAX_LIST) {                 // the listed bytes back into the (normalised) text
                    hipLaunchKernelGGL(k_exc_restore, dim3(((uint32_t)foreign + 255) / 256), dim3(256), 0, stream, d_text,
                                       (const uint32_t*)exc_pos.p, (const uint8_t*)exc_byte.p, (uint32_t)foreign);
                    d_in = d_text;                             // already normalised
                } else {                                       // the list is cut short: from the caller's text again
                    d_in = B.d_in_caller;
                    if ((uintptr_t)d_in & 15u) { HIP_TRY(hipMemcpyAsync(d_text, d_in, n, hipMemcpyDeviceToDevice, stream)); d_in = d_text; }
                }
            }
        }
        HIP_TRY(zero_flush());                              // (builds that did not take the DNA text pass)
        if (!B.dna_table) {
            hipLaunchKernelGGL(k_normalize_bytehist, dim3(B.ngrid), dim3(256), 0, stream, (const uint8_t*)d_in,
                               d_text, n, raw ? 1 : 0, softmask ? 1 : 0, (unsigned long long*)bytehist.p,
                               (uint32_t*)tilefirst.p, (uint64_t*)runends.p, (uint64_t*)tileany.p);
            HIP_TRY(read_at_sync(hist, bytehist.p, sizeof B.hist));
            HIP_TRY(sync_reads());
        }
        rtab.ends = (const uint64_t*)runends.p;            // run-end tables of the normalised text
        rtab.tile_any = (const uint64_t*)tileany.p;
        rtab.first_end = (const uint32_t*)tilefirst.p;
        rtab.ntiles = (uint32_t)((n + TILE - 1) / TILE);
        {
            const uint32_t nblk = (rtab.ntiles + 255) / 256;     // <= 4096 for texts below 2^32 bytes
            if ((rc = ensure(nexttile, (size_t)rtab.ntiles * 4))) return rc;
            if ((rc = ensure(nextblk, (size_t)nblk * 4))) return rc;
            if (nblk <= 16u) {
                hipLaunchKernelGGL(k_next_tile_small, dim3(1), dim3(256), 0, stream, (const uint32_t*)tilefirst.p, rtab.ntiles,
                                   (uint32_t*)nexttile.p);
            } else {
            hipLaunchKernelGGL(k_next_tile_blocks, dim3(nblk), dim3(256), 0, stream, (const uint32_t*)tilefirst.p,
                               rtab.ntiles, (uint32_t*)nexttile.p, (uint32_t*)nextblk.p);
            hipLaunchKernelGGL(k_next_tile_heads, dim3(1), dim3(256), 0, stream, (uint32_t*)nextblk.p, nblk);
            hipLaunchKernelGGL(k_next_tile_apply, dim3(nblk), dim3(256), 0, stream, (uint32_t*)nexttile.p,
                               rtab.ntiles, (const uint32_t*)nextblk.p);
            }
            HIP_TRY(hipGetLastError());
            rtab.next_tile = (const uint32_t*)nexttile.p;
        }
        HIP_TRY(hipEventRecord(ev[1], stream));
        return 0;
    }

    // ---- alphabet -> dense codes (integer order of codes == raw byte order) ----------------------
    int code_table(Build& B)
    {
        const unsigned long long* const hist = B.hist;
        const uint8_t* const dna_bytes = dna_table_bytes();
        KeyParams& kp = B.kp;
        uint32_t sigma = 0;
        for (int c = 0; c < 256; c++) {
            h_lut[c] = 0;
            if (!hist[c]) continue;
            sigma++;
            // eligibility predicate, sufr_builder.rs:446-449
            bool el = c == '$' || !B.is_dna || c == 'A' || c == 'C' || c == 'G' || c == 'T' || B.allow_amb;
            uint32_t code = sigma;                         // dense rank among the bytes present
            if (B.dna_table) for (uint32_t k = 1; k < 8; k++) if (dna_bytes[k] == c) code = k;   // fixed table
            h_lut[c] = (uint16_t)(code | (el ? 0x8000u : 0u));
            if (el) B.eligible_total += hist[c];
        }
        kp.b = 1; while ((1u << kp.b) <= sigma) kp.b++;          // codes 0..sigma need b bits
        if (B.dna_table) kp.b = 3;                               // the packed stream is already written
        leaf_dna3 = B.dna_table;
        kp.K = 64 / kp.b;
        if (key_chars_knob > 0 && key_chars_knob < kp.K && key_chars_knob * kp.b >= 32 && packed_ok_for_knob(kp.b))
            kp.K = key_chars_knob;                               // probes: what a shorter key costs (DESIGN.md section 4)
        kp.dchars = 12 / kp.b; if (kp.dchars < 1) kp.dchars = 1;
        kp.dbits = kp.b * kp.dchars;
        kp.raw_bins = 1u << kp.dbits;
        kp.nbins = kp.raw_bins;
        kp.top_shift = 64 - kp.dbits;
        kp.elig_codes = 0;
        if (kp.b <= 4)
            for (int c = 0; c < 256; c++)
                if (h_lut[c] & 0x8000u) kp.elig_codes |= 1u << (h_lut[c] & 0x7fu);
        kp.detect_period = detect_period ? 1 : 0;
        kp.packed = nullptr;
        B.st.alphabet_size = sigma; B.st.bits_per_char = kp.b; B.st.chars_per_key = kp.K;
        HIP_TRY(hipMemcpyAsync(lut.p, h_lut, sizeof h_lut, hipMemcpyHostToDevice, stream));   // (h_lut is a member)
        return 0;
    }

    // ---- MSD digits: D characters each, as many as 15 bits hold when the bit-packed stream exists -----
    // (DNA: 5 characters, ~1400-1800 of the 32768 nominal values occur), else the 12-bit digits of the
    // text-staging kernels.  The presence pass gives the set of D-mers of the text; the dense digit map
    // numbers them in order.
    int first_digit_map(Build& B)
    {
        const uint64_t n = B.n;
        const bool dna_table = B.dna_table;
        KeyParams& kp = B.kp; std::vector<uint32_t>& pflags = B.pflags; std::vector<uint64_t>& pwords = B.pwords;
        int rc;
        const bool packed_path = B.packed_path = kp.b >= 2 && kp.b <= 4;
        // --max-query-len L with 32 <= L b <= K b (DNA: 11 <= L <= 21; the reference authors' `-m 12`, `-m 16`): the capped
        // build never looks beyond L characters.  Keys keep L characters; the bits below them carry the top of ~position
        // (k_msd_part_text<.., POS>), so equal L-prefixes come out of the MSD levels and the leaf sort in descending position;
        // what still ties is keyed by ~position whole (k_pos_keys); no run keys, no deep levels on the text, no
        // apply_max_query_len over the finished arrays.  Rounds 1-5 built the exact arrays first: `elegans -m 12` 9.6 ms
        // against 4.4 ms without the cap.  Other caps (and 5-bit alphabets) keep that form.  Listed bytes outside the DNA table
        // go with it: the suffixes whose first L symbols hold one are re-placed under the capped order (sufr_exc.inc).
        const bool mql_fast = B.mql_fast = mql_fast_ok && opt_max_query_len > 0 && kp.b == 3 && packed_path &&
                                           opt_max_query_len <= (uint64_t)kp.K && opt_max_query_len * (uint64_t)kp.b >= 32;
        B.mql_charbits = mql_fast ? (int)opt_max_query_len * kp.b : 0;
        if (mql_fast) { kp.K = (int)opt_max_query_len; kp.detect_period = 0; B.st.chars_per_key = (uint32_t)kp.K; }
        int D = packed_path ? 15 / kp.b : kp.dchars;
        int mbits = D * kp.b;
        KeyParams kq = kp;                                 // the presence pass flags digits of mbits bits
        kq.dchars = D; kq.dbits = mbits; kq.raw_bins = 1u << mbits; kq.nbins = kq.raw_bins; kq.top_shift = 64 - mbits;
        if (!dna_table) pflags.assign(kq.raw_bins, 1u);
        const bool want_presence = kq.raw_bins > 256;      // (packed alphabets have 12- to 15-bit digits: always)
        if (packed_path && !dna_table) {
            size_t pbytes, ptail;
            if ((rc = ensure_packed(n, kp.b, pbytes, ptail))) return rc;
            HIP_TRY(hipMemsetAsync((uint8_t*)packedbuf.p + pbytes, 0, ptail, stream));
        }
        if (want_presence) {
            if (!dna_table) {                              // (the DNA text pass has left the flags in pwords)
                if ((rc = ensure(flagsbuf, (size_t)kq.raw_bins * 4))) return rc;
                HIP_TRY(hipMemsetAsync(flagsbuf.p, 0, (size_t)kq.raw_bins * 4, stream));
                if ((rc = launch_presence((uint32_t)B.nwg_t, (size_t)kq.raw_bins + TILE + HALO + 512, B.d_text, n, kq,
                                          B.tchunk, (uint32_t*)flagsbuf.p,
                                          packed_path ? (uint8_t*)packedbuf.p : (uint8_t*)nullptr)))
                    return rc;
                HIP_TRY(read_at_sync(pflags.data(), flagsbuf.p, (size_t)kq.raw_bins * 4));
                HIP_TRY(sync_reads());
            }
            if (dna_table) pwords[0] |= 1ull; else pflags[0] = 1;     // digits entirely past the end of the text
        }
        if (packed_path) kp.packed = (const uint8_t*)packedbuf.p;
        // fewer characters per digit while more than MSD_MAX_BINS values occur
        bool from_words = dna_table;
        if (from_words) {
            uint32_t occ = 0;
            for (const uint64_t w : pwords) occ += (uint32_t)__builtin_popcountll(w);
            if (occ > MSD_MAX_BINS && D > 1) {             // (a text with many symbols beside ACGT: the flag form below)
                pflags.resize(TP_RAW_BINS);
                for (uint32_t v = 0; v < (uint32_t)TP_RAW_BINS; v++) pflags[v] = (uint32_t)((pwords[v >> 6] >> (v & 63u)) & 1ull);
                from_words = false;
            }
        }
        while (!from_words) {
            uint32_t occ = 0;
            for (uint32_t v : pflags) occ += v ? 1u : 0u;
            if (occ <= MSD_MAX_BINS || D == 1) break;
            D--; mbits = D * kp.b;
            std::vector<uint32_t> f2(1u << mbits, 0u);
            for (uint32_t v = 0; v < pflags.size(); v++) if (pflags[v]) f2[v >> kp.b] = 1u;
            pflags.swap(f2);
        }
        DigitMap& dm = B.dm;
        if ((rc = from_words ? upload_digit_map_words(pwords, mbits, dmapbuf, dmaphost, dm, B.present_vals)
                             : upload_digit_map(pflags, mbits, dmapbuf, dmaphost, dm, &B.present_vals))) return rc;
        if (dm.nbins > MSD_MAX_BINS) { set_error("alphabet too large for the radix digit counters"); return SUFR_HIP_E_UNSUPPORTED; }
        const uint32_t NB = B.NB = dm.nbins;
        B.mbits = mbits;
        B.st.digit_bits = (uint32_t)mbits;
        // the text-staging kernels (alphabets of more than 15 symbols) take the same digits through a flat table
        if (!packed_path) {
            kp.dchars = D; kp.dbits = mbits; kp.raw_bins = 1u << mbits; kp.top_shift = 64 - mbits; kp.nbins = (NB + 3u) & ~3u;
            if (want_presence) {
                remaphost.assign(kp.raw_bins, 0);
                uint32_t dense = 0;
                for (uint32_t v = 0; v < kp.raw_bins; v++) { remaphost[v] = (uint16_t)dense; if (pflags[v]) dense++; }
                if ((rc = ensure(remapbuf, (size_t)kp.raw_bins * 2))) return rc;
                HIP_TRY(hipMemcpyAsync(remapbuf.p, remaphost.data(), (size_t)kp.raw_bins * 2, hipMemcpyHostToDevice, stream));
                B.d_remap = (const uint16_t*)remapbuf.p;
            } else {
                kp.nbins = kp.raw_bins;
            }
        }
        return 0;
    }

    // character model of the leaf sort's counting digit: share of the suffix starts below every code
    // (codes that occur but start no suffix -- 'N', '%' -- get a sliver)
    int char_model(Build& B)
    {
        const unsigned long long* const hist = B.hist; const KeyParams& kp = B.kp; CharModel& cc = B.cc;
        int rc;
        double wsum = 0.0;
        double wt[257];
        const uint32_t ncodes = 1u << kp.b;
        for (uint32_t v = 0; v <= 256; v++) wt[v] = 0.0;
        for (int c = 0; c < 256; c++)
            if (hist[c]) { const double x = (h_lut[c] & 0x8000u) ? (double)hist[c] : 0.0; wt[h_lut[c] & 0xffu] += x; wsum += x; }
        const double floor_w = wsum / 4096.0;
        double tot = 0.0;
        for (int c = 0; c < 256; c++)
            if (hist[c] && wt[h_lut[c] & 0xffu] < floor_w) wt[h_lut[c] & 0xffu] = floor_w;
        for (uint32_t v = 0; v < ncodes; v++) tot += wt[v];
        cumhost.assign(ncodes + 1, 0u);
        double before = 0.0, ent2 = 0.0;
        for (uint32_t v = 0; v < ncodes; v++) {
            double f = before / (tot > 0 ? tot : 1.0) * 4294967296.0;
            cumhost[v] = f >= 4294967295.0 ? 0xffffffffu : (uint32_t)f;
            if (wt[v] > 0) { const double p = wt[v] / tot; ent2 -= p * log2(p); }
            before += wt[v];
        }
        cumhost[ncodes] = 0xffffffffu;
        if ((rc = ensure(cumbuf, (size_t)(ncodes + 1) * 4))) return rc;
        HIP_TRY(hipMemcpyAsync(cumbuf.p, cumhost.data(), (size_t)(ncodes + 1) * 4, hipMemcpyHostToDevice, stream));
        cc.cum = (const uint32_t*)cumbuf.p;
        cc.b = kp.b;
        cc.lastbit = B.mql_fast ? 0 : 64 - kp.K * kp.b;     // (a capped build sorts the position bits below the characters too)
        if (ent2 < 0.25) ent2 = 0.25;
        cc.mchars = (int)ceil(13.0 / ent2) + 1;        // ~12 bits of bucket number
        if (cc.mchars > 16) cc.mchars = 16;
        return 0;
    }

    // the raw first digits of the dense range [bin_lo, bin_hi): from the value of its first digit up to that of the first one
    // behind it (none behind it: no upper bound; the first shard: no lower bound)
    static void shard_raw_range(Build& B)
    {
        B.raw_lo = B.bin_lo < B.NB ? B.present_vals[B.bin_lo] : (1u << B.mbits);
        B.raw_hi = B.bin_hi < B.NB ? B.present_vals[B.bin_hi] : (1u << B.mbits);
        if (B.bin_lo == 0) B.raw_lo = 0;
    }

    // ---- level 1: the first-digit histogram, this shard's range of digits and its suffixes, the write cursors ----------
    int count_and_shard(Build& B)
    {
        const uint64_t n = B.n, nwg_t = B.nwg_t, tchunk = B.tchunk;
        const uint32_t G1 = B.G1, NB = B.NB, num_shards = B.num_shards, shard_index = B.shard_index;
        const int mbits = B.mbits;
        const KeyParams& kp = B.kp; const DigitMap& dm = B.dm; const std::vector<uint32_t>& present_vals = B.present_vals;
        const uint16_t* const d_remap = B.d_remap;
        uint32_t& bin_lo = B.bin_lo; uint32_t& bin_hi = B.bin_hi;
        int rc;
        B.raw_lo = 0; B.raw_hi = 1u << mbits;              // raw first-digit range of this shard
        bin_lo = 0; bin_hi = NB;
        if ((rc = ensure(leafbase, ((size_t)NB + 1) * 4))) return rc;
        HIP_TRY(hipEventRecord(ev[2], stream));
        uint64_t s_host = 0;                               // suffixes of this shard, when the host can tell
        bool s_known = false;
        if (B.packed_path) {
            if ((rc = ensure(grouptab, (size_t)G1 * NB * 4))) return rc;
            if ((rc = ensure(gcur, (size_t)G1 * NB * 4))) return rc;
            std::vector<uint32_t> tot;                     // suffix starts per dense first digit (all groups)
            if (B.dna_table) {
                // the text pass has counted raw 5-character digits; a digit of fewer characters (more than
                // MSD_MAX_BINS 5-mers occur) sums the raw values it is a prefix of
                const int fold = 15 - mbits;
                valshost = present_vals;
                if ((rc = ensure(valsbuf, (size_t)NB * 4))) return rc;
                HIP_TRY(hipMemcpyAsync(valsbuf.p, valshost.data(), (size_t)NB * 4, hipMemcpyHostToDevice, stream));
                hipLaunchKernelGGL(k_dense_grouptab, dim3((G1 * NB + 255) / 256), dim3(256), 0, stream,
                                   (const uint32_t*)rawtab.p, G1, (const uint32_t*)valsbuf.p, NB, fold, (uint32_t*)grouptab.p);
                if (num_shards > 1) {
                    tot.assign(NB, 0u);
                    for (uint32_t d = 0; d < NB; d++) {
                        uint64_t t = 0;
                        for (uint32_t j = 0; j < (1u << fold); j++) t += rawtot_host[((size_t)present_vals[d] << fold) + j];
                        tot[d] = (uint32_t)t;
                    }
                } else {
                    s_host = B.eligible_total; s_known = true;  // every eligible position starts a suffix of the one shard
                }
            } else {
                HIP_TRY(hipMemsetAsync(grouptab.p, 0, (size_t)G1 * NB * 4, stream));
                const size_t lds = msd_map_bytes_host(dm.rows) + (size_t)NB * 4;
#define SUFR_HIST_TEXT(BB) hipLaunchKernelGGL(k_msd_hist_text<BB>, dim3((uint32_t)nwg_t), dim3(THREADS), lds, stream, n, kp, \
                                              dm, tchunk, 0u, 1u << mbits, G1, (uint32_t*)grouptab.p)
                if (kp.b == 2) SUFR_HIST_TEXT(2); else if (kp.b == 3) SUFR_HIST_TEXT(3); else SUFR_HIST_TEXT(4);
#undef SUFR_HIST_TEXT
                if (num_shards > 1) {
                    std::vector<uint32_t> gt((size_t)G1 * NB);
                    HIP_TRY(read_at_sync(gt.data(), grouptab.p, gt.size() * 4));
                    HIP_TRY(sync_reads());
                    tot.assign(NB, 0u);
                    for (uint32_t g = 0; g < G1; g++) for (uint32_t d = 0; d < NB; d++) tot[d] += gt[(size_t)g * NB + d];
                }
            }
            HIP_TRY(hipGetLastError());
            if (num_shards > 1) {
                // "pivots chosen on device": shard = contiguous range of first digits with ~s/N suffixes, from
                // the exact counts (identical on every rank, no communication)
                uint64_t all = 0;
                for (uint32_t d = 0; d < NB; d++) all += tot[d];
                uint64_t dummy = 0;
                choose_shard(tot, all, shard_index, num_shards, bin_lo, bin_hi, dummy);
                shard_raw_range(B);
            }
            if (!tot.empty()) {
                for (uint32_t d = bin_lo; d < bin_hi; d++) s_host += tot[d];
                s_known = true;
            }
            hipLaunchKernelGGL(k_msd_cursors0, dim3(1), dim3(CUR0_NT), 0, stream, (const uint32_t*)grouptab.p, G1, NB, bin_lo,
                               bin_hi, (uint32_t*)leafbase.p, (uint32_t*)gcur.p, sc(SC_TOTAL));
        } else {
            if ((rc = ensure(table, (size_t)nwg_t * kp.nbins * 4))) return rc;
            if ((rc = ensure(bintot, (size_t)kp.nbins * 4))) return rc;
            if ((rc = ensure(binbase, (size_t)kp.nbins * 4))) return rc;
            const size_t rm_bytes = d_remap ? (size_t)kp.raw_bins * 2 : 0;
            const size_t lds_hist_text = (size_t)kp.nbins * 4 + TILE + HALO + 512 + rm_bytes;
            if (num_shards > 1) {
                // splitters only need proportions: every 16th tile is histogrammed (identical on every rank);
                // exact shard sizes come from the filtered histogram below
                const uint32_t stride = n > (64u << 20) ? 16u : 1u;
                if ((rc = launch_hist_text((uint32_t)nwg_t, lds_hist_text, B.d_text, n, kp, d_remap, kp.top_shift, tchunk,
                                           0u, kp.raw_bins, stride))) return rc;
                hipLaunchKernelGGL(k_scan_table_cols, dim3((kp.nbins + 255) / 256), dim3(256), 0, stream,
                                   (uint32_t*)table.p, (uint32_t)nwg_t, kp.nbins, (uint32_t*)bintot.p);
                std::vector<uint32_t> tot(kp.nbins);
                HIP_TRY(read_at_sync(tot.data(), bintot.p, (size_t)kp.nbins * 4));
                HIP_TRY(sync_reads());
                tot.resize(NB);
                uint64_t sampled = 0, dummy = 0;
                for (uint32_t v : tot) sampled += v;
                choose_shard(tot, sampled, shard_index, num_shards, bin_lo, bin_hi, dummy);
                shard_raw_range(B);
            }
            if ((rc = launch_hist_text((uint32_t)nwg_t, lds_hist_text, B.d_text, n, kp, d_remap, kp.top_shift, tchunk,
                                       B.raw_lo, B.raw_hi))) return rc;
            hipLaunchKernelGGL(k_scan_table_cols, dim3((kp.nbins + 255) / 256), dim3(256), 0, stream,
                               (uint32_t*)table.p, (uint32_t)nwg_t, kp.nbins, (uint32_t*)bintot.p);
            hipLaunchKernelGGL(k_scan_bins, dim3(1), dim3(256), 0, stream, (const uint32_t*)bintot.p, kp.nbins,
                               (uint32_t*)binbase.p, sc(SC_TOTAL));
            HIP_TRY(hipMemcpyAsync(leafbase.p, binbase.p, (size_t)NB * 4, hipMemcpyDeviceToDevice, stream));
        }
        B.st.top_lo = bin_lo; B.st.top_hi = bin_hi;
        HIP_TRY(hipEventRecord(ev[3], stream));
        unsigned long long s_ull = s_host;
        if (!s_known) {
            HIP_TRY(read_at_sync(&s_ull, sc(SC_TOTAL), 8));
            HIP_TRY(sync_reads());
        }
        B.s = s_ull;
        B.st.num_suffixes = B.s;
        if (B.num_suffixes_out) *B.num_suffixes_out = B.s;
        return 0;
    }

    // ---- the listed bytes back into the text, the suffixes that looked at them re-placed (sufr_exc.inc): bsa / blcp = the m
    // ranks of the build on 'N', the caller's arrays take the result.  `rebuilt`: the general code table has built the text instead.
    int reinsert_listed(Build& B, const uint32_t* bsa, const uint32_t* blcp, uint32_t m, bool& rebuilt)
    {
        const uint32_t nexc = B.nexc;
        rebuilt = false;
        HIP_TRY(hipEventRecord(ev[9], stream));
        std::vector<uint32_t> ep(nexc);
        HIP_TRY(hipMemcpyAsync(ep.data(), exc_pos.p, (size_t)nexc * 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(sync_reads());
        std::sort(ep.begin(), ep.end());
        int rc2;
        if ((rc2 = ensure(exc_sorted, (size_t)nexc * 4))) return rc2;
        HIP_TRY(hipMemcpyAsync(exc_sorted.p, ep.data(), (size_t)nexc * 4, hipMemcpyHostToDevice, stream));
        uint64_t affected = 0, s_final = m;
        ExcShard esh;
        esh.sharded = B.num_shards > 1 ? 1 : 0; esh.raw_lo = B.raw_lo; esh.raw_hi = B.raw_hi; esh.D = B.mbits / B.kp.b; esh.allow_amb = B.allow_amb ? 1 : 0;
        esh.cap = B.mql_fast ? (uint32_t)opt_max_query_len : 0u;
        rc2 = exc_reinsert(*this, B.d_text, B.n, bsa, blcp, m, (const uint32_t*)exc_sorted.p, nexc, B.caller_sa, B.caller_lcp, B.cap, &affected, esh, &s_final);
        HIP_TRY(sync_reads());                              // (ep: a host vector)
        if (rc2 == SUFR_HIP_E_UNSUPPORTED && err.empty()) {
            // more suffixes looked at the listed bytes than the whole-text sort takes (or than sufr_hip_set_exc_max_affected
            // allows): the general code table, from the caller's text.  exc_reinsert may have given up before it put the listed
            // bytes back: they go back here, so that nothing is pending while the text is built again.
            rebuilt = true;
            if (exc_pending) {
                hipLaunchKernelGGL(k_exc_restore, dim3((exc_pending + 255) / 256), dim3(256), 0, stream, B.d_text,
                                   (const uint32_t*)exc_pos.p, (const uint8_t*)exc_byte.p, exc_pending);
                HIP_TRY(hipGetLastError());
                exc_pending = 0;
            }
            if (B.num_shards > 1) return retry_whole_text(B);
            exc_disable = true;
            rc2 = sort_device_u32(B.d_in_caller, B.n, B.flags, 0, 1, B.caller_sa, B.caller_lcp, B.cap, B.num_suffixes_out, B.st_out);
            exc_disable = false;
            return rc2;
        }
        if (rc2 == SUFR_HIP_E_CAPACITY && B.num_suffixes_out) *B.num_suffixes_out = s_final;      // (what the call needs)
        if (rc2) return rc2;
        B.st.num_exceptions = nexc; B.st.num_reinserted = affected;
        if (s_final != m) {                                // (a shard: suffixes moved between the shards)
            B.st.num_suffixes = s_final;
            if (B.num_suffixes_out) *B.num_suffixes_out = s_final;
        }
        B.mql_count = (uint32_t)s_final;
        HIP_TRY(hipEventRecord(ev[10], stream));
        return 0;
    }

    // ---- the retry of a SHARDED build.  This rank's first-digit range was chosen on the 3-bit digits of the text with 'N' for the
    // listed bytes, and the ranks that do not retry keep the suffixes whose TRUE first D bytes lie in their ranges (exc_true_in).
    // The general code table has other digits (4- or 5-bit codes, fewer characters), so a range chosen on its histogram would
    // not fit between the neighbours': suffixes would be lost or repeated.  Instead the rank builds the WHOLE text with the
    // general table as one shard into arrays of its own, and hands out the ranks whose true first D bytes lie in
    // [raw_lo, raw_hi) -- contiguous, because the arrays are in the order of the bytes (a capped build: of its first L >= 8 > D
    // symbols); both ends by binary search, a probe = one rank and the D bytes at it.  Cost: the time of a one-GPU build of the
    // text and two arrays of all its suffixes on this rank, for a text that the whole-text sort cannot take.
    static uint64_t true_prefix_of_digit(uint32_t raw, int D)              // exc_digit_prefix (sufr_exc.inc) on the host
    {
        static const uint8_t bytes[8] = {0, '$', '%', 'A', 'C', 'G', 'N', 'T'};
        uint64_t v = 0;
        for (int i = D - 1; i >= 0; i--) { const uint32_t c = (raw >> (3 * i)) & 7u; v = (v << 9) | (c ? (uint64_t)bytes[c] + 1u : 0u); }
        return v;
    }
    // first rank of sa[0, s) whose suffix has D-byte prefix (9 bits a byte, byte + 1, 0 past the text: exc_true_prefix) >= bound
    int first_rank_at_or_above(const uint32_t* sa, uint64_t s, uint64_t n, int D, uint64_t bound, uint64_t& rank)
    {
        uint64_t lo = 0, hi = s;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            uint32_t p = 0;
            uint8_t b[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            HIP_TRY(hipMemcpyAsync(&p, sa + mid, 4, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (p >= n) { set_error("a suffix array entry past the text"); return SUFR_HIP_E_HIP; }
            const uint64_t have = n - p < (uint64_t)D ? n - p : (uint64_t)D;
            HIP_TRY(hipMemcpyAsync(b, (const uint8_t*)text.p + p, (size_t)have, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            uint64_t v = 0;
            for (int i = 0; i < D; i++) v = (v << 9) | ((uint64_t)i < have ? (uint64_t)b[i] + 1u : 0u);
            if (v < bound) lo = mid + 1; else hi = mid;
        }
        rank = lo;
        return 0;
    }
    int retry_whole_text(Build& B)
    {
        const int D = B.mbits / B.kp.b;
        const uint64_t all = B.eligible_total;             // ('N' starts a suffix iff the byte it stands for does: the count is the true text's)
        int rc;
        if (D < 1 || D > 7) { set_error("first digit of " + std::to_string(D) + " characters"); return SUFR_HIP_E_UNSUPPORTED; }
        if ((rc = ensure(exc_all_sa, all * 4 + 64)) || (rc = ensure(exc_all_lcp, all * 4 + 64))) return rc;
        const uint32_t* const wsa = (const uint32_t*)exc_all_sa.p; const uint32_t* const wlcp = (const uint32_t*)exc_all_lcp.p;
        uint64_t s_all = 0;
        sufr_hip_stats wst;
        memset(&wst, 0, sizeof wst);
        exc_disable = true;
        rc = sort_device_u32(B.d_in_caller, B.n, B.flags, 0, 1, (uint32_t*)exc_all_sa.p, (uint32_t*)exc_all_lcp.p, all, &s_all, &wst);
        exc_disable = false;
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(stream));
        uint64_t first = 0, last = s_all;
        if (B.raw_lo && (rc = first_rank_at_or_above(wsa, s_all, B.n, D, true_prefix_of_digit(B.raw_lo, D), first))) return rc;
        if (!(B.raw_hi >> (3 * D)) && (rc = first_rank_at_or_above(wsa, s_all, B.n, D, true_prefix_of_digit(B.raw_hi, D), last))) return rc;
        const uint64_t mine = last > first ? last - first : 0;
        if (debug) fprintf(stderr, "[sufr_hip debug] retry of shard %u of %u: ranks [%llu, %llu) of %llu\n", B.shard_index, B.num_shards,
                           (unsigned long long)first, (unsigned long long)last, (unsigned long long)s_all);
        if (B.num_suffixes_out) *B.num_suffixes_out = mine;
        wst.num_suffixes = mine; wst.top_lo = B.st.top_lo; wst.top_hi = B.st.top_hi;      // (the shard's own; the rest: the build that made the arrays)
        if (B.st_out) *B.st_out = wst;
        if (mine == 0) return 0;
        if ((rc = check_capacity(mine, B.cap, B.caller_sa, B.caller_lcp))) return rc;
        HIP_TRY(hipMemcpyAsync(B.caller_sa, wsa + first, mine * 4, hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipMemcpyAsync(B.caller_lcp, wlcp + first, mine * 4, hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return 0;
    }

    // a shard without suffixes in the text as it was BUILT still takes the suffixes whose true first bytes fall into its range
    // -- unless that range holds no digit at all (bin_lo == bin_hi: nothing lies in it, and its raw bounds say nothing)
    int empty_shard(Build& B)
    {
        if (B.nexc && B.num_shards > 1 && B.bin_lo < B.bin_hi) {
            bool rebuilt = false;
            int rc = reinsert_listed(B, nullptr, nullptr, 0u, rebuilt);
            if (rc || rebuilt) return rc;
            if (!B.mql_fast && opt_max_query_len > 0 && (rc = apply_max_query_len(opt_max_query_len, B.n, B.caller_sa, B.caller_lcp, B.mql_count))) return rc;
            HIP_TRY(sync_reads());
            HIP_TRY(hipGetLastError());
        }
        return done(B);
    }

    int working_arrays(Build& B)
    {
        const uint64_t s = B.s;
        int rc;
        B.m0 = (uint32_t)s;
        B.d_sa = B.caller_sa; B.d_lcp = B.caller_lcp;
        if (B.nexc) {                                          // the arrays of the build on 'N' for the listed bytes: the caller's are written by exc_reinsert
            // (re-writing the caller's arrays in place, only the blocks of ranks that change, was built and measured in round 6: a
            // suffix that leaves its rank comes back millions of ranks away -- "ACGR" sorts behind ALL of "ACGN...", and half of a
            // soft-mask-ignored genome is N --, so 70-91 % of the blocks shift by one or more: save + write of those is more
            // traffic than this one streaming pass, 66.8 against 62.0 ms with 23 '#' delimiters)
            if ((rc = ensure(exc_sa, s * 4 + 64)) || (rc = ensure(exc_lcp, s * 4 + 64))) return rc;
            B.d_sa = (uint32_t*)exc_sa.p; B.d_lcp = (uint32_t*)exc_lcp.p;
        }
        if ((rc = ensure(recA, s * sizeof(Rec) + 64))) return rc;
        if ((rc = ensure(recB, s * sizeof(Rec) + 64))) return rc;
        const size_t nheads = s / 64 + 2;
        if ((rc = ensure(headsA, nheads * 4))) return rc;
        B.xr[0] = (Rec*)recA.p; B.xr[1] = (Rec*)recB.p;
        return 0;
    }

    // ---- THE radix-partition kernel over the text: nothing but the choice of its instantiation -------------
    int launch_partition(Build& B)
    {
        const uint64_t n = B.n, nwg_t = B.nwg_t, tchunk = B.tchunk;
        const uint32_t G1 = B.G1, NB = B.NB, raw_lo = B.raw_lo, raw_hi = B.raw_hi, num_shards = B.num_shards;
        const bool small_tiles = B.small_tiles, mql_fast = B.mql_fast;
        const KeyParams& kp = B.kp; const DigitMap& dm = B.dm; Rec* const* const xr = B.xr;
        int rc;
        HIP_TRY(hipEventRecord(ev[4], stream));
        if (B.packed_path) {
#define SUFR_PART_TEXT_G(BB, NT_, RN_, SH)                                                                               \
            {                                                                                                            \
                using Geom = PartGeom<BB, NT_, RN_>;                                                                     \
                const size_t lds = Geom::lds_bytes(dm.raw_mask + 1u, NB);                                                \
                if (lds > PART_LDS_MAX) { set_error("first-level digit map too large for the partition kernel"); return SUFR_HIP_E_UNSUPPORTED; } \
                HIP_TRY(hipFuncSetAttribute((const void*)k_msd_part_text<BB, NT_, RN_, SH>,                             \
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                     \
                if (BB == 3 && mql_fast) {                                                                               \
                    HIP_TRY(hipFuncSetAttribute((const void*)k_msd_part_text<3, NT_, RN_, SH, true>,                     \
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                 \
                    hipLaunchKernelGGL((k_msd_part_text<3, NT_, RN_, SH, true>), dim3((uint32_t)nwg_t), dim3(NT_), lds, stream, \
                                       n, kp, dm, tchunk, raw_lo, raw_hi, G1, (uint32_t*)gcur.p, xr[0],                 \
                                       (const uint64_t*)startbuf.p, (uint32_t)(~0ull << (64 - kp.K * kp.b)),            \
                                       (uint32_t)(kp.K * kp.b - 32));                                                   \
                } else                                                                                                   \
                hipLaunchKernelGGL((k_msd_part_text<BB, NT_, RN_, SH>), dim3((uint32_t)nwg_t), dim3(NT_), lds, stream,  \
                                   n, kp, dm, tchunk, raw_lo, raw_hi, G1, (uint32_t*)gcur.p, xr[0],                     \
                                   (const uint64_t*)startbuf.p, (uint32_t)(~0ull << (64 - kp.K * kp.b)), 0u);           \
            }
            // (3-bit codes with more than ~2 600 first digits -- seven symbols that all mix -- take half-size tiles: the three
            // counter arrays and a 65 536-position tile do not share the 160 KB)
#define SUFR_PART_TEXT(BB, NT_, SH)                                                                                      \
            {                                                                                                            \
                if (BB == 3 && NT_ == 1024 && PartGeom<3, 1024, 2>::lds_bytes(dm.raw_mask + 1u, NB) > PART_LDS_MAX) {    \
                    half_tiles = true;                                                                                   \
                    SUFR_PART_TEXT_G(3, 1024, 1, SH)                                                                     \
                } else SUFR_PART_TEXT_G(BB, NT_, 2, SH)                                                                  \
            }
#ifdef SUFR_HIP_PROBES
#define SUFR_PART_TEXT_R3(BB, NT_, SH)                                                                                   \
            {                                                                                                            \
                using Geom = PartGeomR3<BB, NT_, 2>;                                                                     \
                const size_t lds = Geom::lds_bytes((uint32_t)msd_map_bytes_host(dm.rows), NB);                          \
                HIP_TRY(hipFuncSetAttribute((const void*)k_msd_part_text_r3<BB, NT_, 2, SH>,                            \
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                     \
                hipLaunchKernelGGL((k_msd_part_text_r3<BB, NT_, 2, SH>), dim3((uint32_t)nwg_t), dim3(NT_), lds, stream, \
                                   n, kp, dm, tchunk, raw_lo, raw_hi, G1, (uint32_t*)gcur.p, xr[0],                     \
                                   (const uint64_t*)startbuf.p, (uint32_t)(~0ull << (64 - kp.K * kp.b)));               \
            }
#define SUFR_PART_TEXT_V(BB, NT_, SH) { if (part_r3) SUFR_PART_TEXT_R3(BB, NT_, SH) else SUFR_PART_TEXT(BB, NT_, SH) }
#else
#define SUFR_PART_TEXT_V(BB, NT_, SH) SUFR_PART_TEXT(BB, NT_, SH)
#endif
#define SUFR_PART_TEXT_B(BB)                                                                                             \
            {                                                                                                            \
                if (small_tiles) { if (sh) SUFR_PART_TEXT_V(BB, 256, true) else SUFR_PART_TEXT_V(BB, 256, false) }       \
                else { if (sh) SUFR_PART_TEXT_V(BB, 1024, true) else SUFR_PART_TEXT_V(BB, 1024, false) }                 \
            }
            const bool sh = num_shards > 1;
            bool half_tiles = false;
            if (!B.dna_table) {                            // (the DNA text pass has written the suffix-start bitmap)
                const uint32_t nw64 = (uint32_t)((n + 63) / 64);
#define SUFR_STARTBITS(BB) hipLaunchKernelGGL(k_startbits_packed<BB>, dim3((nw64 + 255) / 256), dim3(256), 0, stream, \
                                              kp.packed, n, kp.elig_codes, (uint64_t*)startbuf.p)
                if (kp.b == 2) SUFR_STARTBITS(2); else if (kp.b == 3) SUFR_STARTBITS(3); else SUFR_STARTBITS(4);
#undef SUFR_STARTBITS
            }
            if (kp.b == 2) SUFR_PART_TEXT_B(2) else if (kp.b == 3) SUFR_PART_TEXT_B(3) else SUFR_PART_TEXT_B(4)
#undef SUFR_PART_TEXT_B
#undef SUFR_PART_TEXT_V
#undef SUFR_PART_TEXT
#undef SUFR_PART_TEXT_G
            B.st.partition_variant = half_tiles ? 4u : 3u;
        } else {
            if ((rc = launch_scatter_text((uint32_t)nwg_t, B.d_text, n, kp, B.d_remap, kp.top_shift, tchunk, raw_lo, raw_hi,
                                          num_shards > 1, xr[0]))) return rc;
            B.st.partition_variant = 0u;
        }
        HIP_TRY(hipEventRecord(ev[5], stream));
        HIP_TRY(hipGetLastError());
        return 0;
    }

    // ---- leaf sort + finish of the small buckets; further MSD levels for the others; what no level can split: `left` ----
    int msd_levels(Build& B, LeftOver& left)
    {
        const uint64_t n = B.n, s = B.s;
        const uint32_t m0 = B.m0, NB = B.NB;
        const int mbits = B.mbits;
        const bool mql_fast = B.mql_fast;
        const KeyParams& kp = B.kp; const DigitMap& dm = B.dm; Rec* const* const xr = B.xr; FinishOut& fo = B.fo;
        int rc;
        const uint32_t nwin = B.nwin = (m0 + 127) / 128;     // 128-position windows of the tie bitmaps
        const uint32_t fixcap = B.fixcap = (uint32_t)(s / 32 + 65536);
        if ((rc = ensure(wmaskbuf, (size_t)nwin * 32))) return rc;
        B.wcnt_stride = (nwin + 3u) & ~3u;                   // (the second row starts 16-byte aligned: scan_u32 takes one launch)
        if ((rc = ensure(wcntbuf, (size_t)B.wcnt_stride * 8))) return rc;
        if ((rc = ensure(fixbuf, (size_t)fixcap * 4))) return rc;
        HIP_TRY(zero_later(wmaskbuf.p, (size_t)nwin * 32));
        HIP_TRY(zero_later(sc(SC_NFIX), 8));
        if ((rc = ensure(pairsc, (size_t)PSC_N * 8))) return rc;
        HIP_TRY(zero_later(pairsc.p, (size_t)PSC_N * 8));    // (the pair path's sums: tie_level)
        HIP_TRY(zero_flush());
        fo.SA = B.d_sa; fo.LCP = B.d_lcp; fo.wmask = (unsigned long long*)wmaskbuf.p; fo.fixlist = (uint32_t*)fixbuf.p;
        fo.nfix = (uint32_t*)sc(SC_NFIX); fo.fixcap = fixcap; fo.b = kp.b; fo.K = kp.K;
        rg_active.clear(); rg_run_off = 0;                 // (run buckets of this build: sufr_runs.inc)
        if ((rc = ensure(segst[0], 256))) return rc;
        if ((rc = ensure(segsz[0], 256))) return rc;
        segcur = 0;
        h_seg0[0] = 0u; h_seg0[1] = m0;                 // (a member: the copies are asynchronous)
        HIP_TRY(hipMemcpyAsync(segst[0].p, &h_seg0[0], 4, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(segsz[0].p, &h_seg0[1], 4, hipMemcpyHostToDevice, stream));
        uint32_t nseg = 1;
        uint64_t m = s;
        int src = 0;
        int bits_done = mbits;
        DigitMap dl = dm;                              // digit map of the level that produced the current leaves
        const int maxbits = mql_fast ? 64 : kp.K * kp.b;     // (a capped build: the position bits below the characters are digits too)
        const int charbits = mql_fast ? B.mql_charbits : maxbits;
        uint32_t levels = 1;
        for (;;) {
            uint32_t nbig = 0; uint64_t mbig = 0, maxbig = 0;
            if ((rc = leaf_stage(xr[src], xr[1], nseg, m, dl, B.cc, fo, 64 - bits_done, nbig, mbig, maxbig)))
                return rc;
            if (debug) fprintf(stderr, "[sufr_hip debug] msd level %u: segments=%u records=%llu bits=%d -> big leaves=%u records=%llu\n",
                               levels, nseg, (unsigned long long)m, bits_done, nbig, (unsigned long long)mbig);
            if (!nbig) break;
            segcur ^= 1; nseg = nbig; m = mbig;
            if (levels == 1 && B.packed_path && !mql_fast) {
                if ((rc = run_groups_extract(B.d_text, n, kp, xr[src], xr[1], (uint32_t)(mbits / kp.b), s, fo, nseg, m, maxbig))) return rc;
                if (!nseg) break;
            }
            // digit of the next level: the dense D-character digit while the table of sub-buckets stays small,
            // else as many plain bits as that allows; nothing once the key is used up
            int w = 0;
            const bool in_chars = bits_done < charbits;   // (a digit never holds characters and position bits)
            const int digit_end = in_chars ? charbits : maxbits;
            bool char_digit = false;                      // the dense D-character digit of the text
            if (bits_done < digit_end) {
                w = mbits;
                if (bits_done + w > digit_end) w = digit_end - bits_done;
                uint64_t budget = (1ull << 26) / nseg;      // sub-bucket cells per level (2^28: one level less on the --dna build, -1 ms of 105: the tables themselves cost)
                int wb = 0; while (wb < 12 && (2ull << wb) <= budget) wb++;     // an identity map holds <= MSD_MAX_BINS values
                char_digit = in_chars && bits_done % mbits == 0 && w == mbits && (uint64_t)NB <= budget;
                if (!char_digit) { if (w > wb) w = wb; if (w < 1) w = 1; }
            }
            // Segments are dealt to the groups whole (their workgroups share an XCD and complete each other's lines in
            // its L2): one segment that outweighs a group's share -- the N^k bucket of an --allow-ambiguity build is
            // half of all records -- would leave seven eighths of the chip idle.  Then every workgroup strides over
            // the whole tile list.
            const uint32_t G = (nseg >= 64 && maxbig * msd_groups <= m + m / 2) ? msd_groups : 1u;
            uint32_t SG = 0, tub = 0;
            if ((rc = plan_tiles(nseg, m, G, (uint32_t)(ms_nt * ms_e), SG, tub))) return rc;
            if (w == 0) {
                // these buckets' members share all K key characters: the re-keying levels take them as groups
                // (their records must lie in the array the levels read: xr[1])
                if (src != 1)
                    hipLaunchKernelGGL(k_copy_tiles, dim3(1024), dim3(256), 0, stream, (const Rec*)xr[src],
                                       (const uint4*)tdesc.p, (const unsigned long long*)sc(SC_UTOTAL), xr[1]);
                hipLaunchKernelGGL(k_append_starts, dim3((nseg + 255) / 256), dim3(256), 0, stream,
                                   (const uint32_t*)segst[segcur].p, nseg, fo.fixlist, fo.nfix, fo.fixcap);
                hipLaunchKernelGGL(k_advance_fix, dim3(1), dim3(64), 0, stream, (uint32_t*)sc(SC_NFIX),
                                   (const unsigned long long*)nullptr, nseg);
                HIP_TRY(hipGetLastError());
                left.groups = nseg; left.records = m; left.depth = (uint32_t)(bits_done / kp.b); left.maxbig = maxbig;
                break;
            }
            DigitMap dn = dm;
            if (!char_digit) { if ((rc = identity_digit_map(w, dn))) return rc; }
            bits_done += w;
            const int shift = 64 - bits_done;
            const uint32_t NBn = dn.nbins;
            const uint64_t cells = (uint64_t)nseg * NBn;
            if ((rc = ensure(leafcnt, cells * 4))) return rc;
            if ((rc = ensure(leafoff, cells * 4))) return rc;
            if ((rc = ensure(leafbase, cells * 4))) return rc;
            if ((rc = ensure(leafcur, cells * 4))) return rc;
            HIP_TRY(hipMemsetAsync(leafcnt.p, 0, cells * 4, stream));
            {
                const size_t lds = msd_map_bytes_host(dn.rows) + (size_t)NBn * 4;
                hipLaunchKernelGGL(k_msd_hist, dim3(2048), dim3(THREADS), lds, stream, (const Rec*)xr[src],
                                   (const uint4*)tdesc.p, (const unsigned long long*)sc(SC_UTOTAL), shift, dn,
                                   (uint32_t*)leafcnt.p);
            }
            if ((rc = scan_u32((const uint32_t*)leafcnt.p, (uint32_t)cells, (uint32_t*)leafoff.p))) return rc;
            hipLaunchKernelGGL(k_msd_leafbase, dim3((uint32_t)((cells + 255) / 256)), dim3(256), 0, stream,
                               (const uint32_t*)leafoff.p, (const uint32_t*)segst[segcur].p, nseg, NBn,
                               (uint32_t*)leafbase.p, (uint32_t*)leafcur.p);
            {
#define SUFR_MSD_SCATTER(NT_, E_)                                                                                        \
                {                                                                                                    \
                    const size_t lds = (size_t)(NT_ * E_) * 14 + msd_map_bytes_host(dn.rows) +                      \
                                       (size_t)((NBn + 3u) & ~3u) * 4 + 128;                                        \
                    HIP_TRY(hipFuncSetAttribute((const void*)k_msd_scatter<NT_, E_>,                                \
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));             \
                    hipLaunchKernelGGL((k_msd_scatter<NT_, E_>), dim3(ms_e == 8 ? 1024 : 2048), dim3(NT_), lds, stream, \
                                       (const Rec*)xr[src], (const uint4*)tdesc.p, (const uint32_t*)upre.p, G, SG,  \
                                       (const unsigned long long*)sc(SC_UTOTAL), shift, dn, (uint32_t*)leafcur.p,   \
                                       xr[src ^ 1]);                                                                \
                }
                // (1024 threads / 8192-record tiles: no faster, and one workgroup per CU)
                // (1024 threads x 10: 10 240-record tiles, one workgroup per CU: +2 ms, profiles/r06_level2_tiles.txt)
                if (ms_e == 4) SUFR_MSD_SCATTER(512, 4) else if (ms_e == 6) SUFR_MSD_SCATTER(512, 6) else SUFR_MSD_SCATTER(512, 8)
#undef SUFR_MSD_SCATTER
            }
            HIP_TRY(hipGetLastError());
            src ^= 1;
            dl = dn;
            levels++;
        }
        B.st.num_passes = levels;
        HIP_TRY(hipEventRecord(ev[6], stream));
        // LCP of every window's (and left-over group's) first record with the record before it
        hipLaunchKernelGGL(k_fix_window_lcp, dim3(1024), dim3(256), 0, stream, (const uint32_t*)fixbuf.p,
                           (const uint32_t*)sc(SC_NFIX), fixcap, (const Rec*)xr[1], B.d_lcp, kp.b, kp.K);
        // (the counts of the tie bitmaps, k_tie_counts, are taken in tie_level: behind the pair path, which clears bits)
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev[7], stream));
        B.st.num_levels = 1;
        return 0;
    }

    // the join: once per build, whoever comes first -- its result, its counts, then the run buckets it left to be expanded
    int join_left_chain(Build& B, LeftChain& chain)
    {
        if (!chain.th.joinable()) return 0;                // (not started, or joined already)
        chain.th.join();
        if (chain.rc) { err = helper->err; return chain.rc; }
        B.st.num_levels += chain.st.num_levels;
        B.st.num_large_groups += chain.st.num_large_groups;
        B.st.deep_records += chain.st.deep_records;
        return run_groups_expand(B.d_text, B.n, B.kp, B.d_sa, B.d_lcp);
    }

    // ---- buckets whose members agree on all K key characters: groups for the re-keying levels, here or (from opt_overlap_min
    // records on) on the helper pipeline, side by side with the tie level ----------
    int start_left_chain(Build& B, const LeftOver& left, LeftChain& chain)
    {
        const uint64_t n = B.n;
        const bool mql_fast = B.mql_fast;
        const KeyParams kp = B.kp;                             // (the helper thread takes a copy)
        uint8_t* const d_text = B.d_text; uint32_t* const d_sa = B.d_sa; uint32_t* const d_lcp = B.d_lcp; Rec* const* const xr = B.xr;
        uint32_t left_groups = left.groups;
        int rc;
        // (run buckets of the whole key among them are found here; those taken out after the first level join the list now,
        // with their own depth)
        if (left_groups && left.maxbig >= RG_MIN_SIZE && !mql_fast && (rc = run_groups_find(d_text, n, kp, xr[1], xr[1], (const uint32_t*)segst[segcur].p, (uint32_t*)segsz[segcur].p,
                                                 left_groups, (uint32_t)kp.K, RG_MIN_SIZE, false))) return rc;
        uint32_t early = 0;
        for (const RunGroupState& S : rg_active) if (S.K != (uint32_t)kp.K) early++;
        const uint32_t* depth_of = nullptr;
        if (early) {
            const uint32_t Lall = left_groups + early;
            std::vector<uint32_t> hs(early), hz(early), hd(Lall, left.depth);
            uint32_t e = 0;
            for (const RunGroupState& S : rg_active)
                if (S.K != (uint32_t)kp.K) { hs[e] = S.g.start; hz[e] = S.M; hd[left_groups + e] = S.K; e++; }
            if ((rc = ensure_keep(segst[segcur], (size_t)Lall * 4)) || (rc = ensure_keep(segsz[segcur], (size_t)Lall * 4))) return rc;
            if ((rc = ensure(rg_depth, (size_t)Lall * 4))) return rc;
            HIP_TRY(hipMemcpyAsync((uint32_t*)segst[segcur].p + left_groups, hs.data(), (size_t)early * 4, hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemcpyAsync((uint32_t*)segsz[segcur].p + left_groups, hz.data(), (size_t)early * 4, hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemcpyAsync(rg_depth.p, hd.data(), (size_t)Lall * 4, hipMemcpyHostToDevice, stream));
            HIP_TRY(sync_reads());           // (host vectors)
            depth_of = (const uint32_t*)rg_depth.p;
            left_groups = Lall;
        }
        if (!left_groups) return 0;
        LevelState lg;
        lg.k = nullptr; lg.i = (const uint32_t*)xr[1] + 2; lg.istride = 3; lg.s = nullptr; lg.o = nullptr; lg.m = B.m0; lg.deep = false; lg.sbits = 0;
        lg.L = left_groups; lg.heads_cur = &headsA; lg.heads_nxt = &headsB; lg.depth_cur = &depthA;
        lg.depth_nxt = &depthB; lg.which = 0;
        lg.seg_start = (const uint32_t*)segst[segcur].p; lg.seg_size = (const uint32_t*)segsz[segcur].p;
        lg.seg_depth = left.depth; lg.seg_depth_of = depth_of;
        lg.pos_keys = mql_fast;
        if (mql_fast) lg.seg_depth = (uint32_t)kp.K;          // (they agree on their L characters: every LCP inside is cut back to L)
        const bool side_by_side = overlap_chains && left.records >= (opt_overlap_min ? opt_overlap_min : OVERLAP_MIN_DEFAULT);
        if (debug) fprintf(stderr, "[sufr_hip debug] left-over buckets: groups=%u records=%llu%s\n", left_groups,
                           (unsigned long long)left.records, side_by_side ? " (on the helper pipeline)" : "");
        if (side_by_side) {
            // this chain on the helper pipeline, side by side with the tie runs
            if (!helper) {
                helper.reset(new Pipeline);
                if ((rc = helper->init(device))) { err = helper->err; helper->destroy(); helper.reset(); return rc; }
            }
            Pipeline& H = *helper;
            H.read_env();
            H.debug = debug;
            H.rtab = rtab;
            if ((rc = H.ensure(H.lut, 512)) || (rc = H.ensure(H.scalars, SC_N * 8))) { err = H.err; return rc; }
            HIP_TRY(hipMemcpyAsync(H.lut.p, lut.p, sizeof h_lut, hipMemcpyDeviceToDevice, stream));
            HIP_TRY(hipEventRecord(ev[11], stream));           // the records, the segment list and the code table are in place
            HIP_TRY(hipStreamWaitEvent(H.stream, ev[11], 0));
            lg.heads_cur = &H.headsA; lg.heads_nxt = &H.headsB; lg.depth_cur = &H.depthA; lg.depth_nxt = &H.depthB;
            H.reset_reads();
            chain.st = sufr_hip_stats(); chain.rc = 0;
            H.dbl_entries = 0;
            last_overlapped = 1;
            chain.th = std::thread([&H, &chain, lg, d_text, n, kp, d_sa, d_lcp, this]() {
                (void)hipSetDevice(device);
                chain.rc = H.run_levels(lg, d_text, n, kp, d_sa, d_lcp, chain.st);
                if (hipStreamSynchronize(H.stream) != hipSuccess && !chain.rc) { H.set_error("the helper stream failed"); chain.rc = SUFR_HIP_E_HIP; }
            });
        } else {
            if ((rc = run_levels(lg, d_text, n, kp, d_sa, d_lcp, B.st))) return rc;
            if ((rc = run_groups_expand(d_text, n, kp, d_sa, d_lcp))) return rc;
        }
        return 0;
    }

    // tie runs packed densely: a wave per window (WAVE), or a thread per window
    template <bool WAVE>
    void launch_build_ties(uint32_t nwin, const uint32_t* icur, uint32_t m0, uint32_t K, LevelArrays& A)
    {
        hipLaunchKernelGGL(k_build_ties<WAVE>, dim3(WAVE ? (nwin + 3) / 4 : (nwin + 255) / 256), dim3(256), 0, stream,
                           (const unsigned long long*)wmaskbuf.p, (const uint32_t*)recoff.p, (const uint32_t*)runoff.p, icur, m0, K,
                           (uint32_t*)A.idxA.p, (uint32_t*)A.segA.p, (uint32_t*)A.opos.p, (uint32_t*)depthA.p, (uint8_t*)period.p);
    }

    // ---- the tie level: tie runs (equal whole keys) packed densely, whole segments as groups ----------
    int tie_level(Build& B, LeftChain& chain)
    {
        const uint64_t n = B.n;
        const uint32_t m0 = B.m0, nwin = B.nwin, wcnt_stride = B.wcnt_stride, num_shards = B.num_shards;
        const bool mql_fast = B.mql_fast;
        const KeyParams& kp = B.kp; sufr_hip_stats& st = B.st;
        uint8_t* const d_text = B.d_text; uint32_t* const d_sa = B.d_sa; uint32_t* const d_lcp = B.d_lcp;
        int rc;
        uint32_t* cnt = (uint32_t*)wcntbuf.p;
        const uint32_t* icur = d_sa;                   // tie members lie in SA in key order
        if ((rc = ensure(recoff, (size_t)nwin * 4))) return rc;
        if ((rc = ensure(runoff, (size_t)nwin * 4))) return rc;
        // The pair path (exact builds): count the tie pairs per window, scan, list their ranks, walk them -- all queued ahead
        // of the round trip below, under which the walk runs.  Whether the path pays is decided on the device, from the share of
        // pairs among the tie records (pair_path_taken); the list holds m0 / 8 pairs, what lies beyond it stays with the level.
        // (probes: with the finisher's pair walk switched off the path is off too -- the switch measures a build without walks)
        const bool pair_path = !mql_fast && opt_pair_walk != 2u && !(finish_opts & (1u << 29));
        const uint32_t pair_cap = m0 / 8u + 4096u;
        unsigned long long psums[PSC_N];
        if (pair_path) {
            if ((rc = ensure(pairbuf, (size_t)pair_cap * 4))) return rc;
            const uint32_t nblk = (nwin + 255u) / 256u;            // a workgroup per 256 windows
            uint32_t* blkcnt = (uint32_t*)runoff.p; uint32_t* blkoff = (uint32_t*)recoff.p;       // (free until the scans below)
            unsigned long long* psc = (unsigned long long*)pairsc.p;
            const uint32_t force = opt_pair_walk == 1u ? 1u : 0u;
            hipLaunchKernelGGL(k_pair_counts, dim3(nblk), dim3(256), 0, stream,
                               (const unsigned long long*)wmaskbuf.p, nwin, blkcnt, psc);
            if ((rc = scan_u32(blkcnt, nblk, blkoff, psc + PSC_PAIRS))) return rc;
            hipLaunchKernelGGL(k_pair_list, dim3(nblk), dim3(256), 0, stream,
                               (const unsigned long long*)wmaskbuf.p, nwin, (const uint32_t*)blkcnt, (const uint32_t*)blkoff,
                               (const unsigned long long*)psc, force, PAIR_MIN_PERMILLE, pair_cap, (uint32_t*)pairbuf.p);
            uint32_t grid = (pair_cap + 255u) / 256u;
            if (grid > 8192u) grid = 8192u;                   // (the lanes stride over the list: its length is known on the device only)
            hipLaunchKernelGGL(k_pair_walk, dim3(grid), dim3(256), 0, stream, (const uint32_t*)pairbuf.p, psc, force,
                               PAIR_MIN_PERMILLE, pair_cap, (const uint8_t*)d_text, n, kp, (uint32_t)kp.K, d_sa, d_lcp,
                               (unsigned long long*)wmaskbuf.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(read_at_sync(psums, psc, sizeof psums));
        }
        // wcnt = [records per window | runs per window]: two exclusive scans give the dense offsets
        hipLaunchKernelGGL(k_tie_counts, dim3((nwin + 255) / 256), dim3(256), 0, stream,
                           (const unsigned long long*)wmaskbuf.p, nwin, cnt, wcnt_stride);
        if ((rc = scan_u32((const uint32_t*)cnt, nwin, (uint32_t*)recoff.p, sc(SC_TMP0)))) return rc;
        unsigned long long tot2[2] = {0, 0};          // records in tie runs, tie runs, (and the fix-list length)
        if ((rc = scan_u32((const uint32_t*)(cnt + wcnt_stride), nwin, (uint32_t*)runoff.p, sc(SC_TMP1)))) return rc;
        unsigned long long nf = 0;
        HIP_TRY(read_at_sync(tot2, sc(SC_TMP0), 16));
        HIP_TRY(read_at_sync(&nf, sc(SC_NFIX), 8));
        HIP_TRY(sync_reads());        // one round trip for the three
        if ((uint32_t)nf > B.fixcap) { set_error("internal error: window list overflow"); return SUFR_HIP_E_HIP; }
        const unsigned long long tot_rec = tot2[0], tot_run = tot2[1];
        const uint32_t m2 = (uint32_t)tot_rec, L2 = (uint32_t)tot_run;
        if (pair_path) {
            unsigned long long members = 0, resolved = 0;
            for (uint32_t i = 0; i < 64; i++) { members += psums[PSC_MEMBERS + i]; resolved += psums[PSC_RESOLVED + i]; }
            const unsigned long long pairs = psums[PSC_PAIRS];
            const bool taken = opt_pair_walk == 1u || 2ull * pairs * 1000ull >= members * (unsigned long long)PAIR_MIN_PERMILLE;   // (pair_path_taken)
            const unsigned long long walked = taken ? (pairs < pair_cap ? pairs : (unsigned long long)pair_cap) : 0ull;
            last_pairs_resolved += resolved; last_pairs_left += walked - resolved;
            if (debug) fprintf(stderr, "[sufr_hip debug] pair path: tie records=%llu pairs=%llu %s resolved=%llu handed back=%llu\n",
                               members, pairs, taken ? "walked" : "(too few: not walked)", resolved, walked - resolved);
        }
        if (debug) fprintf(stderr, "[sufr_hip debug] tie level: runs=%u records=%u\n", L2, m2);
        if (m2 == 0) return 0;
        st.num_levels++;
        st.num_large_groups += L2;
        st.deep_records += m2;
        LevelArrays& A = lv[0];
        if ((rc = ensure(A.keyA, (size_t)m2 * 8))) return rc;
        if ((rc = ensure(A.idxA, (size_t)m2 * 4))) return rc;
        if ((rc = ensure(A.segA, (size_t)m2 * 4))) return rc;
        if ((rc = ensure(A.opos, (size_t)m2 * 4))) return rc;
        if ((rc = ensure(depthA, (size_t)L2 * 4))) return rc;
        if ((rc = ensure(period, (size_t)L2))) return rc;
        if ((rc = ensure(headsA, ((size_t)m2 / 64 + 2) * 4))) return rc;
        // (a wave per window pays from ~8 tied records per window on: measured 2.5 / 1.0 ms at 3, ~6 / 16.7 ms at 22)
        if ((uint64_t)m2 >= (uint64_t)nwin * 8) launch_build_ties<true>(nwin, icur, m0, (uint32_t)kp.K, A);
        else launch_build_ties<false>(nwin, icur, m0, (uint32_t)kp.K, A);
        if (mql_fast)
            hipLaunchKernelGGL(k_pos_keys, dim3((m2 + 255) / 256), dim3(256), 0, stream, (const uint32_t*)A.idxA.p, m2, (uint64_t*)A.keyA.p);
        else
        hipLaunchKernelGGL(k_gather_keys, dim3((m2 + 255) / 256), dim3(256), 0, stream,
                           (const uint8_t*)d_text, n, rtab, (const uint16_t*)lut.p,
                           (const uint32_t*)A.idxA.p, (const uint32_t*)A.segA.p, (const uint32_t*)depthA.p,
                           (const uint8_t*)period.p, m2, kp, (uint64_t*)A.keyA.p, (uint32_t*)nullptr);
        uint32_t Lt = 0;
        if ((rc = finish_level((const uint64_t*)A.keyA.p, (const uint32_t*)A.idxA.p, (const uint32_t*)A.segA.p,
                               (const uint32_t*)A.opos.p, (const uint32_t*)depthA.p, m2, 0, d_text, n, kp, d_sa, d_lcp,
                               &headsA, Lt))) return rc;
        LevelState lt;
        lt.k = (const uint64_t*)A.keyA.p; lt.i = (const uint32_t*)A.idxA.p; lt.s = (const uint32_t*)A.segA.p;
        lt.o = (const uint32_t*)A.opos.p; lt.m = m2; lt.deep = true; lt.sbits = 0; lt.L = Lt;
        lt.heads_cur = &headsA; lt.heads_nxt = &headsB; lt.depth_cur = &depthA; lt.depth_nxt = &depthB;
        lt.which = 1;
        // Prefix doubling keys a suffix p of depth d by the RANK of p + d.  A shard holds the ranks of its own first-digit range
        // only (round 4's soak found sharded builds reading whatever the rank array held elsewhere: 38 000 wrong ranks in a
        // 4 Mb text of templated repeats over two shards, then a memory fault): there the rank array is cleared first, and a
        // position without a rank is keyed like one that starts no suffix -- by its run key --, below or above all ranked
        // ones as its first digit lies below or above the shard's range (DblShard).  Without a packed stream to read that
        // digit from, sharded builds stay with the levels.
        dbl_shard = DblShard{kp.packed, kp.b, B.mbits, B.raw_lo, B.raw_hi, num_shards > 1 ? 1 : 0};
        lt.allow_doubling = !mql_fast && (num_shards <= 1 || (B.packed_path && kp.packed != nullptr)); lt.s_total = m0;
        lt.pos_keys = mql_fast;
        before_doubling = [this, &B, &chain]() { return join_left_chain(B, chain); };
        rc = run_levels(lt, d_text, n, kp, d_sa, d_lcp, st);
        before_doubling = nullptr;
        return rc;
    }

    // the times of the phases, from the events the stages have recorded (ev[8]: the end of the build, behind a synchronisation)
    int finish_stats(Build& B)
    {
        sufr_hip_stats& st = B.st;
#ifdef SUFR_HIP_PROBES
        if (debug) {
            unsigned long long ws[4] = {0, 0, 0, 0}, zero[4] = {0, 0, 0, 0};
            (void)hipMemcpyFromSymbol(ws, HIP_SYMBOL(g_walk_stats), sizeof ws);
            (void)hipMemcpyToSymbol(HIP_SYMBOL(g_walk_stats), zero, sizeof zero);
            fprintf(stderr, "[sufr_hip debug] pair walks: %llu, characters walked: %llu, longest: %llu\n", ws[0], ws[1], ws[2]);
            unsigned long long ph[3][16], phz[3][16];
            memset(phz, 0, sizeof phz);
            (void)hipMemcpyFromSymbol(ph, HIP_SYMBOL(g_phase), sizeof ph);
            (void)hipMemcpyToSymbol(HIP_SYMBOL(g_phase), phz, sizeof phz);
            static const char* names[3] = {"k_msd_part_text", "k_msd_scatter", "k_finish<DEEP> (0 load/flags, 1 ranking, 2 pair walks, 3 re-key, 4 writes, 5 rounds x 1000)"};
            for (int k = 0; k < 3; k++) {
                unsigned long long tot = 0;
                for (int i = 0; i < 16; i++) tot += ph[k][i];
                if (!tot) continue;
                fprintf(stderr, "[sufr_hip debug] %s phases (share of wave 0's cycles):", names[k]);
                for (int i = 0; i < 16; i++) if (ph[k][i]) fprintf(stderr, " %d:%.3f", i, (double)ph[k][i] / (double)tot);
                fprintf(stderr, "  (total %.3g cycles)\n", (double)tot);
            }
        }
#endif
        (void)hipEventElapsedTime(&st.ms_total, ev[0], ev[8]);
        (void)hipEventElapsedTime(&st.ms_normalize, ev[0], ev[1]);
        (void)hipEventElapsedTime(&st.ms_hist_text, ev[2], ev[3]);
        (void)hipEventElapsedTime(&st.ms_partition, ev[4], ev[5]);
        (void)hipEventElapsedTime(&st.ms_passes, ev[5], ev[6]);
        (void)hipEventElapsedTime(&st.ms_finish, ev[6], ev[7]);
        (void)hipEventElapsedTime(&st.ms_deep, ev[7], ev[8]);
        if (B.nexc) (void)hipEventElapsedTime(&st.ms_exceptions, ev[9], ev[10]);
        return done(B);
    }

    // Contiguous top-digit range for shard `r` of `R`: cumulative suffix counts balanced to s/R.
    static void choose_shard(const std::vector<uint32_t>& tot, uint64_t total, uint32_t r, uint32_t R,
                             uint32_t& lo, uint32_t& hi, uint64_t& count)
    {
        // boundary k (k = 0..R): smallest bin index such that the cumulative count before it >= k*total/R
        auto boundary = [&](uint32_t k) -> uint32_t {
            if (k == 0) return 0;
            if (k >= R) return (uint32_t)tot.size();
            uint64_t target = (uint64_t)((__uint128_t)total * k / R);
            uint64_t cum = 0;
            for (uint32_t d = 0; d < tot.size(); d++) {
                if (cum >= target) return d;
                cum += tot[d];
            }
            return (uint32_t)tot.size();
        };
        lo = boundary(r); hi = boundary(r + 1);
        count = 0;
        for (uint32_t d = lo; d < hi; d++) count += tot[d];
    }
};

}  // namespace sufr
