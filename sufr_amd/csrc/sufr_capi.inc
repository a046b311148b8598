// sufr_capi.inc -- extern "C" entry points declared in include/sufr_hip.h (included by sufr_kernels.hip).

struct sufr_hip_ctx {
    sufr::Pipeline pl;
    // windowed builds (sufr_wide.inc): window / margin set by sufr_hip_set_window (0: the defaults) and their buffers
    uint64_t wide_window = 0, wide_margin = 0;
    uint64_t array_budget = 0;        // sufr_hip_set_array_budget: device bytes the SA + LCP of a windowed create may take at once (0: no limit set)
    sufr::DevBuf wtext, wsa, wlcp, wblk;
    sufr::DevBuf mtmp, mpoff, mbytes;  // SMEM scan sums, slice offsets and packed slices (sufr_match.inc)
    sufr::DevBuf xq, xoff, xlo, xhi, xcand, xsum;  // MEMs, k-mismatch, k-difference (sufr_mem.inc, sufr_approx.inc, sufr_edit.inc): doubled batch, rank ranges, candidate starts, scan sums
    sufr::DevBuf ecnt, ekeys, ekeys2, ehist;  // k-difference (sufr_edit.inc): ends per candidate, the two key buffers of the sort, its digit counts
    sufr::DevBuf tsc, trows, tmisc;    // alignment traceback (sufr_trace.inc): the scalars of a call, the rows of a chunk, its scan sums and run counts
    uint64_t trace_scratch = 0;        // sufr_hip_set_trace_scratch: bytes of row storage (0: the default)
    sufr::DevBuf kbits, ksum, kstarts; // k-mer counts (sufr_kmer.inc): head / whole words, tile summaries and carries and stats, sequence starts
    std::vector<uint64_t> kmer_starts; // the sequence starts kstarts holds
    uint32_t kmer_tile = 0;            // sufr_hip_set_kmer_tile: ranks per tile (0: the default)
    sufr::DevBuf rell, rpyr, rbits, rsum;  // repeats (sufr_repeat.inc): the clipped LCP, the coarser levels of its min pyramid, flag words and prefixes, tile sums and stats
    uint32_t repeat_tile = 0;          // sufr_hip_set_repeat_tile: ranks per tile (0: the default)
    sufr::DevBuf lzpyr, lzarr, lztab, lzsum;  // LPF and LZ77 (sufr_lz.inc): the two min pyramids, LPF and SRC, the parse tables, tile entries / bases / candidates and stats
    uint32_t lz_rank_tile = 0, lz_pos_tile = 0;  // sufr_hip_set_lz_tile: ranks per LPF tile, positions per parse tile (0: the default)
    sufr::DevBuf bwtbytes, bwtsum, bwttab;  // BWT, runs and LF (sufr_bwt.inc): the BWT bytes, tile summaries / carries / counts and stats, the tiles' bases per occurring byte value
    uint32_t bwt_tile = 0;             // sufr_hip_set_bwt_tile: ranks per tile (0: the default)
    sufr::DevBuf shkeys, shhist, shpre, shsum;  // sequence counts (sufr_shared.inc): the two key buffers of the sort, its digit counts, H / P, tile sums and candidates and stats and the profile
    bool wide(uint64_t n) const { return n >= sufr::SUFR_MAX_TEXT_LEN || (wide_window && n > wide_window); }
};

#include <atomic>
#include <chrono>
#include <mutex>
#include <thread>

namespace {
thread_local std::string g_create_error;

// Host <-> device copies of the large arrays for callers that hand over ordinary (pageable) buffers (the host-buffer ABI the
// libsufr shim binds, sufr_hip_build_u32 / _u64: 3.1 GB in, 15.1 GB out for a human-sized text).  hipMemcpy on pageable memory
// runs at ~11 GB/s on the test box.  Round 1-5: <= 12 threads, each moving one 16 MB piece at a time through one pinned buffer
// (copy -> wait -> memcpy, nothing overlapped), a fresh set of pinned buffers and threads for every array: ~16 GB/s, 1.15-1.26 s
// for the human-sized build.  Round 6: ALL arrays of a call are one list of pieces; a worker owns two pinned buffers and keeps a
// device copy in flight on its stream while it memcpy's the piece before (to_host) or after (to_device) it -- the memcpy also
// takes the first-touch faults of a fresh destination, spread over the workers --; the pinned buffers are allocated once per
// process and reused (hipHostMalloc of 16 MB: ~1.5 ms).
struct CopyJob { void* dst; const void* src; uint64_t bytes; };

struct PinPool {
    std::mutex mu;
    std::vector<void*> free_bufs;
    static constexpr uint64_t PIECE = (uint64_t)8 << 20;
    void* take()
    {
        {
            std::lock_guard<std::mutex> g(mu);
            if (!free_bufs.empty()) { void* p = free_bufs.back(); free_bufs.pop_back(); return p; }
        }
        void* p = nullptr;
        if (hipHostMalloc(&p, PIECE, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        return p;
    }
    void give(void* p) { if (p) { std::lock_guard<std::mutex> g(mu); free_bufs.push_back(p); } }
};
PinPool& pin_pool() { static PinPool* pool = new PinPool; return *pool; }      // (never destroyed: the runtime may be gone at exit)

unsigned copy_workers(uint64_t npieces)
{
    unsigned W = std::thread::hardware_concurrency();
    if (W == 0) W = 4;
    // 6 to 12 workers move the 18.2 GB of a human-sized call at the rate of the link (50-55 GB/s each way, 0.39-0.42 s per call on
    // the test box); 16 and more fight over the page faults of the destination: 24 -> 0.52 s, 48 -> 0.73-0.87 s
    // (profiles/r06_host_abi.txt)
    const unsigned cap = 10;
    if (W > cap) W = cap;
    if (W > npieces) W = (unsigned)npieces;
    return W ? W : 1;
}

int parallel_copy_jobs(int device, const CopyJob* jobs, int njobs, bool to_host)
{
    uint64_t total = 0;
    for (int j = 0; j < njobs; j++) total += jobs[j].bytes;
    if (!total) return 0;
    if (total < ((uint64_t)256 << 20)) {      // threads and streams cost a few ms to set up
        if (hipSetDevice(device) != hipSuccess) return SUFR_HIP_E_HIP;
        for (int j = 0; j < njobs; j++)
            if (jobs[j].bytes && hipMemcpy(jobs[j].dst, jobs[j].src, jobs[j].bytes, to_host ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice) != hipSuccess)
                return SUFR_HIP_E_HIP;
        return 0;
    }
    const uint64_t PIECE = PinPool::PIECE;
    // pieces of all jobs in one numbering: job j owns [first[j], first[j + 1])
    std::vector<uint64_t> first(njobs + 1, 0);
    for (int j = 0; j < njobs; j++) first[j + 1] = first[j] + (jobs[j].bytes + PIECE - 1) / PIECE;
    const uint64_t npieces = first[njobs];
    const unsigned W = copy_workers(npieces);
    std::atomic<uint64_t> next{0};
    std::atomic<int> failed{0};
    auto locate = [&](uint64_t i, uint8_t*& d, const uint8_t*& sp, uint64_t& len) {
        int j = 0;
        while (i >= first[j + 1]) j++;
        const uint64_t off = (i - first[j]) * PIECE;
        len = jobs[j].bytes - off < PIECE ? jobs[j].bytes - off : PIECE;
        d = (uint8_t*)jobs[j].dst + off; sp = (const uint8_t*)jobs[j].src + off;
    };
    auto worker = [&]() {
        void* pin[2] = {pin_pool().take(), pin_pool().take()};
        hipStream_t st = nullptr;
        hipEvent_t ev[2] = {nullptr, nullptr};
        bool ok = pin[0] && pin[1] && hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess &&
                  hipEventCreateWithFlags(&ev[0], hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&ev[1], hipEventDisableTiming) == hipSuccess;
        if (!ok) failed = 1;
        uint8_t* d[2] = {nullptr, nullptr}; const uint8_t* sp[2] = {nullptr, nullptr}; uint64_t len[2] = {0, 0};
        bool busy[2] = {false, false};                    // a device copy of this buffer is in flight
        int cur = 0;
        while (ok && !failed) {
            const uint64_t i = next.fetch_add(1);
            if (i >= npieces) break;
            // buffer `cur` is free here (to_host: its piece was memcpy'd out; to_device: its copy is waited for below)
            if (!to_host && busy[cur]) { if (hipEventSynchronize(ev[cur]) != hipSuccess) { failed = 1; break; } busy[cur] = false; }
            locate(i, d[cur], sp[cur], len[cur]);
            if (to_host) {
                if (hipMemcpyAsync(pin[cur], sp[cur], len[cur], hipMemcpyDeviceToHost, st) != hipSuccess || hipEventRecord(ev[cur], st) != hipSuccess) { failed = 1; break; }
                busy[cur] = true;
                const int prev = cur ^ 1;                 // the piece before: land it while this one flies
                if (busy[prev]) {
                    if (hipEventSynchronize(ev[prev]) != hipSuccess) { failed = 1; break; }
                    memcpy(d[prev], pin[prev], len[prev]);
                    busy[prev] = false;
                }
            } else {
                memcpy(pin[cur], sp[cur], len[cur]);
                if (hipMemcpyAsync(d[cur], pin[cur], len[cur], hipMemcpyHostToDevice, st) != hipSuccess || hipEventRecord(ev[cur], st) != hipSuccess) { failed = 1; break; }
                busy[cur] = true;
            }
            cur ^= 1;
        }
        for (int q = 0; q < 2; q++) {
            const int bq = cur ^ q;                       // (oldest first)
            if (ok && busy[bq]) {
                if (hipEventSynchronize(ev[bq]) != hipSuccess) failed = 1;
                else if (to_host && !failed) memcpy(d[bq], pin[bq], len[bq]);
                busy[bq] = false;
            }
        }
        if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
        for (int q = 0; q < 2; q++) { if (ev[q]) (void)hipEventDestroy(ev[q]); pin_pool().give(pin[q]); }
    };
    std::vector<std::thread> th;
    for (unsigned w = 0; w < W; w++) th.emplace_back(worker);
    for (auto& x : th) x.join();
    if (failed) {
        // (no pinned memory left, no stream: the plain copies are slower, not wrong -- every piece is written whole again)
        (void)hipGetLastError();
        if (hipSetDevice(device) != hipSuccess) return SUFR_HIP_E_HIP;
        for (int j = 0; j < njobs; j++)
            if (jobs[j].bytes && hipMemcpy(jobs[j].dst, jobs[j].src, jobs[j].bytes, to_host ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice) != hipSuccess)
                return SUFR_HIP_E_HIP;
    }
    return 0;
}

int parallel_copy(int device, void* dst, const void* src, uint64_t bytes, bool to_host)
{
    const CopyJob j = {dst, src, bytes};
    return parallel_copy_jobs(device, &j, 1, to_host);
}

// Validates the option pair the way SufrBuilder::new does (sufr_builder.rs:163-165, types.rs:80-83) and
// hands the options to the pipeline for the next sort_device_u32 call.
int take_options(sufr_hip_ctx* ctx, uint64_t max_query_len, const char* seed_mask)
{
    ctx->pl.opt_max_query_len = 0;
    ctx->pl.opt_mask_offsets.clear();
    if (seed_mask && max_query_len > 0) {   // sufr_builder.rs:163-165
        ctx->pl.set_error("Cannot use max_query_len and seed_mask together");
        return SUFR_HIP_E_CONFLICT;
    }
    if (seed_mask) {                        // types.rs:80-83, regex ^1+0[01]*1$ (163-166)
        size_t n = strlen(seed_mask), i = 0;
        bool ok = n >= 3;
        while (ok && i < n && seed_mask[i] == '1') i++;
        ok = ok && i > 0 && i < n && seed_mask[i] == '0';
        for (; ok && i < n; i++) ok = seed_mask[i] == '0' || seed_mask[i] == '1';
        ok = ok && seed_mask[n - 1] == '1';
        if (!ok) {
            ctx->pl.set_error(std::string("Invalid seed mask '") + seed_mask + "'");
            return SUFR_HIP_E_SEED_MASK;
        }
        for (size_t k = 0; k < n; k++)      // "care" offsets, types.rs:124-135
            if (seed_mask[k] == '1') ctx->pl.opt_mask_offsets.push_back((uint32_t)k);
    }
    ctx->pl.opt_max_query_len = max_query_len;
    return 0;
}
}  // namespace

extern "C" {

int sufr_hip_abi_version(void) { return SUFR_HIP_ABI_VERSION; }

int sufr_hip_device_count(void)
{
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) return 0;
    return cnt;
}

sufr_hip_ctx* sufr_hip_create(int device_id)
{
    sufr_hip_ctx* ctx = new (std::nothrow) sufr_hip_ctx();
    if (!ctx) { g_create_error = "out of memory"; return nullptr; }
    int rc = ctx->pl.init(device_id);
    if (rc != 0) {
        g_create_error = ctx->pl.err;
        ctx->pl.destroy();
        delete ctx;
        return nullptr;
    }
    return ctx;
}

extern "C" void sufr_io_release_ctx_(const sufr_hip_ctx* ctx);    // sufr_io.cpp: a windowed shard kept for sufr_hip_shard_write

void sufr_hip_destroy(sufr_hip_ctx* ctx)
{
    if (!ctx) return;
    sufr_io_release_ctx_(ctx);
    (void)hipSetDevice(ctx->pl.device);
    for (sufr::DevBuf* b : {&ctx->wtext, &ctx->wsa, &ctx->wlcp, &ctx->wblk, &ctx->mtmp, &ctx->mpoff, &ctx->mbytes,
                            &ctx->xq, &ctx->xoff, &ctx->xlo, &ctx->xhi, &ctx->xcand, &ctx->xsum,
                            &ctx->ecnt, &ctx->ekeys, &ctx->ekeys2, &ctx->ehist, &ctx->tsc, &ctx->trows, &ctx->tmisc,
                            &ctx->kbits, &ctx->ksum, &ctx->kstarts, &ctx->rell, &ctx->rpyr, &ctx->rbits, &ctx->rsum,
                            &ctx->lzpyr, &ctx->lzarr, &ctx->lztab, &ctx->lzsum,
                            &ctx->bwtbytes, &ctx->bwtsum, &ctx->bwttab,
                            &ctx->shkeys, &ctx->shhist, &ctx->shpre, &ctx->shsum}) ctx->pl.release(*b);
    ctx->pl.destroy();
    delete ctx;
}

const char* sufr_hip_last_error(const sufr_hip_ctx* ctx)
{
    return ctx ? ctx->pl.err.c_str() : g_create_error.c_str();
}

// Internal (sufr_io.cpp): does a text of n bytes take the windowed build on this context?
int sufr_hip_is_wide_(const sufr_hip_ctx* ctx, uint64_t n) { return ctx && ctx->wide(n) ? 1 : 0; }
int sufr_hip_ctx_device_(const sufr_hip_ctx* ctx) { return ctx ? ctx->pl.device : -1; }

void sufr_hip_set_error_(sufr_hip_ctx* ctx, const char* msg)
{
    if (ctx) ctx->pl.set_error(msg ? msg : "");
}

int sufr_hip_set_stream(sufr_hip_ctx* ctx, void* hip_stream)
{
    if (!ctx) return SUFR_HIP_E_INVALID;
    if (ctx->pl.own_stream && ctx->pl.stream) (void)hipStreamDestroy(ctx->pl.stream);
    ctx->pl.own_stream = false;
    ctx->pl.stream = (hipStream_t)hip_stream;
    return 0;
}

int sufr_hip_set_window(sufr_hip_ctx* ctx, uint64_t window, uint64_t margin)
{
    if (!ctx) return SUFR_HIP_E_INVALID;
    if (window && window < 16) { ctx->pl.set_error("window below 16 positions"); return SUFR_HIP_E_INVALID; }
    ctx->wide_window = window;
    ctx->wide_margin = margin;
    return 0;
}

int sufr_hip_set_array_budget(sufr_hip_ctx* ctx, uint64_t bytes)
{
    if (!ctx) return SUFR_HIP_E_INVALID;
    ctx->array_budget = bytes;
    return 0;
}

uint64_t sufr_hip_array_budget_(const sufr_hip_ctx* ctx) { return ctx ? ctx->array_budget : 0; }

int sufr_hip_set_window_retry(sufr_hip_ctx* ctx, uint64_t widest_margin)
{
    if (!ctx) return SUFR_HIP_E_INVALID;
    ctx->pl.opt_wide_retry = widest_margin;
    return 0;
}

uint64_t sufr_hip_window_repairs(const sufr_hip_ctx* ctx) { return ctx ? ctx->pl.wide_orphans : 0; }

int sufr_hip_set_overlap_min(sufr_hip_ctx* ctx, uint64_t min_records)
{
    if (!ctx) return SUFR_HIP_E_INVALID;
    ctx->pl.opt_overlap_min = min_records;
    return 0;
}

int sufr_hip_overlapped(const sufr_hip_ctx* ctx) { return ctx ? (int)ctx->pl.last_overlapped : 0; }
uint64_t sufr_hip_doublings(const sufr_hip_ctx* ctx) { return ctx ? ctx->pl.last_doublings : 0; }

int sufr_hip_set_pair_walk(sufr_hip_ctx* ctx, uint32_t mode)
{
    if (!ctx) return SUFR_HIP_E_INVALID;
    if (mode > 2u) { ctx->pl.set_error("pair walk mode " + std::to_string(mode) + ": 0 (default), 1 (always) or 2 (never)"); return SUFR_HIP_E_INVALID; }
    ctx->pl.opt_pair_walk = mode;
    return 0;
}

int sufr_hip_pairs_walked(const sufr_hip_ctx* ctx, uint64_t* resolved, uint64_t* left_tied)
{
    if (!ctx) return SUFR_HIP_E_INVALID;
    if (resolved) *resolved = ctx->pl.last_pairs_resolved;
    if (left_tied) *left_tied = ctx->pl.last_pairs_left;
    return 0;
}

int sufr_hip_set_exc_max_affected(sufr_hip_ctx* ctx, uint64_t max_affected)
{
    if (!ctx) return SUFR_HIP_E_INVALID;
    if (max_affected > sufr::Pipeline::EXC_MAX_AFFECTED_DEFAULT) {
        ctx->pl.set_error("max_affected " + std::to_string(max_affected) + " > 2^22: the whole-text sort of the affected suffixes and its buffers are sized for 2^22");
        return SUFR_HIP_E_INVALID;
    }
    ctx->pl.opt_exc_max_affected = max_affected;
    return 0;
}

int sufr_hip_exc_retry(const sufr_hip_ctx* ctx) { return ctx ? (int)ctx->pl.last_exc_retry : 0; }
uint64_t sufr_hip_exc_taken(const sufr_hip_ctx* ctx) { return ctx ? ctx->pl.last_exc_taken : 0; }

int sufr_hip_synchronize(sufr_hip_ctx* ctx)
{
    if (!ctx) return SUFR_HIP_E_INVALID;
    if (hipSetDevice(ctx->pl.device) != hipSuccess || hipStreamSynchronize(ctx->pl.stream) != hipSuccess) {
        ctx->pl.set_error("hipStreamSynchronize failed");
        return SUFR_HIP_E_HIP;
    }
    return 0;
}

int sufr_hip_sort_device_u32(sufr_hip_ctx* ctx, const void* d_text, uint64_t n, uint32_t flags,
                             uint64_t max_query_len, const char* seed_mask, uint64_t num_partitions,
                             uint64_t random_seed, uint32_t shard_index, uint32_t num_shards, void* d_sa,
                             void* d_lcp, uint64_t cap, uint64_t* num_suffixes_out, sufr_hip_stats* stats)
{
    (void)num_partitions; (void)random_seed;
    if (!ctx) return SUFR_HIP_E_INVALID;
    ctx->pl.err.clear();
    int rc = take_options(ctx, max_query_len, seed_mask);
    if (rc) return rc;
    if (ctx->wide(n)) {
        if (n >= 0xFFFFFFFFull) { ctx->pl.set_error("text_len >= 2^32 - 1 takes the u64 entry points (suffix_array.rs:461)"); return SUFR_HIP_E_INVALID; }
        if (num_shards == 0 || shard_index >= num_shards) { ctx->pl.set_error("bad shard index"); return SUFR_HIP_E_INVALID; }
        // (round 5: a windowed build shards too -- every window keeps the suffixes of the shard's prefix range, the merge
        // runs per shard; sufr_wide.inc)
        ctx->pl.wide_shard_index = shard_index; ctx->pl.wide_num_shards = num_shards;
        rc = sufr::sort_device_wide<uint32_t>(ctx->pl, d_text, n, flags, ctx->wide_window, ctx->wide_margin, (uint32_t*)d_sa,
                                              (uint32_t*)d_lcp, cap, num_suffixes_out, stats, ctx->wtext, ctx->wsa, ctx->wlcp, ctx->wblk);
        ctx->pl.wide_shard_index = 0; ctx->pl.wide_num_shards = 1;
        return rc;
    }
    return ctx->pl.sort_device_u32(d_text, n, flags, shard_index, num_shards, (uint32_t*)d_sa, (uint32_t*)d_lcp,
                                   cap, num_suffixes_out, stats);
}

int sufr_hip_sort_device_u64(sufr_hip_ctx* ctx, const void* d_text, uint64_t n, uint32_t flags,
                             uint64_t max_query_len, const char* seed_mask, uint64_t num_partitions,
                             uint64_t random_seed, uint32_t shard_index, uint32_t num_shards, void* d_sa,
                             void* d_lcp, uint64_t cap, uint64_t* num_suffixes_out, sufr_hip_stats* stats)
{
    (void)num_partitions; (void)random_seed;
    if (!ctx) return SUFR_HIP_E_INVALID;
    ctx->pl.err.clear();
    int rc = take_options(ctx, max_query_len, seed_mask);
    if (rc) return rc;
    sufr::Pipeline& pl = ctx->pl;
    if (ctx->wide(n)) {
        if (num_shards == 0 || shard_index >= num_shards) { pl.set_error("bad shard index"); return SUFR_HIP_E_INVALID; }
        pl.wide_shard_index = shard_index; pl.wide_num_shards = num_shards;
        rc = sufr::sort_device_wide<uint64_t>(pl, d_text, n, flags, ctx->wide_window, ctx->wide_margin, (uint64_t*)d_sa,
                                              (uint64_t*)d_lcp, cap, num_suffixes_out, stats, ctx->wtext, ctx->wsa, ctx->wlcp, ctx->wblk);
        pl.wide_shard_index = 0; pl.wide_num_shards = 1;
        return rc;
    }
    if (hipSetDevice(pl.device) != hipSuccess) { pl.set_error("hipSetDevice failed"); return SUFR_HIP_E_HIP; }
    uint64_t cap32 = cap < n ? cap : n;
    if ((rc = pl.ensure(pl.sa32, cap32 * 4 + 4))) return rc;
    if ((rc = pl.ensure(pl.lcp32, cap32 * 4 + 4))) return rc;
    uint64_t s = 0;
    rc = pl.sort_device_u32(d_text, n, flags, shard_index, num_shards, (uint32_t*)pl.sa32.p, (uint32_t*)pl.lcp32.p,
                            cap32, &s, stats);
    if (num_suffixes_out) *num_suffixes_out = s;
    if (rc) return rc;
    if (s) {
        hipLaunchKernelGGL(sufr::k_widen, dim3((uint32_t)((s + 255) / 256)), dim3(256), 0, pl.stream,
                           (const uint32_t*)pl.sa32.p, (uint64_t*)d_sa, s);
        hipLaunchKernelGGL(sufr::k_widen, dim3((uint32_t)((s + 255) / 256)), dim3(256), 0, pl.stream,
                           (const uint32_t*)pl.lcp32.p, (uint64_t*)d_lcp, s);
        if (hipStreamSynchronize(pl.stream) != hipSuccess) { pl.set_error("widen failed"); return SUFR_HIP_E_HIP; }
    }
    return 0;
}

static int build_host(sufr_hip_ctx* ctx, int width, const uint8_t* text, uint64_t n, uint32_t flags,
                      uint64_t max_query_len, const char* seed_mask, uint8_t* norm_text_out, void* sa_out,
                      void* lcp_out, uint64_t cap, uint64_t* num_suffixes_out, sufr_hip_stats* stats)
{
    if (!ctx) return SUFR_HIP_E_INVALID;
    sufr::Pipeline& pl = ctx->pl;
    pl.err.clear();
    int rc = take_options(ctx, max_query_len, seed_mask);
    if (rc) return rc;
    if (num_suffixes_out) *num_suffixes_out = 0;
    if (n == 0) return 0;
    if (!text) { pl.set_error("null text"); return SUFR_HIP_E_INVALID; }
    if (hipSetDevice(pl.device) != hipSuccess) { pl.set_error("hipSetDevice failed"); return SUFR_HIP_E_HIP; }
    // stage the raw text at the far end of a scratch allocation; the pipeline normalises into pl.text
    void* d_raw = nullptr;
    if (hipMalloc(&d_raw, n + 64) != hipSuccess) { pl.set_error("hipMalloc(text) failed"); return SUFR_HIP_E_NOMEM; }
    auto fail = [&](int code, const char* what) { pl.set_error(what); (void)hipFree(d_raw); return code; };
    const auto t_start = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point a) { return std::chrono::duration<float>(std::chrono::steady_clock::now() - a).count(); };
    if (parallel_copy(pl.device, d_raw, text, n, false) != 0)
        return fail(SUFR_HIP_E_HIP, "H2D copy of the text failed");
    const float h2d_s = since(t_start);
    uint64_t cap_dev = cap < n ? cap : n;
    if (ctx->wide(n)) {
        // windowed build: the arrays come back at the caller's width; the normalised text is the windows' own copy
        if (width == 4 && n >= 0xFFFFFFFFull) return fail(SUFR_HIP_E_INVALID, "text_len >= 2^32 - 1 takes the u64 entry points");
        void *d_sa = nullptr, *d_lcp = nullptr;
        if (hipMalloc(&d_sa, cap_dev * (size_t)width + 16) != hipSuccess || hipMalloc(&d_lcp, cap_dev * (size_t)width + 16) != hipSuccess) {
            if (d_sa) (void)hipFree(d_sa);
            return fail(SUFR_HIP_E_NOMEM, "hipMalloc of the output arrays failed");
        }
        uint64_t s = 0;
        rc = width == 4
            ? sufr::sort_device_wide<uint32_t>(pl, d_raw, n, flags, ctx->wide_window, ctx->wide_margin, (uint32_t*)d_sa, (uint32_t*)d_lcp,
                                               cap_dev, &s, stats, ctx->wtext, ctx->wsa, ctx->wlcp, ctx->wblk)
            : sufr::sort_device_wide<uint64_t>(pl, d_raw, n, flags, ctx->wide_window, ctx->wide_margin, (uint64_t*)d_sa, (uint64_t*)d_lcp,
                                               cap_dev, &s, stats, ctx->wtext, ctx->wsa, ctx->wlcp, ctx->wblk);
        (void)hipFree(d_raw);
        if (num_suffixes_out) *num_suffixes_out = s;
        if (!rc && norm_text_out && parallel_copy(pl.device, norm_text_out, ctx->wtext.p, n, true) != 0) { pl.set_error("D2H copy of the normalised text failed"); rc = SUFR_HIP_E_HIP; }
        if (!rc && s && (parallel_copy(pl.device, sa_out, d_sa, s * (uint64_t)width, true) != 0 ||
                         parallel_copy(pl.device, lcp_out, d_lcp, s * (uint64_t)width, true) != 0)) { pl.set_error("D2H copy of SA/LCP failed"); rc = SUFR_HIP_E_HIP; }
        (void)hipFree(d_sa); (void)hipFree(d_lcp);
        return rc;
    }
    if ((rc = pl.ensure(pl.sa32, cap_dev * 4 + 4))) { (void)hipFree(d_raw); return rc; }
    if ((rc = pl.ensure(pl.lcp32, cap_dev * 4 + 4))) { (void)hipFree(d_raw); return rc; }
    uint64_t s = 0;
    const auto t_build = std::chrono::steady_clock::now();
    rc = pl.sort_device_u32(d_raw, n, flags, 0, 1, (uint32_t*)pl.sa32.p, (uint32_t*)pl.lcp32.p, cap_dev, &s, stats);
    (void)hipFree(d_raw);
    if (num_suffixes_out) *num_suffixes_out = s;
    if (rc) return rc;
    const float build_s = since(t_build);
    const auto t_out = std::chrono::steady_clock::now();
    struct Phases { sufr_hip_stats* st; float h2d, build; std::chrono::steady_clock::time_point t0;
                    ~Phases() { if (st) { st->host_read_s = h2d; st->host_build_s = build;
                                          st->host_write_s = std::chrono::duration<float>(std::chrono::steady_clock::now() - t0).count(); } } } phases{stats, h2d_s, build_s, t_out};
    if (width == 4) {
        // the three arrays as one list of pieces: no worker idles at the end of one array while another is still to be started
        CopyJob jobs[3]; int nj = 0;
        if (norm_text_out) jobs[nj++] = {norm_text_out, pl.text.p, n};
        if (s) { jobs[nj++] = {sa_out, pl.sa32.p, s * 4}; jobs[nj++] = {lcp_out, pl.lcp32.p, s * 4}; }
        if (parallel_copy_jobs(pl.device, jobs, nj, true) != 0) { pl.set_error("D2H copy of the text / SA / LCP failed"); return SUFR_HIP_E_HIP; }
    } else if (norm_text_out && parallel_copy(pl.device, norm_text_out, pl.text.p, n, true) != 0) {
        pl.set_error("D2H copy of the normalised text failed"); return SUFR_HIP_E_HIP;
    }
    if (s) {
        if (width == 4) {
        } else {
            std::vector<uint32_t> tmp(s);
            for (int which = 0; which < 2; which++) {
                if (hipMemcpyAsync(tmp.data(), which ? pl.lcp32.p : pl.sa32.p, s * 4, hipMemcpyDeviceToHost,
                                   pl.stream) != hipSuccess ||
                    hipStreamSynchronize(pl.stream) != hipSuccess) {
                    pl.set_error("D2H copy of SA/LCP failed"); return SUFR_HIP_E_HIP;
                }
                uint64_t* dst = (uint64_t*)(which ? lcp_out : sa_out);
                for (uint64_t i = 0; i < s; i++) dst[i] = tmp[i];
            }
        }
    }
    if (hipStreamSynchronize(pl.stream) != hipSuccess) { pl.set_error("stream sync failed"); return SUFR_HIP_E_HIP; }
    return 0;
}

// Internal (sufr_io.cpp): build shard `shard_index` of `num_shards` from a host text and leave the normalised
// text, SA and LCP in HBM.
int sufr_hip_build_resident_(sufr_hip_ctx* ctx, const uint8_t* text, uint64_t n, uint32_t flags,
                             uint64_t max_query_len, const char* seed_mask, uint32_t shard_index,
                             uint32_t num_shards, uint64_t* num_suffixes, sufr_hip_stats* stats, int* device,
                             const void** d_text, const void** d_sa, const void** d_lcp)
{
    if (!ctx) return SUFR_HIP_E_INVALID;
    sufr::Pipeline& pl = ctx->pl;
    pl.err.clear();
    int rc = take_options(ctx, max_query_len, seed_mask);
    if (rc) return rc;
    if (num_suffixes) *num_suffixes = 0;
    if (device) *device = pl.device;
    if (n == 0) { pl.set_error("empty text"); return SUFR_HIP_E_INVALID; }
    if (!text) { pl.set_error("null text"); return SUFR_HIP_E_INVALID; }
    if (n >= sufr::SUFR_MAX_TEXT_LEN) {             // before any allocation or copy
        pl.set_error("text_len >= 2^32 - 2^24: resident (sharded) builds take one 32-bit window; use the windowed single-GPU build");
        return SUFR_HIP_E_UNSUPPORTED;
    }
    if (hipSetDevice(pl.device) != hipSuccess) { pl.set_error("hipSetDevice failed"); return SUFR_HIP_E_HIP; }
    void* d_raw = nullptr;
    if (hipMalloc(&d_raw, n + 64) != hipSuccess) { pl.set_error("hipMalloc(text) failed"); return SUFR_HIP_E_NOMEM; }
    if (parallel_copy(pl.device, d_raw, text, n, false) != 0) {
        pl.set_error("H2D copy of the text failed"); (void)hipFree(d_raw); return SUFR_HIP_E_HIP;
    }
    // Output arrays of a shard: ~ s / num_shards entries, not n (N shards on one GPU would otherwise hold N full-size
    // pairs).  The exact count is known once the first-digit histogram is in (before any record is written): a
    // capacity that turns out too small comes back as E_CAPACITY with the count, and the build is repeated.
    uint64_t cap = num_shards > 1 ? n / num_shards + n / 64 + 4096 : n;
    if (cap > n) cap = n;
    uint64_t s = 0;
    for (int attempt = 0; attempt < 2; attempt++) {
        if ((rc = pl.ensure(pl.sa32, cap * 4 + 4)) || (rc = pl.ensure(pl.lcp32, cap * 4 + 4))) { (void)hipFree(d_raw); return rc; }
        rc = pl.sort_device_u32(d_raw, n, flags, shard_index, num_shards, (uint32_t*)pl.sa32.p, (uint32_t*)pl.lcp32.p, cap,
                                &s, stats);
        if (rc != SUFR_HIP_E_CAPACITY || s <= cap || s > n) break;
        cap = s;
        pl.err.clear();                              // (the first attempt's "output capacity" message is not this call's result)
    }
    (void)hipFree(d_raw);
    if (rc) return rc;
    if (num_suffixes) *num_suffixes = s;
    if (d_text) *d_text = pl.text.p;
    if (d_sa) *d_sa = pl.sa32.p;
    if (d_lcp) *d_lcp = pl.lcp32.p;
    return 0;
}

// Internal (sufr_io.cpp): the build-only arrays of the context go back to the device (the outputs stay).
void sufr_hip_release_build_arrays_(sufr_hip_ctx* ctx, int also_text) { if (ctx) ctx->pl.release_build_arrays(also_text != 0); }
// Internal (sufr_io.cpp, the retry of an out-of-core create): the rank arrays of the windows and the oversized 32-bit arrays of
// the last attempt (Pipeline::ensure never shrinks a buffer).
void sufr_hip_release_wide_arrays_(sufr_hip_ctx* ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->pl.device);
    (void)hipStreamSynchronize(ctx->pl.stream);
    sufr::DevBuf* all[] = {&ctx->wsa, &ctx->wlcp, &ctx->wblk, &ctx->pl.sa32, &ctx->pl.lcp32};
    for (auto* b : all) ctx->pl.release(*b);
    ctx->pl.release_build_arrays(false);
}

// Internal (sufr_io.cpp): where the last resident build left its arrays.
int sufr_hip_resident_arrays_(sufr_hip_ctx* ctx, int* device, const void** d_text, const void** d_sa, const void** d_lcp)
{
    if (!ctx) return SUFR_HIP_E_INVALID;
    sufr::Pipeline& pl = ctx->pl;
    if (!pl.text.p || !pl.sa32.p || !pl.lcp32.p) { pl.set_error("no resident build"); return SUFR_HIP_E_INVALID; }
    *device = pl.device; *d_text = pl.text.p; *d_sa = pl.sa32.p; *d_lcp = pl.lcp32.p;
    return 0;
}

// Internal (sufr_io.cpp): first and last suffix of the resident shard of s suffixes.
int sufr_hip_resident_ends_(sufr_hip_ctx* ctx, uint64_t s, uint64_t* first, uint64_t* last)
{
    if (!ctx || !s) return SUFR_HIP_E_INVALID;
    sufr::Pipeline& pl = ctx->pl;
    uint32_t f = 0, l = 0;
    if (hipSetDevice(pl.device) != hipSuccess ||
        hipMemcpy(&f, pl.sa32.p, 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&l, (const uint32_t*)pl.sa32.p + (s - 1), 4, hipMemcpyDeviceToHost) != hipSuccess) {
        pl.set_error("reading the shard's boundary suffixes failed");
        return SUFR_HIP_E_HIP;
    }
    *first = f; *last = l;
    return 0;
}

// Internal (sufr_io.cpp): LCP[0] of the resident shard := find_lcp(prev_last, SA[0], text_len, 0), the boundary
// fix of write() (sufr_builder.rs:893-902), computed on the device text.
int sufr_hip_resident_stitch_(sufr_hip_ctx* ctx, uint64_t n, uint64_t prev_last, uint64_t* lcp_out)
{
    if (!ctx) return SUFR_HIP_E_INVALID;
    sufr::Pipeline& pl = ctx->pl;
    uint32_t f = 0;
    unsigned long long v = 0;
    // (sufr_hip_shard_write releases the build's arrays -- and the text on ranks that do not write it -- when it is done: a
    // second call on the same context, e.g. a retry after ENOSPC, must end in an error code, not in a kernel on a null text)
    if (!pl.text.p || !pl.sa32.p || !pl.lcp32.p || n == 0 || pl.resident_text_len != n) {
        pl.set_error("stitch: the context holds no resident build of a text of this length (sufr_hip_shard_write releases it; "
                     "call sufr_hip_shard_build again)");
        return SUFR_HIP_E_INVALID;
    }
    if (hipSetDevice(pl.device) != hipSuccess ||
        hipMemcpy(&f, pl.sa32.p, 4, hipMemcpyDeviceToHost) != hipSuccess) { pl.set_error("stitch: read failed"); return SUFR_HIP_E_HIP; }
    hipLaunchKernelGGL(sufr::k_lcp_pair, dim3(1), dim3(256), 0, pl.stream, (const uint8_t*)pl.text.p, n, prev_last,
                       (uint64_t)f, pl.sc(sufr::Pipeline::SC_BAD), pl.stitch_order());
    if (hipMemcpyAsync(&v, pl.sc(sufr::Pipeline::SC_BAD), 8, hipMemcpyDeviceToHost, pl.stream) != hipSuccess ||
        hipStreamSynchronize(pl.stream) != hipSuccess) { pl.set_error("stitch: kernel failed"); return SUFR_HIP_E_HIP; }
    const uint32_t v32 = (uint32_t)v;
    if (hipMemcpy(pl.lcp32.p, &v32, 4, hipMemcpyHostToDevice) != hipSuccess) { pl.set_error("stitch: write failed"); return SUFR_HIP_E_HIP; }
    if (lcp_out) *lcp_out = v;
    return 0;
}

}  // extern "C"
template <typename LT>
static int stitch_device(sufr_hip_ctx* ctx, uint64_t n, const uint64_t* d_bounds, uint32_t shard_index, uint32_t num_shards, void* d_lcp)
{
    if (!ctx) return SUFR_HIP_E_INVALID;
    sufr::Pipeline& pl = ctx->pl;
    if (!d_bounds || !d_lcp || shard_index >= num_shards) { pl.set_error("stitch: bad arguments"); return SUFR_HIP_E_INVALID; }
    // the context's text must be the one the shard was built from: the length of its last build says so -- a one-window build
    // leaves the text in pl.text, a windowed one its normalised copy in ctx->wtext (and other bytes in pl.text)
    const uint8_t* text = nullptr;
    if (n != 0 && pl.text.p && n + sufr::TEXT_PAD <= pl.text.cap && pl.resident_text_len == n) text = (const uint8_t*)pl.text.p;
    else if (n != 0 && ctx->wtext.p && pl.wide_text_len == n) text = (const uint8_t*)ctx->wtext.p;
    if (!text) { pl.set_error("stitch: the context's last build was not a build of a text of this length"); return SUFR_HIP_E_INVALID; }
    if (hipSetDevice(pl.device) != hipSuccess) { pl.set_error("stitch: hipSetDevice failed"); return SUFR_HIP_E_HIP; }
    if (shard_index == 0) return 0;
    (void)hipGetLastError();          // (an allocation a build went without -- optional tables, a first try at a large buffer -- leaves its error behind)
    hipLaunchKernelGGL(sufr::k_lcp_stitch<LT>, dim3(1), dim3(256), 0, pl.stream, text, n,
                       (const unsigned long long*)d_bounds, shard_index, (LT*)d_lcp, pl.stitch_order());
    hipError_t he = hipGetLastError();
    if (he == hipSuccess) he = hipStreamSynchronize(pl.stream);
    if (he != hipSuccess) { pl.set_error(std::string("stitch: kernel failed: ") + hipGetErrorString(he)); return SUFR_HIP_E_HIP; }
    return 0;
}

extern "C" {
int sufr_hip_stitch_device_u32(sufr_hip_ctx* ctx, uint64_t n, const uint64_t* d_bounds, uint32_t shard_index,
                               uint32_t num_shards, void* d_lcp)
{
    return stitch_device<uint32_t>(ctx, n, d_bounds, shard_index, num_shards, d_lcp);
}

int sufr_hip_stitch_device_u64(sufr_hip_ctx* ctx, uint64_t n, const uint64_t* d_bounds, uint32_t shard_index,
                               uint32_t num_shards, void* d_lcp)
{
    return stitch_device<uint64_t>(ctx, n, d_bounds, shard_index, num_shards, d_lcp);
}

int sufr_hip_build_u32(sufr_hip_ctx* ctx, const uint8_t* text, uint64_t n, uint32_t flags,
                       uint64_t max_query_len, const char* seed_mask, uint64_t num_partitions,
                       uint64_t random_seed, uint8_t* norm_text_out, uint32_t* sa_out, uint32_t* lcp_out,
                       uint64_t cap, uint64_t* num_suffixes_out, sufr_hip_stats* stats)
{
    (void)num_partitions; (void)random_seed;
    return build_host(ctx, 4, text, n, flags, max_query_len, seed_mask, norm_text_out, sa_out, lcp_out, cap,
                      num_suffixes_out, stats);
}

int sufr_hip_build_u64(sufr_hip_ctx* ctx, const uint8_t* text, uint64_t n, uint32_t flags,
                       uint64_t max_query_len, const char* seed_mask, uint64_t num_partitions,
                       uint64_t random_seed, uint8_t* norm_text_out, uint64_t* sa_out, uint64_t* lcp_out,
                       uint64_t cap, uint64_t* num_suffixes_out, sufr_hip_stats* stats)
{
    (void)num_partitions; (void)random_seed;
    return build_host(ctx, 8, text, n, flags, max_query_len, seed_mask, norm_text_out, sa_out, lcp_out, cap,
                      num_suffixes_out, stats);
}

}  // extern "C"
