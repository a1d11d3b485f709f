// pg_api.cpp -- host side of the C ABI declared in include/pindel_pg.h.
// Owns the GPU context, packs the reference into bit planes, moves read batches
// to HBM, launches the search kernel (pg_kernels.hip) and turns its pooled runs
// back into per-read CSR results.  There is NO CPU implementation of the search
// here: without a working HIP device every entry point fails with PG_E_DEVICE.
// The device classifier's entries are pg_api_classify.cpp; what the two files share is pg_api_priv.h.
#include <hip/hip_runtime.h>

#include <cstddef>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "pg_api_priv.h"
#include "pg_device.h"
#include "pg_host_plan.h"
#include "pg_window_plan.h"
#include "pindel_pg.h"

#include <chrono>
#include <condition_variable>
#include <functional>
#include <exception>
#include <pthread.h>
namespace {

double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
const bool g_host_timing = getenv("PG_HOST_TIMING") != nullptr;

// The environment switches of tests and experiments, read ONCE (getenv on the 50 000-read flush path is a linear scan of the
// environment per call) -- pg_debug_reload_env() re-reads them (tests that change one in mid-process call it).  g_env is a plain
// object read without synchronisation by every caller's thread and by the host pool's workers: pg_debug_reload_env() is a TEST
// hook and must only be called while no pg_* call is in flight on any thread (pindel_pg.h says so; the tests do).
PgEnvSwitches g_env;
std::once_flag g_env_once;
void load_env()
{
    PgEnvSwitches e;
    const char *c = getenv("PG_HOST_CHUNK");                 // (tests: several chunks on a small batch)
    e.host_chunk = c ? (uint32_t)std::min<long>(std::max(1, atoi(c)), PG_DELIVER_CHUNK) : 0u;
    e.no_single_block = getenv("PG_NO_SINGLE_BLOCK") != nullptr;
    e.tiny_delivery = getenv("PG_TEST_TINY_DELIVERY") != nullptr;
    e.tiny_pool = getenv("PG_TEST_TINY_POOL") != nullptr;
    e.force_wide_cells = getenv("PG_FORCE_WIDE_CELLS") != nullptr;
    e.split_launch = getenv("PG_SPLIT_LAUNCH") != nullptr;
    e.generic_kernels = getenv("PG_GENERIC_KERNELS") != nullptr;
    e.lds_pad = getenv("PG_LDS_PAD") ? (uint32_t)atoi(getenv("PG_LDS_PAD")) : 0u;
    e.no_pack_in_place = getenv("PG_NO_PACK_IN_PLACE") != nullptr;
    e.pack_claim = getenv("PG_PACK_CLAIM") ? (uint32_t)std::max(1, atoi(getenv("PG_PACK_CLAIM"))) : 0u;
    e.pack_in_place_min = getenv("PG_PACK_IN_PLACE_MIN") ? (uint32_t)std::max(1, atoi(getenv("PG_PACK_IN_PLACE_MIN"))) : PG_PACK_IN_PLACE_MIN;
    e.no_fixed_len = getenv("PG_NO_FIXED_LEN") != nullptr;
    g_env = e;
}
const PgEnvSwitches &env()
{
    std::call_once(g_env_once, load_env);
    return g_env;
}

// Pinned host memory for results (device-to-host copies at PCIe speed, no staging through pageable pages).
// Pinning is expensive, results are handed out and freed all the time (Pindel flushes a batch every 50 000
// reads): freed blocks go to a small process-wide cache and are reused by the next result of similar size.
struct PinnedCache {
    std::mutex mu;
    std::vector<std::pair<void *, size_t>> free_blocks;
    size_t cached_bytes = 0;
    // page-locked memory kept for reuse: 6 GiB unless PG_PINNED_CACHE_MB says otherwise (0 = no caching)
    const size_t kMaxCached = getenv("PG_PINNED_CACHE_MB") ? (size_t)std::max(0L, atol(getenv("PG_PINNED_CACHE_MB"))) << 20 : (size_t)6 << 30;
    void *get(size_t bytes, size_t *got)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            size_t best = free_blocks.size();
            for (size_t i = 0; i < free_blocks.size(); i++)
                if (free_blocks[i].second >= bytes && free_blocks[i].second <= 2 * bytes + 4096 &&
                    (best == free_blocks.size() || free_blocks[i].second < free_blocks[best].second))
                    best = i;
            if (best != free_blocks.size()) {
                void *p = free_blocks[best].first;
                *got = free_blocks[best].second;
                cached_bytes -= *got;
                free_blocks.erase(free_blocks.begin() + best);
                return p;
            }
        }
        void *p = nullptr;
        const size_t want = (bytes + 4095) & ~(size_t)4095;
        // portable: a cached block may be reused by a context on another GPU
        if (hipHostMalloc(&p, want, hipHostMallocPortable) != hipSuccess) return nullptr;
        *got = want;
        return p;
    }
    void put(void *p, size_t bytes)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (cached_bytes + bytes <= kMaxCached) {
                free_blocks.push_back(std::make_pair(p, bytes));
                cached_bytes += bytes;
                return;
            }
        }
        (void)hipHostFree(p);
    }
    // releases every cached block (when the last context of the process goes away)
    void trim()
    {
        std::vector<std::pair<void *, size_t>> gone;
        {
            std::lock_guard<std::mutex> lk(mu);
            gone.swap(free_blocks);
            cached_bytes = 0;
        }
        for (auto &b : gone) (void)hipHostFree(b.first);
    }
};
PinnedCache g_pinned;
std::mutex g_ctx_mu;
int g_live_ctx = 0;

template <typename T>
struct HostBuf {
    T *p = nullptr;
    size_t n = 0, cap_bytes = 0;
    bool view = false;                // p points into another HostBuf's block (pg_result::block): nothing to give back
    HostBuf() {}
    HostBuf(const HostBuf &) = delete;
    HostBuf &operator=(const HostBuf &) = delete;
    ~HostBuf() { release(); }
    void release()
    {
        if (p && !view) g_pinned.put(p, cap_bytes);
        p = nullptr;
        n = cap_bytes = 0;
        view = false;
    }
    // count elements at `at` inside somebody else's pinned block (room for `room` elements: resize may shrink and regrow within it)
    void set_view(void *at, size_t count, size_t room)
    {
        release();
        p = (T *)at;
        n = count;
        cap_bytes = room * sizeof(T);
        view = true;
    }
    // contents are NOT initialised (they are about to be overwritten by a device-to-host copy)
    bool resize(size_t count)
    {
        if (count * sizeof(T) > cap_bytes) {
            release();
            p = (T *)g_pinned.get(std::max<size_t>(count * sizeof(T), 64), &cap_bytes);
            if (!p) return false;
        }
        n = count;
        return true;
    }
    bool assign(size_t count, T v)
    {
        if (!resize(count)) return false;
        for (size_t i = 0; i < count; i++) p[i] = v;
        return true;
    }
    T *data() { return p; }
    const T *data() const { return p; }
    size_t size() const { return n; }
    T &operator[](size_t i) { return p[i]; }
    const T &operator[](size_t i) const { return p[i]; }
    void swap(HostBuf &o)
    {
        std::swap(p, o.p);
        std::swap(n, o.n);
        std::swap(cap_bytes, o.cap_bytes);
        std::swap(view, o.view);
    }
};

}  // namespace

// The kernel keeps window bounds, anchor positions and candidate positions in signed 32-bit integers
// (pg_window, anchor_pos, `center`, `p`): a padded chromosome must stay below 2^31 with headroom for the
// guard/overhang arithmetic around a window end.
static const uint64_t PG_MAX_CHR_PADDED = 0x7fffffffull - 65536ull;

void log_launch(pg_ctx *ctx, const PgLaunchRec &r)
{
    if (!r.kernel) return;
    const uint32_t i = ctx->launch_n.fetch_add(1u, std::memory_order_relaxed);
    if (i < pg_ctx::PG_LAUNCH_LOG_CAP) ctx->launch_log[i] = r;
}

struct pg_result {
    uint32_t n = 0;
    // one-chunk results of the host path arrive in ONE device-to-host copy: this block; the arrays below are views into it.
    // Declared BEFORE them: members are destroyed in reverse order of declaration, so the views go first and the block is handed
    // back to the pinned cache (where another thread may take it at once) only after nothing points into it any more.
    HostBuf<uint8_t> block;
    HostBuf<uint64_t> close_off, far_off;
    HostBuf<pg_run> close_runs, far_runs;
    HostBuf<uint8_t> rc_flag;
    HostBuf<uint32_t> close_last;
    HostBuf<uint16_t> close_max;
};

namespace {

// probOfReadWithTheseErrors / createProbTable, src/pindel.cpp:781-819
double prob_of_read_with_these_errors(unsigned length, unsigned n_err, double rate)
{
    double chance_correct = 1.0 - rate;
    unsigned n_correct = length - n_err;
    double matched = pow(chance_correct, (double)n_correct);
    double mismatched = 1.0;
    for (unsigned i = 0; i < n_err; i++) mismatched *= (((length - i) * rate) / (n_err - i));
    return matched * mismatched;
}

void make_tables(pg_ctx *ctx)
{
    const double rate = 0.001 + ctx->prm.seq_error_rate;   // pindel.cpp:856
    for (unsigned length = 0; length < 500; length++) {
        double total = 0.0;
        ctx->mm[length] = 0;
        for (unsigned n_err = 0; n_err <= length; n_err++) {
            total += prob_of_read_with_these_errors(length, n_err, rate);
            if (total > ctx->prm.sensitivity) {
                ctx->mm[length] = n_err + 1;
                break;
            }
        }
    }
    ctx->mm[0] = ctx->mm[1] = ctx->mm[2] = ctx->mm[3] = 0;
    for (unsigned length = 500; length < 512; length++) ctx->mm[length] = ctx->mm[499];
    // CheckMismatches: (float)NumMismatches >= (float)(len * MaximumAllowedMismatchRate),
    // src/searcher.cpp:366,383 -> smallest integer that passes, per read length
    for (unsigned length = 0; length < 512; length++) {
        float max_allowed = (float)((double)(size_t)length * ctx->prm.max_allowed_mismatch_rate);
        unsigned n = 0;
        while (!((float)n >= max_allowed) && n < 65535) n++;
        ctx->thr[length] = (uint16_t)n;
    }
}

void free_reference(pg_ctx *ctx)
{
    ctx->ref_epoch++;
    if (ctx->d_lo) (void)hipFree(ctx->d_lo);
    if (ctx->d_hi) (void)hipFree(ctx->d_hi);
    if (ctx->d_nn) (void)hipFree(ctx->d_nn);
    if (ctx->d_word_off) (void)hipFree(ctx->d_word_off);
    if (ctx->d_chr_size) (void)hipFree(ctx->d_chr_size);
    ctx->d_lo = ctx->d_hi = ctx->d_nn = nullptr;
    ctx->d_word_off = nullptr;
    ctx->d_chr_size = nullptr;
    ctx->names.clear();
    ctx->comp_size.clear();
    ctx->word_off.clear();
    ctx->h_lo.clear();
    ctx->h_hi.clear();
    ctx->h_nn.clear();
    ctx->mirror_ok = false;
    ctx->plane_words = 0;
}

PgDevParams dev_params(const pg_ctx *ctx)
{
    PgDevParams p;
    p.max_range_index = ctx->prm.max_range_index;
    p.add_mm = ctx->prm.additional_mismatch;
    p.min_perfect = ctx->prm.min_perfect_match_around_bp;
    p.min_close = ctx->prm.min_close;
    p.spacer = ctx->prm.spacer;
    // breakpoints of the (monotone, checked in pg_create) g_maxMismatch table
    for (int k = 0; k < (int)PG_MM_BREAKS; k++) {
        p.mm_bp[k] = 0xffffffffu;
        for (unsigned L = 0; L < 500; L++)
            if (ctx->mm[L] >= (unsigned)(k + 1)) {
                p.mm_bp[k] = L;
                break;
            }
    }
    return p;
}

void free_batch_buffers(pg_device_batch *b)
{
    b->cls.release();
    if (b->in_arena) {
        if (b->pool_owned && b->pool) (void)hipFree(b->pool);
        if (b->bd_off) (void)hipFree(b->bd_off);          // window clusters are always allocated on their own
        if (b->bd) (void)hipFree(b->bd);
        b->pool = nullptr;
        b->bd_off = nullptr;
        b->bd = nullptr;
        return;
    }
    void *ptrs[] = { b->planes, b->seq, b->seq_off, b->strand, b->pos, b->isz, b->chr, b->rc_flag,
                     b->close_last, b->close_max, b->bd_off, b->bd, b->pool, b->pool_used, b->in_rec, b->out_rec, b->run_tot,
                     b->exact_list, b->exact_count, b->d_soa };
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
}

// fn(lo, hi) over [0, n) in contiguous ranges on a few host threads (one for small n).  The threads are a process-wide
// pool that sleeps between calls: spawning sixteen std::threads per pass cost more than the pass (0.25 ms of the 1.5 ms a
// 4 M-read pg_search_batch spent before its first copy).  One job at a time; a second caller (another context's host
// thread in pg_search_batch_multi) that finds the pool busy runs its ranges on threads of its own as before.
//   * re-entry: a range function that calls host_ranges() again on a pool thread (or on the caller's) finds t_in_pool set and
//     runs its ranges inline (try_lock on a mutex the thread already owns would be undefined behaviour);
//   * fork(): the child has the pool object but none of its threads; the pool lives behind a pointer and a pthread_atfork
//     child handler replaces it with a fresh one (the old object is leaked on purpose: joining threads that do not exist in
//     this process, or destroying mutexes another thread held at the fork, is not defined);
//   * a range function must not throw across threads: an exception on a worker is caught, the job completes, and the first
//     one is rethrown on the calling thread.
thread_local bool t_in_pool = false;
class HostPool {
public:
    ~HostPool()
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (std::thread &t : th_) t.join();
    }
    bool try_run(size_t n, unsigned nt, const std::function<void(size_t, size_t)> &fn)
    {
        if (t_in_pool) return false;                            // re-entry from a range function
        std::unique_lock<std::mutex> job(job_mu_, std::try_to_lock);
        if (!job.owns_lock()) return false;
        struct InPool { InPool() { t_in_pool = true; } ~InPool() { t_in_pool = false; } } in_pool;
        {
            std::lock_guard<std::mutex> lk(mu_);
            while (th_.size() + 1 < nt) {
                const unsigned id = (unsigned)th_.size() + 1;
                th_.emplace_back([this, id] { worker(id); });
            }
            fn_ = &fn;
            n_ = n;
            nt_ = nt;
            remaining_ = nt - 1;
            error_ = nullptr;
            gen_++;
        }
        cv_.notify_all();
        std::exception_ptr mine;
        try {
            fn((size_t)0, n / nt);                              // the caller takes the first range
        } catch (...) {
            mine = std::current_exception();
        }
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [this] { return remaining_ == 0; });
        fn_ = nullptr;
        std::exception_ptr err = mine ? mine : error_;
        error_ = nullptr;
        lk.unlock();
        if (err) std::rethrow_exception(err);
        return true;
    }
private:
    void worker(unsigned id)
    {
        unsigned seen = 0;
        for (;;) {
            const std::function<void(size_t, size_t)> *fn;
            size_t n;
            unsigned nt;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || (gen_ != seen && id < nt_); });
                if (stop_) return;
                seen = gen_;
                fn = fn_;
                n = n_;
                nt = nt_;
            }
            std::exception_ptr err;
            t_in_pool = true;
            try {
                (*fn)(n * id / nt, n * (id + 1) / nt);
            } catch (...) {
                err = std::current_exception();
            }
            std::lock_guard<std::mutex> lk(mu_);
            if (err && !error_) error_ = err;
            if (--remaining_ == 0) done_.notify_one();
        }
    }
    std::mutex job_mu_, mu_;
    std::condition_variable cv_, done_;
    std::vector<std::thread> th_;
    const std::function<void(size_t, size_t)> *fn_ = nullptr;
    size_t n_ = 0;
    unsigned nt_ = 0, remaining_ = 0, gen_ = 0;
    bool stop_ = false;
    std::exception_ptr error_;
};
HostPool *g_host_pool = nullptr;
std::once_flag g_host_pool_once;
HostPool &host_pool()
{
    std::call_once(g_host_pool_once, [] {
        g_host_pool = new HostPool();
        (void)pthread_atfork(nullptr, nullptr, [] { g_host_pool = new HostPool(); t_in_pool = false; });
        atexit([] { HostPool *p = g_host_pool; g_host_pool = nullptr; delete p; });
    });
    return *g_host_pool;
}

template <class Fn>
void host_ranges(size_t n, Fn fn)
{
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const unsigned nt = (unsigned)std::min<size_t>(std::min(hw, 16u), n >> 16);
    if (nt <= 1) {
        fn((size_t)0, n);
        return;
    }
    if (t_in_pool) {                                            // re-entry from a range function: inline, no nt x nt fan-out
        fn((size_t)0, n);
        return;
    }
    if (host_pool().try_run(n, nt, std::function<void(size_t, size_t)>(fn))) return;
    // the pool is busy with another caller's job: threads of this call's own, exceptions carried back like the pool's
    std::vector<std::thread> th;
    std::mutex err_mu;
    std::exception_ptr err;
    for (unsigned t = 0; t < nt; t++)
        th.emplace_back([&, t] {
            try {
                fn(n * t / nt, n * (t + 1) / nt);
            } catch (...) {
                std::lock_guard<std::mutex> lk(err_mu);
                if (!err) err = std::current_exception();
            }
        });
    for (std::thread &x : th) x.join();
    if (err) std::rethrow_exception(err);
}

// max_isz (nullable): largest insert size of the batch
// off_out (nullable, n + 1 entries): the read offsets rebased to 0, written in the same pass
// uniform_len (nullable): the one length all reads have, 0 when they differ (or there are none)
int batch_levels(pg_ctx *ctx, uint32_t ml, uint32_t *levels);
int validation_failure(pg_ctx *ctx, int code);
int validate_and_measure(pg_ctx *ctx, const pg_read_batch *reads, uint32_t *max_len, uint32_t *levels, int32_t *max_isz = nullptr,
                         uint64_t *off_out = nullptr, uint32_t *uniform_len = nullptr)
{
    if (!reads || (reads->n_reads && (!reads->seq_off || !reads->anchor_strand || !reads->anchor_pos ||
                                      !reads->insert_size || !reads->chr_id)))
        return fail(ctx, PG_E_INVALID, "null array in pg_read_batch");
    if (reads->n_reads && !reads->seq && reads->seq_off[reads->n_reads] > reads->seq_off[0])
        return fail(ctx, PG_E_INVALID, "null seq in pg_read_batch");
    if (ctx->names.empty()) return fail(ctx, PG_E_NO_REFERENCE, "no reference loaded");
    const int n_chr = (int)ctx->names.size();
    // per range: first problem found (0 = none; the lowest code wins, as in a sequential scan the first one would), longest read
    // ... and the one length of its reads (NO_LEN: no read yet, MIXED: more than one length)
    static constexpr uint64_t NO_LEN = ~0ull, MIXED = ~0ull - 1ull;
    struct Part {
        int code = 0; uint32_t ml = 1; int32_t isz = 0; uint64_t ul = NO_LEN;
        void see(uint64_t len) { ul = ul == NO_LEN || ul == len ? len : MIXED; }
    };
    std::mutex mu;
    Part all;
    size_t first_bad = (size_t)-1;
    const uint64_t base0 = reads->n_reads ? reads->seq_off[0] : 0;
    if (off_out) off_out[reads->n_reads] = reads->n_reads ? reads->seq_off[reads->n_reads] - base0 : 0;
    host_ranges(reads->n_reads, [&](size_t lo, size_t hi) {
        Part p;
        size_t bad = (size_t)-1;
        for (size_t i = lo; i < hi; i++) {
            int code = 0;
            if (off_out) off_out[i] = reads->seq_off[i] - base0;
            if (reads->seq_off[i + 1] < reads->seq_off[i]) code = 1;
            const uint64_t len = reads->seq_off[i + 1] - reads->seq_off[i];
            if (!code && len > PG_MAX_READ_LEN) code = 2;
            const int c = reads->chr_id[i];
            if (!code && (c < 0 || c >= n_chr)) code = 3;
            if (!code) {
                // the close-end windows (pindel.cpp:2272-2274, 2301-2302) must lie inside the padded string
                const long long apos = (long long)reads->anchor_pos[i] + ctx->prm.spacer;
                const long long isz = reads->insert_size[i];
                const long long wlo = apos - 2 * std::max<long long>(isz, 0) - 2, whi = apos + 2 * std::max<long long>(isz, 0) + 2;
                if (wlo < 0 || whi > (long long)ctx->comp_size[c]) code = 4;
            }
            if (code) {
                p.code = code;
                bad = i;
                break;
            }
            p.ml = std::max<uint32_t>(p.ml, (uint32_t)len);
            p.see(len);
            p.isz = std::max<int32_t>(p.isz, reads->insert_size[i]);
        }
        std::lock_guard<std::mutex> lk(mu);
        all.ml = std::max(all.ml, p.ml);
        all.isz = std::max(all.isz, p.isz);
        if (p.ul != NO_LEN) all.see(p.ul);
        if (p.code && bad < first_bad) {
            first_bad = bad;
            all.code = p.code;
        }
    });
    if (all.code) return validation_failure(ctx, all.code);
    const uint32_t ml = all.ml;
    *max_len = ml;
    if (max_isz) *max_isz = all.isz;
    if (uniform_len) *uniform_len = all.ul == NO_LEN || all.ul == MIXED ? 0u : (uint32_t)all.ul;
    return batch_levels(ctx, ml, levels);
}

// Reads per chunk of download() (PG_HOST_CHUNK: several chunks on a small batch), and the bytes of its device temporaries but
// the gathered runs: per-read sums, 64-bit offsets (2 lists), per-block sums (one slice of blocks per chunk), 64 B of info per chunk
static size_t download_chunk() { return env().host_chunk ? env().host_chunk : PG_DELIVER_CHUNK; }
static size_t download_scratch_bytes(size_t n)
{
    const size_t chunk = download_chunk(), n_chunks = (n + chunk - 1) / chunk;
    return 3 * n * 8 + n_chunks * ((chunk + 255) / 256) * 8 + n_chunks * 64 + 5 * 512;
}

PgSoaIn soa_in(const pg_ctx *ctx, const pg_device_batch *b);

// What the allocation needs to know about a validated batch: measured on host threads (validate_and_measure) or by the
// measurement kernel of pg_device_batch_upload_device.
struct BatchMeasure {
    uint32_t n = 0, max_len = 1, levels = 0, uniform_len = 0;
    int32_t max_isz = 0;
    uint64_t nseq = 0;                 // bases of the batch: seq_off[n] - seq_off[0]
};

// The mismatch levels a batch whose longest read has max_len bases needs (PG_E_UNSUPPORTED beyond PG_MAX_LEVELS).
int batch_levels(pg_ctx *ctx, uint32_t ml, uint32_t *levels)
{
    uint32_t lv = ctx->mm[ml] + (uint32_t)ctx->prm.additional_mismatch + 1;
    for (uint32_t l = 0; l <= ml; l++)
        lv = std::max<uint32_t>(lv, ctx->mm[l] + (uint32_t)ctx->prm.additional_mismatch + 1);
    if (lv > PG_MAX_LEVELS) return fail(ctx, PG_E_UNSUPPORTED, "more than 32 mismatch levels");
    *levels = lv;
    return PG_OK;
}

// The text and status of a validation code (validate_and_measure and its device twin report the same ones).
int validation_failure(pg_ctx *ctx, int code)
{
    switch (code) {
    case 1: return fail(ctx, PG_E_INVALID, "seq_off not monotone");
    case 2: return fail(ctx, PG_E_READ_TOO_LONG, "read longer than 499 bases");
    case 3: return fail(ctx, PG_E_INVALID, "chr_id out of range");
    case 4: return fail(ctx, PG_E_INVALID, "anchor position/insert size reach outside the padded chromosome");
    default: return PG_OK;
    }
}

// Allocates the device buffers of a measured batch: the one item table of both upload entries.  No input is copied here.
// seq_off_ready (hipMalloc'd batches only): the batch's seq_off buffer, already allocated and filled (the measurement kernel of
// the device upload writes the rebased offsets straight into it); the batch takes it over, also when this call fails.
int alloc_batch_buffers(pg_ctx *ctx, const BatchMeasure &m, pg_device_batch **out, bool use_arena, const PgHostPlan *plan,
                        uint64_t *seq_off_ready = nullptr)
{
    pg_device_batch *b = new pg_device_batch();
    b->n = m.n;
    // the batch is bound to the reference it was VALIDATED against (anchor windows, chromosome ids): stamped here and nowhere else --
    // a repack or a new set of windows after a reload of the reference is refused, not re-stamped (stale_batch)
    b->ref_epoch = ctx->ref_epoch;
    b->max_len = m.max_len;
    b->uniform_len = m.uniform_len;
    b->levels = m.levels;
    b->max_isz = m.max_isz;
    b->seq_off = seq_off_ready;
    const uint32_t max_len = m.max_len;
    const size_t n = b->n;
    const uint64_t nseq = m.nseq;
    // every read reserves PG_RESERVE slots (one atomic per claim of reads); lists longer than their share allocate more
    b->pool_shard_cap = (uint32_t)std::min<uint64_t>(((PG_RESERVE + 2ull) * n) / PG_POOL_SHARDS + 512ull, 0x7fffffffull / PG_POOL_SHARDS);
    if (env().tiny_pool) b->pool_shard_cap = 1;      // tests: force the overflow/regrow path
    const size_t n1 = std::max<size_t>(n, 1);
    const PgInputLayout in = pg_input_layout(n);
    // (pointer, bytes) of every buffer; the zeroed block (outputs) is contiguous in the arena case
    struct Item { void **p; size_t bytes; };
    const Item items[] = {
        { (void **)&b->seq, (size_t)nseq + 16 },
        // the five small inputs, one after the other: in the arena they lie as PgInputLayout says (the one-copy upload)
        { (void **)&b->seq_off, in.a[PG_IN_SEQ_OFF].bytes }, { (void **)&b->strand, in.a[PG_IN_STRAND].bytes },
        { (void **)&b->pos, in.a[PG_IN_POS].bytes }, { (void **)&b->isz, in.a[PG_IN_ISZ].bytes }, { (void **)&b->chr, in.a[PG_IN_CHR].bytes },
        // INVARIANT: every allocation of in_rec carries PG_IN_PAD records behind the last read -- search_read touches `rp + 1` with a
        // scalar load whose value is discarded (the next read's record into the scalar cache); this is the only place in_rec is
        // allocated, and a launch over a sub-range [lo, lo + cnt) of the batch touches at most record lo + cnt, which exists.
        { (void **)&b->in_rec, (n1 + PG_IN_PAD) * sizeof(PgInRec) },
        { (void **)&b->planes, n1 * 64 * pg_plane_blocks(max_len) },
        { (void **)&b->exact_list, n1 * 4 },
        { (void **)&b->d_soa, sizeof(PgSoaIn) },
        { (void **)&b->pool, (size_t)b->pool_shard_cap * PG_POOL_SHARDS * sizeof(pg_run) },
        // ---- zero-initialised from here
        { (void **)&b->rc_flag, n1 }, { (void **)&b->close_last, n1 * 4 }, { (void **)&b->close_max, n1 * 2 },
        { (void **)&b->out_rec, n1 * sizeof(PgOutRec) },
        // run-pool cursors, then per set of read counters (two: launches on the two kernel streams overlap) the counters and the
        // cycle accumulators of a -DPG_TIMING diagnostics build, which the kernel finds right behind its counters
        { (void **)&b->pool_used, (PG_POOL_SHARDS * 16 + 2 * (PG_WORK_CTRS * 16 + PG_DIAG_WORDS * 2)) * 4 },   // + a second set of read counters
        { (void **)&b->run_tot, 64 },
        { (void **)&b->exact_count, 64 },
    };
    const size_t n_items = sizeof items / sizeof items[0];
    size_t first_zero = 0;             // the zeroed block starts at rc_flag
    while (items[first_zero].p != (void **)&b->rc_flag) first_zero++;
    auto drop = [&](int code) {
        free_batch_buffers(b);
        delete b;
        return code;
    };
    if (use_arena) {
        size_t need = 4096;
        for (const Item &it : items) need += pg_arena_room(it.bytes);
        // room for the download's temporaries too: gathered runs (no more than the pool holds) and the rest
        need += (size_t)b->pool_shard_cap * PG_POOL_SHARDS * sizeof(pg_run) + download_scratch_bytes(n) + 4096;
        // ... and for the chunk-by-chunk delivery of search_host
        if (plan) need += plan->arena_bytes;
        if (need > ctx->arena.cap) {
            if (ctx->arena.base) (void)hipFree(ctx->arena.base);
            ctx->arena.base = nullptr;
            ctx->arena.cap = 0;
            const size_t want = need + need / 4;
            hipError_t e = hipMalloc((void **)&ctx->arena.base, want);
            if (e != hipSuccess) {
                delete b;
                return fail(ctx, PG_E_NOMEM, std::string("device arena: ") + hipGetErrorString(e));
            }
            ctx->arena.cap = want;
        }
        ctx->arena.used = 0;
        b->in_arena = true;
        for (const Item &it : items) *it.p = ctx->arena.take(it.bytes);
        if ((size_t)((char *)b->chr - (char *)b->seq_off) != in.a[PG_IN_CHR].off) return drop(fail(ctx, PG_E_DEVICE, "the batch inputs do not lie as PgInputLayout says"));
        char *z0 = (char *)*items[first_zero].p;
        char *z1 = (char *)*items[n_items - 1].p + items[n_items - 1].bytes;
        hipError_t e = hipMemsetAsync(z0, 0, (size_t)(z1 - z0), ctx->stream);
        if (e != hipSuccess) return drop(fail(ctx, PG_E_DEVICE, std::string("clearing the batch outputs: ") + hipGetErrorString(e)));
    } else {
        for (size_t k = 0; k < n_items; k++) {
            if (*items[k].p) continue;                    // (seq_off_ready)
            hipError_t e = hipMalloc(items[k].p, items[k].bytes);
            // the delivery's scan / gather trusts the counts: a failed memset must not go unnoticed
            if (e == hipSuccess && k >= first_zero) e = hipMemset(*items[k].p, 0, items[k].bytes);
            if (e != hipSuccess)
                return drop(fail(ctx, e == hipErrorOutOfMemory ? PG_E_NOMEM : PG_E_DEVICE,
                                 std::string("batch buffers: ") + hipGetErrorString(e)));
        }
    }
    *out = b;
    return PG_OK;
}

// Copies the inputs of a batch into its buffers, all with blocking copies of `kind`: from host arrays (off = the offsets rebased
// to 0) or from the caller's device arrays (off = null: the measurement kernel has written the batch's seq_off already).
// seq points at the batch's first base.
int copy_batch_inputs(pg_ctx *ctx, pg_device_batch *b, const pg_read_batch *reads, const uint8_t *seq, uint64_t nseq,
                      const uint64_t *off, hipMemcpyKind kind)
{
    const size_t n = b->n;
    if (!n) return PG_OK;
    hipError_t e = hipSuccess;
    if (nseq) e = hipMemcpy(b->seq, seq, (size_t)nseq, kind);
    if (e == hipSuccess && off) e = hipMemcpy(b->seq_off, off, (n + 1) * sizeof(uint64_t), kind);
    if (e == hipSuccess) e = hipMemcpy(b->strand, reads->anchor_strand, n, kind);
    if (e == hipSuccess) e = hipMemcpy(b->pos, reads->anchor_pos, n * sizeof(int32_t), kind);
    if (e == hipSuccess) e = hipMemcpy(b->isz, reads->insert_size, n * sizeof(int16_t), kind);
    if (e == hipSuccess) e = hipMemcpy(b->chr, reads->chr_id, n * sizeof(int32_t), kind);
    // (a device-to-device copy may return before it has run: the caller may release its buffers when the entry returns)
    if (e == hipSuccess && kind == hipMemcpyDeviceToDevice) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) return fail(ctx, PG_E_DEVICE, std::string("input upload: ") + hipGetErrorString(e));
    return PG_OK;
}

// The pack's view of the inputs for launches that pack in place (launch_range replaces it when the windows or the parameters
// change); on the ctx stream, which every launch of the batch is ordered behind.
int publish_soa(pg_ctx *ctx, pg_device_batch *b)
{
    b->h_soa = soa_in(ctx, b);
    hipError_t e = hipMemcpyAsync(b->d_soa, &b->h_soa, sizeof b->h_soa, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) return fail(ctx, PG_E_DEVICE, std::string("input upload: ") + hipGetErrorString(e));
    b->soa_uploaded = true;
    return PG_OK;
}

// Validates the batch and allocates its device buffers.  copy = true also copies the inputs
// (synchronously); otherwise the caller streams them in (search_host).  off = read offsets rebased to 0.
// use_arena: carve the buffers out of the ctx arena (host-path calls: the batch dies with the call).
// plan (search_host; needs use_arena): the arena gets room for the delivery buffers the caller takes behind the batch, and
// `off` room for the one-copy upload (pg_host_plan.h).
int alloc_batch(pg_ctx *ctx, const pg_read_batch *reads, bool copy, HostBuf<uint64_t> &off, pg_device_batch **out,
                bool use_arena = false, const PgHostPlan *plan = nullptr)
{
    BatchMeasure m;
    if (!off.resize(plan ? plan->off_words : (reads ? reads->n_reads : 0) + (size_t)1)) return fail(ctx, PG_E_NOMEM, "host memory for the read offsets");
    int rc = validate_and_measure(ctx, reads, &m.max_len, &m.levels, &m.max_isz, off.data(), &m.uniform_len);
    if (rc) return rc;
    m.n = reads->n_reads;
    const uint64_t base0 = m.n ? reads->seq_off[0] : 0;
    m.nseq = m.n ? reads->seq_off[m.n] - base0 : 0;
    pg_device_batch *b = nullptr;
    if ((rc = alloc_batch_buffers(ctx, m, &b, use_arena, plan))) return rc;
    if (copy) rc = copy_batch_inputs(ctx, b, reads, m.nseq ? reads->seq + base0 : nullptr, m.nseq, off.data(), hipMemcpyHostToDevice);
    if (!rc) rc = publish_soa(ctx, b);
    if (rc) {
        free_batch_buffers(b);
        delete b;
        return rc;
    }
    *out = b;
    return PG_OK;
}

PgSoaIn soa_in(const pg_ctx *ctx, const pg_device_batch *b)
{
    PgSoaIn a;
    std::memset(&a, 0, sizeof a);      // (compared bytewise by launch_range)
    a.seq = b->seq;
    a.planes = b->planes;
    a.plane_blocks = pg_plane_blocks(b->max_len);
    a.seq_off = b->seq_off;
    a.strand = b->strand;
    a.pos = b->pos;
    a.isz = b->isz;
    a.chr = b->chr;
    a.bd_off = b->bd_off;
    a.exact_list = b->exact_list;
    a.exact_count = b->exact_count;
    a.len_tab = ctx->d_len_tab;
    a.chr_word_off = ctx->d_word_off;
    a.chr_size = ctx->d_chr_size;
    a.spacer = ctx->prm.spacer;
    a.add_mm = ctx->prm.additional_mismatch;
    a.min_close = ctx->prm.min_close;
    return a;
}

PgSoaOut soa_out(const pg_device_batch *b)
{
    PgSoaOut a;
    a.rc_flag = b->rc_flag;
    a.close_last = b->close_last;
    a.close_max = b->close_max;
    return a;
}

// The length of the exact kernel's list, once the batch's pack has finished (synchronous entries only: a device-resident batch is
// searched many times, and every search would otherwise carry a launch that finds nothing to do).
int read_exact_count(pg_ctx *ctx, pg_device_batch *b)
{
    uint32_t n = 0;
    if (b->n) {
        HIP_TRY(ctx, hipMemcpyAsync(&n, b->exact_count, sizeof n, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    b->exact_n = n;
    return PG_OK;
}

// Builds the packed records of reads [lo, lo + cnt) from the SoA inputs (on the ctx stream).
int pack_reads(pg_ctx *ctx, pg_device_batch *b, uint32_t lo, uint32_t cnt, hipStream_t st = nullptr)
{
    const PgSoaIn a = soa_in(ctx, b);
    if (lo == 0 && cnt == b->n && b->n) {       // the whole batch (again): the exact kernel's list starts empty
        HIP_TRY(ctx, hipMemsetAsync(b->exact_count, 0, sizeof(uint32_t), st ? st : ctx->stream));
        b->exact_n = -1;
    }
    PgLaunchRec rec;
    int rc = pg_pack_reads(&a, b->in_rec, lo, cnt, st ? st : ctx->stream, &rec);
    if (rc) return fail(ctx, PG_E_DEVICE, std::string("pack kernel: ") + hipGetErrorString((hipError_t)rc));
    log_launch(ctx, rec);
    return PG_OK;
}

int upload_batch(pg_ctx *ctx, const pg_read_batch *reads, pg_device_batch **out)
{
    // (pinned, from the cache: as a malloc'd array the runtime locks its pages for the copy and the free() of 80 MB after a
    // 10 M-read call spent 13 ms in munmap + unpinning)
    HostBuf<uint64_t> off;
    int rc = alloc_batch(ctx, reads, true, off, out);
    if (rc) return rc;
    if ((rc = pack_reads(ctx, *out, 0, (*out)->n))) {
        free_batch_buffers(*out);
        delete *out;
        *out = nullptr;
    }
    return rc;
}

PgDevBatch dev_batch(const pg_device_batch *b)
{
    PgDevBatch d;
    d.n_reads = b->n;
    d.first_read = 0;
    d.in = b->in_rec;
    d.out = b->out_rec;
    d.seq = b->seq;
    d.planes = b->planes;
    d.plane_blocks = pg_plane_blocks(b->max_len);
    d.bd = b->bd_off ? b->bd : nullptr;
    d.pool = b->pool;
    d.pool_shard_cap = b->pool_shard_cap;
    d.pool_used = b->pool_used;
    d.work_ctr = b->pool_used + PG_POOL_SHARDS * 16;
    d.claim = PG_CLAIM;       // (pg_launch_search sets it from the launch's grid)
    d.exact_list = b->exact_list;
    d.exact_count = b->exact_count;
    d.thr_tab = nullptr;               // (launch_range: the ctx's table)
    d.soa = nullptr;                   // (launch_range: a launch that packs in place)
    return d;
}

bool small_ids(const pg_ctx *ctx, const pg_device_batch *b)
{
    // 32-bit candidate ids when every window of this launch has <= 2^24 positions: ranges 128 * 4^x
    // (x <= 8), close windows 3 * InsertSize (a short), BreakDancer windows as attached
    return ctx->prm.max_range_index <= 8 && (long long)b->max_bd_window <= PG_SMALL_MAX_WINDOW &&
           b->max_bd_cluster <= PG_SMALL_MAX_CLUSTER && !env().force_wide_cells;
}

// Launches the search for reads [lo, lo + cnt) of the batch on the ctx stream.
// st / set: the stream to launch on and the set of read counters to use (launches that may overlap need their own)
// fresh: the set's counters are still zero from the batch's allocation (the first launch on each set)
// pack: the records of the range are (re)built from the batch's SoA inputs first -- by the search kernel itself where that is
// possible (pg_pack_in_place_ok: PgDevBatch::soa), by a pack launch in front of it otherwise
int launch_range(pg_ctx *ctx, pg_device_batch *b, int mode, uint32_t lo, uint32_t cnt, hipStream_t st = nullptr, int set = 0,
                 bool fresh = false, bool pack = false)
{
    PgDevRef ref = dev_ref(ctx);
    PgDevParams prm = dev_params(ctx);
    PgDevBatch d = dev_batch(b);
    d.first_read = lo;
    d.n_reads = cnt;
    if (!st) st = ctx->stream;
    // the persistent launch claims its reads from these counters (set 1 lies behind set 0 and the diagnostics words)
    size_t bytes = (PG_WORK_CTRS * 16 + PG_DIAG_WORDS * 2) * sizeof(uint32_t);
    if (set) {
        d.work_ctr += PG_WORK_CTRS * 16 + PG_DIAG_WORDS * 2;
        bytes = PG_WORK_CTRS * 16 * sizeof(uint32_t);
    }
    if (!ctx->kargs_checked) {
        // once per context: the kernels fetch their arguments from the kernarg segment at offsets of their own (KA() in
        // pg_kernels.hip); a one-wave kernel with the same parameter list compares them with the by-value arguments
        const int bad = pg_debug_kargs_check(&ref, &prm, &d, b->max_len, b->levels, d.work_ctr + PG_WORK_CTRS * 16, st);
        if (bad != 0) return fail(ctx, PG_E_DEVICE, "kernel arguments: the kernarg segment is not laid out as the kernels expect (" + std::to_string(bad) + ")");
        ctx->kargs_checked = true;
    }
    if (!fresh) HIP_TRY(ctx, hipMemsetAsync(d.work_ctr, 0, bytes, st));
    d.thr_tab = ctx->d_thr;
    if (pack && cnt) {
        if (pg_pack_in_place_ok(mode, b->max_len, small_ids(ctx, b) ? 1 : 0, cnt, d.plane_blocks)) {
            const PgSoaIn a = soa_in(ctx, b);
            if (std::memcmp(&a, &b->h_soa, sizeof a) != 0 || !b->soa_uploaded) {     // (the parameters or the windows changed)
                // (launches that overlap on the two kernel streams read the same copy: wait for them before it is replaced)
                if (b->soa_uploaded) HIP_TRY(ctx, hipDeviceSynchronize());
                b->h_soa = a;
                // (blocking: the chunks of the host path alternate between two kernel streams, and every one of them reads this copy)
                HIP_TRY(ctx, hipMemcpy(b->d_soa, &b->h_soa, sizeof a, hipMemcpyHostToDevice));
                b->soa_uploaded = true;
            }
            if (lo == 0 && cnt == b->n) {                 // the whole batch (again): the exact kernel's list starts empty
                HIP_TRY(ctx, hipMemsetAsync(b->exact_count, 0, sizeof(uint32_t), st));
                b->exact_n = -1;
            }
            d.soa = b->d_soa;
        } else if (int rc = pack_reads(ctx, b, lo, cnt, st))
            return rc;
        ctx->last_in_place = d.soa != nullptr;
    }
    PgLaunchRec recs[PG_LAUNCH_RECS_MAX];
    int n_recs = 0;
    // (a batch of one read length under the baked length tables: the launch may run that length's kernel)
    uint32_t fixed_len = 0;
    int lrc = pg_launch_search(&ref, &prm, &d, mode, b->max_len, b->levels, small_ids(ctx, b) ? 1 : 0, st, recs, &n_recs,
                               ctx->fixed_ok ? b->uniform_len : 0u, &fixed_len);
    ctx->last_fixed_len.store(fixed_len, std::memory_order_relaxed);
    if (lrc != 0) return fail(ctx, PG_E_DEVICE, std::string("kernel launch: ") + hipGetErrorString((hipError_t)lrc));
    for (int k = 0; k < n_recs; k++) log_launch(ctx, recs[k]);
    // ... then, behind it on the same stream, the reads of this range that hold a character outside ACGTN, with the reference's
    // read-shortening semantics (setUnmatchedSeq, pindel.cpp:142-169, 2545): a 64-workgroup launch that finds its list empty for
    // every batch a sequencer produced -- skipped when the host has read the list's length and it is zero
    if (b->exact_n != 0) {
        lrc = pg_launch_search_exact(&ref, &prm, &d, mode, b->max_len, b->levels, st, &recs[0]);
        if (lrc != 0) return fail(ctx, PG_E_DEVICE, std::string("exact kernel launch: ") + hipGetErrorString((hipError_t)lrc));
        log_launch(ctx, recs[0]);
    }
    return PG_OK;
}

// After the launches of a search: total runs, and whether a pool shard overflowed (worst > capacity).
int read_cursors(pg_ctx *ctx, pg_device_batch *b, uint32_t *worst, uint64_t *total)
{
    std::vector<uint32_t> cursors(PG_POOL_SHARDS * 16);
    HIP_TRY(ctx, hipMemcpy(cursors.data(), b->pool_used, cursors.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *worst = 0;
    *total = 0;
    for (uint32_t s = 0; s < PG_POOL_SHARDS; s++) {
        *worst = std::max(*worst, cursors[s * 16]);
        *total += cursors[s * 16];
    }
    return PG_OK;
}

// What every search refuses before anything is launched.
int search_refusals(pg_ctx *ctx, const pg_device_batch *b)
{
    if (ctx->names.empty()) return fail(ctx, PG_E_NO_REFERENCE, "no reference loaded");
    // (a batch is validated and its records are packed against the reference loaded at upload time: chromosome offsets and sizes,
    // window bounds; a reference loaded later makes them stale)
    return stale_batch(ctx, b);
}

// One launch of `mode` over the whole batch, waited for: its runs go behind whatever the pool cursors say is there (the caller
// zeroes them, or not), and `searched` is the caller's to set.  *ms: the HIP-event time; *worst / *total: the cursors afterwards.
int search_launch(pg_ctx *ctx, pg_device_batch *b, int mode, bool pack, float *ms, uint32_t *worst, uint64_t *total)
{
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    int rc = launch_range(ctx, b, mode, 0, b->n, nullptr, 0, false, pack);
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
    return read_cursors(ctx, b, worst, total);
}

// A larger pool, of `want` slots per shard (at most what 31-bit slot numbers reach).  The runs of the old one are gone.
int grow_pool(pg_ctx *ctx, pg_device_batch *b, uint64_t want)
{
    const uint32_t ncap = (uint32_t)std::min<uint64_t>(want, 0x7fffffffull / PG_POOL_SHARDS);
    pg_run *npool = nullptr;
    int rc = dev_alloc(ctx, &npool, (size_t)ncap * PG_POOL_SHARDS);
    if (rc) return rc;
    if (!b->in_arena || b->pool_owned) (void)hipFree(b->pool);
    b->pool = npool;
    b->pool_owned = true;
    b->pool_shard_cap = ncap;
    return PG_OK;
}

// Runs the kernel(s) of `mode`; if a pool shard overflowed, the pool is regrown and the launch
// repeated (still entirely on the GPU).
int run_search(pg_ctx *ctx, pg_device_batch *b, int mode, bool pack = false)
{
    if (int rc = search_refusals(ctx, b)) return rc;
    b->cls.drop_search_tables();
    for (int attempt = 0; attempt < 8; attempt++) {
        HIP_TRY(ctx, hipMemsetAsync(b->pool_used, 0, PG_POOL_SHARDS * 16 * sizeof(uint32_t), ctx->stream));
        float ms = 0.f;
        uint32_t worst = 0;
        uint64_t total = 0;
        int rc = search_launch(ctx, b, mode, pack, &ms, &worst, &total);
        if (rc) return rc;
        if (worst <= b->pool_shard_cap) {
            ctx->last_ms = ms;
            ctx->last_runs = total;
            if (mode == PG_MODE_BOTH) b->searched = b->close_searched = true;
            return PG_OK;
        }
        // overflow: grow the pool and redo the launch
        if ((rc = grow_pool(ctx, b, (uint64_t)worst + worst / 4 + 64))) return rc;
    }
    return fail(ctx, PG_E_DEVICE, "run pool kept overflowing");
}

// The two passes of a whole-batch delivery (n > 0), shared by the download to the host and the one into the caller's device
// buffers: the delivery kernels of the host path (pg_deliver_chunk) over the whole batch.  Pass 1 scans every chunk -- per-read
// summaries into the batch's own arrays, local sums, each chunk's base and run counts -- and brings the per-chunk info to the host,
// which sizes (or checks) the run buffers from the totals; pass 2 gathers the runs in read order and writes the 64-bit offsets,
// straight into whatever device buffers the caller names.  Each pass is queued on the ctx stream and waited for separately, so
// that the caller's own copies travel in between.
struct DeliveryPasses {
    pg_ctx *ctx;
    pg_device_batch *b;
    const size_t n, chunk, n_chunks, chunk_blks;
    DevTemps tmp;
    uint2 *local = nullptr, *blk = nullptr;
    unsigned long long *d_info = nullptr;
    HostBuf<unsigned long long> info;
    unsigned long long tot[2] = { 0, 0 };                  // close / far runs of the batch (wait_totals)
    DeliveryPasses(pg_ctx *c, pg_device_batch *batch)
        : ctx(c), b(batch), n(batch->n), chunk(download_chunk()), n_chunks((n + chunk - 1) / chunk), chunk_blks((chunk + 255) / 256),
          tmp(c, batch) {}
    const unsigned long long *d_last_info() const { return d_info + 8 * (n_chunks - 1); }
    int queue_scan()
    {
        local = (uint2 *)tmp.take(n * 8);
        blk = (uint2 *)tmp.take(n_chunks * chunk_blks * 8);
        d_info = (unsigned long long *)tmp.take(n_chunks * 64);
        if (!local || !blk || !d_info) return fail(ctx, PG_E_NOMEM, "device memory for the download's scans");
        if (!info.resize(n_chunks * 8)) return fail(ctx, PG_E_NOMEM, "pinned host memory");
        // (search_host's fallback: its deliveries have advanced the running totals)
        HIP_TRY(ctx, hipMemsetAsync(b->run_tot, 0, 2 * sizeof(unsigned long long), ctx->stream));
        for (size_t k = 0, lo = 0; k < n_chunks; k++, lo += chunk)
            HIP_TRY(ctx, (hipError_t)pg_deliver_scan(b->out_rec + lo, (uint32_t)std::min(chunk, n - lo), b->rc_flag + lo, b->close_last + lo,
                                                     b->close_max + lo, local + lo, blk + k * chunk_blks, b->run_tot, d_info + 8 * k,
                                                     b->pool_used, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(info.data(), d_info, n_chunks * 64, hipMemcpyDeviceToHost, ctx->stream));
        return PG_OK;
    }
    // the totals: the last chunk's base + its runs
    int wait_totals()
    {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const unsigned long long *last = info.data() + 8 * (n_chunks - 1);
        tot[0] = last[0] + last[2];
        tot[1] = last[1] + last[3];
        return PG_OK;
    }
    // d_runs[k]: room for tot[k] runs; a list without a run needs no buffer -- its null pointer is never written through (a null
    // far buffer makes the gather place the far runs behind the close runs: there are none to place).  d_off[k]: n offsets.
    int queue_gather(pg_run *const d_runs[2], unsigned long long *const d_off[2])
    {
        const unsigned long long pool_runs = (unsigned long long)b->pool_shard_cap * PG_POOL_SHARDS;
        for (size_t k = 0, lo = 0; k < n_chunks; k++, lo += chunk)
            HIP_TRY(ctx, (hipError_t)pg_deliver_gather_runs(b->out_rec + lo, (uint32_t)std::min(chunk, n - lo), local + lo, blk + k * chunk_blks,
                                                            d_info + 8 * k, b->pool, pool_runs, tot[0] ? d_runs[0] : nullptr,
                                                            tot[1] ? d_runs[1] : nullptr, std::max(tot[0], tot[1]),
                                                            d_off[0] + lo, d_off[1] + lo, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(info.data(), d_info, n_chunks * 64, hipMemcpyDeviceToHost, ctx->stream));
        return PG_OK;
    }
    int wait_gather()
    {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        // the buffers hold the totals exactly and the search has checked its pool: a gather that ran out of either is a bug
        for (size_t k = 0; k < n_chunks; k++)
            if (info[8 * k + 5]) return fail(ctx, PG_E_DEVICE, "download: the gather of chunk " + std::to_string(k) + " found a run list out of bounds");
        return PG_OK;
    }
};

// Results of a searched batch to the host: the two passes, with temporaries for the gathered runs and offsets, so that the run
// buffers can be sized from the batch's totals and only the compact CSR crosses PCIe (pinned host buffers).
// summaries = false (pg_search_batch_table, between its two launches): the per-read close-end summaries stay on the device
int download(pg_ctx *ctx, pg_device_batch *b, pg_result *r, bool summaries = true)
{
    const size_t n = b->n;
    r->n = b->n;
    if (!r->close_off.resize(n + 1) || !r->far_off.resize(n + 1) || !r->rc_flag.resize(n) || !r->close_last.resize(n) ||
        !r->close_max.resize(n))
        return fail(ctx, PG_E_NOMEM, "pinned host memory for the result");
    r->close_runs.resize(0);
    r->far_runs.resize(0);
    if (!n) {
        r->close_off[0] = r->far_off[0] = 0;
        return PG_OK;
    }
    DeliveryPasses p(ctx, b);
    if (int rc = p.queue_scan()) return rc;
    unsigned long long *d_off[2] = { (unsigned long long *)p.tmp.take(n * 8), (unsigned long long *)p.tmp.take(n * 8) };
    if (!d_off[0] || !d_off[1]) return fail(ctx, PG_E_NOMEM, "device memory for the download's scans");
    // (the per-read summaries travel while the host sizes the run buffers)
    if (summaries) {
        HIP_TRY(ctx, hipMemcpyAsync(r->rc_flag.data(), b->rc_flag, n, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(r->close_last.data(), b->close_last, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(r->close_max.data(), b->close_max, n * 2, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (int rc = p.wait_totals()) return rc;
    const unsigned long long *tot = p.tot;
    pg_run *d_runs[2] = { nullptr, nullptr };
    if (!r->close_runs.resize((size_t)tot[0]) || !r->far_runs.resize((size_t)tot[1]))
        return fail(ctx, PG_E_NOMEM, "pinned host memory for the runs");
    for (int k = 0; k < 2; k++)
        if (tot[k] && !(d_runs[k] = (pg_run *)p.tmp.take((size_t)tot[k] * sizeof(pg_run)))) return fail(ctx, PG_E_NOMEM, "gathered runs");
    if (int rc = p.queue_gather(d_runs, d_off)) return rc;
    HostBuf<uint64_t> *off[2] = { &r->close_off, &r->far_off };
    HostBuf<pg_run> *runs[2] = { &r->close_runs, &r->far_runs };
    for (int k = 0; k < 2; k++)
        if (tot[k]) {
            HIP_TRY(ctx, hipMemcpyAsync(off[k]->data(), d_off[k], n * 8, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(runs[k]->data(), d_runs[k], (size_t)tot[k] * sizeof(pg_run), hipMemcpyDeviceToHost, ctx->stream));
        }
    // (the offsets of a list without a run are all 0: written here while the other list is on its way, not sent -- the batch of
    // the far-end seams has no close run)
    for (int k = 0; k < 2; k++)
        if (!tot[k]) std::memset(off[k]->data(), 0, n * 8);
    if (int rc = p.wait_gather()) return rc;
    r->close_off[n] = tot[0];
    r->far_off[n] = tot[1];
    return PG_OK;
}

// ... and into the caller's device buffers (pg_device_batch_download_device; the pointers have been checked): the gather writes
// the runs and offsets there, the summaries are device-to-device copies, off[n] is stored by a kernel from the last chunk's info.
// Only the per-chunk info crosses to the host.  Nothing is written when a capacity is below its total.
int download_device(pg_ctx *ctx, pg_device_batch *b, const pg_device_result *dst)
{
    const size_t n = b->n;
    if (!n) {                                            // offsets [0]; nothing is launched
        HIP_TRY(ctx, hipMemsetAsync(dst->close_off, 0, 8, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(dst->far_off, 0, 8, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return PG_OK;
    }
    DeliveryPasses p(ctx, b);
    int rc = p.queue_scan();
    if (!rc) rc = p.wait_totals();
    if (rc) return rc;
    if (p.tot[0] > dst->close_cap || p.tot[1] > dst->far_cap)
        return fail(ctx, PG_E_INVALID, "pg_device_result: " + std::string(p.tot[0] > dst->close_cap ? "close_cap" : "far_cap") +
                                           " is below the batch's number of runs (pg_device_batch_result_sizes)");
    if ((rc = check_device_ptr(ctx, dst->close_runs, (size_t)p.tot[0] * sizeof(pg_run), 4, "pg_device_result.close_runs")) ||
        (rc = check_device_ptr(ctx, dst->far_runs, (size_t)p.tot[1] * sizeof(pg_run), 4, "pg_device_result.far_runs")))
        return rc;
    pg_run *d_runs[2] = { dst->close_runs, dst->far_runs };
    unsigned long long *d_off[2] = { (unsigned long long *)dst->close_off, (unsigned long long *)dst->far_off };
    if ((rc = p.queue_gather(d_runs, d_off))) return rc;
    HIP_TRY(ctx, (hipError_t)pg_devio_store_totals(p.d_last_info(), d_off[0] + n, d_off[1] + n, ctx->stream));
    if (dst->rc_flag) HIP_TRY(ctx, hipMemcpyAsync(dst->rc_flag, b->rc_flag, n, hipMemcpyDeviceToDevice, ctx->stream));
    if (dst->close_last) HIP_TRY(ctx, hipMemcpyAsync(dst->close_last, b->close_last, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    if (dst->close_max) HIP_TRY(ctx, hipMemcpyAsync(dst->close_max, b->close_max, n * 2, hipMemcpyDeviceToDevice, ctx->stream));
    return p.wait_gather();
}

// Pass 1 alone: the batch's two totals (pg_device_batch_result_sizes).
int result_sizes(pg_ctx *ctx, pg_device_batch *b, uint64_t *n_close, uint64_t *n_far)
{
    *n_close = *n_far = 0;
    if (!b->n) return PG_OK;
    DeliveryPasses p(ctx, b);
    int rc = p.queue_scan();
    if (!rc) rc = p.wait_totals();
    if (rc) return rc;
    *n_close = p.tot[0];
    *n_far = p.tot[1];
    return PG_OK;
}

// ---------------------------------------------------------------- host in / host out
// Host buffers in, host results out, as a three-stage pipeline over chunks of 64 k to 1 M reads (PgHostPlan::bounds):
//   copy stream      the chunk's inputs, host -> HBM
//   compute stream   pack, search (the kernel takes a read range of the batch), delivery kernels: the chunk's runs
//                    gathered in read order behind the earlier chunks', its 64-bit CSR offsets (pg_deliver_chunk)
//   download stream  the chunk's slice of every result array -> pinned host memory, while the next chunk is searched
// The host only waits for "chunk k delivered", reads the chunk's base and run counts (32 bytes) and queues its copies.
// search_host is the driver: the plan (pg_host_plan.h) says what the call will do, the steps of HostCall do it and return a status.
int hip_status(pg_ctx *ctx, hipError_t e, const char *what)
{
    if (e == hipSuccess) return PG_OK;
    return fail(ctx, e == hipErrorOutOfMemory ? PG_E_NOMEM : PG_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

// Owns the arena batch of one call and the result it has not returned yet.  A call that leaves without setting `ok` has failed:
// nothing it queued on the four streams may outlive the buffers it points at.
struct BatchGuard {
    pg_device_batch *b = nullptr;
    pg_result *r = nullptr;
    bool ok = false;
    ~BatchGuard()
    {
        if (!b) return;                                          // (alloc_batch failed: nothing was queued)
        if (!ok) (void)hipDeviceSynchronize();
        free_batch_buffers(b);
        delete b;
        if (!ok) delete r;
    }
};

// The arrays a delivery writes and a result holds: parts of ONE block (block_views walks PgHostPlan::blk, for the pinned host
// block and the device block alike; runs[1] is null, the far runs follow the close runs) or buffers of their own.
struct DeliveryViews { unsigned long long *off[2]; uint8_t *rc; uint32_t *last; uint16_t *max; pg_run *runs[2]; };
DeliveryViews block_views(const PgHostPlan &p, uint8_t *base)
{
    auto at = [&](int part) { return (void *)(base + p.blk[part].off); };
    return { { (unsigned long long *)at(PG_BLK_CLOSE_OFF), (unsigned long long *)at(PG_BLK_FAR_OFF) }, (uint8_t *)at(PG_BLK_RC),
             (uint32_t *)at(PG_BLK_LAST), (uint16_t *)at(PG_BLK_MAX), { (pg_run *)at(PG_BLK_RUNS), nullptr } };
}

struct Copy { void *dst; const void *src; size_t bytes; };
int queue_copies(pg_ctx *ctx, std::initializer_list<Copy> copies, hipMemcpyKind kind, hipStream_t st, const char *what)
{
    for (const Copy &x : copies)
        if (x.bytes)                                             // (reads without bases, a list without a run in this chunk)
            if (int rc = hip_status(ctx, hipMemcpyAsync(x.dst, x.src, x.bytes, kind, st), what)) return rc;
    return PG_OK;
}

// One call of search_host: what the steps share.
struct HostCall {
    pg_ctx *ctx;
    const pg_read_batch *reads;
    int mode;
    const PgHostPlan &plan;
    HostBuf<uint64_t> &off;                                      // the read offsets rebased to 0 (pinned; one block: + room for the one-copy upload)
    pg_device_batch *b;
    pg_result *r;
    DeliveryViews d{};                                           // device side of the delivery
    uint8_t *d_block = nullptr;
    void *d_local = nullptr, *d_blk = nullptr;
    unsigned long long *d_info = nullptr, tot[2] = { 0, 0 };
    HostBuf<unsigned long long> info;                            // pinned mirror of d_info: 8 values per chunk
    bool whole_batch = false;                // fall back to run_search (pool overflow) + download (pool or delivery overflow)
    double t_res = 0, t_search = 0;

    int setup();
    int queue_chunk(uint32_t k);
    int collect_chunk(uint32_t k);
    int finish();
};

// The result's arrays (views into one pinned block, or buffers of their own with room for `cap` runs per list); then, for a batch
// with reads, streams and events, the delivery buffers (arena: PgHostPlan::takes in order), the info's mirror, the clock's start.
int HostCall::setup()
{
    const PgHostPlan &p = plan;
    const size_t n = r->n = p.n;
    if (p.single) {
        if (!r->block.resize(p.blk_bytes)) return fail(ctx, PG_E_NOMEM, "pinned host memory for the result");
        const DeliveryViews h = block_views(p, r->block.data());
        r->close_off.set_view(h.off[0], n + 1, n + 1);
        r->far_off.set_view(h.off[1], n + 1, n + 1);
        r->rc_flag.set_view(h.rc, n, n);
        r->close_last.set_view(h.last, n, n);
        r->close_max.set_view(h.max, n, n);
        r->close_runs.set_view(h.runs[0], 0, p.cap);
        r->far_runs.set_view(h.runs[0], 0, 0);                   // (placed behind the close runs once their number is known)
    } else if (!r->close_off.resize(n + 1) || !r->far_off.resize(n + 1) || !r->rc_flag.resize(n) || !r->close_last.resize(n) ||
               !r->close_max.resize(n) || !r->close_runs.resize(n ? p.cap : 0) || !r->far_runs.resize(n ? p.cap : 0))
        return fail(ctx, PG_E_NOMEM, "pinned host memory for the result");
    t_res = t_search = now_ms();
    if (!n) {
        r->close_off[0] = r->far_off[0] = 0;
        return PG_OK;
    }
    for (hipStream_t *s : { &ctx->copy_stream, &ctx->dl_stream, &ctx->stream2 })
        if (!*s)
            if (int rc = hip_status(ctx, hipStreamCreate(s), "hipStreamCreate")) return rc;
    while (ctx->events.size() < 2 * (size_t)p.n_chunks + 1) {
        hipEvent_t ev = nullptr;
        if (int rc = hip_status(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreateWithFlags")) return rc;
        ctx->events.push_back(ev);
    }
    void *got[PG_PLAN_MAX_TAKES], **t = got;
    for (int k = 0; k < p.n_takes; k++)
        if (!(got[k] = ctx->arena.take(p.takes[k]))) return fail(ctx, PG_E_NOMEM, "device arena too small for the delivery buffers");
    if (p.single) {
        d = block_views(p, d_block = (uint8_t *)*t++);
    } else {
        d = { { (unsigned long long *)t[2], (unsigned long long *)t[3] }, b->rc_flag, b->close_last, b->close_max, { (pg_run *)t[0], (pg_run *)t[1] } };
        t += 4;
    }
    d_local = *t++;
    d_blk = *t++;
    d_info = (unsigned long long *)*t++;
    if (!info.resize((size_t)p.n_chunks * 8)) return fail(ctx, PG_E_NOMEM, "pinned host memory");
    // (the run-pool cursors, both sets of read counters and the delivery's running totals are zero from alloc_batch's one
    // memset of the output block, queued on ctx->stream)
    if (int rc = hip_status(ctx, hipEventRecord(ctx->ev0, ctx->stream), "hipEventRecord")) return rc;
    if (p.n_chunks > 1) return hip_status(ctx, hipEventRecord(ctx->events[2 * p.n_chunks], ctx->stream), "hipEventRecord");
    return PG_OK;
}

// Chunk k: input copy, waits, search launch, delivery, info copy, event; behind the last chunk the clock's end.
int HostCall::queue_chunk(uint32_t k)
{
    const uint32_t n_chunks = plan.n_chunks, lo = plan.bounds[k], hi = plan.bounds[k + 1], cn = hi - lo;
    const char *ev = "hipEventRecord", *wait = "hipStreamWaitEvent";
    hipStream_t cs = ctx->copy_stream;
    const Copy bases = { b->seq + off[lo], reads->seq ? reads->seq + reads->seq_off[0] + off[lo] : nullptr, (size_t)(off[hi] - off[lo]) };
    // A one-chunk batch (Pindel's own 50 000-read flush): the five small arrays lie one after the other in the arena
    // (alloc_batch, PgInputLayout), so they go as ONE copy from the pinned block that already holds the offsets -- queued before
    // the bases, whose copy from pageable memory blocks the call.  (Five copies cost 60 us of calls and 40 us of serial DMA.)
    const PgInputLayout &in = plan.in;
    int rc;
    if (plan.single && b->in_arena && in.span <= off.cap_bytes) {
        char *h = (char *)off.data();
        memcpy(h + in.a[PG_IN_STRAND].off, reads->anchor_strand, cn);
        memcpy(h + in.a[PG_IN_POS].off, reads->anchor_pos, (size_t)cn * 4);
        memcpy(h + in.a[PG_IN_ISZ].off, reads->insert_size, (size_t)cn * 2);
        memcpy(h + in.a[PG_IN_CHR].off, reads->chr_id, (size_t)cn * 4);
        rc = queue_copies(ctx, { { b->seq_off, h, in.span }, bases }, hipMemcpyHostToDevice, cs, "input copy");
    } else
        rc = queue_copies(ctx, { bases, { b->seq_off + lo, off.data() + lo, (size_t)(cn + 1) * 8 }, { b->strand + lo, reads->anchor_strand + lo, cn },
                                 { b->pos + lo, reads->anchor_pos + lo, (size_t)cn * 4 }, { b->isz + lo, reads->insert_size + lo, (size_t)cn * 2 },
                                 { b->chr + lo, reads->chr_id + lo, (size_t)cn * 4 } }, hipMemcpyHostToDevice, cs, "input copy");
    if (rc || (rc = hip_status(ctx, hipEventRecord(ctx->events[2 * k], cs), ev))) return rc;
    // even chunks on one kernel stream, odd chunks on the other: the next chunk's workgroups move in while this
    // chunk's persistent launch drains; the deliveries stay in chunk order (running totals, shared scratch)
    hipStream_t ks = (k & 1u) ? ctx->stream2 : ctx->stream;
    if (k == 1 && (rc = hip_status(ctx, hipStreamWaitEvent(ks, ctx->events[2 * n_chunks], 0), wait))) return rc;   // (alloc_batch's memset)
    if ((rc = hip_status(ctx, hipStreamWaitEvent(ks, ctx->events[2 * k], 0), wait))) return rc;
    // (the chunk's records: packed by its search launch itself -- pack in place -- or, 64-bit candidate ids, by a launch of their own)
    if ((rc = launch_range(ctx, b, mode, lo, cn, ks, (int)(k & 1u), k < 2, true))) return rc;
    if (k > 0 && (rc = hip_status(ctx, hipStreamWaitEvent(ks, ctx->events[2 * (k - 1) + 1], 0), wait))) return rc;
    const unsigned long long pool_runs = (unsigned long long)b->pool_shard_cap * PG_POOL_SHARDS;
    rc = hip_status(ctx, (hipError_t)pg_deliver_chunk(b->out_rec + lo, cn, d.rc + lo, d.last + lo, d.max + lo, d_local, d_blk, b->run_tot, d_info + 8 * k,
                                                      b->pool, pool_runs, d.runs[0], d.runs[1], plan.cap, d.off[0] + lo, d.off[1] + lo, b->pool_used, ks),
                    "pg_deliver_chunk");
    if (rc || (rc = queue_copies(ctx, { { info.data() + 8 * k, d_info + 8 * k, 64 } }, hipMemcpyDeviceToHost, ks, "info copy"))) return rc;
    if ((rc = hip_status(ctx, hipEventRecord(ctx->events[2 * k + 1], ks), ev))) return rc;
    if (k + 1 < n_chunks) return PG_OK;
    // (the last delivery waited for every earlier one, so its stream's end is the end of the batch)
    if (ks != ctx->stream && (rc = hip_status(ctx, hipStreamWaitEvent(ctx->stream, ctx->events[2 * k + 1], 0), wait))) return rc;
    return hip_status(ctx, hipEventRecord(ctx->ev1, ctx->stream), ev);
}

// Chunk k is delivered: its slices (or the one block) to the host on the download stream -- or, an overflow, whole_batch.
int HostCall::collect_chunk(uint32_t k)
{
    const uint32_t lo = plan.bounds[k], cn = plan.bounds[k + 1] - lo;
    if (int rc = hip_status(ctx, hipEventSynchronize(ctx->events[2 * k + 1]), "hipEventSynchronize")) return rc;
    const unsigned long long *in = info.data() + 8 * k, cap = plan.cap;
    whole_batch = (plan.single ? in[2] + in[3] > cap : (in[0] + in[2] > cap || in[1] + in[3] > cap)) || in[5] || in[4] > b->pool_shard_cap;
    if (whole_batch) return PG_OK;
    tot[0] = in[0] + in[2];                                      // (one block: the bases are 0)
    tot[1] = in[1] + in[3];
    if (plan.single) {
        // offsets, summaries, close runs, far runs: one copy
        const size_t far_at = pg_plan_far_runs_at(plan, (size_t)in[2]), used = far_at + (size_t)in[3] * sizeof(pg_run);
        r->far_runs.set_view(r->block.data() + far_at, (size_t)in[3], (size_t)in[3]);
        return hip_status(ctx, hipMemcpyAsync(r->block.data(), d_block, used, hipMemcpyDeviceToHost, ctx->dl_stream), "result copy");
    }
    // (the close-end summary: only a later pg_far_end_batch on a close-only result reads it)
    const size_t summary = mode == PG_MODE_CLOSE ? cn : 0;
    return queue_copies(ctx, { { r->close_runs.data() + in[0], d.runs[0] + in[0], (size_t)in[2] * sizeof(pg_run) },
                               { r->far_runs.data() + in[1], d.runs[1] + in[1], (size_t)in[3] * sizeof(pg_run) },
                               { r->close_off.data() + lo, d.off[0] + lo, (size_t)cn * 8 }, { r->far_off.data() + lo, d.off[1] + lo, (size_t)cn * 8 },
                               { r->rc_flag.data() + lo, d.rc + lo, cn }, { r->close_last.data() + lo, d.last + lo, summary * 4 },
                               { r->close_max.data() + lo, d.max + lo, summary * 2 } }, hipMemcpyDeviceToHost, ctx->dl_stream, "result copy");
}

// Every chunk is queued and collected: the totals and the trimmed result, or the whole batch again.
int HostCall::finish()
{
    float ms = 0.f;
    int rc = hip_status(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    if (rc || (rc = hip_status(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1), "hipEventElapsedTime"))) return rc;
    t_search = now_ms();
    // (the last chunk's info saw every launch's pool cursors: its delivery waited for all the earlier ones)
    const bool pool_overflow = info[8 * (size_t)(plan.n_chunks - 1) + 4] > b->pool_shard_cap;
    if (pool_overflow) whole_batch = true;
    if ((rc = hip_status(ctx, hipStreamSynchronize(ctx->dl_stream), "hipStreamSynchronize"))) return rc;
    if (!pool_overflow) {
        ctx->last_ms = ms;
        ctx->last_runs = tot[0] + tot[1];
    }
    if (whole_batch) {
        // a pool shard overflowed, or the lists outgrew the delivery buffers: the whole batch again with the regrown pool
        // where needed, then download(): the same delivery kernels over the whole batch, into buffers sized from its totals
        if (pool_overflow && (rc = run_search(ctx, b, mode))) return rc;
        return download(ctx, b, r);
    }
    r->close_off[plan.n] = tot[0];
    r->far_off[plan.n] = tot[1];
    r->close_runs.resize((size_t)tot[0]);
    r->far_runs.resize((size_t)tot[1]);
    if (mode != PG_MODE_CLOSE) {                                 // not downloaded: pg_far_end_batch refuses such a result
        r->close_last.resize(0);
        r->close_max.resize(0);
    }
    return PG_OK;
}

int search_host(pg_ctx *ctx, const pg_read_batch *reads, int mode, pg_result **out)
{
    use_device(ctx);
    if (!ctx || !out) return PG_E_INVALID;
    *out = nullptr;
    // (pinned, from the cache: as a malloc'd array the runtime locks its pages for the copy and the free() of 80 MB after a
    // 10 M-read call spent 13 ms in munmap + unpinning)
    HostBuf<uint64_t> off;
    const double t_start = now_ms();
    const PgHostPlan plan = pg_host_plan(reads ? reads->n_reads : 0u, env().host_chunk, env().no_single_block, env().tiny_delivery);
    BatchGuard g;
    int rc = alloc_batch(ctx, reads, false, off, &g.b, true, &plan);
    if (rc) return rc;
    const double t_alloc = now_ms();
    HostCall c{ ctx, reads, mode, plan, off, g.b, g.r = new pg_result() };
    if ((rc = c.setup())) return rc;
    for (uint32_t k = 0; k < plan.n_chunks; k++)
        if ((rc = c.queue_chunk(k))) return rc;
    // as the chunks get delivered: their slices to the host
    for (uint32_t k = 0; k < plan.n_chunks && !c.whole_batch; k++)
        if ((rc = c.collect_chunk(k))) return rc;
    if (plan.n && (rc = c.finish())) return rc;
    if (g_host_timing)
        fprintf(stderr, "pg_search_batch: %u reads: validate+alloc %.2f ms, result buffers %.2f ms, copy+search+delivery %.2f ms, tail %.2f ms%s\n",
                plan.n, t_alloc - t_start, c.t_res - t_alloc, c.t_search - c.t_res, now_ms() - c.t_search, c.whole_batch ? " (whole-batch fallback)" : "");
    g.ok = true;
    *out = g.r;
    return PG_OK;
}

// Copies the packed planes and the chromosome tables of the ctx to the device.
int upload_reference(pg_ctx *ctx)
{
    std::vector<uint32_t> sizes(ctx->comp_size.size());
    for (size_t c = 0; c < sizes.size(); c++) sizes[c] = (uint32_t)ctx->comp_size[c];
    int rc;
    if ((rc = dev_upload(ctx, &ctx->d_lo, ctx->h_lo.data(), ctx->h_lo.size())) ||
        (rc = dev_upload(ctx, &ctx->d_hi, ctx->h_hi.data(), ctx->h_hi.size())) ||
        (rc = dev_upload(ctx, &ctx->d_nn, ctx->h_nn.data(), ctx->h_nn.size())) ||
        (rc = dev_upload(ctx, &ctx->d_word_off, ctx->word_off.data(), ctx->word_off.size())) ||
        (rc = dev_upload(ctx, &ctx->d_chr_size, sizes.data(), sizes.size()))) {
        free_reference(ctx);
        return rc;
    }
    ctx->plane_words = ctx->h_lo.size();
    ctx->mirror_ok = true;
    return PG_OK;
}

// The host mirror of the planes, for the two entries that read it: after pg_load_reference_device it is filled here, on first
// use, with one device-to-host copy per plane.
int host_mirror(const pg_ctx *ctx)
{
    if (ctx->mirror_ok) return PG_OK;
    use_device(ctx);
    try {
        ctx->h_lo.resize(ctx->plane_words);
        ctx->h_hi.resize(ctx->plane_words);
        ctx->h_nn.resize(ctx->plane_words);
    } catch (...) {
        ctx->h_lo.clear();
        ctx->h_hi.clear();
        ctx->h_nn.clear();
        return PG_E_NOMEM;
    }
    const size_t bytes = (size_t)ctx->plane_words * sizeof(uint32_t);
    if (hipMemcpy(ctx->h_lo.data(), ctx->d_lo, bytes, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(ctx->h_hi.data(), ctx->d_hi, bytes, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(ctx->h_nn.data(), ctx->d_nn, bytes, hipMemcpyDeviceToHost) != hipSuccess)
        return PG_E_DEVICE;
    ctx->mirror_ok = true;
    return PG_OK;
}

}  // namespace

// A pointer a device entry was handed: device memory of the context's own GPU, aligned for its element type, with the `bytes`
// the library will read or write inside its allocation.  Checked before anything is launched: a host pointer must end in a
// status code, never in a fault.  bytes = 0: nothing will be touched, nothing is checked.
int check_device_ptr(pg_ctx *ctx, const void *p, size_t bytes, size_t align, const char *what)
{
    if (!bytes) return PG_OK;
    if (!p) return fail(ctx, PG_E_INVALID, std::string(what) + ": null pointer");
    hipPointerAttribute_t at;
    std::memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();                         // (a pointer the runtime does not know: plain host memory)
        return fail(ctx, PG_E_INVALID, std::string(what) + ": not device memory");
    }
    if (at.type != hipMemoryTypeDevice) return fail(ctx, PG_E_INVALID, std::string(what) + ": not device memory");
    if (at.device != ctx->prm.device) return fail(ctx, PG_E_INVALID, std::string(what) + ": memory of another GPU than the context's");
    if ((uintptr_t)p % align) return fail(ctx, PG_E_INVALID, std::string(what) + ": misaligned for its element type");
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, PG_E_INVALID, std::string(what) + ": not inside a device allocation");
    }
    const uintptr_t lo = (uintptr_t)base, at_p = (uintptr_t)p;
    if (at_p < lo || at_p - lo > size || bytes > size - (at_p - lo))
        return fail(ctx, PG_E_INVALID, std::string(what) + ": reaches past the end of its device allocation");
    return PG_OK;
}

namespace {

// pg_device_batch_upload_device: the batch's arrays are in device memory.  The measurement kernel (pg_devio.hip) is the
// device twin of validate_and_measure; only its 40-byte record comes to the host, which reports, sizes and allocates as the
// host upload does (alloc_batch_buffers), copies device-to-device and packs.
int upload_batch_device(pg_ctx *ctx, const pg_read_batch *d, pg_device_batch **out)
{
    if (!d || (d->n_reads && (!d->seq_off || !d->anchor_strand || !d->anchor_pos || !d->insert_size || !d->chr_id)))
        return fail(ctx, PG_E_INVALID, "null array in pg_read_batch");
    if (ctx->names.empty()) return fail(ctx, PG_E_NO_REFERENCE, "no reference loaded");
    const size_t n = d->n_reads;
    BatchMeasure m;
    m.n = d->n_reads;
    uint64_t *d_off = nullptr;                           // becomes the batch's seq_off
    uint64_t off0 = 0;
    int rc = PG_OK;
    if (n) {                                             // (nothing is checked or launched for an empty batch)
        if ((rc = check_device_ptr(ctx, d->seq_off, (n + 1) * 8, 8, "pg_read_batch.seq_off")) ||
            (rc = check_device_ptr(ctx, d->anchor_strand, n, 1, "pg_read_batch.anchor_strand")) ||
            (rc = check_device_ptr(ctx, d->anchor_pos, n * 4, 4, "pg_read_batch.anchor_pos")) ||
            (rc = check_device_ptr(ctx, d->insert_size, n * 2, 2, "pg_read_batch.insert_size")) ||
            (rc = check_device_ptr(ctx, d->chr_id, n * 4, 4, "pg_read_batch.chr_id")))
            return rc;
        PgReadMeasure h, *d_rec = nullptr;
        std::memset(&h, 0, sizeof h);
        h.first_bad = PG_MEASURE_NONE;
        h.len_min = 0xffffffffu;
        HIP_TRY(ctx, hipMalloc((void **)&d_off, pg_input_layout(n).a[PG_IN_SEQ_OFF].bytes));
        hipError_t e = hipMalloc((void **)&d_rec, sizeof h);
        if (e == hipSuccess) e = hipMemcpyAsync(d_rec, &h, sizeof h, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess)
            e = (hipError_t)pg_devio_measure_reads((const unsigned long long *)d->seq_off, d->anchor_pos, d->insert_size, d->chr_id,
                                                   d->n_reads, ctx->d_chr_size, (int32_t)ctx->names.size(), ctx->prm.spacer,
                                                   (unsigned long long *)d_off, d_rec, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&h, d_rec, sizeof h, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (d_rec) (void)hipFree(d_rec);
        if (e != hipSuccess) rc = fail(ctx, e == hipErrorOutOfMemory ? PG_E_NOMEM : PG_E_DEVICE, std::string("read measurement: ") + hipGetErrorString(e));
        // the host upload's order: a missing seq, then the first bad read's code
        else if (!d->seq && h.offn > h.off0) rc = fail(ctx, PG_E_INVALID, "null seq in pg_read_batch");
        else if (h.first_bad != PG_MEASURE_NONE) rc = validation_failure(ctx, (int)(h.first_bad & 0xffu));
        else rc = check_device_ptr(ctx, d->seq ? d->seq + h.off0 : nullptr, (size_t)(h.offn - h.off0), 1, "pg_read_batch.seq");
        if (rc) {
            (void)hipFree(d_off);
            return rc;
        }
        off0 = h.off0;
        m.nseq = h.offn - h.off0;
        m.max_len = std::max<uint32_t>(h.len_max, 1u);
        m.max_isz = h.isz_max;
        m.uniform_len = h.len_min == h.len_max ? h.len_max : 0u;
    }
    if ((rc = batch_levels(ctx, m.max_len, &m.levels))) {
        if (d_off) (void)hipFree(d_off);
        return rc;
    }
    pg_device_batch *b = nullptr;
    if ((rc = alloc_batch_buffers(ctx, m, &b, false, nullptr, d_off))) return rc;
    rc = copy_batch_inputs(ctx, b, d, m.nseq ? d->seq + off0 : nullptr, m.nseq, nullptr, hipMemcpyDeviceToDevice);
    if (!rc) rc = publish_soa(ctx, b);
    if (!rc) rc = pack_reads(ctx, b, 0, b->n);
    if (rc) {
        free_batch_buffers(b);
        delete b;
        return rc;
    }
    *out = b;
    return PG_OK;
}

// pg_load_reference_device: the planes are built in HBM from the caller's ASCII bases (pg_devio.hip), bit for bit what
// pg_load_reference packs on host threads; the host mirror stays empty until somebody asks (host_mirror).
int load_reference_device(pg_ctx *ctx, int32_t n_chr, const char *const *names, const uint8_t *const *d_seq, const uint64_t *len_padded)
{
    uint64_t total_words = 0;
    std::vector<uint64_t> word_off;
    for (int c = 0; c < n_chr; c++) {
        if (len_padded[c] > PG_MAX_CHR_PADDED) return fail(ctx, PG_E_UNSUPPORTED, "chromosome of 2^31 bases or more (positions are signed 32-bit on the device)");
        if (len_padded[c] < 2ull * ctx->prm.spacer) return fail(ctx, PG_E_INVALID, "chromosome shorter than its spacers");
        total_words += PG_GUARD_WORDS;
        word_off.push_back(total_words);
        total_words += (len_padded[c] + 31) / 32 + PG_GUARD_WORDS;
    }
    total_words += 8;
    for (int c = 0; c < n_chr; c++)
        if (int rc = check_device_ptr(ctx, d_seq[c], (size_t)len_padded[c], 1, "d_seq_padded")) return rc;
    free_reference(ctx);
    for (int c = 0; c < n_chr; c++) {
        ctx->names.push_back(names && names[c] ? names[c] : "");
        ctx->comp_size.push_back(len_padded[c]);
    }
    ctx->word_off = word_off;
    ctx->plane_words = total_words;
    std::vector<uint32_t> sizes(ctx->comp_size.size());
    for (size_t c = 0; c < sizes.size(); c++) sizes[c] = (uint32_t)ctx->comp_size[c];
    const size_t bytes = (size_t)total_words * sizeof(uint32_t);
    int rc;
    if ((rc = dev_alloc(ctx, &ctx->d_lo, total_words)) || (rc = dev_alloc(ctx, &ctx->d_hi, total_words)) ||
        (rc = dev_alloc(ctx, &ctx->d_nn, total_words)) ||
        (rc = dev_upload(ctx, &ctx->d_word_off, ctx->word_off.data(), ctx->word_off.size())) ||
        (rc = dev_upload(ctx, &ctx->d_chr_size, sizes.data(), sizes.size()))) {
        free_reference(ctx);
        return rc;
    }
    // guards, tails and the 8 trailing words are N; the kernel writes every word of every chromosome
    hipError_t e = hipMemsetAsync(ctx->d_lo, 0, bytes, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(ctx->d_hi, 0, bytes, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(ctx->d_nn, 0xff, bytes, ctx->stream);
    for (int c = 0; c < n_chr && e == hipSuccess; c++)
        e = (hipError_t)pg_devio_pack_reference(d_seq[c], len_padded[c], ctx->d_lo + word_off[c], ctx->d_hi + word_off[c],
                                                ctx->d_nn + word_off[c], ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        free_reference(ctx);
        return fail(ctx, PG_E_DEVICE, std::string("reference pack: ") + hipGetErrorString(e));
    }
    return PG_OK;
}

}  // namespace

// ============================================================================== C ABI
extern "C" {

const PgEnvSwitches *pg_env_switches(void) { return &env(); }
void pg_debug_reload_env(void)
{
    (void)env();
    load_env();
}

void pg_default_params(pg_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->abi_version = PG_ABI_VERSION;
    p->device = 0;
    p->max_range_index = 2;
    p->additional_mismatch = 1;
    p->min_perfect_match_around_bp = 3;
    p->min_close = 8;
    p->max_allowed_mismatch_rate = 0.02;
    p->seq_error_rate = 0.01;
    p->sensitivity = 0.95;
    p->spacer = 100000;
}

// Do the context's length tables (pg_len_rec of its parameters) reproduce every baked row of the fixed-length kernels ?
static bool fixed_row_matches(const PgFixedLen &f, const PgLenRec &r)
{
    return f.lvl == r.lvl && f.depth == r.depth && f.jmask0 == r.jmask0 && f.ro == r.ro && f.jmask1 == r.jmask1;
}
static bool fixed_rows_match(const PgLenRec *len_tab)
{
    const PgFixedLen rows[PG_FIXED_LENS] = PG_FIXED_LEN_ROWS;
    for (const PgFixedLen &f : rows)
        if (!fixed_row_matches(f, len_tab[f.len])) return false;
    return true;
}
// (the parameters the default-parameter kernels are built for, pg_launch_search: only such a context would run a fixed-length kernel)
static bool fixed_len_wanted(const pg_params &p)
{
    pg_params d;
    pg_default_params(&d);
    return p.max_range_index == d.max_range_index && p.additional_mismatch == d.additional_mismatch &&
           p.min_perfect_match_around_bp == d.min_perfect_match_around_bp && p.min_close == d.min_close && p.spacer == d.spacer;
}
// Diagnostics (not in the public header; needs no device): the k-th baked row of the fixed-length kernels and what the host's tables
// give for that length under pg_default_params -- five words each: lvl, depth, jmask0, ro, jmask1.  Returns the number of rows
// (k out of range: nothing is written).
int pg_debug_fixed_len_row(int k, uint32_t *len, uint32_t *baked, uint32_t *host)
{
    const PgFixedLen rows[PG_FIXED_LENS] = PG_FIXED_LEN_ROWS;
    if (k < 0 || k >= PG_FIXED_LENS) return PG_FIXED_LENS;
    const PgFixedLen &f = rows[k];
    std::unique_ptr<pg_ctx> ctx(new pg_ctx());
    pg_default_params(&ctx->prm);
    make_tables(ctx.get());
    const PgLenRec r = pg_len_rec((int)f.len, ctx->mm, ctx->thr, ctx->prm.additional_mismatch, ctx->prm.min_close);
    if (len) *len = f.len;
    if (baked) { baked[0] = f.lvl; baked[1] = f.depth; baked[2] = f.jmask0; baked[3] = f.ro; baked[4] = f.jmask1; }
    if (host) { host[0] = r.lvl; host[1] = r.depth; host[2] = r.jmask0; host[3] = r.ro; host[4] = r.jmask1; }
    return PG_FIXED_LENS;
}

int pg_create(const pg_params *p, pg_ctx **out)
{
    if (!p || !out) return PG_E_INVALID;
    *out = nullptr;
    if (p->abi_version != PG_ABI_VERSION) return PG_E_INVALID;
    pg_ctx *ctx = new pg_ctx();
    ctx->prm = *p;
    // pindel.cpp:921-930: -x capped at g_MAX_RANGE_INDEX (9), -a raised to 1
    if (ctx->prm.max_range_index > 9) ctx->prm.max_range_index = 9;
    if (ctx->prm.max_range_index < 0) ctx->prm.max_range_index = 0;
    if (ctx->prm.additional_mismatch < 1) ctx->prm.additional_mismatch = 1;
    if (ctx->prm.min_close < 1 || ctx->prm.min_close > 64 || ctx->prm.min_perfect_match_around_bp < 0 ||
        ctx->prm.min_perfect_match_around_bp > 64) {
        delete ctx;
        return PG_E_UNSUPPORTED;
    }
    make_tables(ctx);
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0 || p->device < 0 || p->device >= n_dev) {
        // No HIP device: there is deliberately no CPU path behind this ABI.
        delete ctx;
        return PG_E_DEVICE;
    }
    if (hipSetDevice(p->device) != hipSuccess || hipStreamCreate(&ctx->stream) != hipSuccess ||
        hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess) {
        delete ctx;
        return PG_E_DEVICE;
    }
    // The persistent launch spreads its read counters over PG_N_XCD = 8 parts and relies on workgroup b running on XCD
    // b % 8 for locality (never for correctness: a workgroup that finds its part empty moves on to the next).  The
    // MI355X reports 256 compute units in 8 XCDs; on anything else the search still works, the note says what was found.
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, p->device) == hipSuccess) {
            const std::string arch = prop.gcnArchName;
            if (arch.rfind("gfx950", 0) != 0) {
                pg_destroy(ctx);
                return PG_E_DEVICE;                     // the library holds gfx950 code only
            }
            if (prop.multiProcessorCount != 256 && getenv("PG_QUIET") == nullptr)
                fprintf(stderr, "pindel_pg: note: device %d reports %d compute units (an MI355X has 256 in 8 XCDs); the per-XCD "
                                "work split stays correct but was tuned for that shape\n", p->device, prop.multiProcessorCount);
        }
    }
    // the kernel evaluates g_maxMismatch[L] from breakpoints: the table must be monotone (it is for every
    // -e/-E tried).  Whether a batch fits the 16 mismatch levels depends on its longest read and is checked
    // per batch (validate_and_measure).
    for (int i = 1; i < 500; i++)
        if (ctx->mm[i] < ctx->mm[i - 1]) {
            pg_destroy(ctx);
            return PG_E_UNSUPPORTED;
        }
    std::vector<PgLenRec> len_tab(512);
    for (int len = 0; len < 512; len++) len_tab[len] = pg_len_rec(len, ctx->mm, ctx->thr, ctx->prm.additional_mismatch, ctx->prm.min_close);
    // the fixed-length kernels hold these fields as constants: this context may run them only if its tables give the baked rows
    ctx->fixed_ok = fixed_rows_match(len_tab.data());
    if (!ctx->fixed_ok && fixed_len_wanted(ctx->prm) && getenv("PG_QUIET") == nullptr)
        fprintf(stderr, "pindel_pg: note: the length tables of these parameters differ from the ones the fixed-length kernels were "
                        "built for; this context runs the other kernels\n");
    if (dev_upload(ctx, &ctx->d_thr, ctx->thr, 512) || dev_upload(ctx, &ctx->d_mm, ctx->mm, 512) ||
        dev_upload(ctx, &ctx->d_len_tab, len_tab.data(), 512)) {
        pg_destroy(ctx);
        return PG_E_DEVICE;
    }
    {
        std::lock_guard<std::mutex> lk(g_ctx_mu);
        g_live_ctx++;
        ctx->counted = true;
    }
    *out = ctx;
    return PG_OK;
}

void pg_destroy(pg_ctx *ctx)
{
    use_device(ctx);
    if (!ctx) return;
    if (ctx->counted) {
        bool last;
        {
            std::lock_guard<std::mutex> lk(g_ctx_mu);
            last = --g_live_ctx == 0;
        }
        if (last) g_pinned.trim();                   // the page-locked result buffers cached for reuse
    }
    free_reference(ctx);
    if (ctx->arena.base) (void)hipFree(ctx->arena.base);
    if (ctx->d_thr) (void)hipFree(ctx->d_thr);
    if (ctx->d_mm) (void)hipFree(ctx->d_mm);
    if (ctx->d_sv_budget) (void)hipFree(ctx->d_sv_budget);
    if (ctx->d_len_tab) (void)hipFree(ctx->d_len_tab);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->evh0) (void)hipEventDestroy(ctx->evh0);
    if (ctx->evh1) (void)hipEventDestroy(ctx->evh1);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
    if (ctx->dl_stream) (void)hipStreamDestroy(ctx->dl_stream);
    if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
    for (hipEvent_t e : ctx->events) (void)hipEventDestroy(e);
    delete ctx;
}

const char *pg_last_error(const pg_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int pg_get_max_mismatch(const pg_ctx *ctx, uint32_t *table500)
{
    if (!ctx || !table500) return PG_E_INVALID;
    memcpy(table500, ctx->mm, 500 * sizeof(uint32_t));
    return PG_OK;
}

int pg_load_reference(pg_ctx *ctx, int32_t n_chr, const char *const *names,
                      const uint8_t *const *seq_padded, const uint64_t *len_padded)
{
    use_device(ctx);
    if (!ctx || n_chr <= 0 || !seq_padded || !len_padded) return fail(ctx, PG_E_INVALID, "bad reference arguments");
    if (n_chr > 32767) return fail(ctx, PG_E_UNSUPPORTED, "more than 32767 chromosomes");
    free_reference(ctx);
    uint64_t total_words = 0;
    for (int c = 0; c < n_chr; c++) {
        if (len_padded[c] > PG_MAX_CHR_PADDED) return fail(ctx, PG_E_UNSUPPORTED, "chromosome of 2^31 bases or more (positions are signed 32-bit on the device)");
        if (len_padded[c] < 2ull * ctx->prm.spacer) return fail(ctx, PG_E_INVALID, "chromosome shorter than its spacers");
        total_words += PG_GUARD_WORDS;
        ctx->word_off.push_back(total_words);
        total_words += (len_padded[c] + 31) / 32 + PG_GUARD_WORDS;
        ctx->names.push_back(names && names[c] ? names[c] : "");
        ctx->comp_size.push_back(len_padded[c]);
    }
    total_words += 8;
    try {
        ctx->h_lo.assign(total_words, 0u);
        ctx->h_hi.assign(total_words, 0u);
        ctx->h_nn.assign(total_words, 0xffffffffu);   // guards and tails are N
    } catch (...) {
        free_reference(ctx);
        return fail(ctx, PG_E_NOMEM, "host memory for the packed reference");
    }
    uint8_t code[256];
    memset(code, 4, sizeof code);
    code['A'] = 0; code['C'] = 1; code['G'] = 2; code['T'] = 3;
    for (int c = 0; c < n_chr; c++) {
        const uint8_t *s = seq_padded[c];
        const uint64_t len = len_padded[c];
        uint32_t *lo = &ctx->h_lo[ctx->word_off[c]], *hi = &ctx->h_hi[ctx->word_off[c]],
                 *nn = &ctx->h_nn[ctx->word_off[c]];
        const uint64_t n_words = (len + 31) / 32;
        // words are independent: pack on all host cores (a 3.1 Gbp genome is ~10 s single-threaded)
        auto pack = [&](uint64_t w0, uint64_t w1) {
            for (uint64_t w = w0; w < w1; w++) {
                uint32_t l = 0, h = 0, n = 0xffffffffu;
                const uint64_t b0 = w * 32, cnt = std::min<uint64_t>(32, len - b0);
                for (uint64_t k = 0; k < cnt; k++) {
                    uint8_t cd = code[s[b0 + k]];
                    if (cd < 4) {
                        l |= (uint32_t)(cd & 1u) << k;
                        h |= (uint32_t)(cd >> 1) << k;
                        n &= ~(1u << k);
                    }
                }
                lo[w] = l; hi[w] = h; nn[w] = n;
            }
        };
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        const unsigned nt = (unsigned)std::min<uint64_t>(hw, std::max<uint64_t>(1, n_words >> 16));
        if (nt <= 1) pack(0, n_words);
        else {
            std::vector<std::thread> th;
            for (unsigned t = 0; t < nt; t++)
                th.emplace_back(pack, n_words * t / nt, n_words * (t + 1) / nt);
            for (std::thread &x : th) x.join();
        }
    }
    return upload_reference(ctx);
}

int pg_load_reference_device(pg_ctx *ctx, int32_t n_chr, const char *const *names,
                             const uint8_t *const *d_seq_padded, const uint64_t *len_padded)
{
    use_device(ctx);
    if (!ctx || n_chr <= 0 || !d_seq_padded || !len_padded) return fail(ctx, PG_E_INVALID, "bad reference arguments");
    if (n_chr > 32767) return fail(ctx, PG_E_UNSUPPORTED, "more than 32767 chromosomes");
    return load_reference_device(ctx, n_chr, names, d_seq_padded, len_padded);
}

// ---- packed reference on disk: the bit planes exactly as they sit in HBM, so a
// genome is packed from FASTA once (Genome::loadChromosome semantics, pg_load_fasta) and mapped back
// in seconds.  Layout: magic, spacer, n_chr, per chromosome {name length, name, padded size, word
// offset}, number of words, then the lo / hi / N planes.
static const char PG_REF_MAGIC[8] = { 'P', 'G', 'R', 'E', 'F', '0', '1', 0 };

int pg_reference_save_packed(const pg_ctx *ctx, const char *path)
{
    if (!ctx || !path) return PG_E_INVALID;
    if (ctx->names.empty()) return PG_E_NO_REFERENCE;
    if (int rc = host_mirror(ctx)) return rc;
    FILE *f = fopen(path, "wb");
    if (!f) return PG_E_INVALID;
    bool ok = fwrite(PG_REF_MAGIC, 1, 8, f) == 8;
    const uint32_t spacer = ctx->prm.spacer, n_chr = (uint32_t)ctx->names.size();
    ok = ok && fwrite(&spacer, 4, 1, f) == 1 && fwrite(&n_chr, 4, 1, f) == 1;
    for (uint32_t c = 0; c < n_chr && ok; c++) {
        const uint32_t nl = (uint32_t)ctx->names[c].size();
        ok = fwrite(&nl, 4, 1, f) == 1 && (nl == 0 || fwrite(ctx->names[c].data(), 1, nl, f) == nl) &&
             fwrite(&ctx->comp_size[c], 8, 1, f) == 1 && fwrite(&ctx->word_off[c], 8, 1, f) == 1;
    }
    const uint64_t nw = ctx->h_lo.size();
    ok = ok && fwrite(&nw, 8, 1, f) == 1 && fwrite(ctx->h_lo.data(), 4, nw, f) == nw &&
         fwrite(ctx->h_hi.data(), 4, nw, f) == nw && fwrite(ctx->h_nn.data(), 4, nw, f) == nw;
    ok = (fclose(f) == 0) && ok;
    return ok ? PG_OK : PG_E_INVALID;
}

int pg_reference_load_packed(pg_ctx *ctx, const char *path)
{
    use_device(ctx);
    if (!ctx || !path) return fail(ctx, PG_E_INVALID, "bad packed-reference arguments");
    FILE *f = fopen(path, "rb");
    if (!f) return fail(ctx, PG_E_INVALID, std::string("cannot open ") + path);
    auto bad = [&](const char *why) {
        fclose(f);
        free_reference(ctx);
        return fail(ctx, PG_E_INVALID, std::string(path) + ": " + why);
    };
    free_reference(ctx);
    char magic[8];
    uint32_t spacer = 0, n_chr = 0;
    if (fread(magic, 1, 8, f) != 8 || memcmp(magic, PG_REF_MAGIC, 8) != 0) return bad("not a packed reference");
    if (fread(&spacer, 4, 1, f) != 1 || fread(&n_chr, 4, 1, f) != 1) return bad("truncated header");
    if (spacer != ctx->prm.spacer) return bad("packed with a different spacer");
    if (n_chr == 0 || n_chr > 32767) return bad("bad chromosome count");
    for (uint32_t c = 0; c < n_chr; c++) {
        uint32_t nl = 0;
        uint64_t size = 0, woff = 0;
        if (fread(&nl, 4, 1, f) != 1 || nl > 4096) return bad("bad chromosome name");
        std::string name(nl, ' ');
        if ((nl && fread(&name[0], 1, nl, f) != nl) || fread(&size, 8, 1, f) != 1 || fread(&woff, 8, 1, f) != 1)
            return bad("truncated chromosome table");
        if (size > PG_MAX_CHR_PADDED || size < 2ull * spacer) return bad("bad chromosome size (2^31 bases or more are not supported)");
        ctx->names.push_back(name);
        ctx->comp_size.push_back(size);
        ctx->word_off.push_back(woff);
    }
    uint64_t nw = 0, expect = 0;
    for (uint32_t c = 0; c < n_chr; c++) {
        expect += PG_GUARD_WORDS;
        if (ctx->word_off[c] != expect) return bad("inconsistent word offsets");
        expect += (ctx->comp_size[c] + 31) / 32 + PG_GUARD_WORDS;
    }
    expect += 8;
    if (fread(&nw, 8, 1, f) != 1 || nw != expect) return bad("inconsistent plane size");
    try {
        ctx->h_lo.resize(nw);
        ctx->h_hi.resize(nw);
        ctx->h_nn.resize(nw);
    } catch (...) {
        fclose(f);
        free_reference(ctx);
        return fail(ctx, PG_E_NOMEM, "host memory for the packed reference");
    }
    if (fread(ctx->h_lo.data(), 4, nw, f) != nw || fread(ctx->h_hi.data(), 4, nw, f) != nw ||
        fread(ctx->h_nn.data(), 4, nw, f) != nw)
        return bad("truncated planes");
    fclose(f);
    return upload_reference(ctx);
}

int pg_load_fasta(pg_ctx *ctx, const char *path)
{
    if (!ctx || !path) return fail(ctx, PG_E_INVALID, "bad fasta arguments");
    std::ifstream in(path, std::ios::binary);
    if (!in) return fail(ctx, PG_E_INVALID, std::string("cannot open ") + path);
    std::string data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    // Genome::loadChromosome (pindel.cpp:272-312): name = first token after '>', every
    // non-blank character is upper-cased, non-ACGT -> N, spacer N's both sides.  The
    // reference's extraction loop appends the final base of the LAST record twice.
    std::vector<std::string> names, seqs;
    size_t i = 0;
    const size_t n = data.size();
    while (i < n && isspace((unsigned char)data[i])) i++;
    if (i >= n || data[i] != '>') return fail(ctx, PG_E_INVALID, "fasta does not start with '>'");
    const std::string spacer(ctx->prm.spacer, 'N');
    while (i < n) {
        i++;   // '>'
        while (i < n && (data[i] == ' ' || data[i] == '\t')) i++;
        size_t j = i;
        while (j < n && !isspace((unsigned char)data[j])) j++;
        names.push_back(data.substr(i, j - i));
        while (j < n && data[j] != '\n') j++;
        std::string s = spacer;
        i = j;
        while (i < n && data[i] != '>') {
            unsigned char ch = (unsigned char)data[i++];
            if (isspace(ch)) continue;
            ch = (unsigned char)toupper(ch);
            if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T') ch = 'N';
            s.push_back((char)ch);
        }
        if (i >= n && s.size() > spacer.size()) s.push_back(s.back());
        s += spacer;
        seqs.push_back(std::move(s));
    }
    std::vector<const char *> np;
    std::vector<const uint8_t *> sp;
    std::vector<uint64_t> lp;
    for (size_t c = 0; c < seqs.size(); c++) {
        np.push_back(names[c].c_str());
        sp.push_back((const uint8_t *)seqs[c].data());
        lp.push_back(seqs[c].size());
    }
    return pg_load_reference(ctx, (int32_t)seqs.size(), np.data(), sp.data(), lp.data());
}

int pg_reference_n_chr(const pg_ctx *ctx) { return ctx ? (int)ctx->names.size() : 0; }

const char *pg_reference_name(const pg_ctx *ctx, int32_t c)
{
    return (ctx && c >= 0 && c < (int)ctx->names.size()) ? ctx->names[c].c_str() : nullptr;
}

uint64_t pg_reference_comp_size(const pg_ctx *ctx, int32_t c)
{
    return (ctx && c >= 0 && c < (int)ctx->names.size()) ? ctx->comp_size[c] : 0;
}

int pg_reference_fetch(const pg_ctx *ctx, int32_t c, uint64_t start, uint64_t n, uint8_t *out)
{
    if (!ctx || !out || c < 0 || c >= (int)ctx->names.size()) return PG_E_INVALID;
    if (start + n > ctx->comp_size[c]) return PG_E_INVALID;
    if (int rc = host_mirror(ctx)) return rc;
    const uint32_t *lo = &ctx->h_lo[ctx->word_off[c]], *hi = &ctx->h_hi[ctx->word_off[c]],
                   *nn = &ctx->h_nn[ctx->word_off[c]];
    for (uint64_t k = 0; k < n; k++) {
        uint64_t p = start + k;
        uint32_t w = (uint32_t)(p >> 5), b = (uint32_t)(p & 31);
        if ((nn[w] >> b) & 1u) out[k] = 'N';
        else out[k] = "ACGT"[((lo[w] >> b) & 1u) | (((hi[w] >> b) & 1u) << 1)];
    }
    return PG_OK;
}

// ---------------------------------------------------------------- device-resident
int pg_device_batch_upload(pg_ctx *ctx, const pg_read_batch *reads, pg_device_batch **out)
{
    use_device(ctx);
    if (!ctx || !out) return PG_E_INVALID;
    *out = nullptr;
    int rc = upload_batch(ctx, reads, out);
    if (rc) return rc;
    return read_exact_count(ctx, *out);
}

static int attach_windows(pg_ctx *ctx, pg_device_batch *b, const pg_windows *bd_hints, bool repack = true);

int pg_device_batch_set_windows(pg_ctx *ctx, pg_device_batch *b, const pg_windows *bd_hints)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    int rc = attach_windows(ctx, b, bd_hints);
    if (rc) return rc;
    return read_exact_count(ctx, b);
}

int pg_device_batch_search(pg_ctx *ctx, pg_device_batch *b)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    return run_search(ctx, b, PG_MODE_BOTH);
}

int pg_device_batch_pack_search(pg_ctx *ctx, pg_device_batch *b)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    int rc = run_search(ctx, b, PG_MODE_BOTH, true);
    if (rc) return rc;
    return b->exact_n < 0 ? read_exact_count(ctx, b) : PG_OK;      // (later searches of the batch skip the exact kernel when its list is empty)
}

int pg_device_batch_repack(pg_ctx *ctx, pg_device_batch *b, double *pack_ms)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    if (int stale = stale_batch(ctx, b)) return stale;
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    int rc = b->n ? pack_reads(ctx, b, 0, b->n) : PG_OK;
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    if (pack_ms) *pack_ms = ms;
    return read_exact_count(ctx, b);
}

int pg_device_batch_download(pg_ctx *ctx, pg_device_batch *b, pg_result **out)
{
    use_device(ctx);
    if (!ctx || !b || !out) return PG_E_INVALID;
    pg_result *r = new pg_result();
    int rc = download(ctx, b, r);
    if (rc) {
        delete r;
        return rc;
    }
    *out = r;
    return PG_OK;
}

// ---- device buffers in and out
int pg_device_batch_upload_device(pg_ctx *ctx, const pg_read_batch *d_reads, pg_device_batch **out)
{
    use_device(ctx);
    if (!ctx || !out) return PG_E_INVALID;
    *out = nullptr;
    int rc = upload_batch_device(ctx, d_reads, out);
    if (rc) return rc;
    return read_exact_count(ctx, *out);
}

int pg_device_batch_result_sizes(pg_ctx *ctx, pg_device_batch *b, uint64_t *n_close_runs, uint64_t *n_far_runs)
{
    use_device(ctx);
    if (!ctx || !b || !n_close_runs || !n_far_runs) return PG_E_INVALID;
    return result_sizes(ctx, b, n_close_runs, n_far_runs);
}

int pg_device_batch_download_device(pg_ctx *ctx, pg_device_batch *b, const pg_device_result *dst)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    if (!dst) return fail(ctx, PG_E_INVALID, "null pg_device_result");
    const size_t n = b->n;
    int rc;
    // (the run buffers are checked once the totals are known: a list without a run needs none)
    if ((rc = check_device_ptr(ctx, dst->close_off, (n + 1) * 8, 8, "pg_device_result.close_off")) ||
        (rc = check_device_ptr(ctx, dst->far_off, (n + 1) * 8, 8, "pg_device_result.far_off")) ||
        (dst->rc_flag && (rc = check_device_ptr(ctx, dst->rc_flag, n, 1, "pg_device_result.rc_flag"))) ||
        (dst->close_last && (rc = check_device_ptr(ctx, dst->close_last, n * 4, 4, "pg_device_result.close_last"))) ||
        (dst->close_max && (rc = check_device_ptr(ctx, dst->close_max, n * 2, 2, "pg_device_result.close_max"))))
        return rc;
    return download_device(ctx, b, dst);
}

void pg_device_batch_free(pg_ctx *ctx, pg_device_batch *b)
{
    use_device(ctx);
    (void)ctx;
    if (!b) return;
    free_batch_buffers(b);
    delete b;
}

// Diagnostics (not in the public header): did the last launch that was asked to pack build its records inside the search kernel ?
int pg_debug_last_pack_in_place(const pg_ctx *ctx) { return ctx && ctx->last_in_place ? 1 : 0; }
// ... and the read length of the fixed-length kernel the last search launch ran (0: it ran any other kernel, or none yet)
uint32_t pg_debug_last_fixed_len(const pg_ctx *ctx) { return ctx ? ctx->last_fixed_len.load(std::memory_order_relaxed) : 0u; }

// Diagnostics (not in the public header): the launch log -- the kernels the search path launched since the last
// pg_debug_clear_launch_log, seven int32 per launch (PgLaunchRec: kernel, NB / PB, NS, id bits, mode, DEF, packed in place).
// Writes the first min(count, cap, PG_LAUNCH_LOG_CAP) records to out (may be null) and returns the count of launches logged.
// Like every debug hook: not while a pg_* call is in flight on the context.
int32_t pg_debug_launch_log(const pg_ctx *ctx, int32_t *out, int32_t cap)
{
    if (!ctx) return PG_E_INVALID;
    const uint32_t n = ctx->launch_n.load(std::memory_order_relaxed);
    const uint32_t k = std::min<uint32_t>(std::min<uint32_t>(n, pg_ctx::PG_LAUNCH_LOG_CAP), cap > 0 ? (uint32_t)cap : 0u);
    static_assert(sizeof(PgLaunchRec) == 7 * sizeof(int32_t), "seven int32 per record");
    if (out && k) std::memcpy(out, ctx->launch_log, (size_t)k * sizeof(PgLaunchRec));
    return (int32_t)std::min<uint32_t>(n, 0x7fffffffu);
}

void pg_debug_clear_launch_log(pg_ctx *ctx)
{
    if (ctx) ctx->launch_n.store(0u, std::memory_order_relaxed);
}

// Diagnostics (not in the public header): overwrites the batch's packed records and bit planes (tests: what a search that packs in
// place finds afterwards is what it packed itself).
int pg_debug_scribble_records(pg_ctx *ctx, pg_device_batch *b)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    const size_t n1 = std::max<size_t>(b->n, 1);
    HIP_TRY(ctx, hipMemsetAsync(b->in_rec, 0xa5, n1 * sizeof(PgInRec), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(b->planes, 0x5a, n1 * 64 * pg_plane_blocks(b->max_len), ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

// Diagnostics (not in the public header): the `reserved` word of every output record (candidates per read; in a
// -DPG_DIAG build the packed per-read counters).
int pg_debug_read_reserved(pg_ctx *ctx, pg_device_batch *b, uint32_t *out, uint32_t n)
{
    use_device(ctx);
    if (!ctx || !b || !out || n > b->n) return PG_E_INVALID;
    std::vector<PgOutRec> recs(n);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (n) HIP_TRY(ctx, hipMemcpy(recs.data(), b->out_rec, (size_t)n * sizeof(PgOutRec), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++) out[i] = recs[i].reserved;
    return PG_OK;
}

// Diagnostics (-DPG_TIMING builds of the kernel): wave-cycles per phase of the last launch on this batch.
int pg_debug_read_phase_cycles(pg_ctx *ctx, pg_device_batch *b, uint64_t *out, uint32_t n)
{
    use_device(ctx);
    if (!ctx || !b || !out || n > PG_DIAG_WORDS) return PG_E_INVALID;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out, b->pool_used + PG_POOL_SHARDS * 16 + PG_WORK_CTRS * 16, (size_t)n * 8, hipMemcpyDeviceToHost));
    return PG_OK;
}

int pg_last_search_stats(const pg_ctx *ctx, double *kernel_ms, uint64_t *n_runs)
{
    if (!ctx) return PG_E_INVALID;
    if (kernel_ms) *kernel_ms = ctx->last_ms;
    if (n_runs) *n_runs = ctx->last_runs;
    return PG_OK;
}

// The output records of the batch's last search, for the two diagnostics below.
static int fetch_out_recs(pg_ctx *ctx, pg_device_batch *b, std::vector<PgOutRec> &recs)
{
    recs.resize(b->n);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (b->n) HIP_TRY(ctx, hipMemcpy(recs.data(), b->out_rec, (size_t)b->n * sizeof(PgOutRec), hipMemcpyDeviceToHost));
    return PG_OK;
}

// Diagnostics: candidates (survivors of the seed filter) the last search of this batch folded, in total.
int pg_device_batch_candidates(pg_ctx *ctx, pg_device_batch *b, double *n_candidates)
{
    use_device(ctx);
    if (!ctx || !b || !n_candidates) return PG_E_INVALID;
    std::vector<PgOutRec> recs;
    if (int rc = fetch_out_recs(ctx, b, recs)) return rc;
    double s = 0.0;
    for (const PgOutRec &r : recs) s += r.reserved;
    *n_candidates = s;
    return PG_OK;
}

int pg_device_batch_algorithmic_bytes(pg_ctx *ctx, pg_device_batch *b, double *bytes)
{
    use_device(ctx);
    if (!ctx || !b || !bytes) return PG_E_INVALID;
    std::vector<PgOutRec> recs;
    if (int rc = fetch_out_recs(ctx, b, recs)) return rc;
    double s = 0.0;
    for (const PgOutRec &r : recs) s += r.alg;
    *bytes = s;
    return PG_OK;
}

int pg_close_end_batch(pg_ctx *ctx, const pg_read_batch *reads, pg_result **out)
{
    return search_host(ctx, reads, PG_MODE_CLOSE, out);
}

int pg_search_batch(pg_ctx *ctx, const pg_read_batch *reads, pg_result **out)
{
    const double t0 = now_ms();
    const int rc = search_host(ctx, reads, PG_MODE_BOTH, out);
    if (g_host_timing) fprintf(stderr, "pg_search_batch: %.2f ms in all\n", now_ms() - t0);
    return rc;
}

// reads [lo, hi) of a batch; the offsets of a slice need not start at 0
static pg_read_batch slice(const pg_read_batch &reads, uint32_t lo, uint32_t hi)
{
    pg_read_batch sub = reads;
    sub.n_reads = hi - lo;
    sub.seq_off += lo;
    sub.anchor_strand += lo;
    sub.anchor_pos += lo;
    sub.insert_size += lo;
    sub.chr_id += lo;
    return sub;
}

int pg_search_batch_multi(pg_ctx *const *ctxs, int32_t n_ctx, const pg_read_batch *reads, pg_result **out)
{
    if (!ctxs || n_ctx <= 0 || !reads || !out) return PG_E_INVALID;
    for (int k = 0; k < n_ctx; k++)
        if (!ctxs[k]) return PG_E_INVALID;
    *out = nullptr;
    const uint32_t n = reads->n_reads;
    if (n_ctx == 1 || n < 2u * (uint32_t)n_ctx) return search_host(ctxs[0], reads, PG_MODE_BOTH, out);
    // contiguous ranges, one host thread per context
    std::vector<pg_result *> parts((size_t)n_ctx, nullptr);
    std::vector<int> rcs((size_t)n_ctx, PG_OK);
    std::vector<std::thread> th;
    for (int k = 0; k < n_ctx; k++)
        th.emplace_back([&, k]() {
            const uint32_t lo = (uint32_t)((uint64_t)n * k / n_ctx), hi = (uint32_t)((uint64_t)n * (k + 1) / n_ctx);
            const pg_read_batch sub = slice(*reads, lo, hi);
            rcs[(size_t)k] = search_host(ctxs[k], &sub, PG_MODE_BOTH, &parts[(size_t)k]);
        });
    for (std::thread &t : th) t.join();
    int rc = PG_OK;
    for (int k = 0; k < n_ctx; k++)
        if (rcs[(size_t)k]) rc = rcs[(size_t)k];
    pg_result *r = nullptr;
    if (rc == PG_OK) {
        r = new pg_result();
        r->n = n;
        uint64_t tc = 0, tf = 0;
        for (pg_result *p : parts) {
            tc += p->close_runs.size();
            tf += p->far_runs.size();
        }
        if (!r->close_off.resize((size_t)n + 1) || !r->far_off.resize((size_t)n + 1) || !r->rc_flag.resize(n) ||
            !r->close_last.resize(n) || !r->close_max.resize(n) || !r->close_runs.resize(tc) || !r->far_runs.resize(tf)) {
            delete r;
            r = nullptr;
            rc = fail(ctxs[0], PG_E_NOMEM, "pinned host memory for the merged result");
        }
    }
    if (r) {
        uint64_t bc = 0, bf = 0;
        size_t at = 0;
        bool summaries = true;
        for (pg_result *p : parts) {
            const size_t m = p->n;
            for (size_t i = 0; i < m; i++) {
                r->close_off[at + i] = bc + p->close_off[i];
                r->far_off[at + i] = bf + p->far_off[i];
            }
            if (m) {
                memcpy(r->rc_flag.data() + at, p->rc_flag.data(), m);
                if (p->close_last.size() == m && p->close_max.size() == m) {
                    memcpy(r->close_last.data() + at, p->close_last.data(), m * 4);
                    memcpy(r->close_max.data() + at, p->close_max.data(), m * 2);
                } else
                    summaries = false;
            }
            if (p->close_runs.size()) memcpy(r->close_runs.data() + bc, p->close_runs.data(), p->close_runs.size() * sizeof(pg_run));
            if (p->far_runs.size()) memcpy(r->far_runs.data() + bf, p->far_runs.data(), p->far_runs.size() * sizeof(pg_run));
            bc += p->close_runs.size();
            bf += p->far_runs.size();
            at += m;
        }
        r->close_off[n] = bc;
        r->far_off[n] = bf;
        if (!summaries) {
            r->close_last.resize(0);
            r->close_max.resize(0);
        }
    }
    for (pg_result *p : parts) delete p;
    *out = r;
    return rc;
}

// ---------------------------------------------------------------- window hints and the far end
// Windows are made ready by pg_window_plan (pg_window_plan.h): validated, and a window of 2^26 positions or more (the width of
// the position field) cut into consecutive pieces -- the reduction over candidates is additive over disjoint position sets.
static const char *window_error(PgWindowStatus s, const char *offsets_not_monotone)
{
    return s == PG_WINDOWS_OFFSETS_NOT_MONOTONE ? offsets_not_monotone
           : s == PG_WINDOWS_NULL_ARRAY         ? "null window array"
                                                : "BreakDancer window on unknown chromosome";
}

// Every attach starts here: the batch is left without windows.
static int clear_windows(pg_ctx *ctx, pg_device_batch *b)
{
    if (int stale = stale_batch(ctx, b)) return stale;
    if (b->bd_off) { (void)hipFree(b->bd_off); b->bd_off = nullptr; }
    if (b->bd) { (void)hipFree(b->bd); b->bd = nullptr; }
    b->max_bd_window = 0;
    b->max_bd_cluster = 0;
    return PG_OK;
}

// ... and passes here before it keeps any: the windows of the batch in all, and the most of one read.
static int window_limits(pg_ctx *ctx, uint64_t in_batch, uint64_t in_cluster)
{
    if (pg_too_many_windows(in_batch)) return fail(ctx, PG_E_UNSUPPORTED, "more than 2^32 BreakDancer windows in a batch");
    if (pg_too_many_in_cluster(in_cluster)) return fail(ctx, PG_E_UNSUPPORTED, "more than 2^29 windows in a BreakDancer cluster");
    return PG_OK;
}

// Validates per-read window clusters and uploads them to the batch (replacing earlier ones).  Nothing the reference
// accepts is refused: BDData::getCorrespondingSearchWindowCluster (src/bddata.cpp:949-979) has no cap on the windows of
// a cluster -- clusters of more than 127 windows switch the launch to 64-bit candidate ids (29 bits of window index) --
// and a long window is searched as pieces.  A batch without a long window is uploaded from the caller's arrays: no copy.
// repack = false: the caller's next search launch packs the batch itself (launch_range with pack)
static int attach_windows(pg_ctx *ctx, pg_device_batch *b, const pg_windows *bd_hints, bool repack)
{
    const size_t n = b->n;
    int rc = clear_windows(ctx, b);
    if (rc) return rc;
    if (!(bd_hints && bd_hints->offset && n)) return n && repack ? pack_reads(ctx, b, 0, b->n) : PG_OK;
    const PgWindowPlan p = pg_window_plan(bd_hints->offset, n, bd_hints->windows, (int)ctx->names.size(), false, nullptr);
    if (p.status) return fail(ctx, PG_E_INVALID, window_error(p.status, "window offsets not monotone"));
    const uint64_t *off = p.offsets(bd_hints->offset);
    if ((rc = window_limits(ctx, off[n], p.largest_group))) return rc;
    b->max_bd_cluster = p.largest_group;
    b->max_bd_window = p.longest;
    if ((rc = dev_upload(ctx, &b->bd_off, off, n + 1)) || (rc = dev_upload(ctx, &b->bd, p.windows(bd_hints->windows), (size_t)off[n])))
        return rc;
    return repack ? pack_reads(ctx, b, 0, b->n) : PG_OK;
}

// A pg_hint_table validated, its windows split into pieces the position field of a candidate id can hold (once per cluster
// window, as attach_windows does per read), in device memory for the lifetime of one call.  The five arrays of `t` are owned here.
struct HintTableDev {
    PgDevHintTable t{};
    uint64_t bytes = 0;
    HintTableDev() = default;
    HintTableDev(const HintTableDev &) = delete;
    ~HintTableDev()
    {
        for (const void *p : { (const void *)t.run_first, (const void *)t.run_cluster, (const void *)t.cluster_off,
                               (const void *)t.cluster_longest, (const void *)t.windows })
            if (p) (void)hipFree(const_cast<void *>(p));
    }
    bool live() const { return t.n_runs != 0; }
};

// Everything that can be wrong with a table is found here, before anything is launched.  A null table or one without runs
// leaves d without runs: "no hints".
static int upload_hint_table(pg_ctx *ctx, const pg_hint_table *table, HintTableDev &d)
{
    if (!table || !table->n_runs) return PG_OK;
    if (ctx->names.empty()) return fail(ctx, PG_E_NO_REFERENCE, "no reference loaded");
    const uint32_t nr = table->n_runs, nc = table->n_clusters;
    if (!table->run_first || !table->run_cluster) return fail(ctx, PG_E_INVALID, "hint table: null run arrays");
    if (nc && !table->cluster_off) return fail(ctx, PG_E_INVALID, "hint table: null cluster offsets");
    for (uint32_t k = 0; k < nr; k++)
        if (table->run_first[k + 1] <= table->run_first[k]) return fail(ctx, PG_E_INVALID, "hint table: run_first not strictly ascending");
    for (uint32_t k = 0; k < nr; k++)
        if (table->run_cluster[k] >= nc) return fail(ctx, PG_E_INVALID, "hint table: run_cluster names a cluster the table does not have");
    std::vector<uint32_t> longest;
    const PgWindowPlan p = pg_window_plan(table->cluster_off, nc, table->windows, (int)ctx->names.size(), true, &longest);
    if (p.status) return fail(ctx, PG_E_INVALID, window_error(p.status, "hint table: cluster_off not monotone"));
    int rc;
    if ((rc = dev_upload(ctx, const_cast<uint32_t **>(&d.t.run_first), table->run_first, nr + (size_t)1)) ||
        (rc = dev_upload(ctx, const_cast<uint32_t **>(&d.t.run_cluster), table->run_cluster, nr)) ||
        (rc = dev_upload(ctx, const_cast<uint64_t **>(&d.t.cluster_off), p.off.data(), p.off.size())) ||
        (rc = dev_upload(ctx, const_cast<uint32_t **>(&d.t.cluster_longest), longest.data(), longest.size())) ||
        (rc = dev_upload(ctx, const_cast<pg_window **>(&d.t.windows), p.win.data(), p.win.size())))
        return rc;
    d.t.n_runs = nr;
    d.bytes = (nr + 1ull) * 4 + (uint64_t)nr * 4 + p.off.size() * 8 + longest.size() * 4 + p.win.size() * sizeof(pg_window);
    return PG_OK;
}

// The per-read window clusters of the batch from a hint table and the close-end summary in the batch's device arrays
// (close_last / close_max): what attach_windows builds from a host CSR, built by the three kernels of pg_hints.hip.  The host
// waits once, for 16 bytes: the total and the two maxima attach_windows would have computed.  The far launch that follows packs
// the batch itself.
static int attach_table(pg_ctx *ctx, pg_device_batch *b, const HintTableDev &d)
{
    const uint32_t n = b->n;
    int rc = clear_windows(ctx, b);
    if (rc) return rc;
    ctx->hint_fill_timed = false;
    ctx->hint_scan_ms = ctx->hint_fill_ms = 0.0;
    ctx->hint_table_bytes = d.bytes;
    ctx->hint_windows = 0;
    if (!n || !d.live()) return PG_OK;
    if (!ctx->evh0) HIP_TRY(ctx, hipEventCreate(&ctx->evh0));
    if (!ctx->evh1) HIP_TRY(ctx, hipEventCreate(&ctx->evh1));
    if ((rc = dev_alloc(ctx, &b->bd_off, (size_t)n + 1))) return rc;
    uint32_t info[4] = { 0u, 0u, 0u, 0u };
    {
        DevTemps tmp(ctx, b);
        unsigned long long *blk = (unsigned long long *)tmp.take((size_t)pg_hint_scan_blocks(n) * 8);
        uint32_t *d_info = (uint32_t *)tmp.take(sizeof info);
        if (!blk || !d_info) return fail(ctx, PG_E_NOMEM, "device memory for the hint lookup's scan");
        HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        if (int e = pg_hint_count_scan(&d.t, b->close_last, b->close_max, n, (unsigned long long *)b->bd_off, blk, d_info, ctx->stream))
            return fail(ctx, PG_E_DEVICE, std::string("hint count / scan kernels: ") + hipGetErrorString((hipError_t)e));
        HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(info, d_info, sizeof info, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        float ms = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        ctx->hint_scan_ms = ms;
    }
    const uint64_t total = (uint64_t)info[0] | ((uint64_t)info[1] << 32);
    if ((rc = window_limits(ctx, total, info[2]))) return rc;
    b->max_bd_cluster = info[2];
    b->max_bd_window = info[3];
    ctx->hint_windows = total;
    if ((rc = dev_alloc(ctx, &b->bd, (size_t)total))) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->evh0, ctx->stream));
    if (int e = pg_hint_fill(&d.t, b->close_last, b->close_max, n, (const unsigned long long *)b->bd_off, b->bd, ctx->stream))
        return fail(ctx, PG_E_DEVICE, std::string("hint fill kernel: ") + hipGetErrorString((hipError_t)e));
    HIP_TRY(ctx, hipEventRecord(ctx->evh1, ctx->stream));
    ctx->hint_fill_timed = true;
    return PG_OK;
}

// ... and once the far launch behind the fill has been waited for: the fill's duration (no wait of its own)
static void note_hint_fill(pg_ctx *ctx)
{
    if (!ctx->hint_fill_timed) return;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->evh0, ctx->evh1) == hipSuccess) ctx->hint_fill_ms = ms;
    ctx->hint_fill_timed = false;
}

// The hints of one far end, in either form: a table with runs is looked up on the device, per-read windows are attached
// otherwise (both null: no hints).
struct FarHints {
    const pg_windows *per_read;
    const HintTableDev *table;
};

// The far end of a batch whose close-end summary (rc_flag, close_last, close_max) is in its device arrays: the output records
// back to that summary alone (no runs in the pool any more), the windows, the far launch -- which packs the reads -- and the
// download.  far_off / far_runs of `dst` are replaced; summaries: rc_flag, close_last and close_max of `dst` as well.
static int far_end_of_batch(pg_ctx *ctx, pg_device_batch *b, FarHints hints, pg_result *dst, bool summaries)
{
    if (b->n) {
        const PgSoaOut a = soa_out(b);
        if (pg_pack_close_summary(&a, b->out_rec, b->n, ctx->stream) != 0)
            return fail(ctx, PG_E_DEVICE, "close-end summary pack kernel failed");
    }
    int rc;
    if ((rc = hints.table && hints.table->live() ? attach_table(ctx, b, *hints.table) : attach_windows(ctx, b, hints.per_read, false)) ||
        (rc = run_search(ctx, b, PG_MODE_FAR, true)))
        return rc;
    note_hint_fill(ctx);
    pg_result tmp;
    if ((rc = download(ctx, b, &tmp))) return rc;
    dst->far_off.swap(tmp.far_off);
    dst->far_runs.swap(tmp.far_runs);
    if (summaries) {
        dst->rc_flag.swap(tmp.rc_flag);
        dst->close_last.swap(tmp.close_last);
        dst->close_max.swap(tmp.close_max);
    }
    return PG_OK;
}

// Far end of `reads` given each read's close-end summary (host arrays; rc_flag may be null = the sequences are
// already in the orientation GetCloseEnd left them in).  far_off / far_runs of `dst` are replaced.
static int far_end_impl(pg_ctx *ctx, const pg_read_batch *reads, const uint8_t *rc_flag, const uint32_t *close_last,
                        const uint16_t *close_max, FarHints hints, pg_result *dst)
{
    BatchGuard g;
    HostBuf<uint64_t> off0;
    int rc = alloc_batch(ctx, reads, true, off0, &g.b, true);
    if (rc) return rc;
    pg_device_batch *b = g.b;
    const size_t n = b->n;
    // (the output block of the batch, rc_flag included, was zeroed by alloc_batch; the records are packed by the search launch)
    if (n && ((rc_flag && hipMemcpyAsync(b->rc_flag, rc_flag, n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) ||
              hipMemcpyAsync(b->close_last, close_last, n * 4, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
              hipMemcpyAsync(b->close_max, close_max, n * 2, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
              hipStreamSynchronize(ctx->stream) != hipSuccess))       // the host arrays may be pageable temporaries
        return fail(ctx, PG_E_DEVICE, "upload of close-end summary failed");
    if ((rc = far_end_of_batch(ctx, b, hints, dst, false))) return rc;
    g.ok = true;
    return PG_OK;
}

// pg_far_end_batch and pg_far_end_batch_table: at most one of bd_hints and table is given
static int far_end_batch(pg_ctx *ctx, const pg_read_batch *reads, pg_result *close, const pg_windows *bd_hints, const pg_hint_table *table)
{
    use_device(ctx);
    if (!ctx || !reads || !close) return PG_E_INVALID;
    if (close->n != reads->n_reads) return fail(ctx, PG_E_INVALID, "close result does not belong to these reads");
    const size_t n = reads->n_reads;
    if (n && (close->rc_flag.size() != n || close->close_last.size() != n || close->close_max.size() != n))
        return fail(ctx, PG_E_INVALID, "close result carries no close-end summary");
    HintTableDev d;
    if (int rc = upload_hint_table(ctx, table, d)) return rc;
    return far_end_impl(ctx, reads, close->rc_flag.data(), close->close_last.data(), close->close_max.data(), { bd_hints, &d }, close);
}

int pg_far_end_batch(pg_ctx *ctx, const pg_read_batch *reads, pg_result *close, const pg_windows *bd_hints)
{
    return far_end_batch(ctx, reads, close, bd_hints, nullptr);
}

int pg_far_end_batch_table(pg_ctx *ctx, const pg_read_batch *reads, pg_result *close, const pg_hint_table *table)
{
    return far_end_batch(ctx, reads, close, nullptr, table);
}

static int far_end_from_close(pg_ctx *ctx, const pg_read_batch *reads, const uint32_t *close_last, const int16_t *close_max,
                              const pg_windows *bd_hints, const pg_hint_table *table, pg_result **out)
{
    use_device(ctx);
    if (!ctx || !reads || !out) return PG_E_INVALID;
    *out = nullptr;
    HintTableDev d;
    if (int trc = upload_hint_table(ctx, table, d)) return trc;
    const size_t n = reads->n_reads;
    if (n && (!close_last || !close_max)) return fail(ctx, PG_E_INVALID, "null close-end summary");
    // MaxLenCloseEnd() of a read without UP_Close is 0: such a read is not searched (farend_searcher.cpp:60-66)
    std::vector<uint16_t> cmax(n);
    for (size_t i = 0; i < n; i++) cmax[i] = close_max[i] > 0 ? (uint16_t)close_max[i] : (uint16_t)0;
    pg_result *r = new pg_result();
    r->n = (uint32_t)n;
    if (!r->close_off.assign(n + 1, 0) || !r->rc_flag.assign(n, 0) || !r->close_last.resize(n) || !r->close_max.resize(n)) {
        delete r;
        return fail(ctx, PG_E_NOMEM, "pinned host memory for the result");
    }
    r->close_runs.resize(0);
    for (size_t i = 0; i < n; i++) {
        r->close_last[i] = close_last[i];
        r->close_max[i] = cmax[i];
    }
    int rc = far_end_impl(ctx, reads, nullptr, close_last, cmax.data(), { bd_hints, &d }, r);
    if (rc) {
        delete r;
        return rc;
    }
    *out = r;
    return PG_OK;
}

int pg_far_end_batch_from_close(pg_ctx *ctx, const pg_read_batch *reads, const uint32_t *close_last,
                                const int16_t *close_max, const pg_windows *bd_hints, pg_result **out)
{
    return far_end_from_close(ctx, reads, close_last, close_max, bd_hints, nullptr, out);
}

int pg_far_end_batch_from_close_table(pg_ctx *ctx, const pg_read_batch *reads, const uint32_t *close_last,
                                      const int16_t *close_max, const pg_hint_table *table, pg_result **out)
{
    return far_end_from_close(ctx, reads, close_last, close_max, nullptr, table, out);
}

// Close end, lookup and far end of one batch: the reads are uploaded once; the close runs are delivered to the host before the
// far launch (run_search zeroes the run-pool cursors per launch), the close-end SUMMARY -- what the lookup and the far end read --
// stays in the batch's device arrays and reaches the host with the far end's results.
int pg_search_batch_table(pg_ctx *ctx, const pg_read_batch *reads, const pg_hint_table *table, pg_result **out)
{
    use_device(ctx);
    if (!ctx || !reads || !out) return PG_E_INVALID;
    *out = nullptr;
    HintTableDev d;
    int rc = upload_hint_table(ctx, table, d);
    if (rc) return rc;
    if (!d.live() || !reads->n_reads) return pg_search_batch(ctx, reads, out);      // (no hints, or nobody to look up)
    BatchGuard g;
    HostBuf<uint64_t> off0;
    if ((rc = alloc_batch(ctx, reads, true, off0, &g.b, true))) return rc;
    if ((rc = run_search(ctx, g.b, PG_MODE_CLOSE, true))) return rc;
    g.r = new pg_result();
    if ((rc = download(ctx, g.b, g.r, false)) || (rc = far_end_of_batch(ctx, g.b, { nullptr, &d }, g.r, true))) return rc;
    *out = g.r;
    g.r = nullptr;
    g.ok = true;
    return PG_OK;
}

// The same on a resident batch, with both run lists left in the pool: the far launch does not zero the pool
// cursors, so its runs go behind the close launch's, and it writes only the far fields of the output records -- the batch ends
// as a fused search leaves it.  A pool that overflowed in either launch is regrown and everything is done again from the close
// launch: the regrown pool has lost the close runs.
int pg_device_batch_search_table(pg_ctx *ctx, pg_device_batch *b, const pg_hint_table *table)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    HintTableDev d;
    int rc = upload_hint_table(ctx, table, d);
    if (rc) return rc;
    if (!d.live() || !b->n) {                   // no hints, or nobody to look up: the fused search of a batch without windows
        // (attach_table without a lookup: the windows of an earlier call detached, the hint statistics zero)
        if ((rc = search_refusals(ctx, b)) || (rc = attach_table(ctx, b, d))) return rc;
        return pg_device_batch_pack_search(ctx, b);
    }
    if ((rc = search_refusals(ctx, b))) return rc;
    b->searched = b->close_searched = false;
    b->cls.drop_search_tables();
    // each launch reserves its PG_RESERVE slots per read, and the batch's pool was sized for one: room for both from the start,
    // or every batch of more than ~87 000 reads would overflow once and run three times (PG_TEST_TINY_POOL: the regrow path)
    const uint64_t two_launches = ((2ull * PG_RESERVE + 2ull) * b->n) / PG_POOL_SHARDS + 512ull;
    if (!env().tiny_pool && b->pool_shard_cap < two_launches && (rc = grow_pool(ctx, b, two_launches))) return rc;
    const PgSoaOut a = soa_out(b);
    for (int attempt = 0; attempt < 8; attempt++) {
        float ms_close = 0.f, ms_far = 0.f;
        uint32_t worst = 0;
        uint64_t total = 0;
        // (the close end reads no windows: those of an earlier call go first, so that they have no say in the launch's kernels)
        if ((rc = clear_windows(ctx, b))) return rc;
        HIP_TRY(ctx, hipMemsetAsync(b->pool_used, 0, PG_POOL_SHARDS * 16 * sizeof(uint32_t), ctx->stream));
        if ((rc = search_launch(ctx, b, PG_MODE_CLOSE, true, &ms_close, &worst, &total))) return rc;
        if (worst <= b->pool_shard_cap) {
            if (pg_unpack_close_summary(b->out_rec, &a, b->n, ctx->stream) != 0)
                return fail(ctx, PG_E_DEVICE, "close-end summary kernel failed");
            if ((rc = attach_table(ctx, b, d)) || (rc = search_launch(ctx, b, PG_MODE_FAR, true, &ms_far, &worst, &total))) return rc;
            note_hint_fill(ctx);
        }
        if (worst <= b->pool_shard_cap) {
            ctx->last_ms = (double)ms_close + (double)ms_far;
            ctx->last_runs = total;
            b->searched = b->close_searched = true;
            return b->exact_n < 0 ? read_exact_count(ctx, b) : PG_OK;
        }
        if ((rc = grow_pool(ctx, b, (uint64_t)worst + worst / 4 + 64))) return rc;
    }
    return fail(ctx, PG_E_DEVICE, "run pool kept overflowing");
}

// The close half of the above on its own: the batch ends close-searched (its records and pool hold the close end alone), which is
// what the DD tables read; `searched` goes, so everything that needs both ends refuses the batch.
int pg_device_batch_close_search(pg_ctx *ctx, pg_device_batch *b)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    int rc;
    if ((rc = search_refusals(ctx, b))) return rc;
    b->searched = b->close_searched = false;
    b->cls.drop_search_tables();
    const PgSoaOut a = soa_out(b);
    for (int attempt = 0; attempt < 8; attempt++) {
        float ms = 0.f;
        uint32_t worst = 0;
        uint64_t total = 0;
        // (the close end reads no windows: those of an earlier call go first, so that they have no say in the launch's kernels)
        if ((rc = clear_windows(ctx, b))) return rc;
        HIP_TRY(ctx, hipMemsetAsync(b->pool_used, 0, PG_POOL_SHARDS * 16 * sizeof(uint32_t), ctx->stream));
        if ((rc = search_launch(ctx, b, PG_MODE_CLOSE, true, &ms, &worst, &total))) return rc;
        if (worst <= b->pool_shard_cap) {
            if (b->n && pg_unpack_close_summary(b->out_rec, &a, b->n, ctx->stream) != 0)
                return fail(ctx, PG_E_DEVICE, "close-end summary kernel failed");
            // (the far half of the records is not this launch's to write: what an earlier full search left there names pool slots
            // that the close runs have taken by now.  The two far words of every 32-byte record go to zero: no far end)
            static_assert(sizeof(PgOutRec) == 32 && offsetof(PgOutRec, far_off) == 8 && offsetof(PgOutRec, far_cnt) == 12, "the far words of a record");
            if (b->n) HIP_TRY(ctx, hipMemset2DAsync((char *)b->out_rec + offsetof(PgOutRec, far_off), sizeof(PgOutRec), 0, 8, b->n, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            ctx->last_ms = (double)ms;
            ctx->last_runs = total;
            b->close_searched = true;
            return b->exact_n < 0 ? read_exact_count(ctx, b) : PG_OK;
        }
        if ((rc = grow_pool(ctx, b, (uint64_t)worst + worst / 4 + 64))) return rc;
    }
    return fail(ctx, PG_E_DEVICE, "run pool kept overflowing");
}

int pg_debug_last_hint_stats(const pg_ctx *ctx, double *scan_ms, double *fill_ms, uint64_t *table_bytes, uint64_t *n_windows)
{
    if (!ctx) return PG_E_INVALID;
    if (scan_ms) *scan_ms = ctx->hint_scan_ms;
    if (fill_ms) *fill_ms = ctx->hint_fill_ms;
    if (table_bytes) *table_bytes = ctx->hint_table_bytes;
    if (n_windows) *n_windows = ctx->hint_windows;
    return PG_OK;
}

int pg_result_view_get(const pg_result *r, pg_result_view *v)
{
    if (!r || !v) return PG_E_INVALID;
    v->n_reads = r->n;
    v->close_off = r->close_off.data();
    v->close_runs = r->close_runs.data();
    v->far_off = r->far_off.data();
    v->far_runs = r->far_runs.data();
    v->rc_flag = r->rc_flag.data();
    return PG_OK;
}

void pg_result_free(pg_result *r) { delete r; }

uint64_t pg_expand_runs(const pg_run *runs, uint64_t n_runs, pg_point *out)
{
    uint64_t k = 0;
    for (uint64_t i = 0; i < n_runs; i++) {
        const pg_run &r = runs[i];
        const bool back = r.flags & PG_RUN_BACKWARD;
        for (uint32_t L = r.len_first; L <= r.len_last; L++, k++) {
            if (!out) continue;
            pg_point &p = out[k];
            uint32_t d = L - r.len_first;
            p.abs_loc = back ? r.abs_loc_first - d : r.abs_loc_first + d;
            p.length = (int16_t)L;
            p.mismatches = r.mismatches;
            p.chr_id = r.chr_id;
            p.direction = back ? '-' : '+';
            p.strand = (r.flags & PG_RUN_ANTISENSE) ? '-' : '+';
        }
    }
    return k;
}

// -q (dispersed duplications): contains_subseq_any_strand(query, window, 15) per item on the device (pg_dd.hip).  The windows
// are read from the reference planes already in HBM; only the queries and five numbers per item are uploaded.  Not on the
// search path: no launch-log record.
int pg_dd_contains_batch(pg_ctx *ctx, uint32_t n, const uint8_t *query, const uint64_t *query_off, const int32_t *chr_id,
                         const uint64_t *win_start, const uint32_t *win_len, uint8_t *out)
{
    use_device(ctx);
    if (!ctx || (n && (!query_off || !chr_id || !win_start || !win_len || !out))) return fail(ctx, PG_E_INVALID, "bad containment arguments");
    if (!ctx->d_lo) return fail(ctx, PG_E_NO_REFERENCE, "no reference loaded");
    ctx->last_ms = 0.0;
    if (n == 0) return PG_OK;
    uint64_t max_win = 0, max_query = 0;
    for (uint32_t i = 0; i < n; i++) {
        max_query = std::max<uint64_t>(max_query, query_off[i + 1] - query_off[i]);
        if (query_off[i + 1] < query_off[i]) return fail(ctx, PG_E_INVALID, "query offsets decrease");
        if (query_off[i + 1] - query_off[i] > PG_MAX_READ_LEN) return fail(ctx, PG_E_READ_TOO_LONG, "containment query longer than 499 bases");
        if (chr_id[i] < 0 || chr_id[i] >= (int32_t)ctx->names.size()) return fail(ctx, PG_E_INVALID, "containment window on an unknown chromosome");
        if (win_start[i] > ctx->comp_size[chr_id[i]] || win_len[i] > ctx->comp_size[chr_id[i]] - win_start[i])
            return fail(ctx, PG_E_INVALID, "containment window outside its chromosome");
        max_win = std::max<uint64_t>(max_win, win_len[i]);
    }
    if (query_off[n] && !query) return fail(ctx, PG_E_INVALID, "bad containment arguments");
    // one wave per (item, strand), at most 8192 resident waves (256 CUs x 4 SIMDs x occupancy 8: each systolic step is a chain of
    // lane exchanges, hidden only by other waves); with queries of more than 64 bases each wave keeps one boundary row of its
    // window, capped at 512 MB in all
    const uint64_t n_tasks = 2ull * n;
    const uint64_t stride = max_query > 64 ? (max_win + 63) / 64 * 64 : 0;
    uint64_t waves = std::min<uint64_t>(n_tasks, 8192);
    if (stride) waves = std::min<uint64_t>(waves, std::max<uint64_t>(4, (512ull << 20) / (stride * 4)));
    const uint64_t blocks = (waves + 3) / 4;
    uint8_t *d_q = nullptr, *d_out = nullptr;
    uint64_t *d_qo = nullptr, *d_ws = nullptr;
    int32_t *d_c = nullptr;
    uint32_t *d_wl = nullptr, *d_scr = nullptr;
    auto release = [&]() {
        for (void *p : { (void *)d_q, (void *)d_out, (void *)d_qo, (void *)d_ws, (void *)d_c, (void *)d_wl, (void *)d_scr })
            if (p) (void)hipFree(p);
    };
    int rc = dev_upload(ctx, &d_q, query ? query : (const uint8_t *)"", (size_t)query_off[n]);
    if (!rc) rc = dev_upload(ctx, &d_qo, query_off, (size_t)n + 1);
    if (!rc) rc = dev_upload(ctx, &d_c, chr_id, n);
    if (!rc) rc = dev_upload(ctx, &d_ws, win_start, n);
    if (!rc) rc = dev_upload(ctx, &d_wl, win_len, n);
    if (!rc) rc = dev_alloc(ctx, &d_out, (size_t)n_tasks);
    if (!rc) rc = dev_alloc(ctx, &d_scr, (size_t)(stride ? blocks * 4 * stride : 1));
    if (rc) {
        release();
        return rc;
    }
    const PgDevRef ref = dev_ref(ctx);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t he = hipEventCreate(&e0);
    if (he == hipSuccess) he = hipEventCreate(&e1);
    if (he == hipSuccess) he = hipEventRecord(e0, ctx->stream);
    if (he == hipSuccess && pg_dd_launch(&ref, ctx->d_mm, d_q, d_qo, d_c, d_ws, d_wl, d_out, d_scr, std::max<uint64_t>(stride, 1),
                                         (uint32_t)n_tasks, (uint32_t)blocks, ctx->stream))
        he = hipErrorLaunchFailure;
    if (he == hipSuccess) he = hipEventRecord(e1, ctx->stream);
    if (he == hipSuccess) he = hipEventSynchronize(e1);
    float ms = 0.f;
    if (he == hipSuccess) he = hipEventElapsedTime(&ms, e0, e1);
    std::vector<uint8_t> two((size_t)n_tasks);
    if (he == hipSuccess) he = hipMemcpy(two.data(), d_out, (size_t)n_tasks, hipMemcpyDeviceToHost);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    release();
    if (he != hipSuccess) return fail(ctx, PG_E_DEVICE, std::string("containment kernel: ") + hipGetErrorString(he));
    for (uint32_t i = 0; i < n; i++) out[i] = (uint8_t)(two[2 * (size_t)i] | two[2 * (size_t)i + 1]);
    ctx->last_ms = ms;
    return PG_OK;
}

}  // extern "C"
