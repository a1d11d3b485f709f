// pg_api_priv.h -- what the two host files of the C ABI share (pg_api.cpp: context, reference, batches, search and delivery;
// pg_api_classify.cpp: the device classifier's entries): the context and the device batch, the error and allocation helpers, the
// checks of a caller's pointers and batches, and the scratch holder of one call.  Not installed; include/pindel_pg.h is the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

#include "pg_device.h"
#include "pg_host_plan.h"
#include "pindel_pg.h"

// Grow-only device arena of a ctx: the buffers of a host-path batch (pg_search_batch & co) are carved out of
// it instead of ~25 hipMalloc / hipFree per call.
struct DevArena {
    char *base = nullptr;
    size_t cap = 0, used = 0;
    void *take(size_t bytes)
    {
        const size_t at = pg_arena_align(used);
        if (at + bytes > cap) return nullptr;
        used = at + bytes;
        return base + at;
    }
};

struct pg_ctx {
    pg_params prm{};
    uint32_t mm[512]{};
    uint16_t thr[512]{};
    uint16_t *d_thr = nullptr;
    uint32_t *d_mm = nullptr;
    int32_t *d_sv_budget = nullptr;    // [PG_SV_BUDGET_N] the NT kinds' mismatch budget by length sum (pg_sv.hip), for sv_budget_rate
    double sv_budget_rate = 0.0;
    PgLenRec *d_len_tab = nullptr;     // [512] pg_len_rec of every read length under this context's parameters (the pack's per-length fields)
    hipStream_t stream = nullptr, copy_stream = nullptr;   // kernels / host-to-device input copies
    hipStream_t dl_stream = nullptr;                       // device-to-host result copies of the chunked host path
    hipStream_t stream2 = nullptr;                         // second kernel stream of the chunked host path (odd chunks)
    std::vector<hipEvent_t> events;                        // reused by the chunked host path (no timing)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // hint tables (pg_hints.hip): events around the fill kernel (created on first use), and the last lookup's figures
    // (pg_debug_last_hint_stats): HIP-event ms of count + scan and of the fill, bytes of the table uploaded, windows written
    hipEvent_t evh0 = nullptr, evh1 = nullptr;
    bool hint_fill_timed = false;
    double hint_scan_ms = 0.0, hint_fill_ms = 0.0;
    uint64_t hint_table_bytes = 0, hint_windows = 0;
    // reference
    std::vector<std::string> names;
    std::vector<uint64_t> comp_size;
    std::vector<uint64_t> word_off;   // index of the word holding AbsLoc 0
    // host mirror of the planes: only pg_reference_fetch and pg_reference_save_packed read it.  A host load fills it on its way
    // to the device; after pg_load_reference_device it is empty (mirror_ok false) until one of the two asks (host_mirror)
    mutable std::vector<uint32_t> h_lo, h_hi, h_nn;
    mutable bool mirror_ok = false;
    uint64_t plane_words = 0;          // words of each plane in HBM
    uint32_t *d_lo = nullptr, *d_hi = nullptr, *d_nn = nullptr;
    uint64_t *d_word_off = nullptr;
    uint32_t *d_chr_size = nullptr;
    DevArena arena;                    // device memory of the host-path batches, reused across calls
    // stats of the last search
    double last_ms = 0.0;
    uint64_t last_runs = 0;
    std::string err;
    bool counted = false;              // in g_live_ctx (the pinned-memory cache is trimmed with the last context)
    uint32_t ref_epoch = 0;            // counts reference (re)loads: a device batch's records hold chromosome offsets and sizes
    bool kargs_checked = false;        // the kernels' view of the kernarg segment was checked on this device (pg_debug_kargs_check)
    bool last_in_place = false;        // the last launch asked to pack did so inside the search kernel (pg_debug_last_pack_in_place)
    // the fixed-length kernels (PgFixedLen, pg_device.h): this context's length tables reproduce every baked row (compared once, at
    // pg_create: only then may a launch run one); the LEN of the last search launch's kernel, 0 if it was any other (pg_debug_last_fixed_len)
    bool fixed_ok = false;
    std::atomic<uint32_t> last_fixed_len{0};
    // The launch log (pg_debug_launch_log): every kernel launch on the search path in launch order, the first PG_LAUNCH_LOG_CAP
    // since the last pg_debug_clear_launch_log; launch_n counts them all.  A slot is claimed atomically (launches of one context
    // may come from more than one host thread) and costs a few host stores, no device work.
    static constexpr uint32_t PG_LAUNCH_LOG_CAP = 256;
    PgLaunchRec launch_log[PG_LAUNCH_LOG_CAP]{};
    std::atomic<uint32_t> launch_n{0};
};

void log_launch(pg_ctx *ctx, const PgLaunchRec &r);

// What the device classifier keeps with a batch (always allocations of their own; null: none built).
struct ClassifierState {
    // the event tables of the last pg_device_batch_events
    pg_event_read *ev_reads = nullptr;     // n
    uint32_t *ev_members = nullptr;        // n: the four member lists back to back
    pg_event *ev_events = nullptr;         // n: the four event lists back to back
    pg_event_sizes ev_sizes{};
    bool ev_built = false;
    pg_event_window ev_window{};           // ... and the window they were built for
    // the SV tables of the last pg_device_batch_sv_events; an events build discards them
    uint32_t *svev_members = nullptr;      // n: the three member lists back to back
    pg_event *svev_events = nullptr;       // n: the three event lists back to back
    uint32_t *svev_ws = nullptr;           // n: the order kernel's ranks of boxes beyond its LDS
    pg_sv_event_sizes svev_sizes{};
    bool svev_built = false;
    // the report records of the last pg_device_batch_report_reads; an events or sv events build discards them
    pg_report_read *rr_records = nullptr;      // n: a read is a member of at most one table
    pg_report_summary *rr_summaries = nullptr; // n
    uint64_t rr_n_records = 0;
    bool rr_built = false;
    // the candidate lists of the last pg_device_batch_classify: they never leave the device
    pg_variant_cand *cl_cands = nullptr, *cl_sv_cands = nullptr;   // n x 2 x PG_VARIANT_CANDS; n x PG_SV_SLOTS
    uint8_t *cl_counts = nullptr, *cl_sv_counts = nullptr;         // n x 2; n x PG_SV_KINDS
    // the long-insertion tables of the last pg_device_batch_li; an events build discards them
    uint32_t *li_members = nullptr;            // n: the two member lists back to back
    pg_li_pos *li_positions = nullptr;         // n: the two position tables back to back
    pg_li_sizes li_sizes{};
    bool li_built = false;
    // the interchromosomal junction tables of the last pg_device_batch_int: made from the search result alone, so a
    // new search discards them (drop_search_tables) and no table build does
    uint32_t *int_members = nullptr;           // n
    pg_int_call *int_calls = nullptr;          // n
    pg_int_sizes int_sizes{};
    bool int_built = false;
    // the dispersed-duplication tables of the last pg_device_batch_dd: made from the close end alone and sized by
    // what the build found (each build frees its predecessor's); a new search discards them as well
    pg_dd_member *dd_members = nullptr;        // dd_sizes.members
    pg_dd_cand *dd_cands = nullptr;            // dd_sizes.cands
    uint8_t *dd_cons = nullptr;                // dd_sizes.cons_bytes
    pg_dd_sizes dd_sizes{};
    bool dd_built = false;
    void drop_search_tables() { int_built = dd_built = false; }

    enum Build { EVENTS, SV_EVENTS, REPORT, LI };
    // A build discards its own tables and whatever was made from them: the SV tables belong to the records of the events build they
    // were made from, the long-insertion tables read those records' Used state, and the report records list the members of both
    // table builds.
    void begin_build(Build which)
    {
        if (which == EVENTS) ev_built = svev_built = li_built = false;
        if (which == SV_EVENTS) svev_built = false;
        if (which == LI) li_built = false;
        if (which != LI) rr_built = false;
    }
    void release()
    {
        for (void *p : { (void *)ev_reads, (void *)ev_members, (void *)ev_events, (void *)svev_members, (void *)svev_events, (void *)svev_ws,
                         (void *)rr_records, (void *)rr_summaries, (void *)cl_cands, (void *)cl_sv_cands, (void *)cl_counts, (void *)cl_sv_counts,
                         (void *)li_members, (void *)li_positions, (void *)int_members, (void *)int_calls, (void *)dd_members, (void *)dd_cands,
                         (void *)dd_cons })
            if (p) (void)hipFree(p);
        *this = ClassifierState();
    }
};

struct pg_device_batch {
    uint32_t n = 0;
    uint32_t max_len = 0, levels = 0;
    uint32_t uniform_len = 0;          // the length of every read of the batch when they all have one (0: mixed lengths, no reads)
    int32_t max_isz = 0;
    int64_t max_bd_window = 0;         // largest BreakDancer window attached (positions)
    uint64_t max_bd_cluster = 0;       // most windows attached to one read
    uint8_t *seq = nullptr;
    uint64_t *seq_off = nullptr;
    uint8_t *strand = nullptr;
    int32_t *pos = nullptr;
    int16_t *isz = nullptr;
    int32_t *chr = nullptr;
    uint8_t *rc_flag = nullptr;
    uint32_t *close_last = nullptr;
    uint16_t *close_max = nullptr;
    uint64_t *bd_off = nullptr;
    pg_window *bd = nullptr;
    PgInRec *in_rec = nullptr;         // packed per-read records the kernel reads / writes (pg_device.h)
    uint32_t ref_epoch = 0;            // pg_ctx::ref_epoch when the records were packed (a reload of the reference: pack again)
    uint64_t *planes = nullptr;        // the reads as bit planes (PgDevBatch::planes)
    PgOutRec *out_rec = nullptr;
    bool in_arena = false;             // buffers belong to the ctx arena (not freed one by one)
    bool pool_owned = false;           // ... except a run pool that had to be regrown
    pg_run *pool = nullptr;
    uint32_t pool_shard_cap = 0;       // runs per shard (PG_POOL_SHARDS shards)
    uint32_t *pool_used = nullptr;     // [PG_POOL_SHARDS * 16]
    unsigned long long *run_tot = nullptr;   // running totals of the chunked delivery (zeroed with the outputs)
    // reads with a character outside ACGTN, listed by the pack kernel for the exact kernel (pg_search_exact_kernel)
    uint32_t *exact_list = nullptr;    // [n]
    uint32_t *exact_count = nullptr;   // device counter (zeroed with the outputs / before a pack of the whole batch)
    PgSoaIn *d_soa = nullptr;          // the pack's view of the inputs, in device memory, for launches that pack in place (PgDevBatch::soa)
    PgSoaIn h_soa;                     // ... and what was copied there last (the source of an asynchronous copy)
    bool soa_uploaded = false;
    long long exact_n = -1;            // host copy of the counter; -1: not read back (the exact kernel is launched regardless)
    bool searched = false;             // close end + far end have run on the batch: its output records and run pool hold a result
    bool close_searched = false;       // the close end has run on the batch (alone, or as part of a search): the close fields of its records hold a result
    ClassifierState cls;               // the device classifier's tables and lists (null / false: none built)
};

// One ctx drives one device; a process may hold several (one host thread each): every entry point selects
// its ctx's device for the calling thread first.
inline void use_device(const pg_ctx *ctx)
{
    if (ctx) (void)hipSetDevice(ctx->prm.device);
}

inline int fail(pg_ctx *ctx, int code, const std::string &msg)
{
    if (ctx) ctx->err = msg;
    return code;
}

// (the device-buffer entries: a caller's pointer, checked before anything is launched -- defined with them, in pg_api.cpp)
int check_device_ptr(pg_ctx *ctx, const void *p, size_t bytes, size_t align, const char *what);

#define HIP_TRY(ctx, call)                                                                  \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(ctx, e_ == hipErrorOutOfMemory ? PG_E_NOMEM : PG_E_DEVICE,           \
                        std::string(#call) + ": " + hipGetErrorString(e_));                  \
    } while (0)

template <typename T>
int dev_alloc(pg_ctx *ctx, T **p, size_t n)
{
    *p = nullptr;
    HIP_TRY(ctx, hipMalloc((void **)p, std::max<size_t>(n, 1) * sizeof(T)));
    return PG_OK;
}

template <typename T>
int dev_upload(pg_ctx *ctx, T **p, const T *src, size_t n)
{
    int rc = dev_alloc(ctx, p, n);
    if (rc) return rc;
    if (n) HIP_TRY(ctx, hipMemcpy(*p, src, n * sizeof(T), hipMemcpyHostToDevice));
    return PG_OK;
}

inline PgDevRef dev_ref(const pg_ctx *ctx)
{
    PgDevRef r;
    r.lo = ctx->d_lo;
    r.hi = ctx->d_hi;
    r.nn = ctx->d_nn;
    r.chr_word_off = ctx->d_word_off;
    r.chr_size = ctx->d_chr_size;
    r.n_chr = (int32_t)ctx->names.size();
    return r;
}

// A device batch whose reference has been replaced since it was validated: its chromosome ids, anchor windows and (once packed)
// word offsets belong to the old reference.
inline int stale_batch(pg_ctx *ctx, const pg_device_batch *b)
{
    if (b->ref_epoch != ctx->ref_epoch && b->n)
        return fail(ctx, PG_E_INVALID, "the reference was (re)loaded after this batch was uploaded: upload the batch again");
    return PG_OK;
}

// Device temporaries of one call: from the ctx arena where the batch lives there and the arena has room, hipMalloc'd otherwise;
// all given back when the call ends.  (Only the host path's own batches live in the arena, and they die with their call: a batch
// that reaches the classifier's entries never does, so a table build, which synchronises in mid-build, holds no arena mark.)
struct DevTemps {
    pg_ctx *ctx;
    const bool in_arena;
    const size_t arena_mark;
    std::vector<void *> owned;                            // hipMalloc'd (none while the arena has room)
    DevTemps(pg_ctx *c, const pg_device_batch *b) : ctx(c), in_arena(b->in_arena), arena_mark(c->arena.used) {}
    DevTemps(const DevTemps &) = delete;
    ~DevTemps()
    {
        for (void *p : owned) (void)hipFree(p);
        if (in_arena) ctx->arena.used = arena_mark;
    }
    void *take(size_t bytes)
    {
        void *p = in_arena ? ctx->arena.take(bytes) : nullptr;
        if (p) return p;
        if (hipMalloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess) return nullptr;
        owned.push_back(p);
        return p;
    }
    // n elements into *p (as dev_alloc: at least one, and its refusal)
    template <typename T>
    int take(T **p, size_t n)
    {
        n = std::max<size_t>(n, 1);
        if (in_arena && (*p = (T *)ctx->arena.take(n * sizeof(T)))) return PG_OK;
        if (int rc = dev_alloc(ctx, p, n)) return rc;
        owned.push_back(*p);
        return PG_OK;
    }
};
