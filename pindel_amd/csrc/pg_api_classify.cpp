// pg_api_classify.cpp -- the device classifier's entries of the C ABI (include/pindel_pg.h): candidates per
// read, event tables, SV event tables, report records, long-insertion tables, junction tables, dispersed-duplication tables, and the
// one call per window that chains the first five.
// Every entry checks its arguments and owns its buffers here; the kernels and their launchers are pg_variant.hip, pg_sv.hip,
// pg_events.hip, pg_sv_events.hip, pg_report.hip, pg_li.hip, pg_int.hip and pg_dd_tables.hip.  What this file shares with pg_api.cpp is pg_api_priv.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "pg_api_priv.h"
#include "pg_device.h"
#include "pindel_pg.h"

namespace {

// ---- the steps every entry shares
// One timed span on the ctx stream: HIP events around what `body` queues, then the wait; last_ms = the span
template <class F>
int timed(pg_ctx *ctx, F body)
{
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    if (int rc = body()) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    ctx->last_ms = ms;
    return PG_OK;
}

void log_kernel(pg_ctx *ctx, int32_t kernel, int32_t blocks)
{
    PgLaunchRec rec{};
    rec.kernel = kernel;
    rec.blocks = blocks;
    log_launch(ctx, rec);
}

// The refusals an entry opens with, in two halves: what an entry checks of its own arguments in between (the candidate kernels:
// the empty batch returns; events: its window) stays between them.
int not_searched(pg_ctx *ctx, const pg_device_batch *b)
{
    if (b->n && !b->searched) return fail(ctx, PG_E_INVALID, "the batch has not been searched: no close and far ends to classify");
    return PG_OK;
}
int entry_refusal(pg_ctx *ctx, const pg_device_batch *b, bool searched_too)
{
    if (ctx->names.empty()) return fail(ctx, PG_E_NO_REFERENCE, "no reference loaded");
    if (int rc = stale_batch(ctx, b)) return rc;
    ctx->last_ms = 0.0;
    return searched_too ? not_searched(ctx, b) : PG_OK;
}

// The five per-read arrays the entries hand around: elements per read, element size, alignment and the field's name in a label
enum { CA_CANDS, CA_COUNTS, CA_SV_CANDS, CA_SV_COUNTS, CA_NAME_ID, CA_N };
struct CandArrayDesc {
    size_t per_read, elem, align;
    const char *field;
};
const CandArrayDesc CAND_ARRAYS[CA_N] = {
    { 2 * PG_VARIANT_CANDS, sizeof(pg_variant_cand), 4, "cands" }, { 2, 1, 1, "counts" },
    { PG_SV_SLOTS, sizeof(pg_variant_cand), 4, "sv_cands" },       { PG_SV_KINDS, 1, 1, "sv_counts" },
    { 1, sizeof(uint32_t), 4, "name_id" },
};
size_t cand_elems(int which, size_t n) { return n * CAND_ARRAYS[which].per_read; }
size_t cand_bytes(int which, size_t n) { return cand_elems(which, n) * CAND_ARRAYS[which].elem; }

struct CandSet {                                              // a set of them (null: not in the set), host or device pointers
    const void *p[CA_N] = { nullptr, nullptr, nullptr, nullptr, nullptr };
    CandSet() {}
    CandSet(const pg_variant_cand *cands, const uint8_t *counts, const pg_variant_cand *sv_cands, const uint8_t *sv_counts,
            const uint32_t *name_id = nullptr)
        : p{ cands, counts, sv_cands, sv_counts, name_id } {}
    const pg_variant_cand *cands() const { return (const pg_variant_cand *)p[CA_CANDS]; }
    const uint8_t *counts() const { return (const uint8_t *)p[CA_COUNTS]; }
    const pg_variant_cand *sv_cands() const { return (const pg_variant_cand *)p[CA_SV_CANDS]; }
    const uint8_t *sv_counts() const { return (const uint8_t *)p[CA_SV_COUNTS]; }
    const uint32_t *name_id() const { return (const uint32_t *)p[CA_NAME_ID]; }
    bool pair_mismatch() const { return (!p[CA_CANDS]) != (!p[CA_COUNTS]) || (!p[CA_SV_CANDS]) != (!p[CA_SV_COUNTS]); }
};

// The arrays `mask` names (bits 1 << CA_*) are device memory of this context's GPU with room for n reads; the labels are
// "<entry>: <field>".  optional: a null array is left out instead of refused.  fields: an entry's own names, where they differ.
int check_cand_set(pg_ctx *ctx, size_t n, const char *entry, const CandSet &s, unsigned mask, bool optional = false,
                   const char *const *fields = nullptr)
{
    for (int k = 0; k < CA_N; k++) {
        if (!(mask >> k & 1u) || (optional && !s.p[k])) continue;
        const std::string label = std::string(entry) + ": " + (fields && fields[k] ? fields[k] : CAND_ARRAYS[k].field);
        if (int rc = check_device_ptr(ctx, s.p[k], cand_bytes(k, n), CAND_ARRAYS[k].align, label.c_str())) return rc;
    }
    return PG_OK;
}
const unsigned CA_PAIRS = 1u << CA_CANDS | 1u << CA_COUNTS, CA_SV_PAIRS = 1u << CA_SV_CANDS | 1u << CA_SV_COUNTS;

// The host arrays of `host` that `mask` names, copied into scratch of `tmp`: the set of their device twins (no reads, or a null
// array: null)
int stage_cand_set(pg_ctx *ctx, DevTemps &tmp, size_t n, const CandSet &host, unsigned mask, CandSet *dev)
{
    for (int k = 0; k < CA_N; k++) {
        if (!n || !(mask >> k & 1u) || !host.p[k]) continue;
        uint8_t *d = nullptr;
        if (int rc = tmp.take(&d, cand_bytes(k, n))) return rc;
        HIP_TRY(ctx, hipMemcpy(d, host.p[k], cand_bytes(k, n), hipMemcpyHostToDevice));
        dev->p[k] = d;
    }
    return PG_OK;
}

// Tables that leave the batch: each one with a destination is copied, count elements from the batch's src.  to_device: the
// destinations are the caller's device pointers, all checked before the first copy.
struct TableCopy {
    void *dst;
    const void *src;
    size_t count, elem, align;
    const char *label;
};
int copy_tables(pg_ctx *ctx, std::initializer_list<TableCopy> tables, bool to_device)
{
    if (to_device)
        for (const TableCopy &t : tables)
            if (t.dst)
                if (int rc = check_device_ptr(ctx, t.dst, t.count * t.elem, t.align, t.label)) return rc;
    for (const TableCopy &t : tables)
        if (t.dst && t.count) HIP_TRY(ctx, hipMemcpy(t.dst, t.src, t.count * t.elem, to_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    return PG_OK;
}

// Several temporaries of one call as ONE allocation of `tmp`: add() notes an array of n elements (at least one), take() allocates and
// hands every array its place, each at a 256-byte boundary of the block
struct TempBlock {
    struct Part {
        void **p;
        size_t at;
    };
    std::vector<Part> parts;
    size_t bytes = 0;
    template <typename T>
    void add(T **p, size_t n)
    {
        parts.push_back({ (void **)p, bytes });
        bytes += (std::max<size_t>(n, 1) * sizeof(T) + 255) & ~(size_t)255;
    }
    int take(pg_ctx *ctx, DevTemps &tmp)
    {
        char *base = (char *)tmp.take(bytes);
        if (!base) return fail(ctx, PG_E_NOMEM, "device memory for a table build's temporaries");
        for (const Part &x : parts) *x.p = base + x.at;
        return PG_OK;
    }
};

unsigned long long pool_runs(const pg_device_batch *b) { return (unsigned long long)b->pool_shard_cap * PG_POOL_SHARDS; }

// ---- the device classifier (pg_variant.hip): deletion and short-insertion candidates of a searched batch
// d_cands / d_counts: device memory (checked by the caller where it is the user's).  The launch is recorded in the launch log and
// timed with HIP events like a search's.
int variant_candidates(pg_ctx *ctx, pg_device_batch *b, pg_variant_cand *d_cands, uint8_t *d_counts)
{
    if (int rc = entry_refusal(ctx, b, false)) return rc;
    if (!b->n) return PG_OK;                                  // nothing is launched for an empty batch
    if (int rc = not_searched(ctx, b)) return rc;
    const PgDevRef ref = dev_ref(ctx);
    return timed(ctx, [&]() -> int {
        if (pg_variant_launch(&ref, b->out_rec, b->pool, pool_runs(b), b->seq, b->seq_off, b->strand, b->chr, ctx->d_mm, ctx->prm.spacer, b->n, d_cands,
                              d_counts, ctx->stream))
            return fail(ctx, PG_E_DEVICE, "launching the variant-candidate kernel failed");
        log_kernel(ctx, PG_KERNEL_VARIANT, 4);                // reads (waves) per workgroup
        return PG_OK;
    });
}

// ---- ... of the five other kinds (pg_sv.hip): DI, tandem-duplication and inversion candidates
// (short)(1 + Seq_Error_Rate * length sum) for every length sum, as the host classifiers compute it: the product is stored before
// the add, so that no compiler fuses the two
int sv_budget_table(pg_ctx *ctx, double rate)
{
    if (ctx->d_sv_budget && std::memcmp(&ctx->sv_budget_rate, &rate, sizeof rate) == 0) return PG_OK;
    std::vector<int32_t> t(PG_SV_BUDGET_N);
    for (int len = 0; len < PG_SV_BUDGET_N; len++) {
        volatile double prod = rate * len;
        const double v = 1 + prod;
        t[(size_t)len] = v >= -32768.0 && v < 32768.0 ? (int32_t)(short)v : 32767;      // (NaN or out of a short's range: undefined on the host)
    }
    if (ctx->d_sv_budget) {
        HIP_TRY(ctx, hipMemcpy(ctx->d_sv_budget, t.data(), t.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    } else if (int rc = dev_upload(ctx, &ctx->d_sv_budget, t.data(), t.size())) {
        return rc;
    }
    ctx->sv_budget_rate = rate;
    return PG_OK;
}

int sv_params_ok(pg_ctx *ctx, const pg_sv_params *p)
{
    if (!p) return fail(ctx, PG_E_INVALID, "sv candidates: null pg_sv_params");
    if (p->min_inversion_size < 0 || p->min_inversion_size > PG_SV_MAX_INVERSION_SIZE)
        return fail(ctx, PG_E_INVALID, "sv candidates: the minimum inversion size (-v) must lie in [0, 2^30]");
    return PG_OK;
}

int sv_candidates(pg_ctx *ctx, pg_device_batch *b, const pg_sv_params *p, pg_variant_cand *d_cands, uint8_t *d_counts)
{
    if (int rc = entry_refusal(ctx, b, false)) return rc;
    if (int rc = sv_params_ok(ctx, p)) return rc;
    if (!b->n) return PG_OK;                                  // nothing is launched for an empty batch
    if (int rc = not_searched(ctx, b)) return rc;
    if (int rc = sv_budget_table(ctx, p->seq_error_rate)) return rc;
    const PgDevRef ref = dev_ref(ctx);
    return timed(ctx, [&]() -> int {
        if (pg_sv_launch(&ref, b->out_rec, b->pool, pool_runs(b), b->seq, b->seq_off, b->strand, b->chr, ctx->d_mm, ctx->d_sv_budget,
                         p->min_num_matched_bases, (uint32_t)p->min_inversion_size, ctx->prm.spacer, b->n, d_cands, d_counts, ctx->stream))
            return fail(ctx, PG_E_DEVICE, "launching the sv-candidate kernel failed");
        log_kernel(ctx, PG_KERNEL_SV, 4);                     // reads (waves) per workgroup
        return PG_OK;
    });
}

// The host-pointer twin of a candidate entry: the lists of `run` in scratch, then to the caller's arrays.  which: CA_CANDS or
// CA_SV_CANDS, the count bytes follow it; what: the entry's name in the out-of-memory refusal
template <class F>
int candidates_to_host(pg_ctx *ctx, pg_device_batch *b, int which, const char *what, pg_variant_cand *cands, uint8_t *counts, F run)
{
    const size_t n = b->n;
    DevTemps tmp(ctx, b);
    pg_variant_cand *d_cands = (pg_variant_cand *)tmp.take(cand_bytes(which, n));
    uint8_t *d_counts = (uint8_t *)tmp.take(cand_bytes(which + 1, n));
    if (!d_cands || !d_counts) return fail(ctx, PG_E_NOMEM, std::string("device memory for the ") + what);
    if (int rc = run(d_cands, d_counts)) return rc;
    HIP_TRY(ctx, hipMemcpy(cands, d_cands, cand_bytes(which, n), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(counts, d_counts, cand_bytes(which + 1, n), hipMemcpyDeviceToHost));
    return PG_OK;
}

}  // namespace

int pg_device_batch_variant_candidates_device(pg_ctx *ctx, pg_device_batch *b, pg_variant_cand *d_cands, uint8_t *d_counts)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    if (int rc = check_cand_set(ctx, b->n, "variant candidates", CandSet(d_cands, d_counts, nullptr, nullptr), CA_PAIRS)) return rc;
    return variant_candidates(ctx, b, d_cands, d_counts);
}

int pg_device_batch_variant_candidates(pg_ctx *ctx, pg_device_batch *b, pg_variant_cand *cands, uint8_t *counts)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    if (b->n && (!cands || !counts)) return fail(ctx, PG_E_INVALID, "variant candidates: null output array");
    if (!b->n || !b->searched) return variant_candidates(ctx, b, nullptr, nullptr);      // (nothing to do, or the refusal)
    return candidates_to_host(ctx, b, CA_CANDS, "variant candidates", cands, counts,
                              [&](pg_variant_cand *d_cands, uint8_t *d_counts) { return variant_candidates(ctx, b, d_cands, d_counts); });
}

int pg_device_batch_sv_candidates_device(pg_ctx *ctx, pg_device_batch *b, const pg_sv_params *p, pg_variant_cand *d_cands, uint8_t *d_counts)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    static const char *const own_fields[CA_N] = { nullptr, nullptr, "cands", "counts", nullptr };      // (this entry has one pair: no sv_ prefix)
    if (int rc = check_cand_set(ctx, b->n, "sv candidates", CandSet(nullptr, nullptr, d_cands, d_counts), CA_SV_PAIRS, false, own_fields)) return rc;
    return sv_candidates(ctx, b, p, d_cands, d_counts);
}

int pg_device_batch_sv_candidates(pg_ctx *ctx, pg_device_batch *b, const pg_sv_params *p, pg_variant_cand *cands, uint8_t *counts)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    if (b->n && (!cands || !counts)) return fail(ctx, PG_E_INVALID, "sv candidates: null output array");
    if (!b->n || !b->searched || sv_params_ok(ctx, p)) return sv_candidates(ctx, b, p, nullptr, nullptr);      // (nothing to do, or the refusal)
    return candidates_to_host(ctx, b, CA_SV_CANDS, "sv candidates", cands, counts,
                              [&](pg_variant_cand *d_cands, uint8_t *d_counts) { return sv_candidates(ctx, b, p, d_cands, d_counts); });
}

// ---- ... its third part (pg_events.hip): window tail, boxes and event tables
namespace {
// the refusals of both build entries, before anything is launched or copied
int events_refusal(pg_ctx *ctx, pg_device_batch *b, const pg_event_window *w, bool lists_null_mismatch)
{
    if (int rc = entry_refusal(ctx, b, false)) return rc;
    if (!w) return fail(ctx, PG_E_INVALID, "events: null pg_event_window");
    if (lists_null_mismatch) return fail(ctx, PG_E_INVALID, "events: candidate arrays come in pairs (records and count bytes)");
    if (w->chr_id < 0 || w->chr_id >= (int32_t)ctx->names.size()) return fail(ctx, PG_E_INVALID, "events: the window's chr_id lies outside the reference");
    if (w->region_start > w->region_end) return fail(ctx, PG_E_INVALID, "events: region_start > region_end");
    return not_searched(ctx, b);
}

// BoxSize from the padded chromosome length, as Caller::process_window computes it (pindel.cpp:1806-1810; NumBoxes: build_events)
uint32_t box_size_of(const pg_ctx *ctx, int32_t chr_id)
{
    const uint32_t box_size = (uint32_t)(ctx->comp_size[(size_t)chr_id] / 30000);
    return box_size ? box_size : 1;
}

// every list of d is device memory (or null)
int build_events(pg_ctx *ctx, pg_device_batch *b, const pg_event_window *w, const CandSet &d)
{
    ClassifierState &c = b->cls;
    c.begin_build(ClassifierState::EVENTS);
    c.ev_sizes = pg_event_sizes{};
    c.ev_window = *w;
    const size_t n = b->n;
    if (!n) {                                                 // nothing is launched for an empty batch
        c.ev_built = true;
        return PG_OK;
    }
    int rc;
    if (!c.ev_reads && ((rc = dev_alloc(ctx, &c.ev_reads, n)) || (rc = dev_alloc(ctx, &c.ev_members, n)) || (rc = dev_alloc(ctx, &c.ev_events, n))))
        return rc;
    DevTemps tmp(ctx, b);
    PgEventArgs a{};
    const size_t n_blk = n / PG_EV_BLOCK + 2;
    if ((rc = tmp.take(&a.rec_a, n)) || (rc = tmp.take(&a.rec_b, n)) || (rc = tmp.take(&a.flag, n)) || (rc = tmp.take(&a.rank, n)) ||
        (rc = tmp.take(&a.blk, n_blk)) || (rc = tmp.take(&a.midx, n)) || (rc = tmp.take(&a.efirst, n + 1)) ||
        (rc = tmp.take(&a.digit_cnt, 256 * n_blk + 1)) || (rc = tmp.take(&a.info, 1)))
        return rc;
    a.out = b->out_rec;
    a.pool = b->pool;
    a.pool_runs = pool_runs(b);
    a.seq = b->seq;
    a.seq_off = b->seq_off;
    a.strand = b->strand;
    a.chr = b->chr;
    a.isz = b->isz;
    a.spacer = ctx->prm.spacer;
    a.n = b->n;
    a.win = *w;
    a.box_size = box_size_of(ctx, w->chr_id);
    a.n_boxes = (uint32_t)(ctx->comp_size[(size_t)w->chr_id] * 2 / a.box_size) + 1;
    a.cands = d.cands();
    a.counts = d.counts();
    a.sv_cands = d.sv_cands();
    a.sv_counts = d.sv_counts();
    a.name_id = d.name_id();
    a.reads = c.ev_reads;
    a.members = c.ev_members;
    a.events = c.ev_events;
    const PgDevRef ref = dev_ref(ctx);
    PgEventInfo info;
    rc = timed(ctx, [&]() -> int {
        if (pg_events_cascade_launch(&a, ctx->stream)) return fail(ctx, PG_E_DEVICE, "launching the event cascade kernels failed");
        log_kernel(ctx, PG_KERNEL_EVENT_CASCADE, (int32_t)PG_EV_BLOCK);
        HIP_TRY(ctx, hipMemcpyAsync(&info, a.info, sizeof info, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (info.n_boxed > n) return fail(ctx, PG_E_DEVICE, "events: the boxed count exceeds the batch");
        if (!info.n_boxed) return PG_OK;                      // (nothing boxed: nothing below indexes an empty array)
        PgEventRec *src = a.rec_b, *dst = a.rec_a;
        for (int pass = 0; pass < PG_EV_SORT_PASSES; pass++) {
            const int word = pass >= 16 ? 4 : 3 - (pass >> 2), shift = pass >= 16 ? 0 : (pass & 3) * 8;
            if ((((info.key_or[word] ^ info.key_and[word]) >> shift) & 0xffu) == 0u) continue;      // the byte is constant: no pass
            if (pg_events_sort_pass_launch(&a, src, dst, info.n_boxed, pass, ctx->stream)) return fail(ctx, PG_E_DEVICE, "launching an event sort pass failed");
            log_kernel(ctx, PG_KERNEL_EVENT_SORT, pass);
            std::swap(src, dst);
        }
        if (pg_events_tables_launch(&ref, &a, src, info.n_boxed, ctx->stream)) return fail(ctx, PG_E_DEVICE, "launching the event table kernels failed");
        log_kernel(ctx, PG_KERNEL_EVENT_TABLES, (int32_t)PG_EV_BLOCK);
        HIP_TRY(ctx, hipMemcpyAsync(&info, a.info, sizeof info, hipMemcpyDeviceToHost, ctx->stream));
        return PG_OK;
    });
    if (rc) return rc;
    if (info.n_boxed) {
        if (info.n_members > info.n_boxed || info.n_events > info.n_members) return fail(ctx, PG_E_DEVICE, "events: inconsistent table sizes");
        for (int t = 0; t < PG_EVENT_TABLES; t++) {
            c.ev_sizes.members[t] = info.member_start[t + 1] - info.member_start[t];
            c.ev_sizes.events[t] = info.event_start[t + 1] - info.event_start[t];
        }
    }
    c.ev_sizes.unresolved = info.n_unresolved;
    c.ev_built = true;
    return PG_OK;
}
const unsigned CA_EVENTS = CA_PAIRS | CA_SV_PAIRS | 1u << CA_NAME_ID;
}  // namespace

int pg_device_batch_events_device(pg_ctx *ctx, pg_device_batch *b, const pg_event_window *window, const pg_variant_cand *d_cands,
                                  const uint8_t *d_counts, const pg_variant_cand *d_sv_cands, const uint8_t *d_sv_counts, const uint32_t *d_name_id)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    const CandSet dev(d_cands, d_counts, d_sv_cands, d_sv_counts, d_name_id);
    if (int rc = events_refusal(ctx, b, window, dev.pair_mismatch())) return rc;
    if (int rc = check_cand_set(ctx, b->n, "events", dev, CA_EVENTS, true)) return rc;
    return build_events(ctx, b, window, dev);
}

int pg_device_batch_events(pg_ctx *ctx, pg_device_batch *b, const pg_event_window *window, const pg_variant_cand *cands, const uint8_t *counts,
                           const pg_variant_cand *sv_cands, const uint8_t *sv_counts, const uint32_t *name_id)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    const CandSet host(cands, counts, sv_cands, sv_counts, name_id);
    if (int rc = events_refusal(ctx, b, window, host.pair_mismatch())) return rc;
    DevTemps tmp(ctx, b);
    CandSet dev;
    if (int rc = stage_cand_set(ctx, tmp, b->n, host, CA_EVENTS, &dev)) return rc;
    return build_events(ctx, b, window, dev);
}

int pg_device_batch_event_sizes(pg_ctx *ctx, pg_device_batch *b, pg_event_sizes *sizes)
{
    use_device(ctx);
    if (!ctx || !b || !sizes) return PG_E_INVALID;
    if (!b->cls.ev_built) return fail(ctx, PG_E_INVALID, "no event tables: pg_device_batch_events has not been run on this batch");
    *sizes = b->cls.ev_sizes;
    return PG_OK;
}

static int events_download(pg_ctx *ctx, pg_device_batch *b, pg_event_read *reads, uint32_t *members, pg_event *events, bool to_device)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    const ClassifierState &c = b->cls;
    if (!c.ev_built) return fail(ctx, PG_E_INVALID, "no event tables: pg_device_batch_events has not been run on this batch");
    size_t nm = 0, ne = 0;
    for (int t = 0; t < PG_EVENT_TABLES; t++) {
        nm += c.ev_sizes.members[t];
        ne += c.ev_sizes.events[t];
    }
    return copy_tables(ctx,
                       { { reads, c.ev_reads, b->n, sizeof(pg_event_read), 2, "events download: reads" },
                         { members, c.ev_members, nm, sizeof(uint32_t), 4, "events download: members" },
                         { events, c.ev_events, ne, sizeof(pg_event), 4, "events download: events" } },
                       to_device);
}

int pg_device_batch_events_download(pg_ctx *ctx, pg_device_batch *b, pg_event_read *reads, uint32_t *members, pg_event *events)
{
    return events_download(ctx, b, reads, members, events, false);
}

int pg_device_batch_events_download_device(pg_ctx *ctx, pg_device_batch *b, pg_event_read *d_reads, uint32_t *d_members, pg_event *d_events)
{
    return events_download(ctx, b, d_reads, d_members, d_events, true);
}

// ---- ... its fourth part (pg_sv_events.hip): the event tables of DI, INV and INV_NT
namespace {
int sv_events_refusal(pg_ctx *ctx, pg_device_batch *b, const void *sv_cands, const void *sv_counts)
{
    if (int rc = entry_refusal(ctx, b, true)) return rc;
    if (!b->cls.ev_built) return fail(ctx, PG_E_INVALID, "sv events: pg_device_batch_events has not been run on this batch");
    if (b->n && (!sv_cands || !sv_counts)) return fail(ctx, PG_E_INVALID, "sv events: null sv candidate arrays");
    if (b->n >= 0x80000000u) return fail(ctx, PG_E_INVALID, "sv events: 2^31 reads or more (bit 31 of a member word is PG_SVEV_MEMBER_DUP)");
    return PG_OK;
}

// d_sv_cands is device memory
int build_sv_events(pg_ctx *ctx, pg_device_batch *b, const pg_variant_cand *d_sv_cands)
{
    ClassifierState &c = b->cls;
    c.begin_build(ClassifierState::SV_EVENTS);
    c.svev_sizes = pg_sv_event_sizes{};
    const size_t n = b->n;
    if (!n) {                                                 // nothing is launched for an empty batch
        c.svev_built = true;
        return PG_OK;
    }
    int rc;
    if (!c.svev_members && ((rc = dev_alloc(ctx, &c.svev_members, n)) || (rc = dev_alloc(ctx, &c.svev_events, n)) || (rc = dev_alloc(ctx, &c.svev_ws, n))))
        return rc;
    DevTemps tmp(ctx, b);
    PgSvEventArgs a{};
    const size_t n_blk = n / PG_EV_BLOCK + 2;
    if ((rc = tmp.take(&a.rec_a, n)) || (rc = tmp.take(&a.rec, n)) || (rc = tmp.take(&a.flag, n)) || (rc = tmp.take(&a.dupf, n)) ||
        (rc = tmp.take(&a.rank, n)) || (rc = tmp.take(&a.blk, n_blk)) || (rc = tmp.take(&a.perm_a, n)) || (rc = tmp.take(&a.perm_b, n)) ||
        (rc = tmp.take(&a.kperm_a, n)) || (rc = tmp.take(&a.kperm_b, n)) || (rc = tmp.take(&a.krank, n)) || (rc = tmp.take(&a.seg_first, n + 1)) ||
        (rc = tmp.take(&a.midx, n)) || (rc = tmp.take(&a.rfirst, n + 1)) || (rc = tmp.take(&a.rmx, n)) || (rc = tmp.take(&a.rfail, n)) ||
        (rc = tmp.take(&a.digit_cnt, 256 * n_blk + 1)) || (rc = tmp.take(&a.info, 1)))
        return rc;
    a.out = b->out_rec;
    a.seq = b->seq;
    a.seq_off = b->seq_off;
    a.strand = b->strand;
    a.spacer = ctx->prm.spacer;
    a.n = b->n;
    a.win = c.ev_window;
    a.box_size = box_size_of(ctx, a.win.chr_id);
    a.sv_cands = d_sv_cands;
    a.reads = c.ev_reads;
    a.members = c.svev_members;
    a.events = c.svev_events;
    a.ws_rank = c.svev_ws;
    const PgDevRef ref = dev_ref(ctx);
    PgSvEventInfo info;
    rc = timed(ctx, [&]() -> int {
        if (pg_sv_events_gather_launch(&a, ctx->stream)) return fail(ctx, PG_E_DEVICE, "launching the sv event gather kernels failed");
        log_kernel(ctx, PG_KERNEL_SV_EVENTS, (int32_t)PG_EV_BLOCK);
        HIP_TRY(ctx, hipMemcpyAsync(&info, a.info, sizeof info, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (info.n_boxed > n) return fail(ctx, PG_E_DEVICE, "sv events: the boxed count exceeds the batch");
        if (!info.n_boxed) return PG_OK;                      // (nothing boxed: nothing below indexes an empty array)
        // a pass over a byte that is constant over the boxed records changes nothing: skipped
        auto sort = [&](uint32_t *&src, uint32_t *&dst, int pass, uint32_t vary) -> int {
            if (!vary) return 0;
            if (pg_sv_events_sort_pass_launch(&a, src, dst, info.n_boxed, pass, ctx->stream)) return -1;
            std::swap(src, dst);
            return 0;
        };
        uint32_t *perm = a.perm_a, *perm_t = a.perm_b, *kperm = a.kperm_a, *kperm_t = a.kperm_b;
        const uint32_t seg_vary = info.seg_or ^ info.seg_and;
        for (int k = 0; k < 4; k++)
            if (sort(perm, perm_t, PG_SVEV_PASS_BOX + k, (seg_vary >> (8 * k)) & 0xffu)) return fail(ctx, PG_E_DEVICE, "launching an sv event sort pass failed");
        for (int pass = 0; pass < PG_SVEV_PASS_TABLE; pass++) {
            const int word = PG_SVEV_KEY_WORDS - 1 - (pass >> 2);
            if (sort(kperm, kperm_t, pass, ((info.key_or[word] ^ info.key_and[word]) >> ((pass & 3) * 8)) & 0xffu))
                return fail(ctx, PG_E_DEVICE, "launching an sv event sort pass failed");
        }
        if (sort(kperm, kperm_t, PG_SVEV_PASS_TABLE, seg_vary >> 24)) return fail(ctx, PG_E_DEVICE, "launching an sv event sort pass failed");
        if (pg_sv_events_tables_launch(&ref, &a, perm, kperm, info.n_boxed, ctx->stream)) return fail(ctx, PG_E_DEVICE, "launching the sv event table kernels failed");
        HIP_TRY(ctx, hipMemcpyAsync(&info, a.info, sizeof info, hipMemcpyDeviceToHost, ctx->stream));
        return PG_OK;
    });
    if (rc) return rc;
    if (info.n_boxed) {
        uint64_t nm = 0, ne = 0;
        for (int t = 0; t < PG_SV_EVENT_TABLES; t++) {
            c.svev_sizes.members[t] = info.n_mem[t];
            c.svev_sizes.events[t] = info.n_ev[t];
            c.svev_sizes.dropped_runs[t] = info.dropped[t];
            nm += info.n_mem[t];
            ne += info.n_ev[t];
        }
        if (nm != info.n_members || nm > info.n_boxed || ne > info.n_runs || info.n_runs > nm) {
            c.svev_sizes = pg_sv_event_sizes{};
            return fail(ctx, PG_E_DEVICE, "sv events: inconsistent table sizes");
        }
    }
    c.svev_built = true;
    return PG_OK;
}
const char *const NO_SV_TABLES = "no sv event tables: pg_device_batch_sv_events has not been run on this batch since its events build";
}  // namespace

int pg_device_batch_sv_events_device(pg_ctx *ctx, pg_device_batch *b, const pg_variant_cand *d_sv_cands, const uint8_t *d_sv_counts)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    if (int rc = sv_events_refusal(ctx, b, d_sv_cands, d_sv_counts)) return rc;
    if (int rc = check_cand_set(ctx, b->n, "sv events", CandSet(nullptr, nullptr, d_sv_cands, d_sv_counts), CA_SV_PAIRS)) return rc;
    return build_sv_events(ctx, b, d_sv_cands);
}

int pg_device_batch_sv_events(pg_ctx *ctx, pg_device_batch *b, const pg_variant_cand *sv_cands, const uint8_t *sv_counts)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    if (int rc = sv_events_refusal(ctx, b, sv_cands, sv_counts)) return rc;
    DevTemps tmp(ctx, b);
    CandSet dev;                                              // (the build reads the records only: the count bytes stay where they are)
    if (int rc = stage_cand_set(ctx, tmp, b->n, CandSet(nullptr, nullptr, sv_cands, sv_counts), 1u << CA_SV_CANDS, &dev)) return rc;
    return build_sv_events(ctx, b, dev.sv_cands());
}

int pg_device_batch_sv_event_sizes(pg_ctx *ctx, pg_device_batch *b, pg_sv_event_sizes *sizes)
{
    use_device(ctx);
    if (!ctx || !b || !sizes) return PG_E_INVALID;
    if (!b->cls.svev_built) return fail(ctx, PG_E_INVALID, NO_SV_TABLES);
    *sizes = b->cls.svev_sizes;
    return PG_OK;
}

static int sv_events_download(pg_ctx *ctx, pg_device_batch *b, uint32_t *members, pg_event *events, bool to_device)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    const ClassifierState &c = b->cls;
    if (!c.svev_built) return fail(ctx, PG_E_INVALID, NO_SV_TABLES);
    size_t nm = 0, ne = 0;
    for (int t = 0; t < PG_SV_EVENT_TABLES; t++) {
        nm += c.svev_sizes.members[t];
        ne += c.svev_sizes.events[t];
    }
    return copy_tables(ctx,
                       { { members, c.svev_members, nm, sizeof(uint32_t), 4, "sv events download: members" },
                         { events, c.svev_events, ne, sizeof(pg_event), 4, "sv events download: events" } },
                       to_device);
}

int pg_device_batch_sv_events_download(pg_ctx *ctx, pg_device_batch *b, uint32_t *members, pg_event *events)
{
    return sv_events_download(ctx, b, members, events, false);
}

int pg_device_batch_sv_events_download_device(pg_ctx *ctx, pg_device_batch *b, uint32_t *d_members, pg_event *d_events)
{
    return sv_events_download(ctx, b, d_members, d_events, true);
}

// ---- ... its fifth part (pg_report.hip): the report records per table member and per read
namespace {
int report_refusal(pg_ctx *ctx, pg_device_batch *b, const CandSet &s)
{
    if (int rc = entry_refusal(ctx, b, true)) return rc;
    if (!b->cls.ev_built) return fail(ctx, PG_E_INVALID, "report reads: pg_device_batch_events has not been run on this batch");
    if (!b->cls.svev_built) return fail(ctx, PG_E_INVALID, "report reads: pg_device_batch_sv_events has not been run on this batch since its events build");
    if (b->n && (!s.cands() || !s.counts() || !s.sv_cands() || !s.sv_counts())) return fail(ctx, PG_E_INVALID, "report reads: null candidate arrays");
    return PG_OK;
}

// every list of d is device memory
int build_report(pg_ctx *ctx, pg_device_batch *b, const CandSet &d)
{
    ClassifierState &c = b->cls;
    c.begin_build(ClassifierState::REPORT);
    c.rr_n_records = 0;
    const size_t n = b->n;
    if (!n) {                                                 // nothing is launched for an empty batch
        c.rr_built = true;
        return PG_OK;
    }
    int rc;
    // (each buffer on its own: an allocation that failed in an earlier call is tried again, never launched with)
    if ((!c.rr_records && (rc = dev_alloc(ctx, &c.rr_records, n))) || (!c.rr_summaries && (rc = dev_alloc(ctx, &c.rr_summaries, n)))) return rc;
    PgReportArgs a{};
    uint64_t total = 0;
    for (int t = 0; t < PG_REPORT_TABLES; t++) {
        a.start[t] = (uint32_t)total;
        total += t < PG_EVENT_TABLES ? c.ev_sizes.members[t] : c.svev_sizes.members[t - PG_EVENT_TABLES];
    }
    // (a read is boxed at most once: the seven lists together hold at most n members, the size of the record buffer)
    if (total > n) return fail(ctx, PG_E_DEVICE, "report reads: the tables hold more members than the batch has reads");
    a.start[PG_REPORT_TABLES] = (uint32_t)total;
    a.out = b->out_rec;
    a.pool = b->pool;
    a.pool_runs = pool_runs(b);
    a.strand = b->strand;
    a.n = b->n;
    a.cands = d.cands();
    a.counts = d.counts();
    a.sv_cands = d.sv_cands();
    a.sv_counts = d.sv_counts();
    a.reads = c.ev_reads;
    a.ev_members = c.ev_members;
    a.sv_members = c.svev_members;
    a.records = c.rr_records;
    a.summaries = c.rr_summaries;
    rc = timed(ctx, [&]() -> int {
        if (pg_report_launch(&a, ctx->stream)) return fail(ctx, PG_E_DEVICE, "launching the report record kernels failed");
        log_kernel(ctx, PG_KERNEL_REPORT, (int32_t)PG_EV_BLOCK);
        return PG_OK;
    });
    if (rc) return rc;
    c.rr_n_records = total;
    c.rr_built = true;
    return PG_OK;
}
const char *const NO_REPORT = "no report records: pg_device_batch_report_reads has not been run on this batch since its table builds";
}  // namespace

int pg_device_batch_report_reads_device(pg_ctx *ctx, pg_device_batch *b, const pg_variant_cand *d_cands, const uint8_t *d_counts,
                                        const pg_variant_cand *d_sv_cands, const uint8_t *d_sv_counts)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    const CandSet dev(d_cands, d_counts, d_sv_cands, d_sv_counts);
    if (int rc = report_refusal(ctx, b, dev)) return rc;
    if (int rc = check_cand_set(ctx, b->n, "report reads", dev, CA_PAIRS | CA_SV_PAIRS)) return rc;
    return build_report(ctx, b, dev);
}

int pg_device_batch_report_reads(pg_ctx *ctx, pg_device_batch *b, const pg_variant_cand *cands, const uint8_t *counts,
                                 const pg_variant_cand *sv_cands, const uint8_t *sv_counts)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    const CandSet host(cands, counts, sv_cands, sv_counts);
    if (int rc = report_refusal(ctx, b, host)) return rc;
    DevTemps tmp(ctx, b);
    CandSet dev;
    if (int rc = stage_cand_set(ctx, tmp, b->n, host, CA_PAIRS | CA_SV_PAIRS, &dev)) return rc;
    return build_report(ctx, b, dev);
}

int pg_device_batch_report_sizes(pg_ctx *ctx, pg_device_batch *b, pg_report_sizes *sizes)
{
    use_device(ctx);
    if (!ctx || !b || !sizes) return PG_E_INVALID;
    if (!b->cls.rr_built) return fail(ctx, PG_E_INVALID, NO_REPORT);
    sizes->records = b->cls.rr_n_records;
    sizes->reads = b->n;
    return PG_OK;
}

static int report_download(pg_ctx *ctx, pg_device_batch *b, pg_report_read *records, pg_report_summary *summaries, bool to_device)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    const ClassifierState &c = b->cls;
    if (!c.rr_built) return fail(ctx, PG_E_INVALID, NO_REPORT);
    return copy_tables(ctx,
                       { { records, c.rr_records, (size_t)c.rr_n_records, sizeof(pg_report_read), 4, "report download: records" },
                         { summaries, c.rr_summaries, b->n, sizeof(pg_report_summary), 4, "report download: summaries" } },
                       to_device);
}

int pg_device_batch_report_download(pg_ctx *ctx, pg_device_batch *b, pg_report_read *records, pg_report_summary *summaries)
{
    return report_download(ctx, b, records, summaries, false);
}

int pg_device_batch_report_download_device(pg_ctx *ctx, pg_device_batch *b, pg_report_read *d_records, pg_report_summary *d_summaries)
{
    return report_download(ctx, b, d_records, d_summaries, true);
}

// ---- ... its sixth part (pg_li.hip): the long-insertion position tables
int pg_device_batch_li(pg_ctx *ctx, pg_device_batch *b, const pg_li_window *window)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    if (int rc = entry_refusal(ctx, b, true)) return rc;
    ClassifierState &c = b->cls;
    if (!c.ev_built) return fail(ctx, PG_E_INVALID, "li: pg_device_batch_events has not been run on this batch");
    if (!window) return fail(ctx, PG_E_INVALID, "li: null pg_li_window");
    if (window->lo > window->hi) return fail(ctx, PG_E_INVALID, "li: lo > hi");
    c.begin_build(ClassifierState::LI);
    c.li_sizes = pg_li_sizes{};
    const size_t n = b->n;
    if (!n) {                                                 // nothing is launched for an empty batch
        c.li_built = true;
        return PG_OK;
    }
    int rc;
    // (each buffer on its own: an allocation that failed in an earlier call is tried again, never launched with)
    if ((!c.li_members && (rc = dev_alloc(ctx, &c.li_members, n))) || (!c.li_positions && (rc = dev_alloc(ctx, &c.li_positions, n)))) return rc;
    DevTemps tmp(ctx, b);
    PgLiArgs a{};
    const size_t n_blk = n / PG_EV_BLOCK + 2;
    if ((rc = tmp.take(&a.rec_a, n)) || (rc = tmp.take(&a.rec_b, n)) || (rc = tmp.take(&a.flag, n)) || (rc = tmp.take(&a.rank, n)) ||
        (rc = tmp.take(&a.blk, n_blk)) || (rc = tmp.take(&a.pfirst, n + 1)) || (rc = tmp.take(&a.digit_cnt, 256 * n_blk + 1)) ||
        (rc = tmp.take(&a.info, 1)))
        return rc;
    a.out = b->out_rec;
    a.pool_runs = pool_runs(b);
    a.seq = b->seq;
    a.seq_off = b->seq_off;
    a.strand = b->strand;
    a.chr = b->chr;
    a.reads = c.ev_reads;
    a.n = b->n;
    a.chr_id = c.ev_window.chr_id;
    a.lo = window->lo;
    a.hi = window->hi;
    a.members = c.li_members;
    a.positions = c.li_positions;
    PgLiInfo info;
    uint32_t n_li = 0, n_plus = 0;
    rc = timed(ctx, [&]() -> int {
        if (pg_li_gather_launch(&a, ctx->stream)) return fail(ctx, PG_E_DEVICE, "launching the long-insertion gather kernels failed");
        log_kernel(ctx, PG_KERNEL_LI, (int32_t)PG_EV_BLOCK);
        HIP_TRY(ctx, hipMemcpyAsync(&info, a.info, sizeof info, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (info.n_li > n || info.n_plus > info.n_li) return fail(ctx, PG_E_DEVICE, "li: the count of long-insertion reads exceeds the batch");
        n_li = info.n_li;
        n_plus = info.n_plus;
        if (!n_li) return PG_OK;                              // (no LI read: nothing below indexes an empty array)
        PgLiRec *src = a.rec_b, *dst = a.rec_a;
        for (int pass = 0; pass < PG_LI_SORT_PASSES; pass++) {
            const int word = pass >= 4 ? 1 : 0, shift = pass >= 4 ? 0 : pass * 8;
            if ((((info.key_or[word] ^ info.key_and[word]) >> shift) & 0xffu) == 0u) continue;      // the byte is constant: no pass
            if (pg_li_sort_pass_launch(&a, src, dst, n_li, pass, ctx->stream)) return fail(ctx, PG_E_DEVICE, "launching a long-insertion sort pass failed");
            log_kernel(ctx, PG_KERNEL_LI, (int32_t)PG_EV_BLOCK);
            std::swap(src, dst);
        }
        if (pg_li_tables_launch(&a, src, n_li, n_plus, ctx->stream)) return fail(ctx, PG_E_DEVICE, "launching the long-insertion table kernels failed");
        log_kernel(ctx, PG_KERNEL_LI, (int32_t)PG_EV_BLOCK);
        HIP_TRY(ctx, hipMemcpyAsync(&info, a.info, sizeof info, hipMemcpyDeviceToHost, ctx->stream));
        return PG_OK;
    });
    if (rc) return rc;
    if (n_li) {
        if (info.n_pos > n_li || info.pos_plus > info.n_pos) return fail(ctx, PG_E_DEVICE, "li: inconsistent table sizes");
        c.li_sizes.members[0] = n_plus;
        c.li_sizes.members[1] = n_li - n_plus;
        c.li_sizes.positions[0] = info.pos_plus;
        c.li_sizes.positions[1] = info.n_pos - info.pos_plus;
    }
    c.li_built = true;
    return PG_OK;
}

static const char *const NO_LI = "no long-insertion tables: pg_device_batch_li has not been run on this batch since its events build";

int pg_device_batch_li_sizes(pg_ctx *ctx, pg_device_batch *b, pg_li_sizes *sizes)
{
    use_device(ctx);
    if (!ctx || !b || !sizes) return PG_E_INVALID;
    if (!b->cls.li_built) return fail(ctx, PG_E_INVALID, NO_LI);
    *sizes = b->cls.li_sizes;
    return PG_OK;
}

static int li_download(pg_ctx *ctx, pg_device_batch *b, uint32_t *members, pg_li_pos *positions, bool to_device)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    const ClassifierState &c = b->cls;
    if (!c.li_built) return fail(ctx, PG_E_INVALID, NO_LI);
    const size_t nm = (size_t)(c.li_sizes.members[0] + c.li_sizes.members[1]), np = (size_t)(c.li_sizes.positions[0] + c.li_sizes.positions[1]);
    return copy_tables(ctx,
                       { { members, c.li_members, nm, sizeof(uint32_t), 4, "li download: members" },
                         { positions, c.li_positions, np, sizeof(pg_li_pos), 4, "li download: positions" } },
                       to_device);
}

int pg_device_batch_li_download(pg_ctx *ctx, pg_device_batch *b, uint32_t *members, pg_li_pos *positions)
{
    return li_download(ctx, b, members, positions, false);
}

int pg_device_batch_li_download_device(pg_ctx *ctx, pg_device_batch *b, uint32_t *d_members, pg_li_pos *d_positions)
{
    return li_download(ctx, b, d_members, d_positions, true);
}

// ---- ... its seventh part (pg_int.hip): the interchromosomal junction tables, from the search result alone
int pg_device_batch_int(pg_ctx *ctx, pg_device_batch *b, const pg_int_window *window)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    if (int rc = entry_refusal(ctx, b, true)) return rc;
    if (!window) return fail(ctx, PG_E_INVALID, "int: null pg_int_window");
    if (!window->chr_rank) return fail(ctx, PG_E_INVALID, "int: null chr_rank");
    if (window->n_chr != ctx->names.size()) return fail(ctx, PG_E_INVALID, "int: n_chr is not the number of chromosomes of the loaded reference");
    ClassifierState &c = b->cls;
    c.int_built = false;
    c.int_sizes = pg_int_sizes{};
    const size_t n = b->n;
    if (!n) {                                                 // nothing is launched for an empty batch
        c.int_built = true;
        return PG_OK;
    }
    int rc;
    // (each buffer on its own: an allocation that failed in an earlier call is tried again, never launched with)
    if ((!c.int_members && (rc = dev_alloc(ctx, &c.int_members, n))) || (!c.int_calls && (rc = dev_alloc(ctx, &c.int_calls, n)))) return rc;
    DevTemps tmp(ctx, b);
    PgIntArgs a{};
    const size_t n_blk = n / PG_EV_BLOCK + 2;
    int32_t *d_rank = nullptr;
    if ((rc = tmp.take(&a.rec_a, n)) || (rc = tmp.take(&a.rec_b, n)) || (rc = tmp.take(&a.flag, n)) || (rc = tmp.take(&a.rank, n)) ||
        (rc = tmp.take(&a.blk, n_blk)) || (rc = tmp.take(&a.cfirst, n + 1)) || (rc = tmp.take(&a.digit_cnt, 256 * n_blk + 1)) ||
        (rc = tmp.take(&a.info, 1)) || (rc = tmp.take(&d_rank, window->n_chr)))
        return rc;
    HIP_TRY(ctx, hipMemcpy(d_rank, window->chr_rank, window->n_chr * sizeof(int32_t), hipMemcpyHostToDevice));
    a.out = b->out_rec;
    a.pool = b->pool;
    a.pool_runs = pool_runs(b);
    a.seq = b->seq;
    a.seq_off = b->seq_off;
    a.strand = b->strand;
    a.chr = b->chr;
    a.chr_rank = d_rank;
    a.n = b->n;
    a.n_chr = window->n_chr;
    a.members = c.int_members;
    a.calls = c.int_calls;
    PgIntInfo info;
    uint32_t n_mem = 0;
    rc = timed(ctx, [&]() -> int {
        if (pg_int_gather_launch(&a, ctx->stream)) return fail(ctx, PG_E_DEVICE, "launching the junction gather kernels failed");
        log_kernel(ctx, PG_KERNEL_INT, (int32_t)PG_EV_BLOCK);
        HIP_TRY(ctx, hipMemcpyAsync(&info, a.info, sizeof info, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (info.n_mem > n) return fail(ctx, PG_E_DEVICE, "int: the count of reads with a call exceeds the batch");
        n_mem = info.n_mem;
        if (!n_mem) return PG_OK;                             // (no read with a call: nothing below indexes an empty array)
        PgIntRec *src = a.rec_b, *dst = a.rec_a;
        for (int pass = 0; pass < PG_INT_SORT_PASSES; pass++) {
            const int word = pass < 12 ? pass >> 2 : pass == 12 ? 3 : 4, shift = (pass < 12 ? pass & 3 : pass == 12 ? 0 : pass - 13) * 8;
            if ((((info.key_or[word] ^ info.key_and[word]) >> shift) & 0xffu) == 0u) continue;      // the byte is constant: no pass
            if (pg_int_sort_pass_launch(&a, src, dst, n_mem, pass, ctx->stream)) return fail(ctx, PG_E_DEVICE, "launching a junction sort pass failed");
            log_kernel(ctx, PG_KERNEL_INT, (int32_t)PG_EV_BLOCK);
            std::swap(src, dst);
        }
        if (pg_int_tables_launch(&a, src, n_mem, ctx->stream)) return fail(ctx, PG_E_DEVICE, "launching the junction table kernels failed");
        log_kernel(ctx, PG_KERNEL_INT, (int32_t)PG_EV_BLOCK);
        HIP_TRY(ctx, hipMemcpyAsync(&info, a.info, sizeof info, hipMemcpyDeviceToHost, ctx->stream));
        return PG_OK;
    });
    if (rc) return rc;
    if (n_mem) {
        if (!info.n_calls || info.n_calls > n_mem) return fail(ctx, PG_E_DEVICE, "int: inconsistent table sizes");
        c.int_sizes.members = n_mem;
        c.int_sizes.calls = info.n_calls;
    }
    c.int_built = true;
    return PG_OK;
}

static const char *const NO_INT = "no junction tables: pg_device_batch_int has not been run on this batch since its search";

int pg_device_batch_int_sizes(pg_ctx *ctx, pg_device_batch *b, pg_int_sizes *sizes)
{
    use_device(ctx);
    if (!ctx || !b || !sizes) return PG_E_INVALID;
    if (!b->cls.int_built) return fail(ctx, PG_E_INVALID, NO_INT);
    *sizes = b->cls.int_sizes;
    return PG_OK;
}

static int int_download(pg_ctx *ctx, pg_device_batch *b, uint32_t *members, pg_int_call *calls, bool to_device)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    const ClassifierState &c = b->cls;
    if (!c.int_built) return fail(ctx, PG_E_INVALID, NO_INT);
    return copy_tables(ctx,
                       { { members, c.int_members, (size_t)c.int_sizes.members, sizeof(uint32_t), 4, "int download: members" },
                         { calls, c.int_calls, (size_t)c.int_sizes.calls, sizeof(pg_int_call), 4, "int download: calls" } },
                       to_device);
}

int pg_device_batch_int_download(pg_ctx *ctx, pg_device_batch *b, uint32_t *members, pg_int_call *calls)
{
    return int_download(ctx, b, members, calls, false);
}

int pg_device_batch_int_download_device(pg_ctx *ctx, pg_device_batch *b, uint32_t *d_members, pg_int_call *d_calls)
{
    return int_download(ctx, b, d_members, d_calls, true);
}

// ---- ... its eighth part (pg_dd_tables.hip): the dispersed-duplication breakpoint tables, their consensus and the
// containment verdicts, from the close end alone
int pg_device_batch_dd(pg_ctx *ctx, pg_device_batch *b, const pg_dd_window *window)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    if (int rc = entry_refusal(ctx, b, false)) return rc;
    if (b->n && !b->close_searched) return fail(ctx, PG_E_INVALID, "dd: the batch has not been close-searched: no close ends to group");
    if (!window) return fail(ctx, PG_E_INVALID, "dd: null pg_dd_window");
    const uint32_t n_seg = window->n_seg;
    if (n_seg && (!window->seg_first || !window->seg_strand)) return fail(ctx, PG_E_INVALID, "dd: n_seg > 0 with a null segment array");
    for (uint32_t s = 0; s < n_seg; s++) {
        if (window->seg_first[s] > window->seg_first[s + 1]) return fail(ctx, PG_E_INVALID, "dd: seg_first decreases");
        if (window->seg_strand[s] != '+' && window->seg_strand[s] != '-') return fail(ctx, PG_E_INVALID, "dd: a segment strand is neither '+' nor '-'");
    }
    if (n_seg && window->seg_first[n_seg] > b->n) return fail(ctx, PG_E_INVALID, "dd: seg_first reaches beyond the batch's reads");
    if (window->chr_id < 0 || (size_t)window->chr_id >= ctx->names.size()) return fail(ctx, PG_E_INVALID, "dd: chr_id is not a chromosome of the loaded reference");
    if (window->min_map_distance < 1) return fail(ctx, PG_E_INVALID, "dd: min_map_distance < 1");
    ClassifierState &c = b->cls;
    c.dd_built = false;
    c.dd_sizes = pg_dd_sizes{};
    // (the tables are sized by what the build finds: its predecessor's go first)
    for (void *p : { (void *)c.dd_members, (void *)c.dd_cands, (void *)c.dd_cons })
        if (p) (void)hipFree(p);
    c.dd_members = nullptr;
    c.dd_cands = nullptr;
    c.dd_cons = nullptr;
    const size_t n = b->n;
    if (!n || !n_seg) {                                       // nothing is launched for an empty batch or without a segment
        c.dd_built = true;
        return PG_OK;
    }
    int rc;
    DevTemps tmp(ctx, b);
    PgDdArgs a{};
    const size_t n_blk = n / PG_EV_BLOCK + 2;
    uint32_t *d_seg_first = nullptr;
    uint8_t *d_seg_strand = nullptr;
    // (one sized block for the read-sized temporaries, a second one below for the candidate-sized ones: a resident batch lives
    // outside the arena, where every array of its own would be a hipMalloc and a hipFree)
    {
        TempBlock blk;
        blk.add(&a.rec_a, n), blk.add(&a.rec_b, n), blk.add(&a.aux, n), blk.add(&a.flag, n), blk.add(&a.keep, n), blk.add(&a.keep_head, n);
        blk.add(&a.rank, n), blk.add(&a.blk, n_blk), blk.add(&a.rank_m, n), blk.add(&a.blk_m, n_blk), blk.add(&a.rank_c, n), blk.add(&a.blk_c, n_blk);
        blk.add(&a.cfirst, n + 1), blk.add(&a.digit_cnt, 256 * n_blk + 1), blk.add(&a.info, 1);
        blk.add(&d_seg_first, (size_t)n_seg + 1), blk.add(&d_seg_strand, n_seg);
        if ((rc = blk.take(ctx, tmp))) return rc;
    }
    HIP_TRY(ctx, hipMemcpy(d_seg_first, window->seg_first, ((size_t)n_seg + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(d_seg_strand, window->seg_strand, n_seg, hipMemcpyHostToDevice));
    a.out = b->out_rec;
    a.seq = b->seq;
    a.seq_off = b->seq_off;
    a.strand = b->strand;
    a.seg_first = d_seg_first;
    a.seg_strand = d_seg_strand;
    a.n = b->n;
    a.n_seg = n_seg;
    a.chr_id = window->chr_id;
    a.min_bp_support = window->min_bp_support;
    a.min_map_distance = window->min_map_distance;
    a.chr_size = (uint32_t)ctx->comp_size[(size_t)window->chr_id];
    a.slot = std::max<uint32_t>(b->max_len, 1u);
    PgDdInfo info;
    uint32_t n_dd = 0, n_mem = 0, n_cands = 0, cons_bytes = 0;
    PgDdRec *sorted = nullptr;
    double ms = 0.0;
    // A, B and the first half of C: which keys are candidates
    rc = timed(ctx, [&]() -> int {
        if (pg_ddt_gather_launch(&a, ctx->stream)) return fail(ctx, PG_E_DEVICE, "launching the DD gather kernels failed");
        log_kernel(ctx, PG_KERNEL_DD_TABLES, (int32_t)PG_EV_BLOCK);
        HIP_TRY(ctx, hipMemcpyAsync(&info, a.info, sizeof info, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (info.n_dd > n) return fail(ctx, PG_E_DEVICE, "dd: the count of DD reads exceeds the batch");
        n_dd = info.n_dd;
        if (!n_dd) return PG_OK;                              // (no DD read: nothing below indexes an empty array)
        PgDdRec *src = a.rec_b, *dst = a.rec_a;
        for (int pass = 0; pass < PG_DD_SORT_PASSES; pass++) {
            const int word = pass < 4 ? 1 : 0, shift = (pass & 3) * 8;
            if ((((info.key_or[word] ^ info.key_and[word]) >> shift) & 0xffu) == 0u) continue;      // the byte is constant: no pass
            if (pg_ddt_sort_pass_launch(&a, src, dst, n_dd, pass, ctx->stream)) return fail(ctx, PG_E_DEVICE, "launching a DD sort pass failed");
            log_kernel(ctx, PG_KERNEL_DD_TABLES, (int32_t)PG_EV_BLOCK);
            std::swap(src, dst);
        }
        sorted = src;
        if (pg_ddt_keys_launch(&a, sorted, n_dd, ctx->stream)) return fail(ctx, PG_E_DEVICE, "launching the DD key kernels failed");
        log_kernel(ctx, PG_KERNEL_DD_TABLES, (int32_t)PG_EV_BLOCK);
        HIP_TRY(ctx, hipMemcpyAsync(&info, a.info, sizeof info, hipMemcpyDeviceToHost, ctx->stream));
        return PG_OK;
    });
    if (rc) return rc;
    ms += ctx->last_ms;
    if (n_dd) {
        if (info.n_mem > n_dd || info.n_cands > info.n_mem || (info.n_mem && !info.n_cands)) return fail(ctx, PG_E_DEVICE, "dd: inconsistent table sizes");
        n_mem = info.n_mem;
        n_cands = info.n_cands;
    }
    if (n_cands) {
        if ((rc = dev_alloc(ctx, &c.dd_members, n_mem)) || (rc = dev_alloc(ctx, &c.dd_cands, n_cands))) return rc;
        {
            TempBlock blk;
            blk.add(&a.slots, (size_t)n_cands * a.slot), blk.add(&a.cons_off, (size_t)n_cands + 1), blk.add(&a.q_off, (size_t)n_cands + 1);
            blk.add(&a.q_chr, n_cands), blk.add(&a.q_ws, n_cands), blk.add(&a.q_wl, n_cands), blk.add(&a.q_out, 2 * (size_t)n_cands);
            if ((rc = blk.take(ctx, tmp))) return rc;
        }
        a.members = c.dd_members;
        a.cands = c.dd_cands;
        // the second half of C, and D up to the lengths' scan
        rc = timed(ctx, [&]() -> int {
            if (pg_ddt_tables_launch(&a, sorted, n_dd, ctx->stream) || pg_ddt_consensus_launch(&a, n_cands, ctx->stream))
                return fail(ctx, PG_E_DEVICE, "launching the DD table and consensus kernels failed");
            log_kernel(ctx, PG_KERNEL_DD_TABLES, (int32_t)(PG_DD_WAVES * 64u));
            HIP_TRY(ctx, hipMemcpyAsync(&cons_bytes, a.cons_off + n_cands, sizeof cons_bytes, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(&info, a.info, sizeof info, hipMemcpyDeviceToHost, ctx->stream));
            return PG_OK;
        });
        if (rc) return rc;
        ms += ctx->last_ms;
        if ((uint64_t)cons_bytes > (uint64_t)n_cands * a.slot || info.max_cons > a.slot || info.n_tested > n_cands)
            return fail(ctx, PG_E_DEVICE, "dd: inconsistent consensus sizes");
        if ((rc = dev_alloc(ctx, &c.dd_cons, cons_bytes))) return rc;
        a.cons = c.dd_cons;
        // E: the containment kernel as pg_dd_contains_batch launches it -- one wave per (candidate, strand), at most 8192 resident
        // waves; with a consensus of more than 64 bases each wave keeps one boundary row of its window, capped at 512 MB in all
        const uint64_t n_tasks = 2ull * n_cands;
        const uint64_t max_win = std::min<uint64_t>(2ull * (uint64_t)window->min_map_distance, a.chr_size);
        const uint64_t stride = info.max_cons > 64 ? (max_win + 63) / 64 * 64 : 0;
        uint64_t waves = std::min<uint64_t>(n_tasks, 8192);
        if (stride) waves = std::min<uint64_t>(waves, std::max<uint64_t>(4, (512ull << 20) / (stride * 4)));
        const uint64_t blocks = (waves + 3) / 4;
        uint32_t *d_scr = nullptr;
        if (info.n_tested && (rc = tmp.take(&d_scr, (size_t)(stride ? blocks * 4 * stride : 1)))) return rc;
        const PgDevRef ref = dev_ref(ctx);
        rc = timed(ctx, [&]() -> int {
            if (pg_ddt_pool_launch(&a, n_cands, ctx->stream)) return fail(ctx, PG_E_DEVICE, "launching the DD pool kernel failed");
            log_kernel(ctx, PG_KERNEL_DD_TABLES, (int32_t)(PG_DD_WAVES * 64u));
            if (!info.n_tested) return PG_OK;                 // (no consensus of 15 bases: no containment test, no flag to set)
            if (pg_dd_launch(&ref, ctx->d_mm, a.cons, a.q_off, a.q_chr, a.q_ws, a.q_wl, a.q_out, d_scr, std::max<uint64_t>(stride, 1),
                             (uint32_t)n_tasks, (uint32_t)blocks, ctx->stream))
                return fail(ctx, PG_E_DEVICE, "launching the containment kernel failed");
            if (pg_ddt_verdict_launch(&a, n_cands, ctx->stream)) return fail(ctx, PG_E_DEVICE, "launching the DD verdict kernel failed");
            log_kernel(ctx, PG_KERNEL_DD_TABLES, (int32_t)PG_EV_BLOCK);
            return PG_OK;
        });
        if (rc) return rc;
        ms += ctx->last_ms;
        c.dd_sizes.members = n_mem;
        c.dd_sizes.cands = n_cands;
        c.dd_sizes.cons_bytes = cons_bytes;
    }
    ctx->last_ms = ms;
    c.dd_built = true;
    return PG_OK;
}

static const char *const NO_DD = "no DD tables: pg_device_batch_dd has not been run on this batch since its search";

int pg_device_batch_dd_sizes(pg_ctx *ctx, pg_device_batch *b, pg_dd_sizes *sizes)
{
    use_device(ctx);
    if (!ctx || !b || !sizes) return PG_E_INVALID;
    if (!b->cls.dd_built) return fail(ctx, PG_E_INVALID, NO_DD);
    *sizes = b->cls.dd_sizes;
    return PG_OK;
}

static int dd_download(pg_ctx *ctx, pg_device_batch *b, pg_dd_member *members, pg_dd_cand *cands, uint8_t *cons, bool to_device)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    const ClassifierState &c = b->cls;
    if (!c.dd_built) return fail(ctx, PG_E_INVALID, NO_DD);
    return copy_tables(ctx,
                       { { members, c.dd_members, (size_t)c.dd_sizes.members, sizeof(pg_dd_member), 4, "dd download: members" },
                         { cands, c.dd_cands, (size_t)c.dd_sizes.cands, sizeof(pg_dd_cand), 8, "dd download: cands" },
                         { cons, c.dd_cons, (size_t)c.dd_sizes.cons_bytes, 1, 1, "dd download: cons" } },
                       to_device);
}

int pg_device_batch_dd_download(pg_ctx *ctx, pg_device_batch *b, pg_dd_member *members, pg_dd_cand *cands, uint8_t *cons)
{
    return dd_download(ctx, b, members, cands, cons, false);
}

int pg_device_batch_dd_download_device(pg_ctx *ctx, pg_device_batch *b, pg_dd_member *d_members, pg_dd_cand *d_cands, uint8_t *d_cons)
{
    return dd_download(ctx, b, d_members, d_cands, d_cons, true);
}

// ---- one call per window: the two candidate kernels, both table builds and the report records, the lists staying with the batch
int pg_device_batch_classify(pg_ctx *ctx, pg_device_batch *b, const pg_classify_params *p, const uint32_t *name_id)
{
    use_device(ctx);
    if (!ctx || !b) return PG_E_INVALID;
    if (!p) return fail(ctx, PG_E_INVALID, "classify: null pg_classify_params");
    // every stage's refusal before the first launch
    if (int rc = events_refusal(ctx, b, &p->window, false)) return rc;
    if (int rc = sv_params_ok(ctx, &p->sv)) return rc;
    if (p->max_listed < 0 || p->max_listed > PG_VARIANT_CANDS) return fail(ctx, PG_E_INVALID, "classify: max_listed must lie in [0, PG_VARIANT_CANDS]");
    if (b->n >= 0x80000000u) return fail(ctx, PG_E_INVALID, "classify: 2^31 reads or more (bit 31 of a member word is PG_SVEV_MEMBER_DUP)");
    const size_t n = b->n;
    ClassifierState &c = b->cls;
    int rc;
    // (each buffer on its own: an allocation that failed in an earlier call is tried again, never launched with)
    if (n && ((!c.cl_cands && (rc = dev_alloc(ctx, &c.cl_cands, cand_elems(CA_CANDS, n)))) ||
              (!c.cl_counts && (rc = dev_alloc(ctx, &c.cl_counts, cand_elems(CA_COUNTS, n)))) ||
              (!c.cl_sv_cands && (rc = dev_alloc(ctx, &c.cl_sv_cands, cand_elems(CA_SV_CANDS, n)))) ||
              (!c.cl_sv_counts && (rc = dev_alloc(ctx, &c.cl_sv_counts, cand_elems(CA_SV_COUNTS, n))))))
        return rc;
    DevTemps tmp(ctx, b);
    CandSet lists(c.cl_cands, c.cl_counts, c.cl_sv_cands, c.cl_sv_counts);
    if ((rc = stage_cand_set(ctx, tmp, n, CandSet(nullptr, nullptr, nullptr, nullptr, name_id), 1u << CA_NAME_ID, &lists))) return rc;
    double ms = 0.0;
    if ((rc = variant_candidates(ctx, b, c.cl_cands, c.cl_counts))) return rc;
    ms += ctx->last_ms;
    if ((rc = sv_candidates(ctx, b, &p->sv, c.cl_sv_cands, c.cl_sv_counts))) return rc;
    ms += ctx->last_ms;
    if (n && p->max_listed < PG_VARIANT_CANDS) {
        rc = timed(ctx, [&]() -> int {
            if (pg_report_cut_launch(c.cl_counts, c.cl_sv_counts, b->n, (uint32_t)p->max_listed, ctx->stream))
                return fail(ctx, PG_E_DEVICE, "launching the list cut kernel failed");
            log_kernel(ctx, PG_KERNEL_REPORT, 0);             // (0: the cut; PG_EV_BLOCK: the records)
            return PG_OK;
        });
        if (rc) return rc;
        ms += ctx->last_ms;
    }
    if ((rc = build_events(ctx, b, &p->window, lists))) return rc;
    ms += ctx->last_ms;
    if ((rc = build_sv_events(ctx, b, c.cl_sv_cands))) return rc;
    ms += ctx->last_ms;
    if ((rc = build_report(ctx, b, lists))) return rc;
    ctx->last_ms += ms;
    return PG_OK;
}
