// pg_events.hip -- the third part of the device classifier: from the candidate lists of a searched batch and one
// window description to event tables.  The host statement of the same function is pg_host_events.hpp; the two must agree byte for byte.
//   stage A  pg_events_cascade_kernel: one thread per read.  The window-dependent tail (bin boundary, region, box) of all seven
//            classifiers in process_window's order, with the Used cascade and the leftover NT_size carried from kind to kind.
//            A few dozen bytes of state over at most 19 records: no wave-wide work, so a thread, not a wave.
//   stage B  the boxed reads of the four sorted kinds are compacted in DESCENDING read index (rank, scan, fill) and ordered by LSD
//            counting passes over the key bytes, skipping the bytes that are constant over the batch.  Every pass is stable, so equal
//            keys keep the descending read index: the order bubblesortReads leaves (the argument above exchange_sort_reference in
//            pg_host_priv.hpp).  The table is the most significant digit and a box is a range of BPLeft, the primary key: ONE sort
//            yields every kind's sorted boxes one after the other, in box order.
//   stage C  markDuplicates per box: a read is a duplicate if an earlier read of its box has the same (Left, Right, name).  Every
//            read that arrives here is still UniqueRead -- a read is boxed at most once per window and only a reporter clears the
//            flag, on the reads of its own boxes -- so "earlier and equal" is the whole test.  Boxes below -M are marked too.
//   stage D  members = the unique reads in order; events = maximal runs of members with an equal key; one wave per event for the
//            support counts, ReportEvent's balance test and the left-aligned range (the 64-steps-per-ballot walks of pg_variant_align.h).
// Plain HIP, vector stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "pg_device.h"
#include "pg_table_prims.h"
#include "pg_variant_align.h"
#include "pg_variant_dev.h"

typedef uint32_t u32;
static_assert(PG_EV_BLOCK == 256u, "one thread per digit value in the counting kernels");
static_assert(sizeof(PgEventRec) == 32 && sizeof(pg_event) == 40 && sizeof(pg_event_read) == 8, "layouts of the tables");

namespace {

__device__ __forceinline__ int table_of(int kind) { return kind == 0 ? 0 : kind == 1 ? 1 : kind == PG_SV_TD ? 2 : kind == PG_SV_TD_NT ? 3 : -1; }
__device__ __forceinline__ int kind_of(int table) { return table == 0 ? 0 : table == 1 ? 1 : table == 2 ? PG_SV_TD : PG_SV_TD_NT; }

__device__ __forceinline__ u32 rec_table(const PgEventRec &r) { return r.w[7] & 0xffu; }
__device__ __forceinline__ bool rec_plus(const PgEventRec &r) { return (r.w[7] >> 8) & 1u; }
__device__ __forceinline__ int32_t rec_read_len(const PgEventRec &r) { return (int32_t)(int16_t)(r.w[7] >> 16); }
__device__ __forceinline__ u32 rec_nt(const PgEventRec &r) { return r.w[3] >> 16; }
__device__ __forceinline__ int32_t rec_bp(const PgEventRec &r) { return (int32_t)(int16_t)((r.w[3] & 0xffffu) ^ 0x8000u); }
// (boxed reads have 0 <= (int)BPLeft: the division is the host's)
__device__ __forceinline__ u32 rec_box(const PgEventRec &r, u32 box_size) { return (u32)((int32_t)r.w[0] / (int32_t)box_size); }

}  // namespace

// ---- stage A
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_events_cascade_kernel(PgEventArgs a)
{
    const u32 i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    pg_event_read rec = pg_event_read();
    uint8_t boxed_flag = 0;
    if (a.chr[i] == a.win.chr_id) {
        const bool plus = a.strand[i] == '+';
        const u32 twice_isz = (u32)(2 * (int32_t)a.isz[i]);
        u32 nt = 0;                                          // the leftover NT_size (unsigned short on the host)
        bool used = false;
        // process_window's order: kind 0, DI, TD and TD_NT, INV and INV_NT, kind 1
        for (int o = 0; o < 7 && !used; o++) {
            const int kind = o == 0 ? 0 : o == 6 ? 1 : o + 1;
            if ((kind == PG_SV_TD || kind == PG_SV_TD_NT) && !a.win.analyze_td) continue;
            if ((kind == PG_SV_INV || kind == PG_SV_INV_NT) && !a.win.analyze_inv) continue;
            const pg_variant_cand *list = nullptr;
            u32 count = 0, cap = 0;
            if (kind < 2) {
                if (a.cands) {
                    list = a.cands + ((size_t)i * 2u + (u32)kind) * PG_VARIANT_CANDS;
                    count = a.counts[(size_t)i * 2u + (u32)kind];
                    cap = PG_VARIANT_CANDS;
                }
            } else if (a.sv_cands) {
                const u32 slot0 = kind == PG_SV_DI ? 0u : kind == PG_SV_TD ? 1u : kind == PG_SV_TD_NT ? 1u + PG_VARIANT_CANDS
                                : kind == PG_SV_INV ? 2u + PG_VARIANT_CANDS : 2u + 2u * PG_VARIANT_CANDS;
                list = a.sv_cands + (size_t)i * PG_SV_SLOTS + slot0;
                count = a.sv_counts[(size_t)i * PG_SV_KINDS + (u32)(kind - PG_SV_DI)];
                cap = (kind == PG_SV_TD || kind == PG_SV_INV) ? PG_VARIANT_CANDS : 1u;
            }
            u32 n_listed = count & ~PG_VARIANT_MORE;
            if (n_listed > cap) n_listed = cap;
            for (u32 j = 0; j < n_listed && !used; j++) {
                const pg_variant_cand c = list[j];
                // readTransgressesBinBoundaries: BPRight > upper - 2 * InsertSize, unsigned, InsertSize a short
                const bool transgress = c.bp_right > a.win.win_end - twice_isz;
                const bool in_region = c.bp_left + 1u >= a.win.region_start && c.bp_left + 1u <= a.win.region_end;
                bool box_it = false;
                if (kind < 2) {
                    if (c.flags & PG_VARIANT_REF_END) used = true;                 // Used, and nothing is boxed
                    else if (transgress) used = true;
                    else if (in_region && (u32)((int32_t)c.bp_left / (int32_t)a.box_size) < a.n_boxes) box_it = used = true;
                } else {
                    if (kind != PG_SV_TD) nt = (u32)(uint16_t)c.nt_rot;            // (searchTandemDuplications leaves NT_size alone)
                    if (c.flags & PG_VARIANT_REF_END) used = true;                 // Used, and the box test still runs
                    const bool check = !(kind == PG_SV_INV && !plus);              // inversions with a '-' anchor skip the test
                    if (check && transgress) used = true;
                    else if (in_region && (u32)((int32_t)c.bp_left / (int32_t)a.box_size) < a.n_boxes) box_it = used = true;
                }
                if (used) {
                    rec.kind = (uint8_t)kind;
                    rec.slot = (uint8_t)j;
                    rec.flags = box_it ? PG_EVR_BOXED : PG_EVR_USED;
                    const int t = table_of(kind);
                    if (box_it) rec.nt_size = (uint16_t)nt;
                    if (box_it && t >= 0) {
                        const uint64_t s0 = a.seq_off[i];
                        int32_t lead;
                        const int32_t RL = post_state_len(a.seq + s0, (int32_t)(a.seq_off[i + 1] - s0), a.out[i].rc_flag, &lead);
                        PgEventRec r;
                        r.w[0] = c.bp_left;
                        r.w[1] = c.bp_right;
                        r.w[2] = c.indel_size;
                        r.w[3] = (nt << 16) | (((u32)(uint16_t)c.bp) ^ 0x8000u);
                        r.w[4] = (u32)c.left;
                        r.w[5] = (u32)c.right;
                        r.w[6] = i;
                        r.w[7] = (u32)t | ((u32)plus << 8) | ((u32)(uint16_t)RL << 16);
                        a.rec_a[i] = r;
                        boxed_flag = 1;
                    }
                }
            }
            if (!used && (count & PG_VARIANT_MORE)) {
                rec.flags = PG_EVR_UNRESOLVED;
                rec.unresolved_kind = (uint8_t)kind;
                atomicAdd(&a.info->n_unresolved, 1u);
                break;
            }
        }
    }
    a.reads[i] = rec;
    a.flag[i] = boxed_flag;
}

// the boxed reads to rec_b in descending read index; the masks of their key bytes
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_events_compact_kernel(PgEventArgs a)
{
    const u32 i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    const u32 nb = a.blk[(a.n + PG_EV_BLOCK - 1u) / PG_EV_BLOCK];
    const bool mine = i < a.n && a.flag[i];
    u32 k_or[5] = { 0u, 0u, 0u, 0u, 0u }, k_and[5] = { ~0u, ~0u, ~0u, ~0u, ~0u };
    if (mine) {
        const PgEventRec r = a.rec_a[i];
        a.rec_b[nb - 1u - (a.rank[i] + a.blk[blockIdx.x])] = r;
        for (int k = 0; k < 4; k++) k_or[k] = k_and[k] = r.w[k];
        k_or[4] = k_and[4] = rec_table(r);
    }
    for (int k = 0; k < 5; k++) {
        const u32 o = wave_or(k_or[k]), n = wave_and(k_and[k]);
        if ((threadIdx.x & 63u) == 0u) {
            if (o) atomicOr(&a.info->key_or[k], o);
            if (n != ~0u) atomicAnd(&a.info->key_and[k], n);
        }
    }
    if (i == 0u) a.info->n_boxed = nb;
}

// ---- stage B: one counting pass.  Key byte `pass`, least significant first: w[3] (BP biased, NT_size), w[2], w[1], w[0], the table
namespace {
__device__ __forceinline__ u32 key_digit(const PgEventRec &r, int pass)
{
    if (pass >= 16) return rec_table(r);
    return (r.w[3 - (pass >> 2)] >> ((pass & 3) * 8)) & 0xffu;
}
}  // namespace

extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_events_digit_count_kernel(const PgEventRec *src, u32 m, int pass, u32 n_blk, u32 *cnt)
{
    tab_digit_count(src, m, n_blk, cnt, [pass](const PgEventRec &r) { return key_digit(r, pass); });
}
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_events_scatter_kernel(const PgEventRec *src, PgEventRec *dst, u32 m, int pass, u32 n_blk,
                                                                                    const u32 *cnt)
{
    tab_scatter(src, dst, m, n_blk, cnt, [pass](const PgEventRec &r) { return key_digit(r, pass); });
}

// ---- stage C: flag[i] = the read is unique.  The walk back over the box is the literal one: quadratic in the size of a box
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_events_unique_kernel(PgEventArgs a, const PgEventRec *s, u32 m)
{
    const u32 i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (i >= m) return;
    bool dup = false;
    if (a.name_id) {                                         // (no name ids: every name differs, nothing is a duplicate)
        const PgEventRec r = s[i];
        const u32 box = rec_box(r, a.box_size), name = a.name_id[r.w[6]];
        for (u32 j = i; j-- > 0u && !dup;) {
            const PgEventRec q = s[j];
            if (rec_table(q) != rec_table(r) || rec_box(q, a.box_size) != box) break;
            dup = q.w[4] == r.w[4] && q.w[5] == r.w[5] && a.name_id[q.w[6]] == name;
        }
        if (dup) a.reads[r.w[6]].flags |= PG_EVR_DUPLICATE;
    }
    a.flag[i] = dup ? 0 : 1;
}

// members[m] = the read, midx[m] = its sorted record, for the unique ones
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_events_member_kernel(PgEventArgs a, const PgEventRec *s, u32 m)
{
    const u32 i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (i >= m || !a.flag[i]) return;
    const u32 at = a.rank[i] + a.blk[blockIdx.x];
    a.members[at] = s[i].w[6];
    a.midx[at] = i;
}

namespace {
// the event key: (BPLeft, BPRight), or (BPLeft, IndelSize) for kind 1 -- a run, not a group: the sort key has BPRight in between
__device__ __forceinline__ bool same_event(const PgEventRec &x, const PgEventRec &y)
{
    if (rec_table(x) != rec_table(y) || x.w[0] != y.w[0]) return false;
    return rec_table(x) == 1u ? x.w[2] == y.w[2] : x.w[1] == y.w[1];
}
}  // namespace

// flag[m] = member m opens an event (the unique flags have been consumed by then; their total moves to info)
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_events_head_kernel(PgEventArgs a, const PgEventRec *s, u32 n_boxed)
{
    const u32 nm = a.blk[(n_boxed + PG_EV_BLOCK - 1u) / PG_EV_BLOCK];       // the total the scan of the unique flags left
    const u32 m = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (m == 0u) a.info->n_members = nm;
    if (m >= n_boxed) return;
    a.flag[m] = m < nm ? (uint8_t)(m == 0u || !same_event(s[a.midx[m - 1u]], s[a.midx[m]])) : (uint8_t)0;
}
// efirst[e] = the first member of event e (one entry more: the number of members); the tables' first members and events
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_events_first_kernel(PgEventArgs a, const PgEventRec *s, u32 n_boxed)
{
    const u32 nm = a.info->n_members;
    const u32 ne = a.blk[(n_boxed + PG_EV_BLOCK - 1u) / PG_EV_BLOCK];
    const u32 m = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (m == 0u) {
        a.info->n_events = ne;
        a.efirst[ne] = nm;
        a.info->member_start[PG_EVENT_TABLES] = nm;
        a.info->event_start[PG_EVENT_TABLES] = ne;
    }
    if (m >= nm) return;
    const u32 e = a.rank[m] + a.blk[blockIdx.x];
    if (a.flag[m]) a.efirst[e] = m;
    // the first member of a table starts that table and the empty ones before it; the last member ends the ones behind its own
    const u32 t = rec_table(s[a.midx[m]]);
    const u32 t_from = m ? rec_table(s[a.midx[m - 1u]]) + 1u : 0u;
    for (u32 k = t_from; k <= t; k++) {
        a.info->member_start[k] = m;
        a.info->event_start[k] = e;
    }
    if (m == nm - 1u)
        for (u32 k = t + 1u; k < PG_EVENT_TABLES; k++) {
            a.info->member_start[k] = nm;
            a.info->event_start[k] = ne;
        }
}

// ---- stage D: one wave per event
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_events_event_kernel(PgDevRef ref, PgEventArgs a, const PgEventRec *s, const u32 *efirst)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 e = blockIdx.x * (PG_EV_BLOCK / 64u) + (threadIdx.x >> 6);
    if (e >= a.info->n_events) return;                        // (whole waves)
    const u32 first = efirst[e], end = efirst[e + 1u];
    const PgEventRec f = s[a.midx[first]];
    const u32 t = rec_table(f);
    const int kind = kind_of((int)t);
    const u32 box = rec_box(f, a.box_size);
    // the support counts and ReportEvent (src/pindel.cpp:2059-2093, Min_Filter_Ratio = 0.5) with its short arithmetic
    u32 n_plus = 0;
    bool lmin = false, lmax = false, rmin = false, rmax = false;
    for (u32 m0 = first; m0 < end; m0 += 64u) {
        const u32 m = m0 + lane;
        bool p = false, c0 = false, c1 = false, c2 = false, c3 = false;
        if (m < end) {
            const PgEventRec r = s[a.midx[m]];
            p = rec_plus(r);
            const int32_t RL = rec_read_len(r), bp = rec_bp(r), nts = (int32_t)rec_nt(r);
            const int16_t rl = (int16_t)(RL - nts);
            const int16_t mn = (int16_t)((int16_t)((rl * 0.5) + 0.5) - 1);
            const int16_t mx = (int16_t)((int16_t)(rl * (1 - 0.5) - 0.5) - 1);
            c0 = bp <= mn;
            c1 = RL - bp - nts <= mn;
            c2 = bp >= mx;
            c3 = RL - bp - nts >= mx;
        }
        n_plus += (u32)__popcll(__ballot(p));
        lmin |= __ballot(c0) != 0ull;
        rmin |= __ballot(c1) != 0ull;
        lmax |= __ballot(c2) != 0ull;
        rmax |= __ballot(c3) != 0ull;
    }
    // GoodIndels[0]: the first unique read of the event's box
    u32 box_head = first;
    for (;;) {
        const bool same = box_head > lane && rec_table(s[a.midx[box_head - 1u - lane]]) == t &&
                          rec_box(s[a.midx[box_head - 1u - lane]], a.box_size) == box;
        const uint64_t mask = __ballot(same);
        if (~mask) {
            box_head -= (u32)__builtin_ctzll(~mask);
            break;
        }
        box_head -= 64u;
    }
    // the left-aligned range
    u32 rs = f.w[0], re = f.w[1];
    const int32_t chr = a.win.chr_id;
    DevRefCode rc;
    rc.lo = ref.lo;
    rc.hi = ref.hi;
    rc.nn = ref.nn;
    rc.word0 = (int64_t)ref.chr_word_off[chr];
    const u32 chr_size = ref.chr_size[chr];
    rc.size = (int64_t)chr_size;
    const PgVaWaveWalk walk = { lane };
    if (!(chr_size < rs || chr_size < re)) {
        if (kind == 1) {
            // NT_str of the first member as 7k rebuilds it: the read's substring behind the pair's own BP, rotated left by nt_rot
            const u32 read = f.w[6];
            const pg_event_read er = a.reads[read];
            const pg_variant_cand c = a.cands[((size_t)read * 2u + 1u) * PG_VARIANT_CANDS + er.slot];
            const PgOutRec o = a.out[read];
            const uint64_t s0 = a.seq_off[read];
            int32_t lead;
            const int32_t RL = post_state_len(a.seq + s0, (int32_t)(a.seq_off[read + 1u] - s0), o.rc_flag, &lead);
            const bool plus = rec_plus(f);
            const ReadCode tcode = { a.seq + s0, lead, RL, plus != (o.rc_flag == 1) };
            int32_t len0 = 0;
            if ((unsigned long long)o.close_off + o.close_cnt <= a.pool_runs && (unsigned long long)o.far_off + o.far_cnt <= a.pool_runs)
                len0 = plus ? point_at(a.pool + o.close_off, o.close_cnt, c.close_idx).len : point_at(a.pool + o.far_off, o.far_cnt, c.far_idx).len;
            const int32_t ins_at = (int32_t)(int16_t)(len0 - 1) + 1;
            u32 len = 0;
            if (ins_at >= 0 && ins_at <= RL && (int64_t)c.indel_size > 0)
                len = (int64_t)c.indel_size < (int64_t)(RL - ins_at) ? c.indel_size : (u32)(RL - ins_at);
            if (len) {
                u32 rot = 0;
                if (len > 1u) {
                    const int64_t q = (int64_t)c.nt_rot % (int64_t)len;
                    rot = (u32)(q < 0 ? q + (int64_t)len : q);
                }
                const auto ins = [&](u32 j) { return tcode(ins_at + (int32_t)((j + rot) % len)); };
                (void)pg_va_real_start_insertion(walk, rc, ins, len, a.spacer, rs, re);
            }
        } else {
            pg_va_real_start_deletion(walk, rc, a.spacer, rs, re);
        }
    }
    if (lane == 0u) {
        const u32 n_reads = end - first;
        u32 flags = 0;
        if (n_reads >= a.win.min_support) flags |= PG_EV_SUPPORT;
        if (kind == 0 || (kind == 1 ? rs < re : !(re < rs || rs == 0u))) flags |= PG_EV_RANGE;
        if (kind == 1 || f.w[2] < a.win.balance_cutoff || (lmin && lmax && rmin && rmax)) flags |= PG_EV_BALANCE;
        if (flags == (PG_EV_SUPPORT | PG_EV_RANGE | PG_EV_BALANCE)) flags |= PG_EV_REPORT;
        pg_event ev;
        ev.bp_left = f.w[0];
        ev.bp_right = f.w[1];
        ev.indel_size = f.w[2];
        ev.first = first - a.info->member_start[t];
        ev.n_reads = n_reads;
        ev.n_plus = n_plus;
        ev.real_start = rs;
        ev.real_end = re;
        ev.box_head = box_head - a.info->member_start[t];
        ev.nt_size = (uint16_t)rec_nt(f);
        ev.kind = (uint8_t)kind;
        ev.flags = (uint8_t)flags;
        a.events[e] = ev;
    }
}

// ---- host side of the launches (pg_api_classify.cpp checks the arguments and owns the buffers)
static inline u32 ev_blocks(u32 m) { return (m + PG_EV_BLOCK - 1u) / PG_EV_BLOCK; }

int pg_events_cascade_launch(const PgEventArgs *a, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    PgEventInfo init;
    memset(&init, 0, sizeof init);
    for (int k = 0; k < 5; k++) init.key_and[k] = ~0u;
    if (hipMemcpyAsync(a->info, &init, sizeof init, hipMemcpyHostToDevice, st) != hipSuccess) return -1;
    if (hipStreamSynchronize(st) != hipSuccess) return -1;     // (init lives on this stack frame)
    if (!a->n) return 0;
    const u32 nb = ev_blocks(a->n);
    hipLaunchKernelGGL(pg_events_cascade_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, *a);
    pg_table_rank_scan_launch(a->flag, a->n, a->rank, a->blk, st);
    hipLaunchKernelGGL(pg_events_compact_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int pg_events_sort_pass_launch(const PgEventArgs *a, const PgEventRec *src, PgEventRec *dst, uint32_t n_boxed, int pass, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!n_boxed) return 0;
    const u32 nb = ev_blocks(n_boxed);
    hipLaunchKernelGGL(pg_events_digit_count_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, src, n_boxed, pass, nb, a->digit_cnt);
    pg_table_scan_launch(a->digit_cnt, 256u * nb, st);
    hipLaunchKernelGGL(pg_events_scatter_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, src, dst, n_boxed, pass, nb, (const u32 *)a->digit_cnt);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int pg_events_tables_launch(const PgDevRef *ref, const PgEventArgs *a, const PgEventRec *sorted, uint32_t n_boxed, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!n_boxed) return 0;
    const u32 nb = ev_blocks(n_boxed);
    hipLaunchKernelGGL(pg_events_unique_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, *a, sorted, n_boxed);
    pg_table_rank_scan_launch(a->flag, n_boxed, a->rank, a->blk, st);
    hipLaunchKernelGGL(pg_events_member_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, *a, sorted, n_boxed);
    hipLaunchKernelGGL(pg_events_head_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, *a, sorted, n_boxed);
    pg_table_rank_scan_launch(a->flag, n_boxed, a->rank, a->blk, st);
    hipLaunchKernelGGL(pg_events_first_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, *a, sorted, n_boxed);
    // (at most n_boxed events: a grid over that many waves, the surplus ones leave at once)
    hipLaunchKernelGGL(pg_events_event_kernel, dim3((n_boxed + PG_EV_BLOCK / 64u - 1u) / (PG_EV_BLOCK / 64u)), dim3(PG_EV_BLOCK), 0, st, *ref, *a,
                       sorted, (const u32 *)a->efirst);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
