// pg_sv_events.hip -- the fourth part of the device classifier: the event tables of DI, INV and INV_NT from the
// per-read records the events build left with the batch.  The host statement of the same function is pg_host_sv_events.hpp; the two
// must agree byte for byte.
//   gather   one thread per read: the boxed reads of the three kinds as records (the pair's fields, the carried NT_size, the strand,
//            the post-state's length, LeftMostPos from the last close point), compacted in ASCENDING read index (rank, scan, fill).
//            The records stay there; what the sorts below move are permutations of their places.
//   segments stable counting passes over the bytes of the box, then the table: the places in (table, box) segments, each in arrival
//            order -- the arrangement the reporters' exchange sorts start from.
//   ranks    a second sort of the places by (table, key) and a scan over its heads: the dense rank of a record's key, one u32.
//   order    pg_sv_events_order_kernel, one wave per non-empty box: the strict exchange sort as record-shift passes (pg_sv_order.h),
//            64 positions per step.  The passes stay sequential: the tie order depends on history.
//   tables   the duplicate walk (literal, one thread per read), members, runs (one wave per run: the largest IndelSize and the
//            harmonisation test), the prefix-AND of the runs of a box, and one wave per event.
// Plain HIP, vector stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "pg_device.h"
#include "pg_sv_order.h"
#include "pg_table_prims.h"
#include "pg_variant_align.h"
#include "pg_variant_dev.h"

typedef uint32_t u32;
static_assert(PG_EV_BLOCK == 256u, "one thread per digit value in the counting kernels");
static_assert(sizeof(PgSvEventRec) == 32 && sizeof(pg_event) == 40 && sizeof(pg_event_read) == 8, "layouts of the tables");
static_assert(PG_SVEV_LDS_BOX * 8u % 1280u == 0u, "the LDS of the order kernel in whole granules");

namespace {

__device__ __forceinline__ int table_of(int kind) { return kind == PG_SV_DI ? 0 : kind == PG_SV_INV ? 1 : kind == PG_SV_INV_NT ? 2 : -1; }
__device__ __forceinline__ int kind_of(u32 table) { return table == 0u ? PG_SV_DI : table == 1u ? PG_SV_INV : PG_SV_INV_NT; }

__device__ __forceinline__ u32 rec_table(const PgSvEventRec &r) { return r.w[5] & 0xffu; }
__device__ __forceinline__ bool rec_plus(const PgSvEventRec &r) { return (r.w[5] >> 8) & 1u; }
__device__ __forceinline__ int32_t rec_read_len(const PgSvEventRec &r) { return (int32_t)(int16_t)(r.w[5] >> 16); }
__device__ __forceinline__ u32 rec_nt(const PgSvEventRec &r) { return r.w[3] >> 16; }
__device__ __forceinline__ int32_t rec_bp(const PgSvEventRec &r) { return (int32_t)(int16_t)((r.w[3] & 0xffffu) ^ 0x8000u); }

// word j of the sort key, most significant first
__device__ __forceinline__ u32 key_word(const PgSvEventRec &r, int j)
{
    const u32 t = rec_table(r);
    if (t == 0u) return j == 0 ? r.w[0] : j == 1 ? r.w[1] : j == 2 ? r.w[3] : 0u;
    return j == 0 ? r.w[0] + r.w[1] : j == 1 ? ~r.w[2] : j == 2 ? r.w[0] : j == 3 ? r.w[1] : t == 2u ? r.w[3] : (r.w[3] & 0xffffu);
}
__device__ __forceinline__ bool same_key(const PgSvEventRec &x, const PgSvEventRec &y)
{
    if (rec_table(x) != rec_table(y)) return false;
    for (int j = 0; j < PG_SVEV_KEY_WORDS; j++)
        if (key_word(x, j) != key_word(y, j)) return false;
    return true;
}
__device__ __forceinline__ u32 sort_digit(const PgSvEventRec &r, int pass)
{
    if (pass < PG_SVEV_PASS_TABLE) return (key_word(r, PG_SVEV_KEY_WORDS - 1 - (pass >> 2)) >> ((pass & 3) * 8)) & 0xffu;
    if (pass == PG_SVEV_PASS_TABLE) return rec_table(r);
    return (r.w[7] >> ((pass - PG_SVEV_PASS_BOX) * 8)) & 0xffu;
}

// One member against its run's largest IndelSize (pg_host_sv.cpp:410): the quotient is a float, 0.95 a double
__device__ __forceinline__ bool harmonise_fails(u32 isz, u32 mx, int32_t RL)
{
    const float q = (float)isz / (float)mx;
    return (double)q < 0.95 || mx + 30u > (u32)RL + isz;
}
// BP of a member harmonised by diff (the two guards of pg_host_sv.cpp:418-422)
__device__ __forceinline__ int32_t harmonised_bp(int32_t bp, int32_t diff, bool plus, int32_t RL)
{
    if (plus) return bp > diff ? (int32_t)(int16_t)(bp - diff) : bp;
    return bp + diff < (int32_t)(int16_t)(RL - 1) ? (int32_t)(int16_t)(bp + diff) : bp;
}

}  // namespace

// ---- gather: the boxed reads of the three kinds, by read
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_sv_events_gather_kernel(PgSvEventArgs a)
{
    const u32 i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const pg_event_read er = a.reads[i];
    const int t = table_of(er.kind);
    uint8_t boxed = 0;
    if ((er.flags & PG_EVR_BOXED) && t >= 0 && er.slot < (t == 1 ? PG_VARIANT_CANDS : 1)) {
        const u32 slot0 = t == 0 ? 0u : t == 1 ? 2u + PG_VARIANT_CANDS : 2u + 2u * PG_VARIANT_CANDS;
        const pg_variant_cand c = a.sv_cands[(size_t)i * PG_SV_SLOTS + slot0 + er.slot];
        const bool plus = a.strand[i] == '+';
        const uint64_t s0 = a.seq_off[i];
        const PgOutRec o = a.out[i];
        int32_t lead;
        const int32_t RL = post_state_len(a.seq + s0, (int32_t)(a.seq_off[i + 1] - s0), o.rc_flag, &lead);
        // LeftMostPos (Caller::note_close_mapped): unsigned arithmetic with the close end's short length
        // (a read without a close end is never boxed; its point counts as all zero)
        const u32 close_len = (u32)(int32_t)(int16_t)o.close_max, close_abs = o.close_max ? o.close_last : 0u;
        const u32 left_most = plus ? close_abs + 1u - close_len : close_abs + close_len - (u32)(int32_t)(int16_t)RL;
        PgSvEventRec r;
        r.w[0] = c.bp_left;
        r.w[1] = c.bp_right;
        r.w[2] = c.indel_size;
        r.w[3] = ((u32)er.nt_size << 16) | (((u32)(uint16_t)c.bp) ^ 0x8000u);
        r.w[4] = i;
        r.w[5] = (u32)t | ((u32)plus << 8) | ((u32)(uint16_t)RL << 16);
        r.w[6] = left_most;
        // (boxed reads have 0 <= (int)BPLeft: the division is the host's; a box lies below 2^24)
        r.w[7] = ((u32)((int32_t)c.bp_left / (int32_t)a.box_size) & 0xffffffu) | ((u32)t << 24);
        a.rec_a[i] = r;
        boxed = 1;
    }
    a.flag[i] = boxed;
}

// the boxed reads to rec in ascending read index; the identity permutations; the masks of the segment and key bytes
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_sv_events_compact_kernel(PgSvEventArgs a)
{
    const u32 i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    const u32 nb = a.blk[(a.n + PG_EV_BLOCK - 1u) / PG_EV_BLOCK];
    const bool mine = i < a.n && a.flag[i];
    u32 k_or[PG_SVEV_KEY_WORDS + 1], k_and[PG_SVEV_KEY_WORDS + 1];
    for (int k = 0; k <= PG_SVEV_KEY_WORDS; k++) {
        k_or[k] = 0u;
        k_and[k] = ~0u;
    }
    if (mine) {
        const PgSvEventRec r = a.rec_a[i];
        const u32 at = a.rank[i] + a.blk[blockIdx.x];
        a.rec[at] = r;
        a.perm_a[at] = at;
        a.kperm_a[at] = at;
        for (int k = 0; k < PG_SVEV_KEY_WORDS; k++) k_or[k] = k_and[k] = key_word(r, k);
        k_or[PG_SVEV_KEY_WORDS] = k_and[PG_SVEV_KEY_WORDS] = r.w[7];
    }
    for (int k = 0; k <= PG_SVEV_KEY_WORDS; k++) {
        const u32 o = wave_or(k_or[k]), n = wave_and(k_and[k]);
        if ((threadIdx.x & 63u) == 0u) {
            u32 *d_or = k < PG_SVEV_KEY_WORDS ? &a.info->key_or[k] : &a.info->seg_or;
            u32 *d_and = k < PG_SVEV_KEY_WORDS ? &a.info->key_and[k] : &a.info->seg_and;
            if (o) atomicOr(d_or, o);
            if (n != ~0u) atomicAnd(d_and, n);
        }
    }
    if (i == 0u) a.info->n_boxed = nb;
}

// ---- one counting pass over the places src[0 .. m): cnt[d * n_blk + b] = places of block b whose record has digit d
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_sv_events_digit_count_kernel(const PgSvEventRec *rec, const u32 *src, u32 m, int pass,
                                                                                           u32 n_blk, u32 *cnt)
{
    tab_digit_count(src, m, n_blk, cnt, [rec, pass](const u32 &p) { return sort_digit(rec[p], pass); });
}
// cnt scanned: the slot of a place = cnt[its digit][its block] + the places of its block before it with the same digit
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_sv_events_scatter_kernel(const PgSvEventRec *rec, const u32 *src, u32 *dst, u32 m, int pass,
                                                                                       u32 n_blk, const u32 *cnt)
{
    tab_scatter(src, dst, m, n_blk, cnt, [rec, pass](const u32 &p) { return sort_digit(rec[p], pass); });
}

// ---- ranks: flag[i] = the place kperm[i] opens a class of equal (table, key)
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_sv_events_key_head_kernel(PgSvEventArgs a, const u32 *kperm, u32 m)
{
    const u32 i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (i >= m) return;
    a.flag[i] = (uint8_t)(i == 0u || !same_key(a.rec[kperm[i - 1u]], a.rec[kperm[i]]));
}
// krank[place] = the classes before its own
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_sv_events_key_rank_kernel(PgSvEventArgs a, const u32 *kperm, u32 m)
{
    const u32 i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (i >= m) return;
    a.krank[kperm[i]] = a.rank[i] + a.blk[blockIdx.x] - (a.flag[i] ? 0u : 1u);
}

// ---- segments: flag[i] = the place perm[i] opens a (table, box) segment
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_sv_events_seg_head_kernel(PgSvEventArgs a, const u32 *perm, u32 m)
{
    const u32 i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (i >= m) return;
    a.flag[i] = (uint8_t)(i == 0u || a.rec[perm[i - 1u]].w[7] != a.rec[perm[i]].w[7]);
}
// seg_first[s] = the first slot of segment s (one entry more: m)
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_sv_events_seg_first_kernel(PgSvEventArgs a, u32 m)
{
    const u32 ns = a.blk[(m + PG_EV_BLOCK - 1u) / PG_EV_BLOCK];
    const u32 i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (i == 0u) {
        a.info->n_segs = ns;
        a.seg_first[ns] = m;
    }
    if (i < m && a.flag[i]) a.seg_first[a.rank[i] + a.blk[blockIdx.x]] = i;
}

// ---- order: one wave per segment, the record-shift passes of pg_sv_order.h over rk[0 .. n) with the places ix[0 .. n)
namespace {
template <class P>
__device__ __forceinline__ void order_passes(P rk, P ix, u32 n, u32 lane)
{
    bool have_lo = false;
    u32 lo = 0;
    for (u32 a = 0; a + 1u < n; a++) {
        const u32 front = rk[a];
        // the front equals the minimum the last executed pass found, a lower bound of everything behind it: already minimal
        if (have_lo && front == lo) continue;
        u32 run_min = front, carry_rk = front, carry_ix = ix[a];
        bool any = false;
        for (u32 c0 = a + 1u; c0 < n; c0 += 64u) {
            const u32 d = c0 + lane;
            const bool valid = d < n;
            const u32 v = valid ? rk[d] : PG_SVO_NONE;
            const u32 p = valid ? ix[d] : 0u;
            // the minimum of everything from the front up to the position before: an exclusive prefix-min seeded with the carry
            u32 inc = v;
            for (int s = 1; s < 64; s <<= 1) {
                const u32 o = (u32)__shfl_up((int)inc, s, 64);
                if (lane >= (u32)s) inc = o < inc ? o : inc;
            }
            u32 excl = (u32)__shfl_up((int)inc, 1, 64);
            excl = lane == 0u ? run_min : (excl < run_min ? excl : run_min);
            const bool is_rec = pg_svo_is_record(v, excl, valid);
            const uint64_t records = __ballot(is_rec);
            // each record takes what the record before it held (the prefix-max over record positions is the ballot's highest bit below)
            const int pl = pg_svo_pred_lane(records, lane);
            const u32 pv = (u32)__shfl((int)v, pl < 0 ? 0 : pl, 64), pp = (u32)__shfl((int)p, pl < 0 ? 0 : pl, 64);
            if (is_rec) {
                rk[d] = pl < 0 ? carry_rk : pv;
                ix[d] = pl < 0 ? carry_ix : pp;
            }
            if (records) {
                const int last = pg_svo_last_lane(records);
                carry_rk = (u32)__shfl((int)v, last, 64);
                carry_ix = (u32)__shfl((int)p, last, 64);
                any = true;
            }
            const u32 chunk_min = (u32)__shfl((int)inc, 63, 64);
            run_min = chunk_min < run_min ? chunk_min : run_min;
        }
        if (any && lane == 0u) {
            rk[a] = carry_rk;
            ix[a] = carry_ix;
        }
        lo = run_min;
        have_lo = true;
        __syncthreads();                                  // (one wave: the next pass reads what other lanes wrote)
    }
}
}  // namespace

extern "C" __global__ void __launch_bounds__(64) pg_sv_events_order_kernel(PgSvEventArgs a, u32 *perm)
{
    __shared__ u32 l_rk[PG_SVEV_LDS_BOX], l_ix[PG_SVEV_LDS_BOX];
    const u32 s = blockIdx.x, lane = threadIdx.x;
    if (s >= a.info->n_segs) return;                       // (whole workgroups)
    const u32 s0 = a.seg_first[s], n = a.seg_first[s + 1u] - s0;
    if (n < 2u) return;
    if (n <= PG_SVEV_LDS_BOX) {
        for (u32 j = lane; j < n; j += 64u) {
            const u32 p = perm[s0 + j];
            l_ix[j] = p;
            l_rk[j] = a.krank[p];
        }
        __syncthreads();
        order_passes(l_rk, l_ix, n, lane);
        for (u32 j = lane; j < n; j += 64u) perm[s0 + j] = l_ix[j];
    } else {
        u32 *rk = a.ws_rank + s0, *ix = perm + s0;
        for (u32 j = lane; j < n; j += 64u) rk[j] = a.krank[ix[j]];
        __syncthreads();
        order_passes(rk, ix, n, lane);
    }
}

// ---- duplicates: dupf[i] = an earlier read of the sorted box, unique or not, starts or ends where this one does, on the same
// strand (DI: with the same length).  The walk is the literal one.  flag[i] = the read is a member: DI lists the unique reads only
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_sv_events_unique_kernel(PgSvEventArgs a, const u32 *perm, u32 m)
{
    const u32 i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    bool member = false;
    u32 t = PG_SV_EVENT_TABLES;
    if (i < m) {
        const PgSvEventRec r = a.rec[perm[i]];
        t = rec_table(r);
        const int32_t lm = (int32_t)r.w[6], RL = rec_read_len(r);
        bool dup = false;
        for (u32 j = i; j-- > 0u && !dup;) {
            const PgSvEventRec q = a.rec[perm[j]];
            if (q.w[7] != r.w[7]) break;
            const int32_t qlm = (int32_t)q.w[6], qRL = rec_read_len(q);
            dup = (t != 0u || qRL == RL) && (qlm == lm || qlm + qRL == lm + RL) && rec_plus(q) == rec_plus(r);
        }
        a.dupf[i] = dup ? 1 : 0;
        member = t != 0u || !dup;
        a.flag[i] = member ? 1 : 0;
    }
    for (u32 k = 0; k < PG_SV_EVENT_TABLES; k++) {
        const u32 c = (u32)__popcll(__ballot(member && t == k));
        if ((threadIdx.x & 63u) == 0u && c) atomicAdd(&a.info->n_mem[k], c);
    }
}

// members[at] = the read (with its duplicate bit for the inversions), midx[at] = its place
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_sv_events_member_kernel(PgSvEventArgs a, const u32 *perm, u32 m)
{
    const u32 i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (i >= m || !a.flag[i]) return;
    const u32 at = a.rank[i] + a.blk[blockIdx.x], p = perm[i];
    a.members[at] = a.rec[p].w[4] | (a.dupf[i] ? PG_SVEV_MEMBER_DUP : 0u);
    a.midx[at] = p;
}

namespace {
// DI: (BPLeft, IndelSize, (short)NT_size); the inversions: BPLeft + BPRight.  Never across a box.
__device__ __forceinline__ bool same_run(const PgSvEventRec &x, const PgSvEventRec &y)
{
    if (x.w[7] != y.w[7]) return false;
    if (rec_table(x) == 0u) return x.w[0] == y.w[0] && x.w[2] == y.w[2] && rec_nt(x) == rec_nt(y);
    return x.w[0] + x.w[1] == y.w[0] + y.w[1];
}
}  // namespace

// flag[m] = member m opens a run (the member flags have been consumed by then; their total moves to info)
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_sv_events_run_head_kernel(PgSvEventArgs a, u32 n_boxed)
{
    const u32 nm = a.blk[(n_boxed + PG_EV_BLOCK - 1u) / PG_EV_BLOCK];
    const u32 m = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (m == 0u) a.info->n_members = nm;
    if (m >= n_boxed) return;
    a.flag[m] = m < nm ? (uint8_t)(m == 0u || !same_run(a.rec[a.midx[m - 1u]], a.rec[a.midx[m]])) : (uint8_t)0;
}
// rfirst[r] = the first member of run r (one entry more: the number of members)
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_sv_events_run_first_kernel(PgSvEventArgs a, u32 n_boxed)
{
    const u32 nm = a.info->n_members;
    const u32 nr = a.blk[(n_boxed + PG_EV_BLOCK - 1u) / PG_EV_BLOCK];
    const u32 m = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (m == 0u) {
        a.info->n_runs = nr;
        a.rfirst[nr] = nm;
    }
    if (m < nm && a.flag[m]) a.rfirst[a.rank[m] + a.blk[blockIdx.x]] = m;
}

// one wave per run of the inversions: rmx = the largest IndelSize, rfail = a member fails the test against it
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_sv_events_run_kernel(PgSvEventArgs a)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 r = blockIdx.x * (PG_EV_BLOCK / 64u) + (threadIdx.x >> 6);
    if (r >= a.info->n_runs) return;                       // (whole waves)
    const u32 first = a.rfirst[r], end = a.rfirst[r + 1u];
    u32 mx = 0;
    bool fail = false;
    if (rec_table(a.rec[a.midx[first]]) != 0u) {
        for (u32 m = first + lane; m < end; m += 64u) {
            const u32 isz = a.rec[a.midx[m]].w[2];
            mx = isz > mx ? isz : mx;
        }
        mx = wave_max(mx);
        for (u32 m = first + lane; m < end; m += 64u) {
            const PgSvEventRec q = a.rec[a.midx[m]];
            fail = fail || harmonise_fails(q.w[2], mx, rec_read_len(q));
        }
        fail = __ballot(fail) != 0ull;
    }
    if (lane == 0u) {
        a.rmx[r] = mx;
        a.rfail[r] = fail ? 1 : 0;
    }
}

// flag[r] = run r yields an event: DI always; an inversion run if neither it nor an earlier run of its box failed (`whether` is
// never re-armed inside a box: a prefix-AND over the runs of a box, walked back literally)
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_sv_events_alive_kernel(PgSvEventArgs a, u32 n_boxed)
{
    const u32 nr = a.info->n_runs;
    const u32 r = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    bool alive = false, dropped = false;
    u32 t = PG_SV_EVENT_TABLES;
    if (r < nr) {
        const PgSvEventRec f = a.rec[a.midx[a.rfirst[r]]];
        t = rec_table(f);
        alive = true;
        if (t != 0u)
            for (u32 j = r + 1u; j-- > 0u && alive;) {
                if (a.rec[a.midx[a.rfirst[j]]].w[7] != f.w[7]) break;
                alive = !a.rfail[j];
            }
        dropped = !alive;
    }
    if (r < n_boxed) a.flag[r] = alive ? 1 : 0;
    for (u32 k = 0; k < PG_SV_EVENT_TABLES; k++) {
        const u32 c = (u32)__popcll(__ballot(alive && t == k)), d = (u32)__popcll(__ballot(dropped && t == k));
        if ((threadIdx.x & 63u) == 0u) {
            if (c) atomicAdd(&a.info->n_ev[k], c);
            if (d) atomicAdd(&a.info->dropped[k], d);
        }
    }
}

// ---- one wave per run that yields an event
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_sv_events_event_kernel(PgDevRef ref, PgSvEventArgs a)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 r = blockIdx.x * (PG_EV_BLOCK / 64u) + (threadIdx.x >> 6);
    if (r >= a.info->n_runs || !a.flag[r]) return;         // (whole waves)
    const u32 e = a.rank[r] + a.blk[r / PG_EV_BLOCK];
    const u32 nm = a.info->n_members;
    const u32 first = a.rfirst[r], end = a.rfirst[r + 1u];
    const PgSvEventRec f = a.rec[a.midx[first]];
    const u32 t = rec_table(f);
    const u32 mx = t != 0u ? a.rmx[r] : 0u;
    u32 member_start = 0;
    for (u32 k = 0; k < t; k++) member_start += a.info->n_mem[k];
    // the support counts and ReportEvent (src/pindel.cpp:2059-2093, Min_Filter_Ratio = 0.5) with its short arithmetic, over the
    // members as the reporter has them by then: the inversions' harmonised
    u32 n_plus = 0;
    bool lmin = false, lmax = false, rmin = false, rmax = false;
    for (u32 m0 = first; m0 < end; m0 += 64u) {
        const u32 m = m0 + lane;
        bool p = false, c0 = false, c1 = false, c2 = false, c3 = false;
        if (m < end) {
            const PgSvEventRec q = a.rec[a.midx[m]];
            p = rec_plus(q);
            const int32_t RL = rec_read_len(q), nts = (int32_t)rec_nt(q);
            int32_t bp = rec_bp(q);
            if (t != 0u) bp = harmonised_bp(bp, (int32_t)(int16_t)((mx - q.w[2]) / 2u), p, RL);
            const int16_t rl = (int16_t)(RL - nts);
            const int16_t mn = (int16_t)((int16_t)((rl * 0.5) + 0.5) - 1);
            const int16_t mxb = (int16_t)((int16_t)(rl * (1 - 0.5) - 0.5) - 1);
            c0 = bp <= mn;
            c1 = RL - bp - nts <= mn;
            c2 = bp >= mxb;
            c3 = RL - bp - nts >= mxb;
        }
        n_plus += (u32)__popcll(__ballot(p));
        lmin |= __ballot(c0) != 0ull;
        rmin |= __ballot(c1) != 0ull;
        lmax |= __ballot(c2) != 0ull;
        rmax |= __ballot(c3) != 0ull;
    }
    // the first member of the event's box
    u32 box_head = first;
    for (;;) {
        const bool same = box_head > lane && a.rec[a.midx[box_head - 1u - lane]].w[7] == f.w[7];
        const uint64_t mask = __ballot(same);
        if (~mask) {
            box_head -= (u32)__builtin_ctzll(~mask);
            break;
        }
        box_head -= 64u;
    }
    u32 bl = f.w[0], br = f.w[1], isz = f.w[2], rs, re;
    bool short_inv = false;
    if (t != 0u) {
        const u32 diff = (u32)(int32_t)(int16_t)((mx - f.w[2]) / 2u);
        bl = f.w[0] - diff;
        br = f.w[1] + diff;
        isz = mx;
        // every run but the last of its box carries the harmonised range, the last one the first member's own
        const bool last_of_box = end >= nm || a.rec[a.midx[end]].w[7] != f.w[7];
        rs = last_of_box ? f.w[0] : bl;
        re = last_of_box ? f.w[1] : br;
    } else {
        rs = bl;
        re = br;
        // is_inversion (pg_host.cpp:700): IndelSize == NT_size and the reverse complement of the NT_size reference bases at
        // spacer + 1 + BPLeft is NT_str -- the read's substring behind BP, cut as 7l's host side cuts it
        const u32 nt = rec_nt(f);
        if (f.w[2] == nt) {
            const int32_t chr = a.win.chr_id;
            DevRefCode rc;
            rc.lo = ref.lo;
            rc.hi = ref.hi;
            rc.nn = ref.nn;
            rc.word0 = (int64_t)ref.chr_word_off[chr];
            rc.size = (int64_t)ref.chr_size[chr];
            const u32 read = f.w[4];
            const PgOutRec o = a.out[read];
            const uint64_t s0 = a.seq_off[read];
            int32_t lead;
            const int32_t RL = post_state_len(a.seq + s0, (int32_t)(a.seq_off[read + 1u] - s0), o.rc_flag, &lead);
            const bool plus = rec_plus(f);
            const ReadCode tcode = { a.seq + s0, lead, RL, plus != (o.rc_flag == 1) };
            const int64_t pos = (int64_t)a.spacer + 1 + (int64_t)f.w[0];
            const int64_t at = (int64_t)rec_bp(f) + 1;
            const int64_t len_ref = pos <= rc.size ? (rc.size - pos < (int64_t)nt ? rc.size - pos : (int64_t)nt) : 0;
            const int64_t len_str = at >= 0 && at <= RL ? ((int64_t)RL - at < (int64_t)nt ? (int64_t)RL - at : (int64_t)nt) : 0;
            short_inv = len_ref == len_str;
            for (int64_t j0 = 0; j0 < len_str && short_inv; j0 += 64) {
                const int64_t j = j0 + lane;
                bool differ = false;
                if (j < len_str) {
                    const uint32_t g = rc(pos + len_ref - 1 - j);
                    differ = tcode((int32_t)(at + j)) != (g < 4u ? 3u - g : g);
                }
                short_inv = __ballot(differ) == 0ull;
            }
        }
    }
    if (lane == 0u) {
        const u32 n_reads = end - first;
        u32 flags = 0;
        if (n_reads >= a.win.min_support) flags |= PG_EV_SUPPORT;
        if (t != 0u && !(re < rs || rs == 0u)) flags |= PG_EV_RANGE;
        if (isz < a.win.balance_cutoff || (lmin && lmax && rmin && rmax)) flags |= PG_EV_BALANCE;
        if (short_inv) flags |= PG_EV_SHORT_INV;
        const u32 need = t != 0u ? (PG_EV_SUPPORT | PG_EV_RANGE | PG_EV_BALANCE) : (PG_EV_SUPPORT | PG_EV_BALANCE);
        if ((flags & need) == need) flags |= PG_EV_REPORT;
        pg_event ev;
        ev.bp_left = bl;
        ev.bp_right = br;
        ev.indel_size = isz;
        ev.first = first - member_start;
        ev.n_reads = n_reads;
        ev.n_plus = n_plus;
        ev.real_start = rs;
        ev.real_end = re;
        ev.box_head = box_head - member_start;
        ev.nt_size = (uint16_t)rec_nt(f);
        ev.kind = (uint8_t)kind_of(t);
        ev.flags = (uint8_t)flags;
        a.events[e] = ev;
    }
}

// ---- host side of the launches (pg_api_classify.cpp checks the arguments and owns the buffers)
static inline u32 ev_blocks(u32 m) { return (m + PG_EV_BLOCK - 1u) / PG_EV_BLOCK; }

int pg_sv_events_gather_launch(const PgSvEventArgs *a, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    PgSvEventInfo init;
    memset(&init, 0, sizeof init);
    init.seg_and = ~0u;
    for (int k = 0; k < PG_SVEV_KEY_WORDS; k++) init.key_and[k] = ~0u;
    if (hipMemcpyAsync(a->info, &init, sizeof init, hipMemcpyHostToDevice, st) != hipSuccess) return -1;
    if (hipStreamSynchronize(st) != hipSuccess) return -1;     // (init lives on this stack frame)
    if (!a->n) return 0;
    const u32 nb = ev_blocks(a->n);
    hipLaunchKernelGGL(pg_sv_events_gather_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, *a);
    pg_table_rank_scan_launch(a->flag, a->n, a->rank, a->blk, st);
    hipLaunchKernelGGL(pg_sv_events_compact_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int pg_sv_events_sort_pass_launch(const PgSvEventArgs *a, const uint32_t *src, uint32_t *dst, uint32_t n_boxed, int pass, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!n_boxed) return 0;
    const u32 nb = ev_blocks(n_boxed);
    hipLaunchKernelGGL(pg_sv_events_digit_count_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, (const PgSvEventRec *)a->rec, src, n_boxed, pass, nb,
                       a->digit_cnt);
    pg_table_scan_launch(a->digit_cnt, 256u * nb, st);
    hipLaunchKernelGGL(pg_sv_events_scatter_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, (const PgSvEventRec *)a->rec, src, dst, n_boxed, pass, nb,
                       (const u32 *)a->digit_cnt);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int pg_sv_events_tables_launch(const PgDevRef *ref, const PgSvEventArgs *a, uint32_t *perm, const uint32_t *kperm, uint32_t n_boxed, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!n_boxed) return 0;
    const u32 nb = ev_blocks(n_boxed);
    const dim3 grid(nb), block(PG_EV_BLOCK);
    const dim3 waves((n_boxed + PG_EV_BLOCK / 64u - 1u) / (PG_EV_BLOCK / 64u));   // (at most n_boxed runs: the surplus waves leave at once)
    hipLaunchKernelGGL(pg_sv_events_key_head_kernel, grid, block, 0, st, *a, kperm, n_boxed);
    pg_table_rank_scan_launch(a->flag, n_boxed, a->rank, a->blk, st);
    hipLaunchKernelGGL(pg_sv_events_key_rank_kernel, grid, block, 0, st, *a, kperm, n_boxed);
    hipLaunchKernelGGL(pg_sv_events_seg_head_kernel, grid, block, 0, st, *a, (const u32 *)perm, n_boxed);
    pg_table_rank_scan_launch(a->flag, n_boxed, a->rank, a->blk, st);
    hipLaunchKernelGGL(pg_sv_events_seg_first_kernel, grid, block, 0, st, *a, n_boxed);
    hipLaunchKernelGGL(pg_sv_events_order_kernel, dim3(n_boxed), dim3(64), 0, st, *a, perm);
    hipLaunchKernelGGL(pg_sv_events_unique_kernel, grid, block, 0, st, *a, (const u32 *)perm, n_boxed);
    pg_table_rank_scan_launch(a->flag, n_boxed, a->rank, a->blk, st);
    hipLaunchKernelGGL(pg_sv_events_member_kernel, grid, block, 0, st, *a, (const u32 *)perm, n_boxed);
    hipLaunchKernelGGL(pg_sv_events_run_head_kernel, grid, block, 0, st, *a, n_boxed);
    pg_table_rank_scan_launch(a->flag, n_boxed, a->rank, a->blk, st);
    hipLaunchKernelGGL(pg_sv_events_run_first_kernel, grid, block, 0, st, *a, n_boxed);
    hipLaunchKernelGGL(pg_sv_events_run_kernel, waves, block, 0, st, *a);
    hipLaunchKernelGGL(pg_sv_events_alive_kernel, grid, block, 0, st, *a, n_boxed);
    pg_table_rank_scan_launch(a->flag, n_boxed, a->rank, a->blk, st);
    hipLaunchKernelGGL(pg_sv_events_event_kernel, waves, block, 0, st, *ref, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
