// pg_dd_tables.hip -- the eighth part of the device classifier: the dispersed-duplication breakpoint tables and their
// consensus.  searchMEIBreakpoints groups the split reads around a discordant cluster by the position of their last close point,
// votes a consensus over the unmapped part of each group and asks whether it lies near the breakpoint; here the groups become
// tables, the vote runs one wave per group and the containment kernel (pg_dd.hip) reads the consensus where it lies, so that _DD is
// written without a point leaving or a consensus entering the GPU.
// The host statement of the same function is dd_tables_from_close (pg_dd.cpp); the two must agree byte for byte.
//   stage A  pg_ddt_flag_kernel: one thread per read.  Its segment by binary search over seg_first, the DD test from the output
//            record and the anchor strand; the DD reads are compacted in ASCENDING read index (rank, scan, fill), with the masks of
//            their key bytes.
//   stage B  LSD counting passes over (seg, pos), skipping the bytes that are constant over the batch.  Every pass is stable, so
//            equal keys keep the ascending read index.
//   stage C  head flags, scan, firsts; a key's count is the distance of two firsts, and a second compaction keeps the members and
//            heads of the keys with enough support: members, candidates (without the consensus fields) and one aux record per member.
//   stage D  pg_ddt_consensus_kernel: one wave per candidate, lanes striding over its members.  Per column each lane yields its
//            member's byte and adds one to that byte's counter in the wave's LDS table; the winner and the 4/5 test are wave-uniform
//            and all of it is integer, so the result does not depend on the order of the additions.  The accepted bytes go to the
//            candidate's slot; a scan over the lengths gives cons_off and pg_ddt_pool_kernel packs the pool.
//   stage E  the window per tested candidate (written with the candidate in stage D), pg_dd_launch over the packed pool, the flags.
// The scan stages and the bodies of the counting passes are the shared ones of pg_table_prims.h, here over a 16-byte record.
// Plain HIP, vector stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "pg_device.h"
#include "pg_table_prims.h"
#include "pg_variant_dev.h"

typedef uint32_t u32;
static_assert(PG_EV_BLOCK == 256u, "one thread per digit value in the counting kernels");
static_assert(sizeof(PgDdRec) == 16 && sizeof(PgDdAux) == 16 && sizeof(pg_dd_member) == 8 && sizeof(pg_dd_cand) == 40, "layouts of the tables");

namespace {

// key byte `pass`, least significant first: pos (w[1]), then seg (w[0])
__device__ __forceinline__ u32 dd_key_digit(const PgDdRec &r, int pass)
{
    const u32 w = pass < 4 ? r.w[1] : r.w[0];
    return (w >> ((pass & 3) * 8)) & 0xffu;
}

// Convert2RC4N (src/pindel.cpp:966-970): unset entries are 0
__device__ __forceinline__ uint8_t dd_rc4n(uint8_t c)
{
    switch (c) {
    case 'A': return 'T';
    case 'C': return 'G';
    case 'G': return 'C';
    case 'T': return 'A';
    case 'N': return 'N';
    default: return 0;
    }
}

// byte p of the read as rc_flag left it: raw = the first byte of the post-state among the bytes as uploaded
__device__ __forceinline__ uint8_t dd_post_byte(const uint8_t *raw, u32 len, u32 rc_flag, u32 p)
{
    if (!rc_flag) return raw[p];
    if (rc_flag == 1u) return dd_rc4n(raw[len - 1u - p]);
    return dd_rc4n(dd_rc4n(raw[p]));                          // two reverse complements: a byte outside ACGTN is 0 by now
}

// the key of member m of the sorted records (its head flags ranked): the heads up to and including m, less one
__device__ __forceinline__ u32 dd_key_of(const PgDdArgs &a, u32 m) { return a.rank[m] + a.blk[m / PG_EV_BLOCK] + (u32)a.flag[m] - 1u; }

}  // namespace

// ---- stage A
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_ddt_flag_kernel(PgDdArgs a)
{
    const u32 i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    // the first k in [0, n_seg] with seg_first[k] > i; the read's segment is k - 1 (a segment of no reads is stepped over: its
    // first equals its successor's)
    u32 lo = 0u, hi = a.n_seg + 1u;
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (a.seg_first[mid] > i) hi = mid;
        else lo = mid + 1u;
    }
    uint8_t is_dd = 0;
    if (lo >= 1u && lo <= a.n_seg) {
        const u32 s = lo - 1u;
        const PgOutRec o = a.out[i];
        if (o.close_max != 0 && a.strand[i] == a.seg_strand[s]) {
            PgDdRec r;
            r.w[0] = s;
            r.w[1] = o.close_last;
            r.w[2] = i;
            r.w[3] = (u32)o.close_max | (u32)o.rc_flag << 16;
            a.rec_a[i] = r;
            is_dd = 1;
        }
    }
    a.flag[i] = is_dd;
}

// the DD reads to rec_b in ascending read index; the masks of their key bytes
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_ddt_compact_kernel(PgDdArgs a)
{
    const u32 i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    const bool mine = i < a.n && a.flag[i];
    u32 k_or[PG_DD_KEY_WORDS], k_and[PG_DD_KEY_WORDS];
#pragma unroll
    for (int k = 0; k < PG_DD_KEY_WORDS; k++) {
        k_or[k] = 0u;
        k_and[k] = ~0u;
    }
    if (mine) {
        const PgDdRec r = a.rec_a[i];
        a.rec_b[a.rank[i] + a.blk[blockIdx.x]] = r;
#pragma unroll
        for (int k = 0; k < PG_DD_KEY_WORDS; k++) k_or[k] = k_and[k] = r.w[k];
    }
#pragma unroll
    for (int k = 0; k < PG_DD_KEY_WORDS; k++) {
        const u32 o = wave_or(k_or[k]), n = wave_and(k_and[k]);
        if ((threadIdx.x & 63u) == 0u) {
            if (o) atomicOr(&a.info->key_or[k], o);
            if (n != ~0u) atomicAnd(&a.info->key_and[k], n);
        }
    }
    if (i == 0u) a.info->n_dd = a.blk[(a.n + PG_EV_BLOCK - 1u) / PG_EV_BLOCK];
}

// ---- stage B: one counting pass.  cnt[d * n_blk + b] = records of block b with digit d
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_ddt_digit_count_kernel(const PgDdRec *src, u32 m, int pass, u32 n_blk, u32 *cnt)
{
    tab_digit_count(src, m, n_blk, cnt, [pass](const PgDdRec &r) { return dd_key_digit(r, pass); });
}
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_ddt_scatter_kernel(const PgDdRec *src, PgDdRec *dst, u32 m, int pass, u32 n_blk,
                                                                                 const u32 *cnt)
{
    tab_scatter(src, dst, m, n_blk, cnt, [pass](const PgDdRec &r) { return dd_key_digit(r, pass); });
}

// ---- stage C: flag[m] = record m opens a key
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_ddt_head_kernel(PgDdArgs a, const PgDdRec *s, u32 n_dd)
{
    const u32 m = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (m >= n_dd) return;
    bool head = m == 0u;
    if (!head) {
        const PgDdRec r = s[m], q = s[m - 1u];
        head = q.w[0] != r.w[0] || q.w[1] != r.w[1];
    }
    a.flag[m] = (uint8_t)head;
}
// cfirst[k] = the first record of key k (one entry more: the number of records)
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_ddt_first_kernel(PgDdArgs a, u32 n_dd)
{
    const u32 n_keys = a.blk[(n_dd + PG_EV_BLOCK - 1u) / PG_EV_BLOCK];
    const u32 m = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (m >= n_dd) return;
    if (a.flag[m]) a.cfirst[a.rank[m] + a.blk[blockIdx.x]] = m;
    if (m == n_dd - 1u) {
        a.cfirst[n_keys] = n_dd;
        a.info->n_keys = n_keys;
    }
}
// keep[m] = record m belongs to a key with enough support; keep_head[m] = ... and opens it
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_ddt_keep_kernel(PgDdArgs a, u32 n_dd)
{
    const u32 m = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (m >= n_dd) return;
    const u32 k = dd_key_of(a, m);
    const u32 count = a.cfirst[k + 1u] - a.cfirst[k];
    const bool keep = a.min_bp_support <= 1 || count >= (u32)a.min_bp_support;
    a.keep[m] = (uint8_t)keep;
    a.keep_head[m] = (uint8_t)(keep && a.flag[m]);
}
// the totals of the two rankings (after their scans)
extern "C" __global__ void pg_ddt_counts_kernel(PgDdArgs a, u32 n_dd)
{
    const u32 nb = (n_dd + PG_EV_BLOCK - 1u) / PG_EV_BLOCK;
    a.info->n_mem = a.blk_m[nb];
    a.info->n_cands = a.blk_c[nb];
}
// members, candidates without the consensus fields, aux records
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_ddt_member_kernel(PgDdArgs a, const PgDdRec *s, u32 n_dd)
{
    const u32 m = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (m >= n_dd || !a.keep[m]) return;
    const PgDdRec r = s[m];
    const u32 dst = a.rank_m[m] + a.blk_m[blockIdx.x];
    const u32 close_len = r.w[3] & 0xffffu, rc_flag = (r.w[3] >> 16) & 0xffu;
    pg_dd_member mem;
    mem.read = r.w[2];
    mem.close_len = (uint16_t)close_len;
    mem.rc_flag = (uint8_t)rc_flag;
    mem.reserved = 0;
    a.members[dst] = mem;
    const uint64_t s0 = a.seq_off[r.w[2]];
    int32_t lead;
    const int32_t len = post_state_len(a.seq + s0, (int32_t)(a.seq_off[r.w[2] + 1u] - s0), rc_flag, &lead);
    PgDdAux x;
    x.base = s0 + (uint64_t)lead;
    x.len = (u32)max(len, 0);
    const u32 u = x.len > close_len ? x.len - close_len : 0u;
    x.u_rc = u | (rc_flag >= 2u ? 2u : rc_flag) << 16;
    a.aux[dst] = x;
    if (a.keep_head[m]) {
        const u32 k = dd_key_of(a, m);
        pg_dd_cand c;
        c.seg = r.w[0];
        c.pos = r.w[1];
        c.first = dst;
        c.n_reads = a.cfirst[k + 1u] - a.cfirst[k];
        c.cons_off = c.cons_len = c.flags = c.win_len = 0u;
        c.win_start = 0ull;
        a.cands[a.rank_c[m] + a.blk_c[blockIdx.x]] = c;
    }
}

// ---- stage D: one wave per candidate
extern "C" __global__ void __launch_bounds__(PG_DD_WAVES * 64u) pg_ddt_consensus_kernel(PgDdArgs a, u32 n_cands)
{
    __shared__ u32 s_cnt[PG_DD_WAVES][256];
    const u32 lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    u32 *cnt = s_cnt[w];
    for (u32 k = lane; k < 256u; k += 64u) cnt[k] = 0u;
    const u32 e = blockIdx.x * PG_DD_WAVES + w;
    if (e >= n_cands) return;                                  // (the whole wave: no barrier below spans the workgroup)
    const u32 first = a.cands[e].first, n_reads = a.cands[e].n_reads, pos = a.cands[e].pos;
    const bool plus = a.seg_strand[a.cands[e].seg] == '+';
    const PgDdAux *aux = a.aux + first;
    u32 max_u = 0u;
    for (u32 j = lane; j < n_reads; j += 64u) max_u = max(max_u, aux[j].u_rc & 0xffffu);
    max_u = min(wave_max(max_u), a.slot);                      // (u <= the read's length <= slot: the slot is never the smaller)
    uint8_t *slot = a.slots + (uint64_t)e * a.slot;
    u32 n_cols = 0u;
    for (u32 i = 0u; i < max_u; i++) {
        u32 n = 0u;
        for (u32 j0 = 0u; j0 < n_reads; j0 += 64u) {
            const u32 j = j0 + lane;
            bool active = false;
            if (j < n_reads) {
                const PgDdAux x = aux[j];
                const u32 u = x.u_rc & 0xffffu;
                if (u > i) {
                    active = true;
                    const uint8_t c = dd_post_byte(a.seq + x.base, x.len, x.u_rc >> 16, u - 1u - i);
                    atomicAdd(&cnt[plus ? dd_rc4n(c) : c], 1u);
                }
            }
            n += (u32)__popcll(__ballot(active));
        }
        // (the additions above and the reads below are LDS operations of one wave, issued and completed in program order)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // the largest count; on a tie the smallest byte as signed char: 0x80 .. 0xff before 0x00 .. 0x7f.  (The contract words the
        // tie, so it is resolved as the reference resolves it, but no output depends on it: tied winners hold at most n / 2 votes
        // each, which never passes the 4 / 5 test below, so a tied column ends the consensus and its winner is not stored.  The '?'
        // of the reference's empty column is likewise out of reach: every column visited has a member, n >= 1.)
        u32 best = 0u, best_rank = 0u;                         // rank 256 - (byte ^ 0x80): larger = earlier in std::map<char,int>
        for (u32 k = lane; k < 256u; k += 64u) {
            const u32 c = cnt[k];
            cnt[k] = 0u;
            const u32 rank = 256u - (k ^ 0x80u);
            if (c > best || (c == best && c && rank > best_rank)) {
                best = c;
                best_rank = rank;
            }
        }
        const u32 mx = wave_max(best);
        const u32 win_rank = wave_max(best == mx && mx ? best_rank : 0u);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // max_count >= 0.8f * read_count of the reference, in integers (they agree for every n up to 200 000 at the threshold and
        // one either side of it)
        if (5ull * mx < 4ull * n) break;
        if (lane == 0u) slot[i] = mx ? (uint8_t)((256u - win_rank) ^ 0x80u) : (uint8_t)'?';
        n_cols++;
    }
    if (lane == 0u) {
        const bool tested = n_cols >= PG_DD_MIN_CONSENSUS;
        const u32 len = tested ? n_cols : 0u;
        a.cons_off[e] = len;
        pg_dd_cand *c = a.cands + e;
        c->cons_len = len;
        u32 flags = 0u, win_len = 0u;
        uint64_t win_start = 0ull;
        if (tested) {
            // the unsigned expressions of the reference; a start at or beyond the chromosome's end has a window of no bases
            const int64_t st = (int64_t)(int32_t)pos - (int64_t)a.min_map_distance;
            win_start = st > 0 ? (uint64_t)st : 0ull;
            if (win_start < (uint64_t)a.chr_size) win_len = min(a.chr_size - (u32)win_start, 2u * (u32)a.min_map_distance);
            flags = PG_DD_TESTED;
            atomicAdd(&a.info->n_tested, 1u);
            atomicMax(&a.info->max_cons, len);
        }
        c->flags = flags;
        c->win_len = win_len;
        c->win_start = win_start;
    }
}

// the pool packed from the slots (a '-' segment's bytes reversed), cons_off, the containment items
extern "C" __global__ void __launch_bounds__(PG_DD_WAVES * 64u) pg_ddt_pool_kernel(PgDdArgs a, u32 n_cands)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 e = blockIdx.x * PG_DD_WAVES + (threadIdx.x >> 6);
    if (e >= n_cands) return;
    const u32 off = a.cons_off[e], len = a.cons_off[e + 1u] - off;
    const bool plus = a.seg_strand[a.cands[e].seg] == '+';
    const uint8_t *slot = a.slots + (uint64_t)e * a.slot;
    for (u32 k = lane; k < len; k += 64u) a.cons[off + k] = slot[plus ? k : len - 1u - k];
    if (lane == 0u) {
        pg_dd_cand *c = a.cands + e;
        c->cons_off = off;                                     // (a dropped consensus: where the next one begins, no bytes)
        a.q_off[e] = off;
        a.q_chr[e] = a.chr_id;
        a.q_ws[e] = c->win_start;
        a.q_wl[e] = c->win_len;
        if (e == n_cands - 1u) {
            a.q_off[n_cands] = a.cons_off[n_cands];
            a.info->cons_bytes = a.cons_off[n_cands];
        }
    }
}

// ---- stage E: the verdicts
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_ddt_verdict_kernel(PgDdArgs a, u32 n_cands)
{
    const u32 e = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (e >= n_cands) return;
    if ((a.cands[e].flags & PG_DD_TESTED) && (a.q_out[2u * e] | a.q_out[2u * e + 1u])) a.cands[e].flags |= PG_DD_CONTAINED;
}

// ---- host side of the launches (pg_api_classify.cpp checks the arguments and owns the buffers)
static inline u32 dd_blocks(u32 m) { return (m + PG_EV_BLOCK - 1u) / PG_EV_BLOCK; }
static inline u32 dd_wave_blocks(u32 m) { return (m + PG_DD_WAVES - 1u) / PG_DD_WAVES; }

int pg_ddt_gather_launch(const PgDdArgs *a, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    PgDdInfo init;
    memset(&init, 0, sizeof init);
    for (int k = 0; k < PG_DD_KEY_WORDS; k++) init.key_and[k] = ~0u;
    if (hipMemcpyAsync(a->info, &init, sizeof init, hipMemcpyHostToDevice, st) != hipSuccess) return -1;
    if (hipStreamSynchronize(st) != hipSuccess) return -1;     // (init lives on this stack frame)
    if (!a->n) return 0;
    const u32 nb = dd_blocks(a->n);
    hipLaunchKernelGGL(pg_ddt_flag_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, *a);
    pg_table_rank_scan_launch(a->flag, a->n, a->rank, a->blk, st);
    hipLaunchKernelGGL(pg_ddt_compact_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int pg_ddt_sort_pass_launch(const PgDdArgs *a, const PgDdRec *src, PgDdRec *dst, uint32_t n_dd, int pass, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!n_dd) return 0;
    const u32 nb = dd_blocks(n_dd);
    hipLaunchKernelGGL(pg_ddt_digit_count_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, src, n_dd, pass, nb, a->digit_cnt);
    pg_table_scan_launch(a->digit_cnt, 256u * nb, st);
    hipLaunchKernelGGL(pg_ddt_scatter_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, src, dst, n_dd, pass, nb, (const u32 *)a->digit_cnt);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int pg_ddt_keys_launch(const PgDdArgs *a, const PgDdRec *sorted, uint32_t n_dd, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!n_dd) return 0;
    const u32 nb = dd_blocks(n_dd);
    hipLaunchKernelGGL(pg_ddt_head_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, *a, sorted, n_dd);
    pg_table_rank_scan_launch(a->flag, n_dd, a->rank, a->blk, st);
    hipLaunchKernelGGL(pg_ddt_first_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, *a, n_dd);
    hipLaunchKernelGGL(pg_ddt_keep_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, *a, n_dd);
    pg_table_rank_scan_launch(a->keep, n_dd, a->rank_m, a->blk_m, st);
    pg_table_rank_scan_launch(a->keep_head, n_dd, a->rank_c, a->blk_c, st);
    hipLaunchKernelGGL(pg_ddt_counts_kernel, dim3(1), dim3(1), 0, st, *a, n_dd);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int pg_ddt_tables_launch(const PgDdArgs *a, const PgDdRec *sorted, uint32_t n_dd, void *stream)
{
    if (!n_dd) return 0;
    hipLaunchKernelGGL(pg_ddt_member_kernel, dim3(dd_blocks(n_dd)), dim3(PG_EV_BLOCK), 0, (hipStream_t)stream, *a, sorted, n_dd);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int pg_ddt_consensus_launch(const PgDdArgs *a, uint32_t n_cands, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!n_cands) return 0;
    hipLaunchKernelGGL(pg_ddt_consensus_kernel, dim3(dd_wave_blocks(n_cands)), dim3(PG_DD_WAVES * 64u), 0, st, *a, n_cands);
    pg_table_scan_launch(a->cons_off, n_cands, st);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int pg_ddt_pool_launch(const PgDdArgs *a, uint32_t n_cands, void *stream)
{
    if (!n_cands) return 0;
    hipLaunchKernelGGL(pg_ddt_pool_kernel, dim3(dd_wave_blocks(n_cands)), dim3(PG_DD_WAVES * 64u), 0, (hipStream_t)stream, *a, n_cands);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int pg_ddt_verdict_launch(const PgDdArgs *a, uint32_t n_cands, void *stream)
{
    if (!n_cands) return 0;
    hipLaunchKernelGGL(pg_ddt_verdict_kernel, dim3(dd_blocks(n_cands)), dim3(PG_EV_BLOCK), 0, (hipStream_t)stream, *a, n_cands);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
