// pg_li.hip -- the sixth part of the device classifier: the long-insertion position tables.  SortOutputLI counts, per
// anchor strand and per position of the last close point, the reads that kept a close end, found no far end and were used by no
// reporter; here those counters become tables with their member reads, so that _LI is written without a point leaving the GPU.
// The host statement of the same function is li_tables_from_reads (pg_host_li.cpp); the two must agree byte for byte.
//   stage A  pg_li_flag_kernel: one thread per read.  Close / far state and the last close point from the result record, the Used
//            state from the events build's record, the post-state read length from the bases; the LI reads are then compacted in
//            ASCENDING read index (rank, scan, fill), with the masks of their key bytes.
//   stage B  LSD counting passes over the key (strand, clamped position), skipping the bytes that are constant over the batch.
//            Every pass is stable, so equal keys keep the ascending read index: the order in which the host pushes them.
//   stage C  head flags (a member whose key differs from its predecessor's opens a position), scan, first members.
//   stage D  one wave per position: n_reads and the OR of its members' balance flags by ballot.  A position usually has a handful
//            of members, but the two ends of the buffered window collect every read beyond them: a wave, not a thread.
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
static_assert(sizeof(PgLiRec) == 16 && sizeof(pg_li_pos) == 16 && sizeof(pg_event_read) == 8, "layouts of the tables");

namespace {

// key byte `pass`, least significant first: the position's four bytes, then the strand
__device__ __forceinline__ u32 li_key_digit(const PgLiRec &r, int pass) { return pass >= 4 ? (r.w[2] & 0xffu) : (r.w[0] >> (pass * 8)) & 0xffu; }

}  // namespace

// ---- stage A
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_li_flag_kernel(PgLiArgs a)
{
    const u32 i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    uint8_t li = 0;
    if (a.chr[i] == a.chr_id) {
        const PgOutRec o = a.out[i];
        const uint8_t sd = a.strand[i];
        // (a list that does not lie in the pool counts as empty, as for the report summaries)
        const bool close = o.close_cnt && (unsigned long long)o.close_off + o.close_cnt <= a.pool_runs;
        const bool far = o.far_cnt && (unsigned long long)o.far_off + o.far_cnt <= a.pool_runs;
        const bool used = (a.reads[i].flags & (PG_EVR_BOXED | PG_EVR_USED)) != 0;
        if (close && !far && !used && (sd == '+' || sd == '-')) {
            const uint64_t s0 = a.seq_off[i];
            int32_t lead;                                                      // (not needed here)
            const int32_t RL = post_state_len(a.seq + s0, (int32_t)(a.seq_off[i + 1] - s0), o.rc_flag, &lead);
            const int32_t twice = 2 * (int32_t)(int16_t)o.close_max;          // UP_Close.back().LengthStr, a short
            const u32 p = o.close_last;                                        // ... and its AbsLoc
            PgLiRec r;
            r.w[0] = p < a.lo ? a.lo : p > a.hi ? a.hi : p;
            r.w[1] = i;
            r.w[2] = sd == '+' ? 0u : 1u;
            r.w[3] = twice > RL ? PG_LI_LONGER : twice < RL ? PG_LI_SHORTER : 0u;
            a.rec_a[i] = r;
            li = 1;
        }
    }
    a.flag[i] = li;
}

// the LI reads to rec_b in ascending read index; the masks of their key bytes and the number of '+' anchors
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_li_compact_kernel(PgLiArgs a)
{
    const u32 i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    const bool mine = i < a.n && a.flag[i];
    u32 k_or[2] = { 0u, 0u }, k_and[2] = { ~0u, ~0u };
    bool plus = false;
    if (mine) {
        const PgLiRec r = a.rec_a[i];
        a.rec_b[a.rank[i] + a.blk[blockIdx.x]] = r;
        k_or[0] = k_and[0] = r.w[0];
        k_or[1] = k_and[1] = r.w[2];
        plus = r.w[2] == 0u;
    }
    const u32 n_plus = (u32)__popcll(__ballot(plus));
    for (int k = 0; k < 2; k++) {
        const u32 o = wave_or(k_or[k]), n = wave_and(k_and[k]);
        if ((threadIdx.x & 63u) == 0u) {
            if (o) atomicOr(&a.info->key_or[k], o);
            if (n != ~0u) atomicAnd(&a.info->key_and[k], n);
        }
    }
    if ((threadIdx.x & 63u) == 0u && n_plus) atomicAdd(&a.info->n_plus, n_plus);
    if (i == 0u) a.info->n_li = a.blk[(a.n + PG_EV_BLOCK - 1u) / PG_EV_BLOCK];
}

// ---- stage B: one counting pass.  cnt[d * n_blk + b] = records of block b with digit d
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_li_digit_count_kernel(const PgLiRec *src, u32 m, int pass, u32 n_blk, u32 *cnt)
{
    tab_digit_count(src, m, n_blk, cnt, [pass](const PgLiRec &r) { return li_key_digit(r, pass); });
}
// cnt scanned: the place of a record = cnt[its digit][its block] + the records of its block before it with the same digit
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_li_scatter_kernel(const PgLiRec *src, PgLiRec *dst, u32 m, int pass, u32 n_blk,
                                                                                const u32 *cnt)
{
    tab_scatter(src, dst, m, n_blk, cnt, [pass](const PgLiRec &r) { return li_key_digit(r, pass); });
}

// ---- stage C: flag[m] = member m opens a position; members[m] = its read
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_li_head_kernel(PgLiArgs a, const PgLiRec *s, u32 n_li)
{
    const u32 m = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (m >= n_li) return;
    const PgLiRec r = s[m];
    bool head = m == 0u;
    if (!head) {
        const PgLiRec q = s[m - 1u];
        head = q.w[0] != r.w[0] || q.w[2] != r.w[2];
    }
    a.flag[m] = (uint8_t)head;
    a.members[m] = r.w[1];
}
// pfirst[e] = the first member of position e (one entry more: the number of members); the positions of the '+' strand
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_li_first_kernel(PgLiArgs a, u32 n_li, u32 n_plus)
{
    const u32 n_pos = a.blk[(n_li + PG_EV_BLOCK - 1u) / PG_EV_BLOCK];
    const u32 m = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (m >= n_li) return;
    const u32 e = a.rank[m] + a.blk[blockIdx.x];
    if (a.flag[m]) a.pfirst[e] = m;
    // (the first '-' member opens a position: the strand is the key's most significant digit)
    if (m == n_plus) a.info->pos_plus = e;
    if (m == n_li - 1u) {
        a.pfirst[n_pos] = n_li;
        a.info->n_pos = n_pos;
        if (n_plus == n_li) a.info->pos_plus = n_pos;
    }
}

// ---- stage D: one wave per position
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_li_pos_kernel(PgLiArgs a, const PgLiRec *s, u32 n_plus)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 e = blockIdx.x * (PG_EV_BLOCK / 64u) + (threadIdx.x >> 6);
    if (e >= a.info->n_pos) return;                           // (whole waves)
    const u32 first = a.pfirst[e], end = a.pfirst[e + 1u];
    bool longer = false, shorter = false;
    for (u32 m0 = first; m0 < end; m0 += 64u) {
        const u32 m = m0 + lane;
        const u32 f = m < end ? s[m].w[3] : 0u;
        longer |= __ballot((f & PG_LI_LONGER) != 0u) != 0ull;
        shorter |= __ballot((f & PG_LI_SHORTER) != 0u) != 0ull;
    }
    if (lane == 0u) {
        const PgLiRec f = s[first];
        pg_li_pos p;
        p.pos = f.w[0];
        p.first = first - (f.w[2] ? n_plus : 0u);
        p.n_reads = end - first;
        p.flags = (longer ? PG_LI_LONGER : 0u) | (shorter ? PG_LI_SHORTER : 0u);
        a.positions[e] = p;
    }
}

// ---- host side of the launches (pg_api_classify.cpp checks the arguments and owns the buffers)
static inline u32 li_blocks(u32 m) { return (m + PG_EV_BLOCK - 1u) / PG_EV_BLOCK; }

int pg_li_gather_launch(const PgLiArgs *a, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    PgLiInfo init;
    memset(&init, 0, sizeof init);
    init.key_and[0] = init.key_and[1] = ~0u;
    if (hipMemcpyAsync(a->info, &init, sizeof init, hipMemcpyHostToDevice, st) != hipSuccess) return -1;
    if (hipStreamSynchronize(st) != hipSuccess) return -1;     // (init lives on this stack frame)
    if (!a->n) return 0;
    const u32 nb = li_blocks(a->n);
    hipLaunchKernelGGL(pg_li_flag_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, *a);
    pg_table_rank_scan_launch(a->flag, a->n, a->rank, a->blk, st);
    hipLaunchKernelGGL(pg_li_compact_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int pg_li_sort_pass_launch(const PgLiArgs *a, const PgLiRec *src, PgLiRec *dst, uint32_t n_li, int pass, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!n_li) return 0;
    const u32 nb = li_blocks(n_li);
    hipLaunchKernelGGL(pg_li_digit_count_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, src, n_li, pass, nb, a->digit_cnt);
    pg_table_scan_launch(a->digit_cnt, 256u * nb, st);
    hipLaunchKernelGGL(pg_li_scatter_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, src, dst, n_li, pass, nb, (const u32 *)a->digit_cnt);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int pg_li_tables_launch(const PgLiArgs *a, const PgLiRec *sorted, uint32_t n_li, uint32_t n_plus, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!n_li) return 0;
    const u32 nb = li_blocks(n_li);
    hipLaunchKernelGGL(pg_li_head_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, *a, sorted, n_li);
    pg_table_rank_scan_launch(a->flag, n_li, a->rank, a->blk, st);
    hipLaunchKernelGGL(pg_li_first_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, *a, n_li, n_plus);
    // (at most n_li positions: a grid over that many waves, the surplus ones leave at once)
    hipLaunchKernelGGL(pg_li_pos_kernel, dim3((n_li + PG_EV_BLOCK / 64u - 1u) / (PG_EV_BLOCK / 64u)), dim3(PG_EV_BLOCK), 0, st, *a, sorted, n_plus);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
