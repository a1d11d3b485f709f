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
// The scan and sort stages restate those of pg_events.hip for a 16-byte record.  Plain HIP, vector stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "pg_device.h"
#include "pg_variant_dev.h"

typedef uint32_t u32;
static_assert(PG_EV_BLOCK == 256u, "one thread per digit value in the counting kernels");
static_assert(sizeof(PgLiRec) == 16 && sizeof(pg_li_pos) == 16 && sizeof(pg_event_read) == 8, "layouts of the tables");

namespace {

// the post-state's length (pg_events.hip): rc_flag applications of setUnmatchedSeq(ReverseComplement()) strip the bytes outside
// ACGTN the read began with (first application) and ended with (second)
__device__ int32_t li_post_state_len(const uint8_t *s, int32_t L, uint32_t rc_flag)
{
    if (!rc_flag) return L;
    int32_t first_ok = 0;
    while (first_ok < L && base_code(s[first_ok]) == (uint32_t)PG_VA_NONE) first_ok++;
    int32_t last_ok = L - 1;
    if (rc_flag >= 2)
        while (last_ok >= first_ok && base_code(s[last_ok]) == (uint32_t)PG_VA_NONE) last_ok--;
    return last_ok + 1 - first_ok;
}

// exclusive scan of one value per thread over a workgroup of NW waves; *total = the workgroup's sum
template <u32 NW>
__device__ __forceinline__ u32 li_block_excl_scan(u32 v, u32 *total)
{
    __shared__ u32 wave_sum[NW];
    const u32 lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    u32 inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const u32 o = (u32)__shfl_up((int)inc, d, 64);
        if (lane >= (u32)d) inc += o;
    }
    if (lane == 63u) wave_sum[w] = inc;
    __syncthreads();
    u32 base = 0, tot = 0;
    for (u32 k = 0; k < NW; k++) {
        const u32 s = wave_sum[k];
        if (k < w) base += s;
        tot += s;
    }
    __syncthreads();                                      // (the next call writes wave_sum again)
    *total = tot;
    return base + inc - v;
}

__device__ __forceinline__ u32 li_wave_or(u32 v)
{
    for (int m = 32; m >= 1; m >>= 1) v |= (u32)__shfl_xor((int)v, m, 64);
    return v;
}
__device__ __forceinline__ u32 li_wave_and(u32 v)
{
    for (int m = 32; m >= 1; m >>= 1) v &= (u32)__shfl_xor((int)v, m, 64);
    return v;
}

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
            const int32_t RL = li_post_state_len(a.seq + s0, (int32_t)(a.seq_off[i + 1] - s0), o.rc_flag);
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

// ---- rank, scan, fill: rank[i] = flagged elements before i in its block, blk[b] = the block's count
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_li_rank_kernel(const uint8_t *flag, u32 m, u32 *rank, u32 *blk)
{
    const u32 i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    const u32 v = i < m ? (u32)(flag[i] != 0) : 0u;
    u32 tot;
    const u32 ex = li_block_excl_scan<PG_EV_BLOCK / 64u>(v, &tot);
    if (i < m) rank[i] = ex;
    if (threadIdx.x == 0u) blk[blockIdx.x] = tot;
}

// one workgroup: a[0 .. m) to its exclusive scan, in place; a[m] = the total (the array has m + 1 entries)
#define PG_LI_SCAN_THREADS 1024u
extern "C" __global__ void __launch_bounds__(PG_LI_SCAN_THREADS) pg_li_scan_kernel(u32 *a, u32 m)
{
    const u32 chunk = (m + PG_LI_SCAN_THREADS - 1u) / PG_LI_SCAN_THREADS;
    const u32 lo = threadIdx.x * chunk < m ? threadIdx.x * chunk : m;
    const u32 hi = lo + chunk < m ? lo + chunk : m;
    u32 s = 0;
    for (u32 k = lo; k < hi; k++) s += a[k];
    u32 tot;
    u32 run = li_block_excl_scan<PG_LI_SCAN_THREADS / 64u>(s, &tot);
    for (u32 k = lo; k < hi; k++) {
        const u32 v = a[k];
        a[k] = run;
        run += v;
    }
    if (threadIdx.x == 0u) a[m] = tot;
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
        const u32 o = li_wave_or(k_or[k]), n = li_wave_and(k_and[k]);
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
    __shared__ u32 hist[256];
    hist[threadIdx.x] = 0u;
    __syncthreads();
    const u32 i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (i < m) atomicAdd(&hist[li_key_digit(src[i], pass)], 1u);
    __syncthreads();
    cnt[threadIdx.x * n_blk + blockIdx.x] = hist[threadIdx.x];
}

// cnt scanned: the place of a record = cnt[its digit][its block] + the records of its block before it with the same digit
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_li_scatter_kernel(const PgLiRec *src, PgLiRec *dst, u32 m, int pass, u32 n_blk,
                                                                                const u32 *cnt)
{
    __shared__ uint8_t dig[PG_EV_BLOCK];
    const u32 i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    PgLiRec r;
    u32 d = 0;
    if (i < m) {
        r = src[i];
        d = li_key_digit(r, pass);
    }
    dig[threadIdx.x] = (uint8_t)d;
    __syncthreads();
    if (i >= m) return;
    u32 before = 0;
    for (u32 t = 0; t < threadIdx.x; t++) before += (u32)(dig[t] == (uint8_t)d);
    dst[cnt[d * n_blk + blockIdx.x] + before] = r;
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

// ---- host side of the launches (pg_api.cpp checks the arguments and owns the buffers)
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
    hipLaunchKernelGGL(pg_li_rank_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, (const uint8_t *)a->flag, a->n, a->rank, a->blk);
    hipLaunchKernelGGL(pg_li_scan_kernel, dim3(1), dim3(PG_LI_SCAN_THREADS), 0, st, a->blk, nb);
    hipLaunchKernelGGL(pg_li_compact_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int pg_li_sort_pass_launch(const PgLiArgs *a, const PgLiRec *src, PgLiRec *dst, uint32_t n_li, int pass, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!n_li) return 0;
    const u32 nb = li_blocks(n_li);
    hipLaunchKernelGGL(pg_li_digit_count_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, src, n_li, pass, nb, a->digit_cnt);
    hipLaunchKernelGGL(pg_li_scan_kernel, dim3(1), dim3(PG_LI_SCAN_THREADS), 0, st, a->digit_cnt, 256u * nb);
    hipLaunchKernelGGL(pg_li_scatter_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, src, dst, n_li, pass, nb, (const u32 *)a->digit_cnt);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int pg_li_tables_launch(const PgLiArgs *a, const PgLiRec *sorted, uint32_t n_li, uint32_t n_plus, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!n_li) return 0;
    const u32 nb = li_blocks(n_li);
    hipLaunchKernelGGL(pg_li_head_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, *a, sorted, n_li);
    hipLaunchKernelGGL(pg_li_rank_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, (const uint8_t *)a->flag, n_li, a->rank, a->blk);
    hipLaunchKernelGGL(pg_li_scan_kernel, dim3(1), dim3(PG_LI_SCAN_THREADS), 0, st, a->blk, nb);
    hipLaunchKernelGGL(pg_li_first_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, *a, n_li, n_plus);
    // (at most n_li positions: a grid over that many waves, the surplus ones leave at once)
    hipLaunchKernelGGL(pg_li_pos_kernel, dim3((n_li + PG_EV_BLOCK / 64u - 1u) / (PG_EV_BLOCK / 64u)), dim3(PG_EV_BLOCK), 0, st, *a, sorted, n_plus);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
