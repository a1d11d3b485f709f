// pg_int.hip -- the seventh part of the device classifier: the interchromosomal junction tables.
// SortAndReportInterChromosomalEvents takes, per read whose far end lies on another chromosome, the pair of points that carries its
// call; here those pairs become tables with their member reads, so that _INT is written without a point leaving the GPU.
// The host statement of the same function is int_tables_from_reads (pg_host_int.cpp); the two must agree byte for byte.
//   stage A  pg_int_flag_kernel: one thread per read.  The junction test from the result record, the chromosome, the anchor strand and
//            the first far run; then the walk over both run lists for the template pair, or the fallback from the two last points.
//            The reads with a call are compacted in ASCENDING read index (rank, scan, fill), with the masks of their key bytes.
//   stage B  LSD counting passes over the key, skipping the bytes that are constant over the batch.  Every pass is stable, so equal
//            keys keep the ascending read index.
//   stage C  head flags (a member whose key differs from its predecessor's opens a call), scan, first members.
//   stage D  one thread per call: groups are a handful of reads, and a call's fields are those of its first member.
// The scan stages and the bodies of the counting passes are the shared ones of pg_table_prims.h, here over a 32-byte record.
// Plain HIP, vector stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "pg_device.h"
#include "pg_table_prims.h"
#include "pg_variant_dev.h"

typedef uint32_t u32;
static_assert(PG_EV_BLOCK == 256u, "one thread per digit value in the counting kernels");
static_assert(sizeof(PgIntRec) == 32 && sizeof(pg_int_call) == 32 && sizeof(pg_run) == 12, "layouts of the tables");

namespace {

// key byte `pass`, least significant first: w[0], w[1], w[2] (four bytes each), the flags (one), w[4] (four)
__device__ __forceinline__ u32 int_key_digit(const PgIntRec &r, int pass)
{
    // (selects, not r.w[word]: an index known only at run time would move the whole record out of its registers)
    const u32 w = pass < 4 ? r.w[0] : pass < 8 ? r.w[1] : pass < 12 ? r.w[2] : pass == 12 ? r.w[3] : r.w[4];
    const int byte = pass < 12 ? pass & 3 : pass == 12 ? 0 : pass - 13;
    return (w >> (byte * 8)) & 0xffu;
}

__device__ __forceinline__ u32 run_abs(const pg_run &r, int32_t d) { return (r.flags & PG_RUN_BACKWARD) ? r.abs_loc_first - (u32)d : r.abs_loc_first + (u32)d; }

}  // namespace

// ---- stage A
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_int_flag_kernel(PgIntArgs a)
{
    const u32 i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    uint8_t has_call = 0;
    const int32_t chr = a.chr[i];
    const PgOutRec o = a.out[i];
    const uint8_t sd = a.strand[i];
    // (a list that does not lie in the pool counts as empty, as for the report summaries)
    const bool close = o.close_cnt && (unsigned long long)o.close_off + o.close_cnt <= a.pool_runs;
    const bool far = o.far_cnt && (unsigned long long)o.far_off + o.far_cnt <= a.pool_runs;
    if (close && far && chr >= 0 && (u32)chr < a.n_chr && (sd == '+' || sd == '-')) {
        const pg_run *cr = a.pool + o.close_off, *fr = a.pool + o.far_off;
        const pg_run f0 = fr[0];                                               // UP_Far[0]
        const int32_t fc = f0.chr_id;
        if (fc >= 0 && (u32)fc < a.n_chr && a.chr_rank[chr] != a.chr_rank[fc]) {
            const bool far_minus = (f0.flags & PG_RUN_ANTISENSE) != 0;
            const bool asc = a.chr_rank[chr] < a.chr_rank[fc] ? sd == '+' : far_minus;
            const uint64_t s0 = a.seq_off[i];
            int32_t lead;                                                      // (not needed here)
            const int32_t len = post_state_len(a.seq + s0, (int32_t)(a.seq_off[i + 1] - s0), o.rc_flag, &lead);
            // The template pair.  Close runs in scan order; within one, the first point d (LengthStr lf + d) for which some far run
            // holds LengthStr len - lf - d: per far run those d form an interval, and its end nearest the scan's start counts.
            // Far runs in the opposite order; a tie keeps the earlier one, which is the first far point the plain loops meet.
            bool found = false;
            u32 close_abs = 0, far_abs = 0;
            for (u32 ka = 0; ka < o.close_cnt && !found; ka++) {
                const pg_run r = cr[asc ? ka : o.close_cnt - 1u - ka];
                const int32_t lf = r.len_first, m = (int32_t)r.len_last - lf + 1;
                int32_t best_d = -1, best_fd = 0;
                u32 best_j = 0;
                for (u32 kb = 0; kb < o.far_cnt; kb++) {
                    const u32 j = asc ? o.far_cnt - 1u - kb : kb;
                    const pg_run q = fr[j];
                    const int32_t d_lo = max(0, len - lf - (int32_t)q.len_last), d_hi = min(m - 1, len - lf - (int32_t)q.len_first);
                    if (d_lo > d_hi) continue;
                    const int32_t d = asc ? d_lo : d_hi;
                    if (best_d < 0 || (asc ? d < best_d : d > best_d)) {
                        best_d = d;
                        best_j = j;
                        best_fd = len - lf - d - (int32_t)q.len_first;
                    }
                }
                if (best_d >= 0) {
                    found = true;
                    close_abs = run_abs(r, best_d);
                    far_abs = run_abs(fr[best_j], best_fd);
                }
            }
            u32 flags = (sd == '+' ? 0u : PG_INT_ANCHOR_MINUS) | (far_minus ? PG_INT_FAR_MINUS : 0u);
            u32 nt = 0;
            if (!found) {
                // the fallback: UP_Close.back() and UP_Far.back(), the last point of either last run
                const pg_run c = cr[o.close_cnt - 1u], f = fr[o.far_cnt - 1u];
                const int32_t cl = c.len_last, fl = f.len_last, eff = cl + fl;
                if (eff >= 30 && cl >= 10 && fl >= 10) {
                    found = true;
                    close_abs = run_abs(c, cl - (int32_t)c.len_first);
                    far_abs = run_abs(f, fl - (int32_t)f.len_first);
                    const int32_t n = eff > len ? len - fl : len - eff;
                    flags |= PG_INT_FALLBACK;
                    nt = ((u32)fl & 0xffffu) << 16 | ((u32)max(n, 0) & 0xffffu);
                }
            }
            if (found) {
                PgIntRec r;
                r.w[0] = nt;
                r.w[1] = far_abs;
                r.w[2] = close_abs;
                r.w[3] = flags;
                r.w[4] = ((u32)chr & 0xffffu) << 16 | ((u32)fc & 0xffffu);
                r.w[5] = i;
                r.w[6] = r.w[7] = 0u;
                a.rec_a[i] = r;
                has_call = 1;
            }
        }
    }
    a.flag[i] = has_call;
}

// the reads with a call to rec_b in ascending read index; the masks of their key bytes
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_int_compact_kernel(PgIntArgs a)
{
    const u32 i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    const bool mine = i < a.n && a.flag[i];
    u32 k_or[PG_INT_KEY_WORDS], k_and[PG_INT_KEY_WORDS];
#pragma unroll
    for (int k = 0; k < PG_INT_KEY_WORDS; k++) {
        k_or[k] = 0u;
        k_and[k] = ~0u;
    }
    if (mine) {
        const PgIntRec r = a.rec_a[i];
        a.rec_b[a.rank[i] + a.blk[blockIdx.x]] = r;
#pragma unroll
        for (int k = 0; k < PG_INT_KEY_WORDS; k++) k_or[k] = k_and[k] = r.w[k];
    }
#pragma unroll
    for (int k = 0; k < PG_INT_KEY_WORDS; k++) {
        const u32 o = wave_or(k_or[k]), n = wave_and(k_and[k]);
        if ((threadIdx.x & 63u) == 0u) {
            if (o) atomicOr(&a.info->key_or[k], o);
            if (n != ~0u) atomicAnd(&a.info->key_and[k], n);
        }
    }
    if (i == 0u) a.info->n_mem = a.blk[(a.n + PG_EV_BLOCK - 1u) / PG_EV_BLOCK];
}

// ---- stage B: one counting pass.  cnt[d * n_blk + b] = records of block b with digit d
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_int_digit_count_kernel(const PgIntRec *src, u32 m, int pass, u32 n_blk, u32 *cnt)
{
    tab_digit_count(src, m, n_blk, cnt, [pass](const PgIntRec &r) { return int_key_digit(r, pass); });
}
// cnt scanned: the place of a record = cnt[its digit][its block] + the records of its block before it with the same digit
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_int_scatter_kernel(const PgIntRec *src, PgIntRec *dst, u32 m, int pass, u32 n_blk,
                                                                                 const u32 *cnt)
{
    tab_scatter(src, dst, m, n_blk, cnt, [pass](const PgIntRec &r) { return int_key_digit(r, pass); });
}

// ---- stage C: flag[m] = member m opens a call; members[m] = its read
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_int_head_kernel(PgIntArgs a, const PgIntRec *s, u32 n_mem)
{
    const u32 m = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (m >= n_mem) return;
    const PgIntRec r = s[m];
    bool head = m == 0u;
    if (!head) {
        const PgIntRec q = s[m - 1u];
#pragma unroll
        for (int k = 0; k < PG_INT_KEY_WORDS; k++) head |= q.w[k] != r.w[k];
    }
    a.flag[m] = (uint8_t)head;
    a.members[m] = r.w[5];
}
// cfirst[e] = the first member of call e (one entry more: the number of members)
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_int_first_kernel(PgIntArgs a, u32 n_mem)
{
    const u32 n_calls = a.blk[(n_mem + PG_EV_BLOCK - 1u) / PG_EV_BLOCK];
    const u32 m = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (m >= n_mem) return;
    if (a.flag[m]) a.cfirst[a.rank[m] + a.blk[blockIdx.x]] = m;
    if (m == n_mem - 1u) {
        a.cfirst[n_calls] = n_mem;
        a.info->n_calls = n_calls;
    }
}

// ---- stage D: one thread per call
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_int_call_kernel(PgIntArgs a, const PgIntRec *s, u32 n_mem)
{
    const u32 e = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (e >= a.info->n_calls) return;
    const u32 first = a.cfirst[e], end = a.cfirst[e + 1u];
    if (first >= n_mem) return;                               // (never: a call has a first member)
    const PgIntRec f = s[first];
    pg_int_call c;
    c.chr = (int16_t)(f.w[4] >> 16);
    c.far_chr = (int16_t)(f.w[4] & 0xffffu);
    c.close_abs = f.w[2];
    c.far_abs = f.w[1];
    c.first = first;
    c.n_reads = end - first;
    c.nt_off = (uint16_t)(f.w[0] >> 16);
    c.nt_len = (uint16_t)(f.w[0] & 0xffffu);
    c.flags = f.w[3];
    c.reserved = 0u;
    a.calls[e] = c;
}

// ---- host side of the launches (pg_api_classify.cpp checks the arguments and owns the buffers)
static inline u32 int_blocks(u32 m) { return (m + PG_EV_BLOCK - 1u) / PG_EV_BLOCK; }

int pg_int_gather_launch(const PgIntArgs *a, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    PgIntInfo init;
    memset(&init, 0, sizeof init);
    for (int k = 0; k < PG_INT_KEY_WORDS; k++) init.key_and[k] = ~0u;
    if (hipMemcpyAsync(a->info, &init, sizeof init, hipMemcpyHostToDevice, st) != hipSuccess) return -1;
    if (hipStreamSynchronize(st) != hipSuccess) return -1;     // (init lives on this stack frame)
    if (!a->n) return 0;
    const u32 nb = int_blocks(a->n);
    hipLaunchKernelGGL(pg_int_flag_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, *a);
    pg_table_rank_scan_launch(a->flag, a->n, a->rank, a->blk, st);
    hipLaunchKernelGGL(pg_int_compact_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int pg_int_sort_pass_launch(const PgIntArgs *a, const PgIntRec *src, PgIntRec *dst, uint32_t n_mem, int pass, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!n_mem) return 0;
    const u32 nb = int_blocks(n_mem);
    hipLaunchKernelGGL(pg_int_digit_count_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, src, n_mem, pass, nb, a->digit_cnt);
    pg_table_scan_launch(a->digit_cnt, 256u * nb, st);
    hipLaunchKernelGGL(pg_int_scatter_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, src, dst, n_mem, pass, nb, (const u32 *)a->digit_cnt);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int pg_int_tables_launch(const PgIntArgs *a, const PgIntRec *sorted, uint32_t n_mem, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!n_mem) return 0;
    const u32 nb = int_blocks(n_mem);
    hipLaunchKernelGGL(pg_int_head_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, *a, sorted, n_mem);
    pg_table_rank_scan_launch(a->flag, n_mem, a->rank, a->blk, st);
    hipLaunchKernelGGL(pg_int_first_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, *a, n_mem);
    // (at most n_mem calls: a grid over that many threads, the surplus ones leave at once)
    hipLaunchKernelGGL(pg_int_call_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, st, *a, sorted, n_mem);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
