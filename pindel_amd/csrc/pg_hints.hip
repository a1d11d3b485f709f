// pg_hints.hip -- position-keyed hint tables (pg_hint_table, pindel_pg.h) resolved on the device: from each read's close-end
// summary (UP_Close.back().AbsLoc / LengthStr, already in HBM) to the per-read window CSR the far end reads
// (pg_device_batch::bd_off / bd), what BDData::getCorrespondingSearchWindowCluster answers per read (src/bddata.cpp:949-979)
// without the summary leaving the device.  Three steps on the context's stream, between the close-end summary and the far launch:
//   count   one thread per read: binary search of run_first (a few KB: it sits in L2), the read's window count; the largest count
//           and the longest window of the clusters actually used folded into two words (what picks 32- or 64-bit candidate ids)
//   scan    exclusive scan of the counts into the 64-bit offsets, n + 1 entries: block sums, scan of the block sums, add
//   fill    one wavefront per read, the lanes stride over the cluster's windows: a coalesced dword copy
// The host reads 16 bytes between scan and fill (total, the two maxima) to size the window array and choose the launch.
// Not search kernels: the default code generation (Makefile).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_device.h"

typedef uint32_t u32;
typedef unsigned long long u64;

#define PG_HINT_BLOCK 256u
#define PG_HINT_ITEMS 4u                                  // counts per thread of the scan
#define PG_HINT_TILE PG_HINT_SCAN_TILE                    // counts per workgroup of the scan
static_assert(PG_HINT_TILE == PG_HINT_BLOCK * PG_HINT_ITEMS, "the scan's tile is one workgroup's threads x items");

// The lookup rule: no windows without a close end or outside [run_first[0], run_first[n_runs]); otherwise the cluster of the run
// that holds p.  Returns the cluster, or -1.
static __device__ __forceinline__ long long hint_cluster(const PgDevHintTable &t, u32 p, u32 close_max)
{
    if (close_max == 0u || t.n_runs == 0u) return -1;
    if (p < t.run_first[0] || p >= t.run_first[t.n_runs]) return -1;
    u32 lo = 0u, hi = t.n_runs;                           // run_first[lo] <= p < run_first[hi]
    while (hi - lo > 1u) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (t.run_first[mid] <= p) lo = mid;
        else hi = mid;
    }
    return (long long)t.run_cluster[lo];
}

static __device__ __forceinline__ u32 wave_max(u32 v)
{
    for (int d = 32; d > 0; d >>= 1) {
        const u32 o = (u32)__shfl_xor((int)v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// cnt[i] = windows of read i (i < n), cnt[n] = 0; info[2] = largest count (saturated at 2^32 - 1), info[3] = longest window used
__global__ void __launch_bounds__(PG_HINT_BLOCK)
pg_hint_count_kernel(PgDevHintTable t, const u32 *close_last, const uint16_t *close_max, u32 n, u64 *cnt, u32 *info)
{
    const u64 i = (u64)blockIdx.x * PG_HINT_BLOCK + threadIdx.x;
    u64 c = 0;
    u32 longest = 0u;
    if (i < n) {
        const long long k = hint_cluster(t, close_last[i], close_max[i]);
        if (k >= 0) {
            c = t.cluster_off[k + 1] - t.cluster_off[k];
            if (c) longest = t.cluster_longest[k];
        }
    }
    if (i <= n) cnt[i] = c;
    const u32 most = wave_max(c > 0xffffffffull ? 0xffffffffu : (u32)c);
    longest = wave_max(longest);
    if ((threadIdx.x & 63u) == 0u) {
        if (most) atomicMax(&info[2], most);
        if (longest) atomicMax(&info[3], longest);
    }
}

// exclusive scan of one value per thread over the workgroup; *total = the workgroup's sum
static __device__ __forceinline__ u64 block_excl_scan(u64 v, u64 *total)
{
    __shared__ u64 wave_sum[PG_HINT_BLOCK / 64u];
    const u32 lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    u64 inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const u64 o = __shfl_up(inc, d, 64);
        if (lane >= (u32)d) inc += o;
    }
    if (lane == 63u) wave_sum[w] = inc;
    __syncthreads();
    u64 base = 0, tot = 0;
    for (u32 k = 0; k < PG_HINT_BLOCK / 64u; k++) {
        const u64 s = wave_sum[k];
        if (k < w) base += s;
        tot += s;
    }
    __syncthreads();                                      // (the next call writes wave_sum again)
    *total = tot;
    return base + inc - v;
}

// pass 1: blk[b] = sum of the counts of tile b
__global__ void __launch_bounds__(PG_HINT_BLOCK)
pg_hint_scan_sums_kernel(const u64 *cnt, u64 m, u64 *blk)
{
    const u64 at = (u64)blockIdx.x * PG_HINT_TILE + (u64)threadIdx.x * PG_HINT_ITEMS;
    u64 s = 0;
    for (u32 k = 0; k < PG_HINT_ITEMS; k++)
        if (at + k < m) s += cnt[at + k];
    u64 tot;
    (void)block_excl_scan(s, &tot);
    if (threadIdx.x == 0u) blk[blockIdx.x] = tot;
}

// pass 2 (one workgroup): blk[] to its exclusive scan; the total into info[0 .. 1] (64 bits)
__global__ void __launch_bounds__(PG_HINT_BLOCK)
pg_hint_scan_blocks_kernel(u64 *blk, u32 n_blk, u32 *info)
{
    u64 carry = 0;
    for (u32 base = 0; base < n_blk; base += PG_HINT_BLOCK) {
        const u32 k = base + threadIdx.x;
        const u64 v = k < n_blk ? blk[k] : 0ull;
        u64 tot;
        const u64 ex = block_excl_scan(v, &tot);
        if (k < n_blk) blk[k] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0u) {
        info[0] = (u32)carry;
        info[1] = (u32)(carry >> 32);
    }
}

// pass 3: the counts of tile b to offsets, in place
__global__ void __launch_bounds__(PG_HINT_BLOCK)
pg_hint_scan_add_kernel(u64 *cnt, u64 m, const u64 *blk)
{
    const u64 at = (u64)blockIdx.x * PG_HINT_TILE + (u64)threadIdx.x * PG_HINT_ITEMS;
    u64 v[PG_HINT_ITEMS], s = 0;
    for (u32 k = 0; k < PG_HINT_ITEMS; k++) {
        v[k] = at + k < m ? cnt[at + k] : 0ull;
        s += v[k];
    }
    u64 tot;
    u64 run = block_excl_scan(s, &tot) + blk[blockIdx.x];
    for (u32 k = 0; k < PG_HINT_ITEMS; k++) {
        if (at + k < m) cnt[at + k] = run;
        run += v[k];
    }
}

// one wavefront per read: the windows of the read's cluster to bd[bd_off[i] .. bd_off[i + 1]), as dwords (a pg_window is three)
__global__ void __launch_bounds__(PG_HINT_BLOCK)
pg_hint_fill_kernel(PgDevHintTable t, const u32 *close_last, const uint16_t *close_max, u32 n, const u64 *bd_off, pg_window *bd)
{
    const u64 i = (u64)blockIdx.x * (PG_HINT_BLOCK / 64u) + (threadIdx.x >> 6);
    if (i >= n) return;
    const u64 lo = bd_off[i], c = bd_off[i + 1] - lo;
    if (!c) return;
    const long long k = hint_cluster(t, close_last[i], close_max[i]);
    if (k < 0) return;
    const u64 from = t.cluster_off[k];
    if (t.cluster_off[k + 1] - from != c) return;         // (cannot happen: the offsets were scanned from these counts)
    const u32 *src = (const u32 *)(t.windows + from);
    u32 *dst = (u32 *)(bd + lo);
    for (u64 j = threadIdx.x & 63u; j < 3ull * c; j += 64ull) dst[j] = src[j];
}

extern "C" int pg_hint_count_scan(const PgDevHintTable *t, const uint32_t *close_last, const uint16_t *close_max, uint32_t n,
                                  unsigned long long *bd_off, unsigned long long *blk, uint32_t *info, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(info, 0, 4 * sizeof(uint32_t), st);
    if (e != hipSuccess) return (int)e;
    const u64 m = (u64)n + 1ull;
    const u32 n_blk = pg_hint_scan_blocks(n);
    pg_hint_count_kernel<<<(u32)((m + PG_HINT_BLOCK - 1ull) / PG_HINT_BLOCK), PG_HINT_BLOCK, 0, st>>>(*t, close_last, close_max, n, bd_off, info);
    pg_hint_scan_sums_kernel<<<n_blk, PG_HINT_BLOCK, 0, st>>>(bd_off, m, blk);
    pg_hint_scan_blocks_kernel<<<1, PG_HINT_BLOCK, 0, st>>>(blk, n_blk, info);
    pg_hint_scan_add_kernel<<<n_blk, PG_HINT_BLOCK, 0, st>>>(bd_off, m, blk);
    return (int)hipGetLastError();
}

extern "C" int pg_hint_fill(const PgDevHintTable *t, const uint32_t *close_last, const uint16_t *close_max, uint32_t n,
                            const unsigned long long *bd_off, pg_window *bd, void *stream)
{
    if (n) {
        const u32 per = PG_HINT_BLOCK / 64u;
        pg_hint_fill_kernel<<<(u32)(((u64)n + per - 1ull) / per), PG_HINT_BLOCK, 0, (hipStream_t)stream>>>(*t, close_last, close_max, n, bd_off, bd);
    }
    return (int)hipGetLastError();
}
