// pg_table_prims.hip -- the rank and scan kernels of the device classifier's table builds (pg_events.hip, pg_sv_events.hip,
// pg_li.hip), once, with their launchers.  Plain HIP, vector stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_device.h"
#include "pg_table_prims.h"

typedef uint32_t u32;

// ---- rank, scan, fill: rank[i] = flagged elements before i in its block, blk[b] = the block's count
extern "C" __global__ void __launch_bounds__(PG_EV_BLOCK) pg_table_rank_kernel(const uint8_t *flag, u32 m, u32 *rank, u32 *blk)
{
    const u32 i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    const u32 v = i < m ? (u32)(flag[i] != 0) : 0u;
    u32 tot;
    const u32 ex = block_excl_scan<PG_EV_BLOCK / 64u>(v, &tot);
    if (i < m) rank[i] = ex;
    if (threadIdx.x == 0u) blk[blockIdx.x] = tot;
}

// one workgroup: a[0 .. m) to its exclusive scan, in place; a[m] = the total (the array has m + 1 entries)
#define PG_TABLE_SCAN_THREADS 1024u
extern "C" __global__ void __launch_bounds__(PG_TABLE_SCAN_THREADS) pg_table_scan_kernel(u32 *a, u32 m)
{
    const u32 chunk = (m + PG_TABLE_SCAN_THREADS - 1u) / PG_TABLE_SCAN_THREADS;
    const u32 lo = threadIdx.x * chunk < m ? threadIdx.x * chunk : m;
    const u32 hi = lo + chunk < m ? lo + chunk : m;
    u32 s = 0;
    for (u32 k = lo; k < hi; k++) s += a[k];
    u32 tot;
    u32 run = block_excl_scan<PG_TABLE_SCAN_THREADS / 64u>(s, &tot);
    for (u32 k = lo; k < hi; k++) {
        const u32 v = a[k];
        a[k] = run;
        run += v;
    }
    if (threadIdx.x == 0u) a[m] = tot;
}

void pg_table_scan_launch(uint32_t *a, uint32_t m, void *stream)
{
    hipLaunchKernelGGL(pg_table_scan_kernel, dim3(1), dim3(PG_TABLE_SCAN_THREADS), 0, (hipStream_t)stream, a, m);
}

void pg_table_rank_scan_launch(const uint8_t *flag, uint32_t m, uint32_t *rank, uint32_t *blk, void *stream)
{
    const u32 nb = (m + PG_EV_BLOCK - 1u) / PG_EV_BLOCK;
    hipLaunchKernelGGL(pg_table_rank_kernel, dim3(nb), dim3(PG_EV_BLOCK), 0, (hipStream_t)stream, flag, m, rank, blk);
    pg_table_scan_launch(blk, nb, stream);
}
