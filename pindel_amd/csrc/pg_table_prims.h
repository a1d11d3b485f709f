// pg_table_prims.h -- what the table builds of the device classifier share (pg_events.hip, pg_sv_events.hip, pg_li.hip, pg_int.hip): the
// workgroup scan, the wave reductions, the post-state's length and the two bodies of one LSD counting pass.  Device-only inline
// code; the rank and scan kernels themselves live once in pg_table_prims.hip (launchers in pg_device.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_device.h"
#include "pg_variant_dev.h"

// the post-state's length (pg_variant.hip): rc_flag applications of setUnmatchedSeq(ReverseComplement()) strip the bytes outside
// ACGTN the read began with (first application) and ended with (second); *lead = its first base among the bytes as uploaded
__device__ inline int32_t post_state_len(const uint8_t *s, int32_t L, uint32_t rc_flag, int32_t *lead)
{
    *lead = 0;
    if (!rc_flag) return L;
    int32_t first_ok = 0;
    while (first_ok < L && base_code(s[first_ok]) == (uint32_t)PG_VA_NONE) first_ok++;
    int32_t last_ok = L - 1;
    if (rc_flag >= 2)
        while (last_ok >= first_ok && base_code(s[last_ok]) == (uint32_t)PG_VA_NONE) last_ok--;
    *lead = first_ok;
    return last_ok + 1 - first_ok;
}

// exclusive scan of one value per thread over a workgroup of NW waves; *total = the workgroup's sum
template <uint32_t NW>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *total)
{
    __shared__ uint32_t wave_sum[NW];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)inc, d, 64);
        if (lane >= (uint32_t)d) inc += o;
    }
    if (lane == 63u) wave_sum[w] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
    for (uint32_t k = 0; k < NW; k++) {
        const uint32_t s = wave_sum[k];
        if (k < w) base += s;
        tot += s;
    }
    __syncthreads();                                      // (the next call writes wave_sum again)
    *total = tot;
    return base + inc - v;
}

__device__ __forceinline__ uint32_t wave_or(uint32_t v)
{
    for (int m = 32; m >= 1; m >>= 1) v |= (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_and(uint32_t v)
{
    for (int m = 32; m >= 1; m >>= 1) v &= (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, m, 64);
        v = o > v ? o : v;
    }
    return v;
}

// ---- one stable LSD counting pass over the elements src[0 .. m), PG_EV_BLOCK per workgroup.  digit_of(const T &) yields an
// element's digit, 0 .. 255: of the record itself where the records move, of the record behind it where a permutation does.
// cnt[d * n_blk + b] = elements of block b with digit d
template <class T, class D>
__device__ __forceinline__ void tab_digit_count(const T *src, uint32_t m, uint32_t n_blk, uint32_t *cnt, D digit_of)
{
    __shared__ uint32_t hist[256];
    hist[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    if (i < m) atomicAdd(&hist[digit_of(src[i])], 1u);
    __syncthreads();
    cnt[threadIdx.x * n_blk + blockIdx.x] = hist[threadIdx.x];
}

// cnt scanned: the place of an element = cnt[its digit][its block] + the elements of its block before it with the same digit
template <class T, class D>
__device__ __forceinline__ void tab_scatter(const T *src, T *dst, uint32_t m, uint32_t n_blk, const uint32_t *cnt, D digit_of)
{
    __shared__ uint8_t dig[PG_EV_BLOCK];
    const uint32_t i = blockIdx.x * PG_EV_BLOCK + threadIdx.x;
    T r;
    uint32_t d = 0;
    if (i < m) {
        r = src[i];
        d = digit_of(r);
    }
    dig[threadIdx.x] = (uint8_t)d;
    __syncthreads();
    if (i >= m) return;
    uint32_t before = 0;
    for (uint32_t t = 0; t < threadIdx.x; t++) before += (uint32_t)(dig[t] == (uint8_t)d);
    dst[cnt[d * n_blk + blockIdx.x] + before] = r;
}
