// pg_variant_dev.h -- device helpers the two classifier kernels share (pg_variant.hip, pg_sv.hip): the reference and the read as
// codes, the points of a run-length-encoded list, the wave-wide minimum and the layout of the ordering key.  HIP only.
#ifndef PG_VARIANT_DEV_H
#define PG_VARIANT_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_device.h"
#include "pg_variant_align.h"

namespace {

// code of the reference base at an AbsLoc (guard words cover the overhang); Outside: the code of a position beyond them
template <uint32_t Outside>
struct DevRefCodeT {
    const uint32_t *lo, *hi, *nn;
    int64_t word0, size;
    __device__ uint32_t operator()(int64_t p) const
    {
        // (a walk ends at the chromosome's own N's, a step reads 63 positions on: inside the guard words.  Nothing is read beyond them.)
        if (p < -(int64_t)(PG_GUARD_WORDS * 32u) || p >= size + (int64_t)(PG_GUARD_WORDS * 32u)) return Outside;
        const int64_t w = word0 + (p >> 5);
        const uint32_t b = (uint32_t)(p & 31);
        if ((nn[w] >> b) & 1u) return (uint32_t)PG_VA_N;
        return ((lo[w] >> b) & 1u) | (((hi[w] >> b) & 1u) << 1);
    }
};
using DevRefCode = DevRefCodeT<(uint32_t)PG_VA_N>;

__device__ __forceinline__ uint32_t base_code(uint8_t ch)
{
    switch (ch) {
    case 'A': return 0u;
    case 'C': return 1u;
    case 'G': return 2u;
    case 'T': return 3u;
    case 'N': return (uint32_t)PG_VA_N;
    default: return (uint32_t)PG_VA_NONE;            // Convert2RC4N leaves NUL
    }
}

// The string NT_str is cut from -- UnmatchedSeq for a '-' anchor, its reverse complement for a '+' anchor -- as codes, read from
// the bytes as uploaded: the post-state is bases [lead, lead + len) of them, reversed and complemented when rc_flag is 1.
struct ReadCode {
    const uint8_t *s;
    int32_t lead, len;
    bool reversed;
    __device__ uint32_t operator()(int32_t j) const
    {
        const uint32_t c = base_code(s[reversed ? lead + len - 1 - j : lead + j]);
        return reversed && c < 4u ? 3u - c : c;
    }
};
struct InsCode {
    ReadCode t;
    int32_t at;
    __device__ uint32_t operator()(uint32_t j) const { return t(at + (int32_t)j); }
};

struct Point { uint32_t abs; int32_t len, mm; bool back; };
// point `idx` of the expanded list of `cnt` runs (idx below the list's number of points)
__device__ __forceinline__ Point point_at(const pg_run *runs, uint32_t cnt, uint32_t idx)
{
    Point p = { 0u, 0, 0, false };
    uint32_t base = 0;
    for (uint32_t k = 0; k < cnt; k++) {
        const pg_run r = runs[k];
        const uint32_t m = (uint32_t)r.len_last - r.len_first + 1u;
        if (idx >= base && idx - base < m) {
            const uint32_t d = idx - base;
            p.back = (r.flags & PG_RUN_BACKWARD) != 0;
            p.abs = p.back ? r.abs_loc_first - d : r.abs_loc_first + d;
            p.len = (int32_t)r.len_first + (int32_t)d;
            p.mm = r.mismatches;
        }
        base += m;
    }
    return p;
}
__device__ __forceinline__ uint32_t points_of(const pg_run *runs, uint32_t cnt)
{
    uint32_t n = 0;
    for (uint32_t k = 0; k < cnt; k++) n += (uint32_t)runs[k].len_last - runs[k].len_first + 1u;
    return n;
}

__device__ __forceinline__ unsigned long long wave_min(unsigned long long v)
{
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(v, m, 64);
        v = o < v ? o : v;
    }
    return v;
}

constexpr unsigned long long NO_KEY = ~0ull;
constexpr int KEY_K_SHIFT = 20, KEY_SUM_SHIFT = 40;
constexpr uint32_t KEY_IDX_MASK = 0xfffffu;

}  // namespace

#endif
