// The pure bit arithmetic of the short form of evaluate / emit_runs (pg_kernels.hip; SE, chosen by pg_short_eval).  In round r of an
// evaluation lane l owns the length L = bps + 64 r + l of a read of `len` bases; lengths up to len - 1 are evaluated.
//
// Compiles for the host too (tests/eval_masks_unit.cpp compares each function with the naive definition): everything here is scalar
// code on wave-uniform values, or one shift by the lane index.
#ifndef PG_EVAL_MASKS_H
#define PG_EVAL_MASKS_H
#include <stdint.h>

#if defined(__HIPCC__)
#define PG_EM_FN __host__ __device__ __forceinline__
#else
#define PG_EM_FN static inline
#endif

// the n lowest bits of a lane mask, n clamped to [0, 64]
PG_EM_FN uint64_t pg_em_low64(int n)
{
    return n >= 64 ? ~0ull : (n <= 0 ? 0ull : ((1ull << n) - 1ull));
}

// The lanes of a round that own a valid length, as a mask: lane l is valid iff r0 + l <= len - 1 (r0 = bps + 64 r, the round's first
// length), that is iff l < len - r0.  Wave-uniform: scalar code, and a literal where len and bps are.  (The ballot of the per-lane
// compare "L <= len - 1" is the same mask for an add and a compare per lane and round.)
PG_EM_FN uint64_t pg_em_valid(int len, int r0)
{
    return pg_em_low64(len - r0);
}

// The lanes above lane l, 0 <= l <= 63: ~low_bits(l + 1) = ~1 << l (empty for l = 63: the shift is by less than 64).
PG_EM_FN uint64_t pg_em_above(int lane)
{
    return ~1ull << lane;
}

// "L >= bps + m1" (a point's length reaches past its mismatches) for a lane whose lowest level m1 is at most M, the read's highest
// g_maxMismatch, M < 64.  Round 0: L - bps = lane, the rule is lane >= m1.  Rounds r >= 1: L - bps >= 64 > M >= m1, always true.
// Returns whether round r needs the per-lane compare at all.
PG_EM_FN bool pg_em_reach_needs_compare(int r)
{
    return r == 0;
}
PG_EM_FN bool pg_em_reach(int r, int lane, uint32_t m1)
{
    return pg_em_reach_needs_compare(r) ? (uint32_t)lane >= m1 : true;
}

#endif
