// Per-lane masks of the fold (pg_kernels.hip: fold_tier_b, tier A of fold_candidates), built from the lane's index and the two
// parameters bps (the first evaluated length) and min_perfect (CheckMismatches' window) alone.  The kernels whose parameters are
// literals rebuild them in every call -- no register is free to keep them -- so what counts is how few instructions that takes.
//
// The cheap forms rest on 0 <= min_perfect <= bps: the window of min_perfect bases that ends at the lane's length L then starts
// at L - min_perfect >= 0, so "the bases before the window" is "the bases before L", shifted down by min_perfect:
//     low(L - m) = low(L) >> m        and the window        [L - m, L) = low(L) & ~(low(L) >> m)
// over as many bits as L can reach, with no second set of clamps.
//
// Compiles for the host too (tests/lane_masks_unit.cpp compares every builder with the naive definition): the device side
// uses v_med3 / v_bfm, the host side plain C++ with the same meaning.
#ifndef PG_LANE_MASKS_H
#define PG_LANE_MASKS_H
#include <stdint.h>

#if defined(__HIPCC__)
#define PG_LM_FN __host__ __device__ __forceinline__
#define PG_LM_MEMBER __host__ __device__ __forceinline__
#else
#define PG_LM_FN static inline
#define PG_LM_MEMBER inline
#endif

// the n lowest bits of a dword, n clamped to [0, 32]
PG_LM_FN uint32_t pg_lm_low32(int n)
{
#if defined(__HIP_DEVICE_COMPILE__)
    int t, f;
    asm("v_med3_i32 %0, %1, 0, 32" : "=v"(t) : "v"(n));
    uint32_t m;
    asm("v_bfm_b32 %0, %1, 0" : "=v"(m) : "v"(t));          // (width t & 31: 0 for t = 32)
    asm("v_bfe_i32 %0, %1, 5, 1" : "=v"(f) : "v"(t));      // -1 for t = 32
    return m | (uint32_t)f;
#else
    return n >= 32 ? 0xffffffffu : (n <= 0 ? 0u : ((1u << n) - 1u));
#endif
}
// ... for n < 32 (clamped below only): no width-32 case
PG_LM_FN uint32_t pg_lm_low32_below32(int n)
{
#if defined(__HIP_DEVICE_COMPILE__)
    int t;
    asm("v_max_i32 %0, 0, %1" : "=v"(t) : "v"(n));
    uint32_t m;
    asm("v_bfm_b32 %0, %1, 0" : "=v"(m) : "v"(t));
    return m;
#else
    return n <= 0 ? 0u : ((1u << n) - 1u);
#endif
}
// ... for 0 <= n < 32: the bit-field mask alone
PG_LM_FN uint32_t pg_lm_low32_exact(int n)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t m;
    asm("v_bfm_b32 %0, %1, 0" : "=v"(m) : "v"(n));
    return m;
#else
    return (1u << n) - 1u;
#endif
}

// Tier B.  In round r the lane owns L = bps + 64 r + lane; of block b (bases [64 b, 64 b + 64) of the read) it needs
//     mk(r, b) = the bases consumed at length L          = low64(L - 64 b)
//     bp(r, b) = CheckMismatches' window [L - m, L)      = low64(L - 64 b) & ~low64(L - m - 64 b)
// Both depend on b - r only, and only b = r and b = r + 1 are neither empty nor full: four masks serve every round.
struct PgFoldMasksB {
    uint64_t w0, w1;         // mk for b = r, b = r + 1
    uint64_t bp0, bp1;       // bp for b = r, b = r + 1
    PG_LM_MEMBER uint64_t mk(int r, int b) const { return b < r ? ~0ull : (b == r ? w0 : (b == r + 1 ? w1 : 0ull)); }
    PG_LM_MEMBER uint64_t bp(int r, int b) const { return b == r ? bp0 : (b == r + 1 ? bp1 : 0ull); }
};
// requires 1 <= bps <= 64 and 0 <= min_perfect <= bps (with literals the tests below fold away)
PG_LM_FN PgFoldMasksB pg_fold_masks_b(int bps, int min_perfect, int lane)
{
    // the base mask low128(n0), n0 = bps + lane in [1, 127], as dwords; n0 >= 1: dword 0 needs no lower clamp, but the
    // clamp of v_med3 is free.  Dword 2 reaches width 32 only for bps >= 33, dword 3 is empty below that.
    const int n0 = bps + lane;
    const uint32_t d0 = pg_lm_low32(n0), d1 = pg_lm_low32(n0 - 32);
    const uint32_t d2 = bps + 63 - 64 < 32 ? pg_lm_low32_below32(n0 - 64) : pg_lm_low32(n0 - 64);
    const uint32_t d3 = bps + 63 - 96 <= 0 ? 0u : pg_lm_low32_below32(n0 - 96);
    PgFoldMasksB k;
    k.w0 = (uint64_t)d0 | ((uint64_t)d1 << 32);
    k.w1 = (uint64_t)d2 | ((uint64_t)d3 << 32);
    // low128(n0 - m) = low128(n0) >> m
    const int m = min_perfect;
    const uint64_t p0 = m == 0 ? k.w0 : (m == 64 ? k.w1 : ((k.w0 >> m) | (k.w1 << (64 - m))));
    const uint64_t p1 = m == 64 ? 0ull : (k.w1 >> m);
    k.bp0 = k.w0 & ~p0;
    k.bp1 = k.w1 & ~p1;
    return k;
}

// Tier A.  Lane 16 q + j owns L = bps + j; the tier is used only when bps + 16 <= 32 and min_perfect < bps, so 1 <= L <= 31:
//     mk  = low32(L)                     the bases consumed at length L
//     bpm = mk & ~(mk >> min_perfect)    CheckMismatches' window [L - m, L)
struct PgFoldMasksA {
    uint32_t mk, bpm;
};
// requires 1 <= bps <= 16 and 0 <= min_perfect <= bps
PG_LM_FN PgFoldMasksA pg_fold_masks_a(int bps, int min_perfect, int lane)
{
    PgFoldMasksA k;
    k.mk = pg_lm_low32_exact(bps + (lane & 15));
    k.bpm = k.mk & ~(k.mk >> min_perfect);
    return k;
}

#endif
