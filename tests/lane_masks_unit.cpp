// Stand-alone check of pindel_amd/csrc/pg_lane_masks.h (host build, run under -fsanitize=address,undefined by
// tests/test_lane_masks_cpu.py): the portable builders of the fold's per-lane masks against the naive definitions, low_bits of
// the clamped argument.  Prints "ok <comparisons>" and returns 0, or the first mismatches and 1.
#include <cstdint>
#include <cstdio>

#include "pg_lane_masks.h"

namespace {

typedef uint64_t u64;
typedef uint32_t u32;

u64 low_bits(int n) { return n >= 64 ? ~0ull : (n <= 0 ? 0ull : ((1ull << n) - 1ull)); }
u32 low32(int n) { return n >= 32 ? 0xffffffffu : (n <= 0 ? 0u : ((1u << n) - 1u)); }

long checked = 0;
int failed = 0;

void expect(u64 got, u64 want, const char *what, int bps, int m, int lane, int r, int b)
{
    checked++;
    if (got == want) return;
    if (failed++ < 20)
        std::printf("%s: bps %d min_perfect %d lane %d round %d block %d: %016llx, naive %016llx\n", what, bps, m, lane, r, b,
                    (unsigned long long)got, (unsigned long long)want);
}

// tier B: every lane, every round and block of NB = 2 and NB = 3; round r, lane l owns L = bps + 64 r + l
void tier_b(int bps, int m)
{
    for (int lane = 0; lane < 64; lane++) {
        const PgFoldMasksB k = pg_fold_masks_b(bps, m, lane);
        for (int nb = 2; nb <= 3; nb++)
            for (int r = 0; r < nb; r++)
                for (int b = 0; b < nb; b++) {
                    const int L = bps + 64 * r + lane;
                    expect(k.mk(r, b), low_bits(L - 64 * b), "mk", bps, m, lane, r, b);
                    expect(k.bp(r, b), low_bits(L - 64 * b) & ~low_bits(L - m - 64 * b), "bp", bps, m, lane, r, b);
                }
    }
}

// tier A: lane 16 q + j owns L = bps + j (the tier is used for bps + 16 <= 32 only)
void tier_a(int bps, int m)
{
    for (int lane = 0; lane < 64; lane++) {
        const PgFoldMasksA k = pg_fold_masks_a(bps, m, lane);
        const int L = bps + (lane & 15);
        expect(k.mk, low32(L), "tier A mk", bps, m, lane, 0, 0);
        expect(k.bpm, low32(L) & ~low32(L - m), "tier A bpm", bps, m, lane, 0, 0);
    }
}

}

int main()
{
    // the dword helpers over and beyond their ranges
    for (int n = -70; n <= 140; n++) {
        expect(pg_lm_low32(n), low32(n), "low32", 0, 0, 0, n, 0);
        if (n < 32) expect(pg_lm_low32_below32(n), low32(n), "low32_below32", 0, 0, 0, n, 0);
        if (n >= 0 && n < 32) expect(pg_lm_low32_exact(n), low32(n), "low32_exact", 0, 0, 0, n, 0);
    }
    // the shipped parameters: the close end's and the far end's first length, Min_Perfect_Match_Around_BP = 3
    tier_b(8, 3);
    tier_b(10, 3);
    tier_a(8, 3);
    tier_a(10, 3);
    // every pair the short form claims
    for (int bps = 1; bps <= 64; bps++)
        for (int m = 0; m <= bps; m++) {
            tier_b(bps, m);
            if (bps + 16 <= 32) tier_a(bps, m);
        }
    if (failed) {
        std::printf("%d of %ld comparisons failed\n", failed, checked);
        return 1;
    }
    std::printf("ok %ld\n", checked);
    return 0;
}
