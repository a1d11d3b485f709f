// Stand-alone check of pindel_amd/csrc/pg_eval_masks.h (host build, run under -fsanitize=address,undefined by
// tests/test_eval_masks_cpu.py): the bit arithmetic of the short form of evaluate / emit_runs against the naive definitions, and the
// two equivalences it rests on, by brute force.  Prints "ok <comparisons>" and returns 0, or the first mismatches and 1.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "pg_eval_masks.h"

namespace {

typedef uint64_t u64;
typedef uint32_t u32;

long checked = 0;
int failed = 0;

void expect(u64 got, u64 want, const char *what, int a, int b, int c, int d)
{
    checked++;
    if (got == want) return;
    if (failed++ < 20)
        std::printf("%s (%d, %d, %d, %d): %016llx, naive %016llx\n", what, a, b, c, d, (unsigned long long)got, (unsigned long long)want);
}

// the ballot of a per-lane condition, as the long form takes it
template <typename F> u64 ballot(F f)
{
    u64 m = 0;
    for (int lane = 0; lane < 64; lane++) m |= (u64)(f(lane) ? 1 : 0) << lane;
    return m;
}

// the n lowest bits, bit by bit
u64 low_naive(int n)
{
    u64 m = 0;
    for (int b = 0; b < 64; b++) m |= (u64)(b < n ? 1 : 0) << b;
    return m;
}

// vm: for every bps, len and round (also the rounds evaluate skips because they start past the read: the mask is empty there)
void valid_masks(int bps)
{
    for (int len = 11; len <= 499; len++)
        for (int r = 0; r < 8; r++) {
            const int r0 = bps + 64 * r;
            expect(pg_em_valid(len, r0), ballot([&](int lane) { return r0 + lane <= len - 1; }), "vm", bps, len, r, 0);
        }
}

// The two compares the short form drops, over one round of one read.  mm: a monotone table with mm[L] <= M for L <= len; the round's
// lanes hold any level m1 in [0, 64] or none (0xffff).  The long form's mask of points, without the terms both forms share, is
//     vm & below-the-first-abort & ballot(m1 <= M) & ballot(L >= bps + m1)
// and the short form's   vm & below-the-first-abort [& ballot(lane >= m1) in round 0].
// Every lane is given every level in turn while the lanes below it hold levels that do not abort, so that the lane is reached.
void dropped_compares(int bps, int len, int M, const int *mm)
{
    for (int r = 0; bps + 64 * r <= len - 1; r++) {
        const int r0 = bps + 64 * r;
        const u64 vm = pg_em_valid(len, r0);
        for (int lane : { 0, 1, 2, 3, 4, 7, 8, 31, 32, 62, 63 })
            for (int lvl = 0; lvl <= 65; lvl++) {
                const u32 m1_here = lvl == 65 ? 0xffffu : (u32)lvl;
                auto m1_of = [&](int l) { return l == lane ? m1_here : 0u; };
                auto lo_of = [&](int l) { return m1_of(l) <= (u32)M ? m1_of(l) : (u32)M + 1u; };
                const u64 ab = vm & ballot([&](int l) { return lo_of(l) > (u32)mm[r0 + l]; });
                const u64 below = ~ab & (ab - 1ull);
                const u64 long_form = vm & below & ballot([&](int l) { return m1_of(l) <= (u32)M; }) &
                                      ballot([&](int l) { return (u32)(r0 + l) >= (u32)bps + m1_of(l); });
                const u64 short_form = vm & below & ballot([&](int l) { return pg_em_reach(r, l, m1_of(l)); });
                expect(short_form, long_form, "dropped compares", len, M, r * 64 + lane, lvl);
            }
    }
}

// The same per lane, exhaustively: every bps, len, round, lane, level and M, on the table mm[L] = min(M, L / 4) (monotone, <= M, and
// slow enough that the levels of round 0 run ahead of it).  A valid lane that does not abort is a point of the long form iff it is
// one of the short form.
void dropped_compares_per_lane(int bps)
{
    for (int len = 11; len <= 499; len++)
        for (int r = 0; bps + 64 * r <= len - 1; r++)
            for (int lane = 0; lane < 64; lane++) {
                const int L = bps + 64 * r + lane;
                if (!((pg_em_valid(len, bps + 64 * r) >> lane) & 1ull)) continue;
                long bad = 0;
                for (int M = 0; M <= 31; M++) {
                    const u32 mmL = (u32)(L / 4 < M ? L / 4 : M);
                    for (u32 m1 = 0; m1 <= 64; m1++) {
                        const u32 lo = m1 <= (u32)M ? m1 : (u32)M + 1u;
                        if (lo > mmL) continue;                              // the lane aborts: no point in either form
                        const bool long_form = m1 <= (u32)M && (u32)L >= (u32)bps + m1;
                        bad += long_form != pg_em_reach(r, lane, m1);
                    }
                }
                expect((u64)bad, 0, "dropped compares per lane", bps, len, r, lane);
            }
}

}

int main()
{
    for (int n = -200; n <= 600; n++) expect(pg_em_low64(n), low_naive(n), "low64", n, 0, 0, 0);
    for (int lane = 0; lane < 64; lane++) expect(pg_em_above(lane), ~low_naive(lane + 1), "above", lane, 0, 0, 0);
    valid_masks(8);
    valid_masks(10);
    for (int r = 0; r < 8; r++) expect(pg_em_reach_needs_compare(r), r == 0, "reach needs compare", r, 0, 0, 0);
    dropped_compares_per_lane(8);
    dropped_compares_per_lane(10);
    // the same on whole rounds, first abort included, for a set of lengths and M: monotone tables that reach M at the read's length -- a staircase whose steps are `step` apart
    // (step 1: the table climbs at once, its levels run ahead of the lanes of round 0; large steps: flat over whole rounds)
    static int mm[512 + 128];
    const int lens[] = { 11, 72, 73, 74, 100, 101, 138, 150, 151, 499 };
    const int steps[] = { 1, 16 }, Ms[] = { 0, 1, 2, 3, 7, 31 };
    for (int bps = 8; bps <= 10; bps += 2)
        for (int len : lens)
            for (int M : Ms)
                for (int step : steps) {
                    for (int L = 0; L < 512 + 128; L++) {
                        const int v = L / step;
                        mm[L] = v < M ? v : M;
                    }
                    dropped_compares(bps, len, M, mm);
                }
    if (failed) {
        std::printf("%d of %ld comparisons failed\n", failed, checked);
        return 1;
    }
    std::printf("ok %ld\n", checked);
    return 0;
}
