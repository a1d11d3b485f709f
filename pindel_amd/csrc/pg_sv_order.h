// pg_sv_order.h -- the order a STRICT exchange sort leaves, 64 positions per step.
//
// The reporters of DI and of the inversions sort a box with
//     for a < d: if key(x[a]) > key(x[d]) swap(x[a], x[d])
// where equality does not swap.  Its tie order depends on the arrangement it started from and is no stable sort of anything, so
// the loop is kept -- but pass `a` over the arrangement at its start is a closed form:
//     d > a is a RECORD if key(x[d]) < min(key(x[a .. d-1])), strictly;
//     with the records p1 < ... < pk and p0 = a:  x[a] <- x[pk],  x[pj] <- old x[p(j-1)]  for j = 1 .. k;  nothing else moves.
// (x[a] always holds the minimum so far: every swap puts a smaller key there, so exactly the records swap, and each receives what
// the record before it left at the front.)  A pass is therefore an exclusive prefix-min that marks the records and, per record,
// the record before it; positions a+1 .. n-1 go in steps of 64 with the minimum and the last record's old value carried.
// The helpers below are shared by the kernel (pg_sv_events.hip: one lane per position, shuffles and a ballot per step) and by plain
// host code (PgSvOrderHost: the 64 lanes of a step in a loop; tests/sv_order_unit.cpp checks it against the literal loop).
// Keys are u32 ranks (equal rank <=> equal key).  No HIP dependency on the host side.
#ifndef PG_SV_ORDER_H
#define PG_SV_ORDER_H

#include <stdint.h>

#if defined(__HIPCC__)
#define PG_SVO_HD __host__ __device__
#else
#define PG_SVO_HD
#endif

#define PG_SVO_NONE 0xffffffffu      // the key of a lane beyond the box: never a record

// lane's position holds a record: its key lies strictly below the minimum of everything from the front up to the position before
PG_SVO_HD inline bool pg_svo_is_record(uint32_t key, uint32_t min_before, bool valid) { return valid && key < min_before; }
// the lane of the record before `lane` within this step's ballot, or -1: it is the one carried in (the front, or an earlier step's)
PG_SVO_HD inline int pg_svo_pred_lane(uint64_t records, uint32_t lane)
{
    const uint64_t below = records & ((1ull << lane) - 1ull);
    return below ? 63 - __builtin_clzll(below) : -1;
}
// the last record of a step (records != 0): its old value is carried on
PG_SVO_HD inline int pg_svo_last_lane(uint64_t records) { return 63 - __builtin_clzll(records); }

// Host form of the whole sort over ranks rk[0 .. n) with their payload ix[0 .. n), both permuted in place.  A pass whose front
// equals the minimum the last executed pass found is skipped: that minimum bounds everything behind it from below.
struct PgSvOrderHost {
    uint64_t passes = 0, skipped = 0;
    void operator()(uint32_t *rk, uint32_t *ix, uint32_t n)
    {
        bool have_lo = false;
        uint32_t lo = 0;
        for (uint32_t a = 0; a + 1u < n; a++) {
            if (have_lo && rk[a] == lo) {
                skipped++;
                continue;
            }
            passes++;
            uint32_t run_min = rk[a], carry_rk = rk[a], carry_ix = ix[a];
            bool any = false;
            for (uint32_t c0 = a + 1u; c0 < n; c0 += 64u) {
                uint32_t v[64], p[64], excl[64];
                uint32_t m = run_min;
                for (uint32_t lane = 0; lane < 64u; lane++) {
                    const uint32_t d = c0 + lane;
                    v[lane] = d < n ? rk[d] : PG_SVO_NONE;
                    p[lane] = d < n ? ix[d] : 0u;
                    excl[lane] = m;
                    if (v[lane] < m) m = v[lane];
                }
                uint64_t records = 0;
                for (uint32_t lane = 0; lane < 64u; lane++)
                    if (pg_svo_is_record(v[lane], excl[lane], c0 + lane < n)) records |= 1ull << lane;
                for (uint32_t lane = 0; lane < 64u; lane++) {
                    if (!((records >> lane) & 1ull)) continue;
                    const int pl = pg_svo_pred_lane(records, lane);
                    rk[c0 + lane] = pl < 0 ? carry_rk : v[pl];
                    ix[c0 + lane] = pl < 0 ? carry_ix : p[pl];
                }
                if (records) {
                    const int last = pg_svo_last_lane(records);
                    carry_rk = v[last];
                    carry_ix = p[last];
                    any = true;
                }
                run_min = m;
            }
            if (any) {
                rk[a] = carry_rk;
                ix[a] = carry_ix;
            }
            lo = run_min;
            have_lo = true;
        }
    }
};

#endif
