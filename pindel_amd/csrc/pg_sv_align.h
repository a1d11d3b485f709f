// pg_sv_align.h -- the left-alignment walks of the tandem-duplication and inversion classifiers, 64 reference positions per step.
//
// LeftMostTD (src/search_tandem_duplications.cpp:194-222) and LeftMostINV (src/search_inversions.cpp:285-318) move one base per
// iteration.  As in pg_variant_align.h a walk is a predicate "does step t still match" evaluated for 64 consecutive t; the walk
// objects (PgVaHostWalk, PgVaWaveWalk) are the ones of that header.  Shared by the kernel (pg_sv.hip) and by plain host code
// (tests/sv_align_unit.cpp checks it against the host library's one-base loops).
//
// Unlike the deletion and insertion walks these compare WITHOUT an N test: N equals N, and the complement of N is N.  What ends a
// walk is therefore not the spacer's first N but a position whose code equals nothing, itself included: Ref returns PG_SV_OUT for
// a position it does not hold (on the device: outside the guard words), so a walk always ends.
// Ref is a functor code(abs_loc): 0..3 = A C G T, PG_VA_N = N, PG_SV_OUT = no such position.
#ifndef PG_SV_ALIGN_H
#define PG_SV_ALIGN_H

#include "pg_variant_align.h"

enum { PG_SV_OUT = 8 };

// ---- step predicates
// LeftMostTD: chr[pos - t] == chr[end - t]
template <class Ref>
PG_VA_HD inline bool pg_sv_td_left(const Ref &ref, int64_t pos, int64_t end, uint32_t t)
{
    const uint32_t a = ref(pos - (int64_t)t);
    return a == ref(end - (int64_t)t) && a != (uint32_t)PG_SV_OUT;
}
// LeftMostINV: chr[pos + t] == Convert2RC4N[chr[end - t]]
template <class Ref>
PG_VA_HD inline bool pg_sv_inv_in(const Ref &ref, int64_t pos, int64_t end, uint32_t t)
{
    const uint32_t a = ref(pos + (int64_t)t), b = ref(end - (int64_t)t);
    return a == (b < 4u ? 3u - b : b) && a != (uint32_t)PG_SV_OUT;
}

// ---- the two alignments on the values.  bp_left / bp_right / bp are BPLeft / BPRight / BP and come back as the function leaves them;
// n = the length of the padded chromosome string.  true: the out-of-range branch (all three are 1, the read is Used).
template <class Walk, class Ref>
PG_VA_HD inline bool pg_sv_left_most_td(const Walk &walk, const Ref &ref, uint32_t n, uint32_t spacer, uint32_t &bp_left, uint32_t &bp_right,
                                        int16_t &bp)
{
    const uint32_t pos = bp_left + spacer, end = bp_right + spacer - 1u;
    if (pos >= n || end >= n) {
        bp_left = bp_right = 1u;
        bp = 1;
        return true;
    }
    int32_t diff = (int32_t)walk([&](uint32_t t) { return pg_sv_td_left(ref, (int64_t)pos, (int64_t)end, t); });
    if (diff > 0) {
        if (diff >= (int32_t)bp) diff = (int32_t)bp - 1;
        bp_left -= (uint32_t)diff;
        bp_right -= (uint32_t)diff;
        bp = (int16_t)((int32_t)bp - (int32_t)(int16_t)diff);
    }
    return false;
}
// plus: the anchor's strand.  The '+' branch clamps diff and moves nothing, as the reference does.
template <class Walk, class Ref>
PG_VA_HD inline bool pg_sv_left_most_inv(const Walk &walk, const Ref &ref, uint32_t n, uint32_t spacer, bool plus, int16_t read_length,
                                         uint32_t &bp_left, uint32_t &bp_right, int16_t &bp)
{
    const uint32_t pos = bp_left + spacer + 1u, end = bp_right + spacer - 1u;
    if (n <= pos + spacer) {
        bp_left = bp_right = 1u;
        bp = 1;
        return true;
    }
    int16_t diff = (int16_t)walk([&](uint32_t t) { return pg_sv_inv_in(ref, (int64_t)pos, (int64_t)end, t); });
    if (diff > 0 && !plus) {
        if ((int32_t)diff + (int32_t)bp >= (int32_t)read_length) diff = (int16_t)((int32_t)read_length - (int32_t)bp - 1);
        bp_left += (uint32_t)(int32_t)diff;
        bp_right -= (uint32_t)(int32_t)diff;
        bp = (int16_t)((int32_t)bp + (int32_t)diff);
    }
    return false;
}

#endif
