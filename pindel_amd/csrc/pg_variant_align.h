// pg_variant_align.h -- the left-alignment walks of SearchVariant::Search, 64 reference positions per step.
//
// GetRealStart4Deletion (src/pindel.cpp:2095-2118) and GetRealStart4Insertion (:2134-2162) move one base per iteration of a
// while loop; a deletion inside a long repeat walks far.  Here a walk is a predicate "does step t still match" evaluated for 64
// consecutive t at once: the first t that fails is the walk's length.  The predicates and the two alignments built from them are
// shared by the kernel (pg_variant.hip: one lane per t, a ballot per step) and by plain host code (a loop over the 64 t of a
// step: tests/variant_align_unit.cpp checks it against the host library's one-base loops).  No HIP dependency on the host side.
//
// Ref is a functor code(abs_loc): 0..3 = A C G T, PG_VA_N = N; positions are AbsLoc (spacer-padded).  Every walk ends at an N:
// the spacers and, on the device, the guard words around each chromosome; a step reads at most 63 positions past that N.
// Ins is a functor code(j) of the inserted string before any rotation, j in [0, len): 0..3, PG_VA_N, or PG_VA_NONE for a byte
// outside ACGTN (which equals no reference base).
#ifndef PG_VARIANT_ALIGN_H
#define PG_VARIANT_ALIGN_H

#include <stdint.h>

#if defined(__HIPCC__)
#define PG_VA_HD __host__ __device__
#else
#define PG_VA_HD
#endif

enum { PG_VA_N = 4, PG_VA_NONE = 7 };

// ---- step predicates
// GetRealStart4Deletion's first loop: chr[pos - t] == chr[end - t], not N
template <class Ref>
PG_VA_HD inline bool pg_va_del_left(const Ref &ref, int64_t pos, int64_t end, uint32_t t)
{
    const uint32_t a = ref(pos - (int64_t)t);
    return a == ref(end - (int64_t)t) && a != (uint32_t)PG_VA_N;
}
// ... its second loop: chr[pos + t] == chr[start + t], not N
template <class Ref>
PG_VA_HD inline bool pg_va_del_right(const Ref &ref, int64_t pos, int64_t start, uint32_t t)
{
    const uint32_t a = ref(pos + (int64_t)t);
    return a == ref(start + (int64_t)t) && a != (uint32_t)PG_VA_N;
}
// GetRealStart4Insertion's first loop: every match rotates the string left by one, so step t compares chr[at + t] with
// the unrotated string's character t mod len
template <class Ref, class Ins>
PG_VA_HD inline bool pg_va_ins_right(const Ref &ref, const Ins &ins, uint32_t len, int64_t at, uint32_t t)
{
    const uint32_t a = ref(at + (int64_t)t);
    return a == ins(t % len) && a != (uint32_t)PG_VA_N;
}
// ... its second loop, entered after `fwd` left rotations: every match rotates right by one, so step t compares
// chr[from - t] with the unrotated string's character (fwd - 1 - t) mod len
template <class Ref, class Ins>
PG_VA_HD inline bool pg_va_ins_left(const Ref &ref, const Ins &ins, uint32_t len, int64_t from, uint32_t fwd, uint32_t t)
{
    const uint32_t a = ref(from - (int64_t)t);
    int64_t j = ((int64_t)fwd - 1 - (int64_t)t) % (int64_t)len;
    if (j < 0) j += len;
    return a == ins((uint32_t)j) && a != (uint32_t)PG_VA_N;
}

// ---- the walk: match(t) for t = 0, 1, ... -> the first t that fails
// host form: the 64 t of a step in a loop, collected into the mask a wave's ballot would give
struct PgVaHostWalk {
    template <class Pred>
    uint32_t operator()(Pred match) const
    {
        for (uint32_t base = 0;; base += 64u) {
            uint64_t m = 0;
            for (uint32_t lane = 0; lane < 64u; lane++)
                if (match(base + lane)) m |= 1ull << lane;
            if (~m) return base + (uint32_t)__builtin_ctzll(~m);
        }
    }
};
#if defined(__HIPCC__)
// wave form: lane l takes t = base + l (call it with the whole wave active)
struct PgVaWaveWalk {
    uint32_t lane;
    template <class Pred>
    __device__ uint32_t operator()(Pred match) const
    {
        for (uint32_t base = 0;; base += 64u) {
            const uint64_t m = __ballot(match(base + lane));
            if (~m) return base + (uint32_t)__builtin_ctzll(~m);
        }
    }
};
#endif

// ---- the two alignments.  rs / re are BPLeft / BPRight (AbsLoc - spacer) and come back as the loops leave them.
template <class Walk, class Ref>
PG_VA_HD inline void pg_va_real_start_deletion(const Walk &walk, const Ref &ref, uint32_t spacer, uint32_t &rs, uint32_t &re)
{
    const uint32_t pos = rs + spacer, start = pos + 1u, end = re + spacer - 1u;
    const uint32_t left = walk([&](uint32_t t) { return pg_va_del_left(ref, (int64_t)pos, (int64_t)end, t); });
    rs = pos - left - spacer;
    const uint32_t pos2 = re + spacer;
    const uint32_t right = walk([&](uint32_t t) { return pg_va_del_right(ref, (int64_t)pos2, (int64_t)start, t); });
    re = pos2 + right - spacer;
}
// returns the net LEFT rotation of the inserted string (left rotations of the first loop minus right rotations of the second)
template <class Walk, class Ref, class Ins>
PG_VA_HD inline int32_t pg_va_real_start_insertion(const Walk &walk, const Ref &ref, const Ins &ins, uint32_t len, uint32_t spacer,
                                                   uint32_t &rs, uint32_t &re)
{
    const uint32_t at = re + spacer;
    const uint32_t fwd = walk([&](uint32_t t) { return pg_va_ins_right(ref, ins, len, (int64_t)at, t); });
    const uint32_t after = at + fwd;
    re = after - spacer;
    const uint32_t back = walk([&](uint32_t t) { return pg_va_ins_left(ref, ins, len, (int64_t)after - 1, fwd, t); });
    rs = after - 1u - back - spacer;
    return (int32_t)fwd - (int32_t)back;
}

#endif
