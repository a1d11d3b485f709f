// The per-candidate step of the fold (pg_kernels.hip: tier A of fold_candidates, fold_tier_b, the quarter merge of evaluate, AccB),
// in its two forms.  Every step takes a candidate's level k, its id and a VERDICT WORD and keeps (min1, min2, argmin) and the verdict
// word of the argmin.  What the word is, is the form (SF, chosen per kernel by pg_short_fold):
//
//   long form  (SF = false)   ok:  1 iff CheckMismatches passed, 0 otherwise and in the empty state.  Every step turns the bits that
//                             decide it (the inequality bits inside the window of min_perfect bases, the whole-read Hamming verdict)
//                             into 0 / 1 with a compare and a select, or a 64-bit compare, a shift and a select.
//   short form (SF = true)    nok: the bits that make CheckMismatches FAIL, ORed together: 0 iff it passed, anything else otherwise
//                             and in the empty state.  The step is one AND (tier A) or one three-way OR (tier B): the only question
//                             ever asked of the word is "is it zero", once, in evaluate's ballot.  The Hamming verdict travels as bits
//                             too: a candidate whose count fails has every inequality bit of its tier A entry set (the window is never
//                             empty: pg_fs_window_never_empty), and ~0 in the word of its tier B header that the long form uses for
//                             the id's high half and the flags.  So the short form needs 32-bit ids and min_perfect < bps (no
//                             "L > min_perfect" test: pg_kernels.hip, Search::len_check).
//
// The selections are the same in both forms -- the same strict `<`, the same tie rule -- so (min1, min2, argmin) are the same bit for
// bit and ok == (nok == 0) after every step.  Compiles for the host too: tests/fold_step_unit.cpp runs both forms side by side.
#ifndef PG_FOLD_STEP_H
#define PG_FOLD_STEP_H
#include <stdint.h>

#if defined(__HIPCC__)
#define PG_FS_FN __host__ __device__ __forceinline__
#else
#define PG_FS_FN static inline
#endif

#define PG_FS_BIG 0xffffu          // "no candidate" level (PG_BIG)

PG_FS_FN uint32_t pg_fs_med3(uint32_t a, uint32_t b, uint32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t r;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
#else
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    return c < lo ? lo : (c > hi ? hi : c);
#endif
}

// the verdict word of the empty state, and the one question asked of a verdict word
template <bool SF> PG_FS_FN uint32_t pg_fs_none() { return SF ? 1u : 0u; }
template <bool SF> PG_FS_FN bool pg_fs_passed(uint32_t v) { return SF ? v == 0u : v != 0u; }

// The window [L - m, L) of a length L >= bps is never empty when 1 <= m <= bps: what lets a set of inequality bits stand for a failed
// Hamming verdict in tier A.
constexpr bool pg_fs_window_never_empty(int bps, int min_perfect) { return min_perfect >= 1 && min_perfect <= bps; }

// fold one candidate (level k, id cid, verdict word vc) into (min1, min2, argmin, its verdict word)
template <typename Id>
PG_FS_FN void pg_fs_fold(uint32_t &m1, uint32_t &m2, Id &id, uint32_t &v, uint32_t k, Id cid, uint32_t vc)
{
    const bool lt = k < m1;
    m2 = pg_fs_med3(m1, m2, k);     // second smallest of {m1 <= m2, k}
    id = lt ? cid : id;
    v = lt ? vc : v;
    m1 = k < m1 ? k : m1;
}
// merge two partial reductions (a <- a + b)
template <typename Id>
PG_FS_FN void pg_fs_merge(uint32_t &a1, uint32_t &a2, Id &aid, uint32_t &av, uint32_t b1, uint32_t b2, Id bid, uint32_t bv)
{
    const bool lt = b1 < a1;
    const uint32_t hi1 = a1 > b1 ? a1 : b1, lo2 = a2 < b2 ? a2 : b2;
    a2 = hi1 < lo2 ? hi1 : lo2;
    aid = lt ? bid : aid;
    av = lt ? bv : av;
    a1 = lt ? b1 : a1;
}

// TIER A.  An entry is {mismatch bits, inequality bits, id, w}; a lane holds mk = the bases [0, L) and bpm = the window [L - m, L).
// The inequality word as the candidate pass writes it, hamok = the whole-read Hamming verdict (nonzero: passed) ...
template <bool SF> PG_FS_FN uint32_t pg_fs_entry_a_y(uint32_t sne, uint32_t hamok)
{
    return SF ? (hamok ? sne : ~0u) : sne;
}
// ... the entry's last word: the long form's id high half | length bound | Hamming verdict in bit 31 (`meta`), nothing in the short one
template <bool SF> PG_FS_FN uint32_t pg_fs_entry_a_w(uint32_t meta) { return SF ? 0u : meta; }
// ... and the verdict word of the entry at the lane's length
template <bool SF> PG_FS_FN uint32_t pg_fs_verdict_a(uint32_t ey, uint32_t ew, uint32_t bpm)
{
    return SF ? (ey & bpm) : ((ey & bpm) == 0u ? (ew >> 31) : 0u);
}
// the level of the entry at the lane's length
PG_FS_FN uint32_t pg_fs_level_a(uint32_t ex, uint32_t mk)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popc(ex & mk);
#else
    return (uint32_t)__builtin_popcount(ex & mk);
#endif
}

// TIER B.  bad = the inequality bits inside the window over the blocks the lane reads; hy = the second word of the candidate's header:
// `meta` in the long form, 0 / ~0 for a passed / failed Hamming verdict in the short one.
template <bool SF> PG_FS_FN uint32_t pg_fs_hdr_b_y(uint32_t meta, uint32_t hamok)
{
    return SF ? (hamok ? 0u : ~0u) : meta;
}
template <bool SF> PG_FS_FN uint32_t pg_fs_verdict_b(uint64_t bad, uint32_t hy)
{
    return SF ? ((uint32_t)bad | (uint32_t)(bad >> 32) | hy) : (bad == 0ull ? (hy >> 31) : 0u);
}

// The state of one length of the rounds >= 1 with 32-bit ids, first word (AccB<u32>): m1 | min(m2, 0x7fff) << 16 | bit 31, which is
// "passed" in the long form and "failed" in the short one.  Levels are mismatch counts <= the read length; PG_FS_BIG only means
// "none", and comes back as 0x7fff in m2: above every level either way.
template <bool SF> PG_FS_FN uint32_t pg_fs_accb_pack(uint32_t m1, uint32_t m2, uint32_t v)
{
    const uint32_t c2 = m2 < 0x7fffu ? m2 : 0x7fffu;
    return m1 | (c2 << 16) | ((SF ? (v != 0u ? 1u : 0u) : v) << 31);
}
PG_FS_FN void pg_fs_accb_unpack(uint32_t x, uint32_t &m1, uint32_t &m2, uint32_t &v)
{
    m1 = x & 0xffffu; m2 = (x >> 16) & 0x7fffu; v = x >> 31;
}

#endif
