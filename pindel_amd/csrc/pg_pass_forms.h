// Two bodies every read runs several times, each in its two forms (pg_kernels.hip: the block computation of fold_candidates, the
// quarter merge of evaluate).  Which form a kernel is compiled from is chosen per kernel by pg_rev_mismatch and pg_tree_merge.
//
//   THE BLOCK OF A KIND-B CANDIDATE.  A kind-B candidate consumes the reference downwards: bit j of its block is the base 63 - j of
//   the 64 the window holds at its position.  The first form reverses the three reference words (code bit 0, code bit 1, N) and
//   combines them with the read's planes; the second combines the unreversed words with a bit-reversed copy of the planes and
//   reverses the one word that comes out.  The combination is bitwise, so brev(f(r, q)) == f(brev(r), brev(q)): the same mismatch
//   word either way.  The read's N word and the length mask are applied after the reversal, from the unreversed plane, in both.
//
//   THE MERGE OF THE TIER A QUARTERS.  pg_fs_merge keeps the two smallest levels and the LEFTMOST argmin of its operands in their
//   order; that reduction is associative, so the tree (q0 + q1) + (q2 + q3) gives what the chain ((q0 + q1) + q2) + q3 gives, ties
//   included.  (The order of the operands is kept: the pairing (0, 2), (1, 3) would not do.)
//
// Compiles for the host too: tests/pass_rev_unit.cpp and tests/quarter_tree_unit.cpp run both forms side by side.
#ifndef PG_PASS_FORMS_H
#define PG_PASS_FORMS_H
#include <stdint.h>
#include "pg_fold_step.h"

#define PG_PF_FN PG_FS_FN

PG_PF_FN uint64_t pg_pf_brev64(uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __brevll(v);
#else
    uint64_t r = 0ull;
    for (int i = 0; i < 64; i++) r |= ((v >> i) & 1ull) << (63 - i);
    return r;
#endif
}
PG_PF_FN uint64_t pg_pf_low_bits(int n)              // clamped to [0, 64]
{
    return n >= 64 ? ~0ull : (n <= 0 ? 0ull : ((1ull << n) - 1ull));
}

// The mismatch word of 64 bases (Matches(): a read N matches any of ACGT, a reference N nothing, an "other" character of the read
// nothing): reference words rlo / rhi / rnn against the read's planes qlo / qhi / qnn / qoo, comp = the read is complemented.
PG_PF_FN uint64_t pg_pf_mismatch(uint64_t rlo, uint64_t rhi, uint64_t rnn, uint64_t qlo, uint64_t qhi, uint64_t qnn, uint64_t qoo, bool comp)
{
    const uint64_t cm = comp ? ~0ull : 0ull;
    const uint64_t x = rlo ^ qlo ^ cm;
    const uint64_t y = rhi ^ qhi ^ cm;
    const uint64_t d = x | y;
    return (d & ~qnn) | rnn | qoo;
}
// ... cut to the `bases` the block holds, and the exact inequality word (the mismatch word with the read's N bits flipped)
PG_PF_FN void pg_pf_finish(uint64_t &m, uint64_t &s, uint64_t qnn, int bases)
{
    const uint64_t lm = pg_pf_low_bits(bases);
    m &= lm;
    s = (m ^ qnn) & lm;
}

// The planes of one block: q[0..3] = code bit 0, code bit 1, N, other
struct PgPfPlanes {
    uint64_t lo, hi, nn, oo;
};
PG_PF_FN PgPfPlanes pg_pf_reversed(const PgPfPlanes &q)
{
    PgPfPlanes r;
    r.lo = pg_pf_brev64(q.lo); r.hi = pg_pf_brev64(q.hi); r.nn = pg_pf_brev64(q.nn); r.oo = pg_pf_brev64(q.oo);
    return r;
}
// First form: the reference words of a kind-B candidate are reversed.  (rlo, rhi, rnn: the 64 window bits as fetched.)
PG_PF_FN void pg_pf_block_ref_reversed(uint64_t rlo, uint64_t rhi, uint64_t rnn, const PgPfPlanes &q, bool comp, bool isB, int bases,
                                       uint64_t &m, uint64_t &s)
{
    if (isB) { rlo = pg_pf_brev64(rlo); rhi = pg_pf_brev64(rhi); rnn = pg_pf_brev64(rnn); }
    m = pg_pf_mismatch(rlo, rhi, rnn, q.lo, q.hi, q.nn, q.oo, comp);
    pg_pf_finish(m, s, q.nn, bases);
}
// Second form: a kind-B candidate takes the reversed copy of the planes (qr = pg_pf_reversed(q)), and its mismatch word is reversed.
PG_PF_FN void pg_pf_block_mis_reversed(uint64_t rlo, uint64_t rhi, uint64_t rnn, const PgPfPlanes &q, const PgPfPlanes &qr, bool comp,
                                       bool isB, int bases, uint64_t &m, uint64_t &s)
{
    const PgPfPlanes &u = isB ? qr : q;
    m = pg_pf_mismatch(rlo, rhi, rnn, u.lo, u.hi, u.nn, u.oo, comp);
    if (isB) m = pg_pf_brev64(m);
    pg_pf_finish(m, s, q.nn, bases);
}

// The state of one tier A quarter at one length: the two smallest levels, the argmin and its verdict word
template <typename Id>
struct PgPfQuarter {
    uint32_t m1, m2;
    Id id;
    uint32_t v;
};
template <typename Id>
PG_PF_FN void pg_pf_merge(PgPfQuarter<Id> &a, const PgPfQuarter<Id> &b)
{
    pg_fs_merge<Id>(a.m1, a.m2, a.id, a.v, b.m1, b.m2, b.id, b.v);
}
// qmask: the quarters that belong to the state -- 1, 3 or 15 (evaluate)
template <typename Id>
PG_PF_FN PgPfQuarter<Id> pg_pf_quarters_chain(const PgPfQuarter<Id> *q, int qmask)
{
    PgPfQuarter<Id> a = q[0];
    for (int k = 1; k < 4; k++)
        if ((qmask >> k) & 1) pg_pf_merge<Id>(a, q[k]);
    return a;
}
// The tree as evaluate runs it: step 1 in quarters 0 and 2 at once (each takes its upper neighbour), step 2 brings quarter 2's
// result to quarter 0; qmask = 3 ends after step 1.
template <typename Id>
PG_PF_FN PgPfQuarter<Id> pg_pf_quarters_tree(const PgPfQuarter<Id> *q, int qmask)
{
    PgPfQuarter<Id> a = q[0], c = q[2];
    if (qmask == 1) return a;
    pg_pf_merge<Id>(a, q[1]);
    pg_pf_merge<Id>(c, q[3]);
    if (qmask == 15) pg_pf_merge<Id>(a, c);
    return a;
}

#endif
