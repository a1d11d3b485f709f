// Stand-alone check of pindel_amd/csrc/pg_fold_step.h (host build, run under -fsanitize=address,undefined by
// tests/test_fold_step_cpu.py): the fold's per-candidate step in its short form (the reduction carries the bits that make
// CheckMismatches fail) against the definitions the kernels had before the header existed (a 0 / 1 verdict), written out below.
// After every step, every merge and every AccB round trip: the same (m1, m2, id), and ok == (nok == 0).  The header's long form is
// held against the same definitions.  Prints "ok <comparisons>" and returns 0, or the first mismatches and 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pg_fold_step.h"
#include "pg_lane_masks.h"

namespace {

typedef uint64_t u64;
typedef uint32_t u32;

const u32 BIG = 0xffffu;
long checked = 0;
int failed = 0;

u64 rng_state = 0x9e3779b97f4a7c15ull;
u32 rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (u32)(rng_state >> 16);
}

// ---- the definitions before the header
u32 old_med3(u32 a, u32 b, u32 c)
{
    const u32 lo = a < b ? a : b, hi = a < b ? b : a;
    return c < lo ? lo : (c > hi ? hi : c);
}
struct St { u32 m1, m2, id, v; };
void old_fold(St &s, u32 k, u32 cid, u32 okc)
{
    const bool lt = k < s.m1;
    s.m2 = old_med3(s.m1, s.m2, k);
    s.id = lt ? cid : s.id;
    s.v = lt ? okc : s.v;
    s.m1 = k < s.m1 ? k : s.m1;
}
void old_merge(St &a, const St &b)
{
    const bool lt = b.m1 < a.m1;
    const u32 hi1 = a.m1 > b.m1 ? a.m1 : b.m1, lo2 = a.m2 < b.m2 ? a.m2 : b.m2;
    a.m2 = hi1 < lo2 ? hi1 : lo2;
    a.id = lt ? b.id : a.id;
    a.v = lt ? b.v : a.v;
    a.m1 = lt ? b.m1 : a.m1;
}
u32 old_accb_pack(u32 m1, u32 m2, u32 ok)
{
    const u32 c2 = m2 < 0x7fffu ? m2 : 0x7fffu;
    return m1 | (c2 << 16) | (ok << 31);
}
void old_accb_unpack(u32 x, u32 &m1, u32 &m2, u32 &ok) { m1 = x & 0xffffu; m2 = (x >> 16) & 0x7fffu; ok = x >> 31; }

// ---- the header's steps on a state, in the form SF
template <bool SF> St none() { return St{ BIG, BIG, 0u, pg_fs_none<SF>() }; }
void new_fold(St &s, u32 k, u32 cid, u32 vc) { pg_fs_fold<u32>(s.m1, s.m2, s.id, s.v, k, cid, vc); }
void new_merge(St &a, const St &b) { pg_fs_merge<u32>(a.m1, a.m2, a.id, a.v, b.m1, b.m2, b.id, b.v); }

void same(const St &o, const St &l, const St &s, const char *what, int x, int y)
{
    checked++;
    const bool good = o.m1 == l.m1 && o.m2 == l.m2 && o.id == l.id && o.v == l.v &&                  // the header's long form
                      o.m1 == s.m1 && o.m2 == s.m2 && o.id == s.id && (o.v != 0u) == (s.v == 0u) &&  // the short form
                      o.v <= 1u && pg_fs_passed<false>(l.v) == pg_fs_passed<true>(s.v);
    if (good) return;
    if (failed++ < 20)
        std::printf("%s (%d, %d): before (%u %u %u ok %u), long form (%u %u %u ok %u), short form (%u %u %u nok %08x)\n", what, x, y,
                    o.m1, o.m2, o.id, o.v, l.m1, l.m2, l.id, l.v, s.m1, s.m2, s.id, s.v);
}

// a candidate: the low mismatch and inequality words of block 0, its whole-read Hamming verdict, the inequality bits of its tier B
// window (as fold_tier_b gathers them at some length), its id
struct Cand { u32 mis, sne, hamok, id; u64 bad; u32 forced; };    // forced: a level to use in place of popcount (BIG = none)

// one lane of tier A: the three states after every candidate of a list
struct Lane3 {
    St o = none<false>(), l = none<false>(), s = none<true>();
};
void tier_a_step(Lane3 &t, const Cand &c, u32 mk, u32 bpm, bool valid)
{
    const u32 meta = (c.hamok ? 0x80000000u : 0u) | (4u << 24);
    u32 k = c.forced != BIG + 1u ? c.forced : (u32)__builtin_popcount(c.mis & mk);
    if (!valid) k = BIG;
    old_fold(t.o, k, c.id, (c.sne & bpm) == 0u ? (meta >> 31) : 0u);
    const u32 kn = c.forced != BIG + 1u ? (valid ? c.forced : BIG) : (valid ? pg_fs_level_a(c.mis, mk) : BIG);
    new_fold(t.l, kn, c.id, pg_fs_verdict_a<false>(pg_fs_entry_a_y<false>(c.sne, c.hamok), pg_fs_entry_a_w<false>(meta), bpm));
    new_fold(t.s, kn, c.id, pg_fs_verdict_a<true>(pg_fs_entry_a_y<true>(c.sne, c.hamok), pg_fs_entry_a_w<true>(meta), bpm));
}
void tier_b_step(Lane3 &t, const Cand &c, u32 k)
{
    const u32 meta = (c.hamok ? 0x80000000u : 0u) | (3u << 24);
    old_fold(t.o, k, c.id, c.bad == 0ull ? (meta >> 31) : 0u);
    new_fold(t.l, k, c.id, pg_fs_verdict_b<false>(c.bad, pg_fs_hdr_b_y<false>(meta, c.hamok)));
    new_fold(t.s, k, c.id, pg_fs_verdict_b<true>(c.bad, pg_fs_hdr_b_y<true>(meta, c.hamok)));
}
void merge3(Lane3 &a, const Lane3 &b)
{
    old_merge(a.o, b.o); new_merge(a.l, b.l); new_merge(a.s, b.s);
}
void accb_round_trip(Lane3 &t, int x, int y)
{
    u32 m1, m2, v;
    old_accb_unpack(old_accb_pack(t.o.m1, t.o.m2, t.o.v), m1, m2, v);
    t.o.m1 = m1; t.o.m2 = m2; t.o.v = v;
    pg_fs_accb_unpack(pg_fs_accb_pack<false>(t.l.m1, t.l.m2, t.l.v), m1, m2, v);
    t.l.m1 = m1; t.l.m2 = m2; t.l.v = v;
    pg_fs_accb_unpack(pg_fs_accb_pack<true>(t.s.m1, t.s.m2, t.s.v), m1, m2, v);
    t.s.m1 = m1; t.s.m2 = m2; t.s.v = v;
    same(t.o, t.l, t.s, "AccB round trip", x, y);
}

Cand random_cand(u32 id, int kind)
{
    Cand c;
    c.id = id;
    c.forced = BIG + 1u;
    c.mis = rnd() & rnd() & rnd();                   // a few mismatches
    c.sne = c.mis ^ (rnd() & rnd() & rnd() & rnd()); // the read's N bits flipped
    c.hamok = rnd() & 1u;
    c.bad = (rnd() & 3u) ? 0ull : ((u64)rnd() << 32 | rnd()) & ((u64)rnd() << 32 | rnd());
    switch (kind) {
    case 1: c.hamok = 0u; c.sne = 0u; c.bad = 0ull; break;                     // a clean window, the Hamming count fails
    case 2: c.hamok = 1u; c.sne |= 0x00ffff00u; c.bad |= 1ull << (rnd() & 63u); break;   // a dirty window, the count passes
    case 3: c.mis = 0u; break;                                                 // level 0: ties with its like
    case 4: c.forced = BIG; break;                                             // a level at PG_BIG
    case 5: c.forced = 0x7fffu + (rnd() % 3u) - 1u; break;                     // around AccB's clip of m2
    case 6: c.hamok = 1u; c.sne = 0u; c.bad = 0ull; break;                     // passes
    case 7: c.bad = 0x80000000ull << (rnd() & 32u); break;                     // one bit, in either half
    default: break;
    }
    return c;
}

// tier A of one pass as the kernels walk it: the list in bufA, quarter q takes every fourth entry from q.  `before`: every
// iteration tests idx < nA and clamps the index; `after`: nA >> 2 iterations without a test, then one with it.  The four quarters
// are merged in order, as evaluate does.
void tier_a_walk(const std::vector<Cand> &list, int bps, int j)
{
    const int nA = (int)list.size();
    const PgFoldMasksA k = pg_fold_masks_a(bps, 3, j);
    Lane3 q_before[4], q_after[4];
    std::vector<Cand> buf(68, random_cand(999u, 0));
    for (int i = 0; i < nA; i++) buf[i] = list[i];
    for (int q = 0; q < 4; q++) {
        int idx = q;
        for (int it = 0; it < (nA + 3) >> 2; it++, idx += 4) tier_a_step(q_before[q], buf[idx < 67 ? idx : 67], k.mk, k.bpm, idx < nA);
        u32 at = 16u * (u32)q;
        for (int it = 0; it < nA >> 2; it++, at += 64u) tier_a_step(q_after[q], buf[at / 16u], k.mk, k.bpm, true);
        if (nA & 3) {
            if (at / 16u >= 68u) { std::printf("tier A walk: entry %u read\n", at / 16u); failed++; return; }
            tier_a_step(q_after[q], buf[at / 16u], k.mk, k.bpm, at < 16u * (u32)nA);
        }
        same(q_before[q].o, q_after[q].l, q_after[q].s, "tier A walk, a quarter", nA, q);
    }
    Lane3 t = q_after[0];
    St o = q_before[0].o;
    for (int q = 1; q < 4; q++) {
        merge3(t, q_after[q]);
        old_merge(o, q_before[q].o);
        same(o, t.l, t.s, "tier A walk, the merge", nA, q);
    }
}

}

int main()
{
    // the window of CheckMismatches is never empty: every lane of tier A at both ends, every lane and round of tier B
    for (int bps : { 8, 10 }) {
        static_assert(pg_fs_window_never_empty(8, 3) && pg_fs_window_never_empty(10, 3) && !pg_fs_window_never_empty(8, 0) &&
                      !pg_fs_window_never_empty(3, 4), "the header's condition");
        for (int lane = 0; lane < 64; lane++) {
            checked++;
            if (pg_fold_masks_a(bps, 3, lane).bpm == 0u) { std::printf("tier A: empty window, bps %d lane %d\n", bps, lane); failed++; }
            const PgFoldMasksB b = pg_fold_masks_b(bps, 3, lane);
            checked++;
            if ((b.bp0 | b.bp1) == 0ull) { std::printf("tier B: empty window, bps %d lane %d\n", bps, lane); failed++; }
        }
    }
    // the empty state
    {
        Lane3 t;
        same(t.o, t.l, t.s, "empty state", 0, 0);
        accb_round_trip(t, 0, 0);
    }
    // random and adversarial streams through one lane of tier A (every length of both ends) and of tier B; an AccB round trip and a
    // merge with another stream's state after every candidate
    for (int round = 0; round < 400; round++) {
        const int bps = (round & 1) ? 8 : 10, j = (round >> 1) & 15;
        const PgFoldMasksA k = pg_fold_masks_a(bps, 3, j);
        const int bias = round % 9;                      // 8: anything
        Lane3 a, b, other;
        for (int i = 0; i < 40; i++) {
            const Cand c = random_cand(1u + (u32)i, (rnd() & 1u) ? bias : (int)(rnd() % 9u));
            tier_a_step(a, c, k.mk, k.bpm, (rnd() & 7u) != 0u);
            same(a.o, a.l, a.s, "tier A step", round, i);
            const u32 kb = c.forced != BIG + 1u ? c.forced : (u32)__builtin_popcount(c.mis) + (rnd() & 1u);
            tier_b_step(b, c, kb);
            same(b.o, b.l, b.s, "tier B step", round, i);
            Lane3 st = b;                                // (a copy: the state in registers stays exact, AccB clips m2)
            accb_round_trip(st, round, i);
            const u32 kn = kb + (rnd() % 3u) - 1u + (kb == 0u);
            tier_b_step(st, random_cand(100u + (u32)i, (int)(rnd() % 9u)), kn < BIG ? kn : BIG);
            same(st.o, st.l, st.s, "tier B step after AccB", round, i);
            tier_a_step(other, random_cand(200u + (u32)i, (int)(rnd() % 9u)), k.mk, k.bpm, true);
            Lane3 m = a;
            merge3(m, other);
            same(m.o, m.l, m.s, "merge", round, i);
            Lane3 m2 = other;
            merge3(m2, b);
            same(m2.o, m2.l, m2.s, "merge, the other way", round, i);
        }
    }
    // ties in every quarter order: four candidates of equal level (level 0) with the verdicts of all sixteen patterns, one per
    // quarter, in each of the 24 orders; then the passes of every size 0 .. 64 as the kernels walk them
    {
        const int perm[24][4] = { { 0, 1, 2, 3 }, { 0, 1, 3, 2 }, { 0, 2, 1, 3 }, { 0, 2, 3, 1 }, { 0, 3, 1, 2 }, { 0, 3, 2, 1 },
                                  { 1, 0, 2, 3 }, { 1, 0, 3, 2 }, { 1, 2, 0, 3 }, { 1, 2, 3, 0 }, { 1, 3, 0, 2 }, { 1, 3, 2, 0 },
                                  { 2, 0, 1, 3 }, { 2, 0, 3, 1 }, { 2, 1, 0, 3 }, { 2, 1, 3, 0 }, { 2, 3, 0, 1 }, { 2, 3, 1, 0 },
                                  { 3, 0, 1, 2 }, { 3, 0, 2, 1 }, { 3, 1, 0, 2 }, { 3, 1, 2, 0 }, { 3, 2, 0, 1 }, { 3, 2, 1, 0 } };
        for (int p = 0; p < 24; p++)
            for (int pat = 0; pat < 16; pat++)
                for (int lvl = 0; lvl < 2; lvl++) {
                    std::vector<Cand> list(4);
                    for (int q = 0; q < 4; q++) {
                        Cand c = random_cand(10u + (u32)q, ((pat >> q) & 1) ? 6 : ((q & 1) ? 1 : 2));
                        c.mis = lvl && q == perm[p][3] ? 1u : 0u;          // (lvl 1: one of the four is a level higher)
                        list[perm[p][q]] = c;
                    }
                    tier_a_walk(list, 8, p & 15);
                }
        for (int nA = 0; nA <= 64; nA++)
            for (int rep = 0; rep < 4; rep++) {
                std::vector<Cand> list;
                for (int i = 0; i < nA; i++) list.push_back(random_cand(1u + (u32)i, rep == 0 ? 3 : (int)(rnd() % 9u)));
                tier_a_walk(list, rep & 1 ? 8 : 10, (nA + rep) & 15);
            }
    }
    // AccB on its own: every combination of the edge levels
    {
        const u32 lv[] = { 0u, 1u, 100u, 0x7ffeu, 0x7fffu, 0x8000u, BIG };
        for (u32 m1 : lv)
            for (u32 m2 : lv) {
                if (m2 < m1 || (m1 > 300u && m1 != BIG)) continue;        // (levels are mismatch counts or PG_BIG, m1 <= m2)
                for (u32 ok = 0u; ok < 2u; ok++)
                    for (u32 nok : { 0u, 1u, 0x80000000u, 0xffffffffu, 4u }) {
                        if ((nok == 0u) != (ok != 0u)) continue;
                        Lane3 t;
                        t.o = St{ m1, m2, 7u, ok }; t.l = t.o; t.s = St{ m1, m2, 7u, nok };
                        accb_round_trip(t, (int)m1, (int)m2);
                        checked++;
                        if (pg_fs_accb_pack<false>(m1, m2, ok) != old_accb_pack(m1, m2, ok) ||
                            (pg_fs_accb_pack<true>(m1, m2, nok) ^ old_accb_pack(m1, m2, ok)) != 0x80000000u) {
                            if (failed++ < 20) std::printf("AccB word: m1 %u m2 %u ok %u nok %08x\n", m1, m2, ok, nok);
                        }
                    }
            }
    }
    if (failed) {
        std::printf("%d of %ld comparisons failed\n", failed, checked);
        return 1;
    }
    std::printf("ok %ld\n", checked);
    return 0;
}
