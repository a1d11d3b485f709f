// Stand-alone host check of the two forms of a candidate's block (pindel_amd/csrc/pg_pass_forms.h): the reference words reversed
// for kind B (pg_pf_block_ref_reversed) against the mismatch word reversed (pg_pf_block_mis_reversed, the planes' bit-reversed copy).
// Random reference and read words; every combination of complement, kind and bases in the block (1, 36, 37, 63, 64 = len - 64 b of
// a second block of 100 / 101 bases and the edges of a word); a read N, a reference N and an "other" character at bit 0, at bit 63
// and inside.  Both outputs, the mismatch word and the exact inequality word, must be equal bit for bit; and the first form is
// checked base by base against Matches() spelled out.  Exit status 0 = every case passed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "pg_pass_forms.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

// base by base: consumed base j of the block against the reference base it meets (F: window bit j, B: window bit 63 - j)
static void by_base(uint64_t rlo, uint64_t rhi, uint64_t rnn, const PgPfPlanes &q, bool comp, bool isB, int bases, uint64_t &m, uint64_t &s)
{
    m = s = 0ull;
    for (int j = 0; j < bases; j++) {
        const int w = isB ? 63 - j : j;
        const unsigned rc = (unsigned)((rlo >> w) & 1u) | ((unsigned)((rhi >> w) & 1u) << 1);
        const bool rn = (rnn >> w) & 1u;
        unsigned qc = (unsigned)((q.lo >> j) & 1u) | ((unsigned)((q.hi >> j) & 1u) << 1);
        if (comp) qc ^= 3u;
        const bool qn = (q.nn >> j) & 1u, qo = (q.oo >> j) & 1u;
        bool mis;
        if (qo || rn) mis = true;                       // an "other" character, or a reference N: matches nothing
        else if (qn) mis = false;                       // a read N matches any of ACGT
        else mis = qc != rc;
        if (mis) m |= 1ull << j;
        if (mis != qn) s |= 1ull << j;                  // the exact inequality: the read's N bits flipped
    }
}

int main()
{
    static const int BASES[] = { 1, 36, 37, 63, 64 };
    static const int SPOTS[] = { 0, 63, 17, 35, 36 };
    long cases = 0, bad = 0;
    for (int it = 0; it < 4000; it++) {
        uint64_t rlo = rnd(), rhi = rnd(), rnn = 0ull;
        PgPfPlanes q;
        q.lo = rnd(); q.hi = rnd(); q.nn = 0ull; q.oo = 0ull;
        // the special characters: none, or at the spots (each independently), or scattered
        const unsigned pick = (unsigned)rnd();
        for (int k = 0; k < 5; k++) {
            if ((pick >> k) & 1u) q.nn |= 1ull << SPOTS[k];
            if ((pick >> (5 + k)) & 1u) rnn |= 1ull << SPOTS[k];
            if ((pick >> (10 + k)) & 1u) q.oo |= 1ull << SPOTS[k];
        }
        if ((pick >> 15) & 1u) { q.nn |= rnd() & rnd() & rnd(); rnn |= rnd() & rnd() & rnd(); q.oo |= rnd() & rnd() & rnd(); }
        q.oo &= ~q.nn;                                  // a character is one or the other
        q.lo &= ~(q.nn | q.oo); q.hi &= ~(q.nn | q.oo); // (the pack kernel leaves their code bits zero)
        const PgPfPlanes qr = pg_pf_reversed(q);
        for (int comp = 0; comp < 2; comp++)
            for (int isB = 0; isB < 2; isB++)
                for (int bases : BASES) {
                    uint64_t m0, s0, m1, s1, m2, s2;
                    pg_pf_block_ref_reversed(rlo, rhi, rnn, q, comp != 0, isB != 0, bases, m0, s0);
                    pg_pf_block_mis_reversed(rlo, rhi, rnn, q, qr, comp != 0, isB != 0, bases, m1, s1);
                    by_base(rlo, rhi, rnn, q, comp != 0, isB != 0, bases, m2, s2);
                    cases++;
                    if (m0 != m1 || s0 != s1 || m0 != m2 || s0 != s2) {
                        if (bad++ < 10)
                            std::printf("MISMATCH it %d comp %d kind %c bases %d: m %016llx %016llx %016llx  s %016llx %016llx %016llx\n", it, comp,
                                        isB ? 'B' : 'F', bases, (unsigned long long)m0, (unsigned long long)m1, (unsigned long long)m2,
                                        (unsigned long long)s0, (unsigned long long)s1, (unsigned long long)s2);
                    }
                }
    }
    // the reversal itself
    for (int i = 0; i < 64; i++)
        if (pg_pf_brev64(1ull << i) != 1ull << (63 - i)) { bad++; std::printf("brev64 bit %d\n", i); }
    std::printf("pass_rev_unit: %ld cases, %ld bad\n", cases, bad);
    return bad ? 1 : 0;
}
