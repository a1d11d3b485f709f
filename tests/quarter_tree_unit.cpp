// Stand-alone host check of the two forms of evaluate's quarter merge (pindel_amd/csrc/pg_pass_forms.h): the chain
// ((q0 + q1) + q2) + q3 against the tree (q0 + q1) + (q2 + q3), for qmask 1, 3 and 15.  Every state of the four quarters with levels
// m1 <= m2 out of {0, 1, 2, 3, PG_FS_BIG}, a distinct id per quarter and both verdict words (passed = 0, failed = a nonzero word of
// the quarter's own): 30 states per quarter, 810 000 combinations.  All four outputs -- the two levels, the argmin and its verdict
// word -- must be equal; ties between quarters (equal m1) must go to the leftmost quarter in both.  Exit status 0 = passed.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pg_pass_forms.h"

typedef PgPfQuarter<uint32_t> Q;

int main()
{
    static const uint32_t LV[] = { 0u, 1u, 2u, 3u, PG_FS_BIG };
    std::vector<Q> states[4];
    for (int k = 0; k < 4; k++)
        for (int i = 0; i < 5; i++)
            for (int j = i; j < 5; j++)
                for (int v = 0; v < 2; v++) {
                    Q s;
                    s.m1 = LV[i]; s.m2 = LV[j]; s.id = 0x1000u + (uint32_t)k; s.v = v ? 0x10u << k : 0u;
                    states[k].push_back(s);
                }
    long cases = 0, bad = 0;
    Q q[4];
    for (const Q &a : states[0])
        for (const Q &b : states[1])
            for (const Q &c : states[2])
                for (const Q &d : states[3]) {
                    q[0] = a; q[1] = b; q[2] = c; q[3] = d;
                    static const int MASKS[] = { 1, 3, 15 };
                    for (int qmask : MASKS) {
                        const Q x = pg_pf_quarters_chain<uint32_t>(q, qmask), y = pg_pf_quarters_tree<uint32_t>(q, qmask);
                        cases++;
                        bool ok = x.m1 == y.m1 && x.m2 == y.m2 && x.id == y.id && x.v == y.v;
                        // the leftmost quarter of the lowest level wins, in either form
                        const int nq = qmask == 1 ? 1 : (qmask == 3 ? 2 : 4);
                        int win = 0;
                        for (int k = 1; k < nq; k++)
                            if (q[k].m1 < q[win].m1) win = k;
                        ok = ok && y.m1 == q[win].m1 && y.id == q[win].id && y.v == q[win].v;
                        // the second level: the second smallest of all the levels held
                        uint32_t lo1 = PG_FS_BIG, lo2 = PG_FS_BIG;
                        for (int k = 0; k < nq; k++)
                            for (uint32_t l : { q[k].m1, q[k].m2 }) {
                                if (l < lo1) { lo2 = lo1; lo1 = l; }
                                else if (l < lo2) lo2 = l;
                            }
                        ok = ok && y.m1 == lo1 && y.m2 == lo2;
                        if (!ok && bad++ < 10)
                            std::printf("MISMATCH qmask %d: chain (%u %u %x %x) tree (%u %u %x %x)\n", qmask, x.m1, x.m2, x.id, x.v, y.m1, y.m2,
                                        y.id, y.v);
                    }
                }
    std::printf("quarter_tree_unit: %ld cases, %ld bad\n", cases, bad);
    return bad ? 1 : 0;
}
