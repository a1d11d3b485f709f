// sv_order_unit.cpp -- the record-shift form of the strict exchange sort (pindel_amd/csrc/pg_sv_order.h) against the literal loop
//     for a < d: if key(x[a]) > key(x[d]) swap(x[a], x[d])
// on every 3-valued sequence of length <= 7, on random sequences of up to 200 elements (few values: long tie classes; chunk seams at
// 64, 65, 128, 129 elements) and on the two examples of DESIGN.md 7n.  Host only; built with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pg_sv_order.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

static long n_cases = 0;
static uint64_t n_skipped = 0;

static void check(const std::vector<uint32_t> &keys)
{
    const uint32_t n = (uint32_t)keys.size();
    std::vector<uint32_t> lit(n), rk(keys), ix(n);
    for (uint32_t i = 0; i < n; i++) lit[i] = ix[i] = i;
    for (uint32_t a = 0; a + 1u < n; a++)
        for (uint32_t d = a + 1u; d < n; d++)
            if (keys[lit[a]] > keys[lit[d]]) std::swap(lit[a], lit[d]);
    PgSvOrderHost sort;
    sort(rk.data(), ix.data(), n);
    n_skipped += sort.skipped;
    for (uint32_t i = 0; i < n; i++)
        if (ix[i] != lit[i] || rk[i] != keys[lit[i]]) {
            std::printf("mismatch at %u of %u:", i, n);
            for (uint32_t k : keys) std::printf(" %u", k);
            std::printf("\n");
            std::exit(1);
        }
    n_cases++;
}

int main()
{
    for (uint32_t len = 0; len <= 7; len++) {
        uint32_t total = 1;
        for (uint32_t i = 0; i < len; i++) total *= 3;
        for (uint32_t code = 0; code < total; code++) {
            std::vector<uint32_t> k(len);
            uint32_t c = code;
            for (uint32_t i = 0; i < len; i++, c /= 3) k[i] = c % 3 * 5;
            check(k);
        }
    }
    const uint32_t seams[] = { 1, 2, 63, 64, 65, 66, 127, 128, 129, 130, 192, 193, 200 };
    for (int it = 0; it < 3000; it++) {
        const uint32_t n = it < 13 * 20 ? seams[it % 13] : 1u + rnd() % 200u;
        const uint32_t values = it % 3 == 0 ? 2u + rnd() % 3u : it % 3 == 1 ? 1u + rnd() % 40u : 0xffffffffu;
        std::vector<uint32_t> k(n);
        for (uint32_t &x : k) x = values == 0xffffffffu ? rnd() : rnd() % values;
        if (it % 7 == 0)                                     // nearly sorted: most passes find no record
            for (uint32_t i = 0; i < n; i++) k[i] = i / 3 + (rnd() % 16 == 0);
        check(k);
    }
    // the tie order depends on history: [5a, 5b, 3] -> 3, 5b, 5a and [5a, 5b, 3, 4] -> 3, 4, 5a, 5b
    {
        uint32_t rk[3] = { 5, 5, 3 }, ix[3] = { 0, 1, 2 };
        PgSvOrderHost()(rk, ix, 3);
        if (ix[0] != 2 || ix[1] != 1 || ix[2] != 0) return 2;
        uint32_t rk4[4] = { 5, 5, 3, 4 }, ix4[4] = { 0, 1, 2, 3 };
        PgSvOrderHost()(rk4, ix4, 4);
        if (ix4[0] != 2 || ix4[1] != 3 || ix4[2] != 0 || ix4[3] != 1) return 3;
        n_cases += 2;
    }
    if (!n_skipped) return 4;                                // the skip of a pass with a minimal front was exercised
    std::printf("ok %ld\n", n_cases);
    return 0;
}
