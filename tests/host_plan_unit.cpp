// Stand-alone check of pindel_amd/csrc/pg_host_plan.h (plain g++, address + undefined-behaviour sanitizers, no GPU): the chunk
// schedule, the one-block layout, the delivery's arena requests and the one-copy input layout.  Prints "ok <cases>" and exits 0,
// or says what failed and exits 1.  tests/test_host_plan_cpu.py builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pg_host_plan.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                                                     \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #cond);                 \
            fprintf(stderr, __VA_ARGS__);                                                    \
            fprintf(stderr, "\n");                                                           \
            if (++g_fail > 20) exit(1);                                                      \
        }                                                                                    \
    } while (0)

// DevArena::take of pg_api_priv.h, on offsets
struct Arena {
    size_t cap, used;
    bool take(size_t bytes, size_t *at)
    {
        *at = pg_arena_align(used);
        if (*at + bytes > cap) return false;
        used = *at + bytes;
        return true;
    }
};

static void check_schedule(const PgHostPlan &p, uint64_t n, uint32_t hc, bool nsb)
{
    const std::vector<uint32_t> &b = p.bounds;
    CHECK(p.n == n && b.size() == (size_t)p.n_chunks + 1, "n %llu hc %u", (unsigned long long)n, hc);
    CHECK(b.front() == 0 && b.back() == n, "n %llu hc %u: %u .. %u", (unsigned long long)n, hc, b.front(), b.back());
    CHECK(n ? p.n_chunks >= 1 : p.n_chunks == 0, "n %llu hc %u", (unsigned long long)n, hc);
    for (size_t k = 0; k + 1 < b.size(); k++) {
        CHECK(b[k] < b[k + 1], "n %llu hc %u: chunk %zu is empty", (unsigned long long)n, hc, k);
        CHECK(b[k + 1] - b[k] <= PG_DELIVER_CHUNK, "n %llu hc %u: chunk %zu has %u reads", (unsigned long long)n, hc, k, b[k + 1] - b[k]);
        if (hc && k + 2 < b.size()) CHECK(b[k + 1] - b[k] == hc, "n %llu hc %u: chunk %zu has %u reads", (unsigned long long)n, hc, k, b[k + 1] - b[k]);
    }
    if (hc && n) CHECK(b.back() - b[b.size() - 2] <= hc, "n %llu hc %u: last chunk", (unsigned long long)n, hc);
    if (!hc && n && n <= PG_HOST_CHUNK) CHECK(p.n_chunks == 1, "n %llu: %u chunks", (unsigned long long)n, p.n_chunks);
    if (!hc && n > PG_HOST_CHUNK) CHECK(p.n_chunks > 1, "n %llu: %u chunks", (unsigned long long)n, p.n_chunks);
    CHECK(p.single == (p.n_chunks == 1 && !nsb), "n %llu hc %u nsb %d: single %d with %u chunks", (unsigned long long)n, hc, nsb, p.single, p.n_chunks);
}

static void check_takes(const PgHostPlan &p, bool tiny, size_t start)
{
    const unsigned long long n = p.n;
    CHECK(p.cap == (p.single ? 2 : 1) * pg_deliver_cap(p.n, tiny), "n %llu", n);
    CHECK(p.n_takes <= PG_PLAN_MAX_TAKES && (p.n_takes > 0) == (p.n > 0), "n %llu: %d takes", n, p.n_takes);
    if (p.n) CHECK(p.n_takes == (p.single ? 4 : 7) && p.takes[p.n_takes - 1] == (size_t)p.n_chunks * 64, "n %llu: %d takes", n, p.n_takes);
    Arena a = { start + p.arena_bytes, start };
    size_t at[PG_PLAN_MAX_TAKES], end = start;
    for (int k = 0; k < p.n_takes; k++) {
        CHECK(a.take(p.takes[k], &at[k]), "n %llu: take %d of %zu bytes does not fit in %zu", n, k, p.takes[k], p.arena_bytes);
        CHECK(at[k] >= end && at[k] % 256 == 0, "n %llu: take %d at %zu overlaps the one before (ends at %zu)", n, k, at[k], end);
        end = at[k] + p.takes[k];
    }
    if (!p.single) {
        if (p.n) {
            CHECK(p.takes[0] == p.cap * sizeof(pg_run) && p.takes[1] == p.takes[0], "n %llu: run buffers", n);
            CHECK(p.takes[2] == ((size_t)p.n + 1) * 8 && p.takes[3] == p.takes[2], "n %llu: offset arrays", n);
        }
        return;
    }
    CHECK(p.takes[0] == p.blk_bytes, "n %llu", n);
    const size_t want[PG_BLK_PARTS] = { ((size_t)p.n + 1) * 8, ((size_t)p.n + 1) * 8, p.n, (size_t)p.n * 4, (size_t)p.n * 2, p.cap * sizeof(pg_run) };
    size_t prev_end = 0;
    for (int k = 0; k < PG_BLK_PARTS; k++) {
        CHECK(p.blk[k].bytes == want[k], "n %llu: part %d has %zu bytes", n, k, p.blk[k].bytes);
        CHECK(p.blk[k].off % 16 == 0 && p.blk[k].off >= prev_end, "n %llu: part %d at %zu", n, k, p.blk[k].off);
        prev_end = p.blk[k].off + p.blk[k].bytes;
        CHECK(prev_end <= p.blk_bytes, "n %llu: part %d ends at %zu of %zu", n, k, prev_end, p.blk_bytes);
    }
    // the two run views at tot_close + tot_far = cap, however the runs split
    for (size_t tot_close : { (size_t)0, (size_t)1, p.cap / 2, p.cap - 1, p.cap }) {
        const size_t far_at = pg_plan_far_runs_at(p, tot_close), far_end = far_at + (p.cap - tot_close) * sizeof(pg_run);
        CHECK(far_at >= p.blk[PG_BLK_RUNS].off && far_end <= p.blk[PG_BLK_RUNS].off + p.blk[PG_BLK_RUNS].bytes, "n %llu: %zu close runs", n, tot_close);
    }
}

static void check_one_copy(uint32_t n)
{
    const PgHostPlan p = pg_host_plan(n, 0, false, false);
    const PgInputLayout &in = p.in;
    CHECK(p.single, "n %u", n);
    // the arena places the five arrays as the layout says: the same takes from an aligned start
    Arena a = { (size_t)1 << 40, 4096 };
    for (int k = 0; k < PG_IN_ARRAYS; k++) {
        size_t at = 0;
        CHECK(a.take(in.a[k].bytes, &at) && at - 4096 == in.a[k].off, "n %u: array %d at %zu, layout says %zu", n, k, at - 4096, in.a[k].off);
    }
    const size_t want[PG_IN_ARRAYS] = { ((size_t)n + 1) * 8, n, (size_t)n * 4, (size_t)n * 2, (size_t)n * 4 };
    for (int k = 0; k < PG_IN_ARRAYS; k++) CHECK(in.a[k].bytes == want[k], "n %u: array %d has %zu bytes", n, k, in.a[k].bytes);
    CHECK(in.span == in.a[PG_IN_CHR].off + (size_t)n * 4, "n %u: span %zu", n, in.span);
    CHECK(in.span <= p.off_words * 8 && p.off_words >= (size_t)n + 1, "n %u: span %zu, room %zu", n, in.span, p.off_words * 8);
    // a plan that is not one block asks for the offsets alone
    CHECK(pg_host_plan(n, 0, true, false).off_words == (size_t)n + 1, "n %u", n);
}

static void check_pinned(uint32_t n, std::vector<uint32_t> want)
{
    const PgHostPlan p = pg_host_plan(n, 0, false, false);
    CHECK(p.bounds == want, "n %u: %zu chunks, want %zu", n, p.bounds.size() - 1, want.size() - 1);
}

int main()
{
    const uint64_t ns[] = { 0, 1, 2, 255, 256, 257, (1u << 18) - 1, 1u << 18, (1u << 18) + 1, 2 * (1u << 18) + 4097, 10000000, 4294967294ull };
    const uint32_t chunks[] = { 0, 1, 7, 256, 1000, 1u << 20 };
    int cases = 0;
    for (uint64_t n : ns)
        for (uint32_t hc : chunks) {
            // (not reachable: a schedule of more than 2^24 chunks -- its boundaries alone are 64 MB and more, its events 2^25)
            if (hc && n / hc > (1u << 24)) continue;
            for (int sw = 0; sw < 4; sw++) {
                const bool nsb = sw & 1, tiny = sw & 2;
                const PgHostPlan p = pg_host_plan((uint32_t)n, hc, nsb, tiny);
                check_schedule(p, n, hc, nsb);
                for (size_t start : { (size_t)1, (size_t)4097, (size_t)1000003 }) check_takes(p, tiny, start);
                cases++;
            }
        }
    // schedules recorded from the loop search_host had before the plan existed
    check_pinned(2 * (1u << 18) + 4097, { 0, 65536, 196608, 458752, 528385 });
    check_pinned(4000000, { 0, 65536, 196608, 458752, 983040, 1988693, 2659128, 3106085, 3404056, 3666200, 3928344, 4000000 });
    check_pinned(10000000, { 0, 65536, 196608, 458752, 983040, 2031616, 3080192, 4128768, 5177344, 6225920, 7274496, 8182997, 8788664, 9192442,
                             9461628, 9723772, 9985916, 10000000 });
    for (uint32_t n : { 1u, 255u, 256u, 257u, 50000u, 1u << 18 }) check_one_copy(n);
    if (g_fail) return 1;
    printf("ok %d\n", cases);
    return 0;
}
