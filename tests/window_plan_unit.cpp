// Stand-alone check of pindel_amd/csrc/pg_window_plan.h (plain g++, address + undefined-behaviour sanitizers, no GPU): validation
// and its order, the cutting of long windows into pieces, the grouping and the two limits.  The expectations are properties of
// the arithmetic (the pieces tile the window), not the header's loop again.  Prints "ok <cases>" and exits 0, or says what failed
// and exits 1.  tests/test_window_plan_cpu.py builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pg_window_plan.h"

static int g_fail = 0, g_cases = 0;
#define CHECK(cond, ...)                                                                     \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #cond);                 \
            fprintf(stderr, __VA_ARGS__);                                                    \
            fprintf(stderr, "\n");                                                           \
            if (++g_fail > 20) exit(1);                                                      \
        }                                                                                    \
    } while (0)

static const long long PIECE = (1ll << 26) - 1;
static const int N_CHR = 3;

static bool same(const pg_window &a, const pg_window &b) { return memcmp(&a, &b, sizeof a) == 0; }

// positions a window covers (start < 0: the one position end - 1), and the pieces it takes
static long long width(const pg_window &w) { return w.start < 0 ? 1 : w.end > w.start ? (long long)w.end - w.start : 0; }
static long long pieces_of(long long positions) { return positions <= PIECE ? 1 : (positions + PIECE - 1) / PIECE; }

// out[0 .. n_out) against the window it was made from: w itself when it fits in one piece; otherwise pieces in order that tile
// [start, end) without gap or overlap, none longer than PIECE, ceil(width / PIECE) of them
static void check_tiling(const pg_window &w, const pg_window *out, size_t n_out, const char *what)
{
    const long long positions = width(w);
    CHECK((long long)n_out == pieces_of(positions), "%s: %zu pieces for %lld positions", what, n_out, positions);
    if (positions <= PIECE) {
        CHECK(n_out == 1 && same(out[0], w), "%s: a window that fits was changed", what);
        return;
    }
    long long at = w.start;
    for (size_t k = 0; k < n_out; k++) {
        CHECK(out[k].chr_id == w.chr_id && out[k].start == at, "%s: piece %zu starts at %d, want %lld", what, k, out[k].start, at);
        CHECK(out[k].end > out[k].start && (long long)out[k].end - out[k].start <= PIECE, "%s: piece %zu is [%d, %d)", what, k, out[k].start, out[k].end);
        at = out[k].end;
    }
    CHECK(at == w.end, "%s: the pieces end at %lld, the window at %d", what, at, w.end);
}

// one window of `positions` positions from `start` (start < 0: the "end - 1" form, one position) in one group
static void one_window(int32_t start, long long positions)
{
    g_cases++;
    const pg_window w = { 1, start, (int32_t)(start < 0 ? 1000 : start + positions) };
    const uint64_t off[2] = { 0, 1 };
    std::vector<uint32_t> longest;
    const PgWindowPlan p = pg_window_plan(off, 1, &w, N_CHR, false, &longest);
    char what[96];
    snprintf(what, sizeof what, "start %d, %lld positions", start, positions);
    CHECK(p.status == PG_WINDOWS_OK, "%s: status %d", what, (int)p.status);
    CHECK(p.as_is == (positions <= PIECE), "%s: as_is %d", what, (int)p.as_is);
    CHECK(p.longest == std::min(positions, PIECE) && longest.size() == 1 && longest[0] == p.longest, "%s: longest %lld", what, p.longest);
    CHECK(p.largest_group == (uint64_t)pieces_of(positions), "%s: largest group %llu", what, (unsigned long long)p.largest_group);
    if (p.as_is) {
        CHECK(p.off.empty() && p.win.empty() && p.offsets(off) == off && p.windows(&w) == &w, "%s: as it is, yet copied", what);
        // asked to copy: the same window, bit for bit (a negative start stays)
        const PgWindowPlan c = pg_window_plan(off, 1, &w, N_CHR, true, nullptr);
        CHECK(!c.as_is && c.off == (std::vector<uint64_t>{ 0, 1 }) && c.win.size() == 1 && same(c.win[0], w), "%s: the copy differs", what);
        CHECK(c.longest == p.longest && c.largest_group == 1, "%s: the copy's figures differ", what);
        return;
    }
    CHECK(p.off.size() == 2 && p.off[0] == 0 && p.off[1] == p.win.size() && p.offsets(off) == p.off.data() && p.windows(&w) == p.win.data(), "%s: offsets", what);
    check_tiling(w, p.win.data(), p.win.size(), what);
}

// groups over a window array; expectations by direct count
static void check_groups(const std::vector<uint64_t> &off, const std::vector<pg_window> &win, bool copy, const char *what)
{
    g_cases++;
    const size_t n = off.size() - 1;
    std::vector<uint32_t> longest;
    const PgWindowPlan p = pg_window_plan(off.data(), n, win.data(), N_CHR, copy, &longest);
    CHECK(p.status == PG_WINDOWS_OK && longest.size() == n, "%s: status %d", what, (int)p.status);
    bool any_long = false;
    for (uint64_t k = off[0]; k < off[n]; k++) any_long |= width(win[k]) > PIECE;
    CHECK(p.as_is == (!any_long && !copy), "%s: as_is %d", what, (int)p.as_is);
    const uint64_t *o = p.offsets(off.data());
    const pg_window *w = p.windows(win.data());
    if (!p.as_is) CHECK(p.off.size() == n + 1 && o[0] == 0 && o[n] == p.win.size(), "%s: offsets of the copy", what);
    uint64_t largest = 0;
    long long all = 0;
    for (size_t g = 0; g < n; g++) {
        uint64_t count = 0, at = o[g];
        long long most = 0;
        for (uint64_t k = off[g]; k < off[g + 1]; k++) {
            const uint64_t m = (uint64_t)pieces_of(width(win[k]));
            if (at + m <= o[g + 1]) check_tiling(win[k], w + at, (size_t)m, what);
            at += m;
            count += m;
            most = std::max(most, std::min(width(win[k]), PIECE));
        }
        // the output offsets are the prefix sums of the piece counts
        CHECK(o[g + 1] - o[g] == count && at == o[g + 1], "%s: group %zu has %llu windows, want %llu", what, g, (unsigned long long)(o[g + 1] - o[g]), (unsigned long long)count);
        CHECK(longest[g] == most, "%s: group %zu longest %u, want %lld", what, g, longest[g], most);
        largest = std::max(largest, count);
        all = std::max(all, most);
    }
    CHECK(p.largest_group == largest && p.longest == all, "%s: largest group %llu, longest %lld", what, (unsigned long long)p.largest_group, p.longest);
}

static void check_status(const std::vector<uint64_t> &off, const pg_window *win, PgWindowStatus want, const char *what)
{
    g_cases++;
    const PgWindowPlan p = pg_window_plan(off.data(), off.size() - 1, win, N_CHR, false, nullptr);
    CHECK(p.status == want, "%s: status %d, want %d", what, (int)p.status, (int)want);
}

int main()
{
    // ---- tiling
    for (long long positions : { 1ll, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE, 2 * PIECE + 1, (1ll << 31) - 65536 })
        for (int32_t start : { 0, 7, 65535 })
            if (start + positions <= 2147483647ll) one_window(start, positions);
    one_window(-1, 1);
    one_window(-5, 1);
    {
        // end - 1 of a window whose end is 0 is -1: one position, passed through
        g_cases++;
        const pg_window w = { 0, -1, 0 };
        const uint64_t off[2] = { 0, 1 };
        const PgWindowPlan p = pg_window_plan(off, 1, &w, N_CHR, false, nullptr);
        CHECK(p.status == PG_WINDOWS_OK && p.as_is && p.longest == 1, "end 0: longest %lld", p.longest);
    }

    // ---- degenerate windows: passed through, 0 towards the longest
    for (const pg_window &w : { pg_window{ 0, 10, 10 }, pg_window{ 2, 500, 20 }, pg_window{ 1, 2147483647, 0 } }) {
        check_groups({ 0, 1 }, { w }, false, "degenerate");
        check_groups({ 0, 1 }, { w }, true, "degenerate, copied");
        check_groups({ 0, 2 }, { w, pg_window{ 0, 5, 9 } }, false, "degenerate beside 4 positions");
    }

    // ---- groups
    const int32_t L = (int32_t)PIECE;
    const std::vector<pg_window> short_win = { { 0, 0, 10 }, { 1, 100, 5000 }, { 2, -1, 77 }, { 0, 3, 4 }, { 1, 9, 9 }, { 2, 1, L + 1 } };
    check_groups({ 0, 0, 2, 2, 5, 6, 6 }, short_win, false, "short windows, empty groups");
    check_groups({ 0, 0, 2, 2, 5, 6, 6 }, short_win, true, "short windows, copied");
    check_groups({ 2, 2, 3, 6 }, short_win, false, "first offset 2");
    check_groups({ 2, 2, 3, 6 }, short_win, true, "first offset 2, copied");
    check_groups({ 6, 6, 6 }, short_win, false, "no windows at offset 6");
    std::vector<pg_window> long_win = short_win;
    long_win[3] = pg_window{ 1, 1000, 1000 + 2 * L + 1 };           // three pieces in the middle of a group
    long_win[5] = pg_window{ 2, 0, L + 1 };                         // two
    check_groups({ 0, 0, 2, 2, 5, 6, 6 }, long_win, false, "a long window inside a group");
    check_groups({ 1, 2, 2, 5 }, long_win, false, "a long window, first offset 1");
    check_groups({ 0, 3, 3 }, long_win, false, "the long windows left out");
    check_groups({ 0, 6 }, long_win, true, "one group of all");
    {
        g_cases++;
        const PgWindowPlan p = pg_window_plan(nullptr, 0, nullptr, N_CHR, true, nullptr);
        CHECK(p.status == PG_WINDOWS_OK && p.largest_group == 0 && p.longest == 0 && p.win.empty(), "no groups");
    }

    // ---- rejections, each alone
    const pg_window good[3] = { { 0, 1, 2 }, { 2, 1, 2 }, { 1, 1, 2 } };
    const pg_window minus[3] = { { 0, 1, 2 }, { -1, 1, 2 }, { 1, 1, 2 } };
    const pg_window beyond[3] = { { 0, 1, 2 }, { 1, 1, 2 }, { N_CHR, 1, 2 } };
    check_status({ 0, 1, 3 }, good, PG_WINDOWS_OK, "good");
    check_status({ 0, 2, 1, 3 }, good, PG_WINDOWS_OFFSETS_NOT_MONOTONE, "offsets go back");
    check_status({ 3, 2 }, good, PG_WINDOWS_OFFSETS_NOT_MONOTONE, "one group that ends before it starts");
    check_status({ 0, 1, 3 }, nullptr, PG_WINDOWS_NULL_ARRAY, "three windows, no array");
    check_status({ 4, 4, 4 }, nullptr, PG_WINDOWS_OK, "no windows, no array");
    check_status({ 0, 1, 3 }, minus, PG_WINDOWS_UNKNOWN_CHROMOSOME, "chr_id -1");
    check_status({ 0, 1, 3 }, beyond, PG_WINDOWS_UNKNOWN_CHROMOSOME, "chr_id n_chr");
    check_status({ 0, 1, 2 }, beyond, PG_WINDOWS_OK, "chr_id n_chr outside every group");
    // ... and two together: offsets before the array, the array before the chromosomes
    check_status({ 0, 2, 1, 3 }, nullptr, PG_WINDOWS_OFFSETS_NOT_MONOTONE, "offsets go back and no array");
    check_status({ 0, 3, 1, 3 }, minus, PG_WINDOWS_OFFSETS_NOT_MONOTONE, "offsets go back and chr_id -1");

    // ---- limits
    g_cases += 4;
    CHECK(!pg_too_many_windows((1ull << 32) - 1) && pg_too_many_windows(1ull << 32), "2^32 windows in a batch");
    CHECK(!pg_too_many_in_cluster((1ull << 29) - 1) && pg_too_many_in_cluster(1ull << 29), "2^29 windows in a cluster");

    if (g_fail) return 1;
    printf("ok %d\n", g_cases);
    return 0;
}
