// pg_window_plan.h -- BreakDancer windows made ready for the device, as plain host arithmetic on outside input: groups of
// windows in CSR form (a group is a read for pg_windows, a cluster for pg_hint_table) are validated, and a window too long for
// the position field of a candidate id is cut into consecutive pieces.  Stated ONCE, here, for both hint forms of pg_api.cpp.
// No HIP and no pg_ctx: tests/window_plan_unit.cpp compiles this header with plain g++.
#ifndef PG_WINDOW_PLAN_H
#define PG_WINDOW_PLAN_H

#include <algorithm>
#include <cstddef>
#include <vector>

#include "pg_device.h"

// The longest window one candidate id can address (the width of its position field).  A longer window is searched as
// consecutive pieces: the reduction over candidates is additive over disjoint position sets.
#define PG_WINDOW_PIECE ((1ll << PG_REL_BITS) - 1)

// start < 0 means end - 1 (farend_searcher.cpp:69-71)
inline long long pg_window_start(const pg_window &w) { return w.start < 0 ? (long long)w.end - 1 : w.start; }

// The limits of one batch: a window index of 32 bits in all, of 29 bits inside a group (the 64-bit candidate ids).
inline bool pg_too_many_windows(uint64_t in_batch) { return in_batch > 0xffffffffull; }
inline bool pg_too_many_in_cluster(uint64_t in_group) { return in_group >= (1ull << 29); }

// What is wrong with the input, in the order it is looked for.
enum PgWindowStatus { PG_WINDOWS_OK = 0, PG_WINDOWS_OFFSETS_NOT_MONOTONE, PG_WINDOWS_NULL_ARRAY, PG_WINDOWS_UNKNOWN_CHROMOSOME };

struct PgWindowPlan {
    PgWindowStatus status = PG_WINDOWS_OK;
    // true: nothing was cut, the caller's offsets and windows are used as they are (off and win stay empty).
    // false: off (from 0) and win replace them.
    bool as_is = true;
    std::vector<uint64_t> off;
    std::vector<pg_window> win;
    uint64_t largest_group = 0;            // most windows of one group, pieces counted
    long long longest = 0;                 // positions of the longest window or piece (0: none, or none with end > start)
    const uint64_t *offsets(const uint64_t *given) const { return as_is ? given : off.data(); }
    const pg_window *windows(const pg_window *given) const { return as_is ? given : win.data(); }
};

// Group g holds windows[off[g] .. off[g + 1]); off[0] need not be 0.  n_chr: chromosomes of the loaded reference.
// copy: fill off / win even when nothing is cut.  group_longest (nullable): per group what `longest` is for all.
// A window that is not cut is passed through bit for bit (a negative start stays negative).
inline PgWindowPlan pg_window_plan(const uint64_t *off, size_t n_groups, const pg_window *windows, int n_chr, bool copy,
                                   std::vector<uint32_t> *group_longest)
{
    PgWindowPlan p;
    if (group_longest) group_longest->assign(n_groups, 0u);
    if (!n_groups) return p;
    const long long piece = PG_WINDOW_PIECE;
    for (size_t g = 0; g < n_groups; g++)
        if (off[g + 1] < off[g]) return p.status = PG_WINDOWS_OFFSETS_NOT_MONOTONE, p;
    if (off[n_groups] > off[0] && !windows) return p.status = PG_WINDOWS_NULL_ARRAY, p;
    bool cut = false;
    for (uint64_t k = off[0]; k < off[n_groups]; k++) {
        const pg_window &w = windows[k];
        if (w.chr_id < 0 || w.chr_id >= n_chr) return p.status = PG_WINDOWS_UNKNOWN_CHROMOSOME, p;
        if ((long long)w.end - pg_window_start(w) > piece) cut = true;
    }
    p.as_is = !cut && !copy;
    if (!p.as_is) {
        p.off.reserve(n_groups + 1);
        p.off.push_back(0);
        p.win.reserve((size_t)(off[n_groups] - off[0]));
    }
    for (size_t g = 0; g < n_groups; g++) {
        long long most = 0;
        for (uint64_t k = off[g]; k < off[g + 1]; k++) {
            const pg_window &w = windows[k];
            const long long st = pg_window_start(w);
            most = std::max(most, std::min((long long)w.end - st, piece));
            if (p.as_is) continue;
            if ((long long)w.end - st <= piece) {
                p.win.push_back(w);
                continue;
            }
            for (long long s0 = st; s0 < (long long)w.end; s0 += piece)
                p.win.push_back(pg_window{ w.chr_id, (int32_t)s0, (int32_t)std::min<long long>(s0 + piece, w.end) });
        }
        if (!p.as_is) p.off.push_back(p.win.size());
        p.largest_group = std::max<uint64_t>(p.largest_group, p.as_is ? off[g + 1] - off[g] : p.off[g + 1] - p.off[g]);
        p.longest = std::max(p.longest, most);
        if (group_longest) (*group_longest)[g] = (uint32_t)most;
    }
    return p;
}

#endif
