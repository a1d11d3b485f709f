// pg_host_plan.h -- the plan of one host-path call (pg_search_batch, pg_close_end_batch) as plain data: the chunk schedule, the
// layout of a one-block delivery, the delivery's arena requests and the layout of the one-copy upload.  Sizes are stated ONCE,
// here: pg_api.cpp sizes the arena and takes from it by walking the same lists, and builds the host views and the device
// pointers of the block from the same array.  No HIP: tests/host_plan_unit.cpp compiles this header with plain g++.
#ifndef PG_HOST_PLAN_H
#define PG_HOST_PLAN_H

#include <algorithm>
#include <cstddef>
#include <vector>

#include "pg_device.h"

// The alignment rule of the device arena (DevArena::take), and the room a buffer needs in an arena that is sized before the
// buffer's position is known.
inline size_t pg_arena_align(size_t at) { return (at + 255) & ~(size_t)255; }
inline size_t pg_arena_room(size_t bytes) { return pg_arena_align(bytes) + 256; }

struct PgSpan { size_t off, bytes; };

// The five small per-read input arrays, taken from the arena one after the other (alloc_batch): offsets from the first.  A
// one-chunk batch sends them with ONE copy of `span` bytes from the pinned block that holds the rebased offsets.
enum { PG_IN_SEQ_OFF, PG_IN_STRAND, PG_IN_POS, PG_IN_ISZ, PG_IN_CHR, PG_IN_ARRAYS };
struct PgInputLayout {
    PgSpan a[PG_IN_ARRAYS];
    size_t span;
};
inline PgInputLayout pg_input_layout(size_t n)
{
    const size_t n1 = std::max<size_t>(n, 1), bytes[PG_IN_ARRAYS] = { (n + 1) * 8, n1, n1 * 4, n1 * 2, n1 * 4 };
    PgInputLayout l;
    size_t at = 0;
    for (int k = 0; k < PG_IN_ARRAYS; k++) {
        l.a[k] = PgSpan{ pg_arena_align(at), bytes[k] };
        at = l.a[k].off + bytes[k];
    }
    l.span = at;
    return l;
}

// The parts of a one-block delivery, in block order; both run lists share PG_BLK_RUNS (the far runs follow the close runs).
enum { PG_BLK_CLOSE_OFF, PG_BLK_FAR_OFF, PG_BLK_RC, PG_BLK_LAST, PG_BLK_MAX, PG_BLK_RUNS, PG_BLK_PARTS };
#define PG_PLAN_MAX_TAKES 7

struct PgHostPlan {
    uint32_t n = 0;
    std::vector<uint32_t> bounds;          // chunk k = reads [bounds[k], bounds[k + 1])
    uint32_t n_chunks = 0;
    bool single = false;                   // ONE chunk, delivered as one block in one device-to-host copy
    size_t cap = 0;                        // runs the delivery has room for: per list, or (single) for both lists together
    PgSpan blk[PG_BLK_PARTS] = {};         // (single) the block's parts, each 16-byte aligned
    size_t blk_bytes = 0;
    // the delivery's arena requests in the order they are taken: the block, or two run buffers and two offset arrays; then the
    // scan's per-read and per-block scratch and the per-chunk info.  arena_bytes: room for all of them from any arena offset.
    size_t takes[PG_PLAN_MAX_TAKES] = {};
    int n_takes = 0;
    size_t arena_bytes = 0;
    PgInputLayout in = {};
    size_t off_words = 0;                  // 64-bit words of the pinned offsets buffer (single: room for the one-copy upload)
};

// Runs per list the chunked delivery has room for (1.04 per read on average; a batch that needs more falls back to the
// whole-batch download, which scans the batch first and sizes its buffers from the totals).  tiny: tests force the fallback.
inline size_t pg_deliver_cap(size_t n, bool tiny) { return tiny ? n / 2 + 8 : 2 * n + 4096; }

// host_chunk, no_single_block, tiny_delivery: PgEnvSwitches
inline PgHostPlan pg_host_plan(uint32_t n, uint32_t host_chunk, bool no_single_block, bool tiny_delivery)
{
    PgHostPlan p;
    p.n = n;
    const bool chunk_env = host_chunk != 0u;                     // (tests: several chunks on a small batch)
    const uint32_t chunk = chunk_env ? host_chunk : PG_HOST_CHUNK;
    // Chunk boundaries.  A launch of 256 k reads runs at 278 M reads/s, one of 1 M at ~310, one of 10 M at 323 (ramp-up and
    // tail of the launch itself: profiles/r04/kernel_experiments.txt), but the first chunk's copy and the last chunk's
    // delivery + download are exposed: small chunks first (a quarter of the base chunk, doubling), up to 2^20 reads in the
    // middle, a third of what is left towards the end.
    std::vector<uint32_t> &bounds = p.bounds;
    bounds.assign(1, 0u);
    if (n > chunk && !chunk_env) {
        uint64_t ramp = chunk / 4;
        while (bounds.back() < n) {
            const uint64_t left = n - bounds.back();
            const uint64_t mid = std::min<uint64_t>(std::max<uint64_t>(left / 3, chunk), PG_DELIVER_CHUNK);
            bounds.push_back((uint32_t)(bounds.back() + std::min<uint64_t>(std::min(ramp, mid), left)));
            if (ramp < PG_DELIVER_CHUNK) ramp *= 2;             // (past `mid` for good: 48 more doublings would wrap it to 0)
        }
    }
    while (bounds.back() < n) bounds.push_back((uint32_t)std::min<uint64_t>((uint64_t)bounds.back() + chunk, n));
    p.n_chunks = (uint32_t)bounds.size() - 1;
    // A batch that is ONE chunk (Pindel's own 50 000-read flushes) gets its whole result in ONE device-to-host copy: offsets,
    // summaries and both run lists are laid out in one device block and one pinned host block (pg_result::block), the
    // result's arrays are views into it -- five copies and their ~10 us of runtime call each otherwise.
    p.single = p.n_chunks == 1 && !no_single_block;
    p.cap = (p.single ? 2 : 1) * pg_deliver_cap(n, tiny_delivery);
    const size_t off_bytes = ((size_t)n + 1) * 8;
    if (p.single) {
        const size_t part[PG_BLK_PARTS] = { off_bytes, off_bytes, n, (size_t)n * 4, (size_t)n * 2, p.cap * sizeof(pg_run) };
        for (int k = 0; k < PG_BLK_PARTS; k++) {
            p.blk[k] = PgSpan{ p.blk_bytes, part[k] };
            p.blk_bytes += (part[k] + 15) & ~(size_t)15;
        }
        p.takes[p.n_takes++] = p.blk_bytes;
    } else if (n) {
        for (size_t bytes : { p.cap * sizeof(pg_run), p.cap * sizeof(pg_run), off_bytes, off_bytes }) p.takes[p.n_takes++] = bytes;
    }
    if (n)
        for (size_t bytes : { (size_t)PG_DELIVER_CHUNK * 8, (size_t)4096 * 8, (size_t)p.n_chunks * 64 }) p.takes[p.n_takes++] = bytes;
    for (int k = 0; k < p.n_takes; k++) p.arena_bytes += pg_arena_room(p.takes[k]);
    p.in = pg_input_layout(n);
    p.off_words = std::max((size_t)n + 1, p.single ? (p.in.span + 7) / 8 : 0);
    return p;
}

// (single) where the far runs start in the block once the close runs are counted; the block's used bytes are
// pg_plan_far_runs_at(p, tot_close) + tot_far * sizeof(pg_run), inside the block while tot_close + tot_far <= cap
inline size_t pg_plan_far_runs_at(const PgHostPlan &p, size_t tot_close) { return p.blk[PG_BLK_RUNS].off + tot_close * sizeof(pg_run); }

#endif
