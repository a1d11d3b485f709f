// pg_dd.hip -- the containment test of -q (dispersed duplications) on the device:
// contains_subseq_any_strand(query, window, 15) of src/search_MEI_util.cpp:188-351, one wave per (item, strand).
//
// The DP (integer scores, candidates m/M, then g, then G, each taken on a strict '<'; column 0 set apart and never
// tested) runs systolically: for a block of 64 query rows, lane r owns row 64b + r and at step t does cell
// (row, t - r).  The cell above (row - 1, j) arrives from lane r - 1 by a one-lane shift, together with the base of
// column j; the diagonal cell is the value that arrived one step earlier; the left cell is the lane's own previous one.
// Lane 0 takes the row above it (the last row of the previous block, or zeros for block 0) and the window's bases from a
// 64-column chunk that the whole wave loads at once; lane 63's row is gathered 64 columns at a time and stored into the
// wave's boundary buffer for the next block.  A cell packs al (bits 0-9), mc (10-19) and the column's base (20-22):
// al <= query length <= 511 and mc < 512.
//
// The boolean of the reference's early exits comes from two facts per row: v = first row with a valid cell
// (al >= 15 && mc <= g_maxMismatch[al]), f = first row whose give-up test fires ((Q-i-1) + max_al_row < 15 -
// g_maxMismatch[15]; min_mismatch_count_current_row is always 0).  result = v exists and (no f or v <= f).  After each
// block both are known for its rows, and the remaining blocks are skipped once either is seen.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_device.h"

namespace {

constexpr uint32_t AL_MASK = 0x3ffu;
constexpr int MC_SHIFT = 10, BASE_SHIFT = 20;
constexpr int DD_MIN_LEN = 15;                   // MIN_CONSENSUS_LENGTH, src/search_MEI.cpp:38

// query byte -> code; a byte outside ACGTN never equals a window base (codes 0-4)
__device__ __forceinline__ uint32_t q_code(uint8_t ch, bool rc)
{
    switch (ch) {
    case 'A': return rc ? 3u : 0u;
    case 'C': return rc ? 2u : 1u;
    case 'G': return rc ? 1u : 2u;
    case 'T': return rc ? 0u : 3u;
    case 'N': return 4u;
    default: return 7u;                          // Convert2RC4N leaves NUL; an IUPAC letter stays itself
    }
}

__device__ __forceinline__ uint32_t ref_code(const PgDevRef &ref, uint64_t word0, uint64_t p)
{
    const uint64_t w = word0 + (p >> 5);
    const uint32_t b = (uint32_t)(p & 31u);
    if ((ref.nn[w] >> b) & 1u) return 4u;
    return ((ref.lo[w] >> b) & 1u) | (((ref.hi[w] >> b) & 1u) << 1);
}

__device__ __forceinline__ uint32_t lane_of(uint32_t v, uint32_t k) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)k); }

}  // namespace

extern "C" __global__ void __launch_bounds__(256) pg_dd_contains_kernel(PgDevRef ref, const uint32_t *__restrict__ mm,
                                                                        const uint8_t *__restrict__ query,
                                                                        const uint64_t *__restrict__ query_off,
                                                                        const int32_t *__restrict__ chr_id,
                                                                        const uint64_t *__restrict__ win_start,
                                                                        const uint32_t *__restrict__ win_len,
                                                                        uint8_t *__restrict__ out2, uint32_t *scratch,
                                                                        uint64_t scratch_stride, uint32_t n_tasks)
{
    __shared__ uint16_t s_mm[512];
    for (uint32_t k = threadIdx.x; k < 512; k += blockDim.x) s_mm[k] = (uint16_t)mm[k];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves_per_block = blockDim.x >> 6;
    const uint32_t wave = blockIdx.x * waves_per_block + (threadIdx.x >> 6);
    const uint32_t n_waves = gridDim.x * waves_per_block;
    uint32_t *bnd = scratch + (uint64_t)wave * scratch_stride;
    const int min_match = DD_MIN_LEN - (int)s_mm[DD_MIN_LEN];
    for (uint32_t task = wave; task < n_tasks; task += n_waves) {
        const uint32_t item = task >> 1;
        const bool rc = (task & 1u) != 0;
        const uint64_t q0 = query_off[item];
        const int Q = (int)(query_off[item + 1] - q0);
        const int D = (int)win_len[item];
        const uint64_t ws = win_start[item];
        const int c = chr_id[item];
        const uint64_t word0 = ref.chr_word_off[c];
        bool result = false;
        const int nb = (Q + 63) >> 6;
        bool decided = Q == 0 || D == 0;
        for (int b = 0; b < nb && !decided; b++) {
            const int row = b * 64 + (int)lane;
            const bool active = row < Q;
            const uint32_t qc = active ? q_code(query[q0 + (rc ? (uint64_t)(Q - 1 - row) : (uint64_t)row)], rc) : 7u;
            const bool last_block = b + 1 == nb;
            uint32_t cur = 0, up_last = 0, chunk = 0, gather = 0;
            int max_al = 0;
            bool valid = false;
            const int steps = D + 63;
            for (int t = 0; t < steps; t++) {
                if ((t & 63) == 0) {
                    const int col = t + (int)lane;
                    uint32_t v = 0;
                    if (col < D) {
                        const uint32_t above = b == 0 ? 0u : __hip_atomic_load(&bnd[col], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        v = above | (ref_code(ref, word0, ws + (uint64_t)col) << BASE_SHIFT);
                    }
                    chunk = v;
                }
                const uint32_t shifted = (uint32_t)__shfl_up((int)cur, 1, 64);
                const uint32_t from_chunk = lane_of(chunk, (uint32_t)(t & 63));
                const uint32_t up = lane == 0 ? from_chunk : shifted;
                const int j = t - (int)lane;
                if (j >= 0 && j < D) {
                    const uint32_t base = (up >> BASE_SHIFT) & 7u;
                    const bool match = base == qc;
                    int al, mc;
                    if (j == 0) {
                        mc = 0;
                        al = match ? 1 : 0;
                    } else {
                        const int pa = (int)(up_last & AL_MASK), pm = (int)((up_last >> MC_SHIFT) & AL_MASK);
                        const int ua = (int)(up & AL_MASK), um = (int)((up >> MC_SHIFT) & AL_MASK);
                        const int la = (int)(cur & AL_MASK), lm = (int)((cur >> MC_SHIFT) & AL_MASK);
                        int best = 0;
                        char act = 'n';
                        const int s_m = pa + 1 - 2 * pm;
                        if (match && best < s_m) {
                            best = s_m;
                            act = 'm';
                        } else {
                            const int s_x = pa - 2 * (pm + 1);
                            if (best < s_x) {
                                best = s_x;
                                act = 'M';
                            }
                        }
                        const int s_g = la - 2 * (lm + 1);
                        if (best < s_g) {
                            best = s_g;
                            act = 'g';
                        }
                        const int s_G = ua + 1 - 2 * (um + 1);
                        if (best < s_G) {
                            best = s_G;
                            act = 'G';
                        }
                        switch (act) {
                        case 'g': mc = lm + 1; al = la; break;
                        case 'G': mc = um + 1; al = ua + 1; break;
                        case 'm': mc = pm; al = pa + 1; break;
                        case 'M': mc = pm + 1; al = pa + 1; break;
                        default: mc = match ? 0 : 1; al = 1; break;
                        }
                        if (al >= DD_MIN_LEN && mc <= (int)s_mm[al]) valid = true;
                        max_al = al > max_al ? al : max_al;
                    }
                    cur = (uint32_t)al | ((uint32_t)mc << MC_SHIFT) | (base << BASE_SHIFT);
                }
                up_last = up;
                if (!last_block) {
                    // lane 63's cell of this step (row 64b + 63, column t - 63) goes to lane (t - 63) & 63 of `gather`
                    const int col = t - 63;
                    if (col >= 0) {
                        const uint32_t v63 = lane_of(cur, 63u) & ((1u << BASE_SHIFT) - 1u);
                        if ((int)lane == (col & 63)) gather = v63;
                        if ((col & 63) == 63 || col == D - 1) {
                            const int dst = (col & ~63) + (int)lane;
                            if (dst <= col) __hip_atomic_store(&bnd[dst], gather, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                    }
                }
            }
            const uint64_t vm = __ballot(active && valid);
            const uint64_t fm = __ballot(active && (Q - row - 1) + max_al < min_match);
            if (vm || fm) {
                decided = true;
                result = vm != 0 && (fm == 0 || __builtin_ctzll(vm) <= __builtin_ctzll(fm));
            }
        }
        if (lane == 0) out2[task] = result ? 1 : 0;
    }
}

// Host side of the launch (pg_api.cpp validates the arguments and owns the buffers).
int pg_dd_launch(const PgDevRef *ref, const uint32_t *d_mm, const uint8_t *d_query, const uint64_t *d_query_off,
                 const int32_t *d_chr, const uint64_t *d_ws, const uint32_t *d_wl, uint8_t *d_out2, uint32_t *d_scratch,
                 uint64_t scratch_stride, uint32_t n_tasks, uint32_t n_blocks, void *stream)
{
    hipLaunchKernelGGL(pg_dd_contains_kernel, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, *ref, d_mm, d_query, d_query_off, d_chr, d_ws,
                       d_wl, d_out2, d_scratch, scratch_stride, n_tasks);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
