// pg_sv.hip -- the per-read stage of the five classifiers process_window runs besides SearchVariant::Search, on the device:
// searchIndels (DI), searchTandemDuplications(NT) and searchInversions(NT).  One wave per read of a searched batch; DESIGN.md 7l.
//
// The three kinds with non-template bases pair UP_Close.back() with UP_Far.back(): the last point of the last run of either
// list, arithmetic on one run each; all lanes compute the same values.  Tandem duplications and inversions visit (close point,
// far point) pairs budget by budget like SearchVariant::Search, in orders of their own, and what they compute for a pair depends on
// the pair alone, so the first visits come in the order of the key (mismatch sum, place of the close point, place of the far
// point) and the wave lists the PG_VARIANT_CANDS smallest keys as pg_variant.hip does: lanes take close points 64 at a time, for a
// close point and a far RUN the one far point that can qualify is the one of length ReadLength - LengthStr(close), the next pair
// is a wave-wide minimum, and the alignment walks of LeftMostTD / LeftMostINV compare 64 reference positions per step
// (pg_sv_align.h).  Those walks have no N test; a position beyond the guard words has a code that equals nothing.
// Integer types mirror the host's (pg_host_priv.hpp): unsigned AbsLoc sums that may wrap, BP and the inversion diff as short,
// IndelSize unsigned.  The mismatch budget of the NT kinds comes from a table made on the host (a + b * c would be contracted
// here).  ReadLength, MAX_SNP_ERROR and the bases are the post-state of GetCloseEnd, derived as in pg_variant.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_device.h"
#include "pg_sv_align.h"
#include "pg_variant_dev.h"

namespace {

using SvRefCode = DevRefCodeT<(uint32_t)PG_SV_OUT>;

struct EndPoint { uint32_t abs; int32_t len, mm; bool back, antisense; };
// the last point of a run (its len_last end) and the first one
__device__ __forceinline__ EndPoint last_point(const pg_run r)
{
    const uint32_t d = (uint32_t)r.len_last - r.len_first;
    const bool back = (r.flags & PG_RUN_BACKWARD) != 0;
    return { back ? r.abs_loc_first - d : r.abs_loc_first + d, (int32_t)r.len_last, (int32_t)r.mismatches, back, (r.flags & PG_RUN_ANTISENSE) != 0 };
}
__device__ __forceinline__ EndPoint first_point(const pg_run r)
{
    return { r.abs_loc_first, (int32_t)r.len_first, (int32_t)r.mismatches, (r.flags & PG_RUN_BACKWARD) != 0, (r.flags & PG_RUN_ANTISENSE) != 0 };
}

struct Fields {
    uint32_t bpl, bpr, indel;
    int32_t left, right, nt;
    int16_t bp;
    uint32_t ci, fi, flags;
};

// the fields of the four inversion geometries (sv_inv_fields, pg_host_priv.hpp)
__device__ __forceinline__ void inv_fields(int geo, uint32_t ca, int32_t cl, uint32_t fa, int32_t fl, int32_t RL, uint32_t spacer, Fields &f)
{
    if (geo == 0) {
        f.left = (int32_t)((ca + 1u) - (uint32_t)cl);
        f.right = (int32_t)(fa - (uint32_t)fl + (uint32_t)RL);
        f.bp = (int16_t)(cl - 1);
        f.indel = fa - ca;
        f.bpl = ca + 1u - spacer;
        f.bpr = fa - spacer;
    } else if (geo == 1) {
        f.right = (int32_t)(ca - (uint32_t)cl + (uint32_t)RL);
        f.left = (int32_t)(fa - (uint32_t)fl + 1u);
        f.bp = (int16_t)(fl - 1);
        f.indel = ca - fa;
        f.bpr = ca - spacer;
        f.bpl = (fa + 1u) - spacer;
    } else if (geo == 2) {
        f.left = (int32_t)(fa + (uint32_t)fl - (uint32_t)RL);
        f.right = (int32_t)(ca + (uint32_t)cl - 1u);
        f.bp = (int16_t)(fl - 1);
        f.indel = ca - fa;
        f.bpl = fa - spacer;
        f.bpr = ca - 1u - spacer;
    } else {
        f.right = (int32_t)(fa + (uint32_t)fl - 1u);
        f.left = (int32_t)(ca + (uint32_t)cl - (uint32_t)RL);
        f.bp = (int16_t)(cl - 1);
        f.indel = fa - ca;
        f.bpl = ca - spacer;
        f.bpr = fa - 1u - spacer;
    }
    f.flags = (uint32_t)geo << PG_SV_GEO_SHIFT;
}
__device__ __forceinline__ bool inv_distance_ok(int geo, uint32_t ca, uint32_t fa, uint32_t MIN)
{
    return geo == 0 ? fa > ca + MIN : geo == 1 ? fa + MIN < ca : geo == 2 ? ca > fa + MIN : ca + MIN < fa;
}

}  // namespace

struct PgSvArgs {
    const PgOutRec *out;
    const pg_run *pool;
    unsigned long long pool_runs;
    const uint8_t *seq;
    const uint64_t *seq_off;
    const uint8_t *strand;
    const int32_t *chr;
    const uint32_t *mm;                // g_maxMismatch, 512 entries
    const int32_t *budget;             // the NT kinds' mismatch budget by length sum, PG_SV_BUDGET_N entries
    int32_t min_matched;               // -d
    uint32_t min_inv;                  // -v
    uint32_t spacer, n;
    uint32_t *cands;                   // n x 88 dwords (PG_SV_SLOTS x 8)
    uint8_t *counts;                   // n x PG_SV_KINDS
};

extern "C" __global__ void __launch_bounds__(256) pg_sv_kernel(PgDevRef ref, PgSvArgs a)
{
    static_assert(sizeof(pg_variant_cand) == 32 && PG_SV_SLOTS == 3 + 2 * PG_VARIANT_CANDS && PG_SV_SLOTS * 8 <= 128, "two dwords per lane and read");
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t read = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (read >= a.n) return;                                     // (whole waves)
    uint32_t word0 = 0, word1 = 0;                               // dwords `lane` and 64 + `lane` of the read's 352 bytes of records
    uint32_t n_di = 0, n_td = 0, n_tdnt = 0, n_inv = 0, n_invnt = 0;
    // lanes 8 (slot & 7) .. + 7 hold the eight dwords of record `slot`: in word0 for slots 0-7, in word1 for slots 8-10
    auto put = [&](uint32_t slot, const Fields &f) {
        const uint32_t q = lane & 7u;
        const uint32_t v = q == 0u ? f.bpl : q == 1u ? f.bpr : q == 2u ? (uint32_t)f.left : q == 3u ? (uint32_t)f.right : q == 4u ? f.indel
                         : q == 5u ? (uint32_t)f.nt : q == 6u ? ((uint32_t)(uint16_t)f.bp | (f.ci << 16)) : (f.fi | (f.flags << 16));
        if ((lane >> 3) == (slot & 7u)) {
            if (slot < 8u) word0 = v;
            else word1 = v;
        }
    };
    const PgOutRec o = a.out[read];
    const uint64_t s0 = a.seq_off[read];
    const int32_t L = (int32_t)(a.seq_off[read + 1] - s0);
    const uint8_t *s = a.seq + s0;
    const uint8_t strand = a.strand[read];
    const int32_t chr = a.chr[read];
    const bool plus = strand == '+';
    bool live = (plus || strand == '-') && o.close_cnt && o.far_cnt && chr >= 0 && chr < ref.n_chr && L > 0 &&
                (unsigned long long)o.close_off + o.close_cnt <= a.pool_runs && (unsigned long long)o.far_off + o.far_cnt <= a.pool_runs;
    const pg_run *close = a.pool + o.close_off, *far = a.pool + o.far_off;
    // FragName == FarFragName: UpdateFarFragName takes the chromosome of the first far point
    if (live && far[0].chr_id != chr) live = false;
    uint32_t nc = 0, nf = 0;
    if (live) {
        nc = points_of(close, o.close_cnt);
        nf = points_of(far, o.far_cnt);
        if (nc > 0xffffu || nf > 0xffffu) live = false;         // (the indices of a candidate are 16 bits; a read has < 500 points a list)
    }
    if (live) {
        // ---- the post-state (as pg_variant.hip): its first base among the bytes as uploaded and its length
        int32_t RL = L;
        if (o.rc_flag) {
            int32_t first_ok = L, last_ok = -1;
            for (int32_t j0 = 0; j0 < L; j0 += 64) {
                const int32_t j = j0 + (int32_t)lane;
                const uint64_t ok = __ballot(j < L && base_code(s[j < L ? j : 0]) != (uint32_t)PG_VA_NONE);
                if (ok) {
                    if (first_ok == L) first_ok = j0 + __builtin_ctzll(ok);
                    last_ok = j0 + 63 - __builtin_clzll(ok);
                }
            }
            RL = (o.rc_flag >= 2 ? last_ok + 1 : L) - first_ok;
            if (RL <= 0) live = false;
        }
        const int32_t max_snp = (int32_t)a.mm[RL < 499 ? RL : 499];
        const int32_t rl_minus = (int32_t)(int16_t)(RL - 1);
        SvRefCode rc;
        rc.lo = ref.lo;
        rc.hi = ref.hi;
        rc.nn = ref.nn;
        rc.word0 = (int64_t)ref.chr_word_off[chr];
        const uint32_t chr_size = ref.chr_size[chr];
        rc.size = (int64_t)chr_size;
        const PgVaWaveWalk walk = { lane };
        const uint32_t spacer = a.spacer, MIN = a.min_inv;
        if (live) {
            // ---- the three kinds of one pair: UP_Close.back() with UP_Far.back()
            const EndPoint cp = last_point(close[o.close_cnt - 1u]), fp = last_point(far[o.far_cnt - 1u]);
            const EndPoint c0 = first_point(close[0]), f0 = first_point(far[0]);
            const uint32_t ca = cp.abs, fa = fp.abs;
            const int32_t cl = cp.len, fl = fp.len, sum = cl + fl;
            const bool shorter = sum < RL;                       // (all three ask for it: the table is read below ReadLength only)
            const bool within = shorter && sum >= 0 && sum < PG_SV_BUDGET_N && !(cp.mm + fp.mm > a.budget[shorter && sum >= 0 && sum < PG_SV_BUDGET_N ? sum : 0]);
            const int32_t nt = (int32_t)(uint16_t)(RL - fl - cl);
            Fields f;
            f.nt = nt;
            f.ci = nc - 1u;
            f.fi = nf - 1u;
            f.flags = 0;
            // searchIndels
            if (within && fp.back == plus && sum >= a.min_matched && (plus ? fa > ca + 1u : ca > fa + 1u)) {
                if (plus) {
                    f.left = (int32_t)(ca - (uint32_t)cl + 1u);
                    f.right = (int32_t)(fa + (uint32_t)fl - 1u);
                    f.bp = (int16_t)(cl - 1);
                    f.bpl = ca - spacer;
                    f.bpr = fa - spacer;
                } else {
                    f.left = (int32_t)(fa - (uint32_t)fl + 1u);
                    f.right = (int32_t)(ca + (uint32_t)cl - 1u);
                    f.bp = (int16_t)(fl - 1);
                    f.bpl = fa - spacer;
                    f.bpr = ca - spacer;
                }
                f.indel = (uint32_t)((f.right - f.left) + nt - rl_minus);
                put(0u, f);
                n_di = 1u;
            }
            // searchTandemDuplicationsNT
            if (within && fp.back == plus && sum > a.min_matched &&
                (plus ? (fa + (uint32_t)fl < ca && fa + (uint32_t)cl < ca) : (ca + (uint32_t)cl < fa && ca + (uint32_t)fl < fa))) {
                if (plus) {
                    f.right = (int32_t)(ca - (uint32_t)cl + 1u);
                    f.left = (int32_t)(fa + (uint32_t)fl - 1u);
                    f.bp = (int16_t)(cl - 1);
                    f.indel = ca - fa + 1u;
                    f.bpr = ca - spacer;
                    f.bpl = fa - spacer;
                } else {
                    f.right = (int32_t)(fa - (uint32_t)fl + 1u);
                    f.left = (int32_t)(ca + (uint32_t)cl - 1u);
                    f.bp = (int16_t)(fl - 1);
                    f.indel = fa - ca + 1u;
                    f.bpr = fa - spacer;
                    f.bpl = ca - spacer;
                }
                put(1u + PG_VARIANT_CANDS, f);
                n_tdnt = 1u;
            }
            // the read-level tests of both inversion classifiers: strand differs, direction is equal between the first points
            const bool inv_read = c0.antisense != f0.antisense && c0.back == f0.back;
            // searchInversionsNT: the far point runs the anchor's way; the first distance test that holds (they exclude each other)
            if (within && inv_read && sum >= a.min_matched && fp.back == !plus) {
                const int g0 = plus ? 0 : 2;
                const int geo = inv_distance_ok(g0, ca, fa, MIN) ? g0 : inv_distance_ok(g0 + 1, ca, fa, MIN) ? g0 + 1 : -1;
                if (geo >= 0) {
                    inv_fields(geo, ca, cl, fa, fl, RL, spacer, f);
                    put(2u + 2u * PG_VARIANT_CANDS, f);
                    n_invnt = 1u;
                }
            }
            // ---- tandem duplications (pass 0) and inversions (pass 1): the PG_VARIANT_CANDS first pairs in first-visit order
            int inv_geo = -1;
            if (inv_read) {
                if (plus) inv_geo = f0.abs > ca + MIN ? 0 : (fa + MIN < c0.abs ? 1 : -1);
                else inv_geo = ca > f0.abs + MIN ? 2 : (c0.abs + MIN < fa ? 3 : -1);
            }
            for (int pass = 0; pass < 2; pass++) {
                const bool td = pass == 0;
                if (!td && inv_geo < 0) break;
                const bool close_asc = td ? plus : (inv_geo == 1 || inv_geo == 3);
                const bool far_asc = td ? !plus : (inv_geo == 0 || inv_geo == 2);
                const bool want_back = td ? plus : !plus;        // TD: the far point runs against the anchor; INV: with it
                const uint32_t slot0 = td ? 1u : 2u + PG_VARIANT_CANDS;
                uint32_t count = 0;
                unsigned long long prev = 0;                     // keys are taken in ascending order; key + 1 so that 0 is "none yet"
                for (;;) {
                    // ---- the smallest key above `prev`
                    unsigned long long best = NO_KEY;
                    for (uint32_t k0 = 0; k0 < nc; k0 += 64u) {
                        const uint32_t k = k0 + lane;
                        if (k >= nc) continue;
                        const Point p = point_at(close, o.close_cnt, close_asc ? k : nc - 1u - k);
                        uint32_t fbase = 0;
                        for (uint32_t r = 0; r < o.far_cnt; r++) {
                            const pg_run fr = far[r];
                            const uint32_t fm = (uint32_t)fr.len_last - fr.len_first + 1u;
                            const uint32_t fb = fbase;
                            fbase += fm;
                            const bool back = (fr.flags & PG_RUN_BACKWARD) != 0;
                            if (back != want_back) continue;
                            const int32_t msum = p.mm + (int32_t)fr.mismatches;
                            if (msum > max_snp) continue;
                            // the far point's place in its run: the one of length ReadLength - LengthStr(close)
                            const int64_t d = (int64_t)(RL - p.len) - (int64_t)fr.len_first;
                            if (d < 0 || d >= (int64_t)fm) continue;
                            const uint32_t pa = back ? fr.abs_loc_first - (uint32_t)d : fr.abs_loc_first + (uint32_t)d;
                            const uint32_t plen = (uint32_t)p.len, qlen = (uint32_t)(RL - p.len);
                            if (td) {
                                if (plus ? !(pa + qlen < p.abs && pa + plen < p.abs) : !(p.abs + plen < pa && p.abs + qlen < pa)) continue;
                                if ((plus ? pa : p.abs) - spacer == 0u) continue;      // BPLeft == 0: assigned, then skipped
                            } else if (!inv_distance_ok(inv_geo, p.abs, pa, MIN)) {
                                continue;
                            }
                            const uint32_t idx = fb + (uint32_t)d;
                            const unsigned long long key = (((unsigned long long)msum << KEY_SUM_SHIFT) | ((unsigned long long)k << KEY_K_SHIFT) |
                                                            (unsigned long long)(far_asc ? idx : KEY_IDX_MASK - idx)) + 1ull;
                            if (key > prev && key < best) best = key;
                        }
                    }
                    best = wave_min(best);
                    if (best == NO_KEY) break;
                    if (count == PG_VARIANT_CANDS) {
                        count |= PG_VARIANT_MORE;
                        break;
                    }
                    prev = best;
                    // ---- the pair's fields, by the whole wave
                    const uint32_t k = (uint32_t)((best - 1ull) >> KEY_K_SHIFT) & KEY_IDX_MASK;
                    const uint32_t low = (uint32_t)(best - 1ull) & KEY_IDX_MASK;
                    Fields g;
                    g.ci = close_asc ? k : nc - 1u - k;
                    g.fi = far_asc ? low : KEY_IDX_MASK - low;
                    g.nt = 0;
                    g.flags = 0;
                    const Point p = point_at(close, o.close_cnt, g.ci), q = point_at(far, o.far_cnt, g.fi);
                    bool ref_end;
                    if (td) {
                        if (plus) {
                            g.right = (int32_t)(p.abs - (uint32_t)p.len + 1u);
                            g.left = (int32_t)(q.abs + (uint32_t)q.len - 1u);
                            g.bp = (int16_t)(p.len - 1);
                            g.indel = p.abs - q.abs + 1u;
                            g.bpr = p.abs - spacer;
                            g.bpl = q.abs - spacer;
                        } else {
                            g.right = (int32_t)(q.abs - (uint32_t)q.len + 1u);
                            g.left = (int32_t)(p.abs + (uint32_t)p.len - 1u);
                            g.bp = (int16_t)(q.len - 1);
                            g.indel = q.abs - p.abs + 1u;
                            g.bpr = q.abs - spacer;
                            g.bpl = p.abs - spacer;
                        }
                        ref_end = pg_sv_left_most_td(walk, rc, chr_size, spacer, g.bpl, g.bpr, g.bp);
                    } else {
                        inv_fields(inv_geo, p.abs, p.len, q.abs, q.len, RL, spacer, g);
                        ref_end = pg_sv_left_most_inv(walk, rc, chr_size, spacer, plus, (int16_t)RL, g.bpl, g.bpr, g.bp);
                    }
                    if (ref_end) g.flags |= PG_VARIANT_REF_END;
                    put(slot0 + count, g);
                    count++;
                    if (ref_end) break;                          // (the read is Used here: no later pair is ever tried)
                }
                if (td) n_td = count;
                else n_inv = count;
            }
        }
    }
    a.cands[(size_t)read * (PG_SV_SLOTS * 8u) + lane] = word0;
    if (lane < PG_SV_SLOTS * 8u - 64u) a.cands[(size_t)read * (PG_SV_SLOTS * 8u) + 64u + lane] = word1;
    if (lane < PG_SV_KINDS)
        a.counts[(size_t)read * PG_SV_KINDS + lane] = (uint8_t)(lane == 0u ? n_di : lane == 1u ? n_td : lane == 2u ? n_tdnt : lane == 3u ? n_inv : n_invnt);
}

// Host side of the launch (pg_api_classify.cpp checks the batch and the parameters and owns the buffers): four reads per workgroup.
int pg_sv_launch(const PgDevRef *ref, const PgOutRec *out, const pg_run *pool, unsigned long long pool_runs, const uint8_t *seq,
                 const uint64_t *seq_off, const uint8_t *strand, const int32_t *chr, const uint32_t *d_mm, const int32_t *d_budget,
                 int32_t min_matched, uint32_t min_inv, uint32_t spacer, uint32_t n, pg_variant_cand *d_cands, uint8_t *d_counts, void *stream)
{
    if (!n) return 0;
    PgSvArgs a;
    a.out = out;
    a.pool = pool;
    a.pool_runs = pool_runs;
    a.seq = seq;
    a.seq_off = seq_off;
    a.strand = strand;
    a.chr = chr;
    a.mm = d_mm;
    a.budget = d_budget;
    a.min_matched = min_matched;
    a.min_inv = min_inv;
    a.spacer = spacer;
    a.n = n;
    a.cands = (uint32_t *)d_cands;
    a.counts = d_counts;
    hipLaunchKernelGGL(pg_sv_kernel, dim3((n + 3u) / 4u), dim3(256), 0, (hipStream_t)stream, *ref, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
