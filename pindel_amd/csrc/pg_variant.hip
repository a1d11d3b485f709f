// pg_variant.hip -- the per-read stage of SearchVariant::Search (src/search_variant.cpp:104-240) on the device, for its two
// kinds: 0 = deletions, 1 = short insertions.  One wave per read of a searched batch; DESIGN.md 7k.
//
// The reference visits (close point, far point) pairs budget by budget, close points ascending ('+' anchor) or descending
// ('-'), far points from the highest index down, and what it computes for a pair depends on the pair alone.  So the first visit
// of every qualifying pair comes in the order of the key (Mismatches(close) + Mismatches(far), k, -far index), k = the close
// point's place in visiting order.  The wave lists the PG_VARIANT_CANDS smallest keys:
//   * lanes take close points 64 at a time; for a close point and a far RUN at most one far point can qualify -- deletions: the
//     one of length ReadLength - LengthStr(close); insertions: the one at AbsLoc(close) +- 1 -- and run-length encoding makes it
//     one piece of arithmetic, no scan over far points;
//   * "the next pair" is a wave-wide minimum over the keys above the last one taken;
//   * its fields are computed by the whole wave: the alignment walks compare 64 reference positions per step
//     (pg_variant_align.h), decoded from the planes.
// Integer types mirror the host's (pg_host.cpp, search_variant): the short casts of BP and diff, unsigned AbsLoc - spacer,
// IndelSize as unsigned.  ReadLength, MAX_SNP_ERROR and the bases are the post-state of GetCloseEnd: rc_flag applications of
// setUnmatchedSeq(ReverseComplement()), shortening included, worked out from the bytes as uploaded.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_device.h"
#include "pg_variant_align.h"
#include "pg_variant_dev.h"

struct PgVariantArgs {
    const PgOutRec *out;
    const pg_run *pool;
    unsigned long long pool_runs;
    const uint8_t *seq;
    const uint64_t *seq_off;
    const uint8_t *strand;
    const int32_t *chr;
    const uint32_t *mm;                // g_maxMismatch, 512 entries
    uint32_t spacer, n;
    uint32_t *cands;                   // n x 64 dwords (2 kinds x PG_VARIANT_CANDS x 8)
    uint8_t *counts;                   // n x 2
};

extern "C" __global__ void __launch_bounds__(256) pg_variant_kernel(PgDevRef ref, PgVariantArgs a)
{
    static_assert(sizeof(pg_variant_cand) == 32 && 2 * PG_VARIANT_CANDS * sizeof(pg_variant_cand) == 256, "one dword per lane and read");
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t read = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (read >= a.n) return;                                     // (whole waves)
    uint32_t my_word = 0;                                        // dword `lane` of the read's 256 bytes of candidates
    uint32_t count[2] = { 0u, 0u };
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
        // ---- the post-state: its first base among the bytes as uploaded, its length, whether it runs backwards through them
        int32_t lead = 0, RL = L;
        if (o.rc_flag) {
            // the first reverse complement turns the bytes outside ACGTN into NULs and setUnmatchedSeq strips the trailing ones:
            // the characters the read BEGAN with; the second one strips what it ended with
            int32_t first_ok = L, last_ok = -1;
            for (int32_t j0 = 0; j0 < L; j0 += 64) {
                const int32_t j = j0 + (int32_t)lane;
                const uint64_t ok = __ballot(j < L && base_code(s[j < L ? j : 0]) != (uint32_t)PG_VA_NONE);
                if (ok) {
                    if (first_ok == L) first_ok = j0 + __builtin_ctzll(ok);
                    last_ok = j0 + 63 - __builtin_clzll(ok);
                }
            }
            lead = first_ok;
            RL = (o.rc_flag >= 2 ? last_ok + 1 : L) - lead;
            if (RL <= 0) live = false;
        }
        const ReadCode tcode = { s, lead, RL, plus != (o.rc_flag == 1) };
        const int32_t max_snp = (int32_t)a.mm[RL < 499 ? RL : 499];
        DevRefCode rc;
        rc.lo = ref.lo;
        rc.hi = ref.hi;
        rc.nn = ref.nn;
        rc.word0 = (int64_t)ref.chr_word_off[chr];
        const uint32_t chr_size = ref.chr_size[chr];
        rc.size = (int64_t)chr_size;
        const PgVaWaveWalk walk = { lane };
        for (int kind = 0; kind < 2 && live; kind++) {
            unsigned long long prev = 0;                         // keys are taken in ascending order; key + 1 so that 0 is "none yet"
            for (;;) {
                // ---- the smallest key above `prev`
                unsigned long long best = NO_KEY;
                for (uint32_t k0 = 0; k0 < nc; k0 += 64u) {
                    const uint32_t k = k0 + lane;
                    if (k >= nc) continue;
                    const Point cp = point_at(close, o.close_cnt, plus ? k : nc - 1u - k);
                    uint32_t fbase = 0;
                    for (uint32_t f = 0; f < o.far_cnt; f++) {
                        const pg_run fr = far[f];
                        const uint32_t fm = (uint32_t)fr.len_last - fr.len_first + 1u;
                        const uint32_t fb = fbase;
                        fbase += fm;
                        const bool back = (fr.flags & PG_RUN_BACKWARD) != 0;
                        if (back != plus) continue;              // fp.Direction must be opposite the anchor's strand
                        const int32_t sum = cp.mm + (int32_t)fr.mismatches;
                        if (sum > max_snp) continue;
                        int64_t d;                               // the far point's place in its run
                        if (kind == 0) {
                            d = (int64_t)(RL - cp.len) - (int64_t)fr.len_first;
                            if (d < 0 || d >= (int64_t)fm) continue;
                            const uint32_t fa = back ? fr.abs_loc_first - (uint32_t)d : fr.abs_loc_first + (uint32_t)d;
                            if (plus ? !(fa > cp.abs + 1u) : !(cp.abs > fa + 1u)) continue;
                        } else {
                            // '+' anchor: far AbsLoc == close AbsLoc + 1 on a BACKWARD run; '-': close AbsLoc == far AbsLoc + 1 on a FORWARD run
                            d = plus ? (int64_t)fr.abs_loc_first - ((int64_t)cp.abs + 1) : ((int64_t)cp.abs - 1) - (int64_t)fr.abs_loc_first;
                            if (d < 0 || d >= (int64_t)fm) continue;
                            if (!(cp.len + (int32_t)fr.len_first + (int32_t)d < RL)) continue;
                        }
                        const uint32_t fi = fb + (uint32_t)d;
                        const unsigned long long key = (((unsigned long long)sum << KEY_SUM_SHIFT) | ((unsigned long long)k << KEY_K_SHIFT) |
                                                        (unsigned long long)(KEY_IDX_MASK - fi)) + 1ull;
                        if (key > prev && key < best) best = key;
                    }
                }
                best = wave_min(best);
                if (best == NO_KEY) break;
                if (count[kind] == PG_VARIANT_CANDS) {
                    count[kind] |= PG_VARIANT_MORE;
                    break;
                }
                prev = best;
                // ---- the pair's fields, by the whole wave
                const uint32_t k = (uint32_t)((best - 1ull) >> KEY_K_SHIFT) & KEY_IDX_MASK;
                const uint32_t fi = KEY_IDX_MASK - ((uint32_t)(best - 1ull) & KEY_IDX_MASK);
                const uint32_t ci = plus ? k : nc - 1u - k;
                const Point cp = point_at(close, o.close_cnt, ci), fp = point_at(far, o.far_cnt, fi);
                int32_t left, right;
                int16_t bp;
                uint32_t bpl, bpr;
                if (plus) {
                    left = (int32_t)(cp.abs - (uint32_t)cp.len + 1u);
                    right = (int32_t)(fp.abs + (uint32_t)fp.len - 1u);
                    bp = (int16_t)(cp.len - 1);
                    bpl = cp.abs - a.spacer;
                    bpr = fp.abs - a.spacer;
                } else {
                    left = (int32_t)(fp.abs - (uint32_t)fp.len + 1u);
                    right = (int32_t)(cp.abs + (uint32_t)cp.len - 1u);
                    bp = (int16_t)(fp.len - 1);
                    bpl = fp.abs - a.spacer;
                    bpr = cp.abs - a.spacer;
                }
                const int32_t rl_minus = (int32_t)(int16_t)(RL - 1);
                const uint32_t indel = kind == 0 ? (uint32_t)((right - left) - rl_minus) : (uint32_t)(rl_minus - (right - left));
                // NT_str = sub(string, BP + 1, IndelSize): empty when the start is outside the string or nothing is asked for
                uint32_t ins_len = 0;
                const int32_t ins_at = (int32_t)bp + 1;
                if (kind == 1 && ins_at >= 0 && ins_at <= RL && (int64_t)indel > 0)
                    ins_len = (int64_t)indel < (int64_t)(RL - ins_at) ? indel : (uint32_t)(RL - ins_at);
                uint32_t flags = 0;
                int32_t rot = 0;
                if (chr_size < bpl || chr_size < bpr) {
                    flags = PG_VARIANT_REF_END;
                } else {
                    uint32_t real_l = bpl, real_r = bpr;
                    if (ins_len) {
                        const InsCode ins = { tcode, ins_at };
                        rot = pg_va_real_start_insertion(walk, rc, ins, ins_len, a.spacer, real_l, real_r);
                    } else {
                        pg_va_real_start_deletion(walk, rc, a.spacer, real_l, real_r);
                    }
                    int16_t diff = (int16_t)(bpl - real_l);
                    diff = !(((int32_t)bp - 1) < (int32_t)diff) ? diff : (int16_t)(bp - 1);
                    if (diff > 0) {
                        bp = (int16_t)(bp - diff);
                        bpl -= (uint32_t)(int32_t)diff;
                        bpr -= (uint32_t)(int32_t)diff;
                    }
                }
                const uint32_t slot = (uint32_t)kind * PG_VARIANT_CANDS + count[kind];
                if ((lane >> 3) == slot) {                       // lanes 8 slot .. 8 slot + 7 hold the record's eight dwords
                    const uint32_t q = lane & 7u;
                    my_word = q == 0u ? bpl : q == 1u ? bpr : q == 2u ? (uint32_t)left : q == 3u ? (uint32_t)right : q == 4u ? indel
                            : q == 5u ? (uint32_t)rot : q == 6u ? ((uint32_t)(uint16_t)bp | (ci << 16)) : (fi | (flags << 16));
                }
                count[kind]++;
                if (flags) break;                                // (the loop marks the read Used here: no later pair is ever tried)
            }
        }
    }
    a.cands[(size_t)read * 64u + lane] = my_word;
    if (lane < 2u) a.counts[(size_t)read * 2u + lane] = (uint8_t)(lane ? count[1] : count[0]);
}

// Host side of the launch (pg_api_classify.cpp checks the batch and owns the buffers): four reads per workgroup.
int pg_variant_launch(const PgDevRef *ref, const PgOutRec *out, const pg_run *pool, unsigned long long pool_runs, const uint8_t *seq,
                      const uint64_t *seq_off, const uint8_t *strand, const int32_t *chr, const uint32_t *d_mm, uint32_t spacer,
                      uint32_t n, pg_variant_cand *d_cands, uint8_t *d_counts, void *stream)
{
    if (!n) return 0;
    PgVariantArgs a;
    a.out = out;
    a.pool = pool;
    a.pool_runs = pool_runs;
    a.seq = seq;
    a.seq_off = seq_off;
    a.strand = strand;
    a.chr = chr;
    a.mm = d_mm;
    a.spacer = spacer;
    a.n = n;
    a.cands = (uint32_t *)d_cands;
    a.counts = d_counts;
    hipLaunchKernelGGL(pg_variant_kernel, dim3((n + 3u) / 4u), dim3(256), 0, (hipStream_t)stream, *ref, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
