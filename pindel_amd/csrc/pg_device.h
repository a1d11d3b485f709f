// pg_device.h -- structures shared by the host API (pg_api.cpp) and the HIP
// kernels (pg_kernels.hip).  Not part of the public C ABI.
#ifndef PG_DEVICE_H
#define PG_DEVICE_H

#include <stdint.h>
#include "pindel_pg.h"

// Reference in HBM: three 1-bit planes per chromosome ("2-bit planar" + N plane),
// 32 bases per 32-bit word, indexed by AbsLoc (spacer-padded coordinates).
//   lo bit = code & 1, hi bit = code >> 1, code: A=0 C=1 G=2 T=3; nn bit = base is N.
// Every chromosome is preceded and followed by PG_GUARD_WORDS words of N so that a
// staged window may overhang either end without bounds checks.
#define PG_GUARD_WORDS 64u

struct PgDevRef {
    const uint32_t *lo;
    const uint32_t *hi;
    const uint32_t *nn;
    const uint64_t *chr_word_off;  // [n_chr] index of the word holding AbsLoc 0
    const uint32_t *chr_size;      // [n_chr] getCompSize()
    int32_t n_chr;
};

#define PG_MM_BREAKS_N 32
struct PgDevParams {
    int32_t max_range_index;
    int32_t add_mm;          // ADDITIONAL_MISMATCH
    int32_t min_perfect;     // Min_Perfect_Match_Around_BP
    int32_t min_close;       // g_MinClose
    uint32_t spacer;
    // g_maxMismatch as breakpoints (the table is monotone): mm(L) = #{k : L >= mm_bp[k]}
    uint32_t mm_bp[PG_MM_BREAKS_N];
};

enum PgMode { PG_MODE_CLOSE = 1, PG_MODE_FAR = 2, PG_MODE_BOTH = 3 };

// Packed per-read records.  pg_pack_reads builds the input records on the device from the SoA arrays of the C ABI;
// the delivery kernels (pg_deliver_chunk) turn the output records into the read-order CSR the C ABI hands out.
//
// The input record is 128 bytes = two lines of the scalar data cache (the second: the seed filter's symbol programs): the search kernel fetches it with scalar loads straight
// into SGPRs, and it holds everything about a read that is a function of (read, parameters) alone, worked out ONCE by the pack
// kernel -- a streaming kernel with every lane busy -- instead of by every wave's scalar unit at the start of every read (round 5:
// profiles/r05/everything_else_breakdown.txt; the CU's one scalar unit is the search kernel's tightest pipe):
//   * the close end's windows: GetCloseEndInner's (pindel.cpp:2250-2326) R = 1 window is [w1s, w1s + 3 isz), its R = 0 window
//     [w1s + isz, w1s + 2 isz) whichever the anchor's strand (w1s = anchor - isz for '+', anchor - 2 isz for '-'); whether the
//     R = 1 window fits one LDS chunk (all four attempts on one grid); the first window fill;
//   * the word offset and size of the anchor's chromosome (no table look-up, no fallback path);
//   * T = g_maxMismatch[len] + ADDITIONAL_MISMATCH + 1 mismatch levels, CheckMismatches' threshold, the seed filter's two
//     depths J (plain / wide windows) with their base masks bits [1, J) and relevance bounds min(T - 1, g_maxMismatch[J] + ADD);
//   * is the first consumed base of either orientation one of ACGT (farend_searcher.cpp:60-66; searcher.cpp:160).
#define PG_RF_CLOSE_OK 1u       // the close end is searched: len - 1 >= g_MinClose and MatchedD is '+' or '-'
#define PG_RF_PLUS 2u           // MatchedD == '+'
#define PG_RF_SHARED_GRID 4u    // 0 < 3 InsertSize <= PG_CHUNK
#define PG_RF_FIRST_OK_FWD 8u   // read[0] is one of ACGT (orientation 0: left to right)
#define PG_RF_FIRST_OK_REV 16u  // read[len - 1] is (orientation 1: from the last base)
#define PG_RF_EXACT 32u         // the read holds a character outside ACGTN: it is on the exact kernel's list (set by an atomic of the pack kernel)
// The seed filter in READ ORDER (round 6, pg_kernels.hip "seed_filter_ro"): the consumed bases 1 .. 3 G in groups of three, the one-hot
// plane of a base's symbol picked by VGPR index (s_set_gpr_idx): the symbols come as a PROGRAM, one dword per group -- byte k =
// 0x30 | symbol of base 3 g + 1 + k (A 0, C 1, G 2, T 3, N 4; the 0x3 nibble is the index mode's operand enables when a 16-bit field
// is moved into M0, and biases the index by 48), byte 3 = 0x30 (| symbol of base 0 in group 0: the seed).  prog[0] = the read left
// to right as it is, prog[1] = the read from its last base, COMPLEMENTED: the only two (orientation, complement) pairs any search
// consumes (kind F reads them as they are; kind B reads the complement, and its planes are laid out in complement order).
#define PG_RO_GROUPS_MAX 8
#define PG_RO_GROUPS_MIN 4
#define PG_RO_OK 0x80000000u     // PgInRec::ro: this read may take the read-order filter (<= 16 mismatch levels, >= 4 groups, ACGTN only
                                 // among the bases a program covers, g_MinClose >= 8)
struct PgInRec {
    // dwords 0 .. 11: fetched at the start of a read
    int32_t  w1s;           // AbsLoc where the close end's R = 1 window starts
    int32_t  isz;           // InsertSize
    int32_t  stage_s, stage_e;   // the first window fill covers positions [stage_s, stage_e) (+ overhangs); 0, 0: none
    uint32_t chr_wo_lo, chr_wo_hi;   // index of the word holding AbsLoc 0 of the anchor's chromosome in the reference planes
    uint32_t lenf;          // read length | PG_RF_* << 16
    uint32_t lvl;           // CheckMismatches' threshold (smallest n with (float)n >= (float)(len * u)) | g_maxMismatch[len] << 16 | T << 24
    uint32_t depth;         // J plain | J wide << 8 | bound plain << 16 | bound wide << 24
    uint32_t jmask0;        // bits [1, J plain)
    uint32_t ro;            // read-order filter: groups plain | groups wide << 4 | bound plain << 8 | bound wide << 16 | PG_RO_OK
                            // (bound = min(T - 1, g_maxMismatch[3 G + 1] + ADD): the depth the groups reach)
    int32_t  chr;           // chromosome of the anchor
    // dwords 12 .. 15: fetched at the start of the far end
    uint32_t chr_size;      // getCompSize() of that chromosome
    uint32_t bd_cnt;        // BreakDancer windows of this read ...
    uint32_t bd_off;        // ... starting at PgDevBatch::bd[bd_off]
    uint32_t jmask1;        // bits [1, J wide)
    // dwords 16 .. 31: fetched by a seed-filter run (one orientation)
    uint32_t prog[2][PG_RO_GROUPS_MAX];
};
#define PG_PACK_CLAIM 8u            // ... of a launch that packs in place (PgDevBatch::soa) ...
#define PG_PACK_CLAIM_LONG 16u      // ... and when a wave takes many of them (pg_launch_search)
#define PG_PACK_IN_PLACE_MIN 1u            // fewest reads of such a launch (measured 20 000 reads .. 10 M: never slower than a pack launch in front)
#define PG_CLAIM 8u          // reads a workgroup of the persistent launch claims per atomic, at most
#define PG_IN_PAD 8u        // records allocated behind the last one (the kernel prefetches the next read's record)
struct PgOutRec {
    uint32_t close_off, close_cnt, far_off, far_cnt;   // runs in the pool
    uint32_t close_last;    // getLastAbsLocCloseEnd()
    uint16_t close_max;     // MaxLenCloseEnd(), 0 = no close end
    uint8_t  rc_flag;       // GetCloseEnd left the read reverse-complemented
    uint8_t  pad;
    uint32_t alg;           // algorithmic bytes of this read
    uint32_t reserved;      // diagnostics: candidates (survivors of the seed filter) folded for this read
};

struct PgSoaIn;
struct PgDevBatch {
    uint32_t n_reads;
    uint32_t first_read;           // offset into the batch arrays handled by this launch
    const PgInRec *in;
    PgOutRec *out;                 // close-end fields: written in CLOSE/BOTH mode, read in FAR mode
    const uint8_t *seq;
    // The reads as bit planes, built once by pg_pack_reads (every lane busy) instead of per read in the search kernel
    // (ten byte compares and eight ballots of a single wave): per read u64[2 orientations][4 planes][plane_blocks],
    // orientation 0 = left to right, 1 = reversed; planes = code bit 0, code bit 1, is-N, is-other; bit j of block b =
    // base 64 b + j.
    const uint64_t *planes;
    uint32_t plane_blocks;         // 64-base blocks per read in `planes` (pg_plane_blocks of the batch's longest read)
    const pg_window *bd;           // BreakDancer windows (nullable)
    // Run pool, split into PG_POOL_SHARDS equal regions with one bump cursor each (a single
    // device-wide cursor saturates at ~88 M atomics/s, MI355X_MICROARCH.md "dequeue").  Workgroup b
    // allocates from shard b % PG_POOL_SHARDS; cursors are 64 bytes apart.
    pg_run *pool;
    uint32_t pool_shard_cap;       // runs per shard
    uint32_t *pool_used;           // [PG_POOL_SHARDS * 16]; cursor > pool_shard_cap means overflow (retry bigger)
    uint32_t *work_ctr;            // [PG_WORK_CTRS * 16] reads claimed per XCD part (zeroed before every launch)
    uint32_t claim;                // reads per claim (set by pg_launch_search: a workgroup's share in the fewest equal claims <= PG_CLAIM)
    // the reads with a character outside ACGTN (pg_pack_kernel appends, pg_search_exact_kernel searches them again with the
    // reference's read-shortening semantics) and CheckMismatches' threshold per read length (the exact kernel recomputes a read's
    // length-dependent fields)
    const uint32_t *exact_list;
    const uint32_t *exact_count;
    const uint16_t *thr_tab;       // [512]
    // PACK IN PLACE (pg_launch_search, BOTH mode): non-null = the records and planes of the launch's reads are built from these SoA
    // arrays (a PgSoaIn in device memory) by the search kernel itself, claim by claim, instead of by a pg_pack_reads launch before it
    const struct PgSoaIn *soa;
};

// SoA views for the pack kernels
static inline uint32_t pg_plane_blocks(uint32_t max_len)
{
    return max_len <= 64u ? 1u : (max_len <= 128u ? 2u : (max_len <= 192u ? 3u : (max_len <= 256u ? 4u : 8u)));
}
struct PgSoaIn {
    const uint8_t *seq;            // the reads' bases ...
    uint64_t *planes;              // ... and where their bit planes go (PgDevBatch::planes)
    uint32_t plane_blocks;
    const uint64_t *seq_off;
    const uint8_t *strand;
    const int32_t *pos;
    const int16_t *isz;
    const int32_t *chr;
    const uint64_t *bd_off;        // nullable
    uint32_t *exact_list;          // nullable: indices of the reads with a character outside ACGTN ...
    uint32_t *exact_count;         // ... and how many (zeroed by the caller before the batch's first pack)
    const struct PgLenRec *len_tab; // [512] the fields of a read's record that follow from its length alone (pg_len_rec)
    const uint64_t *chr_word_off;  // [n_chr] as PgDevRef
    const uint32_t *chr_size;      // [n_chr]
    uint32_t spacer;
    int32_t add_mm;                // ADDITIONAL_MISMATCH
    int32_t min_close;             // g_MinClose
};
// consumed bases the seed filter inspects for a read of `len` bases with T mismatch levels (wide: the chunks of wide far-end
// windows, where a survivor costs a whole candidate pass for a handful of candidates: two more)
#define PG_SEED_J(T) (2 * (T) + 4)
#define PG_SEED_J_WIDE 2
#ifdef __HIPCC__
__host__ __device__
#endif
static inline int pg_seed_depth(int len, int T, int wide)
{
    int J = len - 1 < 32 ? len - 1 : 32;
    const int jt = PG_SEED_J(T) + (wide ? PG_SEED_J_WIDE : 0);
    return J > jt ? jt : J;
}
// groups of three bases the read-order filter inspects (bases 1 .. 3 G): the depth above rounded to whole groups
#ifdef __HIPCC__
__host__ __device__
#endif
static inline int pg_ro_groups(int len, int T, int wide)
{
    const int J = pg_seed_depth(len, T, wide);
    int G = J / 3;                                    // (J - 1 bases: 15 -> 5 groups, 17 -> 6, 19 -> 6, 21 -> 7)
    if (G > PG_RO_GROUPS_MAX) G = PG_RO_GROUPS_MAX;
    while (G > 0 && 3 * G > len - 1) G--;
    return G;
}
// What PgInRec holds that is a function of the read's LENGTH and the search parameters alone (lvl, depth, jmask0, ro, jmask1): one
// table per context, built on the host when the context is created (the pack's per-read lane used to work these out -- two depths,
// two group counts, six table look-ups -- for every read; inside the search kernel that lane's instructions are paid for by a claim of
// eight reads).
struct PgLenRec { uint32_t lvl, depth, jmask0, ro, jmask1, pad[3]; };
static inline struct PgLenRec pg_len_rec(int len, const uint32_t *mm, const uint16_t *thr, int add_mm, int min_close)
{
    struct PgLenRec r;
    const uint32_t M = mm[len] & 0xffu, T = M + (uint32_t)add_mm + 1u;
    const int J0 = pg_seed_depth(len, (int)T, 0), J1 = pg_seed_depth(len, (int)T, 1);
    // relevance bound of a seed: min(T - 1, g_maxMismatch[J] + ADD)  (J >= 0; a one-base read has J = 0)
    uint32_t b0 = (mm[J0 < 0 ? 0 : J0] & 0xffu) + (uint32_t)add_mm, b1 = (mm[J1 < 0 ? 0 : J1] & 0xffu) + (uint32_t)add_mm;
    if (b0 > T - 1u) b0 = T - 1u;
    if (b1 > T - 1u) b1 = T - 1u;
    r.lvl = (uint32_t)thr[len] | (M << 16) | (T << 24);
    r.depth = (uint32_t)(J0 < 0 ? 0 : J0) | ((uint32_t)(J1 < 0 ? 0 : J1) << 8) | (b0 << 16) | (b1 << 24);
    r.jmask0 = J0 > 1 ? ((J0 >= 32 ? 0xffffffffu : (1u << J0) - 1u) & ~1u) : 0u;
    r.jmask1 = J1 > 1 ? ((J1 >= 32 ? 0xffffffffu : (1u << J1) - 1u) & ~1u) : 0u;
    // read-order filter (PgInRec::ro): whole groups of three bases, the relevance bound of the depth they reach
    const int G0 = pg_ro_groups(len, (int)T, 0), G1 = pg_ro_groups(len, (int)T, 1);
    uint32_t rb0 = (mm[3 * G0 + 1] & 0xffu) + (uint32_t)add_mm, rb1 = (mm[3 * G1 + 1] & 0xffu) + (uint32_t)add_mm;
    if (rb0 > T - 1u) rb0 = T - 1u;
    if (rb1 > T - 1u) rb1 = T - 1u;
    r.ro = (uint32_t)G0 | ((uint32_t)G1 << 4) | (rb0 << 8) | (rb1 << 16);
    if (T <= 16u && G0 >= PG_RO_GROUPS_MIN && G1 >= PG_RO_GROUPS_MIN && min_close >= 8) r.ro |= PG_RO_OK;     // (the close end's snapshot covers seven bases)
    r.pad[0] = r.pad[1] = r.pad[2] = 0u;
    return r;
}
// FIXED-LENGTH KERNELS (pg_search_fixed_kernel<NB, NS, LEN>): a sequencer produces reads of one length, and for a batch whose reads
// all have one of the lengths below -- under Pindel's default parameter set -- the length and every record field that follows
// from it (PgLenRec) are compile-time constants of the search kernel instead of scalar registers that live through the whole read.
// One literal row per built length: what pg_len_rec() gives for pg_default_params (tests/test_fixed_length_table.py compares
// them with the host's tables; pg_create compares the context's own and keeps to the other kernels on a mismatch).
struct PgFixedLen { uint32_t len, lvl, depth, jmask0, ro, jmask1; };
#define PG_FIXED_LENS 4
#define PG_FIXED_LEN_ROWS { \
    { 100u, 0x06040002u, 0x03031210u, 0x0000fffeu, 0x80030365u, 0x0003fffeu },   /* M 4, T 6, threshold 2; J 16 / 18; 5 / 6 groups */ \
    { 101u, 0x06040003u, 0x03031210u, 0x0000fffeu, 0x80030365u, 0x0003fffeu },   /* as 100, threshold 3 */ \
    { 150u, 0x07050003u, 0x03031412u, 0x0003fffeu, 0x80030366u, 0x000ffffeu },   /* M 5, T 7, threshold 3; J 18 / 20; 6 / 6 groups */ \
    { 151u, 0x07050004u, 0x03031412u, 0x0003fffeu, 0x80030366u, 0x000ffffeu },   /* as 150, threshold 4 */ \
}
// the row of `len` (len = 0 when it is none of the built lengths)
#ifdef __HIPCC__
__host__ __device__
#endif
constexpr PgFixedLen pg_fixed_len_row(uint32_t len)
{
    constexpr PgFixedLen rows[PG_FIXED_LENS] = PG_FIXED_LEN_ROWS;
    for (int k = 0; k < PG_FIXED_LENS; k++)
        if (rows[k].len == len) return rows[k];
    return PgFixedLen{ 0u, 0u, 0u, 0u, 0u, 0u };
}
struct PgSoaOut {                  // the close-end summary pg_pack_close_summary reads
    uint8_t *rc_flag;
    uint32_t *close_last;
    uint16_t *close_max;
};

// Candidate id = position relative to the search origin | kind (F/B) | window index of a BreakDancer cluster.
//   64-bit ids: rel(26) | kind(1) | region(7)   -- any window the ABI accepts
//   32-bit ids: rel(24) | kind(1) | region(7)   -- every search window of the launch has <= 2^24 positions
#define PG_REL_BITS 26
#define PG_REL_BITS_SMALL 24
#define PG_SMALL_MAX_WINDOW (1 << 24)
#define PG_SMALL_MAX_CLUSTER 127u   // windows per read the 32-bit ids can tell apart
#define PG_MAX_LEVELS 32
#define PG_MM_BREAKS 32
#define PG_POOL_SHARDS 1024u
#define PG_WORK_CTRS 8u           // per-XCD read counters of the persistent launch, 64 bytes apart
#define PG_DIAG_WORDS 64u         // behind the read counters: cycle accumulators of a -DPG_TIMING diagnostics build
// Run-pool slots a workgroup reserves per claimed read with ONE atomic per claim (instead of one or two dependent
// atomic round trips inside every read): the first PG_RES_CLOSE for the read's UP_Close runs, the rest for its UP_Far
// runs (1.04 / 1.03 runs on average); a list that does not fit takes an allocation of its own.
#define PG_RES_CLOSE 4u
#define PG_RES_FAR 4u
#define PG_RESERVE (PG_RES_CLOSE + PG_RES_FAR)

#define PG_CHUNK 2048u            // window positions staged per LDS fill (= 64 lanes x 32-base words)
#define PG_CHUNK_SHIFT 11
#define PG_EQ_ROWS 5u
// LDS window capacity in 32-base words: chunk(s) + overhang of nb 64-base blocks on both sides + slack.  Reads of
// up to 192 bases (nb <= 3) take the chunks of wide far-end windows two at a time; longer reads keep one chunk per
// fill, where the extra KB of LDS would cost a resident wave per SIMD.
#define PG_PAIR_CHUNKS(nb) ((nb) <= 3)
#define PG_WIN_WORDS(nb) (((PG_PAIR_CHUNKS(nb) ? 2u : 1u) * PG_CHUNK + 2u * (64u * (nb))) / 32u + 6u)
// ... of which this many are STATIC LDS.  For reads of 65..192 bases (nb = 2, 3) the second chunk's words are dynamic LDS that only
// launches with -x >= 3 ask for: the static part then fits 28 (nb = 2: 5120 B) or 24 (nb = 3: 6384 B) workgroups per CU -- seven or
// six waves per SIMD -- at the default -x 2, where nothing takes two chunks per fill (a cluster window of more than a chunk
// goes chunk by chunk).  The dynamic part starts where the static LDS ends (the window is the last member of the kernel's one
// static LDS object), so the window stays one array with compile-time addresses.
// (LDS is handed out in granules of 1280 bytes on gfx950 -- hence + 4 words of slack here, not + 6: a fill writes
// (2048 + 128 nb) / 32 + 2 words -- 74 / 78 -- and a candidate reads up to word 4 nb + 63 of a one-chunk window)
#define PG_WIN_STATIC_WORDS(nb) ((nb) == 3 || (nb) == 2 ? (PG_CHUNK + 2u * (64u * (nb))) / 32u + 4u : PG_WIN_WORDS(nb))
#define PG_WIN_DYN_BYTES(nb) ((PG_WIN_WORDS(nb) - PG_WIN_STATIC_WORDS(nb)) * 16u)

// Environment switches of tests and experiments, read once per process by pg_api.cpp (pg_debug_reload_env() re-reads them)
struct PgEnvSwitches {
    uint32_t host_chunk;        // PG_HOST_CHUNK: reads per chunk of the host path (0 = the default schedule)
    uint32_t lds_pad;           // PG_LDS_PAD: extra dynamic LDS per workgroup (lowers occupancy), bytes
    bool no_single_block;       // PG_NO_SINGLE_BLOCK: no one-copy delivery of one-chunk batches
    bool tiny_delivery;         // PG_TEST_TINY_DELIVERY: forces the delivery-overflow fallback
    bool tiny_pool;             // PG_TEST_TINY_POOL: forces the run-pool regrow path
    bool force_wide_cells;      // PG_FORCE_WIDE_CELLS: 64-bit candidate ids
    bool split_launch;          // PG_SPLIT_LAUNCH: close end and far end as two launches
    bool generic_kernels;       // PG_GENERIC_KERNELS: never the default-parameter kernels
    bool no_pack_in_place;      // PG_NO_PACK_IN_PLACE: pg_device_batch_pack_search = pack launch + search launch
    uint32_t pack_claim;        // PG_PACK_CLAIM: reads per claim of a launch that packs in place (0 = the default)
    uint32_t pack_in_place_min; // PG_PACK_IN_PLACE_MIN: fewest reads of such a launch (tests: the path on small batches)
    bool no_fixed_len;          // PG_NO_FIXED_LEN: never the fixed-length kernels (same-process A/B runs)
};

#ifdef __cplusplus
extern "C" {
#endif
const struct PgEnvSwitches *pg_env_switches(void);
// TEST HOOK: not synchronised with readers -- call it only while no pg_* call is in flight on any thread.
void pg_debug_reload_env(void);
// number of kernel arguments whose value fetched from the kernarg segment at PgKArgs' offsets differs from the by-value one (0)
int pg_debug_kargs_check(const PgDevRef *ref, const PgDevParams *prm, const PgDevBatch *batch, uint32_t max_len, uint32_t levels,
                         uint32_t *scratch_dev, void *stream);
// What one kernel launch on the search path ran (the launch log of pg_api.cpp, pg_debug_launch_log): the kernel and its
// template arguments.  The launch functions below fill these when given somewhere to put them (null: nothing is recorded).
enum PgKernelKind { PG_KERNEL_SEARCH = 1, PG_KERNEL_EXACT = 2, PG_KERNEL_PACK = 3, PG_KERNEL_VARIANT = 4, PG_KERNEL_SV = 5,
                    PG_KERNEL_EVENT_CASCADE = 6, PG_KERNEL_EVENT_SORT = 7, PG_KERNEL_EVENT_TABLES = 8, PG_KERNEL_SV_EVENTS = 9 };
enum { PG_KERNEL_REPORT = 10 };    // ... continued: the report kernels of pg_report.hip (blocks 0: the list cut of pg_device_batch_classify)
struct PgLaunchRec {
    int32_t kernel;                // PgKernelKind
    int32_t blocks;                // NB of pg_search_kernel, PB of pg_pack_kernel (0: pg_search_exact_kernel)
    int32_t ns;                    // counter slices of pg_search_kernel (0 otherwise)
    int32_t id_bits;               // 32 / 64: candidate ids of pg_search_kernel (0 otherwise)
    int32_t mode;                  // PgMode of the search and exact kernels (0: the pack)
    int32_t def;                   // pg_search_kernel of the default-parameter family
    int32_t in_place;              // the search launch built its reads' records itself (PgDevBatch::soa)
};
#define PG_LAUNCH_RECS_MAX 2       // records one pg_launch_search writes at most (PG_SPLIT_LAUNCH: close kernel, far kernel)
// Launches the search kernel for the reads of the batch on `stream`.  small_ids selects the
// 32-bit candidate ids (see above for when that is valid).  rec (may be null): room for PG_LAUNCH_RECS_MAX records of the
// kernels launched, *n_rec their number.  uniform_len: the one length every read of the launch has, if the caller vouches for
// it and for the length tables being the baked ones (0: lengths unknown or mixed) -- the launch may then run a fixed-length kernel;
// *fixed_len (may be null): the LEN of the one it ran, 0 for any other kernel.
int pg_launch_search(const PgDevRef *ref, const PgDevParams *prm, const PgDevBatch *batch,
                     int mode, uint32_t max_len, uint32_t levels, int small_ids, void *stream,
                     struct PgLaunchRec *rec, int *n_rec, uint32_t uniform_len, uint32_t *fixed_len);
// may that launch build the records of its reads itself (PgDevBatch::soa) ?
// -q: contains_subseq_any_strand per item (pg_dd.hip); n_tasks = 2 x items (strand = task & 1), out2[task]; workgroups of four
// waves, each wave with scratch_stride words of d_scratch (the boundary row between its 64-row blocks).
int pg_dd_launch(const PgDevRef *ref, const uint32_t *d_mm, const uint8_t *d_query, const uint64_t *d_query_off, const int32_t *d_chr,
                 const uint64_t *d_ws, const uint32_t *d_wl, uint8_t *d_out2, uint32_t *d_scratch, uint64_t scratch_stride, uint32_t n_tasks,
                 uint32_t n_blocks, void *stream);
int pg_pack_in_place_ok(int mode, uint32_t max_len, int small_ids, uint32_t n_reads, uint32_t plane_blocks);
// The device classifier (pg_variant.hip): deletion and short-insertion candidates of the n reads of a searched batch, one wave per
// read -- the output records and run pool of its last search, its reads as uploaded (seq, seq_off, strand, chr) and g_maxMismatch
// (512 entries); d_cands: n x 2 x PG_VARIANT_CANDS records, d_counts: n x 2 bytes.  n = 0 launches nothing.
int pg_variant_launch(const PgDevRef *ref, const PgOutRec *out, const pg_run *pool, unsigned long long pool_runs, const uint8_t *seq,
                      const uint64_t *seq_off, const uint8_t *strand, const int32_t *chr, const uint32_t *d_mm, uint32_t spacer,
                      uint32_t n, pg_variant_cand *d_cands, uint8_t *d_counts, void *stream);
// The device classifier of the five other kinds (pg_sv.hip): the inputs of pg_variant_launch plus d_budget -- the
// mismatch budget of the kinds with non-template bases by length sum, PG_SV_BUDGET_N entries made on the host -- and -d and -v;
// d_cands: n x PG_SV_SLOTS records, d_counts: n x PG_SV_KINDS bytes.  n = 0 launches nothing.
#define PG_SV_BUDGET_N 1024
int pg_sv_launch(const PgDevRef *ref, const PgOutRec *out, const pg_run *pool, unsigned long long pool_runs, const uint8_t *seq,
                 const uint64_t *seq_off, const uint8_t *strand, const int32_t *chr, const uint32_t *d_mm, const int32_t *d_budget,
                 int32_t min_matched, uint32_t min_inv, uint32_t spacer, uint32_t n, pg_variant_cand *d_cands, uint8_t *d_counts, void *stream);
// Position-keyed hint tables (pg_hints.hip): a pg_hint_table in device memory, its windows already split into pieces of at most
// 2^26 - 1 positions, and per cluster the longest of its windows.  pg_hint_count_scan: the reads' window counts scanned into
// bd_off (n + 1 offsets) -- blk: scratch of pg_hint_scan_blocks(n) words; info (4 dwords): the total (64 bits), the most windows
// of one read (saturated at 2^32 - 1), the longest window used.  pg_hint_fill: bd[bd_off[i] .. bd_off[i + 1]) = read i's windows.
struct PgDevHintTable {
    uint32_t n_runs;
    const uint32_t *run_first;       // n_runs + 1
    const uint32_t *run_cluster;     // n_runs
    const uint64_t *cluster_off;     // n_clusters + 1
    const uint32_t *cluster_longest; // n_clusters: positions of the cluster's longest window (0: none)
    const pg_window *windows;
};
#define PG_HINT_SCAN_TILE 1024u      // counts per workgroup of the scan
static inline uint32_t pg_hint_scan_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + 1u + PG_HINT_SCAN_TILE - 1u) / PG_HINT_SCAN_TILE); }
int pg_hint_count_scan(const struct PgDevHintTable *t, const uint32_t *close_last, const uint16_t *close_max, uint32_t n,
                       unsigned long long *bd_off, unsigned long long *blk, uint32_t *info, void *stream);
int pg_hint_fill(const struct PgDevHintTable *t, const uint32_t *close_last, const uint16_t *close_max, uint32_t n,
                 const unsigned long long *bd_off, pg_window *bd, void *stream);
// ... then the reads on the batch's exact list that lie in the launch's range, with the reference's read-shortening semantics
// (rec may be null; rec->kernel stays 0 when nothing was launched)
int pg_launch_search_exact(const PgDevRef *ref, const PgDevParams *prm, const PgDevBatch *batch, int mode,
                           uint32_t max_len, uint32_t levels, void *stream, struct PgLaunchRec *rec);
// in[lo .. lo + cnt) from the SoA input arrays; cnt = 0 is allowed (rec may be null; rec->kernel stays 0 when nothing was launched)
int pg_pack_reads(const PgSoaIn *soa, PgInRec *in, uint32_t lo, uint32_t cnt, void *stream, struct PgLaunchRec *rec);
// close-end summary (rc flag, last AbsLoc, max length) of a host result into the output records
int pg_pack_close_summary(const PgSoaOut *soa, PgOutRec *out, uint32_t n, void *stream);
// ... and out of the output records a close launch wrote into the batch's summary arrays (the records are left as they are)
int pg_unpack_close_summary(const struct PgOutRec *out, const PgSoaOut *soa, uint32_t n, void *stream);
// One chunk (cnt <= PG_DELIVER_CHUNK reads) of a searched batch to read-order CSR behind the earlier chunks: see the
// delivery kernels in pg_kernels.hip.  local / blk: scratch of cnt and 4096 uint2; run_tot: 2 running totals (zeroed
// per batch); info: 8 values for the host {close base, far base, close runs, far runs, fullest pool shard, overflow}.
#define PG_DELIVER_CHUNK (1u << 20)     // reads a delivery handles at most (scan2: 4096 blocks of 256)
#define PG_HOST_CHUNK (1u << 18)        // reads per chunk the host path starts from (and the largest batch that is ONE chunk)
int pg_deliver_chunk(const PgOutRec *out, uint32_t cnt, uint8_t *rc_flag, uint32_t *close_last, uint16_t *close_max,
                     void *local, void *blk, unsigned long long *run_tot, unsigned long long *info,
                     const pg_run *pool, unsigned long long pool_runs, pg_run *close_runs, pg_run *far_runs /* null: behind the close runs */,
                     unsigned long long cap, unsigned long long *close_off, unsigned long long *far_off, const uint32_t *pool_used,
                     void *stream);
// ... and its two halves: the scan (summaries, local / blk, info, the running totals) needs no run buffers; the gather writes the
// offsets and copies the runs of a chunk whose local / blk / info the scan has left in place.
int pg_deliver_scan(const PgOutRec *out, uint32_t cnt, uint8_t *rc_flag, uint32_t *close_last, uint16_t *close_max,
                    void *local, void *blk, unsigned long long *run_tot, unsigned long long *info, const uint32_t *pool_used, void *stream);
int pg_deliver_gather_runs(const PgOutRec *out, uint32_t cnt, const void *local, const void *blk, unsigned long long *info,
                           const pg_run *pool, unsigned long long pool_runs, pg_run *close_runs, pg_run *far_runs /* null: behind the close runs */,
                           unsigned long long cap, unsigned long long *close_off, unsigned long long *far_off, void *stream);
// The device-buffer entries (pg_devio.hip).  Every pointer is device memory the host has already checked.
// What one pass over a batch's arrays in device memory yields (pg_devio_measure_reads): the host initialises it -- first_bad =
// PG_MEASURE_NONE, len_max = 0, len_min = ~0, isz_max = 0 -- and reads it back, 40 bytes.
#define PG_MEASURE_NONE (~0ull)
struct PgReadMeasure {
    unsigned long long first_bad;      // (read index << 8) | code of the bad read with the lowest index (codes: validate_and_measure)
    unsigned long long off0, offn;     // seq_off[0], seq_off[n]
    uint32_t len_max, len_min;         // over the good reads: equal when the batch has ONE read length
    int32_t isz_max;                   // largest insert size (at least 0)
    uint32_t reserved;
};
// words [0, (len + 31) / 32) of a chromosome's planes (lo / hi / nn point at its first word) from its len ASCII bases
int pg_devio_pack_reference(const uint8_t *d_seq, unsigned long long len, uint32_t *lo, uint32_t *hi, uint32_t *nn, void *stream);
// off_out: n + 1 offsets rebased to 0; n = 0 launches nothing
int pg_devio_measure_reads(const unsigned long long *seq_off, const int32_t *pos, const int16_t *isz, const int32_t *chr, uint32_t n,
                           const uint32_t *chr_size, int32_t n_chr, uint32_t spacer, unsigned long long *off_out,
                           struct PgReadMeasure *rec, void *stream);
// *close_end / *far_end = the batch's run totals, from the 8 info values pg_deliver_scan left for its last chunk
int pg_devio_store_totals(const unsigned long long *info, unsigned long long *close_end, unsigned long long *far_end, void *stream);
// Event tables (pg_events.hip): the window tail and cascade per read, the order of the boxed reads of the four
// sorted kinds, duplicates and events.  Every pointer is device memory of the library's own or one the host has checked.
#define PG_EV_BLOCK 256u              // the scan / sort block: reads (records) per workgroup of the count, rank and scatter kernels
// The scan stages every table build shares (pg_table_prims.hip; they launch and return, errors surface at the caller's hipGetLastError):
// rank[i] = flagged elements of flag[0 .. m) before i in its block, then blk[0 .. blocks) to its exclusive scan, blk[blocks] = the total
void pg_table_rank_scan_launch(const uint8_t *flag, uint32_t m, uint32_t *rank, uint32_t *blk, void *stream);
// a[0 .. m) to its exclusive scan in place, a[m] = the total (one workgroup; the array has m + 1 entries)
void pg_table_scan_launch(uint32_t *a, uint32_t m, void *stream);
#define PG_EV_SORT_PASSES 17          // one per key byte, least significant first: BP (2), NT_size (2), IndelSize, BPRight, BPLeft (4 each), table
struct PgEventRec { uint32_t w[8]; }; // one boxed read: BPLeft, BPRight, IndelSize, NT_size << 16 | (BP ^ 0x8000), Left, Right, read, table | plus << 8 | ReadLength << 16
struct PgEventInfo {                  // what the host reads back, 96 bytes
    uint32_t n_boxed;                 // boxed reads of the four tables
    uint32_t n_unresolved;
    uint32_t key_or[5], key_and[5];   // over the boxed records' key words w[0..3] and the table: a byte equal in both is constant
    uint32_t n_members, n_events;
    uint32_t member_start[PG_EVENT_TABLES + 1], event_start[PG_EVENT_TABLES + 1];
};
struct PgEventArgs {
    const PgOutRec *out;
    const pg_run *pool;
    unsigned long long pool_runs;
    const uint8_t *seq;
    const uint64_t *seq_off;
    const uint8_t *strand;
    const int32_t *chr;
    const int16_t *isz;
    uint32_t spacer, n;
    pg_event_window win;
    uint32_t box_size, n_boxes;
    const pg_variant_cand *cands;     // n x 2 x PG_VARIANT_CANDS, or null
    const uint8_t *counts;
    const pg_variant_cand *sv_cands;  // n x PG_SV_SLOTS, or null
    const uint8_t *sv_counts;
    const uint32_t *name_id;          // or null
    pg_event_read *reads;             // n
    uint32_t *members;                // n
    pg_event *events;                 // n
    struct PgEventRec *rec_a, *rec_b; // n each
    uint8_t *flag;                    // n
    uint32_t *rank, *blk;             // n; n / PG_EV_BLOCK + 2
    uint32_t *midx, *efirst;          // n; n + 1
    uint32_t *digit_cnt;              // 256 x (n / PG_EV_BLOCK + 1)
    struct PgEventInfo *info;
};
// stage A and the compaction of the boxed reads into rec_b (descending read index); info->n_boxed and the key masks are then valid
int pg_events_cascade_launch(const struct PgEventArgs *a, void *stream);
// one stable counting pass over key byte `pass` of src[0 .. n_boxed) into dst
int pg_events_sort_pass_launch(const struct PgEventArgs *a, const struct PgEventRec *src, struct PgEventRec *dst, uint32_t n_boxed, int pass,
                               void *stream);
// stages C and D over the sorted records; fills members, events and the rest of info
int pg_events_tables_launch(const PgDevRef *ref, const struct PgEventArgs *a, const struct PgEventRec *sorted, uint32_t n_boxed, void *stream);
// SV event tables (pg_sv_events.hip): DI, INV and INV_NT from the per-read records of the events build.  The boxed
// records stay where the compaction put them (ascending read index); what is sorted are permutations of their places.
#define PG_SVEV_LDS_BOX 640u          // reads of a box the order kernel keeps in LDS (rank + place: 8 bytes each, 4 granules of 1280 bytes)
#define PG_SVEV_KEY_WORDS 5           // DI: BPLeft, BPRight, NT_size << 16 | BP biased, 0, 0.  INV / INV_NT: BPLeft + BPRight, ~IndelSize, BPLeft,
                                      // BPRight, (NT_size << 16 for INV_NT) | BP biased
#define PG_SVEV_PASS_TABLE 20         // sort passes: 0 .. 19 the key bytes, least significant first; 20 the table (key sort);
#define PG_SVEV_PASS_BOX 21           // 21 .. 23 the bytes of the box, 24 the table (segment sort)
#define PG_SVEV_PASS_SEG_TABLE 24
// one boxed read: BPLeft, BPRight, IndelSize, NT_size << 16 | (BP ^ 0x8000), read, table | plus << 8 | ReadLength << 16, LeftMostPos, box | table << 24
struct PgSvEventRec { uint32_t w[8]; };
struct PgSvEventInfo {                // what the host reads back
    uint32_t n_boxed, n_segs, n_members, n_runs;
    uint32_t n_mem[PG_SV_EVENT_TABLES], n_ev[PG_SV_EVENT_TABLES], dropped[PG_SV_EVENT_TABLES];
    uint32_t seg_or, seg_and;         // over w[7] of the boxed records: a byte equal in both is constant
    uint32_t key_or[PG_SVEV_KEY_WORDS], key_and[PG_SVEV_KEY_WORDS];
};
struct PgSvEventArgs {
    const PgOutRec *out;
    const uint8_t *seq;
    const uint64_t *seq_off;
    const uint8_t *strand;
    uint32_t spacer, n;
    pg_event_window win;              // the events build's
    uint32_t box_size;
    const pg_variant_cand *sv_cands;  // n x PG_SV_SLOTS
    const pg_event_read *reads;       // n: the events build's records
    uint32_t *members;                // n
    pg_event *events;                 // n
    uint32_t *ws_rank;                // n: the ranks of boxes above PG_SVEV_LDS_BOX (kept with the batch)
    struct PgSvEventRec *rec_a, *rec; // n each: by read; compacted in ascending read index
    uint8_t *flag, *dupf;             // n each
    uint32_t *rank, *blk;             // n; n / PG_EV_BLOCK + 2
    uint32_t *perm_a, *perm_b;        // n each: places in (table, box) segments, arrival order within a segment
    uint32_t *kperm_a, *kperm_b;      // n each: places by (table, key)
    uint32_t *krank;                  // n: dense rank of a place's key within its table
    uint32_t *seg_first, *midx, *rfirst;   // n + 1; n; n + 1
    uint32_t *rmx;                    // n: a run's largest IndelSize
    uint8_t *rfail;                   // n: a member of the run fails the harmonisation test
    uint32_t *digit_cnt;              // 256 x (n / PG_EV_BLOCK + 2) + 1
    struct PgSvEventInfo *info;
};
// the boxed reads of the three kinds compacted into rec, the identity in perm_a and kperm_a; info->n_boxed and the masks are then valid
int pg_sv_events_gather_launch(const struct PgSvEventArgs *a, void *stream);
// one stable counting pass of the places src[0 .. n_boxed) over digit `pass` of their records into dst
int pg_sv_events_sort_pass_launch(const struct PgSvEventArgs *a, const uint32_t *src, uint32_t *dst, uint32_t n_boxed, int pass, void *stream);
// ranks, segments, the record-shift passes per box (perm is permuted in place), duplicates, members, runs and events
int pg_sv_events_tables_launch(const PgDevRef *ref, const struct PgSvEventArgs *a, uint32_t *perm, const uint32_t *kperm, uint32_t n_boxed,
                               void *stream);
// Report records (pg_report.hip): one pg_report_read per member of the seven member lists and one pg_report_summary
// per read, from the two table builds, the lists they were given and the run pool.
#define PG_REPORT_TABLES (PG_EVENT_TABLES + PG_SV_EVENT_TABLES)
struct PgReportArgs {
    const PgOutRec *out;
    const pg_run *pool;
    unsigned long long pool_runs;
    const uint8_t *strand;
    uint32_t n;
    uint32_t start[PG_REPORT_TABLES + 1];   // member i lies in table t with start[t] <= i < start[t + 1]; start[PG_EVENT_TABLES] = the events build's total
    const pg_variant_cand *cands;     // n x 2 x PG_VARIANT_CANDS
    const uint8_t *counts;
    const pg_variant_cand *sv_cands;  // n x PG_SV_SLOTS
    const uint8_t *sv_counts;
    const pg_event_read *reads;       // n: the events build's records
    const uint32_t *ev_members;       // the four member lists back to back
    const uint32_t *sv_members;       // the three member lists back to back
    pg_report_read *records;          // start[PG_REPORT_TABLES]
    pg_report_summary *summaries;     // n
};
// the summaries of the n reads and the records of the members; n = 0 and "no members" launch nothing that indexes an empty array
int pg_report_launch(const struct PgReportArgs *a, void *stream);
// the count bytes of n reads cut to max_listed pairs (pg_device_batch_classify); n = 0 launches nothing
int pg_report_cut_launch(uint8_t *counts, uint8_t *sv_counts, uint32_t n, uint32_t max_listed, void *stream);
// Long-insertion position tables (pg_li.hip): the reads with a close end and no far end that the events build left
// unused, compacted in ascending read index, ordered by (strand, clamped position) with stable counting passes, then positions.
enum { PG_KERNEL_LI = 11 };           // ... continued: the launch-log id of pg_device_batch_li
#define PG_LI_SORT_PASSES 5           // the four bytes of the position, least significant first, then the strand
struct PgLiRec { uint32_t w[4]; };    // one LI read: clamped position, read, strand (0 '+', 1 '-'), PG_LI_* of this read
struct PgLiInfo {                     // what the host reads back
    uint32_t n_li;                    // LI reads of both strands
    uint32_t n_plus;                  // ... of them with a '+' anchor
    uint32_t key_or[2], key_and[2];   // over w[0] and w[2] of the compacted records: a byte equal in both is constant
    uint32_t n_pos, pos_plus;         // positions of both strands; of the '+' strand
};
struct PgLiArgs {
    const PgOutRec *out;
    unsigned long long pool_runs;
    const uint8_t *seq;
    const uint64_t *seq_off;
    const uint8_t *strand;
    const int32_t *chr;
    const pg_event_read *reads;       // n: the events build's records
    uint32_t n;
    int32_t chr_id;                   // the events build's window chr_id
    uint32_t lo, hi;
    uint32_t *members;                // n
    pg_li_pos *positions;             // n
    struct PgLiRec *rec_a, *rec_b;    // n each
    uint8_t *flag;                    // n
    uint32_t *rank, *blk;             // n; n / PG_EV_BLOCK + 2
    uint32_t *pfirst;                 // n + 1
    uint32_t *digit_cnt;              // 256 x (n / PG_EV_BLOCK + 2) + 1
    struct PgLiInfo *info;
};
// the LI reads flagged and compacted into rec_b (ascending read index); info->n_li, n_plus and the key masks are then valid
int pg_li_gather_launch(const struct PgLiArgs *a, void *stream);
// one stable counting pass over key byte `pass` of src[0 .. n_li) into dst
int pg_li_sort_pass_launch(const struct PgLiArgs *a, const struct PgLiRec *src, struct PgLiRec *dst, uint32_t n_li, int pass, void *stream);
// head flags, members, positions over the sorted records; fills the rest of info.  n_li > 0
int pg_li_tables_launch(const struct PgLiArgs *a, const struct PgLiRec *sorted, uint32_t n_li, uint32_t n_plus, void *stream);
// Interchromosomal junction tables (pg_int.hip): the reads whose far end lies on another chromosome and whose points
// carry a call, compacted in ascending read index, ordered by the call's key with stable counting passes, then one record per call.
enum { PG_KERNEL_INT = 12 };          // ... continued: the launch-log id of pg_device_batch_int
#define PG_INT_KEY_WORDS 5            // w[0 .. 4] of a record, least significant first
#define PG_INT_SORT_PASSES 17         // one per key byte: nt (4), far_abs (4), close_abs (4), flags (1), the chromosomes (4)
// one read with a call: nt_off << 16 | nt_len, far_abs, close_abs, flags, chr << 16 | far_chr, read, 0, 0
struct PgIntRec { uint32_t w[8]; };
struct PgIntInfo {                    // what the host reads back
    uint32_t n_mem;                   // reads with a call
    uint32_t n_calls;
    uint32_t key_or[PG_INT_KEY_WORDS], key_and[PG_INT_KEY_WORDS];   // over the compacted records' key words: a byte equal in both is constant
};
struct PgIntArgs {
    const PgOutRec *out;
    const pg_run *pool;
    unsigned long long pool_runs;
    const uint8_t *seq;
    const uint64_t *seq_off;
    const uint8_t *strand;
    const int32_t *chr;
    const int32_t *chr_rank;          // n_chr, device memory
    uint32_t n, n_chr;
    uint32_t *members;                // n
    pg_int_call *calls;               // n
    struct PgIntRec *rec_a, *rec_b;   // n each
    uint8_t *flag;                    // n
    uint32_t *rank, *blk;             // n; n / PG_EV_BLOCK + 2
    uint32_t *cfirst;                 // n + 1
    uint32_t *digit_cnt;              // 256 x (n / PG_EV_BLOCK + 2) + 1
    struct PgIntInfo *info;
};
// the reads with a call flagged and compacted into rec_b (ascending read index); info->n_mem and the key masks are then valid.  n > 0
int pg_int_gather_launch(const struct PgIntArgs *a, void *stream);
// one stable counting pass over key byte `pass` of src[0 .. n_mem) into dst
int pg_int_sort_pass_launch(const struct PgIntArgs *a, const struct PgIntRec *src, struct PgIntRec *dst, uint32_t n_mem, int pass, void *stream);
// head flags, members, calls over the sorted records; fills info->n_calls.  n_mem > 0
int pg_int_tables_launch(const struct PgIntArgs *a, const struct PgIntRec *sorted, uint32_t n_mem, void *stream);
// Dispersed-duplication breakpoint tables and consensus (pg_dd_tables.hip): the reads of the caller's segments that pass
// the DD test, compacted in ascending read index, ordered by (seg, pos) with stable counting passes; the keys with enough support
// become candidates, one wave per candidate votes its consensus, and the containment kernel runs over the packed pool.
enum { PG_KERNEL_DD_TABLES = 13 };    // ... continued: the launch-log id of pg_device_batch_dd
#define PG_DD_KEY_WORDS 2             // w[0] = seg, w[1] = pos
#define PG_DD_SORT_PASSES 8           // one per key byte, least significant first: pos (4), seg (4)
#define PG_DD_MIN_CONSENSUS 15u       // MIN_CONSENSUS_LENGTH, src/search_MEI.cpp:38
#define PG_DD_WAVES 4u                // candidates per workgroup of the consensus and pool kernels (one wave each)
struct PgDdRec { uint32_t w[4]; };    // one DD read: seg, pos, read, close_len | rc_flag << 16
struct PgDdAux {                      // one member as the consensus kernel reads it
    uint64_t base;                    // offset in seq of the first byte of the read's post-state
    uint32_t len;                     // the post-state's length
    uint32_t u_rc;                    // u = len - close_len | rc_flag << 16
};
struct PgDdInfo {                     // what the host reads back
    uint32_t n_dd;                    // DD reads
    uint32_t n_keys, n_mem, n_cands;  // distinct (seg, pos); members and candidates kept
    uint32_t cons_bytes, max_cons, n_tested;
    uint32_t key_or[PG_DD_KEY_WORDS], key_and[PG_DD_KEY_WORDS];   // over the compacted records' key words: a byte equal in both is constant
};
struct PgDdArgs {
    const PgOutRec *out;
    const uint8_t *seq;
    const uint64_t *seq_off;
    const uint8_t *strand;
    const uint32_t *seg_first;        // n_seg + 1, device memory
    const uint8_t *seg_strand;        // n_seg, device memory
    uint32_t n, n_seg;
    int32_t chr_id, min_bp_support, min_map_distance;
    uint32_t chr_size;                // the padded length of chr_id
    uint32_t slot;                    // bytes per candidate of `slots`: the longest read of the batch
    pg_dd_member *members;            // info.n_mem
    pg_dd_cand *cands;                // info.n_cands
    uint8_t *cons;                    // info.cons_bytes
    struct PgDdRec *rec_a, *rec_b;    // n each
    struct PgDdAux *aux;              // n
    uint8_t *flag, *keep, *keep_head; // n each
    uint32_t *rank, *blk;             // n; n / PG_EV_BLOCK + 2 -- of flag
    uint32_t *rank_m, *blk_m;         // ... of keep
    uint32_t *rank_c, *blk_c;         // ... of keep_head
    uint32_t *cfirst;                 // n + 1
    uint32_t *digit_cnt;              // 256 x (n / PG_EV_BLOCK + 2) + 1
    uint8_t *slots;                   // info.n_cands x slot: the accepted columns per candidate
    uint32_t *cons_off;               // info.n_cands + 1: the lengths, then their scan
    // the containment kernel's items, one per candidate (an untested one has a query of no bytes and a window of none)
    uint64_t *q_off;                  // info.n_cands + 1
    int32_t *q_chr;                   // info.n_cands
    uint64_t *q_ws;
    uint32_t *q_wl;
    uint8_t *q_out;                   // 2 x info.n_cands
    struct PgDdInfo *info;
};
// the DD reads flagged and compacted into rec_b (ascending read index); info->n_dd and the key masks are then valid.  n > 0
int pg_ddt_gather_launch(const struct PgDdArgs *a, void *stream);
// one stable counting pass over key byte `pass` of src[0 .. n_dd) into dst
int pg_ddt_sort_pass_launch(const struct PgDdArgs *a, const struct PgDdRec *src, struct PgDdRec *dst, uint32_t n_dd, int pass, void *stream);
// head flags, firsts and counts over the sorted records, the keys with enough support flagged; fills info->n_keys / n_mem / n_cands.  n_dd > 0
int pg_ddt_keys_launch(const struct PgDdArgs *a, const struct PgDdRec *sorted, uint32_t n_dd, void *stream);
// members, candidates (without the consensus fields) and the members' aux records.  n_dd > 0, members / cands / aux allocated
int pg_ddt_tables_launch(const struct PgDdArgs *a, const struct PgDdRec *sorted, uint32_t n_dd, void *stream);
// one wave per candidate: the consensus into its slot, cons_len, flags and window; then the scan of the lengths.  n_cands > 0
int pg_ddt_consensus_launch(const struct PgDdArgs *a, uint32_t n_cands, void *stream);
// the pool packed from the slots, cons_off and the containment items.  n_cands > 0
int pg_ddt_pool_launch(const struct PgDdArgs *a, uint32_t n_cands, void *stream);
// PG_DD_CONTAINED from the containment kernel's output
int pg_ddt_verdict_launch(const struct PgDdArgs *a, uint32_t n_cands, void *stream);
#ifdef __cplusplus
}
#endif

#endif
