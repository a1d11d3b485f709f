/*
 * pindel_pg.h -- C ABI of the MI355X-native split-read pattern-growth engine.
 *
 * Drop-in boundary for Pindel 0.2.5b9's hot path.  The reference has no FFI
 * layer; these entry points replace its two internal batch seams and the
 * per-read primitives behind them:
 *
 *   pg_close_end_batch  <->  ReadBuffer::flush()           src/read_buffer.cpp:36-101
 *                            (GetCloseEnd per read,        src/pindel.cpp:2531-2605,
 *                             updateReadAfterCloseEndMapping src/reader.cpp:1531-1554)
 *                            and the two loops in ReadInRead src/reader.cpp:248-255,300-305
 *   pg_far_end_batch    <->  SearchFarEnds(chrSeq, reads, chr) src/pindel.cpp:1115-1138
 *                            (SearchFarEnd per read,        src/pindel.cpp:1001-1074,
 *                             SearchFarEndAtPos             src/farend_searcher.cpp:46-103)
 *   pg_search_batch     <->  both of the above back to back (no BreakDancer hints: the hints of a read depend on
 *                            its close end, which the caller does not have yet -- pg_search_batch_table takes them
 *                            as a position-keyed pg_hint_table and looks them up on the device between the two)
 *   pg_load_reference   <->  Genome::loadAll / Chromosome::getSeq()  src/pindel.cpp:236-312
 *   pg_params           <->  the globals the path reads: g_maxMismatch (pindel.cpp:794-819),
 *                            g_MinClose (:88), userSettings->{MaxRangeIndex, ADDITIONAL_MISMATCH,
 *                            Min_Perfect_Match_Around_BP, MaximumAllowedMismatchRate,
 *                            Seq_Error_Rate, sensitivity}, g_SpacerBeforeAfter (pindel.h:122)
 *
 * Conventions: plain pointers and sizes only; the caller owns every input
 * buffer; result objects are owned by the library until pg_result_free.
 * Every function returns 0 (PG_OK) or a negative pg_status; nothing calls
 * exit().  One pg_ctx drives one GPU (HIP device ordinal in pg_params); use
 * one process per GPU.  Calls on one ctx are synchronous and not re-entrant.
 *
 * Coordinates are the reference's AbsLoc: indices into the spacer-padded
 * chromosome string (biological position + spacer).
 */
#ifndef PINDEL_PG_H
#define PINDEL_PG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PG_ABI_VERSION 1
#define PG_MAX_READ_LEN 499      /* g_maxMismatch has 500 entries (pindel.cpp:801) */

typedef enum {
    PG_OK = 0,
    PG_E_INVALID = -1,       /* bad argument                                   */
    PG_E_NOMEM = -2,         /* host or device allocation failed               */
    PG_E_DEVICE = -3,        /* HIP runtime error (see pg_last_error)          */
    PG_E_NO_REFERENCE = -4,  /* pg_load_reference not called                   */
    PG_E_READ_TOO_LONG = -5, /* a read is longer than PG_MAX_READ_LEN          */
    PG_E_UNSUPPORTED = -6    /* parameter outside what the device path handles */
} pg_status;

typedef struct pg_ctx pg_ctx;
typedef struct pg_result pg_result;
typedef struct pg_device_batch pg_device_batch;

/* Pindel command-line flags the path reads (defaults of 0.2.5b9 in brackets). */
typedef struct {
    int32_t  abi_version;                 /* PG_ABI_VERSION                              */
    int32_t  device;                      /* HIP device ordinal                          */
    int32_t  max_range_index;             /* -x [2], capped at 9 (pindel.cpp:125,921)    */
    int32_t  additional_mismatch;         /* -a [1], raised to >=1 (pindel.cpp:927)      */
    int32_t  min_perfect_match_around_bp; /* -m [3]                                      */
    int32_t  min_close;                   /* -H [8]  g_MinClose                          */
    double   max_allowed_mismatch_rate;   /* -u [0.02]                                   */
    double   seq_error_rate;              /* -e [0.01]                                   */
    double   sensitivity;                 /* -E [0.95]                                   */
    uint32_t spacer;                      /* g_SpacerBeforeAfter [100000]                */
    uint32_t reserved;
} pg_params;

/* One batch of one-end-anchored reads: the SPLIT_READ fields the path reads
 * (src/pindel.h:265-383), structure-of-arrays. */
typedef struct {
    uint32_t        n_reads;
    const uint8_t  *seq;            /* concatenated UnmatchedSeq, ASCII, as after setUnmatchedSeq */
    const uint64_t *seq_off;        /* n_reads+1 offsets into seq                                  */
    const uint8_t  *anchor_strand;  /* MatchedD: '+' or '-'                                        */
    const int32_t  *anchor_pos;     /* MatchedRelPos (biological coordinate)                       */
    const int16_t  *insert_size;    /* InsertSize (short, pindel.h:318)                            */
    const int32_t  *chr_id;         /* index of FragName in the loaded reference                   */
} pg_read_batch;

/* A SearchWindow (src/pindel.h:665-716) in AbsLoc coordinates. */
typedef struct {
    int32_t chr_id;
    int32_t start;   /* may be < 0: then start = end-1 (farend_searcher.cpp:69-71) */
    int32_t end;
} pg_window;

/* Per-read BreakDancer clusters (result of BDData::getCorrespondingSearchWindowCluster,
 * src/bddata.cpp:949-971), CSR.  NULL / n = 0 means "no hints". */
typedef struct {
    const uint64_t  *offset;   /* n_reads+1 */
    const pg_window *windows;
} pg_windows;

/* BreakDancer hints keyed by POSITION: the per-window object behind g_bdData.getCorrespondingSearchWindowCluster
 * (src/bddata.cpp:852-967) -- a mask over positions, run-length encoded, and the clusters it indexes.  The library looks
 * each read up on the device, from the close end it has just found or been given:
 *   - a read without a close end (close_max <= 0) gets no windows;
 *   - with p = UP_Close.back().AbsLoc outside [run_first[0], run_first[n_runs]) it gets none either;
 *   - otherwise it gets the windows of cluster run_cluster[k], in order, for the run k that holds p.
 * Any cluster may be empty.  NULL / n_runs = 0 means "no hints".  Every entry that takes a table gives bit for bit the
 * result of its pg_windows sibling fed the per-read clusters this rule expands to; the same limits apply. */
typedef struct {
    uint32_t         n_runs;
    const uint32_t  *run_first;    /* n_runs+1, strictly ascending AbsLoc; run k = [run_first[k], run_first[k+1]) */
    const uint32_t  *run_cluster;  /* n_runs, each < n_clusters */
    uint32_t         n_clusters;
    const uint64_t  *cluster_off;  /* n_clusters+1, monotone */
    const pg_window *windows;      /* as in pg_windows: start < 0 means end-1 */
} pg_hint_table;

/* Run-length-encoded UniquePoints (src/pindel.h:137-158).  A run stands for
 * the points  LengthStr = len_first..len_last  with
 * AbsLoc = abs_loc_first + (LengthStr-len_first)  for direction '+' (FORWARD)
 * AbsLoc = abs_loc_first - (LengthStr-len_first)  for direction '-' (BACKWARD),
 * all with the same Mismatches / Direction / Strand / chromosome. */
typedef struct {
    uint32_t abs_loc_first;
    uint16_t len_first;
    uint16_t len_last;
    uint8_t  mismatches;
    uint8_t  flags;          /* bit0: Direction BACKWARD, bit1: Strand ANTISENSE */
    int16_t  chr_id;
} pg_run;

#define PG_RUN_BACKWARD  0x1u
#define PG_RUN_ANTISENSE 0x2u

/* An expanded UniquePoint. */
typedef struct {
    uint32_t abs_loc;
    int16_t  length;       /* LengthStr  */
    int16_t  mismatches;
    int16_t  chr_id;
    char     direction;    /* '+' FORWARD / '-' BACKWARD */
    char     strand;       /* '+' SENSE   / '-' ANTISENSE */
} pg_point;

/* What a search leaves behind for each read (host memory, owned by the result). */
typedef struct {
    uint32_t        n_reads;
    const uint64_t *close_off;   /* n_reads+1: UP_Close runs of read i are close_runs[close_off[i]..close_off[i+1]) */
    const pg_run   *close_runs;  /* after CleanUniquePoints (pindel.cpp:2904-2941)                                  */
    const uint64_t *far_off;     /* n_reads+1 (all zero after pg_close_end_batch)                                   */
    const pg_run   *far_runs;    /* UP_Far                                                                          */
    const uint8_t  *rc_flag;     /* how GetCloseEnd left UnmatchedSeq (pindel.cpp:2545 "setUnmatchedSeq(ReverseComplement())"):
                                  * 0 as it came; 1 reverse-complemented once; 2 TWICE -- reported only for a read that holds a
                                  * character outside ACGTN, which two reverse complements do not restore: Convert2RC4N
                                  * (pindel.cpp:966-970) makes such characters NUL and setUnmatchedSeq (pindel.cpp:142-157) strips
                                  * the trailing ones, so the read is SHORTER by what it began with (after the first) and ended with
                                  * (after the second); every other read is its old self after two and keeps 0.  The search uses the
                                  * shortened read from that attempt on, exactly as the reference does; an adapter restores the
                                  * post-state by applying setUnmatchedSeq(ReverseComplement()) rc_flag times (pg_adapter.hpp).    */
} pg_result_view;

/* ---- lifetime ---------------------------------------------------------- */
void pg_default_params(pg_params *p);
int  pg_create(const pg_params *p, pg_ctx **out);
void pg_destroy(pg_ctx *ctx);
const char *pg_last_error(const pg_ctx *ctx);
/* g_maxMismatch as the library computed it (500 entries). */
int  pg_get_max_mismatch(const pg_ctx *ctx, uint32_t *table500);

/* ---- reference --------------------------------------------------------- */
/* seq_padded[c] is Chromosome::getSeq(): spacer N's + sequence + spacer N's, ASCII,
 * upper case ACGTN (anything else is taken as N).  Packs to 2-bit planes + N plane
 * and uploads to the ctx's GPU. */
int  pg_load_reference(pg_ctx *ctx, int32_t n_chr, const char *const *names,
                       const uint8_t *const *seq_padded, const uint64_t *len_padded);
/* FASTA loader with Genome::loadChromosome's semantics (pindel.cpp:272-312). */
int  pg_load_fasta(pg_ctx *ctx, const char *path);
/* Packed reference cache: writes / reads the loaded reference as the bit planes it
 * occupies in HBM, so that a genome is packed from FASTA once (Genome::loadChromosome semantics,
 * src/pindel.cpp:272-312, via pg_load_fasta) instead of being parsed character by character on every
 * run.  The file records the spacer it was packed with; loading it into a ctx with another spacer fails. */
int  pg_reference_save_packed(const pg_ctx *ctx, const char *path);
int  pg_reference_load_packed(pg_ctx *ctx, const char *path);
int  pg_reference_n_chr(const pg_ctx *ctx);
const char *pg_reference_name(const pg_ctx *ctx, int32_t chr_id);
uint64_t pg_reference_comp_size(const pg_ctx *ctx, int32_t chr_id);   /* getCompSize() */
/* Unpack [start, start+n) of a chromosome back to ASCII (tests, reporters). */
int  pg_reference_fetch(const pg_ctx *ctx, int32_t chr_id, uint64_t start, uint64_t n, uint8_t *out);

/* ---- the path, host buffers in / host results out ---------------------- */
int  pg_close_end_batch(pg_ctx *ctx, const pg_read_batch *reads, pg_result **out);
/* Both seams on ONE read vector: `close` must be the result of pg_close_end_batch on the same reads (it carries UP_Close
 * and the rc flags) and is extended in place with UP_Far; its close lists and rc flags are left as they are.  The reads
 * are given in their ORIGINAL orientation, which admits exactly two forms per read, with i's flag f = rc_flag[i]:
 *   (a) the read as it was first handed to pg_close_end_batch: the library applies the f
 *       "setUnmatchedSeq(ReverseComplement())" steps itself, shortening included; or
 *   (b) the read as the close end left it (the post-state, f steps applied: what pg_adapter::CloseEndBatch puts into
 *       UnmatchedSeq), reverse-complemented back where f & 1 -- every byte outside ACGTN becoming NUL, nothing stripped --
 *       and unchanged where f is 0 or 2 (what pg_adapter::make_batch(reads, chr_of, rc_flag) uploads).
 * Either way the far end runs on the post-state: on the reverse complement of what is given where f & 1, on the read
 * as given otherwise.  f = 2 means "in hand as is": two reverse complements, the ORIGINAL orientation again -- for form
 * (b) a read whose only characters outside ACGTN were at its ends is then a clean, shorter read that still carries 2.
 * For a read without such characters (a) and (b) are the same bytes.
 * The reference's own call site has a different vector by then -- see pg_far_end_batch_from_close. */
int  pg_far_end_batch(pg_ctx *ctx, const pg_read_batch *reads, pg_result *close,
                      const pg_windows *bd_hints /* nullable */);
/* Seam 2 exactly where the reference calls it: SearchFarEnds(chrSeq, state.Reads_SR, chr), src/pindel.cpp:1115-1138,
 * called at :1888 on the FILTERED UNION of many flushes -- ReadBuffer::flush keeps only the reads that got a close end
 * (src/read_buffer.cpp:55-64), 50 000 raw reads at a time (src/reader.cpp:55).  So this entry takes the reads as the
 * close end left them (UnmatchedSeq already reverse-complemented where GetCloseEnd did so, src/pindel.cpp:2545) and,
 * per read, the two things SearchFarEnd reads from UP_Close:
 *   close_last[i] = UP_Close.back().AbsLoc      getLastAbsLocCloseEnd(), src/pindel.cpp:475-478 (centre of the ranges)
 *   close_max[i]  = UP_Close.back().LengthStr   UP_Close.MaxLen(), src/pindel.cpp:480-483, 490-498 (goodFarEndFound);
 *                                               <= 0: the read has no close end and is not searched
 * No result of an earlier call is needed; anchor_strand / anchor_pos / insert_size of the batch are not read by the far
 * end (they must still be valid arrays).  The result holds UP_Far (far_off / far_runs); its close lists are empty and
 * its rc flags zero. */
int  pg_far_end_batch_from_close(pg_ctx *ctx, const pg_read_batch *reads, const uint32_t *close_last,
                                 const int16_t *close_max, const pg_windows *bd_hints /* nullable */, pg_result **out);
/* Close end + far end of one batch, host buffers in, host results out.  It takes no BreakDancer hints: they follow from
 * each read's close end (see pg_search_batch_table). */
int  pg_search_batch(pg_ctx *ctx, const pg_read_batch *reads, pg_result **out);

/* The same three entries with the hints as a pg_hint_table: the lookup runs on the device (count, scan, fill: three small
 * kernels on the ctx's stream) from the close-end summary that is already there, and the host waits once more, for 16 bytes.
 * A malformed table -- unsorted run_first, a run_cluster value >= n_clusters, non-monotone cluster_off, a window on an
 * unknown chromosome, a null array with a non-zero count -- is PG_E_INVALID before anything is launched.
 *   pg_far_end_batch_from_close_table   seam 2 as the reference calls it, hints included
 *   pg_far_end_batch_table              both seams on one read vector (sibling of pg_far_end_batch)
 *   pg_search_batch_table               close end, lookup and far end in one call: the reads are uploaded once, and the
 *                                       close-end summary stays on the device until the far end has run */
int  pg_far_end_batch_from_close_table(pg_ctx *ctx, const pg_read_batch *reads, const uint32_t *close_last,
                                       const int16_t *close_max, const pg_hint_table *table /* nullable */, pg_result **out);
int  pg_far_end_batch_table(pg_ctx *ctx, const pg_read_batch *reads, pg_result *close, const pg_hint_table *table /* nullable */);
int  pg_search_batch_table(pg_ctx *ctx, const pg_read_batch *reads, const pg_hint_table *table /* nullable */, pg_result **out);

/* Multi-GPU form of pg_search_batch: the reads are split into n_ctx contiguous ranges (reads are independent:
 * the loop of ReadBuffer::flush / SearchFarEnds, src/read_buffer.cpp:36-101, src/pindel.cpp:1115-1138), context k
 * (one GPU each, the same reference loaded in all of them) searches range k on its own host thread, and the
 * results are concatenated in order: identical to pg_search_batch on one context.  No collective between GPUs. */
int  pg_search_batch_multi(pg_ctx *const *ctxs, int32_t n_ctx, const pg_read_batch *reads, pg_result **out);

int  pg_result_view_get(const pg_result *r, pg_result_view *view);
void pg_result_free(pg_result *r);
/* Expand runs to UniquePoints; returns the number of points (call with out = NULL to count). */
uint64_t pg_expand_runs(const pg_run *runs, uint64_t n_runs, pg_point *out);

/* ---- the path, device-resident (what bench.py times) ------------------- */
int  pg_device_batch_upload(pg_ctx *ctx, const pg_read_batch *reads, pg_device_batch **out);
/* Attaches per-read BreakDancer/RP window clusters (the SearchWindowCluster of
 * g_bdData.getCorrespondingSearchWindowCluster(read), src/bddata.cpp:949-979, searched before the
 * ranges, src/pindel.cpp:1006-1018) to a device-resident batch; NULL detaches them.  Same limits as
 * pg_far_end_batch. */
int  pg_device_batch_set_windows(pg_ctx *ctx, pg_device_batch *b, const pg_windows *bd_hints);
/* Close end + far end for every read of the batch; results stay on the GPU.
 * Synchronous: returns when the kernels have finished. */
int  pg_device_batch_search(pg_ctx *ctx, pg_device_batch *b);
int  pg_device_batch_download(pg_ctx *ctx, pg_device_batch *b, pg_result **out);
/* Measurement: runs the pack stage of pg_device_batch_upload again on the resident batch -- ASCII bases (what
 * src/reader.cpp:852-856 hands over) -> the bit planes and packed records the search kernel reads; idempotent -- and
 * returns its HIP-event duration in ms (events on the ctx's own stream). */
int  pg_device_batch_repack(pg_ctx *ctx, pg_device_batch *b, double *pack_ms);
/* Pack + search of the resident batch as ONE step: the result of pg_device_batch_repack followed by pg_device_batch_search.
 * Wherever the batch's plane layout is that of its search kernels (32-bit candidate ids: always) the search kernel builds the planes
 * and records of its reads itself, claim by claim (the pack is HBM-bound, the search is not: no launch of its own).  Synchronous. */
int  pg_device_batch_pack_search(pg_ctx *ctx, pg_device_batch *b);
/* Close end, hint lookup and far end of every read of a resident batch, the results left on the GPU: what pg_search_batch_table
 * computes, with both run lists resident.  Synchronous.  Afterwards the batch is searched, in the state pg_device_batch_search
 * would leave had each read's cluster (by the lookup rule of pg_hint_table) been attached with pg_device_batch_set_windows --
 * close runs, far runs, rc_flag, close_last, close_max -- so pg_device_batch_download, _download_device, _result_sizes, the five
 * classifier stages and pg_device_batch_classify give bit for bit what they give there.
 *   - Three steps on the ctx's stream: a close launch (which packs the reads), the lookup of pg_search_batch_table from the
 *     summary that launch left, and a far launch that appends its runs to the pool behind the close runs.  If the pool
 *     overflows in either launch it is regrown and all three are done again.
 *   - A null table or one with n_runs == 0: attached windows are cleared and the call is pg_device_batch_pack_search.
 *   - A malformed table is PG_E_INVALID before anything is launched (the texts of the _table entries above) and leaves the
 *     batch as it was: still searched if it was, its results intact.  A missing reference and a batch uploaded before a
 *     reference reload are refused before any launch as well.
 *   - The windows the lookup attached stay attached: pg_device_batch_search on the same batch gives the same result again,
 *     pg_device_batch_set_windows(ctx, b, NULL) detaches them.  Calling this entry again, with any table or none, gives that
 *     table's result alone.
 *   - pg_last_search_stats: the two search launches' HIP-event times added up, the pool slots after the far launch;
 *     pg_debug_last_hint_stats: the lookup. */
int  pg_device_batch_search_table(pg_ctx *ctx, pg_device_batch *b, const pg_hint_table *table /* nullable */);
/* The close half of pg_device_batch_search_table on its own: attached windows are cleared, one close launch (which packs the reads)
 * runs with the pool cursors zeroed, and the per-read summary (rc_flag, close_last, close_max) is left in the batch's arrays; a pool
 * that overflowed is regrown and the launch repeated.  Synchronous.  Afterwards the batch is CLOSE-searched, not searched: its
 * output records hold the close end and its pool the close runs, which is what pg_device_batch_dd needs; the classifier stages and
 * pg_device_batch_li / _int / _classify, which need a full search, keep refusing it as a batch that has not been searched.
 * The far fields of the records are cleared: pg_device_batch_download then delivers the close runs and empty far lists, also on a
 * batch that had a full search before.  A full search makes a batch close-searched too.
 * Refusals as for every search (no reference, a batch uploaded before a reference reload).  pg_last_search_stats: the launch's
 * HIP-event time and the pool slots taken. */
int  pg_device_batch_close_search(pg_ctx *ctx, pg_device_batch *b);
void pg_device_batch_free(pg_ctx *ctx, pg_device_batch *b);
/* HIP-event duration (ms) of the kernel of the last search on this ctx (events recorded on
 * the ctx's own stream around the launch) and the run-pool slots it took (reserved per read + allocated; the number
 * of runs is close_off[n] + far_off[n] of the downloaded result). */
int  pg_last_search_stats(const pg_ctx *ctx, double *kernel_ms, uint64_t *n_runs);
/* Algorithmic bytes of the last search of this batch (SURVEY.md 8d formula, accumulated per
 * read by the kernel; DESIGN.md "roofline accounting").  Copies n x 4 bytes back: call it
 * outside any timed region. */
int  pg_device_batch_algorithmic_bytes(pg_ctx *ctx, pg_device_batch *b, double *bytes);
/* Diagnostics: candidate positions (survivors of the kernel's seed filter) that went through the full
 * comparison in the last search of this batch -- what a repeat-rich reference drives up. */
int  pg_device_batch_candidates(pg_ctx *ctx, pg_device_batch *b, double *n_candidates);

/* ---- device buffers in and out: reference, reads and results in the memory of the ctx's GPU -----------------------------
 * For a caller whose data is already in HBM (a GPU decoder, a torch pipeline): the three host round trips of the
 * device-resident path have a sibling that takes or fills device memory.  Common rules:
 *   - Synchronous, like the rest of the ABI: the caller makes sure its inputs are complete (its own streams have finished
 *     writing them) before the call; when a call returns, everything the library wrote is complete.  There is no stream argument.
 *   - Inputs are copied, device to device, into buffers of the library's own: the caller owns its buffers and may release them
 *     when the call returns.  Results are written into buffers the caller allocated.
 *   - Every non-null pointer is checked before anything is launched: it must be device memory of the ctx's own GPU, aligned for
 *     its element type, and the bytes the library will touch must lie inside its allocation -- otherwise PG_E_INVALID, with
 *     pg_last_error naming the array.  A host pointer ends in a status code, never in a fault.  (seq and the run buffers are
 *     checked once their size is known: after the measurement / the first pass.)  A pointer may point INTO an allocation.
 *   - Nothing is launched for an empty batch. */
/* pg_load_reference with the bases in device memory.  names, len_padded and the array d_seq_padded itself are host memory;
 * d_seq_padded[c] points to len_padded[c] ASCII bytes on the device, spacers included, with any alignment.  The planes are
 * built on the device and are bit for bit those of pg_load_reference: A C G T in upper case, every other byte value is N.
 * The same argument checks and status codes; the reference counts as reloaded (device batches uploaded before are refused).
 * pg_reference_fetch and pg_reference_save_packed work as after a host load: the first of them copies the planes to the host. */
int  pg_load_reference_device(pg_ctx *ctx, int32_t n_chr, const char *const *names,
                              const uint8_t *const *d_seq_padded, const uint64_t *len_padded);
/* pg_device_batch_upload with the batch in device memory: d_reads is a host struct whose six array members are device
 * pointers.  The reads are validated and measured on the device in one pass; the status codes and pg_last_error texts are
 * those of pg_device_batch_upload for the same batch (of several bad reads the one with the lowest index is reported), and the
 * result is an ordinary pg_device_batch: set_windows, search, pack_search, repack, download and the diagnostics take it. */
int  pg_device_batch_upload_device(pg_ctx *ctx, const pg_read_batch *d_reads, pg_device_batch **out);
/* Where pg_device_batch_download_device puts a searched batch: device buffers of the caller, laid out as pg_result_view. */
typedef struct {
    uint64_t *close_off;  pg_run *close_runs;  uint64_t close_cap;   /* n+1 offsets; capacity in runs */
    uint64_t *far_off;    pg_run *far_runs;    uint64_t far_cap;
    uint8_t  *rc_flag;    uint32_t *close_last; int16_t *close_max;  /* n each; any of the three may be NULL */
} pg_device_result;
/* The number of runs a download of the batch holds: close_off[n] and far_off[n]. */
int  pg_device_batch_result_sizes(pg_ctx *ctx, pg_device_batch *b, uint64_t *n_close_runs, uint64_t *n_far_runs);
/* pg_device_batch_download into the caller's device buffers: runs and offsets are gathered straight into them (off[n]
 * included; a list without runs gets zeroed offsets and its run pointer may be NULL), only a few bytes per 2^20 reads come
 * to the host.  A capacity below the list's total is PG_E_INVALID and nothing is written.  close_last / close_max are
 * UP_Close.back()'s AbsLoc / LengthStr as pg_far_end_batch_from_close takes them.  The batch stays searchable and
 * downloadable, by either download. */
int  pg_device_batch_download_device(pg_ctx *ctx, pg_device_batch *b, const pg_device_result *dst);

/* ---- device classifier: deletion and short-insertion candidates per read ---------------------------------
 * The per-read stage of SearchVariant::Search (src/search_variant.cpp:104-240) for its two kinds -- 0 = deletions
 * (searchdeletions.cpp), 1 = short insertions (searchshortinsertions.cpp) -- on a searched device batch: for every read and
 * kind the first PG_VARIANT_CANDS distinct (close point, far point) pairs that pass the mismatch, direction and geometry
 * tests, in the order the reference's loops first visit them (mismatch budget, then close points ascending for a '+' anchor
 * and descending for a '-' anchor, then far points from the highest index down), each with the fields the loop has computed
 * when it reaches readTransgressesBinBoundaries.  The window-dependent tests (bin boundary, region, box) stay with the caller. */
#define PG_VARIANT_CANDS 4
#define PG_VARIANT_MORE 0x80u        /* count byte: qualifying pairs exist beyond the ones listed */
#define PG_VARIANT_REF_END 0x1u      /* pg_variant_cand::flags: BPLeft or BPRight lies beyond the chromosome string (the loop marks
                                      * the read Used and stops); the other fields are as they stood before the alignment */
typedef struct {
    uint32_t bp_left, bp_right;      /* BPLeft, BPRight after the left alignment's shift            */
    int32_t  left, right;            /* Left, Right                                                 */
    uint32_t indel_size;             /* IndelSize                                                   */
    int32_t  nt_rot;                 /* kind 1: NT_str is the read's substring rotated LEFT by nt_rot places (negative: right), the
                                      * net effect of GetRealStart4Insertion; reduce it modulo the string's length.  0 for kind 0 */
    int16_t  bp;                     /* BP after the shift                                          */
    uint16_t close_idx, far_idx;     /* the pair: indices of the expanded points in UP_Close / UP_Far */
    uint8_t  flags;                  /* PG_VARIANT_*                                                */
    uint8_t  reserved;               /* 0                                                           */
} pg_variant_cand;
/* cands: n_reads x 2 kinds x PG_VARIANT_CANDS records (unused ones zeroed); counts: n_reads x 2 bytes, the number listed in the
 * low bits and PG_VARIANT_MORE.  A read without a far end, with its far end on another chromosome than its anchor, or with an
 * anchor strand other than '+' / '-' gets count 0.  ReadLength, MAX_SNP_ERROR and the bases are those GetCloseEnd left (rc_flag).
 * The batch must have been searched (PG_E_INVALID otherwise).  Synchronous; pg_last_search_stats then reports the kernel's
 * HIP-event time.  The _device entry writes into device buffers of the caller under the rules of "device buffers in and out". */
int  pg_device_batch_variant_candidates(pg_ctx *ctx, pg_device_batch *b, pg_variant_cand *cands, uint8_t *counts);
int  pg_device_batch_variant_candidates_device(pg_ctx *ctx, pg_device_batch *b, pg_variant_cand *d_cands, uint8_t *d_counts);

/* ---- device classifier: DI, tandem-duplication and inversion candidates per read ---------------------------
 * The per-read stage of the five other classifiers process_window runs, on a searched device batch.  The kinds continue
 * the numbering of 0 and 1; the record is pg_variant_cand with the fields the classifier has assigned when it reaches the
 * window-dependent tail (bin boundary, region, box), which stays with the caller:
 *   PG_SV_DI     searchIndels (src/search_deletions_nt.cpp): one pair, UP_Close.back() and UP_Far.back()
 *   PG_SV_TD     searchTandemDuplications: the first PG_VARIANT_CANDS pairs in first-visit order (budget, close points ascending
 *                for a '+' anchor and descending for '-', far points from the highest index down for '+' and from the lowest up
 *                for '-') after LeftMostTD; a pair with BPLeft == 0 is not listed
 *   PG_SV_TD_NT  searchTandemDuplicationsNT: one pair
 *   PG_SV_INV    searchInversions: the first PG_VARIANT_CANDS pairs (geometries 0 and 2: close points descending, far points
 *                ascending; 1 and 3: the reverse) after LeftMostINV
 *   PG_SV_INV_NT searchInversionsNT: one pair
 * nt_rot carries NT_size for the three kinds with non-template bases (0 for TD and INV); NT_str is cut from the read by the
 * host.  flags: PG_VARIANT_REF_END = LeftMostTD / LeftMostINV took their out-of-range branch (the record then carries BPLeft =
 * BPRight = BP = 1, the read is Used and the box test still runs); bits 4-5 = the inversion geometry of PG_SV_INV and
 * PG_SV_INV_NT (0: '+' anchor, far end right; 1: '+', far end left; 2: '-', far end left; 3: '-', far end right). */
enum { PG_SV_DI = 2, PG_SV_TD = 3, PG_SV_TD_NT = 4, PG_SV_INV = 5, PG_SV_INV_NT = 6 };
#define PG_SV_KINDS 5                /* count bytes per read: DI, TD, TD_NT, INV, INV_NT */
#define PG_SV_SLOTS 11               /* records per read: DI, TD x 4, TD_NT, INV x 4, INV_NT */
#define PG_SV_GEO_SHIFT 4            /* pg_variant_cand::flags bits 4-5: the inversion geometry */
#define PG_SV_MAX_INVERSION_SIZE (1 << 30)
typedef struct {
    double  seq_error_rate;          /* -e */
    int32_t min_num_matched_bases;   /* -d */
    int32_t min_inversion_size;      /* -v: used as unsigned; negative or above PG_SV_MAX_INVERSION_SIZE is PG_E_INVALID */
} pg_sv_params;
/* cands: n_reads x PG_SV_SLOTS records (unused ones zeroed); counts: n_reads x PG_SV_KINDS bytes as for the kinds 0 and 1.
 * Same rules as pg_device_batch_variant_candidates: a searched batch, synchronous, the HIP-event time in pg_last_search_stats. */
int  pg_device_batch_sv_candidates(pg_ctx *ctx, pg_device_batch *b, const pg_sv_params *p, pg_variant_cand *cands, uint8_t *counts);
int  pg_device_batch_sv_candidates_device(pg_ctx *ctx, pg_device_batch *b, const pg_sv_params *p, pg_variant_cand *d_cands,
                                          uint8_t *d_counts);

/* ---- device classifier: window tail, boxes and event tables -------------------------------------------------
 * From the candidate lists of a searched batch and one window description to event tables on the GPU: the window-dependent
 * tail of all seven classifiers in process_window's order (kind 0, DI, TD and TD_NT if analyze_td, INV and INV_NT if analyze_inv,
 * kind 1 last) with the Used cascade between them, then -- for the four kinds whose reporters sort with bubblesortReads and
 * markDuplicates: kind 0, kind 1, PG_SV_TD, PG_SV_TD_NT, "tables" 0..3 in this order -- the boxed reads in the order the sort leaves
 * them, the duplicates marked, and the unique reads grouped into events.  A pure function of the lists, the reads of the batch, the
 * window and the loaded reference; the lists are trusted (close_idx / far_idx are not checked against the points).  BoxSize and
 * NumBoxes follow from the padded chromosome length as Caller::process_window computes them. */
typedef struct {
    int32_t  chr_id;                 /* reads with another chr_id are untouched                                    */
    uint32_t win_end;                /* upper bound of readTransgressesBinBoundaries                              */
    uint32_t region_start, region_end;   /* the region test is on BPLeft + 1, both ends included                  */
    uint32_t min_support;            /* -M NumRead2ReportCutOff                                                    */
    uint32_t balance_cutoff;         /* -B BalanceCutoff                                                           */
    int32_t  analyze_td, analyze_inv;
} pg_event_window;
#define PG_EVENT_TABLES 4            /* kind 0, kind 1, PG_SV_TD, PG_SV_TD_NT */
#define PG_EVR_BOXED      0x1u       /* pg_event_read::flags: the pair (kind, slot) put the read into a box         */
#define PG_EVR_USED       0x2u       /* ... made it Used without a box (PG_VARIANT_REF_END, or it transgresses the window's end) */
#define PG_EVR_UNRESOLVED 0x4u       /* the list of unresolved_kind ended with PG_VARIANT_MORE before a pair made the read Used: the
                                      * read left the cascade there (on the host it goes to the pair search) and is in no event */
#define PG_EVR_DUPLICATE  0x8u       /* markDuplicates: an earlier read of its box has the same (Left, Right, name)  */
typedef struct {
    uint8_t  kind;                   /* the kind whose pair made the read Used (valid with BOXED or USED)           */
    uint8_t  slot;                   /* ... and the pair's place in that kind's list                                */
    uint8_t  flags;                  /* PG_EVR_*; an untouched read is all zero                                     */
    uint8_t  unresolved_kind;        /* valid with PG_EVR_UNRESOLVED                                                */
    uint16_t nt_size;                /* NT_size as the cascade left it when the read was boxed (0 otherwise)        */
    uint16_t reserved;
} pg_event_read;
#define PG_EV_SUPPORT 0x1u           /* pg_event::flags: n_reads >= -M                                              */
#define PG_EV_RANGE   0x2u           /* kind 1: real_start < real_end; TD kinds: !(real_end < real_start || real_start == 0); kind 0: set */
#define PG_EV_BALANCE 0x4u           /* the first member's IndelSize < -B, or ReportEvent over the members; kind 1: set */
#define PG_EV_REPORT  0x8u           /* all three                                                                   */
typedef struct {
    uint32_t bp_left, bp_right, indel_size;   /* of the first member                                                */
    uint32_t first, n_reads;         /* members [first, first + n_reads) of the kind's member list                  */
    uint32_t n_plus;                 /* members with a '+' anchor                                                   */
    uint32_t real_start, real_end;   /* GetRealStart4Deletion (GetRealStart4Insertion with the first member's NT_str for kind 1) */
    uint32_t box_head;               /* member index of the first unique read of the event's box (GoodIndels[0])    */
    uint16_t nt_size;                /* carried NT_size of the first member                                         */
    uint8_t  kind;
    uint8_t  flags;                  /* PG_EV_*                                                                     */
} pg_event;
typedef struct {
    uint64_t members[PG_EVENT_TABLES];   /* unique boxed reads per table                                            */
    uint64_t events[PG_EVENT_TABLES];
    uint64_t unresolved;                 /* reads flagged PG_EVR_UNRESOLVED                                         */
} pg_event_sizes;
/* Builds the tables of the batch for one window and keeps them with the batch (a later build replaces them).  cands / counts and
 * sv_cands / sv_counts: the lists as the two candidate entries yield them, host memory; either pair may be NULL (those kinds' lists
 * then count as empty).  name_id: NULL (all names differ) or one uint32 per read, equal names having equal ids.  Refused with nothing
 * launched: a batch that was not searched, a chr_id outside the reference, region_start > region_end.  n_reads == 0 and "nothing
 * boxed" are valid.  Synchronous; pg_last_search_stats then reports the HIP-event time of the kernels.  The _device siblings take /
 * fill device memory under the rules of "device buffers in and out".
 * pg_device_batch_events_download: reads = n_reads records; members = the four member lists back to back (read indices, in table
 * order); events = the four event lists back to back; sized by pg_device_batch_event_sizes.  Any of the three may be NULL. */
int  pg_device_batch_events(pg_ctx *ctx, pg_device_batch *b, const pg_event_window *window, const pg_variant_cand *cands,
                            const uint8_t *counts, const pg_variant_cand *sv_cands, const uint8_t *sv_counts, const uint32_t *name_id);
int  pg_device_batch_events_device(pg_ctx *ctx, pg_device_batch *b, const pg_event_window *window, const pg_variant_cand *d_cands,
                                   const uint8_t *d_counts, const pg_variant_cand *d_sv_cands, const uint8_t *d_sv_counts,
                                   const uint32_t *d_name_id);
int  pg_device_batch_event_sizes(pg_ctx *ctx, pg_device_batch *b, pg_event_sizes *sizes);
int  pg_device_batch_events_download(pg_ctx *ctx, pg_device_batch *b, pg_event_read *reads, uint32_t *members, pg_event *events);
int  pg_device_batch_events_download_device(pg_ctx *ctx, pg_device_batch *b, pg_event_read *d_reads, uint32_t *d_members,
                                            pg_event *d_events);

/* ---- device classifier: DI and inversion event tables --------------------------------------------------------
 * The three kinds pg_device_batch_events leaves at their per-read records -- PG_SV_DI, PG_SV_INV, PG_SV_INV_NT, "SV tables" 0..2 in
 * this order -- as event tables.  Their reporters sort a box with a STRICT exchange sort (x > y swaps, equality does not), whose tie
 * order depends on the order the box arrives in: ascending read index.  A pure function of the per-read records the events build
 * left with the batch (kind, slot, flags, nt_size), the sv lists, the batch (anchor strand, post-state read length and bases, the
 * last close point: LeftMostPos = AbsLoc + 1 - close_len for a '+' anchor, AbsLoc + close_len - ReadLength for '-'), that build's
 * window (-M, -B), BoxSize and the loaded reference.  No name_id: these reporters do not call markDuplicates.
 *   sort keys    DI: BPLeft, BPRight, carried NT_size, BP (signed).  INV / INV_NT: BPLeft + BPRight (uint32, wrapping), IndelSize
 *                DESCENDING, BPLeft, BPRight, for INV_NT the carried NT_size, BP.
 *   duplicates   a read of the sorted box is one if ANY earlier read of the box, unique or not, has an equal LeftMostPos or an equal
 *                LeftMostPos + ReadLength, and the same anchor strand -- for DI an equal ReadLength as well.
 *   DI           members = the unique reads in sorted order; an event = a maximal run with equal (BPLeft, IndelSize, (short)NT_size).
 *                PG_EV_BALANCE as for the tables of 7m, PG_EV_SHORT_INV = the first member's IndelSize == NT_size and the reverse
 *                complement of those reference bases at spacer + 1 + BPLeft is its NT_str (the reporter then writes a short
 *                inversion); PG_EV_REPORT = SUPPORT and BALANCE.  real_start / real_end = bp_left / bp_right.
 *   INV, INV_NT  members = ALL reads of the box in sorted order, a duplicate with PG_SVEV_MEMBER_DUP in its member word.  A run = a
 *                maximal stretch with an equal BPLeft + BPRight; mx = its largest IndelSize; a member passes if NOT
 *                (IndelSize / (float)mx < 0.95 || mx + 30 > (unsigned)(ReadLength + IndelSize)) and is then harmonised: diff =
 *                (short)((mx - IndelSize) / 2), IndelSize = mx, BPLeft -= diff, BPRight += diff, BP moves by diff under the two
 *                guards of the reporter.  A run with a failing member yields no event, and neither does any later run of its box
 *                (dropped_runs counts them).  The event: bp_left / bp_right = the harmonised first member's, indel_size = mx,
 *                real_start / real_end = the same -- but for the LAST run of a box the first member's values before harmonisation;
 *                PG_EV_RANGE = !(real_end < real_start || real_start == 0); PG_EV_BALANCE over the harmonised members; PG_EV_REPORT
 *                = all three.  A consumer recomputes a member's harmonised fields from indel_size.
 * All events are listed, boxes below -M included (their events cannot reach PG_EV_SUPPORT). */
#define PG_SV_EVENT_TABLES 3         /* PG_SV_DI, PG_SV_INV, PG_SV_INV_NT */
#define PG_EV_SHORT_INV 0x10u        /* pg_event::flags of SV table 0: is_inversion of the first member                    */
#define PG_SVEV_MEMBER_DUP 0x80000000u   /* member word of SV tables 1 and 2: the read is a duplicate                      */
typedef struct {
    uint64_t members[PG_SV_EVENT_TABLES];
    uint64_t events[PG_SV_EVENT_TABLES];
    uint64_t dropped_runs[PG_SV_EVENT_TABLES];   /* runs without an event: a failed harmonisation in or before them        */
} pg_sv_event_sizes;
/* Builds the SV tables of the batch and keeps them with it (an events build or a new sv build replaces them; freed with the batch).
 * sv_cands / sv_counts: the lists the events build was given (host memory; the _device sibling: device memory).  Refused with
 * nothing launched: no events build on this batch (PG_E_INVALID), null lists for a non-empty batch, 2^31 reads or more.  The
 * window is that build's.  n_reads == 0 and "nothing boxed" are valid.  Synchronous; pg_last_search_stats then reports the
 * HIP-event time.  download: members = the three member lists back to back, events likewise; either may be NULL. */
int  pg_device_batch_sv_events(pg_ctx *ctx, pg_device_batch *b, const pg_variant_cand *sv_cands, const uint8_t *sv_counts);
int  pg_device_batch_sv_events_device(pg_ctx *ctx, pg_device_batch *b, const pg_variant_cand *d_sv_cands, const uint8_t *d_sv_counts);
int  pg_device_batch_sv_event_sizes(pg_ctx *ctx, pg_device_batch *b, pg_sv_event_sizes *sizes);
int  pg_device_batch_sv_events_download(pg_ctx *ctx, pg_device_batch *b, uint32_t *members, pg_event *events);
int  pg_device_batch_sv_events_download_device(pg_ctx *ctx, pg_device_batch *b, uint32_t *d_members, pg_event *d_events);

/* ---- device classifier: report records --------------------------------------------------------------------------
 * What a report writer takes from the candidate lists and the points, per table member and per read, so that a caller who writes
 * reports from the tables downloads neither.  A pure function of the two table builds the batch holds, the lists they were given
 * and the batch's run lists.
 *   pg_report_read     one per member of the seven member lists, in order: tables 0..3 of the events build, then SV tables 0..2 of
 *                      the sv build; record i belongs to member i.
 *   pg_report_summary  one per read of the batch: what the pipeline and process_window read of the points for every read. */
#define PG_RR_DUP 0x1u               /* pg_report_read::flags: the member word carries PG_SVEV_MEMBER_DUP (SV tables 1 and 2)   */
#define PG_RR_DI  0x2u               /* ... table 2 (TD): the read's DI list holds a pair; di_bp / di_nt_rot are that pair's    */
typedef struct {
    uint32_t read;                   /* the member: a read index of the batch                                                  */
    pg_variant_cand cand;            /* the pair (kind, slot) the read's pg_event_read names, copied from the lists            */
    uint16_t nt_size;                /* the carried NT_size (pg_event_read::nt_size)                                           */
    uint8_t  table;                  /* 0..3: the events build's tables; 4..6: SV tables 0..2                                  */
    uint8_t  flags;                  /* PG_RR_*                                                                                */
    int16_t  bp0;                    /* table 1: (short)(LengthStr - 1) of close point cand.close_idx for a '+' anchor, of far
                                      * point cand.far_idx otherwise: NT_str is cut from the read behind it.  0 for other tables */
    int16_t  di_bp;                  /* with PG_RR_DI: bp and nt_rot of the DI pair (TD's NT_str is DI's); 0 otherwise         */
    int32_t  di_nt_rot;
} pg_report_read;                    /* 48 bytes, no padding                                                                   */
#define PG_RS_CLOSE          0x1u    /* pg_report_summary::flags: the read has a close end                                     */
#define PG_RS_FAR            0x2u    /* ... a far end                                                                          */
#define PG_RS_FAR_ANTISENSE  0x4u    /* ... whose first point (UP_Far[0]) has Strand ANTISENSE                                 */
#define PG_RS_CLOSE_LEFT     0x8u    /* both ends: UP_Close[0].AbsLoc < UP_Far[0].AbsLoc (the inversion writer orients the read by it) */
#define PG_RS_CLOSE_RIGHT    0x10u   /* both ends: UP_Close[0].AbsLoc > UP_Far[0].AbsLoc                                       */
typedef struct {
    uint32_t close_abs;              /* UP_Close.back().AbsLoc (0 without a close end)                                         */
    int16_t  close_len;              /* UP_Close.back().LengthStr (0 without)                                                  */
    int16_t  far_chr;                /* UP_Far[0]'s chromosome (0 without a far end)                                           */
    uint8_t  flags;                  /* PG_RS_*                                                                                */
    uint8_t  rc_flag;                /* pg_result_view::rc_flag                                                                */
    uint16_t reserved;               /* 0                                                                                      */
} pg_report_summary;                 /* 12 bytes                                                                               */
typedef struct {
    uint64_t records;                /* pg_report_read records: the members of all seven tables                                */
    uint64_t reads;                  /* pg_report_summary records: the reads of the batch                                      */
} pg_report_sizes;
/* Builds both and keeps them with the batch (a new events or sv events build drops them; freed with the batch).  cands / counts and
 * sv_cands / sv_counts: the lists the two table builds were given (host memory; the _device sibling: device memory under the rules
 * of "device buffers in and out").  Refused with nothing launched (PG_E_INVALID): a batch that holds no events build or no sv events
 * build, a null list array for a non-empty batch.  n_reads == 0 and "no members" are valid.  A member whose read, kind or slot lies
 * outside the batch or its lists gets a zeroed record.  Synchronous; pg_last_search_stats then reports the HIP-event time.
 * download: records = pg_report_sizes::records records, summaries = n_reads; either may be NULL. */
int  pg_device_batch_report_reads(pg_ctx *ctx, pg_device_batch *b, const pg_variant_cand *cands, const uint8_t *counts,
                                  const pg_variant_cand *sv_cands, const uint8_t *sv_counts);
int  pg_device_batch_report_reads_device(pg_ctx *ctx, pg_device_batch *b, const pg_variant_cand *d_cands, const uint8_t *d_counts,
                                         const pg_variant_cand *d_sv_cands, const uint8_t *d_sv_counts);
int  pg_device_batch_report_sizes(pg_ctx *ctx, pg_device_batch *b, pg_report_sizes *sizes);
int  pg_device_batch_report_download(pg_ctx *ctx, pg_device_batch *b, pg_report_read *records, pg_report_summary *summaries);
int  pg_device_batch_report_download_device(pg_ctx *ctx, pg_device_batch *b, pg_report_read *d_records, pg_report_summary *d_summaries);

/* One call per window on a searched batch: the two candidate kernels, the events build, the sv events build and the report records.
 * The candidate lists stay in device memory owned by the batch (a later classify of the batch overwrites them; freed with it): no
 * list crosses to the host.  The tables, records and summaries are then delivered by the size and download entries above.
 *   max_listed  0..PG_VARIANT_CANDS.  Below PG_VARIANT_CANDS every list with more than max_listed pairs is cut: its count byte
 *               becomes max_listed | PG_VARIANT_MORE (the records behind stay; nothing reads them).  A read whose cut list did not
 *               make it Used is then PG_EVR_UNRESOLVED: with 0, every read that reaches a list with a pair.
 * name_id: host memory, NULL or one uint32 per read as for pg_device_batch_events.  The refusals are those of the five stages,
 * checked before anything is launched.  pg_last_search_stats then reports the sum of the stages' HIP-event times, the cut's
 * included.  The launch log gets the stages' own records; the cut is logged as the report kernels' id with `blocks` 0. */
typedef struct {
    pg_event_window window;
    pg_sv_params    sv;
    int32_t         max_listed;      /* PG_VARIANT_CANDS: no cut                                                               */
    int32_t         reserved;        /* 0                                                                                      */
} pg_classify_params;
int  pg_device_batch_classify(pg_ctx *ctx, pg_device_batch *b, const pg_classify_params *p, const uint32_t *name_id);

/* ---- device classifier: long-insertion position tables -------------------------------------------------------
 * What SortOutputLI (src/reporter.cpp:1853-2141) counts per position -- the reads that kept a close end and found no far end, by
 * anchor strand and by the position of their last close point -- as tables, so that a caller who writes _LI downloads no point.
 * An LI read is a read of the batch whose chr_id is the events build's window chr_id, that has a close end and no far end, whose
 * pg_event_read::flags carries neither PG_EVR_BOXED nor PG_EVR_USED (PG_EVR_UNRESOLVED alone does not exclude it) and whose anchor
 * strand is '+' or '-'.  Its position is UP_Close.back().AbsLoc clamped into the buffered window: min(max(p, lo), hi).  Per strand
 * (0: '+' anchors, 1: '-' anchors):
 *   the member list     the LI reads' indices sorted by position, ascending read index within one position
 *   the position table  one pg_li_pos per distinct position, ascending: members [first, first + n_reads) of the strand's list.
 *                       n_reads is NOT capped (the reference's counters saturate at Max_short = 128: the consumer's job).  flags:
 *                       PG_LI_LONGER / PG_LI_SHORTER = some member's close end is longer / shorter than half of its read, the
 *                       integer form of LengthStr > ReadLength * 0.5 and < with the read's length after GetCloseEnd (rc_flag).
 * A pure function of the batch (result records, anchor strands, bases), the per-read records of its events build and the window. */
typedef struct { uint32_t lo, hi; } pg_li_window;       /* the buffered window: a position p counts at min(max(p, lo), hi) */
#define PG_LI_LONGER  0x1u           /* some member: 2 * close_len > its post-state read length                             */
#define PG_LI_SHORTER 0x2u           /* some member: 2 * close_len < its post-state read length                             */
typedef struct { uint32_t pos, first, n_reads, flags; } pg_li_pos;            /* 16 bytes */
typedef struct { uint64_t members[2], positions[2]; } pg_li_sizes;            /* 0: '+' anchors, 1: '-' anchors */
/* Builds the tables and keeps them with the batch (a new events build drops them; freed with the batch).  Refused with nothing
 * launched (PG_E_INVALID): a batch that was not searched, a batch without an events build, a null window, lo > hi.  n_reads == 0
 * and "no LI read" are valid.  Synchronous; pg_last_search_stats then reports the HIP-event time of the kernels.
 * pg_device_batch_classify does not run it.  download: members = the two member lists back to back, positions likewise; either may
 * be NULL; the _device sibling fills device memory under the rules of "device buffers in and out". */
int  pg_device_batch_li(pg_ctx *ctx, pg_device_batch *b, const pg_li_window *window);
int  pg_device_batch_li_sizes(pg_ctx *ctx, pg_device_batch *b, pg_li_sizes *sizes);
int  pg_device_batch_li_download(pg_ctx *ctx, pg_device_batch *b, uint32_t *members, pg_li_pos *positions);
int  pg_device_batch_li_download_device(pg_ctx *ctx, pg_device_batch *b, uint32_t *d_members, pg_li_pos *d_positions);

/* ---- device classifier: interchromosomal junction tables ----------------------------------------------------------
 * What SortAndReportInterChromosomalEvents (src/reporter.cpp:2395-2665) takes from the points of the reads whose far end lies on
 * another chromosome -- per read the pair of points that carries its call -- as tables, so that a caller who writes _INT downloads
 * no point.  chr_rank (host memory, n_chr entries): per chromosome of the loaded reference the rank of its name in std::string
 * order, equal names getting equal ranks (the reference walks a std::set<std::string> of names; only the order matters here).
 * A junction read is a read of the batch with 0 <= chr_id < n_chr, an anchor strand '+' or '-', a close end and a far end whose
 * first point (UP_Far[0]) lies on a chromosome fc in [0, n_chr) with chr_rank[chr_id] != chr_rank[fc]: FragName != FarFragName.  No window, no -c / -j filter and no
 * Used state take part (the reference copies these reads before its classifiers run): the build needs a searched batch, no events
 * build.  The call of a junction read, with len its read length after GetCloseEnd (rc_flag):
 *   scan direction   close_ascending = chr_rank[chr_id] < chr_rank[fc] ? the anchor strand is '+' : UP_Far[0] has Strand ANTISENSE
 *   template call    the close points in scan order (index ascending, or descending otherwise); the first one for which some far
 *                    point has LengthStr == len - its LengthStr wins, with the first such far point in the OPPOSITE scan order
 *   fallback call    when no pair fits: c = UP_Close.back(), f = UP_Far.back(), eff = c.LengthStr + f.LengthStr; a call only if
 *                    eff >= 30 and both lengths >= 10.  Its inserted bases are [nt_off, nt_off + nt_len) of the read as rc_flag left
 *                    it: nt_off = f.LengthStr, nt_len = eff > len ? len - nt_off : len - eff (0 where that is negative)
 * A junction read without a call is in no table.  A run list that does not lie in the batch's pool counts as empty.
 *   the member list   the reads that have a call, sorted by key, ascending read index within one key
 *   the call table    one pg_int_call per distinct key: members [first, first + n_reads) of the member list
 * The key is every field of pg_int_call but first / n_reads; the order of both tables is ascending
 * (chr, far_chr, flags, close_abs, far_abs, nt_off, nt_len).  n_reads counts members: it is neither reduced by read names nor split by
 * the inserted bases themselves (two fallback reads with equal offsets and different bases share a call); both are the consumer's job. */
typedef struct { const int32_t *chr_rank; uint32_t n_chr; } pg_int_window;
#define PG_INT_ANCHOR_MINUS 0x1u     /* the anchor strand is not '+'                                                          */
#define PG_INT_FAR_MINUS    0x2u     /* UP_Far[0] has Strand ANTISENSE (the reference's MatchedFarD is '-')                   */
#define PG_INT_FALLBACK     0x4u     /* a fallback call: close_abs / far_abs are the last points', nt_off / nt_len are set    */
typedef struct {
    int16_t  chr, far_chr;           /* the read's chromosome; UP_Far[0]'s                                                    */
    uint32_t close_abs, far_abs;     /* AbsLoc of the chosen close and far point (not reduced by the spacer)                  */
    uint32_t first, n_reads;         /* the members                                                                           */
    uint16_t nt_off, nt_len;         /* the inserted bases within the read as rc_flag left it; 0, 0 for a template call       */
    uint32_t flags;                  /* PG_INT_*                                                                              */
    uint32_t reserved;               /* 0                                                                                     */
} pg_int_call;                       /* 32 bytes, no padding                                                                  */
typedef struct { uint64_t members, calls; } pg_int_sizes;
/* Builds the tables and keeps them with the batch (a new search or upload drops them; freed with the batch).  Refused with nothing
 * launched (PG_E_INVALID): a batch that was not searched, a null window or a null chr_rank, n_chr other than the loaded reference's
 * number of chromosomes.  n_reads == 0 and "no junction read" are valid.  Synchronous; pg_last_search_stats then reports the
 * HIP-event time of the kernels.  pg_device_batch_classify does not run it.  download: either array may be NULL; the _device sibling
 * fills device memory under the rules of "device buffers in and out". */
int  pg_device_batch_int(pg_ctx *ctx, pg_device_batch *b, const pg_int_window *window);
int  pg_device_batch_int_sizes(pg_ctx *ctx, pg_device_batch *b, pg_int_sizes *sizes);
int  pg_device_batch_int_download(pg_ctx *ctx, pg_device_batch *b, uint32_t *members, pg_int_call *calls);
int  pg_device_batch_int_download_device(pg_ctx *ctx, pg_device_batch *b, uint32_t *d_members, pg_int_call *d_calls);

/* ---- device classifier: dispersed-duplication breakpoint tables and consensus ---------------------------------------
 * What searchMEIBreakpoints (src/search_MEI.cpp:367-424) makes of the split reads around its discordant clusters -- per candidate
 * breakpoint the supporting reads, their consensus (get_consensus_unmapped, :156-218) and the containment verdict
 * (contains_subseq_any_strand) -- as tables, so that a caller who writes _DD downloads no point and uploads no consensus.  The build
 * needs a close-searched batch only (pg_device_batch_close_search, or any full search): it reads close_last / close_max / rc_flag of
 * the output records, the anchor strands and the read bytes.
 * Segment s is the reads [seg_first[s], seg_first[s + 1]) of the batch: the split reads ingested for one big-enough cluster (the same
 * BAM record may sit in several segments as separate reads).  A DD read of segment s is a read of it with a close end
 * (close_max != 0) whose anchor strand equals seg_strand[s].  Its key is (s, pos = close_last) -- UP_Close.back() -- and its
 * close_len = close_max.  A candidate is a key with at least min_bp_support DD reads (1 or less admits every key; the reference counts
 * "this read and the later ones with the same position" at a position's first occurrence and never succeeds later: the total count).
 *   the member list     the DD reads of candidates, by (seg, pos) ascending with pos UNSIGNED, ascending read index within a key
 *   the candidate table one pg_dd_cand per candidate in the same order: members [first, first + n_reads)
 *   the consensus pool  the consensus bytes of the candidates back to back: [cons_off, cons_off + cons_len)
 * The signed order of (int)(pos - spacer) that the reference's std::map<int, ...> imposes and the std::sort by unmapped length of a
 * candidate's reads stay with the consumer.
 * Consensus.  Per member, S = the read as rc_flag left it, len its length, u = len - close_len (0 where that is negative).  Column i of
 * a member with u > i is S[u - 1 - i] for a '-' segment and rc4n(S[u - 1 - i]) for a '+' segment (rc4n: A<->T, C<->G, N->N, anything
 * else -> byte 0): the unmapped bases walking away from the breakpoint.  Per column i = 0 .. max u - 1: n = members with u > i; the
 * winner is the byte with the largest count, the smallest byte compared as signed char on a tie (the iteration order of
 * std::map<char,int> with a strict >); the column is accepted iff 5 * max >= 4 * n, and the first rejected column ends the consensus.
 * (The reference tests max_count >= 0.8f * read_count in float: the two agree for every n up to 200 000 at the threshold and one
 * either side of it.)  Fewer than 15 columns: cons_len = 0, no bytes in the pool, not tested.  Otherwise a '+' segment stores the
 * bytes in column order and a '-' segment reversed.
 * Containment, per tested candidate: win_start = max(0, (int)pos - min_map_distance), win_len = min(padded length of chr_id -
 * win_start, 2 * min_map_distance) (0 where win_start is not below that length; the unsigned expressions of the reference otherwise),
 * and PG_DD_CONTAINED = pg_dd_contains_batch of the consensus in that window. */
typedef struct {
    const uint32_t *seg_first;   /* host, n_seg + 1 read indices, non-decreasing, seg_first[n_seg] <= n_reads   */
    const uint8_t  *seg_strand;  /* host, n_seg bytes '+' / '-': the strand of the segment's discordant cluster  */
    uint32_t n_seg;
    int32_t  chr_id;             /* the window's chromosome (containment window, all reads' chr_id)              */
    int32_t  min_bp_support;     /* --MIN_DD_BREAKPOINT_SUPPORT                                                  */
    int32_t  min_map_distance;   /* --MIN_DD_MAP_DISTANCE, >= 1                                                  */
} pg_dd_window;
typedef struct { uint32_t read; uint16_t close_len; uint8_t rc_flag, reserved; } pg_dd_member;        /*  8 bytes */
typedef struct { uint32_t seg, pos, first, n_reads, cons_off, cons_len, flags, win_len; uint64_t win_start; } pg_dd_cand; /* 40 bytes, no padding */
#define PG_DD_TESTED    0x1u   /* cons_len >= 15: the containment test ran */
#define PG_DD_CONTAINED 0x2u   /* ... and found the consensus in the window */
typedef struct { uint64_t members, cands, cons_bytes; } pg_dd_sizes;
/* Builds the tables and keeps them with the batch (a new search or upload drops them; freed with the batch).  Refused with nothing
 * launched (PG_E_INVALID): a batch that is not close-searched, a null window, n_seg > 0 with a null array, seg_first decreasing or
 * beyond n_reads, a strand byte other than '+' / '-', chr_id outside the reference, min_map_distance < 1.  n_reads == 0, n_seg == 0
 * and "no candidate" are valid (a batch of no reads has nothing to search: it is accepted whether it was close-searched or not, as
 * the entries that need a full search accept it).  Synchronous; pg_last_search_stats then reports the summed HIP-event time of the kernels.
 * pg_device_batch_classify does not run it.  download: any pointer may be NULL; the _device sibling fills device memory under the
 * rules of "device buffers in and out". */
int  pg_device_batch_dd(pg_ctx *ctx, pg_device_batch *b, const pg_dd_window *window);
int  pg_device_batch_dd_sizes(pg_ctx *ctx, pg_device_batch *b, pg_dd_sizes *sizes);
int  pg_device_batch_dd_download(pg_ctx *ctx, pg_device_batch *b, pg_dd_member *members, pg_dd_cand *cands, uint8_t *cons);
int  pg_device_batch_dd_download_device(pg_ctx *ctx, pg_device_batch *b, pg_dd_member *d_members, pg_dd_cand *d_cands, uint8_t *d_cons);

/* -q (dispersed duplications): per item i, contains_subseq_any_strand(query_i, window_i, 15) of Pindel's MEI search
 * (src/search_MEI_util.cpp:188-351, bit-exact), where query_i = query[query_off[i] .. query_off[i+1]) (at most
 * PG_MAX_READ_LEN bases) and window_i = the loaded chromosome chr_id[i] at padded (AbsLoc) positions
 * [win_start[i], win_start[i] + win_len[i]), read from the planes on the device.  out[i] = 0 / 1.  Synchronous;
 * pg_last_search_stats then reports the kernel's HIP-event time. */
int  pg_dd_contains_batch(pg_ctx *ctx, uint32_t n, const uint8_t *query, const uint64_t *query_off, const int32_t *chr_id,
                          const uint64_t *win_start, const uint32_t *win_len, uint8_t *out);

#ifdef __cplusplus
}
#endif
#endif /* PINDEL_PG_H */
