// pg_host_capi.cpp -- C entry points of the host library (libpindel_host.so): the steps
// before and after the hot path (loaders, classifiers, reporters), callable from tests and
// from the pindel_pg command line.  No search code here.
#include <cctype>
#include <chrono>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "pg_bam.hpp"
#include "pg_bdhints.hpp"
#include "pg_dd.hpp"
#include "pg_depth.hpp"
#include "pg_host.hpp"
#include "pg_host_events.hpp"
#include "pg_host_report.hpp"
#include "pg_host_sv_events.hpp"
#include "pg_host_priv.hpp"
#include "pg_pipeline.hpp"
#include "pg_rp.hpp"
#include "pg_vcf.hpp"
#include "pindel_pg.h"

using namespace pgh;
using namespace pgh::detail;

static std::string g_err;

extern "C" {

const char *pgh_last_error(void) { return g_err.c_str(); }

struct pgh_settings {
    uint32_t spacer;
    uint32_t min_support;        /* -M */
    uint32_t balance_cutoff;     /* -B */
    double seq_error_rate;       /* -e */
    int32_t min_num_matched_bases; /* -d */
    int32_t min_inversion_size;  /* -v */
    int32_t analyze_td, analyze_inv;
    double window_mbp;           /* -w */
    uint32_t max_mismatch[500];  /* g_maxMismatch (pg_get_max_mismatch) */
    int32_t analyze_li;          /* -l: also write <prefix>_LI */
    int32_t report_close_mapped; /* -s: also write <prefix>_CloseEndMapped */
    const char *region;          /* -c: NULL or "" = ALL */
    const char *include_bed;     /* -j: NULL or "" = none */
    const char *exclude_bed;     /* -J: NULL or "" = none */
    int32_t report_interchromosomal; /* -I: also write <prefix>_INT and <prefix>_INT_final */
    int32_t normal_samples;      /* -N: the germline filter of _TD and _INV (acts with bam_config only) */
    const char *bam_config;      /* NULL or "" = the reads are text input; else the -i configuration they were derived from */
    const char *pindel_config;   /* -P: NULL or "" = none; else its files are read before reads_path */
    uint32_t repairs;            /* --repair: REPAIR_* bits (pg_host.hpp; pgh_parse_repairs); 0 = none.  Last, so earlier layouts hold */
};

static std::string str_or_empty(const char *s) { return s ? s : ""; }

/*
 * Pindel's post-search pipeline for a Pindel-text read file: attaches the given UP_Close /
 * UP_Far (CSR over ALL reads of the file, in file order; reads without close end have an
 * empty range) and the rc flags, then walks chromosomes and 5-Mbp bins like main()
 * (pindel.cpp:1778-1989) and appends <prefix>_D, _SI, _TD, _INV -- and _LI / _CloseEndMapped when
 * analyze_li / report_close_mapped are set, _INT and _INT_final when report_interchromosomal is.  region / include_bed / exclude_bed: the region plan (pg_region.hpp).
 * pindel_config (-P): its files are read first, then reads_path (which may then be NULL or ""); the point arrays cover
 * the concatenated reads in load order.  normal_samples with bam_config: the reads are taken as derived from the BAMs
 * of that -i configuration, so IsGoodTD / IsGoodINV filter as they do for BAM input and read depth comes from those
 * BAMs (pg_depth.hpp); without bam_config the reads are text input and -N changes nothing, as in the reference.
 * repairs: int-pairs, depth-mapq and bed0 act as on the command line; inv-pairs, with normal_samples and
 * bam_config, discovers the discordant read pairs of every window in those BAMs (-A 0) for the inversion filter.
 */
static int call_from_points(const char *fasta_path, const char *reads_path, const char *out_prefix,
                            const pgh_settings *st, uint32_t n_reads,
                            const uint64_t *close_off, const pg_point *close_pts,
                            const uint64_t *far_off, const pg_point *far_pts, const uint8_t *rc_flag,
                            const pg_variant_cand *var_cands, const uint8_t *var_counts,
                            const pg_variant_cand *sv_cands = nullptr, const uint8_t *sv_counts = nullptr, bool use_events = false,
                            const std::vector<SuppliedEvents> *supplied = nullptr, bool use_sv_events = false,
                            const std::vector<SuppliedSvEvents> *supplied_sv = nullptr, bool use_report_reads = false)
{
    std::vector<Chromosome> genome;
    if (load_fasta(fasta_path, genome, st->spacer, g_err)) return -1;
    std::vector<SplitRead> all;
    if (load_pindel_inputs(str_or_empty(st->pindel_config), str_or_empty(reads_path), genome, all, g_err)) return -1;
    if (all.size() != n_reads) {
        g_err = "read count mismatch between the read file and the point arrays";
        return -1;
    }
    Settings S;
    S.spacer = st->spacer;
    S.NumRead2ReportCutOff = st->min_support;
    S.BalanceCutoff = st->balance_cutoff;
    S.Seq_Error_Rate = st->seq_error_rate;
    S.Min_Num_Matched_Bases = st->min_num_matched_bases;
    S.MIN_IndelSize_Inversion = st->min_inversion_size;
    S.Analyze_TD = st->analyze_td != 0;
    S.Analyze_INV = st->analyze_inv != 0;
    S.window_mbp = st->window_mbp;
    S.Analyze_LI = st->analyze_li != 0;
    S.report_close_mapped = st->report_close_mapped != 0;
    S.report_interchromosomal = st->report_interchromosomal != 0;
    memcpy(S.max_mismatch, st->max_mismatch, sizeof S.max_mismatch);
    S.NormalSamples = st->normal_samples != 0;
    S.repairs = st->repairs;
    S.use_events = use_events;
    if (supplied) S.supplied_events = *supplied;
    S.use_sv_events = use_sv_events;
    if (supplied_sv) S.supplied_sv_events = *supplied_sv;
    S.use_report_reads = use_report_reads;
    event_path_stats() = EventPathStats();
    if (S.repairs & ~(uint32_t)REPAIR_ALL) {
        g_err = "unknown bits in the repairs field";
        return -1;
    }
    std::vector<BamSource> bams;
    if (S.NormalSamples && st->bam_config && st->bam_config[0]) {
        if (!read_bam_config(st->bam_config, bams, g_err) || !(S.germline = open_germline(bams, g_err, S.repairs))) return -1;
    }
    // --repair inv-pairs: readers of their own on the BAMs, one window at a time
    std::vector<BamFile> pair_files;
    std::vector<int> pair_isz;
    std::vector<std::string> pair_tags;
    WindowPairs pairs_of;
    if (S.germline_filter() && S.repair(REPAIR_INV_PAIRS)) {
        pair_files = std::vector<BamFile>(bams.size());
        for (size_t k = 0; k < bams.size(); k++) {
            if (!pair_files[k].open(bams[k].path, g_err)) return -1;
            pair_isz.push_back(bams[k].insert_size);
            pair_tags.push_back(bams[k].tag);
        }
        pairs_of = [&](const Chromosome &chrom, unsigned ws, unsigned we, std::vector<DiscordantPair> &out) {
            return window_pairs(pair_files, pair_isz, pair_tags, chrom.name, ws, we, 0, S.spacer, out);
        };
    }
    std::vector<RegionRecord> plan;
    if (region_plan(chromosome_names(genome), chromosome_sizes(genome, read_fai(fasta_path, genome), S.spacer), str_or_empty(st->region),
                    str_or_empty(st->include_bed), str_or_empty(st->exclude_bed), plan, g_err, S.repair(REPAIR_BED0)))
        return -1;
    auto attach = [&](const Chromosome &, int, std::vector<SplitRead> &reads, const std::vector<uint32_t> &index) {
        for (size_t k = 0; k < reads.size(); k++) {
            const uint32_t i = index[k];
            SplitRead &r = reads[k];
            for (uint8_t k = 0; k < rc_flag[i] && k < 2; k++) {      // setUnmatchedSeq(ReverseComplement()), once or twice
                r.UnmatchedSeq = reverse_complement(r.UnmatchedSeq);
                while (!r.UnmatchedSeq.empty() && !std::isalnum((unsigned char)r.UnmatchedSeq.back())) r.UnmatchedSeq.pop_back();
            }
            for (uint64_t q = close_off[i]; q < close_off[i + 1]; q++) r.UP_Close.push_back(to_unique_point(close_pts[q]));
            for (uint64_t q = far_off[i]; q < far_off[i + 1]; q++) r.UP_Far.push_back(to_unique_point(far_pts[q]));
            if (var_cands) {
                r.VarCands = var_cands + (size_t)i * 2 * PG_VARIANT_CANDS;
                r.VarCounts = var_counts + (size_t)i * 2;
            }
            if (sv_cands) {
                r.SvCands = sv_cands + (size_t)i * PG_SV_SLOTS;
                r.SvCounts = sv_counts + (size_t)i * PG_SV_KINDS;
            }
            r.VarIndex = i;
        }
        return 0;
    };
    VariantListStats &vs = variant_list_stats();
    vs.fallbacks = 0;
    vs.visits.clear();
    vs.log_visits = var_cands != nullptr || sv_cands != nullptr;
    return run_pipeline(genome, plan, all, S, out_prefix, attach, pgh::NoFarSearch(), g_err, nullptr, pairs_of);
}

int pgh_call_from_points(const char *fasta_path, const char *reads_path, const char *out_prefix,
                         const pgh_settings *st, uint32_t n_reads,
                         const uint64_t *close_off, const pg_point *close_pts,
                         const uint64_t *far_off, const pg_point *far_pts, const uint8_t *rc_flag)
{
    return call_from_points(fasta_path, reads_path, out_prefix, st, n_reads, close_off, close_pts, far_off, far_pts, rc_flag, nullptr, nullptr);
}

/*
 * pgh_call_from_points with the per-read stage of the deletion and short-insertion classifiers fed from candidate lists
 * (pg_variant_cand, pindel_pg.h; what pg_device_batch_variant_candidates or pgh_variant_candidates yield): var_cands holds
 * n_reads x 2 kinds x PG_VARIANT_CANDS records, var_counts n_reads x 2 count bytes.  Each classifier takes a read's pairs
 * from its list, in order, and applies the window-dependent tests to them; a read whose list is exhausted, with
 * PG_VARIANT_MORE set, before a pair has made it Used goes through the pair search instead (pgh_last_variant_fallbacks
 * counts those).  The reports are the bytes pgh_call_from_points writes.
 */
int pgh_call_from_points_candidates(const char *fasta_path, const char *reads_path, const char *out_prefix,
                                    const pgh_settings *st, uint32_t n_reads,
                                    const uint64_t *close_off, const pg_point *close_pts,
                                    const uint64_t *far_off, const pg_point *far_pts, const uint8_t *rc_flag,
                                    const pg_variant_cand *var_cands, const uint8_t *var_counts)
{
    if (!var_cands || !var_counts) {
        g_err = "pgh_call_from_points_candidates: null candidate arrays";
        return -1;
    }
    return call_from_points(fasta_path, reads_path, out_prefix, st, n_reads, close_off, close_pts, far_off, far_pts, rc_flag, var_cands, var_counts);
}

/*
 * ... with the lists of the five other classifiers as well (what pg_device_batch_sv_candidates or pgh_sv_candidates
 * yield): sv_cands holds n_reads x PG_SV_SLOTS records, sv_counts n_reads x PG_SV_KINDS count bytes.  Either pair of arrays may be
 * null: those classifiers then search the pairs themselves.  With a -v outside [0, PG_SV_MAX_INVERSION_SIZE] the inversion
 * classifiers do not consult their lists.  The fallback counter and the visit hook cover all seven kinds.
 */
int pgh_call_from_points_lists(const char *fasta_path, const char *reads_path, const char *out_prefix, const pgh_settings *st,
                               uint32_t n_reads, const uint64_t *close_off, const pg_point *close_pts, const uint64_t *far_off,
                               const pg_point *far_pts, const uint8_t *rc_flag, const pg_variant_cand *var_cands, const uint8_t *var_counts,
                               const pg_variant_cand *sv_cands, const uint8_t *sv_counts)
{
    if ((var_cands == nullptr) != (var_counts == nullptr) || (sv_cands == nullptr) != (sv_counts == nullptr) || (!var_cands && !sv_cands)) {
        g_err = "pgh_call_from_points_lists: candidate arrays come in pairs, and at least one pair";
        return -1;
    }
    return call_from_points(fasta_path, reads_path, out_prefix, st, n_reads, close_off, close_pts, far_off, far_pts, rc_flag, var_cands, var_counts,
                            sv_cands, sv_counts);
}

/*
 * pgh_call_from_points_lists with the events path switched on: per window process_window builds the event tables
 * from the lists (pgh_events_from_lists' function) and writes deletions, short insertions and tandem duplications from them; DI and
 * the inversions take their boxes from the per-read records.  Both pairs of list arrays are needed.  A window with an unresolved
 * read takes the existing path as a whole (pgh_last_event_fallback_windows).  supplied: n_supplied tables built elsewhere (on the
 * device) for the window (chr, win_start, win_end) over all n_reads reads; a window without an entry uses the host builder.  The
 * reports are the bytes pgh_call_from_points writes.
 */
struct pgh_supplied_events {
    int32_t chr;
    uint32_t win_start, win_end, reserved;
    const pg_event_read *reads;
    const uint32_t *members;
    const pg_event *events;
    pg_event_sizes sizes;
};
int pgh_call_from_points_events(const char *fasta_path, const char *reads_path, const char *out_prefix, const pgh_settings *st,
                                uint32_t n_reads, const uint64_t *close_off, const pg_point *close_pts, const uint64_t *far_off,
                                const pg_point *far_pts, const uint8_t *rc_flag, const pg_variant_cand *var_cands, const uint8_t *var_counts,
                                const pg_variant_cand *sv_cands, const uint8_t *sv_counts, int32_t n_supplied, const pgh_supplied_events *sup)
{
    if (!var_cands || !var_counts || !sv_cands || !sv_counts) {
        g_err = "pgh_call_from_points_events: the lists of both device classifiers are needed";
        return -1;
    }
    std::vector<SuppliedEvents> supplied;
    for (int32_t k = 0; k < n_supplied; k++) {
        SuppliedEvents e;
        e.chr = sup[k].chr;
        e.win_start = sup[k].win_start;
        e.win_end = sup[k].win_end;
        e.n_reads = n_reads;
        e.reads = sup[k].reads;
        e.members = sup[k].members;
        e.events = sup[k].events;
        e.sizes = sup[k].sizes;
        supplied.push_back(e);
    }
    return call_from_points(fasta_path, reads_path, out_prefix, st, n_reads, close_off, close_pts, far_off, far_pts, rc_flag, var_cands, var_counts,
                            sv_cands, sv_counts, true, &supplied);
}
/*
 * pgh_call_from_points_events with the sv_events path switched on as well: DI and the inversions are written from
 * their SV tables -- built per window by pgh_sv_events_from_lists' function, or supplied (sv_sup: n_sv_supplied tables built on the
 * device over all n_reads reads, each beside the entry of `sup` for the same window; tables that do not fit the window are
 * replaced by the host's own) -- where the events path alone calls sort_output_di and sort_output_inv.  A window that falls back
 * falls back as a whole.  The reports are the bytes pgh_call_from_points writes.
 */
struct pgh_supplied_sv_events {
    int32_t chr;
    uint32_t win_start, win_end, reserved;
    const uint32_t *members;
    const pg_event *events;
    pg_sv_event_sizes sizes;
};
int pgh_call_from_points_sv_events(const char *fasta_path, const char *reads_path, const char *out_prefix, const pgh_settings *st,
                                   uint32_t n_reads, const uint64_t *close_off, const pg_point *close_pts, const uint64_t *far_off,
                                   const pg_point *far_pts, const uint8_t *rc_flag, const pg_variant_cand *var_cands, const uint8_t *var_counts,
                                   const pg_variant_cand *sv_cands, const uint8_t *sv_counts, int32_t n_supplied, const pgh_supplied_events *sup,
                                   int32_t n_sv_supplied, const pgh_supplied_sv_events *sv_sup)
{
    if (!var_cands || !var_counts || !sv_cands || !sv_counts) {
        g_err = "pgh_call_from_points_sv_events: the lists of both device classifiers are needed";
        return -1;
    }
    std::vector<SuppliedEvents> supplied;
    for (int32_t k = 0; k < n_supplied; k++) {
        SuppliedEvents e;
        e.chr = sup[k].chr;
        e.win_start = sup[k].win_start;
        e.win_end = sup[k].win_end;
        e.n_reads = n_reads;
        e.reads = sup[k].reads;
        e.members = sup[k].members;
        e.events = sup[k].events;
        e.sizes = sup[k].sizes;
        supplied.push_back(e);
    }
    std::vector<SuppliedSvEvents> supplied_sv;
    for (int32_t k = 0; k < n_sv_supplied; k++) {
        SuppliedSvEvents e;
        e.chr = sv_sup[k].chr;
        e.win_start = sv_sup[k].win_start;
        e.win_end = sv_sup[k].win_end;
        e.members = sv_sup[k].members;
        e.events = sv_sup[k].events;
        e.sizes = sv_sup[k].sizes;
        supplied_sv.push_back(e);
    }
    return call_from_points(fasta_path, reads_path, out_prefix, st, n_reads, close_off, close_pts, far_off, far_pts, rc_flag, var_cands, var_counts,
                            sv_cands, sv_counts, true, &supplied, true, &supplied_sv);
}
/*
 * pgh_call_from_points_sv_events with the tables path switched on: per window the host statements build lists ->
 * tables -> report records -> summaries, the window's reads are replaced by copies without points, lists and pair fields, and
 * Caller::process_window_tables writes the reports from tables, records and summaries alone.  A window with an unresolved read, or
 * whose tables do not fit, takes the existing path and is counted, as before.  The reports are the bytes pgh_call_from_points writes.
 * With analyze_li / report_close_mapped _LI and _CloseEndMapped take the same route: the host statement builds the
 * window's long-insertion tables while its reads still have points, _CloseEndMapped is written from the summaries, and the shared
 * consumer writes _LI from the tables after the reads were stripped; a window that falls back writes both the existing way.
 */
int pgh_call_from_points_report_reads(const char *fasta_path, const char *reads_path, const char *out_prefix, const pgh_settings *st,
                                      uint32_t n_reads, const uint64_t *close_off, const pg_point *close_pts, const uint64_t *far_off,
                                      const pg_point *far_pts, const uint8_t *rc_flag, const pg_variant_cand *var_cands, const uint8_t *var_counts,
                                      const pg_variant_cand *sv_cands, const uint8_t *sv_counts)
{
    if (!var_cands || !var_counts || !sv_cands || !sv_counts) {
        g_err = "pgh_call_from_points_report_reads: the lists of both device classifiers are needed";
        return -1;
    }
    return call_from_points(fasta_path, reads_path, out_prefix, st, n_reads, close_off, close_pts, far_off, far_pts, rc_flag, var_cands, var_counts,
                            sv_cands, sv_counts, true, nullptr, true, nullptr, true);
}
/* windows of the last run written by process_window_tables, and the report records they took */
uint64_t pgh_last_report_windows(void) { return event_path_stats().report_windows; }
uint64_t pgh_last_report_records(void) { return event_path_stats().report_records; }
/* ... and those whose _INT was written by the consumer from the window's junction tables */
uint64_t pgh_last_int_table_windows(void) { return event_path_stats().int_table_windows; }
/* windows of the last run whose DI and inversion reports came from SV tables / ... from supplied SV tables */
uint64_t pgh_last_sv_event_table_windows(void) { return event_path_stats().sv_table_windows; }
uint64_t pgh_last_sv_event_supplied_windows(void) { return event_path_stats().sv_supplied_windows; }
/* windows of the last run with the events path that took the existing path / were written from tables / ... from supplied tables */
uint64_t pgh_last_event_fallback_windows(void) { return event_path_stats().fallback_windows; }
uint64_t pgh_last_event_table_windows(void) { return event_path_stats().table_windows; }
uint64_t pgh_last_event_supplied_windows(void) { return event_path_stats().supplied_windows; }
/* the windows the events path saw, six values each: chromosome index, win_start, win_end, region_start, region_end, reads */
uint64_t pgh_last_event_windows(uint32_t *out, uint64_t cap)
{
    const std::vector<uint32_t> &v = event_path_stats().windows;
    const uint64_t n = v.size() / 6;
    if (out) std::copy(v.begin(), v.begin() + (size_t)std::min(n, cap) * 6, out);
    return n;
}

/* reads of the last pgh_call_from_points_candidates that went through the pair search after their list (both kinds, all windows) */
uint64_t pgh_last_variant_fallbacks(void) { return variant_list_stats().fallbacks; }

/*
 * Test hook: every consultation of a list in the last pgh_call_from_points_candidates, seven values each -- read index, kind,
 * and what the window-dependent tests compared against: the window's end, the region's start and end, the number of boxes and
 * the box size.  Returns the number of consultations (only cap are written); their order is not defined.
 */
uint64_t pgh_last_variant_visits(uint32_t *out, uint64_t cap)
{
    const std::vector<uint32_t> &v = variant_list_stats().visits;
    const uint64_t n = v.size() / 7;
    if (out) std::copy(v.begin(), v.begin() + (size_t)std::min(n, cap) * 7, out);
    return n;
}

/*
 * The per-read stage of SearchVariant::Search as candidate lists (pg_variant_cand, pindel_pg.h), on the host: for every read and
 * both kinds the first PG_VARIANT_CANDS distinct qualifying pairs in the order the loops first visit them, and PG_VARIANT_MORE
 * when there are more.  Written as those loops -- mismatch budget, close points, every far point from the highest index down --
 * around the function the classifier itself uses for a pair: the reference the device classifier is tested against.
 * chr_seq[c]: the padded chromosome (spacer N's on both sides), chr_len[c] its length.  The reads come as they were handed to the
 * search (seq, seq_off, strand, chr_id) with its rc flags and the expanded points (CSR); ReadLength and MAX_SNP_ERROR are taken
 * from the read as rc_flag applications of setUnmatchedSeq(ReverseComplement()) leave it.  mm500 = g_maxMismatch.
 * cands: n_reads x 2 x PG_VARIANT_CANDS records (unused ones zeroed), counts: n_reads x 2.
 */
int pgh_variant_candidates(int32_t n_chr, const char *const *chr_seq, const uint64_t *chr_len, uint32_t spacer, uint32_t n_reads,
                           const uint8_t *seq, const uint64_t *seq_off, const uint8_t *strand, const int32_t *chr_id, const uint8_t *rc_flag,
                           const uint64_t *close_off, const pg_point *close_pts, const uint64_t *far_off, const pg_point *far_pts,
                           const uint32_t *mm500, pg_variant_cand *cands, uint8_t *counts)
{
    std::vector<std::string> ref((size_t)std::max(n_chr, 0));
    for (int32_t c = 0; c < n_chr; c++) ref[(size_t)c].assign(chr_seq[c], (size_t)chr_len[c]);
    memset(cands, 0, (size_t)n_reads * 2 * PG_VARIANT_CANDS * sizeof(pg_variant_cand));
    memset(counts, 0, (size_t)n_reads * 2);
    pg_adapter::parallel_ranges(n_reads, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) {
            if (far_off[i + 1] == far_off[i] || close_off[i + 1] == close_off[i]) continue;
            if (strand[i] != '+' && strand[i] != '-') continue;
            if (chr_id[i] < 0 || chr_id[i] >= n_chr) continue;
            if (far_pts[far_off[i]].chr_id != chr_id[i]) continue;           // FragName != FarFragName (UpdateFarFragName: the first far point's)
            SplitRead r;
            r.UnmatchedSeq.assign((const char *)seq + seq_off[i], (size_t)(seq_off[i + 1] - seq_off[i]));
            pg_adapter::apply_rc_flag(r, rc_flag[i]);
            r.ReadLength = (short)r.UnmatchedSeq.size();
            r.MAX_SNP_ERROR = (short)mm500[std::min<int>(r.ReadLength, 499)];
            r.MatchedD = (char)strand[i];
            for (uint64_t q = close_off[i]; q < close_off[i + 1]; q++) r.UP_Close.push_back(to_unique_point(close_pts[q]));
            for (uint64_t q = far_off[i]; q < far_off[i + 1]; q++) r.UP_Far.push_back(to_unique_point(far_pts[q]));
            const bool plus = r.MatchedD == '+';
            const int nc = (int)r.UP_Close.size(), nf = (int)r.UP_Far.size();
            for (int kind = 0; kind < 2; kind++) {
                pg_variant_cand *list = cands + (i * 2 + (size_t)kind) * PG_VARIANT_CANDS;
                std::vector<std::pair<int, int>> seen;                       // pairs listed so far (a pair comes round again at every higher budget)
                unsigned n_listed = 0;
                bool more = false, stop = false;
                VariantPair pair;
                for (short budget = 0; budget <= r.MAX_SNP_ERROR && !stop; budget++)
                    for (int k = 0; k < nc && !stop; k++) {
                        const int ci = plus ? k : nc - 1 - k;
                        const UniquePoint &cp = r.UP_Close[ci];
                        if (cp.Mismatches > budget) continue;
                        for (int fi = nf - 1; fi >= 0 && !stop; fi--) {
                            const UniquePoint &fp = r.UP_Far[fi];
                            if (fp.Mismatches > budget) continue;
                            if (fp.Mismatches + cp.Mismatches > budget) continue;
                            if (std::find(seen.begin(), seen.end(), std::make_pair(ci, fi)) != seen.end()) continue;
                            if (!variant_pair(r, kind, ci, fi, ref[(size_t)chr_id[i]], spacer, pair)) continue;
                            if (n_listed == PG_VARIANT_CANDS) {
                                more = stop = true;
                                break;
                            }
                            seen.push_back(std::make_pair(ci, fi));
                            list[n_listed++] = pair.c;
                            if (pair.c.flags & PG_VARIANT_REF_END) stop = true;   // the loop marks the read Used: no later pair is tried
                        }
                    }
                counts[i * 2 + (size_t)kind] = (uint8_t)(n_listed | (more ? PG_VARIANT_MORE : 0u));
            }
        }
    });
    return 0;
}

/*
 * The per-read stage of the five other classifiers as candidate lists, on the host: plain loops over mismatch
 * budget, close points and every far point in the classifier's own order around the functions the classifiers use for a pair
 * (pg_host_priv.hpp) -- the reference the device classifier (pg_sv_kernel) is tested against.  Inputs as pgh_variant_candidates,
 * plus prm.  cands: n_reads x PG_SV_SLOTS records (unused ones zeroed), counts: n_reads x PG_SV_KINDS.  -1: prm is refused.
 */
int pgh_sv_candidates(int32_t n_chr, const char *const *chr_seq, const uint64_t *chr_len, uint32_t spacer, uint32_t n_reads,
                      const uint8_t *seq, const uint64_t *seq_off, const uint8_t *strand, const int32_t *chr_id, const uint8_t *rc_flag,
                      const uint64_t *close_off, const pg_point *close_pts, const uint64_t *far_off, const pg_point *far_pts,
                      const uint32_t *mm500, const pg_sv_params *prm, pg_variant_cand *cands, uint8_t *counts)
{
    if (!prm || prm->min_inversion_size < 0 || prm->min_inversion_size > PG_SV_MAX_INVERSION_SIZE) {
        g_err = "pgh_sv_candidates: the minimum inversion size must lie in [0, 2^30]";
        return -1;
    }
    std::vector<std::string> ref((size_t)std::max(n_chr, 0));
    for (int32_t c = 0; c < n_chr; c++) ref[(size_t)c].assign(chr_seq[c], (size_t)chr_len[c]);
    memset(cands, 0, (size_t)n_reads * PG_SV_SLOTS * sizeof(pg_variant_cand));
    memset(counts, 0, (size_t)n_reads * PG_SV_KINDS);
    const unsigned MIN = (unsigned)prm->min_inversion_size;
    pg_adapter::parallel_ranges(n_reads, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) {
            if (far_off[i + 1] == far_off[i] || close_off[i + 1] == close_off[i]) continue;
            if (strand[i] != '+' && strand[i] != '-') continue;
            if (chr_id[i] < 0 || chr_id[i] >= n_chr) continue;
            if (far_pts[far_off[i]].chr_id != chr_id[i]) continue;           // FragName != FarFragName
            SplitRead r;
            r.UnmatchedSeq.assign((const char *)seq + seq_off[i], (size_t)(seq_off[i + 1] - seq_off[i]));
            pg_adapter::apply_rc_flag(r, rc_flag[i]);
            r.ReadLength = (short)r.UnmatchedSeq.size();
            r.MAX_SNP_ERROR = (short)mm500[std::min<int>(r.ReadLength, 499)];
            r.MatchedD = (char)strand[i];
            for (uint64_t q = close_off[i]; q < close_off[i + 1]; q++) r.UP_Close.push_back(to_unique_point(close_pts[q]));
            for (uint64_t q = far_off[i]; q < far_off[i + 1]; q++) r.UP_Far.push_back(to_unique_point(far_pts[q]));
            const std::string &chr = ref[(size_t)chr_id[i]];
            const bool plus = r.MatchedD == '+';
            const int nc = (int)r.UP_Close.size(), nf = (int)r.UP_Far.size();
            pg_variant_cand *rec = cands + i * PG_SV_SLOTS;
            uint8_t *cnt = counts + i * PG_SV_KINDS;
            VariantPair pair;
            if (sv_pair_di(r, *prm, spacer, pair)) {
                rec[sv_slot_base()[0]] = pair.c;
                cnt[0] = 1;
            }
            if (sv_pair_td_nt(r, *prm, spacer, pair)) {
                rec[sv_slot_base()[2]] = pair.c;
                cnt[2] = 1;
            }
            if (sv_inv_nt_read_ok(r, *prm))
                for (int which = 0; which < 2 && !cnt[4]; which++)
                    if (sv_pair_inv_nt(r, *prm, which, spacer, pair)) {
                        rec[sv_slot_base()[4]] = pair.c;
                        cnt[4] = 1;
                    }
            // the two kinds with loops: first visits of distinct pairs, in the loops' order
            const int geo = sv_inv_read_ok(r) ? sv_inv_geometry(r, MIN) : -1;
            for (int kind : { (int)PG_SV_TD, (int)PG_SV_INV }) {
                if (kind == PG_SV_INV && geo < 0) continue;
                const bool close_asc = kind == PG_SV_TD ? plus : (geo == 1 || geo == 3);
                const bool far_asc = kind == PG_SV_TD ? !plus : (geo == 0 || geo == 2);
                pg_variant_cand *list = rec + sv_slot_base()[kind - PG_SV_DI];
                std::vector<std::pair<int, int>> seen;
                unsigned n_listed = 0;
                bool more = false, stop = false;
                for (short budget = 0; budget <= r.MAX_SNP_ERROR && !stop; budget++)
                    for (int k = 0; k < nc && !stop; k++) {
                        const int ci = close_asc ? k : nc - 1 - k;
                        const UniquePoint &cp = r.UP_Close[ci];
                        if (cp.Mismatches > budget) continue;
                        for (int j = 0; j < nf && !stop; j++) {
                            const int fi = far_asc ? j : nf - 1 - j;
                            const UniquePoint &fp = r.UP_Far[fi];
                            if (fp.Mismatches > budget) continue;
                            if (fp.Mismatches + cp.Mismatches > budget) continue;
                            if (std::find(seen.begin(), seen.end(), std::make_pair(ci, fi)) != seen.end()) continue;
                            if (!(kind == PG_SV_TD ? sv_pair_td(r, ci, fi, chr, spacer, pair) : sv_pair_inv(r, geo, ci, fi, MIN, chr, spacer, pair)))
                                continue;
                            if (n_listed == PG_VARIANT_CANDS) {
                                more = stop = true;
                                break;
                            }
                            seen.push_back(std::make_pair(ci, fi));
                            list[n_listed++] = pair.c;
                            if (pair.c.flags & PG_VARIANT_REF_END) stop = true;   // the read is Used: no later pair is tried
                        }
                    }
                cnt[kind - PG_SV_DI] = (uint8_t)(n_listed | (more ? PG_VARIANT_MORE : 0u));
            }
        }
    });
    return 0;
}

/*
 * Event tables from candidate lists (pindel_pg.h "window tail, boxes and event tables"), on the host: the plain-loop
 * statement (pg_host_events.hpp) the device entry pg_device_batch_events is compared with, byte for byte.  The reads and points as
 * pgh_variant_candidates takes them, plus insert_size; either pair of list arrays and name_id may be null.  out_reads: n_reads
 * records; out_members / out_events: room for n_reads entries each (a read is boxed at most once), filled table after table;
 * sizes: what was filled.  -1: the window is refused (chr_id outside the reference, region_start > region_end).
 */
int pgh_events_from_lists(int32_t n_chr, const char *const *chr_seq, const uint64_t *chr_len, uint32_t spacer, uint32_t n_reads,
                          const uint8_t *seq, const uint64_t *seq_off, const uint8_t *strand, const int32_t *chr_id, const uint8_t *rc_flag,
                          const int16_t *insert_size, const uint64_t *close_off, const pg_point *close_pts, const uint64_t *far_off,
                          const pg_point *far_pts, const pg_event_window *w, const pg_variant_cand *cands, const uint8_t *counts,
                          const pg_variant_cand *sv_cands, const uint8_t *sv_counts, const uint32_t *name_id, pg_event_read *out_reads,
                          uint32_t *out_members, pg_event *out_events, pg_event_sizes *sizes)
{
    if (!w || !sizes || w->chr_id < 0 || w->chr_id >= n_chr) {
        g_err = "pgh_events_from_lists: the window's chr_id lies outside the reference";
        return -1;
    }
    if (w->region_start > w->region_end) {
        g_err = "pgh_events_from_lists: region_start > region_end";
        return -1;
    }
    if ((cands == nullptr) != (counts == nullptr) || (sv_cands == nullptr) != (sv_counts == nullptr)) {
        g_err = "pgh_events_from_lists: candidate arrays come in pairs";
        return -1;
    }
    const std::string ref(chr_seq[w->chr_id], (size_t)chr_len[w->chr_id]);
    auto post_state = [&](uint32_t i, SplitRead &r) {
        r.UnmatchedSeq.assign((const char *)seq + seq_off[i], (size_t)(seq_off[i + 1] - seq_off[i]));
        pg_adapter::apply_rc_flag(r, rc_flag[i]);
        r.ReadLength = (short)r.UnmatchedSeq.size();
        r.MatchedD = (char)strand[i];
    };
    std::vector<EventReadIn> in(n_reads);
    pg_adapter::parallel_ranges(n_reads, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) {
            EventReadIn &e = in[i];
            e.in_window = chr_id[i] == w->chr_id;
            if (!e.in_window) continue;
            SplitRead r;
            post_state((uint32_t)i, r);
            e.plus = strand[i] == '+';
            e.insert_size = insert_size[i];
            e.read_length = r.ReadLength;
            e.name_id = name_id ? name_id[i] : (uint32_t)i;
            if (cands) {
                e.var = cands + i * 2 * PG_VARIANT_CANDS;
                e.var_counts = counts + i * 2;
            }
            if (sv_cands) {
                e.sv = sv_cands + i * PG_SV_SLOTS;
                e.sv_counts = sv_counts + i * PG_SV_KINDS;
            }
        }
    });
    EventTables tabs;
    events_from_lists(ref, spacer, *w, in, [&](uint32_t i, const pg_variant_cand &c) {
        SplitRead r;
        post_state(i, r);
        for (uint64_t q = close_off[i]; q < close_off[i + 1]; q++) r.UP_Close.push_back(to_unique_point(close_pts[q]));
        for (uint64_t q = far_off[i]; q < far_off[i + 1]; q++) r.UP_Far.push_back(to_unique_point(far_pts[q]));
        VariantPair p;
        if (!variant_pair_from_cand(r, 1, c, p)) return std::string();
        return p.nt;
    }, tabs);
    if (n_reads) memcpy(out_reads, tabs.reads.data(), (size_t)n_reads * sizeof(pg_event_read));
    size_t m = 0, e = 0;
    for (int t = 0; t < PG_EVENT_TABLES; t++) {
        sizes->members[t] = tabs.members[t].size();
        sizes->events[t] = tabs.events[t].size();
        if (!tabs.members[t].empty()) memcpy(out_members + m, tabs.members[t].data(), tabs.members[t].size() * sizeof(uint32_t));
        if (!tabs.events[t].empty()) memcpy(out_events + e, tabs.events[t].data(), tabs.events[t].size() * sizeof(pg_event));
        m += tabs.members[t].size();
        e += tabs.events[t].size();
    }
    sizes->unresolved = tabs.unresolved;
    return 0;
}

/*
 * The event tables of DI, INV and INV_NT from the per-read records of an events build (pindel_pg.h "DI and inversion
 * event tables"), on the host: the plain-loop statement (pg_host_sv_events.hpp) the device entry pg_device_batch_sv_events is
 * compared with, byte for byte.  The reads and close points as pgh_events_from_lists takes them; recs: n_reads records of that
 * entry (or of the device's); sv_cands: the lists it was given; w: its window.  out_members / out_events: room for n_reads entries
 * each, filled table after table; sizes: what was filled.  -1: the window's chr_id lies outside the reference.
 */
int pgh_sv_events_from_lists(int32_t n_chr, const char *const *chr_seq, const uint64_t *chr_len, uint32_t spacer, uint32_t n_reads,
                             const uint8_t *seq, const uint64_t *seq_off, const uint8_t *strand, const uint8_t *rc_flag,
                             const uint64_t *close_off, const pg_point *close_pts, const pg_event_window *w, const pg_event_read *recs,
                             const pg_variant_cand *sv_cands, uint32_t *out_members, pg_event *out_events, pg_sv_event_sizes *sizes)
{
    if (!w || !sizes || w->chr_id < 0 || w->chr_id >= n_chr) {
        g_err = "pgh_sv_events_from_lists: the window's chr_id lies outside the reference";
        return -1;
    }
    if (n_reads && (!recs || !sv_cands)) {
        g_err = "pgh_sv_events_from_lists: null records or sv candidate array";
        return -1;
    }
    const std::string ref(chr_seq[w->chr_id], (size_t)chr_len[w->chr_id]);
    auto post_state = [&](uint32_t i, SplitRead &r) {
        r.UnmatchedSeq.assign((const char *)seq + seq_off[i], (size_t)(seq_off[i + 1] - seq_off[i]));
        pg_adapter::apply_rc_flag(r, rc_flag[i]);
        r.ReadLength = (short)r.UnmatchedSeq.size();
        r.MatchedD = (char)strand[i];
    };
    std::vector<SvEventReadIn> in(n_reads);
    pg_adapter::parallel_ranges(n_reads, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) {
            if (!(recs[i].flags & PG_EVR_BOXED)) continue;
            SplitRead r;
            post_state((uint32_t)i, r);
            SvEventReadIn &e = in[i];
            e.plus = strand[i] == '+';
            e.read_length = r.ReadLength;
            // LeftMostPos, Caller::note_close_mapped (a read without a close end is never boxed; its point counts as all zero)
            UniquePoint last;
            last.AbsLoc = 0;
            last.LengthStr = 0;
            if (close_off[i + 1] > close_off[i]) last = to_unique_point(close_pts[close_off[i + 1] - 1]);
            const short close_len = last.LengthStr;
            e.left_most = e.plus ? (int)(last.AbsLoc + 1 - close_len) : (int)(last.AbsLoc + close_len - r.getReadLength());
        }
    });
    SvEventTables tabs;
    auto cand_of = [&](size_t i, int kind, unsigned slot) -> const pg_variant_cand & {
        return sv_cands[i * PG_SV_SLOTS + sv_slot_base()[kind - PG_SV_DI] + slot];
    };
    sv_events_from_lists(ref, spacer, *w, in, recs, cand_of, [&](uint32_t i, const pg_variant_cand &c) {
        SplitRead r;
        post_state(i, r);
        return r.MatchedD == '+' ? sub(reverse_complement(r.UnmatchedSeq), c.bp + 1, (unsigned short)c.nt_rot)
                                 : sub(r.UnmatchedSeq, c.bp + 1, (unsigned short)c.nt_rot);
    }, tabs);
    size_t m = 0, e = 0;
    for (int t = 0; t < PG_SV_EVENT_TABLES; t++) {
        sizes->members[t] = tabs.members[t].size();
        sizes->events[t] = tabs.events[t].size();
        sizes->dropped_runs[t] = tabs.dropped_runs[t];
        if (!tabs.members[t].empty()) memcpy(out_members + m, tabs.members[t].data(), tabs.members[t].size() * sizeof(uint32_t));
        if (!tabs.events[t].empty()) memcpy(out_events + e, tabs.events[t].data(), tabs.events[t].size() * sizeof(pg_event));
        m += tabs.members[t].size();
        e += tabs.events[t].size();
    }
    return 0;
}

/*
 * Report records from tables, lists and points (pindel_pg.h "report records"), on the host: the plain-loop statement
 * (pg_host_report.hpp) the device entry pg_device_batch_report_reads is compared with, byte for byte.  strand, rc_flag and the
 * points as pgh_events_from_lists takes them; recs, ev_members / ev_sizes and sv_members / sv_sizes: the per-read records and the
 * member lists of the two table builds, back to back as they are downloaded; cands, sv_cands, sv_counts: the lists they were given.
 * out_records: room for every member of the seven lists; out_summaries: n_reads; sizes: what was filled.  -1: a null array.
 */
int pgh_report_reads_from_lists(uint32_t n_reads, const uint8_t *strand, const uint8_t *rc_flag, const uint64_t *close_off,
                                const pg_point *close_pts, const uint64_t *far_off, const pg_point *far_pts, const pg_event_read *recs,
                                const uint32_t *ev_members, const pg_event_sizes *ev_sizes, const uint32_t *sv_members,
                                const pg_sv_event_sizes *sv_sizes, const pg_variant_cand *cands, const pg_variant_cand *sv_cands,
                                const uint8_t *sv_counts, pg_report_read *out_records, pg_report_summary *out_summaries, pg_report_sizes *sizes)
{
    if (!ev_sizes || !sv_sizes || !sizes || (n_reads && (!strand || !rc_flag || !close_off || !far_off || !recs || !cands || !sv_cands || !sv_counts))) {
        g_err = "pgh_report_reads_from_lists: null array";
        return -1;
    }
    std::vector<UniquePoint> close(n_reads ? (size_t)close_off[n_reads] : 0), far(n_reads ? (size_t)far_off[n_reads] : 0);
    for (size_t q = 0; q < close.size(); q++) close[q] = to_unique_point(close_pts[q]);
    for (size_t q = 0; q < far.size(); q++) far[q] = to_unique_point(far_pts[q]);
    std::vector<ReportReadIn> in(n_reads);
    for (uint32_t i = 0; i < n_reads; i++) {
        ReportReadIn &r = in[i];
        r.plus = strand[i] == '+';
        r.rc_flag = rc_flag[i];
        r.close = close.data() + close_off[i];
        r.n_close = (size_t)(close_off[i + 1] - close_off[i]);
        r.far = far.data() + far_off[i];
        r.n_far = (size_t)(far_off[i + 1] - far_off[i]);
        r.var = cands + (size_t)i * 2 * PG_VARIANT_CANDS;
        r.sv = sv_cands + (size_t)i * PG_SV_SLOTS;
        r.sv_counts = sv_counts + (size_t)i * PG_SV_KINDS;
    }
    std::vector<uint32_t> evm[PG_EVENT_TABLES], svm[PG_SV_EVENT_TABLES];
    size_t m = 0;
    for (int t = 0; t < PG_EVENT_TABLES; t++) {
        if (ev_sizes->members[t]) evm[t].assign(ev_members + m, ev_members + m + ev_sizes->members[t]);
        m += ev_sizes->members[t];
    }
    m = 0;
    for (int t = 0; t < PG_SV_EVENT_TABLES; t++) {
        if (sv_sizes->members[t]) svm[t].assign(sv_members + m, sv_members + m + sv_sizes->members[t]);
        m += sv_sizes->members[t];
    }
    std::vector<pg_report_read> records;
    std::vector<pg_report_summary> summaries;
    report_reads_from_lists(in, recs, evm, svm, records, summaries);
    if (!records.empty()) memcpy(out_records, records.data(), records.size() * sizeof(pg_report_read));
    if (n_reads) memcpy(out_summaries, summaries.data(), (size_t)n_reads * sizeof(pg_report_summary));
    sizes->records = records.size();
    sizes->reads = n_reads;
    return 0;
}

/*
 * The long-insertion position tables (pindel_pg.h "long-insertion position tables"), on the host: the plain-loop
 * statement (li_tables_from_reads) the device entry pg_device_batch_li is compared with, byte for byte.  The reads as they were
 * handed to the search (seq, seq_off, strand, chr_id) with the rc flags; the post-state read length is taken from the read as rc_flag
 * applications of setUnmatchedSeq(ReverseComplement()) leave it.  close_off / close_pts: the expanded close points (the last one
 * counts); far_off: only whether the read has a far end.  recs: the events build's per-read records, win_chr its window's chr_id.
 * out_members, out_positions: room for n_reads entries each, both strands back to back; sizes: what was filled.  -1: a null array
 * or lo > hi.
 */
int pgh_li_tables_from_lists(uint32_t n_reads, const uint8_t *seq, const uint64_t *seq_off, const uint8_t *strand, const int32_t *chr_id,
                             const uint8_t *rc_flag, const uint64_t *close_off, const pg_point *close_pts, const uint64_t *far_off,
                             const pg_event_read *recs, int32_t win_chr, uint32_t lo, uint32_t hi, uint32_t *out_members,
                             pg_li_pos *out_positions, pg_li_sizes *sizes)
{
    if (!sizes || (n_reads && (!seq_off || !strand || !chr_id || !rc_flag || !close_off || !far_off || !recs || !out_members || !out_positions))) {
        g_err = "pgh_li_tables_from_lists: null array";
        return -1;
    }
    if (lo > hi) {
        g_err = "pgh_li_tables_from_lists: lo > hi";
        return -1;
    }
    std::vector<LiReadIn> in(n_reads);
    for (uint32_t i = 0; i < n_reads; i++) {
        LiReadIn &e = in[i];
        e.in_window = chr_id[i] == win_chr;
        e.has_close = close_off[i + 1] > close_off[i];
        e.has_far = far_off[i + 1] > far_off[i];
        e.strand = (char)strand[i];
        SplitRead r;
        r.UnmatchedSeq.assign((const char *)seq + seq_off[i], (size_t)(seq_off[i + 1] - seq_off[i]));
        pg_adapter::apply_rc_flag(r, rc_flag[i]);
        e.read_length = (int32_t)(short)r.UnmatchedSeq.size();
        if (e.has_close) {
            const UniquePoint last = to_unique_point(close_pts[close_off[i + 1] - 1]);
            e.close_abs = last.AbsLoc;
            e.close_len = last.LengthStr;
        }
    }
    LiTables t;
    li_tables_from_reads(in, recs, lo, hi, t);
    size_t m = 0, p = 0;
    for (int s = 0; s < 2; s++) {
        if (!t.members[s].empty()) memcpy(out_members + m, t.members[s].data(), t.members[s].size() * sizeof(uint32_t));
        if (!t.positions[s].empty()) memcpy(out_positions + p, t.positions[s].data(), t.positions[s].size() * sizeof(pg_li_pos));
        m += t.members[s].size();
        p += t.positions[s].size();
        sizes->members[s] = t.members[s].size();
        sizes->positions[s] = t.positions[s].size();
    }
    return 0;
}

/*
 * Test hook: the single consumer of the long-insertion tables (Caller::sort_output_li_tables) on tables made by hand.  One
 * chromosome chr_name / chr_seq (padded), a window [win_start, win_end) whose buffered window follows from max_insert_size as in
 * SortOutputLI, n_reads reads -- sequence, anchor strand and close length each; read i is named "r<i>", tagged "S", mapped at i --
 * and the tables over them (members / positions of both strands back to back, sizes).  marks: n_marks padded positions an earlier
 * report has marked.  Appends to <out_prefix>_LI.  -1: a table that points outside its arrays.
 */
int pgh_li_write_from_tables(const char *chr_name, const char *chr_seq, uint64_t chr_len, uint32_t spacer, uint32_t min_support,
                             uint32_t win_start, uint32_t win_end, int32_t max_insert_size, uint32_t n_reads, const uint8_t *seq,
                             const uint64_t *seq_off, const uint8_t *strand, const int16_t *close_len, const uint32_t *members,
                             const pg_li_pos *positions, const pg_li_sizes *sizes, const uint32_t *marks, uint32_t n_marks,
                             const char *out_prefix)
{
    if (!chr_name || !chr_seq || !sizes || !out_prefix || (n_reads && (!seq || !seq_off || !strand || !close_len))) {
        g_err = "pgh_li_write_from_tables: null array";
        return -1;
    }
    LiTables t;
    size_t m = 0, p = 0;
    for (int s = 0; s < 2; s++) {
        for (uint64_t k = 0; k < sizes->members[s]; k++) {
            if (members[m + k] >= n_reads) {
                g_err = "pgh_li_write_from_tables: a member outside the reads";
                return -1;
            }
            t.members[s].push_back(members[m + k]);
        }
        for (uint64_t k = 0; k < sizes->positions[s]; k++) {
            const pg_li_pos &q = positions[p + k];
            if ((uint64_t)q.first + q.n_reads > sizes->members[s]) {
                g_err = "pgh_li_write_from_tables: a position outside its member list";
                return -1;
            }
            t.positions[s].push_back(q);
        }
        m += sizes->members[s];
        p += sizes->positions[s];
    }
    std::vector<Chromosome> genome(1);
    genome[0].name = chr_name;
    genome[0].seq.assign(chr_seq, (size_t)chr_len);
    Settings S;
    S.spacer = spacer;
    S.NumRead2ReportCutOff = min_support;
    S.Analyze_LI = true;
    Caller caller(S, &genome, out_prefix, false);
    caller.note_insert_size(max_insert_size);
    std::vector<SplitRead> reads(n_reads);
    std::vector<pg_report_summary> summaries(n_reads);
    for (uint32_t i = 0; i < n_reads; i++) {
        SplitRead &r = reads[i];
        r.Name = "r" + std::to_string(i);
        r.UnmatchedSeq.assign((const char *)seq + seq_off[i], (size_t)(seq_off[i + 1] - seq_off[i]));
        r.ReadLength = (short)r.UnmatchedSeq.size();
        r.MatchedD = (char)strand[i];
        r.MatchedRelPos = i;
        r.MS = 60;
        r.InsertSize = (short)max_insert_size;
        r.Tag = "S";
        r.FragName = chr_name;
        r.chr_id = 0;
        pg_report_summary &s = summaries[i];
        memset(&s, 0, sizeof s);
        s.close_len = close_len[i];
        s.flags = PG_RS_CLOSE;
    }
    caller.apply_summaries(reads, summaries.data(), false);
    caller.begin_region();
    caller.set_marks_for_test(genome[0], marks, n_marks);
    caller.write_li_from_tables(genome[0], reads, win_start, win_end, t, summaries.data());
    return 0;
}

/*
 * The interchromosomal junction tables (pindel_pg.h "interchromosomal junction tables"), on the host: the plain-loop
 * statement (int_tables_from_reads) the device entry pg_device_batch_int is compared with, byte for byte.  The reads as they were
 * handed to the search (seq, seq_off, strand, chr_id) with the rc flags; the post-state read length is taken from the read as rc_flag
 * applications of setUnmatchedSeq(ReverseComplement()) leave it.  The expanded points of both ends (CSR); chr_rank: n_chr ranks.
 * out_members, out_calls: room for n_reads entries each; sizes: what was filled.  -1: a null array.
 */
int pgh_int_tables_from_lists(uint32_t n_reads, const uint8_t *seq, const uint64_t *seq_off, const uint8_t *strand, const int32_t *chr_id,
                              const uint8_t *rc_flag, const uint64_t *close_off, const pg_point *close_pts, const uint64_t *far_off,
                              const pg_point *far_pts, const int32_t *chr_rank, uint32_t n_chr, uint32_t *out_members, pg_int_call *out_calls,
                              pg_int_sizes *sizes)
{
    if (!sizes || (n_chr && !chr_rank) ||
        (n_reads && (!seq_off || !strand || !chr_id || !rc_flag || !close_off || !far_off || !out_members || !out_calls))) {
        g_err = "pgh_int_tables_from_lists: null array";
        return -1;
    }
    std::vector<UniquePoint> close(n_reads ? (size_t)close_off[n_reads] : 0), far(n_reads ? (size_t)far_off[n_reads] : 0);
    for (size_t q = 0; q < close.size(); q++) close[q] = to_unique_point(close_pts[q]);
    for (size_t q = 0; q < far.size(); q++) far[q] = to_unique_point(far_pts[q]);
    std::vector<IntReadIn> in(n_reads);
    for (uint32_t i = 0; i < n_reads; i++) {
        IntReadIn &e = in[i];
        e.chr = chr_id[i];
        e.strand = (char)strand[i];
        SplitRead r;
        r.UnmatchedSeq.assign((const char *)seq + seq_off[i], (size_t)(seq_off[i + 1] - seq_off[i]));
        pg_adapter::apply_rc_flag(r, rc_flag[i]);
        e.read_length = (int32_t)(short)r.UnmatchedSeq.size();
        e.close = close.data() + close_off[i];
        e.n_close = (size_t)(close_off[i + 1] - close_off[i]);
        e.far = far.data() + far_off[i];
        e.n_far = (size_t)(far_off[i + 1] - far_off[i]);
        if (e.n_far) {
            e.far_chr = e.far[0].chr;
            e.far_minus = e.far[0].Strand == '-';
        }
    }
    IntTables t;
    int_tables_from_reads(in, chr_rank, n_chr, t);
    if (!t.members.empty()) memcpy(out_members, t.members.data(), t.members.size() * sizeof(uint32_t));
    if (!t.calls.empty()) memcpy(out_calls, t.calls.data(), t.calls.size() * sizeof(pg_int_call));
    sizes->members = t.members.size();
    sizes->calls = t.calls.size();
    return 0;
}

/*
 * Test hook: the single consumer of the junction tables (Caller::report_interchr_tables) on tables made by hand.  n_reads reads --
 * name, chromosome name, far chromosome name (NUL-terminated strings each) and sequence as rc_flag left it -- the ascending indices
 * of the junction reads among them, and the tables over them.  repairs: REPAIR_* bits (int-pairs).  Appends to <out_prefix>_INT.
 * -1: a table or a junction index that points outside its arrays.
 */
int pgh_int_write_from_tables(uint32_t spacer, uint32_t repairs, uint32_t n_reads, const char *const *names, const char *const *chr_names,
                              const char *const *far_names, const uint8_t *seq, const uint64_t *seq_off, const uint32_t *junction,
                              uint32_t n_junction, const uint32_t *members, const pg_int_call *calls, const pg_int_sizes *sizes,
                              const char *out_prefix)
{
    if (!sizes || !out_prefix || (n_reads && (!names || !chr_names || !far_names || !seq_off)) || (n_junction && !junction) ||
        (sizes->members && !members) || (sizes->calls && !calls)) {
        g_err = "pgh_int_write_from_tables: null array";
        return -1;
    }
    IntTables t;
    for (uint64_t k = 0; k < sizes->members; k++) {
        if (members[k] >= n_reads) {
            g_err = "pgh_int_write_from_tables: a member outside the reads";
            return -1;
        }
        t.members.push_back(members[k]);
    }
    for (uint64_t k = 0; k < sizes->calls; k++) {
        if ((uint64_t)calls[k].first + calls[k].n_reads > sizes->members) {
            g_err = "pgh_int_write_from_tables: a call outside the member list";
            return -1;
        }
        t.calls.push_back(calls[k]);
    }
    std::vector<uint32_t> junc(junction, junction + n_junction);
    for (size_t k = 0; k < junc.size(); k++)
        if (junc[k] >= n_reads || (k && junc[k] <= junc[k - 1])) {
            g_err = "pgh_int_write_from_tables: the junction reads are ascending indices of the reads";
            return -1;
        }
    Settings S;
    S.spacer = spacer;
    S.report_interchromosomal = true;
    S.repairs = repairs;
    Caller caller(S, nullptr, out_prefix, false);
    std::vector<SplitRead> reads(n_reads);
    for (uint32_t i = 0; i < n_reads; i++) {
        SplitRead &r = reads[i];
        r.Name = names[i];
        r.FragName = chr_names[i];
        r.FarFragName = far_names[i];
        r.UnmatchedSeq.assign((const char *)seq + seq_off[i], (size_t)(seq_off[i + 1] - seq_off[i]));
        r.ReadLength = (short)r.UnmatchedSeq.size();
    }
    caller.report_interchr_tables(reads, junc, t);
    return 0;
}

/* Numbers names by first occurrence: id[i] = the index of the first name equal to names[i] among the distinct ones (the name_id
 * array of the events entries).  names: n NUL-terminated strings. */
void pgh_name_ids(uint32_t n, const char *const *names, uint32_t *id)
{
    std::unordered_map<std::string, uint32_t> seen;
    seen.reserve((size_t)n * 2);
    for (uint32_t i = 0; i < n; i++) id[i] = seen.emplace(names[i], (uint32_t)seen.size()).first->second;
}

/* "int-pairs,depth-mapq" / "all" -> the bits of pgh_settings.repairs; -1 = an unknown name or an empty list (pgh_last_error) */
int64_t pgh_parse_repairs(const char *list)
{
    uint32_t mask = 0;
    if (!parse_repairs(str_or_empty(list), mask, g_err)) return -1;
    return (int64_t)mask;
}

/*
 * Average read depth of [beg, end) (0-based) of chromosome chr_name in one BAM, as the reference's bam2depth counts it
 * (pg_depth.hpp): 0 when the BAM's header lacks the chromosome, NaN for an empty region.  0 = done, -1 = the file
 * cannot be read (pgh_last_error).
 */
int pgh_region_depth_mapq(const char *bam_path, const char *chr_name, int64_t beg, int64_t end, uint32_t min_mapq, double *avg);
int pgh_region_depth(const char *bam_path, const char *chr_name, int64_t beg, int64_t end, double *avg)
{
    return pgh_region_depth_mapq(bam_path, chr_name, beg, end, 0, avg);
}

/* ... counting only the records with MAPQ >= min_mapq (0: every record, as the reference does; 20: --repair depth-mapq) */
int pgh_region_depth_mapq(const char *bam_path, const char *chr_name, int64_t beg, int64_t end, uint32_t min_mapq, double *avg)
{
    BamFile bam;
    if (!bam.open(bam_path, g_err)) return -1;
    DepthSums d;
    d.add(beg, end);
    if (!depth_sums(bam, chr_name, d, min_mapq)) {
        g_err = std::string(bam_path) + ": BAM read failed";
        return -1;
    }
    *avg = d.avg(0);
    return 0;
}

/*
 * getRelativeCoverageInternal: per BAM the depth of the event [start, end) against its two flanks of the same length,
 * clipped to [0, chr_size): 2 * (2 * sv) / (before + after), -1 when before + after == 0, NaN when a flank has no length.
 */
int pgh_depth_ratio_mapq(int32_t n_bams, const char *const *bam_paths, const char *chr_name, int64_t chr_size, int64_t start,
                         int64_t end, uint32_t min_mapq, double *ratio);
int pgh_depth_ratio(int32_t n_bams, const char *const *bam_paths, const char *chr_name, int64_t chr_size, int64_t start, int64_t end,
                    double *ratio)
{
    return pgh_depth_ratio_mapq(n_bams, bam_paths, chr_name, chr_size, start, end, 0, ratio);
}

/* ... counting only the records with MAPQ >= min_mapq */
int pgh_depth_ratio_mapq(int32_t n_bams, const char *const *bam_paths, const char *chr_name, int64_t chr_size, int64_t start,
                         int64_t end, uint32_t min_mapq, double *ratio)
{
    for (int32_t k = 0; k < n_bams; k++) {
        BamFile bam;
        if (!bam.open(bam_paths[k], g_err)) return -1;
        if (!depth_ratio(bam, chr_name, chr_size, start, end, ratio[k], min_mapq)) {
            g_err = std::string(bam_paths[k]) + ": BAM read failed";
            return -1;
        }
    }
    return 0;
}

/* IsGoodTD's rule on the ratios of the measured BAMs (reporter.cpp:1141-1152): 1 = the event is kept */
int pgh_depth_rule_td(int32_t n, const double *ratio) { return depth_rule_td(ratio, n > 0 ? (size_t)n : 0) ? 1 : 0; }

/*
 * The region plan of -c region -j include_bed -J exclude_bed (any may be NULL or "") on the reference fasta_path (its
 * .fai sizes when present): 3 values per record (chromosome index in the FASTA, start, end), in plan order.  Returns the
 * number of records (also when it exceeds cap; only cap are written), -1 = unreadable input, unknown chromosome, start
 * beyond the chromosome or a malformed BED line, -2 = -c syntax (pgh_last_error says which).
 */
int64_t pgh_region_plan_bed(const char *fasta_path, const char *region, const char *include_bed, const char *exclude_bed,
                            int32_t bed_zero_based, uint32_t *out, uint64_t cap);
int64_t pgh_region_plan(const char *fasta_path, const char *region, const char *include_bed, const char *exclude_bed,
                        uint32_t *out, uint64_t cap)
{
    return pgh_region_plan_bed(fasta_path, region, include_bed, exclude_bed, 0, out, cap);
}

/* ... with bed_zero_based != 0 the records of both BED files are 0-based and half-open (--repair bed0) */
int64_t pgh_region_plan_bed(const char *fasta_path, const char *region, const char *include_bed, const char *exclude_bed,
                            int32_t bed_zero_based, uint32_t *out, uint64_t cap)
{
    std::vector<Chromosome> genome;
    if (load_fasta(fasta_path, genome, 0, g_err)) return -1;
    std::vector<RegionRecord> plan;
    const int rc = region_plan(chromosome_names(genome), chromosome_sizes(genome, read_fai(fasta_path, genome), 0), str_or_empty(region),
                               str_or_empty(include_bed), str_or_empty(exclude_bed), plan, g_err, bed_zero_based != 0);
    if (rc) return rc == REGION_BAD_SYNTAX ? -2 : -1;
    for (size_t k = 0; k < plan.size() && k < cap; k++) {
        out[3 * k] = (uint32_t)plan[k].chr;
        out[3 * k + 1] = plan[k].start;
        out[3 * k + 2] = plan[k].end;
    }
    return (int64_t)plan.size();
}

/* pindel2vcf's flags (pg_vcf.hpp VcfOptions); pgh_vcf_default_options fills in the reference's defaults. */
struct pgh_vcf_options {
    const char *reference;       /* -r */
    const char *reference_name;  /* -R */
    const char *reference_date;  /* -d */
    const char *report;          /* -p: NULL or "" = none */
    const char *prefix;          /* -P: NULL or "" = none */
    const char *vcf;             /* -v: NULL or "" = <report>.vcf / <prefix>.vcf */
    const char *chromosome;      /* -c: NULL or "" = all */
    int32_t window_size, min_coverage;
    double het_cutoff, hom_cutoff;
    int32_t min_size, max_size, both_strands, min_supporting_samples, min_supporting_reads, max_supporting_reads;
    int32_t region_start, region_end, max_internal_repeats, max_internal_repeatlength, max_postindel_repeats;
    int32_t max_postindel_repeatlength, compact_output_limit, only_balanced_samples, minimum_strand_support, gatk_compatible;
};

void pgh_vcf_default_options(pgh_vcf_options *o)
{
    const VcfOptions d;
    *o = pgh_vcf_options{};
    o->window_size = d.window_size;
    o->min_coverage = d.min_coverage;
    o->het_cutoff = d.het_cutoff;
    o->hom_cutoff = d.hom_cutoff;
    o->min_size = d.min_size;
    o->max_size = d.max_size;
    o->both_strands = d.both_strands;
    o->min_supporting_samples = d.min_supporting_samples;
    o->min_supporting_reads = d.min_supporting_reads;
    o->max_supporting_reads = d.max_supporting_reads;
    o->region_start = d.region_start;
    o->region_end = d.region_end;
    o->max_internal_repeats = d.max_internal_repeats;
    o->max_internal_repeatlength = d.max_internal_repeatlength;
    o->max_postindel_repeats = d.max_postindel_repeats;
    o->max_postindel_repeatlength = d.max_postindel_repeatlength;
    o->compact_output_limit = d.compact_output_limit;
    o->only_balanced_samples = d.only_balanced_samples;
    o->minimum_strand_support = d.minimum_strand_support;
    o->gatk_compatible = d.gatk_compatible;
}

/* Pindel reports -> VCF (pg_vcf.hpp).  0 = written, 1 = error (pgh_last_error says which; no output file is left). */
int pgh_reports_to_vcf(const pgh_vcf_options *o)
{
    VcfOptions v;
    v.reference = str_or_empty(o->reference);
    v.reference_name = str_or_empty(o->reference_name);
    v.reference_date = str_or_empty(o->reference_date);
    v.report = str_or_empty(o->report);
    v.prefix = str_or_empty(o->prefix);
    v.vcf = str_or_empty(o->vcf);
    v.chromosome = str_or_empty(o->chromosome);
    v.window_size = o->window_size;
    v.min_coverage = o->min_coverage;
    v.het_cutoff = o->het_cutoff;
    v.hom_cutoff = o->hom_cutoff;
    v.min_size = o->min_size;
    v.max_size = o->max_size;
    v.both_strands = o->both_strands != 0;
    v.min_supporting_samples = o->min_supporting_samples;
    v.min_supporting_reads = o->min_supporting_reads;
    v.max_supporting_reads = o->max_supporting_reads;
    v.region_start = o->region_start;
    v.region_end = o->region_end;
    v.max_internal_repeats = o->max_internal_repeats;
    v.max_internal_repeatlength = o->max_internal_repeatlength;
    v.max_postindel_repeats = o->max_postindel_repeats;
    v.max_postindel_repeatlength = o->max_postindel_repeatlength;
    v.compact_output_limit = o->compact_output_limit;
    v.only_balanced_samples = o->only_balanced_samples != 0;
    v.minimum_strand_support = o->minimum_strand_support;
    v.gatk_compatible = o->gatk_compatible != 0;
    return reports_to_vcf(v, g_err) ? 1 : 0;
}

// The clusters of the n_q query positions q (hint_windows, pg_bdhints.hpp) into the caller's arrays: out_off has n_q + 1
// entries, out_win 3 ints (chr id, start, end) per window.  false: out_win (room for cap windows) is too small.
static bool pack_hint_windows(const pgh::BDHints &h, uint32_t n_q, const uint32_t *q, uint64_t *out_off, int32_t *out_win, uint64_t cap)
{
    const pgh::HintWindows hw = pgh::hint_windows(h, n_q, [&](size_t i) { return q[i]; });
    if (hw.win.size() > cap) return false;
    std::copy(hw.off.begin(), hw.off.end(), out_off);
    for (size_t k = 0; k < hw.win.size(); k++) {
        out_win[3 * k] = hw.win[k].chr_id;
        out_win[3 * k + 1] = (int32_t)hw.win[k].start;
        out_win[3 * k + 2] = (int32_t)hw.win[k].end;
    }
    return true;
}

// BreakDancer hints (pg_bdhints.hpp) for one bin: clusters of the reads whose last close-end point is at
// q[i].  out_off has n_q + 1 entries, out_win 3 ints (chr id, start, end) per window; returns the status
// of load_file (0 / 1 = ignored), -1 = cannot open, -2 = unknown chromosome, -3 = out_win too small.
int pgh_bd_query(const char *path, uint32_t spacer, int32_t n_chr, const char *const *names, int32_t chr_id,
                 uint32_t start, uint32_t end, uint32_t n_q, const uint32_t *q, uint64_t *out_off,
                 int32_t *out_win, uint64_t cap, uint64_t *n_events)
{
    pgh::BDHints h;
    std::string note;
    const int rc = h.load_file(path, spacer, note);
    if (n_events) *n_events = h.n_events();
    g_err = note;
    if (rc < 0) return -1;
    std::vector<std::string> nm(names, names + n_chr);
    if (!h.load_region(nm, chr_id, start, end, g_err)) return -2;
    return pack_hint_windows(h, n_q, q, out_off, out_win, cap) ? rc : -3;
}

// The same region as a position-keyed table (BDHints::table, pg_hint_table of pindel_pg.h) into the caller's arrays: run_first
// (room for cap_runs + 1), run_cluster (cap_runs), cluster_off (cap_clusters + 1), out_win 3 ints (chr id, start, end) per window
// (cap_win windows); counts[0 .. 2] = runs, clusters, windows -- filled in whatever the capacities, so that a caller may ask with
// capacities of 0 first.  Returns as pgh_bd_query; -3 = an array is too small (nothing but counts was written).
int pgh_bd_table(const char *path, uint32_t spacer, int32_t n_chr, const char *const *names, int32_t chr_id, uint32_t start,
                 uint32_t end, uint32_t *run_first, uint32_t *run_cluster, uint64_t cap_runs, uint64_t *cluster_off,
                 uint64_t cap_clusters, int32_t *out_win, uint64_t cap_win, uint64_t *counts, uint64_t *n_events)
{
    pgh::BDHints h;
    std::string note;
    const int rc = h.load_file(path, spacer, note);
    if (n_events) *n_events = h.n_events();
    g_err = note;
    if (rc < 0) return -1;
    std::vector<std::string> nm(names, names + n_chr);
    if (!h.load_region(nm, chr_id, start, end, g_err)) return -2;
    const pgh::BDHints::Table t = h.table();
    const uint64_t n_clusters = t.cluster_off.empty() ? 0 : t.cluster_off.size() - 1;
    if (counts) {
        counts[0] = t.run_cluster.size();
        counts[1] = n_clusters;
        counts[2] = t.win.size();
    }
    if (t.run_cluster.size() > cap_runs || n_clusters > cap_clusters || t.win.size() > cap_win) return -3;
    std::copy(t.run_first.begin(), t.run_first.end(), run_first);
    std::copy(t.run_cluster.begin(), t.run_cluster.end(), run_cluster);
    std::copy(t.cluster_off.begin(), t.cluster_off.end(), cluster_off);
    for (size_t k = 0; k < t.win.size(); k++) {
        out_win[3 * k] = t.win[k].chr_id;
        out_win[3 * k + 1] = (int32_t)t.win[k].start;
        out_win[3 * k + 2] = (int32_t)t.win[k].end;
    }
    return rc;
}

// BAM ingest (pg_bam.hpp): the split-read candidates of one window of one BAM file as the SoA batch of the C ABI.
// Returns a handle (pgh_bam_ingest_free) or null (pgh_last_error).
void *pgh_bam_ingest(const char *bam_path, const char *chr_name, int32_t chr_id, uint64_t chr_padded_size, int64_t win_start,
                     int64_t win_end, int32_t insert_size, const char *tag, uint32_t min_anchor_quality, uint32_t spacer,
                     int32_t use_index, uint64_t *n_reads, uint64_t *n_bases)
{
    pgh::BamFile bam;
    if (!bam.open(bam_path, g_err, use_index != 0)) return nullptr;
    pgh::BamIngestSettings st;
    st.min_anchor_quality = min_anchor_quality;
    st.spacer = spacer;
    pgh::BamIngest ing(st);
    pgh::IngestedReads *out = new pgh::IngestedReads();
    out->clear();
    if (!ing.read_window(bam, chr_name, chr_id, chr_padded_size, win_start, win_end, insert_size, tag ? tag : "", *out)) {
        g_err = ing.error;
        delete out;
        return nullptr;
    }
    if (n_reads) *n_reads = out->size();
    if (n_bases) *n_bases = out->batch.seq.size();
    return out;
}

int pgh_bam_ingest_view(void *h, const uint8_t **seq, const uint64_t **off, const uint8_t **strand, const int32_t **pos,
                        const int16_t **isz, const int32_t **chr, const int16_t **ms)
{
    if (!h) return -1;
    pgh::IngestedReads *r = (pgh::IngestedReads *)h;
    *seq = r->batch.seq.data();
    *off = r->batch.off.data();
    *strand = r->batch.strand.data();
    *pos = r->batch.pos.data();
    *isz = r->batch.isz.data();
    *chr = r->batch.chr.data();
    *ms = r->ms.data();
    return 0;
}

const char *pgh_bam_ingest_name(void *h, uint64_t i)
{
    pgh::IngestedReads *r = (pgh::IngestedReads *)h;
    return (r && i < r->names.size()) ? r->names[i].c_str() : nullptr;
}

// the reference-supporting reads of the window (isRefRead / build_record_RefRead): 3 values each (pos, length, tag index)
uint64_t pgh_bam_ingest_ref_reads(void *h, uint32_t *out, uint64_t cap)
{
    pgh::IngestedReads *r = (pgh::IngestedReads *)h;
    if (!r) return 0;
    for (size_t i = 0; i < r->ref_reads.size() && i < cap; i++) {
        out[3 * i] = r->ref_reads[i].pos;
        out[3 * i + 1] = r->ref_reads[i].length;
        out[3 * i + 2] = r->ref_reads[i].tag;
    }
    return r->ref_reads.size();
}

void pgh_bam_ingest_free(void *h) { delete (pgh::IngestedReads *)h; }

// What the BAI reader makes of an index file (test hook: the reference ships .bai files of its demo BAMs): per
// reference 4 values -- bins (without the pseudo-bin), chunks, 64-bit sum of all chunk begin/end offsets, linear-index
// entries; returns the number of references or -1.
int32_t pgh_bai_summary(const char *bai_path, uint64_t *out, uint32_t cap_refs)
{
    FILE *f = fopen(bai_path, "rb");
    if (!f) return -1;
    pgh::BamFile::BaiBins bins;
    std::vector<std::vector<uint64_t>> linear;
    const bool ok = pgh::BamFile::read_bai(f, bins, linear);
    fclose(f);
    if (!ok) return -1;
    for (size_t t = 0; t < bins.size() && t < cap_refs; t++) {
        uint64_t chunks = 0, sum = 0;
        for (const auto &kv : bins[t])
            for (const auto &c : kv.second) {
                chunks++;
                sum += c.first + c.second;
            }
        for (uint64_t v : linear[t]) sum += v;
        out[4 * t] = bins[t].size();
        out[4 * t + 1] = chunks;
        out[4 * t + 2] = sum;
        out[4 * t + 3] = linear[t].size();
    }
    return (int32_t)bins.size();
}

// Read-pair discovery (pg_rp.hpp) on one window of one BAM: its BreakDancer-like events, with the interchromosomal pairs'
// events after the same-chromosome ones when interchr is set (what -I adds).  rp_path (nullable): the lines of <prefix>_RP.
// names (nullable) receives the chromosome names of the BAM header.  false: a file error (g_err).
static bool window_rp_events(const char *bam_path, const char *chr_name, int64_t win_start, int64_t win_end, int32_t insert_size,
                             const char *tag, uint32_t min_anchor_quality, uint32_t spacer, bool interchr, const char *rp_path,
                             std::vector<pgh::RpEvent> &ev, std::vector<std::string> *names = nullptr)
{
    pgh::BamFile bam;
    if (!bam.open(bam_path, g_err)) return false;
    std::vector<pgh::RpRead> rp, rp_inter;
    if (!pgh::rp_discover(bam, chr_name, win_start, win_end, insert_size, tag ? tag : "", min_anchor_quality, rp, interchr ? &rp_inter : nullptr))
        return false;
    std::ofstream f;
    if (rp_path) f.open(rp_path, std::ios::trunc);
    ev = pgh::rp_events(rp, spacer, rp_path ? &f : nullptr);
    if (interchr) {
        const std::vector<pgh::RpEvent> inter = pgh::rp_events_interchr(rp_inter, spacer, rp_path ? &f : nullptr);
        ev.insert(ev.end(), inter.begin(), inter.end());
    }
    if (names) *names = bam.header().names;
    return true;
}

// The same-chromosome events of one window of one BAM: out receives 4 values per event (pos1, pos1b, pos2, pos2b, Pindel
// coordinates).  Returns the number of events, -1 on a file error.
int64_t pgh_rp_events(const char *bam_path, const char *chr_name, int64_t win_start, int64_t win_end, int32_t insert_size,
                      const char *tag, uint32_t min_anchor_quality, uint32_t spacer, const char *rp_path, uint32_t *out, uint64_t cap)
{
    std::vector<pgh::RpEvent> ev;
    if (!window_rp_events(bam_path, chr_name, win_start, win_end, insert_size, tag, min_anchor_quality, spacer, false, rp_path, ev)) return -1;
    for (size_t i = 0; i < ev.size() && i < cap; i++) {
        out[4 * i] = ev[i].pos1;
        out[4 * i + 1] = ev[i].pos1b;
        out[4 * i + 2] = ev[i].pos2;
        out[4 * i + 3] = ev[i].pos2b;
    }
    return (int64_t)ev.size();
}

// The events of `ev` as 6 values each: chromosome index of the first side (in `names`; -1 = unknown), pos1, pos1b, then the same for
// the second side
static void events_with_chromosomes(const std::vector<pgh::RpEvent> &ev, const std::vector<std::string> &names, int64_t *out, uint64_t cap)
{
    auto id_of = [&](const std::string &n) {
        for (size_t c = 0; c < names.size(); c++)
            if (names[c] == n) return (int64_t)c;
        return (int64_t)-1;
    };
    for (size_t i = 0; i < ev.size() && i < cap; i++) {
        const int64_t v[6] = { id_of(ev[i].chr1), ev[i].pos1, ev[i].pos1b, id_of(ev[i].chr2), ev[i].pos2, ev[i].pos2b };
        for (int k = 0; k < 6; k++) out[6 * i + k] = v[k];
    }
}

// pgh_rp_events with the interchromosomal pairs of the window (interchr != 0: what -I adds; their events and _RP lines follow the
// same-chromosome ones) and with the chromosomes of both sides: out receives 6 values per event (events_with_chromosomes; the
// chromosome index is the one of the BAM header).  Returns the number of events, -1 on a file error.
int64_t pgh_rp_events_chr(const char *bam_path, const char *chr_name, int64_t win_start, int64_t win_end, int32_t insert_size,
                          const char *tag, uint32_t min_anchor_quality, uint32_t spacer, int32_t interchr, const char *rp_path, int64_t *out,
                          uint64_t cap)
{
    std::vector<pgh::RpEvent> ev;
    std::vector<std::string> names;
    if (!window_rp_events(bam_path, chr_name, win_start, win_end, insert_size, tag, min_anchor_quality, spacer, interchr != 0, rp_path, ev, &names))
        return -1;
    events_with_chromosomes(ev, names, out, cap);
    return (int64_t)ev.size();
}

// The interchromosomal clustering alone (rp_events_interchr) on pairs given as arrays, as build_record_RP_Discovery would have left
// them: chromosome indices (into names) and strands ('+' / '-') of both sides, positions, insert size, read length, sample tag index
// (into tags).  out / rp_path as for pgh_rp_events_chr; seconds (nullable) receives the time of the clustering.
int64_t pgh_rp_interchr_pairs(uint32_t n, const int32_t *chr_a, const int32_t *chr_b, const uint8_t *d_a, const uint8_t *d_b,
                              const uint32_t *pos_a, const uint32_t *pos_b, const int32_t *insert_size, const int16_t *read_length,
                              const int32_t *tag, int32_t n_names, const char *const *names, int32_t n_tags, const char *const *tags,
                              uint32_t spacer, const char *rp_path, int64_t *out, uint64_t cap, double *seconds)
{
    std::vector<std::string> nm(names, names + n_names), tg(tags, tags + n_tags);
    std::vector<pgh::RpRead> rp(n);
    for (uint32_t i = 0; i < n; i++) {
        pgh::RpRead &t = rp[i];
        if (chr_a[i] < 0 || chr_a[i] >= n_names || chr_b[i] < 0 || chr_b[i] >= n_names || tag[i] < 0 || tag[i] >= n_tags) {
            g_err = "pgh_rp_interchr_pairs: index out of range";
            return -1;
        }
        t.ChrA = chr_a[i];
        t.ChrB = chr_b[i];
        t.ChrNameA = nm[(size_t)chr_a[i]];
        t.ChrNameB = nm[(size_t)chr_b[i]];
        t.DA = (char)d_a[i];
        t.DB = (char)d_b[i];
        t.PosA = t.OriginalPosA = pos_a[i];
        t.PosB = t.OriginalPosB = pos_b[i];
        t.InsertSize = insert_size[i];
        t.ReadLength = read_length[i];
        t.Tags.push_back(tg[(size_t)tag[i]]);
    }
    std::ofstream f;
    if (rp_path) f.open(rp_path, std::ios::trunc);
    const auto t0 = std::chrono::steady_clock::now();
    const std::vector<pgh::RpEvent> ev = pgh::rp_events_interchr(rp, spacer, rp_path ? &f : nullptr);
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    events_with_chromosomes(ev, nm, out, cap);
    return (int64_t)ev.size();
}

// The window hints of one bin exactly as `pindel_pg -i ... [-b file]` with -R hands them to the far end
// (run_bam_pipeline): events of the -b file (bd_path may be null / empty) + the read-pair events of this window of
// this BAM (UpdateBD; [win_start, win_end) = the window as clipped to the chromosome), loadRegion for the bin
// [win_start, region_end) (the unclipped bin, as main() hands it over), then the cluster of every query position
// (= last close-end AbsLoc).
// out_off: n_q + 1 entries, out_win: 3 ints (chr id, start, end) per window.  Returns the number of read-pair
// events, -1 on a file error, -2 unknown chromosome, -3 out_win too small.
// interchr != 0: with -I's interchromosomal pairs (UpdateBD hands both kinds to the event list).  ev_out (nullable) receives the
// read-pair events themselves, 6 values per event (events_with_chromosomes, indices into names).
int64_t pgh_window_hints_chr(const char *bd_path, const char *bam_path, int32_t n_chr, const char *const *names, int32_t chr_id,
                             int64_t win_start, int64_t win_end, int64_t region_end, int32_t insert_size, const char *tag,
                             uint32_t min_anchor_quality, uint32_t spacer, int32_t interchr, uint32_t n_q, const uint32_t *q, uint64_t *out_off,
                             int32_t *out_win, uint64_t cap, int64_t *ev_out, uint64_t ev_cap)
{
    pgh::BDHints h;
    std::string note;
    if (bd_path && bd_path[0] && h.load_file(bd_path, spacer, note) < 0) {
        g_err = note;
        return -1;
    }
    std::vector<std::string> nm(names, names + n_chr);
    std::vector<pgh::RpEvent> ev;
    if (!window_rp_events(bam_path, nm[chr_id].c_str(), win_start, win_end, insert_size, tag, min_anchor_quality, spacer, interchr != 0, nullptr, ev))
        return -1;
    if (ev_out) events_with_chromosomes(ev, nm, ev_out, ev_cap);
    h.update_with_rp(rp_sides(ev));
    if (!h.load_region(nm, chr_id, (unsigned)win_start + spacer, (unsigned)region_end + spacer, g_err)) return -2;
    return pack_hint_windows(h, n_q, q, out_off, out_win, cap) ? (int64_t)ev.size() : -3;
}

// ... for the same-chromosome pairs alone, without the events
int64_t pgh_window_hints(const char *bd_path, const char *bam_path, int32_t n_chr, const char *const *names, int32_t chr_id,
                         int64_t win_start, int64_t win_end, int64_t region_end, int32_t insert_size, const char *tag,
                         uint32_t min_anchor_quality, uint32_t spacer, uint32_t n_q, const uint32_t *q, uint64_t *out_off, int32_t *out_win, uint64_t cap)
{
    return pgh_window_hints_chr(bd_path, bam_path, n_chr, names, chr_id, win_start, win_end, region_end, insert_size, tag, min_anchor_quality,
                                spacer, 0, n_q, q, out_off, out_win, cap, NULL, 0);
}

// MergeInterChr alone: the _INT_final text of an _INT file (write_int_final, pg_host_int.cpp)
int pgh_int_final(const char *int_path, const char *final_path)
{
    pgh::write_int_final(int_path, final_path);
    return 0;
}

// Test hook (tests/test_cpu_suite.py): sorts indices 0..n-1 by keys[] with the reference's O(n^2)
// exchange sort and with its fast equivalent; the two outputs must be identical.
void pgh_test_exchange_sort(const int32_t *keys, uint32_t n, uint32_t *out_reference, uint32_t *out_fast)
{
    std::vector<unsigned> a(n), b(n);
    for (uint32_t i = 0; i < n; i++) a[i] = b[i] = i;
    auto less = [&](unsigned x, unsigned y) { return keys[x] < keys[y]; };
    pgh::detail::exchange_sort_reference(a, less);
    pgh::detail::exchange_sort_fast(b, less);
    for (uint32_t i = 0; i < n; i++) {
        out_reference[i] = a[i];
        out_fast[i] = b[i];
    }
}

// -q's containment test on the host (src/search_MEI_util.cpp:188-351): out[i] = contains_subseq_any_strand(query_i, db_i, 15) with
// query_i = q[q_off[i] .. q_off[i+1]), db_i = db[db_off[i] .. db_off[i+1]) and g_maxMismatch = mm500; items on up to n_threads threads.
int pgh_dd_contains_cpu(uint32_t n, const uint8_t *q, const uint64_t *q_off, const uint8_t *db, const uint64_t *db_off, const uint32_t *mm500,
                        uint8_t *out, int n_threads)
{
    const unsigned nt = (unsigned)std::max(1, std::min(n_threads > 0 ? n_threads : 1, 64));
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++)
        th.emplace_back([=]() {
            for (uint32_t i = t; i < n; i += nt) {
                const std::string query((const char *)q + q_off[i], (size_t)(q_off[i + 1] - q_off[i]));
                out[i] = dd_contains_any_strand(query, (const char *)db + db_off[i], (size_t)(db_off[i + 1] - db_off[i]), mm500) ? 1 : 0;
            }
        });
    for (std::thread &x : th) x.join();
    return 0;
}

/*
 * The dispersed-duplication breakpoint tables (pindel_pg.h "dispersed-duplication breakpoint tables"), on the host: the
 * plain-loop statement (dd_tables_from_close) the device entry pg_device_batch_dd is compared with, byte for byte.  The reads as they
 * were handed to the search (seq, seq_off, strand) with their close end (has, rc_flag, last_abs = close_last, last_len = close_max);
 * the segments and window parameters of pg_dd_window; chrom = the chrom_len padded bases of chr_id, mm500 = g_maxMismatch: the
 * containment test runs on the host.  out_members: room for n_reads entries, out_cands likewise, out_cons: cons_cap bytes; sizes:
 * what was filled.  -1: a null array, an argument pg_device_batch_dd refuses, or a consensus pool beyond cons_cap.
 */
int pgh_dd_tables_from_close(uint32_t n_reads, const uint8_t *seq, const uint64_t *seq_off, const uint8_t *strand, const uint8_t *has,
                             const uint8_t *rc_flag, const uint32_t *last_abs, const uint16_t *last_len, const uint32_t *seg_first,
                             const uint8_t *seg_strand, uint32_t n_seg, int32_t chr_id, int32_t min_bp_support, int32_t min_map_distance,
                             const uint8_t *chrom, uint64_t chrom_len, const uint32_t *mm500, pg_dd_member *out_members, pg_dd_cand *out_cands,
                             uint8_t *out_cons, uint64_t cons_cap, pg_dd_sizes *sizes)
{
    if (!sizes || !mm500 || (chrom_len && !chrom) || (n_seg && (!seg_first || !seg_strand)) ||
        (n_reads && (!seq_off || !strand || !has || !rc_flag || !last_abs || !last_len || !out_members || !out_cands))) {
        g_err = "pgh_dd_tables_from_close: null array";
        return -1;
    }
    for (uint32_t s = 0; s < n_seg; s++)
        if (seg_first[s] > seg_first[s + 1] || seg_first[s + 1] > n_reads || (seg_strand[s] != '+' && seg_strand[s] != '-')) {
            g_err = "pgh_dd_tables_from_close: malformed segments";
            return -1;
        }
    if (min_map_distance < 1) {
        g_err = "pgh_dd_tables_from_close: min_map_distance < 1";
        return -1;
    }
    pg_adapter::Batch batch;
    batch.off.assign(1, 0);
    if (n_reads) {
        batch.off.assign(seq_off, seq_off + n_reads + 1);
        batch.seq.assign(seq, seq + seq_off[n_reads]);
        batch.strand.assign(strand, strand + n_reads);
    }
    std::vector<DDClose> close(n_reads);
    for (uint32_t i = 0; i < n_reads; i++) {
        close[i].has = has[i];
        close[i].rc_flag = rc_flag[i];
        close[i].last_abs = last_abs[i];
        close[i].last_len = last_len[i];
    }
    DDWindow w;
    w.chr_id = chr_id;
    w.chr_len = chrom_len;
    w.min_bp_support = min_bp_support;
    w.min_map_distance = min_map_distance;
    const std::string chrom_seq = chrom_len ? std::string((const char *)chrom, (size_t)chrom_len) : std::string();
    DDTables t;
    dd_tables_from_close(batch, close, std::vector<uint32_t>(seg_first, seg_first + (n_seg ? n_seg + 1 : 0)),
                         std::vector<uint8_t>(seg_strand, seg_strand + n_seg), w, chrom_seq, mm500, t);
    if (t.cons.size() > cons_cap) {
        g_err = "pgh_dd_tables_from_close: the consensus pool exceeds cons_cap";
        return -1;
    }
    if (!t.members.empty()) memcpy(out_members, t.members.data(), t.members.size() * sizeof(pg_dd_member));
    if (!t.cands.empty()) memcpy(out_cands, t.cands.data(), t.cands.size() * sizeof(pg_dd_cand));
    if (!t.cons.empty()) memcpy(out_cons, t.cons.data(), t.cons.size());
    sizes->members = t.members.size();
    sizes->cands = t.cands.size();
    sizes->cons_bytes = t.cons.size();
    return 0;
}

/*
 * Test hook: the single consumer of the breakpoint tables (dd_cands_text) on tables made by hand.  The n_reads split reads as ingested
 * (name as a NUL-terminated string, bytes, anchor strand; every read gets `sample`), the tables and the number of segments.  text
 * (text_cap bytes): per segment and candidate, in the consumer's order, a line "C seg bio_bp tested contained consensus" followed by
 * one line "R name sample sequence mapped unmapped" per read (tab-separated).  -1: tables that do not fit the reads, or a text
 * beyond text_cap.
 */
int pgh_dd_cands_from_tables(uint32_t spacer, uint32_t n_reads, const char *const *names, const char *sample, const uint8_t *seq,
                             const uint64_t *seq_off, const uint8_t *strand, uint32_t n_seg, const pg_dd_member *members, const pg_dd_cand *cands,
                             const uint8_t *cons, const pg_dd_sizes *sizes, char *text, uint64_t text_cap)
{
    if (!sizes || !text || !text_cap || !sample || (n_reads && (!names || !seq_off || !strand)) || (sizes->members && !members) ||
        (sizes->cands && !cands) || (sizes->cons_bytes && !cons)) {
        g_err = "pgh_dd_cands_from_tables: null array";
        return -1;
    }
    DDTables t;
    t.members.assign(members, members + sizes->members);
    t.cands.assign(cands, cands + sizes->cands);
    t.cons.assign(cons, cons + sizes->cons_bytes);
    std::vector<std::string> nm(n_reads);
    for (uint32_t i = 0; i < n_reads; i++) nm[i] = names[i];
    std::string out;
    if (!dd_cands_text(spacer, nm, sample, seq, seq_off, strand, n_reads, n_seg, t, out)) {
        g_err = "pgh_dd_cands_from_tables: the tables do not fit the reads";
        return -1;
    }
    if (out.size() + 1 > text_cap) {
        g_err = "pgh_dd_cands_from_tables: the text exceeds text_cap";
        return -1;
    }
    memcpy(text, out.c_str(), out.size() + 1);
    return 0;
}

// The close end of one batch for pgh_dd_run, supplied by the caller: per read has / rc_flag / UP_Close.back() AbsLoc, LengthStr.
typedef int (*pgh_dd_close_cb)(uint32_t n, const uint8_t *seq, const uint64_t *off, const uint8_t *strand, const int32_t *pos,
                               const int16_t *isz, const int32_t *chr, uint8_t *has, uint8_t *rc_flag, uint32_t *last_abs,
                               uint16_t *last_len);

// The -q pipeline (pg_dd.hpp) of `pindel_pg -f fasta -i config -o prefix -q [flags]` with the close ends from `close_cb` (null: no read
// has one) and the containment test on the host.  opts: MAX_DD_BREAKPOINT_DISTANCE, MAX_DISTANCE_CLUSTER_READS, MIN_DD_CLUSTER_SIZE,
// MIN_DD_BREAKPOINT_SUPPORT, MIN_DD_MAP_DISTANCE, DD_REPORT_DUPLICATION_READS, -A, -n; mm_rate = -u; region / include_bed /
// exclude_bed (nullable) = -c / -j / -J.  The configuration file, the region plan and the read selection are the command line's own
// (read_bam_config, region_plan, BamIngestSettings).  stats6 (nullable): discordant reads, clusters, breakpoints, containment tests,
// breakpoints kept by them, events; bp5 (nullable, cap breakpoints): tid, pos, strand, #reads, #split reads per breakpoint; tested
// (nullable, tested_cap bytes): per containment test a line "tid pos strand #split-reads consensus contained" (tab-separated).
// Returns the number of breakpoints, or -1 (pgh_last_error).
int64_t pgh_dd_run(const char *fasta, const char *bam_config, const char *prefix, const int32_t *opts, double mm_rate, const char *region,
                   const char *include_bed, const char *exclude_bed, double window_mbp, uint32_t spacer, const uint32_t *mm500,
                   pgh_dd_close_cb close_cb, uint64_t *stats6, int32_t *bp5, uint64_t cap, char *tested, uint64_t tested_cap)
{
    std::string err;
    std::vector<Chromosome> genome;
    if (load_fasta(fasta, genome, spacer, err)) {
        g_err = err;
        return -1;
    }
    std::vector<BamSource> bams;
    if (!read_bam_config(bam_config, bams, err)) {
        g_err = err;
        return -1;
    }
    const std::vector<unsigned> sizes = chromosome_sizes(genome, read_fai(fasta, genome), spacer);
    std::vector<RegionRecord> plan;
    if (region_plan(chromosome_names(genome), sizes, region ? region : "", include_bed ? include_bed : "", exclude_bed ? exclude_bed : "",
                    plan, err)) {
        g_err = err;
        return -1;
    }
    BamIngestSettings ing;
    ing.min_anchor_quality = (unsigned)opts[6];
    ing.spacer = spacer;
    ing.nm = opts[7];
    ing.max_mismatch_rate = mm_rate;
    DDSettings dd;
    dd.max_bp_distance = opts[0];
    dd.max_distance_cluster = opts[1];
    dd.min_cluster_size = opts[2];
    dd.min_bp_support = opts[3];
    dd.min_map_distance = opts[4];
    dd.report_dup_reads = opts[5] != 0;
    std::vector<uint32_t> mm(mm500, mm500 + 500);
    auto close_fn = [&](int, const pg_adapter::Batch &b, std::vector<DDClose> &out) {
        const size_t n = b.strand.size();
        out.assign(n, DDClose());
        if (!close_cb || !n) return 0;
        std::vector<uint8_t> has(n), rcf(n);
        std::vector<uint32_t> la(n);
        std::vector<uint16_t> ll(n);
        const int rc = close_cb((uint32_t)n, b.seq.data(), b.off.data(), b.strand.data(), b.pos.data(), b.isz.data(), b.chr.data(), has.data(),
                                rcf.data(), la.data(), ll.data());
        for (size_t i = 0; i < n; i++) {
            out[i].has = has[i];
            out[i].rc_flag = rcf[i];
            out[i].last_abs = la[i];
            out[i].last_len = ll[i];
        }
        return rc;
    };
    auto contains_fn = [&](const std::vector<std::string> &q, const std::vector<int32_t> &chr, const std::vector<uint64_t> &st,
                           const std::vector<uint32_t> &len, std::vector<uint8_t> &found) {
        found.assign(q.size(), 0);
        for (size_t i = 0; i < q.size(); i++)
            found[i] = dd_contains_any_strand(q[i], genome[(size_t)chr[i]].seq.data() + st[i], len[i], mm.data()) ? 1 : 0;
        return 0;
    };
    DDStats stats;
    if (run_dd(genome, sizes, plan, bams, ing, window_mbp, dd, prefix, close_fn, contains_fn, err, &stats)) {
        g_err = err;
        return -1;
    }
    if (stats6) {
        const size_t v[6] = { stats.discordant, stats.clusters, stats.breakpoints, stats.candidates, stats.kept_by_containment, stats.events };
        for (int k = 0; k < 6; k++) stats6[k] = v[k];
    }
    const size_t n_bp = stats.bp_list.size() / 5;
    if (bp5)
        for (size_t k = 0; k < std::min<size_t>(n_bp, cap) * 5; k++) bp5[k] = stats.bp_list[k];
    if (tested && tested_cap) {
        const size_t m = std::min<size_t>(stats.tested.size(), tested_cap - 1);
        memcpy(tested, stats.tested.data(), m);
        tested[m] = 0;
    }
    return (int64_t)n_bp;
}

}  // extern "C"
