// pindel_pg -- command line with Pindel's flags for the path this repository implements:
//   pindel_pg -f ref.fa (-p reads.txt[.gz] | -P text_config | -i bam_config) -o prefix
//                                              [-x 2 -a 1 -m 3 -u 0.02 -e 0.01 -E 0.95 -H 8
//                                               -M 1 -B 100 -d 30 -v 50 -w 5 -G device -l -s -S -I
//                                               -c ALL|chr[:start[-end]] -j include.bed -J exclude.bed -N
//                                               --repair int-pairs,inv-pairs,depth-mapq,bed0|all
//                                               --device-classifier [-listed 0..4 -hints -li -int -dd]]
// FASTA + Pindel-text reads -> close/far-end search on the MI355X (C ABI, libpindel_pg.so)
// -> SV classification and <prefix>_D/_SI/_TD/_INV reports (host code in this directory);
// -l adds <prefix>_LI (long insertions), -s <prefix>_CloseEndMapped (the reads with a close end),
// -S writes <prefix>_CloseEndMapped only (no far end, no SV search); -q adds <prefix>_DD (dispersed duplications, BAM input,
// pg_dd.hpp); -I adds <prefix>_INT and <prefix>_INT_final (interchromosomal events, pg_host_int.cpp: far ends on other chromosomes
// need window hints, i.e. BAM input with -R or `-b file --bd-hints on`; on the --device-classifier path -I needs
// --device-classifier-int, which writes _INT from junction tables built on the device; likewise -q needs
// --device-classifier-dd there, which takes the breakpoint tables, their consensus and the containment verdicts of _DD from the device,
// DESIGN.md 7s).  -P lists Pindel-text files, one per line (read before a
// -p file when both are given); a text file whose name ends in .gz is read through zlib.  -N (--NormalSamples) turns on the
// germline filter of _TD and _INV for BAM input (pg_depth.hpp); for text input it changes nothing.
// --repair LIST (off by default) turns on fixes of reference defects that are otherwise reproduced byte for byte:
// int-pairs (-I reports every chromosome pair of a window), inv-pairs (-N counts read pairs for inversions of two read lengths or
// more instead of dropping them all), depth-mapq (-N's read depth ignores records below MAPQ 20), bed0 (-j / -J files are 0-based,
// half-open); `all` is all four.  An unknown name or an empty list is a usage error (exit status 2, nothing written).
// Like the reference, every run
// creates all seven files (_D _SI _TD _INV _LI _BP _CloseEndMapped); _BP stays empty, as the
// reference's breakpoint report is not called.  -c, -j and -J select the regions searched (pg_region.hpp); they are
// checked before the first device call (exit status 2 for -c syntax, 1 for an unreadable file or an unknown chromosome).
// Flags and their defaults follow src/fn_parameters.cpp; BAM input (-i) is read without htslib (pg_bam.hpp).
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <fstream>
#include <algorithm>
#include <iterator>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "pg_adapter.hpp"
#include "pg_bdhints.hpp"
#include "pg_cli.hpp"
#include "pg_dd.hpp"
#include "pg_host.hpp"
#include "pg_pipeline.hpp"
#include "pg_region.hpp"
#include "pindel_pg.h"

using namespace pgh;

static double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static int fail(const std::string &msg, int status = 1)
{
    fprintf(stderr, "pindel_pg: %s\n", msg.c_str());
    return status;
}

// What the search steps add up over the windows of a run
struct RunCounts {
    size_t n_close = 0, n_far = 0;
    double t_search = 0.0;
};

static const auto chr_of = [](const SplitRead &r) { return r.chr_id; };
static const auto make_point = [](const pg_point &p) { return to_unique_point(p); };

// The inputs a run needs, and the -P list: checked before anything is written and before any device is touched
static int check_inputs(const CliOptions &o)
{
    const bool text_input = !o.reads_path.empty() || !o.pindel_config.empty();
    if (text_input && !o.bam_config.empty())
        return fail("mixed input is not supported: give either BAM input (-i) or Pindel-text input (-p, -P), not both", 2);
    if (o.fasta.empty() || (!text_input && o.bam_config.empty()) || o.prefix.empty()) {
        fprintf(stderr, "usage: pindel_pg -f ref.fa (-p reads.txt[.gz] | -P text_config.txt | -i bam_config.txt) -o prefix [options]\n");
        return 2;
    }
    std::vector<std::string> listed;
    std::string err;
    if (!o.pindel_config.empty() && read_pindel_config(o.pindel_config, listed, err)) return fail(err);
    return 0;
}

// TestFileForOutput (pindel.cpp:932-938): every output file exists, empty, from the start
// (... and with -I its two files: <prefix>_INT is truncated here, where the reference only ever appends to it)
static int create_outputs(const CliOptions &o)
{
    std::vector<const char *> suffixes = { "_D", "_SI", "_TD", "_INV", "_LI", "_BP", "_CloseEndMapped" };
    if (o.S.report_interchromosomal) suffixes.insert(suffixes.end(), { "_INT", "_INT_final" });
    for (const char *sf : suffixes) {
        std::ofstream f((o.prefix + sf).c_str(), std::ios::trunc);
        if (!f) return fail("cannot write " + o.prefix + sf);
    }
    return 0;
}

// The reference and the region plan (main's IncludeBed, src/pindel.cpp:1605-1720), complete before any device is touched;
// sizes: the chromosome sizes the plan was made with
static int load_genome_and_plan(const CliOptions &o, std::vector<Chromosome> &genome, std::vector<unsigned> &sizes, std::vector<RegionRecord> &plan)
{
    std::string err;
    if (load_fasta(o.fasta, genome, o.prm.spacer, err)) return fail(err);
    sizes = chromosome_sizes(genome, read_fai(o.fasta, genome), o.prm.spacer);
    const int rc = region_plan(chromosome_names(genome), sizes, o.region, o.include_bed, o.exclude_bed, plan, err, o.S.repair(REPAIR_BED0));
    return rc ? fail(err, rc) : 0;
}

// The reads of Pindel-text input, or the BAMs of -i (one line per BAM: file, insert size, sample tag; readBamConfigFile,
// src/pindel.cpp) with -N's germline filter on them
static int load_reads(CliOptions &o, const std::vector<Chromosome> &genome, std::vector<SplitRead> &all, std::vector<BamSource> &bams)
{
    std::string err;
    if (o.bam_config.empty() && load_pindel_inputs(o.pindel_config, o.reads_path, genome, all, err)) return fail(err);
    if (!o.bam_config.empty() && !read_bam_config(o.bam_config, bams, err)) return fail(err);
    // -N: IsGoodTD / IsGoodINV filter only when the reads come from BAMs (they return true early for -p and -P)
    if (o.S.NormalSamples && !bams.empty() && !(o.S.germline = open_germline(bams, err, o.S.repairs))) return fail(err);
    if (o.S.NormalSamples && bams.empty()) printf("pindel_pg: -N has no effect on Pindel-text input (as in Pindel)\n");
    return 0;
}

// -G 0,1,...: one pg_ctx per device, the reference replicated into each (the reads of every bin are sharded over them);
// destroyed with this object
struct Devices {
    std::vector<pg_ctx *> ctxs;
    Devices() = default;
    Devices(const Devices &) = delete;
    Devices &operator=(const Devices &) = delete;
    ~Devices() { for (pg_ctx *c : ctxs) pg_destroy(c); }
    int open(const CliOptions &o, const std::vector<Chromosome> &genome)
    {
        for (int d : o.devices) {
            pg_params p = o.prm;
            p.device = d;
            pg_ctx *c = nullptr;
            const int rc = pg_create(&p, &c);
            if (rc) {
                fprintf(stderr, "pindel_pg: pg_create failed (%d) on device %d: no usable MI355X / HIP device\n", rc, d);
                return 1;
            }
            ctxs.push_back(c);
        }
        std::vector<const char *> names;
        std::vector<const uint8_t *> seqs;
        std::vector<uint64_t> lens;
        for (const Chromosome &c : genome) {
            names.push_back(c.name.c_str());
            seqs.push_back((const uint8_t *)c.seq.data());
            lens.push_back(c.seq.size());
        }
        for (pg_ctx *c : ctxs)
            if (pg_load_reference(c, (int32_t)genome.size(), names.data(), seqs.data(), lens.data()))
                return fail(std::string("pg_load_reference: ") + pg_last_error(c));
        return 0;
    }
};

// -b: Pindel 0.2.5b9 loads the file but, for Pindel-text input, never hands its events to the far-end
// search.  That is the default here too.  "--bd-hints on" searches the windows of
// the file's events before the ranges, the way the BAM path of the reference does (pg_bdhints.hpp).
static int load_hints(const CliOptions &o, BDHints &bd)
{
    if (!o.bd_path.empty()) {
        std::string note;
        const int brc = bd.load_file(o.bd_path, o.prm.spacer, note);
        if (brc < 0) return fail(note);
        if (brc > 0) printf("pindel_pg: %s\n", note.c_str());
        printf("pindel_pg: BD events: %zu%s\n", bd.n_events(), o.use_bd ? "" : " (not used for Pindel-text input; --bd-hints on to use them)");
    }
    if (o.S.report_interchromosomal && o.bam_config.empty() && !(o.use_bd && bd.n_events()))
        printf("pindel_pg: -I without window hints (BAM input, or -b file --bd-hints on): no far end is searched on another chromosome, "
               "%s_INT and %s_INT_final stay empty\n", o.prefix.c_str(), o.prefix.c_str());
    return 0;
}

// The reads of every bin are sharded over the devices in contiguous ranges (reads are independent: the loop of SearchFarEnds /
// ReadBuffer::flush, src/pindel.cpp:1115-1138) and the results concatenated in order -- identical reports for any device
// count.  n items on nd devices are one shard when there are not two items per device.
static size_t n_shards(size_t nd, size_t n) { return (nd > 1 && n >= 2 * nd) ? nd : 1; }
// fn(d, lo, hi) on the shards [n * d / np, n * (d + 1) / np), one host thread per shard when there are several; the last
// non-zero status in device order
template <class Fn>
static int for_shards(size_t nd, size_t n, Fn fn)
{
    const size_t np = n_shards(nd, n);
    if (np == 1) return fn((size_t)0, (size_t)0, n);
    std::vector<int> rcs(np, 0);
    std::vector<std::thread> th;
    for (size_t d = 0; d < np; d++) th.emplace_back([&, d]() { rcs[d] = fn(d, n * d / np, n * (d + 1) / np); });
    for (std::thread &x : th) x.join();
    int r = 0;
    for (int x : rcs)
        if (x) r = x;
    return r;
}

// fn(ctx, part) on the shards of `reads`: the parts are moved out and back, so the order is kept
template <class Fn>
static int on_devices(const std::vector<pg_ctx *> &ctxs, std::vector<SplitRead> &reads, Fn fn)
{
    if (n_shards(ctxs.size(), reads.size()) == 1) return fn(ctxs[0], reads);
    return for_shards(ctxs.size(), reads.size(), [&](size_t d, size_t lo, size_t hi) {
        std::vector<SplitRead> part(std::make_move_iterator(reads.begin() + lo), std::make_move_iterator(reads.begin() + hi));
        const int r = fn(ctxs[d], part);
        std::move(part.begin(), part.end(), reads.begin() + lo);
        return r;
    });
}

// What the seam steps of the two pipelines work with
struct Seams {
    const CliOptions &o;
    const std::vector<pg_ctx *> &ctxs;
    BDHints &bd;
    bool use_bd;                                 // window hints are live (--bd-hints on; BAM input: -R)
    std::vector<std::string> chr_names;
    RunCounts &counts;
};

// Seam 1 (ReadBuffer::flush, src/read_buffer.cpp:36-101): the close end of ALL reads of the bin, `flush_reads` at a
// time like the reference's 50 000-read buffer (src/reader.cpp:55; 0 = the whole bin in one call -- the results do
// not depend on it).  The pipeline then keeps the reads with a close end, as flush() does (:55-64).
struct CloseSearch {
    const Seams &s;
    int operator()(const Chromosome &, int, std::vector<SplitRead> &reads, const std::vector<uint32_t> &) const
    {
        const double t0 = now_s();
        const size_t flush_reads = s.o.flush_reads;
        const int r = on_devices(s.ctxs, reads, [flush_reads](pg_ctx *c, std::vector<SplitRead> &part) {
            const size_t step = flush_reads ? flush_reads : std::max<size_t>(part.size(), 1);
            if (step >= part.size()) {
                pg_result *res = nullptr;
                const int rr = pg_adapter::CloseEndBatch(c, part, chr_of, make_point, &res);
                pg_result_free(res);
                return rr;
            }
            for (size_t lo = 0; lo < part.size(); lo += step) {
                const size_t hi = std::min(part.size(), lo + step);
                std::vector<SplitRead> buf(std::make_move_iterator(part.begin() + lo), std::make_move_iterator(part.begin() + hi));
                pg_result *res = nullptr;
                const int rr = pg_adapter::CloseEndBatch(c, buf, chr_of, make_point, &res);
                pg_result_free(res);
                std::move(buf.begin(), buf.end(), part.begin() + lo);
                if (rr) return rr;
            }
            return 0;
        });
        if (s.o.S.only_close_mapped)          // (otherwise the far-end step counts the reads that kept a close end)
            for (const SplitRead &x : reads) s.counts.n_close += !x.UP_Close.empty();
        s.counts.t_search += now_s() - t0;
        return r;
    }
};

// Seam 1 of the BAM path, on the ingested structure-of-arrays batch: one pg_close_end_batch per device on a contiguous part
struct CloseSoa {
    const Seams &s;
    int operator()(const Chromosome &, int, const pg_adapter::Batch &batch, CloseView &view) const
    {
        const double t0 = now_s();
        const size_t n = batch.strand.size(), np = n_shards(s.ctxs.size(), n);
        std::vector<pg_result *> res(np, nullptr);
        const int r = for_shards(s.ctxs.size(), n, [&](size_t d, size_t lo, size_t hi) {
            pg_read_batch v = batch.view();
            v.n_reads = (uint32_t)(hi - lo);
            v.seq_off += lo;
            v.anchor_strand += lo;
            v.anchor_pos += lo;
            v.insert_size += lo;
            v.chr_id += lo;
            return pg_close_end_batch(s.ctxs[d], &v, &res[d]);
        });
        view.release = [res]() { for (pg_result *x : res) pg_result_free(x); };
        if (r) {
            view.release();
            view.release = nullptr;
            return r;
        }
        for (size_t d = 0; d < np; d++) {
            pg_result_view rv;
            pg_result_view_get(res[d], &rv);
            if (s.o.S.only_close_mapped)
                for (size_t i = 0; i < rv.n_reads; i++) s.counts.n_close += rv.close_off[i + 1] > rv.close_off[i];
            ClosePart p;
            p.first = n * d / np;
            p.n = rv.n_reads;
            p.rc_flag = rv.rc_flag;
            p.close_off = rv.close_off;
            p.close_runs = rv.close_runs;
            view.parts.push_back(p);
        }
        s.counts.t_search += now_s() - t0;
        return 0;
    }
};

// BDHints::table() as the C ABI takes it: a pg_hint_table over the arrays kept here
struct HintTableView {
    BDHints::Table tab;
    std::vector<pg_window> win;
    pg_hint_table t = { 0, nullptr, nullptr, 0, nullptr, nullptr };
    void set(BDHints::Table &&from)
    {
        tab = std::move(from);
        win.resize(tab.win.size());
        for (size_t k = 0; k < win.size(); k++) win[k] = { tab.win[k].chr_id, (int32_t)tab.win[k].start, (int32_t)tab.win[k].end };
        t.n_runs = (uint32_t)tab.run_cluster.size();
        t.run_first = tab.run_first.data();
        t.run_cluster = tab.run_cluster.data();
        t.n_clusters = tab.cluster_off.empty() ? 0u : (uint32_t)(tab.cluster_off.size() - 1);
        t.cluster_off = tab.cluster_off.data();
        t.windows = win.empty() ? nullptr : win.data();
    }
};

// Seam 2 (SearchFarEnds, src/pindel.cpp:1115-1138, called at :1888 on state.Reads_SR): the far end of the reads that
// kept a close end -- the filtered union of the flushes -- through pg_far_end_batch_from_close (a hinted window: through
// pg_far_end_batch_from_close_table, with the window's hints as one table).
struct FarSearch {
    const Seams &s;
    int operator()(const Chromosome &, int chr_id, std::vector<SplitRead> &kept, unsigned ws, unsigned we) const
    {
        const double t0 = now_s();
        const bool hinted = s.use_bd && s.bd.n_events() && !kept.empty();
        if (hinted) {
            // the window main() is working on, as it hands it to g_bdData.loadRegion (currentWindow_cs, pindel.cpp:1828, 1853):
            // [ws, we) + spacer, we clipped to the end of the scanned region (LoopingSearchWindow::updateEndPositions).  NOT
            // derived from the reads: a BAM window also holds reads whose anchor lies before ws (reader.cpp has no position
            // filter on that path), and the bin of min(MatchedRelPos) would then be the previous window.
            std::string berr;
            if (!s.bd.load_region(s.chr_names, chr_id, ws + s.o.prm.spacer, we + s.o.prm.spacer, berr)) return fail(berr, (int)PG_E_INVALID);
        }
        const BDHints &bd = s.bd;
        // the window's hints as ONE position-keyed table, looked up per read on the device (pg_far_end_batch_from_close_table);
        // PGH_HINT_LOOKUP=host: the per-read lookup on the host and the replicated upload instead (same reports)
        static const bool host_lookup = [] { const char *e = getenv("PGH_HINT_LOOKUP"); return e && std::string(e) == "host"; }();
        HintTableView tab;
        if (hinted && !host_lookup) tab.set(bd.table());
        if (hinted) {
            if (host_lookup) printf("Window hints: host lookup, per-read clusters uploaded\n");
            else printf("Window hints: device lookup, table of %u runs / %u clusters / %zu windows\n", tab.t.n_runs, tab.t.n_clusters, tab.win.size());
        }
        const pg_hint_table *tp = hinted && !host_lookup ? &tab.t : nullptr;
        const int r = on_devices(s.ctxs, kept, [&bd, hinted, tp](pg_ctx *c, std::vector<SplitRead> &part) {
            if (!hinted || part.empty()) return pg_adapter::SearchFarEnds(c, part, chr_of, make_point, nullptr);
            if (tp) return pg_adapter::SearchFarEndsTable(c, part, chr_of, make_point, tp);
            const HintWindows hw = hint_windows(bd, part.size(), [&](size_t i) { return part[i].UP_Close.back().AbsLoc; });
            std::vector<pg_window> win(hw.win.size());
            for (size_t k = 0; k < win.size(); k++) win[k] = { hw.win[k].chr_id, (int32_t)hw.win[k].start, (int32_t)hw.win[k].end };
            const pg_windows hints = { hw.off.data(), win.empty() ? nullptr : win.data() };
            return pg_adapter::SearchFarEnds(c, part, chr_of, make_point, &hints);
        });
        size_t bin_far = 0;
        for (const SplitRead &x : kept) bin_far += !x.UP_Far.empty();
        s.counts.n_close += kept.size();
        s.counts.n_far += bin_far;
        // ReportCloseAndFarEndCounts (src/pindel.cpp:1094-1113), over the reads that kept a close end
        printf("Total: %zu;\tClose_end_found %zu;\tFar_end_found %zu;\tUsed\t0.\n\nFor LI and BP: %zu\n\n", kept.size(), kept.size(),
               bin_far, kept.size() - bin_far);
        s.counts.t_search += now_s() - t0;
        return r;
    }
};

// --device-classifier: one window as one device batch -- upload, fused search, name ids by first occurrence,
// pg_device_batch_classify with the window process_window would use, the tables, records and summaries downloaded, and
// Caller::process_window_from_tables.  The points stay on the device unless the window has an unresolved read or its tables do not
// fit: then pg_device_batch_download fetches them and the window goes on through the existing steps.
struct DeviceClassifierStats {
    size_t windows = 0, from_tables = 0, fallbacks = 0, unresolved = 0, records = 0, runs_kept = 0, hinted = 0;
    size_t li_windows = 0, li_bytes = 0;         // windows with LI tables, and the bytes downloaded for them
    size_t int_windows = 0, int_bytes = 0;       // windows with junction tables, and the bytes downloaded for them
};
struct DeviceClassifier {
    const Seams &s;
    DeviceClassifierStats &st;
    bool bam;                                    // BAM input: ReadLength follows the sequence GetCloseEnd left
    std::vector<int32_t> chr_rank;               // -I: the ranks of the reference's chromosome names (pg_int_window), once per run
    int operator()(const Chromosome &chrom, int chr_id, std::vector<SplitRead> &reads, unsigned ws, unsigned we, unsigned bed_start,
                   unsigned bed_end, Caller &caller, const std::function<void()> &after_close) const
    {
        const double t0 = now_s();
        pg_ctx *ctx = s.ctxs[0];
        const size_t n = reads.size();
        const pg_adapter::Batch batch = pg_adapter::make_batch(reads, chr_of);
        pg_read_batch v = batch.view();
        pg_device_batch *b = nullptr;
        int rc = pg_device_batch_upload(ctx, &v, &b);
        if (rc) return rc;
        struct Free {
            pg_ctx *c;
            pg_device_batch *b;
            ~Free() { pg_device_batch_free(c, b); }
        } free_batch = { ctx, b };
        // a hinted window (--device-classifier-hints): FarSearch's condition without `kept` -- the close ends are
        // not on the host -- its region and its table, looked up on the device between the close and the far launch
        const bool hinted = s.use_bd && s.bd.n_events() && n;
        if (hinted) {
            std::string berr;
            if (!s.bd.load_region(s.chr_names, chr_id, ws + s.o.prm.spacer, we + s.o.prm.spacer, berr)) return fail(berr, (int)PG_E_INVALID);
            HintTableView tab;
            tab.set(s.bd.table());
            printf("Window hints: device lookup, table of %u runs / %u clusters / %zu windows\n", tab.t.n_runs, tab.t.n_clusters, tab.win.size());
            if ((rc = pg_device_batch_search_table(ctx, b, &tab.t))) return rc;
            st.hinted++;
        } else if ((rc = pg_device_batch_pack_search(ctx, b)))
            return rc;
        std::vector<uint32_t> name_id(n);
        {
            std::unordered_map<std::string, uint32_t> seen;
            seen.reserve(n * 2);
            for (size_t i = 0; i < n; i++) name_id[i] = seen.emplace(reads[i].Name, (uint32_t)seen.size()).first->second;
        }
        pg_classify_params p;
        p.window.chr_id = chr_id;
        p.window.win_end = we;
        p.window.region_start = bed_start;
        p.window.region_end = bed_end;
        p.window.min_support = s.o.S.NumRead2ReportCutOff;
        p.window.balance_cutoff = s.o.S.BalanceCutoff;
        p.window.analyze_td = s.o.S.Analyze_TD;
        p.window.analyze_inv = s.o.S.Analyze_INV;
        p.sv.seq_error_rate = s.o.S.Seq_Error_Rate;
        p.sv.min_num_matched_bases = s.o.S.Min_Num_Matched_Bases;
        p.sv.min_inversion_size = s.o.S.MIN_IndelSize_Inversion;
        p.max_listed = s.o.device_classifier_listed < 0 ? PG_VARIANT_CANDS : s.o.device_classifier_listed;
        p.reserved = 0;
        if ((rc = pg_device_batch_classify(ctx, b, &p, name_id.data()))) return rc;
        pg_event_sizes es;
        pg_sv_event_sizes ss;
        pg_report_sizes rs;
        if ((rc = pg_device_batch_event_sizes(ctx, b, &es)) || (rc = pg_device_batch_sv_event_sizes(ctx, b, &ss)) ||
            (rc = pg_device_batch_report_sizes(ctx, b, &rs)))
            return rc;
        size_t nm = 0, ne = 0, snm = 0, sne = 0;
        for (int t = 0; t < PG_EVENT_TABLES; t++) nm += es.members[t], ne += es.events[t];
        for (int t = 0; t < PG_SV_EVENT_TABLES; t++) snm += ss.members[t], sne += ss.events[t];
        std::vector<pg_event_read> recs(n);
        std::vector<pg_event> events(ne), sv_events(sne);
        std::vector<pg_report_read> records(rs.records);
        std::vector<pg_report_summary> summaries(n);
        // (the member lists stay on the device: every member has its record)
        if ((rc = pg_device_batch_events_download(ctx, b, recs.data(), nullptr, events.data())) ||
            (rc = pg_device_batch_sv_events_download(ctx, b, nullptr, sv_events.data())) ||
            (rc = pg_device_batch_report_download(ctx, b, records.data(), summaries.data())))
            return rc;
        // ReportCloseAndFarEndCounts (src/pindel.cpp:1094-1113), over the reads that kept a close end, from the summaries
        size_t n_close = 0, n_far = 0;
        for (const pg_report_summary &x : summaries) {
            n_close += (x.flags & PG_RS_CLOSE) != 0;
            n_far += (x.flags & PG_RS_CLOSE) && (x.flags & PG_RS_FAR);
        }
        s.counts.n_close += n_close;
        s.counts.n_far += n_far;
        printf("Total: %zu;\tClose_end_found %zu;\tFar_end_found %zu;\tUsed\t0.\n\nFor LI and BP: %zu\n\n", n_close, n_close, n_far,
               n_close - n_far);
        st.windows++;
        // do the tables fit ?  every member has a record of a read of this window, every event lies in its member list
        bool fits = rs.records == nm + snm && rs.reads == n;
        for (const pg_report_read &r : records) fits = fits && r.read < n && r.table < PG_EVENT_TABLES + PG_SV_EVENT_TABLES;
        {
            size_t e0 = 0;
            for (int t = 0; t < PG_EVENT_TABLES && fits; t++) {
                for (size_t k = 0; k < es.events[t]; k++) {
                    const pg_event &ev = events[e0 + k];
                    fits = fits && ev.n_reads > 0 && (uint64_t)ev.first + ev.n_reads <= es.members[t] && ev.box_head <= ev.first;
                }
                e0 += (size_t)es.events[t];
            }
            e0 = 0;
            for (int t = 0; t < PG_SV_EVENT_TABLES && fits; t++) {
                for (size_t k = 0; k < ss.events[t]; k++) {
                    const pg_event &ev = sv_events[e0 + k];
                    fits = fits && ev.n_reads > 0 && (uint64_t)ev.first + ev.n_reads <= ss.members[t];
                }
                e0 += (size_t)ss.events[t];
            }
        }
        if (es.unresolved == 0 && fits) {
            // -l (--device-classifier-li): the long-insertion position tables of the window, built on the device from
            // the records the classify left; the pipeline has noted every read's insert size before this call
            LiTables li;
            const bool want_li = s.o.S.Analyze_LI && n_close;
            if (want_li) {
                pg_li_window lw;
                caller.li_window(chrom, ws, we, lw.lo, lw.hi);
                pg_li_sizes ls;
                if ((rc = pg_device_batch_li(ctx, b, &lw)) || (rc = pg_device_batch_li_sizes(ctx, b, &ls))) return rc;
                std::vector<uint32_t> members((size_t)(ls.members[0] + ls.members[1]));
                std::vector<pg_li_pos> positions((size_t)(ls.positions[0] + ls.positions[1]));
                if ((rc = pg_device_batch_li_download(ctx, b, members.data(), positions.data()))) return rc;
                size_t m0 = 0, p0 = 0;
                bool li_fits = true;
                for (int k = 0; k < 2; k++) {
                    li.members[k].assign(members.begin() + m0, members.begin() + m0 + (size_t)ls.members[k]);
                    li.positions[k].assign(positions.begin() + p0, positions.begin() + p0 + (size_t)ls.positions[k]);
                    for (uint32_t m : li.members[k]) li_fits = li_fits && m < n;
                    for (const pg_li_pos &q : li.positions[k]) li_fits = li_fits && (uint64_t)q.first + q.n_reads <= ls.members[k];
                    m0 += (size_t)ls.members[k];
                    p0 += (size_t)ls.positions[k];
                }
                if (!li_fits) return fail("the long-insertion tables of a window do not fit its reads", (int)PG_E_DEVICE);
                st.li_windows++;
                st.li_bytes += members.size() * sizeof(uint32_t) + positions.size() * sizeof(pg_li_pos);
            }
            // -I (--device-classifier-int): the junction tables of the window, built on the device from the search
            // result alone
            IntTables junctions;
            const bool want_int = s.o.S.report_interchromosomal && n_close;
            if (want_int) {
                const pg_int_window iw = { chr_rank.data(), (uint32_t)chr_rank.size() };
                pg_int_sizes is;
                if ((rc = pg_device_batch_int(ctx, b, &iw)) || (rc = pg_device_batch_int_sizes(ctx, b, &is))) return rc;
                junctions.members.resize((size_t)is.members);
                junctions.calls.resize((size_t)is.calls);
                if ((rc = pg_device_batch_int_download(ctx, b, junctions.members.data(), junctions.calls.data()))) return rc;
                bool int_fits = true;
                for (uint32_t m : junctions.members) int_fits = int_fits && m < n;
                for (const pg_int_call &q : junctions.calls) int_fits = int_fits && (uint64_t)q.first + q.n_reads <= is.members;
                if (!int_fits) return fail("the junction tables of a window do not fit its reads", (int)PG_E_DEVICE);
                st.int_windows++;
                st.int_bytes += junctions.members.size() * sizeof(uint32_t) + junctions.calls.size() * sizeof(pg_int_call);
            }
            s.counts.t_search += now_s() - t0;
            if (n_close) {                       // (a window without a close end has nothing to classify, as in the existing steps)
                caller.apply_summaries(reads, summaries.data(), bam);
                if (after_close) after_close();
                // -s: the reads that kept a close end, in input order, the sequence as rc_flag left it
                if (s.o.S.report_close_mapped) caller.report_close_mapped_summaries(reads, summaries.data());
                caller.process_window_from_tables(chrom, reads, ws, we, bed_start, bed_end, recs.data(), es, events.data(), ss, sv_events.data(),
                                                  records.data(), summaries.data(), true);
                if (want_li) caller.write_li_from_tables(chrom, reads, ws, we, li, summaries.data());
                if (want_int) caller.write_int_from_tables(reads, summaries.data(), junctions);
            } else if (after_close) after_close();
            uint64_t close_runs = 0, far_runs = 0;
            (void)pg_device_batch_result_sizes(ctx, b, &close_runs, &far_runs);
            st.runs_kept += (size_t)(close_runs + far_runs);
            st.from_tables++;
            st.records += records.size();
            return 0;
        }
        // the fallback: the window's points after all, and the existing steps
        st.fallbacks++;
        st.unresolved += (size_t)es.unresolved;
        pg_result *res = nullptr;
        if ((rc = pg_device_batch_download(ctx, b, &res))) return rc;
        pg_result_view rv;
        pg_result_view_get(res, &rv);
        const bool length_follows = bam;
        pg_adapter::parallel_ranges(n, [&](size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; i++) {
                pg_adapter::apply_rc_flag(reads[i], rv.rc_flag[i]);
                if (length_follows) reads[i].ReadLength = (short)reads[i].UnmatchedSeq.size();
                pg_adapter::fill_points(reads[i].UP_Close, rv.close_runs, rv.close_off[i], rv.close_off[i + 1], make_point);
                pg_adapter::fill_points(reads[i].UP_Far, rv.far_runs, rv.far_off[i], rv.far_off[i + 1], make_point);
            }
        });
        pg_result_free(res);
        s.counts.t_search += now_s() - t0;
        return 1;
    }
};

// -q: searchMEImain (src/search_MEI.cpp:963-1024) over the same plan and windows, after the split-read search.  The reference
// runs it INSTEAD of that search and exits (`exit(searchMEImain(...))`, src/pindel.cpp:1745-1746, its other reports left
// empty); here both run, and _DD does not depend on the order (difference 3).
static int dd_close(pg_ctx *ctx, const pg_adapter::Batch &batch, std::vector<DDClose> &outc)
{
    pg_read_batch v = batch.view();
    pg_result *res = nullptr;
    const int r = pg_close_end_batch(ctx, &v, &res);
    if (r) return r;
    pg_result_view rv;
    pg_result_view_get(res, &rv);
    outc.assign(rv.n_reads, DDClose());
    for (size_t i = 0; i < rv.n_reads; i++) {
        if (rv.close_off[i + 1] == rv.close_off[i]) continue;
        std::vector<UniquePoint> pts;
        pg_adapter::fill_points(pts, rv.close_runs, rv.close_off[i], rv.close_off[i + 1], make_point);
        outc[i].has = 1;
        outc[i].rc_flag = rv.rc_flag[i];
        outc[i].last_abs = pts.back().AbsLoc;
        outc[i].last_len = (uint16_t)pts.back().LengthStr;
    }
    pg_result_free(res);
    return 0;
}

static int dd_contains(pg_ctx *ctx, const std::vector<std::string> &q, const std::vector<int32_t> &chr, const std::vector<uint64_t> &st,
                       const std::vector<uint32_t> &len, std::vector<uint8_t> &found)
{
    std::vector<uint8_t> qs;
    std::vector<uint64_t> qo(1, 0);
    for (const std::string &x : q) {
        qs.insert(qs.end(), x.begin(), x.end());
        qo.push_back(qs.size());
    }
    found.assign(q.size(), 0);
    return pg_dd_contains_batch(ctx, (uint32_t)q.size(), qs.data(), qo.data(), chr.data(), st.data(), len.data(), found.data());
}

// --device-classifier-dd: the breakpoint tables of one window's split reads from the device -- a resident upload, the
// close end alone, pg_device_batch_dd and ONE download of members, candidates and consensus pool.  No point and no consensus crosses
// the bus before the verdicts.
static int dd_device_tables(pg_ctx *ctx, const pg_adapter::Batch &batch, const std::vector<uint32_t> &seg_first, const std::vector<uint8_t> &seg_strand,
                            const DDWindow &w, DDTables &out)
{
    pg_read_batch v = batch.view();
    pg_device_batch *b = nullptr;
    int rc = pg_device_batch_upload(ctx, &v, &b);
    if (rc) return rc;
    struct Free {
        pg_ctx *c;
        pg_device_batch *b;
        ~Free() { pg_device_batch_free(c, b); }
    } free_batch = { ctx, b };
    pg_dd_window dw;
    dw.seg_first = seg_first.data();
    dw.seg_strand = seg_strand.data();
    dw.n_seg = (uint32_t)seg_strand.size();
    dw.chr_id = w.chr_id;
    dw.min_bp_support = w.min_bp_support;
    dw.min_map_distance = w.min_map_distance;
    pg_dd_sizes sz;
    if ((rc = pg_device_batch_close_search(ctx, b)) || (rc = pg_device_batch_dd(ctx, b, &dw)) || (rc = pg_device_batch_dd_sizes(ctx, b, &sz))) return rc;
    out.members.resize((size_t)sz.members);
    out.cands.resize((size_t)sz.cands);
    out.cons.resize((size_t)sz.cons_bytes);
    return pg_device_batch_dd_download(ctx, b, out.members.data(), out.cands.data(), out.cons.data());
}

static int detect_dd(const CliOptions &o, pg_ctx *ctx, const std::vector<Chromosome> &genome, const std::vector<unsigned> &sizes,
                     const std::vector<RegionRecord> &plan, const std::vector<BamSource> &bams, const BamIngestSettings &ing, std::string &err)
{
    if (bams.empty()) {
        // Pindel-text input has no discordant reads: no breakpoint, where the reference ends with std::out_of_range
        std::ofstream((o.prefix + "_DD").c_str(), std::ios::trunc);
        printf("pindel_pg: -q needs BAM input (-i) for discordant read pairs; no dispersed-duplication breakpoint, %s_DD is empty\n", o.prefix.c_str());
        return 0;
    }
    DDStats dst;
    const int rc = run_dd(
        genome, sizes, plan, bams, ing, o.S.window_mbp, o.dd, o.prefix,
        [ctx](int, const pg_adapter::Batch &batch, std::vector<DDClose> &outc) { return dd_close(ctx, batch, outc); },
        [ctx](const std::vector<std::string> &q, const std::vector<int32_t> &chr, const std::vector<uint64_t> &st, const std::vector<uint32_t> &len,
              std::vector<uint8_t> &found) { return dd_contains(ctx, q, chr, st, len, found); },
        err, &dst,
        o.device_classifier_dd ? DDTablesFn([ctx](const pg_adapter::Batch &batch, const std::vector<uint32_t> &seg_first,
                                                  const std::vector<uint8_t> &seg_strand, const DDWindow &w,
                                                  DDTables &out) { return dd_device_tables(ctx, batch, seg_first, seg_strand, w, out); })
                               : DDTablesFn());
    if (rc) return rc;
    printf("pindel_pg: dispersed duplications: %zu discordant reads, %zu clusters, %zu breakpoints, %zu consensus tests "
           "(GPU %.3f s, %zu kept), %zu events\n", dst.discordant, dst.clusters, dst.breakpoints, dst.candidates,
           dst.contains_seconds, dst.kept_by_containment, dst.events);
    if (o.device_classifier_dd)
        printf("pindel_pg: dispersed duplications: %zu windows built from device tables, %zu bytes downloaded for them\n", dst.table_windows,
               dst.table_bytes);
    if (!dst.note.empty()) printf("pindel_pg: %s\n", dst.note.c_str());
    return 0;
}

int main(int argc, char **argv)
{
    const double t_start = now_s();
    CliOptions o;
    pg_default_params(&o.prm);
    std::string err;
    if (parse_cli(argc, argv, o, err)) return fail(err, 2);
    int rc = check_inputs(o);
    if (!rc) rc = create_outputs(o);
    if (rc) return rc;
    std::vector<Chromosome> genome;
    std::vector<unsigned> sizes;
    std::vector<RegionRecord> plan;
    if ((rc = load_genome_and_plan(o, genome, sizes, plan))) return rc;
    if (plan.empty()) {
        printf("pindel_pg: no region left to search (every record of the include list is excluded); the reports are empty\n");
        return 0;
    }
    if (o.S.repairs) printf("pindel_pg: repairs in effect: %s\n", repairs_text(o.S.repairs).c_str());
    for (const RegionRecord &r : plan) printf("Processing region: %s\t%u\t%u\n", genome[r.chr].name.c_str(), r.start, r.end);
    std::vector<SplitRead> all;
    std::vector<BamSource> bams;
    if ((rc = load_reads(o, genome, all, bams))) return rc;
    Devices dev;
    if ((rc = dev.open(o, genome))) return rc;
    pg_ctx *ctx = dev.ctxs[0];
    o.S.spacer = o.prm.spacer;
    o.S.log_counts = true;
    pg_get_max_mismatch(ctx, o.S.max_mismatch);
    const double t_loaded = now_s();
    BDHints bd;
    if ((rc = load_hints(o, bd))) return rc;
    BamIngestSettings ing;                 // -A, -n, -u: the split-read selection of the main search and of -q
    ing.min_anchor_quality = o.min_anchor_quality;
    ing.spacer = o.prm.spacer;
    ing.nm = o.ref_read_nm;
    ing.max_mismatch_rate = o.prm.max_allowed_mismatch_rate;
    RunCounts counts;
    // BAM input: with -R (default) the window hints are live -- the events of a -b file plus the read-pair events of
    // every window; without -R the reference never hands any event to the search (UpdateBD is not called)
    const Seams seams = { o, dev.ctxs, bd, bams.empty() ? o.use_bd : o.search_rp, chromosome_names(genome), counts };
    size_t n_reads = all.size(), n_rp_events = 0;
    double li_seconds = 0.0;
    DeviceClassifierStats dc_stats;
    DeviceClassify device_classify;
    if (o.device_classifier) device_classify = DeviceClassifier{ seams, dc_stats, !bams.empty(), int_chr_ranks(seams.chr_names) };
    if (!bams.empty()) {
        n_reads = 0;
        rc = run_bam_pipeline(genome, plan, bams, ing, o.S, o.prefix, CloseSoa{ seams }, FarSearch{ seams }, err, &n_reads, &bd, o.search_rp,
                              &n_rp_events, &li_seconds, device_classify);
        if (o.search_rp) printf("pindel_pg: read-pair events added as window hints: %zu\n", n_rp_events);
    } else
        rc = run_pipeline(genome, plan, all, o.S, o.prefix, CloseSearch{ seams }, FarSearch{ seams }, err, &li_seconds, WindowPairs(),
                          device_classify);
    if (!rc && o.detect_dd) rc = detect_dd(o, ctx, genome, sizes, plan, bams, ing, err);
    if (rc) {
        fprintf(stderr, "pindel_pg: %s (%s)\n", err.c_str(), pg_last_error(ctx));
        return 1;
    }
    if (o.S.only_close_mapped)
        printf("pindel_pg: %zu reads, close end %zu (-S: close-end-mapped reads only, no far-end search)\n", n_reads, counts.n_close);
    else
        printf("pindel_pg: %zu reads, close end %zu, far end %zu\n", n_reads, counts.n_close, counts.n_far);
    if (o.device_classifier) {
        printf("pindel_pg: device classifier: %zu windows, %zu from tables, %zu fell back, %zu unresolved reads, %zu report records, "
               "%zu runs not downloaded", dc_stats.windows, dc_stats.from_tables, dc_stats.fallbacks, dc_stats.unresolved, dc_stats.records,
               dc_stats.runs_kept);
        if (o.device_classifier_hints) printf(", %zu hinted windows", dc_stats.hinted);
        if (o.device_classifier_li) printf(", %zu windows with LI tables", dc_stats.li_windows);
        if (o.device_classifier_int) printf(", %zu windows with junction tables", dc_stats.int_windows);
        printf("\n");
    }
    // the phases the reference's Timer reports (pindel.cpp:1990-1996), wall-clock seconds
    printf("pindel_pg: loading %.2f s, split-read search (GPU, incl. adapters) %.2f s, classification + reports %.2f s\n",
           t_loaded - t_start, counts.t_search, now_s() - t_loaded - counts.t_search);
    if (o.S.Analyze_LI && !o.S.only_close_mapped)
        printf("pindel_pg: long insertions (_LI, host, part of classification + reports) %.3f s\n", li_seconds);
    if (o.device_classifier_li && o.S.Analyze_LI)
        printf("pindel_pg: long-insertion tables downloaded: %zu bytes for %zu reads\n", dc_stats.li_bytes, n_reads);
    if (o.device_classifier_int && o.S.report_interchromosomal)
        printf("pindel_pg: junction tables downloaded: %zu bytes for %zu reads\n", dc_stats.int_bytes, n_reads);
    return 0;
}
