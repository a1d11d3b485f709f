// pg_pipeline.hpp -- main()'s chromosome / 5-Mbp-bin loop (src/pindel.cpp:1778-1989) around a
// pluggable search step.  Shared by the pindel_pg command line (search = GPU through the C ABI)
// and by pgh_call_from_points (search = attach externally computed points, used by the tests).
#ifndef PG_PIPELINE_HPP
#define PG_PIPELINE_HPP

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <future>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "pg_bam.hpp"
#include "pg_bdhints.hpp"
#include "pg_depth.hpp"
#include "pg_host.hpp"
#include "pg_region.hpp"
#include "pg_rp.hpp"

namespace pgh {

// .fai sizes (init_g_ChrNameAndSizeAndIndex, pindel.cpp:1332-1348); 0 when absent
inline std::vector<unsigned> read_fai(const std::string &fasta_path, const std::vector<Chromosome> &genome)
{
    std::vector<unsigned> fai(genome.size(), 0);
    std::ifstream f((fasta_path + ".fai").c_str());
    std::string name, rest;
    unsigned size;
    while (f >> name >> size) {
        std::getline(f, rest);
        for (size_t c = 0; c < genome.size(); c++)
            if (genome[c].name == name) fai[c] = size;
    }
    return fai;
}

// The chromosome sizes of the region plan: the .fai length, or the FASTA length without one
inline std::vector<unsigned> chromosome_sizes(const std::vector<Chromosome> &genome, const std::vector<unsigned> &fai, unsigned spacer)
{
    std::vector<unsigned> sizes(genome.size());
    for (size_t c = 0; c < genome.size(); c++) sizes[c] = fai[c] ? fai[c] : (unsigned)(genome[c].seq.size() - 2 * spacer);
    return sizes;
}

inline std::vector<std::string> chromosome_names(const std::vector<Chromosome> &genome)
{
    std::vector<std::string> names;
    for (const Chromosome &c : genome) names.push_back(c.name);
    return names;
}

// Frees the strings and point lists of a window's reads on several threads (the destructors of ~10^7 reads are
// seconds of single-threaded work otherwise); the vector itself is left empty.
inline void release_reads(std::vector<SplitRead> &v)
{
    pg_adapter::parallel_ranges(v.size(), [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) {
            SplitRead gone;
            std::swap(gone, v[i]);
        }
    });
    std::vector<SplitRead>().swap(v);
}

// The end of a run with the germline filter: its PGH_TIMING figure, and a BAM it could not read is the run's error
inline int germline_done(const Settings &S, bool timing, std::string &err)
{
    if (!S.germline_filter()) return 0;
    if (timing)
        fprintf(stderr, "pgh timing: germline filter %.3f s (read depth of %zu BAM regions, summed over the reporter threads)\n",
                S.germline->seconds(), S.germline->queries());
    if (!S.germline->error().empty()) {
        err = "germline filter: " + S.germline->error();
        return -1;
    }
    return 0;
}

// --repair inv-pairs: what IsGoodINV reads of the pairs rp_events left (pg_rp.hpp)
inline std::vector<DiscordantPair> discordant_pairs(const std::vector<RpRead> &left)
{
    std::vector<DiscordantPair> out;
    out.reserve(left.size());
    for (const RpRead &r : left) {
        DiscordantPair p = { r.DA, r.DB, r.PosA, r.PosB, (unsigned)r.InsertSize, r.ReadLength };
        out.push_back(p);
    }
    return out;
}

// Read-pair events as BDHints::update_with_rp takes them: the two sides of each
inline std::vector<std::pair<BDHints::RpSide, BDHints::RpSide>> rp_sides(const std::vector<RpEvent> &ev)
{
    std::vector<std::pair<BDHints::RpSide, BDHints::RpSide>> sides;
    sides.reserve(ev.size());
    for (const RpEvent &e : ev) {
        BDHints::RpSide a = { e.chr1, e.pos1, e.pos1b }, b = { e.chr2, e.pos2, e.pos2b };
        sides.push_back(std::make_pair(a, b));
    }
    return sides;
}

// The same-chromosome discordant pairs of window [ws, we) of `chr_name` over all BAMs, for a pipeline that does not
// discover them anyway: discovery and UpdateBD's steps, no event kept, no _RP line.  false: a BAM read failed.
inline bool window_pairs(std::vector<BamFile> &files, const std::vector<int> &insert_sizes, const std::vector<std::string> &tags,
                         const std::string &chr_name, unsigned ws, unsigned we, unsigned min_anchor_quality, unsigned spacer,
                         std::vector<DiscordantPair> &out)
{
    std::vector<RpRead> rp, left;
    for (size_t k = 0; k < files.size(); k++)
        if (!rp_discover(files[k], chr_name, ws, we, insert_sizes[k], tags[k], min_anchor_quality, rp)) return false;
    rp_events(rp, spacer, nullptr, &left);
    out = discordant_pairs(left);
    return true;
}

// The two seams, in the reference's order (src/pindel.cpp:1816-1888):
//   search(chrom, chr_id, reads, index_in_all)   on ALL reads of the window: must fill UP_Close (empty when there is no
//                                                close end) and leave UnmatchedSeq as GetCloseEnd would
//                                                (ReadBuffer::flush, src/read_buffer.cpp:36-101); may fill UP_Far too
//   far_search(chrom, chr_id, kept, ws, we)      on the reads that kept a close end (state.Reads_SR): fills UP_Far
//                                                (SearchFarEnds, src/pindel.cpp:1115-1138, called at :1888); [ws, we) =
//                                                the window being processed, biological coordinates (currentWindow,
//                                                src/pindel.cpp:1828: what g_bdData.loadRegion is given at :1853)
// With S.close_mapped_output() the reads that kept a close end are written to <prefix>_CloseEndMapped before the far end
// (src/pindel.cpp:1880-1883); with S.only_close_mapped (-S) that is all: no far end, no classifiers, no reports.
// li_seconds (nullable) receives the host time of the _LI reporter over all windows.
// pairs_of(chrom, ws, we, pairs) (may be empty): the window's discordant pairs for --repair inv-pairs, asked for every
// window that is classified; false = a BAM could not be read.
typedef std::function<bool(const Chromosome &, unsigned, unsigned, std::vector<DiscordantPair> &)> WindowPairs;
// --device-classifier: one window on the device.  classify(chrom, chr_id, reads, ws, we, bed_start, bed_end, caller,
// after_close) is given ALL reads of the window as loaded and runs upload, fused search, pg_device_batch_classify and the downloads.
//   0    the reports are written (Caller::process_window_from_tables); after_close (may be empty) was called once the summaries
//        were applied to the reads and before anything was written
//   1    the window fell back: the reads now carry UP_Close, UP_Far and the sequence as GetCloseEnd left it, and go on through the
//        existing steps, the far-end search excepted
//   < 0  a pg status
// Either way it has printed the far-end step's line and counted the window's close and far ends.
typedef std::function<int(const Chromosome &, int, std::vector<SplitRead> &, unsigned, unsigned, unsigned, unsigned, Caller &,
                          const std::function<void()> &)> DeviceClassify;
struct NoFarSearch {
    int operator()(const Chromosome &, int, std::vector<SplitRead> &, unsigned, unsigned) const { return 0; }
};

// Both pipelines walk a region plan (pg_region.hpp) record by record, in plan order (main's IncludeBed loop,
// src/pindel.cpp:1777-1987): record [S, E] on chromosome c is searched in windows from S - 10 kbp in steps of -w, each
// ending at min(start + W, biological size, E + 10 kbp), and its calls are restricted to [S, E] (readInSpecifiedRegion).
// A read in the windows of two records is searched and reported in both, as in the reference.  CurrentChrMask starts
// empty at every record; Count_LI, g_maxInsertSize, the event numbers and the _RP stream run on across records.
// Under -j the reference also calls ControlState::CleanUPReads at every record.  That has no effect here: the reference
// clears the same vectors at the end of every window (pindel.cpp:1962-1968), and so do these loops (reads, kept reads,
// read-pair events and reference-supporting reads all live for one window only).
template <class Search, class FarSearch>
int run_pipeline(const std::vector<Chromosome> &genome, const std::vector<RegionRecord> &plan,
                 const std::vector<SplitRead> &all, const Settings &S, const std::string &prefix,
                 Search search, FarSearch far_search, std::string &err, double *li_seconds = nullptr,
                 const WindowPairs &pairs_of = WindowPairs(), const DeviceClassify &device_classify = DeviceClassify())
{
    Caller caller(S, &genome, prefix, true);
    const unsigned WINDOW = (unsigned)(S.window_mbp * 1000000);
    if (WINDOW == 0) {
        err = "window size (-w) must be at least 0.000001 Mbp";
        return -1;
    }
    // PGH_TIMING=1: wall-clock seconds per stage of this loop on stderr (diagnostics)
    const bool timing = getenv("PGH_TIMING") != nullptr;
    double t_copy = 0, t_search = 0, t_keep = 0, t_call = 0, t_free = 0;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    // The Pindel-text reader rescans the whole file for every window and raises g_maxPos for EVERY read it
    // passes (reader.cpp:224-226), so after the first window of a record g_maxPos is the largest position
    // in the file; the windows then run until they pass it.  Here the reads are sorted once: per chromosome
    // the indices of its reads by position (input order among equal positions); a record takes the range of
    // its windows from that list and bins it by window, in input order, instead of one pass over all reads
    // per window.
    unsigned file_max_pos = 0;
    std::vector<std::vector<uint32_t>> by_chr(genome.size());
    for (uint32_t i = 0; i < all.size(); i++) {
        file_max_pos = std::max(file_max_pos, all[i].MatchedRelPos);
        if (all[i].chr_id >= 0 && all[i].chr_id < (int)genome.size()) by_chr[all[i].chr_id].push_back(i);
    }
    for (std::vector<uint32_t> &v : by_chr)
        if (!std::is_sorted(v.begin(), v.end(), [&](uint32_t a, uint32_t b) { return all[a].MatchedRelPos < all[b].MatchedRelPos; }))
            std::stable_sort(v.begin(), v.end(), [&](uint32_t a, uint32_t b) { return all[a].MatchedRelPos < all[b].MatchedRelPos; });
    for (const RegionRecord &rec : plan) {
        const size_t c = (size_t)rec.chr;
        const Chromosome &chrom = genome[c];
        const unsigned biol = (unsigned)(chrom.seq.size() - 2 * S.spacer);
        const unsigned bed_start = rec.start, bed_end = rec.end;
        const unsigned global_start = region_global_start(rec), global_end = region_global_end(rec, biol);
        caller.begin_region();
        // windows that will be visited: ws = G, G + W, ... while !(ws >= g_maxPos || ws > global_end), at least one
        std::vector<unsigned> starts;
        {
            uint64_t ws = global_start;
            do {
                starts.push_back((unsigned)ws);
                ws += WINDOW;
            } while (!(ws >= file_max_pos || ws > global_end));
        }
        std::vector<std::vector<uint32_t>> bins(starts.size());
        {
            const std::vector<uint32_t> &v = by_chr[c];
            auto first = std::lower_bound(v.begin(), v.end(), global_start,
                                          [&](uint32_t i, unsigned p) { return all[i].MatchedRelPos < p; });
            for (auto it = first; it != v.end() && all[*it].MatchedRelPos < global_end; ++it) {
                const unsigned pos = all[*it].MatchedRelPos;
                const size_t w = (pos - global_start) / WINDOW;
                // a read is picked up by window w iff ws <= pos < min(ws + W, global_end)
                if (w < starts.size() && (uint64_t)pos < std::min<uint64_t>((uint64_t)starts[w] + WINDOW, global_end)) bins[w].push_back(*it);
            }
            for (std::vector<uint32_t> &b : bins)                                      // input order
                if (!std::is_sorted(b.begin(), b.end())) std::sort(b.begin(), b.end());
        }
        for (size_t w = 0; w < starts.size(); w++) {
            if (bins[w].empty()) continue;
            const unsigned ws = starts[w], we = (unsigned)std::min<uint64_t>((uint64_t)ws + WINDOW, global_end);
            double t0 = now();
            std::vector<SplitRead> reads(bins[w].size());
            pg_adapter::parallel_ranges(reads.size(), [&](size_t lo, size_t hi) {
                for (size_t k = lo; k < hi; k++) {
                    const uint32_t i = bins[w][k];
                    reads[k] = all[i];
                    if (reads[k].MatchedRelPos > biol) reads[k].MatchedRelPos = biol;   // reader.cpp:233-235
                    reads[k].MAX_SNP_ERROR = (short)S.max_mismatch[std::min<int>(all[i].ReadLength, 499)];
                }
            });
            t_copy += now() - t0; t0 = now();
            int rc = 0;
            bool far_done = false;
            if (device_classify) {
                for (const SplitRead &r : reads) caller.note_insert_size(r.InsertSize);
                rc = device_classify(chrom, (int)c, reads, ws, we, bed_start, bed_end, caller, std::function<void()>());
                if (rc < 0) {
                    err = "device classifier step failed";
                    return rc;
                }
                if (rc == 0) {                                              // written from tables
                    t_call += now() - t0; t0 = now();
                    release_reads(reads);
                    t_free += now() - t0;
                    continue;
                }
                far_done = true;
            } else if ((rc = search(chrom, (int)c, reads, bins[w]))) {
                err = "search step failed";
                return rc;
            }
            t_search += now() - t0; t0 = now();
            for (const SplitRead &r : reads) caller.note_insert_size(r.InsertSize);
            caller.note_close_mapped_all(reads);                        // reader.cpp:258-291
            std::vector<SplitRead> kept;
            {
                size_t n_kept = 0;
                for (const SplitRead &r : reads) n_kept += r.UP_Close.empty() ? 0 : 1;
                kept.reserve(n_kept);
            }
            for (SplitRead &r : reads)
                if (!r.UP_Close.empty()) kept.push_back(std::move(r));      // `reads` is not used after this loop
            if (S.close_mapped_output() && !S.close_mapped_by_window() && !kept.empty()) caller.report_close_mapped(kept);
            t_keep += now() - t0; t0 = now();
            if (!S.only_close_mapped && !kept.empty() && !far_done && (rc = far_search(chrom, (int)c, kept, ws, we))) {
                err = "far-end search step failed";
                return rc;
            }
            t_search += now() - t0; t0 = now();
            if (pairs_of && !S.only_close_mapped && !kept.empty()) {
                std::vector<DiscordantPair> pairs;
                if (!pairs_of(chrom, ws, we, pairs)) {
                    err = "BAM read failed during the read-pair discovery of --repair inv-pairs";
                    return -1;
                }
                caller.set_window_pairs(std::move(pairs));
            }
            if (!S.only_close_mapped && !kept.empty()) caller.process_window(chrom, kept, ws, we, bed_start, bed_end);
            t_call += now() - t0; t0 = now();
            release_reads(kept);
            release_reads(reads);
            t_free += now() - t0;
        }
    }
    if (timing)
        fprintf(stderr, "pgh timing: pipeline: copy reads %.3f s, search step %.3f s, keep %.3f s, classify + report %.3f s, free %.3f s\n",
                t_copy, t_search, t_keep, t_call, t_free);
    if (li_seconds) *li_seconds = caller.li_seconds;
    return germline_done(S, timing, err);
}

// BAM input (`-i config`): main()'s loop with get_SR_Reads per window (src/pindel.cpp:1816-1982,
// src/reader.cpp:1427-1470).  The windows of each plan record run from its global start in steps of the bin size
// while the start does not pass the record's global end (LoopingSearchWindow::finished without the Pindel-text
// shortcut); every window reads
// its candidates from every BAM of the configuration through pg_bam.hpp, so only one window's reads are in
// memory at a time (a coordinate-sorted BAM delivers them bin by bin).
struct BamSource {
    std::string path, tag;
    int insert_size = 0;
};

// -i: one line per BAM: file, insert size, sample tag (readBamConfigFile, src/pindel.cpp); a relative file name is relative to
// the configuration file.  false: the file cannot be read or lists no BAM (err says which).
inline bool read_bam_config(const std::string &config, std::vector<BamSource> &bams, std::string &err)
{
    std::ifstream cf(config.c_str());
    if (!cf) {
        err = "cannot open " + config;
        return false;
    }
    BamSource b;
    while (cf >> b.path >> b.insert_size >> b.tag) {
        if (b.path[0] != '/') {
            const size_t sl = config.rfind('/');
            if (sl != std::string::npos) b.path = config.substr(0, sl + 1) + b.path;
        }
        bams.push_back(b);
    }
    if (bams.empty()) {
        err = "no BAM files in " + config;
        return false;
    }
    return true;
}

// -N: the BAMs of the configuration as the germline filter measures them (pg_depth.hpp); null with err set when one
// cannot be opened.  repairs: with REPAIR_DEPTH_MAPQ the depth counts records of MAPQ >= 20 only.
inline std::shared_ptr<const GermlineDepth> open_germline(const std::vector<BamSource> &bams, std::string &err, uint32_t repairs = 0)
{
    std::vector<std::string> paths, tags;
    for (const BamSource &b : bams) {
        paths.push_back(b.path);
        tags.push_back(b.tag);
    }
    std::shared_ptr<GermlineDepth> g(new GermlineDepth());
    if (!g->open(paths, tags, err, (repairs & REPAIR_DEPTH_MAPQ) ? (unsigned)DEPTH_MAPQ_FLOOR : 0u)) return nullptr;
    return g;
}

// The close end of one window of the BAM path, straight on the ingested structure-of-arrays batch (no SplitRead per
// candidate): what comes back per contiguous part of the batch (one part per device).
struct ClosePart {
    size_t first = 0, n = 0;              // reads [first, first + n) of the batch
    const uint8_t *rc_flag = nullptr;     // per read of the part
    const uint64_t *close_off = nullptr;  // n + 1 offsets into close_runs
    const pg_run *close_runs = nullptr;
};
struct CloseView {
    std::vector<ClosePart> parts;
    std::function<void()> release;        // frees what the pointers point into
};

// bd != null && search_rp: before the reads of a window are taken, its discordant read pairs become BreakDancer-like
// events (get_RP_Reads_Discovery + BDData::UpdateBD, src/pindel.cpp:1838-1848; -R, default on) next to the events of
// a -b file; the search step then looks their windows up per read (loadRegion / getCorrespondingSearchWindowCluster).
// With S.report_interchromosomal (-I) the pairs whose mates lie on different chromosomes are kept and clustered as
// well (rp_events_interchr): their events and _RP lines follow the window's same-chromosome ones, as in UpdateBD.
//
//   close_soa(chrom, chr_id, batch, view)   ReadBuffer::flush on the window's candidates as ingested (SoA): the close
//                                           ends as run lists + rc flags; only the reads that have one become SplitReads
//                                           (UnmatchedSeq reverse-complemented where GetCloseEnd did, UP_Close filled)
//   far_search(chrom, chr_id, kept, ws, we) SearchFarEnds on those reads; [ws, we) = the window (for the hints' loadRegion)
//
// The windows are a three-stage pipeline on the host: while window k is searched and classified, a second thread
// already reads window k + 1 from the BAMs (read-pair discovery + ingest, the stage that dominates a BAM-fed run).
template <class CloseSoa, class FarSearch>
int run_bam_pipeline(const std::vector<Chromosome> &genome, const std::vector<RegionRecord> &plan,
                     const std::vector<BamSource> &bams, const BamIngestSettings &ingest, const Settings &S,
                     const std::string &prefix, CloseSoa close_soa, FarSearch far_search, std::string &err, size_t *n_reads_total = nullptr,
                     BDHints *bd = nullptr, bool search_rp = false, size_t *n_rp_events = nullptr,
                     double *li_seconds = nullptr, const DeviceClassify &device_classify = DeviceClassify())
{
    Caller caller(S, &genome, prefix, true);
    std::ofstream rp_out;
    if (bd && search_rp) rp_out.open((prefix + "_RP").c_str(), std::ios::trunc);
    const unsigned WINDOW = (unsigned)(S.window_mbp * 1000000);
    if (WINDOW == 0) {
        err = "window size (-w) must be at least 0.000001 Mbp";
        return -1;
    }
    std::vector<BamFile> files(bams.size());
    for (size_t k = 0; k < bams.size(); k++)
        if (!files[k].open(bams[k].path, err)) return -1;
    // PGH_TIMING=1: wall-clock seconds per stage of this loop on stderr (diagnostics)
    const bool timing = getenv("PGH_TIMING") != nullptr;
    double t_wait = 0, t_close = 0, t_keep = 0, t_far = 0, t_cov = 0, t_call = 0, t_free = 0;
    double t_rp = 0, t_rp_inter = 0, t_ingest = 0;         // (on the reader thread; t_rp_inter: the -I clustering, part of t_rp)
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_begin = now();

    // the windows of every plan record, in plan order (LoopingSearchWindow::finished without the Pindel-text shortcut);
    // rec: the record's index in the plan, first: the record's first window
    struct Win { size_t c, rec; unsigned ws, we; bool first; };
    std::vector<Win> wins;
    for (size_t k = 0; k < plan.size(); k++) {
        const size_t c = (size_t)plan[k].chr;
        const unsigned biol = (unsigned)(genome[c].seq.size() - 2 * S.spacer);
        const unsigned global_end = region_global_end(plan[k], biol);
        for (uint64_t ws = region_global_start(plan[k]); !(ws > global_end); ws += WINDOW)
            wins.push_back({ c, k, (unsigned)ws, (unsigned)std::min<uint64_t>(ws + WINDOW, global_end), ws == region_global_start(plan[k]) });
    }
    // what the reader thread hands over for one window
    struct WinData {
        IngestedReads in;
        std::vector<std::pair<BDHints::RpSide, BDHints::RpSide>> sides;   // read-pair events of the window
        std::vector<DiscordantPair> pairs;                                // --repair inv-pairs: its same-chromosome pairs
        size_t n_events = 0;
        std::string error;
    };
    // (only this function touches `files` and `rp_out`, one window at a time, in window order)
    auto read_win = [&](size_t w) {
        std::unique_ptr<WinData> d(new WinData());
        const Win &win = wins[w];
        const Chromosome &chrom = genome[win.c];
        double t0 = now();
        // --repair inv-pairs under -N: the pairs are discovered with -R false too, for the filter alone (no hint, no _RP line)
        const bool hints = bd && search_rp;
        const bool inv_pairs = S.germline_filter() && S.repair(REPAIR_INV_PAIRS) && S.Analyze_INV && !S.only_close_mapped;
        if (hints || inv_pairs) {
            std::vector<RpRead> rp, rp_inter, left;
            for (size_t k = 0; k < bams.size(); k++)
                if (!rp_discover(files[k], chrom.name, win.ws, win.we, bams[k].insert_size, bams[k].tag, ingest.min_anchor_quality, rp,
                                 hints && S.report_interchromosomal ? &rp_inter : nullptr)) {
                    d->error = bams[k].path + ": BAM read failed";
                    return d;
                }
            std::vector<RpEvent> ev = rp_events(rp, S.spacer, hints ? &rp_out : nullptr, inv_pairs ? &left : nullptr);
            if (inv_pairs) d->pairs = discordant_pairs(left);
            if (!hints) ev.clear();
            if (hints && S.report_interchromosomal) {
                const double t1 = now();
                const std::vector<RpEvent> inter = rp_events_interchr(rp_inter, S.spacer, &rp_out);
                ev.insert(ev.end(), inter.begin(), inter.end());
                t_rp_inter += now() - t1;
            }
            d->sides = rp_sides(ev);
            d->n_events = ev.size();
        }
        t_rp += now() - t0; t0 = now();
        d->in.clear();
        BamIngest ing(ingest);
        for (size_t k = 0; k < bams.size(); k++)
            if (!ing.read_window(files[k], chrom.name, (int)win.c, chrom.seq.size(), win.ws, win.we, bams[k].insert_size, bams[k].tag, d->in)) {
                d->error = bams[k].path + ": " + ing.error;
                return d;
            }
        t_ingest += now() - t0;
        return d;
    };
    std::future<std::unique_ptr<WinData>> ahead;
    std::future<void> trash;
    if (!wins.empty()) ahead = std::async(std::launch::async, read_win, (size_t)0);
    int status = 0;
    for (size_t w = 0; w < wins.size(); w++) {
        double t0 = now();
        std::unique_ptr<WinData> d = ahead.get();
        if (w + 1 < wins.size() && d->error.empty()) ahead = std::async(std::launch::async, read_win, w + 1);
        t_wait += now() - t0; t0 = now();
        if (!d->error.empty()) {
            err = d->error;
            return -1;
        }
        const Win &win = wins[w];
        const size_t c = win.c;
        const Chromosome &chrom = genome[c];
        const unsigned bed_start = plan[win.rec].start, bed_end = plan[win.rec].end;
        if (win.first) caller.begin_region();
        if (bd && search_rp) {
            bd->update_with_rp(d->sides);
            if (n_rp_events) *n_rp_events += d->n_events;
        }
        IngestedReads &in = d->in;
        if (n_reads_total) *n_reads_total += in.size();
        if (in.size() == 0) continue;
        for (size_t i = 0; i < in.size(); i++) caller.note_insert_size(in.batch.isz[i]);
        auto ref_coverage = [&]() {   // UpdateRefReadCoverage, after the close ends (sample names) and before the classifiers
            std::vector<Caller::RefReadSpan> spans(in.ref_reads.size());
            for (size_t i = 0; i < spans.size(); i++) {
                spans[i].pos = in.ref_reads[i].pos;
                spans[i].length = in.ref_reads[i].length;
                spans[i].tag = in.ref_reads[i].tag;
            }
            caller.update_ref_coverage(spans, in.ref_tags, win.ws, win.we);
        };
        int rc = 0;
        std::vector<SplitRead> kept;
        bool far_done = false;
        if (device_classify) {
            // every candidate of the window as a SplitRead as ingested: no close end yet, the sequence as it came
            std::vector<SplitRead> reads(in.size());
            pg_adapter::parallel_ranges(reads.size(), [&](size_t lo, size_t hi) {
                for (size_t i = lo; i < hi; i++) {
                    SplitRead &r = reads[i];
                    r.Name = in.names[i];
                    r.UnmatchedSeq.assign((const char *)in.batch.seq.data() + in.batch.off[i], (size_t)(in.batch.off[i + 1] - in.batch.off[i]));
                    r.ReadLength = (short)r.UnmatchedSeq.size();
                    r.MatchedD = (char)in.batch.strand[i];
                    r.MatchedRelPos = (unsigned)in.batch.pos[i];
                    r.MS = in.ms[i];
                    r.InsertSize = in.batch.isz[i];
                    r.Tag = in.tags[i];
                    r.FragName = chrom.name;
                    r.chr_id = (int)c;
                }
            });
            rc = device_classify(chrom, (int)c, reads, win.ws, win.we, bed_start, bed_end, caller, ref_coverage);
            if (rc < 0) {
                err = "device classifier step failed";
                status = rc;
                break;
            }
            t_call += now() - t0; t0 = now();
            if (rc == 0) continue;                            // written from tables
            for (SplitRead &r : reads)
                if (!r.UP_Close.empty()) {
                    r.MAX_SNP_ERROR = (short)S.max_mismatch[std::min<int>(r.ReadLength, 499)];
                    kept.push_back(std::move(r));
                }
            far_done = true;
        } else {
        CloseView view;
        rc = close_soa(chrom, (int)c, in.batch, view);
        if (rc) {
            err = "search step failed";
            status = rc;
            break;
        }
        t_close += now() - t0; t0 = now();
        // the reads that kept a close end (ReadBuffer::flush, src/read_buffer.cpp:55-64), in input order
        std::vector<uint32_t> kept_idx;
        std::vector<const ClosePart *> kept_part;
        for (const ClosePart &p : view.parts)
            for (size_t i = 0; i < p.n; i++)
                if (p.close_off[i + 1] > p.close_off[i]) {
                    kept_idx.push_back((uint32_t)(p.first + i));
                    kept_part.push_back(&p);
                }
        kept.resize(kept_idx.size());
        pg_adapter::parallel_ranges(kept.size(), [&](size_t lo, size_t hi) {
            for (size_t k = lo; k < hi; k++) {
                const size_t i = kept_idx[k];
                const ClosePart &p = *kept_part[k];
                const size_t j = i - p.first;
                SplitRead &r = kept[k];
                r.Name = in.names[i];
                r.UnmatchedSeq.assign((const char *)in.batch.seq.data() + in.batch.off[i], (size_t)(in.batch.off[i + 1] - in.batch.off[i]));
                pg_adapter::apply_rc_flag(r, p.rc_flag[j]);                        // setUnmatchedSeq(RC), pindel.cpp:2545 (once or twice)
                r.ReadLength = (short)r.UnmatchedSeq.size();
                r.MatchedD = (char)in.batch.strand[i];
                r.MatchedRelPos = (unsigned)in.batch.pos[i];
                r.MS = in.ms[i];
                r.InsertSize = in.batch.isz[i];
                r.Tag = in.tags[i];
                r.FragName = chrom.name;
                r.chr_id = (int)c;
                r.MAX_SNP_ERROR = (short)S.max_mismatch[std::min<int>(r.ReadLength, 499)];
                pg_adapter::fill_points(r.UP_Close, p.close_runs, p.close_off[j], p.close_off[j + 1],
                                        [](const pg_point &q) { return to_unique_point(q); });   // (a lambda, not the function's address: inlined)
            }
        });
        if (view.release) view.release();
        }
        caller.note_close_mapped_all(kept);
        if (S.close_mapped_output() && !S.close_mapped_by_window() && !kept.empty()) caller.report_close_mapped(kept);
        t_keep += now() - t0; t0 = now();
        if (!S.only_close_mapped && !kept.empty() && !far_done && (rc = far_search(chrom, (int)c, kept, win.ws, win.we))) {
            err = "far-end search step failed";
            status = rc;
            break;
        }
        t_far += now() - t0; t0 = now();
        if (!S.only_close_mapped) ref_coverage();
        t_cov += now() - t0; t0 = now();
        caller.set_window_pairs(std::move(d->pairs));
        if (!S.only_close_mapped && !kept.empty()) caller.process_window(chrom, kept, win.ws, win.we, bed_start, bed_end);
        t_call += now() - t0; t0 = now();
        // the window's reads are freed behind the next window's work (one disposal in flight)
        if (trash.valid()) trash.wait();
        {
            std::shared_ptr<std::vector<SplitRead>> dead_reads(new std::vector<SplitRead>(std::move(kept)));
            std::shared_ptr<WinData> dead_win(d.release());
            trash = std::async(std::launch::async, [dead_reads, dead_win]() mutable {
                release_reads(*dead_reads);
                dead_reads.reset();
                dead_win.reset();
            });
        }
        t_free += now() - t0;
    }
    if (ahead.valid()) ahead.wait();                      // (an early exit must not leave the reader running on dead objects)
    if (trash.valid()) trash.wait();
    if (timing)
        fprintf(stderr, "pgh timing: BAM pipeline %.3f s wall: waiting for the reader %.3f s, close end %.3f s, keep + SplitReads %.3f s, "
                        "far end %.3f s, reference coverage %.3f s, classify + report %.3f s, free %.3f s | reader thread: read-pair "
                        "discovery %.3f s (of which interchromosomal clustering %.3f s), ingest %.3f s (inflate + decode on threads %.3f, "
                        "selection rules on threads %.3f, layout %.3f)\n",
                now() - t_begin, t_wait, t_close, t_keep, t_far, t_cov, t_call, t_free, t_rp, t_rp_inter, t_ingest,
                ingest_timing().inflate_decode, ingest_timing().select, ingest_timing().layout);
    if (li_seconds) *li_seconds = caller.li_seconds;
    const int grc = germline_done(S, timing, err);
    return status ? status : grc;
}

}  // namespace pgh
#endif
