// pg_host.hpp -- C++ host side around the split-read search: the reference's data
// model (SPLIT_READ, UniquePoint, Chromosome), its text/FASTA loaders, the SV
// classifiers and the text reporters that consume UP_Close / UP_Far.
//
// This mirrors the reference's interface for the steps either side of the hot path
//  so that breakpoint calls can be compared byte for
// byte with the reference's golden files:
//   loaders      Genome::loadChromosome src/pindel.cpp:272-312, PindelReadReader
//                src/pindel_read_reader.cpp:53-66, ReadInRead src/reader.cpp:196-361
//   classifiers  SearchVariant::Search src/search_variant.cpp:48-266 (+ searchdeletions.cpp,
//                searchshortinsertions.cpp), searchIndels src/search_deletions_nt.cpp:26-140
//   reporters    SortOutputD / OutputDeletions, SortOutputDI / OutputDI, SortOutputSI /
//                OutputSIs  src/reporter.cpp; SortOutputLI src/reporter.cpp:1853-2141 and
//                ReportCloseMappedReads src/pindel.cpp:1076-1092 (pg_host_li.cpp);
//                SortAndReportInterChromosomalEvents src/reporter.cpp:2428-2665 and MergeInterChr
//                src/pindel.cpp:1514-1579 (pg_host_int.cpp)
// The search itself is NOT here: UP_Close / UP_Far come from the GPU through the C ABI
// (include/pindel_pg.h, of which this file uses the plain C types).  No HIP dependency in this file; plain g++.
#ifndef PG_HOST_HPP
#define PG_HOST_HPP

#include <algorithm>
#include <cstdint>
#include <map>
#include <memory>
#include <set>
#include <fstream>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "pindel_pg.h"

namespace pgh {

struct UniquePoint {              // src/pindel.h:137-158
    int chr = -1;
    short LengthStr = 0;
    unsigned AbsLoc = 0;
    char Direction = 'N';         // '+' FORWARD, '-' BACKWARD
    char Strand = 'N';            // '+' SENSE, '-' ANTISENSE
    short Mismatches = 0;
};

// A point of the C ABI as the classifiers read it (inline: it runs per point of every read that has a close end)
inline UniquePoint to_unique_point(const pg_point &p)
{
    UniquePoint u;
    u.chr = p.chr_id;
    u.LengthStr = p.length;
    u.AbsLoc = p.abs_loc;
    u.Direction = p.direction;
    u.Strand = p.strand;
    u.Mismatches = p.mismatches;
    return u;
}

struct SplitRead {                // the SPLIT_READ fields used downstream, src/pindel.h:265-383
    std::string Name, UnmatchedSeq, FragName, FarFragName, Tag, NT_str;
    char MatchedD = 0, MatchedFarD = 0;
    unsigned MatchedRelPos = 0;
    short MS = 0, InsertSize = 0;
    short ReadLength = 0, MAX_SNP_ERROR = 0;
    std::vector<UniquePoint> UP_Close, UP_Far;
    short BP = 0;
    int Left = 0, Right = 0;
    unsigned BPLeft = 0, BPRight = 0, IndelSize = 0;
    unsigned short NT_size = 0;
    std::string NT_str_2;         // inversions: second non-template string
    unsigned short NT_size_2 = 0;
    bool UniqueRead = false, Used = false;
    int LeftMostPos = 0;
    // the tables path, whose reads have no points: the sign of UP_Close[0].AbsLoc - UP_Far[0].AbsLoc, from the
    // read's pg_report_summary (OutputInversions orients the read by it)
    signed char CloseVsFar = 0;
    int chr_id = -1;
    std::map<std::string, unsigned> SampleName2Number;
    // The device classifier's lists for this read (pg_variant_cand, pindel_pg.h): 2 kinds x PG_VARIANT_CANDS records and the 2 count
    // bytes; VarIndex = the read's index in the caller's arrays.  Null: SearchVariant's stage searches the pairs itself.
    const pg_variant_cand *VarCands = nullptr;
    const uint8_t *VarCounts = nullptr;
    uint32_t VarIndex = 0;
    // ... and its lists for the five other classifiers: PG_SV_SLOTS records and PG_SV_KINDS count bytes.  Null:
    // those classifiers search the pairs themselves.
    const pg_variant_cand *SvCands = nullptr;
    const uint8_t *SvCounts = nullptr;
    short getReadLength() const { return ReadLength; }
    short getReadLengthMinus() const { return (short)(ReadLength - 1); }
};

struct Chromosome {
    std::string name;
    std::string seq;              // spacer + sequence + spacer
};

class GermlineDepth;              // pg_depth.hpp: the BAMs a -N run measures read depth in

// --repair: opt-in fixes of reference defects that are reproduced by default.  A bit per name.
enum : uint32_t {
    REPAIR_INT_PAIRS = 1u,        // int-pairs: -I reports every chromosome pair of a window, not only the first
    REPAIR_INV_PAIRS = 2u,        // inv-pairs: -N counts the window's read pairs for a large inversion (IsGoodINV's loop)
    REPAIR_DEPTH_MAPQ = 4u,       // depth-mapq: -N's read depth counts records with MAPQ >= 20 only
    REPAIR_BED0 = 8u,             // bed0: -j / -J records are 0-based and half-open
    REPAIR_ALL = 15u
};
enum { DEPTH_MAPQ_FLOOR = 20 };   // what getRelativeCoverageForFiltering passes (and bam2depth ignores)

const struct { const char *name; uint32_t bit; } repair_names[] = {
    { "int-pairs", REPAIR_INT_PAIRS }, { "inv-pairs", REPAIR_INV_PAIRS }, { "depth-mapq", REPAIR_DEPTH_MAPQ }, { "bed0", REPAIR_BED0 },
};
// "name,name,..." or "all" -> bitmask.  false: an unknown name or an empty list (err says which).  (Inline, like the
// rest of what the command line's parser needs: pg_cli.hpp links against nothing.)
inline bool parse_repairs(const std::string &list, uint32_t &mask, std::string &err)
{
    mask = 0;
    const std::string known = "int-pairs, inv-pairs, depth-mapq, bed0 or all";
    if (list.empty()) {
        err = "--repair needs a list of names: " + known;
        return false;
    }
    for (size_t at = 0; at <= list.size();) {
        const size_t comma = std::min(list.find(',', at), list.size());
        const std::string name = list.substr(at, comma - at);
        uint32_t bit = name == "all" ? (uint32_t)REPAIR_ALL : 0;
        for (const auto &r : repair_names)
            if (name == r.name) bit = r.bit;
        if (!bit) {
            err = "--repair: unknown name '" + name + "' (known: " + known + ")";
            return false;
        }
        mask |= bit;
        at = comma + 1;
    }
    return true;
}
// the names of `mask`, comma-separated, in the order of the bits ("" for 0)
inline std::string repairs_text(uint32_t mask)
{
    std::string out;
    for (const auto &r : repair_names)
        if (mask & r.bit) out += (out.empty() ? "" : ",") + std::string(r.name);
    return out;
}

// One same-chromosome discordant read pair of a window as BDData::UpdateBD leaves it before clearing its list
// (RP_READ after ModifyRP, src/bddata.cpp:646-733): what IsGoodINV's loop reads of it.  InsertSize is
// Experimental_InsertSize, the insert size of the BAM's configuration line (src/reader.cpp:1042).
struct DiscordantPair {
    char DA, DB;
    unsigned PosA, PosB, InsertSize;
    short ReadLength;
};
// IsGoodINV's loop (src/output_sorter.cpp:283-365) for an event of `support` reads with breakpoints [real_start,
// real_end], as written -- plus one comparison of the two counts after the loop (the reference compares before it
// counts the pair in hand, so the last pair of the list would never count).  counts (nullable): CountLeft, CountRight.
bool inv_pairs_good(const std::vector<DiscordantPair> &pairs, unsigned support, unsigned real_start, unsigned real_end,
                    unsigned *counts = nullptr);

// Event tables of one window as pg_device_batch_events_download yields them, over ALL reads of the run (indexed by
// SplitRead::VarIndex): n_reads records, the four member lists and the four event lists back to back.
struct SuppliedEvents {
    int chr = -1;
    unsigned win_start = 0, win_end = 0;
    uint32_t n_reads = 0;
    const pg_event_read *reads = nullptr;
    const uint32_t *members = nullptr;
    const pg_event *events = nullptr;
    pg_event_sizes sizes{};
};

// The SV tables of one window as pg_device_batch_sv_events_download yields them, over ALL reads of the run: the
// three member lists and the three event lists back to back.  They go with the SuppliedEvents of the same window.
struct SuppliedSvEvents {
    int chr = -1;
    unsigned win_start = 0, win_end = 0;
    const uint32_t *members = nullptr;
    const pg_event *events = nullptr;
    pg_sv_event_sizes sizes{};
};

struct Settings {                 // the flags the downstream steps read (src/fn_parameters.cpp)
    unsigned spacer = 100000;
    unsigned NumRead2ReportCutOff = 1;   // -M
    unsigned BalanceCutoff = 100;        // -B
    double Seq_Error_Rate = 0.01;        // -e
    int Min_Num_Matched_Bases = 30;      // -d
    int MIN_IndelSize_Inversion = 50;    // -v
    bool Analyze_TD = true, Analyze_INV = true;   // -t, -r
    double window_mbp = 5.0;             // -w
    unsigned max_mismatch[500] = {0};    // g_maxMismatch
    bool log_counts = false;             // print the reference's cross-check lines (far-end counts and checksum)
    bool Analyze_LI = false;             // -l: <prefix>_LI (SortOutputLI)
    bool report_close_mapped = false;    // -s: <prefix>_CloseEndMapped (ReportCloseMappedReads)
    bool only_close_mapped = false;      // -S: close end + _CloseEndMapped only, no far end, no SV search
    bool close_mapped_output() const { return report_close_mapped || only_close_mapped; }
    bool report_interchromosomal = false; // -I: <prefix>_INT per window and <prefix>_INT_final at the end of the run
    // -N (--NormalSamples): IsGoodTD / IsGoodINV's germline filter.  It only acts on reads that come from BAMs
    // (the reference returns true early for -p and -P): `germline` holds those BAMs and is null for text input.
    bool NormalSamples = false;
    std::shared_ptr<const GermlineDepth> germline;
    bool germline_filter() const { return NormalSamples && germline; }
    uint32_t repairs = 0;                // --repair: REPAIR_* bits (default none: the reference's behaviour, defects included)
    bool repair(uint32_t bit) const { return (repairs & bit) != 0; }
    // Opt-in: process_window builds event tables from the reads' candidate lists and writes deletions, short
    // insertions and tandem duplications from them; supplied_events: tables a caller built elsewhere (on the device) for a window.
    bool use_events = false;
    std::vector<SuppliedEvents> supplied_events;
    // ... and writes DI and the inversions from the SV tables instead of through sort_output_di / sort_output_inv;
    // supplied_sv_events: tables built elsewhere, used for a window whose event tables were supplied too.
    bool use_sv_events = false;
    std::vector<SuppliedSvEvents> supplied_sv_events;
    // ... and, with both of the above: builds the report records and summaries of the window, replaces its reads by
    // copies without points, lists and pair fields, and writes the reports from tables, records and summaries alone
    // (Caller::process_window_tables).
    bool use_report_reads = false;
    // ... on that route -s is written per window by process_window -- from the summaries, or from the points of a
    // window that falls back -- and not by the pipeline before the far end
    bool close_mapped_by_window() const { return use_events && use_sv_events && use_report_reads && report_close_mapped && !only_close_mapped; }
};

// What the events path of the last run did.  windows: six values per window process_window saw with use_events set -- chromosome
// index, win_start, win_end, region_start, region_end, reads -- in order.
struct EventPathStats {
    uint64_t fallback_windows = 0;       // windows with an unresolved read (or without usable lists): the existing path ran
    uint64_t table_windows = 0;          // windows written from tables
    uint64_t supplied_windows = 0;       // ... of them, from supplied tables
    uint64_t sv_table_windows = 0;       // windows whose DI and inversion reports were written from SV tables
    uint64_t sv_supplied_windows = 0;    // ... of them, from supplied SV tables
    uint64_t report_windows = 0;         // windows written by process_window_tables, from records and summaries
    uint64_t report_records = 0;         // ... and the records they took
    uint64_t int_table_windows = 0;      // windows whose _INT was written from junction tables built before the reads lost their points
    std::vector<uint32_t> windows;
};
EventPathStats &event_path_stats();

// The long-insertion position tables (include/pindel_pg.h "device classifier: long-insertion position tables") on
// the host.  LiReadIn: what the contract reads of one read of the batch; LiTables: per strand (0 '+', 1 '-') the member list and
// the position table.  li_tables_from_reads states the contract in plain loops: the reference pg_device_batch_li is compared with,
// byte for byte, and what the existing _LI path builds its counters from.  recs (nullable): the events build's per-read records;
// a read is used if its `used` is set or its record carries PG_EVR_BOXED or PG_EVR_USED.
struct LiReadIn {
    bool in_window = true;               // chr_id == the events build's window chr_id
    bool has_close = false, has_far = false;
    bool used = false;
    char strand = 0;                     // the anchor strand
    uint32_t close_abs = 0;              // UP_Close.back().AbsLoc
    int32_t close_len = 0;               // UP_Close.back().LengthStr
    int32_t read_length = 0;             // the post-state read length
};
struct LiTables {
    std::vector<uint32_t> members[2];
    std::vector<pg_li_pos> positions[2];
};
void li_tables_from_reads(const std::vector<LiReadIn> &in, const pg_event_read *recs, uint32_t lo, uint32_t hi, LiTables &out);

// The interchromosomal junction tables (include/pindel_pg.h "interchromosomal junction tables") on the host.
// IntReadIn: what the contract reads of one read; IntTables: the member list and the call table.  int_tables_from_reads states the
// contract in plain loops over the points: the reference pg_device_batch_int is compared with, byte for byte, and what
// Caller::report_interchr builds its calls from.
struct IntReadIn {
    int chr = -1, far_chr = -1;          // the read's chromosome; UP_Far[0]'s
    char strand = 0;                     // the anchor strand
    bool far_minus = false;              // UP_Far[0] has Strand ANTISENSE
    int32_t read_length = 0;             // the post-state read length
    const UniquePoint *close = nullptr, *far = nullptr;
    size_t n_close = 0, n_far = 0;
};
struct IntTables {
    std::vector<uint32_t> members;
    std::vector<pg_int_call> calls;
};
void int_tables_from_reads(const std::vector<IntReadIn> &in, const int32_t *chr_rank, uint32_t n_chr, IntTables &out);
// Ranks of names in std::string order, equal names getting equal ranks: the chr_rank of pg_int_window
std::vector<int32_t> int_chr_ranks(const std::vector<std::string> &names);

int load_fasta(const std::string &path, std::vector<Chromosome> &out, unsigned spacer, std::string &err);

// Pindel-text reads (3 lines per read), appended to `out`.  Trailing non-alphanumerics of SEQ are stripped
// (setUnmatchedSeq).  Reads on unknown chromosomes are kept with chr_id = -1.  A name longer than three
// characters that ends in ".gz" is read through zlib (getLineReaderByFilename, src/pindel.cpp:740-751), all
// members of the file; one that does not inflate is an error.
int load_pindel_text(const std::string &path, const std::vector<Chromosome> &genome,
                     std::vector<SplitRead> &out, std::string &err);

// -P (readPindelConfigFile, src/pindel.cpp:705-737): the first token of every line of `config` is a Pindel-text
// file, the rest of the line is ignored; a last line without a newline counts (the reference drops it).  A relative
// name is tried as given and then relative to the configuration's directory.  Non-zero: the configuration cannot
// be read, lists no file, or lists one that does not exist (err names both).
int read_pindel_config(const std::string &config, std::vector<std::string> &files, std::string &err);
// The reads of a run: the files of the -P configuration in order, then the -p file (src/reader.cpp:1469-1483);
// either may be empty.
int load_pindel_inputs(const std::string &config, const std::string &reads_path, const std::vector<Chromosome> &genome,
                       std::vector<SplitRead> &out, std::string &err);

std::string reverse_complement(const std::string &s);

// SearchVariant's stage fed from candidate lists (SplitRead::VarCands): what the last run did with them.
//   fallbacks   reads whose list was exhausted without making them Used and carried PG_VARIANT_MORE: the pair search ran for them
//   visits      with log_visits set, seven values per (read, kind) whose list was consulted: VarIndex, kind, and what the
//               window-dependent tests compare against -- win_end, region_start, region_end, NumBoxes, BoxSize
struct VariantListStats {
    uint64_t fallbacks = 0;
    bool log_visits = false;
    std::vector<uint32_t> visits;
};
VariantListStats &variant_list_stats();      // (reset by the caller before a run; filled under a lock)

// MergeInterChr (src/pindel.cpp:1514-1579): the calls of int_path (the lines of <prefix>_INT) paired within 10 bp on
// both sides, or alone with support >= 4, written to final_path (created empty when there is no call)
void write_int_final(const std::string &int_path, const std::string &final_path);

// Everything that happens to the reads of ONE chromosome after the close-end stage, with the
// reference's global counters (SV indices, g_reportLength, g_sampleNames) kept across calls.
class Caller {
public:
    Caller(const Settings &s, const std::vector<Chromosome> *genome, const std::string &out_prefix,
           bool truncate_outputs);
    // reads: reads anchored on `chrom` in input order, each with UP_Close/UP_Far filled and
    // UnmatchedSeq in the orientation GetCloseEnd left it.  Reads without a close end must
    // already have been dropped (ReadInRead / ReadBuffer::flush do that).
    void process_window(const Chromosome &chrom, std::vector<SplitRead> &reads, unsigned win_start,
                        unsigned win_end, unsigned region_start, unsigned region_end);
    // post-close-end bookkeeping of ReadInRead (reader.cpp:258-291): CloseEndLength, LeftMostPos,
    // g_reportLength, sample names.  Call once per read that has a close end.
    void note_close_mapped(SplitRead &r);
    // ... for every read of `reads` that has a close end, on a few threads
    void note_close_mapped_all(std::vector<SplitRead> &reads);
    // g_maxInsertSize (GetCloseEndInner, pindel.cpp:2257): the largest InsertSize of any read that entered the close-end
    // search, with or without a close end; never reset.  LI's border buffer is four times it.
    void note_insert_size(int insert_size)
    {
        if (insert_size > g_maxInsertSize) g_maxInsertSize = insert_size;
    }
    // ReportCloseMappedReads (pindel.cpp:1076-1092): the reads of a window that kept a close end, in their order, as
    // Pindel-text records (UnmatchedSeq as GetCloseEnd left it), appended to <prefix>_CloseEndMapped
    void report_close_mapped(const std::vector<SplitRead> &reads);
    // The start of a region-plan record (pindel.cpp:1801-1804 sits inside the record loop): CurrentChrMask all 'N'
    void begin_region()
    {
        chr_marks_.clear();
        mask_chr_ = nullptr;
    }
    unsigned long far_end_checksum = 0;
    double li_seconds = 0.0;             // host time spent in SortOutputLI, all windows so far
    // UpdateRefReadCoverage (pindel.cpp:1272-1330), BAM input: per sample (in the order of the sample-name set as
    // it stands now) the number of reference-supporting reads over every position of the window [start, end];
    // a read counts from its second to its last-but-one base and only if it lies inside the window.  The two
    // coverage integers per sample of every report header come from here (0 0 without it, as for text input).
    struct RefReadSpan { uint32_t pos; uint16_t length; uint16_t tag; };
    void update_ref_coverage(const std::vector<RefReadSpan> &reads, const std::vector<std::string> &tags,
                             unsigned start, unsigned end);
    // --repair inv-pairs: the same-chromosome discordant pairs of the window that process_window is called for next
    // (all BAMs of the run); the inversion reporter's verdict is a function of the event and this list alone
    void set_window_pairs(std::vector<DiscordantPair> pairs) { inv_pairs_ = std::move(pairs); }
    // The tables path for a caller whose window was classified on the device: `reads` are ALL reads of the window as
    // loaded, in the order of the device batch -- no points, no lists, no pair field set.
    //   apply_summaries             per read: rc_flag applied to UnmatchedSeq (read_length_follows: ReadLength becomes its length, as
    //                               the BAM pipeline does), then what note_close_mapped and UpdateFarFragName take from the points
    //   process_window_from_tables  process_window's frame around process_window_tables: the tables as the download entries yield
    //                               them (members per table in n_members, events back to back in table order), the report records
    //                               and the summaries.  summaries_applied: apply_summaries has been called on these reads already.
    void apply_summaries(std::vector<SplitRead> &reads, const pg_report_summary *summaries, bool read_length_follows);
    void process_window_from_tables(const Chromosome &chrom, std::vector<SplitRead> &reads, unsigned win_start, unsigned win_end,
                                    unsigned region_start, unsigned region_end, const pg_event_read *recs, const pg_event_sizes &sizes,
                                    const pg_event *events, const pg_sv_event_sizes &sv_sizes, const pg_event *sv_events,
                                    const pg_report_read *records, const pg_report_summary *summaries, bool summaries_applied);
    // -l and -s on the tables path, for reads without points:
    //   li_window                        the buffered window of SortOutputLI for [win_start, win_end): four times g_maxInsertSize on
    //                                    either side (every read that entered a search so far must have been noted: note_insert_size)
    //   write_li_from_tables             _LI of the window from its position tables (over `reads`, the window's reads in batch order) and
    //                                    the summaries' close lengths; call it after process_window_from_tables, where process_window
    //                                    runs SortOutputLI
    //   report_close_mapped_summaries    report_close_mapped for reads whose summaries have been applied: PG_RS_CLOSE stands for
    //                                    a non-empty UP_Close
    void li_window(const Chromosome &chrom, unsigned win_start, unsigned win_end, unsigned &lo, unsigned &hi) const;
    void write_li_from_tables(const Chromosome &chrom, std::vector<SplitRead> &reads, unsigned win_start, unsigned win_end,
                              const LiTables &tables, const pg_report_summary *summaries);
    void report_close_mapped_summaries(const std::vector<SplitRead> &reads, const pg_report_summary *summaries);
    // tests: CurrentChrMask of `chrom` as earlier reports would have left it (padded positions)
    void set_marks_for_test(const Chromosome &chrom, const uint32_t *marks, uint32_t n)
    {
        mask_chr_ = &chrom;
        chr_marks_.clear();
        if (n) chr_marks_.insert(marks, marks + n);
    }
    ~Caller();

private:
    // The four report files, opened once (append) with a large buffer and flushed at the end of every window.
    // (The reference re-opens the file for every event and flushes every line; the bytes are the same.)
    enum { REP_D = 0, REP_SI, REP_TD, REP_INV, REP_N };
    std::ofstream rep_[REP_N];
    std::vector<char> rep_buf_[REP_N];
    std::ostream &report(int which);        // the file -- or, inside for_boxes, the calling worker's buffer
    void flush_reports();
    // _LI and _CloseEndMapped: written outside for_boxes, so plain files (append, large buffer)
    std::ofstream li_out_, cem_out_, int_out_;
    std::vector<char> li_buf_, cem_buf_, int_buf_;
    std::ofstream &open_append(std::ofstream &f, std::vector<char> &buf, const char *suffix);
    // CurrentChrMask (pindel.cpp:1801-1804): the positions of this chromosome where an event has been reported so far
    // ('B'), kept as a set; reset at every region record (begin_region) and when the chromosome changes.  The reporters call mark() with the breakpoints they print; inside for_boxes the marks
    // are collected per worker and applied when the boxes are done (setting a mark commutes, so the order of the boxes
    // and workers does not matter).
    std::set<unsigned> chr_marks_;
    const Chromosome *mask_chr_ = nullptr;
    void mark(unsigned bp);
    void apply_marks(const std::vector<unsigned> &abs_positions);
    int count_li_ = 0;                   // Count_LI: function-static in the reference, runs across windows and chromosomes
    int g_maxInsertSize = 0;
    // The event number at the head of a report entry.  Entries are formatted box by box in parallel (for_boxes),
    // so `out << ev_no(kind)` writes nothing and only marks the place; the number -- the running count of that kind
    // (D entries print template + non-template deletions so far) -- is put in when the boxes' texts are written in
    // box order.
    enum EvKind { EV_D = 0, EV_D_NT, EV_SI, EV_TD, EV_INV, EV_N };
    struct EvNo { EvKind kind; };
    static EvNo ev_no(EvKind k) { EvNo e = { k }; return e; }
    friend std::ostream &operator<<(std::ostream &out, EvNo e);
    unsigned take_event_number(int k);
    // body(b) for every box, on a few threads; what it wrote through report() lands in the files in box order
    void for_boxes(unsigned n_boxes, const std::function<void(unsigned)> &body);
    Settings S;
    const std::vector<Chromosome> *genome;
    std::string prefix;
    short g_reportLength = 1;
    std::set<std::string> g_sampleNames;
    int d_template = 0, d_nontemplate = 0;   // deletionFileData
    unsigned n_si = 0, n_td = 0, n_inv = 0;
    unsigned BoxSize = 1;
    unsigned g_RegionStart = 0, g_RegionEnd = 0;
    std::vector<std::vector<int>> ref_cov_;   // [sample][position - cov_start_]
    unsigned cov_start_ = 0;

    struct Ctx;
    void search_variant(Ctx &c, int kind);
    void search_indels(Ctx &c);
    void search_tandem_dup(Ctx &c);
    void search_tandem_dup_nt(Ctx &c);
    void search_inversions(Ctx &c);
    void search_inversions_nt(Ctx &c);
    void sort_output_d(Ctx &c, std::vector<std::vector<unsigned>> &boxes);
    void sort_output_di(Ctx &c, std::vector<std::vector<unsigned>> &boxes);
    void sort_output_si(Ctx &c, std::vector<std::vector<unsigned>> &boxes);
    void sort_output_td(Ctx &c, std::vector<std::vector<unsigned>> &boxes, bool nt);
    void sort_output_inv(Ctx &c, std::vector<std::vector<unsigned>> &boxes, bool nt);
    std::string support_columns(const std::vector<SplitRead> &ev, unsigned s, unsigned e,
                                unsigned bp_left, unsigned bp_right, unsigned &n_reads);
    void output_deletion(Ctx &c, std::vector<SplitRead> &g, unsigned s, unsigned e, unsigned rs, unsigned re);
    void output_di(Ctx &c, std::vector<SplitRead> &g, unsigned s, unsigned e);
    void output_si(Ctx &c, std::vector<SplitRead> &g, unsigned s, unsigned e, unsigned rs, unsigned re);
    void output_td(Ctx &c, std::vector<SplitRead> &g, unsigned s, unsigned e, unsigned rs, unsigned re);
    void output_inv(Ctx &c, std::vector<SplitRead> &g, unsigned s, unsigned e, unsigned rs, unsigned re);
    void output_short_inv(Ctx &c, std::vector<SplitRead> &g, unsigned s, unsigned e);
    // SortOutputLI in two parts: the position tables of the window's reads (li_tables_from_reads over their points -- or, on the
    // tables route of the events path, the ones process_window_events left in Ctx before the reads lost their points), then
    // sort_output_li_tables: the walk over the buffered window, the pairing, the event membership and the text, from the tables,
    // chr_marks_, close_len (UP_Close.back().LengthStr per read) and fields a read without points has
    void sort_output_li(Ctx &c, unsigned win_start, unsigned win_end);
    void sort_output_li_tables(Ctx &c, unsigned lo, unsigned hi, const LiTables &tables, const int16_t *close_len);
    // -I (pg_host_int.cpp): the window's reads whose far end lies on another chromosome, copied before the classifiers
    // touch them (InterChromosome_SR, pindel.cpp:1905-1917), and their calls, appended to <prefix>_INT after the window's
    // other reports (pindel.cpp:1940-1942)
    std::vector<SplitRead> interchr_;
    std::vector<int32_t> int_chr_rank_;  // the ranks of the genome's chromosome names (int_chr_ranks), computed at the first use
    bool int_chr_rank_ready_ = false;
    std::vector<DiscordantPair> inv_pairs_;
    // the events path (pg_host_events.cpp): false = the window has to go through the existing path
    bool process_window_events(Ctx &c);
    // one table / one SV table written in table order, shared by the events path and the tables path: make_good fills `good` -- the
    // table's members with their pairs applied -- and is called only if an event is flagged PG_EV_REPORT
    typedef std::function<void(std::vector<SplitRead> &)> MakeGood;
    void write_event_table(Ctx &c, int t, const std::vector<pg_event> &events, const MakeGood &make_good);
    void write_sv_event_table(Ctx &c, int t, const std::vector<pg_event> &events, const MakeGood &make_good);
    // the tables path: the window's reads as loaded -- no points, no lists, no pair field set -- and the event tables
    // (recs: per read; n_members: the seven member lists' sizes; events / sv_events: per table), the report records (one per
    // member, in order) and the summaries (per read; rc_flag is applied to the read here).  What note_close_mapped_all, the
    // UpdateFarFragName loop and process_window_events do, from those inputs alone, with the same output_* calls in the same order.
    void process_window_tables(Ctx &c, const pg_event_read *recs, const uint64_t *n_members, const std::vector<pg_event> *events,
                               const std::vector<pg_event> *sv_events, const pg_report_read *records, const pg_report_summary *summaries,
                               bool summaries_applied = false);
    void collect_interchr(const std::vector<SplitRead> &reads);
    // report_interchr in two parts: the junction tables of the copied reads (int_tables_from_reads over their points),
    // then report_interchr_tables, the one consumer of such tables wherever they were built
    void report_interchr();

public:
    // _INT of one window from its junction tables.  reads: the window's reads in the order the tables index them; they need no points,
    // only Name, FragName, FarFragName and UnmatchedSeq as rc_flag left it.  junction: the indices of the junction reads, with or
    // without a call, ascending (the reference enters every one of them into its name set).  Call it where process_window reports _INT.
    void report_interchr_tables(const std::vector<SplitRead> &reads, const std::vector<uint32_t> &junction, const IntTables &tables);
    // ... with the junction reads taken from the summaries of reads they were applied to (apply_summaries)
    void write_int_from_tables(const std::vector<SplitRead> &reads, const pg_report_summary *summaries, const IntTables &tables);
};

}  // namespace pgh
#endif
