// pg_cli.hpp -- the pindel_pg command line as data: what the flags set (CliOptions), the one table of flags with the
// destination of each, and the parser that walks it.  Flags and their defaults follow src/fn_parameters.cpp.  Nothing here
// touches a device or needs libpindel_pg.so: the caller fills CliOptions::prm with pg_default_params before parsing.
#ifndef PG_CLI_HPP
#define PG_CLI_HPP

#include <cctype>
#include <cstdlib>
#include <string>
#include <vector>

#include "pg_dd.hpp"
#include "pg_host.hpp"
#include "pg_region.hpp"
#include "pindel_pg.h"

namespace pgh {

struct CliOptions {
    std::string fasta, reads_path, pindel_config, bam_config, prefix, bd_path;   // -f, -p, -P, -i, -o, -b
    std::string region, include_bed, exclude_bed;                                // -c, -j, -J
    pg_params prm{};                       // the search's own flags (-x -a -m -u -e -E -H) on the library's defaults
    Settings S;                            // what the classifiers and reporters read
    DDSettings dd;                         // -q's flags
    unsigned min_anchor_quality = 0;       // -A  } with -u, the split-read selection of the BAM reader (BamIngestSettings)
    int ref_read_nm = 2;                   // -n  }
    bool search_rp = true;                 // -R: discordant read pairs as window hints (BAM input only)
    bool use_bd = false;                   // --bd-hints on: the events of a -b file as window hints for Pindel-text input
    size_t flush_reads = 0;                // --flush-reads: reads per close-end call (0 = a whole bin)
    bool detect_dd = false;                // -q
    std::string gpu_list;                  // -G as typed
    std::vector<int> devices;              // ... and as parsed; without -G, prm.device alone
    bool device_classifier = false;        // --device-classifier: windows are classified on the device and written from tables
    int device_classifier_listed = -1;     // --device-classifier-listed 0..4: pg_classify_params::max_listed (-1: not given, no cut)
    bool device_classifier_hints = false;  // --device-classifier-hints: hinted windows are searched on the device-resident path
    bool device_classifier_li = false;     // --device-classifier-li: -l and -s are written from device tables and summaries
    bool device_classifier_int = false;    // --device-classifier-int: -I is written from device junction tables and summaries
    bool device_classifier_dd = false;     // --device-classifier-dd: -q takes its breakpoint tables and consensus from the device
};

// A flag's word as the parser hands it to the row: as typed, as a number (kinds i and f), as a switch's state (kind u)
struct CliArg {
    const char *text;
    long i;
    double f;
    bool on;
};
// false: the word is refused and err says why (status 2)
typedef bool (*CliSet)(CliOptions &o, const CliArg &a, std::string &err);
struct CliFlag {
    const char *sh, *lg;                   // short ("" = none) and long spelling
    char kind;                             // i int, f float, s string, u unary switch
    CliSet set;                            // where the word goes; null = accepted and ignored
};

#define PG_CLI_SET(statement) [](CliOptions &o, const CliArg &a, std::string &) { statement; return true; }
// The rows with a side condition
inline bool cli_set_window(CliOptions &o, const CliArg &a, std::string &err)
{
    if ((unsigned)(a.f * 1000000) == 0) {          // -w: a window of no bases
        err = "-w must be at least 0.000001 (Mbp)";
        return false;
    }
    o.S.window_mbp = a.f;
    return true;
}
inline bool cli_set_region(CliOptions &o, const CliArg &a, std::string &err)
{
    RegionSpec spec;                               // -c: the syntax is checked here, the chromosome with the region plan
    if (parse_region(a.text, spec, err)) return false;
    o.region = a.text;
    return true;
}
inline bool cli_set_threads(CliOptions &, const CliArg &a, std::string &)
{
    // -T: host threads of the classifiers / reporters (the search itself runs on the GPU); a PGH_THREADS already set wins
    if (a.i >= 1) setenv("PGH_THREADS", std::to_string(a.i).c_str(), 0);
    return true;
}

// Value flags need a word, and a numeric one a word that does not start with '-' and is a number; a unary switch takes an
// optional true/false word (readParameters, fn_parameters.cpp:366-406).  A flag given twice takes its last value.
static const CliFlag CLI_FLAGS[] = {
    { "-f", "--fasta", 's', PG_CLI_SET(o.fasta = a.text) },
    { "-p", "--pindel-file", 's', PG_CLI_SET(o.reads_path = a.text) },
    { "-P", "--pindel-config-file", 's', PG_CLI_SET(o.pindel_config = a.text) },
    { "-i", "--config-file", 's', PG_CLI_SET(o.bam_config = a.text) },
    { "-o", "--output-prefix", 's', PG_CLI_SET(o.prefix = a.text) },
    { "-x", "--max_range_index", 'i', PG_CLI_SET(o.prm.max_range_index = (int)a.i) },
    { "-a", "--additional_mismatch", 'i', PG_CLI_SET(o.prm.additional_mismatch = (int)a.i) },
    { "-m", "--min_perfect_match_around_BP", 'i', PG_CLI_SET(o.prm.min_perfect_match_around_bp = (int)a.i) },
    { "-u", "--maximum_allowed_mismatch_rate", 'f', PG_CLI_SET(o.prm.max_allowed_mismatch_rate = a.f) },
    { "-e", "--sequencing_error_rate", 'f', PG_CLI_SET(o.prm.seq_error_rate = o.S.Seq_Error_Rate = a.f) },   // search and reporters
    { "-E", "--sensitivity", 'f', PG_CLI_SET(o.prm.sensitivity = a.f) },
    { "-H", "--min_close", 'i', PG_CLI_SET(o.prm.min_close = (int)a.i) },
    { "-M", "--minimum_support_for_event", 'i', PG_CLI_SET(o.S.NumRead2ReportCutOff = (unsigned)a.i) },
    { "-B", "--balance_cutoff", 'i', PG_CLI_SET(o.S.BalanceCutoff = (unsigned)a.i) },
    { "-d", "--min_num_matched_bases", 'i', PG_CLI_SET(o.S.Min_Num_Matched_Bases = (int)a.i) },
    { "-v", "--min_inversion_size", 'i', PG_CLI_SET(o.S.MIN_IndelSize_Inversion = (int)a.i) },
    { "-w", "--window_size", 'f', cli_set_window },
    { "-T", "--number_of_threads", 'i', cli_set_threads },
    { "-b", "--breakdancer", 's', PG_CLI_SET(o.bd_path = a.text) },
    { "-G", "--gpus", 's', PG_CLI_SET(o.gpu_list = a.text) },                                    // parsed after the last flag
    { "", "--bd-hints", 's', PG_CLI_SET(o.use_bd = std::string(a.text) == "on") },              // any other word is off
    { "", "--flush-reads", 'i', PG_CLI_SET(o.flush_reads = a.i > 0 ? (size_t)a.i : 0) },
    { "-c", "--chromosome", 's', cli_set_region },
    { "-j", "--include", 's', PG_CLI_SET(o.include_bed = a.text) },
    { "-J", "--exclude", 's', PG_CLI_SET(o.exclude_bed = a.text) },
    { "", "--repair", 's', [](CliOptions &o, const CliArg &a, std::string &err) { return parse_repairs(a.text, o.S.repairs, err); } },
    { "-n", "--NM", 'i', PG_CLI_SET(o.ref_read_nm = (int)a.i) },       // "-n" is registered twice in the reference; --NM comes first
    { "", "--min_NT_size", 'i', nullptr },                             // not read on this path
    { "-A", "--anchor_quality", 'i', PG_CLI_SET(o.min_anchor_quality = (unsigned)a.i) },
    { "-L", "--logfilename", 's', nullptr },                           // no effect on this path
    { "-r", "--report_inversions", 'u', PG_CLI_SET(o.S.Analyze_INV = a.on) },
    { "-t", "--report_duplications", 'u', PG_CLI_SET(o.S.Analyze_TD = a.on) },
    { "-l", "--report_long_insertions", 'u', PG_CLI_SET(o.S.Analyze_LI = a.on) },
    { "-k", "--report_breakpoints", 'u', nullptr },                    // (beyond the empty _BP file) a report this program does not write
    { "-s", "--report_close_mapped_reads", 'u', PG_CLI_SET(o.S.report_close_mapped = a.on) },
    { "-S", "--report_only_close_mapped_reads", 'u', PG_CLI_SET(o.S.only_close_mapped = a.on) },
    { "-I", "--report_interchromosomal_events", 'u', PG_CLI_SET(o.S.report_interchromosomal = a.on) },
    { "-C", "--IndelCorrection", 'u', nullptr },                       // a search this program does not run
    { "-N", "--NormalSamples", 'u', PG_CLI_SET(o.S.NormalSamples = a.on) },
    { "-R", "--RP", 'u', PG_CLI_SET(o.search_rp = a.on) },
    { "-q", "--detect_DD", 'u', PG_CLI_SET(o.detect_dd = true) },   // on whatever its word: the reference tests isSet() (pindel.cpp:1992)
    { "", "--MAX_DD_BREAKPOINT_DISTANCE", 'i', PG_CLI_SET(o.dd.max_bp_distance = (int)a.i) },
    { "", "--MAX_DISTANCE_CLUSTER_READS", 'i', PG_CLI_SET(o.dd.max_distance_cluster = (int)a.i) },
    { "", "--MIN_DD_CLUSTER_SIZE", 'i', PG_CLI_SET(o.dd.min_cluster_size = (int)a.i) },
    { "", "--MIN_DD_BREAKPOINT_SUPPORT", 'i', PG_CLI_SET(o.dd.min_bp_support = (int)a.i) },
    { "", "--MIN_DD_MAP_DISTANCE", 'i', PG_CLI_SET(o.dd.min_map_distance = (int)a.i) },
    { "", "--DD_REPORT_DUPLICATION_READS", 'u', PG_CLI_SET(o.dd.report_dup_reads = a.on) },
};
// The flags of the device classifier, a table of their own that parse_cli walks when no row of CLI_FLAGS matches
static const CliFlag CLI_DEVICE_FLAGS[] = {
    { "", "--device-classifier", 'u', PG_CLI_SET(o.device_classifier = a.on) },
    { "", "--device-classifier-listed", 'i', [](CliOptions &o, const CliArg &a, std::string &err) {
         if (a.i < 0 || a.i > PG_VARIANT_CANDS) {
             err = "--device-classifier-listed takes a number of pairs from 0 to 4";
             return false;
         }
         o.device_classifier_listed = (int)a.i;
         return true;
     } },
};
// ... and the switch that admits window hints there, in a third table that parse_cli walks after it
static const CliFlag CLI_DEVICE_HINT_FLAGS[] = {
    { "", "--device-classifier-hints", 'u', PG_CLI_SET(o.device_classifier_hints = a.on) },
};
// ... and the switch that admits -l and -s there, in a fourth table that parse_cli walks after it
static const CliFlag CLI_DEVICE_LI_FLAGS[] = {
    { "", "--device-classifier-li", 'u', PG_CLI_SET(o.device_classifier_li = a.on) },
};
// ... and the switch that admits -I there, in a fifth table that parse_cli walks after it
static const CliFlag CLI_DEVICE_INT_FLAGS[] = {
    { "", "--device-classifier-int", 'u', PG_CLI_SET(o.device_classifier_int = a.on) },
};
// ... and the switch that admits -q there, in a sixth table that parse_cli walks last
static const CliFlag CLI_DEVICE_DD_FLAGS[] = {
    { "", "--device-classifier-dd", 'u', PG_CLI_SET(o.device_classifier_dd = a.on) },
};
#undef PG_CLI_SET

// What --device-classifier does not deliver yet: "" or the refusal, looked at after the last flag.  -l / -s,
// -I and -q are admitted by a switch of their own each; -S, -N and several devices stay refused.
inline std::string device_classifier_refusal(const CliOptions &o)
{
    if (!o.device_classifier)
        return o.device_classifier_listed >= 0  ? "--device-classifier-listed needs --device-classifier"
               : o.device_classifier_hints      ? "--device-classifier-hints needs --device-classifier"
               : o.device_classifier_li         ? "--device-classifier-li needs --device-classifier"
               : o.device_classifier_int        ? "--device-classifier-int needs --device-classifier"
               : o.device_classifier_dd         ? "--device-classifier-dd needs --device-classifier"
                                                : "";
    const bool li = o.device_classifier_li;                // -l and -s are admitted with the switch alone
    const bool junctions = o.device_classifier_int;        // ... and -I with its own
    const bool dd = o.device_classifier_dd;                // ... and -q with its own
    const char *with = o.S.Analyze_LI && !li ? "-l" : o.S.report_close_mapped && !li ? "-s" : o.S.only_close_mapped ? "-S"
                     : o.S.report_interchromosomal && !junctions ? "-I"
                     : o.detect_dd && !dd ? "-q" : o.S.NormalSamples ? "-N" : nullptr;
    if (with) return std::string("--device-classifier cannot be combined with ") + with + ": its report needs points or pairs this path does not deliver";
    if (o.use_bd && !o.device_classifier_hints) return "--device-classifier cannot be combined with --bd-hints on: window hints are not searched on this path";
    if (!o.bam_config.empty() && o.search_rp && !o.device_classifier_hints)
        return "--device-classifier with BAM input needs -R false: read-pair window hints are not searched on this path";
    if (o.devices.size() > 1) return "--device-classifier runs on one device: give -G a single device";
    return "";
}

// -G 0,1,...: numbers >= 0 separated by single commas; one comma may end the list.  false: not such a list, or empty
inline bool parse_device_list(const std::string &list, std::vector<int> &devices)
{
    const char *q = list.c_str();
    while (*q) {
        char *endp = nullptr;
        const long d = strtol(q, &endp, 10);
        if (endp == q || d < 0 || (*endp != 0 && *endp != ',')) return false;
        devices.push_back((int)d);
        q = *endp ? endp + 1 : endp;
    }
    return !devices.empty();
}

// argv -> o.  0, or 2 with err = what pindel_pg prints after "pindel_pg: ".  Flag errors come first, in the order of the
// arguments; the device list is looked at after the last flag.
inline int parse_cli(int argc, char **argv, CliOptions &o, std::string &err)
{
    for (int i = 1; i < argc; i++) {
        const std::string f = argv[i];
        const CliFlag *fl = nullptr;
        for (const CliFlag &x : CLI_FLAGS)
            if ((x.sh[0] && f == x.sh) || f == x.lg) fl = &x;
        if (!fl)
            for (const CliFlag &x : CLI_DEVICE_FLAGS)
                if (f == x.lg) fl = &x;
        if (!fl)
            for (const CliFlag &x : CLI_DEVICE_HINT_FLAGS)
                if (f == x.lg) fl = &x;
        if (!fl)
            for (const CliFlag &x : CLI_DEVICE_LI_FLAGS)
                if (f == x.lg) fl = &x;
        if (!fl)
            for (const CliFlag &x : CLI_DEVICE_INT_FLAGS)
                if (f == x.lg) fl = &x;
        if (!fl)
            for (const CliFlag &x : CLI_DEVICE_DD_FLAGS)
                if (f == x.lg) fl = &x;
        if (!fl) {
            err = "unknown argument: " + f;
            return 2;
        }
        CliArg a = { "", 0, 0.0, true };
        if (fl->kind == 'u') {
            // the optional word: one that starts with f, F or 0 turns the switch off, any other word turns it on
            if (i + 1 < argc && argv[i + 1][0] != '-') {
                a.text = argv[++i];
                const char c0 = (char)tolower((unsigned char)a.text[0]);
                a.on = !(c0 == 'f' || c0 == '0');
            }
        } else {
            if (i + 1 >= argc) {
                err = "argument of " + f + " lacking.";
                return 2;
            }
            a.text = argv[++i];
            if (a.text[0] == '-' && fl->kind != 's') {      // (a string may start with '-')
                err = "argument of " + f + " seems erroneous.";
                return 2;
            }
            if (fl->kind != 's') {
                char *endp = nullptr;
                if (fl->kind == 'i') a.i = strtol(a.text, &endp, 10);
                else a.f = strtod(a.text, &endp);
                if (endp == a.text || *endp != 0) {
                    err = "argument of " + f + " is not a number: " + a.text;
                    return 2;
                }
            }
        }
        if (fl->set && !fl->set(o, a, err)) return 2;
    }
    o.devices.clear();
    if (o.gpu_list.empty()) o.devices.push_back(o.prm.device);
    else if (!parse_device_list(o.gpu_list, o.devices)) {
        err = "bad device list " + o.gpu_list;
        return 2;
    }
    err = device_classifier_refusal(o);
    if (!err.empty()) return 2;
    return 0;
}

}  // namespace pgh
#endif
