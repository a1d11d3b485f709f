// Stand-alone check of pindel_amd/csrc/host/pg_cli.hpp (plain g++, address + undefined-behaviour sanitizers, no GPU, no
// libpindel_pg.so): every row of the flag table reaches its field and no other, by both spellings; every quirk of the parser; the
// five error texts; repeated flags.  Prints "ok <cases>" and exits 0, or says what failed and exits 1.
// tests/test_cli_options_cpu.py builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "pg_cli.hpp"

using namespace pgh;

static int g_fail = 0, g_cases = 0;
#define CHECK(cond, ...)                                                                     \
    do {                                                                                     \
        g_cases++;                                                                           \
        if (!(cond)) {                                                                       \
            fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #cond);                 \
            fprintf(stderr, __VA_ARGS__);                                                    \
            fprintf(stderr, "\n");                                                           \
            if (++g_fail > 20) exit(1);                                                      \
        }                                                                                    \
    } while (0)

// pg_default_params (pg_api.cpp) by hand: the defaults of include/pindel_pg.h
static CliOptions defaults()
{
    CliOptions o;
    o.prm.abi_version = PG_ABI_VERSION;
    o.prm.device = 0;
    o.prm.max_range_index = 2;
    o.prm.additional_mismatch = 1;
    o.prm.min_perfect_match_around_bp = 3;
    o.prm.min_close = 8;
    o.prm.max_allowed_mismatch_rate = 0.02;
    o.prm.seq_error_rate = 0.01;
    o.prm.sensitivity = 0.95;
    o.prm.spacer = 100000;
    return o;
}

// the name of the first field in which a and b differ, "" when there is none
static std::string first_difference(const CliOptions &a, const CliOptions &b)
{
#define FIELD(f) \
    if (!(a.f == b.f)) return #f;
    FIELD(fasta) FIELD(reads_path) FIELD(pindel_config) FIELD(bam_config) FIELD(prefix) FIELD(bd_path)
    FIELD(region) FIELD(include_bed) FIELD(exclude_bed)
    FIELD(prm.abi_version) FIELD(prm.device) FIELD(prm.max_range_index) FIELD(prm.additional_mismatch)
    FIELD(prm.min_perfect_match_around_bp) FIELD(prm.min_close) FIELD(prm.max_allowed_mismatch_rate) FIELD(prm.seq_error_rate)
    FIELD(prm.sensitivity) FIELD(prm.spacer) FIELD(prm.reserved)
    FIELD(S.spacer) FIELD(S.NumRead2ReportCutOff) FIELD(S.BalanceCutoff) FIELD(S.Seq_Error_Rate) FIELD(S.Min_Num_Matched_Bases)
    FIELD(S.MIN_IndelSize_Inversion) FIELD(S.Analyze_TD) FIELD(S.Analyze_INV) FIELD(S.window_mbp) FIELD(S.log_counts)
    FIELD(S.Analyze_LI) FIELD(S.report_close_mapped) FIELD(S.only_close_mapped) FIELD(S.report_interchromosomal)
    FIELD(S.NormalSamples) FIELD(S.germline) FIELD(S.repairs)
    FIELD(dd.max_bp_distance) FIELD(dd.max_distance_cluster) FIELD(dd.min_cluster_size) FIELD(dd.min_bp_support)
    FIELD(dd.min_map_distance) FIELD(dd.report_dup_reads)
    FIELD(min_anchor_quality) FIELD(ref_read_nm) FIELD(search_rp) FIELD(use_bd) FIELD(flush_reads) FIELD(detect_dd)
    FIELD(gpu_list) FIELD(devices)
#undef FIELD
    if (memcmp(a.S.max_mismatch, b.S.max_mismatch, sizeof a.S.max_mismatch)) return "S.max_mismatch";
    return "";
}

struct Parsed {
    int status;
    std::string err;
    CliOptions o;
};
static Parsed parse(std::vector<std::string> words)
{
    words.insert(words.begin(), "pindel_pg");
    std::vector<char *> argv;
    for (std::string &w : words) argv.push_back(&w[0]);
    Parsed p = { 0, "", defaults() };
    p.status = parse_cli((int)argv.size(), argv.data(), p.o, p.err);
    return p;
}

// words parse, and change the defaults exactly as `change` does
static void expect(const std::vector<std::string> &words, const std::function<void(CliOptions &)> &change)
{
    std::string line;
    for (const std::string &w : words) line += " " + w;
    const Parsed p = parse(words);
    CliOptions want = defaults();
    want.devices.assign(1, 0);
    change(want);
    CHECK(p.status == 0 && p.err.empty(), "%s: status %d, %s", line.c_str(), p.status, p.err.c_str());
    CHECK(first_difference(p.o, want).empty(), "%s: field %s", line.c_str(), first_difference(p.o, want).c_str());
}
// words are refused with status 2 and this text
static void expect_error(const std::vector<std::string> &words, const std::string &text)
{
    const Parsed p = parse(words);
    CHECK(p.status == 2 && p.err == text, "%s ...: status %d, \"%s\" instead of \"%s\"", words[0].c_str(), p.status, p.err.c_str(), text.c_str());
}

// One row of the table as this test expects it: the short spelling ("" = none), the long one, a word, and what it does
struct Row {
    const char *sh, *lg, *word;
    std::function<void(CliOptions &)> change;
};
#define SETS(...) [](CliOptions &o) { __VA_ARGS__; }
static const Row ROWS[] = {
    { "-f", "--fasta", "r.fa", SETS(o.fasta = "r.fa") },
    { "-p", "--pindel-file", "-reads", SETS(o.reads_path = "-reads") },
    { "-P", "--pindel-config-file", "list.txt", SETS(o.pindel_config = "list.txt") },
    { "-i", "--config-file", "bams.txt", SETS(o.bam_config = "bams.txt") },
    { "-o", "--output-prefix", "-name", SETS(o.prefix = "-name") },                      // a string may start with '-'
    { "-x", "--max_range_index", "5", SETS(o.prm.max_range_index = 5) },
    { "-a", "--additional_mismatch", "3", SETS(o.prm.additional_mismatch = 3) },
    { "-m", "--min_perfect_match_around_BP", "7", SETS(o.prm.min_perfect_match_around_bp = 7) },
    { "-u", "--maximum_allowed_mismatch_rate", "0.05", SETS(o.prm.max_allowed_mismatch_rate = 0.05) },
    { "-e", "--sequencing_error_rate", "0.02", SETS(o.prm.seq_error_rate = 0.02; o.S.Seq_Error_Rate = 0.02) },   // both fields
    { "-E", "--sensitivity", "0.5", SETS(o.prm.sensitivity = 0.5) },
    { "-H", "--min_close", "11", SETS(o.prm.min_close = 11) },
    { "-M", "--minimum_support_for_event", "4", SETS(o.S.NumRead2ReportCutOff = 4) },
    { "-B", "--balance_cutoff", "9", SETS(o.S.BalanceCutoff = 9) },
    { "-d", "--min_num_matched_bases", "31", SETS(o.S.Min_Num_Matched_Bases = 31) },
    { "-v", "--min_inversion_size", "60", SETS(o.S.MIN_IndelSize_Inversion = 60) },
    { "-w", "--window_size", "0.000001", SETS(o.S.window_mbp = 0.000001) },              // the smallest window accepted
    { "-T", "--number_of_threads", "0", SETS((void)o) },                                 // (below 1: not even the environment changes)
    { "-b", "--breakdancer", "bd.txt", SETS(o.bd_path = "bd.txt") },
    { "-G", "--gpus", "2,0", SETS(o.gpu_list = "2,0"; o.devices = { 2, 0 }) },
    { "", "--bd-hints", "on", SETS(o.use_bd = true) },
    { "", "--flush-reads", "7", SETS(o.flush_reads = 7) },
    { "-c", "--chromosome", "chr1:5-9", SETS(o.region = "chr1:5-9") },
    { "-j", "--include", "in.bed", SETS(o.include_bed = "in.bed") },
    { "-J", "--exclude", "ex.bed", SETS(o.exclude_bed = "ex.bed") },
    { "", "--repair", "bed0,int-pairs", SETS(o.S.repairs = REPAIR_BED0 | REPAIR_INT_PAIRS) },
    { "-n", "--NM", "4", SETS(o.ref_read_nm = 4) },
    { "", "--min_NT_size", "12", SETS((void)o) },                                        // accepted and ignored
    { "-A", "--anchor_quality", "20", SETS(o.min_anchor_quality = 20) },
    { "-L", "--logfilename", "log.txt", SETS((void)o) },                                 // accepted and ignored
    { "-r", "--report_inversions", "false", SETS(o.S.Analyze_INV = false) },
    { "-t", "--report_duplications", "0", SETS(o.S.Analyze_TD = false) },
    { "-l", "--report_long_insertions", "", SETS(o.S.Analyze_LI = true) },
    { "-k", "--report_breakpoints", "", SETS((void)o) },                                 // accepted and ignored
    { "-s", "--report_close_mapped_reads", "true", SETS(o.S.report_close_mapped = true) },
    { "-S", "--report_only_close_mapped_reads", "", SETS(o.S.only_close_mapped = true) },
    { "-I", "--report_interchromosomal_events", "", SETS(o.S.report_interchromosomal = true) },
    { "-C", "--IndelCorrection", "true", SETS((void)o) },                                // accepted and ignored
    { "-N", "--NormalSamples", "", SETS(o.S.NormalSamples = true) },
    { "-R", "--RP", "False", SETS(o.search_rp = false) },
    { "-q", "--detect_DD", "", SETS(o.detect_dd = true) },
    { "", "--MAX_DD_BREAKPOINT_DISTANCE", "351", SETS(o.dd.max_bp_distance = 351) },
    { "", "--MAX_DISTANCE_CLUSTER_READS", "101", SETS(o.dd.max_distance_cluster = 101) },
    { "", "--MIN_DD_CLUSTER_SIZE", "4", SETS(o.dd.min_cluster_size = 4) },
    { "", "--MIN_DD_BREAKPOINT_SUPPORT", "5", SETS(o.dd.min_bp_support = 5) },
    { "", "--MIN_DD_MAP_DISTANCE", "8001", SETS(o.dd.min_map_distance = 8001) },
    { "", "--DD_REPORT_DUPLICATION_READS", "", SETS(o.dd.report_dup_reads = true) },
};

static std::vector<std::string> with_word(const char *flag, const char *word)
{
    std::vector<std::string> w(1, flag);
    if (word[0]) w.push_back(word);          // ("": a switch without its optional word)
    return w;
}

static void check_rows()
{
    // the two tables list the same flags, so no row of the parser's goes untested
    const size_t n_rows = sizeof ROWS / sizeof ROWS[0], n_flags = sizeof CLI_FLAGS / sizeof CLI_FLAGS[0];
    CHECK(n_rows == n_flags, "%zu rows here, %zu in CLI_FLAGS", n_rows, n_flags);
    for (const CliFlag &f : CLI_FLAGS) {
        size_t hits = 0;
        for (const Row &r : ROWS) hits += !strcmp(r.sh, f.sh) && !strcmp(r.lg, f.lg);
        CHECK(hits == 1, "%s / %s is in %zu rows of this test", f.sh, f.lg, hits);
    }
    setenv("PGH_THREADS", "5", 1);           // (-T rows must leave it alone)
    for (const Row &r : ROWS) {
        if (r.sh[0]) expect(with_word(r.sh, r.word), r.change);
        expect(with_word(r.lg, r.word), r.change);
    }
    CHECK(std::string(getenv("PGH_THREADS")) == "5", "PGH_THREADS is %s", getenv("PGH_THREADS"));
    expect({}, SETS((void)o));               // no argument: the defaults, device 0
    CliOptions d = defaults();
    d.prm.device = 3;                        // without -G the library's default device is the list
    std::string err;
    char name[] = "pindel_pg";
    char *argv[] = { name };
    CHECK(parse_cli(1, argv, d, err) == 0 && d.devices == std::vector<int>(1, 3), "default device list");
}

static void check_quirks()
{
    // a unary switch takes an optional word: f, F or 0 first turns it off, any other word turns it on; a flag is no word
    expect({ "-R" }, SETS((void)o));
    expect({ "-R", "yes" }, SETS((void)o));
    expect({ "-R", "false" }, SETS(o.search_rp = false));
    expect({ "-R", "0" }, SETS(o.search_rp = false));
    expect({ "-R", "F" }, SETS(o.search_rp = false));
    expect({ "-R", "-l" }, SETS(o.S.Analyze_LI = true));
    expect({ "-l", "no" }, SETS(o.S.Analyze_LI = true));                 // ("no" does not start with f, F or 0)
    expect({ "-r", "1" }, SETS((void)o));
    expect({ "-l", "off", "-s" }, SETS(o.S.Analyze_LI = true; o.S.report_close_mapped = true));
    // -q is on whatever its word, and takes the word
    expect({ "-q", "false" }, SETS(o.detect_dd = true));
    expect({ "-q", "0", "-l" }, SETS(o.detect_dd = true; o.S.Analyze_LI = true));
    // a value that starts with '-' is erroneous for numeric flags only
    expect_error({ "-x", "-3" }, "argument of -x seems erroneous.");
    expect_error({ "--max_range_index", "-3" }, "argument of --max_range_index seems erroneous.");
    expect_error({ "-u", "-0.5" }, "argument of -u seems erroneous.");
    expect({ "-o", "-name" }, SETS(o.prefix = "-name"));
    // -w: rejected when (unsigned)(v * 1000000) == 0
    expect_error({ "-w", "0.0000001" }, "-w must be at least 0.000001 (Mbp)");
    expect_error({ "-w", "0" }, "-w must be at least 0.000001 (Mbp)");
    expect({ "-w", "0.000001" }, SETS(o.S.window_mbp = 0.000001));
    expect({ "-w", "2.5" }, SETS(o.S.window_mbp = 2.5));
    // --flush-reads clamps a negative value to 0 -- one that gets past the check above, which refuses "-5"
    expect_error({ "--flush-reads", "-5" }, "argument of --flush-reads seems erroneous.");
    expect({ "--flush-reads", " -5" }, SETS((void)o));                   // (strtol skips the blank: -5, clamped to 0)
    expect({ "--flush-reads", "0" }, SETS((void)o));
    expect({ "--flush-reads", "+5" }, SETS(o.flush_reads = 5));
    // --bd-hints is on only for the word "on"
    expect({ "--bd-hints", "ON" }, SETS((void)o));
    expect({ "--bd-hints", "on", "--bd-hints", "true" }, SETS((void)o));
    // -e lands in both fields (the row above); -c syntax and the --repair list are checked at parse time
    expect({ "-c", "ALL" }, SETS(o.region = "ALL"));
    expect({ "-c", "chr2:1,000-2,000" }, SETS(o.region = "chr2:1,000-2,000"));
    {
        const Parsed p = parse({ "-c", "chr1:9-5x" });
        CHECK(p.status == 2 && !p.err.empty() && p.o.region.empty(), "-c chr1:9-5x: status %d, %s", p.status, p.err.c_str());
        RegionSpec spec;
        std::string want;
        CHECK(parse_region("chr1:9-5x", spec, want) != 0 && p.err == want, "-c chr1:9-5x: \"%s\" instead of \"%s\"", p.err.c_str(), want.c_str());
    }
    expect({ "--repair", "all" }, SETS(o.S.repairs = REPAIR_ALL));
    for (const char *bad : { "", "nothing", "bed0,", "bed0,,int-pairs" }) {
        const Parsed p = parse({ "--repair", bad });
        uint32_t mask = 0;
        std::string want;
        const bool ok = parse_repairs(bad, mask, want);
        CHECK((p.status == 0) == ok && p.err == (ok ? "" : want), "--repair '%s': status %d, %s", bad, p.status, p.err.c_str());
    }
    // -T sets PGH_THREADS for values of at least 1, and only where it is not set
    unsetenv("PGH_THREADS");
    expect({ "-T", "0" }, SETS((void)o));
    CHECK(getenv("PGH_THREADS") == nullptr, "-T 0 set PGH_THREADS");
    expect({ "-T", "3" }, SETS((void)o));
    CHECK(getenv("PGH_THREADS") && std::string(getenv("PGH_THREADS")) == "3", "-T 3");
    expect({ "-T", "4" }, SETS((void)o));
    CHECK(std::string(getenv("PGH_THREADS")) == "3", "-T 4 after -T 3 (the variable was set)");
    // -G: numbers >= 0 separated by single commas, one comma may end the list (pinned from the parent's binary)
    expect({ "-G", "0,0,0" }, SETS(o.gpu_list = "0,0,0"; o.devices = { 0, 0, 0 }));
    expect({ "-G", "1," }, SETS(o.gpu_list = "1,"; o.devices = { 1 }));
    expect({ "-G", "" }, SETS((void)o));
    expect_error({ "-G", "0,,1" }, "bad device list 0,,1");
    expect_error({ "-G", "," }, "bad device list ,");
    expect_error({ "-G", "a" }, "bad device list a");
    expect_error({ "-G", "0,-1" }, "bad device list 0,-1");
    expect_error({ "-G", "0;1" }, "bad device list 0;1");
    // ... looked at after the last flag: a later flag error comes first, and a later list replaces a bad one
    expect_error({ "-G", "a", "-x" }, "argument of -x lacking.");
    expect({ "-G", "a", "-G", "1" }, SETS(o.gpu_list = "1"; o.devices = { 1 }));
}

static void check_errors_and_repeats()
{
    expect_error({ "--frobnicate" }, "unknown argument: --frobnicate");
    expect_error({ "reads.txt" }, "unknown argument: reads.txt");
    expect_error({ "-f", "r.fa", "-Z", "1" }, "unknown argument: -Z");
    expect_error({ "-x" }, "argument of -x lacking.");
    expect_error({ "--fasta" }, "argument of --fasta lacking.");                          // (the argument as typed)
    expect_error({ "-M", "-1" }, "argument of -M seems erroneous.");
    expect_error({ "-x", "two" }, "argument of -x is not a number: two");
    expect_error({ "-x", "2.5" }, "argument of -x is not a number: 2.5");
    expect_error({ "--window_size", "5Mbp" }, "argument of --window_size is not a number: 5Mbp");
    expect_error({ "-x", "" }, "argument of -x is not a number: ");
    expect_error({ "-G", "x" }, "bad device list x");
    // a flag given twice takes its last value
    expect({ "-x", "3", "-x", "4" }, SETS(o.prm.max_range_index = 4));
    expect({ "-f", "a.fa", "--fasta", "b.fa" }, SETS(o.fasta = "b.fa"));
    expect({ "-R", "false", "-R" }, SETS((void)o));
    expect({ "-l", "-l", "false" }, SETS((void)o));
    expect({ "-q", "-q", "false" }, SETS(o.detect_dd = true));
    expect({ "--repair", "bed0", "--repair", "int-pairs" }, SETS(o.S.repairs = REPAIR_INT_PAIRS));
    expect({ "-e", "0.5", "-e", "0.02" }, SETS(o.prm.seq_error_rate = 0.02; o.S.Seq_Error_Rate = 0.02));
    // an error stops the parse where it stands: what came before is set, what comes after is not
    const Parsed p = parse({ "-x", "4", "-a", "x", "-m", "9" });
    CHECK(p.status == 2 && p.o.prm.max_range_index == 4 && p.o.prm.min_perfect_match_around_bp == 3, "partial parse");
}

int main()
{
    check_rows();
    check_quirks();
    check_errors_and_repeats();
    if (g_fail) return 1;
    printf("ok %d\n", g_cases);
    return 0;
}
