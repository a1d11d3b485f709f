// Stand-alone check of the fourth flag table of pindel_amd/csrc/host/pg_cli.hpp, CLI_DEVICE_LI_FLAGS (plain g++, address +
// undefined-behaviour sanitizers, no GPU, no libpindel_pg.so): --device-classifier-li is parsed, admits -l and -s on the
// device-classifier path and nothing else -- without it both refusals keep their status and their text, with it -S, -I, -q, -N
// and several devices stay refused.  It composes with --device-classifier-hints and --device-classifier-listed.  Prints
// "ok <cases>" and exits 0, or says what failed and exits 1.  tests/test_cli_device_li_cpu.py builds and runs it.
#include <cstdio>
#include <cstdlib>
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
    Parsed p = { 0, "", CliOptions() };
    p.status = parse_cli((int)argv.size(), argv.data(), p.o, p.err);
    return p;
}
static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }
static std::string refusal(const char *flag)
{
    return std::string("--device-classifier cannot be combined with ") + flag + ": its report needs points or pairs this path does not deliver";
}

int main()
{
    const char *const LI = "--device-classifier-li";
    const char *const DC = "--device-classifier";
    // the one row of a table of its own: the three tables before it keep their rows
    CHECK(sizeof CLI_DEVICE_LI_FLAGS / sizeof CLI_DEVICE_LI_FLAGS[0] == 1 && sizeof CLI_DEVICE_HINT_FLAGS / sizeof CLI_DEVICE_HINT_FLAGS[0] == 1 &&
              sizeof CLI_DEVICE_FLAGS / sizeof CLI_DEVICE_FLAGS[0] == 2, "rows");
    CHECK(std::string(CLI_DEVICE_LI_FLAGS[0].lg) == LI && CLI_DEVICE_LI_FLAGS[0].kind == 'u' && CLI_DEVICE_LI_FLAGS[0].sh[0] == 0, "a unary switch");
    for (const CliFlag &y : CLI_FLAGS) CHECK(std::string(LI) != y.lg, "not a row of CLI_FLAGS");
    for (const CliFlag &y : CLI_DEVICE_FLAGS) CHECK(std::string(LI) != y.lg, "not a row of CLI_DEVICE_FLAGS");
    for (const CliFlag &y : CLI_DEVICE_HINT_FLAGS) CHECK(std::string(LI) != y.lg, "not a row of CLI_DEVICE_HINT_FLAGS");
    // the untouched defaults
    Parsed p = parse({ "-p", "reads" });
    CHECK(p.status == 0 && !p.o.device_classifier && !p.o.device_classifier_li && !p.o.device_classifier_hints && p.o.device_classifier_listed == -1,
          "defaults: %s", p.err.c_str());
    CHECK(!p.o.S.Analyze_LI && !p.o.S.report_close_mapped && !p.o.S.only_close_mapped, "defaults of -l -s -S");
    p = parse({ "-p", "reads", "-l", "-s" });
    CHECK(p.status == 0 && p.o.S.Analyze_LI && p.o.S.report_close_mapped && !p.o.device_classifier_li, "without the device classifier nothing differs");
    p = parse({ "-p", "reads", DC });
    CHECK(p.status == 0 && p.o.device_classifier && !p.o.device_classifier_li, "off by default: %s", p.err.c_str());
    // the switch with and without its optional word; alone it changes no other option
    p = parse({ "-p", "reads", DC, LI });
    CHECK(p.status == 0 && p.o.device_classifier && p.o.device_classifier_li && !p.o.S.Analyze_LI && !p.o.S.report_close_mapped, "%s", p.err.c_str());
    CHECK(p.o.S.Analyze_TD && p.o.S.Analyze_INV && p.o.search_rp && !p.o.use_bd && p.o.devices.size() == 1 && !p.o.device_classifier_hints, "nothing else moves");
    p = parse({ LI, "true", DC, "-M", "3" });
    CHECK(p.status == 0 && p.o.device_classifier_li && p.o.S.NumRead2ReportCutOff == 3, "%s", p.err.c_str());
    for (const char *off : { "false", "0", "F" }) {
        p = parse({ DC, LI, off });
        CHECK(p.status == 0 && p.o.device_classifier && !p.o.device_classifier_li, "%s: %s", off, p.err.c_str());
    }
    // admitted: -l, -s and both, in any order, on both input routes
    p = parse({ "-p", "reads", DC, LI, "-l" });
    CHECK(p.status == 0 && p.o.S.Analyze_LI && !p.o.S.report_close_mapped && p.o.device_classifier_li, "-l: %s", p.err.c_str());
    p = parse({ "-p", "reads", DC, LI, "-s" });
    CHECK(p.status == 0 && !p.o.S.Analyze_LI && p.o.S.report_close_mapped, "-s: %s", p.err.c_str());
    p = parse({ "-p", "reads", DC, LI, "-l", "-s" });
    CHECK(p.status == 0 && p.o.S.Analyze_LI && p.o.S.report_close_mapped, "-l -s: %s", p.err.c_str());
    p = parse({ "-s", "-l", "true", LI, "-p", "reads", DC });
    CHECK(p.status == 0 && p.o.S.Analyze_LI && p.o.S.report_close_mapped, "the order does not matter: %s", p.err.c_str());
    p = parse({ "-p", "reads", DC, LI, "--report_long_insertions", "--report_close_mapped_reads" });
    CHECK(p.status == 0 && p.o.S.Analyze_LI && p.o.S.report_close_mapped, "the long spellings: %s", p.err.c_str());
    p = parse({ "-i", "bams.txt", DC, LI, "-l", "-s", "-R", "false" });
    CHECK(p.status == 0 && p.o.S.Analyze_LI && !p.o.search_rp, "BAM input: %s", p.err.c_str());
    // it composes with the two other switches
    p = parse({ "-i", "bams.txt", DC, LI, "--device-classifier-hints", "-l", "-s" });
    CHECK(p.status == 0 && p.o.search_rp && p.o.device_classifier_hints && p.o.device_classifier_li, "with hints, -R on: %s", p.err.c_str());
    p = parse({ "-p", "reads", DC, LI, "--device-classifier-hints", "-b", "bd.txt", "--bd-hints", "on", "-l" });
    CHECK(p.status == 0 && p.o.use_bd && p.o.S.Analyze_LI, "with --bd-hints on: %s", p.err.c_str());
    p = parse({ "-p", "reads", DC, LI, "--device-classifier-listed", "0", "-l", "-s" });
    CHECK(p.status == 0 && p.o.device_classifier_listed == 0 && p.o.S.Analyze_LI, "with listed: %s", p.err.c_str());
    // the hints' own refusals are not lifted by this switch
    p = parse({ "-i", "bams.txt", DC, LI, "-l" });
    CHECK(p.status == 2 && p.err == "--device-classifier with BAM input needs -R false: read-pair window hints are not searched on this path", "%s", p.err.c_str());
    p = parse({ "-p", "reads", DC, LI, "-b", "bd.txt", "--bd-hints", "on", "-l" });
    CHECK(p.status == 2 && p.err == "--device-classifier cannot be combined with --bd-hints on: window hints are not searched on this path", "%s", p.err.c_str());
    // without it (absent, or switched off): both refusals stand, same text, status 2
    for (int k = 0; k < 2; k++)
        for (const char *flag : { "-l", "-s" }) {
            std::vector<std::string> w = { "-p", "reads", DC, flag };
            if (k) w.insert(w.end(), { LI, "false" });
            p = parse(w);
            CHECK(p.status == 2 && p.err == refusal(flag), "%d %s: %s", k, flag, p.err.c_str());
        }
    p = parse({ "-p", "reads", DC, "-l", "-s" });
    CHECK(p.status == 2 && p.err == refusal("-l"), "-l is named first: %s", p.err.c_str());
    p = parse({ "-p", "reads", DC, "--device-classifier-hints", "-s" });
    CHECK(p.status == 2 && p.err == refusal("-s"), "the hints switch does not admit it: %s", p.err.c_str());
    // the switch implies nothing on its own
    p = parse({ "-p", "reads", LI });
    CHECK(p.status == 2 && p.err == "--device-classifier-li needs --device-classifier", "%s", p.err.c_str());
    p = parse({ "-p", "reads", LI, "-l", "-s" });
    CHECK(p.status == 2 && p.err == "--device-classifier-li needs --device-classifier", "%s", p.err.c_str());
    p = parse({ DC, "false", LI });
    CHECK(p.status == 2 && p.err == "--device-classifier-li needs --device-classifier", "%s", p.err.c_str());
    p = parse({ "-p", "reads", LI, "false", "-l" });
    CHECK(p.status == 0 && !p.o.device_classifier_li && p.o.S.Analyze_LI, "switched off it asks for nothing: %s", p.err.c_str());
    p = parse({ "-p", "reads", "--device-classifier-listed", "2", LI });
    CHECK(p.status == 2 && p.err == "--device-classifier-listed needs --device-classifier", "the earlier refusals come first: %s", p.err.c_str());
    p = parse({ "-p", "reads", "--device-classifier-hints", LI });
    CHECK(p.status == 2 && p.err == "--device-classifier-hints needs --device-classifier", "%s", p.err.c_str());
    // what stays refused, with the switch or without
    for (int k = 0; k < 2; k++)
        for (const char *flag : { "-S", "-I", "-q", "-N" }) {
            std::vector<std::string> w = { "-p", "reads", DC, flag };
            if (k) w.push_back(LI);
            p = parse(w);
            CHECK(p.status == 2 && p.err == refusal(flag), "%d %s: %s", k, flag, p.err.c_str());
            if (k) {
                w.insert(w.end(), { "-l", "-s" });
                p = parse(w);
                CHECK(p.status == 2 && p.err == refusal(flag), "%s beside -l -s: %s", flag, p.err.c_str());
            }
        }
    for (int k = 0; k < 2; k++) {
        std::vector<std::string> w = { "-p", "reads", DC, "-G", "0,1" };
        if (k) w.insert(w.end(), { LI, "-l" });
        p = parse(w);
        CHECK(p.status == 2 && p.err == "--device-classifier runs on one device: give -G a single device", "%d: %s", k, p.err.c_str());
    }
    p = parse({ "-p", "reads", DC, LI, "-l", "-G", "3" });
    CHECK(p.status == 0 && p.o.devices == std::vector<int>{ 3 }, "%s", p.err.c_str());
    // an unknown spelling is still unknown; the switch's word is optional, a flag behind it is not its word
    p = parse({ "--device-classifier-l" });
    CHECK(p.status == 2 && p.err == "unknown argument: --device-classifier-l", "%s", p.err.c_str());
    p = parse({ DC, LI, "-l" });
    CHECK(p.status == 0 && p.o.device_classifier_li && p.o.S.Analyze_LI, "%s", p.err.c_str());
    CHECK(has(refusal("-l"), "with -l:"), "the text the existing checks look for");
    if (g_fail) return 1;
    printf("ok %d\n", g_cases);
    return 0;
}
