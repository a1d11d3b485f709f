// Stand-alone check of the sixth flag table of pindel_amd/csrc/host/pg_cli.hpp, CLI_DEVICE_DD_FLAGS (plain g++, address +
// undefined-behaviour sanitizers, no GPU, no libpindel_pg.so): --device-classifier-dd is parsed, admits -q on the device-classifier
// path and nothing else -- without it the refusal keeps its status and its text, with it -l, -s, -I without their own switches, -S,
// -N and several devices stay refused.  It composes with --device-classifier-hints, -li, -int and -listed and with -R false.
// Prints "ok <cases>" and exits 0, or says what failed and exits 1.  tests/test_cli_device_dd_cpu.py builds and runs it.
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
static std::string refusal(const char *flag)
{
    return std::string("--device-classifier cannot be combined with ") + flag + ": its report needs points or pairs this path does not deliver";
}

int main()
{
    const char *const DD = "--device-classifier-dd";
    const char *const INT = "--device-classifier-int";
    const char *const LI = "--device-classifier-li";
    const char *const HINTS = "--device-classifier-hints";
    const char *const DC = "--device-classifier";
    const char *const NEEDS = "--device-classifier-dd needs --device-classifier";
    // the one row of a table of its own: the five tables before it keep their rows
    CHECK(sizeof CLI_DEVICE_DD_FLAGS / sizeof CLI_DEVICE_DD_FLAGS[0] == 1 && sizeof CLI_DEVICE_INT_FLAGS / sizeof CLI_DEVICE_INT_FLAGS[0] == 1 &&
              sizeof CLI_DEVICE_LI_FLAGS / sizeof CLI_DEVICE_LI_FLAGS[0] == 1 && sizeof CLI_DEVICE_HINT_FLAGS / sizeof CLI_DEVICE_HINT_FLAGS[0] == 1 &&
              sizeof CLI_DEVICE_FLAGS / sizeof CLI_DEVICE_FLAGS[0] == 2,
          "rows");
    CHECK(std::string(CLI_DEVICE_DD_FLAGS[0].lg) == DD && CLI_DEVICE_DD_FLAGS[0].kind == 'u' && CLI_DEVICE_DD_FLAGS[0].sh[0] == 0, "a unary switch");
    for (const CliFlag &y : CLI_FLAGS) CHECK(std::string(DD) != y.lg, "not a row of CLI_FLAGS");
    for (const CliFlag &y : CLI_DEVICE_FLAGS) CHECK(std::string(DD) != y.lg, "not a row of CLI_DEVICE_FLAGS");
    for (const CliFlag &y : CLI_DEVICE_HINT_FLAGS) CHECK(std::string(DD) != y.lg, "not a row of CLI_DEVICE_HINT_FLAGS");
    for (const CliFlag &y : CLI_DEVICE_LI_FLAGS) CHECK(std::string(DD) != y.lg, "not a row of CLI_DEVICE_LI_FLAGS");
    for (const CliFlag &y : CLI_DEVICE_INT_FLAGS) CHECK(std::string(DD) != y.lg, "not a row of CLI_DEVICE_INT_FLAGS");
    // the untouched defaults
    Parsed p = parse({ "-i", "bams.txt" });
    CHECK(p.status == 0 && !p.o.device_classifier && !p.o.device_classifier_dd && !p.o.device_classifier_int && !p.o.device_classifier_li &&
              !p.o.device_classifier_hints && p.o.device_classifier_listed == -1 && !p.o.detect_dd,
          "defaults: %s", p.err.c_str());
    p = parse({ "-i", "bams.txt", "-q" });
    CHECK(p.status == 0 && p.o.detect_dd && !p.o.device_classifier_dd, "without the device classifier nothing differs");
    p = parse({ "-p", "reads", DC });
    CHECK(p.status == 0 && p.o.device_classifier && !p.o.device_classifier_dd, "off by default: %s", p.err.c_str());
    // the switch with and without its optional word; alone it changes no other option
    p = parse({ "-p", "reads", DC, DD });
    CHECK(p.status == 0 && p.o.device_classifier && p.o.device_classifier_dd && !p.o.detect_dd, "%s", p.err.c_str());
    CHECK(p.o.S.Analyze_TD && p.o.S.Analyze_INV && p.o.search_rp && !p.o.use_bd && p.o.devices.size() == 1 && !p.o.device_classifier_hints &&
              !p.o.device_classifier_li && !p.o.device_classifier_int && !p.o.S.Analyze_LI && !p.o.S.report_close_mapped && !p.o.S.report_interchromosomal,
          "nothing else moves");
    CHECK(p.o.dd.min_bp_support == 3 && p.o.dd.min_map_distance == 8000 && !p.o.dd.report_dup_reads, "the DD flags keep their defaults");
    p = parse({ DD, "true", DC, "-M", "3" });
    CHECK(p.status == 0 && p.o.device_classifier_dd && p.o.S.NumRead2ReportCutOff == 3, "%s", p.err.c_str());
    for (const char *off : { "false", "0", "F" }) {
        p = parse({ DC, DD, off });
        CHECK(p.status == 0 && p.o.device_classifier && !p.o.device_classifier_dd, "%s: %s", off, p.err.c_str());
    }
    // admitted: -q, in any order and spelling, on both input routes (Pindel-text input writes the empty _DD and the note)
    p = parse({ "-i", "bams.txt", DC, DD, "-q", "-R", "false" });
    CHECK(p.status == 0 && p.o.detect_dd && p.o.device_classifier_dd && !p.o.search_rp, "-q: %s", p.err.c_str());
    p = parse({ "-q", DD, "-R", "false", "-i", "bams.txt", DC });
    CHECK(p.status == 0 && p.o.detect_dd, "the order does not matter: %s", p.err.c_str());
    p = parse({ "-i", "bams.txt", DC, DD, "--detect_DD", "-R", "false" });
    CHECK(p.status == 0 && p.o.detect_dd, "the long spelling: %s", p.err.c_str());
    p = parse({ "-p", "reads", DC, DD, "-q" });
    CHECK(p.status == 0 && p.o.detect_dd, "Pindel-text input: %s", p.err.c_str());
    p = parse({ "-i", "bams.txt", DC, DD, "-q", "-R", "false", "--MIN_DD_MAP_DISTANCE", "400", "--MIN_DD_BREAKPOINT_SUPPORT", "2",
                "--DD_REPORT_DUPLICATION_READS" });
    CHECK(p.status == 0 && p.o.dd.min_map_distance == 400 && p.o.dd.min_bp_support == 2 && p.o.dd.report_dup_reads, "the DD flags: %s", p.err.c_str());
    p = parse({ "-i", "bams.txt", DC, DD, "-q", "-R", "false", "-T", "8", "-w", "0.02" });
    CHECK(p.status == 0 && p.o.S.window_mbp == 0.02, "with -T and -w: %s", p.err.c_str());
    // it composes with the four other switches
    p = parse({ "-i", "bams.txt", DC, DD, HINTS, "-q" });
    CHECK(p.status == 0 && p.o.search_rp && p.o.device_classifier_hints && p.o.device_classifier_dd, "with hints, -R on: %s", p.err.c_str());
    p = parse({ "-i", "bams.txt", DC, DD, HINTS, LI, "-q", "-l", "-s" });
    CHECK(p.status == 0 && p.o.detect_dd && p.o.S.Analyze_LI && p.o.S.report_close_mapped && p.o.device_classifier_li, "with -li -l -s: %s", p.err.c_str());
    p = parse({ "-i", "bams.txt", DC, DD, HINTS, INT, "-q", "-I" });
    CHECK(p.status == 0 && p.o.detect_dd && p.o.S.report_interchromosomal && p.o.device_classifier_int, "with -int -I: %s", p.err.c_str());
    p = parse({ "-i", "bams.txt", DC, DD, "--device-classifier-listed", "0", "-q", "-R", "false" });
    CHECK(p.status == 0 && p.o.device_classifier_listed == 0 && p.o.detect_dd, "with listed: %s", p.err.c_str());
    p = parse({ "-i", "bams.txt", DC, DD, HINTS, LI, INT, "--device-classifier-listed", "2", "-q", "-I", "-l", "-s" });
    CHECK(p.status == 0 && p.o.detect_dd && p.o.S.report_interchromosomal && p.o.S.Analyze_LI && p.o.S.report_close_mapped, "all five: %s", p.err.c_str());
    // the hints' own refusals are not lifted by this switch
    p = parse({ "-i", "bams.txt", DC, DD, "-q" });
    CHECK(p.status == 2 && p.err == "--device-classifier with BAM input needs -R false: read-pair window hints are not searched on this path", "%s", p.err.c_str());
    p = parse({ "-p", "reads", DC, DD, "-b", "bd.txt", "--bd-hints", "on", "-q" });
    CHECK(p.status == 2 && p.err == "--device-classifier cannot be combined with --bd-hints on: window hints are not searched on this path", "%s", p.err.c_str());
    // without it (absent, or switched off): -q's refusal stands, same text, status 2 -- whatever other switch is given
    for (int k = 0; k < 5; k++) {
        std::vector<std::string> w = { "-p", "reads", DC, "-q" };
        if (k == 1) w.insert(w.end(), { DD, "false" });
        if (k == 2) w.push_back(LI);
        if (k == 3) w.push_back(HINTS);
        if (k == 4) w.push_back(INT);
        p = parse(w);
        CHECK(p.status == 2 && p.err == refusal("-q"), "%d: %s", k, p.err.c_str());
    }
    // the switch implies nothing on its own; the earlier switches' refusals come first, -int's last among them
    p = parse({ "-p", "reads", DD });
    CHECK(p.status == 2 && p.err == NEEDS, "%s", p.err.c_str());
    p = parse({ "-i", "bams.txt", DD, "-q" });
    CHECK(p.status == 2 && p.err == NEEDS, "%s", p.err.c_str());
    p = parse({ DC, "false", DD });
    CHECK(p.status == 2 && p.err == NEEDS, "%s", p.err.c_str());
    p = parse({ "-i", "bams.txt", DD, "false", "-q" });
    CHECK(p.status == 0 && !p.o.device_classifier_dd && p.o.detect_dd, "switched off it asks for nothing: %s", p.err.c_str());
    p = parse({ "-p", "reads", "--device-classifier-listed", "2", DD });
    CHECK(p.status == 2 && p.err == "--device-classifier-listed needs --device-classifier", "%s", p.err.c_str());
    p = parse({ "-p", "reads", HINTS, DD });
    CHECK(p.status == 2 && p.err == "--device-classifier-hints needs --device-classifier", "%s", p.err.c_str());
    p = parse({ "-p", "reads", LI, DD });
    CHECK(p.status == 2 && p.err == "--device-classifier-li needs --device-classifier", "%s", p.err.c_str());
    p = parse({ "-p", "reads", DD, INT });
    CHECK(p.status == 2 && p.err == "--device-classifier-int needs --device-classifier", "the check comes after the -int one: %s", p.err.c_str());
    // what stays refused, with the switch or without: -l, -s and -I need their own switches, -S and -N have none
    for (int k = 0; k < 2; k++)
        for (const char *flag : { "-l", "-s", "-S", "-I", "-N" }) {
            std::vector<std::string> w = { "-p", "reads", DC, flag };
            if (k) w.push_back(DD);
            p = parse(w);
            CHECK(p.status == 2 && p.err == refusal(flag), "%d %s: %s", k, flag, p.err.c_str());
            if (k) {
                w.push_back("-q");
                p = parse(w);
                CHECK(p.status == 2 && p.err == refusal(flag), "%s beside -q: %s", flag, p.err.c_str());
            }
        }
    for (const char *flag : { "-S", "-N" }) {
        p = parse({ "-p", "reads", DC, DD, INT, LI, "-q", "-I", "-l", "-s", flag });
        CHECK(p.status == 2 && p.err == refusal(flag), "%s beside every switch: %s", flag, p.err.c_str());
    }
    for (int k = 0; k < 2; k++) {
        std::vector<std::string> w = { "-p", "reads", DC, "-G", "0,0" };
        if (k) w.insert(w.end(), { DD, "-q" });
        p = parse(w);
        CHECK(p.status == 2 && p.err == "--device-classifier runs on one device: give -G a single device", "%d: %s", k, p.err.c_str());
    }
    p = parse({ "-p", "reads", DC, DD, "-q", "-G", "3" });
    CHECK(p.status == 0 && p.o.devices == std::vector<int>{ 3 }, "%s", p.err.c_str());
    // an unknown spelling is still unknown; the switch's word is optional, a flag behind it is not its word
    p = parse({ "--device-classifier-d" });
    CHECK(p.status == 2 && p.err == "unknown argument: --device-classifier-d", "%s", p.err.c_str());
    p = parse({ DC, DD, "-q" });
    CHECK(p.status == 0 && p.o.device_classifier_dd && p.o.detect_dd, "%s", p.err.c_str());
    if (g_fail) return 1;
    printf("ok %d\n", g_cases);
    return 0;
}
