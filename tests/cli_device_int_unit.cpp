// Stand-alone check of the fifth flag table of pindel_amd/csrc/host/pg_cli.hpp, CLI_DEVICE_INT_FLAGS (plain g++, address +
// undefined-behaviour sanitizers, no GPU, no libpindel_pg.so): --device-classifier-int is parsed, admits -I on the device-classifier
// path and nothing else -- without it the refusal keeps its status and its text, with it -l, -s, -S, -q, -N and several devices stay
// refused.  It composes with --device-classifier-hints, --device-classifier-li and --device-classifier-listed.  Prints "ok <cases>"
// and exits 0, or says what failed and exits 1.  tests/test_cli_device_int_cpu.py builds and runs it.
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
    const char *const INT = "--device-classifier-int";
    const char *const LI = "--device-classifier-li";
    const char *const HINTS = "--device-classifier-hints";
    const char *const DC = "--device-classifier";
    const char *const NEEDS = "--device-classifier-int needs --device-classifier";
    // the one row of a table of its own: the four tables before it keep their rows
    CHECK(sizeof CLI_DEVICE_INT_FLAGS / sizeof CLI_DEVICE_INT_FLAGS[0] == 1 && sizeof CLI_DEVICE_LI_FLAGS / sizeof CLI_DEVICE_LI_FLAGS[0] == 1 &&
              sizeof CLI_DEVICE_HINT_FLAGS / sizeof CLI_DEVICE_HINT_FLAGS[0] == 1 && sizeof CLI_DEVICE_FLAGS / sizeof CLI_DEVICE_FLAGS[0] == 2,
          "rows");
    CHECK(std::string(CLI_DEVICE_INT_FLAGS[0].lg) == INT && CLI_DEVICE_INT_FLAGS[0].kind == 'u' && CLI_DEVICE_INT_FLAGS[0].sh[0] == 0, "a unary switch");
    for (const CliFlag &y : CLI_FLAGS) CHECK(std::string(INT) != y.lg, "not a row of CLI_FLAGS");
    for (const CliFlag &y : CLI_DEVICE_FLAGS) CHECK(std::string(INT) != y.lg, "not a row of CLI_DEVICE_FLAGS");
    for (const CliFlag &y : CLI_DEVICE_HINT_FLAGS) CHECK(std::string(INT) != y.lg, "not a row of CLI_DEVICE_HINT_FLAGS");
    for (const CliFlag &y : CLI_DEVICE_LI_FLAGS) CHECK(std::string(INT) != y.lg, "not a row of CLI_DEVICE_LI_FLAGS");
    // the untouched defaults
    Parsed p = parse({ "-p", "reads" });
    CHECK(p.status == 0 && !p.o.device_classifier && !p.o.device_classifier_int && !p.o.device_classifier_li && !p.o.device_classifier_hints &&
              p.o.device_classifier_listed == -1,
          "defaults: %s", p.err.c_str());
    CHECK(!p.o.S.report_interchromosomal && p.o.S.repairs == 0, "defaults of -I and --repair");
    p = parse({ "-p", "reads", "-I" });
    CHECK(p.status == 0 && p.o.S.report_interchromosomal && !p.o.device_classifier_int, "without the device classifier nothing differs");
    p = parse({ "-p", "reads", DC });
    CHECK(p.status == 0 && p.o.device_classifier && !p.o.device_classifier_int, "off by default: %s", p.err.c_str());
    // the switch with and without its optional word; alone it changes no other option
    p = parse({ "-p", "reads", DC, INT });
    CHECK(p.status == 0 && p.o.device_classifier && p.o.device_classifier_int && !p.o.S.report_interchromosomal, "%s", p.err.c_str());
    CHECK(p.o.S.Analyze_TD && p.o.S.Analyze_INV && p.o.search_rp && !p.o.use_bd && p.o.devices.size() == 1 && !p.o.device_classifier_hints &&
              !p.o.device_classifier_li && !p.o.S.Analyze_LI && !p.o.S.report_close_mapped,
          "nothing else moves");
    p = parse({ INT, "true", DC, "-M", "3" });
    CHECK(p.status == 0 && p.o.device_classifier_int && p.o.S.NumRead2ReportCutOff == 3, "%s", p.err.c_str());
    for (const char *off : { "false", "0", "F" }) {
        p = parse({ DC, INT, off });
        CHECK(p.status == 0 && p.o.device_classifier && !p.o.device_classifier_int, "%s: %s", off, p.err.c_str());
    }
    // admitted: -I, in any order and spelling, on both input routes
    p = parse({ "-p", "reads", DC, INT, "-I" });
    CHECK(p.status == 0 && p.o.S.report_interchromosomal && p.o.device_classifier_int, "-I: %s", p.err.c_str());
    p = parse({ "-I", "true", INT, "-p", "reads", DC });
    CHECK(p.status == 0 && p.o.S.report_interchromosomal, "the order does not matter: %s", p.err.c_str());
    p = parse({ "-p", "reads", DC, INT, "--report_interchromosomal_events" });
    CHECK(p.status == 0 && p.o.S.report_interchromosomal, "the long spelling: %s", p.err.c_str());
    p = parse({ "-i", "bams.txt", DC, INT, "-I", "-R", "false" });
    CHECK(p.status == 0 && p.o.S.report_interchromosomal && !p.o.search_rp, "BAM input: %s", p.err.c_str());
    p = parse({ "-p", "reads", DC, INT, "-I", "--repair", "int-pairs" });
    CHECK(p.status == 0 && p.o.S.repair(REPAIR_INT_PAIRS), "with --repair int-pairs: %s", p.err.c_str());
    p = parse({ "-p", "reads", DC, INT, "-I", "-w", "0.02" });
    CHECK(p.status == 0 && p.o.S.window_mbp == 0.02, "with -w: %s", p.err.c_str());
    // it composes with the three other switches
    p = parse({ "-i", "bams.txt", DC, INT, HINTS, "-I" });
    CHECK(p.status == 0 && p.o.search_rp && p.o.device_classifier_hints && p.o.device_classifier_int, "with hints, -R on: %s", p.err.c_str());
    p = parse({ "-p", "reads", DC, INT, HINTS, "-b", "bd.txt", "--bd-hints", "on", "-I" });
    CHECK(p.status == 0 && p.o.use_bd && p.o.S.report_interchromosomal, "with --bd-hints on: %s", p.err.c_str());
    p = parse({ "-p", "reads", DC, INT, "--device-classifier-listed", "0", "-I" });
    CHECK(p.status == 0 && p.o.device_classifier_listed == 0 && p.o.S.report_interchromosomal, "with listed: %s", p.err.c_str());
    p = parse({ "-i", "bams.txt", DC, INT, LI, HINTS, "-I", "-l", "-s" });
    CHECK(p.status == 0 && p.o.S.report_interchromosomal && p.o.S.Analyze_LI && p.o.S.report_close_mapped && p.o.device_classifier_li, "with -li -l -s: %s",
          p.err.c_str());
    // the hints' own refusals are not lifted by this switch
    p = parse({ "-i", "bams.txt", DC, INT, "-I" });
    CHECK(p.status == 2 && p.err == "--device-classifier with BAM input needs -R false: read-pair window hints are not searched on this path", "%s", p.err.c_str());
    p = parse({ "-p", "reads", DC, INT, "-b", "bd.txt", "--bd-hints", "on", "-I" });
    CHECK(p.status == 2 && p.err == "--device-classifier cannot be combined with --bd-hints on: window hints are not searched on this path", "%s", p.err.c_str());
    // without it (absent, or switched off): -I's refusal stands, same text, status 2 -- whatever other switch is given
    for (int k = 0; k < 4; k++) {
        std::vector<std::string> w = { "-p", "reads", DC, "-I" };
        if (k == 1) w.insert(w.end(), { INT, "false" });
        if (k == 2) w.push_back(LI);
        if (k == 3) w.push_back(HINTS);
        p = parse(w);
        CHECK(p.status == 2 && p.err == refusal("-I"), "%d: %s", k, p.err.c_str());
    }
    // the switch implies nothing on its own
    p = parse({ "-p", "reads", INT });
    CHECK(p.status == 2 && p.err == NEEDS, "%s", p.err.c_str());
    p = parse({ "-p", "reads", INT, "-I" });
    CHECK(p.status == 2 && p.err == NEEDS, "%s", p.err.c_str());
    p = parse({ DC, "false", INT });
    CHECK(p.status == 2 && p.err == NEEDS, "%s", p.err.c_str());
    p = parse({ "-p", "reads", INT, "false", "-I" });
    CHECK(p.status == 0 && !p.o.device_classifier_int && p.o.S.report_interchromosomal, "switched off it asks for nothing: %s", p.err.c_str());
    p = parse({ "-p", "reads", "--device-classifier-listed", "2", INT });
    CHECK(p.status == 2 && p.err == "--device-classifier-listed needs --device-classifier", "the earlier refusals come first: %s", p.err.c_str());
    p = parse({ "-p", "reads", HINTS, INT });
    CHECK(p.status == 2 && p.err == "--device-classifier-hints needs --device-classifier", "%s", p.err.c_str());
    p = parse({ "-p", "reads", LI, INT });
    CHECK(p.status == 2 && p.err == "--device-classifier-li needs --device-classifier", "%s", p.err.c_str());
    // what stays refused, with the switch or without: -l and -s need their own switch, -S, -q and -N have none
    for (int k = 0; k < 2; k++)
        for (const char *flag : { "-l", "-s", "-S", "-q", "-N" }) {
            std::vector<std::string> w = { "-p", "reads", DC, flag };
            if (k) w.push_back(INT);
            p = parse(w);
            CHECK(p.status == 2 && p.err == refusal(flag), "%d %s: %s", k, flag, p.err.c_str());
            if (k) {
                w.push_back("-I");
                p = parse(w);
                CHECK(p.status == 2 && p.err == refusal(flag), "%s beside -I: %s", flag, p.err.c_str());
            }
        }
    for (const char *flag : { "-S", "-q", "-N" }) {
        p = parse({ "-p", "reads", DC, INT, LI, "-I", "-l", "-s", flag });
        CHECK(p.status == 2 && p.err == refusal(flag), "%s beside both switches: %s", flag, p.err.c_str());
    }
    for (int k = 0; k < 2; k++) {
        std::vector<std::string> w = { "-p", "reads", DC, "-G", "0,1" };
        if (k) w.insert(w.end(), { INT, "-I" });
        p = parse(w);
        CHECK(p.status == 2 && p.err == "--device-classifier runs on one device: give -G a single device", "%d: %s", k, p.err.c_str());
    }
    p = parse({ "-p", "reads", DC, INT, "-I", "-G", "3" });
    CHECK(p.status == 0 && p.o.devices == std::vector<int>{ 3 }, "%s", p.err.c_str());
    // an unknown spelling is still unknown; the switch's word is optional, a flag behind it is not its word
    p = parse({ "--device-classifier-in" });
    CHECK(p.status == 2 && p.err == "unknown argument: --device-classifier-in", "%s", p.err.c_str());
    p = parse({ DC, INT, "-I" });
    CHECK(p.status == 0 && p.o.device_classifier_int && p.o.S.report_interchromosomal, "%s", p.err.c_str());
    if (g_fail) return 1;
    printf("ok %d\n", g_cases);
    return 0;
}
