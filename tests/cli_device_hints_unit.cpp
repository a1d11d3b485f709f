// Stand-alone check of the third flag table of pindel_amd/csrc/host/pg_cli.hpp, CLI_DEVICE_HINT_FLAGS (plain g++, address +
// undefined-behaviour sanitizers, no GPU, no libpindel_pg.so): --device-classifier-hints is parsed, admits window hints on the
// device-classifier path (--bd-hints on; BAM input with -R on) and nothing else -- without it every refusal keeps its status and
// its text, with it the reports that need points stay refused.  Prints "ok <cases>" and exits 0, or says what failed and exits 1.
// tests/test_resident_hints_cpu.py builds and runs it.
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

int main()
{
    const char *const HINTS = "--device-classifier-hints";
    // a row of a table of its own: the two tables before it keep their rows
    CHECK(sizeof CLI_DEVICE_HINT_FLAGS / sizeof CLI_DEVICE_HINT_FLAGS[0] == 1 && sizeof CLI_DEVICE_FLAGS / sizeof CLI_DEVICE_FLAGS[0] == 2, "rows");
    for (const CliFlag &y : CLI_FLAGS) CHECK(std::string(HINTS) != y.lg, "not a row of CLI_FLAGS");
    for (const CliFlag &y : CLI_DEVICE_FLAGS) CHECK(std::string(HINTS) != y.lg, "not a row of CLI_DEVICE_FLAGS");
    // off by default; the switch with and without its optional word
    Parsed p = parse({ "-p", "reads", "--device-classifier" });
    CHECK(p.status == 0 && p.o.device_classifier && !p.o.device_classifier_hints, "default: %s", p.err.c_str());
    p = parse({ "-p", "reads", "--device-classifier", HINTS });
    CHECK(p.status == 0 && p.o.device_classifier && p.o.device_classifier_hints && p.o.device_classifier_listed == -1, "%s", p.err.c_str());
    CHECK(p.o.S.Analyze_TD && p.o.S.Analyze_INV && p.o.search_rp && !p.o.use_bd && p.o.devices.size() == 1, "nothing else moves");
    p = parse({ HINTS, "true", "--device-classifier", "-M", "3" });
    CHECK(p.status == 0 && p.o.device_classifier_hints && p.o.S.NumRead2ReportCutOff == 3, "%s", p.err.c_str());
    for (const char *off : { "false", "0", "F" }) {
        p = parse({ "--device-classifier", HINTS, off });
        CHECK(p.status == 0 && p.o.device_classifier && !p.o.device_classifier_hints, "%s: %s", off, p.err.c_str());
    }
    p = parse({ "--device-classifier", HINTS, "--device-classifier-listed", "2" });
    CHECK(p.status == 0 && p.o.device_classifier_hints && p.o.device_classifier_listed == 2, "%s", p.err.c_str());
    // with it: window hints are admitted, on both routes
    p = parse({ "-p", "reads", "--device-classifier", HINTS, "-b", "bd.txt", "--bd-hints", "on" });
    CHECK(p.status == 0 && p.o.use_bd && p.o.device_classifier && p.o.device_classifier_hints, "%s", p.err.c_str());
    p = parse({ "-b", "bd.txt", "--bd-hints", "on", HINTS, "--device-classifier", "-p", "reads" });
    CHECK(p.status == 0 && p.o.use_bd, "the order does not matter: %s", p.err.c_str());
    p = parse({ "-i", "bams.txt", "--device-classifier", HINTS });
    CHECK(p.status == 0 && p.o.search_rp && p.o.bam_config == "bams.txt", "%s", p.err.c_str());
    p = parse({ "-i", "bams.txt", "--device-classifier", HINTS, "-R" });
    CHECK(p.status == 0 && p.o.search_rp, "%s", p.err.c_str());
    p = parse({ "-i", "bams.txt", "--device-classifier", HINTS, "-R", "false" });
    CHECK(p.status == 0 && !p.o.search_rp, "%s", p.err.c_str());
    p = parse({ "-i", "bams.txt", "-b", "bd.txt", "--device-classifier", HINTS });
    CHECK(p.status == 0, "%s", p.err.c_str());
    // without it (absent, or switched off): both keep status 2 and their texts
    for (int k = 0; k < 2; k++) {
        std::vector<std::string> w = { "-p", "reads", "--device-classifier", "-b", "bd.txt", "--bd-hints", "on" };
        std::vector<std::string> v = { "-i", "bams.txt", "--device-classifier" };
        if (k) {
            w.insert(w.end(), { HINTS, "false" });
            v.insert(v.end(), { HINTS, "false" });
        }
        p = parse(w);
        CHECK(p.status == 2 && p.err == "--device-classifier cannot be combined with --bd-hints on: window hints are not searched on this path",
              "%d: %s", k, p.err.c_str());
        p = parse(v);
        CHECK(p.status == 2 && p.err == "--device-classifier with BAM input needs -R false: read-pair window hints are not searched on this path",
              "%d: %s", k, p.err.c_str());
    }
    // the switch implies nothing on its own
    p = parse({ "-p", "reads", HINTS });
    CHECK(p.status == 2 && p.err == "--device-classifier-hints needs --device-classifier", "%s", p.err.c_str());
    p = parse({ "-p", "reads", HINTS, "-b", "bd.txt", "--bd-hints", "on" });
    CHECK(p.status == 2 && has(p.err, "--device-classifier-hints needs --device-classifier"), "%s", p.err.c_str());
    p = parse({ "--device-classifier", "false", HINTS });
    CHECK(p.status == 2 && has(p.err, "needs --device-classifier"), "%s", p.err.c_str());
    p = parse({ "-p", "reads", HINTS, "false" });
    CHECK(p.status == 0 && !p.o.device_classifier_hints, "switched off it asks for nothing: %s", p.err.c_str());
    p = parse({ "-p", "reads", "--device-classifier-listed", "2", HINTS });
    CHECK(p.status == 2 && has(p.err, "--device-classifier-listed needs --device-classifier"), "the earlier refusal comes first: %s", p.err.c_str());
    // the reports this path does not deliver stay refused, hints or not
    for (const char *flag : { "-I", "-l", "-s", "-S", "-q", "-N" }) {
        p = parse({ "-p", "reads", "--device-classifier", HINTS, flag });
        CHECK(p.status == 2 && has(p.err, "--device-classifier") && has(p.err, (std::string("with ") + flag + ":").c_str()), "%s: %s", flag, p.err.c_str());
        p = parse({ "-p", "reads", "--device-classifier", HINTS, "-b", "bd.txt", "--bd-hints", "on", flag });
        CHECK(p.status == 2 && has(p.err, (std::string("with ") + flag + ":").c_str()), "%s with hints: %s", flag, p.err.c_str());
        p = parse({ "-i", "bams.txt", "--device-classifier", HINTS, flag });
        CHECK(p.status == 2 && has(p.err, (std::string("with ") + flag + ":").c_str()), "%s, BAM input: %s", flag, p.err.c_str());
    }
    p = parse({ "-p", "reads", "--device-classifier", HINTS, "-G", "0,1" });
    CHECK(p.status == 2 && has(p.err, "--device-classifier") && has(p.err, "one device"), "%s", p.err.c_str());
    p = parse({ "-i", "bams.txt", "--device-classifier", HINTS, "-G", "0,1" });
    CHECK(p.status == 2 && has(p.err, "one device"), "%s", p.err.c_str());
    p = parse({ "-p", "reads", "--device-classifier", HINTS, "-G", "3" });
    CHECK(p.status == 0 && p.o.devices == std::vector<int>{ 3 }, "%s", p.err.c_str());
    // an unknown spelling is still unknown
    p = parse({ "--device-classifier-hint" });
    CHECK(p.status == 2 && p.err == "unknown argument: --device-classifier-hint", "%s", p.err.c_str());
    if (g_fail) return 1;
    printf("ok %d\n", g_cases);
    return 0;
}
