// Stand-alone check of the second flag table of pindel_amd/csrc/host/pg_cli.hpp, CLI_DEVICE_FLAGS (plain g++, address +
// undefined-behaviour sanitizers, no GPU, no libpindel_pg.so): --device-classifier and --device-classifier-listed are parsed, touch
// nothing else, and every combination the path does not deliver is refused with status 2 and a text that names the flag.
// Prints "ok <cases>" and exits 0, or says what failed and exits 1.  tests/test_cli_device_flags_cpu.py builds and runs it.
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
    CHECK(sizeof CLI_DEVICE_FLAGS / sizeof CLI_DEVICE_FLAGS[0] == 2, "two rows");
    for (const CliFlag &x : CLI_DEVICE_FLAGS)
        for (const CliFlag &y : CLI_FLAGS) CHECK(std::string(x.lg) != y.lg && !x.sh[0], "%s is a row of its own table only", x.lg);
    // defaults: off, no cut; the plain command line is untouched
    Parsed p = parse({ "-f", "r.fa", "-p", "reads", "-o", "out" });
    CHECK(p.status == 0 && !p.o.device_classifier && p.o.device_classifier_listed == -1, "defaults: %s", p.err.c_str());
    // the switch, with and without its optional word
    p = parse({ "-p", "reads", "--device-classifier" });
    CHECK(p.status == 0 && p.o.device_classifier && p.o.device_classifier_listed == -1 && p.o.reads_path == "reads", "%s", p.err.c_str());
    CHECK(p.o.S.Analyze_TD && p.o.S.Analyze_INV && p.o.search_rp && p.o.devices.size() == 1, "nothing else moves");
    p = parse({ "--device-classifier", "false" });
    CHECK(p.status == 0 && !p.o.device_classifier, "%s", p.err.c_str());
    p = parse({ "--device-classifier", "true", "-M", "3" });
    CHECK(p.status == 0 && p.o.device_classifier && p.o.S.NumRead2ReportCutOff == 3, "%s", p.err.c_str());
    // the number of listed pairs
    for (int k = 0; k <= 4; k++) {
        p = parse({ "--device-classifier", "--device-classifier-listed", std::to_string(k) });
        CHECK(p.status == 0 && p.o.device_classifier && p.o.device_classifier_listed == k, "listed %d: %s", k, p.err.c_str());
        p = parse({ "--device-classifier-listed", std::to_string(k), "--device-classifier" });
        CHECK(p.status == 0 && p.o.device_classifier_listed == k, "the order of the two does not matter: %s", p.err.c_str());
    }
    for (const char *bad : { "5", "17" }) {
        p = parse({ "--device-classifier", "--device-classifier-listed", bad });
        CHECK(p.status == 2 && has(p.err, "--device-classifier-listed") && has(p.err, "0 to 4"), "%s: %s", bad, p.err.c_str());
    }
    p = parse({ "--device-classifier", "--device-classifier-listed", "-1" });
    CHECK(p.status == 2 && has(p.err, "--device-classifier-listed"), "%s", p.err.c_str());
    p = parse({ "--device-classifier", "--device-classifier-listed", "two" });
    CHECK(p.status == 2 && has(p.err, "--device-classifier-listed") && has(p.err, "not a number"), "%s", p.err.c_str());
    p = parse({ "--device-classifier", "--device-classifier-listed" });
    CHECK(p.status == 2 && has(p.err, "--device-classifier-listed") && has(p.err, "lacking"), "%s", p.err.c_str());
    // --device-classifier-listed implies nothing on its own
    p = parse({ "-p", "reads", "--device-classifier-listed", "2" });
    CHECK(p.status == 2 && has(p.err, "--device-classifier-listed needs --device-classifier"), "%s", p.err.c_str());
    p = parse({ "--device-classifier", "false", "--device-classifier-listed", "2" });
    CHECK(p.status == 2 && has(p.err, "needs --device-classifier"), "%s", p.err.c_str());
    // the reports this path does not deliver
    for (const char *flag : { "-l", "-s", "-S", "-I", "-q", "-N" }) {
        p = parse({ "-p", "reads", "--device-classifier", flag });
        CHECK(p.status == 2 && has(p.err, "--device-classifier") && has(p.err, (std::string("with ") + flag + ":").c_str()), "%s: %s", flag, p.err.c_str());
        p = parse({ flag, "--device-classifier", "-p", "reads" });
        CHECK(p.status == 2 && has(p.err, "--device-classifier"), "%s in front: %s", flag, p.err.c_str());
        if (std::string(flag) != "-q") {                       // (-q is on whatever its word)
            p = parse({ "-p", "reads", "--device-classifier", flag, "false" });
            CHECK(p.status == 0, "%s false is no refusal: %s", flag, p.err.c_str());
        }
        p = parse({ "-p", "reads", flag });
        CHECK(p.status == 0, "%s alone: %s", flag, p.err.c_str());
    }
    // live window hints
    p = parse({ "-p", "reads", "--device-classifier", "-b", "bd.txt", "--bd-hints", "on" });
    CHECK(p.status == 2 && has(p.err, "--device-classifier") && has(p.err, "--bd-hints on"), "%s", p.err.c_str());
    p = parse({ "-p", "reads", "--device-classifier", "-b", "bd.txt" });
    CHECK(p.status == 0, "-b without --bd-hints on: %s", p.err.c_str());
    p = parse({ "-i", "bams.txt", "--device-classifier" });
    CHECK(p.status == 2 && has(p.err, "--device-classifier") && has(p.err, "-R false"), "%s", p.err.c_str());
    p = parse({ "-i", "bams.txt", "--device-classifier", "-R", "false" });
    CHECK(p.status == 0 && p.o.device_classifier && !p.o.search_rp, "%s", p.err.c_str());
    p = parse({ "-p", "reads", "--device-classifier", "-R" });
    CHECK(p.status == 0, "-R means nothing for Pindel-text input: %s", p.err.c_str());
    // one device
    p = parse({ "-p", "reads", "--device-classifier", "-G", "0,1" });
    CHECK(p.status == 2 && has(p.err, "--device-classifier") && has(p.err, "one device"), "%s", p.err.c_str());
    p = parse({ "-p", "reads", "--device-classifier", "-G", "3" });
    CHECK(p.status == 0 && p.o.devices == std::vector<int>{ 3 }, "%s", p.err.c_str());
    p = parse({ "-p", "reads", "-G", "0,1" });
    CHECK(p.status == 0 && p.o.devices.size() == 2, "without the flag -G 0,1 stands: %s", p.err.c_str());
    // an unknown spelling is still unknown
    p = parse({ "--device-classifie" });
    CHECK(p.status == 2 && p.err == "unknown argument: --device-classifie", "%s", p.err.c_str());
    if (g_fail) return 1;
    printf("ok %d\n", g_cases);
    return 0;
}
