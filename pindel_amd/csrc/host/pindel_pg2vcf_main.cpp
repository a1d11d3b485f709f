// pindel_pg2vcf -- Pindel's pindel2vcf: the _D, _SI, _LI, _INV and _TD reports of a run -> one VCF 4.0 file.
//   pindel_pg2vcf -r ref.fa -R <reference name> -d <date> (-p report | -P prefix) [-v out.vcf] [filters]
// Every flag of the reference converter, short and long, with its defaults (createParameters,
// src/pindel2vcf.cpp:1982-2047); the conversion itself is pg_vcf.cpp.  Like the reference's readParameters (2061-2098),
// a flag's value may not start with '-', and a yes/no flag takes an optional value (f... or 0 for no).  Unlike it, an
// unknown flag or a missing value is an error: the reference stops reading its arguments there and runs on.
// Exit status 0, or 1 for a usage error or a failed conversion (checkParameters, 2135-2162).
#include <cstdio>
#include <cstdlib>
#include <cctype>
#include <iostream>
#include <string>
#include <vector>

#include "pg_vcf.hpp"

namespace {

enum Kind { STR, INT, FLOAT, BOOL };

struct Flag {
    const char *short_name, *long_name;
    Kind kind;
    void *target;
    const char *help;
    bool required;
    bool set;
};

void print_help(const std::vector<Flag> &flags)
{
    std::cout << "\npindel_pg2vcf: Pindel reports (_D _SI _LI _INV _TD) to VCF 4.0, byte for byte as pindel2vcf 0.6.3\n\n"
              << "Usage:  pindel_pg2vcf -r <reference.fa> -R <reference name> -d <date> (-p <report> | -P <prefix>) [-v <out.vcf>]\n\n"
              << "        -P <prefix> reads <prefix>_D, _SI, _LI, _INV and _TD as one input; a report that is missing is skipped.\n"
              << "        Without -v the output is <report>.vcf or <prefix>.vcf.\n\n";
    for (const Flag &f : flags)
        std::cout << "  " << f.short_name << "/" << f.long_name << "  " << f.help << (f.required ? " (required)" : "") << "\n";
    std::cout << "\n";
}

}  // namespace

int main(int argc, char **argv)
{
    pgh::VcfOptions o;
    bool help = false;
    std::vector<Flag> flags = {
        { "-r", "--reference", STR, &o.reference, "FASTA file of the reference genome", true, false },
        { "-R", "--reference_name", STR, &o.reference_name, "name and version of the reference genome (##reference=)", true, false },
        { "-d", "--reference_date", STR, &o.reference_date, "date of that reference version (##fileDate=)", true, false },
        { "-p", "--pindel_output", STR, &o.report, "one Pindel report", false, false },
        { "-P", "--pindel_output_root", STR, &o.prefix, "prefix of a run's reports: <prefix>_D, _SI, _LI, _INV, _TD", false, false },
        { "-v", "--vcf", STR, &o.vcf, "output VCF (default: <report>.vcf or <prefix>.vcf)", false, false },
        { "-c", "--chromosome", STR, &o.chromosome, "convert only this chromosome (default: all, in FASTA order)", false, false },
        { "-w", "--window_size", INT, &o.window_size, "window in millions of bases in which events are sorted (default 300)", false, false },
        { "-mc", "--min_coverage", INT, &o.min_coverage, "reads (event + reference) needed for a genotype other than 0/0 (default 10)", false, false },
        { "-he", "--het_cutoff", FLOAT, &o.het_cutoff, "allele fraction from which a genotype is 0/1 (default 0.2)", false, false },
        { "-ho", "--hom_cutoff", FLOAT, &o.hom_cutoff, "allele fraction from which a genotype is 1/1 (default 0.8)", false, false },
        { "-is", "--min_size", INT, &o.min_size, "smallest event size written (default 1)", false, false },
        { "-as", "--max_size", INT, &o.max_size, "largest event size written (default: no limit)", false, false },
        { "-b", "--both_strands_supported", BOOL, &o.both_strands, "only events with reads on both strands (default false)", false, false },
        { "-m", "--min_supporting_samples", INT, &o.min_supporting_samples, "samples that must support an event (default 1)", false, false },
        { "-e", "--min_supporting_reads", INT, &o.min_supporting_reads, "reads that must support an event (default 1)", false, false },
        { "-f", "--max_supporting_reads", INT, &o.max_supporting_reads, "most reads an event may have (default: no limit)", false, false },
        { "-sr", "--region_start", INT, &o.region_start, "first position written (default 0)", false, false },
        { "-er", "--region_end", INT, &o.region_end, "last position written (default: no limit)", false, false },
        { "-ir", "--max_internal_repeats", INT, &o.max_internal_repeats,
          "drop indels whose inserted or deleted bases repeat a unit more than this often (default: no limit)", false, false },
        { "-co", "--compact_output_limit", INT, &o.compact_output_limit,
          "write events with a REF or ALT longer than this as 'first base, <SVTYPE>' (default 1000000; 1 or less: never)", false, false },
        { "-il", "--max_internal_repeatlength", INT, &o.max_internal_repeatlength, "longest repeat unit -ir looks for (default: no limit)", false, false },
        { "-pr", "--max_postindel_repeats", INT, &o.max_postindel_repeats,
          "drop indels whose repeat unit recurs after the event more than this often (default: no limit)", false, false },
        { "-pl", "--max_postindel_repeatlength", INT, &o.max_postindel_repeatlength, "longest repeat unit -pr looks for (default: no limit)", false, false },
        { "-sb", "--only_balanced_samples", BOOL, &o.only_balanced_samples,
          "count a sample only if both strands have -ss reads (default false)", false, false },
        { "-ss", "--minimum_strand_support", INT, &o.minimum_strand_support, "reads a strand needs for a sample to count (default 1)", false, false },
        { "-G", "--gatk_compatible", BOOL, &o.gatk_compatible,
          "GATK-compatible output: 0/0 and 0/1 genotypes, equal-length replacements without the base before (default false)", false, false },
        { "-h", "--help", BOOL, &help, "print this help", false, false },
    };
    if (argc == 1) {
        print_help(flags);
        return 0;
    }
    for (int i = 1; i < argc; i++) {
        const std::string arg = argv[i];
        Flag *f = nullptr;
        for (Flag &c : flags)
            if (arg == c.short_name || arg == c.long_name) f = &c;
        if (!f) {
            std::cerr << "pindel_pg2vcf: unknown argument: " << arg << "\n";
            return 1;
        }
        f->set = true;
        if (f->kind == BOOL) {
            bool v = true;
            if (i + 1 < argc && argv[i + 1][0] != '-') {
                const char c = argv[i + 1][0];
                if (std::tolower((unsigned char)c) == 'f' || c == '0') v = false;
                i++;
            }
            *(bool *)f->target = v;
            continue;
        }
        if (i + 1 >= argc) {
            std::cerr << "pindel_pg2vcf: argument of " << arg << " lacking\n";
            return 1;
        }
        const char *val = argv[++i];
        if (val[0] == '-') {
            std::cerr << "pindel_pg2vcf: argument of " << arg << " seems erroneous: " << val << "\n";
            return 1;
        }
        if (f->kind == STR) *(std::string *)f->target = val;
        else if (f->kind == INT) *(int *)f->target = std::atoi(val);
        else *(double *)f->target = std::atof(val);
    }
    if (help) {
        print_help(flags);
        return 0;
    }
    bool ok = true;
    for (const Flag &f : flags)
        if (f.required && !f.set) {
            std::cerr << "pindel_pg2vcf: required parameter " << f.short_name << "/" << f.long_name << " needs to be set\n";
            ok = false;
        }
    const bool p = flags[3].set, P = flags[4].set;
    if (p && P) {
        std::cerr << "pindel_pg2vcf: -p and -P cannot be used together\n";
        ok = false;
    } else if (!p && !P) {
        std::cerr << "pindel_pg2vcf: a pindel input is needed: -p <report> or -P <prefix>\n";
        ok = false;
    }
    if (!ok) {
        std::cerr << "Run pindel_pg2vcf -h for the flags.\n";
        return 1;
    }
    std::string err;
    if (pgh::reports_to_vcf(o, err, &std::cout)) {
        std::cerr << "pindel_pg2vcf: " << err << "\n";
        return 1;
    }
    std::cout << "Wrote " << pgh::vcf_output_path(o) << "\n";
    return 0;
}
