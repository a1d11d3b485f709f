// pg_vcf.hpp -- pindel2vcf: Pindel's _D, _SI, _LI, _INV and _TD reports -> VCF 4.0.
// A restatement of the reference converter's default behaviour and of all of its flags (src/pindel2vcf.cpp,
// version 0.6.3), used by the pindel_pg2vcf command line, pgh_reports_to_vcf and hostlib.reports_to_vcf.
// The bytes of the output follow the reference exactly; how it gets there does not: the reports are parsed once and
// the records bucketed per chromosome in input order, and the FASTA is read once, where the reference re-reads every
// report once per FASTA contig and per window and re-scans the FASTA for every contig (pg_vcf.cpp has the details).
#ifndef PG_VCF_HPP
#define PG_VCF_HPP

#include <ostream>
#include <string>

namespace pgh {

// The converter's flags (createParameters, pindel2vcf.cpp:1982-2047), with the reference's defaults.
struct VcfOptions {
    std::string reference;          // -r  FASTA (required)
    std::string reference_name;     // -R  ##reference= (required)
    std::string reference_date;     // -d  ##fileDate= (required)
    std::string report;             // -p  one report
    std::string prefix;             // -P  <prefix>_D, _SI, _LI, _INV, _TD
    std::string vcf;                // -v  default <-p>.vcf / <-P>.vcf
    std::string chromosome;         // -c  only this chromosome ("" = all, in FASTA order)
    int window_size = 300;          // -w  window in Mbp
    int min_coverage = 10;          // -mc
    double het_cutoff = 0.2;        // -he
    double hom_cutoff = 0.8;        // -ho
    int min_size = 1;               // -is
    int max_size = -1;              // -as
    bool both_strands = false;      // -b
    int min_supporting_samples = 1; // -m
    int min_supporting_reads = 1;   // -e
    int max_supporting_reads = -1;  // -f
    int region_start = 0;           // -sr
    int region_end = -1;            // -er
    int max_internal_repeats = -1;        // -ir
    int max_internal_repeatlength = -1;   // -il
    int max_postindel_repeats = -1;       // -pr
    int max_postindel_repeatlength = -1;  // -pl
    int compact_output_limit = 1000000;   // -co
    bool only_balanced_samples = false;   // -sb
    int minimum_strand_support = 1;       // -ss
    bool gatk_compatible = false;         // -G
};

// Writes opt.vcf (or its default).  Returns 0, or 1 with the reason in err (the output file is then removed).  Progress
// lines go to log when it is given.
int reports_to_vcf(const VcfOptions &opt, std::string &err, std::ostream *log = nullptr);

// The VCF path a run writes to: opt.vcf, else <report>.vcf or <prefix>.vcf (setParameters, 2165-2178).
std::string vcf_output_path(const VcfOptions &opt);

}  // namespace pgh

#endif
