// pg_vcf.cpp -- pindel2vcf restated (pg_vcf.hpp).  Line numbers are those of the reference's src/pindel2vcf.cpp.
//
// What decides the bytes:
//   * Input.  -p is one report, -P the five reports <prefix>_D _SI _LI _INV _TD, read as one stream in that order; a
//     file that does not open is skipped (InputReader, 312-372; main 2331-2341).  A record is a summary line whose
//     second field is D, I, LI, TD or INV (isSVSummarizingLine, 1647).  A last summary line without a newline at the
//     end of the last report that opens is not converted: the reference's eof() is already true after reading it
//     (convertIndelToSVdata 1759-1765 and the loop at 2276-2284).
//   * Fields.  The reference reads a line with operator>> on a stringstream, counting tokens from where it stands
//     (fetchElement, 1600); Tokens below does the same, including what a read past the end yields.
//   * Samples.  VCF columns follow std::set order (makeSampleMap, 2225).  A line is "0.2.4u or later" -- 7 fields per
//     sample, the two reference-coverage integers included -- once one line has more tokens than 31 + 5 * samples
//     (1723); the flag never goes back, and decides the RD header line and GT:ref,alt against 1/.:n sample fields.
//   * Order.  Each chromosome is cut into windows of -w Mbp; each window std::sorts, by (position, SVLEN), the record
//     held back from the previous window followed by its own records in input order, prints every record but the
//     last, and holds that one back (reportSVsInChromosome, 2245-2313).  Records on the same position with the same
//     SVLEN come out in the order std::sort leaves them in, so the keys below are sorted with std::sort on exactly
//     that sequence.
//
// Deliberate differences from the reference, all on input it mishandles:
//   * a record on a chromosome that is not in the FASTA is an error (the reference stops with an error for LI records
//     only, and drops other records silently);
//   * a reference position past the end of its chromosome is an error (the reference reads past its string);
//   * -w 0 or less is an error (the reference never leaves its window loop); windows are counted in 64 bits;
//   * a FASTA header name also ends at '\r' when the sequence is read (the reference's reading pass keeps the '\r',
//     finds no sequence for the name and reads out of bounds), and a name that occurs twice is an error (the
//     reference converts that chromosome twice, with the first sequence);
//   * malformed NT fields, which make the reference throw std::out_of_range and abort, are an error;
//   * a sample with no reads at all under -mc 0 is ./. (the reference divides 0 by 0 and returns no genotype).
#include "pg_vcf.hpp"

#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

namespace pgh {
namespace {

struct VcfError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

bool is_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r'; }

// One line read token by token with operator>>, as fetchElement (1600) and countElements (1610) do.
struct Tokens {
    std::vector<std::string> tok;
    size_t next = 0;
    bool fail = false;

    explicit Tokens(const std::string &line)
    {
        size_t i = 0;
        const size_t n = line.size();
        while (i < n) {
            while (i < n && is_space(line[i])) i++;
            size_t j = i;
            while (j < n && !is_space(line[j])) j++;
            if (j > i) tok.emplace_back(line, i, j - i);
            i = j;
        }
    }
    // fetchElement(n): the n-th token from here.  Past the end the stream fails, and the value is the last token this
    // call did read ("" if none): a failed operator>> leaves its string alone.
    std::string fetch(int n)
    {
        std::string e;
        for (int k = 0; k < n && !fail; k++) {
            if (next < tok.size()) e = tok[next++];
            else fail = true;
        }
        return e;
    }
    // countElements counts the read that fails too
    int count_elements() const { return (int)tok.size() + 1; }
};

int to_int(const std::string &s) { return std::atoi(s.c_str()); }

// isSVSummarizingLine (1647) with isPindelSVIdentifier (1635)
bool is_summary_line(const std::string &line)
{
    Tokens t(line);
    if (t.count_elements() < 2) return false;
    const std::string item = t.fetch(2);
    return item == "D" || item == "I" || item == "LI" || item == "TD" || item == "INV";
}

struct Genotype {
    int plus = 0, minus = 0, ref = 0;   // d_readDepthPlus, d_readDepthMinus, d_totalRefSupport
    int reads() const { return plus + minus; }
};

// SVData (1000-1166): what convertIndelToSVdata fills in.  The sequence-dependent parts (REF, ALT, HOMSEQ) are
// computed when the record's chromosome is read.
struct Record {
    std::string chrom, type;   // DEL RPL INS DUP:TANDEM INV
    int pos = 0, end = 0, svlen = 0, homlen = 0;
    int hom_from = 0, hom_to = 0;   // HOMSEQ = reference [hom_from, hom_to)
    int replace = 0, replace2 = -1;
    std::string nt, nt2, homseq;
    std::vector<Genotype> fmt;

    bool long_insertion() const { return type == "INS" && svlen == 0; }
    // altSameLengthAsRef (1138)
    bool same_length() const { return (type == "RPL" && svlen == replace) || (type == "INV" && replace == 0 && replace2 == 0); }
};

struct Converter {
    const VcfOptions &o;
    std::ostream *log;
    bool v024 = false;                     // pindel024uOrLater
    std::set<std::string> samples, chroms; // getSampleNamesAndChromosomeNames (1666)
    std::map<std::string, int> sample_id;
    std::vector<Record> recs;
    const std::string *seq = nullptr;      // the chromosome being written, with a leading N (1-based)

    Converter(const VcfOptions &opt, std::ostream *l) : o(opt), log(l) {}

    void note(const std::string &s)
    {
        if (log) *log << s << "\n";
    }

    // getPosition (1008): -G moves equal-length replacements one base on, and that also moves them in the sort
    int position(const Record &r) const { return o.gatk_compatible && r.same_length() ? r.pos + 1 : r.pos; }

    char at(const Record &r, long p) const
    {
        if (p < 0 || p >= (long)seq->size())
            throw VcfError("the record at " + r.chrom + ":" + std::to_string(r.pos) + " reaches position " + std::to_string(p) +
                           ", past the end of the chromosome (" + std::to_string(seq->size() - 1) + " bp)");
        return (*seq)[p];
    }

    // ---- reading ------------------------------------------------------------------------------------------------

    // the scan before the conversion (getSampleNamesAndChromosomeNames, 1666-1740)
    void scan(const std::string &line)
    {
        Tokens ls(line);
        const int elements = ls.count_elements();
        const std::string type = ls.fetch(2);
        if (type == "LI") {
            chroms.insert(ls.fetch(2));
            samples.insert(ls.fetch(7));
            std::string s = ls.fetch(5);
            while (!ls.fail) {
                samples.insert(s);
                s = ls.fetch(5);
            }
            return;
        }
        chroms.insert(ls.fetch(6));
        const int n_samples = to_int(ls.fetch(20));
        const std::string first = ls.fetch(4);
        if (!first.empty()) samples.insert(first);
        if (elements > 32 + 5 * n_samples) v024 = true;
        const int per_sample = v024 ? 7 : 5;
        std::string s = ls.fetch(per_sample);
        while (!ls.fail) {
            if (!s.empty()) samples.insert(s);
            s = ls.fetch(per_sample);
        }
    }

    void add_genotype(Record &r, const std::string &name, int plus, int minus, int ref)
    {
        auto it = sample_id.find(name);
        if (it == sample_id.end()) {
            note("Error: could not find sample " + name);
            return;
        }
        r.fmt[it->second] = Genotype{ plus, minus, ref };
    }

    // convertIndelToSVdata (1755-1946)
    Record parse(const std::string &line)
    {
        Record r;
        r.fmt.assign(std::max<size_t>(1, samples.size()), Genotype{});
        Tokens ls(line);
        const std::string type = ls.fetch(2);
        if (type == "LI") {   // 1770-1822: "<i> LI ChrID <chr> <pos> + <n> <end> - <n> <sample> + <n> - <n> ..."
            r.type = "INS";
            r.svlen = 0;
            r.chrom = ls.fetch(2);
            r.pos = to_int(ls.fetch(1));
            ls.fetch(2);
            r.end = to_int(ls.fetch(1));
            ls.fetch(2);
            std::string name = ls.fetch(1);
            int plus = to_int(ls.fetch(2)), minus = to_int(ls.fetch(2));
            while (!ls.fail) {
                add_genotype(r, name, plus, minus, 0);
                name = ls.fetch(1);
                plus = to_int(ls.fetch(2));
                minus = to_int(ls.fetch(2));
            }
            return r;
        }
        r.svlen = to_int(ls.fetch(1));
        const std::string n_nt_field = ls.fetch(2);   // "<n>" or, for inversions, "<n>:<m>"
        const int n_nt = to_int(n_nt_field);
        bool simple_inversion = false;                // the "INV 2 NT 2 "TG"" form (1847-1849)
        int n_nt_inv = -1;
        const bool inv = type == "INV";
        if (inv) {
            const size_t sep = n_nt_field.find(':');
            if (sep == std::string::npos) simple_inversion = true;
            else n_nt_inv = to_int(n_nt_field.substr(sep + 1));
        }
        std::string nt = ls.fetch(1);   // "\"ACG\"" or "\"\":\"GCT\""
        if (inv) {
            const size_t sep = nt.find(':');
            if (sep == std::string::npos) {
                simple_inversion = true;
            } else {
                if (sep + 2 > nt.size()) throw VcfError("malformed NT field in: " + line);
                r.nt2 = nt.substr(sep + 2, n_nt_inv < 0 ? std::string::npos : (size_t)n_nt_inv);
                nt = nt.substr(0, sep);
            }
        }
        if (!nt.empty()) nt.erase(0, 1);
        if (n_nt < 0 || (size_t)n_nt > nt.size()) throw VcfError("malformed NT field in: " + line);
        nt.erase(n_nt);
        if (!simple_inversion) r.nt = nt;
        r.chrom = ls.fetch(2);
        r.pos = to_int(ls.fetch(2));                 // BP start
        const int left_end = to_int(ls.fetch(1));    // BP end
        ls.fetch(2);                                 // BP_range start
        const int right_end = to_int(ls.fetch(1));   // BP_range end
        r.end = left_end;
        r.homlen = right_end - left_end;
        r.hom_from = left_end;
        r.hom_to = right_end;
        if (type == "D") {
            r.type = n_nt == 0 ? "DEL" : "RPL";
            r.replace = n_nt;
        } else if (type == "I") {
            r.type = "INS";
        } else if (type == "TD") {
            r.type = "DUP:TANDEM";
            r.replace = n_nt;
        } else {
            r.type = "INV";
            r.replace = simple_inversion ? 0 : n_nt;
            r.replace2 = simple_inversion ? 0 : n_nt_inv;
        }
        // per sample: name [ref-start ref-end] +total +unique -total -unique
        std::string name = ls.fetch(18);
        int ref_a = 0, ref_b = 0;
        if (v024) {
            ref_a = to_int(ls.fetch(1));
            ref_b = to_int(ls.fetch(1));
        }
        int plus = to_int(ls.fetch(1)), minus = to_int(ls.fetch(2));
        while (!ls.fail) {
            add_genotype(r, name, plus, minus, std::max(ref_a, ref_b));
            name = ls.fetch(2);
            if (v024) {
                ref_a = to_int(ls.fetch(1));
                ref_b = to_int(ls.fetch(1));
            }
            plus = to_int(ls.fetch(1));
            minus = to_int(ls.fetch(2));
        }
        return r;
    }

    // ---- alleles ------------------------------------------------------------------------------------------------

    // getReference (1206): for indels the base before the event is included
    std::string ref_allele(const Record &r) const
    {
        if (r.long_insertion()) return std::string(1, at(r, r.pos));
        std::string s;
        const int start = o.gatk_compatible && r.same_length() ? r.pos + 1 : r.pos;
        for (int p = start; p < r.end; p++) s += at(r, p);
        return s;
    }

    static std::string reverse_complement(const std::string &s)
    {
        std::string c;
        c.reserve(s.size());
        for (size_t i = s.size(); i-- > 0;) {
            switch (s[i]) {
            case 'A': c += 'T'; break;
            case 'C': c += 'G'; break;
            case 'G': c += 'C'; break;
            case 'T': c += 'A'; break;
            default: c += 'N';
            }
        }
        return c;
    }

    // getAlternative (1168)
    std::string alt_allele(const Record &r) const
    {
        if (r.long_insertion()) return "<INS>";
        std::string alt;
        const bool gatk_same = o.gatk_compatible && r.same_length();
        if (r.type == "INS" || r.type == "DEL" || r.type == "RPL") {
            if (!gatk_same) alt += at(r, r.pos);
            alt += r.nt;
        } else if (r.type == "DUP:TANDEM") {
            const std::string ref = ref_allele(r);
            alt = ref + r.nt + ref.substr(1);
        } else if (r.type == "INV") {
            const std::string ref = ref_allele(r);
            if (gatk_same) {
                alt = reverse_complement(ref);
            } else {
                alt += at(r, r.pos);
                alt += r.nt;
                alt += reverse_complement(ref.substr(1));
                alt += r.nt2;
            }
        }
        return alt;
    }

    // ---- filters (throughFilter, 2181-2222) ---------------------------------------------------------------------

    // testHypothesis (1357): how often hyp repeats to make up seq, 0 if it does not
    static int test_hypothesis(const std::string &hyp, const std::string &seq)
    {
        for (size_t i = 0; i < seq.size(); i++)
            if (hyp[i % hyp.size()] != seq[i]) return 0;
        return (int)(seq.size() / hyp.size());
    }

    // countRepeats (1373): the repeat count of the unit (at most max_len long, any length when negative) that explains
    // most of seq
    static int count_repeats(const std::string &seq, int max_len, int &best_size)
    {
        int longest = std::min(max_len, (int)(seq.size() / 2));
        if (max_len < 0) longest = (int)(seq.size() / 2);
        std::string hyp;
        size_t best_len = 0, best_num = 0;
        for (int len = 1; len <= longest; len++) {
            hyp += seq[len - 1];
            const int reps = test_hypothesis(hyp, seq);
            if (reps > 0 && (size_t)reps * hyp.size() > best_len * best_num) {
                best_len = hyp.size();
                best_num = (size_t)reps;
            }
        }
        best_size = (int)best_len;
        return (int)best_num;
    }

    // getSVSequence (1397): the inserted or deleted bases; for a replacement the new sequence
    std::string sv_sequence(const Record &r) const
    {
        const std::string ref = ref_allele(r), alt = alt_allele(r);
        const size_t max_pos = std::min(ref.size(), alt.size());
        size_t p = 0;
        while (p < max_pos && ref[p] == alt[p]) p++;
        if (p == max_pos) return max_pos == ref.size() ? alt.substr(p) : ref.substr(p);
        return alt.substr(p);
    }

    // withinAllowedRepeatsInternal (1440)
    bool internal_repeats_ok(const Record &r) const
    {
        int unit = 0;
        return count_repeats(sv_sequence(r), o.max_internal_repeatlength, unit) <= o.max_internal_repeats;
    }

    // withinAllowedRepeatsPostIndel (1418)
    bool postindel_repeats_ok(const Record &r) const
    {
        const std::string s = sv_sequence(r);
        int unit = 0;
        const int count = count_repeats(s, o.max_postindel_repeatlength, unit);
        if (unit > 0) return test_hypothesis(s.substr(0, unit), s + r.homseq) - count <= o.max_postindel_repeats;
        int best = 0;
        const int extended = count_repeats(s + r.homseq, o.max_postindel_repeatlength, best);
        // the reference divides by best == 0 here; the quotient converts to INT_MIN, which passes
        if (best == 0) return true;
        const int post = best * extended - (int)s.size();
        return (int)((double)post / best) <= o.max_postindel_repeats;
    }

    bool passes(const Record &r) const
    {
        if (o.min_size > 1 && std::abs(r.svlen) < o.min_size) return false;
        if (o.max_size > 0 && std::abs(r.svlen) > o.max_size) return false;
        int reads = 0, n_samples = 0;
        bool any_plus = false, any_minus = false;
        for (const Genotype &g : r.fmt) {
            reads += g.reads();
            any_plus |= g.plus > 0;
            any_minus |= g.minus > 0;
            // getNumSupportSamples (1310)
            if (o.only_balanced_samples ? (g.plus >= o.minimum_strand_support && g.minus >= o.minimum_strand_support)
                                        : (g.plus >= o.minimum_strand_support || g.minus >= o.minimum_strand_support))
                n_samples++;
        }
        if (o.both_strands && !(any_plus && any_minus)) return false;
        if (o.min_supporting_samples >= 1 && n_samples < o.min_supporting_samples) return false;
        if (o.min_supporting_reads >= 1 && reads < o.min_supporting_reads) return false;
        if (o.max_supporting_reads >= 1 && reads > o.max_supporting_reads) return false;
        if (o.region_start > 0 && position(r) < o.region_start) return false;
        if (o.region_end > 0 && position(r) > o.region_end) return false;
        if (o.max_internal_repeats >= 0 && !internal_repeats_ok(r)) return false;
        if (o.max_postindel_repeats >= 0 && !postindel_repeats_ok(r)) return false;
        return true;
    }

    // ---- writing ------------------------------------------------------------------------------------------------

    // deriveGenotype (908): allele fraction in float against the -he / -ho cutoffs, below -mc reads 0/0
    std::string genotype(const Genotype &g) const
    {
        const int event = g.reads(), ref = g.ref;
        if (event + ref < o.min_coverage) return "0/0";
        const float af = (float)event / (event + ref);
        if (af < o.het_cutoff) return "0/0";
        if (af >= o.het_cutoff && af < o.hom_cutoff) return "0/1";
        if (af >= o.hom_cutoff) return "1/1";
        return "./.";   // 0 / 0 reads (see the head of this file)
    }

    // createHeader (737-785)
    void header(std::ostream &out) const
    {
        out << "##fileformat=VCFv4.0\n"
            << "##fileDate=" << o.reference_date << "\n"
            << "##source=pindel\n"
            << "##reference=" << o.reference_name << "\n"
            << "##INFO=<ID=END,Number=1,Type=Integer,Description=\"End position of the variant described in this record\">\n"
            << "##INFO=<ID=HOMLEN,Number=1,Type=Integer,Description=\"Length of base pair identical micro-homology at event breakpoints\">\n"
            << "##INFO=<ID=PF,Number=1,Type=Integer,Description=\"The number of samples carry the variant\">\n"
            << "##INFO=<ID=HOMSEQ,Number=.,Type=String,Description=\"Sequence of base pair identical micro-homology at event breakpoints\">\n"
            << "##INFO=<ID=SVLEN,Number=1,Type=Integer,Description=\"Difference in length between REF and ALT alleles\">\n"
            << "##INFO=<ID=SVTYPE,Number=1,Type=String,Description=\"Type of structural variant\">\n"
            << "##INFO=<ID=NTLEN,Number=.,Type=Integer,Description=\"Number of bases inserted in place of deleted code\">\n"
            << "##FORMAT=<ID=PL,Number=3,Type=Integer,Description=\"Normalized, Phred-scaled likelihoods for genotypes as defined in the VCF specification\">\n"
            << "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n";
        if (v024) out << "##FORMAT=<ID=RD,Number=1,Type=Integer,Description=\"Reference depth, how many reads support the reference\">\n";
        out << "##FORMAT=<ID=AD,Number=2,Type=Integer,Description=\"Allele depth, how many reads support this allele\">\n";
        out << "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO";
        if (!samples.empty()) {
            out << "\tFORMAT";
            for (const std::string &s : samples) out << "\t" << s;
        }
        out << "\n";
    }

    // operator<<(SVData) (1529-1597), with getOutputFormattedReference / -Alternative (1237-1270) for -co
    void write(std::ostream &out, const Record &r) const
    {
        const std::string ref = ref_allele(r), alt = alt_allele(r);
        std::string ref_out = ref, alt_out = alt;
        if (alt != "<INS>" && o.compact_output_limit > 1 &&
            (ref.size() > (size_t)o.compact_output_limit || alt.size() > (size_t)o.compact_output_limit)) {
            ref_out.erase(1);
            alt_out = "<" + r.type + ">";
        }
        std::string line = r.chrom + "\t" + std::to_string(position(r)) + "\t.\t" + ref_out + "\t" + alt_out + "\t.\tPASS\t";
        line += "END=" + std::to_string((int)(r.pos + ref.size() - 1)) + ";HOMLEN=" + std::to_string(r.homlen) + ";";
        if (r.homlen != 0) line += "HOMSEQ=" + r.homseq + ";";
        line += "SVLEN=";
        if ((r.type == "RPL" || r.type == "DEL") && r.svlen > 0) line += "-";
        line += std::to_string(r.svlen) + ";SVTYPE=" + r.type;
        if (r.type == "RPL" || r.type == "DUP:TANDEM" || r.type == "INV") line += ";NTLEN=" + std::to_string(r.replace);
        if (r.type == "INV") line += "," + std::to_string(r.replace2);
        line += "\tGT:AD";
        const bool with_ref = v024 && alt != "<INS>";
        for (const Genotype &g : r.fmt) {
            line += "\t";
            if (with_ref) {   // getGTRDAD (984)
                line += genotype(g) + ":" + std::to_string(g.ref) + "," + std::to_string(g.reads());
            } else {          // getGTAD (991) with getGTold (960)
                const bool none = g.plus == 0 && g.minus == 0;
                line += o.gatk_compatible ? (none ? "0/0" : "0/1") : (none ? "." : "1/.");
                line += ":" + std::to_string(g.reads());
            }
        }
        line += "\n";
        out << line;
    }

    // reportSVsInChromosome (2245-2313) for one chromosome; idx are its records in input order
    void write_chromosome(std::ostream &out, const std::string &sequence, const std::vector<int> &idx)
    {
        seq = &sequence;
        for (int i : idx) {   // HOMSEQ, read when the reference parses the record (1885-1889)
            Record &r = recs[i];
            r.homseq.clear();
            for (int p = r.hom_from; p < r.hom_to; p++) r.homseq += at(r, p);
        }
        const long long size = (long long)sequence.size();
        const long long w = (long long)o.window_size * 1000000;
        long long n_windows = 0;
        for (long long end = w;; end += w) {   // do { ... } while (regionEnd < size)
            n_windows++;
            if (end >= size) break;
        }
        std::vector<std::vector<int>> in_window((size_t)n_windows);
        for (int i : idx) {
            const long long p = position(recs[i]);
            if (p >= 0 && p / w < n_windows) in_window[(size_t)(p / w)].push_back(i);
        }
        struct Key {
            int pos, svlen, idx;
        };
        // SVData::operator< (1342): chromosome (the same here), then position, then SVLEN
        auto less = [](const Key &a, const Key &b) { return a.pos != b.pos ? a.pos < b.pos : a.svlen < b.svlen; };
        bool held = false;
        int held_idx = -1;
        for (const std::vector<int> &win : in_window) {
            std::vector<Key> svs;
            if (held) svs.push_back(Key{ position(recs[held_idx]), recs[held_idx].svlen, held_idx });
            for (int i : win) svs.push_back(Key{ position(recs[i]), recs[i].svlen, i });
            std::sort(svs.begin(), svs.end(), less);
            for (size_t k = 0; k + 1 < svs.size(); k++)
                if (passes(recs[svs[k].idx])) write(out, recs[svs[k].idx]);
            if (!svs.empty()) {
                held = true;
                held_idx = svs.back().idx;
            }
        }
        if (held && passes(recs[held_idx])) write(out, recs[held_idx]);
        seq = nullptr;
    }
};

// A FASTA header's name: from the second character, at least one character, up to a space, tab, '\n' or '\r'
// (readReference, 1963-1967)
std::string fasta_name(const std::string &header)
{
    std::string name;
    size_t k = 1;
    do {
        if (k < header.size()) name += header[k];
        k++;
    } while (k < header.size() && header[k] != ' ' && header[k] != '\t' && header[k] != '\n' && header[k] != '\r');
    return name;
}

// readReference (1949-1978): the chromosome names in file order.  The first line is a header whatever it holds;
// every later line starting with '>' is one.
bool fasta_names(const std::string &path, std::vector<std::string> &names, std::string &err)
{
    std::ifstream f(path.c_str());
    if (!f) {
        err = "Cannot open reference file " + path;
        return false;
    }
    std::string line;
    bool first = true;
    while (std::getline(f, line)) {
        if (first || (!line.empty() && line[0] == '>')) names.push_back(fasta_name(line));
        first = false;
    }
    if (first) {
        err = "the reference file " + path + " is empty";
        return false;
    }
    return true;
}

}  // namespace

std::string vcf_output_path(const VcfOptions &opt)
{
    if (!opt.vcf.empty()) return opt.vcf;
    return (opt.report.empty() ? opt.prefix : opt.report) + ".vcf";
}

int reports_to_vcf(const VcfOptions &opt, std::string &err, std::ostream *log)
{
    err.clear();
    if (opt.reference.empty()) err += "Required parameter -r/--reference needs to be set. ";
    if (opt.reference_name.empty()) err += "Required parameter -R/--reference_name needs to be set. ";
    if (opt.reference_date.empty()) err += "Required parameter -d/--reference_date needs to be set. ";
    if (!opt.report.empty() && !opt.prefix.empty()) err += "-p and -P cannot be used together. ";
    if (opt.report.empty() && opt.prefix.empty()) err += "A pindel input is needed: -p <report> or -P <prefix>. ";
    if (opt.window_size <= 0) err += "-w must be at least 1 (Mbp). ";
    if (!err.empty()) {
        err.pop_back();
        return 1;
    }
    Converter cv(opt, log);
    const std::string out_path = vcf_output_path(opt);
    bool output_open = false;
    try {
        // the input: the reports that open, as one stream
        std::vector<std::string> files;
        if (!opt.report.empty()) files.push_back(opt.report);
        else
            for (const char *suf : { "_D", "_SI", "_LI", "_INV", "_TD" }) files.push_back(opt.prefix + suf);
        struct Line {
            std::string text;
            int file;
            bool unterminated;
        };
        std::vector<Line> summary;
        int last_open = -1;
        for (size_t k = 0; k < files.size(); k++) {
            std::ifstream f(files[k].c_str());
            if (!f) continue;
            last_open = (int)k;
            std::string line;
            while (std::getline(f, line))
                if (is_summary_line(line)) summary.push_back(Line{ line, (int)k, f.eof() });
        }
        if (last_open < 0) {
            err = "The pindel file (-p) does not exist.";
            return 1;
        }
        if (!summary.empty() && summary.back().unterminated && summary.back().file == last_open) summary.pop_back();

        for (const Line &l : summary) cv.scan(l.text);
        int n = 0;
        for (const std::string &s : cv.samples) cv.sample_id[s] = n++;
        cv.recs.reserve(summary.size());
        for (const Line &l : summary) cv.recs.push_back(cv.parse(l.text));

        std::vector<std::string> names;
        if (!fasta_names(opt.reference, names, err)) return 1;
        std::map<std::string, std::vector<int>> by_chrom;   // record indices per chromosome, in input order
        for (size_t i = 0; i < cv.recs.size(); i++) by_chrom[cv.recs[i].chrom].push_back((int)i);
        {
            std::set<std::string> seen;
            for (const std::string &nm : names)
                if (!seen.insert(nm).second) {
                    err = "the reference names chromosome \"" + nm + "\" twice";
                    return 1;
                }
            for (const auto &kv : by_chrom)
                if (!seen.count(kv.first)) {
                    err = "Reference chromosome \"" + kv.first + "\" not found!";
                    return 1;
                }
        }
        cv.note("Samples: " + std::to_string(cv.samples.size()) + "; chromosomes with events: " + std::to_string(cv.chroms.size()) +
                "; records: " + std::to_string(cv.recs.size()));

        std::ofstream out(out_path.c_str(), std::ios::binary | std::ios::trunc);
        if (!out) {
            err = "cannot write " + out_path;
            return 1;
        }
        output_open = true;
        cv.header(out);

        // one pass over the FASTA: each chromosome with records, in file order (or -c only), is read and written
        std::ifstream fa(opt.reference.c_str());
        std::string line, name, sequence;
        bool in_target = false, first = true;
        const std::vector<int> *target_idx = nullptr;
        auto flush = [&]() {
            if (in_target) cv.write_chromosome(out, sequence, *target_idx);
            sequence.clear();
        };
        while (std::getline(fa, line)) {
            if (first || (!line.empty() && line[0] == '>')) {
                flush();
                first = false;
                name = fasta_name(line);
                auto it = by_chrom.find(name);
                in_target = (opt.chromosome.empty() || opt.chromosome == name) && it != by_chrom.end();
                target_idx = in_target ? &it->second : nullptr;
                if (in_target) sequence = "N";   // 1-based positions
                continue;
            }
            if (!in_target) continue;
            // Chromosome::readFromFile (650-693): letters only, upper-cased; anything but ACGTN becomes N
            for (char ch : line) {
                const char c = (char)std::toupper((unsigned char)ch);
                if (c >= 'A' && c <= 'Z') sequence += (c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N') ? c : 'N';
            }
        }
        flush();
        out.close();
        if (!out) {
            err = "writing " + out_path + " failed";
            std::remove(out_path.c_str());
            return 1;
        }
    } catch (const std::exception &e) {
        err = e.what();
        if (output_open) std::remove(out_path.c_str());
        return 1;
    }
    return 0;
}

}  // namespace pgh
