// pg_host_int.cpp -- interchromosomal events (-I, --report_interchromosomal_events; default off):
//   the copy of the reads whose far end lies on another chromosome   src/pindel.cpp:1905-1917 (before SearchSVs)
//   SortAndReportInterChromosomalEvents -> <prefix>_INT              src/reporter.cpp:2395-2665 (once per window, after the SV reporters)
//   MergeInterChr -> <prefix>_INT_final                              src/pindel.cpp:1514-1579 (once, at the end of the run)
// Restated, no code shared.  The search that finds those far ends is the ordinary one: a window cluster may name any
// chromosome (SearchFarEnd, src/pindel.cpp:1001-1020).  What the reference computes here and only prints on stdout
// (Left, Right, BP) is left out.
#include <fstream>
#include <iterator>
#include <map>
#include <set>
#include <sstream>

#include "pg_host_priv.hpp"

namespace pgh {

using namespace detail;

void Caller::collect_interchr(const std::vector<SplitRead> &reads)
{
    interchr_.clear();
    for (const SplitRead &r : reads)
        if (!r.UP_Far.empty() && r.FragName != r.FarFragName) interchr_.push_back(r);   // (no -c / -j filter applies)
}

namespace {

std::string strand_text(char d) { return d == '+' ? "+" : d == '-' ? "-" : ""; }        // SameStrand
std::string other_strand_text(char d) { return d == '+' ? "-" : d == '-' ? "+" : ""; }  // OtherStrand

// The call of one read, or "" when it supports none.  `close_ascending`: the close points are scanned from the first
// and the far points from the last; otherwise the other way round.  The first pair whose lengths add up to the read
// length gives the template call; else the last point of either side, if long enough, with what lies between as the
// non-template sequence -- always UnmatchedSeq from the far length on, whatever the orientation of the read.
std::string interchr_call(const SplitRead &r, bool close_ascending, unsigned spacer)
{
    const int nc = (int)r.UP_Close.size(), nf = (int)r.UP_Far.size(), len = r.getReadLength();
    int ci = -1, fi = -1;
    for (int a = 0; a < nc && ci < 0; a++) {
        const int c = close_ascending ? a : nc - 1 - a;
        for (int b = 0; b < nf; b++) {
            const int f = close_ascending ? nf - 1 - b : b;
            if (r.UP_Close[c].LengthStr + r.UP_Far[f].LengthStr == len) {
                ci = c;
                fi = f;
                break;
            }
        }
    }
    std::string inserted = "\"\"";
    if (ci < 0) {
        const UniquePoint &c = r.UP_Close.back(), &f = r.UP_Far.back();
        const unsigned effective = (unsigned)(c.LengthStr + f.LengthStr);
        if (!(effective >= 30 && c.LengthStr >= 10 && f.LengthStr >= 10)) return std::string();
        inserted = "\"" + sub(r.UnmatchedSeq, f.LengthStr, (long)(unsigned)(len - effective)) + "\"";
        ci = nc - 1;
        fi = nf - 1;
    }
    std::ostringstream o;
    o << "Anchor " << strand_text(r.MatchedD) << " " << r.FragName << " " << (int)(r.UP_Close[ci].AbsLoc - spacer) << " "
      << other_strand_text(r.MatchedD) << " " << r.FarFragName << " " << (int)(r.UP_Far[fi].AbsLoc - spacer) << " "
      << strand_text(r.MatchedFarD) << " " << inserted;
    return o.str();
}

}  // namespace

// The reference loops over every pair (first < second) of the chromosome names its reads touch, and inside over every
// read -- but it enters a read's name into ReadNames when the read is VISITED, matching or not (reporter.cpp:2464-2471).
// Every read is visited during the first pair, so later pairs find every name taken: only reads between the two
// smallest names of the window are ever reported.  That is kept, as one pass with those two names.  A second read of
// the same name is skipped.  Used is false for every copy (they are taken before the classifiers run).
//
// --repair int-pairs: every pair is looked at, in the reference's order, and a name is entered only when
// its read matches the pair in hand; the calls are counted and written pair by pair.  The lines of the first pair come
// first; they are the unrepaired lines unless one of its reads shares its name with an earlier read of another pair
// (taken without the repair, free with it: the first pair's own count can then be higher).
void Caller::report_interchr()
{
    if (interchr_.empty()) return;
    std::set<std::string> names;
    for (const SplitRead &r : interchr_) {
        names.insert(r.FragName);
        names.insert(r.FarFragName);
    }
    std::vector<std::pair<std::string, std::string>> pairs;
    for (auto first = names.begin(); first != names.end(); ++first)
        for (auto second = std::next(first); second != names.end(); ++second) pairs.emplace_back(*first, *second);
    if (!S.repair(REPAIR_INT_PAIRS)) pairs.resize(1);       // the first pair takes every name
    std::set<std::string> seen;
    std::ofstream &out = open_append(int_out_, int_buf_, "_INT");
    for (const auto &pair : pairs) {
        std::map<std::string, int> calls;                   // CallAndSupport: call string -> reads, in string order
        for (const SplitRead &r : interchr_) {
            const bool ab = r.FragName == pair.first && r.FarFragName == pair.second;
            const bool ba = r.FragName == pair.second && r.FarFragName == pair.first;
            if (S.repair(REPAIR_INT_PAIRS) && !ab && !ba) continue;
            if (!seen.insert(r.Name).second) continue;
            std::string call;
            if (ab) call = interchr_call(r, r.MatchedD == '+', S.spacer);
            else if (ba) call = interchr_call(r, r.MatchedFarD == '-', S.spacer);   // (sic: the far strand)
            if (!call.empty()) calls[call]++;
        }
        for (const auto &kv : calls)
            if (kv.second >= 2) out << kv.first << "\tsupport: " << kv.second << '\n';
    }
    out.flush();
    interchr_.clear();
}

void write_int_final(const std::string &int_path, const std::string &final_path)
{
    struct Call {
        char AnchorD, FirstD, SecondD;
        std::string FirstChrName, SecondChrName, InsertedSequence;
        unsigned FirstPos, SecondPos, NumSupport;
    };
    const unsigned cutoff = 2;
    std::vector<Call> all;
    {
        std::ifstream in(int_path.c_str());
        Call one;
        std::string word;
        while (in >> word >> one.AnchorD >> one.FirstChrName >> one.FirstPos >> one.FirstD >> one.SecondChrName >> one.SecondPos >>
               one.SecondD >> one.InsertedSequence >> word >> one.NumSupport)
            all.push_back(one);
    }
    std::ofstream out(final_path.c_str(), std::ios::trunc);
    auto infor = [&](const Call &c) {
        out << c.AnchorD << "\t" << c.FirstChrName << "\t" << c.FirstPos << "\t" << c.FirstD << "\t" << c.SecondChrName << "\t" << c.SecondPos
            << "\t" << c.SecondD << "\t" << c.InsertedSequence << "\t" << c.NumSupport;
    };
    auto near = [](unsigned a, unsigned b) { return std::abs((int)(a - b)) < 10; };     // abs() of an unsigned difference, as int
    if (all.size() == 1 && all[0].NumSupport >= cutoff * 2) {                               // (and once more below, with the labels)
        const Call &c = all[0];
        out << c.FirstChrName << "\t" << c.FirstPos << "\t" << c.SecondChrName << "\t" << c.SecondPos << "\t" << c.InsertedSequence << "\t"
            << c.NumSupport << "\t";
        infor(c);
        out << '\n';
    }
    for (size_t a = 0; a < all.size(); a++) {
        bool reported = false;
        for (size_t b = a + 1; b < all.size(); b++) {       // an earlier partner is never looked at again
            const Call &x = all[a], &y = all[b];
            if (x.FirstChrName != y.FirstChrName || x.SecondChrName != y.SecondChrName) continue;
            if (!(near(x.FirstPos, y.FirstPos) && near(x.SecondPos, y.SecondPos) && x.NumSupport + y.NumSupport >= cutoff)) continue;
            out << "chr\t" << x.FirstChrName << "\tpos\t" << (unsigned)((x.FirstPos + y.FirstPos) / 2) << "\tchr\t" << x.SecondChrName << "\tpos\t"
                << (unsigned)((x.SecondPos + y.SecondPos) / 2) << "\tseq\t" << x.InsertedSequence << "\tsupport\t" << x.NumSupport + y.NumSupport
                << "\tINFOR\t";
            infor(x);
            out << "\t";
            infor(y);
            out << '\n';
            reported = true;
            break;
        }
        if (!reported && all[a].NumSupport >= cutoff * 2) {
            const Call &x = all[a];
            out << "chr\t" << x.FirstChrName << "\tpos\t" << x.FirstPos << "\tchr\t" << x.SecondChrName << "\tpos\t" << x.SecondPos << "\tseq\t"
                << x.InsertedSequence << "\tsupport\t" << x.NumSupport << "\tINFOR\t";
            infor(x);
            out << '\n';
        }
    }
}

}  // namespace pgh
