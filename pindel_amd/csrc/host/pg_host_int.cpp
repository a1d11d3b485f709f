// pg_host_int.cpp -- interchromosomal events (-I, --report_interchromosomal_events; default off):
//   the copy of the reads whose far end lies on another chromosome   src/pindel.cpp:1905-1917 (before SearchSVs)
//   SortAndReportInterChromosomalEvents -> <prefix>_INT              src/reporter.cpp:2395-2665 (once per window, after the SV reporters)
//   MergeInterChr -> <prefix>_INT_final                              src/pindel.cpp:1514-1579 (once, at the end of the run)
// Restated, no code shared.  The _INT reporter comes in two parts: int_tables_from_reads -- the call of every
// junction read as tables with their member reads, the host statement of pg_int.hip -- and report_interchr_tables, the one consumer
// of such tables, wherever they were built.  The search that finds those far ends is the ordinary one: a window cluster may name any
// chromosome (SearchFarEnd, src/pindel.cpp:1001-1020).  What the reference computes here and only prints on stdout
// (Left, Right, BP) is left out.
#include <algorithm>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <set>
#include <sstream>
#include <tuple>

#include "pg_host_priv.hpp"

namespace pgh {

using namespace detail;

void Caller::collect_interchr(const std::vector<SplitRead> &reads)
{
    interchr_.clear();
    for (const SplitRead &r : reads)
        if (!r.UP_Far.empty() && r.FragName != r.FarFragName) interchr_.push_back(r);   // (no -c / -j filter applies)
}

std::vector<int32_t> int_chr_ranks(const std::vector<std::string> &names)
{
    const std::set<std::string> order(names.begin(), names.end());
    std::vector<int32_t> rank(names.size());
    for (size_t k = 0; k < names.size(); k++) rank[k] = (int32_t)std::distance(order.begin(), order.find(names[k]));
    return rank;
}

namespace {

// The call of one junction read as the key fields of a pg_int_call, or false when it supports none.  `close_ascending`: the close
// points are scanned from the first and the far points from the last; otherwise the other way round.  The first pair whose lengths
// add up to the read length gives the template call; else the last point of either side, if long enough, with what lies between
// as the non-template sequence -- always UnmatchedSeq from the far length on, whatever the orientation of the read.
bool int_read_call(const IntReadIn &r, bool close_ascending, pg_int_call &call)
{
    const int nc = (int)r.n_close, nf = (int)r.n_far, len = r.read_length;
    int ci = -1, fi = -1;
    for (int a = 0; a < nc && ci < 0; a++) {
        const int c = close_ascending ? a : nc - 1 - a;
        for (int b = 0; b < nf; b++) {
            const int f = close_ascending ? nf - 1 - b : b;
            if (r.close[c].LengthStr + r.far[f].LengthStr == len) {
                ci = c;
                fi = f;
                break;
            }
        }
    }
    call.nt_off = call.nt_len = 0;
    call.flags = (r.strand == '+' ? 0u : PG_INT_ANCHOR_MINUS) | (r.far_minus ? PG_INT_FAR_MINUS : 0u);
    if (ci < 0) {
        const UniquePoint &c = r.close[nc - 1], &f = r.far[nf - 1];
        const int effective = c.LengthStr + f.LengthStr;
        if (!(effective >= 30 && c.LengthStr >= 10 && f.LengthStr >= 10)) return false;
        // sub(UnmatchedSeq, f.LengthStr, (long)(unsigned)(len - effective)): a negative count runs to the end of the read
        const int n = effective > len ? len - f.LengthStr : len - effective;
        call.nt_off = (uint16_t)f.LengthStr;
        call.nt_len = (uint16_t)std::max(n, 0);
        call.flags |= PG_INT_FALLBACK;
        ci = nc - 1;
        fi = nf - 1;
    }
    call.close_abs = r.close[ci].AbsLoc;
    call.far_abs = r.far[fi].AbsLoc;
    return true;
}

bool int_key_less(const pg_int_call &x, const pg_int_call &y)
{
    return std::make_tuple(x.chr, x.far_chr, x.flags, x.close_abs, x.far_abs, x.nt_off, x.nt_len) <
           std::make_tuple(y.chr, y.far_chr, y.flags, y.close_abs, y.far_abs, y.nt_off, y.nt_len);
}

}  // namespace

// The contract of include/pindel_pg.h in plain loops: the call of every junction read, the reads that have one sorted by its key (a
// stable sort keeps the ascending read index), then one entry per distinct key.
void int_tables_from_reads(const std::vector<IntReadIn> &in, const int32_t *chr_rank, uint32_t n_chr, IntTables &out)
{
    out = IntTables();
    std::vector<std::pair<pg_int_call, uint32_t>> at;         // (key, read)
    for (size_t k = 0; k < in.size(); k++) {
        const IntReadIn &r = in[k];
        if (!r.n_close || !r.n_far || (r.strand != '+' && r.strand != '-')) continue;
        if (r.chr < 0 || (uint32_t)r.chr >= n_chr || r.far_chr < 0 || (uint32_t)r.far_chr >= n_chr) continue;
        if (chr_rank[r.chr] == chr_rank[r.far_chr]) continue;                     // FragName == FarFragName
        pg_int_call call;
        memset(&call, 0, sizeof call);
        const bool close_ascending = chr_rank[r.chr] < chr_rank[r.far_chr] ? r.strand == '+' : r.far_minus;   // (sic: the far strand)
        if (!int_read_call(r, close_ascending, call)) continue;
        call.chr = (int16_t)r.chr;
        call.far_chr = (int16_t)r.far_chr;
        at.push_back(std::make_pair(call, (uint32_t)k));
    }
    std::stable_sort(at.begin(), at.end(), [](const std::pair<pg_int_call, uint32_t> &x, const std::pair<pg_int_call, uint32_t> &y) {
        return int_key_less(x.first, y.first);
    });
    for (size_t i = 0; i < at.size();) {
        size_t j = i;
        while (j < at.size() && !int_key_less(at[i].first, at[j].first)) out.members.push_back(at[j++].second);
        pg_int_call call = at[i].first;
        call.first = (uint32_t)i;
        call.n_reads = (uint32_t)(j - i);
        out.calls.push_back(call);
        i = j;
    }
}

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
//
// The statement: the junction tables of the copied reads, chromosomes numbered by the order of their names.
void Caller::report_interchr()
{
    if (interchr_.empty()) return;
    std::set<std::string> names;
    for (const SplitRead &r : interchr_) {
        names.insert(r.FragName);
        names.insert(r.FarFragName);
    }
    auto id_of = [&](const std::string &name) { return (int)std::distance(names.begin(), names.find(name)); };
    std::vector<int32_t> rank(names.size());
    for (size_t k = 0; k < rank.size(); k++) rank[k] = (int32_t)k;
    std::vector<IntReadIn> in(interchr_.size());
    std::vector<uint32_t> junction(interchr_.size());
    for (size_t k = 0; k < interchr_.size(); k++) {
        const SplitRead &r = interchr_[k];
        IntReadIn &e = in[k];
        e.chr = id_of(r.FragName);
        e.far_chr = id_of(r.FarFragName);
        e.strand = r.MatchedD;
        e.far_minus = r.MatchedFarD == '-';
        e.read_length = r.getReadLength();
        e.close = r.UP_Close.data();
        e.n_close = r.UP_Close.size();
        e.far = r.UP_Far.data();
        e.n_far = r.UP_Far.size();
        junction[k] = (uint32_t)k;
    }
    IntTables tables;
    int_tables_from_reads(in, rank.data(), (uint32_t)rank.size(), tables);
    report_interchr_tables(interchr_, junction, tables);
    interchr_.clear();
}

void Caller::write_int_from_tables(const std::vector<SplitRead> &reads, const pg_report_summary *summaries, const IntTables &tables)
{
    std::vector<uint32_t> junction;
    for (size_t k = 0; k < reads.size(); k++)
        if ((summaries[k].flags & PG_RS_FAR) && reads[k].FragName != reads[k].FarFragName) junction.push_back((uint32_t)k);
    report_interchr_tables(reads, junction, tables);
}

// The consumer: pair policy, name set, the text of a call and the counting, from the tables and fields a read without points has.
void Caller::report_interchr_tables(const std::vector<SplitRead> &reads, const std::vector<uint32_t> &junction, const IntTables &tables)
{
    if (junction.empty()) return;
    std::set<std::string> names;
    for (uint32_t k : junction) {
        names.insert(reads[k].FragName);
        names.insert(reads[k].FarFragName);
    }
    std::vector<std::pair<std::string, std::string>> pairs;
    for (auto first = names.begin(); first != names.end(); ++first)
        for (auto second = std::next(first); second != names.end(); ++second) pairs.emplace_back(*first, *second);
    if (!S.repair(REPAIR_INT_PAIRS)) pairs.resize(1);       // the first pair takes every name
    const uint32_t NONE = ~0u;
    std::vector<uint32_t> call_of(reads.size(), NONE);      // the call of a read that has one
    for (size_t e = 0; e < tables.calls.size(); e++) {
        const pg_int_call &c = tables.calls[e];
        for (uint64_t m = c.first; m < (uint64_t)c.first + c.n_reads && m < tables.members.size(); m++)
            if (tables.members[(size_t)m] < reads.size()) call_of[tables.members[(size_t)m]] = (uint32_t)e;
    }
    // the text of a call up to its inserted bases, built when its first member is counted
    std::vector<std::string> head(tables.calls.size());
    auto text_of = [&](uint32_t e, const SplitRead &r) {
        const pg_int_call &c = tables.calls[e];
        if (head[e].empty()) {
            const bool anchor_minus = (c.flags & PG_INT_ANCHOR_MINUS) != 0;
            std::ostringstream o;
            o << "Anchor " << (anchor_minus ? "-" : "+") << " " << r.FragName << " " << (int)(c.close_abs - S.spacer) << " "
              << (anchor_minus ? "+" : "-") << " " << r.FarFragName << " " << (int)(c.far_abs - S.spacer) << " "
              << ((c.flags & PG_INT_FAR_MINUS) ? "-" : "+") << " ";
            head[e] = o.str();
        }
        // (a fallback group splits by its bases here: reads with equal offsets and different bases are different calls)
        return head[e] + "\"" + ((c.flags & PG_INT_FALLBACK) ? sub(r.UnmatchedSeq, c.nt_off, c.nt_len) : std::string()) + "\"";
    };
    std::set<std::string> seen;
    std::ofstream &out = open_append(int_out_, int_buf_, "_INT");
    for (const auto &pair : pairs) {
        std::map<std::string, int> calls;                   // CallAndSupport: call string -> reads, in string order
        for (uint32_t k : junction) {
            const SplitRead &r = reads[k];
            const bool ab = r.FragName == pair.first && r.FarFragName == pair.second;
            const bool ba = r.FragName == pair.second && r.FarFragName == pair.first;
            if (S.repair(REPAIR_INT_PAIRS) && !ab && !ba) continue;
            if (!seen.insert(r.Name).second) continue;
            if ((ab || ba) && call_of[k] != NONE) calls[text_of(call_of[k], r)]++;
        }
        for (const auto &kv : calls)
            if (kv.second >= 2) out << kv.first << "\tsupport: " << kv.second << '\n';
    }
    out.flush();
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
