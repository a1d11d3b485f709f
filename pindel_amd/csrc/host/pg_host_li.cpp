// pg_host_li.cpp -- the reports of the reads that have a close end and no far end:
//   SortOutputLI             src/reporter.cpp:1853-2141 (called last in SearchSVs, src/pindel.cpp:1167-1169)
//   ReportCloseMappedReads   src/pindel.cpp:1076-1092 (called before the far end, src/pindel.cpp:1880-1883)
// Both run on the host after the search; they read only UP_Close / UP_Far of the window's reads and the event
// breakpoints the four SV reporters left in CurrentChrMask (Caller::mark).
#include <algorithm>
#include <fstream>
#include <map>
#include <sstream>
#include <unordered_map>

#include "pg_host_priv.hpp"

namespace pgh {

using namespace detail;

std::ofstream &Caller::open_append(std::ofstream &f, std::vector<char> &buf, const char *suffix)
{
    if (!f.is_open()) {
        buf.resize(4u << 20);
        f.rdbuf()->pubsetbuf(buf.data(), (std::streamsize)buf.size());
        f.open((prefix + suffix).c_str(), std::ios::app);
    }
    return f;
}

void Caller::report_close_mapped(const std::vector<SplitRead> &reads)
{
    std::ofstream &out = open_append(cem_out_, cem_buf_, "_CloseEndMapped");
    for (const SplitRead &r : reads) {
        if (r.UP_Close.empty()) continue;
        out << r.Name << '\n' << r.UnmatchedSeq << '\n' << r.MatchedD << '\t' << r.FragName << '\t' << r.MatchedRelPos << '\t'
            << r.MS << '\t' << r.InsertSize << '\t' << r.Tag << '\n';
    }
    out.flush();
}

namespace {

const unsigned MAX_SHORT = 128;          // Max_short, src/pindel.h:126: the per-position counters stop there
const char *const LI_HASHES = "########################################################";
const char *const LI_DASHES = "--------------------------------------------------------";

// A per-position counter of the reference (a ShiftedVector over the buffered window, src/shifted_vector.h: indices
// outside [lo, hi] go to the nearest end), kept sparse: the positions that are non-zero, sorted, with their counts.
struct SparseCount {
    std::vector<std::pair<unsigned, unsigned>> v;
    void build(std::vector<unsigned> &pos)
    {
        std::sort(pos.begin(), pos.end());
        for (size_t i = 0; i < pos.size();) {
            size_t j = i;
            while (j < pos.size() && pos[j] == pos[i]) j++;
            v.push_back(std::make_pair(pos[i], (unsigned)std::min<size_t>(j - i, MAX_SHORT)));
            i = j;
        }
    }
    unsigned at(unsigned p) const
    {
        auto it = std::lower_bound(v.begin(), v.end(), std::make_pair(p, 0u));
        return it != v.end() && it->first == p ? it->second : 0u;
    }
};

}  // namespace

void Caller::sort_output_li(Ctx &c, unsigned win_start, unsigned win_end)
{
    std::vector<SplitRead> &reads = *c.reads;
    const std::string &chr = c.chrom->seq;
    const unsigned border = 4u * (unsigned)g_maxInsertSize;
    const unsigned abs_start = S.spacer + win_start;
    unsigned abs_end = S.spacer + win_end;
    if (abs_end > chr.size() - S.spacer) abs_end = (unsigned)(chr.size() - S.spacer);
    // the buffered window (the reference's unsigned start wraps for a border wider than the spacer; here it stops at 10)
    const unsigned lo = abs_start > border + 10 ? abs_start - border : 10u, hi = abs_end + border;
    auto clamp = [&](unsigned p) { return std::min(std::max(p, lo), hi); };
    auto li_read = [](const SplitRead &r) { return !r.Used && r.UP_Far.empty() && !r.UP_Close.empty(); };
    SparseCount plus_pos, minus_pos;
    {
        std::vector<unsigned> pp, mp;
        for (const SplitRead &r : reads) {
            if (!li_read(r)) continue;
            if (r.MatchedD == '+') pp.push_back(clamp(r.UP_Close.back().AbsLoc));
            else if (r.MatchedD == '-') mp.push_back(clamp(r.UP_Close.back().AbsLoc));
        }
        plus_pos.build(pp);
        minus_pos.build(mp);
    }
    const unsigned cutoff = S.NumRead2ReportCutOff;
    // the first mark the reference's downward scan from p + 10 to p - 10 meets: the largest marked position <= p + 10,
    // if it is >= p - 10
    auto mark_near = [&](unsigned p, unsigned &m) {
        auto it = chr_marks_.upper_bound(p + 10);
        if (it == chr_marks_.begin()) return false;
        --it;
        if (*it + 10 < p) return false;
        m = *it;
        return true;
    };
    // candidate (plus, minus) pairs: a '-' position with support, then a '+' position from one before it to 30 after
    // it; a mark within 10 of either skips ahead (and moves the '-' position on, which also moves the inner bound).
    // The reference visits every position of the buffered window; only those with a mark within 10 or with '-'
    // support do anything, so the walk goes from one such position to the next (with -M 0 every position has support).
    struct Pos { unsigned plus, minus; std::vector<unsigned> p_reads, m_reads; };
    std::vector<Pos> positions;
    std::unordered_map<unsigned, int> event_of;
    size_t next_minus = 0;
    for (unsigned im = lo; im < hi; im++) {
        if (cutoff > 0) {
            unsigned next = hi;
            while (next_minus < minus_pos.v.size() && (minus_pos.v[next_minus].first < im || minus_pos.v[next_minus].second < cutoff))
                next_minus++;
            if (next_minus < minus_pos.v.size()) next = minus_pos.v[next_minus].first;
            auto mk = chr_marks_.lower_bound(im - 10);
            if (mk != chr_marks_.end()) next = std::min(next, std::max(im, *mk - 10));
            if (next >= hi) break;
            im = next;
        }
        unsigned m;
        if (mark_near(im, m)) {
            im = m + 10;
            continue;
        }
        if (minus_pos.at(clamp(im)) < cutoff) continue;
        for (unsigned ip = im - 1; ip <= im + 30; ip++) {
            if (mark_near(ip, m)) {
                if (m + 10 > im) im = m + 10;
                continue;
            }
            if (plus_pos.at(clamp(ip)) >= cutoff) {
                Pos q;
                q.plus = ip;
                q.minus = im;
                positions.push_back(q);
                event_of[clamp(ip)] = (int)positions.size() - 1;
                event_of[clamp(im)] = (int)positions.size() - 1;
            }
        }
    }
    for (unsigned i = 0; i < reads.size(); i++) {
        SplitRead &r = reads[i];
        if (!li_read(r)) continue;
        auto e = event_of.find(clamp(r.UP_Close.back().AbsLoc));
        if (e == event_of.end()) continue;
        r.Used = true;
        (r.MatchedD == '+' ? positions[(size_t)e->second].p_reads : positions[(size_t)e->second].m_reads).push_back(i);
    }
    const std::vector<std::string> names(g_sampleNames.begin(), g_sampleNames.end());
    std::map<std::string, size_t> index;
    for (size_t k = 0; k < names.size(); k++) index[names[k]] = k;
    const long rl = g_reportLength;
    std::ostringstream out;
    for (const Pos &q : positions) {
        if (q.m_reads.empty() || q.p_reads.empty()) continue;
        // balance: some supporting read's close end is longer (shorter) than half of it
        bool bal[4] = { false, false, false, false };     // +: longer, shorter; -: longer, shorter
        auto balance = [&](const std::vector<unsigned> &v, bool *b) {
            for (unsigned i : v) {
                const SplitRead &r = reads[i];
                const float len = (float)r.UP_Close.back().LengthStr;
                if (len > r.getReadLength() * 0.5) b[0] = true;
                else if (len < r.getReadLength() * 0.5) b[1] = true;
            }
        };
        balance(q.p_reads, bal);
        balance(q.m_reads, bal + 2);
        std::vector<unsigned> sup_p(names.size(), 0), sup_m(names.size(), 0);
        auto sample = [&](const SplitRead &r) {        // (a tag outside the set: index 0, as std::map::operator[] gives)
            auto it = index.find(r.Tag);
            return it == index.end() ? (size_t)0 : it->second;
        };
        for (unsigned i : q.m_reads) sup_m[sample(reads[i])]++;
        for (unsigned i : q.p_reads) sup_p[sample(reads[i])]++;
        bool one_sample = false;
        for (size_t k = 0; k < names.size(); k++)
            if (sup_p[k] > 0 && sup_m[k] > 0) {
                one_sample = true;
                break;
            }
        if (!one_sample || !(bal[0] || bal[1] || bal[2] || bal[3])) continue;
        const SplitRead &first = reads[q.p_reads[0]];
        out << LI_HASHES << '\n';
        out << count_li_++ << "\tLI\tChrID " << first.FragName << '\t' << q.plus - S.spacer + 1 << "\t+ " << q.p_reads.size()
            << '\t' << q.minus - S.spacer + 1 << "\t- " << q.m_reads.size();
        for (size_t k = 0; k < names.size(); k++) out << '\t' << names[k] << " + " << sup_p[k] << " - " << sup_m[k];
        out << '\n';
        out << sub(chr, (long)q.plus - rl + 1, rl) << cap2low(sub(chr, (long)q.plus + 1, rl)) << '\n';
        for (unsigned i : q.p_reads) {
            const SplitRead &r = reads[i];
            const long indent = rl - r.UP_Close.back().LengthStr;
            out << std::string(indent > 0 ? (size_t)indent : 0, ' ') << reverse_complement(r.UnmatchedSeq) << '\t' << r.MatchedD
                << '\t' << r.MatchedRelPos << '\t' << r.MS << '\t' << r.Tag << '\t' << r.Name << '\n';
        }
        out << LI_DASHES << '\n';
        out << cap2low(sub(chr, (long)q.minus - rl, rl)) << sub(chr, (long)q.minus, rl) << '\n';
        for (unsigned i : q.m_reads) {
            const SplitRead &r = reads[i];
            const long indent = rl + r.UP_Close.back().LengthStr - r.getReadLength();
            // (no tab between the sequence and MatchedD, as in reporter.cpp)
            out << std::string(indent > 0 ? (size_t)indent : 0, ' ') << r.UnmatchedSeq << r.MatchedD << '\t' << r.MatchedRelPos
                << '\t' << r.MS << '\t' << r.Tag << '\t' << r.Name << '\n';
        }
    }
    std::ofstream &f = open_append(li_out_, li_buf_, "_LI");
    const std::string text = out.str();
    f.write(text.data(), (std::streamsize)text.size());
    f.flush();
}

}  // namespace pgh
