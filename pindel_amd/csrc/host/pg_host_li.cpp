// pg_host_li.cpp -- the reports of the reads that have a close end and no far end:
//   SortOutputLI             src/reporter.cpp:1853-2141 (called last in SearchSVs, src/pindel.cpp:1167-1169)
//   ReportCloseMappedReads   src/pindel.cpp:1076-1092 (called before the far end, src/pindel.cpp:1880-1883)
// Both run on the host after the search; they read only UP_Close / UP_Far of the window's reads and the event
// breakpoints the four SV reporters left in CurrentChrMask (Caller::mark).  SortOutputLI comes in two parts:
// li_tables_from_reads -- the per-position counters with their member reads as tables, the host statement of pg_li.hip --
// and sort_output_li_tables, the one consumer of such tables, wherever they were built.
#include <algorithm>
#include <chrono>
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

void Caller::report_close_mapped_summaries(const std::vector<SplitRead> &reads, const pg_report_summary *summaries)
{
    std::ofstream &out = open_append(cem_out_, cem_buf_, "_CloseEndMapped");
    for (size_t k = 0; k < reads.size(); k++) {
        if (!(summaries[k].flags & PG_RS_CLOSE)) continue;
        const SplitRead &r = reads[k];
        out << r.Name << '\n' << r.UnmatchedSeq << '\n' << r.MatchedD << '\t' << r.FragName << '\t' << r.MatchedRelPos << '\t'
            << r.MS << '\t' << r.InsertSize << '\t' << r.Tag << '\n';
    }
    out.flush();
}

// The contract of include/pindel_pg.h in plain loops: per strand the LI reads by clamped position (a stable sort keeps the
// ascending read index), then one entry per distinct position.
void li_tables_from_reads(const std::vector<LiReadIn> &in, const pg_event_read *recs, uint32_t lo, uint32_t hi, LiTables &out)
{
    out = LiTables();
    for (int s = 0; s < 2; s++) {
        std::vector<std::pair<uint32_t, uint32_t>> at;       // (clamped position, read)
        for (size_t k = 0; k < in.size(); k++) {
            const LiReadIn &r = in[k];
            if (!r.in_window || !r.has_close || r.has_far || r.used) continue;
            if (recs && (recs[k].flags & (PG_EVR_BOXED | PG_EVR_USED))) continue;
            if (r.strand != (s == 0 ? '+' : '-')) continue;
            at.push_back(std::make_pair(std::min(std::max(r.close_abs, lo), hi), (uint32_t)k));
        }
        std::stable_sort(at.begin(), at.end(), [](const std::pair<uint32_t, uint32_t> &x, const std::pair<uint32_t, uint32_t> &y) { return x.first < y.first; });
        for (size_t i = 0; i < at.size();) {
            size_t j = i;
            pg_li_pos p = { at[i].first, (uint32_t)i, 0u, 0u };
            for (; j < at.size() && at[j].first == at[i].first; j++) {
                const LiReadIn &r = in[at[j].second];
                if (2 * r.close_len > r.read_length) p.flags |= PG_LI_LONGER;
                if (2 * r.close_len < r.read_length) p.flags |= PG_LI_SHORTER;
                out.members[s].push_back(at[j].second);
            }
            p.n_reads = (uint32_t)(j - i);
            out.positions[s].push_back(p);
            i = j;
        }
    }
}

namespace {

const unsigned MAX_SHORT = 128;          // Max_short, src/pindel.h:126: the per-position counters stop there
const char *const LI_HASHES = "########################################################";
const char *const LI_DASHES = "--------------------------------------------------------";

// A per-position counter of the reference (a ShiftedVector over the buffered window, src/shifted_vector.h: indices
// outside [lo, hi] go to the nearest end) read from a position table: the count saturates at Max_short here.
const pg_li_pos *li_find(const std::vector<pg_li_pos> &v, unsigned p)
{
    auto it = std::lower_bound(v.begin(), v.end(), p, [](const pg_li_pos &x, unsigned q) { return x.pos < q; });
    return it != v.end() && it->pos == p ? &*it : nullptr;
}
unsigned li_count(const pg_li_pos &p) { return std::min<unsigned>(p.n_reads, MAX_SHORT); }
unsigned li_at(const std::vector<pg_li_pos> &v, unsigned p)
{
    const pg_li_pos *q = li_find(v, p);
    return q ? li_count(*q) : 0u;
}

}  // namespace

void Caller::li_window(const Chromosome &chrom, unsigned win_start, unsigned win_end, unsigned &lo, unsigned &hi) const
{
    const std::string &chr = chrom.seq;
    const unsigned border = 4u * (unsigned)g_maxInsertSize;
    const unsigned abs_start = S.spacer + win_start;
    unsigned abs_end = S.spacer + win_end;
    if (abs_end > chr.size() - S.spacer) abs_end = (unsigned)(chr.size() - S.spacer);
    // the buffered window (the reference's unsigned start wraps for a border wider than the spacer; here it stops at 10)
    lo = abs_start > border + 10 ? abs_start - border : 10u;
    hi = abs_end + border;
}

void Caller::write_li_from_tables(const Chromosome &chrom, std::vector<SplitRead> &reads, unsigned win_start, unsigned win_end,
                                  const LiTables &tables, const pg_report_summary *summaries)
{
    const double t0 = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    Ctx c;
    c.chrom = &chrom;
    c.reads = &reads;
    unsigned lo, hi;
    li_window(chrom, win_start, win_end, lo, hi);
    std::vector<int16_t> close_len(reads.size());
    for (size_t k = 0; k < reads.size(); k++) close_len[k] = summaries[k].close_len;
    sort_output_li_tables(c, lo, hi, tables, close_len.data());
    li_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count() - t0;
}

void Caller::sort_output_li(Ctx &c, unsigned win_start, unsigned win_end)
{
    unsigned lo, hi;
    li_window(*c.chrom, win_start, win_end, lo, hi);
    if (c.li_ready) {                    // (the tables route: the reads have no points any more)
        sort_output_li_tables(c, lo, hi, c.li, c.li_close_len.data());
        return;
    }
    const std::vector<SplitRead> &reads = *c.reads;
    std::vector<LiReadIn> in(reads.size());
    std::vector<int16_t> close_len(reads.size(), 0);
    for (size_t k = 0; k < reads.size(); k++) {
        const SplitRead &r = reads[k];
        LiReadIn &e = in[k];
        e.has_close = !r.UP_Close.empty();
        e.has_far = !r.UP_Far.empty();
        e.used = r.Used;
        e.strand = r.MatchedD;
        e.read_length = r.getReadLength();
        if (e.has_close) {
            e.close_abs = r.UP_Close.back().AbsLoc;
            e.close_len = close_len[k] = r.UP_Close.back().LengthStr;
        }
    }
    LiTables tables;
    li_tables_from_reads(in, nullptr, lo, hi, tables);
    sort_output_li_tables(c, lo, hi, tables, close_len.data());
}

void Caller::sort_output_li_tables(Ctx &c, unsigned lo, unsigned hi, const LiTables &tables, const int16_t *close_len)
{
    std::vector<SplitRead> &reads = *c.reads;
    const std::string &chr = c.chrom->seq;
    auto clamp = [&](unsigned p) { return std::min(std::max(p, lo), hi); };
    const std::vector<pg_li_pos> &plus_pos = tables.positions[0], &minus_pos = tables.positions[1];
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
    struct Pos { unsigned plus, minus; std::vector<unsigned> p_reads, m_reads; unsigned bal[2] = { 0u, 0u }; };
    std::vector<Pos> positions;
    std::unordered_map<unsigned, int> event_of;
    size_t next_minus = 0;
    for (unsigned im = lo; im < hi; im++) {
        if (cutoff > 0) {
            unsigned next = hi;
            while (next_minus < minus_pos.size() && (minus_pos[next_minus].pos < im || li_count(minus_pos[next_minus]) < cutoff)) next_minus++;
            if (next_minus < minus_pos.size()) next = minus_pos[next_minus].pos;
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
        if (li_at(minus_pos, clamp(im)) < cutoff) continue;
        for (unsigned ip = im - 1; ip <= im + 30; ip++) {
            if (mark_near(ip, m)) {
                if (m + 10 > im) im = m + 10;
                continue;
            }
            if (li_at(plus_pos, clamp(ip)) >= cutoff) {
                Pos q;
                q.plus = ip;
                q.minus = im;
                positions.push_back(q);
                event_of[clamp(ip)] = (int)positions.size() - 1;
                event_of[clamp(im)] = (int)positions.size() - 1;
            }
        }
    }
    // event_of is keyed by position whatever the strand: an event takes the members of BOTH strands' tables at every position
    // mapped to it, in ascending read index (the order of the reference's pass over the reads)
    for (const auto &e : event_of) {
        Pos &q = positions[(size_t)e.second];
        for (int s = 0; s < 2; s++) {
            const pg_li_pos *p = li_find(tables.positions[s], e.first);
            if (!p) continue;
            std::vector<unsigned> &into = s == 0 ? q.p_reads : q.m_reads;
            into.insert(into.end(), tables.members[s].begin() + p->first, tables.members[s].begin() + p->first + p->n_reads);
            q.bal[s] |= p->flags;
        }
    }
    for (Pos &q : positions) {
        std::sort(q.p_reads.begin(), q.p_reads.end());
        std::sort(q.m_reads.begin(), q.m_reads.end());
        for (unsigned i : q.p_reads) reads[i].Used = true;
        for (unsigned i : q.m_reads) reads[i].Used = true;
    }
    const std::vector<std::string> names(g_sampleNames.begin(), g_sampleNames.end());
    std::map<std::string, size_t> index;
    for (size_t k = 0; k < names.size(); k++) index[names[k]] = k;
    const long rl = g_reportLength;
    std::ostringstream out;
    for (const Pos &q : positions) {
        if (q.m_reads.empty() || q.p_reads.empty()) continue;
        // balance: some supporting read's close end is longer (shorter) than half of it -- PG_LI_LONGER / PG_LI_SHORTER of either strand
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
        if (!one_sample || !((q.bal[0] | q.bal[1]) & (PG_LI_LONGER | PG_LI_SHORTER))) continue;
        const SplitRead &first = reads[q.p_reads[0]];
        out << LI_HASHES << '\n';
        out << count_li_++ << "\tLI\tChrID " << first.FragName << '\t' << q.plus - S.spacer + 1 << "\t+ " << q.p_reads.size()
            << '\t' << q.minus - S.spacer + 1 << "\t- " << q.m_reads.size();
        for (size_t k = 0; k < names.size(); k++) out << '\t' << names[k] << " + " << sup_p[k] << " - " << sup_m[k];
        out << '\n';
        out << sub(chr, (long)q.plus - rl + 1, rl) << cap2low(sub(chr, (long)q.plus + 1, rl)) << '\n';
        for (unsigned i : q.p_reads) {
            const SplitRead &r = reads[i];
            const long indent = rl - close_len[i];
            out << std::string(indent > 0 ? (size_t)indent : 0, ' ') << reverse_complement(r.UnmatchedSeq) << '\t' << r.MatchedD
                << '\t' << r.MatchedRelPos << '\t' << r.MS << '\t' << r.Tag << '\t' << r.Name << '\n';
        }
        out << LI_DASHES << '\n';
        out << cap2low(sub(chr, (long)q.minus - rl, rl)) << sub(chr, (long)q.minus, rl) << '\n';
        for (unsigned i : q.m_reads) {
            const SplitRead &r = reads[i];
            const long indent = rl + close_len[i] - r.getReadLength();
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
