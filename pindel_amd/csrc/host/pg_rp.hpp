// pg_rp.hpp -- discordant read pairs of a window as BreakDancer-like events (second half):
// what `-R` (default on for BAM input) adds to the far-end search windows.
//
// Restated from the reference (no code shared):
//   fetch_func_RP_Discovery / build_record_RP_Discovery   src/reader.cpp:925-1097, 1197-1245   which pairs count
//   get_RP_Reads_Discovery                                 src/reader.cpp:1378-1410             all BAMs of the run
//   BDData::UpdateBD                                       src/bddata.cpp:646-812               events = external + RP
//   ModifyRP / InitializeA1B1 / RecipicalOverlap / ProcessSameChromosomeSameStrand / Summarize
//                                                          src/bddata.cpp:138-560
// The reference's arithmetic is kept as written, including `abs()` of unsigned differences (taken as int) and the
// never-true `shift_distance * 2 < shift_distance` of the second coordinate.  Its OpenMP loops race (ModifyRP updates
// reads that other iterations read; UpdateBD pushes events in completion order): this is the sequential order,
// and the final event list is sorted anyway.
//
// Interchromosomal pairs (`-I`, default off): build_record_RP_Discovery keeps a pair with tid != mtid as it is (no swap
// of sides) in a list of its own; with -I, UpdateBD clusters that list after the same-chromosome one
// (ModifyRP_InterChr / Summarize_InterChr, src/bddata.cpp:362-383, 439-468, 581-623, 735-806): rp_events_interchr below.
//
// PARITY STATUS: unpinned -- the reference's BAM path cannot be built here (htslib) and the one BAM it ships
// (demo/simulated_MEI) has no same-chromosome discordant cluster: checked against an independent restatement on
// synthetic pairs (tests/test_bam_ingest.py) and on that BAM (tests/test_mei_bam.py: both find no event).
#ifndef PG_RP_HPP
#define PG_RP_HPP

#include <algorithm>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "pg_bam.hpp"

namespace pgh {

struct RpRead {
    std::string ChrNameA, ChrNameB;
    int ChrA = -1, ChrB = -1;          // their indices in the BAM header (what rp_events_interchr compares)
    char DA = 'k', DB = 'k';
    unsigned PosA = 0, PosB = 0, OriginalPosA = 0, OriginalPosB = 0, PosA1 = 0, PosB1 = 0;
    int InsertSize = 0;
    short ReadLength = 0;
    unsigned NumberOfIdentical = 0;
    bool Report = false, Visited = false;
    std::vector<std::string> Tags;
};

struct RpEvent {                       // one BreakDancerEvent (both directions are derived by the consumer)
    std::string chr1, chr2;
    unsigned pos1, pos1b, pos2, pos2b; // Pindel coordinates (spacer included): position, position2 of each side
};

// build_record_RP_Discovery for every record of the window: same-chromosome pairs are appended to `out`, pairs whose
// mate lies on another chromosome to `interchr` when that is given (LeftReads_InterChr; left out otherwise)
inline bool rp_discover(BamFile &bam, const std::string &chr_name, int64_t win_start, int64_t win_end, int insert_size,
                        const std::string &tag, unsigned min_anchor_quality, std::vector<RpRead> &out,
                        std::vector<RpRead> *interchr = nullptr)
{
    const BamHeader &hdr = bam.header();
    const int tid = hdr.id_of(chr_name);
    auto consider = [&](const BamRecord &r, std::vector<RpRead> &dst, std::vector<RpRead> *dst_inter) {
        if (!(r.flag & BAM_FPAIRED)) return;
        if (r.mapq < min_anchor_quality) return;
        if ((r.flag & BAM_FUNMAP) || (r.flag & BAM_FMUNMAP)) return;                     // both mates mapped
        const bool rev = (r.flag & BAM_FREVERSE) != 0, mrev = (r.flag & BAM_FMREVERSE) != 0;
        if (!((r.tid != r.mtid) || std::abs(r.tlen) > 3 * insert_size + 1000 || rev == mrev)) return;
        if (r.tid != r.mtid && !dst_inter) return;                                        // (only -I uses that list)
        if (r.mtid < 0 || (size_t)r.mtid >= hdr.names.size()) return;
        RpRead t;
        t.DA = rev ? '-' : '+';
        t.DB = mrev ? '-' : '+';
        t.PosA = t.OriginalPosA = (unsigned)r.pos;
        t.PosB = t.OriginalPosB = (unsigned)r.mpos;
        t.ChrNameA = hdr.names[(size_t)r.tid];
        t.ChrNameB = hdr.names[(size_t)r.mtid];
        t.ChrA = r.tid;
        t.ChrB = r.mtid;
        t.InsertSize = insert_size;
        t.Tags.push_back(tag);
        t.ReadLength = (short)r.l_seq;
        if (r.tid != r.mtid) {                                                            // as it is: no swap of sides
            dst_inter->push_back(t);
            return;
        }
        if (!(t.PosA < t.PosB)) {                                                         // first coordinate = the smaller one
            std::swap(t.DA, t.DB);
            std::swap(t.PosA, t.PosB);
            std::swap(t.OriginalPosA, t.OriginalPosB);
            std::swap(t.ChrNameA, t.ChrNameB);
            std::swap(t.ChrA, t.ChrB);
        }
        dst.push_back(t);
    };
    // with an index: sub-ranges of the window on several threads, taken in order afterwards (BamFile::query_split)
    const unsigned nt = bam.split_parts(tid, win_start, win_end);
    if (nt > 1) {
        std::vector<std::vector<RpRead>> parts(nt), parts_inter(nt);
        if (!bam.query_split(tid, win_start, win_end, nt, [&](unsigned t, const BamRecord &r, const BamFile &) {
                consider(r, parts[t], interchr ? &parts_inter[t] : nullptr);
            }))
            return false;
        for (const std::vector<RpRead> &part : parts) out.insert(out.end(), part.begin(), part.end());
        if (interchr)
            for (const std::vector<RpRead> &part : parts_inter) interchr->insert(interchr->end(), part.begin(), part.end());
        return true;
    }
    return bam.query(tid, win_start, win_end, [&](const BamRecord &r) { consider(r, out, interchr); });
}

namespace rp_detail {

inline int iabs_u(unsigned a, unsigned b) { return std::abs((int)(a - b)); }            // abs(unsigned - unsigned) as the reference compiles it

inline bool reciprocal_overlap(const RpRead &first, const RpRead &second)
{
    const int distance = 1000;
    if (iabs_u(first.PosA, first.PosA1) > distance || iabs_u(first.PosB, first.PosB1) > distance ||
        iabs_u(second.PosA, second.PosA1) > distance || iabs_u(second.PosB, second.PosB1) > distance)
        return false;
    const float cutoff = 0.9f;
    unsigned fa = (first.PosA + first.PosA1) / 2, fb = (first.PosB + first.PosB1) / 2;
    if (fa > fb) std::swap(fa, fb);
    unsigned sa = (second.PosA + second.PosA1) / 2, sb = (second.PosB + second.PosB1) / 2;
    if (sa > sb) std::swap(sa, sb);
    if (first.DA != second.DA || first.DB != second.DB) return false;
    if (fa > sb + 200 || fb + 200 < sa) return false;
    if (fa <= sa && sb <= fb && (double)(sb - sa) / (double)(fb - fa) >= cutoff) return true;
    if (sa <= fa && fb <= sb && (double)(fb - fa) / (double)(sb - sa) >= cutoff) return true;
    if (fa <= sa && sa <= fb && fb <= sb && (double)(fb - sa) / (double)(fb - fa) >= cutoff &&
        (double)(fb - sa) / (double)(sb - sa) >= cutoff)
        return true;
    if (sa <= fa && fa <= sb && sb <= fb && (double)(sb - fa) / (double)(fb - fa) >= cutoff &&
        (double)(sb - fa) / (double)(sb - sa) >= cutoff)
        return true;
    return false;
}

inline void initialize_a1b1(std::vector<RpRead> &v)
{
    for (RpRead &r : v) {
        const unsigned D = (unsigned)r.InsertSize, L = (unsigned)r.ReadLength;
        if (r.DA == '+') {
            r.PosA = r.PosA > L * 2 ? r.PosA - L * 2 : 1;
            r.PosA1 = r.PosA + D + L * 2;
        } else {
            r.PosA = r.PosA > D ? r.PosA - D : 1;
            r.PosA1 = r.PosA + D + L;
        }
        if (r.DB == '+') {
            r.PosB = r.PosB > L * 2 ? r.PosB - L * 2 : 1;
            r.PosB1 = r.PosB + D + L;
        } else {
            r.PosB = r.PosB > D ? r.PosB - D : 1;
            r.PosB1 = r.PosB + D + L;
        }
    }
}

// ProcessSameChromosomeSameStrand on `first` and the box [sA, sA1] x [sB, sB1] of `second`
inline void same_chr_same_strand(RpRead &f, unsigned sA, unsigned sA1, unsigned sB, unsigned sB1)
{
    if (sA1 - sA > 10000 || sB1 - sB > 10000) return;
    if ((f.DA == '+' && f.PosA < sA && sA < f.PosA1 && f.PosA1 < sA1) ||
        (f.DA == '-' && f.PosA < sA1 && sA1 < f.PosA1 && sA < f.PosA)) {
        f.PosA = sA;
        f.PosA1 = sA1;
    }
    if ((f.DB == '+' && f.PosB < sB && sB < f.PosB1 && f.PosB1 < sB1) ||
        (f.DB == '-' && sB < f.PosB && f.PosB < sB1 && sB1 < f.PosB1)) {
        f.PosB = sB;
        f.PosB1 = sB1;
    }
}
inline void same_chr_same_strand(RpRead &f, const RpRead &s) { same_chr_same_strand(f, s.PosA, s.PosA1, s.PosB, s.PosB1); }

inline void modify_rp(std::vector<RpRead> &v)
{
    if (v.empty()) return;
    std::sort(v.begin(), v.end(), [](const RpRead &a, const RpRead &b) {          // Compare2RP: descending
        if (a.OriginalPosA > b.OriginalPosA) return true;
        if (a.OriginalPosA == b.OriginalPosA) return a.OriginalPosB > b.OriginalPosB;
        return false;
    });
    initialize_a1b1(v);
    for (size_t i = 0; i < v.size(); i++)
        for (size_t j = 0; j < v.size(); j++) {
            const RpRead &second = v[j];                                           // (i == j: itself; nothing changes)
            if (reciprocal_overlap(v[i], second) && v[i].DA == second.DA && v[i].DB == second.DB) same_chr_same_strand(v[i], second);
        }
    for (RpRead &r : v) {
        if (r.DA == '+') { r.PosA += (unsigned)r.ReadLength; r.PosA1 += (unsigned)r.ReadLength; }
        if (r.DB == '+') { r.PosB += (unsigned)r.ReadLength; r.PosB1 += (unsigned)r.ReadLength; }
        if (r.ChrNameA == r.ChrNameB && iabs_u(r.PosA, r.PosB) < 500) r.Visited = true;
    }
}

inline bool same_box(const RpRead &a, const RpRead &b)
{
    return a.PosA == b.PosA && a.PosB == b.PosB && a.PosA1 == b.PosA1 && a.PosB1 == b.PosB1 && a.DA == b.DA && a.DB == b.DB;
}

inline void summarize(std::vector<RpRead> &v)
{
    const unsigned Cutoff = 5;
    if (v.size() < 5) {
        for (RpRead &r : v) r.Report = false;
        return;
    }
    std::vector<size_t> good;
    for (size_t i = 0; i + 1 < v.size(); i++) {
        if (v[i].Visited) continue;
        v[i].NumberOfIdentical = 1;
        for (size_t j = i + 1; j < v.size(); j++) {
            if (v[j].Visited) continue;
            if (same_box(v[i], v[j])) {
                v[i].NumberOfIdentical++;
                v[j].Visited = true;
                v[i].Tags.insert(v[i].Tags.end(), v[j].Tags.begin(), v[j].Tags.end());
                v[j].Tags.clear();
            }
        }
        good.push_back(i);
    }
    if (good.empty()) return;
    if (good.size() == 1) {
        v[good[0]].Report = v[good[0]].NumberOfIdentical >= Cutoff;
        return;
    }
    for (size_t a = 0; a + 1 < good.size(); a++) {
        RpRead &ra = v[good[a]];
        if (ra.Visited) continue;
        for (size_t b = a + 1; b < good.size(); b++) {
            RpRead &rb = v[good[b]];
            if (rb.Visited) continue;
            if (same_box(ra, rb)) {
                ra.NumberOfIdentical += rb.NumberOfIdentical;
                rb.Visited = true;
                ra.Tags.insert(ra.Tags.end(), rb.Tags.begin(), rb.Tags.end());
                rb.Tags.clear();
            }
        }
        ra.Report = ra.NumberOfIdentical >= Cutoff;
    }
}

}  // namespace rp_detail

// BDData::UpdateBD for the read pairs of one window: the events they support (>= 5 identical pairs), in the
// reference's order of discovery; `rp_out` (nullable) receives the lines the reference appends to <prefix>_RP.
// `left` (nullable) receives the list as it stands when UpdateBD clears it (src/bddata.cpp:733): sorted, boxes set by
// ModifyRP -- what IsGoodINV was written to count in (--repair inv-pairs).
inline std::vector<RpEvent> rp_events(std::vector<RpRead> &reads, unsigned spacer, std::ofstream *rp_out,
                                      std::vector<RpRead> *left = nullptr)
{
    using namespace rp_detail;
    std::vector<RpEvent> events;
    std::sort(reads.begin(), reads.end(), [](const RpRead &a, const RpRead &b) {   // SortByFirstAndThenSecondCoordinate
        if (a.PosA != b.PosA) return a.PosA < b.PosA;
        if (a.PosB != b.PosB) return a.PosB < b.PosB;
        return false;
    });
    modify_rp(reads);
    summarize(reads);
    for (RpRead &r : reads) {
        if (!r.Report) continue;
        const unsigned shift = (unsigned)r.InsertSize;
        unsigned f1 = r.PosA + spacer, f2 = r.PosA1 + spacer;
        if (f1 > f2) std::swap(f1, f2);
        if (r.DA == '+' && f1 > shift) f1 -= shift;
        else if (shift * 2 < spacer) f2 += shift;
        unsigned s1 = r.PosB + spacer, s2 = r.PosB1 + spacer;
        if (s1 > s2) std::swap(s1, s2);
        if (r.DB == '+' && s1 > shift) s1 -= shift;
        // (the reference's "else if (shift_distance * 2 < shift_distance)" never holds: s2 stays)
        if (r.ChrNameA.empty() || r.ChrNameB.empty()) continue;
        RpEvent e = { r.ChrNameA, r.ChrNameB, f1, f2, s1, s2 };
        events.push_back(e);
        if (rp_out) {
            std::ofstream &o = *rp_out;
            o << r.ChrNameA << "\t" << (f1 > spacer ? f1 - spacer : 1) << "\t" << f2 - spacer << "\t" << r.DA << "\t" << f2 - f1 << "\t"
              << r.ChrNameB << "\t" << (s1 > spacer ? s1 - spacer : 1) << "\t" << s2 - spacer << "\t" << r.DB << "\t" << s2 - s1 << "\t"
              << std::abs((int)s1 - (int)f1) << "\tSupport: " << r.NumberOfIdentical << "\t";
            // DisplayBDSupportPerSample: tags sorted, "\t<tag> <count>" per tag
            std::sort(r.Tags.begin(), r.Tags.end());
            for (size_t i = 0; i < r.Tags.size();) {
                size_t j = i;
                while (j < r.Tags.size() && r.Tags[j] == r.Tags[i]) j++;
                o << "\t" << r.Tags[i] << " " << (j - i);
                i = j;
            }
            o << std::endl;
        }
    }
    if (left) left->swap(reads);
    reads.clear();
    return events;
}

namespace rp_detail {

// The reads a read can meet in the two double loops below: those of its chromosome pair, either way round, by ascending
// index.  group_of[i] = the list read i belongs to.
struct PairGroups {
    std::vector<std::vector<uint32_t>> members;
    std::vector<uint32_t> group_of;
    explicit PairGroups(const std::vector<RpRead> &v) : group_of(v.size())
    {
        std::vector<std::pair<std::pair<int, int>, uint32_t>> keyed(v.size());
        for (uint32_t i = 0; i < v.size(); i++) keyed[i] = { { std::min(v[i].ChrA, v[i].ChrB), std::max(v[i].ChrA, v[i].ChrB) }, i };
        std::sort(keyed.begin(), keyed.end());
        for (size_t k = 0; k < keyed.size(); k++) {
            if (k == 0 || keyed[k].first != keyed[k - 1].first) members.emplace_back();
            members.back().push_back(keyed[k].second);
            group_of[keyed[k].second] = (uint32_t)(members.size() - 1);
        }
    }
};

// ModifyRP_InterChr (src/bddata.cpp:439-468) with UpdateFirstBasedOnSecondInterChromosome (:362-383).  The reference's loop
// is serial and order-dependent: `first` is rewritten while it sweeps over every `second`, and later `first`s read the
// rewritten values.  A `second` of another chromosome pair is a no-op, so each `first` sweeps its own group only -- in
// the same ascending index order; groups do not read each other, so they are done one after the other, each on a
// compact copy of its boxes.  The same chromosome pair: ProcessSameChromosomeSameStrand when the strands agree; the
// pair with its sides swapped: `second` is looked at with its sides exchanged.  The last read is never a `first` (the
// loop stops at size() - 1), and no read length is added afterwards (unlike ModifyRP).
inline void modify_rp_interchr(std::vector<RpRead> &v, const PairGroups &g)
{
    struct Box {
        unsigned a, a1, b, b1;
        int chr_a;
        char da, db;
    };
    std::vector<Box> box;
    for (const std::vector<uint32_t> &m : g.members) {
        box.resize(m.size());
        for (size_t x = 0; x < m.size(); x++) {
            const RpRead &r = v[m[x]];
            box[x] = { r.PosA, r.PosA1, r.PosB, r.PosB1, r.ChrA, r.DA, r.DB };
        }
        for (size_t x = 0; x < m.size(); x++) {
            if ((size_t)m[x] + 1 == v.size()) continue;
            RpRead &f = v[m[x]];
            for (size_t y = 0; y < m.size(); y++) {
                const Box &s = box[y];
                if (y == x) continue;                       // (itself: every test of the update is strict, nothing changes)
                if (f.ChrA == s.chr_a) {                    // the same pair the same way round (the group holds both ways only)
                    if (f.DA == s.da && f.DB == s.db) same_chr_same_strand(f, s.a, s.a1, s.b, s.b1);
                } else if (f.DA == s.db && f.DB == s.da)
                    same_chr_same_strand(f, s.b, s.b1, s.a, s.a1);
            }
            box[x].a = f.PosA;
            box[x].a1 = f.PosA1;
            box[x].b = f.PosB;
            box[x].b1 = f.PosB1;
        }
    }
}

// Summarize_InterChr (src/bddata.cpp:581-623): the count starts at 0 (so >= 5 means five OTHER pairs), only PosA / PosB
// are compared (not PosA1 / PosB1), and the last read is never a `first`.
inline void summarize_interchr(std::vector<RpRead> &v, const PairGroups &g)
{
    const unsigned Cutoff = 5;
    for (size_t i = 0; i + 1 < v.size(); i++) {
        RpRead &f = v[i];
        if (f.Visited) continue;
        f.NumberOfIdentical = 0;
        const std::vector<uint32_t> &m = g.members[g.group_of[i]];
        for (auto it = std::upper_bound(m.begin(), m.end(), (uint32_t)i); it != m.end(); ++it) {
            RpRead &s = v[*it];
            if (s.Visited) continue;
            if (f.ChrA == s.ChrA && f.ChrB == s.ChrB && f.PosA == s.PosA && f.PosB == s.PosB && f.DA == s.DA && f.DB == s.DB) {
                f.NumberOfIdentical++;
                if (!f.Tags.empty()) {
                    f.Tags.insert(f.Tags.end(), s.Tags.begin(), s.Tags.end());
                    s.Tags.clear();
                }
                s.Visited = true;
            }
        }
        f.Report = f.NumberOfIdentical >= Cutoff;
    }
}

}  // namespace rp_detail

// The second half of BDData::UpdateBD (src/bddata.cpp:735-806), with -I: the interchromosomal pairs of one window (all
// BAMs of the run, in discovery order) -> events and the lines the reference appends to <prefix>_RP after the window's
// same-chromosome lines.  Unlike above, the second coordinate's window is widened too (`shift * 2 < spacer`).
inline std::vector<RpEvent> rp_events_interchr(std::vector<RpRead> &reads, unsigned spacer, std::ostream *rp_out)
{
    using namespace rp_detail;
    std::vector<RpEvent> events;
    if (reads.empty()) return events;
    std::sort(reads.begin(), reads.end(), [](const RpRead &a, const RpRead &b) {   // Compare2RP: descending
        if (a.OriginalPosA > b.OriginalPosA) return true;
        if (a.OriginalPosA == b.OriginalPosA) return a.OriginalPosB > b.OriginalPosB;
        return false;
    });
    initialize_a1b1(reads);
    const PairGroups groups(reads);
    modify_rp_interchr(reads, groups);
    summarize_interchr(reads, groups);
    for (RpRead &r : reads) {
        if (!r.Report) continue;
        const unsigned shift = (unsigned)r.InsertSize;
        unsigned f1 = r.PosA + spacer, f2 = r.PosA1 + spacer, s1 = r.PosB + spacer, s2 = r.PosB1 + spacer;
        if (f1 > f2) std::swap(f1, f2);
        if (r.DA == '+' && f1 > shift) f1 -= shift;
        else if (shift * 2 < spacer) f2 += shift;
        if (s1 > s2) std::swap(s1, s2);
        if (r.DB == '+' && s1 > shift) s1 -= shift;
        else if (shift * 2 < spacer) s2 += shift;
        if (r.ChrNameA.empty() || r.ChrNameB.empty()) continue;
        RpEvent e = { r.ChrNameA, r.ChrNameB, f1, f2, s1, s2 };
        events.push_back(e);
        if (rp_out) {
            std::ostream &o = *rp_out;
            o << r.ChrNameA << "\t" << (f1 > spacer ? f1 - spacer : 1) << "\t" << f2 - spacer << "\t" << r.DA << "\t" << f2 - f1 << "\t"
              << r.ChrNameB << "\t" << (s1 > spacer ? s1 - spacer : 1) << "\t" << s2 - spacer << "\t" << r.DB << "\t0\t"
              << "\tSupport: " << r.NumberOfIdentical;
            std::sort(r.Tags.begin(), r.Tags.end());                               // DisplayBDSupportPerSample
            for (size_t i = 0; i < r.Tags.size();) {
                size_t j = i;
                while (j < r.Tags.size() && r.Tags[j] == r.Tags[i]) j++;
                o << "\t" << r.Tags[i] << " " << (j - i);
                i = j;
            }
            o << std::endl;
        }
    }
    reads.clear();
    return events;
}

}  // namespace pgh
#endif
