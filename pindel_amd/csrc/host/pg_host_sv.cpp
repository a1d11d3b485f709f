// pg_host_sv.cpp -- tandem duplications and inversions: classifiers + reporters.
//   searchTandemDuplications(NT)   src/search_tandem_duplications.cpp:29-222, _nt.cpp:27-131
//   searchInversions(NT)           src/search_inversions.cpp:29-318, _nt.cpp:27-200
//   SortAndOutputTandemDuplications / OutputTDs   src/reporter.cpp:1157-1287, 157-269
//   DoSortAndOutputInversions / OutputInversions  src/output_sorter.cpp:69-257, reporter.cpp:446-628
//   OutputShortInversion                          src/reporter.cpp:1588-1696
#include <algorithm>
#include <fstream>
#include <sstream>

#include "pg_depth.hpp"
#include "pg_host_priv.hpp"

namespace pgh {

using namespace detail;

// Places a classified read into its box (the tail shared by all classifiers).
#define PGH_BOX_READ(r, ri, boxes, check_transgress)                                         \
    do {                                                                                     \
        if ((check_transgress) && transgresses((r), c.win_end)) {                            \
            (r).Used = true;                                                                 \
        } else if ((r).BPLeft + 1 >= c.region_start && (r).BPLeft + 1 <= c.region_end) {     \
            unsigned box_ = (unsigned)((int)(r).BPLeft / (int)BoxSize);                      \
            if (box_ < c.NumBoxes) {                                                         \
                (boxes)[box_].push_back(ri);                                                 \
                (r).Used = true;                                                             \
            }                                                                                \
        }                                                                                    \
    } while (0)

// (LeftMostTD and LeftMostINV, and the body of every classifier for one pair: pg_host_priv.hpp)

void Caller::search_tandem_dup(Ctx &c)
{
    std::vector<SplitRead> &reads = *c.reads;
    const std::string &ref = c.chrom->seq;
    std::vector<std::vector<unsigned>> boxes(c.NumBoxes);
    std::mutex stats_mu;
    classify_reads(reads.size(), boxes, [&](unsigned lo_, unsigned hi_, BoxSink &sink) {
    ListLog log;
    VariantPair pair;
    for (unsigned ri = lo_; ri < hi_; ri++) {
        SplitRead &r = reads[ri];
        if (r.Used || r.UP_Far.empty() || r.FragName != r.FarFragName) continue;
        const bool plus = r.MatchedD == '+';
        if (!plus && r.MatchedD != '-') continue;
        auto tail = [&](const VariantPair &) { PGH_BOX_READ(r, ri, sink, true); };
        if (r.SvCands) {
            log.visit(r.VarIndex, PG_SV_TD, c.win_end, c.region_start, c.region_end, c.NumBoxes, BoxSize);
            if (!sv_consult_list(r, PG_SV_TD, pair, tail)) continue;
            log.fallbacks++;
        }
        const int nc = (int)r.UP_Close.size(), nf = (int)r.UP_Far.size();
        const FarByLength by_len(r);
        for (short budget = 0; budget <= r.MAX_SNP_ERROR; budget++) {
            for (int k = 0; k < nc; k++) {
                if (r.Used) break;
                const int ci = plus ? k : nc - 1 - k;
                const UniquePoint &cp = r.UP_Close[ci];
                if (cp.Mismatches > budget) continue;
                // only the far point of length ReadLength - LengthStr(close) can pass the tests below
                int fi_first, fi_last;
                by_len.range_desc(r.getReadLength(), cp.LengthStr, nf, fi_first, fi_last);
                int j_first = 0, j_last = nf - 1;
                if (by_len.usable) {
                    if (fi_first < 0) continue;
                    j_first = j_last = plus ? nf - 1 - fi_first : fi_first;
                }
                for (int j = j_first; j <= j_last; j++) {
                    if (r.Used) break;
                    const int fi = plus ? nf - 1 - j : j;
                    const UniquePoint &fp = r.UP_Far[fi];
                    if (fp.Mismatches > budget) continue;
                    if (fp.Mismatches + cp.Mismatches > budget) continue;
                    bool assigned;
                    const bool ok = sv_pair_td(r, ci, fi, ref, S.spacer, pair, &assigned);
                    if (ok || assigned) apply_sv_pair(r, PG_SV_TD, pair);     // (a pair with BPLeft == 0 is assigned, then skipped)
                    if (ok) tail(pair);
                }
            }
        }
    }
    log.flush(stats_mu);
    });
    sort_output_td(c, boxes, false);
}

void Caller::search_tandem_dup_nt(Ctx &c)
{
    std::vector<SplitRead> &reads = *c.reads;
    std::vector<std::vector<unsigned>> boxes(c.NumBoxes);
    const pg_sv_params prm = { S.Seq_Error_Rate, S.Min_Num_Matched_Bases, S.MIN_IndelSize_Inversion };
    std::mutex stats_mu;
    classify_reads(reads.size(), boxes, [&](unsigned lo_, unsigned hi_, BoxSink &sink) {
    ListLog log;
    VariantPair pair;
    for (unsigned ri = lo_; ri < hi_; ri++) {
        SplitRead &r = reads[ri];
        if (r.Used || r.UP_Far.empty() || r.FragName != r.FarFragName) continue;
        auto tail = [&](const VariantPair &) { PGH_BOX_READ(r, ri, sink, true); };
        if (r.SvCands) {
            log.visit(r.VarIndex, PG_SV_TD_NT, c.win_end, c.region_start, c.region_end, c.NumBoxes, BoxSize);
            if (!sv_consult_list(r, PG_SV_TD_NT, pair, tail)) continue;
            log.fallbacks++;
        }
        if (!sv_pair_td_nt(r, prm, S.spacer, pair)) continue;
        apply_sv_pair(r, PG_SV_TD_NT, pair);
        tail(pair);
    }
    log.flush(stats_mu);
    });
    sort_output_td(c, boxes, true);
}

// OutputTDs, src/reporter.cpp:157-269
void Caller::output_td(Ctx &c, std::vector<SplitRead> &g, unsigned s, unsigned e, unsigned, unsigned)
{
    std::ostream &out = report(REP_TD);
    const std::string &ref = c.chrom->seq;
    const SplitRead &f = g[s];
    unsigned n_reads = 0;
    std::string sup = support_columns(g, s, e, f.BPLeft - 1, f.BPRight + 1, n_reads);
    mark(f.BPLeft);                      // reporter.cpp:194-195
    mark(f.BPRight);
    out << HASHES << '\n';
    out << ev_no(EV_TD) << "\tTD " << f.IndelSize << "\tNT " << f.NT_size << " \"" << f.NT_str << "\"\tChrID "
        << f.FragName << "\tBP " << f.BPLeft << "\t" << f.BPRight + 2 << "\tBP_range " << f.BPLeft << "\t"
        << f.BPRight + 2 << sup << '\n';
    const long rl = g_reportLength;
    out << sub(ref, (long)f.BPRight + S.spacer - rl + 1, rl) << std::string(f.NT_size, ' ')
        << cap2low(sub(ref, (long)f.BPLeft + S.spacer, rl)) << '\n';
    for (unsigned i = s; i <= e; i++) {
        const SplitRead &r = g[i];
        short before = (short)(rl - r.BP - 1);
        out << std::string(before > 0 ? before : 0, ' ');
        out << (r.MatchedD == '-' ? r.UnmatchedSeq : reverse_complement(r.UnmatchedSeq)) << '\n';
        out << read_tail(r) << '\n';
    }
}

// SortAndOutputTandemDuplications, src/reporter.cpp:1157-1287
void Caller::sort_output_td(Ctx &c, std::vector<std::vector<unsigned>> &boxes, bool)
{
    std::vector<SplitRead> &reads = *c.reads;
    const std::string &ref = c.chrom->seq;
    struct Ev { unsigned s, e, bl, br, rs, re; };
    for_boxes(c.NumBoxes, [&](unsigned b) {
        std::vector<unsigned> &box = boxes[b];
        if (box.empty() || box.size() < S.NumRead2ReportCutOff) return;
        exchange_sort(reads, box);                       // bubblesortReads
        mark_duplicates(reads, box);                     // markDuplicates
        std::vector<SplitRead> good;
        for (unsigned i : box)
            if (reads[i].UniqueRead) good.push_back(reads[i]);
        if (good.empty()) return;
        std::vector<Ev> evs;
        Ev cur = { 0, 0, good[0].BPLeft, good[0].BPRight, 0, 0 };
        auto close_event = [&]() {
            cur.rs = cur.bl;
            cur.re = cur.br;
            real_start_deletion(ref, S.spacer, cur.rs, cur.re);
            evs.push_back(cur);
        };
        for (unsigned i = 1; i < good.size(); i++) {
            if (good[i].BPLeft == cur.bl && good[i].BPRight == cur.br) cur.e = i;
            else {
                close_event();
                cur.s = cur.e = i;
                cur.bl = good[i].BPLeft;
                cur.br = good[i].BPRight;
            }
        }
        close_event();
        for (const Ev &ev : evs) {
            if (ev.e - ev.s + 1 < S.NumRead2ReportCutOff) continue;
            // IsGoodTD (reporter.cpp:1093-1155); beyond its first two tests it only acts under -N on BAM-derived reads
            if (ev.re < ev.rs || ev.rs == 0) continue;
            if (S.germline_filter() && ev.re - ev.rs >= (unsigned)(good[0].getReadLength() * 2)) {
                // (good[0]: the first read of the box's list, not of the event -- GoodIndels[0], reporter.cpp:1113)
                std::set<std::string> tags;                  // UpdateSampleID: the samples among the event's reads
                for (unsigned i = ev.s; i <= ev.e; i++) tags.insert(good[i].Tag);
                if (!S.germline->good_td(c.chrom->name, (int64_t)c.chrom->seq.size() - 2 * (int64_t)S.spacer, ev.rs, ev.re, tags)) continue;
            }
            if (good[ev.s].IndelSize < S.BalanceCutoff || report_event(good, ev.s, ev.e)) {
                output_td(c, good, ev.s, ev.e, ev.rs, ev.re);
            }
        }
    });
}

// ------------------------------------------------------------------------------ inversions
void Caller::search_inversions(Ctx &c)
{
    std::vector<SplitRead> &reads = *c.reads;
    const std::string &ref = c.chrom->seq;
    std::vector<std::vector<unsigned>> boxes(c.NumBoxes);
    const unsigned MIN = (unsigned)S.MIN_IndelSize_Inversion;
    std::mutex stats_mu;
    classify_reads(reads.size(), boxes, [&](unsigned lo_, unsigned hi_, BoxSink &sink) {
    ListLog log;
    VariantPair pair;
    for (unsigned ri = lo_; ri < hi_; ri++) {
        SplitRead &r = reads[ri];
        if (r.Used || r.UP_Far.empty() || r.FragName != r.FarFragName) continue;
        if (!sv_inv_read_ok(r)) continue;
        const int nc = (int)r.UP_Close.size(), nf = (int)r.UP_Far.size();
        const bool plus = r.MatchedD == '+';
        if (!plus && r.MatchedD != '-') continue;
        auto tail = [&](const VariantPair &) { PGH_BOX_READ(r, ri, sink, plus); };   // the '-' branches skip the bin-border test
        if (r.SvCands && sv_list_usable(S)) {
            log.visit(r.VarIndex, PG_SV_INV, c.win_end, c.region_start, c.region_end, c.NumBoxes, BoxSize);
            if (!sv_consult_list(r, PG_SV_INV, pair, tail)) continue;
            log.fallbacks++;
        }
        // which of the two geometries (search_inversions.cpp:53, 118, 186, 245)
        const int geo = sv_inv_geometry(r, MIN);
        if (geo < 0) continue;
        const bool close_desc = (geo == 0 || geo == 2);   // CloseIndex from the back, FarIndex ascending
        for (short budget = 0; budget <= r.MAX_SNP_ERROR; budget++) {
            for (int k = 0; k < nc; k++) {
                if (r.Used) break;
                const int ci = close_desc ? nc - 1 - k : k;
                const UniquePoint &cp = r.UP_Close[ci];
                if (cp.Mismatches > budget) continue;
                for (int j = 0; j < nf; j++) {
                    if (r.Used) break;
                    const int fi = close_desc ? j : nf - 1 - j;
                    const UniquePoint &fp = r.UP_Far[fi];
                    if (fp.Mismatches > budget) continue;
                    if (fp.Mismatches + cp.Mismatches > budget) continue;
                    if (!sv_pair_inv(r, geo, ci, fi, MIN, ref, S.spacer, pair)) continue;
                    apply_sv_pair(r, PG_SV_INV, pair);
                    tail(pair);
                }
            }
        }
    }
    log.flush(stats_mu);
    });
    sort_output_inv(c, boxes, false);
}

void Caller::search_inversions_nt(Ctx &c)
{
    std::vector<SplitRead> &reads = *c.reads;
    std::vector<std::vector<unsigned>> boxes(c.NumBoxes);
    const pg_sv_params prm = { S.Seq_Error_Rate, S.Min_Num_Matched_Bases, S.MIN_IndelSize_Inversion };
    std::mutex stats_mu;
    classify_reads(reads.size(), boxes, [&](unsigned lo_, unsigned hi_, BoxSink &sink) {
    ListLog log;
    VariantPair pair;
    for (unsigned ri = lo_; ri < hi_; ri++) {
        SplitRead &r = reads[ri];
        if (r.Used || r.UP_Far.empty() || r.FragName != r.FarFragName) continue;
        auto tail = [&](const VariantPair &) { PGH_BOX_READ(r, ri, sink, true); };
        if (r.SvCands && sv_list_usable(S)) {
            log.visit(r.VarIndex, PG_SV_INV_NT, c.win_end, c.region_start, c.region_end, c.NumBoxes, BoxSize);
            if (!sv_consult_list(r, PG_SV_INV_NT, pair, tail)) continue;
            log.fallbacks++;
        }
        if (!sv_inv_nt_read_ok(r, prm)) continue;
        for (int which = 0; which < 2; which++) {          // (both distance tests run, the second also after the first has boxed the read)
            if (!sv_pair_inv_nt(r, prm, which, S.spacer, pair)) continue;
            apply_sv_pair(r, PG_SV_INV_NT, pair);
            tail(pair);
        }
    }
    log.flush(stats_mu);
    });
    sort_output_inv(c, boxes, true);
}

// OutputInversions, src/reporter.cpp:446-628
void Caller::output_inv(Ctx &c, std::vector<SplitRead> &g, unsigned s, unsigned e, unsigned, unsigned)
{
    std::ostream &out = report(REP_INV);
    const std::string &ref = c.chrom->seq;
    const SplitRead &f = g[s];
    short lnt = 0, rnt = 0;
    std::string lstr, rstr;
    for (unsigned i = s; i <= e; i++)
        if (g[i].MatchedD == '+') {
            lnt = (short)g[i].NT_size;
            lstr = g[i].NT_str;
            break;
        }
    for (unsigned i = s; i <= e; i++)
        if (g[i].MatchedD == '-') {
            rnt = (short)g[i].NT_size;
            rstr = g[i].NT_str;
            break;
        }
    unsigned n_reads = 0;
    std::string sup = support_columns(g, s, e, f.BPLeft - 1, f.BPRight + 1, n_reads);
    mark(f.BPLeft);                      // reporter.cpp:517-518
    mark(f.BPRight);
    out << HASHES << '\n';
    out << ev_no(EV_INV) << "\tINV " << f.IndelSize << "\tNT " << lnt << ":" << rnt << " \"" << lstr << "\":\"" << rstr
        << "\"\tChrID " << f.FragName << "\tBP " << f.BPLeft + 1 - 1 << "\t" << f.BPRight + 1 + 1 << "\tBP_range "
        << f.BPLeft + 1 - 1 << "\t" << f.BPRight + 1 + 1 << sup << '\n';
    const long rl = g_reportLength;
    out << sub(ref, (long)f.BPLeft + S.spacer - rl, rl) << std::string(lnt > 0 ? lnt : 0, ' ')
        << cap2low(reverse_complement(sub(ref, (long)f.BPRight + 1 + S.spacer - rl, rl))) << '\n';
    for (unsigned i = s; i <= e; i++) {
        const SplitRead &r = g[i];
        if (r.MatchedD != '+') continue;
        short before = (short)(rl - r.BP - 1);
        out << std::string(before > 0 ? before : 0, ' ');
        if (close_left_of_far(r))
            out << reverse_complement(r.UnmatchedSeq) << std::string(r.BP > 0 ? r.BP : 0, ' ');
        else
            out << r.UnmatchedSeq;
        out << read_tail(r) << '\n';
    }
    out << DASHES << '\n';
    out << cap2low(reverse_complement(sub(ref, (long)f.BPLeft + S.spacer, rl))) << std::string(rnt > 0 ? rnt : 0, ' ')
        << sub(ref, (long)f.BPRight + 1 + S.spacer, rl) << '\n';
    for (unsigned i = s; i <= e; i++) {
        const SplitRead &r = g[i];
        if (r.MatchedD != '-') continue;
        short before = (short)(rl - r.BP - 1);
        out << std::string(before > 0 ? before : 0, ' ');
        if (close_right_of_far(r))
            out << r.UnmatchedSeq << std::string(r.BP > 0 ? r.BP : 0, ' ');
        else
            out << reverse_complement(r.UnmatchedSeq);
        out << read_tail(r) << '\n';
    }
}

// OutputShortInversion, src/reporter.cpp:1588-1696
void Caller::output_short_inv(Ctx &c, std::vector<SplitRead> &g, unsigned s, unsigned e)
{
    std::ostream &out = report(REP_INV);
    const std::string &ref = c.chrom->seq;
    const SplitRead &f = g[s];
    unsigned n_reads = 0;
    std::string sup = support_columns(g, s, e, f.BPLeft, f.BPRight, n_reads);
    mark(f.BPLeft);                      // reporter.cpp:1625-1626
    mark(f.BPRight);
    out << HASHES << '\n';
    out << ev_no(EV_INV) << "\tINV " << f.IndelSize << "\tNT " << f.NT_size << " \"" << f.NT_str << "\"\tChrID "
        << f.FragName << "\tBP " << f.BPLeft + 1 << "\t" << f.BPRight + 1 << "\tBP_range " << f.BPLeft + 1 << "\t"
        << f.BPRight + 1 << sup << '\n';
    const long rl = g_reportLength;
    out << sub(ref, (long)f.Left - rl + f.BP + 1, rl)
        << cap2low(reverse_complement(sub(ref, (long)f.Left + f.BP + 1, f.NT_size)))
        << sub(ref, (long)f.Left + f.BP + 1 + f.IndelSize, rl) << '\n';
    for (unsigned i = s; i <= e; i++) {
        const SplitRead &r = g[i];
        short before = (short)(rl - r.BP - 1);
        out << std::string(before > 0 ? before : 0, ' ');
        out << (r.MatchedD == '-' ? r.UnmatchedSeq : reverse_complement(r.UnmatchedSeq)) << "\t";
        out << read_tail(r) << '\n';
    }
}

// OutputSorter::DoSortAndOutputInversions, src/output_sorter.cpp:69-257
void Caller::sort_output_inv(Ctx &c, std::vector<std::vector<unsigned>> &boxes, bool nt)
{
    std::vector<SplitRead> &reads = *c.reads;
    struct Ev { unsigned s, e, rs, re; };
    for_boxes(c.NumBoxes, [&](unsigned b) {
        std::vector<unsigned> &box = boxes[b];
        if (box.empty() || box.size() < S.NumRead2ReportCutOff) return;
        const size_t n = box.size();
        for (size_t a = 0; a + 1 < n; a++)
            for (size_t d = a + 1; d < n; d++) {
                const SplitRead &x = reads[box[a]], &y = reads[box[d]];
                bool swap = false;
                const unsigned sx = x.BPLeft + x.BPRight, sy = y.BPLeft + y.BPRight;
                if (sx < sy) continue;
                else if (sx > sy) swap = true;
                else if (x.IndelSize > y.IndelSize) continue;      // larger ones first
                else if (x.IndelSize < y.IndelSize) swap = true;
                else if (x.BPLeft < y.BPLeft) continue;
                else if (x.BPLeft > y.BPLeft) swap = true;
                else {
                    if (x.BPRight < y.BPRight) continue;
                    else if (x.BPRight > y.BPRight) swap = true;
                    else if (nt) {
                        if (x.NT_size < y.NT_size) continue;
                        else if (x.NT_size > y.NT_size) swap = true;
                        else if (x.BP > y.BP) swap = true;
                    } else if (x.BP > y.BP) swap = true;
                }
                if (swap) std::swap(box[a], box[d]);
            }
        for (size_t a = 0; a + 1 < n; a++)
            for (size_t d = a + 1; d < n; d++) {
                const SplitRead &x = reads[box[a]];
                SplitRead &y = reads[box[d]];
                if ((x.LeftMostPos == y.LeftMostPos ||
                     x.LeftMostPos + x.getReadLength() == y.LeftMostPos + y.getReadLength()) &&
                    x.MatchedD == y.MatchedD)
                    y.UniqueRead = false;
            }
        std::vector<SplitRead> good;                 // ALL reads of the box, unique or not
        for (unsigned i : box) good.push_back(reads[i]);
        if (good.empty()) return;
        std::vector<Ev> evs;
        unsigned cs = 0, ce = 0, cbl = good[0].BPLeft, cbr = good[0].BPRight;
        bool whether = true;                          // never re-armed inside a box (output_sorter.cpp:150)
        auto harmonise = [&]() {
            unsigned mx = 0;
            for (unsigned i = cs; i <= ce; i++) mx = std::max(mx, good[i].IndelSize);
            for (unsigned i = cs; i <= ce; i++) {
                SplitRead &r = good[i];
                if (r.IndelSize / (float)mx < 0.95 || mx + 30 > (unsigned)(r.getReadLength() + r.IndelSize)) {
                    whether = false;
                    break;
                }
                short diff = (short)((mx - r.IndelSize) / 2);
                r.IndelSize = mx;
                r.BPLeft = r.BPLeft - diff;
                r.BPRight = r.BPRight + diff;
                if (r.MatchedD == '+') {
                    if (r.BP > diff) r.BP = (short)(r.BP - diff);
                } else {
                    if (r.BP + diff < r.getReadLengthMinus()) r.BP = (short)(r.BP + diff);
                }
            }
        };
        for (unsigned i = 1; i < good.size(); i++) {
            if (good[i].BPLeft + good[i].BPRight == cbl + cbr) {
                ce = i;
            } else {
                harmonise();
                if (whether) evs.push_back({ cs, ce, good[cs].BPLeft, good[cs].BPRight });
                cs = ce = i;
                cbl = good[i].BPLeft;
                cbr = good[i].BPRight;
            }
        }
        harmonise();
        if (whether) evs.push_back({ cs, ce, cbl, cbr });
        for (const Ev &ev : evs) {
            if (ev.e - ev.s + 1 < S.NumRead2ReportCutOff) continue;
            if (ev.re < ev.rs || ev.rs == 0) continue;          // IsGoodINV (output_sorter.cpp:264-369)
            // ... under -N on BAM-derived reads: an event of two read lengths or more needs >= 5 supporting pairs on each
            // side among Reads_RP_Discovery -- a list UpdateBD has emptied by then (bddata.cpp:733; never filled with
            // -R false), so none is ever counted and the event is dropped.  --repair inv-pairs counts in the list as
            // it stood before it was emptied.
            if (S.germline_filter() && ev.re - ev.rs >= (unsigned)good[ev.s].getReadLength() * 2 &&
                !(S.repair(REPAIR_INV_PAIRS) && inv_pairs_good(inv_pairs_, ev.e - ev.s + 1, ev.rs, ev.re)))
                continue;
            if (good[ev.s].IndelSize < S.BalanceCutoff || report_event(good, ev.s, ev.e))
                output_inv(c, good, ev.s, ev.e, ev.rs, ev.re);
        }
    });
}

// The arithmetic is the reference's: unsigned 32-bit throughout (RP_READ's positions and Experimental_InsertSize are
// unsigned, ReadLength is a short that the additions convert).  ChrNameA == ChrNameB holds for every pair of the list
// (build_record_RP_Discovery puts the others into a list of their own).
bool inv_pairs_good(const std::vector<DiscordantPair> &pairs, unsigned support, unsigned RealStart, unsigned RealEnd, unsigned *counts)
{
    unsigned Cutoff = support / 2;
    if (Cutoff < 5) Cutoff = 5;
    unsigned CountLeft = 0, CountRight = 0;
    bool good = false;
    for (const DiscordantPair &p : pairs) {
        if (CountLeft >= Cutoff && CountRight >= Cutoff) {
            good = true;
            break;
        }
        if (p.DA != p.DB) continue;
        const unsigned L = (unsigned)p.ReadLength, I = p.InsertSize;
        // the smaller position first (the reference spells both orders out)
        const unsigned lo = p.PosA < p.PosB ? p.PosA : p.PosB, hi = p.PosA < p.PosB ? p.PosB : p.PosA;
        if (p.DA == '+') {
            if (lo < RealStart + L && hi + L > RealStart && hi < RealEnd + L && lo + I + L > RealStart && hi + I + L > RealEnd) CountLeft++;
        } else {
            if (lo + L > RealStart && lo < RealEnd + L && hi + L > RealEnd && lo < RealStart + I + L && hi < RealEnd + I + L) CountRight++;
        }
    }
    if (CountLeft >= Cutoff && CountRight >= Cutoff) good = true;      // the repair's addition: the last pair counts too
    if (counts) {
        counts[0] = CountLeft;
        counts[1] = CountRight;
    }
    return good;
}

}  // namespace pgh
