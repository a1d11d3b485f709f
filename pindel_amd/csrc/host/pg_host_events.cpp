// pg_host_events.cpp -- the opt-in events path of Caller::process_window: the window's event tables are built
// from the reads' candidate lists (pg_host_events.hpp) or taken from the caller (built on the device), and deletions, short
// insertions and tandem duplications are written from them -- `good` from the member lists with the pairs' fields applied, the
// reporters' output_* functions for the events flagged PG_EV_REPORT, in table order.  DI and the inversions take their boxes from
// the per-read records and keep their own reporters (their exchange sorts are strict: no stable sort reproduces their tie order)
// -- or, with Settings::use_sv_events, are written from their SV tables (pg_host_sv_events.hpp) in the same places.
// The reports must be the bytes of the existing path: that is what pins pg_host_events.hpp to the reference's gold reports.
#include <cctype>
#include <unordered_map>

#include "pg_depth.hpp"
#include "pg_host_events.hpp"
#include "pg_host_priv.hpp"
#include "pg_host_report.hpp"
#include "pg_host_sv_events.hpp"

namespace pgh {

using namespace detail;

EventPathStats &event_path_stats()
{
    static EventPathStats s;
    return s;
}

// Supplied SV tables (over all reads of the run, beside the supplied event tables `sup` of the same window) to the window's own
// read indices.  false: they do not fit this window's reads and records -- a member the window does not hold or that its record
// did not box for the table's kind, a member list of another size than the records give, an event outside its member list.
static bool sv_tables_from_supplied(const SuppliedSvEvents &e, const SuppliedEvents &sup, const std::vector<SplitRead> &reads,
                                    const std::vector<pg_event_read> &recs, SvEventTables &out)
{
    std::unordered_map<uint32_t, uint32_t> local;
    local.reserve(reads.size() * 2);
    for (size_t k = 0; k < reads.size(); k++) local[reads[k].VarIndex] = (uint32_t)k;
    out = SvEventTables();
    size_t m0 = 0, e0 = 0;
    for (int t = 0; t < PG_SV_EVENT_TABLES; t++) {
        const int kind = sv_event_kind_of(t);
        size_t boxed = 0;
        for (const pg_event_read &r : recs) boxed += (r.flags & PG_EVR_BOXED) && r.kind == kind;
        const uint64_t nm = e.sizes.members[t], ne = e.sizes.events[t];
        if (kind == PG_SV_DI ? nm > boxed : nm != boxed) return false;
        std::vector<char> taken(reads.size(), 0);
        for (uint64_t k = 0; k < nm; k++) {
            const uint32_t word = e.members[m0 + k], idx = word & ~PG_SVEV_MEMBER_DUP;
            if (idx >= sup.n_reads || (kind == PG_SV_DI && (word & PG_SVEV_MEMBER_DUP))) return false;
            auto it = local.find(idx);
            if (it == local.end()) return false;
            const pg_event_read &r = recs[it->second];
            if (!(r.flags & PG_EVR_BOXED) || r.kind != kind || taken[it->second]) return false;
            taken[it->second] = 1;
            out.members[t].push_back(it->second | (word & PG_SVEV_MEMBER_DUP));
        }
        out.events[t].assign(e.events + e0, e.events + e0 + ne);
        uint64_t next = 0;
        for (const pg_event &ev : out.events[t]) {
            if (ev.n_reads == 0 || ev.first < next || (uint64_t)ev.first + ev.n_reads > nm || ev.kind != kind) return false;
            next = (uint64_t)ev.first + ev.n_reads;
        }
        out.dropped_runs[t] = e.sizes.dropped_runs[t];
        m0 += nm;
        e0 += ne;
    }
    return true;
}

// one table written in table order: the order of the boxes, and of the events within each
void Caller::write_event_table(Ctx &c, int t, const std::vector<pg_event> &events, const MakeGood &make_good)
{
    const int kind = event_kind_of(t);
    bool any = false;
    for (const pg_event &ev : events) any = any || (ev.flags & PG_EV_REPORT);
    if (!any) return;
    std::vector<SplitRead> good;
    make_good(good);
    for_boxes(1, [&](unsigned) {
        for (const pg_event &ev : events) {
            if (!(ev.flags & PG_EV_REPORT)) continue;
            const unsigned s = ev.first, e = ev.first + ev.n_reads - 1;
            if (kind == 0) output_deletion(c, good, s, e, ev.real_start, ev.real_end);
            else if (kind == 1) output_si(c, good, s, e, ev.real_start, ev.real_end);
            else {
                // IsGoodTD's -N test (sort_output_td), with GoodIndels[0] = the first unique read of the event's box
                if (S.germline_filter() && ev.real_end - ev.real_start >= (unsigned)(good[ev.box_head].getReadLength() * 2)) {
                    std::set<std::string> tags;
                    for (unsigned i = s; i <= e; i++) tags.insert(good[i].Tag);
                    if (!S.germline->good_td(c.chrom->name, (int64_t)c.chrom->seq.size() - 2 * (int64_t)S.spacer, ev.real_start, ev.real_end, tags))
                        continue;
                }
                output_td(c, good, s, e, ev.real_start, ev.real_end);
            }
        }
    });
}

// one SV table written: the reporters' output_* for the events flagged PG_EV_REPORT, the inversions' runs harmonised first
void Caller::write_sv_event_table(Ctx &c, int t, const std::vector<pg_event> &events, const MakeGood &make_good)
{
    const int kind = sv_event_kind_of(t);
    bool any = false;
    for (const pg_event &ev : events) any = any || (ev.flags & PG_EV_REPORT);
    if (!any) return;
    std::vector<SplitRead> good;
    make_good(good);
    for_boxes(1, [&](unsigned) {
        for (const pg_event &ev : events) {
            if (!(ev.flags & PG_EV_REPORT)) continue;
            const unsigned s = ev.first, e = ev.first + ev.n_reads - 1;
            if (kind == PG_SV_DI) {
                if (ev.flags & PG_EV_SHORT_INV) output_short_inv(c, good, s, e);
                else output_di(c, good, s, e);
                continue;
            }
            // the run harmonised from the event's IndelSize, as sort_output_inv's harmonise() leaves its members
            for (unsigned i = s; i <= e; i++) {
                SplitRead &r = good[i];
                const unsigned mx = ev.indel_size;
                const short diff = (short)((mx - r.IndelSize) / 2);
                r.IndelSize = mx;
                r.BPLeft = r.BPLeft - diff;
                r.BPRight = r.BPRight + diff;
                if (r.MatchedD == '+') {
                    if (r.BP > diff) r.BP = (short)(r.BP - diff);
                } else {
                    if (r.BP + diff < r.getReadLengthMinus()) r.BP = (short)(r.BP + diff);
                }
            }
            // IsGoodINV's -N test (sort_output_inv)
            if (S.germline_filter() && ev.real_end - ev.real_start >= (unsigned)good[s].getReadLength() * 2 &&
                !(S.repair(REPAIR_INV_PAIRS) && inv_pairs_good(inv_pairs_, ev.n_reads, ev.real_start, ev.real_end)))
                continue;
            output_inv(c, good, s, e, ev.real_start, ev.real_end);
        }
    });
}

// What the pipeline and process_window take from the points of every read, from its summary instead
void Caller::apply_summaries(std::vector<SplitRead> &reads, const pg_report_summary *summaries, bool read_length_follows)
{
    for (size_t k = 0; k < reads.size(); k++) {
        SplitRead &r = reads[k];
        const pg_report_summary &s = summaries[k];
        for (uint8_t f = 0; f < s.rc_flag && f < 2; f++) {          // setUnmatchedSeq(ReverseComplement()), once or twice
            r.UnmatchedSeq = reverse_complement(r.UnmatchedSeq);
            while (!r.UnmatchedSeq.empty() && !std::isalnum((unsigned char)r.UnmatchedSeq.back())) r.UnmatchedSeq.pop_back();
        }
        if (read_length_follows) r.ReadLength = (short)r.UnmatchedSeq.size();
        if (s.flags & PG_RS_CLOSE) {
            // note_close_mapped, from the summary's UP_Close.back()
            if (g_reportLength < r.getReadLength()) g_reportLength = r.getReadLength();
            r.Used = false;
            r.UniqueRead = true;
            if (r.MatchedD == '+') r.LeftMostPos = (int)(s.close_abs + 1 - s.close_len);
            else r.LeftMostPos = (int)(s.close_abs + s.close_len - r.getReadLength());
            r.SampleName2Number.insert(std::make_pair(r.Tag, 1u));
            g_sampleNames.insert(r.Tag);
        }
        if (s.flags & PG_RS_FAR) {
            // UpdateFarFragName, from the summary's UP_Far[0]
            const int fc = s.far_chr;
            r.FarFragName = (genome && fc >= 0 && fc < (int)genome->size()) ? (*genome)[fc].name : r.FragName;
            r.MatchedFarD = (s.flags & PG_RS_FAR_ANTISENSE) ? '-' : '+';
            r.CloseVsFar = (s.flags & PG_RS_CLOSE_LEFT) ? -1 : (s.flags & PG_RS_CLOSE_RIGHT) ? 1 : 0;
        }
    }
}

void Caller::process_window_from_tables(const Chromosome &chrom, std::vector<SplitRead> &reads, unsigned win_start, unsigned win_end,
                                        unsigned region_start, unsigned region_end, const pg_event_read *recs, const pg_event_sizes &sizes,
                                        const pg_event *events, const pg_sv_event_sizes &sv_sizes, const pg_event *sv_events,
                                        const pg_report_read *records, const pg_report_summary *summaries, bool summaries_applied)
{
    Ctx c;                                                    // (process_window's frame)
    c.chrom = &chrom;
    c.reads = &reads;
    BoxSize = (unsigned)(chrom.seq.size() / 30000);
    if (BoxSize == 0) BoxSize = 1;
    c.NumBoxes = (unsigned)(chrom.seq.size() * 2 / BoxSize) + 1;
    c.win_start = win_start;
    c.win_end = win_end;
    c.region_start = region_start;
    c.region_end = region_end;
    g_RegionStart = win_start;
    g_RegionEnd = win_end;
    if (mask_chr_ != &chrom) {
        chr_marks_.clear();
        mask_chr_ = &chrom;
    }
    uint64_t n_members[PG_EVENT_TABLES + PG_SV_EVENT_TABLES];
    std::vector<pg_event> ev[PG_EVENT_TABLES], sv[PG_SV_EVENT_TABLES];
    size_t e0 = 0;
    for (int t = 0; t < PG_EVENT_TABLES; t++) {
        n_members[t] = sizes.members[t];
        ev[t].assign(events + e0, events + e0 + sizes.events[t]);
        e0 += (size_t)sizes.events[t];
    }
    e0 = 0;
    for (int t = 0; t < PG_SV_EVENT_TABLES; t++) {
        n_members[PG_EVENT_TABLES + t] = sv_sizes.members[t];
        sv[t].assign(sv_events + e0, sv_events + e0 + sv_sizes.events[t]);
        e0 += (size_t)sv_sizes.events[t];
    }
    process_window_tables(c, recs, n_members, ev, sv, records, summaries, summaries_applied);
    flush_reports();
}

// The tables path.  Nothing here reads a point, a list or a pair field of the window's reads: they have none.
void Caller::process_window_tables(Ctx &c, const pg_event_read *recs, const uint64_t *n_members, const std::vector<pg_event> *events,
                                   const std::vector<pg_event> *sv_events, const pg_report_read *records, const pg_report_summary *summaries,
                                   bool summaries_applied)
{
    std::vector<SplitRead> &reads = *c.reads;
    const size_t n = reads.size();
    if (!summaries_applied) apply_summaries(reads, summaries, false);
    for (size_t k = 0; k < n; k++)
        if (recs[k].flags & (PG_EVR_BOXED | PG_EVR_USED)) reads[k].Used = true;
    size_t first[PG_EVENT_TABLES + PG_SV_EVENT_TABLES + 1];
    first[0] = 0;
    for (int t = 0; t < PG_EVENT_TABLES + PG_SV_EVENT_TABLES; t++) first[t + 1] = first[t] + (size_t)n_members[t];
    // `good` of a table: the member's read with the record applied
    auto good_of = [&](int table, std::vector<SplitRead> &good) {
        const int kind = table < PG_EVENT_TABLES ? event_kind_of(table) : sv_event_kind_of(table - PG_EVENT_TABLES);
        // the reporters clear UniqueRead on the duplicates of an inversion box that reaches -M: the box from the pair's own BPLeft
        std::vector<unsigned> box_size;
        if (table > PG_EVENT_TABLES) {
            box_size.assign(c.NumBoxes, 0);
            for (size_t m = first[table]; m < first[table + 1]; m++) {
                const unsigned box = (unsigned)((int)records[m].cand.bp_left / (int)BoxSize);
                if (box < c.NumBoxes) box_size[box]++;
            }
        }
        good.clear();
        good.reserve(first[table + 1] - first[table]);
        VariantPair p;
        for (size_t m = first[table]; m < first[table + 1]; m++) {
            const pg_report_read &rec = records[m];
            good.push_back(reads[rec.read]);
            SplitRead &g = good.back();
            p.c = rec.cand;
            if (kind < 2) {
                p.nt = kind == 1 ? variant_nt_str(g, rec.bp0, rec.cand.indel_size, rec.cand.nt_rot) : std::string();
                apply_variant_pair(g, p);
            } else {
                if (kind == PG_SV_TD) {
                    // searchTandemDuplications leaves NT_str alone: it is DI's where DI listed a pair, and empty otherwise
                    g.NT_str.clear();
                    if (rec.flags & PG_RR_DI) g.NT_str = sv_nt_str(g, PG_SV_DI, rec.di_bp, rec.di_nt_rot, 0);
                }
                p.nt = sv_nt_str(g, kind, rec.cand.bp, rec.cand.nt_rot, rec.cand.flags);
                apply_sv_pair(g, kind, p);
            }
            g.NT_size = rec.nt_size;
            g.Used = true;
            if (rec.flags & PG_RR_DUP) {
                const unsigned box = (unsigned)((int)rec.cand.bp_left / (int)BoxSize);
                if (box < c.NumBoxes && box_size[box] >= S.NumRead2ReportCutOff) g.UniqueRead = false;
            }
        }
    };
    auto write_table = [&](int t) { write_event_table(c, t, events[t], [&](std::vector<SplitRead> &good) { good_of(t, good); }); };
    auto write_sv_table = [&](int t) {
        write_sv_event_table(c, t, sv_events[t], [&](std::vector<SplitRead> &good) { good_of(PG_EVENT_TABLES + t, good); });
    };
    write_table(0);
    write_sv_table(0);
    if (S.Analyze_TD) {
        write_table(2);
        write_table(3);
    }
    if (S.Analyze_INV) {
        write_sv_table(1);
        write_sv_table(2);
    }
    write_table(1);
    event_path_stats().report_windows++;
    event_path_stats().report_records += first[PG_EVENT_TABLES + PG_SV_EVENT_TABLES];
}

bool Caller::process_window_events(Ctx &c)
{
    std::vector<SplitRead> &reads = *c.reads;
    const std::string &ref = c.chrom->seq;
    const size_t n = reads.size();
    // the lists of both device classifiers for every read, and a -v the inversion lists are consulted with
    if (!sv_list_usable(S)) return false;
    for (const SplitRead &r : reads)
        if (!r.VarCands || !r.SvCands) return false;
    pg_event_window w;
    w.chr_id = 0;
    w.win_end = c.win_end;
    w.region_start = c.region_start;
    w.region_end = c.region_end;
    w.min_support = S.NumRead2ReportCutOff;
    w.balance_cutoff = S.BalanceCutoff;
    w.analyze_td = S.Analyze_TD;
    w.analyze_inv = S.Analyze_INV;
    if (w.region_start > w.region_end) return false;

    EventTables tabs;
    const SuppliedEvents *sup = nullptr;
    for (const SuppliedEvents &e : S.supplied_events)
        if (genome && e.chr >= 0 && e.chr < (int)genome->size() && &(*genome)[e.chr] == c.chrom && e.win_start == c.win_start && e.win_end == c.win_end)
            sup = &e;
    bool from_supplied = false;
    if (sup) {
        // the supplied tables index the reads of the whole run: to the window's own indices.  Tables that touch a read the window
        // does not hold (the device cascade sees every read of the chromosome) are not this window's: the host builds its own.
        std::unordered_map<uint32_t, uint32_t> local;
        local.reserve(n * 2);
        for (size_t k = 0; k < n; k++) local[reads[k].VarIndex] = (uint32_t)k;
        bool ok = true;
        for (uint32_t i = 0; i < sup->n_reads && ok; i++)
            if (sup->reads[i].flags) ok = local.count(i) != 0;
        tabs.reads.assign(n, pg_event_read());
        for (size_t k = 0; k < n && ok; k++) {
            ok = reads[k].VarIndex < sup->n_reads;
            if (ok) tabs.reads[k] = sup->reads[reads[k].VarIndex];
        }
        size_t m0 = 0, e0 = 0;
        for (int t = 0; t < PG_EVENT_TABLES && ok; t++) {
            for (uint64_t k = 0; k < sup->sizes.members[t] && ok; k++) {
                auto it = local.find(sup->members[m0 + k]);
                ok = it != local.end();
                if (ok) tabs.members[t].push_back(it->second);
            }
            tabs.events[t].assign(sup->events + e0, sup->events + e0 + sup->sizes.events[t]);
            for (const pg_event &ev : tabs.events[t])
                ok = ok && (uint64_t)ev.first + ev.n_reads <= sup->sizes.members[t] && ev.box_head <= ev.first && ev.n_reads > 0;
            m0 += sup->sizes.members[t];
            e0 += sup->sizes.events[t];
        }
        tabs.unresolved = sup->sizes.unresolved;
        from_supplied = ok;
    }
    if (!from_supplied) {
        std::vector<EventReadIn> in(n);
        std::unordered_map<std::string, uint32_t> names;
        names.reserve(n * 2);
        for (size_t k = 0; k < n; k++) {
            const SplitRead &r = reads[k];
            EventReadIn &e = in[k];
            e.in_window = true;
            e.plus = r.MatchedD == '+';
            e.insert_size = r.InsertSize;
            e.read_length = r.getReadLength();
            e.name_id = names.emplace(r.Name, (uint32_t)names.size()).first->second;
            e.var = r.VarCands;
            e.var_counts = r.VarCounts;
            e.sv = r.SvCands;
            e.sv_counts = r.SvCounts;
        }
        tabs = EventTables();
        events_from_lists(ref, S.spacer, w, in, [&](uint32_t k, const pg_variant_cand &cand) {
            VariantPair p;
            if (!variant_pair_from_cand(reads[k], 1, cand, p)) return std::string();
            return p.nt;
        }, tabs);
    }
    // A read whose list ran out goes to the pair search on the host; the tables do not replay that: the whole window takes the
    // existing path.  So does a window whose records do not fit its reads' lists.
    if (tabs.unresolved) return false;
    for (size_t k = 0; k < n; k++) {
        const pg_event_read &rec = tabs.reads[k];
        if (!(rec.flags & (PG_EVR_BOXED | PG_EVR_USED))) continue;
        const pg_variant_cand *list;
        uint8_t count;
        unsigned cap;
        EventReadIn e;
        e.var = reads[k].VarCands;
        e.var_counts = reads[k].VarCounts;
        e.sv = reads[k].SvCands;
        e.sv_counts = reads[k].SvCounts;
        if (rec.kind > PG_SV_INV_NT) return false;
        event_list(e, rec.kind, list, count, cap);
        if (rec.slot >= std::min<unsigned>(count & ~PG_VARIANT_MORE, cap)) return false;
    }
    if (from_supplied) event_path_stats().supplied_windows++;

    auto cand_of = [&](size_t k) -> const pg_variant_cand & {
        const pg_event_read &rec = tabs.reads[k];
        return rec.kind < 2 ? reads[k].VarCands[rec.kind * PG_VARIANT_CANDS + rec.slot]
                            : reads[k].SvCands[sv_slot_base()[rec.kind - PG_SV_DI] + rec.slot];
    };
    for (size_t k = 0; k < n; k++)
        if (tabs.reads[k].flags & (PG_EVR_BOXED | PG_EVR_USED)) reads[k].Used = true;

    // `good` of a table: the members with the pair's fields applied, the NT_size the cascade carried and the NT_str that goes with it
    auto good_of = [&](int t, std::vector<SplitRead> &good) {
        const int kind = event_kind_of(t);
        good.clear();
        good.reserve(tabs.members[t].size());
        VariantPair p;
        for (uint32_t k : tabs.members[t]) {
            good.push_back(reads[k]);
            SplitRead &g = good.back();
            const pg_variant_cand &cand = cand_of(k);
            if (kind < 2) {
                variant_pair_from_cand(reads[k], kind, cand, p);
                apply_variant_pair(g, p);
            } else {
                if (kind == PG_SV_TD) {
                    // searchTandemDuplications leaves NT_str alone: it is DI's where DI listed a pair (applied, whatever the window
                    // made of it), and empty otherwise (kind 0 assigns an empty one, a fresh read has none)
                    g.NT_str.clear();
                    if ((reads[k].SvCounts[0] & ~PG_VARIANT_MORE) >= 1 && sv_pair_from_cand(reads[k], PG_SV_DI, reads[k].SvCands[0], p)) g.NT_str = p.nt;
                }
                sv_pair_from_cand(reads[k], kind, cand, p);
                apply_sv_pair(g, kind, p);
            }
            g.NT_size = tabs.reads[k].nt_size;
            g.Used = true;
        }
    };
    auto write_table = [&](int t) { write_event_table(c, t, tabs.events[t], [&](std::vector<SplitRead> &good) { good_of(t, good); }); };
    // the boxes of a kind that keeps its own reporter, from the per-read records: ascending read index, as the classifier pushes
    auto boxes_of = [&](int kind, std::vector<std::vector<unsigned>> &boxes) {
        boxes.assign(c.NumBoxes, std::vector<unsigned>());
        VariantPair p;
        for (size_t k = 0; k < n; k++) {
            const pg_event_read &rec = tabs.reads[k];
            if (!(rec.flags & PG_EVR_BOXED) || rec.kind != kind) continue;
            const pg_variant_cand &cand = cand_of(k);
            sv_pair_from_cand(reads[k], kind, cand, p);
            apply_sv_pair(reads[k], kind, p);
            const unsigned box = (unsigned)((int)cand.bp_left / (int)BoxSize);
            if (box < c.NumBoxes) boxes[box].push_back((unsigned)k);
        }
    };
    std::vector<std::vector<unsigned>> boxes;
    // ---- the sv_events path: DI and the inversions from their SV tables, in the places of the two reporters
    SvEventTables svt;
    if (S.use_sv_events) {
        bool sv_supplied = false;
        if (from_supplied)
            for (const SuppliedSvEvents &e : S.supplied_sv_events)
                if (e.chr == sup->chr && e.win_start == c.win_start && e.win_end == c.win_end && sv_tables_from_supplied(e, *sup, reads, tabs.reads, svt))
                    sv_supplied = true;
        if (!sv_supplied) {
            // supplied tables that do not fit (or none): the host statement over the window's own reads
            std::vector<SvEventReadIn> in(n);
            for (size_t k = 0; k < n; k++) {
                in[k].plus = reads[k].MatchedD == '+';
                in[k].read_length = reads[k].getReadLength();
                in[k].left_most = reads[k].LeftMostPos;
            }
            svt = SvEventTables();
            sv_events_from_lists(ref, S.spacer, w, in, tabs.reads.data(),
                                 [&](size_t k, int kind, unsigned slot) -> const pg_variant_cand & { return reads[k].SvCands[sv_slot_base()[kind - PG_SV_DI] + slot]; },
                                 [&](uint32_t k, const pg_variant_cand &cand) {
                                     VariantPair p;
                                     sv_pair_from_cand(reads[k], PG_SV_DI, cand, p);
                                     return p.nt;
                                 }, svt);
        }
        event_path_stats().sv_table_windows++;
        if (sv_supplied) event_path_stats().sv_supplied_windows++;
    }
    // ---- the tables path: the records and summaries of the window from its tables, lists and points (the host
    // statement of pg_report.hip); then the reads lose their points, lists and pair fields, and the reports are written from tables,
    // records and summaries alone.  If these are the bytes of the paths above, the writers consult nothing the device does not deliver.
    if (S.use_report_reads && S.use_sv_events) {
        std::vector<ReportReadIn> in(n);
        for (size_t k = 0; k < n; k++) {
            const SplitRead &r = reads[k];
            ReportReadIn &e = in[k];
            e.plus = r.MatchedD == '+';
            e.rc_flag = 0;                                    // (UnmatchedSeq is the post-state already: nothing left to apply)
            e.close = r.UP_Close.data();
            e.n_close = r.UP_Close.size();
            e.far = r.UP_Far.data();
            e.n_far = r.UP_Far.size();
            e.var = r.VarCands;
            e.sv = r.SvCands;
            e.sv_counts = r.SvCounts;
        }
        std::vector<pg_report_read> records;
        std::vector<pg_report_summary> summaries;
        report_reads_from_lists(in, tabs.reads.data(), tabs.members, svt.members, records, summaries);
        // -s and -l on this route: _CloseEndMapped from the summaries, the long-insertion tables from the host
        // statement while the reads still have their points; sort_output_li then finds them in the frame
        if (S.report_close_mapped) report_close_mapped_summaries(reads, summaries.data());
        if (S.Analyze_LI) {
            unsigned lo, hi;
            li_window(*c.chrom, c.win_start, c.win_end, lo, hi);
            std::vector<LiReadIn> li_in(n);
            c.li_close_len.assign(n, 0);
            for (size_t k = 0; k < n; k++) {
                const SplitRead &r = reads[k];
                LiReadIn &e = li_in[k];
                e.has_close = !r.UP_Close.empty();
                e.has_far = !r.UP_Far.empty();
                e.strand = r.MatchedD;
                e.read_length = r.getReadLength();
                if (e.has_close) {
                    e.close_abs = r.UP_Close.back().AbsLoc;
                    e.close_len = c.li_close_len[k] = r.UP_Close.back().LengthStr;
                }
            }
            li_tables_from_reads(li_in, tabs.reads.data(), lo, hi, c.li);
            c.li_ready = true;
        }
        // -I on this route: the junction tables from the host statement while the reads still have their points;
        // process_window then writes _INT from them and the summaries, where it reports _INT
        if (S.report_interchromosomal) {
            if (!int_chr_rank_ready_) {                       // (the ranks depend on the reference alone: once per run)
                std::vector<std::string> chr_names;
                if (genome)
                    for (const Chromosome &g : *genome) chr_names.push_back(g.name);
                int_chr_rank_ = int_chr_ranks(chr_names);
                int_chr_rank_ready_ = true;
            }
            const std::vector<int32_t> &rank = int_chr_rank_;
            std::vector<IntReadIn> int_in(n);
            for (size_t k = 0; k < n; k++) {
                const SplitRead &r = reads[k];
                IntReadIn &e = int_in[k];
                e.chr = r.chr_id;
                e.strand = r.MatchedD;
                e.read_length = r.getReadLength();
                e.close = r.UP_Close.data();
                e.n_close = r.UP_Close.size();
                e.far = r.UP_Far.data();
                e.n_far = r.UP_Far.size();
                if (e.n_far) {
                    e.far_chr = r.UP_Far[0].chr;
                    e.far_minus = r.UP_Far[0].Strand == '-';
                }
            }
            int_tables_from_reads(int_in, rank.data(), (uint32_t)rank.size(), c.int_tables);
            c.int_summaries = summaries;
            c.int_ready = true;
        }
        for (SplitRead &r : reads) {
            SplitRead bare;
            bare.Name.swap(r.Name);
            bare.UnmatchedSeq.swap(r.UnmatchedSeq);
            bare.FragName.swap(r.FragName);
            bare.Tag.swap(r.Tag);
            bare.MatchedD = r.MatchedD;
            bare.MatchedRelPos = r.MatchedRelPos;
            bare.MS = r.MS;
            bare.InsertSize = r.InsertSize;
            bare.ReadLength = r.ReadLength;
            bare.MAX_SNP_ERROR = r.MAX_SNP_ERROR;
            bare.chr_id = r.chr_id;
            bare.VarIndex = r.VarIndex;
            r = std::move(bare);
        }
        uint64_t n_members[PG_EVENT_TABLES + PG_SV_EVENT_TABLES];
        for (int t = 0; t < PG_EVENT_TABLES; t++) n_members[t] = tabs.members[t].size();
        for (int t = 0; t < PG_SV_EVENT_TABLES; t++) n_members[PG_EVENT_TABLES + t] = svt.members[t].size();
        process_window_tables(c, tabs.reads.data(), n_members, tabs.events, svt.events, records.data(), summaries.data());
        return true;
    }
    // one SV table written: what sort_output_di / sort_output_inv leave of the kind -- the pairs applied to the window's reads, the
    // duplicates of the boxes that reach -M marked -- and the reporters' output_* for the events flagged PG_EV_REPORT
    auto write_sv_table = [&](int t) {
        const int kind = sv_event_kind_of(t);
        boxes_of(kind, boxes);
        std::vector<char> dup(n, 0);
        if (kind == PG_SV_DI) {
            for (size_t k = 0; k < n; k++) dup[k] = (tabs.reads[k].flags & PG_EVR_BOXED) && tabs.reads[k].kind == kind;
            for (uint32_t m : svt.members[t]) dup[m] = 0;
        } else {
            for (uint32_t m : svt.members[t])
                if (m & PG_SVEV_MEMBER_DUP) dup[m & ~PG_SVEV_MEMBER_DUP] = 1;
        }
        for (const std::vector<unsigned> &box : boxes)
            if (!box.empty() && box.size() >= S.NumRead2ReportCutOff)
                for (unsigned k : box)
                    if (dup[k]) reads[k].UniqueRead = false;
        write_sv_event_table(c, t, svt.events[t], [&](std::vector<SplitRead> &good) {
            good.reserve(svt.members[t].size());
            for (uint32_t m : svt.members[t]) {
                good.push_back(reads[m & ~PG_SVEV_MEMBER_DUP]);              // (the pair is applied, NT_size is the carried one)
                good.back().NT_size = tabs.reads[m & ~PG_SVEV_MEMBER_DUP].nt_size;
            }
        });
    };
    write_table(0);
    if (S.use_sv_events) write_sv_table(0);
    else {
        boxes_of(PG_SV_DI, boxes);
        sort_output_di(c, boxes);
    }
    if (S.Analyze_TD) {
        write_table(2);
        write_table(3);
    }
    if (S.Analyze_INV) {
        if (S.use_sv_events) {
            write_sv_table(1);
            write_sv_table(2);
        } else {
            boxes_of(PG_SV_INV, boxes);
            sort_output_inv(c, boxes, false);
            boxes_of(PG_SV_INV_NT, boxes);
            sort_output_inv(c, boxes, true);
        }
    }
    write_table(1);
    return true;
}

}  // namespace pgh
