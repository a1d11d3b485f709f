// pg_host_sv_events.hpp -- the event tables of DI, INV and INV_NT from the per-read records and the sv lists, on the host
// (DESIGN.md 7n): the plain-loop statement of what pg_sv_events.hip computes on the device, with the same inputs and byte-identical
// outputs (pgh_sv_events_from_lists), and what the sv_events path of Caller::process_window_events writes these three kinds from.
// It calls neither sort_output_di nor sort_output_inv: it is the second statement of their strict exchange sorts (the literal
// O(n^2) loop: the tie order depends on the arrangement a box arrives in), of their duplicate walks and of the inversions' run
// harmonisation with its `whether` that is never re-armed inside a box, pinned to them by the reports that path must reproduce.
#ifndef PG_HOST_SV_EVENTS_HPP
#define PG_HOST_SV_EVENTS_HPP

#include <map>
#include <string>
#include <vector>

#include "pg_host_events.hpp"

namespace pgh {
namespace detail {

// what the three reporters read of one read beside its record and its pair
struct SvEventReadIn {
    bool plus = false;                        // MatchedD == '+'
    short read_length = 0;                    // the post-state's (getReadLength())
    int left_most = 0;                        // LeftMostPos, from UP_Close.back() (Caller::note_close_mapped)
};

struct SvEventTables {
    std::vector<uint32_t> members[PG_SV_EVENT_TABLES];
    std::vector<pg_event> events[PG_SV_EVENT_TABLES];
    uint64_t dropped_runs[PG_SV_EVENT_TABLES] = { 0, 0, 0 };
};

inline int sv_event_kind_of(int table) { return table == 0 ? PG_SV_DI : table == 1 ? PG_SV_INV : PG_SV_INV_NT; }

// one read of a box: the fields the reporters sort, compare and harmonise
struct SvBoxed {
    uint32_t read;
    unsigned BPLeft, BPRight, IndelSize;
    unsigned short NT_size;
    short BP;
    bool dup;
};

// "x > y" of the exchange loops: pg_host.cpp:719-735 for DI, pg_host_sv.cpp:368-389 for the inversions
inline bool sv_strictly_greater(int kind, const SvBoxed &x, const SvBoxed &y)
{
    if (kind == PG_SV_DI) {
        if (x.BPLeft != y.BPLeft) return x.BPLeft > y.BPLeft;
        if (x.BPRight != y.BPRight) return x.BPRight > y.BPRight;
        if (x.NT_size != y.NT_size) return x.NT_size > y.NT_size;
        return x.BP > y.BP;
    }
    const unsigned sx = x.BPLeft + x.BPRight, sy = y.BPLeft + y.BPRight;
    if (sx != sy) return sx > sy;
    if (x.IndelSize != y.IndelSize) return x.IndelSize < y.IndelSize;      // larger ones first
    if (x.BPLeft != y.BPLeft) return x.BPLeft > y.BPLeft;
    if (x.BPRight != y.BPRight) return x.BPRight > y.BPRight;
    if (kind == PG_SV_INV_NT && x.NT_size != y.NT_size) return x.NT_size > y.NT_size;
    return x.BP > y.BP;
}

// ReportEvent (report_event of pg_host_priv.hpp) over reads given by their fields
inline bool sv_report_event(const std::vector<SvBoxed> &g, const std::vector<SvEventReadIn> &in, size_t s, size_t e)
{
    bool lmin = false, lmax = false, rmin = false, rmax = false;
    for (size_t k = s; k < e; k++) {
        const short RL = in[g[k].read].read_length;
        const short bp = g[k].BP;
        const unsigned short nts = g[k].NT_size;
        short rl = (short)(RL - nts);
        short mn = (short)((short)((rl * 0.5) + 0.5) - 1);
        short mx = (short)((short)(rl * (1 - 0.5) - 0.5) - 1);
        if (bp <= mn) lmin = true;
        if (RL - bp - nts <= mn) rmin = true;
        if (bp >= mx) lmax = true;
        if (RL - bp - nts >= mx) rmax = true;
    }
    return lmin && lmax && rmin && rmax;
}

// One member harmonised to its run's largest IndelSize (pg_host_sv.cpp:405-424); false: the test fails, nothing is changed
inline bool sv_harmonise(SvBoxed &r, unsigned mx, bool plus, short read_length)
{
    if (r.IndelSize / (float)mx < 0.95 || mx + 30 > (unsigned)(read_length + r.IndelSize)) return false;
    const short diff = (short)((mx - r.IndelSize) / 2);
    r.IndelSize = mx;
    r.BPLeft = r.BPLeft - diff;
    r.BPRight = r.BPRight + diff;
    if (plus) {
        if (r.BP > diff) r.BP = (short)(r.BP - diff);
    } else {
        if (r.BP + diff < (short)(read_length - 1)) r.BP = (short)(r.BP + diff);
    }
    return true;
}

// recs: the per-read records of the events build.  cand_of(read index, kind, slot): the listed pair (a reference);
// nt_str(read index, record): NT_str of a DI pair.
template <class CandOf, class NtStr>
inline void sv_events_from_lists(const std::string &ref, unsigned spacer, const pg_event_window &w, const std::vector<SvEventReadIn> &in,
                                 const pg_event_read *recs, CandOf cand_of, NtStr nt_str, SvEventTables &out)
{
    const size_t n = in.size();
    unsigned box_size, n_boxes;
    event_boxes(ref.size(), box_size, n_boxes);
    for (int t = 0; t < PG_SV_EVENT_TABLES; t++) {
        const int kind = sv_event_kind_of(t);
        std::vector<uint32_t> &mem = out.members[t];
        std::vector<pg_event> &evs = out.events[t];
        mem.clear();
        evs.clear();
        out.dropped_runs[t] = 0;
        // the boxes in arrival order: ascending read index, as classify_reads pushes
        std::map<unsigned, std::vector<SvBoxed>> boxes;
        for (size_t i = 0; i < n; i++) {
            const pg_event_read &rec = recs[i];
            if (!(rec.flags & PG_EVR_BOXED) || rec.kind != kind || rec.slot >= (kind == PG_SV_INV ? PG_VARIANT_CANDS : 1)) continue;
            const pg_variant_cand &c = cand_of(i, kind, (unsigned)rec.slot);
            boxes[(unsigned)((int)c.bp_left / (int)box_size)].push_back(SvBoxed{ (uint32_t)i, c.bp_left, c.bp_right, c.indel_size, rec.nt_size, c.bp, false });
        }
        for (auto &kv : boxes) {
            std::vector<SvBoxed> &box = kv.second;
            const size_t m = box.size();
            // the strict exchange sort, literally
            for (size_t a = 0; a + 1 < m; a++)
                for (size_t d = a + 1; d < m; d++)
                    if (sv_strictly_greater(kind, box[a], box[d])) std::swap(box[a], box[d]);
            // the duplicate walk, literally: any earlier read of the box, unique or not
            for (size_t a = 0; a + 1 < m; a++)
                for (size_t d = a + 1; d < m; d++) {
                    const SvEventReadIn &x = in[box[a].read], &y = in[box[d].read];
                    if ((kind != PG_SV_DI || x.read_length == y.read_length) &&
                        (x.left_most == y.left_most || x.left_most + x.read_length == y.left_most + y.read_length) && x.plus == y.plus)
                        box[d].dup = true;
                }
            const uint32_t box_head = (uint32_t)mem.size();
            auto open_event = [&](const SvBoxed &f, size_t first, size_t count) {
                pg_event ev = pg_event();
                ev.kind = (uint8_t)kind;
                ev.bp_left = f.BPLeft;
                ev.bp_right = f.BPRight;
                ev.indel_size = f.IndelSize;
                ev.nt_size = f.NT_size;
                ev.first = (uint32_t)first;
                ev.n_reads = (uint32_t)count;
                ev.box_head = box_head;
                return ev;
            };
            if (kind == PG_SV_DI) {
                std::vector<SvBoxed> good;
                for (const SvBoxed &r : box)
                    if (!r.dup) good.push_back(r);
                for (const SvBoxed &g : good) mem.push_back(g.read);
                for (size_t s = 0; s < good.size();) {
                    size_t e = s + 1;
                    while (e < good.size() && good[e].BPLeft == good[s].BPLeft && good[e].IndelSize == good[s].IndelSize &&
                           (short)good[e].NT_size == (short)good[s].NT_size)
                        e++;
                    const SvBoxed &f = good[s];
                    pg_event ev = open_event(f, box_head + s, e - s);
                    ev.real_start = f.BPLeft;
                    ev.real_end = f.BPRight;
                    for (size_t k = s; k < e; k++) ev.n_plus += in[good[k].read].plus;
                    unsigned flags = 0;
                    if (ev.n_reads >= w.min_support) flags |= PG_EV_SUPPORT;
                    if (f.IndelSize < w.balance_cutoff || sv_report_event(good, in, s, e)) flags |= PG_EV_BALANCE;
                    // is_inversion, pg_host.cpp:700
                    if (f.IndelSize == f.NT_size) {
                        const pg_variant_cand &c = cand_of((size_t)f.read, kind, (unsigned)recs[f.read].slot);
                        if (reverse_complement(sub(ref, (long)spacer + 1 + f.BPLeft, f.NT_size)) == nt_str(f.read, c)) flags |= PG_EV_SHORT_INV;
                    }
                    if ((flags & (PG_EV_SUPPORT | PG_EV_BALANCE)) == (PG_EV_SUPPORT | PG_EV_BALANCE)) flags |= PG_EV_REPORT;
                    ev.flags = (uint8_t)flags;
                    evs.push_back(ev);
                    s = e;
                }
                continue;
            }
            // the inversions: ALL reads of the box are members, duplicates flagged in the member word
            for (const SvBoxed &r : box) mem.push_back(r.read | (r.dup ? PG_SVEV_MEMBER_DUP : 0u));
            std::vector<SvBoxed> good(box);
            bool whether = true;                      // never re-armed inside a box
            for (size_t s = 0; s < m;) {
                size_t e = s + 1;
                while (e < m && good[e].BPLeft + good[e].BPRight == good[s].BPLeft + good[s].BPRight) e++;
                const unsigned raw_left = good[s].BPLeft, raw_right = good[s].BPRight;
                unsigned mx = 0;
                for (size_t k = s; k < e; k++) mx = std::max(mx, good[k].IndelSize);
                for (size_t k = s; k < e; k++)
                    if (!sv_harmonise(good[k], mx, in[good[k].read].plus, in[good[k].read].read_length)) {
                        whether = false;
                        break;
                    }
                if (!whether) {
                    out.dropped_runs[t]++;
                    s = e;
                    continue;
                }
                const SvBoxed &f = good[s];
                pg_event ev = open_event(f, box_head + s, e - s);
                // every run but the last of its box carries the harmonised range, the last one the first member's own
                ev.real_start = e < m ? f.BPLeft : raw_left;
                ev.real_end = e < m ? f.BPRight : raw_right;
                for (size_t k = s; k < e; k++) ev.n_plus += in[good[k].read].plus;
                unsigned flags = 0;
                if (ev.n_reads >= w.min_support) flags |= PG_EV_SUPPORT;
                if (!(ev.real_end < ev.real_start || ev.real_start == 0)) flags |= PG_EV_RANGE;
                if (f.IndelSize < w.balance_cutoff || sv_report_event(good, in, s, e)) flags |= PG_EV_BALANCE;
                if (flags == (PG_EV_SUPPORT | PG_EV_RANGE | PG_EV_BALANCE)) flags |= PG_EV_REPORT;
                ev.flags = (uint8_t)flags;
                evs.push_back(ev);
                s = e;
            }
        }
    }
}

}  // namespace detail
}  // namespace pgh
#endif
