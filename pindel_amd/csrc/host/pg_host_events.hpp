// pg_host_events.hpp -- event tables from candidate lists, on the host: the plain-loop statement of what
// pg_events.hip computes on the device, with the same inputs and byte-identical outputs (pgh_events_from_lists), and what
// Caller::process_window builds its opt-in "events" path from.  It calls none of the sort_output_* reporters: it is the second
// statement of their sorting, duplicate marking and grouping, pinned to them by the reports that path must reproduce.
#ifndef PG_HOST_EVENTS_HPP
#define PG_HOST_EVENTS_HPP

#include <algorithm>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "pg_host_priv.hpp"

namespace pgh {
namespace detail {

// what the cascade reads of one read
struct EventReadIn {
    bool in_window = false;                   // chr_id == the window's
    bool plus = false;                        // MatchedD == '+'
    short insert_size = 0;
    short read_length = 0;                    // the post-state's (getReadLength())
    uint32_t name_id = 0;                     // equal names <-> equal ids
    const pg_variant_cand *var = nullptr;     // 2 x PG_VARIANT_CANDS records, or null
    const uint8_t *var_counts = nullptr;      // 2
    const pg_variant_cand *sv = nullptr;      // PG_SV_SLOTS records, or null
    const uint8_t *sv_counts = nullptr;       // PG_SV_KINDS
};

struct EventTables {
    std::vector<pg_event_read> reads;
    std::vector<uint32_t> members[PG_EVENT_TABLES];
    std::vector<pg_event> events[PG_EVENT_TABLES];
    uint64_t unresolved = 0;
};

inline int event_table_of(int kind) { return kind == 0 ? 0 : kind == 1 ? 1 : kind == PG_SV_TD ? 2 : kind == PG_SV_TD_NT ? 3 : -1; }
inline int event_kind_of(int table) { return table == 0 ? 0 : table == 1 ? 1 : table == 2 ? PG_SV_TD : PG_SV_TD_NT; }

// BoxSize / NumBoxes, pindel.cpp:1806-1810, as Caller::process_window has them
inline void event_boxes(size_t chr_len, unsigned &box_size, unsigned &n_boxes)
{
    box_size = (unsigned)(chr_len / 30000);
    if (box_size == 0) box_size = 1;
    n_boxes = (unsigned)(chr_len * 2 / box_size) + 1;
}

// The list of `kind` of a read: its records, its count byte and how many records a list of the kind can hold
inline void event_list(const EventReadIn &r, int kind, const pg_variant_cand *&list, uint8_t &count, unsigned &cap)
{
    list = nullptr;
    count = 0;
    cap = 0;
    if (kind < 2) {
        if (!r.var) return;
        list = r.var + kind * PG_VARIANT_CANDS;
        count = r.var_counts[kind];
        cap = PG_VARIANT_CANDS;
    } else {
        if (!r.sv) return;
        list = r.sv + sv_slot_base()[kind - PG_SV_DI];
        count = r.sv_counts[kind - PG_SV_DI];
        cap = (kind == PG_SV_TD || kind == PG_SV_INV) ? PG_VARIANT_CANDS : 1u;
    }
}

// nt_str(read index, record): NT_str of a kind 1 pair (needs the read's bases and points: the caller has them)
template <class NtStr>
inline void events_from_lists(const std::string &ref, unsigned spacer, const pg_event_window &w, const std::vector<EventReadIn> &in,
                              NtStr nt_str, EventTables &out)
{
    const size_t n = in.size();
    out.reads.assign(n, pg_event_read());
    out.unresolved = 0;
    unsigned box_size, n_boxes;
    event_boxes(ref.size(), box_size, n_boxes);
    struct Boxed {
        uint32_t read;
        const pg_variant_cand *c;
        uint16_t nt;
        unsigned box;
    };
    std::vector<Boxed> boxed[PG_EVENT_TABLES];

    // ---- stage A: the cascade, read by read, in process_window's order
    int order[7], n_order = 0;
    order[n_order++] = 0;
    order[n_order++] = PG_SV_DI;
    if (w.analyze_td) {
        order[n_order++] = PG_SV_TD;
        order[n_order++] = PG_SV_TD_NT;
    }
    if (w.analyze_inv) {
        order[n_order++] = PG_SV_INV;
        order[n_order++] = PG_SV_INV_NT;
    }
    order[n_order++] = 1;
    for (size_t i = 0; i < n; i++) {
        const EventReadIn &r = in[i];
        if (!r.in_window) continue;
        pg_event_read &rec = out.reads[i];
        uint16_t nt = 0;                                    // the leftover NT_size
        bool used = false;
        for (int o = 0; o < n_order && !used; o++) {
            const int kind = order[o];
            const pg_variant_cand *list;
            uint8_t count;
            unsigned cap;
            event_list(r, kind, list, count, cap);
            const unsigned n_listed = std::min<unsigned>(count & ~PG_VARIANT_MORE, cap);
            for (unsigned j = 0; j < n_listed && !used; j++) {
                const pg_variant_cand &c = list[j];
                bool box_it = false;
                unsigned box = 0;
                // readTransgressesBinBoundaries: unsigned arithmetic with a short insert size
                const bool transgress = c.bp_right > w.win_end - 2 * r.insert_size;
                const bool in_region = c.bp_left + 1 >= w.region_start && c.bp_left + 1 <= w.region_end;
                if (kind < 2) {
                    if (c.flags & PG_VARIANT_REF_END) used = true;
                    else if (transgress) used = true;
                    else if (in_region) {
                        box = (unsigned)((int)c.bp_left / (int)box_size);
                        if (box < n_boxes) box_it = used = true;
                    }
                } else {
                    if (kind != PG_SV_TD) nt = (uint16_t)c.nt_rot;
                    if (c.flags & PG_VARIANT_REF_END) used = true;           // ... and the box test still runs
                    const bool check = !(kind == PG_SV_INV && !r.plus);   // inversions with a '-' anchor skip the transgression test
                    if (check && transgress) used = true;
                    else if (in_region) {
                        box = (unsigned)((int)c.bp_left / (int)box_size);
                        if (box < n_boxes) box_it = used = true;
                    }
                }
                if (used) {
                    rec.kind = (uint8_t)kind;
                    rec.slot = (uint8_t)j;
                    rec.flags = box_it ? PG_EVR_BOXED : PG_EVR_USED;
                    if (box_it) {
                        rec.nt_size = nt;
                        const int t = event_table_of(kind);
                        if (t >= 0) boxed[t].push_back(Boxed{ (uint32_t)i, &c, nt, box });
                    }
                }
            }
            if (!used && (count & PG_VARIANT_MORE)) {
                rec.flags = PG_EVR_UNRESOLVED;
                rec.unresolved_kind = (uint8_t)kind;
                out.unresolved++;
                break;
            }
        }
    }

    for (int t = 0; t < PG_EVENT_TABLES; t++) {
        std::vector<Boxed> &bx = boxed[t];
        const int kind = event_kind_of(t);
        // ---- stage B: the order bubblesortReads leaves a box in -- ascending by smaller()'s key, equal keys in descending read
        // index (the argument above exchange_sort_reference).  A box is a range of BPLeft, the primary key, so one sort of the
        // whole kind is the sorted boxes one after the other, in box order.
        std::sort(bx.begin(), bx.end(), [](const Boxed &a, const Boxed &b) {
            if (a.c->bp_left != b.c->bp_left) return a.c->bp_left < b.c->bp_left;
            if (a.c->bp_right != b.c->bp_right) return a.c->bp_right < b.c->bp_right;
            if (a.c->indel_size != b.c->indel_size) return a.c->indel_size < b.c->indel_size;
            if (a.nt != b.nt) return a.nt < b.nt;
            if (a.c->bp != b.c->bp) return a.c->bp < b.c->bp;
            return a.read > b.read;
        });
        // ---- stage C: markDuplicates per box.  A read is boxed at most once in a window (boxing makes it Used), and only a
        // reporter clears UniqueRead, on the reads of its own boxes: every read that arrives here is still unique, so within a
        // (Left, Right, name) class of a box the first is unique and all later ones are duplicates.  The host reporters skip a
        // box with fewer than -M reads; marking there too changes only reads of events that cannot reach the cutoff.
        std::vector<Boxed> good;
        std::set<std::tuple<int, int, uint32_t>> seen;
        for (size_t k = 0; k < bx.size(); k++) {
            if (k == 0 || bx[k].box != bx[k - 1].box) seen.clear();
            // (without name ids the caller numbers the reads themselves: nothing is ever a duplicate)
            const std::tuple<int, int, uint32_t> key(bx[k].c->left, bx[k].c->right, in[bx[k].read].name_id);
            const bool dup = !seen.insert(key).second;
            if (dup) out.reads[bx[k].read].flags |= PG_EVR_DUPLICATE;
            else good.push_back(bx[k]);
        }
        // ---- stage D: events = maximal runs of consecutive members with an equal key
        std::vector<uint32_t> &mem = out.members[t];
        std::vector<pg_event> &evs = out.events[t];
        mem.clear();
        evs.clear();
        for (const Boxed &g : good) mem.push_back(g.read);
        uint32_t box_head = 0;
        for (size_t s = 0; s < good.size();) {
            if (s == 0 || good[s].box != good[s - 1].box) box_head = (uint32_t)s;
            size_t e = s + 1;
            while (e < good.size() && good[e].c->bp_left == good[s].c->bp_left &&
                   (kind == 1 ? good[e].c->indel_size == good[s].c->indel_size : good[e].c->bp_right == good[s].c->bp_right))
                e++;
            const pg_variant_cand &f = *good[s].c;
            pg_event ev = pg_event();
            ev.kind = (uint8_t)kind;
            ev.bp_left = f.bp_left;
            ev.bp_right = f.bp_right;
            ev.indel_size = f.indel_size;
            ev.nt_size = good[s].nt;
            ev.first = (uint32_t)s;
            ev.n_reads = (uint32_t)(e - s);
            ev.box_head = box_head;
            unsigned rs = f.bp_left, re = f.bp_right;
            if (kind == 1) {
                std::string str = nt_str(good[s].read, f);
                if (!str.empty()) real_start_insertion(ref, spacer, str, rs, re);
            } else {
                real_start_deletion(ref, spacer, rs, re);
            }
            ev.real_start = rs;
            ev.real_end = re;
            bool lmin = false, lmax = false, rmin = false, rmax = false;        // ReportEvent, with its short arithmetic
            for (size_t k = s; k < e; k++) {
                const EventReadIn &r = in[good[k].read];
                if (r.plus) ev.n_plus++;
                const short bp = good[k].c->bp;
                const unsigned short nts = good[k].nt;
                short rl = (short)(r.read_length - nts);
                short mn = (short)((short)((rl * 0.5) + 0.5) - 1);
                short mx = (short)((short)(rl * (1 - 0.5) - 0.5) - 1);
                if (bp <= mn) lmin = true;
                if (r.read_length - bp - nts <= mn) rmin = true;
                if (bp >= mx) lmax = true;
                if (r.read_length - bp - nts >= mx) rmax = true;
            }
            unsigned flags = 0;
            if (ev.n_reads >= w.min_support) flags |= PG_EV_SUPPORT;
            if (kind == 0 || (kind == 1 ? rs < re : !(re < rs || rs == 0))) flags |= PG_EV_RANGE;
            if (kind == 1 || f.indel_size < w.balance_cutoff || (lmin && lmax && rmin && rmax)) flags |= PG_EV_BALANCE;
            if (flags == (PG_EV_SUPPORT | PG_EV_RANGE | PG_EV_BALANCE)) flags |= PG_EV_REPORT;
            ev.flags = (uint8_t)flags;
            evs.push_back(ev);
            s = e;
        }
    }
}

}  // namespace detail
}  // namespace pgh
#endif
