// pg_host_report.hpp -- report records from tables, lists and points, on the host: the plain-loop statement of what
// pg_report.hip gathers on the device, with the same inputs and byte-identical outputs (pgh_report_reads_from_lists).  One
// pg_report_read per member of the seven member lists -- what good_of / write_sv_table of pg_host_events.cpp take from the lists
// and the points for that member -- and one pg_report_summary per read: what the pipeline and process_window read of the points.
#ifndef PG_HOST_REPORT_HPP
#define PG_HOST_REPORT_HPP

#include <cstring>
#include <vector>

#include "pg_host_events.hpp"
#include "pg_host_sv_events.hpp"

namespace pgh {
namespace detail {

// what the records read of one read
struct ReportReadIn {
    bool plus = false;                        // MatchedD == '+'
    uint8_t rc_flag = 0;
    const UniquePoint *close = nullptr;       // UP_Close
    size_t n_close = 0;
    const UniquePoint *far = nullptr;         // UP_Far
    size_t n_far = 0;
    const pg_variant_cand *var = nullptr;     // 2 x PG_VARIANT_CANDS records
    const pg_variant_cand *sv = nullptr;      // PG_SV_SLOTS records
    const uint8_t *sv_counts = nullptr;       // PG_SV_KINDS
};

// recs: the events build's per-read records; ev_members[t] / sv_members[t]: the member lists of its tables and of the SV tables
// (member words: PG_SVEV_MEMBER_DUP marks an inversion's duplicate).  A member whose read, kind or slot lies outside the reads or
// their lists gets a zeroed record; a point index outside its list counts as LengthStr 0.
inline void report_reads_from_lists(const std::vector<ReportReadIn> &in, const pg_event_read *recs, const std::vector<uint32_t> *ev_members,
                                    const std::vector<uint32_t> *sv_members, std::vector<pg_report_read> &records,
                                    std::vector<pg_report_summary> &summaries)
{
    const size_t n = in.size();
    summaries.assign(n, pg_report_summary());
    for (size_t i = 0; i < n; i++) {
        const ReportReadIn &r = in[i];
        pg_report_summary &s = summaries[i];
        std::memset(&s, 0, sizeof s);
        s.rc_flag = r.rc_flag;
        if (r.n_close) {
            s.close_abs = r.close[r.n_close - 1].AbsLoc;
            s.close_len = r.close[r.n_close - 1].LengthStr;
            s.flags |= PG_RS_CLOSE;
        }
        if (r.n_far) {
            s.far_chr = (int16_t)r.far[0].chr;
            s.flags |= PG_RS_FAR;
            if (r.far[0].Strand == '-') s.flags |= PG_RS_FAR_ANTISENSE;
            if (r.n_close && r.close[0].AbsLoc < r.far[0].AbsLoc) s.flags |= PG_RS_CLOSE_LEFT;
            if (r.n_close && r.close[0].AbsLoc > r.far[0].AbsLoc) s.flags |= PG_RS_CLOSE_RIGHT;
        }
    }
    records.clear();
    for (int t = 0; t < PG_EVENT_TABLES + PG_SV_EVENT_TABLES; t++) {
        const std::vector<uint32_t> &members = t < PG_EVENT_TABLES ? ev_members[t] : sv_members[t - PG_EVENT_TABLES];
        for (uint32_t word : members) {
            const uint32_t read = t < PG_EVENT_TABLES ? word : word & ~PG_SVEV_MEMBER_DUP;
            pg_report_read rec;
            std::memset(&rec, 0, sizeof rec);
            records.push_back(rec);
            if (read >= n) continue;
            const ReportReadIn &r = in[read];
            const pg_event_read &er = recs[read];
            const pg_variant_cand *c = nullptr;
            if (er.kind < 2) {
                if (er.slot < PG_VARIANT_CANDS) c = r.var + er.kind * PG_VARIANT_CANDS + er.slot;
            } else if (er.kind <= PG_SV_INV_NT) {
                const unsigned cap = (er.kind == PG_SV_TD || er.kind == PG_SV_INV) ? PG_VARIANT_CANDS : 1u;
                if (er.slot < cap) c = r.sv + sv_slot_base()[er.kind - PG_SV_DI] + er.slot;
            }
            if (!c) continue;
            rec.read = read;
            rec.cand = *c;
            rec.nt_size = er.nt_size;
            rec.table = (uint8_t)t;
            if (t >= PG_EVENT_TABLES && (word & PG_SVEV_MEMBER_DUP)) rec.flags |= PG_RR_DUP;
            if (t == 1) {
                // what variant_pair_from_cand cuts NT_str behind
                short len0 = 0;
                if (r.plus) {
                    if (c->close_idx < r.n_close) len0 = r.close[c->close_idx].LengthStr;
                } else if (c->far_idx < r.n_far) {
                    len0 = r.far[c->far_idx].LengthStr;
                }
                rec.bp0 = (short)(len0 - 1);
            }
            if (t == 2 && (r.sv_counts[0] & ~PG_VARIANT_MORE) >= 1) {
                // searchTandemDuplications leaves NT_str alone: it is DI's where DI listed a pair
                rec.flags |= PG_RR_DI;
                rec.di_bp = r.sv[0].bp;
                rec.di_nt_rot = r.sv[0].nt_rot;
            }
            records.back() = rec;
        }
    }
}

}  // namespace detail
}  // namespace pgh
#endif
