// pg_host_priv.hpp -- helpers shared by pg_host.cpp and pg_host_sv.cpp (not installed).
#ifndef PG_HOST_PRIV_HPP
#define PG_HOST_PRIV_HPP

#include <sstream>
#include <string>
#include <algorithm>
#include <functional>
#include <unordered_set>
#include <utility>
#include <cstdlib>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#include "pg_host.hpp"

namespace pgh {

struct Caller::Ctx {
    const Chromosome *chrom;
    std::vector<SplitRead> *reads;
    unsigned NumBoxes;
    unsigned win_start, win_end;
    unsigned region_start, region_end;
    // the tables route: the window's long-insertion tables and close lengths, built before its reads lost their points
    bool li_ready = false;
    LiTables li;
    std::vector<int16_t> li_close_len;
    // ... and its interchromosomal junction tables, with the summaries that name the junction reads
    bool int_ready = false;
    IntTables int_tables;
    std::vector<pg_report_summary> int_summaries;
};

namespace detail {

inline char rc4n(char c)   // Convert2RC4N, src/pindel.cpp:966-970 (unset entries are 0)
{
    switch (c) {
    case 'A': return 'T';
    case 'C': return 'G';
    case 'G': return 'C';
    case 'T': return 'A';
    case 'N': return 'N';
    default: return 0;
    }
}

inline std::string cap2low(const std::string &s)        // Cap2LowArray, src/pindel.cpp:971-976
{
    std::string o(s.size(), 0);
    for (size_t i = 0; i < s.size(); i++) {
        switch (s[i]) {
        case 'A': o[i] = 'a'; break;
        case 'C': o[i] = 'c'; break;
        case 'G': o[i] = 'g'; break;
        case 'T': o[i] = 't'; break;
        case 'N': case '$': o[i] = 'n'; break;
        default: o[i] = 0; break;
        }
    }
    return o;
}

// std::string::substr that never throws (the reference only calls it in range)
inline std::string sub(const std::string &s, long pos, long n)
{
    if (pos < 0 || (size_t)pos > s.size() || n <= 0) return std::string();
    return s.substr((size_t)pos, (size_t)n);
}

// readTransgressesBinBoundaries, src/pindel.cpp:561-564
inline bool transgresses(const SplitRead &r, unsigned upper) { return r.BPRight > upper - 2 * r.InsertSize; }

static const char *const HASHES =
    "####################################################################################################";
static const char *const DASHES =
    "----------------------------------------------------------------------------------------------------";

inline std::string read_tail(const SplitRead &r)
{
    std::ostringstream o;
    o << "\t" << r.MatchedD << "\t" << r.MatchedRelPos << "\t" << r.MS << "\t" << r.Tag << "\t" << r.Name;
    return o.str();
}

// GetRealStart4Deletion, src/pindel.cpp:2095-2118
inline void real_start_deletion(const std::string &chr, unsigned spacer, unsigned &rs, unsigned &re)
{
    if (chr.size() < rs || chr.size() < re) return;
    unsigned pos = rs + spacer, start = pos + 1, end = re + spacer - 1;
    while (chr[pos] == chr[end] && chr[pos] != 'N') {
        --pos;
        --end;
    }
    rs = pos - spacer;
    pos = re + spacer;
    while (chr[pos] == chr[start] && chr[pos] != 'N') {
        ++pos;
        ++start;
    }
    re = pos - spacer;
}

// GetRealStart4Insertion, src/pindel.cpp:2134-2162
inline void real_start_insertion(const std::string &chr, unsigned spacer, std::string &ins, unsigned &rs, unsigned &re)
{
    if (chr.size() < rs || chr.size() < re) return;
    unsigned after = re + spacer;
    while (chr[after] == ins[0] && chr[after] != 'N') {
        ins = ins.substr(1) + ins[0];
        after++;
    }
    re = after - spacer;
    unsigned before = after - 1;
    while (chr[before] == ins[ins.size() - 1] && chr[before] != 'N') {
        ins = ins[ins.size() - 1] + ins.substr(0, ins.size() - 1);
        before--;
    }
    rs = before - spacer;
}

// One (close point, far point) pair of SearchVariant::Search (src/search_variant.cpp:120-214; kind 0 = deletions, 1 = short
// insertions): the direction and geometry tests, then everything the loop computes for the pair before
// readTransgressesBinBoundaries -- Left, Right, BP, IndelSize, NT_str, BPLeft / BPRight left-aligned against the reference and
// the `diff` shift -- as a pg_variant_cand (pindel_pg.h) plus the string.  false: the pair does not qualify.  With
// PG_VARIANT_REF_END set the loop marks the read Used and stops; the fields are then those before the alignment.
struct VariantPair {
    pg_variant_cand c;
    std::string nt;               // NT_str as the alignment left it
};
inline bool variant_pair(const SplitRead &r, int kind, int ci, int fi, const std::string &ref, unsigned spacer, VariantPair &out)
{
    const bool plus = r.MatchedD == '+';
    const UniquePoint &cp = r.UP_Close[ci], &fp = r.UP_Far[fi];
    if (fp.Direction != (plus ? '-' : '+')) return false;
    bool ok;
    if (kind == 0) {
        ok = plus ? (fp.LengthStr + cp.LengthStr == r.getReadLength() && fp.AbsLoc > cp.AbsLoc + 1)
                  : (cp.LengthStr + fp.LengthStr == r.getReadLength() && cp.AbsLoc > fp.AbsLoc + 1);
    } else {
        ok = plus ? (fp.AbsLoc == cp.AbsLoc + 1 && cp.LengthStr + fp.LengthStr < r.getReadLength())
                  : (cp.AbsLoc == fp.AbsLoc + 1 && fp.LengthStr + cp.LengthStr < r.getReadLength());
    }
    if (!ok) return false;
    int Left, Right;
    short BP;
    if (plus) {
        Left = (int)(cp.AbsLoc - cp.LengthStr + 1);
        Right = (int)(fp.AbsLoc + fp.LengthStr - 1);
        BP = (short)(cp.LengthStr - 1);
    } else {
        Left = (int)(fp.AbsLoc - fp.LengthStr + 1);
        Right = (int)(cp.AbsLoc + cp.LengthStr - 1);
        BP = (short)(fp.LengthStr - 1);
    }
    unsigned IndelSize;
    if (kind == 0) {
        IndelSize = (unsigned)((Right - Left) - r.getReadLengthMinus());
        out.nt.clear();
    } else {
        IndelSize = (unsigned)(r.getReadLengthMinus() - (Right - Left));
        out.nt = plus ? sub(reverse_complement(r.UnmatchedSeq), BP + 1, IndelSize) : sub(r.UnmatchedSeq, BP + 1, IndelSize);
    }
    unsigned BPLeft, BPRight;
    if (plus) {
        BPLeft = cp.AbsLoc - spacer;
        BPRight = fp.AbsLoc - spacer;
    } else {
        BPLeft = fp.AbsLoc - spacer;
        BPRight = cp.AbsLoc - spacer;
    }
    pg_variant_cand &c = out.c;
    c = pg_variant_cand();
    c.close_idx = (uint16_t)ci;
    c.far_idx = (uint16_t)fi;
    c.left = Left;
    c.right = Right;
    c.indel_size = IndelSize;
    unsigned real_l = BPLeft, real_r = BPRight;
    if (ref.size() < real_l || ref.size() < real_r) {
        c.flags = PG_VARIANT_REF_END;
    } else {
        if (!out.nt.empty()) {
            real_start_insertion(ref, spacer, out.nt, real_l, real_r);
            // left rotations = how far the right end moved; right rotations = the distance the second loop walked back from it
            c.nt_rot = (int32_t)(real_r - BPRight) - (int32_t)(real_r - 1 - real_l);
        } else {
            real_start_deletion(ref, spacer, real_l, real_r);
        }
        short diff = (short)(BPLeft - real_l);
        diff = !((BP - 1) < diff) ? diff : (short)(BP - 1);
        if (diff > 0) {
            BP -= diff;
            BPLeft -= diff;
            BPRight -= diff;
        }
    }
    c.bp = BP;
    c.bp_left = BPLeft;
    c.bp_right = BPRight;
    return true;
}

// UP_Close[0] against UP_Far[0], as OutputInversions orients a read.  A read that has its points is judged by them and never
// consults CloseVsFar; only a read of the tables path, which has neither list, is judged by what its summary said of
// them.  A writer that reads a point in any other way faults on such a read: that is how the gold tests of that path catch it.
inline bool close_left_of_far(const SplitRead &r)
{
    return r.UP_Close.empty() || r.UP_Far.empty() ? r.CloseVsFar < 0 : r.UP_Close[0].AbsLoc < r.UP_Far[0].AbsLoc;
}
inline bool close_right_of_far(const SplitRead &r)
{
    return r.UP_Close.empty() || r.UP_Far.empty() ? r.CloseVsFar > 0 : r.UP_Close[0].AbsLoc > r.UP_Far[0].AbsLoc;
}

// NT_str of a kind 1 pair: the read's substring behind bp0 (LengthStr - 1 of the pair's close point for a '+' anchor, of its far
// point otherwise; pg_report_read::bp0), rotated left by nt_rot
inline std::string variant_nt_str(const SplitRead &r, short bp0, unsigned indel_size, int32_t nt_rot)
{
    std::string nt = r.MatchedD == '+' ? sub(reverse_complement(r.UnmatchedSeq), bp0 + 1, indel_size) : sub(r.UnmatchedSeq, bp0 + 1, indel_size);
    const long len = (long)nt.size();
    if (len > 1) {
        const long rot = (((long)nt_rot % len) + len) % len;
        std::rotate(nt.begin(), nt.begin() + rot, nt.end());
    }
    return nt;
}

// A listed candidate back to what variant_pair yields: NT_str is rebuilt from the read (cut as the loop cuts it, then rotated).
// false: the record does not fit the read (indices outside its point lists).
inline bool variant_pair_from_cand(const SplitRead &r, int kind, const pg_variant_cand &c, VariantPair &out)
{
    if (c.close_idx >= r.UP_Close.size() || c.far_idx >= r.UP_Far.size()) return false;
    out.c = c;
    out.nt.clear();
    if (kind == 1) {
        const bool plus = r.MatchedD == '+';
        const short bp0 = (short)((plus ? r.UP_Close[c.close_idx].LengthStr : r.UP_Far[c.far_idx].LengthStr) - 1);
        out.nt = variant_nt_str(r, bp0, c.indel_size, c.nt_rot);
    }
    return true;
}

inline void apply_variant_pair(SplitRead &r, const VariantPair &p)
{
    r.Left = p.c.left;
    r.Right = p.c.right;
    r.BP = p.c.bp;
    r.IndelSize = p.c.indel_size;
    r.NT_str = p.nt;
    r.BPLeft = p.c.bp_left;
    r.BPRight = p.c.bp_right;
}

// ---- the five other classifiers: one function per (close point, far point) pair, used by the classifiers'
// loops (pg_host.cpp, pg_host_sv.cpp) and by pgh_sv_candidates.  Each yields a pg_variant_cand with what the classifier has
// assigned when it reaches the window-dependent tail, and NT_str where the kind has one.  false: the pair does not qualify.

// LeftMostTD, src/search_tandem_duplications.cpp:194-222, on the values.  true: the out-of-range branch (the read is Used)
inline bool left_most_td(const std::string &ref, unsigned spacer, unsigned &BPLeft, unsigned &BPRight, short &BP)
{
    unsigned pos = BPLeft + spacer, orig = pos, end = BPRight + spacer - 1;
    unsigned n = (unsigned)ref.size();
    if (pos >= n || end >= n) {
        BPLeft = 1;
        BPRight = 1;
        BP = 1;
        return true;
    }
    while (ref[pos] == ref[end]) {
        --pos;
        --end;
    }
    int diff = (int)(orig - pos);
    if (diff > 0) {
        if (diff >= BP) diff = BP - 1;
        BPLeft -= diff;
        BPRight -= diff;
        BP -= (short)diff;
    }
    return false;
}

// LeftMostINV, src/search_inversions.cpp:285-318, on the values
inline bool left_most_inv(const std::string &ref, unsigned spacer, bool plus, short read_length, unsigned &BPLeft, unsigned &BPRight, short &BP)
{
    unsigned n = (unsigned)ref.size();
    unsigned pos = BPLeft + spacer + 1, orig = pos, end = BPRight + spacer - 1;
    if (n <= pos + spacer || n <= orig + spacer) {
        BPLeft = 1;
        BPRight = 1;
        BP = 1;
        return true;
    }
    while (ref[pos] == rc4n(ref[end])) {
        ++pos;
        --end;
    }
    short diff = (short)(pos - orig);
    if (diff > 0) {
        if (plus) {
            if (diff >= BP) diff = (short)(BP - 1);
        } else {
            if (diff + BP >= read_length) diff = (short)(read_length - BP - 1);
            BPLeft += diff;
            BPRight -= diff;
            BP += diff;
        }
    }
    return false;
}

// the mismatch budget of the kinds with non-template bases: (short)(1 + Seq_Error_Rate * length sum), the product rounded on its own
inline short sv_nt_budget(double rate, int len_sum)
{
    volatile double prod = rate * len_sum;
    return (short)(1 + prod);
}

// -v as the lists take it: used as unsigned, so a negative value or one above 2^30 lets the unsigned sums wrap and the two
// distance tests of searchInversionsNT overlap; no list is made or consulted then
inline bool sv_list_usable(const Settings &S) { return S.MIN_IndelSize_Inversion >= 0 && S.MIN_IndelSize_Inversion <= PG_SV_MAX_INVERSION_SIZE; }

inline const int *sv_slot_base()
{
    static const int base[PG_SV_KINDS] = { 0, 1, 1 + PG_VARIANT_CANDS, 2 + PG_VARIANT_CANDS, 2 + 2 * PG_VARIANT_CANDS };
    return base;
}

// searchIndels, src/search_deletions_nt.cpp:40-120: UP_Close.back() with UP_Far.back()
inline bool sv_pair_di(const SplitRead &r, const pg_sv_params &prm, unsigned spacer, VariantPair &out)
{
    const UniquePoint &cp = r.UP_Close.back();
    const UniquePoint &fp = r.UP_Far.back();
    if (fp.Mismatches + cp.Mismatches > sv_nt_budget(prm.seq_error_rate, fp.LengthStr + cp.LengthStr)) return false;
    const bool plus = r.MatchedD == '+';
    if (!plus && r.MatchedD != '-') return false;
    if (fp.Direction != (plus ? '-' : '+')) return false;
    if (!(fp.LengthStr + cp.LengthStr < r.getReadLength() && fp.LengthStr + cp.LengthStr >= prm.min_num_matched_bases)) return false;
    pg_variant_cand &c = out.c;
    c = pg_variant_cand();
    unsigned short NT_size;
    if (plus) {
        if (!(fp.AbsLoc > cp.AbsLoc + 1)) return false;
        c.left = (int)(cp.AbsLoc - cp.LengthStr + 1);
        c.right = (int)(fp.AbsLoc + fp.LengthStr - 1);
        c.bp = (short)(cp.LengthStr - 1);
        NT_size = (unsigned short)(r.getReadLength() - fp.LengthStr - cp.LengthStr);
        out.nt = sub(reverse_complement(r.UnmatchedSeq), c.bp + 1, NT_size);
        c.indel_size = (unsigned)((c.right - c.left) + NT_size - r.getReadLengthMinus());
        c.bp_left = cp.AbsLoc - spacer;
        c.bp_right = fp.AbsLoc - spacer;
    } else {
        if (!(cp.AbsLoc > fp.AbsLoc + 1)) return false;
        c.left = (int)(fp.AbsLoc - fp.LengthStr + 1);
        c.right = (int)(cp.AbsLoc + cp.LengthStr - 1);
        c.bp = (short)(fp.LengthStr - 1);
        NT_size = (unsigned short)(r.getReadLength() - cp.LengthStr - fp.LengthStr);
        out.nt = sub(r.UnmatchedSeq, c.bp + 1, NT_size);
        c.indel_size = (unsigned)((c.right - c.left) - r.getReadLengthMinus() + NT_size);
        c.bp_left = fp.AbsLoc - spacer;
        c.bp_right = cp.AbsLoc - spacer;
    }
    c.nt_rot = NT_size;
    c.close_idx = (uint16_t)(r.UP_Close.size() - 1);
    c.far_idx = (uint16_t)(r.UP_Far.size() - 1);
    return true;
}

// searchTandemDuplications, src/search_tandem_duplications.cpp:60-180, one pair.  *assigned (nullable): the loop assigned the
// read's fields for this pair although it then skipped it (BPLeft == 0); out.c holds them
inline bool sv_pair_td(const SplitRead &r, int ci, int fi, const std::string &ref, unsigned spacer, VariantPair &out, bool *assigned = nullptr)
{
    const bool plus = r.MatchedD == '+';
    const UniquePoint &cp = r.UP_Close[ci], &fp = r.UP_Far[fi];
    if (assigned) *assigned = false;
    pg_variant_cand &c = out.c;
    c = pg_variant_cand();
    out.nt.clear();
    if (plus) {
        if (fp.Direction != '-') return false;
        if (!(fp.LengthStr + cp.LengthStr == r.getReadLength() && fp.AbsLoc + fp.LengthStr < cp.AbsLoc && fp.AbsLoc + cp.LengthStr < cp.AbsLoc))
            return false;
        c.right = (int)(cp.AbsLoc - cp.LengthStr + 1);
        c.left = (int)(fp.AbsLoc + fp.LengthStr - 1);
        c.bp = (short)(cp.LengthStr - 1);
        c.indel_size = cp.AbsLoc - fp.AbsLoc + 1;
        c.bp_right = cp.AbsLoc - spacer;
        c.bp_left = fp.AbsLoc - spacer;
    } else {
        if (fp.Direction != '+') return false;
        if (!(cp.LengthStr + fp.LengthStr == r.getReadLength() && cp.AbsLoc + cp.LengthStr < fp.AbsLoc && cp.AbsLoc + fp.LengthStr < fp.AbsLoc))
            return false;
        c.right = (int)(fp.AbsLoc - fp.LengthStr + 1);
        c.left = (int)(cp.AbsLoc + cp.LengthStr - 1);
        c.bp = (short)(fp.LengthStr - 1);
        c.indel_size = fp.AbsLoc - cp.AbsLoc + 1;
        c.bp_right = fp.AbsLoc - spacer;
        c.bp_left = cp.AbsLoc - spacer;
    }
    c.close_idx = (uint16_t)ci;
    c.far_idx = (uint16_t)fi;
    if (c.bp_left == 0) {
        if (assigned) *assigned = true;
        return false;
    }
    unsigned bl = c.bp_left, br = c.bp_right;
    short bp = c.bp;
    if (left_most_td(ref, spacer, bl, br, bp)) c.flags = PG_VARIANT_REF_END;
    c.bp_left = bl;
    c.bp_right = br;
    c.bp = bp;
    return true;
}

// searchTandemDuplicationsNT, src/search_tandem_duplications_nt.cpp:40-125
inline bool sv_pair_td_nt(const SplitRead &r, const pg_sv_params &prm, unsigned spacer, VariantPair &out)
{
    const UniquePoint &cp = r.UP_Close.back();
    const UniquePoint &fp = r.UP_Far.back();
    if (fp.LengthStr + cp.LengthStr >= r.getReadLength()) return false;
    if (fp.Mismatches + cp.Mismatches > sv_nt_budget(prm.seq_error_rate, fp.LengthStr + cp.LengthStr)) return false;
    pg_variant_cand &c = out.c;
    c = pg_variant_cand();
    unsigned short NT_size;
    if (r.MatchedD == '+') {
        if (fp.Direction != '-') return false;
        if (!(fp.AbsLoc + fp.LengthStr < cp.AbsLoc && fp.AbsLoc + cp.LengthStr < cp.AbsLoc &&
              fp.LengthStr + cp.LengthStr > prm.min_num_matched_bases))
            return false;
        c.right = (int)(cp.AbsLoc - cp.LengthStr + 1);
        c.left = (int)(fp.AbsLoc + fp.LengthStr - 1);
        c.bp = (short)(cp.LengthStr - 1);
        c.indel_size = cp.AbsLoc - fp.AbsLoc + 1;
        NT_size = (unsigned short)(r.getReadLength() - cp.LengthStr - fp.LengthStr);
        out.nt = sub(reverse_complement(r.UnmatchedSeq), c.bp + 1, NT_size);
        c.bp_right = cp.AbsLoc - spacer;
        c.bp_left = fp.AbsLoc - spacer;
    } else if (r.MatchedD == '-') {
        if (fp.Direction != '+') return false;
        if (!(cp.AbsLoc + cp.LengthStr < fp.AbsLoc && cp.AbsLoc + fp.LengthStr < fp.AbsLoc &&
              fp.LengthStr + cp.LengthStr > prm.min_num_matched_bases))
            return false;
        c.right = (int)(fp.AbsLoc - fp.LengthStr + 1);
        c.left = (int)(cp.AbsLoc + cp.LengthStr - 1);
        c.bp = (short)(fp.LengthStr - 1);
        c.indel_size = fp.AbsLoc - cp.AbsLoc + 1;
        NT_size = (unsigned short)(r.getReadLength() - cp.LengthStr - fp.LengthStr);
        out.nt = sub(r.UnmatchedSeq, c.bp + 1, NT_size);
        c.bp_right = fp.AbsLoc - spacer;
        c.bp_left = cp.AbsLoc - spacer;
    } else {
        return false;
    }
    c.nt_rot = NT_size;
    c.close_idx = (uint16_t)(r.UP_Close.size() - 1);
    c.far_idx = (uint16_t)(r.UP_Far.size() - 1);
    return true;
}

// The read-level tests of both inversion classifiers: strand differs and direction is equal between the first points
inline bool sv_inv_read_ok(const SplitRead &r)
{
    return r.UP_Close[0].Strand != r.UP_Far[0].Strand && r.UP_Close[0].Direction == r.UP_Far[0].Direction;
}
// ... and which geometry searchInversions takes for the read (src/search_inversions.cpp:53, 118, 186, 245); -1: none
inline int sv_inv_geometry(const SplitRead &r, unsigned MIN)
{
    if (r.MatchedD == '+') {
        if (r.UP_Far[0].AbsLoc > r.UP_Close.back().AbsLoc + MIN) return 0;
        if (r.UP_Far.back().AbsLoc + MIN < r.UP_Close[0].AbsLoc) return 1;
    } else if (r.MatchedD == '-') {
        if (r.UP_Close.back().AbsLoc > r.UP_Far[0].AbsLoc + MIN) return 2;
        if (r.UP_Close[0].AbsLoc + MIN < r.UP_Far.back().AbsLoc) return 3;
    }
    return -1;
}

// The fields the four geometries assign (shared by searchInversions and searchInversionsNT); RL = the read's length
inline void sv_inv_fields(int geo, const UniquePoint &cp, const UniquePoint &fp, short RL, unsigned spacer, pg_variant_cand &c)
{
    if (geo == 0) {
        c.left = (int)((cp.AbsLoc + 1) - cp.LengthStr);
        c.right = (int)(fp.AbsLoc - fp.LengthStr + RL);
        c.bp = (short)(cp.LengthStr - 1);
        c.indel_size = fp.AbsLoc - cp.AbsLoc;
        c.bp_left = cp.AbsLoc + 1 - spacer;
        c.bp_right = fp.AbsLoc - spacer;
    } else if (geo == 1) {
        c.right = (int)(cp.AbsLoc - cp.LengthStr + RL);
        c.left = (int)(fp.AbsLoc - fp.LengthStr + 1);
        c.bp = (short)(fp.LengthStr - 1);
        c.indel_size = cp.AbsLoc - fp.AbsLoc;
        c.bp_right = cp.AbsLoc - spacer;
        c.bp_left = (fp.AbsLoc + 1) - spacer;
    } else if (geo == 2) {
        c.left = (int)(fp.AbsLoc + fp.LengthStr - RL);
        c.right = (int)(cp.AbsLoc + cp.LengthStr - 1);
        c.bp = (short)(fp.LengthStr - 1);
        c.indel_size = cp.AbsLoc - fp.AbsLoc;
        c.bp_left = fp.AbsLoc - spacer;
        c.bp_right = cp.AbsLoc - 1 - spacer;
    } else {
        c.right = (int)(fp.AbsLoc + fp.LengthStr - 1);
        c.left = (int)(cp.AbsLoc + cp.LengthStr - RL);
        c.bp = (short)(cp.LengthStr - 1);
        c.indel_size = fp.AbsLoc - cp.AbsLoc;
        c.bp_left = cp.AbsLoc - spacer;
        c.bp_right = fp.AbsLoc - 1 - spacer;
    }
    c.flags = (uint8_t)(geo << PG_SV_GEO_SHIFT);
}
inline bool sv_inv_distance_ok(int geo, const UniquePoint &cp, const UniquePoint &fp, unsigned MIN)
{
    switch (geo) {
    case 0: return fp.AbsLoc > cp.AbsLoc + MIN;
    case 1: return fp.AbsLoc + MIN < cp.AbsLoc;
    case 2: return cp.AbsLoc > fp.AbsLoc + MIN;
    default: return cp.AbsLoc + MIN < fp.AbsLoc;
    }
}

// searchInversions, src/search_inversions.cpp:40-280, one pair of a read of geometry geo
inline bool sv_pair_inv(const SplitRead &r, int geo, int ci, int fi, unsigned MIN, const std::string &ref, unsigned spacer, VariantPair &out)
{
    const bool plus = r.MatchedD == '+';
    const UniquePoint &cp = r.UP_Close[ci], &fp = r.UP_Far[fi];
    if (fp.Direction != (plus ? '+' : '-')) return false;
    if (fp.LengthStr + cp.LengthStr != r.getReadLength()) return false;
    if (!sv_inv_distance_ok(geo, cp, fp, MIN)) return false;
    pg_variant_cand &c = out.c;
    c = pg_variant_cand();
    out.nt.clear();
    sv_inv_fields(geo, cp, fp, r.getReadLength(), spacer, c);
    c.close_idx = (uint16_t)ci;
    c.far_idx = (uint16_t)fi;
    unsigned bl = c.bp_left, br = c.bp_right;
    short bp = c.bp;
    if (left_most_inv(ref, spacer, plus, r.getReadLength(), bl, br, bp)) c.flags |= PG_VARIANT_REF_END;
    c.bp_left = bl;
    c.bp_right = br;
    c.bp = bp;
    return true;
}

// searchInversionsNT, src/search_inversions_nt.cpp:40-195: UP_Close.back() with UP_Far.back().  which = 0 / 1: the first / second
// distance test of the anchor's strand (geometries 0, 1 for '+' and 2, 3 for '-').  The tests before them are sv_inv_nt_read_ok's.
inline bool sv_inv_nt_read_ok(const SplitRead &r, const pg_sv_params &prm)
{
    const UniquePoint &cp = r.UP_Close.back();
    const UniquePoint &fp = r.UP_Far.back();
    if (fp.Mismatches + cp.Mismatches > sv_nt_budget(prm.seq_error_rate, fp.LengthStr + cp.LengthStr)) return false;
    if (!sv_inv_read_ok(r)) return false;
    if (!(fp.LengthStr + cp.LengthStr < r.getReadLength() && fp.LengthStr + cp.LengthStr >= prm.min_num_matched_bases)) return false;
    const bool plus = r.MatchedD == '+';
    if (!plus && r.MatchedD != '-') return false;
    return fp.Direction == (plus ? '+' : '-');
}
inline bool sv_pair_inv_nt(const SplitRead &r, const pg_sv_params &prm, int which, unsigned spacer, VariantPair &out)
{
    const UniquePoint &cp = r.UP_Close.back();
    const UniquePoint &fp = r.UP_Far.back();
    const int geo = (r.MatchedD == '+' ? 0 : 2) + which;
    if (!sv_inv_distance_ok(geo, cp, fp, (unsigned)prm.min_inversion_size)) return false;
    pg_variant_cand &c = out.c;
    c = pg_variant_cand();
    sv_inv_fields(geo, cp, fp, r.getReadLength(), spacer, c);
    const unsigned short NT_size = (unsigned short)(r.getReadLength() - fp.LengthStr - cp.LengthStr);
    out.nt = (geo == 0 || geo == 3) ? sub(reverse_complement(r.UnmatchedSeq), c.bp + 1, NT_size) : sub(r.UnmatchedSeq, c.bp + 1, NT_size);
    c.nt_rot = NT_size;
    c.close_idx = (uint16_t)(r.UP_Close.size() - 1);
    c.far_idx = (uint16_t)(r.UP_Far.size() - 1);
    return true;
}

// NT_str of a pair of kind PG_SV_*: cut from the read behind bp (empty for the two kinds without non-template bases)
inline std::string sv_nt_str(const SplitRead &r, int kind, short bp, int32_t nt_rot, uint8_t flags)
{
    if (kind == PG_SV_TD || kind == PG_SV_INV) return std::string();
    const int geo = (flags >> PG_SV_GEO_SHIFT) & 3;
    const bool from_rc = kind == PG_SV_INV_NT ? (geo == 0 || geo == 3) : r.MatchedD == '+';
    return from_rc ? sub(reverse_complement(r.UnmatchedSeq), bp + 1, (unsigned short)nt_rot) : sub(r.UnmatchedSeq, bp + 1, (unsigned short)nt_rot);
}

// A listed record of kind PG_SV_* back to what the pair function yields: NT_str is cut from the read again.  false: the record
// does not fit the read.
inline bool sv_pair_from_cand(const SplitRead &r, int kind, const pg_variant_cand &c, VariantPair &out)
{
    if (c.close_idx >= r.UP_Close.size() || c.far_idx >= r.UP_Far.size()) return false;
    out.c = c;
    out.nt = sv_nt_str(r, kind, c.bp, c.nt_rot, c.flags);
    return true;
}

// The read takes a pair's values: exactly the fields the kind's classifier assigns (searchTandemDuplications leaves NT_size and
// NT_str alone).  With PG_VARIANT_REF_END the read is Used, and the box test still runs.
inline void apply_sv_pair(SplitRead &r, int kind, const VariantPair &p)
{
    r.Left = p.c.left;
    r.Right = p.c.right;
    r.BP = p.c.bp;
    r.IndelSize = p.c.indel_size;
    r.BPLeft = p.c.bp_left;
    r.BPRight = p.c.bp_right;
    if (kind != PG_SV_TD) {
        r.NT_size = (unsigned short)p.c.nt_rot;
        r.NT_str = p.nt;
    }
    if (p.c.flags & PG_VARIANT_REF_END) r.Used = true;
}

// The list of one kind consulted for a read: every listed pair, in order, through tail(pair) until one makes the read Used.
// true: the classifier's own search must still run (the list was cut short with PG_VARIANT_MORE, or did not fit the read).
template <class Tail>
inline bool sv_consult_list(SplitRead &r, int kind, VariantPair &pair, Tail tail)
{
    const uint8_t count = r.SvCounts[kind - PG_SV_DI];
    const unsigned cap = (kind == PG_SV_TD || kind == PG_SV_INV) ? PG_VARIANT_CANDS : 1u;
    const unsigned n_listed = std::min<unsigned>(count & ~PG_VARIANT_MORE, cap);
    const pg_variant_cand *list = r.SvCands + sv_slot_base()[kind - PG_SV_DI];
    bool listed_ok = true;
    for (unsigned j = 0; j < n_listed && !r.Used && listed_ok; j++) {
        listed_ok = sv_pair_from_cand(r, kind, list[j], pair);
        if (listed_ok) {
            apply_sv_pair(r, kind, pair);
            tail(pair);
        }
    }
    return !(r.Used || (listed_ok && !(count & PG_VARIANT_MORE)));
}

// What one thread of a classifier did with the lists, added to variant_list_stats() when its range of reads is done
struct ListLog {
    uint64_t fallbacks = 0;
    std::vector<uint32_t> visits;
    void visit(uint32_t index, int kind, unsigned win_end, unsigned region_start, unsigned region_end, unsigned n_boxes, unsigned box_size)
    {
        if (!variant_list_stats().log_visits) return;
        const uint32_t v[7] = { index, (uint32_t)kind, win_end, region_start, region_end, n_boxes, box_size };
        visits.insert(visits.end(), v, v + 7);
    }
    void flush(std::mutex &mu)
    {
        if (!fallbacks && visits.empty()) return;
        std::lock_guard<std::mutex> lk(mu);
        VariantListStats &stats = variant_list_stats();
        stats.fallbacks += fallbacks;
        stats.visits.insert(stats.visits.end(), visits.begin(), visits.end());
    }
};

// ReportEvent, src/pindel.cpp:2059-2093 (Min_Filter_Ratio = 0.5)
inline bool report_event(const std::vector<SplitRead> &g, unsigned s, unsigned e)
{
    bool lmin = false, lmax = false, rmin = false, rmax = false;
    for (unsigned i = s; i <= e; i++) {
        short rl = (short)(g[i].getReadLength() - g[i].NT_size);
        short mn = (short)((short)((rl * 0.5) + 0.5) - 1);
        short mx = (short)((short)(rl * (1 - 0.5) - 0.5) - 1);
        if (g[i].BP <= mn) lmin = true;
        if (g[i].getReadLength() - g[i].BP - g[i].NT_size <= mn) rmin = true;
        if (g[i].BP >= mx) lmax = true;
        if (g[i].getReadLength() - g[i].BP - g[i].NT_size >= mx) rmax = true;
    }
    return lmin && lmax && rmin && rmax;
}

// smaller(), src/reporter.cpp:908-929 (all reads of one window share FragName)
inline bool smaller(const SplitRead &a, const SplitRead &b)
{
    if (a.BPLeft != b.BPLeft) return a.BPLeft < b.BPLeft;
    if (a.BPRight != b.BPRight) return a.BPRight < b.BPRight;
    if (a.IndelSize != b.IndelSize) return a.IndelSize < b.IndelSize;
    if (a.NT_size != b.NT_size) return a.NT_size < b.NT_size;
    if (a.BP != b.BP) return a.BP < b.BP;
    return false;
}

// The classifiers pair every close-end point with every far-end point (budget x |UP_Close| x |UP_Far|
// iterations per read, search_variant.cpp:104-240 and friends) although most of them test
// "LengthStr(close) + LengthStr(far) == ReadLength" first.  UP_Far holds at most one point per length, in
// increasing length (it is one evaluation of the pattern growth), so the only far point that can pass
// that test is found by length; the loop body then runs for that index alone -- same first hit, same
// outcome.  If a caller hands in a list that is not strictly increasing the full loop is used.
struct FarByLength {
    short idx[512];
    bool usable;
    explicit FarByLength(const SplitRead &r) : usable(true)
    {
        for (int i = 0; i < 512; i++) idx[i] = -1;
        int prev = -1;
        const int nf = (int)r.UP_Far.size();
        for (int j = 0; j < nf; j++) {
            const int L = r.UP_Far[j].LengthStr;
            if (L <= prev || L < 0 || L >= 512 || nf > 32000) {
                usable = false;
                return;
            }
            idx[L] = (short)j;
            prev = L;
        }
    }
    // [first, last] = the far indices (descending walk first >= last) that can pair with a close point of
    // length close_len in a read of length read_len; empty when first < last
    void range_desc(int read_len, int close_len, int nf, int &first, int &last) const
    {
        if (!usable) {
            first = nf - 1;
            last = 0;
            return;
        }
        const int L = read_len - close_len;
        const int j = (L >= 0 && L < 512) ? idx[L] : -1;
        first = j;
        last = j < 0 ? 0 : j;
    }
};

// The same idea for the tests on positions (short insertions: "far AbsLoc == close AbsLoc + 1"): the far
// points sorted by (AbsLoc ascending, index descending); the entries of one AbsLoc are then exactly the
// points the descending loop over all far points would have tested successfully, in the same order.
struct FarByLoc {
    std::vector<std::pair<unsigned, int>> v;
    explicit FarByLoc(const SplitRead &r)
    {
        v.reserve(r.UP_Far.size());
        for (int j = 0; j < (int)r.UP_Far.size(); j++) v.push_back(std::make_pair(r.UP_Far[j].AbsLoc, -j));
        std::sort(v.begin(), v.end());
    }
    // [b, e): entries with the given AbsLoc; far index = -v[k].second, descending as k grows
    void range(unsigned loc, size_t &b, size_t &e) const
    {
        b = std::lower_bound(v.begin(), v.end(), std::make_pair(loc, -0x7fffffff)) - v.begin();
        e = b;
        while (e < v.size() && v[e].first == loc) e++;
    }
};

// bubblesortReads, src/reporter.cpp:932-942: an exchange sort that also swaps EQUAL elements,
//     for a < b: if (!smaller(x[a], x[b])) swap(x[a], x[b])
// Its (unstable-looking) order of equal reads is visible in the reports, so it has to be reproduced
// exactly -- but not in O(n^2): that loop leaves the elements sorted by key with equal elements in the
// REVERSE of their original order, i.e. it equals a stable sort of the reversed sequence.  (Each pass
// moves the last of the minimal elements to the front and shifts the others of its class one place
// down the chain; tests/test_cpu_suite.py checks the two against each other on random inputs.)
template <class Less>
inline void exchange_sort_reference(std::vector<unsigned> &idx, Less less)      // the O(n^2) original
{
    const size_t n = idx.size();
    for (size_t a = 0; a + 1 < n; a++)
        for (size_t b = a + 1; b < n; b++)
            if (!less(idx[a], idx[b])) std::swap(idx[a], idx[b]);
}
template <class Less>
inline void exchange_sort_fast(std::vector<unsigned> &idx, Less less)
{
    std::reverse(idx.begin(), idx.end());
    std::stable_sort(idx.begin(), idx.end(), less);
}
inline void exchange_sort(const std::vector<SplitRead> &reads, std::vector<unsigned> &idx)
{
    exchange_sort_fast(idx, [&](unsigned a, unsigned b) { return smaller(reads[a], reads[b]); });
}

// markDuplicates, src/reporter.cpp:946-972: walking the sorted box, a read that is still unique makes
// every LATER read with the same (Left, Right, Name) non-unique.  So within a (Left, Right, Name)
// class everything behind its first unique member is cleared: one hash lookup per read.
inline void mark_duplicates(std::vector<SplitRead> &reads, const std::vector<unsigned> &idx)
{
    struct Key {
        int left, right;
        const std::string *name;
        bool operator==(const Key &o) const { return left == o.left && right == o.right && *name == *o.name; }
    };
    struct Hash {
        size_t operator()(const Key &k) const
        {
            return std::hash<std::string>()(*k.name) ^ ((size_t)(unsigned)k.left * 0x9e3779b97f4a7c15ull) ^ ((size_t)(unsigned)k.right << 21);
        }
    };
    std::unordered_set<Key, Hash> seen_unique;
    seen_unique.reserve(idx.size() * 2);
    for (unsigned i : idx) {
        SplitRead &x = reads[i];
        const Key k = { x.Left, x.Right, &x.Name };
        if (seen_unique.count(k)) x.UniqueRead = false;
        else if (x.UniqueRead) seen_unique.insert(k);
    }
}

}  // namespace detail

// The classifiers' per-read loops on a few threads: body(lo, hi, sink) runs the loop over reads [lo, hi) and queues
// reads for boxes through sink[box].push_back(ri); afterwards the boxes receive them range by range, i.e. in ascending
// read index like the sequential loop would have pushed them.  (Every iteration touches its own read only.)
// threads for the classifiers and reporters: min(hardware, 16), or PGH_THREADS when set (1 = sequential)
inline unsigned host_threads()
{
    unsigned hw = std::thread::hardware_concurrency();
    if (hw == 0) hw = 1;
    unsigned v = std::min(hw, 16u);
    if (const char *e = getenv("PGH_THREADS")) {
        const int k = atoi(e);
        if (k >= 1) v = (unsigned)std::min(k, 64);
    }
    return v;
}

struct BoxSink {
    std::vector<std::pair<unsigned, unsigned>> v;
    struct Ref {
        BoxSink &s;
        unsigned b;
        void push_back(unsigned ri) { s.v.emplace_back(b, ri); }
    };
    Ref operator[](unsigned b) { return Ref{ *this, b }; }
};
template <class Body>
inline void classify_reads(size_t n, std::vector<std::vector<unsigned>> &boxes, Body body)
{
    const unsigned nt = (unsigned)std::max<size_t>(1, std::min<size_t>(host_threads(), n / 8192 + 1));
    std::vector<BoxSink> sinks(nt);
    if (nt == 1) body(0u, (unsigned)n, sinks[0]);
    else {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nt; t++)
            th.emplace_back([&, t]() { body((unsigned)(n * t / nt), (unsigned)(n * (t + 1) / nt), sinks[t]); });
        for (std::thread &x : th) x.join();
    }
    for (BoxSink &s : sinks)
        for (const auto &p : s.v) boxes[p.first].push_back(p.second);
}

}  // namespace pgh
#endif
