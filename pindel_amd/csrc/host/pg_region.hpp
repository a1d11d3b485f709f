// pg_region.hpp -- the region plan: which parts of which chromosomes a run searches, in which order.
// Pindel's -c, -j and -J (SearchRegion, src/user_defined_settings.cpp:104-162; the IncludeBed set-up in main,
// src/pindel.cpp:1605-1720; CleanUpBedRecord, src/pindel.cpp:1380-1511), restated once for every caller:
// the pindel_pg command line, pgh_call_from_points and pgh_region_plan.
//
//   -c ALL                one record [1, size] per chromosome, in reference order
//   -c <chr>              [1, size]
//   -c <chr>:<s>          [s, size]
//   -c <chr>:<s>-<e>      [s, min(e, size)]          (commas in the coordinates are ignored)
//   -j include.bed        the file's records instead (with -c ALL as given; with a -c region only those on its
//                         chromosome that overlap it, clipped to it).  BED values are taken as Pindel's 1-based
//                         positions, with no 0-based shift, as the reference does -- unless bed_zero_based is set
//                         (--repair bed0): then a record [s, e) of either file is the positions s + 1 ... e,
//                         before anything else is done with it, and a record without a base (s == e) is left out.
//   -J exclude.bed        CleanUpBedRecord on the include list (see clean_up below)
//
// `size` is the chromosome's .fai length, or the FASTA length without an .fai (the same number for a consistent
// index).  Each record [S, E] is then searched in windows from S - 10 kbp to E + 10 kbp (pg_pipeline.hpp).
//
// Differences from the reference, on input it mishandles:
//   * a BED line that does not parse is an error naming its line number (the reference stops reading the file
//     there, silently); blank lines and lines starting with '#', "track" or "browser" are skipped;
//   * an include record on a chromosome that is not in the reference is an error (the reference dereferences a
//     null chromosome);
//   * an exclude list that removes every record gives an empty plan (the reference underflows size() - 1).
#ifndef PG_REGION_HPP
#define PG_REGION_HPP

#include <algorithm>
#include <cctype>
#include <cstdint>
#include <fstream>
#include <string>
#include <utility>
#include <vector>

namespace pgh {

struct RegionRecord {
    int chr = -1;                  // index into the genome
    unsigned start = 0, end = 0;   // Pindel coordinates, both ends included
};

// -c as given on the command line, syntax only (no reference needed)
struct RegionSpec {
    bool all = true;
    std::string chr;
    bool has_start = false, has_end = false;
    unsigned start = 1, end = 0;
};

enum { REGION_OK = 0, REGION_BAD_INPUT = 1, REGION_BAD_SYNTAX = 2 };

namespace region_detail {

// a decimal number without sign that fits in 32 bits
inline bool parse_u32(const std::string &s, unsigned &v)
{
    if (s.empty() || s.size() > 10) return false;
    uint64_t x = 0;
    for (char ch : s) {
        if (ch < '0' || ch > '9') return false;
        x = x * 10 + (unsigned)(ch - '0');
    }
    if (x > 0xffffffffull) return false;
    v = (unsigned)x;
    return true;
}

inline int find_chr(const std::vector<std::string> &names, const std::string &name)
{
    for (size_t c = 0; c < names.size(); c++)
        if (names[c] == name) return (int)c;
    return -1;
}

// chr start end per line, the rest of the line ignored; start > end swapped (the reference's reading loop)
struct BedLine {
    std::string chr;
    unsigned start, end;
};
inline int read_bed(const std::string &path, std::vector<BedLine> &out, std::string &err)
{
    std::ifstream f(path.c_str());
    if (!f) {
        err = "cannot open BED file " + path;
        return REGION_BAD_INPUT;
    }
    std::string line;
    for (size_t no = 1; std::getline(f, line); no++) {
        std::vector<std::string> field;
        size_t p = 0;
        while (field.size() < 3) {
            while (p < line.size() && std::isspace((unsigned char)line[p])) p++;
            if (p >= line.size()) break;
            const size_t q = p;
            while (p < line.size() && !std::isspace((unsigned char)line[p])) p++;
            field.push_back(line.substr(q, p - q));
        }
        if (field.empty() || field[0][0] == '#' || field[0] == "track" || field[0] == "browser") continue;
        BedLine b;
        if (field.size() < 3 || !parse_u32(field[1], b.start) || !parse_u32(field[2], b.end)) {
            err = path + " line " + std::to_string(no) + ": expected <chromosome> <start> <end>, got \"" + line + "\"";
            return REGION_BAD_INPUT;
        }
        b.chr = field[0];
        if (b.start > b.end) std::swap(b.start, b.end);
        out.push_back(b);
    }
    return REGION_OK;
}

// CleanUpBedRecord (pindel.cpp:1380-1511), in its order and with its quirks.  Nothing happens without an exclude.
//  1. Each include record (records appended on the way included) against each exclude on its chromosome, until the
//     record is empty (start == end): an exclude containing it empties it; one strictly inside it cuts it in two,
//     the right piece [exclude end, end] appended at the END of the list; a one-sided overlap trims it.
//  2. Empty records are dropped.
//  3. One pairwise pass merges overlapping (or touching) records of a chromosome: one contained in a later one is
//     emptied and the pass moves on to the next `first`; a later one contained in it is emptied, likewise; a partial
//     overlap widens `first` and empties the later one.  Emptied records still take part in later comparisons.
//  4. Empty records are dropped; the rest are sorted by (chromosome index, start) with the reference's exchange
//     sort, which swaps only on a strictly smaller key.
inline void clean_up(std::vector<RegionRecord> &inc, const std::vector<RegionRecord> &exc)
{
    if (exc.empty()) return;
    for (size_t i = 0; i < inc.size(); i++) {
        for (const RegionRecord &x : exc) {
            if (inc[i].start == inc[i].end) break;
            if (inc[i].chr != x.chr) continue;
            RegionRecord &r = inc[i];
            if (r.start > x.end || x.start > r.end) continue;
            if (x.start <= r.start && r.end <= x.end) r.end = r.start;
            else if (r.start < x.start && x.end < r.end) {
                RegionRecord right = r;
                right.start = x.end;
                r.end = x.start;
                inc.push_back(right);                  // (may reallocate: `r` is not used after this)
                continue;
            } else if (x.start <= r.start && r.start < x.end && x.end < r.end) r.start = x.end;
            else if (r.start < x.start && x.start < r.end && r.end < x.end) r.end = x.start;
        }
    }
    std::vector<RegionRecord> res;
    for (const RegionRecord &r : inc)
        if (r.start != r.end) res.push_back(r);
    for (size_t a = 0; a + 1 < res.size(); a++) {
        for (size_t b = a + 1; b < res.size(); b++) {
            RegionRecord &f = res[a], &s = res[b];
            if (f.chr != s.chr) continue;
            if (f.start > s.end || s.start > f.end) continue;
            if (s.start <= f.start && f.end <= s.end) {
                f.end = f.start;
                break;
            } else if (f.start <= s.start && s.end <= f.end) {
                s.start = s.end;
                break;
            } else if (s.start <= f.start && f.start <= s.end && s.end <= f.end) {
                f.start = s.start;
                s.start = s.end;
            } else if (f.start <= s.start && s.start <= f.end && f.end <= s.end) {
                f.end = s.end;
                s.start = s.end;
            }
        }
    }
    inc.clear();
    for (const RegionRecord &r : res)
        if (r.start != r.end) inc.push_back(r);
    auto less = [](const RegionRecord &p, const RegionRecord &q) { return p.chr != q.chr ? p.chr < q.chr : p.start < q.start; };
    bool tie = false;                                  // with distinct keys any sort gives the exchange sort's order
    {
        std::vector<std::pair<int, unsigned>> keys;
        for (const RegionRecord &r : inc) keys.push_back(std::make_pair(r.chr, r.start));
        std::sort(keys.begin(), keys.end());
        tie = std::adjacent_find(keys.begin(), keys.end()) != keys.end();
    }
    if (!tie) std::sort(inc.begin(), inc.end(), less);
    else
        for (size_t a = 0; a + 1 < inc.size(); a++)
            for (size_t b = a + 1; b < inc.size(); b++)
                if (less(inc[b], inc[a])) std::swap(inc[a], inc[b]);
    // (the reference's sort loop also clips each end to the chromosome size: every end here is within it already)
}

}  // namespace region_detail

// -c syntax (SearchRegion::SearchRegion): ALL, <chr>, <chr>:<start>, <chr>:<start>-<end>.  REGION_BAD_SYNTAX for a
// coordinate that is not a number or an end below the start.  An empty string means ALL.
inline int parse_region(const std::string &text, RegionSpec &spec, std::string &err)
{
    spec = RegionSpec();
    if (text.empty() || text == "ALL") return REGION_OK;
    spec.all = false;
    const size_t colon = text.find(':');
    spec.chr = text.substr(0, colon);
    if (colon == std::string::npos) return REGION_OK;
    std::string coords;
    for (char ch : text.substr(colon + 1))
        if (ch != ',') coords.push_back(ch);
    const size_t dash = coords.find('-');
    spec.has_start = true;
    spec.has_end = dash != std::string::npos;
    if (!region_detail::parse_u32(coords.substr(0, dash), spec.start) ||
        (spec.has_end && !region_detail::parse_u32(coords.substr(dash + 1), spec.end))) {
        err = "cannot parse the region '" + text + "': give -c ALL, -c <chromosome> or -c <chromosome>:<start>[-<end>], "
              "for example -c 20, -c 20:1,000 or -c 20:1,000-50,000";
        return REGION_BAD_SYNTAX;
    }
    if (spec.has_end && spec.end < spec.start) {
        err = "region '" + text + "': the end lies before the start";
        return REGION_BAD_SYNTAX;
    }
    return REGION_OK;
}

// The plan: the ordered records a run searches.  names / sizes: the reference's chromosomes and their sizes.
// include_bed / exclude_bed: empty = none.  Returns REGION_OK, REGION_BAD_SYNTAX (-c) or REGION_BAD_INPUT (an unknown
// chromosome, a start beyond the chromosome's end, an unreadable or malformed BED file); err says which.
inline int region_plan(const std::vector<std::string> &names, const std::vector<unsigned> &sizes, const std::string &region,
                       const std::string &include_bed, const std::string &exclude_bed, std::vector<RegionRecord> &plan,
                       std::string &err, bool bed_zero_based = false)
{
    using namespace region_detail;
    plan.clear();
    RegionSpec spec;
    int rc = parse_region(region, spec, err);
    if (rc) return rc;
    // BED's [s, e), 0-based, as Pindel positions s + 1 ... e (read_bed has put the smaller value first)
    auto zero_based = [&](std::vector<BedLine> &bed) {
        if (!bed_zero_based) return;
        std::vector<BedLine> kept;
        for (BedLine b : bed) {
            if (b.start == b.end) continue;
            b.start++;
            kept.push_back(b);
        }
        bed.swap(kept);
    };
    RegionRecord target;                                // the -c region, when there is one
    if (!spec.all) {
        target.chr = find_chr(names, spec.chr);
        if (target.chr < 0) {
            err = "region '" + region + "': there is no chromosome " + spec.chr + " in the reference";
            return REGION_BAD_INPUT;
        }
        const unsigned size = sizes[target.chr];
        target.start = spec.has_start ? spec.start : 1;
        target.end = spec.has_end ? std::min(spec.end, size) : size;
        if (target.start > size) {
            err = "region '" + region + "': the start lies beyond the end of " + spec.chr + " (" + std::to_string(size) + ")";
            return REGION_BAD_INPUT;
        }
    }
    if (include_bed.empty()) {
        if (spec.all)
            for (size_t c = 0; c < names.size(); c++) {
                RegionRecord r;
                r.chr = (int)c;
                r.start = 1;
                r.end = sizes[c];
                plan.push_back(r);
            }
        else plan.push_back(target);
    } else {
        std::vector<BedLine> bed;
        if ((rc = read_bed(include_bed, bed, err))) return rc;
        zero_based(bed);
        for (const BedLine &b : bed) {
            RegionRecord r;
            r.chr = find_chr(names, b.chr);
            if (r.chr < 0) {
                err = include_bed + ": there is no chromosome " + b.chr + " in the reference";
                return REGION_BAD_INPUT;
            }
            r.start = b.start;
            r.end = std::min(b.end, sizes[r.chr]);
            if (!spec.all) {                            // keep what overlaps the -c region, clipped to it
                if (r.chr != target.chr || b.start > target.end || target.start > b.end) continue;
                r.start = std::max(b.start, target.start);
                r.end = std::min(b.end, target.end);
            }
            plan.push_back(r);
        }
    }
    if (!exclude_bed.empty()) {
        std::vector<BedLine> bed;
        if ((rc = read_bed(exclude_bed, bed, err))) return rc;
        zero_based(bed);
        std::vector<RegionRecord> exc;
        for (const BedLine &b : bed) {                  // (an exclude on a chromosome the reference lacks matches nothing)
            RegionRecord r;
            r.chr = find_chr(names, b.chr);
            r.start = b.start;
            r.end = b.end;
            if (r.chr >= 0) exc.push_back(r);
        }
        clean_up(plan, exc);
    }
    return REGION_OK;
}

// Where the windows of record [S, E] run (LoopingSearchWindow with Bed_start / Bed_end, pindel.cpp:383-394): from
// S - 10 kbp (AROUND_REGION_BUFFER, not below 0) to min(biological size, E + 10 kbp).
inline unsigned region_global_start(const RegionRecord &r) { return r.start >= 10000u ? r.start - 10000u : 0u; }
inline unsigned region_global_end(const RegionRecord &r, unsigned biol)
{
    return (unsigned)std::min<uint64_t>(biol, (uint64_t)r.end + 10000u);
}

}  // namespace pgh
#endif
