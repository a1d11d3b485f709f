// pg_depth.hpp -- read depth of a region and the -N (--NormalSamples) germline filter's use of it, on top of
// pg_bam.hpp (no htslib):
//
//   bam2depth                     src/bam2depth.cpp:37-110   average pileup depth of [beg, end) per BAM
//   getRelativeCoverageInternal   src/bam2depth.cpp:112-137  depth of an event against its two flanks
//   IsGoodTD (the depth branch)   src/reporter.cpp:1113-1153 which BAMs are measured, and the rule on their ratios
//   UpdateSampleID                src/reporter.cpp:140-155
//
// The pileup the reference walks position by position is restated as a sum over CIGAR blocks: the depth it adds
// up at a position is the number of kept reads with an M / = / X base there (deleted and skipped positions are in
// the pileup but subtracted again, bam2depth.cpp:82-88; the base-quality floor is 0), so the sum over [beg, end)
// is the total length of (M / = / X block) n [beg, end).  A read is kept by the pileup's default mask (unmapped,
// secondary, QC-fail and duplicate reads go; supplementary ones stay); a read without CIGAR is not piled up.
// The mapping-quality floor the reference passes (20) never takes effect: bam2depth's local mapQ stays 0
// (bam2depth.cpp:41, 59).  That quirk is kept: MAPQ is not looked at -- unless a floor is asked for (`min_mapq`, what
// --repair depth-mapq sets to the 20 the reference meant): then a record below it is not piled up.
//
// Deliberate differences: htslib's pileup cap of 8000 reads per position is not reproduced; a
// chromosome that a BAM's header lacks gives depth 0 for that BAM (the reference then pileups the whole file with
// no chromosome test); without a .bai the file is scanned with the chromosome test (BamFile::query).
#ifndef PG_DEPTH_HPP
#define PG_DEPTH_HPP

#include <chrono>
#include <cstdint>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "pg_bam.hpp"

namespace pgh {

// Up to three half-open intervals of one chromosome and, per interval, the pileup sum described above.  The sums
// are additive over records, so one pass over the hull of the intervals equals one pass per interval.
struct DepthSums {
    int64_t beg[3] = { 0, 0, 0 }, end[3] = { 0, 0, 0 };
    int64_t sum[3] = { 0, 0, 0 };
    int n = 0;
    void add(int64_t b, int64_t e)
    {
        beg[n] = b;
        end[n] = e;
        sum[n++] = 0;
    }
    // (double)sum / (end - beg), as bam2depth.cpp:93 divides: an empty interval is 0 / 0 = NaN
    double avg(int k) const { return (double)sum[k] / (double)(end[k] - beg[k]); }
};

inline bool depth_record_kept(const BamRecord &r, unsigned min_mapq = 0)
{
    return !(r.flag & (BAM_FUNMAP | BAM_FSECONDARY | BAM_FQCFAIL | BAM_FDUP)) && !r.cigar.empty() && (unsigned)r.mapq >= min_mapq;
}

inline void depth_add_record(const BamRecord &r, DepthSums &d, unsigned min_mapq = 0)
{
    if (!depth_record_kept(r, min_mapq)) return;
    int64_t at = r.pos;
    for (uint32_t c : r.cigar) {
        const int op = c & 15;
        const int64_t len = (int64_t)(c >> 4);
        if (op == BAM_CMATCH || op == 7 || op == 8) {          // M, =, X
            for (int k = 0; k < d.n; k++) {
                const int64_t lo = std::max(at, d.beg[k]), hi = std::min(at + len, d.end[k]);
                if (hi > lo) d.sum[k] += hi - lo;
            }
            at += len;
        } else if (op == BAM_CDEL || op == BAM_CREF_SKIP)
            at += len;                                         // on the reference, not counted
    }
}

// Fills d.sum from the records of chromosome chr_name in `bam`; false: the file could not be read.
inline bool depth_sums(BamFile &bam, const std::string &chr_name, DepthSums &d, unsigned min_mapq = 0)
{
    int64_t lo = 0, hi = 0;
    bool any = false;
    for (int k = 0; k < d.n; k++) {
        d.sum[k] = 0;
        if (d.end[k] <= d.beg[k]) continue;                    // nothing can lie in it
        lo = any ? std::min(lo, d.beg[k]) : d.beg[k];
        hi = any ? std::max(hi, d.end[k]) : d.end[k];
        any = true;
    }
    const int tid = bam.header().id_of(chr_name);
    if (!any || tid < 0 || hi <= 0) return true;
    return bam.query(tid, lo, hi, [&](const BamRecord &r) { depth_add_record(r, d, min_mapq); });
}

// getRelativeCoverageInternal for one BAM: the depth of [start, end) against its two flanks of the same length,
// clipped to the chromosome (chr_size = its biological size).  -1 when both flanks are empty of reads; a flank of
// length zero gives NaN, which the callers' comparisons let fall through as the reference's do.
inline bool depth_ratio(BamFile &bam, const std::string &chr_name, int64_t chr_size, int64_t start, int64_t end, double &ratio,
                        unsigned min_mapq = 0)
{
    const int64_t L = end - start;
    DepthSums d;
    d.add(start - L >= 0 ? start - L : 0, start);
    d.add(start, end);
    d.add(end, end + L > chr_size ? chr_size : end + L);
    if (!depth_sums(bam, chr_name, d, min_mapq)) return false;
    const double before = d.avg(0), sv = d.avg(1), after = d.avg(2);
    if (before + after == 0) ratio = -1;
    else ratio = 2 * (2 * sv) / (before + after);
    return true;
}

// The rule of IsGoodTD on the ratios of the measured BAMs (reporter.cpp:1141-1152)
inline bool depth_rule_td(const double *ratio, size_t n)
{
    size_t good = 0;
    for (size_t k = 0; k < n; k++)
        if (ratio[k] >= 2.7) good++;
    return (n == 1 && good == 1) || (n > 1 && n <= 4 && n - good <= 1) || (n > 4 && ((float)good / n) > 0.66);
}

// What the reporters of a -N run on BAM-derived reads ask: the BAMs of the configuration, opened once; every
// question is answered through a reader of its own (BamFile::open_like: own file handle, shared header and
// index), so the box-parallel reporters and the pipeline's reader thread never share a handle.
class GermlineDepth {
public:
    bool open(const std::vector<std::string> &paths, const std::vector<std::string> &tags, std::string &err, unsigned min_mapq = 0)
    {
        min_mapq_ = min_mapq;
        files_ = std::vector<BamFile>(paths.size());
        tags_ = tags;
        for (size_t k = 0; k < paths.size(); k++)
            if (!files_[k].open(paths[k], err)) return false;
        return true;
    }
    // IsGoodTD's depth branch for the event [start, end) whose reads carry `event_tags`: the BAMs whose tag is among
    // them, in configuration order (UpdateSampleID), each measured, then the rule.  A BAM that cannot be read counts
    // as ratio -1 (its error is kept for the end of the run).
    bool good_td(const std::string &chr_name, int64_t chr_size, int64_t start, int64_t end, const std::set<std::string> &event_tags) const
    {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<double> ratios;
        for (size_t k = 0; k < files_.size(); k++) {
            if (!event_tags.count(tags_[k])) continue;
            double ratio = -1;
            BamFile mine;
            std::string err;
            if (!mine.open_like(files_[k], err) || !depth_ratio(mine, chr_name, chr_size, start, end, ratio, min_mapq_)) {
                std::lock_guard<std::mutex> g(mu_);
                if (error_.empty()) error_ = err.empty() ? "BAM read failed during the germline filter" : err;
                ratio = -1;
            }
            ratios.push_back(ratio);
        }
        const bool keep = depth_rule_td(ratios.data(), ratios.size());
        std::lock_guard<std::mutex> g(mu_);
        seconds_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        queries_ += ratios.size();
        return keep;
    }
    // PGH_TIMING: seconds spent in good_td (summed over the reporter threads) and the BAM regions it measured
    double seconds() const { return seconds_; }
    size_t queries() const { return queries_; }
    const std::string &error() const { return error_; }

private:
    std::vector<BamFile> files_;
    std::vector<std::string> tags_;
    unsigned min_mapq_ = 0;
    mutable std::mutex mu_;
    mutable double seconds_ = 0;
    mutable size_t queries_ = 0;
    mutable std::string error_;
};

}  // namespace pgh
#endif
