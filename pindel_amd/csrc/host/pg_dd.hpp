// pg_dd.hpp -- -q: dispersed duplications (_DD), Pindel's MEI search (src/search_MEI.cpp, src/search_MEI_util.cpp)
// restated on this repository's BAM reader.  The two steps that need the reference's search code come in as callbacks:
// the close end of the split reads around each cluster (the command line: pg_close_end_batch) and the containment test
// of each candidate breakpoint's consensus (the command line: pg_dd_contains_batch; dd_contains_any_strand below is the
// same test on the host).
#ifndef PG_DD_HPP
#define PG_DD_HPP

#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "pg_adapter.hpp"
#include "pg_host.hpp"
#include "pg_region.hpp"

namespace pgh {

struct BamSource;
struct BamIngestSettings;

// The DD flags of src/fn_parameters.cpp:305-350
struct DDSettings {
    int max_bp_distance = 350;        // --MAX_DD_BREAKPOINT_DISTANCE
    int max_distance_cluster = 100;   // --MAX_DISTANCE_CLUSTER_READS
    int min_cluster_size = 3;         // --MIN_DD_CLUSTER_SIZE
    int min_bp_support = 3;           // --MIN_DD_BREAKPOINT_SUPPORT
    int min_map_distance = 8000;      // --MIN_DD_MAP_DISTANCE
    bool report_dup_reads = false;    // --DD_REPORT_DUPLICATION_READS
};

// contains_subseq (src/search_MEI_util.cpp:188-342) as written: db = db_len bytes, max_mismatch = g_maxMismatch (500 entries).
// A window of 0 bases is false (the reference's arrays would have no column 0).
bool dd_contains_subseq(const std::string &query, const char *db, size_t db_len, int min_length, const uint32_t *max_mismatch);
// contains_subseq_any_strand (:346-349): the query, then its ReverseComplement (Convert2RC4N), with min_length 15
bool dd_contains_any_strand(const std::string &query, const char *db, size_t db_len, const uint32_t *max_mismatch);

// The close end of one batch of split-read candidates: per read whether it has one, the rc flag of pg_result_view and
// UP_Close.back() (AbsLoc, LengthStr).
struct DDClose {
    uint8_t has = 0, rc_flag = 0;
    uint32_t last_abs = 0;
    uint16_t last_len = 0;
};
typedef std::function<int(int chr_id, const pg_adapter::Batch &batch, std::vector<DDClose> &out)> DDCloseFn;
// The containment test of many items at once: out[i] = contains_subseq_any_strand(queries[i], chromosome chr[i] at padded
// positions [start[i], start[i] + len[i]))
typedef std::function<int(const std::vector<std::string> &queries, const std::vector<int32_t> &chr, const std::vector<uint64_t> &start,
                          const std::vector<uint32_t> &len, std::vector<uint8_t> &out)>
    DDContainsFn;

struct DDStats {
    size_t discordant = 0, clusters = 0, breakpoints = 0, candidates = 0, kept_by_containment = 0, events = 0;
    double contains_seconds = 0.0;
    std::vector<int> bp_list;         // per breakpoint found (searchMEIBreakpoints order): tid, pos, strand, #reads, #split reads
    std::string tested;               // per containment test: "tid pos strand #split-reads consensus contained" lines (tab-separated)
    std::string note;                 // set when the run differs from what the reference would do (no breakpoint at all)
};

// searchMEImain (src/search_MEI.cpp:963-1024): writes <prefix>_DD.  ingest (-A, -n, -u, spacer) and window_mbp (-w) as in the
// main search; sizes = the chromosome sizes of the region plan.  0 = done; otherwise err says why.
int run_dd(const std::vector<Chromosome> &genome, const std::vector<unsigned> &sizes, const std::vector<RegionRecord> &plan,
           const std::vector<BamSource> &bams, const BamIngestSettings &ingest, double window_mbp, const DDSettings &dd,
           const std::string &prefix, const DDCloseFn &close_fn, const DDContainsFn &contains_fn, std::string &err,
           DDStats *stats = nullptr);

}  // namespace pgh
#endif
