// pg_dd.hpp -- -q: dispersed duplications (_DD), Pindel's MEI search (src/search_MEI.cpp, src/search_MEI_util.cpp)
// restated on this repository's BAM reader.  The two steps that need the reference's search code come in as callbacks:
// the close end of the split reads around each cluster (the command line: pg_close_end_batch) and the containment test
// of each candidate breakpoint's consensus (the command line: pg_dd_contains_batch; dd_contains_any_strand below is the
// same test on the host).
// Between the two lies the breakpoint step in two parts: dd_tables_from_close states the contract of pindel_pg.h
// "dispersed-duplication breakpoint tables" in plain loops -- members, candidates, consensus pool, verdicts -- and one consumer
// turns such tables into the reads and candidates of searchMEIBreakpoints.  A third callback (DDTablesFn; the command line:
// pg_device_batch_close_search + pg_device_batch_dd) may supply the tables instead of close end + statement + containment.
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

// pg_dd_window without the segment arrays, and the padded length of its chromosome
struct DDWindow {
    int32_t chr_id = 0;
    uint64_t chr_len = 0;
    int32_t min_bp_support = 3, min_map_distance = 8000;
};
// The tables of the contract: pg_dd_sizes is their three sizes
struct DDTables {
    std::vector<pg_dd_member> members;
    std::vector<pg_dd_cand> cands;
    std::vector<uint8_t> cons;
};
// The statement.  close: one DDClose per read of the batch (has = a close end, last_abs / last_len = close_last / close_max);
// segment s = the reads [seg_first[s], seg_first[s + 1]) with cluster strand seg_strand[s].  PG_DD_CONTAINED comes from ONE call of
// contains_fn over the tested candidates in table order (none tested: no call).  0, or what contains_fn returned.
int dd_tables_from_close(const pg_adapter::Batch &batch, const std::vector<DDClose> &close, const std::vector<uint32_t> &seg_first,
                         const std::vector<uint8_t> &seg_strand, const DDWindow &w, const DDContainsFn &contains_fn, DDTables &out);
// ... with the containment test on the host: dd_contains_any_strand in chrom_seq, the padded bases of w.chr_id
int dd_tables_from_close(const pg_adapter::Batch &batch, const std::vector<DDClose> &close, const std::vector<uint32_t> &seg_first,
                         const std::vector<uint8_t> &seg_strand, const DDWindow &w, const std::string &chrom_seq, const uint32_t *max_mismatch,
                         DDTables &out);
// The tables of one window's split reads from elsewhere (the device): replaces close end + statement + containment
typedef std::function<int(const pg_adapter::Batch &batch, const std::vector<uint32_t> &seg_first, const std::vector<uint8_t> &seg_strand,
                          const DDWindow &w, DDTables &out)>
    DDTablesFn;

// Test hook of the consumer: the candidates it makes of `tables` over n_reads split reads (names, bytes as ingested, anchor
// strands; every read's sample is `sample`) in n_seg segments, as text: per candidate a line "C seg bio_bp tested contained
// consensus", then per read a line "R name sample sequence mapped unmapped" (tab-separated).  false: tables that do not fit the reads.
bool dd_cands_text(unsigned spacer, const std::vector<std::string> &names, const std::string &sample, const uint8_t *seq, const uint64_t *seq_off,
                   const uint8_t *strand, uint32_t n_reads, uint32_t n_seg, const DDTables &tables, std::string &out);

struct DDStats {
    size_t discordant = 0, clusters = 0, breakpoints = 0, candidates = 0, kept_by_containment = 0, events = 0;
    size_t table_windows = 0, table_bytes = 0;   // windows whose tables came from a DDTablesFn, and the bytes of those tables
    double contains_seconds = 0.0;
    std::vector<int> bp_list;         // per breakpoint found (searchMEIBreakpoints order): tid, pos, strand, #reads, #split reads
    std::string tested;               // per containment test: "tid pos strand #split-reads consensus contained" lines (tab-separated)
    std::string note;                 // set when the run differs from what the reference would do (no breakpoint at all)
};

// searchMEImain (src/search_MEI.cpp:963-1024): writes <prefix>_DD.  ingest (-A, -n, -u, spacer) and window_mbp (-w) as in the
// main search; sizes = the chromosome sizes of the region plan.  0 = done; otherwise err says why.  tables_fn (optional): see
// DDTablesFn; contains_seconds is then the time of its calls.
int run_dd(const std::vector<Chromosome> &genome, const std::vector<unsigned> &sizes, const std::vector<RegionRecord> &plan,
           const std::vector<BamSource> &bams, const BamIngestSettings &ingest, double window_mbp, const DDSettings &dd,
           const std::string &prefix, const DDCloseFn &close_fn, const DDContainsFn &contains_fn, std::string &err,
           DDStats *stats = nullptr, const DDTablesFn &tables_fn = DDTablesFn());

}  // namespace pgh
#endif
