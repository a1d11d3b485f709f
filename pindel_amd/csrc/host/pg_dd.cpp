// pg_dd.cpp -- -q: Pindel's dispersed-duplication search (src/search_MEI.cpp) on pg_bam.hpp; see pg_dd.hpp.
// Every sort below is std::sort on the sequence the reference sorts, in the same order, with the reference's comparators
// (they have ties: the order of equal elements is then that of the same library's std::sort on the same input).
#include "pg_dd.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <map>
#include <set>
#include <sstream>

#include "pg_bam.hpp"
#include "pg_host_priv.hpp"
#include "pg_pipeline.hpp"

namespace pgh {

// ------------------------------------------------------------------------------------------ the containment test
bool dd_contains_subseq(const std::string &query, const char *db, size_t db_length, int min_length, const uint32_t *max_mismatch)
{
    if (db_length == 0) return false;
    const size_t query_length = query.size();
    const int min_match_length = min_length - (int)max_mismatch[min_length];
    std::vector<int> mcA(db_length, 0), mcB(db_length, 0), alA(db_length, 0), alB(db_length, 0);
    int *prev_mc = mcA.data(), *current_mc = mcB.data(), *prev_al = alA.data(), *current_al = alB.data();
    for (size_t i = 0; i < query_length; i++) {
        const int min_mismatch_count_current_row = 0;             // (never lowered: counts are never negative)
        int max_alignment_length_current_row = 0;
        current_mc[0] = 0;
        current_al[0] = db[0] == query[i] ? 1 : 0;
        for (size_t j = 1; j < db_length; j++) {
            int max_score = 0;
            char action = 'n';
            int score = (prev_al[j - 1] + 1) * 1 + prev_mc[j - 1] * -2;
            if (query[i] == db[j] && max_score < score) {
                max_score = score;
                action = 'm';
            } else {
                score = prev_al[j - 1] * 1 + (prev_mc[j - 1] + 1) * -2;
                if (max_score < score) {
                    max_score = score;
                    action = 'M';
                }
            }
            score = current_al[j - 1] * 1 + (current_mc[j - 1] + 1) * -2;
            if (max_score < score) {
                max_score = score;
                action = 'g';
            }
            score = (prev_al[j] + 1) * 1 + (prev_mc[j] + 1) * -2;
            if (max_score < score) {
                max_score = score;
                action = 'G';
            }
            switch (action) {
            case 'g': current_mc[j] = current_mc[j - 1] + 1; current_al[j] = current_al[j - 1]; break;
            case 'G': current_mc[j] = prev_mc[j] + 1; current_al[j] = prev_al[j] + 1; break;
            case 'm': current_mc[j] = prev_mc[j - 1]; current_al[j] = prev_al[j - 1] + 1; break;
            case 'M': current_mc[j] = prev_mc[j - 1] + 1; current_al[j] = prev_al[j - 1] + 1; break;
            default:
                current_mc[j] = query[i] == db[j] ? 0 : 1;
                current_al[j] = 1;
                break;
            }
            if (current_al[j] >= min_length && current_mc[j] <= (int)max_mismatch[current_al[j]]) return true;
            if (current_al[j] > max_alignment_length_current_row) max_alignment_length_current_row = current_al[j];
        }
        if ((int)(query_length - i - 1) + (max_alignment_length_current_row - min_mismatch_count_current_row) < min_match_length) return false;
        std::swap(prev_al, current_al);
        std::swap(prev_mc, current_mc);
    }
    return false;
}

bool dd_contains_any_strand(const std::string &query, const char *db, size_t db_len, const uint32_t *max_mismatch)
{
    return dd_contains_subseq(query, db, db_len, 15, max_mismatch) || dd_contains_subseq(reverse_complement(query), db, db_len, 15, max_mismatch);
}

// ------------------------------------------------------------------------------------------ the breakpoint tables
// The contract of pindel_pg.h "dispersed-duplication breakpoint tables" in plain loops: what get_breakpoints and
// get_consensus_unmapped (src/search_MEI.cpp:120-218, 367-424) make of the close ends, as the device entry pg_device_batch_dd
// builds it.  The two must agree byte for byte.
int dd_tables_from_close(const pg_adapter::Batch &batch, const std::vector<DDClose> &close, const std::vector<uint32_t> &seg_first,
                         const std::vector<uint8_t> &seg_strand, const DDWindow &w, const DDContainsFn &contains_fn, DDTables &out)
{
    out = DDTables();
    const size_t n = batch.strand.size(), n_seg = seg_strand.size();
    // the DD reads: segment by segment in ascending read index, then by (seg, pos) with pos unsigned -- a stable sort, so that equal
    // keys keep the ascending read index
    struct DDRead {
        uint32_t seg, pos, read;
    };
    std::vector<DDRead> dd;
    for (size_t s = 0; s < n_seg; s++)
        for (size_t i = seg_first[s]; i < seg_first[s + 1] && i < n; i++)
            if (close[i].has && batch.strand[i] == seg_strand[s]) dd.push_back({ (uint32_t)s, close[i].last_abs, (uint32_t)i });
    std::stable_sort(dd.begin(), dd.end(), [](const DDRead &a, const DDRead &b) { return a.seg != b.seg ? a.seg < b.seg : a.pos < b.pos; });
    for (size_t g0 = 0; g0 < dd.size();) {
        size_t g1 = g0;
        while (g1 < dd.size() && dd[g1].seg == dd[g0].seg && dd[g1].pos == dd[g0].pos) g1++;
        const size_t first = g0, end = g1;
        g0 = g1;
        // (the reference counts "this read and the later ones" at a position's first occurrence only: the total)
        if (w.min_bp_support > 1 && end - first < (size_t)w.min_bp_support) continue;
        const bool plus = seg_strand[dd[first].seg] == '+';
        pg_dd_cand c;
        c.seg = dd[first].seg;
        c.pos = dd[first].pos;
        c.first = (uint32_t)out.members.size();
        c.n_reads = (uint32_t)(end - first);
        c.cons_off = (uint32_t)out.cons.size();
        c.cons_len = c.flags = c.win_len = 0;
        c.win_start = 0;
        // per member the unmapped bases walking away from the breakpoint
        std::vector<std::string> walk;
        size_t max_u = 0;
        for (size_t k = first; k < end; k++) {
            const uint32_t i = dd[k].read;
            out.members.push_back({ i, close[i].last_len, close[i].rc_flag, 0 });
            SplitRead r;
            r.UnmatchedSeq.assign((const char *)batch.seq.data() + batch.off[i], (size_t)(batch.off[i + 1] - batch.off[i]));
            pg_adapter::apply_rc_flag(r, close[i].rc_flag);
            const std::string &S = r.UnmatchedSeq;
            const size_t u = S.size() > close[i].last_len ? S.size() - close[i].last_len : 0;
            std::string wk(u, '\0');
            for (size_t col = 0; col < u; col++) wk[col] = plus ? detail::rc4n(S[u - 1 - col]) : S[u - 1 - col];
            max_u = std::max(max_u, u);
            walk.push_back(wk);
        }
        std::string cons;
        for (size_t col = 0; col < max_u; col++) {
            int counts[256] = { 0 }, n_col = 0;
            for (const std::string &wk : walk)
                if (wk.size() > col) {
                    n_col++;
                    counts[(uint8_t)wk[col]]++;
                }
            // the largest count, the smallest signed char on a tie: std::map<char,int> in order with a strict >
            char best = '?';
            int max_count = 0;
            for (int v = -128; v < 128; v++)
                if (counts[(uint8_t)(signed char)v] > max_count) {
                    max_count = counts[(uint8_t)(signed char)v];
                    best = (char)v;
                }
            // max_count >= 0.8f * read_count in integers: the two agree for every n up to 200 000 at the threshold and one either
            // side of it
            if (5ll * max_count < 4ll * n_col) break;
            cons += best;
        }
        if (cons.size() >= 15u) {
            // (sr_strand is the opposite of the cluster strand, and the reference reverses for sr_strand == PLUS)
            if (!plus) std::reverse(cons.begin(), cons.end());
            c.cons_len = (uint32_t)cons.size();
            c.flags = PG_DD_TESTED;
            // the unsigned expressions of searchMEIBreakpoints; a start at or beyond the chromosome's end has a window of no bases
            const int64_t st = (int64_t)(int32_t)c.pos - (int64_t)w.min_map_distance;
            c.win_start = st > 0 ? (uint64_t)st : 0;
            if (c.win_start < w.chr_len) c.win_len = std::min((unsigned)w.chr_len - (unsigned)c.win_start, 2 * (unsigned)w.min_map_distance);
            out.cons.insert(out.cons.end(), cons.begin(), cons.end());
        }
        out.cands.push_back(c);
    }
    // the containment tests of all tested candidates as ONE call
    std::vector<std::string> queries;
    std::vector<int32_t> q_chr;
    std::vector<uint64_t> q_start;
    std::vector<uint32_t> q_len;
    for (const pg_dd_cand &c : out.cands)
        if (c.flags & PG_DD_TESTED) {
            queries.push_back(std::string((const char *)out.cons.data() + c.cons_off, c.cons_len));
            q_chr.push_back(w.chr_id);
            q_start.push_back(c.win_start);
            q_len.push_back(c.win_len);
        }
    if (queries.empty()) return 0;
    std::vector<uint8_t> found(queries.size(), 0);
    if (const int rc = contains_fn(queries, q_chr, q_start, q_len, found)) return rc;
    size_t item = 0;
    for (pg_dd_cand &c : out.cands)
        if (c.flags & PG_DD_TESTED)
            if (found[item++]) c.flags |= PG_DD_CONTAINED;
    return 0;
}

int dd_tables_from_close(const pg_adapter::Batch &batch, const std::vector<DDClose> &close, const std::vector<uint32_t> &seg_first,
                         const std::vector<uint8_t> &seg_strand, const DDWindow &w, const std::string &chrom_seq, const uint32_t *max_mismatch,
                         DDTables &out)
{
    return dd_tables_from_close(
        batch, close, seg_first, seg_strand, w,
        [&](const std::vector<std::string> &q, const std::vector<int32_t> &, const std::vector<uint64_t> &st, const std::vector<uint32_t> &len,
            std::vector<uint8_t> &found) {
            found.assign(q.size(), 0);
            for (size_t i = 0; i < q.size(); i++) found[i] = dd_contains_any_strand(q[i], chrom_seq.data() + st[i], len[i], max_mismatch) ? 1 : 0;
            return 0;
        },
        out);
}

namespace {

const char PLUS = '+', MINUS = '-';
const std::string COMMENT_PREFIX = "# ";

// simple_read, src/search_MEI.h
struct SimpleRead {
    std::string name;
    int32_t tid = -1, pos = -1;
    char strand = '?', evidence_strand = 0;
    std::string sample_name, sequence;
    int32_t mate_tid = -1, mate_pos = -1;
    char mate_strand = '?';
    bool is_split = false;
    std::string mapped_sequence, unmapped_sequence;
};

struct Breakpoint {                   // MEI_breakpoint
    int tid = 0, pos = 0;
    char strand = 0;
    std::vector<SimpleRead> reads, split_reads;
};

struct Event {                        // MEI_event
    Breakpoint fwd, rev;
    std::vector<SimpleRead> fwd_mapping, rev_mapping;
};

bool comp_simple_read(const SimpleRead *a, const SimpleRead *b)
{
    if (a->strand == PLUS && b->strand != PLUS) return true;
    if (a->strand != PLUS && b->strand == PLUS) return false;
    return a->pos < b->pos;
}
bool comp_simple_read_pos(const SimpleRead &a, const SimpleRead &b)
{
    if (a.tid != b.tid) return a.tid < b.tid;
    if (a.pos != b.pos) return a.pos < b.pos;
    return a.strand < b.strand;
}
bool comp_mapsize(const SimpleRead &a, const SimpleRead &b) { return a.mapped_sequence.length() > b.mapped_sequence.length(); }
bool comp_unmapped_seqsize(const SimpleRead &a, const SimpleRead &b) { return a.unmapped_sequence.length() > b.unmapped_sequence.length(); }
bool comp_breakpoint_pos(const Breakpoint &a, const Breakpoint &b) { return a.tid < b.tid || (a.tid == b.tid && a.pos < b.pos); }

std::string base_read_name(const std::string &n)
{
    const size_t f = n.find("/", 0);
    if (f != std::string::npos && f > 0) return n.substr(1, f - 1);
    return n;
}

std::string bam_sequence(const BamRecord &r)
{
    static const char nt16[] = "=ACMGRSVTWYHKDBN";
    std::string s((size_t)r.l_seq, 'N');
    for (int k = 0; k < r.l_seq; k++) s[(size_t)k] = nt16[(r.seq4[(size_t)k >> 1] >> ((~k & 1) << 2)) & 15];
    return s;
}

// get_sample_dictionary (search_MEI_util.cpp:355-379)
std::map<std::string, std::string> sample_dictionary(const std::string &text)
{
    std::map<std::string, std::string> d;
    std::istringstream hs(text);
    std::string line;
    while (getline(hs, line)) {
        if (line.compare(0, 3, "@RG") != 0) continue;
        size_t idpos = line.find("\tID:"), smpos = line.find("\tSM:");
        if (idpos == std::string::npos || smpos == std::string::npos) continue;
        idpos += 4;
        smpos += 4;
        line += '\t';
        d.insert(std::make_pair(std::string(line, idpos, line.find('\t', idpos) - idpos), std::string(line, smpos, line.find('\t', smpos) - smpos)));
    }
    return d;
}

// What a run keeps between windows (MEI_data + the pieces of ControlState it reads)
struct DDState {
    const std::vector<Chromosome> *genome;
    const std::vector<BamSource> *bams;
    std::vector<BamFile> *files;
    std::set<std::string> sample_tags;                       // g_sampleNames
    std::map<std::string, std::string> sample_names;         // MEI_data::sample_names (the last BAM's header)
    unsigned insert_size = 0;                                // MEI_data::current_insert_size (the last BAM's)
    std::vector<Breakpoint> breakpoints;
    DDStats *stats;
};

// get_sample_name (search_MEI_util.cpp:382-397)
void sample_name_of(const DDState &st, const std::string &rg, std::string &out)
{
    auto it = st.sample_names.find(rg);
    if (it != st.sample_names.end()) out = it->second;
    else if (st.sample_tags.size() == 1) out = *st.sample_tags.begin();
}

// load_discordant_reads + fetch_disc_read_callback (search_MEI.cpp:689-767)
bool load_discordant(DDState &st, const DDSettings &dd, const std::string &chr_name, unsigned ws, unsigned we, std::vector<SimpleRead> &out,
                     std::string &err)
{
    for (size_t k = 0; k < st.bams->size(); k++) {
        BamFile &bam = (*st.files)[k];
        if (!bam.has_index()) continue;                      // "Failed to load index": the window is skipped for this file
        const int tid = bam.header().id_of(chr_name);
        if (tid < 0) continue;
        st.sample_names = sample_dictionary(bam.header().text);
        st.insert_size = (unsigned)(*st.bams)[k].insert_size;
        const unsigned isz = st.insert_size;
        if (!bam.query(tid, ws, we, [&](const BamRecord &b) {
                if ((b.flag & BAM_FUNMAP) || (b.flag & BAM_FMUNMAP)) return;
                // is_concordant (search_MEI.cpp:46-64)
                const bool rev = (b.flag & BAM_FREVERSE) != 0, mrev = (b.flag & BAM_FMREVERSE) != 0;
                const bool concordant = b.tid == b.mtid && rev != mrev && (unsigned int)std::abs(b.tlen) < b.l_seq + 2 * isz;
                if (concordant) return;
                if (!(b.tid != b.mtid || std::abs(b.pos - b.mpos) > dd.min_map_distance)) return;
                SimpleRead r;
                r.name = "@" + b.qname + ((b.flag & BAM_FREAD1) ? "/1" : "/2");
                r.tid = b.tid;
                r.pos = b.pos;
                r.strand = rev ? MINUS : PLUS;
                sample_name_of(st, b.aux_str("RG"), r.sample_name);
                r.sequence = bam_sequence(b);
                r.mate_tid = b.mtid;
                r.mate_pos = b.mpos;
                r.mate_strand = mrev ? MINUS : PLUS;
                out.push_back(r);
            })) {
            err = (*st.bams)[k].path + ": BAM read failed";
            return false;
        }
    }
    return true;
}

// cluster_reads (search_MEI.cpp:70-112)
void cluster_reads(std::vector<SimpleRead *> &reads, int insert_size, const DDSettings &dd, std::vector<std::vector<SimpleRead *>> &clusters)
{
    if (reads.empty()) return;
    std::sort(reads.begin(), reads.end(), comp_simple_read);
    std::vector<SimpleRead *> current;
    SimpleRead *last = reads[0], *first = last;
    current.push_back(last);
    for (size_t i = 1; i < reads.size(); i++) {
        SimpleRead *r = reads[i];
        if ((r->pos - last->pos) <= dd.max_distance_cluster && (unsigned)(r->pos - first->pos) <= (insert_size - first->sequence.length()) &&
            last->strand == r->strand)
            current.push_back(r);
        else {
            clusters.push_back(current);
            current.clear();
            current.push_back(r);
            first = r;
        }
        last = r;
    }
    if (!current.empty()) clusters.push_back(current);
}

// get_breakpoint_estimation (search_MEI.cpp:335-362)
void breakpoint_estimation(const std::vector<SimpleRead *> &cluster, int tid, char strand, std::vector<Breakpoint> &bps)
{
    float dist_mean = 0;
    for (unsigned int i = 0; i < (cluster.size() - 1); i++) dist_mean += (1.0 / (i + 1)) * ((cluster[i + 1]->pos - cluster[i]->pos) - dist_mean);
    float read_len_mean = 0;
    for (unsigned int i = 0; i < cluster.size(); i++) read_len_mean += (1.0 / (i + 1)) * (cluster[i]->sequence.length() - read_len_mean);
    (void)read_len_mean;
    const int outer_pos_high = cluster.back()->pos + cluster.back()->sequence.length();
    const int outer_pos_low = cluster[0]->pos;
    const int estimation = (strand == PLUS) ? outer_pos_high + dist_mean : outer_pos_low - dist_mean;
    Breakpoint bp;
    bp.tid = tid;
    bp.pos = estimation;
    bp.strand = strand;
    for (const SimpleRead *r : cluster) bp.reads.push_back(*r);
    bps.push_back(bp);
}

// One candidate breakpoint of a cluster as searchMEIBreakpoints holds it
struct Cand {
    size_t cluster;
    int bio_bp;
    std::vector<SimpleRead> split_reads;
    std::string consensus;
    bool tested = false, contained = false;
};

// The one consumer of the breakpoint tables: per segment the candidates in the order of the reference's
// std::map<int, ...> over (int)(pos - spacer) -- the tables order pos unsigned -- each with its reads as get_breakpoints makes
// them (name, sample, sequence, mapped / unmapped part; table order = the order the reference appends them in) after the std::sort
// by unmapped length that get_consensus_unmapped leaves behind, and its consensus.  false: a table that does not fit the reads.
bool cands_from_tables(const DDState &st, const DDTables &t, const IngestedReads &in, const std::vector<size_t> &big, unsigned spacer,
                       std::vector<std::vector<Cand>> &cands)
{
    cands.assign(big.size(), std::vector<Cand>());
    std::vector<std::map<int, size_t>> order(big.size());
    for (size_t e = 0; e < t.cands.size(); e++) {
        const pg_dd_cand &c = t.cands[e];
        if (c.seg >= big.size() || !c.n_reads || (uint64_t)c.first + c.n_reads > t.members.size() ||
            (uint64_t)c.cons_off + c.cons_len > t.cons.size() || ((c.flags & PG_DD_TESTED) != 0) != (c.cons_len != 0))
            return false;
        if (!order[c.seg].insert(std::make_pair((int)(c.pos - spacer), e)).second) return false;
    }
    for (size_t b = 0; b < big.size(); b++)
        for (const auto &kv : order[b]) {
            const pg_dd_cand &tc = t.cands[kv.second];
            Cand c;
            c.cluster = big[b];
            c.bio_bp = kv.first;
            for (uint32_t k = tc.first; k < tc.first + tc.n_reads; k++) {
                const pg_dd_member &m = t.members[k];
                if (m.read >= in.size()) return false;
                SplitRead r;
                r.UnmatchedSeq.assign((const char *)in.batch.seq.data() + in.batch.off[m.read], (size_t)(in.batch.off[m.read + 1] - in.batch.off[m.read]));
                pg_adapter::apply_rc_flag(r, m.rc_flag);
                if (m.close_len > r.UnmatchedSeq.size()) return false;
                SimpleRead s;
                s.is_split = true;
                s.name = in.names[m.read];
                if ((char)in.batch.strand[m.read] == PLUS) {
                    s.sequence = reverse_complement(r.UnmatchedSeq);
                    s.mapped_sequence = s.sequence.substr(0, m.close_len);
                    s.unmapped_sequence = s.sequence.substr(m.close_len, s.sequence.length());
                } else {
                    s.sequence = r.UnmatchedSeq;
                    s.mapped_sequence = s.sequence.substr(s.sequence.length() - m.close_len, s.sequence.length());
                    s.unmapped_sequence = s.sequence.substr(0, s.sequence.length() - m.close_len);
                }
                sample_name_of(st, in.read_groups[m.read], s.sample_name);
                c.split_reads.push_back(s);
            }
            std::sort(c.split_reads.begin(), c.split_reads.end(), comp_unmapped_seqsize);
            c.consensus.assign((const char *)t.cons.data() + tc.cons_off, tc.cons_len);
            c.tested = (tc.flags & PG_DD_TESTED) != 0;
            c.contained = (tc.flags & PG_DD_CONTAINED) != 0;
            cands[b].push_back(c);
        }
    return true;
}

// searchMEIBreakpoints (search_MEI.cpp:367-424) for the discordant reads of one window; get_breakpoints' split-read fetch
// (get_split_reads_for_cluster, :120-150) runs for all clusters first, with ONE close-end call, and the containment tests of
// all their candidates then run as ONE call: statement (dd_tables_from_close), then consumer (cands_from_tables).  With a
// tables_fn the tables come from it instead of close_fn, the statement and contains_fn.
int window_breakpoints(DDState &st, const DDSettings &dd, int chr_id, std::vector<SimpleRead> &disc, const BamIngestSettings &ingest,
                       const DDCloseFn &close_fn, const DDContainsFn &contains_fn, const DDTablesFn &tables_fn, std::string &err)
{
    const Chromosome &chrom = (*st.genome)[(size_t)chr_id];
    std::vector<SimpleRead *> ptrs;
    for (SimpleRead &r : disc) ptrs.push_back(&r);
    std::vector<std::vector<SimpleRead *>> clusters;
    cluster_reads(ptrs, (int)st.insert_size, dd, clusters);
    st.stats->clusters += clusters.size();
    // the split reads of every cluster that is big enough, in the reference's order (per BAM, the kept reads in input order)
    std::vector<size_t> big;
    for (size_t i = 0; i < clusters.size(); i++)
        if (clusters[i].size() >= (size_t)dd.min_cluster_size) big.push_back(i);
    const unsigned spacer = ingest.spacer;
    BamIngestSettings ing = ingest;
    ing.read_groups = true;                        // SPLIT_READ::read_group: the RG of the anchor, for get_sample_name
    IngestedReads in;
    in.clear();
    std::vector<uint32_t> seg_first(big.size() + 1, 0);
    std::vector<uint8_t> seg_strand(big.size(), 0);
    for (size_t b = 0; b < big.size(); b++) {
        const std::vector<SimpleRead *> &cl = clusters[big[b]];
        const char strand = cl[0]->strand;
        seg_strand[b] = (uint8_t)strand;
        const int outer = strand == MINUS ? cl.back()->pos : cl[0]->pos;
        for (size_t k = 0; k < st.bams->size(); k++) {
            const int isz = (*st.bams)[k].insert_size;
            const int lower = strand == PLUS ? outer - isz : outer - 2 * isz, upper = strand == PLUS ? outer + 2 * isz : outer + isz;
            // SearchWindow holds unsigned positions: a negative bound wraps round (and the fetch then finds nothing)
            const int64_t lo = (int64_t)(unsigned)lower, hi = (int64_t)(unsigned)upper;
            BamIngest bi(ing);
            if (lo < hi && !bi.read_window((*st.files)[k], chrom.name, chr_id, chrom.seq.size(), lo, hi, isz, (*st.bams)[k].tag, in)) {
                err = (*st.bams)[k].path + ": " + bi.error;
                return -1;
            }
        }
        seg_first[b + 1] = (uint32_t)in.size();
    }
    DDWindow w;
    w.chr_id = chr_id;
    w.chr_len = chrom.seq.size();
    w.min_bp_support = dd.min_bp_support;
    w.min_map_distance = dd.min_map_distance;
    DDTables tables;
    if (in.size() && tables_fn) {
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = tables_fn(in.batch, seg_first, seg_strand, w, tables);
        st.stats->contains_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (rc) {
            err = "building the DD breakpoint tables failed";
            return rc;
        }
        st.stats->table_windows++;
        st.stats->table_bytes += tables.members.size() * sizeof(pg_dd_member) + tables.cands.size() * sizeof(pg_dd_cand) + tables.cons.size();
    } else if (in.size()) {
        std::vector<DDClose> close;
        int rc = close_fn(chr_id, in.batch, close);
        if (rc) {
            err = "close-end search of the DD split reads failed";
            return rc;
        }
        rc = dd_tables_from_close(in.batch, close, seg_first, seg_strand, w,
                                  [&](const std::vector<std::string> &q, const std::vector<int32_t> &chr, const std::vector<uint64_t> &start,
                                      const std::vector<uint32_t> &len, std::vector<uint8_t> &found) {
                                      const auto t0 = std::chrono::steady_clock::now();
                                      const int r = contains_fn(q, chr, start, len, found);
                                      st.stats->contains_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                                      return r;
                                  },
                                  tables);
        if (rc) {
            err = "containment test of the DD consensus sequences failed";
            return rc;
        }
    }
    std::vector<std::vector<Cand>> cands;
    if (!cands_from_tables(st, tables, in, big, spacer, cands)) {
        err = "the DD breakpoint tables of a window do not fit its split reads";
        return -1;
    }
    for (const pg_dd_cand &c : tables.cands) st.stats->candidates += (c.flags & PG_DD_TESTED) != 0;
    for (size_t b = 0; b < big.size(); b++) {
        const std::vector<SimpleRead *> &cl = clusters[big[b]];
        const char strand = cl[0]->strand;
        const int tid = cl[0]->tid;
        std::vector<Breakpoint> bps;
        for (Cand &c : cands[b]) {
            if (c.tested)
                st.stats->tested += std::to_string(tid) + "\t" + std::to_string(c.bio_bp) + "\t" + strand + "\t" + std::to_string(c.split_reads.size()) +
                                    "\t" + c.consensus + "\t" + (c.contained ? "1" : "0") + "\n";
            if (!c.tested || c.contained) continue;
            st.stats->kept_by_containment++;
            Breakpoint bp;
            bp.tid = tid;
            bp.pos = c.bio_bp;
            bp.strand = strand;
            bp.split_reads = c.split_reads;
            for (const SimpleRead *r : cl) bp.reads.push_back(*r);
            bps.push_back(bp);
        }
        if (bps.size() > 1) {
            size_t best_support = 0;
            Breakpoint best;
            for (const Breakpoint &bp : bps)
                if (bp.split_reads.size() > best_support) {
                    best = bp;
                    best_support = bp.split_reads.size();
                }
            bps.clear();
            bps.push_back(best);
        } else if (bps.empty())
            breakpoint_estimation(cl, tid, strand, bps);
        for (const Breakpoint &bp : bps) {
            st.breakpoints.push_back(bp);
            for (int v : { bp.tid, bp.pos, (int)bp.strand, (int)bp.reads.size(), (int)bp.split_reads.size() }) st.stats->bp_list.push_back(v);
        }
    }
    return 0;
}

// the windows of one plan record (main's LoopingSearchWindow, as run_bam_pipeline walks them)
std::vector<std::pair<unsigned, unsigned>> record_windows(const RegionRecord &r, unsigned biol, unsigned window)
{
    std::vector<std::pair<unsigned, unsigned>> w;
    const unsigned global_end = region_global_end(r, biol);
    for (uint64_t ws = region_global_start(r); !(ws > global_end); ws += window)
        w.push_back(std::make_pair((unsigned)ws, (unsigned)std::min<uint64_t>(ws + window, global_end)));
    return w;
}

// report_split_read_support (search_MEI.cpp:562-616)
void report_split_read_support(const std::vector<Chromosome> &genome, const std::map<int, std::string> &names, unsigned spacer,
                               Breakpoint &bp, bool fiveprime, std::ostream &out)
{
    std::vector<SimpleRead> &sr = bp.split_reads;
    if (sr.empty()) return;
    if (fiveprime) std::sort(sr.begin(), sr.end(), comp_mapsize);
    else std::sort(sr.rbegin(), sr.rend(), comp_unmapped_seqsize);
    const SimpleRead first = sr.front(), last = sr.back();
    const int base = fiveprime ? (int)first.mapped_sequence.length() : (int)last.unmapped_sequence.length();
    const int end = fiveprime ? (int)last.unmapped_sequence.length() : (int)first.mapped_sequence.length();
    const int offset = fiveprime ? 1 : 0;
    const std::string &chr_name = names.at(bp.tid);
    std::string reference;
    for (const Chromosome &c : genome)                    // get_fasta_subseq
        if (c.name == chr_name) {
            reference = c.seq.substr((size_t)(bp.pos - base + offset + (int)spacer), (size_t)(base + end));
            break;
        }
    int counter = 0;
    for (char &ch : reference) {                         // set_reference_highlight
        ch = ((fiveprime && counter < base) || (!fiveprime && counter >= base)) ? (char)std::toupper((unsigned char)ch)
                                                                               : (char)std::tolower((unsigned char)ch);
        counter++;
    }
    const std::string REFERENCE_PREFIX = "Reference: ";
    out << COMMENT_PREFIX << REFERENCE_PREFIX << reference << "\n";
    for (const SimpleRead &r : sr) {
        int indent = (int)REFERENCE_PREFIX.length();
        indent += fiveprime ? base - (int)r.mapped_sequence.length() : base - (int)r.unmapped_sequence.length();
        out << COMMENT_PREFIX << std::string((size_t)(unsigned)indent, ' ');
        if (fiveprime) out << r.mapped_sequence << r.unmapped_sequence;
        else out << r.unmapped_sequence << r.mapped_sequence;
        out << " (name: " << r.name << " sample: " << r.sample_name << ") " << "\n";
    }
}

// reportMEIevent (search_MEI.cpp:620-673) with set_evidence_strands, get_event_supporting_reads, report_supporting_reads
void report_event(const std::vector<Chromosome> &genome, const std::map<int, std::string> &names, unsigned spacer, Event &ev, size_t number,
                  std::ostream &out)
{
    for (SimpleRead &r : ev.fwd.reads) r.evidence_strand = PLUS;
    for (SimpleRead &r : ev.fwd.split_reads) r.evidence_strand = PLUS;
    for (SimpleRead &r : ev.fwd_mapping) r.evidence_strand = PLUS;
    for (SimpleRead &r : ev.rev.reads) r.evidence_strand = MINUS;
    for (SimpleRead &r : ev.rev.split_reads) r.evidence_strand = MINUS;
    for (SimpleRead &r : ev.rev_mapping) r.evidence_strand = MINUS;
    std::vector<SimpleRead> all;
    all.insert(all.end(), ev.fwd_mapping.begin(), ev.fwd_mapping.end());
    all.insert(all.end(), ev.fwd.split_reads.begin(), ev.fwd.split_reads.end());
    all.insert(all.end(), ev.rev_mapping.begin(), ev.rev_mapping.end());
    all.insert(all.end(), ev.rev.split_reads.begin(), ev.rev.split_reads.end());
    std::vector<SimpleRead> assoc = ev.fwd.reads;
    assoc.insert(assoc.end(), ev.rev.reads.begin(), ev.rev.reads.end());
    for (SimpleRead read : assoc) {
        const std::string rn = base_read_name(read.name);
        bool added = false;
        for (const SimpleRead &s : all)
            if (rn == base_read_name(s.name)) {
                added = true;
                break;
            }
        if (added) continue;
        std::swap(read.pos, read.mate_pos);
        std::swap(read.tid, read.mate_tid);
        std::swap(read.strand, read.mate_strand);
        read.sequence = "?";
        all.push_back(read);
    }
    const size_t n_all = ev.fwd.reads.size() + ev.fwd.split_reads.size() + ev.rev.reads.size() + ev.rev.split_reads.size();
    const std::string &chr = names.at(ev.fwd.tid);
    out << "####################################################################################################" << "\n";
    out << number << "\t" << "DD" << "\t" << chr << "\t" << ev.fwd.pos << "\t" << ev.rev.pos;
    out << "\t" << n_all << "\t" << ev.fwd.reads.size() << "\t" << ev.fwd.split_reads.size();
    out << "\t" << ev.rev.reads.size() << "\t" << ev.rev.split_reads.size() << "\n";
    out << COMMENT_PREFIX << "Dispersed Duplication insertion (DD) found on chromosome '" << chr << "', breakpoint at " << ev.fwd.pos
        << " (estimated from + strand), " << ev.rev.pos << " (estimated from - strand)" << "\n";
    out << COMMENT_PREFIX << "Found " << n_all << " supporting reads, of which " << ev.fwd.reads.size() << " discordant reads and "
        << ev.fwd.split_reads.size() << " split reads at 5' end, " << ev.rev.reads.size() << " discordant reads and "
        << ev.rev.split_reads.size() << " split reads at 3' end." << "\n";
    out << COMMENT_PREFIX << "Supporting reads for insertion location (5' end):" << "\n";
    report_split_read_support(genome, names, spacer, ev.fwd, true, out);
    out << COMMENT_PREFIX << "Supporting reads for insertion location (3' end):" << "\n";
    report_split_read_support(genome, names, spacer, ev.rev, false, out);
    out << "# All supporting sequences for this insertion (i.e. sequences that map inside the inserted element):" << "\n";
    std::sort(all.begin(), all.end(), comp_simple_read_pos);
    for (const SimpleRead &r : all) {
        if (r.is_split)
            out << "?\t?\t?\t" << r.name << "\t" << r.sample_name << "\t" << r.evidence_strand << "\t" << r.unmapped_sequence << "\n";
        else
            out << names.at(r.tid) << "\t" << r.pos << "\t" << r.strand << "\t" << r.name << "\t" << r.sample_name << "\t" << r.evidence_strand
                << "\t" << r.sequence << "\n";
    }
}

}  // namespace

bool dd_cands_text(unsigned spacer, const std::vector<std::string> &names, const std::string &sample, const uint8_t *seq, const uint64_t *seq_off,
                   const uint8_t *strand, uint32_t n_reads, uint32_t n_seg, const DDTables &tables, std::string &out)
{
    DDStats stats;
    DDState st;
    st.genome = nullptr;
    st.bams = nullptr;
    st.files = nullptr;
    st.stats = &stats;
    st.sample_tags.insert(sample);
    IngestedReads in;
    in.clear();
    if (n_reads) {
        in.batch.off.assign(seq_off, seq_off + n_reads + 1);
        in.batch.seq.assign(seq, seq + seq_off[n_reads]);
        in.batch.strand.assign(strand, strand + n_reads);
    }
    in.names = names;
    in.read_groups.assign(n_reads, std::string());
    std::vector<size_t> big(n_seg);
    for (uint32_t b = 0; b < n_seg; b++) big[b] = b;
    std::vector<std::vector<Cand>> cands;
    if (!cands_from_tables(st, tables, in, big, spacer, cands)) return false;
    out.clear();
    for (uint32_t b = 0; b < n_seg; b++)
        for (const Cand &c : cands[b]) {
            out += "C\t" + std::to_string(b) + "\t" + std::to_string(c.bio_bp) + "\t" + (c.tested ? "1" : "0") + "\t" + (c.contained ? "1" : "0") + "\t" +
                   c.consensus + "\n";
            for (const SimpleRead &r : c.split_reads)
                out += "R\t" + r.name + "\t" + r.sample_name + "\t" + r.sequence + "\t" + r.mapped_sequence + "\t" + r.unmapped_sequence + "\n";
        }
    return true;
}

int run_dd(const std::vector<Chromosome> &genome, const std::vector<unsigned> &sizes, const std::vector<RegionRecord> &plan,
           const std::vector<BamSource> &bams, const BamIngestSettings &ingest, double window_mbp, const DDSettings &dd,
           const std::string &prefix, const DDCloseFn &close_fn, const DDContainsFn &contains_fn, std::string &err, DDStats *stats,
           const DDTablesFn &tables_fn)
{
    const unsigned spacer = ingest.spacer;
    DDStats local;
    if (!stats) stats = &local;
    std::ofstream out((prefix + "_DD").c_str(), std::ios::trunc);
    if (!out) {
        err = "cannot write " + prefix + "_DD";
        return -1;
    }
    const unsigned WINDOW = (unsigned)(window_mbp * 1000000);
    std::vector<BamFile> files(bams.size());
    for (size_t k = 0; k < bams.size(); k++)
        if (!files[k].open(bams[k].path, err)) return -1;
    DDState st;
    st.genome = &genome;
    st.bams = &bams;
    st.files = &files;
    st.stats = stats;
    for (const BamSource &b : bams) st.sample_tags.insert(b.tag);
    // searchMEImain's loop over the plan's records and their windows
    for (const RegionRecord &rec : plan) {
        const Chromosome &chrom = genome[(size_t)rec.chr];
        const unsigned biol = (unsigned)(chrom.seq.size() - 2 * spacer);
        for (const auto &w : record_windows(rec, biol, WINDOW)) {
            std::vector<SimpleRead> disc;
            if (!load_discordant(st, dd, chrom.name, w.first, w.second, disc, err)) return -1;
            stats->discordant += disc.size();
            const int rc = window_breakpoints(st, dd, rec.chr, disc, ingest, close_fn, contains_fn, tables_fn, err);
            if (rc) return rc;
        }
    }
    stats->breakpoints = st.breakpoints.size();
    // get_sequence_name_dictionary: the targets of the first BAM
    std::map<int, std::string> names;
    if (!files.empty())
        for (size_t t = 0; t < files[0].header().names.size(); t++) names.insert(std::make_pair((int)t, files[0].header().names[t]));
    // searchMEI (search_MEI.cpp:891-940)
    std::vector<Breakpoint> &bps = st.breakpoints;
    if (bps.empty()) {
        // (the reference reads breakpoints.at(0 - 1) here and ends with std::out_of_range)
        stats->note = "no dispersed-duplication breakpoint found; " + prefix + "_DD is empty";
        return 0;
    }
    std::sort(bps.begin(), bps.end(), comp_breakpoint_pos);
    std::vector<Event> events;
    for (size_t i = 0; i + 1 < bps.size(); i++) {
        if (bps[i].strand == bps[i + 1].strand || (bps[i + 1].pos - bps[i].pos) > dd.max_bp_distance || bps[i].tid != bps[i + 1].tid) continue;
        Event e;
        if (bps[i].strand == PLUS) {
            e.fwd = bps[i];
            e.rev = bps[i + 1];
        } else {
            e.fwd = bps[i + 1];
            e.rev = bps[i];
        }
        events.push_back(e);
    }
    stats->events = events.size();
    if (dd.report_dup_reads && !events.empty()) {
        // append_cluster_connections (search_MEI.cpp:773-888): every chromosome whole, 1..size, in the reference's windows
        std::map<std::string, size_t> fwd_links, rev_links, exclude;
        for (size_t i = 0; i < events.size(); i++) {
            for (const SimpleRead &r : events[i].fwd.reads) {
                fwd_links.insert(std::make_pair(base_read_name(r.name), i));
                exclude.insert(std::make_pair(r.name, i));
            }
            for (const SimpleRead &r : events[i].rev.reads) {
                rev_links.insert(std::make_pair(base_read_name(r.name), i));
                exclude.insert(std::make_pair(r.name, i));
            }
        }
        for (size_t c = 0; c < genome.size(); c++) {
            RegionRecord whole;
            whole.chr = (int)c;
            whole.start = 1;
            whole.end = sizes[c];
            const unsigned biol = (unsigned)(genome[c].seq.size() - 2 * spacer);
            for (const auto &w : record_windows(whole, biol, WINDOW)) {
                std::vector<SimpleRead> disc;
                if (!load_discordant(st, dd, genome[c].name, w.first, w.second, disc, err)) return -1;
                for (const SimpleRead &r : disc) {
                    const std::string bn = base_read_name(r.name);
                    int idx = -1;
                    char strand = PLUS;
                    auto m = fwd_links.find(bn);
                    if (m != fwd_links.end()) idx = (int)m->second;
                    else if ((m = rev_links.find(bn)) != rev_links.end()) {
                        idx = (int)m->second;
                        strand = MINUS;
                    }
                    if (idx < 0 || exclude.find(r.name) != exclude.end()) continue;
                    (strand == PLUS ? events[(size_t)idx].fwd_mapping : events[(size_t)idx].rev_mapping).push_back(r);
                }
            }
        }
    }
    for (size_t i = 0; i < events.size(); i++) report_event(genome, names, spacer, events[i], i + 1, out);
    out.close();
    if (!out) {
        err = "cannot write " + prefix + "_DD";
        return -1;
    }
    return 0;
}

}  // namespace pgh
