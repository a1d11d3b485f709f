"""`--repair` on the host: hostlib.call_from_points(repairs=...), region_plan(bed_zero_based=...),
region_depth / depth_ratio(min_mapq=...) against the independent restatements of tests/repair_restated.py, on the -I sample of
tests/interchr_synth.py, on random read sets, and on the two-sample synthetic of tests/repair_synth.py.  Points come from
the CPU oracle (or are made up, for the random read sets: the _INT reporter reads lengths and positions only)."""
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import pyoracle
from pindel_amd import binding, hostio, hostlib
from tests import bam_writer as bw
from tests import germline_synth as gs
from tests import golden_util as gu
from tests import interchr_common as ic
from tests import interchr_restated as ir
from tests import interchr_synth as syn
from tests import repair_restated as rr
from tests import repair_synth as rs
from tests import test_depth_cpu as tdc
from tests import test_interchr_cpu as tic

SPACER = ic.SPACER


# ------------------------------------------------------------------------------------------------ int-pairs
def parse_int(text):
    """_INT lines -> (chr, pos, far chr, far pos, support)"""
    return [(c[1], c[2], c[3], c[4], c[6]) for c in tic._parse_int(text)]


def assert_every_junction_is_called(int_text):
    """a call with support >= 2 at each planted junction of the sample, seen from the chromosome left of it (the anchors of
    half its split reads) -- for all three chromosome pairs"""
    calls = parse_int(int_text)
    near = lambda a, b: abs(a - b) <= 3                      # (AbsLoc is the last matched base; see check_sample_reports)
    for lc, p, nt, rc, q in syn.junctions():
        a, b = syn.NAMES[lc], syn.NAMES[rc]
        assert any(n >= 2 and ((c1 == a and near(p1, p) and c2 == b and near(p2, q)) or (c1 == b and near(p1, q) and c2 == a and near(p2, p)))
                   for c1, p1, c2, p2, n in calls), (a, p, b, q, calls)
    assert {frozenset((c[0], c[2])) for c in calls} == {frozenset(x) for x in (("chrA", "chrB"), ("chrB", "chrC"), ("chrA", "chrC"))}


def test_int_pairs_reports_every_chromosome_pair(tmp_path):
    s = syn.make(str(tmp_path))
    csr, per_window = tic._text_route_expected(s, tmp_path)
    want = [rr.int_lines_all_pairs(reads, SPACER) for _, _, reads in per_window]
    want_int = "".join(t for t, _ in want)
    st = hostlib.default_settings(pyoracle.max_mismatch_table())
    st.window_mbp = float(syn.WINDOW_MBP)
    st.report_interchromosomal = 1
    on, off = str(tmp_path / "repaired"), str(tmp_path / "as_is")
    hostlib.call_from_points(s["fasta"], s["reads_txt"], on, st, *csr, repairs="int-pairs")
    hostlib.call_from_points(s["fasta"], s["reads_txt"], off, st, *csr)
    got = open(on + "_INT").read()
    assert got == want_int
    assert open(on + "_INT_final").read() == ir.int_final(want_int)          # _INT_final changes only through _INT
    assert_every_junction_is_called(got)
    # as it stands only chrA / chrB is ever printed from a window that touches chrB
    plain = open(off + "_INT").read()
    assert plain == "".join(ir.int_lines(reads, SPACER)[0] for _, _, reads in per_window)
    assert not any({c[0], c[2]} == {"chrB", "chrC"} for c in parse_int(plain))
    # Window by window the unrepaired lines are the first lines of the repaired ones.  Both files equal the concatenation of
    # their restatement's windows (asserted above), so the property is checked on those; some window gains lines.
    grew = 0
    for (_, _, reads), (text, first_pair) in zip(per_window, want):
        old = ir.int_lines(reads, SPACER)[0]
        assert text.startswith(old) and old == first_pair
        grew += text != old
    assert grew >= 2
    # the other reports do not change, and the field of the settings does what the keyword does
    for suf in gu.SUFFIXES:
        assert open(f"{on}_{suf}", "rb").read() == open(f"{off}_{suf}", "rb").read(), suf
    st.repairs = hostlib.REPAIRS["int-pairs"]
    hostlib.call_from_points(s["fasta"], s["reads_txt"], str(tmp_path / "field"), st, *csr)
    assert open(tmp_path / "field_INT").read() == want_int


RANDOM_NAMES = ("chrT", "chrB", "chrM", "chrA")             # FASTA order is not name order
RANDOM_LEN = 2000
RANDOM_SPACER = 200                                         # (a small one: the cost of a call grows with the padded length)


def _random_read_set(rng):
    """1-40 reads on four small chromosomes, every one with its far end on another chromosome (so no classifier takes it) and
    1-3 made-up points per end.  The reads are drawn from 1-5 junctions, so calls do repeat: a junction fixes the anchor's
    chromosome and strand, the far chromosome and strand, the sequence and the points, half of them with a pair of points
    that adds up to the read length (the others give a call with non-template bases, or none).  A read now and then differs
    from its junction in one point.  Names repeat, also across junctions.
    -> (Pindel-text lines, CSR arrays, the restatement's read lists per chromosome in FASTA order)"""
    at = lambda: RANDOM_SPACER + rng.randint(100, RANDOM_LEN - 100)
    junctions = []
    for _ in range(rng.randint(1, 5)):
        L = rng.choice([60, 80, 100])
        c = rng.randrange(4)
        far_c = rng.choice([x for x in range(4) if x != c])
        close = [(rng.randint(8, L // 2), at(), c) for _ in range(rng.randint(1, 3))]
        far = [(rng.randint(8, L // 2), at(), far_c) for _ in range(rng.randint(1, 3))]
        if rng.random() < 0.5:
            far[rng.randrange(len(far))] = (L - rng.choice(close)[0], at(), far_c)
        junctions.append(dict(seq="".join(rng.choice("ACGT") for _ in range(L)), strand=rng.choice("+-"), chr=c, close=close, far=far,
                              far_strand=rng.choice("+-")))
    n = rng.randint(1, 40)
    reads = []
    for i in range(n):
        r = dict(rng.choice(junctions), name=f"@r{rng.randint(0, max(3, 2 * n // 3))}/1", pos=rng.randint(100, RANDOM_LEN - 100))
        if rng.random() < 0.15:
            which = rng.choice(["close", "far"])
            pts = list(r[which])
            k = rng.randrange(len(pts))
            pts[k] = (pts[k][0], at(), pts[k][2])
            r[which] = pts
        reads.append(r)
    reads.sort(key=lambda r: r["chr"])                      # (stable: per chromosome in the order drawn)
    text = "".join(f'{r["name"]}\n{r["seq"]}\n{r["strand"]}\t{RANDOM_NAMES[r["chr"]]}\t{r["pos"]}\t60\t300\tT\n' for r in reads)
    cp = np.zeros(sum(len(r["close"]) for r in reads), dtype=pyoracle.POINT_DTYPE)
    fp = np.zeros(sum(len(r["far"]) for r in reads), dtype=pyoracle.POINT_DTYPE)
    co, fo = [0], [0]
    for r in reads:
        for arr, off, pts, strand in ((cp, co, r["close"], r["strand"]), (fp, fo, r["far"], r["far_strand"])):
            for k, (length, loc, chrom) in enumerate(pts):
                arr[off[-1] + k] = (loc, length, 0, chrom, b"+", strand.encode())
            off.append(off[-1] + len(pts))
    csr = (np.array(co, dtype=np.uint64), cp, np.array(fo, dtype=np.uint64), fp, np.zeros(len(reads), dtype=np.uint8))
    windows = []
    for c in range(4):                                       # one window per chromosome, its reads in input order
        mine = [r for r in reads if r["chr"] == c]
        windows.append([dict(Name=r["name"], FragName=RANDOM_NAMES[c], FarFragName=RANDOM_NAMES[r["far"][0][2]], MatchedD=r["strand"],
                             MatchedFarD=r["far_strand"], ReadLength=len(r["seq"]), UnmatchedSeq=r["seq"],
                             UP_Close=[(p[0], p[1]) for p in r["close"]], UP_Far=[(p[0], p[1]) for p in r["far"]]) for r in mine])
    return text, csr, windows


def test_int_pairs_on_random_read_sets(tmp_path):
    rng = random.Random(4321)
    fasta = tmp_path / "four.fa"
    with open(fasta, "w") as fh:
        for name in RANDOM_NAMES:
            fh.write(f">{name}\n" + "".join(rng.choice("ACGT") for _ in range(RANDOM_LEN)) + "\n")
    st = hostlib.default_settings(pyoracle.max_mismatch_table())
    st.report_interchromosomal = 1
    st.spacer = RANDOM_SPACER
    n_lines = n_later_pairs = n_repeated = n_nt = n_first_differs = 0
    for case in range(200):
        text, csr, windows = _random_read_set(rng)
        reads_txt = tmp_path / "reads.txt"
        reads_txt.write_text(text)
        want = [rr.int_lines_all_pairs(w, RANDOM_SPACER) for w in windows]
        as_is = [ir.int_lines(w, RANDOM_SPACER)[0] for w in windows]
        # every set with the repair; every fifth also without it (test_interchr_cpu.py has no random read sets)
        for repairs, expect in (("int-pairs", "".join(t for t, _ in want)), (None, "".join(as_is)))[:2 if case % 5 == 0 else 1]:
            prefix = str(tmp_path / "r")
            hostlib.call_from_points(str(fasta), str(reads_txt), prefix, st, *csr, repairs=repairs)
            assert open(prefix + "_INT").read() == expect, (case, repairs)
            assert open(prefix + "_INT_final").read() == ir.int_final(expect), (case, repairs)
        for w, (t, first), old in zip(windows, want, as_is):
            # (the unrepaired lines need not come first here: a name shared with an earlier read of ANOTHER pair is taken
            # without the repair and free with it, so the first pair's own counts can grow)
            assert t.startswith(first), case
            n_first_differs += first != old
            n_later_pairs += t != first
            n_repeated += len({r["Name"] for r in w}) < len(w)
            n_nt += sum(1 for line in t.splitlines() if '""' not in line)
        n_lines += sum(t.count("\n") for t, _ in want)
    # the sets do exercise the reporter: lines, lines of later pairs, calls with non-template bases, repeated names
    counts = (n_lines, n_later_pairs, n_nt, n_repeated, n_first_differs)
    assert n_lines >= 200 and n_later_pairs >= 50 and n_nt >= 20 and n_repeated >= 100 and n_first_differs >= 5, counts


# ------------------------------------------------------------------------------------------------ inv-pairs, depth-mapq
SUFFIXES = ("D", "SI", "TD", "INV", "LI")


def full_counts(pairs, rs_, re_):
    """CountLeft, CountRight over the whole list (a cutoff no count reaches: the loop never leaves early)"""
    _, left, right = rr.is_good_inv(pairs, 1 << 30, rs_, re_)
    return left, right


def check_fixture(s, plain):
    """Conditions on the fixture, by the restatements alone: the planted counts, none within one of its cutoff but the edge
    case; the edge case decided by the last pair of the list; the planted depth ratios far from 2.7 both ways."""
    pairs = rr.pair_state([s["records"][t] for t in rs.TAGS], [rs.ISZ] * len(rs.TAGS), 0, 0, rs.CHR_LEN)
    assert len(pairs) == sum(a + b for a, b in rs.ENTRIES.values())
    by_name = {rs.planted(b): b for b in rs.blocks(plain["INV"])}
    assert list(by_name) == ["INV_edge", "INV_both", "INV_one", "INV_s"]
    verdicts = {}
    for name in rs.LARGE_INV:
        support, start, end = rs.inv_event(by_name[name])
        assert end - start >= 2 * rs.READ and max(support // 2, 5) == rs.CUTOFF, (name, support)
        for ds in (-10, 0, 10):                              # ... and for breakpoints a few bases off
            for de in (-10, 0, 10):
                assert full_counts(pairs, start + ds, end + de) == rs.ENTRIES[name], (name, ds, de)
        for n in rs.ENTRIES[name]:
            assert abs(n - rs.CUTOFF) > 1 or name == "INV_edge"
        verdicts[name] = rr.is_good_inv(pairs, support, start, end)[0]
    assert verdicts == {"INV_edge": True, "INV_both": True, "INV_one": False}
    support, start, end = rs.inv_event(by_name["INV_edge"])
    assert rr.is_good_inv(pairs, support, start, end, after_loop=False)[0] is False        # the reference's loop alone drops it:
    assert rr.is_good_inv(pairs[-1:], 1 << 30, start, end)[1] == 1                         # the last pair of the list counts (left)
    assert rr.is_good_inv(pairs[:-1], support, start, end)[0] is False                     # ... and decides
    assert rs.inv_event(by_name["INV_s"])[2] - rs.inv_event(by_name["INV_s"])[1] < 2 * rs.READ
    # TD_q: S1's ratio is high with every record and low from MAPQ 20 on; S2's is low either way
    _, a, b = rs.EVENTS["TD_q"]
    for tag in rs.TAGS:
        for floor in (0, 20):
            depth = rr.depth_array_mapq(s["records"][tag], 0, rs.CHR_LEN, floor)
            ratios = [gs.ratio(depth, rs.CHR_LEN, a + i, b + j) for i in (-10, 0, 10) for j in (-10, 0, 10)]
            high = tag == "S1" and floor == 0
            assert all(r >= 3.2 for r in ratios) if high else all(r <= 2.2 for r in ratios), (tag, floor, ratios)
    for ev in rs.EVENTS:
        assert {t[7] for t in s["text"] if t[0].startswith("@" + ev + "_")} == set(rs.TAGS)


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    d = tmp_path_factory.mktemp("repair")
    s = rs.make(str(d))
    chroms = hostio.load_fasta(s["fasta"])
    b = hostio.read_pindel_text(s["reads_txt"], [n for n, _ in chroms], [len(q) - 200000 for _, q in chroms])
    p = pyoracle.make_params(max_range_index=rs.MAX_RANGE_INDEX)
    r = pyoracle.search_batch(p, [q for _, q in chroms], b.seq, b.seq_off, b.anchor_strand, b.anchor_pos, b.insert_size, b.chr_id)
    co, cp = gu.csr_from_strided(r["close_cnt"], r["close_pts"])
    fo, fp = gu.csr_from_strided(r["far_cnt"], r["far_pts"])
    s["points"] = (co, cp, fo, fp, r["rc_flag"])
    s["dir"] = d
    s["plain"] = run(s, "plain")
    check_fixture(s, s["plain"])
    return s


def run(s, name, **kw):
    st = hostlib.default_settings(pyoracle.max_mismatch_table())
    st.analyze_li = 1
    prefix = str(s["dir"] / name)
    hostlib.call_from_points(s["fasta"], s["reads_txt"], prefix, st, *s["points"], **kw)
    return {suf: open(f"{prefix}_{suf}", "rb").read() for suf in SUFFIXES}


def expected(plain, dropped):
    """the run without -N minus the dropped blocks, later event numbers lowered (the method of test_germline_cpu.py)"""
    out = dict(plain)
    out["TD"], out["INV"] = rs.without(plain["TD"], dropped), rs.without(plain["INV"], dropped)
    return out


# what -N drops of the planted events, per set of repairs
DROPPED = {None: rs.LARGE_INV, "inv-pairs": ("INV_one",), "depth-mapq": rs.LARGE_INV + ("TD_q",), "inv-pairs,depth-mapq": ("INV_one", "TD_q"),
           "all": ("INV_one", "TD_q")}


@pytest.mark.parametrize("repairs", list(DROPPED), ids=lambda r: r or "none")
def test_normal_samples_with_repairs(sample, repairs):
    got = run(sample, "N_" + (repairs or "none").replace(",", "_"), normal_samples=True, bam_config=sample["config"], repairs=repairs)
    assert got == expected(sample["plain"], DROPPED[repairs])
    kept = [rs.planted(b) for b in rs.blocks(got["INV"])]
    assert kept == [e for e in ("INV_edge", "INV_both", "INV_one", "INV_s") if e not in DROPPED[repairs]]


def test_the_names_do_nothing_without_n_or_on_text_input(sample):
    assert run(sample, "no_N", bam_config=sample["config"], repairs="all") == sample["plain"]
    assert run(sample, "text", normal_samples=True, repairs="all") == sample["plain"]


def test_inv_pairs_does_not_depend_on_host_threads(sample, monkeypatch):
    outs = []
    for threads in ("1", "8"):
        monkeypatch.setenv("PGH_THREADS", threads)
        outs.append(run(sample, f"all_t{threads}", normal_samples=True, bam_config=sample["config"], repairs="all"))
    assert outs[0] == outs[1] == expected(sample["plain"], DROPPED["all"])


def test_region_depth_with_a_mapq_floor(tmp_path):
    """on the messy BAM of test_depth_cpu.py (MAPQ 0, 19, 20 and 60, every CIGAR operation and flag): == on the doubles"""
    recs = tdc._records()
    assert {r["mapq"] for r in recs if not r["flag"] & gs._SKIP} == {0, 19, 20, 60}
    bam = str(tmp_path / "messy.bam")
    bw.write_bam(bam, tdc.REFS, recs, block_bytes=4096)
    for floor in (0, 19, 20, 21, 60, 61):
        for tid, (name, size) in enumerate(tdc.REFS):
            depth = rr.depth_array_mapq(recs, tid, size, floor)
            if floor == 0:
                assert (depth == gs.depth_array(recs, tid, size)).all()
            for beg, end in tdc.REGIONS:
                want, got = gs.avg_depth(depth, beg, end), hostlib.region_depth(bam, name, beg, end, min_mapq=floor)
                assert got == want or (np.isnan(got) and np.isnan(want)), (floor, name, beg, end, got, want)
    d0, d20 = rr.depth_array_mapq(recs, 0, 5000, 0), rr.depth_array_mapq(recs, 0, 5000, 20)
    assert d20.sum() < d0.sum() and (rr.depth_array_mapq(recs, 0, 5000, 19) != d20).any()     # 19 is below the floor, 20 is not
    assert hostlib.region_depth(bam, "chr1", 0, 5000) == hostlib.region_depth(bam, "chr1", 0, 5000, min_mapq=0)
    for start, end in ((1000, 2000), (100, 163), (40, 300)):
        want = gs.ratio(d20, 5000, start, end)
        assert hostlib.depth_ratio([bam], "chr1", 5000, start, end, min_mapq=hostlib.DEPTH_MAPQ_FLOOR) == [want]
        assert hostlib.depth_ratio([bam], "chr1", 5000, start, end) == [gs.ratio(d0, 5000, start, end)]


# ------------------------------------------------------------------------------------------------ bed0
def test_bed0_shifts_the_start(tmp_path):
    rng = random.Random(3)
    fasta = tmp_path / "one.fa"
    fasta.write_text(">chr\n" + "".join(rng.choice("ACGT") for _ in range(1000)) + "\n")
    (tmp_path / "one.fa.fai").write_text("chr\t1000\t5\t1000\t1001\n")
    inc, exc = tmp_path / "inc.bed", tmp_path / "exc.bed"
    inc.write_text("chr 99 200\n")
    assert hostlib.region_plan(str(fasta), include_bed=str(inc)) == [("chr", 99, 200)]
    assert hostlib.region_plan(str(fasta), include_bed=str(inc), bed_zero_based=True) == [("chr", 100, 200)]
    # -J through CleanUpBedRecord: an exclude strictly inside cuts the record in two, [start, exclude start] and [exclude end, end]
    exc.write_text("chr 149 160\n")
    assert hostlib.region_plan(str(fasta), include_bed=str(inc), exclude_bed=str(exc)) == [("chr", 99, 149), ("chr", 160, 200)]
    assert hostlib.region_plan(str(fasta), include_bed=str(inc), exclude_bed=str(exc), bed_zero_based=True) == [("chr", 100, 150), ("chr", 160, 200)]
    # the shift comes before the clipping to -c and to the chromosome; a record without a base is left out; -c itself is unchanged
    inc.write_text("chr 0 50\nchr 300 300\nchr 900 2000\n")
    assert hostlib.region_plan(str(fasta), include_bed=str(inc), bed_zero_based=True) == [("chr", 1, 50), ("chr", 901, 1000)]
    assert hostlib.region_plan(str(fasta), region="chr:1-950", include_bed=str(inc), bed_zero_based=True) == [("chr", 1, 50), ("chr", 901, 950)]
    assert hostlib.region_plan(str(fasta), region="chr:99-200", bed_zero_based=True) == [("chr", 99, 200)]


# ------------------------------------------------------------------------------------------------ plumbing
def test_repairs_mask_and_layout():
    assert hostlib.repairs_mask(None) == 0 and hostlib.repairs_mask("all") == 15
    assert hostlib.repairs_mask("bed0,int-pairs") == hostlib.repairs_mask(["int-pairs", "bed0"]) == 9
    for bad in ("", "nonsense", "bed0,", "ALL"):
        with pytest.raises(ValueError):
            hostlib.repairs_mask(bad)
    # the new field is the last one: every earlier field keeps its offset
    assert hostlib.HostSettings._fields_[-1][0] == "repairs"
    assert hostlib.HostSettings.repairs.offset >= hostlib.HostSettings.pindel_config.offset + 8
    assert hostlib.default_settings(pyoracle.max_mismatch_table()).repairs == 0


@pytest.mark.parametrize("args", [["--repair", "nonsense"], ["--repair", ""], ["--repair"]], ids=["unknown", "empty", "missing"])
def test_command_line_rejects_a_bad_repair_list(tmp_path, args):
    exe = os.path.join(os.path.dirname(binding.LIB_PATH), "pindel_pg")
    fa, reads_txt = gu.unpack(tmp_path)
    prefix = tmp_path / "out" / "o"
    prefix.parent.mkdir()
    out = subprocess.run([exe, "-f", fa, "-p", reads_txt, "-o", str(prefix)] + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 2, (out.returncode, out.stderr)
    assert "--repair" in out.stderr and "pg_create" not in out.stderr
    assert os.listdir(prefix.parent) == []                   # before any file is created or truncated
