"""Region selection: `-c chr[:start[-end]]`, `-j include.bed` and `-J exclude.bed` (pindel_amd/csrc/host/pg_region.hpp).

  * The plan: hostlib.region_plan = a restatement here, written from the documented behaviour, for a table of cases, and
    the error cases raise.
  * The reports: call_from_points on the oracle's points for the sim1chrVs2 gold reads, with a plan, gives the gold event
    blocks whose left BP lies in each record, record by record, renumbered from 0 (the regions lie >= 2 kbp from every gold
    breakpoint); _LI follows tests/li_consumer.py record by record with the mask cleared; no dependence on host threads; a
    single chromosome of a two-chromosome set gives that chromosome's blocks of the whole-genome run.
  * The command line validates -c / -j / -J before it touches a device (exit 2 for syntax, 1 for files and chromosomes), and
    an empty plan writes empty reports and exits 0 -- all without a GPU.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pyoracle
from pindel_amd import hostio, hostlib
from tests import golden_util as gu
from tests import li_consumer as li
from tests.test_li_pin import _expected_on_the_text_route, _records
from tests.test_li_report import _li_reads, _oracle, _synthetic

BUFFER = 10000          # AROUND_REGION_BUFFER: a record's windows reach this far beyond it


# ------------------------------------------------------------------------------------------- the plan, restated
def _bed(path, rows):
    with open(path, "w") as f:
        for r in rows:
            f.write((r if isinstance(r, str) else "\t".join(str(x) for x in r)) + "\n")
    return str(path)


def _read_bed(path):
    out = []
    for line in open(path):
        f = line.split()
        if not f or f[0].startswith("#") or f[0] in ("track", "browser"):
            continue
        a, b = int(f[1]), int(f[2])
        out.append([f[0], min(a, b), max(a, b)])
    return out


def _exclude(records, excludes):
    """The reference's clean-up of the include list against the exclude list (pindel.cpp CleanUpBedRecord)."""
    if not excludes:
        return records
    recs = [list(r) for r in records]
    i = 0
    while i < len(recs):                                 # (pieces appended at the end are visited too)
        r = recs[i]
        for c, xs, xe in excludes:
            if r[1] == r[2]:
                break                                    # emptied: no further exclude looks at it
            if c != r[0] or r[1] > xe or xs > r[2]:
                continue
            if xs <= r[1] and r[2] <= xe:
                r[2] = r[1]                              # contained: emptied
            elif r[1] < xs and xe < r[2]:
                recs.append([r[0], xe, r[2]])            # strictly inside: the right piece goes last
                r[2] = xs
            elif xs <= r[1] < xe < r[2]:
                r[1] = xe                                # covers the left side
            elif r[1] < xs < r[2] < xe:
                r[2] = xs                                # covers the right side
        i += 1
    recs = [r for r in recs if r[1] != r[2]]
    for a in range(len(recs) - 1):                       # one merge pass, no repeat
        for b in range(a + 1, len(recs)):
            f, s = recs[a], recs[b]
            if f[0] != s[0] or f[1] > s[2] or s[1] > f[2]:
                continue
            if s[1] <= f[1] and f[2] <= s[2]:
                f[2] = f[1]
                break
            if f[1] <= s[1] and s[2] <= f[2]:
                s[1] = s[2]
                break
            if s[1] <= f[1] <= s[2] <= f[2]:
                f[1], s[1] = s[1], s[2]
            elif f[1] <= s[1] <= f[2] <= s[2]:
                f[2], s[1] = s[2], s[2]
    return [r for r in recs if r[1] != r[2]]


def _sort_like_the_reference(recs, order):
    """the reference's exchange sort by (chromosome index, start): swaps on a strictly smaller key only"""
    recs = list(recs)
    key = lambda r: (order[r[0]], r[1])
    for a in range(len(recs) - 1):
        for b in range(a + 1, len(recs)):
            if key(recs[b]) < key(recs[a]):
                recs[a], recs[b] = recs[b], recs[a]
    return recs


def restated_plan(sizes, region=None, include=None, exclude=None):
    """sizes: [(name, size)] in reference order"""
    size = dict(sizes)
    order = {n: k for k, (n, _) in enumerate(sizes)}
    target = None
    if region and region != "ALL":
        name, _, coords = region.partition(":")
        if name not in size:
            raise ValueError("unknown chromosome")
        start, end = 1, size[name]
        if coords:
            coords = coords.replace(",", "")
            s, dash, e = coords.partition("-")
            if not s.isdigit() or (dash and not e.isdigit()):
                raise ValueError("syntax")
            start = int(s)
            if dash:
                if int(e) < start:
                    raise ValueError("end before start")
                end = min(int(e), size[name])
        if start > size[name]:
            raise ValueError("start beyond the chromosome")
        target = (name, start, end)
    if include is None:
        recs = [[n, 1, s] for n, s in sizes] if target is None else [list(target)]
    else:
        recs = []
        for c, s, e in _read_bed(include):
            if c not in size:
                raise ValueError("unknown chromosome in the BED file")
            if target is None:
                recs.append([c, s, min(e, size[c])])
            elif c == target[0] and not (s > target[2] or target[1] > e):
                recs.append([c, max(s, target[1]), min(e, target[2])])
    if exclude is not None:
        ex = [x for x in _read_bed(exclude) if x[0] in size]
        if ex:
            recs = _sort_like_the_reference(_exclude(recs, ex), order)
    return [tuple(r) for r in recs]


@pytest.fixture(scope="module")
def gold(tmp_path_factory):
    """the sim1chrVs2 reference and reads with the oracle's points (one 200-kbp chromosome "1")"""
    tmp = tmp_path_factory.mktemp("gold")
    fa, reads_txt = gu.unpack(tmp)
    chroms = hostio.load_fasta(fa)
    batch = hostio.read_pindel_text(reads_txt, [n for n, _ in chroms], [len(s) - 200000 for _, s in chroms])
    return fa, reads_txt, chroms, _oracle(chroms, batch)


@pytest.fixture(scope="module")
def two_chr(tmp_path_factory):
    """a reference with chromosomes A (50 kbp) and B (80 kbp), no .fai: the sizes are the FASTA lengths"""
    d = tmp_path_factory.mktemp("two")
    fa = str(d / "two.fa")
    with open(fa, "w") as f:
        for name, n in (("A", 50000), ("B", 80000)):
            seq = ("ACGTTGCA" * (n // 8 + 1))[:n]
            f.write(f">{name} some description\n")
            for i in range(0, n, 70):
                f.write(seq[i:i + 70] + "\n")
    # (the loader gives the last chromosome one base more: the reference's end-of-file quirk, tests/test_mei_bam.py)
    sizes = [(n, len(x) - 200000) for n, x in hostio.load_fasta(fa)]
    assert sizes == [("A", 50000), ("B", 80001)]
    return fa, sizes


def _plan_cases(d):
    b = lambda name, rows: _bed(d / name, rows)
    one = [("1", 200000)]
    return [
        (one, dict(region="ALL")), (one, dict(region="1")), (one, dict(region="1:1")), (one, dict(region="1:5,000")),
        (one, dict(region="1:5,000-60,000")), (one, dict(region="1:150000-999999")), (one, dict()),
        # swapped coordinates, an end beyond the chromosome, comments and a track line, extra columns
        (one, dict(include=b("swap.bed", ["# comment", "track name=x", "", ("1", 60000, 50000, "name", 0, "+"), ("1", 190000, 250000)]))),
        # -c region + -j: only the overlapping records, clipped to the region
        (one, dict(region="1:40,000-100,000", include=b("clip.bed", [("1", 10000, 20000), ("1", 30000, 50000), ("1", 60000, 70000),
                                                                     ("1", 90000, 120000), ("1", 100000, 110000)]))),
        # overlapping include records: as given without -J; merged (one pass, then sorted) with -J
        (one, dict(include=b("ovl.bed", [("1", 50000, 80000), ("1", 10000, 20000), ("1", 70000, 90000), ("1", 15000, 18000),
                                         ("1", 5000, 12000), ("1", 90000, 95000)]))),
        (one, dict(include=d / "ovl.bed", exclude=b("far.bed", [("1", 199000, 199500), ("2", 1, 100)]))),
        # an exclude strictly inside the first record: its right piece is appended last, then the list is sorted
        (one, dict(include=b("two.bed", [("1", 10000, 50000), ("1", 100000, 150000)]), exclude=b("mid.bed", [("1", 20000, 30000)]))),
        # an exclude containing a record; ones covering one side; ones touching a border
        (one, dict(include=b("three.bed", [("1", 10000, 20000), ("1", 30000, 40000), ("1", 60000, 70000), ("1", 80000, 90000)]),
                   exclude=b("sides.bed", [("1", 5000, 25000), ("1", 25000, 35000), ("1", 65000, 75000), ("1", 90000, 95000),
                                           ("1", 79000, 80000)]))),
        (one, dict(region="1", exclude=b("split2.bed", [("1", 150000, 160000), ("1", 30000, 40000)]))),
        # everything excluded: an empty plan
        (one, dict(region="1:100-5000", exclude=b("all.bed", [("1", 1, 200000)]))),
        (one, dict(include=d / "two.bed", exclude=d / "all.bed")),
    ]


def test_plan_equals_restatement(gold, tmp_path):
    fa = gold[0]
    for sizes, kw in _plan_cases(tmp_path):
        kw = {k: (str(v) if v is not None else None) for k, v in kw.items()}
        want = restated_plan(sizes, kw.get("region"), kw.get("include"), kw.get("exclude"))
        got = hostlib.region_plan(fa, kw.get("region"), kw.get("include"), kw.get("exclude"))
        assert got == want, kw
    # a few fixed points of the table, spelled out
    assert hostlib.region_plan(fa, "1:5,000-60,000") == [("1", 5000, 60000)]
    assert hostlib.region_plan(fa, "1:5,000") == [("1", 5000, 200000)]
    assert hostlib.region_plan(fa, include_bed=str(tmp_path / "swap.bed")) == [("1", 50000, 60000), ("1", 190000, 200000)]
    assert hostlib.region_plan(fa, include_bed=str(tmp_path / "two.bed"), exclude_bed=str(tmp_path / "mid.bed")) == [
        ("1", 10000, 20000), ("1", 30000, 50000), ("1", 100000, 150000)]
    assert hostlib.region_plan(fa, "1:100-5000", exclude_bed=str(tmp_path / "all.bed")) == []


def test_plan_two_chromosomes_and_fasta_sizes(two_chr, tmp_path):
    """without a .fai the FASTA lengths are the sizes; ALL is one record per chromosome in reference order; an exclude
    list sorts by the reference's chromosome order"""
    fa, sizes = two_chr
    assert hostlib.region_plan(fa) == [("A", 1, 50000), ("B", 1, 80001)]
    inc = _bed(tmp_path / "i.bed", [("B", 5000, 9000), ("A", 100, 900000), ("B", 1000, 2000)])
    exc = _bed(tmp_path / "x.bed", [("A", 200, 300), ("C", 1, 5)])
    for kw in (dict(include=inc), dict(include=inc, exclude=exc), dict(region="B:1,500", include=inc, exclude=exc),
               dict(region="A", exclude=exc)):
        want = restated_plan(sizes, kw.get("region"), kw.get("include"), kw.get("exclude"))
        assert hostlib.region_plan(fa, kw.get("region"), kw.get("include"), kw.get("exclude")) == want, kw
    assert hostlib.region_plan(fa, include_bed=inc, exclude_bed=exc) == [("A", 100, 200), ("A", 300, 50000), ("B", 1000, 2000),
                                                                       ("B", 5000, 9000)]


@pytest.mark.parametrize("kw", [
    dict(region="1:60-50"), dict(region="X"), dict(region="1:300000"), dict(region="1:abc"), dict(region="1:5,000-"),
    dict(region="1:-5"), dict(include="bad"), dict(include="unknown_chr"), dict(include="missing"), dict(exclude="bad"),
])
def test_plan_errors_raise(gold, tmp_path, kw):
    fa = gold[0]
    files = {"bad": _bed(tmp_path / "bad.bed", [("1", 10, 20), "1\t30", ("1", 40, 50)]),
             "unknown_chr": _bed(tmp_path / "unk.bed", [("1", 10, 20), ("X", 1, 100)]),
             "missing": str(tmp_path / "nope.bed")}
    args = {k: files.get(v, v) for k, v in kw.items()}
    with pytest.raises(ValueError) as e:
        hostlib.region_plan(fa, args.get("region"), args.get("include"), args.get("exclude"))
    if "bad" in kw.values():
        assert "line 2" in str(e.value)
    if "region" in kw:
        with pytest.raises(ValueError):
            restated_plan([("1", 200000)], kw["region"])


# ------------------------------------------------------------------------------------------- reports from a plan
def blocks(data: bytes):
    """event blocks of a report file: (left BP, bytes from its '####' line up to the next)"""
    out, cur = [], None
    for line in data.split(b"\n")[:-1] if data.endswith(b"\n") else data.split(b"\n"):
        if line.startswith(b"####"):
            cur = [line]
            out.append(cur)
        elif cur is not None:
            cur.append(line)
        else:
            assert not line, line
    res = []
    for b in out:
        m = re.search(rb"\tBP (\d+)\t", b[1])
        res.append((int(m.group(1)) if m else None, b"\n".join(b) + b"\n"))
    return res


def renumber(bl):
    """the blocks with their index field set to 0, 1, ... in order"""
    out = b""
    for k, b in enumerate(bl):
        head, first, rest = b.split(b"\n", 2)
        out += head + b"\n" + b"%d" % k + first[first.index(b"\t"):] + b"\n" + rest
    return out


def gold_bytes(suffix):
    import gzip
    return gzip.open(os.path.join(gu.GOLD, f"simulated_test.out_{suffix}.gz")).read()


def expected_from_gold(plan, suffix):
    """the rule: per plan record, in order, the gold blocks whose left BP lies in [S, E], in gold order; renumbered"""
    gb = blocks(gold_bytes(suffix))
    return renumber([b for _, s, e in plan for bp, b in gb if s <= bp <= e])


def _call(gold, prefix, threads=None, li_on=False, cem_on=False, window_mbp=5.0, **region):
    fa, reads_txt, chroms, r = gold
    co, cp = gu.csr_from_strided(r["close_cnt"], r["close_pts"])
    fo, fp = gu.csr_from_strided(r["far_cnt"], r["far_pts"])
    st = hostlib.default_settings(pyoracle.max_mismatch_table())
    st.analyze_li, st.report_close_mapped, st.window_mbp = int(li_on), int(cem_on), window_mbp
    hostlib.call_from_points(fa, reads_txt, prefix, st, co, cp, fo, fp, r["rc_flag"], **region)
    return {s: open(f"{prefix}_{s}", "rb").read() for s in gu.SUFFIXES + (("LI",) if li_on else ()) + (("CloseEndMapped",) if cem_on else ())}


def _assert_same(got: bytes, want: bytes, what):
    g, w = gu.normalise(got), gu.normalise(want)
    assert len(g) == len(w), f"{what}: {len(g)} lines, expected {len(w)}"
    for i, (a, b) in enumerate(zip(g, w)):
        assert a == b, f"{what} line {i + 1}:\n got  {a[:200]!r}\n want {b[:200]!r}"


def report_cases(d):
    """(name, call_from_points region keywords) of the gold-derived cases"""
    b = lambda name, rows: _bed(d / name, rows)
    return [
        ("c1", dict(region="1")),
        ("c1_1", dict(region="1:1")),
        ("j_whole", dict(include_bed=b("whole.bed", [("1", 1, 200000)]))),
        ("J_empty_middle", dict(exclude_bed=b("x150.bed", [("1", 150000, 160000)]))),
        ("c_25_45", dict(region="1:25,000-45,000")),
        ("j_three", dict(include_bed=b("three.bed", [("1", 25000, 45000), ("1", 55000, 65000), ("1", 95000, 125000)]))),
        ("j_reversed", dict(include_bed=b("rev.bed", [("1", 95000, 125000), ("1", 25000, 45000)]))),
        ("J_55_65", dict(exclude_bed=b("x55.bed", [("1", 55000, 65000)]))),
    ]


def _plan_of(gold, kw):
    return hostlib.region_plan(gold[0], kw.get("region"), kw.get("include_bed"), kw.get("exclude_bed"))


def test_reports_follow_the_plan(gold, tmp_path):
    """Every case gives, per report, the gold blocks of its records in plan order, renumbered.  -c 1, -c 1:1, -j of the
    whole chromosome and an exclude where no event lies are the gold files themselves; -c 1:25,000-45,000 is the two TDs.
    (With -J the reference sorts the cleaned-up list by start, so the exclude at 55-65 kbp gives [1, 55000] then
    [65000, 200000]: gold order minus the excluded events.  j_reversed, an include list in reverse order without -J, is the
    case whose events come out of gold order: the second record's before the first's.)"""
    for name, kw in report_cases(tmp_path):
        plan = _plan_of(gold, kw)
        got = _call(gold, str(tmp_path / name), **kw)
        for suf in gu.SUFFIXES:
            _assert_same(got[suf], expected_from_gold(plan, suf), f"{name} _{suf}")
        if name in ("c1", "c1_1", "j_whole", "J_empty_middle"):
            gu.assert_reports_match_gold(str(tmp_path / name))
        if name == "c_25_45":
            assert [bp for bp, _ in blocks(got["TD"])] == [29997, 40000]
            assert got["D"] == got["SI"] == got["INV"] == b""
        if name == "J_55_65":
            assert plan == [("1", 1, 55000), ("1", 65000, 200000)]
        if name == "j_reversed":
            inv = [bp for bp, _ in blocks(got["INV"])]
            assert inv == [100000, 109999, 109999, 100000, 110000, 120000] and [bp for bp, _ in blocks(got["TD"])] == [29997, 40000]
            assert blocks(got["INV"])[0][1].split(b"\n")[1].startswith(b"0\tINV 800\t")


def test_li_of_one_chromosome_is_gold(gold, tmp_path):
    got = _call(gold, str(tmp_path / "c1"), li_on=True, region="1")
    assert got["LI"].split(b"\n") == _expected_on_the_text_route()


def _li_per_record(gold, plan, reports):
    """_LI of a one-window-per-record run: li_consumer's SortOutputLI per record -- the record's window [G, E + 10 kbp),
    the reads of it that kept a close end, the mask of the events that record reported (cleared at every record), Count_LI,
    the maximum insert size, the report length and the sample set carried over."""
    fa, reads_txt, chroms, r = gold
    recs = _records(reads_txt)
    seq = chroms[0][1]
    biol = len(seq) - 200000
    all_li = _li_reads(recs, r)
    by_name = {}
    want, count, upto, isz = b"", 0, [], 0
    per_rec = {suf: blocks(reports[suf]) for suf in gu.SUFFIXES}
    for _, s, e in plan:
        g, ge = max(s - BUFFER, 0), min(biol, e + BUFFER)
        in_win = [x for x in all_li if g <= x.pos < ge]
        isz = max([isz] + [x[6] for x in recs if g <= x[4] < ge])
        upto += in_win
        mine = {suf: b"".join(b for bp, b in per_rec[suf] if s <= bp <= e) for suf in gu.SUFFIXES}
        text = li.sort_output_li(seq, in_win, li.masked_positions(mine), g, ge, isz, max(x.length for x in upto),
                                 sorted({x.tag for x in upto}), count_start=count)
        count += text.count(b"\tLI\tChrID ")
        want += text
    return want


def test_li_per_record_and_thread_count(gold, tmp_path, monkeypatch):
    kw = report_cases(tmp_path)[5][1]
    plan = _plan_of(gold, kw)
    assert plan == [("1", 25000, 45000), ("1", 55000, 65000), ("1", 95000, 125000)]
    outs = {}
    for threads in ("1", "8"):
        monkeypatch.setenv("PGH_THREADS", threads)
        outs[threads] = _call(gold, str(tmp_path / f"t{threads}"), li_on=True, cem_on=True, **kw)
    assert outs["1"] == outs["8"]
    got = outs["1"]
    want = _li_per_record(gold, plan, got)
    assert want.count(b"\tLI\tChrID ") >= 3
    assert got["LI"] == want
    # SortOutputLI scans the whole window, not just the record: the breakpoints of events outside the records are not in the
    # record's mask (they are not reported), so their split reads show up as LI -- at 50 kbp in both the first and the
    # second record's windows ([15k, 55k) and [45k, 75k)), which overlap
    heads = [int(l.split(b"\t")[3]) for l in got["LI"].split(b"\n") if b"\tLI\tChrID " in l]
    assert heads.count(50000) == 2 and 20000 in heads and 129416 in heads


def test_close_end_mapped_lists_a_read_once_per_record(gold, tmp_path):
    """overlapping windows: a read in the windows of two records is searched, and listed, in each"""
    fa, reads_txt, chroms, r = gold
    kw = dict(include_bed=_bed(tmp_path / "o.bed", [("1", 30000, 40000), ("1", 45000, 60000)]))
    got = _call(gold, str(tmp_path / "o"), cem_on=True, **kw)
    recs = _records(reads_txt)
    want = 0
    for _, s, e in _plan_of(gold, kw):
        want += sum(1 for x, n in zip(recs, r["close_cnt"]) if n and max(s - BUFFER, 0) <= x[4] < e + BUFFER)
    assert got["CloseEndMapped"].count(b"\n") == 3 * want
    assert want > sum(1 for x, n in zip(recs, r["close_cnt"]) if n and 20000 <= x[4] < 70000)


def _strip_index(data: bytes, chr_name):
    return [b.split(b"\n", 2)[2] + b.split(b"\n", 2)[1].partition(b"\t")[2] for _, b in blocks(data)
            if f"\tChrID {chr_name}\t".encode() in b.split(b"\n")[1]]


def test_second_chromosome_alone_equals_its_part_of_all(tmp_path):
    fa, reads_txt, _ = _synthetic(tmp_path)
    chroms = hostio.load_fasta(fa)
    batch = hostio.read_pindel_text(reads_txt, [n for n, _ in chroms], [len(s) - 200000 for _, s in chroms])
    r = _oracle(chroms, batch)
    g = (fa, reads_txt, chroms, r)
    whole = _call(g, str(tmp_path / "all"), li_on=True)
    alone = _call(g, str(tmp_path / "b"), li_on=True, region="chrB")
    assert whole["LI"].count(b"\tLI\tChrID chrB") >= 2
    for suf in gu.SUFFIXES + ("LI",):
        assert _strip_index(alone[suf], "chrB") == _strip_index(whole[suf], "chrB"), suf
        assert _strip_index(alone[suf], "chrA") == []
    assert alone["LI"].split(b"\n")[1].startswith(b"0\tLI\tChrID chrB")


# ------------------------------------------------------------------------------------------- command line, no GPU
def _exe():
    from pindel_amd import binding
    return os.path.join(os.path.dirname(binding.LIB_PATH), "pindel_pg")


@pytest.mark.parametrize("args,status,message", [
    (["-c", "1:60-50"], 2, "end lies before the start"),
    (["-c", "1:x"], 2, "cannot parse the region"),
    (["-c", "X"], 1, "no chromosome X"),
    (["-c", "1:300000"], 1, "beyond the end"),
    (["-j", "BAD"], 1, "line 2"),
    (["-j", "UNK"], 1, "no chromosome X"),
    (["-j", "MISSING"], 1, "cannot open BED file"),
    (["-J", "BAD"], 1, "line 2"),
])
def test_command_line_rejects_bad_regions(gold, tmp_path, args, status, message):
    files = {"BAD": _bed(tmp_path / "bad.bed", [("1", 10, 20), "1 abc 30"]),
             "UNK": _bed(tmp_path / "unk.bed", [("X", 1, 100)]), "MISSING": str(tmp_path / "missing.bed")}
    args = [files.get(a, a) for a in args]
    out = subprocess.run([_exe(), "-f", gold[0], "-p", gold[1], "-o", str(tmp_path / "o")] + args, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == status, (out.returncode, out.stderr)
    assert message in out.stderr
    assert "pg_create" not in out.stderr


def test_command_line_empty_plan_writes_empty_reports(gold, tmp_path):
    exc = _bed(tmp_path / "all.bed", [("1", 1, 200000)])
    prefix = str(tmp_path / "e")
    out = subprocess.run([_exe(), "-f", gold[0], "-p", gold[1], "-o", prefix, "-c", "1:5000-6000", "-J", exc],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "no region left to search" in out.stdout
    for suf in ("D", "SI", "TD", "INV", "LI", "BP", "CloseEndMapped"):
        assert open(f"{prefix}_{suf}", "rb").read() == b"", suf
