"""Region selection on the MI355X: `pindel_pg -c / -j / -J` through the close-end and far-end searches.

  * Text route (sim1chrVs2): every region case of tests/test_region_plan.py, with -s -l, writes the same bytes as the CPU
    route (call_from_points on the oracle's points with the same plan); one multi-record plan again with -w 0.02 (several
    windows per record, starts offset by the record), with -S and with two contexts on one device.
  * BAM route (the reference's demo BAM, simulated_MEI): -j of both chromosomes whole = -c ALL, every file and _RP; -c chr1 and
    -c chr2 = the ALL run's blocks of that chromosome except the index; a sub-region on two contexts = one context.
"""
import os
import subprocess

import pytest

from tests import golden_util as gu
from tests.test_region_plan import _bed, _call, blocks, gold, report_cases  # noqa: F401  (gold: the module fixture)

REPORTS = ("D", "SI", "TD", "INV", "LI", "CloseEndMapped")
ALL_FILES = REPORTS + ("BP",)


def _exe():
    from pindel_amd import binding
    return os.path.join(os.path.dirname(binding.LIB_PATH), "pindel_pg")


def _run(args, timeout=600):
    out = subprocess.run([_exe()] + args, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr
    return out


def _files(prefix, names=ALL_FILES):
    return {s: open(f"{prefix}_{s}", "rb").read() for s in names}


def _cli_region_args(kw):
    a = []
    if kw.get("region"):
        a += ["-c", kw["region"]]
    if kw.get("include_bed"):
        a += ["-j", kw["include_bed"]]
    if kw.get("exclude_bed"):
        a += ["-J", kw["exclude_bed"]]
    return a


@pytest.mark.gpu
def test_text_route_every_region_case_equals_the_cpu_route(gold, tmp_path):
    fa, reads_txt = gold[0], gold[1]
    base = ["-f", fa, "-p", reads_txt, "-l", "-s", "-T", "4"]
    for name, kw in report_cases(tmp_path):
        p = str(tmp_path / f"gpu_{name}")
        out = _run(base + ["-o", p] + _cli_region_args(kw))
        assert "Processing region: 1\t" in out.stdout
        want = _call(gold, str(tmp_path / f"cpu_{name}"), li_on=True, cem_on=True, **kw)
        got = _files(p)
        for suf in REPORTS:
            assert got[suf] == want[suf], f"{name} _{suf}"
        assert got["BP"] == b""
        if name == "c_25_45":
            assert [bp for bp, _ in blocks(got["TD"])] == [29997, 40000]


@pytest.mark.gpu
def test_text_route_multi_record_plan_small_windows_close_only_and_two_contexts(gold, tmp_path):
    fa, reads_txt = gold[0], gold[1]
    kw = dict(report_cases(tmp_path))["j_three"]
    base = ["-f", fa, "-p", reads_txt, "-l", "-s", "-T", "4"] + _cli_region_args(kw)
    # -w 0.02: records of 20-30 kbp plus 10 kbp either side in 20-kbp windows from S - 10 kbp
    p = str(tmp_path / "w")
    _run(base + ["-o", p, "-w", "0.02"])
    want = _call(gold, str(tmp_path / "cpu_w"), li_on=True, cem_on=True, window_mbp=0.02, **kw)
    got = _files(p)
    for suf in REPORTS:
        assert got[suf] == want[suf], f"-w 0.02 _{suf}"
    # one device / two contexts on it / close end only
    one = str(tmp_path / "one")
    _run(base + ["-o", one])
    ref = _files(one)
    assert ref["CloseEndMapped"] and sum(len(blocks(ref[s])) for s in gu.SUFFIXES) > 0
    two = str(tmp_path / "two")
    _run(base + ["-o", two, "-G", "0,0"])
    assert _files(two) == ref
    only = str(tmp_path / "only")
    out = _run(base + ["-o", only, "-S"])
    assert "far end" not in out.stdout
    got = _files(only)
    assert got["CloseEndMapped"] == ref["CloseEndMapped"]
    for suf in ("D", "SI", "TD", "INV", "LI", "BP"):
        assert got[suf] == b"", suf


def _mei(tmp_path):
    from tests.test_mei_bam import _chroms
    d, chroms = _chroms(tmp_path)
    return d, [(n, len(s) - 200000) for n, s in chroms]


def _strip_index(data: bytes, chr_name):
    out = []
    for _, b in blocks(data):
        sep, head, rest = b.split(b"\n", 2)
        if f"\tChrID {chr_name}\t".encode() in head:
            out.append(head.partition(b"\t")[2] + b"\n" + rest)
    return out


def _close_mapped_of(data: bytes, chr_name):
    """the _CloseEndMapped records (three lines each) anchored on chr_name"""
    lines = data.split(b"\n")
    return [lines[k:k + 3] for k in range(0, len(lines) - 2, 3) if lines[k + 2].split(b"\t")[1] == chr_name.encode()]


@pytest.mark.gpu
def test_bam_route_regions(tmp_path):
    d, sizes = _mei(tmp_path)
    base = ["-f", os.path.join(d, "reference.fa"), "-i", os.path.join(d, "config"), "-l", "-s", "-T", "4"]
    names = ALL_FILES + ("RP",)
    whole = str(tmp_path / "all")
    _run(base + ["-o", whole, "-c", "ALL"])
    ref = _files(whole, names)
    assert ref["CloseEndMapped"]
    # -j of both chromosomes whole, in .fai order: the same plan, the same bytes
    bed = _bed(tmp_path / "both.bed", [(n, 1, s) for n, s in sizes])
    j = str(tmp_path / "j")
    out = _run(base + ["-o", j, "-j", bed])
    assert out.stdout.count("Processing region: ") == 2
    assert _files(j, names) == ref
    # one chromosome alone: its blocks of the ALL run, except the index
    seen = 0
    for n, _ in sizes:
        p = str(tmp_path / f"c_{n}")
        _run(base + ["-o", p, "-c", n])
        got = _files(p, names)
        for suf in gu.SUFFIXES + ("LI",):
            assert _strip_index(got[suf], n) == _strip_index(ref[suf], n), f"-c {n} _{suf}"
            other = [m for m, _ in sizes if m != n][0]
            assert _strip_index(got[suf], other) == []
            seen += len(_strip_index(got[suf], n))
        assert _close_mapped_of(got["CloseEndMapped"], n) == _close_mapped_of(ref["CloseEndMapped"], n)
        assert _close_mapped_of(got["CloseEndMapped"], n) and _close_mapped_of(got["CloseEndMapped"], other) == []
    assert seen == sum(len(blocks(ref[s])) for s in gu.SUFFIXES + ("LI",))
    # a sub-region on two contexts of one device = one context
    sub = ["-c", f"{sizes[0][0]}:20,000-70,000"]
    one, two = str(tmp_path / "sub1"), str(tmp_path / "sub2")
    _run(base + ["-o", one] + sub)
    _run(base + ["-o", two, "-G", "0,0"] + sub)
    assert _files(one, names) == _files(two, names)
