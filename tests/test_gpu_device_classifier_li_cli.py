"""pindel_pg --device-classifier --device-classifier-li: -l and -s on the device-classifier path.  _LI is written by
the shared consumer from the long-insertion position tables the device built (pg_device_batch_li), _CloseEndMapped from the
summaries; no point leaves the GPU unless a window falls back.  All seven report files must be the bytes of the plain -l -s run, and
in one window _LI is what the reference's gold file gives on the text route."""
import os
import re
import subprocess

import pytest

from pindel_amd import binding
from tests import bam_writer as bw
from tests import golden_util as gu
from tests.test_bam_ingest import _gold_text_records, _pairs_for_text_records
from tests.test_li_pin import _expected_on_the_text_route

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(binding.LIB_PATH), "pindel_pg")
TIMEOUT = 300
SUFFIXES = ("D", "SI", "TD", "INV", "LI", "BP", "CloseEndMapped")
LINE = re.compile(r"pindel_pg: device classifier: (\d+) windows, (\d+) from tables, (\d+) fell back, (\d+) unresolved reads, "
                  r"(\d+) report records, (\d+) runs not downloaded(?:, (\d+) hinted windows)?, (\d+) windows with LI tables")
DC = ("--device-classifier", "--device-classifier-li")


@pytest.fixture(scope="module")
def gold(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dc_li_cli")
    fa, reads_txt = gu.unpack(tmp)
    return dict(tmp=tmp, fa=fa, reads_txt=reads_txt)


def run(gold, name, *extra, inputs=None):
    prefix = str(gold["tmp"] / name)
    out = subprocess.run([EXE, "-f", gold["fa"], *(inputs or ("-p", gold["reads_txt"])), "-o", prefix, "-T", "2", *extra],
                         capture_output=True, text=True, timeout=TIMEOUT)
    return out, prefix


def reports(prefix):
    return {s: open(f"{prefix}_{s}", "rb").read() for s in SUFFIXES}


def summary(out):
    m = LINE.search(out.stdout)
    assert m, out.stdout[-2000:]
    return dict(zip(("windows", "tables", "fallbacks", "unresolved", "records", "runs_kept", "hinted", "li_windows"),
                    (int(x) if x is not None else None for x in m.groups())))


def records_of(close_end_mapped: bytes):
    lines = close_end_mapped.split(b"\n")
    return [tuple(lines[i:i + 3]) for i in range(0, len(lines) - 1, 3)]


SCENARIOS = {"one_window": (), "w_0.02": ("-w", "0.02"), "region": ("-c", "1:20000-150000"), "M3": ("-M", "3")}


@pytest.fixture(scope="module")
def plain_runs(gold):
    """the plain -l -s run of every scenario, once"""
    out = {}
    for name, extra in SCENARIOS.items():
        res, prefix = run(gold, f"{name}_plain", "-l", "-s", *extra)
        assert res.returncode == 0, res.stderr
        out[name] = (res, reports(prefix))
    return out


@pytest.mark.parametrize("scenario", sorted(SCENARIOS))
def test_seven_reports_equal_the_plain_run(gold, plain_runs, scenario):
    extra = SCENARIOS[scenario]
    plain, want = plain_runs[scenario]
    flagged, f_prefix = run(gold, f"{scenario}_dc", *DC, "-l", "-s", *extra)
    assert flagged.returncode == 0, flagged.stderr
    got = reports(f_prefix)
    for s in SUFFIXES:
        assert got[s] == want[s], s
    assert len(want["LI"]) > 0 and len(want["CloseEndMapped"]) > 0
    s = summary(flagged)
    assert s["windows"] > 0 and s["tables"] == s["windows"] and s["fallbacks"] == 0 and s["unresolved"] == 0     # every window from tables
    assert 0 < s["li_windows"] <= s["windows"] and s["runs_kept"] > 0
    assert (s["windows"] > 3) == (scenario == "w_0.02")
    assert "windows with LI tables" not in plain.stdout
    assert re.search(r"long-insertion tables downloaded: \d+ bytes", flagged.stdout)
    if scenario == "one_window":
        gu.assert_reports_match_gold(f_prefix)
        assert got["LI"].split(b"\n") == _expected_on_the_text_route()
        assert len(records_of(got["CloseEndMapped"])) == 14862


@pytest.mark.parametrize("extra", [(), ("-w", "0.02")])
def test_lists_cut_to_nothing_fall_back(gold, plain_runs, extra):
    """--device-classifier-listed 0: the windows with a listed pair take the existing steps, which write both files; the bytes stay
    and no read is written to _CloseEndMapped twice."""
    tag = "cut0" + "_".join(extra)
    _, want = plain_runs["w_0.02" if extra else "one_window"]
    flagged, f_prefix = run(gold, f"{tag}_dc", *DC, "--device-classifier-listed", "0", "-l", "-s", *extra)
    assert flagged.returncode == 0, flagged.stderr
    got = reports(f_prefix)
    for s in SUFFIXES:
        assert got[s] == want[s], s
    s = summary(flagged)
    assert s["fallbacks"] > 0 and s["tables"] + s["fallbacks"] == s["windows"]
    assert len(records_of(got["CloseEndMapped"])) == len(records_of(want["CloseEndMapped"]))


@pytest.mark.parametrize("flag", ["-l", "-s"])
def test_either_report_alone(gold, flag):
    plain, p_prefix = run(gold, f"alone{flag}_plain", flag, "-w", "0.02")
    flagged, f_prefix = run(gold, f"alone{flag}_dc", *DC, flag, "-w", "0.02")
    assert plain.returncode == 0 and flagged.returncode == 0, (plain.stderr, flagged.stderr)
    got, want = reports(f_prefix), reports(p_prefix)
    assert got == want
    assert (len(got["LI"]) > 0) == (flag == "-l") and (len(got["CloseEndMapped"]) > 0) == (flag == "-s")
    assert (summary(flagged)["li_windows"] > 0) == (flag == "-l")


def test_bam_input(gold):
    """pindel_pg -i on the gold reads as a BAM: -R false, and -R on with --device-classifier-hints"""
    tmp = gold["tmp"]
    bw.write_bam(str(tmp / "gold.bam"), [("1", 200000)], _pairs_for_text_records(_gold_text_records()), with_index=False)
    cfg = tmp / "config.txt"
    cfg.write_text("gold.bam\t500\tSIM1CHRVS2\n")
    inputs = ("-i", str(cfg))
    for tag, more, hints in (("norp", ("-R", "false"), ()), ("rp", (), ("--device-classifier-hints",))):
        plain, p_prefix = run(gold, f"bam_{tag}_plain", "-l", "-s", *more, inputs=inputs)
        flagged, f_prefix = run(gold, f"bam_{tag}_dc", *DC, *hints, "-l", "-s", *more, inputs=inputs)
        assert plain.returncode == 0 and flagged.returncode == 0, (plain.stderr, flagged.stderr)
        got, want = reports(f_prefix), reports(p_prefix)
        for s in SUFFIXES:
            assert got[s] == want[s], (tag, s)
        assert len(want["LI"]) > 0 and len(want["CloseEndMapped"]) > 0
        s = summary(flagged)
        assert s["tables"] == s["windows"] > 0 and s["fallbacks"] == 0 and s["li_windows"] > 0
        assert (s["hinted"] is not None) == bool(hints)


REFUSALS = [(("-l",), "with -l:"), (("-s",), "with -s:"), (("--device-classifier-li", "false", "-l"), "with -l:"),
            (("--device-classifier-li", "-S"), "with -S:"), (("--device-classifier-li", "-l", "-I"), "with -I:"),
            (("--device-classifier-li", "-q"), "with -q:"), (("--device-classifier-li", "-s", "-N"), "with -N:"),
            (("--device-classifier-li", "-l", "-G", "0,0"), "one device")]


@pytest.mark.parametrize("extra,text", REFUSALS, ids=[" ".join(e) for e, _ in REFUSALS])
def test_refusals_that_remain(gold, extra, text):
    """Status 2 before any device is touched, the text as before, and no output file written."""
    out, prefix = run(gold, "refused_" + re.sub(r"\W", "", " ".join(extra)), "--device-classifier", *extra)
    assert out.returncode == 2 and "--device-classifier" in out.stderr and text in out.stderr, out.stderr
    assert not any(os.path.exists(f"{prefix}_{s}") for s in SUFFIXES)


def test_the_switch_alone_is_refused(gold):
    out, prefix = run(gold, "refused_li_alone", "--device-classifier-li", "-l")
    assert out.returncode == 2 and "--device-classifier-li needs --device-classifier" in out.stderr
    assert not any(os.path.exists(f"{prefix}_{s}") for s in SUFFIXES)
