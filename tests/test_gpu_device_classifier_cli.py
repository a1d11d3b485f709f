"""pindel_pg --device-classifier: every window classified on the device -- upload, fused search,
pg_device_batch_classify -- and written by Caller::process_window_from_tables from the downloaded tables, records and summaries; the
points stay on the GPU unless a window falls back.  The four reports must be the bytes of the run without the flag, and in one
window those of the reference's gold reports."""
import os
import re
import subprocess

import pytest

from pindel_amd import binding
from tests import bam_writer as bw
from tests import golden_util as gu
from tests.test_bam_ingest import _gold_text_records, _pairs_for_text_records

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(binding.LIB_PATH), "pindel_pg")
TIMEOUT = 300
LINE = re.compile(r"pindel_pg: device classifier: (\d+) windows, (\d+) from tables, (\d+) fell back, (\d+) unresolved reads, "
                  r"(\d+) report records, (\d+) runs not downloaded")


@pytest.fixture(scope="module")
def gold(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dc_cli")
    fa, reads_txt = gu.unpack(tmp)
    return dict(tmp=tmp, fa=fa, reads_txt=reads_txt)


def run(gold, name, *extra, inputs=None):
    prefix = str(gold["tmp"] / name)
    out = subprocess.run([EXE, "-f", gold["fa"], *(inputs or ("-p", gold["reads_txt"])), "-o", prefix, "-T", "2", *extra],
                         capture_output=True, text=True, timeout=TIMEOUT)
    return out, prefix


def reports(prefix):
    return [open(f"{prefix}_{s}", "rb").read() for s in gu.SUFFIXES]


def summary(out):
    m = LINE.search(out.stdout)
    assert m, out.stdout[-2000:]
    return dict(zip(("windows", "tables", "fallbacks", "unresolved", "records", "runs_kept"), (int(x) for x in m.groups())))


SCENARIOS = {"one_window": (), "w_0.02": ("-w", "0.02"), "region": ("-c", "1:20000-150000"), "M3": ("-M", "3"), "B10": ("-B", "10"),
             "no_td_inv": ("-r", "false", "-t", "false")}


@pytest.mark.parametrize("scenario", sorted(SCENARIOS))
def test_reports_equal_the_run_without_the_flag(gold, scenario):
    extra = SCENARIOS[scenario]
    plain, p_prefix = run(gold, f"{scenario}_plain", *extra)
    flagged, f_prefix = run(gold, f"{scenario}_dc", "--device-classifier", *extra)
    assert plain.returncode == 0 and flagged.returncode == 0, (plain.stderr, flagged.stderr)
    assert "device classifier" not in plain.stdout
    assert reports(f_prefix) == reports(p_prefix)
    s = summary(flagged)
    assert s["windows"] > 0 and s["tables"] == s["windows"] and s["fallbacks"] == 0 and s["unresolved"] == 0     # every window from tables
    assert s["records"] > 0 and s["runs_kept"] > 0
    assert (s["windows"] > 3) == (scenario == "w_0.02")
    # the far-end step's lines and the run's counts come from the summaries
    count = lambda o: re.findall(r"^(Total: \d+;\tClose_end_found \d+;\tFar_end_found \d+;)", o.stdout, re.M)
    assert count(flagged) == count(plain) and len(count(plain)) > 0
    assert re.search(r"pindel_pg: \d+ reads, close end \d+, far end \d+", plain.stdout).group(0) in flagged.stdout
    if scenario == "one_window":
        gu.assert_reports_match_gold(f_prefix)
        assert "close end 14862, far end 10968" in flagged.stdout


@pytest.mark.parametrize("extra", [(), ("-w", "0.02")])
def test_lists_cut_to_nothing_fall_back(gold, extra):
    """--device-classifier-listed 0: every read that reaches a list with a pair is unresolved, its window fetches its points and
    takes the existing path; the bytes stay."""
    tag = "cut0" + "_".join(extra)
    plain, p_prefix = run(gold, f"{tag}_plain", *extra)
    flagged, f_prefix = run(gold, f"{tag}_dc", "--device-classifier", "--device-classifier-listed", "0", *extra)
    assert plain.returncode == 0 and flagged.returncode == 0, (plain.stderr, flagged.stderr)
    assert reports(f_prefix) == reports(p_prefix)
    s = summary(flagged)
    assert s["fallbacks"] > 0 and s["unresolved"] > 0 and s["tables"] + s["fallbacks"] == s["windows"]
    if not extra:
        gu.assert_reports_match_gold(f_prefix)
    # cut to one pair the gold set needs no fallback (the first listed pair makes every such read Used)
    one, o_prefix = run(gold, f"{tag}_dc1", "--device-classifier", "--device-classifier-listed", "1", *extra)
    assert one.returncode == 0 and reports(o_prefix) == reports(p_prefix)
    assert summary(one)["fallbacks"] == 0


def test_bam_input(gold):
    """pindel_pg -i on the gold reads as a BAM, with -R false: the same reports with and without the flag."""
    tmp = gold["tmp"]
    bw.write_bam(str(tmp / "gold.bam"), [("1", 200000)], _pairs_for_text_records(_gold_text_records()), with_index=False)
    cfg = tmp / "config.txt"
    cfg.write_text("gold.bam\t500\tSIM1CHRVS2\n")
    inputs = ("-i", str(cfg))
    plain, p_prefix = run(gold, "bam_plain", "-R", "false", inputs=inputs)
    flagged, f_prefix = run(gold, "bam_dc", "-R", "false", "--device-classifier", inputs=inputs)
    assert plain.returncode == 0 and flagged.returncode == 0, (plain.stderr, flagged.stderr)
    assert reports(f_prefix) == reports(p_prefix)
    gu.assert_reports_match_gold(f_prefix)
    s = summary(flagged)
    assert s["tables"] == s["windows"] > 0 and s["fallbacks"] == 0
    assert "14862 reads, close end 14862, far end 10968" in flagged.stdout
    cut, c_prefix = run(gold, "bam_dc0", "-R", "false", "--device-classifier", "--device-classifier-listed", "0", inputs=inputs)
    assert cut.returncode == 0 and reports(c_prefix) == reports(p_prefix) and summary(cut)["fallbacks"] > 0


REFUSALS = [(("-l",), "-l"), (("-s",), "-s"), (("-S",), "-S"), (("-I",), "-I"), (("-q",), "-q"), (("-N",), "-N"),
            (("-b", "nowhere.txt", "--bd-hints", "on"), "--bd-hints on"), (("-G", "0,0"), "one device"),
            (("--device-classifier-listed", "5"), "0 to 4")]


@pytest.mark.parametrize("extra,text", REFUSALS, ids=[t for _, t in REFUSALS])
def test_refusals(gold, extra, text):
    """Status 2 before any device is touched, a text that names the flag, and no output file written."""
    out, prefix = run(gold, "refused_" + re.sub(r"\W", "", text), "--device-classifier", *extra)
    assert out.returncode == 2 and "--device-classifier" in out.stderr and text in out.stderr, out.stderr
    assert not any(os.path.exists(f"{prefix}_{s}") for s in gu.SUFFIXES)


def test_more_refusals(gold):
    out, prefix = run(gold, "refused_listed_alone", "--device-classifier-listed", "2")
    assert out.returncode == 2 and "--device-classifier-listed needs --device-classifier" in out.stderr
    assert not os.path.exists(prefix + "_D")
    cfg = gold["tmp"] / "config_r.txt"
    cfg.write_text("gold.bam\t500\tSIM1CHRVS2\n")
    out, prefix = run(gold, "refused_bam_rp", "--device-classifier", inputs=("-i", str(cfg)))
    assert out.returncode == 2 and "--device-classifier" in out.stderr and "-R false" in out.stderr
    assert not os.path.exists(prefix + "_D")
