"""pindel_pg --device-classifier --device-classifier-hints --device-classifier-int -I: -I on the device-classifier
path.  _INT is written by the shared consumer from the junction tables the device built (pg_device_batch_int) and the summaries; no
point leaves the GPU unless a window falls back.  On the BAM and on the text + --bd-hints on inputs of tests/interchr_synth.py every
report file, _INT and _INT_final must be the bytes of the plain -I run (the planted junctions have 11 split reads per side and strand,
so _INT is not empty)."""
import os
import re
import subprocess

import pytest

from pindel_amd import binding
from tests import interchr_synth as syn

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(binding.LIB_PATH), "pindel_pg")
TIMEOUT = 300
SUFFIXES = ("D", "SI", "TD", "INV", "LI", "BP", "CloseEndMapped", "INT", "INT_final")
LINE = re.compile(r"pindel_pg: device classifier: (\d+) windows, (\d+) from tables, (\d+) fell back, (\d+) unresolved reads, "
                  r"(\d+) report records, (\d+) runs not downloaded, (\d+) hinted windows(?:, (\d+) windows with LI tables)?, "
                  r"(\d+) windows with junction tables")
DC = ("--device-classifier", "--device-classifier-hints", "--device-classifier-int")


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    d = tmp_path_factory.mktemp("dc_int_cli")
    s = syn.make(str(d))
    return dict(tmp=d, s=s, bam=("-i", s["config"]), text=("-p", s["reads_txt"], "-b", s["bd"], "--bd-hints", "on"))


def run(sample, name, inputs, *extra):
    prefix = str(sample["tmp"] / name)
    out = subprocess.run([EXE, "-f", sample["s"]["fasta"], *inputs, "-o", prefix, "-T", "2", *extra], capture_output=True, text=True,
                         timeout=TIMEOUT, cwd=str(sample["tmp"]))
    return out, prefix


def reports(prefix):
    return {s: open(f"{prefix}_{s}", "rb").read() for s in SUFFIXES}


def summary(out):
    m = LINE.search(out.stdout)
    assert m, out.stdout[-2000:]
    return dict(zip(("windows", "tables", "fallbacks", "unresolved", "records", "runs_kept", "hinted", "li_windows", "int_windows"),
                    (int(x) if x is not None else None for x in m.groups())))


def both(sample, tag, inputs, *extra, dc=DC):
    plain, p_prefix = run(sample, f"{tag}_plain", inputs, "-I", *extra)
    flagged, f_prefix = run(sample, f"{tag}_dc", inputs, *dc, "-I", *extra)
    assert plain.returncode == 0 and flagged.returncode == 0, (plain.stderr[-2000:], flagged.stderr[-2000:])
    got, want = reports(f_prefix), reports(p_prefix)
    for s in SUFFIXES:
        assert got[s] == want[s], (tag, s)
    assert len(want["INT"]) > 0 and want["INT"].count(b"support: ") >= 3 and len(want["INT_final"]) > 0
    assert "windows with junction tables" not in plain.stdout
    assert re.search(r"junction tables downloaded: \d+ bytes", flagged.stdout)
    return summary(flagged), got


@pytest.mark.parametrize("route", ["bam", "text"])
def test_all_reports_equal_the_plain_run(sample, route):
    s, got = both(sample, route, sample[route], "-w", syn.WINDOW_MBP)
    assert s["windows"] > 3 and s["tables"] == s["windows"] and s["fallbacks"] == 0 and s["unresolved"] == 0      # every window from tables
    assert 0 < s["int_windows"] <= s["windows"] and s["hinted"] > 0 and s["li_windows"] is None
    assert b"\tD %d\t" % syn.DEL_LEN in got["D"]


@pytest.mark.parametrize("route", ["bam", "text"])
def test_every_chromosome_pair_with_the_repair(sample, route):
    s, got = both(sample, f"{route}_pairs", sample[route], "-w", syn.WINDOW_MBP, "--repair", "int-pairs")
    assert s["fallbacks"] == 0 and s["int_windows"] > 0
    # (ii) chrB -> chrC is written only with the repair
    plain = reports(str(sample["tmp"] / f"{route}_plain")) if os.path.exists(str(sample["tmp"] / f"{route}_plain_INT")) else None
    assert b" chrB " in got["INT"] and b" chrC " in got["INT"]
    if plain is not None:
        assert got["INT"].count(b"\n") > plain["INT"].count(b"\n")


def test_one_window_per_chromosome(sample):
    s, _ = both(sample, "bam_whole", sample["bam"])
    assert 3 <= s["windows"] == s["tables"] and s["int_windows"] >= 3


def test_lists_cut_to_nothing_fall_back(sample):
    """--device-classifier-listed 0: the windows with a listed pair take the existing steps, which report _INT themselves; the bytes
    stay and _INT is written once per window either way."""
    s, _ = both(sample, "bam_cut0", sample["bam"], "-w", syn.WINDOW_MBP, dc=DC + ("--device-classifier-listed", "0"))
    assert s["fallbacks"] > 0 and s["tables"] + s["fallbacks"] == s["windows"] and 0 < s["int_windows"] <= s["tables"]


def test_together_with_the_long_insertion_switch(sample):
    s, got = both(sample, "bam_li", sample["bam"], "-w", syn.WINDOW_MBP, "-l", "-s", dc=DC + ("--device-classifier-li",))
    assert s["fallbacks"] == 0 and s["li_windows"] > 0 and s["int_windows"] > 0
    assert len(got["CloseEndMapped"]) > 0


REFUSALS = [(("-I",), "with -I:"), (("--device-classifier-int", "false", "-I"), "with -I:"), (("--device-classifier-li", "-I"), "with -I:"),
            (("--device-classifier-int", "-I", "-l"), "with -l:"), (("--device-classifier-int", "-I", "-s"), "with -s:"),
            (("--device-classifier-int", "-I", "-S"), "with -S:"), (("--device-classifier-int", "-I", "-q"), "with -q:"),
            (("--device-classifier-int", "-I", "-N"), "with -N:"), (("--device-classifier-int", "-I", "-G", "0,0"), "one device")]


@pytest.mark.parametrize("extra,text", REFUSALS, ids=[" ".join(e) for e, _ in REFUSALS])
def test_refusals_that_remain(sample, extra, text):
    """Status 2 before any device is touched, the text as before, and no output file written.  The first and the third case -- -I
    without the new switch, and beside --device-classifier-li only -- are refused before this feature as well: they pin that the old
    refusal stands with its text.  The others need the switch to exist."""
    out, prefix = run(sample, "refused_" + re.sub(r"\W", "", " ".join(extra)), sample["text"], "--device-classifier", "--device-classifier-hints", *extra)
    assert out.returncode == 2 and "--device-classifier" in out.stderr and text in out.stderr, out.stderr
    assert not any(os.path.exists(f"{prefix}_{s}") for s in SUFFIXES)


def test_the_switch_alone_is_refused(sample):
    out, prefix = run(sample, "refused_int_alone", sample["text"], "--device-classifier-int", "-I")
    assert out.returncode == 2 and "--device-classifier-int needs --device-classifier" in out.stderr
    assert not any(os.path.exists(f"{prefix}_{s}") for s in SUFFIXES)
