"""pindel_pg --device-classifier --device-classifier-dd -q: -q on the device-classifier path.  Per window the split reads
around the discordant clusters are uploaded once, close-searched on the device (pg_device_batch_close_search) and turned into breakpoint
tables, consensus and containment verdicts there (pg_device_batch_dd); the shared consumer writes _DD from one download.  On the demo
BAM (tests/golden/simulated_MEI) and on the planted events of tests/dd_synth.py every report file must be the bytes of the plain run
with the same flags."""
import os
import re
import subprocess

import pytest

from pindel_amd import binding
from tests import dd_synth
from tests.test_mei_bam import _unpack

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(binding.LIB_PATH), "pindel_pg")
TIMEOUT = 300
SUFFIXES = ("D", "SI", "TD", "INV", "LI", "BP", "CloseEndMapped", "DD")
DC = ("--device-classifier", "--device-classifier-dd")
HINTS = ("--device-classifier-hints",)
TABLES = re.compile(r"pindel_pg: dispersed duplications: (\d+) windows built from device tables, (\d+) bytes downloaded for them")
TESTS = re.compile(r"pindel_pg: dispersed duplications: \d+ discordant reads, \d+ clusters, (\d+) breakpoints, (\d+) consensus tests "
                   r"\(GPU [\d.]+ s, (\d+) kept\), (\d+) events")


@pytest.fixture(scope="module")
def samples(tmp_path_factory):
    demo = _unpack(tmp_path_factory.mktemp("dc_dd_demo"))
    d = str(tmp_path_factory.mktemp("dc_dd_synth"))
    syn = dd_synth.make(d)
    return dict(demo=dict(tmp=demo, fasta=os.path.join(demo, "reference.fa"), config=os.path.join(demo, "config"), text=os.path.join(demo, "input"),
                          extra=()),
                synth=dict(tmp=d, fasta=syn["fasta"], config=syn["config"], extra=("--MIN_DD_MAP_DISTANCE", "400")), plain={})


def run(s, name, *flags, inputs=None):
    prefix = os.path.join(str(s["tmp"]), name)
    out = subprocess.run([EXE, "-f", s["fasta"], *(inputs or ("-i", s["config"])), "-o", prefix, *s["extra"], *flags], capture_output=True, text=True,
                         timeout=TIMEOUT, cwd=str(s["tmp"]))
    return out, prefix


def reports(prefix, more=()):
    return {x: open(f"{prefix}_{x}", "rb").read() for x in SUFFIXES + tuple(more)}


def plain_run(samples, which, flags, more=()):
    """the plain -q run with `flags`, once per sample and flag set"""
    key = (which, flags)
    if key not in samples["plain"]:
        out, prefix = run(samples[which], "plain_" + re.sub(r"\W", "", "".join(flags)), "-q", *flags)
        assert out.returncode == 0, out.stderr[-2000:]
        assert not TABLES.search(out.stdout)
        samples["plain"][key] = (reports(prefix, more), out.stdout)
    return samples["plain"][key]


def both(samples, which, tag, flags=(), dc=DC + HINTS, dc_flags=None, more=()):
    want, plain_log = plain_run(samples, which, tuple(flags), more)
    out, prefix = run(samples[which], "dc_" + tag, *dc, "-q", *(flags if dc_flags is None else dc_flags))
    assert out.returncode == 0, out.stderr[-2000:]
    got = reports(prefix, more)
    for x in got:
        assert got[x] == want[x], (which, tag, x)
    assert len(want["DD"]) > 0 and b"\tDD\t" in want["DD"]
    m = TABLES.search(out.stdout)
    assert m and int(m.group(1)) >= 1 and int(m.group(2)) > 0, out.stdout[-2000:]           # at least one window from device tables
    a, b = TESTS.search(out.stdout), TESTS.search(plain_log)
    assert a and b and a.groups() == b.groups()                                           # the line keeps its wording and its counts
    return out.stdout, got


@pytest.mark.parametrize("which", ["demo", "synth"])
def test_all_reports_equal_the_plain_run(samples, which):
    log, _ = both(samples, which, "hints")
    if which == "synth":                                                                  # both outcomes of the containment test
        _, tests, kept, _ = (int(x) for x in TESTS.search(log).groups())
        assert kept > 0 and tests - kept > 0


@pytest.mark.parametrize("which", ["demo", "synth"])
def test_without_read_pair_hints(samples, which):
    both(samples, which, "norp", flags=("-R", "false"), dc=DC)


@pytest.mark.parametrize("which", ["demo", "synth"])
def test_with_the_duplication_reads(samples, which):
    both(samples, which, "dup", flags=("--DD_REPORT_DUPLICATION_READS",))


@pytest.mark.parametrize("threads", ["1", "8"])
@pytest.mark.parametrize("which", ["demo", "synth"])
def test_host_threads_change_nothing(samples, which, threads):
    both(samples, which, "t" + threads, flags=(), dc_flags=("-T", threads))


@pytest.mark.parametrize("which", ["demo", "synth"])
def test_together_with_the_long_insertion_switch(samples, which):
    log, got = both(samples, which, "li", flags=("-l", "-s"), dc=DC + HINTS + ("--device-classifier-li",))
    assert "windows with LI tables" in log and len(got["CloseEndMapped"]) > 0


@pytest.mark.parametrize("which", ["demo", "synth"])
def test_together_with_the_junction_switch(samples, which):
    log, _ = both(samples, which, "int", flags=("-I",), dc=DC + HINTS + ("--device-classifier-int",), more=("INT", "INT_final"))
    assert "windows with junction tables" in log


def test_q_with_pindel_text_input_writes_an_empty_dd_and_a_note(samples):
    s = samples["demo"]
    out, prefix = run(s, "dc_text", *DC, "-q", inputs=("-p", s["text"]))
    assert out.returncode == 0, out.stderr[-2000:]
    assert os.path.getsize(prefix + "_DD") == 0 and "_DD is empty" in out.stdout


REFUSALS = [(("-q",), "with -q:"), (("--device-classifier-dd", "false", "-q"), "with -q:"), (("--device-classifier-int", "-q"), "with -q:"),
            (("--device-classifier-dd", "-q", "-S"), "with -S:"), (("--device-classifier-dd", "-q", "-N"), "with -N:"),
            (("--device-classifier-dd", "-q", "-G", "0,0"), "one device"), (("--device-classifier-dd", "-q", "-I"), "with -I:"),
            (("--device-classifier-dd", "-q", "-l"), "with -l:")]


@pytest.mark.parametrize("extra,text", REFUSALS, ids=[" ".join(e) for e, _ in REFUSALS])
def test_refusals_that_remain(samples, extra, text):
    """Status 2 before any device is touched, the text as before, and no output file written.  The first and the third case -- -q
    without the new switch, and beside --device-classifier-int only -- are refused before this feature as well: they pin that the old
    refusal stands with its text.  The others need the switch to exist."""
    s = samples["demo"]
    out, prefix = run(s, "refused_" + re.sub(r"\W", "", " ".join(extra)), "--device-classifier", "--device-classifier-hints", *extra)
    assert out.returncode == 2 and "--device-classifier" in out.stderr and text in out.stderr, out.stderr
    assert not any(os.path.exists(f"{prefix}_{x}") for x in SUFFIXES)


def test_the_switch_alone_is_refused(samples):
    out, prefix = run(samples["demo"], "refused_dd_alone", "--device-classifier-dd", "-q")
    assert out.returncode == 2 and "--device-classifier-dd needs --device-classifier" in out.stderr
    assert not any(os.path.exists(f"{prefix}_{x}") for x in SUFFIXES)
