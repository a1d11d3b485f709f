"""-N (--NormalSamples) through the command line on BAM input: `pindel_pg -i config [-N]` on the two-sample synthetic of
tests/germline_synth.py, with the expectations of tests/test_germline_cpu.py."""
import pytest

from tests import cli_chain as cli
from tests import germline_synth as gs
from tests import golden_util as gu
from tests.test_germline_cpu import SUFFIXES, check_expectations, check_fixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    d = tmp_path_factory.mktemp("germline_gpu")
    s = gs.make(str(d))
    check_fixture(s)
    s["dir"] = d
    s["base"] = ["-f", s["fasta"], "-i", s["config"], "-x", gs.MAX_RANGE_INDEX, "-l"]
    return s


def reports(prefix):
    return {suf: cli.read(f"{prefix}_{suf}") for suf in SUFFIXES}


def test_n_on_the_synthetic_bams(sample):
    d = sample["dir"]
    cli.run(sample["base"] + ["-o", d / "plain"])
    out = cli.run(sample["base"] + ["-N", "-o", d / "N"], env={"PGH_TIMING": "1"})
    assert "germline filter" in out.stderr
    check_expectations(reports(d / "plain"), reports(d / "N"))
    cli.run(sample["base"] + ["-N", "false", "-o", d / "N_false"])
    assert reports(d / "N_false") == reports(d / "plain")
    # the long name, and without read-pair discovery (-R false never fills the list IsGoodINV counts in either)
    cli.run(sample["base"] + ["--NormalSamples", "-R", "false", "-o", d / "N_noR"])
    assert reports(d / "N_noR") == reports(d / "N")


def test_n_does_not_depend_on_threads_or_devices(sample):
    d = sample["dir"]
    runs = {"t1": ["-T", "1"], "t8": ["-T", "8"], "g1": ["-G", "0"], "g2": ["-G", "0,0"]}
    for k, extra in runs.items():
        cli.run(sample["base"] + ["-N"] + extra + ["-o", d / k])
    want = reports(d / "t1")
    assert [gs.planted(b) for b in gs.blocks(want["TD"])] == ["TD_a", "TD_c"]
    for k in ("t8", "g1", "g2"):
        assert reports(d / k) == want, k


def test_n_changes_nothing_for_text_input(tmp_path):
    fa, reads_txt = gu.unpack(tmp_path)
    out = cli.run(["-f", fa, "-p", reads_txt, "-N", "-o", tmp_path / "N"])
    assert "close end 14862, far end 10968" in out.stdout
    gu.assert_reports_match_gold(str(tmp_path / "N"))


def test_mixed_input_is_a_usage_error(sample, tmp_path):
    out = cli.run(sample["base"] + ["-p", sample["reads_txt"], "-o", tmp_path / "x"], expect=2)
    assert "mixed input is not supported" in out.stderr
