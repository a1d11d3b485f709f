"""-P (a list of Pindel-text files) and gzipped Pindel-text input through the command line, on the gold reads."""
import gzip

import pytest

from tests import cli_chain as cli
from tests import golden_util as gu

pytestmark = pytest.mark.gpu
REPORTS = ("_D", "_SI", "_TD", "_INV", "_LI", "_CloseEndMapped")


@pytest.fixture(scope="module")
def parts(tmp_path_factory):
    """the gold read file cut at record boundaries into A (plain), B (gzipped) and C (plain, another sample tag)"""
    d = tmp_path_factory.mktemp("inputs_gpu")
    fa, reads_txt = gu.unpack(d)
    lines = cli.read(reads_txt).split(b"\n")
    cut = lambda lo, hi: b"".join(x + b"\n" for x in lines[3 * lo:3 * hi])
    a, b, c = cut(0, 5000), cut(5000, 10000), cut(10000, 14862).replace(b"\tSIM1CHRVS2\n", b"\tTHIRD\n")
    assert a + b + cut(10000, 14862) == cli.read(reads_txt) and b"\tTHIRD\n" in c
    (d / "A.txt").write_bytes(a)
    (d / "B.txt.gz").write_bytes(gzip.compress(b))
    (d / "C.txt").write_bytes(c)
    (d / "ABC.txt").write_bytes(a + b + c)
    (d / "reads.txt.gz").write_bytes(gzip.compress(cli.read(reads_txt)))
    (d / "AB.cfg").write_text(f"{d / 'A.txt'}\tfirst sample\nB.txt.gz")          # a relative name, no final newline
    (d / "ABrest.cfg").write_text(f"{d / 'A.txt'}\n{d / 'B.txt.gz'}\n{d / 'rest.txt'}\n")
    (d / "rest.txt").write_bytes(cut(10000, 14862))
    return dict(dir=d, fasta=fa)


def test_config_and_gzip_give_the_gold_reports(parts):
    d, fa = parts["dir"], parts["fasta"]
    out = cli.run(["-f", fa, "-P", d / "ABrest.cfg", "-o", d / "P"])
    assert "close end 14862, far end 10968" in out.stdout
    gu.assert_reports_match_gold(str(d / "P"))
    out = cli.run(["-f", fa, "-p", d / "reads.txt.gz", "-o", d / "gz"])
    assert "close end 14862, far end 10968" in out.stdout
    gu.assert_reports_match_gold(str(d / "gz"))


def test_config_then_file_equals_the_concatenation(parts):
    d, fa = parts["dir"], parts["fasta"]
    cli.run(["-f", fa, "--pindel-config-file", d / "AB.cfg", "-p", d / "C.txt", "-l", "-s", "-o", d / "PC"])
    cli.run(["-f", fa, "-p", d / "ABC.txt", "-l", "-s", "-o", d / "cat"])
    for suf in REPORTS:
        assert cli.read(f"{d}/PC{suf}") == cli.read(f"{d}/cat{suf}"), suf
    assert b"\tTHIRD\t@" in cli.read(f"{d}/cat_D") + cli.read(f"{d}/cat_SI") + cli.read(f"{d}/cat_INV")


def test_bad_inputs_end_the_run_before_the_search(parts, tmp_path):
    d, fa = parts["dir"], parts["fasta"]
    (tmp_path / "missing.cfg").write_text(f"{d / 'A.txt'}\nnot_there.txt\n")
    out = cli.run(["-f", fa, "-P", tmp_path / "missing.cfg", "-o", tmp_path / "x"], expect=1)
    assert "not_there.txt" in out.stderr and "missing.cfg" in out.stderr
    (tmp_path / "empty.cfg").write_text("\n")
    out = cli.run(["-f", fa, "-P", tmp_path / "empty.cfg", "-o", tmp_path / "x"], expect=1)
    assert "empty.cfg" in out.stderr
    out = cli.run(["-f", fa, "-P", tmp_path / "nowhere.cfg", "-o", tmp_path / "x"], expect=1)
    assert "nowhere.cfg" in out.stderr
    whole = cli.read(d / "reads.txt.gz")
    (tmp_path / "cut.txt.gz").write_bytes(whole[:len(whole) // 2])
    out = cli.run(["-f", fa, "-p", tmp_path / "cut.txt.gz", "-o", tmp_path / "x"], expect=1)
    assert "cut.txt.gz" in out.stderr
