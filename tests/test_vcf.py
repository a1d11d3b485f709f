"""pindel_pg2vcf / hostlib.reports_to_vcf: Pindel's pindel2vcf (pindel_amd/csrc/host/pg_vcf.hpp), pinned byte for byte.

  * The reference's own regression target: its gold reports (tests/golden/sim1chrVs2) through
    `pindel2vcf -R SIMCHROM -r sim1chrVs2.fa -P simulated_test.out -d 00000000` give its gold VCF.
  * tests/golden/vcf: outputs of the reference converter for a flag matrix on the gold reports, for the reports of the
    text route, and for a two-sample synthetic report set (tests/golden/vcf/README.md has every command line).
  * The text route end to end on the CPU: oracle search -> call_from_points (-l) -> converter.
  * Errors: exit status 1 and no output file.
"""
import gzip
import os
import shutil
import subprocess

import pytest

from oracle import pyoracle
from pindel_amd import hostio, hostlib
from tests import golden_util as gu

FX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vcf")
SUFFIXES = ("D", "SI", "LI", "INV", "TD")


def _gunzip(src, dst):
    with gzip.open(src, "rb") as s, open(dst, "wb") as d:
        shutil.copyfileobj(s, d)
    return str(dst)


def _gold_vcf():
    return gzip.open(os.path.join(gu.GOLD, "simulated_test.out.vcf.gz")).read()


def _gold_inputs(tmp_path):
    """sim1chrVs2.fa and the gold reports under tmp_path/gold/simulated_test.out_*; returns (fasta, prefix)"""
    fa = _gunzip(os.path.join(gu.GOLD, "sim1chrVs2.fa.gz"), tmp_path / "sim1chrVs2.fa")
    (tmp_path / "gold").mkdir(exist_ok=True)
    prefix = str(tmp_path / "gold" / "simulated_test.out")
    for s in SUFFIXES:
        _gunzip(os.path.join(gu.GOLD, f"simulated_test.out_{s}.gz"), f"{prefix}_{s}")
    return fa, prefix


def _text_route_reports(prefix):
    """The gold reports as the text route writes them: `0 0` reference coverage, LI 6 with `- 2` (tests/test_li_pin.py)"""
    for s in SUFFIXES:
        lines = []
        for line in gzip.open(os.path.join(gu.GOLD, f"simulated_test.out_{s}.gz")).read().split(b"\n"):
            line = b"\n".join(gu.normalise(line)).replace(b" X X ", b" 0 0 ")
            if line.startswith(b"6\tLI\t"):
                line = line.replace(b"- 8\tSIM1CHRVS2 + 4 - 8", b"- 2\tSIM1CHRVS2 + 4 - 2")
            lines.append(line)
        with open(f"{prefix}_{s}", "wb") as f:
            f.write(b"\n".join(lines))


def _synth_inputs(tmp_path):
    d = os.path.join(FX, "synth")
    fa = _gunzip(os.path.join(d, "synth.fa.gz"), tmp_path / "synth.fa")
    (tmp_path / "synth").mkdir(exist_ok=True)
    prefix = str(tmp_path / "synth" / "synth")
    for s in SUFFIXES:
        _gunzip(os.path.join(d, f"synth_{s}.gz"), f"{prefix}_{s}")
    return fa, prefix


def _cases():
    out = []
    with open(os.path.join(FX, "cases.tsv")) as f:
        for line in f:
            if line.startswith("#") or not line.strip():
                continue
            name, inp, flags = (line.rstrip("\n").split("\t") + [""])[:3]
            out.append((name, inp, flags.split()))
    return out


INPUTS = {"gold": ("SIMCHROM", "00000000"), "text": ("SIMCHROM", "00000000"), "synth": ("SYNTH", "20261015")}


def _inputs(tmp_path, inp):
    if inp == "synth":
        return _synth_inputs(tmp_path)
    fa, prefix = _gold_inputs(tmp_path)
    if inp == "text":
        prefix = str(tmp_path / "text_route.out")
        _text_route_reports(prefix)
    return fa, prefix


def _cli(args, timeout=120):
    return subprocess.run([hostlib.vcf_cli()] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)


def test_gold_reports_give_the_gold_vcf(tmp_path):
    fa, prefix = _gold_inputs(tmp_path)
    out = _cli(["-R", "SIMCHROM", "-r", fa, "-P", prefix, "-d", "00000000"])
    assert out.returncode == 0, out.stdout + out.stderr
    got = open(prefix + ".vcf", "rb").read()     # -v defaults to <-P>.vcf
    assert got == _gold_vcf()
    assert sum(1 for l in got.split(b"\n") if l and not l.startswith(b"#")) == 37


def test_gold_reports_give_the_gold_vcf_through_hostlib(tmp_path):
    fa, prefix = _gold_inputs(tmp_path)
    out = hostlib.reports_to_vcf(fa, tmp_path / "py.vcf", prefix=prefix, reference_name="SIMCHROM", reference_date="00000000")
    assert open(out, "rb").read() == _gold_vcf()


def test_one_report_with_p(tmp_path):
    """-p reads one file; its VCF holds the gold records of that type (the deletions), in the gold order"""
    fa, prefix = _gold_inputs(tmp_path)
    out = _cli(["-R", "SIMCHROM", "-r", fa, "-p", prefix + "_D", "-d", "00000000"])
    assert out.returncode == 0, out.stdout + out.stderr
    got = open(prefix + "_D.vcf", "rb").read().split(b"\n")
    want = [l for l in _gold_vcf().split(b"\n") if l.startswith(b"#") or b"SVTYPE=DEL" in l or b"SVTYPE=RPL" in l]
    assert [l for l in got if l] == want


@pytest.mark.parametrize("name,inp,flags", _cases(), ids=[c[0] for c in _cases()])
def test_fixture(tmp_path, name, inp, flags):
    fa, prefix = _inputs(tmp_path, inp)
    R, d = INPUTS[inp]
    want = gzip.open(os.path.join(FX, name)).read()
    out = _cli(["-r", fa, "-R", R, "-d", d, "-P", prefix, "-v", tmp_path / "cli.vcf"] + flags)
    assert out.returncode == 0, out.stdout + out.stderr
    assert open(tmp_path / "cli.vcf", "rb").read() == want


def _kw(flags):
    """pindel2vcf flags -> reports_to_vcf keywords"""
    by_flag = {flag: key for key, (_, flag) in hostlib.VCF_FLAGS.items()}
    kw, i = {}, 0
    while i < len(flags):
        key = by_flag[flags[i]]
        if flags[i] in ("-G", "-b", "-sb"):
            kw[key] = True
            i += 1
        else:
            kw[key] = flags[i + 1] if key == "chromosome" else float(flags[i + 1]) if key.endswith("cutoff") else int(flags[i + 1])
            i += 2
    return kw


@pytest.mark.parametrize("name,inp,flags", _cases(), ids=[c[0] for c in _cases()])
def test_fixture_through_hostlib(tmp_path, name, inp, flags):
    fa, prefix = _inputs(tmp_path, inp)
    R, d = INPUTS[inp]
    out = hostlib.reports_to_vcf(fa, tmp_path / "py.vcf", prefix=prefix, reference_name=R, reference_date=d, **_kw(flags))
    assert open(out, "rb").read() == gzip.open(os.path.join(FX, name)).read()


def test_every_flag_of_the_matrix_changes_its_output():
    """the fixtures pin something: each flagged output differs from the unflagged one of its input"""
    base = {"gold": _gold_vcf(), "synth": gzip.open(os.path.join(FX, "synth.default.vcf.gz")).read()}
    for name, inp, flags in _cases():
        if flags:
            assert gzip.open(os.path.join(FX, name)).read() != base[inp], name


def test_text_route_end_to_end_on_the_cpu(tmp_path):
    """oracle search of the gold reads -> call_from_points with -l -> converter == the text-route fixture"""
    fa, reads_txt = gu.unpack(tmp_path)
    chroms = hostio.load_fasta(fa)
    batch = hostio.read_pindel_text(reads_txt, [n for n, _ in chroms], [len(s) - hostio.SPACER * 2 for _, s in chroms])
    r = pyoracle.search_batch(pyoracle.make_params(), [s for _, s in chroms], batch.seq, batch.seq_off, batch.anchor_strand,
                              batch.anchor_pos, batch.insert_size, batch.chr_id)
    co, cp = gu.csr_from_strided(r["close_cnt"], r["close_pts"])
    fo, fp = gu.csr_from_strided(r["far_cnt"], r["far_pts"])
    st = hostlib.default_settings(pyoracle.max_mismatch_table())
    st.analyze_li = 1
    prefix = str(tmp_path / "P")
    hostlib.call_from_points(fa, reads_txt, prefix, st, co, cp, fo, fp, r["rc_flag"])
    want = gzip.open(os.path.join(FX, "text_route.vcf.gz")).read()
    out = _cli(["-R", "SIMCHROM", "-r", fa, "-P", prefix, "-d", "00000000"])
    assert out.returncode == 0, out.stdout + out.stderr
    assert open(prefix + ".vcf", "rb").read() == want
    hostlib.reports_to_vcf(fa, tmp_path / "py.vcf", prefix=prefix, reference_name="SIMCHROM", reference_date="00000000")
    assert open(tmp_path / "py.vcf", "rb").read() == want


def test_last_summary_line_without_newline(tmp_path):
    """the reference does not convert a summary line that ends the last report without a newline; one that ends an
    earlier report is converted"""
    fa, prefix = _gold_inputs(tmp_path)
    one = str(tmp_path / "one_D")
    line = [l for l in open(prefix + "_D") if l.startswith("0\tD ")][0].rstrip("\n")
    with open(one, "w") as f:
        f.write(line)
    out = _cli(["-R", "S", "-r", fa, "-p", one, "-d", "1"])
    assert out.returncode == 0, out.stdout + out.stderr
    assert not [l for l in open(one + ".vcf") if not l.startswith("#")]
    with open(one, "a") as f:
        f.write("\n")
    assert _cli(["-R", "S", "-r", fa, "-p", one, "-d", "1"]).returncode == 0
    assert len([l for l in open(one + ".vcf") if not l.startswith("#")]) == 1
    two = str(tmp_path / "two")
    with open(two + "_D", "w") as f:
        f.write(line)
    shutil.copy(prefix + "_TD", two + "_TD")
    assert _cli(["-R", "S", "-r", fa, "-P", two, "-d", "1"]).returncode == 0
    body = [l for l in open(two + ".vcf") if not l.startswith("#")]
    assert len(body) == 1 + 3 and sum("SVTYPE=DEL" in l for l in body) == 1


def test_help_lists_every_flag():
    out = _cli(["-h"])
    assert out.returncode == 0
    for short, long in [("-r", "--reference"), ("-R", "--reference_name"), ("-d", "--reference_date"), ("-p", "--pindel_output"),
                        ("-P", "--pindel_output_root"), ("-v", "--vcf"), ("-c", "--chromosome"), ("-w", "--window_size"),
                        ("-mc", "--min_coverage"), ("-he", "--het_cutoff"), ("-ho", "--hom_cutoff"), ("-is", "--min_size"),
                        ("-as", "--max_size"), ("-b", "--both_strands_supported"), ("-m", "--min_supporting_samples"),
                        ("-e", "--min_supporting_reads"), ("-f", "--max_supporting_reads"), ("-sr", "--region_start"),
                        ("-er", "--region_end"), ("-ir", "--max_internal_repeats"), ("-il", "--max_internal_repeatlength"),
                        ("-pr", "--max_postindel_repeats"), ("-pl", "--max_postindel_repeatlength"),
                        ("-co", "--compact_output_limit"), ("-sb", "--only_balanced_samples"),
                        ("-ss", "--minimum_strand_support"), ("-G", "--gatk_compatible"), ("-h", "--help")]:
        assert f"  {short}/{long}  " in out.stdout, short
    assert _cli([]).returncode == 0   # no arguments: the help, like the reference


def test_long_flag_names(tmp_path):
    fa, prefix = _gold_inputs(tmp_path)
    out = _cli(["--reference_name", "SIMCHROM", "--reference", fa, "--pindel_output_root", prefix, "--reference_date", "00000000",
                "--vcf", tmp_path / "long.vcf", "--gatk_compatible", "--compact_output_limit", "50"])
    assert out.returncode == 0, out.stdout + out.stderr
    want = _cli(["-R", "SIMCHROM", "-r", fa, "-P", prefix, "-d", "00000000", "-v", tmp_path / "short.vcf", "-G", "-co", "50"])
    assert want.returncode == 0
    assert open(tmp_path / "long.vcf", "rb").read() == open(tmp_path / "short.vcf", "rb").read() != _gold_vcf()


def _fails(args, tmp_path, what):
    out = _cli(args)
    assert out.returncode == 1, (args, out.stdout, out.stderr)
    assert what in out.stdout + out.stderr, (what, out.stdout, out.stderr)


def test_errors(tmp_path):
    fa, prefix = _gold_inputs(tmp_path)
    v = tmp_path / "e.vcf"
    ok = ["-r", fa, "-R", "S", "-d", "1", "-P", prefix, "-v", v]
    for k in ("-r", "-R", "-d"):
        args = list(ok)
        i = args.index(k)
        del args[i:i + 2]
        _fails(args, tmp_path, f"required parameter {k}/")
    _fails(ok + ["-p", prefix + "_D"], tmp_path, "-p and -P cannot be used together")
    _fails(["-r", fa, "-R", "S", "-d", "1", "-v", v], tmp_path, "-p <report> or -P <prefix>")
    _fails(["-r", fa, "-R", "S", "-d", "1", "-P", tmp_path / "nothing_here", "-v", v], tmp_path, "does not exist")
    _fails(["-r", fa, "-R", "S", "-d", "1", "-p", tmp_path / "nothing_here_D", "-v", v], tmp_path, "does not exist")
    _fails(ok + ["-w", "0"], tmp_path, "-w must be at least 1")
    _fails(ok + ["-x", "1"], tmp_path, "unknown argument")
    _fails(ok + ["-w"], tmp_path, "lacking")
    _fails(ok + ["-co", "-1"], tmp_path, "seems erroneous")
    _fails(["-r", tmp_path / "no.fa", "-R", "S", "-d", "1", "-P", prefix, "-v", v], tmp_path, "Cannot open reference file")
    assert not v.exists()
    # a record on a chromosome that is not in the FASTA: an LI record (the reference's error) and a deletion
    for suf, old, new in (("LI", b"\tChrID 1\t", b"\tChrID chrX\t"), ("D", b"\tChrID 1\t", b"\tChrID chrX\t")):
        other = str(tmp_path / f"other_{suf}")
        data = open(f"{prefix}_{suf}", "rb").read()
        assert old in data
        with open(other, "wb") as f:
            f.write(data.replace(old, new, 1))
        _fails(["-r", fa, "-R", "S", "-d", "1", "-p", other, "-v", v], tmp_path, 'Reference chromosome "chrX" not found')
        assert not v.exists()
    # hostlib: the same errors as exceptions
    with pytest.raises(RuntimeError, match="-w must be at least 1"):
        hostlib.reports_to_vcf(fa, v, prefix=prefix, reference_name="S", reference_date="1", window_size=0)
    with pytest.raises(RuntimeError, match="cannot be used together"):
        hostlib.reports_to_vcf(fa, v, prefix=prefix, report=prefix + "_D", reference_name="S", reference_date="1")
    with pytest.raises(RuntimeError, match="does not exist"):
        hostlib.reports_to_vcf(fa, v, prefix=str(tmp_path / "none"), reference_name="S", reference_date="1")
    with pytest.raises(ValueError, match="unknown flag"):
        hostlib.reports_to_vcf(fa, v, prefix=prefix, reference_name="S", reference_date="1", no_such_flag=1)
    assert not v.exists()


def test_fasta_header_text_and_order(tmp_path):
    """a header's name ends at a space, tab or '\\r'; chromosomes are written in FASTA order and ones without events are
    skipped"""
    fa, prefix = _gold_inputs(tmp_path)
    seq = "".join(l.strip() for l in open(fa) if not l.startswith(">"))
    crlf = tmp_path / "crlf.fa"
    with open(crlf, "w", newline="") as f:
        f.write(">chrEmpty\r\nACGTACGT\r\n>1\tsim chromosome\r\n")
        for k in range(0, len(seq), 60):
            f.write(seq[k:k + 60] + "\r\n")
    out = _cli(["-R", "SIMCHROM", "-r", crlf, "-P", prefix, "-d", "00000000", "-v", tmp_path / "crlf.vcf"])
    assert out.returncode == 0, out.stdout + out.stderr
    assert open(tmp_path / "crlf.vcf", "rb").read() == _gold_vcf()
