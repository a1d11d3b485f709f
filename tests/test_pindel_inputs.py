"""-P (a list of Pindel-text files) and gzipped Pindel-text input on the host: hostlib.call_from_points with reads_config=,
points from the CPU oracle on the gold reads (tests/golden/sim1chrVs2)."""
import gzip
import os

import pytest

from oracle import pyoracle
from pindel_amd import hostio, hostlib
from tests import golden_util as gu

CUT = 6000            # reads in the first part


@pytest.fixture(scope="module")
def gold(tmp_path_factory):
    d = tmp_path_factory.mktemp("inputs")
    fa, reads_txt = gu.unpack(d)
    chroms = hostio.load_fasta(fa)
    batch = hostio.read_pindel_text(reads_txt, [n for n, _ in chroms], [len(s) - 200000 for _, s in chroms])
    r = pyoracle.search_batch(pyoracle.make_params(), [s for _, s in chroms], batch.seq, batch.seq_off, batch.anchor_strand,
                              batch.anchor_pos, batch.insert_size, batch.chr_id)
    co, cp = gu.csr_from_strided(r["close_cnt"], r["close_pts"])
    fo, fp = gu.csr_from_strided(r["far_cnt"], r["far_pts"])
    lines = open(reads_txt, "rb").read().split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) == 3 * batch.n
    a, b = b"\n".join(lines[:3 * CUT]) + b"\n", b"\n".join(lines[3 * CUT:])         # cut at a record boundary
    (d / "A.txt").write_bytes(a)
    with gzip.open(d / "B.txt.gz", "wb") as f:
        f.write(b)
    return dict(dir=d, fasta=fa, reads_txt=reads_txt, a=a, b=b, points=(co, cp, fo, fp, r["rc_flag"]),
                settings=hostlib.default_settings(pyoracle.max_mismatch_table()))


def call(g, prefix, reads_txt=None, **kw):
    hostlib.call_from_points(g["fasta"], reads_txt, str(prefix), g["settings"], *g["points"], **kw)
    return {suf: open(f"{prefix}_{suf}", "rb").read() for suf in gu.SUFFIXES}


def test_config_of_a_plain_and_a_gzipped_part_gives_the_gold_reports(gold):
    d = gold["dir"]
    cfg = d / "parts.cfg"
    # the first token of a line is the file, the rest is ignored; a relative name is looked up beside the configuration
    cfg.write_text(f"{d / 'A.txt'}\tsampleA 500 anything else\n\nB.txt.gz\n")
    call(gold, d / "cfg", reads_config=str(cfg))
    gu.assert_reports_match_gold(str(d / "cfg"))
    # the whole file gzipped through -p's route, and as two gzip members back to back
    with gzip.open(d / "whole.txt.gz", "wb") as f:
        f.write(gold["a"] + gold["b"])
    call(gold, d / "gz", reads_txt=str(d / "whole.txt.gz"))
    gu.assert_reports_match_gold(str(d / "gz"))
    (d / "members.txt.gz").write_bytes(gzip.compress(gold["a"]) + gzip.compress(gold["b"]))
    call(gold, d / "members", reads_txt=str(d / "members.txt.gz"))
    gu.assert_reports_match_gold(str(d / "members"))
    # -P and -p together: the -P files come first, then the -p file
    (d / "only_a.cfg").write_text(f"{d / 'A.txt'}\n")
    call(gold, d / "both", reads_txt=str(d / "B.txt.gz"), reads_config=str(d / "only_a.cfg"))
    gu.assert_reports_match_gold(str(d / "both"))


def test_two_samples_listed_equal_their_concatenation(gold):
    d = gold["dir"]
    b2 = gold["b"].replace(b"\tSIM1CHRVS2\n", b"\tSECOND\n")
    assert b2 != gold["b"] and b2.count(b"\tSECOND\n") == gold["b"].count(b"\n") // 3
    (d / "B2.txt").write_bytes(b2)
    (d / "cat.txt").write_bytes(gold["a"] + b2)
    listed = call(gold, d / "listed", reads_config=[d / "A.txt", d / "B2.txt"])
    whole = call(gold, d / "whole", reads_txt=str(d / "cat.txt"))
    assert listed == whole
    # both samples reach the reports, and some events carry reads of both
    every = b"".join(whole.values())
    assert b"\tSECOND\t@" in every and b"\tSIM1CHRVS2\t@" in every and b"NumSupSamples 2\t2\t" in every


def test_last_line_without_a_newline_is_used(gold):
    d = gold["dir"]
    cfg = d / "no_newline.cfg"
    cfg.write_bytes(f"{d / 'A.txt'}\n{d / 'B.txt.gz'}".encode())
    call(gold, d / "nonl", reads_config=str(cfg))
    gu.assert_reports_match_gold(str(d / "nonl"))


def test_error_cases(gold, tmp_path):
    d = gold["dir"]
    cfg = tmp_path / "missing.cfg"
    cfg.write_text(f"{d / 'A.txt'}\nnot_there.txt\n")
    with pytest.raises(RuntimeError) as e:
        call(gold, tmp_path / "x", reads_config=str(cfg))
    assert "not_there.txt" in str(e.value) and "missing.cfg" in str(e.value)           # the message names both
    empty = tmp_path / "empty.cfg"
    empty.write_text("\n   \n")
    with pytest.raises(RuntimeError, match="empty.cfg"):
        call(gold, tmp_path / "x", reads_config=str(empty))
    with pytest.raises(RuntimeError, match="nowhere.cfg"):
        call(gold, tmp_path / "x", reads_config=str(tmp_path / "nowhere.cfg"))
    # a .gz that does not inflate is an error, never a short read list: damaged in the middle, cut short, not gzip at all
    whole = gzip.compress(gold["a"] + gold["b"])
    damaged = bytearray(whole)
    for k in range(len(whole) // 2, len(whole) // 2 + 64):
        damaged[k] ^= 0x5a
    for name, data in (("damaged.txt.gz", bytes(damaged)), ("cut.txt.gz", whole[:len(whole) // 2]), ("plain.txt.gz", gold["a"] + gold["b"]),
                       ("trailing.txt.gz", whole + b"junk")):
        (tmp_path / name).write_bytes(data)
        with pytest.raises(RuntimeError, match=name):
            call(gold, tmp_path / "x", reads_txt=str(tmp_path / name))
    # the reference's rule for the suffix: longer than three characters and ending in .gz; nothing else is inflated
    os.makedirs(tmp_path / "sub", exist_ok=True)
    (tmp_path / "sub" / "reads.gzip").write_bytes(gold["a"] + gold["b"])
    call(gold, tmp_path / "sub" / "ok", reads_txt=str(tmp_path / "sub" / "reads.gzip"))
    gu.assert_reports_match_gold(str(tmp_path / "sub" / "ok"))


def test_command_line_checks_its_inputs_before_any_device(gold, tmp_path):
    """pindel_pg ends with status 1 on an unreadable configuration, a listed file that does not exist, a configuration
    without files and a .gz that does not inflate -- before it creates a device context, so also on a machine without a
    GPU; -i together with -p / -P is a usage error (status 2)."""
    import subprocess
    from pindel_amd import binding
    exe = os.path.join(os.path.dirname(binding.LIB_PATH), "pindel_pg")
    d = gold["dir"]

    def fails(args, status, *words):
        out = subprocess.run([exe, "-f", gold["fasta"], "-o", str(tmp_path / "x")] + [str(a) for a in args], capture_output=True,
                             text=True, timeout=60)
        assert out.returncode == status, (out.returncode, out.stderr[-500:])
        assert all(w in out.stderr for w in words), out.stderr[-500:]
        assert "pg_create" not in out.stderr
    (tmp_path / "missing.cfg").write_text(f"{d / 'A.txt'}\nnot_there.txt\n")
    fails(["-P", tmp_path / "missing.cfg"], 1, "not_there.txt", "missing.cfg")
    (tmp_path / "empty.cfg").write_text("\n")
    fails(["-P", tmp_path / "empty.cfg"], 1, "empty.cfg")
    fails(["-P", tmp_path / "nowhere.cfg"], 1, "nowhere.cfg")
    whole = gzip.compress(gold["a"] + gold["b"])
    (tmp_path / "cut.txt.gz").write_bytes(whole[:len(whole) // 2])
    fails(["-p", tmp_path / "cut.txt.gz"], 1, "cut.txt.gz")
    (tmp_path / "cut.cfg").write_text(f"{d / 'A.txt'}\n{tmp_path / 'cut.txt.gz'}\n")
    fails(["-P", tmp_path / "cut.cfg"], 1, "cut.txt.gz")
    fails(["-P", tmp_path / "cut.cfg", "-i", tmp_path / "bams.cfg"], 2, "mixed input is not supported")
    fails(["-p", d / "A.txt", "-i", tmp_path / "bams.cfg"], 2, "mixed input is not supported")
