"""-m gpu: `pindel_pg --repair` on the MI355X against the oracle-fed host pipeline with the same repairs
(hostlib.call_from_points: the reads as the BAM ingest delivers them, points from the CPU oracle, the window hints through the
host library's C entry), on the -I sample of tests/interchr_synth.py and the two-sample synthetic of tests/repair_synth.py.
Every run goes through tests/cli_chain.run: a time limit of its own, and nothing is started after an abnormal exit."""
import os

import numpy as np
import pytest

from oracle import pyoracle
from pindel_amd import hostio, hostlib
from tests import cli_chain as cli
from tests import golden_util as gu
from tests import interchr_common as ic
from tests import interchr_restated as ir
from tests import interchr_synth as syn
from tests import repair_restated as rr
from tests import repair_synth as rs
from tests.test_bam_ingest import ingest
from tests.test_repair_cpu import DROPPED, SUFFIXES, assert_every_junction_is_called, check_fixture, expected

pytestmark = pytest.mark.gpu
SPACER = ic.SPACER


# ------------------------------------------------------------------------------------------------ -I --repair int-pairs
def _bam_route(s, d):
    """The windows of `pindel_pg -i -I` as run_bam_pipeline walks them (the way of test_gpu_interchr.py): ingest, oracle close
    end, the window's hints (read pairs of both kinds), oracle far end.  -> (a Pindel-text file of the ingested reads, the CSR
    point arrays over it, the restatement's read lists per window)"""
    L = ic.lib()
    names = list(syn.NAMES)
    chroms = hostio.load_fasta(s["fasta"])
    lines, res_all, per_window = [], [], []
    for cid, (name, seq) in enumerate(chroms):
        for ws, we in syn.windows():
            got = ingest(s["bam"], name, cid, len(seq), ws, we, syn.ISZ, tag=syn.TAG)
            if not got:
                continue
            # the text pipeline bins a read by its position: the two routes walk the same windows only if every read lies in its own
            assert all(ws <= g[3] < we for g in got), (name, ws)
            b = ic.batch_of(got, cid)

            def windows_of(last):
                off = np.zeros(b.n + 1, dtype=np.uint64)
                win = np.zeros(3 * 8192, dtype=np.int32)
                n_ev = L.pgh_window_hints_chr(None, s["bam"].encode(), len(names), ic.c_names(names), cid, ws, we, we, syn.ISZ,
                                              syn.TAG.encode(), 0, SPACER, 1, b.n, last.ctypes.data, off.ctypes.data, win.ctypes.data, 8192,
                                              None, 0)
                assert n_ev >= 0, L.pgh_last_error()
                return off, win[:3 * int(off[-1])]
            res = ic.oracle_with_windows(chroms, b, windows_of)
            res_all.append(res)
            lines += [f"{g[0]}\n{g[1]}\n{g[2]}\t{name}\t{g[3]}\t{g[4]}\t{g[5]}\t{syn.TAG}\n" for g in got]
            per_window.append(ic.restated_reads(names, chroms, got, res, name))
    reads_txt = d / "ingested.txt"
    reads_txt.write_text("".join(lines))
    cat = {k: np.concatenate([r[k] for r in res_all]) for k in ("close_cnt", "far_cnt", "rc_flag")}
    co, cp = gu.csr_from_strided(cat["close_cnt"], np.concatenate([r["close_pts"] for r in res_all]))
    fo, fp = gu.csr_from_strided(cat["far_cnt"], np.concatenate([r["far_pts"] for r in res_all]))
    return str(reads_txt), (co, cp, fo, fp, cat["rc_flag"]), per_window


def test_int_pairs_equals_the_oracle_fed_pipeline(tmp_path):
    s = syn.make(str(tmp_path))
    reads_txt, csr, per_window = _bam_route(s, tmp_path)
    st = hostlib.default_settings(pyoracle.max_mismatch_table())
    st.window_mbp = float(syn.WINDOW_MBP)
    st.report_interchromosomal = 1
    base = ["-f", s["fasta"], "-i", s["config"], "-w", syn.WINDOW_MBP, "-I"]
    for name, repairs in (("repaired", "int-pairs"), ("as_is", None)):
        hostlib.call_from_points(s["fasta"], reads_txt, str(tmp_path / f"host_{name}"), st, *csr, repairs=repairs)
        out = cli.run(base + (["--repair", repairs] if repairs else []) + ["-o", tmp_path / f"gpu_{name}"])
        assert ("repairs in effect: int-pairs" in out.stdout) == bool(repairs)
        for suf in ("_INT", "_INT_final"):
            assert cli.read(f"{tmp_path}/gpu_{name}{suf}") == cli.read(f"{tmp_path}/host_{name}{suf}"), (name, suf)
    # ... which is the restatement's text, holds all three chromosome pairs, and starts with the unrepaired lines in every window
    got = cli.read(tmp_path / "gpu_repaired_INT").decode()
    assert got == "".join(rr.int_lines_all_pairs(w, SPACER)[0] for w in per_window)
    assert_every_junction_is_called(got)
    assert cli.read(tmp_path / "gpu_as_is_INT").decode() == "".join(ir.int_lines(w, SPACER)[0] for w in per_window)
    assert all(rr.int_lines_all_pairs(w, SPACER)[0].startswith(ir.int_lines(w, SPACER)[0]) for w in per_window)
    # the other reports and _RP do not depend on the repair
    for suf in ("_D", "_SI", "_TD", "_INV", "_RP"):
        assert cli.read(f"{tmp_path}/gpu_repaired{suf}") == cli.read(f"{tmp_path}/gpu_as_is{suf}"), suf


# ------------------------------------------------------------------------------------------------ -N --repair inv-pairs,depth-mapq
@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    d = tmp_path_factory.mktemp("repair_gpu")
    s = rs.make(str(d))
    chroms = hostio.load_fasta(s["fasta"])
    b = hostio.read_pindel_text(s["reads_txt"], [n for n, _ in chroms], [len(q) - 200000 for _, q in chroms])
    p = pyoracle.make_params(max_range_index=rs.MAX_RANGE_INDEX)
    r = pyoracle.search_batch(p, [q for _, q in chroms], b.seq, b.seq_off, b.anchor_strand, b.anchor_pos, b.insert_size, b.chr_id)
    co, cp = gu.csr_from_strided(r["close_cnt"], r["close_pts"])
    fo, fp = gu.csr_from_strided(r["far_cnt"], r["far_pts"])
    s["points"] = (co, cp, fo, fp, r["rc_flag"])
    s["dir"] = d
    s["base"] = ["-f", s["fasta"], "-i", s["config"], "-x", rs.MAX_RANGE_INDEX, "-l"]
    return s


def host(s, name, **kw):
    st = hostlib.default_settings(pyoracle.max_mismatch_table())
    st.analyze_li = 1
    prefix = str(s["dir"] / name)
    hostlib.call_from_points(s["fasta"], s["reads_txt"], prefix, st, *s["points"], **kw)
    return {suf: cli.read(f"{prefix}_{suf}") for suf in SUFFIXES}


def reports(prefix):
    return {suf: cli.read(f"{prefix}_{suf}") for suf in SUFFIXES}


def test_inv_pairs_and_depth_mapq_equal_the_oracle_fed_pipeline(sample):
    d = sample["dir"]
    check_fixture(sample, host(sample, "host_plain"))
    cli.run(sample["base"] + ["-o", d / "plain"])
    plain = reports(d / "plain")
    for repairs in ("inv-pairs,depth-mapq", None, "inv-pairs", "depth-mapq"):
        name = (repairs or "none").replace(",", "_")
        out = cli.run(sample["base"] + ["-N"] + (["--repair", repairs] if repairs else []) + ["-o", d / name])
        assert (f"repairs in effect: {repairs}\n" in out.stdout) if repairs else ("repairs in effect" not in out.stdout)
        got, want = reports(d / name), host(sample, "host_" + name, normal_samples=True, bam_config=sample["config"], repairs=repairs)
        for suf in ("TD", "INV"):
            assert got[suf] == want[suf], (repairs, suf)
        # ... and the command line's own run without -N minus the dropped blocks, every report
        assert got == expected(plain, DROPPED[repairs]), repairs
    # -R false: the pairs are still discovered for the filter, but give no hint and no _RP line
    cli.run(sample["base"] + ["-R", "false", "-o", d / "plain_noR"])
    cli.run(sample["base"] + ["-N", "--repair", "inv-pairs", "-R", "false", "-o", d / "inv_noR"])
    assert reports(d / "inv_noR") == expected(reports(d / "plain_noR"), DROPPED["inv-pairs"])
    assert [rs.planted(b) for b in rs.blocks(cli.read(d / "inv_noR_INV"))] == ["INV_edge", "INV_both", "INV_s"]
    assert not os.path.exists(d / "inv_noR_RP") and cli.read(d / "inv-pairs_RP") == cli.read(d / "plain_RP") != b""
    # without -N the names change nothing
    cli.run(sample["base"] + ["--repair", "inv-pairs,depth-mapq", "-o", d / "no_N"])
    assert reports(d / "no_N") == plain


def test_repair_all_does_not_depend_on_threads_or_devices(sample):
    d = sample["dir"]
    runs = {"t1": ["-T", "1"], "t8": ["-T", "8"], "g1": ["-G", "0"], "g2": ["-G", "0,0"]}
    for k, extra in runs.items():
        cli.run(sample["base"] + ["-N", "--repair", "all"] + extra + ["-o", d / k])
    want = reports(d / "t1")
    assert [rs.planted(b) for b in rs.blocks(want["INV"])] == ["INV_edge", "INV_both", "INV_s"] and want["TD"] == b""
    for k in ("t8", "g1", "g2"):
        assert reports(d / k) == want, k


def test_without_the_flag_nothing_changes(tmp_path):
    """a sanity check on the gold sample: the reports of a run without --repair are the reference's"""
    fa, reads_txt = gu.unpack(tmp_path)
    out = cli.run(["-f", fa, "-p", reads_txt, "-o", tmp_path / "gold"])
    assert "repairs in effect" not in out.stdout and "close end 14862, far end 10968" in out.stdout
    gu.assert_reports_match_gold(str(tmp_path / "gold"))
