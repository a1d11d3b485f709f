"""The product's _LI (SortOutputLI, src/reporter.cpp:1853-2141) and _CloseEndMapped (ReportCloseMappedReads,
src/pindel.cpp:1076-1092) reports: `pindel_pg -l / -s / -S` and hostlib.call_from_points(analyze_li, report_close_mapped).

  * CPU: oracle points for the sim1chrVs2 gold reads -> the gold _LI with exactly the text-route adjustment
    tests/test_li_pin.py derives (7 events byte for byte, LI 6 with 2 of its 8 '-' reads), for any number of host threads;
    _CloseEndMapped = its restatement here, and = the gold file except for the 30 reads the search reverse-complements;
    small windows and a synthetic two-chromosome set = tests/li_consumer.py window by window (Count_LI carried over,
    CurrentChrMask taken from the product's own reports of the windows so far, reset per chromosome).
  * GPU: the same bytes from the command line, on every device / flush layout, with -S, and on the BAM route.
"""
import gzip
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle
from pindel_amd import hostio, hostlib
from tests import golden_util as gu
from tests import li_consumer as li
from tests.test_li_pin import _expected_on_the_text_route, _records

ALL_SUFFIXES = ("D", "SI", "TD", "INV", "LI", "BP", "CloseEndMapped")
# the reads (record index in the gold file) whose close end the search finds only on the reverse complement
# (rc_flag 1): their _CloseEndMapped sequence is the reverse complement of the gold one (see
# test_close_end_mapped_restated_and_pinned_by_gold)
FLIPPED = [3624, 3625, 3626, 3627, 4656, 4657, 4658, 4659, 9668, 9669, 9670, 9671, 10864, 10865, 10866, 10867, 13334, 13335,
           14282, 14283, 14286, 14287, 14288, 14289, 14290, 14291, 14340, 14341, 14342, 14343]


def _oracle(chroms, batch):
    return pyoracle.search_batch(pyoracle.make_params(), [s for _, s in chroms], batch.seq, batch.seq_off, batch.anchor_strand,
                                 batch.anchor_pos, batch.insert_size, batch.chr_id)


def _gold_run(tmp_path):
    fa, reads_txt = gu.unpack(tmp_path)
    chroms = hostio.load_fasta(fa)
    batch = hostio.read_pindel_text(reads_txt, [n for n, _ in chroms], [len(s) - 200000 for _, s in chroms])
    return fa, reads_txt, chroms, _oracle(chroms, batch)


def _call(fa, reads_txt, prefix, r, window_mbp=5.0, li_on=True, cem_on=True, keep=None):
    """call_from_points with the oracle result r; keep (bool per read): only those reads (a shorter read file)"""
    close_cnt, close_pts, far_cnt, far_pts, rc = r["close_cnt"], r["close_pts"], r["far_cnt"], r["far_pts"], r["rc_flag"]
    if keep is not None:
        recs = [x for x, k in zip(_records(reads_txt), keep) if k]
        reads_txt = prefix + ".reads.txt"
        _write_text(reads_txt, recs)
        close_cnt, close_pts, far_cnt, far_pts, rc = close_cnt[keep], close_pts[keep], far_cnt[keep], far_pts[keep], rc[keep]
    co, cp = gu.csr_from_strided(close_cnt, close_pts)
    fo, fp = gu.csr_from_strided(far_cnt, far_pts)
    st = hostlib.default_settings(pyoracle.max_mismatch_table())
    st.window_mbp = window_mbp
    st.analyze_li = int(li_on)
    st.report_close_mapped = int(cem_on)
    hostlib.call_from_points(fa, reads_txt, prefix, st, co, cp, fo, fp, rc)


def _write_text(path, recs):
    with open(path, "w") as f:
        for name, seq, d, chrom, pos, ms, isz, tag in recs:
            f.write(f"{name}\n{seq}\n{d}\t{chrom}\t{pos}\t{ms}\t{isz}\t{tag}\n")


def _flip(seq: bytes, flag: int) -> bytes:
    """setUnmatchedSeq(ReverseComplement()) once or twice (pg_adapter.hpp apply_rc_flag): \\0 outside ACGTN, trailing
    non-alphanumerics dropped"""
    for _ in range(min(int(flag), 2)):
        seq = li.reverse_complement(seq)
        while seq and not chr(seq[-1]).isalnum():
            seq = seq[:-1]
    return seq


def _close_end_mapped(recs, close_cnt, rc_flag) -> bytes:
    """ReportCloseMappedReads restated: the reads with a close end, in input order, as GetCloseEnd left them."""
    out = []
    for (name, seq, d, chrom, pos, ms, isz, tag), n, f in zip(recs, close_cnt, rc_flag):
        if n:
            out.append(name.encode() + b"\n" + _flip(seq.encode(), f) + f"\n{d}\t{chrom}\t{pos}\t{ms}\t{isz}\t{tag}\n".encode())
    return b"".join(out)


def _li_reads(recs, r, chr_name=None):
    """LIRead per read with a close end (input order), from the oracle result r"""
    out = []
    for i, (name, seq, d, chrom, pos, ms, isz, tag) in enumerate(recs):
        if not r["close_cnt"][i] or (chr_name is not None and chrom != chr_name):
            continue
        last = r["close_pts"][i][r["close_cnt"][i] - 1]
        x = li.LIRead()
        s = _flip(seq.encode(), r["rc_flag"][i])
        x.name, x.seq, x.strand, x.pos, x.ms, x.tag, x.frag = name, s, d, pos, ms, tag, chrom
        x.close_abs, x.close_len, x.has_far, x.length = int(last["abs_loc"]), int(last["length"]), bool(r["far_cnt"][i] > 0), len(s)
        out.append(x)
    return out


def _reports(prefix, chr_name=None):
    """the four SV reports of a run; with chr_name only the event headers of that chromosome"""
    out = {}
    for suf in gu.SUFFIXES:
        data = open(f"{prefix}_{suf}", "rb").read()
        if chr_name is not None:
            data = b"\n".join(l for l in data.split(b"\n") if f"\tChrID {chr_name}\t".encode() in l)
        out[suf] = data
    return out


# ------------------------------------------------------------------------------------------------------------ CPU
def test_oracle_li_equals_gold_on_the_text_route(tmp_path):
    fa, reads_txt, chroms, r = _gold_run(tmp_path)
    prefix = str(tmp_path / "o")
    _call(fa, reads_txt, prefix, r)
    gu.assert_reports_match_gold(prefix)                          # the four SV reports are unchanged by -l / -s
    got = open(prefix + "_LI", "rb").read().split(b"\n")
    want = _expected_on_the_text_route()
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"_LI line {k + 1}:\n got  {a[:160]!r}\n want {b[:160]!r}"
    assert sum(1 for l in got if b"\tLI\tChrID " in l) == 8
    # the defaults write neither report (existing callers see no new file)
    _call(fa, reads_txt, str(tmp_path / "d"), r, li_on=False, cem_on=False)
    assert not os.path.exists(str(tmp_path / "d_LI")) and not os.path.exists(str(tmp_path / "d_CloseEndMapped"))


def test_li_and_close_end_mapped_do_not_depend_on_host_threads(tmp_path, monkeypatch):
    """The reporters mark CurrentChrMask from several threads (for_boxes): the mask, and so _LI, is the same for any count."""
    fa, reads_txt, chroms, r = _gold_run(tmp_path)
    outs = {}
    for threads in ("1", "2", "7", "16"):
        monkeypatch.setenv("PGH_THREADS", threads)
        prefix = str(tmp_path / f"t{threads}")
        _call(fa, reads_txt, prefix, r)
        outs[threads] = [open(f"{prefix}_{s}", "rb").read() for s in ("LI", "CloseEndMapped")]
    assert outs["1"][0] == b"\n".join(_expected_on_the_text_route())
    assert outs["1"] == outs["2"] == outs["7"] == outs["16"]


def test_close_end_mapped_restated_and_pinned_by_gold(tmp_path):
    """_CloseEndMapped = the restatement (rc flag applied, input order).  Against the gold file -- which is this run's
    INPUT, written by the reference from its BAM run: 14 832 of the 14 862 records are identical; the other 30 are the reads
    whose close end the search finds only after reverse-complementing them (rc_flag 1): GetCloseEnd leaves them flipped,
    so their sequence line is the reverse complement of the gold one, and nothing else differs."""
    fa, reads_txt, chroms, r = _gold_run(tmp_path)
    prefix = str(tmp_path / "o")
    _call(fa, reads_txt, prefix, r)
    got = open(prefix + "_CloseEndMapped", "rb").read()
    recs = _records(reads_txt)
    assert got == _close_end_mapped(recs, r["close_cnt"], r["rc_flag"])
    gold = gzip.open(os.path.join(gu.GOLD, "simulated_test.out_CloseEndMapped.gz")).read()
    g, w = got.split(b"\n"), gold.split(b"\n")
    assert len(g) == len(w) == 3 * 14862 + 1
    differing = [k for k in range(14862) if g[3 * k:3 * k + 3] != w[3 * k:3 * k + 3]]
    assert differing == FLIPPED == [int(i) for i in np.nonzero(r["rc_flag"])[0]]
    assert 14862 - len(differing) == 14832
    for k in differing:
        assert g[3 * k] == w[3 * k] and g[3 * k + 2] == w[3 * k + 2]
        assert g[3 * k + 1] == li.reverse_complement(w[3 * k + 1]) and r["rc_flag"][k] == 1


def test_li_window_by_window(tmp_path):
    """-w 0.03: the 200-kbp chromosome in seven windows.  _LI = sort_output_li per window with Count_LI carried over,
    g_maxInsertSize / g_reportLength / the sample set as they stand, and the mask from the product's own reports of the
    windows so far (a run on the reads of those windows alone: the marks of later windows must not count)."""
    fa, reads_txt, chroms, r = _gold_run(tmp_path)
    W = 30000
    prefix = str(tmp_path / "w")
    _call(fa, reads_txt, prefix, r, window_mbp=W / 1e6)
    got = open(prefix + "_LI", "rb").read()
    recs = _records(reads_txt)
    chr_seq = chroms[0][1]
    biol = len(chr_seq) - 200000
    pos = np.array([min(x[4], biol) for x in recs])
    reads = _li_reads(recs, r)
    read_win = {id(x): min(x.pos, biol) // W for x in reads}
    want, count, n_events = b"", 0, 0
    for w in range(int(pos.max()) // W + 1):
        so_far = pos < (w + 1) * W
        in_win = [x for x in reads if read_win[id(x)] == w]
        if not in_win:
            continue
        p = str(tmp_path / f"upto{w}")
        _call(fa, reads_txt, p, r, window_mbp=W / 1e6, li_on=False, cem_on=False, keep=so_far)
        mask = li.masked_positions(_reports(p))
        upto = [x for x in reads if read_win[id(x)] <= w]
        text = li.sort_output_li(chr_seq, in_win, mask, w * W, min((w + 1) * W, biol), max(x[6] for x, k in zip(recs, so_far) if k),
                                 max(x.length for x in upto), sorted({x.tag for x in upto}), count_start=count)
        n = text.count(b"\tLI\tChrID ")
        count += n
        n_events += n
        want += text
    assert n_events >= 5
    assert got == want


def _synthetic(tmp_path):
    """Two chromosomes.  chrA: a 50-bp deletion at X0 (split reads with both ends) and a long insertion at X1; chrB: long
    insertions at X0 -- the deletion's place on chrA: without the mask reset per chromosome its marks would hide it -- and
    at X2.  A long insertion: '+' reads whose close end stops at the insertion and '-' reads whose close end starts there,
    the rest of each read being inserted sequence that is nowhere in the reference (no far end)."""
    from pindel_amd import synth
    rng = np.random.default_rng(5)
    X0, X1, X2, L = 20000, 41000, 33000, 60000
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    rc = lambda s: s.translate(comp)[::-1]
    biol = {c: synth.make_reference(L, seed=s, n_gaps=0)[100000:-100000] for c, s in (("chrA", 41), ("chrB", 42))}
    recs = []

    def plant_li(c, X, k0):
        B = biol[c]
        ins = bytes(rng.choice(list(b"ACGT"), 400))
        for j, k in enumerate(range(22, 80, 9)):
            s = rc(B[X - k:X] + ins[:100 - k])
            recs.append((f"@{c}_li{X}_{j}/1", s.decode(), "+", c, X - 250, 60, 500, "S1"))
        for j, k in enumerate(range(24, 80, 8)):
            s = ins[-(100 - k):] + B[X:X + k]
            recs.append((f"@{c}_li{X}_{j}/2", s.decode(), "-", c, X + 250, 60, 500, "S1"))

    def plant_del(c, X, D):
        B = biol[c]
        for j, k in enumerate(range(30, 71, 8)):
            recs.append((f"@{c}_d{X}_{j}/1", rc(B[X - k:X] + B[X + D:X + D + 100 - k]).decode(), "+", c, X - 250, 60, 500, "S1"))
            recs.append((f"@{c}_d{X}_{j}/2", (B[X - (100 - k):X] + B[X + D:X + D + k]).decode(), "-", c, X + D + 250, 60, 500, "S1"))

    plant_del("chrA", X0, 50)
    plant_li("chrA", X1, 0)
    plant_li("chrB", X0, 0)
    plant_li("chrB", X2, 0)
    recs.sort(key=lambda x: (x[3], x[4]))
    fa = str(tmp_path / "syn.fa")
    with open(fa, "wb") as f:
        for c in ("chrA", "chrB"):
            f.write(b">" + c.encode() + b"\n")
            for i in range(0, L, 60):
                f.write(biol[c][i:i + 60] + b"\n")
    reads_txt = str(tmp_path / "syn.txt")
    _write_text(reads_txt, recs)
    return fa, reads_txt, (X0, X1, X2)


def test_li_two_chromosomes_with_planted_insertions(tmp_path):
    fa, reads_txt, (X0, X1, X2) = _synthetic(tmp_path)
    chroms = hostio.load_fasta(fa)
    batch = hostio.read_pindel_text(reads_txt, [n for n, _ in chroms], [len(s) - 200000 for _, s in chroms])
    r = _oracle(chroms, batch)
    prefix = str(tmp_path / "syn")
    _call(fa, reads_txt, prefix, r)
    got = open(prefix + "_LI", "rb").read()
    recs = _records(reads_txt)
    want, count, upto = b"", 0, []
    for cid, (name, seq) in enumerate(chroms):
        reads = _li_reads(recs, r, name)
        upto += reads
        mask = li.masked_positions(_reports(prefix, name))
        want += li.sort_output_li(seq, reads, mask, 0, len(seq) - 200000, 500, max(x.length for x in upto),
                                  sorted({x.tag for x in upto}), count_start=count)
        count = want.count(b"\tLI\tChrID ")
    assert got == want
    heads = [l.split(b"\t") for l in got.split(b"\n") if b"\tLI\tChrID " in l]
    assert [h[0] for h in heads] == [b"%d" % i for i in range(len(heads))]        # Count_LI runs on across chromosomes
    where = {(h[2].split()[1].decode(), int(h[3])) for h in heads}
    assert where == {("chrA", X1), ("chrB", X2), ("chrB", X0)}, where
    # chrA's deletion at X0 is reported (so its marks exist) -- and the chromosome change clears them for chrB
    assert b"ChrID chrA\tBP %d" % X0 in open(prefix + "_D", "rb").read()
    assert any(abs(m - (X0 + li.SPACER)) <= 10 for m in li.masked_positions(_reports(prefix, "chrA")))


# ------------------------------------------------------------------------------------------------------------ GPU
def _exe():
    from pindel_amd import binding
    return os.path.join(os.path.dirname(binding.LIB_PATH), "pindel_pg")


def _run(args, timeout=600):
    out = subprocess.run([_exe()] + args, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr
    return out


def _read(prefix, suf):
    return open(f"{prefix}_{suf}", "rb").read()


@pytest.mark.gpu
def test_command_line_li_and_close_end_mapped(tmp_path):
    """pindel_pg -l -s: gold SV reports, _LI = the CPU expectation, _CloseEndMapped = the restatement; the same bytes with
    three contexts and four host threads and in 4 000-read flushes; -S writes the same _CloseEndMapped and nothing else;
    the switches take the reference's optional true / false words."""
    fa, reads_txt, chroms, r = _gold_run(tmp_path)
    want_li = b"\n".join(_expected_on_the_text_route())
    want_cem = _close_end_mapped(_records(reads_txt), r["close_cnt"], r["rc_flag"])
    base = ["-f", fa, "-p", reads_txt]
    p = str(tmp_path / "ls")
    out = _run(base + ["-o", p, "-l", "-s", "-T", "1"])
    assert "close end 14862, far end 10968" in out.stdout and "long insertions (_LI, host" in out.stdout
    gu.assert_reports_match_gold(p)
    assert _read(p, "LI") == want_li
    assert _read(p, "CloseEndMapped") == want_cem
    assert _read(p, "BP") == b""
    for name, extra in (("multi", ["-G", "0,0,0", "-T", "4"]), ("flush", ["--flush-reads", "4000"])):
        q = str(tmp_path / name)
        out = _run(base + ["-o", q, "-l", "-s"] + extra)
        assert "close end 14862, far end 10968" in out.stdout
        gu.assert_reports_match_gold(q)
        assert _read(q, "LI") == want_li and _read(q, "CloseEndMapped") == want_cem, name
    # -S: close end only
    q = str(tmp_path / "only")
    out = _run(base + ["-o", q, "-S", "true", "-l", "-T", "1"])
    assert "close end 14862 (-S" in out.stdout
    assert "Far_end_found" not in out.stdout and "far end" not in out.stdout and "Far ends already mapped" not in out.stdout
    assert _read(q, "CloseEndMapped") == want_cem
    for suf in ("D", "SI", "TD", "INV", "LI", "BP"):
        assert _read(q, suf) == b"", suf
    # -l false, -s 0: neither report is written, the files exist (empty), the SV reports are gold
    q = str(tmp_path / "off")
    out = _run(base + ["-o", q, "-l", "false", "-s", "0", "-T", "1"])
    assert "close end 14862, far end 10968" in out.stdout and "long insertions" not in out.stdout
    gu.assert_reports_match_gold(q)
    for suf in ALL_SUFFIXES:
        assert os.path.exists(f"{q}_{suf}"), suf
    assert _read(q, "LI") == _read(q, "BP") == _read(q, "CloseEndMapped") == b""
    # -S 0 is no -S; -s false -S 1 still writes _CloseEndMapped (reportCloseMappedReads = -s || -S)
    q = str(tmp_path / "sfalse")
    out = _run(base + ["-o", q, "-s", "false", "-S", "1", "-T", "1"])
    assert _read(q, "CloseEndMapped") == want_cem and _read(q, "D") == b""


@pytest.mark.gpu
def test_command_line_bam_route_li_and_close_end_mapped(tmp_path):
    """pindel_pg -i (the reference's demo BAM, simulated_MEI) -l -s -R false: _CloseEndMapped = the restatement over the
    ingested reads with the oracle's close ends; _LI = sort_output_li per chromosome with those close ends, the run's own
    reports as the mask and Count_LI carried from chr1 to chr2."""
    from tests.test_bam_ingest import ingest
    from tests.test_mei_bam import BAM, ISZ, TAG, _chroms
    d, chroms = _chroms(tmp_path)
    prefix = os.path.join(d, "gpu")
    out = _run(["-f", os.path.join(d, "reference.fa"), "-i", os.path.join(d, "config"), "-o", prefix, "-l", "-s", "-R", "false"])
    want_cem, want_li, count, upto = b"", b"", 0, []
    n_close = 0
    for cid, (name, s) in enumerate(chroms):
        got = ingest(BAM, name, cid, len(s), 0, 5_000_000, ISZ, tag=TAG)
        recs = [(g[0], g[1], g[2], name, g[3], g[4], g[5], TAG) for g in got]
        b = hostio.batch_from_lists([g[1].encode() for g in got], [g[2].encode() for g in got], [g[3] for g in got],
                                    [g[5] for g in got], [cid] * len(got))
        r = pyoracle.search_batch(pyoracle.make_params(), [x for _, x in chroms], b.seq, b.seq_off, b.anchor_strand, b.anchor_pos,
                                  b.insert_size, b.chr_id)
        n_close += int((r["close_cnt"] > 0).sum())
        want_cem += _close_end_mapped(recs, r["close_cnt"], r["rc_flag"])
        reads = _li_reads(recs, r)
        upto += reads
        want_li += li.sort_output_li(s, reads, li.masked_positions(_reports(prefix, name)), 0, len(s) - 200000, ISZ,
                                     max(x.length for x in upto), sorted({x.tag for x in upto}), count_start=count)
        count = want_li.count(b"\tLI\tChrID ")
    assert f"close end {n_close}," in out.stdout
    assert _read(prefix, "CloseEndMapped") == want_cem and want_cem.count(b"\n") == 3 * n_close
    assert _read(prefix, "LI") == want_li
