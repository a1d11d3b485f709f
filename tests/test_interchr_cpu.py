"""-I (--report_interchromosomal_events) on the host: the read-pair clustering, the _INT reporter and the _INT_final merge
against the independent restatement tests/interchr_restated.py (the reference's BAM path cannot be built here, and its two
gold _INT_final files are empty), on the seeded sample of tests/interchr_synth.py and on random inputs."""
import os
import random

import numpy as np

from oracle import pyoracle
from pindel_amd import hostio, hostlib
from tests import golden_util as gu
from tests import interchr_common as ic
from tests import interchr_restated as ir
from tests import interchr_synth as syn

SPACER = ic.SPACER


def _window_of(pos):
    return pos // syn.WINDOW


def _assert_sample_is_dense_enough(s):
    for c in s["counts"]:
        assert c["spanning"] >= 12 and c["split_plus"] >= 6 and c["split_minus"] >= 6, c
    names = [r["qname"] for r in s["records"] if r["flag"] & ic.F["UNMAP"]]
    assert len(names) - len(set(names)) == 1                  # unique but for the deliberate duplicate
    assert abs(_window_of(syn.X) - _window_of(syn.Z)) >= 2
    assert _window_of(syn.Y) == _window_of(syn.U) and _window_of(syn.V) == _window_of(syn.W)


def test_rp_interchr_events_equal_the_restatement(tmp_path):
    L = ic.lib()
    s = syn.make(str(tmp_path))
    _assert_sample_is_dense_enough(s)
    names = list(syn.NAMES)
    # the synthetic BAM, window by window: discovery + clustering through the C entry == the restatement
    found = {}
    for cid, name in enumerate(names):
        for ws, we in syn.windows():
            out = np.zeros(6 * 256, dtype=np.int64)
            rp_path = tmp_path / "rp.txt"
            n = L.pgh_rp_events_chr(s["bam"].encode(), name.encode(), ws, we, syn.ISZ, syn.TAG.encode(), 0, SPACER, 1, str(rp_path).encode(),
                                    out.ctypes.data, 256)
            assert n >= 0, L.pgh_last_error()
            pairs = ic.discover_interchr(s["records"], cid, ws, we, syn.ISZ, syn.TAG, names)
            want_ev, want_rp = ir.rp_interchr(pairs, SPACER)
            assert ic.events_from(out, n, names) == want_ev, (name, ws)
            assert rp_path.read_text() == want_rp, (name, ws)
            for e in want_ev:
                found.setdefault((name, ws), []).append(e)
            # without -I the same entry keeps the interchromosomal pairs out, and the old entry still does
            assert L.pgh_rp_events_chr(s["bam"].encode(), name.encode(), ws, we, syn.ISZ, syn.TAG.encode(), 0, SPACER, 0, None, out.ctypes.data, 256) == 0
    # every junction side: one event whose two windows (BreakDancer window span 200) hold both breakpoints
    for (c1, p1, c2, p2) in (("chrA", syn.X, "chrB", syn.Y), ("chrB", syn.Y, "chrA", syn.X), ("chrB", syn.U, "chrC", syn.V),
                             ("chrC", syn.V, "chrB", syn.U), ("chrC", syn.W, "chrA", syn.Z), ("chrA", syn.Z, "chrC", syn.W)):
        evs = [e for e in found.get((c1, _window_of(p1) * syn.WINDOW), []) if e[0] == c1 and e[3] == c2]
        assert len(evs) >= 1, (c1, p1, found)
        assert any(e[1] - 200 <= p1 + SPACER <= e[2] + 200 and e[4] - 200 <= p2 + SPACER <= e[5] + 200 for e in evs), (c1, p1, evs)
    # 200 random pair sets: mixed chromosome pairs, swapped sides, both strands, 1-60 pairs, no tie in (PosA, PosB)
    rng = random.Random(1234)
    tags = ["S1", "S2", "T"]
    n_events = n_swapped_sets = 0
    for case in range(200):
        n = rng.randint(1, 60)
        centres = [(rng.sample(names, 2), rng.randint(5000, 90000), rng.randint(5000, 90000), rng.choice("+-"), rng.choice("+-"))
                   for _ in range(rng.randint(1, 3))]
        pairs, used = [], set()
        while len(pairs) < n:
            (ca, cb), pa, pb, da, db = rng.choice(centres)
            a, b = pa + rng.randint(-150, 150), pb + rng.randint(-150, 150)
            if rng.random() < 0.1:
                da, db = rng.choice("+-"), rng.choice("+-")
            p = dict(ChrNameA=ca, ChrNameB=cb, DA=da, DB=db, PosA=a, PosB=b, InsertSize=rng.choice([300, 400, 500]),
                     ReadLength=rng.choice([100, 100, 150]), Tag=rng.choice(tags))
            if rng.random() < 0.3:                              # the same junction seen from the other side
                p.update(ChrNameA=cb, ChrNameB=ca, DA=db, DB=da, PosA=b, PosB=a)
                n_swapped_sets += 1
            if (p["PosA"], p["PosB"]) in used:
                continue
            used.add((p["PosA"], p["PosB"]))
            pairs.append(p)
        got_ev, got_rp = ic.cluster_pairs(pairs, names, tags, tmp_path / "rp_random.txt")
        want_ev, want_rp = ir.rp_interchr(pairs, SPACER)
        assert got_ev == want_ev, case
        assert got_rp == want_rp, case
        n_events += len(want_ev)
    assert n_events >= 50 and n_swapped_sets >= 200              # the random sets do report events, swapped sides included
    print("random pair sets: events", n_events)


def _text_route_expected(s, tmp_path):
    """reads.txt window by window as run_pipeline bins it: oracle close end, the windows of ctx.bd for the bin, oracle far end.
    -> (CSR arrays for call_from_points over the whole file, the restatement's read lists per window [(chr, ws, reads)])"""
    L = ic.lib()
    names = list(syn.NAMES)
    chroms = hostio.load_fasta(s["fasta"])
    per_window, res_all = [], []
    text = s["text"]
    for cid, name in enumerate(names):
        mine = [t for t in text if t[3] == name]
        for w in sorted({_window_of(t[4]) for t in mine}):
            ws, we = w * syn.WINDOW, min((w + 1) * syn.WINDOW, syn.CHR_LEN)
            got = [(t[0], t[1], t[2], t[4], t[5], t[6], cid) for t in mine if _window_of(t[4]) == w]
            b = ic.batch_of(got, cid)

            def windows_of(last):
                off = np.zeros(b.n + 1, dtype=np.uint64)
                win = np.zeros(3 * 4096, dtype=np.int32)
                n_ev = ic.C.c_uint64()
                rc = L.pgh_bd_query(s["bd"].encode(), SPACER, len(names), ic.c_names(names), cid, ws + SPACER, we + SPACER, b.n,
                                    last.ctypes.data, off.ctypes.data, win.ctypes.data, 4096, ic.C.byref(n_ev))
                assert rc == 0 and n_ev.value == 3, L.pgh_last_error()
                return off, win[:3 * int(off[-1])]
            res = ic.oracle_with_windows(chroms, b, windows_of)
            res_all.append(res)
            per_window.append((name, ws, ic.restated_reads(names, chroms, got, res, name)))
    cat = {k: np.concatenate([r[k] for r in res_all]) for k in ("close_cnt", "far_cnt", "rc_flag")}
    co, cp = gu.csr_from_strided(cat["close_cnt"], np.concatenate([r["close_pts"] for r in res_all]))
    fo, fp = gu.csr_from_strided(cat["far_cnt"], np.concatenate([r["far_pts"] for r in res_all]))
    return (co, cp, fo, fp, cat["rc_flag"]), per_window


def _parse_int(text):
    """_INT lines -> (anchor D, chr, pos, far chr, far pos, sequence, support)"""
    out = []
    for line in text.splitlines():
        call, _, sup = line.partition("\tsupport: ")
        f = call.split(" ")
        out.append((f[1], f[2], int(f[3]), f[5], int(f[6]), f[8], int(sup)))
    return out


def check_sample_reports(per_window, int_text, final_text):
    """the conditions the synthetic sample has to meet, on the restatement's output (so an empty result cannot pass)"""
    by = {}
    for name, ws, reads in per_window:
        t, n = ir.int_lines(reads, SPACER)
        by[(name, ws)] = (_parse_int(t), n, reads)
    # "at the planted position": AbsLoc is the last matched base of either end (one or two below the 1-based position after
    # the junction), and bases that happen to agree on both sides of a junction of random sequence move the split
    near = lambda a, b: abs(a - b) <= 3
    final = [l.split("\t") for l in final_text.splitlines()]
    # chrA, window of X: the reciprocal junction with chrB; window of Z: the junction with chrC and its non-template bases
    calls_x = by[("chrA", _window_of(syn.X) * syn.WINDOW)][0]
    assert any(c[1] == "chrA" and near(c[2], syn.X) and c[3] == "chrB" and near(c[4], syn.Y) and c[5] == '""' and c[6] >= 4 for c in calls_x), calls_x
    assert {c[0] for c in calls_x} == {"+", "-"}                  # both anchor strands of the reciprocal junction
    calls_z = by[("chrA", _window_of(syn.Z) * syn.WINDOW)][0]
    assert any(c[1] == "chrA" and near(c[2], syn.Z) and c[3] == "chrC" and near(c[4], syn.W) and c[5] != '""' and c[6] >= 4 for c in calls_z), calls_z
    for far_chr, pos in (("chrB", syn.X), ("chrC", syn.Z)):
        assert any(l[1] == "chrA" and l[5] == far_chr and near(int(l[3]), pos) for l in final if l[0] == "chr"), (far_chr, final_text)
    # chrB: (i) is printed; the reads of (ii) are collected and never printed (chrA < chrB < chrC: the first pair takes every name)
    calls_b, n_b, reads_b = by[("chrB", _window_of(syn.Y) * syn.WINDOW)]
    assert any(c[1] == "chrB" and near(c[2], syn.Y) and c[3] == "chrA" and near(c[4], syn.X) for c in calls_b), calls_b
    assert all(c[3] == "chrA" for c in calls_b)
    assert sum(1 for r in ir.collect(reads_b) if r["FarFragName"] == "chrC") >= 6
    # chrC: reads towards chrB and towards chrA are collected, nothing is printed (its own name sorts last)
    calls_c, n_c, reads_c = by[("chrC", _window_of(syn.V) * syn.WINDOW)]
    assert calls_c == [] and n_c >= 12
    assert {r["FarFragName"] for r in ir.collect(reads_c)} == {"chrA", "chrB"}
    assert int_text and final_text


def test_int_report_from_points(tmp_path):
    s = syn.make(str(tmp_path))
    _assert_sample_is_dense_enough(s)
    csr, per_window = _text_route_expected(s, tmp_path)
    want_int, want_final, collected = ic.int_reports([reads for _, _, reads in per_window])
    check_sample_reports(per_window, want_int, want_final)
    st = hostlib.default_settings(pyoracle.max_mismatch_table())
    st.window_mbp = float(syn.WINDOW_MBP)
    st.report_interchromosomal = 1
    prefix = str(tmp_path / "on")
    hostlib.call_from_points(s["fasta"], s["reads_txt"], prefix, st, *csr)
    assert open(prefix + "_INT").read() == want_int
    assert open(prefix + "_INT_final").read() == want_final
    # without the flag: the same reports, and neither file
    st.report_interchromosomal = 0
    off = str(tmp_path / "off")
    hostlib.call_from_points(s["fasta"], s["reads_txt"], off, st, *csr)
    for suf in gu.SUFFIXES:
        assert open(f"{prefix}_{suf}", "rb").read() == open(f"{off}_{suf}", "rb").read(), suf
    assert not os.path.exists(off + "_INT") and not os.path.exists(off + "_INT_final")
    # a second run into the same prefix starts _INT afresh (the reference would append)
    st.report_interchromosomal = 1
    hostlib.call_from_points(s["fasta"], s["reads_txt"], prefix, st, *csr)
    assert open(prefix + "_INT").read() == want_int


def _final_of(tmp_path, text):
    L = ic.lib()
    src, dst = tmp_path / "calls_INT", tmp_path / "calls_INT_final"
    src.write_text(text)
    assert L.pgh_int_final(str(src).encode(), str(dst).encode()) == 0
    return dst.read_text()


def test_merge_interchr_cases(tmp_path):
    call = lambda d, c1, p1, c2, p2, fd, seq, n: f"Anchor {d} {c1} {p1} {'-' if d == '+' else '+'} {c2} {p2} {fd} {seq}\tsupport: {n}\n"
    # empty
    assert _final_of(tmp_path, "") == ""
    # one call: printed twice, without and with the labels; below the single-line cutoff (4): nothing
    one = call("+", "chrA", 30000, "chrB", 50001, "+", '""', 5)
    assert _final_of(tmp_path, one) == ('chrA\t30000\tchrB\t50001\t""\t5\t+\tchrA\t30000\t-\tchrB\t50001\t+\t""\t5\n'
                                        'chr\tchrA\tpos\t30000\tchr\tchrB\tpos\t50001\tseq\t""\tsupport\t5\tINFOR\t+\tchrA\t30000\t-\tchrB\t50001\t+\t""\t5\n')
    assert _final_of(tmp_path, call("+", "chrA", 30000, "chrB", 50001, "+", '""', 3)) == ""
    # two calls within 10 bp: one merged line (the second call, alone and below the cutoff, adds nothing)
    two = call("+", "chrA", 30000, "chrB", 50001, "+", '""', 2) + call("-", "chrA", 30005, "chrB", 50008, "-", '"ACG"', 3)
    assert _final_of(tmp_path, two) == ('chr\tchrA\tpos\t30002\tchr\tchrB\tpos\t50004\tseq\t""\tsupport\t5\tINFOR\t+\tchrA\t30000\t-\tchrB\t50001\t+\t""\t2'
                                        '\t-\tchrA\t30005\t+\tchrB\t50008\t-\t"ACG"\t3\n')
    cases = [
        "", one, two,
        # a chain of three: a-b merged, b-c merged, c alone (support 4) printed
        call("+", "chrA", 100, "chrB", 200, "+", '""', 2) + call("+", "chrA", 108, "chrB", 208, "+", '""', 2) + call("-", "chrA", 116, "chrB", 216, "-", '""', 4),
        # supports below both cutoffs; a pair adding up to 2 is merged, a single 3 is not printed
        call("+", "chrA", 100, "chrB", 200, "+", '""', 1) + call("+", "chrA", 101, "chrB", 201, "+", '""', 1) + call("+", "chrC", 5000, "chrB", 100, "-", '""', 3),
        # 10 bp apart is not "within 10"; other chromosome pair; positions the other way round (the unsigned difference)
        call("+", "chrA", 100, "chrB", 200, "+", '""', 4) + call("+", "chrA", 110, "chrB", 200, "+", '""', 4) + call("+", "chrA", 95, "chrC", 200, "+", '""', 4)
        + call("-", "chrA", 91, "chrB", 195, "-", '"TT"', 6),
        # a malformed line ends the reading there
        call("+", "chrA", 100, "chrB", 200, "+", '""', 4) + "Anchor + chrA x - chrB 5 + \"\"\tsupport: 9\n" + call("+", "chrA", 101, "chrB", 201, "+", '""', 4),
    ]
    for k, text in enumerate(cases):
        assert _final_of(tmp_path, text) == ir.int_final(text), k
    chain = ir.int_final(cases[3]).splitlines()
    assert len(chain) == 3 and chain[0].count("INFOR") == 1 and "\tsupport\t4\tINFOR\t+\tchrA\t100" in chain[0] and chain[2].startswith("chr\tchrA\tpos\t116")


def test_single_chromosome_gold_run_has_empty_int_files(tmp_path):
    fa, reads_txt = gu.unpack(tmp_path)
    chroms = hostio.load_fasta(fa)
    batch = hostio.read_pindel_text(reads_txt, [n for n, _ in chroms], [len(s) - 200000 for _, s in chroms])
    p = pyoracle.make_params()
    r = pyoracle.search_batch(p, [s for _, s in chroms], batch.seq, batch.seq_off, batch.anchor_strand, batch.anchor_pos, batch.insert_size,
                              batch.chr_id)
    co, cp = gu.csr_from_strided(r["close_cnt"], r["close_pts"])
    fo, fp = gu.csr_from_strided(r["far_cnt"], r["far_pts"])
    st = hostlib.default_settings(pyoracle.max_mismatch_table())
    st.report_interchromosomal = 1
    prefix = str(tmp_path / "gold_i")
    hostlib.call_from_points(fa, reads_txt, prefix, st, co, cp, fo, fp, r["rc_flag"])
    gu.assert_reports_match_gold(prefix)
    # as the reference's own simulated_test.out_INT_final (0 bytes)
    assert os.path.getsize(prefix + "_INT_final") == 0 and os.path.getsize(prefix + "_INT") == 0
