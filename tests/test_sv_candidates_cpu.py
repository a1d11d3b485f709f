"""Candidate lists for the DI, tandem-duplication and inversion classifiers, host side: hostlib.sv_candidates lists,
per read, the pair of each single-pair kind and the first VARIANT_CANDS pairs of TD and INV in the order the classifiers' loops
first visit them, and call_from_points(sv_candidates=...) classifies from those lists.  On the reference's gold set (points from
the CPU oracle) the four reports must be the bytes of a run without the lists, and the number of reads that fell back to a
classifier's own search must be what the lists, the windows and the insert sizes imply.  The gold set alone does not show every
kind on both strands; the constructed reads of tests/sv_cases.py are checked here, on the CPU, to do so.  The 64-positions-per-step
walks of the device classifier are checked against the host's one-base loops by tests/sv_align_unit.cpp."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle
from pindel_amd import hostio, hostlib
from tests import golden_util as gu
from tests import sv_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MORE = hostlib.VARIANT_MORE


@pytest.fixture(scope="module")
def gold(tmp_path_factory):
    """The gold set searched once by the oracle, and its candidate lists of all seven kinds."""
    tmp = tmp_path_factory.mktemp("sv_gold")
    fa, reads_txt = gu.unpack(tmp)
    chroms = hostio.load_fasta(fa)
    batch = hostio.read_pindel_text(reads_txt, [n for n, _ in chroms], [len(s) - 200000 for _, s in chroms])
    r = pyoracle.search_batch(pyoracle.make_params(), [s for _, s in chroms], batch.seq, batch.seq_off, batch.anchor_strand,
                              batch.anchor_pos, batch.insert_size, batch.chr_id)
    co, cp = gu.csr_from_strided(r["close_cnt"], r["close_pts"])
    fo, fp = gu.csr_from_strided(r["far_cnt"], r["far_pts"])
    mm = pyoracle.max_mismatch_table()
    reads = (chroms, batch.seq, batch.seq_off, batch.anchor_strand, batch.chr_id, r["rc_flag"], co, cp, fo, fp, mm)
    return dict(tmp=tmp, fa=fa, reads_txt=reads_txt, batch=batch, points=(co, cp, fo, fp, r["rc_flag"]), mm=mm, reads=reads,
                sv=hostlib.sv_candidates(*reads), var=hostlib.variant_candidates(*reads))


def derived_fallbacks(cands, counts, insert_size, strand, visits):
    """The reads that must have gone through a classifier's own search: per consultation of a list of kind 2..6 (read, kind, the
    window's end, the region, the boxes) every listed pair fails the window-dependent tests without making the read Used -- the
    classifiers' tail restated on 32-bit integers; inversions of a '-' anchor skip the bin-boundary test -- and the list says
    there are more pairs."""
    u32 = 0xffffffff
    n = 0
    for i, kind, win_end, reg_s, reg_e, n_boxes, box_size in visits.tolist():
        if kind < 2:
            continue
        count = int(counts[i, kind - 2])
        slot = hostlib.SV_SLOT[kind]
        used = False
        for c in cands[i, slot:slot + min(count & 0x7f, hostlib.SV_LIST_LEN[kind])]:
            bp_left, bp_right = int(c["bp_left"]), int(c["bp_right"])
            if c["flags"] & hostlib.VARIANT_REF_END:
                used = True
            elif not (kind == 5 and strand[i] == ord("-")) and bp_right > ((win_end - 2 * int(insert_size[i])) & u32):
                used = True
            elif reg_s <= ((bp_left + 1) & u32) <= reg_e:
                signed = bp_left - (1 << 32) if bp_left >> 31 else bp_left
                used = (int(signed / box_size) & u32) < n_boxes
            if used:
                break
        if not used and count & MORE:
            n += 1
    return n


def run(gold, name, settings, sv=None, var=None, **kw):
    prefix = str(gold["tmp"] / name)
    hostlib.call_from_points(gold["fa"], gold["reads_txt"], prefix, settings, *gold["points"], variant_candidates=var, sv_candidates=sv, **kw)
    return [open(f"{prefix}_{s}", "rb").read() for s in gu.SUFFIXES]


def small_windows(settings):
    s = hostlib.HostSettings.from_buffer_copy(settings)
    s.window_mbp = 0.02
    return s


def other_settings(settings):
    s = hostlib.HostSettings.from_buffer_copy(settings)
    s.min_inversion_size = 0         # -v 0
    s.min_num_matched_bases = 45     # -d
    s.seq_error_rate = 0.03          # -e
    return s


SCENARIOS = {
    "whole": (lambda s: s, {}),
    "half": (lambda s: s, {"region": "1:1-100000"}),
    "windows": (small_windows, {}),
    "settings": (other_settings, {}),
}


def check_shape(cands, counts, n):
    assert cands.shape == (n, hostlib.SV_SLOTS) and counts.shape == (n, 5)
    listed = counts & 0x7f
    raw = cands.view(np.uint8).reshape(n, hostlib.SV_SLOTS, 32)
    for kind, slot in hostlib.SV_SLOT.items():
        cap = hostlib.SV_LIST_LEN[kind]
        assert listed[:, kind - 2].max() <= cap
        assert ((counts[:, kind - 2] & MORE) == 0)[listed[:, kind - 2] < cap].all()           # "more" only behind a full list
        for j in range(cap):
            assert not raw[:, slot + j][listed[:, kind - 2] <= j].any()                       # unused records are zero
    assert not (counts[:, [0, 2, 4]] & MORE).any()                                            # the single-pair kinds never say "more"
    assert not cands["nt_rot"][:, 1:5].any() and not cands["nt_rot"][:, 6:10].any()           # NT_size is 0 for TD and INV
    for slot in (0, 5, 10):
        got = cands[:, slot][listed[:, {0: 0, 5: 2, 10: 4}[slot]] > 0]
        assert (got["nt_rot"] > 0).all()                                                      # ... and positive where bases were left over


def test_lists_have_the_expected_shape(gold):
    cands, counts = gold["sv"]
    check_shape(cands, counts, gold["batch"].n)
    listed = counts & 0x7f
    assert (listed > 0).sum(axis=0).min() > 0, (listed > 0).sum(axis=0).tolist()          # the gold set shows every kind


def coverage(listed, strand):
    """per kind: (reads with a candidate on '+', on '-', with more than one record)"""
    plus = strand == ord("+")
    return {k: (int((listed[plus, k - 2] > 0).sum()), int((listed[~plus, k - 2] > 0).sum()), int((listed[:, k - 2] > 1).sum()))
            for k in hostlib.SV_KINDS}


def test_constructed_reads_cover_every_kind_on_both_strands(gold):
    """The coverage the comparisons rest on: gold set + tests/sv_cases.py, with the oracle's points."""
    total = {k: np.array(v) for k, v in coverage(gold["sv"][1] & 0x7f, gold["batch"].anchor_strand).items()}
    for name, chroms, batch, prm in sv_cases.all_cases():
        cands, counts = sv_cases.host_lists(chroms, batch, prm)
        check_shape(cands, counts, batch.n)
        sv_cases.check_case(name, batch, cands, counts)
        for k, v in coverage(counts & 0x7f, batch.anchor_strand).items():
            total[k] += np.array(v)
    for k, (p, m, multi) in total.items():
        assert p > 0 and m > 0, (hostlib.SV_KINDS[k], p, m)
    assert total[3][2] > 0 and total[5][2] > 0


@pytest.mark.parametrize("threads", ["1", "16"])
@pytest.mark.parametrize("scenario", sorted(SCENARIOS))
def test_reports_from_lists_are_byte_identical(gold, monkeypatch, scenario, threads):
    monkeypatch.setenv("PGH_THREADS", threads)
    make, kw = SCENARIOS[scenario]
    st = make(hostlib.default_settings(gold["mm"]))
    sv = gold["sv"] if scenario != "settings" else hostlib.sv_candidates(*gold["reads"], settings=st)
    plain = run(gold, f"{scenario}_{threads}_plain", st, **kw)
    listed = run(gold, f"{scenario}_{threads}_sv", st, sv, **kw)
    assert listed == plain
    visits = hostlib.last_variant_visits()
    assert set(visits[:, 1].tolist()) == {2, 3, 4, 5, 6} and len(visits) > 1000
    assert hostlib.last_variant_fallbacks() == derived_fallbacks(*sv, gold["batch"].insert_size, gold["batch"].anchor_strand, visits)
    both = run(gold, f"{scenario}_{threads}_both", st, sv, gold["var"], **kw)
    assert both == plain
    assert set(hostlib.last_variant_visits()[:, 1].tolist()) == set(range(7))
    assert b"\tTD " in plain[2] and b"\tINV " in plain[3] and b"\tD " in plain[0]
    if scenario == "whole":
        gu.assert_reports_match_gold(str(gold["tmp"] / f"{scenario}_{threads}_sv"))
        gu.assert_reports_match_gold(str(gold["tmp"] / f"{scenario}_{threads}_both"))
    if scenario == "settings":
        assert sv[0].tobytes() != gold["sv"][0].tobytes()                 # the settings reached the lists


def test_truncated_lists(gold, monkeypatch):
    """Lists cut by hand: TD and INV to one record with "more" set, the single-pair kinds zeroed with "more" set (the consumer then
    runs the classifier's own code).  Same reports; the fallback count is the derived one."""
    monkeypatch.setenv("PGH_THREADS", "4")
    st = hostlib.default_settings(gold["mm"])
    b = gold["batch"]
    plain = run(gold, "cut_plain", st)
    cands, counts = gold["sv"][0].copy(), gold["sv"][1].copy()
    for kind in (3, 5):
        slot = hostlib.SV_SLOT[kind]
        has = (counts[:, kind - 2] & 0x7f) > 0
        counts[has, kind - 2] = 1 | MORE
        cands[:, slot + 1:slot + hostlib.VARIANT_CANDS] = np.zeros((), dtype=cands.dtype)
    for kind in (2, 4, 6):
        counts[:, kind - 2] = MORE
        cands[:, hostlib.SV_SLOT[kind]] = np.zeros((), dtype=cands.dtype)
    assert run(gold, "cut_sv", st, (cands, counts)) == plain
    visits = hostlib.last_variant_visits()
    want = derived_fallbacks(cands, counts, b.insert_size, b.anchor_strand, visits)
    single = int(np.isin(visits[:, 1], (2, 4, 6)).sum())
    assert single > 1000 and want >= single and hostlib.last_variant_fallbacks() == want
    # under a region that ends before most events the one listed pair fails the region test and the search takes over
    half = {"region": "1:1-45000"}
    cut_plain = run(gold, "cut_half_plain", st, **half)
    assert run(gold, "cut_half_sv", st, (cands, counts), **half) == cut_plain
    visits = hostlib.last_variant_visits()
    multi = visits[np.isin(visits[:, 1], (3, 5))]
    assert derived_fallbacks(cands, counts, b.insert_size, b.anchor_strand, multi) > 0
    assert hostlib.last_variant_fallbacks() == derived_fallbacks(cands, counts, b.insert_size, b.anchor_strand, visits)
    # everything cut: every consultation falls back
    counts[:] = MORE
    cands[:] = np.zeros((), dtype=cands.dtype)
    assert run(gold, "cut_all", st, (cands, counts)) == plain
    assert hostlib.last_variant_fallbacks() == len(hostlib.last_variant_visits())
    run(gold, "cut_none", st)
    assert hostlib.last_variant_fallbacks() == 0 and len(hostlib.last_variant_visits()) == 0


def test_bad_inputs_are_refused(gold):
    st = hostlib.default_settings(gold["mm"])
    with pytest.raises(ValueError):
        run(gold, "bad", st, (gold["sv"][0][:-1], gold["sv"][1][:-1]))
    for v in (-1, (1 << 30) + 1):
        with pytest.raises(ValueError):
            hostlib.sv_candidates(*gold["reads"], settings=(0.01, 30, v))
    # a consumer whose -v is refused searches the pairs itself: the inversion lists are not consulted
    bad = hostlib.HostSettings.from_buffer_copy(st)
    bad.min_inversion_size = -1
    plain = run(gold, "badv_plain", bad)
    assert run(gold, "badv_sv", bad, gold["sv"]) == plain
    assert set(hostlib.last_variant_visits()[:, 1].tolist()) == {2, 3, 4}


def test_alignment_walks_unit(tmp_path):
    """tests/sv_align_unit.cpp: the 64-positions-per-step walks against left_most_td / left_most_inv; plain, and as a stand-alone
    program under the address and undefined-behaviour sanitizers."""
    inc = [f"-I{os.path.join(ROOT, d)}" for d in ("include", "pindel_amd/csrc", "pindel_amd/csrc/host")]
    for tag, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = str(tmp_path / f"sv_align_unit_{tag}")
        subprocess.run(["g++", "-std=c++17", "-Wall", *flags, *inc, os.path.join(ROOT, "tests", "sv_align_unit.cpp"), "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        assert "sv_align_unit ok" in out.stdout
