"""Candidate lists for the deletion and short-insertion classifiers, host side: hostlib.variant_candidates
enumerates each read's first VARIANT_CANDS (close point, far point) pairs in the order SearchVariant's loops first visit them,
and call_from_points(variant_candidates=...) classifies from those lists.  On the reference's gold set (points from the CPU
oracle) the four reports must be the bytes of a run without the lists, and the number of reads that fell back to the pair search
must be exactly what the lists, the windows and the insert sizes imply.  The 64-positions-per-step alignment walks the device
classifier uses are checked against the host library's loops by a stand-alone program (tests/variant_align_unit.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle
from pindel_amd import hostio, hostlib
from tests import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold(tmp_path_factory):
    """The gold set searched once by the oracle, and its candidate lists."""
    tmp = tmp_path_factory.mktemp("variant_gold")
    fa, reads_txt = gu.unpack(tmp)
    chroms = hostio.load_fasta(fa)
    batch = hostio.read_pindel_text(reads_txt, [n for n, _ in chroms], [len(s) - 200000 for _, s in chroms])
    r = pyoracle.search_batch(pyoracle.make_params(), [s for _, s in chroms], batch.seq, batch.seq_off, batch.anchor_strand,
                              batch.anchor_pos, batch.insert_size, batch.chr_id)
    co, cp = gu.csr_from_strided(r["close_cnt"], r["close_pts"])
    fo, fp = gu.csr_from_strided(r["far_cnt"], r["far_pts"])
    mm = pyoracle.max_mismatch_table()
    cands, counts = hostlib.variant_candidates(chroms, batch.seq, batch.seq_off, batch.anchor_strand, batch.chr_id, r["rc_flag"],
                                               co, cp, fo, fp, mm)
    return dict(tmp=tmp, fa=fa, reads_txt=reads_txt, batch=batch, points=(co, cp, fo, fp, r["rc_flag"]), mm=mm, cands=cands, counts=counts)


def derived_fallbacks(cands, counts, insert_size, visits):
    """The reads that must have gone through the pair search: per consultation of a list (read, kind, the window's end, the
    region, the boxes) every listed pair fails the window-dependent tests without making the read Used -- the tests of
    SearchVariant's loop body, restated on 32-bit integers -- and the list says there are more pairs."""
    u32 = 0xffffffff
    n = 0
    for i, kind, win_end, reg_s, reg_e, n_boxes, box_size in visits.tolist():
        count = int(counts[i, kind])
        used = False
        for c in cands[i, kind, :count & 0x7f]:
            bp_left, bp_right = int(c["bp_left"]), int(c["bp_right"])
            if c["flags"] & hostlib.VARIANT_REF_END:
                used = True                                                   # BPLeft / BPRight beyond the chromosome string
            elif bp_right > ((win_end - 2 * int(insert_size[i])) & u32):
                used = True                                                   # readTransgressesBinBoundaries
            elif reg_s <= ((bp_left + 1) & u32) <= reg_e:
                signed = bp_left - (1 << 32) if bp_left >> 31 else bp_left
                box = int(signed / box_size) & u32                            # (C++ integer division truncates towards zero)
                used = box < n_boxes
            if used:
                break
        if not used and count & hostlib.VARIANT_MORE:
            n += 1
    return n


def run(gold, name, settings, lists=None, **kw):
    prefix = str(gold["tmp"] / name)
    hostlib.call_from_points(gold["fa"], gold["reads_txt"], prefix, settings, *gold["points"], variant_candidates=lists, **kw)
    return [open(f"{prefix}_{s}", "rb").read() for s in gu.SUFFIXES]


def small_windows(settings):
    s = hostlib.HostSettings.from_buffer_copy(settings)
    s.window_mbp = 0.02                    # 20-kbp windows: reads within two insert sizes of a window's end transgress it
    return s


SCENARIOS = {
    "whole": (lambda s: s, {}),
    "half": (lambda s: s, {"region": "1:1-100000"}),              # -c: the first half of the 200-kbp chromosome
    "windows": (small_windows, {}),
}


def test_lists_have_the_expected_shape(gold):
    cands, counts = gold["cands"], gold["counts"]
    n = gold["batch"].n
    assert cands.shape == (n, 2, hostlib.VARIANT_CANDS) and counts.shape == (n, 2)
    listed = counts & 0x7f
    assert listed.max() == hostlib.VARIANT_CANDS          # (CleanUniquePoints leaves these reads few close points: none has a fifth pair)
    assert ((counts & hostlib.VARIANT_MORE) == 0)[listed < hostlib.VARIANT_CANDS].all()       # "more" only behind a full list
    assert (listed[:, 0] > 0).sum() > 500 and (listed[:, 1] > 0).sum() > 500
    # unused records are zeroed, listed ones are distinct pairs
    raw = cands.view(np.uint8).reshape(n, 2, hostlib.VARIANT_CANDS, 32)
    for j in range(hostlib.VARIANT_CANDS):
        assert not raw[:, :, j][listed <= j].any()
    for j in range(1, hostlib.VARIANT_CANDS):
        both = listed > j
        same = (cands["close_idx"][:, :, j] == cands["close_idx"][:, :, j - 1]) & (cands["far_idx"][:, :, j] == cands["far_idx"][:, :, j - 1])
        assert not (same & both).any()
    # deletions carry no rotation; insertions in repeats do
    assert not cands["nt_rot"][:, 0].any() and cands["nt_rot"][:, 1].any()


@pytest.mark.parametrize("threads", ["1", "16"])
@pytest.mark.parametrize("scenario", sorted(SCENARIOS))
def test_reports_from_lists_are_byte_identical(gold, monkeypatch, scenario, threads):
    monkeypatch.setenv("PGH_THREADS", threads)
    make, kw = SCENARIOS[scenario]
    st = make(hostlib.default_settings(gold["mm"]))
    plain = run(gold, f"{scenario}_{threads}_plain", st, **kw)
    listed = run(gold, f"{scenario}_{threads}_lists", st, (gold["cands"], gold["counts"]), **kw)
    assert listed == plain
    assert b"\tD " in plain[0] and b"\tI " in plain[1]
    if scenario == "whole":
        gu.assert_reports_match_gold(str(gold["tmp"] / f"{scenario}_{threads}_lists"))
    visits = hostlib.last_variant_visits()
    assert len(visits) > 1000
    want = derived_fallbacks(gold["cands"], gold["counts"], gold["batch"].insert_size, visits)
    assert hostlib.last_variant_fallbacks() == want
    if scenario == "windows":
        # some read transgressed its window: it was consulted for deletions, is in no report's box, and never reached the insertions
        kinds = {}
        for v in visits.tolist():
            kinds.setdefault(v[0], set()).add(v[1])
        t = 0
        for i, ks in kinds.items():
            c = gold["cands"][i, 0, 0]
            if ks == {0} and gold["counts"][i, 0]:
                we = [v[2] for v in visits.tolist() if v[0] == i][0]
                t += int(c["bp_right"]) > we - 2 * int(gold["batch"].insert_size[i])
        assert t > 0


def test_forced_fallback(gold, monkeypatch):
    """Lists truncated by hand to "nothing listed, more exist" for every other read: those reads go through the pair search whenever
    they reach the stage, and the reports do not change."""
    monkeypatch.setenv("PGH_THREADS", "4")
    st = hostlib.default_settings(gold["mm"])
    cands, counts = gold["cands"].copy(), gold["counts"].copy()
    cut = np.arange(gold["batch"].n) % 2 == 0
    cands[cut] = np.zeros((), dtype=cands.dtype)
    counts[cut] = hostlib.VARIANT_MORE
    plain = run(gold, "forced_plain", st)
    assert run(gold, "forced_lists", st, (cands, counts)) == plain
    visits = hostlib.last_variant_visits()
    reached = int(cut[visits[:, 0]].sum())
    assert reached > 5000
    rest = visits[~cut[visits[:, 0]]]
    assert hostlib.last_variant_fallbacks() == reached + derived_fallbacks(cands, counts, gold["batch"].insert_size, rest)
    assert hostlib.last_variant_fallbacks() == derived_fallbacks(cands, counts, gold["batch"].insert_size, visits)
    # lists cut to their first pair, "more" set, under a region that ends 5 kbp before the events most of the longer lists belong
    # to (they lie in the 10-kbp margin the windows add): the listed pair is tried, fails the region test, the pair search takes over
    cands, counts = gold["cands"].copy(), gold["counts"].copy()
    long = (counts & 0x7f) > 1
    assert long.sum() > 20
    counts[long] = 1 | hostlib.VARIANT_MORE
    cands[:, :, 1:][long] = np.zeros((), dtype=cands.dtype)
    half = {"region": "1:1-45000"}
    cut_plain = run(gold, "cut_plain", st, **half)
    assert run(gold, "cut_lists", st, (cands, counts), **half) == cut_plain
    want = derived_fallbacks(cands, counts, gold["batch"].insert_size, hostlib.last_variant_visits())
    assert want > 0 and hostlib.last_variant_fallbacks() == want
    # every list truncated: every consultation falls back
    counts[:] = hostlib.VARIANT_MORE
    cands[:] = np.zeros((), dtype=cands.dtype)
    assert run(gold, "forced_all", st, (cands, counts)) == plain
    assert hostlib.last_variant_fallbacks() == len(hostlib.last_variant_visits())
    # a run without lists consults none and reports no fallback
    run(gold, "forced_none", st)
    assert hostlib.last_variant_fallbacks() == 0 and len(hostlib.last_variant_visits()) == 0


def test_lists_of_the_wrong_size_are_refused(gold):
    st = hostlib.default_settings(gold["mm"])
    with pytest.raises(ValueError):
        run(gold, "bad", st, (gold["cands"][:-1], gold["counts"][:-1]))


def test_alignment_walks_unit(tmp_path):
    """tests/variant_align_unit.cpp: the 64-positions-per-step walks against real_start_deletion / real_start_insertion."""
    exe = str(tmp_path / "variant_align_unit")
    inc = [f"-I{os.path.join(ROOT, d)}" for d in ("include", "pindel_amd/csrc", "pindel_amd/csrc/host")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", *inc, os.path.join(ROOT, "tests", "variant_align_unit.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "variant_align_unit ok" in out.stdout
