"""-N (--NormalSamples) on the host: hostlib.call_from_points with normal_samples and bam_config on the two-sample synthetic
of tests/germline_synth.py, points from the CPU oracle.  The expected _TD and _INV are the reports of the run without -N
with the blocks of the dropped events removed and the later event numbers lowered."""
import numpy as np
import pytest

from oracle import pyoracle
from pindel_amd import hostio, hostlib
from tests import germline_synth as gs
from tests import golden_util as gu

SUFFIXES = ("D", "SI", "TD", "INV", "LI")


def check_fixture(s):
    """A condition on the fixture, not on the code under test: by the Python restatement every planted ratio is >= 3.2 or
    <= 2.2 for every (start, end) within 100 bases of the planted one, so no breakpoint shift decides a verdict."""
    size = gs.CHR_LEN
    for tag in gs.TAGS:
        depth = gs.depth_array(s["records"][tag], 0, size)
        csum = np.concatenate([[0], np.cumsum(depth)]).astype(np.float64)          # (exact: the sums are far below 2^53)
        for ev in ("TD_a", "TD_b"):
            _, a, b = gs.EVENTS[ev]
            st, en = np.meshgrid(np.arange(a - 100, a + 101), np.arange(b - 100, b + 101), indexing="ij")
            L = en - st
            avg = lambda lo, hi: (csum[hi] - csum[lo]) / (hi - lo)
            r = 2 * (2 * avg(st, en)) / (avg(st - L, st) + avg(en, en + L))
            # the vectorised form is the restatement: spot-check it against gs.ratio at the corners and the centre
            for i, j in ((0, 0), (0, 200), (200, 0), (200, 200), (100, 100)):
                assert r[i, j] == gs.ratio(depth, size, int(st[i, j]), int(en[i, j]))
            high = ev == "TD_a" and tag == "S1"
            assert (r >= 3.2).all() if high else (r <= 2.2).all(), (tag, ev, float(r.min()), float(r.max()))
    # TD_c lies where the depth is flat: were it measured, it would be dropped
    _, a, b = gs.EVENTS["TD_c"]
    for tag in gs.TAGS:
        depth = gs.depth_array(s["records"][tag], 0, size)
        assert all(gs.ratio(depth, size, a + i, b + j) <= 2.2 for i in (-10, 0, 10) for j in (-10, 0, 10))
    # every event has reads of both samples
    for ev in gs.EVENTS:
        assert {t[7] for t in s["text"] if t[0].startswith("@" + ev + "_")} == set(gs.TAGS)


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    d = tmp_path_factory.mktemp("germline")
    s = gs.make(str(d))
    check_fixture(s)
    chroms = hostio.load_fasta(s["fasta"])
    b = hostio.read_pindel_text(s["reads_txt"], [n for n, _ in chroms], [len(q) - 200000 for _, q in chroms])
    p = pyoracle.make_params(max_range_index=gs.MAX_RANGE_INDEX)
    r = pyoracle.search_batch(p, [q for _, q in chroms], b.seq, b.seq_off, b.anchor_strand, b.anchor_pos, b.insert_size, b.chr_id)
    co, cp = gu.csr_from_strided(r["close_cnt"], r["close_pts"])
    fo, fp = gu.csr_from_strided(r["far_cnt"], r["far_pts"])
    s["points"] = (co, cp, fo, fp, r["rc_flag"])
    s["dir"] = d
    return s


def run(s, name, **kw):
    st = hostlib.default_settings(pyoracle.max_mismatch_table())
    st.analyze_li = 1
    prefix = str(s["dir"] / name)
    hostlib.call_from_points(s["fasta"], s["reads_txt"], prefix, st, *s["points"], **kw)
    return {suf: open(f"{prefix}_{suf}", "rb").read() for suf in SUFFIXES}


def check_expectations(plain, filtered):
    """the planted events of a run without -N, and what -N makes of its reports"""
    assert [gs.planted(b) for b in gs.blocks(plain["TD"])] == ["TD_a", "TD_b", "TD_c"]
    assert [gs.planted(b) for b in gs.blocks(plain["INV"])] == ["INV_s", "INV_l"]
    assert [b[0] for b in gs.blocks(plain["TD"])] == [0, 1, 2]
    assert filtered["TD"] == gs.without(plain["TD"], gs.DROPPED)
    assert filtered["INV"] == gs.without(plain["INV"], gs.DROPPED)
    assert [gs.planted(b) for b in gs.blocks(filtered["TD"])] == ["TD_a", "TD_c"]
    assert [b[0] for b in gs.blocks(filtered["TD"])] == [0, 1]                  # a dropped event takes no number
    assert [gs.planted(b) for b in gs.blocks(filtered["INV"])] == ["INV_s"]
    for suf in SUFFIXES:
        if suf not in ("TD", "INV"):
            assert filtered[suf] == plain[suf], suf


def test_normal_samples_filters_td_and_inv(sample):
    plain = run(sample, "plain")
    filtered = run(sample, "N", normal_samples=True, bam_config=sample["config"])
    check_expectations(plain, filtered)
    assert gs.without(plain["TD"], ()) == plain["TD"]                           # (the helper itself: nothing dropped, same bytes)


def test_settings_fields_do_the_same_as_the_keywords(sample):
    st = hostlib.default_settings(pyoracle.max_mismatch_table())
    st.analyze_li = 1
    st.normal_samples = 1
    st.bam_config = sample["config"].encode()
    prefix = str(sample["dir"] / "fields")
    hostlib.call_from_points(sample["fasta"], sample["reads_txt"], prefix, st, *sample["points"])
    want = run(sample, "N_again", normal_samples=True, bam_config=sample["config"])
    assert {suf: open(f"{prefix}_{suf}", "rb").read() for suf in SUFFIXES} == want


def test_text_input_is_not_filtered(sample):
    """-N without BAMs behind the reads (-p / -P input): the reference returns true early, every byte stays"""
    assert run(sample, "N_text", normal_samples=True) == run(sample, "plain2")
    assert run(sample, "cfg_only", bam_config=sample["config"]) == run(sample, "plain3")      # ... and BAMs without -N


def test_reports_do_not_depend_on_host_threads(sample, monkeypatch):
    outs = []
    for threads in ("1", "8"):
        monkeypatch.setenv("PGH_THREADS", threads)
        outs.append(run(sample, f"N_t{threads}", normal_samples=True, bam_config=sample["config"]))
    assert outs[0] == outs[1]


def test_only_the_samples_of_the_event_are_measured(sample, tmp_path):
    """UpdateSampleID: the BAMs whose tag occurs among the event's reads, in configuration order.  With S1's BAM under
    another tag, TD_a is measured in S2's flat BAM alone (n = 1, good = 0) and goes; with S2's BAM under another tag,
    it is measured in S1's alone (n = 1, good = 1) and stays."""
    plain = run(sample, "plain4")
    for other, kept in (("S1", False), ("S2", True)):
        cfg = tmp_path / f"config_{other}"
        cfg.write_text("".join(f"{sample['bams'][t]} {gs.ISZ} {'X' + t if t == other else t}\n" for t in gs.TAGS))
        got = run(sample, f"N_{other}", normal_samples=True, bam_config=str(cfg))
        assert got["TD"] == gs.without(plain["TD"], ("TD_b",) if kept else ("TD_a", "TD_b"))


def test_a_missing_bam_is_an_error(sample, tmp_path):
    cfg = tmp_path / "config_bad"
    cfg.write_text(f"{tmp_path}/nowhere.bam 300 S1\n")
    with pytest.raises(RuntimeError, match="nowhere.bam"):
        run(sample, "bad", normal_samples=True, bam_config=str(cfg))
