"""The event tables of DI, INV and INV_NT, host side.  hostlib.sv_events_from_lists -- the reference the device
entry is compared with -- is checked here against a literal Python restatement of the three reporters (the strict exchange loops,
the double duplicate loops, the linear grouping, harmonise() with a `whether` that is never re-armed inside a box) on random
arrays in which ties dominate, and through the reports of the gold set, which call_from_points(sv_events=...) must write byte for
byte as without it.  The entries, dtypes and constants are checked against the public header."""
import ctypes
import os
import re

import numpy as np
import pytest

from pindel_amd import binding, hostlib
from tests import sv_events_common as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ exports, dtypes, constants
def test_abi_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pindel_pg.h")).read()
    binding.build()
    lib = ctypes.CDLL(binding.LIB_PATH)
    for sym in ("pg_device_batch_sv_events", "pg_device_batch_sv_events_device", "pg_device_batch_sv_event_sizes",
                "pg_device_batch_sv_events_download", "pg_device_batch_sv_events_download_device"):
        assert f"{sym}(" in hdr and sym in binding.EXPORTS and hasattr(lib, sym), sym
    host = hostlib.lib()
    for sym in ("pgh_sv_events_from_lists", "pgh_call_from_points_sv_events"):
        assert hasattr(host, sym), sym
    for name in ("sv_events", "sv_events_tensors", "sv_event_sizes"):
        assert callable(getattr(binding.Engine, name))
    with open(binding.LIB_PATH, "rb") as f:
        blob = f.read()
    for kernel in (b"pg_sv_events_gather_kernel", b"pg_sv_events_order_kernel", b"pg_sv_events_unique_kernel", b"pg_sv_events_run_kernel",
                   b"pg_sv_events_event_kernel"):
        assert kernel in blob, kernel


def test_layouts_and_constants_agree_with_the_header():
    hdr = open(os.path.join(ROOT, "include", "pindel_pg.h")).read()
    dev = open(os.path.join(ROOT, "pindel_amd", "csrc", "pg_device.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} pg_sv_event_sizes;", hdr).group(1)
    fields = re.findall(r"uint64_t (\w+)\[PG_SV_EVENT_TABLES\];", body)
    for mod in (binding, hostlib):
        assert fields == [f for f, _ in mod.SvEventSizes._fields_] == ["members", "events", "dropped_runs"]
        assert ctypes.sizeof(mod.SvEventSizes) == 72
        assert "#define PG_SV_EVENT_TABLES 3" in hdr and mod.SV_EVENT_TABLES == 3 and tuple(mod.SV_EVENT_KINDS) == (2, 5, 6)
        for name, macro in (("EV_SHORT_INV", "PG_EV_SHORT_INV"), ("SVEV_MEMBER_DUP", "PG_SVEV_MEMBER_DUP")):
            m = re.search(r"#define " + macro + r"\s+(0x[0-9a-f]+)u", hdr)
            assert m and int(m.group(1), 16) == getattr(mod, name), name
        # the new flag is none of the four the tables of 7m use
        assert mod.EV_SHORT_INV & (mod.EV_SUPPORT | mod.EV_RANGE | mod.EV_BALANCE | mod.EV_REPORT) == 0
    assert re.search(r"enum \{ PG_SV_DI = 2, PG_SV_TD = 3, PG_SV_TD_NT = 4, PG_SV_INV = 5, PG_SV_INV_NT = 6 \}", hdr)
    assert "PG_KERNEL_EVENT_TABLES = 8, PG_KERNEL_SV_EVENTS = 9 }" in dev and binding.KERNEL_SV_EVENTS == 9
    assert f"#define PG_SVEV_LDS_BOX {binding.SVEV_LDS_BOX}u" in dev and binding.SVEV_LDS_BOX * 8 % 1280 == 0


# ------------------------------------------------------------------------------------------------ random arrays
WINDOWS = [dict(), dict(min_support=2), dict(min_support=3, balance_cutoff=10), dict(balance_cutoff=0), dict(min_support=2, balance_cutoff=1)]


@pytest.fixture(scope="module")
def seen():
    return sc.new_seen()


@pytest.mark.parametrize("n", [1, 2, 3, 7, 40, 65, 120, 200])
def test_random_arrays_against_the_literal_restatement(seen, n):
    rng = np.random.default_rng(7000 + n)
    chrom = sc.make_chrom(rng)
    for trial, wkw in enumerate(WINDOWS):
        inp = sc.random_input(rng, n, chrom, one_box=trial == 3, few_keys=trial in (1, 4), spread=trial in (1, 4))
        w = hostlib.event_window(**wkw)
        got = sc.host_tables(inp, w, chrom)
        want = sc.restate(inp, w, chrom)
        sc.assert_same_tables(got, want, f"n = {n}, window {wkw}")
        for t in range(3):
            ev = got["events"][t]
            need = 7 if t else 5
            assert (((ev["flags"] & need) == need) == ((ev["flags"] & hostlib.EV_REPORT) != 0)).all()
            assert (ev["box_head"] <= ev["first"]).all() and (ev["kind"] == sc.SV_TABLE_KINDS[t]).all()
        sc.note_coverage(seen, inp, got, chrom)


def test_coverage(seen):
    """The comparison above cannot pass on nothing: see sv_events_common.assert_coverage."""
    sc.assert_coverage(seen)


def test_tie_order_depends_on_history():
    """The two examples of DESIGN.md 7n through the host statement: three and four DI reads of one box whose keys are 5, 5, 3 and
    5, 5, 3, 4 (in BP) leave the box as 3, 5b, 5a and as 3, 4, 5a, 5b -- no stable sort of anything."""
    rng = np.random.default_rng(3)
    chrom = sc.make_chrom(rng)
    for bps, order in (([5, 5, 3], [2, 1, 0]), ([5, 5, 3, 4], [2, 3, 0, 1])):
        n = len(bps)
        inp = sc.random_input(rng, n, chrom)
        inp["recs"][:] = np.zeros((), dtype=inp["recs"].dtype)
        inp["sv"][0][:] = np.zeros((), dtype=inp["sv"][0].dtype)
        for i, bp in enumerate(bps):
            inp["recs"][i]["kind"], inp["recs"][i]["flags"] = 2, hostlib.EVR_BOXED
            c = inp["sv"][0][i, 0]
            c["bp_left"], c["bp_right"], c["indel_size"], c["bp"] = 5001, 5100, 7, bp
        # different close ends: nothing is a duplicate
        inp["close_pts"]["abs_loc"] = 6000 + 100 * np.arange(n)
        inp["close_abs"] = inp["close_pts"]["abs_loc"].astype(np.int64)
        got = sc.host_tables(inp, hostlib.event_window(), chrom)
        assert got["members"][0].tolist() == order
        sc.assert_same_tables(got, sc.restate(inp, hostlib.event_window(), chrom))


def test_refusals():
    rng = np.random.default_rng(5)
    chrom = sc.make_chrom(rng)
    inp = sc.random_input(rng, 5, chrom)
    for bad in (dict(chr_id=1), dict(chr_id=-1)):
        with pytest.raises(ValueError):
            sc.host_tables(inp, hostlib.event_window(**bad), chrom)


# ------------------------------------------------------------------------------------------------ the gold set: reports from SV tables
from tests.test_events_cpu import GOLD_SCENARIOS, doubled, gold, with_fields  # noqa: E402, F401  (gold: the module's fixture)


def gold_run(gold, name, settings, events, sv_events=None, var=None, sv=None, points=None, **kw):
    from tests import golden_util as gu
    prefix = str(gold["tmp"] / name)
    reads_txt = None if "reads_config" in kw else gold["reads_txt"]
    hostlib.call_from_points(gold["fa"], reads_txt, prefix, settings, *(points or gold["points"]), variant_candidates=var or gold["var"],
                             sv_candidates=sv or gold["sv"], events=events, sv_events=sv_events, **kw)
    return [open(f"{prefix}_{s}", "rb").read() for s in gu.SUFFIXES]


@pytest.mark.parametrize("threads", ["1", "16"])
@pytest.mark.parametrize("scenario", sorted(GOLD_SCENARIOS))
def test_reports_from_sv_tables_are_byte_identical(gold, monkeypatch, scenario, threads):
    """One window and 20-kbp windows, -c, -M 3, -B 10, INV off: the reports with sv_events are the bytes of the run without the
    events path.  The gold _INV holds 13 events of up to 664 tied reads: the tie order of the strict sort decides their read lines."""
    from tests import golden_util as gu
    monkeypatch.setenv("PGH_THREADS", threads)
    fields, kw = GOLD_SCENARIOS[scenario]
    st = with_fields(hostlib.default_settings(gold["mm"]), **fields)
    plain = gold_run(gold, f"sv_{scenario}_{threads}_plain", st, None, **kw)
    tabled = gold_run(gold, f"sv_{scenario}_{threads}_tables", st, True, True, **kw)
    assert tabled == plain
    assert hostlib.last_event_fallback_windows() == 0
    n_table, n_supplied = hostlib.last_event_table_windows()
    assert hostlib.last_sv_event_table_windows() == (n_table, 0) and n_table == len(hostlib.last_event_windows()) > 0
    inv = plain[gu.SUFFIXES.index("INV")]
    assert b"\tD " in plain[0] and (b"\tINV " in inv) == ("no_" not in scenario)
    if scenario == "one_window":
        gu.assert_reports_match_gold(str(gold["tmp"] / f"sv_{scenario}_{threads}_tables"))
        assert inv.count(b"\tINV ") >= 13 and b"\tNT " in plain[0]


@pytest.mark.parametrize("fields", [{}, dict(min_support=3), dict(window_mbp=0.02)])
def test_reads_listed_twice_sv(gold, monkeypatch, fields):
    """The read file listed twice: every read has a copy with the same LeftMostPos, so every box is half duplicates."""
    monkeypatch.setenv("PGH_THREADS", "4")
    points, var, sv = doubled(gold)
    st = with_fields(hostlib.default_settings(gold["mm"]), **fields)
    tag = "_".join(f"{k}{v}" for k, v in fields.items()) or "default"
    kw = dict(points=points, var=var, sv=sv, reads_config=[gold["reads_txt"], gold["reads_txt"]])
    plain = gold_run(gold, f"sv_twice_{tag}_plain", st, None, **kw)
    assert gold_run(gold, f"sv_twice_{tag}_tables", st, True, True, **kw) == plain
    assert hostlib.last_event_fallback_windows() == 0 and hostlib.last_sv_event_table_windows()[0] > 0


def test_truncated_lists_fall_back_sv(gold, monkeypatch):
    """Lists cut by hand: a window that holds such a read takes the existing path as a whole, the others their tables."""
    monkeypatch.setenv("PGH_THREADS", "4")
    st = with_fields(hostlib.default_settings(gold["mm"]), window_mbp=0.02)
    cands, counts = gold["var"][0].copy(), gold["var"][1].copy()
    cut = np.zeros(gold["batch"].n, dtype=bool)
    cut[np.nonzero((counts[:, 0] & 0x7f) > 0)[0][::40]] = True
    cands[cut] = np.zeros((), dtype=cands.dtype)
    counts[cut] = hostlib.VARIANT_MORE
    plain = gold_run(gold, "sv_cut_plain", st, None)
    assert gold_run(gold, "sv_cut_tables", st, True, True, var=(cands, counts)) == plain
    n_fallback, (n_table, _) = hostlib.last_event_fallback_windows(), hostlib.last_event_table_windows()
    assert n_fallback > 0 and n_table > 0 and hostlib.last_sv_event_table_windows() == (n_table, 0)


def test_supplied_sv_tables(gold, monkeypatch):
    """Tables built outside the run (here by the two host statements over all reads, as the device builds them) for the one window;
    SV tables that do not fit -- another window's, a member list cut short, a member moved to another table -- are replaced."""
    monkeypatch.setenv("PGH_THREADS", "4")
    st = hostlib.default_settings(gold["mm"])
    plain = gold_run(gold, "sv_supplied_plain", st, None)
    assert gold_run(gold, "sv_supplied_probe", st, True, True) == plain
    wins = hostlib.last_event_windows()
    assert len(wins) == 1
    chr_index, ws, we, rs, re_, n_reads = [int(x) for x in wins[0]]
    b = gold["batch"]
    co, cp, fo, fp, rc = gold["points"]
    w = hostlib.event_window(chr_id=chr_index, win_end=we, region_start=rs, region_end=re_, min_support=st.min_support,
                             balance_cutoff=st.balance_cutoff)
    names = b.names if len(b.names) == b.n else None
    t = hostlib.events_from_lists(gold["chroms"], b.seq, b.seq_off, b.anchor_strand, b.chr_id, rc, b.insert_size, co, cp, fo, fp, w,
                                  gold["var"], gold["sv"], hostlib.name_ids(names) if names else None)
    s = hostlib.sv_events_from_lists(gold["chroms"], b.seq, b.seq_off, b.anchor_strand, rc, co, cp, w, t["reads"], gold["sv"])
    assert s["n_events"][1] >= 13 and s["n_events"][0] > 0 and max(int(e["n_reads"]) for e in s["events"][1]) >= 600
    key = (chr_index, ws, we)
    assert gold_run(gold, "sv_supplied_tables", st, {key: t}, {key: s}) == plain
    assert hostlib.last_event_table_windows() == (1, 1) and hostlib.last_sv_event_table_windows() == (1, 1)
    # SV tables without supplied event tables, and for another window: the host builds its own
    assert gold_run(gold, "sv_supplied_alone", st, True, {key: s}) == plain
    assert hostlib.last_sv_event_table_windows() == (1, 0)
    assert gold_run(gold, "sv_supplied_other", st, {key: t}, {(chr_index, ws + 1, we): s}) == plain
    assert hostlib.last_sv_event_table_windows() == (1, 0)
    # tables that do not fit the window's records
    short = dict(s, members_flat=s["members_flat"][:-1], n_members=[s["n_members"][0], s["n_members"][1], s["n_members"][2] - 1],
                 events_flat=s["events_flat"][:sum(s["n_events"][:2])], n_events=[s["n_events"][0], s["n_events"][1], 0])
    assert gold_run(gold, "sv_supplied_short", st, {key: t}, {key: short}) == plain
    assert hostlib.last_sv_event_table_windows() == (1, 0)
    moved = dict(s, n_members=[s["n_members"][0] + 1, s["n_members"][1] - 1, s["n_members"][2]])
    assert gold_run(gold, "sv_supplied_moved", st, {key: t}, {key: moved}) == plain
    assert hostlib.last_sv_event_table_windows() == (1, 0)


def test_sv_events_need_the_events_path(gold):
    st = hostlib.default_settings(gold["mm"])
    with pytest.raises(ValueError):
        hostlib.call_from_points(gold["fa"], gold["reads_txt"], str(gold["tmp"] / "bad"), st, *gold["points"], variant_candidates=gold["var"],
                                 sv_candidates=gold["sv"], sv_events=True)
