"""Report records on the host (pg_host_report.hpp): the header's layouts and entries, and
hostlib.report_reads_from_lists -- the plain-loop statement the device is compared with -- against a literal Python restatement on
random arrays: one record per member of the seven member lists with the pair its read's record names, the carried NT_size, the
LengthStr NT_str is cut behind (table 1) and the DI companion (table 2); one summary per read."""
import ctypes
import os
import re

import numpy as np
import pytest

from pindel_amd import binding, hostlib
from tests import test_events_cpu as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPACER = ec.SPACER


# ------------------------------------------------------------------------------------------------ exports, dtypes, constants
def test_abi_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pindel_pg.h")).read()
    binding.build()
    lib = ctypes.CDLL(binding.LIB_PATH)
    for sym in ("pg_device_batch_report_reads", "pg_device_batch_report_reads_device", "pg_device_batch_report_sizes",
                "pg_device_batch_report_download", "pg_device_batch_report_download_device", "pg_device_batch_classify"):
        assert f"{sym}(" in hdr and sym in binding.EXPORTS and hasattr(lib, sym), sym
    assert hasattr(hostlib.lib(), "pgh_report_reads_from_lists")
    for name in ("classify", "report_reads", "report_reads_tensors", "report_sizes", "report_download", "report_tensors"):
        assert callable(getattr(binding.Engine, name)), name
    with open(binding.LIB_PATH, "rb") as f:
        blob = f.read()
    for kernel in (b"pg_report_read_kernel", b"pg_report_summary_kernel", b"pg_report_cut_kernel"):
        assert kernel in blob, kernel


def test_layouts_and_constants_agree_with_the_header():
    hdr = open(os.path.join(ROOT, "include", "pindel_pg.h")).read()
    ctype = {"uint8_t": "u1", "uint16_t": "<u2", "int16_t": "<i2", "uint32_t": "<u4", "int32_t": "<i4"}
    for mod in (binding, hostlib):
        for struct, dtype in (("pg_report_read", mod.REPORT_READ_DTYPE), ("pg_report_summary", mod.REPORT_SUMMARY_DTYPE)):
            want = ec.header_struct(hdr, struct)
            assert [n for _, n in want] == list(dtype.names), struct
            for typ, name in want:
                assert dtype.fields[name][0] == (mod.VARIANT_CAND_DTYPE if typ == "pg_variant_cand" else np.dtype(ctype[typ])), (struct, name)
        assert mod.REPORT_READ_DTYPE.itemsize == 48 and mod.REPORT_SUMMARY_DTYPE.itemsize == 12
        assert [n for _, n in ec.header_struct(hdr, "pg_report_sizes")] == [f for f, _ in mod.ReportSizes._fields_]
        assert ctypes.sizeof(mod.ReportSizes) == 16
        for name in ("RR_DUP", "RR_DI", "RS_CLOSE", "RS_FAR", "RS_FAR_ANTISENSE", "RS_CLOSE_LEFT", "RS_CLOSE_RIGHT"):
            m = re.search(r"#define PG_" + name + r"\s+(0x[0-9a-f]+)u", hdr)
            assert m and int(m.group(1), 16) == getattr(mod, name), name
    assert [n for _, n in ec.header_struct(hdr, "pg_classify_params")] == [f for f, _ in binding.ClassifyParams._fields_]
    assert ctypes.sizeof(binding.ClassifyParams) == 56 and binding.ClassifyParams.max_listed.offset == 48
    dev = open(os.path.join(ROOT, "pindel_amd", "csrc", "pg_device.h")).read()
    assert "PG_KERNEL_REPORT = 10" in dev and binding.KERNEL_REPORT == 10
    assert binding.REPORT_TABLES == 7 and "#define PG_REPORT_TABLES (PG_EVENT_TABLES + PG_SV_EVENT_TABLES)" in dev


# ------------------------------------------------------------------------------------------------ random arrays
def random_input(rng, n, chrom):
    """The random lists of tests/test_events_cpu.py over reads with 1..6 close points and 0..5 far points each (the pairs of a read's
    lists index them at random), rc flags 0..2 and far ends on two chromosomes and both strands.  A read without a far end has no
    lists, as the candidate entries leave it."""
    inp = ec.random_input(rng, n, chrom)
    n_close = rng.integers(1, 7, size=n)
    n_far = rng.integers(0, 6, size=n)
    co = np.zeros(n + 1, dtype=np.uint64)
    fo = np.zeros(n + 1, dtype=np.uint64)
    co[1:] = np.cumsum(n_close)
    fo[1:] = np.cumsum(n_far)

    def points(total, abs_choices):
        p = np.zeros(total, dtype=binding.POINT_DTYPE)
        p["abs_loc"] = rng.choice(abs_choices, size=total)
        p["length"] = rng.integers(5, 30, size=total)
        p["chr_id"] = rng.choice([0, 1], size=total, p=[0.8, 0.2])
        p["direction"] = rng.choice([b"+", b"-"], size=total)
        p["strand"] = rng.choice([b"+", b"-"], size=total)
        return p
    close_pts = points(int(co[-1]), [5000, 5001, 5003])
    # half of the reads end their close list on one point: equal LeftMostPos, so that a box of inversions holds duplicates
    same = (co[1:] - 1)[rng.random(n) < 0.5].astype(np.int64)
    close_pts["abs_loc"][same], close_pts["length"][same] = 5000, 10
    inp.update(close_off=co, far_off=fo, close_pts=close_pts, far_pts=points(int(fo[-1]), [7000, 7100]),
               rc_flag=rng.choice(np.array([0, 0, 1, 2], dtype=np.uint8), size=n))
    var, var_n = inp["var"]
    sv, sv_n = inp["sv"]
    var_n[n_far == 0] = 0
    sv_n[n_far == 0] = 0
    var[n_far == 0] = np.zeros((), dtype=var.dtype)
    sv[n_far == 0] = np.zeros((), dtype=sv.dtype)
    for i in range(n):
        if n_far[i]:
            var["close_idx"][i] = rng.integers(0, n_close[i], size=var["close_idx"][i].shape)
            var["far_idx"][i] = rng.integers(0, n_far[i], size=var["far_idx"][i].shape)
            sv["close_idx"][i] = rng.integers(0, n_close[i], size=sv["close_idx"][i].shape)
            sv["far_idx"][i] = rng.integers(0, n_far[i], size=sv["far_idx"][i].shape)
    return inp


def tables_of(inp, w, chrom):
    ev = ec.host_tables(inp, w, chrom)
    svt = hostlib.sv_events_from_lists([("chrR", chrom)], inp["seq"], inp["seq_off"], inp["strand"], inp["rc_flag"], inp["close_off"],
                                       inp["close_pts"], w, ev["reads"], inp["sv"], spacer=SPACER)
    return ev, svt


def statement(inp, ev, svt):
    return hostlib.report_reads_from_lists(inp["strand"], inp["rc_flag"], inp["close_off"], inp["close_pts"], inp["far_off"], inp["far_pts"],
                                           ev, svt, inp["var"], inp["sv"])


def restate(strand, rc_flag, close_off, close_pts, far_off, far_pts, ev, svt, var, sv):
    """pindel_pg.h "report records", literally"""
    n = len(strand)
    summaries = np.zeros(n, dtype=hostlib.REPORT_SUMMARY_DTYPE)
    for i in range(n):
        c = close_pts[int(close_off[i]):int(close_off[i + 1])]
        f = far_pts[int(far_off[i]):int(far_off[i + 1])]
        s = summaries[i]
        s["rc_flag"] = rc_flag[i]
        if len(c):
            s["close_abs"], s["close_len"] = c[-1]["abs_loc"], c[-1]["length"]
            s["flags"] |= hostlib.RS_CLOSE
        if len(f):
            s["far_chr"] = f[0]["chr_id"]
            s["flags"] |= hostlib.RS_FAR | (hostlib.RS_FAR_ANTISENSE if f[0]["strand"] == b"-" else 0)
            if len(c) and c[0]["abs_loc"] != f[0]["abs_loc"]:
                s["flags"] |= hostlib.RS_CLOSE_LEFT if c[0]["abs_loc"] < f[0]["abs_loc"] else hostlib.RS_CLOSE_RIGHT
    var_c = np.asarray(var[0]).reshape(n, 2, hostlib.VARIANT_CANDS)
    sv_c, sv_n = np.asarray(sv[0]).reshape(n, hostlib.SV_SLOTS), np.asarray(sv[1]).reshape(n, 5)
    records = []
    for t in range(7):
        for word in (ev["members"][t] if t < 4 else svt["members"][t - 4]):
            word = int(word)
            i = word if t < 4 else word & 0x7fffffff
            er = ev["reads"][i]
            kind, slot = int(er["kind"]), int(er["slot"])
            r = np.zeros((), dtype=hostlib.REPORT_READ_DTYPE)
            r["read"] = i
            r["cand"] = var_c[i, kind, slot] if kind < 2 else sv_c[i, hostlib.SV_SLOT[kind] + slot]
            r["nt_size"] = er["nt_size"]
            r["table"] = t
            if t >= 4 and word & hostlib.SVEV_MEMBER_DUP:
                r["flags"] |= hostlib.RR_DUP
            if t == 1:
                if strand[i] == ord("+"):
                    length = close_pts[int(close_off[i]) + int(r["cand"]["close_idx"])]["length"]
                else:
                    length = far_pts[int(far_off[i]) + int(r["cand"]["far_idx"])]["length"]
                r["bp0"] = int(length) - 1
            if t == 2 and (int(sv_n[i, 0]) & 0x7f) >= 1:
                r["flags"] |= hostlib.RR_DI
                r["di_bp"], r["di_nt_rot"] = sv_c[i, 0]["bp"], sv_c[i, 0]["nt_rot"]
            records.append(r)
    return np.array(records, dtype=hostlib.REPORT_READ_DTYPE), summaries


def new_seen():
    return dict(si_plus_close=0, si_minus_far=0, late_close_idx=0, td_with_di=0, td_without_di=0, inv_dup=0, shortened=0, no_far=0,
                tables=np.zeros(7, np.int64))


def note_coverage(seen, records, summaries, strand, first_run_points=None):
    """first_run_points: per read the points of the first run of its close list (None: every point counts as a run of its own)"""
    for r in records:
        t, i = int(r["table"]), int(r["read"])
        seen["tables"][t] += 1
        if t == 1 and strand[i] == ord("+"):
            seen["si_plus_close"] += 1
            seen["late_close_idx"] += int(r["cand"]["close_idx"] >= (1 if first_run_points is None else first_run_points[i]))
        seen["si_minus_far"] += int(t == 1 and strand[i] != ord("+"))
        seen["td_with_di"] += int(t == 2 and (r["flags"] & hostlib.RR_DI) != 0)
        seen["td_without_di"] += int(t == 2 and (r["flags"] & hostlib.RR_DI) == 0)
        seen["inv_dup"] += int(t in (5, 6) and (r["flags"] & hostlib.RR_DUP) != 0)
    seen["shortened"] += int((summaries["rc_flag"] == 2).sum())
    seen["no_far"] += int(((summaries["flags"] & hostlib.RS_FAR) == 0).sum())


def assert_coverage(seen):
    for key, count in seen.items():
        if key != "tables":
            assert count > 0, (key, seen)
    assert (seen["tables"] > 0).all(), seen


@pytest.fixture(scope="module")
def seen():
    return new_seen()


@pytest.mark.parametrize("n", [1, 2, 3, 7, 40, 120, 200])
def test_random_arrays_against_the_literal_restatement(seen, n):
    rng = np.random.default_rng(7000 + n)
    chrom = ec.make_chrom(rng)
    for wkw in ec.WINDOWS:
        inp = random_input(rng, n, chrom)
        ev, svt = tables_of(inp, hostlib.event_window(**wkw), chrom)
        records, summaries = statement(inp, ev, svt)
        want_r, want_s = restate(inp["strand"], inp["rc_flag"], inp["close_off"], inp["close_pts"], inp["far_off"], inp["far_pts"], ev, svt,
                                 inp["var"], inp["sv"])
        what = f"n = {n}, window {wkw}"
        assert len(records) == sum(ev["n_members"]) + sum(svt["n_members"]) == len(want_r), what
        assert summaries.tobytes() == want_s.tobytes(), (what, np.nonzero(summaries != want_s)[0][:5])
        assert records.tobytes() == want_r.tobytes(), (what, np.nonzero(records != want_r)[0][:5])
        assert (summaries["reserved"] == 0).all() and (records["cand"]["reserved"] == 0).all()
        note_coverage(seen, records, summaries, inp["strand"])


def test_coverage(seen):
    """The comparison above cannot pass on nothing: a kind 1 member on each anchor strand (bp0 from the close and from the far point),
    a pair whose close point is not the list's first, a TD member with and without a DI companion, an inversion member with the
    duplicate bit, a shortened read, a read without a far end, and members in all seven tables."""
    assert_coverage(seen)


def test_members_outside_the_lists_get_zeroed_records():
    """A member word beyond the reads, or a record that names a kind or a slot no list has: a zeroed record, nothing read."""
    rng = np.random.default_rng(5)
    chrom = ec.make_chrom(rng)
    inp = random_input(rng, 60, chrom)
    ev, svt = tables_of(inp, hostlib.event_window(), chrom)
    assert sum(ev["n_members"]) >= 3
    ev = dict(ev, reads=ev["reads"].copy(), members_flat=ev["members_flat"].copy())
    a, b, c = (int(x) for x in ev["members_flat"][:3])
    ev["members_flat"][0] = 60
    ev["reads"]["kind"][b] = 7
    ev["reads"]["slot"][c] = 4
    records, _ = statement(inp, ev, svt)
    zero = np.zeros((), dtype=hostlib.REPORT_READ_DTYPE).tobytes()
    assert [records[k].tobytes() == zero for k in range(3)] == [True, True, True]
    assert any(r.tobytes() != zero for r in records[3:])


def test_empty_input():
    e = np.zeros(0, dtype=np.uint8)
    off = np.zeros(1, dtype=np.uint64)
    pts = np.zeros(0, dtype=binding.POINT_DTYPE)
    ev = dict(reads=np.zeros(0, dtype=hostlib.EVENT_READ_DTYPE), members_flat=np.zeros(0, dtype=np.uint32), n_members=[0] * 4)
    svt = dict(members_flat=np.zeros(0, dtype=np.uint32), n_members=[0] * 3)
    none = np.zeros(0, dtype=hostlib.VARIANT_CAND_DTYPE)
    records, summaries = hostlib.report_reads_from_lists(e, e, off, pts, off, pts, ev, svt, (none, e), (none, e))
    assert len(records) == 0 and len(summaries) == 0


# ------------------------------------------------------------------------------------------------ the gold set: reports from records
gold = ec.gold                     # (the fixture: the gold set searched once by the oracle, with the lists of both classifiers)


def report_run(gold, name, st, **kw):
    return ec.gold_run(gold, name, st, None, report_reads=True, **kw)


@pytest.mark.parametrize("threads", ["1", "16"])
@pytest.mark.parametrize("scenario", sorted(ec.GOLD_SCENARIOS))
def test_reports_from_records_are_byte_identical(gold, monkeypatch, scenario, threads):
    """call_from_points(report_reads=True): per window the reads lose their points, lists and pair fields, and the reports come from
    tables, records and summaries alone -- the bytes of the run without it, and in one window those of the gold reports."""
    from tests import golden_util as gu
    monkeypatch.setenv("PGH_THREADS", threads)
    fields, kw = ec.GOLD_SCENARIOS[scenario]
    st = ec.with_fields(hostlib.default_settings(gold["mm"]), **fields)
    plain = ec.gold_run(gold, f"rr_{scenario}_{threads}_plain", st, None, **kw)
    got = report_run(gold, f"rr_{scenario}_{threads}_records", st, **kw)
    assert got == plain
    wins = hostlib.last_event_windows()
    assert hostlib.last_event_fallback_windows() == 0 and hostlib.last_report_windows() == len(wins) > 0
    assert hostlib.last_report_records() > 0
    assert (len(wins) > 3) == ("windows" in scenario)
    assert b"\tD " in plain[0] and b"\tI " in plain[1]
    if scenario == "one_window":
        gu.assert_reports_match_gold(str(gold["tmp"] / f"rr_{scenario}_{threads}_records"))
        assert b"\tTD " in plain[2] and len(plain[3]) > 0


@pytest.mark.parametrize("fields", [{}, dict(min_support=3), dict(window_mbp=0.02)])
def test_reads_listed_twice_from_records(gold, monkeypatch, fields):
    monkeypatch.setenv("PGH_THREADS", "4")
    points, var, sv = ec.doubled(gold)
    st = ec.with_fields(hostlib.default_settings(gold["mm"]), **fields)
    tag = "_".join(f"{k}{v}" for k, v in fields.items()) or "default"
    kw = dict(points=points, var=var, sv=sv, reads_config=[gold["reads_txt"], gold["reads_txt"]])
    plain = ec.gold_run(gold, f"rr_twice_{tag}_plain", st, None, **kw)
    assert report_run(gold, f"rr_twice_{tag}_records", st, **kw) == plain
    assert hostlib.last_event_fallback_windows() == 0 and hostlib.last_report_windows() == len(hostlib.last_event_windows()) > 0


def cut_lists(lists, max_listed):
    """every list with more than max_listed pairs cut to that many + VARIANT_MORE (pg_device_batch_classify's max_listed)"""
    cands, counts = lists
    counts = counts.copy()
    counts[(counts & 0x7f) > max_listed] = max_listed | hostlib.VARIANT_MORE
    return cands, counts


@pytest.mark.parametrize("window_mbp", [5.0, 0.02, 0.005])
def test_cut_lists(gold, monkeypatch, window_mbp):
    """Lists cut to 0 pairs: every window that holds a listed pair falls back to the existing path, and the bytes stay.  Lists cut to
    1 or 2 pairs: on the gold set the first listed pair makes every such read Used, so no window falls back."""
    monkeypatch.setenv("PGH_THREADS", "4")
    st = ec.with_fields(hostlib.default_settings(gold["mm"]), window_mbp=window_mbp)
    tag = f"rr_cut_{window_mbp}"
    plain = ec.gold_run(gold, f"{tag}_plain", st, None)
    for k in (1, 2):
        var, sv = cut_lists(gold["var"], k), cut_lists(gold["sv"], k)
        assert (var[1] != gold["var"][1]).any() and (sv[1] != gold["sv"][1]).any()
        assert report_run(gold, f"{tag}_{k}", st, var=var, sv=sv) == plain
        assert hostlib.last_event_fallback_windows() == 0 and hostlib.last_report_windows() == len(hostlib.last_event_windows())
    var, sv = cut_lists(gold["var"], 0), cut_lists(gold["sv"], 0)
    assert report_run(gold, f"{tag}_0", st, var=var, sv=sv) == plain
    wins = hostlib.last_event_windows()
    n_fallback, n_records_windows = hostlib.last_event_fallback_windows(), hostlib.last_report_windows()
    assert n_fallback > 0 and n_fallback + n_records_windows == len(wins)
    assert hostlib.last_report_records() == 0                              # (a window that did not fall back held no listed pair)


def test_report_reads_needs_both_lists(gold):
    st = hostlib.default_settings(gold["mm"])
    with pytest.raises(ValueError):
        hostlib.call_from_points(gold["fa"], gold["reads_txt"], str(gold["tmp"] / "rr_bad"), st, *gold["points"], variant_candidates=gold["var"],
                                 report_reads=True)
