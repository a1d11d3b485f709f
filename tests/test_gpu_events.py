"""The third part of the device classifier (pg_events.hip): event tables of a searched device batch for one window,
against hostlib.events_from_lists -- the plain-loop statement on the host -- fed the same lists and the points the same search
downloaded.  Every byte of the per-read records, the member lists and the event records must be equal, and the sizes."""
import ctypes as C

import numpy as np
import pytest

from pindel_amd import binding, hostlib, synth
from tests import golden_util as gu
from tests import shortening_cases as sc
from tests import sv_cases
from tests import variant_cases as vc
from tests.test_gpu_variant_candidates import point_csr, searched

pytestmark = pytest.mark.gpu

B = binding.EVENT_BLOCK            # the scan / sort block of the implementation
WHOLE = dict(chr_id=0, win_end=0xffffffff, region_start=0, region_end=0xffffffff, min_support=1, balance_cutoff=100,
             analyze_td=1, analyze_inv=1)


def window(**kw):
    return binding.EventWindow(**{**WHOLE, **kw})


def assert_tables_equal(got, want, what):
    assert got["unresolved"] == want["unresolved"], what
    assert got["n_members"] == want["n_members"] and got["n_events"] == want["n_events"], (what, got["n_members"], want["n_members"],
                                                                                           got["n_events"], want["n_events"])
    for name in want["reads"].dtype.names:
        d = np.nonzero(got["reads"][name] != want["reads"][name])[0]
        assert len(d) == 0, f"{what}: per-read field {name} differs for reads {d[:6].tolist()}: device {got['reads'][name][d[:6]].tolist()}, host {want['reads'][name][d[:6]].tolist()}"
    assert got["reads"].tobytes() == want["reads"].tobytes(), what
    d = np.nonzero(got["members_flat"] != want["members_flat"])[0]
    assert len(d) == 0, f"{what}: members differ from place {d[:4].tolist()}: device {got['members_flat'][d[:6]].tolist()}, host {want['members_flat'][d[:6]].tolist()}"
    for name in want["events_flat"].dtype.names:
        d = np.nonzero(got["events_flat"][name] != want["events_flat"][name])[0]
        assert len(d) == 0, f"{what}: event field {name} differs for events {d[:6].tolist()}: device {got['events_flat'][name][d[:6]].tolist()}, host {want['events_flat'][name][d[:6]].tolist()}"
    assert got["events_flat"].tobytes() == want["events_flat"].tobytes(), what


class Case:
    """One searched batch with its lists, kept on the device until close()."""

    def __init__(self, eng, chroms, batch, prm=None, bd=None, bd_off=None):
        self.eng, self.chroms, self.batch = eng, chroms, batch
        self.db, self.res = searched(eng, chroms, batch, bd, bd_off)
        self.var = eng.variant_candidates(self.db)
        self.sv = eng.sv_candidates(self.db, prm)
        self.co, self.cp = point_csr(self.res.close_off, self.res.close_runs)
        self.fo, self.fp = point_csr(self.res.far_off, self.res.far_runs)

    def host(self, w, var="own", sv="own", name_id=None):
        b = self.batch
        return hostlib.events_from_lists(self.chroms, b.seq, b.seq_off, b.anchor_strand, b.chr_id, self.res.rc_flag, b.insert_size,
                                         self.co, self.cp, self.fo, self.fp, w, self.var if var == "own" else var,
                                         self.sv if sv == "own" else sv, name_id)

    def check(self, w, what, var="own", sv="own", name_id=None):
        got = self.eng.events(self.db, w, self.var if var == "own" else var, self.sv if sv == "own" else sv, name_id)
        want = self.host(w, var, sv, name_id)
        assert_tables_equal(got, want, what)
        return want

    def close(self):
        self.eng.free_device_batch(self.db)


@pytest.fixture(scope="module")
def eng(engine_factory):
    return engine_factory()


@pytest.fixture(scope="module")
def seen():
    """per table: events, events with two members or more, events with both strands, events that are not reported; reads used
    without a box; duplicates"""
    return dict(events=np.zeros(4, np.int64), multi=np.zeros(4, np.int64), both=np.zeros(4, np.int64), unreported=np.zeros(4, np.int64),
                used=0, dups=0, unresolved=0)


def note(seen, t):
    for k in range(4):
        ev = t["events"][k]
        seen["events"][k] += len(ev)
        seen["multi"][k] += int((ev["n_reads"] >= 2).sum())
        seen["both"][k] += int(((ev["n_plus"] > 0) & (ev["n_plus"] < ev["n_reads"])).sum())
        seen["unreported"][k] += int(((ev["flags"] & hostlib.EV_REPORT) == 0).sum())
    seen["used"] += int(((t["reads"]["flags"] & hostlib.EVR_USED) != 0).sum())
    seen["dups"] += int(((t["reads"]["flags"] & hostlib.EVR_DUPLICATE) != 0).sum())
    seen["unresolved"] += t["unresolved"]


def windows_for(batch, chroms):
    """The windows of the CPU list: the whole chromosome, a win_end inside the reads' span, a region that excludes half of them, -M
    1 and 3, TD and INV switched off."""
    mid = int(np.median(batch.anchor_pos))
    return [("whole", window()), ("win_end inside", window(win_end=mid)), ("half region", window(region_start=0, region_end=mid)),
            ("-M 3", window(min_support=3)), ("-B 10", window(balance_cutoff=10)), ("no TD", window(analyze_td=0)),
            ("no INV", window(analyze_inv=0)), ("neither", window(analyze_td=0, analyze_inv=0))]


def tripled(batch):
    return sc.concat([batch, batch, batch])


@pytest.mark.parametrize("read_len", [100, 150])
def test_synthetic_reads(eng, seen, read_len):
    chroms = [("chrS", synth.make_reference(60_000, seed=41))]
    batch = synth.make_reads(chroms[0][1], 260, read_len=read_len, seed=42 + read_len, mix=(0.2, 0.1, 0.3, 0.3, 0.1))
    c = Case(eng, chroms, batch)
    try:
        for name, w in windows_for(batch, chroms):
            note(seen, c.check(w, f"synthetic {read_len} bp, {name}"))
        # either pair of lists may be missing: those kinds' lists count as empty
        note(seen, c.check(window(), "no sv lists", sv=None))
        note(seen, c.check(window(), "no variant lists", var=None))
        t = c.check(window(), "no lists at all", var=None, sv=None)
        assert not t["reads"].view(np.uint8).any() and t["n_members"] == [0] * 4
    finally:
        c.close()


def test_every_read_three_times(eng, seen):
    """Ties in every key; with equal name ids for the copies markDuplicates fires, with distinct ids (and with none) it does not."""
    chroms = [("chrS", synth.make_reference(60_000, seed=41))]
    one = synth.make_reads(chroms[0][1], 260, read_len=100, seed=142, mix=(0.2, 0.1, 0.3, 0.3, 0.1))
    batch = tripled(one)
    c = Case(eng, chroms, batch)
    try:
        same = np.tile(np.arange(one.n, dtype=np.uint32), 3)
        for name, w in windows_for(batch, chroms)[:4]:
            a = c.check(w, f"tripled, equal ids, {name}", name_id=same)
            b = c.check(w, f"tripled, distinct ids, {name}", name_id=np.arange(batch.n, dtype=np.uint32))
            n = c.check(w, f"tripled, no ids, {name}")
            note(seen, a)
            note(seen, b)
            assert ((a["reads"]["flags"] & hostlib.EVR_DUPLICATE) != 0).sum() > 0
            assert not (b["reads"]["flags"] & hostlib.EVR_DUPLICATE).any() and b["reads"].tobytes() == n["reads"].tobytes()
            # of the three copies the one with the highest read index comes first and is the one that stays unique
            dup = (a["reads"]["flags"] & hostlib.EVR_DUPLICATE) != 0
            assert not dup[2 * one.n:].any() and (dup[:one.n] == dup[one.n:2 * one.n]).all()
    finally:
        c.close()


def test_constructed_cases(eng, seen):
    """The cases of tests/variant_cases.py and tests/sv_cases.py (the exact-kernel case among them: the post-state read length feeds
    the balance test)."""
    cases = [(n, ch, b, None) for n, ch, b in vc.all_cases()] + list(sv_cases.all_cases())
    for name, chroms, one, prm in cases:
        # every read three times: each event has three members or more, and -M 4 leaves the small ones unreported
        c = Case(eng, chroms, tripled(one), prm)
        try:
            for wname, w in (("whole", window()), ("-M 4 -B 10", window(min_support=4, balance_cutoff=10))):
                note(seen, c.check(w, f"{name}, {wname}"))
            note(seen, c.check(window(), f"{name}, equal ids", name_id=np.tile(np.arange(one.n, dtype=np.uint32), 3)))
        finally:
            c.close()


def boxed_in_tables(reads):
    return ((reads["flags"] & hostlib.EVR_BOXED) != 0) & np.isin(reads["kind"], hostlib.EVENT_KINDS)


def test_seams(eng):
    """Boxed counts of B - 1, B, B + 1 and 2 B + 1 (the scan / sort block), 0 and 1; batches of 1, 63, 64 and 65 reads."""
    chroms = [("chrS", synth.make_reference(60_000, seed=41))]
    batch = synth.make_reads(chroms[0][1], 1100, read_len=100, seed=7, mix=(0.25, 0.25, 0.3, 0.1, 0.1))
    c = Case(eng, chroms, batch)
    try:
        full = c.check(window(), "seams: the whole batch")
        cum = np.cumsum(boxed_in_tables(full["reads"]))
    finally:
        c.close()
    assert cum[-1] >= 2 * B + 1, int(cum[-1])
    prefixes = [int(np.searchsorted(cum, k)) + 1 for k in (1, B - 1, B, B + 1, 2 * B + 1)] + [1, 63, 64, 65]
    for n in prefixes:
        sub = batch.slice(0, n)
        c = Case(eng, chroms, sub)
        try:
            t = c.check(window(), f"seams: {n} reads")
            if n in prefixes[:5]:
                assert int(boxed_in_tables(t["reads"]).sum()) == (1, B - 1, B, B + 1, 2 * B + 1)[prefixes.index(n)]
            ids = (np.arange(n, dtype=np.uint32) // 2)
            c.check(window(min_support=2), f"seams: {n} reads, paired ids", name_id=ids)
        finally:
            c.close()
    # nothing boxed: a region no read reaches
    c = Case(eng, chroms, batch.slice(0, 300))
    try:
        t = c.check(window(region_start=0xfffffff0, region_end=0xfffffffe), "seams: nothing boxed")
        assert not boxed_in_tables(t["reads"]).any() and t["n_events"] == [0] * 4
    finally:
        c.close()


def test_unresolved_reads(eng, seen):
    """Lists cut by hand with PG_VARIANT_MORE set: those reads leave the cascade at that kind, are counted and are in no event."""
    chroms = [("chrS", synth.make_reference(60_000, seed=41))]
    batch = synth.make_reads(chroms[0][1], 260, read_len=100, seed=142, mix=(0.2, 0.1, 0.3, 0.3, 0.1))
    c = Case(eng, chroms, batch)
    try:
        cands, counts = c.var[0].copy(), c.var[1].copy()
        cut = (np.arange(batch.n) % 3 == 0) & ((counts[:, 0] & 0x7f) > 0)
        cands[cut, 0] = np.zeros((), dtype=cands.dtype)
        counts[cut, 0] = hostlib.VARIANT_MORE
        svc, svn = c.sv[0].copy(), c.sv[1].copy()
        cut_td = (np.arange(batch.n) % 3 == 1) & ((svn[:, 1] & 0x7f) > 0)
        svn[cut_td, 1] = hostlib.VARIANT_MORE
        svc[cut_td, 1:5] = np.zeros((), dtype=svc.dtype)
        assert cut.sum() > 3 and cut_td.sum() > 3
        t = c.check(window(), "cut lists", var=(cands, counts), sv=(svc, svn))
        note(seen, t)
        un = (t["reads"]["flags"] & hostlib.EVR_UNRESOLVED) != 0
        assert t["unresolved"] == un.sum() >= cut.sum() + 1
        assert un[cut].all() and (t["reads"]["unresolved_kind"][cut] == 0).all()
        assert (t["reads"]["unresolved_kind"][un & cut_td] == 3).any()
        assert not np.isin(np.nonzero(un)[0], t["members_flat"]).any()
    finally:
        c.close()


def test_tensors_refusals_and_launch_log(eng):
    chroms = [("chrS", synth.make_reference(60_000, seed=41))]
    batch = synth.make_reads(chroms[0][1], 200, seed=77, mix=(0.2, 0.1, 0.3, 0.3, 0.1))
    eng.load_reference(chroms)
    db = eng.upload(batch)
    # not searched: refused, by both entries, with nothing launched
    eng.clear_launch_log()
    with pytest.raises(binding.PgError) as e:
        eng.events(db, window())
    assert e.value.code == -1 and "searched" in str(e.value)
    with pytest.raises(binding.PgError):
        eng.events_tensors(db, window())
    assert eng.launch_log() == []
    eng.search_device(db)
    var, sv = eng.variant_candidates(db), eng.sv_candidates(db)
    vt, st = eng.variant_candidates_tensors(db), eng.sv_candidates_tensors(db)
    eng.clear_launch_log()
    for bad in (window(chr_id=1), window(chr_id=-1), window(region_start=10, region_end=9)):
        with pytest.raises(binding.PgError) as e:
            eng.events(db, bad, var, sv)
        assert e.value.code == -1
        with pytest.raises(binding.PgError):
            eng.events_tensors(db, bad, vt, st)
    with pytest.raises(binding.PgError):
        eng.event_sizes(db)                                                # no tables yet
    assert eng.launch_log() == []
    # the build logs its own kernel ids, after 4 (variant) and 5 (sv), and reports its HIP-event time
    got = eng.events(db, window(), var, sv)
    ids = [r.kernel for r in eng.launch_log()]
    assert ids[0] == binding.KERNEL_EVENT_CASCADE and ids[-1] == binding.KERNEL_EVENT_TABLES and set(ids[1:-1]) == {binding.KERNEL_EVENT_SORT}
    assert eng.last_stats()[0] > 0.0
    assert sum(got["n_events"]) > 0
    # events_tensors equals events
    import torch
    nid = np.arange(batch.n, dtype=np.uint32) // 2
    for name_id in (None, nid):
        got = eng.events(db, window(), var, sv, name_id)
        t = eng.events_tensors(db, window(), vt, st, None if name_id is None else torch.from_numpy(name_id.view(np.int32)).to(vt["cands"].device))
        assert t["reads"].is_cuda and t["members"].is_cuda and t["events"].is_cuda
        assert_tables_equal(binding.events_from_tensors(t), got, "tensors")
    # a host pointer to a _device entry is a status, and nothing is launched
    eng.clear_launch_log()
    L = eng._L
    w = window()
    host_c = np.ascontiguousarray(var[0])
    assert L.pg_device_batch_events_device(eng._h, db, C.addressof(w), host_c.ctypes.data, vt["counts"].data_ptr(), None, None, None) == -1
    assert b"not device memory" in L.pg_last_error(eng._h)
    assert L.pg_device_batch_events_device(eng._h, db, C.addressof(w), vt["cands"].data_ptr(), vt["counts"].data_ptr(), None, None,
                                           nid.ctypes.data) == -1
    assert b"not device memory" in L.pg_last_error(eng._h)
    assert eng.launch_log() == []
    eng.events(db, window(), var, sv)
    host_reads = np.zeros(batch.n, dtype=binding.EVENT_READ_DTYPE)
    assert L.pg_device_batch_events_download_device(eng._h, db, host_reads.ctypes.data, None, None) == -1
    assert b"not device memory" in L.pg_last_error(eng._h)
    # the two candidate entries still log only their own kernel ids
    eng.clear_launch_log()
    eng.variant_candidates(db)
    eng.sv_candidates(db)
    assert [r.kernel for r in eng.launch_log()] == [4, 5]
    eng.free_device_batch(db)
    # an empty batch: valid, nothing launched
    empty = eng.upload(batch.slice(0, 0))
    eng.search_device(empty)
    eng.clear_launch_log()
    t0 = eng.events(empty, window())
    assert len(t0["reads"]) == 0 and t0["n_members"] == [0] * 4 and t0["n_events"] == [0] * 4 and t0["unresolved"] == 0
    tt = eng.events_tensors(empty, window())
    assert tt["reads"].shape[0] == 0
    assert eng.launch_log() == []
    eng.free_device_batch(empty)


def test_reads_of_another_chromosome_are_untouched(eng):
    name, chroms, batch, bd, bd_off = vc.translocation_case()
    c = Case(eng, chroms, batch, None, bd, bd_off)
    try:
        for chr_id in (0, 1):
            t = c.check(window(chr_id=chr_id), f"{name}, window on chromosome {chr_id}")
            assert not t["reads"][batch.chr_id != chr_id].view(np.uint8).any()
    finally:
        c.close()


def test_coverage(seen):
    """The comparisons above cannot pass on nothing."""
    for k in range(4):
        assert seen["events"][k] > 0 and seen["multi"][k] > 0 and seen["unreported"][k] > 0, (k, {n: v.tolist() if hasattr(v, "tolist") else v for n, v in seen.items()})
    assert seen["both"][0] > 0 and seen["both"][1] > 0
    assert seen["used"] > 0 and seen["dups"] > 0 and seen["unresolved"] > 0


def test_gold_set_end_to_end(eng, tmp_path):
    """The gold set as one window: searched and classified on the GPU, its event tables built on the GPU, reported on the host from
    those tables -- the gold reports."""
    from pindel_amd import hostio
    fa, reads_txt = gu.unpack(tmp_path)
    chroms = hostio.load_fasta(fa)
    batch = hostio.read_pindel_text(reads_txt, [n for n, _ in chroms], [len(s) - 200000 for _, s in chroms])
    c = Case(eng, chroms, batch)
    try:
        st = hostlib.default_settings(eng.max_mismatch_table())
        points = (c.co, c.cp, c.fo, c.fp, c.res.rc_flag)
        probe = str(tmp_path / "probe")
        hostlib.call_from_points(fa, reads_txt, probe, st, *points, variant_candidates=c.var, sv_candidates=c.sv, events=True)
        gu.assert_reports_match_gold(probe)
        assert hostlib.last_event_fallback_windows() == 0
        wins = hostlib.last_event_windows()
        assert len(wins) == 1
        chr_index, ws, we, rs, re_, n_reads = [int(x) for x in wins[0]]
        w = window(chr_id=chr_index, win_end=we, region_start=rs, region_end=re_, min_support=st.min_support, balance_cutoff=st.balance_cutoff)
        assert len(batch.names) == batch.n
        t = c.check(w, "gold set", name_id=hostlib.name_ids(batch.names))
        assert t["unresolved"] == 0 and all(n > 0 for n in t["n_events"][:3])
        got = eng.events(c.db, w, c.var, c.sv, hostlib.name_ids(batch.names))
        prefix = str(tmp_path / "gpu_tables")
        hostlib.call_from_points(fa, reads_txt, prefix, st, *points, variant_candidates=c.var, sv_candidates=c.sv, events={(chr_index, ws, we): got})
        assert hostlib.last_event_table_windows() == (1, 1)
        gu.assert_reports_match_gold(prefix)
    finally:
        c.close()
