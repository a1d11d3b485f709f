"""The fourth part of the device classifier (pg_sv_events.hip): the event tables of DI, INV and INV_NT of a searched
device batch, against hostlib.sv_events_from_lists -- the plain-loop statement on the host with its literal exchange sort -- fed the
per-read records the device's events build left, the same lists and the close points the same search downloaded.  Every byte of
the member lists and the event records must be equal, and the sizes."""
import ctypes as C

import numpy as np
import pytest

from pindel_amd import binding, hostlib, synth
from tests import golden_util as gu
from tests import shortening_cases
from tests import sv_cases
from tests import sv_events_common as sc
from tests.test_gpu_variant_candidates import point_csr, searched

pytestmark = pytest.mark.gpu

LIMIT = binding.SVEV_LDS_BOX       # reads of a box the order kernel keeps in LDS
WHOLE = dict(chr_id=0, win_end=0xffffffff, region_start=0, region_end=0xffffffff, min_support=1, balance_cutoff=100,
             analyze_td=1, analyze_inv=1)
# hand-made lists: the padded synthetic chromosome has boxes of 8 bases -- 5006 and 5007 share one, 5008 opens the next
LEFTS = (5006, 5007, 5008, 9000)
HAND = dict(region_end=20000)      # ... and the pairs in front of a chosen inversion slot lie outside this region


def window(**kw):
    return binding.EventWindow(**{**WHOLE, **kw})


def assert_tables_equal(got, want, what):
    assert got["n_members"] == want["n_members"] and got["n_events"] == want["n_events"] and got["dropped_runs"] == want["dropped_runs"], (
        what, got["n_members"], want["n_members"], got["n_events"], want["n_events"], got["dropped_runs"], want["dropped_runs"])
    d = np.nonzero(got["members_flat"] != want["members_flat"])[0]
    assert len(d) == 0, f"{what}: members differ from place {d[:4].tolist()}: device {got['members_flat'][d[:6]].tolist()}, host {want['members_flat'][d[:6]].tolist()}"
    for name in want["events_flat"].dtype.names:
        d = np.nonzero(got["events_flat"][name] != want["events_flat"][name])[0]
        assert len(d) == 0, f"{what}: event field {name} differs for events {d[:6].tolist()}: device {got['events_flat'][name][d[:6]].tolist()}, host {want['events_flat'][name][d[:6]].tolist()}"
    assert got["events_flat"].tobytes() == want["events_flat"].tobytes(), what


class Case:
    """One searched batch, kept on the device until close()."""

    def __init__(self, eng, chroms, batch, prm=None):
        self.eng, self.chroms, self.batch, self.prm = eng, chroms, batch, prm
        self.db, self.res = searched(eng, chroms, batch)
        self.co, self.cp = point_csr(self.res.close_off, self.res.close_runs)
        self._lists = None

    def own_lists(self):
        if self._lists is None:
            self._lists = (self.eng.variant_candidates(self.db), self.eng.sv_candidates(self.db, self.prm))
        return self._lists

    def check(self, w, what, var, sv):
        """events build, sv build, and the host statement over the records of the former"""
        recs = self.eng.events(self.db, w, var, sv)["reads"]
        got = self.eng.sv_events(self.db, sv)
        b = self.batch
        want = hostlib.sv_events_from_lists(self.chroms, b.seq, b.seq_off, b.anchor_strand, self.res.rc_flag, self.co, self.cp, w, recs, sv)
        assert_tables_equal(got, want, what)
        return want, dict(n=b.n, recs=recs, sv=sv)

    def close(self):
        self.eng.free_device_batch(self.db)


@pytest.fixture(scope="module")
def eng(engine_factory):
    return engine_factory()


def synthetic(n, read_len=100, seed=142):
    chroms = [("chrS", synth.make_reference(60_000, seed=41))]
    return chroms, synth.make_reads(chroms[0][1], n, read_len=read_len, seed=seed, mix=(0.1, 0.05, 0.15, 0.6, 0.1))


def tripled(batch):
    return shortening_cases.concat([batch, batch, batch])


def n_boxed(recs, kinds=sc.SV_TABLE_KINDS):
    return int((((recs["flags"] & hostlib.EVR_BOXED) != 0) & np.isin(recs["kind"], kinds)).sum())


# ------------------------------------------------------------------------------------------------ searched reads, their own lists
@pytest.mark.parametrize("read_len", [100, 150])
def test_synthetic_reads_tripled(eng, read_len):
    """Every read three times: ties in every key, and the copies are duplicates of each other (equal LeftMostPos)."""
    chroms, one = synthetic(260, read_len, 42 + read_len)
    c = Case(eng, chroms, tripled(one))
    try:
        var, sv = c.own_lists()
        mid = int(np.median(one.anchor_pos))
        total = np.zeros(3, np.int64)
        dups = 0
        for name, w in (("whole", window()), ("half region", window(region_end=mid)), ("-M 3", window(min_support=3)),
                        ("-B 10", window(balance_cutoff=10)), ("no TD", window(analyze_td=0)), ("no INV", window(analyze_inv=0))):
            t, inp = c.check(w, f"synthetic {read_len} bp, {name}", var, sv)
            total += np.array(t["n_events"])
            dups += n_boxed(inp["recs"], (2,)) - t["n_members"][0] + int(sum((m & hostlib.SVEV_MEMBER_DUP != 0).sum() for m in t["members"][1:]))
            if name == "no INV":
                assert t["n_members"][1:] == [0, 0]
        assert total[1] > 0 and total.sum() > total[1] and dups > 0, (total, dups)
        # no sv lists were given to the events build: nothing is boxed by these kinds
        t, _ = c.check(window(), "lists that box nothing", var, (np.zeros_like(sv[0]), np.zeros_like(sv[1])))
        assert t["n_members"] == [0, 0, 0] and t["n_events"] == [0, 0, 0]
    finally:
        c.close()


def test_constructed_cases(eng):
    """The cases of tests/sv_cases.py, every read three times."""
    events = np.zeros(3, np.int64)
    for name, chroms, one, prm in sv_cases.all_cases():
        c = Case(eng, chroms, tripled(one), prm)
        try:
            var, sv = c.own_lists()
            for wname, w in (("whole", window()), ("-M 4 -B 10", window(min_support=4, balance_cutoff=10))):
                t, _ = c.check(w, f"{name}, {wname}", var, sv)
                events += np.array(t["n_events"])
        finally:
            c.close()
    assert (events > 0).all(), events


# ------------------------------------------------------------------------------------------------ hand-made lists
def with_close_end(c):
    return np.nonzero((np.diff(c.co.astype(np.int64)) > 0) & (c.batch.chr_id == 0))[0]


def hand_lists(rng, c, **kw):
    """random lists (sv_events_common.random_lists) for the reads of the case that have a close end, none for the others"""
    n = c.batch.n
    _, (sv, sv_n) = sc.random_lists(rng, n, lefts=LEFTS, **kw)
    drop = np.ones(n, dtype=bool)
    drop[with_close_end(c)] = False
    sv[drop] = np.zeros((), dtype=sv.dtype)
    sv_n[drop] = 0
    return sv, sv_n


def test_hand_made_lists(eng):
    """The device trusts the lists: the random arrays of the CPU test over a small searched batch (every read three times, so that
    LeftMostPos collides), with the same coverage assertions."""
    chroms, one = synthetic(130)
    c = Case(eng, chroms, tripled(one))
    seen = sc.new_seen()
    try:
        rng = np.random.default_rng(9100)
        for trial, wkw in enumerate([dict(), dict(min_support=2), dict(min_support=3, balance_cutoff=10), dict(balance_cutoff=0),
                                     dict(min_support=2, balance_cutoff=1), dict(), dict(balance_cutoff=0), dict(min_support=2)]):
            sv = hand_lists(rng, c, one_box=trial == 3, few_keys=trial in (1, 4, 6), p_fail=0.05 if trial < 4 else 0.01)
            t, inp = c.check(window(**HAND, **wkw), f"hand-made lists, trial {trial}", None, sv)
            assert n_boxed(inp["recs"]) > 100 and (inp["recs"]["slot"] > 0).any()
            sc.note_coverage(seen, inp, t, chroms[0][1])
    finally:
        c.close()
    sc.assert_coverage(seen)


def one_box_lists(c, kind, sizes, rng):
    """consecutive boxes (8 bases each, from 5000) of the given sizes for one kind, over the reads that have a close end"""
    reads = with_close_end(c)
    assert len(reads) >= sum(sizes), (len(reads), sizes)
    n = c.batch.n
    sv = np.zeros((n, hostlib.SV_SLOTS), dtype=hostlib.VARIANT_CAND_DTYPE)
    sv_n = np.zeros((n, 5), dtype=np.uint8)
    at = 0
    for b, size in enumerate(sizes):
        for i in reads[at:at + size]:
            r = sv[i, hostlib.SV_SLOT[kind]]
            r["bp_left"] = 5000 + 8 * b + rng.integers(0, 3)
            r["bp_right"] = rng.choice([6100, 6101, 6102])
            r["indel_size"] = rng.choice([0, 1, 2]) if kind == 2 else rng.choice([100, 99, 98])
            r["bp"] = rng.choice([30, 50, 51])
            r["nt_rot"] = 0 if kind == 5 else rng.integers(0, 3)
            r["left"], r["right"] = 100, 300
            sv_n[i, kind - 2] = 1
        at += size
    return sv, sv_n


@pytest.mark.parametrize("size", [1, 2, 63, 64, 65, 128, 129, LIMIT - 1, LIMIT, LIMIT + 1])
def test_box_sizes(eng, size):
    """One box of `size` reads -- the chunk seams of the order kernel and both sides of its LDS limit -- followed by an adjacent box
    of 5 and one of 1, the last of its table, for each of the three kinds."""
    chroms, one = synthetic(400, seed=7)
    c = Case(eng, chroms, tripled(one))
    try:
        rng = np.random.default_rng(size)
        for kind in sc.SV_TABLE_KINDS:
            t, inp = c.check(window(), f"box of {size}, kind {kind}", None, one_box_lists(c, kind, (size, 5, 1), rng))
            table = sc.SV_TABLE_KINDS.index(kind)
            assert n_boxed(inp["recs"]) == size + 6
            assert t["n_members"][table] == (size + 6 if kind != 2 else t["n_members"][0]) and sum(t["n_members"]) == t["n_members"][table]
            box = np.array([sc.fields_of(inp, int(m) & 0x7fffffff)[0] // 8 for m in t["members"][table]])
            assert (np.diff(box) >= 0).all() and len(set(box.tolist())) == 3
    finally:
        c.close()


def test_batch_sizes(eng):
    """Batches of 1, 63, 64 and 65 reads, and a batch in which nothing is boxed."""
    chroms, batch = synthetic(300, seed=11)
    for n in (1, 63, 64, 65):
        c = Case(eng, chroms, batch.slice(0, n))
        try:
            rng = np.random.default_rng(n)
            t, inp = c.check(window(**HAND), f"{n} reads", None, hand_lists(rng, c, p_boxed=1.0))
            assert n_boxed(inp["recs"]) == len(with_close_end(c))
            c.check(window(), f"{n} reads, own lists", *c.own_lists())
        finally:
            c.close()
    c = Case(eng, chroms, batch)
    try:
        var, sv = c.own_lists()
        t, inp = c.check(window(region_start=0xfffffff0, region_end=0xfffffffe), "nothing boxed", var, sv)
        assert n_boxed(inp["recs"]) == 0 and t["n_members"] == [0] * 3 and t["n_events"] == [0] * 3 and t["dropped_runs"] == [0] * 3
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ tensors, refusals, launch log
def test_tensors_refusals_and_launch_log(eng):
    chroms, batch = synthetic(200, seed=77)
    eng.load_reference(chroms)
    db = eng.upload(batch)
    L = eng._L
    some = (np.zeros((batch.n, hostlib.SV_SLOTS), dtype=hostlib.VARIANT_CAND_DTYPE), np.zeros((batch.n, 5), dtype=np.uint8))
    # not searched: refused with nothing launched
    eng.clear_launch_log()
    with pytest.raises(binding.PgError) as e:
        eng.sv_events(db, some)
    assert e.value.code == -1 and "searched" in str(e.value)
    assert eng.launch_log() == []
    eng.search_device(db)
    var, sv = eng.variant_candidates(db), eng.sv_candidates(db)
    vt, st = eng.variant_candidates_tensors(db), eng.sv_candidates_tensors(db)
    # searched, but no events build: refused by both entries, and there are no tables to size or download
    eng.clear_launch_log()
    with pytest.raises(binding.PgError) as e:
        eng.sv_events(db, sv)
    assert e.value.code == -1 and "pg_device_batch_events" in str(e.value)
    with pytest.raises(binding.PgError):
        eng.sv_events_tensors(db, st)
    with pytest.raises(binding.PgError):
        eng.sv_event_sizes(db)
    assert eng.launch_log() == []
    eng.events(db, window(), var, sv)
    with pytest.raises(binding.PgError):
        eng.sv_event_sizes(db)                                             # the events build alone makes no SV tables
    # the build logs one record of its own id and reports its HIP-event time
    eng.clear_launch_log()
    got = eng.sv_events(db, sv)
    assert [r.kernel for r in eng.launch_log()] == [binding.KERNEL_SV_EVENTS]
    assert eng.last_stats()[0] > 0.0 and sum(got["n_events"]) > 0
    # sv_events_tensors equals sv_events
    t = eng.sv_events_tensors(db, st)
    assert t["members"].is_cuda and t["events"].is_cuda
    assert_tables_equal(binding.sv_events_from_tensors(t), got, "tensors")
    # a host pointer to a _device entry is a status, and nothing is launched
    eng.clear_launch_log()
    host_c = np.ascontiguousarray(sv[0])
    assert L.pg_device_batch_sv_events_device(eng._h, db, host_c.ctypes.data, st["counts"].data_ptr()) == -1
    assert b"not device memory" in L.pg_last_error(eng._h)
    assert eng.launch_log() == []
    eng.sv_events(db, sv)
    host_members = np.zeros(batch.n, dtype=np.uint32)
    assert L.pg_device_batch_sv_events_download_device(eng._h, db, host_members.ctypes.data, None) == -1
    assert b"not device memory" in L.pg_last_error(eng._h)
    # a new events build discards the SV tables
    eng.events(db, window(min_support=2), var, sv)
    with pytest.raises(binding.PgError):
        eng.sv_event_sizes(db)
    again = eng.sv_events(db, sv)
    assert again["members_flat"].tobytes() == got["members_flat"].tobytes()
    eng.free_device_batch(db)
    # an empty batch: valid, nothing launched
    empty = eng.upload(batch.slice(0, 0))
    eng.search_device(empty)
    eng.events(empty, window())
    eng.clear_launch_log()
    t0 = eng.sv_events(empty, (some[0][:0], some[1][:0]))
    assert t0["n_members"] == [0] * 3 and t0["n_events"] == [0] * 3
    tt = eng.sv_events_tensors(empty, (st["cands"][:0], st["counts"][:0]))
    assert tt["members"].shape[0] == 0
    assert eng.launch_log() == []
    eng.free_device_batch(empty)


# ------------------------------------------------------------------------------------------------ end to end
def test_gold_set_end_to_end(eng, tmp_path):
    """The gold set as one window: searched and classified on the GPU, both sets of tables built on the GPU, reported on the host
    from them -- the gold reports, with their 13 inversion events of up to 664 tied reads."""
    from pindel_amd import hostio
    fa, reads_txt = gu.unpack(tmp_path)
    chroms = hostio.load_fasta(fa)
    batch = hostio.read_pindel_text(reads_txt, [n for n, _ in chroms], [len(s) - 200000 for _, s in chroms])
    c = Case(eng, chroms, batch)
    try:
        var, sv = c.own_lists()
        fo, fp = point_csr(c.res.far_off, c.res.far_runs)
        st = hostlib.default_settings(eng.max_mismatch_table())
        points = (c.co, c.cp, fo, fp, c.res.rc_flag)
        probe = str(tmp_path / "probe")
        hostlib.call_from_points(fa, reads_txt, probe, st, *points, variant_candidates=var, sv_candidates=sv, events=True, sv_events=True)
        gu.assert_reports_match_gold(probe)
        assert hostlib.last_event_fallback_windows() == 0 and hostlib.last_sv_event_table_windows() == (1, 0)
        wins = hostlib.last_event_windows()
        assert len(wins) == 1
        chr_index, ws, we, rs, re_, n_reads = [int(x) for x in wins[0]]
        w = window(chr_id=chr_index, win_end=we, region_start=rs, region_end=re_, min_support=st.min_support, balance_cutoff=st.balance_cutoff)
        ids = hostlib.name_ids(batch.names)
        tables = eng.events(c.db, w, var, sv, ids)
        got = eng.sv_events(c.db, sv)
        want = hostlib.sv_events_from_lists(chroms, batch.seq, batch.seq_off, batch.anchor_strand, c.res.rc_flag, c.co, c.cp, w, tables["reads"], sv)
        assert_tables_equal(got, want, "gold set")
        assert got["n_events"][1] >= 13 and max(int(e["n_reads"]) for e in got["events"][1]) >= 600 and got["n_events"][0] > 0
        prefix = str(tmp_path / "gpu_tables")
        key = (chr_index, ws, we)
        hostlib.call_from_points(fa, reads_txt, prefix, st, *points, variant_candidates=var, sv_candidates=sv, events={key: tables},
                                 sv_events={key: got})
        assert hostlib.last_event_table_windows() == (1, 1) and hostlib.last_sv_event_table_windows() == (1, 1)
        gu.assert_reports_match_gold(prefix)
    finally:
        c.close()
