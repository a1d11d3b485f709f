"""The fifth part of the device classifier (pg_report.hip): the report records and summaries of a searched device
batch against hostlib.report_reads_from_lists -- the plain-loop statement on the host -- fed the tables the device built, the
same lists and the points the same search downloaded.  Every byte must be equal.  And pg_device_batch_classify against the five
separate entries, with and without its list cut."""
import ctypes as C

import numpy as np
import pytest

from pindel_amd import binding, hostlib, synth
from tests import shortening_cases
from tests import sv_cases
from tests import variant_cases as vc
from tests.test_gpu_variant_candidates import point_csr, searched
from tests.test_report_reads_cpu import assert_coverage, new_seen, note_coverage

pytestmark = pytest.mark.gpu

B = binding.EVENT_BLOCK
WHOLE = dict(chr_id=0, win_end=0xffffffff, region_start=0, region_end=0xffffffff, min_support=1, balance_cutoff=100,
             analyze_td=1, analyze_inv=1)


def window(**kw):
    return binding.EventWindow(**{**WHOLE, **kw})


def tripled(batch):
    return shortening_cases.concat([batch, batch, batch])


class Case:
    """One searched batch with its points, kept on the device until close()."""

    def __init__(self, eng, chroms, batch, prm=None, bd=None, bd_off=None):
        self.eng, self.chroms, self.batch, self.prm = eng, chroms, batch, prm
        self.db, self.res = searched(eng, chroms, batch, bd, bd_off)
        self.co, self.cp = point_csr(self.res.close_off, self.res.close_runs)
        self.fo, self.fp = point_csr(self.res.far_off, self.res.far_runs)
        self._lists = None

    def own_lists(self):
        if self._lists is None:
            self._lists = (self.eng.variant_candidates(self.db), self.eng.sv_candidates(self.db, self.prm))
        return self._lists

    def first_run_points(self):
        """per read the points of the first run of its close list (0: no close end)"""
        runs, off = self.res.close_runs, self.res.close_off.astype(np.int64)
        per_run = runs["len_last"].astype(np.int64) - runs["len_first"].astype(np.int64) + 1
        out = np.zeros(self.batch.n, dtype=np.int64)
        has = off[1:] > off[:-1]
        out[has] = per_run[off[:-1][has]]
        return out

    def statement(self, ev, svt, var, sv):
        return hostlib.report_reads_from_lists(self.batch.anchor_strand, self.res.rc_flag, self.co, self.cp, self.fo, self.fp, ev, svt, var, sv)

    def check(self, w, what, var, sv, name_id=None, seen=None):
        """the two table builds, the records, and the host statement over the tables of the former"""
        ev = self.eng.events(self.db, w, var, sv, name_id)
        svt = self.eng.sv_events(self.db, sv)
        records, summaries = self.eng.report_reads(self.db, var, sv)
        want_r, want_s = self.statement(ev, svt, var, sv)
        assert self.eng.report_sizes(self.db) == (len(want_r), self.batch.n), what
        assert len(records) == sum(ev["n_members"]) + sum(svt["n_members"]), what
        assert_same(records, summaries, want_r, want_s, what)
        if seen is not None:
            note_coverage(seen, records, summaries, self.batch.anchor_strand, self.first_run_points())
        return records, summaries, ev, svt

    def close(self):
        self.eng.free_device_batch(self.db)


def assert_same(records, summaries, want_r, want_s, what):
    assert len(summaries) == len(want_s) and len(records) == len(want_r), (what, len(records), len(want_r))
    d = np.nonzero(summaries != want_s)[0]
    assert len(d) == 0, f"{what}: summaries differ for reads {d[:6].tolist()}: device {summaries[d[:3]].tolist()}, host {want_s[d[:3]].tolist()}"
    d = np.nonzero(records != want_r)[0]
    assert len(d) == 0, f"{what}: records differ for members {d[:6].tolist()}: device {records[d[:3]].tolist()}, host {want_r[d[:3]].tolist()}"
    assert summaries.tobytes() == want_s.tobytes() and records.tobytes() == want_r.tobytes(), what


@pytest.fixture(scope="module")
def eng(engine_factory):
    return engine_factory()


@pytest.fixture(scope="module")
def seen():
    return new_seen()


def synthetic(n, read_len=100, seed=142, mix=(0.2, 0.1, 0.3, 0.3, 0.1)):
    chroms = [("chrS", synth.make_reference(60_000, seed=41))]
    return chroms, synth.make_reads(chroms[0][1], n, read_len=read_len, seed=seed, mix=mix)


# ------------------------------------------------------------------------------------------------ searched reads, their own lists
@pytest.mark.parametrize("read_len", [100, 150])
def test_synthetic_reads_tripled(eng, seen, read_len):
    chroms, one = synthetic(260, read_len, 42 + read_len)
    c = Case(eng, chroms, tripled(one))
    try:
        var, sv = c.own_lists()
        mid = int(np.median(one.anchor_pos))
        same = np.tile(np.arange(one.n, dtype=np.uint32), 3)
        total = 0
        for name, w, ids in (("whole", window(), None), ("equal ids", window(), same), ("half region", window(region_end=mid), None),
                             ("-M 3 -B 10", window(min_support=3, balance_cutoff=10), same), ("no TD", window(analyze_td=0), None),
                             ("no INV", window(analyze_inv=0), None)):
            records, summaries, _, _ = c.check(w, f"synthetic {read_len} bp, {name}", var, sv, ids, seen)
            total += len(records)
        assert total > 0
        assert ((summaries["flags"] & hostlib.RS_CLOSE) != 0).tolist() == (np.diff(c.co.astype(np.int64)) > 0).tolist()
    finally:
        c.close()


def test_constructed_cases(eng, seen):
    """The cases of tests/variant_cases.py and tests/sv_cases.py, every read three times."""
    cases = [(n, ch, b, None) for n, ch, b in vc.all_cases()] + list(sv_cases.all_cases())
    members = 0
    for name, chroms, one, prm in cases:
        c = Case(eng, chroms, tripled(one), prm)
        try:
            var, sv = c.own_lists()
            records, _, _, _ = c.check(window(), name, var, sv, None, seen)
            members += len(records)
        finally:
            c.close()
    assert members > 0


def test_far_end_on_another_chromosome(eng, seen):
    name, chroms, batch, bd, bd_off = vc.translocation_case()
    c = Case(eng, chroms, batch, bd=bd, bd_off=bd_off)
    try:
        var, sv = c.own_lists()
        _, summaries, _, _ = c.check(window(), name, var, sv, None, seen)
        assert (summaries["far_chr"][(summaries["flags"] & hostlib.RS_FAR) != 0] != 0).any()
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ hand-made lists
def eligible(c):
    """reads of chromosome 0 with a close and a far end: the pairs of a hand-made list index their points"""
    return np.nonzero((np.diff(c.co.astype(np.int64)) > 0) & (np.diff(c.fo.astype(np.int64)) > 0) & (c.batch.chr_id == 0))[0]


def hand_lists(rng, c, reads, kinds):
    """One boxed pair of kinds[k] for reads[k] (bp_left from a few values inside the padded chromosome's first boxes), its close_idx
    and far_idx random points of the read -- for a read with two close runs or more, a point of a later run.  A TD pair comes with
    a DI pair in front of it half of the time (outside the region [0, 20000], so that the cascade passes it by)."""
    n = c.batch.n
    var = np.zeros((n, 2, hostlib.VARIANT_CANDS), dtype=hostlib.VARIANT_CAND_DTYPE)
    var_n = np.zeros((n, 2), dtype=np.uint8)
    sv = np.zeros((n, hostlib.SV_SLOTS), dtype=hostlib.VARIANT_CAND_DTYPE)
    sv_n = np.zeros((n, 5), dtype=np.uint8)
    nc, nf, first = np.diff(c.co.astype(np.int64)), np.diff(c.fo.astype(np.int64)), c.first_run_points()

    def fill(r, i):
        r["bp_left"] = rng.choice([5006, 5007, 5008, 9000])
        r["bp_right"] = rng.choice([6100, 6101, 6102])
        r["left"], r["right"] = 100, 300
        r["bp"] = rng.choice([30, 50, 51])
        r["close_idx"] = rng.integers(first[i], nc[i]) if nc[i] > first[i] else rng.integers(0, nc[i])
        r["far_idx"] = rng.integers(0, nf[i])
    for i, kind in zip(reads, kinds):
        if kind < 2:
            r = var[i, kind, 0]
            fill(r, i)
            r["indel_size"] = rng.choice([1, 2, 3]) if kind == 1 else rng.choice([20, 21])
            r["nt_rot"] = rng.integers(-3, 4) if kind == 1 else 0
            var_n[i, kind] = 1
            continue
        if kind == 3 and rng.random() < 0.5:
            d = sv[i, 0]
            fill(d, i)
            d["bp_left"], d["bp_right"], d["indel_size"], d["nt_rot"] = 80000, 80100, 2, rng.integers(1, 4)
            sv_n[i, 0] = 1
        r = sv[i, hostlib.SV_SLOT[kind]]
        fill(r, i)
        r["indel_size"] = rng.choice([100, 99, 98])
        r["nt_rot"] = rng.integers(0, 3) if kind in (2, 4, 6) else 0
        if kind in (5, 6):
            r["flags"] = int(rng.integers(0, 4)) << 4
        sv_n[i, kind - 2] = 1
    return (var, var_n), (sv, sv_n)


def test_hand_made_lists(eng, seen):
    """The device trusts the lists: random pairs of every kind over a searched batch, every read three times (so that the inversions'
    boxes hold duplicates), with the coverage assertions of the CPU test -- the rc_flag 2 read comes with the constructed cases."""
    chroms, one = synthetic(200)
    c = Case(eng, chroms, tripled(one))
    try:
        rng = np.random.default_rng(9200)
        reads = eligible(c)
        assert len(reads) > 150 and (np.diff(c.res.close_off.astype(np.int64))[reads] >= 2).any()
        for trial in range(3):
            kinds = np.tile(rng.choice([0, 1, 1, 2, 3, 3, 4, 5, 5, 6], size=one.n), 3)[reads]
            var, sv = hand_lists(rng, c, reads, kinds)
            records, _, ev, svt = c.check(window(region_end=20000, min_support=trial + 1), f"hand-made lists, trial {trial}", var, sv, None, seen)
            assert len(records) > 100
    finally:
        c.close()


def test_coverage(seen):
    assert_coverage(seen)


def test_seams(eng):
    """Member totals of 0, 1, B - 1, B and B + 1 (one thread per member, B a block), over 560 reads; batches of 1, 63, 64 and 65
    reads with their own lists; nothing boxed."""
    chroms, batch = synthetic(560, seed=7)
    c = Case(eng, chroms, batch)
    try:
        reads = eligible(c)
        assert len(reads) >= B + 1, len(reads)
        rng = np.random.default_rng(3)
        for total in (0, 1, B - 1, B, B + 1):
            # (kinds whose member lists hold every boxed read: DI's drops its duplicates)
            var, sv = hand_lists(rng, c, reads[:total], np.resize([0, 1, 5, 6], total))
            records, _, _, _ = c.check(window(), f"{total} members", var, sv)
            assert len(records) == total
        var, sv = c.own_lists()
        records, _, _, _ = c.check(window(region_start=0xfffffff0, region_end=0xfffffffe), "nothing boxed", var, sv)
        assert len(records) == 0
    finally:
        c.close()
    for n in (1, 63, 64, 65):
        c = Case(eng, chroms, batch.slice(0, n))
        try:
            var, sv = c.own_lists()
            _, summaries, _, _ = c.check(window(), f"{n} reads", var, sv)
            assert len(summaries) == n
        finally:
            c.close()


# ------------------------------------------------------------------------------------------------ entries, refusals, the launch log
def test_tensors_refusals_and_launch_log(eng):
    chroms, batch = synthetic(200, seed=77)
    eng.load_reference(chroms)
    db = eng.upload(batch)
    L = eng._L
    none = (np.zeros((batch.n, 2, 4), dtype=binding.VARIANT_CAND_DTYPE), np.zeros((batch.n, 2), dtype=np.uint8))
    none_sv = (np.zeros((batch.n, binding.SV_SLOTS), dtype=binding.VARIANT_CAND_DTYPE), np.zeros((batch.n, 5), dtype=np.uint8))
    # not searched: refused, with nothing launched
    eng.clear_launch_log()
    with pytest.raises(binding.PgError) as e:
        eng.report_reads(db, none, none_sv)
    assert e.value.code == -1 and "searched" in str(e.value)
    with pytest.raises(binding.PgError) as e:
        eng.classify(db, window())
    assert e.value.code == -1 and "searched" in str(e.value)
    assert eng.launch_log() == []
    eng.search_device(db)
    var, sv = eng.variant_candidates(db), eng.sv_candidates(db)
    vt, st = eng.variant_candidates_tensors(db), eng.sv_candidates_tensors(db)
    # no events build, then no sv build: refused by both entries, and no sizes or download either
    eng.clear_launch_log()
    for tensors in (False, True):
        with pytest.raises(binding.PgError) as e:
            eng.report_reads_tensors(db, vt, st) if tensors else eng.report_reads(db, var, sv)
        assert e.value.code == -1 and "pg_device_batch_events " in str(e.value)
    with pytest.raises(binding.PgError):
        eng.report_sizes(db)
    assert eng.launch_log() == []
    ev = eng.events(db, window(), var, sv)
    eng.clear_launch_log()
    for tensors in (False, True):
        with pytest.raises(binding.PgError) as e:
            eng.report_reads_tensors(db, vt, st) if tensors else eng.report_reads(db, var, sv)
        assert e.value.code == -1 and "pg_device_batch_sv_events" in str(e.value)
    assert eng.launch_log() == []
    svt = eng.sv_events(db, sv)
    # a host pointer to a _device entry is a status, and nothing is launched
    eng.clear_launch_log()
    host_c = np.ascontiguousarray(var[0])
    args = [vt["cands"].data_ptr(), vt["counts"].data_ptr(), st["cands"].data_ptr(), st["counts"].data_ptr()]
    for k, bad in enumerate((host_c.ctypes.data, var[1].ctypes.data, np.ascontiguousarray(sv[0]).ctypes.data, sv[1].ctypes.data)):
        a = list(args)
        a[k] = bad
        assert L.pg_device_batch_report_reads_device(eng._h, db, *a) == -1
        assert b"not device memory" in L.pg_last_error(eng._h)
    assert L.pg_device_batch_report_reads(eng._h, db, None, var[1].ctypes.data, host_c.ctypes.data, sv[1].ctypes.data) == -1
    assert eng.launch_log() == []
    # the build logs its own kernel id and reports its HIP-event time; the tensor entries equal the host ones
    records, summaries = eng.report_reads(db, var, sv)
    assert [(r.kernel, r.blocks) for r in eng.launch_log()] == [(binding.KERNEL_REPORT, B)]
    assert eng.last_stats()[0] > 0.0 and len(records) > 0
    t = eng.report_reads_tensors(db, vt, st)
    assert t["records"].is_cuda and t["summaries"].is_cuda
    assert t["records"].cpu().numpy().tobytes() == records.tobytes() and t["summaries"].cpu().numpy().tobytes() == summaries.tobytes()
    host_r = np.zeros(len(records), dtype=binding.REPORT_READ_DTYPE)
    assert L.pg_device_batch_report_download_device(eng._h, db, host_r.ctypes.data, None) == -1
    assert b"not device memory" in L.pg_last_error(eng._h)
    # a new events build drops the records, and so does a new sv build
    eng.events(db, window(), var, sv)
    with pytest.raises(binding.PgError):
        eng.report_download(db)
    eng.sv_events(db, sv)
    eng.report_reads(db, var, sv)
    eng.sv_events(db, sv)
    with pytest.raises(binding.PgError):
        eng.report_sizes(db)
    # classify: a bad max_listed, window or -v is refused before anything is launched
    eng.clear_launch_log()
    for kw in (dict(max_listed=-1), dict(max_listed=5), dict(window=window(chr_id=3)), dict(settings=(0.01, 30, -1))):
        with pytest.raises(binding.PgError) as e:
            eng.classify(db, **{"window": window(), **kw})
        assert e.value.code == -1
    assert eng.launch_log() == []
    eng.free_device_batch(db)
    # an empty batch: valid, nothing launched
    empty = eng.upload(batch.slice(0, 0))
    eng.search_device(empty)
    eng.clear_launch_log()
    eng.events(empty, window())
    eng.sv_events(empty, (none_sv[0][:0], none_sv[1][:0]))
    r0, s0 = eng.report_reads(empty, (none[0][:0], none[1][:0]), (none_sv[0][:0], none_sv[1][:0]))
    assert len(r0) == 0 and len(s0) == 0 and eng.report_sizes(empty) == (0, 0)
    eng.classify(empty, window())
    assert eng.report_sizes(empty) == (0, 0) and eng.event_sizes(empty) == ([0] * 4, [0] * 4, 0)
    assert eng.launch_log() == []
    eng.free_device_batch(empty)


# ------------------------------------------------------------------------------------------------ one call per window
def cut(lists, max_listed):
    """pg_device_batch_classify's cut, by hand: a count byte above max_listed becomes max_listed | VARIANT_MORE"""
    cands, counts = lists
    counts = counts.copy()
    counts[(counts & 0x7f) > max_listed] = max_listed | hostlib.VARIANT_MORE
    return cands, counts


@pytest.mark.parametrize("max_listed", [4, 1, 0])
def test_classify_equals_the_separate_entries(eng, max_listed):
    chroms, one = synthetic(260, 100, 142)
    c = Case(eng, chroms, tripled(one))
    try:
        var, sv = c.own_lists()
        ids = np.tile(np.arange(one.n, dtype=np.uint32), 3)
        for name, w, name_id in (("whole", window(), None), ("-M 3, equal ids", window(min_support=3), ids)):
            what = f"classify, max_listed {max_listed}, {name}"
            var_c, sv_c = cut(var, max_listed), cut(sv, max_listed)
            want_r, want_s, want_ev, want_sv = c.check(w, what, var_c, sv_c, name_id)
            eng.clear_launch_log()
            eng.classify(c.db, w, None, max_listed, name_id)
            log = [(r.kernel, r.blocks) for r in eng.launch_log()]
            assert [k for k, _ in log[:2]] == [4, 5] and log[-1] == (binding.KERNEL_REPORT, B)
            assert ((binding.KERNEL_REPORT, 0) in log) == (max_listed < 4)
            assert eng.last_stats()[0] > 0.0
            ev, svt = eng.events_download(c.db), eng.sv_events_download(c.db)
            assert ev["unresolved"] == want_ev["unresolved"] and ev["n_members"] == want_ev["n_members"] and ev["n_events"] == want_ev["n_events"], what
            assert svt["n_members"] == want_sv["n_members"] and svt["n_events"] == want_sv["n_events"] and svt["dropped_runs"] == want_sv["dropped_runs"], what
            for key in ("reads", "members_flat", "events_flat"):
                assert ev[key].tobytes() == want_ev[key].tobytes(), (what, key)
            for key in ("members_flat", "events_flat"):
                assert svt[key].tobytes() == want_sv[key].tobytes(), (what, key)
            records, summaries = eng.report_download(c.db)
            assert_same(records, summaries, want_r, want_s, what)
            if max_listed == 0:
                # every read that reaches a list with a pair is unresolved, and nothing is boxed
                has_pair = ((var[1] & 0x7f) > 0).any(axis=1) | ((sv[1] & 0x7f) > 0).any(axis=1)
                assert ev["unresolved"] == int(has_pair.sum()) > 0 and len(records) == 0
            else:
                assert len(records) > 0
    finally:
        c.close()
