"""The sixth part of the device classifier (pg_li.hip): the long-insertion position tables of a searched device batch
against hostlib.li_tables_from_lists -- the plain-loop statement on the host -- fed the per-read records the device's events build
left and the points the same search downloaded.  Every byte must be equal.  The reads are tests/li_cases.py: a 20 kb chromosome with
three long insertions, reads straddling each junction from both sides (a close end, no far end), reads without a close end and
ordinary deletion reads, 100 and 150 bases long."""
import numpy as np
import pytest

from pindel_amd import binding, hostlib
from tests import li_cases as lc
from tests.test_gpu_variant_candidates import point_csr

pytestmark = pytest.mark.gpu

WHOLE = dict(chr_id=0, win_end=0xffffffff, region_start=0, region_end=0xffffffff, min_support=1, balance_cutoff=100, analyze_td=1, analyze_inv=1)
LO, HI = lc.SPACER - 4 * lc.INSERT_SIZE, lc.SPACER + 20000 + 4 * lc.INSERT_SIZE


@pytest.fixture(scope="module")
def eng(engine_factory):
    e = engine_factory()
    e.load_reference(lc.chromosome())
    return e


class Case:
    """One searched batch, classified for the whole chromosome, with its downloaded points; on the device until close()."""

    def __init__(self, eng, recs, classify=True):
        self.eng, self.batch = eng, lc.batch_from(recs)
        self.db = eng.upload(self.batch)
        eng.search_device(self.db)
        self.res = eng.download(self.db)
        self.co, self.cp = point_csr(self.res.close_off, self.res.close_runs)
        self.fo = point_csr(self.res.far_off, self.res.far_runs)[0]
        if classify:
            eng.classify(self.db, binding.EventWindow(**WHOLE))

    def li_reads(self):
        return np.nonzero((np.diff(self.co.astype(np.int64)) > 0) & (np.diff(self.fo.astype(np.int64)) == 0))[0]

    def statement(self, lo, hi):
        recs = self.eng.events_download(self.db)["reads"]
        b = self.batch
        return hostlib.li_tables_from_lists(b.seq, b.seq_off, b.anchor_strand, b.chr_id, self.res.rc_flag, self.co, self.cp, self.fo, recs, 0, lo, hi)

    def check(self, lo, hi, what):
        got, want = self.eng.li(self.db, lo, hi), self.statement(lo, hi)
        assert got["n_members"] == want["n_members"] and got["n_positions"] == want["n_positions"], (what, got["n_members"], want["n_members"])
        assert got["members_flat"].tolist() == want["members_flat"].tolist(), what
        assert got["positions_flat"].tobytes() == want["positions_flat"].tobytes(), (what, got["positions_flat"][:4], want["positions_flat"][:4])
        assert self.eng.li_sizes(self.db) == (want["n_members"], want["n_positions"])
        return got

    def close(self):
        self.eng.free_device_batch(self.db)


@pytest.fixture(scope="module")
def pool(eng):
    """1080 junction reads, 6 without a close end, 6 deletion reads, searched once: which of them are LI reads"""
    recs = lc.records(180, 6, 6, seed=21)
    c = Case(eng, recs, classify=False)
    try:
        li_idx = c.li_reads()
    finally:
        c.close()
    assert len(li_idx) >= 1025
    return recs, li_idx


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(eng, pool, n):
    recs, li_idx = pool
    first = int(li_idx[0])
    c = Case(eng, recs[first:first + n])
    try:
        got = c.check(LO, HI, f"{n} reads")
        assert sum(got["n_members"]) == len(c.li_reads()) >= 1
        assert eng.last_stats()[0] > 0.0
        if n >= 63:
            assert min(got["n_members"]) > 0 and min(got["n_positions"]) > 0
            for s in range(2):
                assert (np.diff(got["positions"][s]["pos"].astype(np.int64)) > 0).all()
                assert got["positions"][s]["first"].tolist() == np.concatenate([[0], np.cumsum(got["positions"][s]["n_reads"])[:-1]]).tolist()
            flags = np.concatenate([got["positions"][s]["flags"] for s in range(2)])
            assert (flags & binding.LI_LONGER).any() and (flags & binding.LI_SHORTER).any()
    finally:
        c.close()


@pytest.mark.parametrize("k", [0, 1, 255, 256, 257, 1024, 1025])
def test_li_read_totals(eng, pool, k):
    """k LI reads beside the reads that are none: the compaction and the sort at one block, at its edge and beyond it; at 1024 the
    shared scan kernel has one digit count per thread (4 blocks x 256 digits), at 1025 two with a ragged tail (1280 counts)"""
    recs, li_idx = pool
    others = sorted(set(range(len(recs))) - set(li_idx.tolist()))
    pick = sorted(li_idx[:k].tolist() + others)
    c = Case(eng, [recs[i] for i in pick])
    try:
        got = c.check(LO, HI, f"{k} LI reads")
        assert sum(got["n_members"]) == k == len(c.li_reads())
        if k == 0:
            assert got["members_flat"].size == 0 and got["positions_flat"].size == 0
    finally:
        c.close()


def test_one_position_one_strand_and_the_window_ends(eng):
    c = Case(eng, lc.records(60, 3, 3, seed=3, only_plus=True, junctions=(lc.JUNCTIONS[0],)))
    try:
        got = c.check(LO, HI, "one strand")
        assert got["n_members"][0] >= 50 and got["n_members"][1] == 0 and got["n_positions"][1] == 0
        assert int(got["positions"][0]["n_reads"].max()) >= 30          # (the junction's position holds most of them)
        j = lc.JUNCTIONS[0]
        one = c.check(j - 1, j - 1, "lo == hi")
        assert one["n_positions"] == [1, 0] and int(one["positions"][0]["n_reads"][0]) == one["n_members"][0] == got["n_members"][0]
        assert one["members"][0].tolist() == sorted(one["members"][0].tolist())
        # a window that ends before / begins behind the junction: its reads count at that end (a read of random sequence may
        # have found a close end anywhere, so the number of positions comes from the downloaded points)
        raw = c.cp["abs_loc"][c.co[1:].astype(np.int64)[got["members"][0]] - 1].astype(np.int64)
        for lo, hi, what in ((LO, j - 40, "the junction's reads at hi"), (j + 40, HI, "the junction's reads at lo")):
            t = c.check(lo, hi, what)
            assert t["n_positions"][0] == len(set(np.clip(raw, lo, hi).tolist())) <= 3
            at_end = t["positions"][0][t["positions"][0]["pos"] == (hi if hi < j else lo)]
            assert len(at_end) == 1 and int(at_end["n_reads"][0]) >= 50
    finally:
        c.close()
    c = Case(eng, lc.records(40, 3, 3, seed=4))
    try:
        j = lc.JUNCTIONS[1]
        got = c.check(j, j, "lo == hi, both strands")
        assert got["n_positions"] == [1, 1] and min(got["n_members"]) >= 90
        assert int(got["positions"][1]["n_reads"][0]) == got["n_members"][1] and int(got["positions"][1]["first"][0]) == 0
    finally:
        c.close()


def test_shortened_read(eng):
    """reads that end in bytes outside ACGTN and keep their close end at the fourth attempt (rc_flag 2): the balance flags use the
    length they have afterwards"""
    c = Case(eng, lc.shortened_records(8) + lc.records(5, 2, 2, seed=6))
    try:
        got = c.check(LO, HI, "shortened")
        members = got["members_flat"]
        assert (c.res.rc_flag[members] == 2).any()
    finally:
        c.close()


def test_hand_made_lists_use_a_read_without_a_far_end(eng, pool):
    """The lists are trusted: a pair listed for a read that has no far end boxes it (or makes it Used), and it is no LI read then;
    a list that ends with VARIANT_MORE leaves it unresolved, and it stays one."""
    recs, li_idx = pool
    c = Case(eng, recs[:200], classify=False)
    try:
        li_reads = c.li_reads()
        assert len(li_reads) >= 100
        boxed, used, unresolved = (int(x) for x in li_reads[:3])
        n = c.batch.n
        var = np.zeros((n, 2, hostlib.VARIANT_CANDS), dtype=hostlib.VARIANT_CAND_DTYPE)
        var_n = np.zeros((n, 2), dtype=np.uint8)
        for i in (boxed, used):
            r = var[i, 0, 0]
            r["bp_left"], r["bp_right"], r["indel_size"], r["left"], r["right"], r["bp"] = lc.SPACER + 5000, lc.SPACER + 5061, 60, 100, 300, 40
            var_n[i, 0] = 1
        var["flags"][used, 0, 0] = hostlib.VARIANT_REF_END
        var_n[unresolved, 0] = hostlib.VARIANT_MORE
        sv = (np.zeros((n, hostlib.SV_SLOTS), dtype=hostlib.VARIANT_CAND_DTYPE), np.zeros((n, 5), dtype=np.uint8))
        ev = eng.events(c.db, binding.EventWindow(**WHOLE), (var, var_n), sv)
        assert ev["reads"]["flags"][boxed] & hostlib.EVR_BOXED and ev["reads"]["flags"][used] == hostlib.EVR_USED
        assert ev["reads"]["flags"][unresolved] == hostlib.EVR_UNRESOLVED
        got = c.check(LO, HI, "hand-made lists")
        members = set(got["members_flat"].tolist())
        assert boxed not in members and used not in members and unresolved in members
        assert members == set(li_reads.tolist()) - {boxed, used}
    finally:
        c.close()


def test_tensor_entries(eng, pool):
    import torch
    recs, _ = pool
    c = Case(eng, recs[:130])
    try:
        want = c.check(LO, HI, "tensors")
        t = eng.li_tensors(c.db, LO, HI)
        assert t["n_members"] == want["n_members"] and t["n_positions"] == want["n_positions"]
        assert t["members"].dtype == torch.int32 and t["members"].cpu().numpy().astype(np.uint32).tolist() == want["members_flat"].tolist()
        assert t["positions"].cpu().numpy().tobytes() == want["positions_flat"].tobytes()
    finally:
        c.close()


def test_refusals_launch_nothing(eng, pool):
    recs, _ = pool
    batch = lc.batch_from(recs[:70])
    db = eng.upload(batch)
    try:
        eng.clear_launch_log()
        with pytest.raises(binding.PgError, match="not been searched"):
            eng.li(db, LO, HI)
        assert eng.launch_log() == []
        eng.search_device(db)
        eng.clear_launch_log()
        with pytest.raises(binding.PgError, match="pg_device_batch_events has not been run"):
            eng.li(db, LO, HI)
        with pytest.raises(binding.PgError):
            eng.li_sizes(db)
        eng.classify(db, binding.EventWindow(**WHOLE))
        eng.clear_launch_log()
        with pytest.raises(binding.PgError, match="lo > hi"):
            eng.li(db, HI, LO)
        with pytest.raises(binding.PgError):
            eng.li_download(db)                                   # (a refused build leaves no tables)
        assert eng.launch_log() == []
        got = eng.li(db, LO, HI)
        assert sum(got["n_members"]) > 0
        # a host pointer given to the _device entry ends in a status code
        members = np.zeros(sum(got["n_members"]), dtype=np.uint32)
        positions = np.zeros(sum(got["n_positions"]), dtype=binding.LI_POS_DTYPE)
        L = eng._L
        assert L.pg_device_batch_li_download_device(eng._h, db, members.ctypes.data, None) == -1
        assert b"not device memory" in L.pg_last_error(eng._h)
        assert L.pg_device_batch_li_download_device(eng._h, db, None, positions.ctypes.data) == -1
        assert b"not device memory" in L.pg_last_error(eng._h)
        assert not members.any() and not positions["n_reads"].any()
    finally:
        eng.free_device_batch(db)


def test_launch_log_and_lifetime(eng, pool):
    recs, _ = pool
    batch = lc.batch_from(recs[:90])
    db = eng.upload(batch)
    try:
        eng.search_device(db)
        eng.clear_launch_log()
        eng.classify(db, binding.EventWindow(**WHOLE))
        assert all(r.kernel != binding.KERNEL_LI for r in eng.launch_log())      # classify does not run it
        with pytest.raises(binding.PgError):
            eng.li_sizes(db)
        eng.clear_launch_log()
        got = eng.li(db, LO, HI)
        log = eng.launch_log()
        assert len(log) >= 3 and all(r.kernel == binding.KERNEL_LI and r.blocks == binding.EVENT_BLOCK for r in log)
        ms, _ = eng.last_stats()
        assert ms > 0.0
        assert eng.li_download(db)["members_flat"].tolist() == got["members_flat"].tolist()
        # a new events build drops the tables
        eng.classify(db, binding.EventWindow(**WHOLE))
        with pytest.raises(binding.PgError, match="no long-insertion tables"):
            eng.li_sizes(db)
        with pytest.raises(binding.PgError):
            eng.li_download(db)
        assert eng.li(db, LO, HI)["members_flat"].tolist() == got["members_flat"].tolist()
    finally:
        eng.free_device_batch(db)


def test_empty_batch(eng):
    db = eng.upload(lc.batch_from(lc.records(1, 0, 0)).slice(0, 0))
    try:
        eng.search_device(db)
        eng.classify(db, binding.EventWindow(**WHOLE))
        eng.clear_launch_log()
        got = eng.li(db, LO, HI)
        assert got["n_members"] == [0, 0] and got["n_positions"] == [0, 0] and eng.launch_log() == []
    finally:
        eng.free_device_batch(db)
