"""The seventh part of the device classifier (pg_int.hip): the interchromosomal junction tables of a searched device
batch against hostlib.int_tables_from_lists -- the plain-loop statement on the host -- fed the points the same search downloaded.
Every byte must be equal.  The far ends on other chromosomes come from the search itself: the three-chromosome reference of
tests/interchr_synth.py, its own split reads and the junction reads of tests/int_cases.py, searched with a hint table whose windows
lie around the planted breakpoints."""
import ctypes as C

import numpy as np
import pytest

from pindel_amd import binding, hostio, hostlib
from tests import int_cases as ic
from tests import interchr_synth as syn
from tests.test_gpu_variant_candidates import point_csr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(engine_factory, tmp_path_factory):
    s = syn.make(str(tmp_path_factory.mktemp("int_tables")))
    chroms = hostio.load_fasta(s["fasta"])
    eng = engine_factory()
    eng.load_reference(chroms)
    rank = hostlib.chr_ranks([n for n, _ in chroms])
    assert rank.tolist() == [0, 1, 2] == eng.chr_ranks().tolist()
    return dict(s=s, chroms=chroms, eng=eng, rank=rank, biol=ic.biological(chroms), table=ic.hint_table())


class Case:
    """One batch searched with the hint table, with its downloaded points; on the device until close()."""

    def __init__(self, world, batch):
        self.world, self.eng, self.batch = world, world["eng"], batch
        self.db = self.eng.upload(batch)
        self.eng.search_table_device(self.db, world["table"])
        self.res = self.eng.download(self.db)
        self.co, self.cp = point_csr(self.res.close_off, self.res.close_runs)
        self.fo, self.fp = point_csr(self.res.far_off, self.res.far_runs)

    def junction_reads(self):
        """reads with a close end and a far end whose first point lies on another chromosome"""
        has = (np.diff(self.co.astype(np.int64)) > 0) & (np.diff(self.fo.astype(np.int64)) > 0)
        first = np.minimum(self.fo[:-1].astype(np.int64), max(len(self.fp) - 1, 0))
        far_chr = self.fp["chr_id"][first] if len(self.fp) else np.zeros(self.batch.n, np.int16)
        return np.nonzero(has & (far_chr != self.batch.chr_id))[0]

    def runs_of(self, members):
        """(close runs, far runs) per member, from the CSR offsets of the downloaded run lists"""
        return np.diff(self.res.close_off.astype(np.int64))[members], np.diff(self.res.far_off.astype(np.int64))[members]

    def pair_depends_on_direction(self, i):
        """read i (not shortened) has a template pair, and the ascending scan picks another one than the descending scan"""
        c = self.cp["length"][int(self.co[i]):int(self.co[i + 1])].tolist()
        f = self.fp["length"][int(self.fo[i]):int(self.fo[i + 1])].tolist()
        length = int(self.batch.seq_off[i + 1] - self.batch.seq_off[i])

        def pair(asc):
            for a in (range(len(c)) if asc else range(len(c) - 1, -1, -1)):
                for b in (range(len(f) - 1, -1, -1) if asc else range(len(f))):
                    if c[a] + f[b] == length:
                        return a, b
            return None
        return self.res.rc_flag[i] == 0 and pair(True) is not None and pair(True) != pair(False)

    def statement(self, rank=None):
        b = self.batch
        return hostlib.int_tables_from_lists(b.seq, b.seq_off, b.anchor_strand, b.chr_id, self.res.rc_flag, self.co, self.cp, self.fo, self.fp,
                                             self.world["rank"] if rank is None else rank)

    def check(self, what, rank=None):
        got, want = self.eng.int_calls(self.db, rank), self.statement(rank)
        assert got["members"].tolist() == want["members"].tolist(), what
        assert got["calls"].tobytes() == want["calls"].tobytes(), (what, got["calls"][:4], want["calls"][:4])
        assert self.eng.int_sizes(self.db) == (len(want["members"]), len(want["calls"]))
        return got

    def close(self):
        self.eng.free_device_batch(self.db)


@pytest.fixture(scope="module")
def pool(world):
    """320 junction reads of every kind and 30 reads that are none, searched once: which of them are junction reads"""
    recs = ic.records(world["biol"], 320, seed=2, shortened_every=7, snp_every=5)
    c = Case(world, ic.batch_from(recs))
    try:
        idx = c.junction_reads()
    finally:
        c.close()
    assert len(idx) >= 300
    return recs, idx, ic.fillers(world["biol"], 30)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(world, pool, n):
    recs, idx, _ = pool
    first = int(idx[0])
    c = Case(world, ic.batch_from(recs[first:first + n]))
    try:
        got = c.check(f"{n} reads")
        calls, members = got["calls"], got["members"]
        assert 1 <= len(members) <= len(c.junction_reads()) and world["eng"].last_stats()[0] > 0.0
        assert int(calls["n_reads"].sum()) == len(members)
        assert calls["first"].tolist() == np.concatenate([[0], np.cumsum(calls["n_reads"])[:-1]]).tolist()
        if n >= 63:
            flags = calls["flags"]
            for bit in (binding.INT_ANCHOR_MINUS, binding.INT_FAR_MINUS, binding.INT_FALLBACK):
                assert (flags & bit).any() and not (flags & bit).all(), bit        # both anchor strands, both far strands, both kinds of call
            fallback = (flags & binding.INT_FALLBACK) != 0
            assert (calls["nt_len"][fallback] > 0).any() and not calls["nt_len"][~fallback].any() and not calls["nt_off"][~fallback].any()
            assert len(set(calls["chr"].tolist())) == 3 and (calls["chr"] != calls["far_chr"]).all()
            assert (calls["n_reads"] >= 2).any()
            assert (c.res.rc_flag[members] == 2).any()                             # shortened reads among the members
            # the walk over run pairs is exercised: members with several close runs AND several far runs (the reads with a planted
            # mismatch in either part), and members whose pair is another one under the opposite scan direction
            close_runs, far_runs = c.runs_of(members)
            assert ((close_runs > 1) & (far_runs > 1)).sum() >= 5
            assert sum(c.pair_depends_on_direction(int(i)) for i in members) >= 10
    finally:
        c.close()


@pytest.mark.parametrize("k", [0, 1, 255, 256, 257])
def test_junction_read_totals(world, pool, k):
    """k junction reads beside 30 reads that are none: the compaction and the sort at one block, at its edge and beyond it"""
    recs, idx, others = pool
    picked = [recs[i] for i in idx[:k].tolist()]
    mixed = picked + others
    order = np.random.default_rng(k).permutation(len(mixed))
    c = Case(world, ic.batch_from([mixed[i] for i in order]))
    try:
        got = c.check(f"{k} junction reads")
        assert len(c.junction_reads()) == k                       # (from the downloaded points: the totals are the test's, not assumed)
        assert len(got["members"]) <= k and (k == 0 or len(got["members"]) > 0)
        assert set(got["members"].tolist()) <= set(c.junction_reads().tolist())
        if k == 0:
            assert got["members"].size == 0 and got["calls"].size == 0
        # the duplicate name of the reference: with equal ranks for two of the chromosomes their reads are no junction reads
        if k == 257:
            merged = c.check("equal ranks", rank=np.array([0, 0, 1], dtype=np.int32))
            assert 0 < len(merged["members"]) < len(got["members"])
            assert not ((merged["calls"]["chr"] <= 1) & (merged["calls"]["far_chr"] <= 1)).any()
    finally:
        c.close()


def test_the_synthetic_sample_itself(world):
    """the split reads of tests/interchr_synth.py (11 per side and strand of every junction)"""
    chroms = world["chroms"]
    batch = hostio.read_pindel_text(world["s"]["reads_txt"], [n for n, _ in chroms], [len(q) - 200000 for _, q in chroms])
    c = Case(world, batch)
    try:
        got = c.check("synthetic sample")
        assert len(c.junction_reads()) >= 60 and len(got["members"]) >= 60
        assert {(int(x["chr"]), int(x["far_chr"])) for x in got["calls"]} >= {(0, 1), (1, 0), (1, 2), (2, 0)}
        assert (got["calls"]["nt_len"] > 0).any()                  # junction (iii) carries non-template bases
    finally:
        c.close()


def test_tensor_entries(world, pool):
    import torch
    recs, idx, _ = pool
    eng = world["eng"]
    c = Case(world, ic.batch_from(recs[:130]))
    try:
        want = c.check("tensors")
        t = eng.int_tensors(c.db)
        assert (t["n_members"], t["n_calls"]) == (len(want["members"]), len(want["calls"])) and t["n_calls"] > 0
        assert t["members"].dtype == torch.int32 and t["members"].cpu().numpy().astype(np.uint32).tolist() == want["members"].tolist()
        assert t["calls"].cpu().numpy().tobytes() == want["calls"].tobytes()
        # a host pointer given to the _device entry ends in a status code
        members = np.zeros(len(want["members"]), dtype=np.uint32)
        calls = np.zeros(len(want["calls"]), dtype=binding.INT_CALL_DTYPE)
        L = eng._L
        assert L.pg_device_batch_int_download_device(eng._h, c.db, members.ctypes.data, None) == -1
        assert b"not device memory" in L.pg_last_error(eng._h)
        assert L.pg_device_batch_int_download_device(eng._h, c.db, None, calls.ctypes.data) == -1
        assert not members.any() and not calls["n_reads"].any()
    finally:
        c.close()


def test_refusals_launch_nothing(world, pool):
    recs, _, _ = pool
    eng, rank = world["eng"], world["rank"]
    L = eng._L
    db = eng.upload(ic.batch_from(recs[:70]))
    try:
        eng.clear_launch_log()
        with pytest.raises(binding.PgError, match="not been searched"):
            eng.int_calls(db)
        assert eng.launch_log() == []
        eng.search_table_device(db, world["table"])
        eng.clear_launch_log()
        with pytest.raises(binding.PgError, match="no junction tables"):
            eng.int_sizes(db)
        assert L.pg_device_batch_int(eng._h, db, None) == -1 and b"null pg_int_window" in L.pg_last_error(eng._h)
        w = binding.IntWindow(None, 3)
        assert L.pg_device_batch_int(eng._h, db, C.addressof(w)) == -1 and b"null chr_rank" in L.pg_last_error(eng._h)
        for bad in (rank[:2], np.concatenate([rank, rank])):
            with pytest.raises(binding.PgError, match="n_chr is not the number of chromosomes"):
                eng.int_calls(db, np.ascontiguousarray(bad))
        with pytest.raises(binding.PgError):
            eng.int_download(db)                                  # (a refused build leaves no tables)
        assert eng.launch_log() == []
        assert len(eng.int_calls(db)["members"]) > 0
    finally:
        eng.free_device_batch(db)


def test_launch_log_and_lifetime(world, pool):
    recs, _, _ = pool
    eng = world["eng"]
    whole = binding.EventWindow(chr_id=0, win_end=0xffffffff, region_start=0, region_end=0xffffffff, min_support=1, balance_cutoff=100,
                                analyze_td=1, analyze_inv=1)
    db = eng.upload(ic.batch_from(recs[:90]))
    try:
        eng.search_table_device(db, world["table"])
        eng.clear_launch_log()
        eng.classify(db, whole)
        assert all(r.kernel != binding.KERNEL_INT for r in eng.launch_log())     # classify does not run it
        with pytest.raises(binding.PgError):
            eng.int_sizes(db)
        eng.clear_launch_log()
        got = eng.int_calls(db)
        log = eng.launch_log()
        assert len(log) >= 3 and all(r.kernel == binding.KERNEL_INT and r.blocks == binding.EVENT_BLOCK for r in log)
        assert eng.last_stats()[0] > 0.0
        assert eng.int_download(db)["members"].tolist() == got["members"].tolist() and len(got["members"]) > 0
        # the tables need no events build and survive one; a second search drops them
        eng.classify(db, whole)
        assert eng.int_download(db)["calls"].tobytes() == got["calls"].tobytes()
        eng.search_table_device(db, world["table"])
        with pytest.raises(binding.PgError, match="no junction tables"):
            eng.int_sizes(db)
        with pytest.raises(binding.PgError):
            eng.int_download(db)
        assert eng.int_calls(db)["calls"].tobytes() == got["calls"].tobytes()
        # without the table no far end leaves the anchor's chromosome: a valid build of empty tables
        eng.set_windows(db, None)
        eng.pack_search_device(db)
        eng.clear_launch_log()
        none = eng.int_calls(db)
        assert none["members"].size == 0 and none["calls"].size == 0 and len(eng.launch_log()) == 1
    finally:
        eng.free_device_batch(db)                                 # (free after a build)


def test_empty_batch(world, pool):
    recs, _, _ = pool
    eng = world["eng"]
    db = eng.upload(ic.batch_from(recs[:1]).slice(0, 0))
    try:
        eng.search_device(db)
        eng.clear_launch_log()
        got = eng.int_calls(db)
        assert got["members"].size == 0 and got["calls"].size == 0 and eng.launch_log() == [] and eng.int_sizes(db) == (0, 0)
    finally:
        eng.free_device_batch(db)
