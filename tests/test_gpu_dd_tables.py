"""The eighth part of the device classifier (pg_dd_tables.hip): the dispersed-duplication breakpoint tables, their
consensus and the containment verdicts of a close-searched device batch against hostlib.dd_tables_from_close -- the plain-loop
statement on the host -- both fed by the same close-only search: the statement's close ends are those a download of that search
delivers.  Every byte must be equal.  The reads are
those of tests/dd_tables_cases.py; what a case is meant to hold is asserted on the statement's output.  And the close-only search
of a resident batch (pg_device_batch_close_search) against pg_close_end_batch."""
import ctypes as C

import numpy as np
import pytest

from pindel_amd import binding, hostlib
from tests import dd_restated
from tests import dd_tables_cases as dc
from tests import instantiations as inst
from tests.test_gpu_variant_candidates import point_csr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(engine_factory):
    chroms, biol = dc.reference()
    eng = engine_factory()
    eng.load_reference(chroms)
    return dict(chroms=chroms, biol=biol, eng=eng, mm=eng.max_mismatch_table())


def close_from(res, n):
    """per read: has a close end, rc_flag, UP_Close.back()'s AbsLoc and LengthStr -- from a downloaded result, as pindel_pg -q reads them"""
    off, pts = point_csr(res.close_off, res.close_runs)
    has = (np.diff(off.astype(np.int64)) > 0).astype(np.uint8)
    last = np.maximum(off[1:].astype(np.int64) - 1, 0)
    la = np.where(has, pts["abs_loc"][last] if len(pts) else 0, 0).astype(np.uint32)
    ll = np.where(has, pts["length"][last] if len(pts) else 0, 0).astype(np.uint16)
    return res, has, np.asarray(res.rc_flag, dtype=np.uint8)[:n], la, ll


def close_ends(eng, batch):
    """... from pg_close_end_batch on the same reads"""
    return close_from(eng.close_end_batch(batch), batch.n)


class Case:
    """One plan of tests/dd_tables_cases.py: uploaded and close-searched, with the statement's tables; on the device until close()."""

    def __init__(self, world, plan, support=3, mmd=400):
        self.world, self.eng = world, world["eng"]
        self.batch, self.first, self.strand = plan.batch()
        self.support, self.mmd = support, mmd
        self.db = self.eng.upload(self.batch)
        self.eng.close_search(self.db)
        self.res, self.has, self.rc, self.la, self.ll = close_from(self.eng.download(self.db), self.batch.n)

    def statement(self, support=None, mmd=None):
        b = self.batch
        return hostlib.dd_tables_from_close(b.seq, b.seq_off, b.anchor_strand, self.has, self.rc, self.la, self.ll, self.first, self.strand, 0,
                                            self.world["chroms"][0][1], self.world["mm"], self.support if support is None else support,
                                            self.mmd if mmd is None else mmd)

    def check(self, what, support=None, mmd=None):
        want = self.statement(support, mmd)
        got = self.eng.dd_tables(self.db, self.first, self.strand, 0, self.support if support is None else support, self.mmd if mmd is None else mmd)
        assert got["members"].tobytes() == want["members"].tobytes(), (what, got["members"][:6], want["members"][:6])
        assert got["cands"].tobytes() == want["cands"].tobytes(), (what, got["cands"][:6], want["cands"][:6])
        assert got["cons"] == want["cons"], what
        assert self.eng.dd_sizes(self.db) == (len(want["members"]), len(want["cands"]), len(want["cons"]))
        c = want["cands"]
        assert int(c["n_reads"].sum()) == len(want["members"])
        assert c["first"].tolist() == np.concatenate([[0], np.cumsum(c["n_reads"])[:-1]]).astype(np.int64).tolist()[:len(c)]
        return want

    def close(self):
        self.eng.free_device_batch(self.db)


def contained_by_cpu(world, t):
    """PG_DD_CONTAINED of the tested candidates from pgh_dd_contains_cpu over their windows"""
    chrom = world["chroms"][0][1]
    tested = [c for c in t["cands"] if int(c["flags"]) & binding.DD_TESTED]
    q = [t["cons"][int(c["cons_off"]):int(c["cons_off"]) + int(c["cons_len"])].decode("latin-1") for c in tested]
    db = [chrom[int(c["win_start"]):int(c["win_start"]) + int(c["win_len"])] for c in tested]
    return [bool(int(c["flags"]) & binding.DD_CONTAINED) for c in tested], [bool(x) for x in dd_restated.cpu_contains(q, db, world["mm"])]


def _leads(c, t):
    """members with rc_flag 1 whose read as uploaded begins with bytes outside ACGTN"""
    m = t["members"][t["members"]["rc_flag"] == 1]
    return sum(1 for i in m["read"] if c.batch.seq[int(c.batch.seq_off[i])] not in b"ACGTN")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(world, n):
    c = Case(world, dc.sized_batch(world["biol"], n, seed=n), support=3 if n > 1 else 1)
    try:
        assert c.batch.n == n
        t = c.check(f"{n} reads")
        assert len(t["cands"]) >= 1 and world["eng"].last_stats()[0] > 0.0
        if n >= 63:
            assert set(t["cands"]["seg"].tolist()) == {0, 1} and len(set(t["cands"]["n_reads"].tolist())) >= 2
            flags = t["cands"]["flags"]
            assert (flags & binding.DD_CONTAINED).any() and not (flags & binding.DD_CONTAINED).all() and (flags & binding.DD_TESTED).all()
            rc = t["members"]["rc_flag"]
            assert (rc == 2).any() and (rc == 0).any() and (rc == 1).any()          # reads the search shortened; reads it turned round
            assert _leads(c, t) >= 2
            got, want = contained_by_cpu(world, t)
            assert got == want
    finally:
        c.close()


@pytest.mark.parametrize("k", [0, 1, 63, 64, 65])
def test_candidate_counts(world, k):
    c = Case(world, dc.counted_candidates(world["biol"], k, seed=k))
    try:
        t = c.check(f"{k} candidates")
        assert len(t["cands"]) == k and len(t["members"]) == 3 * k
        assert (np.diff(c.first.astype(np.int64)) == 0).sum() == 2                 # segments of no reads
        assert not c.has.all() and c.has.sum() >= 3 * k + 10                       # reads without a close end; DD reads that are no members
        assert int(c.first[-1]) < c.batch.n                                        # reads outside every segment
        in_tables = set(t["members"]["read"].tolist())
        wrong = [i for i in range(int(c.first[-1])) if c.has[i] and i not in in_tables]
        seg_of = np.searchsorted(c.first, np.array(wrong), side="right") - 1
        strands = np.frombuffer(c.strand, dtype=np.uint8)
        assert (c.batch.anchor_strand[wrong] != strands[seg_of]).sum() == 6         # a read whose strand differs from its segment's
        short = (c.batch.anchor_strand[wrong] == strands[seg_of]).sum()             # support of min_bp_support - 1 (and a chance close end)
        assert 4 <= short <= 6
        one = c.check("min_bp_support 1", support=1)                                # ... which min_bp_support 1 admits
        assert len(one["cands"]) == k + 2 + (short - 4) and (one["cands"]["n_reads"] == 2).sum() == 2
        if k >= 63:
            got, want = contained_by_cpu(world, t)
            assert got == want and True in got and False in got
    finally:
        c.close()


@pytest.mark.parametrize("k", [255, 256, 257, 1024, 1025])
def test_dd_read_totals(world, k):
    """k DD reads beside reads that are none: the compaction, the sort and the head flags at one block of DD records, at its edge and
    beyond it (dd_key_of reads blk[m / PG_EV_BLOCK]); from 258 reads on one key's members are the sorted records 255, 256 and 257"""
    c = Case(world, dc.dd_read_totals(world["biol"], k, seed=k))
    try:
        t = c.check(f"{k} DD reads")
        dc.assert_dd_read_totals(t, c.statement(support=1), k)
        c.check(f"{k} DD reads, min_bp_support 1", support=1)
    finally:
        c.close()


@pytest.mark.parametrize("m", [63, 64, 65, 130])
def test_one_candidate_of_many_members(world, m):
    c = Case(world, dc.one_big_candidate(world["biol"], m, seed=m))
    try:
        t = c.check(f"{m} members")
        assert sorted(t["cands"]["n_reads"].tolist()) == [4, m]
        assert len(set(t["cands"]["pos"].tolist())) == 2 and abs(int(t["cands"]["pos"][0]) - int(t["cands"]["pos"][1])) == 1   # one breakpoint, two segments
        big = t["cands"][int(np.argmax(t["cands"]["n_reads"]))]
        mem = t["members"][int(big["first"]):int(big["first"]) + m]
        assert mem["read"].tolist() == sorted(mem["read"].tolist())                # ascending read index within a key
        u = np.diff(c.batch.seq_off.astype(np.int64))[mem["read"]] - mem["close_len"]
        assert len(set(u.tolist())) >= 20 and int(big["cons_len"]) == int(u.max())  # n shrinks along the columns, to one member
    finally:
        c.close()


def test_vote_edges(world):
    c = Case(world, dc.vote_edges(world["biol"]))
    try:
        t = c.check("vote edges")
        cands = t["cands"]
        lens = {(int(x["seg"]), int(x["pos"]) - dc.SPACER): int(x["cons_len"]) for x in cands}
        key = lambda s, p: next(v for (ss, pp), v in lens.items() if ss == s and abs(pp - p) <= 1)
        assert key(0, 5000) == dc.GUARD + 16                                       # 4 of 5 accepted: the consensus runs through
        assert key(0, 5200) == 15                                                  # 3 of 4 rejected in column 15: exactly 15, kept
        assert key(0, 5400) == 0                                                   # a tie in column 14: 14 columns, dropped
        dropped = next(x for x in cands if int(x["cons_len"]) == 0)
        assert int(dropped["flags"]) == 0 and int(dropped["win_len"]) == 0
        assert key(1, 5000) == dc.GUARD + 9                                        # the tie of a byte >= 0x80 with a base ends it there
        nul = next(x for x in cands if int(x["seg"]) == 0 and abs(int(x["pos"]) - dc.SPACER - 5600) <= 1)
        assert t["cons"][int(nul["cons_off"]) + dc.GUARD + 3] == 0                   # rc4n of an IUPAC letter: byte 0 wins its column
        assert (t["members"]["rc_flag"] == 2).sum() == 3
        # members found after one reverse complement, on either strand; five of them behind two bytes outside ACGTN, which that strips:
        # their post-state begins two bytes into the read as uploaded
        flipped = t["members"][t["members"]["rc_flag"] == 1]
        assert len(flipped) == 10 and set(c.batch.anchor_strand[flipped["read"]].tolist()) == {ord("+"), ord("-")} and _leads(c, t) == 5
        for x in cands:
            if abs(int(x["pos"]) - dc.SPACER - (5800 if int(x["seg"]) == 0 else 5600)) <= 1:
                assert int(x["cons_len"]) == dc.GUARD + 20 and (t["members"]["rc_flag"][int(x["first"]):int(x["first"]) + 5] == 1).all()
        got, want = contained_by_cpu(world, t)
        assert got == want and got.count(True) == 1
        # a window clamped at 0 and cut by the chromosome's end
        wide = c.check("wide windows", mmd=200000)
        tested = wide["cands"][(wide["cands"]["flags"] & 1) != 0]
        assert (tested["win_start"] == 0).all() and (tested["win_len"] == len(world["chroms"][0][1])).all()
    finally:
        c.close()


def test_tensor_entries(world):
    import torch
    eng = world["eng"]
    c = Case(world, dc.vote_edges(world["biol"]))
    try:
        want = c.check("tensors")
        t = eng.dd_tensors(c.db, c.first, c.strand, 0, 3, 400)
        assert (t["n_members"], t["n_cands"], t["cons_bytes"]) == (len(want["members"]), len(want["cands"]), len(want["cons"])) and t["n_cands"] > 0
        assert t["members"].dtype == torch.uint8 and t["members"].cpu().numpy().tobytes() == want["members"].tobytes()
        assert t["cands"].cpu().numpy().tobytes() == want["cands"].tobytes() and t["cons"].cpu().numpy().tobytes() == want["cons"]
        # a host pointer given to the _device entry ends in a status code
        members = np.zeros(len(want["members"]), dtype=binding.DD_MEMBER_DTYPE)
        L = eng._L
        assert L.pg_device_batch_dd_download_device(eng._h, c.db, members.ctypes.data, None, None) == -1
        assert b"not device memory" in L.pg_last_error(eng._h) and not members["close_len"].any()
        assert L.pg_device_batch_dd_download(eng._h, c.db, None, None, None) == 0      # any pointer may be NULL
    finally:
        c.close()


def test_refusals_launch_nothing(world):
    eng = world["eng"]
    L = eng._L
    batch, first, strand = dc.vote_edges(world["biol"]).batch()
    db = eng.upload(batch)
    try:
        eng.clear_launch_log()
        with pytest.raises(binding.PgError, match="not been close-searched"):
            eng.dd_tables(db, first, strand, 0)
        assert eng.launch_log() == []
        eng.close_search(db)
        eng.clear_launch_log()
        with pytest.raises(binding.PgError, match="no DD tables"):
            eng.dd_sizes(db)
        assert L.pg_device_batch_dd(eng._h, db, None) == -1 and b"null pg_dd_window" in L.pg_last_error(eng._h)
        f = np.ascontiguousarray(first, dtype=np.uint32)
        s = np.frombuffer(strand, dtype=np.uint8)
        for w, text in ((binding.DdWindow(None, s.ctypes.data, 2, 0, 3, 400), b"null segment array"),
                        (binding.DdWindow(f.ctypes.data, None, 2, 0, 3, 400), b"null segment array")):
            assert L.pg_device_batch_dd(eng._h, db, C.addressof(w)) == -1 and text in L.pg_last_error(eng._h)
        down = first.copy()
        down[1] = down[2] + 1
        beyond = first.copy()
        beyond[2] = batch.n + 1
        for args, text in (((down, strand, 0), "seg_first decreases"), ((beyond, strand, 0), "beyond the batch"), ((first, b"+?", 0), "neither"),
                           ((first, strand, 1), "chr_id"), ((first, strand, -1), "chr_id")):
            with pytest.raises(binding.PgError, match=text):
                eng.dd_tables(db, *args)
        for mmd in (0, -5):
            with pytest.raises(binding.PgError, match="min_map_distance"):
                eng.dd_tables(db, first, strand, 0, 3, mmd)
        with pytest.raises(binding.PgError):
            eng.dd_download(db)                                   # (a refused build leaves no tables)
        assert eng.launch_log() == []
        assert len(eng.dd_tables(db, first, strand, 0)["members"]) > 0
        # n_seg 0 and "no candidate" are valid
        none = eng.dd_tables(db, [], b"", 0)
        assert none["members"].size == 0 and none["cands"].size == 0 and none["cons"] == b"" and eng.dd_sizes(db) == (0, 0, 0)
        none = eng.dd_tables(db, first, strand, 0, 100)
        assert none["members"].size == 0 and none["cands"].size == 0
    finally:
        eng.free_device_batch(db)


def test_launch_log_and_lifetime(world):
    eng = world["eng"]
    batch, first, strand = dc.vote_edges(world["biol"]).batch()
    whole = binding.EventWindow(chr_id=0, win_end=0xffffffff, region_start=0, region_end=0xffffffff, min_support=1, balance_cutoff=100,
                                analyze_td=1, analyze_inv=1)
    db = eng.upload(batch)
    try:
        eng.close_search(db)
        eng.clear_launch_log()
        got = eng.dd_tables(db, first, strand, 0)
        log = eng.launch_log()
        assert len(log) >= 5 and all(r.kernel == binding.KERNEL_DD_TABLES for r in log)      # (the containment launch is not logged)
        assert {r.blocks for r in log} == {binding.EVENT_BLOCK}
        assert eng.last_stats()[0] > 0.0
        assert eng.dd_download(db)["cands"].tobytes() == got["cands"].tobytes() and len(got["cands"]) > 0
        # a full search keeps the batch close-searched and drops the tables; classify does not run the build
        eng.pack_search_device(db)
        with pytest.raises(binding.PgError, match="no DD tables"):
            eng.dd_sizes(db)
        eng.clear_launch_log()
        eng.classify(db, whole)
        assert all(r.kernel != binding.KERNEL_DD_TABLES for r in eng.launch_log())
        with pytest.raises(binding.PgError, match="no DD tables"):
            eng.dd_download(db)
        assert eng.dd_tables(db, first, strand, 0)["cands"].tobytes() == got["cands"].tobytes()
        # ... and a close search after it drops them again
        eng.close_search(db)
        with pytest.raises(binding.PgError, match="no DD tables"):
            eng.dd_sizes(db)
        again = eng.dd_tables(db, first, strand, 0)
        assert again["cands"].tobytes() == got["cands"].tobytes() and again["cons"] == got["cons"]
    finally:
        eng.free_device_batch(db)                                 # (free after a build)


def test_empty_batch(world):
    eng = world["eng"]
    batch, _, _ = dc.vote_edges(world["biol"]).batch()
    db = eng.upload(batch.slice(0, 0))
    try:
        eng.close_search(db)
        eng.clear_launch_log()
        got = eng.dd_tables(db, [0, 0], b"+", 0)
        assert got["members"].size == 0 and got["cands"].size == 0 and eng.launch_log() == [] and eng.dd_sizes(db) == (0, 0, 0)
    finally:
        eng.free_device_batch(db)


# ------------------------------------------------------------------------------------------------ the close-only search
def _same_close(eng, db, res, n):
    got = eng.download(db)
    assert got.close_off.tolist() == res.close_off.tolist() and got.close_runs.tobytes() == res.close_runs.tobytes()
    assert np.asarray(got.rc_flag)[:n].tolist() == np.asarray(res.rc_flag)[:n].tolist()
    assert int(got.far_off[-1]) == 0


def test_close_search_is_the_close_end(world):
    eng = world["eng"]
    batch, first, strand = dc.sized_batch(world["biol"], 257, seed=3).batch()
    res, has, rc, la, ll = close_ends(eng, batch)
    whole = binding.EventWindow(chr_id=0, win_end=0xffffffff, region_start=0, region_end=0xffffffff, min_support=1, balance_cutoff=100,
                                analyze_td=1, analyze_inv=1)
    db = eng.upload(batch)
    try:
        eng.clear_launch_log()
        eng.close_search(db)
        log = eng.launch_log()
        # the one search launch is the close-only kernel tests/instantiations.py names for this batch
        max_len = int(batch.lengths().max())
        want = [r for r in inst.expected_launches(max_len, inst.levels_of(max_len), True, True, inst.CLOSE, n_reads=batch.n, pack=True, exact=False)
                if r[0] == inst.SEARCH]
        got = [tuple(r) for r in log if r.kernel == inst.SEARCH]
        assert got == want and len(got) == 1 and inst.kernel_of(got[0]) in inst.ALL_KERNELS and got[0][4] == inst.CLOSE
        ms, runs = eng.last_stats()
        assert ms > 0.0 and runs > 0
        _same_close(eng, db, res, batch.n)
        t = eng.download_tensors(db)
        assert t["close_last"].cpu().numpy().astype(np.uint32)[has != 0].tolist() == la[has != 0].tolist()
        assert t["close_max"].cpu().numpy().astype(np.uint16)[has != 0].tolist() == ll[has != 0].tolist()
        # the batch is not searched: what needs both ends refuses it, with the status it has today
        for call in (lambda: eng.classify(db, whole), lambda: eng.int_calls(db)):
            with pytest.raises(binding.PgError, match="not been searched"):
                call()
        # after a full search the close-only search clears the far half of the records: a download delivers no stale far list
        eng.pack_search_device(db)
        assert int(eng.download(db).far_off[-1]) > 100
        eng.close_search(db)
        _same_close(eng, db, res, batch.n)
        with pytest.raises(binding.PgError, match="not been searched"):
            eng.classify(db, whole)
    finally:
        eng.free_device_batch(db)


def test_close_search_pool_regrow(world, pg_env):
    """PG_TEST_TINY_POOL: the close launch overflows the pool, the pool is regrown and the launch repeated; same result, same tables"""
    eng = world["eng"]
    plan = dc.vote_edges(world["biol"])
    batch, first, strand = plan.batch()
    res, has, rc, la, ll = close_ends(eng, batch)
    want = hostlib.dd_tables_from_close(batch.seq, batch.seq_off, batch.anchor_strand, has, rc, la, ll, first, strand, 0, world["chroms"][0][1],
                                        world["mm"], 3, 400)
    pg_env.set("PG_TEST_TINY_POOL", "1")
    db = eng.upload(batch)
    try:
        eng.clear_launch_log()
        eng.close_search(db)
        modes = [r.mode for r in eng.launch_log() if r.kernel == inst.SEARCH]
        assert len(modes) >= 2 and set(modes) == {inst.CLOSE}, modes
        got = eng.dd_tables(db, first, strand, 0, 3, 400)
        assert got["members"].tobytes() == want["members"].tobytes() and got["cands"].tobytes() == want["cands"].tobytes() and got["cons"] == want["cons"]
        _same_close(eng, db, res, batch.n)
    finally:
        eng.free_device_batch(db)
