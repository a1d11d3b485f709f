"""-m gpu: the fixed-length kernels (pg_search_fixed_kernel<NB, NS, LEN>: the read length and every record field that follows from
it are constants of the kernel, PgFixedLen in pg_device.h).  A batch takes one only if all its reads have one of the built lengths,
the parameters are Pindel's defaults, the ids 32-bit and the launch the fused one; Engine.last_fixed_len() says which kernel the last
search launch was.  Every batch here is compared bit for bit with the oracle (tests/parity.py), on the three entries of the ABI that
launch the fused kernel: pack_search_device (the kernel packs its own records), search_device (records packed at upload) and
search_batch (the host path)."""
import hashlib

import numpy as np
import pytest

from pindel_amd import synth
from pindel_amd.binding import WINDOW_DTYPE
from pindel_amd.hostio import SPACER
from tests import shortening_cases as sc
from tests.parity import compare_result, run_oracle

pytestmark = pytest.mark.gpu

BUILT = [100, 101, 150, 151]          # PG_FIXED_LEN_ROWS (pg_device.h)
BIOL = 700_000
ISZ = 500


@pytest.fixture(scope="module")
def ref():
    return [("chrF", synth.make_reference(BIOL, seed=67))]


def _end_reads(ref_seq, L, n, seed):
    """reads anchored within one insert size of either end of the chromosome; every second one carries the sequence next to its
    anchor, on the side and in the orientation its close end is looked for, and a piece from 1 kb further inside"""
    base = synth.make_reads(ref_seq, n, read_len=L, seed=seed)
    rng = np.random.default_rng(seed)
    at_start = np.arange(n) % 4 < 2
    base.anchor_pos[:] = np.where(at_start, rng.integers(0, ISZ, n), BIOL - rng.integers(0, ISZ, n)).astype(np.int32)
    refb = np.frombuffer(ref_seq, dtype=np.uint8)
    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b"ACGTN")] = list(b"TGCAN")
    off = base.seq_off.astype(np.int64)
    a = (6 * L) // 10
    for i in range(0, n, 2):
        plus = base.anchor_strand[i] == ord("+")
        apos = int(base.anchor_pos[i]) + SPACER
        p = apos + int(rng.integers(0, 300)) if plus else apos - int(rng.integers(0, 300)) - L
        inward = 1000 if at_start[i] else -1000
        if plus:      # the close end is the read's left part, the far end follows
            s = np.concatenate([refb[p:p + a], refb[p + inward:p + inward + (L - a)]])
            s = comp[s[::-1]]
        else:         # the close end is the read's right part
            s = np.concatenate([refb[p + inward:p + inward + (L - a)], refb[p + L - a:p + L]])
        base.seq[off[i]:off[i] + L] = s
    return base


_cache = {}


def _batch(ref, L, kind):
    """(batch, oracle result) of a named input, built once"""
    key = (L, kind)
    if key not in _cache:
        r = ref[0][1]
        if kind == "std":
            b = synth.make_reads(r, 20_000, read_len=L, seed=700 + L)
        elif kind == "noisy":
            b = synth.make_reads(r, 20_000, read_len=L, seed=800 + L, error_rate=0.05, n_rate=0.02)
        elif kind == "ends":
            b = _end_reads(r, L, 2_000, seed=900 + L)
        elif kind == "small":
            b = synth.make_reads(r, 3_000, read_len=L, seed=1000 + L)
        else:
            raise KeyError(kind)
        _cache[key] = (b, run_oracle({}, ref, b))
    return _cache[key]


def _three_entries(eng, batch, orc, want_len, bd=None, bd_off=None, in_place=True):
    db = eng.upload(batch)
    try:
        if bd is not None:
            eng.set_windows(db, bd, bd_off)
        eng.scribble_records(db)
        eng.pack_search_device(db)
        assert eng.last_step_in_place() == in_place
        assert eng.last_fixed_len() == want_len
        compare_result(eng.download(db), orc, batch.n)
        eng.repack(db)
        eng.search_device(db)
        assert eng.last_fixed_len() == want_len
        compare_result(eng.download(db), orc, batch.n)
    finally:
        eng.free_device_batch(db)
    if bd is None:
        res = eng.search_batch(batch)
        assert eng.last_fixed_len() == want_len
        compare_result(res, orc, batch.n)


@pytest.mark.parametrize("kind", ["std", "noisy", "ends"])
@pytest.mark.parametrize("L", BUILT)
def test_built_lengths_against_the_oracle(engine_factory, ref, L, kind):
    eng = engine_factory()
    eng.load_reference(ref)
    batch, orc = _batch(ref, L, kind)
    assert (orc["close_cnt"] > 0).sum() > batch.n // 10 and (orc["far_cnt"] > 0).sum() > batch.n // 20
    _three_entries(eng, batch, orc, L)


def test_a_context_that_ran_nothing_reports_zero():
    from pindel_amd import binding
    eng = binding.Engine()
    try:
        assert eng.last_fixed_len() == 0
    finally:
        eng.close()


@pytest.mark.parametrize("L", BUILT)
def test_host_path_in_several_chunks(engine_factory, ref, pg_env, L):
    eng = engine_factory()
    eng.load_reference(ref)
    batch, orc = _batch(ref, L, "std")
    pg_env.set("PG_HOST_CHUNK", "3000")
    res = eng.search_batch(batch)
    assert eng.last_fixed_len() == L
    compare_result(res, orc, batch.n)


@pytest.mark.parametrize("L", sorted({L + d for L in BUILT for d in (-1, 1)} - set(BUILT)))
def test_neighbouring_lengths_run_the_other_kernels(engine_factory, ref, L):
    """uniform batches of the lengths next to the built ones (those that are not built themselves)"""
    eng = engine_factory()
    eng.load_reference(ref)
    batch, orc = _batch(ref, L, "small")
    _three_entries(eng, batch, orc, 0)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("L", BUILT)
def test_one_read_of_another_length(engine_factory, ref, L, where):
    eng = engine_factory()
    eng.load_reference(ref)
    same = _batch(ref, L, "small")[0]
    other = _batch(ref, L - 1, "small")[0]
    n = 2_000
    k = {"first": 0, "middle": n // 2, "last": n - 1}[where]
    batch = sc.concat([same.slice(0, k), other.slice(k, k + 1), same.slice(k + 1, n)])
    lens = batch.lengths()
    assert batch.n == n and lens[k] == L - 1 and (np.delete(lens, k) == L).all()
    _three_entries(eng, batch, run_oracle({}, ref, batch), 0)


@pytest.mark.parametrize("kw", [dict(min_close=9), dict(seq_error_rate=0.05)], ids=["min_close-9", "other-length-tables"])
@pytest.mark.parametrize("L", BUILT)
def test_other_parameters_run_the_other_kernels(engine_factory, ref, L, kw):
    """one parameter off the defaults; and parameters the default-parameter kernels do take (-e changes no constant of theirs), whose
    length tables are not the baked ones"""
    eng = engine_factory(**kw)
    eng.load_reference(ref)
    batch = _batch(ref, L, "small")[0]
    _three_entries(eng, batch, run_oracle(kw, ref, batch), 0)


@pytest.mark.parametrize("L", BUILT)
def test_generic_kernels_forced(engine_factory, ref, pg_env, L):
    pg_env.set("PG_GENERIC_KERNELS", "1")
    eng = engine_factory()
    eng.load_reference(ref)
    batch, orc = _batch(ref, L, "small")
    _three_entries(eng, batch, orc, 0)


@pytest.mark.parametrize("L", BUILT)
def test_more_than_127_windows_in_a_cluster(engine_factory, ref, L):
    """64-bit candidate ids: no fixed-length kernel.  The same batch with 127 windows keeps 32-bit ids and takes one."""
    eng = engine_factory()
    eng.load_reference(ref)
    batch = _batch(ref, L, "small")[0].slice(0, 600)
    rng = np.random.default_rng(L)
    for per, want in ((128, 0), (127, L)):
        cnt = np.ones(batch.n, dtype=np.int64)
        cnt[batch.n // 3] = per
        bd_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
        bd = np.zeros(int(bd_off[-1]), dtype=WINDOW_DTYPE)
        st = rng.integers(1000, BIOL - 30_000, len(bd))
        bd["start"] = st
        bd["end"] = st + rng.integers(50, 400, len(bd))
        first = bd_off[:-1].astype(np.int64)          # every read's first window: its own far-end neighbourhood
        bd["start"][first] = np.clip(batch.anchor_pos.astype(np.int64) - 12_000, 0, BIOL - 24_000)
        bd["end"][first] = bd["start"][first] + 24_000
        orc = run_oracle({}, ref, batch, bd=bd, bd_off=bd_off)
        assert (orc["far_cnt"] > 0).sum() > 30
        # (64-bit ids: the kernels of 129 .. 192 bases have four blocks per read, the planes three -- a pack launch of its own)
        _three_entries(eng, batch, orc, want, bd=bd, bd_off=bd_off, in_place=per == 127 or L <= 128)


@pytest.mark.parametrize("L", BUILT)
def test_reads_on_the_exact_list(engine_factory, ref, L):
    """uniform length, one read in twelve with a character outside ACGTN: the fixed-length kernel searches all of them with the
    length of the record, the exact kernel behind it overrides the listed ones with the reference's shortening (rc_flag 2 among them)"""
    eng = engine_factory()
    eng.load_reference(ref)
    r = ref[0][1]
    plain = _batch(ref, L, "small")[0]
    junk = [sc.lead_case(sc.clean_reads(r, 60, L - 1, seed=41), b"R"), sc.lead_case(sc.clean_reads(r, 60, L - 2, seed=42), b"RY"),
            sc.trail_case(sc.moved(sc.clean_reads(r, 60, L - 2, seed=43)), b"RK"), sc.trail_case(sc.moved(sc.clean_reads(r, 60, L - 1, seed=44)), b"r"),
            sc.inner_case(sc.moved(sc.clean_reads(r, 60, L, seed=45)), L // 2), sc.inner_case(sc.clean_reads(r, 60, L, seed=46), 0),
            sc.inner_case(sc.clean_reads(r, 60, L, seed=47), L - 1)]
    j = sc.concat(junk)
    parts = []
    for k in range(min(j.n, plain.n // 11)):
        parts += [plain.slice(11 * k, 11 * k + 11), j.slice(k, k + 1)]
    batch = sc.concat(parts)
    assert (batch.lengths() == L).all() and batch.n >= 12 * 200
    orc = run_oracle({}, ref, batch)
    assert (orc["rc_flag"] == 2).sum() > 20 and (orc["rc_flag"] == 1).sum() > 100
    assert (orc["len_out"] < L).sum() > 50             # reads the reference shortened
    _three_entries(eng, batch, orc, L)


def _digest(res):
    h = hashlib.sha256()
    for a in (res.close_off, res.far_off, res.rc_flag, res.close_runs, res.far_runs):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("L", BUILT)
def test_fixed_against_generic_in_one_process(engine_factory, ref, pg_env, L):
    eng = engine_factory()
    eng.load_reference(ref)
    batch = synth.make_reads(ref[0][1], 50_000, read_len=L, seed=1100 + L)
    db = eng.upload(batch)
    try:
        got = {}
        for off in (False, True, False):
            if off:
                pg_env.set("PG_NO_FIXED_LEN", "1")
            else:
                pg_env.unset("PG_NO_FIXED_LEN")
            eng.scribble_records(db)
            eng.pack_search_device(db)
            assert eng.last_fixed_len() == (0 if off else L)
            got.setdefault(off, []).append(_digest(eng.download(db)))
            eng.search_device(db)
            assert eng.last_fixed_len() == (0 if off else L)
            got[off].append(_digest(eng.download(db)))
        assert len(set(got[False]) | set(got[True])) == 1, got
    finally:
        eng.free_device_batch(db)


@pytest.mark.parametrize("n", [7, 1])
@pytest.mark.parametrize("L", BUILT)
def test_single_claims(engine_factory, ref, L, n):
    """one short claim (its first read is the one that must not touch its successor's record when n = 1)"""
    eng = engine_factory()
    eng.load_reference(ref)
    batch, orc = _batch(ref, L, "small")
    has = np.nonzero((orc["close_cnt"] > 0) & (orc["far_cnt"] > 0))[0]
    lo = int(has[5])
    sub = batch.slice(lo, lo + n)
    _three_entries(eng, sub, run_oracle({}, ref, sub), L)
