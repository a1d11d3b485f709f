"""-m gpu: the two far-end seams on reads the close end left SHORTENED (the derivation: tests/shortening_cases.py).

A far-only launch gets the reads in one of two forms, neither of which is the read first handed to the close end when that read
had characters outside ACGTN:
  (B) pg_far_end_batch(reads, close result): the post-state reads reverse-complemented back where rc_flag & 1 -- what
      pg_adapter::SearchFarEnds(reads, ..., close_result, hints) uploads -- with the close end's rc_flag 0, 1 or 2;
  (C) pg_far_end_batch_from_close(reads, UP_Close.back()): the post-state reads of the reads that kept a close end.
The trail family is the one no other test hands to a far-only launch: its junk was at the end only, two reverse complements
stripped it, so the read that comes back is CLEAN (not on the exact list: the ordinary kernels search it), carries rc_flag 2 and is
up to two characters shorter -- at L = 64, 128 and 192 one 64-base block fewer than the close launch packed.
The expectation is always the oracle on the ORIGINAL batch (it does the shortening itself), bit for bit."""
import numpy as np
import pytest

from pindel_amd import binding, hostio, synth
from tests import instantiations as I
from tests import shortening_cases as sc
from tests.parity import compare_result, oracle_points, points_per_read, run_oracle

pytestmark = pytest.mark.gpu

LENGTHS = (64, 100, 125, 128, 192)
FAMILIES = sc.SEAM_FAMILIES + ("mixed",)
REF_LEN = 600_000


@pytest.fixture(scope="module")
def ref():
    return [("chrS", synth.make_reference(REF_LEN, seed=31))]


@pytest.fixture(scope="module")
def engine(engine_factory, ref):
    eng = engine_factory()
    eng.load_reference(ref)
    return eng


@pytest.fixture(scope="module")
def engine_mri4(engine_factory, ref):
    eng = engine_factory(max_range_index=4)
    eng.load_reference(ref)
    return eng


_CASES = {}


def _case(ref, family, L, windows=False, **params):
    """(original batch, bd, bd_off, the oracle's result on it): built once per module"""
    key = (family, L, windows, tuple(sorted(params.items())))
    if key not in _CASES:
        batch = sc.seam_mixed(ref[0][1], L) if family == "mixed" else sc.seam_family(ref[0][1], family, L)
        bd = bd_off = None
        if windows:
            bd, bd_off = I.windows_for(batch, 3, len(ref[0][1]), 900 + L)
        _CASES[key] = (batch, bd, bd_off, run_oracle(params, ref, batch, bd=bd, bd_off=bd_off))
    return _CASES[key]


def _post_is_clean(batch, orc):
    off = batch.seq_off.astype(np.int64)
    return np.array([not sc.has_junk(orc["seq"][off[i]:off[i] + int(orc["len_out"][i])].tobytes()) for i in range(batch.n)])


def _not_vacuous(family, batch, orc):
    """the counts that make a pass mean something, on the oracle's result"""
    far = orc["far_cnt"][:batch.n] > 0
    flag = orc["rc_flag"][:batch.n]
    if family in ("trail", "trail2"):
        n2 = int(((flag == 2) & far & _post_is_clean(batch, orc)).sum())
        assert n2 >= 150, ("clean rc_flag 2 reads with a far end", n2)
    elif family in ("lead", "lead_of_trail"):
        assert int(((flag == 1) & far).sum()) >= 150
    elif family.startswith("inner"):
        assert int(((flag == 2) & far).sum()) >= 100
        # (an R at the last position is a NUL at the FRONT of the read after one reverse complement, the far end's first consumed
        # character: "CurrentBase == 'N' -> return", farend_searcher.cpp:60-66 -- a once-flipped read of that batch has no far end)
        if family != "inner_last":
            assert int(((flag == 1) & far).sum()) >= 15
    else:
        # 25 reads per family, two in three of them found at attempt 3: four families come back clean with a 2, one with a NUL
        # inside, two with a 1
        clean = _post_is_clean(batch, orc)
        junk = np.array([sc.has_junk(s) for s in sc.seqs_of(batch)])
        assert int(((flag == 2) & far & clean & junk).sum()) >= 40 and int(((flag == 1) & far & junk).sum()) >= 20
        assert int(((flag == 2) & far & ~clean).sum()) >= 8


def _far_kernel(eng, reads, generic, wide, params):
    """the one search kernel of a far-only launch over `reads`, against the plan's mirror of the dispatch rules"""
    recs = [tuple(r) for r in eng.launch_log() if tuple(r)[0] == I.SEARCH]
    assert len(recs) == 1, recs
    max_len = int(reads.lengths().max())
    small = I.small_ids(max_range_index=params.get("max_range_index", 2), max_cluster=3, force_wide=wide)
    ns = I.counter_slices(I.levels_of(max_len, **params))
    dflt = I.is_default(params) and not generic and ns <= 4 and small
    assert recs[0][:6] == I.search_rec(I.class_blocks(max_len, small), ns, 32 if small else 64, I.FAR, dflt, 0)[:6], recs
    return recs[0]


def _shortened_only(batch, bd, bd_off, orc, L):
    """the reads whose post-state is at most L long (a few reads of a junk-ended family are placed at attempt 0 and keep their
    junk: with them in the batch the far-only launch stays in the close launch's block class), with their share of the oracle's
    result and of the windows"""
    n = batch.n
    sel = np.nonzero(orc["len_out"][:n] <= L)[0]
    seqs = sc.seqs_of(batch)
    sub = sc.batch_of([seqs[i] for i in sel], batch.anchor_strand[sel], batch.anchor_pos[sel], batch.insert_size[sel], batch.chr_id[sel])
    off = batch.seq_off.astype(np.int64)
    o = {k: orc[k][:n][sel] for k in ("rc_flag", "len_out", "close_cnt", "far_cnt", "close_pts", "far_pts")}
    o["seq"] = np.concatenate([orc["seq"][off[i]:off[i + 1]] for i in sel])
    sbd = sbd_off = None
    if bd is not None:
        bo = bd_off.astype(np.int64)
        sbd = np.concatenate([bd[bo[i]:bo[i + 1]] for i in sel])
        sbd_off = np.concatenate([[0], np.cumsum(bo[sel + 1] - bo[sel])]).astype(np.uint64)
    return sub, sbd, sbd_off, o


def _run(eng, family, L, case, **cfg):
    """both entries on the whole batch and, where the junk made the longest original read cross a 64-base boundary (L = 64, 128,
    192: originals of 65 / 66, 129 / 130, 193 / 194 characters), on the reads that were shortened alone: that far-only launch packs one
    block fewer than the close launch did"""
    batch, bd, bd_off, orc = case
    _not_vacuous(family, batch, orc)
    _both_entries(eng, batch, bd, bd_off, orc, **cfg)
    if L % 64 == 0 and int(batch.lengths().max()) > L:
        sub, sbd, sbd_off, o = _shortened_only(batch, bd, bd_off, orc, L)
        assert sub.n >= batch.n * 3 // 4 and _blocks(sub) == L // 64 + 1
        _not_vacuous(family, sub, o)
        _both_entries(eng, sub, sbd, sbd_off, o, crossing=True, **cfg)


def _both_entries(eng, batch, bd, bd_off, orc, generic=False, wide=False, crossing=False, **params):
    n = batch.n
    close = eng.close_end_batch(batch)
    compare_result(close, orc, n, check_far=False)
    assert close.far_off[-1] == 0
    flags = close.rc_flag.copy()
    has, close_last, close_max = sc.close_back(close)
    close_off, close_runs = close.close_off.copy(), close.close_runs.copy()
    post = sc.post_state(batch, flags)
    np.testing.assert_array_equal(post.lengths(), orc["len_out"][:n])

    # (B) the close_result overload: post-state, un-flipped where flag & 1, with the flags of the close end
    up = sc.unflipped(post, flags)
    if crossing:
        assert _blocks(up) == _blocks(batch) - 1                                 # one block class below the close launch
    eng.clear_launch_log()
    both = eng.far_end_batch(up, close, bd, bd_off)
    _far_kernel(eng, up, generic, wide, params)
    compare_result(both, orc, n)
    np.testing.assert_array_equal(both.rc_flag, flags)                          # (a 2 stays a 2)
    np.testing.assert_array_equal(both.close_off, close_off)
    assert both.close_runs.tobytes() == close_runs.tobytes()

    # (C) from nothing but the kept post-state reads and UP_Close.back()
    kept = np.nonzero(has)[0]
    seqs = sc.seqs_of(post)
    kb = hostio.batch_from_lists([seqs[i] for i in kept], [bytes([c]) for c in batch.anchor_strand[kept]], batch.anchor_pos[kept],
                                 batch.insert_size[kept], batch.chr_id[kept])
    kbd = kbd_off = None
    if bd is not None:
        bo = bd_off.astype(np.int64)
        kbd = np.concatenate([bd[bo[i]:bo[i + 1]] for i in kept])
        kbd_off = np.concatenate([[0], np.cumsum(bo[kept + 1] - bo[kept])]).astype(np.uint64)
    eng.clear_launch_log()
    assert not crossing or _blocks(kb) == _blocks(batch) - 1
    far = eng.far_end_batch_from_close(kb, close_last[kept], close_max[kept], kbd, kbd_off)
    _far_kernel(eng, kb, generic, wide, params)
    assert far.n == len(kept) and far.close_off[-1] == 0 and len(far.close_runs) == 0 and not far.rc_flag.any()
    np.testing.assert_array_equal(points_per_read(far.far_off, far.far_runs), orc["far_cnt"][kept], err_msg="UP_Far points per read")
    g_far = binding.expand_runs(far.far_runs)
    o_far = np.concatenate([oracle_points(orc, int(i), "far") for i in kept])
    if g_far.tobytes() != o_far.tobytes():
        for k, i in enumerate(kept):
            a, b = int(far.far_off[k]), int(far.far_off[k + 1])
            g = binding.expand_runs(far.far_runs[a:b])
            o = oracle_points(orc, int(i), "far")
            assert g.tobytes() == o.tobytes(), (f"read {int(i)} (rc_flag {int(flags[i])}) UP_Far from close", g[:1], o[:1])
        raise AssertionError("UP_Far of the far end from close")


def _blocks(batch):
    """64-base blocks of the longest read: the launch's kernel class"""
    return (int(batch.lengths().max()) + 63) // 64


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("family", FAMILIES)
def test_far_seams_on_post_state_reads(engine, ref, family, L):
    _run(engine, family, L, _case(ref, family, L))


@pytest.mark.parametrize("L", (64, 128))
@pytest.mark.parametrize("family", ("trail2", "mixed"))
@pytest.mark.parametrize("switch", ("PG_GENERIC_KERNELS", "PG_FORCE_WIDE_CELLS"))
def test_far_seams_under_a_kernel_switch(engine, ref, pg_env, switch, family, L):
    pg_env.set(switch, "1")
    _run(engine, family, L, _case(ref, family, L), generic=switch == "PG_GENERIC_KERNELS", wide=switch == "PG_FORCE_WIDE_CELLS")


@pytest.mark.parametrize("L", (64, 128))
@pytest.mark.parametrize("family", ("trail2", "mixed"))
def test_far_seams_with_max_range_index_4(engine_mri4, ref, family, L):
    _run(engine_mri4, family, L, _case(ref, family, L, max_range_index=4), max_range_index=4)


@pytest.mark.parametrize("L", (64, 128))
@pytest.mark.parametrize("family", ("trail2", "mixed"))
def test_far_seams_with_window_hints(engine, ref, family, L):
    _run(engine, family, L, _case(ref, family, L, windows=True))
