"""-m gpu: the fold's per-lane masks (pindel_amd/csrc/pg_lane_masks.h) at the places where they change shape.

Tier B folds a long-lived candidate in rounds of 64 lengths: round r holds L = bps + 64 r + lane, bps = 8 at the close end and 10 at
the far end, and CheckMismatches' window of Min_Perfect_Match_Around_BP bases ends at L.  The planted split reads here sweep the
matched length of the close end and of the far end over every length of [bps + 60, bps + 68] (the first round boundary; for 150 / 151
bases also [bps + 124, bps + 132], the second), on both anchor strands, and every case has four twins with one substitution 1, 2, 3 and
4 bases before the break: inside the window and just outside it, windows that straddle a 64-base block among them.

Read lengths 100, 101 (fixed-length kernels, NB = 2), 150, 151 (NB = 3), 99 (default-parameter kernel, not a fixed-length one) and
100 with -m 5 (generic kernels).  Every batch goes through pack_search_device and through the two far-end seams (far_end_batch,
far_end_batch_from_close), bit for bit against the oracle, and the launch log must name the expected kernel.  What the batches
cover is asserted on the oracle's output alone, before any GPU result is looked at."""
import numpy as np
import pytest

from pindel_amd import synth
from pindel_amd.hostio import SPACER
from tests import instantiations as I
from tests import shortening_cases as sc
from tests.parity import compare_result, run_oracle
from tests.test_gpu_far_seam_states import _both_entries

pytestmark = pytest.mark.gpu

BIOL = 300_000
ISZ = 500
BPS = {"close": 8, "far": 10}      # the first evaluated length: -H / g_MinClose, farend_searcher.cpp:90
REPS = 3                           # geometries per (sweep, length, strand)
# (id, read length, parameters, the fixed-length kernel of the fused launch or 0)
CONFIGS = [("L100", 100, {}, 100), ("L101", 101, {}, 101), ("L150", 150, {}, 150), ("L151", 151, {}, 151),
           ("L99-default", 99, {}, 0), ("L100-m5", 100, dict(min_perfect_match=5), 0)]


def swept(L, end):
    """the matched lengths of one end that the reads of length L sweep: four either side of every round boundary inside the read"""
    return [BPS[end] + 64 * r + d for r in range(1, 3 if L >= 150 else 2) for d in range(-4, 5)]


@pytest.fixture(scope="module")
def ref():
    return [("chrK", synth.make_reference(BIOL, seed=97))]


def _planted(ref_seq, L, seed):
    """(batch, twin_of): deletion reads whose close part is `c` bases and whose far part is the other L - c.  Per swept length of
    either end, strand and repetition one clean read and its four twins; twin_of[i] = the clean read of read i (itself for a
    clean one).  The deletion is placed where neither part can extend over the break by chance on matching bases."""
    refb = np.frombuffer(ref_seq, dtype=np.uint8)
    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b"ACGTN")] = list(b"TGCAN")
    nxt = np.zeros(256, dtype=np.uint8)
    nxt[list(b"ACGT")] = list(b"CGTA")
    rng = np.random.default_rng(seed)
    seqs, strand, pos, twin_of = [], [], [], []
    for end in ("close", "far"):
        for m in swept(L, end):
            c = m if end == "close" else L - m           # the close part's length
            if not BPS["close"] <= c <= L - BPS["far"]:
                continue
            for plus in (True, False):
                for rep in range(REPS):
                    sp = c if plus else L - c                # the left part's length: the close end is the part next to the anchor
                    bp = int(rng.integers(SPACER + 4000, SPACER + BIOL - 8000))
                    d = int(rng.integers(*[(40, 100), (150, 400), (600, 1800)][rep % 3]))
                    while refb[bp + d] == refb[bp] or refb[bp - 1] == refb[bp + d - 1]:
                        d += 1
                    true = np.concatenate([refb[bp - sp:bp], refb[bp + d:bp + d + L - sp]])
                    slack = int(rng.integers(0, ISZ - L - 20))
                    apos = (bp - sp - slack if plus else bp + d + (L - sp) + slack) - SPACER
                    clean = len(seqs)
                    for k in range(5):                       # k bases before the break, seen from the swept end (0: none)
                        s = true.copy()
                        if k:
                            left_side = (end == "close") == plus
                            at = sp - k if left_side else sp + k - 1
                            s[at] = nxt[s[at]]
                        seqs.append((comp[s[::-1]] if plus else s).tobytes())      # (the mate of a '+' anchor is read from the reverse strand)
                        strand.append(ord("+") if plus else ord("-"))
                        pos.append(apos)
                        twin_of.append(clean)
    return sc.batch_of(seqs, strand, pos, [ISZ] * len(seqs)), np.array(twin_of)


_CASES = {}


def _case(ref, cid):
    """(batch, the oracle's result), built and checked for coverage once"""
    if cid not in _CASES:
        _, L, params, _ = next(c for c in CONFIGS if c[0] == cid)
        batch, twin_of = _planted(ref[0][1], L, seed=3000 + 7 * L + len(params))
        orc = run_oracle(params, ref, batch)
        _covered(batch, twin_of, orc, L)
        _CASES[cid] = (batch, orc)
    return _CASES[cid]


def _last_lengths(orc, i, which):
    cnt = int(orc[which + "_cnt"][i])
    return int(orc[which + "_pts"][i][:cnt]["length"].max()) if cnt else 0


def _covered(batch, twin_of, orc, L):
    """on the oracle's output alone: every swept length is the last point of a close end and of a far end at least once, and
    substitution twins differ from their clean cases"""
    n = batch.n
    for end in ("close", "far"):
        seen = {_last_lengths(orc, i, end) for i in range(n) if twin_of[i] == i}
        missing = [m for m in swept(L, end) if m not in seen]
        assert not missing, (f"no {end} end of the clean reads ends at", missing)
    differ = 0
    for i in np.nonzero(twin_of != np.arange(n))[0]:
        j = int(twin_of[i])
        differ += not (sc.same_points(orc, int(i), orc, j))
    assert differ >= n // 10, ("substitution twins that differ from their clean case", differ, n)


def _fused_kernel(eng, L, params, fixed):
    assert eng.last_fixed_len() == fixed
    recs = [tuple(r) for r in eng.launch_log() if tuple(r)[0] == I.SEARCH]
    assert len(recs) == 1, recs
    ns = I.counter_slices(I.levels_of(L, **params))
    want = I.search_rec(I.class_blocks(L, True), ns, 32, I.BOTH, I.is_default(params), 1)
    assert recs[0] == want, (recs, want)


@pytest.mark.parametrize("cid", [c[0] for c in CONFIGS])
def test_round_boundaries_and_the_window(engine_factory, ref, cid):
    _, L, params, fixed = next(c for c in CONFIGS if c[0] == cid)
    batch, orc = _case(ref, cid)                      # (asserts the coverage)
    eng = engine_factory(**params)
    eng.load_reference(ref)
    db = eng.upload(batch)
    try:
        eng.scribble_records(db)
        eng.clear_launch_log()
        eng.pack_search_device(db)
        _fused_kernel(eng, L, params, fixed)
        compare_result(eng.download(db), orc, batch.n)
    finally:
        eng.free_device_batch(db)
    _both_entries(eng, batch, None, None, orc, **params)
