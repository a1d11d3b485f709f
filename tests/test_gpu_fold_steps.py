"""-m gpu: the fold's per-candidate step (pindel_amd/csrc/pg_fold_step.h) where its short form differs from the long one: the tier A
walk (full iterations without the validity test, a tail, the ring lists of the fused far-end pass), the Hamming verdict carried as
inequality bits, and the AccB state of the rounds >= 1.

The reads are planted on a reference built for the test, one read per 1600-base slot.  A DECOY of a read is a copy of the first 14
bases one end's growth consumes, followed by 7 bases that all differ from the read's next ones: it passes the seed filter as a
level-0 candidate, ties with the true candidate up to 14 bases and is dead before bps + 16, so it is a tier A entry.
  tier A pass sizes   per close-end read k decoys in the window of attempt 0 (R = 0), k = 0 .. 9, both anchor strands
  far-end rings       decoys per ring of the far end's nested ranges (64, 256, 1024 either side of the close end's last point):
                      (n0, n1, n2) = (0, 0, k) and (0, k, 0) for k = 0 .. 9, (k, 0, 0) for k = 0 .. 5 (what fits 128 bases beside the
                      read's own close part), (1, 2, 5), (3, 1, 0); the true far end lies in ring 2, so every ring is evaluated
  Hamming verdict     a read that lies on the reference in one piece with thr - 1 substitutions (CheckMismatches' whole-read count
                      fails on a clean window: no close end) next to its twin with thr (a close end); the same at the far end (a copy
                      of the read's first 30 bases near the anchor, the read's origin in ring 2).  These winners are long-lived: a
                      candidate that dies before bps + 16 has at least T > thr mismatches, so its count cannot fail.
  rounds >= 1         the sweep of tests/test_gpu_fold_masks.py (last points either side of bps + 64, with 150 bases of bps + 128, one
                      substitution inside and just outside CheckMismatches' window), on the plain reference
Read lengths 100, 101 (fixed-length kernels, NB = 2), 150 (NB = 3, passes of 32), 99 (default-parameter kernel) and 100 with -m 5
(generic kernels: the long form next to the short one).  Every batch goes through pack_search_device and through the two far-end seams,
bit for bit against the oracle, and the launch log must name the expected kernel.  What the batches cover is asserted on the inputs
(brute-force counts of the decoys over the windows) and on the oracle's output alone, before any GPU result is looked at; at most 5 %
of the planted reads may miss their class by chance."""
import numpy as np
import pytest

from pindel_amd import synth
from pindel_amd.hostio import SPACER
from tests import shortening_cases as sc
from tests.parity import compare_result, run_oracle
from tests.test_gpu_far_seam_states import _both_entries
from tests.test_gpu_fold_masks import BPS, _fused_kernel, _planted

pytestmark = pytest.mark.gpu

BIOL = 300_000
ISZ = 500
W = 1600                           # a read's slot
BP = 700                           # the break, in slot coordinates of the '+' frame
SLACK = 60                         # anchor to the read's first base
KM = 14                            # a decoy's matching bases
DV = 7                             # ... and its divergent ones
CONFIGS = [("L100", 100, {}, 100), ("L101", 101, {}, 101), ("L150", 150, {}, 150), ("L99-default", 99, {}, 0),
           ("L100-m5", 100, dict(min_perfect_match=5), 0)]
RING_PATTERNS = ([(0, 0, k) for k in range(10)] + [(k, 0, 0) for k in range(6)] + [(0, k, 0) for k in range(10)] +
                 [(1, 2, 5), (3, 1, 0)])
RING0_AT = [22, 43, -20, -41, -62]                 # a decoy's seed base relative to BP: beside the break and beside the close part
SPANS = (64, 256, 1024)

_COMP = np.zeros(256, dtype=np.uint8)
_COMP[list(b"ACGTN")] = list(b"TGCAN")
_NXT = np.zeros(256, dtype=np.uint8)
_NXT[list(b"ACGT")] = list(b"CGTA")


def _rc(a):
    return _COMP[a[::-1]]


def _thr(L):
    """CheckMismatches passes from this whole-read count on: (float)n >= (float)(len * 0.02)"""
    n = 0
    while np.float32(n) < np.float32(L * 0.02):
        n += 1
    return n


def _slot(slot, L, cls, arg):
    """plants one read of class `cls` into `slot` (the '+' frame: the close end grows to the right from the read's first base, the
    far end to the left from its last); returns (cur, anchor position in the slot, what the coverage check expects)"""
    if cls == "ham_close":
        cur = slot[BP - 40:BP - 40 + L].copy()
        for i in range(arg):
            cur[45 + 12 * i] = _NXT[cur[45 + 12 * i]]
        return cur, BP - 40 - SLACK, dict(cls=cls, subs=arg)
    if cls == "ham_far":
        cur = slot[BP + 500:BP + 500 + L].copy()
        slot[BP - 30:BP] = cur[:30]
        slot[BP:BP + 8] = _NXT[cur[30:38]]
        for i in range(arg):
            cur[45 + 12 * i] = _NXT[cur[45 + 12 * i]]
        return cur, BP - 30 - SLACK, dict(cls=cls, subs=arg, c=30)
    c, d = (40, 450) if cls == "tier_a" else (16, 500)
    if slot[BP + d] == slot[BP]:                              # neither part extends over the break on matching bases
        slot[BP] = _NXT[slot[BP]]
    if slot[BP - 1] == slot[BP + d - 1]:
        slot[BP + d - 1] = _NXT[slot[BP + d - 1]]
    cur = np.concatenate([slot[BP - c:BP], slot[BP + d:BP + d + L - c]])
    if cls == "tier_a":
        for j in range(arg):                                 # forward decoys inside the window of attempt 0
            p = BP + 40 + 24 * j
            slot[p:p + KM] = cur[:KM]
            slot[p + KM:p + KM + DV] = _NXT[cur[KM:KM + DV]]
        return cur, BP - c - SLACK, dict(cls=cls, k=arg, c=c)
    at = [RING0_AT[j] for j in range(arg[0])] + [70 + 21 * j for j in range(arg[1])] + [262 + 21 * j for j in range(arg[2])]
    for o in at:                                             # backward decoys: the seed base at BP + o
        p = BP + o
        slot[p - KM + 1:p + 1] = cur[L - KM:]
        slot[p - KM + 1 - DV:p - KM + 1] = _NXT[cur[L - KM - DV:L - KM]]
    return cur, BP - c - SLACK, dict(cls=cls, rings=arg, c=c)


def _build(L, seed):
    """(reference, batch, what each read was planted as)"""
    refb = np.frombuffer(synth.make_reference(BIOL, seed=seed), dtype=np.uint8).copy()
    thr = _thr(L)
    plan = [("tier_a", k) for k in range(10)] + [("rings", p) for p in RING_PATTERNS]
    plan += [(h, j) for h in ("ham_close", "ham_far") for j in (thr - 1, thr)] * 3
    seqs, strand, pos, want = [], [], [], []
    s0 = SPACER + 2000
    for plus in (True, False):
        for cls, arg in plan:
            assert s0 + W < SPACER + BIOL - 2000, "the reference is too short for the plan"
            slot = refb[s0:s0 + W].copy()
            cur, apos, w = _slot(slot, L, cls, arg)
            # the '-' frame is the mirror image: the slot reverse-complemented, the same read, the window ending where it began
            refb[s0:s0 + W] = slot if plus else _rc(slot)
            seqs.append(_rc(cur).tobytes())
            strand.append(ord("+") if plus else ord("-"))
            pos.append(s0 + (apos if plus else W - apos) - SPACER)
            want.append(w)
            s0 += W
    return refb.tobytes(), sc.batch_of(seqs, strand, pos, [ISZ] * len(seqs)), want


def _hits(refb, km, forward, lo, hi):
    """positions p of [lo, hi) where a growth that consumes `km` first finds all of it: forward ref[p : p + 14], backward
    ref[p - 13 : p + 1] read down from p"""
    if hi <= lo:
        return 0
    if forward:
        v = np.lib.stride_tricks.sliding_window_view(refb[lo:hi + KM - 1], KM)
    else:
        v = np.lib.stride_tricks.sliding_window_view(refb[lo - KM + 1:hi], KM)
    return int((v == km).all(axis=1).sum())


def _covered(ref_seq, batch, want, orc, L):
    """on the inputs and the oracle's output alone"""
    refb = np.frombuffer(ref_seq, dtype=np.uint8)
    seqs = sc.seqs_of(batch)
    missed, sizes, rings_seen, ham = 0, set(), set(), {}
    for i, w in enumerate(want):
        plus = batch.anchor_strand[i] == ord("+")
        seq = np.frombuffer(seqs[i], dtype=np.uint8)
        cur = _rc(seq) if plus else seq                     # what attempt 0 of the close end grows, and from which end
        a = int(batch.anchor_pos[i]) + SPACER
        lo, hi = (a, a + ISZ) if plus else (a - ISZ, a)
        ccnt, fcnt = int(orc["close_cnt"][i]), int(orc["far_cnt"][i])
        cmax = int(orc["close_pts"][i][:ccnt]["length"].max()) if ccnt else 0
        fmax = int(orc["far_pts"][i][:fcnt]["length"].max()) if fcnt else 0
        if w["cls"] == "ham_close":                         # (attempt 0 had a point: the read did not go on to the retries)
            ham.setdefault((w["cls"], w["subs"]), []).append(ccnt > 0 and not orc["rc_flag"][i] and cmax >= 44)
            continue
        if w["cls"] == "ham_far":
            if cmax < w["c"] or orc["rc_flag"][i]:
                missed += 1
            else:
                ham.setdefault((w["cls"], w["subs"]), []).append(fcnt > 0)
            continue
        # (the close end stops at the break: the far end's rings are centred on it; the far end may run on past it on mismatches)
        if orc["rc_flag"][i] or cmax != w["c"] or fmax < L - w["c"]:
            missed += 1
            continue
        if w["cls"] == "tier_a":
            n = _hits(refb, cur[:KM] if plus else cur[-KM:], plus, lo, hi)
            assert n == w["k"] + 1, ("decoys in the window of attempt 0", i, n, w)
            sizes.add(w["k"])
        else:
            # the far end grows the other end of the read, on the other strand's terms: kind B from the last base down for a '+'
            # anchor, kind F from the first base up for a '-' one
            centre = int(orc["close_pts"][i][ccnt - 1]["abs_loc"])
            km = cur[-KM:] if plus else cur[:KM]
            inner, got = 0, []
            for s in SPANS:
                n = _hits(refb, km, not plus, centre - s, centre + s)
                got.append(n - inner)
                inner = n
            assert tuple(got) == (w["rings"][0], w["rings"][1], w["rings"][2] + 1), ("decoys per ring", i, got, w)
            rings_seen.add(w["rings"])
    assert missed * 20 <= len(want), ("planted reads outside their class", missed, len(want))
    assert sizes == set(range(10)), sizes
    assert rings_seen == set(RING_PATTERNS), set(RING_PATTERNS) - rings_seen
    thr = _thr(L)
    for h in ("ham_close", "ham_far"):
        assert ham[(h, thr - 1)] and not any(ham[(h, thr - 1)]), (h, "a point although the whole-read count fails", ham)
        assert ham[(h, thr)] and all(ham[(h, thr)]), (h, "no point at the threshold", ham)


def _rounds_covered(orc, n, L):
    last = {end: max(int(orc[end + "_pts"][i][:int(orc[end + "_cnt"][i])]["length"].max()) if orc[end + "_cnt"][i] else 0
                     for i in range(n)) for end in ("close", "far")}
    for end in ("close", "far"):
        assert last[end] > BPS[end] + (128 if L >= 150 else 64), (end, last)


_CASES = {}


def _case(cid):
    """the two batches of a configuration with their references and the oracle's results, built and checked for coverage once"""
    if cid not in _CASES:
        _, L, params, _ = next(c for c in CONFIGS if c[0] == cid)
        ref_seq, batch, want = _build(L, seed=411 + L)
        ref = [("chrK", ref_seq)]
        orc = run_oracle(params, ref, batch)
        if not params:                                      # (the classes are defined for Pindel's default parameters)
            _covered(ref_seq, batch, want, orc, L)
        plain = [("chrK", synth.make_reference(BIOL, seed=97))]
        sweep, _ = _planted(plain[0][1], L, seed=5000 + 7 * L + len(params))
        sweep_orc = run_oracle(params, plain, sweep)
        _rounds_covered(sweep_orc, sweep.n, L)
        _CASES[cid] = ((ref, batch, orc), (plain, sweep, sweep_orc))
    return _CASES[cid]


@pytest.mark.parametrize("cid", [c[0] for c in CONFIGS])
def test_fold_steps(engine_factory, cid):
    _, L, params, fixed = next(c for c in CONFIGS if c[0] == cid)
    for ref, batch, orc in _case(cid):                      # (asserts the coverage)
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
