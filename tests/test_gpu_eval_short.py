"""-m gpu: the evaluation of a search state and the emission of its runs (evaluate, count_kept, emit_runs; pg_kernels.hip) at their
edges, bit for bit against the oracle.  The fixed-length kernels and five default-parameter kernels run the short form of the three
functions (pg_short_eval, pg_eval_masks.h), every other kernel the long form: every case goes through

    fixed     a batch whose reads all have L bases, L = 100, 101 (two rounds of 64 lengths), 150, 151 (three): the fixed-length kernel
              -- the short form, the read's length a literal
    default   the same batch and one read of L - 2 bases: the fused default-parameter kernel for any length, <2 or 3, 3, BOTH> -- both
              stay on the LONG form (they spill more on the short one): a control, like the next
    generic   the first batch with PG_GENERIC_KERNELS=1: the generic kernel, long form
    far-only  the first batch through the split entries (close_end_batch, then far_end_batch and far_end_batch_from_close): the
              far-only launch of the 150- and 151-base batches runs <3, 3, FAR, defaults> -- the short form with the read's length a
              run-time value, the scalar mask of the valid lanes no literal; that of the 100- and 101-base batches <2, 3, FAR,
              defaults>, long form.  The close-end launch in front of it is a long-form kernel at every length.

and the launch log says which kernel ran.

The reads are planted on a small synthetic reference, one slot of 2 500 bases per geometry, mismatches placed by position.  "Index"
below is the index of a base in the order an end consumes the read (the close end from the base next to the anchor, the far end from
the other end of the read); the length L' consumes the indices below L'.  A "twin" is a second copy of the consumed bases planted
inside the same search window, with substitutions of its own, so that two candidates tie at some lengths and part at others.
g_maxMismatch is 2 up to length 32, 3 up to 74, 4 up to 125, 5 beyond (default rates); a candidate past it ends the evaluation
(abort), a substitution inside the last three consumed bases fails CheckMismatches, a point needs every other candidate two levels
above the lowest.

The cases (per length, both anchor strands, GEOMS geometries x REPS anchor positions each):
    random        random reads: no candidate or none that lives
    abort0        substitutions at indices 1, 3, 5: level 3 at the first evaluated length 8 (lane 0 of round 0) -- no point
    only_bps      substitutions at 8, 11, 14: one point, at exactly L' = bps = 8, then CheckMismatches fails until the abort at 15
    only_last     the whole read lies at one place (four substitutions, see NOISE), and so does a twin but for indices len - 3 and
                  len - 2: tied up to len - 3, one level apart at len - 2, two at len - 1 -- one point, at exactly L' = len - 1 (the
                  last lane of the last round)
    boundary      a clean close end of 80 bases: points at 71 (lane 63 of round 0) and 72 (lane 0 of round 1), same candidate and
                  level -- two runs on the device, since a run never spans two rounds
    first1/2      substitutions at index 1 / at 1 and 2 (the first base must match: it seeds the candidates): level k at every
                  evaluated length, "L' >= bps + level" bites at lanes 0 .. k - 1 -- the first point is at 8 + k
    round1        the read at one place and a twin of 90 bases with substitutions at 80 and 81: tied through round 0, points from 82
                  on only
    at_M          M = g_maxMismatch[len] substitutions in the last 30 bases, the last at len - 15: level M at the last valid length
                  len - 1 (m1 == M, a point)
    past_M        the same and one more at len - 3: level M + 1 at len - 2, the abort one length before the last -- the last point
                  is at len - 3
    tie_ab/ba     no true location; twin A holds 14 bases of the read, twin B 12 and substitutions at 12 and 13 (both short-lived:
                  tier A), A before B and B before A: tied up to 12, one level apart at 13, a point of A at 14.  NOT CONTROLLED
                  AND NOT COUNTED: which quarter of tier A a twin lands in.  It follows from the twin's rank among the short-lived
                  candidates of the window, the chance survivors of the seed filter included, and nothing in the oracle's output
                  shows it; the 8 geometries x 32 anchors per order leave it to chance.  The case shows that the two orders of
                  two tied short-lived candidates give the reference's points; it does not show that a tie was merged across two
                  given quarters (the merge is the parent's code: the tree merge was not built).
    dropped       the true location carries substitutions at 2 and 5 (level 2), a clean short-lived twin of 14 bases wins the
                  lengths up to 14: CleanUniquePoints keeps the runs of the last point's candidate alone -- the kept points start
                  after 14, not at 10
    ring0         a deletion of 30-50 bases: the far end is found in the innermost range and completes the read (goodFarEndFound)
    ring2         the far part of the read is nowhere; a short-lived twin G0 of its first 20 bases lies in the innermost range, a
                  twin G2 with substitutions at 14 and 15 between 300 and 900 bases out: range 0 yields points 10 .. 20, range 2
                  -- both twins in the state -- points 16 .. 20 only, the same MaxLen: the later result replaces the earlier (>=)

How many reads of each case reach the situation is counted on the oracle's output alone, before any GPU result is looked at, and
asserted against WANT below.  Of 256 reads per case and length (random: 200), at 100 / 101 / 150 / 151 bases:
    random 158 / 156 / 160 / 161      abort0 192 / 256 / 224 / 256      first1 256 / 219 / 244 / 224      first2 168 / 221 / 201 / 230
    every other case 256 at every length
(the reads that fall short meet a chance candidate of the window within two levels of the planted one at the lengths in question)."""
import numpy as np
import pytest

from oracle import pyoracle
from pindel_amd import synth
from pindel_amd.hostio import SPACER
from tests import instantiations as I
from tests import shortening_cases as sc
from tests.parity import compare_result, run_oracle
from tests.test_gpu_far_seam_states import _both_entries

pytestmark = pytest.mark.gpu

BIOL = 300_000
ISZ = 500
ISZ_NARROW = 80
SLOT = 2500
GEOMS = 4          # slots per (case, strand)
REPS = 32          # anchor positions per slot
LENGTHS = (100, 101, 150, 151)
PLANTED = ("abort0", "only_bps", "only_last", "boundary", "first1", "first2", "round1", "at_M", "past_M", "tie_ab", "tie_ba",
           "dropped", "ring0", "ring2")
N_RANDOM = 200
# CheckMismatches also rejects a point whose read, laid along the reference from the point's start, shows fewer than 2 % mismatches (a
# read that simply maps): a read that lies at one place carries these four substitutions, each where g_maxMismatch allows its level
NOISE = [34, 44, 54, 76]
# reads of the case (of 2 x GEOMS x REPS = 256, random: 200) that must reach the situation, per length
WANT = dict(random=100, abort0=128, only_bps=160, only_last=224, boundary=224, first1=160, first2=128, round1=224, at_M=224,
            past_M=224, tie_ab=192, tie_ba=192, dropped=192, ring0=224, ring2=160)

_COMP = np.zeros(256, dtype=np.uint8)
_COMP[list(b"ACGTN")] = list(b"TGCAN")
_NXT = np.zeros(256, dtype=np.uint8)
_NXT[list(b"ACGT")] = list(b"CGTA")


def _sub(a, idx):
    for i in idx:
        a[i] = _NXT[a[i]]


def _build(L, seed):
    """(reference, batch, case name of every read).  Works on the forward strand: `true` is the read as the reference shows it,
    close part and far part; a '+' anchor's read is its reverse complement and its close end the left part."""
    rng = np.random.default_rng(seed)
    refb = np.frombuffer(synth.make_reference(BIOL, seed=seed + 1), dtype=np.uint8).copy()
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    M = int(pyoracle.max_mismatch_table()[L])
    seqs, strand, pos, names, iszs = [], [], [], [], []
    slot = 0
    for name in PLANTED:
        for plus in (True, False):
            for _ in range(GEOMS):
                mid = SPACER + 4000 + SLOT * slot + SLOT // 2
                slot += 1
                assert mid + SLOT < SPACER + BIOL - 4000
                whole = name in ("only_last", "round1", "at_M", "past_M")     # no far part: the read lies at one place
                c = L if whole else (80 if name == "boundary" else 60)         # the close part's length
                d = 0 if whole else (int(rng.integers(30, 50)) if name == "ring0" else 200)
                # the close part lies at [a0, a0 + c): consumed from a0 upwards ('+') or from a0 + c - 1 downwards ('-')
                a0 = mid if plus else mid - c
                close = refb[a0:a0 + c].copy()

                def at(j, base=None):
                    """reference index of the close end's consumed index j (of a copy `base` bases further on)"""
                    return (a0 + j if plus else a0 + c - 1 - j) + (base or 0)

                def twin(delta, n, subs):
                    """plant the first n consumed bases `delta` bases further on, substitutions at `subs`"""
                    for j in range(n):
                        refb[at(j, delta)] = refb[at(j)]
                    _sub(refb, [at(j, delta) for j in subs])

                cons = close if plus else close[::-1]         # (a view: edits below go to the read, not to the reference)
                if name in ("tie_ab", "tie_ba", "dropped"):
                    first = 200 if name == "tie_ab" else -200
                    if name == "dropped":
                        twin(first, 17, [14, 15, 16])
                        _sub(cons, [2, 5])
                    else:
                        # no true location: the read keeps its first bases, the reference under it is drawn again
                        twin(first, 17, [14, 15, 16])
                        twin(-first, 15, [12, 13, 14])
                        refb[a0:a0 + c] = rng.choice(acgt, c)
                elif name == "only_last":
                    twin(200 if plus else -200, L, [L - 3, L - 2])
                    _sub(cons, NOISE)
                elif name == "round1":
                    twin(200 if plus else -200, 90, [80, 81])
                    _sub(cons, NOISE)
                else:
                    _sub(cons, {"abort0": [1, 3, 5], "only_bps": [8, 11, 14], "first1": [1], "first2": [1, 2],
                                "at_M": [L - 15 - 5 * k for k in range(M)], "past_M": [L - 15 - 5 * k for k in range(M)] + [L - 3],
                                }.get(name, []))
                # the far part: the reference beyond a deletion of d bases, or (ring2) nothing the reference holds
                f = L - c
                if plus:
                    far = refb[a0 + c + d:a0 + c + d + f].copy()
                else:
                    far = refb[a0 - d - f:a0 - d].copy()
                if name == "ring2":
                    far = rng.choice(acgt, f)
                    fcons = far[::-1] if plus else far            # the far end consumes the read from its other end
                    center = a0 + c - 1 if plus else a0           # the last close-end point
                    for dist, subs in ((30, [20, 21, 22]), (int(rng.integers(300, 900)), [14, 15, 20, 21, 22])):
                        # a far-end candidate `dist` bases beyond the center, consumed towards it
                        g = fcons[:23].copy()
                        _sub(g, subs)
                        for j in range(23):
                            refb[center + dist + 22 - j if plus else center - dist - 22 + j] = g[j]
                true = np.concatenate([close, far]) if plus else np.concatenate([far, close])
                # (a narrow window where the point of the case is a level-1 or level-2 candidate alone at the shortest lengths:
                # among 500 positions chance candidates within two levels of it are the rule)
                isz = ISZ_NARROW if name in ("abort0", "only_bps", "first1", "first2") else ISZ
                for _ in range(REPS):
                    # the anchor: the close end `slack` bases inside the R = 0 window, twins 200 bases either side included
                    slack = int(rng.integers(5, isz - 5)) if isz == ISZ_NARROW else int(rng.integers(210, ISZ - 210 - 20))
                    apos = (a0 - slack if plus else a0 + c + slack) - SPACER
                    seqs.append((_COMP[true[::-1]] if plus else true).tobytes())
                    strand.append(ord("+") if plus else ord("-"))
                    pos.append(apos)
                    names.append(name)
                    iszs.append(isz)
    for i in range(N_RANDOM):
        seqs.append(rng.choice(acgt, L).tobytes())
        strand.append(ord("+") if i & 1 else ord("-"))
        pos.append(int(rng.integers(5000, BIOL - 5000)))
        names.append("random")
        iszs.append(ISZ)
    return [("chrE", refb.tobytes())], sc.batch_of(seqs, strand, pos, iszs), np.array(names)


def _reached(orc, i, name, L, M):
    """does read i reach the situation its case is about ?  (the oracle's points alone)"""
    cp = orc["close_pts"][i][:int(orc["close_cnt"][i])]
    fp = orc["far_pts"][i][:int(orc["far_cnt"][i])]
    cl = cp["length"].tolist()
    cm = cp["mismatches"].tolist()
    fl = fp["length"].tolist()
    if name in ("random", "abort0"):
        return not cl and not fl
    noise = len(NOISE)
    if name == "only_bps":
        return cl == [8] and cm == [0]
    if name == "only_last":
        return cl == [L - 1] and cm == [noise]
    if name == "boundary":
        return 71 in cl and 72 in cl and cm[cl.index(71)] == cm[cl.index(72)]
    if name in ("first1", "first2"):
        k = int(name[-1])
        return bool(cl) and min(cl) == 8 + k and cm[cl.index(8 + k)] == k
    if name == "round1":
        return bool(cl) and min(cl) == 82 and cm[cl.index(82)] == noise
    if name == "at_M":
        return bool(cl) and max(cl) == L - 1 and cm[cl.index(L - 1)] == M
    if name == "past_M":
        return bool(cl) and max(cl) == L - 3 and cm[cl.index(L - 3)] == M
    if name in ("tie_ab", "tie_ba"):
        return bool(cl) and min(cl) == 14 and cm[cl.index(14)] == 0
    if name == "dropped":
        return bool(cl) and min(cl) > 14 and set(cm) == {2}
    if name == "ring0":
        return bool(cl) and bool(fl) and max(cl) + max(fl) >= L
    if name == "ring2":
        return fl == [16, 17, 18, 19, 20]
    raise AssertionError(name)


_CASES = {}


def _case(L):
    """(reference, batch, the oracle's result, reference and oracle result of the batch with one shorter read), built once; asserts
    that every case reaches its situation"""
    if L not in _CASES:
        ref, batch, names = _build(L, seed=5100 + L)
        orc = run_oracle({}, ref, batch)
        M = int(pyoracle.max_mismatch_table()[L])
        counts = {}
        for name in ("random",) + PLANTED:
            idx = np.nonzero(names == name)[0]
            counts[name] = sum(_reached(orc, int(i), name, L, M) for i in idx)
        short = [c for c in counts if counts[c] < WANT[c] or counts[c] == 0]
        assert not short, ("cases that do not reach their situation", {c: counts[c] for c in short}, counts)
        # the default-parameter kernel's batch: one read of another length in front (a clean read without its first two bases)
        seqs = sc.seqs_of(batch)
        i0 = int(np.nonzero(names == "boundary")[0][0])
        other = seqs[i0][2:]
        mixed = sc.batch_of([other] + seqs, [batch.anchor_strand[i0]] + batch.anchor_strand.tolist(),
                            [batch.anchor_pos[i0]] + batch.anchor_pos.tolist(), [ISZ] + batch.insert_size.tolist())
        _CASES[L] = (ref, batch, orc, mixed, run_oracle({}, ref, mixed))
    return _CASES[L]


def _fused_kernel(eng, L, fixed, default):
    assert eng.last_fixed_len() == fixed
    recs = [tuple(r) for r in eng.launch_log() if tuple(r)[0] == I.SEARCH]
    assert len(recs) == 1, recs
    want = I.search_rec(I.class_blocks(L, True), I.counter_slices(I.levels_of(L)), 32, I.BOTH, default, 1)
    assert recs[0] == want, (recs, want)


@pytest.mark.parametrize("path", ["fixed", "default", "generic"])
@pytest.mark.parametrize("L", LENGTHS)
def test_evaluation_edges(engine_factory, pg_env, L, path):
    ref, batch, orc, mixed, orc_mixed = _case(L)          # (asserts the coverage)
    if path == "generic":
        pg_env.set("PG_GENERIC_KERNELS", "1")
    if path == "default":
        batch, orc = mixed, orc_mixed
    eng = engine_factory()
    eng.load_reference(ref)
    db = eng.upload(batch)
    try:
        eng.scribble_records(db)
        eng.clear_launch_log()
        eng.pack_search_device(db)
        _fused_kernel(eng, L, L if path == "fixed" else 0, path != "generic")
        compare_result(eng.download(db), orc, batch.n)
    finally:
        eng.free_device_batch(db)


@pytest.mark.parametrize("L", LENGTHS)
def test_evaluation_edges_far_only(engine_factory, L):
    """the split entries: a close-end launch, then far-only launches over the reads it left (150 / 151 bases: the short form with a
    run-time length); _both_entries asserts the far-only kernel from the launch log and compares both ends with the oracle"""
    ref, batch, orc, _, _ = _case(L)
    assert (orc["far_cnt"][:batch.n] > 0).sum() >= WANT["ring0"] + WANT["ring2"]      # the far-only launch has far ends to find
    eng = engine_factory()
    eng.load_reference(ref)
    _both_entries(eng, batch, None, None, orc)
