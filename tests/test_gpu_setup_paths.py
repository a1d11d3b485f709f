"""-m gpu: the two set-up fast paths of the search kernel, at the inputs where they switch, against the oracle bit for bit.

Close end (scan_staged, pg_kernels.hip): attempt 0 runs as straight-line code on the window staged at the start of the read when
that window is one whole chunk -- insert size 682 (3 x 682 = 2046: the shared grid of the R = 1 window), 683 (2049: the read's own
grid, one chunk) -- and through the generic path otherwise: insert size 2049 (own grid, more than a chunk), a first consumed base
'N', a read too short for a close end.  Far end: "no clipping" holds when the widest range keeps clear of both spacers; the close
ends are placed so that center - maxspan - spacer and center + maxspan + spacer - chr_size take the values -1, 0 and +1.

Every case goes through search_device and pack_search_device, on the default-parameter kernels and with PG_GENERIC_KERNELS=1.
The conditions that keep a case from passing vacuously are asserted on the oracle's result (CPU) before the GPU runs."""
import numpy as np
import pytest

from pindel_amd import hostio, synth
from pindel_amd.hostio import SPACER
from tests.parity import compare_result, run_oracle

pytestmark = pytest.mark.gpu

CHUNK = 2048
BIOL = 300_000
_RC = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTN", b"TGCAN"):
    _RC[_a] = _b


@pytest.fixture(scope="module")
def ref():
    # (300 000 bases: too short for make_reference's N gaps and repeat family -- plain sequence between the two spacers)
    return [("chrP", synth.make_reference(BIOL, seed=707))]


def _split_read(refb, plus, bp, sp, d, length):
    """A read with a deletion of d bases at AbsLoc bp, sp bases left of it, as Pindel receives it: (sequence, AbsLoc where its
    close end is grown from).  '+' anchor: the mate comes from the reverse strand, the close end is the left part, grown left to
    right from its first base; '-': the right part, grown right to left from its last base."""
    bases = np.concatenate([refb[bp - sp:bp], refb[bp + d:bp + d + length - sp]])
    if plus:
        return _RC[bases[::-1]], bp - sp
    return bases, bp + d + length - sp - 1


def _stage_start(apos, plus, isz):
    """first position of the window staged at the start of the read (pack_block, pg_kernels.hip)"""
    w1s = apos - isz if plus else apos - 2 * isz
    return w1s if 0 < 3 * isz <= CHUNK else w1s + isz


def _close_batch(refb, length, isz, seed):
    """(batch, attempt-3 reads).  340 reads: ordinary ones on both strands, then groups that set the staged window's first base
    at bit 0 and at bit 31 of a reference word, move the anchor so that only the R = 1 window holds the close end (attempt 3),
    put an 'N' at either end of the read, lean the window over the chromosome's first word, and one 8-base read."""
    rng = np.random.default_rng(seed)
    seqs, strands, pos = [], [], []
    att3 = []
    for i in range(340):
        plus = bool(i & 1)
        sp = int(rng.integers(length // 4, 3 * length // 4))
        d = int(rng.integers(30, 400))
        bp = int(rng.integers(SPACER + 3 * isz + 200, SPACER + BIOL - 3 * isz - 1000))
        s, at = _split_read(refb, plus, bp, sp, d, length)
        s = s.copy()
        err = rng.random(length) < 0.01
        s[err] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), int(err.sum()))
        slack = int(rng.integers(0, isz - 40))
        # '+': the R = 0 window is [apos, apos + isz), '-': [apos - isz, apos)
        apos = at - slack if plus else at + 1 + slack
        if 100 <= i < 180:
            want = 0 if i < 140 else 31
            # (slack < isz - 40: the close end stays inside the R = 0 window)
            if plus:
                apos -= (_stage_start(apos, plus, isz) - want) % 32
            else:
                apos += (want - _stage_start(apos, plus, isz)) % 32
            assert _stage_start(apos, plus, isz) % 32 == want
        elif 180 <= i < 240:
            # the close end in one of the R = 1 window's outer thirds: below the R = 0 window or beyond it
            off = int(rng.integers(20, isz - 20))
            if i & 2:
                apos = at + off if plus else at + isz + 1 + off
            else:
                apos = at - isz - off if plus else at - off
            att3.append(i)
        elif 240 <= i < 260:
            s[-1] = ord("N")            # the first base attempt 0 consumes (orientation 1)
        elif 260 <= i < 280:
            s[0] = ord("N")             # ... and the retries'
        elif 280 <= i < 288:
            plus = False
            apos = 2 * isz + 2 + (0, 1, 29, 30, 31, 32, 61, 126)[i - 280]       # (the smallest anchors pg_api accepts: w1s = 2 ...)
        elif i == 300:
            s = s[:8]
        seqs.append(s.tobytes())
        strands.append(b"+" if plus else b"-")
        pos.append(apos - SPACER)
    n = len(seqs)
    return hostio.batch_from_lists(seqs, strands, pos, [isz] * n, [0] * n), np.array(att3)


def _run_both_ways(engine_factory, pg_env, ref, batch, orc, **params):
    for generic in (False, True):
        if generic:
            pg_env.set("PG_GENERIC_KERNELS", "1")
        eng = engine_factory(**params)
        eng.load_reference(ref)
        db = eng.upload(batch)
        eng.search_device(db)
        compare_result(eng.download(db), orc, batch.n)
        eng.scribble_records(db)
        eng.pack_search_device(db)
        compare_result(eng.download(db), orc, batch.n)
        eng.free_device_batch(db)


@pytest.mark.parametrize("isz", [682, 683, 2049])
@pytest.mark.parametrize("length", [100, 129])
def test_close_end_attempt_0(engine_factory, pg_env, ref, length, isz):
    refb = np.frombuffer(ref[0][1], dtype=np.uint8)
    batch, att3 = _close_batch(refb, length, isz, seed=1000 + 7 * length + isz)
    orc = run_oracle({}, ref, batch)
    has = orc["close_cnt"][:batch.n] > 0
    assert has.sum() * 2 >= batch.n, "fewer than half of the reads have a close end"
    for strand in b"+-":
        assert (has & (batch.anchor_strand == strand)).sum() >= 100
    assert has[100:140].sum() >= 20 and has[140:180].sum() >= 20, "the word-aligned / bit-31 windows find no close end"
    # attempt 3: found in the original orientation, at a position the R = 0 window does not hold -- attempt 0 failed
    apos = batch.anchor_pos.astype(np.int64) + SPACER
    n3 = 0
    for i in att3:
        if has[i] and orc["rc_flag"][i] == 0:
            p = int(orc["close_pts"][i][0]["abs_loc"])
            lo = apos[i] if batch.anchor_strand[i] == ord("+") else apos[i] - isz
            if not (lo <= p < lo + isz):
                n3 += 1
    assert n3 >= 20, f"{n3} reads find their close end at attempt 3"
    assert not has[300] and not has[280:288].any()
    _run_both_ways(engine_factory, pg_env, ref, batch, orc)


def _far_batch(refb, maxspan, seed, max_del):
    """300 reads: a third with the last close-end point (the far end's center) within a few bases of spacer + maxspan, a third
    as close to chr_size - spacer - maxspan, a third anywhere."""
    rng = np.random.default_rng(seed)
    size = len(refb)
    seqs, strands, pos = [], [], []
    isz, length = 500, 100
    for i in range(300):
        plus = bool(i & 1)
        sp = int(rng.integers(30, 70))
        d = int(rng.integers(40, max_del))
        jit = int(rng.integers(-2, 3))
        if i % 3 == 0:
            c = SPACER + maxspan + jit
        elif i % 3 == 1:
            c = size - SPACER - maxspan + jit
        else:
            c = int(rng.integers(SPACER + 20_000, size - SPACER - 20_000))
        # '+': the close end is the left part, its last point bp - 1; '-': the right part, its last point bp + d
        bp = c + 1 if plus else c - d
        if not plus and bp - sp < SPACER + 5:
            d = int(rng.integers(40, min(max_del, maxspan - 80)))
            bp = c - d
        s, at = _split_read(refb, plus, bp, sp, d, length)
        slack = int(rng.integers(0, isz - 40))
        apos = at - slack if plus else at + 1 + slack
        seqs.append(s.tobytes())
        strands.append(b"+" if plus else b"-")
        pos.append(apos - SPACER)
    n = len(seqs)
    return hostio.batch_from_lists(seqs, strands, pos, [isz] * n, [0] * n)


@pytest.mark.parametrize("x", [2, 1, 3])
def test_far_end_clipping_test(engine_factory, pg_env, ref, x):
    refb = np.frombuffer(ref[0][1], dtype=np.uint8)
    size = len(refb)
    maxspan = 64 << (2 * x)
    batch = _far_batch(refb, maxspan, seed=2000 + x, max_del=min(900, maxspan - 60) if x < 3 else 3800)
    params = dict(max_range_index=x)
    orc = run_oracle(params, ref, batch)
    n = batch.n
    far = orc["far_cnt"][:n] > 0
    assert far.sum() * 4 >= n, "fewer than a quarter of the reads have a far end"
    # the far end's center: the last close-end point
    center = np.array([int(orc["close_pts"][i][orc["close_cnt"][i] - 1]["abs_loc"]) if orc["close_cnt"][i] else -1 for i in range(n)])
    lo_edge = center - maxspan - SPACER
    hi_edge = center + maxspan + SPACER - size
    for v in (-1, 0, 1):
        assert ((lo_edge == v) & (center >= 0)).sum() >= 3, f"no read with center - maxspan - spacer = {v}"
        assert ((hi_edge == v) & (center >= 0)).sum() >= 3, f"no read with center + maxspan + spacer - chr_size = {v}"
    edge = (center >= 0) & ((np.abs(lo_edge) <= 1) | (np.abs(hi_edge) <= 1))
    assert (far & edge).sum() >= 10, "the reads at the edges find no far end"
    if x == 3:
        # far ends that only the range beyond the innermost chunk reaches
        dist = np.array([abs(int(orc["far_pts"][i][0]["abs_loc"]) - center[i]) if far[i] else 0 for i in range(n)])
        assert (dist > 1100).sum() >= 10
    _run_both_ways(engine_factory, pg_env, ref, batch, orc, **params)
