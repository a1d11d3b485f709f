"""Junction reads for the interchromosomal junction tables on the three-chromosome reference of
tests/interchr_synth.py: 100-base split reads across its four planted junctions, anchored on either side ('+' left of the junction,
'-' right of it), with the far part on the far chromosome's own strand or on its reverse strand (the far end is then ANTISENSE),
with or without a few bases inserted at the junction (a fallback call with bases), and '-' anchored ones followed by two bytes outside
ACGTN (rc_flag 2).  Deletion reads on chrA and reads of a repeat the reference does not hold are the reads that are no junction reads.
The far ends are reached through one hint table: a single run over every position, whose cluster holds a window around each of the
six breakpoints."""
import numpy as np

from pindel_amd import hostio
from pindel_amd.binding import HintTable, WINDOW_DTYPE
from tests import interchr_synth as syn

SPACER = 100000
READ, ISZ = syn.READ, syn.ISZ
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
NT = b"GATTACAG"


def revcomp(s: bytes) -> bytes:
    return s.translate(_COMP)[::-1]


def hint_table(width=300):
    """one run over all positions of a padded chromosome, one cluster: a window of +- width around every breakpoint"""
    points = [(0, syn.X), (1, syn.Y), (1, syn.U), (2, syn.V), (2, syn.W), (0, syn.Z)]
    win = np.zeros(len(points), dtype=WINDOW_DTYPE)
    win["chr_id"] = [c for c, _ in points]
    win["start"] = [SPACER + p - width for _, p in points]
    win["end"] = [SPACER + p + width for _, p in points]
    return HintTable([SPACER, SPACER + syn.CHR_LEN + 1], [1], [0, 0, len(points)], win)


def _snp(part: bytes) -> bytes:
    """the base in the middle of `part` replaced by another one"""
    at = len(part) // 2
    return part[:at] + (b"A" if part[at:at + 1] != b"A" else b"C") + part[at + 1:]


def junction_read(biol, j, k, plus_anchor, antisense=False, nt=b"", tail=b"", snp=False):
    """One record (sequence, strand, anchor position, chromosome) of junction j = (lc, p, _, rc, q): k bases (plus nt) left of the
    junction.  A '+' anchor lies on lc upstream of p, a '-' anchor on rc downstream of q; the other side is the far end.  snp: a
    mismatch in the middle of either part, so that the points before and behind it form runs of their own."""
    lc, p, _, rc, q = j
    m = READ - k - len(nt)
    mark = _snp if snp else (lambda part: part)
    if plus_anchor:
        right = revcomp(biol[rc][q - m:q]) if antisense else biol[rc][q:q + m]
        fwd = mark(biol[lc][p - k:p]) + nt + mark(right)
        return revcomp(fwd) + tail, b"+", p - k + READ - ISZ, lc
    left = revcomp(biol[lc][p:p + k]) if antisense else biol[lc][p - k:p]
    fwd = mark(left) + nt + mark(biol[rc][q:q + m])
    return fwd + tail, b"-", q + ISZ - k - len(nt), rc


def records(biol, n, seed=0, shortened_every=0, snp_every=0):
    """n junction reads cycling over the four junctions, both anchor sides, both far strands and the inserted bases; every
    snp_every-th with a mismatch in the middle of either part"""
    rng = np.random.default_rng(seed)
    js = syn.junctions()
    out = []
    for i in range(n):
        j = js[i % 4]
        plus = (i // 4) % 2 == 0
        antisense = (i // 8) % 2 == 1
        nt = NT if (i // 16) % 3 == 2 else b""
        k = int(rng.integers(30, 61))
        rec = junction_read(biol, j, k, plus, antisense, nt, snp=bool(snp_every) and i % snp_every == snp_every - 2)
        if shortened_every and i % shortened_every == shortened_every - 1:
            s, strand, pos, c = junction_read(biol, j, k, False, antisense, nt, tail=b"XX")
            rec = (s, strand, pos - ISZ, c)          # the anchor one insert size away: the fourth attempt keeps the close end
        out.append(rec)
    return out


def fillers(biol, n, seed=1):
    """reads that are no junction reads: across the 40-base deletion on chrA (a far end on the same chromosome), and of a repeat the
    reference does not hold (no close end)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if i % 3 == 2:
            out.append((b"AC" * 50, b"-", int(rng.integers(20_000, 80_000)), int(rng.integers(0, 3))))
            continue
        k = int(rng.integers(30, 61))
        out.append(junction_read(biol, (0, syn.DEL_AT, b"", 0, syn.DEL_AT + syn.DEL_LEN), k, i % 2 == 0))
    return out


def batch_from(recs):
    return hostio.batch_from_lists([r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs], [ISZ] * len(recs), [r[3] for r in recs])


def biological(chroms):
    return [bytes(np.frombuffer(s, dtype=np.uint8)[SPACER:-SPACER]) for _, s in chroms]
