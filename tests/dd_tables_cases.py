"""Split reads for the dispersed-duplication breakpoint tables on one random chromosome.  Every read is a unique piece
of the reference that ends at a breakpoint p (a '+' anchor: the k bases before p, handed over reverse-complemented) or begins at one
(a '-' anchor: the k bases from p on), plus the unmapped part, which the case controls as a WALK: walk[i] is the base i steps away
from the breakpoint, the column i of the contract.  The first GUARD columns of every walk differ from the reference there, so that
no chance extension of the close end moves the breakpoint, and every vote edge lies behind them."""
import numpy as np

from pindel_amd import hostio

SPACER = 100000
CHR_LEN = 40000
ISZ = 300
GUARD = 8
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def reference(seed=11):
    rng = np.random.default_rng(seed)
    biol = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), CHR_LEN))
    return [("chrD", b"N" * SPACER + biol + b"N" * SPACER)], biol


def other_base(b, step=1):
    return b"ACGT"[(b"ACGT".index(b) + step) % 4]


def guarded_walk(biol, strand, p, tail):
    """GUARD bases that differ from the reference walking away from breakpoint p, then `tail`"""
    if strand == b"+":
        g = bytes(other_base(biol[p + i]) for i in range(GUARD))
    else:
        g = bytes(other_base(biol[p - 1 - i]) for i in range(GUARD))
    return g + tail


def member(biol, strand, p, k, walk, junk=b"", shift=0):
    """(bytes, strand, anchor position, chromosome): k mapped bases at breakpoint p and `walk`.  junk: bytes outside ACGTN behind a
    '-' read; shift: the anchor moved by that many bases (a later attempt of the close end finds the read)."""
    if strand == b"+":
        seq = bytes(reversed(walk)).translate(_COMP) + biol[p - k:p].translate(_COMP)[::-1]
        return seq, strand, p - k - 200 + shift, 0
    seq = bytes(reversed(walk)) + biol[p:p + k]
    return seq + junk, strand, p - len(walk) + ISZ + shift, 0


def random_tail(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n))


class Plan:
    """Segments of reads; batch() gives the ReadBatch with seg_first / seg_strand"""

    def __init__(self, biol, seed=0):
        self.biol, self.rng = biol, np.random.default_rng(seed)
        self.recs, self.seg_first, self.seg_strand = [], [0], b""
        self.k_next = 25
        self.flipped = 0

    def group(self, strand, p, n, tail=None, tail_len=24, lens=None, edits=(), junk_every=0, contained=False, flip_every=0):
        """n members at breakpoint p sharing one walk.  lens: the members' walk lengths (beyond that: the full walk); edits:
        (member, column, byte) substitutions; contained: the tail is the reference 150 bases from p (the consensus lies in its window);
        flip_every: every such member is handed over in the other orientation, every second one of the plan behind two bytes outside
        ACGTN -- the close end is found after one reverse complement (rc_flag 1), which strips those bytes: the post-state then
        begins two bytes into the read as uploaded"""
        if tail is None:
            tail = self.biol[p + 150:p + 150 + tail_len] if contained else random_tail(self.rng, tail_len)
            if contained and strand == b"-":
                tail = tail[::-1]
        walk = guarded_walk(self.biol, strand, p, tail)
        for j in range(n):
            w = bytearray(walk[:lens[j]] if lens and j < len(lens) else walk)
            for (m, col, byte) in edits:
                if m == j and col < len(w):
                    w[col] = byte
            k = self.k_next
            self.k_next = 25 + (self.k_next - 24) % 150                # a unique piece of the reference per member of a group
            junk = b"XX" if junk_every and strand == b"-" and j % junk_every == junk_every - 1 else b""
            rec = member(self.biol, strand, p, k, bytes(w), junk, -ISZ if junk else 0)
            if flip_every and not junk and j % flip_every == flip_every - 1:
                self.flipped += 1
                lead = b"XX" if self.flipped % 2 == 0 else b""
                rec = (lead + rec[0].translate(_COMP)[::-1],) + rec[1:]
            self.recs.append(rec)
        return walk

    def stray(self, strand, n=1):
        """reads without a close end: a repeat the reference does not hold"""
        for _ in range(n):
            self.recs.append((b"AC" * 40, strand, int(self.rng.integers(1000, CHR_LEN - 1000)), 0))

    def end_segment(self, strand):
        self.seg_first.append(len(self.recs))
        self.seg_strand += strand

    def batch(self):
        r = self.recs
        return (hostio.batch_from_lists([x[0] for x in r], [x[1] for x in r], [x[2] for x in r], [ISZ] * len(r), [x[3] for x in r]),
                np.array(self.seg_first, dtype=np.uint32), self.seg_strand)


def sized_batch(biol, n, seed=0):
    """n reads in two segments, one per strand (the second one empty below 2 reads): groups of 3 to 5 members 120 bases apart"""
    pl = Plan(biol, seed)
    left = n
    p = 2000
    for strand in (b"+", b"-"):
        want = left if strand == b"-" else (n + 1) // 2
        while want > 0:
            g = min(want, 3 + (p // 120) % 3)
            pl.group(strand, p, g, lens=[GUARD + 24 - (j % 3) for j in range(g)], junk_every=4 if strand == b"-" else 0,
                     contained=(p // 120) % 2 == 0, flip_every=3)
            want -= g
            left -= g
            p += 120
        pl.end_segment(strand)
    return pl


def counted_candidates(biol, n_cands, seed=0):
    """n_cands candidates of three members each, alternating segments of either strand, with an empty segment between them, a key one
    member short of the support, a read of the other strand and a read without a close end"""
    pl = Plan(biol, seed)
    p = 3000
    for strand in (b"+", b"-"):
        for c in range(n_cands // 2 + (n_cands % 2 if strand == b"+" else 0)):
            pl.group(strand, p, 3, contained=c % 2 == 1)
            p += 110
        pl.group(strand, p, 2)                                        # one short of min_bp_support 3
        p += 110
        pl.group(b"-" if strand == b"+" else b"+", p, 3)              # the other strand: not DD reads of this segment
        p += 110
        pl.stray(strand)
        pl.end_segment(strand)
        pl.end_segment(b"-")                                          # a segment of no reads
    pl.group(b"+", p, 3)                                              # outside every segment
    return pl


def dd_read_totals(biol, k, seed=0):
    """Exactly k DD reads beside reads that are none: keys of three members each, half of them in a '+' segment and half in a '-'
    segment over the same breakpoints, appended in a shuffled order of position (the sort has work to do); the k % 3 reads left over
    form one key below the support at the highest position of the '-' segment, so that every DD record in front of it is a member
    and sorted record m is member m: key 85 holds records 255, 256 and 257, key 170 records 510 to 512, key 256 begins at 768.
    The reads that are none can be no DD reads whatever the search finds for them: groups of the other strand inside either
    segment, and a group behind the last segment."""
    pl = Plan(biol, seed)
    keys = k // 3
    per_seg = [(keys + 1) // 2, keys // 2]
    for s, strand in enumerate((b"+", b"-")):
        other = b"-" if strand == b"+" else b"+"
        order = pl.rng.permutation(per_seg[s])
        for j, g in enumerate(order):
            pl.group(strand, 1500 + 110 * int(g), 3)
            if j % 40 == 7:
                pl.group(other, 1500 + 110 * int(g), 3)              # the other strand at the same breakpoint: no DD reads
        if s == 1 and k % 3:
            pl.group(strand, 1500 + 110 * per_seg[1], k % 3)         # below min_bp_support 3: DD reads that are no members
        pl.group(other, 1555, 3)
        pl.end_segment(strand)
    pl.group(b"+", 1500, 3)                                           # outside every segment
    return pl


def assert_dd_read_totals(t, every, k, block=256):
    """What dd_read_totals(biol, k) is meant to hold, on the statement's tables at min_bp_support 3 (t) and 1 (every: each DD read is
    a member there, so its member count is the DD-read count)"""
    assert len(every["members"]) == k and len(t["members"]) == k - k % 3
    c = t["cands"]
    assert len(c) == k // 3 and (c["n_reads"] == 3).all() and set(c["seg"].tolist()) == {0, 1}
    # the members are the first k - k % 3 DD records in sorted order: the same reads in the same places
    assert every["members"]["read"][:len(t["members"])].tolist() == t["members"]["read"].tolist()
    pos = c["pos"].astype(np.int64) + (c["seg"].astype(np.int64) << 32)
    assert (np.diff(pos) > 0).all()
    if k > block + 1:
        across = c[(c["first"] < block) & (c["first"] + c["n_reads"] > block)]
        assert len(across) == 1 and int(across[0]["first"]) == block - 1          # records 255, 256 and 257
        assert (c["first"] % block == 0).sum() >= 2                               # ... and a key that begins a block


def one_big_candidate(biol, n_members, seed=0):
    """one candidate of n_members members whose walks shrink (n falls along the columns), beside a small one at the same position in
    a segment of the other strand"""
    pl = Plan(biol, seed)
    pl.group(b"-", 9000, n_members, tail_len=40, lens=[GUARD + 40 - (j % 23) for j in range(n_members)])
    pl.end_segment(b"-")
    pl.group(b"+", 9000, 4)
    pl.end_segment(b"+")
    return pl


def vote_edges(biol, seed=0):
    """The edges of the vote, each a few columns behind the guard: 4 of 5 (accepted) and 3 of 4 (rejected, leaving exactly 15 columns),
    a two-way tie (14 columns: dropped), a byte >= 0x80 tied with a base on the '-' strand, an IUPAC letter in every member of a '+'
    group (byte 0 wins its column), members of different lengths, reads shortened by the search (bytes outside ACGTN behind them), reads handed over in
    the other orientation (rc_flag 1), some behind bytes outside ACGTN"""
    pl = Plan(biol, seed)
    pl.group(b"+", 5000, 5, tail_len=16, edits=[(3, GUARD + 6, ord("N"))], lens=[GUARD + 16] * 4 + [GUARD + 12])       # 4 of 5
    pl.group(b"+", 5200, 4, tail_len=16, edits=[(2, 15, ord("N"))])                                                    # 3 of 4 in column 15
    pl.group(b"+", 5400, 4, tail_len=16, edits=[(2, 14, ord("N")), (3, 14, ord("N"))])                                 # tie in column 14
    pl.group(b"+", 5600, 3, tail_len=12, edits=[(m, GUARD + 3, ord("R")) for m in range(3)])                           # byte 0 wins
    pl.group(b"+", 5800, 5, tail_len=20, flip_every=1, lens=[GUARD + 20 - j for j in range(5)])                        # rc_flag 1, two with a lead
    pl.end_segment(b"+")
    pl.group(b"-", 5000, 4, tail_len=16, edits=[(0, GUARD + 9, 0xc1), (1, GUARD + 9, 0xc1)])                           # tie with a byte >= 0x80
    pl.group(b"-", 5200, 6, tail_len=20, junk_every=2, lens=[GUARD + 20 - j for j in range(6)])
    pl.group(b"-", 5400, 3, tail_len=20, contained=True)
    pl.group(b"-", 5600, 5, tail_len=20, flip_every=1, lens=[GUARD + 20 - j for j in range(5)])                        # rc_flag 1 on this strand
    pl.end_segment(b"-")
    return pl
