"""Constructed reads for the device classifier's tests (tests/test_gpu_variant_candidates.py): small references with the
structures that make the classifier's paths differ -- repeats (long alignment walks), microhomology (several qualifying pairs,
ordered by strand), mismatches near the breakpoint (the mismatch sum orders before the close point), long reads (more than 64
close points), a second chromosome.  Every case is (name, chromosomes, batch); what a case must show is asserted by the test
on the expected arrays, so a case that stops exercising its path fails loudly."""
import numpy as np

from tests.shortening_cases import batch_of, rc_ref

SPACER = 100000


def rand_bases(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=n))


def padded(bio: bytes) -> bytes:
    return b"N" * SPACER + bio + b"N" * SPACER


def split_read(bio, left_start, left_len, right_start, read_len, plus, ins=b"", slack=120, mutate=()):
    """A read whose first left_len bases are bio[left_start:], then `ins`, then bio[right_start:] up to read_len bases in all
    (forward strand); mutate: offsets in the read whose base is replaced by another one.  A '+' anchor lies upstream (its
    close end is the left part; the read comes reverse-complemented, as its mate was sequenced), a '-' anchor downstream.
    Returns (sequence, strand, anchor position)."""
    right_len = read_len - left_len - len(ins)
    fwd = bytearray(bio[left_start:left_start + left_len] + ins + bio[right_start:right_start + right_len])
    assert len(fwd) == read_len
    for at in mutate:
        fwd[at] = ord("A") if fwd[at] != ord("A") else ord("C")
    if plus:
        return rc_ref(bytes(fwd)), ord("+"), max(left_start - slack, 0)
    return bytes(fwd), ord("-"), right_start + right_len + slack


def both_strands(bio, *a, **kw):
    return [split_read(bio, *a, plus=True, **kw), split_read(bio, *a, plus=False, **kw)]


def as_batch(reads, isz=500, chr_id=0):
    return batch_of([r[0] for r in reads], [r[1] for r in reads], [r[2] for r in reads], [isz] * len(reads), chr_id)


def repeat_cases(seed=5):
    """Deletions inside a 300-base homopolymer and a dinucleotide repeat (150-bp reads: flank, up to 90 repeat bases, flank), one
    whose left walk is stopped by an N in the deleted copy, microhomology at the breakpoint, insertions into repeats."""
    rng = np.random.default_rng(seed)
    flank = lambda n: rand_bases(rng, n, b"CGT")             # (no A: the homopolymer's ends are where the flanks begin)
    out = []
    # -- homopolymer: reference flank + A x 300 + flank, reads see 40 / 90 of the A's
    left, right = flank(3000), flank(3000)
    bio = left + b"A" * 300 + right
    reads = []
    for L, seen in ((100, 40), (150, 90)):
        fl = (L - seen) // 2
        for cut in (0, seen // 2, seen):                      # where in the read's run of A's the two parts meet
            reads += both_strands(bio, len(left) - fl, fl + cut, len(left) + 300 - (seen - cut), L)
    out.append(("homopolymer", [("chrH", padded(bio))], as_batch(reads)))
    # -- ... with an N among the deleted A's, five bases left of the far part's copy (the pairs listed first walk a few bases
    # only; the long walk that an N ends is long_left_walk_n below)
    bio_n = bytearray(bio)
    bio_n[len(left) + 300 - 90 - 5] = ord("N")
    out.append(("homopolymer_n", [("chrH", padded(bytes(bio_n)))], as_batch(reads[6:])))
    # -- dinucleotide repeat (CT) x 150 between A/G flanks
    fl2 = lambda n: rand_bases(rng, n, b"AG")
    left2, right2 = fl2(3000), fl2(3000)
    bio2 = left2 + b"CT" * 150 + right2
    reads2 = []
    for L, seen in ((100, 40), (150, 90), (150, 89)):
        fl = (L - seen) // 2
        reads2 += both_strands(bio2, len(left2) - fl, fl + seen // 2, len(left2) + 300 - (seen - seen // 2), L)
    out.append(("dinucleotide", [("chrD", padded(bio2))], as_batch(reads2)))
    # -- a decoy 500 bases upstream -- the left flank's last 30 bases and 70 A's -- makes every close point of a '+' read that ends
    # within the first 70 A's ambiguous: the first close point left is 71 A's into the run, and the left walk takes them all back
    # (more than 64 positions, over a plane word's boundary); with an N among the deleted A's the walk ends there instead
    for name, n_at in (("long_left_walk", None), ("long_left_walk_n", 40)):
        for unit, alphabet in ((b"A", b"CGT"), (b"CT", b"AG")):
            lf, rf = rand_bases(rng, 3000, alphabet), rand_bases(rng, 3000, alphabet)
            rep = unit * (300 // len(unit))
            gap = rand_bases(rng, 170, alphabet)
            bio3 = lf + rep[:70] + gap + lf[-30:] + rep + rf
            start = len(lf) + 70 + len(gap) + 30                   # the true run's first base
            if n_at is not None:
                b3 = bytearray(bio3)
                b3[start + 300 - 19 - 1 - n_at] = ord("N")         # n_at bases left of the last deleted base of the first pair
                bio3 = bytes(b3)
            r = split_read(bio3, start - 30, 30 + 71, start + 300 - 19, 150, plus=True, slack=320)
            out.append((f"{name}_{unit.decode()}", [("chrW", padded(bio3))], as_batch([r])))
    return out


def microhomology_cases(seed=6):
    """A 400-base deletion whose first m bases repeat behind it (m = 3, 8): m + 1 pairs qualify without a mismatch; a mismatch in the
    read next to the breakpoint (pairs with one mismatch come earlier among the close points than the exact one); a mismatch
    deep in the far part (two far runs)."""
    rng = np.random.default_rng(seed)
    out = []
    for m in (3, 8):
        a, d, b = rand_bases(rng, 3000), rand_bases(rng, 400), rand_bases(rng, 3000)
        b = d[:m] + bytes([ord("A") if d[m] != ord("A") else ord("C")]) + b[m + 1:]      # homology of exactly m bases
        a = a[:-1] + bytes([ord("G") if d[-1] != ord("G") else ord("T")])                # ... and none on the left
        bio = a + d + b
        reads = []
        for L in (100, 150):
            reads += both_strands(bio, len(a) - L // 2, L // 2, len(a) + 400, L)
            reads += both_strands(bio, len(a) - L // 2, L // 2, len(a) + 400, L, mutate=(L - 12,))          # deep in the right part
            reads += both_strands(bio, len(a) - L // 2, L // 2, len(a) + 400, L, mutate=(10,))              # deep in the left part
        out.append((f"microhomology{m}", [("chrM", padded(bio))], as_batch(reads)))
    # a read error right behind the breakpoint region of homology: the far part reaches past it with one mismatch
    a, d, b = rand_bases(rng, 3000), rand_bases(rng, 400), rand_bases(rng, 3000)
    tail = a[-6:]
    d = d[:-6] + bytes([ord("A") if tail[0] != ord("A") else ord("C")]) + tail[1:-1] + bytes([ord("G") if tail[-1] != ord("G") else ord("T")])
    bio = a + d + b
    reads = both_strands(bio, len(a) - 50, 50, len(a) + 400, 100) + both_strands(bio, len(a) - 75, 75, len(a) + 400, 150)
    out.append(("budget_order", [("chrB", padded(bio))], as_batch(reads)))
    return out


def long_read_cases(seed=7):
    """250-bp reads with the breakpoint 150 bases in: well over 64 close points ('+' anchors) or far points ('-')."""
    rng = np.random.default_rng(seed)
    a, d, b = rand_bases(rng, 3000), rand_bases(rng, 500), rand_bases(rng, 3000)
    bio = a + d + b
    reads = both_strands(bio, len(a) - 150, 150, len(a) + 500, 250) + both_strands(bio, len(a) - 100, 100, len(a) + 500, 250)
    reads += both_strands(bio, len(a) - 150, 150, len(a), 250, ins=b"GATTACA")
    return [("long_reads", [("chrL", padded(bio))], as_batch(reads))]


def insertion_cases(seed=8):
    """Short insertions: one base into a homopolymer (at its start, inside, at its end), one unit into a tandem repeat (at
    several phases, and two units), a unique string."""
    rng = np.random.default_rng(seed)
    left, right = rand_bases(rng, 3000, b"CGT"), rand_bases(rng, 3000, b"CGT")
    left3, right3 = rand_bases(rng, 3000, b"AT"), rand_bases(rng, 3000, b"AT")
    bio = left + b"A" * 12 + right + left3 + b"ACG" * 8 + right3 + rand_bases(rng, 2000)
    h = len(left)                                              # the homopolymer's first base
    t = h + 12 + len(right) + len(left3)                       # the tandem repeat's
    u = t + 24 + len(right3) + 1000                            # a place in the unique tail
    reads = []
    for at in (0, 5, 12):
        reads += both_strands(bio, h + at - 45, 45, h + at, 100, ins=b"A")
    for at, unit in ((0, b"ACG"), (4, b"CGA"), (11, b"GAC"), (24, b"ACG"), (9, b"ACGACG")):
        reads += both_strands(bio, t + at - 60, 60, t + at, 150, ins=unit)
    reads += both_strands(bio, u - 50, 50, u, 100, ins=b"TTGCA")
    return [("insertions", [("chrI", padded(bio))], as_batch(reads))]


def chromosome_end_case(seed=9):
    """A deletion whose right breakpoint lies 30 bases before the chromosome's last base."""
    rng = np.random.default_rng(seed)
    bio = rand_bases(rng, 5000)
    L = 100
    reads = both_strands(bio, 5000 - 300 - 30 - 70, 70, 5000 - 30, L, slack=0) + both_strands(bio, 5, 60, 400, L)
    return [("chromosome_end", [("chrE", padded(bio))], as_batch(reads))]


def translocation_case(seed=10):
    """Reads whose other part lies on a second chromosome, found there through a window hint: (name, chromosomes, batch, windows,
    window offsets).  The last two reads are ordinary deletions on the first chromosome."""
    from pindel_amd.binding import WINDOW_DTYPE
    rng = np.random.default_rng(seed)
    a, b = rand_bases(rng, 6000), rand_bases(rng, 6000)
    reads, wins, offs = [], [], [0]
    for p, q in ((2000, 3000), (2500, 1500), (3100, 4000)):
        fwd = a[p - 50:p] + b[q:q + 50]
        reads.append((rc_ref(fwd), ord("+"), p - 50 - 150))
        wins.append((1, q + SPACER - 300, q + SPACER + 300))
        offs.append(len(wins))
        fwd = b[q - 50:q] + a[p:p + 50]
        reads.append((fwd, ord("-"), p + 50 + 150))
        wins.append((1, q + SPACER - 300, q + SPACER + 300))
        offs.append(len(wins))
    reads += both_strands(a, 4000 - 50, 50, 4000 + 300, 100)
    offs += [len(wins), len(wins)]
    return ("translocation", [("chrA", padded(a)), ("chrB", padded(b))], as_batch(reads), np.array(wins, dtype=WINDOW_DTYPE),
            np.array(offs, dtype=np.uint64))


def all_cases():
    return repeat_cases() + microhomology_cases() + long_read_cases() + insertion_cases() + chromosome_end_case()
