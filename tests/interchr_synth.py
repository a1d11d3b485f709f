"""A synthetic sample with planted interchromosomal junctions for -I (tests/bam_writer.py), in the style of dd_synth.py.

Three chromosomes of random sequence, chrA < chrB < chrC, each CHR_LEN long (five search windows at `-w WINDOW_MBP`).
The sample carries three junctions; each is a derivative chromosome `left[:p] + nt + right[q:]`:

  (i)   chrA:X <-> chrB:Y, reciprocal    chrA[:X] + chrB[Y:]   and   chrB[:Y] + chrA[X:]
  (ii)  chrB:U  -> chrC:V                chrB[:U] + chrC[V:]
  (iii) chrC:W  -> chrA:Z                chrC[:W] + NT + chrA[Z:]        (a few non-template bases)

X and Z are three windows apart on chrA; Y and U share a window of chrB; V and W share a window of chrC.

Around every junction 100-bp read pairs (insert 300 +- 15) are drawn from the derivative and 'aligned' by construction:
  * spanning pairs: the '+' mate wholly left of the junction, the '-' mate wholly right of it; both mapped, each record
    pointing at its mate on the other chromosome (the discordant pairs -I clusters);
  * split reads: one mate across the junction (unmapped, stored as sequenced, at its anchor's position), the other mapped
    on one side: '+' anchors left of the junction, '-' anchors right of it.
No two records of a kind share a position, so the unstable sort of the reference cannot matter.  One split-read name is
used twice on purpose (the reference reports a name once per window).

A split read whose far part Pindel would also find by chance next to its anchor (a dozen bases of random sequence do occur
within a few insert sizes) is not generated: the CPU oracle is asked, without any window hint, and the read is left out when
it reports a far end.  So without hints no junction read has a far end, and the ordinary reports of a run do not depend on
whether the junctions' windows were searched.  A 40-base deletion on chrA (DEL_AT, in a window without a junction) with
split reads of its own gives those reports something to hold."""
import os
import random

from oracle import pyoracle
from pindel_amd import hostio
from tests import bam_writer as bw

READ, ISZ, JITTER = 100, 300, 15
TAG = "SYN"
CHR_LEN = 100_000
WINDOW = 20_000
WINDOW_MBP = "0.02"
NAMES = ("chrA", "chrB", "chrC")
X, Y = 30_000, 50_000          # (i)
U, V = 45_000, 70_000          # (ii)
W, Z = 65_000, 90_000          # (iii)
NT = "ACGTTGCA"
DEL_AT, DEL_LEN = 50_000, 40   # chrA[:DEL_AT] + chrA[DEL_AT + DEL_LEN:]
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def revcomp(s):
    return "".join(_COMP[c] for c in reversed(s))


def junctions():
    """(left chromosome index, position, non-template bases, right chromosome index, position) per derivative"""
    return [(0, X, "", 1, Y), (1, Y, "", 0, X), (1, U, "", 2, V), (2, W, NT, 0, Z)]


def make(d, seed=23, n_spanning=15, split_step=4):
    """Writes d/interchr.fa (+ .fai), d/interchr.bam (+ .bai), d/config, d/reads.txt (the split reads as Pindel text) and
    d/ctx.bd (a BreakDancer file with the three junctions).  Returns a dict with the paths, the chromosomes, the BAM
    records and, per derivative, the numbers of spanning pairs and of split reads per anchor strand."""
    rng = random.Random(seed)
    chroms = ["".join(rng.choice("ACGT") for _ in range(CHR_LEN)) for _ in NAMES]
    fasta = os.path.join(d, "interchr.fa")
    with open(fasta, "w") as fh, open(fasta + ".fai", "w") as fai:
        at = 0
        for n, s in zip(NAMES, chroms):
            fh.write(f">{n}\n")
            at += len(n) + 2
            fai.write(f"{n}\t{len(s)}\t{at}\t60\t61\n")
            for i in range(0, len(s), 60):
                fh.write(s[i:i + 60] + "\n")
            at += len(s) + (len(s) + 59) // 60
    padded = [q for _, q in hostio.load_fasta(fasta)]
    oracle_params = pyoracle.make_params()

    def chance_far_end(seq, strand, chrom, pos):
        b = hostio.batch_from_lists([seq.encode()], [strand.encode()], [pos], [ISZ], [chrom])
        r = pyoracle.search_batch(oracle_params, padded, b.seq, b.seq_off, b.anchor_strand, b.anchor_pos, b.insert_size, b.chr_id)
        return int(r["far_cnt"][0]) > 0
    F = bw.FLAG
    recs, text, counts = [], [], []
    serial = [0]
    dup_pending = [True]

    def name(prefix):
        serial[0] += 1
        return f"{prefix}{serial[0]}"

    for lc, p, nt, rc, q in junctions() + [(0, DEL_AT, "", 0, DEL_AT + DEL_LEN)]:
        is_junction = lc != rc
        der = chroms[lc][:p] + nt + chroms[rc][q:]
        jl, jr = p, p + len(nt)                     # the derivative's junction: [jl, jr) is non-template

        def place(lo):                              # a read [lo, lo + READ) of the derivative -> (tid, pos) or None (across)
            if lo + READ <= jl:
                return lc, lo
            if lo >= jr:
                return rc, q + lo - jr
            return None
        n_span = 0
        # spanning pairs: fragment [f, f + isz), '+' mate at f, '-' mate at f + isz - READ
        for k in range(n_spanning if is_junction else 0):
            f = jl - READ - 5 * k - (k % 3)          # distinct positions on the left ...
            isz = ISZ - JITTER + (7 * k + 3 * len(counts)) % (2 * JITTER + 1)
            g = max(f + isz - READ, jr + 2 * k)      # ... and on the right
            a, b = place(f), place(g)
            assert a is not None and b is not None and a[0] == lc and b[0] == rc
            qn = name("span")
            recs.append(dict(qname=qn, flag=F["PAIRED"] | F["READ1"] | F["MREVERSE"], tid=a[0], pos=a[1], mapq=60, cigar=[(0, READ)],
                             seq=der[f:f + READ], mtid=b[0], mpos=b[1], tlen=0))
            recs.append(dict(qname=qn, flag=F["PAIRED"] | F["READ2"] | F["REVERSE"], tid=b[0], pos=b[1], mapq=60, cigar=[(0, READ)],
                             seq=der[g:g + READ], mtid=a[0], mpos=a[1], tlen=0))
            n_span += 1
        n_plus = n_minus = 0
        # split reads with a '+' anchor: the '-' mate lies across the junction, k of its bases left of it
        for k in range(30, 71, split_step):
            g = jl - k
            f = g + READ - (ISZ + (k % 7) - 3)
            a = place(f)
            assert a is not None and a[0] == lc and place(g) is None
            mate = revcomp(der[g:g + READ])
            if is_junction and chance_far_end(mate, "+", a[0], a[1]):
                continue
            qn = name("split")
            if dup_pending[0] and n_plus == 1:       # the deliberate duplicate: the name of the read before it
                qn, dup_pending[0] = f"split{serial[0] - 1}", False
            recs.append(dict(qname=qn, flag=F["PAIRED"] | F["READ1"] | F["MUNMAP"], tid=a[0], pos=a[1], mapq=60, cigar=[(0, READ)],
                             seq=der[f:f + READ], mtid=a[0], mpos=a[1], tlen=0))
            recs.append(dict(qname=qn, flag=F["PAIRED"] | F["READ2"] | F["UNMAP"], tid=a[0], pos=a[1], mapq=0, cigar=[], seq=mate,
                             mtid=a[0], mpos=a[1], tlen=0))
            text.append((f"@{qn}/2", mate, "+", NAMES[a[0]], a[1], 60, ISZ, TAG))
            n_plus += 1
        # split reads with a '-' anchor: the '+' mate lies across the junction
        for k in range(30, 71, split_step):
            f = jl - k
            g = f + (ISZ + (k % 5) - 2) - READ
            b = place(g)
            assert b is not None and b[0] == rc and place(f) is None
            mate = der[f:f + READ]
            if is_junction and chance_far_end(mate, "-", b[0], b[1] + READ):
                continue
            qn = name("split")
            recs.append(dict(qname=qn, flag=F["PAIRED"] | F["READ2"] | F["MUNMAP"] | F["REVERSE"], tid=b[0], pos=b[1], mapq=60,
                             cigar=[(0, READ)], seq=der[g:g + READ], mtid=b[0], mpos=b[1], tlen=0))
            recs.append(dict(qname=qn, flag=F["PAIRED"] | F["READ1"] | F["UNMAP"] | F["MREVERSE"], tid=b[0], pos=b[1], mapq=0, cigar=[],
                             seq=mate, mtid=b[0], mpos=b[1], tlen=0))
            text.append((f"@{qn}/1", mate, "-", NAMES[b[0]], b[1] + READ, 60, ISZ, TAG))
            n_minus += 1
        if is_junction:
            counts.append(dict(left=NAMES[lc], right=NAMES[rc], spanning=n_span, split_plus=n_plus, split_minus=n_minus))
    # coordinate order; of a split pair the mapped anchor comes first (the order a sorted BAM of such pairs has)
    order = sorted(range(len(recs)), key=lambda i: (recs[i]["tid"], recs[i]["pos"], recs[i]["flag"] & F["UNMAP"], i))
    recs = [recs[i] for i in order]
    bam = os.path.join(d, "interchr.bam")
    bw.write_bam(bam, [(n, CHR_LEN) for n in NAMES], recs)
    config = os.path.join(d, "config")
    with open(config, "w") as fh:
        fh.write(f"interchr.bam {ISZ} {TAG}\n")
    reads_txt = os.path.join(d, "reads.txt")
    chr_rank = {n: i for i, n in enumerate(NAMES)}
    text.sort(key=lambda t: (chr_rank[t[3]], t[4]))
    with open(reads_txt, "w") as fh:
        for nm, seq, strand, chrom, pos, ms, isz, tag in text:
            fh.write(f"{nm}\n{seq}\n{strand}\t{chrom}\t{pos}\t{ms}\t{isz}\t{tag}\n")
    bd_path = os.path.join(d, "ctx.bd")
    with open(bd_path, "w") as fh:
        fh.write("#Chr1\tPos1\tOrientation1\tChr2\tPos2\tOrientation2\tType\tSize\tScore\tnum_Reads\n")
        for (c1, p1, c2, p2) in ((0, X, 1, Y), (1, U, 2, V), (2, W, 0, Z)):
            fh.write(f"{NAMES[c1]}\t{p1}\t10+0-\t{NAMES[c2]}\t{p2}\t0+10-\tCTX\t-300\t99\t10\n")
    return dict(fasta=fasta, bam=bam, config=config, reads_txt=reads_txt, bd=bd_path, chroms=list(zip(NAMES, chroms)), records=recs,
                text=text, counts=counts)


def windows(chr_len=CHR_LEN, window=WINDOW):
    """the windows `pindel_pg -i` walks on one whole chromosome: [ws, we) from 0 in steps of the window while ws <= the end"""
    out, ws = [], 0
    while not ws > chr_len:
        out.append((ws, min(ws + window, chr_len)))
        ws += window
    return out
