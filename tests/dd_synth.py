"""A synthetic BAM with planted dispersed duplications for -q (tests/bam_writer.py).

Two chromosomes of random sequence: elements of chrA are inserted into chrB's sample copy, and read pairs (100 bp reads,
400 bp fragments, every few bases) are drawn around each insertion and 'aligned' by construction: a read inside a flank maps to
chrB, a read inside the element maps to chrA at the element's source, a read across a junction is unmapped.  So each
insertion gives a '+' and a '-' cluster of discordant reads on chrB (mates on chrA) and split reads across both junctions.

With a small --MIN_DD_MAP_DISTANCE the containment window is short.  The sequence next to a breakpoint then holds no copy of
the element, and the breakpoint is kept; every event in `dropped` also gets copies of its element's ends planted in chrB near
the insertion, so its consensus IS found there and those breakpoints are dropped (estimated from the clusters instead)."""
import os
import random

from tests import bam_writer as bw
from tests.dd_restated import revcomp

READ, FRAG, STEP = 100, 400, 3
TAG = "SYN"


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def make(d, events=((20000, 10000, 400), (40000, 30000, 400)), dropped=(1,), seed=17, chr_len=60000, copy_at=250):
    """Writes d/synth.fa, d/synth.bam (+ .bai) and d/config.  events: (insertion position on chrB, source on chrA, length).
    Returns dict(fasta, config, chrA, chrB, elements, events, unmapped = the names of the reads across a junction)."""
    rng = random.Random(seed)
    chr_a = _rand(rng, chr_len)
    chr_b = list(_rand(rng, chr_len))
    elements = []
    for k, (p, src, n) in enumerate(events):
        e = chr_a[src:src + n]
        elements.append(e)
        if k in dropped:                     # the element's ends, copied near the insertion (outside the reads' flanks)
            chr_b[p - copy_at - 80:p - copy_at] = list(e[:80])
            chr_b[p + copy_at:p + copy_at + 80] = list(e[-80:])
    chr_b = "".join(chr_b)
    refs = [("chrA", len(chr_a)), ("chrB", len(chr_b))]
    recs = []
    pair = 0
    for (p, src, n), e in zip(events, elements):
        flank = 1000
        seg = chr_b[p - flank:p] + e + chr_b[p:p + flank]

        def place(lo):                       # segment [lo, lo + READ) -> (tid, pos) or None across a junction
            hi = lo + READ
            if hi <= flank:
                return 1, p - flank + lo
            if lo >= flank and hi <= flank + n:
                return 0, src + lo - flank
            if lo >= flank + n:
                return 1, p + lo - flank - n
            return None
        for f in range(0, len(seg) - FRAG + 1, STEP):
            pair += 1
            name = f"p{pair}"
            first_fwd = pair % 2 == 0         # which mate reads the forward strand
            spans = [(f, False), (f + FRAG - READ, True)]      # (segment start, read on the reverse strand)
            mates = []
            for lo, rev in spans:
                fwd_seq = seg[lo:lo + READ]
                mates.append(dict(loc=place(lo), rev=rev, ref_seq=fwd_seq, seq_read=revcomp(fwd_seq) if rev else fwd_seq))
            if mates[0]["loc"] is None and mates[1]["loc"] is None:
                continue
            for i, m in enumerate(mates):
                o = mates[1 - i]
                flag = bw.FLAG["PAIRED"] | (bw.FLAG["READ1"] if (i == 0) == first_fwd else bw.FLAG["READ2"])
                if m["loc"] is None:
                    flag |= bw.FLAG["UNMAP"]
                    tid, pos = o["loc"]
                    seq, cigar = m["seq_read"], []
                else:
                    tid, pos = m["loc"]
                    seq, cigar = m["ref_seq"], [(0, READ)]
                    if m["rev"]:
                        flag |= bw.FLAG["REVERSE"]
                if o["loc"] is None:
                    flag |= bw.FLAG["MUNMAP"]
                    mtid, mpos = tid, pos
                else:
                    mtid, mpos = o["loc"]
                    if o["rev"]:
                        flag |= bw.FLAG["MREVERSE"]
                tlen = 0
                if m["loc"] is not None and o["loc"] is not None and tid == mtid:
                    tlen = (mpos + READ - pos) if pos <= mpos else -(pos + READ - mpos)
                recs.append(dict(qname=name, flag=flag, tid=tid, pos=pos, mapq=60, cigar=cigar, seq=seq, mtid=mtid, mpos=mpos,
                                 tlen=tlen, tags={"RG": "rg1"}))
    unmapped = {"@%s/%d" % (r["qname"], 1 if r["flag"] & bw.FLAG["READ1"] else 2) for r in recs if r["flag"] & bw.FLAG["UNMAP"]}
    recs.sort(key=lambda r: (r["tid"], r["pos"], r["flag"] & bw.FLAG["UNMAP"]))
    bam = os.path.join(d, "synth.bam")
    bw.write_bam(bam, refs, recs, header_text="@HD\tVN:1.6\tSO:coordinate\n@RG\tID:rg1\tSM:planted\n")
    fasta = os.path.join(d, "synth.fa")
    with open(fasta, "w") as fh:
        for name, s in (("chrA", chr_a), ("chrB", chr_b)):
            fh.write(f">{name}\n")
            for i in range(0, len(s), 60):
                fh.write(s[i:i + 60] + "\n")
    config = os.path.join(d, "config")
    with open(config, "w") as fh:
        fh.write(f"synth.bam {FRAG} {TAG}\n")
    return dict(fasta=fasta, config=config, chrA=chr_a, chrB=chr_b, elements=elements, events=list(events), unmapped=unmapped)
