"""Fixtures of the -N (--NormalSamples) tests: an independent restatement of Pindel's read-depth arithmetic
(src/bam2depth.cpp) and a two-sample synthetic with planted tandem duplications and inversions (tests/bam_writer.py),
in the style of interchr_synth.py.

The restatement walks the pileup the way the reference does, position by position: depth[p] = the number of kept
records with an M / = / X base at p.  (The code under test adds up CIGAR blocks cut to the region instead.)

The synthetic: one chromosome chrG of CHR_LEN random bases, two samples S1 and S2, one BAM each.  Both BAMs are tiled
with fully matching 100-bp reads every STEP bases (depth READ / STEP = 50); sample S1 has a second tiling over TD_a.
Five events, each with split reads in both samples (an anchor mapped outside the event's junction, its mate unmapped
across it):

  TD_a   1 kb   S1's depth doubled over the duplication    -> -N keeps it (2 BAMs measured, 1 good: n - good <= 1)
  TD_b   1 kb   flat depth                                 -> -N drops it
  TD_c   150 bp flat depth                                 -> kept: shorter than two reads, never measured
  INV_s  150 bp                                            -> kept: shorter than two reads
  INV_l  1 kb                                              -> dropped (no read pair can be counted)

A 1-kb far end lies beyond the default search range (-x 2: 512 bases), so the runs on this sample use -x 3."""
import os
import random

import numpy as np

from tests import bam_writer as bw

F = bw.FLAG
READ, ISZ, STEP = 100, 300, 2
CHR, CHR_LEN = "chrG", 20_000
TAGS = ("S1", "S2")
MAX_RANGE_INDEX = 3
# name -> (kind, start, end): the duplicated / inverted segment is [start, end) (0-based)
EVENTS = {"TD_a": ("TD", 3000, 4000), "TD_b": ("TD", 7000, 8000), "TD_c": ("TD", 10000, 10150),
          "INV_s": ("INV", 12000, 12150), "INV_l": ("INV", 15000, 16000)}
DROPPED = ("TD_b", "INV_l")
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
_SKIP = F["UNMAP"] | F["SECONDARY"] | F["QCFAIL"] | F["DUP"]


def revcomp(s):
    return "".join(_COMP[c] for c in reversed(s))


# ---------------------------------------------------------------------------------------------- the restatement
def depth_array(records, tid, length):
    """per position of reference `tid`: kept records with an M / = / X base there (int64)"""
    depth = np.zeros(length, dtype=np.int64)
    for r in records:
        if r["tid"] != tid or r["flag"] & _SKIP or not r.get("cigar"):
            continue
        at = r["pos"]
        for op, n in r["cigar"]:
            if op in (0, 7, 8):
                for p in range(max(at, 0), min(at + n, length)):
                    depth[p] += 1
                at += n
            elif op in (2, 3):
                at += n
    return depth


def avg_depth(depth, beg, end):
    """(double)sum / (end - beg) with IEEE division: NaN for an empty region (bam2depth.cpp:93)"""
    total = int(depth[max(beg, 0):max(min(end, len(depth)), 0)].sum()) if end > beg else 0
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(total) / np.float64(end - beg))


def ratio(depth, size, start, end):
    """getRelativeCoverageInternal for one BAM"""
    L = end - start
    before = avg_depth(depth, max(start - L, 0), start)
    sv = avg_depth(depth, start, end)
    after = avg_depth(depth, end, min(end + L, size))
    if before + after == 0:
        return -1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(2) * (np.float64(2) * np.float64(sv)) / (np.float64(before) + np.float64(after)))


def rule_td(ratios):
    """IsGoodTD on the ratios of the measured BAMs (reporter.cpp:1141-1152); the last comparison is in single precision"""
    n, good = len(ratios), sum(1 for r in ratios if r >= 2.7)
    return (n == 1 and good == 1) or (1 < n <= 4 and n - good <= 1) or (n > 4 and np.float32(good) / np.float32(n) > 0.66)


# ---------------------------------------------------------------------------------------------- the synthetic
def _derivative(ref, kind, a, b):
    """the sample's sequence around the event and its junctions: [(position in the derivative, left side maps as
    lo -> lo + dl, right side as lo -> lo + dr)]; only the sides outside the rearranged segment are used for anchors"""
    if kind == "TD":
        return ref[:b] + ref[a:], [(b, 0, a - b)]
    return ref[:a] + revcomp(ref[a:b]) + ref[b:], [(a, 0, None), (b, None, 0)]


def make(d, seed=41):
    """Writes d/germline.fa (+ .fai), d/S1.bam, d/S2.bam (+ .bai), d/config and d/reads.txt (the split reads as the BAM
    ingest delivers them, S1's then S2's).  Returns a dict with the paths, the reference, the records per sample and the
    text reads."""
    rng = random.Random(seed)
    ref = "".join(rng.choice("ACGT") for _ in range(CHR_LEN))
    fasta = os.path.join(d, "germline.fa")
    with open(fasta, "w") as fh, open(fasta + ".fai", "w") as fai:
        fh.write(f">{CHR}\n")
        fai.write(f"{CHR}\t{CHR_LEN}\t{len(CHR) + 2}\t60\t61\n")
        for i in range(0, CHR_LEN, 60):
            fh.write(ref[i:i + 60] + "\n")
    recs = {t: [] for t in TAGS}
    text = {t: {} for t in TAGS}
    for t in TAGS:                                   # the flat tiling
        for k, p in enumerate(range(0, CHR_LEN - READ + 1, STEP)):
            recs[t].append(dict(qname=f"{t}cov{k}", flag=0, tid=0, pos=p, mapq=60, cigar=[(0, READ)], seq=ref[p:p + READ]))
    a, b = EVENTS["TD_a"][1:]
    for k, p in enumerate(range(a - READ // 2, b - READ // 2, STEP)):      # S1's second copy of TD_a
        recs["S1"].append(dict(qname=f"S1dup{k}", flag=0, tid=0, pos=p, mapq=60, cigar=[(0, READ)], seq=ref[p:p + READ]))
    serial = 0
    for ev, (kind, a, b) in EVENTS.items():
        der, juncs = _derivative(ref, kind, a, b)
        for j, dl, dr in juncs:
            for n, k in enumerate(range(30, 71, 4)):
                t = TAGS[n % 2]
                if dl is not None:                   # '+' anchor left of the junction, its '-' mate across it
                    g = j - k
                    f = g + READ - (ISZ + (k % 7) - 3)
                    serial += 1
                    qn, pos, mate = f"{ev}_{serial}", f + dl, revcomp(der[g:g + READ])
                    recs[t].append(dict(qname=qn, flag=F["PAIRED"] | F["READ1"] | F["MUNMAP"], tid=0, pos=pos, mapq=60,
                                        cigar=[(0, READ)], seq=der[f:f + READ], mtid=0, mpos=pos, tlen=0))
                    recs[t].append(dict(qname=qn, flag=F["PAIRED"] | F["READ2"] | F["UNMAP"], tid=0, pos=pos, mapq=0, cigar=[],
                                        seq=mate, mtid=0, mpos=pos, tlen=0))
                    text[t][qn] = (f"@{qn}/2", mate, "+", CHR, pos, 60, ISZ, t)
                if dr is not None:                   # '-' anchor right of the junction, its '+' mate across it
                    f = j - k
                    g = f + (ISZ + (k % 5) - 2) - READ
                    serial += 1
                    qn, pos, mate = f"{ev}_{serial}", g + dr, der[f:f + READ]
                    recs[t].append(dict(qname=qn, flag=F["PAIRED"] | F["READ2"] | F["MUNMAP"] | F["REVERSE"], tid=0, pos=pos,
                                        mapq=60, cigar=[(0, READ)], seq=der[g:g + READ], mtid=0, mpos=pos, tlen=0))
                    recs[t].append(dict(qname=qn, flag=F["PAIRED"] | F["READ1"] | F["UNMAP"] | F["MREVERSE"], tid=0, pos=pos,
                                        mapq=0, cigar=[], seq=mate, mtid=0, mpos=pos, tlen=0))
                    text[t][qn] = (f"@{qn}/1", mate, "-", CHR, pos + READ, 60, ISZ, t)
    bams, reads = {}, []
    for t in TAGS:
        order = sorted(range(len(recs[t])), key=lambda i: (recs[t][i]["pos"], recs[t][i]["flag"] & F["UNMAP"], i))
        recs[t] = [recs[t][i] for i in order]
        bams[t] = os.path.join(d, f"{t}.bam")
        bw.write_bam(bams[t], [(CHR, CHR_LEN)], recs[t])
        reads += [text[t][r["qname"]] for r in recs[t] if r["flag"] & F["UNMAP"]]
    config = os.path.join(d, "config")
    with open(config, "w") as fh:
        for t in TAGS:
            fh.write(f"{t}.bam {ISZ} {t}\n")
    reads_txt = os.path.join(d, "reads.txt")
    with open(reads_txt, "w") as fh:
        for nm, seq, strand, chrom, pos, ms, isz, tag in reads:
            fh.write(f"{nm}\n{seq}\n{strand}\t{chrom}\t{pos}\t{ms}\t{isz}\t{tag}\n")
    return dict(fasta=fasta, bams=bams, config=config, reads_txt=reads_txt, ref=ref, records=recs, text=reads)


# ---------------------------------------------------------------------------------------------- reports
def blocks(data):
    """a _TD / _INV report cut into its events: [(event number, BP left, BP right, bytes of the block)]"""
    out = []
    for chunk in data.split(b"#" * 100 + b"\n")[1:]:
        head = chunk.split(b"\n", 1)[0].split(b"\t")
        at = head.index(next(x for x in head if x.startswith(b"BP ")))
        out.append((int(head[0]), int(head[at].split(b" ")[1]), int(head[at + 1]), chunk))
    return out


def planted(block):
    """the planted event a block reports (its breakpoints within 10 bases of the segment's ends), or None"""
    for name, (_, a, b) in EVENTS.items():
        if abs(block[1] - a) <= 10 and abs(block[2] - b) <= 10:
            return name
    return None


def without(data, dropped):
    """the report without the blocks of the `dropped` planted events, the later event numbers lowered"""
    out, n = b"", 0
    for blk in blocks(data):
        if planted(blk) in dropped:
            continue
        num, rest = blk[3].split(b"\t", 1)
        out += b"#" * 100 + b"\n" + str(n).encode() + b"\t" + rest
        n += 1
    return out
