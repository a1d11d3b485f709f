"""The synthetic of the `--repair inv-pairs` and `--repair depth-mapq` tests (tests/bam_writer.py), in the style of
germline_synth.py, whose building blocks it uses: one chromosome chrR, two samples S1 and S2, one BAM each, every event
with split reads in both samples.  Under -N (BAM input):

  INV_edge  1 kb    5 '++' entries at its left end, 5 '--' at its right end: exactly the cutoff on each side, and the pair
                    that decides lies LAST in the list (the list is in descending order of position, and nothing lies
                    left of this inversion)                        -> kept by inv-pairs -- only with the comparison after the loop
  INV_both  1 kb    18 '++' and 18 '--' entries                    -> kept by inv-pairs
  INV_one   1 kb    18 '++' entries, no '--'                       -> dropped
  INV_s     150 bp  shorter than two reads: never measured         -> kept
  TD_q      1 kb    S1's depth doubled over it by records of MAPQ 0 and 19, on a flat tiling of MAPQ 60 and 20
                                                                   -> kept as the reference counts, dropped by depth-mapq
Without inv-pairs all three 1-kb inversions are dropped.

An 'entry' is one BAM record of a pair whose mates map to the same strand: read-pair discovery lists every record, so a
pair with both records in the file gives two entries.  The odd counts come from a pair with one record in the file.
IsGoodINV looks at the pairs as ModifyRP left them (the position is the left edge of a box: a '+' end moved left by one
read length, a '-' end by the insert size of the configuration line), so the '--' pairs that count are those of a library
wider than the configuration says: their ends lie 225-300 bases behind the breakpoints.  Every planted position keeps at
least 20 bases from each bound of the loop's conditions, so no breakpoint shift of a few bases decides a count.

Each 1-kb inversion has 5 split reads per breakpoint, so no event has more than 10 reads and the cutoff max(5, support / 2)
is 5 for every one of them."""
import os
import random

from tests import bam_writer as bw
from tests import germline_synth as gs

F = bw.FLAG
READ, ISZ, STEP = gs.READ, gs.ISZ, gs.STEP
CHR, CHR_LEN = "chrR", 24_000
TAGS = ("S1", "S2")
MAX_RANGE_INDEX = gs.MAX_RANGE_INDEX
EVENTS = {"INV_edge": ("INV", 3000, 4000), "INV_both": ("INV", 8000, 9000), "INV_one": ("INV", 13000, 14000),
          "INV_s": ("INV", 17000, 17150), "TD_q": ("TD", 20000, 21000)}
LARGE_INV = ("INV_edge", "INV_both", "INV_one")
ENTRIES = {"INV_edge": (5, 5), "INV_both": (18, 18), "INV_one": (18, 0)}      # '++' entries, '--' entries
CUTOFF = 5
TILED = (18_000, 23_000)                 # the flat tiling: TD_q, its two flanks and a margin
SPLIT_STEP = {"INV": 10, "TD": 4}        # 5 / 11 split reads per junction side


def make(d, seed=59):
    """Writes d/repair.fa (+ .fai), d/S1.bam, d/S2.bam (+ .bai), d/config and d/reads.txt (the split reads as the BAM ingest
    delivers them, S1's then S2's).  Returns the paths, the reference, the records per sample and the text reads."""
    rng = random.Random(seed)
    ref = "".join(rng.choice("ACGT") for _ in range(CHR_LEN))
    fasta = os.path.join(d, "repair.fa")
    with open(fasta, "w") as fh, open(fasta + ".fai", "w") as fai:
        fh.write(f">{CHR}\n")
        fai.write(f"{CHR}\t{CHR_LEN}\t{len(CHR) + 2}\t60\t61\n")
        for i in range(0, CHR_LEN, 60):
            fh.write(ref[i:i + 60] + "\n")
    recs = {t: [] for t in TAGS}
    text = {t: {} for t in TAGS}
    plain = lambda qn, p, q: dict(qname=qn, flag=0, tid=0, pos=p, mapq=q, cigar=[(0, READ)], seq=ref[p:p + READ])
    for t in TAGS:                                   # the flat tiling, MAPQ 60 and 20
        for k, p in enumerate(range(TILED[0], TILED[1] - READ + 1, STEP)):
            recs[t].append(plain(f"{t}cov{k}", p, 20 if k % 3 == 1 else 60))
    a, b = EVENTS["TD_q"][1:]
    for k, p in enumerate(range(a - READ // 2, b - READ // 2, STEP)):      # S1's second copy of TD_q, MAPQ 0 and 19
        recs["S1"].append(plain(f"S1dup{k}", p, 19 if k % 2 else 0))
    # the same-strand pairs: entry i belongs to pair i // 2, its first record (i even) or its mate's (i odd)
    for ev in LARGE_INV:
        _, a, b = EVENTS[ev]
        for side, n in zip("+-", ENTRIES[ev]):
            for i in range(n):
                j = i // 2
                if side == "+":
                    lo, hi, flag = a - 110 - 9 * j, b - 110 - 7 * j, 0
                else:
                    lo, hi, flag = a + 225 + 5 * j, b + 225 + 6 * j, F["REVERSE"] | F["MREVERSE"]
                pos, mpos = (lo, hi) if i % 2 == 0 else (hi, lo)
                recs[TAGS[j % 2]].append(dict(qname=f"{ev}_pair{side}{j}", flag=F["PAIRED"] | (F["READ1"] if i % 2 == 0 else F["READ2"]) | flag,
                                              tid=0, pos=pos, mapq=60, cigar=[(0, READ)], seq=ref[pos:pos + READ], mtid=0, mpos=mpos,
                                              tlen=(hi + READ - lo) * (1 if i % 2 == 0 else -1)))
    serial = 0
    for ev, (kind, a, b) in EVENTS.items():          # the split reads, as germline_synth.make writes them
        der, juncs = gs._derivative(ref, kind, a, b)
        for j, dl, dr in juncs:
            for n, k in enumerate(range(30, 71, SPLIT_STEP[kind])):
                t = TAGS[n % 2]
                if dl is not None:                   # '+' anchor left of the junction, its '-' mate across it
                    g = j - k
                    f = g + READ - (ISZ + (k % 7) - 3)
                    serial += 1
                    qn, pos, mate = f"{ev}_{serial}", f + dl, gs.revcomp(der[g:g + READ])
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
blocks = gs.blocks


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


def inv_event(block):
    """(support, RealStart, RealEnd) of an _INV block as IsGoodINV is given them: the header's `Supports` is the number of
    reads of the event, and it prints BPLeft and BPRight + 2"""
    head = block[3].split(b"\n", 1)[0].split(b"\t")
    support = int(next(x for x in head if x.startswith(b"Supports ")).split(b" ")[1])
    return support, block[1], block[2] - 2
