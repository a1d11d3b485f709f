"""pindel_pg --device-classifier --device-classifier-hints: hinted windows on the device-classifier path -- the
window's BreakDancer region as one table, pg_device_batch_search_table in place of the fused search, everything after it as in 7o.
The reports must be the bytes of the run without the two flags, on Pindel-text input with --bd-hints on and on BAM input with -R
on, and the hints must have been searched: a long deletion that no read reaches without them is in _D.

The sample is built here, in the style of tests/interchr_synth.py: one chromosome of 100 kb (five windows at -w 0.02), a 40-base
deletion with split reads of its own, a 30 kb deletion with split reads on both sides -- none of which the CPU oracle gives a far
end without hints -- discordant pairs across it (and a decoy cluster below it: the reference's Summarize never reports the last
group it looks at, the one with the smallest coordinate) and a BreakDancer file that names it."""
import os
import random
import re

import pytest

from oracle import pyoracle
from pindel_amd import hostio
from tests import bam_writer as bw
from tests import golden_util as gu
from tests import interchr_synth as syn
from tests.test_gpu_device_classifier_cli import EXE, LINE, TIMEOUT

import subprocess

pytestmark = pytest.mark.gpu

READ, ISZ = 100, 300
TAG = "SYN"
CHR, CHR_LEN = "chrL", 100_000
WINDOW_MBP = "0.02"
SMALL_AT, SMALL_LEN = 30_000, 40
LONG_AT, LONG_END = 50_000, 80_000                  # the long deletion: [LONG_AT, LONG_END) is gone
DECOY_AT, DECOY_END = 42_000, 85_000                # discordant pairs only: no split read lies near either side
HINTED = ("--device-classifier", "--device-classifier-hints")


def make(d, seed=29):
    rng = random.Random(seed)
    chrom = "".join(rng.choice("ACGT") for _ in range(CHR_LEN))
    fasta = os.path.join(d, "long_del.fa")
    with open(fasta, "w") as fh, open(fasta + ".fai", "w") as fai:
        fh.write(f">{CHR}\n")
        fai.write(f"{CHR}\t{CHR_LEN}\t{len(CHR) + 2}\t60\t61\n")
        for i in range(0, CHR_LEN, 60):
            fh.write(chrom[i:i + 60] + "\n")
    padded = [q for _, q in hostio.load_fasta(fasta)]
    oracle_params = pyoracle.make_params()

    def chance_far_end(seq, strand, pos):
        b = hostio.batch_from_lists([seq.encode()], [strand.encode()], [pos], [ISZ], [0])
        r = pyoracle.search_batch(oracle_params, padded, b.seq, b.seq_off, b.anchor_strand, b.anchor_pos, b.insert_size, b.chr_id)
        return int(r["far_cnt"][0]) > 0
    F = bw.FLAG
    recs, text = [], []
    serial = [0]
    n_long = 0

    def name(prefix):
        serial[0] += 1
        return f"{prefix}{serial[0]}"

    for p, q in ((SMALL_AT, SMALL_AT + SMALL_LEN), (LONG_AT, LONG_END)):
        is_long = q - p > 1000
        der = chrom[:p] + chrom[q:]

        def place(lo):                              # a read [lo, lo + READ) of the derivative -> its position, or None (across)
            if lo + READ <= p:
                return lo
            if lo >= p:
                return q + lo - p
            return None
        # split reads with a '+' anchor: the '-' mate lies across the junction, k of its bases left of it
        for k in range(30, 71, 4):
            g = p - k
            f = g + READ - (ISZ + (k % 7) - 3)
            a = place(f)
            assert a is not None and place(g) is None
            mate = syn.revcomp(der[g:g + READ])
            if is_long and chance_far_end(mate, "+", a):
                continue
            qn = name("split")
            recs.append(dict(qname=qn, flag=F["PAIRED"] | F["READ1"] | F["MUNMAP"], tid=0, pos=a, mapq=60, cigar=[(0, READ)],
                             seq=der[f:f + READ], mtid=0, mpos=a, tlen=0))
            recs.append(dict(qname=qn, flag=F["PAIRED"] | F["READ2"] | F["UNMAP"], tid=0, pos=a, mapq=0, cigar=[], seq=mate,
                             mtid=0, mpos=a, tlen=0))
            text.append((f"@{qn}/2", mate, "+", CHR, a, 60, ISZ, TAG))
            n_long += is_long
        # split reads with a '-' anchor: the '+' mate lies across the junction
        for k in range(30, 71, 4):
            f = p - k
            g = f + (ISZ + (k % 5) - 2) - READ
            b = place(g)
            assert b is not None and place(f) is None
            mate = der[f:f + READ]
            if is_long and chance_far_end(mate, "-", b + READ):
                continue
            qn = name("split")
            recs.append(dict(qname=qn, flag=F["PAIRED"] | F["READ2"] | F["MUNMAP"] | F["REVERSE"], tid=0, pos=b, mapq=60,
                             cigar=[(0, READ)], seq=der[g:g + READ], mtid=0, mpos=b, tlen=0))
            recs.append(dict(qname=qn, flag=F["PAIRED"] | F["READ1"] | F["UNMAP"] | F["MREVERSE"], tid=0, pos=b, mapq=0, cigar=[],
                             seq=mate, mtid=0, mpos=b, tlen=0))
            text.append((f"@{qn}/1", mate, "-", CHR, b + READ, 60, ISZ, TAG))
            n_long += is_long
    assert n_long >= 12
    # discordant pairs: the '+' mate left of the deletion, the '-' mate right of it (tests/test_bam_ingest.py's shape), eight per cluster
    for a, b in ((LONG_AT, LONG_END), (DECOY_AT, DECOY_END)):
        for k in range(8):
            pa, pb = a - 350 + 23 * k, b + 50 + 19 * k
            qn = name("span")
            recs.append(dict(qname=qn, flag=F["PAIRED"] | F["READ1"] | F["MREVERSE"], tid=0, pos=pa, mapq=60, cigar=[(0, READ)],
                             seq=chrom[pa:pa + READ], mtid=0, mpos=pb, tlen=pb - pa + READ))
            recs.append(dict(qname=qn, flag=F["PAIRED"] | F["READ2"] | F["REVERSE"], tid=0, pos=pb, mapq=60, cigar=[(0, READ)],
                             seq=chrom[pb:pb + READ], mtid=0, mpos=pa, tlen=-(pb - pa + READ)))
    order = sorted(range(len(recs)), key=lambda i: (recs[i]["pos"], recs[i]["flag"] & F["UNMAP"], i))
    recs = [recs[i] for i in order]
    bw.write_bam(os.path.join(d, "long_del.bam"), [(CHR, CHR_LEN)], recs)
    config = os.path.join(d, "config")
    with open(config, "w") as fh:
        fh.write(f"long_del.bam {ISZ} {TAG}\n")
    reads_txt = os.path.join(d, "reads.txt")
    text.sort(key=lambda t: t[4])
    with open(reads_txt, "w") as fh:
        for nm, seq, strand, chrom_name, pos, ms, isz, tag in text:
            fh.write(f"{nm}\n{seq}\n{strand}\t{chrom_name}\t{pos}\t{ms}\t{isz}\t{tag}\n")
    bd_path = os.path.join(d, "del.bd")
    with open(bd_path, "w") as fh:
        fh.write("#Chr1\tPos1\tOrientation1\tChr2\tPos2\tOrientation2\tType\tSize\tScore\tnum_Reads\n")
        fh.write(f"{CHR}\t{LONG_AT}\t10+0-\t{CHR}\t{LONG_END}\t0+10-\tDEL\t{LONG_END - LONG_AT}\t99\t10\n")
    return dict(fasta=fasta, config=config, reads_txt=reads_txt, bd=bd_path, n_long=n_long)


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dc_hints_cli")
    s = make(str(tmp))
    s["tmp"] = tmp
    return s


@pytest.fixture(scope="module")
def interchr(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dc_hints_interchr")
    s = syn.make(str(tmp))
    s["tmp"] = tmp
    return s


def run(s, name, *args):
    prefix = str(s["tmp"] / name)
    out = subprocess.run([EXE, "-f", s["fasta"], "-o", prefix, "-T", "2", "-w", WINDOW_MBP, *args], capture_output=True, text=True,
                         timeout=TIMEOUT, cwd=str(s["tmp"]))
    return out, prefix


def reports(prefix, suffixes=gu.SUFFIXES):
    return {suf: open(f"{prefix}_{suf}", "rb").read() for suf in suffixes}


def summary(out):
    m = LINE.search(out.stdout)
    assert m, out.stdout[-2000:]
    d = dict(zip(("windows", "tables", "fallbacks", "unresolved", "records", "runs_kept"), (int(x) for x in m.groups())))
    h = re.search(r"runs not downloaded, (\d+) hinted windows$", out.stdout, re.M)
    d["hinted"] = int(h.group(1)) if h else None
    return d


def deletion_sizes(prefix):
    sizes = []
    for line in open(prefix + "_D"):
        f = line.split("\t")
        if len(f) > 5 and f[1].startswith("D "):
            sizes.append(int(f[1].split()[1]))
    return sizes


LONG = LONG_END - LONG_AT


def test_text_route(sample):
    s = sample
    text = ("-p", s["reads_txt"], "-b", s["bd"])
    plain, p_prefix = run(s, "text_plain", *text, "--bd-hints", "on")
    flagged, f_prefix = run(s, "text_dc", *text, "--bd-hints", "on", *HINTED)
    unhinted, u_prefix = run(s, "text_unhinted", *text)
    for o in (plain, flagged, unhinted):
        assert o.returncode == 0, o.stderr[-2000:]
    assert reports(f_prefix) == reports(p_prefix)
    # the hints were searched: the long deletion is called with them and not without
    assert LONG in deletion_sizes(p_prefix) and LONG in deletion_sizes(f_prefix) and LONG not in deletion_sizes(u_prefix)
    assert SMALL_LEN in deletion_sizes(f_prefix) and SMALL_LEN in deletion_sizes(u_prefix)
    n_plain, n_flagged = plain.stdout.count("Window hints: device lookup"), flagged.stdout.count("Window hints: device lookup")
    assert n_flagged == n_plain >= 1 and "Window hints" not in unhinted.stdout
    sm = summary(flagged)
    assert sm["windows"] > 0 and sm["tables"] == sm["windows"] and sm["fallbacks"] == 0 and sm["hinted"] == n_flagged
    assert "device classifier" not in plain.stdout
    count = lambda o: re.findall(r"^(Total: \d+;\tClose_end_found \d+;\tFar_end_found \d+;)", o.stdout, re.M)
    assert count(flagged) == count(plain) and count(plain) != count(unhinted)
    # lists cut to nothing: every window with a pair fetches its points (both lists are resident) and takes the existing path
    cut, c_prefix = run(s, "text_dc0", *text, "--bd-hints", "on", *HINTED, "--device-classifier-listed", "0")
    assert cut.returncode == 0, cut.stderr[-2000:]
    assert reports(c_prefix) == reports(p_prefix) and summary(cut)["fallbacks"] > 0


def test_bam_route(sample):
    s = sample
    bam = ("-i", s["config"])
    plain, p_prefix = run(s, "bam_plain", *bam)
    flagged, f_prefix = run(s, "bam_dc", *bam, *HINTED)
    no_rp, n_prefix = run(s, "bam_no_rp", *bam, "-R", "false")
    for o in (plain, flagged, no_rp):
        assert o.returncode == 0, o.stderr[-2000:]
    assert reports(f_prefix) == reports(p_prefix)
    rp = reports(f_prefix, ("RP",))["RP"]
    assert rp == reports(p_prefix, ("RP",))["RP"] and len(rp) > 0
    assert LONG in deletion_sizes(p_prefix) and LONG in deletion_sizes(f_prefix) and LONG not in deletion_sizes(n_prefix)
    line = re.search(r"read-pair events added as window hints: \d+", plain.stdout)
    assert line and line.group(0) in flagged.stdout
    n_plain, n_flagged = plain.stdout.count("Window hints: device lookup"), flagged.stdout.count("Window hints: device lookup")
    assert n_flagged == n_plain >= 1
    sm = summary(flagged)
    assert sm["windows"] > 0 and sm["tables"] + sm["fallbacks"] == sm["windows"] and sm["hinted"] == n_flagged


def test_far_ends_on_other_chromosomes(interchr):
    """tests/interchr_synth.py's sample without -I, text route: the hinted windows lie on other chromosomes"""
    s = interchr
    text = ("-p", s["reads_txt"], "-b", s["bd"], "--bd-hints", "on")
    plain, p_prefix = run(s, "ctx_plain", *text)
    flagged, f_prefix = run(s, "ctx_dc", *text, *HINTED)
    assert plain.returncode == 0 and flagged.returncode == 0, (plain.stderr[-2000:], flagged.stderr[-2000:])
    assert reports(f_prefix) == reports(p_prefix)
    assert syn.DEL_LEN in deletion_sizes(f_prefix)
    n = flagged.stdout.count("Window hints: device lookup")
    assert n == plain.stdout.count("Window hints: device lookup") >= 3 and summary(flagged)["hinted"] == n
    count = lambda o: re.findall(r"^(Total: \d+;\tClose_end_found \d+;\tFar_end_found \d+;)", o.stdout, re.M)
    assert count(flagged) == count(plain)


def test_refusals_with_the_switch(sample):
    s = sample
    text = ("-p", s["reads_txt"], "-b", s["bd"], "--bd-hints", "on")
    out, prefix = run(s, "refused_I", *text, *HINTED, "-I")
    assert out.returncode == 2 and "--device-classifier" in out.stderr and "with -I:" in out.stderr, out.stderr
    assert not any(os.path.exists(f"{prefix}_{suf}") for suf in gu.SUFFIXES)
    out, prefix = run(s, "refused_alone", *text, "--device-classifier-hints")
    assert out.returncode == 2 and "--device-classifier-hints needs --device-classifier" in out.stderr, out.stderr
    assert not any(os.path.exists(f"{prefix}_{suf}") for suf in gu.SUFFIXES)
