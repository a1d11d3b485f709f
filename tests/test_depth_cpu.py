"""Read depth of a region (hostlib.region_depth, hostlib.depth_ratio: pg_depth.hpp) against the independent restatement in
tests/germline_synth.py, compared exactly (== on the doubles), and -N's rule on the ratios (hostlib.depth_rule_td)."""
import math
import random

import numpy as np
import pytest

from pindel_amd import hostlib
from tests import bam_writer as bw
from tests import germline_synth as gs

F = bw.FLAG
REFS = [("chr1", 5000), ("chr2", 3000)]


def _records():
    """a deliberately messy set: every CIGAR operation, every flag the pileup looks at, MAPQ 0, reads at both ends of chr1"""
    rng = random.Random(5)
    cigars = ["100M", "40M5I55M", "50M10D50M", "30M200N70M", "20S80M", "10H90M", "60=40X", "25M2I3D20M5S", "5S10M1P10M100N30M10D40M5H"]
    flags = [0, 0, 0, F["REVERSE"], F["UNMAP"], F["SECONDARY"], F["QCFAIL"], F["DUP"], 2048, 2048 | F["REVERSE"],
             F["PAIRED"] | F["PROPER"] | F["READ1"], F["SECONDARY"] | 2048]
    recs = []
    for k in range(1500):
        tid = 0 if k % 3 else 1
        cig = bw.cigar_ops(rng.choice(cigars))
        qlen = sum(n for op, n in cig if op in (0, 1, 4, 7, 8))
        span = sum(n for op, n in cig if op in (0, 2, 3, 7, 8))
        recs.append(dict(qname=f"r{k}", flag=rng.choice(flags), tid=tid, pos=rng.randrange(0, REFS[tid][1] - span + 1),
                         mapq=rng.choice([0, 0, 19, 20, 60]), cigar=cig, seq="A" * qlen))
    recs.append(dict(qname="nocigar", flag=0, tid=0, pos=700, mapq=60, cigar=[], seq="A" * 100))      # not piled up
    recs.append(dict(qname="at0", flag=0, tid=0, pos=0, mapq=0, cigar=[(0, 100)], seq="A" * 100))
    recs.append(dict(qname="atend", flag=0, tid=0, pos=4900, mapq=60, cigar=[(0, 100)], seq="A" * 100))
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    return recs


@pytest.fixture(scope="module")
def messy(tmp_path_factory):
    d = tmp_path_factory.mktemp("depth")
    recs = _records()
    paths = dict(indexed=str(d / "indexed.bam"), plain=str(d / "plain.bam"), chr1_only=str(d / "chr1_only.bam"))
    bw.write_bam(paths["indexed"], REFS, recs, block_bytes=4096)           # many BGZF blocks
    bw.write_bam(paths["plain"], REFS, recs, with_index=False)
    only = [r for r in recs if r["tid"] == 0]
    bw.write_bam(paths["chr1_only"], REFS[:1], only)
    depth = {name: gs.depth_array(recs, tid, size) for tid, (name, size) in enumerate(REFS)}
    # the fixture holds what it is meant to: kept records of every operation, and every kind of dropped record
    ops = {op for r in recs if not r["flag"] & gs._SKIP for op, _ in r["cigar"]}
    assert ops == set(range(9))
    assert all(any(r["flag"] & F[f] for r in recs) for f in ("UNMAP", "SECONDARY", "QCFAIL", "DUP")) and any(r["flag"] & 2048 for r in recs)
    assert any(r["mapq"] == 0 and not r["flag"] & gs._SKIP for r in recs)
    return dict(paths=paths, recs=recs, depth=depth)


REGIONS = [(0, 5000), (0, 1), (4999, 5000), (1000, 1001), (1234, 2345), (100, 163), (2500, 2500), (0, 100), (4900, 5000),
           (4950, 5100), (3000, 2900), (17, 4093)]


def test_region_depth_equals_the_restatement(messy):
    for name, size in REFS:
        for beg, end in REGIONS:
            if beg > size:
                continue
            want = gs.avg_depth(messy["depth"][name], beg, end)
            for kind in ("indexed", "plain"):              # with a .bai, and scanned without one
                got = hostlib.region_depth(messy["paths"][kind], name, beg, end)
                assert got == want or (math.isnan(got) and math.isnan(want)), (name, beg, end, kind, got, want)
    # reads straddling beg and end do count, only with their bases inside: the region's sum changes base by base
    d = messy["depth"]["chr1"]
    assert len({gs.avg_depth(d, 1200 + k, 1300) for k in range(5)}) > 1
    assert gs.avg_depth(d, 0, 5000) > 5.0
    # supplementary records count, MAPQ-0 records count: a restatement without them differs
    for drop in (lambda r: r["flag"] & 2048, lambda r: r["mapq"] == 0):
        fewer = gs.depth_array([r for r in messy["recs"] if not drop(r)], 0, 5000)
        assert gs.avg_depth(fewer, 0, 5000) < hostlib.region_depth(messy["paths"]["indexed"], "chr1", 0, 5000)


def test_region_clipped_at_the_chromosome_ends(messy):
    d = messy["depth"]["chr1"]
    p = messy["paths"]["indexed"]
    # the sum only holds positions of the chromosome, the divisor is the region asked for
    assert hostlib.region_depth(p, "chr1", -300, 200) == int(d[:200].sum()) / 500
    assert hostlib.region_depth(p, "chr1", 4800, 5400) == int(d[4800:].sum()) / 600
    assert int(d[:200].sum()) > 0 and int(d[4800:].sum()) > 0


def test_chromosome_missing_from_a_bam_and_unreadable_files(messy, tmp_path):
    assert hostlib.region_depth(messy["paths"]["chr1_only"], "chr2", 0, 3000) == 0.0
    assert hostlib.region_depth(messy["paths"]["chr1_only"], "chr1", 0, 5000) == gs.avg_depth(messy["depth"]["chr1"], 0, 5000)
    assert hostlib.region_depth(messy["paths"]["indexed"], "chrNone", 0, 100) == 0.0
    with pytest.raises(RuntimeError):
        hostlib.region_depth(str(tmp_path / "absent.bam"), "chr1", 0, 100)
    # a BAM cut inside a block is an error, never a smaller depth
    data = open(messy["paths"]["plain"], "rb").read()
    cut = tmp_path / "cut.bam"
    cut.write_bytes(data[:len(data) // 2])
    with pytest.raises(RuntimeError):
        hostlib.region_depth(str(cut), "chr1", 0, 5000)


def test_depth_ratio_equals_the_restatement(messy):
    paths = [messy["paths"]["indexed"], messy["paths"]["chr1_only"], messy["paths"]["plain"]]
    seen_nan = seen_minus1 = 0
    cases = [("chr1", 5000, 2000, 2500), ("chr1", 5000, 100, 900), ("chr1", 5000, 4200, 4900), ("chr1", 5000, 0, 400),
             ("chr1", 5000, 4600, 5000), ("chr1", 5000, 0, 5000), ("chr2", 3000, 1000, 1200), ("chr2", 3000, 500, 900), ("chr2", 3000, 0, 3000),
             ("chr2", 3000, 2999, 3000)]
    for name, size, start, end in cases:
        got = hostlib.depth_ratio(paths, name, size, start, end)
        for k, path in enumerate(paths):
            depth = messy["depth"][name] if not (k == 1 and name == "chr2") else gs.depth_array([], 0, size)
            want = gs.ratio(depth, size, start, end)
            assert got[k] == want or (math.isnan(got[k]) and math.isnan(want)), (name, start, end, k, got[k], want)
            seen_nan += math.isnan(want)
            seen_minus1 += want == -1.0
    assert seen_nan >= 4 and seen_minus1 >= 2
    # a zero-length flank: start 0 (no room before) and end == size (no room after) give 0 / 0; a NaN is never >= 2.7
    assert math.isnan(hostlib.depth_ratio(paths[:1], "chr1", 5000, 0, 400)[0])
    assert math.isnan(hostlib.depth_ratio(paths[:1], "chr1", 5000, 4600, 5000)[0])
    assert not hostlib.depth_rule_td([float("nan")])
    # -1: both flanks without a read (here: the chromosome is not in the BAM, all three depths are 0)
    assert hostlib.depth_ratio(paths[1:2], "chr2", 3000, 1000, 1200) == [-1.0]


def test_ratio_on_a_planted_step():
    """hand-made depths: a flat file gives exactly 2, a doubled event exactly 4; 1.35x is the threshold 2.7"""
    flat = [10] * 3000
    assert gs.ratio(np.array(flat), 3000, 1000, 2000) == 2.0
    assert gs.ratio(np.array([10] * 1000 + [20] * 1000 + [10] * 1000), 3000, 1000, 2000) == 4.0


def test_decision_rule():
    hi, lo = 2.7, 2.6999999999999997            # the two sides of the threshold (>= 2.7 is good)
    cases = [
        ([hi], True), ([lo], False), ([-1.0], False), ([float("nan")], False), ([], False),
        ([hi, hi], True), ([hi, lo], True), ([lo, hi], True), ([lo, lo], False),
        ([hi, hi, hi, lo], True), ([hi, hi, lo, lo], False), ([hi, hi, hi, hi], True), ([lo, -1.0, float("nan"), hi], False),
        ([hi, hi, hi, hi, lo], True), ([hi, hi, hi, lo, lo], False), ([hi] * 5, True),       # 4/5 = 0.8, 3/5 = 0.6
        ([hi, hi, hi, hi, lo, lo], True), ([hi, hi, hi, lo, lo, lo], False),                 # 4/6 = 0.667 > 0.66, 3/6
        ([hi] * 5 + [lo], True), ([3.2, 6.4, 100.0, 2.2, 2.0, 2.71], True),
    ]
    for ratios, want in cases:
        assert hostlib.depth_rule_td(ratios) is want, ratios
        assert bool(gs.rule_td(ratios)) is want, ratios
    assert {len(r) for r, _ in cases} >= {1, 2, 4, 5, 6}
