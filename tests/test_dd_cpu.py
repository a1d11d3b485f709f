"""-q (dispersed duplications) on the host: the C++ containment test against an independent Python restatement, the
discordant reads / clusters / breakpoint estimates of the reference's own MEI demo against a restatement, and the new flags."""
import os
import random
import subprocess

import pytest

from oracle import pyoracle
from tests import dd_restated as R
from tests.test_mei_bam import BAM, ISZ, _decode_bam, _unpack

MM = [int(x) for x in pyoracle.max_mismatch_table()[:500]]
IUPAC = "MRWSYKVHDB"


def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _mutate(rng, s, rate, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) if rng.random() < rate else c for c in s)


def contains_cases(seed=7, n_random=1600):
    """Random and crafted (query, window) pairs; the windows are what a chromosome substring can hold (ACGTN)."""
    rng = random.Random(seed)
    cases = []
    for k in range(n_random):
        d = rng.choice([1, 2, 5, 16, 40, 90, 160, 260])
        db = _rand(rng, d)
        kind = k % 8
        if kind == 0:
            q = _rand(rng, rng.randint(15, 40))
        elif kind in (1, 2) and d >= 20:
            a = rng.randint(0, d - 15)
            q = _mutate(rng, db[a:a + rng.randint(15, min(60, d - a))], 0.06 * (kind - 1))
        elif kind == 3 and d >= 20:
            a = rng.randint(0, d - 15)
            q = R.revcomp(_mutate(rng, db[a:a + rng.randint(15, min(60, d - a))], 0.04))     # true only on the reverse strand
        elif kind == 4:
            db = "N" * rng.randint(0, d) + db[:max(0, d - 1)]                               # a window that starts in the spacer
            q = "N" * rng.randint(0, 20) + _rand(rng, rng.randint(5, 20))
        elif kind == 5:
            q = _mutate(rng, db[:30] if d >= 30 else _rand(rng, 30), 0.1, "ACGT" + IUPAC)     # IUPAC letters in the query
        elif kind == 6:
            q = _rand(rng, rng.randint(15, 25), "AC")
            db = _rand(rng, d, "AC")
        else:
            base = _rand(rng, 18)
            q = _mutate(rng, base + _rand(rng, rng.randint(0, 12)), 0.12)
            db = _rand(rng, rng.randint(0, 10)) + base + _rand(rng, rng.randint(0, 30))
        cases.append((q, db))
    # long queries (up to 499) and long windows (to 2 x 10^5) with a match found early
    for L in (64, 65, 128, 499):
        db = _rand(rng, 600)
        cases.append((_mutate(rng, db[10:10 + L], 0.02) if L < 500 else db[:L], db))
        cases.append((_rand(rng, L), db[:300]))
    for d in (20000, 200000):
        db = _rand(rng, d)
        cases.append((db[5:40], db))
        cases.append((R.revcomp(db[d - 60:d - 20]), db))
    return cases


def test_host_containment_equals_the_python_restatement():
    cases = contains_cases()
    assert len(cases) >= 2000 - 400                     # (+ the block below: >= 2000 in all)
    extra_rng = random.Random(11)
    for _ in range(400):
        db = _rand(extra_rng, extra_rng.randint(15, 60))
        cases.append((_mutate(extra_rng, db[:extra_rng.randint(15, len(db))], 0.15), db))
    got = R.cpu_contains([q for q, _ in cases], [d for _, d in cases], MM)
    classes = {"true": 0, "false": 0, "v==f": 0, "v==f+1": 0, "reverse_only": 0, "empty_window": 0, "iupac": 0, "n_window": 0}
    for (q, db), g in zip(cases, got):
        want, v, f = R.contains_vf(q, db, MM)
        any_strand = want or R.contains_vf(R.revcomp(q), db, MM)[0]
        assert bool(g) == any_strand, (q, db[:80], len(db))
        classes["true" if any_strand else "false"] += 1
        classes["v==f"] += v is not None and v == f
        classes["v==f+1"] += v is not None and f is not None and v == f + 1
        classes["reverse_only"] += any_strand and not want
        classes["empty_window"] += len(db) <= 1
        classes["iupac"] += any(c in IUPAC for c in q)
        classes["n_window"] += db.startswith("N")
    print(classes)
    assert len(cases) >= 2000
    # v == f and v == f + 1 cannot happen: a valid cell has al >= 15 > 15 - g_maxMismatch[15] - (Q-i-1), so its row never gives
    # up, and al grows by at most one per row, so a row after one that gave up reaches at most 15 - g_maxMismatch[15] - (Q-i-1)
    # <= 15 only on the last row.  The restatement confirms it on every case; the kernel's rule v <= f is checked regardless.
    assert classes.pop("v==f") == 0 and classes.pop("v==f+1") == 0
    for k, n in classes.items():
        assert n > 0, (k, classes)


def test_demo_discordant_reads_clusters_and_estimates_equal_the_restatement(tmp_path):
    """runme line 1 of demo/simulated_MEI without split reads (no close ends): every breakpoint is the estimate from its cluster."""
    d = _unpack(tmp_path)
    refs, recs = _decode_bam(BAM)
    n_disc, clusters, est = R.restated_breakpoint_estimates(recs, len(refs), ISZ)
    assert n_disc == [38, 38]
    assert [len(c) for c in clusters] == [19, 19, 19, 19]
    stats, bps, _ = R.dd_run(os.path.join(d, "reference.fa"), os.path.join(d, "config"), os.path.join(d, "est"), MM)
    assert stats[:3] == [76, 4, 4]
    assert [(t, p, s, n) for t, p, s, n, _ in bps] == est
    # chr2: the '+' and '-' estimates lie within MAX_DD_BREAKPOINT_DISTANCE: one event; chr1: about 1 kb apart, none
    assert stats[5] == 1
    dd = open(os.path.join(d, "est_DD")).read().splitlines()
    assert dd[1].split("\t")[:5] == ["1", "DD", "chr2", str(est[2][1]), str(est[3][1])]


def _exe():
    from pindel_amd import binding
    return os.path.join(os.path.dirname(binding.LIB_PATH), "pindel_pg")


@pytest.mark.parametrize("flag,value", [("--MAX_DD_BREAKPOINT_DISTANCE", "350"), ("--MAX_DISTANCE_CLUSTER_READS", "100"),
                                        ("--MIN_DD_CLUSTER_SIZE", "3"), ("--MIN_DD_BREAKPOINT_SUPPORT", "3"),
                                        ("--MIN_DD_MAP_DISTANCE", "8000"), ("--DD_REPORT_DUPLICATION_READS", None), ("-q", None),
                                        ("--detect_DD", "false")])
def test_dd_flags_parse(flag, value):
    """The flags are known: without -f the run stops at the usage line, not at 'unknown argument'; a value flag wants a number."""
    exe = _exe()
    if not os.path.exists(exe):
        pytest.skip("pindel_pg is built by __graft_entry__.build()")
    args = [exe, flag] + ([value] if value else [])
    out = subprocess.run(args, capture_output=True, text=True)
    assert out.returncode == 2 and "usage:" in out.stderr, out.stderr
    if value and value[0].isdigit():
        out = subprocess.run([exe, flag, "x1"], capture_output=True, text=True)
        assert out.returncode == 2 and "is not a number" in out.stderr, out.stderr


SYN_OPTS = (350, 100, 3, 3, 400, 0)          # --MIN_DD_MAP_DISTANCE 400: containment windows of 800 bases


def _split_read_lines(dd_text, header):
    """The split-read block after `header` in a _DD: (reference line, [(aligned text, name)])."""
    lines = dd_text.splitlines()
    k = lines.index(header)
    ref = lines[k + 1][len("# Reference: "):]
    reads = []
    for x in lines[k + 2:]:
        if not x.startswith("#  "):
            break
        body, name = x[2:].split(" (name: ")
        reads.append((body, name.split(" ")[0]))
    return ref, reads


def test_planted_dd_keeps_and_drops_breakpoints_as_the_restatements_say(tmp_path):
    """A synthetic BAM with two planted dispersed duplications (tests/dd_synth.py), oracle close ends: the consensus of the
    first event has no local copy (its breakpoints are kept, with their split reads), the second event's ends were copied next to
    it (its breakpoints are dropped and estimated).  Every containment decision, the kept breakpoints' split reads and their
    consensus are checked against the Python restatements and against what was planted."""
    from pindel_amd import hostio
    from tests import dd_synth
    d = str(tmp_path)
    syn = dd_synth.make(d)
    seqs = [s for _, s in hostio.load_fasta(syn["fasta"])]
    stats, bps, tested = R.dd_run(syn["fasta"], syn["config"], os.path.join(d, "h"), MM, opts=SYN_OPTS,
                                  close_cb=R.oracle_close_cb(seqs))
    assert stats[4] > 0 and stats[3] - stats[4] > 0, stats          # kept and dropped breakpoints
    assert stats[5] == 2
    for tid, pos, strand, n_split, cons, contained in tested:
        start = max(0, pos + 100000 - SYN_OPTS[4])
        window = seqs[tid][start:start + 2 * SYN_OPTS[4]].decode()
        assert R.contains_any_strand(cons, window, MM) == contained, (tid, pos, strand)
        if tid == 1:                                                  # chrB: the planted events
            k = 0 if abs(pos - syn["events"][0][0]) < 10 else 1
            assert abs(pos - syn["events"][k][0]) <= 3
            e = syn["elements"][k]
            # the consensus is the element next to the breakpoint: its start ('+' cluster) or its end ('-' cluster)
            assert (e.find(cons) <= 3) if strand == "+" else (e.rfind(cons) + len(cons) >= len(e) - 3), (strand, cons)
            assert contained == (k == 1)
    dd = open(os.path.join(d, "h_DD")).read()
    assert dd.count("\tDD\tchrB\t") == 2
    # the kept event: its split reads as the report aligns them, their consensus restated, their names all reads across a junction
    tested_b = {(p, s): (n, c) for t, p, s, n, c, x in tested if t == 1 and not x}
    assert len(tested_b) == 2
    for header, strand in (("# Supporting reads for insertion location (5' end):", "+"),
                           ("# Supporting reads for insertion location (3' end):", "-")):
        ref, reads = _split_read_lines(dd, header)
        base = len(ref) - len(ref.lstrip("ACGTN")) if strand == "+" else len(ref) - len(ref.lstrip("acgtn"))
        if strand == "+":
            unmapped = [body[len("Reference: ") + base:] for body, _ in reads]
        else:
            unmapped = [body[len("Reference: "):len("Reference: ") + base].lstrip() for body, _ in reads]
        n, cons = [v for (p, s), v in tested_b.items() if s == strand][0]
        assert len(reads) == n >= 20
        assert R.consensus_unmapped(unmapped, "-" if strand == "+" else "+") == cons
        assert {name for _, name in reads} <= syn["unmapped"]
