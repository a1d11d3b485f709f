"""A small synthetic set for the long-insertion tables: a chromosome of 20 kb with a few long insertions of random
sequence, and reads that straddle each junction from both sides -- a stretch of reference up to the junction, then bases of the
insertion -- so that they find a close end and no far end.  Beside them reads of random sequence (no close end) and ordinary
deletion reads (a close and a far end), 100 and 150 bases long.  tests/test_li_tables_cpu.py checks with the oracle and the host
statement that the set yields position pairs the walk reports; tests/test_gpu_li_tables.py searches it on the device."""
import numpy as np

from pindel_amd.hostio import SPACER
from tests import shortening_cases as sc

JUNCTIONS = (SPACER + 5000, SPACER + 9000, SPACER + 13000)
INSERT_SIZE = 500
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def chromosome(seed=77):
    rng = np.random.default_rng(seed)
    return [("chrL", b"N" * SPACER + bytes(rng.choice(_ACGT, size=20000)) + b"N" * SPACER)]


def _rand(rng, n):
    return bytes(rng.choice(_ACGT, size=n))


def junction_read(rng, ref, junction, plus, length):
    """(sequence, strand, anchor position): `keep` reference bases on the anchor's side of the junction, the rest of the insertion,
    in the orientation the close end's first attempt tries (the mate of a '+' anchor is read from the reverse strand)"""
    keep = int(rng.integers(30, length - 30))
    slack = int(rng.integers(0, 200))
    if plus:
        forward = ref[junction - keep:junction] + _rand(rng, length - keep)
        return sc.rc_ref(forward), ord("+"), junction - keep - slack - SPACER
    forward = _rand(rng, length - keep) + ref[junction:junction + keep]
    return forward, ord("-"), junction + keep + slack - SPACER


def deletion_read(rng, ref, length):
    """a '+' anchored read over a deletion of 60 bases: a close and a far end"""
    bp = int(rng.integers(SPACER + 1000, SPACER + 19000 - 300))
    keep = int(rng.integers(40, length - 40))
    forward = ref[bp - keep:bp] + ref[bp + 60:bp + 60 + length - keep]
    return sc.rc_ref(forward), ord("+"), bp - keep - int(rng.integers(0, 200)) - SPACER


def batch_from(records):
    return sc.batch_of([r[0] for r in records], [r[1] for r in records], [r[2] for r in records], [INSERT_SIZE] * len(records))


def records(n_junction, n_no_close, n_deletion, seed=5, only_plus=False, junctions=JUNCTIONS, shuffle=True):
    """n_junction reads per junction and side, n_no_close reads of random sequence, n_deletion deletion reads, shuffled"""
    rng = np.random.default_rng(seed)
    ref = chromosome()[0][1]
    out = []
    for j in junctions:
        for plus in ((True,) if only_plus else (True, False)):
            out += [junction_read(rng, ref, j, plus, int(rng.choice([100, 150]))) for _ in range(n_junction)]
    out += [(_rand(rng, int(rng.choice([100, 150]))), int(rng.choice([ord("+"), ord("-")])), int(rng.integers(2000, 18000))) for _ in range(n_no_close)]
    out += [deletion_read(rng, ref, int(rng.choice([100, 150]))) for _ in range(n_deletion)]
    if shuffle:
        out = [out[k] for k in rng.permutation(len(out))]
    return out


def shortened_records(n, seed=9):
    """'-' anchored junction reads with two bytes outside ACGTN behind them and the anchor one insert size further away: the first
    three attempts of the close end find nothing, the fourth sees the read without those bytes (rc_flag 2, two bases shorter)"""
    rng = np.random.default_rng(seed)
    ref = chromosome()[0][1]
    out = []
    for _ in range(n):
        s, strand, pos = junction_read(rng, ref, JUNCTIONS[1], False, 100)
        out.append((s + b"XX", strand, pos - INSERT_SIZE))
    return out
