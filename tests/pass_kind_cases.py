"""Reads for the two forms of pg_pass_forms.h (tests/test_gpu_pass_kinds.py, tests/test_gpu_quarter_tree.py, tests/test_pass_kind_cases_cpu.py).

Built like tests/pass_idle_cases.py, whose builders are used as they are: the chromosome is 'N' throughout but for planted pieces of
the reads, the reads are runs of one letter, so the planted copies are the only candidates and their order in the window is known.
Index j below is the j-th base a search consumes; a piece is the first m consumed bases as the reference shows them.

  kinds    (blocks of a candidate, both kinds)  the close end of a '+' anchor grows left to right (kind F), that of a '-' anchor right to
           left (kind B); the far end holds both kinds in one pass.  One long copy (alive into the second 64-base block, which holds
           36 bases of a 100-base read and 37 of a 101-base one) with substitutions at 30 and 45 (a read that simply maps is no split
           read), and on top of that per case: the copy at the first / last position attempt 0's window admits and one position
           outside either; a substitution at 63, at 64, at both; an N in the read at 0, 63, 64; an N in the reference under 0, 63, 64.
           Far cases: a long copy of one kind with the same variants at 63 / 64 and a worse long copy of the other kind beside it.
  quarters (ties across the tier A quarters)  k = 2, 3, 4, 5, 8 short-lived copies of the first 16 consumed bases (dead before
           bps + 16: tier A; quarter = rank in the window modulo 4) tie at every length: no point.  The same with copy i two bases
           longer, every i: it is alone two levels below the others at length 18 -- one point, whichever quarter holds it.  Far end:
           copies of 18 bases in all three rings (two in ring 0) tie; one copy of 20 bases in ring 0, 1 or 2 wins at length 20 once
           its ring is part of the state (qmask 1, 3, 15).
"""
import numpy as np

from pindel_amd.hostio import SPACER
from tests import pass_idle_cases as pic
from tests.parity import run_oracle

REGION = pic.REGION
ISZ = 2000
ISZ_FAR = 300
M_CLOSE_FAR = 30       # the close part of a far case
M_FAR = 72             # a long far-end copy
BASE_SUBS = (30, 45)
WORSE_SUBS = (20, 30, 45, 50)


class Case:
    def __init__(self, name, seq, strand, anchor, isz, n_copies):
        self.name, self.seq, self.strand, self.anchor, self.isz, self.n_copies = name, seq, strand, anchor, isz, n_copies


def _edit(piece, strand_step, m, subs=(), ns=()):
    """the piece with a base no read holds ('T' in a close piece of C / G runs; see _far_edit) at consumed indices subs, 'N' at ns;
    strand_step > 0: consumed index j is piece[j], otherwise piece[m - 1 - j]"""
    p = bytearray(piece)
    for j, ch in [(j, b"T") for j in subs] + [(j, b"N") for j in ns]:
        if j < m:
            p[j if strand_step > 0 else m - 1 - j] = ch[0]
    return bytes(p)


def _read_n(seq, strand, close, j):
    """the read with an N at consumed index j of its close end (close) or of its far end"""
    s = bytearray(seq)
    if close:
        s[len(s) - 1 - j] = ord("N")         # both strands: the close end consumes the read from its last base ('+': as RC)
    else:
        s[j] = ord("N")                       # the far end consumes it from its first base
    return bytes(s)


def _region(idx):
    return SPACER + REGION * idx + REGION // 2


def _chrom(n):
    return bytearray(b"N" * (2 * SPACER + REGION * (n + 1)))


def _anchor(strand, ws, isz):
    return ws - SPACER if strand == "+" else ws + isz - SPACER


KIND_VARIANTS = [("base", {}), ("sub63", dict(subs=(63,))), ("sub64", dict(subs=(64,))), ("sub63_64", dict(subs=(63, 64))),
                 ("readN0", dict(read_n=0)), ("readN63", dict(read_n=63)), ("readN64", dict(read_n=64)),
                 ("refN0", dict(ns=(0,))), ("refN63", dict(ns=(63,))), ("refN64", dict(ns=(64,)))]
KIND_PLACES = ["first", "last", "before", "after"]


def build_kinds(L):
    """(chromosome, cases): close cases without a far end (the read begins with N), then far cases"""
    plan = [("close", s, v) for s in "+-" for v in [n for n, _ in KIND_VARIANTS] + KIND_PLACES]
    plan += [("far", s, k, v) for s in "+-" for k in "FB" for v, kw in KIND_VARIANTS if "0" not in v]
    chrom = _chrom(len(plan))
    cases, pending = [], []
    var = dict(KIND_VARIANTS)
    for idx, item in enumerate(plan):
        mid, strand = _region(idx), item[1]
        step = 1 if strand == "+" else -1
        if item[0] == "close":
            m = L - 1
            seq = pic._read(strand, L, m, False)
            ws = mid - ISZ // 2
            kw = var.get(item[2], {})
            pos = {"first": ws, "last": ws + ISZ - 1, "before": ws - 1, "after": ws + ISZ}.get(item[2], mid)
            piece, off = pic._close_piece(seq, strand, m)
            piece = _edit(piece, step, m, BASE_SUBS + tuple(kw.get("subs", ())), kw.get("ns", ()))
            pic._plant(chrom, pos, piece, off)
            if "read_n" in kw:
                seq = _read_n(seq, strand, True, kw["read_n"])
            cases.append(Case(f"close{strand}{item[2]}", seq, strand, _anchor(strand, ws, ISZ), ISZ, 1))
        else:
            kind, v = item[2], item[3]
            seq = pic._read(strand, L, M_CLOSE_FAR, True)
            ws = mid - ISZ_FAR // 2
            piece, off = pic._close_piece(seq, strand, M_CLOSE_FAR)
            pic._plant(chrom, mid, piece, off)
            cases.append(Case(f"far{strand}{kind}{v}", seq, strand, _anchor(strand, ws, ISZ_FAR), ISZ_FAR, 3))
            pending.append((len(cases) - 1, kind, var[v]))
    first = run_oracle({}, [("chrK", bytes(chrom))], batch_of(cases))
    for i, kind, kw in pending:
        c = cases[i]
        assert first["close_cnt"][i] > 0, c.name
        center = int(first["close_pts"][i][first["close_cnt"][i] - 1]["abs_loc"])
        other = "B" if kind == "F" else "F"
        # the long copy of `kind` on one side of the centre, the worse copy of the other kind on the other side, both in the outer ring
        for k, side, subs, ns in ((kind, 1, BASE_SUBS + tuple(kw.get("subs", ())), kw.get("ns", ())), (other, -1, WORSE_SUBS, ())):
            piece, off = pic._far_piece(c.seq, k, M_FAR)
            piece = _far_edit(piece, k, M_FAR, subs, ns)
            lo = center + 300 if side > 0 else center - 300 - M_FAR
            pic._plant(chrom, lo + off, piece, off)
        if "read_n" in kw:
            c.seq = _read_n(c.seq, c.strand, False, kw["read_n"])
    return bytes(chrom), cases


def _far_edit(piece, kind, m, subs, ns):
    """far pieces: kind F shows the read's bases left to right (A G...G C...), kind B their complement right to left; a 'T' in an F piece
    and an 'A' in a B piece is a base neither the read nor its complement holds there"""
    p = bytearray(piece)
    for j, ch in [(j, b"T" if kind == "F" else b"A") for j in subs] + [(j, b"N") for j in ns]:
        p[j if kind == "F" else m - 1 - j] = ch[0]
    return bytes(p)


QUARTER_COPIES = (2, 3, 4, 5, 8)
SHORT, BETTER = 16, 18                 # consumed bases of a tied copy / of the better one (close end: bps 8, tier A up to 24)
SHORT_FAR, BETTER_FAR = 18, 20         # (far end: bps 10, tier A up to 26)


def build_quarters(L):
    """(chromosome, cases).  Case names: q{strand}{k}tie, q{strand}{k}b{i} (copy i is the better one), f{strand}tie, f{strand}r{ring}"""
    plan = []
    for s in "+-":
        for k in QUARTER_COPIES:
            plan.append(("q", s, k, None))
            plan += [("q", s, k, i) for i in range(k)]
        plan += [("f", s, None, r) for r in (None, 0, 1, 2)]
    chrom = _chrom(len(plan))
    cases, pending = [], []
    for idx, (what, strand, k, better) in enumerate(plan):
        mid = _region(idx)
        if what == "q":
            seq = pic._read(strand, L, L - 1, False)
            ws = mid - ISZ // 2
            start = ws + 40
            for j in range(k):
                piece, off = pic._close_piece(seq, strand, BETTER if j == better else SHORT)
                pic._plant(chrom, start + off, piece, off)
                start += len(piece) + 12
            cases.append(Case(f"q{strand}{k}" + ("tie" if better is None else f"b{better}"), seq, strand, _anchor(strand, ws, ISZ), ISZ, k))
        else:
            seq = pic._read(strand, L, M_CLOSE_FAR, True)
            ws = mid - ISZ_FAR // 2
            piece, off = pic._close_piece(seq, strand, M_CLOSE_FAR)
            pic._plant(chrom, mid, piece, off)
            cases.append(Case(f"f{strand}" + ("tie" if better is None else f"r{better}"), seq, strand, _anchor(strand, ws, ISZ_FAR), ISZ_FAR, 6))
            pending.append((len(cases) - 1, better))
    first = run_oracle({}, [("chrQ", bytes(chrom))], batch_of(cases))
    for i, better in pending:
        c = cases[i]
        assert first["close_cnt"][i] > 0, c.name
        center = int(first["close_pts"][i][first["close_cnt"][i] - 1]["abs_loc"])
        free = 1 if c.strand == "+" else -1          # the side of the centre the close piece leaves free
        # (distance from the centre, side, ring): two copies in ring 0, one in ring 1, two in ring 2 -- kinds F, B alternating
        spots = [(10, free, 0), (36, free, 0), (M_CLOSE_FAR + 60, -free, 1), (300, free, 2), (340, -free, 2)]
        done = set()
        for n, (dist, side, ring) in enumerate(spots):
            is_better = better == ring and ring not in done
            done.add(ring)
            m = BETTER_FAR if is_better else SHORT_FAR
            kind = "F" if n % 2 == 0 else "B"
            piece, off = pic._far_piece(c.seq, kind, m)
            lo = center + dist if side > 0 else center - dist - m + 1
            pic._plant(chrom, lo + off, piece, off)
    return bytes(chrom), cases


def batch_of(cases, order=None):
    return pic.batch_of(cases, order)


def check_situations(L, cases, orc, first=0):
    """every case reaches the situation it is named for -- read from the oracle's points alone (read i of the result is case i - first)"""
    for k, c in enumerate(cases):
        i = first + k
        cl = orc["close_pts"][i][:int(orc["close_cnt"][i])]["length"].tolist()
        fp = orc["far_pts"][i][:int(orc["far_cnt"][i])]
        fl = fp["length"].tolist()
        v = c.name[6:] if c.name.startswith("close") else c.name[5:]
        if c.name.startswith("close"):
            assert not fl, c.name                                     # (the read begins with N: no far end)
            if v in ("readN0", "refN0"):
                assert not cl, c.name                                 # the first consumed base must match: no candidate
            elif v == "sub63_64":
                assert cl and max(cl) == 63, (c.name, cl)             # level 4 from length 65 on: past g_maxMismatch up to 74
            else:
                assert cl and max(cl) == L - 1 and min(cl) == 8, (c.name, cl)
        elif c.name.startswith("far"):
            assert cl and max(cl) == M_CLOSE_FAR, (c.name, cl)
            want = {"base": M_FAR, "sub63": 63, "sub64": 64, "sub63_64": 63, "refN63": 63, "refN64": 64}.get(v, M_FAR)
            assert fl and max(fl) == want, (c.name, fl)               # the long copy wins up to its first extra mismatch
            assert set(fp["direction"].tolist()) == {b"+" if c.name[4] == "F" else b"-"}, c.name
        elif c.name.startswith("q"):
            assert cl == ([] if c.name.endswith("tie") else [BETTER]) and not fl, (c.name, cl)
        else:
            assert cl and max(cl) == M_CLOSE_FAR, (c.name, cl)
            assert fl == ([] if c.name.endswith("tie") else [BETTER_FAR]), (c.name, fl)
