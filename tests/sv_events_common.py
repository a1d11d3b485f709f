"""Shared by tests/test_sv_events_cpu.py and tests/test_gpu_sv_events.py: hand-made per-read records and sv lists
whose keys come from three or four values per field, the literal Python restatement of the DI and inversion reporters
(pg_host.cpp:709-775, pg_host_sv.cpp:360-452) over them, and the coverage a comparison on such arrays must reach."""
import numpy as np

from pindel_amd import binding, hostlib

U32 = 0xffffffff
SPACER = 1000
COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
SV_TABLE_KINDS = (2, 5, 6)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def to_short(v):
    v &= 0xffff
    return v - 0x10000 if v & 0x8000 else v


def to_int(v):
    v &= U32
    return v - (1 << 32) if v >> 31 else v


def make_chrom(rng, bio_len=88000):
    return b"N" * SPACER + bytes(rng.choice(ACGT, size=bio_len)) + b"N" * SPACER


def box_size_of(chrom):
    return max(len(chrom) // 30000, 1)


LEFTS = (5000, 5001, 5002, 9000)      # with a box of 3 bases: two adjacent boxes and a third
BIG_RIGHT = 0xfffff000                # BPLeft + BPRight wraps, and no window end minus two insert sizes lies below it
FILLER_LEFT = 80000                   # an inversion pair in front of the chosen slot: outside the region [0, 20000]


def random_lists(rng, n, kinds=(2, 5, 6), p_boxed=0.9, one_box=False, few_keys=False, lefts=LEFTS, p_fail=0.05):
    """(records, (sv cands, sv counts)) for n reads: every read boxed (with probability p_boxed) by one pair of one of `kinds`, the
    pair's fields from three or four values each.  BPRight BIG_RIGHT makes BPLeft + BPRight wrap; IndelSize 98 harmonises to 100,
    50 (with probability p_fail) fails against it, 0 comes with a BPRight of its own: a run with mx == 0.  lefts: the values of
    BPLeft (one_box: the second and third only).  few_keys: two values for BPRight, BP and NT_size -- long tie classes.  An
    inversion pair in slot 1 .. 3 has FILLER_LEFT pairs in front of it, which a cascade over the region [0, 20000] passes by."""
    recs = np.zeros(n, dtype=hostlib.EVENT_READ_DTYPE)
    sv = np.zeros((n, hostlib.SV_SLOTS), dtype=hostlib.VARIANT_CAND_DTYPE)
    sv_n = np.zeros((n, 5), dtype=np.uint8)
    kind = rng.choice(np.array(kinds), size=n)
    boxed = rng.random(n) < p_boxed
    for i in range(n):
        k = int(kind[i])
        if not boxed[i]:
            # what the SV tables must ignore: a read boxed by another kind, one Used without a box, an untouched one
            other = rng.integers(0, 3)
            if other == 0:
                recs[i]["kind"], recs[i]["flags"] = rng.choice([0, 1, 3, 4]), hostlib.EVR_BOXED
            elif other == 1:
                recs[i]["kind"], recs[i]["flags"] = k, hostlib.EVR_USED
            continue
        slot = int(rng.integers(0, 4)) if k == 5 else 0
        c = sv[i, hostlib.SV_SLOT[k] + slot]
        for j in range(slot):
            f = sv[i, hostlib.SV_SLOT[k] + j]
            f["bp_left"], f["bp_right"], f["left"], f["right"], f["indel_size"] = FILLER_LEFT, FILLER_LEFT + 100, 100, 300, 100
        c["bp_left"] = rng.choice(lefts[1:3] if one_box else lefts, p=None if one_box else [0.3, 0.3, 0.25, 0.15])
        c["bp_right"] = rng.choice([5100, BIG_RIGHT], p=[0.8, 0.2]) if few_keys else rng.choice([5100, 5101, 5102, BIG_RIGHT], p=[0.35, 0.3, 0.2, 0.15])
        c["indel_size"] = rng.choice([0, 1, 2, 3], p=[0.3, 0.3, 0.2, 0.2]) if k == 2 else rng.choice([100, 98, 50], p=[0.6, 0.4 - p_fail, p_fail])
        if k != 2 and rng.random() < 0.2:
            c["indel_size"], c["bp_right"] = 0, 5200                  # a sum of their own: a run with mx == 0
        c["bp"] = rng.choice([19, 20] if few_keys else [3, 19, 20, 36])
        c["left"], c["right"] = 100, 300
        nt = int(rng.integers(0, 2 if few_keys else 4)) if k != 5 else 0
        c["nt_rot"] = nt
        if k != 2:
            c["flags"] = int(rng.integers(0, 4)) << 4
        sv_n[i, k - 2] = slot + 1
        recs[i]["kind"], recs[i]["slot"], recs[i]["flags"], recs[i]["nt_size"] = k, slot, hostlib.EVR_BOXED, nt
    return recs, (sv, sv_n)


def random_input(rng, n, chrom, spread=False, **kw):
    """n reads of 40 (a few of 38) bases with one close point each -- LeftMostPos from a handful of values -- and random_lists over
    them (spread: from many, so that few reads are duplicates).  Most DI reads with IndelSize == NT_size get the bases planted that
    make their event a short inversion."""
    recs, (sv, sv_n) = random_lists(rng, n, **kw)
    lens = rng.choice([40, 38], size=n, p=[0.85, 0.15])
    seqs = [bytearray(rng.choice(ACGT, size=int(l)).tobytes()) for l in lens]
    strand = rng.choice(np.array([ord("+"), ord("-")], dtype=np.uint8), size=n)
    for i in range(n):
        if recs[i]["kind"] != 2 or not recs[i]["flags"] & hostlib.EVR_BOXED or rng.random() < 0.4:
            continue
        c = sv[i, 0]
        nt, bp, pos = int(c["nt_rot"]), int(c["bp"]), SPACER + 1 + int(c["bp_left"])
        if int(c["indel_size"]) != nt or bp + 1 + nt > len(seqs[i]):
            continue
        want = chrom[pos:pos + nt].translate(COMP)[::-1]
        src = bytearray(bytes(seqs[i]).translate(COMP)[::-1]) if strand[i] == ord("+") else seqs[i]
        src[bp + 1:bp + 1 + nt] = want
        seqs[i] = bytearray(bytes(src).translate(COMP)[::-1]) if strand[i] == ord("+") else src
    seqs = [bytes(s) for s in seqs]
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    close_abs = rng.integers(6000, 8000, size=n) if spread else rng.choice([6000, 6001, 6010], size=n)
    close = np.array([(int(a), int(l), 0, 0, b"+", b"+") for a, l in zip(close_abs, rng.choice([10, 11, 12], size=n))], dtype=binding.POINT_DTYPE)
    return dict(n=n, seqs=seqs, seq=np.frombuffer(b"".join(seqs), dtype=np.uint8), seq_off=off, strand=strand, rc_flag=np.zeros(n, dtype=np.uint8),
                close_off=np.arange(n + 1, dtype=np.uint64), close_pts=close, recs=recs, sv=(sv, sv_n),
                read_len=np.array([len(s) for s in seqs]), close_abs=close["abs_loc"].astype(np.int64), close_len=close["length"].astype(np.int64))


def host_tables(inp, w, chrom):
    return hostlib.sv_events_from_lists([("chrR", chrom)], inp["seq"], inp["seq_off"], inp["strand"], inp["rc_flag"], inp["close_off"],
                                        inp["close_pts"], w, inp["recs"], inp["sv"], spacer=SPACER)


def fields_of(inp, i):
    """(BPLeft, BPRight, IndelSize, carried NT_size, BP) of a boxed read"""
    r = inp["recs"][i]
    c = inp["sv"][0].reshape(inp["n"], hostlib.SV_SLOTS)[i, hostlib.SV_SLOT[int(r["kind"])] + int(r["slot"])]
    return int(c["bp_left"]), int(c["bp_right"]), int(c["indel_size"]), int(r["nt_size"]), int(c["bp"])


def left_most(inp, i):
    plus = inp["strand"][i] == ord("+")
    a, l, RL = int(inp["close_abs"][i]), to_short(int(inp["close_len"][i])), to_short(int(inp["read_len"][i]))
    return to_int(a + 1 - l) if plus else to_int(a + l - RL)


def sort_key(kind, f):
    bl, br, isz, nt, bp = f
    if kind == 2:
        return (bl, br, nt, bp)
    return ((bl + br) & U32, -isz, bl, br, nt if kind == 6 else 0, bp)


def balance(inp, members):
    """ReportEvent over (read, NT_size, BP) triples"""
    lmin = lmax = rmin = rmax = False
    for i, nt, bp in members:
        RL = int(inp["read_len"][i])
        rl = to_short(RL - nt)
        mn = to_short(to_short(int(rl * 0.5 + 0.5)) - 1)
        mx = to_short(to_short(int(rl * (1 - 0.5) - 0.5)) - 1)
        lmin |= bp <= mn
        rmin |= RL - bp - nt <= mn
        lmax |= bp >= mx
        rmax |= RL - bp - nt >= mx
    return lmin and lmax and rmin and rmax


def nt_str_of(inp, i, bp, nt):
    seq = inp["seqs"][i]
    src = seq.translate(COMP)[::-1] if inp["strand"][i] == ord("+") else seq
    return src[bp + 1:bp + 1 + nt] if 0 <= bp + 1 <= len(src) and nt > 0 else b""


def restate(inp, w, chrom):
    """The three reporters, literally: the exchange loops with their strict compares, the double duplicate loops, the linear
    grouping, harmonise() with `whether` never re-armed inside a box.  Returns members, events (tuples in EVENT_DTYPE order) and
    dropped runs per table."""
    n, bs = inp["n"], box_size_of(chrom)
    members, events, dropped = [], [], []
    for kind in SV_TABLE_KINDS:
        boxes = {}
        for i in range(n):
            r = inp["recs"][i]
            if r["flags"] & hostlib.EVR_BOXED and r["kind"] == kind:
                boxes.setdefault(int(to_int(fields_of(inp, i)[0]) / bs) & U32, []).append(i)
        mem, evs, drop = [], [], 0
        for box in sorted(boxes):
            idx = boxes[box]
            key = {i: sort_key(kind, fields_of(inp, i)) for i in idx}
            for a in range(len(idx) - 1):
                for d in range(a + 1, len(idx)):
                    if key[idx[a]] > key[idx[d]]:
                        idx[a], idx[d] = idx[d], idx[a]
            unique = {i: True for i in idx}
            for a in range(len(idx) - 1):
                for d in range(a + 1, len(idx)):
                    x, y = idx[a], idx[d]
                    lx, ly, rx, ry = left_most(inp, x), left_most(inp, y), int(inp["read_len"][x]), int(inp["read_len"][y])
                    if (kind != 2 or rx == ry) and (lx == ly or lx + rx == ly + ry) and inp["strand"][x] == inp["strand"][y]:
                        unique[y] = False
            head = len(mem)
            if kind == 2:
                good = [i for i in idx if unique[i]]
                f = {i: fields_of(inp, i) for i in good}
                s = 0
                while s < len(good):
                    e = s
                    bl, br, isz, nt, bp = f[good[s]]
                    while e + 1 < len(good) and (f[good[e + 1]][0], f[good[e + 1]][2], to_short(f[good[e + 1]][3])) == (bl, isz, to_short(nt)):
                        e += 1
                    flags = 0
                    if e - s + 1 >= w.min_support:
                        flags |= hostlib.EV_SUPPORT
                    if isz < w.balance_cutoff or balance(inp, [(i, f[i][3], f[i][4]) for i in good[s:e + 1]]):
                        flags |= hostlib.EV_BALANCE
                    if isz == nt:
                        pos = SPACER + 1 + bl
                        replaced = chrom[pos:pos + nt] if pos <= len(chrom) and nt > 0 else b""
                        if replaced.translate(COMP)[::-1] == nt_str_of(inp, good[s], bp, nt):
                            flags |= hostlib.EV_SHORT_INV
                    if flags & 5 == 5:
                        flags |= hostlib.EV_REPORT
                    n_plus = sum(int(inp["strand"][i] == ord("+")) for i in good[s:e + 1])
                    evs.append((bl, br, isz, head + s, e - s + 1, n_plus, bl, br, head, nt, kind, flags))
                    s = e + 1
                mem += good
                continue
            mem += [i | (0 if unique[i] else hostlib.SVEV_MEMBER_DUP) for i in idx]
            good = [list(fields_of(inp, i)) for i in idx]
            whether = True
            cs = 0
            cbl, cbr = good[0][0], good[0][1]

            def harmonise(cs, ce):
                nonlocal whether
                mx = max(g[2] for g in good[cs:ce + 1])
                for k in range(cs, ce + 1):
                    g, i = good[k], idx[k]
                    RL = int(inp["read_len"][i])
                    with np.errstate(divide="ignore", invalid="ignore"):
                        q = float(np.float32(g[2]) / np.float32(mx))
                    if q < 0.95 or ((mx + 30) & U32) > ((RL + g[2]) & U32):
                        whether = False
                        break
                    diff = to_short((mx - g[2]) // 2)
                    g[2] = mx
                    g[0] = (g[0] - diff) & U32
                    g[1] = (g[1] + diff) & U32
                    if inp["strand"][i] == ord("+"):
                        if g[4] > diff:
                            g[4] = to_short(g[4] - diff)
                    elif g[4] + diff < to_short(RL - 1):
                        g[4] = to_short(g[4] + diff)
                return mx

            runs = []
            for k in range(1, len(good)):
                if (good[k][0] + good[k][1]) & U32 == (cbl + cbr) & U32:
                    continue
                harmonise(cs, k - 1)
                runs.append((cs, k - 1, good[cs][0], good[cs][1], whether))
                cs = k
                cbl, cbr = good[k][0], good[k][1]
            harmonise(cs, len(good) - 1)
            runs.append((cs, len(good) - 1, cbl, cbr, whether))
            for s, e, rs, re_, ok in runs:
                if not ok:
                    drop += 1
                    continue
                flags = 0
                if e - s + 1 >= w.min_support:
                    flags |= hostlib.EV_SUPPORT
                if not (re_ < rs or rs == 0):
                    flags |= hostlib.EV_RANGE
                if good[s][2] < w.balance_cutoff or balance(inp, [(idx[k], good[k][3], good[k][4]) for k in range(s, e + 1)]):
                    flags |= hostlib.EV_BALANCE
                if flags == 7:
                    flags |= hostlib.EV_REPORT
                n_plus = sum(int(inp["strand"][idx[k]] == ord("+")) for k in range(s, e + 1))
                evs.append((good[s][0], good[s][1], good[s][2], head + s, e - s + 1, n_plus, rs, re_, head, good[s][3], kind, flags))
        members.append(np.array(mem, dtype=np.uint32))
        events.append(np.array(evs, dtype=hostlib.EVENT_DTYPE) if evs else np.zeros(0, dtype=hostlib.EVENT_DTYPE))
        dropped.append(drop)
    return dict(members=members, events=events, dropped_runs=dropped)


def new_seen():
    z = lambda: np.zeros(3, np.int64)
    return dict(odd_ties=z(), dups=z(), harmonised=z(), failed_with_later=z(), last_run_differs=z(), mx_zero=z(), short_inv=0, wraps=z(),
                events=z(), multi=z(), no_balance=z())


def note_coverage(seen, inp, tabs, chrom):
    """What the tables `tabs` of the input exercised, added to `seen` (per SV table)."""
    bs = box_size_of(chrom)
    for t, kind in enumerate(SV_TABLE_KINDS):
        words = [int(x) for x in tabs["members"][t]]
        reads = [x & 0x7fffffff for x in words]
        f = [fields_of(inp, i) for i in reads]
        ev = tabs["events"][t]
        seen["events"][t] += len(ev)
        seen["multi"][t] += int((ev["n_reads"] >= 2).sum())
        seen["no_balance"][t] += int(((ev["flags"] & hostlib.EV_BALANCE) == 0).sum())
        # tie classes: consecutive members of a box with an equal sort key
        s = 0
        while s < len(reads):
            e = s
            while e + 1 < len(reads) and sort_key(kind, f[e + 1]) == sort_key(kind, f[s]) and f[e + 1][0] // bs == f[s][0] // bs:
                e += 1
            cls = reads[s:e + 1]
            if len(cls) >= 3 and cls != sorted(cls) and cls != sorted(cls, reverse=True):
                seen["odd_ties"][t] += 1
            s = e + 1
        n_boxed = int(((inp["recs"]["flags"] & hostlib.EVR_BOXED != 0) & (inp["recs"]["kind"] == kind)).sum())
        seen["dups"][t] += n_boxed - len(reads) if kind == 2 else sum(1 for x in words if x & hostlib.SVEV_MEMBER_DUP)
        if kind == 2:
            seen["short_inv"] += int(((ev["flags"] & hostlib.EV_SHORT_INV != 0) & (ev["nt_size"] > 0)).sum())
            continue
        covered = np.zeros(len(reads), dtype=bool)
        for e in ev:
            a, b = int(e["first"]), int(e["first"]) + int(e["n_reads"])
            covered[a:b] = True
            isz = [f[k][2] for k in range(a, b)]
            seen["harmonised"][t] += any(x != int(e["indel_size"]) for x in isz)
            seen["mx_zero"][t] += int(e["indel_size"]) == 0
            seen["wraps"][t] += any(f[k][0] + f[k][1] > U32 for k in range(a, b))
            # the first member of a run has the run's largest IndelSize (the second sort key, descending): its harmonisation is the
            # identity, so the range of a box's last run cannot differ from the harmonised one
            seen["last_run_differs"][t] += (int(e["real_start"]), int(e["real_end"])) != (int(e["bp_left"]), int(e["bp_right"]))
        # the first run of a box without an event with another run of the box behind it
        s = 0
        while s < len(reads):
            e = s
            while e + 1 < len(reads) and f[e + 1][0] // bs == f[s][0] // bs:
                e += 1
            lost = [k for k in range(s, e + 1) if not covered[k]]
            if lost:
                first_sum = (f[lost[0]][0] + f[lost[0]][1]) & U32
                seen["failed_with_later"][t] += any((f[k][0] + f[k][1]) & U32 != first_sum for k in lost)
            s = e + 1
    return seen


def assert_coverage(seen):
    """Per table it applies to: a tie class of three reads or more left in an order that is neither ascending nor descending read
    index; a duplicate; a harmonised run with mx different from a member's IndelSize; a failed harmonisation with a later run in
    the same box; mx == 0; a sum that wraps; a short inversion with bases to compare.  `A last run whose range differs from the
    harmonised values' cannot occur -- the first member of a run carries the run's largest IndelSize, its diff is 0 -- and is
    asserted to be absent."""
    assert (seen["odd_ties"] > 0).all() and (seen["dups"] > 0).all() and (seen["events"] > 0).all() and (seen["multi"] > 0).all(), seen
    for name in ("harmonised", "failed_with_later", "mx_zero", "wraps"):
        assert (seen[name][1:] > 0).all(), (name, seen)
    assert (seen["last_run_differs"] == 0).all(), seen
    assert seen["short_inv"] > 0 and (seen["no_balance"] > 0).all(), seen


def assert_same_tables(got, want, what=""):
    assert list(got["n_members"]) == [len(m) for m in want["members"]], (what, got["n_members"])
    assert list(got["dropped_runs"]) == list(want["dropped_runs"]), (what, got["dropped_runs"], want["dropped_runs"])
    for t in range(3):
        assert got["members"][t].tolist() == want["members"][t].tolist(), (what, t)
        assert len(got["events"][t]) == len(want["events"][t]), (what, t)
        for name in hostlib.EVENT_DTYPE.names:
            assert got["events"][t][name].tolist() == want["events"][t][name].tolist(), (what, t, name)
