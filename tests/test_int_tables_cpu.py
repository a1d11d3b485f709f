"""The interchromosomal junction tables on the host: the header's layouts and entries; hostlib.int_tables_from_lists --
the plain-loop statement the device is compared with -- against a literal Python restatement of interchr_call plus grouping on random
arrays, with assertions that the inputs cover the contract's corners; the single consumer (Caller::report_interchr_tables) on tables
made by hand against tests/interchr_restated.py; and the synthetic set of tests/interchr_synth.py: call_from_points(report_reads=True)
with -I writes _INT and _INT_final through the tables route, byte for byte what the run without it writes."""
import ctypes
import os
import re

import numpy as np
import pytest

from pindel_amd import binding, hostlib
from tests import interchr_restated as ir
from tests import test_events_cpu as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMP = {ord("A"): ord("T"), ord("C"): ord("G"), ord("G"): ord("C"), ord("T"): ord("A"), ord("N"): ord("N")}
SPACER = 100000


# ------------------------------------------------------------------------------------------------ exports, dtypes, constants
def test_abi_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pindel_pg.h")).read()
    binding.build()
    lib = ctypes.CDLL(binding.LIB_PATH)
    for sym in ("pg_device_batch_int", "pg_device_batch_int_sizes", "pg_device_batch_int_download", "pg_device_batch_int_download_device"):
        assert f"{sym}(" in hdr and sym in binding.EXPORTS and hasattr(lib, sym), sym
    for sym in ("pgh_int_tables_from_lists", "pgh_int_write_from_tables"):
        assert hasattr(hostlib.lib(), sym), sym
    for name in ("int_calls", "int_tensors", "int_sizes", "int_download"):
        assert callable(getattr(binding.Engine, name)), name
    with open(binding.LIB_PATH, "rb") as f:
        blob = f.read()
    for kernel in (b"pg_int_flag_kernel", b"pg_int_compact_kernel", b"pg_int_digit_count_kernel", b"pg_int_scatter_kernel", b"pg_int_head_kernel",
                   b"pg_int_first_kernel", b"pg_int_call_kernel"):
        assert kernel in blob, kernel


def test_layouts_and_constants_agree_with_the_header():
    hdr = open(os.path.join(ROOT, "include", "pindel_pg.h")).read()
    np_of = {"int16_t": "<i2", "uint16_t": "<u2", "uint32_t": "<u4"}
    for mod in (binding, hostlib):
        want = ec.header_struct(hdr, "pg_int_call")
        assert [n for _, n in want] == list(mod.INT_CALL_DTYPE.names)
        assert all(mod.INT_CALL_DTYPE.fields[n][0] == np.dtype(np_of[t]) for t, n in want)
        assert mod.INT_CALL_DTYPE.itemsize == 32 == sum(np.dtype(np_of[t]).itemsize for t, _ in want)        # no padding
        assert [(t, n) for t, n in ec.header_struct(hdr, "pg_int_sizes")] == [("uint64_t", f) for f, _ in mod.IntSizes._fields_]
        assert ctypes.sizeof(mod.IntSizes) == 16
        for name in ("INT_ANCHOR_MINUS", "INT_FAR_MINUS", "INT_FALLBACK"):
            m = re.search(r"#define PG_" + name + r"\s+(0x[0-9a-f]+)u", hdr)
            assert m and int(m.group(1), 16) == getattr(mod, name), name
    assert [n.split("*")[-1].strip() for _, n in ec.header_struct(hdr, "pg_int_window")] == [f for f, _ in binding.IntWindow._fields_]
    assert ctypes.sizeof(binding.IntWindow) == 16
    dev = open(os.path.join(ROOT, "pindel_amd", "csrc", "pg_device.h")).read()
    assert "PG_KERNEL_INT = 12" in dev and binding.KERNEL_INT == 12 == binding.KERNEL_LI + 1
    # the header states the order of the tables
    assert "(chr, far_chr, flags, close_abs, far_abs, nt_off, nt_len)" in hdr


# ------------------------------------------------------------------------------------------------ the contract, literally
def post_state(seq: bytes, rc_flag: int) -> bytes:
    """rc_flag applications of setUnmatchedSeq(ReverseComplement()): a byte outside ACGTN becomes NUL, trailing non-alphanumerics go"""
    for _ in range(min(int(rc_flag), 2)):
        seq = bytes(COMP.get(c, 0) for c in reversed(seq))
        while seq and not chr(seq[-1]).isalnum():
            seq = seq[:-1]
    return seq


def one_call(close, far, rl, ascending):
    """interchr_call, literally.  close / far: lists of (LengthStr, AbsLoc).  -> (close_abs, far_abs, nt_off, nt_len, fallback) or None,
    and for the coverage notes the pair of indices of a template call"""
    order_c = range(len(close)) if ascending else range(len(close) - 1, -1, -1)
    order_f = range(len(far) - 1, -1, -1) if ascending else range(len(far))
    for ci in order_c:
        for fi in order_f:
            if close[ci][0] + far[fi][0] == rl:
                return (close[ci][1], far[fi][1], 0, 0, False), (ci, fi)
    c, f = close[-1], far[-1]
    eff = c[0] + f[0]
    if not (eff >= 30 and c[0] >= 10 and f[0] >= 10):
        return None, None
    n = (rl - eff) & 0xFFFFFFFF                                   # (long)(unsigned)(len - eff)
    n = max(min(n, rl - f[0]), 0)                                 # substr stops at the end of the read
    return (c[1], f[1], f[0], n, True), None


def points_of(inp, which, i):
    off, pts = inp[which + "_off"], inp[which + "_pts"]
    return [(int(p["length"]), int(p["abs_loc"])) for p in pts[int(off[i]):int(off[i + 1])]]


def restate(inp, rank):
    """pindel_pg.h "interchromosomal junction tables", literally: (members, calls as tuples in the dtype's field order), the per-read
    notes the coverage assertions read"""
    n, n_chr = len(inp["strand"]), len(rank)
    keyed, notes = [], []
    for i in range(n):
        note = dict(junction=False, call=None)
        notes.append(note)
        close, far = points_of(inp, "close", i), points_of(inp, "far", i)
        chr_id = int(inp["chr_id"][i])
        note["no_far"] = bool(close) and not far
        if not close or not far or inp["strand"][i] not in b"+-" or not 0 <= chr_id < n_chr:
            continue
        f0 = inp["far_pts"][int(inp["far_off"][i])]
        fc = int(f0["chr_id"])
        if not 0 <= fc < n_chr:
            continue
        note["equal_ranks"] = rank[chr_id] == rank[fc] and chr_id != fc
        if rank[chr_id] == rank[fc]:
            continue
        far_minus = f0["strand"] == b"-"
        plus = inp["strand"][i] == ord("+")
        lower = rank[chr_id] < rank[fc]
        ascending = plus if lower else far_minus
        raw = inp["seqs"][i]
        rl = len(post_state(raw, inp["rc_flag"][i]))
        call, pair = one_call(close, far, rl, ascending)
        other, other_pair = one_call(close, far, rl, not ascending)
        note.update(junction=True, direction=(lower, plus if lower else far_minus), call=call, pair=pair, other_pair=other_pair, rl=rl,
                    raw_call=one_call(close, far, len(raw), ascending)[0], last=(close[-1][0], far[-1][0]))
        if call is None:
            continue
        flags = (0 if plus else hostlib.INT_ANCHOR_MINUS) | (hostlib.INT_FAR_MINUS if far_minus else 0) | (hostlib.INT_FALLBACK if call[4] else 0)
        keyed.append(((chr_id, fc, flags, call[0], call[1], call[2], call[3]), i))
    keyed.sort(key=lambda t: t[0])                                # (stable: ascending read index within a key)
    members, calls = [], []
    for key, i in keyed:
        if not calls or calls[-1][0] != key:
            calls.append([key, len(members), 0])
        calls[-1][2] += 1
        members.append(i)
    return members, [(k[0], k[1], k[3], k[4], first, cnt, k[5], k[6], k[2], 0) for k, first, cnt in calls], notes


NAMES = ["chrB", "chrA", "chrC", "chrA"]                          # (ranks 1, 0, 2, 0: the duplicate name shares its rank)


def build_input(reads):
    """reads: dicts with seq (bytes), strand (int), chr, rc_flag, close / far: lists of (LengthStr, AbsLoc, chr, strand byte)"""
    n = len(reads)
    seqs = [r["seq"] for r in reads]
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    out = dict(seqs=seqs, seq=np.frombuffer(b"".join(seqs), dtype=np.uint8) if n else np.zeros(0, np.uint8), seq_off=off,
               strand=np.array([r["strand"] for r in reads], dtype=np.uint8), chr_id=np.array([r["chr"] for r in reads], dtype=np.int32),
               rc_flag=np.array([r["rc_flag"] for r in reads], dtype=np.uint8))
    for which in ("close", "far"):
        o = np.zeros(n + 1, dtype=np.uint64)
        o[1:] = np.cumsum([len(r[which]) for r in reads])
        pts = np.zeros(int(o[-1]), dtype=binding.POINT_DTYPE)
        flat = [p for r in reads for p in r[which]]
        if flat:
            pts["length"], pts["abs_loc"] = [p[0] for p in flat], [p[1] for p in flat]
            pts["chr_id"], pts["strand"] = [p[2] for p in flat], [p[3] for p in flat]
        pts["direction"] = b"+"
        out[which + "_off"], out[which + "_pts"] = o, pts
    return out


def random_reads(rng, n):
    """n reads of 40 or 41 bases, some with bytes outside ACGTN at either end, on four chromosomes (two share a name), with 0..4 close
    points and 0..3 far points whose lengths often add up to the read, far ends on any chromosome and strand, rc flags 0..2 and the odd
    anchor strand that is neither '+' nor '-'."""
    reads = []
    for _ in range(n):
        body = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(rng.choice([40, 41]))))
        seq = b"X" * int(rng.choice([0, 0, 0, 1, 2])) + body + b"." * int(rng.choice([0, 0, 1]))
        chr_id = int(rng.choice([0, 1, 2, 3, 3]))
        far_chr = int(rng.choice([0, 1, 2, 3]))
        far_strand = b"-" if rng.random() < 0.5 else b"+"
        close = [(int(rng.choice([9, 10, 11, 12, 15, 19, 20, 21, 25])), int(SPACER + rng.choice([700, 701, 9999, 10000])), chr_id, b"+")
                 for _ in range(int(rng.choice([0, 1, 1, 2, 3, 4])))]
        far = [(int(rng.choice([9, 10, 15, 16, 19, 20, 21, 25, 28, 30, 31])), int(SPACER + rng.choice([300, 301, 5000])), far_chr, far_strand)
               for _ in range(int(rng.choice([0, 1, 1, 2, 3])))]
        reads.append(dict(seq=seq, strand=int(rng.choice(np.frombuffer(b"+-*", dtype=np.uint8), p=[0.48, 0.48, 0.04])), chr=chr_id,
                          rc_flag=int(rng.choice([0, 0, 1, 2])), close=close, far=far))
    return reads


def crafted_reads():
    """the corners, each by hand (40 bases unless said otherwise; chromosome 1 = chrA has the lowest rank, 0 = chrB, 2 = chrC)"""
    s40 = b"ACGTTGCAAC" * 4
    r = lambda **kw: dict(dict(seq=s40, strand=ord("+"), chr=1, rc_flag=0, close=[], far=[]), **kw)
    c = lambda length, at=700, ch=1: (length, SPACER + at, ch, b"+")
    f = lambda length, at=300, ch=0, sd=b"+": (length, SPACER + at, ch, sd)
    return [
        # the four scan directions, template calls
        r(close=[c(20)], far=[f(20)]), r(strand=ord("-"), close=[c(20)], far=[f(20)]),
        r(chr=0, close=[c(20, ch=0)], far=[f(20, ch=1, sd=b"-")]), r(chr=0, close=[c(20, ch=0)], far=[f(20, ch=1)]),
        # two pairs fit: ascending takes (close 0, far 1), descending (close 1, far 0)
        r(close=[c(15, 700), c(20, 705)], far=[f(20, 300), f(25, 305)]), r(strand=ord("-"), close=[c(15, 700), c(20, 705)], far=[f(20, 300), f(25, 305)]),
        # fallbacks: with bases (eff 35 < 40), eff > len, eff == len is a template call
        r(close=[c(15)], far=[f(20)]), r(close=[c(25)], far=[f(21)]),
        # the three failing conditions at the boundary
        r(close=[c(14)], far=[f(15)]), r(close=[c(15)], far=[f(15)]),        # eff 29 / 30
        r(close=[c(9)], far=[f(25)]), r(close=[c(10)], far=[f(25)]),         # the last close point 9 / 10
        r(close=[c(25)], far=[f(9)]), r(close=[c(25)], far=[f(10)]),         # the last far point 9 / 10
        # rc_flag 2 shortens "X" + 40 + "." to 40: 20 + 20 fits only then (42 as uploaded)
        r(seq=b"X" + s40 + b".", rc_flag=2, close=[c(20)], far=[f(20)]),
        # equal ranks (chromosomes 1 and 3 are both chrA), no far end
        r(chr=3, close=[c(20, ch=3)], far=[f(20, ch=1)]), r(close=[c(20)]),
        # a second member of the first call, and a far end on a chromosome outside the reference
        r(close=[c(20)], far=[f(20)]), r(close=[c(20)], far=[f(20, ch=9)]),
    ]


def statement(inp, rank):
    return hostlib.int_tables_from_lists(inp["seq"], inp["seq_off"], inp["strand"], inp["chr_id"], inp["rc_flag"], inp["close_off"],
                                         inp["close_pts"], inp["far_off"], inp["far_pts"], rank)


CORNERS = ("lower_plus", "lower_minus", "higher_far_minus", "higher_far_plus", "pair_differs", "template", "fallback_bases", "fallback_eff_gt_len",
           "eff_29", "eff_30", "close_9", "close_10", "far_9", "far_10", "shortened_only", "equal_ranks", "no_far", "group_of_two")


def note_coverage(seen, notes, calls):
    for x in notes:
        seen["no_far"] |= x["no_far"]
        seen["equal_ranks"] |= x.get("equal_ranks", False)
        if not x["junction"]:
            continue
        lower, flag = x["direction"]
        seen["lower_plus"] |= lower and flag
        seen["lower_minus"] |= lower and not flag
        seen["higher_far_minus"] |= not lower and flag
        seen["higher_far_plus"] |= not lower and not flag
        seen["pair_differs"] |= x["pair"] is not None and x["other_pair"] is not None and x["pair"] != x["other_pair"]
        call, (cl, fl) = x["call"], x["last"]
        if x["pair"] is None:
            seen["eff_29"] |= call is None and cl + fl == 29 and cl >= 10 and fl >= 10
            seen["eff_30"] |= call is not None and cl + fl == 30
            seen["close_9"] |= call is None and cl == 9 and fl >= 21
            seen["close_10"] |= call is not None and cl == 10
            seen["far_9"] |= call is None and fl == 9 and cl >= 21
            seen["far_10"] |= call is not None and fl == 10
        if call is not None:
            seen["template"] |= not call[4]
            seen["fallback_bases"] |= call[4] and call[3] > 0 and cl + fl < x["rl"]
            seen["fallback_eff_gt_len"] |= call[4] and cl + fl > x["rl"]
            seen["shortened_only"] |= not call[4] and (x["raw_call"] is None or x["raw_call"][4])
    seen["group_of_two"] |= any(c[5] >= 2 for c in calls)


def test_random_arrays_against_the_literal_restatement():
    rank = hostlib.chr_ranks(NAMES)
    assert rank.tolist() == [1, 0, 2, 0]
    seen = dict.fromkeys(CORNERS, False)
    batches = [crafted_reads()]
    for n in (1, 2, 3, 7, 40, 64, 65, 120, 200):
        rng = np.random.default_rng(9100 + n)
        batches += [random_reads(rng, n) for _ in range(6)]
    rng = np.random.default_rng(5)
    mixed = random_reads(rng, 150) + crafted_reads()
    batches.append([mixed[k] for k in rng.permutation(len(mixed))])
    n_calls = 0
    for k, reads in enumerate(batches):
        inp = build_input(reads)
        got = statement(inp, rank)
        members, calls, notes = restate(inp, rank.tolist())
        assert got["members"].tolist() == members, k
        assert [tuple(int(x) for x in c) for c in got["calls"]] == calls, k
        assert sum(c[5] for c in calls) == len(members) and sorted((c[0], c[1], c[8], c[2], c[3], c[6], c[7]) for c in calls) == [
            (c[0], c[1], c[8], c[2], c[3], c[6], c[7]) for c in calls], k
        n_calls += len(calls)
        if k == 0:                                                # every corner is in the crafted batch alone
            crafted = dict.fromkeys(CORNERS, False)
            note_coverage(crafted, notes, calls)
            assert all(crafted.values()), crafted
        note_coverage(seen, notes, calls)
    assert all(seen.values()) and n_calls > 200, (seen, n_calls)


def test_empty_input_and_a_reference_without_chromosomes():
    inp = build_input([])
    got = statement(inp, hostlib.chr_ranks(NAMES))
    assert got["members"].size == 0 and got["calls"].size == 0
    inp = build_input(crafted_reads())
    got = statement(inp, np.zeros(0, dtype=np.int32))
    assert got["members"].size == 0 and got["calls"].size == 0


# ------------------------------------------------------------------------------------------------ the consumer on hand-made tables
def restated_lines(reads, int_pairs=False):
    """tests/interchr_restated.int_lines, and its loop with --repair int-pairs: every pair in the reference's order, a
    name entered only when its read matches the pair in hand, the calls counted and written pair by pair"""
    if not int_pairs:
        return ir.int_lines(reads, SPACER)[0]
    sr = ir.collect(reads)
    chr_names = sorted({r["FragName"] for r in sr} | {r["FarFragName"] for r in sr})
    read_names, out = set(), ""
    for a in range(len(chr_names)):
        for b in range(a + 1, len(chr_names)):
            first, second = chr_names[a], chr_names[b]
            calls = {}
            for r in sr:
                ab = r["FragName"] == first and r["FarFragName"] == second
                ba = r["FragName"] == second and r["FarFragName"] == first
                if not ab and not ba or r["Name"] in read_names:
                    continue
                read_names.add(r["Name"])
                call = ir._one_read(r, r["MatchedD"] == "+" if ab else r["MatchedFarD"] == "-", SPACER)
                if call is not None:
                    calls[call] = calls.get(call, 0) + 1
            out += "".join(f"{c}\tsupport: {n}\n" for c, n in sorted(calls.items()) if n >= 2)
    return out


CHR = ["chrA", "chrB", "chrC"]


def hand_read(name, chr_id, far_chr, strand, far_strand, close, far, seq=b"ACGTTGCAAC" * 4):
    """close / far: lists of (LengthStr, AbsLoc)"""
    return dict(Name=name, FragName=CHR[chr_id], FarFragName=CHR[far_chr], MatchedD=strand, MatchedFarD=far_strand, ReadLength=len(seq),
                UnmatchedSeq=seq.decode(), UP_Close=close, UP_Far=far, chr=chr_id, far_chr=far_chr)


def consume(tmp_path, tag, reads, int_pairs=False):
    """the tables of `reads` (dicts of hand_read) from the host statement, then the consumer over reads without points"""
    inp = build_input([dict(seq=r["UnmatchedSeq"].encode(), strand=ord(r["MatchedD"]), chr=r["chr"], rc_flag=0,
                            close=[(l, a, r["chr"], b"+") for l, a in r["UP_Close"]],
                            far=[(l, a, r["far_chr"], r["MatchedFarD"].encode()) for l, a in r["UP_Far"]]) for r in reads])
    t = statement(inp, hostlib.chr_ranks(CHR))
    prefix = str(tmp_path / tag)
    junction = [k for k, r in enumerate(reads) if r["UP_Far"] and r["FragName"] != r["FarFragName"]]
    hostlib.int_write_from_tables(prefix, [r["Name"] for r in reads], [r["FragName"] for r in reads], [r["FarFragName"] for r in reads],
                                  [r["UnmatchedSeq"].encode() for r in reads], junction, t["members"], t["calls"],
                                  repairs=hostlib.REPAIRS["int-pairs"] if int_pairs else 0, spacer=SPACER)
    return (open(prefix + "_INT").read() if os.path.exists(prefix + "_INT") else ""), t


def template(name, at, far_at, chr_id=0, far_chr=1, strand="+", far_strand="+"):
    return hand_read(name, chr_id, far_chr, strand, far_strand, [(20, SPACER + at)], [(20, SPACER + far_at)])


def test_consumer_duplicate_name_whose_first_read_has_no_call(tmp_path):
    # "dup" first comes without a call (9 + 9), then with one: the name is taken, the second is skipped and the call stays at 2
    reads = [hand_read("dup", 0, 1, "+", "+", [(9, SPACER + 500)], [(9, SPACER + 900)]), template("a", 500, 900), template("dup", 500, 900),
             template("b", 500, 900)]
    got, t = consume(tmp_path, "dup", reads)
    assert got == restated_lines(reads) == 'Anchor + chrA 500 - chrB 900 + ""\tsupport: 2\n'
    assert t["calls"]["n_reads"].tolist() == [3]                  # (the table counts members: names are the consumer's job)


def test_consumer_name_shared_across_pairs_with_and_without_int_pairs(tmp_path):
    # "x" is first seen on chrB -> chrC: without the repair the first pair (chrA, chrB) visits it and takes its name
    reads = [template("x", 700, 800, chr_id=1, far_chr=2), template("x", 500, 900), template("y", 500, 900), template("z", 700, 800, chr_id=1, far_chr=2),
             template("w", 700, 800, chr_id=1, far_chr=2)]
    got, _ = consume(tmp_path, "shared", reads)
    assert got == restated_lines(reads) == ""                     # chrA/chrB: only "y" counts; chrB/chrC is never looked at
    got, _ = consume(tmp_path, "shared_repair", reads, int_pairs=True)
    assert got == restated_lines(reads, int_pairs=True)
    assert got == 'Anchor + chrA 500 - chrB 900 + ""\tsupport: 2\nAnchor + chrB 700 - chrC 800 + ""\tsupport: 2\n'


def test_consumer_fallback_group_splits_by_its_bases(tmp_path):
    # three fallback reads with equal points and offsets: one call in the table; two carry the same bases, the third others
    s1, s2 = b"ACGTTGCAAC" * 4, b"ACGTTGCAAC" * 2 + b"TTTTT" + b"ACGTTGCAAC"[5:] + b"ACGTTGCAAC"
    mk = lambda name, seq: hand_read(name, 0, 1, "-", "-", [(15, SPACER + 500)], [(20, SPACER + 900)], seq=seq)
    reads = [mk("a", s1), mk("b", s2), mk("c", s1)]
    got, t = consume(tmp_path, "split", reads)
    assert t["calls"]["n_reads"].tolist() == [3] and int(t["calls"]["flags"][0]) & hostlib.INT_FALLBACK
    assert (int(t["calls"]["nt_off"][0]), int(t["calls"]["nt_len"][0])) == (20, 5)
    assert got == restated_lines(reads) == 'Anchor - chrA 500 + chrB 900 - "ACGTT"\tsupport: 2\n'
    # ... and a group of two that splits drops below 2: nothing is written
    got, t = consume(tmp_path, "split_below", reads[:2])
    assert t["calls"]["n_reads"].tolist() == [2] and got == restated_lines(reads[:2]) == ""


def test_consumer_orders_lines_by_the_call_string(tmp_path):
    # positions 9999 and 10000: the tables order them by number, the lines go out in string order ("10000" < "9999")
    reads = [template(f"r{k}", at, 900) for k, at in enumerate([9999, 10000, 9999, 10000])]
    got, t = consume(tmp_path, "order", reads)
    assert (t["calls"]["close_abs"] - SPACER).tolist() == [9999, 10000]
    assert got == restated_lines(reads) == 'Anchor + chrA 10000 - chrB 900 + ""\tsupport: 2\nAnchor + chrA 9999 - chrB 900 + ""\tsupport: 2\n'


def test_consumer_refuses_tables_that_point_outside(tmp_path):
    calls = np.zeros(1, dtype=hostlib.INT_CALL_DTYPE)
    calls["n_reads"] = 2
    with pytest.raises(ValueError):
        hostlib.int_write_from_tables(str(tmp_path / "bad"), ["a"], ["chrA"], ["chrB"], [b"ACGT"], [0], [0], calls)
    with pytest.raises(ValueError):
        hostlib.int_write_from_tables(str(tmp_path / "bad"), ["a"], ["chrA"], ["chrB"], [b"ACGT"], [0], [1], calls[:0])


# ------------------------------------------------------------------------------------------------ the synthetic set: -I from tables
@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    """tests/interchr_synth.py searched window by window by the oracle with the windows of its BreakDancer file (far ends on other
    chromosomes), and the lists of both classifiers over those points"""
    from oracle import pyoracle
    from pindel_amd import hostio
    from tests import interchr_synth as syn
    from tests.test_interchr_cpu import _text_route_expected
    tmp = tmp_path_factory.mktemp("int_synth")
    s = syn.make(str(tmp))
    csr, _ = _text_route_expected(s, tmp)
    chroms = hostio.load_fasta(s["fasta"])
    batch = hostio.read_pindel_text(s["reads_txt"], [n for n, _ in chroms], [len(q) - 200000 for _, q in chroms])
    mm = pyoracle.max_mismatch_table()
    co, cp, fo, fp, rc_flag = csr
    assert batch.n == len(co) - 1
    args = (chroms, batch.seq, batch.seq_off, batch.anchor_strand, batch.chr_id, rc_flag, co, cp, fo, fp, mm)
    return dict(tmp=tmp, s=s, csr=csr, mm=mm, var=hostlib.variant_candidates(*args), sv=hostlib.sv_candidates(*args), window_mbp=float(syn.WINDOW_MBP))


@pytest.mark.parametrize("threads", ["1", "16"])
def test_synthetic_set_through_the_tables_route(synth, monkeypatch, threads):
    from tests import golden_util as gu
    monkeypatch.setenv("PGH_THREADS", threads)
    s = synth["s"]
    st = ec.with_fields(hostlib.default_settings(synth["mm"]), window_mbp=synth["window_mbp"], report_interchromosomal=1)
    out = {}
    for rr in (False, True):
        prefix = str(synth["tmp"] / f"int_{threads}_{rr}")
        hostlib.call_from_points(s["fasta"], s["reads_txt"], prefix, st, *synth["csr"], variant_candidates=synth["var"], sv_candidates=synth["sv"],
                                 report_reads=rr)
        out[rr] = {suf: open(f"{prefix}_{suf}", "rb").read() for suf in tuple(gu.SUFFIXES) + ("INT", "INT_final")}
        # the host-side pin: with report_reads every window's _INT comes from its junction tables, after the reads were stripped
        assert hostlib.last_int_table_windows() == (hostlib.last_report_windows() if rr else 0)
        if rr:
            assert hostlib.last_report_windows() == len(hostlib.last_event_windows()) > 3 and hostlib.last_event_fallback_windows() == 0
    assert out[True] == out[False]
    # lists cut to 0 pairs: every window with a listed pair falls back and reports _INT from copies made at that point; the bytes stay
    from tests.test_report_reads_cpu import cut_lists
    prefix = str(synth["tmp"] / f"int_{threads}_cut")
    hostlib.call_from_points(s["fasta"], s["reads_txt"], prefix, st, *synth["csr"], variant_candidates=cut_lists(synth["var"], 0),
                             sv_candidates=cut_lists(synth["sv"], 0), report_reads=True)
    assert {suf: open(f"{prefix}_{suf}", "rb").read() for suf in out[False]} == out[False]
    assert hostlib.last_event_fallback_windows() > 0
    assert hostlib.last_int_table_windows() + hostlib.last_event_fallback_windows() == len(hostlib.last_event_windows())
    assert len(out[True]["INT"]) > 0 and len(out[True]["INT_final"]) > 0 and out[True]["INT"].count(b"support: ") >= 3
