"""Independent restatements for the tests of `--repair`, written from the reference's text and sharing
nothing with the C++ under test:

  int_lines_all_pairs(reads, spacer)   SortAndReportInterChromosomalEvents (src/reporter.cpp:2428-2665) as --repair int-pairs
                                       runs it: every chromosome-name pair, a read's name entered only when the read matches
                                       the pair in hand, calls counted and written pair by pair
  pair_state(records, ...)             build_record_RP_Discovery + the part of BDData::UpdateBD before its clear()
                                       (src/reader.cpp:1003-1094, src/bddata.cpp:138-560, 646-733): the same-chromosome
                                       discordant pairs of a window in the state IsGoodINV would have met them in
  is_good_inv(pairs, ...)              IsGoodINV's loop (src/output_sorter.cpp:283-365), both orders of the positions spelled
                                       out as there; after_loop=True adds the repair's comparison after the loop
  depth_array_mapq(records, ...)       the pileup of src/bam2depth.cpp, position by position, with its MAPQ floor acting"""
import numpy as np

from tests import bam_writer as bw
from tests import interchr_restated as ir

M32 = 0xFFFFFFFF
F = bw.FLAG


# ------------------------------------------------------------------------------------------------ int-pairs
def int_lines_all_pairs(reads, spacer=100000):
    """reads: as interchr_restated.int_lines takes them.  -> (text appended to _INT, lines of the first pair alone)"""
    sr = ir.collect(reads)
    if not sr:
        return "", ""
    chr_names = sorted({r["FragName"] for r in sr} | {r["FarFragName"] for r in sr})
    read_names, text, first_text = set(), "", None
    for a in range(len(chr_names)):
        for b in range(a + 1, len(chr_names)):
            first, second = chr_names[a], chr_names[b]
            calls = {}
            for r in sr:
                if r["FragName"] == first and r["FarFragName"] == second:
                    ascending = r["MatchedD"] == "+"
                elif r["FragName"] == second and r["FarFragName"] == first:
                    ascending = r["MatchedFarD"] == "-"
                else:
                    continue                                     # not of this pair: its name is not entered
                if r["Name"] in read_names:
                    continue
                read_names.add(r["Name"])
                call = ir._one_read(r, ascending, spacer)
                if call is not None:
                    calls[call] = calls.get(call, 0) + 1
            lines = "".join(f"{c}\tsupport: {n}\n" for c, n in sorted(calls.items()) if n >= 2)
            if first_text is None:
                first_text = lines
            text += lines
    return text, first_text


# ------------------------------------------------------------------------------------------------ inv-pairs
def _i32(x):
    x &= M32
    return x - (1 << 32) if x >= 1 << 31 else x


def _uabs(a, b):
    return abs(_i32(a - b))


def pair_state(records_per_bam, insert_sizes, tid, ws, we, min_q=0):
    """records_per_bam: the records of every BAM of the configuration, in its order and in file order; insert_sizes: theirs.
    -> the list UpdateBD clears, in its order: dicts with DA, DB, PosA, PosB, InsertSize, ReadLength"""
    rp = []
    for records, isz in zip(records_per_bam, insert_sizes):
        for r in records:
            if r["tid"] != tid or r["flag"] & F["UNMAP"] or not r.get("cigar"):
                continue
            end = r["pos"] + sum(n for op, n in r["cigar"] if op in (0, 2, 3, 7, 8))
            if not (r["pos"] < we and end > ws):
                continue
            f = r["flag"]
            if not f & F["PAIRED"] or r.get("mapq", 0) < min_q or f & F["MUNMAP"]:
                continue
            rev, mrev = bool(f & F["REVERSE"]), bool(f & F["MREVERSE"])
            if r.get("mtid", tid) != tid or not (abs(r.get("tlen", 0)) > 3 * isz + 1000 or rev == mrev):
                continue
            d = dict(DA="-" if rev else "+", DB="-" if mrev else "+", PosA=r["pos"], PosB=r["mpos"], ReadLength=len(r["seq"]),
                     InsertSize=isz)
            if not d["PosA"] < d["PosB"]:
                d["DA"], d["DB"], d["PosA"], d["PosB"] = d["DB"], d["DA"], d["PosB"], d["PosA"]
            d["OA"], d["OB"] = d["PosA"], d["PosB"]
            rp.append(d)
    rp.sort(key=lambda d: (d["PosA"], d["PosB"]))                    # SortByFirstAndThenSecondCoordinate
    rp.sort(key=lambda d: (-d["OA"], -d["OB"]))                      # ModifyRP: Compare2RP
    for d in rp:                                                     # InitializeA1B1
        D, L = d["InsertSize"], d["ReadLength"]
        if d["DA"] == "+":
            d["PosA"] = d["PosA"] - 2 * L if d["PosA"] > 2 * L else 1
            d["A1"] = d["PosA"] + D + 2 * L
        else:
            d["PosA"] = d["PosA"] - D if d["PosA"] > D else 1
            d["A1"] = d["PosA"] + D + L
        if d["DB"] == "+":
            d["PosB"] = d["PosB"] - 2 * L if d["PosB"] > 2 * L else 1
        else:
            d["PosB"] = d["PosB"] - D if d["PosB"] > D else 1
        d["B1"] = d["PosB"] + D + L

    def overlap(a, b):                                               # RecipicalOverlap
        if max(_uabs(a["PosA"], a["A1"]), _uabs(a["PosB"], a["B1"]), _uabs(b["PosA"], b["A1"]), _uabs(b["PosB"], b["B1"])) > 1000:
            return False
        fa, fb = sorted(((a["PosA"] + a["A1"]) // 2, (a["PosB"] + a["B1"]) // 2))
        sa, sb = sorted(((b["PosA"] + b["A1"]) // 2, (b["PosB"] + b["B1"]) // 2))
        if a["DA"] != b["DA"] or a["DB"] != b["DB"] or fa > sb + 200 or fb + 200 < sa:
            return False
        c = 0.9
        if fa <= sa and sb <= fb and (sb - sa) / (fb - fa) >= c:
            return True
        if sa <= fa and fb <= sb and (fb - fa) / (sb - sa) >= c:
            return True
        if fa <= sa <= fb <= sb and (fb - sa) / (fb - fa) >= c and (fb - sa) / (sb - sa) >= c:
            return True
        if sa <= fa <= sb <= fb and (sb - fa) / (fb - fa) >= c and (sb - fa) / (sb - sa) >= c:
            return True
        return False

    for a in rp:                                                     # the double loop of ModifyRP, serial
        for b in rp:
            if a is b or not overlap(a, b):
                continue
            if b["A1"] - b["PosA"] > 10000 or b["B1"] - b["PosB"] > 10000:
                continue
            if (a["DA"] == "+" and a["PosA"] < b["PosA"] < a["A1"] < b["A1"]) or \
                    (a["DA"] == "-" and a["PosA"] < b["A1"] < a["A1"] and b["PosA"] < a["PosA"]):
                a["PosA"], a["A1"] = b["PosA"], b["A1"]
            if (a["DB"] == "+" and a["PosB"] < b["PosB"] < a["B1"] < b["B1"]) or \
                    (a["DB"] == "-" and b["PosB"] < a["PosB"] < b["B1"] < a["B1"]):
                a["PosB"], a["B1"] = b["PosB"], b["B1"]
    for d in rp:
        if d["DA"] == "+":
            d["PosA"] += d["ReadLength"]
        if d["DB"] == "+":
            d["PosB"] += d["ReadLength"]
    # (Summarize changes counts, tags and flags only: nothing the loop below reads)
    return rp


def is_good_inv(pairs, support, real_start, real_end, after_loop=True):
    """-> (verdict, CountLeft, CountRight) for an event of `support` reads of two read lengths or more"""
    cutoff = max(support // 2, 5)
    left_good = right_good = False
    n_left = n_right = 0
    u = lambda x: x & M32
    for p in pairs:
        if n_left >= cutoff:
            left_good = True
        if n_right >= cutoff:
            right_good = True
        if left_good and right_good:
            return True, n_left, n_right
        if p["DA"] != p["DB"]:
            continue
        A, B, L, E = p["PosA"], p["PosB"], p["ReadLength"], p["InsertSize"]
        if p["DA"] == "+":
            if A < B:
                if A < u(real_start + L) and u(B + L) > real_start and B < u(real_end + L):
                    if u(A + E + L) > real_start:
                        if u(B + E + L) > real_end:
                            n_left += 1
            else:
                if B < u(real_start + L) and u(A + L) > real_start and A < u(real_end + L):
                    if u(B + E + L) > real_start:
                        if u(A + E + L) > real_end:
                            n_left += 1
        else:
            if A < B:
                if u(A + L) > real_start and A < u(real_end + L) and u(B + L) > real_end:
                    if A < u(real_start + E + L):
                        if B < u(real_end + E + L):
                            n_right += 1
            else:
                if u(B + L) > real_start and B < u(real_end + L) and u(A + L) > real_end:
                    if B < u(real_start + E + L):
                        if A < u(real_end + E + L):
                            n_right += 1
    if after_loop and n_left >= cutoff and n_right >= cutoff:
        return True, n_left, n_right
    return False, n_left, n_right


# ------------------------------------------------------------------------------------------------ depth-mapq
_SKIP = F["UNMAP"] | F["SECONDARY"] | F["QCFAIL"] | F["DUP"]


def depth_array_mapq(records, tid, length, min_mapq):
    """per position: the kept records of MAPQ >= min_mapq with an M / = / X base there"""
    depth = np.zeros(length, dtype=np.int64)
    for r in records:
        if r["tid"] != tid or r["flag"] & _SKIP or not r.get("cigar") or r.get("mapq", 0) < min_mapq:
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
