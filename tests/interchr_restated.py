"""An independent restatement of what Pindel 0.2.5b9 does for -I (--report_interchromosomal_events), written from the
reference's text and sharing no helper with the C++ under test (pindel_amd/csrc/host/pg_rp.hpp, pg_host_int.cpp):

  rp_interchr(pairs, spacer)   interchromosomal read pairs of one window -> BreakDancer-like events + their _RP lines
                               (ModifyRP_InterChr / Summarize_InterChr / the second half of BDData::UpdateBD, src/bddata.cpp)
  int_lines(reads, spacer)     the window's split reads -> the lines appended to <prefix>_INT
                               (the copy at src/pindel.cpp:1905-1917 + SortAndReportInterChromosomalEvents, src/reporter.cpp)
  int_final(text)              the text of <prefix>_INT -> the text of <prefix>_INT_final (MergeInterChr, src/pindel.cpp)

Everything is kept literal, the quadratic loops and the loop over all chromosome-name pairs included; unsigned 32-bit
arithmetic is spelled out where the reference relies on it."""

M32 = 0xFFFFFFFF


def _abs_u(a, b):
    """abs(a - b) on unsigned operands, the difference taken as int"""
    d = (a - b) & M32
    if d >= 1 << 31:
        d -= 1 << 32
    return abs(d)


# ------------------------------------------------------------------------------------------------ read pairs
def _initialize_a1b1(v):
    for r in v:
        dist, rl = r["InsertSize"] & M32, r["ReadLength"]
        if r["DA"] == "+":
            r["PosA"] = r["PosA"] - rl * 2 if r["PosA"] > rl * 2 else 1
            r["PosA1"] = r["PosA"] + dist + rl * 2
        else:
            r["PosA"] = r["PosA"] - dist if r["PosA"] > dist else 1
            r["PosA1"] = r["PosA"] + dist + rl
        if r["DB"] == "+":
            r["PosB"] = r["PosB"] - rl * 2 if r["PosB"] > rl * 2 else 1
            r["PosB1"] = r["PosB"] + dist + rl
        else:
            r["PosB"] = r["PosB"] - dist if r["PosB"] > dist else 1
            r["PosB1"] = r["PosB"] + dist + rl


def _process_same_strand(f, s):
    if ((s["PosA1"] - s["PosA"]) & M32) > 10000 or ((s["PosB1"] - s["PosB"]) & M32) > 10000:
        return
    if ((f["DA"] == "+" and f["PosA"] < s["PosA"] < f["PosA1"] < s["PosA1"]) or
            (f["DA"] == "-" and f["PosA"] < s["PosA1"] < f["PosA1"] and s["PosA"] < f["PosA"])):
        f["PosA"], f["PosA1"] = s["PosA"], s["PosA1"]
    if ((f["DB"] == "+" and f["PosB"] < s["PosB"] < f["PosB1"] < s["PosB1"]) or
            (f["DB"] == "-" and s["PosB"] < f["PosB"] < s["PosB1"] < f["PosB1"])):
        f["PosB"], f["PosB1"] = s["PosB"], s["PosB1"]


def _update_first_on_second(f, s):
    if f["ChrNameA"] == s["ChrNameA"] and f["ChrNameB"] == s["ChrNameB"]:
        if f["DA"] == s["DA"] and f["DB"] == s["DB"]:
            _process_same_strand(f, s)
    elif f["ChrNameA"] == s["ChrNameB"] and f["ChrNameB"] == s["ChrNameA"]:
        if f["DA"] == s["DB"] and f["DB"] == s["DA"]:
            t = dict(s, DA=s["DB"], DB=s["DA"], PosA=s["PosB"], PosA1=s["PosB1"], PosB=s["PosA"], PosB1=s["PosA1"])
            _process_same_strand(f, t)


def rp_interchr(pairs, spacer=100000):
    """pairs: dicts with ChrNameA, ChrNameB, DA, DB, PosA, PosB, InsertSize, ReadLength, Tag, in the order the reader found
    them (no two with the same (PosA, PosB): the reference's std::sort is not stable).
    -> (events [(chr1, pos1, pos1b, chr2, pos2, pos2b)], the _RP text)"""
    v = []
    for p in pairs:
        v.append(dict(p, OriginalPosA=p["PosA"], OriginalPosB=p["PosB"], PosA1=0, PosB1=0, NumberOfIdentical=0, Report=False,
                      Visited=False, Tags=[p["Tag"]]))
    if not v:
        return [], ""
    v.sort(key=lambda r: (-r["OriginalPosA"], -r["OriginalPosB"]))                 # Compare2RP
    _initialize_a1b1(v)
    for first in range(len(v) - 1):                                                # serial; stops before the last
        for second in range(len(v)):
            _update_first_on_second(v[first], v[second])
    for first in range(len(v) - 1):                                                # Summarize_InterChr
        f = v[first]
        if f["Visited"]:
            continue
        f["NumberOfIdentical"] = 0
        for second in range(first + 1, len(v)):
            s = v[second]
            if s["Visited"]:
                continue
            if all(f[k] == s[k] for k in ("ChrNameA", "ChrNameB", "PosA", "PosB", "DA", "DB")):
                f["NumberOfIdentical"] += 1
                if f["Tags"]:
                    f["Tags"] += s["Tags"]
                    s["Tags"] = []
                s["Visited"] = True
        f["Report"] = f["NumberOfIdentical"] >= 5
    events, text = [], []
    for r in v:
        if not r["Report"]:
            continue
        shift = r["InsertSize"] & M32
        f1, f2 = (r["PosA"] + spacer) & M32, (r["PosA1"] + spacer) & M32
        s1, s2 = (r["PosB"] + spacer) & M32, (r["PosB1"] + spacer) & M32
        if f1 > f2:
            f1, f2 = f2, f1
        if r["DA"] == "+" and f1 > shift:
            f1 -= shift
        elif shift * 2 < spacer:
            f2 += shift
        if s1 > s2:
            s1, s2 = s2, s1
        if r["DB"] == "+" and s1 > shift:
            s1 -= shift
        elif shift * 2 < spacer:
            s2 += shift
        if r["ChrNameA"] == "" or r["ChrNameB"] == "":
            continue
        events.append((r["ChrNameA"], f1, f2, r["ChrNameB"], s1, s2))
        line = (f'{r["ChrNameA"]}\t{f1 - spacer if f1 > spacer else 1}\t{f2 - spacer}\t{r["DA"]}\t{f2 - f1}\t'
                f'{r["ChrNameB"]}\t{s1 - spacer if s1 > spacer else 1}\t{s2 - spacer}\t{r["DB"]}\t0\t'
                f'\tSupport: {r["NumberOfIdentical"]}')
        tags = sorted(r["Tags"])                                                   # DisplayBDSupportPerSample
        count, cur = 1, tags[0]
        for t in tags[1:]:
            if t == cur:
                count += 1
            else:
                line += f"\t{cur} {count}"
                cur, count = t, 1
        line += f"\t{cur} {count}"
        text.append(line + "\n")
    return events, "".join(text)


# ------------------------------------------------------------------------------------------------ _INT
def collect(reads):
    """the copy made after UpdateFarFragName: reads with a far end on another chromosome, in order"""
    return [r for r in reads if r["UP_Far"] and r["FragName"] != r["FarFragName"]]


def _same(d):
    return d if d in "+-" and d else ""


def _other(d):
    return {"+": "-", "-": "+"}.get(d, "")


def _one_read(r, ascending, spacer):
    """-> the call string or None.  UP_Close / UP_Far: lists of (LengthStr, AbsLoc)."""
    close, far, rl = r["UP_Close"], r["UP_Far"], r["ReadLength"]
    used, bp_left, bp_right, inserted = False, None, None, None
    if ascending:
        for ci in range(len(close)):
            if used:
                break
            for fi in range(len(far) - 1, -1, -1):
                if used:
                    break
                if close[ci][0] + far[fi][0] == rl:
                    used, bp_left, bp_right, inserted = True, close[ci][1] - spacer, far[fi][1] - spacer, '""'
    else:
        for ci in range(len(close) - 1, -1, -1):
            if used:
                break
            for fi in range(len(far)):
                if used:
                    break
                if close[ci][0] + far[fi][0] == rl:
                    used, bp_left, bp_right, inserted = True, close[ci][1] - spacer, far[fi][1] - spacer, '""'
    if not used:
        eff = close[-1][0] + far[-1][0]
        if eff >= 30 and close[-1][0] >= 10 and far[-1][0] >= 10:
            n = (rl - eff) & M32
            inserted = '"' + r["UnmatchedSeq"][far[-1][0]:far[-1][0] + n] + '"'
            bp_left, bp_right = close[-1][1] - spacer, far[-1][1] - spacer
        else:
            return None
    return (f'Anchor {_same(r["MatchedD"])} {r["FragName"]} {bp_left} {_other(r["MatchedD"])} {r["FarFragName"]} {bp_right} '
            f'{_same(r["MatchedFarD"])} {inserted}')


def int_lines(reads, spacer=100000):
    """reads: the window's reads that kept a close end, in input order: dicts with Name, FragName, FarFragName, MatchedD,
    MatchedFarD, ReadLength, UnmatchedSeq, UP_Close, UP_Far.  -> (text appended to _INT, number of reads collected)"""
    sr = collect(reads)
    if not sr:
        return "", 0
    chr_names = sorted({r["FragName"] for r in sr} | {r["FarFragName"] for r in sr})
    read_names, calls = set(), {}
    for a in range(len(chr_names)):
        for b in range(a + 1, len(chr_names)):
            first, second = chr_names[a], chr_names[b]
            for r in sr:
                if r["Name"] in read_names:                      # seen (= visited) before: skipped, matching or not
                    continue
                read_names.add(r["Name"])
                call = None
                if r["FragName"] == first and r["FarFragName"] == second:
                    call = _one_read(r, r["MatchedD"] == "+", spacer)
                elif r["FragName"] == second and r["FarFragName"] == first:
                    call = _one_read(r, r["MatchedFarD"] == "-", spacer)
                if call is not None:
                    calls[call] = calls.get(call, 0) + 1
    return "".join(f"{c}\tsupport: {n}\n" for c, n in sorted(calls.items()) if n >= 2), len(sr)


# ------------------------------------------------------------------------------------------------ _INT_final
class _In:
    """operator>> on a text: words, single characters and unsigned numbers, white space skipped before each"""

    def __init__(self, text):
        self.t, self.i, self.ok = text, 0, True

    def _skip(self):
        while self.i < len(self.t) and self.t[self.i].isspace():
            self.i += 1
        if self.i >= len(self.t):
            self.ok = False

    def word(self):
        self._skip()
        j = self.i
        while j < len(self.t) and not self.t[j].isspace():
            j += 1
        w, self.i = self.t[self.i:j], j
        return w

    def char(self):
        self._skip()
        if not self.ok:
            return ""
        self.i += 1
        return self.t[self.i - 1]

    def unsigned(self):
        self._skip()
        j = self.i
        while j < len(self.t) and self.t[j].isdigit():
            j += 1
        if j == self.i:
            self.ok = False
            return 0
        v, self.i = int(self.t[self.i:j]), j
        return v


def int_final(text):
    calls, s = [], _In(text)
    while True:
        s.word()
        c = dict(AnchorD=s.char(), FirstChrName=s.word(), FirstPos=s.unsigned(), FirstD=s.char(), SecondChrName=s.word(),
                 SecondPos=s.unsigned(), SecondD=s.char(), Seq=s.word())
        s.word()
        c["N"] = s.unsigned()
        if not s.ok:
            break
        calls.append(c)
    cutoff, out = 2, []

    def infor(c):
        return (f'{c["AnchorD"]}\t{c["FirstChrName"]}\t{c["FirstPos"]}\t{c["FirstD"]}\t{c["SecondChrName"]}\t{c["SecondPos"]}\t'
                f'{c["SecondD"]}\t{c["Seq"]}\t{c["N"]}')
    if len(calls) == 0:
        return ""
    if len(calls) < 2 and calls[0]["N"] >= cutoff * 2:
        c = calls[0]
        out.append(f'{c["FirstChrName"]}\t{c["FirstPos"]}\t{c["SecondChrName"]}\t{c["SecondPos"]}\t{c["Seq"]}\t{c["N"]}\t' + infor(c))
    for a in range(len(calls)):
        reported = False
        for b in range(a, len(calls)):
            if a == b:
                continue
            x, y = calls[a], calls[b]
            if x["FirstChrName"] == y["FirstChrName"] and x["SecondChrName"] == y["SecondChrName"]:
                if (_abs_u(x["FirstPos"], y["FirstPos"]) < 10 and _abs_u(x["SecondPos"], y["SecondPos"]) < 10 and
                        x["N"] + y["N"] >= cutoff):
                    out.append(f'chr\t{x["FirstChrName"]}\tpos\t{((x["FirstPos"] + y["FirstPos"]) & M32) // 2}\tchr\t{x["SecondChrName"]}\t'
                               f'pos\t{((x["SecondPos"] + y["SecondPos"]) & M32) // 2}\tseq\t{x["Seq"]}\tsupport\t{x["N"] + y["N"]}\tINFOR\t'
                               + infor(x) + "\t" + infor(y))
                    reported = True
                    break
        if not reported and calls[a]["N"] >= cutoff * 2:
            x = calls[a]
            out.append(f'chr\t{x["FirstChrName"]}\tpos\t{x["FirstPos"]}\tchr\t{x["SecondChrName"]}\tpos\t{x["SecondPos"]}\tseq\t{x["Seq"]}\t'
                       f'support\t{x["N"]}\tINFOR\t' + infor(x))
    return "".join(line + "\n" for line in out)
