"""The inputs and the host half of the classifier parity hunt (scripts/fuzz_classifier.py, tests/test_classifier_fuzz_cpu.py); importing
this module touches neither the GPU nor a library.

fuzz_input(seed) draws what scripts/fuzz_parity.py draws -- a repeat-ridden reference, random search parameters, mixed read lengths,
re-anchored reads, bytes outside ACGTN from seed 600000 on, window clusters on other chromosomes -- and on top of it reads of planted
events on both strands, junction reads into the other chromosomes, reads drawn several times, and the arguments of every part of the
classifier.  HostChain runs the plain-loop host statements of hostlib over the lists of one search, each fed what the one before it
delivered; tally() counts what they hold."""
import types

import numpy as np

from pindel_amd import hostlib, synth
from pindel_amd.binding import WINDOW_DTYPE
from pindel_amd.hostio import ReadBatch
from scripts.fuzz_parity import SPACER, nasty_reference, random_params

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTN", b"TGCAN"):
    _COMP[_a] = _b
SEARCHES = ("search_device", "pack_search_device", "search_table_device")


def _revcomp(a):
    return _COMP[a][::-1]


def _junk_bytes(rng, batch):
    """bytes outside ACGTN at the start, the end or inside of one read in twelve (the stream of scripts/fuzz_parity.py from seed
    600000 on): the reads the search shortens (rc_flag 2) or strips of their leading bytes when it reverse-complements them"""
    junk = np.frombuffer(b"RYKMSWBDHVrykmacgtn*=.", dtype=np.uint8)
    off = batch.seq_off.astype(np.int64)
    for i in np.nonzero(rng.random(batch.n) < 1.0 / 12)[0]:
        a, b = int(off[i]), int(off[i + 1])
        how = int(rng.integers(0, 6))
        k1, k2 = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        if how in (0, 2, 5):
            batch.seq[a:a + k1] = junk[rng.integers(0, len(junk), k1)]
        if how in (1, 2, 5):
            batch.seq[b - k2:b] = junk[rng.integers(0, 10, k2)]
        if how in (3, 4, 5):
            m = int(rng.integers(1, 4))
            batch.seq[rng.integers(a, b, m)] = junk[rng.integers(0, len(junk), m)]
        if how == 4 and b - a > 8:
            batch.seq[a + 1:b] = _revcomp(batch.seq[a + 1:b].copy())
            batch.seq[a] = junk[rng.integers(0, 10)]
        last = batch.seq[b - 1]
        if not ((48 <= last <= 57) or (65 <= last <= 90) or (97 <= last <= 122)):
            batch.seq[b - 1] = ord("R")


def _place(batch, i, forward, plus, left_start, right_end, isz, rng):
    """read i becomes `forward` (reference orientation) as the search receives it: a '+' anchor sits upstream of the read, which is
    handed over reverse-complemented; a '-' anchor downstream (positions without the spacer)"""
    a = int(batch.seq_off[i])
    batch.seq[a:a + len(forward)] = _revcomp(forward) if plus else forward
    slack = int(rng.integers(0, max(isz - len(forward) - 20, 1)))
    batch.anchor_strand[i] = ord("+") if plus else ord("-")
    batch.anchor_pos[i] = max((left_start - slack if plus else right_end + slack) - SPACER, 0)


def _planted_events(rng, ref, length, batch, slots, isz):
    """Reads of planted events written over the reads `slots`: per event 2 to 6 reads with their own split points, on both anchor
    strands -- deletions, short insertions, tandem duplications and tandem duplications with inserted bases, the kinds of the four
    event tables.  (Copies of one read share its anchor strand: only reads like these give an event members of both strands.)"""
    r = np.frombuffer(ref, dtype=np.uint8)
    lens = batch.lengths()
    at = 0
    while at < len(slots):
        kind = int(rng.integers(0, 4))
        size = int(rng.choice([1, 7, 60, 900])) if kind == 0 else int(rng.integers(1, 12)) if kind == 1 else int(rng.integers(320, 2000))
        nt = _ACGT[rng.integers(0, 4, size if kind == 1 else int(rng.integers(1, 6)))]
        bp = SPACER + int(rng.integers(4000, length - 4000))
        for i in slots[at:at + int(rng.integers(2, 7))]:
            at += 1
            n = int(lens[i])
            sp = int(rng.integers(12, n - 11))
            left = r[bp - sp:bp]
            if kind == 0:
                fwd, right_end = np.concatenate([left, r[bp + size:bp + size + n - sp]]), bp + size + n - sp
            elif kind == 1:
                ins = nt[:max(min(len(nt), n - sp - 10), 1)]
                fwd, right_end = np.concatenate([left, ins, r[bp:bp + n - sp - len(ins)]]), bp + n - sp - len(ins)
            else:
                ins = nt[:max(min(len(nt), n - sp - 10), 1)] if kind == 3 else nt[:0]
                fwd, right_end = np.concatenate([left, ins, r[bp - size:bp - size + n - sp - len(ins)]]), bp
            _place(batch, i, fwd, bool(rng.random() < 0.5), bp - sp, right_end, isz, rng)


def _junction_reads(rng, chroms, length, batch, slots, isz):
    """Junction reads written over the reads `slots`: one part from chromosome 0 beside the anchor, the other from another
    chromosome, in either orientation, with 0 to 5 bases between them in two reads of five (the fallback call of -I); returns the
    window that holds each read's far part"""
    refs = [np.frombuffer(s, dtype=np.uint8) for _, s in chroms]
    lens = batch.lengths()
    win = np.zeros(len(slots), dtype=WINDOW_DTYPE)
    for w, i in enumerate(slots):
        n = int(lens[i])
        k = int(rng.integers(min(12, n // 2), n - min(12, n // 2) + 1))
        nt = _ACGT[rng.integers(0, 4, int(rng.integers(1, 6)) if rng.random() < 0.4 and n >= 40 else 0)]
        m = max(n - k - len(nt), 1)
        nt = nt[:n - k - m]
        p = SPACER + int(rng.integers(2 * isz + 400, length - 2 * isz - 400))
        c = int(rng.integers(1, len(chroms)))
        q = SPACER + int(rng.integers(500, len(chroms[c][1]) - 2 * SPACER - 500 - m))
        far = refs[c][q:q + m]
        if rng.random() < 0.5:
            far = _revcomp(far)
        plus = bool(rng.random() < 0.5)
        fwd = np.concatenate([refs[0][p - k:p], nt, far]) if plus else np.concatenate([far, nt, refs[0][p:p + k]])
        _place(batch, i, fwd, plus, p - k, p + k, isz, rng)
        win[w] = (c, q - int(rng.integers(50, 400)), q + m + int(rng.integers(50, 400)))
    return win


def _csr_gather(off, data, idx):
    off = off.astype(np.int64)
    cnt = off[idx + 1] - off[idx]
    new = np.concatenate([[0], np.cumsum(cnt)])
    take = np.repeat(off[idx] - new[:-1], cnt) + np.arange(int(new[-1]), dtype=np.int64)
    return new.astype(np.uint64), data[take]


def _first_occurrence(labels):
    """labels renumbered by first occurrence, as hostlib.name_ids numbers names"""
    _, first, inv = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    return rank[inv].astype(np.uint32)


def fuzz_input(seed, n_reads=1500):
    """Everything one iteration of the hunt needs, drawn from np.random.default_rng(seed).  Seed streams as in scripts/fuzz_parity.py
    (from 200000: wide parameter ranges; 300000-399999: Pindel's default search parameters; from 600000: bytes outside ACGTN), and
    400000-499999: always two or three chromosomes (elsewhere a third of the seeds).  Returns a namespace: chroms, batch, kw (engine
    keyword arguments), bd / bd_off (None without windows), name_id, search (a name of SEARCHES), window (EventWindow keyword
    arguments), settings (-e, -d, -v), max_listed, li (lo, hi), dd (seg_first, seg_strand, min_bp_support, min_map_distance) and
    what describes the draw (lens, isz, n_copies, n_planted, n_junction)."""
    rng = np.random.default_rng(seed)
    length = int(rng.integers(150_000, 400_000))
    ref = nasty_reference(rng, length)
    chroms = [("f", ref)]
    wide = seed >= 200000
    kw = random_params(rng, wide)
    if 300000 <= seed < 400000:
        kw = {k: v for k, v in kw.items() if k in ("max_mismatch_rate", "seq_error_rate", "sensitivity")}
    lens = sorted(set(int(x) for x in rng.choice([24, 36, 50, 64, 76, 100, 101, 128, 129, 150, 192, 200, 250, 300], size=int(rng.integers(1, 4)))))
    isz = int(rng.choice([120, 200, 350, 480, 500, 700, 800, 1200] if wide else [200, 350, 500, 800]))
    batch = synth.make_reads(ref, n_reads, seed=seed + 1, read_lens=lens, insert_size=isz, error_rate=float(rng.choice([0.0, 0.01, 0.03])),
                             n_rate=float(rng.choice([0.0, 0.001, 0.02])), max_del=int(rng.choice([50, 2000, 20000])))
    n = n_reads
    k = n // 3                                             # re-anchored at random places: windows full of repeats, mostly no close end
    batch.anchor_pos[:k] = rng.integers(2 * isz + 10, length - 2 * isz - 10, k).astype(np.int32)
    multi = 400000 <= seed < 500000 or rng.random() < 0.34
    if multi:
        for name in ("g", "h")[:int(rng.integers(1, 3))]:
            chroms.append((name, nasty_reference(rng, int(rng.integers(60_000, 150_000)))))
    # planted events and junction reads take the places of reads behind the re-anchored third
    spare = k + rng.permutation(n - k)
    planted = spare[:n // 6]
    junction = spare[n // 6:n // 6 + n // 8] if multi else spare[:0]
    _planted_events(rng, ref, length, batch, planted, isz)
    bd = bd_off = None
    if multi:
        jwin = _junction_reads(rng, chroms, length, batch, junction, isz)
        cnt = rng.integers(0, 5, n)
        cnt[rng.random(n) < 0.3] = 0
        owner = np.repeat(np.arange(n), cnt)
        w = np.zeros(len(owner), dtype=WINDOW_DTYPE)
        other = rng.random(len(owner)) < 0.2
        w["chr_id"] = np.where(other, rng.integers(1, len(chroms), len(owner)), 0)
        size = np.array([len(s) for _, s in chroms])[w["chr_id"]]
        centre = np.where(other, rng.integers(SPACER + 300, 1 << 30, len(owner)) % (size - 2 * SPACER - 600) + SPACER + 300,
                          batch.anchor_pos[owner].astype(np.int64) + SPACER + rng.integers(-30000, 30000, len(owner)))
        centre = np.clip(centre, SPACER + 300, size - SPACER - 300)
        half = rng.integers(20, 1500, len(owner))
        w["start"] = np.maximum(centre - half, 1)
        w["end"] = np.minimum(centre + half, size - 1)
        w["start"][rng.random(len(owner)) < 0.03] = -1
        # a junction read's own window at a random place of its cluster
        owner = np.concatenate([owner, junction])
        order = np.argsort(owner + 0.98 * rng.random(len(owner)), kind="stable")
        bd = np.concatenate([w, jwin])[order]
        bd_off = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=n))]).astype(np.uint64)
    if seed >= 600000:
        _junk_bytes(rng, batch)
    # reads drawn 2 to 6 times: a source's copies and the single reads, shuffled through the batch
    share = float(rng.choice([0.2, 0.35, 0.5]))
    copies = rng.integers(2, 7, n)
    n_src = int(np.searchsorted(np.cumsum(copies), share * n))
    perm = rng.permutation(n)
    total = int(copies[:n_src].sum())
    origin = np.concatenate([np.repeat(perm[:n_src], copies[:n_src]), perm[n_src:n_src + n - total]])
    is_copy = np.arange(n) < total
    same_name = np.repeat(rng.random(n_src) < 0.5, copies[:n_src])
    label = np.where(is_copy & np.concatenate([same_name, np.zeros(n - total, dtype=bool)]), origin, n + np.arange(n))
    shuffle = rng.permutation(n)
    origin, is_copy, label = origin[shuffle], is_copy[shuffle], label[shuffle]
    seq_off, seq = _csr_gather(batch.seq_off, batch.seq, origin)
    seq = seq.copy()
    out = ReadBatch(seq=seq, seq_off=seq_off, anchor_strand=batch.anchor_strand[origin].copy(), anchor_pos=batch.anchor_pos[origin].copy(),
                    insert_size=batch.insert_size[origin].copy(), chr_id=batch.chr_id[origin].copy())
    start, ln = seq_off[:-1].astype(np.int64), np.diff(seq_off.astype(np.int64))
    n_sub = np.where(is_copy, rng.integers(0, 4, n), 0)
    for s in range(3):                                     # each copy its own 0 to 3 substitutions
        hit = np.nonzero(n_sub > s)[0]
        seq[start[hit] + rng.integers(0, ln[hit])] = _ACGT[rng.integers(0, 4, len(hit))]
    moved = is_copy & (rng.random(n) < 1.0 / 3)            # a third of the copies: the anchor moved by up to 50
    out.anchor_pos[moved] = np.maximum(out.anchor_pos[moved] + rng.integers(-50, 51, int(moved.sum())), 0).astype(np.int32)
    if bd is not None:
        bd_off, bd = _csr_gather(bd_off, bd, origin)
    # the arguments of the parts
    mid = int(np.median(out.anchor_pos))                  # (win_end and the region are positions without the spacer)
    window = dict(chr_id=0, win_end=0xffffffff, region_start=0, region_end=0xffffffff, min_support=int(rng.integers(1, 5)),
                  balance_cutoff=int(rng.choice([100, 10, 0])), analyze_td=int(rng.random() < 0.8), analyze_inv=int(rng.random() < 0.8))
    how = int(rng.integers(0, 4))
    if how == 1:
        window["win_end"] = mid
    elif how == 2:
        window["region_end"] = mid
    elif how == 3:
        window["region_start"] = mid
    settings = (float(kw.get("seq_error_rate", 0.01)), int(rng.choice([20, 30, 45])), int(rng.choice([0, 50, 500])))
    max_listed = int(rng.integers(0, 5))
    lo, hi = SPACER - 4 * isz, SPACER + length + 4 * isz
    if rng.random() < 0.5:
        lo, hi = (SPACER + int(x) for x in np.quantile(out.anchor_pos, [0.25, 0.75]))
    n_seg = int(rng.integers(1, 7))
    cuts = np.sort(np.concatenate([[rng.integers(0, 30)], rng.integers(0, n, n_seg - 1), [n - rng.integers(1, 60)]])).astype(np.uint32)
    if n_seg >= 2 and rng.random() < 0.6:                  # a segment of no reads
        j = int(rng.integers(1, n_seg))
        cuts[j] = cuts[j - 1]
    dd = dict(seg_first=cuts, seg_strand=bytes(rng.choice(np.frombuffer(b"+-", dtype=np.uint8), n_seg)), min_bp_support=int(rng.integers(1, 5)),
              min_map_distance=int(rng.choice([50, 400, 2000])))
    search = SEARCHES[int(rng.integers(0, 3 if bd is None else 2))]
    return types.SimpleNamespace(seed=seed, chroms=chroms, batch=out, kw=kw, bd=bd, bd_off=bd_off, name_id=_first_occurrence(label), search=search,
                                 window=window, settings=settings, max_listed=max_listed, li=(lo, hi), dd=dd, lens=lens, isz=isz,
                                 n_copies=int(is_copy.sum()), n_planted=len(planted), n_junction=len(junction))


def describe(inp):
    """the drawn arguments on one line (the failure record of the hunt)"""
    return (f"params={inp.kw} lens={inp.lens} isz={inp.isz} chromosomes={len(inp.chroms)} search={inp.search} window={inp.window} "
            f"settings={inp.settings} max_listed={inp.max_listed} li={inp.li} dd=({inp.dd['seg_first'].tolist()}, {inp.dd['seg_strand']!r}, "
            f"{inp.dd['min_bp_support']}, {inp.dd['min_map_distance']})")


def cut(lists, max_listed):
    """pg_device_batch_classify's cut, by hand: a count byte above max_listed becomes max_listed | VARIANT_MORE"""
    cands, counts = lists
    counts = counts.copy()
    counts[(counts & 0x7f) > max_listed] = max_listed | hostlib.VARIANT_MORE
    return cands, counts


def lists_of_oracle(orc, n):
    """the oracle's result as the lists the statements take: rc_flag and the expanded points of both ends as CSR"""
    out = dict(rc_flag=orc["rc_flag"][:n])
    for end, key in (("close", "c"), ("far", "f")):
        cnt = orc[end + "_cnt"][:n].astype(np.int64)
        pts = orc[end + "_pts"][:n]
        out[key + "o"] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
        out[key + "p"] = pts[np.arange(pts.shape[1])[None, :] < cnt[:, None]] if n else pts.reshape(-1)
    return out


def close_of_lists(lists):
    """per read: has a close end, rc_flag, UP_Close.back()'s AbsLoc and LengthStr"""
    off, pts = lists["co"].astype(np.int64), lists["cp"]
    has = (np.diff(off) > 0).astype(np.uint8)
    last = np.maximum(off[1:] - 1, 0)
    la = np.where(has, pts["abs_loc"][last] if len(pts) else 0, 0).astype(np.uint32)
    ll = np.where(has, pts["length"][last] if len(pts) else 0, 0).astype(np.uint16)
    return has, np.asarray(lists["rc_flag"], dtype=np.uint8), la, ll


class HostChain:
    """The host statements of the classifier over the lists of one search (rc_flag, co / cp, fo / fp: the expanded points as CSR),
    each fed what the statement before it delivered; mm: g_maxMismatch of the drawn -e and -E.  A method computes its part once."""

    def __init__(self, inp, lists, mm):
        self.inp, self.l, self.mm, self._done = inp, lists, mm, {}
        self.window = hostlib.EventWindow(*[int(inp.window[f]) for f, _ in hostlib.EventWindow._fields_])

    def _once(self, key, make):
        if key not in self._done:
            self._done[key] = make()
        return self._done[key]

    def _reads(self):
        b, l = self.inp.batch, self.l
        return (self.inp.chroms, b.seq, b.seq_off, b.anchor_strand, b.chr_id, l["rc_flag"], l["co"], l["cp"], l["fo"], l["fp"], self.mm)

    def variant(self):
        return self._once("var", lambda: hostlib.variant_candidates(*self._reads()))

    def sv(self):
        return self._once("sv", lambda: hostlib.sv_candidates(*self._reads(), self.inp.settings))

    def events(self, var=None, sv=None, key="ev"):
        b, l = self.inp.batch, self.l
        return self._once(key, lambda: hostlib.events_from_lists(
            self.inp.chroms, b.seq, b.seq_off, b.anchor_strand, b.chr_id, l["rc_flag"], b.insert_size, l["co"], l["cp"], l["fo"], l["fp"],
            self.window, var or self.variant(), sv or self.sv(), self.inp.name_id))

    def sv_events(self, ev=None, sv=None, key="svt"):
        b, l = self.inp.batch, self.l
        return self._once(key, lambda: hostlib.sv_events_from_lists(
            self.inp.chroms, b.seq, b.seq_off, b.anchor_strand, l["rc_flag"], l["co"], l["cp"], self.window, (ev or self.events())["reads"],
            sv or self.sv()))

    def report(self, ev=None, svt=None, var=None, sv=None, key="rep"):
        b, l = self.inp.batch, self.l
        return self._once(key, lambda: hostlib.report_reads_from_lists(
            b.anchor_strand, l["rc_flag"], l["co"], l["cp"], l["fo"], l["fp"], ev or self.events(), svt or self.sv_events(),
            var or self.variant(), sv or self.sv()))

    def classified(self):
        """(events, sv events, (records, summaries)) of the lists cut at max_listed: what one classify call delivers"""
        var, sv = cut(self.variant(), self.inp.max_listed), cut(self.sv(), self.inp.max_listed)
        ev = self.events(var, sv, "ev_c")
        svt = self.sv_events(ev, sv, "svt_c")
        return ev, svt, self.report(ev, svt, var, sv, "rep_c")

    def li(self):
        b, l = self.inp.batch, self.l
        return self._once("li", lambda: hostlib.li_tables_from_lists(b.seq, b.seq_off, b.anchor_strand, b.chr_id, l["rc_flag"], l["co"], l["cp"], l["fo"],
                                                                     self.classified()[0]["reads"], 0, *self.inp.li))

    def int_calls(self):
        b, l = self.inp.batch, self.l
        rank = hostlib.chr_ranks([name for name, _ in self.inp.chroms])
        return self._once("int", lambda: hostlib.int_tables_from_lists(b.seq, b.seq_off, b.anchor_strand, b.chr_id, l["rc_flag"], l["co"], l["cp"], l["fo"],
                                                                       l["fp"], rank))

    def dd(self, close=None):
        """close: (has, rc_flag, last AbsLoc, last LengthStr) of a close-only search; None: those of the lists"""
        b, d = self.inp.batch, self.inp.dd
        has, rc, la, ll = close or close_of_lists(self.l)
        return self._once("dd", lambda: hostlib.dd_tables_from_close(b.seq, b.seq_off, b.anchor_strand, has, rc, la, ll, d["seg_first"], d["seg_strand"], 0,
                                                                     self.inp.chroms[0][1], self.mm, d["min_bp_support"], d["min_map_distance"]))

    def all(self):
        self.report()
        self.classified()
        self.li()
        if len(self.inp.chroms) > 1:
            self.int_calls()
        self.dd()
        return self


def _runs_per_read(off, pts):
    """runs of consecutive lengths with equal mismatches, chromosome and orientation per read, from expanded points"""
    off = off.astype(np.int64)
    if not len(pts):
        return np.zeros(len(off) - 1, dtype=np.int64)
    head = np.ones(len(pts), dtype=bool)
    same = (pts["length"][1:] == pts["length"][:-1] + 1)
    for f in ("mismatches", "chr_id", "direction", "strand"):
        same &= pts[f][1:] == pts[f][:-1]
    head[1:] = ~same
    head[off[:-1][off[:-1] < len(pts)]] = True
    cum = np.concatenate([[0], np.cumsum(head)])
    return cum[off[1:]] - cum[off[:-1]]


def tally(chain):
    """What the statements of a chain hold: the figures tests/test_classifier_fuzz_cpu.py asserts of the committed seeds"""
    l, inp = chain.l, chain.inp
    t = dict(multi_close=int((np.diff(l["co"].astype(np.int64)) >= 2).sum()), multi_far_runs=int((_runs_per_read(l["fo"], l["fp"]) >= 2).sum()))
    var, sv = chain.variant(), chain.sv()
    t["more"] = int(((var[1] & hostlib.VARIANT_MORE) != 0).any(axis=1).sum() + ((sv[1] & hostlib.VARIANT_MORE) != 0).any(axis=1).sum())
    ev = chain.events()
    flags = ev["reads"]["flags"]
    t["boxed"] = int(((flags & hostlib.EVR_BOXED) != 0).sum())
    t["duplicates"] = int(((flags & hostlib.EVR_DUPLICATE) != 0).sum())
    t["multi"] = [int((e["n_reads"] >= 2).sum()) for e in ev["events"]]
    t["both"] = [int(((e["n_plus"] > 0) & (e["n_plus"] < e["n_reads"])).sum()) for e in ev["events"]]
    t["unresolved"] = chain.classified()[0]["unresolved"]
    t["sv_events"] = chain.sv_events()["n_events"]
    li = chain.li()
    t["li_multi"] = [int((p["n_reads"] >= 2).sum()) for p in li["positions"]]
    if len(inp.chroms) > 1:
        calls = chain.int_calls()["calls"]
        fb = (calls["flags"] & hostlib.INT_FALLBACK) != 0
        t["int"] = dict(calls=len(calls), fallback=int(fb.sum()), template=int((~fb).sum()), multi=int((calls["n_reads"] >= 2).sum()))
    dd = chain.dd()
    c = dd["cands"]
    tested = (c["flags"] & hostlib.DD_TESTED) != 0
    t["dd"] = dict(multi=int((c["n_reads"] >= 2).sum()), tested=int(tested.sum()), dropped=int((c["cons_len"] == 0).sum()),
                   contained=int((tested & ((c["flags"] & hostlib.DD_CONTAINED) != 0)).sum()),
                   clear=int((tested & ((c["flags"] & hostlib.DD_CONTAINED) == 0)).sum()),
                   rc=[int((dd["members"]["rc_flag"] == v).sum()) for v in range(3)])
    return t
