"""Event tables from candidate lists, host side.  hostlib.events_from_lists -- the reference the device entry is
compared with -- is checked here against a literal restatement: the cascade read by read, the O(n^2) exchange loop of
bubblesortReads that swaps on !smaller, the double walk of markDuplicates and the linear grouping of the reporters, on random
candidate arrays in which ties dominate.  The entries, dtypes and constants are checked against the public header."""
import ctypes
import os
import re

import numpy as np
import pytest

from pindel_amd import binding, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 0xffffffff
SPACER = 1000
N = ord("N")
TABLE_KINDS = (0, 1, 3, 4)
ORDER = (0, 2, 3, 4, 5, 6, 1)                  # process_window's order of the seven kinds
COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


# ------------------------------------------------------------------------------------------------ exports, dtypes, constants
def test_abi_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pindel_pg.h")).read()
    binding.build()
    lib = ctypes.CDLL(binding.LIB_PATH)
    for sym in ("pg_device_batch_events", "pg_device_batch_events_device", "pg_device_batch_event_sizes",
                "pg_device_batch_events_download", "pg_device_batch_events_download_device"):
        assert f"{sym}(" in hdr and sym in binding.EXPORTS and hasattr(lib, sym), sym
    host = hostlib.lib()
    for sym in ("pgh_events_from_lists", "pgh_name_ids"):
        assert hasattr(host, sym), sym
    for name in ("events", "events_tensors", "event_sizes"):
        assert callable(getattr(binding.Engine, name))
    with open(binding.LIB_PATH, "rb") as f:
        blob = f.read()
    for kernel in (b"pg_events_cascade_kernel", b"pg_events_scatter_kernel", b"pg_events_unique_kernel", b"pg_events_event_kernel"):
        assert kernel in blob, kernel


def header_struct(hdr, name):
    """[(type, field)] of a typedef struct of the header"""
    body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        out += [(typ, n.strip()) for n in names.split(",")]
    return out


def test_layouts_and_constants_agree_with_the_header():
    hdr = open(os.path.join(ROOT, "include", "pindel_pg.h")).read()
    ctype = {"uint8_t": "u1", "uint16_t": "<u2", "uint32_t": "<u4", "int32_t": "<i4"}
    for mod in (binding, hostlib):
        for struct, dtype in (("pg_event_read", mod.EVENT_READ_DTYPE), ("pg_event", mod.EVENT_DTYPE)):
            want = header_struct(hdr, struct)
            assert [n for _, n in want] == list(dtype.names), struct
            assert [np.dtype(ctype[t]) for t, _ in want] == [dtype.fields[n][0] for n in dtype.names], struct
        assert [n for _, n in header_struct(hdr, "pg_event_window")] == [f for f, _ in mod.EventWindow._fields_]
        assert ctypes.sizeof(mod.EventWindow) == 32 and ctypes.sizeof(mod.EventSizes) == 72
        assert mod.EVENT_READ_DTYPE.itemsize == 8 and mod.EVENT_DTYPE.itemsize == 40
        for name in ("EVR_BOXED", "EVR_USED", "EVR_UNRESOLVED", "EVR_DUPLICATE", "EV_SUPPORT", "EV_RANGE", "EV_BALANCE", "EV_REPORT"):
            m = re.search(r"#define PG_" + name + r"\s+(0x[0-9a-f]+)u", hdr)
            assert m and int(m.group(1), 16) == getattr(mod, name), name
        assert "#define PG_EVENT_TABLES 4" in hdr and mod.EVENT_TABLES == 4 and tuple(mod.EVENT_KINDS) == TABLE_KINDS
    dev = open(os.path.join(ROOT, "pindel_amd", "csrc", "pg_device.h")).read()
    assert "PG_KERNEL_EVENT_CASCADE = 6, PG_KERNEL_EVENT_SORT = 7, PG_KERNEL_EVENT_TABLES = 8" in dev
    assert (binding.KERNEL_EVENT_CASCADE, binding.KERNEL_EVENT_SORT, binding.KERNEL_EVENT_TABLES) == (6, 7, 8)
    assert f"#define PG_EV_BLOCK {binding.EVENT_BLOCK}u" in dev


def test_name_ids_number_names_by_first_occurrence():
    assert hostlib.name_ids(["b", "a", "b", "c", "a", "b"]).tolist() == [0, 1, 0, 2, 1, 0]
    assert hostlib.name_ids([]).tolist() == []


# ------------------------------------------------------------------------------------------------ the literal restatement
def to_short(v):
    v &= 0xffff
    return v - 0x10000 if v & 0x8000 else v


def real_start_deletion(chrom, rs, re_):
    if len(chrom) < rs or len(chrom) < re_:
        return rs, re_
    pos, end = rs + SPACER, re_ + SPACER - 1
    start = pos + 1
    while chrom[pos] == chrom[end] and chrom[pos] != N:
        pos -= 1
        end -= 1
    out_rs = pos - SPACER
    pos = re_ + SPACER
    while chrom[pos] == chrom[start] and chrom[pos] != N:
        pos += 1
        start += 1
    return out_rs, pos - SPACER


def real_start_insertion(chrom, ins, rs, re_):
    if len(chrom) < rs or len(chrom) < re_:
        return rs, re_
    after = re_ + SPACER
    while chrom[after] == ins[0] and chrom[after] != N:
        ins = ins[1:] + ins[:1]
        after += 1
    out_re = after - SPACER
    before = after - 1
    while chrom[before] == ins[-1] and chrom[before] != N:
        ins = ins[-1:] + ins[:-1]
        before -= 1
    return before - SPACER, out_re


def nt_str_of(inp, i, c):
    """NT_str of a kind 1 record: the read's substring behind the pair's own BP, rotated left by nt_rot"""
    seq = inp["seqs"][i]
    plus = inp["strand"][i] == ord("+")
    bp0 = int(inp["close_len"][i] if plus else inp["far_len"][i]) - 1
    src = seq.translate(COMP)[::-1] if plus else seq
    s = src[bp0 + 1:bp0 + 1 + int(c["indel_size"])] if 0 <= bp0 + 1 <= len(src) else b""
    if len(s) > 1:
        rot = int(c["nt_rot"]) % len(s)
        s = s[rot:] + s[:rot]
    return s


def restate(inp, w, chrom):
    n = inp["n"]
    box_size = max(len(chrom) // 30000, 1)
    n_boxes = len(chrom) * 2 // box_size + 1
    reads = np.zeros(n, dtype=hostlib.EVENT_READ_DTYPE)
    boxes = {k: {} for k in TABLE_KINDS}           # kind -> box -> read indices in push order
    state = {}
    unresolved = 0
    for i in range(n):
        if inp["chr_id"][i] != w.chr_id:
            continue
        plus = inp["strand"][i] == ord("+")
        used, nt = False, 0
        for kind in ORDER:
            if kind in (3, 4) and not w.analyze_td or kind in (5, 6) and not w.analyze_inv:
                continue
            if kind < 2:
                lst, count, cap = inp["var"][0][i, kind], int(inp["var"][1][i, kind]), 4
            else:
                s0 = hostlib.SV_SLOT[kind]
                cap = hostlib.SV_LIST_LEN[kind]
                lst, count = inp["sv"][0][i, s0:s0 + cap], int(inp["sv"][1][i, kind - 2])
            for j in range(min(count & 0x7f, cap)):
                c = lst[j]
                bl, br = int(c["bp_left"]), int(c["bp_right"])
                transgress = br > ((w.win_end - 2 * int(inp["isz"][i])) & U32)
                in_region = w.region_start <= ((bl + 1) & U32) <= w.region_end
                signed = bl - (1 << 32) if bl >> 31 else bl
                box = int(signed / box_size) & U32
                box_it = False
                if kind < 2:
                    if c["flags"] & 1 or transgress:
                        used = True
                    elif in_region and box < n_boxes:
                        box_it = used = True
                else:
                    if kind != 3:
                        nt = int(c["nt_rot"]) & 0xffff
                    if c["flags"] & 1:
                        used = True
                    if not (kind == 5 and not plus) and transgress:
                        used = True
                    elif in_region and box < n_boxes:
                        box_it = used = True
                if used:
                    reads[i]["kind"], reads[i]["slot"] = kind, j
                    reads[i]["flags"] = hostlib.EVR_BOXED if box_it else hostlib.EVR_USED
                    if box_it:
                        reads[i]["nt_size"] = nt
                        if kind in boxes:
                            boxes[kind].setdefault(box, []).append(i)
                            state[i] = (c, nt)
                    break
            if used:
                break
            if count & 0x80:
                reads[i]["flags"], reads[i]["unresolved_kind"] = hostlib.EVR_UNRESOLVED, kind
                unresolved += 1
                break

    def key(i):
        c, nt = state[i]
        return (int(c["bp_left"]), int(c["bp_right"]), int(c["indel_size"]), nt, int(c["bp"]))

    members, events = [], []
    for kind in TABLE_KINDS:
        mem, evs = [], []
        for box in sorted(boxes[kind]):
            idx = list(boxes[kind][box])
            for a in range(len(idx) - 1):                      # bubblesortReads: swaps on !smaller, equal elements too
                for b in range(a + 1, len(idx)):
                    if not key(idx[a]) < key(idx[b]):
                        idx[a], idx[b] = idx[b], idx[a]
            unique = [True] * len(idx)
            for a in range(len(idx)):                          # markDuplicates
                if not unique[a]:
                    continue
                for b in range(a + 1, len(idx)):
                    ca, cb = state[idx[a]][0], state[idx[b]][0]
                    if ca["left"] == cb["left"] and ca["right"] == cb["right"] and inp["name_id"][idx[a]] == inp["name_id"][idx[b]]:
                        unique[b] = False
            for a, i in enumerate(idx):
                if not unique[a]:
                    reads[i]["flags"] |= hostlib.EVR_DUPLICATE
            good = [i for a, i in enumerate(idx) if unique[a]]
            head = len(mem)
            s = 0
            while s < len(good):                               # the reporters' linear grouping
                f = state[good[s]][0]
                e = s
                while e + 1 < len(good):
                    g = state[good[e + 1]][0]
                    if g["bp_left"] != f["bp_left"] or (g["indel_size"] != f["indel_size"] if kind == 1 else g["bp_right"] != f["bp_right"]):
                        break
                    e += 1
                rs, re_ = int(f["bp_left"]), int(f["bp_right"])
                if kind == 1:
                    s_nt = nt_str_of(inp, good[s], f)
                    if s_nt:
                        rs, re_ = real_start_insertion(chrom, s_nt, rs, re_)
                else:
                    rs, re_ = real_start_deletion(chrom, rs, re_)
                lmin = lmax = rmin = rmax = False
                n_plus = 0
                for i in good[s:e + 1]:
                    c, nt = state[i]
                    RL, bp = len(inp["seqs"][i]), int(c["bp"])
                    n_plus += inp["strand"][i] == ord("+")
                    rl = to_short(RL - nt)
                    mn = to_short(to_short(int(rl * 0.5 + 0.5)) - 1)
                    mx = to_short(to_short(int(rl * (1 - 0.5) - 0.5)) - 1)
                    lmin |= bp <= mn
                    rmin |= RL - bp - nt <= mn
                    lmax |= bp >= mx
                    rmax |= RL - bp - nt >= mx
                flags = 0
                if e - s + 1 >= w.min_support:
                    flags |= hostlib.EV_SUPPORT
                if kind == 0 or (rs < re_ if kind == 1 else not (re_ < rs or rs == 0)):
                    flags |= hostlib.EV_RANGE
                if kind == 1 or int(f["indel_size"]) < w.balance_cutoff or (lmin and lmax and rmin and rmax):
                    flags |= hostlib.EV_BALANCE
                if flags == 7:
                    flags |= hostlib.EV_REPORT
                evs.append((int(f["bp_left"]), int(f["bp_right"]), int(f["indel_size"]), head + s, e - s + 1, int(n_plus), rs & U32, re_ & U32,
                            head, state[good[s]][1], kind, flags))
                s = e + 1
            mem += good
        members.append(np.array(mem, dtype=np.uint32))
        events.append(np.array(evs, dtype=hostlib.EVENT_DTYPE) if evs else np.zeros(0, dtype=hostlib.EVENT_DTYPE))
    return dict(reads=reads, members=members, events=events, unresolved=unresolved)


# ------------------------------------------------------------------------------------------------ random candidate arrays
def make_chrom(rng, bio_len=88000):
    return b"N" * SPACER + bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=bio_len)) + b"N" * SPACER


def random_input(rng, n, chrom):
    """n reads of 40 bases with one close and one far point each, and random lists whose keys are drawn from three or four values per
    field.  A BPLeft beyond the chromosome string (95000) leaves the left alignment out, so that the range test can fail; BPLeft
    9000 fails the region [1, 9000] of some windows (the test is on BPLeft + 1): a DI pair there leaves its NT_size to kind 1."""
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=40)) for _ in range(n)]
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    strand = rng.choice(np.array([ord("+"), ord("-")], dtype=np.uint8), size=n)
    pts = lambda lens: np.array([(5000, int(l), 0, 0, b"+", b"+") for l in lens], dtype=binding.POINT_DTYPE)
    close_len, far_len = rng.integers(5, 16, size=n), rng.integers(5, 16, size=n)

    def records(shape, kinds_with_nt, small_indel):
        c = np.zeros(shape, dtype=hostlib.VARIANT_CAND_DTYPE)
        c["bp_left"] = rng.choice([5000, 5001, 5002, 9000, 95000], size=shape, p=[0.3, 0.25, 0.2, 0.2, 0.05])
        c["bp_right"] = rng.choice([5100, 5101, 9100, 9400], size=shape, p=[0.4, 0.3, 0.2, 0.1])
        c["left"] = rng.choice([100, 101], size=shape)
        c["right"] = rng.choice([300, 301], size=shape)
        c["indel_size"] = rng.choice([1, 2, 3] if small_indel else [1, 2, 150], size=shape)
        c["bp"] = rng.choice([3, 19, 20, 36], size=shape)
        c["nt_rot"] = kinds_with_nt(shape)
        c["flags"] = (rng.random(shape) < 0.05).astype(np.uint8)
        return c

    var = records((n, 2, 4), lambda s: 0, False)
    var[:, 1] = records((n, 4), lambda s: rng.integers(-3, 4, size=s), True)
    sv = records((n, hostlib.SV_SLOTS), lambda s: 0, False)
    for kind in (2, 4, 6):
        sv["nt_rot"][:, hostlib.SV_SLOT[kind]] = rng.integers(0, 3, size=n)

    def count_bytes(shape, cap):
        listed = np.minimum(rng.choice([0, 0, 1, 2, 4], size=shape), cap)
        more = (rng.random(shape) < 0.08) & (listed == cap)
        return (listed | (more * 0x80)).astype(np.uint8)

    var_n = count_bytes((n, 2), 4)
    sv_n = np.stack([count_bytes(n, hostlib.SV_LIST_LEN[k]) for k in (2, 3, 4, 5, 6)], axis=1)
    # the later kinds see only the reads the earlier ones left: some reads have lists for kind 1 alone (or for it and DI), for TD
    # alone, for TD_NT alone, so that enough of them reach those kinds
    focus = rng.choice(4, size=n, p=[0.4, 0.25, 0.15, 0.2])
    var_n[focus > 0, 0] = 0
    var_n[focus > 1, 1] = 0
    sv_n[focus == 1, 1:] = 0
    sv_n[(focus == 1) & (rng.random(n) < 0.5), 0] = 0
    sv_n[focus == 2, 0] = 0
    sv_n[focus == 2, 2:] = 0
    sv_n[focus == 3, :2] = 0
    sv_n[focus == 3, 3:] = 0
    # unused records are zeroed, as the candidate entries leave them
    for k in range(2):
        for j in range(4):
            var[(var_n[:, k] & 0x7f) <= j, k, j] = np.zeros((), dtype=var.dtype)
    for k in (2, 3, 4, 5, 6):
        for j in range(hostlib.SV_LIST_LEN[k]):
            sv[(sv_n[:, k - 2] & 0x7f) <= j, hostlib.SV_SLOT[k] + j] = np.zeros((), dtype=sv.dtype)
    chr_id = (rng.random(n) < 0.05).astype(np.int32)
    return dict(n=n, seqs=seqs, seq=np.frombuffer(b"".join(seqs), dtype=np.uint8), seq_off=off, strand=strand, chr_id=chr_id,
                rc_flag=np.zeros(n, dtype=np.uint8), isz=rng.choice(np.array([100, 200], dtype=np.int16), size=n),
                close_off=np.arange(n + 1, dtype=np.uint64), close_pts=pts(close_len), far_off=np.arange(n + 1, dtype=np.uint64),
                far_pts=pts(far_len), close_len=close_len, far_len=far_len, var=(var, var_n), sv=(sv, sv_n),
                name_id=rng.integers(0, max(n // 3, 1), size=n).astype(np.uint32))


def host_tables(inp, w, chrom, name_id="own"):
    return hostlib.events_from_lists([("chrR", chrom)], inp["seq"], inp["seq_off"], inp["strand"], inp["chr_id"], inp["rc_flag"], inp["isz"],
                                     inp["close_off"], inp["close_pts"], inp["far_off"], inp["far_pts"], w, inp["var"], inp["sv"],
                                     inp["name_id"] if name_id == "own" else name_id, spacer=SPACER)


WINDOWS = [dict(), dict(region_start=1, region_end=9000), dict(win_end=9700), dict(win_end=9700, region_start=1, region_end=9000, min_support=2),
           dict(min_support=3, balance_cutoff=10), dict(analyze_td=0), dict(analyze_inv=0), dict(analyze_td=0, analyze_inv=0, min_support=2)]


@pytest.fixture(scope="module")
def seen():
    return dict(multi=np.zeros(4, np.int64), both=np.zeros(4, np.int64), no_support=np.zeros(4, np.int64), no_range=np.zeros(4, np.int64),
                no_balance=np.zeros(4, np.int64), used_transgress=np.zeros(7, np.int64), used_ref_end=np.zeros(7, np.int64), carried_to_si=0,
                dups=np.zeros(4, np.int64), unresolved=0, ties=0)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 40, 120, 200])
def test_random_arrays_against_the_literal_restatement(seen, n):
    rng = np.random.default_rng(1000 + n)
    chrom = make_chrom(rng)
    for trial, wkw in enumerate(WINDOWS):
        inp = random_input(rng, n, chrom)
        w = hostlib.event_window(**wkw)
        got = host_tables(inp, w, chrom)
        want = restate(inp, w, chrom)
        what = f"n = {n}, window {wkw}"
        assert got["unresolved"] == want["unresolved"], what
        assert got["reads"].tobytes() == want["reads"].tobytes(), (what, np.nonzero(got["reads"] != want["reads"])[0][:5])
        for t in range(4):
            assert got["members"][t].tolist() == want["members"][t].tolist(), (what, t)
            assert len(got["events"][t]) == len(want["events"][t]), (what, t)
            for name in hostlib.EVENT_DTYPE.names:
                assert got["events"][t][name].tolist() == want["events"][t][name].tolist(), (what, t, name)
            ev = got["events"][t]
            seen["multi"][t] += int((ev["n_reads"] >= 2).sum())
            seen["both"][t] += int(((ev["n_plus"] > 0) & (ev["n_plus"] < ev["n_reads"])).sum())
            seen["no_support"][t] += int(((ev["flags"] & hostlib.EV_SUPPORT) == 0).sum())
            seen["no_range"][t] += int(((ev["flags"] & hostlib.EV_RANGE) == 0).sum())
            seen["no_balance"][t] += int(((ev["flags"] & hostlib.EV_BALANCE) == 0).sum())
            assert (((ev["flags"] & 7) == 7) == ((ev["flags"] & hostlib.EV_REPORT) != 0)).all()
            assert (ev["box_head"] <= ev["first"]).all()
        r = got["reads"]
        for i in np.nonzero(r["flags"] & hostlib.EVR_USED)[0]:
            kind, slot = int(r["kind"][i]), int(r["slot"][i])
            c = inp["var"][0][i, kind, slot] if kind < 2 else inp["sv"][0][i, hostlib.SV_SLOT[kind] + slot]
            seen["used_ref_end" if c["flags"] & 1 else "used_transgress"][kind] += 1
        boxed_si = ((r["flags"] & hostlib.EVR_BOXED) != 0) & (r["kind"] == 1)
        seen["carried_to_si"] += int((r["nt_size"][boxed_si] != 0).sum())
        for t, kind in enumerate(TABLE_KINDS):
            seen["dups"][t] += int((((r["flags"] & hostlib.EVR_DUPLICATE) != 0) & (r["kind"] == kind)).sum())
        seen["unresolved"] += got["unresolved"]
        # without name ids nothing is a duplicate, and the members are all the boxed reads
        plain = host_tables(inp, w, chrom, name_id=None)
        assert not (plain["reads"]["flags"] & hostlib.EVR_DUPLICATE).any()
        assert sum(plain["n_members"]) == int((((r["flags"] & hostlib.EVR_BOXED) != 0) & np.isin(r["kind"], TABLE_KINDS)).sum())


def test_coverage(seen):
    """The comparison above cannot pass on nothing: per kind an event with two members or more, one with both strands, one that
    fails each flag bit that can fail for the kind, duplicates; reads used without a box through the bin boundary and through
    PG_VARIANT_REF_END; a read that reached kind 1 with a carried NT_size; unresolved reads."""
    for t in range(4):
        assert seen["multi"][t] > 0 and seen["both"][t] > 0 and seen["no_support"][t] > 0 and seen["dups"][t] > 0, (t, seen)
    assert seen["no_range"][0] == 0 and (seen["no_range"][1:] > 0).all(), seen["no_range"]          # kind 0: always set
    assert seen["no_balance"][1] == 0 and seen["no_balance"][0] > 0 and (seen["no_balance"][2:] > 0).all(), seen["no_balance"]
    assert (seen["used_transgress"][list(TABLE_KINDS)] > 0).all() and (seen["used_ref_end"][:2] > 0).all(), (seen["used_transgress"], seen["used_ref_end"])
    assert seen["carried_to_si"] > 0 and seen["unresolved"] > 0


def test_refusals():
    rng = np.random.default_rng(5)
    chrom = make_chrom(rng)
    inp = random_input(rng, 5, chrom)
    for bad in (dict(chr_id=1), dict(chr_id=-1), dict(region_start=10, region_end=9)):
        with pytest.raises(ValueError):
            host_tables(inp, hostlib.event_window(**bad), chrom)


# ------------------------------------------------------------------------------------------------ the gold set: reports from tables
@pytest.fixture(scope="module")
def gold(tmp_path_factory):
    """The gold set searched once by the oracle, with the lists of both classifiers."""
    from oracle import pyoracle
    from pindel_amd import hostio
    from tests import golden_util as gu
    tmp = tmp_path_factory.mktemp("events_gold")
    fa, reads_txt = gu.unpack(tmp)
    chroms = hostio.load_fasta(fa)
    batch = hostio.read_pindel_text(reads_txt, [n for n, _ in chroms], [len(s) - 200000 for _, s in chroms])
    r = pyoracle.search_batch(pyoracle.make_params(), [s for _, s in chroms], batch.seq, batch.seq_off, batch.anchor_strand,
                              batch.anchor_pos, batch.insert_size, batch.chr_id)
    co, cp = gu.csr_from_strided(r["close_cnt"], r["close_pts"])
    fo, fp = gu.csr_from_strided(r["far_cnt"], r["far_pts"])
    mm = pyoracle.max_mismatch_table()
    args = (chroms, batch.seq, batch.seq_off, batch.anchor_strand, batch.chr_id, r["rc_flag"], co, cp, fo, fp, mm)
    return dict(tmp=tmp, fa=fa, reads_txt=reads_txt, batch=batch, chroms=chroms, points=(co, cp, fo, fp, r["rc_flag"]), mm=mm,
                var=hostlib.variant_candidates(*args), sv=hostlib.sv_candidates(*args))


def gold_run(gold, name, settings, events, var=None, sv=None, points=None, **kw):
    from tests import golden_util as gu
    prefix = str(gold["tmp"] / name)
    reads_txt = None if "reads_config" in kw else gold["reads_txt"]
    hostlib.call_from_points(gold["fa"], reads_txt, prefix, settings, *(points or gold["points"]), variant_candidates=var or gold["var"],
                             sv_candidates=sv or gold["sv"], events=events, **kw)
    return [open(f"{prefix}_{s}", "rb").read() for s in gu.SUFFIXES]


def with_fields(settings, **fields):
    s = hostlib.HostSettings.from_buffer_copy(settings)
    for k, v in fields.items():
        setattr(s, k, v)
    return s


GOLD_SCENARIOS = {
    "one_window": ({}, {}),
    "windows_20k": (dict(window_mbp=0.02), {}),              # reads within two insert sizes of a window's end transgress it
    "region": ({}, {"region": "1:1-100000"}),                # -c
    "windows_region": (dict(window_mbp=0.02), {"region": "1:20000-150000"}),
    "M3": (dict(min_support=3), {}),
    "B10": (dict(balance_cutoff=10), {}),
    "no_td_inv": (dict(analyze_td=0, analyze_inv=0), {}),
    "no_inv_windows": (dict(analyze_inv=0, window_mbp=0.02), {}),
}


@pytest.mark.parametrize("threads", ["1", "16"])
@pytest.mark.parametrize("scenario", sorted(GOLD_SCENARIOS))
def test_reports_from_tables_are_byte_identical(gold, monkeypatch, scenario, threads):
    from tests import golden_util as gu
    monkeypatch.setenv("PGH_THREADS", threads)
    fields, kw = GOLD_SCENARIOS[scenario]
    st = with_fields(hostlib.default_settings(gold["mm"]), **fields)
    plain = gold_run(gold, f"{scenario}_{threads}_plain", st, None, **kw)
    tabled = gold_run(gold, f"{scenario}_{threads}_events", st, True, **kw)
    assert tabled == plain
    assert hostlib.last_event_fallback_windows() == 0
    n_table, n_supplied = hostlib.last_event_table_windows()
    wins = hostlib.last_event_windows()
    assert n_table == len(wins) > 0 and n_supplied == 0
    assert (len(wins) > 3) == ("windows" in scenario)
    assert b"\tD " in plain[0] and b"\tI " in plain[1]
    if scenario == "one_window":
        gu.assert_reports_match_gold(str(gold["tmp"] / f"{scenario}_{threads}_events"))
        assert b"\tTD " in plain[2]


def doubled(gold):
    """Every read twice, with the same name: the point arrays and the lists of the file listed twice"""
    co, cp, fo, fp, rc = gold["points"]
    two = lambda off: np.concatenate([off, off[1:] + off[-1]])
    points = (two(co), np.concatenate([cp, cp]), two(fo), np.concatenate([fp, fp]), np.concatenate([rc, rc]))
    var = tuple(np.concatenate([a, a]) for a in gold["var"])
    sv = tuple(np.concatenate([a, a]) for a in gold["sv"])
    return points, var, sv


@pytest.mark.parametrize("fields", [{}, dict(min_support=3), dict(window_mbp=0.02)])
def test_reads_listed_twice(gold, monkeypatch, fields):
    """The read file listed twice through reads_config: every read occurs twice with the same name, so markDuplicates fires and
    ties exist in every key."""
    monkeypatch.setenv("PGH_THREADS", "4")
    points, var, sv = doubled(gold)
    st = with_fields(hostlib.default_settings(gold["mm"]), **fields)
    tag = "_".join(f"{k}{v}" for k, v in fields.items()) or "default"
    kw = dict(points=points, var=var, sv=sv, reads_config=[gold["reads_txt"], gold["reads_txt"]])
    plain = gold_run(gold, f"twice_{tag}_plain", st, None, **kw)
    tabled = gold_run(gold, f"twice_{tag}_events", st, True, **kw)
    assert tabled == plain
    assert hostlib.last_event_fallback_windows() == 0 and hostlib.last_event_table_windows()[0] > 0
    single = gold_run(gold, f"twice_{tag}_single", st, None)
    assert plain != single                                                 # the doubled reads show: as duplicates or as support


def test_truncated_lists_fall_back(gold, monkeypatch):
    """Lists cut by hand (PG_VARIANT_MORE set): a window that holds such a read takes the existing path, the bytes stay."""
    monkeypatch.setenv("PGH_THREADS", "4")
    st = with_fields(hostlib.default_settings(gold["mm"]), window_mbp=0.02)
    cands, counts = gold["var"][0].copy(), gold["var"][1].copy()
    cut = np.zeros(gold["batch"].n, dtype=bool)
    cut[np.nonzero((counts[:, 0] & 0x7f) > 0)[0][::40]] = True
    cands[cut] = np.zeros((), dtype=cands.dtype)
    counts[cut] = hostlib.VARIANT_MORE
    plain = gold_run(gold, "cut_plain", st, None)
    tabled = gold_run(gold, "cut_events", st, True, var=(cands, counts))
    assert tabled == plain
    n_fallback, (n_table, _) = hostlib.last_event_fallback_windows(), hostlib.last_event_table_windows()
    assert n_fallback > 0 and n_table > 0 and n_fallback + n_table == len(hostlib.last_event_windows())
    # every list truncated: every window falls back
    counts[:] = hostlib.VARIANT_MORE
    cands[:] = np.zeros((), dtype=cands.dtype)
    assert gold_run(gold, "cut_all_events", st, True, var=(cands, counts)) == plain
    assert hostlib.last_event_table_windows()[0] == 0 and hostlib.last_event_fallback_windows() == len(hostlib.last_event_windows())


def test_supplied_tables(gold, monkeypatch):
    """Tables built outside the run (here by events_from_lists over all reads, as the device builds them) for the one window."""
    monkeypatch.setenv("PGH_THREADS", "4")
    st = hostlib.default_settings(gold["mm"])
    plain = gold_run(gold, "supplied_plain", st, None)
    assert gold_run(gold, "supplied_probe", st, True) == plain
    wins = hostlib.last_event_windows()
    assert len(wins) == 1
    chr_index, ws, we, rs, re_, n_reads = [int(x) for x in wins[0]]
    b = gold["batch"]
    co, cp, fo, fp, rc = gold["points"]
    w = hostlib.event_window(chr_id=chr_index, win_end=we, region_start=rs, region_end=re_, min_support=st.min_support,
                             balance_cutoff=st.balance_cutoff)
    names = b.names if len(b.names) == b.n else None
    t = hostlib.events_from_lists(gold["chroms"], b.seq, b.seq_off, b.anchor_strand, b.chr_id, rc, b.insert_size, co, cp, fo, fp, w,
                                  gold["var"], gold["sv"], hostlib.name_ids(names) if names else None)
    assert t["unresolved"] == 0 and all(n > 0 for n in t["n_events"][:3])
    assert gold_run(gold, "supplied_events", st, {(chr_index, ws, we): t}) == plain
    assert hostlib.last_event_table_windows() == (1, 1)
    # tables for another window are not used: the host builds its own
    assert gold_run(gold, "supplied_other", st, {(chr_index, ws + 1, we): t}) == plain
    assert hostlib.last_event_table_windows() == (1, 0)


def test_events_need_both_lists(gold):
    st = hostlib.default_settings(gold["mm"])
    with pytest.raises(ValueError):
        hostlib.call_from_points(gold["fa"], gold["reads_txt"], str(gold["tmp"] / "bad"), st, *gold["points"], variant_candidates=gold["var"],
                                 events=True)
