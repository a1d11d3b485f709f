"""The dispersed-duplication breakpoint tables without a GPU: the header, the exports and the layouts; the host
statement hostlib.dd_tables_from_close against the literal restatement of tests/dd_tables_restated.py on a hand-made batch that
holds every edge of the contract and on random batches; the DD-read totals of tests/dd_tables_cases.py through the oracle's close end
and the statement; and the one consumer on hand-made tables."""
import os
import re

import numpy as np
import pytest

from oracle import pyoracle
from pindel_amd import binding, hostlib
from tests import dd_restated
from tests import dd_tables_cases as dc
from tests import dd_tables_restated as R
from tests.parity import run_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
MM = pyoracle.max_mismatch_table(0.01, 0.95)


# ------------------------------------------------------------------------------------------------ header, exports, layouts
def test_header_exports_and_layouts():
    h = open(os.path.join(ROOT, "include", "pindel_pg.h")).read()
    for sym in ("pg_device_batch_close_search", "pg_device_batch_dd", "pg_device_batch_dd_sizes", "pg_device_batch_dd_download",
                "pg_device_batch_dd_download_device"):
        assert re.search(r"\bint\s+" + sym + r"\(pg_ctx \*", h), sym
        assert sym in binding.EXPORTS
    assert "typedef struct { uint32_t read; uint16_t close_len; uint8_t rc_flag, reserved; } pg_dd_member;" in h
    assert ("typedef struct { uint32_t seg, pos, first, n_reads, cons_off, cons_len, flags, win_len; uint64_t win_start; } pg_dd_cand;") in h
    assert "typedef struct { uint64_t members, cands, cons_bytes; } pg_dd_sizes;" in h
    assert "#define PG_DD_TESTED    0x1u" in h and "#define PG_DD_CONTAINED 0x2u" in h
    for field in ("const uint32_t *seg_first;", "const uint8_t  *seg_strand;", "uint32_t n_seg;", "int32_t  chr_id;", "int32_t  min_bp_support;",
                  "int32_t  min_map_distance;"):
        assert field in h, field
    assert "200 000" in h                                       # the integer form of the float test, and how far it was checked
    assert binding.DD_MEMBER_DTYPE.itemsize == 8 and binding.DD_CAND_DTYPE.itemsize == 40
    assert binding.DD_MEMBER_DTYPE is hostlib.DD_MEMBER_DTYPE and binding.DD_CAND_DTYPE is hostlib.DD_CAND_DTYPE       # one copy
    assert binding.DD_CAND_DTYPE.fields["win_start"][1] == 32 and binding.DD_MEMBER_DTYPE.fields["close_len"][1] == 4
    assert (binding.DD_TESTED, binding.DD_CONTAINED) == (1, 2) == (hostlib.DD_TESTED, hostlib.DD_CONTAINED)
    import ctypes as C
    assert C.sizeof(binding.DdWindow) == 32 and C.sizeof(binding.DdSizes) == 24
    for name in ("close_search", "dd_tables", "dd_tensors", "dd_sizes", "dd_download"):
        assert callable(getattr(binding.Engine, name))


def test_launch_log_id_continues_the_enum():
    d = open(os.path.join(ROOT, "pindel_amd", "csrc", "pg_device.h")).read()
    assert "enum { PG_KERNEL_DD_TABLES = 13 };" in d and "enum { PG_KERNEL_INT = 12 };" in d
    assert binding.KERNEL_DD_TABLES == 13 == binding.KERNEL_INT + 1


def test_the_float_test_in_integers():
    """max >= 0.8f * n (float) against 5 * max >= 4 * n at the threshold and one either side (here to 20 000; the header says how far
    it was checked)"""
    n = np.arange(1, 20001, dtype=np.int64)
    for d in (-1, 0, 1):
        m = np.clip((4 * n + 4) // 5 + d, 0, None)
        f = m.astype(np.float32) >= np.float32(0.8) * n.astype(np.float32)
        assert (f == (5 * m >= 4 * n)).all()


# ------------------------------------------------------------------------------------------------ reads from walks
def read_from_walk(walk: bytes, mapped: bytes, strand: bytes, rc_flag=0, tail=b""):
    """The bytes of a read whose post-state S = unmapped + mapped has `walk` as its columns: S[u - 1 - i] = walk[i] for '-',
    its complement for '+' (a byte outside ACGTN stays: its column is then byte 0).  rc_flag 1: handed over reverse-complemented;
    rc_flag 2: as S, followed by `tail` (bytes outside ACGTN, which two reverse complements strip)."""
    un = bytes(reversed(walk)) if strand == b"-" else bytes(reversed(walk)).translate(_COMP)
    s = un + mapped
    if rc_flag == 1:
        return s.translate(_COMP)[::-1]
    return s + (tail if rc_flag == 2 else b"")


class Inputs:
    def __init__(self):
        self.seqs, self.strands, self.has, self.rc, self.abs, self.len = [], b"", [], [], [], []

    def add(self, seq, strand, has=1, rc=0, pos=0, close_len=0):
        self.seqs.append(seq)
        self.strands += strand
        self.has.append(has)
        self.rc.append(rc)
        self.abs.append(pos)
        self.len.append(close_len)
        return len(self.seqs) - 1


def run_both(inp, seg_first, seg_strand, chrom, support, mmd, python_contains=False):
    n = len(inp.seqs)
    seq = np.frombuffer(b"".join(inp.seqs), dtype=np.uint8) if n else np.zeros(0, np.uint8)
    off = np.concatenate([[0], np.cumsum([len(s) for s in inp.seqs])]).astype(np.uint64)
    got = hostlib.dd_tables_from_close(seq, off, np.frombuffer(inp.strands, dtype=np.uint8), inp.has, inp.rc, inp.abs, inp.len, seg_first, seg_strand,
                                       0, chrom, MM, support, mmd)

    def contains(c, ws, wl):
        q, db = c.decode("latin-1"), chrom[ws:ws + wl].decode("latin-1")
        if python_contains:
            return dd_restated.contains_any_strand(q, db, MM)
        return bool(dd_restated.cpu_contains([q], [db], MM, threads=1)[0])
    stats = {}
    want = R.tables(inp.seqs, inp.strands, inp.has, inp.rc, inp.abs, inp.len, seg_first, seg_strand, len(chrom), support, mmd, contains, stats)
    assert got["members"].tobytes() == want["members"].tobytes(), (got["members"], want["members"])
    assert got["cands"].tobytes() == want["cands"].tobytes(), (got["cands"], want["cands"])
    assert got["cons"] == want["cons"]
    return got, stats


def hand_made():
    rng = np.random.default_rng(5)

    def bases(k):
        return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), k))
    chrom = bases(200)
    inp = Inputs()
    ids = {}

    def group(key, strand, pos, walks, rcs=None):
        out = []
        for k, w in enumerate(walks):
            mapped = bases(12 + k)
            rc = rcs[k] if rcs else 0
            out.append(inp.add(read_from_walk(w, mapped, strand, rc, tail=b".."), strand, 1, rc, pos, len(mapped)))
        ids[key] = out

    def mutate(w, at, to=None):
        return w[:at] + (to if to is not None else bytes([b"ACGT"[(b"ACGT".index(w[at]) + 1) % 4]])) + w[at + 1:]
    seg_first = [0]
    # ---- segment 0, '+'
    a = bases(20)                                               # A: 4 of 5 in column 16 (accepted); one member two columns shorter
    group("A", b"+", 100, [a, a, a, mutate(a, 16), a[:18]])
    b = bases(22)                                               # B: 3 of 4 in column 15 (rejected): a consensus of exactly 15, kept
    group("B", b"+", 120, [b, b, b, mutate(b, 15)])
    c = bases(22)                                               # C: a two-way tie in column 14, byte 0 (rc4n of 0xc1) against a base: 14 columns, dropped
    group("C", b"+", 140, [c, c, mutate(c, 14, b"\xc1"), mutate(c, 14, b"\xc1")])
    d = bases(16)                                               # D: an IUPAC letter in every member's column 3: rc4n leaves byte 0, which wins
    group("D", b"+", 160, [mutate(d, 3, b"R")] * 3)
    inp.add(bases(30), b"-", 1, 0, 100, 10)                     # a read whose strand differs from its segment's
    inp.add(bases(30), b"+", 0, 0, 0, 0)                        # a read without a close end
    seg_first.append(len(inp.seqs))
    # ---- segment 1, '-': the position of A again; rc_flag 1 and 2; a member with u == 0; support one short of the minimum
    e = bases(24)
    group("E", b"-", 100, [e, e[:20], e[:17]], rcs=[1, 2, 0])
    ids["E"].append(inp.add(bases(14), b"-", 1, 0, 100, 14))    # u == 0
    f = bases(20)
    group("F", b"-", 50, [f, f])
    k = bases(22)                                               # K: a two-way tie of a byte >= 0x80 (kept as it is on this strand) against a base
    group("K", b"-", 140, [k, k, mutate(k, 17, b"\xc1"), mutate(k, 17, b"\xc1")])
    seg_first.append(len(inp.seqs))
    seg_first.append(len(inp.seqs))                             # ---- segment 2: no reads
    # ---- segment 3, '+': the window clamped at 0 (and the consensus in it), the window cut by the chromosome's end
    group("I", b"+", 10, [chrom[20:40]] * 3)
    group("J", b"+", 190, [bases(18)] * 3)
    seg_first.append(len(inp.seqs))
    inp.add(read_from_walk(a, bases(12), b"+"), b"+", 1, 0, 100, 12)     # outside every segment
    return chrom, inp, seg_first, b"+--+", ids


def test_hand_made_batch_holds_every_edge():
    chrom, inp, seg_first, seg_strand, ids = hand_made()
    got, stats = run_both(inp, seg_first, seg_strand, chrom, 3, 30, python_contains=True)
    cands = {(int(c["seg"]), int(c["pos"])): c for c in got["cands"]}
    assert sorted(cands) == [(0, 100), (0, 120), (0, 140), (0, 160), (1, 100), (1, 140), (3, 10), (3, 190)]   # F is one short; table order
    assert [(int(c["seg"]), int(c["pos"])) for c in got["cands"]] == sorted(cands)
    assert set(seg_strand) == {ord("+"), ord("-")} and (0, 100) in cands and (1, 100) in cands           # one position in two segments
    members_of = lambda k: got["members"]["read"][int(cands[k]["first"]):int(cands[k]["first"]) + int(cands[k]["n_reads"])].tolist()
    assert members_of((0, 100)) == ids["A"] and members_of((1, 100)) == ids["E"]                        # ascending read index within a key
    in_tables = set(got["members"]["read"].tolist())
    assert not in_tables & set(ids["F"]) and 2 in stats["support"] and 3 in stats["support"]            # min_bp_support - 1 and min_bp_support
    wrong_strand, no_close, outside = ids["D"][-1] + 1, ids["D"][-1] + 2, len(inp.seqs) - 1
    assert inp.strands[wrong_strand] == ord("-") and not inp.has[no_close] and not {wrong_strand, no_close, outside} & in_tables
    by = {(s["seg"], s["pos"]): s for s in stats["cands"]}
    assert (4, 5, True) in by[(0, 100)]["votes"] and by[(0, 100)]["columns"] == [20] and by[(0, 100)]["n_per_column"][-1] == 4
    assert (3, 4, False) in by[(0, 120)]["votes"] and int(cands[(0, 120)]["cons_len"]) == 15
    # two-way ties go to the smaller signed char: byte 0 before a base, a byte >= 0x80 before both
    assert len(by[(0, 140)]["ties"]) == 1 and by[(0, 140)]["ties"][0][1] == 0 and len(by[(0, 140)]["ties"][0][0]) == 2
    assert len(by[(1, 140)]["ties"]) == 1 and by[(1, 140)]["ties"][0][1] == 0xc1 and len(by[(1, 140)]["ties"][0][0]) == 2
    assert by[(1, 140)]["columns"] == [17] and int(cands[(1, 140)]["cons_len"]) == 17
    assert by[(0, 140)]["columns"] == [14] and int(cands[(0, 140)]["cons_len"]) == 0 and int(cands[(0, 140)]["flags"]) == 0
    assert int(cands[(0, 140)]["cons_off"]) == int(cands[(0, 160)]["cons_off"])                         # a dropped consensus takes no bytes
    assert by[(0, 160)].get("nul_won") and got["cons"][int(cands[(0, 160)]["cons_off"]) + 3] == 0
    e = got["members"][int(cands[(1, 100)]["first"]):][:4]
    assert e["rc_flag"].tolist() == [1, 2, 0, 0] and 0 in by[(1, 100)]["lens"] and len(set(by[(1, 100)]["lens"])) == 4
    assert by[(1, 100)]["n_per_column"][0] == 3 and by[(1, 100)]["n_per_column"][-1] == 1               # n shrinks along the columns
    assert (int(cands[(3, 10)]["win_start"]), int(cands[(3, 10)]["win_len"])) == (0, 60)                # clamped at 0
    assert (int(cands[(3, 190)]["win_start"]), int(cands[(3, 190)]["win_len"])) == (160, 40)            # cut by the chromosome's end
    assert int(cands[(3, 10)]["flags"]) == 3 and int(cands[(3, 190)]["flags"]) == 1 and int(cands[(0, 100)]["flags"]) == 1
    # a '-' segment stores its columns reversed, a '+' segment in order
    e_walk = R.walk_of(inp.seqs[ids["E"][0]], 1, inp.len[ids["E"][0]], False)
    c = cands[(1, 100)]
    assert got["cons"][int(c["cons_off"]):int(c["cons_off"]) + int(c["cons_len"])] == e_walk[::-1] and int(c["cons_len"]) == 24
    c = cands[(3, 10)]
    assert got["cons"][int(c["cons_off"]):int(c["cons_off"]) + int(c["cons_len"])] == chrom[20:40]
    # min_bp_support 1 (and less) admits every key: F and the single reads no longer fall out
    one, _ = run_both(inp, seg_first, seg_strand, chrom, 1, 30)
    assert (1, 50) in {(int(c["seg"]), int(c["pos"])) for c in one["cands"]} and set(ids["F"]) <= set(one["members"]["read"].tolist())
    zero, _ = run_both(inp, seg_first, seg_strand, chrom, 0, 30)
    assert zero["cands"].tobytes() == one["cands"].tobytes()
    # n_seg 0
    none, _ = run_both(inp, [], b"", chrom, 3, 30)
    assert none["members"].size == 0 and none["cands"].size == 0 and none["cons"] == b""


def test_refusals_of_the_statement():
    chrom, inp, seg_first, seg_strand, _ = hand_made()
    seq = np.frombuffer(b"".join(inp.seqs), dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum([len(s) for s in inp.seqs])]).astype(np.uint64)
    args = (seq, off, np.frombuffer(inp.strands, dtype=np.uint8), inp.has, inp.rc, inp.abs, inp.len)
    down = list(seg_first)
    down[1], down[2] = down[2], down[1]
    for first, strand, mmd in ((down, seg_strand, 30), (seg_first[:-1] + [len(inp.seqs) + 1], seg_strand, 30), (seg_first, b"+-?+", 30),
                               (seg_first, seg_strand, 0)):
        with pytest.raises(ValueError):
            hostlib.dd_tables_from_close(*args, first, strand, 0, chrom, MM, 3, mmd)


@pytest.mark.parametrize("seed", range(12))
def test_random_batches(seed):
    """1 to 200 reads in up to five segments over a handful of positions: members that agree on a walk with a few substitutions and
    different lengths, IUPAC letters and bytes >= 0x80 among them, all three rc flags, positions at both ends of the chromosome and
    one beyond 2^31"""
    rng = np.random.default_rng(100 + seed)
    n = [1, 2, 7, 33, 64, 65, 100, 129, 150, 177, 199, 200][seed]
    chrom = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 300))
    n_seg = int(rng.integers(1, 6))
    cuts = np.sort(rng.integers(0, n + 1, n_seg + 1)).tolist()
    seg_strand = bytes(rng.choice(np.frombuffer(b"+-", dtype=np.uint8), n_seg))
    positions = [5, 120, 121, 290, 0x80000010]
    walks = {p: bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 40)) for p in positions}
    walks[120] = chrom[100:140]
    inp = Inputs()
    for i in range(n):
        s = int(np.searchsorted(cuts, i, side="right")) - 1
        strand = bytes([seg_strand[s]]) if 0 <= s < n_seg and rng.random() < 0.9 else bytes(rng.choice(np.frombuffer(b"+-", dtype=np.uint8), 1))
        pos = positions[int(rng.integers(0, len(positions)))]
        w = bytearray(walks[pos][:int(rng.integers(0, 41))])
        for at in range(len(w)):
            if rng.random() < 0.04:
                w[at] = int(rng.choice(np.frombuffer(b"ACGTNR\xc1", dtype=np.uint8)))
        rc = int(rng.integers(0, 3))
        if rc == 1:
            w = bytearray(b if b in b"ACGTN" else ord("A") for b in w)       # (handed over reverse-complemented: ACGTN only)
        mapped = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), int(rng.integers(8, 30))))
        inp.add(read_from_walk(bytes(w), mapped, strand, rc, tail=b"#"), strand, int(rng.random() < 0.85), rc, pos, len(mapped))
    support = int(rng.integers(1, 5))
    got, stats = run_both(inp, cuts, seg_strand, chrom, support, int(rng.integers(1, 200)))
    assert int(got["cands"]["n_reads"].sum()) == len(got["members"])
    if n >= 100:
        assert len(got["cands"]) >= 2 and (got["cands"]["flags"] & 1).any()


# ------------------------------------------------------------------------------------------------ the plans of the GPU test
def oracle_close_ends(chroms, batch):
    """per read: has a close end, rc_flag, UP_Close.back()'s AbsLoc and LengthStr -- from the CPU oracle's close end"""
    r = run_oracle({}, chroms, batch, do_far=False)
    cnt = r["close_cnt"].astype(np.int64)
    last = r["close_pts"][np.arange(batch.n), np.maximum(cnt - 1, 0)]
    has = (cnt > 0).astype(np.uint8)
    return has, r["rc_flag"], np.where(has, last["abs_loc"], 0).astype(np.uint32), np.where(has, last["length"], 0).astype(np.uint16)


@pytest.mark.parametrize("k", [255, 256, 257, 1024, 1025])
def test_dd_read_totals_plan(k):
    """tests/dd_tables_cases.py dd_read_totals through the oracle's close end and the statement alone: the plan holds what
    tests/test_gpu_dd_tables.py asserts of it on the device's close ends"""
    chroms, biol = dc.reference()
    batch, first, strand = dc.dd_read_totals(biol, k, seed=k).batch()
    has, rc, la, ll = oracle_close_ends(chroms, batch)
    tables = [hostlib.dd_tables_from_close(batch.seq, batch.seq_off, batch.anchor_strand, has, rc, la, ll, first, strand, 0, chroms[0][1], MM,
                                           support, 400) for support in (3, 1)]
    dc.assert_dd_read_totals(tables[0], tables[1], k)
    assert batch.n > k + 12 and int(first[-1]) < batch.n


# ------------------------------------------------------------------------------------------------ the consumer
def test_consumer_on_hand_made_tables():
    """Tables made by hand, ordered as the contract orders them (pos unsigned): with a spacer above a position, (int)(pos - spacer) is
    negative and the consumer's std::map<int> order differs from the table's.  On a real chromosome that cannot occur -- a position
    is an AbsLoc, never below the spacer -- so the order is forced here with positions either side of 2^31 + spacer."""
    rng = np.random.default_rng(9)

    def bases(k):
        return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), k))
    spacer = 1000
    names, seqs, strands = [], [], b""
    members, cands, cons = [], [], b""
    plan = [(0, b"+", 5000, [20, 26, 23]), (0, b"+", 0x80000000 + 2000, [18, 18, 30]), (1, b"-", 400, [25, 16]), (1, b"-", 3000, [17, 21, 19, 40])]
    for seg, strand, pos, lens in plan:
        walk = bases(max(lens))
        first = len(members)
        for k, u in enumerate(lens):
            mapped = bases(10 + k)
            rc = (k % 3) if strand == b"-" else 0
            names.append(f"@r{len(names)}/1")
            seqs.append(read_from_walk(walk[:u], mapped, strand, rc, tail=b".."))
            strands += strand
            members.append((len(seqs) - 1, len(mapped), rc, 0))
        c = walk if strand == b"+" else walk[::-1]
        cands.append((seg, pos, first, len(lens), len(cons), len(c), 1 | (2 if pos == 3000 else 0), 60, 0))
        cons += c
    t = dict(members=np.array(members, dtype=hostlib.DD_MEMBER_DTYPE), cands=np.array(cands, dtype=hostlib.DD_CAND_DTYPE), cons=cons)
    assert [(int(c["seg"]), int(c["pos"])) for c in t["cands"]] == sorted((int(c["seg"]), int(c["pos"])) for c in t["cands"])
    got = hostlib.dd_cands_from_tables(names, seqs, np.frombuffer(strands, dtype=np.uint8), 2, t["members"], t["cands"], t["cons"], sample="S",
                                       spacer=spacer)
    want = R.consumer(names, seqs, strands, 2, t, "S", spacer)
    assert [g[:5] for g in got] == [w[:5] for w in want]
    # std::map<int> order: the position beyond 2^31 + spacer comes first in segment 0, 400 - 1000 < 0 first in segment 1
    assert [g[1] for g in got] == [0x80000000 + 2000 - spacer - (1 << 32), 4000, -600, 2000]
    assert [g[1] for g in got] != [((int(c["pos"]) - spacer) & 0xffffffff) for c in t["cands"]]
    for g, w in zip(got, want):
        assert sorted(g[5]) == sorted(w[5])
        lens = [len(r[4]) for r in g[5]]
        assert lens == sorted(lens, reverse=True)                # comp_unmapped_seqsize
        for name, sample, sequence, mapped, unmapped in g[5]:
            assert sample == "S" and sequence in (mapped + unmapped, unmapped + mapped)
    # the pipeline of tests/dd_restated.py votes the same consensus over the consumer's unmapped parts
    for g, (seg, strand, pos, lens) in zip(sorted(got, key=lambda g: (g[0], g[1] & 0xffffffff)), sorted(plan, key=lambda p: (p[0], (p[2] - spacer) & 0xffffffff))):
        sr_strand = "-" if strand == b"+" else "+"
        assert dd_restated.consensus_unmapped([r[4] for r in g[5]], sr_strand) == g[4]
    # tables that do not fit the reads are refused
    bad = t["members"].copy()
    bad["read"][0] = len(seqs)
    with pytest.raises(ValueError, match="do not fit"):
        hostlib.dd_cands_from_tables(names, seqs, np.frombuffer(strands, dtype=np.uint8), 2, bad, t["cands"], t["cons"], spacer=spacer)
