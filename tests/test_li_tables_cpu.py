"""The long-insertion position tables on the host: the header's layouts and entries; hostlib.li_tables_from_lists --
the plain-loop statement the device is compared with -- against a literal Python restatement of the contract on random arrays, with
assertions that the generated cases cover the contract's corners; the single consumer (Caller::sort_output_li_tables) on tables made
by hand against tests/li_consumer.py; and the gold set: call_from_points(report_reads=True) with -l and -s writes _LI and
_CloseEndMapped through the tables route, byte for byte what the run without it writes."""
import ctypes
import os
import re

import numpy as np
import pytest

from pindel_amd import binding, hostlib
from tests import li_consumer as li
from tests import test_events_cpu as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMP = {ord("A"): ord("T"), ord("C"): ord("G"), ord("G"): ord("C"), ord("T"): ord("A"), ord("N"): ord("N")}


# ------------------------------------------------------------------------------------------------ exports, dtypes, constants
def test_abi_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pindel_pg.h")).read()
    binding.build()
    lib = ctypes.CDLL(binding.LIB_PATH)
    for sym in ("pg_device_batch_li", "pg_device_batch_li_sizes", "pg_device_batch_li_download", "pg_device_batch_li_download_device"):
        assert f"{sym}(" in hdr and sym in binding.EXPORTS and hasattr(lib, sym), sym
    for sym in ("pgh_li_tables_from_lists", "pgh_li_write_from_tables"):
        assert hasattr(hostlib.lib(), sym), sym
    for name in ("li", "li_tensors", "li_sizes", "li_download"):
        assert callable(getattr(binding.Engine, name)), name
    with open(binding.LIB_PATH, "rb") as f:
        blob = f.read()
    for kernel in (b"pg_li_flag_kernel", b"pg_li_compact_kernel", b"pg_li_scatter_kernel", b"pg_li_head_kernel", b"pg_li_pos_kernel",
                   b"pg_table_rank_kernel", b"pg_table_scan_kernel"):
        assert kernel in blob, kernel


def test_layouts_and_constants_agree_with_the_header():
    hdr = open(os.path.join(ROOT, "include", "pindel_pg.h")).read()
    for mod in (binding, hostlib):
        want = ec.header_struct(hdr, "pg_li_pos")
        assert [n for _, n in want] == list(mod.LI_POS_DTYPE.names)
        assert all(t == "uint32_t" and mod.LI_POS_DTYPE.fields[n][0] == np.dtype("<u4") for t, n in want)
        assert mod.LI_POS_DTYPE.itemsize == 16
        assert [(t, n.split("[")[0]) for t, n in ec.header_struct(hdr, "pg_li_sizes")] == [("uint64_t", f) for f, _ in mod.LiSizes._fields_]
        assert ctypes.sizeof(mod.LiSizes) == 32
        for name in ("LI_LONGER", "LI_SHORTER"):
            m = re.search(r"#define PG_" + name + r"\s+(0x[0-9a-f]+)u", hdr)
            assert m and int(m.group(1), 16) == getattr(mod, name), name
    assert [n for _, n in ec.header_struct(hdr, "pg_li_window")] == [f for f, _ in binding.LiWindow._fields_]
    assert ctypes.sizeof(binding.LiWindow) == 8
    dev = open(os.path.join(ROOT, "pindel_amd", "csrc", "pg_device.h")).read()
    assert "PG_KERNEL_LI = 11" in dev and binding.KERNEL_LI == 11


# ------------------------------------------------------------------------------------------------ the contract, literally
def post_state(seq: bytes, rc_flag: int) -> bytes:
    """rc_flag applications of setUnmatchedSeq(ReverseComplement()): a byte outside ACGTN becomes NUL, trailing non-alphanumerics go"""
    for _ in range(min(int(rc_flag), 2)):
        seq = bytes(COMP.get(c, 0) for c in reversed(seq))
        while seq and not chr(seq[-1]).isalnum():
            seq = seq[:-1]
    return seq


def restate(inp, win_chr, lo, hi):
    """pindel_pg.h "long-insertion position tables", literally.  Returns (members, positions) per strand and per read why it is out."""
    n = len(inp["strand"])
    members, positions = [[], []], [[], []]
    for s, sd in enumerate(b"+-"):
        at = {}
        for i in range(n):
            if inp["chr_id"][i] != win_chr:
                continue
            has_close = inp["close_off"][i + 1] > inp["close_off"][i]
            has_far = inp["far_off"][i + 1] > inp["far_off"][i]
            if not has_close or has_far or (int(inp["recs"]["flags"][i]) & (hostlib.EVR_BOXED | hostlib.EVR_USED)) or inp["strand"][i] != sd:
                continue
            last = inp["close_pts"][int(inp["close_off"][i + 1]) - 1]
            at.setdefault(min(max(int(last["abs_loc"]), lo), hi), []).append(i)
        for p in sorted(at):
            flags = 0
            for i in at[p]:
                length = len(post_state(inp["seqs"][i], inp["rc_flag"][i]))
                twice = 2 * int(inp["close_pts"][int(inp["close_off"][i + 1]) - 1]["length"])
                flags |= hostlib.LI_LONGER if twice > length else hostlib.LI_SHORTER if twice < length else 0
            positions[s].append((p, len(members[s]), len(at[p]), flags))
            members[s] += at[p]
    return members, positions


LO, HI = 5000, 5200


def random_input(rng, n, only_strand=None):
    """n reads of 20, 21 or 40 bases, some starting or ending with bytes outside ACGTN, with 0..3 close points at positions below, at,
    inside, at and above the buffered window [LO, HI], a far end for some, every state of the events build's record, two chromosomes,
    rc flags 0..2 and the odd anchor strand that is neither '+' nor '-'."""
    seqs = []
    for _ in range(n):
        body = bytes(rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=int(rng.choice([20, 40]))))
        seqs.append(b"X" * int(rng.choice([0, 0, 1, 2])) + body + b"." * int(rng.choice([0, 0, 0, 1])))
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    strand = rng.choice(np.frombuffer(b"+-*", dtype=np.uint8), size=n, p=[0.48, 0.48, 0.04])
    if only_strand is not None:
        strand[:] = only_strand
    n_close = rng.choice([0, 1, 2, 3], size=n, p=[0.15, 0.5, 0.25, 0.1])
    n_far = rng.choice([0, 1], size=n, p=[0.7, 0.3])
    co, fo = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
    co[1:], fo[1:] = np.cumsum(n_close), np.cumsum(n_far)
    close_pts = np.zeros(int(co[-1]), dtype=binding.POINT_DTYPE)
    close_pts["abs_loc"] = rng.choice([LO - 7, LO - 1, LO, LO + 1, 5100, HI - 1, HI, HI + 3, HI + 900], size=len(close_pts))
    close_pts["length"] = rng.choice([9, 10, 11, 20, 25], size=len(close_pts))
    close_pts["direction"], close_pts["strand"] = b"+", b"+"
    far_pts = np.zeros(int(fo[-1]), dtype=binding.POINT_DTYPE)
    far_pts["abs_loc"], far_pts["length"] = 7000, 12
    recs = np.zeros(n, dtype=hostlib.EVENT_READ_DTYPE)
    recs["flags"] = rng.choice([0, hostlib.EVR_BOXED, hostlib.EVR_USED, hostlib.EVR_UNRESOLVED, hostlib.EVR_BOXED | hostlib.EVR_DUPLICATE], size=n,
                               p=[0.6, 0.1, 0.1, 0.15, 0.05])
    return dict(seqs=seqs, seq=np.frombuffer(b"".join(seqs), dtype=np.uint8) if n else np.zeros(0, np.uint8), seq_off=off, strand=strand,
                chr_id=rng.choice([0, 0, 0, 1], size=n).astype(np.int32), rc_flag=rng.choice(np.array([0, 0, 1, 2], dtype=np.uint8), size=n),
                close_off=co, close_pts=close_pts, far_off=fo, far_pts=far_pts, recs=recs)


def statement(inp, win_chr, lo, hi):
    return hostlib.li_tables_from_lists(inp["seq"], inp["seq_off"], inp["strand"], inp["chr_id"], inp["rc_flag"], inp["close_off"],
                                        inp["close_pts"], inp["far_off"], inp["recs"], win_chr, lo, hi)


def note_coverage(seen, inp, members, positions):
    """which corners of the contract this case holds"""
    n = len(inp["strand"])
    last = lambda i: inp["close_pts"][int(inp["close_off"][i + 1]) - 1]
    for s in range(2):
        for p, first, cnt, flags in positions[s]:
            raw = [int(last(i)["abs_loc"]) for i in members[s][first:first + cnt]]
            seen["lo_merge"] |= p == LO and min(raw) < LO and LO in raw
            seen["hi_merge"] |= p == HI and max(raw) > HI and HI in raw
            for i in members[s][first:first + cnt]:
                pre, post, twice = len(inp["seqs"][i]), len(post_state(inp["seqs"][i], inp["rc_flag"][i])), 2 * int(last(i)["length"])
                seen["equal_sets_neither"] |= cnt == 1 and twice == post and flags == 0
                seen["shortened_differs"] |= pre != post and np.sign(twice - pre) != np.sign(twice - post)
                seen["unresolved_included"] |= int(inp["recs"]["flags"][i]) == hostlib.EVR_UNRESOLVED
    seen["empty_strand"] |= (len(members[0]) == 0) != (len(members[1]) == 0)
    inside = set(members[0]) | set(members[1])
    for i in range(n):
        eligible = inp["chr_id"][i] == 0 and inp["close_off"][i + 1] > inp["close_off"][i] and inp["strand"][i] in b"+-"
        far, f = inp["far_off"][i + 1] > inp["far_off"][i], int(inp["recs"]["flags"][i])
        if eligible and i not in inside:
            seen["out_boxed"] |= not far and f == hostlib.EVR_BOXED
            seen["out_used"] |= not far and f == hostlib.EVR_USED
            seen["out_far"] |= far and f == 0


def test_random_arrays_against_the_literal_restatement():
    seen = dict.fromkeys(("lo_merge", "hi_merge", "equal_sets_neither", "shortened_differs", "unresolved_included", "empty_strand",
                          "out_boxed", "out_used", "out_far"), False)
    for n in (1, 2, 3, 7, 40, 64, 65, 120, 200):
        rng = np.random.default_rng(7000 + n)
        for trial in range(6):
            inp = random_input(rng, n, only_strand=ord("-") if trial == 5 else None)
            got = statement(inp, 0, LO, HI)
            members, positions = restate(inp, 0, LO, HI)
            for s in range(2):
                assert got["members"][s].tolist() == members[s], (n, trial, s)
                assert [tuple(int(x) for x in p) for p in got["positions"][s]] == positions[s], (n, trial, s)
                assert all(LO <= p[0] <= HI for p in positions[s])
            assert got["n_members"] == [len(members[0]), len(members[1])]
            note_coverage(seen, inp, members, positions)
    assert all(seen.values()), seen


def test_lo_equals_hi_and_another_chromosome():
    rng = np.random.default_rng(7)
    inp = random_input(rng, 120)
    got = statement(inp, 0, 5100, 5100)
    members, positions = restate(inp, 0, 5100, 5100)
    for s in range(2):
        assert got["members"][s].tolist() == members[s] == sorted(members[s]) and len(positions[s]) == 1
        assert [tuple(int(x) for x in p) for p in got["positions"][s]] == positions[s]
    other = statement(inp, 1, LO, HI)
    assert other["members"][0].tolist() == restate(inp, 1, LO, HI)[0][0] and set(other["members_flat"].tolist()) <= set(np.nonzero(inp["chr_id"] == 1)[0].tolist())
    with pytest.raises(ValueError):
        statement(inp, 0, 5101, 5100)


def test_empty_input():
    inp = random_input(np.random.default_rng(1), 0)
    got = statement(inp, 0, LO, HI)
    assert got["n_members"] == [0, 0] and got["n_positions"] == [0, 0] and got["members_flat"].size == 0 and got["positions_flat"].size == 0


# ------------------------------------------------------------------------------------------------ the consumer on hand-made tables
P = li.SPACER + 1500


def hand_chrom(rng):
    return b"N" * li.SPACER + bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=3000)) + b"N" * li.SPACER


def consumer_reads(seqs, strands, close_abs, close_len):
    out = []
    for i, s in enumerate(seqs):
        x = li.LIRead()
        x.name, x.seq, x.strand, x.pos, x.ms, x.tag, x.frag = f"r{i}", s, strands[i], i, 60, "S", "chrH"
        x.close_abs, x.close_len, x.has_far, x.length = close_abs[i], close_len[i], False, len(s)
        out.append(x)
    return out


def write_hand(tmp_path, name, chrom, seqs, strands, close_len, tables, min_support, marks=(), win_end=3000):
    prefix = str(tmp_path / name)
    members = [m for s in range(2) for m in tables[s][0]]
    positions = np.array([p for s in range(2) for p in tables[s][1]], dtype=hostlib.LI_POS_DTYPE)
    hostlib.li_write_from_tables(("chrH", chrom), prefix, seqs, np.frombuffer("".join(strands).encode(), dtype=np.uint8), close_len, members,
                                 positions, [len(tables[s][0]) for s in range(2)], [len(tables[s][1]) for s in range(2)], 0, win_end, 500,
                                 min_support=min_support, marks=marks, spacer=li.SPACER)
    return open(prefix + "_LI", "rb").read() if os.path.exists(prefix + "_LI") else b""


@pytest.mark.parametrize("k", [127, 128, 129])
def test_counters_saturate_in_the_consumer(tmp_path, k):
    """n_reads is not capped in the tables; the cutoff compares min(n_reads, 128): -M 128 is met by 128 and 129 members (all of them
    are written), -M 129 by no position at all."""
    rng = np.random.default_rng(k)
    chrom = hand_chrom(rng)
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=40)) for _ in range(2 * k)]
    strands = ["-"] * k + ["+"] * k
    close_abs, close_len = [P] * k + [P + 5] * k, [25] * (2 * k)
    tables = [(list(range(k, 2 * k)), [(P + 5, 0, k, hostlib.LI_LONGER)]), (list(range(k)), [(P, 0, k, hostlib.LI_LONGER)])]
    reads = consumer_reads(seqs, strands, close_abs, close_len)
    for M in (128, 129):
        got = write_hand(tmp_path, f"sat_{k}_{M}", chrom, seqs, strands, close_len, tables, M)
        assert got == li.sort_output_li(chrom, reads, set(), 0, 3000, 500, 40, ["S"], cutoff=M)
        if M == 128 and k >= 128:
            assert f"\t+ {k}\t".encode() in got and f"\t- {k}\t".encode() in got and got.count(b"\tS\tr") == 2 * k
        else:
            assert got == b""


def test_event_membership_is_blind_to_the_strand(tmp_path):
    """event_of is keyed by position whatever the strand and the last pair written wins: the '+' read at the '-' position joins the
    '+' reads of the event that took that position last, in ascending read index."""
    rng = np.random.default_rng(11)
    chrom = hand_chrom(rng)
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=40)) for _ in range(4)]
    strands, close_abs, close_len = ["-", "+", "+", "+"], [P, P, P + 5, P + 400], [12, 30, 20, 25]
    # '+' table: P (read 1), P + 5 (read 2), P + 400 (read 3, no '-' support near it); '-' table: P (read 0)
    tables = [([1, 2, 3], [(P, 0, 1, hostlib.LI_LONGER), (P + 5, 1, 1, 0), (P + 400, 2, 1, hostlib.LI_LONGER)]), ([0], [(P, 0, 1, hostlib.LI_SHORTER)])]
    got = write_hand(tmp_path, "blind", chrom, seqs, strands, close_len, tables, 1)
    want = li.sort_output_li(chrom, consumer_reads(seqs, strands, close_abs, close_len), set(), 0, 3000, 500, 40, ["S"], cutoff=1)
    assert got == want
    lines = got.split(b"\n")
    assert got.count(b"#" * 56) == 1 and f"\t{P + 5 - li.SPACER + 1}\t+ 2\t{P - li.SPACER + 1}\t- 1\t".encode() in lines[1]
    assert [l.rsplit(b"\t", 1)[1] for l in lines[3:5]] == [b"r1", b"r2"]
    # a mark within ten bases of the '-' position: the walk skips it
    assert write_hand(tmp_path, "blind_marked", chrom, seqs, strands, close_len, tables, 1, marks=[P + 3]) == b""
    assert li.sort_output_li(chrom, consumer_reads(seqs, strands, close_abs, close_len), {P + 3}, 0, 3000, 500, 40, ["S"], cutoff=1) == b""


def test_host_statement_feeds_the_consumer(tmp_path):
    """the statement's tables, given to the consumer, write what the restated reporter writes from the reads themselves"""
    rng = np.random.default_rng(12)
    chrom = hand_chrom(rng)
    n = 60
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(rng.choice([30, 40])))) for _ in range(n)]
    strands = [str(rng.choice(["+", "-"])) for _ in range(n)]
    close_abs = [int(P + rng.choice([0, 3, 8, 20, 200])) for _ in range(n)]
    close_len = [int(rng.choice([12, 15, 20, 25])) for _ in range(n)]
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    pts = np.zeros(n, dtype=binding.POINT_DTYPE)
    pts["abs_loc"], pts["length"] = close_abs, close_len
    unit = np.arange(n + 1, dtype=np.uint64)
    lo, hi = li.SPACER - 2000, li.SPACER + 3000 + 2000
    t = hostlib.li_tables_from_lists(np.frombuffer(b"".join(seqs), dtype=np.uint8), off, np.frombuffer("".join(strands).encode(), dtype=np.uint8),
                                     np.zeros(n, np.int32), np.zeros(n, np.uint8), unit, pts, np.zeros(n + 1, np.uint64),
                                     np.zeros(n, dtype=hostlib.EVENT_READ_DTYPE), 0, lo, hi)
    tables = [(t["members"][s].tolist(), [tuple(int(x) for x in p) for p in t["positions"][s]]) for s in range(2)]
    for M in (1, 3):
        got = write_hand(tmp_path, f"fed_{M}", chrom, seqs, strands, close_len, tables, M)
        assert got == li.sort_output_li(chrom, consumer_reads(seqs, strands, close_abs, close_len), set(), 0, 3000, 500, 40, ["S"], cutoff=M)
        assert got.count(b"#" * 56) >= 1


def test_synthetic_set_yields_pairs_the_walk_reports(tmp_path):
    """tests/li_cases.py, which the GPU tests search on the device: with the oracle's points, the host statement's tables hold both
    strands at every junction, a shortened read (rc_flag 2) among the members, and the consumer writes the three insertions -- the
    bytes the restated reporter writes from the reads."""
    from oracle import pyoracle
    from tests import golden_util as gu
    from tests import li_cases as lc
    chroms = lc.chromosome()
    b = lc.batch_from(lc.records(20, 10, 10) + lc.shortened_records(6))
    r = pyoracle.search_batch(pyoracle.make_params(), [s for _, s in chroms], b.seq, b.seq_off, b.anchor_strand, b.anchor_pos, b.insert_size, b.chr_id)
    co, cp = gu.csr_from_strided(r["close_cnt"], r["close_pts"])
    fo, _ = gu.csr_from_strided(r["far_cnt"], r["far_pts"])
    n = b.n
    has_close, has_far = np.diff(co.astype(np.int64)) > 0, np.diff(fo.astype(np.int64)) > 0
    assert (~has_close).sum() >= 5 and (has_close & has_far).sum() >= 10 and (has_close & ~has_far).sum() >= 100
    lo, hi = li.SPACER - 4 * lc.INSERT_SIZE, li.SPACER + 20000 + 4 * lc.INSERT_SIZE
    t = hostlib.li_tables_from_lists(b.seq, b.seq_off, b.anchor_strand, b.chr_id, r["rc_flag"], co, cp, fo, np.zeros(n, dtype=hostlib.EVENT_READ_DTYPE),
                                     0, lo, hi)
    assert sorted(t["members_flat"].tolist()) == np.nonzero(has_close & ~has_far)[0].tolist()
    assert (r["rc_flag"][t["members_flat"]] == 2).any() and min(t["n_members"]) >= 50
    raw = [b.seq[int(b.seq_off[i]):int(b.seq_off[i + 1])].tobytes() for i in range(n)]
    seqs = [post_state(raw[i], r["rc_flag"][i]) for i in range(n)]
    assert any(len(seqs[i]) == len(raw[i]) - 2 for i in t["members_flat"])
    strands = [chr(c) for c in b.anchor_strand]
    close_abs = [int(cp[int(co[i + 1]) - 1]["abs_loc"]) if has_close[i] else 0 for i in range(n)]
    close_len = [int(cp[int(co[i + 1]) - 1]["length"]) if has_close[i] else 0 for i in range(n)]
    tables = [(t["members"][s].tolist(), [tuple(int(x) for x in p) for p in t["positions"][s]]) for s in range(2)]
    reads = []
    for i in np.nonzero(has_close)[0]:
        x = li.LIRead()
        x.name, x.seq, x.strand, x.pos, x.ms, x.tag, x.frag = f"r{i}", seqs[i], strands[i], int(i), 60, "S", "chrH"
        x.close_abs, x.close_len, x.has_far, x.length = close_abs[i], close_len[i], bool(has_far[i]), len(seqs[i])
        reads.append(x)
    for M in (1, 3):
        got = write_hand(tmp_path, f"synthetic_{M}", chroms[0][1], seqs, strands, close_len, tables, M, win_end=20000)
        assert got == li.sort_output_li(chroms[0][1], reads, set(), 0, 20000, lc.INSERT_SIZE, max(len(s) for s in seqs), ["S"], cutoff=M)
        heads = [l for l in got.split(b"\n") if b"\tLI\t" in l]
        assert len(heads) >= 3
        for j in lc.JUNCTIONS:
            assert any(f"\t{j - 1 - li.SPACER + 1}\t+ ".encode() in h and f"\t{j - li.SPACER + 1}\t- ".encode() in h for h in heads), (M, j)


# ------------------------------------------------------------------------------------------------ the gold set: -l and -s from tables
gold = ec.gold                     # (the fixture: the gold set searched once by the oracle, with the lists of both classifiers)
SUFFIXES = ("D", "SI", "TD", "INV", "LI", "CloseEndMapped")


def li_run(gold, name, st, report_reads, **kw):
    prefix = str(gold["tmp"] / name)
    hostlib.call_from_points(gold["fa"], gold["reads_txt"], prefix, st, *gold["points"], variant_candidates=kw.pop("var", gold["var"]),
                             sv_candidates=kw.pop("sv", gold["sv"]), report_reads=report_reads, **kw)
    return [open(f"{prefix}_{s}", "rb").read() for s in SUFFIXES]


@pytest.mark.parametrize("threads", ["1", "16"])
@pytest.mark.parametrize("window_mbp", [5.0, 0.02, 0.005])
def test_li_and_close_end_mapped_through_the_tables_route(gold, monkeypatch, window_mbp, threads):
    from tests.test_li_pin import _expected_on_the_text_route
    monkeypatch.setenv("PGH_THREADS", threads)
    st = ec.with_fields(hostlib.default_settings(gold["mm"]), window_mbp=window_mbp, analyze_li=1, report_close_mapped=1)
    tag = f"li_{window_mbp}_{threads}"
    plain = li_run(gold, f"{tag}_plain", st, False)
    got = li_run(gold, f"{tag}_tables", st, True)
    for suf, a, b in zip(SUFFIXES, got, plain):
        assert a == b, suf
    wins = hostlib.last_event_windows()
    assert hostlib.last_event_fallback_windows() == 0 and hostlib.last_report_windows() == len(wins) > 0
    assert len(plain[4]) > 0 and plain[5].count(b"\n") % 3 == 0 and len(plain[5]) > 0
    if window_mbp == 5.0:
        assert got[4].split(b"\n") == _expected_on_the_text_route()
    # lists cut to 0 pairs: every window with a listed pair falls back, the bytes stay and _CloseEndMapped is written once per window
    from tests.test_report_reads_cpu import cut_lists
    cut = li_run(gold, f"{tag}_cut", st, True, var=cut_lists(gold["var"], 0), sv=cut_lists(gold["sv"], 0))
    for suf, a, b in zip(SUFFIXES, cut, plain):
        assert a == b, suf
    assert hostlib.last_event_fallback_windows() > 0


@pytest.mark.parametrize("fields", [dict(analyze_li=1), dict(report_close_mapped=1), dict(analyze_li=1, report_close_mapped=1, min_support=3)])
def test_either_report_alone_and_a_higher_cutoff(gold, monkeypatch, fields):
    monkeypatch.setenv("PGH_THREADS", "4")
    st = ec.with_fields(hostlib.default_settings(gold["mm"]), window_mbp=0.02, **fields)
    tag = "li_" + "_".join(f"{k}{v}" for k, v in fields.items())
    prefix = lambda rr: str(gold["tmp"] / f"{tag}_{rr}")
    out = {}
    for rr in (False, True):
        hostlib.call_from_points(gold["fa"], gold["reads_txt"], prefix(rr), st, *gold["points"], variant_candidates=gold["var"],
                                 sv_candidates=gold["sv"], report_reads=rr)
        out[rr] = {s: open(f"{prefix(rr)}_{s}", "rb").read() if os.path.exists(f"{prefix(rr)}_{s}") else None for s in SUFFIXES}
    assert out[True] == out[False]
    assert (out[True]["LI"] is not None and len(out[True]["LI"]) > 0) == bool(fields.get("analyze_li"))
    assert bool(out[True]["CloseEndMapped"]) == bool(fields.get("report_close_mapped"))
