"""Helpers shared by tests/test_interchr_cpu.py and tests/test_gpu_interchr.py: the C entries -I added, and the way from an
oracle search result to the read lists tests/interchr_restated.py takes."""
import ctypes as C

import numpy as np

from oracle import pyoracle
from pindel_amd import hostio, hostlib
from tests import bam_writer as bw
from tests import interchr_restated as ir

SPACER = 100000
F = bw.FLAG


def lib():
    L = hostlib.lib()
    L.pgh_rp_events_chr.restype = C.c_int64
    L.pgh_rp_events_chr.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.c_int32, C.c_char_p, C.c_uint32, C.c_uint32, C.c_int32,
                                    C.c_char_p, C.c_void_p, C.c_uint64]
    L.pgh_rp_interchr_pairs.restype = C.c_int64
    L.pgh_rp_interchr_pairs.argtypes = [C.c_uint32] + [C.c_void_p] * 9 + [C.c_int32, C.POINTER(C.c_char_p), C.c_int32, C.POINTER(C.c_char_p),
                                                                        C.c_uint32, C.c_char_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_double)]
    L.pgh_window_hints_chr.restype = C.c_int64
    L.pgh_window_hints_chr.argtypes = [C.c_char_p, C.c_char_p, C.c_int32, C.POINTER(C.c_char_p), C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                                       C.c_int32, C.c_char_p, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_uint64, C.c_void_p, C.c_uint64]
    L.pgh_int_final.argtypes = [C.c_char_p, C.c_char_p]
    L.pgh_bd_query.argtypes = [C.c_char_p, C.c_uint32, C.c_int32, C.POINTER(C.c_char_p), C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    return L


def c_names(names):
    return (C.c_char_p * len(names))(*[n.encode() for n in names])


def events_from(out, n, names):
    return [(names[int(out[6 * i])], int(out[6 * i + 1]), int(out[6 * i + 2]), names[int(out[6 * i + 3])], int(out[6 * i + 4]),
             int(out[6 * i + 5])) for i in range(n)]


def cluster_pairs(pairs, names, tags, rp_path, seconds=None):
    """the C++ interchromosomal clustering on `pairs` (dicts as tests/interchr_restated.rp_interchr takes) -> (events, _RP text)"""
    L = lib()
    n = len(pairs)
    ni, ti = {x: i for i, x in enumerate(names)}, {x: i for i, x in enumerate(tags)}
    a = lambda key, dt, f=lambda v: v: np.array([f(p[key]) for p in pairs], dtype=dt)
    arrs = [a("ChrNameA", np.int32, ni.get), a("ChrNameB", np.int32, ni.get), a("DA", np.uint8, ord), a("DB", np.uint8, ord),
            a("PosA", np.uint32), a("PosB", np.uint32), a("InsertSize", np.int32), a("ReadLength", np.int16), a("Tag", np.int32, ti.get)]
    out = np.zeros(6 * max(n, 1), dtype=np.int64)
    sec = C.c_double()
    k = L.pgh_rp_interchr_pairs(n, *[x.ctypes.data for x in arrs], len(names), c_names(names), len(tags), c_names(tags), SPACER,
                                str(rp_path).encode(), out.ctypes.data, max(n, 1), C.byref(sec))
    assert k >= 0, L.pgh_last_error()
    if seconds is not None:
        seconds.append(sec.value)
    return events_from(out, k, names), open(rp_path).read()


def discover_interchr(records, tid, ws, we, isz, tag, names, min_q=0):
    """build_record_RP_Discovery restated for the pairs whose mate lies on another chromosome: the records of chromosome
    `tid` that reach into [ws, we), in file order"""
    out = []
    for r in records:
        if r["tid"] != tid or r["flag"] & F["UNMAP"] or not r["cigar"]:
            continue
        end = r["pos"] + sum(n for op, n in r["cigar"] if op in (0, 2, 3, 7, 8))
        if not (r["pos"] < we and end > ws):
            continue
        if not r["flag"] & F["PAIRED"] or r.get("mapq", 0) < min_q or r["flag"] & F["MUNMAP"]:
            continue
        if r["tid"] == r["mtid"]:
            continue
        out.append(dict(ChrNameA=names[r["tid"]], ChrNameB=names[r["mtid"]], DA="-" if r["flag"] & F["REVERSE"] else "+",
                        DB="-" if r["flag"] & F["MREVERSE"] else "+", PosA=r["pos"], PosB=r["mpos"], InsertSize=isz,
                        ReadLength=len(r["seq"]), Tag=tag))
    return out


_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def restated_reads(names, chroms, got, res, fragname):
    """The reads of one window that kept a close end, as interchr_restated.int_lines takes them.  got: (name, seq, strand, pos,
    ...) per read in input order; res: pyoracle.search_batch's result for them; fragname: the window's chromosome."""
    out = []
    for i, g in enumerate(got):
        nc, nf = int(res["close_cnt"][i]), int(res["far_cnt"][i])
        if nc == 0:
            continue
        seq = g[1].encode()
        for _ in range(min(int(res["rc_flag"][i]), 2)):
            seq = seq.translate(_COMP)[::-1]
        cp, fp = res["close_pts"][i][:nc], res["far_pts"][i][:nf]
        r = dict(Name=g[0], FragName=fragname, FarFragName="", MatchedD=g[2], MatchedFarD="", ReadLength=len(seq),
                 UnmatchedSeq=seq.decode(), UP_Close=[(int(p["length"]), int(p["abs_loc"])) for p in cp],
                 UP_Far=[(int(p["length"]), int(p["abs_loc"])) for p in fp])
        if nf:
            r["FarFragName"] = names[int(fp[0]["chr_id"])]
            r["MatchedFarD"] = fp[0]["strand"].decode()
        out.append(r)
    return out


def batch_of(got, cid):
    return hostio.batch_from_lists([g[1].encode() for g in got], [g[2].encode() for g in got], [g[3] for g in got], [g[5] for g in got],
                                   [cid] * len(got))


def oracle_with_windows(chroms, b, windows_of):
    """close end by the oracle, then windows_of(last close AbsLoc per read (0 = no close end)) -> (n + 1 offsets, k x 3 windows),
    then the whole search with the windows of the reads that kept a close end"""
    p = pyoracle.make_params()
    seqs = [s for _, s in chroms]
    args = (b.seq, b.seq_off, b.anchor_strand, b.anchor_pos, b.insert_size, b.chr_id)
    close = pyoracle.search_batch(p, seqs, *args, do_far=False)
    last = np.array([int(close["close_pts"][i][close["close_cnt"][i] - 1]["abs_loc"]) if close["close_cnt"][i] else 0
                     for i in range(b.n)], dtype=np.uint32)
    off, win = windows_of(last)
    cnt = np.diff(np.asarray(off).astype(np.int64))
    keep = np.repeat(close["close_cnt"] > 0, cnt)
    cnt[close["close_cnt"] == 0] = 0
    w3 = np.asarray(win, dtype=np.int32).reshape(-1, 3)[keep]
    bd = np.zeros(len(w3), dtype=pyoracle.WINDOW_DTYPE)
    bd["chr_id"], bd["start"], bd["end"] = w3[:, 0], w3[:, 1], w3[:, 2]
    bd_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
    return pyoracle.search_batch(p, seqs, *args, bd=bd, bd_off=bd_off)


def int_reports(per_window_reads):
    """[reads of window 1, reads of window 2, ...] -> (_INT text, _INT_final text, reads collected per window)"""
    text, collected = "", []
    for reads in per_window_reads:
        t, n = ir.int_lines(reads, SPACER)
        text += t
        collected.append(n)
    return text, ir.int_final(text), collected
