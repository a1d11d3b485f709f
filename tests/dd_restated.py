"""Independent Python restatements of -q's pieces, written from src/search_MEI_util.cpp and src/search_MEI.cpp:
contains_subseq (with the first valid row v and the first give-up row f it implies) and the discordant-read rules,
clusters and breakpoint estimates.  Shared by tests/test_dd_cpu.py and tests/test_gpu_dd.py."""
import ctypes as C

import numpy as np

from pindel_amd import hostlib

RC4N = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def revcomp(q):
    """ReverseComplement with Convert2RC4N: anything outside ACGTN becomes NUL."""
    return "".join(RC4N.get(c, "\0") for c in reversed(q))


def contains_vf(query, db, mm, min_length=15):
    """contains_subseq (src/search_MEI_util.cpp:188-342) as a full DP: returns (result, v, f) where v = first row with a valid
    cell and f = first row whose give-up test fires (None when there is none); result is what the early exits return."""
    n, q = len(db), len(query)
    if n == 0:
        return False, None, None
    min_match = min_length - mm[min_length]
    pal, pmc = [0] * n, [0] * n
    v = f = None
    for i in range(q):
        qi = query[i]
        cal, cmc = [0] * n, [0] * n
        cal[0] = 1 if db[0] == qi else 0
        max_al = 0
        for j in range(1, n):
            best, act = 0, "n"
            s = pal[j - 1] + 1 - 2 * pmc[j - 1]
            if qi == db[j] and best < s:
                best, act = s, "m"
            else:
                s = pal[j - 1] - 2 * (pmc[j - 1] + 1)
                if best < s:
                    best, act = s, "M"
            s = cal[j - 1] - 2 * (cmc[j - 1] + 1)
            if best < s:
                best, act = s, "g"
            s = pal[j] + 1 - 2 * (pmc[j] + 1)
            if best < s:
                best, act = s, "G"
            if act == "g":
                cmc[j], cal[j] = cmc[j - 1] + 1, cal[j - 1]
            elif act == "G":
                cmc[j], cal[j] = pmc[j] + 1, pal[j] + 1
            elif act == "m":
                cmc[j], cal[j] = pmc[j - 1], pal[j - 1] + 1
            elif act == "M":
                cmc[j], cal[j] = pmc[j - 1] + 1, pal[j - 1] + 1
            else:
                cmc[j], cal[j] = (0 if qi == db[j] else 1), 1
            if v is None and cal[j] >= min_length and cmc[j] <= mm[cal[j]]:
                v = i
            max_al = max(max_al, cal[j])
        if f is None and (q - i - 1) + max_al < min_match:
            f = i
        if v is not None or (f is not None and i >= f + 1):
            # the result is decided; one row past f tells v == f + 1 apart
            break
        pal, pmc = cal, cmc
    return (v is not None and (f is None or v <= f)), v, f


def contains_any_strand(query, db, mm):
    return contains_vf(query, db, mm)[0] or contains_vf(revcomp(query), db, mm)[0]


def cpu_contains(queries, dbs, mm, threads=16):
    """The host library's C++ restatement (pgh_dd_contains_cpu)."""
    L = hostlib.lib()
    L.pgh_dd_contains_cpu.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    qb = [q.encode("latin-1") for q in queries]
    db = [d.encode("latin-1") if isinstance(d, str) else bytes(d) for d in dbs]
    qa = np.frombuffer(b"".join(qb) + b"\0", dtype=np.uint8)
    da = np.frombuffer(b"".join(db) + b"\0", dtype=np.uint8)
    qo = np.concatenate([[0], np.cumsum([len(x) for x in qb])]).astype(np.uint64)
    do = np.concatenate([[0], np.cumsum([len(x) for x in db])]).astype(np.uint64)
    mm = np.ascontiguousarray(mm[:500], dtype=np.uint32)
    out = np.zeros(max(1, len(qb)), dtype=np.uint8)
    assert L.pgh_dd_contains_cpu(len(qb), qa.ctypes.data, qo.ctypes.data, da.ctypes.data, do.ctypes.data, mm.ctypes.data,
                                 out.ctypes.data, threads) == 0
    return out[:len(qb)]


DD_DEFAULTS = (350, 100, 3, 3, 8000, 0)


def dd_run(fasta, config, prefix, mm, opts=DD_DEFAULTS, close_cb=None, window_mbp=5.0, spacer=100000, anchor_q=0, nm=2, mm_rate=0.02,
           region=None):
    """pgh_dd_run: the -q pipeline on the host (close ends from close_cb, containment on the CPU).
    Returns (stats6, breakpoints as (tid, pos, strand, n_reads, n_split), tested as (tid, pos, strand, n_split, consensus, contained))."""
    L = hostlib.lib()
    L.pgh_dd_run.restype = C.c_int64
    L.pgh_dd_run.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_double, C.c_char_p, C.c_char_p, C.c_char_p, C.c_double,
                             C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint64]
    o = np.array(list(opts) + [anchor_q, nm], dtype=np.int32)
    mm = np.ascontiguousarray(mm[:500], dtype=np.uint32)
    st = np.zeros(6, dtype=np.uint64)
    bp = np.zeros(5 * 4096, dtype=np.int32)
    tested = C.create_string_buffer(1 << 20)
    n = L.pgh_dd_run(str(fasta).encode(), str(config).encode(), str(prefix).encode(), o.ctypes.data, mm_rate,
                     region.encode() if region else None, None, None, window_mbp, spacer, mm.ctypes.data,
                     C.cast(close_cb, C.c_void_p) if close_cb is not None else None, st.ctypes.data, bp.ctypes.data, 4096, tested, 1 << 20)
    assert n >= 0, L.pgh_last_error()
    t = [x.split("\t") for x in tested.value.decode().splitlines()]
    return ([int(x) for x in st], [(int(a), int(b), chr(c), int(d), int(e)) for a, b, c, d, e in bp[:5 * n].reshape(-1, 5)],
            [(int(a), int(b), c, int(d), e, f == "1") for a, b, c, d, e, f in t])


def consensus_unmapped(unmapped, strand):
    """get_consensus_unmapped (src/search_MEI.cpp:156-218) on the unmapped parts of a candidate's split reads; strand = the split
    reads' mapping strand (the opposite of the cluster's)."""
    if not unmapped:
        return ""
    max_len = max(len(u) for u in unmapped)
    out = []
    for i in range(max_len):
        counts = {}
        n = 0
        for u in unmapped:
            k = i if strand == "-" else len(u) - 1 - i
            if 0 <= k < len(u):
                n += 1
                counts[u[k]] = counts.get(u[k], 0) + 1
        best_c, best = "?", 0
        for ch in sorted(counts):
            if counts[ch] > best:
                best_c, best = ch, counts[ch]
        if best >= np.float32(0.8) * np.float32(n):
            out.append(best_c)
        else:
            break
    s = "".join(out)
    if len(s) < 15:
        return ""
    return s[::-1] if strand == "+" else s


CLOSE_CB = C.CFUNCTYPE(C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)


def restated_breakpoint_estimates(recs, n_chr, insert_size, min_map=8000, max_dist=100, min_cluster=3):
    """fetch_disc_read_callback + is_concordant + cluster_reads + get_breakpoint_estimation on decoded BAM records (one window per
    chromosome: these are shorter than the -w window).  Returns (discordant per chromosome, clusters, estimates)."""
    n_disc, clusters, est = [], [], []
    for tid in range(n_chr):
        reads = []
        for r in recs:
            if r["tid"] != tid or r["flag"] & 12:
                continue
            rev, mrev = bool(r["flag"] & 16), bool(r["flag"] & 32)
            conc = r["tid"] == r["mtid"] and rev != mrev and abs(r["tlen"]) < len(r["seq"]) + 2 * insert_size
            if conc or not (r["tid"] != r["mtid"] or abs(r["pos"] - r["mpos"]) > min_map):
                continue
            reads.append(("-" if rev else "+", r["pos"], len(r["seq"]), tid))
        n_disc.append(len(reads))
        # comp_simple_read: '+' first, then position (the demo has no ties)
        reads.sort(key=lambda x: (x[0] != "+", x[1]))
        cl = []
        for r in reads:
            if cl and r[1] - cl[-1][-1][1] <= max_dist and (r[1] - cl[-1][0][1]) <= insert_size - cl[-1][0][2] and r[0] == cl[-1][-1][0]:
                cl[-1].append(r)
            else:
                cl.append([r])
        clusters += cl
        for c in cl:
            if len(c) < min_cluster:
                continue
            dist = np.float32(0)
            for i in range(len(c) - 1):
                dist = np.float32(np.float64(dist) + (1.0 / (i + 1)) * np.float64(np.float32(c[i + 1][1] - c[i][1]) - dist))
            high = c[-1][1] + c[-1][2]
            low = c[0][1]
            e = np.float32(high) + dist if c[0][0] == "+" else np.float32(low) - dist
            est.append((tid, int(e), c[0][0], len(c)))
    return n_disc, clusters, est


def oracle_close_cb(seqs):
    """A pgh_dd_run close-end callback from the CPU oracle (oracle/pyoracle.py) on the padded chromosomes `seqs`."""
    from oracle import pyoracle
    p = pyoracle.make_params()

    def cb(n, seq, off, strand, pos, isz, chr_, has, rcf, last_abs, last_len):
        offs = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), (n + 1,)).copy()
        args = [np.ctypeslib.as_array(C.cast(seq, C.POINTER(C.c_uint8)), (int(offs[-1]),)).copy(), offs]
        for ptr, ty in ((strand, C.c_uint8), (pos, C.c_int32), (isz, C.c_int16), (chr_, C.c_int32)):
            args.append(np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ty)), (n,)).copy())
        r = pyoracle.search_batch(p, seqs, *args, do_far=False)
        h = np.ctypeslib.as_array(C.cast(has, C.POINTER(C.c_uint8)), (n,))
        f = np.ctypeslib.as_array(C.cast(rcf, C.POINTER(C.c_uint8)), (n,))
        la = np.ctypeslib.as_array(C.cast(last_abs, C.POINTER(C.c_uint32)), (n,))
        ll = np.ctypeslib.as_array(C.cast(last_len, C.POINTER(C.c_uint16)), (n,))
        for i in range(n):
            k = int(r["close_cnt"][i])
            h[i] = k > 0
            f[i] = r["rc_flag"][i]
            if k:
                last = r["close_pts"][i][k - 1]
                la[i], ll[i] = int(last["abs_loc"]), int(last["length"])
        return 0
    return CLOSE_CB(cb)
