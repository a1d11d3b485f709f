"""The contract of the dispersed-duplication breakpoint tables (include/pindel_pg.h) restated literally in Python:
dict counting, `sorted` over signed bytes, and the reference's float test max >= np.float32(0.8) * n.  hostlib.dd_tables_from_close
(the host statement) and Engine.dd_tables (the device) are compared with it.  The containment verdict comes from a callback."""
import numpy as np

from pindel_amd import hostlib

_RC = {ord("A"): ord("T"), ord("C"): ord("G"), ord("G"): ord("C"), ord("T"): ord("A"), ord("N"): ord("N")}


def rc4n(b):
    """Convert2RC4N: unset entries are 0"""
    return _RC.get(b, 0)


def signed(b):
    return b - 256 if b >= 128 else b


def apply_rc_flag(seq: bytes, flag: int) -> bytes:
    """rc_flag applications of setUnmatchedSeq(ReverseComplement()): reverse complement, then trailing non-alphanumerics go"""
    for _ in range(min(int(flag), 2)):
        seq = bytes(rc4n(c) for c in reversed(seq))
        while seq and not chr(seq[-1]).isalnum():
            seq = seq[:-1]
    return seq


def walk_of(seq: bytes, rc_flag: int, close_len: int, plus: bool) -> bytes:
    """the unmapped bases of one member walking away from the breakpoint: column i of the contract"""
    s = apply_rc_flag(seq, rc_flag)
    u = max(len(s) - close_len, 0)
    if plus:
        return bytes(rc4n(s[len(s) - 1 - close_len - i]) for i in range(u))
    return bytes(s[u - 1 - i] for i in range(u))


def consensus_of(walks, plus: bool, stats=None) -> bytes:
    """get_consensus_unmapped over the members' walks; b"" for a consensus of fewer than 15 columns.  stats (a dict): what occurred."""
    out = []
    for i in range(max((len(w) for w in walks), default=0)):
        counts, n = {}, 0
        for w in walks:
            if len(w) > i:
                n += 1
                counts[w[i]] = counts.get(w[i], 0) + 1
        best_c, best = ord("?"), 0
        for ch in sorted(counts, key=signed):                  # std::map<char,int> in order, a strict >
            if counts[ch] > best:
                best_c, best = ch, counts[ch]
        ok = bool(best >= np.float32(0.8) * np.float32(n))
        if stats is not None:
            stats.setdefault("votes", set()).add((best, n, ok))
            if sum(1 for v in counts.values() if v == best) > 1:
                stats.setdefault("ties", []).append((sorted(k for k, v in counts.items() if v == best), best_c))
            if best_c == 0 and ok:
                stats["nul_won"] = True
            stats.setdefault("n_per_column", []).append(n)
        if not ok:
            break
        out.append(best_c)
    if stats is not None:
        stats.setdefault("columns", []).append(len(out))
    if len(out) < 15:
        return b""
    return bytes(out) if plus else bytes(reversed(out))


def tables(seqs, strands, has, rc_flag, last_abs, last_len, seg_first, seg_strand, chr_len, min_bp_support, min_map_distance, contains,
           stats=None):
    """members, cands, cons as the contract words them.  seqs: the reads' bytes as handed to the search; strands: their anchor strands
    (bytes of length n); contains(consensus, win_start, win_len) -> bool."""
    n = len(seqs)
    seg_strand = bytes(seg_strand.encode() if isinstance(seg_strand, str) else seg_strand)
    keys = {}
    for s in range(len(seg_strand)):
        for i in range(int(seg_first[s]), min(int(seg_first[s + 1]), n)):
            if has[i] and strands[i] == seg_strand[s]:
                keys.setdefault((s, int(last_abs[i])), []).append(i)        # (ascending read index: the loop's own order)
    members, cands, cons = [], [], b""
    for (s, pos) in sorted(keys):                                           # pos is unsigned here
        reads = keys[(s, pos)]
        if stats is not None:
            stats.setdefault("support", set()).add(len(reads))
        if min_bp_support > 1 and len(reads) < min_bp_support:
            continue
        plus = seg_strand[s] == ord("+")
        first = len(members)
        walks = []
        for i in reads:
            members.append((i, int(last_len[i]), int(rc_flag[i]), 0))
            walks.append(walk_of(bytes(seqs[i]), int(rc_flag[i]), int(last_len[i]), plus))
        st = {} if stats is not None else None
        c = consensus_of(walks, plus, st)
        if stats is not None:
            stats.setdefault("cands", []).append(dict(seg=s, pos=pos, n=len(reads), lens=[len(w) for w in walks], **st))
        flags = win_len = win_start = 0
        if c:
            flags = hostlib.DD_TESTED
            pos_i = pos - (1 << 32) if pos >= 1 << 31 else pos               # (int)pos
            win_start = max(0, pos_i - min_map_distance)
            if win_start < chr_len:
                win_len = min(((chr_len & 0xffffffff) - win_start) & 0xffffffff, (2 * min_map_distance) & 0xffffffff)
            if contains(c, win_start, win_len):
                flags |= hostlib.DD_CONTAINED
        cands.append((s, pos, first, len(reads), len(cons), len(c), flags, win_len, win_start))
        cons += c
    return dict(members=np.array(members, dtype=hostlib.DD_MEMBER_DTYPE).reshape(-1), cands=np.array(cands, dtype=hostlib.DD_CAND_DTYPE).reshape(-1),
                cons=cons)


def consumer(names, seqs, strands, n_seg, t, sample="S", spacer=100000):
    """The consumer: per segment the candidates in the order of std::map<int> over (int)(pos - spacer), each with its reads as
    get_breakpoints makes them, here in table order.  The consumer itself leaves them as std::sort by descending unmapped length does,
    which is not stable: a caller compares the reads as multisets and their unmapped lengths as a descending sequence."""
    out = []
    for s in range(n_seg):
        idx = [e for e in range(len(t["cands"])) if int(t["cands"][e]["seg"]) == s]

        def bio(e):
            v = (int(t["cands"][e]["pos"]) - spacer) & 0xffffffff
            return v - (1 << 32) if v >= 1 << 31 else v
        for e in sorted(idx, key=bio):
            c = t["cands"][e]
            reads = []
            for m in t["members"][int(c["first"]):int(c["first"]) + int(c["n_reads"])]:
                i = int(m["read"])
                q = apply_rc_flag(bytes(seqs[i]), int(m["rc_flag"]))
                k = int(m["close_len"])
                if strands[i] == ord("+"):
                    q = bytes(rc4n(b) for b in reversed(q))
                    mapped, unmapped = q[:k], q[k:]
                else:
                    mapped, unmapped = q[len(q) - k:], q[:len(q) - k]
                reads.append((names[i], sample, q.decode("latin-1"), mapped.decode("latin-1"), unmapped.decode("latin-1")))
            out.append((s, bio(e), bool(int(c["flags"]) & hostlib.DD_TESTED), bool(int(c["flags"]) & hostlib.DD_CONTAINED),
                        t["cons"][int(c["cons_off"]):int(c["cons_off"]) + int(c["cons_len"])].decode("latin-1"), reads))
    return out
