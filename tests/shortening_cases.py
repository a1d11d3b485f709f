"""Reads that BEGIN or END with characters outside ACGTN, and what the reference does with them (round 6: the last known
divergence of oracle and kernels from Pindel 0.2.5b9 is closed).

Source (written out by hand from it):
  * GetCloseEnd, src/pindel.cpp:2531-2575: attempts (R0, seq), then "setUnmatchedSeq(ReverseComplement(seq))" and (R0, seq'),
    then (R1, seq'), then setUnmatchedSeq(ReverseComplement(seq')) and (R1, seq'').
  * ReverseComplement, :2037-2048 with Convert2RC4N, :966-970: every character that is not one of ACGTN becomes NUL.
  * setUnmatchedSeq, :142-169: trailing characters that are not alphanumeric are stripped; ReadLength, MAX_SNP_ERROR and
    TOTAL_SNP_ERROR_CHECKED are recomputed from the new length.
So for a read s = J + X + K (J / K = the leading / trailing runs of characters outside ACGTN, X clean at both ends):
  seq'  = RC(s) without its last |J| characters   = NUL^|K| + RC(X)          length n - |J|
  seq'' = RC(seq') without its last |K| characters = X (inner junk -> NUL)    length n - |J| - |K|
and a read the first attempt does not place is searched, from then on, exactly like the SHORTER read: attempts 1 and 2 see seq',
attempt 3 sees seq'', the far end sees whichever GetCloseEnd left.  The cases below are built so that this can be stated as an
equivalence with a CLEAN read whose result is pinned elsewhere (gold reports, the rest of the suite):

  lead   s = J + RC(c)        c a clean split read that keeps its close end at attempt 0 (rc_flag 0).  seq' = c: whenever attempt 0
                              on s finds nothing, s must give exactly c's UP_Close and UP_Far, rc_flag 1, ReadLength |c|.
  trail  s = c + K, anchor moved one insert size so that c's close end lies in the R = 1 window only: attempts 0-2 find nothing
                              (no seed: the first consumed character is junk / NUL), attempt 3 sees seq'' = c: s must give what the
                              clean read c gives with the same moved anchor when THAT is found at attempt 3, rc_flag 2, ReadLength |c|.
  126    lead with |c| = 125, |J| = 1: ReadLength drops from 126 to 125 and g_maxMismatch from 5 to 4 (one level fewer).
"""
import numpy as np

from pindel_amd import synth
from pindel_amd.synth import ReadBatch

_COMP = np.zeros(256, dtype=np.uint8)
for a, b in zip(b"ACGTN", b"TGCAN"):
    _COMP[a] = b


def rc_ref(s: bytes) -> bytes:
    """ReverseComplement with Convert2RC4N: characters outside ACGTN become NUL."""
    return _COMP[np.frombuffer(s, dtype=np.uint8)][::-1].tobytes()


def batch_of(seqs, strand, pos, isz, chr_id=0):
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return ReadBatch(seq=np.frombuffer(b"".join(seqs), dtype=np.uint8).copy(), seq_off=off,
                     anchor_strand=np.asarray(strand, dtype=np.uint8), anchor_pos=np.asarray(pos, dtype=np.int32),
                     insert_size=np.asarray(isz, dtype=np.int16),
                     chr_id=np.full(len(seqs), chr_id, dtype=np.int32) if np.isscalar(chr_id) else np.asarray(chr_id, dtype=np.int32))


def seqs_of(batch):
    return [batch.seq[int(batch.seq_off[i]):int(batch.seq_off[i + 1])].tobytes() for i in range(batch.n)]


def clean_reads(ref, n, read_len, seed):
    """split reads (deletions, insertions, duplications) in the orientation attempt 0 tries"""
    return synth.make_reads(ref, n, seed=seed, read_len=read_len, mix=(0.6, 0.2, 0.2, 0.0, 0.0), rc_retry_frac=0.0, n_rate=0.0)


def lead_case(clean, junk: bytes):
    """s = junk + RC(c) for every clean read c, same anchors"""
    return batch_of([junk + rc_ref(c) for c in seqs_of(clean)], clean.anchor_strand, clean.anchor_pos, clean.insert_size)


def moved(clean):
    """the same reads with the anchor one insert size further from the close end: R = 0 misses it, R = 1 holds it"""
    plus = clean.anchor_strand == ord("+")
    pos = np.where(plus, clean.anchor_pos.astype(np.int64) + clean.insert_size, clean.anchor_pos.astype(np.int64) - clean.insert_size)
    return ReadBatch(seq=clean.seq, seq_off=clean.seq_off, anchor_strand=clean.anchor_strand, anchor_pos=pos.astype(np.int32),
                     insert_size=clean.insert_size, chr_id=clean.chr_id)


def trail_case(clean_moved, junk: bytes):
    return batch_of([c + junk for c in seqs_of(clean_moved)], clean_moved.anchor_strand, clean_moved.anchor_pos, clean_moved.insert_size)


def inner_case(clean, at: int, ch: bytes = b"R"):
    """one character outside ACGTN INSIDE the read: the length never changes, two reverse complements leave a NUL there"""
    return batch_of([c[:at] + ch + c[at + 1:] for c in seqs_of(clean)], clean.anchor_strand, clean.anchor_pos, clean.insert_size)


def concat(batches):
    off = [np.zeros(1, dtype=np.uint64)]
    base = 0
    for b in batches:
        off.append(b.seq_off[1:].astype(np.uint64) + np.uint64(base))
        base += len(b.seq)
    return ReadBatch(seq=np.concatenate([b.seq for b in batches]), seq_off=np.concatenate(off),
                     anchor_strand=np.concatenate([b.anchor_strand for b in batches]),
                     anchor_pos=np.concatenate([b.anchor_pos for b in batches]),
                     insert_size=np.concatenate([b.insert_size for b in batches]),
                     chr_id=np.concatenate([b.chr_id for b in batches]))


# ------------------------------------------------------------------ the read as the close end left it (the two far-end seams)
# GetCloseEnd leaves a read "setUnmatchedSeq(ReverseComplement())"-ed rc_flag times (0, 1 or 2).  pg_far_end_batch_from_close takes
# that post-state as it is; pg_far_end_batch takes it with the reads of an odd flag reverse-complemented back (what
# pg_adapter::make_batch(..., un_rc) uploads) together with the flags.  For a read with characters outside ACGTN neither is the
# read that was first handed to the close end.
_ALNUM = frozenset(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz")


def flip(s: bytes) -> bytes:
    """setUnmatchedSeq(ReverseComplement(s)): rc_ref, then the trailing bytes that are not alphanumeric go (pindel.cpp:142-157)"""
    r = rc_ref(s)
    n = len(r)
    while n > 0 and r[n - 1] not in _ALNUM:
        n -= 1
    return r[:n]


def _with_seqs(batch, seqs):
    return batch_of(seqs, batch.anchor_strand, batch.anchor_pos, batch.insert_size, batch.chr_id)


def post_state(batch, rc_flag):
    """every read flipped rc_flag[i] times: UnmatchedSeq as GetCloseEnd left it"""
    out = []
    for s, f in zip(seqs_of(batch), rc_flag):
        assert 0 <= int(f) <= 2
        for _ in range(int(f)):
            s = flip(s)
        out.append(s)
    return _with_seqs(batch, out)


def unflipped(post_batch, rc_flag):
    """what pg_adapter::make_batch(reads, chr_of, rc_flag) uploads: the reverse complement (everything but ACGTN -> NUL, nothing
    stripped) where flag & 1, the read unchanged otherwise -- a flag of 2 leaves it as it is"""
    return _with_seqs(post_batch, [rc_ref(s) if int(f) & 1 else s for s, f in zip(seqs_of(post_batch), rc_flag)])


def close_back(result):
    """UP_Close.back() per read from the last run of its close list: (has a close end, AbsLoc as uint32, LengthStr as int16);
    0 / 0 for a read without one"""
    off = result.close_off.astype(np.int64)
    has = np.diff(off) > 0
    last_run = result.close_runs[off[1:][has] - 1]
    d = last_run["len_last"].astype(np.int64) - last_run["len_first"]
    back = (last_run["flags"] & 1) != 0
    loc = np.zeros(len(has), dtype=np.int64)
    loc[has] = np.where(back, last_run["abs_loc_first"].astype(np.int64) - d, last_run["abs_loc_first"].astype(np.int64) + d)
    mx = np.zeros(len(has), dtype=np.int16)
    mx[has] = last_run["len_last"].astype(np.int16)
    return has, loc.astype(np.uint32), mx


# The families of the far-seam tests (tests/test_seam_states_cpu.py, tests/test_gpu_far_seam_states.py): L is the length of the clean
# read c, i.e. of the post-state of the lead / trail families; the ORIGINAL read is |junk| longer.
#   family         original read                      post-state
#   trail, trail2  c + "R", c + "RK", moved anchor    c, rc_flag 2          (clean again: not a read of the exact list any more)
#   lead           "R" + RC(c)                        c, rc_flag 1
#   lead_of_trail  "W" + RC(c + "S"), moved anchor    c, rc_flag 1
#   inner_*        c with an R at 0, L // 2 or L - 1, moved anchor: NUL inside (or stripped at the end), rc_flag 0 / 1 / 2
SEAM_FAMILIES = ("trail", "trail2", "lead", "lead_of_trail", "inner_mid", "inner_first", "inner_last")
# seeds of the clean reads per L, chosen on the oracle alone so that every batch clears the counts the tests assert
SEAM_SEED = {64: 78, 100: 82, 125: 81, 128: 79, 192: 80}


def seam_family(ref_seq, family, L, n=300, seed=None):
    c = clean_reads(ref_seq, n, L, seed=SEAM_SEED[L] if seed is None else seed)
    if family == "trail":
        return trail_case(moved(c), b"R")
    if family == "trail2":
        return trail_case(moved(c), b"RK")
    if family == "lead":
        return lead_case(c, b"R")
    if family == "lead_of_trail":
        return lead_case(trail_case(moved(c), b"S"), b"W")
    if family == "inner_mid":
        return inner_case(moved(c), L // 2)
    if family == "inner_first":
        return inner_case(moved(c), 0)
    if family == "inner_last":
        return inner_case(moved(c), L - 1)
    raise KeyError(family)


def seam_mixed(ref_seq, L, per=25, n_plain=4000):
    """`per` reads of every family scattered among ordinary reads of the same length: all the post-states in one launch"""
    plain = synth.make_reads(ref_seq, n_plain, seed=500 + L, read_len=L)
    step = n_plain // len(SEAM_FAMILIES)
    parts = []
    for k, fam in enumerate(SEAM_FAMILIES):
        parts.append(plain.slice(step * k, step * (k + 1) if k + 1 < len(SEAM_FAMILIES) else n_plain))
        parts.append(seam_family(ref_seq, fam, L).slice(40 * k, 40 * k + per))
    return concat(parts)


def has_junk(s: bytes) -> bool:
    return any(ch not in b"ACGTN" for ch in s)


def same_points(a, i, b, j):
    for which in ("close", "far"):
        ca, cb = int(a[which + "_cnt"][i]), int(b[which + "_cnt"][j])
        if ca != cb or a[which + "_pts"][i][:ca].tobytes() != b[which + "_pts"][j][:cb].tobytes():
            return False
    return True
