"""Constructed reads for the tests of the DI, tandem-duplication and inversion candidate lists (tests/test_sv_candidates_cpu.py,
tests/test_gpu_sv_candidates.py), built from variant_cases.split_read and shortening_cases.  Every case is (name,
chromosomes, batch, settings) with settings = None (Pindel's defaults) or (-e, -d, -v); check_case asserts on the host arrays
that the case exercises its path, so a case that stops doing so fails loudly.

Coordinates: a tandem duplication of bio[s:e) gives the junction read bio[e-a:e] + bio[s:s+b]; an inversion of bio[s:e) gives
four junction reads, one per geometry of searchInversions (0: '+' anchor left of s, 1: '+' anchor inside, close end at e; 2: '-'
anchor right of e, 3: '-' anchor inside, close end at s).

Not here, because no search produces them: a LeftMostTD walk of more than 64 steps and one cut by its diff >= BP
clamp -- the loops visit the leftmost junction first; tests/sv_align_unit.cpp covers both."""
import numpy as np

from tests import shortening_cases as sc
from tests.shortening_cases import rc_ref
from tests.variant_cases import as_batch, both_strands, padded, rand_bases

KIND = {"DI": 2, "TD": 3, "TD_NT": 4, "INV": 5, "INV_NT": 6}


def unlike(follows, precedes):
    """Non-template bases that differ, place by place, from what follows the left part in the reference and from what precedes the
    right part: neither part can be extended into them, so the lengths of the parts are exact."""
    assert len(follows) == len(precedes)
    return bytes(next(c for c in b"ACGT" if c != x and c != y) for x, y in zip(follows, precedes))


def split_nt(bio, left_start, left_len, right_start, read_len, n_nt, **kw):
    """both_strands of variant_cases with n_nt non-template bases made by unlike()"""
    ins = unlike(bio[left_start + left_len:left_start + left_len + n_nt], bio[right_start - n_nt:right_start])
    return both_strands(bio, left_start, left_len, right_start, read_len, ins=ins, **kw)


def joined(left, right, plus, anchor, ins=b"", mutate=()):
    """A read whose forward sequence is left + ins + right; '+' anchors get it reverse-complemented (variant_cases.split_read)."""
    fwd = bytearray(left + ins + right)
    for at in mutate:
        fwd[at] = ord("A") if fwd[at] != ord("A") else ord("C")
    return (rc_ref(bytes(fwd)), ord("+"), anchor) if plus else (bytes(fwd), ord("-"), anchor)


def inversion_read(bio, s, e, geo, L, a, n_nt=0, slack=120, mutate=()):
    """The junction read of geometry geo of an inversion of bio[s:e): a bases of close end, n_nt non-template bases, the rest far end."""
    b = L - a - n_nt
    n = n_nt
    ins = b""
    if n:
        follows = (bio[s:s + n], bio[e:e + n], rc_ref(bio[s - n:s]), rc_ref(bio[e - n:e]))[geo]
        precedes = (rc_ref(bio[e:e + n]), rc_ref(bio[s:s + n]), bio[e - n:e], bio[s - n:s])[geo]
        ins = unlike(follows, precedes)
    if geo == 0:
        return joined(bio[s - a:s], rc_ref(bio[e - b:e]), True, s - a - slack, ins, mutate)
    if geo == 1:
        return joined(bio[e - a:e], rc_ref(bio[s - b:s]), True, e - a - slack, ins, mutate)
    if geo == 2:
        return joined(rc_ref(bio[s:s + b]), bio[e:e + a], False, e + a + slack, ins, mutate)
    return joined(rc_ref(bio[e:e + b]), bio[s:s + a], False, s + a + slack, ins, mutate)


def td_reads(bio, s, e, L, a, n_nt=0, **kw):
    return split_nt(bio, e - a, a, s, L, n_nt, **kw)


def host_lists(chroms, batch, prm):
    """hostlib.sv_candidates on the points of the CPU oracle"""
    from oracle import pyoracle
    from pindel_amd import hostlib
    from tests import golden_util as gu
    r = pyoracle.search_batch(pyoracle.make_params(), [s for _, s in chroms], batch.seq, batch.seq_off, batch.anchor_strand,
                              batch.anchor_pos, batch.insert_size, batch.chr_id)
    co, cp = gu.csr_from_strided(r["close_cnt"], r["close_pts"])
    fo, fp = gu.csr_from_strided(r["far_cnt"], r["far_pts"])
    return hostlib.sv_candidates(chroms, batch.seq, batch.seq_off, batch.anchor_strand, batch.chr_id, r["rc_flag"], co, cp, fo, fp,
                                 pyoracle.max_mismatch_table(), settings=prm)


def di_cases(seed=21):
    """Deletions of 400 bases with 1, 3 and 8 non-template bases at the breakpoint."""
    rng = np.random.default_rng(seed)
    a, d, b = rand_bases(rng, 3000), rand_bases(rng, 400), rand_bases(rng, 3000)
    bio = a + d + b
    reads = []
    for n_nt in (1, 3, 8):
        reads += split_nt(bio, len(a) - 45, 45, len(a) + 400, 100, n_nt)
    return [("di_nt", [("chrD", padded(bio))], as_batch(reads), None)]


def td_cases(seed=22):
    """Tandem duplications of 600 bases without and with non-template bases; 250-bp reads (more than 64 close points).  (The far
    end on a second chromosome is translocation_case of variant_cases.)"""
    rng = np.random.default_rng(seed)
    bio = rand_bases(rng, 8000)
    s, e = 3000, 3600
    reads = td_reads(bio, s, e, 100, 50) + td_reads(bio, s, e, 150, 60)
    out = [("td_plain", [("chrT", padded(bio))], as_batch(reads), None)]
    reads = td_reads(bio, s, e, 100, 45, n_nt=8) + td_reads(bio, s, e, 150, 70, n_nt=12)
    out.append(("td_nt", [("chrT", padded(bio))], as_batch(reads), None))
    reads = td_reads(bio, s, e, 250, 150) + td_reads(bio, s, e, 250, 100)
    out.append(("td_long_reads", [("chrT", padded(bio))], as_batch(reads), None))
    return out


def td_homology_cases(seed=23):
    """Microhomology: the m bases before the duplicated segment repeat at its end, so m + 1 junctions fit (m = 3: four pairs; m = 8:
    "more" is set)."""
    rng = np.random.default_rng(seed)
    out = []
    for m in (3, 8):
        bio = bytearray(rand_bases(rng, 8000))
        s, e = 3000, 3600
        bio[s - m:s] = bio[e - m:e]
        bio[s - m - 1] = ord("A") if bio[e - m - 1] != ord("A") else ord("C")        # homology of exactly m bases
        bio[e] = ord("G") if bio[s] != ord("G") else ord("T")
        bio = bytes(bio)
        reads = td_reads(bio, s, e, 100, 50) + td_reads(bio, s, e, 150, 75)
        out.append((f"td_homology{m}", [("chrM", padded(bio))], as_batch(reads), None))
    return out


def td_budget_order_cases(seed=24):
    """Ten bases of homology with one difference, two bases from the junction: the two junctions without a mismatch are listed
    first although the junctions that take the difference as a mismatch come earlier among the close points ('+') or later ('-')."""
    rng = np.random.default_rng(seed)
    bio = bytearray(rand_bases(rng, 8000))
    s, e = 3000, 3600
    bio[s - 10:s] = bio[e - 10:e]
    bio[e - 2] = ord("A") if bio[s - 2] != ord("A") else ord("C")
    bio[s - 11] = ord("A") if bio[e - 11] != ord("A") else ord("C")
    bio[e] = ord("G") if bio[s] != ord("G") else ord("T")
    bio = bytes(bio)
    reads = td_reads(bio, s, e, 100, 50) + td_reads(bio, s, e, 150, 75)
    return [("td_budget_order", [("chrO", padded(bio))], as_batch(reads), None)]


def inversion_cases(seed=25):
    """An inversion of 900 bases: the four geometries without and with non-template bases, 100 and 150 bp."""
    rng = np.random.default_rng(seed)
    bio = rand_bases(rng, 9000)
    s, e = 4000, 4900
    plain, nt = [], []
    for geo in range(4):
        plain += [inversion_read(bio, s, e, geo, 100, 50), inversion_read(bio, s, e, geo, 150, 60)]
        nt += [inversion_read(bio, s, e, geo, 100, 45, n_nt=8), inversion_read(bio, s, e, geo, 150, 70, n_nt=12)]
    chroms = [("chrV", padded(bio))]
    out = [("inv_plain", chroms, as_batch(plain), None), ("inv_nt", chroms, as_batch(nt), None)]
    long_reads = [inversion_read(bio, s, e, geo, 250, 150) for geo in range(4)]
    out.append(("inv_long_reads", chroms, as_batch(long_reads), None))
    return out


def inversion_palindrome_cases(seed=26):
    """An inverted segment whose ends are reverse complements of each other (60 bases): LeftMostINV walks through them."""
    rng = np.random.default_rng(seed)
    bio = bytearray(rand_bases(rng, 9000))
    s, e = 4000, 4900
    bio[e - 60:e] = rc_ref(bytes(bio[s:s + 60]))
    bio = bytes(bio)
    reads = [inversion_read(bio, s, e, geo, 150, 75) for geo in range(4)]
    return [("inv_palindromic_flanks", [("chrP", padded(bio))], as_batch(reads), None)]


def threshold_cases(seed=27):
    """The thresholds of the settings: breakpoint distance exactly -v and -v + 1, matched bases exactly -d and -d - 1."""
    rng = np.random.default_rng(seed)
    bio = rand_bases(rng, 9000)
    s = 4000
    out = []
    # an inversion of 300 bases with non-template bases: the last points of both lists lie exactly 300 apart, and the distance
    # must exceed -v (searchInversions itself tests the read's outermost points first, which lie closer together)
    reads = [inversion_read(bio, s, s + 300, geo, 100, 45, n_nt=8) for geo in range(4)]
    for name, v in (("inv_distance_min_plus_1", 299), ("inv_distance_min", 300)):
        out.append((name, [("chrV", padded(bio))], as_batch(reads), (0.01, 30, v)))
    # non-template bases that leave exactly 60 matched bases of 100, with -d 60 and -d 61
    nt_reads = [inversion_read(bio, s, s + 900, geo, 100, 30, n_nt=40) for geo in range(4)]
    nt_reads += td_reads(bio, s, s + 600, 100, 30, n_nt=40)
    nt_reads += split_nt(bio, s - 30, 30, s + 400, 100, 40)
    for name, d in (("matched_bases_at_d", 60), ("matched_bases_below_d", 61), ("matched_bases_above_d", 59)):
        out.append((name, [("chrV", padded(bio))], as_batch(nt_reads), (0.01, d, 50)))
    return out


def budget_cases(seed=28):
    """The NT kinds' mismatch budget (short)(1 + rate * length sum): with -e 0.02 it is 2 up to a length sum of 99 and 3 from 100
    on.  150-bp reads with 50 or 51 non-template bases (length sum 100 / 99) and two or three mismatches deep in their parts."""
    rng = np.random.default_rng(seed)
    bio = rand_bases(rng, 9000)
    s = 4000
    reads = []
    for n_nt in (50, 51):
        for mut in ((10, 20), (10, 20, 140)):
            reads += split_nt(bio, s - 50, 50, s + 400, 150, n_nt, mutate=mut)
            reads += td_reads(bio, s, s + 600, 150, 50, n_nt=n_nt, mutate=mut)
    return [("nt_budget_edge", [("chrB", padded(bio))], as_batch(reads), (0.02, 30, 50))]


def exact_kernel_cases(seed=29):
    """Reads of the exact kernel: characters outside ACGTN in front (rc_flag 1) or behind (rc_flag 2), 126 -> 125 bases."""
    from pindel_amd import synth
    ref = synth.make_reference(200_000, seed=seed)
    clean = synth.make_reads(ref, 90, seed=seed + 1, read_len=125, mix=(0.1, 0.1, 0.4, 0.4, 0.0), rc_retry_frac=0.0, n_rate=0.0)
    batch = sc.concat([sc.lead_case(clean, b"R"), sc.trail_case(sc.moved(clean), b"K"), clean])
    return [("exact_kernel", [("chrS", ref)], batch, None)]


def all_cases():
    return (di_cases() + td_cases() + td_homology_cases() + td_budget_order_cases() + inversion_cases() + inversion_palindrome_cases() +
            threshold_cases() + budget_cases() + exact_kernel_cases())


def listed(counts, kind):
    return counts[:, KIND[kind] - 2] & 0x7f


def records(cands, kind, j=0):
    from pindel_amd import hostlib
    return cands[:, hostlib.SV_SLOT[KIND[kind]] + j]


def check_case(name, batch, cands, counts):
    """What the case must show, on the expected (host) arrays."""
    plus = batch.anchor_strand == ord("+")
    more = lambda kind: (counts[:, KIND[kind] - 2] & 0x80) != 0
    if name == "di_nt":
        assert listed(counts, "DI").all(), name
        assert sorted(set(records(cands, "DI")["nt_rot"].tolist())) == [1, 3, 8]
    elif name == "td_plain":
        assert listed(counts, "TD").all() and not listed(counts, "TD_NT").any(), name
    elif name == "td_nt":
        assert listed(counts, "TD_NT").all() and sorted(set(records(cands, "TD_NT")["nt_rot"].tolist())) == [8, 12], name
    elif name == "td_long_reads":
        assert listed(counts, "TD").all(), name
        idx = np.concatenate([records(cands, "TD")["close_idx"], records(cands, "TD")["far_idx"]])
        assert idx.max() > 64, name                                         # the lane loop's second round
    elif name == "td_budget_order":
        assert (listed(counts, "TD") == 4).all(), (name, listed(counts, "TD").tolist())
        k = np.stack([records(cands, "TD", j)["close_idx"].astype(int) for j in range(4)], axis=1)
        assert (k[plus][:, 2] < k[plus][:, 0]).all() and (k[~plus][:, 2] > k[~plus][:, 0]).all(), (name, k.tolist())
    elif name.startswith("td_homology"):
        m = int(name[len("td_homology"):])
        assert (listed(counts, "TD") == 4).all(), (name, listed(counts, "TD").tolist())
        if m == 8:
            assert more("TD").all(), name                                   # nine junctions without a mismatch alone
        d = np.diff(np.stack([records(cands, "TD", j)["close_idx"].astype(int) for j in range(4)], axis=1), axis=1)
        assert (d[plus] == 1).all() and (d[~plus] == -1).all(), (name, d.tolist())     # close points ascending for '+', descending for '-'
    elif name in ("inv_plain", "inv_long_reads", "inv_palindromic_flanks"):
        assert listed(counts, "INV").all(), (name, listed(counts, "INV").tolist())
        geo = (records(cands, "INV")["flags"] >> 4) & 3
        assert sorted(set(geo.tolist())) == [0, 1, 2, 3], name
        if name == "inv_long_reads":
            assert max(records(cands, "INV")["close_idx"].max(), records(cands, "INV")["far_idx"].max()) > 64
        if name == "inv_palindromic_flanks":
            assert (listed(counts, "INV") == 4).all() and more("INV").all(), name        # every junction inside the flanks fits
    elif name == "inv_nt":
        assert listed(counts, "INV_NT").all() and not listed(counts, "INV").any(), name
        geo = (records(cands, "INV_NT")["flags"] >> 4) & 3
        assert sorted(set(geo.tolist())) == [0, 1, 2, 3] and sorted(set(records(cands, "INV_NT")["nt_rot"].tolist())) == [8, 12], name
    elif name.startswith("inv_distance"):
        want = name == "inv_distance_min_plus_1"
        assert (listed(counts, "INV_NT") > 0).all() == want and (listed(counts, "INV_NT") > 0).any() == want, (name, listed(counts, "INV_NT").tolist())
        if want:
            assert (records(cands, "INV_NT")["indel_size"] == 300).all(), name
    elif name.startswith("matched_bases"):
        # -d is inclusive for DI and INV_NT and exclusive for TD_NT
        di, td, inv = listed(counts, "DI")[6:], listed(counts, "TD_NT")[4:6], listed(counts, "INV_NT")[:4]
        want = {"matched_bases_at_d": (True, False, True), "matched_bases_below_d": (False, False, False), "matched_bases_above_d": (True, True, True)}[name]
        assert (bool(di.all()), bool(td.all()), bool(inv.all())) == want and (bool(di.any()), bool(td.any()), bool(inv.any())) == want, name
    elif name == "nt_budget_edge":
        # per block of four reads (DI +, DI -, TD_NT +, TD_NT -): 50 non-template bases, 2 / 3 mismatches; 51, 2 / 3
        got = np.where(np.arange(batch.n) % 4 < 2, listed(counts, "DI"), listed(counts, "TD_NT")).reshape(4, 4).any(axis=1)
        assert got.tolist() == [True, True, True, False], (name, got.tolist())
    elif name == "exact_kernel":
        # the parts with rc_flag 1 and 2 (90 reads each): tandem duplications in both, inversions in the first
        assert (listed(counts, "TD")[:90] > 0).sum() >= 5 and (listed(counts, "TD")[90:180] > 0).sum() >= 5, name
        assert (listed(counts, "INV")[:90] > 0).sum() >= 5, name
    else:
        raise AssertionError(f"no check for case {name}")
