"""The kernels the library can launch, the rules that pick one per launch, and a plan of inputs that reaches every one of them.

The library ships pg_search_kernel<NB, NS, Id, mode, DEF> (102 instantiations), pg_search_exact_kernel<mode> (3) and
pg_pack_kernel<PB> (5).  pg_launch_search / launch / launch_ns / launch_modes (pg_kernels.hip) pick one search kernel per
launch from the batch's longest read (NB), the candidate-id width (Id, small_ids in pg_api.cpp), the mismatch levels (NS),
the parameters (DEF) and the mode; launch_range (pg_api.cpp) adds the pack kernel when the search cannot pack in place
(pg_pack_in_place_ok) and the exact kernel behind it.  `expected_launches` is a plain mirror of those rules, checked against
the library's launch log (Engine.launch_log) by tests/test_gpu_instantiation_matrix.py; `CASES` holds one case per
(NB, NS, Id, DEF) cell and edge, and tests/test_instantiation_plan.py checks on the CPU that the plan reaches every kernel of
the code object and that every case lands where it says.
"""
from __future__ import annotations

import re
from dataclasses import dataclass, field

import numpy as np

from oracle import pyoracle

SEARCH, EXACT, PACK = 1, 2, 3                   # PgKernelKind
CLOSE, FAR, BOTH = 1, 2, 3                      # PgMode
MODE_NAMES = {CLOSE: "CLOSE", FAR: "FAR", BOTH: "BOTH"}
MAX_LEVELS = 32                                 # PG_MAX_LEVELS
SMALL_MAX_CLUSTER = 127                         # PG_SMALL_MAX_CLUSTER
SMALL_MAX_WINDOW = 1 << 24                      # PG_SMALL_MAX_WINDOW
PACK_IN_PLACE_MIN = 1                           # PG_PACK_IN_PLACE_MIN
DEF_PARAMS = dict(max_range_index=2, additional_mismatch=1, min_perfect_match=3, min_close=8, spacer=100000)   # PG_DEF_*


# ---------------------------------------------------------------- the mirror
def plane_blocks(max_len):
    """pg_plane_blocks (pg_device.h): 64-base blocks of the batch's bit-plane layout."""
    return 1 if max_len <= 64 else 2 if max_len <= 128 else 3 if max_len <= 192 else 4 if max_len <= 256 else 8


def class_blocks(max_len, small_ids):
    """search_class_blocks / pg_launch_search (pg_kernels.hip): NB of the search kernel a batch runs."""
    nb = 2 if max_len <= 128 else 4 if max_len <= 256 else 8
    if not small_ids:
        return nb
    return 1 if max_len <= 64 else nb if nb == 2 else 3 if max_len <= 192 else nb


def counter_slices(levels):
    """launch (pg_kernels.hip): NS from the batch's mismatch levels"""
    assert 1 <= levels <= MAX_LEVELS
    return 3 if levels <= 8 else 4 if levels <= 16 else 5


def levels_of(max_len, seq_error_rate=0.01, sensitivity=0.95, additional_mismatch=1, **_):
    """validate_and_measure (pg_api.cpp): the largest g_maxMismatch[l] + ADDITIONAL_MISMATCH + 1 over l <= the longest read"""
    t = pyoracle.max_mismatch_table(seq_error_rate, sensitivity)
    return int(t[:max_len + 1].max()) + max(1, additional_mismatch) + 1


def is_default(params):
    """the five parameters the default-parameter kernels hold as constants (launch_ns)"""
    p = dict(DEF_PARAMS, **{k: v for k, v in params.items() if k in DEF_PARAMS})
    p["additional_mismatch"] = max(1, p["additional_mismatch"])
    return p == DEF_PARAMS


def small_ids(max_range_index=2, max_window=0, max_cluster=0, force_wide=False):
    """small_ids (pg_api.cpp): 32-bit candidate ids"""
    return max_range_index <= 8 and max_window <= SMALL_MAX_WINDOW and max_cluster <= SMALL_MAX_CLUSTER and not force_wide


def pack_in_place_ok(mode, max_len, small, n_reads, split=False, no_pack_in_place=False, pack_in_place_min=PACK_IN_PLACE_MIN):
    """pg_pack_in_place_ok (pg_kernels.hip)"""
    if (mode == BOTH and split) or no_pack_in_place:
        return False
    return class_blocks(max_len, small) == plane_blocks(max_len) and n_reads >= pack_in_place_min


def search_rec(nb, ns, id_bits, mode, default, in_place):
    return (SEARCH, nb, ns, id_bits, mode, int(default), int(in_place))


def exact_rec(mode):
    return (EXACT, 0, 0, 0, mode, 0, 0)


def pack_rec(pb):
    return (PACK, pb, 0, 0, 0, 0, 0)


def expected_launches(max_len, levels, small, default, mode, n_reads=1, pack=True, exact=True, generic=False, split=False,
                      no_pack_in_place=False, pack_in_place_min=PACK_IN_PLACE_MIN):
    """The launch-log records of one launch_range (pg_api.cpp) over n_reads reads: the pack kernel in front where the search
    cannot pack in place (pack = the range's records are to be built), the search kernel(s), the exact kernel behind them
    (exact = the batch's exact list is not known to be empty).  Records as Engine.launch_log gives them, as plain tuples."""
    out = []
    in_place = False
    if pack:
        in_place = pack_in_place_ok(mode, max_len, small, n_reads, split, no_pack_in_place, pack_in_place_min)
        if not in_place:
            out.append(pack_rec(plane_blocks(max_len)))
    nb, ns, id_bits = class_blocks(max_len, small), counter_slices(levels), 32 if small else 64
    dflt = default and not generic and ns <= 4 and small
    if mode == BOTH and not split:
        out.append(search_rec(nb, ns, id_bits, BOTH, dflt, in_place))
    else:
        for m in (CLOSE, FAR):
            if mode & m:
                out.append(search_rec(nb, ns, id_bits, m, dflt, in_place))
    if exact:
        out.append(exact_rec(mode))
    return out


def _all_kernels():
    ks = set()
    for small in (True, False):
        for nb in ((1, 2, 3, 4, 8) if small else (2, 4, 8)):
            for ns in (3, 4, 5):
                for mode in (CLOSE, FAR, BOTH):
                    for default in ((False, True) if small and ns <= 4 else (False,)):
                        ks.add(search_rec(nb, ns, 32 if small else 64, mode, default, 0)[:6])
    ks |= {exact_rec(m)[:6] for m in (CLOSE, FAR, BOTH)}
    ks |= {pack_rec(pb)[:6] for pb in (1, 2, 3, 4, 8)}
    return frozenset(ks)


# every kernel the library ships, as (kind, blocks, ns, id_bits, mode, default): a launch record without its in-place flag
ALL_KERNELS = _all_kernels()


def kernel_of(rec):
    return tuple(rec)[:6]


def kernel_name(k):
    kind, blocks, ns, id_bits, mode, default = k
    if kind == SEARCH:
        return f"pg_search_kernel<{blocks}, {ns}, u{id_bits}, {MODE_NAMES[mode]}, {'true' if default else 'false'}>"
    if kind == EXACT:
        return f"pg_search_exact_kernel<{MODE_NAMES[mode]}>"
    return f"pg_pack_kernel<{blocks}>"


def kernel_from_symbol(sym):
    """a mangled kernel name of the code object -> the kernel key (None: not a search / exact / pack kernel)"""
    m = re.match(r"_Z16pg_search_kernelILi(\d+)ELi(\d+)E([jy])Li(\d)ELb([01])E", sym)
    if m:
        return (SEARCH, int(m[1]), int(m[2]), 32 if m[3] == "j" else 64, int(m[4]), int(m[5]))
    m = re.match(r"_Z22pg_search_exact_kernelILi(\d)E", sym)
    if m:
        return exact_rec(int(m[1]))[:6]
    m = re.match(r"_Z14pg_pack_kernelILi(\d+)E", sym)
    if m:
        return pack_rec(int(m[1]))[:6]
    return None


# ---------------------------------------------------------------- the plan
# Paths of the GPU matrix: (a) search_batch, (b) upload + scribble + pack_search_device (PG_PACK_IN_PLACE_MIN=1),
# (c) PG_NO_PACK_IN_PLACE=1 + repack + search_device, (d) close_end_batch, (e) far_end_batch_from_close fed from (d),
# (f) PG_SPLIT_LAUNCH=1 + search_batch.  Windows: only the device-resident paths and the far end take the case's windows.
PATHS = ("a", "b", "c", "d", "e", "f")
PATH_WINDOWS = {"a": False, "b": True, "c": True, "d": False, "e": True, "f": False}

# levels a case's longest read must land on: the bottom and the top of each NS range (NS = 3: "8 or fewer" -- 7, so that a point
# can still set the top slice)
LEVEL_TARGET = {(3, "low"): 7, (3, "high"): 8, (4, "low"): 9, (4, "high"): 16, (5, "low"): 17, (5, "high"): 32}
# the counter's top slice: a point with at least this many mismatches sets it
TOP_SLICE = {3: 4, 4: 8, 5: 16}
# longest read of a case: the first and the last length of its kernel's block class
LONGEST = {(32, 1): (36, 64), (32, 2): (65, 128), (32, 3): (129, 192), (32, 4): (193, 256), (32, 8): (257, 499),
           (64, 2): (36, 128), (64, 4): (129, 256), (64, 8): (257, 499)}

# (-e, -E, -a) per (longest read, target levels): -a 1 wherever the table reaches the target (pyoracle.max_mismatch_table); 17
# levels at 36 bases and 32 at 64 need -a on top of the highest -e (only the generic family has NS = 5)
RATES = {
    (36, 7): (0.04, 0.95, 1), (36, 8): (0.0575, 0.95, 1), (36, 9): (0.075, 0.95, 1), (36, 16): (0.145, 0.999, 1),
    (36, 17): (0.15, 0.95, 6),
    (64, 8): (0.0325, 0.95, 1), (64, 9): (0.0425, 0.95, 1), (64, 16): (0.125, 0.95, 1),
    (64, 17): (0.1375, 0.95, 1), (64, 32): (0.15, 0.999, 11),
    (65, 7): (0.0225, 0.95, 1), (65, 8): (0.03, 0.95, 1), (65, 9): (0.04, 0.95, 1), (65, 16): (0.1225, 0.95, 1),
    (65, 17): (0.135, 0.95, 1),
    (128, 8): (0.015, 0.95, 1), (128, 9): (0.02, 0.95, 1), (128, 16): (0.0625, 0.95, 1),
    (128, 17): (0.0675, 0.95, 1), (128, 32): (0.1475, 0.99, 1),
    (129, 7): (0.01, 0.95, 1), (129, 8): (0.015, 0.95, 1), (129, 9): (0.02, 0.95, 1), (129, 16): (0.06, 0.95, 1),
    (129, 17): (0.0675, 0.95, 1), (129, 32): (0.145, 0.99, 1),
    (192, 8): (0.01, 0.95, 1), (192, 9): (0.015, 0.95, 1), (192, 16): (0.04, 0.95, 1),
    (192, 17): (0.045, 0.95, 1), (192, 32): (0.11, 0.95, 1),
    (193, 7): (0.0075, 0.95, 1), (193, 8): (0.01, 0.95, 1), (193, 9): (0.015, 0.95, 1), (193, 16): (0.04, 0.95, 1),
    (193, 17): (0.045, 0.95, 1), (193, 32): (0.11, 0.95, 1),
    (256, 8): (0.0075, 0.95, 1), (256, 9): (0.01, 0.95, 1), (256, 16): (0.03, 0.95, 1),
    (256, 17): (0.0325, 0.95, 1), (256, 32): (0.0825, 0.95, 1),
    (257, 7): (0.005, 0.95, 1), (257, 8): (0.0075, 0.95, 1), (257, 9): (0.01, 0.95, 1), (257, 16): (0.03, 0.95, 1),
    (257, 17): (0.0325, 0.95, 1), (257, 32): (0.0825, 0.95, 1),
    (499, 8): (0.0025, 0.99, 1), (499, 9): (0.005, 0.95, 1), (499, 16): (0.015, 0.95, 1),
    (499, 17): (0.0175, 0.95, 1), (499, 32): (0.0425, 0.95, 1),
}


@dataclass(frozen=True)
class Case:
    id: str
    nb: int                     # the search kernel's blocks (NB)
    id_bits: int                # 32 / 64
    ns: int
    default: bool               # the default-parameter family (DEF)
    edge: str                   # "low" / "high"
    longest: int                # the batch's longest read
    levels: int                 # what validate_and_measure must find
    params: dict = field(default_factory=dict)          # Engine / oracle keyword arguments
    generic_switch: bool = False                        # PG_GENERIC_KERNELS=1 (else a parameter off the defaults makes it generic)
    wide: str = ""              # how the 64-bit ids come: "force" (PG_FORCE_WIDE_CELLS) / "windows" (clusters of `windows`)
    windows: int = 0            # windows per read (0: none)
    n_reads: int = 480
    seed: int = 0

    @property
    def lengths(self):
        """the longest read, and shorter ones with length = 0, 1 and 63 (mod 64) where those are long enough to split"""
        L = self.longest
        short = {L - ((L - r) % 64 or 64) for r in (0, 1, 63)}
        return [L] + sorted(x for x in short if 24 <= x < L)

    @property
    def junk(self):
        """reads with characters outside ACGTN (the exact kernel runs beside the main one)"""
        return self.longest >= 100

    def small_ids_on(self, path):
        return small_ids(self.params.get("max_range_index", 2), 0, self.windows if PATH_WINDOWS[path] else 0,
                         force_wide=self.wide == "force")

    def switches(self, path):
        """PG_* switches of the path (the environment of the launch)"""
        env = {}
        if self.generic_switch:
            env["PG_GENERIC_KERNELS"] = "1"
        if self.wide == "force":
            env["PG_FORCE_WIDE_CELLS"] = "1"
        if path == "b":
            env["PG_PACK_IN_PLACE_MIN"] = "1"
        if path == "c":
            env["PG_NO_PACK_IN_PLACE"] = "1"
        if path == "f":
            env["PG_SPLIT_LAUNCH"] = "1"
        return env

    def expected(self, path, n_reads):
        """the distinct launch records of one path over the case's batch of n_reads reads"""
        kw = dict(max_len=self.longest, levels=self.levels, small=self.small_ids_on(path), default=is_default(self.params),
                  n_reads=n_reads, generic=self.generic_switch)
        if path in ("a", "b"):
            recs = expected_launches(mode=BOTH, **kw)
        elif path == "c":
            # repack (a pack launch of its own), then a search that does not pack; the exact kernel only for a non-empty list
            recs = [pack_rec(plane_blocks(self.longest))] + expected_launches(mode=BOTH, pack=False, exact=self.junk,
                                                                             no_pack_in_place=True, **kw)
        elif path == "d":
            recs = expected_launches(mode=CLOSE, **kw)
        elif path == "e":
            recs = expected_launches(mode=FAR, **kw)
        else:
            recs = expected_launches(mode=BOTH, split=True, **kw)
        return set(recs)


def _make_cases():
    cases = []
    seed = 1000
    cells = [(32, nb, ns, d) for nb in (1, 2, 3, 4, 8) for ns in (3, 4, 5) for d in ((True, False) if ns <= 4 else (False,))]
    cells += [(64, nb, ns, False) for nb in (2, 4, 8) for ns in (3, 4, 5)]
    for k, (id_bits, nb, ns, default) in enumerate(cells):
        for edge in ("low", "high"):
            L = LONGEST[(id_bits, nb)][edge == "high"]
            lv = LEVEL_TARGET[(ns, edge)]
            e, s, a = RATES[(L, lv)]
            params = dict(seq_error_rate=e, sensitivity=s)
            generic_switch = False
            if a != 1:
                params["additional_mismatch"] = a
            elif not default and ns <= 4 and id_bits == 32:
                # the generic family on a parameter off the defaults (low), or on the defaults with PG_GENERIC_KERNELS (high)
                if edge == "low":
                    params.update([dict(min_perfect_match=4), dict(min_close=9), dict(max_range_index=3)][k % 3])
                else:
                    generic_switch = True
            wide, windows = "", 0
            if id_bits == 64:
                # the real way -- clusters of 128 windows -- for NS = 3 at the top of each class; PG_FORCE_WIDE_CELLS elsewhere
                wide, windows = ("windows", 128) if ns == 3 and edge == "high" else ("force", 0)
            seed += 17
            cid = f"{'u32' if id_bits == 32 else 'u64'}-nb{nb}-ns{ns}-{'def' if default else 'gen'}-{edge}-L{L}"
            cases.append(Case(cid, nb, id_bits, ns, default, edge, L, lv, params, generic_switch, wide, windows, seed=seed))
    # twins of the window cases: exactly 127 windows per read stay on 32-bit ids (on the default parameters: DEF)
    for c in [c for c in cases if c.wide == "windows"]:
        cases.append(Case(c.id.replace("u64", "u32").replace("-gen-", "-def-") + "-127win", class_blocks(c.longest, True), 32, c.ns,
                          True, c.edge, c.longest, c.levels, c.params, False, "", 127, c.n_reads, c.seed + 1))
    return cases


CASES = _make_cases()


def top_slice_needed(case):
    """the mismatch count whose points set the counter's top slice, where the parameters admit such a point at the longest
    read (None where they do not: 9 levels admit 7 mismatches at -a 1, 17 levels 15 -- the bottom of NS = 4 and NS = 5 has
    its top slice set by candidates the filter then drops, never by a point)"""
    t = pyoracle.max_mismatch_table(case.params.get("seq_error_rate", 0.01), case.params.get("sensitivity", 0.95))
    return TOP_SLICE[case.ns] if TOP_SLICE[case.ns] <= int(t[case.longest]) else None


# The largest mismatch count of a point in UP_Close and in UP_Far that each case's inputs reach (the oracle, on build_batch's
# seeded reads).  The parameters admit g_maxMismatch[longest read] (one or two more for the longest reads); a point that long
# is almost the whole read, and the split reads here place their breakpoint at 20-80 % of the read, so the counts admitted
# at the longest read itself are out of their reach.  The GPU matrix asserts the oracle still reaches these.
MM_REACH = {
    "u32-nb1-ns3-def-low-L36": 4,
    "u32-nb1-ns3-def-high-L64": 5,
    "u32-nb1-ns3-gen-low-L36": 4,
    "u32-nb1-ns3-gen-high-L64": 5,
    "u32-nb1-ns4-def-low-L36": 6,
    "u32-nb1-ns4-def-high-L64": 13,
    "u32-nb1-ns4-gen-low-L36": 5,
    "u32-nb1-ns4-gen-high-L64": 12,
    "u32-nb1-ns5-gen-low-L36": 9,
    "u32-nb1-ns5-gen-high-L64": 18,
    "u32-nb2-ns3-def-low-L65": 4,
    "u32-nb2-ns3-def-high-L128": 5,
    "u32-nb2-ns3-gen-low-L65": 4,
    "u32-nb2-ns3-gen-high-L128": 5,
    "u32-nb2-ns4-def-low-L65": 6,
    "u32-nb2-ns4-def-high-L128": 13,
    "u32-nb2-ns4-gen-low-L65": 6,
    "u32-nb2-ns4-gen-high-L128": 12,
    "u32-nb2-ns5-gen-low-L65": 13,
    "u32-nb2-ns5-gen-high-L128": 25,
    "u32-nb3-ns3-def-low-L129": 4,
    "u32-nb3-ns3-def-high-L192": 5,
    "u32-nb3-ns3-gen-low-L129": 4,
    "u32-nb3-ns3-gen-high-L192": 5,
    "u32-nb3-ns4-def-low-L129": 6,
    "u32-nb3-ns4-def-high-L192": 12,
    "u32-nb3-ns4-gen-low-L129": 6,
    "u32-nb3-ns4-gen-high-L192": 12,
    "u32-nb3-ns5-gen-low-L129": 13,
    "u32-nb3-ns5-gen-high-L192": 27,
    "u32-nb4-ns3-def-low-L193": 4,
    "u32-nb4-ns3-def-high-L256": 5,
    "u32-nb4-ns3-gen-low-L193": 5,
    "u32-nb4-ns3-gen-high-L256": 5,
    "u32-nb4-ns4-def-low-L193": 6,
    "u32-nb4-ns4-def-high-L256": 12,
    "u32-nb4-ns4-gen-low-L193": 6,
    "u32-nb4-ns4-gen-high-L256": 12,
    "u32-nb4-ns5-gen-low-L193": 13,
    "u32-nb4-ns5-gen-high-L256": 26,
    "u32-nb8-ns3-def-low-L257": 4,
    "u32-nb8-ns3-def-high-L499": 5,
    "u32-nb8-ns3-gen-low-L257": 4,
    "u32-nb8-ns3-gen-high-L499": 5,
    "u32-nb8-ns4-def-low-L257": 7,
    "u32-nb8-ns4-def-high-L499": 13,
    "u32-nb8-ns4-gen-low-L257": 6,
    "u32-nb8-ns4-gen-high-L499": 12,
    "u32-nb8-ns5-gen-low-L257": 13,
    "u32-nb8-ns5-gen-high-L499": 27,
    "u64-nb2-ns3-gen-low-L36": 4,
    "u64-nb2-ns3-gen-high-L128": 5,
    "u64-nb2-ns4-gen-low-L36": 6,
    "u64-nb2-ns4-gen-high-L128": 13,
    "u64-nb2-ns5-gen-low-L36": 8,
    "u64-nb2-ns5-gen-high-L128": 27,
    "u64-nb4-ns3-gen-low-L129": 4,
    "u64-nb4-ns3-gen-high-L256": 5,
    "u64-nb4-ns4-gen-low-L129": 6,
    "u64-nb4-ns4-gen-high-L256": 12,
    "u64-nb4-ns5-gen-low-L129": 12,
    "u64-nb4-ns5-gen-high-L256": 24,
    "u64-nb8-ns3-gen-low-L257": 4,
    "u64-nb8-ns3-gen-high-L499": 5,
    "u64-nb8-ns4-gen-low-L257": 6,
    "u64-nb8-ns4-gen-high-L499": 12,
    "u64-nb8-ns5-gen-low-L257": 12,
    "u64-nb8-ns5-gen-high-L499": 27,
    "u32-nb2-ns3-def-high-L128-127win": 5,
    "u32-nb4-ns3-def-high-L256-127win": 6,
    "u32-nb8-ns3-def-high-L499-127win": 5,
}


def case_launches(case, n_reads):
    """path -> the distinct launch records the case expects there"""
    return {p: case.expected(p, n_reads) for p in PATHS}


# ---------------------------------------------------------------- inputs
def reference():
    from pindel_amd import synth
    return [("chrM", synth.make_reference(900_000, seed=881))]


def build_batch(case, ref_seq):
    """(batch, bd, bd_off): split reads at the case's lengths -- four error rates up to the table's limit, so that points carry
    mismatch counts up to what the parameters admit -- plus reads with characters outside ACGTN where the case has them."""
    from pindel_amd import synth
    from tests import shortening_cases as sc
    lens = case.lengths
    t = pyoracle.max_mismatch_table(case.params.get("seq_error_rate", 0.01), case.params.get("sensitivity", 0.95))
    top = int(t[case.longest])
    seqs, strand, pos, isz = [], [], [], []
    tiers = (0.35, 0.8, 1.25, 1.6)
    for j, frac in enumerate(tiers):
        rate = min(0.3, frac * max(top, 1) / case.longest)
        b = synth.make_reads(ref_seq, case.n_reads // len(tiers), seed=case.seed * 7 + j, read_lens=[lens[0]] * len(lens) + lens,
                             error_rate=rate, n_rate=0.002, mix=(0.45, 0.2, 0.15, 0.1, 0.1))
        seqs += sc.seqs_of(b)
        strand += list(b.anchor_strand)
        pos += list(b.anchor_pos)
        isz += list(b.insert_size)
    if case.junk:
        clean = sc.clean_reads(ref_seq, 12, case.longest - 2, seed=case.seed + 3)
        for jb in (sc.lead_case(clean.slice(0, 6), b"RY"), sc.inner_case(clean.slice(6, 12), case.longest // 2)):
            seqs += sc.seqs_of(jb)
            strand += list(jb.anchor_strand)
            pos += list(jb.anchor_pos)
            isz += list(jb.insert_size)
    batch = sc.batch_of(seqs, strand, pos, isz)
    if not case.windows:
        return batch, None, None
    return batch, *windows_for(batch, case.windows, len(ref_seq), case.seed)


def windows_for(batch, per, ref_len, seed):
    """`per` BreakDancer windows per read: the first around the read's own far-end neighbourhood, the rest scattered"""
    from pindel_amd import binding
    from pindel_amd.hostio import SPACER
    rng = np.random.default_rng(seed)
    biol = ref_len - 2 * SPACER
    bd = np.zeros(batch.n * per, dtype=binding.WINDOW_DTYPE)
    st = rng.integers(1000, biol - 2000, len(bd))
    bd["start"] = st
    bd["end"] = st + rng.integers(50, 400, len(bd))
    ap = batch.anchor_pos.astype(np.int64)
    bd["start"][::per] = np.clip(ap - 12000, 0, biol - 24000)
    bd["end"][::per] = bd["start"][::per] + 24000
    return bd, (np.arange(batch.n + 1) * per).astype(np.uint64)
