"""ctypes binding of the host-side library (pindel_amd/libpindel_host.so): loaders, SV
classifiers and text reporters written in C++ (pindel_amd/csrc/host/).  No search code."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpindel_host.so")


class HostSettings(C.Structure):
    _fields_ = [
        ("spacer", C.c_uint32), ("min_support", C.c_uint32), ("balance_cutoff", C.c_uint32),
        ("seq_error_rate", C.c_double), ("min_num_matched_bases", C.c_int32),
        ("min_inversion_size", C.c_int32), ("analyze_td", C.c_int32), ("analyze_inv", C.c_int32),
        ("window_mbp", C.c_double), ("max_mismatch", C.c_uint32 * 500),
        ("analyze_li", C.c_int32), ("report_close_mapped", C.c_int32),
        ("region", C.c_char_p), ("include_bed", C.c_char_p), ("exclude_bed", C.c_char_p),
        ("report_interchromosomal", C.c_int32),
        ("normal_samples", C.c_int32), ("bam_config", C.c_char_p), ("pindel_config", C.c_char_p),
        ("repairs", C.c_uint32)]


# --repair names -> bits of HostSettings.repairs (pindel_amd/csrc/host/pg_host.hpp REPAIR_*)
REPAIRS = {"int-pairs": 1, "inv-pairs": 2, "depth-mapq": 4, "bed0": 8}
DEPTH_MAPQ_FLOOR = 20


class VcfOptions(C.Structure):
    """pgh_vcf_options: pindel2vcf's flags (pindel_amd/csrc/host/pg_vcf.hpp)"""
    _fields_ = [(n, C.c_char_p) for n in ("reference", "reference_name", "reference_date", "report", "prefix", "vcf",
                                          "chromosome")] + [
        ("window_size", C.c_int32), ("min_coverage", C.c_int32), ("het_cutoff", C.c_double), ("hom_cutoff", C.c_double)] + [
        (n, C.c_int32) for n in ("min_size", "max_size", "both_strands", "min_supporting_samples", "min_supporting_reads",
                                 "max_supporting_reads", "region_start", "region_end", "max_internal_repeats",
                                 "max_internal_repeatlength", "max_postindel_repeats", "max_postindel_repeatlength",
                                 "compact_output_limit", "only_balanced_samples", "minimum_strand_support", "gatk_compatible")]


# reports_to_vcf keyword -> (VcfOptions field, pindel2vcf flag)
VCF_FLAGS = {
    "chromosome": ("chromosome", "-c"), "window_size": ("window_size", "-w"), "min_coverage": ("min_coverage", "-mc"),
    "het_cutoff": ("het_cutoff", "-he"), "hom_cutoff": ("hom_cutoff", "-ho"), "min_size": ("min_size", "-is"),
    "max_size": ("max_size", "-as"), "both_strands_supported": ("both_strands", "-b"),
    "min_supporting_samples": ("min_supporting_samples", "-m"), "min_supporting_reads": ("min_supporting_reads", "-e"),
    "max_supporting_reads": ("max_supporting_reads", "-f"), "region_start": ("region_start", "-sr"),
    "region_end": ("region_end", "-er"), "max_internal_repeats": ("max_internal_repeats", "-ir"),
    "max_internal_repeatlength": ("max_internal_repeatlength", "-il"), "max_postindel_repeats": ("max_postindel_repeats", "-pr"),
    "max_postindel_repeatlength": ("max_postindel_repeatlength", "-pl"), "compact_output_limit": ("compact_output_limit", "-co"),
    "only_balanced_samples": ("only_balanced_samples", "-sb"), "minimum_strand_support": ("minimum_strand_support", "-ss"),
    "gatk_compatible": ("gatk_compatible", "-G"),
}


def build(force=False):
    src_dir = os.path.join(_HERE, "csrc")
    host_dir = os.path.join(src_dir, "host")
    srcs = [os.path.join(host_dir, f) for f in os.listdir(host_dir)]
    if force or not os.path.exists(LIB_PATH) or any(
            os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs):
        subprocess.check_call(["make", "-C", src_dir, "host"] + (["-B"] if force else []),
                              stdout=subprocess.DEVNULL)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(LIB_PATH)
        L.pgh_last_error.restype = C.c_char_p
        L.pgh_call_from_points.argtypes = [
            C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(HostSettings), C.c_uint32,
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.pgh_call_from_points_candidates.argtypes = L.pgh_call_from_points.argtypes + [C.c_void_p, C.c_void_p]
        L.pgh_call_from_points_lists.argtypes = L.pgh_call_from_points.argtypes + [C.c_void_p] * 4
        L.pgh_sv_candidates.argtypes = [C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32] + [C.c_void_p] * 13
        L.pgh_last_variant_fallbacks.restype = C.c_uint64
        L.pgh_last_variant_fallbacks.argtypes = []
        L.pgh_last_variant_visits.restype = C.c_uint64
        L.pgh_last_variant_visits.argtypes = [C.c_void_p, C.c_uint64]
        L.pgh_variant_candidates.argtypes = [C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32] + [C.c_void_p] * 12
        L.pgh_call_from_points_events.argtypes = L.pgh_call_from_points.argtypes + [C.c_void_p] * 4 + [C.c_int32, C.c_void_p]
        L.pgh_call_from_points_sv_events.argtypes = L.pgh_call_from_points_events.argtypes + [C.c_int32, C.c_void_p]
        L.pgh_call_from_points_report_reads.argtypes = L.pgh_call_from_points.argtypes + [C.c_void_p] * 4
        for f in ("pgh_last_event_fallback_windows", "pgh_last_event_table_windows", "pgh_last_event_supplied_windows",
                  "pgh_last_sv_event_table_windows", "pgh_last_sv_event_supplied_windows", "pgh_last_report_windows",
                  "pgh_last_report_records", "pgh_last_int_table_windows"):
            getattr(L, f).restype = C.c_uint64
            getattr(L, f).argtypes = []
        L.pgh_last_event_windows.restype = C.c_uint64
        L.pgh_last_event_windows.argtypes = [C.c_void_p, C.c_uint64]
        L.pgh_name_ids.argtypes = [C.c_uint32, C.POINTER(C.c_char_p), C.c_void_p]
        L.pgh_name_ids.restype = None
        L.pgh_region_depth.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.POINTER(C.c_double)]
        L.pgh_region_depth_mapq.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.c_uint32, C.POINTER(C.c_double)]
        L.pgh_depth_ratio_mapq.argtypes = [C.c_int32, C.POINTER(C.c_char_p), C.c_char_p, C.c_int64, C.c_int64, C.c_int64, C.c_uint32,
                                           C.POINTER(C.c_double)]
        L.pgh_region_plan_bed.restype = C.c_int64
        L.pgh_region_plan_bed.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32, C.c_void_p, C.c_uint64]
        L.pgh_parse_repairs.restype = C.c_int64
        L.pgh_parse_repairs.argtypes = [C.c_char_p]
        L.pgh_depth_ratio.argtypes = [C.c_int32, C.POINTER(C.c_char_p), C.c_char_p, C.c_int64, C.c_int64, C.c_int64,
                                      C.POINTER(C.c_double)]
        L.pgh_depth_rule_td.argtypes = [C.c_int32, C.POINTER(C.c_double)]
        L.pgh_region_plan.restype = C.c_int64
        L.pgh_region_plan.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_uint64]
        L.pgh_vcf_default_options.argtypes = [C.POINTER(VcfOptions)]
        L.pgh_reports_to_vcf.argtypes = [C.POINTER(VcfOptions)]
        _lib = L
    return _lib


def default_settings(max_mismatch) -> HostSettings:
    """Pindel 0.2.5b9 defaults of the flags the classifiers/reporters read."""
    s = HostSettings()
    s.spacer = 100000
    s.min_support = 1          # -M
    s.balance_cutoff = 100     # -B
    s.seq_error_rate = 0.01    # -e
    s.min_num_matched_bases = 30   # -d
    s.min_inversion_size = 50      # -v
    s.analyze_td = 1
    s.analyze_inv = 1
    s.window_mbp = 5.0
    s.analyze_li = 0           # -l (default false): <prefix>_LI
    s.report_close_mapped = 0  # -s (default false): <prefix>_CloseEndMapped
    s.region = None            # -c (None = ALL)
    s.include_bed = None       # -j (None = no include list)
    s.exclude_bed = None       # -J (None = no exclude list)
    s.report_interchromosomal = 0  # -I (default false): <prefix>_INT and <prefix>_INT_final
    s.normal_samples = 0       # -N (default false): the germline filter of _TD and _INV; acts with bam_config only
    s.bam_config = None        # the -i configuration the reads were derived from (None = text input)
    s.pindel_config = None     # -P (None = no list of Pindel-text files)
    s.repairs = 0              # --repair (default none): bits of REPAIRS, see repairs_mask
    for i in range(500):
        s.max_mismatch[i] = int(max_mismatch[i])
    return s


def _enc(x):
    return None if x is None else str(x).encode()


def repairs_mask(repairs):
    """--repair's argument -> the bits of HostSettings.repairs.  repairs: None (no repair), a comma-separated string
    ("int-pairs,depth-mapq", "all") or an iterable of names.  Raises ValueError for an unknown name or an empty list,
    as the command line ends with status 2 (parsed by the host library, so both agree on the names)."""
    if repairs is None:
        return 0
    text = repairs if isinstance(repairs, str) else ",".join(repairs)
    mask = lib().pgh_parse_repairs(text.encode())
    if mask < 0:
        raise ValueError((lib().pgh_last_error() or b"").decode())
    return int(mask)


def region_plan(fasta, region=None, include_bed=None, exclude_bed=None, bed_zero_based=False):
    """The records a run with -c region -j include_bed -J exclude_bed searches, in order: a list of
    (chromosome name, start, end), Pindel coordinates, both ends included (pindel_amd/csrc/host/pg_region.hpp).
    bed_zero_based (--repair bed0): the records of both BED files are 0-based and half-open, [s, e) = positions s + 1 ... e;
    by default they are taken as Pindel positions, as the reference does.
    Raises ValueError for a malformed region, an unknown chromosome, a start beyond the chromosome, an
    unreadable or malformed BED file."""
    L = lib()
    names = _fasta_names(fasta)
    cap = 64
    while True:
        out = np.zeros(3 * cap, dtype=np.uint32)
        n = L.pgh_region_plan_bed(_enc(fasta), _enc(region), _enc(include_bed), _enc(exclude_bed), int(bool(bed_zero_based)),
                                  out.ctypes.data, cap)
        if n < 0:
            raise ValueError("region plan: " + (L.pgh_last_error() or b"").decode())
        if n <= cap:
            return [(names[int(out[3 * k])], int(out[3 * k + 1]), int(out[3 * k + 2])) for k in range(n)]
        cap = int(n)


def _fasta_names(fasta):
    """the FASTA's record names in file order (the chromosome indices of the host library)"""
    out = []
    with open(fasta, "rb") as f:
        for line in f:
            if line.startswith(b">"):
                nm = line[1:].split()
                out.append(nm[0].decode() if nm else "")
    return out


def region_depth(bam, chrom, beg, end, min_mapq=0):
    """Average read depth of [beg, end) (0-based) of chromosome `chrom` in one BAM, counted as Pindel's bam2depth does
    (pindel_amd/csrc/host/pg_depth.hpp): M/=/X bases of the reads that are not unmapped, secondary, QC-fail or duplicate,
    over end - beg.  MAPQ is ignored by default, as in the reference; min_mapq=20 is what --repair depth-mapq counts with
    (records below it are left out).  0.0 when the BAM's header lacks the chromosome, NaN for an empty region."""
    L = lib()
    out = C.c_double(0.0)
    if L.pgh_region_depth_mapq(_enc(bam), _enc(chrom), int(beg), int(end), int(min_mapq), C.byref(out)):
        raise RuntimeError("pgh_region_depth: " + (L.pgh_last_error() or b"").decode())
    return out.value


def depth_ratio(bams, chrom, chrom_size, start, end, min_mapq=0):
    """Per BAM the standardised depth of the event [start, end) against its two flanks of the same length, clipped to
    [0, chrom_size): 2 * (2 * sv) / (before + after); -1.0 when before + after == 0, NaN when a flank has no length
    (getRelativeCoverageInternal).  min_mapq as for region_depth.  Returns a list of floats in the order of `bams`."""
    L = lib()
    paths = (C.c_char_p * len(bams))(*[_enc(b) for b in bams])
    out = (C.c_double * len(bams))()
    if L.pgh_depth_ratio_mapq(len(bams), paths, _enc(chrom), int(chrom_size), int(start), int(end), int(min_mapq), out):
        raise RuntimeError("pgh_depth_ratio: " + (L.pgh_last_error() or b"").decode())
    return list(out)


def depth_rule_td(ratios):
    """-N's decision on a tandem duplication from the ratios of the BAMs measured for it (IsGoodTD): True = kept."""
    arr = (C.c_double * len(ratios))(*[float(r) for r in ratios])
    return bool(lib().pgh_depth_rule_td(len(ratios), arr))


# pg_variant_cand (include/pindel_pg.h): one candidate of the deletion / short-insertion classifiers
VARIANT_CANDS = 4
VARIANT_MORE = 0x80
VARIANT_REF_END = 1
VARIANT_CAND_DTYPE = np.dtype([("bp_left", "<u4"), ("bp_right", "<u4"), ("left", "<i4"), ("right", "<i4"), ("indel_size", "<u4"),
                               ("nt_rot", "<i4"), ("bp", "<i2"), ("close_idx", "<u2"), ("far_idx", "<u2"), ("flags", "u1"),
                               ("reserved", "u1")], align=True)
assert VARIANT_CAND_DTYPE.itemsize == 32


def variant_candidates(chroms, seq, seq_off, anchor_strand, chr_id, rc_flag, close_off, close_pts, far_off, far_pts, max_mismatch,
                       spacer=100000):
    """The per-read stage of the deletion and short-insertion classifiers as candidate lists, computed on the host with the
    classifier's own loops (pgh_variant_candidates): the reference the device classifier (Engine.variant_candidates) is compared
    with.  chroms: [(name, padded bytes)] as hostio.load_fasta returns; the reads as they were handed to the search, the search's
    rc flags and its expanded points (CSR, 12-byte pg_point records); max_mismatch: g_maxMismatch (500 entries).
    Returns (cands, counts): VARIANT_CAND_DTYPE[n, 2, VARIANT_CANDS] and uint8[n, 2] (low bits: pairs listed, VARIANT_MORE: more exist)."""
    L = lib()
    n = len(seq_off) - 1
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64)
    strand = np.ascontiguousarray(anchor_strand, dtype=np.uint8)
    chr_id = np.ascontiguousarray(chr_id, dtype=np.int32)
    rc_flag = np.ascontiguousarray(rc_flag, dtype=np.uint8)
    close_off = np.ascontiguousarray(close_off, dtype=np.uint64)
    far_off = np.ascontiguousarray(far_off, dtype=np.uint64)
    close_pts = np.ascontiguousarray(close_pts)
    far_pts = np.ascontiguousarray(far_pts)
    assert close_pts.dtype.itemsize == 12 and far_pts.dtype.itemsize == 12
    mm = np.ascontiguousarray(max_mismatch, dtype=np.uint32)
    assert len(mm) >= 500 and len(strand) == n and len(chr_id) == n and len(rc_flag) == n
    bufs = [bytes(s) for _, s in chroms]
    ptrs = (C.c_char_p * len(bufs))(*bufs)
    lens = (C.c_uint64 * len(bufs))(*[len(b) for b in bufs])
    cands = np.zeros((n, 2, VARIANT_CANDS), dtype=VARIANT_CAND_DTYPE)
    counts = np.zeros((n, 2), dtype=np.uint8)
    rc = L.pgh_variant_candidates(len(bufs), ptrs, lens, int(spacer), n, seq.ctypes.data, seq_off.ctypes.data, strand.ctypes.data,
                                  chr_id.ctypes.data, rc_flag.ctypes.data, close_off.ctypes.data, close_pts.ctypes.data,
                                  far_off.ctypes.data, far_pts.ctypes.data, mm.ctypes.data, cands.ctypes.data, counts.ctypes.data)
    if rc:
        raise RuntimeError("pgh_variant_candidates: " + (L.pgh_last_error() or b"").decode())
    return cands, counts


# the five other classifiers (include/pindel_pg.h): kind -> name; SV_SLOTS records and SV_KINDS count bytes per read in
# the order DI, TD x VARIANT_CANDS, TD_NT, INV x VARIANT_CANDS, INV_NT
SV_KINDS = {2: "DI", 3: "TD", 4: "TD_NT", 5: "INV", 6: "INV_NT"}
SV_SLOTS = 3 + 2 * VARIANT_CANDS
SV_SLOT = {2: 0, 3: 1, 4: 1 + VARIANT_CANDS, 5: 2 + VARIANT_CANDS, 6: 2 + 2 * VARIANT_CANDS}
SV_LIST_LEN = {2: 1, 3: VARIANT_CANDS, 4: 1, 5: VARIANT_CANDS, 6: 1}
SV_GEO_SHIFT = 4


class SvParams(C.Structure):
    """pg_sv_params: -e, -d, -v"""
    _fields_ = [("seq_error_rate", C.c_double), ("min_num_matched_bases", C.c_int32), ("min_inversion_size", C.c_int32)]


def sv_candidates(chroms, seq, seq_off, anchor_strand, chr_id, rc_flag, close_off, close_pts, far_off, far_pts, max_mismatch,
                  settings=None, spacer=100000):
    """The per-read stage of the DI, tandem-duplication and inversion classifiers as candidate lists, computed on the host with
    plain loops around the classifiers' own pair functions (pgh_sv_candidates): the reference the device classifier
    (Engine.sv_candidates) is compared with.  Arguments as variant_candidates(); settings: None (Pindel's defaults), a (rate, -d,
    -v) tuple or anything with seq_error_rate, min_num_matched_bases and min_inversion_size (HostSettings).  Raises ValueError for
    a -v outside [0, 2^30].  Returns (cands, counts): VARIANT_CAND_DTYPE[n, SV_SLOTS] and uint8[n, 5]; kind k has its records
    from SV_SLOT[k] on and count byte k - 2."""
    L = lib()
    n = len(seq_off) - 1
    if settings is None:
        prm = SvParams(0.01, 30, 50)
    elif isinstance(settings, (tuple, list)):
        prm = SvParams(float(settings[0]), int(settings[1]), int(settings[2]))
    else:
        prm = SvParams(float(settings.seq_error_rate), int(settings.min_num_matched_bases), int(settings.min_inversion_size))
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64)
    strand = np.ascontiguousarray(anchor_strand, dtype=np.uint8)
    chr_id = np.ascontiguousarray(chr_id, dtype=np.int32)
    rc_flag = np.ascontiguousarray(rc_flag, dtype=np.uint8)
    close_off = np.ascontiguousarray(close_off, dtype=np.uint64)
    far_off = np.ascontiguousarray(far_off, dtype=np.uint64)
    close_pts = np.ascontiguousarray(close_pts)
    far_pts = np.ascontiguousarray(far_pts)
    assert close_pts.dtype.itemsize == 12 and far_pts.dtype.itemsize == 12
    mm = np.ascontiguousarray(max_mismatch, dtype=np.uint32)
    assert len(mm) >= 500 and len(strand) == n and len(chr_id) == n and len(rc_flag) == n
    bufs = [bytes(s) for _, s in chroms]
    ptrs = (C.c_char_p * len(bufs))(*bufs)
    lens = (C.c_uint64 * len(bufs))(*[len(b) for b in bufs])
    cands = np.zeros((n, SV_SLOTS), dtype=VARIANT_CAND_DTYPE)
    counts = np.zeros((n, len(SV_KINDS)), dtype=np.uint8)
    rc = L.pgh_sv_candidates(len(bufs), ptrs, lens, int(spacer), n, seq.ctypes.data, seq_off.ctypes.data, strand.ctypes.data,
                             chr_id.ctypes.data, rc_flag.ctypes.data, close_off.ctypes.data, close_pts.ctypes.data,
                             far_off.ctypes.data, far_pts.ctypes.data, mm.ctypes.data, C.addressof(prm), cands.ctypes.data, counts.ctypes.data)
    if rc:
        raise ValueError("pgh_sv_candidates: " + (L.pgh_last_error() or b"").decode())
    return cands, counts


# event tables (include/pindel_pg.h): tables 0..3 = kind 0, kind 1, TD, TD_NT
EVENT_TABLES = 4
EVENT_KINDS = (0, 1, 3, 4)
EVR_BOXED, EVR_USED, EVR_UNRESOLVED, EVR_DUPLICATE = 1, 2, 4, 8
EV_SUPPORT, EV_RANGE, EV_BALANCE, EV_REPORT = 1, 2, 4, 8
EVENT_READ_DTYPE = np.dtype([("kind", "u1"), ("slot", "u1"), ("flags", "u1"), ("unresolved_kind", "u1"), ("nt_size", "<u2"),
                             ("reserved", "<u2")], align=True)
EVENT_DTYPE = np.dtype([("bp_left", "<u4"), ("bp_right", "<u4"), ("indel_size", "<u4"), ("first", "<u4"), ("n_reads", "<u4"),
                        ("n_plus", "<u4"), ("real_start", "<u4"), ("real_end", "<u4"), ("box_head", "<u4"), ("nt_size", "<u2"),
                        ("kind", "u1"), ("flags", "u1")], align=True)
assert EVENT_READ_DTYPE.itemsize == 8 and EVENT_DTYPE.itemsize == 40


class EventWindow(C.Structure):
    """pg_event_window"""
    _fields_ = [("chr_id", C.c_int32), ("win_end", C.c_uint32), ("region_start", C.c_uint32), ("region_end", C.c_uint32),
                ("min_support", C.c_uint32), ("balance_cutoff", C.c_uint32), ("analyze_td", C.c_int32), ("analyze_inv", C.c_int32)]


class EventSizes(C.Structure):
    """pg_event_sizes"""
    _fields_ = [("members", C.c_uint64 * EVENT_TABLES), ("events", C.c_uint64 * EVENT_TABLES), ("unresolved", C.c_uint64)]


def event_window(chr_id=0, win_end=0xffffffff, region_start=0, region_end=0xffffffff, min_support=1, balance_cutoff=100,
                 analyze_td=True, analyze_inv=True):
    """A pg_event_window; the defaults are one window over everything with Pindel's -M 1 and -B 100."""
    return EventWindow(int(chr_id), int(win_end), int(region_start), int(region_end), int(min_support), int(balance_cutoff),
                       int(bool(analyze_td)), int(bool(analyze_inv)))


def event_tables(reads, members, events, sizes):
    """The three flat outputs of an events entry as a dict: reads (EVENT_READ_DTYPE[n]), members / events (lists of the four
    tables' arrays, in EVENT_KINDS order), unresolved, and the flat arrays themselves (members_flat, events_flat)."""
    nm = [int(x) for x in sizes.members]
    ne = [int(x) for x in sizes.events]
    mo = np.concatenate([[0], np.cumsum(nm)]).astype(np.int64)
    eo = np.concatenate([[0], np.cumsum(ne)]).astype(np.int64)
    members = members[:mo[-1]]
    events = events[:eo[-1]]
    return dict(reads=reads, members=[members[mo[t]:mo[t + 1]] for t in range(EVENT_TABLES)],
                events=[events[eo[t]:eo[t + 1]] for t in range(EVENT_TABLES)], unresolved=int(sizes.unresolved),
                members_flat=members, events_flat=events, n_members=nm, n_events=ne)


def name_ids(names):
    """Numbers names by first occurrence (pgh_name_ids): the name_id array of the events entries, uint32 per read."""
    L = lib()
    enc = [n if isinstance(n, bytes) else str(n).encode() for n in names]
    arr = (C.c_char_p * len(enc))(*enc)
    out = np.zeros(len(enc), dtype=np.uint32)
    L.pgh_name_ids(len(enc), arr, out.ctypes.data)
    return out


def events_from_lists(chroms, seq, seq_off, anchor_strand, chr_id, rc_flag, insert_size, close_off, close_pts, far_off, far_pts,
                      window, variant=None, sv=None, name_id=None, spacer=100000):
    """Event tables from candidate lists on the host (pgh_events_from_lists): the reference Engine.events is compared
    with, byte for byte.  Reads and points as variant_candidates() takes them, plus insert_size; window: an EventWindow; variant /
    sv: (cands, counts) pairs as the candidate entries return them, or None (empty lists); name_id: None (all names differ) or
    uint32 per read.  Returns event_tables(...).  Raises ValueError for a refused window."""
    L = lib()
    n = len(seq_off) - 1
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64)
    strand = np.ascontiguousarray(anchor_strand, dtype=np.uint8)
    chr_id = np.ascontiguousarray(chr_id, dtype=np.int32)
    rc_flag = np.ascontiguousarray(rc_flag, dtype=np.uint8)
    isz = np.ascontiguousarray(insert_size, dtype=np.int16)
    close_off = np.ascontiguousarray(close_off, dtype=np.uint64)
    far_off = np.ascontiguousarray(far_off, dtype=np.uint64)
    close_pts = np.ascontiguousarray(close_pts)
    far_pts = np.ascontiguousarray(far_pts)
    assert close_pts.dtype.itemsize == 12 and far_pts.dtype.itemsize == 12
    assert len(strand) == n and len(chr_id) == n and len(rc_flag) == n and len(isz) == n
    vc = vn = sc = sn = nid = None
    if variant is not None:
        vc = np.ascontiguousarray(variant[0], dtype=VARIANT_CAND_DTYPE)
        vn = np.ascontiguousarray(variant[1], dtype=np.uint8)
        assert vc.size == n * 2 * VARIANT_CANDS and vn.size == n * 2
    if sv is not None:
        sc = np.ascontiguousarray(sv[0], dtype=VARIANT_CAND_DTYPE)
        sn = np.ascontiguousarray(sv[1], dtype=np.uint8)
        assert sc.size == n * SV_SLOTS and sn.size == n * len(SV_KINDS)
    if name_id is not None:
        nid = np.ascontiguousarray(name_id, dtype=np.uint32)
        assert len(nid) == n
    bufs = [bytes(s) for _, s in chroms]
    ptrs = (C.c_char_p * len(bufs))(*bufs)
    lens = (C.c_uint64 * len(bufs))(*[len(b) for b in bufs])
    reads = np.zeros(n, dtype=EVENT_READ_DTYPE)
    members = np.zeros(max(n, 1), dtype=np.uint32)
    events = np.zeros(max(n, 1), dtype=EVENT_DTYPE)
    sizes = EventSizes()
    ptr = lambda a: a.ctypes.data if a is not None else None
    L.pgh_events_from_lists.argtypes = [C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32] + [C.c_void_p] * 20
    rc = L.pgh_events_from_lists(len(bufs), ptrs, lens, int(spacer), n, ptr(seq), ptr(seq_off), ptr(strand), ptr(chr_id), ptr(rc_flag),
                                 ptr(isz), ptr(close_off), ptr(close_pts), ptr(far_off), ptr(far_pts), C.addressof(window), ptr(vc), ptr(vn),
                                 ptr(sc), ptr(sn), ptr(nid), ptr(reads), ptr(members), ptr(events), C.addressof(sizes))
    if rc:
        raise ValueError("pgh_events_from_lists: " + (L.pgh_last_error() or b"").decode())
    return event_tables(reads, members, events, sizes)


# SV event tables (include/pindel_pg.h): tables 0..2 = DI, INV, INV_NT; the events are EVENT_DTYPE records
SV_EVENT_TABLES = 3
SV_EVENT_KINDS = (2, 5, 6)
EV_SHORT_INV = 0x10
SVEV_MEMBER_DUP = 0x80000000


class SvEventSizes(C.Structure):
    """pg_sv_event_sizes"""
    _fields_ = [("members", C.c_uint64 * SV_EVENT_TABLES), ("events", C.c_uint64 * SV_EVENT_TABLES),
                ("dropped_runs", C.c_uint64 * SV_EVENT_TABLES)]


def sv_event_tables(members, events, sizes):
    """The flat outputs of an sv events entry as a dict: members / events (lists of the three tables' arrays, in SV_EVENT_KINDS
    order), dropped_runs, and the flat arrays themselves (members_flat, events_flat)."""
    nm = [int(x) for x in sizes.members]
    ne = [int(x) for x in sizes.events]
    mo = np.concatenate([[0], np.cumsum(nm)]).astype(np.int64)
    eo = np.concatenate([[0], np.cumsum(ne)]).astype(np.int64)
    members = members[:mo[-1]]
    events = events[:eo[-1]]
    return dict(members=[members[mo[t]:mo[t + 1]] for t in range(SV_EVENT_TABLES)],
                events=[events[eo[t]:eo[t + 1]] for t in range(SV_EVENT_TABLES)], dropped_runs=[int(x) for x in sizes.dropped_runs],
                members_flat=members, events_flat=events, n_members=nm, n_events=ne)


def sv_events_from_lists(chroms, seq, seq_off, anchor_strand, rc_flag, close_off, close_pts, window, reads, sv, spacer=100000):
    """The event tables of DI, INV and INV_NT on the host (pgh_sv_events_from_lists): the reference Engine.sv_events
    is compared with, byte for byte -- the literal exchange sort, the literal duplicate walk and the sequential `whether` of the
    reporters.  Reads and close points as events_from_lists takes them; window: that build's EventWindow; reads: its per-read
    records (EVENT_READ_DTYPE[n]); sv: the (cands, counts) pair it was given.  Returns sv_event_tables(...)."""
    L = lib()
    n = len(seq_off) - 1
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64)
    strand = np.ascontiguousarray(anchor_strand, dtype=np.uint8)
    rc_flag = np.ascontiguousarray(rc_flag, dtype=np.uint8)
    close_off = np.ascontiguousarray(close_off, dtype=np.uint64)
    close_pts = np.ascontiguousarray(close_pts)
    recs = np.ascontiguousarray(reads, dtype=EVENT_READ_DTYPE)
    sc = np.ascontiguousarray(sv[0], dtype=VARIANT_CAND_DTYPE)
    assert close_pts.dtype.itemsize == 12
    assert len(strand) == n and len(rc_flag) == n and len(close_off) == n + 1 and len(recs) == n and sc.size == n * SV_SLOTS
    bufs = [bytes(s) for _, s in chroms]
    ptrs = (C.c_char_p * len(bufs))(*bufs)
    lens = (C.c_uint64 * len(bufs))(*[len(b) for b in bufs])
    members = np.zeros(max(n, 1), dtype=np.uint32)
    events = np.zeros(max(n, 1), dtype=EVENT_DTYPE)
    sizes = SvEventSizes()
    L.pgh_sv_events_from_lists.argtypes = [C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32] + [C.c_void_p] * 12
    rc = L.pgh_sv_events_from_lists(len(bufs), ptrs, lens, int(spacer), n, seq.ctypes.data, seq_off.ctypes.data, strand.ctypes.data,
                                    rc_flag.ctypes.data, close_off.ctypes.data, close_pts.ctypes.data, C.addressof(window),
                                    recs.ctypes.data, sc.ctypes.data, members.ctypes.data, events.ctypes.data, C.addressof(sizes))
    if rc:
        raise ValueError("pgh_sv_events_from_lists: " + (L.pgh_last_error() or b"").decode())
    return sv_event_tables(members, events, sizes)


# report records (include/pindel_pg.h): pg_report_read per table member, pg_report_summary per read
RR_DUP, RR_DI = 1, 2
RS_CLOSE, RS_FAR, RS_FAR_ANTISENSE, RS_CLOSE_LEFT, RS_CLOSE_RIGHT = 1, 2, 4, 8, 16
REPORT_READ_DTYPE = np.dtype([("read", "<u4"), ("cand", VARIANT_CAND_DTYPE), ("nt_size", "<u2"), ("table", "u1"), ("flags", "u1"),
                              ("bp0", "<i2"), ("di_bp", "<i2"), ("di_nt_rot", "<i4")], align=True)
REPORT_SUMMARY_DTYPE = np.dtype([("close_abs", "<u4"), ("close_len", "<i2"), ("far_chr", "<i2"), ("flags", "u1"), ("rc_flag", "u1"),
                                 ("reserved", "<u2")], align=True)
assert REPORT_READ_DTYPE.itemsize == 48 and REPORT_SUMMARY_DTYPE.itemsize == 12


class ReportSizes(C.Structure):
    """pg_report_sizes"""
    _fields_ = [("records", C.c_uint64), ("reads", C.c_uint64)]


def report_reads_from_lists(anchor_strand, rc_flag, close_off, close_pts, far_off, far_pts, events, sv_events, variant, sv):
    """Report records on the host (pgh_report_reads_from_lists): the reference Engine.report_reads is compared with,
    byte for byte.  Strands, rc flags and points as events_from_lists takes them; events / sv_events: the dicts of the two table
    builds (reads, members_flat, n_members); variant / sv: the (cands, counts) pairs they were given.  Returns (records, summaries):
    REPORT_READ_DTYPE per member of the seven member lists in order, REPORT_SUMMARY_DTYPE per read."""
    L = lib()
    strand = np.ascontiguousarray(anchor_strand, dtype=np.uint8)
    n = len(strand)
    rc_flag = np.ascontiguousarray(rc_flag, dtype=np.uint8)
    close_off = np.ascontiguousarray(close_off, dtype=np.uint64)
    far_off = np.ascontiguousarray(far_off, dtype=np.uint64)
    close_pts = np.ascontiguousarray(close_pts)
    far_pts = np.ascontiguousarray(far_pts)
    assert close_pts.dtype.itemsize == 12 and far_pts.dtype.itemsize == 12
    recs = np.ascontiguousarray(events["reads"], dtype=EVENT_READ_DTYPE)
    evm = np.ascontiguousarray(events["members_flat"], dtype=np.uint32)
    svm = np.ascontiguousarray(sv_events["members_flat"], dtype=np.uint32)
    ev_sizes = EventSizes()
    sv_sizes = SvEventSizes()
    for t in range(EVENT_TABLES):
        ev_sizes.members[t] = int(events["n_members"][t])
    for t in range(SV_EVENT_TABLES):
        sv_sizes.members[t] = int(sv_events["n_members"][t])
    vc = np.ascontiguousarray(variant[0], dtype=VARIANT_CAND_DTYPE)
    sc = np.ascontiguousarray(sv[0], dtype=VARIANT_CAND_DTYPE)
    sn = np.ascontiguousarray(sv[1], dtype=np.uint8)
    assert len(rc_flag) == n and len(close_off) == n + 1 and len(far_off) == n + 1 and len(recs) == n
    assert vc.size == n * 2 * VARIANT_CANDS and sc.size == n * SV_SLOTS and sn.size == n * len(SV_KINDS)
    assert evm.size == sum(ev_sizes.members) and svm.size == sum(sv_sizes.members)
    records = np.zeros(max(evm.size + svm.size, 1), dtype=REPORT_READ_DTYPE)
    summaries = np.zeros(max(n, 1), dtype=REPORT_SUMMARY_DTYPE)
    sizes = ReportSizes()
    L.pgh_report_reads_from_lists.argtypes = [C.c_uint32] + [C.c_void_p] * 17
    rc = L.pgh_report_reads_from_lists(n, strand.ctypes.data, rc_flag.ctypes.data, close_off.ctypes.data, close_pts.ctypes.data,
                                       far_off.ctypes.data, far_pts.ctypes.data, recs.ctypes.data, evm.ctypes.data, C.addressof(ev_sizes),
                                       svm.ctypes.data, C.addressof(sv_sizes), vc.ctypes.data, sc.ctypes.data, sn.ctypes.data,
                                       records.ctypes.data, summaries.ctypes.data, C.addressof(sizes))
    if rc:
        raise ValueError("pgh_report_reads_from_lists: " + (L.pgh_last_error() or b"").decode())
    return records[:int(sizes.records)], summaries[:n]


# long-insertion position tables (include/pindel_pg.h): strand 0 = '+' anchors, 1 = '-' anchors
LI_LONGER, LI_SHORTER = 1, 2
LI_POS_DTYPE = np.dtype([("pos", "<u4"), ("first", "<u4"), ("n_reads", "<u4"), ("flags", "<u4")])
assert LI_POS_DTYPE.itemsize == 16


class LiSizes(C.Structure):
    """pg_li_sizes"""
    _fields_ = [("members", C.c_uint64 * 2), ("positions", C.c_uint64 * 2)]


def li_tables(members, positions, sizes):
    """The flat outputs of a long-insertion entry as a dict: members / positions (lists of the two strands' arrays), the flat arrays
    (members_flat, positions_flat) and the sizes (n_members, n_positions)."""
    nm = [int(x) for x in sizes.members]
    npos = [int(x) for x in sizes.positions]
    mo, po = [0, nm[0], nm[0] + nm[1]], [0, npos[0], npos[0] + npos[1]]
    members, positions = members[:mo[2]], positions[:po[2]]
    return dict(members=[members[mo[s]:mo[s + 1]] for s in range(2)], positions=[positions[po[s]:po[s + 1]] for s in range(2)],
                members_flat=members, positions_flat=positions, n_members=nm, n_positions=npos)


def li_tables_from_lists(seq, seq_off, anchor_strand, chr_id, rc_flag, close_off, close_pts, far_off, reads, win_chr, lo, hi):
    """The long-insertion position tables on the host (pgh_li_tables_from_lists): the reference Engine.li is compared
    with, byte for byte.  Reads, rc flags and close points as events_from_lists takes them; far_off: the far ends' CSR offsets (only
    whether a read has one counts); reads: the events build's per-read records (EVENT_READ_DTYPE[n]); win_chr: that build's window
    chr_id; [lo, hi]: the buffered window.  Returns li_tables(...)."""
    L = lib()
    n = len(seq_off) - 1
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64)
    strand = np.ascontiguousarray(anchor_strand, dtype=np.uint8)
    chr_id = np.ascontiguousarray(chr_id, dtype=np.int32)
    rc_flag = np.ascontiguousarray(rc_flag, dtype=np.uint8)
    close_off = np.ascontiguousarray(close_off, dtype=np.uint64)
    far_off = np.ascontiguousarray(far_off, dtype=np.uint64)
    close_pts = np.ascontiguousarray(close_pts)
    recs = np.ascontiguousarray(reads, dtype=EVENT_READ_DTYPE)
    assert close_pts.dtype.itemsize == 12
    assert len(strand) == n and len(chr_id) == n and len(rc_flag) == n and len(close_off) == n + 1 and len(far_off) == n + 1 and len(recs) == n
    members = np.zeros(max(n, 1), dtype=np.uint32)
    positions = np.zeros(max(n, 1), dtype=LI_POS_DTYPE)
    sizes = LiSizes()
    L.pgh_li_tables_from_lists.argtypes = [C.c_uint32] + [C.c_void_p] * 9 + [C.c_int32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 3
    rc = L.pgh_li_tables_from_lists(n, seq.ctypes.data, seq_off.ctypes.data, strand.ctypes.data, chr_id.ctypes.data, rc_flag.ctypes.data,
                                    close_off.ctypes.data, close_pts.ctypes.data, far_off.ctypes.data, recs.ctypes.data, int(win_chr),
                                    int(lo), int(hi), members.ctypes.data, positions.ctypes.data, C.addressof(sizes))
    if rc:
        raise ValueError("pgh_li_tables_from_lists: " + (L.pgh_last_error() or b"").decode())
    return li_tables(members, positions, sizes)


def li_write_from_tables(chrom, out_prefix, seqs, anchor_strand, close_len, members, positions, n_members, n_positions, win_start,
                         win_end, max_insert_size, min_support=1, marks=(), spacer=100000):
    """Test hook (pgh_li_write_from_tables): the single consumer of the long-insertion tables on tables made by hand.  chrom: (name,
    padded sequence); seqs: the reads' sequences (bytes each); members / positions: both strands back to back, n_members /
    n_positions their sizes per strand; marks: padded positions an earlier report marked.  Appends to <out_prefix>_LI."""
    L = lib()
    n = len(seqs)
    seq = np.frombuffer(b"".join(seqs), dtype=np.uint8) if n else np.zeros(0, dtype=np.uint8)
    seq_off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    strand = np.ascontiguousarray(anchor_strand, dtype=np.uint8)
    close_len = np.ascontiguousarray(close_len, dtype=np.int16)
    members = np.ascontiguousarray(members, dtype=np.uint32)
    positions = np.ascontiguousarray(positions, dtype=LI_POS_DTYPE)
    marks = np.ascontiguousarray(marks, dtype=np.uint32)
    sizes = LiSizes()
    for s in range(2):
        sizes.members[s] = int(n_members[s])
        sizes.positions[s] = int(n_positions[s])
    assert len(strand) == n and len(close_len) == n and members.size == sum(n_members) and positions.size == sum(n_positions)
    name, padded = chrom
    padded = bytes(padded)
    L.pgh_li_write_from_tables.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64] + [C.c_uint32] * 4 + [C.c_int32, C.c_uint32] + \
        [C.c_void_p] * 8 + [C.c_uint32, C.c_char_p]
    rc = L.pgh_li_write_from_tables(name.encode(), padded, len(padded), int(spacer), int(min_support), int(win_start), int(win_end),
                                    int(max_insert_size), n, seq.ctypes.data if n else None, seq_off.ctypes.data, strand.ctypes.data if n else None,
                                    close_len.ctypes.data if n else None, members.ctypes.data if members.size else None,
                                    positions.ctypes.data if positions.size else None, C.addressof(sizes),
                                    marks.ctypes.data if marks.size else None, int(marks.size), str(out_prefix).encode())
    if rc:
        raise ValueError("pgh_li_write_from_tables: " + (L.pgh_last_error() or b"").decode())


# interchromosomal junction tables (include/pindel_pg.h): pg_int_call, pg_int_sizes
INT_ANCHOR_MINUS, INT_FAR_MINUS, INT_FALLBACK = 1, 2, 4
INT_CALL_DTYPE = np.dtype([("chr", "<i2"), ("far_chr", "<i2"), ("close_abs", "<u4"), ("far_abs", "<u4"), ("first", "<u4"), ("n_reads", "<u4"),
                           ("nt_off", "<u2"), ("nt_len", "<u2"), ("flags", "<u4"), ("reserved", "<u4")])
assert INT_CALL_DTYPE.itemsize == 32


class IntSizes(C.Structure):
    """pg_int_sizes"""
    _fields_ = [("members", C.c_uint64), ("calls", C.c_uint64)]


def chr_ranks(names):
    """The chr_rank of pg_int_window: per name its rank in string order (bytewise, as std::string compares), equal names sharing one."""
    order = sorted({n.encode() if isinstance(n, str) else bytes(n) for n in names})
    return np.array([order.index(n.encode() if isinstance(n, str) else bytes(n)) for n in names], dtype=np.int32)


def int_tables_from_lists(seq, seq_off, anchor_strand, chr_id, rc_flag, close_off, close_pts, far_off, far_pts, chr_rank):
    """The interchromosomal junction tables on the host (pgh_int_tables_from_lists): the reference Engine.int_calls is
    compared with, byte for byte.  Reads, rc flags and the expanded points of both ends as events_from_lists takes them; chr_rank:
    see chr_ranks().  Returns a dict: members (uint32 read indices), calls (INT_CALL_DTYPE)."""
    L = lib()
    n = len(seq_off) - 1
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64)
    strand = np.ascontiguousarray(anchor_strand, dtype=np.uint8)
    chr_id = np.ascontiguousarray(chr_id, dtype=np.int32)
    rc_flag = np.ascontiguousarray(rc_flag, dtype=np.uint8)
    close_off = np.ascontiguousarray(close_off, dtype=np.uint64)
    far_off = np.ascontiguousarray(far_off, dtype=np.uint64)
    close_pts = np.ascontiguousarray(close_pts)
    far_pts = np.ascontiguousarray(far_pts)
    chr_rank = np.ascontiguousarray(chr_rank, dtype=np.int32)
    assert close_pts.dtype.itemsize == 12 and far_pts.dtype.itemsize == 12
    assert len(strand) == n and len(chr_id) == n and len(rc_flag) == n and len(close_off) == n + 1 and len(far_off) == n + 1
    members = np.zeros(max(n, 1), dtype=np.uint32)
    calls = np.zeros(max(n, 1), dtype=INT_CALL_DTYPE)
    sizes = IntSizes()
    L.pgh_int_tables_from_lists.argtypes = [C.c_uint32] + [C.c_void_p] * 10 + [C.c_uint32] + [C.c_void_p] * 3
    rc = L.pgh_int_tables_from_lists(n, seq.ctypes.data, seq_off.ctypes.data, strand.ctypes.data, chr_id.ctypes.data, rc_flag.ctypes.data,
                                     close_off.ctypes.data, close_pts.ctypes.data, far_off.ctypes.data, far_pts.ctypes.data,
                                     chr_rank.ctypes.data if chr_rank.size else None, int(chr_rank.size), members.ctypes.data,
                                     calls.ctypes.data, C.addressof(sizes))
    if rc:
        raise ValueError("pgh_int_tables_from_lists: " + (L.pgh_last_error() or b"").decode())
    return dict(members=members[:int(sizes.members)], calls=calls[:int(sizes.calls)])


def int_write_from_tables(out_prefix, names, chr_names, far_names, seqs, junction, members, calls, repairs=0, spacer=100000):
    """Test hook (pgh_int_write_from_tables): the single consumer of the junction tables on tables made by hand.  Per read its name,
    chromosome name, far chromosome name and sequence (bytes) as rc_flag left it; junction: the ascending indices of the junction
    reads; members / calls: the tables; repairs: REPAIR_* bits.  Appends to <out_prefix>_INT."""
    L = lib()
    n = len(seqs)
    assert len(names) == n and len(chr_names) == n and len(far_names) == n
    seq = np.frombuffer(b"".join(seqs), dtype=np.uint8) if n else np.zeros(0, dtype=np.uint8)
    seq_off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    junction = np.ascontiguousarray(junction, dtype=np.uint32)
    members = np.ascontiguousarray(members, dtype=np.uint32)
    calls = np.ascontiguousarray(calls, dtype=INT_CALL_DTYPE)
    sizes = IntSizes(int(members.size), int(calls.size))

    def strings(v):
        return (C.c_char_p * max(n, 1))(*[s.encode() if isinstance(s, str) else bytes(s) for s in v])
    L.pgh_int_write_from_tables.argtypes = [C.c_uint32] * 3 + [C.c_void_p] * 6 + [C.c_uint32] + [C.c_void_p] * 3 + [C.c_char_p]
    a, b, c = strings(names), strings(chr_names), strings(far_names)
    rc = L.pgh_int_write_from_tables(int(spacer), int(repairs), n, C.cast(a, C.c_void_p), C.cast(b, C.c_void_p), C.cast(c, C.c_void_p),
                                     seq.ctypes.data if seq.size else None, seq_off.ctypes.data, junction.ctypes.data if junction.size else None,
                                     int(junction.size), members.ctypes.data if members.size else None,
                                     calls.ctypes.data if calls.size else None, C.addressof(sizes), str(out_prefix).encode())
    if rc:
        raise ValueError("pgh_int_write_from_tables: " + (L.pgh_last_error() or b"").decode())


# pg_dd_member, pg_dd_cand, pg_dd_sizes and the flags: one copy, the binding's (importing it loads no library)
from .binding import DD_CAND_DTYPE, DD_CONTAINED, DD_MEMBER_DTYPE, DD_TESTED, DdSizes  # noqa: E402


def _seg_arrays(seg_first, seg_strand):
    strand = np.frombuffer(seg_strand.encode() if isinstance(seg_strand, str) else bytes(seg_strand), dtype=np.uint8)
    first = np.ascontiguousarray(seg_first, dtype=np.uint32)
    assert not strand.size or first.size == strand.size + 1, "seg_first has n_seg + 1 entries"
    return first, strand


def dd_tables_from_close(seq, seq_off, anchor_strand, has, rc_flag, last_abs, last_len, seg_first, seg_strand, chr_id, chrom, mm,
                         min_bp_support=3, min_map_distance=8000):
    """The dispersed-duplication breakpoint tables on the host (pgh_dd_tables_from_close): the reference Engine.dd_tables
    is compared with, byte for byte.  The reads as handed to the search; per read whether it has a close end, its rc flag,
    UP_Close.back()'s AbsLoc (close_last) and LengthStr (close_max); the segments and parameters of pg_dd_window; chrom: the padded
    bases of chr_id (bytes), mm: g_maxMismatch (the containment test runs on the host).  Returns a dict: members (DD_MEMBER_DTYPE),
    cands (DD_CAND_DTYPE), cons (bytes)."""
    L = lib()
    n = len(seq_off) - 1
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64)
    strand = np.ascontiguousarray(anchor_strand, dtype=np.uint8)
    has = np.ascontiguousarray(has, dtype=np.uint8)
    rc_flag = np.ascontiguousarray(rc_flag, dtype=np.uint8)
    last_abs = np.ascontiguousarray(last_abs, dtype=np.uint32)
    last_len = np.ascontiguousarray(last_len, dtype=np.uint16)
    first, sstrand = _seg_arrays(seg_first, seg_strand)
    chrom = np.frombuffer(bytes(chrom), dtype=np.uint8)
    mm = np.ascontiguousarray(mm[:500], dtype=np.uint32)
    assert len(strand) == n and len(has) == n and len(rc_flag) == n and len(last_abs) == n and len(last_len) == n and mm.size == 500
    members = np.zeros(max(n, 1), dtype=DD_MEMBER_DTYPE)
    cands = np.zeros(max(n, 1), dtype=DD_CAND_DTYPE)
    cons = np.zeros(max(int(seq.size), 1), dtype=np.uint8)        # (a consensus is no longer than its longest member)
    sizes = DdSizes()
    vp = C.c_void_p
    L.pgh_dd_tables_from_close.argtypes = [C.c_uint32] + [vp] * 9 + [C.c_uint32, C.c_int32, C.c_int32, C.c_int32, vp, C.c_uint64, vp, vp, vp, vp,
                                                                     C.c_uint64, vp]
    rc = L.pgh_dd_tables_from_close(n, seq.ctypes.data if seq.size else None, seq_off.ctypes.data, strand.ctypes.data, has.ctypes.data,
                                    rc_flag.ctypes.data, last_abs.ctypes.data, last_len.ctypes.data, first.ctypes.data if first.size else None,
                                    sstrand.ctypes.data if sstrand.size else None, int(sstrand.size), int(chr_id), int(min_bp_support),
                                    int(min_map_distance), chrom.ctypes.data if chrom.size else None, int(chrom.size), mm.ctypes.data,
                                    members.ctypes.data, cands.ctypes.data, cons.ctypes.data, int(cons.size), C.addressof(sizes))
    if rc:
        raise ValueError("pgh_dd_tables_from_close: " + (L.pgh_last_error() or b"").decode())
    return dict(members=members[:int(sizes.members)], cands=cands[:int(sizes.cands)], cons=cons[:int(sizes.cons_bytes)].tobytes())


def dd_cands_from_tables(names, seqs, anchor_strand, n_seg, members, cands, cons, sample="S", spacer=100000):
    """Test hook (pgh_dd_cands_from_tables): the single consumer of the DD breakpoint tables on tables made by hand.  Per split read its
    name, bytes as ingested and anchor strand; the tables.  Returns the consumer's candidates in its order as a list of
    (seg, bio_bp, tested, contained, consensus, [(name, sample, sequence, mapped, unmapped), ...])."""
    L = lib()
    n = len(seqs)
    assert len(names) == n and len(anchor_strand) == n
    seq = np.frombuffer(b"".join(seqs), dtype=np.uint8) if n else np.zeros(0, dtype=np.uint8)
    seq_off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    strand = np.ascontiguousarray(anchor_strand, dtype=np.uint8)
    members = np.ascontiguousarray(members, dtype=DD_MEMBER_DTYPE)
    cands = np.ascontiguousarray(cands, dtype=DD_CAND_DTYPE)
    cons = np.frombuffer(bytes(cons), dtype=np.uint8)
    sizes = DdSizes(int(members.size), int(cands.size), int(cons.size))
    nm = (C.c_char_p * max(n, 1))(*[s.encode() if isinstance(s, str) else bytes(s) for s in names])
    text = C.create_string_buffer(1 << 20)
    vp = C.c_void_p
    L.pgh_dd_cands_from_tables.argtypes = [C.c_uint32, C.c_uint32, vp, C.c_char_p, vp, vp, vp, C.c_uint32, vp, vp, vp, vp, C.c_char_p, C.c_uint64]
    rc = L.pgh_dd_cands_from_tables(int(spacer), n, C.cast(nm, vp), sample.encode(), seq.ctypes.data if seq.size else None, seq_off.ctypes.data,
                                    strand.ctypes.data if n else None, int(n_seg), members.ctypes.data if members.size else None,
                                    cands.ctypes.data if cands.size else None, cons.ctypes.data if cons.size else None, C.addressof(sizes),
                                    text, 1 << 20)
    if rc:
        raise ValueError("pgh_dd_cands_from_tables: " + (L.pgh_last_error() or b"").decode())
    out = []
    for line in text.value.decode("latin-1").split("\n"):
        f = line.split("\t")
        if f[0] == "C":
            out.append((int(f[1]), int(f[2]), f[3] == "1", f[4] == "1", f[5], []))
        elif f[0] == "R":
            out[-1][5].append(tuple(f[1:6]))
    return out


def last_report_windows():
    """Windows of the last call_from_points(report_reads=True) that Caller::process_window_tables wrote from records and summaries."""
    return int(lib().pgh_last_report_windows())


def last_report_records():
    """... and the report records those windows took."""
    return int(lib().pgh_last_report_records())


def last_int_table_windows():
    """Windows of the last call_from_points(report_reads=True) with -I whose _INT lines were written by the consumer from junction
    tables built while the window's reads still had points, not from copies of the reads."""
    return int(lib().pgh_last_int_table_windows())


def last_variant_fallbacks():
    """Reads of the last call_from_points(variant_candidates=...) whose list ran out, with VARIANT_MORE set, before one of its
    pairs had made the read Used: they went through the classifier's own pair search."""
    return int(lib().pgh_last_variant_fallbacks())


def last_variant_visits():
    """Test hook: the list consultations of the last call_from_points(variant_candidates=...), a uint32[k, 7] array of (read
    index, kind, window end, region start, region end, number of boxes, box size) in no particular order."""
    L = lib()
    k = int(L.pgh_last_variant_visits(None, 0))
    out = np.zeros((max(k, 1), 7), dtype=np.uint32)
    L.pgh_last_variant_visits(out.ctypes.data, k)
    return out[:k]


def call_from_points(fasta, reads_txt, out_prefix, settings, close_off, close_pts, far_off, far_pts,
                     rc_flag, region=None, include_bed=None, exclude_bed=None, reads_config=None, normal_samples=None,
                     bam_config=None, repairs=None, variant_candidates=None, sv_candidates=None, events=None, sv_events=None,
                     report_reads=False):
    """Classify + report (_D, _SI, _TD, _INV) from per-read UP_Close / UP_Far points (CSR over
    all reads of the file, 12-byte pg_point records).  settings.analyze_li / settings.report_close_mapped
    add <out_prefix>_LI / <out_prefix>_CloseEndMapped, settings.report_interchromosomal <out_prefix>_INT and
    <out_prefix>_INT_final (reads whose far points lie on another chromosome than their anchor).  region / include_bed / exclude_bed (-c, -j, -J)
    override the settings' fields of the same names when given; by default the whole genome is searched.
    reads_config (-P): a file that lists Pindel-text files, one per line, or a list of such files; they are read in order
    before reads_txt (which may then be None), and the point arrays cover the concatenated reads in load order.  A text file
    whose name ends in .gz is read through zlib.  normal_samples (-N) with bam_config (an -i configuration): the reads are
    taken as derived from those BAMs, and _TD / _INV pass the germline filter with read depth from them; without bam_config
    -N changes nothing (text input).  Both override the settings' fields when given.  repairs (--repair; see repairs_mask):
    opt-in fixes of reference defects, replacing the settings' field when given: int-pairs, depth-mapq and bed0 as on the
    command line; inv-pairs, with normal_samples and bam_config, discovers the discordant read pairs of every window in those
    BAMs for the inversion filter.  variant_candidates: (cands, counts) as variant_candidates() or Engine.variant_candidates
    return them, for the same reads -- the deletion and short-insertion classifiers then take each read's pairs from its list
    and search only where a list runs out (last_variant_fallbacks); the reports are the same bytes.  sv_candidates: (cands,
    counts) as sv_candidates() or Engine.sv_candidates return them, made with these settings' -e, -d and -v -- the same for the
    DI, tandem-duplication and inversion classifiers; with or without variant_candidates.  events (needs both
    lists): True -- per window the event tables are built from the lists (events_from_lists' function) and deletions, short
    insertions and tandem duplications are written from them, DI and the inversions from the per-read records; a window with an
    unresolved read takes the existing path (last_event_fallback_windows); the reports are the same bytes.  Or a dict {(chromosome
    index or name, win_start, win_end): tables} of tables built elsewhere over all reads (what Engine.events returns): a window
    without an entry uses the host builder (last_event_windows lists the windows of a run).  sv_events (needs
    events): True -- DI and the inversions are written from their SV tables (sv_events_from_lists' function) instead of through
    the reporters' own quadratic sorts; the reports are the same bytes.  Or a dict {window: tables} of SV tables built elsewhere
    (what Engine.sv_events returns), used for the windows whose event tables are supplied too; tables that do not fit a window
    are replaced by the host's own (last_sv_event_table_windows).  report_reads (needs both lists, implies the
    host-built events and sv_events paths): per window the host statements build lists -> tables -> report records -> summaries,
    the window's reads are replaced by copies without points, lists and pair fields, and the reports are written from tables,
    records and summaries alone (last_report_windows, last_report_records); a window with an unresolved read takes the existing
    path (last_event_fallback_windows); the reports are the same bytes."""
    L = lib()
    tmp_cfg = None
    if reads_config is not None and not isinstance(reads_config, (str, bytes, os.PathLike)):
        with tempfile.NamedTemporaryFile("w", suffix=".pindel_config", delete=False) as f:
            f.write("".join(f"{os.path.abspath(str(x))}\n" for x in reads_config))
            tmp_cfg = reads_config = f.name
    keep = [_enc(region), _enc(include_bed), _enc(exclude_bed), _enc(reads_config), _enc(bam_config)]     # (alive until the call returns)
    if any(k is not None for k in keep) or normal_samples is not None or repairs is not None:
        settings = HostSettings.from_buffer_copy(settings)
        for field, v in zip(("region", "include_bed", "exclude_bed", "pindel_config", "bam_config"), keep):
            if v is not None:
                setattr(settings, field, v)
        if normal_samples is not None:
            settings.normal_samples = int(bool(normal_samples))
        if repairs is not None:
            settings.repairs = repairs_mask(repairs)
    close_off = np.ascontiguousarray(close_off, dtype=np.uint64)
    far_off = np.ascontiguousarray(far_off, dtype=np.uint64)
    close_pts = np.ascontiguousarray(close_pts)
    far_pts = np.ascontiguousarray(far_pts)
    rc_flag = np.ascontiguousarray(rc_flag, dtype=np.uint8)
    assert close_pts.dtype.itemsize == 12 and far_pts.dtype.itemsize == 12
    args = (str(fasta).encode(), _enc(reads_txt), str(out_prefix).encode(), C.byref(settings), len(close_off) - 1,
            close_off.ctypes.data, close_pts.ctypes.data, far_off.ctypes.data, far_pts.ctypes.data, rc_flag.ctypes.data)
    try:
        n = len(close_off) - 1
        cands = counts = sv_c = sv_n = None
        if variant_candidates is not None:
            cands = np.ascontiguousarray(variant_candidates[0], dtype=VARIANT_CAND_DTYPE)
            counts = np.ascontiguousarray(variant_candidates[1], dtype=np.uint8)
            if cands.size != n * 2 * VARIANT_CANDS or counts.size != n * 2:
                raise ValueError(f"variant_candidates: {cands.size} records and {counts.size} counts for {n} reads")
        if sv_candidates is not None:
            sv_c = np.ascontiguousarray(sv_candidates[0], dtype=VARIANT_CAND_DTYPE)
            sv_n = np.ascontiguousarray(sv_candidates[1], dtype=np.uint8)
            if sv_c.size != n * SV_SLOTS or sv_n.size != n * len(SV_KINDS):
                raise ValueError(f"sv_candidates: {sv_c.size} records and {sv_n.size} counts for {n} reads")
        if report_reads:
            if cands is None or sv_c is None:
                raise ValueError("report_reads: variant_candidates and sv_candidates are both needed")
            if isinstance(events, dict) or isinstance(sv_events, dict):
                raise ValueError("report_reads: the tables are built on the host, supplied ones are not taken")
            rc = L.pgh_call_from_points_report_reads(*args, cands.ctypes.data, counts.ctypes.data, sv_c.ctypes.data, sv_n.ctypes.data)
        elif events:
            if cands is None or sv_c is None:
                raise ValueError("events: variant_candidates and sv_candidates are both needed")
            sup, keep_ev = _supplied_events(events, fasta, n)
            if sv_events:
                sv_sup, keep_sv = _supplied_sv_events(sv_events, fasta)
                rc = L.pgh_call_from_points_sv_events(*args, cands.ctypes.data, counts.ctypes.data, sv_c.ctypes.data, sv_n.ctypes.data,
                                                      len(sup) if sup is not None else 0, sup, len(sv_sup) if sv_sup is not None else 0, sv_sup)
            else:
                rc = L.pgh_call_from_points_events(*args, cands.ctypes.data, counts.ctypes.data, sv_c.ctypes.data, sv_n.ctypes.data,
                                                   len(sup) if sup is not None else 0, sup)
        elif sv_events:
            raise ValueError("sv_events: the events path is needed (events=True or supplied tables)")
        elif variant_candidates is None and sv_candidates is None:
            rc = L.pgh_call_from_points(*args)
        elif sv_candidates is None:
            rc = L.pgh_call_from_points_candidates(*args, cands.ctypes.data, counts.ctypes.data)
        else:
            rc = L.pgh_call_from_points_lists(*args, cands.ctypes.data if cands is not None else None,
                                              counts.ctypes.data if counts is not None else None, sv_c.ctypes.data, sv_n.ctypes.data)
    finally:
        if tmp_cfg:
            os.unlink(tmp_cfg)
    if rc:
        raise RuntimeError("pgh_call_from_points: " + (L.pgh_last_error() or b"").decode())


class SuppliedEvents(C.Structure):
    """pgh_supplied_events: the tables of one window, built elsewhere over all reads of the run"""
    _fields_ = [("chr", C.c_int32), ("win_start", C.c_uint32), ("win_end", C.c_uint32), ("reserved", C.c_uint32),
                ("reads", C.c_void_p), ("members", C.c_void_p), ("events", C.c_void_p), ("sizes", EventSizes)]


def _supplied_events(events, fasta, n):
    """the events argument of call_from_points -> (array of SuppliedEvents or None, what must stay alive)"""
    if events is True or not isinstance(events, dict):
        return None, []
    names = _fasta_names(fasta)
    arr = (SuppliedEvents * len(events))()
    keep = []
    for k, ((chrom, ws, we), t) in enumerate(events.items()):
        reads = np.ascontiguousarray(t["reads"], dtype=EVENT_READ_DTYPE)
        members = np.ascontiguousarray(t["members_flat"], dtype=np.uint32)
        evs = np.ascontiguousarray(t["events_flat"], dtype=EVENT_DTYPE)
        if len(reads) != n or len(members) != sum(t["n_members"]) or len(evs) != sum(t["n_events"]):
            raise ValueError(f"events: the tables of window {(chrom, ws, we)} do not fit {n} reads and their own sizes")
        keep += [reads, members, evs]
        sz = EventSizes()
        for q in range(EVENT_TABLES):
            sz.members[q], sz.events[q] = int(t["n_members"][q]), int(t["n_events"][q])
        sz.unresolved = int(t["unresolved"])
        arr[k] = SuppliedEvents(names.index(chrom) if isinstance(chrom, str) else int(chrom), int(ws), int(we), 0, reads.ctypes.data,
                                members.ctypes.data, evs.ctypes.data, sz)
    return arr, keep


class SuppliedSvEvents(C.Structure):
    """pgh_supplied_sv_events: the SV tables of one window, built elsewhere over all reads of the run"""
    _fields_ = [("chr", C.c_int32), ("win_start", C.c_uint32), ("win_end", C.c_uint32), ("reserved", C.c_uint32),
                ("members", C.c_void_p), ("events", C.c_void_p), ("sizes", SvEventSizes)]


def _supplied_sv_events(sv_events, fasta):
    """the sv_events argument of call_from_points -> (array of SuppliedSvEvents or None, what must stay alive)"""
    if sv_events is True or not isinstance(sv_events, dict):
        return None, []
    names = _fasta_names(fasta)
    arr = (SuppliedSvEvents * len(sv_events))()
    keep = []
    for k, ((chrom, ws, we), t) in enumerate(sv_events.items()):
        members = np.ascontiguousarray(t["members_flat"], dtype=np.uint32)
        evs = np.ascontiguousarray(t["events_flat"], dtype=EVENT_DTYPE)
        if len(members) != sum(t["n_members"]) or len(evs) != sum(t["n_events"]):
            raise ValueError(f"sv_events: the tables of window {(chrom, ws, we)} do not fit their own sizes")
        keep += [members, evs]
        sz = SvEventSizes()
        for q in range(SV_EVENT_TABLES):
            sz.members[q], sz.events[q], sz.dropped_runs[q] = int(t["n_members"][q]), int(t["n_events"][q]), int(t["dropped_runs"][q])
        arr[k] = SuppliedSvEvents(names.index(chrom) if isinstance(chrom, str) else int(chrom), int(ws), int(we), 0, members.ctypes.data,
                                  evs.ctypes.data, sz)
    return arr, keep


def last_sv_event_table_windows():
    """(windows whose DI and inversion reports were written from SV tables, of them from supplied tables) of the last
    call_from_points(sv_events=...)"""
    return int(lib().pgh_last_sv_event_table_windows()), int(lib().pgh_last_sv_event_supplied_windows())


def last_event_fallback_windows():
    """Windows of the last call_from_points(events=...) that held an unresolved read and went through the existing path."""
    return int(lib().pgh_last_event_fallback_windows())


def last_event_table_windows():
    """(windows written from tables, of them from supplied tables) of the last call_from_points(events=...)"""
    return int(lib().pgh_last_event_table_windows()), int(lib().pgh_last_event_supplied_windows())


def last_event_windows():
    """The windows the last call_from_points(events=...) processed, in order: a uint32[k, 6] array of (chromosome index, win_start,
    win_end, region_start, region_end, reads) -- what the window description of Engine.events takes for each."""
    L = lib()
    k = int(L.pgh_last_event_windows(None, 0))
    out = np.zeros((max(k, 1), 6), dtype=np.uint32)
    L.pgh_last_event_windows(out.ctypes.data, k)
    return out[:k]


def vcf_cli():
    """Path of the pindel_pg2vcf command line (built by `make all`; `make vcf` builds it alone)."""
    exe = os.path.join(_HERE, "pindel_pg2vcf")
    host_dir = os.path.join(_HERE, "csrc", "host")
    srcs = [os.path.join(host_dir, f) for f in ("pindel_pg2vcf_main.cpp", "pg_vcf.cpp", "pg_vcf.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "vcf"], stdout=subprocess.DEVNULL)
    return exe


def reports_to_vcf(fasta, out_vcf, prefix=None, report=None, *, reference_name, reference_date, **flags):
    """pindel2vcf: Pindel reports -> out_vcf (pindel_amd/csrc/host/pg_vcf.hpp).  prefix reads <prefix>_D, _SI, _LI, _INV
    and _TD (-P), report one file (-p); exactly one of them.  reference_name / reference_date are -R / -d.  flags are the
    converter's other options by long name (VCF_FLAGS: window_size=1 is -w 1, gatk_compatible=True is -G, ...), with the
    reference's defaults.  Raises ValueError for an unknown flag and RuntimeError when the conversion fails."""
    L = lib()
    o = VcfOptions()
    L.pgh_vcf_default_options(C.byref(o))
    keep = {"reference": _enc(fasta), "reference_name": _enc(reference_name), "reference_date": _enc(reference_date),
            "report": _enc(report), "prefix": _enc(prefix), "vcf": _enc(out_vcf)}
    for k, v in flags.items():
        if k not in VCF_FLAGS:
            raise ValueError(f"reports_to_vcf: unknown flag {k!r}")
        field = VCF_FLAGS[k][0]
        if field == "chromosome":
            keep[field] = _enc(v)
        elif field in ("het_cutoff", "hom_cutoff"):
            setattr(o, field, float(v))
        else:
            setattr(o, field, int(v))
    for field, v in keep.items():   # (alive until the call returns)
        setattr(o, field, v)
    if L.pgh_reports_to_vcf(C.byref(o)):
        raise RuntimeError("pgh_reports_to_vcf: " + (L.pgh_last_error() or b"").decode())
    return str(out_vcf)
