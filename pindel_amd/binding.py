"""ctypes binding of the C ABI in include/pindel_pg.h (pindel_amd/libpindel_pg.so).

This is glue only: every computation happens in the HIP library.  If the library
is missing or no MI355X is visible the calls raise -- there is no Python or CPU
implementation of the search behind this module.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from collections import namedtuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PG_LIBRARY") or os.path.join(_HERE, "libpindel_pg.so")      # (PG_LIBRARY: an experiment build, scripts/build_variant.sh)

PG_OK = 0
PG_E_DEVICE = -3


class PgError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__(f"pindel_pg error {code}: {msg}")
        self.code = code


class PgParams(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("device", C.c_int32), ("max_range_index", C.c_int32),
        ("additional_mismatch", C.c_int32), ("min_perfect_match_around_bp", C.c_int32),
        ("min_close", C.c_int32), ("max_allowed_mismatch_rate", C.c_double),
        ("seq_error_rate", C.c_double), ("sensitivity", C.c_double),
        ("spacer", C.c_uint32), ("reserved", C.c_uint32)]


class PgReadBatch(C.Structure):
    _fields_ = [
        ("n_reads", C.c_uint32), ("seq", C.c_void_p), ("seq_off", C.c_void_p),
        ("anchor_strand", C.c_void_p), ("anchor_pos", C.c_void_p),
        ("insert_size", C.c_void_p), ("chr_id", C.c_void_p)]


class PgWindows(C.Structure):
    _fields_ = [("offset", C.c_void_p), ("windows", C.c_void_p)]


class PgHintTable(C.Structure):
    _fields_ = [("n_runs", C.c_uint32), ("run_first", C.c_void_p), ("run_cluster", C.c_void_p),
                ("n_clusters", C.c_uint32), ("cluster_off", C.c_void_p), ("windows", C.c_void_p)]


class PgDeviceResult(C.Structure):
    _fields_ = [
        ("close_off", C.c_void_p), ("close_runs", C.c_void_p), ("close_cap", C.c_uint64),
        ("far_off", C.c_void_p), ("far_runs", C.c_void_p), ("far_cap", C.c_uint64),
        ("rc_flag", C.c_void_p), ("close_last", C.c_void_p), ("close_max", C.c_void_p)]


class PgResultView(C.Structure):
    _fields_ = [
        ("n_reads", C.c_uint32), ("close_off", C.POINTER(C.c_uint64)), ("close_runs", C.c_void_p),
        ("far_off", C.POINTER(C.c_uint64)), ("far_runs", C.c_void_p),
        ("rc_flag", C.POINTER(C.c_uint8))]


RUN_DTYPE = np.dtype([("abs_loc_first", "<u4"), ("len_first", "<u2"), ("len_last", "<u2"),
                      ("mismatches", "u1"), ("flags", "u1"), ("chr_id", "<i2")], align=True)
POINT_DTYPE = np.dtype([("abs_loc", "<u4"), ("length", "<i2"), ("mismatches", "<i2"),
                        ("chr_id", "<i2"), ("direction", "S1"), ("strand", "S1")], align=True)
WINDOW_DTYPE = np.dtype([("chr_id", "<i4"), ("start", "<i4"), ("end", "<i4")], align=True)
assert RUN_DTYPE.itemsize == 12 and POINT_DTYPE.itemsize == 12 and WINDOW_DTYPE.itemsize == 12
# pg_variant_cand: one candidate of the device classifier (Engine.variant_candidates); PG_VARIANT_CANDS per read and kind
VARIANT_CANDS = 4
VARIANT_MORE = 0x80
VARIANT_REF_END = 1
VARIANT_CAND_DTYPE = np.dtype([("bp_left", "<u4"), ("bp_right", "<u4"), ("left", "<i4"), ("right", "<i4"), ("indel_size", "<u4"),
                               ("nt_rot", "<i4"), ("bp", "<i2"), ("close_idx", "<u2"), ("far_idx", "<u2"), ("flags", "u1"),
                               ("reserved", "u1")], align=True)
assert VARIANT_CAND_DTYPE.itemsize == 32
# the five other classifiers (Engine.sv_candidates): kinds PG_SV_*, SV_KINDS count bytes and SV_SLOTS records per read --
# DI, TD x VARIANT_CANDS, TD_NT, INV x VARIANT_CANDS, INV_NT; SV_SLOT[kind] = the kind's first record, SV_COUNT[kind] its count byte
SV_DI, SV_TD, SV_TD_NT, SV_INV, SV_INV_NT = 2, 3, 4, 5, 6
SV_KINDS = 5
SV_SLOTS = 3 + 2 * VARIANT_CANDS
SV_SLOT = {SV_DI: 0, SV_TD: 1, SV_TD_NT: 1 + VARIANT_CANDS, SV_INV: 2 + VARIANT_CANDS, SV_INV_NT: 2 + 2 * VARIANT_CANDS}
SV_COUNT = {k: k - SV_DI for k in SV_SLOT}
SV_GEO_SHIFT = 4                        # flags bits 4-5: the inversion geometry of SV_INV / SV_INV_NT records
SV_MAX_INVERSION_SIZE = 1 << 30


class SvParams(C.Structure):
    """pg_sv_params: the settings the five classifiers read (-e, -d, -v)"""
    _fields_ = [("seq_error_rate", C.c_double), ("min_num_matched_bases", C.c_int32), ("min_inversion_size", C.c_int32)]


def sv_params(settings=None):
    """A pg_sv_params from None (Pindel's defaults), a (rate, -d, -v) tuple, an SvParams, or anything with the attributes
    seq_error_rate, min_num_matched_bases and min_inversion_size (hostlib.HostSettings)."""
    if settings is None:
        return SvParams(0.01, 30, 50)
    if isinstance(settings, SvParams):
        return settings
    if isinstance(settings, (tuple, list)):
        return SvParams(float(settings[0]), int(settings[1]), int(settings[2]))
    return SvParams(float(settings.seq_error_rate), int(settings.min_num_matched_bases), int(settings.min_inversion_size))

# event tables (Engine.events): pg_event_window, pg_event_read, pg_event, pg_event_sizes; tables 0..3 = the kinds
# EVENT_KINDS (deletions, short insertions, TD, TD_NT)
EVENT_TABLES = 4
EVENT_KINDS = (0, 1, SV_TD, SV_TD_NT)
EVR_BOXED, EVR_USED, EVR_UNRESOLVED, EVR_DUPLICATE = 1, 2, 4, 8
EV_SUPPORT, EV_RANGE, EV_BALANCE, EV_REPORT = 1, 2, 4, 8
KERNEL_EVENT_CASCADE, KERNEL_EVENT_SORT, KERNEL_EVENT_TABLES = 6, 7, 8      # launch-log ids after 4 (variant) and 5 (sv)
EVENT_BLOCK = 256                       # PG_EV_BLOCK: the scan / sort block of the events kernels
EVENT_READ_DTYPE = np.dtype([("kind", "u1"), ("slot", "u1"), ("flags", "u1"), ("unresolved_kind", "u1"), ("nt_size", "<u2"),
                             ("reserved", "<u2")], align=True)
EVENT_DTYPE = np.dtype([("bp_left", "<u4"), ("bp_right", "<u4"), ("indel_size", "<u4"), ("first", "<u4"), ("n_reads", "<u4"),
                        ("n_plus", "<u4"), ("real_start", "<u4"), ("real_end", "<u4"), ("box_head", "<u4"), ("nt_size", "<u2"),
                        ("kind", "u1"), ("flags", "u1")], align=True)
assert EVENT_READ_DTYPE.itemsize == 8 and EVENT_DTYPE.itemsize == 40
# SV event tables (Engine.sv_events): tables 0..2 = DI, INV, INV_NT; the events are EVENT_DTYPE records
SV_EVENT_TABLES = 3
SV_EVENT_KINDS = (SV_DI, SV_INV, SV_INV_NT)
EV_SHORT_INV = 0x10                     # PG_EV_SHORT_INV: a DI event the reporter writes as a short inversion
SVEV_MEMBER_DUP = 0x80000000            # PG_SVEV_MEMBER_DUP: bit 31 of an inversion member word
KERNEL_SV_EVENTS = 9                    # launch-log id after the three of the events build
SVEV_LDS_BOX = 640                      # PG_SVEV_LDS_BOX: reads of a box the order kernel keeps in LDS


# report records (Engine.report_reads): pg_report_read per member of the seven member lists (tables 0..3 of the
# events build, then SV tables 0..2), pg_report_summary per read
REPORT_TABLES = EVENT_TABLES + SV_EVENT_TABLES
RR_DUP, RR_DI = 1, 2
RS_CLOSE, RS_FAR, RS_FAR_ANTISENSE, RS_CLOSE_LEFT, RS_CLOSE_RIGHT = 1, 2, 4, 8, 16
KERNEL_REPORT = 10                      # launch-log id of the report kernels (blocks 0: the list cut of classify)
REPORT_READ_DTYPE = np.dtype([("read", "<u4"), ("cand", VARIANT_CAND_DTYPE), ("nt_size", "<u2"), ("table", "u1"), ("flags", "u1"),
                              ("bp0", "<i2"), ("di_bp", "<i2"), ("di_nt_rot", "<i4")], align=True)
REPORT_SUMMARY_DTYPE = np.dtype([("close_abs", "<u4"), ("close_len", "<i2"), ("far_chr", "<i2"), ("flags", "u1"), ("rc_flag", "u1"),
                                 ("reserved", "<u2")], align=True)
assert REPORT_READ_DTYPE.itemsize == 48 and REPORT_SUMMARY_DTYPE.itemsize == 12


class ReportSizes(C.Structure):
    """pg_report_sizes"""
    _fields_ = [("records", C.c_uint64), ("reads", C.c_uint64)]


# long-insertion position tables (Engine.li): pg_li_window, pg_li_pos, pg_li_sizes; strand 0 = '+' anchors, 1 = '-'
LI_LONGER, LI_SHORTER = 1, 2
KERNEL_LI = 11                          # launch-log id of the long-insertion kernels
LI_POS_DTYPE = np.dtype([("pos", "<u4"), ("first", "<u4"), ("n_reads", "<u4"), ("flags", "<u4")])
assert LI_POS_DTYPE.itemsize == 16


class LiWindow(C.Structure):
    """pg_li_window"""
    _fields_ = [("lo", C.c_uint32), ("hi", C.c_uint32)]


class LiSizes(C.Structure):
    """pg_li_sizes"""
    _fields_ = [("members", C.c_uint64 * 2), ("positions", C.c_uint64 * 2)]


def _li_tables(members, positions, nm, npos):
    mo, po = [0, nm[0], nm[0] + nm[1]], [0, npos[0], npos[0] + npos[1]]
    return dict(members=[members[mo[s]:mo[s + 1]] for s in range(2)], positions=[positions[po[s]:po[s + 1]] for s in range(2)],
                members_flat=members, positions_flat=positions, n_members=nm, n_positions=npos)


# interchromosomal junction tables (Engine.int_calls): pg_int_window, pg_int_call, pg_int_sizes
INT_ANCHOR_MINUS, INT_FAR_MINUS, INT_FALLBACK = 1, 2, 4
KERNEL_INT = 12                         # launch-log id of the junction kernels
INT_CALL_DTYPE = np.dtype([("chr", "<i2"), ("far_chr", "<i2"), ("close_abs", "<u4"), ("far_abs", "<u4"), ("first", "<u4"), ("n_reads", "<u4"),
                           ("nt_off", "<u2"), ("nt_len", "<u2"), ("flags", "<u4"), ("reserved", "<u4")])
assert INT_CALL_DTYPE.itemsize == 32


class IntWindow(C.Structure):
    """pg_int_window"""
    _fields_ = [("chr_rank", C.c_void_p), ("n_chr", C.c_uint32)]


class IntSizes(C.Structure):
    """pg_int_sizes"""
    _fields_ = [("members", C.c_uint64), ("calls", C.c_uint64)]


# dispersed-duplication breakpoint tables (Engine.dd_tables): pg_dd_window, pg_dd_member, pg_dd_cand, pg_dd_sizes
DD_TESTED, DD_CONTAINED = 1, 2
KERNEL_DD_TABLES = 13                   # launch-log id of the DD table kernels
DD_MEMBER_DTYPE = np.dtype([("read", "<u4"), ("close_len", "<u2"), ("rc_flag", "u1"), ("reserved", "u1")])
DD_CAND_DTYPE = np.dtype([("seg", "<u4"), ("pos", "<u4"), ("first", "<u4"), ("n_reads", "<u4"), ("cons_off", "<u4"), ("cons_len", "<u4"),
                          ("flags", "<u4"), ("win_len", "<u4"), ("win_start", "<u8")])
assert DD_MEMBER_DTYPE.itemsize == 8 and DD_CAND_DTYPE.itemsize == 40


class DdWindow(C.Structure):
    """pg_dd_window"""
    _fields_ = [("seg_first", C.c_void_p), ("seg_strand", C.c_void_p), ("n_seg", C.c_uint32), ("chr_id", C.c_int32),
                ("min_bp_support", C.c_int32), ("min_map_distance", C.c_int32)]


class DdSizes(C.Structure):
    """pg_dd_sizes"""
    _fields_ = [("members", C.c_uint64), ("cands", C.c_uint64), ("cons_bytes", C.c_uint64)]


class EventWindow(C.Structure):
    """pg_event_window"""
    _fields_ = [("chr_id", C.c_int32), ("win_end", C.c_uint32), ("region_start", C.c_uint32), ("region_end", C.c_uint32),
                ("min_support", C.c_uint32), ("balance_cutoff", C.c_uint32), ("analyze_td", C.c_int32), ("analyze_inv", C.c_int32)]


class EventSizes(C.Structure):
    """pg_event_sizes"""
    _fields_ = [("members", C.c_uint64 * EVENT_TABLES), ("events", C.c_uint64 * EVENT_TABLES), ("unresolved", C.c_uint64)]


class SvEventSizes(C.Structure):
    """pg_sv_event_sizes"""
    _fields_ = [("members", C.c_uint64 * SV_EVENT_TABLES), ("events", C.c_uint64 * SV_EVENT_TABLES),
                ("dropped_runs", C.c_uint64 * SV_EVENT_TABLES)]


class ClassifyParams(C.Structure):
    """pg_classify_params"""
    _fields_ = [("window", EventWindow), ("sv", SvParams), ("max_listed", C.c_int32), ("reserved", C.c_int32)]


def event_window(window):
    """A pg_event_window from an EventWindow (of this module or hostlib's), a dict of its fields or a tuple in field order."""
    if isinstance(window, EventWindow):
        return window
    if isinstance(window, dict):
        return EventWindow(**{k: int(v) for k, v in window.items()})
    if isinstance(window, (tuple, list)):
        return EventWindow(*[int(v) for v in window])
    return EventWindow(*[int(getattr(window, f)) for f, _ in EventWindow._fields_])


# one record of the library's launch log (PgLaunchRec, pg_device.h); it keeps the first LAUNCH_LOG_CAP (pg_ctx::PG_LAUNCH_LOG_CAP)
LaunchRec = namedtuple("LaunchRec", "kernel blocks ns id_bits mode default in_place")
LAUNCH_LOG_CAP = 256

# every symbol include/pindel_pg.h declares
EXPORTS = [
    "pg_default_params", "pg_create", "pg_destroy", "pg_last_error", "pg_get_max_mismatch",
    "pg_load_reference", "pg_load_fasta", "pg_reference_save_packed", "pg_reference_load_packed", "pg_reference_n_chr", "pg_reference_name",
    "pg_reference_comp_size", "pg_reference_fetch", "pg_close_end_batch", "pg_far_end_batch",
    "pg_far_end_batch_from_close", "pg_far_end_batch_from_close_table", "pg_far_end_batch_table", "pg_search_batch_table",
    "pg_search_batch", "pg_search_batch_multi", "pg_result_view_get", "pg_result_free", "pg_expand_runs",
    "pg_device_batch_upload", "pg_device_batch_set_windows", "pg_device_batch_search", "pg_device_batch_download",
    "pg_device_batch_free", "pg_last_search_stats", "pg_device_batch_algorithmic_bytes",
    "pg_device_batch_candidates", "pg_device_batch_repack", "pg_device_batch_pack_search", "pg_dd_contains_batch",
    "pg_load_reference_device", "pg_device_batch_upload_device", "pg_device_batch_result_sizes", "pg_device_batch_download_device",
    "pg_device_batch_variant_candidates", "pg_device_batch_variant_candidates_device",
    "pg_device_batch_sv_candidates", "pg_device_batch_sv_candidates_device",
    "pg_device_batch_events", "pg_device_batch_events_device", "pg_device_batch_event_sizes",
    "pg_device_batch_events_download", "pg_device_batch_events_download_device",
    "pg_device_batch_sv_events", "pg_device_batch_sv_events_device", "pg_device_batch_sv_event_sizes",
    "pg_device_batch_sv_events_download", "pg_device_batch_sv_events_download_device",
    "pg_device_batch_report_reads", "pg_device_batch_report_reads_device", "pg_device_batch_report_sizes",
    "pg_device_batch_report_download", "pg_device_batch_report_download_device", "pg_device_batch_classify",
    "pg_device_batch_search_table",
    "pg_device_batch_li", "pg_device_batch_li_sizes", "pg_device_batch_li_download", "pg_device_batch_li_download_device",
    "pg_device_batch_int", "pg_device_batch_int_sizes", "pg_device_batch_int_download", "pg_device_batch_int_download_device",
    "pg_device_batch_close_search",
    "pg_device_batch_dd", "pg_device_batch_dd_sizes", "pg_device_batch_dd_download", "pg_device_batch_dd_download_device"]


def build(force: bool = False) -> str:
    """hipcc --offload-arch=gfx950 build of the library (cross-compiles without a GPU)."""
    src_dir = os.path.join(_HERE, "csrc")
    srcs = [os.path.join(src_dir, f) for f in os.listdir(src_dir)
            if f.endswith((".hip", ".cpp", ".h"))] + [
        os.path.join(_HERE, "..", "include", "pindel_pg.h")]
    if force or not os.path.exists(LIB_PATH) or any(
            os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs):
        r = subprocess.run(["make", "-C", src_dir, "-B", "all"], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"building {LIB_PATH} failed (make exit {r.returncode}):\n{r.stdout[-8000:]}")
    return LIB_PATH


_lib = None


def use_library(path):
    """Tests: bind a differently configured build of the library (call before the first use)."""
    global _lib, LIB_PATH
    _lib = None
    LIB_PATH = path


def reload_env():
    """The library reads its PG_* environment switches once per process; tests that change one call this afterwards."""
    L = lib()
    L.pg_debug_reload_env.restype = None
    L.pg_debug_reload_env()


def lib():
    """Load the shared library (building it first if the sources are newer)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        build()
    L = C.CDLL(LIB_PATH)
    vp, i32, u32, u64 = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64
    L.pg_default_params.argtypes = [C.POINTER(PgParams)]
    L.pg_default_params.restype = None
    L.pg_create.argtypes = [C.POINTER(PgParams), C.POINTER(vp)]
    L.pg_destroy.argtypes = [vp]
    L.pg_destroy.restype = None
    L.pg_last_error.argtypes = [vp]
    L.pg_last_error.restype = C.c_char_p
    L.pg_get_max_mismatch.argtypes = [vp, vp]
    L.pg_load_reference.argtypes = [vp, i32, C.POINTER(C.c_char_p), C.POINTER(vp), C.POINTER(u64)]
    L.pg_load_fasta.argtypes = [vp, C.c_char_p]
    L.pg_dd_contains_batch.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, vp]
    L.pg_reference_save_packed.argtypes = [vp, C.c_char_p]
    L.pg_reference_load_packed.argtypes = [vp, C.c_char_p]
    L.pg_reference_n_chr.argtypes = [vp]
    L.pg_reference_name.argtypes = [vp, i32]
    L.pg_reference_name.restype = C.c_char_p
    L.pg_reference_comp_size.argtypes = [vp, i32]
    L.pg_reference_comp_size.restype = u64
    L.pg_reference_fetch.argtypes = [vp, i32, u64, u64, vp]
    L.pg_close_end_batch.argtypes = [vp, C.POINTER(PgReadBatch), C.POINTER(vp)]
    L.pg_far_end_batch.argtypes = [vp, C.POINTER(PgReadBatch), vp, C.POINTER(PgWindows)]
    L.pg_far_end_batch_from_close.argtypes = [vp, C.POINTER(PgReadBatch), vp, vp, C.POINTER(PgWindows), C.POINTER(vp)]
    L.pg_search_batch.argtypes = [vp, C.POINTER(PgReadBatch), C.POINTER(vp)]
    L.pg_far_end_batch_table.argtypes = [vp, C.POINTER(PgReadBatch), vp, C.POINTER(PgHintTable)]
    L.pg_far_end_batch_from_close_table.argtypes = [vp, C.POINTER(PgReadBatch), vp, vp, C.POINTER(PgHintTable), C.POINTER(vp)]
    L.pg_search_batch_table.argtypes = [vp, C.POINTER(PgReadBatch), C.POINTER(PgHintTable), C.POINTER(vp)]
    L.pg_search_batch_multi.argtypes = [C.POINTER(vp), i32, C.POINTER(PgReadBatch), C.POINTER(vp)]
    L.pg_result_view_get.argtypes = [vp, C.POINTER(PgResultView)]
    L.pg_result_free.argtypes = [vp]
    L.pg_result_free.restype = None
    L.pg_expand_runs.argtypes = [vp, u64, vp]
    L.pg_expand_runs.restype = u64
    L.pg_device_batch_upload.argtypes = [vp, C.POINTER(PgReadBatch), C.POINTER(vp)]
    L.pg_device_batch_set_windows.argtypes = [vp, vp, C.POINTER(PgWindows)]
    L.pg_device_batch_search.argtypes = [vp, vp]
    L.pg_device_batch_download.argtypes = [vp, vp, C.POINTER(vp)]
    L.pg_device_batch_free.argtypes = [vp, vp]
    L.pg_device_batch_free.restype = None
    L.pg_last_search_stats.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(u64)]
    L.pg_device_batch_algorithmic_bytes.argtypes = [vp, vp, C.POINTER(C.c_double)]
    L.pg_device_batch_candidates.argtypes = [vp, vp, C.POINTER(C.c_double)]
    L.pg_device_batch_repack.argtypes = [vp, vp, C.POINTER(C.c_double)]
    L.pg_device_batch_pack_search.argtypes = [vp, vp]
    L.pg_device_batch_search_table.argtypes = [vp, vp, C.POINTER(PgHintTable)]
    L.pg_debug_last_hint_stats.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(u64), C.POINTER(u64)]
    L.pg_load_reference_device.argtypes = [vp, i32, C.POINTER(C.c_char_p), C.POINTER(vp), C.POINTER(u64)]
    L.pg_device_batch_upload_device.argtypes = [vp, C.POINTER(PgReadBatch), C.POINTER(vp)]
    L.pg_device_batch_result_sizes.argtypes = [vp, vp, C.POINTER(u64), C.POINTER(u64)]
    L.pg_device_batch_download_device.argtypes = [vp, vp, C.POINTER(PgDeviceResult)]
    L.pg_device_batch_variant_candidates.argtypes = [vp, vp, vp, vp]
    L.pg_device_batch_variant_candidates_device.argtypes = [vp, vp, vp, vp]
    L.pg_device_batch_sv_candidates.argtypes = [vp, vp, vp, vp, vp]
    L.pg_device_batch_sv_candidates_device.argtypes = [vp, vp, vp, vp, vp]
    L.pg_device_batch_events.argtypes = [vp] * 8
    L.pg_device_batch_events_device.argtypes = [vp] * 8
    L.pg_device_batch_event_sizes.argtypes = [vp, vp, vp]
    L.pg_device_batch_events_download.argtypes = [vp] * 5
    L.pg_device_batch_events_download_device.argtypes = [vp] * 5
    L.pg_device_batch_sv_events.argtypes = [vp] * 4
    L.pg_device_batch_sv_events_device.argtypes = [vp] * 4
    L.pg_device_batch_sv_event_sizes.argtypes = [vp, vp, vp]
    L.pg_device_batch_sv_events_download.argtypes = [vp] * 4
    L.pg_device_batch_sv_events_download_device.argtypes = [vp] * 4
    L.pg_device_batch_report_reads.argtypes = [vp] * 6
    L.pg_device_batch_report_reads_device.argtypes = [vp] * 6
    L.pg_device_batch_report_sizes.argtypes = [vp, vp, vp]
    L.pg_device_batch_report_download.argtypes = [vp] * 4
    L.pg_device_batch_report_download_device.argtypes = [vp] * 4
    L.pg_device_batch_classify.argtypes = [vp] * 4
    L.pg_device_batch_li.argtypes = [vp, vp, vp]
    L.pg_device_batch_li_sizes.argtypes = [vp, vp, vp]
    L.pg_device_batch_li_download.argtypes = [vp] * 4
    L.pg_device_batch_li_download_device.argtypes = [vp] * 4
    L.pg_device_batch_int.argtypes = [vp, vp, vp]
    L.pg_device_batch_int_sizes.argtypes = [vp, vp, vp]
    L.pg_device_batch_int_download.argtypes = [vp] * 4
    L.pg_device_batch_int_download_device.argtypes = [vp] * 4
    L.pg_device_batch_close_search.argtypes = [vp, vp]
    L.pg_device_batch_dd.argtypes = [vp, vp, vp]
    L.pg_device_batch_dd_sizes.argtypes = [vp, vp, vp]
    L.pg_device_batch_dd_download.argtypes = [vp] * 5
    L.pg_device_batch_dd_download_device.argtypes = [vp] * 5
    _lib = L
    return L


def expand_runs(runs: np.ndarray) -> np.ndarray:
    """pg_expand_runs: run-length-encoded runs -> UniquePoint records."""
    L = lib()
    runs = np.ascontiguousarray(runs, dtype=RUN_DTYPE)
    n = L.pg_expand_runs(runs.ctypes.data, len(runs), None)
    out = np.zeros(n, dtype=POINT_DTYPE)
    if n:
        L.pg_expand_runs(runs.ctypes.data, len(runs), out.ctypes.data)
    return out


class Result:
    """Host copy of a pg_result: CSR runs for UP_Close / UP_Far + rc flags."""

    def __init__(self, handle, owner):
        self._h = handle
        self._owner = owner
        v = PgResultView()
        rc = lib().pg_result_view_get(handle, C.byref(v))
        if rc:
            raise PgError(rc)
        n = v.n_reads
        self.n = n
        self.close_off = np.ctypeslib.as_array(v.close_off, shape=(n + 1,)).copy()
        self.far_off = np.ctypeslib.as_array(v.far_off, shape=(n + 1,)).copy()
        self.rc_flag = np.ctypeslib.as_array(v.rc_flag, shape=(n,)).copy() if n else np.zeros(0, np.uint8)

        def runs(ptr, cnt):
            if not cnt:
                return np.zeros(0, dtype=RUN_DTYPE)
            buf = (C.c_uint8 * (cnt * 12)).from_address(ptr)
            return np.frombuffer(buf, dtype=RUN_DTYPE).copy()
        self.close_runs = runs(v.close_runs, int(self.close_off[-1]))
        self.far_runs = runs(v.far_runs, int(self.far_off[-1]))

    def refresh(self):
        self.__init__(self._h, self._owner)

    def close_points(self, i):
        return expand_runs(self.close_runs[int(self.close_off[i]):int(self.close_off[i + 1])])

    def far_points(self, i):
        return expand_runs(self.far_runs[int(self.far_off[i]):int(self.far_off[i + 1])])

    def free(self):
        if self._h:
            lib().pg_result_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class HintTable:
    """A pg_hint_table: BreakDancer hints keyed by position.  Run k covers the close-end positions
    [run_first[k], run_first[k + 1]) and names cluster run_cluster[k], whose windows are windows[cluster_off[c]:cluster_off[c + 1]].
    The arrays are taken as they are (the library validates them)."""

    def __init__(self, run_first, run_cluster, cluster_off, windows):
        self.run_first = np.ascontiguousarray(run_first, dtype=np.uint32)
        self.run_cluster = np.ascontiguousarray(run_cluster, dtype=np.uint32)
        self.cluster_off = np.ascontiguousarray(cluster_off, dtype=np.uint64)
        self.windows = np.ascontiguousarray(windows, dtype=WINDOW_DTYPE)

    def struct(self):
        def ptr(a):
            return a.ctypes.data if len(a) else None
        return PgHintTable(len(self.run_cluster), ptr(self.run_first), ptr(self.run_cluster),
                           max(len(self.cluster_off) - 1, 0), ptr(self.cluster_off), ptr(self.windows))

    def expand(self, close_last, close_max):
        """The lookup rule restated in numpy: the per-read (bd, bd_off) the table stands for."""
        p = np.asarray(close_last, dtype=np.int64)
        has = np.asarray(close_max, dtype=np.int64) > 0
        n_runs = len(self.run_cluster)
        counts = np.zeros(len(p), dtype=np.int64)
        first = np.zeros(len(p), dtype=np.int64)
        if n_runs and len(p):
            rf = self.run_first.astype(np.int64)
            k = np.searchsorted(rf, p, side="right") - 1
            ok = has & (p >= rf[0]) & (p < rf[n_runs])
            c = self.run_cluster[np.clip(k, 0, n_runs - 1)].astype(np.int64)
            off = self.cluster_off.astype(np.int64)
            counts = np.where(ok, off[c + 1] - off[c], 0)
            first = off[c]
        bd_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        idx = np.repeat(first - bd_off[:-1].astype(np.int64), counts) + np.arange(int(bd_off[-1]), dtype=np.int64)
        return self.windows[idx], bd_off


def _hint_args(bd, hints):
    if bd is not None and hints is not None:
        raise ValueError("give either per-read windows (bd, bd_off) or a HintTable (hints), not both")


def _windows_struct(bd, bd_off):
    """(bd, bd_off) -> (PgWindows or None, keepalive)."""
    if bd is None:
        return None, ()
    bd = np.ascontiguousarray(bd, dtype=WINDOW_DTYPE)
    bd_off = np.ascontiguousarray(bd_off, dtype=np.uint64)
    return PgWindows(bd_off.ctypes.data, bd.ctypes.data), (bd, bd_off)


def _batch_struct(batch):
    """batch: pindel_amd.hostio.ReadBatch -> (PgReadBatch, keepalive)."""
    seq = np.ascontiguousarray(batch.seq, dtype=np.uint8)
    off = np.ascontiguousarray(batch.seq_off, dtype=np.uint64)
    st = np.ascontiguousarray(batch.anchor_strand, dtype=np.uint8)
    pos = np.ascontiguousarray(batch.anchor_pos, dtype=np.int32)
    isz = np.ascontiguousarray(batch.insert_size, dtype=np.int16)
    cid = np.ascontiguousarray(batch.chr_id, dtype=np.int32)
    s = PgReadBatch(len(off) - 1, seq.ctypes.data, off.ctypes.data, st.ctypes.data,
                    pos.ctypes.data, isz.ctypes.data, cid.ctypes.data)
    return s, (seq, off, st, pos, isz, cid)


# ---- torch tensors in device memory (Engine.load_reference_tensors / upload_tensors / download_tensors).  The checks are plain
# functions of the tensors' attributes: they need no GPU and do not import torch (the methods that call them do).
# seq_off and the result offsets travel as int64: the same bits as the ABI's uint64 below 2^63 (torch has no full uint64);
# close_last likewise as int32.
READ_TENSOR_DTYPES = (("seq", ("torch.uint8",)), ("seq_off", ("torch.int64", "torch.uint64")), ("anchor_strand", ("torch.uint8",)),
                      ("anchor_pos", ("torch.int32",)), ("insert_size", ("torch.int16",)), ("chr_id", ("torch.int32",)))


def check_tensor(name, t, dtypes, device, length=None):
    """ValueError unless t is a 1-D contiguous tensor of one of `dtypes` (their str(), e.g. "torch.uint8") on `device` (its str(),
    e.g. "cuda:0"), with `length` elements when one is given."""
    if not hasattr(t, "dtype") or not hasattr(t, "is_contiguous") or not hasattr(t, "data_ptr"):
        raise ValueError(f"{name}: a torch tensor is expected, got {type(t).__name__}")
    if str(t.dtype) not in dtypes:
        raise ValueError(f"{name}: dtype {t.dtype}, expected {' or '.join(dtypes)}")
    if t.dim() != 1:
        raise ValueError(f"{name}: {t.dim()} dimensions, expected 1")
    if not t.is_contiguous():
        raise ValueError(f"{name}: not contiguous")
    if str(t.device) != device:
        raise ValueError(f"{name}: on {t.device}, expected {device}")
    if length is not None and t.numel() != length:
        raise ValueError(f"{name}: {t.numel()} elements, expected {length}")


def check_read_tensors(seq, seq_off, anchor_strand, anchor_pos, insert_size, chr_id, device):
    """The wrapper's checks of upload_tensors, before the library is called; returns the number of reads."""
    if not hasattr(seq_off, "numel") or seq_off.numel() < 1:
        raise ValueError("seq_off: n + 1 offsets are expected, at least one")
    n = seq_off.numel() - 1
    given = dict(seq=seq, seq_off=seq_off, anchor_strand=anchor_strand, anchor_pos=anchor_pos, insert_size=insert_size, chr_id=chr_id)
    for name, dtypes in READ_TENSOR_DTYPES:
        check_tensor(name, given[name], dtypes, device, None if name == "seq" else n + 1 if name == "seq_off" else n)
    last = int(seq_off[-1].item())
    if seq.numel() < last:
        raise ValueError(f"seq: {seq.numel()} bases, shorter than seq_off[-1] = {last}")
    return n


def check_reference_tensors(chroms, device):
    """The wrapper's checks of load_reference_tensors: [(name, uint8 tensor)]."""
    for nm, t in chroms:
        check_tensor(f"chromosome {nm}", t, ("torch.uint8",), device)


def runs_from_tensor(t) -> np.ndarray:
    """The uint8[n_runs, 12] tensor of download_tensors as a RUN_DTYPE array (a CPU copy)."""
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return a.reshape(-1).view(RUN_DTYPE)


def sv_cands_from_tensor(t) -> np.ndarray:
    """The uint8[n, SV_SLOTS * 32] tensor of sv_candidates_tensors as a VARIANT_CAND_DTYPE[n, SV_SLOTS] array (a CPU copy)."""
    a = np.ascontiguousarray(t.cpu().numpy())
    return a.reshape(-1).view(VARIANT_CAND_DTYPE).reshape(-1, SV_SLOTS)


def _event_tables(reads, members, events, nm, ne, unresolved):
    mo = np.concatenate([[0], np.cumsum(nm)]).astype(np.int64)
    eo = np.concatenate([[0], np.cumsum(ne)]).astype(np.int64)
    return dict(reads=reads, members=[members[mo[t]:mo[t + 1]] for t in range(EVENT_TABLES)],
                events=[events[eo[t]:eo[t + 1]] for t in range(EVENT_TABLES)], unresolved=int(unresolved),
                members_flat=members, events_flat=events, n_members=list(nm), n_events=list(ne))


def _sv_event_tables(members, events, nm, ne, dropped):
    mo = np.concatenate([[0], np.cumsum(nm)]).astype(np.int64)
    eo = np.concatenate([[0], np.cumsum(ne)]).astype(np.int64)
    return dict(members=[members[mo[t]:mo[t + 1]] for t in range(SV_EVENT_TABLES)],
                events=[events[eo[t]:eo[t + 1]] for t in range(SV_EVENT_TABLES)], dropped_runs=list(dropped),
                members_flat=members, events_flat=events, n_members=list(nm), n_events=list(ne))


def sv_events_from_tensors(t) -> dict:
    """The dict of sv_events_tensors as the dict sv_events returns (CPU copies)."""
    members = np.ascontiguousarray(t["members"].cpu().numpy()).view(np.uint32)
    events = np.ascontiguousarray(t["events"].cpu().numpy()).reshape(-1).view(EVENT_DTYPE)
    return _sv_event_tables(members, events, t["n_members"], t["n_events"], t["dropped_runs"])


def events_from_tensors(t) -> dict:
    """The dict of events_tensors as the dict events returns (CPU copies)."""
    reads = np.ascontiguousarray(t["reads"].cpu().numpy()).reshape(-1).view(EVENT_READ_DTYPE)
    members = np.ascontiguousarray(t["members"].cpu().numpy()).view(np.uint32)
    events = np.ascontiguousarray(t["events"].cpu().numpy()).reshape(-1).view(EVENT_DTYPE)
    return _event_tables(reads, members, events, t["n_members"], t["n_events"], t["unresolved"])


def variant_cands_from_tensor(t) -> np.ndarray:
    """The uint8[n, 256] tensor of variant_candidates_tensors as a VARIANT_CAND_DTYPE[n, 2, VARIANT_CANDS] array (a CPU copy)."""
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return a.reshape(-1).view(VARIANT_CAND_DTYPE).reshape(-1, 2, VARIANT_CANDS)


class Engine:
    """One pg_ctx = one GPU."""

    def __init__(self, device=0, max_range_index=2, additional_mismatch=1, min_perfect_match=3,
                 min_close=8, max_mismatch_rate=0.02, seq_error_rate=0.01, sensitivity=0.95,
                 spacer=100000):
        L = lib()
        p = PgParams()
        L.pg_default_params(C.byref(p))
        p.device = device
        p.max_range_index = max_range_index
        p.additional_mismatch = additional_mismatch
        p.min_perfect_match_around_bp = min_perfect_match
        p.min_close = min_close
        p.max_allowed_mismatch_rate = max_mismatch_rate
        p.seq_error_rate = seq_error_rate
        p.sensitivity = sensitivity
        p.spacer = spacer
        h = C.c_void_p()
        rc = L.pg_create(C.byref(p), C.byref(h))
        if rc:
            raise PgError(rc, "pg_create failed (no usable HIP device?)" if rc == PG_E_DEVICE else "pg_create")
        self._h = h
        self._L = L
        self._device = device
        self._batch_n = {}       # reads of every live device batch, by handle (download_tensors sizes its tensors from it)

    def _check(self, rc):
        if rc:
            raise PgError(rc, (self._L.pg_last_error(self._h) or b"").decode())

    def close(self):
        if self._h:
            self._L.pg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def max_mismatch_table(self):
        t = np.zeros(500, dtype=np.uint32)
        self._check(self._L.pg_get_max_mismatch(self._h, t.ctypes.data))
        return t

    def load_reference(self, chroms):
        """chroms: [(name, padded_bytes)] as hostio.load_fasta returns."""
        n = len(chroms)
        names = (C.c_char_p * n)(*[nm.encode() for nm, _ in chroms])
        bufs = [np.frombuffer(s, dtype=np.uint8) for _, s in chroms]
        ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        lens = (C.c_uint64 * n)(*[len(b) for b in bufs])
        self._check(self._L.pg_load_reference(self._h, n, names, ptrs, lens))

    def load_fasta(self, path):
        self._check(self._L.pg_load_fasta(self._h, str(path).encode()))

    def save_packed(self, path):
        self._check(self._L.pg_reference_save_packed(self._h, str(path).encode()))

    def load_packed(self, path):
        self._check(self._L.pg_reference_load_packed(self._h, str(path).encode()))

    def reference_info(self):
        n = self._L.pg_reference_n_chr(self._h)
        return [(self._L.pg_reference_name(self._h, c).decode(),
                 int(self._L.pg_reference_comp_size(self._h, c))) for c in range(n)]

    def reference_fetch(self, chr_id, start, n):
        out = np.zeros(n, dtype=np.uint8)
        self._check(self._L.pg_reference_fetch(self._h, chr_id, start, n, out.ctypes.data))
        return out.tobytes()

    def dd_contains(self, queries, chr_id, win_start, win_len):
        """-q's containment test (pg_dd_contains_batch): per item, contains_subseq_any_strand(queries[i], the loaded chromosome
        chr_id[i] at padded positions [win_start[i], win_start[i] + win_len[i]), 15).  Returns (uint8 array, kernel ms)."""
        n = len(queries)
        qb = [bytes(q) if not isinstance(q, str) else q.encode() for q in queries]
        q = np.frombuffer(b"".join(qb) or b"\0", dtype=np.uint8)
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(x) for x in qb]) if n else []
        cid = np.ascontiguousarray(chr_id, dtype=np.int32)
        ws = np.ascontiguousarray(win_start, dtype=np.uint64)
        wl = np.ascontiguousarray(win_len, dtype=np.uint32)
        out = np.zeros(max(n, 1), dtype=np.uint8)
        self._check(self._L.pg_dd_contains_batch(self._h, n, q.ctypes.data, off.ctypes.data, cid.ctypes.data, ws.ctypes.data,
                                                 wl.ctypes.data, out.ctypes.data))
        ms = C.c_double()
        self._L.pg_last_search_stats(self._h, C.byref(ms), None)
        return out[:n], ms.value

    # ---- host in / host out
    def close_end_batch(self, batch) -> Result:
        s, keep = _batch_struct(batch)
        h = C.c_void_p()
        self._check(self._L.pg_close_end_batch(self._h, C.byref(s), C.byref(h)))
        return Result(h, self)

    def far_end_batch(self, batch, close: Result, bd=None, bd_off=None, hints=None) -> Result:
        _hint_args(bd, hints)
        s, keep = _batch_struct(batch)
        if hints is not None:
            entry, h = self._L.pg_far_end_batch_table, hints.struct()
        else:
            entry = self._L.pg_far_end_batch
            h, keep_w = _windows_struct(bd, bd_off)
        self._check(entry(self._h, C.byref(s), close._h, C.byref(h) if h is not None else None))
        close.refresh()
        return close

    def far_end_batch_from_close(self, batch, close_last, close_max, bd=None, bd_off=None, hints=None) -> Result:
        """pg_far_end_batch_from_close: the reads as the close end left them + UP_Close.back()'s AbsLoc / LengthStr.
        hints: a HintTable looked up on the device (pg_far_end_batch_from_close_table) instead of per-read windows."""
        _hint_args(bd, hints)
        s, keep = _batch_struct(batch)
        cl = np.ascontiguousarray(close_last, dtype=np.uint32)
        cm = np.ascontiguousarray(close_max, dtype=np.int16)
        if hints is not None:
            entry, h = self._L.pg_far_end_batch_from_close_table, hints.struct()
        else:
            entry = self._L.pg_far_end_batch_from_close
            h, keep_w = _windows_struct(bd, bd_off)
        out = C.c_void_p()
        self._check(entry(self._h, C.byref(s), cl.ctypes.data, cm.ctypes.data, C.byref(h) if h is not None else None, C.byref(out)))
        return Result(out, self)

    def search_batch(self, batch, hints=None) -> Result:
        """hints: a HintTable -- close end, lookup on the device, far end (pg_search_batch_table)."""
        s, keep = _batch_struct(batch)
        h = C.c_void_p()
        if hints is not None:
            t = hints.struct()
            self._check(self._L.pg_search_batch_table(self._h, C.byref(s), C.byref(t), C.byref(h)))
        else:
            self._check(self._L.pg_search_batch(self._h, C.byref(s), C.byref(h)))
        return Result(h, self)

    def last_hint_stats(self):
        """measurement: the last hint-table lookup of this context -- HIP-event ms of its count + scan kernels and of its fill
        kernel, bytes of the table uploaded, windows written"""
        a, b, c, d = C.c_double(), C.c_double(), C.c_uint64(), C.c_uint64()
        self._check(self._L.pg_debug_last_hint_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, d.value

    @staticmethod
    def search_batch_multi(engines, batch) -> "Result":
        """pg_search_batch_multi: contiguous shards of one batch on several contexts (one GPU each), concatenated."""
        s, keep = _batch_struct(batch)
        hs = (C.c_void_p * len(engines))(*[e._h for e in engines])
        h = C.c_void_p()
        rc = lib().pg_search_batch_multi(hs, len(engines), C.byref(s), C.byref(h))
        if rc:
            raise PgError(rc, (lib().pg_last_error(engines[0]._h) or b"").decode())
        return Result(h, engines[0])

    # ---- device resident
    def upload(self, batch):
        s, keep = _batch_struct(batch)
        h = C.c_void_p()
        self._check(self._L.pg_device_batch_upload(self._h, C.byref(s), C.byref(h)))
        self._batch_n[h.value] = s.n_reads
        return h

    # ---- device memory in and out (torch tensors on this engine's GPU)
    def _torch_ready(self):
        """torch, this engine's device string, after waiting for torch's current stream on it (the library's calls are synchronous
        and run on streams of its own: what the caller queued must have finished)."""
        import torch
        torch.cuda.current_stream(self._device).synchronize()
        return torch, f"cuda:{self._device}"

    def load_reference_tensors(self, chroms):
        """load_reference with the padded chromosomes as uint8 tensors on the GPU: [(name, tensor)] (pg_load_reference_device).
        A tensor may be a slice of a larger one."""
        _, dev = self._torch_ready()
        check_reference_tensors(chroms, dev)
        n = len(chroms)
        names = (C.c_char_p * n)(*[nm.encode() for nm, _ in chroms])
        ptrs = (C.c_void_p * n)(*[t.data_ptr() for _, t in chroms])
        lens = (C.c_uint64 * n)(*[t.numel() for _, t in chroms])
        self._check(self._L.pg_load_reference_device(self._h, n, names, ptrs, lens))

    def upload_tensors(self, seq, seq_off, anchor_strand, anchor_pos, insert_size, chr_id):
        """upload with the batch's six arrays as tensors on the GPU (pg_device_batch_upload_device); the library copies them."""
        _, dev = self._torch_ready()
        n = check_read_tensors(seq, seq_off, anchor_strand, anchor_pos, insert_size, chr_id, dev)
        s = PgReadBatch(n, seq.data_ptr() if seq.numel() else None, seq_off.data_ptr(), anchor_strand.data_ptr(),
                        anchor_pos.data_ptr(), insert_size.data_ptr(), chr_id.data_ptr())
        h = C.c_void_p()
        self._check(self._L.pg_device_batch_upload_device(self._h, C.byref(s), C.byref(h)))
        self._batch_n[h.value] = n
        return h

    def result_sizes(self, dbatch):
        """(close runs, far runs) a download of the searched batch holds (pg_device_batch_result_sizes)."""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self._L.pg_device_batch_result_sizes(self._h, dbatch, C.byref(a), C.byref(b)))
        return a.value, b.value

    def download_into(self, dbatch, close_off, close_runs, far_off, far_runs, rc_flag=None, close_last=None, close_max=None):
        """pg_device_batch_download_device into tensors of the caller's: offsets int64[n + 1], runs uint8[capacity, 12], the
        optional summaries uint8 / int32 / int16 [n]."""
        _, dev = self._torch_ready()
        n = self._batch_n[dbatch.value]
        check_tensor("close_off", close_off, ("torch.int64", "torch.uint64"), dev, n + 1)
        check_tensor("far_off", far_off, ("torch.int64", "torch.uint64"), dev, n + 1)
        for name, t in (("close_runs", close_runs), ("far_runs", far_runs)):
            if str(t.dtype) != "torch.uint8" or t.dim() != 2 or t.shape[1] != 12 or not t.is_contiguous() or str(t.device) != dev:
                raise ValueError(f"{name}: a contiguous uint8[capacity, 12] tensor on {dev} is expected")
        for name, t, dt in (("rc_flag", rc_flag, "torch.uint8"), ("close_last", close_last, "torch.int32"), ("close_max", close_max, "torch.int16")):
            if t is not None:
                check_tensor(name, t, (dt,), dev, n)

        def ptr(t):
            return t.data_ptr() if t is not None and t.numel() else None
        d = PgDeviceResult(close_off.data_ptr(), ptr(close_runs), close_runs.shape[0], far_off.data_ptr(), ptr(far_runs),
                           far_runs.shape[0], ptr(rc_flag), ptr(close_last), ptr(close_max))
        self._check(self._L.pg_device_batch_download_device(self._h, dbatch, C.byref(d)))

    def download_tensors(self, dbatch, summaries=True):
        """download with the result staying on the GPU: a dict of tensors on this engine's device -- close_off / far_off int64[n + 1],
        close_runs / far_runs uint8[n_runs, 12] (runs_from_tensor views a CPU copy as RUN_DTYPE), and unless summaries is False
        rc_flag uint8[n], close_last int32[n], close_max int16[n]."""
        torch, dev = self._torch_ready()
        n = self._batch_n[dbatch.value]
        nc, nf = self.result_sizes(dbatch)
        out = dict(close_off=torch.empty(n + 1, dtype=torch.int64, device=dev), close_runs=torch.empty((nc, 12), dtype=torch.uint8, device=dev),
                   far_off=torch.empty(n + 1, dtype=torch.int64, device=dev), far_runs=torch.empty((nf, 12), dtype=torch.uint8, device=dev))
        if summaries:
            out.update(rc_flag=torch.empty(n, dtype=torch.uint8, device=dev), close_last=torch.empty(n, dtype=torch.int32, device=dev),
                       close_max=torch.empty(n, dtype=torch.int16, device=dev))
        self.download_into(dbatch, **out)
        return out

    def variant_candidates(self, dbatch):
        """The device classifier on a searched device batch (pg_device_batch_variant_candidates): per read the first VARIANT_CANDS
        deletion (kind 0) and short-insertion (kind 1) candidates in the order Pindel's loops first visit them.  Returns (cands,
        counts): VARIANT_CAND_DTYPE[n, 2, VARIANT_CANDS] and uint8[n, 2] (low bits: pairs listed, VARIANT_MORE: more exist).
        last_stats()[0] is then the kernel's HIP-event time."""
        n = self._batch_n[dbatch.value]
        cands = np.zeros((n, 2, VARIANT_CANDS), dtype=VARIANT_CAND_DTYPE)
        counts = np.zeros((n, 2), dtype=np.uint8)
        self._check(self._L.pg_device_batch_variant_candidates(self._h, dbatch, cands.ctypes.data if n else None,
                                                               counts.ctypes.data if n else None))
        return cands, counts

    def variant_candidates_into(self, dbatch, cands, counts):
        """pg_device_batch_variant_candidates_device into tensors of the caller's on this engine's GPU: cands uint8[n, 2 *
        VARIANT_CANDS * 32] (the records' bytes), counts uint8[n, 2]."""
        _, dev = self._torch_ready()
        n = self._batch_n[dbatch.value]
        for name, t, width in (("cands", cands, 2 * VARIANT_CANDS * 32), ("counts", counts, 2)):
            if str(t.dtype) != "torch.uint8" or t.dim() != 2 or tuple(t.shape) != (n, width) or not t.is_contiguous() or str(t.device) != dev:
                raise ValueError(f"{name}: a contiguous uint8[{n}, {width}] tensor on {dev} is expected")
        self._check(self._L.pg_device_batch_variant_candidates_device(self._h, dbatch, cands.data_ptr() if n else None,
                                                                      counts.data_ptr() if n else None))

    def variant_candidates_tensors(self, dbatch):
        """variant_candidates with the lists staying on the GPU: a dict of tensors on this engine's device -- cands uint8[n, 256]
        (variant_cands_from_tensor views a CPU copy as VARIANT_CAND_DTYPE[n, 2, VARIANT_CANDS]) and counts uint8[n, 2]."""
        torch, dev = self._torch_ready()
        n = self._batch_n[dbatch.value]
        out = dict(cands=torch.empty((n, 2 * VARIANT_CANDS * 32), dtype=torch.uint8, device=dev),
                   counts=torch.empty((n, 2), dtype=torch.uint8, device=dev))
        self.variant_candidates_into(dbatch, **out)
        return out

    def sv_candidates(self, dbatch, settings=None):
        """The device classifier of the five other kinds on a searched device batch (pg_device_batch_sv_candidates): per read the
        DI, TD_NT and INV_NT candidate and the first VARIANT_CANDS tandem-duplication and inversion candidates in the order Pindel's
        loops first visit them.  settings: see sv_params().  Returns (cands, counts): VARIANT_CAND_DTYPE[n, SV_SLOTS] (SV_SLOT[kind] =
        the kind's first record) and uint8[n, SV_KINDS] (SV_COUNT[kind]; low bits: pairs listed, VARIANT_MORE: more exist)."""
        n = self._batch_n[dbatch.value]
        prm = sv_params(settings)
        cands = np.zeros((n, SV_SLOTS), dtype=VARIANT_CAND_DTYPE)
        counts = np.zeros((n, SV_KINDS), dtype=np.uint8)
        self._check(self._L.pg_device_batch_sv_candidates(self._h, dbatch, C.addressof(prm), cands.ctypes.data if n else None,
                                                          counts.ctypes.data if n else None))
        return cands, counts

    def sv_candidates_into(self, dbatch, cands, counts, settings=None):
        """pg_device_batch_sv_candidates_device into tensors of the caller's on this engine's GPU: cands uint8[n, SV_SLOTS * 32]
        (the records' bytes), counts uint8[n, SV_KINDS]."""
        _, dev = self._torch_ready()
        n = self._batch_n[dbatch.value]
        prm = sv_params(settings)
        for name, t, width in (("cands", cands, SV_SLOTS * 32), ("counts", counts, SV_KINDS)):
            if str(t.dtype) != "torch.uint8" or t.dim() != 2 or tuple(t.shape) != (n, width) or not t.is_contiguous() or str(t.device) != dev:
                raise ValueError(f"{name}: a contiguous uint8[{n}, {width}] tensor on {dev} is expected")
        self._check(self._L.pg_device_batch_sv_candidates_device(self._h, dbatch, C.addressof(prm), cands.data_ptr() if n else None,
                                                                 counts.data_ptr() if n else None))

    def sv_candidates_tensors(self, dbatch, settings=None):
        """sv_candidates with the lists staying on the GPU: a dict of tensors on this engine's device -- cands uint8[n, SV_SLOTS *
        32] (sv_cands_from_tensor views a CPU copy as VARIANT_CAND_DTYPE[n, SV_SLOTS]) and counts uint8[n, SV_KINDS]."""
        torch, dev = self._torch_ready()
        n = self._batch_n[dbatch.value]
        out = dict(cands=torch.empty((n, SV_SLOTS * 32), dtype=torch.uint8, device=dev),
                   counts=torch.empty((n, SV_KINDS), dtype=torch.uint8, device=dev))
        self.sv_candidates_into(dbatch, settings=settings, **out)
        return out

    def event_sizes(self, dbatch):
        """pg_device_batch_event_sizes: (members per table, events per table, unresolved reads) of the tables built last."""
        sz = EventSizes()
        self._check(self._L.pg_device_batch_event_sizes(self._h, dbatch, C.addressof(sz)))
        return [int(x) for x in sz.members], [int(x) for x in sz.events], int(sz.unresolved)

    def events(self, dbatch, window, variant=None, sv=None, name_id=None):
        """Event tables of a searched device batch for one window (pg_device_batch_events): the window-dependent tail
        and Used cascade of all seven classifiers over the candidate lists, then the boxed reads of deletions, short insertions, TD
        and TD_NT sorted, duplicates marked and grouped into events, all on the GPU.  window: see event_window(); variant / sv: the
        (cands, counts) pairs variant_candidates / sv_candidates return, or None (empty lists); name_id: None (all names differ) or
        uint32 per read.  Returns a dict: reads EVENT_READ_DTYPE[n]; members and events, lists of four arrays (uint32 read indices,
        EVENT_DTYPE) in EVENT_KINDS order; unresolved; members_flat / events_flat (the four back to back, as downloaded)."""
        n = self._batch_n[dbatch.value]
        w = event_window(window)
        keep = []

        def ptr(a, dtype, size):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype)
            if a.size != size:
                raise ValueError(f"events: an array of {size} {dtype} is expected, got {a.size}")
            keep.append(a)
            return a.ctypes.data if size else None
        vc = vn = sc = sn = None
        if variant is not None:
            vc, vn = ptr(variant[0], VARIANT_CAND_DTYPE, n * 2 * VARIANT_CANDS), ptr(variant[1], np.uint8, n * 2)
        if sv is not None:
            sc, sn = ptr(sv[0], VARIANT_CAND_DTYPE, n * SV_SLOTS), ptr(sv[1], np.uint8, n * SV_KINDS)
        nid = ptr(name_id, np.uint32, n)
        self._check(self._L.pg_device_batch_events(self._h, dbatch, C.addressof(w), vc, vn, sc, sn, nid))
        nm, ne, unresolved = self.event_sizes(dbatch)
        reads = np.zeros(n, dtype=EVENT_READ_DTYPE)
        members = np.zeros(sum(nm), dtype=np.uint32)
        events = np.zeros(sum(ne), dtype=EVENT_DTYPE)
        self._check(self._L.pg_device_batch_events_download(self._h, dbatch, reads.ctypes.data if n else None,
                                                            members.ctypes.data if members.size else None,
                                                            events.ctypes.data if events.size else None))
        return _event_tables(reads, members, events, nm, ne, unresolved)

    def events_tensors(self, dbatch, window, variant=None, sv=None, name_id=None):
        """events with everything staying on the GPU (pg_device_batch_events_device and its download sibling): variant / sv are the
        dicts variant_candidates_tensors / sv_candidates_tensors return (or (cands, counts) tensor pairs), name_id an int32 / uint32
        tensor of n entries or None.  Returns a dict of tensors on this engine's device: reads uint8[n, 8], members int32[total],
        events uint8[total, 40], plus n_members / n_events (lists of four) and unresolved."""
        torch, dev = self._torch_ready()
        n = self._batch_n[dbatch.value]
        w = event_window(window)

        def pair(x, widths):
            if x is None:
                return None, None
            c, k = (x["cands"], x["counts"]) if isinstance(x, dict) else x
            for name, t, width in (("cands", c, widths[0]), ("counts", k, widths[1])):
                if str(t.dtype) != "torch.uint8" or tuple(t.shape) != (n, width) or not t.is_contiguous() or str(t.device) != dev:
                    raise ValueError(f"events: {name}: a contiguous uint8[{n}, {width}] tensor on {dev} is expected")
            return (c.data_ptr(), k.data_ptr()) if n else (None, None)
        vc, vn = pair(variant, (2 * VARIANT_CANDS * 32, 2))
        sc, sn = pair(sv, (SV_SLOTS * 32, SV_KINDS))
        nid = None
        if name_id is not None:
            if name_id.numel() != n or name_id.element_size() != 4 or not name_id.is_contiguous() or str(name_id.device) != dev:
                raise ValueError(f"events: name_id: a contiguous 32-bit tensor of {n} entries on {dev} is expected")
            nid = name_id.data_ptr() if n else None
        self._check(self._L.pg_device_batch_events_device(self._h, dbatch, C.addressof(w), vc, vn, sc, sn, nid))
        nm, ne, unresolved = self.event_sizes(dbatch)
        out = dict(reads=torch.empty((n, 8), dtype=torch.uint8, device=dev), members=torch.empty(sum(nm), dtype=torch.int32, device=dev),
                   events=torch.empty((sum(ne), 40), dtype=torch.uint8, device=dev))
        self._check(self._L.pg_device_batch_events_download_device(self._h, dbatch, out["reads"].data_ptr() if n else None,
                                                                   out["members"].data_ptr() if sum(nm) else None,
                                                                   out["events"].data_ptr() if sum(ne) else None))
        out.update(n_members=nm, n_events=ne, unresolved=unresolved)
        return out

    def sv_event_sizes(self, dbatch):
        """pg_device_batch_sv_event_sizes: (members, events, dropped runs) per SV table of the tables built last."""
        sz = SvEventSizes()
        self._check(self._L.pg_device_batch_sv_event_sizes(self._h, dbatch, C.addressof(sz)))
        return [int(x) for x in sz.members], [int(x) for x in sz.events], [int(x) for x in sz.dropped_runs]

    def sv_events(self, dbatch, sv):
        """Event tables of DI, INV and INV_NT (pg_device_batch_sv_events) from the per-read records the last events()
        of this batch left with it, for that build's window: each box in the order the reporters' strict exchange sorts leave,
        duplicates, the inversions' runs harmonised, events -- all on the GPU.  sv: the (cands, counts) pair that build was given.
        Returns a dict: members and events, lists of three arrays (uint32 member words -- read indices, SVEV_MEMBER_DUP marking an
        inversion's duplicates -- and EVENT_DTYPE) in SV_EVENT_KINDS order; dropped_runs; members_flat / events_flat."""
        n = self._batch_n[dbatch.value]
        sc = np.ascontiguousarray(sv[0], dtype=VARIANT_CAND_DTYPE)
        sn = np.ascontiguousarray(sv[1], dtype=np.uint8)
        if sc.size != n * SV_SLOTS or sn.size != n * SV_KINDS:
            raise ValueError(f"sv_events: {sc.size} records and {sn.size} counts for {n} reads")
        self._check(self._L.pg_device_batch_sv_events(self._h, dbatch, sc.ctypes.data if n else None, sn.ctypes.data if n else None))
        nm, ne, dropped = self.sv_event_sizes(dbatch)
        members = np.zeros(sum(nm), dtype=np.uint32)
        events = np.zeros(sum(ne), dtype=EVENT_DTYPE)
        self._check(self._L.pg_device_batch_sv_events_download(self._h, dbatch, members.ctypes.data if members.size else None,
                                                               events.ctypes.data if events.size else None))
        return _sv_event_tables(members, events, nm, ne, dropped)

    def sv_events_tensors(self, dbatch, sv):
        """sv_events with everything staying on the GPU (pg_device_batch_sv_events_device and its download sibling): sv is the dict
        sv_candidates_tensors returns (or a (cands, counts) tensor pair).  Returns a dict of tensors on this engine's device:
        members int32[total], events uint8[total, 40], plus n_members / n_events / dropped_runs (lists of three)."""
        torch, dev = self._torch_ready()
        n = self._batch_n[dbatch.value]
        c, k = (sv["cands"], sv["counts"]) if isinstance(sv, dict) else sv
        for name, t, width in (("cands", c, SV_SLOTS * 32), ("counts", k, SV_KINDS)):
            if str(t.dtype) != "torch.uint8" or tuple(t.shape) != (n, width) or not t.is_contiguous() or str(t.device) != dev:
                raise ValueError(f"sv_events: {name}: a contiguous uint8[{n}, {width}] tensor on {dev} is expected")
        self._check(self._L.pg_device_batch_sv_events_device(self._h, dbatch, c.data_ptr() if n else None, k.data_ptr() if n else None))
        nm, ne, dropped = self.sv_event_sizes(dbatch)
        out = dict(members=torch.empty(sum(nm), dtype=torch.int32, device=dev), events=torch.empty((sum(ne), 40), dtype=torch.uint8, device=dev))
        self._check(self._L.pg_device_batch_sv_events_download_device(self._h, dbatch, out["members"].data_ptr() if sum(nm) else None,
                                                                      out["events"].data_ptr() if sum(ne) else None))
        out.update(n_members=nm, n_events=ne, dropped_runs=dropped)
        return out

    def report_sizes(self, dbatch):
        """pg_device_batch_report_sizes: (report records, reads) of the records built last."""
        sz = ReportSizes()
        self._check(self._L.pg_device_batch_report_sizes(self._h, dbatch, C.addressof(sz)))
        return int(sz.records), int(sz.reads)

    def report_download(self, dbatch):
        """pg_device_batch_report_download: (records, summaries) -- REPORT_READ_DTYPE per member of the seven member lists in order
        (tables 0..3 of the events build, then SV tables 0..2), REPORT_SUMMARY_DTYPE per read."""
        nr, n = self.report_sizes(dbatch)
        records = np.zeros(nr, dtype=REPORT_READ_DTYPE)
        summaries = np.zeros(n, dtype=REPORT_SUMMARY_DTYPE)
        self._check(self._L.pg_device_batch_report_download(self._h, dbatch, records.ctypes.data if nr else None,
                                                            summaries.ctypes.data if n else None))
        return records, summaries

    def report_reads(self, dbatch, variant, sv):
        """Report records of a batch that holds an events build and an sv events build (pg_device_batch_report_reads):
        per table member the pair its read's record names, the carried NT_size and the few point-derived values the report writers
        need; per read a summary of its close and far end.  variant / sv: the (cands, counts) pairs the two builds were given.
        Returns report_download(dbatch)."""
        n = self._batch_n[dbatch.value]
        vc = np.ascontiguousarray(variant[0], dtype=VARIANT_CAND_DTYPE)
        vn = np.ascontiguousarray(variant[1], dtype=np.uint8)
        sc = np.ascontiguousarray(sv[0], dtype=VARIANT_CAND_DTYPE)
        sn = np.ascontiguousarray(sv[1], dtype=np.uint8)
        if vc.size != n * 2 * VARIANT_CANDS or vn.size != n * 2 or sc.size != n * SV_SLOTS or sn.size != n * SV_KINDS:
            raise ValueError(f"report_reads: lists of another size than {n} reads give")
        self._check(self._L.pg_device_batch_report_reads(self._h, dbatch, vc.ctypes.data if n else None, vn.ctypes.data if n else None,
                                                         sc.ctypes.data if n else None, sn.ctypes.data if n else None))
        return self.report_download(dbatch)

    def report_tensors(self, dbatch):
        """report_download into tensors on this engine's device (pg_device_batch_report_download_device): records uint8[total, 48],
        summaries uint8[n, 12]."""
        torch, dev = self._torch_ready()
        nr, n = self.report_sizes(dbatch)
        out = dict(records=torch.empty((nr, 48), dtype=torch.uint8, device=dev), summaries=torch.empty((n, 12), dtype=torch.uint8, device=dev))
        self._check(self._L.pg_device_batch_report_download_device(self._h, dbatch, out["records"].data_ptr() if nr else None,
                                                                   out["summaries"].data_ptr() if n else None))
        return out

    def report_reads_tensors(self, dbatch, variant, sv):
        """report_reads with everything staying on the GPU (pg_device_batch_report_reads_device and its download sibling): variant /
        sv are the dicts variant_candidates_tensors / sv_candidates_tensors return (or (cands, counts) tensor pairs).  Returns
        report_tensors(dbatch)."""
        _, dev = self._torch_ready()
        n = self._batch_n[dbatch.value]
        ptrs = []
        for x, widths in ((variant, (2 * VARIANT_CANDS * 32, 2)), (sv, (SV_SLOTS * 32, SV_KINDS))):
            c, k = (x["cands"], x["counts"]) if isinstance(x, dict) else x
            for name, t, width in (("cands", c, widths[0]), ("counts", k, widths[1])):
                if str(t.dtype) != "torch.uint8" or tuple(t.shape) != (n, width) or not t.is_contiguous() or str(t.device) != dev:
                    raise ValueError(f"report_reads: {name}: a contiguous uint8[{n}, {width}] tensor on {dev} is expected")
                ptrs.append(t.data_ptr() if n else None)
        self._check(self._L.pg_device_batch_report_reads_device(self._h, dbatch, *ptrs))
        return self.report_tensors(dbatch)

    def classify(self, dbatch, window, settings=None, max_listed=VARIANT_CANDS, name_id=None):
        """One call per window on a searched device batch (pg_device_batch_classify): both candidate kernels, the events build, the
        sv events build and the report records; the candidate lists stay on the GPU.  window: see event_window(); settings: see
        sv_params(); max_listed: lists longer than this are cut and marked VARIANT_MORE; name_id: None or uint32 per read.
        The tables and records are then delivered by events_download / sv_events_download / report_download."""
        n = self._batch_n[dbatch.value]
        prm = ClassifyParams(event_window(window), sv_params(settings), int(max_listed), 0)
        nid = None
        if name_id is not None:
            nid = np.ascontiguousarray(name_id, dtype=np.uint32)
            if nid.size != n:
                raise ValueError(f"classify: name_id: {n} entries are expected, got {nid.size}")
        self._check(self._L.pg_device_batch_classify(self._h, dbatch, C.addressof(prm), nid.ctypes.data if nid is not None and n else None))

    def li_sizes(self, dbatch):
        """pg_device_batch_li_sizes: (members per strand, positions per strand) of the long-insertion tables built last."""
        sz = LiSizes()
        self._check(self._L.pg_device_batch_li_sizes(self._h, dbatch, C.addressof(sz)))
        return [int(x) for x in sz.members], [int(x) for x in sz.positions]

    def li_download(self, dbatch):
        """The long-insertion tables the batch holds (pg_device_batch_li_download) as a dict: members and positions, lists of two
        arrays (uint32 read indices, LI_POS_DTYPE) for the '+' and the '-' anchors; members_flat / positions_flat (back to back)."""
        nm, npos = self.li_sizes(dbatch)
        members = np.zeros(sum(nm), dtype=np.uint32)
        positions = np.zeros(sum(npos), dtype=LI_POS_DTYPE)
        self._check(self._L.pg_device_batch_li_download(self._h, dbatch, members.ctypes.data if members.size else None,
                                                        positions.ctypes.data if positions.size else None))
        return _li_tables(members, positions, nm, npos)

    def _li_build(self, dbatch, lo, hi):
        if not (0 <= int(lo) < 2 ** 32 and 0 <= int(hi) < 2 ** 32):
            raise ValueError("li: lo and hi are uint32 positions")
        w = LiWindow(int(lo), int(hi))
        self._check(self._L.pg_device_batch_li(self._h, dbatch, C.addressof(w)))

    def li(self, dbatch, lo, hi):
        """Long-insertion position tables of a batch that holds an events build (pg_device_batch_li): per anchor
        strand the reads with a close end and no far end that the events build left unused, sorted by the position of their last
        close point clamped into [lo, hi], and one LI_POS_DTYPE record per distinct position.  Returns li_download(dbatch)."""
        self._li_build(dbatch, lo, hi)
        return self.li_download(dbatch)

    def li_tensors(self, dbatch, lo, hi):
        """li with the tables staying on the GPU (pg_device_batch_li_download_device): a dict of tensors on this engine's device,
        members int32[total], positions uint8[total, 16], plus n_members / n_positions (lists of two)."""
        torch, dev = self._torch_ready()
        self._li_build(dbatch, lo, hi)
        nm, npos = self.li_sizes(dbatch)
        out = dict(members=torch.empty(sum(nm), dtype=torch.int32, device=dev), positions=torch.empty((sum(npos), 16), dtype=torch.uint8, device=dev))
        self._check(self._L.pg_device_batch_li_download_device(self._h, dbatch, out["members"].data_ptr() if sum(nm) else None,
                                                               out["positions"].data_ptr() if sum(npos) else None))
        out.update(n_members=nm, n_positions=npos)
        return out

    def int_sizes(self, dbatch):
        """pg_device_batch_int_sizes: (members, calls) of the junction tables built last."""
        sz = IntSizes()
        self._check(self._L.pg_device_batch_int_sizes(self._h, dbatch, C.addressof(sz)))
        return int(sz.members), int(sz.calls)

    def int_download(self, dbatch):
        """The junction tables the batch holds (pg_device_batch_int_download) as a dict: members (uint32 read indices sorted by their
        call's key) and calls (INT_CALL_DTYPE, one per distinct key)."""
        nm, nc = self.int_sizes(dbatch)
        members = np.zeros(nm, dtype=np.uint32)
        calls = np.zeros(nc, dtype=INT_CALL_DTYPE)
        self._check(self._L.pg_device_batch_int_download(self._h, dbatch, members.ctypes.data if nm else None, calls.ctypes.data if nc else None))
        return dict(members=members, calls=calls)

    def chr_ranks(self):
        """The chr_rank of pg_int_window for the loaded reference: per chromosome the rank of its name in string order."""
        names = [self._L.pg_reference_name(self._h, c) for c in range(self._L.pg_reference_n_chr(self._h))]
        order = sorted(set(names))
        return np.array([order.index(n) for n in names], dtype=np.int32)

    def _int_build(self, dbatch, chr_rank):
        rank = np.ascontiguousarray(self.chr_ranks() if chr_rank is None else chr_rank, dtype=np.int32)
        w = IntWindow(rank.ctypes.data if rank.size else None, int(rank.size))
        self._check(self._L.pg_device_batch_int(self._h, dbatch, C.addressof(w)))

    def int_calls(self, dbatch, chr_rank=None):
        """Interchromosomal junction tables of a searched batch (pg_device_batch_int): the reads whose far end lies on
        another chromosome and whose points carry a call, sorted by the call's key, and one INT_CALL_DTYPE record per distinct key.
        chr_rank: int32 per chromosome of the reference (None: chr_ranks()).  Returns int_download(dbatch)."""
        self._int_build(dbatch, chr_rank)
        return self.int_download(dbatch)

    def int_tensors(self, dbatch, chr_rank=None):
        """int_calls with the tables staying on the GPU (pg_device_batch_int_download_device): a dict of tensors on this engine's
        device, members int32[n_members], calls uint8[n_calls, 32], plus n_members / n_calls."""
        torch, dev = self._torch_ready()
        self._int_build(dbatch, chr_rank)
        nm, nc = self.int_sizes(dbatch)
        out = dict(members=torch.empty(nm, dtype=torch.int32, device=dev), calls=torch.empty((nc, 32), dtype=torch.uint8, device=dev))
        self._check(self._L.pg_device_batch_int_download_device(self._h, dbatch, out["members"].data_ptr() if nm else None,
                                                                out["calls"].data_ptr() if nc else None))
        out.update(n_members=nm, n_calls=nc)
        return out

    def dd_sizes(self, dbatch):
        """pg_device_batch_dd_sizes: (members, cands, cons_bytes) of the DD tables built last."""
        sz = DdSizes()
        self._check(self._L.pg_device_batch_dd_sizes(self._h, dbatch, C.addressof(sz)))
        return int(sz.members), int(sz.cands), int(sz.cons_bytes)

    def dd_download(self, dbatch):
        """The DD tables the batch holds (pg_device_batch_dd_download) as a dict: members (DD_MEMBER_DTYPE, by (seg, pos), ascending read
        index within a key), cands (DD_CAND_DTYPE, one per candidate) and cons (the consensus pool, bytes)."""
        nm, nc, nb = self.dd_sizes(dbatch)
        members = np.zeros(nm, dtype=DD_MEMBER_DTYPE)
        cands = np.zeros(nc, dtype=DD_CAND_DTYPE)
        cons = np.zeros(nb, dtype=np.uint8)
        self._check(self._L.pg_device_batch_dd_download(self._h, dbatch, members.ctypes.data if nm else None, cands.ctypes.data if nc else None,
                                                        cons.ctypes.data if nb else None))
        return dict(members=members, cands=cands, cons=cons.tobytes())

    def _dd_build(self, dbatch, seg_first, seg_strand, chr_id, min_bp_support, min_map_distance):
        first = np.ascontiguousarray(seg_first, dtype=np.uint32)
        strand = np.frombuffer(seg_strand.encode() if isinstance(seg_strand, str) else bytes(seg_strand), dtype=np.uint8)
        n_seg = int(strand.size)
        assert first.size == (n_seg + 1 if n_seg else first.size), "seg_first has n_seg + 1 entries"
        w = DdWindow(first.ctypes.data if first.size else None, strand.ctypes.data if n_seg else None, n_seg, int(chr_id),
                     int(min_bp_support), int(min_map_distance))
        self._check(self._L.pg_device_batch_dd(self._h, dbatch, C.addressof(w)))

    def dd_tables(self, dbatch, seg_first, seg_strand, chr_id, min_bp_support=3, min_map_distance=8000):
        """Dispersed-duplication breakpoint tables of a close-searched batch (pg_device_batch_dd).  seg_first: n_seg + 1
        read indices; seg_strand: n_seg bytes '+' / '-' (str or bytes); chr_id: the window's chromosome.  Returns dd_download(dbatch)."""
        self._dd_build(dbatch, seg_first, seg_strand, chr_id, min_bp_support, min_map_distance)
        return self.dd_download(dbatch)

    def dd_tensors(self, dbatch, seg_first, seg_strand, chr_id, min_bp_support=3, min_map_distance=8000):
        """dd_tables with the tables staying on the GPU (pg_device_batch_dd_download_device): a dict of uint8 tensors on this engine's
        device, members [n_members, 8], cands [n_cands, 40], cons [cons_bytes], plus n_members / n_cands / cons_bytes."""
        torch, dev = self._torch_ready()
        self._dd_build(dbatch, seg_first, seg_strand, chr_id, min_bp_support, min_map_distance)
        nm, nc, nb = self.dd_sizes(dbatch)
        out = dict(members=torch.empty((nm, 8), dtype=torch.uint8, device=dev), cands=torch.empty((nc, 40), dtype=torch.uint8, device=dev),
                   cons=torch.empty(nb, dtype=torch.uint8, device=dev))
        self._check(self._L.pg_device_batch_dd_download_device(self._h, dbatch, out["members"].data_ptr() if nm else None,
                                                               out["cands"].data_ptr() if nc else None, out["cons"].data_ptr() if nb else None))
        out.update(n_members=nm, n_cands=nc, cons_bytes=nb)
        return out

    def events_download(self, dbatch):
        """The event tables the batch holds (pg_device_batch_event_sizes / _events_download) as the dict events() returns."""
        n = self._batch_n[dbatch.value]
        nm, ne, unresolved = self.event_sizes(dbatch)
        reads = np.zeros(n, dtype=EVENT_READ_DTYPE)
        members = np.zeros(sum(nm), dtype=np.uint32)
        events = np.zeros(sum(ne), dtype=EVENT_DTYPE)
        self._check(self._L.pg_device_batch_events_download(self._h, dbatch, reads.ctypes.data if n else None,
                                                            members.ctypes.data if members.size else None,
                                                            events.ctypes.data if events.size else None))
        return _event_tables(reads, members, events, nm, ne, unresolved)

    def sv_events_download(self, dbatch):
        """The SV tables the batch holds (pg_device_batch_sv_event_sizes / _sv_events_download) as the dict sv_events() returns."""
        nm, ne, dropped = self.sv_event_sizes(dbatch)
        members = np.zeros(sum(nm), dtype=np.uint32)
        events = np.zeros(sum(ne), dtype=EVENT_DTYPE)
        self._check(self._L.pg_device_batch_sv_events_download(self._h, dbatch, members.ctypes.data if members.size else None,
                                                               events.ctypes.data if events.size else None))
        return _sv_event_tables(members, events, nm, ne, dropped)

    def set_windows(self, dbatch, bd=None, bd_off=None):
        """Per-read BreakDancer window clusters for a device-resident batch (None detaches them)."""
        w, keep = _windows_struct(bd, bd_off)
        self._check(self._L.pg_device_batch_set_windows(self._h, dbatch, C.byref(w) if w is not None else None))

    def search_device(self, dbatch):
        self._check(self._L.pg_device_batch_search(self._h, dbatch))

    def pack_search_device(self, dbatch):
        """repack + search_device as one step (large batches: one launch, the search kernel packs its own reads)"""
        self._check(self._L.pg_device_batch_pack_search(self._h, dbatch))

    def search_table_device(self, dbatch, hints=None):
        """hints: a HintTable or None -- close end, lookup on the device and far end of a resident batch, both run lists left on
        the GPU (pg_device_batch_search_table); None: pack_search_device on the batch without windows"""
        t = hints.struct() if hints is not None else None
        self._check(self._L.pg_device_batch_search_table(self._h, dbatch, C.byref(t) if t is not None else None))

    def close_search(self, dbatch):
        """The close end alone of a resident batch (pg_device_batch_close_search): the batch ends close-searched -- what dd_tables
        needs -- and not searched: everything that needs both ends refuses it."""
        self._check(self._L.pg_device_batch_close_search(self._h, dbatch))

    def last_step_in_place(self) -> bool:
        """tests: did the last pack_search_device build its records inside the search kernel (one launch)?"""
        self._L.pg_debug_last_pack_in_place.argtypes = [C.c_void_p]
        return bool(self._L.pg_debug_last_pack_in_place(self._h))

    def last_fixed_len(self) -> int:
        """tests: the read length of the fixed-length kernel (pg_search_fixed_kernel) the last search launch ran; 0 when it ran
        any other kernel, or none yet"""
        self._L.pg_debug_last_fixed_len.argtypes = [C.c_void_p]
        self._L.pg_debug_last_fixed_len.restype = C.c_uint32
        return int(self._L.pg_debug_last_fixed_len(self._h))

    def launch_log(self):
        """tests: the kernels the search path launched since the last clear_launch_log, in launch order -- LaunchRec tuples
        (kernel 1 search / 2 exact / 3 pack, blocks = NB or PB, ns, id_bits, mode, default, in_place)."""
        L = self._L
        L.pg_debug_launch_log.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.pg_debug_launch_log.restype = C.c_int32
        n = L.pg_debug_launch_log(self._h, None, 0)
        self._check(min(n, 0))
        if n > LAUNCH_LOG_CAP:
            raise PgError(PG_E_DEVICE, f"launch log overflowed: {n} launches, room for {LAUNCH_LOG_CAP}")
        out = np.zeros((max(n, 1), 7), dtype=np.int32)
        L.pg_debug_launch_log(self._h, out.ctypes.data, n)
        return [LaunchRec(*map(int, r)) for r in out[:n]]

    def clear_launch_log(self):
        self._L.pg_debug_clear_launch_log.argtypes = [C.c_void_p]
        self._L.pg_debug_clear_launch_log.restype = None
        self._L.pg_debug_clear_launch_log(self._h)

    def scribble_records(self, dbatch):
        """tests: overwrite the packed records and planes of the batch"""
        self._L.pg_debug_scribble_records.argtypes = [C.c_void_p, C.c_void_p]
        self._check(self._L.pg_debug_scribble_records(self._h, dbatch))

    def repack(self, dbatch) -> float:
        """The pack stage (ASCII bases -> bit planes + packed records) again on the resident batch; HIP-event ms."""
        ms = C.c_double()
        self._check(self._L.pg_device_batch_repack(self._h, dbatch, C.byref(ms)))
        return ms.value

    def download(self, dbatch) -> Result:
        h = C.c_void_p()
        self._check(self._L.pg_device_batch_download(self._h, dbatch, C.byref(h)))
        return Result(h, self)

    def free_device_batch(self, dbatch):
        self._batch_n.pop(dbatch.value, None)
        self._L.pg_device_batch_free(self._h, dbatch)

    def last_stats(self):
        ms = C.c_double()
        runs = C.c_uint64()
        self._check(self._L.pg_last_search_stats(self._h, C.byref(ms), C.byref(runs)))
        return ms.value, runs.value

    def candidates(self, dbatch):
        """Diagnostics: seed-filter survivors folded by the last search of the batch."""
        n = C.c_double()
        self._check(self._L.pg_device_batch_candidates(self._h, dbatch, C.byref(n)))
        return n.value

    def algorithmic_bytes(self, dbatch):
        b = C.c_double()
        self._check(self._L.pg_device_batch_algorithmic_bytes(self._h, dbatch, C.byref(b)))
        return b.value
