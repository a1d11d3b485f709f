"""The entries of the device classifier of the five other kinds: declared in the public header, exported by both
libraries, bound in Python, and the kernel is in the shipped code object.  No GPU needed."""
import ctypes
import os

from pindel_amd import binding, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pindel_pg.h")).read()
    binding.build()
    lib = ctypes.CDLL(binding.LIB_PATH)
    for sym in ("pg_device_batch_sv_candidates", "pg_device_batch_sv_candidates_device"):
        assert f"{sym}(" in hdr and sym in binding.EXPORTS and hasattr(lib, sym), sym
    host = hostlib.lib()
    for sym in ("pgh_sv_candidates", "pgh_call_from_points_lists", "pgh_call_from_points_candidates", "pgh_variant_candidates"):
        assert hasattr(host, sym), sym
    for name in ("sv_candidates", "sv_candidates_into", "sv_candidates_tensors"):
        assert callable(getattr(binding.Engine, name))
    assert hostlib.SV_KINDS == {2: "DI", 3: "TD", 4: "TD_NT", 5: "INV", 6: "INV_NT"}


def test_layout_constants_agree_with_the_header():
    hdr = open(os.path.join(ROOT, "include", "pindel_pg.h")).read()
    assert "#define PG_SV_KINDS 5" in hdr and "#define PG_SV_SLOTS 11" in hdr and "#define PG_SV_GEO_SHIFT 4" in hdr
    assert "PG_SV_DI = 2, PG_SV_TD = 3, PG_SV_TD_NT = 4, PG_SV_INV = 5, PG_SV_INV_NT = 6" in hdr
    assert binding.SV_KINDS == 5 and binding.SV_SLOTS == 11 == hostlib.SV_SLOTS and binding.SV_GEO_SHIFT == 4 == hostlib.SV_GEO_SHIFT
    assert binding.SV_SLOT == {2: 0, 3: 1, 4: 5, 5: 6, 6: 10} == hostlib.SV_SLOT
    assert binding.SV_COUNT == {2: 0, 3: 1, 4: 2, 5: 3, 6: 4}
    assert binding.SV_SLOTS * binding.VARIANT_CAND_DTYPE.itemsize == 352
    assert ctypes.sizeof(binding.SvParams) == 16 == ctypes.sizeof(hostlib.SvParams)
    p = binding.sv_params(hostlib.default_settings([0] * 500))
    assert (p.seq_error_rate, p.min_num_matched_bases, p.min_inversion_size) == (0.01, 30, 50)
    d = binding.sv_params(None)
    assert (d.seq_error_rate, d.min_num_matched_bases, d.min_inversion_size) == (0.01, 30, 50)


def test_library_holds_the_kernel():
    binding.build()
    with open(binding.LIB_PATH, "rb") as f:
        blob = f.read()
    assert b"pg_sv_kernel" in blob and b"pg_variant_kernel" in blob
