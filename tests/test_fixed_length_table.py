"""CPU: the literal rows the fixed-length kernels are built from (PG_FIXED_LEN_ROWS, pg_device.h) are what the host computes for
Pindel's default parameters -- pg_len_rec() over the tables of pg_default_params -- read from the built library through
pg_debug_fixed_len_row (no device needed), and the library's code object holds one fixed-length kernel per row."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from pindel_amd import binding

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
FIELDS = ("lvl", "depth", "jmask0", "ro", "jmask1")


def _rows():
    binding.build()
    L = C.CDLL(binding.LIB_PATH)
    L.pg_debug_fixed_len_row.argtypes = [C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.pg_debug_fixed_len_row.restype = C.c_int
    n = L.pg_debug_fixed_len_row(-1, None, None, None)
    rows = []
    for k in range(n):
        ln, baked, host = C.c_uint32(), (C.c_uint32 * 5)(), (C.c_uint32 * 5)()
        assert L.pg_debug_fixed_len_row(k, C.byref(ln), baked, host) == n
        rows.append((int(ln.value), list(baked), list(host)))
    return rows


def test_baked_rows_equal_the_host_tables():
    rows = _rows()
    assert rows, "no fixed-length kernel built"
    from tests.test_gpu_fixed_length import BUILT
    assert [ln for ln, _, _ in rows] == BUILT          # (the lengths the GPU tests go through)
    for ln, baked, host in rows:
        assert dict(zip(FIELDS, baked)) == dict(zip(FIELDS, host)), f"{ln} bases"
        # the row is one the read-order filter takes, with the counter of up to eight mismatch levels (NS = 3)
        T = baked[0] >> 24
        assert 0 < T <= 8 and baked[3] & 0x80000000


def test_one_kernel_per_row(tmp_path):
    if not os.path.exists(OBJDUMP):
        pytest.skip("no llvm-objdump in this image")
    rows = _rows()
    lib = str(tmp_path / "lib.so")
    shutil.copy(binding.LIB_PATH, lib)
    subprocess.run([OBJDUMP, "--offloading", lib], cwd=tmp_path, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
    cos = [f for f in os.listdir(tmp_path) if "gfx950" in f]
    assert cos, "no gfx950 code object in the library"
    notes = subprocess.run([READELF, "--notes", str(tmp_path / cos[0])], stdout=subprocess.PIPE, text=True, check=True).stdout
    got = sorted(tuple(map(int, m.groups())) for m in re.finditer(r"\.name:\s+_Z22pg_search_fixed_kernelILi(\d+)ELi(\d+)ELi(\d+)EE", notes))
    # the block class of the length (32-bit ids) and three counter slices
    want = sorted(((ln + 63) // 64, 3, ln) for ln, _, _ in rows)
    assert got == want
