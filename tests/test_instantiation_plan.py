"""The instantiation plan (tests/instantiations.py) on the CPU: the kernels of the built library's gfx950 code object are
exactly the plan's, the plan's cases reach every one of them through the mirror of the dispatch rules, and every case lands
on the levels, block class and id width it names."""
import os
import shutil
import subprocess

import pytest

from oracle import pyoracle
from pindel_amd import binding
from tests import instantiations as I

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def _code_object_kernels(tmp_path):
    """(kernel keys, unparsed names) of the search / exact / pack kernels in the library's gfx950 code object"""
    if not os.path.exists(OBJDUMP):
        pytest.skip("no llvm-objdump in this image")
    binding.build()
    lib = str(tmp_path / "lib.so")
    shutil.copy(binding.LIB_PATH, lib)
    subprocess.run([OBJDUMP, "--offloading", lib], cwd=tmp_path, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
    cos = [f for f in os.listdir(tmp_path) if "gfx950" in f]
    assert cos, "no gfx950 code object in the library"
    notes = subprocess.run([READELF, "--notes", str(tmp_path / cos[0])], stdout=subprocess.PIPE, text=True, check=True).stdout
    names = {ln.split(":", 1)[1].strip() for ln in notes.splitlines() if ln.strip().startswith(".name:")}
    names = {n for n in names if any(k in n for k in ("pg_search_kernel", "pg_search_exact_kernel", "pg_pack_kernel"))}
    keys = {n: I.kernel_from_symbol(n) for n in names}
    return {k for k in keys.values() if k}, sorted(n for n, k in keys.items() if k is None)


def test_code_object_kernels_equal_the_plan(tmp_path):
    got, unparsed = _code_object_kernels(tmp_path)
    assert not unparsed, f"kernels the plan cannot name: {unparsed}"
    missing = sorted(I.kernel_name(k) for k in I.ALL_KERNELS - got)
    extra = sorted(I.kernel_name(k) for k in got - I.ALL_KERNELS)
    assert not missing and not extra, f"not in the library: {missing}; not in the plan: {extra}"
    assert len(I.ALL_KERNELS) == 110
    assert sum(k[0] == I.SEARCH for k in I.ALL_KERNELS) == 102


def test_cases_cover_every_kernel():
    covered = set()
    for c in I.CASES:
        for recs in I.case_launches(c, 400).values():
            covered |= {I.kernel_of(r) for r in recs}
    missing = sorted(I.kernel_name(k) for k in I.ALL_KERNELS - covered)
    assert not missing, f"no case launches {missing}"
    assert covered <= I.ALL_KERNELS


def test_one_low_and_one_high_case_per_cell():
    cells = {}
    for c in I.CASES:
        if not c.id.endswith("-127win"):
            cells.setdefault((c.nb, c.id_bits, c.ns, c.default), []).append(c.edge)
    assert len(cells) == 34 and all(sorted(v) == ["high", "low"] for v in cells.values())
    assert len({c.id for c in I.CASES}) == len(I.CASES)


@pytest.mark.parametrize("case", I.CASES, ids=[c.id for c in I.CASES])
def test_case_lands_on_its_cell(case):
    p = case.params
    t = pyoracle.max_mismatch_table(p.get("seq_error_rate", 0.01), p.get("sensitivity", 0.95))
    a = max(1, p.get("additional_mismatch", 1))
    levels = int(t[:case.longest + 1].max()) + a + 1
    assert levels == case.levels == I.levels_of(case.longest, **p) == I.LEVEL_TARGET[(case.ns, case.edge)]
    assert I.counter_slices(levels) == case.ns
    assert case.longest == I.LONGEST[(case.id_bits, I.class_blocks(case.longest, case.id_bits == 32))][case.edge == "high"] \
        or case.id.endswith("-127win")
    # the longest read is the first / the last length of its block class
    lo, hi = {1: (1, 64), 2: (65, 128), 3: (129, 192), 4: (193, 256), 8: (257, 499)}[case.nb] if case.id_bits == 32 else \
        {2: (1, 128), 4: (129, 256), 8: (257, 499)}[case.nb]
    assert lo <= case.longest <= hi and (case.longest == hi) == (case.edge == "high")
    # shorter reads at 0, 1 and 63 (mod 64) where those are long enough to split
    assert all(x % 64 in (0, 1, 63) for x in case.lengths[1:]) and max(case.lengths) == case.longest
    assert len(case.lengths) >= (3 if case.longest > 192 else 1)
    # the id width on every path
    for path in I.PATHS:
        small = case.small_ids_on(path)
        wide_here = case.wide == "force" or (case.wide == "windows" and I.PATH_WINDOWS[path])
        assert small == (not wide_here)
        if not small or case.id_bits == 32:
            assert I.class_blocks(case.longest, small) == case.nb
        recs = case.expected(path, 400)
        search = [r for r in recs if r[0] == I.SEARCH]
        assert search and all(r[2] == case.ns for r in search)
        if case.id_bits == 32 or wide_here:
            assert all(r[1] == case.nb and r[3] == case.id_bits and r[5] == int(case.default) for r in search), (path, recs)
    if case.wide == "windows":
        assert case.windows == I.SMALL_MAX_CLUSTER + 1
    if case.id.endswith("-127win"):
        assert case.windows == I.SMALL_MAX_CLUSTER and case.id_bits == 32
    # the parameters: the defaults exactly for the DEF cells
    assert I.is_default(p) == case.default or not case.default and (case.generic_switch or case.ns == 5 or case.id_bits == 64)
    # what the GPU test asserts about the points must be possible under the reference's rules
    admitted = int(t[case.longest])
    assert I.top_slice_needed(case) in (None, I.TOP_SLICE[case.ns]) and (I.top_slice_needed(case) or 0) <= admitted
    assert I.MM_REACH[case.id] <= admitted


def test_mirror_of_the_dispatch_rules():
    """a few launches written out by hand"""
    # the headline: 100-base reads, defaults, fused, packed in place
    assert I.expected_launches(100, 7, True, True, I.BOTH, 50_000) == [(1, 2, 3, 32, 3, 1, 1), (2, 0, 0, 0, 3, 0, 0)]
    # 150-base reads with 64-bit ids: the kernel has 4 blocks, the planes 3 -> a pack launch of its own
    assert I.expected_launches(150, 7, False, True, I.BOTH, 10) == [(3, 3, 0, 0, 0, 0, 0), (1, 4, 3, 64, 3, 0, 0),
                                                                    (2, 0, 0, 0, 3, 0, 0)]
    # split launches never pack in place
    assert I.expected_launches(64, 9, True, False, I.BOTH, 10, split=True) == [(3, 1, 0, 0, 0, 0, 0), (1, 1, 4, 32, 1, 0, 0),
                                                                              (1, 1, 4, 32, 2, 0, 0), (2, 0, 0, 0, 3, 0, 0)]
    assert not I.pack_in_place_ok(I.FAR, 100, True, 5, pack_in_place_min=6)
    assert [I.plane_blocks(x) for x in (64, 65, 128, 129, 192, 193, 256, 257, 499)] == [1, 2, 2, 3, 3, 4, 4, 8, 8]
    assert [I.class_blocks(x, False) for x in (36, 128, 129, 256, 257)] == [2, 2, 4, 4, 8]
    assert [I.counter_slices(x) for x in (8, 9, 16, 17, 32)] == [3, 4, 4, 5, 5]
    assert not I.small_ids(max_range_index=9) and not I.small_ids(max_cluster=128) and I.small_ids(max_cluster=127)
    assert not I.is_default(dict(min_close=9)) and I.is_default(dict(additional_mismatch=0, seq_error_rate=0.05))
