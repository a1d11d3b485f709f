"""CPU: the preparation of BreakDancer windows (pindel_amd/csrc/pg_window_plan.h) -- validation and its order, long windows cut
into pieces, groups, the two limits -- checked by a stand-alone host program (tests/window_plan_unit.cpp) built with
-fsanitize=address,undefined.  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("windows") / "window_plan_unit"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pindel_amd", "csrc"),
                    os.path.join(ROOT, "tests", "window_plan_unit.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_window_plan(plan_program):
    """Every case of window_plan_unit.cpp, with piece = 2^26 - 1: windows of 1, piece - 1, piece, piece + 1, 2 piece, 2 piece + 1
    and 2^31 - 65536 positions come back as ceil(width / piece) pieces that tile [start, end) in order, none longer than a piece,
    and a window that fits comes back as it is, uncopied, a negative start included; a window with end <= start passes through
    and counts 0; empty groups, a first offset other than 0 and a long window inside a group give offsets that are the prefix
    sums of the piece counts, the largest group and each group's longest window as counted directly; non-monotone offsets, a
    null array with windows, chr_id -1 and chr_id n_chr are refused, offsets first; the limits hold at 2^32 and 2^29."""
    run = subprocess.run([plan_program], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]          # (the sanitizers report on stderr)
    word, cases = run.stdout.split()
    assert word == "ok" and int(cases) > 50


def test_the_window_plan_header_needs_no_hip(tmp_path):
    """pg_window_plan.h compiles on its own with plain g++ -std=c++17 (no HIP header on the include path)."""
    src = tmp_path / "only_windows.cpp"
    src.write_text('#include "pg_window_plan.h"\n'
                   'int main() { const pg_window w = { 0, 0, 1 << 27 }; const uint64_t off[2] = { 0, 1 };\n'
                   '             return pg_window_plan(off, 1, &w, 1, false, nullptr).win.size() == 3 ? 0 : 1; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "pindel_amd", "csrc"), str(src), "-o", str(tmp_path / "only_windows")], check=True)
    assert subprocess.run([str(tmp_path / "only_windows")]).returncode == 0
