"""CPU: the record-shift form of the strict exchange sort (pindel_amd/csrc/pg_sv_order.h) against the literal
loop of the reference's DI and inversion reporters, by a stand-alone host program (tests/sv_order_unit.cpp) built with
-fsanitize=address,undefined.  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sv_order_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("svorder") / "sv_order_unit"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "pindel_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sv_order_unit.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_sv_order(sv_order_program):
    """Every 3-valued sequence of length 0 .. 7 (3280), 3 000 random ones of up to 200 elements (two to four values, up to forty,
    all different, nearly sorted; the chunk seams at 64 and 128) and the two examples whose tie order depends on history: the same
    permutation as the literal loop, and the skip of a pass with a minimal front taken at least once.  The sanitizers report on
    stderr."""
    run = subprocess.run([sv_order_program], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.stdout[-4000:], run.stderr[-4000:])
    word, cases = run.stdout.split()
    assert word == "ok" and int(cases) == 3280 + 3000 + 2
