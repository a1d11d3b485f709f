"""CPU: the fold's per-candidate step (pindel_amd/csrc/pg_fold_step.h) in its short form against the definitions the kernels had
before it, by a stand-alone host program (tests/fold_step_unit.cpp) built with -fsanitize=address,undefined.  No GPU, nothing
loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fold_step_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("foldstep") / "fold_step_unit"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "pindel_amd", "csrc"),
                    os.path.join(ROOT, "tests", "fold_step_unit.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_fold_step(fold_step_program):
    """Random and adversarial candidate streams (the empty state, a clean window with a failed Hamming count, a dirty window with a
    passed one, ties in every quarter order, levels at PG_BIG, m2 at AccB's 0x7fff clip) through the tier A step, the tier B verdict,
    the merge and the AccB round trip: identical (m1, m2, id) and ok == (nok == 0) after each; tier A passes of every size 0 .. 64
    walked with and without the validity test in the full iterations; CheckMismatches' window holds a base on every lane of both
    ends.  The sanitizers report on stderr."""
    run = subprocess.run([fold_step_program], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.stdout[-4000:], run.stderr[-4000:])
    word, cases = run.stdout.split()
    # 400 streams x 40 candidates x 6 comparisons, 24 orders x 16 verdict patterns x 2 x 7, 65 x 4 passes x 7
    assert word == "ok" and int(cases) > 400 * 40 * 6 + 24 * 16 * 2 * 7 + 65 * 4 * 7
