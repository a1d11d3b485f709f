"""CPU: the fold's per-lane mask builders (pindel_amd/csrc/pg_lane_masks.h) against the naive definitions, by a stand-alone host
program (tests/lane_masks_unit.cpp) built with -fsanitize=address,undefined.  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def masks_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("masks") / "lane_masks_unit"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "pindel_amd", "csrc"),
                    os.path.join(ROOT, "tests", "lane_masks_unit.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_lane_masks(masks_program):
    """Every lane 0-63; bps 8 and 10 with min_perfect 3; every (bps, min_perfect) with 0 <= min_perfect <= bps <= 64; every round
    and block of NB = 2 and NB = 3; tier A's 16 lengths for every bps it is used with: the header's masks equal low_bits of the
    clamped arguments, and no shift in them is undefined (the sanitizers report on stderr)."""
    run = subprocess.run([masks_program], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.stdout[-4000:], run.stderr[-4000:])
    word, cases = run.stdout.split()
    # 64 lanes x (4 + 9) round / block pairs x 2 masks per (bps, min_perfect) pair, 2 080 pairs with min_perfect >= 1
    assert word == "ok" and int(cases) > 64 * 13 * 2 * 2080
