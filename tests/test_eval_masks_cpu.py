"""CPU: the bit arithmetic of the short form of evaluate / emit_runs (pindel_amd/csrc/pg_eval_masks.h) against the naive definitions,
by a stand-alone host program (tests/eval_masks_unit.cpp) built with -fsanitize=address,undefined.  No GPU, nothing loaded into
Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def masks_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("evalmasks") / "eval_masks_unit"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "pindel_amd", "csrc"),
                    os.path.join(ROOT, "tests", "eval_masks_unit.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_eval_masks(masks_program):
    """Every lane 0-63, bps 8 and 10, every read length 11-499 and every round: the scalar mask of the valid lanes equals the ballot of
    "L <= len - 1"; the mask above a lane equals ~low_bits(lane + 1); and a valid lane that does not abort is a point with the compares
    "m1 <= M" and "L >= bps + m1" iff it is one with the round-wise rule alone, for every level 0-64 and every M 0-31 on monotone
    tables bounded by M (per lane exhaustively; on whole rounds with the first abort for a set of lengths and table shapes).  No shift
    in the header is undefined (the sanitizers report on stderr)."""
    run = subprocess.run([masks_program], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.stdout[-4000:], run.stderr[-4000:])
    word, cases = run.stdout.split()
    # vm: 2 bps x 489 lengths x 8 rounds; per lane: one comparison per valid (bps, len, round, lane), more than 2 x 489 x 64
    assert word == "ok" and int(cases) > 2 * 489 * 8 + 2 * 489 * 64
