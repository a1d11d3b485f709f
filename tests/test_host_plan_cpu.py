"""CPU: the plan of a host-path call (pindel_amd/csrc/pg_host_plan.h) -- chunk schedule, one-block layout, the delivery's arena
requests and the one-copy input layout -- checked by a stand-alone host program (tests/host_plan_unit.cpp) built with
-fsanitize=address,undefined.  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("plan") / "host_plan_unit"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pindel_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_plan_unit.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_host_plan(plan_program):
    """Every n x PG_HOST_CHUNK x PG_NO_SINGLE_BLOCK x PG_TEST_TINY_DELIVERY case of host_plan_unit.cpp: bounds from 0 to n and
    strictly increasing, no chunk above PG_DELIVER_CHUNK, the override honoured, one block exactly for one chunk; the takes fit
    the byte total from an unaligned arena offset without overlap; the block's parts are aligned and inside the block; the
    pinned schedules; the one-copy input span inside the room the plan reserves."""
    run = subprocess.run([plan_program], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]          # (the sanitizers report on stderr)
    word, cases = run.stdout.split()
    assert word == "ok" and int(cases) > 200


def test_the_plan_header_needs_no_hip(tmp_path):
    """pg_host_plan.h compiles on its own with plain g++ -std=c++17 (no HIP header on the include path)."""
    src = tmp_path / "only_plan.cpp"
    src.write_text('#include "pg_host_plan.h"\nint main() { return pg_host_plan(3, 0, false, false).n_chunks == 1 ? 0 : 1; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "pindel_amd", "csrc"), str(src), "-o", str(tmp_path / "only_plan")], check=True)
    assert subprocess.run([str(tmp_path / "only_plan")]).returncode == 0
