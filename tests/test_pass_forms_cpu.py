"""CPU: the two forms of a candidate's block and of evaluate's quarter merge (pindel_amd/csrc/pg_pass_forms.h) side by side, by two
stand-alone host programs (tests/pass_rev_unit.cpp, tests/quarter_tree_unit.cpp) built with -fsanitize=address,undefined.  No GPU,
nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path_factory, name):
    exe = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "pindel_amd", "csrc"),
                    os.path.join(ROOT, "tests", name + ".cpp"), "-o", str(exe)], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def pass_rev_program(tmp_path_factory):
    return _build(tmp_path_factory, "pass_rev_unit")


@pytest.fixture(scope="module")
def quarter_tree_program(tmp_path_factory):
    return _build(tmp_path_factory, "quarter_tree_unit")


def test_block_forms(pass_rev_program):
    """Reference words reversed against mismatch word reversed, and both against Matches() base by base: 4000 random word sets (read
    N, reference N and "other" characters at bit 0, bit 63 and inside) x complement x kind x 1, 36, 37, 63, 64 bases in the block; the
    mismatch word and the exact inequality word equal bit for bit.  The sanitizers report on stderr."""
    run = subprocess.run([pass_rev_program], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.stdout[-4000:], run.stderr[-4000:])
    assert run.stdout.strip() == "pass_rev_unit: %d cases, 0 bad" % (4000 * 2 * 2 * 5)


def test_quarter_tree(quarter_tree_program):
    """The chain against the tree for qmask 1, 3 and 15 over every state of four quarters with levels m1 <= m2 out of {0, 1, 2, 3,
    PG_FS_BIG}, distinct ids and both verdict words: the two levels, the argmin (the leftmost quarter of the lowest level) and its
    verdict word."""
    run = subprocess.run([quarter_tree_program], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.stdout[-4000:], run.stderr[-4000:])
    assert run.stdout.strip() == "quarter_tree_unit: %d cases, 0 bad" % (30 ** 4 * 3)
