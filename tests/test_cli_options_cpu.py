"""CPU: the pindel_pg command line as data (pindel_amd/csrc/host/pg_cli.hpp) -- every row of the flag table, every quirk of the
parser, its error texts and repeated flags -- checked by a stand-alone host program (tests/cli_options_unit.cpp) built with
-fsanitize=address,undefined.  The header links against nothing: no host source, no libpindel_pg.so, no HIP.  No GPU, nothing
loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cli_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cli") / "cli_options_unit"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pindel_amd", "csrc", "host"),
                    os.path.join(ROOT, "tests", "cli_options_unit.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_cli_options(cli_program):
    """Every case of cli_options_unit.cpp.  Each row of CLI_FLAGS, by its short and its long spelling, changes its own field of a
    default CliOptions and no other (compared field by field), and the test's own table lists exactly the parser's rows.  The
    quirks: a switch's optional word (-R false / 0 / F against -R and -R yes), -q on whatever its word, "seems erroneous" for
    numeric flags only (-x -3 against -o -name), -w's smallest window (0.0000001 refused, 0.000001 taken), --flush-reads' clamp,
    --bd-hints ON is off, -e in both fields, -c and --repair checked while parsing, -T and PGH_THREADS, the -G lists 0,,1 / , /
    1, / a as the parent's binary took them.  The five error texts with status 2, and the last of a repeated flag.

    `--flush-reads -5`: the word starts with '-', so the flag, being numeric, refuses it as "seems erroneous" -- before and after
    this header existed (the parent's binary says the same).  The clamp to 0 is reached by what strtol reads past that check
    (" -5"), and that is what is pinned."""
    env = dict(os.environ)
    env.pop("PGH_THREADS", None)
    run = subprocess.run([cli_program], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]          # (the sanitizers report on stderr)
    word, cases = run.stdout.split()
    assert word == "ok" and int(cases) > 300
