"""CPU: the second flag table of pg_cli.hpp, CLI_DEVICE_FLAGS (--device-classifier, --device-classifier-listed),
checked by a stand-alone host program (tests/cli_device_flags_unit.cpp) built with -fsanitize=address,undefined.  No GPU, nothing
loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cli_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cli_device") / "cli_device_flags_unit"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pindel_amd", "csrc", "host"),
                    os.path.join(ROOT, "tests", "cli_device_flags_unit.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_cli_device_flags(cli_program):
    """Both flags are parsed (the switch with its optional word, the number 0..4), the defaults stay untouched otherwise, and every
    refusal the parser alone can decide gives status 2 and a text that names the flag: --device-classifier-listed without the
    switch or outside 0..4; the switch with -l, -s, -S, -I, -q or -N, with --bd-hints on, with BAM input and -R on, with a -G list
    of more than one device."""
    run = subprocess.run([cli_program], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]          # (the sanitizers report on stderr)
    word, cases = run.stdout.split()
    assert word == "ok" and int(cases) > 60
