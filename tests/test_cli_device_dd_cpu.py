"""CPU: the sixth flag table of pg_cli.hpp, CLI_DEVICE_DD_FLAGS (--device-classifier-dd), checked by a stand-alone
host program (tests/cli_device_dd_unit.cpp) built with -fsanitize=address,undefined.  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cli_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cli_device_dd") / "cli_device_dd_unit"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pindel_amd", "csrc", "host"),
                    os.path.join(ROOT, "tests", "cli_device_dd_unit.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_cli_device_dd_flag(cli_program):
    """The switch is parsed with its optional word and is off by default; with --device-classifier it admits -q, on both input routes,
    beside --device-classifier-hints, -li, -int and -listed and with -R false; without it (absent or false) -q's refusal keeps status 2
    and its text; alone it is refused, after the -int check; -l, -s and -I without their own switches, -S, -N and a -G list of several
    devices stay refused either way."""
    run = subprocess.run([cli_program], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]          # (the sanitizers report on stderr)
    word, cases = run.stdout.split()
    assert word == "ok" and int(cases) > 60
