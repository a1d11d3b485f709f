"""CPU: what window hints on the device-resident path add above the kernels -- the entry pg_device_batch_search_table
in the header, the library and the binding, and the switch --device-classifier-hints of pg_cli.hpp, checked by a stand-alone host
program (tests/cli_device_hints_unit.cpp) built with -fsanitize=address,undefined.  No GPU, nothing sanitized loaded into Python."""
import ctypes
import os
import subprocess

import pytest

from pindel_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pindel_pg.h")).read()
    binding.build()
    lib = ctypes.CDLL(binding.LIB_PATH)
    sym = "pg_device_batch_search_table"
    assert f"{sym}(pg_ctx *ctx, pg_device_batch *b, const pg_hint_table *table" in hdr
    assert sym in binding.EXPORTS and hasattr(lib, sym)
    assert callable(getattr(binding.Engine, "search_table_device"))
    with open(binding.LIB_PATH, "rb") as f:
        assert b"pg_unpack_close_kernel" in f.read()


@pytest.fixture(scope="module")
def cli_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cli_device_hints") / "cli_device_hints_unit"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pindel_amd", "csrc", "host"),
                    os.path.join(ROOT, "tests", "cli_device_hints_unit.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_cli_device_classifier_hints(cli_program):
    """The switch is parsed with and without its word; with it --device-classifier goes together with --bd-hints on and with BAM
    input while -R is on; without it both keep status 2 and their texts; alone it is status 2 and names --device-classifier; -I,
    -l, -s, -S, -q, -N and a -G list of two devices stay refused with it."""
    run = subprocess.run([cli_program], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]          # (the sanitizers report on stderr)
    word, cases = run.stdout.split()
    assert word == "ok" and int(cases) > 60
