"""The whole route on the MI355X: `pindel_pg -l` searches the gold reads on the GPU and writes the reports, then
`pindel_pg2vcf -P` converts them.  The VCF is byte for byte the text-route fixture (tests/golden/vcf/text_route.vcf.gz:
the reference converter's output for the gold reports as the text route writes them), with one device context and
with two (-G 0,0).  A step that fails ends the test before the next one starts."""
import gzip
import os
import subprocess

import pytest

from pindel_amd import binding, hostlib
from tests import golden_util as gu

FX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vcf")


def _run(args, timeout):
    out = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, f"{args[0]} exit {out.returncode}:\n{out.stdout[-3000:]}\n{out.stderr[-3000:]}"
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("gpus", [None, "0,0"], ids=["one_context", "G_0_0"])
def test_gpu_search_reports_to_vcf(tmp_path, gpus):
    binding.build()
    fa, reads_txt = gu.unpack(tmp_path)
    exe = os.path.join(os.path.dirname(binding.LIB_PATH), "pindel_pg")
    prefix = str(tmp_path / "P")
    _run([exe, "-f", fa, "-p", reads_txt, "-o", prefix, "-l", "-T", "1"] + (["-G", gpus] if gpus else []), timeout=600)
    _run([hostlib.vcf_cli(), "-P", prefix, "-r", fa, "-R", "SIMCHROM", "-d", "00000000"], timeout=120)
    got = open(prefix + ".vcf", "rb").read()
    assert got == gzip.open(os.path.join(FX, "text_route.vcf.gz")).read()
