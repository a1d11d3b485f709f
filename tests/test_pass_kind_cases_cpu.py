"""The constructed reads of tests/pass_kind_cases.py on the CPU: the oracle's points show that every case reaches the situation the GPU
tests (tests/test_gpu_pass_kinds.py, tests/test_gpu_quarter_tree.py) mean it to."""
import pytest

from tests import pass_kind_cases as pkc
from tests.parity import run_oracle


@pytest.mark.parametrize("L", [100, 101])
@pytest.mark.parametrize("which", ["kinds", "quarters"])
def test_cases_reach_their_situations(L, which):
    chrom, cases = (pkc.build_kinds if which == "kinds" else pkc.build_quarters)(L)
    orc = run_oracle({}, [("chrC", chrom)], pkc.batch_of(cases))
    pkc.check_situations(L, cases, orc)
    assert len({c.name for c in cases}) == len(cases) == (60 if which == "kinds" else 62)
