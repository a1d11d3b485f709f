"""The constructed reads of tests/pass_idle_cases.py on the CPU: the oracle accepts them, and the planted copies are the only positions
that resemble the bases a seed filter looks at -- so the candidate counts tests/test_gpu_pass_idle_lanes.py asserts on the GPU are the
intended ones."""
import numpy as np
import pytest

from tests import pass_idle_cases as pic
from tests.parity import run_oracle


@pytest.mark.parametrize("L", [100, 150])
def test_planted_counts_and_oracle(L):
    chrom, cases = pic.build(L)
    P = pic.pass_size(L)
    orc = run_oracle({}, [("chrN", chrom)], pic.batch_of(cases))
    by_name = {c.name: i for i, c in enumerate(cases)}
    for i, c in enumerate(cases):
        assert pic.check_planted(chrom, c) == c.expect, c.name
        if c.name.startswith("close"):
            # no far end (the read begins with N); a close end at attempt 0 unless nothing is planted
            assert orc["far_cnt"][i] == 0
            assert (orc["close_cnt"][i] > 0) == (c.expect > 0) and orc["rc_flag"][i] == 0, c.name
        else:
            assert orc["close_cnt"][i] > 0 and orc["rc_flag"][i] == 0, c.name
            assert int(orc["close_pts"][i][orc["close_cnt"][i] - 1]["abs_loc"]) == c.center, c.name
    assert {c.expect for c in cases if c.name.startswith("close")} == {0, 1, P, P + 1}
    assert {c.expect - 1 for c in cases if c.name.startswith("far")} == {P, P + 1}
    assert len(by_name) == len(cases) == 12
    assert sum(orc["far_cnt"][i] > 0 for i, c in enumerate(cases) if c.name.startswith("far")) >= 2       # (far ends are found too)
    # the close end of the long copy is alive into the second 64-base block, a short copy is dead in the first
    # (T = 6 levels at 100 bases, 7 at 150: PG_FIXED_LEN_ROWS)
    T = 6 if L == 100 else 7
    assert max(0, 64 - (6 * L) // 10) < T <= 64 - pic.SEED
