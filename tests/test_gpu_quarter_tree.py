"""-m gpu: ties and unique points across the tier A quarters (evaluate's quarter merge; pg_tree_merge in pg_kernels.hip merges the
quarters as a tree where the other kernels merge them one after the other).  The reads of tests/pass_kind_cases.py (build_quarters):
2, 3, 4, 5 and 8 short-lived copies of a read's first bases are the only candidates of the close end's window, so copy i is entry i of
the tier A list and lies in quarter i modulo 4; all tied -- no point -- or copy i two bases longer, for every i: one point at length
18, whichever quarter holds the winner and however many entries its quarter holds.  The far end: tied copies in all three rings of
the fused pass and the longer copy in ring 0, 1 or 2, so the evaluations of the three nested ranges merge quarter 0 alone, quarters
0 and 1, and all four.  Bit for bit against the oracle on the fixed-length kernels for 100 and 101 bases, and once on the
default-parameter kernel for any length in a fresh child process."""
import pytest

from tests import pass_kind_cases as pkc
from tests import test_gpu_pass_kinds as tk

pytestmark = pytest.mark.gpu


def inputs(L):
    return tk.inputs(L, pkc.build_quarters, "quarters")


@pytest.mark.parametrize("L", [100, 101])
def test_ties_and_winners_in_every_quarter_fixed(engine_factory, L):
    ref, cases, batch, orc = inputs(L)
    names = {c.name for c in cases}
    assert {f"q{s}{k}b{i}" for s in "+-" for k in pkc.QUARTER_COPIES for i in range(k)} <= names
    assert {f"f{s}r{r}" for s in "+-" for r in range(3)} | {f"f{s}tie" for s in "+-"} <= names
    total = tk.run(engine_factory(), ref, batch, orc, L)
    assert total >= 4 * sum(c.n_copies for c in cases)


def test_ties_and_winners_any_length_kernel():
    tk.run_child("quarters", 100)
