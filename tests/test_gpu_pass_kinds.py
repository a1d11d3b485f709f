"""-m gpu: the block of a candidate in both kinds (fold_candidates; pg_rev_mismatch in pg_kernels.hip reverses a kind-B candidate's
mismatch word where the other kernels reverse its three reference words).  The reads of tests/pass_kind_cases.py (build_kinds): the
close end of a '+' anchor is a pass of kind F alone, that of a '-' anchor of kind B alone, the far-end pass holds a long copy of
either kind at once; the copy at the first and the last position attempt 0's window admits (and one position outside: found in the
R = 1 window); a substitution, a read N and a reference N at bases 63 and 64 -- the last of the first block and the first of the
second, which holds 36 bases of a 100-base read and 37 of a 101-base one -- and a read N / reference N at base 0.  Bit for bit against
the oracle through pack_search_device on the fixed-length kernels for 100 and 101 bases (pg_debug_last_fixed_len asserted), and once
on the default-parameter kernel for any length (PG_NO_FIXED_LEN=1) in a fresh child process.  In the batch every case stands at
several positions modulo eight among ordinary reads of a second chromosome."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pindel_amd import synth                                  # noqa: E402
from tests import pass_kind_cases as pkc                      # noqa: E402
from tests import shortening_cases as sc                      # noqa: E402
from tests.parity import compare_result, run_oracle           # noqa: E402

pytestmark = pytest.mark.gpu

_built = {}


def inputs(L, build=pkc.build_kinds, tag="kinds"):
    """(reference, cases, batch, its oracle result, index of the first constructed read), built once; asserts the coverage"""
    if (tag, L) not in _built:
        chrom, cases = build(L)
        plain_ref = synth.make_reference(120_000, seed=70 + L, n_gaps=0)
        ref = [("chrK", chrom), ("chrP", plain_ref)]
        n = len(cases)
        # every case once in order (the coverage is read from these), then at shifted positions modulo eight
        order = list(range(n)) + [(t + t // n) % n for t in range(3 * n)]
        built = pkc.batch_of(cases, order)
        plain = synth.make_reads(plain_ref, 64, read_len=L, seed=71 + L)
        plain.chr_id[:] = 1
        batch = sc.concat([plain.slice(0, 32), built, plain.slice(32, 64)])
        assert (batch.lengths() == L).all()
        orc = run_oracle({}, ref, batch)
        pkc.check_situations(L, cases, orc, first=32)
        _built[(tag, L)] = (ref, cases, batch, orc)
    return _built[(tag, L)]


def run(eng, ref, batch, orc, want_len):
    eng.load_reference(ref)
    db = eng.upload(batch)
    try:
        eng.scribble_records(db)
        eng.pack_search_device(db)
        assert eng.last_fixed_len() == want_len
        compare_result(eng.download(db), orc, batch.n)
        return eng.candidates(db)
    finally:
        eng.free_device_batch(db)


@pytest.mark.parametrize("L", [100, 101])
def test_blocks_of_both_kinds_fixed(engine_factory, L):
    ref, cases, batch, orc = inputs(L)
    total = run(engine_factory(), ref, batch, orc, L)
    assert total >= 4 * sum(c.n_copies for c in cases if "N0" not in c.name)


def child_main(tag, L):
    """the default-parameter kernel for any length: PG_NO_FIXED_LEN is read once per process"""
    from pindel_amd import binding
    assert os.environ.get("PG_NO_FIXED_LEN") == "1"
    from tests import test_gpu_quarter_tree as tq
    ref, cases, batch, orc = inputs(L) if tag == "kinds" else tq.inputs(L)
    eng = binding.Engine()
    try:
        run(eng, ref, batch, orc, 0)
    finally:
        eng.close()
    print("child ok", tag, L)


def run_child(tag, L):
    env = dict(os.environ, PG_NO_FIXED_LEN="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-s", os.path.abspath(__file__), tag, str(L)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"child ok {tag} {L}" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_blocks_of_both_kinds_any_length_kernel():
    run_child("kinds", 100)


if __name__ == "__main__":
    child_main(sys.argv[1], int(sys.argv[2]))
