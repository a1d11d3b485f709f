"""-m gpu: the candidate pass with lanes that hold no candidate (fold_candidates; its open form, pg_open_pass in pg_kernels.hip, computes
in every lane and reads every queue slot, written or not).  The reads of tests/pass_idle_cases.py have a known number of candidates per
pass -- 0, 1, PG_PASS and PG_PASS + 1 at the close end, PG_PASS and PG_PASS + 1 in the far end's innermost chunk (the fused pass and its
fallback), with and without candidates in the two inner rings -- and every batch is compared bit for bit with the oracle through
pack_search_device, on the fixed-length kernel, on the default-parameter kernel for any length (PG_NO_FIXED_LEN) and at 150 bases
(PG_PASS = 32).  The counts are asserted from the device's own record: a batch of one read, whose candidates Engine.candidates
returns.  In the batch of a few hundred reads every case stands at every position modulo eight, so each is the first read of some
workgroup (claims of eight), the one that finds the queue as the kernel start left it; ordinary reads of a second chromosome run among them."""
import pytest

from pindel_amd import synth
from tests import pass_idle_cases as pic
from tests import shortening_cases as sc
from tests.parity import compare_result, run_oracle

pytestmark = pytest.mark.gpu

_built = {}


def _inputs(L):
    """(reference, cases, the batch of a few hundred reads, its oracle result, per case (batch of one, oracle result)), built once"""
    if L not in _built:
        chrom, cases = pic.build(L)
        plain_ref = synth.make_reference(150_000, seed=90 + L, n_gaps=0)
        ref = [("chrN", chrom), ("chrP", plain_ref)]
        # read t of the constructed part is case (t // 8 + t % 8) mod 12: every case stands at every position modulo eight, so whatever
        # the phase of the claims of eight, each case heads one; 96 ordinary reads in the middle
        order = [(t // 8 + t % 8) % len(cases) for t in range(480)]
        built = pic.batch_of(cases, order)
        plain = synth.make_reads(plain_ref, 96, read_len=L, seed=91 + L)
        plain.chr_id[:] = 1
        batch = sc.concat([built.slice(0, 240), plain, built.slice(240, 480)])
        assert (batch.lengths() == L).all() and batch.n == 576
        singles = []
        for i in range(len(cases)):
            one = pic.batch_of(cases, [i])
            singles.append((one, run_oracle({}, ref, one)))
        _built[L] = (ref, cases, batch, run_oracle({}, ref, batch), singles)
    return _built[L]


def _run(eng, batch, orc, want_len):
    db = eng.upload(batch)
    try:
        eng.scribble_records(db)
        eng.pack_search_device(db)
        assert eng.last_fixed_len() == want_len
        compare_result(eng.download(db), orc, batch.n)
        return eng.candidates(db)
    finally:
        eng.free_device_batch(db)


KERNELS = [(100, True), (100, False), (150, True)]
IDS = ["fixed-100", "defaults-100", "fixed-150"]


@pytest.mark.parametrize("L,fixed", KERNELS, ids=IDS)
def test_every_case_alone_has_its_candidates(engine_factory, pg_env, L, fixed):
    """a launch of one read per case: bit-exact, and the read's candidate count is the planted one (no case passes for want of
    candidates: 0, 1, PG_PASS, PG_PASS + 1 at the close end; 1 + PG_PASS and 1 + PG_PASS + 1 with the far end)"""
    if not fixed:
        pg_env.set("PG_NO_FIXED_LEN", "1")
    eng = engine_factory()
    ref, cases, _, _, singles = _inputs(L)
    eng.load_reference(ref)
    got = {}
    for c, (one, orc) in zip(cases, singles):
        got[c.name] = int(_run(eng, one, orc, L if fixed else 0))
    print(got)
    assert got == {c.name: c.expect for c in cases}
    P = pic.pass_size(L)
    assert sorted(set(got.values())) == [0, 1, P, P + 1, P + 2]


@pytest.mark.parametrize("L,fixed", KERNELS, ids=IDS)
def test_cases_heading_every_claim(engine_factory, pg_env, L, fixed):
    if not fixed:
        pg_env.set("PG_NO_FIXED_LEN", "1")
    eng = engine_factory()
    ref, cases, batch, orc, _ = _inputs(L)
    eng.load_reference(ref)
    assert (orc["close_cnt"] > 0).sum() > batch.n // 2 and (orc["far_cnt"] > 0).sum() > batch.n // 8
    total = _run(eng, batch, orc, L if fixed else 0)
    # (the ordinary reads' candidates are not planted: a lower bound)
    assert total >= 40 * sum(c.expect for c in cases)
