"""The classifier parity hunt is not vacuous, shown without a GPU: for exactly the seeds tests/test_gpu_classifier_fuzz.py commits, the
inputs of scripts/fuzz_classifier_input.py are searched with the CPU oracle and the host statements of the whole chain
(HostChain: the comparison-free half of scripts/fuzz_classifier.py) run on the oracle's lists.  What they hold is asserted here --
conditions on the inputs: a seed set that stops meeting them is changed, or the generator, never the condition."""
import numpy as np
import pytest

from oracle import pyoracle
from pindel_amd import binding
from scripts.fuzz_classifier_input import HostChain, fuzz_input, lists_of_oracle, tally
from tests.parity import run_oracle
from tests.test_gpu_classifier_fuzz import N_READS, STREAMS

_cache = {}


def tallied(seed):
    """the tally of one seed (computed once per session); nothing may be skipped: the oracle accepts every committed parameter set"""
    if seed not in _cache:
        inp = fuzz_input(seed, N_READS)
        orc = run_oracle(inp.kw, inp.chroms, inp.batch, bd=inp.bd, bd_off=inp.bd_off)
        mm = pyoracle.max_mismatch_table(inp.kw.get("seq_error_rate", 0.01), inp.kw.get("sensitivity", 0.95))
        t = tally(HostChain(inp, lists_of_oracle(orc, inp.batch.n), mm).all())
        t.update(max_listed=inp.max_listed, chromosomes=len(inp.chroms), search=inp.search, kw=inp.kw, n=inp.batch.n)
        _cache[seed] = t
    return _cache[seed]


def every():
    return [tallied(s) for seeds in STREAMS.values() for s in seeds]


def test_streams_are_what_they_are_named():
    assert set(STREAMS) == {"low", "default_parameters", "wide", "multi_chromosome", "outside_acgtn"}
    assert all(3 <= len(s) <= 5 and len(set(s)) == len(s) for s in STREAMS.values())
    assert all(s < 200000 for s in STREAMS["low"]) and all(200000 <= s < 300000 for s in STREAMS["wide"])
    assert all(300000 <= s < 400000 for s in STREAMS["default_parameters"]) and all(400000 <= s < 500000 for s in STREAMS["multi_chromosome"])
    assert all(s >= 600000 for s in STREAMS["outside_acgtn"])
    search = ("max_range_index", "additional_mismatch", "min_perfect_match", "min_close")
    assert not any(k in tallied(s)["kw"] for s in STREAMS["default_parameters"] for k in search)
    assert any(k in tallied(s)["kw"] for s in STREAMS["low"] + STREAMS["wide"] for k in search)
    assert all(tallied(s)["chromosomes"] >= 2 for s in STREAMS["multi_chromosome"])
    assert {tallied(s)["chromosomes"] for seeds in STREAMS.values() for s in seeds} == {1, 2, 3}
    assert {t["search"] for t in every()} == {"search_device", "pack_search_device", "search_table_device"}
    assert {t["max_listed"] for t in every()} >= {0, 4} and all(t["n"] == N_READS for t in every())


@pytest.mark.parametrize("stream", sorted(STREAMS))
def test_every_stream_holds_the_hard_reads(stream):
    ts = [tallied(s) for s in STREAMS[stream]]
    assert sum(t["multi_close"] for t in ts) > 0 and sum(t["multi_far_runs"] for t in ts) > 0       # several close points; several far runs
    assert sum(t["more"] for t in ts) > 0                                                           # VARIANT_MORE
    assert max(t["boxed"] for t in ts) >= 2 * binding.EVENT_BLOCK + 1                               # more than two scan / sort blocks
    for table in range(4):
        assert sum(t["multi"][table] for t in ts) > 0, f"no event of table {table} with two members"
        assert sum(t["both"][table] for t in ts) > 0, f"no event of table {table} with members of both strands"


def test_the_set_holds_every_kind_of_table_entry():
    ts = every()
    assert sum(t["duplicates"] for t in ts) > 0                                                     # EVR_DUPLICATE
    assert any(t["unresolved"] > 0 and t["max_listed"] < 4 for t in ts)
    for table in range(3):
        assert sum(t["sv_events"][table] for t in ts) > 0, f"no SV event of table {table}"
    for strand in range(2):
        assert sum(t["li_multi"][strand] for t in ts) > 0, f"no LI position with two reads on strand {strand}"
    dd = [t["dd"] for t in ts]
    assert sum(d["multi"] for d in dd) > 0 and sum(d["tested"] for d in dd) > 0 and sum(d["dropped"] for d in dd) > 0
    assert sum(d["contained"] for d in dd) > 0 and sum(d["clear"] for d in dd) > 0


def test_the_multi_chromosome_stream_holds_junction_calls():
    calls = [tallied(s)["int"] for s in STREAMS["multi_chromosome"]]
    assert sum(c["fallback"] for c in calls) > 0 and sum(c["template"] for c in calls) > 0 and sum(c["multi"] for c in calls) > 0


def test_the_stream_outside_acgtn_holds_every_rc_flag_among_the_dd_members():
    rc = np.sum([tallied(s)["dd"]["rc"] for s in STREAMS["outside_acgtn"]], axis=0)
    assert (rc > 0).all(), rc.tolist()
