"""-m gpu: every kernel the library can launch, reached on purpose and checked against the oracle (tests/instantiations.py).

Per case (one (NB, NS, Id, DEF) cell at its low or high edge) the batch runs through six paths -- (a) search_batch, (b) upload +
scribble + pack_search_device, (c) PG_NO_PACK_IN_PLACE + repack + search_device, (d) close_end_batch, (e)
far_end_batch_from_close fed from (d), (f) PG_SPLIT_LAUNCH + search_batch -- and after each one the library's launch log must
name the kernels the plan's mirror of the dispatch rules predicts, and the result must equal the oracle bit for bit."""
import json
import os

import numpy as np
import pytest

from pindel_amd import binding, hostio
from tests import instantiations as I
from tests import shortening_cases as sc
from tests.parity import compare_result, oracle_points, points_per_read, run_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    return I.reference()


@pytest.fixture(scope="module")
def first_launch():
    """kernel -> the first case that launched it; written to $PG_MATRIX_REPORT (a JSON file) when that is set"""
    seen = {}
    yield seen
    path = os.environ.get("PG_MATRIX_REPORT")
    if path:
        with open(path, "w") as fh:
            json.dump({I.kernel_name(k): v for k, v in sorted(seen.items())}, fh, indent=1)


def _max_mm(orc, which, idx):
    pts = [oracle_points(orc, int(i), which) for i in idx]
    pts = [p for p in pts if len(p)]
    return int(np.concatenate(pts)["mismatches"].max()) if pts else -1


def _kept_for_far(batch, close, orc, bd, bd_off):
    """the reads with a close end as GetCloseEnd left them (the oracle's sequences: reverse-complemented and shortened where it
    did so -- (d) equals the oracle, so these are what (d) left), UP_Close.back() from (d), and their windows"""
    has, close_last, close_max = sc.close_back(close)
    kept = np.nonzero(has)[0]
    off = batch.seq_off.astype(np.int64)
    seqs = [orc["seq"][off[i]:off[i] + int(orc["len_out"][i])].tobytes() for i in kept]
    kb = hostio.batch_from_lists(seqs, [bytes([c]) for c in batch.anchor_strand[kept]], batch.anchor_pos[kept],
                                 batch.insert_size[kept], batch.chr_id[kept])
    kbd = kbd_off = None
    if bd is not None:
        bo = bd_off.astype(np.int64)
        kbd = np.concatenate([bd[bo[i]:bo[i + 1]] for i in kept])
        kbd_off = np.concatenate([[0], np.cumsum(bo[kept + 1] - bo[kept])]).astype(np.uint64)
    return kept, kb, close_last[kept], close_max[kept], kbd, kbd_off


@pytest.mark.parametrize("case", I.CASES, ids=[c.id for c in I.CASES])
def test_instantiation(case, ref, pg_env, first_launch):
    batch, bd, bd_off = I.build_batch(case, ref[0][1])
    n = batch.n
    # the oracle with the case's windows (device-resident paths, far end) and without (the host paths take none)
    orc = run_oracle(case.params, ref, batch, bd=bd, bd_off=bd_off)
    orc_host = run_oracle(case.params, ref, batch) if bd is not None else orc

    # the inputs reach the edge the case names
    lens = batch.lengths()
    assert ((orc["close_cnt"] > 0) & (lens == case.longest)).sum() >= 10, "reads at the longest length find no close end"
    if (lens % 64 == 1).any():
        assert ((orc["close_cnt"] > 0) & (lens % 64 == 1)).sum() >= 10, "reads at 1 (mod 64) bases find no close end"
    all_reads = range(n)
    mm_close, mm_far = _max_mm(orc, "close", all_reads), _max_mm(orc, "far", all_reads)
    top = I.top_slice_needed(case)
    if top is not None:
        assert mm_close >= top and mm_far >= top, ("no point sets the counter's top slice", mm_close, mm_far, top)
    assert mm_close >= I.MM_REACH[case.id] and mm_far >= I.MM_REACH[case.id], (mm_close, mm_far, I.MM_REACH[case.id])
    if case.junk:
        assert any(b not in b"ACGTN" for b in set(batch.seq.tobytes()))

    for k, v in case.switches("a").items():          # (the case's own switches: PG_GENERIC_KERNELS, PG_FORCE_WIDE_CELLS)
        pg_env.set(k, v)
    eng = binding.Engine(**case.params)
    try:
        eng.load_reference(ref)

        def check_log(path, n_reads):
            got = set(eng.launch_log())
            want = case.expected(path, n_reads)
            assert got == want, (path, sorted(got), sorted(want))
            for r in got:
                first_launch.setdefault(I.kernel_of(r), f"{case.id} ({path})")

        def with_switches(path, fn):
            extra = {k: v for k, v in case.switches(path).items() if k not in case.switches("a")}
            for k, v in extra.items():
                pg_env.set(k, v)
            try:
                return fn()
            finally:
                for k in extra:
                    pg_env.unset(k)

        # (a) host pipeline, fused launch
        eng.clear_launch_log()
        res = eng.search_batch(batch)
        check_log("a", n)
        compare_result(res, orc_host, n)

        # (b) device-resident, one launch that packs in place over scribbled records
        def path_b():
            db = eng.upload(batch)
            try:
                if bd is not None:
                    eng.set_windows(db, bd, bd_off)
                eng.scribble_records(db)
                eng.clear_launch_log()
                eng.pack_search_device(db)
                check_log("b", n)
                compare_result(eng.download(db), orc, n)
            finally:
                eng.free_device_batch(db)
        with_switches("b", path_b)

        # (c) the pack kernel, then a search that does not pack
        def path_c():
            db = eng.upload(batch)
            try:
                if bd is not None:
                    eng.set_windows(db, bd, bd_off)
                eng.clear_launch_log()
                eng.repack(db)
                eng.search_device(db)
                check_log("c", n)
                compare_result(eng.download(db), orc, n)
            finally:
                eng.free_device_batch(db)
        with_switches("c", path_c)

        # (d) close end alone
        eng.clear_launch_log()
        close = eng.close_end_batch(batch)
        check_log("d", n)
        compare_result(close, orc_host, n, check_far=False)
        assert close.far_off[-1] == 0

        # (e) far end alone, from (d)'s close ends, with the case's windows
        kept, kb, close_last, close_max, kbd, kbd_off = _kept_for_far(batch, close, orc, bd, bd_off)
        assert len(kept) >= 50          # (17 levels at 36 bases, -a 6 -e 0.15: a quarter of the reads keep a close end)
        eng.clear_launch_log()
        far = eng.far_end_batch_from_close(kb, close_last, close_max, kbd, kbd_off)
        check_log("e", len(kept))
        np.testing.assert_array_equal(points_per_read(far.far_off, far.far_runs), orc["far_cnt"][kept], err_msg="UP_Far points per read")
        g_far = binding.expand_runs(far.far_runs)
        o_far = np.concatenate([oracle_points(orc, int(i), "far") for i in kept])
        assert g_far.tobytes() == o_far.tobytes(), "UP_Far of the far end from close"
        assert (orc["far_cnt"][kept] > 0).sum() >= 10

        # (f) close end and far end as two launches
        def path_f():
            eng.clear_launch_log()
            res = eng.search_batch(batch)
            check_log("f", n)
            compare_result(res, orc_host, n)
        with_switches("f", path_f)
    finally:
        eng.close()
