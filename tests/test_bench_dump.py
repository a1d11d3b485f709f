"""bench.py --dump-outputs without a GPU: dump_outputs() on CSR results shaped like binding.Result (the GPU run of the
flag is in tests/test_bench_cli.py)."""
import os
from types import SimpleNamespace

import numpy as np

import bench
from pindel_amd.binding import RUN_DTYPE


def _result(n, seed, max_runs=4):
    """n reads with 0..max_runs close and far runs each, every field of a run derived from its position."""
    rng = np.random.default_rng(seed)
    parts = {}
    for k in ("close", "far"):
        cnt = rng.integers(0, max_runs + 1, n)
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
        runs = np.zeros(int(off[-1]), dtype=RUN_DTYPE)
        j = np.arange(len(runs))
        runs["abs_loc_first"] = 60_000_000 + 7 * j
        runs["len_first"], runs["len_last"] = j % 90 + 10, j % 90 + 12
        runs["mismatches"], runs["flags"], runs["chr_id"] = j % 5, j % 4, j % 3
        parts[k + "_off"], parts[k + "_runs"] = off, runs
    return SimpleNamespace(rc_flag=rng.integers(0, 2, n).astype(np.uint8), **parts)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_a_small_batch_is_dumped_whole_in_float(tmp_path):
    parts = [_result(300, 1), _result(200, 2)]          # two launches of one step (wgs-bins): read order is launch order
    bench.dump_outputs(str(tmp_path), parts, seed=5)
    got = _load(tmp_path)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    np.testing.assert_array_equal(got["read_index"], np.arange(500))
    np.testing.assert_array_equal(got["rc_flag"], np.concatenate([p.rc_flag for p in parts]))
    for k in ("close", "far"):
        off = [p.__dict__[k + "_off"].astype(np.int64) for p in parts]
        np.testing.assert_array_equal(got[k + "_count"], np.concatenate([np.diff(o) for o in off]))
        runs = np.concatenate([p.__dict__[k + "_runs"] for p in parts])
        for f in bench.RUN_FIELDS:
            np.testing.assert_array_equal(got[f"{k}_{f}"], runs[f], err_msg=f"{k}_{f}")
    assert got["close_abs_loc_first"].dtype == np.float64


def test_a_large_batch_is_a_seeded_sample_within_the_byte_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_READS_MAX", 1000)
    res = _result(5000, 3)
    bench.dump_outputs(str(tmp_path / "a"), [res], seed=7)
    bench.dump_outputs(str(tmp_path / "b"), [_result(5000, 3)], seed=7)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    reads = a["read_index"].astype(np.int64)
    assert len(reads) == 1000 and (np.diff(reads) > 0).all() and reads[-1] < 5000
    off = res.far_off.astype(np.int64)
    np.testing.assert_array_equal(a["far_count"], off[reads + 1] - off[reads])
    idx = np.concatenate([np.arange(off[i], off[i + 1]) for i in reads])
    np.testing.assert_array_equal(a["far_abs_loc_first"], res.far_runs["abs_loc_first"][idx])
    np.testing.assert_array_equal(a["rc_flag"], res.rc_flag[reads])

    # a cap the sample does not fit in: reads are dropped from its end, the files stay under the cap
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", (1 << 16) + 20_000)
    bench.dump_outputs(str(tmp_path / "c"), [res], seed=7)
    c = _load(tmp_path / "c")
    assert 0 < len(c["read_index"]) < 1000
    np.testing.assert_array_equal(c["read_index"], a["read_index"][:len(c["read_index"])])
    assert sum(os.path.getsize(tmp_path / "c" / f) for f in os.listdir(tmp_path / "c")) <= bench.DUMP_BYTES_MAX
