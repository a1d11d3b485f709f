"""-m gpu: pg_device_batch_result_sizes / pg_device_batch_download_device -- a searched batch delivered into the caller's
device tensors equals the download to the host."""
import numpy as np
import pytest

from pindel_amd import binding, synth
from pindel_amd.hostio import ReadBatch

pytestmark = pytest.mark.gpu

E_INVALID = -1


@pytest.fixture(scope="module")
def genome():
    return synth.make_genome([400_000, 250_000], seed=41)


@pytest.fixture(scope="module")
def eng(engine_factory, genome):
    e = engine_factory()
    e.load_reference(genome)
    return e


@pytest.fixture(scope="module")
def searched(eng, genome):
    """The 5000-read batch, searched, and its host download."""
    batch = synth.make_reads_genome(genome, 5000, seed=42)
    db = eng.upload(batch)
    eng.search_device(db)
    yield db, eng.download(db)
    eng.free_device_batch(db)


def junk_batch(genome, n=700):
    """Reads that find no close end (all N): both lists are empty -- the shape the device-resident path has for a list
    without runs (its search always runs both ends, so a batch with far runs and no close runs cannot be built through it)."""
    good = synth.make_reads_genome(genome, n, seed=5)
    seq = np.full(len(good.seq), ord("N"), dtype=np.uint8)
    return ReadBatch(seq=seq, seq_off=good.seq_off, anchor_strand=good.anchor_strand, anchor_pos=good.anchor_pos,
                     insert_size=good.insert_size, chr_id=good.chr_id)


def assert_equals_host(t, res):
    assert np.array_equal(t["close_off"].cpu().numpy().view(np.uint64), res.close_off)
    assert np.array_equal(t["far_off"].cpu().numpy().view(np.uint64), res.far_off)
    assert binding.runs_from_tensor(t["close_runs"]).tobytes() == res.close_runs.tobytes()
    assert binding.runs_from_tensor(t["far_runs"]).tobytes() == res.far_runs.tobytes()
    if "rc_flag" in t:
        assert np.array_equal(t["rc_flag"].cpu().numpy(), res.rc_flag)


def close_summary(res):
    """close_last / close_max as the library defines them: UP_Close.back()'s AbsLoc / LengthStr (0 without a close end)."""
    n = res.n
    last, mx = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int16)
    for i in range(n):
        lo, hi = int(res.close_off[i]), int(res.close_off[i + 1])
        if hi > lo:
            p = res.close_points(i)[-1]
            last[i], mx[i] = p["abs_loc"], p["length"]
    return last, mx


def test_download_tensors_equals_download(eng, searched):
    db, res = searched
    assert eng.result_sizes(db) == (int(res.close_off[-1]), int(res.far_off[-1]))
    assert res.close_off[-1] > 1000 and res.far_off[-1] > 500
    t = eng.download_tensors(db)
    assert all(str(x.device) == "cuda:0" for x in t.values())
    assert_equals_host(t, res)
    last, mx = close_summary(res)
    has = mx > 0
    assert np.array_equal(t["close_max"].cpu().numpy(), mx)
    assert np.array_equal(t["close_last"].cpu().numpy().view(np.uint32)[has], last[has])
    # a host download afterwards still equals the first, and so does a second device download
    again = eng.download(db)
    for k in ("close_off", "far_off", "rc_flag"):
        assert np.array_equal(getattr(again, k), getattr(res, k))
    assert again.close_runs.tobytes() == res.close_runs.tobytes() and again.far_runs.tobytes() == res.far_runs.tobytes()
    assert_equals_host(eng.download_tensors(db), res)


def test_several_chunks(eng, searched, pg_env):
    """(chunks of 1000 reads: the gather of every chunk writes its slice of the caller's buffers)"""
    db, res = searched
    pg_env.set("PG_HOST_CHUNK", "1000")
    assert_equals_host(eng.download_tensors(db), res)


def test_optional_arrays_may_be_null(eng, searched):
    db, res = searched
    t = eng.download_tensors(db, summaries=False)
    assert set(t) == {"close_off", "close_runs", "far_off", "far_runs"}
    assert_equals_host(t, res)


def test_a_capacity_one_short_writes_nothing(eng, searched):
    import torch
    db, res = searched
    n, (nc, nf) = res.n, eng.result_sizes(db)
    for short in ("close", "far"):
        off = [torch.full((n + 1,), -7, dtype=torch.int64, device="cuda:0") for _ in range(2)]
        runs = [torch.full((nc - (short == "close"), 12), 0xA5, dtype=torch.uint8, device="cuda:0"),
                torch.full((nf - (short == "far"), 12), 0xA5, dtype=torch.uint8, device="cuda:0")]
        rc = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda:0")
        with pytest.raises(binding.PgError) as e:
            eng.download_into(db, off[0], runs[0], off[1], runs[1], rc_flag=rc)
        assert e.value.code == E_INVALID and f"{short}_cap" in str(e.value)
        assert all(bool((x == -7).all()) for x in off) and all(bool((x == 0xA5).all()) for x in runs + [rc])
    assert_equals_host(eng.download_tensors(db), res)


def test_a_host_pointer_is_refused(eng, searched):
    import ctypes as C
    import torch
    db, res = searched
    n, (nc, nf) = res.n, eng.result_sizes(db)
    dev = dict(close_off=torch.empty(n + 1, dtype=torch.int64, device="cuda:0"), close_runs=torch.empty((nc, 12), dtype=torch.uint8, device="cuda:0"),
               far_off=torch.empty(n + 1, dtype=torch.int64, device="cuda:0"), far_runs=torch.empty((nf, 12), dtype=torch.uint8, device="cuda:0"),
               rc_flag=torch.empty(n, dtype=torch.uint8, device="cuda:0"), close_last=torch.empty(n, dtype=torch.int32, device="cuda:0"),
               close_max=torch.empty(n, dtype=torch.int16, device="cuda:0"))
    for name, t in dev.items():
        host = np.zeros(t.numel() * t.element_size() + 8, dtype=np.uint8)
        ptrs = {k: v.data_ptr() for k, v in dev.items()}
        ptrs[name] = host.ctypes.data + (-host.ctypes.data) % 8
        d = binding.PgDeviceResult(ptrs["close_off"], ptrs["close_runs"], nc, ptrs["far_off"], ptrs["far_runs"], nf,
                                   ptrs["rc_flag"], ptrs["close_last"], ptrs["close_max"])
        assert eng._L.pg_device_batch_download_device(eng._h, db, C.byref(d)) == E_INVALID, name
        assert name.encode() in eng._L.pg_last_error(eng._h)
        assert not host.any()
    eng.download_into(db, **dev)
    assert_equals_host(dev, res)


def test_lists_without_runs(eng, genome):
    import torch
    batch = junk_batch(genome)
    db = eng.upload_tensors(*[torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (
        batch.seq, batch.seq_off.view(np.int64), batch.anchor_strand, batch.anchor_pos, batch.insert_size, batch.chr_id)])
    eng.search_device(db)
    res = eng.download(db)
    assert res.close_off[-1] == 0 and res.far_off[-1] == 0 and eng.result_sizes(db) == (0, 0)
    t = eng.download_tensors(db)
    assert t["close_runs"].shape == (0, 12) and not bool(t["close_off"].any()) and not bool(t["far_off"].any())
    assert_equals_host(t, res)
    eng.free_device_batch(db)


def test_empty_batch_launches_nothing(eng, genome):
    empty = synth.make_reads_genome(genome, 50, seed=1).slice(0, 0)
    db = eng.upload(empty)
    eng.clear_launch_log()
    eng.search_device(db)
    before = eng.launch_log()
    assert eng.result_sizes(db) == (0, 0)
    t = eng.download_tensors(db)
    assert eng.launch_log() == before
    assert t["close_off"].tolist() == [0] and t["far_off"].tolist() == [0] and t["close_runs"].shape == (0, 12)
    assert t["rc_flag"].numel() == 0
    eng.free_device_batch(db)
