"""-m gpu: pg_device_batch_upload_device -- a batch whose arrays are device tensors gives the batch, the statuses and the
kernels of the host upload."""
import ctypes as C

import numpy as np
import pytest

from pindel_amd import binding, synth
from pindel_amd.hostio import ReadBatch

pytestmark = pytest.mark.gpu

E_INVALID, E_READ_TOO_LONG = -1, -5
FIELDS = ("seq", "seq_off", "anchor_strand", "anchor_pos", "insert_size", "chr_id")


@pytest.fixture(scope="module")
def genome():
    return synth.make_genome([400_000, 250_000], seed=41)


@pytest.fixture(scope="module")
def eng(engine_factory, genome):
    e = engine_factory()
    e.load_reference(genome)
    return e


@pytest.fixture(scope="module")
def reads5000(genome):
    return synth.make_reads_genome(genome, 5000, seed=42)


def to_tensors(batch):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (
        np.asarray(batch.seq, dtype=np.uint8), np.asarray(batch.seq_off, dtype=np.uint64).view(np.int64),
        np.asarray(batch.anchor_strand, dtype=np.uint8), np.asarray(batch.anchor_pos, dtype=np.int32),
        np.asarray(batch.insert_size, dtype=np.int16), np.asarray(batch.chr_id, dtype=np.int32))]


def same_result(a, b, what=""):
    for k in ("close_off", "far_off", "rc_flag"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), (what, k)
    for k in ("close_runs", "far_runs"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), (what, k)


def run(eng, db, step="search"):
    """search (or pack + search) and download; returns (result, fixed length, launch log)"""
    eng.clear_launch_log()
    (eng.pack_search_device if step == "pack_search" else eng.search_device)(db)
    return eng.download(db), eng.last_fixed_len(), eng.launch_log()


def both_paths(eng, batch, step="search"):
    h = eng.upload(batch)
    d = eng.upload_tensors(*to_tensors(batch))
    try:
        return run(eng, h, step), run(eng, d, step)
    finally:
        eng.free_device_batch(h)
        eng.free_device_batch(d)


def mixed_batch(genome, n=3000, seed=43):
    """Reads of 1 .. 499 bases (synth's 499-base reads cut short), some with characters outside ACGTN."""
    full = synth.make_reads_genome(genome, n, seed=seed, read_len=499)
    rng = np.random.default_rng(seed)
    lens = rng.choice([1, 22, 64, 65, 128, 129, 499, 100, 37], size=n)
    lens[:9] = [1, 22, 64, 65, 128, 129, 499, 100, 37]
    rows = np.asarray(full.seq, dtype=np.uint8).reshape(n, 499).copy()
    odd = np.frombuffer(b"acgtRYKMSWBDHVU.-*\x00", dtype=np.uint8)
    for i in rng.choice(n, size=n // 20, replace=False):          # the exact kernel's list
        k = int(rng.integers(0, lens[i]))
        rows[i, k] = odd[rng.integers(0, len(odd))]
    seq = np.concatenate([rows[i, :lens[i]] for i in range(n)])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return ReadBatch(seq=seq, seq_off=off, anchor_strand=full.anchor_strand, anchor_pos=full.anchor_pos,
                     insert_size=full.insert_size, chr_id=full.chr_id)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 5000])
def test_uniform_batches_equal_the_host_upload(eng, reads5000, n):
    """Uniform 100-base reads on two chromosomes: the same result, the same fixed-length kernel, the same launches."""
    (rh, fh, lh), (rd, fd, ld) = both_paths(eng, reads5000.slice(0, n))
    same_result(rh, rd, n)
    assert fh == fd and lh == ld
    if n:
        assert fh == 100 and rh.close_off[-1] > 0


def test_a_batch_that_does_not_start_at_offset_zero(eng, reads5000):
    """seq_off[0] > 0: the offsets are rebased and only the batch's bases are copied."""
    import torch
    sub = reads5000.slice(100, 400)
    t = to_tensors(reads5000)
    d = eng.upload_tensors(t[0], t[1][100:401].contiguous(), *[x[100:400].contiguous() for x in t[2:]])
    h = eng.upload(sub)
    same_result(run(eng, h)[0], run(eng, d)[0])
    eng.free_device_batch(h)
    eng.free_device_batch(d)
    torch.cuda.synchronize()


@pytest.mark.parametrize("step", ["search", "pack_search"])
def test_mixed_lengths_and_odd_characters(eng, genome, step):
    batch = mixed_batch(genome)
    (rh, fh, lh), (rd, fd, ld) = both_paths(eng, batch, step)
    same_result(rh, rd, step)
    assert fh == fd == 0 and lh == ld
    assert any(r.kernel == 2 for r in ld)                         # the exact kernel ran: the list was built from the device copy


def test_uniform_pack_search(eng, reads5000):
    (rh, fh, lh), (rd, fd, ld) = both_paths(eng, reads5000, "pack_search")
    same_result(rh, rd)
    assert fh == fd == 100 and lh == ld


def _copy(batch, **kw):
    d = {k: np.array(getattr(batch, k)) for k in FIELDS}
    d.update(kw)
    return ReadBatch(**d)


def _plant(batch, where):
    """where: {index: code} -- code 1 (seq_off not monotone), 3 (chr_id out of range) or 4 (anchor outside the chromosome)"""
    off, chr_id, pos = (np.array(batch.seq_off), np.array(batch.chr_id), np.array(batch.anchor_pos))
    for i, code in where.items():
        if code == 1:
            off[i + 1] = off[i] - 1
        elif code == 3:
            chr_id[i] = 2
        else:
            pos[i] = -100_000
    return _copy(batch, seq_off=off, chr_id=chr_id, anchor_pos=pos)


def _status(eng, fn, batch):
    try:
        eng.free_device_batch(fn(batch))
        return 0, ""
    except binding.PgError as e:
        return e.code, str(e)


def _both_status(eng, batch):
    return _status(eng, eng.upload, batch), _status(eng, lambda b: eng.upload_tensors(*to_tensors(b)), batch)


def _with_length(batch, i, length):
    lens = np.diff(np.asarray(batch.seq_off).astype(np.int64))
    lens[i] = length
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    seq = np.resize(np.asarray(batch.seq), int(off[-1]))
    return _copy(batch, seq=seq, seq_off=off)


@pytest.mark.parametrize("code,status", [(1, E_INVALID), (2, E_READ_TOO_LONG), (3, E_INVALID), (4, E_INVALID)])
def test_validation_codes_equal_the_host_uploads(eng, reads5000, code, status):
    bad = _with_length(reads5000, 1234, 500) if code == 2 else _plant(reads5000, {1234: code})
    host, dev = _both_status(eng, bad)
    assert host == dev and host[0] == status and host[1]


def test_length_limits(eng, reads5000):
    host, dev = _both_status(eng, _with_length(reads5000, 77, 499))
    assert host == dev == (0, "")
    host, dev = _both_status(eng, _with_length(reads5000, 77, 500))
    assert host == dev and host[0] == E_READ_TOO_LONG


@pytest.mark.parametrize("codes", [(3, 1), (1, 3)])
def test_the_bad_read_with_the_lowest_index_is_reported(eng, reads5000, codes):
    """Two bad reads in different wavefronts and workgroups (70, 4100): whichever code sits at 70 is the one reported."""
    alone = _both_status(eng, _plant(reads5000, {70: codes[0]}))
    host, dev = _both_status(eng, _plant(reads5000, {70: codes[0], 4100: codes[1]}))
    assert host == dev == alone[0] and host[0] == E_INVALID
    assert ("chr_id" in host[1]) == (codes[0] == 3) and ("monotone" in host[1]) == (codes[0] == 1)


@pytest.mark.parametrize("which", range(6))
def test_a_host_pointer_is_refused_with_a_status(eng, reads5000, which):
    """A numpy (host) pointer in place of one device array: PG_E_INVALID naming the array, and the engine goes on working."""
    batch = reads5000.slice(0, 300)
    t = to_tensors(batch)
    host = [np.ascontiguousarray(x.cpu().numpy()) for x in t]
    ptrs = [x.data_ptr() for x in t]
    ptrs[which] = host[which].ctypes.data
    s = binding.PgReadBatch(batch.n, *ptrs)
    h = C.c_void_p()
    assert eng._L.pg_device_batch_upload_device(eng._h, C.byref(s), C.byref(h)) == E_INVALID
    assert not h.value and FIELDS[which].encode() in eng._L.pg_last_error(eng._h)
    d = eng.upload_tensors(*t)
    hb = eng.upload(batch)
    same_result(run(eng, hb)[0], run(eng, d)[0])
    eng.free_device_batch(hb)
    eng.free_device_batch(d)


def test_an_array_shorter_than_the_batch_is_refused(eng, reads5000):
    """n_reads beyond the allocation behind a pointer: refused before anything reads past its end."""
    import torch
    batch = reads5000.slice(0, 300)
    t = to_tensors(batch)
    big_n = 1 << 22                                               # (more bytes per array than a small tensor's allocation holds)
    ptrs = [x.data_ptr() for x in t]
    off = torch.zeros(big_n + 1, dtype=torch.int64, device="cuda:0")
    ptrs[1] = off.data_ptr()
    s = binding.PgReadBatch(big_n, *ptrs)
    h = C.c_void_p()
    assert eng._L.pg_device_batch_upload_device(eng._h, C.byref(s), C.byref(h)) == E_INVALID
    assert b"allocation" in eng._L.pg_last_error(eng._h)


def test_window_hints_on_a_device_uploaded_batch(eng, genome, reads5000):
    """set_windows on the new batch: per-read BreakDancer clusters (some on the other chromosome, some with start < 0)."""
    batch = reads5000.slice(0, 2000)
    rng = np.random.default_rng(7)
    wins, offs = [], [0]
    close = eng.close_end_batch(batch)                            # hints: 0-4 windows per read around plausible far ends
    for i in range(batch.n):
        lo, hi = int(close.close_off[i]), int(close.close_off[i + 1])
        for _ in range(int(rng.integers(0, 5)) if hi > lo else 0):
            c = int(batch.chr_id[i]) if rng.random() < 0.8 else 1 - int(batch.chr_id[i])
            size = len(genome[c][1])
            centre = int(close.close_runs[lo]["abs_loc_first"]) + int(rng.integers(-150_000, 150_000))
            centre = min(max(centre, 100_300), size - 100_300)
            wins.append((c, -1 if rng.random() < 0.05 else centre - 200, centre + 200))
        offs.append(len(wins))
    bd, bd_off = np.array(wins, dtype=binding.WINDOW_DTYPE), np.array(offs, dtype=np.uint64)
    h, d = eng.upload(batch), eng.upload_tensors(*to_tensors(batch))
    assert len(bd) > 2000
    eng.set_windows(h, bd, bd_off)
    eng.set_windows(d, bd, bd_off)
    (rh, fh, lh), (rd, fd, ld) = run(eng, h), run(eng, d)
    same_result(rh, rd)
    assert fh == fd and lh == ld
    eng.free_device_batch(h)
    eng.free_device_batch(d)
