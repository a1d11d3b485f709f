"""-m gpu: pg_load_reference_device -- the reference packed on the GPU from device tensors equals the host pack bit for bit."""
import numpy as np
import pytest

from pindel_amd import binding

pytestmark = pytest.mark.gpu

SPACER = 100_000
BIO_LENGTHS = [1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 100_003]
E_INVALID, E_UNSUPPORTED = -1, -6


def _chromosome(rng, length):
    """Random ACGT with runs of N, lower case, IUPAC letters, NUL and bytes >= 128 sprinkled in; spacer-padded."""
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, length)].copy()
    odd = np.frombuffer(b"acgtnNRYKMSWBDHVU-*\x00\x01\x7f\x80\xc1\xff@[`", dtype=np.uint8)
    k = max(1, length // 9)
    s[rng.integers(0, length, k)] = odd[rng.integers(0, len(odd), k)]
    if length > 300:
        for _ in range(3):                                # runs of N, across word boundaries
            at = int(rng.integers(0, length - 200))
            s[at:at + int(rng.integers(1, 150))] = ord("N")
    pad = np.full(SPACER, ord("N"), dtype=np.uint8)
    return np.concatenate([pad, s, pad])


@pytest.fixture(scope="module")
def chroms():
    rng = np.random.default_rng(20261019)
    out = [(f"c{L}", _chromosome(rng, L)) for L in BIO_LENGTHS]
    out[2][1][:5] = np.frombuffer(b"AcGtT", dtype=np.uint8)   # (not only N in the head spacer)
    return out


@pytest.fixture(scope="module")
def engines(engine_factory, chroms):
    """One engine loaded from host bytes, one from the same bytes as device tensors (one an odd-offset slice of a larger tensor)."""
    import torch
    host, dev = engine_factory(), engine_factory()
    host.load_reference([(nm, s.tobytes()) for nm, s in chroms])
    tensors = []
    for k, (nm, s) in enumerate(chroms):
        if k == 7:
            big = torch.zeros(len(s) + 77, dtype=torch.uint8, device="cuda:0")
            big[13:13 + len(s)] = torch.from_numpy(s).to("cuda:0")
            t = big[13:13 + len(s)]
            assert t.data_ptr() % 2 == 1 and t.is_contiguous()
        else:
            t = torch.from_numpy(s).to("cuda:0")
        tensors.append((nm, t))
    dev.load_reference_tensors(tensors)
    return host, dev, tensors


def test_packed_planes_are_byte_identical(engines, tmp_path):
    """save_packed writes the planes as they sit in HBM: guards, tails and trailing words included."""
    host, dev, _ = engines
    a, b = tmp_path / "host.pgref", tmp_path / "dev.pgref"
    host.save_packed(a)
    dev.save_packed(b)
    assert a.read_bytes() == b.read_bytes()


def test_fetch_of_every_chromosome_is_equal(engines, chroms):
    host, dev, _ = engines
    assert host.reference_info() == dev.reference_info()
    for c, (nm, s) in enumerate(chroms):
        got = dev.reference_fetch(c, 0, len(s))
        assert got == host.reference_fetch(c, 0, len(s)), nm
        want = np.where(np.isin(s, np.frombuffer(b"ACGT", dtype=np.uint8)), s, ord("N")).astype(np.uint8)
        assert got == want.tobytes(), nm


def test_fetch_first_then_save(engine_factory, chroms, tmp_path):
    """The lazy mirror is filled by whichever of the two readers comes first; a later host load replaces it."""
    import torch
    eng = engine_factory()
    nm, s = chroms[4]
    eng.load_reference_tensors([(nm, torch.from_numpy(s).to("cuda:0"))])
    first = eng.reference_fetch(0, SPACER - 3, 70)
    other = chroms[5]
    eng.load_reference([(other[0], other[1].tobytes())])
    second = eng.reference_fetch(0, SPACER - 3, 70)
    assert second != first and second[3:67] == bytes(np.where(np.isin(other[1], list(b"ACGT")), other[1], ord("N")).astype(np.uint8)[SPACER:SPACER + 64])
    eng.load_reference_tensors([(nm, torch.from_numpy(s).to("cuda:0"))])
    eng.save_packed(tmp_path / "again.pgref")                 # (the other reader first this time)
    assert eng.reference_fetch(0, SPACER - 3, 70) == first


def test_argument_errors_are_the_host_entrys(engine_factory):
    import ctypes as C
    import torch
    eng = engine_factory()
    L = eng._L

    def both(n, host_ptrs, dev_ptrs, lens):
        names = (C.c_char_p * max(len(lens), 1))(*[b"x"] * len(lens))
        la = (C.c_uint64 * max(len(lens), 1))(*lens)
        hp = (C.c_void_p * max(len(lens), 1))(*host_ptrs)
        dp = (C.c_void_p * max(len(lens), 1))(*dev_ptrs)
        h = L.pg_load_reference(eng._h, n, names, hp, la)
        h_msg = L.pg_last_error(eng._h)
        d = L.pg_load_reference_device(eng._h, n, names, dp, la)
        return h, d, h_msg, L.pg_last_error(eng._h)

    short = np.full(1000, ord("N"), dtype=np.uint8)
    t = torch.from_numpy(short).to("cuda:0")
    h, d, hm, dm = both(0, [short.ctypes.data], [t.data_ptr()], [1000])                  # n_chr limits
    assert h == d == E_INVALID and hm == dm
    h, d, hm, dm = both(40000, [short.ctypes.data], [t.data_ptr()], [1000])
    assert h == d == E_UNSUPPORTED and hm == dm
    h, d, hm, dm = both(1, [short.ctypes.data], [t.data_ptr()], [1000])                  # shorter than its spacers
    assert h == d == E_INVALID and hm == dm and b"spacers" in dm
    h, d, hm, dm = both(1, [short.ctypes.data], [t.data_ptr()], [2 ** 31])               # the 2^31 limit (checked before any read)
    assert h == d == E_UNSUPPORTED and hm == dm
    assert L.pg_load_reference_device(eng._h, 1, None, None, None) == E_INVALID
    # a host pointer, and a length past the allocation: a status, not a fault -- and the engine still loads
    pad = np.full(2 * SPACER + 10, ord("N"), dtype=np.uint8)
    names, la = (C.c_char_p * 1)(b"x"), (C.c_uint64 * 1)(len(pad))
    assert L.pg_load_reference_device(eng._h, 1, names, (C.c_void_p * 1)(pad.ctypes.data), la) == E_INVALID
    assert b"d_seq_padded" in L.pg_last_error(eng._h)
    small = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    la2 = (C.c_uint64 * 1)(1 << 30)
    assert L.pg_load_reference_device(eng._h, 1, names, (C.c_void_p * 1)(small.data_ptr()), la2) == E_INVALID
    eng.load_reference_tensors([("x", torch.from_numpy(pad).to("cuda:0"))])
    assert eng.reference_info() == [("x", len(pad))]
    with pytest.raises(ValueError):
        eng.load_reference_tensors([("x", torch.from_numpy(pad))])                      # a CPU tensor: the wrapper's check


def test_batch_uploaded_before_a_device_reload_is_stale(engines):
    from pindel_amd import synth
    _, dev, tensors = engines
    big = np.frombuffer(tensors[-1][1].cpu().numpy().tobytes(), dtype=np.uint8)
    batch = synth.make_reads(big.tobytes(), 50, seed=3, max_del=2000, insert_size=300, chr_id=len(tensors) - 1)
    db = dev.upload(batch)
    dev.search_device(db)
    dev.load_reference_tensors(tensors)
    with pytest.raises(binding.PgError) as e:
        dev.search_device(db)
    assert e.value.code == E_INVALID and "(re)loaded" in str(e.value)
    dev.free_device_batch(db)
    db = dev.upload(batch)
    dev.search_device(db)
    dev.free_device_batch(db)
