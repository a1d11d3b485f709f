"""The device classifier of the five other kinds (pg_sv_kernel): DI, tandem-duplication and inversion candidates per
read of a searched device batch, against hostlib.sv_candidates -- plain loops around the classifiers' own pair functions -- fed the
points the same search downloaded.  Count bytes and every byte of every record must be equal."""
import numpy as np
import pytest

from pindel_amd import binding, hostlib, synth
from tests import golden_util as gu
from tests import sv_cases
from tests import variant_cases as vc
from tests.test_gpu_variant_candidates import point_csr, searched

pytestmark = pytest.mark.gpu


def expected(eng, chroms, batch, res, prm=None):
    co, cp = point_csr(res.close_off, res.close_runs)
    fo, fp = point_csr(res.far_off, res.far_runs)
    return hostlib.sv_candidates(chroms, batch.seq, batch.seq_off, batch.anchor_strand, batch.chr_id, res.rc_flag, co, cp, fo, fp,
                                 eng.max_mismatch_table(), settings=prm)


def assert_same(got, want, what):
    (gc, gn), (wc, wn) = got, want
    assert gn.shape == wn.shape and gc.shape == wc.shape
    bad = np.nonzero((gn != wn).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: count bytes differ for reads {bad[:8].tolist()}: device {gn[bad[:4]].tolist()}, host {wn[bad[:4]].tolist()}"
    if gc.tobytes() != wc.tobytes():
        for name in wc.dtype.names:
            d = np.argwhere(gc[name] != wc[name])
            assert len(d) == 0, f"{what}: field {name} differs at (read, slot) {d[:6].tolist()}: device {gc[name][tuple(d[0])]}, host {wc[name][tuple(d[0])]}"
        raise AssertionError(f"{what}: the records differ outside their fields")


def run_case(eng, chroms, batch, what, prm=None, bd=None, bd_off=None):
    db, res = searched(eng, chroms, batch, bd, bd_off)
    try:
        got = eng.sv_candidates(db, prm)
        want = expected(eng, chroms, batch, res, prm)
        assert_same(got, want, what)
    finally:
        eng.free_device_batch(db)
    return want, res


def coverage(counts, strand):
    """per kind: reads with a candidate on '+', on '-', with more than one record"""
    listed = counts & 0x7f
    plus = strand == ord("+")
    return {k: np.array([(listed[plus, k - 2] > 0).sum(), (listed[~plus, k - 2] > 0).sum(), (listed[:, k - 2] > 1).sum()]) for k in hostlib.SV_KINDS}


@pytest.fixture(scope="module")
def eng(engine_factory):
    return engine_factory()


@pytest.fixture(scope="module")
def seen():
    """coverage summed over the tests of this module that compare the kernel with the host"""
    return {k: np.zeros(3, dtype=np.int64) for k in hostlib.SV_KINDS}


@pytest.mark.parametrize("read_len", [100, 150])
def test_synthetic_reads(eng, seen, read_len):
    """Reads of all SV types, '+' and '-' anchors, with Pindel's default settings and with others (-e 0.03, -d 45, -v 0)."""
    chroms = [("chrS", synth.make_reference(60_000, seed=41))]
    batch = synth.make_reads(chroms[0][1], 260, read_len=read_len, seed=42 + read_len, mix=(0.2, 0.1, 0.3, 0.3, 0.1))
    for prm in (None, (0.03, 45, 0)):
        (cands, counts), _ = run_case(eng, chroms, batch, f"synthetic {read_len} bp {prm}", prm)
        cov = coverage(counts, batch.anchor_strand)
        # (the synthetic inversions are junctions a '+' anchor sees; the '-' geometries come from tests/sv_cases.py)
        assert cov[3][0] >= 3 and cov[3][1] >= 3 and cov[5][0] >= 3, {hostlib.SV_KINDS[k]: v.tolist() for k, v in cov.items()}
        for k, v in cov.items():
            seen[k] += v


def test_constructed_cases(eng, seen):
    """Every case of tests/sv_cases.py; what a case must show is asserted on the host arrays."""
    for name, chroms, batch, prm in sv_cases.all_cases():
        (cands, counts), res = run_case(eng, chroms, batch, name, prm)
        sv_cases.check_case(name, batch, cands, counts)
        if name == "exact_kernel":
            assert (res.rc_flag[:90] == 1).sum() >= 30 and (res.rc_flag[90:180] == 2).sum() >= 30
        for k, v in coverage(counts, batch.anchor_strand).items():
            seen[k] += v


def test_far_end_on_another_chromosome(eng):
    name, chroms, batch, bd, bd_off = vc.translocation_case()
    (cands, counts), res = run_case(eng, chroms, batch, name, None, bd, bd_off)
    far_chr = np.array([int(res.far_runs[int(res.far_off[i])]["chr_id"]) if res.far_off[i + 1] > res.far_off[i] else -1 for i in range(batch.n)])
    assert (far_chr[:6] == 1).all() and (far_chr[6:] == 0).all()
    assert not counts[:6].any() and not cands[:6].view(np.uint8).any()


def test_coverage(seen):
    """The comparisons above cannot pass on nothing: every kind listed a candidate for '+' and for '-' reads, TD and INV more than one."""
    for k, (p, m, multi) in seen.items():
        assert p > 0 and m > 0, (hostlib.SV_KINDS[k], int(p), int(m))
    assert seen[3][2] > 0 and seen[5][2] > 0


def test_device_entry_and_refusals(eng):
    chroms = [("chrS", synth.make_reference(60_000, seed=41))]
    batch = synth.make_reads(chroms[0][1], 200, seed=77, mix=(0.2, 0.1, 0.3, 0.3, 0.1))
    eng.load_reference(chroms)
    db = eng.upload(batch)
    # not searched yet: refused, by both entries, with nothing launched
    eng.clear_launch_log()
    with pytest.raises(binding.PgError) as e:
        eng.sv_candidates(db)
    assert e.value.code == -1 and "searched" in str(e.value)
    with pytest.raises(binding.PgError):
        eng.sv_candidates_tensors(db)
    assert eng.launch_log() == []
    eng.search_device(db)
    eng.clear_launch_log()
    # a -v that is negative as an int or above 2^30 is refused, by both entries
    for v in (-1, (1 << 30) + 1):
        with pytest.raises(binding.PgError) as e:
            eng.sv_candidates(db, (0.01, 30, v))
        assert e.value.code == -1 and "-v" in str(e.value)
        with pytest.raises(binding.PgError):
            eng.sv_candidates_tensors(db, (0.01, 30, v))
    assert eng.launch_log() == []
    eng.clear_launch_log()
    cands, counts = eng.sv_candidates(db)
    assert [r.kernel for r in eng.launch_log()] == [5]                     # the new kernel's id, and nothing else
    assert eng.last_stats()[0] > 0.0
    assert cands.shape == (batch.n, binding.SV_SLOTS) and counts.shape == (batch.n, binding.SV_KINDS)
    t = eng.sv_candidates_tensors(db)
    assert t["cands"].is_cuda and t["counts"].is_cuda
    assert binding.sv_cands_from_tensor(t["cands"]).tobytes() == cands.tobytes()
    assert t["counts"].cpu().numpy().tobytes() == counts.tobytes()
    assert (counts & 0x7f).any()
    # the largest -v that is accepted runs (and lists no inversion)
    c2, n2 = eng.sv_candidates(db, (0.01, 30, 1 << 30))
    assert not n2[:, 3:].any() and n2[:, :3].tobytes() == counts[:, :3].tobytes()
    # the other classifier is untouched by all this: its own id in the log
    eng.clear_launch_log()
    eng.variant_candidates(db)
    assert [r.kernel for r in eng.launch_log()] == [4]
    # a host pointer for either output is a status code, and nothing is launched
    eng.clear_launch_log()
    L = eng._L
    import ctypes as C
    prm = binding.sv_params(None)
    host_c, host_n = np.zeros_like(cands), np.zeros_like(counts)
    for c_ptr, n_ptr in ((host_c.ctypes.data, t["counts"].data_ptr()), (t["cands"].data_ptr(), host_n.ctypes.data)):
        assert L.pg_device_batch_sv_candidates_device(eng._h, db, C.addressof(prm), c_ptr, n_ptr) == -1
        assert b"not device memory" in L.pg_last_error(eng._h)
    assert eng.launch_log() == []
    eng.free_device_batch(db)
    # an empty batch: nothing to list, nothing launched
    empty = eng.upload(batch.slice(0, 0))
    eng.search_device(empty)
    eng.clear_launch_log()
    c0, n0 = eng.sv_candidates(empty)
    assert c0.shape == (0, binding.SV_SLOTS) and n0.shape == (0, binding.SV_KINDS)
    t0 = eng.sv_candidates_tensors(empty)
    assert t0["cands"].shape[0] == 0
    assert eng.launch_log() == []
    eng.free_device_batch(empty)


def test_gold_set_end_to_end(eng, tmp_path):
    """The gold set searched on the GPU, classified by both device classifiers, windowed and reported on the host: the gold reports."""
    from pindel_amd import hostio
    from tests.test_sv_candidates_cpu import derived_fallbacks as sv_fallbacks
    from tests.test_variant_candidates_cpu import derived_fallbacks as var_fallbacks
    fa, reads_txt = gu.unpack(tmp_path)
    chroms = hostio.load_fasta(fa)
    batch = hostio.read_pindel_text(reads_txt, [n for n, _ in chroms], [len(s) - 200000 for _, s in chroms])
    db, res = searched(eng, chroms, batch)
    var = eng.variant_candidates(db)
    sv = eng.sv_candidates(db)
    eng.free_device_batch(db)
    assert_same(sv, expected(eng, chroms, batch, res), "gold set")
    co, cp = point_csr(res.close_off, res.close_runs)
    fo, fp = point_csr(res.far_off, res.far_runs)
    st = hostlib.default_settings(eng.max_mismatch_table())
    prefix = str(tmp_path / "gpu_lists")
    hostlib.call_from_points(fa, reads_txt, prefix, st, co, cp, fo, fp, res.rc_flag, variant_candidates=var, sv_candidates=sv)
    gu.assert_reports_match_gold(prefix)
    visits = hostlib.last_variant_visits()
    assert set(visits[:, 1].tolist()) == set(range(7))
    want = var_fallbacks(var[0], var[1], batch.insert_size, visits[visits[:, 1] < 2]) + \
        sv_fallbacks(sv[0], sv[1], batch.insert_size, batch.anchor_strand, visits)
    assert hostlib.last_variant_fallbacks() == want
