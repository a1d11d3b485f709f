"""The device classifier (pg_variant_kernel): deletion and short-insertion candidates per read of a searched device
batch, against hostlib.variant_candidates -- the classifier's own loops on the host -- fed the points the same search
downloaded.  Count bytes and every byte of every candidate record must be equal."""
import numpy as np
import pytest

from pindel_amd import binding, hostlib, synth
from tests import golden_util as gu
from tests import shortening_cases as sc
from tests import variant_cases as vc

pytestmark = pytest.mark.gpu


def point_csr(off, runs):
    per_run = runs["len_last"].astype(np.int64) - runs["len_first"].astype(np.int64) + 1
    cum = np.concatenate([[0], np.cumsum(per_run)])
    return cum[off.astype(np.int64)].astype(np.uint64), binding.expand_runs(runs)


def searched(eng, chroms, batch, bd=None, bd_off=None):
    """(device batch, downloaded result) of one search on the device"""
    eng.load_reference(chroms)
    db = eng.upload(batch)
    if bd is not None:
        eng.set_windows(db, bd, bd_off)
    eng.search_device(db)
    return db, eng.download(db)


def expected(eng, chroms, batch, res):
    co, cp = point_csr(res.close_off, res.close_runs)
    fo, fp = point_csr(res.far_off, res.far_runs)
    return hostlib.variant_candidates(chroms, batch.seq, batch.seq_off, batch.anchor_strand, batch.chr_id, res.rc_flag, co, cp, fo, fp,
                                      eng.max_mismatch_table())


def assert_same(got, want, what):
    (gc, gn), (wc, wn) = got, want
    assert gn.shape == wn.shape and gc.shape == wc.shape
    bad = np.nonzero((gn != wn).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: count bytes differ for reads {bad[:8].tolist()}: device {gn[bad[:4]].tolist()}, host {wn[bad[:4]].tolist()}"
    if gc.tobytes() != wc.tobytes():
        for name in wc.dtype.names:
            d = np.argwhere(gc[name] != wc[name])
            assert len(d) == 0, f"{what}: field {name} differs at (read, kind, place) {d[:6].tolist()}: device {gc[name][tuple(d[0])]}, host {wc[name][tuple(d[0])]}"
        raise AssertionError(f"{what}: the records differ outside their fields")


def run_case(eng, chroms, batch, what, bd=None, bd_off=None):
    db, res = searched(eng, chroms, batch, bd, bd_off)
    try:
        got = eng.variant_candidates(db)
        want = expected(eng, chroms, batch, res)
        assert_same(got, want, what)
    finally:
        eng.free_device_batch(db)
    return want, res


@pytest.fixture(scope="module")
def eng(engine_factory):
    return engine_factory()


@pytest.mark.parametrize("read_len", [100, 150])
def test_synthetic_reads(eng, read_len):
    """Reads of all SV types with default parameters, '+' and '-' anchors."""
    chroms = [("chrS", synth.make_reference(60_000, seed=41))]
    batch = synth.make_reads(chroms[0][1], 260, read_len=read_len, seed=42 + read_len)
    (cands, counts), _ = run_case(eng, chroms, batch, f"synthetic {read_len} bp")
    listed = counts & 0x7f
    plus = batch.anchor_strand == ord("+")
    for kind in (0, 1):
        assert (listed[plus, kind] > 0).sum() >= 5 and (listed[~plus, kind] > 0).sum() >= 5
    assert (listed > 1).any()


def test_repeats_and_long_walks(eng):
    seen = {}
    for name, chroms, batch in vc.repeat_cases():
        (cands, counts), _ = run_case(eng, chroms, batch, name)
        seen[name] = (cands, counts)
        assert (counts[:, 0] & 0x7f).all(), name                       # every read is a deletion call
    # the decoy leaves the first close point 71 repeat bases into the run: BP moves back by the whole left walk (more than a
    # step of 64), or to the N that ends it
    for unit in ("A", "CT"):
        c = seen[f"long_left_walk_{unit}"][0][0, 0, 0]
        n = seen[f"long_left_walk_n_{unit}"][0][0, 0, 0]
        assert c["bp"] == 29 and n["bp"] == 29 + 31 and n["bp_left"] == c["bp_left"] + 31
    assert (seen["homopolymer"][1][:, 0] & hostlib.VARIANT_MORE).all()


def test_order_of_pairs(eng):
    for name, chroms, batch in vc.microhomology_cases():
        (cands, counts), res = run_case(eng, chroms, batch, name)
        plus = batch.anchor_strand == ord("+")
        full = (counts[:, 0] & 0x7f) == hostlib.VARIANT_CANDS
        assert full.all(), name
        if name == "microhomology8":
            assert (counts[:, 0] & hostlib.VARIANT_MORE).all()           # nine pairs without a mismatch alone
        if name.startswith("microhomology"):
            # without a mismatch the close points come ascending for a '+' anchor, descending for a '-' anchor
            d = np.diff(cands["close_idx"][:, 0].astype(np.int64), axis=1)
            assert (d[plus] == 1).all() and (d[~plus] == -1).all()
            far_runs = np.diff(res.far_off.astype(np.int64))
            assert (far_runs > 1).any()                                    # a mismatch deep in the far part: two far runs
        if name == "budget_order":
            # the pairs without a mismatch first, although pairs with one come earlier among the close points
            ci = cands["close_idx"][:, 0].astype(np.int64)
            assert (ci[plus][:, 2] < ci[plus][:, 0]).all() and (ci[~plus][:, 2] > ci[~plus][:, 0]).all()


def test_long_reads_and_insertions(eng):
    for name, chroms, batch in vc.long_read_cases() + vc.insertion_cases() + vc.chromosome_end_case():
        (cands, counts), _ = run_case(eng, chroms, batch, name)
        listed = counts & 0x7f
        assert (listed.sum(axis=1) > 0).all(), name
        if name == "long_reads":
            assert cands["close_idx"][listed > 0].max() > 128             # the lane loop's third round
        if name == "insertions":
            assert (listed[:, 1] > 1).all() and (cands["nt_rot"][:, 1, 1] < 0).all()
            assert sorted(set(cands["indel_size"][:, 1, 0].tolist())) == [1, 3, 5, 6]
        assert not cands["flags"].any()


def test_far_end_on_another_chromosome(eng):
    name, chroms, batch, bd, bd_off = vc.translocation_case()
    (cands, counts), res = run_case(eng, chroms, batch, name, bd, bd_off)
    far_chr = np.array([int(res.far_runs[int(res.far_off[i])]["chr_id"]) if res.far_off[i + 1] > res.far_off[i] else -1 for i in range(batch.n)])
    assert (far_chr[:6] == 1).all() and (far_chr[6:] == 0).all()
    assert not counts[:6].any() and (counts[6:, 0] & 0x7f).all()


def test_reads_of_the_exact_kernel(eng):
    """Reads with characters outside ACGTN: shortened by the first reverse complement ("R" + RC(c): rc_flag 1), by both (c + "R" with
    a moved anchor: rc_flag 2), and with one inside.  ReadLength, MAX_SNP_ERROR and the bases are the post-state's: 126 -> 125 bases
    takes a mismatch level away."""
    chroms = [("chrS", synth.make_reference(400_000, seed=3))]
    for L in (100, 125):
        clean = sc.clean_reads(chroms[0][1], 120, L, seed=900 + L)
        batch = sc.concat([sc.lead_case(clean, b"R"), sc.trail_case(sc.moved(clean), b"RK"), sc.inner_case(sc.moved(clean), L // 2), clean])
        (cands, counts), res = run_case(eng, chroms, batch, f"exact kernel {L}")
        listed = counts & 0x7f
        for k, flag in enumerate((1, 2)):
            part = slice(120 * k, 120 * (k + 1))
            hit = (res.rc_flag[part] == flag) & (listed[part].sum(axis=1) > 0)
            assert hit.sum() >= 10, (L, flag, int(hit.sum()))
        assert (listed[360:].sum(axis=1) > 0).sum() >= 10


def test_device_entry_and_refusals(eng):
    chroms = [("chrS", synth.make_reference(60_000, seed=41))]
    batch = synth.make_reads(chroms[0][1], 200, seed=77)
    eng.load_reference(chroms)
    db = eng.upload(batch)
    # not searched yet: refused, by both entries, with nothing launched
    eng.clear_launch_log()
    with pytest.raises(binding.PgError) as e:
        eng.variant_candidates(db)
    assert e.value.code == -1 and "searched" in str(e.value)
    with pytest.raises(binding.PgError):
        eng.variant_candidates_tensors(db)
    assert eng.launch_log() == []
    eng.search_device(db)
    eng.clear_launch_log()
    cands, counts = eng.variant_candidates(db)
    assert [r.kernel for r in eng.launch_log()] == [4]
    assert eng.last_stats()[0] > 0.0
    t = eng.variant_candidates_tensors(db)
    assert t["cands"].is_cuda and t["counts"].is_cuda
    assert binding.variant_cands_from_tensor(t["cands"]).tobytes() == cands.tobytes()
    assert t["counts"].cpu().numpy().tobytes() == counts.tobytes()
    assert (counts & 0x7f).any()
    # a host pointer for either output is a status code, and nothing is launched
    eng.clear_launch_log()
    L = eng._L
    host_c, host_n = np.zeros_like(cands), np.zeros_like(counts)
    for c_ptr, n_ptr in ((host_c.ctypes.data, t["counts"].data_ptr()), (t["cands"].data_ptr(), host_n.ctypes.data)):
        assert L.pg_device_batch_variant_candidates_device(eng._h, db, c_ptr, n_ptr) == -1
        assert b"not device memory" in L.pg_last_error(eng._h)
    assert eng.launch_log() == []
    eng.free_device_batch(db)
    # an empty batch: nothing to list, nothing launched
    empty = eng.upload(batch.slice(0, 0))
    eng.search_device(empty)
    eng.clear_launch_log()
    c0, n0 = eng.variant_candidates(empty)
    assert c0.shape == (0, 2, binding.VARIANT_CANDS) and n0.shape == (0, 2)
    t0 = eng.variant_candidates_tensors(empty)
    assert t0["cands"].shape[0] == 0
    assert eng.launch_log() == []
    eng.free_device_batch(empty)


def test_gold_set_end_to_end(eng, tmp_path):
    """The gold set searched on the GPU, classified on the GPU, windowed and reported on the host: the gold reports."""
    from pindel_amd import hostio
    from tests.test_variant_candidates_cpu import derived_fallbacks
    fa, reads_txt = gu.unpack(tmp_path)
    chroms = hostio.load_fasta(fa)
    batch = hostio.read_pindel_text(reads_txt, [n for n, _ in chroms], [len(s) - 200000 for _, s in chroms])
    db, res = searched(eng, chroms, batch)
    got = eng.variant_candidates(db)
    eng.free_device_batch(db)
    assert_same(got, expected(eng, chroms, batch, res), "gold set")
    co, cp = point_csr(res.close_off, res.close_runs)
    fo, fp = point_csr(res.far_off, res.far_runs)
    st = hostlib.default_settings(eng.max_mismatch_table())
    prefix = str(tmp_path / "gpu_lists")
    hostlib.call_from_points(fa, reads_txt, prefix, st, co, cp, fo, fp, res.rc_flag, variant_candidates=got)
    gu.assert_reports_match_gold(prefix)
    assert hostlib.last_variant_fallbacks() == derived_fallbacks(got[0], got[1], batch.insert_size, hostlib.last_variant_visits())
