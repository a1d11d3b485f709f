"""-m gpu: position-keyed hint tables (pg_hint_table) -- the window hints of a read looked up on the device from its close end.
Every table entry point against the per-read entry fed the windows the lookup rule expands to (binding.HintTable.expand, pinned
on the CPU by tests/test_hint_table_cpu.py), and against the oracle."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

from pindel_amd import binding, synth
from pindel_amd.binding import HintTable, WINDOW_DTYPE
from pindel_amd.hostio import ReadBatch
from tests import shortening_cases as sc
from tests.parity import compare_result, points_per_read, run_oracle

pytestmark = pytest.mark.gpu
SPACER = 100000
E_INVALID = -1
SIZES = (700_000, 500_000)


@pytest.fixture(scope="module")
def world(engine_factory):
    """Two chromosomes, 2 000 reads on both (as test_multi_chromosome_and_breakdancer_hints), one engine, the oracle's close end."""
    chroms = [("a", synth.make_reference(SIZES[0], seed=31)), ("b", synth.make_reference(SIZES[1], seed=32))]
    eng = engine_factory()
    eng.load_reference(chroms)
    b0 = synth.make_reads(chroms[0][1], 1200, seed=33, chr_id=0, max_del=200000)
    b1 = synth.make_reads(chroms[1][1], 800, seed=34, chr_id=1, max_del=100000)
    batch = ReadBatch(
        seq=np.concatenate([b0.seq, b1.seq]),
        seq_off=np.concatenate([b0.seq_off, b1.seq_off[1:] + b0.seq_off[-1]]),
        anchor_strand=np.concatenate([b0.anchor_strand, b1.anchor_strand]),
        anchor_pos=np.concatenate([b0.anchor_pos, b1.anchor_pos]),
        insert_size=np.concatenate([b0.insert_size, b1.insert_size]),
        chr_id=np.concatenate([b0.chr_id, b1.chr_id]))
    orc_close = run_oracle({}, chroms, batch, do_far=False)
    cnt = orc_close["close_cnt"][:batch.n]
    last = np.array([int(orc_close["close_pts"][i][cnt[i] - 1]["abs_loc"]) if cnt[i] else 0 for i in range(batch.n)], dtype=np.uint32)
    mx = np.array([int(orc_close["close_pts"][i][cnt[i] - 1]["length"]) if cnt[i] else 0 for i in range(batch.n)], dtype=np.int16)
    return dict(chroms=chroms, eng=eng, batch=batch, close_last=last, close_max=mx)


def _random_windows(rng, n, width=400):
    w = np.zeros(n, dtype=WINDOW_DTYPE)
    w["chr_id"] = rng.integers(0, 2, n)
    size = np.where(w["chr_id"] == 0, SIZES[0], SIZES[1]) + 2 * SPACER
    st = rng.integers(SPACER + 300, size - SPACER - 300 - width)
    w["start"] = st
    w["end"] = st + width
    return w


def _random_table(rng, lo, hi, n_runs, n_clusters, max_per=4, neg_rate=0.05):
    """n_runs runs over [lo, hi), n_clusters clusters of 0 .. max_per windows on both chromosomes (cluster 0 and every seventh
    are empty), some windows with start = -1"""
    cuts = np.sort(rng.choice(np.arange(lo, hi), size=n_runs + 1, replace=False)).astype(np.uint32)
    per = rng.integers(0, max_per + 1, n_clusters)
    per[::7] = 0
    off = np.concatenate([[0], np.cumsum(per)]).astype(np.uint64)
    win = _random_windows(rng, int(off[-1]))
    win["start"][rng.random(len(win)) < neg_rate] = -1
    return HintTable(cuts, rng.integers(0, n_clusters, n_runs), off, win)


def _same_far(a, b):
    np.testing.assert_array_equal(a.far_off, b.far_off)
    assert a.far_runs.tobytes() == b.far_runs.tobytes()


def test_table_paths_equal_the_oracle(world):
    """far_end_batch(hints=) and search_batch(hints=) == the oracle fed the windows the table expands to."""
    eng, chroms, batch = world["eng"], world["chroms"], world["batch"]
    last, mx = world["close_last"], world["close_max"]
    rng = np.random.default_rng(71)
    has = mx > 0
    lo, hi = int(last[has].min()), int(last[has].max())
    # (the outermost reads lie outside the table: 1 000 positions of margin on either side)
    table = _random_table(rng, lo + 1000, hi - 1000, int(rng.integers(200, 401)), 90)
    bd, bd_off = table.expand(last, mx)
    cnt = np.diff(bd_off.astype(np.int64))
    assert (cnt > 0).sum() > 800 and ((cnt == 0) & has).sum() > 50
    assert (bd["chr_id"] != np.repeat(batch.chr_id, cnt)).sum() > 500 and (bd["start"] < 0).sum() > 20
    orc = run_oracle({}, chroms, batch, bd=bd, bd_off=bd_off)
    assert (orc["far_cnt"] > 0).sum() > 500
    close = eng.close_end_batch(batch)
    compare_result(eng.far_end_batch(batch, close, hints=table), orc, batch.n)
    compare_result(eng.search_batch(batch, hints=table), orc, batch.n)
    # and seam 2 on its own, both ways, from the same summary
    kept = _post_state(batch, eng.close_end_batch(batch))
    _same_far(eng.far_end_batch_from_close(kept, last, mx, hints=table), eng.far_end_batch_from_close(kept, last, mx, bd=bd, bd_off=bd_off))


def _post_state(batch, close):
    """the reads as the close end left them (reverse-complemented where rc_flag is set; these reads hold ACGTN only)"""
    lut = np.zeros(256, dtype=np.uint8)
    for x, y in zip(b"ACGTN", b"TGCAN"):
        lut[x] = y
    seq = batch.seq.copy()
    off = batch.seq_off.astype(np.int64)
    for i in np.nonzero(close.rc_flag)[0]:
        seq[off[i]:off[i + 1]] = lut[batch.seq[off[i]:off[i + 1]][::-1]]
    return ReadBatch(seq=seq, seq_off=batch.seq_off, anchor_strand=batch.anchor_strand, anchor_pos=batch.anchor_pos,
                     insert_size=batch.insert_size, chr_id=batch.chr_id)


def _edge_table():
    """Seven runs, hand-made: an empty cluster in the middle, one cluster named by two runs that are not neighbours, a window
    with start = -1, a window on the other chromosome."""
    first = SPACER + np.array([20_000, 20_001, 20_050, 31_000, 31_064, 90_000, 90_003, 150_000], dtype=np.int64)
    cluster = [1, 2, 0, 3, 1, 4, 2]
    win = np.array([(0, SPACER + 200_000, SPACER + 200_400), (0, SPACER + 260_000, SPACER + 260_400),          # cluster 1
                    (0, SPACER + 300_000, SPACER + 300_400),                                                  # cluster 2
                    (1, SPACER + 180_000, SPACER + 180_400), (0, -1, SPACER + 370_000), (0, SPACER + 380_000, SPACER + 380_400),   # 3
                    (0, SPACER + 400_000, SPACER + 400_400)], dtype=WINDOW_DTYPE)                              # cluster 4
    return HintTable(first, cluster, [0, 0, 2, 3, 6, 7], win)


def _junction_reads(chroms, far_win, seed):
    """One 100-base split read per entry of far_win, anchored '-' on chromosome a: 60 bases that end in the middle of the
    window far_win[k] (on either chromosome) + 40 bases of chromosome a next to the anchor (the close end).  The far end lies
    nowhere near the anchor: only a search of that window finds it."""
    from pindel_amd import hostio
    rng = np.random.default_rng(seed)
    biol = [np.frombuffer(s, dtype=np.uint8)[SPACER:-SPACER] for _, s in chroms]
    seqs, poss = [], []
    for w in far_win:
        q = int(w["end"]) - 200 - SPACER
        p = int(rng.integers(540_000, 640_000))              # (clear of the N gaps, the repeat family and the microsatellite)
        seqs.append(np.concatenate([biol[int(w["chr_id"])][q - 60:q], biol[0][p:p + 40]]).tobytes())
        poss.append(p + 40 + int(rng.integers(150, 300)))
    n = len(seqs)
    return hostio.batch_from_lists(seqs, [b"-"] * n, poss, [500] * n, [0] * n)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_lookup_edges(world, n):
    """close_last set by hand to every run boundary and the position before it (first and last included), some reads without a
    close end; batches at the wave and block seams of count, scan and fill.  Every read is a junction read whose far end lies
    in a window of the cluster its position names (or, for a position without windows, in a window it does not get), so what
    the lookup hands the far end decides what it finds."""
    eng, chroms = world["eng"], world["chroms"]
    table = _edge_table()
    pos = np.sort(np.concatenate([table.run_first.astype(np.int64), table.run_first.astype(np.int64) - 1]))
    i = np.arange(n)
    last = pos[(i + n) % len(pos)].astype(np.uint32)
    bd1, off1 = table.expand(last, np.ones(n, dtype=np.int16))
    cnt1 = np.diff(off1.astype(np.int64))
    far_win = [bd1[int(off1[k]) + k % cnt1[k]] if cnt1[k] else table.windows[0] for k in range(n)]
    raw = _junction_reads(chroms, far_win, seed=200 + n)
    close = eng.close_end_batch(raw)
    has, _, real_mx = sc.close_back(close)
    batch = _post_state(raw, close)
    mx = np.where(i % 5 == 3, 0, real_mx).astype(np.int16)
    bd, bd_off = table.expand(last, mx)
    cnt = np.diff(bd_off.astype(np.int64))
    want_cnt = {int(p): c for p, c in zip(pos, [0, 2, 2, 1, 1, 0, 0, 3, 3, 2, 2, 1, 1, 1, 1, 0])}
    for k in range(n):
        assert cnt[k] == (want_cnt[int(last[k])] if mx[k] > 0 else 0)
    got = eng.far_end_batch_from_close(batch, last, mx, hints=table)
    want = eng.far_end_batch_from_close(batch, last, mx, bd=bd, bd_off=bd_off)
    assert got.n == n
    _same_far(got, want)
    if n == 4097:
        # the windows matter: 4097 x 12/16 positions with windows x 4/5 reads not switched off = 2 458 reads are handed the
        # window their far end lies in (fewer where the close end was not found or the window has start = -1)
        plain = eng.far_end_batch_from_close(batch, last, mx)
        with_w = points_per_read(got.far_off, got.far_runs) > 0
        without = points_per_read(plain.far_off, plain.far_runs) > 0
        print(f"edges: close end {int(has.sum())}, windows for {int((cnt > 0).sum())}, far end through the table "
              f"{int(with_w.sum())} ({int((with_w & (cnt > 0)).sum())} of them with windows), without windows {int(without.sum())}")
        assert has.sum() > 3000 and (with_w & ~without & (cnt > 0)).sum() > 1500
        assert not with_w[mx == 0].any()


def test_scan_across_blocks(world):
    """70 000 reads: 69 tiles of the scan (block sums, their scan, add), both GPU paths from the same close end."""
    eng, chroms = world["eng"], world["chroms"]
    batch = synth.make_reads(chroms[0][1], 70_000, seed=91, chr_id=0)
    c1 = eng.close_end_batch(batch)
    has, last, mx = sc.close_back(c1)
    rng = np.random.default_rng(92)
    table = _random_table(rng, int(last[has].min()) + 500, int(last[has].max()) - 500, 24, 9, max_per=5)
    bd, bd_off = table.expand(last, mx)
    cnt = np.diff(bd_off.astype(np.int64))
    assert has.sum() > 30_000 and (cnt > 0).sum() > 5_000 and len(set(cnt.tolist())) >= 4
    got = eng.far_end_batch(batch, c1, hints=table)
    want = eng.far_end_batch(batch, eng.close_end_batch(batch), bd=bd, bd_off=bd_off)
    _same_far(got, want)
    np.testing.assert_array_equal(got.close_off, want.close_off)
    assert got.close_runs.tobytes() == want.close_runs.tobytes() and np.array_equal(got.rc_flag, want.rc_flag)
    assert (points_per_read(got.far_off, got.far_runs) > 0).sum() > 10_000
    fused = eng.search_batch(batch, hints=table)
    _same_far(fused, want)
    np.testing.assert_array_equal(fused.close_off, want.close_off)
    assert fused.close_runs.tobytes() == want.close_runs.tobytes() and np.array_equal(fused.rc_flag, want.rc_flag)


def _search_records(eng):
    return [r for r in eng.launch_log() if r.kernel == 1]


def test_clusters_of_300_windows(world):
    """The shape of test_more_than_127_windows_in_a_cluster as a table: 300 windows per cluster, 64-bit candidate ids on both
    paths (the same search record in the launch log), == the oracle."""
    eng, chroms = world["eng"], world["chroms"]
    batch = synth.make_reads(chroms[0][1], 600, seed=43)
    close = eng.close_end_batch(batch)
    has, last, mx = sc.close_back(close)
    rng = np.random.default_rng(44)
    per, n_clusters = 300, 12
    win = _random_windows(rng, per * n_clusters)
    win["end"] = win["start"] + rng.integers(50, 400, len(win))
    win["start"][rng.random(len(win)) < 0.02] = -1
    lo, hi = int(last[has].min()), int(last[has].max()) + 1
    cuts = np.unique(np.linspace(lo, hi, 41).astype(np.int64))
    table = HintTable(cuts, np.arange(len(cuts) - 1) % n_clusters, np.arange(n_clusters + 1) * per, win)
    bd, bd_off = table.expand(last, mx)
    assert (np.diff(bd_off.astype(np.int64)) == per).sum() == has.sum() > 300
    orc = run_oracle({}, chroms, batch, bd=bd, bd_off=bd_off)
    eng.clear_launch_log()
    got = eng.far_end_batch(batch, close, hints=table)
    rec_table = [r for r in _search_records(eng) if r.mode == 2]
    compare_result(got, orc, batch.n)
    eng.clear_launch_log()
    want = eng.far_end_batch(batch, eng.close_end_batch(batch), bd=bd, bd_off=bd_off)
    rec_csr = [r for r in _search_records(eng) if r.mode == 2]
    _same_far(got, want)
    assert rec_table == rec_csr and len(rec_table) == 1 and rec_table[0].id_bits == 64
    assert (orc["far_cnt"] > 0).sum() > 200


def test_window_of_more_than_2_26_positions_as_a_table(engine_factory):
    """The window of test_window_of_more_than_2_26_positions as a one-cluster table: split into pieces once, at upload."""
    n_bases = (1 << 26) + 700_000
    ref = [("chrW", synth.make_reference(n_bases, seed=51))]
    eng = engine_factory()
    eng.load_reference(ref)
    batch = synth.make_reads(ref[0][1], 6, seed=52)
    win = np.zeros(1, dtype=WINDOW_DTYPE)
    win["start"] = SPACER + 1000
    win["end"] = SPACER + 1000 + (1 << 26) + 5000
    table = HintTable([0, 0xffffffff], [0], [0, 1], win)
    bd = np.repeat(win, batch.n)
    bd_off = np.arange(batch.n + 1).astype(np.uint64)
    orc = run_oracle({}, ref, batch, bd=bd, bd_off=bd_off)
    # (a read without a close end gets no windows from the table; the oracle searches no far end for it either way)
    compare_result(eng.search_batch(batch, hints=table), orc, batch.n)
    compare_result(eng.far_end_batch(batch, eng.close_end_batch(batch), hints=table), orc, batch.n)
    assert (orc["close_cnt"] > 0).sum() >= 3
    eng.close()


def _code(fn):
    with pytest.raises(binding.PgError) as e:
        fn()
    return e.value.code, str(e.value)


def test_malformed_tables_are_refused(world):
    eng, chroms, batch = world["eng"], world["chroms"], world["batch"].slice(0, 300)
    last, mx = world["close_last"][:300], world["close_max"][:300]
    good = _edge_table()
    rf, rc, co, w = good.run_first, good.run_cluster, good.cluster_off, good.windows
    unsorted = rf.copy()
    unsorted[3] = unsorted[2]                                # not STRICTLY ascending
    bad_cluster = rc.copy()
    bad_cluster[4] = 5                                       # n_clusters is 5
    bad_off = co.copy()
    bad_off[2], bad_off[3] = bad_off[3], bad_off[2]
    bad_chr = w.copy()
    bad_chr["chr_id"][2] = 2
    neg_chr = w.copy()
    neg_chr["chr_id"][0] = -1
    cases = {"run_first": HintTable(unsorted, rc, co, w), "run_cluster": HintTable(rf, bad_cluster, co, w),
             "cluster_off": HintTable(rf, rc, bad_off, w), "unknown chromosome": HintTable(rf, rc, co, bad_chr),
             "unknown chromosome ": HintTable(rf, rc, co, neg_chr)}
    for what, t in cases.items():
        for call in (lambda: eng.search_batch(batch, hints=t), lambda: eng.far_end_batch_from_close(batch, last, mx, hints=t),
                     lambda: eng.far_end_batch(batch, eng.close_end_batch(batch), hints=t)):
            code, msg = _code(call)
            assert code == E_INVALID and what.strip() in msg, (what, code, msg)
    # null arrays with non-zero counts
    L = binding.lib()
    s, keep = binding._batch_struct(batch)
    for field in ("run_first", "run_cluster", "cluster_off", "windows"):
        t = good.struct()
        setattr(t, field, None)
        h = C.c_void_p()
        assert L.pg_search_batch_table(eng._h, C.byref(s), C.byref(t), C.byref(h)) == E_INVALID, field
        assert b"null" in L.pg_last_error(eng._h) and not h.value
    # a null table and a table without runs are "no hints"; the engine still searches correctly
    orc = run_oracle({}, chroms, batch)
    compare_result(eng.search_batch(batch, hints=HintTable([], [], [0], np.zeros(0, WINDOW_DTYPE))), orc, batch.n)
    h = C.c_void_p()
    assert L.pg_search_batch_table(eng._h, C.byref(s), None, C.byref(h)) == 0
    compare_result(binding.Result(h, eng), orc, batch.n)
    bd, bd_off = good.expand(last, mx)
    compare_result(eng.search_batch(batch, hints=good), run_oracle({}, chroms, batch, bd=bd, bd_off=bd_off), batch.n)
    none = eng.search_batch(batch.slice(0, 0), hints=good)     # ... and nobody to look up
    assert none.n == 0 and len(none.close_runs) == 0 and len(none.far_runs) == 0


# ------------------------------------------------------------------------------------------ command line
EXE = os.path.join(os.path.dirname(binding.LIB_PATH), "pindel_pg")


def _run(args, env=None):
    e = dict(os.environ)
    e.pop("PGH_THREADS", None)
    e.pop("PGH_HINT_LOOKUP", None)
    e.update(env or {})
    out = subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, env=e)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


def _reports(prefix):
    out = {}
    for f in sorted(glob.glob(f"{prefix}_*")):
        with open(f, "rb") as fh:
            out[os.path.basename(f)[len(os.path.basename(str(prefix))):]] = fh.read()
    return out


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    from tests import interchr_synth as syn
    return syn.make(str(tmp_path_factory.mktemp("hint_cli")))


@pytest.mark.parametrize("route", ["bam", "text"])
def test_command_line_reports_do_not_depend_on_where_the_lookup_runs(sample, tmp_path, route):
    from tests import interchr_synth as syn
    s = sample
    if route == "bam":
        args = ["-f", s["fasta"], "-i", s["config"], "-w", syn.WINDOW_MBP, "-I"]
    else:
        args = ["-f", s["fasta"], "-p", s["reads_txt"], "-b", s["bd"], "--bd-hints", "on", "-w", syn.WINDOW_MBP, "-I"]
    dev = _run(args + ["-o", tmp_path / "dev"])
    host = _run(args + ["-o", tmp_path / "host"], env={"PGH_HINT_LOOKUP": "host"})
    a, b = _reports(tmp_path / "dev"), _reports(tmp_path / "host")
    assert set(a) == set(b) and {"_D", "_INT", "_INT_final"} <= set(a)
    for suf in a:
        assert a[suf] == b[suf], suf
    assert len(a["_INT"]) > 0
    n_dev, n_host = dev.count("Window hints: device lookup"), host.count("Window hints: host lookup")
    assert n_dev == n_host >= 3 and "host lookup" not in dev and "device lookup" not in host
    assert n_dev <= dev.count("Close_end_found")             # once per window, and only for the hinted ones
