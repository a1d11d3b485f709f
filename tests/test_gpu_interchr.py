"""-m gpu: `pindel_pg -I` on the MI355X against the oracle-fed pipeline (ingest and window hints through the host library's C
entries, search by the CPU oracle, _RP / _INT / _INT_final by the independent restatement tests/interchr_restated.py), and
the search engine at the shapes -I produces: window clusters on more chromosomes than the kernel's LDS table holds."""
import glob
import os
import subprocess

import numpy as np
import pytest

from pindel_amd import binding, hostio, synth
from tests import interchr_common as ic
from tests import interchr_restated as ir
from tests import interchr_synth as syn
from tests.parity import compare_result, run_oracle
from tests.test_bam_ingest import ingest
from tests.test_interchr_cpu import _text_route_expected, check_sample_reports

pytestmark = pytest.mark.gpu
SPACER = ic.SPACER
EXE = os.path.join(os.path.dirname(binding.LIB_PATH), "pindel_pg")
REPORTS = ("_D", "_SI", "_TD", "_INV")


def _run(args, env=None):
    e = dict(os.environ)
    e.pop("PGH_THREADS", None)
    e.update(env or {})
    out = subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, env=e)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def _bam_route_expected(s):
    """window by window as run_bam_pipeline walks them: ingest, oracle close end, the hints of the window (read pairs of both
    kinds), oracle far end -> (_RP text, read lists per window [(chr, ws, reads)], reads with a close end, with a far end)"""
    L = ic.lib()
    names = list(syn.NAMES)
    chroms = hostio.load_fasta(s["fasta"])
    rp_text, per_window = "", []
    n_close = n_far = 0
    for cid, (name, seq) in enumerate(chroms):
        for ws, we in syn.windows():
            pairs = ic.discover_interchr(s["records"], cid, ws, we, syn.ISZ, syn.TAG, names)
            want_ev, want_rp = ir.rp_interchr(pairs, SPACER)
            rp_text += want_rp
            got = ingest(s["bam"], name, cid, len(seq), ws, we, syn.ISZ, tag=syn.TAG)
            if not got:
                continue
            b = ic.batch_of(got, cid)
            events = []

            def windows_of(last):
                off = np.zeros(b.n + 1, dtype=np.uint64)
                win = np.zeros(3 * 8192, dtype=np.int32)
                ev = np.zeros(6 * 64, dtype=np.int64)
                n_ev = L.pgh_window_hints_chr(None, s["bam"].encode(), len(names), ic.c_names(names), cid, ws, we, we, syn.ISZ,
                                              syn.TAG.encode(), 0, SPACER, 1, b.n, last.ctypes.data, off.ctypes.data, win.ctypes.data, 8192,
                                              ev.ctypes.data, 64)
                assert n_ev >= 0, L.pgh_last_error()
                events.extend(ic.events_from(ev, n_ev, names))
                return off, win[:3 * int(off[-1])]
            res = ic.oracle_with_windows(chroms, b, windows_of)
            assert events == want_ev                          # the hints entry hands the search the restatement's events
            n_close += int((res["close_cnt"] > 0).sum())
            n_far += int((res["far_cnt"] > 0).sum())
            per_window.append((name, ws, ic.restated_reads(names, chroms, got, res, name)))
    return rp_text, per_window, n_close, n_far


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    d = tmp_path_factory.mktemp("interchr")
    return d, syn.make(str(d))


def test_i_on_the_synthetic_bam_equals_the_oracle_fed_pipeline(sample):
    d, s = sample
    base = ["-f", s["fasta"], "-i", s["config"], "-w", syn.WINDOW_MBP]
    so = _run(base + ["-I", "-o", d / "on"])
    want_rp, per_window, n_close, n_far = _bam_route_expected(s)
    want_int, want_final, collected = ic.int_reports([reads for _, _, reads in per_window])
    check_sample_reports(per_window, want_int, want_final)
    assert f"close end {n_close}, far end {n_far}" in so, so[-600:]
    assert _read(d / "on_RP").decode() == want_rp and want_rp.count("\n") >= 6
    assert _read(d / "on_INT").decode() == want_int
    assert _read(d / "on_INT_final").decode() == want_final
    # the other reports do not change with -I, and `-I false` is no -I: the same files with the same bytes, no _INT
    _run(base + ["-o", d / "plain"])
    _run(base + ["-I", "false", "-o", d / "off"])
    # (no junction read of the sample has a chance far end near its anchor -- tests/interchr_synth.py asks the oracle -- so what
    # the hints of -I change in the search cannot reach these reports; the planted deletion is called in both runs)
    for suf in REPORTS:
        assert _read(f"{d}/on{suf}") == _read(f"{d}/plain{suf}"), suf
    assert b"\tD %d\t" % syn.DEL_LEN in _read(f"{d}/plain_D")
    files = lambda p: sorted(os.path.basename(f)[len(p):] for f in glob.glob(f"{d}/{p}_*"))
    assert files("off") == files("plain") and "_INT" not in files("plain") and "_INT_final" not in files("plain")
    assert set(files("on")) == set(files("plain")) | {"_INT", "_INT_final"}
    for suf in files("plain"):
        assert _read(f"{d}/off{suf}") == _read(f"{d}/plain{suf}"), suf
    # -S with -I: no far end, two empty files, no error
    _run(base + ["-I", "-S", "-o", d / "close_only"])
    assert os.path.getsize(d / "close_only_INT") == 0 and os.path.getsize(d / "close_only_INT_final") == 0


def test_i_does_not_depend_on_threads_or_devices(sample):
    d, s = sample
    base = ["-f", s["fasta"], "-i", s["config"], "-w", syn.WINDOW_MBP, "-I"]
    runs = {"t1": ["-T", "1"], "t16": ["-T", "16"], "g1": ["-G", "0"], "g3": ["-G", "0,0,0"]}
    for k, extra in runs.items():
        _run(base + extra + ["-o", d / k])
    assert os.path.getsize(d / "t1_INT") > 0 and os.path.getsize(d / "t1_INT_final") > 0
    for suf in REPORTS + ("_RP", "_INT", "_INT_final"):
        want = _read(f"{d}/t1{suf}")
        for k in ("t16", "g1", "g3"):
            assert _read(f"{d}/{k}{suf}") == want, (k, suf)


def test_text_route_with_bd_hints(sample, tmp_path):
    d, s = sample
    args = ["-f", s["fasta"], "-p", s["reads_txt"], "-b", s["bd"], "--bd-hints", "on", "-w", syn.WINDOW_MBP]
    so = _run(args + ["-I", "-o", tmp_path / "text"])
    csr, per_window = _text_route_expected(s, tmp_path)
    want_int, want_final, collected = ic.int_reports([reads for _, _, reads in per_window])
    check_sample_reports(per_window, want_int, want_final)
    assert _read(tmp_path / "text_INT").decode() == want_int
    assert _read(tmp_path / "text_INT_final").decode() == want_final
    assert "far end %d" % sum(1 for _, _, reads in per_window for r in reads if r["UP_Far"]) in so, so[-600:]
    # without a hint source -I is legal: a note and two empty files
    so = _run(["-f", s["fasta"], "-p", s["reads_txt"], "-w", syn.WINDOW_MBP, "-I", "-o", tmp_path / "nohints"])
    assert "-I without window hints" in so
    assert os.path.getsize(tmp_path / "nohints_INT") == 0 and os.path.getsize(tmp_path / "nohints_INT_final") == 0


N_CHR = 30          # more than PG_CHR_TAB = 24 (pindel_amd/csrc/pg_kernels.hip)


def _translocation_batch(chroms, read_len, n, seed):
    """n reads anchored on a random chromosome whose other part comes from another one (at least a third of them from
    chromosomes 24-29), each with 0-4 window clusters: the true far end among decoys on any chromosome."""
    from pindel_amd.binding import WINDOW_DTYPE
    rng = np.random.default_rng(seed)
    comp = np.zeros(256, np.uint8)
    for x, y in zip(b"ACGTN", b"TGCAN"):
        comp[x] = y
    biol = [np.frombuffer(s, dtype=np.uint8)[SPACER:-SPACER] for _, s in chroms]
    seqs, strands, poss, inss, cids, wins, offs = [], [], [], [], [], [], [0]
    for i in range(n):
        c = int(rng.integers(0, N_CHR))
        far_c = int(rng.integers(24, N_CHR)) if i % 3 == 0 else int(rng.integers(0, N_CHR))
        if far_c == c:
            far_c = (c + 1) % N_CHR if c < 24 or i % 3 else 24 + (c - 24 + 1) % 6
        k = int(rng.integers(read_len // 3, 2 * read_len // 3))
        p = int(rng.integers(2000, len(biol[c]) - 2000))
        q = int(rng.integers(2000, len(biol[far_c]) - 2000))
        isz = 500
        if rng.random() < 0.5:                                  # '+' anchor left of the junction, read = c[p-k:p] + far[q:...]
            read = np.concatenate([biol[c][p - k:p], biol[far_c][q:q + read_len - k]])
            seqs.append(comp[read[::-1]].tobytes())
            strands.append(b"+")
            poss.append(p - k - int(rng.integers(150, 300)))
        else:                                                   # '-' anchor right of it, read = far[...:q] + c[p:p+k]
            read = np.concatenate([biol[far_c][q - (read_len - k):q], biol[c][p:p + k]])
            seqs.append(read.tobytes())
            strands.append(b"-")
            poss.append(p + k + int(rng.integers(150, 300)))
        inss.append(isz)
        cids.append(c)
        n_win = int(rng.integers(0, 5))
        true_at = int(rng.integers(0, n_win)) if n_win else -1
        for w in range(n_win):
            if w == true_at:
                wc, centre = far_c, q + SPACER
            else:
                wc = int(rng.integers(24, N_CHR)) if rng.random() < 0.4 else int(rng.integers(0, N_CHR))
                centre = int(rng.integers(2000, len(biol[wc]) - 2000)) + SPACER
            wins.append((wc, centre - 300, centre + 300))
        offs.append(len(wins))
    batch = hostio.batch_from_lists(seqs, strands, poss, inss, cids)
    return batch, np.array(wins, dtype=WINDOW_DTYPE), np.array(offs, dtype=np.uint64)


@pytest.mark.parametrize("read_len", [100, 150, 250])
def test_cross_chromosome_clusters_beyond_the_lds_table(engine_factory, read_len):
    """30 chromosomes, more than the 24 of the kernel's LDS chromosome table: with 100-bp reads the table is in LDS and
    chromosomes 24-29 fall through to global loads, with 150- and 250-bp reads there is no table at all.  0-4 window clusters
    per read, a third of the true far ends on chromosomes 24-29, through far_end_batch and through set_windows + search_device.
    (test_many_chromosomes_150bp stops at exactly 24 chromosomes and has no windows.)"""
    chroms = [(f"c{c:02d}", synth.make_reference(260_000 + 3_000 * c, seed=900 + c)) for c in range(N_CHR)]
    batch, bd, bd_off = _translocation_batch(chroms, read_len, 2400, seed=70 + read_len)
    cnt = np.diff(bd_off.astype(np.int64))
    high = np.repeat(np.arange(batch.n), cnt)[bd["chr_id"] >= 24]
    assert len(bd) > 0 and (bd["chr_id"] >= 24).sum() * 3 >= len(bd) and len(set(high.tolist())) > 500
    orc = run_oracle({}, chroms, batch, bd=bd, bd_off=bd_off)
    far_chr = np.array([int(orc["far_pts"][i][0]["chr_id"]) if orc["far_cnt"][i] else -1 for i in range(batch.n)])
    elsewhere = (far_chr >= 0) & (far_chr != batch.chr_id)
    print(f"read length {read_len}: far end on another chromosome {int(elsewhere.sum())}, of them on 24-29 {int((elsewhere & (far_chr >= 24)).sum())}")
    assert int(elsewhere.sum()) >= 500 and int((elsewhere & (far_chr >= 24)).sum()) >= 100
    eng = engine_factory()
    eng.load_reference(chroms)
    close = eng.close_end_batch(batch)
    compare_result(close, orc, batch.n, check_far=False)
    both = eng.far_end_batch(batch, close, bd=bd, bd_off=bd_off)
    compare_result(both, orc, batch.n)
    db = eng.upload(batch)
    eng.set_windows(db, bd, bd_off)
    eng.search_device(db)
    compare_result(eng.download(db), orc, batch.n)
    eng.free_device_batch(db)
