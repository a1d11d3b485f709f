"""-q (dispersed duplications) on the MI355X: the containment kernel (pg_dd_contains_batch) bit-exact with the host restatement,
and `pindel_pg -f reference.fa -i config -o X -q` (demo/simulated_MEI/runme line 1) equal to the same host pipeline fed by
oracle close ends and the host containment test."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import pyoracle
from tests import dd_restated as R
from tests import golden_util as gu
from tests.test_dd_cpu import IUPAC, _mutate, _rand
from tests.test_mei_bam import _unpack

pytestmark = pytest.mark.gpu
MM = [int(x) for x in pyoracle.max_mismatch_table()[:500]]
SPACER = 100000


def _items(chroms, n, seed):
    """Windows into the padded chromosomes (some starting in the spacer, up to 2 x 8000 bases and a few far longer) and
    queries of 15-499 bases: planted (both strands, mutated), random, with N runs and IUPAC letters."""
    rng = random.Random(seed)
    q, cid, ws, wl = [], [], [], []
    for k in range(n):
        c = rng.randrange(len(chroms))
        s = chroms[c][1]
        kind = k % 10
        d = rng.choice([1, 15, 64, 200, 700, 2000]) if kind < 8 else rng.choice([16000, 16001])
        if k % 997 == 0:
            d = 200000
        d = min(d, len(s) - 2 * SPACER)
        start = rng.randint(SPACER - 300, len(s) - SPACER - d) if kind != 7 else rng.randint(0, SPACER - 5)
        d = min(d, len(s) - start)
        w = s[start:start + d].decode()
        L = rng.choice([15, 20, 40, 63, 64, 65, 100, 128, 129, 250, 499]) if kind in (0, 5) else rng.randint(15, 120)
        if kind in (1, 2) and d > 20:
            a = rng.randint(0, max(0, d - 15))
            x = _mutate(rng, w[a:a + L], 0.05 * (kind - 1))
        elif kind == 3 and d > 20:
            a = rng.randint(0, max(0, d - 15))
            x = R.revcomp(_mutate(rng, w[a:a + L], 0.03))
        elif kind == 4:
            x = "N" * rng.randint(1, 30) + _rand(rng, rng.randint(0, 30))
        elif kind == 6:
            x = _mutate(rng, w[:L] if d >= 15 else _rand(rng, L), 0.1, "ACGT" + IUPAC)
        else:
            x = _rand(rng, L)
        x = x[:499] if len(x) >= 15 else x + _rand(rng, 15 - len(x))
        q.append(x)
        cid.append(c)
        ws.append(start)
        wl.append(d)
    return q, cid, ws, wl


def test_containment_kernel_equals_the_host_restatement(tmp_path):
    from pindel_amd import binding, synth
    ref = [("chrA", synth.make_reference(120_000, seed=21)), ("chrB", synth.make_reference(260_000, seed=22))]
    eng = binding.Engine(device=0)
    eng.load_reference(ref)
    chroms = [(n, bytes(s)) for n, s in ref]
    q, cid, ws, wl = _items(chroms, 10_000, seed=5)
    got, ms = eng.dd_contains(q, cid, ws, wl)
    want = R.cpu_contains(q, [chroms[c][1][s:s + n] for c, s, n in zip(cid, ws, wl)], MM)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(q[i], cid[i], ws[i], wl[i], int(got[i]), int(want[i])) for i in bad[:5]]
    assert 0 < want.sum() < len(want)
    # the device path agrees with the Python restatement on a sample (the C++ restatement is checked against it on the CPU)
    for i in range(0, 10_000, 97):
        if wl[i] <= 2000:
            assert bool(got[i]) == R.contains_any_strand(q[i], chroms[cid[i]][1][ws[i]:ws[i] + wl[i]].decode(), MM)
    cells = sum(2 * len(x) * n for x, n in zip(q, wl))
    print(f"{len(q)} items, {int(want.sum())} true, kernel {ms:.2f} ms, {cells / (ms * 1e-3) / 1e9:.1f} G DP cells/s (upper bound)")
    eng.close()


def _run(d, prefix, *extra):
    from pindel_amd import binding
    exe = os.path.join(os.path.dirname(binding.LIB_PATH), "pindel_pg")
    out = subprocess.run([exe, "-f", os.path.join(d, "reference.fa"), "-i", os.path.join(d, "config"), "-o", os.path.join(d, prefix)]
                         + list(extra), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return out.stdout


def test_runme_line_1_equals_the_host_pipeline_with_oracle_close_ends(tmp_path):
    from pindel_amd import hostio
    d = _unpack(tmp_path)
    seqs = [s for _, s in hostio.load_fasta(os.path.join(d, "reference.fa"))]
    log = _run(d, "gpu", "-q")
    assert "dispersed duplications:" in log, log[-800:]
    _run(d, "plain")
    for suf in list(gu.SUFFIXES) + ["LI", "BP", "RP", "CloseEndMapped"]:
        a, b = os.path.join(d, "gpu_" + suf), os.path.join(d, "plain_" + suf)
        if os.path.exists(b):
            assert open(a, "rb").read() == open(b, "rb").read(), f"-q changed _{suf}"
    cb = R.oracle_close_cb(seqs)
    stats, bps, _ = R.dd_run(os.path.join(d, "reference.fa"), os.path.join(d, "config"), os.path.join(d, "want"), MM, close_cb=cb)
    got = open(os.path.join(d, "gpu_DD"), "rb").read()
    assert got == open(os.path.join(d, "want_DD"), "rb").read()
    print("demo -q:", stats, bps)
    print(got.decode()[:1500])
    lines = got.decode().splitlines()
    events = [x.split("\t") for x in lines if x[:1].isdigit()]
    assert len(events) == 1 and events[0][1:3] == ["DD", "chr2"]
    for extra, name in ((["-G", "0,0"], "g2"), (["-T", "1"], "t1"), (["-T", "8"], "t8")):
        _run(d, name, "-q", *extra)
        assert open(os.path.join(d, name + "_DD"), "rb").read() == got, extra
    _run(d, "dup", "-q", "--DD_REPORT_DUPLICATION_READS")
    R.dd_run(os.path.join(d, "reference.fa"), os.path.join(d, "config"), os.path.join(d, "wantdup"), MM,
             opts=R.DD_DEFAULTS[:5] + (1,), close_cb=cb)
    assert open(os.path.join(d, "dup_DD"), "rb").read() == open(os.path.join(d, "wantdup_DD"), "rb").read()
    # without -q there is no _DD; -q false still runs it (the reference tests isSet())
    assert not os.path.exists(os.path.join(d, "plain_DD"))
    _run(d, "qfalse", "-q", "false")
    assert open(os.path.join(d, "qfalse_DD"), "rb").read() == got


def test_q_with_pindel_text_input_writes_an_empty_dd_and_a_note(tmp_path):
    from pindel_amd import binding
    d = _unpack(tmp_path)
    exe = os.path.join(os.path.dirname(binding.LIB_PATH), "pindel_pg")
    out = subprocess.run([exe, "-f", os.path.join(d, "reference.fa"), "-p", os.path.join(d, "input"), "-o", os.path.join(d, "t"), "-q"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert os.path.getsize(os.path.join(d, "t_DD")) == 0
    assert "_DD is empty" in out.stdout


def test_planted_dd_bam_keeps_and_drops_breakpoints_like_the_host_pipeline(tmp_path):
    """The synthetic BAM of tests/dd_synth.py (one event whose consensus has no local copy, one whose ends were copied next to it):
    `pindel_pg -q --MIN_DD_MAP_DISTANCE 400` on the MI355X == the host pipeline fed by oracle close ends; both outcomes of the
    containment test occur."""
    from pindel_amd import binding, hostio
    from tests import dd_synth
    d = str(tmp_path)
    syn = dd_synth.make(d)
    exe = os.path.join(os.path.dirname(binding.LIB_PATH), "pindel_pg")
    out = subprocess.run([exe, "-f", syn["fasta"], "-i", syn["config"], "-o", os.path.join(d, "gpu"), "-q", "--MIN_DD_MAP_DISTANCE", "400"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    line = [x for x in out.stdout.splitlines() if "dispersed duplications:" in x][0]
    print(line)
    seqs = [s for _, s in hostio.load_fasta(syn["fasta"])]
    stats, _, _ = R.dd_run(syn["fasta"], syn["config"], os.path.join(d, "want"), MM, opts=(350, 100, 3, 3, 400, 0),
                           close_cb=R.oracle_close_cb(seqs))
    assert stats[4] > 0 and stats[3] - stats[4] > 0
    assert f"{stats[3]} consensus tests" in line and f"{stats[4]} kept" in line
    got = open(os.path.join(d, "gpu_DD"), "rb").read()
    assert got == open(os.path.join(d, "want_DD"), "rb").read()
    assert got.count(b"\tDD\tchrB\t") == 2 and b"# Reference: " in got and b"?\t?\t?\t@p" in got
