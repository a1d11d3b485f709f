"""Position-keyed hint tables, host side (no GPU): BDHints::table() through pgh_bd_table against the dense per-position
lookup (pgh_bd_query) on the reference's real COLO-829 BreakDancer file, and the ctypes layout of pg_hint_table."""
import ctypes as C
import gzip
import os
import shutil
import subprocess

import numpy as np

from pindel_amd import binding, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "tests", "golden", "demo")
SPACER = 100000


def _gunzip(name, tmp_path):
    dst = os.path.join(str(tmp_path), name)
    with gzip.open(os.path.join(DEMO, name + ".gz"), "rb") as s, open(dst, "wb") as d:
        shutil.copyfileobj(s, d)
    return dst


def bd_table(L, path, names, chr_id, start, end):
    """pgh_bd_table: (run_first, run_cluster, cluster_off, windows[n, 3], n_events); asks for the sizes first."""
    L.pgh_bd_table.argtypes = [C.c_char_p, C.c_uint32, C.c_int32, C.POINTER(C.c_char_p), C.c_int32, C.c_uint32, C.c_uint32,
                               C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                               C.c_void_p]
    arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
    counts = np.zeros(3, dtype=np.uint64)
    nev = C.c_uint64()
    rc = L.pgh_bd_table(path.encode(), SPACER, len(names), arr, chr_id, start, end, None, None, 0, None, 0, None, 0,
                        counts.ctypes.data, C.byref(nev))
    assert rc in (0, -3), rc
    nr, nc, nw = (int(x) for x in counts)
    run_first = np.zeros(nr + 1, dtype=np.uint32)
    run_cluster = np.zeros(max(nr, 1), dtype=np.uint32)
    cluster_off = np.zeros(nc + 1, dtype=np.uint64)
    win = np.zeros((max(nw, 1), 3), dtype=np.int32)
    rc = L.pgh_bd_table(path.encode(), SPACER, len(names), arr, chr_id, start, end, run_first.ctypes.data, run_cluster.ctypes.data,
                        nr, cluster_off.ctypes.data, nc, win.ctypes.data, nw, counts.ctypes.data, C.byref(nev))
    assert rc == 0, rc
    return run_first, run_cluster[:nr], cluster_off, win[:nw], nev.value


def lookup(run_first, run_cluster, cluster_off, p):
    """The lookup rule of pg_hint_table restated: per position (first window, count) of its cluster; count 0 outside the runs."""
    p = np.asarray(p, dtype=np.int64)
    n_runs = len(run_cluster)
    if not n_runs:
        return np.zeros(len(p), np.int64), np.zeros(len(p), np.int64)
    rf = run_first.astype(np.int64)
    k = np.searchsorted(rf, p, side="right") - 1
    inside = (p >= rf[0]) & (p < rf[n_runs])
    c = run_cluster[np.clip(k, 0, n_runs - 1)].astype(np.int64)
    off = cluster_off.astype(np.int64)
    return off[c], np.where(inside, off[c + 1] - off[c], 0)


def test_table_equals_the_dense_lookup(tmp_path):
    L = hostlib.lib()
    L.pgh_bd_query.argtypes = [C.c_char_p, C.c_uint32, C.c_int32, C.POINTER(C.c_char_p), C.c_int32, C.c_uint32,
                               C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    path = _gunzip("COLO-829.20.BreakDancer.sv", tmp_path)
    # the densest megabase of the file: 198 event ends
    start, end = SPACER + 25_500_000, SPACER + 26_500_000
    win_start, win_end = start - 3000, end + 3000            # loadRegion's margins (3 x 1000)
    run_first, run_cluster, cluster_off, win, n_ev = bd_table(L, path, ["20"], 0, start, end)
    assert n_ev == 310
    assert len(run_first) == len(run_cluster) + 1 and (np.diff(run_first.astype(np.int64)) > 0).all()
    assert (run_cluster[1:] != run_cluster[:-1]).all()       # equal neighbours are merged
    assert int(run_first[0]) == win_start + 1 and int(run_first[-1]) == win_end
    assert (run_cluster < len(cluster_off) - 1).all() and int(cluster_off[-1]) == len(win)
    # the dense answer, position by position
    q = np.arange(win_start - 2, win_end + 3, dtype=np.uint32)
    off = np.zeros(len(q) + 1, dtype=np.uint64)
    cap = 8_000_000
    dense = np.zeros(3 * cap, dtype=np.int32)
    nev = C.c_uint64()
    arr = (C.c_char_p * 1)(b"20")
    rc = L.pgh_bd_query(path.encode(), SPACER, 1, arr, 0, start, end, len(q), q.ctypes.data, off.ctypes.data, dense.ctypes.data,
                        cap, C.byref(nev))
    assert rc == 0, rc
    off = off.astype(np.int64)
    dense = dense[:3 * int(off[-1])].reshape(-1, 3)
    first, count = lookup(run_first, run_cluster, cluster_off, q)
    np.testing.assert_array_equal(count, np.diff(off))
    idx = np.repeat(first - off[:-1], count) + np.arange(int(off[-1]), dtype=np.int64)
    np.testing.assert_array_equal(win[idx], dense)
    # not an empty table: many distinct clusters are hit, and the edges answer "none"
    _, cnt_run = lookup(run_first, run_cluster, cluster_off, run_first[:-1])
    used = np.unique(run_cluster[cnt_run > 0])
    assert len(used) >= 10, len(used)
    assert count[:3].tolist() == [0, 0, 0] and count[-3:].tolist() == [0, 0, 0]


def test_table_of_a_region_without_events(tmp_path):
    L = hostlib.lib()
    bd = tmp_path / "bd.txt"
    bd.write_text("chrA\t5000\t10+0-\tchrA\t9000\t0+10-\tDEL\t4000\t99\t10\n")
    run_first, run_cluster, cluster_off, win, n_ev = bd_table(L, str(bd), ["chrA", "chrB"], 1, SPACER + 50_000, SPACER + 60_000)
    assert n_ev == 1
    # one run over the whole window, naming the empty cluster
    assert len(run_cluster) == 1 and int(cluster_off[run_cluster[0] + 1]) == int(cluster_off[run_cluster[0]])
    _, count = lookup(run_first, run_cluster, cluster_off, np.arange(SPACER + 40_000, SPACER + 70_000))
    assert not count.any()


def test_hint_table_ctypes_layout(tmp_path):
    """sizeof / field offsets of binding.PgHintTable == the C struct's, from a compiled probe."""
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pindel_pg.h"\n'
                     'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(pg_hint_table), offsetof(pg_hint_table, n_runs),\n'
                     '  offsetof(pg_hint_table, run_first), offsetof(pg_hint_table, run_cluster), offsetof(pg_hint_table, n_clusters),\n'
                     '  offsetof(pg_hint_table, cluster_off), offsetof(pg_hint_table, windows)); return 0; }\n')
    exe = tmp_path / "probe"
    r = subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    T = binding.PgHintTable
    assert got == [C.sizeof(T)] + [getattr(T, f).offset for f, _ in T._fields_]


def test_hint_table_expand_and_argument_check():
    """HintTable.expand is the rule (used by the GPU tests as the per-read expansion); bd and hints together are refused
    before anything touches the library."""
    w = np.zeros(5, dtype=binding.WINDOW_DTYPE)
    w["start"] = np.arange(5)
    t = binding.HintTable([10, 20, 30], [1, 0], [0, 2, 5], w)
    bd, off = t.expand([9, 10, 19, 20, 29, 30, 15], [5, 5, 5, 5, 5, 5, 0])
    assert off.tolist() == [0, 0, 3, 6, 8, 10, 10, 10] and bd["start"].tolist() == [2, 3, 4, 2, 3, 4, 0, 1, 0, 1]
    s = t.struct()
    assert s.n_runs == 2 and s.n_clusters == 2
    import pytest
    eng = object.__new__(binding.Engine)                     # no context: the check comes first
    eng._h = None
    with pytest.raises(ValueError):
        binding.Engine.far_end_batch_from_close(eng, None, [], [], bd=bd, bd_off=off, hints=t)
    with pytest.raises(ValueError):
        binding.Engine.far_end_batch(eng, None, None, bd=bd, bd_off=off, hints=t)
