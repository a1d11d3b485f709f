"""What resolving window hints costs at seam 2 (pg_far_end_batch_from_close), both ways, on the same reads:

  table     pg_far_end_batch_from_close_table: the window's hint table uploaded once, the per-read clusters built on the device
            by the count / scan / fill kernels of pg_hints.hip (their HIP-event time is reported);
  per read  the lookup on the host (numpy restatement of the rule; the command line's C++ loop does the same work) and the upload
            of the replicated per-read clusters -- the baseline, same build, same process.

The table is the reference's real COLO-829 chr20 BreakDancer file (tests/golden/demo) over its densest 5-Mbp search window; the
reference sequence is synthetic at chr20's size.  Half of the reads have their close end within 150 bases of an event (the reads
a caller looks for), the rest anywhere in the window.  The two ways alternate, REPEATS times after one warm-up each; medians are
reported, and the results of the two must be identical.  Prints one JSON line.

    python scripts/hint_lookup_cost.py [--reads 1000000] [--repeats 5] [--lib pindel_amd/libpindel_pg_parent.so]
"""
import argparse
import gzip
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pindel_amd import binding, hostlib, synth  # noqa: E402
from pindel_amd.hostio import ReadBatch  # noqa: E402
from tests.test_hint_table_cpu import bd_table  # noqa: E402

SPACER = 100000
DEMO = os.path.join(ROOT, "tests", "golden", "demo")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--lib", help="measure this build of the library (binding.use_library)")
    a = ap.parse_args()
    if a.lib:
        binding.use_library(os.path.abspath(a.lib))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("hint_lookup_cost.py measures on the GPU: none is visible")
    size = int(open(os.path.join(DEMO, "hs_ref_chr20.fa.fai")).read().split()[1])
    ref = synth.make_reference(size, seed=20260927, device=torch.device("cuda", 0))
    lo, hi = 25_000_000 + SPACER, 30_000_000 + SPACER
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "bd.sv")
        with gzip.open(os.path.join(DEMO, "COLO-829.20.BreakDancer.sv.gz"), "rb") as s, open(path, "wb") as o:
            shutil.copyfileobj(s, o)
        run_first, run_cluster, cluster_off, win, n_ev = bd_table(hostlib.lib(), path, ["20"], 0, lo, hi)
    w = np.zeros(len(win), dtype=binding.WINDOW_DTYPE)
    w["chr_id"], w["start"], w["end"] = win[:, 0], win[:, 1], win[:, 2]
    table = binding.HintTable(run_first, run_cluster, cluster_off, w)
    # close ends: half next to the starts of runs that have windows, half anywhere in the window
    rng = np.random.default_rng(5)
    n, L = a.reads, a.read_len
    cnt_run = np.diff(cluster_off.astype(np.int64))[run_cluster]
    hot = run_first[:-1][cnt_run > 0].astype(np.int64)
    last = np.where(rng.random(n) < 0.5, hot[rng.integers(0, len(hot), n)] + rng.integers(-150, 150, n), rng.integers(lo, hi, n))
    last = np.sort(last).astype(np.uint32)
    mx = np.full(n, 30, dtype=np.int16)
    # the reads: the reference at their close end (what the far end then finds is beside the point: both ways search the same)
    refa = np.frombuffer(ref, dtype=np.uint8)
    seq = refa[(last.astype(np.int64)[:, None] + np.arange(L)[None, :]).ravel()]
    batch = ReadBatch(seq=seq, seq_off=(np.arange(n + 1) * L).astype(np.uint64), anchor_strand=np.full(n, ord("-"), np.uint8),
                      anchor_pos=(last.astype(np.int64) - SPACER + 300).astype(np.int32), insert_size=np.full(n, 500, np.int16),
                      chr_id=np.zeros(n, np.int32))
    eng = binding.Engine(device=0)
    eng.load_reference([("20", ref)])

    def by_table():
        t0 = time.perf_counter()
        r = eng.far_end_batch_from_close(batch, last, mx, hints=table)
        wall = time.perf_counter() - t0
        scan_ms, fill_ms, table_bytes, n_win = eng.last_hint_stats()
        return r, dict(wall_ms=wall * 1e3, search_ms=eng.last_stats()[0], scan_ms=scan_ms, fill_ms=fill_ms, upload_bytes=table_bytes,
                       windows=n_win)

    def per_read():
        t0 = time.perf_counter()
        bd, bd_off = table.expand(last, mx)
        t1 = time.perf_counter()
        r = eng.far_end_batch_from_close(batch, last, mx, bd=bd, bd_off=bd_off)
        wall = time.perf_counter() - t0
        return r, dict(wall_ms=wall * 1e3, host_lookup_ms=(t1 - t0) * 1e3, search_ms=eng.last_stats()[0],
                       upload_bytes=int(bd_off.nbytes + bd.nbytes), windows=int(bd_off[-1]))

    ra, _ = by_table()                                       # warm-up, and the results of the two ways
    rb, _ = per_read()
    assert np.array_equal(ra.far_off, rb.far_off) and ra.far_runs.tobytes() == rb.far_runs.tobytes(), "the two ways differ"
    del ra, rb
    runs = {"table": [], "per_read": []}
    for _ in range(a.repeats):
        runs["table"].append(by_table()[1])
        runs["per_read"].append(per_read()[1])

    def med(rows):
        out = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
        out["wall_ms_min_max"] = [round(min(r["wall_ms"] for r in rows), 2), round(max(r["wall_ms"] for r in rows), 2)]
        return {k: (round(v, 3) if isinstance(v, float) else v) for k, v in out.items()}
    t, p = med(runs["table"]), med(runs["per_read"])
    print(json.dumps({"reads": n, "read_len": L, "bd_events": int(n_ev), "table_runs": len(run_cluster),
                      "table_clusters": len(cluster_off) - 1, "table_windows": len(w), "repeats": a.repeats,
                      "table": t, "per_read": p,
                      "hint_kernels_ms": round(t["scan_ms"] + t["fill_ms"], 3),
                      "wall_ms_saved": round(p["wall_ms"] - t["wall_ms"], 2),
                      "note": "per_read.host_lookup_ms is numpy's vectorised lookup, part of per_read.wall_ms; wall times hold the "
                              "same far-end search (search_ms) either way"}))
    eng.close()


if __name__ == "__main__":
    main()
