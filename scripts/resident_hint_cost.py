"""What the resident hinted search costs beside the host-result entry, on the same reads and the same table (the set-up of
scripts/hint_lookup_cost.py: the COLO-829 chr20 BreakDancer table over its densest 5-Mbp window, a synthetic chr20, reads at close
ends half next to events and half anywhere):

  host      pg_search_batch_table: upload, close launch, close runs to the host, lookup, far launch, far runs to the host
  resident  pg_device_batch_upload + pg_device_batch_search_table + pg_device_batch_download: both run lists stay in the pool
            until one download

The two alternate, REPEATS times after one warm-up each; medians are reported and the results must be identical.  search_ms is
what pg_last_search_stats reports: the far launch alone for `host`, close + far for `resident`.  Prints one JSON line.

    python scripts/resident_hint_cost.py [--reads 1000000] [--repeats 3]
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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--read-len", type=int, default=100)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("resident_hint_cost.py measures on the GPU: none is visible")
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
    rng = np.random.default_rng(5)
    n, L = a.reads, a.read_len
    cnt_run = np.diff(cluster_off.astype(np.int64))[run_cluster]
    hot = run_first[:-1][cnt_run > 0].astype(np.int64)
    last = np.where(rng.random(n) < 0.5, hot[rng.integers(0, len(hot), n)] + rng.integers(-150, 150, n), rng.integers(lo, hi, n))
    last = np.sort(last).astype(np.uint32)
    refa = np.frombuffer(ref, dtype=np.uint8)
    seq = refa[(last.astype(np.int64)[:, None] + np.arange(L)[None, :]).ravel()]
    batch = ReadBatch(seq=seq, seq_off=(np.arange(n + 1) * L).astype(np.uint64), anchor_strand=np.full(n, ord("-"), np.uint8),
                      anchor_pos=(last.astype(np.int64) - SPACER + 300).astype(np.int32), insert_size=np.full(n, 500, np.int16),
                      chr_id=np.zeros(n, np.int32))
    eng = binding.Engine(device=0)
    eng.load_reference([("20", ref)])

    def stats(wall):
        scan_ms, fill_ms, _, n_win = eng.last_hint_stats()
        return dict(wall_ms=wall * 1e3, search_ms=eng.last_stats()[0], lookup_ms=scan_ms + fill_ms, windows=n_win)

    def host():
        t0 = time.perf_counter()
        r = eng.search_batch(batch, hints=table)
        return r, stats(time.perf_counter() - t0)

    def resident():
        t0 = time.perf_counter()
        db = eng.upload(batch)
        eng.search_table_device(db, table)
        s = stats(0.0)
        r = eng.download(db)
        eng.free_device_batch(db)
        s["wall_ms"] = (time.perf_counter() - t0) * 1e3
        return r, s

    ra, _ = host()
    rb, _ = resident()
    for f in ("close_off", "far_off", "rc_flag"):
        assert np.array_equal(getattr(ra, f), getattr(rb, f)), f
    assert ra.close_runs.tobytes() == rb.close_runs.tobytes() and ra.far_runs.tobytes() == rb.far_runs.tobytes(), "the two differ"
    del ra, rb
    runs = {"host": [], "resident": []}
    for _ in range(a.repeats):
        runs["host"].append(host()[1])
        runs["resident"].append(resident()[1])

    def med(rows):
        out = {k: round(float(np.median([r[k] for r in rows])), 3) for k in rows[0]}
        out["wall_ms_each"] = [round(r["wall_ms"], 2) for r in rows]
        return out
    print(json.dumps({"reads": n, "read_len": L, "table_runs": len(run_cluster), "repeats": a.repeats, "host": med(runs["host"]),
                      "resident": med(runs["resident"]),
                      "note": "search_ms: the far launch alone for host, close + far launches for resident"}))
    eng.close()


if __name__ == "__main__":
    main()
