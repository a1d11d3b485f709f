"""-q's containment test: the kernel (pg_dd_contains_batch, HIP-event time) against the host C++ restatement (one thread) on the
same items -- consensus-like queries of 30-100 bases against windows of 2 x MIN_DD_MAP_DISTANCE (16 000 bases) on a synthetic
reference, half of them planted (true), half random (almost always false: the whole DP).  Prints one JSON line.

    python scripts/dd_rate.py [--items 4096] [--cpu-items 64]
"""
import argparse
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import pyoracle  # noqa: E402
from pindel_amd import binding, synth  # noqa: E402
from tests import dd_restated as R  # noqa: E402

SPACER = 100000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=4096)
    ap.add_argument("--cpu-items", type=int, default=64)
    ap.add_argument("--window", type=int, default=16000)
    a = ap.parse_args()
    ref = [("chrS", synth.make_reference(4_000_000, seed=31))]
    s = bytes(ref[0][1])
    rng = random.Random(3)
    q, cid, ws, wl = [], [], [], []
    for k in range(a.items):
        st = rng.randint(SPACER, len(s) - SPACER - a.window)
        w = s[st:st + a.window].decode()
        L = rng.randint(30, 100)
        if k % 2:
            p = rng.randint(0, a.window - L)
            q.append("".join(rng.choice("ACGT") if rng.random() < 0.03 else c for c in w[p:p + L]))
        else:
            q.append("".join(rng.choice("ACGT") for _ in range(L)))
        cid.append(0)
        ws.append(st)
        wl.append(a.window)
    eng = binding.Engine(device=0)
    eng.load_reference(ref)
    eng.dd_contains(q[:8], cid[:8], ws[:8], wl[:8])                     # warm-up
    runs = [eng.dd_contains(q, cid, ws, wl) for _ in range(3)]
    got = runs[-1][0]
    ms = sorted(r[1] for r in runs)[1]
    cells = sum(2 * len(x) * n for x, n in zip(q, wl))                    # both strands, whole DP (an upper bound)
    n_cpu = min(a.cpu_items, a.items)
    mm = pyoracle.max_mismatch_table()
    t0 = time.perf_counter()
    want = R.cpu_contains(q[:n_cpu], [s[x:x + n] for x, n in zip(ws[:n_cpu], wl[:n_cpu])], mm, threads=1)
    cpu_s = time.perf_counter() - t0
    assert (want == got[:n_cpu]).all(), "kernel and host restatement differ"
    print(json.dumps({
        "items": a.items, "window": a.window, "true": int(got.sum()),
        "kernel_ms": round(ms, 3), "kernel_items_per_s": round(a.items / (ms * 1e-3)),
        "kernel_dp_cells_per_s_upper_bound": round(cells / (ms * 1e-3)),
        "cpu_items": n_cpu, "cpu_one_thread_s": round(cpu_s, 3), "cpu_items_per_s": round(n_cpu / cpu_s, 1),
        "speedup_vs_one_cpu_thread": round((a.items / (ms * 1e-3)) / (n_cpu / cpu_s), 1),
        "note": "cells/s counts every cell of both strands; early exits make the real count smaller for true items"}))
    eng.close()


if __name__ == "__main__":
    main()
