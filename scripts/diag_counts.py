"""Diagnostics: per-read event counts of a -DPG_DIAG build (LDS fills, seed-filter runs, candidate passes, evaluations)
on the bench workload:  python scripts/diag_counts.py <lib.so> [reads] (PG_X=<n> selects -x n, PG_LEN the read length;
PG_DIAG_LAYOUT=2 for a -DPG_DIAG=2 build: the census of the evaluations; PG_DIAG_LAYOUT=3 for a -DPG_DIAG=3 build: the census of the
fold's loops; PG_DIAG_LAYOUT=4 for a -DPG_DIAG=4 build: block bodies by kind and merged evaluations by qmask)"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pindel_amd import binding, synth

binding.use_library(os.path.abspath(sys.argv[1]))
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
dev = torch.device("cuda", 0)
ref = synth.make_reference(62_435_964, seed=20260927, device=dev)
kw, rkw = {}, {}
if os.environ.get("PG_X"):
    kw["max_range_index"] = int(os.environ["PG_X"])
if os.environ.get("PG_LEN"):
    rkw["read_len"] = int(os.environ["PG_LEN"])
batch = synth.make_reads(ref, n, seed=20260928, device=dev, **rkw)
eng = binding.Engine(**kw)
eng.load_reference([("20", ref)])
db = eng.upload(batch)
eng.search_device(db)
L = binding.lib()
L.pg_debug_read_reserved.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
out = np.zeros(n, dtype=np.uint32)
assert L.pg_debug_read_reserved(eng._h, db, out.ctypes.data, n) == 0
if os.environ.get("PG_DIAG_LAYOUT") == "2":
    # a -DPG_DIAG=2 build: the census of the evaluations, a nibble per count (Search::dg, pg_kernels.hip)
    names = ["close-end evaluations", "far-end evaluations", "evaluations, no point", "rounds run", "rounds without a point",
             "emit_runs calls", "quarter merges via LDS"]
    for k, nm in enumerate(names):
        f = (out >> (4 * k)) & 0xf
        hist = np.bincount(f, minlength=16)
        print(f"{nm:24s} mean {f.mean():6.3f}  histogram 0..15: {(hist[:16] / n).round(3).tolist()}")
    ev = ((out & 0xf) + ((out >> 4) & 0xf)).astype(np.int64)
    print(f"{'evaluations':24s} mean {ev.mean():6.3f}; rounds per evaluation {((out >> 12) & 0xf).sum() / max(int(ev.sum()), 1):.3f}")
elif os.environ.get("PG_DIAG_LAYOUT") == "3":
    # a -DPG_DIAG=3 build: the census of the fold's loops (Search::dg, pg_kernels.hip); "full" = the share of reads whose field is at
    # its highest value, a bound on the overflows into the next field
    fields = [("tier A full iterations, no rings", 0, 6), ("tier A tail iterations, no rings", 6, 4), ("tier A iterations, rings", 10, 6),
              ("tier B candidate-rounds, round 0", 16, 6), ("tier B candidate-rounds, rounds >= 1", 22, 5), ("AccB stores", 27, 4)]
    for nm, sh, w in fields:
        f = (out >> sh) & ((1 << w) - 1)
        hist = np.bincount(f, minlength=10)
        print(f"{nm:38s} mean {f.mean():7.3f}  full {(f == (1 << w) - 1).mean():.5f}  histogram 0..9: {(hist[:10] / n).round(3).tolist()}")
elif os.environ.get("PG_DIAG_LAYOUT") == "4":
    # a -DPG_DIAG=4 build: the census of the block bodies by kind and of the merged evaluations by qmask (Search::dg, pg_kernels.hip)
    fields = [("close-end block bodies, kind B", 0, 6), ("close-end block bodies, kind F", 6, 6), ("mixed-pass block bodies", 12, 6),
              ("evaluations merging two quarters", 18, 5), ("evaluations merging four quarters", 23, 5)]
    for nm, sh, w in fields:
        f = (out >> sh) & ((1 << w) - 1)
        hist = np.bincount(f, minlength=10)
        print(f"{nm:38s} mean {f.mean():7.3f}  full {(f == (1 << w) - 1).mean():.5f}  histogram 0..9: {(hist[:10] / n).round(3).tolist()}")
else:
    names = ["LDS fills", "seed-filter runs", "candidate passes", "evaluations"]
    for k, nm in enumerate(names):
        f = (out >> (8 * k)) & 0xff
        hist = np.bincount(f, minlength=8)
        print(f"{nm:18s} mean {f.mean():6.3f}  histogram 0..9: {(hist[:10] / n).round(3).tolist()}")
print("kernel ms", round(eng.last_stats()[0], 2))
