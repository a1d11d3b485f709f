"""Diagnostics: the fixed-length kernels against the kernels they replace in ONE process, on the same reads, with the shipped
library: PG_NO_FIXED_LEN toggled between the rounds (pg_debug_reload_env).
   python scripts/ab_fixed.py [reads] [read length ...]        (default 2 000 000 reads; 100 and 150 bases)
Per length and round: the kernel the step ran (fixed length, 0 = the default-parameter kernel), the best of three steps in ms (the
step of bench.py: pg_device_batch_pack_search) and a digest of the downloaded result (equal digests = bit-identical results)."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pindel_amd import binding, synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
lens = [int(x) for x in sys.argv[2:]] or [100, 150]
dev = torch.device("cuda", 0)
ref = synth.make_reference(62_435_964, seed=20260927, device=dev)
eng = binding.Engine()
eng.load_reference([("20", ref)])
for L in lens:
    batch = synth.make_reads(ref, n, seed=20260928, device=dev, read_len=L)
    db = eng.upload(batch)
    for rnd in range(4):                       # fixed, generic, fixed, generic
        if rnd % 2:
            os.environ["PG_NO_FIXED_LEN"] = "1"
        else:
            os.environ.pop("PG_NO_FIXED_LEN", None)
        binding.reload_env()
        ms = []
        for _ in range(3):
            eng.pack_search_device(db)
            ms.append(eng.last_stats()[0])
        res = eng.download(db)
        h = hashlib.sha256()
        for a in (res.close_off, res.far_off, res.rc_flag, res.close_runs, res.far_runs):
            h.update(a.tobytes())
        print(f"{n} x {L} bp  fixed_len {eng.last_fixed_len():3d}  step ms {min(ms):8.3f}  (all: {' '.join(f'{x:.3f}' for x in ms)})  "
              f"digest {h.hexdigest()[:16]}", flush=True)
    eng.free_device_batch(db)
os.environ.pop("PG_NO_FIXED_LEN", None)
eng.close()
