#!/usr/bin/env python3
"""What the device-buffer entries cost next to their host siblings, on the default benchmark shapes (bench.py's sv10m: the
chr20-shaped reference, 10 M x 100 bp reads from synth):

    pg_load_reference        against  pg_load_reference_device         (Engine.load_reference / load_reference_tensors)
    pg_device_batch_upload   against  pg_device_batch_upload_device    (Engine.upload / upload_tensors)
    pg_device_batch_download against  pg_device_batch_download_device  (Engine.download / download_tensors)

Each sibling starts from data where it expects it -- host arrays for the host entry, tensors on the GPU for the device
entry -- and every call is synchronous, so a host clock around the call is the call's time.  One warm-up pair, then three
alternating repetitions per pair.  Prints a markdown table; there is no speed bar, a slower device path is called out.

    python scripts/device_io_cost.py [--reads N] [--chr-len L] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pindel_amd import binding, synth  # noqa: E402

CHR20_LEN = 62_435_964
REPS = 3


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def alternate(host_fn, dev_fn, after=lambda out: None):
    """One warm-up of each, then REPS alternating repetitions; returns the two lists of ms."""
    h, d = [], []
    for rep in range(REPS + 1):
        for times, fn in ((h, host_fn), (d, dev_fn)):
            ms, out = timed(fn)
            after(out)
            if rep:
                times.append(ms)
    return h, d


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--chr-len", type=int, default=CHR20_LEN)
    ap.add_argument("--seed", type=int, default=20260927)
    ap.add_argument("--out", help="also write the table to this file")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("device_io_cost.py needs the GPU: there is nothing to time without one")
    dev = "cuda:0"
    ref = synth.make_reference(args.chr_len, seed=args.seed, device=dev)
    batch = synth.make_reads(ref, args.reads, read_len=args.read_len, seed=args.seed + 1, device=dev)
    ref_t = torch.frombuffer(bytearray(ref), dtype=torch.uint8).to(dev)
    reads_t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (
        batch.seq, batch.seq_off.astype(np.uint64).view(np.int64), batch.anchor_strand, batch.anchor_pos, batch.insert_size,
        batch.chr_id)]
    torch.cuda.synchronize()
    eng = binding.Engine(device=0)
    rows = []

    h, d = alternate(lambda: eng.load_reference([("20", ref)]), lambda: eng.load_reference_tensors([("20", ref_t)]))
    rows.append(("reference", "pg_load_reference", "pg_load_reference_device", h, d))
    t_mirror, _ = timed(lambda: eng.reference_fetch(0, 0, 64))        # (the device load's deferred cost: the host mirror, on first use)

    h, d = alternate(lambda: eng.upload(batch), lambda: eng.upload_tensors(*reads_t), after=eng.free_device_batch)
    rows.append(("reads", "pg_device_batch_upload", "pg_device_batch_upload_device", h, d))

    db = eng.upload_tensors(*reads_t)
    eng.search_device(db)
    h, d = alternate(lambda: eng.download(db), lambda: eng.download_tensors(db),
                     after=lambda out: out.free() if hasattr(out, "free") else None)
    rows.append(("results", "pg_device_batch_download", "pg_device_batch_download_device (sizes + download)", h, d))
    n_close, n_far = eng.result_sizes(db)
    eng.free_device_batch(db)
    eng.close()

    lines = [f"Shapes: reference {args.chr_len} bp (+ spacers), {batch.n} x {args.read_len} bp reads, "
             f"{n_close} close runs and {n_far} far runs in the result.  Milliseconds per call, host clock around the synchronous "
             f"call, {REPS} alternating repetitions after one warm-up pair: median (min - max).", "",
             "| traffic | host entry | ms | device entry | ms | device / host |", "|---|---|---|---|---|---|"]

    def cell(x):
        return f"{np.median(x):.1f} ({min(x):.1f} - {max(x):.1f})"
    slower = []
    for what, hn, dn, h, d in rows:
        ratio = float(np.median(d) / np.median(h))
        lines.append(f"| {what} | `{hn}` | {cell(h)} | `{dn}` | {cell(d)} | {ratio:.2f} |")
        if ratio > 1.0:
            slower.append(f"`{dn}` is SLOWER than its host sibling here ({ratio:.2f} x).")
    lines += ["", f"First `pg_reference_fetch` after the device load (fills the host mirror, three device-to-host copies): {t_mirror:.1f} ms."]
    lines += [""] + (slower or ["No device entry is slower than its host sibling on these shapes."])
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
