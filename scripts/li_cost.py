#!/usr/bin/env python3
"""What -l costs on the device-classifier path (the figures of profiles/variant/README.md): on the 2 M-read synthetic
set of scripts/variant_cost.py

  * the HIP-event time of pg_device_batch_li over the whole batch as one window (best of 5), its launches, and the bytes a
    consumer downloads per read for the tables;
  * the phase times `pindel_pg -l` prints, without and with --device-classifier --device-classifier-li, on the same binary, the
    runs alternating; the seven report files of the two modes are compared.

  python scripts/li_cost.py [--reads N] [--chr-len L] [--dir D] [--repeats R] [--parent-exe pindel_pg of the parent commit]
"""
import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--chr-len", type=int, default=40_000_000)
    ap.add_argument("--dir", default="/tmp/li_cost")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--parent-exe", default=None)
    a = ap.parse_args()
    from pindel_amd import binding, synth
    from pindel_amd.hostio import ReadBatch
    os.makedirs(a.dir, exist_ok=True)
    n = a.reads

    def note(what):
        print(f"[{time.strftime('%H:%M:%S')}] {what}", file=sys.stderr, flush=True)
    note("reference and reads")
    ref = synth.make_reference(a.chr_len, seed=3)
    biol = np.frombuffer(ref, dtype=np.uint8)[100000:-100000]
    fa, reads_txt = os.path.join(a.dir, "ref.fa"), os.path.join(a.dir, "reads.txt")
    with open(fa, "wb") as f:
        f.write(b">chrS\n")
        rows = biol[:len(biol) // 60 * 60].reshape(-1, 60)
        f.write(np.concatenate([rows, np.full((len(rows), 1), 10, dtype=np.uint8)], axis=1).tobytes())
        if len(biol) % 60:
            f.write(biol[len(rows) * 60:].tobytes() + b"\n")
    b = synth.make_reads(ref, n, seed=4)
    order = np.argsort(b.anchor_pos, kind="stable")
    seq = np.asarray(b.seq).reshape(n, 100)[order]
    strand, pos = b.anchor_strand[order], b.anchor_pos[order]
    with open(reads_txt, "wb") as f:
        for lo in range(0, n, 100_000):
            f.write(b"".join(b"@r%d/1\n%s\n%c\tchrS\t%d\t60\t500\tS1\n" % (k, seq[k].tobytes(), int(strand[k]), int(pos[k]))
                             for k in range(lo, min(lo + 100_000, n))))
    batch = ReadBatch(seq=seq.reshape(-1), seq_off=(np.arange(n + 1) * 100).astype(np.uint64), anchor_strand=strand, anchor_pos=pos,
                      insert_size=b.insert_size[order], chr_id=b.chr_id[order])
    note("search, classify and the long-insertion tables on the GPU")
    eng = binding.Engine(device=0)
    eng.load_reference([("chrS", ref)])
    db = eng.upload(batch)
    eng.search_device(db)
    eng.classify(db, binding.EventWindow(0, 0xffffffff, 0, 0xffffffff, 1, 100, 1, 1))
    classify_ms = eng.last_stats()[0]
    lo, hi = 100000 - 2000, 100000 + a.chr_len + 2000
    ms = []
    for _ in range(5):
        eng.clear_launch_log()
        t = eng.li(db, lo, hi)
        ms.append(eng.last_stats()[0])
    launches = len(eng.launch_log())
    nm, npos = t["n_members"], t["n_positions"]
    eng.free_device_batch(db)
    eng.close()
    table_bytes = sum(nm) * 4 + sum(npos) * 16
    print(f"## {n} synthetic 100-bp reads, reference of {a.chr_len} bases\n")
    print(f"- pg_device_batch_li (flag, compact, counting passes, heads, positions; one window over the chromosome) {min(ms):.3f} ms (best of 5; "
          f"all: {', '.join(f'{x:.3f}' for x in ms)}) = {min(ms) * 1e6 / n:.2f} ns per read, beside pg_device_batch_classify's {classify_ms:.3f} ms "
          f"of the same run; {launches} logged launches (gather, sort passes, tables)")
    print(f"- LI reads '+' / '-': {nm[0]} / {nm[1]} ({100.0 * sum(nm) / n:.1f} % of the reads), positions {npos[0]} / {npos[1]}")
    print(f"- bytes downloaded for the tables: {table_bytes} = {table_bytes / n:.2f} per read (members 4 x {sum(nm) / n:.3f}, positions 16 x "
          f"{sum(npos) / n:.3f})\n", flush=True)
    exe = os.path.join(os.path.dirname(binding.LIB_PATH), "pindel_pg")
    modes = {"plain": (exe,), "tables": (exe, "--device-classifier", "--device-classifier-li")}
    if a.parent_exe:                                          # the parent commit's command line, the baseline of every time
        modes = {"parent": (a.parent_exe,), **modes}
    print("| run | loading | search (GPU, incl. adapters) | classification + reports | of which _LI on the host | wall |\n|---|---|---|---|---|---|")
    notes = []
    for k in range(a.repeats):
        for mode, extra in modes.items():
            note(f"pindel_pg -l, {mode}, run {k + 1}")
            prefix = os.path.join(a.dir, f"out_{mode}")
            t0 = time.time()
            r = subprocess.run([extra[0], "-f", fa, "-p", reads_txt, "-o", prefix, "-l", *extra[1:]], capture_output=True, text=True, timeout=900)
            wall = time.time() - t0
            if r.returncode:
                print(f"pindel_pg failed ({mode}): {r.stderr[-2000:]}")
                return 1
            ph = re.search(r"loading ([\d.]+) s, split-read search \(GPU, incl. adapters\) ([\d.]+) s, classification \+ reports ([\d.]+) s", r.stdout)
            li = re.search(r"long insertions \(_LI, host, part of classification \+ reports\) ([\d.]+) s", r.stdout)
            print(f"| {mode}, {k + 1} | {ph.group(1)} | {ph.group(2)} | {ph.group(3)} | {li.group(1)} | {wall:.2f} |", flush=True)
            if mode == "tables" and k == 0:
                dc = re.search(r"pindel_pg: device classifier:.*", r.stdout)
                dl = re.search(r"pindel_pg: long-insertion tables downloaded:.*", r.stdout)
                notes = [m.group(0) for m in (dc, dl) if m]
    print("\n" + "\n".join("- `" + x + "`" for x in notes))
    same = {s: open(os.path.join(a.dir, f"out_plain_{s}"), "rb").read() == open(os.path.join(a.dir, f"out_tables_{s}"), "rb").read()
            for s in ("D", "SI", "TD", "INV", "LI", "BP", "CloseEndMapped")}
    print(f"\n- the seven report files of the two modes byte-identical: {all(same.values())} ({same}); _LI holds "
          f"{os.path.getsize(os.path.join(a.dir, 'out_plain_LI'))} bytes")
    if a.parent_exe:
        same = all(open(os.path.join(a.dir, f"out_parent_{s}"), "rb").read() == open(os.path.join(a.dir, f"out_plain_{s}"), "rb").read()
                   for s in ("D", "SI", "TD", "INV", "LI", "BP", "CloseEndMapped"))
        print(f"- the parent's seven files and the plain run's byte-identical: {same}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
