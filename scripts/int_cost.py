#!/usr/bin/env python3
"""What -I costs on the device-classifier path (the figures of profiles/variant/README.md): on a 2 M-read synthetic
set -- the reads of scripts/li_cost.py on chrS, one in twenty replaced by a split read whose far part lies on a second chromosome,
chrT, at one of 200 breakpoints that a hint table (and, for the command line, a BreakDancer file) names --

  * the HIP-event time of pg_device_batch_int over the whole batch (best of 5), its launches, and the bytes a consumer downloads
    per read for the tables;
  * the phase times `pindel_pg -I -b ctx.bd --bd-hints on` prints, without and with --device-classifier --device-classifier-hints
    --device-classifier-int, on the same binary, the runs alternating; the report files of the two modes are compared.

  python scripts/int_cost.py [--reads N] [--chr-len L] [--dir D] [--repeats R] [--parent-exe pindel_pg of the parent commit]
"""
import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
SPACER = 100000
SUFFIXES = ("D", "SI", "TD", "INV", "LI", "BP", "CloseEndMapped", "INT", "INT_final")


def write_fasta(f, name, biol):
    f.write(b">" + name + b"\n")
    rows = biol[:len(biol) // 60 * 60].reshape(-1, 60)
    f.write(np.concatenate([rows, np.full((len(rows), 1), 10, dtype=np.uint8)], axis=1).tobytes())
    if len(biol) % 60:
        f.write(biol[len(rows) * 60:].tobytes() + b"\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--chr-len", type=int, default=40_000_000)
    ap.add_argument("--dir", default="/tmp/int_cost")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--parent-exe", default=None)
    a = ap.parse_args()
    from pindel_amd import binding, synth
    from pindel_amd.binding import HintTable, WINDOW_DTYPE
    from pindel_amd.hostio import ReadBatch
    os.makedirs(a.dir, exist_ok=True)
    n, n_bp, far_len = a.reads, 200, 2_000_000

    def note(what):
        print(f"[{time.strftime('%H:%M:%S')}] {what}", file=sys.stderr, flush=True)
    note("references and reads")
    refs = [synth.make_reference(a.chr_len, seed=3), synth.make_reference(far_len, seed=5)]
    biol = [np.frombuffer(r, dtype=np.uint8)[SPACER:-SPACER] for r in refs]
    fa, reads_txt, bd_path = (os.path.join(a.dir, x) for x in ("ref.fa", "reads.txt", "ctx.bd"))
    with open(fa, "wb") as f:
        write_fasta(f, b"chrS", biol[0])
        write_fasta(f, b"chrT", biol[1])
    b = synth.make_reads(refs[0], n, seed=4)
    seq = np.asarray(b.seq).reshape(n, 100).copy()
    strand, pos = b.anchor_strand.copy(), b.anchor_pos.copy()
    # every twentieth read: 60 bases that end at a breakpoint of chrT + 40 bases of chrS behind a breakpoint there, anchored '-'
    rng = np.random.default_rng(6)
    bp_s = (np.arange(n_bp) + 1) * (a.chr_len // (n_bp + 2)) + rng.integers(0, 1000, n_bp)
    bp_t = (np.arange(n_bp) + 1) * (far_len // (n_bp + 2)) + rng.integers(0, 1000, n_bp)
    junction = np.arange(0, n, 20)
    for i in junction:
        k = int(rng.integers(0, n_bp))
        p, q = int(bp_s[k]), int(bp_t[k])
        cut = int(rng.integers(45, 71))                       # bases of chrT
        seq[i] = np.concatenate([biol[1][q - cut:q], biol[0][p:p + 100 - cut]])
        strand[i] = ord("-")
        pos[i] = p + 100 - cut + int(rng.integers(150, 300))
    order = np.argsort(pos, kind="stable")
    seq, strand, pos = seq[order], strand[order], pos[order]
    with open(reads_txt, "wb") as f:
        for lo in range(0, n, 100_000):
            f.write(b"".join(b"@r%d/1\n%s\n%c\tchrS\t%d\t60\t500\tS1\n" % (k, seq[k].tobytes(), int(strand[k]), int(pos[k]))
                             for k in range(lo, min(lo + 100_000, n))))
    with open(bd_path, "w") as f:
        f.write("#Chr1\tPos1\tOrientation1\tChr2\tPos2\tOrientation2\tType\tSize\tScore\tnum_Reads\n")
        for p, q in zip(bp_s, bp_t):
            f.write(f"chrS\t{int(p)}\t10+0-\tchrT\t{int(q)}\t0+10-\tCTX\t-300\t99\t10\n")
    batch = ReadBatch(seq=seq.reshape(-1), seq_off=(np.arange(n + 1) * 100).astype(np.uint64), anchor_strand=strand, anchor_pos=pos,
                      insert_size=b.insert_size[order], chr_id=b.chr_id[order])
    # the table: the 200 positions around a breakpoint of chrS name the window around its partner on chrT, every other position none
    first, cluster, off = [], [], [0, 0]
    win = np.zeros(n_bp, dtype=WINDOW_DTYPE)
    for k in range(n_bp):
        first += [SPACER + int(bp_s[k]) - 100, SPACER + int(bp_s[k]) + 100]
        cluster += [k + 1, 0]
        win[k] = (1, SPACER + int(bp_t[k]) - 300, SPACER + int(bp_t[k]) + 100)
        off.append(k + 1)
    table = HintTable(first, cluster[:-1], off, win)
    note("hinted search and the junction tables on the GPU")
    eng = binding.Engine(device=0)
    eng.load_reference([("chrS", refs[0]), ("chrT", refs[1])])
    db = eng.upload(batch)
    eng.search_table_device(db, table)
    search_ms = eng.last_stats()[0]
    ms = []
    for _ in range(5):
        eng.clear_launch_log()
        t = eng.int_calls(db)
        ms.append(eng.last_stats()[0])
    launches = len(eng.launch_log())
    nm, nc = len(t["members"]), len(t["calls"])
    fallback = int(((t["calls"]["flags"] & binding.INT_FALLBACK) != 0).sum())
    eng.free_device_batch(db)
    eng.close()
    table_bytes = nm * 4 + nc * 32
    print(f"## {n} synthetic 100-bp reads on chrS ({a.chr_len} bases), {len(junction)} of them split reads towards chrT ({far_len} bases)\n")
    print(f"- pg_device_batch_int (flag and pair walk, compact, counting passes, heads, calls) {min(ms):.3f} ms (best of 5; all: "
          f"{', '.join(f'{x:.3f}' for x in ms)}) = {min(ms) * 1e6 / n:.2f} ns per read, beside the hinted search's {search_ms:.3f} ms of the same run; "
          f"{launches} logged launches (gather, sort passes, tables)")
    print(f"- reads with a call: {nm} ({100.0 * nm / n:.2f} % of the reads), calls {nc}, of them fallback calls {fallback}")
    print(f"- bytes downloaded for the tables: {table_bytes} = {table_bytes / n:.3f} per read (members 4 x {nm / n:.4f}, calls 32 x {nc / n:.5f})\n",
          flush=True)
    exe = os.path.join(os.path.dirname(binding.LIB_PATH), "pindel_pg")
    modes = {"plain": (exe,), "tables": (exe, "--device-classifier", "--device-classifier-hints", "--device-classifier-int")}
    if a.parent_exe:                                          # the parent commit's command line, the baseline of every time
        modes = {"parent": (a.parent_exe,), **modes}
    print("| run | loading | search (GPU, incl. adapters) | classification + reports | three phases | wall |\n|---|---|---|---|---|---|")
    notes = []
    for k in range(a.repeats):
        for mode, extra in modes.items():
            note(f"pindel_pg -I, {mode}, run {k + 1}")
            prefix = os.path.join(a.dir, f"out_{mode}")
            t0 = time.time()
            r = subprocess.run([extra[0], "-f", fa, "-p", reads_txt, "-b", bd_path, "--bd-hints", "on", "-o", prefix, "-I", *extra[1:]],
                               capture_output=True, text=True, timeout=900)
            wall = time.time() - t0
            if r.returncode:
                print(f"pindel_pg failed ({mode}): {r.stderr[-2000:]}")
                return 1
            ph = re.search(r"loading ([\d.]+) s, split-read search \(GPU, incl. adapters\) ([\d.]+) s, classification \+ reports ([\d.]+) s", r.stdout)
            total = sum(float(ph.group(g)) for g in (1, 2, 3))
            print(f"| {mode}, {k + 1} | {ph.group(1)} | {ph.group(2)} | {ph.group(3)} | {total:.2f} | {wall:.2f} |", flush=True)
            if mode == "tables" and k == 0:
                dc = re.search(r"pindel_pg: device classifier:.*", r.stdout)
                dl = re.search(r"pindel_pg: junction tables downloaded:.*", r.stdout)
                notes = [m.group(0) for m in (dc, dl) if m]
    print("\n" + "\n".join("- `" + x + "`" for x in notes))
    read = lambda mode, s: open(os.path.join(a.dir, f"out_{mode}_{s}"), "rb").read()
    same = {s: read("plain", s) == read("tables", s) for s in SUFFIXES}
    print(f"\n- the report files of the two modes byte-identical: {all(same.values())} ({same}); _INT holds "
          f"{os.path.getsize(os.path.join(a.dir, 'out_plain_INT'))} bytes, {read('plain', 'INT').count(10)} lines")
    if a.parent_exe:
        print(f"- the parent's files and the plain run's byte-identical: {all(read('parent', s) == read('plain', s) for s in SUFFIXES)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
