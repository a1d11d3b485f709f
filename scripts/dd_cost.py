#!/usr/bin/env python3
"""What -q costs on the device-classifier path (the figures of profiles/variant/README.md): on a BAM in the style of
tests/dd_synth.py scaled up -- more planted dispersed duplications, a read pair every base instead of every third --

  * the HIP-event time of pg_device_batch_close_search and of pg_device_batch_dd (best of 5) over the split reads the -q pipeline
    hands to its close-end step for the whole chromosome, as ONE batch with one segment per anchor strand, and the bytes of the tables
    a consumer downloads per split read against the bytes of the close-end result (runs, offsets, summaries) the plain path downloads;
  * the wall time and the `dispersed duplications:` lines of `pindel_pg -q --MIN_DD_MAP_DISTANCE 400`, without and with
    --device-classifier --device-classifier-hints --device-classifier-dd, three runs each, alternating; the report files are compared.

  python scripts/dd_cost.py [--events N] [--dir D] [--repeats R] [--parent-exe pindel_pg of the parent commit]
"""
import argparse
import ctypes as C
import os
import re
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
SUFFIXES = ("D", "SI", "TD", "INV", "LI", "BP", "CloseEndMapped", "DD")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=60)
    ap.add_argument("--dir", default="/tmp/dd_cost")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-exe", default=None)
    a = ap.parse_args()
    from pindel_amd import binding, hostio
    from tests import dd_restated, dd_synth
    os.makedirs(a.dir, exist_ok=True)

    def note(what):
        print(f"[{time.strftime('%H:%M:%S')}] {what}", file=sys.stderr, flush=True)
    note("the BAM")
    dd_synth.STEP = 1
    chr_len = 4000 * (a.events + 2)
    events = tuple((4000 * (k + 1), 4000 * (k + 1) + 1500, 400) for k in range(a.events))
    syn = dd_synth.make(a.dir, events=events, dropped=tuple(range(1, a.events, 2)), chr_len=chr_len)
    chroms = hostio.load_fasta(syn["fasta"])
    # the split reads of the pipeline's close-end step: captured from the host pipeline (no close end given back)
    captured = []

    def cb(n, seq, off, strand, pos, isz, chr_, has, rcf, last_abs, last_len):
        offs = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), (n + 1,)).copy()
        got = [np.ctypeslib.as_array(C.cast(seq, C.POINTER(C.c_uint8)), (int(offs[-1]),)).copy(), offs]
        for ptr, ty in ((strand, C.c_uint8), (pos, C.c_int32), (isz, C.c_int16), (chr_, C.c_int32)):
            got.append(np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ty)), (n,)).copy())
        captured.append(got)
        return 0
    eng = binding.Engine(device=0)
    eng.load_reference(chroms)
    mm = eng.max_mismatch_table()
    note("the split reads of -q")
    dd_restated.dd_run(syn["fasta"], syn["config"], os.path.join(a.dir, "capture"), mm, opts=(350, 100, 3, 3, 400, 0), close_cb=dd_restated.CLOSE_CB(cb))
    seq, off, strand, pos, isz, chr_ = max(captured, key=lambda g: len(g[2]))
    n = len(strand)
    lens = np.diff(off.astype(np.int64))
    order = np.argsort(strand != ord("+"), kind="stable")          # the '+' anchors, then the '-' anchors: one segment each
    seqs = [seq[int(off[i]):int(off[i + 1])].tobytes() for i in order]
    batch = hostio.batch_from_lists(seqs, [bytes([strand[i]]) for i in order], pos[order], isz[order], chr_[order])
    n_plus = int((strand == ord("+")).sum())
    first, sstrand = np.array([0, n_plus, n], dtype=np.uint32), b"+-"
    chr_id = int(chr_[0])
    note("close-only search and the DD tables on the GPU")
    res = eng.close_end_batch(batch)
    plain_bytes = res.close_runs.nbytes + res.close_off.nbytes + n * 7
    db = eng.upload(batch)
    close_ms, dd_ms = [], []
    for _ in range(5):
        eng.close_search(db)
        close_ms.append(eng.last_stats()[0])
        eng.clear_launch_log()
        t = eng.dd_tables(db, first, sstrand, chr_id, 3, 400)
        dd_ms.append(eng.last_stats()[0])
    launches = len(eng.launch_log())
    eng.free_device_batch(db)
    eng.close()
    nm, nc, nb = len(t["members"]), len(t["cands"]), len(t["cons"])
    table_bytes = nm * 8 + nc * 40 + nb
    tested = int(((t["cands"]["flags"] & 1) != 0).sum())
    contained = int(((t["cands"]["flags"] & 2) != 0).sum())
    print(f"## {a.events} planted dispersed duplications on a chromosome of {chr_len} bases, a read pair every base: {n} split reads "
          f"(mean length {lens.mean():.1f}) in the largest window\n")
    print(f"- pg_device_batch_close_search {min(close_ms):.3f} ms (best of 5; all: {', '.join(f'{x:.3f}' for x in close_ms)})")
    print(f"- pg_device_batch_dd (flag, compact, counting passes, keys, members, consensus, pool, containment, verdicts) {min(dd_ms):.3f} ms "
          f"(best of 5; all: {', '.join(f'{x:.3f}' for x in dd_ms)}); {launches} logged launches")
    print(f"- members {nm}, candidates {nc} (tested {tested}, contained {contained}), consensus pool {nb} bytes")
    print(f"- bytes downloaded for the tables: {table_bytes} = {table_bytes / n:.2f} per split read; the close-end result the plain path downloads "
          f"(runs, offsets, summaries): {plain_bytes} = {plain_bytes / n:.2f} per split read\n", flush=True)
    exe = os.path.join(os.path.dirname(binding.LIB_PATH), "pindel_pg")
    modes = {"plain": (exe,), "tables": (exe, "--device-classifier", "--device-classifier-hints", "--device-classifier-dd")}
    if a.parent_exe:                                          # the parent commit's command line, the baseline of every time
        modes = {"parent": (os.path.abspath(a.parent_exe),), **modes}
    print("| run | loading | search (GPU, incl. adapters) | classification + reports | -q consensus tests (s) | wall |\n|---|---|---|---|---|---|")
    notes = []
    for k in range(a.repeats):
        for mode, extra in modes.items():
            note(f"pindel_pg -q, {mode}, run {k + 1}")
            prefix = os.path.join(a.dir, f"out_{mode}")
            t0 = time.time()
            r = subprocess.run([extra[0], "-f", syn["fasta"], "-i", syn["config"], "-o", prefix, "-q", "--MIN_DD_MAP_DISTANCE", "400", *extra[1:]],
                               capture_output=True, text=True, timeout=900, cwd=a.dir)
            wall = time.time() - t0
            if r.returncode:
                print(f"pindel_pg failed ({mode}): {r.stderr[-2000:]}")
                return 1
            ph = re.search(r"loading ([\d.]+) s, split-read search \(GPU, incl. adapters\) ([\d.]+) s, classification \+ reports ([\d.]+) s", r.stdout)
            dd = re.search(r"consensus tests \(GPU ([\d.]+) s", r.stdout)
            print(f"| {mode}, {k + 1} | {ph.group(1)} | {ph.group(2)} | {ph.group(3)} | {dd.group(1)} | {wall:.2f} |", flush=True)
            if mode == "tables" and k == 0:
                notes = [m.group(0) for m in re.finditer(r"pindel_pg: dispersed duplications:.*", r.stdout)]
    print("\n" + "\n".join("- `" + x + "`" for x in notes))
    read = lambda mode, s: open(os.path.join(a.dir, f"out_{mode}_{s}"), "rb").read()
    same = {s: read("plain", s) == read("tables", s) for s in SUFFIXES}
    n_events = read("plain", "DD").count(b"\tDD\t")
    print(f"\n- the report files of the two modes byte-identical: {all(same.values())} ({same}); _DD holds "
          f"{os.path.getsize(os.path.join(a.dir, 'out_plain_DD'))} bytes, {n_events} events")
    if a.parent_exe:
        print(f"- the parent's files and the plain run's byte-identical: {all(read('parent', s) == read('plain', s) for s in SUFFIXES)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
