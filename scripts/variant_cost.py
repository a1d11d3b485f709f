"""Measurement (one MI355X + its host): what the device classifiers (pg_variant_kernel; pg_sv_kernel, 7l; the events entry,
7m; the sv events entry, 7n) cost and what
they take off the host.  On n synthetic 100-bp reads (all SV types, default parameters), searched on the GPU:
  * the kernel's HIP-event time, per batch and per read;
  * the host's `deletions` and `short insertions` laps of call_from_points (PGH_TIMING=1: the per-read stage plus the
    kind's box sorting and reporting) without and with the candidate lists, next to the other classifiers' laps;
  * pg_sv_kernel's HIP-event time beside it, and the five laps it feeds (`indels (DI)`, `tandem dup`, `tandem dup NT`, `inversions`,
    `inversions NT`) with the lists of both kernels (column `sv`);
  * with --parent-lib: the same two laps of a libpindel_host.so built from the parent commit, on the same points.
Prints a markdown block (profiles/variant/README.md quotes it).

    python scripts/variant_cost.py [--reads 2000000] [--chr-len 40000000] [--parent-lib path/to/libpindel_host.so] [--dir /tmp/variant_cost]
                                   [--device-only]      (the device stages alone: no host runs)
"""
import argparse
import ctypes as C
import os
import re
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from pindel_amd import hostlib

ARRAYS = ("co", "cp", "fo", "fp", "rc_flag", "cands", "counts", "sv_cands", "sv_counts", "mm")
SV_LAPS = ("indels (DI)", "tandem dup", "tandem dup NT", "inversions", "inversions NT")


def child(mode, work, parent_lib):
    """one call_from_points in a process of its own (PGH_TIMING is read once per process; a second host library cannot share one)"""
    a = {k: np.load(os.path.join(work, k + ".npy"), mmap_mode="r") for k in ARRAYS}
    if mode == "parent":
        L = C.CDLL(parent_lib)
        L.pgh_last_error.restype = C.c_char_p
        L.pgh_call_from_points.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(hostlib.HostSettings), C.c_uint32] + [C.c_void_p] * 5
        hostlib._lib = L
    st = hostlib.default_settings(a["mm"])
    lists = (a["cands"], a["counts"]) if mode in ("lists", "sv") else None
    sv = (a["sv_cands"], a["sv_counts"]) if mode == "sv" else None
    t0 = time.time()
    hostlib.call_from_points(os.path.join(work, "ref.fa"), os.path.join(work, "reads.txt"), os.path.join(work, "out_" + mode), st,
                             a["co"], a["cp"], a["fo"], a["fp"], a["rc_flag"], variant_candidates=lists, sv_candidates=sv)
    print(f"wall {time.time() - t0:.3f}")
    if mode in ("lists", "sv"):
        print(f"fallbacks {hostlib.last_variant_fallbacks()}")


def laps_of(mode, work, parent_lib):
    env = dict(os.environ, PGH_TIMING="1")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--dir", work] + (["--parent-lib", parent_lib] if parent_lib else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError(f"{mode}: {r.stderr[-2000:]}")
    laps = {}
    for what, sec in re.findall(r"pgh timing: (.+?)\s+([0-9.]+) s \(\d+ reads\)", r.stderr):
        laps[what.strip()] = laps.get(what.strip(), 0.0) + float(sec)
    m = re.search(r"classify \+ report ([0-9.]+) s", r.stderr)
    extra = {"wall": float(re.search(r"wall ([0-9.]+)", r.stdout).group(1)), "classify + report": float(m.group(1)) if m else float("nan")}
    f = re.search(r"fallbacks (\d+)", r.stdout)
    if f:
        extra["fallbacks"] = int(f.group(1))
    return laps, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--chr-len", type=int, default=40_000_000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--dir", default="/tmp/variant_cost")
    ap.add_argument("--child", default=None)
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.dir, a.parent_lib)
    from pindel_amd import binding, synth
    os.makedirs(a.dir, exist_ok=True)
    n = a.reads

    def note(what):
        print(f"[{time.strftime('%H:%M:%S')}] {what}", file=sys.stderr, flush=True)
    note("reference and reads")
    ref = synth.make_reference(a.chr_len, seed=3)
    biol = np.frombuffer(ref, dtype=np.uint8)[100000:-100000]
    with open(os.path.join(a.dir, "ref.fa"), "wb") as f:
        f.write(b">chrS\n")
        rows = biol[:len(biol) // 60 * 60].reshape(-1, 60)
        f.write(np.concatenate([rows, np.full((len(rows), 1), 10, dtype=np.uint8)], axis=1).tobytes())
        if len(biol) % 60:
            f.write(biol[len(rows) * 60:].tobytes() + b"\n")
    b = synth.make_reads(ref, n, seed=4)
    order = np.argsort(b.anchor_pos, kind="stable")
    seq = np.asarray(b.seq).reshape(n, 100)[order]
    strand, pos = b.anchor_strand[order], b.anchor_pos[order]
    with open(os.path.join(a.dir, "reads.txt"), "wb") as f:
        for lo in range(0, n, 100_000):
            f.write(b"".join(b"@r%d/1\n%s\n%c\tchrS\t%d\t60\t500\tS1\n" % (k, seq[k].tobytes(), int(strand[k]), int(pos[k]))
                             for k in range(lo, min(lo + 100_000, n))))
    from pindel_amd.hostio import ReadBatch
    batch = ReadBatch(seq=seq.reshape(-1), seq_off=(np.arange(n + 1) * 100).astype(np.uint64), anchor_strand=strand, anchor_pos=pos,
                      insert_size=b.insert_size[order], chr_id=b.chr_id[order])
    note("search and classify on the GPU")
    eng = binding.Engine(device=0)
    eng.load_reference([("chrS", ref)])
    db = eng.upload(batch)
    eng.search_device(db)
    search_ms = eng.last_stats()[0]
    ms = []
    for _ in range(5):
        cands, counts = eng.variant_candidates(db)
        ms.append(eng.last_stats()[0])
    sv_ms = []
    for _ in range(5):
        sv_cands, sv_counts = eng.sv_candidates(db)
        sv_ms.append(eng.last_stats()[0])
    # the events stage: one window over the whole chromosome, lists and tables in device memory
    note("event tables on the GPU")
    vt, svt = eng.variant_candidates_tensors(db), eng.sv_candidates_tensors(db)
    ev_ms = []
    for _ in range(5):
        eng.clear_launch_log()
        ev = eng.events_tensors(db, binding.EventWindow(0, 0xffffffff, 0, 0xffffffff, 1, 100, 1, 1), vt, svt)
        ev_ms.append(eng.last_stats()[0])
    ev_sorts = sum(1 for r in eng.launch_log() if r.kernel == binding.KERNEL_EVENT_SORT)
    # the sv events stage over the records of that build: DI, INV and INV_NT
    note("sv event tables on the GPU")
    svev_ms = []
    for _ in range(5):
        svev = eng.sv_events_tensors(db, svt)
        svev_ms.append(eng.last_stats()[0])
    # the report records over those two builds, then the whole window in one call with the lists kept on the device
    note("report records and classify on the GPU")
    rr_ms = []
    for _ in range(5):
        eng.report_reads_tensors(db, vt, svt)
        rr_ms.append(eng.last_stats()[0])
    cl_ms = []
    for _ in range(5):
        eng.classify(db, binding.EventWindow(0, 0xffffffff, 0, 0xffffffff, 1, 100, 1, 1))
        cl_ms.append(eng.last_stats()[0])
    n_records = eng.report_sizes(db)[0]
    cl_ev, cl_sv = eng.event_sizes(db), eng.sv_event_sizes(db)
    ev_reads = binding.events_from_tensors(ev)["reads"]
    del vt, svt
    res = eng.download(db)
    eng.free_device_batch(db)

    def csr(off, runs):
        per_run = runs["len_last"].astype(np.int64) - runs["len_first"].astype(np.int64) + 1
        cum = np.concatenate([[0], np.cumsum(per_run)])
        return cum[off.astype(np.int64)].astype(np.uint64), binding.expand_runs(runs)
    note("expand and save the points")
    co, cp = csr(res.close_off, res.close_runs)
    fo, fp = csr(res.far_off, res.far_runs)
    arrays = dict(co=co, cp=cp, fo=fo, fp=fp, rc_flag=np.asarray(res.rc_flag), cands=cands, counts=counts, sv_cands=sv_cands, sv_counts=sv_counts,
                  mm=eng.max_mismatch_table())
    for k in ARRAYS:
        np.save(os.path.join(a.dir, k + ".npy"), arrays[k])
    listed = counts & 0x7f
    print(f"## {n} synthetic 100-bp reads, reference of {a.chr_len} bases\n")
    print(f"- runs per read {(len(res.close_runs) + len(res.far_runs)) / n:.2f}, points per read {(len(cp) + len(fp)) / n:.1f}")
    print(f"- reads with a deletion candidate {(listed[:, 0] > 0).sum()}, with an insertion candidate {(listed[:, 1] > 0).sum()}, "
          f"lists with more pairs behind them {((counts & 0x80) != 0).sum()}")
    print(f"- search kernel {search_ms:.2f} ms; pg_variant_kernel {min(ms):.3f} ms (best of 5; all: {', '.join(f'{x:.3f}' for x in ms)}) = "
          f"{min(ms) * 1e6 / n:.2f} ns per read")
    sv_listed = sv_counts & 0x7f
    print("- reads with a candidate of DI / TD / TD NT / INV / INV NT: " + " / ".join(str(int((sv_listed[:, k] > 0).sum())) for k in range(5)) +
          f", lists with more pairs behind them {((sv_counts & 0x80) != 0).sum()}")
    print(f"- pg_sv_kernel {min(sv_ms):.3f} ms (best of 5; all: {', '.join(f'{x:.3f}' for x in sv_ms)}) = {min(sv_ms) * 1e6 / n:.2f} ns per read\n",
          flush=True)
    print(f"- events entry (cascade, sort, duplicates, events; lists and tables in device memory) {min(ev_ms):.3f} ms (best of 5; all: "
          f"{', '.join(f'{x:.3f}' for x in ev_ms)}) = {min(ev_ms) * 1e6 / n:.2f} ns per read; members per table {ev['n_members']}, events per table "
          f"{ev['n_events']}, unresolved reads {ev['unresolved']}, sort passes launched (of 17 key bytes) {ev_sorts}\n", flush=True)
    # the largest box of the three kinds, from the records of the events build: what the sequential passes of one wave see
    recs = ev_reads
    sv_flat = np.asarray(sv_cands).reshape(n, binding.SV_SLOTS)
    box = 0
    for kind in binding.SV_EVENT_KINDS:
        idx = np.nonzero(((recs["flags"] & binding.EVR_BOXED) != 0) & (recs["kind"] == kind))[0]
        if len(idx):
            left = sv_flat["bp_left"][idx, binding.SV_SLOT[kind] + recs["slot"][idx].astype(np.int64)]
            box = max(box, int(np.bincount(left // max(len(ref) // 30000, 1)).max()))
    print(f"- sv events entry (DI, INV, INV_NT: gather, segment and key sorts, record-shift passes per box, duplicates, runs, events; lists "
          f"and tables in device memory) {min(svev_ms):.3f} ms (best of 5; all: {', '.join(f'{x:.3f}' for x in svev_ms)}) = "
          f"{min(svev_ms) * 1e6 / n:.2f} ns per read, beside the events entry's {min(ev_ms):.3f} ms of the same run; members per table "
          f"{svev['n_members']}, events per table {svev['n_events']}, dropped runs {svev['dropped_runs']}, largest box {box} reads\n", flush=True)
    # what a caller of classify downloads (per-read records, member lists, events, report records, summaries) beside the search result
    # (offsets, runs, rc flags) it no longer needs
    table_bytes = n * 8 + (sum(cl_ev[0]) + sum(cl_sv[0])) * 4 + (sum(cl_ev[1]) + sum(cl_sv[1])) * 40 + n_records * 48 + n * 12
    point_bytes = (n + 1) * 16 + (len(res.close_runs) + len(res.far_runs)) * 12 + n
    print(f"- report records entry (one thread per member, one per read) {min(rr_ms):.3f} ms (best of 5; all: "
          f"{', '.join(f'{x:.3f}' for x in rr_ms)}) = {min(rr_ms) * 1e6 / n:.2f} ns per read; {n_records} records\n"
          f"- pg_device_batch_classify (both candidate kernels, both table builds, the records; sum of the stages' HIP-event times) "
          f"{min(cl_ms):.3f} ms (best of 5; all: {', '.join(f'{x:.3f}' for x in cl_ms)}) = {min(cl_ms) * 1e6 / n:.2f} ns per read\n"
          f"- bytes a consumer downloads per read: tables, records and summaries {table_bytes / n:.1f}; the run-length-encoded search "
          f"result {point_bytes / n:.1f} (expanded on the host to {(len(cp) + len(fp)) * 12 / n:.0f} bytes of points)\n", flush=True)
    if a.device_only:
        return
    modes = ["plain", "lists", "sv"] + (["parent"] if a.parent_lib else [])
    got = {}
    for m in modes:
        note(f"host run: {m}")
        got[m] = laps_of(m, a.dir, a.parent_lib)
    names = list(got["plain"][0])
    print("| lap (s) | " + " | ".join(modes) + " |\n|---|" + "---|" * len(modes))
    for what in names:
        print(f"| {what} | " + " | ".join(f"{got[m][0].get(what, float('nan')):.3f}" for m in modes) + " |")
    for what in ("classify + report", "wall"):
        print(f"| {what} (whole call) | " + " | ".join(f"{got[m][1][what]:.3f}" for m in modes) + " |")
    p = got["plain"][0]
    total = sum(p.values())
    two = p.get("deletions", 0.0) + p.get("short insertions", 0.0)
    saved = two - got["lists"][0].get("deletions", 0.0) - got["lists"][0].get("short insertions", 0.0)
    print(f"\n- `deletions` + `short insertions` = {two:.3f} s of {total:.3f} s in laps ({100 * two / total:.1f} %); with the lists they "
          f"take {two - saved:.3f} s: the per-read stage was {saved:.3f} s ({100 * saved / total:.1f} % of the laps)")
    print(f"- reads that fell back to the pair search: {got['lists'][1].get('fallbacks')}")
    five = sum(p.get(k, 0.0) for k in SV_LAPS)
    five_sv = sum(got["sv"][0].get(k, 0.0) for k in SV_LAPS)
    print(f"- the five laps pg_sv_kernel feeds = {five:.3f} s of {total:.3f} s ({100 * five / total:.1f} %); with its lists they take {five_sv:.3f} s: "
          f"their per-read stage was {five - five_sv:.3f} s ({100 * (five - five_sv) / total:.1f} % of the laps); fallbacks with all seven lists: "
          f"{got['sv'][1].get('fallbacks')}")
    all_sv = sum(got["sv"][0].values())
    print(f"- host time of the stages the events entry stands for (window tail, box sorting, duplicates, grouping -- and the report "
          f"formatting, which stays on the host): all laps with the lists of both kernels = {all_sv:.3f} s, against {min(ev_ms) / 1e3:.4f} s "
          f"on the device")
    same = all(open(os.path.join(a.dir, f"out_plain_{s}"), "rb").read() == open(os.path.join(a.dir, f"out_{m}_{s}"), "rb").read()
               for s in ("D", "SI", "TD", "INV") for m in ("lists", "sv"))
    print(f"- reports with and without the lists byte-identical: {same}")


if __name__ == "__main__":
    main()
