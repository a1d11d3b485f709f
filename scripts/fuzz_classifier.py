"""Randomised parity hunt for the device classifier: every part of it against its plain-loop host statement (pindel_amd/hostlib.py),
byte for byte, on the inputs of scripts/fuzz_classifier_input.py -- repeat-ridden references, random search parameters, read lengths
from 24 to 300 in one batch, reads drawn several times, planted events on both strands, junction reads, bytes outside ACGTN -- and
random arguments of every part.

    python scripts/fuzz_classifier.py [iterations] [first_seed]

One batch is uploaded once and searched on the device; the downloaded lists feed the host statements (the search itself is
scripts/fuzz_parity.py's business).  Then, each against its statement: variant_candidates, sv_candidates, events, sv_events,
report_reads, classify in one call (against the statements fed the lists cut by hand), li, int_calls (more than one chromosome), and
after a close-only search dd_tables with its containment bits against the CPU containment; a full search afterwards must reproduce
the first download.  Prints one line per iteration and stops at the first mismatch (exit code 1) after saving the seed and the drawn
arguments as fuzz_classifier_fail_<seed>.txt in the directory FUZZ_OUT names (fuzz_out/ without it).  tests/test_gpu_classifier_fuzz.py runs fixed seeds of it."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from pindel_amd import binding
from scripts.fuzz_classifier_input import HostChain, describe, fuzz_input, tally
from tests import test_gpu_events as t_events
from tests import test_gpu_report_reads as t_report
from tests import test_gpu_sv_candidates as t_sv
from tests import test_gpu_sv_events as t_sv_events
from tests import test_gpu_variant_candidates as t_variant
from tests.test_gpu_dd_tables import close_from, contained_by_cpu
from tests.test_gpu_variant_candidates import point_csr


SKIPPED = []            # seeds whose parameters the library rejected (a skip, as in scripts/fuzz_parity.py)


def _search(eng, db, inp):
    if inp.bd is not None:
        eng.set_windows(db, inp.bd, inp.bd_off)
    if inp.search == "search_table_device":
        eng.search_table_device(db, None)
    else:
        getattr(eng, inp.search)(db)
    return eng.download(db)


def _same_tables(got, want, fields, what):
    for f in fields:
        g, w = got[f], want[f]
        same = g == w if isinstance(w, (list, bytes)) else (len(g) == len(w) and g.tobytes() == w.tobytes())
        if not same:
            d = np.nonzero(g != w)[0][:4].tolist() if not isinstance(w, (list, bytes)) and len(g) == len(w) else "sizes"
            raise AssertionError(f"{what}: {f} differs at {d}: device {g[:4] if d == 'sizes' else g[d]}, host {w[:4] if d == 'sizes' else w[d]}")


def compare(eng, db, inp, res, part):
    """The chain of one iteration on a searched batch; part[0] names the part under comparison.  Returns the host chain."""
    n = inp.batch.n
    co, cp = point_csr(res.close_off, res.close_runs)
    fo, fp = point_csr(res.far_off, res.far_runs)
    mm = eng.max_mismatch_table()
    chain = HostChain(inp, dict(rc_flag=res.rc_flag, co=co, cp=cp, fo=fo, fp=fp), mm)
    part[0] = "variant_candidates"
    var = eng.variant_candidates(db)
    t_variant.assert_same(var, chain.variant(), part[0])
    part[0] = "sv_candidates"
    sv = eng.sv_candidates(db, inp.settings)
    t_sv.assert_same(sv, chain.sv(), part[0])
    part[0] = "events"
    t_events.assert_tables_equal(eng.events(db, inp.window, var, sv, inp.name_id), chain.events(), part[0])
    part[0] = "sv_events"
    t_sv_events.assert_tables_equal(eng.sv_events(db, sv), chain.sv_events(), part[0])
    part[0] = "report_reads"
    t_report.assert_same(*eng.report_reads(db, var, sv), *chain.report(), part[0])
    part[0] = f"classify (max_listed {inp.max_listed})"
    eng.classify(db, inp.window, inp.settings, inp.max_listed, inp.name_id)
    ev, svt, rep = chain.classified()
    t_events.assert_tables_equal(eng.events_download(db), ev, part[0] + ", events")
    t_sv_events.assert_tables_equal(eng.sv_events_download(db), svt, part[0] + ", sv events")
    t_report.assert_same(*eng.report_download(db), *rep, part[0] + ", report")
    part[0] = "li"
    _same_tables(eng.li(db, *inp.li), chain.li(), ("n_members", "n_positions", "members_flat", "positions_flat"), part[0])
    if len(inp.chroms) > 1:
        part[0] = "int_calls"
        _same_tables(eng.int_calls(db), chain.int_calls(), ("members", "calls"), part[0])
    part[0] = "dd_tables"
    eng.close_search(db)
    d = inp.dd
    want = chain.dd(close_from(eng.download(db), n)[1:])
    _same_tables(eng.dd_tables(db, d["seg_first"], d["seg_strand"], 0, d["min_bp_support"], d["min_map_distance"]), want, ("members", "cands", "cons"), part[0])
    part[0] = "dd containment"
    got_bits, cpu_bits = contained_by_cpu(dict(chroms=inp.chroms, mm=mm), want)
    assert got_bits == cpu_bits, f"PG_DD_CONTAINED differs from the CPU containment for tested candidates {[i for i, (a, b) in enumerate(zip(got_bits, cpu_bits)) if a != b][:6]}"
    part[0] = "search after the close-only search"
    again = _search(eng, db, inp)
    for f in ("close_off", "close_runs", "far_off", "far_runs", "rc_flag"):
        assert getattr(again, f).tobytes() == getattr(res, f).tobytes(), f"{f} of the second download differs from the first"
    return chain


def one_iteration(seed, n_reads=1500, verbose=True):
    inp = fuzz_input(seed, n_reads)
    try:
        eng = binding.Engine(**inp.kw)
    except binding.PgError as e:          # a parameter set the library rejects
        SKIPPED.append(seed)
        if verbose:
            print(f"seed {seed}: parameters rejected ({e}); skipped")
        return True
    part = ["search"]
    db = None
    try:
        eng.load_reference(inp.chroms)
        db = eng.upload(inp.batch)
        chain = compare(eng, db, inp, _search(eng, db, inp), part)
    except binding.PgError as e:
        if part[0] != "search":
            raise
        SKIPPED.append(seed)
        if verbose:
            print(f"seed {seed}: rejected by the library ({e}); skipped")
        return True
    except AssertionError as e:
        out = os.environ.get("FUZZ_OUT", "fuzz_out")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, f"fuzz_classifier_fail_{seed}.txt"), "w") as f:
            f.write(f"seed {seed} n_reads {n_reads} part {part[0]}\n{describe(inp)}\n{e}\n")
        print(f"seed {seed}: MISMATCH in {part[0]}: {e}\n  {describe(inp)}")
        return False
    finally:
        if db is not None:
            eng.free_device_batch(db)
        eng.close()
    if verbose:
        t = tally(chain)
        print(f"seed {seed}: ok  {inp.search} chromosomes {len(inp.chroms)} lens={inp.lens} params={inp.kw} max_listed {inp.max_listed} "
              f"close>=2 {t['multi_close']} more {t['more']} boxed {t['boxed']} events>=2 {t['multi']} sv {t['sv_events']} "
              f"int {t.get('int', {}).get('calls', '-')} dd {t['dd']['multi']}/{t['dd']['tested']}")
    return True


if __name__ == "__main__":
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    quiet = os.environ.get("FUZZ_QUIET") is not None          # one summary line per call (the committed campaign log)
    for s in range(first, first + iters):
        if not one_iteration(s, verbose=not quiet):
            sys.exit(1)
    print("seeds", first, "..", first + iters - 1, ":", iters - len(SKIPPED), "iterations, every part of the classifier byte-equal to its host statement;",
          len(SKIPPED), "skipped")
