"""CPU: "the read as the close end left it" -- tests/shortening_cases.py's flip / post_state / unflipped, which the GPU tests of the
two far-end seams (tests/test_gpu_far_seam_states.py) upload -- against the oracle's own post-state, and pg_adapter's
apply_rc_flag / make_batch(..., un_rc) against that helper (a stand-alone host program built with -fsanitize=address,undefined)."""
import os
import subprocess

import numpy as np
import pytest

from pindel_amd import synth
from tests import shortening_cases as sc
from tests.parity import run_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (64, 100, 128)


@pytest.fixture(scope="module")
def ref():
    return [("chrS", synth.make_reference(600_000, seed=31))]


def _odd():
    return sc.batch_of([b"R" * 40, b"*" * 12, b"RRRRACGT", b"ACGTACGTACGTR", b"NACGTTGCAACGTTGCAACGTR*"],
                       [ord("+"), ord("-"), ord("+"), ord("-"), ord("+")], [200000] * 5, [500] * 5)


def _batches(ref_seq, L):
    out = [sc.seam_family(ref_seq, fam, L) for fam in sc.SEAM_FAMILIES]
    out.append(sc.moved(sc.clean_reads(ref_seq, 300, L, seed=sc.SEAM_SEED[L])))                # clean, found at attempt 3: flag 0
    out.append(synth.make_reads(ref_seq, 300, seed=60 + L, read_len=L))                        # ordinary reads, flags 0 and 1
    return out


@pytest.fixture(scope="module")
def oracle_states(ref):
    """(batch, the oracle's result) for every family at every length, and the odd batch"""
    out = []
    for L in LENGTHS:
        for b in _batches(ref[0][1], L):
            out.append((b, run_oracle({}, ref, b)))
    odd = _odd()
    out.append((odd, run_oracle({}, ref, odd)))
    return out


def test_flip_by_hand():
    assert sc.flip(b"ACGTN") == b"NACGT"
    assert sc.flip(b"RYACGG") == b"CCGT"                         # leading junk -> trailing NUL -> stripped
    assert sc.flip(b"ACGGRK") == b"\0\0CCGT"                     # trailing junk -> leading NUL: stays ...
    assert sc.flip(sc.flip(b"ACGGRK")) == b"ACGG"                # ... until the second reverse complement
    assert sc.flip(sc.flip(b"ACRGG")) == b"AC\0GG"
    assert sc.flip(b"RRR") == b"" and sc.flip(b"") == b""
    b = sc.batch_of([b"ACGGRK", b"RYACGG", b"ACGT"], [43] * 3, [5, 6, 7], [500] * 3)
    post = sc.post_state(b, [2, 1, 0])
    assert sc.seqs_of(post) == [b"ACGG", b"CCGT", b"ACGT"] and list(post.anchor_pos) == [5, 6, 7]
    assert sc.seqs_of(sc.unflipped(post, [2, 1, 0])) == [b"ACGG", b"ACGG", b"ACGT"]
    assert sc.seqs_of(sc.unflipped(sc.batch_of([b"\0CC"], [43], [5], [500]), [1])) == [b"GG\0"]


def test_post_state_is_what_the_oracle_leaves(oracle_states):
    n = differ = 0
    flags = np.zeros(3, dtype=np.int64)
    for batch, orc in oracle_states:
        post = sc.post_state(batch, orc["rc_flag"])
        off = batch.seq_off.astype(np.int64)
        for i, s in enumerate(sc.seqs_of(post)):
            want = orc["seq"][off[i]:off[i] + int(orc["len_out"][i])].tobytes()
            differ += s != want
            n += 1
        flags += np.bincount(orc["rc_flag"], minlength=3)[:3]
    assert n == len(LENGTHS) * 9 * 300 + 5
    assert differ == 0, f"{differ} of {n} reads"
    assert (flags > 1000).all(), flags                              # every flag value is well represented


@pytest.fixture(scope="module")
def seam_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("seam") / "adapter_seam_states"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pindel_amd", "csrc", "host"),
                    "-I" + os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "adapter_seam_states.cpp"), "-pthread",
                    "-o", str(exe)], check=True)
    return str(exe)


def _hex(s):
    return s.hex() if s else "-"


@pytest.mark.parametrize("read_type", ["ref", "plain"])
def test_adapter_post_state_and_upload_equal_the_helper(oracle_states, seam_program, read_type):
    """apply_rc_flag with the oracle's flags, then make_batch(..., un_rc): the sequence left in the read and the bytes uploaded for
    pg_far_end_batch.  Every read also goes in with the two flags the oracle did not give it."""
    lines, want = [], []
    for batch, orc in oracle_states:
        for k in range(3):
            flag = (orc["rc_flag"].astype(np.int64) + k) % 3 if k else orc["rc_flag"]
            if k and batch.n > 5:
                flag = flag[:40]
            sub = batch.slice(0, len(flag)) if len(flag) < batch.n else batch
            post = sc.post_state(sub, flag)
            for s, p, u, f in zip(sc.seqs_of(sub), sc.seqs_of(post), sc.seqs_of(sc.unflipped(post, flag)), flag):
                lines.append(f"{_hex(s)} {int(f)}")
                want.append(f"{_hex(p)} {_hex(u)}")
    assert len(lines) > 8000
    run = subprocess.run([seam_program, read_type], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]          # (the sanitizers report on stderr)
    got = run.stdout.splitlines()
    assert len(got) == len(want)
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (len(bad), lines[bad[0]], got[bad[0]], want[bad[0]])
