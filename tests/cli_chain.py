"""pindel_pg runs for the GPU tests of the input flags: every run under a time limit of its own, and chained -- once a run
has timed out or died of a signal, no later run of the session is started (the device may be in trouble; the first failure is
the finding)."""
import os
import subprocess

from pindel_amd import binding

EXE = os.path.join(os.path.dirname(binding.LIB_PATH), "pindel_pg")
_broken = []


def run(args, timeout=120, env=None, expect=0):
    """-> the finished process; asserts its exit status is `expect`"""
    assert not _broken, f"not started: an earlier pindel_pg run ended abnormally ({_broken[0]})"
    e = dict(os.environ)
    e.pop("PGH_THREADS", None)               # (-T sets it only where it is not set)
    e.update(env or {})
    cmd = [EXE] + [str(a) for a in args]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, env=e, timeout=timeout)
    except subprocess.TimeoutExpired:
        _broken.append("time limit: " + " ".join(cmd))
        raise
    if out.returncode < 0 or out.returncode in (124, 134, 137, 139):
        _broken.append(f"status {out.returncode}: " + " ".join(cmd))
    assert out.returncode == expect, (out.returncode, out.stderr[-2000:])
    return out


def read(path):
    with open(path, "rb") as fh:
        return fh.read()
