"""The checks the tensor wrappers of pindel_amd.binding make before the library is called (no GPU needed)."""
import os
import subprocess
import sys

import pytest

from pindel_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reads(n=4, length=10):
    import torch
    return dict(seq=torch.zeros(n * length, dtype=torch.uint8), seq_off=torch.arange(0, (n + 1) * length, length, dtype=torch.int64),
                anchor_strand=torch.full((n,), ord("+"), dtype=torch.uint8), anchor_pos=torch.zeros(n, dtype=torch.int32),
                insert_size=torch.zeros(n, dtype=torch.int16), chr_id=torch.zeros(n, dtype=torch.int32))


def test_well_formed_tensors_pass():
    assert binding.check_read_tensors(device="cpu", **_reads()) == 4
    assert binding.check_read_tensors(device="cpu", **_reads(n=0)) == 0


@pytest.mark.parametrize("name", ["seq", "seq_off", "anchor_strand", "anchor_pos", "insert_size", "chr_id"])
def test_wrong_dtype(name):
    import torch
    r = _reads()
    r[name] = r[name].to(torch.float32)
    with pytest.raises(ValueError, match=name):
        binding.check_read_tensors(device="cpu", **r)


def test_non_contiguous():
    import torch
    r = _reads()
    r["anchor_pos"] = torch.zeros(8, dtype=torch.int32)[::2]
    with pytest.raises(ValueError, match="anchor_pos: not contiguous"):
        binding.check_read_tensors(device="cpu", **r)
    with pytest.raises(ValueError, match="not contiguous"):
        binding.check_reference_tensors([("c", torch.zeros(64, dtype=torch.uint8)[::2])], "cpu")


def test_cpu_tensor_where_the_engines_gpu_is_expected():
    import torch
    with pytest.raises(ValueError, match="on cpu, expected cuda:0"):
        binding.check_read_tensors(device="cuda:0", **_reads())
    with pytest.raises(ValueError, match="on cpu, expected cuda:0"):
        binding.check_reference_tensors([("c", torch.zeros(64, dtype=torch.uint8))], "cuda:0")
    with pytest.raises(ValueError, match="torch tensor"):
        binding.check_tensor("x", [1, 2, 3], ("torch.uint8",), "cpu")


def test_short_seq_and_wrong_lengths():
    r = _reads()
    r["seq"] = r["seq"][:39]
    with pytest.raises(ValueError, match="shorter than seq_off"):
        binding.check_read_tensors(device="cpu", **r)
    r = _reads()
    r["chr_id"] = r["chr_id"][:3]
    with pytest.raises(ValueError, match="chr_id: 3 elements, expected 4"):
        binding.check_read_tensors(device="cpu", **r)
    r = _reads()
    r["seq_off"] = r["seq_off"][:0]
    with pytest.raises(ValueError, match="seq_off"):
        binding.check_read_tensors(device="cpu", **r)


def test_runs_from_tensor_views_the_run_records():
    import numpy as np
    import torch
    runs = np.zeros(3, dtype=binding.RUN_DTYPE)
    runs["abs_loc_first"] = [5, 70000, 2 ** 31 + 9]
    runs["len_last"] = [1, 2, 499]
    runs["chr_id"] = [0, -1, 7]
    t = torch.from_numpy(runs.view(np.uint8).reshape(3, 12).copy())
    assert binding.runs_from_tensor(t).tobytes() == runs.tobytes()
    assert binding.runs_from_tensor(torch.zeros((0, 12), dtype=torch.uint8)).shape == (0,)


def test_binding_imports_without_torch():
    """`import torch` happens inside the tensor methods only: the module loads where torch cannot be imported."""
    code = ("import sys; sys.modules['torch'] = None\n"
            "from pindel_amd import binding\n"
            "assert hasattr(binding.Engine, 'upload_tensors') and 'pg_load_reference_device' in binding.EXPORTS\n"
            "try:\n    import torch\nexcept ImportError:\n    print('no torch, binding ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and "no torch, binding ok" in r.stdout, r.stderr
