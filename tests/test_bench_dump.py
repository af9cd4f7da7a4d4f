"""bench.py --dump-outputs: what the last timed step returned, written as .npy files so that two builds run with the same
arguments can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from conftest import ROOT


def test_dump_outputs_keeps_small_arrays_whole_and_samples_large_ones_at_fixed_positions(tmp_path):
    torch.manual_seed(0)
    model = torch.nn.Linear(3, 2)
    loss, logits = torch.tensor(0.5), torch.arange(10000, dtype=torch.float64)
    budget = 4 * 1000
    runs = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), loss, logits, model, budget=budget)
        runs.append({n: np.load(tmp_path / d / n) for n in sorted(os.listdir(tmp_path / d))})
    a, b = runs
    assert sorted(a) == ["logits.npy", "loss.npy", "param.bias.npy", "param.weight.npy"]
    assert all(v.dtype == np.float32 for v in a.values()) and sum(v.nbytes for v in a.values()) <= budget
    assert a["loss.npy"].shape == () and a["loss.npy"] == np.float32(0.5)
    assert np.array_equal(a["param.weight.npy"], model.weight.detach().numpy())
    assert np.array_equal(a["param.bias.npy"], model.bias.detach().numpy())
    # 1 + 2 + 6 elements whole, the rest of the 1000 for the logits: their values are their positions, sorted, the same twice
    lg = a["logits.npy"]
    assert lg.shape == (991,) and np.all(np.diff(lg) >= 0) and np.all((lg >= 0) & (lg < 10000) & (lg == np.round(lg)))
    assert all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["cfg2", "cfg2mb"])
def test_bench_dump_outputs_of_two_runs_agree(workload, tmp_path):
    """the same arguments twice: the same files, the loss the line reports, logits for every edge of the last step"""
    dumps, lines = [], []
    for d in ("a", "b"):
        p = subprocess.run([sys.executable, "bench.py", "--workload", workload, "--steps", "3", "--warmup", "1",
                            "--no-extras", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / d)],
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        lines.append(json.loads(p.stdout))
        dumps.append({n: np.load(tmp_path / d / n) for n in sorted(os.listdir(tmp_path / d))})
    for line, dump in zip(lines, dumps):
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        assert {"loss.npy", "logits.npy"} <= set(dump) and any(k.startswith("param.") for k in dump)
        assert all(v.dtype == np.float32 for v in dump.values()) and sum(v.nbytes for v in dump.values()) <= 64 << 20
        assert dump["loss.npy"] == np.float32(line["config"]["final_loss"])
        if workload == "cfg2":
            assert dump["logits.npy"].shape == (line["config"]["sim_edges"],)
    a, b = dumps
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and np.allclose(a[k], b[k], rtol=1e-5, atol=1e-6), k
