"""bench.py --dump-outputs: what the last timed pass handed its caller, as DIR/<name>.npy, the same on every run of the same arguments
and within the size budget (CPU: the stub workload, host-only; the real workloads' dumps are taken by `python bench.py` on the GPU box)."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "diff-hybrid-traffic-sim_amd")]
import bench  # noqa: E402


def _stub(args, timeout=120):
    env = dict(os.environ, OMP_NUM_THREADS="1", HIP_VISIBLE_DEVICES="-1")      # host-only, like the stub launcher tests
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "stub", "--gpus", "1"] + args, env=env,
                          capture_output=True, text=True, timeout=timeout)


def test_dump_outputs_of_the_last_timed_pass_are_reproducible(tmp_path):
    got = []
    for run in ("a", "b"):
        p = _stub(["--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / run)])
        assert p.returncode == 0, p.stderr[-2000:]
        o = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
        assert o["steps"] == 3 and o["warmup"] == 1 and o["ms_per_step"] > 0
        assert sorted(os.listdir(tmp_path / run)) == ["g_action.npy", "loss.npy"]
        got.append({n: np.load(tmp_path / run / (n + ".npy")) for n in ("g_action", "loss")})
    a = np.arange(6, dtype=np.float32).reshape(2, 3)             # the stub's rank-0 "action": loss = sum a^2, gradient 2 a
    for d in got:
        assert d["g_action"].dtype == np.float32 and np.array_equal(d["g_action"], 2 * a)
        assert d["loss"].dtype == np.float32 and d["loss"].tolist() == [55.0]
    assert all(np.array_equal(got[0][n], got[1][n]) for n in got[0])


def test_dump_outputs_keep_a_fixed_sample_within_the_budget(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(bench, "DUMP_BUDGET_B", 4000)
    arrays = {"a": torch.arange(3000.0).reshape(1000, 3), "b": torch.arange(500, dtype=torch.int32), "one": torch.tensor([1.0]),
              "wide": torch.ones(1, 2000, dtype=torch.float64)}
    for run in ("x", "y"):
        bench.dump_outputs(str(tmp_path / run), arrays)
    x = {n: np.load(tmp_path / "x" / (n + ".npy")) for n in arrays}
    y = {n: np.load(tmp_path / "y" / (n + ".npy")) for n in arrays}
    assert sum(v.nbytes for v in x.values()) <= 4000
    assert [x[n].dtype for n in ("a", "b", "one", "wide")] == [np.float32, np.float64, np.float32, np.float64]
    assert x["one"].tolist() == [1.0] and x["wide"].ndim == 1 and 0 < x["wide"].size < 2000
    rows = x["a"][:, 0] / 3                                      # row k of `a` starts with 3 k: the sample is rows, in order
    assert 0 < rows.size < 1000 and np.all(np.diff(rows) > 0) and np.array_equal(x["a"], np.arange(3000.0).reshape(1000, 3)[rows.astype(int)])
    assert all(np.array_equal(x[n], y[n]) for n in arrays)      # the same sample every time


def test_steps_below_one_are_refused():
    p = _stub(["--steps", "0"])
    assert p.returncode == 2 and "--steps must be at least 1" in p.stderr
