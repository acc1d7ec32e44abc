"""bench.py as the driver runs it: `python bench.py --gpus N` must start N ranks itself.

CPU part: the launcher fails loudly (non-zero, no JSON) when the ranks cannot run.  GPU part (`-m gpu`): two ranks on the
one leased GPU (collectives over gloo, because RCCL refuses two ranks on one device) -- the JSON line says n_gpus = 2, the
value counts both ranks' units, and the all-reduced [gradient || loss] buffer equals the sum of the two shards' buffers.
"""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def run_bench(args, timeout=900, env=None):
    e = dict(os.environ)
    e.pop("RANK", None), e.pop("WORLD_SIZE", None), e.pop("LOCAL_RANK", None)
    e.update(env or {})
    p = subprocess.run([sys.executable, BENCH] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout,
                       env=e, cwd=ROOT)
    return p


def last_json(text):
    lines = [l for l in text.splitlines() if l.startswith("{")]
    assert lines, "no JSON line in: %r" % text[-2000:]
    return json.loads(lines[-1])


def test_bench_has_no_undefined_globals():
    """A static pass over bench.py and the entry module (they only run on the GPU box): every global name a function
    body loads is defined at module level, imported, or a builtin."""
    import ast
    import builtins
    for path in (BENCH, os.path.join(ROOT, "__graft_entry__.py")):
        tree = ast.parse(open(path).read())
        defined = set(dir(builtins)) | {"__file__", "__name__"}
        for node in ast.walk(tree):
            if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
                defined.add(node.name)
                if isinstance(node, ast.FunctionDef):
                    defined.update(a.arg for a in node.args.args + node.args.kwonlyargs)
                    defined.update(a.arg for a in (node.args.vararg, node.args.kwarg) if a)
            elif isinstance(node, (ast.Import, ast.ImportFrom)):
                defined.update((a.asname or a.name).split(".")[0] for a in node.names)
            elif isinstance(node, ast.Name) and isinstance(node.ctx, (ast.Store, ast.Del)):
                defined.add(node.id)
            elif isinstance(node, ast.arg):
                defined.add(node.arg)
            elif isinstance(node, ast.ExceptHandler) and node.name:
                defined.add(node.name)
        missing = sorted({n.id for n in ast.walk(tree) if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Load)} - defined)
        assert not missing, "%s uses undefined names: %s" % (os.path.basename(path), missing)


def test_launcher_fails_loudly_without_gpus():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu tests")
    p = run_bench(["--gpus", "2", "--workload", "macro", "--lanes", "8", "--time-steps", "5", "--no-cpu-baseline"], timeout=300)
    assert p.returncode != 0
    assert "needs a GPU" in p.stderr and "rank(s) failed" in p.stderr
    assert not [l for l in p.stdout.splitlines() if l.startswith("{")]


@pytest.mark.gpu
def test_two_ranks_macro_lanes(cuda):
    one = run_bench(["--gpus", "1", "--workload", "macro", "--lanes", "64", "--time-steps", "50", "--steps", "3", "--warmup", "1",
                     "--no-cpu-baseline"])
    assert one.returncode == 0, one.stderr[-3000:]
    two = run_bench(["--gpus", "2", "--workload", "macro", "--lanes", "64", "--time-steps", "50", "--steps", "3", "--warmup", "1",
                     "--no-cpu-baseline"], env={"DHTS_DIST_BACKEND": "gloo"})
    assert two.returncode == 0, two.stderr[-3000:]
    a, b = last_json(one.stdout), last_json(two.stdout)
    assert a["n_gpus"] == 1 and b["n_gpus"] == 2 and b["scaling"] == "weak"
    assert b["config"]["lanes_per_gpu"] == 64
    # value = units of ALL ranks / max-over-ranks time: both ranks' 64 x 512 x 50 cell-steps per pass
    units = 64 * 512 * 50
    assert abs(b["value"] * b["ms_per_step"] * 1e-3 / (2 * units) - 1.0) < 1e-9
    assert abs(a["value"] * a["ms_per_step"] * 1e-3 / units - 1.0) < 1e-9
    chk = b["allreduce_check"]
    assert len(chk["rank_parts"]) == 2 and chk["rank_parts"][0] != chk["rank_parts"][1]      # different shards (seed + rank)
    assert abs(chk["reduced"] - chk["sum_of_rank_parts"]) <= 1e-6 * abs(chk["sum_of_rank_parts"])
    # rank 0 of the two-rank run owns the same lanes as the one-rank run: same loss
    assert chk["rank_parts"][0] == a["loss_last_pass"] and b["loss_last_pass"] == chk["reduced"]


@pytest.mark.gpu
def test_two_ranks_hybrid_replicas_shared_schedule(cuda):
    """BASELINE config 5's pattern: replicas sharded over ranks, d reward / d (shared signal schedule) + reward all-reduced."""
    two = run_bench(["--gpus", "2", "--workload", "itscp_hybrid", "--lanes", "8", "--steps", "2", "--warmup", "1",
                     "--no-cpu-baseline"], env={"DHTS_DIST_BACKEND": "gloo"})
    assert two.returncode == 0, two.stderr[-3000:]
    b = last_json(two.stdout)
    assert b["n_gpus"] == 2 and b["config"]["lanes_per_gpu"] == 8
    assert "replicas sharded over 2" in b["config"]["parallelism"]
    chk = b["allreduce_check"]
    assert abs(chk["reduced"] - chk["sum_of_rank_parts"]) <= 1e-6 * abs(chk["sum_of_rank_parts"])
    assert chk["grad_max_abs_diff"] <= 1e-6 * max(abs(x) for x in chk["rank_parts"])
    units = 8 * b["config"]["units_per_lane"] * b["config"]["time_steps"]
    assert abs(b["value"] * b["ms_per_step"] * 1e-3 / (2 * units) - 1.0) < 1e-9


@pytest.mark.gpu
def test_two_ranks_default_command_appends_config5(cuda):
    """What `bench.py --gpus N --full` adds for N > 1: behind the config-2 loop every rank runs the itscp hybrid network (here 8 replicas
    per rank instead of 256) with the all-reduce of [d reward / d action (45) || reward]; the line names the backend and every
    rank's device."""
    two = run_bench(["--gpus", "2", "--workload", "macro", "--lanes", "64", "--time-steps", "50", "--steps", "3", "--warmup", "1",
                     "--no-cpu-baseline", "--also-replicas", "8", "--full"], env={"DHTS_DIST_BACKEND": "gloo"})
    assert two.returncode == 0, two.stderr[-3000:]
    b = last_json(two.stdout)
    col = b["collective"]
    assert col["backend"] == "gloo" and col["world"] == 2 and len(col["devices"]) == 2
    assert all(d["name"] and d["device"].startswith("cuda:") for d in col["devices"])
    sec = b["also"][0]
    assert sec["n_gpus"] == 2 and "8 replicas per rank x 2 ranks = 16 replicas" in sec["config"]
    chk = sec["allreduce_check"]
    assert chk["buffer_floats"] == 46 and len(chk["rank_parts"]) == 2 and chk["rank_parts"][0] != chk["rank_parts"][1]
    assert abs(chk["reduced"] - chk["sum_of_rank_parts"]) <= 1e-6 * abs(chk["sum_of_rank_parts"])
    assert chk["grad_max_abs_diff"] <= 1e-6 * max(abs(x) for x in chk["rank_parts"])
    units = 8 * 256 * 600
    assert abs(sec["value"] * sec["ms_per_pass"] * 1e-3 / (2 * units) - 1.0) < 1e-9


@pytest.mark.gpu
def test_more_ranks_than_gpus_exits_nonzero_without_named_gloo(cuda):
    """Two ranks, one GPU, no DHTS_DIST_BACKEND: the run must fail instead of reporting a gloo number as if it were RCCL's."""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("needs fewer GPUs than ranks")
    e = {k: v for k, v in os.environ.items() if k != "DHTS_DIST_BACKEND"}
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--workload", "macro", "--lanes", "8", "--time-steps", "5", "--steps", "1",
                        "--warmup", "0", "--no-cpu-baseline"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600,
                       env={k: v for k, v in e.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}, cwd=ROOT)
    assert p.returncode != 0
    assert "refusing to fall back to gloo" in p.stderr
    assert not [l for l in p.stdout.splitlines() if l.startswith("{")]


RCCL_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.path.join(%(root)r, "diff-hybrid-traffic-sim_amd"))
import torch
import torch.distributed as dist
from dhts import dist as D
rank, world, local = D.init()
assert dist.is_initialized() and dist.get_backend() == "nccl" and world == 1
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
flat = torch.arange(46, dtype=torch.float32, device=dev)             # [d loss / d action (45) || loss]
ref = flat.clone()
D.allreduce_sum_(flat)
torch.cuda.synchronize()
assert torch.equal(flat, ref), "a one-rank sum must return the buffer"
big = torch.ones(1 << 20, dtype=torch.float32, device=dev)           # 4 MB: a ring-sized message, not only a latency-sized one
D.allreduce_sum_(big)
assert float(big.sum()) == float(1 << 20)
parts = D.gather_to_rank0(flat)
assert parts.shape == (1, 46) and torch.equal(parts[0], ref.cpu())
assert D.max_over_ranks(1.25, dev) == 1.25
D.barrier()
print(json.dumps({"backend": dist.get_backend(), "world": world, "ok": True}))
dist.destroy_process_group()
"""


@pytest.mark.gpu
def test_rccl_collectives_on_one_gpu(cuda):
    """RCCL itself, before the first multi-GPU run: a fresh child process initialises backend "nccl" (= RCCL on ROCm) with one
    rank (DHTS_DIST_FORCE=1 makes dhts.dist build the group and run its collectives at world size 1) and drives every helper
    bench.py uses -- all-reduce of a device buffer, max over ranks, gather, barrier."""
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29533",
               DHTS_DIST_FORCE="1", DHTS_DIST_BACKEND="nccl")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    p = subprocess.run([sys.executable, "-c", RCCL_CHILD % {"root": ROOT}], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    assert last_json(p.stdout) == {"backend": "nccl", "world": 1, "ok": True}


@pytest.mark.gpu
def test_bench_over_rccl_with_one_rank(cuda):
    """bench.py's whole measured loop with its per-pass all-reduce going through RCCL (one rank, DHTS_DIST_FORCE=1)."""
    p = run_bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--lanes", "64", "--time-steps", "50", "--no-cpu-baseline", "--no-also"],
                  env={"RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "1", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29534",
                       "DHTS_DIST_FORCE": "1", "DHTS_DIST_BACKEND": "nccl"})
    assert p.returncode == 0, p.stderr[-3000:]
    out = last_json(p.stdout)
    assert out["n_gpus"] == 1 and out["value"] > 0 and out["config"]["lanes_per_gpu"] == 64
    # the identity gather of the N > 1 line, over RCCL: backend by name, this rank's device with its PCI bus id and uuid
    col = out["collective"]
    assert col["backend"] == "nccl" and col["world"] == 1 and col["distinct_devices"] == 1
    d = col["devices"][0]
    assert d["rank"] == 0 and d["device"] == "cuda:0" and d["pci_bus_id"] and d["uuid"] and "gfx950" in d["arch"]
