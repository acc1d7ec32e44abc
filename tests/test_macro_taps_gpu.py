"""Detector taps of the fused ARZ rollout on the GPU (dhts_macro_rollout_fwd_taps / _bwd_taps and dhts.macro_rollout with `detectors`):
every kernel family the taps plan can pick, with constant boundary cells and with a schedule, against the history path (same leaves,
the loss on hist[:, :, :, det]) and against the oracle; the raw operators (every element written, nothing beside them, repeatable,
lanes independent, an index outside the lane skipped); the plan; the fault record; the example.  Shapes are the smallest that reach
each plan entry and each wavefront boundary; every T <= 12."""
import os
import subprocess
import sys

import numpy as np
import pytest

import macro_sched_ref as R
from util import TOL_GRAD, TOL_STATE, grad_report, options, state_report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, DX, UM = 0.01, 5.0, 30.0
LANE, ONE_PHASE, PAIR = 0, 1, 2          # plan: fwd_kernel
GENERAL, FAST, FAST2 = 0, 1, 2           # plan: bwd_pipelined


# id: (L, N, T, variant, group, detectors, forward kernel, lanes per workgroup, reverse kernel of the taps plan, its block)
# Detector sets: cell 0 and cell N - 1; both sides of every wavefront boundary (63 / 64, 127 / 128; N / 2 - 1 / N / 2 for the pair
# kernel); the two cells of one pair-kernel thread (2m, 2m + 1); D = 1; D = N for N <= 65; more than 64 entries at N = 256.
CASES = {
    # pair kernel: lanes per workgroup 1, 2, 4 forced; odd and even T, T = 1
    "pair128_g1": (4, 128, 1, 0, 1, [0, 63, 64, 127], PAIR, 1, FAST, 128),
    "pair128_g2": (4, 128, 2, 0, 2, [5], PAIR, 2, FAST, 128),
    "pair128_g4": (4, 128, 5, 0, 4, [0, 1, 62, 63, 64, 65, 126, 127], PAIR, 4, FAST, 128),
    "pair256_g1": (4, 256, 12, 0, 1, list(range(0, 256, 3)), PAIR, 1, FAST, 256),                  # 86 detectors
    "pair256_g2": (4, 256, 7, 0, 2, [63, 64, 127, 128, 191, 192, 255], PAIR, 2, FAST, 256),
    "pair256_g4": (4, 256, 4, 0, 4, [0, 127, 128, 254, 255], PAIR, 4, FAST, 256),
    "pair512": (2, 512, 3, 0, 0, [0, 63, 64, 127, 128, 255, 256, 510, 511], PAIR, 1, FAST, 512),
    # lane kernel
    "lane1": (3, 1, 6, 0, 0, [0], LANE, 1, GENERAL, 64),
    "lane2": (3, 2, 7, 0, 0, [0, 1], LANE, 1, FAST, 64),
    "lane63": (2, 63, 9, 0, 0, list(range(63)), LANE, 1, FAST, 64),
    "lane64": (2, 64, 1, 0, 0, list(range(64)), LANE, 1, FAST, 64),
    "lane65": (2, 65, 10, 0, 0, list(range(65)), LANE, 1, FAST, 128),
    "lane130": (2, 130, 11, 0, 0, [0, 63, 64, 65, 127, 128, 129], LANE, 1, FAST, 256),
    "lane1000": (1, 1000, 3, 0, 0, [0, 63, 64, 127, 128, 500, 999], LANE, 1, FAST, 1024),
    # 1026 .. 2048 cells: the taps plan takes the general reverse sweep (include/dhts.h), as the history does
    "lane1026": (1, 1026, 3, 0, 0, [0, 63, 64, 1023, 1024, 1025], LANE, 1, GENERAL, 512),
    "lane2048": (1, 2048, 4, 0, 0, [0, 127, 128, 1024, 2047], LANE, 1, GENERAL, 512),
    # the run-time pass count (three passes on 11 wavefronts); the dense two-pass lane kernel with the pair kernel turned off; the
    # reverse sweep's 512-thread block on a lane shorter than it
    "lane2100": (1, 2100, 3, 0, 0, [0, 63, 64, 1023, 1024, 2099], LANE, 1, GENERAL, 512),
    "lane128_nopair": (2, 128, 5, 2, 0, [0, 63, 64, 127], LANE, 1, FAST, 128),
    "lane300": (2, 300, 4, 0, 0, [0, 149, 150, 299], LANE, 1, FAST, 512),
    # one-phase kernel: forced, and where the plan picks it itself
    "onephase65": (2, 65, 5, 1, 0, list(range(65)), ONE_PHASE, 1, FAST, 128),
    "onephase2500": (1, 2500, 3, 0, 0, [0, 63, 64, 2499], ONE_PHASE, 1, GENERAL, 512),
    # T = 0: nothing to step, nothing to sweep, no row of readings
    "pair128_t0": (4, 128, 0, 0, 0, [0, 127], PAIR, None, GENERAL, None),
    "lane64_t0": (2, 64, 0, 0, 0, [3], LANE, 1, GENERAL, None),
}
BOTH = [False, True]                     # constant boundary cells / a schedule


def check_plan(case):
    """The taps plan is the plan of the same shape without a history; bwd_pipelined too, except at 1026 .. 2048 cells."""
    from dhts import ops
    L, N, T, _, _, det, fwd, G, bwd, blk = CASES[case]
    desc = ops.macro_desc(L, N, DT, DX, UM)
    plan, plain = ops.macro_taps_plan(desc, T, len(det)), ops.macro_rollout_plan(desc, T, want_hist=False)
    for k in ("fwd_kernel", "fwd_lanes_per_group", "fwd_waves", "fwd_passes", "fwd_full_lane"):
        assert plan[k] == plain[k], (k, plan, plain)
    if 1026 <= N <= 2048 and T > 0:
        assert plain["bwd_pipelined"] == FAST2 and plan["bwd_pipelined"] == GENERAL
        assert plan["bwd_block"] == ops.macro_rollout_plan(desc, T, want_hist=True)["bwd_block"]
    else:
        assert plan["bwd_pipelined"] == plain["bwd_pipelined"] and plan["bwd_block"] == plain["bwd_block"], (plan, plain)
    assert plan["fwd_kernel"] == fwd, plan
    assert plan["bwd_pipelined"] == bwd, plan
    assert G is None or plan["fwd_lanes_per_group"] == G, plan
    assert blk is None or plan["bwd_block"] == blk, plan
    return plan


def inputs(case, sched):
    """tests/test_macro_sched_gpu.py's recipe: random state and independent random boundary cells per step, on some steps a boundary
    density below 1e-5 or exactly 0 (the solver's vacuum branches); the T = 0 cases start slow (see there).  Constant boundaries: one
    more row drawn behind the schedule."""
    L, N, T = CASES[case][:3]
    rng = np.random.default_rng(sum(map(ord, case)))
    r0 = rng.uniform(0.05, 0.95, (L, N)).astype(np.float32)
    u0 = rng.uniform(0.0, UM if T > 0 else 0.25, (L, N)).astype(np.float32)
    gr = rng.uniform(0.05, 0.95, (T, L, 2)).astype(np.float32)
    gu = rng.uniform(0.0, UM, (T, L, 2)).astype(np.float32)
    if T >= 2:
        gr[T // 2, 0, 0] = 3e-6
        gr[T - 1, L - 1, 1] = 0.0
        gr[0, 0, 1] = 8e-6
    cr = rng.uniform(0.05, 0.95, (L, 2)).astype(np.float32)
    cu = rng.uniform(0.0, UM, (L, 2)).astype(np.float32)
    return (r0, u0, gr, gu) if sched else (r0, u0, cr, cu)


def weights(case):
    """The loss: sum of w * (r, y, u) at the detectors after every step, plus wf * (rT, uT)."""
    L, N, T = CASES[case][:3]
    rng = np.random.default_rng(1000 + sum(map(ord, case)))
    return rng.standard_normal((T, L, 3, len(CASES[case][5]))).astype(np.float32), rng.standard_normal((2, L, N)).astype(np.float32)


_both_paths = {}


def both_paths(cuda, case, sched):
    """The same leaves through want_hist=True (the loss on hist[:, :, :, det]) and through detectors=det; computed once per case."""
    import torch
    import dhts
    key = (case, sched)
    if key not in _both_paths:
        L, N, T, variant, group, det = CASES[case][:6]
        w, wf = (torch.tensor(a, device=cuda) for a in weights(case))
        idx = torch.tensor(det, device=cuda)
        res = {}
        with options(variant, group):
            check_plan(case)
            for path in ("hist", "taps"):
                leaves = [torch.tensor(a, device=cuda, requires_grad=True) for a in inputs(case, sched)]
                if path == "hist":
                    out = dhts.macro_rollout(*leaves, T, DT, DX, UM, want_hist=True)
                    read = out[4][:, :, :, idx]
                else:
                    out = dhts.macro_rollout(*leaves, T, DT, DX, UM, detectors=det)
                    read = out[4]
                assert tuple(read.shape) == (T, L, 3, len(det))
                loss = (read * w).sum() + (out[0] * wf[0]).sum() + (out[2] * wf[1]).sum()
                grads = torch.autograd.grad(loss, leaves, allow_unused=True)
                res[path] = dict(state=[o.detach() for o in out[:3]], read=read.detach(), grads=grads)
        _both_paths[key] = res
    return _both_paths[key]


@pytest.mark.parametrize("sched", BOTH, ids=["const", "sched"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_detectors_equal_the_history_path(cuda, case, sched):
    """States and readings bit for bit.  Gradients bit for bit wherever both paths run the same forward and reverse kernel family --
    every lane and one-phase case, the 1026 .. 2048 range included (both take the general sweep there) --; within TOL_GRAD for the pair
    shapes, where the history takes the lane kernel forward and the detectors stay on the pair kernel (the exception lists of the
    tape come in another order).  Nothing is skipped."""
    import torch
    from dhts import ops
    L, N, T = CASES[case][:3]
    res = both_paths(cuda, case, sched)
    h, t = res["hist"], res["taps"]
    for k in range(3):
        assert torch.equal(h["state"][k], t["state"][k]), "state plane %d" % k
    assert torch.equal(h["read"], t["read"])
    desc = ops.macro_desc(L, N, DT, DX, UM)
    same_kernels = CASES[case][6] != PAIR
    assert ops.macro_rollout_plan(desc, T, want_hist=True)["bwd_pipelined"] == CASES[case][8]        # the same reverse kernel family
    for name, a, b in zip(("g_r0", "g_u0", "g_ghost_r", "g_ghost_u"), h["grads"], t["grads"]):
        assert (a is None) == (b is None)
        if a is None or not a.numel():
            assert a is None or a.shape == b.shape
            continue
        assert a.shape == b.shape
        equal = torch.equal(a, b)
        print("%s %s %s: %s" % (case, "sched" if sched else "const", name, "equal" if equal else "not bit-equal"))
        if same_kernels:
            assert equal, name
        else:
            assert grad_report("%s %s" % (case, name), b.cpu().numpy(), a.cpu().numpy()) <= TOL_GRAD


@pytest.mark.parametrize("sched", BOTH, ids=["const", "sched"])
@pytest.mark.parametrize("case", ["pair256_g2", "lane65", "lane1026", "onephase65"])
def test_detectors_against_the_oracle(cuda, oracle, case, sched):
    """One case per kernel family: the oracle's history gathered at det, and its reverse sweep with the weights scattered to det."""
    L, N, T, _, _, det = CASES[case][:6]
    r0, u0, gr, gu = inputs(case, sched)
    w, wf = weights(case)
    gh = np.zeros((3, T, L, N), np.float32)
    gh[:, :, :, det] = w.transpose(2, 0, 1, 3)
    if sched:
        f = R.sched_fwd(oracle, r0, u0, gr, gu, DT, DX, UM)
        b = R.sched_bwd(oracle, f, g_rT=wf[0], g_uT=wf[1], gh_r=gh[0], gh_y=gh[1], gh_u=gh[2])
    else:
        f = oracle.macro_rollout_fwd(r0, u0, gr, gu, T, DT, DX, UM, want_hist=True)
        b = oracle.macro_rollout_bwd(f, g_rT=wf[0], g_uT=wf[1], gh_r=gh[0], gh_y=gh[1], gh_u=gh[2])
    t = both_paths(cuda, case, sched)["taps"]
    for j, k in enumerate(("rT", "yT", "uT")):
        assert state_report("%s %s" % (case, k), t["state"][j].cpu().numpy(), f[k]) <= TOL_STATE
    read = t["read"].cpu().numpy()
    for j, k in enumerate(("hist_r", "hist_y", "hist_u")):
        assert state_report("%s readings of %s" % (case, k), read[:, :, j], f[k][:, :, det]) <= TOL_STATE
    for k, g in zip(("g_r0", "g_u0", "g_ghost_r", "g_ghost_u"), t["grads"]):
        assert grad_report("%s %s" % (case, k), g.cpu().numpy(), b[k]) <= TOL_GRAD


# ---- at the entry points ------------------------------------------------------------------------------------------------------------
def ghost_quads(cuda, gr, gu):
    import torch
    from dhts import ops
    tr, tu = torch.tensor(gr, device=cuda), torch.tensor(gu, device=cuda)
    gy, gq = ops.macro_state_from_ru(tr, tu, UM)
    return torch.stack([tr, gy, tu, gq], dim=-1).contiguous()


GUARD, SENTINEL = 257, 12345.0


def raw_run(cuda, case, sched, lanes=None, det=None, poison=()):
    """One forward and one reverse launch at the raw operators, on all lanes or on the lanes `lanes` alone.  The readings go into the
    middle of a larger buffer: NaN where they belong, a sentinel on both sides.  poison: columns of g_taps that hold NaN."""
    import torch
    from dhts import ops
    L, N, T = CASES[case][:3]
    det = CASES[case][5] if det is None else det
    D = len(det)
    r0, u0, gr, gu = inputs(case, sched)
    rng = np.random.default_rng(7)
    g_r, g_y = rng.standard_normal((2, L, N)).astype(np.float32)
    g_t = rng.standard_normal((T, L, 2, D)).astype(np.float32)
    g_t[..., list(poison)] = np.nan
    if lanes is not None:
        r0, u0, g_r, g_y, g_t = r0[lanes], u0[lanes], g_r[lanes], g_y[lanes], g_t[:, lanes]
        gr, gu = (gr[:, lanes], gu[:, lanes]) if sched else (gr[lanes], gu[lanes])
        L = len(lanes)
    desc = ops.macro_desc(L, N, DT, DX, UM)
    r, u = torch.tensor(r0, device=cuda), torch.tensor(u0, device=cuda)
    y, q = ops.macro_state_from_ru(r, u, UM)
    tape = torch.zeros(ops.macro_tape_numel(desc, T), dtype=torch.float32, device=cuda)
    n = T * L * 3 * D
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=cuda)
    taps = buf[GUARD:GUARD + n].view(T, L, 3, D)
    taps.fill_(float("nan"))
    err = ops.new_error_record(cuda)
    dt = torch.tensor(det, dtype=torch.int32, device=cuda)
    state, taps_out = ops.macro_rollout_fwd_taps(desc, T, r, y, u, q, ghost_quads(cuda, gr, gu), dt, tape=tape, err=err, taps=taps)
    assert taps_out.data_ptr() == taps.data_ptr()
    g_r0, g_y0, g_ghost = ops.macro_rollout_bwd_taps(desc, T, tape, torch.tensor(g_r, device=cuda), torch.tensor(g_y, device=cuda), dt,
                                                     torch.tensor(g_t, device=cuda), sched=sched, err=err)
    assert err.tolist()[0] == 0, err.tolist()
    assert tuple(g_ghost.shape) == ((T, L, 2, 2) if sched else (L, 2, 2))
    b = buf.cpu().numpy()
    assert np.all(b[:GUARD] == SENTINEL) and np.all(b[GUARD + n:] == SENTINEL), "a store beside the readings"
    return dict(state=[s.cpu().numpy() for s in state], taps=taps.cpu().numpy(), g_r0=g_r0.cpu().numpy(), g_y0=g_y0.cpu().numpy(),
                g_ghost=g_ghost.cpu().numpy())


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("sched", BOTH, ids=["const", "sched"])
@pytest.mark.parametrize("case", ["pair128_g4", "pair256_g1", "pair512", "lane65", "lane130", "lane1026", "onephase65", "onephase2500"])
def test_raw_operators_write_every_reading_repeat_and_keep_lanes_apart(cuda, case, sched):
    L, N, T, variant, group = CASES[case][:5]
    keep = L - 1
    with options(variant, group):
        check_plan(case)
        a = raw_run(cuda, case, sched)
        b = raw_run(cuda, case, sched)
        c = raw_run(cuda, case, sched, lanes=[keep])
    assert not np.isnan(a["taps"]).any(), "%d readings were not written" % int(np.isnan(a["taps"]).sum())
    for k in range(4):
        assert same_bits(a["state"][k], b["state"][k]) and same_bits(a["state"][k][keep:keep + 1], c["state"][k])
    assert same_bits(a["taps"], b["taps"]) and same_bits(a["taps"][:, keep:keep + 1], c["taps"])
    for k in ("g_r0", "g_y0"):
        assert same_bits(a[k], b[k]) and same_bits(a[k][keep:keep + 1], c[k])
    assert same_bits(a["g_ghost"], b["g_ghost"])
    assert same_bits(a["g_ghost"][:, keep:keep + 1] if sched else a["g_ghost"][keep:keep + 1], c["g_ghost"])


@pytest.mark.parametrize("case", ["pair128_g2", "lane65", "lane1026", "onephase65"])
def test_an_index_outside_the_lane_matches_no_cell(cuda, case):
    """The raw operators do not look at det (include/dhts.h, index contract): an entry outside [0, N) is compared away before any
    address is formed from it -- its column of the readings stays as it was, its column of g_taps is not read -- and the columns
    beside it are those of a run without it."""
    L, N, T, variant, group = CASES[case][:5]
    with options(variant, group):
        good = raw_run(cuda, case, True, det=[2, N - 1])
        a = raw_run(cuda, case, True, det=[2, N - 1, N, N + 70000, -5], poison=(2, 3, 4))
    assert same_bits(a["taps"][..., :2], good["taps"])
    assert np.isnan(a["taps"][..., 2:]).all()                                # not written
    # the three columns of g_taps behind them hold NaN: read, they would reach every gradient
    assert np.isfinite(a["g_r0"]).all() and np.isfinite(a["g_y0"]).all() and np.isfinite(a["g_ghost"]).all()


def test_a_cfl_fault_names_the_same_step_lane_and_interface_as_the_plain_rollout(cuda):
    """tests/test_macro_sched_gpu.py's recipe: a downstream boundary speed far above dx / dt on the last step of lane 2."""
    import torch
    from dhts import _lib, ops
    L, N, T = 4, 128, 6
    rng = np.random.default_rng(1)
    r0 = torch.tensor(rng.uniform(0.2, 0.8, (L, N)).astype(np.float32), device=cuda)
    u0 = torch.tensor(rng.uniform(5.0, 20.0, (L, N)).astype(np.float32), device=cuda)
    gr = np.full((T, L, 2), 0.5, np.float32)
    gu = np.full((T, L, 2), 10.0, np.float32)
    gu[T - 1, 2, 1] = 5000.0                                                  # step 5, lane 2, the downstream cell: interface N
    desc = ops.macro_desc(L, N, DT, DX, UM)
    y, q = ops.macro_state_from_ru(r0, u0, UM)
    det = torch.tensor([0, 64, 127], dtype=torch.int32, device=cuda)
    plain, taps = ops.new_error_record(cuda), ops.new_error_record(cuda)
    ops.macro_rollout_fwd_sched(desc, T, r0, y, u0, q, ghost_quads(cuda, gr, gu), err=plain)
    ops.macro_rollout_fwd_taps(desc, T, r0, y, u0, q, ghost_quads(cuda, gr, gu), det, err=taps)
    assert plain.tolist() == [_lib.FAULT_CFL, T - 1, 2, N]
    assert taps.tolist() == plain.tolist()


# ---- through dhts.macro_rollout -------------------------------------------------------------------------------------------------------
def test_a_cuda_tensor_of_detectors_gives_what_the_list_gives(cuda):
    import torch
    import dhts
    case = "lane130"
    L, N, T, _, _, det = CASES[case][:6]
    res = []
    for d in (det, torch.tensor(det, dtype=torch.int32, device=cuda), torch.tensor(det), np.array(det).tolist()):
        leaves = [torch.tensor(a, device=cuda, requires_grad=True) for a in inputs(case, True)]
        out = dhts.macro_rollout(*leaves, T, DT, DX, UM, detectors=d, check_faults=False)
        assert len(out) == 5 and tuple(out[4].shape) == (T, L, 3, len(det))
        res.append((out, torch.autograd.grad((out[4] ** 2).sum() + out[0].sum(), leaves)))
    for out, grads in res[1:]:
        assert all(torch.equal(a, b) for a, b in zip(out, res[0][0]))
        assert all(torch.equal(a, b) for a, b in zip(grads, res[0][1]))
    # a loss that does not look at the readings, and no gradient at all
    leaves = [torch.tensor(a, device=cuda, requires_grad=True) for a in inputs(case, False)]
    out = dhts.macro_rollout(*leaves, T, DT, DX, UM, detectors=det)
    ref = dhts.macro_rollout(*leaves, T, DT, DX, UM)
    g1 = torch.autograd.grad((out[0] ** 2).sum(), leaves)
    g2 = torch.autograd.grad((ref[0] ** 2).sum(), leaves)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
    with torch.no_grad():
        out = dhts.macro_rollout(*[x.detach() for x in leaves], T, DT, DX, UM, detectors=det)
    assert torch.equal(out[0], ref[0]) and not out[4].requires_grad


def run_example(tmp_path, readings):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    cwd = os.path.join(str(tmp_path), readings)
    os.makedirs(cwd)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "estimate_inflow.py"), "--n_cell", "64", "--n_timestep", "60",
                          "--n_episode", "8", "--seed", "1", "--readings", readings], cwd=cwd, env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    files = [os.path.join(dp, f) for dp, _, fs in os.walk(cwd) for f in fs if f == "trial_0.txt"]
    assert len(files) == 1, files
    return open(files[0]).read()


def test_inflow_example_logs_the_same_lines_with_detectors_and_with_the_history(cuda, tmp_path):
    det, hist = run_example(tmp_path, "detectors"), run_example(tmp_path, "history")
    assert det == hist
    losses = [float(line.split()[-1]) for line in det.splitlines() if line.strip()]
    print("inflow loss: first %.6g, last %.6g over %d iterations" % (losses[0], losses[-1], len(losses)))
    assert len(losses) == 8 and losses[0] > 0 and losses[-1] < losses[0]
