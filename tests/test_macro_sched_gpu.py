"""Time-varying boundary cells of the fused ARZ rollout on the GPU (dhts_macro_rollout_fwd_sched / _bwd_sched and dhts.macro_rollout with
[T][L][2] boundaries): every kernel family the plan can pick against the chained oracle (tests/macro_sched_ref.py) and the reference's
goldens, the constant schedule against the constant-boundary entry points bit for bit, lane independence and repeatability, and the
operator's interface.  Shapes are the smallest that reach each plan entry; every T <= 12 unless a golden fixes it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import macro_sched_ref as R
from util import TOL_GRAD, TOL_STATE, grad_report, meta_of, options, state_report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, DX, UM = 0.01, 5.0, 30.0
LANE, ONE_PHASE, PAIR = 0, 1, 2          # plan: fwd_kernel
GENERAL, FAST, FAST2 = 0, 1, 2           # plan: bwd_pipelined


# id: (L, N, T, want_hist, variant, group, forward kernel, lanes per workgroup, reverse kernel, its block)
CASES = {
    # pair kernel: lanes per workgroup 1, 2, 4 forced; odd and even T (the step body ping-pongs on n & 1), T = 1
    "pair128_g1": (4, 128, 1, False, 0, 1, PAIR, 1, FAST, 128),
    "pair128_g2": (4, 128, 2, False, 0, 2, PAIR, 2, FAST, 128),
    "pair128_g4": (4, 128, 5, False, 0, 4, PAIR, 4, FAST, 128),
    "pair256_g1": (4, 256, 12, False, 0, 1, PAIR, 1, FAST, 256),
    "pair256_g2": (4, 256, 7, False, 0, 2, PAIR, 2, FAST, 256),
    "pair256_g4": (4, 256, 4, False, 0, 4, PAIR, 4, FAST, 256),
    "pair512": (2, 512, 3, False, 0, 0, PAIR, 1, FAST, 512),
    # lane kernel, with and without the history
    "lane1": (3, 1, 6, False, 0, 0, LANE, 1, GENERAL, 64),
    "lane1_hist": (3, 1, 5, True, 0, 0, LANE, 1, GENERAL, 64),
    "lane2": (3, 2, 7, False, 0, 0, LANE, 1, FAST, 64),
    "lane2_hist": (3, 2, 2, True, 0, 0, LANE, 1, FAST, 64),
    "lane63": (2, 63, 9, False, 0, 0, LANE, 1, FAST, 64),
    "lane63_hist": (2, 63, 12, True, 0, 0, LANE, 1, FAST, 64),
    "lane64": (2, 64, 1, False, 0, 0, LANE, 1, FAST, 64),
    "lane64_hist": (2, 64, 8, True, 0, 0, LANE, 1, FAST, 64),
    "lane65": (2, 65, 10, False, 0, 0, LANE, 1, FAST, 128),
    "lane65_hist": (2, 65, 3, True, 0, 0, LANE, 1, FAST, 128),
    "lane130": (2, 130, 11, False, 0, 0, LANE, 1, FAST, 256),
    "lane130_hist": (2, 130, 4, True, 0, 0, LANE, 1, FAST, 256),
    "lane256_hist": (2, 256, 6, True, 0, 0, LANE, 1, FAST, 256),
    "lane1000": (1, 1000, 3, False, 0, 0, LANE, 1, FAST, 1024),
    "lane1026": (1, 1026, 3, False, 0, 0, LANE, 1, FAST2, 1024),
    "lane2048": (1, 2048, 4, False, 0, 0, LANE, 1, FAST2, 1024),
    # the run-time pass count (three passes on 11 wavefronts); the dense two-pass lane kernel with the pair kernel turned off; the
    # reverse sweep's 512- and 1024-thread blocks with per-step cotangents
    "lane2100": (1, 2100, 3, False, 0, 0, LANE, 1, GENERAL, 512),
    "lane2100_hist": (1, 2100, 3, True, 0, 0, LANE, 1, GENERAL, 512),
    "lane128_nopair": (2, 128, 5, False, 2, 0, LANE, 1, FAST, 128),
    "lane300_hist": (2, 300, 4, True, 0, 0, LANE, 1, FAST, 512),
    "lane1000_hist": (1, 1000, 3, True, 0, 0, LANE, 1, FAST, 1024),
    # one-phase kernel: forced, and where the plan picks it itself (the lane's records do not fit the two-phase kernels' LDS)
    "onephase65": (2, 65, 5, False, 1, 0, ONE_PHASE, 1, FAST, 128),
    "onephase65_hist": (2, 65, 4, True, 1, 0, ONE_PHASE, 1, FAST, 128),
    "onephase2500": (1, 2500, 3, False, 0, 0, ONE_PHASE, 1, GENERAL, 512),
    # T = 0: nothing to step, nothing to sweep
    "pair128_t0": (4, 128, 0, False, 0, 0, PAIR, None, GENERAL, None),
    "lane64_t0": (2, 64, 0, False, 0, 0, LANE, 1, GENERAL, None),
}


def check_plan(case):
    from dhts import ops
    L, N, T, hist, _, _, fwd, G, bwd, blk = CASES[case]
    plan = ops.macro_rollout_plan(ops.macro_desc(L, N, DT, DX, UM), T, want_hist=hist)
    assert plan["fwd_kernel"] == fwd, plan
    assert plan["bwd_pipelined"] == bwd, plan
    assert G is None or plan["fwd_lanes_per_group"] == G, plan
    assert blk is None or plan["bwd_block"] == blk, plan
    return plan


def inputs(case, seed=None):
    """Random state and independent random boundary cells per step; on some steps a boundary density below 1e-5 or exactly 0 (the
    solver's vacuum branches).  The T = 0 cases start with speeds in [0, 0.25]: with nothing stepped the final_sq tap's g_r0 is 2 r0
    plus cancelling float32 terms of size 2 u |u - u_eq| / r, and over the full speed range one ulp of the reference's own x ** -0.5
    moves it by more than TOL_GRAD (tests/test_macro_sched.py::test_why_the_t0_cases_of_the_gpu_tests_start_slow has the arithmetic)."""
    L, N, T = CASES[case][:3]
    rng = np.random.default_rng(sum(map(ord, case)) if seed is None else seed)
    r0 = rng.uniform(0.05, 0.95, (L, N)).astype(np.float32)
    u0 = rng.uniform(0.0, UM if T > 0 else 0.25, (L, N)).astype(np.float32)
    gr = rng.uniform(0.05, 0.95, (T, L, 2)).astype(np.float32)
    gu = rng.uniform(0.0, UM, (T, L, 2)).astype(np.float32)
    if T >= 2:
        gr[T // 2, 0, 0] = 3e-6
        gr[T - 1, L - 1, 1] = 0.0
        gr[0, 0, 1] = 8e-6
    return r0, u0, gr, gu


@pytest.mark.parametrize("case", sorted(CASES))
def test_device_against_the_chained_oracle(cuda, oracle, case):
    import torch
    import dhts
    L, N, T, hist, variant, group = CASES[case][:6]
    r0, u0, gr, gu = inputs(case)
    tap = "every_sum" if hist else "final_sq"
    f = R.sched_fwd(oracle, r0, u0, gr, gu, DT, DX, UM)
    b = R.sched_bwd(oracle, f, **R.taps(f, tap))
    leaves = [torch.tensor(a, device=cuda, requires_grad=True) for a in (r0, u0, gr, gu)]
    with options(variant, group):
        check_plan(case)
        out = dhts.macro_rollout(*leaves, T, DT, DX, UM, want_hist=hist)
        rT, yT, uT = out[:3]
        loss = (out[4][:, :, 0].sum() + out[4][:, :, 1].sum() + out[4][:, :, 2].sum()) if hist else (rT ** 2).sum() + (uT ** 2).sum()
        grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    for k, a in (("rT", rT), ("yT", yT), ("uT", uT)):
        assert state_report("%s %s" % (case, k), a.detach().cpu().numpy(), f[k]) <= TOL_STATE
    if hist and T > 0:
        for j, k in enumerate(("hist_r", "hist_y", "hist_u")):
            assert state_report("%s %s" % (case, k), out[4][:, :, j].detach().cpu().numpy(), f[k]) <= TOL_STATE
    assert tuple(grads[2].shape) == (T, L, 2) and tuple(grads[3].shape) == (T, L, 2)
    for k, g in zip(("g_r0", "g_u0", "g_ghost_r", "g_ghost_u"), grads):
        if b[k].size:
            assert grad_report("%s %s" % (case, k), g.cpu().numpy(), b[k]) <= TOL_GRAD


@pytest.mark.parametrize("name", ["pulse64", "sanity", "small"])
def test_device_against_the_reference(cuda, golden_dir, name):
    import torch
    import dhts
    g = np.load(os.path.join(golden_dir, "macro_sched_%s.npz" % name))
    m = meta_of(g)
    T, hist = m["T"], m["tap"] == "every_sum"
    leaves = [torch.tensor(a, device=cuda, requires_grad=True)
              for a in (g["r0"][None], g["u0"][None], g["ghost_r"][:, None], g["ghost_u"][:, None])]
    out = dhts.macro_rollout(*leaves, T, m["dt"], m["dx"], m["u_max"], want_hist=True)
    rT, yT, uT, h = out[0], out[1], out[2], out[4]
    loss = (h[:, :, 0].sum() + h[:, :, 1].sum() + h[:, :, 2].sum()) if hist else (rT ** 2).sum() + (uT ** 2).sum()
    loss.backward()
    for k, a in (("rT", rT), ("yT", yT), ("uT", uT)):
        assert state_report("%s %s" % (name, k), a.detach().cpu().numpy()[0], g[k]) <= TOL_STATE
    n = g["steps_r"].shape[0]
    for j, k in enumerate(("steps_r", "steps_y", "steps_u")):
        assert state_report("%s %s" % (name, k), h[:n, 0, j].detach().cpu().numpy(), g[k]) <= TOL_STATE
    assert abs(float(loss) - float(g["loss"])) <= TOL_STATE * abs(float(g["loss"]))
    assert grad_report("%s g_r0" % name, leaves[0].grad.cpu().numpy()[0], g["g_r0"]) <= TOL_GRAD
    assert grad_report("%s g_u0" % name, leaves[1].grad.cpu().numpy()[0], g["g_u0"]) <= TOL_GRAD
    assert grad_report("%s g_ghost_r" % name, leaves[2].grad.cpu().numpy()[:, 0], g["g_ghost_r"]) <= TOL_GRAD
    assert grad_report("%s g_ghost_u" % name, leaves[3].grad.cpu().numpy()[:, 0], g["g_ghost_u"]) <= TOL_GRAD


# ---- at the entry points ------------------------------------------------------------------------------------------------------------
def raw_run(cuda, case, ghost, sched, g_hist_seed=3):
    """One forward and one reverse launch at the C entry points.  ghost: [L][2][4] (sched = False) or [T][L][2][4].  The tape starts
    as zeros so that what no kernel writes (padding, the exception slots behind the count) compares equal."""
    import torch
    from dhts import ops
    L, N, T, hist = CASES[case][:4]
    r0, u0, _, _ = inputs(case)
    desc = ops.macro_desc(L, N, DT, DX, UM)
    r = torch.tensor(r0, device=cuda)
    u = torch.tensor(u0, device=cuda)
    y, q = ops.macro_state_from_ru(r, u, UM)
    tape = torch.zeros(ops.macro_tape_numel(desc, T), dtype=torch.float32, device=cuda)
    h = torch.zeros(T, L, 3, N, dtype=torch.float32, device=cuda) if hist else None
    err = ops.new_error_record(cuda)
    fwd = ops.macro_rollout_fwd_sched if sched else ops.macro_rollout_fwd
    state = fwd(desc, T, r, y, u, q, ghost, tape=tape, hist=h, err=err)
    rng = np.random.default_rng(g_hist_seed)
    g_r = torch.tensor(rng.standard_normal((L, N)).astype(np.float32), device=cuda)
    g_y = torch.tensor(rng.standard_normal((L, N)).astype(np.float32), device=cuda)
    gh = torch.tensor(rng.standard_normal((T, L, 2, N)).astype(np.float32), device=cuda) if hist else None
    bwd = ops.macro_rollout_bwd_sched if sched else ops.macro_rollout_bwd
    g_r0, g_y0, g_ghost = bwd(desc, T, tape, g_r, g_y, g_hist=gh, err=err)
    assert err.tolist()[0] == 0, err.tolist()
    blocks = ops.macro_tape_expand(desc, T, tape) if T > 0 else None
    return dict(state=[s.cpu().numpy() for s in state], hist=None if h is None else h.cpu().numpy(), tape=tape.cpu().numpy(),
                blocks=None if blocks is None else blocks.cpu().numpy(), g_r0=g_r0.cpu().numpy(), g_y0=g_y0.cpu().numpy(),
                g_ghost=g_ghost.cpu().numpy())


def ghost_quads(cuda, gr, gu):
    import torch
    from dhts import ops
    tr, tu = torch.tensor(gr, device=cuda), torch.tensor(gu, device=cuda)
    gy, gq = ops.macro_state_from_ru(tr, tu, UM)
    return torch.stack([tr, gy, tu, gq], dim=-1).contiguous()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# one shape per forward and per reverse kernel
CONSTANT = ["pair128_g2", "pair256_g4", "pair512", "lane1", "lane63", "lane65_hist", "lane256_hist", "lane1000", "lane1026", "lane2048",
            "onephase65", "onephase2500"]


@pytest.mark.parametrize("case", CONSTANT)
def test_constant_schedule_is_the_constant_boundary_path_bit_for_bit(cuda, case):
    L, N, T, hist, variant, group = CASES[case][:6]
    _, _, gr, gu = inputs(case)
    ghost = ghost_quads(cuda, gr[0], gu[0])                                  # [L][2][4]
    sched = ghost[None].repeat(T, 1, 1, 1).contiguous()
    with options(variant, group):
        plan = check_plan(case)
        a = raw_run(cuda, case, ghost, False)
        b = raw_run(cuda, case, sched, True)
    for k in range(4):
        assert same_bits(a["state"][k], b["state"][k]), "state plane %d" % k
    if hist:
        assert same_bits(a["hist"], b["hist"])
    # the tape as the reverse sweep reads it; the rows themselves where the order of a row's exception list is fixed (one wavefront
    # appends to a lane's queue, or the one-phase kernel's fixed slots) -- with several wavefronts it is the order their atomics land in
    assert same_bits(a["blocks"], b["blocks"])
    if plan["fwd_kernel"] == ONE_PHASE or plan["fwd_waves"] == 1:
        assert same_bits(a["tape"], b["tape"])
    assert same_bits(a["g_r0"], b["g_r0"]) and same_bits(a["g_y0"], b["g_y0"])
    assert b["g_ghost"].shape == (T, L, 2, 2) and b["g_ghost"].dtype == np.float64
    acc = np.zeros((L, 2, 2), np.float64)
    for t in range(T - 1, -1, -1):                                           # the sweep's order: newest step first
        acc = acc + b["g_ghost"][t]
    assert same_bits(acc, a["g_ghost"])
    # every addend is a float32 value
    assert same_bits(b["g_ghost"].astype(np.float32).astype(np.float64), b["g_ghost"])


@pytest.mark.parametrize("case", ["pair128_g4", "pair256_g2", "lane65_hist", "lane1026", "onephase65"])
def test_runs_repeat_and_lanes_do_not_see_their_neighbours(cuda, case):
    L, N, T, hist, variant, group = CASES[case][:6]
    _, _, gr, gu = inputs(case)
    with options(variant, group):
        check_plan(case)
        a = raw_run(cuda, case, ghost_quads(cuda, gr, gu), True)
        b = raw_run(cuda, case, ghost_quads(cuda, gr, gu), True)
        rng = np.random.default_rng(99)
        gr2, gu2 = rng.uniform(0.05, 0.95, gr.shape).astype(np.float32), rng.uniform(0.0, UM, gu.shape).astype(np.float32)
        keep = 1 if L > 1 else 0
        gr2[:, keep], gu2[:, keep] = gr[:, keep], gu[:, keep]                # every other lane gets another schedule
        c = raw_run(cuda, case, ghost_quads(cuda, gr2, gu2), True)
    for k in range(4):
        assert same_bits(a["state"][k], b["state"][k])
        assert same_bits(a["state"][k][keep], c["state"][k][keep])
    for k in ("g_r0", "g_y0"):
        assert same_bits(a[k], b[k]) and same_bits(a[k][keep], c[k][keep])
    assert same_bits(a["g_ghost"], b["g_ghost"]) and same_bits(a["g_ghost"][:, keep], c["g_ghost"][:, keep])
    assert same_bits(a["blocks"], b["blocks"]) and same_bits(a["blocks"][:, keep], c["blocks"][:, keep])
    if hist:
        assert same_bits(a["hist"], b["hist"]) and same_bits(a["hist"][:, keep], c["hist"][:, keep])
    if L > 1:
        other = 0 if keep else 1
        assert not same_bits(a["state"][0][other], c["state"][0][other])     # the changed schedules did arrive


def test_a_cfl_fault_names_step_lane_and_interface(cuda, oracle):
    """A downstream boundary speed far above dx / dt on one step of one lane: the record says which, and it is where the chained oracle's
    step fails.  (The downstream cell: a fast upstream cell against slower traffic gives a shock whose speeds pass the check, in the
    oracle too.  The last step: the first fault of a launch wins the record, and nothing can fault behind this one.)"""
    import torch
    from dhts import _lib, ops
    L, N, T = 4, 128, 6
    rng = np.random.default_rng(1)
    r0 = torch.tensor(rng.uniform(0.2, 0.8, (L, N)).astype(np.float32), device=cuda)
    u0 = torch.tensor(rng.uniform(5.0, 20.0, (L, N)).astype(np.float32), device=cuda)
    gr = np.full((T, L, 2), 0.5, np.float32)
    gu = np.full((T, L, 2), 10.0, np.float32)
    gu[T - 1, 2, 1] = 5000.0                                                  # step 5, lane 2, the downstream cell: interface N
    with pytest.raises(AssertionError, match=r"CFL check \(lane 2, step %d, interface %d\)" % (T - 1, N)):
        R.sched_fwd(oracle, r0.cpu().numpy(), u0.cpu().numpy(), gr, gu, DT, DX, UM)
    desc = ops.macro_desc(L, N, DT, DX, UM)
    y, q = ops.macro_state_from_ru(r0, u0, UM)
    err = ops.new_error_record(cuda)
    ops.macro_rollout_fwd_sched(desc, T, r0, y, u0, q, ghost_quads(cuda, gr, gu), err=err)
    assert err.tolist() == [_lib.FAULT_CFL, T - 1, 2, N]


# ---- through dhts.macro_rollout -------------------------------------------------------------------------------------------------------
def test_operator_shapes_errors_and_a_history_tap(cuda):
    import torch
    import dhts
    L, N, T = 3, 40, 9
    rng = np.random.default_rng(8)
    r0 = torch.tensor(rng.uniform(0.1, 0.9, (L, N)).astype(np.float32), device=cuda, requires_grad=True)
    u0 = torch.tensor(rng.uniform(0.0, UM, (L, N)).astype(np.float32), device=cuda, requires_grad=True)
    gr = torch.tensor(rng.uniform(0.1, 0.9, (T, L, 2)).astype(np.float32), device=cuda, requires_grad=True)
    gu = torch.tensor(rng.uniform(0.0, UM, (T, L, 2)).astype(np.float32), device=cuda, requires_grad=True)
    for bad_r, bad_u in ((gr, gu[0]), (gr[0], gu), (gr[:T - 1], gu[:T - 1]), (gr[:, :2], gu[:, :2]), (gr, gu[:T - 1])):
        with pytest.raises(ValueError):
            dhts.macro_rollout(r0, u0, bad_r, bad_u, T, DT, DX, UM)
    rT, yT, uT, qT, hist = dhts.macro_rollout(r0, u0, gr, gu, T, DT, DX, UM, want_hist=True)
    assert tuple(hist.shape) == (T, L, 3, N)
    # a tap on the density history at one cell: d / d boundary(t) has the schedule's shape, and the step-t boundary cannot reach a
    # state recorded before step t
    tap = hist[4, :, 0, 0].sum()
    g_gr, g_gu = torch.autograd.grad(tap, [gr, gu], retain_graph=True)
    assert tuple(g_gr.shape) == (T, L, 2) and tuple(g_gu.shape) == (T, L, 2)
    assert float(g_gr[5:].abs().sum()) == 0.0 and float(g_gu[5:].abs().sum()) == 0.0
    assert float(g_gr[:5, :, 0].abs().sum()) > 0.0                            # the upstream cells of the steps before do reach it
    grads = torch.autograd.grad((rT ** 2).sum() + (uT ** 2).sum(), [r0, u0, gr, gu])
    assert [tuple(g.shape) for g in grads] == [(L, N), (L, N), (T, L, 2), (T, L, 2)]
    # the constant form is untouched: [L][2] in, [L][2] out
    c_r, c_u = gr[0].detach().clone().requires_grad_(True), gu[0].detach().clone().requires_grad_(True)
    out = dhts.macro_rollout(r0, u0, c_r, c_u, T, DT, DX, UM)
    g2 = torch.autograd.grad((out[0] ** 2).sum(), [c_r, c_u])
    assert [tuple(g.shape) for g in g2] == [(L, 2), (L, 2)]
    # check_faults=False (what a HIP-graph capture asks for: no read-back) computes the same
    o1 = dhts.macro_rollout(r0, u0, gr, gu, T, DT, DX, UM, check_faults=False)
    g3 = torch.autograd.grad((o1[0] ** 2).sum() + (o1[2] ** 2).sum(), [r0, u0, gr, gu])
    assert torch.equal(o1[0], rT) and all(torch.equal(a, b) for a, b in zip(g3, grads))


def test_inflow_example_reduces_its_loss(cuda, tmp_path):
    """examples/estimate_inflow.py at 64 cells x 60 steps ends its iterations with a loss below the one it started from."""
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "estimate_inflow.py"), "--n_cell", "64", "--n_timestep", "60",
                          "--n_episode", "30", "--n_lane", "2", "--seed", "0"], cwd=str(tmp_path), env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    files = [os.path.join(dp, f) for dp, _, fs in os.walk(str(tmp_path)) for f in fs if f.startswith("trial_") and f.endswith(".txt")]
    assert files, "no trial_k.txt written"
    losses = [float(line.split()[-1]) for line in open(files[0]) if line.strip()]
    print("inflow loss: first %.6g, last %.6g over %d iterations" % (losses[0], losses[-1], len(losses)))
    assert len(losses) >= 30 and losses[0] > 0 and losses[-1] < losses[0]
