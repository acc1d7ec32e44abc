"""Gradient of the fused IDM rollout with respect to the driver parameters, on the device: dhts.micro_rollout with
params.requires_grad against the reference's goldens (tests/golden/micro_params_*.npz) and against the float64 restatement of
tests/test_micro_params.py (validated there against the goldens and the oracle).  Needs a real MI355X: python -m pytest tests -m gpu"""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_micro_params import GOLDENS, golden_case, per_plane, restated
from util import TOL_GRAD, TOL_STATE, grad_report, rel_elem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = np.array([30.0, 24.0, 27.0, 0.5, 0.1, 5.0])          # MicroVehicle.default_micro_vehicle(30), micro_vehicle.py:31-72


def lanes(rng, L, V, sl=30.0, random_params=True):
    """Collision-free lanes by construction: the spacing / jitter of tools/gen_goldens.py micro_rollout (20 m + U[0, 10), speeds in
    [0.3, 0.7] of the speed limit), per-vehicle parameters drawn like its `random` branch."""
    p0 = (np.arange(V)[None, :] * 20.0 + rng.uniform(0, 10, (L, V))).astype(np.float32)
    v0 = rng.uniform(0.3 * sl, 0.7 * sl, (L, V)).astype(np.float32)
    par = np.tile(DEFAULT[:, None, None], (1, L, V))
    if random_params:
        par[0] = sl * rng.uniform(0.8, 1.5, (L, V))
        par[1] = sl * rng.uniform(0.6, 1.5, (L, V))
        par[2] = sl * rng.uniform(0.8, 1.2, (L, V))
        par[3] = 5.0 * rng.uniform(0.1, 1.0, (L, V))
        par[4] = rng.uniform(0.1, 1.5, (L, V))
    head = np.tile(np.array([[1000.0, 0.0]]), (L, 1))
    return p0, v0, par, head


def device_run(cuda, p0, v0, par, head, T, dt, tap, count=None, want_params=True, g_pT=None, g_vT=None, g_hist=None, params_t=None):
    """dhts.micro_rollout + backward of `tap` (or of the given cotangents) -> dict of numpy arrays."""
    import torch
    import dhts
    tp0 = torch.tensor(p0, device=cuda, requires_grad=True)
    tv0 = torch.tensor(v0, device=cuda, requires_grad=True)
    tpar = params_t if params_t is not None else torch.tensor(par, device=cuda, dtype=torch.float64, requires_grad=want_params)
    thead = torch.tensor(head, device=cuda, dtype=torch.float64, requires_grad=True)
    cnt = None if count is None else torch.tensor(count, device=cuda, dtype=torch.int32)
    want_hist = tap == "every_sum" or g_hist is not None
    out = dhts.micro_rollout(tp0, tv0, tpar, thead, T, dt, count=cnt, want_hist=want_hist)
    pT, vT = out[0], out[1]
    if tap is None:
        loss = (pT * torch.tensor(g_pT, device=cuda)).sum() + (vT * torch.tensor(g_vT, device=cuda)).sum()
        if g_hist is not None:
            loss = loss + (out[2] * torch.tensor(g_hist, device=cuda)).sum()
    else:
        loss = out[2].sum() if tap == "every_sum" else 1e-4 * (pT ** 2).sum() + (vT ** 2).sum()
    loss.backward()
    torch.cuda.synchronize()
    n = lambda t: None if t is None else t.detach().cpu().numpy()      # noqa: E731
    return dict(pT=n(pT), vT=n(vT), hist=n(out[2]) if want_hist else None, g_p0=n(tp0.grad), g_v0=n(tv0.grad), g_head=n(thead.grad),
                g_params=n(tpar.grad) if params_t is None else None)


# =================================================================================================================
# known-answer partials
# =================================================================================================================
def kat_operands(n=4096, seed=11):
    """a_max a_pref v v_target dp dv min_space time_pref dt: free road, car following, operands under the spacing clip (the leader
    much faster), under the acceleration clip (a gap far below the optimal spacing) and gaps the lane replaces by a constant (collided,
    zero, below POSITION_DELTA_EPS)."""
    rng = np.random.default_rng(seed)
    inp = np.stack([rng.uniform(16, 45, n), rng.uniform(12, 45, n), rng.uniform(0.5, 30, n), rng.uniform(16, 36, n),
                    rng.uniform(5, 200, n), rng.uniform(-5, 5, n), rng.uniform(0.5, 5, n), rng.uniform(0.1, 1.5, n),
                    rng.choice([0.01, 1.0 / 30.0, 0.1], n)], 1)
    q = n // 8
    inp[q:2 * q, 5] = -rng.uniform(30, 80, q)                      # spacing clip
    inp[2 * q:3 * q, 4] = rng.uniform(0.01, 0.5, q)                # acceleration clip
    inp[3 * q:3 * q + 40, 4] = -rng.uniform(0.1, 3, 40)            # collided: both deltas become the constant 0
    inp[3 * q + 40:3 * q + 80, 4] = rng.uniform(0, 9e-6, 40)       # below the clamp
    inp[3 * q + 80, 4] = 0.0
    return inp


def kat_reference(inp):
    """float64 autograd of IDM.compute_acceleration's formula (model/micro/_idm.py:30-49) under the lane's collision rule and clamp
    (_micro_lane.py:151-166) -> d acc / d (a_max, a_pref, v_target, min_space, time_pref, gap) [n][6], the two clip flags."""
    import torch
    x = torch.tensor(inp, dtype=torch.float64)
    a, b, vt, s0, tp, gap = (x[:, k].clone().requires_grad_(True) for k in (0, 1, 3, 6, 7, 4))
    v, dv, dt = x[:, 2], x[:, 5], x[:, 8]
    zero, eps = torch.zeros_like(v), torch.full_like(v, 1e-5)
    hit = gap < 0
    g, d = torch.where(hit, zero, gap), torch.where(hit, zero, dv)
    g = torch.where(eps > g, eps, g)
    s = s0 + v * tp + (v * d) / (2 * (a * b) ** 0.5)
    cs = s < 0
    s = torch.where(cs, zero, s)
    acc = a * (1.0 - (v / vt) ** 4 - (s / g) ** 2)
    ca = acc < -v / dt
    acc = torch.where(ca, -v / dt, acc)
    acc.sum().backward()
    return torch.stack([t.grad for t in (a, b, vt, s0, tp, gap)], 1).numpy(), ca.numpy(), cs.numpy()


def test_param_partials_known_answer(cuda):
    """dhts_idm_param_jac_batch -- the function the reverse sweep calls -- against float64 autograd: relative 1e-12, entry by entry
    (double in, double out); entries the reference has as exact zeros (clips, constant gaps) are exact zeros."""
    import torch
    from dhts import ops
    inp = kat_operands()
    ref, ca, cs = kat_reference(inp)
    assert ca.sum() > 100 and cs.sum() > 100 and (~ca & ~cs).sum() > 1000 and (inp[:, 4] < 1e-5).sum() > 80
    dev, dca, dcs = ops.idm_param_jac_batch(torch.tensor(inp, device=cuda))
    dev, dca, dcs = dev.cpu().numpy(), dca.cpu().numpy(), dcs.cpu().numpy()
    assert np.array_equal(dca, ca) and np.array_equal(dcs, cs)
    assert np.all(dev[ref == 0] == 0)
    assert np.all(dev[inp[:, 4] < 1e-5, 5] == 0) and np.all(dev[ca] == 0)
    nz = ref != 0
    err = np.abs(dev[nz] - ref[nz]) / np.abs(ref[nz])
    print("parameter partials vs float64 autograd over %d operand sets: relative p50 / p99 / max = %.1e %.1e %.1e"
          % (len(inp), np.percentile(err, 50), np.percentile(err, 99), err.max()))
    assert err.max() <= 1e-12


# =================================================================================================================
# the rollout
# =================================================================================================================
@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_as_lanes_of_one_launch(cuda, golden_dir, name):
    """The golden as lane 2 of a ragged launch: lane 0 = its last vehicles only (a shorter lane), lane 1 = empty, lane 3 = the same
    lane with other drivers.  Lane 2 against the reference's numbers, all lanes against the restatement, per parameter plane."""
    c = golden_case(golden_dir, name)
    g, T, dt, tap = c["g"], c["T"], c["dt"], c["tap"]
    V = c["p0"].shape[1]
    k = V - 3
    p0, v0 = np.tile(c["p0"], (4, 1)), np.tile(c["v0"], (4, 1))
    par, head = np.tile(c["params"], (1, 4, 1)), np.tile(c["head"], (4, 1))
    p0[0, :k], v0[0, :k], par[:, 0, :k] = c["p0"][0, 3:], c["v0"][0, 3:], c["params"][:, 0, 3:]
    par[:5, 3, :] *= np.random.default_rng(3).uniform(0.9, 1.1, (5, V))
    count = [k, 0, V, V]
    d = device_run(cuda, p0, v0, par, head, T, dt, tap, count=count)
    r = restated(p0, v0, par, head, T, dt, tap, count=count)
    assert np.all(np.isfinite(d["g_params"]))
    assert np.all(d["g_params"][:, 1, :] == 0) and np.all(d["g_params"][:, 0, k:] == 0)
    assert max(rel_elem(d["pT"], r["pT"]), rel_elem(d["vT"], r["vT"])) <= TOL_STATE
    for lane in (0, 2, 3):
        assert per_plane("%s lane %d device vs restatement" % (name, lane), d["g_params"][:, lane], r["g_params"][:, lane]) <= TOL_GRAD
    live = np.arange(V)[None, :] < np.array(count)[:, None]     # (slots beyond count pass through: the device returns 0 for them)
    assert grad_report("%s device vs restatement d loss / d p0" % name, d["g_p0"] * live, r["g_p0"] * live) <= TOL_GRAD
    assert grad_report("%s device vs restatement d loss / d v0" % name, d["g_v0"] * live, r["g_v0"] * live) <= TOL_GRAD
    assert per_plane("%s device vs golden" % name, d["g_params"][:, 2, :], g["g_params"].T) <= TOL_GRAD


@pytest.mark.parametrize("waves", [1, 2, 4])
def test_sweep_against_the_restatement(cuda, waves):
    """V in {1, 7, 64, 65, 256, 300, 1024} x L in {1, 5} x T in {1, 50, 200}, with and without count, with and without a loss on
    hist, under DHTS_OPT_MICRO_FWD_WAVES 1, 2, 4: every parameter plane within TOL_GRAD of the restatement; with them, bit-identity of
    everything else with the call that does not ask for the parameter gradient, repeatability, the zero slots."""
    from dhts import _lib
    rng = np.random.default_rng(100 + waves)
    lib = _lib.lib()
    assert lib.dhts_set_option(_lib.OPT_MICRO_FWD_WAVES, waves) == 0
    try:
        worst, cases = 0.0, 0
        for V in (1, 7, 64, 65, 256, 300, 1024):
            for L in (1, 5):
                for T in (1, 50, 200):
                    with_count, with_hist = bool(cases & 1), bool((cases >> 1) & 1)
                    cases += 1
                    for flip in (False, True):                         # both settings of (count, hist) for every shape
                        uc, uh = with_count != flip, with_hist != flip
                        p0, v0, par, head = lanes(rng, L, V)
                        count = [int(x) for x in rng.integers(max(V // 2, 1), V + 1, L)] if uc else None
                        if uc and L > 1:
                            count[1] = 0
                        g_pT, g_vT = rng.normal(size=(L, V)).astype(np.float32), rng.normal(size=(L, V)).astype(np.float32)
                        g_hist = rng.normal(size=(T, L, 2, V)).astype(np.float32) if uh else None
                        d = device_run(cuda, p0, v0, par, head, T, 0.01, None, count=count, g_pT=g_pT, g_vT=g_vT, g_hist=g_hist)
                        r = restated(p0, v0, par, head, T, 0.01, None, count=count, g_pT=g_pT, g_vT=g_vT, g_hist=g_hist)
                        tag = "V=%d L=%d T=%d count=%s hist=%s waves=%d" % (V, L, T, uc, uh, waves)
                        for q in range(6):
                            scale = max(float(np.max(np.abs(r["g_params"][q]))), 1e-30)
                            e = float(np.max(np.abs(d["g_params"][q] - r["g_params"][q])) / scale)
                            worst = max(worst, e)
                            assert e <= TOL_GRAD, "%s plane %d: %.2e" % (tag, q, e)
                        if count is not None:
                            for lane, n in enumerate(count):
                                assert np.all(d["g_params"][:, lane, n:] == 0), tag
                        # the same call without the parameter gradient: bit-identical outputs and state / head-gap gradients
                        s = device_run(cuda, p0, v0, par, head, T, 0.01, None, count=count, want_params=False, g_pT=g_pT, g_vT=g_vT, g_hist=g_hist)
                        assert s["g_params"] is None
                        for key in ("pT", "vT", "g_p0", "g_v0", "g_head"):
                            assert np.array_equal(d[key], s[key], equal_nan=True), "%s: %s differs from the state-only call" % (tag, key)
                        if uh:                                         # (the history holds live slots only: the rest is never written)
                            live = np.arange(V)[None, :] < np.array(count if count is not None else [V] * L)[:, None]
                            assert np.array_equal(d["hist"][:, live[:, None, :].repeat(2, 1)], s["hist"][:, live[:, None, :].repeat(2, 1)]), \
                                "%s: hist differs from the state-only call" % tag
                        d2 = device_run(cuda, p0, v0, par, head, T, 0.01, None, count=count, g_pT=g_pT, g_vT=g_vT, g_hist=g_hist)
                        assert np.array_equal(d["g_params"], d2["g_params"]), "%s: g_params differs between two runs" % tag
        print("waves %d: %d shapes x 2, worst parameter plane %.2e" % (waves, cases, worst))
    finally:
        lib.dhts_set_option(_lib.OPT_MICRO_FWD_WAVES, 0)


def test_lanes_are_independent(cuda):
    """A lane's result does not depend on its neighbours in the batch: bit for bit."""
    rng = np.random.default_rng(8)
    L, V, T = 6, 130, 60
    p0, v0, par, head = lanes(rng, L, V)
    count = [130, 0, 77, 130, 1, 64]
    full = device_run(cuda, p0, v0, par, head, T, 0.01, "every_sum", count=count)
    for lane in (0, 2, 4):
        one = device_run(cuda, p0[lane:lane + 1], v0[lane:lane + 1], par[:, lane:lane + 1], head[lane:lane + 1], T, 0.01, "every_sum",
                         count=count[lane:lane + 1])
        assert np.array_equal(one["g_params"][:, 0], full["g_params"][:, lane])
        assert np.array_equal(one["g_p0"][0], full["g_p0"][lane])


def test_shared_parameters_and_graph_replay(cuda):
    """params = theta[:, None, None].expand(6, L, V): theta.grad is the float64 sum of the planes; one captured-graph replay of forward +
    backward gives the eager result (nothing is allocated inside backward)."""
    import torch
    import dhts
    rng = np.random.default_rng(21)
    L, V, T, dt = 8, 64, 40, 0.01
    p0, v0, _, head = lanes(rng, L, V, random_params=False)
    tp0, tv0 = torch.tensor(p0, device=cuda), torch.tensor(v0, device=cuda)
    thead = torch.tensor(head, device=cuda, dtype=torch.float64)

    def run(theta):
        pT, vT, hist = dhts.micro_rollout(tp0, tv0, theta[:, None, None].expand(6, L, V), thead, T, dt, want_hist=True, check_faults=False)
        return (hist ** 2).mean() + (vT ** 2).mean()

    theta = torch.tensor(DEFAULT, device=cuda, requires_grad=True)
    loss = run(theta)
    loss.backward()
    eager = theta.grad.clone()
    full = torch.tensor(np.tile(DEFAULT[:, None, None], (1, L, V)), device=cuda, requires_grad=True)
    pT, vT, hist = dhts.micro_rollout(tp0, tv0, full, thead, T, dt, want_hist=True)
    ((hist ** 2).mean() + (vT ** 2).mean()).backward()
    assert torch.equal(eager, full.grad.sum(dim=(1, 2)))
    assert bool(torch.all(torch.isfinite(eager))) and float(eager.abs().min()) > 0

    static = torch.tensor(DEFAULT, device=cuda, requires_grad=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                               # warm-up outside the capture
        run(static).backward()
    torch.cuda.current_stream().wait_stream(side)
    static.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run(static)
        captured.backward()
    static.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static.grad, eager) and float(captured) == float(loss)


def test_parameter_tape_of_another_shape_is_refused(cuda):
    """A ptape written for another shape is not read: DHTS_FAULT_CAPACITY (index -3) and NaN, never a silent wrong answer."""
    import torch
    from dhts import _lib, ops
    rng = np.random.default_rng(2)
    L, V, T = 3, 70, 5
    p0, v0, par, head = lanes(rng, L, V)
    desc = ops.micro_desc(L, V, 0.01)
    tp, tv = torch.tensor(p0, device=cuda), torch.tensor(v0, device=cuda)
    tpar, thead = torch.tensor(par, device=cuda), torch.tensor(head, device=cuda)
    tape = torch.empty(ops.micro_tape_numel(desc, T), device=cuda)
    ptape = torch.zeros(ops.micro_param_tape_numel(desc, T), device=cuda)
    ops.micro_rollout_fwd(desc, T, tp, tv, tpar, thead, tape=tape, ptape=ptape)
    g = torch.ones(L, V, device=cuda)
    g_params = torch.empty(6, L, V, dtype=torch.float64, device=cuda)
    err = ops.new_error_record(cuda)
    ops.micro_rollout_bwd(desc, T, tape, g, g, err=err, ptape=ptape, params=tpar, g_params=g_params)
    assert err.tolist()[0] == 0 and bool(torch.all(torch.isfinite(g_params)))
    other = ops.micro_desc(L, V, 0.01)
    ptape4 = torch.zeros(ops.micro_param_tape_numel(other, T - 1), device=cuda)
    ops.micro_rollout_fwd(other, T - 1, tp, tv, tpar, thead, tape=tape, ptape=ptape4)       # a tape of T - 1 steps
    big = torch.zeros_like(ptape)
    big[:ptape4.numel()] = ptape4
    ops.micro_rollout_bwd(desc, T, tape, g, g, err=err, ptape=big, params=tpar, g_params=g_params)
    code, _, _, index = err.tolist()
    assert code == _lib.FAULT_CAPACITY and index == -3 and bool(torch.all(torch.isnan(g_params)))
    with pytest.raises(ValueError):
        ops.micro_rollout_bwd(desc, T, tape, g, g, ptape=ptape4, params=tpar, g_params=g_params)


def test_calibration_example_reduces_its_loss(cuda, tmp_path):
    """examples/calibrate_idm.py --n_episode 50 on a small problem ends with a loss below the one it started from."""
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "calibrate_idm.py"), "--n_episode", "50", "--n_lane", "8",
                          "--n_vehicle", "16", "--n_step", "100"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    files = [os.path.join(dp, f) for dp, _, fs in os.walk(str(tmp_path)) for f in fs if f.startswith("trial_") and f.endswith(".txt")]
    assert files, "no trial_k.txt written"
    losses = [float(line.split()[-1]) for line in open(files[0]) if line.strip()]
    print("calibration loss: first %.6g, last %.6g over %d iterations" % (losses[0], losses[-1], len(losses)))
    assert len(losses) >= 50 and losses[-1] < losses[0]
