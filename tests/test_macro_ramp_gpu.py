"""On-ramp inflow of the checkpointed ARZ rollout on the GPU (dhts.macro_rollout(ramps=, inflow=)): states, readings, sse and
every gradient against the chained oracle tests/macro_ramp_ref.py for the three boundary forms and the three observation forms, zero
inflow against the EXISTING checkpointed forms bit for bit, the segment length, mass on the ring, translation over the seam, indices
outside the lane, the CFL record, T = 0 and the example.  The cases are macro_ramp_ref's (tests/test_macro_ramp.py holds them to the
input conditions on the oracle); every one is a few thousand cell-steps."""
import os
import subprocess
import sys

import numpy as np
import pytest

import macro_ramp_ref as R
from macro_ramp_ref import DT, DX, LANES, UM, F
from macro_sched_ref import boundary_ry_to_ru
from util import TOL_GRAD, TOL_STATE, grad_report, rel_max, state_report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {"state": 0.0, "grad": 0.0}


def tt(cuda, a, grad=False):
    import torch
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=cuda, requires_grad=grad)


def bits(a):
    return a.detach().cpu().numpy().view(np.int32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def rollout(cuda, r, u, gr, gu, T, loss, N, ramps=None, inflow=None, target=None, checkpoint=True, grad=True, det=None):
    """dhts.macro_rollout of one case -> (outputs, dict of the leaves' gradients).  gr None: a ring.  ramps None: the existing form."""
    import dhts
    leaves = dict(r0=tt(cuda, r, grad), u0=tt(cuda, u, grad), ghost_r=tt(cuda, gr, grad), ghost_u=tt(cuda, gu, grad))
    kw = dict(checkpoint=checkpoint, ring=gr is None)
    if ramps is not None:
        leaves["inflow"] = tt(cuda, inflow, grad)
        kw.update(ramps=ramps, inflow=leaves["inflow"])
    if loss == "detectors":
        kw["detectors"] = R.case_detectors(N, ramps) if det is None else det
    elif loss == "target":
        kw["target"] = tt(cuda, target)
    out = dhts.macro_rollout(leaves["r0"], leaves["u0"], leaves["ghost_r"], leaves["ghost_u"], T, DT, DX, UM, **kw)
    if grad:
        (((out[0] ** 2).sum() + (out[2] ** 2).sum()) if loss == "final" else out[4].sum()).backward()
    return out, {k: (v.grad if v is not None and grad else None) for k, v in leaves.items()}


def case(cuda, oracle, bound, N, ramps, T, loss, checkpoint=True, **kw):
    c = R.case_oracle(oracle, bound, N, ramps, T, loss)
    out, g = rollout(cuda, c["r"], c["u"], c["gr"], c["gu"], T, loss, N, list(ramps), c["inflow"], c["tg"], checkpoint, **kw)
    return c, out, g


def held(kind, tag, a, ref):
    e = (state_report if kind == "state" else grad_report)(tag, a.detach().cpu().numpy() if hasattr(a, "detach") else a, ref)
    WORST[kind] = max(WORST[kind], e)
    return e


# ---- (a), (b): states, readings, sse and gradients against the chained oracle -------------------------------------------------------
@pytest.mark.parametrize("N,ramps", R.RAMP_SETS)
@pytest.mark.parametrize("loss", R.LOSSES)
def test_against_the_chained_oracle(cuda, oracle, N, ramps, loss):
    for T, segment in R.STEPS:
        for bound in R.BOUNDS:
            c, out, g = case(cuda, oracle, bound, N, ramps, T, loss, checkpoint=segment or True)
            f, b = c["f"], c[loss]
            tag = "%s N=%d %s T=%d %s" % (bound, N, ramps, T, loss)
            # the float32 states and readings: measured 0 in every case, so equality is what is held; sse is a double sum
            # taken in another order than numpy's and is held at TOL_STATE
            for k, name in enumerate(("rT", "yT", "uT")):
                assert held("state", "%s %s" % (name, tag), out[k], f[name]) == 0.0
            if loss == "detectors":
                det = R.case_detectors(N, ramps)
                for k, name in enumerate(("hist_r", "hist_y", "hist_u")):
                    assert held("state", "readings %s %s" % (name, tag), out[4][:, :, k], f[name][:, :, det]) == 0.0
            if loss == "target":
                assert held("state", "sse %s" % tag, out[4], R.case_sse(f, c["tg"])) <= TOL_STATE
            assert held("grad", "g_r0 %s" % tag, g["r0"], b["g_r0"]) <= TOL_GRAD
            assert held("grad", "g_u0 %s" % tag, g["u0"], b["g_u0"]) <= TOL_GRAD
            assert held("grad", "g_inflow %s" % tag, g["inflow"], b["g_inflow"]) <= TOL_GRAD
            if bound == "sched":
                assert held("grad", "g_ghost_r %s" % tag, g["ghost_r"], b["g_ghost_r"]) <= TOL_GRAD
                assert held("grad", "g_ghost_u %s" % tag, g["ghost_u"], b["g_ghost_u"]) <= TOL_GRAD
            if bound == "const":                 # the constant cells' gradient: the per-step cotangents summed in double, then the glue
                want_r, want_u = boundary_ry_to_ru(b["g_ghost_ry"].sum(axis=0), c["gr"], c["gu"], UM)
                assert held("grad", "g_ghost_r %s" % tag, g["ghost_r"], want_r) <= TOL_GRAD
                assert held("grad", "g_ghost_u %s" % tag, g["ghost_u"], want_u) <= TOL_GRAD
    print("largest difference so far: states %.2e, gradients %.2e" % (WORST["state"], WORST["grad"]))


def test_long_ring_and_the_one_cell_ring(cuda, oracle):
    """The 64-cell ring for 2 N + 5 steps at the plan's own segment, ramps at both ends of the seam; and N = 1, where the cell is its own
    neighbour, the step leaves it as it is and the source alone moves it: exactly the chain of float32 adds."""
    N, ramps, T = R.RING_LONG
    for loss in R.LOSSES:
        c, out, g = case(cuda, oracle, "ring", N, ramps, T, loss)
        for k, name in enumerate(("rT", "yT", "uT")):
            assert held("state", "%s long ring %s" % (name, loss), out[k], c["f"][name]) == 0.0
        for k, name in (("r0", "g_r0"), ("u0", "g_u0"), ("inflow", "g_inflow")):
            assert held("grad", "%s long ring %s" % (name, loss), g[k], c[loss][name]) <= TOL_GRAD
    c, out, g = case(cuda, oracle, "ring", 1, (0,), 11, "final")
    chain = c["r"][:, 0].copy()
    for t in range(11):
        chain = (chain.astype(np.float64) + DT * c["inflow"][t, :, 0].astype(np.float64)).astype(F)
    assert np.array_equal(out[0].detach().cpu().numpy()[:, 0], chain)
    assert np.array_equal(out[0].detach().cpu().numpy(), c["f"]["rT"]) and np.array_equal(out[1].detach().cpu().numpy(), c["f"]["yT"])
    assert held("grad", "g_inflow N=1", g["inflow"], c["final"]["g_inflow"]) <= TOL_GRAD


# ---- (c): zero inflow is the existing checkpointed form -------------------------------------------------------------------------------
@pytest.mark.parametrize("N,ramps", [(3, (0, 1, 2)), (64, (0, 63)), (65, (63, 64)), (300, (150, 151))])
@pytest.mark.parametrize("loss", R.LOSSES)
def test_zero_inflow_is_the_existing_form(cuda, oracle, N, ramps, loss):
    import torch
    T = 11
    for bound in R.BOUNDS:
        c = R.case_oracle(oracle, bound, N, ramps, T)
        zero = np.zeros_like(c["inflow"])
        det = R.case_detectors(N, ramps)
        a, ga = rollout(cuda, c["r"], c["u"], c["gr"], c["gu"], T, loss, N, list(ramps), zero, c["tg"], 4)
        b, gb = rollout(cuda, c["r"], c["u"], c["gr"], c["gu"], T, loss, N, None, None, c["tg"], 4, det=det)
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert torch.equal(x, y), (bound, loss)
        for k in ("r0", "u0", "ghost_r", "ghost_u"):
            assert (ga[k] is None) == (gb[k] is None) and (ga[k] is None or torch.equal(ga[k], gb[k])), (bound, loss, k)
        # ... and inflow.grad is then the cut identity's value: for the last row, dt times the incoming cotangent of r itself
        if loss == "final":
            from dhts import ops
            g_r = (2 * a[0].detach()).contiguous()
            g_y = torch.zeros_like(g_r)
            ops.macro_u_tap_bwd(a[0].detach().contiguous(), a[1].detach().contiguous(), (2 * a[2].detach()).contiguous(), g_r, g_y, UM)
            want = (DT * g_r.double()).float()[:, list(ramps)]
            assert torch.equal(ga["inflow"][T - 1], want), bound
        assert bool((ga["inflow"] != 0).any())


@pytest.mark.parametrize("N,ramps", [(64, (0, 63)), (65, (63, 64))])
@pytest.mark.parametrize("loss", R.LOSSES)
@pytest.mark.parametrize("bound", R.BOUNDS)
def test_zero_inflow_gradient_is_the_cut_identity_in_every_row(cuda, oracle, bound, N, ramps, loss):
    """Rows t < T - 1 of inflow.grad, which the SWEEP's owner writes: with all-zero inflow, row t is (float)(dt (double)G_r) with G_r
    what the EXISTING kRamp = false pair yields, through the raw wrappers and in (r, y), for the rollout's remaining T - 1 - t steps
    started from the state after step t -- its g_r0, and in front of it row t's own detector column resp. target pair, added as the
    sweep adds them.  Held under torch.equal for the three boundary forms and the three losses."""
    import torch
    import dhts
    from dhts import ops
    T, S = 11, 4
    c = R.case_oracle(oracle, bound, N, ramps, T)
    out, g = rollout(cuda, c["r"], c["u"], c["gr"], c["gu"], T, loss, N, list(ramps), np.zeros_like(c["inflow"]), c["tg"], S)
    got, cols = g["inflow"], list(ramps)
    det_cells = R.case_detectors(N, ramps)
    det = torch.tensor(det_cells, dtype=torch.int32, device=cuda) if loss == "detectors" else None
    tg = tt(cuda, c["tg"])
    rT, yT, uT = (out[k].detach().contiguous() for k in range(3))
    g_rT, g_yT = torch.zeros_like(rT), torch.zeros_like(rT)
    if loss == "final":
        g_rT = (2 * rT).contiguous()
        ops.macro_u_tap_bwd(rT, yT, (2 * uT).contiguous(), g_rT, g_yT, UM)
    if loss == "detectors":
        gs = ops._per_step_cotangent(out[4].detach(), torch.ones_like(out[4]), UM)         # [T][L][2][D]: the whole run's rows
    for t in (0, 3, T - 2):
        n = T - 1 - t
        cut = (lambda a, lo, hi: None if a is None else tt(cuda, a if a.ndim == 2 else a[lo:hi]))
        with torch.no_grad():                # the state after step t: the existing form (zero inflow has its bits, the test above)
            st = dhts.macro_rollout(tt(cuda, c["r"]), tt(cuda, c["u"]), cut(c["gr"], 0, t + 1), cut(c["gu"], 0, t + 1), t + 1, DT, DX, UM,
                                    ring=bound == "ring", checkpoint=S)
        r_t, y_t, u_t, q_t = (x.contiguous() for x in st[:4])
        ghost = None if bound == "ring" else ops._macro_leaves(r_t, u_t, cut(c["gr"], t + 1, T), cut(c["gu"], t + 1, T), UM)[-1]
        desc = ops.macro_desc(LANES, N, DT, DX, UM)
        ckpt = torch.empty(ops.macro_ckpt_numel(desc, n, S), dtype=torch.float32, device=cuda)
        if loss == "target":
            rest = tg[t + 1:].contiguous()
            ops.macro_rollout_fwd_ckpt_target(desc, n, r_t, y_t, u_t, q_t, ghost, ckpt, rest, segment=S)
            G = ops.macro_rollout_bwd_ckpt_target(desc, n, ckpt, r_t, y_t, u_t, q_t, ghost, g_rT, g_yT, rest,
                                                  g_sse=torch.ones(LANES, 2, dtype=torch.float64, device=cuda), final=(rT, yT, uT), segment=S)[0]
            a = torch.where(torch.isnan(tg[t, :, 0]), torch.zeros_like(r_t), 2 * (r_t - tg[t, :, 0])).contiguous()
            g_u = torch.where(torch.isnan(tg[t, :, 1]), torch.zeros_like(r_t), 2 * (u_t - tg[t, :, 1])).contiguous()
            ops.macro_u_tap_bwd(r_t, y_t, g_u, a, torch.zeros_like(a), UM)                 # row t's pair, as the replay forms it
            G = G + a
        else:
            ops.macro_rollout_fwd_ckpt(desc, n, r_t, y_t, u_t, q_t, ghost, ckpt, segment=S, det=det)
            G = ops.macro_rollout_bwd_ckpt(desc, n, ckpt, r_t, y_t, u_t, q_t, ghost, g_rT, g_yT, segment=S, det=det,
                                           g_taps=None if det is None else gs[t + 1:].contiguous())[0].clone()
            if det is not None:
                G[:, det_cells] += gs[t, :, 0, :]                                            # row t's own detector column
        want = (DT * G.double()).float()[:, cols]
        assert torch.equal(got[t], want), (bound, loss, t, (got[t] - want).abs().max().item())
        assert bool((got[t] != 0).any())


# ---- (d): the segment length ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,ramps", [(64, (0, 63)), (129, (63, 64))])
@pytest.mark.parametrize("loss", R.LOSSES)
def test_the_segment_changes_no_bit(cuda, oracle, N, ramps, loss):
    T = 11
    for bound in R.BOUNDS:
        got = [case(cuda, oracle, bound, N, ramps, T, loss, checkpoint=s)[1:] for s in (1, 4, True)]
        for out, g in got[1:]:
            for x, y in zip(out, got[0][0]):
                assert same_bits(x, y), (bound, loss)
            for k, v in g.items():
                assert v is None or same_bits(v, got[0][1][k]), (bound, loss, k)


# ---- (e): mass on the ring --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,ramps,T", [(1, (0,), 11), (2, (0, 1), 11), (64, (0, 63), 133), (65, (63, 64), 11), (300, (0, 299), 11)])
def test_mass_balance_on_the_ring(cuda, oracle, N, ramps, T):
    """|sum r_T - sum r_0 - dt sum inflow| per lane, sums in float64, within T (N + R) 2^-24 max r: one float32 store per cell-step and
    one more per ramp cell-step, each half an ulp of a value below max r < 1."""
    c, out, _ = case(cuda, oracle, "ring", N, ramps, T, "final", grad=False)
    r_T = out[0].detach().cpu().numpy().astype(np.float64)
    got = np.abs(r_T.sum(axis=1) - c["r"].astype(np.float64).sum(axis=1) - DT * c["inflow"].astype(np.float64).sum(axis=(0, 2)))
    bound = T * (N + len(ramps)) * 2.0 ** -24 * max(float(r_T.max()), float(c["f"]["hist_r"].max()), float(c["r"].max()))
    print("mass balance N=%d T=%d: %.3e (bound %.3e)" % (N, T, got.max(), bound))
    assert got.max() <= bound


# ---- (f): translation over the seam -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (2, 64, 65))
def test_rolling_the_ring_rolls_the_result(cuda, oracle, N):
    import torch
    ramps, T = (0, N - 1), 11
    c = R.case_oracle(oracle, "ring", N, ramps, T)
    rng = np.random.default_rng(N)
    w = tt(cuda, rng.standard_normal((2, LANES, N)).astype(F))
    rolled = sorted((k + 1) % N for k in ramps)                          # cells 0 and N - 1 become 1 and 0
    cols = [ramps.index((k - 1) % N) for k in rolled]
    res = []
    for r, u, cells, inflow, ww in ((c["r"], c["u"], list(ramps), c["inflow"], w),
                                    (np.roll(c["r"], 1, 1), np.roll(c["u"], 1, 1), rolled, c["inflow"][:, :, cols], torch.roll(w, 1, 2))):
        import dhts
        tr, tu, ti = tt(cuda, r, True), tt(cuda, u, True), tt(cuda, inflow, True)
        out = dhts.macro_rollout(tr, tu, None, None, T, DT, DX, UM, ring=True, checkpoint=4, ramps=cells, inflow=ti)
        ((out[0] * ww[0]).sum() + (out[2] * ww[1]).sum()).backward()
        res.append((out, tr.grad, tu.grad, ti.grad))
    (a, a_r, a_u, a_i), (b, b_r, b_u, b_i) = res
    for k in range(4):
        assert same_bits(torch.roll(a[k], 1, 1), b[k]), k
    e = max(rel_max(b_r.cpu().numpy(), np.roll(a_r.cpu().numpy(), 1, 1)), rel_max(b_u.cpu().numpy(), np.roll(a_u.cpu().numpy(), 1, 1)),
            rel_max(b_i.cpu().numpy(), a_i.cpu().numpy()[:, :, cols]))
    print("N = %d: largest difference of rolled gradients %.2e" % (N, e))
    assert e <= TOL_GRAD


# ---- (g): indices outside the lane ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", R.BOUNDS)
def test_bad_indices_name_no_cell(cuda, oracle, bound):
    import torch
    N, ramps, T = 65, (63, 64), 11
    c = R.case_oracle(oracle, bound, N, ramps, T)
    wide = np.zeros((T, LANES, 4), F)
    wide[:, :, 1], wide[:, :, 3] = c["inflow"][:, :, 0], c["inflow"][:, :, 1]
    wide[:, :, 0], wide[:, :, 2] = 7.0, -9.0                             # what the two bad columns hold must not matter
    cells = torch.tensor([N, 63, -1, 64], dtype=torch.int32, device=cuda)
    for loss in R.LOSSES:
        det = torch.tensor(R.case_detectors(N, ramps), dtype=torch.int32, device=cuda)
        a, ga = rollout(cuda, c["r"], c["u"], c["gr"], c["gu"], T, loss, N, list(ramps), c["inflow"], c["tg"], 4)
        b, gb = rollout(cuda, c["r"], c["u"], c["gr"], c["gu"], T, loss, N, cells, wide, c["tg"], 4, det=det)
        for x, y in zip(a, b):
            assert torch.equal(x, y), loss
        for k in ("r0", "u0", "ghost_r", "ghost_u"):
            assert ga[k] is None or torch.equal(ga[k], gb[k]), (loss, k)
        assert torch.equal(gb["inflow"][:, :, [1, 3]], ga["inflow"]) and not bool(gb["inflow"][:, :, [0, 2]].any())


# ---- (h): the CFL record ----------------------------------------------------------------------------------------------------------------
def test_cfl_fault_of_a_huge_inflow(cuda, oracle):
    """An inflow of 1e9 / s into cell 40 of lane 1 in step 2 leaves a density of 1e7 there: the next step's interfaces beside it fail the
    CFL test on the oracle and on the device alike -- the project's own fault record, raised by arithmetic; no device fault."""
    import dhts
    from dhts import _lib, ops
    N, ramps, T = 65, (40,), 6
    r, u = R.case_state(N, ramps)
    gr, gu = R.case_bounds("const", T)
    inflow = R.ramp_inflow(T, LANES, 1, DT)
    inflow[2, 1, 0] = 1e9
    f = R.ramp_fwd(oracle, r, u, T, DT, DX, UM, ramps, inflow, gr, gu, check=False)
    assert f["rc"] is not None and f["rc"][:2] == (3, 1)
    for bound in R.BOUNDS:
        g = (None, None) if bound == "ring" else ((gr, gu) if bound == "const" else (np.broadcast_to(gr, (T, LANES, 2)), np.broadcast_to(gu, (T, LANES, 2))))
        want = R.ramp_fwd(oracle, r, u, T, DT, DX, UM, ramps, inflow, g[0], g[1], check=False)["rc"]
        with pytest.raises(AssertionError, match=r"CFL condition.*\(step %d, lane %d, " % want[:2]):
            dhts.macro_rollout(tt(cuda, r), tt(cuda, u), tt(cuda, g[0]), tt(cuda, g[1]), T, DT, DX, UM, ring=bound == "ring", checkpoint=True,
                               ramps=list(ramps), inflow=tt(cuda, inflow))
    desc = ops.macro_desc(LANES, N, DT, DX, UM)
    tr, tu = tt(cuda, r), tt(cuda, u)
    y, q = ops.macro_state_from_ru(tr, tu, UM)
    err = ops.new_error_record(cuda)
    ckpt = tt(cuda, np.zeros(ops.macro_ckpt_numel(desc, T), F))
    ops.macro_rollout_fwd_ckpt_ramp(desc, T, tr, y, tu, q, None, ckpt, tt(cuda, np.array(ramps, np.int32)), tt(cuda, inflow), err=err)
    assert err.tolist()[:3] == [_lib.FAULT_CFL, 3, 1]


# ---- T = 0 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", R.BOUNDS)
def test_no_steps_pass_through(cuda, oracle, bound):
    N, ramps = 65, (63, 64)
    r, u = R.case_state(N, ramps)
    gr, gu = R.case_bounds(bound, 0)
    empty = np.zeros((0, LANES, 2), F)
    for loss in R.LOSSES:
        out, g = rollout(cuda, r, u, gr, gu, 0, loss, N, list(ramps), empty, np.zeros((0, LANES, 2, N), F))
        assert same_bits(out[0], tt(cuda, r)) and same_bits(out[2], tt(cuda, u))
        assert tuple(g["inflow"].shape) == (0, LANES, 2)
        if loss == "final":
            # d(r^2 + u^2) / d(r, u) through the float32 glue (r, u) -> (r, y) -> (r, u): two terms of size |2 u| um / (2 sqrt r) < 1e3
            # cancel in g_r0, so it is 2 r to a few float32 roundings of those, 2e-4; g_u0 = (g / r) r has no such terms
            assert np.allclose(g["r0"].cpu().numpy(), 2 * r, rtol=0, atol=2e-4) and np.allclose(g["u0"].cpu().numpy(), 2 * u, rtol=1e-6)


# ---- (i): the example -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ([], ["--estimate"]))
def test_the_example_lowers_its_loss_and_writes_its_log(cuda, mode, tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "ramp_metering.py"), "--n_cell", "48", "--n_timestep", "80", "--n_episode", "12",
           "--run_name", "t"] + mode
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout + p.stderr
    sub = "estimate" if mode else "meter"
    lines = open(os.path.join(str(tmp_path), "result", "ramp", "t", sub, "trial_0.txt")).read().split("\n")[:-1]
    losses = [float(line.split()[-1]) for line in lines]
    assert len(losses) == 12 and losses[-1] < losses[0], p.stdout
