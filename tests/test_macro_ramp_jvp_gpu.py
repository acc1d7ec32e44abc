"""On-ramp inflow and its tangent on the fused forward + tangent kernel on the GPU (dhts.macro_rollout_jvp(fused=True, ramps=, inflow=,
t_inflow=)): the primal's bits against the checkpointed forward with the same source, every tangent against the float64
chain tests/macro_ramp_jvp_ref.py, the adjoint identity against the existing reverse form, bit relations with the existing fused
kernel (zero inflow, slices of the directions, one entry of t_inflow, rolling a ring), indices outside the lane, guard bands, the
record of a non-finite tangent and the example.  The cases are macro_ramp_ref's (tests/test_macro_ramp.py holds them to the input
conditions on the oracle); every one is a few thousand cell-steps."""
import os
import subprocess
import sys

import numpy as np
import pytest

import macro_ramp_jvp_ref as RJ
import macro_ramp_ref as R
from macro_ramp_ref import DT, DX, LANES, UM, F
from util import TOL_GRAD, grad_report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 5                                # two launches, of 4 and 1
WORST = {"tangent": 0.0}


def tt(cuda, a, grad=False):
    import torch
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=cuda, requires_grad=grad)


def bits(a):
    return a.detach().cpu().numpy().view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def seeds(bound, N, n_ramp, T, seed=0):
    """Seeded normal tangents of every leaf at once, K directions: t_r0, t_u0 [K][L][N]; on an open lane t_ghost_r, t_ghost_u [K][L][2]
    or, beside a schedule, [K][T][L][2]; t_inflow [K][T][L][R]."""
    rng = np.random.default_rng(1000 * N + 10 * T + seed)
    s = dict(t_r0=rng.standard_normal((K, LANES, N)).astype(F), t_u0=rng.standard_normal((K, LANES, N)).astype(F),
             t_inflow=rng.standard_normal((K, T, LANES, n_ramp)).astype(F))
    if bound != "ring":
        shape = (K, LANES, 2) if bound == "const" else (K, T, LANES, 2)
        s["t_ghost_r"], s["t_ghost_u"] = rng.standard_normal(shape).astype(F), rng.standard_normal(shape).astype(F)
    return s


def fused(cuda, c, T, ramps=None, inflow=None, tangents=None, det=None, sl=slice(0, K), **kw):
    """dhts.macro_rollout_jvp(fused=True) of a case, the directions `sl` of `tangents`.  ramps None: the existing form."""
    import dhts
    tan = {k: tt(cuda, v[sl]) for k, v in tangents.items()}
    if ramps is not None:
        kw.update(ramps=ramps, inflow=tt(cuda, inflow))
    return dhts.macro_rollout_jvp(tt(cuda, c["r"]), tt(cuda, c["u"]), tt(cuda, c["gr"]), tt(cuda, c["gu"]), T, DT, DX, UM, fused=True,
                                  ring=c["gr"] is None, detectors=det, **tan, **kw)


def reference(c, bound, T, s, d, det):
    """The float64 chain of direction d."""
    tg = {}
    if bound == "const":
        tg = dict(t_gr=np.tile(s["t_ghost_r"][d][None], (T, 1, 1)), t_gu=np.tile(s["t_ghost_u"][d][None], (T, 1, 1)))
    elif bound == "sched":
        tg = dict(t_gr=s["t_ghost_r"][d], t_gu=s["t_ghost_u"][d])
    return RJ.ramp_jvp(c["f"], t_r0=s["t_r0"][d], t_u0=s["t_u0"][d], t_inflow=s["t_inflow"][d], det=det, **tg)


# ---- primal bits, tangents against the float64 chain -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,ramps", R.RAMP_SETS)
def test_primal_bits_and_tangents_against_the_chain(cuda, oracle, N, ramps):
    """The first call below is dhts.macro_rollout_jvp(..., ramps=...): a TypeError without the feature."""
    import dhts
    for T, _ in R.STEPS:
        for bound in R.BOUNDS:
            c = R.case_oracle(oracle, bound, N, ramps, T)
            s = seeds(bound, N, len(ramps), T)
            for det in (None, R.case_detectors(N, ramps)):
                prim, tan = fused(cuda, c, T, list(ramps), c["inflow"], s, det)
                want = dhts.macro_rollout(tt(cuda, c["r"]), tt(cuda, c["u"]), tt(cuda, c["gr"]), tt(cuda, c["gu"]), T, DT, DX, UM,
                                          ring=bound == "ring", checkpoint=True, ramps=list(ramps), inflow=tt(cuda, c["inflow"]), detectors=det)
                assert len(prim) == len(want) == (4 if det is None else 5)
                for k in range(len(want)):
                    assert same_bits(prim[k], want[k]), (bound, T, det, k)
                for k, name in enumerate(("rT", "yT", "uT")):          # ... which are the oracle's (tests/test_macro_ramp_gpu.py)
                    assert np.array_equal(prim[k].cpu().numpy(), c["f"][name])
                assert tuple(tan[0].shape) == (K, LANES, N) and (det is None or tuple(tan[3].shape) == (K, T, LANES, 3, len(det)))
                for d in range(K):
                    ref = reference(c, bound, T, s, d, det)
                    tag = "%s N=%d %s T=%d det=%s direction %d" % (bound, N, ramps, T, det is not None, d)
                    for k, name in enumerate(("t_rT", "t_yT", "t_uT")):
                        e = grad_report("%s %s" % (name, tag), tan[k][d].cpu().numpy(), ref[name])
                        WORST["tangent"] = max(WORST["tangent"], e)
                        assert e <= TOL_GRAD, (name, tag)
                    if det is not None:
                        e = grad_report("t_readings %s" % tag, tan[3][d].cpu().numpy(), ref["t_read"])
                        WORST["tangent"] = max(WORST["tangent"], e)
                        assert e <= TOL_GRAD, tag
    print("largest tangent difference so far: %.2e" % WORST["tangent"])


# ---- the adjoint identity against the existing reverse form ----------------------------------------------------------------------------
@pytest.mark.parametrize("N,ramps", R.RAMP_SETS)
def test_adjoint_identity_against_the_reverse_form(cuda, oracle, N, ramps):
    """<w, J t> with J t from the fused call against <J^T w, t> with J^T w from dhts.macro_rollout(checkpoint=True, ramps=, inflow=,
    detectors=).backward(): seeded weights on rT, uT and the readings, every leaf's tangent at once, per direction, within TOL_GRAD of
    the sum of the absolute products of the left side (tests/test_macro_ring_gpu.py::test_fused_tangents' measure)."""
    import dhts
    T = 11
    det = R.case_detectors(N, ramps)
    for bound in R.BOUNDS:
        c = R.case_oracle(oracle, bound, N, ramps, T)
        s = seeds(bound, N, len(ramps), T, seed=1)
        rng = np.random.default_rng(N + T)
        w_r, w_u = (tt(cuda, rng.standard_normal((LANES, N)).astype(F)) for _ in range(2))
        w_d = tt(cuda, rng.standard_normal((T, LANES, 3, len(det))).astype(F))
        prim, tan = fused(cuda, c, T, list(ramps), c["inflow"], s, det)
        leaves = dict(t_r0=tt(cuda, c["r"], True), t_u0=tt(cuda, c["u"], True), t_ghost_r=tt(cuda, c["gr"], True),
                      t_ghost_u=tt(cuda, c["gu"], True), t_inflow=tt(cuda, c["inflow"], True))
        out = dhts.macro_rollout(leaves["t_r0"], leaves["t_u0"], leaves["t_ghost_r"], leaves["t_ghost_u"], T, DT, DX, UM, ring=bound == "ring",
                                 checkpoint=True, ramps=list(ramps), inflow=leaves["t_inflow"], detectors=det)
        ((out[0] * w_r).sum() + (out[2] * w_u).sum() + (out[4] * w_d).sum()).backward()
        assert float(leaves["t_inflow"].grad.abs().sum()) > 0
        for d in range(K):
            left = [tan[0][d].double() * w_r.double(), tan[2][d].double() * w_u.double(), tan[3][d].double() * w_d.double()]
            lhs, scale = float(sum(x.sum() for x in left)), float(sum(x.abs().sum() for x in left))
            rhs = float(sum((v.grad.double() * tt(cuda, s[k][d]).double()).sum() for k, v in leaves.items() if v is not None))
            print("%s N = %d %s direction %d: <w, J t> = %.6e, <J^T w, t> = %.6e, |d| / sum |products| = %.2e"
                  % (bound, N, ramps, d, lhs, rhs, abs(lhs - rhs) / max(scale, 1e-30)))
            assert abs(lhs - rhs) <= TOL_GRAD * max(scale, 1e-30), (bound, d)


# ---- bit relations -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,ramps", [(3, (0, 1, 2)), (64, (0, 63)), (65, (63, 64)), (300, (150, 151))])
def test_zero_inflow_without_t_inflow_is_the_existing_fused_call(cuda, oracle, N, ramps):
    T = 11
    for bound in R.BOUNDS:
        c = R.case_oracle(oracle, bound, N, ramps, T)
        s = seeds(bound, N, len(ramps), T)
        del s["t_inflow"]
        for det in (None, R.case_detectors(N, ramps)):
            a = fused(cuda, c, T, list(ramps), np.zeros_like(c["inflow"]), s, det)
            b = fused(cuda, c, T, None, None, s, det)
            for x, y in zip(a[0] + a[1], b[0] + b[1]):
                assert same_bits(x, y), (bound, det)


@pytest.mark.parametrize("N,ramps", [(3, (0, 1, 2)), (65, (63, 64)), (129, (0, 128))])
def test_a_direction_does_not_depend_on_its_slot_or_launch(cuda, oracle, N, ramps):
    T = 11
    det = R.case_detectors(N, ramps)
    for bound in R.BOUNDS:
        c = R.case_oracle(oracle, bound, N, ramps, T)
        s = seeds(bound, N, len(ramps), T)
        full = fused(cuda, c, T, list(ramps), c["inflow"], s, det)
        for sl in (slice(0, 1), slice(4, 5), slice(1, 4), slice(0, 4), slice(2, 5)):      # K = 1, 1, 3, 4, 3: other slots, other launches
            part = fused(cuda, c, T, list(ramps), c["inflow"], s, det, sl)
            for k in range(5):
                assert same_bits(part[0][k], full[0][k]), (bound, sl, k)
            for k in range(4):
                assert same_bits(part[1][k], full[1][k][sl]), "%s: direction %s in a launch of %d: output %d" % (bound, sl, sl.stop - sl.start, k)
        only = dict(t_inflow=s["t_inflow"])                      # t_inflow as the one tangent given ...
        zeros = {k: np.zeros_like(v) for k, v in s.items() if k != "t_inflow"}
        a = fused(cuda, c, T, list(ramps), c["inflow"], only, det)
        b = fused(cuda, c, T, list(ramps), c["inflow"], dict(zeros, **only), det)      # ... is the others at zero
        for x, y in zip(a[1], b[1]):
            assert same_bits(x, y), bound
        assert float(a[1][0].abs().sum()) > 0


@pytest.mark.parametrize("bound", R.BOUNDS)
def test_a_run_time_number_of_passes_changes_no_bit(cuda, oracle, bound):
    """DHTS_OPT_MACRO_FWD_WAVES = 1 puts the 300-cell lane on ONE wavefront of five passes: the kernel forms with a run-time number of
    passes, which hold no row of inflow in registers and load in the step.  Same bits as the plan's own mapping (three wavefronts of two
    passes), primal and tangents, with the ramps either side of a pass boundary and at both ends."""
    from dhts import _lib, ops
    N, T = 300, 11
    for ramps in ((63, 64), (0, 299)):
        c = R.case_oracle(oracle, bound, N, ramps, T)
        s = seeds(bound, N, len(ramps), T)
        det = R.case_detectors(N, ramps)
        desc = ops.macro_desc(LANES, N, DT, DX, UM)
        assert ops.macro_fwd_jvp_plan(desc, T, K)["passes"] == 2
        want = fused(cuda, c, T, list(ramps), c["inflow"], s, det)
        assert _lib.lib().dhts_set_option(_lib.OPT_MACRO_FWD_WAVES, 1) == 0
        try:
            assert ops.macro_fwd_jvp_plan(desc, T, K)["passes"] == 5
            got = fused(cuda, c, T, list(ramps), c["inflow"], s, det)
            only = fused(cuda, c, T, list(ramps), c["inflow"], {k: v for k, v in s.items() if k != "t_inflow"}, det)
        finally:
            _lib.lib().dhts_set_option(_lib.OPT_MACRO_FWD_WAVES, 0)
        for x, y in zip(want[0] + want[1], got[0] + got[1]):
            assert same_bits(x, y), (bound, ramps)
        for x, y in zip(want[0], only[0]):               # t_inflow NULL: nothing is loaded, the primal is the same
            assert same_bits(x, y), (bound, ramps)


@pytest.mark.parametrize("bound", R.BOUNDS)
def test_one_entry_of_t_inflow_is_a_tangent_seeded_behind_its_step(cuda, oracle, bound):
    """Zero inflow, every tangent zero but t_inflow[0][t][l][j] = a: the final tangents are those of the EXISTING fused operator
    (ops.macro_rollout_fwd_jvp without ramps) over the remaining T - 1 - t steps from the state after step t, started from
    t_r = (float)(dt a) at cell ramps[j] of lane l and t_y = 0 -- bit for bit."""
    import torch
    import dhts
    from dhts import ops
    N, ramps, T = 65, (63, 64), 11
    c = R.case_oracle(oracle, bound, N, ramps, T)
    a = 0.8125
    for t, l, j in ((3, 1, 0), (0, 2, 1), (T - 1, 0, 1)):
        t_in = np.zeros((1, T, LANES, len(ramps)), F)
        t_in[0, t, l, j] = a
        _, tan = fused(cuda, c, T, list(ramps), np.zeros_like(c["inflow"]), dict(t_inflow=t_in))
        cut = (lambda x, lo, hi: None if x is None else tt(cuda, x if x.ndim == 2 else x[lo:hi]))
        with torch.no_grad():                # the state after step t: the existing checkpointed form
            st = dhts.macro_rollout(tt(cuda, c["r"]), tt(cuda, c["u"]), cut(c["gr"], 0, t + 1), cut(c["gu"], 0, t + 1), t + 1, DT, DX, UM,
                                    ring=bound == "ring", checkpoint=True)
        r_t, y_t, u_t, q_t = (x.contiguous() for x in st[:4])
        ghost = None if bound == "ring" else ops._macro_leaves(r_t, u_t, cut(c["gr"], t + 1, T), cut(c["gu"], t + 1, T), UM)[-1]
        t_r = torch.zeros(1, LANES, N, device=cuda)
        t_r[0, l, ramps[j]] = float(np.float32(DT * np.float64(np.float32(a))))
        _, want = ops.macro_rollout_fwd_jvp(ops.macro_desc(LANES, N, DT, DX, UM), T - 1 - t, r_t, y_t, u_t, q_t, ghost, t_r, torch.zeros_like(t_r))
        assert same_bits(tan[0], want[0]) and same_bits(tan[1], want[1]), (bound, t)
        assert float(tan[0].abs().sum()) > 0


@pytest.mark.parametrize("N", (2, 64, 65))
def test_rolling_the_ring_rolls_primal_and_tangents(cuda, oracle, N):
    import torch
    ramps, T = (0, N - 1), 11
    c = R.case_oracle(oracle, "ring", N, ramps, T)
    s = seeds("ring", N, len(ramps), T)
    det = sorted({0, N - 1})
    rolled = sorted((k + 1) % N for k in ramps)                          # cells 0 and N - 1 become 1 and 0
    cols = [ramps.index((k - 1) % N) for k in rolled]
    a = fused(cuda, c, T, list(ramps), c["inflow"], s, det)
    c2 = dict(r=np.roll(c["r"], 1, 1), u=np.roll(c["u"], 1, 1), gr=None, gu=None)
    s2 = dict(t_r0=np.roll(s["t_r0"], 1, 2), t_u0=np.roll(s["t_u0"], 1, 2), t_inflow=s["t_inflow"][:, :, :, cols])
    b = fused(cuda, c2, T, rolled, c["inflow"][:, :, cols], s2, sorted((k + 1) % N for k in det))
    dcols = [det.index((k - 1) % N) for k in sorted((k + 1) % N for k in det)]
    for k in range(4):
        assert same_bits(torch.roll(a[0][k], 1, 1), b[0][k]), k
    for k in range(3):
        assert same_bits(torch.roll(a[1][k], 1, 2), b[1][k]), k
    assert same_bits(a[0][4][:, :, :, dcols], b[0][4]) and same_bits(a[1][3][:, :, :, :, dcols], b[1][3])


# ---- indices outside the lane ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", R.BOUNDS)
def test_bad_indices_name_no_cell(cuda, oracle, bound):
    import torch
    N, ramps, T = 65, (63, 64), 11
    c = R.case_oracle(oracle, bound, N, ramps, T)
    s = seeds(bound, N, len(ramps), T)
    wide = np.zeros((T, LANES, 4), F)
    wide[:, :, 1], wide[:, :, 3] = c["inflow"][:, :, 0], c["inflow"][:, :, 1]
    wide[:, :, 0], wide[:, :, 2] = 7.0, -9.0                             # what the two bad columns hold must not matter
    t_wide = np.full((K, T, LANES, 4), 3.0, F)
    t_wide[:, :, :, 1], t_wide[:, :, :, 3] = s["t_inflow"][:, :, :, 0], s["t_inflow"][:, :, :, 1]
    cells = torch.tensor([N, 63, -1, 64], dtype=torch.int32, device=cuda)
    det = R.case_detectors(N, ramps)
    a = fused(cuda, c, T, list(ramps), c["inflow"], s, det)
    b = fused(cuda, c, T, cells, wide, dict(s, t_inflow=t_wide), det)
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert same_bits(x, y)


# ---- guard bands ------------------------------------------------------------------------------------------------------------------------------
GUARD, SENTINEL = 257, 12345.0


def guarded(cuda, shape):
    import torch
    n = int(np.prod(shape))
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=cuda)
    view = buf[GUARD:GUARD + n]
    view.fill_(float("nan"))
    return buf, view.view(*shape)


def intact(buf, view):
    b = buf.cpu().numpy()
    n = view.numel()
    return bool(np.all(b[:GUARD] == SENTINEL) and np.all(b[GUARD + n:] == SENTINEL)) and not bool(view.isnan().any())


@pytest.mark.parametrize("N", (1, 65, 129))
def test_guard_bands_around_every_output(cuda, N):
    from dhts import ops
    L, T = LANES, 7
    ramps = {1: (0,), 65: (63, 64), 129: (0, 128)}[N]
    det = sorted({0, N - 1})
    D = len(det)
    desc = ops.macro_desc(L, N, DT, DX, UM)
    r, u = R.case_state(N, ramps)
    tr, tu = tt(cuda, r), tt(cuda, u)
    y, q = ops.macro_state_from_ru(tr, tu, UM)
    rng = np.random.default_rng(N)
    inflow = tt(cuda, R.ramp_inflow(T, L, len(ramps), DT, seed=N))
    cells, dt_ = tt(cuda, np.array(ramps, np.int32)), tt(cuda, np.array(det, np.int32))
    for bound in R.BOUNDS if N > 1 else ("ring",):
        gr, gu = R.case_bounds(bound, T)
        ghost = None if bound == "ring" else ops._macro_leaves(tr, tu, tt(cuda, gr), tt(cuda, gu), UM)[-1]
        g = dict(out=[guarded(cuda, (L, N)) for _ in range(4)] + [guarded(cuda, (K, L, N)) for _ in range(2)],
                 taps=guarded(cuda, (T, L, 3, D)), t_taps=guarded(cuda, (K, T, L, 2, D)))
        ops.macro_rollout_fwd_jvp(desc, T, tr, y, tu, q, ghost, tt(cuda, rng.standard_normal((K, L, N)).astype(F)),
                                  tt(cuda, rng.standard_normal((K, L, N)).astype(F)), det=dt_, out=tuple(v for _, v in g["out"]),
                                  taps=g["taps"][1], t_taps=g["t_taps"][1], ramps=cells, inflow=inflow,
                                  t_inflow=tt(cuda, rng.standard_normal((K, T, L, len(ramps))).astype(F)))
        for i, (buf, view) in enumerate(g["out"] + [g["taps"], g["t_taps"]]):
            assert intact(buf, view), "%s: a store beside buffer %d, or elements of it not written" % (bound, i)


# ---- a non-finite tangent -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", R.BOUNDS)
def test_a_nan_in_t_inflow_goes_on_the_tangent_record(cuda, oracle, bound):
    """One NaN entry of t_inflow at (t, l, j): err_jvp holds (DHTS_FAULT_NAN, t, l, ramps[j]) -- the lane's earliest --, the forward's
    record stays clean, and the public call raises from the tangent record."""
    import dhts
    from dhts import _lib, ops
    N, ramps, T = 65, (63, 64), 11
    c = R.case_oracle(oracle, bound, N, ramps, T)
    s = seeds(bound, N, len(ramps), T)
    t, l, j = 4, 1, 1
    s["t_inflow"][K - 1, t, l, j] = np.nan             # the last direction: the second launch
    desc = ops.macro_desc(LANES, N, DT, DX, UM)
    tr, tu = tt(cuda, c["r"]), tt(cuda, c["u"])
    y, q = ops.macro_state_from_ru(tr, tu, UM)
    ghost = None if bound == "ring" else ops._macro_leaves(tr, tu, tt(cuda, c["gr"]), tt(cuda, c["gu"]), UM)[-1]
    err, err_jvp = ops.new_error_record(cuda), ops.new_error_record(cuda)
    t_r = tt(cuda, s["t_r0"])
    ops.macro_rollout_fwd_jvp(desc, T, tr, y, tu, q, ghost, t_r, t_r.clone(), err=err, err_jvp=err_jvp,
                              ramps=tt(cuda, np.array(ramps, np.int32)), inflow=tt(cuda, c["inflow"]), t_inflow=tt(cuda, s["t_inflow"]))
    assert err.tolist()[0] == 0
    assert err_jvp.tolist() == [_lib.FAULT_NAN, t, l, ramps[j]]
    with pytest.raises(Exception, match=r"step %d, lane %d" % (t, l)):
        fused(cuda, c, T, list(ramps), c["inflow"], s)


# ---- T = 0 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", R.BOUNDS)
def test_no_steps_pass_through(cuda, oracle, bound):
    N, ramps = 65, (63, 64)
    r, u = R.case_state(N, ramps)
    gr, gu = R.case_bounds(bound, 0)
    s = seeds(bound, N, len(ramps), 0)
    prim, tan = fused(cuda, dict(r=r, u=u, gr=gr, gu=gu), 0, list(ramps), np.zeros((0, LANES, 2), F), s, [0, 64])
    assert same_bits(prim[0], tt(cuda, r)) and same_bits(prim[2], tt(cuda, u)) and same_bits(tan[0], tt(cuda, s["t_r0"]))
    assert tuple(prim[4].shape) == (0, LANES, 3, 2) and tuple(tan[3].shape) == (K, 0, LANES, 3, 2)


# ---- the example ----------------------------------------------------------------------------------------------------------------------------
def test_the_example_fits_the_pulse_by_levenberg_marquardt(cuda, tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "ramp_metering.py"), "--n_cell", "48", "--n_timestep", "80", "--n_episode", "12",
           "--run_name", "t", "--seed", "3", "--estimate", "--method", "lm"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout + p.stderr
    lines = open(os.path.join(str(tmp_path), "result", "ramp", "t", "estimate", "trial_0.txt")).read().split("\n")[:-1]
    errors, losses = [float(line.split()[0]) for line in lines], [float(line.split()[1]) for line in lines]
    print(p.stdout)
    assert len(errors) == 12 and errors[-1] < errors[0] and losses[-1] < losses[0], p.stdout
