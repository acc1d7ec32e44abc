"""On-ramp inflow and its tangent on the fused forward + tangent kernel (dhts.macro_rollout_jvp(fused=True, ramps=, inflow=, t_inflow=),
DESIGN 4n) without a GPU: the float64 chain tests/macro_ramp_jvp_ref.py against the chain it extends and against the oracle adjoint
macro_ramp_ref.ramp_bwd, the ValueErrors of the public call, the C entry points' argument checks and the compiler's resource listing of
macro_kernels.hip before and with the ramp forms of the fused kernel."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import macro_jvp_ref as J
import macro_ramp_jvp_ref as RJ
import macro_ramp_ref as R
from macro_ramp_ref import DT, DX, UM, F, ramp_bwd, ramp_fwd
from util import TOL_GRAD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. zero t_inflow is the chain it extends -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,ramps", [(3, (0, 1, 2)), (65, (63, 64)), (20, (0, 19))])
@pytest.mark.parametrize("bound", ("const", "sched"))
def test_zero_t_inflow_is_the_existing_chain(oracle, bound, N, ramps):
    T, L = 9, R.LANES
    f = R.case_oracle(oracle, bound, N, ramps, T)["f"]
    rng = np.random.default_rng(N)
    t_r0, t_u0 = rng.standard_normal((2, L, N))
    t_gr, t_gu = rng.standard_normal((2, T, L, 2))
    det = R.case_detectors(N, ramps)
    want = J.jvp(f, t_r0=t_r0, t_u0=t_u0, t_gr=t_gr, t_gu=t_gu, det=det)
    for t_inflow in (None, np.zeros((T, L, len(ramps)))):
        got = RJ.ramp_jvp(f, t_r0=t_r0, t_u0=t_u0, t_gr=t_gr, t_gu=t_gu, t_inflow=t_inflow, det=det)
        for k in want:
            assert np.all(got[k] == want[k]), k
    assert np.abs(want["t_read"]).max() > 0


# ---- 2. the adjoint identity against the oracle's reverse chain ----------------------------------------------------------------------
@pytest.mark.parametrize("N,ramps", [(3, (0, 1, 2)), (20, (0, 7, 19)), (65, (63, 64))])
@pytest.mark.parametrize("bound", R.BOUNDS)
def test_adjoint_identity_against_ramp_bwd(oracle, bound, N, ramps):
    """<g, J t> with J t from macro_ramp_jvp_ref against <J^T g, t> with J^T g from macro_ramp_ref.ramp_bwd, its g_inflow term
    sum(g_inflow * t_inflow) included, for random cotangents g of the final (r, y, u) alone and of (r, y, u) at the detector cells after
    every step alone, and random tangents of every leaf at once.
    The bound is TOL_GRAD of the sum of the absolute products of the left side, that of the two identity tests of
    tests/test_macro_jvp.py, and not the 1e-9 a float64 pair would meet: ramp_bwd is the oracle's float32 sweep (float32 cotangents, a
    float32 g_inflow), so the reference chain alone misses 1e-9 -- the figures this test prints are 2.7e-9 .. 2.1e-7, the rounding of
    that sweep."""
    T, L = 9, R.LANES
    f = R.case_oracle(oracle, bound, N, ramps, T)["f"]
    ring = bound == "ring"
    rng = np.random.default_rng(7 * N + len(bound))
    det = R.case_detectors(N, ramps)
    worst = 0.0
    for loss in ("final", "detectors"):
        t_r0, t_u0 = rng.standard_normal((2, L, N))
        t_gr, t_gu = (None, None) if ring else rng.standard_normal((2, T, L, 2))
        t_in = rng.standard_normal((T, L, len(ramps)))
        o = RJ.ramp_jvp(f, t_r0=t_r0, t_u0=t_u0, t_gr=t_gr, t_gu=t_gu, t_inflow=t_in, det=det)
        if loss == "final":
            g = rng.standard_normal((3, L, N)).astype(F)
            b = ramp_bwd(oracle, f, g_rT=g[0], g_yT=g[1], g_uT=g[2])
            left = [g[0].astype(np.float64) * o["t_rT"], g[1].astype(np.float64) * o["t_yT"], g[2].astype(np.float64) * o["t_uT"]]
        else:
            g = np.zeros((3, T, L, N), F)
            g[:, :, :, det] = rng.standard_normal((3, T, L, len(det))).astype(F)
            b = ramp_bwd(oracle, f, gh_r=g[0], gh_y=g[1], gh_u=g[2])
            left = [g[:, :, :, det].astype(np.float64).transpose(1, 2, 0, 3) * o["t_read"]]
        right = [b["g_r0"].astype(np.float64) * t_r0, b["g_u0"].astype(np.float64) * t_u0, b["g_inflow"].astype(np.float64) * t_in]
        if not ring:
            right += [b["g_ghost_r"].astype(np.float64) * t_gr, b["g_ghost_u"].astype(np.float64) * t_gu]
        assert np.abs(right[2]).sum() > 0, "the inflow term takes part"
        lhs, rhs = sum(float(x.sum()) for x in left), sum(float(x.sum()) for x in right)
        scale = sum(float(np.abs(x).sum()) for x in left)
        worst = max(worst, abs(lhs - rhs) / scale)
        print("%s N%d %s: <g, J t> = %.12g, <J^T g, t> = %.12g, |d| / sum |products| = %.2e" % (bound, N, loss, lhs, rhs, abs(lhs - rhs) / scale))
        assert abs(lhs - rhs) <= TOL_GRAD * scale
    # the inflow term alone: every other tangent zero, one entry of t_inflow
    t_in = np.zeros((T, L, len(ramps)))
    t_in[T // 2, 1, len(ramps) - 1] = 1.0
    o = RJ.ramp_jvp(f, t_inflow=t_in)
    g = rng.standard_normal((3, L, N)).astype(F)
    b = ramp_bwd(oracle, f, g_rT=g[0], g_yT=g[1], g_uT=g[2])
    left = [g[0].astype(np.float64) * o["t_rT"], g[1].astype(np.float64) * o["t_yT"], g[2].astype(np.float64) * o["t_uT"]]
    lhs, scale = sum(float(x.sum()) for x in left), sum(float(np.abs(x).sum()) for x in left)
    assert scale > 0 and abs(lhs - float(b["g_inflow"][T // 2, 1, len(ramps) - 1])) <= TOL_GRAD * scale


# ---- 3. the public call's ValueErrors, no device --------------------------------------------------------------------------------------
def test_value_errors_without_a_device():
    import torch
    import dhts
    L, N, T, K = 2, 16, 5, 3
    r0, u0 = torch.full((L, N), 0.3), torch.full((L, N), 10.0)
    g = torch.full((L, 2), 0.2)
    inflow, t_inflow, t_r0 = torch.zeros(T, L, 2), torch.zeros(K, T, L, 2), torch.zeros(K, L, N)

    def call(**kw):
        kw.setdefault("fused", True)
        ring = kw.get("ring", False)
        return dhts.macro_rollout_jvp(r0, u0, None if ring else g, None if ring else g, T, 0.01, 5.0, 30.0, **kw)
    for ring in (False, True):
        with pytest.raises(ValueError, match="ramps and inflow go together"):
            call(ramps=[1, 2], t_r0=t_r0, ring=ring)
        with pytest.raises(ValueError, match="ramps and inflow go together"):
            call(inflow=inflow, t_r0=t_r0, ring=ring)
        with pytest.raises(ValueError, match="t_inflow needs ramps"):
            call(t_inflow=t_inflow, ring=ring)
        with pytest.raises(ValueError, match="at least one of"):
            call(ramps=[1, 2], inflow=inflow, ring=ring)
        for bad in ([2, 1], [1, 1], [-1, 2], [3, N], [], [1.5, 2], torch.tensor([2, 1]), torch.tensor([0.0, 1.0])):
            with pytest.raises(ValueError, match="`ramps`"):
                call(ramps=bad, inflow=inflow, t_inflow=t_inflow, ring=ring)
        with pytest.raises(ValueError, match=r"inflow must be a float32 tensor of shape \(T, L, R\) = \(5, 2, 2\)"):
            call(ramps=[1, 2], inflow=inflow[:, :, :1], t_inflow=t_inflow, ring=ring)
        with pytest.raises(ValueError, match="inflow must be a float32 tensor"):
            call(ramps=[1, 2], inflow=inflow.double(), t_inflow=t_inflow, ring=ring)
        with pytest.raises(ValueError, match="inflow must live on r0's device"):
            call(ramps=[1, 2], inflow=inflow.to("meta"), t_inflow=t_inflow, ring=ring)
        with pytest.raises(ValueError, match=r"t_inflow must have shape \(3, 5, 2, 2\)"):
            call(ramps=[1, 2], inflow=inflow, t_inflow=t_inflow[:, :, :, :1], ring=ring)
        with pytest.raises(ValueError, match=r"t_inflow must have shape \(3, 5, 2, 2\)"):
            call(ramps=[1, 2], inflow=inflow, t_inflow=t_inflow[:, 1:], ring=ring)
        with pytest.raises(ValueError, match="all tangents share K = 3"):            # K is that of the first tangent given
            call(ramps=[1, 2], inflow=inflow, t_r0=t_r0, t_inflow=t_inflow[:2], ring=ring)
        with pytest.raises(ValueError, match="t_inflow must be a float32 tensor on r0's device"):
            call(ramps=[1, 2], inflow=inflow, t_inflow=t_inflow.double(), ring=ring)
        with pytest.raises(ValueError, match="t_inflow must be a float32 tensor on r0's device"):
            call(ramps=[1, 2], inflow=inflow, t_inflow=t_inflow.to("meta"), ring=ring)
        with pytest.raises(ValueError, match="leading direction axis"):
            call(ramps=[1, 2], inflow=inflow, t_inflow=t_inflow.tolist(), ring=ring)
        with pytest.raises(ValueError, match="`detectors`"):
            call(ramps=[1, 2], inflow=inflow, t_inflow=t_inflow, detectors=[3, 1], ring=ring)
    # the taped pair has no source: each of the three names fused=True
    for kw in (dict(ramps=[1, 2], inflow=inflow, t_r0=t_r0), dict(ramps=[1, 2], inflow=inflow, t_inflow=t_inflow)):
        with pytest.raises(ValueError, match="fused=True"):
            call(fused=False, **kw)
    with pytest.raises(ValueError, match="ramps and inflow go together"):
        call(fused=False, ramps=[1, 2], t_r0=t_r0)
    with pytest.raises(ValueError, match="t_inflow needs ramps"):
        call(fused=False, t_inflow=t_inflow)
    with pytest.raises(ValueError, match="ghost_r and ghost_u must be None when ring"):
        dhts.macro_rollout_jvp(r0, u0, g, g, T, 0.01, 5.0, 30.0, fused=True, ring=True, ramps=[1], inflow=inflow[:, :, :1],
                               t_inflow=t_inflow[:, :, :, :1])


def test_value_errors_of_the_raw_operators_without_a_device():
    import torch
    from dhts import ops
    L, N, T, K = 2, 16, 5, 3
    desc = ops.macro_desc(L, N, 0.01, 5.0, 30.0)
    s, gh, t = torch.zeros(L, N), torch.zeros(L, 2, 4), torch.zeros(K, L, N)
    cells, inflow, t_inflow = torch.zeros(2, dtype=torch.int32), torch.zeros(T, L, 2), torch.zeros(K, T, L, 2)
    with pytest.raises(ValueError, match="ramps and inflow go together"):
        ops.macro_rollout_fwd_jvp(desc, T, s, s, s, s, gh, t, t, ramps=cells)
    with pytest.raises(ValueError, match="ramps and inflow go together"):
        ops.macro_rollout_fwd_jvp_ring(desc, T, s, s, s, s, t, t, inflow=inflow)
    with pytest.raises(ValueError, match="t_inflow without ramps"):
        ops.macro_rollout_fwd_jvp(desc, T, s, s, s, s, gh, t, t, t_inflow=t_inflow)


# ---- 4. the C entry points' argument checks, no device ---------------------------------------------------------------------------------
def test_entry_points_reject_bad_ramp_arguments_without_a_device():
    """DHTS_E_INVALID before anything is dereferenced or launched: the addresses handed over are not memory."""
    from dhts import _lib, ops
    lib = _lib.lib()
    L, N, T = 2, 16, 5
    desc = ops.macro_desc(L, N, 0.01, 5.0, 30.0)
    p = C.c_void_p(0x1000)           # "an address": never read
    d = C.byref(desc)

    def open_lane(ramps=p, n_ramp=2, inflow=p, t_inflow=p, T=T, n_dir=1, sched=0, t_r=p, ghost=p):
        return lib.dhts_macro_rollout_fwd_jvp_ramp(d, T, n_dir, p, p, p, p, ghost, sched, t_r, p, None, p, p, p, p, p, p, None, 0, None,
                                                   None, None, None, None, ramps, n_ramp, inflow, t_inflow)

    def ring(ramps=p, n_ramp=2, inflow=p, t_inflow=p, T=T, n_dir=1, t_r=p):
        return lib.dhts_macro_rollout_fwd_jvp_ring_ramp(d, T, n_dir, p, p, p, p, t_r, p, p, p, p, p, p, p, None, 0, None, None, None,
                                                        None, None, ramps, n_ramp, inflow, t_inflow)
    for f in (open_lane, ring):
        assert f(ramps=None) == _lib.E_INVALID and f(inflow=None) == _lib.E_INVALID
        assert f(n_ramp=-1) == _lib.E_INVALID and f(n_ramp=-3, T=0) == _lib.E_INVALID
        assert f(ramps=None, t_inflow=None) == _lib.E_INVALID
        assert f(n_dir=0) == _lib.E_INVALID and f(t_r=None) == _lib.E_INVALID and f(T=-1) == _lib.E_INVALID        # the siblings' own
    assert open_lane(ghost=None) == _lib.E_INVALID
    big = ops.macro_desc(L, 1411, 0.01, 5.0, 30.0)                  # the cell limits hold as they stand
    assert lib.dhts_macro_rollout_fwd_jvp_ramp(C.byref(big), T, 1, p, p, p, p, p, 0, p, p, None, p, p, p, p, p, p, None, 0, None, None, None,
                                               None, None, p, 2, p, p) == _lib.E_INVALID
    for name in ("dhts_macro_rollout_fwd_jvp_ramp", "dhts_macro_rollout_fwd_jvp_ring_ramp"):
        txt = open(os.path.join(ROOT, "include", "dhts.h")).read()
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
        assert m, "include/dhts.h does not declare %s" % name
        assert len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
    plan = ops.macro_fwd_jvp_plan(ops.macro_desc(L, 997, 0.01, 5.0, 30.0), T, 5)
    assert plan["dirs_per_launch"] == 4 and plan["launches"] == 2


# ---- 5. the compiler's resource listing -----------------------------------------------------------------------------------------------
def _listing(name):
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", name)).read().splitlines():
        kernel, figures = line.split(" SGPRs ")
        rows[kernel.strip()] = "SGPRs " + " ".join(figures.split())
    return rows


def test_resource_listing_keeps_every_existing_kernel():
    """profiles/macro_ramp_jvp_resources_parent.txt against profiles/macro_ramp_jvp_resources.txt (compiler output for gfx950, one line
    per kernel of macro_kernels.hip): every kernel of the parent has identical figures, the fifty-four fused forward + tangent ones under
    the name that the new last template argument gives them (kRamp = false); the fifty-four new lines are their kRamp = true siblings --
    kK in {1, 2, 4} x kP in {0, 1, 2} x three boundaries x kTaps --, none with scratch, a vector-register spill or static LDS."""
    parent, new = _listing("macro_ramp_jvp_resources_parent.txt"), _listing("macro_ramp_jvp_resources.txt")
    stem = "macro_rollout_fwd_jvp_kernel<"

    def renamed(k, ramp="false"):
        return k[:-1] + ", %s>" % ramp if k.startswith(stem) else k
    assert len(parent) == 233 and sum(k.startswith(stem) for k in parent) == 54
    for k, figures in parent.items():
        assert new.get(renamed(k)) == figures, k
    added = sorted(set(new) - {renamed(k) for k in parent})
    assert added == sorted(renamed(k, "true") for k in parent if k.startswith(stem))
    forms = {(kk, kp, kb, kt) for kk in (1, 2, 4) for kp in (0, 1, 2) for kb in (0, 1, 2) for kt in ("false", "true")}
    assert {tuple(int(x) if x.isdigit() else x for x in re.match(r".*<(\d), (\d), \(dhts::MacroBoundary\)(\d), (\w+), true>", k).groups())
            for k in added} == forms

    def num(row, key):
        return int(re.search(r"%s\s+(\d+)" % key, row).group(1))
    for k in added:
        assert " scratch 0 " in new[k] and " vgpr_spill 0 " in new[k] and num(new[k], "AGPRs") == 0, (k, new[k])
        assert num(new[k], "LDS") == 0 and num(new[k], "VGPRs") <= 168, (k, new[k])
