"""On-ramp inflow of the checkpointed ARZ rollout (dhts.macro_rollout(ramps=, inflow=)) without a GPU: the chained oracle
tests/macro_ramp_ref.py against the chains it extends, its own bookkeeping (the cut identity), the input conditions of every case
tests/test_macro_ramp_gpu.py runs, the ValueErrors of the public call, the C entry points' argument checks and the compiler's resource
listing of macro_kernels.hip before and with the ramp forms."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import macro_ramp_ref as R
from macro_ramp_ref import DT, DX, UM, F, ramp_bwd, ramp_fwd
from macro_ring_ref import ring_bwd, ring_fwd
from macro_sched_ref import sched_bwd, sched_fwd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. zero inflow is the chain it extends -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,ramps", [(3, (0, 1, 2)), (65, (63, 64)), (20, (0, 19))])
def test_zero_inflow_is_the_existing_chain(oracle, N, ramps):
    T, L = 9, R.LANES
    r, u = R.case_state(N, ramps)
    zero = np.zeros((T, L, len(ramps)), F)
    gh = np.random.default_rng(N).standard_normal((3, T, L, N)).astype(F)
    cot = dict(gh_r=gh[0], gh_y=gh[1], gh_u=gh[2])
    gr, gu = R.case_bounds("sched", T)
    for f, want_f, want_g in (
            (ramp_fwd(oracle, r, u, T, DT, DX, UM, ramps, zero, gr, gu), sched_fwd(oracle, r, u, gr, gu, DT, DX, UM), sched_bwd),
            (ramp_fwd(oracle, r, u, T, DT, DX, UM, ramps, zero), ring_fwd(oracle, r, u, T, DT, DX, UM), ring_bwd)):
        for k in ("rT", "yT", "uT", "qT", "hist_r", "hist_y", "hist_u"):
            assert np.array_equal(f[k], want_f[k]), k
        for kw in (dict(g_rT=2 * f["rT"], g_uT=2 * f["uT"]), cot):
            got, want = ramp_bwd(oracle, f, **kw), want_g(oracle, want_f, **kw)
            for k in want:
                assert np.array_equal(got[k], want[k]), k


# ---- 2. the cut identity ----------------------------------------------------------------------------------------------------------------
def _rest(f, t):
    """The rollout's remaining T - 1 - t steps as a run of its own, started from the state after step t: what sched_bwd / ring_bwd take."""
    g = dict(T=f["T"] - 1 - t, um=f["um"], r0=f["hist_r"][t], u0=f["hist_u"][t], tape=[steps[t + 1:] for steps in f["tape"]],
             rT=f["rT"], yT=f["yT"], uT=f["uT"])
    for k in ("hist_r", "hist_y", "hist_u"):
        g[k] = f[k][t + 1:]
    if not f["ring"]:
        g["gr"], g["gu"] = f["gr"][t + 1:], f["gu"][t + 1:]
    return g


@pytest.mark.parametrize("bound", R.BOUNDS)
def test_cut_identity(oracle, bound):
    """g_inflow[t, l, j] is dt times the g_r that the EXISTING chain (sched_bwd / ring_bwd) yields at cell ramps[j] for the rollout's
    remaining T - 1 - t steps started from the state after step t.  The existing chains return the gradient of the leaves (r, u); the
    sweep's running cotangent is that of (r, y) with y = r (u - u_eq(r)), so L_y = g_u / r and L_r = g_r - L_y dy/dr, formed here in
    double: the identity holds the bookkeeping -- which row, which cell, which step -- to the rounding of that float32 glue, 1e-5 of
    the largest entry, not the arithmetic."""
    N, ramps, T = 20, (0, 7, 19), 9
    c = R.case_oracle(oracle, bound, N, ramps, T, "final")
    f, b = c["f"], c["final"]
    cot = R.case_cotangents(f, "final", N, ramps)
    for t in (0, 3, T - 2):
        rest = (ring_bwd if bound == "ring" else sched_bwd)(oracle, _rest(f, t), **cot)
        r, u = f["hist_r"][t].astype(np.float64), f["hist_u"][t].astype(np.float64)
        ueq = UM * (1.0 - np.sqrt(r + 1e-5))
        dueq = -UM * 0.5 / np.sqrt(r + 1e-5)
        L_y = rest["g_u0"].astype(np.float64) / r
        L_r = rest["g_r0"].astype(np.float64) - L_y * ((u - ueq) - r * dueq)
        want = DT * L_r[:, list(ramps)]
        assert np.max(np.abs(b["g_inflow"][t] - want)) <= 1e-5 * np.max(np.abs(want)), t
    a, _ = R.glue_u_bwd(f["rT"], f["yT"], UM, cot["g_uT"])          # row T - 1: the incoming cotangent itself
    want = (DT * (np.asarray(cot["g_rT"], F) + a).astype(np.float64)).astype(F)
    assert np.array_equal(b["g_inflow"][T - 1], want[:, list(ramps)])


# ---- 3. the input conditions of every GPU case --------------------------------------------------------------------------------------
def test_every_gpu_case_meets_the_input_conditions(oracle):
    """rc == 0 in every step (ramp_fwd asserts it), every r inside [0.02, 0.98], every ramp cell's g_inflow with a non-zero entry under
    each of the three losses, and an interface beside every ramp cell non-trivial in some step.  (The one-cell ring is exempt from the
    last: both of its interfaces have the same state on either side in every step.)"""
    from dhts import ops
    n = neg = tot = 0
    for bound, N, ramps, T in R.all_cases():
        c = R.case_oracle(oracle, bound, N, ramps, T)
        f = c["f"]
        assert f["rc"] is None
        lo, hi = min(f["hist_r"].min(), f["r0"].min()), max(f["hist_r"].max(), f["r0"].max())
        assert 0.02 <= lo and hi <= 0.98, (bound, N, ramps, T, lo, hi)
        assert np.abs(c["inflow"].astype(np.float64)).sum(axis=0).max() * DT <= 0.2 * (1 + 1e-6)
        neg, tot = neg + int((c["inflow"] < 0).sum()), tot + c["inflow"].size
        for loss in R.LOSSES:
            g = R.case_oracle(oracle, bound, N, ramps, T, loss)[loss]["g_inflow"]
            assert np.all(np.any(g != 0, axis=(0, 1))), (bound, N, ramps, T, loss)
        if N > 1:
            for l in range(R.LANES):
                for cell in ramps:
                    assert R.interface_live(f, l, cell), (bound, N, ramps, T, l, cell)
        n += 1
    assert n == 2 * 3 * len(R.RAMP_SETS) + 2 + len(R.RING_EXTRA) and 0.15 < neg / tot < 0.25
    passes = {N: ops.macro_ckpt_plan(ops.macro_desc(R.LANES, N, DT, DX, UM), 11)["passes"] for N, _ in R.RAMP_SETS}
    assert passes[64] == 1 and passes[2] == 1 and passes[65] == 2 and passes[129] == 2 and passes[300] == 2


# ---- 4. the public call's ValueErrors, no device --------------------------------------------------------------------------------------
def test_value_errors_without_a_device():
    import torch
    import dhts
    L, N, T = 2, 16, 5
    r0, u0 = torch.full((L, N), 0.3), torch.full((L, N), 10.0)
    g = torch.full((L, 2), 0.2)
    inflow = torch.zeros(T, L, 2)

    def call(**kw):
        kw.setdefault("checkpoint", True)
        ring = kw.get("ring", False)
        return dhts.macro_rollout(r0, u0, None if ring else g, None if ring else g, T, 0.01, 5.0, 30.0, **kw)
    with pytest.raises(ValueError, match="ramps and inflow go together"):
        call(ramps=[1, 2])
    with pytest.raises(ValueError, match="ramps and inflow go together"):
        call(inflow=inflow)
    with pytest.raises(ValueError, match="ramps live on the checkpointed path only"):
        call(ramps=[1, 2], inflow=inflow, checkpoint=None)
    with pytest.raises(ValueError, match="ramps do not take want_hist"):
        call(ramps=[1, 2], inflow=inflow, want_hist=True)
    for bad in ([2, 1], [1, 1], [-1, 2], [3, N], [], [1.5, 2], torch.tensor([2, 1]), torch.tensor([0.0, 1.0])):
        with pytest.raises(ValueError, match="`ramps`"):
            call(ramps=bad, inflow=inflow)
    with pytest.raises(ValueError, match=r"inflow must be a float32 tensor of shape \(T, L, R\) = \(5, 2, 2\)"):
        call(ramps=[1, 2], inflow=inflow[:, :, :1])
    with pytest.raises(ValueError, match="inflow must be a float32 tensor"):
        call(ramps=[1, 2], inflow=inflow.double())
    with pytest.raises(ValueError, match="inflow must be a float32 tensor"):
        call(ramps=[1, 2], inflow=inflow.tolist())
    with pytest.raises(ValueError, match="inflow must live on r0's device"):
        call(ramps=[1, 2], inflow=inflow.to("meta"))
    for ring in (False, True):                   # the forms' own checks still come first or after, none of them on a device
        with pytest.raises(ValueError, match="target does not take detectors"):
            call(ramps=[1, 2], inflow=inflow, ring=ring, detectors=[0], target=torch.zeros(T, L, 2, N))
        with pytest.raises(ValueError, match="`detectors`"):
            call(ramps=[1, 2], inflow=inflow, ring=ring, detectors=[3, 1])
        with pytest.raises(ValueError, match="segment must be"):
            call(ramps=[1, 2], inflow=inflow, ring=ring, checkpoint=10 ** 6)
    # target and checkpoint handed over by position land in ramps and inflow, which now stand in front of them: told so, loudly
    with pytest.raises(ValueError, match="target= and checkpoint= are passed by keyword"):
        dhts.macro_rollout(r0, u0, g, g, T, 0.01, 5.0, 30.0, False, True, None, False, torch.zeros(T, L, 2, N), True)
    with pytest.raises(ValueError, match="target= and checkpoint= are passed by keyword"):
        dhts.macro_rollout(r0, u0, g, g, T, 0.01, 5.0, 30.0, False, True, None, False, torch.zeros(T, L, 2, N))
    with pytest.raises(ValueError, match="ghost_r and ghost_u must be None when ring"):
        dhts.macro_rollout(r0, u0, g, g, T, 0.01, 5.0, 30.0, ring=True, checkpoint=True, ramps=[1], inflow=inflow[:, :, :1])


# ---- 5. the C entry points' argument checks, no device ---------------------------------------------------------------------------------
def test_entry_points_reject_bad_ramp_arguments_without_a_device():
    """DHTS_E_INVALID before anything is dereferenced or launched: the addresses handed over are not memory."""
    from dhts import _lib, ops
    lib = _lib.lib()
    L, N, T = 2, 16, 5
    desc = ops.macro_desc(L, N, 0.01, 5.0, 30.0)
    p = C.c_void_p(0x1000)           # "an address": never read
    d = C.byref(desc)

    def fwd(ramps=p, n_ramp=2, inflow=p, ring=0, ghost=p, T=T):
        return lib.dhts_macro_rollout_fwd_ckpt_ramp(d, T, 0, p, p, p, p, ghost, 0, p, p, p, p, None, 0, None, p, ramps, n_ramp, inflow, ring,
                                                    None, None)

    def bwd(ramps=p, n_ramp=2, inflow=p, g_inflow=p, ring=0, ghost=p):
        return lib.dhts_macro_rollout_bwd_ckpt_ramp(d, T, 0, p, p, p, p, p, ghost, 0, p, p, None, 0, None, p, p, p, ramps, n_ramp, inflow,
                                                    g_inflow, ring, None, None)

    def fwd_t(ramps=p, n_ramp=2, inflow=p, ring=0, ghost=p):
        return lib.dhts_macro_rollout_fwd_ckpt_target_ramp(d, T, 0, p, p, p, p, ghost, 0, p, p, p, p, p, p, p, ramps, n_ramp, inflow, ring,
                                                           None, None)

    def bwd_t(ramps=p, n_ramp=2, inflow=p, g_inflow=p, ring=0, ghost=p):
        return lib.dhts_macro_rollout_bwd_ckpt_target_ramp(d, T, 0, p, p, p, p, p, ghost, 0, p, p, p, p, p, p, p, p, p, p, ramps, n_ramp,
                                                           inflow, g_inflow, ring, None, None)
    for f in (fwd, bwd, fwd_t, bwd_t):
        assert f(ramps=None) == _lib.E_INVALID and f(inflow=None) == _lib.E_INVALID
        assert f(n_ramp=0) == _lib.E_INVALID and f(n_ramp=N + 1) == _lib.E_INVALID and f(n_ramp=-3) == _lib.E_INVALID
        assert f(ring=1) == _lib.E_INVALID                       # a ring takes no ghost
    assert bwd(g_inflow=None) == _lib.E_INVALID and bwd_t(g_inflow=None) == _lib.E_INVALID
    assert fwd(n_ramp=0, T=0) == _lib.E_INVALID                  # n_ramp is checked whatever T is


# ---- 6. the compiler's resource listing -----------------------------------------------------------------------------------------------
def _listing(name):
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", name)).read().splitlines():
        kernel, figures = line.split(" SGPRs ")
        rows[kernel.strip()] = "SGPRs " + " ".join(figures.split())
    return rows


def test_resource_listing_keeps_every_existing_kernel():
    """profiles/macro_ramp_resources_parent.txt against profiles/macro_ramp_resources.txt (compiler output for gfx950, one line per kernel
    of macro_kernels.hip): every kernel of the parent has identical figures, the twenty-seven checkpointed ones under the name that the
    new last template argument gives them (kRamp = false); the twenty-seven new lines are their kRamp = true siblings, none with scratch
    or a vector-register spill, none below the reverse kernels' occupancy."""
    parent, new = _listing("macro_ramp_resources_parent.txt"), _listing("macro_ramp_resources.txt")
    stems = ("macro_rollout_ckpt_fwd_kernel<", "macro_rollout_ckpt_bwd_kernel<", "macro_rollout_ckpt_fwd_target_kernel<",
             "macro_rollout_ckpt_bwd_target_kernel<")

    def renamed(k, ramp="false"):
        return k[:-1] + ", %s>" % ramp if k.startswith(stems) else k
    assert len(parent) == 206 and sum(k.startswith(stems) for k in parent) == 27
    for k, figures in parent.items():
        assert new.get(renamed(k)) == figures, k
    added = sorted(set(new) - {renamed(k) for k in parent})
    assert added == sorted(renamed(k, "true") for k in parent if k.startswith(stems))

    def num(row, key):
        return int(re.search(r"%s\s+(\d+)" % key, row).group(1))
    for k in added:
        sibling = new[k[:-len("true>")] + "false>"]
        assert " scratch 0 " in new[k] and " vgpr_spill 0 " in new[k], (k, new[k])
        assert num(new[k], "LDS") == num(sibling, "LDS") == 0
        if "_bwd_" in k:
            assert num(new[k], "occupancy") == num(sibling, "occupancy"), (k, new[k], sibling)
        else:
            assert num(new[k], "occupancy") >= num(sibling, "occupancy") - 1, (k, new[k], sibling)
