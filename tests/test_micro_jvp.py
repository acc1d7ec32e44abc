"""Forward-mode tangent sweep of the fused IDM rollout (dhts_micro_rollout_jvp / dhts_micro_jvp_plan and dhts.micro_rollout_jvp): the
boundary of the library -- header, bindings, exports, argument checks, the plan, the operator's ValueErrors -- and the two references of
tests/test_micro_jvp_gpu.py (tests/micro_jvp_ref.py): the numpy chain, held against the pinned oracle adjoint by the dot-product identity
<g, J t> = <J^T g, t>, and the float64 yardstick torch.func.jvp(lane_rollout), held against the chain on the oracle's tape.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import micro_jvp_ref as J
from test_micro_params_gpu import lanes
from util import TOL_GRAD, TOL_STATE, rel_elem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dhts_micro_rollout_jvp", "dhts_micro_jvp_plan")
# (L, V, T, dt, head gap): the shapes the yardstick was checked at; collision-free in the oracle
SHAPES = [(3, 70, 60, 0.05, (1000.0, 0.0)), (2, 130, 100, 0.05, (15.0, 2.0)), (2, 300, 200, 0.02, (1000.0, 0.0)), (1, 1, 5, 0.1, (1000.0, 0.0))]
IDS = ["L%d_V%d_T%d" % s[:3] for s in SHAPES]


def test_header_library_and_bindings_hold_the_new_entry_points():
    import dhts
    from dhts import _lib, ops
    raw = open(os.path.join(ROOT, "include", "dhts.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib.lib()
    for name in NEW:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, txt)
        assert m, "include/dhts.h does not declare %s" % name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
        assert len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name          # the header's argument count
    assert len(_lib.SIGNATURES[NEW[0]][1]) == 16 and len(_lib.SIGNATURES[NEW[1]][1]) == 5
    assert "_micro_lane.py:131-214" in raw[raw.index("Forward-mode tangent sweep (Jacobian-vector products) over a rollout's tape"):]
    for name in ("micro_rollout_jvp", "micro_jvp_plan"):
        assert callable(getattr(ops, name))
    assert callable(dhts.micro_rollout_jvp) and dhts.micro_rollout_jvp is not ops.micro_rollout_jvp


def jvp_args(some, **kw):
    """(n_dir, tape, ptape, count, params, t_p, t_v, t_head, t_params, t_p_out, t_v_out, t_hist, err, stream)"""
    a = dict(n_dir=3, tape=some, ptape=some, count=some, params=some, t_p=some, t_v=some, t_head=some, t_params=some, t_p_out=some,
             t_v_out=some, t_hist=some, err=some, stream=None)
    a.update(kw)
    return list(a.values())


def test_bad_arguments_are_rejected_without_a_gpu():
    from dhts import _lib
    lib = _lib.lib()
    ok = _lib.MicroDesc(4, 70, 0.01)
    some = C.c_void_p(64)                      # a non-NULL pointer that is never dereferenced: the checks come first
    jvp, plan = lib.dhts_micro_rollout_jvp, lib.dhts_micro_jvp_plan
    out = (C.c_int32 * 8)()
    for T in (0, 3):
        for n_dir in (0, -2):
            assert jvp(C.byref(ok), T, *jvp_args(some, n_dir=n_dir)) == _lib.E_INVALID
        for missing in ("t_p", "t_v", "t_p_out", "t_v_out"):
            assert jvp(C.byref(ok), T, *jvp_args(some, **{missing: None})) == _lib.E_INVALID
            assert jvp(C.byref(ok), T, *jvp_args(some, ptape=None, params=None, t_params=None, **{missing: None})) == _lib.E_INVALID
        for a in ("ptape", "params", "t_params"):                       # the three go together: one missing, two missing
            assert jvp(C.byref(ok), T, *jvp_args(some, **{a: None})) == _lib.E_INVALID
            two = {b: None for b in ("ptape", "params", "t_params") if b != a}
            assert jvp(C.byref(ok), T, *jvp_args(some, **two)) == _lib.E_INVALID
    assert jvp(C.byref(ok), 3, *jvp_args(some, tape=None)) == _lib.E_INVALID
    assert jvp(C.byref(ok), -1, *jvp_args(some)) == _lib.E_INVALID
    for bad in (_lib.MicroDesc(4, 5000, 0.01), _lib.MicroDesc(4, 0, 0.01), _lib.MicroDesc(0, 70, 0.01), _lib.MicroDesc(4, 70, 0.0)):
        assert jvp(C.byref(bad), 3, *jvp_args(some)) == _lib.E_INVALID
        assert plan(C.byref(bad), 3, 1, 0, C.byref(out)) == _lib.E_INVALID
    assert jvp(None, 3, *jvp_args(some)) == _lib.E_INVALID
    assert plan(None, 3, 1, 0, C.byref(out)) == _lib.E_INVALID
    assert plan(C.byref(ok), 3, 1, 0, None) == _lib.E_INVALID
    assert plan(C.byref(ok), 3, 0, 0, C.byref(out)) == _lib.E_INVALID
    assert plan(C.byref(ok), -1, 1, 0, C.byref(out)) == _lib.E_INVALID


def test_the_plan_needs_no_device():
    """One vehicle per thread: the block is the lane rounded up to 64.  Launches of 4, then 2, then 1 directions, a remainder of 3 in one
    launch of 4 with a slot masked, with and without t_params; LDS = two copies of the leader hand-over per direction (8 B a slot,
    V + 1 slots), with t_params two more of the pre-step state, and 16 B of head-gap tangents per direction.  T = 0 launches too (it
    zeroes the slots beyond count)."""
    from dhts import ops
    widest = {1: 1, 2: 2, 3: 4, 4: 4, 5: 4, 6: 4, 7: 4, 8: 4}
    launches = {1: 1, 2: 1, 3: 1, 4: 1, 5: 2, 6: 2, 7: 2, 8: 2}
    for V, block in ((1, 64), (64, 64), (65, 128), (1024, 1024)):
        for K in widest:
            for want_params in (False, True):
                for T in (0, 5):
                    p = ops.micro_jvp_plan(ops.micro_desc(3, V, 0.01), T, K, want_params)
                    lds = 8 * (2 * widest[K] + (2 if want_params else 0)) * (V + 1) + 16 * widest[K]
                    assert p == dict(block=block, dirs_per_launch=widest[K], launches=launches[K], lds_bytes=lds), (V, K, want_params, p)
    assert ops.micro_jvp_plan(ops.micro_desc(1, 1024, 0.01), 5, 4, True)["lds_bytes"] <= 160 * 1024


def test_value_errors_of_the_operator_come_before_anything_touches_a_device():
    import torch
    import dhts
    L, V, T, K = 2, 8, 5, 3
    p0, v0 = torch.zeros(L, V), torch.zeros(L, V)
    par, head = torch.ones(6, L, V, dtype=torch.float64), torch.zeros(L, 2, dtype=torch.float64)
    tp = torch.zeros(K, L, V)
    run = dhts.micro_rollout_jvp
    bad = [
        dict(),                                                       # no tangent at all
        dict(t_p0=torch.zeros(L, V)),                                 # no direction axis
        dict(t_p0=torch.zeros(0, L, V)),                              # K = 0
        dict(t_p0=tp, t_v0=torch.zeros(K + 1, L, V)),                 # two values of K
        dict(t_v0=torch.zeros(K, L, V + 1)),
        dict(t_p0=torch.zeros(K, L + 1, V)),
        dict(t_p0=tp, t_head=torch.zeros(K, L, 3, dtype=torch.float64)),
        dict(t_head=torch.zeros(K, L, dtype=torch.float64)),
        dict(t_p0=tp, t_head=torch.zeros(K + 1, L, 2, dtype=torch.float64)),
        dict(t_params=torch.zeros(K, 5, L, V, dtype=torch.float64)),
        dict(t_params=torch.zeros(K, 6, L, V + 1, dtype=torch.float64)),
        dict(t_p0=tp, t_params=torch.zeros(6, L, V, dtype=torch.float64)),
        dict(t_p0=[[0.0]]),                                           # not a tensor
        dict(t_p0=tp, count=torch.zeros(L + 1, dtype=torch.int32)),
        dict(t_p0=tp, count=torch.zeros(L, dtype=torch.int64)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            run(p0, v0, par, head, T, 0.01, **kw)
    with pytest.raises(ValueError):
        run(p0, torch.zeros(L, V + 1), par, head, T, 0.01, t_p0=tp)
    with pytest.raises(ValueError):
        run(p0, v0, par[:5], head, T, 0.01, t_p0=tp)
    with pytest.raises(ValueError):
        run(p0, v0, par, torch.zeros(L, 3, dtype=torch.float64), T, 0.01, t_p0=tp)
    with pytest.raises(ValueError):
        run(p0, v0, par, head, -1, 0.01, t_p0=tp)
    with pytest.raises(ValueError):
        run(torch.zeros(V), torch.zeros(V), par, head, T, 0.01, t_p0=tp)
    with pytest.raises(TypeError):
        run(p0, v0, par, head, T, 0.01, tp)                           # tangents are keyword-only


# ---- the references ------------------------------------------------------------------------------------------------------------------
_cache = {}


def oracle_run(oracle, shape):
    """The oracle's rollout of a shape, computed once: inputs (tests/test_micro_params_gpu.lanes), tape and history."""
    if shape not in _cache:
        L, V, T, dt, head = shape
        p0, v0, par, _ = lanes(np.random.default_rng(1000 + V), L, V)
        f = oracle.micro_rollout_fwd(p0, v0, np.ascontiguousarray(par.transpose(1, 2, 0)), T, dt, head_dp=head[0], head_dv=head[1],
                                     want_hist=True)
        assert f["rc"] == 0, "the lanes are collision-free in the oracle"
        _cache[shape] = (p0, v0, par, np.tile(np.array([head]), (L, 1)), f)
    return _cache[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_chain_against_the_oracle_adjoint(oracle, shape):
    """<g, J t> with J t from micro_jvp_ref.chain on the oracle's tape against <J^T g, t> with J^T g from the oracle's reverse sweep, for
    random cotangents of the final state and of the state after every step and random tangents of p0, v0 and the head gap: equal within
    TOL_GRAD of the sum of the absolute products of the left side, evaluated in float64."""
    L, V, T, dt, _ = shape
    f = oracle_run(oracle, shape)[4]
    rng = np.random.default_rng(7 + V)
    for trial in range(2):
        g_pT, g_vT = rng.standard_normal((2, L, V)).astype(np.float32)
        gh_p, gh_v = rng.standard_normal((2, T, L, V)).astype(np.float32)
        t_p0, t_v0 = rng.standard_normal((2, L, V)).astype(np.float32)
        t_head = rng.standard_normal((L, 2))
        b = oracle.micro_rollout_bwd(f, g_pT=g_pT, g_vT=g_vT, gh_p=gh_p, gh_v=gh_v)
        lhs = scale = 0.0
        for lane in range(L):
            t_pT, t_vT, t_hist = J.chain(f["tape"][:, lane], t_p0[lane], t_v0[lane], t_head[lane])
            assert np.abs(t_pT).max() > 0 and np.abs(t_vT).max() > 0
            for g, t in ((g_pT[lane], t_pT), (g_vT[lane], t_vT), (gh_p[:, lane], t_hist[:, 0]), (gh_v[:, lane], t_hist[:, 1])):
                prod = g.astype(np.float64) * t.astype(np.float64)
                lhs, scale = lhs + float(prod.sum()), scale + float(np.abs(prod).sum())
        rhs = float((b["g_p0"].astype(np.float64) * t_p0).sum() + (b["g_v0"].astype(np.float64) * t_v0).sum()
                    + (b["g_head"].astype(np.float64) * t_head).sum())
        print("L%d V%d T%d trial %d: <g, J t> = %.9g, <J^T g, t> = %.9g, |d| / sum |products| = %.2e"
              % (L, V, T, trial, lhs, rhs, abs(lhs - rhs) / scale))
        assert abs(lhs - rhs) <= TOL_GRAD * scale


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_chain_against_the_float64_yardstick(oracle, shape):
    """The float32 chain on the oracle's tape against torch.func.jvp of lane_rollout in float64, for a tangent of each of p0, v0 and the
    head gap alone and of all three: TOL_GRAD, norm-relative per output plane (measured: 1.7e-6 or better)."""
    L, V, T, dt, _ = shape
    p0, v0, par, head, f = oracle_run(oracle, shape)
    rng = np.random.default_rng(70 + V)
    t_p0, t_v0 = rng.standard_normal((2, L, V)).astype(np.float32)
    t_head = rng.standard_normal((L, 2))
    zs, zh = np.zeros((L, V), np.float32), np.zeros((L, 2))
    worst = 0.0
    for tag, a, b, c in (("t_p0", t_p0, zs, zh), ("t_v0", zs, t_v0, zh), ("t_head", zs, zs, t_head), ("all", t_p0, t_v0, t_head)):
        y = J.yardstick(p0, v0, par, head, T, dt, t_p0=a, t_v0=b, t_head=c)
        assert max(rel_elem(y["hist"][:, :, 0], f["hist_p"]), rel_elem(y["hist"][:, :, 1], f["hist_v"])) <= TOL_STATE      # one rollout
        got = dict(t_pT=np.zeros((L, V), np.float32), t_vT=np.zeros((L, V), np.float32), t_hist=np.zeros((T, L, 2, V), np.float32))
        for lane in range(L):
            got["t_pT"][lane], got["t_vT"][lane], got["t_hist"][:, lane] = J.chain(f["tape"][:, lane], a[lane], b[lane], c[lane])
        worst = max(worst, J.compare("L%d V%d T%d %s chain vs yardstick" % (L, V, T, tag), got, y, None, TOL_GRAD))
    print("L%d V%d T%d: worst plane %.2e" % (L, V, T, worst))


def test_yardstick_runs_forward_mode_through_ragged_lanes():
    """Forward-mode autograd runs through lane_rollout as it stands, ragged count included: slots at or beyond count pass their tangents
    through, and the live part is the rollout of the shorter lane; a parameter tangent reaches the state."""
    rng = np.random.default_rng(4)
    L, V, T, dt = 3, 9, 12, 0.05
    p0, v0, par, head = lanes(rng, L, V)
    head[1] = (15.0, 2.0)
    count = [9, 4, 0]
    t_p0, t_v0 = rng.standard_normal((2, L, V)).astype(np.float32)
    t_par, t_head = rng.standard_normal((6, L, V)), rng.standard_normal((L, 2))
    y = J.yardstick(p0, v0, par, head, T, dt, count=count, t_p0=t_p0, t_v0=t_v0, t_params=t_par, t_head=t_head)
    live = J.live_mask(L, V, count)
    assert np.array_equal(y["t_pT"][~live], t_p0[~live]) and np.array_equal(y["t_vT"][~live], t_v0[~live])
    s = J.yardstick(p0[1:2, :4], v0[1:2, :4], par[:, 1:2, :4], head[1:2], T, dt, t_p0=t_p0[1:2, :4], t_v0=t_v0[1:2, :4],
                    t_params=t_par[:, 1:2, :4], t_head=t_head[1:2])
    assert np.array_equal(s["t_pT"][0], y["t_pT"][1, :4]) and np.array_equal(s["t_vT"][0], y["t_vT"][1, :4])
    assert np.array_equal(s["t_hist"][:, 0], y["t_hist"][:, 1, :, :4])
    only = J.yardstick(p0, v0, par, head, T, dt, count=count, t_params=t_par)
    assert np.abs(only["t_vT"][0]).min() > 0 and np.all(only["t_vT"][2] == 0)
    # against a central difference of the same function along the same direction (float32 states: a coarse check of the sign and size)
    eps = 1e-3
    up = J.yardstick(p0, v0, par + eps * t_par, head + eps * t_head, T, dt, count=count)
    dn = J.yardstick(p0, v0, par - eps * t_par, head - eps * t_head, T, dt, count=count)
    ph = J.yardstick(p0, v0, par, head, T, dt, count=count, t_params=t_par, t_head=t_head)
    fd = (up["vT"].astype(np.float64) - dn["vT"]) / (2 * eps)
    assert np.max(np.abs(fd - ph["t_vT"])[live]) <= 2e-2 * np.max(np.abs(ph["t_vT"][live]))
