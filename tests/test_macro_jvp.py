"""Forward-mode tangent sweep of the fused ARZ rollout (dhts_macro_rollout_jvp / dhts_macro_jvp_plan / the two glue entry points and
dhts.macro_rollout_jvp): the boundary of the library -- header, bindings, exports, argument checks, the operator's ValueErrors, the new
option -- and the yardstick of tests/test_macro_jvp_gpu.py, the float64 chain of tests/macro_jvp_ref.py, held against the pinned oracle
adjoint by the dot-product identity <g, J t> = <J^T g, t>.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import macro_jvp_ref as J
import macro_sched_ref as R
from util import TOL_GRAD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dhts_macro_rollout_jvp", "dhts_macro_jvp_plan", "dhts_macro_state_from_ru_jvp", "dhts_macro_u_tap_jvp")
DT, DX, UM = 0.01, 5.0, 30.0


def test_header_library_and_bindings_hold_the_new_entry_points():
    import dhts
    from dhts import _lib, ops
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dhts.h")).read(), flags=re.S)
    lib = _lib.lib()
    for name in NEW:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, txt)
        assert m, "include/dhts.h does not declare %s" % name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
        assert len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name          # the header's argument count
    assert len(_lib.SIGNATURES[NEW[0]][1]) == 15 and len(_lib.SIGNATURES[NEW[1]][1]) == 5
    assert len(_lib.SIGNATURES[NEW[2]][1]) == 8 and len(_lib.SIGNATURES[NEW[3]][1]) == 8
    assert re.search(r"#define\s+DHTS_OPT_MACRO_JVP_VARIANT\s+11\b", txt) and _lib.OPT_MACRO_JVP_VARIANT == 11      # (10 stays unknown)
    assert lib.dhts_version() == 100
    for name in ("macro_rollout_jvp", "macro_jvp_plan", "macro_state_from_ru_jvp", "macro_u_tap_jvp"):
        assert callable(getattr(ops, name))
    assert callable(dhts.macro_rollout_jvp) and dhts.macro_rollout_jvp is not ops.macro_rollout_jvp


def jvp_args(some, **kw):
    """(tape, n_dir, t_r, t_y, t_ghost, ghost_is_sched, t_r_out, t_y_out, det, n_det, t_taps, err, stream)"""
    a = dict(tape=some, n_dir=3, t_r=some, t_y=some, t_ghost=some, ghost_is_sched=0, t_r_out=some, t_y_out=some, det=some, n_det=4,
             t_taps=some, err=some, stream=None)
    a.update(kw)
    return list(a.values())


def test_bad_arguments_are_rejected_without_a_gpu():
    from dhts import _lib
    lib = _lib.lib()
    N = 128
    ok = _lib.MacroDesc(n_lanes=4, n_cells=N, dt=0.01, dx=5.0, u_max=30.0)
    some = C.c_void_p(64)                      # a non-NULL pointer that is never dereferenced: the checks come first
    jvp, plan = lib.dhts_macro_rollout_jvp, lib.dhts_macro_jvp_plan
    out = (C.c_int32 * 8)()
    for T in (0, 3):
        for sched in (0, 1):
            for n_dir in (0, -2):
                assert jvp(C.byref(ok), T, *jvp_args(some, n_dir=n_dir, ghost_is_sched=sched)) == _lib.E_INVALID
            for missing in ("t_r", "t_y", "t_r_out", "t_y_out"):
                assert jvp(C.byref(ok), T, *jvp_args(some, ghost_is_sched=sched, **{missing: None})) == _lib.E_INVALID
            assert jvp(C.byref(ok), T, *jvp_args(some, det=None, ghost_is_sched=sched)) == _lib.E_INVALID         # t_taps without det
            assert jvp(C.byref(ok), T, *jvp_args(some, t_taps=None, ghost_is_sched=sched)) == _lib.E_INVALID      # det without t_taps
            for n_det in (0, -1, N + 1):
                assert jvp(C.byref(ok), T, *jvp_args(some, n_det=n_det, ghost_is_sched=sched)) == _lib.E_INVALID
        assert jvp(C.byref(ok), T, *jvp_args(some, t_ghost=None, ghost_is_sched=1)) == _lib.E_INVALID             # a schedule that is not there
    assert jvp(C.byref(ok), 3, *jvp_args(some, tape=None)) == _lib.E_INVALID
    assert jvp(C.byref(ok), -1, *jvp_args(some)) == _lib.E_INVALID
    bads = (_lib.MacroDesc(n_lanes=0, n_cells=N, dt=0.01, dx=5.0, u_max=30.0),
            _lib.MacroDesc(n_lanes=4, n_cells=0, dt=0.01, dx=5.0, u_max=30.0),
            _lib.MacroDesc(n_lanes=4, n_cells=_lib.MACRO_MAX_CELLS + 1, dt=0.01, dx=5.0, u_max=30.0),
            _lib.MacroDesc(n_lanes=4, n_cells=N, dt=0.0, dx=5.0, u_max=30.0),
            _lib.MacroDesc(n_lanes=4, n_cells=N, dt=0.01, dx=5.0, u_max=-1.0))
    for bad in bads:
        assert jvp(C.byref(bad), 3, *jvp_args(some)) == _lib.E_INVALID
        assert plan(C.byref(bad), 3, 1, 1, C.byref(out)) == _lib.E_INVALID
    assert jvp(None, 3, *jvp_args(some)) == _lib.E_INVALID
    assert plan(None, 3, 1, 1, C.byref(out)) == _lib.E_INVALID
    assert plan(C.byref(ok), 3, 1, 1, None) == _lib.E_INVALID
    assert plan(C.byref(ok), 3, 0, 1, C.byref(out)) == _lib.E_INVALID
    assert plan(C.byref(ok), -1, 1, 1, C.byref(out)) == _lib.E_INVALID
    for n_det in (-1, N + 1):
        assert plan(C.byref(ok), 3, 1, n_det, C.byref(out)) == _lib.E_INVALID
    for glue in (lib.dhts_macro_state_from_ru_jvp, lib.dhts_macro_u_tap_jvp):
        assert glue(-1, 30.0, some, some, some, some, some, None) == _lib.E_INVALID
        for i in range(5):
            a = [some] * 5
            a[i] = None
            assert glue(8, 30.0, *a, None) == _lib.E_INVALID
        assert glue(0, 30.0, some, some, some, some, some, None) == _lib.OK       # nothing to do, nothing dereferenced


def test_the_new_option_takes_0_and_1():
    from dhts import _lib
    lib = _lib.lib()
    try:
        assert lib.dhts_set_option(_lib.OPT_MACRO_JVP_VARIANT, 1) == _lib.OK
        assert lib.dhts_set_option(_lib.OPT_MACRO_JVP_VARIANT, 2) == _lib.E_INVALID
        assert lib.dhts_set_option(_lib.OPT_MACRO_JVP_VARIANT, -1) == _lib.E_INVALID
    finally:
        assert lib.dhts_set_option(_lib.OPT_MACRO_JVP_VARIANT, 0) == _lib.OK
    assert lib.dhts_set_option(99, 0) == _lib.E_INVALID and lib.dhts_set_option(10, 0) == _lib.E_INVALID


def test_the_plan_needs_no_device():
    """Launches of 4, then 2, then 1 directions, a remainder of 3 in one launch of 4 with a slot masked; the fast kernel for 2 .. 1024 cells and T > 0; the option forces the general kernel;
    lanes too long for four directions' planes in 160 KB of LDS take two per launch."""
    from dhts import _lib, ops
    widest = {1: 1, 2: 2, 3: 4, 4: 4, 5: 4, 6: 4, 7: 4}
    launches = {1: 1, 2: 1, 3: 1, 4: 1, 5: 2, 6: 2, 7: 2}
    for N, block in ((2, 64), (64, 64), (65, 128), (128, 128), (300, 512), (512, 512), (1000, 1024), (1024, 1024)):
        for K in widest:
            p = ops.macro_jvp_plan(ops.macro_desc(3, N, DT, DX, UM), 5, K, 1)
            assert p == dict(kernel=1, block=block, dirs_per_launch=widest[K], launches=launches[K]), (N, K, p)
    for N, block in ((1, 64), (1025, 512), (1026, 512), (2100, 512)):
        p = ops.macro_jvp_plan(ops.macro_desc(3, N, DT, DX, UM), 5, 5)
        assert p == dict(kernel=0, block=block, dirs_per_launch=4, launches=2), (N, p)
    p = ops.macro_jvp_plan(ops.macro_desc(1, 4000, DT, DX, UM), 5, 5)
    assert p == dict(kernel=0, block=512, dirs_per_launch=2, launches=3), p
    p = ops.macro_jvp_plan(ops.macro_desc(2, 64, DT, DX, UM), 0, 3)
    assert p["kernel"] == 0 and p["launches"] == 0, p
    try:
        assert _lib.lib().dhts_set_option(_lib.OPT_MACRO_JVP_VARIANT, 1) == 0
        p = ops.macro_jvp_plan(ops.macro_desc(3, 300, DT, DX, UM), 5, 4)
        assert p == dict(kernel=0, block=320, dirs_per_launch=4, launches=1), p
    finally:
        _lib.lib().dhts_set_option(_lib.OPT_MACRO_JVP_VARIANT, 0)


def test_value_errors_of_the_operator_come_before_anything_touches_a_device():
    import torch
    import dhts
    L, N, T, K = 2, 8, 5, 3
    r0, u0, g, gs = torch.zeros(L, N), torch.zeros(L, N), torch.zeros(L, 2), torch.zeros(T, L, 2)
    tr, tg, tgs = torch.zeros(K, L, N), torch.zeros(K, L, 2), torch.zeros(K, T, L, 2)
    run = dhts.macro_rollout_jvp
    bad = [
        dict(),                                                       # no tangent at all
        dict(t_r0=torch.zeros(L, N)),                                 # no direction axis
        dict(t_r0=torch.zeros(0, L, N)),                              # K = 0
        dict(t_r0=tr, t_u0=torch.zeros(K + 1, L, N)),                 # two values of K
        dict(t_r0=torch.zeros(K, L, N + 1)),
        dict(t_r0=tr, t_ghost_r=tgs),                                 # a schedule of tangents at constant boundary cells
        dict(t_ghost_u=torch.zeros(K, L, 3)),
        dict(t_r0=tr, t_ghost_r=torch.zeros(K + 1, L, 2)),
        dict(t_r0=tr, detectors=[3, 2]),
        dict(t_r0=tr, detectors=[0, N]),
        dict(t_r0=tr, detectors=[]),
        dict(t_r0=[[0.0]]),                                           # not a tensor
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            run(r0, u0, g, g, T, DT, DX, UM, **kw)
    for kw in (dict(t_r0=tr, t_ghost_r=tg), dict(t_ghost_u=torch.zeros(K, T + 1, L, 2)), dict(t_ghost_r=torch.zeros(K, L, 2, 2))):
        with pytest.raises(ValueError):                               # constant tangents at a schedule; a schedule of another length
            run(r0, u0, gs, gs, T, DT, DX, UM, **kw)
    with pytest.raises(ValueError):
        run(r0, u0, g, gs, T, DT, DX, UM, t_r0=tr)                    # the two boundary planes in two forms
    with pytest.raises(ValueError):
        run(r0, torch.zeros(L, N + 1), g, g, T, DT, DX, UM, t_r0=tr)
    with pytest.raises(TypeError):
        run(r0, u0, g, g, T, DT, DX, UM, tr)                          # tangents are keyword-only


# ---- the reference chain against the pinned adjoint -----------------------------------------------------------------------------------
class Recorder:
    """The oracle with the Riemann case of every interface of every step on record (macro_sched_ref.sched_fwd keeps the blocks only)."""

    def __init__(self, O):
        self.O, self.cases = O, []

    def macro_step(self, *a, **kw):
        o = self.O.macro_step(*a, **kw)
        self.cases.append(o["case"].copy())
        return o

    def macro_step_bwd(self, *a, **kw):
        return self.O.macro_step_bwd(*a, **kw)


def inputs(L, N, T, seed):
    """tests/test_macro_sched_gpu.py's recipe: random state and independent random boundary cells per step, on some steps a boundary
    density below 1e-5 or exactly 0 (the solver's vacuum branches); one more row drawn behind the schedule for the constant form."""
    rng = np.random.default_rng(seed)
    r0 = rng.uniform(0.05, 0.95, (L, N)).astype(np.float32)
    u0 = rng.uniform(0.0, UM, (L, N)).astype(np.float32)
    gr = rng.uniform(0.05, 0.95, (T, L, 2)).astype(np.float32)
    gu = rng.uniform(0.0, UM, (T, L, 2)).astype(np.float32)
    if T >= 2:
        gr[T // 2, 0, 0] = 3e-6
        gr[T - 1, L - 1, 1] = 0.0
        gr[0, 0, 1] = 8e-6
    cr = rng.uniform(0.05, 0.95, (L, 2)).astype(np.float32)
    cu = rng.uniform(0.0, UM, (L, 2)).astype(np.float32)
    return r0, u0, gr, gu, cr, cu


SHAPES = {(2, 1, 6): 11, (2, 2, 7): 12, (2, 65, 10): 13}           # (L, N, T): seed


@pytest.mark.parametrize("sched", [False, True], ids=["const", "sched"])
@pytest.mark.parametrize("shape", sorted(SHAPES), ids=lambda s: "L%d_N%d_T%d" % s)
def test_reference_chain_against_the_oracle_adjoint(oracle, shape, sched):
    """<g, J t> with J t from macro_jvp_ref against <J^T g, t> with J^T g from macro_sched_ref.sched_bwd, for random cotangents g of the
    final (r, y, u) and of (r, y, u) after every step and random tangents t of all four leaves: equal within TOL_GRAD of the sum of the
    absolute products of the left side.  A constant boundary is the same row in front of every step: its tangent is repeated, its
    cotangent summed over the steps."""
    L, N, T = shape
    r0, u0, gr, gu, cr, cu = inputs(L, N, T, SHAPES[shape])
    if not sched:
        gr, gu = np.tile(cr[None], (T, 1, 1)), np.tile(cu[None], (T, 1, 1))
    rec = Recorder(oracle)
    f = R.sched_fwd(rec, r0, u0, gr, gu, DT, DX, UM)
    cases = np.concatenate(rec.cases)
    assert len(rec.cases) == L * T and (cases == 0).any() and (cases != 0).any(), "one trivial and one non-trivial interface at least"
    rng = np.random.default_rng(100 + SHAPES[shape])
    det = list(range(N))
    for trial in range(3):
        g_fin = rng.standard_normal((3, L, N)).astype(np.float32)
        g_hist = rng.standard_normal((3, T, L, N)).astype(np.float32)
        t_r0, t_u0 = rng.standard_normal((2, L, N))
        t_g = rng.standard_normal((2, L, 2)) if not sched else rng.standard_normal((2, T, L, 2))
        t_gr, t_gu = (np.tile(t_g[:, None], (1, T, 1, 1)) if not sched else t_g)
        b = R.sched_bwd(oracle, f, g_rT=g_fin[0], g_yT=g_fin[1], g_uT=g_fin[2], gh_r=g_hist[0], gh_y=g_hist[1], gh_u=g_hist[2])
        o = J.jvp(f, t_r0=t_r0, t_u0=t_u0, t_gr=t_gr, t_gu=t_gu, det=det)
        assert max(np.abs(o[k]).max() for k in ("t_rT", "t_yT", "t_uT")) > 0 and np.abs(o["t_read"]).max() > 0
        left = [g_fin[0].astype(np.float64) * o["t_rT"], g_fin[1].astype(np.float64) * o["t_yT"], g_fin[2].astype(np.float64) * o["t_uT"],
                g_hist.astype(np.float64).transpose(1, 2, 0, 3) * o["t_read"]]
        right = [b["g_r0"].astype(np.float64) * t_r0, b["g_u0"].astype(np.float64) * t_u0,
                 b["g_ghost_r"].astype(np.float64) * t_gr, b["g_ghost_u"].astype(np.float64) * t_gu]
        lhs, rhs = sum(float(x.sum()) for x in left), sum(float(x.sum()) for x in right)
        scale = sum(float(np.abs(x).sum()) for x in left)
        print("L%d N%d T%d %s trial %d: <g, J t> = %.9g, <J^T g, t> = %.9g, |d| / sum |products| = %.2e"
              % (L, N, T, "sched" if sched else "const", trial, lhs, rhs, abs(lhs - rhs) / scale))
        assert abs(lhs - rhs) <= TOL_GRAD * scale
