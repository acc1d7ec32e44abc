"""Time-varying boundary cells of the fused ARZ rollout (dhts_macro_rollout_fwd_sched / _bwd_sched): the yardstick of
tests/test_macro_sched_gpu.py -- the chained oracle of tests/macro_sched_ref.py -- against the reference's own numbers
(tests/golden/macro_sched_*.npz, tools/gen_goldens.py G4s) and against the oracle's constant-boundary rollout, and the boundary of the
library: header, bindings, exports, argument checks.  No GPU needed."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import macro_sched_ref as R
from util import TOL_GRAD, TOL_STATE, grad_report, meta_of, state_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dhts_macro_rollout_fwd_sched", "dhts_macro_rollout_bwd_sched")
GOLDENS = sorted(os.path.basename(p)[len("macro_sched_"):-len(".npz")]
                 for p in glob.glob(os.path.join(ROOT, "tests", "golden", "macro_sched_*.npz")))


def test_the_three_goldens_are_there():
    assert GOLDENS == ["pulse64", "sanity", "small"]


@pytest.mark.parametrize("name", GOLDENS)
def test_chained_oracle_reproduces_the_reference(golden_dir, oracle, name):
    g = np.load(os.path.join(golden_dir, "macro_sched_%s.npz" % name))
    m = meta_of(g)
    T, N = m["T"], m["N"]
    assert g["ghost_r"].shape == (T, 2) and g["g_ghost_r"].shape == (T, 2) and g["r0"].shape == (N,)
    f = R.sched_fwd(oracle, g["r0"][None], g["u0"][None], g["ghost_r"][:, None], g["ghost_u"][:, None], m["dt"], m["dx"], m["u_max"])
    b = R.sched_bwd(oracle, f, **R.taps(f, m["tap"]))
    for k in ("rT", "yT", "uT"):
        assert state_report("%s %s" % (name, k), f[k][0], g[k]) <= TOL_STATE
    n = g["steps_r"].shape[0]
    assert n >= 1
    for k, h in (("steps_r", "hist_r"), ("steps_y", "hist_y"), ("steps_u", "hist_u")):
        assert state_report("%s %s" % (name, k), f[h][:n, 0], g[k]) <= TOL_STATE
    loss = float((f["rT"].astype(np.float64) ** 2).sum() + (f["uT"].astype(np.float64) ** 2).sum()) if m["tap"] == "final_sq" else \
        float(sum(f[h].astype(np.float64).sum() for h in ("hist_r", "hist_y", "hist_u")))
    assert abs(loss - float(g["loss"])) <= TOL_STATE * abs(float(g["loss"]))
    assert grad_report("%s g_r0" % name, b["g_r0"][0], g["g_r0"]) <= TOL_GRAD
    assert grad_report("%s g_u0" % name, b["g_u0"][0], g["g_u0"]) <= TOL_GRAD
    assert grad_report("%s g_ghost_r" % name, b["g_ghost_r"][:, 0], g["g_ghost_r"]) <= TOL_GRAD
    assert grad_report("%s g_ghost_u" % name, b["g_ghost_u"][:, 0], g["g_ghost_u"]) <= TOL_GRAD


@pytest.mark.parametrize("tap", ["final_sq", "every_sum"])
def test_constant_schedule_is_the_constant_boundary_rollout(oracle, tap):
    rng = np.random.default_rng(5)
    L, N, T, dt, dx, um = 2, 37, 25, 0.01, 5.0, 30.0
    r0 = rng.uniform(0.05, 0.95, (L, N)).astype(np.float32)
    u0 = rng.uniform(0.0, um, (L, N)).astype(np.float32)
    gr = rng.uniform(0.05, 0.95, (L, 2)).astype(np.float32)
    gu = rng.uniform(0.0, um, (L, 2)).astype(np.float32)
    of = oracle.macro_rollout_fwd(r0, u0, gr, gu, T, dt, dx, um, want_hist=True)
    f = R.sched_fwd(oracle, r0, u0, np.tile(gr[None], (T, 1, 1)), np.tile(gu[None], (T, 1, 1)), dt, dx, um)
    for k in ("rT", "yT", "uT", "hist_r", "hist_y", "hist_u"):
        assert np.array_equal(f[k], of[k]), k
    if tap == "final_sq":
        ob = oracle.macro_rollout_bwd(of, g_rT=2 * of["rT"], g_uT=2 * of["uT"])
    else:
        one = np.ones((T, L, N), np.float32)
        ob = oracle.macro_rollout_bwd(of, gh_r=one, gh_y=one, gh_u=one)
    b = R.sched_bwd(oracle, f, **R.taps(f, tap))
    assert grad_report("g_r0", b["g_r0"], ob["g_r0"]) <= TOL_GRAD
    assert grad_report("g_u0", b["g_u0"], ob["g_u0"]) <= TOL_GRAD
    # the per-step boundary cotangents, summed in float64, are the rollout's boundary gradient
    s_r, s_u = R.boundary_ry_to_ru(b["g_ghost_ry"].sum(axis=0), gr, gu, um)
    assert grad_report("sum_t g_ghost_r", s_r, ob["g_ghost_r"]) <= TOL_GRAD
    assert grad_report("sum_t g_ghost_u", s_u, ob["g_ghost_u"]) <= TOL_GRAD
    # (the (r, y) -> (r, u) formula is linear in the cotangent: per step and summed is the same thing up to float32 rounding)
    assert grad_report("sum_t of the per-step leaves", b["g_ghost_r"].astype(np.float64).sum(axis=0), ob["g_ghost_r"]) <= TOL_GRAD


def test_header_library_and_bindings_hold_the_new_entry_points():
    from dhts import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dhts.h")).read(), flags=re.S)
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), "include/dhts.h does not declare %s" % name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    # beside the constant-boundary pair, argument for argument
    assert _lib.SIGNATURES[NEW[0]] == _lib.SIGNATURES["dhts_macro_rollout_fwd"]
    assert _lib.SIGNATURES[NEW[1]] == _lib.SIGNATURES["dhts_macro_rollout_bwd"]
    assert len(_lib.SIGNATURES[NEW[0]][1]) == 15 and len(_lib.SIGNATURES[NEW[1]][1]) == 11


def test_bad_arguments_are_rejected_without_a_gpu():
    from dhts import _lib
    lib = _lib.lib()
    ok = _lib.MacroDesc(n_lanes=4, n_cells=128, dt=0.01, dx=5.0, u_max=30.0)
    some = C.c_void_p(64)                      # a non-NULL pointer that is never dereferenced: the checks come first
    assert lib.dhts_macro_rollout_fwd_sched(C.byref(ok), 3, *([None] * 13)) == _lib.E_INVALID
    assert lib.dhts_macro_rollout_bwd_sched(C.byref(ok), 3, *([None] * 9)) == _lib.E_INVALID
    for T in (0, 3):
        args = [some] * 13
        args[4] = None                         # ghost_sched
        assert lib.dhts_macro_rollout_fwd_sched(C.byref(ok), T, *args) == _lib.E_INVALID
        args = [some] * 9
        args[6] = None                         # g_ghost_sched (optional in dhts_macro_rollout_bwd, required here)
        assert lib.dhts_macro_rollout_bwd_sched(C.byref(ok), T, *args) == _lib.E_INVALID
    for missing in (0, 3, 5, 8):               # r, ueq, r_out, ueq_out
        args = [some] * 13
        args[missing] = None
        assert lib.dhts_macro_rollout_fwd_sched(C.byref(ok), 3, *args) == _lib.E_INVALID
    for missing in (0, 1, 4):                  # tape (T > 0), g_r, g_r_out
        args = [some] * 9
        args[missing] = None
        assert lib.dhts_macro_rollout_bwd_sched(C.byref(ok), 3, *args) == _lib.E_INVALID
    bads = (_lib.MacroDesc(n_lanes=0, n_cells=128, dt=0.01, dx=5.0, u_max=30.0),
            _lib.MacroDesc(n_lanes=4, n_cells=0, dt=0.01, dx=5.0, u_max=30.0),
            _lib.MacroDesc(n_lanes=4, n_cells=_lib.MACRO_MAX_CELLS + 1, dt=0.01, dx=5.0, u_max=30.0),
            _lib.MacroDesc(n_lanes=4, n_cells=128, dt=0.0, dx=5.0, u_max=30.0),
            _lib.MacroDesc(n_lanes=4, n_cells=128, dt=0.01, dx=5.0, u_max=-1.0))
    for bad in bads:
        assert lib.dhts_macro_rollout_fwd_sched(C.byref(bad), 3, *([some] * 13)) == _lib.E_INVALID
        assert lib.dhts_macro_rollout_bwd_sched(C.byref(bad), 3, *([some] * 9)) == _lib.E_INVALID
    assert lib.dhts_macro_rollout_fwd_sched(None, 3, *([some] * 13)) == _lib.E_INVALID
    assert lib.dhts_macro_rollout_bwd_sched(None, 3, *([some] * 9)) == _lib.E_INVALID
    assert lib.dhts_macro_rollout_fwd_sched(C.byref(ok), -1, *([some] * 13)) == _lib.E_INVALID
    assert lib.dhts_macro_rollout_bwd_sched(C.byref(ok), -1, *([some] * 9)) == _lib.E_INVALID


def test_shape_errors_of_the_operator_need_no_gpu():
    """dhts.macro_rollout: mixed ranks and a first dimension other than T are ValueErrors, raised before anything touches a device."""
    import torch
    import dhts
    r0, u0 = torch.zeros(2, 8), torch.zeros(2, 8)
    with pytest.raises(ValueError):
        dhts.macro_rollout(r0, u0, torch.zeros(5, 2, 2), torch.zeros(2, 2), 5, 0.01, 5.0, 30.0)
    with pytest.raises(ValueError):
        dhts.macro_rollout(r0, u0, torch.zeros(2, 2), torch.zeros(5, 2, 2), 5, 0.01, 5.0, 30.0)
    with pytest.raises(ValueError):
        dhts.macro_rollout(r0, u0, torch.zeros(4, 2, 2), torch.zeros(4, 2, 2), 5, 0.01, 5.0, 30.0)
    with pytest.raises(ValueError):
        dhts.macro_rollout(r0, u0, torch.zeros(5, 3, 2), torch.zeros(5, 3, 2), 5, 0.01, 5.0, 30.0)


def _t0_move(monkeypatch, oracle, u_hi):
    """How far one ulp of x ** -0.5 moves g_r0 of the final_sq tap at T = 0 (norm-relative, the larger of one ulp up and one ulp down)."""
    rng = np.random.default_rng(64)
    L, N, um = 4, 128, 30.0
    r0 = rng.uniform(0.05, 0.95, (L, N)).astype(np.float32)
    u0 = rng.uniform(0.0, u_hi, (L, N)).astype(np.float32)
    none = np.zeros((0, L, 2), np.float32)
    f = R.sched_fwd(oracle, r0, u0, none, none, 0.01, 5.0, um)
    base = R.sched_bwd(oracle, f, **R.taps(f, "final_sq"))["g_r0"]
    plain, move = R.rsqrt, 0.0
    for to in (np.float32(np.inf), np.float32(0)):
        monkeypatch.setattr(R, "rsqrt", lambda t: np.nextafter(plain(t), to))
        g = R.sched_bwd(oracle, f, **R.taps(f, "final_sq"))["g_r0"]
        move = max(move, float(np.max(np.abs(g.astype(np.float64) - base)) / np.max(np.abs(base))))
    monkeypatch.setattr(R, "rsqrt", plain)
    return move


def test_why_the_t0_cases_of_the_gpu_tests_start_slow(monkeypatch, oracle):
    """At T = 0 the final_sq tap's g_r0 is 2 r0 (at most 1.9) plus float32 terms that cancel in pairs: the pow backward of u_eq in the
    speed tap and again in from_r_u, each u_max g_u / (2 sqrt(r)) = 30 u / sqrt(r), up to 4000 at u = 30 and r = 0.05, and the division's
    backward against from_r_u's product, each 2 u |u - u_eq| / r, up to 8000.  One float32 ulp at 4000 is 2.4e-4 = 1.3e-4 of max |g|.
    x ** -0.5 is the one operation there that faithful float32 evaluations round differently (powf in the oracle, 1 / sqrtf on the
    device), so over the full speed range the reference's own g_r0 is not defined to TOL_GRAD at T = 0: one ulp of it moves g_r0 by
    more.  With u0 <= 0.25 every term stays below 2 * 0.25 * 23.3 / 0.05 = 233, one ulp is 1.5e-5, and a few flipped roundings stay
    far inside the bound.  tests/test_macro_sched_gpu.py draws the speeds of its two T = 0 cases from that range.  After one step or
    more the terms no longer cancel, max |g| is of their size, and the full range is used."""
    full, slow = _t0_move(monkeypatch, oracle, 30.0), _t0_move(monkeypatch, oracle, 0.25)
    print("T = 0, one ulp of x ** -0.5: g_r0 moves by %.2e of max |g| with u0 in [0, 30], by %.2e with u0 in [0, 0.25]" % (full, slow))
    assert full > TOL_GRAD
    assert slow <= TOL_GRAD / 4
