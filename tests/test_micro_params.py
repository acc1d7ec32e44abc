"""Gradient of the fused IDM rollout with respect to the driver parameters: the boundary (header, exports, bindings, argument
checks, the parameter tape's documented size) and the yardstick the GPU sweeps of tests/test_micro_params_gpu.py use -- a float64
torch restatement of the reference's plain MicroLane step (road/lane/_micro_lane.py:131-214 over model/micro/_idm.py:30-49) with
the float32 store per step of the fused kernel, differentiated by plain autograd -- checked against every micro_params_*.npz golden
(the reference's own numbers: tools/gen_goldens.py G6p) and against the C oracle.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from util import TOL_GRAD, TOL_STATE, grad_report, rel_elem, rel_max

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dhts_micro_param_tape_bytes", "dhts_micro_rollout_fwd_params", "dhts_micro_rollout_bwd_params", "dhts_idm_param_jac_batch")
GOLDENS = ("inv10", "rand24", "dense16")
PLANES = ("accel_max", "accel_pref", "target_speed", "min_space", "time_pref", "length")


# =================================================================================================================
# the yardstick
# =================================================================================================================
def lane_rollout(p0, v0, params, head, T, dt, count=None, store32=True):
    """The plain MicroLane's rollout for L lanes at once.  p0, v0 [L][V] float32 torch tensors; params [6][L][V] float64 (accel_max,
    accel_pref, target_speed, min_space, time_pref, length); head [L][2] float64; count [L] integers or None.  Slot i follows slot
    i + 1, slot count - 1 is the head.  Arithmetic in float64, the state stored as float32 after every step (what the fused kernel and
    dMicroLane do; store32=False: the state stays float64 between the steps, as in the plain lane with float64 attribute tensors, and
    is rounded only where it is read).  Returns pT, vT [L][V] float32 and hist [T][L][2][V] float32, all differentiable w.r.t. every input."""
    import torch
    L, V = p0.shape
    n = torch.full((L,), V, dtype=torch.int64) if count is None else torch.as_tensor(count, dtype=torch.int64)
    idx = torch.arange(V)[None, :]
    live, is_head = idx < n[:, None], idx == (n[:, None] - 1)
    a, b, vt, s0, tp, ln = params
    ln_lead = torch.cat([ln[:, 1:], ln[:, -1:]], 1)
    eps, zero = torch.tensor(1e-5, dtype=torch.float64), torch.tensor(0.0, dtype=torch.float64)
    p, v, hist = p0, v0, []
    for _ in range(T):
        pd, vd = p.double(), v.double()
        pl, vl = torch.cat([pd[:, 1:], pd[:, -1:]], 1), torch.cat([vd[:, 1:], vd[:, -1:]], 1)
        gap = torch.where(is_head, head[:, 0:1], (pl - pd).abs() - (ln_lead + ln) * 0.5)        # compute_state_delta, :195-214
        dv = torch.where(is_head, head[:, 1:2], vd - vl)
        hit = gap < 0                                                                            # "Set deltas to 0", :151-160
        gap, dv = torch.where(hit, zero, gap), torch.where(hit, zero, dv)
        gap = torch.where(eps > gap, eps, gap)                                                   # max(gap, POSITION_DELTA_EPS), :166
        s = s0 + vd * tp + (vd * dv) / (2 * (a * b) ** 0.5)                                      # _idm.py:30-41
        s = torch.where(s < 0, zero, s)
        acc = a * (1.0 - (vd / vt) ** 4 - (s / gap) ** 2)
        floor = -vd / dt
        acc = torch.where(acc < floor, floor, acc)                                               # :48-49
        np_, nv_ = pd + dt * vd, vd + dt * acc                                                   # :182-183
        p = torch.where(live, np_.float() if store32 else np_, p)                                # float32 store
        v = torch.where(live, nv_.float() if store32 else nv_, v)
        hist.append(torch.stack([p.float(), v.float()], 1))
    return p.float(), v.float(), (torch.stack(hist) if hist else torch.zeros(0, L, 2, V))


def tap_loss(tap, pT, vT, hist):
    return hist.sum() if tap == "every_sum" else 1e-4 * (pT ** 2).sum() + (vT ** 2).sum()


def restated(p0, v0, params, head, T, dt, tap, count=None, g_pT=None, g_vT=None, g_hist=None, store32=True):
    """Run lane_rollout on numpy inputs and differentiate `tap` (or the given cotangents): dict of numpy arrays."""
    import torch
    tp0 = torch.tensor(np.asarray(p0, np.float32), requires_grad=True)
    tv0 = torch.tensor(np.asarray(v0, np.float32), requires_grad=True)
    tpar = torch.tensor(np.asarray(params, np.float64), requires_grad=True)
    thead = torch.tensor(np.asarray(head, np.float64), requires_grad=True)
    pT, vT, hist = lane_rollout(tp0, tv0, tpar, thead, T, dt, count, store32)
    if tap is None:
        loss = (pT * torch.tensor(g_pT)).sum() + (vT * torch.tensor(g_vT)).sum()
        if g_hist is not None and T > 0:
            loss = loss + (hist * torch.tensor(g_hist)).sum()
    else:
        loss = tap_loss(tap, pT, vT, hist)
    loss.backward()
    z = lambda t: t.grad.numpy() if t.grad is not None else np.zeros(tuple(t.shape))      # noqa: E731
    return dict(pT=pT.detach().numpy(), vT=vT.detach().numpy(), hist=hist.detach().numpy(), loss=float(loss.detach()),
                g_p0=z(tp0), g_v0=z(tv0), g_params=z(tpar), g_head=z(thead))


def per_plane(tag, got, ref):
    """TOL_GRAD norm-relative, plane by plane (the planes differ by three orders of magnitude).  got, ref [6][...]."""
    worst = 0.0
    for k, name in enumerate(PLANES):
        worst = max(worst, grad_report("%s d loss / d %s" % (tag, name), got[k], ref[k]))
    return worst


def golden_case(golden_dir, name):
    g = np.load(os.path.join(golden_dir, "micro_params_%s.npz" % name))
    return dict(p0=g["p0"][None], v0=g["v0"][None], params=np.ascontiguousarray(g["params"].T[:, None, :]), head=g["head"][None],
                T=int(g["T"]), dt=float(g["dt"]), tap=str(g["tap"]), g=g)


@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_reproduces_the_reference(golden_dir, oracle, name):
    """The restatement against the reference's plain MicroLane with float64 attribute tensors (the golden), and its states and state
    gradients against the C oracle (dMicroLane's analytic operator): this is what makes it a yardstick at shapes the reference is too
    slow for.

    The golden's lane stores its state as float32 after every step through the lane's own get_state_vector / set_state_vector, as
    dMicroLane and the fused rollout do (tools/gen_goldens.py G6p); the run whose state stays float64 is kept beside it and has its own
    test below."""
    c = golden_case(golden_dir, name)
    g, T, dt = c["g"], c["T"], c["dt"]
    r = restated(c["p0"], c["v0"], c["params"], c["head"], T, dt, c["tap"])
    V = c["p0"].shape[1]
    f = oracle.micro_rollout_fwd(c["p0"], c["v0"], g["params"][None], T, dt, head_dp=c["head"][0, 0], head_dv=c["head"][0, 1], want_hist=False)
    assert f["rc"] == 0
    e_s = max(rel_elem(r["pT"], f["pT"]), rel_elem(r["vT"], f["vT"]))
    print("%s: restatement vs oracle state %.2e; loss %.9g (golden %.9g)" % (name, e_s, r["loss"], float(g["loss"])))
    assert e_s <= TOL_STATE
    assert max(rel_elem(r["pT"][0], g["pT"]), rel_elem(r["vT"][0], g["vT"])) <= TOL_STATE
    assert abs(r["loss"] - float(g["loss"])) <= TOL_STATE * abs(float(g["loss"]))
    if c["tap"] == "every_sum":
        ones = np.ones((T, 1, V), np.float32)
        b = oracle.micro_rollout_bwd(f, g_pT=np.zeros((1, V), np.float32), g_vT=np.zeros((1, V), np.float32), gh_p=ones, gh_v=ones)
    else:
        b = oracle.micro_rollout_bwd(f, g_pT=np.float32(2e-4) * f["pT"], g_vT=2 * f["vT"])
    assert grad_report("%s restatement vs oracle d loss / d p0" % name, r["g_p0"], b["g_p0"]) <= TOL_GRAD
    assert grad_report("%s restatement vs oracle d loss / d v0" % name, r["g_v0"], b["g_v0"]) <= TOL_GRAD
    assert grad_report("%s restatement vs golden d loss / d p0" % name, r["g_p0"][0], g["g_p0"]) <= TOL_GRAD
    assert grad_report("%s restatement vs golden d loss / d v0" % name, r["g_v0"][0], g["g_v0"]) <= TOL_GRAD
    assert per_plane("%s restatement vs golden" % name, r["g_params"][:, 0, :], g["g_params"].T) <= TOL_GRAD
    assert np.all(np.isfinite(g["g_params"])) and np.all(np.abs(g["g_params"]).max(axis=0) > 0), "every plane has a reference number"


@pytest.mark.parametrize("name", GOLDENS)
def test_float64_state_restatement_is_the_plain_lane(golden_dir, name):
    """The golden's second run, with the lane's state left in float64 between the steps (what float64 attribute tensors promote it to),
    against the same restatement without its float32 store: every parameter plane and both state gradients within TOL_GRAD.  Over
    dense16's 400 steps the two rollouts differ by 1.3e-4 in d loss / d accel_max: the float32 store is part of the rollout that is
    differentiated, so each run is compared with its own restatement."""
    c = golden_case(golden_dir, name)
    g = c["g"]
    r = restated(c["p0"], c["v0"], c["params"], c["head"], c["T"], c["dt"], c["tap"], store32=False)
    assert per_plane("%s float64-state restatement vs golden" % name, r["g_params"][:, 0, :], g["g_params_f64state"].T) <= TOL_GRAD
    assert grad_report("%s float64-state restatement vs golden d loss / d p0" % name, r["g_p0"][0], g["g_p0_f64state"]) <= TOL_GRAD
    assert grad_report("%s float64-state restatement vs golden d loss / d v0" % name, r["g_v0"][0], g["g_v0_f64state"]) <= TOL_GRAD


def test_restatement_masks_and_clips():
    """Slots at or beyond count get exactly 0, the head's gap carries no length, and a step under the acceleration clip holds no
    parameter (the vehicle stops: v' = v + dt (-v / dt))."""
    rng = np.random.default_rng(5)
    L, V, T, dt = 2, 6, 1, 0.1
    p0 = (np.arange(V)[None, :] * 30.0 + rng.uniform(0, 5, (L, V))).astype(np.float32)
    v0 = rng.uniform(5, 10, (L, V)).astype(np.float32)
    params = np.tile(np.array([30.0, 24.0, 27.0, 0.5, 0.1, 5.0])[:, None, None], (1, L, V))
    head = np.array([[1000.0, 0.0], [0.5, 0.0]])           # lane 1: the head vehicle brakes to a stop at once (acceleration clip)
    r = restated(p0, v0, params, head, T, dt, "every_sum", count=[4, 6])
    assert np.all(r["g_params"][:, 0, 4:] == 0)
    assert r["g_params"][5, 0, 3] != 0 and np.all(r["g_params"][:5, 1, 5] == 0)       # head: length through its follower's gap only
    assert r["hist"][0, 1, 1, 5] == 0.0 and np.any(r["g_params"][:5, 1, 4] != 0)


# =================================================================================================================
# the boundary
# =================================================================================================================
def test_header_library_and_bindings_hold_the_new_entry_points():
    from dhts import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dhts.h")).read(), flags=re.S)
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), "include/dhts.h does not declare %s" % name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    n_args = {n: len(_lib.SIGNATURES[n][1]) for n in NEW}
    assert n_args == dict(zip(NEW, (2, 14, 15, 5)))


def test_bad_arguments_are_rejected_without_a_gpu():
    from dhts import _lib
    lib = _lib.lib()
    ok = _lib.MicroDesc(4, 70, 0.01)
    some = C.c_void_p(64)                      # a non-NULL pointer that is never dereferenced: the checks come first
    assert lib.dhts_micro_rollout_fwd_params(C.byref(ok), 1, *([None] * 12)) == _lib.E_INVALID
    args = [some] * 12
    args[8] = None                             # ptape
    assert lib.dhts_micro_rollout_fwd_params(C.byref(ok), 1, *args) == _lib.E_INVALID
    args = [some] * 12
    args[7] = None                             # tape: the reverse sweep reads the acceleration clip off it
    assert lib.dhts_micro_rollout_fwd_params(C.byref(ok), 1, *args) == _lib.E_INVALID
    for missing in (1, 3, 10):                 # ptape, params, g_params
        args = [some] * 13
        args[missing] = None
        assert lib.dhts_micro_rollout_bwd_params(C.byref(ok), 1, *args) == _lib.E_INVALID
    for bad in (_lib.MicroDesc(4, 5000, 0.01), _lib.MicroDesc(0, 70, 0.01), _lib.MicroDesc(4, 70, 0.0)):
        assert lib.dhts_micro_rollout_fwd_params(C.byref(bad), 1, *([some] * 12)) == _lib.E_INVALID
        assert lib.dhts_micro_rollout_bwd_params(C.byref(bad), 1, *([some] * 13)) == _lib.E_INVALID
        assert lib.dhts_micro_param_tape_bytes(C.byref(bad), 10) == 0
    assert lib.dhts_micro_rollout_bwd_params(C.byref(ok), -1, *([some] * 13)) == _lib.E_INVALID
    assert lib.dhts_micro_param_tape_bytes(C.byref(ok), -1) == 0
    assert lib.dhts_idm_param_jac_batch(0, some, some, some, None) == _lib.E_INVALID
    assert lib.dhts_idm_param_jac_batch(8, None, some, some, None) == _lib.E_INVALID
    assert lib.dhts_idm_param_jac_batch(8, some, None, some, None) == _lib.E_INVALID
    assert lib.dhts_idm_param_jac_batch(8, some, some, None, None) == _lib.E_INVALID


@pytest.mark.parametrize("L,V,T", [(4096, 256, 1000), (1, 1, 1), (5, 65, 7), (3, 1024, 0), (7, 300, 50)])
def test_param_tape_bytes_match_the_documented_layout(L, V, T):
    """include/dhts.h: 64 B header | head gaps [L][2] double rounded up to whole 64 B | 8 B per vehicle-step over [T][L][Vp]; the
    plan reports the 8 in plan[5], and the existing tape keeps its 12."""
    from dhts import _lib
    lib = _lib.lib()
    d = _lib.MicroDesc(L, V, 0.01)
    Vp = (V + 63) // 64 * 64
    assert lib.dhts_micro_param_tape_bytes(C.byref(d), T) == 64 + (16 * L + 63) // 64 * 64 + 8 * T * L * Vp
    assert lib.dhts_micro_tape_bytes(C.byref(d), T) == 12 * T * L * Vp
    plan = (C.c_int32 * 8)()
    assert lib.dhts_micro_rollout_plan(C.byref(d), T, 0, C.byref(plan)) == 0
    assert plan[5] == 8 and plan[6] == Vp and plan[7] == 0
    doc = open(os.path.join(ROOT, "include", "dhts.h")).read()
    assert "8 bytes per vehicle-step" in doc
