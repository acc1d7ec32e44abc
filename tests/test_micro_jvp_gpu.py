"""Forward-mode tangent sweep of the fused IDM rollout on the device: dhts.micro_rollout_jvp and the raw dhts_micro_rollout_jvp against
the float64 yardstick and the numpy chain of tests/micro_jvp_ref.py (both checked on the CPU in tests/test_micro_jvp.py), against the
device's own reverse sweep by the dot-product identity, and against itself: bit-identity across K, slots, runs and lane order, exact
zeros, guard bands, the fault records.  Needs a real MI355X: python -m pytest tests -m gpu"""
import os
import subprocess
import sys

import numpy as np
import pytest

import micro_jvp_ref as J
from test_micro_params_gpu import lanes
from util import TOL_GRAD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.02
HEADS = ((1000.0, 0.0), (15.0, 2.0), (0.5, 0.0))       # free road; car following; under the acceleration clip (the head stops at once)
# (L, V, T, count): wavefront edges, several wavefronts per lane, the largest block; T below the prefetch depth, odd and even (the LDS
# parity); ragged counts with 0, 1 and V.  Lane l takes head gap l mod 3; the rollouts of 50 steps keep to the first two (a lane that
# queues up behind a stopped head for a second sits on the kinks of the clip, where the float64 yardstick is no yardstick).
CASES = [(3, 1, 3, None), (3, 2, 7, [2, 1, 0]), (4, 63, 2, None), (3, 64, 50, [64, 0, 33]), (3, 65, 1, [65, 1, 64]),
         (5, 130, 50, [130, 0, 77, 1, 64]), (3, 300, 7, None), (3, 1024, 20, [1024, 513, 0]), (3, 70, 0, [70, 0, 5])]
IDS = ["L%d_V%d_T%d%s" % (c[0], c[1], c[2], "" if c[3] is None else "_ragged") for c in CASES]
LEAVES = ("t_p0", "t_v0", "t_head", "t_params")


def case_inputs(case):
    L, V, T, count = case
    rng = np.random.default_rng(31 * V + T)
    p0, v0, par, head = lanes(rng, L, V)
    for lane in range(L):
        head[lane] = HEADS[lane % (3 if T <= 7 else 2)]
        stop_head(par, head, lane, V if count is None else count[lane])
    t = dict(t_p0=rng.standard_normal((L, V)).astype(np.float32), t_v0=rng.standard_normal((L, V)).astype(np.float32),
             t_head=rng.standard_normal((L, 2)), t_params=rng.standard_normal((6, L, V)))
    return p0, v0, par, head, t


def stop_head(par, head, lane, n):
    """A lane with the head gap (0.5, 0): its head vehicle keeps 5 m + 1.5 s of headway, so that its desired spacing is at least 37 times
    the gap and its braking, a (1 - (s / gap)^2) < -1000 a, is below the clip's floor -v / dt at every speed and step size used here."""
    if n > 0 and tuple(head[lane]) == HEADS[2]:
        par[3, lane, n - 1], par[4, lane, n - 1] = 5.0, 1.5


def directions(t, names):
    """One direction per name (that leaf's tangent alone, the others zero), then all of them together: dict name -> [K][...]."""
    K = len(names) + 1
    out = {}
    for n in names:
        a = np.zeros((K,) + t[n].shape, t[n].dtype)
        a[names.index(n)] = t[n]
        a[K - 1] = t[n]
        out[n] = a
    return out


def device_jvp(cuda, p0, v0, par, head, T, dt, count=None, want_hist=False, check_faults=True, **tang):
    import torch
    import dhts
    dt64 = {"t_head": torch.float64, "t_params": torch.float64}
    kw = {n: torch.tensor(a, device=cuda, dtype=dt64.get(n, torch.float32)) for n, a in tang.items() if a is not None}
    cnt = None if count is None else torch.tensor(count, device=cuda, dtype=torch.int32)
    prim, tan = dhts.micro_rollout_jvp(torch.tensor(p0, device=cuda), torch.tensor(v0, device=cuda),
                                       torch.tensor(par, device=cuda, dtype=torch.float64), torch.tensor(head, device=cuda, dtype=torch.float64),
                                       T, dt, count=cnt, want_hist=want_hist, check_faults=check_faults, **kw)
    torch.cuda.synchronize()
    assert all(not x.requires_grad and x.grad_fn is None for x in prim + tan), "no autograd graph is recorded"
    n = lambda x: x.cpu().numpy()      # noqa: E731
    return dict(pT=n(prim[0]), vT=n(prim[1]), hist=n(prim[2]) if want_hist else None,
                t_pT=n(tan[0]), t_vT=n(tan[1]), t_hist=n(tan[2]) if want_hist else None)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


_yard = {}


def yard(case, names):
    """The yardstick's directions of a case, computed once and left unchanged."""
    key = (CASES.index(case), names)
    if key not in _yard:
        L, V, T, count = case
        p0, v0, par, head, t = case_inputs(case)
        d = directions(t, names)
        _yard[key] = [J.yardstick(p0, v0, par, head, T, DT, count=count, **{n: d[n][k] for n in names}) for k in range(len(names) + 1)]
    return _yard[key]


# =================================================================================================================
# (a) primal bits, (b) the yardstick
# =================================================================================================================
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_tangents_against_the_float64_yardstick(cuda, case):
    """Each of t_p0, t_v0, t_head, t_params alone and all four together (K = 5, the t_params kernel), and t_p0, t_v0, t_head alone and
    together (K = 4, the state-only kernel), with and without t_hist: live slots within TOL_GRAD of the yardstick, norm-relative per
    output plane; dead slots exactly 0; the call without t_hist returns the bits of the call with it; the primal outputs are
    dhts.micro_rollout's bits."""
    import torch
    import dhts
    L, V, T, count = case
    p0, v0, par, head, t = case_inputs(case)
    cnt = None if count is None else torch.tensor(count, device=cuda, dtype=torch.int32)
    ref = dhts.micro_rollout(torch.tensor(p0, device=cuda), torch.tensor(v0, device=cuda), torch.tensor(par, device=cuda),
                             torch.tensor(head, device=cuda), T, DT, count=cnt, want_hist=True)
    live = J.live_mask(L, V, count)
    for names in (LEAVES, LEAVES[:3]):
        d = directions(t, names)
        K = len(names) + 1
        with_h = device_jvp(cuda, p0, v0, par, head, T, DT, count=count, want_hist=True, **d)
        without = device_jvp(cuda, p0, v0, par, head, T, DT, count=count, want_hist=False, **d)
        assert with_h["t_hist"].shape == (K, T, L, 2, V) and with_h["t_pT"].shape == (K, L, V)
        assert same_bits(with_h["t_pT"], without["t_pT"]) and same_bits(with_h["t_vT"], without["t_vT"])
        for o in (with_h, without):
            assert same_bits(o["pT"], ref[0].cpu().numpy()) and same_bits(o["vT"], ref[1].cpu().numpy())
        lt = np.broadcast_to(live[None, :, None, :], (T, L, 2, V))
        assert same_bits(with_h["hist"][lt], ref[2].cpu().numpy()[lt])
        for lane in range(L):                    # the lanes with the gap (0.5, 0) are under the clip: their heads stand still
            n = V if count is None else count[lane]
            if T > 0 and n > 0 and tuple(head[lane]) == HEADS[2]:
                assert with_h["vT"][lane, n - 1] == 0.0
        ys = yard(case, names)
        for k in range(K):
            got = dict(t_pT=with_h["t_pT"][k], t_vT=with_h["t_vT"][k], t_hist=with_h["t_hist"][k])
            J.compare("%s K=%d direction %d (%s)" % (IDS[CASES.index(case)], K, k, names[k] if k < K - 1 else "all"), got, ys[k], count, TOL_GRAD)


# =================================================================================================================
# (c) the numpy chain on the device's own tape, (g) guard bands
# =================================================================================================================
def raw_forward(cuda, p0, v0, par, head, T, dt, count=None, want_ptape=False):
    import torch
    from dhts import ops
    L, V = p0.shape
    desc = ops.micro_desc(L, V, dt)
    tape = torch.empty(ops.micro_tape_numel(desc, T), dtype=torch.float32, device=cuda)
    ptape = torch.zeros(ops.micro_param_tape_numel(desc, T), dtype=torch.float32, device=cuda) if want_ptape else None
    cnt = None if count is None else torch.tensor(count, device=cuda, dtype=torch.int32)
    tpar = torch.tensor(par, device=cuda, dtype=torch.float64)
    ops.micro_rollout_fwd(desc, T, torch.tensor(p0, device=cuda), torch.tensor(v0, device=cuda), tpar,
                          torch.tensor(head, device=cuda, dtype=torch.float64), count=cnt, tape=tape, ptape=ptape)
    return desc, tape, ptape, cnt, tpar


def guarded(shape, cuda, guard=256):
    """A NaN-prefilled flat buffer and the view of `shape` in its middle."""
    import torch
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * guard,), float("nan"), dtype=torch.float32, device=cuda)
    return buf, buf[guard:guard + n].view(*shape)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_chain_on_the_devices_own_tape_and_guard_bands(cuda, case):
    """The raw entry point, K = 3 (one launch of four slots, one masked): tangents against the numpy chain on blocks expanded from the
    device's own tape.  The two run the same float32 operations, so they differ by the rare double rounding of the chain's emulated
    fused multiply-add only; the bound is what T steps of four roundings of 2^-24 each could add up to, norm-relative per plane.
    The outputs sit in the middle of NaN-prefilled buffers: every element is written, nothing outside is."""
    import torch
    from dhts import ops
    L, V, T, count = case
    p0, v0, par, head, t = case_inputs(case)
    K = 3
    rng = np.random.default_rng(5)
    t_p, t_v = rng.standard_normal((2, K, L, V)).astype(np.float32)
    t_head = rng.standard_normal((K, L, 2))
    t_par = rng.standard_normal((K, 6, L, V))
    for want_params in (False, True):
        desc, tape, ptape, cnt, tpar = raw_forward(cuda, p0, v0, par, head, T, DT, count, want_ptape=want_params)
        bufs = [guarded((K, L, V), cuda), guarded((K, L, V), cuda), guarded((K, T, L, 2, V), cuda)]
        err = ops.new_error_record(cuda)
        kw = dict(ptape=ptape, params=tpar, t_params=torch.tensor(t_par, device=cuda)) if want_params else {}
        o = ops.micro_rollout_jvp(desc, T, tape if T > 0 else None, torch.tensor(t_p, device=cuda), torch.tensor(t_v, device=cuda),
                                  count=cnt, t_head=torch.tensor(t_head, device=cuda), err=err, out=(bufs[0][1], bufs[1][1]),
                                  t_hist=bufs[2][1], **kw)
        torch.cuda.synchronize()
        assert err.tolist()[0] == 0
        assert o[0].data_ptr() == bufs[0][1].data_ptr() and o[1].data_ptr() == bufs[1][1].data_ptr() and o[2] is bufs[2][1]
        for buf, view in bufs:
            b = buf.cpu().numpy()
            assert np.all(np.isnan(b[:256])) and np.all(np.isnan(b[b.size - 256:])), "a guard band was written"
            assert np.all(np.isfinite(b[256:b.size - 256])), "an element was not written"
        if want_params:
            continue
        dqs = J.expand(tape.cpu().numpy(), L, V, T, DT)
        tol = max(T, 1) * 4 * 2.0 ** -24
        for k in range(K):
            ref = dict(t_pT=np.zeros((L, V), np.float32), t_vT=np.zeros((L, V), np.float32), t_hist=np.zeros((T, L, 2, V), np.float32))
            for lane in range(L):
                n = V if count is None else count[lane]
                ref["t_pT"][lane], ref["t_vT"][lane], ref["t_hist"][:, lane] = J.chain(dqs[:, lane], t_p[k, lane], t_v[k, lane], t_head[k, lane], n)
            got = dict(t_pT=o[0][k].cpu().numpy(), t_vT=o[1][k].cpu().numpy(), t_hist=o[2][k].cpu().numpy())
            J.compare("%s direction %d vs chain" % (IDS[CASES.index(case)], k), got, ref, count, tol)


# =================================================================================================================
# (d) bit-identity across K, slots, runs and lane order
# =================================================================================================================
@pytest.mark.parametrize("want_params", [False, True], ids=["state", "params"])
def test_a_direction_does_not_depend_on_k_or_slot(cuda, want_params):
    """Direction i of a K-direction call equals the K = 1 call of it, bit for bit, for K = 1 .. 5 and every slot (K = 3 rides in four
    slots with one masked, K = 5 in two launches); two runs give the same bits; permuting the lanes permutes the results."""
    L, V, T = 4, 130, 7
    count = [130, 0, 77, 1]
    rng = np.random.default_rng(17)
    p0, v0, par, head = lanes(rng, L, V)
    head[0], head[2], head[3] = HEADS[1], HEADS[2], HEADS[1]
    stop_head(par, head, 2, count[2])
    names = LEAVES if want_params else LEAVES[:3]
    shapes = dict(t_p0=(L, V), t_v0=(L, V), t_head=(L, 2), t_params=(6, L, V))
    full = {n: rng.standard_normal((5,) + shapes[n]).astype(np.float32 if n in ("t_p0", "t_v0") else np.float64) for n in names}
    keys = ("t_pT", "t_vT", "t_hist")
    single = [device_jvp(cuda, p0, v0, par, head, T, DT, count=count, want_hist=True, **{n: full[n][i:i + 1] for n in names}) for i in range(5)]
    for K in range(1, 6):
        for first in range(0, 6 - K):            # directions first .. first + K - 1: every direction visits every slot
            o = device_jvp(cuda, p0, v0, par, head, T, DT, count=count, want_hist=True, **{n: full[n][first:first + K] for n in names})
            for i in range(K):
                for key in keys:
                    assert same_bits(o[key][i], single[first + i][key][0]), "K=%d first=%d slot %d: %s differs from the K = 1 call" % (K, first, i, key)
    a = device_jvp(cuda, p0, v0, par, head, T, DT, count=count, want_hist=True, **full)
    b = device_jvp(cuda, p0, v0, par, head, T, DT, count=count, want_hist=True, **full)
    assert all(same_bits(a[key], b[key]) for key in keys), "two runs differ"
    perm = [2, 0, 3, 1]
    lane_axis = dict(t_p0=1, t_v0=1, t_head=1, t_params=2)
    c = device_jvp(cuda, p0[perm], v0[perm], par[:, perm], head[perm], T, DT, count=[count[i] for i in perm], want_hist=True,
                   **{n: np.take(full[n], perm, axis=lane_axis[n]) for n in names})
    assert same_bits(c["t_pT"], a["t_pT"][:, perm]) and same_bits(c["t_vT"], a["t_vT"][:, perm]) and same_bits(c["t_hist"], a["t_hist"][:, :, perm])


# =================================================================================================================
# (e) adjointness with the device's own reverse sweep
# =================================================================================================================
@pytest.mark.parametrize("shape", [(3, 65, 7, [65, 30, 1]), (3, 130, 50, None), (3, 1024, 20, [1024, 513, 0])], ids=["V65_T7", "V130_T50", "V1024_T20"])
@pytest.mark.parametrize("on_hist", [False, True], ids=["final", "history"])
def test_forward_and_reverse_sweeps_are_adjoint(cuda, shape, on_hist):
    """<g, J t> = <J^T g, t> with J^T g from dhts.micro_rollout's backward, for a tangent of each of the five leaves (p0, v0, the head
    gap's position and speed parts, the driver parameters) and cotangents of the final state or of the history: evaluated in float64,
    within 1e-4 of sum |g_i (J t)_i|."""
    import torch
    import dhts
    L, V, T, count = shape
    rng = np.random.default_rng(3 + V)
    p0, v0, par, head = lanes(rng, L, V)
    for lane in range(L):
        head[lane] = HEADS[lane % (3 if T <= 7 else 2)]
        stop_head(par, head, lane, V if count is None else count[lane])
    tp0, tv0 = torch.tensor(p0, device=cuda, requires_grad=True), torch.tensor(v0, device=cuda, requires_grad=True)
    tpar, thead = torch.tensor(par, device=cuda, requires_grad=True), torch.tensor(head, device=cuda, requires_grad=True)
    cnt = None if count is None else torch.tensor(count, device=cuda, dtype=torch.int32)
    pT, vT, hist = dhts.micro_rollout(tp0, tv0, tpar, thead, T, DT, count=cnt, want_hist=True)
    live = J.live_mask(L, V, count)
    g_p, g_v = rng.standard_normal((2, L, V)).astype(np.float32) * (0.0 if on_hist else 1.0)
    g_h = rng.standard_normal((T, L, 2, V)).astype(np.float32) * (1.0 if on_hist else 0.0) * live[None, :, None, :]
    ((pT * torch.tensor(g_p, device=cuda)).sum() + (vT * torch.tensor(g_v, device=cuda)).sum() + (hist * torch.tensor(g_h, device=cuda)).sum()).backward()
    K = 5
    t = dict(t_p0=np.zeros((K, L, V), np.float32), t_v0=np.zeros((K, L, V), np.float32), t_head=np.zeros((K, L, 2)), t_params=np.zeros((K, 6, L, V)))
    t["t_p0"][0], t["t_v0"][1] = rng.standard_normal((2, L, V))
    t["t_head"][2, :, 0], t["t_head"][3, :, 1] = rng.standard_normal((2, L))
    t["t_params"][4] = rng.standard_normal((6, L, V))
    o = device_jvp(cuda, p0, v0, par, head, T, DT, count=count, want_hist=True, **t)
    grads = dict(t_p0=tp0.grad, t_v0=tv0.grad, t_head=thead.grad, t_params=tpar.grad)
    for k, leaf in enumerate(("t_p0", "t_v0", "t_head", "t_head", "t_params")):
        left = [g_p.astype(np.float64) * o["t_pT"][k], g_v.astype(np.float64) * o["t_vT"][k], g_h.astype(np.float64) * o["t_hist"][k]]
        lhs, scale = sum(float(x.sum()) for x in left), sum(float(np.abs(x).sum()) for x in left)
        rhs = float((grads[leaf].cpu().numpy().astype(np.float64) * t[leaf][k]).sum())
        print("V%d T%d %s direction %d (%s): <g, J t> = %.9g, <J^T g, t> = %.9g, |d| / sum |products| = %.2e"
              % (V, T, "history" if on_hist else "final", k, leaf, lhs, rhs, abs(lhs - rhs) / max(scale, 1e-300)))
        assert scale > 0 or T == 0
        assert abs(lhs - rhs) <= 1e-4 * scale


# =================================================================================================================
# (f) exact zeros, the state-only bits, the clip
# =================================================================================================================
def test_zeros_dead_slots_and_the_clip(cuda):
    """A zero tangent gives exact zeros; t_params = 0 gives the bits of the state-only call; dead slots and empty lanes are exact zeros
    whatever their input tangents; under the acceleration clip the parameter term is absent: a head that stops in its one step returns
    the bits of the state-only call, its followers do not."""
    L, V, T = 3, 70, 7
    count = [70, 0, 33]
    rng = np.random.default_rng(23)
    p0, v0, par, head = lanes(rng, L, V)
    head[0], head[2] = HEADS[1], HEADS[2]
    stop_head(par, head, 2, count[2])
    z = device_jvp(cuda, p0, v0, par, head, T, DT, count=count, want_hist=True, t_p0=np.zeros((2, L, V), np.float32),
                   t_params=np.zeros((2, 6, L, V)), t_head=np.zeros((2, L, 2)))
    assert all(np.all(z[k] == 0) for k in ("t_pT", "t_vT", "t_hist"))
    t_p, t_v = rng.standard_normal((2, 2, L, V)).astype(np.float32)
    t_head = rng.standard_normal((2, L, 2))
    state = device_jvp(cuda, p0, v0, par, head, T, DT, count=count, want_hist=True, t_p0=t_p, t_v0=t_v, t_head=t_head)
    zero_q = device_jvp(cuda, p0, v0, par, head, T, DT, count=count, want_hist=True, t_p0=t_p, t_v0=t_v, t_head=t_head,
                        t_params=np.zeros((2, 6, L, V)))
    assert all(same_bits(state[k], zero_q[k]) for k in ("t_pT", "t_vT", "t_hist"))
    live = J.live_mask(L, V, count)
    for o in (state, zero_q):
        assert np.all(o["t_pT"][:, ~live] == 0) and np.all(o["t_vT"][:, ~live] == 0)
        assert np.all(o["t_hist"][:, :, ~live[:, None, :].repeat(2, 1)] == 0)
    # one step, head gap (0.5, 0): the head vehicle (slot count - 1) is under the clip, its follower is not
    one = [device_jvp(cuda, p0, v0, par, head, 1, DT, count=count, want_hist=True, t_p0=t_p, t_v0=t_v, t_head=t_head, **kw)
           for kw in ({}, dict(t_params=rng.standard_normal((2, 6, L, V))))]
    assert one[0]["vT"][2, 32] == 0.0, "the head of lane 2 stops in its one step (acceleration clip)"
    assert same_bits(one[0]["t_vT"][:, 2, 32], one[1]["t_vT"][:, 2, 32]) and same_bits(one[0]["t_pT"], one[1]["t_pT"])
    assert np.all(one[1]["t_vT"][:, 2, 32] == 0)
    assert np.all(one[0]["t_vT"][:, 2, :32] != one[1]["t_vT"][:, 2, :32]) and np.all(one[0]["t_vT"][:, 0] != one[1]["t_vT"][:, 0])


# =================================================================================================================
# (h) fault records
# =================================================================================================================
def test_fault_records(cuda):
    """A NaN in one initial tangent is on record as DHTS_FAULT_NAN with its lane and step 0 (the operator raises like the reverse
    sweep's check); a parameter tape of another shape gives NaN tangents and the capacity fault, index -3, and is not read."""
    import torch
    from dhts import _lib, ops
    L, V, T = 4, 70, 5
    rng = np.random.default_rng(2)
    p0, v0, par, head = lanes(rng, L, V)
    desc, tape, ptape, cnt, tpar = raw_forward(cuda, p0, v0, par, head, T, DT, want_ptape=True)
    t_p = torch.zeros(2, L, V, device=cuda)
    t_p[1, 2, 40] = float("nan")
    t_v = torch.ones(2, L, V, device=cuda)
    err = ops.new_error_record(cuda)
    o = ops.micro_rollout_jvp(desc, T, tape, t_p, t_v, err=err)
    code, step, lane, index = err.tolist()
    assert (code, step, lane) == (_lib.FAULT_NAN, 0, 2) and index in (39, 40)
    assert bool(torch.all(torch.isfinite(o[0][0]))) and bool(torch.isnan(o[0][1, 2, 40]))
    with pytest.raises(AssertionError):
        device_jvp(cuda, p0, v0, par, head, T, DT, t_p0=t_p.cpu().numpy())
    device_jvp(cuda, p0, v0, par, head, T, DT, check_faults=False, t_p0=t_p.cpu().numpy())
    # the parameter tape
    t_q = torch.ones(2, 6, L, V, dtype=torch.float64, device=cuda)
    err = ops.new_error_record(cuda)
    o = ops.micro_rollout_jvp(desc, T, tape, t_v, t_v, ptape=ptape, params=tpar, t_params=t_q, want_hist=True, err=err)
    assert err.tolist()[0] == 0 and all(bool(torch.all(torch.isfinite(x))) for x in o)
    _, _, ptape4, _, _ = raw_forward(cuda, p0, v0, par, head, T - 1, DT, want_ptape=True)      # a tape of T - 1 steps
    big = torch.zeros_like(ptape)
    big[:ptape4.numel()] = ptape4
    o = ops.micro_rollout_jvp(desc, T, tape, t_v, t_v, ptape=big, params=tpar, t_params=t_q, want_hist=True, err=err)
    code, _, _, index = err.tolist()
    assert code == _lib.FAULT_CAPACITY and index == -3 and all(bool(torch.all(torch.isnan(x))) for x in o)
    with pytest.raises(ValueError):
        ops.micro_rollout_jvp(desc, T, tape, t_v, t_v, ptape=ptape4, params=tpar, t_params=t_q)
    with pytest.raises(ValueError):
        ops.micro_rollout_jvp(desc, T, tape, t_v, t_v, ptape=ptape, t_params=t_q)


# =================================================================================================================
# (i) the example
# =================================================================================================================
@pytest.mark.parametrize("method", ["lm", "adam"])
def test_calibration_example_lowers_its_loss(cuda, tmp_path, method):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "calibrate_idm.py"), "--method", method, "--n_lane", "2",
                          "--n_vehicle", "8", "--n_step", "40", "--n_episode", "6"], cwd=str(tmp_path), env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    files = [os.path.join(dp, f) for dp, _, fs in os.walk(str(tmp_path)) for f in fs if f.startswith("trial_") and f.endswith(".txt")]
    assert files, "no trial_k.txt written"
    losses = [float(line.split()[-1]) for line in open(files[0]) if line.strip()]
    print("calibration (%s) loss: first %.6g, last %.6g over %d iterations" % (method, losses[0], losses[-1], len(losses)))
    assert len(losses) == 6 and losses[-1] < losses[0]
