"""A closed ARZ lane on the GPU (dhts.macro_rollout(ring=True), dhts.macro_rollout_jvp(ring=True, fused=True) and the raw _ring
wrappers): the forward's bits and the tangents' against EXISTING device code on an open lane that holds the state three times (T <= N:
the open ends cannot reach the middle copy), translation round the ring, the chained oracle tests/macro_ring_ref.py for T > N, folded
gradients of the tiled lane, the target form against detectors at every cell, the adjoint identity between the new reverse and forward
forms, mass, the longest lanes, the CFL record at the seam and the edges.  Every case is a few thousand cell-steps per lane."""
import os
import subprocess
import sys

import numpy as np
import pytest

from macro_ring_ref import FOLD_STEPS, ORACLE_CASES, SIZES, jump_state, ring_bwd, ring_fwd
from util import TOL_GRAD, TOL_STATE, grad_report, rel_max, state_report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, DX, UM = 0.01, 5.0, 30.0


def tt(cuda, a, grad=False):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device=cuda, requires_grad=grad)


def bits(a):
    return a.detach().cpu().numpy().view(np.int32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def ring(cuda, r, u, T, checkpoint=True, **kw):
    import dhts
    return dhts.macro_rollout(tt(cuda, r), tt(cuda, u), None, None, T, DT, DX, UM, ring=True, checkpoint=checkpoint, **kw)


def ring_grads(cuda, r, u, T, loss, checkpoint=True, **kw):
    import dhts
    tr, tu = tt(cuda, r, True), tt(cuda, u, True)
    out = dhts.macro_rollout(tr, tu, None, None, T, DT, DX, UM, ring=True, checkpoint=checkpoint, **kw)
    loss(out).backward()
    return out, tr.grad, tu.grad


def ends(L, seed=5):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.1, 0.9, (L, 2)).astype(np.float32), rng.uniform(0.0, UM, (L, 2)).astype(np.float32)


def tiled(cuda, r, u, T, grad=False, **kw):
    """EXISTING code: the taped dhts.macro_rollout on the open lane of 3 N cells that holds the state three times, any boundary cells."""
    import dhts
    gr, gu = ends(r.shape[0])
    tr, tu = tt(cuda, np.tile(r, (1, 3)), grad), tt(cuda, np.tile(u, (1, 3)), grad)
    return dhts.macro_rollout(tr, tu, tt(cuda, gr), tt(cuda, gu), T, DT, DX, UM, **kw), tr, tu


def steps_of(N):
    return sorted({1, min(7, N), N})


# ---- 1. forward bits against existing code ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", (1, 3))
@pytest.mark.parametrize("N", SIZES)
def test_forward_is_the_middle_copy_of_the_tiled_lane(cuda, N, L):
    import dhts
    r, u = jump_state(L, N, seed=N)
    det = sorted({0, N // 2, N - 1})
    for T in steps_of(N):
        (tiles, _, _) = tiled(cuda, r, u, T, detectors=[N + d for d in det])
        plain = ring(cuda, r, u, T)
        tapped = ring(cuda, r, u, T, detectors=det)
        t_r0 = tt(cuda, np.ones((1, L, N), np.float32))
        fused, _ = dhts.macro_rollout_jvp(tt(cuda, r), tt(cuda, u), None, None, T, DT, DX, UM, ring=True, fused=True, t_r0=t_r0, detectors=det)
        for k in range(4):
            want = tiles[k][:, N:2 * N]
            assert same_bits(plain[k], want) and same_bits(tapped[k], want) and same_bits(fused[k], want), (N, T, k)
        assert same_bits(tapped[4], tiles[4]) and same_bits(fused[4], tiles[4]), "readings, T = %d" % T
        if N > 1:
            assert not same_bits(tiles[0][:, :N], tiles[0][:, N:2 * N]), "the open end did not move the first copy"


# ---- 2. translation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,m", [(2, 1), (3, 2), (63, 1), (64, 63), (65, 64), (128, 64), (129, 65), (300, 171)])
def test_translation(cuda, N, m):
    import torch
    import dhts
    L, T = 3, min(2 * N + 5, 650)
    r, u = jump_state(L, N, seed=N)
    rm, um_ = np.roll(r, m, axis=1), np.roll(u, m, axis=1)
    loss = lambda o: (o[0] ** 2).sum() + (o[2] ** 2).sum()
    a, g_r, g_u = ring_grads(cuda, r, u, T, loss)
    b, g_rm, g_um = ring_grads(cuda, rm, um_, T, loss)
    t_r0 = np.random.default_rng(N).standard_normal((2, L, N)).astype(np.float32)
    fa, ta = dhts.macro_rollout_jvp(tt(cuda, r), tt(cuda, u), None, None, T, DT, DX, UM, ring=True, fused=True, t_r0=tt(cuda, t_r0))
    fb, tb = dhts.macro_rollout_jvp(tt(cuda, rm), tt(cuda, um_), None, None, T, DT, DX, UM, ring=True, fused=True,
                                    t_r0=tt(cuda, np.roll(t_r0, m, axis=2)))
    for k in range(4):
        assert same_bits(torch.roll(a[k], m, 1), b[k]) and same_bits(torch.roll(fa[k], m, 1), fb[k]), k
    e = max(rel_max(g_rm.cpu().numpy(), np.roll(g_r.cpu().numpy(), m, 1)), rel_max(g_um.cpu().numpy(), np.roll(g_u.cpu().numpy(), m, 1)),
            *(rel_max(tb[k].cpu().numpy(), np.roll(ta[k].cpu().numpy(), m, 2)) for k in range(3)))
    print("N = %d, m = %d: largest difference of rolled gradients and tangents %.2e" % (N, m, e))
    assert e <= TOL_GRAD


# ---- 3. the chained oracle, T > N -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,N,T", ORACLE_CASES)
@pytest.mark.parametrize("loss", ("final", "detectors"))
def test_against_the_chained_oracle(cuda, oracle, L, N, T, loss):
    r, u = jump_state(L, N, seed=N)
    f = ring_fwd(oracle, r, u, T, DT, DX, UM)
    rng = np.random.default_rng(T)
    if loss == "final":
        w_r, w_u = rng.standard_normal((2, L, N)).astype(np.float32)
        out, g_r, g_u = ring_grads(cuda, r, u, T, lambda o: (o[0] * tt(cuda, w_r)).sum() + (o[2] * tt(cuda, w_u)).sum())
        b = ring_bwd(oracle, f, g_rT=w_r, g_uT=w_u)
    else:
        det = sorted({0, N // 2, N - 1})
        w = rng.standard_normal((T, L, 3, len(det))).astype(np.float32)
        out, g_r, g_u = ring_grads(cuda, r, u, T, lambda o: (o[4] * tt(cuda, w)).sum(), detectors=det)
        gh = np.zeros((3, T, L, N), np.float32)
        gh[:, :, :, det] = w.transpose(2, 0, 1, 3)
        b = ring_bwd(oracle, f, gh_r=gh[0], gh_y=gh[1], gh_u=gh[2])
        for k, name in enumerate(("hist_r", "hist_y", "hist_u")):
            assert state_report("readings %s" % name, out[4][:, :, k].detach().cpu().numpy(), f[name][:, :, det]) <= TOL_STATE
    for k, name in enumerate(("rT", "yT", "uT")):
        assert state_report(name, out[k].detach().cpu().numpy(), f[name]) <= TOL_STATE
    assert grad_report("g_r0 N=%d T=%d %s" % (N, T, loss), g_r.cpu().numpy(), b["g_r0"]) <= TOL_GRAD
    assert grad_report("g_u0 N=%d T=%d %s" % (N, T, loss), g_u.cpu().numpy(), b["g_u0"]) <= TOL_GRAD


# ---- 4. reverse against existing code; the segment length ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_gradients_fold_the_tiled_lane_and_do_not_depend_on_the_segment(cuda, N):
    import torch
    from dhts import ops
    L, T = 3, min(N, FOLD_STEPS)
    r, u = jump_state(L, N, seed=N)
    rng = np.random.default_rng(N)
    w_r, w_u = rng.standard_normal((2, L, N)).astype(np.float32)
    w3_r, w3_u = np.zeros((2, L, 3 * N), np.float32)
    w3_r[:, N:2 * N], w3_u[:, N:2 * N] = w_r, w_u
    loss = lambda o: (o[0] * tt(cuda, w_r)).sum() + (o[2] * tt(cuda, w_u)).sum()
    plan = ops.macro_ckpt_plan(ops.macro_desc(L, N, DT, DX, UM), T)
    got = [ring_grads(cuda, r, u, T, loss, checkpoint=c) for c in (True, 1, 3, plan["max_segment"])]
    for _, g_r, g_u in got[1:]:
        assert same_bits(g_r, got[0][1]) and same_bits(g_u, got[0][2]), "the segment length changes a bit of the gradient"
    out, tr, tu = tiled(cuda, r, u, T, grad=True)
    ((out[0] * tt(cuda, w3_r)).sum() + (out[2] * tt(cuda, w3_u)).sum()).backward()
    for name, g, t in (("g_r0", got[0][1], tr), ("g_u0", got[0][2], tu)):
        folded = t.grad.cpu().numpy().astype(np.float64).reshape(L, 3, N).sum(axis=1)
        assert grad_report("%s N=%d T=%d" % (name, N, T), g.cpu().numpy(), folded) <= TOL_GRAD


# ---- 5. target equals detectors at every cell ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,N,T", [(3, 1, 7), (3, 2, 9), (3, 65, 135), (1, 129, 30), (1, 300, 9)])
def test_target_equals_detectors_at_every_cell(cuda, L, N, T):
    import torch
    r, u = jump_state(L, N, seed=N)
    rng = np.random.default_rng(N)
    target = np.stack([rng.uniform(0.1, 0.9, (T, L, N)), rng.uniform(0.0, UM, (T, L, N))], axis=2).astype(np.float32)
    target[rng.uniform(size=target.shape) < 0.2] = np.nan
    tg = tt(cuda, target)
    w = tt(cuda, rng.uniform(0.5, 1.5, (L, 2)))

    def by_detectors(o):
        x = torch.stack([o[4][:, :, 0], o[4][:, :, 2]], dim=2)                 # (r, u) of every cell after every step
        e = torch.where(torch.isnan(tg), torch.zeros_like(x), x - tg)
        by_detectors.sse = (e.double() ** 2).sum(dim=(0, 3))
        return (by_detectors.sse * w).sum()
    a, g_r, g_u = ring_grads(cuda, r, u, T, lambda o: (o[4] * w).sum(), target=tg)
    b, h_r, h_u = ring_grads(cuda, r, u, T, by_detectors, detectors=list(range(N)))
    for k in range(4):
        assert same_bits(a[k], b[k])
    assert state_report("sse", a[4].detach().cpu().numpy(), by_detectors.sse.detach().cpu().numpy()) <= TOL_STATE
    assert grad_report("g_r0 target", g_r.cpu().numpy(), h_r.cpu().numpy()) <= TOL_GRAD
    assert grad_report("g_u0 target", g_u.cpu().numpy(), h_u.cpu().numpy()) <= TOL_GRAD


# ---- 6. fused tangents --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_fused_tangents(cuda, N):
    import torch
    import dhts
    L, T = 3, min(N, FOLD_STEPS)
    r, u = jump_state(L, N, seed=N)
    rng = np.random.default_rng(N)
    t_r, t_u = rng.standard_normal((2, 5, L, N)).astype(np.float32)
    det = sorted({0, N - 1})

    def jvp(sl, **kw):
        return dhts.macro_rollout_jvp(tt(cuda, r), tt(cuda, u), None, None, T, DT, DX, UM, ring=True, fused=True, t_r0=tt(cuda, t_r[sl]),
                                      t_u0=tt(cuda, t_u[sl]), detectors=det, **kw)
    full = jvp(slice(0, 5))
    for sl in (slice(0, 1), slice(4, 5), slice(1, 4), slice(0, 4), slice(2, 5)):      # K = 1, 1, 3, 4, 3: other slots, other launches
        part = jvp(sl)
        for k in range(5):
            assert same_bits(part[0][k], full[0][k])
        for k in range(4):
            assert same_bits(part[1][k], full[1][k][sl]), "direction %s in a launch of %d: output %d" % (sl, sl.stop - sl.start, k)
    # the tiled lane's fused call (existing code) with the direction tiled three times
    gr, gu = ends(L)
    tl = dhts.macro_rollout_jvp(tt(cuda, np.tile(r, (1, 3))), tt(cuda, np.tile(u, (1, 3))), tt(cuda, gr), tt(cuda, gu), T, DT, DX, UM, fused=True,
                                t_r0=tt(cuda, np.tile(t_r, (1, 1, 3))), t_u0=tt(cuda, np.tile(t_u, (1, 1, 3))), detectors=[N + d for d in det])
    for k in range(3):
        assert same_bits(full[1][k], tl[1][k][:, :, N:2 * N]), "tangent %d against the tiled lane" % k
    assert same_bits(full[1][3], tl[1][3]), "tangent readings against the tiled lane"
    # <g, J t> = <J^T g, t> between the new reverse and forward forms
    w_r, w_u = rng.standard_normal((2, L, N)).astype(np.float32)
    _, g_r, g_u = ring_grads(cuda, r, u, T, lambda o: (o[0] * tt(cuda, w_r)).sum() + (o[2] * tt(cuda, w_u)).sum())
    for d in range(5):
        lhs = float((full[1][0][d].double() * tt(cuda, w_r).double()).sum() + (full[1][2][d].double() * tt(cuda, w_u).double()).sum())
        rhs = float((g_r.double() * tt(cuda, t_r[d]).double()).sum() + (g_u.double() * tt(cuda, t_u[d]).double()).sum())
        scale = float((full[1][0][d].double().abs() * tt(cuda, w_r).double().abs()).sum() +
                      (full[1][2][d].double().abs() * tt(cuda, w_u).double().abs()).sum())
        print("N = %d direction %d: <g, J t> = %.6e, <J^T g, t> = %.6e" % (N, d, lhs, rhs))
        assert abs(lhs - rhs) <= TOL_GRAD * max(scale, 1e-30)


# ---- 7. mass ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (2, 65, 300))
def test_mass_is_conserved(cuda, N):
    L, T = 3, min(2 * N + 5, 650)
    r, u = jump_state(L, N, seed=N)
    out = ring(cuda, r, u, T, detectors=list(range(N)))
    top = max(float(r.max()), float(out[4][:, :, 0].max()))
    drift = np.abs(out[0].double().sum(dim=1).cpu().numpy() - r.astype(np.float64).sum(axis=1))
    bound = T * N * 2.0 ** -24 * top
    print("N = %d, T = %d: mass drift %s, bound %.3e" % (N, T, drift, bound))
    assert np.all(drift <= bound)


# ---- 8. the longest lanes -----------------------------------------------------------------------------------------------------------
def test_long_lanes(cuda, oracle):
    import torch
    import dhts
    L, T = 1, 8
    # checkpointed, 1319 cells, and the target form, 1239 cells: forward bits and folded gradients of the tiled lane on the TAPED path
    # (3957 / 3717 cells).  The target case weighs sse, over a finite target with a fifth of its entries unobserved: the tiled lane forms
    # the same squared error in torch, from the middle copy of its history
    for N, fit in ((1319, False), (1239, True)):
        r, u = jump_state(L, N, seed=N)
        rng = np.random.default_rng(N)
        w_r = rng.standard_normal((L, N)).astype(np.float32)
        w3 = np.zeros((L, 3 * N), np.float32)
        w3[:, N:2 * N] = w_r
        if fit:
            target = np.stack([rng.uniform(0.1, 0.9, (T, L, N)), rng.uniform(0.0, UM, (T, L, N))], axis=2).astype(np.float32)
            target[rng.uniform(size=target.shape) < 0.2] = np.nan
            tg, w_s = tt(cuda, target), tt(cuda, rng.uniform(0.5, 1.5, (L, 2)))
            out, g_r, g_u = ring_grads(cuda, r, u, T, lambda o: (o[0] * tt(cuda, w_r)).sum() + (o[4] * w_s).sum(), target=tg)
            tiles, tr, tu = tiled(cuda, r, u, T, grad=True, want_hist=True)
            x = torch.stack([tiles[4][:, :, 0, N:2 * N], tiles[4][:, :, 2, N:2 * N]], dim=2)
            e = torch.where(torch.isnan(tg), torch.zeros_like(x), x - tg)
            sse = (e.double() ** 2).sum(dim=(0, 3))
            ((tiles[0] * tt(cuda, w3)).sum() + (sse * w_s).sum()).backward()
            assert state_report("sse N=%d" % N, out[4].detach().cpu().numpy(), sse.detach().cpu().numpy()) <= TOL_STATE
        else:
            out, g_r, g_u = ring_grads(cuda, r, u, T, lambda o: (o[0] * tt(cuda, w_r)).sum())
            tiles, tr, tu = tiled(cuda, r, u, T, grad=True)
            (tiles[0] * tt(cuda, w3)).sum().backward()
        for k in range(4):
            assert same_bits(out[k], tiles[k][:, N:2 * N]), (N, k)
        for name, g, t in (("g_r0", g_r, tr), ("g_u0", g_u, tu)):
            folded = t.grad.cpu().numpy().astype(np.float64).reshape(L, 3, N).sum(axis=1)
            assert grad_report("%s N=%d" % (name, N), g.cpu().numpy(), folded) <= TOL_GRAD
    # fused, 1410 cells, one direction: against the chained oracle
    N = 1410
    r, u = jump_state(L, N, seed=N)
    f = ring_fwd(oracle, r, u, T, DT, DX, UM)
    t_r = np.random.default_rng(N).standard_normal((1, L, N)).astype(np.float32)
    prim, tan = dhts.macro_rollout_jvp(tt(cuda, r), tt(cuda, u), None, None, T, DT, DX, UM, ring=True, fused=True, t_r0=tt(cuda, t_r))
    for k, name in enumerate(("rT", "yT", "uT")):
        assert state_report("1410 %s" % name, prim[k].cpu().numpy(), f[name]) <= TOL_STATE
    w_r = np.random.default_rng(1).standard_normal((L, N)).astype(np.float32)
    b = ring_bwd(oracle, f, g_rT=w_r)
    lhs = float((tan[0][0].double() * tt(cuda, w_r).double()).sum())
    rhs = float((b["g_r0"].astype(np.float64) * t_r[0]).sum())
    scale = float((tan[0][0].double().abs() * tt(cuda, w_r).double().abs()).sum())
    print("1410: <g, J t> = %.6e (device), <J^T g, t> = %.6e (oracle)" % (lhs, rhs))
    assert abs(lhs - rhs) <= TOL_GRAD * scale


# ---- 9. the CFL record at the seam --------------------------------------------------------------------------------------------------
def test_cfl_fault_at_the_seam(cuda, oracle):
    """A speed of 5000 in cell 0 of lane 2: interfaces 0 and N, the one seam, fail the CFL test in step 0 and no other interface does
    (the oracle rejects the same step and names interface 0).  The kernels record a fault of interface N as one of interface 0, so the
    record does not depend on which of the two threads wins raise_fault's compare-and-swap: (DHTS_FAULT_CFL, 0, 2, 0).  No device fault
    is involved: the sticky record is the path the schedule's test uses."""
    import dhts
    from dhts import _lib, ops
    L, N, T = 4, 65, 3
    r, u = jump_state(L, N, seed=1)
    u[2, 0] = 5000.0
    f = ring_fwd(oracle, r, u, T, DT, DX, UM, check=False)
    assert f["rc"] == (0, 2, 0)
    desc = ops.macro_desc(L, N, DT, DX, UM)
    tr, tu = tt(cuda, r), tt(cuda, u)
    y, q = ops.macro_state_from_ru(tr, tu, UM)
    err = ops.new_error_record(cuda)
    ckpt = tt(cuda, np.zeros(ops.macro_ckpt_numel(desc, T), np.float32))
    ops.macro_rollout_fwd_ckpt_ring(desc, T, tr, y, tu, q, ckpt, err=err)
    assert err.tolist() == [_lib.FAULT_CFL, 0, 2, 0]
    err, err_j = ops.new_error_record(cuda), ops.new_error_record(cuda)
    ops.macro_rollout_fwd_jvp_ring(desc, T, tr, y, tu, q, tt(cuda, np.ones((1, L, N), np.float32)), tt(cuda, np.zeros((1, L, N), np.float32)),
                                   err=err, err_jvp=err_j)
    assert err.tolist() == [_lib.FAULT_CFL, 0, 2, 0]
    with pytest.raises(AssertionError, match=r"CFL condition.*\(step 0, lane 2, interface 0\)"):
        ring(cuda, r, u, T)


# ---- 10. edges ----------------------------------------------------------------------------------------------------------------------
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
    import torch
    from dhts import ops
    L, T, K, S = 3, 7, 3, 3
    r, u = jump_state(L, N, seed=N)
    det = sorted({0, N - 1})
    D = len(det)
    desc = ops.macro_desc(L, N, DT, DX, UM)
    tr, tu, dt = tt(cuda, r), tt(cuda, u), tt(cuda, np.array(det, np.int32))
    y, q = ops.macro_state_from_ru(tr, tu, UM)
    rng = np.random.default_rng(N)
    g = dict(state=[guarded(cuda, (L, N)) for _ in range(4)], taps=guarded(cuda, (T, L, 3, D)), ckpt=guarded(cuda, (ops.macro_ckpt_numel(desc, T, S),)),
             grads=[guarded(cuda, (L, N)) for _ in range(2)], jvp=[guarded(cuda, (L, N)) for _ in range(4)] + [guarded(cuda, (K, L, N)) for _ in range(2)],
             jtaps=guarded(cuda, (T, L, 3, D)), t_taps=guarded(cuda, (K, T, L, 2, D)))
    ops.macro_rollout_fwd_ckpt_ring(desc, T, tr, y, tu, q, g["ckpt"][1], segment=S, det=dt, out=tuple(v for _, v in g["state"]), taps=g["taps"][1])
    ck = g["ckpt"][1].clone()
    ops.macro_rollout_bwd_ckpt_ring(desc, T, g["ckpt"][1], tr, y, tu, q, tt(cuda, rng.standard_normal((L, N)).astype(np.float32)),
                                    tt(cuda, rng.standard_normal((L, N)).astype(np.float32)), segment=S, det=dt,
                                    g_taps=tt(cuda, rng.standard_normal((T, L, 2, D)).astype(np.float32)), out=tuple(v for _, v in g["grads"]))
    assert torch.equal(ck.view(torch.int32), g["ckpt"][1].view(torch.int32)), "the reverse sweep wrote into the checkpoints"
    ops.macro_rollout_fwd_jvp_ring(desc, T, tr, y, tu, q, tt(cuda, rng.standard_normal((K, L, N)).astype(np.float32)),
                                   tt(cuda, rng.standard_normal((K, L, N)).astype(np.float32)), det=dt, out=tuple(v for _, v in g["jvp"]),
                                   taps=g["jtaps"][1], t_taps=g["t_taps"][1])
    pairs = g["state"] + g["grads"] + g["jvp"] + [g["taps"], g["ckpt"], g["jtaps"], g["t_taps"]]
    for i, (buf, view) in enumerate(pairs):
        assert intact(buf, view), "a store beside buffer %d, or elements of it not written" % i
    # the target pair
    tg = tt(cuda, rng.uniform(0.1, 0.9, (T, L, 2, N)).astype(np.float32))
    st, gd = [guarded(cuda, (L, N)) for _ in range(4)], [guarded(cuda, (L, N)) for _ in range(2)]
    S_t = ops.macro_ckpt_target_plan(desc, T)["segment"]
    ckb = guarded(cuda, (ops.macro_ckpt_numel(desc, T, S_t),))
    out, sse = ops.macro_rollout_fwd_ckpt_target_ring(desc, T, tr, y, tu, q, ckb[1], tg, out=tuple(v for _, v in st))
    ops.macro_rollout_bwd_ckpt_target_ring(desc, T, ckb[1], tr, y, tu, q, torch.zeros_like(tr), torch.zeros_like(tr), tg,
                                           g_sse=torch.ones(L, 2, dtype=torch.float64, device=cuda), final=out[:3], out=tuple(v for _, v in gd))
    for i, (buf, view) in enumerate(st + gd + [ckb]):
        assert intact(buf, view), "target pair: a store beside buffer %d, or elements of it not written" % i
    for k in range(4):
        assert same_bits(out[k], g["state"][k][1])


def test_no_steps_non_contiguous_inputs_and_which_leaves_ask_for_gradients(cuda):
    import torch
    import dhts
    L, N, T = 3, 65, 9
    r, u = jump_state(L, N, seed=3)
    # T = 0: outputs, cotangents and tangents pass through
    out, g_r, g_u = ring_grads(cuda, r, u, 0, lambda o: (o[0] * 2).sum() + (o[2] * 3).sum())
    assert same_bits(out[0], tt(cuda, r)) and same_bits(out[2], tt(cuda, u))
    assert np.allclose(g_r.cpu().numpy(), 2.0) and np.allclose(g_u.cpu().numpy(), 3.0)
    out0 = ring(cuda, r, u, 0, detectors=[0, 5])
    assert tuple(out0[4].shape) == (0, L, 3, 2)
    sse = ring(cuda, r, u, 0, target=tt(cuda, np.zeros((0, L, 2, N), np.float32)))[4]
    assert float(sse.abs().sum()) == 0.0
    t_r = np.random.default_rng(0).standard_normal((2, L, N)).astype(np.float32)
    prim, tan = dhts.macro_rollout_jvp(tt(cuda, r), tt(cuda, u), None, None, 0, DT, DX, UM, ring=True, fused=True, t_r0=tt(cuda, t_r))
    assert same_bits(prim[0], tt(cuda, r)) and same_bits(tan[0], tt(cuda, t_r))
    # non-contiguous leaves
    wide_r, wide_u = tt(cuda, np.repeat(r, 2, axis=1)), tt(cuda, np.repeat(u, 2, axis=1))
    ref = ring(cuda, r, u, T)
    got = dhts.macro_rollout(wide_r[:, ::2], wide_u[:, ::2], None, None, T, DT, DX, UM, ring=True, checkpoint=True)
    for k in range(4):
        assert same_bits(got[k], ref[k])
    # only r0, only u0, neither
    loss = lambda o: (o[0] ** 2).sum() + (o[2] ** 2).sum()
    _, g_r, g_u = ring_grads(cuda, r, u, T, loss)
    for want_r, want_u in ((True, False), (False, True), (False, False)):
        tr, tu = tt(cuda, r, want_r), tt(cuda, u, want_u)
        o = dhts.macro_rollout(tr, tu, None, None, T, DT, DX, UM, ring=True, checkpoint=True)
        assert o[0].requires_grad == (want_r or want_u)
        if want_r or want_u:
            loss(o).backward()
            assert (tr.grad is not None) == want_r and (tu.grad is not None) == want_u
            assert same_bits(tr.grad if want_r else tu.grad, g_r if want_r else g_u)


# ---- 11. the example ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ([], ["--fused-loss"], ["--method", "lm"]))
def test_the_example_recovers_the_bump(cuda, mode):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "ring_wave.py"), "--cells", "24", "--steps", "60", "--iters", "12"] + mode
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    losses = [float(line.split()[-1]) for line in p.stdout.splitlines() if line.startswith("iter")]
    assert len(losses) >= 2 and losses[-1] < losses[0], p.stdout
    mass = [line for line in p.stdout.splitlines() if line.startswith("mass")]
    assert mass and mass[0].rstrip().endswith("conserved"), p.stdout
