"""Yardstick of the ring-road form of the IDM rollout (dhts.micro_rollout(ring=...)): lead_rollout of tests/micro_lead_ref.py with the
head's leader taken from the lane's own tail.  The count vehicles of a lane drive on a ring of circumference ring[l]; the head (slot
count - 1) is an ordinary follower of the image of the tail (slot 0) one circumference ahead, seen at
((float)((double)p_tail + ring), v_tail) of the tail's state before the step.  Positions stay unwrapped.  The tail's length is in the
head's gap and is live.  tests/test_micro_ring.py validates it against lead_rollout fed its own tail trajectory and against chained
oracle steps; tests/test_micro_ring_gpu.py holds the kernels against it where existing device code cannot reach."""
import numpy as np


def ring_rollout(p0, v0, params, ring, T, dt, count=None, store32=True):
    """p0, v0 [L][V] float32 torch tensors; params [6][L][V] float64; ring [L] float64 (data); count [L] integers or None.  Arithmetic
    in float64, the state stored as float32 after every step.  Returns pT, vT [L][V] float32 and hist [T][L][2][V] float32,
    differentiable w.r.t. p0, v0 and params."""
    import torch
    L, V = p0.shape
    n = torch.full((L,), V, dtype=torch.int64) if count is None else torch.as_tensor(count, dtype=torch.int64)
    idx = torch.arange(V)[None, :]
    live, is_head = idx < n[:, None], idx == (n[:, None] - 1)
    ring = torch.as_tensor(ring, dtype=torch.float64).detach()[:, None]
    a, b, vt, s0, tp, ln = params
    ln_front = torch.cat([ln[:, 1:], ln[:, -1:]], 1)
    ln_front = torch.where(is_head, ln[:, 0:1].expand(L, V), ln_front)                           # the tail's length, live
    eps, zero = torch.tensor(1e-5, dtype=torch.float64), torch.tensor(0.0, dtype=torch.float64)
    p, v, hist = p0, v0, []
    for t in range(T):
        pd, vd = p.double(), v.double()
        pl, vl = torch.cat([pd[:, 1:], pd[:, -1:]], 1), torch.cat([vd[:, 1:], vd[:, -1:]], 1)
        pl = torch.where(is_head, (pd[:, 0:1] + ring).float().double(), pl)                      # the tail, one circumference ahead
        vl = torch.where(is_head, vd[:, 0:1], vl)
        gap = (pl - pd).abs() - (ln_front + ln) * 0.5                                            # compute_state_delta, :195-214
        dv = vd - vl
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


def restated_ring(p0, v0, params, ring, T, dt, count=None, g_pT=None, g_vT=None, g_hist=None):
    """ring_rollout on numpy inputs, differentiated for the given cotangents: dict of numpy arrays."""
    import torch
    tp0 = torch.tensor(np.asarray(p0, np.float32), requires_grad=True)
    tv0 = torch.tensor(np.asarray(v0, np.float32), requires_grad=True)
    tpar = torch.tensor(np.asarray(params, np.float64), requires_grad=True)
    pT, vT, hist = ring_rollout(tp0, tv0, tpar, torch.tensor(np.asarray(ring, np.float64)), T, dt, count)
    loss = (pT * torch.tensor(np.asarray(g_pT, np.float32))).sum() + (vT * torch.tensor(np.asarray(g_vT, np.float32))).sum()
    if g_hist is not None and T > 0:
        loss = loss + (hist * torch.tensor(np.asarray(g_hist, np.float32))).sum()
    if loss.requires_grad:
        loss.backward()
    z = lambda t: t.grad.numpy() if t.grad is not None else np.zeros(tuple(t.shape))      # noqa: E731
    return dict(pT=pT.detach().numpy(), vT=vT.detach().numpy(), hist=hist.detach().numpy(), g_p0=z(tp0), g_v0=z(tv0), g_params=z(tpar))


def tail_image(p_tail, ring):
    """The position the head sees the tail at: (float)((double)p_tail + ring), numpy, ring broadcast over the leading axes."""
    return (np.asarray(p_tail, np.float32).astype(np.float64) + np.asarray(ring, np.float64)).astype(np.float32)
