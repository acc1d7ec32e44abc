"""Yardstick of the recorded-leader form of the IDM rollout (dhts.micro_rollout(lead=...)): lane_rollout of tests/test_micro_params.py
with a leader row per step.  The head vehicle (slot count - 1) is an ordinary follower of a prescribed vehicle whose (p, v) in step t is
lead[t]; no head gap exists.  tests/test_micro_lead.py validates it against the C oracle's single step and against the oracle's full
rollout split at a vehicle; tests/test_micro_lead_gpu.py uses it for the one case existing device code cannot reach (a full lane of
1024, whose leader has no slot in a V + 1 yardstick)."""
import numpy as np


def lead_rollout(p0, v0, params, lead, T, dt, count=None, lead_length=None, store32=True):
    """p0, v0 [L][V] float32 torch tensors; params [6][L][V] float64; lead [T][L][2] float32; lead_length [L] float64 or None (the head's
    own length, as a constant: the head's length carries its own share of the gap only); count [L] integers or None.  Arithmetic in
    float64, the state stored as float32 after every step.  Returns pT, vT [L][V] float32 and hist [T][L][2][V] float32, differentiable
    w.r.t. p0, v0, params and lead."""
    import torch
    L, V = p0.shape
    n = torch.full((L,), V, dtype=torch.int64) if count is None else torch.as_tensor(count, dtype=torch.int64)
    idx = torch.arange(V)[None, :]
    live, is_head = idx < n[:, None], idx == (n[:, None] - 1)
    a, b, vt, s0, tp, ln = params
    ln_front = torch.cat([ln[:, 1:], ln[:, -1:]], 1)
    ln_head = ln.detach() if lead_length is None else torch.as_tensor(lead_length, dtype=torch.float64)[:, None].expand(L, V)
    ln_front = torch.where(is_head, ln_head, ln_front)
    eps, zero = torch.tensor(1e-5, dtype=torch.float64), torch.tensor(0.0, dtype=torch.float64)
    p, v, hist = p0, v0, []
    for t in range(T):
        pd, vd = p.double(), v.double()
        pl, vl = torch.cat([pd[:, 1:], pd[:, -1:]], 1), torch.cat([vd[:, 1:], vd[:, -1:]], 1)
        pl = torch.where(is_head, lead[t][:, 0:1].double(), pl)
        vl = torch.where(is_head, lead[t][:, 1:2].double(), vl)
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


def restated_lead(p0, v0, params, lead, T, dt, count=None, lead_length=None, g_pT=None, g_vT=None, g_hist=None):
    """lead_rollout on numpy inputs, differentiated for the given cotangents: dict of numpy arrays."""
    import torch
    tp0 = torch.tensor(np.asarray(p0, np.float32), requires_grad=True)
    tv0 = torch.tensor(np.asarray(v0, np.float32), requires_grad=True)
    tpar = torch.tensor(np.asarray(params, np.float64), requires_grad=True)
    tlead = torch.tensor(np.asarray(lead, np.float32), requires_grad=True)
    pT, vT, hist = lead_rollout(tp0, tv0, tpar, tlead, T, dt, count, lead_length)
    loss = (pT * torch.tensor(np.asarray(g_pT, np.float32))).sum() + (vT * torch.tensor(np.asarray(g_vT, np.float32))).sum()
    if g_hist is not None and T > 0:
        loss = loss + (hist * torch.tensor(np.asarray(g_hist, np.float32))).sum()
    loss.backward()
    z = lambda t: t.grad.numpy() if t.grad is not None else np.zeros(tuple(t.shape))      # noqa: E731
    return dict(pT=pT.detach().numpy(), vT=vT.detach().numpy(), hist=hist.detach().numpy(), g_p0=z(tp0), g_v0=z(tv0), g_params=z(tpar),
                g_lead=z(tlead))


def trajectory_before_steps(x0, hist_x):
    """What a vehicle is seen at IN step t, from its initial value x0 [...] and its value after every step hist_x [T][...]: [T][...]."""
    T = hist_x.shape[0]
    if T == 0:
        return hist_x.copy()
    return np.concatenate([np.asarray(x0)[None], hist_x[:T - 1]], 0)
