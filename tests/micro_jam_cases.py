"""Stop-and-go inputs of the IDM rollout and a census of the branches they reach, shared by tests/test_micro_jam.py (no GPU) and
tests/test_micro_jam_gpu.py.  Every other micro test runs on the collision-free lanes() of tests/test_micro_params_gpu.py, where no
vehicle meets a clip; here the acceleration clip (acc < -v / dt: the vehicle stops at exactly 0 and the step holds no parameter), the
spacing clip (s* < 0) and, in a family of its own, the collision rule fire at many vehicle-steps.

A case is (p0, v0, params, boundary, count, T, dt) as numpy arrays with a fixed seed, plus its kind: "head" (boundary = head [L][2]
float64, lane_rollout of tests/test_micro_params.py), "lead" (boundary = lead [T][L][2] float32, lead_rollout of
tests/micro_lead_ref.py) or "ring" (boundary = ring [L] float64, ring_rollout of tests/micro_ring_ref.py).

census() runs that float64 restatement without autograd and re-decides every branch of every vehicle-step from the states it went
through, with the relative decision margins
    |acc - floor| / (|acc| + |floor|)                       of moving vehicles (the acceleration clip),
    |s_raw| / (s0 + v T + |v dv| / (2 sqrt(a b)))           (the spacing clip).
The device decides in double with a reciprocal in place of a division; a margin of 1e-4 is nine orders of magnitude above what
separates the two, so that no branch of a clean case can be taken differently by a correct kernel."""
import collections

import numpy as np

from test_micro_params_gpu import DEFAULT, lanes

Case = collections.namedtuple("Case", "name kind p0 v0 params boundary count T dt")
MARGIN = 1e-4


def jam_counts(V, L):
    """Ragged counts as counts(V) of tests/test_micro_ring_gpu.py, the long lanes first: a full lane, an empty one, half a lane, then
    two vehicles and one."""
    return [min(c, V) for c in (V, 0, V // 2, 2, 1)][:L]


# =================================================================================================================
# the builders
# =================================================================================================================
def stop_wave(seed, L, V, T, dt, name=None):
    """lanes() with the head gap (0.5, 0): the head vehicle stops at once and a stop wave runs upstream."""
    rng = np.random.default_rng(seed)
    p0, v0, par, head = lanes(rng, L, V)
    head[:] = (0.5, 0.0)
    return Case(name or "stop_wave_V%d_T%d" % (V, T), "head", p0, v0, par, head, jam_counts(V, L), T, dt)


def pull_away_lanes(rng, L, V):
    """Default drivers with min_space in [0.3, 0.8] and time_pref in [0.05, 0.15]; every third vehicle starts at 10 to 14 m/s, the
    others at 24 to 28 m/s: a vehicle behind a slow one closes in (no clip yet), a slow one behind a fast one sees its leader pull
    away by more than 2 sqrt(a b) (s0 + v T) / v, and its desired spacing is negative: the spacing clip."""
    p0 = (np.arange(V)[None, :] * 20.0 + rng.uniform(0, 10, (L, V))).astype(np.float32)
    slow = (np.arange(V)[None, :] + np.arange(L)[:, None]) % 3 == 0
    v0 = np.where(slow, rng.uniform(10, 14, (L, V)), rng.uniform(24, 28, (L, V))).astype(np.float32)
    par = np.tile(DEFAULT[:, None, None], (1, L, V))
    par[3] = rng.uniform(0.3, 0.8, (L, V))
    par[4] = rng.uniform(0.05, 0.15, (L, V))
    par[5] = rng.uniform(4.0, 6.0, (L, V))
    return p0, v0, par


def pull_away(seed, L, V, T, dt, name=None):
    """pull_away_lanes behind a stopped head: both clips."""
    rng = np.random.default_rng(seed)
    p0, v0, par = pull_away_lanes(rng, L, V)
    head = np.tile(np.array([[0.5, 0.0]]), (L, 1))
    return Case(name or "pull_away_V%d_T%d" % (V, T), "head", p0, v0, par, head, jam_counts(V, L), T, dt)


def jammed_ring(seed, L, V, T, dt, room=8.0, pull=False, name=None):
    """Lanes closed to a ring whose circumference leaves the head about `room` metres to the image of the tail, and a tail that
    stands at first and crawls (a target speed of 1 m/s): the head brakes to a stop behind it and the jam runs back through the
    followers, while the tail's own cotangent is handed to a head that is clipped.  The lanes are lanes() with lengths of their own
    (the acceleration clip), or with `pull` pull_away_lanes (the spacing clip as well)."""
    rng = np.random.default_rng(seed)
    if pull:
        p0, v0, par = pull_away_lanes(rng, L, V)
    else:
        p0, v0, par, _ = lanes(rng, L, V)
        par[5] = rng.uniform(4.0, 6.0, (L, V))
    v0[:, 0], par[2, :, 0] = 0.0, 1.0
    cnt = jam_counts(V, L)
    ring = np.array([(float(p0[l, c - 1]) - float(p0[l, 0]) if c > 0 else 0.0) + 0.5 * (par[5, l, 0] + par[5, l, max(c - 1, 0)])
                     + room + rng.uniform(-1.0, 1.0) for l, c in enumerate(cnt)])
    return Case(name or "ring_V%d_T%d" % (V, T), "ring", p0, v0, par, ring, cnt, T, dt)


def braking_leader(seed, L, V, T, dt, name=None):
    """lanes() behind a recorded leader that starts 25 m in front of the head vehicle at 15 m/s, brakes with 4 to 6 m/s^2 to a stop
    and stays there."""
    rng = np.random.default_rng(seed)
    p0, v0, par, _ = lanes(rng, L, V)
    cnt = jam_counts(V, L)
    dec = rng.uniform(4.0, 6.0, L)
    v = np.maximum(15.0 - dec[None, :] * dt * np.arange(T)[:, None], 0.0)
    start = np.array([float(p0[l, c - 1]) + 25.0 if c > 0 else 10.0 for l, c in enumerate(cnt)])
    p = start[None, :] + np.concatenate([np.zeros((1, L)), np.cumsum(v[:-1] * dt, 0)], 0)
    lead = np.stack([p, v], -1).astype(np.float32)
    return Case(name or "lead_V%d_T%d" % (V, T), "lead", p0, v0, par, lead, cnt, T, dt)


# =================================================================================================================
# the restatement and the census
# =================================================================================================================
def rollout(case, p0, v0, params, boundary):
    """The float64 restatement of the case's kind on torch tensors -> (pT, vT, hist), differentiable."""
    from micro_lead_ref import lead_rollout
    from micro_ring_ref import ring_rollout
    from test_micro_params import lane_rollout
    if case.kind == "head":
        return lane_rollout(p0, v0, params, boundary, case.T, case.dt, case.count)
    if case.kind == "lead":
        return lead_rollout(p0, v0, params, boundary, case.T, case.dt, case.count)
    return ring_rollout(p0, v0, params, boundary, case.T, case.dt, case.count)


def leaves(case, grad=True):
    """The case's inputs as torch leaves: p0, v0 float32, params float64, the boundary in its own type (a ring is data)."""
    import torch
    b32 = case.kind == "lead"
    return (torch.tensor(case.p0, requires_grad=grad), torch.tensor(case.v0, requires_grad=grad),
            torch.tensor(case.params, dtype=torch.float64, requires_grad=grad),
            torch.tensor(np.asarray(case.boundary, np.float32 if b32 else np.float64), requires_grad=grad and case.kind != "ring"))


class Restated:
    """The restatement's run of a case with its autograd graph, computed once and left unchanged (restated(case)): pT, vT, hist as
    numpy arrays, and grads(loss_of) = the gradients of loss_of(pT, vT, hist), a torch scalar, as numpy arrays g_p0, g_v0 [L][V],
    g_params [6][L][V], g_boundary (g_head [L][2] / g_lead [T][L][2]; None on a ring)."""

    def __init__(self, case):
        self.case = case
        self.x = leaves(case)
        self.out = rollout(case, *self.x)
        self.pT, self.vT, self.hist = (t.detach().numpy() for t in self.out)

    def grads(self, loss_of):
        import torch
        diff = [t for t in self.x if t.requires_grad]
        g = list(torch.autograd.grad(loss_of(*self.out), diff, retain_graph=True, allow_unused=True))
        g = [np.zeros(tuple(t.shape)) if y is None else y.numpy() for t, y in zip(diff, g)] + [None]
        return dict(g_p0=g[0], g_v0=g[1], g_params=g[2], g_boundary=g[3])


_restated = {}


def restated(case):
    if case.name not in _restated:
        _restated[case.name] = Restated(case)
    return _restated[case.name]


def linear_loss(g_pT, g_vT, g_third=None, device=None):
    """out -> <g_pT, pT> + <g_vT, vT> [+ <g_third, the third output>] for torch outputs on `device`; a None cotangent is left out."""
    import torch
    gs = [None if g is None else torch.tensor(np.ascontiguousarray(g, np.float32), device=device) for g in (g_pT, g_vT, g_third)]

    def loss_of(*out):
        return sum((o * g).sum() for o, g in zip(out, gs) if g is not None)
    return loss_of


def cotangents(case):
    """Random cotangents of pT, vT [L][V] and of the history [T][L][2][V], float32, zero at slots at or beyond count."""
    rng = np.random.default_rng(7)
    L, V = case.p0.shape
    live = live_mask(case)
    g_pT, g_vT = (rng.standard_normal((2, L, V)) * live).astype(np.float32)
    return g_pT, g_vT, (rng.standard_normal((case.T, L, 2, V)) * live[None, :, None, :]).astype(np.float32)


def reference(case, g_pT=None, g_vT=None, g_hist=None):
    """The restatement's states and, with cotangents, its autograd gradients: dict of numpy arrays."""
    r = restated(case)
    out = dict(pT=r.pT, vT=r.vT, hist=r.hist)
    if g_pT is not None or g_vT is not None or g_hist is not None:
        out.update(r.grads(linear_loss(g_pT, g_vT, g_hist)))
    return out


# =================================================================================================================
# the yardstick's own error
# =================================================================================================================
def rollout_unrounded_cotangents(case, p0, v0, params, boundary):
    """The three restatements on float64 leaves with the float32 store as a straight-through rounding: the forward is theirs bit for
    bit, the backward carries every cotangent and the forward mode every tangent in double.  (The restatements -- and the device --
    round the state's cotangents and tangents to float32 once per step; what that rounding is worth is the yardstick's own error.)"""
    import torch

    class Store32(torch.autograd.Function):
        @staticmethod
        def forward(x):
            return x.float().double()

        @staticmethod
        def setup_context(ctx, inputs, output):
            pass

        @staticmethod
        def backward(ctx, g):
            return g

        @staticmethod
        def jvp(ctx, t):
            return t

    L, V = p0.shape
    idx = torch.arange(V)[None, :]
    n = torch.as_tensor(case.count, dtype=torch.int64)[:, None]
    live, is_head = idx < n, idx == n - 1
    a, b, vt, s0, tp, ln = params
    ln_front = torch.cat([ln[:, 1:], ln[:, -1:]], 1)
    if case.kind == "lead":
        ln_front = torch.where(is_head, ln.detach(), ln_front)
    elif case.kind == "ring":
        ln_front = torch.where(is_head, ln[:, 0:1].expand(L, V), ln_front)
    eps, zero = torch.tensor(1e-5, dtype=torch.float64), torch.tensor(0.0, dtype=torch.float64)
    p, v, hist = p0, v0, []
    for t in range(case.T):
        pl, vl = torch.cat([p[:, 1:], p[:, -1:]], 1), torch.cat([v[:, 1:], v[:, -1:]], 1)
        if case.kind == "lead":
            pl, vl = torch.where(is_head, boundary[t][:, 0:1], pl), torch.where(is_head, boundary[t][:, 1:2], vl)
        elif case.kind == "ring":
            pl, vl = torch.where(is_head, Store32.apply(p[:, 0:1] + boundary.detach()[:, None]), pl), torch.where(is_head, v[:, 0:1], vl)
        gap, dv = (pl - p).abs() - (ln_front + ln) * 0.5, v - vl
        if case.kind == "head":
            gap, dv = torch.where(is_head, boundary[:, 0:1], gap), torch.where(is_head, boundary[:, 1:2], dv)
        hit = gap < 0
        gap, dv = torch.where(hit, zero, gap), torch.where(hit, zero, dv)
        gap = torch.where(eps > gap, eps, gap)
        s = s0 + v * tp + (v * dv) / (2 * (a * b) ** 0.5)
        s = torch.where(s < 0, zero, s)
        acc = a * (1.0 - (v / vt) ** 4 - (s / gap) ** 2)
        floor = -v / case.dt
        acc = torch.where(acc < floor, floor, acc)
        p, v = torch.where(live, Store32.apply(p + case.dt * v), p), torch.where(live, Store32.apply(v + case.dt * acc), v)
        hist.append(torch.stack([p, v], 1))
    return p, v, torch.stack(hist)


def own_error(case):
    """The float32 rounding of the cotangents in the yardstick's gradients under cotangents(case): [(lane, plane name, max |difference| /
    max |plane|)] for g_p0, g_v0 and the six parameter planes of every non-empty lane, against rollout_unrounded_cotangents; and
    whether that rollout's history is the restatement's bit for bit."""
    import torch
    from test_micro_params import PLANES
    g = cotangents(case)
    ref = reference(case, *g)
    x = [torch.tensor(np.asarray(t, np.float64), requires_grad=True) for t in (case.p0, case.v0, case.params)]
    out = rollout_unrounded_cotangents(case, *x, torch.tensor(np.asarray(case.boundary, np.float64)))
    same = np.array_equal(out[2].detach().numpy().astype(np.float32), ref["hist"])
    sum((y * torch.tensor(c).double()).sum() for y, c in zip(out, g)).backward()
    exact = dict(g_p0=x[0].grad.numpy(), g_v0=x[1].grad.numpy(), g_params=x[2].grad.numpy())
    rows = []
    for lane, cnt in enumerate(case.count):
        planes = [("g_p0", ref["g_p0"][lane], exact["g_p0"][lane]), ("g_v0", ref["g_v0"][lane], exact["g_v0"][lane])]
        planes += [(name, ref["g_params"][q, lane], exact["g_params"][q, lane]) for q, name in enumerate(PLANES)]
        rows += [(lane, name, float(np.abs(r - e)[:cnt].max() / np.abs(e[:cnt]).max())) for name, r, e in planes if cnt and np.any(e[:cnt])]
    return rows, same


_own_forward = {}


def own_error_forward(case, k):
    """own_error for forward mode: direction k of directions(case, .) through torch.func.jvp of the restatement against the same
    direction with every tangent carried in double: [(lane, plane name, max |difference| / max |plane|)] for t_pT, t_vT and the two
    planes of t_hist; planes that are rounding noise in both (below 1e-12 of the loudest lane's) are left out, as quiet_plane has it."""
    import torch
    if (case.name, k) in _own_forward:
        return _own_forward[(case.name, k)]
    ref = reference_jvp(case, k)
    t = [None if a is None else a[k] for a in directions(case, k + 1)]
    prim = [torch.tensor(np.asarray(a, np.float64)) for a in (case.p0, case.v0, case.params, case.boundary)]
    tang = [torch.zeros_like(x) if a is None else torch.tensor(np.asarray(a, np.float64)) for x, a in zip(prim, t)]
    _, ex = torch.func.jvp(lambda p, v, a, b: rollout_unrounded_cotangents(case, p, v, a, b), tuple(prim), tuple(tang))
    ex = dict(t_pT=ex[0].numpy(), t_vT=ex[1].numpy(), t_hist=ex[2].numpy())
    rows = []
    for name, r, e in (("t_pT", ref["t_pT"], ex["t_pT"]), ("t_vT", ref["t_vT"], ex["t_vT"]),
                       ("t_hist p", ref["t_hist"][:, :, 0], ex["t_hist"][:, :, 0]), ("t_hist v", ref["t_hist"][:, :, 1], ex["t_hist"][:, :, 1])):
        for lane, cnt in enumerate(case.count):
            rl, el = np.take(r, lane, -2)[..., :cnt], np.take(e, lane, -2)[..., :cnt]
            if cnt and not quiet_plane(el, e):
                rows.append((lane, name, float(np.abs(rl - el).max() / np.abs(el).max())))
    _own_forward[(case.name, k)] = rows
    return rows


TANGENT_PLANES = ("t_pT", "t_vT", "t_hist p", "t_hist v")


def tangent_criteria(case, k):
    """How direction k of the yardstick can judge each tangent plane of each non-empty lane: {(lane, plane): criterion}.
      "zero"     the plane is exactly 0 in the yardstick (nothing of the direction reaches it): exactly 0 on the device
      "lane"     the yardstick's own float32 rounding moves it by at most 1e-5 (TOL_GRAD / 10) of the lane's own maximum: held against that
      "loudest"  it moves it by more, or the plane is rounding noise (quiet_plane): held against the loudest lane of the same output"""
    ref = reference_jvp(case, k)
    own = {(lane, name): e for lane, name, e in own_error_forward(case, k)}
    planes = dict(zip(TANGENT_PLANES, (ref["t_pT"], ref["t_vT"], ref["t_hist"][:, :, 0], ref["t_hist"][:, :, 1])))
    out = {}
    for lane, cnt in enumerate(case.count):
        for name in TANGENT_PLANES if cnt else ():
            if not np.any(np.take(planes[name], lane, -2)[..., :cnt]):
                out[(lane, name)] = "zero"
            else:
                out[(lane, name)] = "lane" if own.get((lane, name), 1.0) <= 1e-5 else "loudest"
    return out


def quiet_plane(lane_plane, all_lanes):
    """A lane's plane that holds nothing but rounding noise: below 1e-12 of the same quantity's maximum over all lanes (a lane at rest,
    whose v + dt (-v / dt) leaves 1e-17 of a tangent where the device leaves exactly 0)."""
    return float(np.abs(lane_plane).max(initial=0.0)) <= 1e-12 * float(np.abs(all_lanes).max(initial=0.0))


# =================================================================================================================
# forward mode
# =================================================================================================================
def directions(case, K):
    """K directions of the differentiable leaves: t_p0, t_v0 [K][L][V] float32, t_params [K][6][L][V] float64 (scaled: a parameter's
    unit tangent moves a lane far more than a state's) and the boundary's (t_head [K][L][2] float64, t_lead [K][T][L][2] float32, None
    on a ring).  Direction 0 moves every leaf, 1 the state alone, 2 the parameters alone, 3 the boundary alone (on a ring: every leaf
    again), the others every leaf.  Direction k does not depend on K."""
    L, V = case.p0.shape
    t_p0, t_v0, t_par = np.zeros((K, L, V), np.float32), np.zeros((K, L, V), np.float32), np.zeros((K, 6, L, V))
    t_b = None if case.kind == "ring" else (np.zeros((K, L, 2)) if case.kind == "head" else np.zeros((K, case.T, L, 2), np.float32))
    for k in range(K):
        rng = np.random.default_rng(2000 + k)
        a, b = rng.standard_normal((2, L, V)).astype(np.float32)
        q = 0.1 * rng.standard_normal((6, L, V))
        e = None if t_b is None else (0.1 * rng.standard_normal(t_b.shape[1:])).astype(t_b.dtype)
        every = k not in (1, 2, 3) or (k == 3 and t_b is None)
        if every or k == 1:
            t_p0[k], t_v0[k] = a, b
        if every or k == 2:
            t_par[k] = q
        if t_b is not None and (every or k == 3):
            t_b[k] = e
    return t_p0, t_v0, t_par, t_b


_jvp = {}


def reference_jvp(case, k):
    """Direction k of directions(case, .) through torch.func.jvp of the case's restatement, computed once -> dict t_pT, t_vT [L][V],
    t_hist [T][L][2][V]."""
    import torch
    if (case.name, k) not in _jvp:
        t_p0, t_v0, t_par, t_b = (None if t is None else t[k] for t in directions(case, k + 1))
        prim = leaves(case, grad=False)
        tang = [torch.tensor(np.asarray(t, x.numpy().dtype)) for x, t in zip(prim[:3], (t_p0, t_v0, t_par))]
        if case.kind == "ring":
            _, t = torch.func.jvp(lambda p, v, a: rollout(case, p, v, a, prim[3]), prim[:3], tuple(tang))
        else:
            tang.append(torch.tensor(np.asarray(t_b, prim[3].numpy().dtype)))
            _, t = torch.func.jvp(lambda p, v, a, b: rollout(case, p, v, a, b), prim, tuple(tang))
        _jvp[(case.name, k)] = dict(t_pT=t[0].numpy(), t_vT=t[1].numpy(), t_hist=t[2].numpy())
    return _jvp[(case.name, k)]


def adjoint_gap(g, jt, grads, tangents):
    """(<g, J t>, <J^T g, t>, sum of the absolute terms of the first), in double; a None pair is left out."""
    d = lambda a: np.asarray(a, np.float64).ravel()      # noqa: E731
    fwd = np.concatenate([d(x) * d(y) for x, y in zip(g, jt) if x is not None and y is not None])
    rev = np.concatenate([d(x) * d(y) for x, y in zip(grads, tangents) if x is not None and y is not None])
    return fwd.sum(), rev.sum(), np.abs(fwd).sum()


def live_mask(case):
    L, V = case.p0.shape
    return np.arange(V)[None, :] < np.asarray(case.count)[:, None]


_census = {}


def census(case):
    """Every vehicle-step of the restatement's run of `case`, re-decided in float64 numpy from the states before the step.  Returns a
    dict of [T][L][V] arrays, False / inf at slots at or beyond count: clip_a, clip_s, collided, small_gap (raw gap < 1e-5, collisions
    included), stopped (v == 0 AFTER the step: what the history shows), moving (v != 0 before it), margin_a (moving vehicles), margin_s;
    `hist` [T][L][2][V] the restatement's history and `head` [L][V] the head slots.  Computed once per case name."""
    if case.name in _census:
        return _census[case.name]
    import torch
    with torch.no_grad():
        hist = rollout(case, *leaves(case, grad=False))[2].numpy()
    T, dt = case.T, case.dt
    L, V = case.p0.shape
    live = live_mask(case)
    is_head = np.arange(V)[None, :] == (np.asarray(case.count)[:, None] - 1)
    a, b, vt, s0, tp, ln = np.asarray(case.params, np.float64)
    pb = np.concatenate([case.p0[None], hist[:T - 1, :, 0]], 0).astype(np.float64)              # the states before step t
    vb = np.concatenate([case.v0[None], hist[:T - 1, :, 1]], 0).astype(np.float64)
    pl, vl = np.concatenate([pb[..., 1:], pb[..., -1:]], -1), np.concatenate([vb[..., 1:], vb[..., -1:]], -1)
    ln_front = np.concatenate([ln[:, 1:], ln[:, -1:]], 1)
    if case.kind == "head":
        gap = np.where(is_head, case.boundary[:, 0:1], np.abs(pl - pb) - (ln_front + ln) * 0.5)
        dv = np.where(is_head, case.boundary[:, 1:2], vb - vl)
    else:
        if case.kind == "lead":
            lead = np.asarray(case.boundary, np.float64)
            pl, vl = np.where(is_head, lead[:, :, 0:1], pl), np.where(is_head, lead[:, :, 1:2], vl)
            ln_front = np.where(is_head, ln, ln_front)
        else:
            image = (pb[..., 0:1] + np.asarray(case.boundary)[None, :, None]).astype(np.float32).astype(np.float64)
            pl, vl = np.where(is_head, image, pl), np.where(is_head, vb[..., 0:1], vl)
            ln_front = np.where(is_head, ln[:, 0:1], ln_front)
        gap, dv = np.abs(pl - pb) - (ln_front + ln) * 0.5, vb - vl
    collided = gap < 0
    small = gap < 1e-5
    g, d = np.where(collided, 0.0, gap), np.where(collided, 0.0, dv)
    g = np.maximum(g, 1e-5)
    kin = np.abs(vb * d) / (2 * np.sqrt(a * b))
    s_raw = s0 + vb * tp + (vb * d) / (2 * np.sqrt(a * b))
    clip_s = s_raw < 0
    s = np.where(clip_s, 0.0, s_raw)
    acc = a * (1.0 - (vb / vt) ** 4 - (s / g) ** 2)
    floor = -vb / dt
    clip_a = acc < floor
    moving = vb != 0
    with np.errstate(all="ignore"):
        margin_a = np.where(moving, np.abs(acc - floor) / (np.abs(acc) + np.abs(floor)), np.inf)
        margin_s = np.abs(s_raw) / (s0 + vb * tp + kin)
    lt = np.broadcast_to(live[None], (T, L, V))
    on = lambda x: np.where(lt, x, False)                 # noqa: E731
    c = dict(clip_a=on(clip_a), clip_s=on(clip_s), collided=on(collided), small_gap=on(small), stopped=on(hist[:, :, 1] == 0),
             moving=on(moving), margin_a=np.where(lt, margin_a, np.inf), margin_s=np.where(lt, margin_s, np.inf), hist=hist,
             head=is_head & live)
    _census[case.name] = c
    return c


def summary(case):
    """One line of counts for a test log."""
    c = census(case)
    followers = c["clip_a"] & ~c["head"][None]
    return ("%s (%s, L=%d V=%d T=%d dt=%g count=%s): acceleration clips %d (%d on followers, %d vehicles), spacing clips %d (%d vehicles), "
            "collided %d, gap < 1e-5 %d, v == 0 %d, margins %.1e %.1e"
            % (case.name, case.kind, case.p0.shape[0], case.p0.shape[1], case.T, case.dt, case.count, c["clip_a"].sum(), followers.sum(),
               followers.any(0).sum(), c["clip_s"].sum(), c["clip_s"].any(0).sum(), c["collided"].sum(), c["small_gap"].sum(),
               c["stopped"].sum(), c["margin_a"].min(), c["margin_s"].min()))


def longest_standstill(case):
    """The longest run of consecutive steps some live vehicle ends at v == 0, and whether some vehicle moves again after one."""
    st = census(case)["stopped"]
    best, run = 0, np.zeros(st.shape[1:], int)
    for t in range(st.shape[0]):
        run = np.where(st[t], run + 1, 0)
        best = max(best, int(run.max()))
    live = np.broadcast_to(live_mask(case)[None], st.shape)
    restarts = bool(np.any(st[:-1] & ~st[1:] & live[1:]))
    return best, restarts


def first_collision(case):
    """(step, lane, slot) of the first collision in the order the library's record keeps: the lowest step, then lane, then slot."""
    idx = np.argwhere(census(case)["collided"])
    return None if len(idx) == 0 else tuple(int(x) for x in idx[0])


# =================================================================================================================
# the chosen cases
# =================================================================================================================
# V in {5, 64, 65, 130} (one wavefront, its edge, one slot beyond it, three wavefronts), T in {37, 150}, L in 3 .. 5 with an empty and a
# half-filled lane.  The stop wave needs dt >= 0.1 to leave the head within these steps.  The step sizes are 0.1, 0.2 and 0.25: the
# v == 0 criterion needs the restatement's v + dt (-v / dt) to round back to exactly 0 at every clipped step, which it does at these and
# does not at dt = 0.15.  Every case meets the conditions of tests/test_micro_jam.py; for the braking leader and the large ring that
# includes the yardstick's own error -- every plane of g_p0, g_v0 and g_params of every lane is determined to TOL_GRAD / 10 by float32
# cotangents (the length plane of a short lane is the small difference of two gap sums, and is the plane that decides it there).
def clean_cases():
    return [stop_wave(1, 3, 65, 150, 0.1), stop_wave(2, 3, 130, 37, 0.2), pull_away(3, 5, 64, 150, 0.1), pull_away(4, 3, 5, 37, 0.1),
            jammed_ring(5, 3, 65, 37, 0.25), jammed_ring(8, 3, 130, 150, 0.1, pull=True, name="ring_pull_V130_T150"),
            jammed_ring(5, 3, 5, 37, 0.1, pull=True, name="ring_pull_V5_T37"), braking_leader(48, 3, 65, 150, 0.1)]


CLEAN = clean_cases()
CLEAN_IDS = [c.name for c in CLEAN]
HEAD = [c for c in CLEAN if c.kind == "head"]
RING = [c for c in CLEAN if c.kind == "ring"]
LEAD = [c for c in CLEAN if c.kind == "lead"]


# The stop wave at dt = 0.25: the followers run into the standing queue.  In the first case one vehicle collides (119 vehicle-steps from
# step 31 on), so that "the first collision" is one record whatever thread writes it; in the second six vehicles on two lanes do (414
# vehicle-steps) and the record is the first collision of one of them (the first fault of a launch wins: a race between vehicles).
def collision_cases():
    return [stop_wave(17, 3, 65, 150, 0.25, name="collide_one_V65_T150"), stop_wave(19, 3, 65, 150, 0.25, name="collide_six_V65_T150")]


COLLIDE = collision_cases()
COLLIDE_IDS = [c.name for c in COLLIDE]


# The tangent planes (direction of directions(), lane, plane) that the yardstick itself does not determine to TOL_GRAD / 10 of the lane's
# own maximum (tangent_criteria: "loudest"), so that tests/test_micro_jam_gpu.py holds them against the loudest lane of the output: planes
# of the half-filled lane 2 behind a stop wave or a braking leader, and t_vT of lanes of two vehicles that have all but come to rest.
# tests/test_micro_jam.py checks that these are exactly those planes.
LOUDEST_LANE_PLANES = {
    "stop_wave_V65_T150": {(0, 2, "t_hist p"), (0, 2, "t_hist v"), (0, 2, "t_vT"), (2, 2, "t_hist v")},
    "stop_wave_V130_T37": set(),
    "pull_away_V64_T150": {(1, 2, "t_hist p"), (1, 3, "t_vT"), (3, 3, "t_vT")},
    "pull_away_V5_T37": set(),
    "ring_V65_T37": set(),
    "ring_pull_V130_T150": set(),
    "ring_pull_V5_T37": {(1, 2, "t_vT")},
    "lead_V65_T150": {(2, 0, "t_hist v"), (2, 2, "t_hist v")},
}
