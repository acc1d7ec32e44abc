"""References for the forward-mode tangent sweep of the fused IDM rollout (dhts_micro_rollout_jvp), shared by tests/test_micro_jvp.py and
tests/test_micro_jvp_gpu.py.

chain: the tangent recurrence of ONE lane in numpy on dqs-layout blocks [T][V][2][2][2] (dqs[t][i][0] = dEgo, dqs[t][i][1] = dLeading,
row-major 2 x 2 in (p, v)) -- the oracle's micro_rollout_fwd tape, or blocks expanded from the device's compact tape (expand) -- in the
kernel's float32 operations, with its virtual-leader rule for the head vehicle: the head (slot n - 1) follows (p + head_dp, v - head_dv),
    t_pl = (float)((double)t_p + t_head[0])        t_vl = (float)((double)t_v - t_head[1]).
yardstick: torch.func.jvp in float64 of lane_rollout (tests/test_micro_params.py, validated there against the reference's goldens and the
oracle), the restatement of the plain MicroLane the parameter gradient is tested with; every leaf has a tangent there, the driver
parameters included.  It passes slots at or beyond count through (their tangents come back as they went in); the device returns 0."""
import numpy as np

F, D = np.float32, np.float64


def dot2(a0, b0, a1, b1):
    """csrc/arz_device.hpp dot2 in float32: fma(a1, b1, a0 * b0).  The product a0 b0 is rounded to float32; the fused multiply-add is
    evaluated in float64 (a product of two float32 numbers is exact there) and rounded once to float32."""
    prod = (np.asarray(a0, F) * np.asarray(b0, F)).astype(F)
    return (np.asarray(a1, F).astype(D) * np.asarray(b1, F).astype(D) + prod.astype(D)).astype(F)


def expand(tape, L, V, T, dt):
    """The device's compact tape (float32 [T][L][Vp][3] = e2, e3, l3) -> dqs [T][L][V][2][2][2] as the reverse sweep re-inserts the
    constants: dEgo = [[1, dt], [e2, e3]], dLeading = [[0, 0], [-e2, l3]]."""
    Vp = (V + 63) // 64 * 64
    c = np.asarray(tape, F).reshape(T, L, Vp, 3)[:, :, :V]
    dqs = np.zeros((T, L, V, 2, 2, 2), F)
    dqs[..., 0, 0, 0], dqs[..., 0, 0, 1] = 1.0, F(dt)
    dqs[..., 0, 1, 0], dqs[..., 0, 1, 1] = c[..., 0], c[..., 1]
    dqs[..., 1, 1, 0], dqs[..., 1, 1, 1] = -c[..., 0], c[..., 2]
    return dqs


def chain(dqs, t_p, t_v, t_head=None, n=None):
    """One lane: dqs [T][V][2][2][2] float32, t_p, t_v [V], t_head (t_head_dp, t_head_dv) float64 or None, n = vehicles on the lane
    (None: V).  Returns (t_pT [V], t_vT [V], t_hist [T][2][V]) float32; slots at or beyond n are 0.  The first rows of the blocks are
    the constants [1, dt] and [0, 0] (the leader's tangents enter the speed only)."""
    dqs = np.asarray(dqs, F)
    T, V = dqs.shape[:2]
    n = V if n is None else int(n)
    th = np.zeros(2, D) if t_head is None else np.asarray(t_head, D)
    tp, tv = np.zeros(V, F), np.zeros(V, F)
    tp[:n], tv[:n] = np.asarray(t_p, F)[:n], np.asarray(t_v, F)[:n]
    hist = np.zeros((T, 2, V), F)
    for t in range(T if n > 0 else 0):
        E, Ld = dqs[t, :n, 0], dqs[t, :n, 1]
        a, b = tp[:n], tv[:n]
        al, bl = np.empty(n, F), np.empty(n, F)
        al[:-1], bl[:-1] = a[1:], b[1:]
        al[-1], bl[-1] = F(D(a[-1]) + th[0]), F(D(b[-1]) - th[1])
        n_p = dot2(E[:, 0, 0], a, E[:, 0, 1], b)
        n_v = (dot2(E[:, 1, 0], a, E[:, 1, 1], b) + dot2(Ld[:, 1, 0], al, Ld[:, 1, 1], bl)).astype(F)
        tp[:n], tv[:n] = n_p, n_v
        hist[t, 0], hist[t, 1] = tp, tv
    return tp, tv, hist


def yardstick(p0, v0, params, head, T, dt, count=None, t_p0=None, t_v0=None, t_params=None, t_head=None):
    """One direction through torch.func.jvp of lane_rollout: p0, v0 [L][V] float32, params [6][L][V], head [L][2] float64 and their
    tangents (None: zero).  Returns a dict of numpy arrays: pT, vT, hist and t_pT, t_vT [L][V], t_hist [T][L][2][V]."""
    import torch
    from test_micro_params import lane_rollout
    prim = (torch.tensor(np.asarray(p0, F)), torch.tensor(np.asarray(v0, F)), torch.tensor(np.asarray(params, D)),
            torch.tensor(np.asarray(head, D)))
    tang = tuple(torch.zeros_like(x) if t is None else torch.tensor(np.asarray(t, x.numpy().dtype))
                 for x, t in zip(prim, (t_p0, t_v0, t_params, t_head)))
    out, t = torch.func.jvp(lambda p, v, a, h: lane_rollout(p, v, a, h, T, dt, count), prim, tang)
    return dict(pT=out[0].numpy(), vT=out[1].numpy(), hist=out[2].numpy(), t_pT=t[0].numpy(), t_vT=t[1].numpy(), t_hist=t[2].numpy())


def live_mask(L, V, count):
    return np.arange(V)[None, :] < (np.full(L, V) if count is None else np.asarray(count))[:, None]


def plane_errors(got, ref, live):
    """Norm-relative error max |got - ref| / max |ref| over the live slots of one output plane (float64)."""
    g, r = np.asarray(got, D)[live], np.asarray(ref, D)[live]
    if g.size == 0:
        return 0.0
    return float(np.max(np.abs(g - r)) / max(float(np.max(np.abs(r))), 1e-30))


def compare(tag, got, ref, count, tol):
    """got, ref: dicts with t_pT, t_vT [L][V] and optionally t_hist [T][L][2][V].  Live slots against the reference within tol,
    norm-relative per output plane (t_p, t_v, and the two planes of the history); slots at or beyond count exactly 0 in `got`.
    Prints every figure before it asserts; returns the worst one."""
    L, V = np.asarray(ref["t_pT"]).shape
    live = live_mask(L, V, count)
    planes = [("t_pT", got["t_pT"], ref["t_pT"], live), ("t_vT", got["t_vT"], ref["t_vT"], live)]
    if got.get("t_hist") is not None and np.asarray(got["t_hist"]).shape[0] > 0:
        T = np.asarray(got["t_hist"]).shape[0]
        lt = np.broadcast_to(live[None], (T, L, V))
        planes += [("t_hist p", np.asarray(got["t_hist"])[:, :, 0], np.asarray(ref["t_hist"])[:, :, 0], lt),
                   ("t_hist v", np.asarray(got["t_hist"])[:, :, 1], np.asarray(ref["t_hist"])[:, :, 1], lt)]
    errs = []
    for name, g, r, m in planes:
        e = plane_errors(g, r, m)
        errs.append(e)
        print("%s %s: max |d| / max |ref| = %.2e" % (tag, name, e))
    for name, g, r, m in planes:
        assert np.all(np.asarray(g)[~m] == 0), "%s %s: a slot at or beyond count is not exactly 0" % (tag, name)
    for (name, _, _, _), e in zip(planes, errs):
        assert e <= tol, "%s %s: %.2e > %.1e" % (tag, name, e, tol)
    return max(errs) if errs else 0.0
