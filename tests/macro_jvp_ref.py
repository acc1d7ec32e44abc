"""The chained tangent (forward mode) of the straight-lane rollout in numpy, the counterpart of macro_sched_ref.sched_bwd: tangents of
the leaves (r0, u0, ghost_r, ghost_u) -> tangents of the final (r, y, u) and of (r, y, u) at chosen cells after every step.  The glue
partials (from_r_u in front, the speed tap behind) are evaluated in float64; a step is t'_k = d0 t_{k-1} + d1 t_k + d2 t_{k+1} in float64
on the oracle's float32 blocks dqs [N][3][2][2] (row-major 2 x 2 in (r, y)), the boundary cells' tangents in front of cell 0 and behind
cell N - 1.  tests/test_macro_jvp.py holds it against the oracle adjoint (<g, J t> = <J^T g, t>).  No GPU, no torch."""
import numpy as np

import macro_sched_ref as R

EPS = R.EPS
D = np.float64


def dueq_dr(r, um):
    """d u_eq / d r in float64: zero where max(r, 0.) picked the constant."""
    r = np.asarray(r, D)
    return np.where(0.0 > r, 0.0, -float(um) * 0.5 / np.sqrt(np.maximum(r, 0.0) + EPS))


def y_partials(r, u, um):
    """(dy/dr, dy/du) of y = r (u - u_eq(r)) at float32 (r, u), in float64."""
    r32 = np.asarray(r, np.float32)
    rr, uu = r32.astype(D), np.asarray(u, np.float32).astype(D)
    ueq = R.glue_u_eq(r32, um).astype(D)
    return (uu - ueq) - rr * dueq_dr(rr, um), rr


def u_partials(r, y, um):
    """(du/dr, du/dy) of the speed tap u = y / max(r, eps) + u_eq(max(r, eps)) at float32 (r, y), in float64 (below eps: a constant density)."""
    rr, yy = np.asarray(r, np.float32).astype(D), np.asarray(y, np.float32).astype(D)
    small = rr < np.float32(EPS)
    rs = np.where(small, 1.0, rr)
    return np.where(small, 0.0, -yy / rs / rs + dueq_dr(rs, um)), np.where(small, 1.0 / float(np.float32(EPS)), 1.0 / rs)


def chain(blocks, t_r, t_y, t_ghost=None, det=None):
    """The (r, y) chain of ONE lane.  blocks [T][N][3][2][2]; t_r, t_y [N]; t_ghost None or [T][2 sides][2 (r, y)]; det: cells to read.
    Returns (t_r, t_y) after the last step and, with det, taps [T][2][len(det)]."""
    T = len(blocks)
    t = np.stack([np.asarray(t_r, D), np.asarray(t_y, D)], axis=-1)              # [N][2]
    N = t.shape[0]
    taps = np.zeros((T, 2, 0 if det is None else len(det)), D)
    for s in range(T):
        b = np.asarray(blocks[s], D)
        pad = np.zeros((N + 2, 2), D)
        pad[1:-1] = t
        if t_ghost is not None:
            pad[0], pad[N + 1] = t_ghost[s][0], t_ghost[s][1]
        t = (np.einsum("kij,kj->ki", b[:, 1], pad[1:-1]) + np.einsum("kij,kj->ki", b[:, 0], pad[:-2])
             + np.einsum("kij,kj->ki", b[:, 2], pad[2:]))
        if det is not None:
            taps[s] = t[list(det)].T
    return t[:, 0], t[:, 1], taps


def jvp(f, t_r0=None, t_u0=None, t_gr=None, t_gu=None, det=None, blocks=None):
    """f: what macro_sched_ref.sched_fwd returns (boundary cells [T][L][2]).  Tangents of ONE direction: t_r0, t_u0 [L][N]; t_gr, t_gu
    [T][L][2] (a constant boundary: the same row T times); None = zero.  blocks: [L][T][N][3][2][2] instead of the oracle's.
    Returns dict t_rT, t_yT, t_uT [L][N] and, with det, t_read [T][L][3][len(det)], all float64."""
    L, N = f["r0"].shape
    T, um = f["T"], f["um"]
    z = np.zeros((L, N), D)
    t_r0 = z if t_r0 is None else np.asarray(t_r0, D)
    t_u0 = z if t_u0 is None else np.asarray(t_u0, D)
    a, b = y_partials(f["r0"], f["u0"], um)
    t_y0 = a * t_r0 + b * t_u0
    t_g = None
    if t_gr is not None or t_gu is not None:
        zg = np.zeros((T, L, 2), D)
        t_gr = zg if t_gr is None else np.asarray(t_gr, D)
        t_gu = zg if t_gu is None else np.asarray(t_gu, D)
        a, b = y_partials(f["gr"], f["gu"], um)
        t_g = np.stack([t_gr, a * t_gr + b * t_gu], axis=-1)                    # [T][L][2 sides][2 (r, y)]
    nd = 0 if det is None else len(det)
    out = dict(t_rT=np.zeros((L, N), D), t_yT=np.zeros((L, N), D), t_read=np.zeros((T, L, 3, nd), D))
    for l in range(L):
        bl = f["tape"][l] if blocks is None else blocks[l]
        out["t_rT"][l], out["t_yT"][l], taps = chain(bl, t_r0[l], t_y0[l], None if t_g is None else t_g[:, l], det)
        if det is not None and T:
            out["t_read"][:, l, :2] = taps
            a, b = u_partials(f["hist_r"][:, l][:, list(det)], f["hist_y"][:, l][:, list(det)], um)
            out["t_read"][:, l, 2] = a * taps[:, 0] + b * taps[:, 1]
    a, b = u_partials(f["rT"], f["yT"], um)
    out["t_uT"] = a * out["t_rT"] + b * out["t_yT"]
    return out
