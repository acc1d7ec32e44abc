"""The chained tangent (forward mode) of the on-ramp rollouts in numpy (dhts_macro_rollout_fwd_jvp_ramp / _ring_ramp): the
float64 chain macro_jvp_ref.chain on the blocks of macro_ramp_ref.ramp_fwd's tape with one change -- behind step s, in front of that
step's detector read, the density tangent of every ramp cell inside [0, N) gets dt * t_inflow[s][l][j]; the source is identity in
(r, y), so nothing else of a step changes.  An open lane takes the boundary cells' tangents as macro_jvp_ref.jvp does, a ring pads with
the opposite end's tangents.  The glue partials are macro_jvp_ref's and are not restated.  No GPU, no torch."""
import numpy as np

from macro_jvp_ref import D, u_partials, y_partials


def ramp_chain(blocks, t_r, t_y, ramps, t_inflow, dt, t_ghost=None, ring=False, det=None):
    """The (r, y) chain of ONE lane.  blocks [T][N][3][2][2]; t_r, t_y [N]; ramps [R] cell indices, t_inflow [T][R]; t_ghost None or
    [T][2 sides][2 (r, y)] (an open lane); ring: the pads are the opposite end's tangents.  det: cells to read.
    Returns (t_r, t_y) after the last step and taps [T][2][len(det)] (post-source)."""
    T = len(blocks)
    t = np.stack([np.asarray(t_r, D), np.asarray(t_y, D)], axis=-1)              # [N][2]
    N = t.shape[0]
    taps = np.zeros((T, 2, 0 if det is None else len(det)), D)
    for s in range(T):
        b = np.asarray(blocks[s], D)
        pad = np.zeros((N + 2, 2), D)
        pad[1:-1] = t
        if ring:
            pad[0], pad[N + 1] = t[N - 1], t[0]
        elif t_ghost is not None:
            pad[0], pad[N + 1] = t_ghost[s][0], t_ghost[s][1]
        t = (np.einsum("kij,kj->ki", b[:, 1], pad[1:-1]) + np.einsum("kij,kj->ki", b[:, 0], pad[:-2])
             + np.einsum("kij,kj->ki", b[:, 2], pad[2:]))
        for j, c in enumerate(ramps):
            if 0 <= c < N:
                t[c, 0] = t[c, 0] + float(dt) * D(t_inflow[s][j])
        if det is not None:
            taps[s] = t[list(det)].T
    return t[:, 0], t[:, 1], taps


def ramp_jvp(f, t_r0=None, t_u0=None, t_gr=None, t_gu=None, t_inflow=None, det=None):
    """f: what macro_ramp_ref.ramp_fwd returns.  Tangents of ONE direction: t_r0, t_u0 [L][N]; t_gr, t_gu [T][L][2] (an open lane; a
    constant boundary: the same row T times); t_inflow [T][L][R]; None = zero.
    Returns dict t_rT, t_yT, t_uT [L][N] and, with det, t_read [T][L][3][len(det)] (post-source), all float64."""
    L, N = f["r0"].shape
    T, um, ramps = f["T"], f["um"], f["ramps"]
    z = np.zeros((L, N), D)
    t_r0 = z if t_r0 is None else np.asarray(t_r0, D)
    t_u0 = z if t_u0 is None else np.asarray(t_u0, D)
    t_in = np.zeros((T, L, len(ramps)), D) if t_inflow is None else np.asarray(t_inflow, D).reshape(T, L, len(ramps))
    a, b = y_partials(f["r0"], f["u0"], um)
    t_y0 = a * t_r0 + b * t_u0
    t_g = None
    if not f["ring"] and (t_gr is not None or t_gu is not None):
        zg = np.zeros((T, L, 2), D)
        t_gr = zg if t_gr is None else np.asarray(t_gr, D)
        t_gu = zg if t_gu is None else np.asarray(t_gu, D)
        a, b = y_partials(f["gr"], f["gu"], um)
        t_g = np.stack([t_gr, a * t_gr + b * t_gu], axis=-1)                    # [T][L][2 sides][2 (r, y)]
    nd = 0 if det is None else len(det)
    out = dict(t_rT=np.zeros((L, N), D), t_yT=np.zeros((L, N), D), t_read=np.zeros((T, L, 3, nd), D))
    for l in range(L):
        out["t_rT"][l], out["t_yT"][l], taps = ramp_chain(f["tape"][l], t_r0[l], t_y0[l], ramps, t_in[:, l], f["dt"],
                                                          None if t_g is None else t_g[:, l], f["ring"], det)
        if det is not None and T:
            out["t_read"][:, l, :2] = taps
            a, b = u_partials(f["hist_r"][:, l][:, list(det)], f["hist_y"][:, l][:, list(det)], um)
            out["t_read"][:, l, 2] = a * taps[:, 0] + b * taps[:, 1]
    a, b = u_partials(f["rT"], f["yT"], um)
    out["t_uT"] = a * out["t_rT"] + b * out["t_yT"]
    return out
