"""The chained oracle of the schedule rollouts (dhts_macro_rollout_fwd_sched / _bwd_sched): T calls of oracle.macro_step per lane over
the N + 2 padded state, the two boundary cells set from row t of the schedule in front of step t, then T calls of
oracle.macro_step_bwd, newest step first, whose entries 0 and N + 1 are the cotangent of that step's boundary cells.  The float32
glue around the steps -- FullQ.from_r_u for the initial state and every boundary cell, the speed tap's and from_r_u's backward -- and
the double (r, y) -> (r, u) formula for the boundary cotangent restate oracle/dhts_oracle.c:269-328 and :538-545 in numpy, operation
for operation; tests/test_macro_sched.py holds them against oracle.macro_rollout_fwd / _bwd (constant schedule: equal states) and
against the reference's own numbers (tests/golden/macro_sched_*.npz).  No GPU, no torch."""
import numpy as np

EPS = 1e-5
F = np.float32


def rsqrt(t):
    """x ** -0.5 of the pow backward, float32.  The one operation of the glue that two faithful float32 evaluations may round differently
    (powf(x, -0.5f) here and in the oracle, 1 / sqrtf(x) on the device); tests/test_macro_sched.py moves it by one ulp."""
    return np.power(t, F(-0.5), dtype=F)


def glue_u_eq(r, um):
    r = np.asarray(r, F)
    t = F(1.0) - np.sqrt(np.maximum(r, F(0)) + F(EPS), dtype=F)
    neg = F(float(um) * (1.0 - (0.0 + EPS) ** 0.5))          # max(r, 0.) picked the Python float: double, cast where it meets a tensor
    return np.where(F(0) > r, neg, F(um) * t).astype(F)


def from_r_u(r, u, um):
    """(y, u_eq) of FullQ.from_r_u in float32."""
    r, u = np.asarray(r, F), np.asarray(u, F)
    q = glue_u_eq(r, um)
    return (r * (u - q)).astype(F), q


def glue_u_bwd(r, y, um, g_u):
    """(g_r, g_y) contributions of a cotangent on u = y / max(r, eps) + u_eq(max(r, eps)) (set_r_y), float32 as autograd evaluates it."""
    r, y, g_u = np.asarray(r, F), np.asarray(y, F), np.asarray(g_u, F)
    small = r < F(EPS)
    rs = np.where(small, F(1), r)
    g_y = np.where(small, g_u / F(EPS), g_u / rs).astype(F)
    gd = (-g_u * ((y / rs) / rs)).astype(F)
    t = rs + F(EPS)
    gp = ((-(g_u * F(um))) * (F(0.5) * rsqrt(t))).astype(F)
    g_r = np.where(small, F(0), gd + gp).astype(F)
    return g_r, g_y


def glue_y_bwd(r, u, um, g_y):
    """(g_r, g_u) contributions of a cotangent on y = r (u - u_eq(r)) (from_r_u), float32."""
    r, u, g_y = np.asarray(r, F), np.asarray(u, F), np.asarray(g_y, F)
    diff = (u - glue_u_eq(r, um)).astype(F)
    g_diff = (g_y * r).astype(F)
    acc = (g_y * diff).astype(F)
    t = np.maximum(r, F(0)) + F(EPS)
    extra = ((-((-g_diff) * F(um))) * (F(0.5) * rsqrt(t))).astype(F)
    return np.where(F(0) > r, acc, acc + extra).astype(F), g_diff


def boundary_ry_to_ru(g_ry, gr, gu, um):
    """Cotangent of the boundary (r, y) [...][2] (double) -> of the boundary leaves (r, u), in double, rounded to float32 at the end."""
    g_ry = np.asarray(g_ry, np.float64)
    rr, uu = np.asarray(gr, F).astype(np.float64), np.asarray(gu, F).astype(np.float64)
    ueq = glue_u_eq(np.asarray(gr, F), um).astype(np.float64)
    dueq = np.where(0.0 > rr, 0.0, -float(um) * 0.5 / np.sqrt(np.maximum(rr, 0.0) + EPS))
    return ((g_ry[..., 0] + g_ry[..., 1] * ((uu - ueq) - rr * dueq)).astype(F), (g_ry[..., 1] * rr).astype(F))


def sched_fwd(O, r0, u0, gr, gu, dt, dx, um):
    """r0, u0 [L][N]; gr, gu [T][L][2].  Returns dict: rT, yT, uT, qT [L][N], hist_r / _y / _u [T][L][N], tape (per lane and step: dqs)."""
    r0, u0, gr, gu = (np.ascontiguousarray(a, F) for a in (r0, u0, gr, gu))
    L, N = r0.shape
    T = gr.shape[0]
    assert gr.shape == (T, L, 2) and gu.shape == (T, L, 2)
    gy, gq = from_r_u(gr, gu, um)
    y0, q0 = from_r_u(r0, u0, um)
    out = dict(T=T, um=um, r0=r0, u0=u0, gr=gr, gu=gu, tape=[[None] * T for _ in range(L)],
               hist_r=np.zeros((T, L, N), F), hist_y=np.zeros((T, L, N), F), hist_u=np.zeros((T, L, N), F))
    fin = np.zeros((4, L, N), F)
    for l in range(L):
        st = np.zeros((4, N + 2), F)
        st[:, 1:-1] = r0[l], y0[l], u0[l], q0[l]
        for t in range(T):
            st[:, 0] = gr[t, l, 0], gy[t, l, 0], gu[t, l, 0], gq[t, l, 0]
            st[:, N + 1] = gr[t, l, 1], gy[t, l, 1], gu[t, l, 1], gq[t, l, 1]
            o = O.macro_step(st, dt, dx, um)
            assert o["rc"] == 0, "the oracle's step fails its CFL check (lane %d, step %d, interface %d)" % (l, t, o["err_index"])
            out["tape"][l][t] = o["dqs"]
            st[:, 1:-1] = o["nr"], o["ny"], o["nu"], o["nueq"]
            out["hist_r"][t, l], out["hist_y"][t, l], out["hist_u"][t, l] = o["nr"], o["ny"], o["nu"]
        fin[:, l] = st[:, 1:-1]
    out["rT"], out["yT"], out["uT"], out["qT"] = fin
    return out


def sched_bwd(O, f, g_rT=None, g_yT=None, g_uT=None, gh_r=None, gh_y=None, gh_u=None):
    """Cotangents of the final (r, y, u) [L][N] and of the state after every step [T][L][N] (None = none).  Returns g_r0, g_u0 [L][N],
    g_ghost_ry [T][L][2][2] float64 (what g_ghost_sched holds) and g_ghost_r, g_ghost_u [T][L][2] float32."""
    L, N = f["r0"].shape
    T, um = f["T"], f["um"]
    g_r0, g_y0 = np.zeros((L, N), F), np.zeros((L, N), F)
    g_ry = np.zeros((T, L, 2, 2), np.float64)
    for l in range(L):
        gr = np.zeros(N, F) if g_rT is None else np.array(g_rT[l], F)
        gy = np.zeros(N, F) if g_yT is None else np.array(g_yT[l], F)
        if g_uT is not None:
            a, b = glue_u_bwd(f["rT"][l], f["yT"][l], um, g_uT[l])
            gr, gy = gr + a, gy + b
        for t in range(T - 1, -1, -1):
            if gh_r is not None:
                gr = gr + np.asarray(gh_r[t, l], F)
            if gh_y is not None:
                gy = gy + np.asarray(gh_y[t, l], F)
            if gh_u is not None:
                a, b = glue_u_bwd(f["hist_r"][t, l], f["hist_y"][t, l], um, gh_u[t, l])
                gr, gy = gr + a, gy + b
            ngr, ngy = O.macro_step_bwd(f["tape"][l][t], gr.astype(F), gy.astype(F))
            g_ry[t, l, 0] = ngr[0], ngy[0]
            g_ry[t, l, 1] = ngr[N + 1], ngy[N + 1]
            gr, gy = ngr[1:-1].copy(), ngy[1:-1].copy()
        g_r0[l], g_y0[l] = gr, gy
    a, g_u0 = glue_y_bwd(f["r0"], f["u0"], um, g_y0)
    g_gr, g_gu = boundary_ry_to_ru(g_ry, f["gr"], f["gu"], um)
    return dict(g_r0=(g_r0 + a).astype(F), g_u0=g_u0, g_ghost_ry=g_ry, g_ghost_r=g_gr, g_ghost_u=g_gu)


def taps(f, tap):
    """The cotangents of the two losses the goldens use: final_sq = sum rT^2 + sum uT^2; every_sum = sum over the steps of r + y + u."""
    if tap == "final_sq":
        return dict(g_rT=2 * f["rT"], g_uT=2 * f["uT"])
    one = np.ones_like(f["hist_r"])
    return dict(gh_r=one, gh_y=one, gh_u=one)
