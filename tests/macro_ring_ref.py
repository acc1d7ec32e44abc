"""The chained oracle of the ring rollouts (dhts_macro_rollout_*_ring): macro_sched_ref.sched_fwd / sched_bwd with two changes.  In
front of every step the two padded columns are set from the lane itself, st[:, 0] = st[:, N] (cell N - 1) and st[:, N + 1] = st[:, 1]
(cell 0); in the backward the cotangents oracle.macro_step_bwd leaves in entries 0 and N + 1 are added to cells N - 1 and 0 in front of
the next older step.  The float32 glue is macro_sched_ref's and is not restated.  tests/test_macro_ring.py holds ring_fwd / ring_bwd
against an open lane of three copies of the state.  No GPU, no torch."""
import numpy as np

from macro_sched_ref import F, from_r_u, glue_u_bwd, glue_y_bwd


def ring_fwd(O, r0, u0, T, dt, dx, um, check=True):
    """r0, u0 [L][N].  Returns dict: rT, yT, uT, qT [L][N], hist_r / _y / _u [T][L][N], tape (per lane and step: dqs), and rc: None, or
    (step, lane, interface) of the first step whose CFL check the oracle fails (check=False; the states from there on are not filled)."""
    r0, u0 = (np.ascontiguousarray(a, F) for a in (r0, u0))
    L, N = r0.shape
    y0, q0 = from_r_u(r0, u0, um)
    out = dict(T=T, um=um, r0=r0, u0=u0, rc=None, tape=[[None] * T for _ in range(L)],
               hist_r=np.zeros((T, L, N), F), hist_y=np.zeros((T, L, N), F), hist_u=np.zeros((T, L, N), F))
    fin = np.zeros((4, L, N), F)
    for l in range(L):
        st = np.zeros((4, N + 2), F)
        st[:, 1:-1] = r0[l], y0[l], u0[l], q0[l]
        for t in range(T):
            st[:, 0] = st[:, N]
            st[:, N + 1] = st[:, 1]
            o = O.macro_step(st, dt, dx, um)
            if o["rc"] != 0:
                assert not check, "the oracle's step fails its CFL check (lane %d, step %d, interface %d)" % (l, t, o["err_index"])
                if out["rc"] is None or t < out["rc"][0]:
                    out["rc"] = (t, l, int(o["err_index"]))
                break
            out["tape"][l][t] = o["dqs"]
            st[:, 1:-1] = o["nr"], o["ny"], o["nu"], o["nueq"]
            out["hist_r"][t, l], out["hist_y"][t, l], out["hist_u"][t, l] = o["nr"], o["ny"], o["nu"]
        fin[:, l] = st[:, 1:-1]
    out["rT"], out["yT"], out["uT"], out["qT"] = fin
    return out


def ring_bwd(O, f, g_rT=None, g_yT=None, g_uT=None, gh_r=None, gh_y=None, gh_u=None):
    """Cotangents of the final (r, y, u) [L][N] and of the state after every step [T][L][N] (None = none).  Returns g_r0, g_u0 [L][N]."""
    L, N = f["r0"].shape
    T, um = f["T"], f["um"]
    g_r0, g_y0 = np.zeros((L, N), F), np.zeros((L, N), F)
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
            gr, gy = ngr[1:-1].copy(), ngy[1:-1].copy()
            gr[N - 1] += ngr[0]; gy[N - 1] += ngy[0]
            gr[0] += ngr[N + 1]; gy[0] += ngy[N + 1]
        g_r0[l], g_y0[l] = gr, gy
    a, g_u0 = glue_y_bwd(f["r0"], f["u0"], um, g_y0)
    return dict(g_r0=(g_r0 + a).astype(F), g_u0=g_u0)


def jump_state(L, N, seed=0, at=None, width=None):
    """A uniform state plus a density jump that crosses the seam: cells [at, at + width) mod N are dense and slow.  Defaults put the jump
    over the last and the first cells; with fewer than four cells the one dense cell is cell 0, so that the seam itself is the jump
    (light on its left, dense on its right: with the dense cell on the left the seam interface is trivial in every step).  Lanes differ
    by a small random ripple, so that no two of them compute the same thing."""
    rng = np.random.default_rng(seed)
    width = max(N // 3, 1) if width is None else width
    if at is None:
        at = (N - (width + 1) // 2) % N if N >= 4 else 0
    r = np.full((L, N), 0.25, F) + rng.uniform(0, 0.02, (L, N)).astype(F)
    u = np.full((L, N), 12.0, F) + rng.uniform(0, 0.5, (L, N)).astype(F)
    cells = (at + np.arange(width)) % N
    r[:, cells] += F(0.45)
    u[:, cells] -= F(8.0)
    return r, u


# the shapes tests/test_macro_ring_gpu.py runs (tests/test_macro_ring.py asserts on the oracle that the seam interface is non-trivial in
# every one of them with two cells or more)
SIZES = (1, 2, 3, 63, 64, 65, 128, 129, 300)
ORACLE_CASES = [(3, 1, 7), (3, 2, 9), (3, 3, 11), (1, 63, 131), (3, 64, 70), (1, 65, 135), (1, 128, 140), (1, 129, 263), (1, 300, 7),
                (1, 300, 305)]                       # (L, N, T): T > N but for the short 300-cell case
FOLD_STEPS = 40                                      # the fold and tangent cases run min(N, FOLD_STEPS) steps on 3 lanes


def seam_is_live(f, lane):
    """Whether interface 0 (= N) of the chained oracle's run is non-trivial in at least one step: its B block, d2 of cell N - 1 up to
    the factor -dt / dx, is non-zero, so that the seam carries both Jacobians."""
    N = f["r0"].shape[1]
    return any(np.any(f["tape"][lane][t][N - 1, 2] != 0) for t in range(f["T"]))
