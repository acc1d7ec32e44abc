"""The chained oracle of the on-ramp rollouts (dhts_macro_rollout_*_ckpt_ramp): macro_sched_ref.sched_fwd / sched_bwd and
macro_ring_ref.ring_fwd / ring_bwd with one change each.  Forward: behind oracle.macro_step of step t the density of every ramp cell gets
one more float32 operation, nr[c] = float32(float64(nr[c]) + dt float64(inflow[t, l, j])), y stays, and (u, u_eq) of the cell are
oracle.arz_from_r_y of the new pair -- the state after step t, which the next step, the history and the final state all see.
Backward: in front of oracle.macro_step_bwd of step t and behind the per-step cotangents of that row, g_inflow[t, l, j] =
float32(dt float64(g_r[c])): the source is identity in (r, y).  A ramp index outside [0, N) names no cell: nothing is added and its
column of g_inflow stays 0.  The float32 glue is macro_sched_ref's and is not restated.  No GPU, no torch."""
import numpy as np

from macro_sched_ref import F, boundary_ry_to_ru, from_r_u, glue_u_bwd, glue_y_bwd


def ramp_fwd(O, r0, u0, T, dt, dx, um, ramps, inflow, gr=None, gu=None, check=True):
    """r0, u0 [L][N]; ramps [R] cell indices; inflow [T][L][R].  gr, gu: the boundary cells [L][2] or a schedule [T][L][2]; None: a ring.
    Returns dict as sched_fwd / ring_fwd: rT, yT, uT, qT [L][N], hist_r / _y / _u [T][L][N] (post-source), tape (per lane and step: dqs),
    and rc: None or (step, lane, interface) of the first failed CFL check (check=False)."""
    r0, u0 = (np.ascontiguousarray(a, F) for a in (r0, u0))
    L, N = r0.shape
    ramps = [int(c) for c in ramps]
    inflow = np.ascontiguousarray(inflow, F).reshape(T, L, len(ramps))
    ring = gr is None
    if not ring:
        gr, gu = (np.ascontiguousarray(a, F) for a in (gr, gu))
        if gr.ndim == 2:
            gr, gu = (np.broadcast_to(a, (T, L, 2)).copy() for a in (gr, gu))
        assert gr.shape == (T, L, 2) and gu.shape == (T, L, 2)
        gy, gq = from_r_u(gr, gu, um)
    y0, q0 = from_r_u(r0, u0, um)
    out = dict(T=T, um=um, dt=dt, r0=r0, u0=u0, gr=gr, gu=gu, ring=ring, ramps=ramps, inflow=inflow, rc=None,
               tape=[[None] * T for _ in range(L)],
               hist_r=np.zeros((T, L, N), F), hist_y=np.zeros((T, L, N), F), hist_u=np.zeros((T, L, N), F))
    fin = np.zeros((4, L, N), F)
    for l in range(L):
        st = np.zeros((4, N + 2), F)
        st[:, 1:-1] = r0[l], y0[l], u0[l], q0[l]
        for t in range(T):
            if ring:
                st[:, 0] = st[:, N]
                st[:, N + 1] = st[:, 1]
            else:
                st[:, 0] = gr[t, l, 0], gy[t, l, 0], gu[t, l, 0], gq[t, l, 0]
                st[:, N + 1] = gr[t, l, 1], gy[t, l, 1], gu[t, l, 1], gq[t, l, 1]
            o = O.macro_step(st, dt, dx, um)
            if o["rc"] != 0:
                assert not check, "the oracle's step fails its CFL check (lane %d, step %d, interface %d)" % (l, t, o["err_index"])
                if out["rc"] is None or t < out["rc"][0]:
                    out["rc"] = (t, l, int(o["err_index"]))
                break
            nr, ny, nu, nueq = o["nr"], o["ny"], o["nu"], o["nueq"]
            for j, c in enumerate(ramps):
                if 0 <= c < N:
                    nr[c] = F(np.float64(nr[c]) + dt * np.float64(inflow[t, l, j]))
                    nu[c], nueq[c] = O.arz_from_r_y(nr[c], ny[c], um)
            out["tape"][l][t] = o["dqs"]
            st[:, 1:-1] = nr, ny, nu, nueq
            out["hist_r"][t, l], out["hist_y"][t, l], out["hist_u"][t, l] = nr, ny, nu
        fin[:, l] = st[:, 1:-1]
    out["rT"], out["yT"], out["uT"], out["qT"] = fin
    return out


def ramp_bwd(O, f, g_rT=None, g_yT=None, g_uT=None, gh_r=None, gh_y=None, gh_u=None, start=None):
    """Cotangents of the final (r, y, u) [L][N] and of the state after every step [T][L][N] (None = none).  Returns g_r0, g_u0 [L][N],
    g_inflow [T][L][R] float32 and, with boundary cells, g_ghost_ry [T][L][2][2] float64 and g_ghost_r, g_ghost_u [T][L][2] float32
    (per step; a constant boundary's gradient is their sum over the steps, formed in double from g_ghost_ry by the caller).
    start: sweep the steps T - 1 .. start only and return the running (g_r, g_y) [L][N] in front of step `start` as cut_r, cut_y."""
    L, N = f["r0"].shape
    T, um, dt, ramps, ring = f["T"], f["um"], f["dt"], f["ramps"], f["ring"]
    g_r0, g_y0 = np.zeros((L, N), F), np.zeros((L, N), F)
    g_ry = np.zeros((T, L, 2, 2), np.float64)
    g_in = np.zeros((T, L, len(ramps)), F)
    first = 0 if start is None else start
    for l in range(L):
        gr = np.zeros(N, F) if g_rT is None else np.array(g_rT[l], F)
        gy = np.zeros(N, F) if g_yT is None else np.array(g_yT[l], F)
        if g_uT is not None:
            a, b = glue_u_bwd(f["rT"][l], f["yT"][l], um, g_uT[l])
            gr, gy = gr + a, gy + b
        for t in range(T - 1, first - 1, -1):
            if gh_r is not None:
                gr = gr + np.asarray(gh_r[t, l], F)
            if gh_y is not None:
                gy = gy + np.asarray(gh_y[t, l], F)
            if gh_u is not None:
                a, b = glue_u_bwd(f["hist_r"][t, l], f["hist_y"][t, l], um, gh_u[t, l])
                gr, gy = gr + a, gy + b
            for j, c in enumerate(ramps):
                if 0 <= c < N:
                    g_in[t, l, j] = F(dt * np.float64(gr[c]))
            ngr, ngy = O.macro_step_bwd(f["tape"][l][t], gr.astype(F), gy.astype(F))
            gr, gy = ngr[1:-1].copy(), ngy[1:-1].copy()
            if ring:
                gr[N - 1] += ngr[0]; gy[N - 1] += ngy[0]
                gr[0] += ngr[N + 1]; gy[0] += ngy[N + 1]
            else:
                g_ry[t, l, 0] = ngr[0], ngy[0]
                g_ry[t, l, 1] = ngr[N + 1], ngy[N + 1]
        g_r0[l], g_y0[l] = gr, gy
    if start is not None:
        return dict(cut_r=g_r0, cut_y=g_y0, g_inflow=g_in)
    a, g_u0 = glue_y_bwd(f["r0"], f["u0"], um, g_y0)
    out = dict(g_r0=(g_r0 + a).astype(F), g_u0=g_u0, g_inflow=g_in)
    if not ring:
        out["g_ghost_ry"] = g_ry
        out["g_ghost_r"], out["g_ghost_u"] = boundary_ry_to_ru(g_ry, f["gr"], f["gu"], um)
    return out


def ramp_state(L, N, seed=0):
    """A lane with a dense, slow block in its middle third (a downstream bottleneck for the cells in front of it) and a small random
    ripple per lane, so that interfaces beside a ramp anywhere on the lane are non-trivial within a few steps and no two lanes agree."""
    rng = np.random.default_rng(seed)
    r = np.full((L, N), 0.30, F) + rng.uniform(0, 0.04, (L, N)).astype(F)
    u = np.full((L, N), 11.0, F) + rng.uniform(0, 1.0, (L, N)).astype(F)
    lo, hi = N // 3, max(2 * N // 3, N // 3 + 1)
    r[:, lo:hi] += F(0.35)
    u[:, lo:hi] -= F(7.0)
    return r, u


def ramp_inflow(T, L, R, dt, seed=0):
    """Per-lane random rates whose sum over the T steps adds at most 0.2 to a cell (|dt sum_t inflow| <= dt sum_t |inflow| <= 0.2), about
    a fifth of them negative (an off-ramp)."""
    rng = np.random.default_rng(1000 + seed)
    a = rng.uniform(0.2, 1.0, (T, L, R))
    a[rng.uniform(size=a.shape) < 0.2] *= -1.0
    return (a * (0.2 / (dt * max(T, 1)))).astype(F)


# ---- the cases tests/test_macro_ramp_gpu.py runs; tests/test_macro_ramp.py holds every one of them to the input conditions on the oracle ----
DT, DX, UM = 0.01, 5.0, 30.0
LANES = 3
BOUNDS = ("const", "sched", "ring")
LOSSES = ("final", "detectors", "target")
# (N, ramps): both ends, both ends together, the two cells either side of the first 64-cell pass, every cell of a three-cell lane, an
# interior pair; N = 2 .. 64 run one pass per wavefront, 65 .. 300 two (macro_ckpt_plan's "passes")
RAMP_SETS = [(2, (0,)), (2, (1,)), (2, (0, 1)), (3, (0, 1, 2)), (64, (0, 63)), (64, (20, 41)), (65, (0,)), (65, (64,)), (65, (63, 64)),
             (129, (0, 128)), (129, (63, 64)), (129, (40, 100)), (300, (0, 299)), (300, (63, 64)), (300, (150, 151))]
STEPS = ((1, 0), (11, 4))            # (T, segment): one step; three segments, the last one short, at a segment of four
RING_LONG = (64, (0, 63), 2 * 64 + 5)      # the 64-cell ring at the plan's own segment: more than twice round
RING_EXTRA = [(2, (0, 1), 11), (65, (0, 64), 11)]      # further rings of the mass and translation tests


LEVELS = ((0.25, 13.0), (0.45, 4.0), (0.62, 1.5), (0.74, 0.4))      # (r, u): each step up is a shock the Riemann solver has to solve


def case_state(N, ramps, seed=0):
    """A uniform light lane with a ripple per lane and cell, and a staircase at every run of adjacent ramp cells: the cell in front of
    the run stays on the base level and the run climbs LEVELS from there, so that the interface on the left of every ramp cell is a
    shock whose flux depends on both sides from the first step on (a weaker jump is upwind: "trivial").  A run that starts at cell 0
    begins on the base level itself and the cell behind it climbs once more: cell 0 of an open lane has a boundary cell on its left,
    whose interface leaves no block of its own in dqs, so it is the interface on its right that is held live.  The boundary cells are
    light and fast."""
    rng = np.random.default_rng(seed + 7 * N)
    level = np.zeros(N, int)
    c = 0
    while c < N:
        if c in ramps:
            at_zero = c == 0
            k = 0 if at_zero else 1
            while c < N and c in ramps:
                level[c] = k
                k, c = k + 1, c + 1
            if at_zero and c < N:                        # the run started at cell 0: the cell behind it
                level[c] = k
                c += 1
        else:
            c += 1
    r = np.array([LEVELS[k][0] for k in level], F)[None, :] + rng.uniform(0, 0.03, (LANES, N)).astype(F)
    u = np.array([LEVELS[k][1] for k in level], F)[None, :] + rng.uniform(0, 0.3, (LANES, N)).astype(F)
    return r, u


def case_bounds(bound, T, seed=0):
    """(gr, gu): None for a ring, [L][2] constant or [T][L][2] scheduled boundary cells, light and fast."""
    if bound == "ring":
        return None, None
    rng = np.random.default_rng(seed + 31 * T)
    shape = (LANES, 2) if bound == "const" else (T, LANES, 2)
    return rng.uniform(0.10, 0.16, shape).astype(F), rng.uniform(14.0, 16.0, shape).astype(F)


def case_detectors(N, ramps):
    return sorted(set(ramps) | {0, N // 2, N - 1})


def case_target(N, ramps, T, seed=0):
    """[T][L][2][N]: a fifth of the entries not observed, the ramp cells' last row always."""
    rng = np.random.default_rng(seed + 13 * N + T)
    tg = np.stack([rng.uniform(0.1, 0.9, (T, LANES, N)), rng.uniform(0.0, UM, (T, LANES, N))], axis=2).astype(F)
    keep = tg[T - 1][:, :, list(ramps)].copy() if T else None
    tg[rng.uniform(size=tg.shape) < 0.2] = np.nan
    if T:
        tg[T - 1][:, :, list(ramps)] = keep
    return tg


def case_cotangents(f, loss, N, ramps, target=None):
    """The keyword arguments of ramp_bwd for the three losses: sum of the squared final (r, u); the sum of all readings (r, y, u) at
    case_detectors; sse.sum() against `target` (the float32 residuals the kernels form, twice, NaN = 0)."""
    if loss == "final":
        return dict(g_rT=2 * f["rT"], g_uT=2 * f["uT"])
    if loss == "detectors":
        gh = np.zeros((f["T"],) + f["r0"].shape, F)
        gh[:, :, case_detectors(N, ramps)] = 1
        return dict(gh_r=gh, gh_y=gh, gh_u=gh)
    e_r = np.where(np.isnan(target[:, :, 0]), F(0), F(2) * (f["hist_r"] - target[:, :, 0])).astype(F)
    e_u = np.where(np.isnan(target[:, :, 1]), F(0), F(2) * (f["hist_u"] - target[:, :, 1])).astype(F)
    return dict(gh_r=e_r, gh_u=e_u)


def case_sse(f, target):
    """[L][2] float64: the sums of the squared float32 residuals."""
    e_r = np.where(np.isnan(target[:, :, 0]), F(0), f["hist_r"] - target[:, :, 0]).astype(F).astype(np.float64)
    e_u = np.where(np.isnan(target[:, :, 1]), F(0), f["hist_u"] - target[:, :, 1]).astype(F).astype(np.float64)
    return np.stack([(e_r ** 2).sum(axis=(0, 2)), (e_u ** 2).sum(axis=(0, 2))], axis=1)


_CACHE = {}


def case_oracle(O, bound, N, ramps, T, loss=None):
    """The chained oracle's forward run of a case and, with `loss`, its backward run -- computed once per session and shared."""
    key = (bound, N, tuple(ramps), T)
    if key not in _CACHE:
        r, u = case_state(N, ramps)
        gr, gu = case_bounds(bound, T)
        inflow = ramp_inflow(T, LANES, len(ramps), DT, seed=N + T)
        _CACHE[key] = dict(r=r, u=u, gr=gr, gu=gu, inflow=inflow, f=ramp_fwd(O, r, u, T, DT, DX, UM, ramps, inflow, gr, gu),
                           tg=case_target(N, ramps, T))
    c = _CACHE[key]
    if loss is not None and loss not in c:
        c[loss] = ramp_bwd(O, c["f"], **case_cotangents(c["f"], loss, N, ramps, c["tg"]))
    return c


def all_cases():
    for N, ramps in RAMP_SETS:
        for T, _ in STEPS:
            for bound in BOUNDS:
                yield bound, N, ramps, T
    yield "ring", RING_LONG[0], RING_LONG[1], RING_LONG[2]
    yield "ring", 1, (0,), 11
    for N, ramps, T in RING_EXTRA:
        yield "ring", N, ramps, T


def interface_live(f, lane, cell):
    """Whether the interface on the left or on the right of `cell` is non-trivial in at least one step, read as
    macro_ring_ref.seam_is_live reads dqs: block 2 of the cell on the interface's left is non-zero (on a ring the left of cell 0 is cell
    N - 1; on an open lane interface 0 has a boundary cell on its left and no block of its own)."""
    N = f["r0"].shape[1]
    left = (cell - 1) % N if f["ring"] else cell - 1
    cells = [cell] + ([left] if left >= 0 else [])
    return any(np.any(f["tape"][lane][t][k, 2] != 0) for t in range(f["T"]) for k in cells)
