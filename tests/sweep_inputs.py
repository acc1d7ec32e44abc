"""Seeded inputs for the device-math sweeps (tests/test_device_math_sweep_gpu.py, tests/test_hp_ref.py).

Rows follow dhts.ops.arz_interface_batch / idm_batch ([n][9] float64).  Values the kernels keep in float32 (cell r y u u_eq, vehicle
speed, gap) are float32 values; values the reference keeps as Python floats (u_max, vehicle parameters, dt, a source lane's ghost
cell, the speed difference v - v_lead of two float32 speeds) are doubles.  Each family is a list of edge classes
(name, rows, dt, dx): typical states and the places where a kernel's case logic or its rounding can go wrong.
"""
from decimal import Decimal, localcontext

import numpy as np

F32 = np.float32
EPS32 = F32(1e-5)                       # float32(1e-5) < 1e-5 < its successor


def f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def nudge32(x, k):
    """x moved by k float32 ulps (k an int array)."""
    x = np.asarray(x, np.float32).copy()
    k = np.asarray(k)
    for s in range(int(np.abs(k).max()) if k.size else 0):
        m = np.abs(k) > s
        x[m] = np.nextafter(x[m], np.where(k[m] > 0, np.inf, -np.inf).astype(np.float32))
    return x.astype(np.float64)


def nudge64(x, k):
    x = np.asarray(x, np.float64).copy()
    k = np.asarray(k)
    for s in range(int(np.abs(k).max()) if k.size else 0):
        m = np.abs(k) > s
        x[m] = np.nextafter(x[m], np.where(k[m] > 0, np.inf, -np.inf))
    return x


# ---- ARZ ------------------------------------------------------------------------------------------------------------------
def u_eq32(r, um):
    """u_eq of a float32 density as the float32 state stores it (one double evaluation, rounded)."""
    return f32(um * (1.0 - np.sqrt(np.maximum(r, 0.0) + 1e-5)))


def cell(r, u, um):
    r, u = f32(r), f32(u)
    q = u_eq32(r, um)
    return r, f32(r * (u - q)), u, q


def rows(L, R, um):
    n = len(L[0])
    return np.stack(list(L) + list(R) + [np.broadcast_to(np.float64(um), (n,))], 1).astype(np.float64)


def arz_classes(n, seed=0):
    """[(name, inp [n][9], dt, dx)]: about n rows per class."""
    rng = np.random.default_rng(seed)
    U = rng.uniform
    out = []

    def std(um, r_lo=0.0, r_hi=1.0):
        return cell(U(r_lo, r_hi, n), U(0, um, n), um), cell(U(r_lo, r_hi, n), U(0, um, n), um)

    for um in (30.0, 15.0):
        L, R = std(um)
        out.append(("typical_um%d" % um, rows(L, R, um), 0.01, 5.0))
    um = 30.0
    # vacuum: r = 0 on one side or both
    L, R = std(um)
    side = rng.integers(0, 3, n)
    rl = np.where(side != 1, 0.0, L[0]); rr = np.where(side != 0, 0.0, R[0])
    out.append(("r0", rows(cell(rl, L[2], um), cell(rr, R[2], um), um), 0.01, 5.0))
    # the float32 neighbours of 1e-5 on either side
    k = rng.integers(-3, 4, n)
    re = nudge32(np.full(n, EPS32), k)
    L, R = std(um)
    sw = rng.integers(0, 2, n).astype(bool)
    out.append(("r_eps", rows(cell(np.where(sw, re, L[0]), L[2], um), cell(np.where(sw, R[0], re), R[2], um), um), 0.01, 5.0))
    # jams
    L, R = std(um, 0.97, 1.0)
    out.append(("jam", rows(L, R, um), 0.01, 5.0))
    # |uL - uR| one float32 ulp either side of 1e-5
    L, R = std(um, 0.02, 1.0)
    uL = f32(U(1, um - 1, n))
    sgn = rng.choice([-1.0, 1.0], n)
    uR = nudge32(f32(uL - sgn * 1e-5), rng.integers(-2, 3, n))
    out.append(("dU_eps", rows(cell(L[0], uL, um), cell(R[0], uR, um), um), 0.01, 5.0))
    # r_m - r_L near 0: the max(r_m - r_L, EPSILON) clamp of the shock speed (u_L > u_R by a hair, small r_L)
    rl = f32(10 ** U(-5, -1, n))
    uL = f32(U(1, um - 1, n))
    dU = um * 1e-5 / (2 * np.sqrt(rl)) * 10 ** U(-1, 1, n)
    uR = f32(uL - np.maximum(dU, 2e-5))
    out.append(("rm_rl", rows(cell(rl, uL, um), cell(U(0.02, 1, n), uR, um), um), 0.01, 5.0))
    # u_max + u_L - u_eq,L close to u_R (branch 5 against 6), u_L < u_R
    L = cell(U(0.02, 1, n), U(0, 10, n), um)
    uR = nudge32(f32(um + L[2] - L[3]), rng.integers(-3, 4, n))
    out.append(("qmu_uR", rows(L, cell(U(0.02, 1, n), uR, um), um), 0.01, 5.0))
    # lambda_0(Q_L) = u_L - u_max sqrt(r_L) / 2 close to 0 (case 0 against the rarefaction cases)
    rl = f32(U(1e-4, 1, n))
    uL = nudge32(f32(0.5 * um * np.sqrt(rl)), rng.integers(-3, 4, n))
    out.append(("l0l_0", rows(cell(rl, uL, um), cell(U(0.0, 1, n), U(0, um, n), um), um), 0.01, 5.0))
    # stale u_eq (a deposited cell keeps the u_eq of its density before the deposit)
    L, R = std(um)
    L = (L[0], L[1], L[2], f32(U(0, um, n)))
    R = (R[0], R[1], R[2], f32(U(0, um, n)))
    out.append(("stale_ueq", rows(L, R, um), 0.01, 5.0))
    # wave speeds close to dx / dt = 20 (u of a cell is a speed the solver reports)
    L, R = std(um)
    uR = nudge32(np.full(n, F32(20.0)), rng.integers(-3, 4, n)) * rng.choice([-1.0, 1.0], n)
    out.append(("cfl", rows(L, cell(R[0], uR, um), um), 0.05, 1.0))
    # the threshold itself: r = 1e-5 exactly, which only a double input can hold (a float32 density never equals it), beside any state
    L, R = std(um)
    side = rng.integers(0, 2, n).astype(bool)
    out.append(("r_eps_f64", rows((np.where(side, 1e-5, L[0]),) + L[1:], (np.where(side, R[0], 1e-5),) + R[1:], um), 0.01, 5.0))
    # an itscp source lane's upstream ghost: doubles with all their bits, u = u_eq = u_eq(r) in double, y = 0; r = 1e-5 exactly
    # and its double neighbours among them
    rs = U(0.0, 0.6, n)
    pick = rng.integers(0, 4, n)
    rs = np.where(pick == 0, nudge64(np.full(n, 1e-5), rng.integers(-2, 3, n)), rs)
    us = um * (1.0 - np.sqrt(rs + 1e-5))
    R = cell(U(0, 1, n), U(0, um, n), um)
    Rk = list(R)
    # and u_R with |u_L - u_R| = 1e-5 exactly in double where it can be had
    sel = pick == 1
    Rk[2] = np.where(sel, f32(us - 1e-5), R[2])
    out.append(("src_ghost", rows((rs, np.zeros(n), us, us), tuple(Rk), um), 0.01, 5.0))
    return out


# ---- IDM ------------------------------------------------------------------------------------------------------------------
DEFAULT = (30.0, 24.0, 27.0, 0.5, 0.1)          # MicroVehicle.default_micro_vehicle(30): a_max, a_pref, v_target, min_space, T
FAST = (60.0, 48.0, 54.0, 0.5, 0.1)             # the same at a speed limit of 60
DTS = np.array([1.0 / 30.0, 0.01, 0.05, 0.1])


def rv_params(rng, n, sl=30.0):
    """MicroVehicle.random_micro_vehicle(sl) ranges (the *_rv fixtures): a_max, a_pref, v_target, min_space, T."""
    U = rng.uniform
    return np.stack([U(1.5, 2.0, n) * sl, U(1.0, 1.5, n) * sl, U(0.8, 1.2, n) * sl, U(1.0, 2.0, n), U(0.2, 0.6, n)], 1)


def idm_rows(P, v, gap, dv, dt):
    n = len(v)
    P = np.broadcast_to(np.asarray(P, np.float64), (n, 5))
    return np.stack([P[:, 0], P[:, 1], v, P[:, 2], gap, dv, P[:, 3], P[:, 4], dt], 1).astype(np.float64)


def sstar_root_dv(P, v):
    """dv with s* = min_space + v T + v dv / (2 sqrt(a_max a_pref)) = 0, exactly (decimal), rounded to the nearest double."""
    out = np.empty(len(v))
    with localcontext() as c:
        c.prec = 60
        for i in range(len(v)):
            a, b, _, s0, T = (Decimal(float(x)) for x in P[i])
            vv = Decimal(float(v[i]))
            out[i] = float(-(s0 + vv * T) * 2 * (a * b).sqrt() / vv)
    return out


def idm_classes(n, seed=0):
    """[(name, inp [n][9])]."""
    rng = np.random.default_rng(seed)
    U = rng.uniform
    out = []

    def base(P):
        v = f32(U(0, 35, n))
        vl = f32(U(0, 35, n))
        return P, v, f32(U(0.1, 200, n)), v - vl, DTS[rng.integers(0, 4, n)]

    out.append(("default", idm_rows(*base(DEFAULT))))
    out.append(("fast", idm_rows(*base(FAST))))
    out.append(("rv", idm_rows(*base(rv_params(rng, n)))))
    P, v, g, dv, dt = base(DEFAULT)
    out.append(("gap_neg", idm_rows(P, v, f32(-U(0, 5, n)), dv, dt)))
    out.append(("gap_zero", idm_rows(P, v, np.zeros(n), dv, dt)))
    out.append(("gap_eps", idm_rows(P, v, nudge32(np.full(n, EPS32), rng.integers(-3, 4, n)), dv, dt)))
    out.append(("gap_1000", idm_rows(P, v, np.full(n, 1000.0), np.where(rng.integers(0, 2, n) == 0, 0.0, dv), dt)))
    out.append(("v0", idm_rows(P, np.zeros(n), g, dv, dt)))
    Pr = rv_params(rng, n)
    vt = nudge32(f32(Pr[:, 2]), rng.integers(-3, 4, n))
    out.append(("v_target", idm_rows(Pr, vt, g, dv, dt)))
    # s* within a few double ulps of 0: the speed difference that zeroes it, and its neighbours
    P = rv_params(rng, n)
    P[: n // 2] = DEFAULT
    v = f32(U(0.5, 35, n))
    dvs = nudge64(sstar_root_dv(P, v), rng.integers(-3, 4, n))
    out.append(("sstar_0", idm_rows(P, v, f32(U(0.5, 100, n)), dvs, dt)))
    # acc within a few ulps of -v / dt: the gap at which a_max (1 - (v / v_t)^4 - (s* / gap)^2) = -v / dt, and its neighbours
    P, v, _, dv, dt = base(DEFAULT)
    v = f32(U(1, 30, n))
    dv = f32(U(0, 10, n))
    a, b, vt_, s0, T = (np.asarray(DEFAULT)[i] for i in range(5))
    s = s0 + v * T + v * dv / (2 * np.sqrt(a * b))
    gap = s / np.sqrt(1 - (v / vt_) ** 4 + v / (dt * a))
    half = n // 2
    g_clip = np.concatenate([nudge64(gap[:half], rng.integers(-3, 4, half)), nudge32(f32(gap[half:]), rng.integers(-2, 3, n - half))])
    out.append(("acc_floor", idm_rows(P, v, g_clip, dv, dt)))
    return out
