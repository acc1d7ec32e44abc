"""Exact-arithmetic restatement of the interface solver and the IDM step, to adjudicate the device math.

The reference's formulas -- ARZ.riemann_solve (model/macro/_arz.py:213-332) with its helpers (:122-199), the analytic Jacobians
(model/macro/darz.py:35-233), IDM.compute_acceleration (model/micro/_idm.py:6-50), the Euler step and the gap handling of
road/lane/_micro_lane.py:151-183 and dIDM (model/micro/didm.py:13-103, un-clamped deltas: road/lane/dmicro_lane.py:97) -- are
evaluated in Python's `decimal` at 70 digits on the exact values of the double inputs (Decimal(float) is exact).  Every
intermediate is an `X`: its exact value and a forward error bound B for a double evaluation of the same formula, grown by running
error analysis (cancellation is priced in: the rounding of a + b costs a unit times |a| + |b|, not times |a + b|):

  U  = 2^-52 per addition, subtraction or multiplication -- two double ulps: the rounding itself plus the reference's libm pow
       (within one ulp) where it takes a power, or a contraction the production form writes as an explicit fma;
  UQ = 2^-43 per division or square root -- the production form takes both from a v_rcp_f64 / v_rsq_f64 seed (relative error
       <= 2^-23) and one Newton / Goldschmidt step, which leaves 1.5 x 2^-46; 1 / x as the square of a refined 1 / sqrt(x) doubles
       that, and a division becomes a refined reciprocal and a product: 2^-43 covers it with room (src fast_math.hpp).

A double result d of any of the three evaluations (oracle, IEEE device variant, production variant) must lie within B of the exact
value.  A float32 result f is a valid rounding when round32(v - B) <= f <= round32(v + B): f is the rounding of some double that the
bound allows, so two evaluations may differ in a float32 entry only where the exact value is within B of the midpoint between the
two roundings.  A case decision is an exact comparison of a deciding quantity with its threshold: `margins` lists each with its
signed distance from the threshold and the bound of that distance; two evaluations may decide differently only where
|margin| <= bound.
"""
from decimal import Decimal, localcontext, Context, ROUND_HALF_EVEN

import numpy as np

CTX = Context(prec=70, rounding=ROUND_HALF_EVEN, Emin=-999999, Emax=999999)
U = Decimal(2) ** -52
UQ = Decimal(2) ** -43
ZERO = Decimal(0)
INF = Decimal("Infinity")
EPS = Decimal(1e-5)                 # EPSILON, model/macro/_arz.py:2 (the double nearest 1e-5)
GAP_EPS = Decimal(1e-5)             # POSITION_DELTA_EPS, road/lane/_micro_lane.py:166


def D(x):
    return Decimal(float(x))


class X:
    """Exact value `v` of a formula and the bound `e` of a double evaluation's distance from it."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=ZERO):
        self.v = v if isinstance(v, Decimal) else D(v)
        self.e = e

    def __add__(self, o):
        o = o if isinstance(o, X) else X(o)
        return _rounded(self.v + o.v, self, o, self.e + o.e + U * (abs(self.v) + abs(o.v) + self.e + o.e))

    def __sub__(self, o):
        o = o if isinstance(o, X) else X(o)
        return _rounded(self.v - o.v, self, o, self.e + o.e + U * (abs(self.v) + abs(o.v) + self.e + o.e))

    def __neg__(self):
        return X(-self.v, self.e)

    def __mul__(self, o):
        o = o if isinstance(o, X) else X(o)
        e = abs(self.v) * o.e + abs(o.v) * self.e + self.e * o.e
        return _rounded(self.v * o.v, self, o, e + U * (abs(self.v) + self.e) * (abs(o.v) + o.e))

    __radd__ = __add__
    __rmul__ = __mul__

    def __rsub__(self, o):
        return X(o) - self

    def __truediv__(self, o):
        o = o if isinstance(o, X) else X(o)
        den = abs(o.v) - o.e
        if den <= 0:
            return X(self.v / o.v if o.v != 0 else ZERO, INF)
        q = self.v / o.v
        e = (self.e + abs(q) * o.e) / den
        return X(q, e + UQ * (abs(q) + e))

    def __rtruediv__(self, o):
        return X(o) / self

    def sqrt(self):
        a = max(self.v, ZERO)
        s = a.sqrt()
        e = self.e.sqrt() if self.e != INF else INF
        if s > 0 and self.e != INF:
            e = min(e, self.e / s)
        return X(s, e + UQ * (s + e))

    def max(self, c):
        """max(self, c) for an exact c: 1-Lipschitz, the bound carries over."""
        c = c if isinstance(c, Decimal) else D(c)
        return X(c if c > self.v else self.v, self.e)


def _rounded(v, a, b, e):
    """An addition or multiplication of two exact operands whose result is a double is exact in every IEEE evaluation."""
    if a.e == 0 and b.e == 0 and D(float(v)) == v:
        return X(v, ZERO)
    return X(v, e)


def _ctx(f):
    def g(*a, **k):
        with localcontext(CTX):
            return f(*a, **k)
    g.__doc__ = f.__doc__
    g.__name__ = f.__name__
    return g


# ---- ARZ --------------------------------------------------------------------------------------------------------------
def _u_eq(r, um):               # compute_u_eq, _arz.py:134-139 (max(r, 0.), gamma = 0.5)
    return um * (1 - (r.max(ZERO) + X(EPS)).sqrt())


def _u_eq_prime(r, um):         # compute_u_eq_prime, _arz.py:147-150 (max(r, EPSILON))
    return (-um * X(Decimal("0.5"))) / r.max(EPS).sqrt()


@_ctx
def arz(L, R, um, dt=0.01, dx=5.0, case=None):
    """One interface: L, R = (r, y, u, u_eq) as doubles, um = u_max.  Returns a dict with
      case      the reference's case index (0 = Q_L, 1 = Q_M, 2 = Q_C), branch 1..6 of riemann_solve,
      margins   [(name, margin, bound)] of every comparison on the way (a case needs all of them settled),
      q0, flux, speed, dL, dR, fp   X values (dL, dR, fp as lists of 4, row-major),
      cfl       (margin, bound) of dt * max(|speed|, 1e-5) < dx for the worse speed (_macro_lane.py:141-146).
    `case` forces the outputs of another case (a tie): they are then what that case's formulas give."""
    rL, yL, uL, qL = (X(v) for v in L)
    rR, yR, uR, qR = (X(v) for v in R)
    um = X(um)
    m = []
    half = X(Decimal("0.5"))

    def lam0(r, u):             # FullQ.lambda_0, _arz.py:103-104
        return u + r * _u_eq_prime(r, um)

    def qm_r():                 # compute_Qm :185-199: r = (r_L ** gamma + (u_L - u_R) / u_max) ** (1 / gamma)
        b = rL.sqrt() + (uL - uR) / um
        return b * b

    m.append(("rL<eps", rL.v - EPS, ZERO))
    rm = None
    if rL.v < EPS:                                          # :225-230
        br, ci, s0, s1 = 1, 0, X(ZERO), uL
    else:
        m.append(("rR<eps", rR.v - EPS, ZERO))
        if rR.v < EPS:                                      # :233-249
            l0l = lam0(rL, uL)
            s0 = (l0l + (um + uL - qL)) * half
            br, s1 = 2, s0
            m.append(("l0l>=0", l0l.v, l0l.e))
            ci = 0 if l0l.v >= 0 else 2
        else:
            du = uL - uR
            m.append(("|dU|<eps", abs(du.v) - EPS, du.e))
            if abs(du.v) < EPS:                             # :252-257
                br, ci, s0, s1 = 3, 0, X(ZERO), uR
            else:
                m.append(("uL>uR", uL.v - uR.v, ZERO))
                if uL.v > uR.v:                             # :260-274
                    rm = qm_r()
                    diff = rm * uR - rL * uL
                    s0 = diff / (rm - rL).max(EPS)
                    br, s1 = 4, uR
                    m.append(("speed0>=0", diff.v, diff.e))
                    ci = 0 if diff.v >= 0 else 1
                else:
                    qmu = um + uL - qL
                    d5 = qmu - uR
                    m.append(("qm_u>uR", d5.v, qmu.e + U * (abs(qmu.v) + abs(uR.v))))
                    l0l = lam0(rL, uL)
                    m.append(("l0l>=0", l0l.v, l0l.e))
                    if d5.v > 0:                            # :277-296
                        rm = qm_r()
                        l0m = lam0(rm, uR)
                        s0 = (l0l + l0m) * half
                        br, s1 = 5, uR
                        if l0l.v >= 0:
                            ci = 0
                        else:
                            m.append(("l0m<=0", l0m.v, l0m.e))
                            ci = 1 if l0m.v <= 0 else 2
                    else:                                   # :299-314
                        s0 = (l0l + qmu) * half
                        br, s1 = 6, uR
                        ci = 0 if l0l.v >= 0 else 2
    out = dict(case=ci, branch=br, margins=m, speed=[s0, s1])
    # CFL assert, _macro_lane.py:141-146: dt < dx / max(|speed|, EPS) for both speeds
    cm = None
    for s in (s0, s1):
        a = X(abs(s.v), s.e).max(Decimal(1e-5))
        t = X(dx) - X(dt) * a
        c = (t.v, t.e + U * abs(D(dx)))
        cm = c if cm is None or c[0] < cm[0] else cm
    out["cfl"] = cm
    if case is not None:
        ci = int(case)
    out["out_case"] = ci
    # ---- Q_0 (:316-326) and its Jacobians (darz.py:194-215) ----
    rLc = rL.max(EPS)
    if ci == 0:                                             # compute_Ql :156-166 (set_r_y on floats)
        r0, y0 = rL, yL
        u0 = yL / rLc + _u_eq(rLc, um)
        q0 = _u_eq(rL, um)
        dL = [X(1), X(0), X(0), X(1)]
        dR = [X(0)] * 4
    else:
        ueqp_L = _u_eq_prime(rL, um)
        duL_drL = -yL / (rLc * rLc) + ueqp_L
        duL_dyL = 1 / rLc
        if ci == 1:                                         # compute_Qm :185-199, compute_dM darz.py:35-122
            r0 = rm if rm is not None else qm_r()
            u0 = uR
            q0 = _u_eq(r0, um)
            y0 = r0 * (u0 - q0)
            rRc = rR.max(EPS)
            ueqp_M = _u_eq_prime(r0, um)
            duR_drR = -yR / (rRc * rRc) + _u_eq_prime(rRc, um)
            duR_dyR = 1 / rRc
            a = X(2) * r0.sqrt()
            b = half / rLc.sqrt()
            inv_um = 1 / um
            drM_drL = a * (b + inv_um * duL_drL)
            drM_dyL = a * (inv_um * duL_dyL)
            e = u0 - q0
            dyM_drL = drM_drL * e + r0 * (-ueqp_M * drM_drL)
            dyM_dyL = drM_dyL * e + r0 * (-ueqp_M * drM_dyL)
            minv = -1 / um
            drM_drR = a * (minv * duR_drR)
            drM_dyR = a * (minv * duR_dyR)
            dyM_drR = drM_drR * e + r0 * (duR_drR - ueqp_M * drM_drR)
            dyM_dyR = drM_dyR * e + r0 * (duR_dyR - ueqp_M * drM_dyR)
            dL = [drM_drL, drM_dyL, dyM_drL, dyM_dyL]
            dR = [drM_drR, drM_dyR, dyM_drR, dyM_dyR]
        else:                                               # compute_Qc :168-183, compute_dC darz.py:124-192
            g3 = half / X(Decimal("1.5"))                   # gamma / (gamma + 1)
            base = uL + um * rL.sqrt()
            t = base / (X(Decimal("1.5")) * um)
            r0 = t * t
            u0 = g3 * base
            q0 = _u_eq(r0, um)
            y0 = r0 * (u0 - q0)
            ueqp_C = _u_eq_prime(r0, um)
            f = um * half / rLc.sqrt()
            duC_drL = g3 * (duL_drL + f)
            duC_dyL = g3 * duL_dyL
            e = (r0.sqrt() / half) / (X(Decimal("1.5")) * um)
            drC_drL = e * (duL_drL + f)
            drC_dyL = e * duL_dyL
            g = u0 - q0
            dyC_drL = drC_drL * g + r0 * (duC_drL - ueqp_C * drC_drL)
            dyC_dyL = drC_dyL * g + r0 * (duC_dyL - ueqp_C * drC_dyL)
            dL = [drC_drL, drC_dyL, dyC_drL, dyC_dyL]
            dR = [X(0)] * 4
    # ---- flux (_arz.py:94-101) and flux Jacobian at Q_0 (darz.py:217-233) ----
    r0c = r0.max(EPS)
    ueqp0 = _u_eq_prime(r0c, um)
    yor = y0 / r0c
    fp = [q0 + r0c * ueqp0, X(1), y0 * ueqp0 - yor * yor, (X(2) * y0) / r0c + q0]
    out.update(q0=[r0, y0, u0, q0], flux=[r0 * u0, y0 * u0], dL=dL, dR=dR, fp=fp)
    return out


# ---- IDM ----------------------------------------------------------------------------------------------------------------
@_ctx
def idm(a_max, a_pref, v, v_target, dp, dv, min_space, time_pref, dt, flags=None):
    """One vehicle step with the RAW gap dp and speed difference dv (dhts.ops.idm_batch's row).  Returns a dict with
      clipped_acc, clipped_spacing, collided, margins [(name, margin, bound)],
      acc, sstar, next_v (X; next_v before its float32 store), dEgo, dLeading (lists of 4 X, row-major),
      finite: False where the Jacobians divide by a zero gap (the reference's own values are then inf / nan).
    `flags` = (clipped_acc, clipped_spacing) forces the outputs of the other side of a tie."""
    a_max, a_pref, v, vt, s0, T, dt = (X(x) for x in (a_max, a_pref, v, v_target, min_space, time_pref, dt))
    dp_raw, dv_raw = X(dp), X(dv)
    collided = dp_raw.v < 0                                  # _micro_lane.py:151-162: deltas zeroed
    dpx, dvx = (X(0), X(0)) if collided else (dp_raw, dv_raw)
    dpc = dpx.max(GAP_EPS)                                   # :166
    m = []
    two_sab = X(2) * (a_max * a_pref).sqrt()                 # _idm.py:41-50
    s = s0 + v * T + (v * dvx) / two_sab
    m.append(("s*<0", s.v, s.e))
    cs = s.v < 0
    s = s.max(ZERO)
    vr = v / vt
    vr2 = vr * vr
    sr = s / dpc
    acc = a_max * (X(1) - vr2 * vr2 - sr * sr)
    floor = -v / dt
    m.append(("acc<-v/dt", acc.v - floor.v, acc.e + floor.e))
    ca = acc.v < floor.v
    if flags is not None:
        ca, cs = bool(flags[0]), bool(flags[1])
        if cs:
            s = X(ZERO)
            sr = X(ZERO)
            acc = a_max * (X(1) - vr2 * vr2)
    acc = floor if ca else acc
    next_v = v + dt * acc                                    # _micro_lane.py:182-183
    out = dict(clipped_acc=ca, clipped_spacing=cs, collided=collided, margins=m, acc=acc, sstar=s, next_v=next_v, finite=True)
    dE = [X(1), dt, X(0), X(0)]
    dLd = [X(0)] * 4
    if not ca:                                               # didm.py:38-103 with the un-clamped deltas
        if dp_raw.v == 0:
            out["finite"] = False
        else:
            dp2 = dp_raw * dp_raw
            s2_dp3 = (s * s) / (dp2 * dp_raw)
            s_dp2 = s / dp2
            free = X(-4) * ((v * v * v) / ((vt * vt) * (vt * vt)))
            dE[2] = dt * (X(-2) * a_max * s2_dp3)
            dLd[2] = dt * (X(2) * a_max * s2_dp3)
            if cs:
                dE[3] = X(1) + dt * a_max * free
                dLd[3] = dt * a_max * (X(-2) * s_dp2)
            else:
                dE[3] = X(1) + dt * a_max * (free - X(2) * s_dp2 * (T + (v + dv_raw) / two_sab))
                dLd[3] = dt * a_max * (X(-2) * s_dp2 * (-v / two_sab))
    out.update(dEgo=dE, dLeading=dLd)
    return out


# ---- adjudication -------------------------------------------------------------------------------------------------------
def f32_range(x):
    """[lo, hi]: the float32 values that are roundings of some double within x.e of x.v (widened by one double ulp on each side so
    that the double rounding Decimal -> double -> float32 cannot narrow it)."""
    if x.e == INF:
        return -np.inf, np.inf
    with localcontext(CTX):
        lo, hi = float(x.v - x.e), float(x.v + x.e)
    return np.float32(np.nextafter(lo, -np.inf)), np.float32(np.nextafter(hi, np.inf))


def f32_ok(f, x):
    lo, hi = f32_range(x)
    return bool(lo <= np.float32(f) <= hi)


def f64_ok(d, x):
    """A double result within the bound (in units of the bound: the returned ratio must be <= 1)."""
    if x.e == INF:
        return True, 0.0
    with localcontext(CTX):
        err = abs(D(d) - x.v)
        return err <= x.e, float(err / x.e) if x.e > 0 else (0.0 if err == 0 else float("inf"))


def tie(margins, name):
    """(margin, bound) of the decision `name`, None if the path did not take it."""
    for n, mg, b in margins:
        if n == name:
            return mg, b
    return None


def case_ties(margins):
    """Names of the decisions whose margin lies within its bound (where two evaluations may go different ways).  A comparison of
    exact operands (bound 0) is never one: at margin 0 it has one answer."""
    return [n for n, mg, b in margins if b > 0 and abs(mg) <= b]


# ---- tables over many rows -----------------------------------------------------------------------------------------------
def _vf(x):
    with localcontext(CTX):
        return float(x.v), (float(x.e) if x.e != INF else np.inf)


def _table(items, keys):
    """Columns of per-row results: for each X output `k`, k_v (nearest double) and k_e (bound); float32 outputs also k_lo, k_hi."""
    n = len(items)
    out = {}
    for k, width, is32 in keys:
        v = np.empty((n, width)); e = np.empty((n, width))
        lo = np.empty((n, width), np.float32); hi = np.empty((n, width), np.float32)
        for i, h in enumerate(items):
            xs = h[k] if width > 1 else [h[k]]
            for j, x in enumerate(xs):
                v[i, j], e[i, j] = _vf(x)
                if is32:
                    lo[i, j], hi[i, j] = f32_range(x)
        out[k + "_v"], out[k + "_e"] = v, e
        if is32:
            out[k + "_lo"], out[k + "_hi"] = lo, hi
    return out


ARZ_KEYS = (("q0", 4, False), ("flux", 2, False), ("speed", 2, False), ("dL", 4, True), ("dR", 4, True), ("fp", 4, True))
IDM_KEYS = (("acc", 1, False), ("sstar", 1, False), ("next_v", 1, True), ("dEgo", 4, True), ("dLeading", 4, True))


def arz_table(inp, dt=0.01, dx=5.0, cases=None):
    """arz() over the rows of inp [n][9]; `cases` [n] forces each row's output case.  Columns: case, tie (a case decision within
    its bound), cfl_m / cfl_e, and the output columns of _table."""
    items = [arz(r[:4], r[4:8], r[8], dt, dx, None if cases is None else int(cases[i])) for i, r in enumerate(inp)]
    t = _table(items, ARZ_KEYS)
    t["case"] = np.array([h["case"] for h in items])
    t["tie"] = np.array([bool(case_ties(h["margins"])) for h in items])
    t["cfl_m"] = np.array([float(h["cfl"][0]) for h in items])
    t["cfl_e"] = np.array([float(h["cfl"][1]) for h in items])
    return t


def idm_table(inp, flags=None):
    """idm() over the rows of inp [n][9]; `flags` [n][2] forces each row's clips.  Columns: clipped_acc, clipped_spacing, tie_acc,
    tie_spacing, finite, and the output columns of _table."""
    items = [idm(*r, flags=None if flags is None else flags[i]) for i, r in enumerate(inp)]
    t = _table(items, IDM_KEYS)
    for k in ("clipped_acc", "clipped_spacing", "finite", "collided"):
        t[k] = np.array([h[k] for h in items])
    t["tie_spacing"] = np.array(["s*<0" in case_ties(h["margins"]) for h in items])
    t["tie_acc"] = np.array(["acc<-v/dt" in case_ties(h["margins"]) for h in items])
    return t


def within64(d, t, k):
    """|d - exact| <= bound, per entry, and the error in units of the bound (one double ulp of slack for the exact value's own
    rounding to double)."""
    v, e = t[k + "_v"], t[k + "_e"]
    d = np.asarray(d, np.float64).reshape(v.shape)
    err = np.abs(d - v)
    same = (d == v) | (np.isnan(d) & np.isnan(v))
    ok = same | (err <= e + np.spacing(np.abs(v)))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(same, 0.0, err / e)
    return ok, ratio


def within32(f, t, k):
    """float32 entries that are roundings the bound allows."""
    lo, hi = t[k + "_lo"], t[k + "_hi"]
    f = np.asarray(f, np.float32).reshape(lo.shape)
    return (lo <= f) & (f <= hi)
