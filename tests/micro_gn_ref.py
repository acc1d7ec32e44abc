"""Reference for the Gauss-Newton normal equations the fused IDM rollout forms in its kernel (dhts_micro_rollout_fwd_jvp_gn), shared by
tests/test_micro_gn.py and tests/test_micro_gn_gpu.py.

normal_equations: ONE lane in numpy.  It takes the float32 states x and tangents t the kernel holds after each sampled step -- the rows
of micro_jvp_ref.chain's t_hist, or of the device's samples / t_samples -- forms the residual r = x - target in float32 as the kernel
does, the masked products in float64 (a product of two float32 numbers is exact there) and sums them with math.fsum, which rounds the
exact sum once.  So the reference has no summation error of its own, and a device sum of the same n exact terms in any order lies
within (n - 1) 2^-53 sum|terms| (1 + O(n 2^-53)) of it; the tests assert n 2^-52 sum|terms|, twice that.

expected: the same for every lane of a call from the arrays of the sampled form, with numpy's float64 sums (for shapes where a Python
loop over the terms would be slow); its own error shares the bound above, which is why the bound carries the factor two."""
import math

import numpy as np

F, D = np.float32, np.float64


def normal_equations(x, t, target, live):
    """x, target [R][2][P] float32, t [K][R][2][P] float32, live [P] bool (columns whose slot is below count).  An entry counts when
    its column is live and its target is not NaN.  Returns (sse [2], jtr [K], jtj [K][K]) float64 and (n, abs_jtr [K], abs_jtj [K][K]):
    the number of terms of the lane (both planes) and the sums of their magnitudes, for the bound."""
    x, target, t = np.asarray(x, F), np.asarray(target, F), np.asarray(t, F)
    K = t.shape[0]
    with np.errstate(invalid="ignore"):
        r = (x - target).astype(F)
    seen = ~np.isnan(target) & np.asarray(live, bool)[None, None, :]
    rd = r.astype(D)[seen]
    sse = np.array([math.fsum((r.astype(D)[:, c][seen[:, c]]) ** 2) for c in range(2)], D)
    td = [t[a].astype(D)[seen] for a in range(K)]
    jtr = np.array([math.fsum(td[a] * rd) for a in range(K)], D)
    jtj = np.array([[math.fsum(td[a] * td[b]) for b in range(K)] for a in range(K)], D).reshape(K, K)
    abs_jtr = np.array([math.fsum(np.abs(td[a] * rd)) for a in range(K)], D)
    abs_jtj = np.array([[math.fsum(np.abs(td[a] * td[b])) for b in range(K)] for a in range(K)], D).reshape(K, K)
    return (sse, jtr, jtj), (int(seen.sum()), abs_jtr, abs_jtj)


def expected(samples, t_samples, target, live_cols):
    """samples, target [R][L][2][P] float32, t_samples [K][R][L][2][P] float32, live_cols [L][P] bool.  Returns a dict of float64
    arrays: sse [L][2], jtr [L][K], jtj [L][K][K], their magnitude sums abs_sse, abs_jtr, abs_jtj and n [L], the terms per lane."""
    x, target, t = np.asarray(samples, F), np.asarray(target, F), np.asarray(t_samples, F)
    with np.errstate(invalid="ignore"):
        r = (x - target).astype(F).astype(D)
    seen = ~np.isnan(target) & np.asarray(live_cols, bool)[None, :, None, :]
    r = np.where(seen, r, 0.0)
    td = np.where(seen[None], t.astype(D), 0.0)
    sse = np.einsum("rlcp,rlcp->lc", r, r)
    jtr = np.einsum("arlcp,rlcp->la", td, r)
    jtj = np.einsum("arlcp,brlcp->lab", td, td)
    return dict(sse=sse, jtr=jtr, jtj=jtj, abs_sse=sse, abs_jtr=np.einsum("arlcp,rlcp->la", np.abs(td), np.abs(r)),
                abs_jtj=np.einsum("arlcp,brlcp->lab", np.abs(td), np.abs(td)), n=seen.sum(axis=(0, 2, 3)))


def within_bound(got, want, abs_sum, n):
    """|got - want| against n 2^-52 sum|terms| per entry -> (ok, the largest ratio |got - want| / (2^-52 sum|terms|) per term seen, i.e.
    in units of the bound's n).  An entry without a term must be exactly 0."""
    got, want, abs_sum = np.asarray(got, D), np.asarray(want, D), np.asarray(abs_sum, D)
    n = np.asarray(n, D).reshape((-1,) + (1,) * (got.ndim - 1))
    err = np.abs(got - want)
    bound = n * 2.0 ** -52 * abs_sum
    ok = bool(np.all(err <= bound))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(abs_sum > 0, err / (2.0 ** -52 * abs_sum * np.maximum(n, 1)), 0.0)
    return ok, float(ratio.max()) if ratio.size else 0.0
