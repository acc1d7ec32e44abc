#!/usr/bin/env python3
"""A wave on a ring road: which initial density perturbation produced these observations?

The truth is a closed ARZ lane (dhts.macro_rollout(ring=True)) in a uniform state plus a localised density bump, run for more than two
laps of the wave (T > 2 N): the wave passes the seam between the last and the first cell at least twice, and what is observed late
depends on the initial state through that seam.  The observations are the densities at a few detectors after every step (default), or
the whole density and speed field (--fused-loss: target=, the squared error is formed inside the kernels and no history exists).
The unknown is the initial density r0 of every cell, fitted by Adam through the checkpointed reverse sweep
(checkpoint=True, ring=True) -- or, with --method lm, the bump's three parameters (height, centre, width), fitted by
Levenberg-Marquardt through dhts.macro_rollout_jvp(ring=True, fused=True): the readings and their Jacobian in one kernel, no tape.

Prints one line "iter <k> <loss>" per iteration and, at the end, the lane's mass sum_k r[k] before and after the truth's rollout: a
ring conserves it up to the float32 store of each cell.  Every simulated step runs in the HIP kernels.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diff-hybrid-traffic-sim_amd"))

import torch as th  # noqa: E402

import dhts  # noqa: E402


def bump(theta, N, dev):
    """Density of a uniform state plus a periodic Gaussian bump, theta = (height, centre, width) in (density, cells, cells)."""
    k = th.arange(N, device=dev, dtype=th.float32)
    d = (k - theta[1] + N / 2) % N - N / 2               # signed distance round the ring
    return (0.25 + theta[0] * th.exp(-0.5 * (d / theta[2]) ** 2))[None, :]


def main():
    ap = argparse.ArgumentParser("The initial density bump of a ring road from what detectors saw (MI355X)")
    ap.add_argument("--cells", type=int, default=64)
    ap.add_argument("--steps", type=int, default=0, help="0: 2 N + 16, a little more than two laps of the information")
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--detectors", type=int, default=4)
    ap.add_argument("--fused-loss", action="store_true", help="observe the whole field: target=, the loss is formed in the kernels")
    ap.add_argument("--method", choices=("adam", "lm"), default="adam")
    ap.add_argument("--lr", type=float, default=2e-2)
    args = ap.parse_args()
    dev = th.device("cuda", 0)
    N = args.cells
    T = args.steps or 2 * N + 16
    dt, dx, um = 0.05, 5.0, 30.0
    u0 = th.full((1, N), 12.0, device=dev)
    truth = th.tensor([0.3, 0.8 * N, max(N / 12.0, 1.0)], device=dev)
    det = sorted(set(int(round(i * N / args.detectors)) % N for i in range(args.detectors)))

    def roll(r0, **kw):
        return dhts.macro_rollout(r0, u0, None, None, T, dt, dx, um, ring=True, checkpoint=True, **kw)
    r_true = bump(truth, N, dev)
    with th.no_grad():
        rT, _, _, _, seen = roll(r_true, detectors=list(range(N)))
    field = th.stack([seen[:, :, 0], seen[:, :, 2]], dim=2).contiguous()          # [T][1][2][N]: density and speed after every step
    obs = seen[:, :, 0][:, :, det].contiguous()

    if args.method == "lm":
        theta, lam = th.tensor([0.15, 0.7 * N, max(N / 8.0, 1.5)], device=dev), 1e-2

        def residual_and_jacobian(theta):
            # the bump's own Jacobian [N][3], formed in torch: three tangent directions of r0
            d_r0 = th.autograd.functional.jacobian(lambda p: bump(p, N, dev)[0], theta)
            prim, tan = dhts.macro_rollout_jvp(bump(theta, N, dev), u0, None, None, T, dt, dx, um, ring=True, fused=True,
                                               t_r0=d_r0.t().reshape(3, 1, N).contiguous(), detectors=det)
            return (prim[4][:, :, 0] - obs).reshape(-1), tan[3][:, :, :, 0].reshape(3, -1).t()
        res, J = residual_and_jacobian(theta)
        for it in range(args.iters):
            print("iter %d %.6e" % (it, float((res ** 2).sum())))
            step = th.linalg.solve(J.t() @ J + lam * th.diag((J.t() @ J).diagonal() + 1e-12), -(J.t() @ res))
            trial = theta + step
            trial[2] = trial[2].clamp_min(0.5)
            res_t, J_t = residual_and_jacobian(trial)
            if float((res_t ** 2).sum()) < float((res ** 2).sum()):
                theta, res, J, lam = trial, res_t, J_t, lam * 0.3
            else:
                lam *= 5.0
        print("iter %d %.6e" % (args.iters, float((res ** 2).sum())))
        print("theta %s truth %s" % (theta.tolist(), truth.tolist()))
    else:
        r0 = th.full((1, N), 0.25 + float(truth[0]) * float(truth[2]) * 2.5 / N, device=dev, requires_grad=True)     # the truth's mean: a flat ring
        opt = th.optim.Adam([r0], lr=args.lr)
        for it in range(args.iters + 1):
            opt.zero_grad()
            if args.fused_loss:
                loss = roll(r0, target=field)[4].sum()
            else:
                loss = ((roll(r0, detectors=det)[4][:, :, 0] - obs) ** 2).sum()
            print("iter %d %.6e" % (it, float(loss)))
            if it < args.iters:
                loss.backward()
                opt.step()
        print("error of r0 %.3e (flat start %.3e)" % (float((r0.detach() - r_true).abs().max()), float((r_true - r_true.mean()).abs().max())))
    m0, m1 = float(r_true.double().sum()), float(rT.double().sum())
    bound = T * N * 2.0 ** -24 * float(seen[:, :, 0].max())
    print("mass before %.9f after %.9f difference %.2e bound %.2e %s" % (m0, m1, abs(m1 - m0), bound,
                                                                            "conserved" if abs(m1 - m0) <= bound else "NOT conserved"))


if __name__ == "__main__":
    main()
