#!/usr/bin/env python3
"""Pulse fitting on a macroscopic lane: which platoon -- height, centre and width of a density pulse in the upstream boundary cell --
produced these downstream detector readings?

estimate_inflow.py's set-up (a lane in a uniform free-flow state, the upstream boundary cell at its equilibrium speed, a few detectors
that record the density after every step) with THREE unknowns per lane instead of a [T] profile: a nonlinear least-squares problem of
T x D residuals.  --method lm (default) solves it with Levenberg-Marquardt: one dhts.macro_rollout_jvp call with K = 3 directions -- the
pulse's own Jacobian w.r.t. (height, centre, width), formed in torch, as three tangent schedules of the boundary cell -- returns the
readings AND their [T * D] x 3 Jacobian in one pass over the rollout tape; the 3 x 3 normal equations are solved per lane in torch, a
step is kept where it lowers the lane's loss (one more rollout, no tape) and the damping follows; with --fused that call steps the
rollout and its tangents in one kernel and allocates no tape at all (dhts.macro_rollout_jvp(fused=True): the same trial file, bit for
bit, and a horizon that memory no longer limits).  --method adam fits the same three
numbers with Adam through dhts.macro_rollout and its reverse sweep, for comparison.  Every trial solves n_lane independent problems.

Same output conventions as the other examples: one log line "{parameter_error} {loss}" per episode in
result/pulse/<run>/<method>/trial_<k>.txt and one summary line per trial.  Every simulated step (forward, tangent and adjoint) runs in
the HIP kernels.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diff-hybrid-traffic-sim_amd"))

import torch as th  # noqa: E402

import dhts  # noqa: E402


def main():
    ap = argparse.ArgumentParser("Height, centre and width of an upstream density pulse from downstream detectors (MI355X)")
    ap.add_argument("--n_trial", type=int, default=1)
    ap.add_argument("--n_cell", type=int, default=64)
    ap.add_argument("--n_timestep", type=int, default=300)
    ap.add_argument("--cell_length", type=float, default=5.0)
    ap.add_argument("--speed_limit", type=float, default=30.0)
    ap.add_argument("--delta_time", type=float, default=0.01)
    ap.add_argument("--n_episode", type=int, default=20)
    ap.add_argument("--n_lane", type=int, default=1)
    ap.add_argument("--n_detector", type=int, default=4)
    ap.add_argument("--method", choices=("lm", "adam"), default="lm")
    ap.add_argument("--lr", type=float, default=2e-2, help="Adam's step, in units of (density, T steps, T steps)")
    ap.add_argument("--damping", type=float, default=1e-2, help="Levenberg-Marquardt: the first damping factor")
    ap.add_argument("--fused", action="store_true",
                    help="--method lm: step the rollout and its three tangents in one kernel, without a tape (same results, bit for bit)")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--run_name", default=None)
    args = ap.parse_args()

    dev = th.device("cuda", 0)
    if args.seed is not None:
        th.manual_seed(args.seed)
    L, N, T, um = args.n_lane, args.n_cell, args.n_timestep, args.speed_limit
    dt, dx = args.delta_time, args.cell_length
    run = args.run_name or "pulse_{}".format(time.strftime("%Y%m%d_%H%M%S"))
    log_dir = os.path.join("result", "pulse", run, args.method)
    os.makedirs(log_dir, exist_ok=True)
    det32 = th.unique(th.linspace(0, max(N // 8, 1), args.n_detector, device=dev).long().clamp(0, N - 1)).to(th.int32)
    D = det32.numel()
    r_base = 0.2
    tt = th.arange(T, device=dev, dtype=th.float32)[:, None]            # [T][1]
    scale = th.tensor([1.0, float(T), float(T)], device=dev)            # the parameters are kept in units of (density, T, T)

    def u_eq(r):
        return um * (1.0 - th.sqrt(r + 1e-5))

    def pulse(p):
        """p [L][3] = (height, centre / T, width / T) -> the upstream density [T][L] and z = (t - centre) / width."""
        h, c, w = p[:, 0][None], p[:, 1][None] * T, p[:, 2][None] * T
        z = (tt - c) / w
        return r_base + h * th.exp(-z ** 2), z

    def schedule(up_r):
        """[T][L] upstream densities -> boundary (r, u) [T][L][2]: upstream at its equilibrium speed, downstream the base state."""
        down = th.full_like(up_r, r_base)
        return th.stack([up_r, down], dim=-1), th.stack([u_eq(up_r), u_eq(down)], dim=-1)

    def densities(p):
        """[T][L][D]: the density at the detectors after every step (differentiable in p)."""
        gr, gu = schedule(pulse(p)[0])
        return dhts.macro_rollout(r0, u0, gr, gu, T, dt, dx, um, detectors=det32)[4][:, :, 0]

    def clamp(p):
        lo = th.tensor([0.0, 0.0, 1.0 / T], device=dev)
        hi = th.tensor([0.79, 1.0, 1.0], device=dev)
        return th.minimum(th.maximum(p, lo), hi)

    def jacobian(p):
        """The density readings [T][L][D] and their Jacobian w.r.t. p [L][T * D][3]: one K = 3 call."""
        up, z = pulse(p)
        ex, e = th.exp(-z ** 2), up - r_base                            # e = h exp(-z^2)
        w = p[:, 2][None] * T
        d_up = th.stack([ex, e * 2 * z / w * T, e * 2 * z ** 2 / w * T])                          # [3][T][L]: d up / d (h, c / T, w / T)
        d_ueq = -um * 0.5 / th.sqrt(up + 1e-5)                          # d u_eq / d r at the upstream cell
        zero = th.zeros_like(d_up)
        t_gr, t_gu = th.stack([d_up, zero], dim=-1), th.stack([d_up * d_ueq, zero], dim=-1)      # [3][T][L][2]
        gr, gu = schedule(up)
        primal, tang = dhts.macro_rollout_jvp(r0, u0, gr, gu, T, dt, dx, um, t_ghost_r=t_gr.contiguous(), t_ghost_u=t_gu.contiguous(),
                                              detectors=det32, fused=args.fused)
        return primal[4][:, :, 0], tang[3][:, :, :, 0].permute(2, 1, 3, 0).reshape(L, T * D, 3)

    for trial in range(args.n_trial):
        r0 = th.full((L, N), r_base, device=dev)
        u0 = u_eq(r0)
        p_true = th.stack([0.35 + 0.25 * th.rand(L, device=dev), 0.25 + 0.15 * th.rand(L, device=dev),
                           0.08 + 0.06 * th.rand(L, device=dev)], dim=1)                           # [L][3]
        with th.no_grad():
            obs = densities(p_true).clone()
        p = th.tensor([0.3, 0.3, 0.12], device=dev).repeat(L, 1)
        lines = []
        t0 = time.time()
        if args.method == "lm":
            lam = th.full((L,), args.damping, device=dev)
            for ep in range(args.n_episode):
                rd, jac = jacobian(p)
                res = (rd - obs).permute(1, 0, 2).reshape(L, T * D)                                # [L][T D]
                loss = (res ** 2).sum(dim=1)
                lines.append("{} {}\n".format((((p - p_true) * scale) ** 2).sum().item(), loss.sum().item()))
                jtj = jac.transpose(1, 2) @ jac                                                    # [L][3][3]
                jtr = (jac.transpose(1, 2) @ res[:, :, None])[:, :, 0]
                damp = th.diag_embed(lam[:, None] * th.diagonal(jtj, dim1=1, dim2=2).clamp_min(1e-12))
                step = -th.linalg.solve((jtj + damp).double().cpu(), jtr.double().cpu()).float().to(dev)      # (3 x 3 per lane)
                trial_p = clamp(p + step)
                with th.no_grad():
                    new_loss = ((densities(trial_p) - obs) ** 2).sum(dim=(0, 2))
                better = new_loss < loss
                p = th.where(better[:, None], trial_p, p)
                lam = th.where(better, lam / 3.0, lam * 3.0).clamp(1e-9, 1e9)
        else:
            p = p.clone().requires_grad_(True)
            opt = th.optim.Adam([p], lr=args.lr)
            for ep in range(args.n_episode):
                loss = ((densities(p) - obs) ** 2).sum()
                lines.append("{} {}\n".format((((p.detach() - p_true) * scale) ** 2).sum().item(), loss.item()))
                opt.zero_grad(set_to_none=False)
                loss.backward()
                opt.step()
                with th.no_grad():
                    p.copy_(clamp(p))
        th.cuda.synchronize()
        dt_wall = time.time() - t0
        with open(os.path.join(log_dir, "trial_{}.txt".format(trial)), "w") as f:
            f.writelines(lines)
        first, last = lines[0].split(), lines[-1].split()
        print("Trial # {} ({}): loss {:.6g} -> {:.6g}, parameter error {:.6g} -> {:.6g} in {} episodes, {:.2f} s".format(
            trial, args.method, float(first[1]), float(last[1]), float(first[0]), float(last[0]), args.n_episode, dt_wall))


if __name__ == "__main__":
    main()
