#!/usr/bin/env python3
"""Ramp metering on a macroscopic lane: how much of an on-ramp's demand should be let onto the mainline in every step?

A lane runs into a bottleneck: its downstream boundary cell is dense and slow, and the congestion that starts there grows upstream.
One on-ramp a third of the way down the lane has a demand that arrives on a schedule (a smooth pulse, a platoon reaching the ramp).
What is admitted, rate[t] (vehicles per second as normalised density times metres per second), enters the ramp cell as a density
rate rate[t] / dx through dhts.macro_rollout(..., checkpoint=True, ramps=[cell], inflow=...): a source term behind every step of the
fused rollout, differentiable per step.  What is held back waits in the ramp queue, kept in torch:

    w[t + 1] = w[t] + dt (demand[t] - rate[t])

Adam minimises the total time spent -- the mainline density summed over detectors spread along the lane and over the steps
(detectors=: the readings after every step, nothing of size [T][L][N]), plus the queue summed over the steps -- plus a penalty on a
negative queue (vehicles admitted before they arrived).  The first guess admits the mean demand in every step, which does just that
in the early steps; the gradient reaches every step's rate through the queue and through the rollout's inflow.grad.

--estimate turns the problem round: the ramp's demand is admitted as it arrives, detectors downstream of the ramp record the density
after every step, and the [T] profile is recovered from those readings alone, starting from an empty ramp.

--estimate --method lm knows that the demand is a pulse and fits its three numbers (height, centre, width) instead of T free rates, by
Levenberg-Marquardt as fit_pulse.py does: the [T * D] x 3 Jacobian of the readings is ONE dhts.macro_rollout_jvp(fused=True, ramps=,
inflow=, t_inflow=) call with K = 3 directions, t_inflow = d rate / d theta / dx -- the rollout and its three tangents in one kernel, no
tape --, a step is kept where it lowers the lane's loss and the damping follows.

Same output conventions as estimate_inflow.py: one log line "{aux} {loss}" per episode in result/ramp/<run>/<meter|estimate>/trial_<k>.txt
(aux: the largest queue resp. the profile error) and one summary line per trial.  PyTorch does the optimiser step and the
queue; every simulated step (forward and adjoint) runs in the HIP kernels.
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
    ap = argparse.ArgumentParser("Ramp metering / ramp demand estimation through the on-ramp source of the ARZ rollout (MI355X)")
    ap.add_argument("--n_trial", type=int, default=1)
    ap.add_argument("--n_cell", type=int, default=64)
    ap.add_argument("--n_timestep", type=int, default=300)
    ap.add_argument("--cell_length", type=float, default=5.0)
    ap.add_argument("--speed_limit", type=float, default=30.0)
    ap.add_argument("--delta_time", type=float, default=0.01)
    ap.add_argument("--n_episode", type=int, default=100)
    ap.add_argument("--n_lane", type=int, default=1)
    ap.add_argument("--n_detector", type=int, default=8)
    ap.add_argument("--lr", type=float, default=0.0, help="0: 0.02 for metering, 0.1 for --estimate (rates are of order 1)")
    ap.add_argument("--penalty", type=float, default=1e3, help="weight of the squared negative queue")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--estimate", action="store_true", help="recover the ramp's demand profile from downstream detector readings")
    ap.add_argument("--method", choices=("adam", "lm"), default="adam",
                    help="--estimate: adam fits T free rates; lm fits the pulse's height, centre and width by Levenberg-Marquardt")
    ap.add_argument("--damping", type=float, default=1e-2, help="--method lm: the first damping factor")
    ap.add_argument("--run_name", default=None)
    args = ap.parse_args()
    if args.method == "lm" and not args.estimate:
        ap.error("--method lm fits the demand profile: it goes with --estimate")

    dev = th.device("cuda", 0)
    if args.seed is not None:
        th.manual_seed(args.seed)
    L, N, T, um = args.n_lane, args.n_cell, args.n_timestep, args.speed_limit
    dt, dx = args.delta_time, args.cell_length
    run = args.run_name or "ramp_{}".format(time.strftime("%Y%m%d_%H%M%S"))
    log_dir = os.path.join("result", "ramp", run, "estimate" if args.estimate else "meter")
    os.makedirs(log_dir, exist_ok=True)
    ramp = max(N // 3, 1)
    ramps = th.tensor([ramp], dtype=th.int32, device=dev)             # on the device already: used as it is, no upload per episode
    if args.estimate:      # downstream of the ramp, within reach of what enters there during the horizon
        det = th.unique(th.linspace(ramp, min(ramp + max(N // 8, 1), N - 1), args.n_detector, device=dev).long())
    else:
        det = th.unique(th.linspace(0, N - 1, args.n_detector, device=dev).long())
    det32 = det.to(th.int32)
    spacing = N / det.numel()                                         # cells a detector stands for
    lr = args.lr or (0.1 if args.estimate else 0.02)

    def u_eq(r):
        return um * (1.0 - th.sqrt(r + 1e-5))

    def densities(rate):
        """[T][L][detectors]: the density at the detectors after every step, with rate [T][L] admitted at the ramp."""
        inflow = (rate / dx)[:, :, None].contiguous()                 # [T][L][1]: density per second
        return dhts.macro_rollout(r0, u0, ghost_r, ghost_u, T, dt, dx, um, detectors=det32, checkpoint=True, ramps=ramps,
                                  inflow=inflow)[4][:, :, 0]

    def queue(rate):
        """[T + 1][L]: the ramp queue in front of every step and behind the last, as normalised density times metres (like r dx)."""
        return th.cat([th.zeros(1, L, device=dev), th.cumsum(dt * (demand - rate), dim=0)], dim=0)

    def pulse(p):
        """p [L][3] = (height, centre / T, width / T) -> the rate [T][L] and z = (t - centre) / width."""
        z = (tt - p[:, 1][None] * T) / (p[:, 2][None] * T)
        return p[:, 0][None] * th.exp(-z ** 2), z

    def clamp(p):
        return th.minimum(th.maximum(p, th.tensor([0.0, 0.0, 1.0 / T], device=dev)), th.tensor([10.0, 1.0, 1.0], device=dev))

    def jacobian(p):
        """The density readings [T][L][D] and their Jacobian w.r.t. p [L][T * D][3]: one K = 3 call of the fused forward + tangent kernel."""
        rate, z = pulse(p)
        w = p[:, 2][None] * T
        d_rate = th.stack([th.exp(-z ** 2), rate * 2 * z / w * T, rate * 2 * z ** 2 / w * T])      # [3][T][L]: d rate / d (h, c / T, w / T)
        primal, tang = dhts.macro_rollout_jvp(r0, u0, ghost_r, ghost_u, T, dt, dx, um, detectors=det32, fused=True, ramps=ramps,
                                              inflow=(rate / dx)[:, :, None].contiguous(), t_inflow=(d_rate / dx)[:, :, :, None].contiguous())
        D = det32.numel()
        return primal[4][:, :, 0], tang[3][:, :, :, 0].permute(2, 1, 3, 0).reshape(L, T * D, 3)

    for trial in range(args.n_trial):
        r0 = th.full((L, N), 0.25, device=dev)
        u0 = u_eq(r0)
        # upstream: the initial state arriving; downstream: the bottleneck, dense and slow
        ghost_r = th.tensor([0.25, 0.75], device=dev).repeat(L, 1)
        ghost_u = th.stack([u_eq(ghost_r[:, 0]), 0.25 * u_eq(ghost_r[:, 1])], dim=-1)
        tt = th.arange(T, device=dev, dtype=th.float32)[:, None]
        peak = 2.0 + 1.5 * th.rand(1, L, device=dev)                  # pulse height, centre and width differ per lane
        mid = (0.35 + 0.15 * th.rand(1, L, device=dev)) * T
        wid = (0.10 + 0.05 * th.rand(1, L, device=dev)) * T
        demand = peak * th.exp(-((tt - mid) / wid) ** 2)              # [T][L]
        if args.estimate:
            with th.no_grad():
                obs = densities(demand).clone()
        lines = []
        t0 = time.time()
        if args.method == "lm":
            p = th.tensor([1.5, 0.5, 0.2], device=dev).repeat(L, 1)      # a low, late, wide pulse
            lam = th.full((L,), args.damping, device=dev)
            for ep in range(args.n_episode):
                rd, jac = jacobian(p)
                res = (rd - obs).permute(1, 0, 2).reshape(L, -1)                                   # [L][T D]
                loss = (res ** 2).sum(dim=1)
                lines.append("{} {}\n".format(((pulse(p)[0] - demand) ** 2).sum().item(), loss.sum().item()))
                jtj = jac.transpose(1, 2) @ jac                                                    # [L][3][3]
                jtr = (jac.transpose(1, 2) @ res[:, :, None])[:, :, 0]
                damp = th.diag_embed(lam[:, None] * th.diagonal(jtj, dim1=1, dim2=2).clamp_min(1e-12))
                step = -th.linalg.solve((jtj + damp).double().cpu(), jtr.double().cpu()).float().to(dev)      # (3 x 3 per lane)
                trial_p = clamp(p + step)
                with th.no_grad():
                    new_loss = ((densities(pulse(trial_p)[0]) - obs) ** 2).sum(dim=(0, 2))
                better = new_loss < loss
                p = th.where(better[:, None], trial_p, p)
                lam = th.where(better, lam / 3.0, lam * 3.0).clamp(1e-9, 1e9)
        else:
            if args.estimate:
                rate = th.zeros(T, L, device=dev, requires_grad=True)
            else:
                rate = demand.mean(dim=0, keepdim=True).repeat(T, 1).requires_grad_(True)
            opt = th.optim.Adam([rate], lr=lr)
            for ep in range(args.n_episode):
                if args.estimate:
                    loss = ((densities(rate) - obs) ** 2).sum()
                    aux = ((rate.detach() - demand) ** 2).sum()
                else:
                    w = queue(rate)
                    tts = dt * (densities(rate).sum() * spacing * dx + w[1:].sum())
                    loss = tts + args.penalty * (th.relu(-w) ** 2).sum()
                    aux = w.detach().max()
                opt.zero_grad(set_to_none=False)
                loss.backward()
                opt.step()
                with th.no_grad():
                    rate.clamp_(min=0.0)
                lines.append("{} {}\n".format(aux.item(), loss.item()))
        th.cuda.synchronize()
        dt_wall = time.time() - t0
        with open(os.path.join(log_dir, "trial_{}.txt".format(trial)), "w") as f:
            f.writelines(lines)
        first, last = lines[0].split(), lines[-1].split()
        print("Trial # {}: loss {:.6f} -> {:.6f}, {} {:.6f} -> {:.6f} in {} episodes, {:.2f} s "
              "({:.3e} differentiable cell-steps/s)".format(trial, float(first[1]), float(last[1]),
                                                            "profile error" if args.estimate else "largest queue", float(first[0]),
                                                            float(last[0]), args.n_episode, dt_wall, L * N * T * args.n_episode / dt_wall))


if __name__ == "__main__":
    main()
