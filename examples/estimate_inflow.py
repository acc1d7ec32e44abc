#!/usr/bin/env python3
"""Inflow estimation on a macroscopic lane: which upstream density profile produced these downstream detector readings?

A lane starts in a known uniform free-flow state.  The truth is a smooth density pulse in the upstream boundary cell (a platoon
arriving), the cell at its equilibrium speed; the downstream boundary cell stays at the initial state.  A few detectors downstream
record the density after every step.  From those readings alone the [T] upstream density profile is recovered with Adam: the loss is
on the detector READINGS (dhts.macro_rollout with detectors=...: the state at those cells after every step, nothing of size
[T][L][N]) and its gradient reaches every step's boundary cell through the per-step boundary cotangent of the fused rollout
(ghost_r, ghost_u of shape [T][L][2]).  --readings history takes the readings out of the full state history (want_hist=True)
instead: the same numbers, log line for log line, at the cost of the history.  --checkpoint [S] keeps the state every S steps
instead of the rollout tape and replays a segment at a time in the reverse sweep: again the same log, for horizons whose tape does not
fit the device.  --readings field fits the whole density field instead of a few detectors (a density field from video or trajectory
data): the loss, summed in double, is on the density plane of the want_hist=True history; with --checkpoint [S] --fused-loss the
checkpointed kernels read the observed field themselves (dhts.macro_rollout(checkpoint=..., target=...); its speed plane is NaN, not
observed) and return the sums, so that neither the history nor its cotangent exists: the same profile errors and, to the rounding of a
double sum, the same losses.  Every trial solves n_lane independent problems at
once.  What a detector at cell c can see of the profile ends c cells' travel time before the end of the horizon: the tail of the
profile stays at its first guess.

Same output conventions as inverse_macro.py: one log line "{profile_error} {loss}" per episode in
result/inflow/<run>/gd/trial_<k>.txt and one summary line per trial.  PyTorch does the optimiser step; every simulated step (forward
and adjoint) runs in the HIP kernels.
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
    ap = argparse.ArgumentParser("Upstream inflow profile from downstream detectors (gradient descent, MI355X)")
    ap.add_argument("--n_trial", type=int, default=1)
    ap.add_argument("--n_cell", type=int, default=64)
    ap.add_argument("--n_timestep", type=int, default=300)
    ap.add_argument("--cell_length", type=float, default=5.0)
    ap.add_argument("--speed_limit", type=float, default=30.0)
    ap.add_argument("--delta_time", type=float, default=0.01)
    ap.add_argument("--n_episode", type=int, default=100)
    ap.add_argument("--n_lane", type=int, default=1)
    ap.add_argument("--n_detector", type=int, default=4)
    ap.add_argument("--lr", type=float, default=2e-2)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--readings", choices=("detectors", "history", "field"), default="detectors",
                    help="read the detectors through dhts.macro_rollout(detectors=...) or out of the full state history; field: fit the "
                         "density of every cell after every step")
    ap.add_argument("--checkpoint", nargs="?", type=int, const=0, default=None, metavar="S",
                    help="reverse mode from checkpoints instead of the tape (dhts.macro_rollout(checkpoint=...)): the same log, and no "
                         "buffer of the rollout grows with --n_timestep faster than 8 B per cell per S steps; without S the plan's segment")
    ap.add_argument("--fused-loss", action="store_true",
                    help="with --readings field --checkpoint: the squared error and its gradient inside the checkpointed kernels "
                         "(dhts.macro_rollout(target=...)), no state history")
    ap.add_argument("--run_name", default=None)
    args = ap.parse_args()
    if args.fused_loss and (args.readings != "field" or args.checkpoint is None):
        ap.error("--fused-loss goes with --readings field --checkpoint [S]")
    if args.checkpoint is not None and (args.readings == "history" or (args.readings == "field" and not args.fused_loss)):
        ap.error("--checkpoint goes with --readings detectors, or with --readings field --fused-loss: the state history is of size "
                 "n_timestep anyway")
    checkpoint = None if args.checkpoint is None else (True if args.checkpoint == 0 else args.checkpoint)

    dev = th.device("cuda", 0)
    if args.seed is not None:
        th.manual_seed(args.seed)
    L, N, T, um = args.n_lane, args.n_cell, args.n_timestep, args.speed_limit
    dt, dx = args.delta_time, args.cell_length
    run = args.run_name or "inflow_{}".format(time.strftime("%Y%m%d_%H%M%S"))
    log_dir = os.path.join("result", "inflow", run, "gd")
    os.makedirs(log_dir, exist_ok=True)
    # detectors in the first eighth of the lane: at free-flow speed the pulse covers about a cell per 30 steps (dx = 5, dt = 0.01)
    det = th.unique(th.linspace(0, max(N // 8, 1), args.n_detector, device=dev).long().clamp(0, N - 1))
    det32 = det.to(th.int32)                                           # on the device already: used as it is, no upload per episode
    r_base = 0.2

    def densities(gr, gu):
        """[T][L][detectors]: the density at the detectors after every step."""
        if args.readings == "detectors":
            return dhts.macro_rollout(r0, u0, gr, gu, T, dt, dx, um, detectors=det32, checkpoint=checkpoint)[4][:, :, 0].contiguous()
        if args.readings == "field":
            return dhts.macro_rollout(r0, u0, gr, gu, T, dt, dx, um, want_hist=True)[4][:, :, 0]
        return dhts.macro_rollout(r0, u0, gr, gu, T, dt, dx, um, want_hist=True)[4][:, :, 0][:, :, det]

    def loss_of(gr, gu):
        if args.fused_loss:                    # the kernels hold the rollout against `target` themselves: sse [L][2] in double
            return dhts.macro_rollout(r0, u0, gr, gu, T, dt, dx, um, checkpoint=checkpoint, target=target)[4][:, 0].sum()
        if args.readings == "field":
            return ((densities(gr, gu).double() - obs.double()) ** 2).sum()
        return ((densities(gr, gu) - obs) ** 2).sum()

    def u_eq(r):
        return um * (1.0 - th.sqrt(r + 1e-5))

    def schedule(up_r):
        """[T][L] upstream densities -> boundary (r, u) [T][L][2]: upstream at its equilibrium speed, downstream the base state."""
        down = th.full_like(up_r, r_base)
        return th.stack([up_r, down], dim=-1), th.stack([u_eq(up_r), u_eq(down)], dim=-1)

    for trial in range(args.n_trial):
        r0 = th.full((L, N), r_base, device=dev)
        u0 = u_eq(r0)
        tt = th.arange(T, device=dev, dtype=th.float32)[:, None]
        peak = 0.35 + 0.25 * th.rand(1, L, device=dev)                 # pulse height, centre and width differ per lane
        mid = (0.25 + 0.15 * th.rand(1, L, device=dev)) * T
        wid = (0.08 + 0.06 * th.rand(1, L, device=dev)) * T
        up_true = r_base + peak * th.exp(-((tt - mid) / wid) ** 2)     # [T][L]
        with th.no_grad():
            obs = densities(*schedule(up_true)).clone()                # the density readings
            if args.fused_loss:                                        # [T][L][2][N]: the observed densities; no speed is observed
                target = th.stack([obs, th.full_like(obs, float("nan"))], dim=2).contiguous()
        up_est = th.full((T, L), r_base, device=dev, requires_grad=True)
        opt = th.optim.Adam([up_est], lr=args.lr)
        lines = []
        t0 = time.time()
        for ep in range(args.n_episode):
            gr, gu = schedule(up_est)
            loss = loss_of(gr, gu)
            err = ((up_est.detach() - up_true) ** 2).sum()
            opt.zero_grad(set_to_none=False)
            loss.backward()
            opt.step()
            with th.no_grad():
                up_est.clamp_(0.0, 1.0)
            lines.append("{} {}\n".format(err.item(), loss.item()))
        th.cuda.synchronize()
        dt_wall = time.time() - t0
        with open(os.path.join(log_dir, "trial_{}.txt".format(trial)), "w") as f:
            f.writelines(lines)
        first, last = lines[0].split(), lines[-1].split()
        print("Trial # {}: loss {:.6f} -> {:.6f}, profile error {:.6f} -> {:.6f} in {} episodes, {:.2f} s "
              "({:.3e} differentiable cell-steps/s)".format(trial, float(first[1]), float(last[1]), float(first[0]), float(last[0]),
                                                            args.n_episode, dt_wall, L * N * T * args.n_episode / dt_wall))


if __name__ == "__main__":
    main()
