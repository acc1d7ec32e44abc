#!/usr/bin/env python3
"""Calibration of IDM drivers from observed trajectories: the inverse problem the parameter gradient of the fused micro rollout serves.

L lanes of V vehicles (example/inverse/micro.py's initial states: 4 len spacing + U[0, 2 len) jitter, v ~ lerp(0.3, 0.7) u_max), all
driven by ONE shared driver theta = (accel_max, accel_pref, target_speed, min_space, time_pref); the observed trajectories are a rollout
of the ground-truth driver (MicroVehicle.default_micro_vehicle).  params = theta[:, None, None].expand(...) puts the same five numbers
(and the fixed vehicle length) on every vehicle, so autograd sums the per-vehicle gradients of dhts.micro_rollout back onto theta;
loss = mean squared distance to the observed (p, v) at every step; Adam on theta, kept inside a box around the initial guess.
--method lm fits the same five numbers with Levenberg-Marquardt instead: the residuals are the T x L x 2 x V trajectory differences, and
their Jacobian has five columns, so ONE dhts.micro_rollout_jvp call with K = 5 directions (unit direction i of theta expanded over
every vehicle, want_hist=True) returns the trajectories AND the whole Jacobian in one pass over the rollout tape; the 5 x 5 normal
equations are formed and solved on the device, a step is kept where it lowers the loss (one more rollout, no tape) and the damping
follows.  Same box, same log.  --fused steps the rollout and the five tangents in one kernel (fused=True): no tape, no parameter tape,
the same numbers bit for bit.  --checkpoint [S] (Adam) runs the reverse mode from checkpoints (dhts.micro_rollout(checkpoint=...)): the
state every S steps (the library's own S when none is given) instead of 20 B of tapes per vehicle-step, the same log bit for bit.
--observe P,E: floating-car data instead of a dense history -- the truth and the fit both observe P evenly spaced probe slots of every
lane every E-th step (dhts.micro_rollout(probes=, every=) / micro_rollout_jvp(probes=, every=)); residuals and Jacobian are then
T // E x L x 2 x P numbers, and with --checkpoint / --fused nothing of size T x V is allocated.  Works with every method and path.
--leader: "leader trajectory given, followers observed", the form of every real car-following data set -- the ground truth is a
rollout of n_vehicle + 1 vehicles per lane on the existing path; the head vehicle's recorded trajectory becomes `lead`
(dhts.micro_rollout(lead=, lead_length=) / micro_rollout_jvp(lead=, ...)), and the n_vehicle followers behind it are fitted.  A
recorded leader lives on the tape-free paths: with --checkpoint (Adam) or --method lm --fused, each with or without --observe.
--fused-loss (with --checkpoint, Adam, the dense fit, with or without --leader): the kernels read the observed trajectories themselves
(dhts.micro_rollout(target=observed)) and return the squared error per lane, loss = sse.sum() / observed.numel(); neither the history
nor its cotangent is allocated, so the fit holds `observed` and the checkpoints and nothing else of size T x V.  The same log up to
the summation order of the loss (float64 in the kernels, float32 in torch.mean).
--method lm --fused --fused-loss: the normal equations inside the fused kernel (dhts.micro_rollout_jvp(fused=True, target=observed)) --
the call returns sse [L][2], J^T r [L][5] and J^T J [L][5][5] in float64, summed over the lanes here, instead of hist and five
directions of t_hist; the trial step's loss is dhts.micro_rollout(checkpoint=True, target=observed)'s sse without grad (with --observe
the sse of the same fused call with one direction: the checkpointed target form is dense).  The fit then holds `observed` and nothing else of size T x V, with
and without --observe, --leader and --ring.  The same first loss up to the summation order; the later lines pass through the solve.
--ring C: the closed experiment of car-following research -- n_vehicle drivers on a ring road of circumference C metres, the head
following the tail one circumference ahead (dhts.micro_rollout(ring=) / micro_rollout_jvp(ring=)).  The truth is a ring rollout of a
perturbed platoon (even spacing C / n_vehicle with a jitter, random speeds: what grows into stop-and-go waves), and the fit runs on the
same ring.  A ring lives on the tape-free paths: with --checkpoint (Adam, optionally --fused-loss or --observe) or --method lm --fused.
Log lines "{parameter_error} {loss}" per iteration in result/calibrate/<run>/gd/trial_k.txt (lm: .../lm/trial_k.txt), like the other examples.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diff-hybrid-traffic-sim_amd"))

import torch as th  # noqa: E402

import dhts  # noqa: E402
from road.vehicle.micro_vehicle import MicroVehicle  # noqa: E402


def main():
    ap = argparse.ArgumentParser("IDM calibration from trajectories (gradient descent on the driver parameters, MI355X)")
    ap.add_argument("--n_trial", type=int, default=1)
    ap.add_argument("--n_lane", type=int, default=64)
    ap.add_argument("--n_vehicle", type=int, default=32)
    ap.add_argument("--n_step", type=int, default=200)
    ap.add_argument("--vehicle_length", type=float, default=5.0)
    ap.add_argument("--speed_limit", type=float, default=30.0)
    ap.add_argument("--delta_time", type=float, default=0.01)
    ap.add_argument("--n_episode", type=int, default=100)
    ap.add_argument("--lr", type=float, default=2e-2)
    ap.add_argument("--method", choices=("adam", "lm"), default="adam")
    ap.add_argument("--damping", type=float, default=1e-2, help="Levenberg-Marquardt: the first damping factor")
    ap.add_argument("--fused", action="store_true", help="Levenberg-Marquardt: rollout and tangents in one tape-free kernel")
    ap.add_argument("--checkpoint", type=int, nargs="?", const=True, default=None, metavar="S",
                    help="Adam: reverse mode from checkpoints every S steps (no S: the library's choice) instead of the tapes")
    ap.add_argument("--observe", default=None, metavar="P,E",
                    help="observe P evenly spaced probe slots per lane every E-th step instead of every vehicle at every step")
    ap.add_argument("--leader", action="store_true",
                    help="fit the followers of a recorded leader: the truth has n_vehicle + 1 vehicles, its head's trajectory is given")
    ap.add_argument("--fused-loss", action="store_true",
                    help="Adam with --checkpoint: the squared error and its gradient inside the rollout kernels (target=), no history; "
                         "--method lm --fused: the normal equations J^T J, J^T r and the loss inside the fused kernel")
    ap.add_argument("--ring", type=float, default=None, metavar="C",
                    help="a ring road of circumference C metres: the head vehicle follows the tail (needs --checkpoint or --method lm --fused)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--run_name", default=None)
    args = ap.parse_args()
    if args.fused and args.method != "lm":
        ap.error("--fused belongs to --method lm")
    if args.checkpoint is not None and args.method != "adam":
        ap.error("--checkpoint belongs to --method adam")
    if args.leader and not (args.fused or args.checkpoint is not None):
        ap.error("--leader lives on the tape-free paths: add --checkpoint (Adam) or --method lm --fused")
    if args.ring is not None and not (args.fused or args.checkpoint is not None):
        ap.error("--ring lives on the tape-free paths: add --checkpoint (Adam, optionally --fused-loss or --observe) or --method lm --fused")
    if args.ring is not None and args.leader:
        ap.error("--ring and --leader exclude each other: on a ring the head vehicle follows the tail")
    if args.ring is not None and args.ring < 2.0 * args.vehicle_length * args.n_vehicle:
        ap.error("--ring C is too short for n_vehicle vehicles: give each at least two vehicle lengths")
    if args.fused_loss and args.method == "lm" and not args.fused:
        ap.error("--fused-loss with --method lm forms the normal equations in the fused kernel: add --fused")
    if args.fused_loss and args.method == "adam" and (args.checkpoint is None or args.observe is not None):
        ap.error("--fused-loss is the dense fit on the checkpointed path: add --checkpoint, drop --observe")
    sampled = {}                                  # the arguments of a sampled call; none: the dense history
    if args.observe is not None:
        try:
            n_probe, every = (int(x) for x in args.observe.split(","))
        except ValueError:
            ap.error("--observe takes two integers: P,E")
        if not (1 <= n_probe <= args.n_vehicle and every >= 1):
            ap.error("--observe P,E needs 1 <= P <= n_vehicle and E >= 1")
        sampled = dict(probes=[(2 * i + 1) * args.n_vehicle // (2 * n_probe) for i in range(n_probe)], every=every)

    dev = th.device("cuda", 0)
    th.manual_seed(args.seed)
    L, V, T, um, ln, dt = args.n_lane, args.n_vehicle, args.n_step, args.speed_limit, args.vehicle_length, args.delta_time
    run = args.run_name or "idm_{}".format(time.strftime("%Y%m%d_%H%M%S"))
    log_dir = os.path.join("result", "calibrate", run, "gd" if args.method == "adam" else args.method)
    os.makedirs(log_dir, exist_ok=True)

    truth = th.tensor(MicroVehicle.default_micro_vehicle(um).params(), dtype=th.float64, device=dev)
    length = truth[5:6]
    head = th.tensor([[1000.0, 0.0]], dtype=th.float64, device=dev).expand(L, 2).contiguous()

    # --leader: the recorded leader of a trial (lead, lead_length), made with its truth; --ring: the circumference of every lane's ring
    follow = {} if args.ring is None else dict(ring=th.full((L,), args.ring, dtype=th.float64, device=dev))
    # with a leader or on a ring the dense history is the sampled form of every slot at every step
    observe = sampled or dict(probes=list(range(V)), every=1)

    def rollout(theta):
        params = th.cat([theta, length])[:, None, None].expand(6, L, V)
        if follow:
            return dhts.micro_rollout(p0, v0, params, None, T, dt, checkpoint=True if args.fused else args.checkpoint, **follow, **observe)[2]
        if sampled:      # (the fused fit's loss evaluations: the tape-free forward too, no grad is asked of it)
            return dhts.micro_rollout(p0, v0, params, head, T, dt, checkpoint=True if args.fused else args.checkpoint, **sampled)[2]
        return dhts.micro_rollout(p0, v0, params, head, T, dt, want_hist=True, checkpoint=args.checkpoint)[2]

    def squared_error(theta):
        """--fused-loss: sum((hist - observed)^2) [L][2] float64 from the kernels; hist is never written."""
        params = th.cat([theta, length])[:, None, None].expand(6, L, V)
        return dhts.micro_rollout(p0, v0, params, None if follow else head, T, dt, checkpoint=args.checkpoint, target=observed, **follow)[2]

    for trial in range(args.n_trial):
        p0 = (th.arange(V, device=dev) * 4.0 * ln)[None, :] + th.rand(L, V, device=dev) * 2.0 * ln
        v0 = th.lerp(th.tensor(0.3 * um, device=dev), th.tensor(0.7 * um, device=dev), th.rand(L, V, device=dev))
        if args.ring is not None:
            # a perturbed platoon all around the ring: even spacing, each vehicle up to a quarter of the free road ahead of its mark
            spacing = args.ring / V
            p0 = (th.arange(V, device=dev) * spacing)[None, :] + th.rand(L, V, device=dev) * 0.25 * (spacing - ln)
        if args.leader:
            # the truth: V + 1 vehicles on the existing path; the head's (p, v) before every step is the record the fit is given
            p_all = th.cat([p0, p0[:, -1:] + 4.0 * ln + th.rand(L, 1, device=dev) * 2.0 * ln], 1)
            v_all = th.cat([v0, th.lerp(th.tensor(0.3 * um, device=dev), th.tensor(0.7 * um, device=dev), th.rand(L, 1, device=dev))], 1)
            with th.no_grad():
                full = dhts.micro_rollout(p_all, v_all, truth[:, None, None].expand(6, L, V + 1), head, T, dt, want_hist=True)[2]
            first = th.stack([p_all[:, V], v_all[:, V]], -1)[None]
            follow = dict(lead=th.cat([first, full[:T - 1, :, :, V]], 0).contiguous(), lead_length=length.expand(L).contiguous())
            observed = full[observe["every"] - 1::observe["every"]][..., th.tensor(observe["probes"], device=dev)].contiguous()
        else:
            with th.no_grad():
                observed = rollout(truth[:5])
        guess = truth[:5] * (1.0 + 0.2 * (2.0 * th.rand(5, dtype=th.float64, device=dev) - 1.0))
        lo, hi = 0.5 * guess, 1.5 * guess
        lines = []
        t0 = time.time()
        if args.method == "lm":
            theta, lam = guess.clone(), args.damping
            unit = th.zeros(5, 6, L, V, dtype=th.float64, device=dev)      # direction i: d params / d theta_i, the same on every vehicle
            for i in range(5):
                unit[i, i] = 1.0
            def normal_equations(theta, directions=unit):
                """--fused-loss: (loss, J^T J, J^T r) from the fused kernel; neither hist nor t_hist is written."""
                params = th.cat([theta, length])[:, None, None].expand(6, L, V)
                (_, _, sse), (_, _, jtr, jtj) = dhts.micro_rollout_jvp(p0, v0, params, None if follow else head, T, dt, t_params=directions,
                                                                        fused=True, target=observed, **follow, **sampled)
                return sse.sum() / observed.numel(), jtj.sum(0), jtr.sum(0)

            def trial_loss(theta):
                """--fused-loss: the loss alone, no grad -- the checkpointed target form, or (sampled: that form is dense) the fused call's sse."""
                if sampled:          # one direction is one launch of the narrowest kernel: the same sse
                    return normal_equations(theta, unit[:1])[0]
                params = th.cat([theta, length])[:, None, None].expand(6, L, V)
                with th.no_grad():
                    sse = dhts.micro_rollout(p0, v0, params, None if follow else head, T, dt, checkpoint=True, target=observed, **follow)[2]
                return sse.sum() / observed.numel()

            for ep in range(args.n_episode):
                params = th.cat([theta, length])[:, None, None].expand(6, L, V)
                if args.fused_loss:
                    loss, jtj, jtr = normal_equations(theta)
                    err = ((theta - truth[:5]) / truth[:5]).abs().max()
                    lines.append("{} {}\n".format(err.item(), loss.item()))
                    step = -th.linalg.solve(jtj + th.diag(lam * th.diagonal(jtj).clamp_min(1e-30)), jtr)
                    trial_theta = th.max(th.min(theta + step, hi), lo)
                    if trial_loss(trial_theta).item() < loss.item():
                        theta, lam = trial_theta, max(lam / 3.0, 1e-9)
                    else:
                        lam = min(lam * 3.0, 1e9)
                    continue
                if follow:
                    (_, _, hist), (_, _, t_hist) = dhts.micro_rollout_jvp(p0, v0, params, None, T, dt, t_params=unit, fused=True, **follow,
                                                                          **observe)
                else:
                    (_, _, hist), (_, _, t_hist) = dhts.micro_rollout_jvp(p0, v0, params, head, T, dt, t_params=unit, want_hist=not sampled,
                                                                          fused=args.fused, **sampled)
                res = (hist - observed).reshape(-1).double()
                jac = t_hist.reshape(5, -1).double()                        # [5][T L 2 V] (observed: [5][T // E L 2 P]): column i of the Jacobian
                loss = (res ** 2).mean()
                err = ((theta - truth[:5]) / truth[:5]).abs().max()
                lines.append("{} {}\n".format(err.item(), loss.item()))
                jtj, jtr = jac @ jac.T, jac @ res
                step = -th.linalg.solve(jtj + th.diag(lam * th.diagonal(jtj).clamp_min(1e-30)), jtr)
                trial_theta = th.max(th.min(theta + step, hi), lo)
                new_loss = ((rollout(trial_theta) - observed) ** 2).mean()
                if new_loss.item() < loss.item():
                    theta, lam = trial_theta, max(lam / 3.0, 1e-9)
                else:
                    lam = min(lam * 3.0, 1e9)
        else:
            theta = guess.clone().requires_grad_(True)
            opt = th.optim.Adam([theta], lr=args.lr)
            for ep in range(args.n_episode):
                if args.fused_loss:
                    loss = squared_error(theta).sum() / observed.numel()
                else:
                    loss = ((rollout(theta) - observed) ** 2).mean()
                opt.zero_grad()
                loss.backward()
                err = ((theta.detach() - truth[:5]) / truth[:5]).abs().max()
                opt.step()
                with th.no_grad():
                    theta.copy_(th.max(th.min(theta, hi), lo))
                lines.append("{} {}\n".format(err.item(), loss.item()))
        th.cuda.synchronize()
        wall = time.time() - t0
        with open(os.path.join(log_dir, "trial_{}.txt".format(trial)), "w") as f:
            f.writelines(lines)
        first, last = lines[0].split(), lines[-1].split()
        print("Trial # {}: loss {:.6g} -> {:.6g}, worst relative parameter error {:.3f} -> {:.3f} in {} episodes, {:.2f} s".format(
            trial, float(first[1]), float(last[1]), float(first[0]), float(last[0]), args.n_episode, wall))


if __name__ == "__main__":
    main()
