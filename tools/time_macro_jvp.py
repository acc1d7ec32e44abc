#!/usr/bin/env python3
"""Time the tangent sweep (dhts_macro_rollout_jvp) against the reverse sweep of the same tape on one GPU, and the tape-free fused
forward + tangent kernel (dhts_macro_rollout_fwd_jvp) against what it replaces: the forward that writes the tape plus the sweep.

BASELINE config 2's shape by default (1024 lanes x 512 cells x 1000 steps, bench.py's seeded inputs, the tape written by the
benchmarked forward kernel).  Device events around each launch, warm-up passes first, the kernels ALTERNATING inside every timed pass
(reverse sweep, the forward with its tape, then per K = 1, 2, 4, ... directions the sweep and the fused call) so that a drift of the box
reaches all of them alike; the median and the spread of the passes are reported, "fused" with the time of the pair it replaces
(replaces_ms = fwd_tape + the sweep of the same K), their ratio, and the [T]-sized bytes each path allocates.  --detectors D: the
detector forms of all three (D cells spread over the first eighth of the lane, as examples/fit_pulse.py places them).  Prints one JSON
line; needs a GPU (there is no CPU path).

    python tools/time_macro_jvp.py [--lanes 1024 --cells 512 --steps 1000 --dirs 1 2 3 4 8 --passes 15 --warmup 3 --detectors 0]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diff-hybrid-traffic-sim_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=1024)
    ap.add_argument("--cells", type=int, default=512)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--dirs", type=int, nargs="+", default=[1, 2, 3, 4, 8])
    ap.add_argument("--passes", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--detectors", type=int, default=0, help="detector cells (0: none)")
    ap.add_argument("--general", action="store_true", help="DHTS_OPT_MACRO_JVP_VARIANT = 1: the general kernel")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_macro_jvp.py needs a GPU")
    from bench import MacroWorkload
    from dhts import _lib, ops
    dev = torch.device("cuda:0")
    L, N, T, um = args.lanes, args.cells, args.steps, 30.0
    r0, u0, gr, gu = (t.to(dev) for t in MacroWorkload.inputs(0, L, N, um))
    desc = ops.macro_desc(L, N, 0.01, 5.0, um)
    y0, q0 = ops.macro_state_from_ru(r0, u0, um)
    gy, gq = ops.macro_state_from_ru(gr, gu, um)
    ghost = torch.stack([gr, gy, gu, gq], dim=-1).contiguous()
    tape = torch.zeros(ops.macro_tape_numel(desc, T), dtype=torch.float32, device=dev)
    err = ops.new_error_record(dev)
    det = None
    if args.detectors > 0:
        det = torch.unique(torch.linspace(0, max(N // 8, 1), args.detectors, device=dev).long().clamp(0, N - 1)).to(torch.int32)
    D = det.numel() if det is not None else 0
    out_f = tuple(torch.empty_like(r0) for _ in range(4))
    taps = torch.empty(T, L, 3, D, dtype=torch.float32, device=dev) if D else None

    def forward_with_tape():
        if det is not None:
            return ops.macro_rollout_fwd_taps(desc, T, r0, y0, u0, q0, ghost, det, tape=tape, err=err, out=out_f, taps=taps)[0]
        return ops.macro_rollout_fwd(desc, T, r0, y0, u0, q0, ghost, tape=tape, err=err, out=out_f)

    rT, yT, uT, _ = (t.clone() for t in forward_with_tape())
    assert err.tolist()[0] == 0, err.tolist()
    if args.general:
        assert _lib.lib().dhts_set_option(_lib.OPT_MACRO_JVP_VARIANT, 1) == 0
    kmax = max(args.dirs)
    gen = torch.Generator(device="cpu").manual_seed(7)
    t_r, t_y = (torch.randn(kmax, L, N, generator=gen).to(dev) for _ in range(2))
    t_g = torch.randn(kmax, L, 2, 2, generator=gen).to(dev)
    g_r, g_y = 2 * rT, torch.zeros_like(rT)
    ops.macro_u_tap_bwd(rT, yT, 2 * uT, g_r, g_y, um)
    out_b = (torch.empty_like(g_r), torch.empty_like(g_y))
    out_j = (torch.empty_like(t_r), torch.empty_like(t_y))
    g_ghost = torch.zeros(L, 2, 2, dtype=torch.float64, device=dev)
    t_taps = torch.empty(kmax, T, L, 2, D, dtype=torch.float32, device=dev) if D else None
    out_p = tuple(torch.empty_like(r0) for _ in range(4))
    err_jvp = ops.new_error_record(dev)
    fused_kmax = ops.macro_fwd_jvp_plan(desc, T, kmax)["dirs_per_launch"]      # 0: the lane does not fit the fused kernel

    def run(what):
        if what == "bwd":
            ops.macro_rollout_bwd(desc, T, tape, g_r, g_y, err=err, out=out_b, g_ghost=g_ghost)
        elif what == "fwd_tape":
            forward_with_tape()
        elif isinstance(what, tuple):              # ("fused", K)
            k = what[1]
            ops.macro_rollout_fwd_jvp(desc, T, r0, y0, u0, q0, ghost, t_r[:k], t_y[:k], t_ghost=t_g[:k], det=det, err=err, err_jvp=err_jvp,
                                      out=out_p + (out_j[0][:k], out_j[1][:k]), taps=taps, t_taps=t_taps[:k] if D else None)
        else:
            ops.macro_rollout_jvp(desc, T, tape, t_r[:what], t_y[:what], t_ghost=t_g[:what], det=det, err=err,
                                  out=(out_j[0][:what], out_j[1][:what]), t_taps=t_taps[:what] if D else None)

    kinds = ["bwd", "fwd_tape"]
    for k in args.dirs:
        kinds += [k, ("fused", k)] if fused_kmax > 0 else [k]
    times = {k: [] for k in kinds}
    for p in range(args.warmup + args.passes):
        for k in kinds:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(k)
            b.record()
            b.synchronize()
            if p >= args.warmup:
                times[k].append(a.elapsed_time(b))
    assert err.tolist()[0] == 0 and err_jvp.tolist()[0] == 0, (err.tolist(), err_jvp.tolist())

    def stat(v):
        return dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))

    bwd = statistics.median(times["bwd"])
    rec = dict(shape=[L, N, T], detectors=D, passes=args.passes, tape_bytes=tape.numel() * 4, general=bool(args.general),
               plan={str(k): ops.macro_jvp_plan(desc, T, k) for k in args.dirs}, bwd=stat(times["bwd"]), fwd_tape=stat(times["fwd_tape"]),
               jvp={}, fused={})
    one = statistics.median(times[1]) if 1 in times else None
    for k in args.dirs:
        s = stat(times[k])
        s["over_bwd"] = round(s["median_ms"] / bwd, 3)
        if one:
            s["over_k1"] = round(s["median_ms"] / one, 3)
            s["ms_per_direction"] = round(s["median_ms"] / k, 4)
        rec["jvp"][str(k)] = s
        if fused_kmax > 0:
            f = stat(times[("fused", k)])
            f["replaces_ms"] = round(statistics.median(times["fwd_tape"]) + statistics.median(times[k]), 4)
            f["over_replaced"] = round(f["median_ms"] / f["replaces_ms"], 3)
            f["ms_per_direction"] = round(f["median_ms"] / k, 4)
            f["plan"] = ops.macro_fwd_jvp_plan(desc, T, k, D)
            readings = 4 * T * L * D * (3 + 2 * k)                              # taps + t_taps: what the caller asked for
            f["t_sized_bytes"] = dict(fused=readings, taped=readings + tape.numel() * 4)
            rec["fused"][str(k)] = f
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
