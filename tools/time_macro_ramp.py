#!/usr/bin/env python3
"""Time the checkpointed ARZ pair with on-ramps against the same pair without them -- forward + reverse sweep through the raw wrappers on
buffers made once, a constant boundary, on one GPU:

    a  ops.macro_rollout_fwd_ckpt + macro_rollout_bwd_ckpt            the kRamp = false kernels, which every call without ramps launches
    b  ops.macro_rollout_fwd_ckpt_ramp + macro_rollout_bwd_ckpt_ramp  the same build's kRamp = true siblings with 4 ramps spread over the
                                                                      lane (and the memset of g_inflow the reverse entry point issues)
1024 lanes x 512 cells x 1000 steps and 4096 x 64 x 1000, each plain and with 4 detectors (readings out, their cotangents back in).
Device events around one forward + reverse, warm-up passes first, the two forms ALTERNATING inside every timed pass and every pass
starting with the other one; the median and the spread of the passes and the ratio of the medians are reported.  Prints one JSON line
per shape and form; needs a GPU (there is no CPU path).

    python tools/time_macro_ramp.py [--shapes 1024x512x1000,4096x64x1000 --passes 15 --warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diff-hybrid-traffic-sim_amd"))

import torch  # noqa: E402

DT, DX, UM = 0.01, 5.0, 30.0
RAMPS = 4


def measure(dev, L, N, T, n_det, passes, warmup):
    from dhts import ops
    d = ops.macro_desc(L, N, DT, DX, UM)
    g = torch.Generator(device="cpu").manual_seed(1234)
    f32 = dict(dtype=torch.float32, device=dev)
    r = (0.2 + 0.4 * torch.rand(L, N, generator=g)).to(dev)
    u = (5.0 + 10.0 * torch.rand(L, N, generator=g)).to(dev)
    gr, gu = (0.2 + 0.4 * torch.rand(L, 2, generator=g)).to(dev), (5.0 + 10.0 * torch.rand(L, 2, generator=g)).to(dev)
    y, q = ops.macro_state_from_ru(r, u, UM)
    gy, gq = ops.macro_state_from_ru(gr, gu, UM)
    ghost = torch.stack([gr, gy, gu, gq], dim=-1).contiguous()
    ramps = torch.tensor([(2 * k + 1) * N // (2 * RAMPS) for k in range(RAMPS)], dtype=torch.int32, device=dev)
    inflow = ((torch.rand(T, L, RAMPS, generator=g) - 0.2) * (0.05 / (DT * T))).to(dev)      # adds at most 0.04 to a cell, a fifth negative
    det = torch.tensor([(2 * k + 1) * N // (2 * n_det) + 1 for k in range(n_det)], dtype=torch.int32, device=dev) if n_det else None
    S = ops.macro_ckpt_plan(d, T, n_det)["segment"]
    ckpt = torch.empty(ops.macro_ckpt_numel(d, T, S), **f32)
    out = tuple(torch.empty(L, N, **f32) for _ in range(4))
    gout = (torch.empty(L, N, **f32), torch.empty(L, N, **f32))
    g_r, g_y = torch.randn(L, N, **f32), torch.randn(L, N, **f32)
    taps = torch.empty(T, L, 3, n_det, **f32) if n_det else None
    g_taps = torch.randn(T, L, 2, n_det, **f32) if n_det else None
    g_ghost = torch.empty(L, 2, 2, dtype=torch.float64, device=dev)
    g_inflow = torch.empty(T, L, RAMPS, **f32)

    def step(form):
        if form == "a":
            ops.macro_rollout_fwd_ckpt(d, T, r, y, u, q, ghost, ckpt, segment=S, det=det, out=out, taps=taps)
            ops.macro_rollout_bwd_ckpt(d, T, ckpt, r, y, u, q, ghost, g_r, g_y, segment=S, det=det, g_taps=g_taps, out=gout)
        else:
            ops.macro_rollout_fwd_ckpt_ramp(d, T, r, y, u, q, ghost, ckpt, ramps, inflow, segment=S, det=det, out=out, taps=taps)
            ops.macro_rollout_bwd_ckpt_ramp(d, T, ckpt, r, y, u, q, ghost, g_r, g_y, ramps, inflow, segment=S, det=det, g_taps=g_taps,
                                            out=gout, g_ghost=g_ghost, g_inflow=g_inflow)

    forms = ["a", "b"]
    times = {form: [] for form in forms}
    for p in range(warmup + passes):
        for form in forms[p % 2:] + forms[:p % 2]:
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step(form)
            z.record()
            z.synchronize()
            if p >= warmup:
                times[form].append(a.elapsed_time(z))
    rec = dict(shape=[L, N, T], detectors=n_det, ramps=RAMPS, segment=S, passes=passes)
    for form in forms:
        v = times[form]
        rec[form] = dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))
    rec["b_over_a"] = round(rec["b"]["median_ms"] / rec["a"]["median_ms"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x512x1000,4096x64x1000", help="comma-separated LxNxT")
    ap.add_argument("--passes", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_macro_ramp.py needs a GPU")
    dev = torch.device("cuda:0")
    for shape in args.shapes.split(","):
        L, N, T = (int(x) for x in shape.split("x"))
        for n_det in (0, 4):
            print(json.dumps(measure(dev, L, N, T, n_det, args.passes, args.warmup)), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
