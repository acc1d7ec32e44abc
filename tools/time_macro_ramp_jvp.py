#!/usr/bin/env python3
"""Time the fused forward + tangent kernel of the ARZ rollout with on-ramps against the same kernel without them -- through the raw
wrapper on buffers made once, a constant boundary, on one GPU:

    a  ops.macro_rollout_fwd_jvp                                  the kRamp = false kernel, which every call without ramps launches
    b  ops.macro_rollout_fwd_jvp(ramps=, inflow=, t_inflow=)      the same build's kRamp = true sibling with 4 ramps spread over the lane
    c  ops.macro_rollout_fwd_jvp(ramps=, inflow=)                 (--split) the source without its tangent: t_inflow NULL, one load per
                                                                  ramp cell and step instead of 1 + K

1024 lanes x 512 cells x 1000 steps and 4096 x 64 x 1000, each with K = 1 and K = 4 directions, plain and with 4 detectors (readings
and tangent readings out).  Device events around one call, warm-up passes first, the forms ALTERNATING inside every timed pass and every
pass starting with another one; the median and the spread of the passes and the ratios of the medians are reported.  Prints one JSON
line per shape, K and form; needs a GPU (there is no CPU path).

    python tools/time_macro_ramp_jvp.py [--shapes 1024x512x1000,4096x64x1000 --dirs 1,4 --passes 15 --warmup 3 --split]
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


def measure(dev, L, N, T, K, n_det, passes, warmup, split):
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
    t_inflow = torch.randn(K, T, L, RAMPS, **f32)
    det = torch.tensor([(2 * k + 1) * N // (2 * n_det) + 1 for k in range(n_det)], dtype=torch.int32, device=dev) if n_det else None
    t_r, t_y = torch.randn(K, L, N, **f32), torch.randn(K, L, N, **f32)
    out = tuple(torch.empty(L, N, **f32) for _ in range(4)) + (torch.empty(K, L, N, **f32), torch.empty(K, L, N, **f32))
    taps = torch.empty(T, L, 3, n_det, **f32) if n_det else None
    t_taps = torch.empty(K, T, L, 2, n_det, **f32) if n_det else None

    def step(form):
        kw = {} if form == "a" else dict(ramps=ramps, inflow=inflow, t_inflow=t_inflow if form == "b" else None)
        ops.macro_rollout_fwd_jvp(d, T, r, y, u, q, ghost, t_r, t_y, det=det, out=out, taps=taps, t_taps=t_taps, **kw)

    forms = ["a", "b"] + (["c"] if split else [])
    times = {form: [] for form in forms}
    for p in range(warmup + passes):
        k = p % len(forms)
        for form in forms[k:] + forms[:k]:
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step(form)
            z.record()
            z.synchronize()
            if p >= warmup:
                times[form].append(a.elapsed_time(z))
    plan = ops.macro_fwd_jvp_plan(d, T, K, n_det)
    rec = dict(shape=[L, N, T], directions=K, detectors=n_det, ramps=RAMPS, waves=plan["waves"], passes_per_wave=plan["passes"], passes=passes)
    for form in forms:
        v = times[form]
        rec[form] = dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))
    rec["b_over_a"] = round(rec["b"]["median_ms"] / rec["a"]["median_ms"], 4)
    if split:
        rec["c_over_a"] = round(rec["c"]["median_ms"] / rec["a"]["median_ms"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x512x1000,4096x64x1000", help="comma-separated LxNxT")
    ap.add_argument("--dirs", default="1,4", help="comma-separated numbers of directions")
    ap.add_argument("--passes", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--split", action="store_true", help="also time the source without its tangent (form c)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_macro_ramp_jvp.py needs a GPU")
    dev = torch.device("cuda:0")
    for shape in args.shapes.split(","):
        L, N, T = (int(x) for x in shape.split("x"))
        for K in (int(x) for x in args.dirs.split(",")):
            for n_det in (0, 4):
                print(json.dumps(measure(dev, L, N, T, K, n_det, args.passes, args.warmup, args.split)), flush=True)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
