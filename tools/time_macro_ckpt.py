#!/usr/bin/env python3
"""Time the checkpointed reverse mode of the ARZ rollout (dhts_macro_rollout_fwd_ckpt + _bwd_ckpt) against the taped pair on one GPU.

BASELINE config 2's shape by default (1024 lanes x 512 cells x 1000 steps, bench.py's seeded inputs).  Device events around each
call, warm-up passes first, the variants ALTERNATING inside every timed pass -- taped forward, taped reverse sweep, then for every
segment length S the checkpointed forward and reverse sweep -- so that a drift of the box reaches all of them alike; the median and
the spread of the passes are reported, each checkpointed pair as a ratio to the taped pair of the same run, with the plan of the launch
and the [T]-sized bytes each path allocates.  A segment longer than the reverse kernel's LDS holds (max_segment) is left out and named.
--detectors D: the detector forms of both pairs (D cells spread over the first eighth of the lane, as examples/estimate_inflow.py
places them).  Prints one JSON line; needs a GPU (there is no CPU path).

    python tools/time_macro_ckpt.py [--lanes 1024 --cells 512 --steps 1000 --segments 1 2 3 4 6 8 12 16 --passes 15 --warmup 3 --detectors 4]
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
    ap.add_argument("--segments", type=int, nargs="+", default=[1, 2, 3, 4, 6, 8, 12, 16], help="max_segment and the plan's are always added")
    ap.add_argument("--passes", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--detectors", type=int, default=4, help="detector cells (0: none)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_macro_ckpt.py needs a GPU")
    from bench import MacroWorkload
    from dhts import ops
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
    out_t, out_c = (tuple(torch.empty_like(r0) for _ in range(4)) for _ in range(2))
    gout_t, gout_c = ((torch.empty_like(r0), torch.empty_like(r0)) for _ in range(2))
    taps_t, taps_c = (torch.empty(T, L, 3, D, dtype=torch.float32, device=dev) if D else None for _ in range(2))
    gen = torch.Generator(device="cpu").manual_seed(7)
    g_taps = torch.randn(T, L, 2, D, generator=gen).to(dev) if D else None

    def taped_fwd():
        if D:
            return ops.macro_rollout_fwd_taps(desc, T, r0, y0, u0, q0, ghost, det, tape=tape, err=err, out=out_t, taps=taps_t)[0]
        return ops.macro_rollout_fwd(desc, T, r0, y0, u0, q0, ghost, tape=tape, err=err, out=out_t)

    rT, yT, uT, _ = taped_fwd()
    assert err.tolist()[0] == 0, err.tolist()
    g_r, g_y = (2.0 * rT).clone(), (2e-2 * yT).clone()

    own = ops.macro_ckpt_plan(desc, T, D)
    top = own["max_segment"]
    if top < 1:
        sys.exit("lanes of %d cells do not fit the checkpointed reverse sweep" % N)
    want = sorted(set(args.segments + [top, own["segment"]]))
    segs, left_out = [s for s in want if s <= top], [s for s in want if s > top]
    ckpt = {s: torch.empty(ops.macro_ckpt_numel(desc, T, s), dtype=torch.float32, device=dev) for s in segs}
    res = {}

    def run(kind, s):
        if kind == "fwd":
            taped_fwd()
        elif kind == "bwd":
            if D:
                res["taped"] = ops.macro_rollout_bwd_taps(desc, T, tape, g_r, g_y, det, g_taps, err=err, out=gout_t)
            else:
                res["taped"] = ops.macro_rollout_bwd(desc, T, tape, g_r, g_y, err=err, out=gout_t)
        elif kind == "fwd_ckpt":
            ops.macro_rollout_fwd_ckpt(desc, T, r0, y0, u0, q0, ghost, ckpt[s], segment=s, det=det, err=err, out=out_c, taps=taps_c)
        else:
            res["ckpt"] = ops.macro_rollout_bwd_ckpt(desc, T, ckpt[s], r0, y0, u0, q0, ghost, g_r, g_y, segment=s, det=det, g_taps=g_taps,
                                                     err=err, out=gout_c)

    kinds = [("fwd", 0), ("bwd", 0)]
    for s in segs:
        kinds += [("fwd_ckpt", s), ("bwd_ckpt", s)]
    times = {k: [] for k in kinds}
    for p in range(args.warmup + args.passes):
        for kd in kinds:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(*kd)
            b.record()
            b.synchronize()
            if p >= args.warmup:
                times[kd].append(a.elapsed_time(b))
    assert err.tolist()[0] == 0, err.tolist()
    # the last checkpointed pair of the passes left the taped pair's bits behind
    same = all(torch.equal(a, b) for a, b in zip(out_c, out_t)) and all(torch.equal(a, b) for a, b in zip(res["ckpt"], res["taped"]))
    same = same and (not D or torch.equal(taps_c, taps_t))

    def stat(v):
        return dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))

    fwd, bwd = stat(times[("fwd", 0)]), stat(times[("bwd", 0)])
    rec = dict(shape=[L, N, T], detectors=D, passes=args.passes, bit_equal_to_taped=bool(same),
               taped=dict(fwd=fwd, bwd=bwd, pair_ms=round(fwd["median_ms"] + bwd["median_ms"], 4), t_sized_bytes=tape.numel() * 4,
                          plan=ops.macro_taps_plan(desc, T, D) if D else ops.macro_rollout_plan(desc, T)),
               plan_segment=own["segment"], segments_beyond_max_segment=left_out, ckpt={})
    for s in segs:
        f, b = stat(times[("fwd_ckpt", s)]), stat(times[("bwd_ckpt", s)])
        pair = f["median_ms"] + b["median_ms"]
        rec["ckpt"]["S%d" % s] = dict(fwd=f, bwd=b, pair_ms=round(pair, 4), over_taped=round(pair / rec["taped"]["pair_ms"], 3),
                                      fwd_over_taped=round(f["median_ms"] / fwd["median_ms"], 3),
                                      bwd_over_taped=round(b["median_ms"] / bwd["median_ms"], 3),
                                      t_sized_bytes=ckpt[s].numel() * 4, plan=ops.macro_ckpt_plan(desc, T, D, s))
    print(json.dumps(rec))
    assert same, "the checkpointed pair did not reproduce the taped pair's bits"


if __name__ == "__main__":
    main()
