#!/usr/bin/env python3
"""Time the checkpointed reverse mode of the IDM rollout (dhts_micro_rollout_fwd_ckpt + _bwd_ckpt) against the taped pair on one GPU.

BASELINE config 3's shape by default (4096 lanes x 256 vehicles x 1000 steps, bench.py's seeded inputs).  Device events around each
call, warm-up passes first, the variants ALTERNATING inside every timed pass -- taped forward, taped reverse sweep, then for every
segment length S the checkpointed forward and reverse sweep, all of it state-only and again with the parameter gradient -- so that a
drift of the box reaches all of them alike; the median and the spread of the passes are reported, each checkpointed pair as a ratio to the
taped pair of its kind, with the plan of the launch and the [T]-sized bytes each path allocates.  A segment longer than the reverse
kernel's LDS holds (max_segment, shorter with the parameter gradient) is left out and named.  Prints one JSON line; needs a GPU (there is
no CPU path).

    python tools/time_micro_ckpt.py [--lanes 4096 --vehicles 256 --steps 1000 --segments 2 4 8 16 32 --passes 15 --warmup 3]
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
    ap.add_argument("--lanes", type=int, default=4096)
    ap.add_argument("--vehicles", type=int, default=256)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--segments", type=int, nargs="+", default=[2, 4, 8, 16, 32], help="max_segment is always added")
    ap.add_argument("--passes", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_micro_ckpt.py needs a GPU")
    from bench import MicroWorkload
    from dhts import ops
    dev = torch.device("cuda:0")
    L, V, T = args.lanes, args.vehicles, args.steps
    w = MicroWorkload(dev, 0, L, V, T)
    desc, tape, err = w.desc, w.tape, w.err
    ptape = torch.zeros(ops.micro_param_tape_numel(desc, T), dtype=torch.float32, device=dev)
    pT, vT = ops.micro_rollout_fwd(desc, T, w.p0, w.v0, w.params, w.head, tape=tape, err=err, out=w.out, ptape=ptape)
    assert err.tolist()[0] == 0, err.tolist()
    g_p, g_v = 2e-4 * pT, 2.0 * vT
    g_params = torch.empty(6, L, V, dtype=torch.float64, device=dev)
    out_c = (torch.empty_like(w.p0), torch.empty_like(w.v0))
    gout_c = (torch.empty_like(w.p0), torch.empty_like(w.v0))

    segs, left_out, ckpt = {}, {}, {}
    for with_q in (False, True):
        own = ops.micro_ckpt_plan(desc, T, with_q)
        top = own["max_segment"]
        want = sorted(set(args.segments + [top, own["segment"]]))
        segs[with_q] = [s for s in want if s <= top]
        left_out[with_q] = [s for s in want if s > top]
        for s in segs[with_q]:
            if s not in ckpt:
                ckpt[s] = torch.empty(ops.micro_ckpt_numel(desc, T, s), dtype=torch.float32, device=dev)

    def run(kind, with_q, s):
        if kind == "fwd":
            ops.micro_rollout_fwd(desc, T, w.p0, w.v0, w.params, w.head, tape=tape, err=err, out=w.out, ptape=ptape if with_q else None)
        elif kind == "bwd":
            kw = dict(ptape=ptape, params=w.params, g_params=g_params) if with_q else {}
            ops.micro_rollout_bwd(desc, T, tape, g_p, g_v, err=err, out=w.gout, g_head=w.g_head, **kw)
        elif kind == "fwd_ckpt":
            ops.micro_rollout_fwd_ckpt(desc, T, w.p0, w.v0, w.params, w.head, ckpt[s], segment=s, err=err, out=out_c)
        else:
            ops.micro_rollout_bwd_ckpt(desc, T, ckpt[s], w.params, w.head, g_p, g_v, segment=s, err=err, out=gout_c, g_head=w.g_head,
                                       g_params=g_params if with_q else None)

    kinds = []
    for with_q in (False, True):
        kinds += [("fwd", with_q, 0), ("bwd", with_q, 0)]
        for s in segs[with_q]:
            kinds += [("fwd_ckpt", with_q, s), ("bwd_ckpt", with_q, s)]
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
    assert torch.equal(out_c[0], w.out[0]) and torch.equal(out_c[1], w.out[1]) and torch.equal(gout_c[0], w.gout[0])

    def stat(v):
        return dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))

    rec = dict(shape=[L, V, T], passes=args.passes, tape_bytes=tape.numel() * 4, param_tape_bytes=ptape.numel() * 4)
    for with_q in (False, True):
        name = "params" if with_q else "state"
        fwd, bwd = stat(times[("fwd", with_q, 0)]), stat(times[("bwd", with_q, 0)])
        taped_bytes = tape.numel() * 4 + (ptape.numel() * 4 if with_q else 0)
        r = dict(taped=dict(fwd=fwd, bwd=bwd, pair_ms=round(fwd["median_ms"] + bwd["median_ms"], 4), t_sized_bytes=taped_bytes),
                 plan_segment=ops.micro_ckpt_plan(desc, T, with_q)["segment"], segments_beyond_max_segment=left_out[with_q], ckpt={})
        for s in segs[with_q]:
            f, b = stat(times[("fwd_ckpt", with_q, s)]), stat(times[("bwd_ckpt", with_q, s)])
            pair = f["median_ms"] + b["median_ms"]
            r["ckpt"]["S%d" % s] = dict(fwd=f, bwd=b, pair_ms=round(pair, 4), over_taped=round(pair / r["taped"]["pair_ms"], 3),
                                        fwd_over_taped=round(f["median_ms"] / fwd["median_ms"], 3),
                                        bwd_over_taped=round(b["median_ms"] / bwd["median_ms"], 3),
                                        t_sized_bytes=ckpt[s].numel() * 4, plan=ops.micro_ckpt_plan(desc, T, with_q, s))
        rec[name] = r
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
