#!/usr/bin/env python3
"""Time the IDM tangent sweep (dhts_micro_rollout_jvp) against the reverse sweeps of the same tape on one GPU.

BASELINE config 3's shape by default (4096 lanes x 256 vehicles x 1000 steps, bench.py's seeded inputs, the tape and the parameter tape
written by the benchmarked forward kernel).  Device events around each call, warm-up passes first, the kernels ALTERNATING inside every
timed pass (reverse sweep, reverse sweep with the parameter gradient, then the tangent sweep state-only and with t_params at K = 1, 2, 4,
5 directions, then K = 4 with t_hist) so that a drift of the box reaches all of them alike; the median and the spread of the passes are
reported, each tangent sweep as a ratio to the reverse sweep of its kind and to its K = 1.  The same passes also time the tape-free
fused kernel (dhts_micro_rollout_fwd_jvp) at the same K and what it replaces -- the forward that writes the tape (with t_params: and the
parameter tape) plus the tape sweep --, and the record names the [T]-sized bytes each path allocates.  Prints one JSON line; needs a GPU
(there is no CPU path).

    python tools/time_micro_jvp.py [--lanes 4096 --vehicles 256 --steps 1000 --dirs 1 2 4 5 --hist_dirs 4 --passes 15 --warmup 3]
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
    ap.add_argument("--dirs", type=int, nargs="+", default=[1, 2, 4, 5])
    ap.add_argument("--hist_dirs", type=int, default=4, help="directions of the run that also writes t_hist (0: none)")
    ap.add_argument("--passes", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_micro_jvp.py needs a GPU")
    from bench import MicroWorkload
    from dhts import ops
    dev = torch.device("cuda:0")
    L, V, T = args.lanes, args.vehicles, args.steps
    w = MicroWorkload(dev, 0, L, V, T)
    desc, tape, err = w.desc, w.tape, w.err
    ptape = torch.zeros(ops.micro_param_tape_numel(desc, T), dtype=torch.float32, device=dev)
    pT, vT = ops.micro_rollout_fwd(desc, T, w.p0, w.v0, w.params, w.head, tape=tape, err=err, out=w.out, ptape=ptape)
    assert err.tolist()[0] == 0, err.tolist()
    kmax = max(args.dirs + [args.hist_dirs])
    gen = torch.Generator(device="cpu").manual_seed(7)
    t_p, t_v = (torch.randn(kmax, L, V, generator=gen).to(dev) for _ in range(2))
    t_head = torch.randn(kmax, L, 2, generator=gen, dtype=torch.float64).to(dev)
    t_par = torch.randn(kmax, 6, L, V, generator=gen, dtype=torch.float64).to(dev)
    t_hist = torch.empty(args.hist_dirs, T, L, 2, V, dtype=torch.float32, device=dev) if args.hist_dirs else None
    g_p, g_v = 2e-4 * pT, 2.0 * vT
    g_params = torch.empty(6, L, V, dtype=torch.float64, device=dev)
    out_j = (torch.empty_like(t_p), torch.empty_like(t_v))
    out_f = (torch.empty_like(w.p0), torch.empty_like(w.v0))
    err_jvp = ops.new_error_record(dev)

    def run(kind, k):
        if kind == "bwd":
            ops.micro_rollout_bwd(desc, T, tape, g_p, g_v, err=err, out=w.gout, g_head=w.g_head)
        elif kind == "bwd_params":
            ops.micro_rollout_bwd(desc, T, tape, g_p, g_v, err=err, out=w.gout, g_head=w.g_head, ptape=ptape, params=w.params, g_params=g_params)
        elif kind == "fwd":
            ops.micro_rollout_fwd(desc, T, w.p0, w.v0, w.params, w.head, tape=tape, err=err, out=w.out)
        elif kind == "fwd_params":
            ops.micro_rollout_fwd(desc, T, w.p0, w.v0, w.params, w.head, tape=tape, err=err, out=w.out, ptape=ptape)
        elif kind.startswith("fused_"):
            ops.micro_rollout_fwd_jvp(desc, T, w.p0, w.v0, w.params, w.head, t_p[:k], t_v[:k], t_head=t_head[:k],
                                      t_params=t_par[:k] if kind == "fused_params" else None, err=err, err_jvp=err_jvp,
                                      out=out_f + (out_j[0][:k], out_j[1][:k], None, t_hist if kind == "fused_state_hist" else None))
        else:
            kw = dict(ptape=ptape, params=w.params, t_params=t_par[:k]) if kind == "params" else {}
            ops.micro_rollout_jvp(desc, T, tape, t_p[:k], t_v[:k], t_head=t_head[:k], err=err, out=(out_j[0][:k], out_j[1][:k]),
                                  t_hist=t_hist if kind == "state_hist" else None, **kw)

    kinds = [("bwd", 0), ("bwd_params", 0)] + [("state", k) for k in args.dirs] + [("params", k) for k in args.dirs]
    if args.hist_dirs:
        kinds.append(("state_hist", args.hist_dirs))
    n_taped = len(kinds)
    kinds += [("fwd", 0), ("fwd_params", 0)] + [("fused_state", k) for k in args.dirs] + [("fused_params", k) for k in args.dirs]
    if args.hist_dirs:
        kinds.append(("fused_state_hist", args.hist_dirs))
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
    assert err.tolist()[0] == 0 and err_jvp.tolist()[0] == 0, (err.tolist(), err_jvp.tolist())

    def stat(v):
        return dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))

    rec = dict(shape=[L, V, T], passes=args.passes, tape_bytes=tape.numel() * 4, param_tape_bytes=ptape.numel() * 4,
               bwd=stat(times[("bwd", 0)]), bwd_params=stat(times[("bwd_params", 0)]), jvp={})
    for kind, k in kinds[2:n_taped]:
        s = stat(times[(kind, k)])
        base = "bwd_params" if kind == "params" else "bwd"
        s["over_" + base] = round(s["median_ms"] / rec[base]["median_ms"], 3)
        one = times.get(("state" if kind == "state_hist" else kind, 1))
        if one:
            s["over_k1"] = round(s["median_ms"] / statistics.median(one), 3)
        s["ms_per_direction"] = round(s["median_ms"] / k, 4)
        s["plan"] = ops.micro_jvp_plan(desc, T, k, kind == "params")
        rec["jvp"]["%s_k%d" % (kind, k)] = s
    # the fused kernel against the pair it replaces, timed in the same passes
    rec["fwd_tape"], rec["fwd_tape_params"] = stat(times[("fwd", 0)]), stat(times[("fwd_params", 0)])
    rec["fused"] = {}
    hist_bytes = t_hist.numel() * 4 if t_hist is not None else 0
    for kind, k in kinds[n_taped + 2:]:
        s = stat(times[(kind, k)])
        with_q = kind == "fused_params"
        fwd = rec["fwd_tape_params" if with_q else "fwd_tape"]["median_ms"]
        sweep = rec["jvp"]["%s_k%d" % (kind[len("fused_"):], k)]["median_ms"]
        s["replaces_ms"] = round(fwd + sweep, 4)
        s["over_replaced"] = round(s["median_ms"] / (fwd + sweep), 3)
        s["ms_per_direction"] = round(s["median_ms"] / k, 4)
        s["plan"] = ops.micro_fwd_jvp_plan(desc, T, k, with_q)
        extra = hist_bytes if kind == "fused_state_hist" else 0
        s["t_sized_bytes"] = dict(fused=extra, taped=tape.numel() * 4 + (ptape.numel() * 4 if with_q else 0) + extra)
        rec["fused"]["%s_k%d" % (kind[len("fused_"):], k)] = s
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
