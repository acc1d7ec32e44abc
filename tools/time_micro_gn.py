#!/usr/bin/env python3
"""Time the Jacobian part of one Levenberg-Marquardt iteration of the dense trajectory fit of the IDM rollout -- the loss, J^T J and J^T r
of K = 5 parameter directions (unit direction i of the shared driver expanded over every vehicle, t_params) -- in its two fused forms,
and measure what each allocates, on one GPU.

    a  the histories in memory: dhts.micro_rollout_jvp(fused=True, want_hist=True) returns hist and five directions of t_hist; the
       residual, its float64 copy, the float64 copy of the Jacobian and the two products are torch's (examples/calibrate_idm.py
       --method lm --fused)
    b  the normal equations inside the kernel: dhts.micro_rollout_jvp(fused=True, target=observed) returns sse, J^T r and J^T J per
       lane, summed over the lanes here (--fused-loss); observed is read once per launch, nothing else of size T x V exists.  K = 5
       under a launch width of 4 is three launches (the pair-of-blocks scheme), each of which recomputes the primal.
A small shape and BASELINE config 3's (4096 lanes x 256 vehicles x 1000 steps, bench.py's seeded inputs) by default.  observed is a
rollout of the same lanes with every parameter 5 % off, so the residuals are those of a fit under way.  Device events around each form,
warm-up passes first, the two forms ALTERNATING inside every timed pass and every pass starting with the other one; the median and the
spread of the passes are reported.  Before the passes each form is run once on its own: bytes = the peak of
torch.cuda.max_memory_allocated above the resident inputs (observed among them: it is the data).  A form a that does not fit the card
at the shape is said so and timed at the largest number of lanes (halved until it fits) that does, beside form b at the full shape and
at that one.  Prints one JSON line per shape; needs a GPU (there is no CPU path).

    python tools/time_micro_gn.py [--shapes 64x256x400,4096x256x1000 --passes 6 --warmup 2 --budget 300]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diff-hybrid-traffic-sim_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

K = 5


def a_bytes(L, V, T):
    """What form a holds at its peak, at least: hist and K directions of t_hist in float32, the float64 Jacobian and residual."""
    dense = T * L * 2 * V * 4
    return (1 + K) * dense + 2 * (1 + K) * dense


def measure(dev, L, V, T, passes, warmup, forms, budget=300.0):
    import dhts
    from bench import MicroWorkload
    from dhts import ops
    w = MicroWorkload(dev, 0, L, V, T)
    dt = w.desc.dt
    dense_bytes = T * L * 2 * V * 4
    with torch.no_grad():
        observed = dhts.micro_rollout(w.p0, w.v0, w.params * 1.05, w.head, T, dt, want_hist=True, checkpoint=True, check_faults=False)[2]
    observed = observed.contiguous()
    unit = torch.zeros(K, 6, L, V, dtype=torch.float64, device=dev)
    for i in range(K):
        unit[i, i] = 1.0

    def step(form):
        if form == "a":
            (_, _, hist), (_, _, t_hist) = dhts.micro_rollout_jvp(w.p0, w.v0, w.params, w.head, T, dt, t_params=unit, want_hist=True, fused=True,
                                                                  check_faults=False)
            res = (hist - observed).reshape(-1).double()
            jac = t_hist.reshape(K, -1).double()
            return (res ** 2).sum(), jac @ jac.T, jac @ res
        (_, _, sse), (_, _, jtr, jtj) = dhts.micro_rollout_jvp(w.p0, w.v0, w.params, w.head, T, dt, t_params=unit, fused=True, target=observed,
                                                                check_faults=False)
        return sse.sum(), jtj.sum(0), jtr.sum(0)

    rec = dict(shape=[L, V, T], K=K, passes=passes, dense_history_bytes=dense_bytes, plan=ops.micro_fwd_jvp_gn_plan(w.desc, T, K, True))
    bytes_of, out, solo = {}, {}, 0.0
    for form in forms:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        resident = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        out[form] = step(form)
        torch.cuda.synchronize()
        solo += time.perf_counter() - t0
        bytes_of[form] = torch.cuda.max_memory_allocated() - resident
    # form a's float64 products take about a minute per pass at the large shape: fewer passes there, and the record says so
    while passes > 2 and solo * (warmup + passes) > budget:
        passes -= 2
    if solo * (warmup + passes) > budget:
        warmup = min(warmup, 1)
    rec.update(passes=passes, warmup=warmup)
    if len(forms) == 2:          # the two forms sum the same exact terms: equal to the summation order
        rec["rel_diff"] = dict(zip(("loss", "jtj", "jtr"), (float((x - y).abs().max() / x.abs().max().clamp_min(1e-300))
                                                            for x, y in zip(out["a"], out["b"]))))
    del out
    times = {form: [] for form in forms}
    for p in range(warmup + passes):
        for form in forms[p % len(forms):] + forms[:p % len(forms)]:
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step(form)
            z.record()
            z.synchronize()
            if p >= warmup:
                times[form].append(a.elapsed_time(z))
    for form in forms:
        v = times[form]
        rec[form] = dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), bytes=bytes_of[form])
    if len(forms) == 2:
        rec["b_over_a"] = round(rec["b"]["median_ms"] / rec["a"]["median_ms"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x256x400,4096x256x1000", help="comma-separated LxVxT")
    ap.add_argument("--passes", type=int, default=6, help="an even number gives each form each place equally often")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--budget", type=float, default=300.0, help="seconds a shape's passes may take: fewer passes (2 at the least) beyond it")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_micro_gn.py needs a GPU")
    dev = torch.device("cuda:0")
    for shape in args.shapes.split(","):
        L, V, T = (int(x) for x in shape.split("x"))
        free = torch.cuda.mem_get_info()[0]
        room = free - T * L * 2 * V * 4 - K * 6 * L * V * 8 - (2 << 30)          # beside observed, the directions and some slack
        if a_bytes(L, V, T) <= room:
            try:
                print(json.dumps(measure(dev, L, V, T, args.passes, args.warmup, ["a", "b"], args.budget)), flush=True)
                continue
            except torch.cuda.OutOfMemoryError:              # (the estimate leaves torch's own temporaries out)
                torch.cuda.empty_cache()
        note = "a: its histories and their float64 copies (%d bytes) do not fit the card (%d bytes free) at %d lanes" % (a_bytes(L, V, T), free, L)
        rec = measure(dev, L, V, T, args.passes, args.warmup, ["b"], args.budget)
        rec["left_out"] = note
        print(json.dumps(rec), flush=True)
        La = L
        while La > 1 and a_bytes(La, V, T) > room + (L - La) * T * 2 * V * 4:
            La //= 2
        rec = measure(dev, La, V, T, args.passes, args.warmup, ["a", "b"], args.budget)
        rec["note"] = "the largest number of lanes (halving from %d) at which form a fits" % L
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
