#!/usr/bin/env python3
"""Time one iteration of the dense trajectory fit of the IDM rollout -- loss = mean((hist - observed)^2), forward + backward through
dhts.micro_rollout with the parameter gradient -- in its two checkpointed forms, and measure what each allocates, on one GPU.

    a  the history in memory: dhts.micro_rollout(want_hist=True, checkpoint=True), the loss in torch (hist, hist - observed and g_hist
       [T][L][2][V] are written and read)
    b  the loss inside the kernels: dhts.micro_rollout(target=observed, checkpoint=True), loss = sse.sum() / observed.numel() (observed
       is read once per direction; nothing else of size T x V exists)
BASELINE config 3's shape by default (4096 lanes x 256 vehicles x 1000 steps, bench.py's seeded inputs) and one small shape.  observed is
a rollout of the same lanes with every parameter 5 % off, so the residuals are those of a fit under way.  Device events around forward +
backward, warm-up passes first, the two forms ALTERNATING inside every timed pass and every pass starting with the other one; the median
and the spread of the passes are reported, and the median of the forward part (the rollout and, in form a, the loss in torch) and of the
backward part beside them.  --segment S gives both forms the same segment length instead of each plan's own.  Before the passes each
form is run once on its own: bytes = the peak of torch.cuda.max_memory_allocated above the resident inputs (observed among them: it is
the data).  A form a that does not fit the card is named and left out.  --kernels adds a line per shape with the kernels alone: the raw wrappers on buffers made once, 20 launches per
pair of events (nothing of the host between them), median of 7 -- the checkpointed forward without a history, with hist and with
target, the reverse sweep with g_hist and with target.  Prints one JSON line per shape; needs a GPU (there is no CPU path).

    python tools/time_micro_target.py [--shapes 4096x256x1000,64x256x400 --passes 10 --warmup 2 --segment S --kernels]
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


def measure(dev, L, V, T, passes, warmup, segment):
    import dhts
    from bench import MicroWorkload
    from dhts import ops
    w = MicroWorkload(dev, 0, L, V, T)
    dt = w.desc.dt
    dense_bytes = T * L * 2 * V * 4
    with torch.no_grad():
        observed = dhts.micro_rollout(w.p0, w.v0, w.params * 1.05, w.head, T, dt, want_hist=True, checkpoint=True, check_faults=False)[2]
    observed = observed.contiguous()
    leaves = [w.p0.clone().requires_grad_(True), w.v0.clone().requires_grad_(True), w.params.clone().requires_grad_(True),
              w.head.clone().requires_grad_(True)]

    ck = segment or True

    def step(form, mid=None):
        for t in leaves:
            t.grad = None
        if form == "a":
            hist = dhts.micro_rollout(*leaves, T, dt, want_hist=True, checkpoint=ck, check_faults=False)[2]
            loss = ((hist - observed) ** 2).mean()
        else:
            loss = dhts.micro_rollout(*leaves, T, dt, checkpoint=ck, check_faults=False, target=observed)[2].sum() / observed.numel()
        if mid is not None:
            mid.record()
        loss.backward()
        return loss

    rec = dict(shape=[L, V, T], passes=passes, dense_history_bytes=dense_bytes, left_out=[],
               segment=dict(a=ops.micro_ckpt_plan(w.desc, T, True, segment or 0)["segment"],
                            b=ops.micro_ckpt_target_plan(w.desc, T, True, segment or 0)["segment"]))
    forms, bytes_of, loss_of, grads = [], {}, {}, {}
    for form in ("a", "b"):
        free = torch.cuda.mem_get_info()[0]
        if form == "a" and 4 * dense_bytes + (1 << 30) > free:
            rec["left_out"].append("a: its histories (%d bytes) do not fit the card (%d bytes free)" % (4 * dense_bytes, free))
            continue
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        resident = torch.cuda.memory_allocated()
        loss_of[form] = float(step(form))
        torch.cuda.synchronize()
        bytes_of[form] = torch.cuda.max_memory_allocated() - resident
        grads[form] = [t.grad.clone() for t in leaves]
        forms.append(form)
    if len(forms) == 2:          # the two forms fit the same thing: the loss to the summation order, the gradients as numbers
        rec["loss_rel_diff"] = abs(loss_of["a"] - loss_of["b"]) / abs(loss_of["a"])
        rec["grad_max_rel_diff"] = max(float((x - y).abs().max() / x.abs().max().clamp_min(1e-30)) for x, y in zip(grads["a"], grads["b"]))
    del grads
    times = {form: [] for form in forms}
    fwd = {form: [] for form in forms}
    for p in range(warmup + passes):
        for form in forms[p % len(forms):] + forms[:p % len(forms)]:
            a, m, z = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            a.record()
            step(form, m)
            z.record()
            z.synchronize()
            if p >= warmup:
                times[form].append(a.elapsed_time(z))
                fwd[form].append(a.elapsed_time(m))
    for form in forms:
        v = times[form]
        f_ms = statistics.median(fwd[form])
        rec[form] = dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), fwd_ms=round(f_ms, 4),
                         bwd_ms=round(statistics.median(v) - f_ms, 4), bytes=bytes_of[form], loss=loss_of[form])
    if len(forms) == 2:
        rec["b_over_a"] = round(rec["b"]["median_ms"] / rec["a"]["median_ms"], 3)
    assert ops.micro_bwd_fault(warn=False) is None
    return rec


def kernels(dev, L, V, T):
    from bench import MicroWorkload
    from dhts import ops
    w = MicroWorkload(dev, 0, L, V, T)
    d = w.desc
    Sa, Sb = ops.micro_ckpt_plan(d, T, True)["segment"], ops.micro_ckpt_target_plan(d, T, True)["segment"]
    f32 = dict(dtype=torch.float32, device=dev)
    hist = torch.empty(T, L, 2, V, **f32)
    cka, ckb = torch.empty(ops.micro_ckpt_numel(d, T, Sa), **f32), torch.empty(ops.micro_ckpt_numel(d, T, Sb), **f32)
    ops.micro_rollout_fwd_ckpt(d, T, w.p0, w.v0, w.params * 1.05, w.head, cka, segment=Sa, hist=hist)
    target = hist.clone()
    out, gout = (torch.empty(L, V, **f32), torch.empty(L, V, **f32)), (torch.empty(L, V, **f32), torch.empty(L, V, **f32))
    g_head, g_par = torch.zeros(L, 2, dtype=torch.float64, device=dev), torch.empty(6, L, V, dtype=torch.float64, device=dev)
    g_hist, g_p, g_v = torch.randn(T, L, 2, V, **f32), torch.randn(L, V, **f32), torch.randn(L, V, **f32)
    sse, g_sse = torch.empty(L, 2, dtype=torch.float64, device=dev), torch.ones(L, 2, dtype=torch.float64, device=dev)
    runs = {
        "fwd_plain": lambda: ops.micro_rollout_fwd_ckpt(d, T, w.p0, w.v0, w.params, w.head, cka, segment=Sa, out=out),
        "fwd_hist": lambda: ops.micro_rollout_fwd_ckpt(d, T, w.p0, w.v0, w.params, w.head, cka, segment=Sa, hist=hist, out=out),
        "fwd_target": lambda: ops.micro_rollout_fwd_ckpt_target(d, T, w.p0, w.v0, w.params, ckb, target, head=w.head, segment=Sb, sse=sse,
                                                                out=out),
        "bwd_hist": lambda: ops.micro_rollout_bwd_ckpt(d, T, cka, w.params, w.head, g_p, g_v, segment=Sa, g_hist=g_hist, out=gout,
                                                       g_head=g_head, g_params=g_par),
        "bwd_target": lambda: ops.micro_rollout_bwd_ckpt_target(d, T, ckb, w.params, g_p, g_v, target, g_sse=g_sse, head=w.head, segment=Sb,
                                                                out=gout, g_head=g_head, g_params=g_par),
    }
    rec = dict(shape=[L, V, T], kernels_ms={}, segment=dict(hist=Sa, target=Sb))
    for name, fn in runs.items():
        for _ in range(3):
            fn()
        ts = []
        for _ in range(7):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(20):
                fn()
            z.record()
            z.synchronize()
            ts.append(a.elapsed_time(z) / 20)
        rec["kernels_ms"][name] = round(statistics.median(ts), 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x256x1000,64x256x400", help="comma-separated LxVxT")
    ap.add_argument("--passes", type=int, default=10, help="an even number gives each form each place equally often")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--segment", type=int, default=0, help="the segment length of both forms (0: each plan's own)")
    ap.add_argument("--kernels", action="store_true", help="also time the kernels alone through the raw wrappers")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_micro_target.py needs a GPU")
    dev = torch.device("cuda:0")
    for shape in args.shapes.split(","):
        L, V, T = (int(x) for x in shape.split("x"))
        print(json.dumps(measure(dev, L, V, T, args.passes, args.warmup, args.segment)), flush=True)
        if args.kernels:
            print(json.dumps(kernels(dev, L, V, T)), flush=True)


if __name__ == "__main__":
    main()
