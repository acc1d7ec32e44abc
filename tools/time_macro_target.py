#!/usr/bin/env python3
"""Time one iteration of the dense fit of the ARZ rollout -- loss = sum((hist - observed)^2) over the density and the speed plane,
forward + backward through dhts.macro_rollout with a boundary schedule as leaves beside (r0, u0) -- in its two forms, and measure what
each allocates, on one GPU.

    a  the history in memory: dhts.macro_rollout(want_hist=True), the taped path, the loss in torch in double (the tape, hist, the
       residuals and g_hist [T][L][.][N] are written and read)
    b  the loss inside the kernels: dhts.macro_rollout(checkpoint=True, target=observed), loss = sse.sum() (observed is read once per
       direction; nothing else of size T x N exists but the checkpoints)
1024 lanes x 512 cells x 1000 steps (if form a fits the device) and 64 x 512 x 400.  observed is a rollout of the same lanes from a
state 5 % off, so the residuals are those of a fit under way.  Device events around forward + backward, warm-up passes first, the two
forms ALTERNATING inside every timed pass and every pass starting with the other one; the median and the spread of the passes are
reported, and the median of the forward part (the rollout and, in form a, the loss in torch) and of the backward part beside them.
Before the passes each form is run once on its own: bytes = the peak of torch.cuda.max_memory_allocated above the resident inputs
(observed among them: it is the data).  A form a that does not fit the card is named and left out.  --kernels adds a line per shape with
the kernels alone: the raw wrappers on buffers made once, 20 launches per pair of events (nothing of the host between them), median of
7 -- the checkpointed forward plain and with target, the reverse sweep plain and with target, each at its own plan's segment.  Prints one
JSON line per shape; needs a GPU (there is no CPU path).

    python tools/time_macro_target.py [--shapes 1024x512x1000,64x512x400 --passes 10 --warmup 2 --kernels]
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


def inputs(dev, L, N, T):
    g = torch.Generator(device="cpu").manual_seed(1234)
    r0 = (0.2 + 0.4 * torch.rand(L, N, generator=g)).to(dev)
    u0 = (5.0 + 10.0 * torch.rand(L, N, generator=g)).to(dev)
    gr = (0.2 + 0.4 * torch.rand(T, L, 2, generator=g)).to(dev)
    gu = (5.0 + 10.0 * torch.rand(T, L, 2, generator=g)).to(dev)
    return r0, u0, gr, gu


def observed_field(dev, L, N, T, r0, u0, gr, gu):
    """[T][L][2][N]: density and speed of a rollout from a state 5 % off, made a part of the lanes at a time (the history of all of them
    would not fit beside form a)."""
    import dhts
    obs = torch.empty(T, L, 2, N, dtype=torch.float32, device=dev)
    step = max(1, min(L, (1 << 28) // max(T * N * 12, 1)))
    with torch.no_grad():
        for l in range(0, L, step):
            s = slice(l, l + step)
            h = dhts.macro_rollout(r0[s] * 1.05, u0[s] * 0.95, gr[:, s].contiguous(), gu[:, s].contiguous(), T, DT, DX, UM, want_hist=True)[4]
            obs[:, s, 0], obs[:, s, 1] = h[:, :, 0], h[:, :, 2]
            del h
    return obs


def measure(dev, L, N, T, passes, warmup):
    import dhts
    from dhts import ops
    desc = ops.macro_desc(L, N, DT, DX, UM)
    data = inputs(dev, L, N, T)
    observed = observed_field(dev, L, N, T, *data)
    leaves = [t.clone().requires_grad_(True) for t in data]
    plane_bytes = T * L * N * 4
    tape_bytes = ops.macro_tape_numel(desc, T) * 4

    def step(form, mid=None):
        for t in leaves:
            t.grad = None
        if form == "a":
            hist = dhts.macro_rollout(*leaves, T, DT, DX, UM, want_hist=True)[4]
            loss = ((hist[:, :, 0].double() - observed[:, :, 0].double()) ** 2).sum() + \
                ((hist[:, :, 2].double() - observed[:, :, 1].double()) ** 2).sum()
        else:
            loss = dhts.macro_rollout(*leaves, T, DT, DX, UM, checkpoint=True, target=observed)[4].sum()
        if mid is not None:
            mid.record()
        loss.backward()
        return loss

    rec = dict(shape=[L, N, T], passes=passes, plane_bytes=plane_bytes, tape_bytes=tape_bytes, left_out=[],
               segment=ops.macro_ckpt_target_plan(desc, T)["segment"])
    forms, bytes_of, loss_of, grads = [], {}, {}, {}
    for form in ("a", "b"):
        free = torch.cuda.mem_get_info()[0]
        need = tape_bytes + 14 * plane_bytes + (1 << 30)      # tape, hist (3), g_hist (3 + 2), double temporaries of two planes
        if form == "a" and need > free:
            rec["left_out"].append("a: its tape and histories (%d bytes) do not fit the card (%d bytes free)" % (need, free))
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
        rec["grads_equal"] = all(bool(torch.equal(x, y)) for x, y in zip(grads["a"], grads["b"]))
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
        rec["b_bytes_over_a"] = round(rec["b"]["bytes"] / rec["a"]["bytes"], 4)
    return rec


def kernels(dev, L, N, T):
    from dhts import ops
    d = ops.macro_desc(L, N, DT, DX, UM)
    r, u, gr, gu = inputs(dev, L, N, T)
    target = observed_field(dev, L, N, T, r, u, gr, gu)
    y, q = ops.macro_state_from_ru(r, u, UM)
    gy, gq = ops.macro_state_from_ru(gr, gu, UM)
    ghost = torch.stack([gr, gy, gu, gq], dim=-1).contiguous()
    Sa, Sb = ops.macro_ckpt_plan(d, T)["segment"], ops.macro_ckpt_target_plan(d, T)["segment"]
    f32 = dict(dtype=torch.float32, device=dev)
    cka, ckb = torch.empty(ops.macro_ckpt_numel(d, T, Sa), **f32), torch.empty(ops.macro_ckpt_numel(d, T, Sb), **f32)
    out = tuple(torch.empty(L, N, **f32) for _ in range(4))
    gout = (torch.empty(L, N, **f32), torch.empty(L, N, **f32))
    g_r, g_y = torch.randn(L, N, **f32), torch.randn(L, N, **f32)
    sse, g_sse = torch.empty(L, 2, dtype=torch.float64, device=dev), torch.ones(L, 2, dtype=torch.float64, device=dev)
    g_ghost = torch.empty(T, L, 2, 2, dtype=torch.float64, device=dev)
    runs = {
        "fwd_plain": lambda: ops.macro_rollout_fwd_ckpt(d, T, r, y, u, q, ghost, cka, segment=Sa, out=out),
        "fwd_target": lambda: ops.macro_rollout_fwd_ckpt_target(d, T, r, y, u, q, ghost, ckb, target, segment=Sb, sse=sse, out=out),
        "bwd_plain": lambda: ops.macro_rollout_bwd_ckpt(d, T, cka, r, y, u, q, ghost, g_r, g_y, segment=Sa, out=gout),
        "bwd_target": lambda: ops.macro_rollout_bwd_ckpt_target(d, T, ckb, r, y, u, q, ghost, g_r, g_y, target, g_sse=g_sse, final=out[:3],
                                                                segment=Sb, out=gout, g_ghost=g_ghost),
    }
    rec = dict(shape=[L, N, T], kernels_ms={}, segment=dict(plain=Sa, target=Sb))
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
    ap.add_argument("--shapes", default="1024x512x1000,64x512x400", help="comma-separated LxNxT")
    ap.add_argument("--passes", type=int, default=10, help="an even number gives each form each place equally often")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernels", action="store_true", help="also time the kernels alone through the raw wrappers")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_macro_target.py needs a GPU")
    dev = torch.device("cuda:0")
    for shape in args.shapes.split(","):
        L, N, T = (int(x) for x in shape.split("x"))
        print(json.dumps(measure(dev, L, N, T, args.passes, args.warmup)), flush=True)
        torch.cuda.empty_cache()
        if args.kernels:
            print(json.dumps(kernels(dev, L, N, T)), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
