#!/usr/bin/env python3
"""What detector taps cost beside the plain macro rollout, and what they save against the state history, at BASELINE config 2's shape
(1024 lanes x 512 cells x 1000 steps, 8 detectors spread over the lane): ops.macro_rollout_fwd / _fwd_taps / _fwd(hist) and
_bwd / _bwd_taps / _bwd(g_hist), and the schedule pair beside them, in ONE process, alternated, timed with HIP events.

    python tools/probes/macro_taps_path.py [--lanes 1024 --cells 512 --steps 1000 --detectors 8 --rounds 7] > profiles/macro_taps_path.log
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "diff-hybrid-traffic-sim_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dhts import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=1024)
    ap.add_argument("--cells", type=int, default=512)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--detectors", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    L, N, T, D = a.lanes, a.cells, a.steps, a.detectors
    dev = torch.device("cuda", 0)
    dt, dx, um = 0.01, 5.0, 30.0
    rng = np.random.default_rng(0)
    desc = ops.macro_desc(L, N, dt, dx, um)
    r = torch.tensor(rng.uniform(0.05, 0.95, (L, N)).astype(np.float32), device=dev)
    u = torch.tensor(rng.uniform(0.0, um, (L, N)).astype(np.float32), device=dev)
    y, q = ops.macro_state_from_ru(r, u, um)
    gr = torch.tensor(rng.uniform(0.05, 0.95, (L, 2)).astype(np.float32), device=dev)
    gu = torch.tensor(rng.uniform(0.0, um, (L, 2)).astype(np.float32), device=dev)
    gy, gq = ops.macro_state_from_ru(gr, gu, um)
    ghost = torch.stack([gr, gy, gu, gq], dim=-1).contiguous()
    sched = ghost[None].repeat(T, 1, 1, 1).contiguous()
    det = torch.tensor(np.linspace(0, N - 1, D).round().astype(np.int32), device=dev)
    tape = torch.empty(ops.macro_tape_numel(desc, T), dtype=torch.float32, device=dev)
    hist = torch.empty(T, L, 3, N, dtype=torch.float32, device=dev)
    taps = torch.empty(T, L, 3, D, dtype=torch.float32, device=dev)
    out = tuple(torch.empty_like(r) for _ in range(4))
    g_r = torch.tensor(rng.standard_normal((L, N)).astype(np.float32), device=dev)
    g_y = torch.tensor(rng.standard_normal((L, N)).astype(np.float32), device=dev)
    g_taps = torch.tensor(rng.standard_normal((T, L, 2, D)).astype(np.float32), device=dev)
    g_hist = torch.zeros(T, L, 2, N, dtype=torch.float32, device=dev)
    g_hist[:, :, :, det.long()] = g_taps
    g_out = (torch.empty_like(r), torch.empty_like(r))
    err = ops.new_error_record(dev)
    runs = {
        "fwd plain": lambda: ops.macro_rollout_fwd(desc, T, r, y, u, q, ghost, tape=tape, err=err, out=out),
        "fwd taps": lambda: ops.macro_rollout_fwd_taps(desc, T, r, y, u, q, ghost, det, tape=tape, err=err, out=out, taps=taps),
        "fwd hist": lambda: ops.macro_rollout_fwd(desc, T, r, y, u, q, ghost, tape=tape, hist=hist, err=err, out=out),
        "fwd sched": lambda: ops.macro_rollout_fwd_sched(desc, T, r, y, u, q, sched, tape=tape, err=err, out=out),
        "fwd sched taps": lambda: ops.macro_rollout_fwd_taps(desc, T, r, y, u, q, sched, det, tape=tape, err=err, out=out, taps=taps),
        "bwd plain": lambda: ops.macro_rollout_bwd(desc, T, tape, g_r, g_y, err=err, out=g_out),
        "bwd taps": lambda: ops.macro_rollout_bwd_taps(desc, T, tape, g_r, g_y, det, g_taps, err=err, out=g_out),
        "bwd hist": lambda: ops.macro_rollout_bwd(desc, T, tape, g_r, g_y, g_hist=g_hist, err=err, out=g_out),
        "bwd sched": lambda: ops.macro_rollout_bwd_sched(desc, T, tape, g_r, g_y, err=err, out=g_out),
        "bwd sched taps": lambda: ops.macro_rollout_bwd_taps(desc, T, tape, g_r, g_y, det, g_taps, sched=True, err=err, out=g_out),
    }
    print("shape %d x %d x %d, %d detectors at %s" % (L, N, T, D, det.tolist()))
    print("plan plain %s\nplan taps  %s\nplan hist  %s" % (ops.macro_rollout_plan(desc, T), ops.macro_taps_plan(desc, T, D),
                                                        ops.macro_rollout_plan(desc, T, want_hist=True)))
    times = {k: [] for k in runs}
    for rnd in range(a.rounds + 1):                      # round 0 warms up
        for k, f in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            if rnd:
                times[k].append(e0.elapsed_time(e1))
    assert err.tolist()[0] == 0, err.tolist()
    for k, v in times.items():
        print("%-15s ms: median %.3f  min %.3f  max %.3f  (%s)" % (k, float(np.median(v)), min(v), max(v), " ".join("%.3f" % x for x in v)))
    med = {k: float(np.median(v)) for k, v in times.items()}
    for d in ("fwd", "bwd"):
        print("%s: taps / plain = %.3f, taps / hist = %.3f, sched taps / sched = %.3f" % (
            d, med[d + " taps"] / med[d + " plain"], med[d + " taps"] / med[d + " hist"], med[d + " sched taps"] / med[d + " sched"]))


if __name__ == "__main__":
    main()
