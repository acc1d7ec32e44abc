#!/usr/bin/env python3
"""Record tests/golden/torch_sqrt_f32.npz: the float32 square roots of the torch build the reference's fixtures were generated with,
wherever they differ from the correctly rounded one, over every argument the oracle's glue evaluates on the fixtures of
tests/test_oracle_golden.py::test_glue_square_root_as_torch_computes_it.  torch's CPU float32 sqrt is not correctly rounded on that
build (one ulp low for ~0.6 % of the arguments), and how it rounds depends on the host's CPU; the stored exceptions let the test hand the
oracle that environment's square root on any host.  Run it only where the probe below shows the generating environment's rounding
and the test passes with the live torch.sqrt.  CPU only.
    python tools/gen_sqrt_golden.py
"""
import json
import os
import platform
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "diff-hybrid-traffic-sim_amd"), os.path.join(ROOT, "tests")]
from test_oracle_golden import GLUE_SQRT_ITSCP, GLUE_SQRT_ROLLOUTS, itscp_hybrid_tables      # noqa: E402
from dhts.network import group_routes      # noqa: E402
from oracle import oracle as O      # noqa: E402
from util import meta_of      # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
O.build()
_buf = torch.zeros((), dtype=torch.float32)
seen = {}


def torch_sqrt(x):
    _buf.fill_(x)
    s = torch.sqrt(_buf).item()
    seen[x] = s
    return s


probe = torch.full((), 0.16979104280471802, dtype=torch.float32)
assert float(torch.sqrt(probe)) == float(np.float32(0.41205707)), "this torch build rounds sqrt(0.16979104f) correctly: not the environment"
try:
    O.set_sqrtf_hook(torch_sqrt)
    O.set_numpy_mean(1)
    for name in GLUE_SQRT_ITSCP:
        g = np.load(os.path.join(GOLDEN, "itscp_%s.npz" % name))
        t, m = itscp_hybrid_tables(g)
        rows = g["spawn_routes"] if g["spawn_routes"].shape[0] else -np.ones((1, 2), np.int32)
        routes, route_ptr = group_routes(rows, t.n_lanes)
        o = O.net_hybrid(t, routes, route_ptr, g["action"], m["num_intersection"] ** 2, m["simulation_frequency"] * m["signal_length"],
                         1.0 / m["simulation_frequency"], m["speed_limit"], m["static_speed"], m["vehicle_length"])
        assert o["rc"] == 0
    O.set_numpy_mean(0)
    for name in GLUE_SQRT_ROLLOUTS:
        g = np.load(os.path.join(GOLDEN, "macro_rollout_%s.npz" % name))
        m = meta_of(g)
        assert O.macro_rollout_fwd(g["r0"], g["u0"], g["ghost_r"], g["ghost_u"], m["T"], m["dt"], m["dx"], m["u_max"])["rc"] == 0
finally:
    O.set_sqrtf_hook(None)
    O.set_numpy_mean(0)
x = np.array(sorted(seen), dtype=np.float32)
s = np.array([seen[float(v)] for v in x], dtype=np.float32)
ieee = np.sqrt(x)                            # numpy's float32 sqrt: correctly rounded
bad = s != ieee
meta = dict(torch=torch.__version__, numpy=np.__version__, machine=platform.machine(), arguments=int(x.size), exceptions=int(bad.sum()),
            generator="tools/gen_sqrt_golden.py", what="x: float32 arguments where torch.sqrt of a 0-dim float32 tensor differs from the "
            "correctly rounded square root; sqrt: torch's result")
np.savez_compressed(os.path.join(GOLDEN, "torch_sqrt_f32.npz"), x=x[bad], sqrt=s[bad], meta=np.array(json.dumps(meta)))
print(json.dumps(meta))
