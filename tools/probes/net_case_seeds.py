"""Which seed each hand-built network of tests/net_cases.py keeps, and why: for every case, attempts 0, 1, ... until one meets the
conditions tests/test_net_cases.py asserts (net_cases.conditioning_failures, nontrivial_failures); prints the attempt kept and what
each earlier one missed.  CPU only.  The output is the seed list of profiles/net_layout_cases.log; net_cases.SEEDS must agree with it.

    python tools/probes/net_case_seeds.py [case ...]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "diff-hybrid-traffic-sim_amd"), os.path.join(ROOT, "tests")]

import net_cases as nc              # noqa: E402
from oracle import oracle as O      # noqa: E402

O.build()
ok = True
for name in sys.argv[1:] or list(nc.BUILDERS):
    kept, tried = nc.try_seeds(name, O)
    print("%s: attempt %s kept (net_cases.SEEDS has %d); %d tried before it" % (name, kept, nc.SEEDS.get(name, 0), len(tried)))
    for k, bad in tried:
        print("    %d: %s" % (k, "; ".join(bad)))
    ok = ok and kept == nc.SEEDS.get(name, 0)
sys.exit(0 if ok else 1)
