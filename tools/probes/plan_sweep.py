#!/usr/bin/env python3
"""What the plan entry points answer over a grid of shapes that crosses every threshold of the launchers, and what dhts_set_option
answers at the edges of every option's accepted values -- to compare two builds of the library (the host launch layer is refactored
without touching a kernel: both must answer the same everywhere).

    DHTS_LIB=<one build>/libdhts.so  python tools/probes/plan_sweep.py a.json
    DHTS_LIB=<other build>/libdhts.so python tools/probes/plan_sweep.py b.json
    python tools/probes/plan_sweep.py --compare a.json b.json

The plan entry points launch nothing.  The macro and micro sweeps and the option table need no GPU; the hybrid plans (the shapes
tests/test_hybrid_gpu.py asks about) need device tables and are swept when a GPU is there (--no-hybrid leaves them out)."""
import ctypes as C
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "diff-hybrid-traffic-sim_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

MACRO_CELLS = (1, 63, 64, 65, 127, 128, 129, 256, 512, 1000, 1024, 1025, 1026, 2048, 2500)
MACRO_LANES = (1, 255, 256, 1024, 1536, 4096)
MACRO_T = (0, 1, 1000)
MACRO_JVP_CELLS = (997, 998, 1239, 1240, 1410, 1411)
MACRO_CKPT_CELLS = (1, 2, 64, 65, 128, 1239, 1240, 1319, 1320, 2048)
MICRO_CAP = (1, 63, 64, 65, 128, 129, 256, 1023, 1024)
MICRO_LANES = (1, 4096, 4097)
MICRO_T = (0, 1, 7, 1000)
MICRO_DIRS = (1, 2, 3, 4, 5, 9)
HYBRID_NETS = ("hybrid_rv_b", "hybrid_rv_d", "hybrid_p3", "hybrid_l10", "hybrid_n2", "hybrid_p2", "hybrid", "hybrid_s2")
# every option: the values just inside and just outside what it accepts (and a few in between)
OPTION_VALUES = {
    "OPT_MACRO_FWD_WAVES": (-1, 0, 1, 8, 16, 17),
    "OPT_MICRO_FWD_WAVES": (-1, 0, 1, 2, 3, 4, 5, 8),
    "OPT_MACRO_FWD_VARIANT": (-1, 0, 1, 2, 3),
    "OPT_MACRO_FWD_GROUP": (-1, 0, 1, 2, 3, 4, 5, 8),
    "OPT_MACRO_FWD_ROTATE": (-1, 0, 1, 2),
    "OPT_MACRO_JVP_VARIANT": (-1, 0, 1, 2),
    "OPT_NETSTEP_LDS_KB": (-1, 0, 1, 48, 158, 159, 160),
    "OPT_NETSTEP_BLOCK": (-1, 0, 1, 64, 128, 255, 256, 257, 512, 768, 1024, 1025, 2048),
    "OPT_HYB_PACK": (-1, 0, 1, 2, 3),
    "OPT_REWARD_CHAIN": (-1, 0, 1, 2),
}
OPTION_DEFAULTS = {"OPT_MACRO_FWD_ROTATE": 1, "OPT_HYB_PACK": 2}


def sweep(hybrid):
    from dhts import _lib
    lib = _lib.lib()
    out = {}

    def opt(name, v):
        return lib.dhts_set_option(getattr(_lib, name), v)

    for name, values in OPTION_VALUES.items():
        for v in values:
            out["option %s=%d" % (name, v)] = opt(name, v)
        assert opt(name, OPTION_DEFAULTS.get(name, 0)) == 0
    out["option 0=0"] = lib.dhts_set_option(0, 0)
    out["option 10=0"] = lib.dhts_set_option(10, 0)

    plan = (C.c_int32 * 8)()
    for variant, waves, group in itertools.product((0, 1, 2), range(17), (0, 1, 2, 4)):
        assert opt("OPT_MACRO_FWD_VARIANT", variant) == 0 and opt("OPT_MACRO_FWD_WAVES", waves) == 0 and opt("OPT_MACRO_FWD_GROUP", group) == 0
        for N, L, T, hist in itertools.product(MACRO_CELLS, MACRO_LANES, MACRO_T, (0, 1)):
            d = _lib.MacroDesc(L, N, 0.01, 5.0, 30.0)
            rc = lib.dhts_macro_rollout_plan(C.byref(d), T, hist, C.byref(plan))
            out["macro v%d w%d g%d N%d L%d T%d h%d" % (variant, waves, group, N, L, T, hist)] = [rc] + list(plan)
        for N, L, T, n_det in itertools.product(MACRO_CELLS, MACRO_LANES, MACRO_T, (1, None)):        # (None: a detector in every cell)
            d = _lib.MacroDesc(L, N, 0.01, 5.0, 30.0)
            rc = lib.dhts_macro_taps_plan(C.byref(d), T, n_det or N, C.byref(plan))
            out["taps v%d w%d g%d N%d L%d T%d d%d" % (variant, waves, group, N, L, T, n_det or N)] = [rc] + list(plan)
    for name in ("OPT_MACRO_FWD_VARIANT", "OPT_MACRO_FWD_WAVES", "OPT_MACRO_FWD_GROUP"):
        assert opt(name, 0) == 0
    for waves in (0, 1, 2, 4):
        assert opt("OPT_MICRO_FWD_WAVES", waves) == 0
        for V, L, T, cnt in itertools.product(MICRO_CAP, MICRO_LANES, (0, 1, 1000), (0, 1)):
            d = _lib.MicroDesc(L, V, 0.01)
            rc = lib.dhts_micro_rollout_plan(C.byref(d), T, cnt, C.byref(plan))
            out["micro w%d V%d L%d T%d c%d" % (waves, V, L, T, cnt)] = [rc] + list(plan)
    assert opt("OPT_MICRO_FWD_WAVES", 0) == 0
    # the tape-free micro paths: the two segment plans (and the checkpoint bytes that follow from the first) at the edges of what a
    # ring holds, the direction grouping of the two tangent sweeps
    for V, T, want in itertools.product(MICRO_CAP, MICRO_T, (0, 1)):
        d = _lib.MicroDesc(4, V, 0.01)
        for kind, fn in (("ckpt", lib.dhts_micro_ckpt_plan), ("ckpt_target", lib.dhts_micro_ckpt_target_plan)):
            assert fn(C.byref(d), T, want, 0, C.byref(plan)) == 0
            longest = plan[2]
            for segment in (0, 1, longest, longest + 1, -1):
                for k in range(8):
                    plan[k] = -7                                  # (a refused call leaves the plan as it was: seen as -7)
                rc = fn(C.byref(d), T, want, segment, C.byref(plan))
                out["%s V%d T%d q%d s%d" % (kind, V, T, want, segment)] = [rc] + list(plan)
                if kind == "ckpt" and not want:
                    out["ckpt_bytes V%d T%d s%d" % (V, T, segment)] = [int(lib.dhts_micro_ckpt_bytes(C.byref(d), T, segment))]
        for kind, fn in (("jvp", lib.dhts_micro_jvp_plan), ("fwd_jvp", lib.dhts_micro_fwd_jvp_plan)):
            for n_dir in MICRO_DIRS:
                rc = fn(C.byref(d), T, n_dir, want, C.byref(plan))
                out["%s V%d T%d q%d k%d" % (kind, V, T, want, n_dir)] = [rc] + list(plan)
    # the tape-free macro paths, the same way: the two tangent plans at the lane lengths where a launch loses directions (997 / 998,
    # 1239 / 1240, 1410 / 1411), under every forced wave count and both tangent kernels; the two segment plans and the checkpoint bytes
    # at the lengths where the passes, the target ring and the plain ring change (64 / 65, 1239 / 1240, 1319 / 1320)
    for waves, general in itertools.product(range(17), (0, 1)):
        assert opt("OPT_MACRO_FWD_WAVES", waves) == 0 and opt("OPT_MACRO_JVP_VARIANT", general) == 0
        for N, T, n_dir in itertools.product(MACRO_CELLS + MACRO_JVP_CELLS, MACRO_T, MICRO_DIRS):
            d = _lib.MacroDesc(4, N, 0.01, 5.0, 30.0)
            for kind, fn in (("macro_jvp", lib.dhts_macro_jvp_plan), ("macro_fwd_jvp", lib.dhts_macro_fwd_jvp_plan)):
                for k in range(8):
                    plan[k] = -7
                rc = fn(C.byref(d), T, n_dir, 0, C.byref(plan))
                out["%s w%d j%d N%d T%d k%d" % (kind, waves, general, N, T, n_dir)] = [rc] + list(plan)
    assert opt("OPT_MACRO_FWD_WAVES", 0) == 0 and opt("OPT_MACRO_JVP_VARIANT", 0) == 0
    for N, T in itertools.product(MACRO_CKPT_CELLS, MICRO_T):
        d = _lib.MacroDesc(4, N, 0.01, 5.0, 30.0)
        for kind, fn in (("macro_ckpt", lambda *a: lib.dhts_macro_ckpt_plan(a[0], a[1], 0, *a[2:])),
                         ("macro_ckpt_target", lib.dhts_macro_ckpt_target_plan)):
            assert fn(C.byref(d), T, 0, C.byref(plan)) == 0
            longest = plan[3]
            for segment in (0, 1, longest, longest + 1, -1):
                for k in range(8):
                    plan[k] = -7
                rc = fn(C.byref(d), T, segment, C.byref(plan))
                out["%s N%d T%d s%d" % (kind, N, T, segment)] = [rc] + list(plan)
                if kind == "macro_ckpt":
                    out["macro_ckpt_bytes N%d T%d s%d" % (N, T, segment)] = [int(lib.dhts_macro_ckpt_bytes(C.byref(d), T, segment))]
    if hybrid:
        import numpy as np
        import torch
        from dhts import ops
        from test_oracle_golden import itscp_hybrid_tables
        dev = torch.device("cuda", 0)
        for net in HYBRID_NETS:
            g = np.load(os.path.join(ROOT, "tests", "golden", "itscp_%s.npz" % net))
            t, m = itscp_hybrid_tables(g)
            sq = m["num_intersection"] ** 2
            for cap, two, pack in itertools.product((0, 16, 32, 64, 128), (-1, 0, 1), (0, 1, 2)):
                tab = ops.DeviceHybridTables(t, g["spawn_routes"], dev, lane_capacity=cap)
                tab.two_per_cu = two
                assert opt("OPT_HYB_PACK", pack) == 0
                for R in (1, 2, 3, 255, 256, 257, 512, 1024):
                    p = ops.net_hybrid_plan(R, len(g["action"]), tab, sq)
                    out["hybrid %s cap%d two%d pack%d R%d" % (net, cap, two, pack, R)] = [int(p[k]) for k in sorted(p)]
        assert opt("OPT_HYB_PACK", 2) == 0
    return out


def main(argv):
    if argv and argv[0] == "--compare":
        a, b = (json.load(open(p)) for p in argv[1:3])
        bad = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
        for k in bad[:40]:
            print("DIFFERS %s: %s | %s" % (k, a.get(k), b.get(k)))
        kinds = {}
        for k in a:
            kinds[k.split()[0]] = kinds.get(k.split()[0], 0) + 1
        print(json.dumps({"entries": len(a), "by_kind": kinds, "only_in_one": len(set(a) ^ set(b)), "different": len(bad)}))
        return 1 if bad else 0
    hybrid = "--no-hybrid" not in argv
    paths = [x for x in argv if not x.startswith("--")]
    if hybrid:
        import torch
        hybrid = torch.cuda.is_available()
    out = sweep(hybrid)
    if paths:
        with open(paths[0], "w") as f:
            json.dump(out, f, indent=0, sort_keys=True)
    print(json.dumps({"entries": len(out), "hybrid": bool(hybrid)}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
