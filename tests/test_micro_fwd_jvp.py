"""The tape-free fused rollout + tangent kernel of the IDM rollout (dhts_micro_rollout_fwd_jvp / dhts_micro_fwd_jvp_plan,
ops.micro_rollout_fwd_jvp, dhts.micro_rollout_jvp(fused=True)): the boundary of the library -- header, bindings, exports, argument
checks, the plan, the operator's ValueErrors.  What it computes is held against the taped path bit for bit in
tests/test_micro_fwd_jvp_gpu.py.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dhts_micro_rollout_fwd_jvp", "dhts_micro_fwd_jvp_plan")
POINTERS = ("p", "v", "count", "params", "head", "t_p", "t_v", "t_head", "t_params", "p_out", "v_out", "t_p_out", "t_v_out", "hist",
            "t_hist", "err", "err_jvp")
REQUIRED = ("p", "v", "params", "head", "t_p", "t_v", "p_out", "v_out", "t_p_out", "t_v_out")


def test_header_library_and_bindings_hold_the_new_entry_points():
    import dhts
    from dhts import _lib, ops
    raw = open(os.path.join(ROOT, "include", "dhts.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib.lib()
    for name in NEW:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, txt)
        assert m, "include/dhts.h does not declare %s" % name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
        assert len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name          # the header's argument count
    assert len(_lib.SIGNATURES[NEW[0]][1]) == 21 and len(_lib.SIGNATURES[NEW[1]][1]) == 5
    comment = raw[raw.index("The rollout AND n_dir = K tangent directions of it in one kernel"):raw.index("int " + NEW[0])]
    for cited in ("_micro_lane.py:131-214", "_idm.py:30-49", "dmicro_lane.py:87-127"):      # what the pair it replaces cites
        assert cited in comment
    for name in ("micro_rollout_fwd_jvp", "micro_fwd_jvp_plan"):
        assert callable(getattr(ops, name))
    import inspect
    assert inspect.signature(dhts.micro_rollout_jvp).parameters["fused"].default is False, "the default stays the taped path"


def fused_args(some, **kw):
    a = dict(n_dir=3, stream=None, **{n: some for n in POINTERS})
    a.update(kw)
    return [a["n_dir"]] + [a[n] for n in POINTERS] + [a["stream"]]


def test_bad_arguments_are_rejected_without_a_gpu():
    from dhts import _lib
    lib = _lib.lib()
    ok = _lib.MicroDesc(4, 70, 0.01)
    some = C.c_void_p(64)                      # a non-NULL pointer that is never dereferenced: the checks come first
    run, plan = lib.dhts_micro_rollout_fwd_jvp, lib.dhts_micro_fwd_jvp_plan
    out = (C.c_int32 * 8)()
    for T in (0, 3):
        for n_dir in (0, -2):
            assert run(C.byref(ok), T, *fused_args(some, n_dir=n_dir)) == _lib.E_INVALID
        for missing in REQUIRED:
            assert run(C.byref(ok), T, *fused_args(some, **{missing: None})) == _lib.E_INVALID
            assert run(C.byref(ok), T, *fused_args(some, t_params=None, t_head=None, count=None, **{missing: None})) == _lib.E_INVALID
    assert run(C.byref(ok), -1, *fused_args(some)) == _lib.E_INVALID
    for bad in (_lib.MicroDesc(4, 5000, 0.01), _lib.MicroDesc(4, 0, 0.01), _lib.MicroDesc(0, 70, 0.01), _lib.MicroDesc(4, 70, 0.0)):
        assert run(C.byref(bad), 3, *fused_args(some)) == _lib.E_INVALID
        assert plan(C.byref(bad), 3, 1, 0, C.byref(out)) == _lib.E_INVALID
    assert run(None, 3, *fused_args(some)) == _lib.E_INVALID
    assert plan(None, 3, 1, 0, C.byref(out)) == _lib.E_INVALID
    assert plan(C.byref(ok), 3, 1, 0, None) == _lib.E_INVALID
    assert plan(C.byref(ok), 3, 0, 0, C.byref(out)) == _lib.E_INVALID
    assert plan(C.byref(ok), -1, 1, 0, C.byref(out)) == _lib.E_INVALID


def test_the_plan_needs_no_device():
    """One vehicle per thread: the block is the lane rounded up to 64.  The launch widths (4, 2, 1, never more than the plan's widest)
    are taken off the plan itself by asking it for the remainder until nothing is left: they cover n_dir in the number of launches the
    plan names, a remainder of 3 in ONE launch of 4.  LDS = two copies of the state hand-over and two per direction of the tangents'
    (8 B a slot, V + 1 slots), 16 B of head-gap tangents per direction; within the 160 KB of a workgroup."""
    from dhts import ops
    for V, block in ((1, 64), (64, 64), (65, 128), (1024, 1024)):
        for want_params in (False, True):
            for T in (0, 5):
                desc = ops.micro_desc(3, V, 0.01)
                cap = ops.micro_fwd_jvp_plan(desc, T, 9, want_params)["dirs_per_launch"]
                assert cap in (1, 2, 4)
                for K in range(1, 10):
                    p = ops.micro_fwd_jvp_plan(desc, T, K, want_params)
                    assert set(p) == {"block", "dirs_per_launch", "launches", "lds_bytes"}
                    assert p["block"] == block == (V + 63) // 64 * 64
                    assert p["dirs_per_launch"] in (1, 2, 4) and p["dirs_per_launch"] <= cap
                    assert p["lds_bytes"] == 8 * (2 + 2 * p["dirs_per_launch"]) * (V + 1) + 16 * p["dirs_per_launch"]
                    assert p["lds_bytes"] <= 160 * 1024
                    widths, rem = [], K
                    while rem > 0:
                        w = ops.micro_fwd_jvp_plan(desc, T, rem, want_params)["dirs_per_launch"]
                        assert w <= widths[-1] if widths else w == p["dirs_per_launch"]
                        widths.append(w)
                        rem -= min(w, rem)
                    assert len(widths) == p["launches"] and sum(widths) >= K, (V, K, want_params, widths, p)
                    assert sum(widths) - K == (1 if widths[-1] == 4 and K % 4 == 3 else 0), "only a remainder of 3 rides masked"
                assert ops.micro_fwd_jvp_plan(desc, T, 3, want_params)["launches"] == (1 if cap == 4 else 2)


def test_value_errors_of_the_operator_are_unchanged_with_fused():
    import torch
    import dhts
    L, V, T, K = 2, 8, 5, 3
    p0, v0 = torch.zeros(L, V), torch.zeros(L, V)
    par, head = torch.ones(6, L, V, dtype=torch.float64), torch.zeros(L, 2, dtype=torch.float64)
    tp = torch.zeros(K, L, V)

    def run(*a, **kw):
        return dhts.micro_rollout_jvp(*a, fused=True, **kw)

    bad = [
        dict(),                                                       # no tangent at all
        dict(t_p0=torch.zeros(L, V)),                                 # no direction axis
        dict(t_p0=torch.zeros(0, L, V)),                              # K = 0
        dict(t_p0=tp, t_v0=torch.zeros(K + 1, L, V)),                 # two values of K
        dict(t_v0=torch.zeros(K, L, V + 1)),
        dict(t_p0=torch.zeros(K, L + 1, V)),
        dict(t_p0=tp, t_head=torch.zeros(K, L, 3, dtype=torch.float64)),
        dict(t_head=torch.zeros(K, L, dtype=torch.float64)),
        dict(t_p0=tp, t_head=torch.zeros(K + 1, L, 2, dtype=torch.float64)),
        dict(t_params=torch.zeros(K, 5, L, V, dtype=torch.float64)),
        dict(t_params=torch.zeros(K, 6, L, V + 1, dtype=torch.float64)),
        dict(t_p0=tp, t_params=torch.zeros(6, L, V, dtype=torch.float64)),
        dict(t_p0=[[0.0]]),                                           # not a tensor
        dict(t_p0=tp, count=torch.zeros(L + 1, dtype=torch.int32)),
        dict(t_p0=tp, count=torch.zeros(L, dtype=torch.int64)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            run(p0, v0, par, head, T, 0.01, **kw)
    with pytest.raises(ValueError):
        run(p0, torch.zeros(L, V + 1), par, head, T, 0.01, t_p0=tp)
    with pytest.raises(ValueError):
        run(p0, v0, par[:5], head, T, 0.01, t_p0=tp)
    with pytest.raises(ValueError):
        run(p0, v0, par, torch.zeros(L, 3, dtype=torch.float64), T, 0.01, t_p0=tp)
    with pytest.raises(ValueError):
        run(p0, v0, par, head, -1, 0.01, t_p0=tp)
    with pytest.raises(ValueError):
        run(torch.zeros(V), torch.zeros(V), par, head, T, 0.01, t_p0=tp)
    with pytest.raises(TypeError):
        run(p0, v0, par, head, T, 0.01, tp)                           # tangents are keyword-only
