"""The checkpointed reverse mode of the IDM rollout (dhts_micro_rollout_fwd_ckpt / _bwd_ckpt, dhts_micro_ckpt_plan / _bytes,
ops.micro_rollout_fwd_ckpt / _bwd_ckpt, dhts.micro_rollout(checkpoint=...)): the boundary of the library -- header, bindings, exports,
argument checks, the plan for every lane size, the operator's ValueErrors.  What it computes is held against the taped path bit for bit
in tests/test_micro_ckpt_gpu.py.  No GPU needed."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dhts_micro_ckpt_plan", "dhts_micro_ckpt_bytes", "dhts_micro_rollout_fwd_ckpt", "dhts_micro_rollout_bwd_ckpt")
FWD = ("p", "v", "count", "params", "head", "p_out", "v_out", "ckpt", "hist", "err", "stream")
FWD_REQUIRED = ("p", "v", "params", "head", "p_out", "v_out", "ckpt")
BWD = ("ckpt", "count", "params", "head", "g_p", "g_v", "g_hist", "g_p_out", "g_v_out", "g_head", "g_params", "err", "stream")
BWD_REQUIRED = ("ckpt", "params", "head", "g_p", "g_v", "g_p_out", "g_v_out")
LDS_BUDGET = 160 * 1024


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
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW] == [5, 3, 14, 16]
    assert _lib.SIGNATURES[NEW[1]][0] is C.c_size_t
    comment = raw[raw.index("The rollout's REVERSE mode without a tape in memory"):raw.index("int " + NEW[0])]
    for cited in ("dmicro_lane.py:230-269", "_micro_lane.py:131-214", ":87-127", "dmicro_lane.py:271-298", ":130-153", "_idm.py:30-49"):
        assert cited in comment, cited            # what dhts_micro_rollout_fwd / _bwd / _fwd_params cite
    for name in ("micro_rollout_fwd_ckpt", "micro_rollout_bwd_ckpt", "micro_ckpt_plan", "micro_ckpt_numel"):
        assert callable(getattr(ops, name))
    assert inspect.signature(dhts.micro_rollout).parameters["checkpoint"].default is None, "the default stays the taped path"
    assert list(inspect.signature(ops.MicroRollout.forward).parameters)[-1] == "checkpoint"


def call_args(names, some, **kw):
    a = {n: some for n in names}
    a["stream"] = None
    a.update(kw)
    return [a[n] for n in names]


def test_bad_arguments_are_rejected_without_a_gpu():
    from dhts import _lib
    lib = _lib.lib()
    ok = _lib.MicroDesc(4, 70, 0.01)
    some = C.c_void_p(64)                      # a non-NULL pointer that is never dereferenced: the checks come first
    fwd, bwd, plan, size = (getattr(lib, n) for n in (NEW[2], NEW[3], NEW[0], NEW[1]))
    out = (C.c_int32 * 8)()
    assert plan(C.byref(ok), 3, 0, 0, C.byref(out)) == _lib.OK
    top = {False: None, True: None}
    for wp in (False, True):
        assert plan(C.byref(ok), 3, int(wp), 0, C.byref(out)) == _lib.OK
        top[wp] = out[2]
    assert 1 <= top[True] < top[False]
    for T in (0, 3):
        for missing in FWD_REQUIRED:
            if T == 0 and missing == "ckpt":
                continue                       # (no checkpoint exists for T = 0: NULL is accepted, as the taped forward takes a NULL tape)
            assert fwd(C.byref(ok), T, 3, *call_args(FWD, some, **{missing: None})) == _lib.E_INVALID
            assert fwd(C.byref(ok), T, 0, *call_args(FWD, some, count=None, hist=None, err=None, **{missing: None})) == _lib.E_INVALID
        for missing in BWD_REQUIRED:
            if T == 0 and missing == "ckpt":
                continue
            assert bwd(C.byref(ok), T, 3, *call_args(BWD, some, **{missing: None})) == _lib.E_INVALID
            assert bwd(C.byref(ok), T, 0, *call_args(BWD, some, count=None, g_hist=None, g_params=None, **{missing: None})) == _lib.E_INVALID
        # a segment outside 0 .. max_segment: the forward and the byte count take what the state-only sweep takes, the sweep with
        # g_params the shorter one
        for seg in (-1, -7, top[False] + 1, 1 << 30):
            assert fwd(C.byref(ok), T, seg, *call_args(FWD, some)) == _lib.E_INVALID
            assert bwd(C.byref(ok), T, seg, *call_args(BWD, some)) == _lib.E_INVALID
            assert bwd(C.byref(ok), T, seg, *call_args(BWD, some, g_params=None)) == _lib.E_INVALID
            assert size(C.byref(ok), T, seg) == 0
            for wp in (0, 1):
                assert plan(C.byref(ok), T, wp, seg, C.byref(out)) == _lib.E_INVALID
        assert bwd(C.byref(ok), T, top[True] + 1, *call_args(BWD, some)) == _lib.E_INVALID
        assert plan(C.byref(ok), T, 1, top[True] + 1, C.byref(out)) == _lib.E_INVALID
        assert plan(C.byref(ok), T, 0, top[True] + 1, C.byref(out)) == _lib.OK
    assert fwd(C.byref(ok), -1, 3, *call_args(FWD, some)) == _lib.E_INVALID
    assert bwd(C.byref(ok), -1, 3, *call_args(BWD, some)) == _lib.E_INVALID
    assert size(C.byref(ok), -1, 3) == 0
    for bad in (_lib.MicroDesc(4, 5000, 0.01), _lib.MicroDesc(4, 0, 0.01), _lib.MicroDesc(0, 70, 0.01), _lib.MicroDesc(4, 70, 0.0)):
        assert fwd(C.byref(bad), 3, 1, *call_args(FWD, some)) == _lib.E_INVALID
        assert bwd(C.byref(bad), 3, 1, *call_args(BWD, some)) == _lib.E_INVALID
        assert plan(C.byref(bad), 3, 0, 1, C.byref(out)) == _lib.E_INVALID
        assert size(C.byref(bad), 3, 1) == 0
    assert fwd(None, 3, 1, *call_args(FWD, some)) == _lib.E_INVALID
    assert bwd(None, 3, 1, *call_args(BWD, some)) == _lib.E_INVALID
    assert plan(None, 3, 0, 1, C.byref(out)) == _lib.E_INVALID
    assert plan(C.byref(ok), 3, 0, 1, None) == _lib.E_INVALID
    assert plan(C.byref(ok), -1, 0, 1, C.byref(out)) == _lib.E_INVALID
    assert size(None, 3, 1) == 0


def test_the_plan_for_every_lane_size():
    """V = 1 .. 1024, with and without the parameter gradient: one vehicle per thread (the block is the lane rounded up to 64); the
    reverse kernel's LDS is the documented sum -- the state hand-over 2 x 8 (V + 1), four cotangent arrays 4 x 4 (V + 2), and per step of
    the segment 12 V of tape entries plus, with params, 8 (V + 1) of pre-step states -- within the 160 KB of a CU at the plan's segment,
    at max_segment, and no longer at max_segment + 1; C = ceil(T / S); the buffer is C x L x Vp x 8 bytes; an explicit segment comes
    back unchanged; the plan's own segment is one value for both reverse kernels (the forward does not know which will follow)."""
    from dhts import ops
    L = 3
    for V in range(1, 1025):
        desc = ops.micro_desc(L, V, 0.01)
        Vp = (V + 63) // 64 * 64
        fixed = 16 * (V + 1) + 16 * (V + 2)
        own = {}
        for wp in (False, True):
            per_step = 12 * V + (8 * (V + 1) if wp else 0)
            for T in (0, 1, 1000) if V % 97 == 1 or V in (64, 1024) else (1000,):
                p = ops.micro_ckpt_plan(desc, T, wp)
                assert set(p) == {"block", "segment", "max_segment", "checkpoints", "fwd_lds_bytes", "bwd_lds_bytes", "bwd_groups_per_cu"}
                S, top = p["segment"], p["max_segment"]
                assert p["block"] == Vp
                assert 1 <= S <= top, (V, wp, p)
                assert p["fwd_lds_bytes"] == 16 * (V + 1)
                assert p["bwd_lds_bytes"] == fixed + S * per_step <= LDS_BUDGET
                assert fixed + top * per_step <= LDS_BUDGET < fixed + (top + 1) * per_step
                assert p["bwd_groups_per_cu"] == LDS_BUDGET // p["bwd_lds_bytes"] >= 1
                assert p["checkpoints"] == -(-T // S)
                assert ops.micro_ckpt_numel(desc, T) * 4 == p["checkpoints"] * L * Vp * 8
                for seg in {1, 2, 3, S, top, max(1, top // 2)}:
                    e = ops.micro_ckpt_plan(desc, T, wp, seg)
                    assert e["segment"] == seg and e["max_segment"] == top and e["checkpoints"] == -(-T // seg)
                    assert e["bwd_lds_bytes"] == fixed + seg * per_step <= LDS_BUDGET
                    assert ops.micro_ckpt_numel(desc, T, seg) * 4 == e["checkpoints"] * L * Vp * 8
                with pytest.raises(ValueError):
                    ops.micro_ckpt_plan(desc, T, wp, top + 1)
                with pytest.raises(ValueError):
                    ops.micro_ckpt_plan(desc, T, wp, -1)
            own[wp] = S
        assert own[False] == own[True], V
    d = ops.micro_desc(L, 1024, 0.01)
    assert ops.micro_ckpt_plan(d, 5, True)["max_segment"] == 6            # (163840 - 32816) / 20488
    assert ops.micro_ckpt_plan(d, 5, True, 6)["bwd_lds_bytes"] > 64 * 1024


def test_value_errors_come_before_any_device_use():
    """CPU tensors, no device in sight: a bad `checkpoint` is a ValueError (not the RuntimeError a launch on them would be), whether or
    not anything requires grad."""
    import torch
    import dhts
    from dhts import ops
    L, V, T = 2, 8, 5
    par, head = torch.ones(6, L, V, dtype=torch.float64), torch.zeros(L, 2, dtype=torch.float64)
    for V_, grads in ((8, False), (8, True), (1024, True)):
        p0, v0 = torch.zeros(L, V_, requires_grad=grads), torch.zeros(L, V_)
        q = torch.ones(6, L, V_, dtype=torch.float64, requires_grad=grads)
        desc = ops.micro_desc(L, V_, 0.01)
        top = ops.micro_ckpt_plan(desc, T, grads)["max_segment"]
        for bad in (0, -1, -5, 2.0, 2.5, "3", (3,), [2], top + 1, 1 << 40):
            with pytest.raises(ValueError):
                dhts.micro_rollout(p0, v0, q, head, T, 0.01, checkpoint=bad)
    # the state-only sweep takes longer segments than the one with the parameter gradient
    desc = ops.micro_desc(L, 1024, 0.01)
    s_top, p_top = (ops.micro_ckpt_plan(desc, T, wp)["max_segment"] for wp in (False, True))
    assert p_top < s_top
    with pytest.raises(ValueError):
        dhts.micro_rollout(torch.zeros(L, 1024), torch.zeros(L, 1024), torch.ones(6, L, 1024, dtype=torch.float64, requires_grad=True),
                           head, T, 0.01, checkpoint=s_top)
    # the raw wrappers check the buffer and the segment themselves
    desc = ops.micro_desc(L, V, 0.01)
    z = torch.zeros(L, V)
    with pytest.raises(ValueError):
        ops.micro_rollout_fwd_ckpt(desc, T, z, z, par, head, torch.zeros(3), segment=2)
    with pytest.raises(ValueError):
        ops.micro_rollout_fwd_ckpt(desc, T, z, z, par, head, torch.zeros(ops.micro_ckpt_numel(desc, T, 2)), segment=-2)
    with pytest.raises(ValueError):
        ops.micro_rollout_bwd_ckpt(desc, T, torch.zeros(3), par, head, z, z, segment=2)
    with pytest.raises(ValueError):
        ops.micro_rollout_bwd_ckpt(desc, T, torch.zeros(ops.micro_ckpt_numel(desc, T, 2)), par, head, z, z, segment=2,
                                   g_params=torch.zeros(6, L, V))
