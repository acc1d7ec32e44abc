"""The trajectory-fit loss inside the checkpointed micro rollout (dhts_micro_rollout_fwd_ckpt_target / _bwd_ckpt_target,
dhts_micro_ckpt_target_plan, the ops wrappers of the same names, dhts.micro_rollout(target=)): the boundary of the library -- header,
bindings, exports, argument checks, every ValueError, the plan of the target forms next to the untouched plan of their siblings, the
resource records.  What the kernels compute is held against existing device code in tests/test_micro_target_gpu.py.  No GPU needed."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD = ("p", "v", "count", "params", "head", "lead", "lead_length", "p_out", "v_out", "ckpt", "target", "sse", "err", "stream")
BWD = ("ckpt", "count", "params", "head", "lead", "lead_length", "g_p", "g_v", "target", "g_sse", "g_p_out", "g_v_out", "g_head", "g_lead",
       "g_params", "err", "stream")
NAMES = {"dhts_micro_rollout_fwd_ckpt_target": FWD, "dhts_micro_rollout_bwd_ckpt_target": BWD}
LDS_BUDGET = 160 * 1024

# dhts.ops.micro_ckpt_plan(micro_desc(3, V, 0.01), 1000, want_params) as the parent commit's build returns it, in the order
# (block, segment, max_segment, checkpoints, fwd_lds_bytes, bwd_lds_bytes, bwd_groups_per_cu): the siblings' plan does not move
PARENT_PLAN = {
    (1, False): (64, 16, 13646, 63, 32, 272, 602),
    (1, True): (64, 16, 5848, 63, 32, 528, 310),
    (2, False): (64, 16, 6822, 63, 48, 496, 330),
    (2, True): (64, 16, 3411, 63, 48, 880, 186),
    (64, False): (64, 6, 210, 167, 1040, 6704, 24),
    (64, True): (64, 6, 125, 167, 1040, 9824, 16),
    (65, False): (128, 14, 207, 72, 1056, 13048, 12),
    (65, True): (128, 14, 123, 72, 1056, 20440, 8),
    (130, False): (192, 8, 102, 125, 2096, 16688, 9),
    (130, True): (192, 8, 61, 125, 2096, 25072, 6),
    (256, False): (256, 6, 50, 167, 4112, 26672, 6),
    (256, True): (256, 6, 30, 167, 4112, 39008, 4),
    (1000, False): (1024, 6, 10, 167, 16016, 104048, 1),
    (1000, True): (1024, 6, 6, 167, 16016, 152096, 1),
    (1024, False): (1024, 6, 10, 167, 16400, 106544, 1),
    (1024, True): (1024, 6, 6, 167, 16400, 155744, 1),
}


def test_header_library_and_bindings_hold_the_new_entry_points():
    import dhts
    from dhts import _lib, ops
    raw = open(os.path.join(ROOT, "include", "dhts.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib.lib()
    for name, names in NAMES.items():
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, txt)
        assert m, "include/dhts.h does not declare %s" % name
        assert getattr(lib, name) is not None
        assert len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1 == len(names) + 3, name        # d, T, segment first
        declared = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
        assert declared[3:] == list(names), "the header's argument names of %s" % name
        assert [i for i, t in enumerate(_lib.SIGNATURES[name][1]) if t is C.c_int] == [1, 2], name
    assert re.search(r"\bdhts_micro_ckpt_target_plan\s*\(", txt) and _lib.SIGNATURES["dhts_micro_ckpt_target_plan"] == \
        _lib.SIGNATURES["dhts_micro_ckpt_plan"]
    comment = raw[raw.index("THE TRAJECTORY-FIT LOSS inside the checkpointed pair"):raw.index("int dhts_micro_ckpt_target_plan")]
    for cited in ("_micro_lane.py:131-214", "dmicro_lane.py:230-269", "dmicro_lane.py:271-298", ":130-153", "DHTS_E_INVALID",
                  "[T][L][2][V]", "[L][2] DOUBLE", "NaN", "exactly 0", "No atomics"):
        assert cited in comment, cited
    for name in ("micro_rollout_fwd_ckpt_target", "micro_rollout_bwd_ckpt_target", "micro_ckpt_target_plan", "MicroRolloutTarget"):
        assert callable(getattr(ops, name))
    assert dhts.MicroRolloutTarget is ops.MicroRolloutTarget
    par = inspect.signature(dhts.micro_rollout).parameters
    assert par["target"].default is None and list(par)[-1] == "target"
    assert list(inspect.signature(ops.MicroRollout.forward).parameters)[-1] == "checkpoint", "the existing operators keep their signatures"
    assert list(inspect.signature(ops.MicroRolloutSamples.forward).parameters)[-1] == "every"
    assert list(inspect.signature(ops.MicroRolloutLead.forward).parameters)[-1] == "observe"


def call_args(names, some, **kw):
    """Every pointer `some`, in the head form (lead, lead_length, g_lead NULL) unless told otherwise."""
    a = {n: some for n in names}
    a.update(stream=None, lead=None, lead_length=None)
    if "g_lead" in names:
        a.update(g_lead=None)
    a.update(kw)
    return [a[n] for n in names]


def test_bad_arguments_are_rejected_without_a_gpu():
    """DHTS_E_INVALID with nothing dereferenced: `some` is a pointer nobody may follow, and no device exists here to launch on."""
    from dhts import _lib
    lib = _lib.lib()
    ok = _lib.MicroDesc(4, 70, 0.01)
    some = C.c_void_p(64)
    fwd, bwd = lib.dhts_micro_rollout_fwd_ckpt_target, lib.dhts_micro_rollout_bwd_ckpt_target
    lead_f, lead_b = dict(head=None, lead=some), dict(head=None, lead=some, g_head=None, g_lead=some)
    for fn, names, required, lead in ((fwd, FWD, ("p", "v", "params", "p_out", "v_out", "target", "sse"), lead_f),
                                      (bwd, BWD, ("ckpt", "params", "g_p", "g_v", "target", "g_p_out", "g_v_out"), lead_b)):
        for form in ({}, lead):
            for missing in required:
                kw = dict(form)
                kw[missing] = None
                assert fn(C.byref(ok), 5, 1, *call_args(names, some, **kw)) == _lib.E_INVALID, (names is FWD, missing)
            for bad in (_lib.MicroDesc(4, 5000, 0.01), _lib.MicroDesc(0, 70, 0.01), _lib.MicroDesc(4, 70, 0.0)):
                assert fn(C.byref(bad), 5, 1, *call_args(names, some, **form)) == _lib.E_INVALID
            assert fn(C.byref(ok), -1, 1, *call_args(names, some, **form)) == _lib.E_INVALID
            assert fn(C.byref(ok), 5, -1, *call_args(names, some, **form)) == _lib.E_INVALID
        # head and lead: exactly one
        assert fn(C.byref(ok), 5, 1, *call_args(names, some, lead=some)) == _lib.E_INVALID
        assert fn(C.byref(ok), 5, 1, *call_args(names, some, head=None)) == _lib.E_INVALID
        assert fn(C.byref(ok), 5, 1, *call_args(names, some, lead_length=some)) == _lib.E_INVALID       # a leader's length without a leader
    # the boundary's cotangent goes with the boundary
    assert bwd(C.byref(ok), 5, 1, *call_args(BWD, some, g_lead=some)) == _lib.E_INVALID
    assert bwd(C.byref(ok), 5, 1, *call_args(BWD, some, head=None, lead=some, g_head=some, g_lead=some)) == _lib.E_INVALID
    assert bwd(C.byref(ok), 5, 1, *call_args(BWD, some, head=None, lead=some, g_head=None, g_lead=None)) == _lib.E_INVALID
    # a segment the reverse kernel's ring cannot hold -- the TARGET plan's, shorter than the siblings'
    plan, sib = (C.c_int32 * 8)(), (C.c_int32 * 8)()
    for want_params, g_params in ((0, None), (1, some)):
        assert lib.dhts_micro_ckpt_target_plan(C.byref(ok), 5, want_params, 0, C.byref(plan)) == 0
        assert lib.dhts_micro_ckpt_plan(C.byref(ok), 5, want_params, 0, C.byref(sib)) == 0
        assert plan[2] < sib[2]
        assert bwd(C.byref(ok), 5, plan[2] + 1, *call_args(BWD, some, g_params=g_params)) == _lib.E_INVALID
        assert lib.dhts_micro_ckpt_target_plan(C.byref(ok), 5, want_params, plan[2] + 1, C.byref(sib)) == _lib.E_INVALID
    assert lib.dhts_micro_ckpt_target_plan(C.byref(ok), 5, 0, 0, C.byref(plan)) == 0
    assert fwd(C.byref(ok), 5, plan[2] + 1, *call_args(FWD, some)) == _lib.E_INVALID
    assert lib.dhts_micro_ckpt_target_plan(C.byref(ok), 5, 0, 0, None) == _lib.E_INVALID


def test_every_value_error_is_raised_before_a_device_is_touched():
    """CPU tensors throughout: a call that reached a kernel wrapper would raise TypeError (not a CUDA tensor), not ValueError.  Before
    `target` existed the first call failed with TypeError: unexpected keyword argument 'target'."""
    import numpy as np
    import torch
    import dhts
    L, V, T, dt = 2, 5, 4, 0.1
    p0, v0 = torch.zeros(L, V), torch.zeros(L, V)
    params = torch.ones(6, L, V, dtype=torch.float64)
    head = torch.zeros(L, 2, dtype=torch.float64)
    lead = torch.zeros(T, L, 2)
    target = torch.zeros(T, L, 2, V)
    with pytest.raises(ValueError, match="checkpoint=True"):
        dhts.micro_rollout(p0, v0, params, head, T, dt, target=target)
    with pytest.raises(ValueError, match="checkpoint=True"):
        dhts.micro_rollout(p0, v0, params, head, T, dt, target=target, checkpoint=False)
    with pytest.raises(ValueError, match="checkpoint=True"):
        dhts.micro_rollout(p0, v0, params, None, T, dt, target=target, lead=lead)
    with pytest.raises(ValueError, match="does not take want_hist"):
        dhts.micro_rollout(p0, v0, params, head, T, dt, target=target, checkpoint=True, want_hist=True)
    with pytest.raises(ValueError, match="does not take probes / every"):
        dhts.micro_rollout(p0, v0, params, head, T, dt, target=target, checkpoint=True, probes=[0, 1])
    with pytest.raises(ValueError, match="does not take probes / every"):
        dhts.micro_rollout(p0, v0, params, head, T, dt, target=target, checkpoint=True, every=2)
    with pytest.raises(ValueError, match="does not take probes / every"):
        dhts.micro_rollout(p0, v0, params, None, T, dt, target=target, checkpoint=True, lead=lead, probes=[0], every=2)
    for bad in (torch.zeros(T + 1, L, 2, V), torch.zeros(T, L, 2, V + 1), torch.zeros(T, L, V, 2), torch.zeros(T, L, 2 * V),
                torch.zeros(T, L, 2, V, dtype=torch.float64), torch.zeros(T, L, 2, V, dtype=torch.float16),
                np.zeros((T, L, 2, V), np.float32)):
        with pytest.raises(ValueError, match="target must be a float32 tensor of shape"):
            dhts.micro_rollout(p0, v0, params, head, T, dt, target=bad, checkpoint=True)
        with pytest.raises(ValueError, match="target must be a float32 tensor of shape"):
            dhts.micro_rollout(p0, v0, params, None, T, dt, target=bad, checkpoint=2, lead=lead)
    with pytest.raises(ValueError, match="p0's device"):
        dhts.micro_rollout(p0, v0, params, head, T, dt, target=torch.zeros(T, L, 2, V, device="meta"), checkpoint=True)
    with pytest.raises(ValueError, match="must be contiguous"):
        dhts.micro_rollout(p0, v0, params, head, T, dt, target=torch.zeros(T, L, V, 2).transpose(2, 3), checkpoint=True)
    with pytest.raises(ValueError, match="must be contiguous"):
        dhts.micro_rollout(p0, v0, params, head, T, dt, target=torch.zeros(2 * T, L, 2, V)[::2], checkpoint=True)
    with pytest.raises(ValueError, match="not differentiable"):
        dhts.micro_rollout(p0, v0, params, head, T, dt, target=torch.zeros(T, L, 2, V, requires_grad=True), checkpoint=True)
    # the checkpoint argument, against the target forms' own plan
    with pytest.raises(ValueError, match="checkpoint must be"):
        dhts.micro_rollout(p0, v0, params, head, T, dt, target=target, checkpoint=-2)
    with pytest.raises(ValueError, match="max_segment of the target forms"):
        dhts.micro_rollout(p0, v0, params, head, T, dt, target=target, checkpoint=10 ** 6)
    from dhts import ops
    desc = ops.micro_desc(L, V, dt)
    between = ops.micro_ckpt_target_plan(desc, T, True)["max_segment"] + 1
    assert between <= ops.micro_ckpt_plan(desc, T, True)["max_segment"]          # the siblings would take it
    with pytest.raises(ValueError, match="max_segment of the target forms"):
        dhts.micro_rollout(p0, v0, params.clone().requires_grad_(), head, T, dt, target=target, checkpoint=between)
    with pytest.raises(ValueError, match="head must be given"):
        dhts.micro_rollout(p0, v0, params, None, T, dt, target=target, checkpoint=True)
    # the leader's checks hold next to target
    with pytest.raises(ValueError, match="head must be None"):
        dhts.micro_rollout(p0, v0, params, head, T, dt, target=target, checkpoint=True, lead=lead)
    with pytest.raises(ValueError, match="lead_length needs lead"):
        dhts.micro_rollout(p0, v0, params, head, T, dt, target=target, checkpoint=True, lead_length=torch.ones(L, dtype=torch.float64))
    with pytest.raises(ValueError, match="lead must be a float32 tensor"):
        dhts.micro_rollout(p0, v0, params, None, T, dt, target=target, checkpoint=True, lead=torch.zeros(T + 1, L, 2))
    # ... and the raw wrappers' own, which need no device either
    ck = torch.zeros(0)
    with pytest.raises(ValueError, match="exactly one of head and lead"):
        ops.micro_rollout_fwd_ckpt_target(desc, T, p0, v0, params, None, target, head=head, lead=lead)
    with pytest.raises(ValueError, match="exactly one of head and lead"):
        ops.micro_rollout_bwd_ckpt_target(desc, T, ck, params, p0, v0, target)
    with pytest.raises(ValueError, match="target must be a contiguous float32"):
        ops.micro_rollout_fwd_ckpt_target(desc, T, p0, v0, params, None, target[:, :, :, :-1], head=head)
    with pytest.raises(ValueError, match="ckpt must be"):
        ops.micro_rollout_bwd_ckpt_target(desc, T, ck, params, p0, v0, target, head=head)


def test_target_plan_for_every_lane_width():
    """dhts_micro_ckpt_target_plan for V = 1 .. 1024 and both reverse kernels: the ring of max_segment steps fits the 160 KB of a CU and
    one step more does not; 1 <= segment <= max_segment; a longer segment is rejected; the bytes are the documented function of the
    shape: the siblings' plus two floats per vehicle-step."""
    from dhts import ops
    T = 1000
    for V in range(1, 1025):
        desc = ops.micro_desc(3, V, 0.01)
        fixed = 8 * 2 * (V + 1) + 4 * 4 * (V + 2)
        for want_params in (False, True):
            step = 12 * V + 8 * V + (8 * (V + 1) if want_params else 0)
            pl = ops.micro_ckpt_target_plan(desc, T, want_params)
            S, M = pl["segment"], pl["max_segment"]
            assert pl["block"] == (V + 63) // 64 * 64 and pl["fwd_lds_bytes"] == 8 * 2 * (V + 1)
            assert 1 <= S <= M, (V, want_params, pl)
            assert pl["bwd_lds_bytes"] == fixed + S * step and pl["checkpoints"] == (T + S - 1) // S
            assert pl["bwd_groups_per_cu"] == LDS_BUDGET // pl["bwd_lds_bytes"] >= 1
            at_max = ops.micro_ckpt_target_plan(desc, T, want_params, M)
            assert at_max["segment"] == M and at_max["bwd_lds_bytes"] == fixed + M * step <= LDS_BUDGET
            assert fixed + (M + 1) * step > LDS_BUDGET
            with pytest.raises(ValueError, match="max_segment of the target forms"):
                ops.micro_ckpt_target_plan(desc, T, want_params, M + 1)
            # the default: the longest segment, up to 16, that leaves 16 wavefronts resident by LDS when sized with the parameter ring
            groups = -(-16 // (pl["block"] // 64))
            step_p = 12 * V + 8 * V + 8 * (V + 1)
            want = min(max((LDS_BUDGET // groups - fixed) // step_p, 0), 16, ops.micro_ckpt_target_plan(desc, T, True)["max_segment"])
            assert S == max(want, 1), (V, want_params, pl)
            # the checkpoint buffer of the resolved segment
            assert ops.micro_ckpt_numel(desc, T, S) == 2 * pl["checkpoints"] * 3 * pl["block"]


def test_the_siblings_plan_is_the_parents():
    from dhts import ops
    for (V, want_params), want in PARENT_PLAN.items():
        got = ops.micro_ckpt_plan(ops.micro_desc(3, V, 0.01), 1000, want_params)
        assert tuple(got.values()) == want, (V, want_params, got)


def test_resource_listing_keeps_every_existing_kernel():
    """profiles/micro_target_resources_parent.txt against profiles/micro_target_resources.txt (compiler output for gfx950, one line per
    kernel): every kernel of the parent is there with identical figures, and the new lines are the six target forms, none with scratch or
    a spill, none above the 128 VGPRs a block of 1024 threads may use."""
    def read(name):
        rows = {}
        for line in open(os.path.join(ROOT, "profiles", name)).read().splitlines():
            kernel, figures = line.split(" SGPRs ")
            rows[kernel.strip()] = "SGPRs " + " ".join(figures.split())
        return rows
    parent, new = read("micro_target_resources_parent.txt"), read("micro_target_resources.txt")
    assert len(parent) == 131
    for k, figures in parent.items():
        assert new.get(k) == figures, k
    added = sorted(set(new) - set(parent))
    assert added == ["micro_rollout_ckpt_bwd_target_kernel<false, false>", "micro_rollout_ckpt_bwd_target_kernel<false, true>",
                     "micro_rollout_ckpt_bwd_target_kernel<true, false>", "micro_rollout_ckpt_bwd_target_kernel<true, true>",
                     "micro_rollout_ckpt_fwd_target_kernel<false>", "micro_rollout_ckpt_fwd_target_kernel<true>"]
    for k in added:
        assert " scratch 0 " in new[k] and " sgpr_spill 0 vgpr_spill 0 " in new[k], (k, new[k])
        assert int(re.search(r"VGPRs\s+(\d+)", new[k]).group(1)) <= 128, (k, new[k])
