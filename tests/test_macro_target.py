"""The dense-fit loss inside the checkpointed macro rollout (dhts_macro_rollout_fwd_ckpt_target / _bwd_ckpt_target,
dhts_macro_ckpt_target_plan, the ops wrappers of the same names, dhts.macro_rollout(target=)): the boundary of the library -- header,
bindings, exports, argument checks, every ValueError, the plan of the target forms next to the untouched plan of their siblings, the
resource records.  What the kernels compute is held against existing device code in tests/test_macro_target_gpu.py.  No GPU needed."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD = ("r", "y", "u", "ueq", "ghost", "ghost_is_sched", "r_out", "y_out", "u_out", "ueq_out", "ckpt", "target", "sse", "err", "stream")
BWD = ("ckpt", "r", "y", "u", "ueq", "ghost", "ghost_is_sched", "g_r", "g_y", "target", "g_sse", "r_fin", "y_fin", "u_fin", "g_r_out",
       "g_y_out", "g_ghost", "err", "stream")
NAMES = {"dhts_macro_rollout_fwd_ckpt_target": FWD, "dhts_macro_rollout_bwd_ckpt_target": BWD}
LDS_BUDGET = 160 * 1024
FIRST_THAT_DOES_NOT_FIT = 1240          # include/dhts.h; the siblings: 1320
SHAPES = (1, 2, 63, 64, 65, 130, 300, 512, 1000)
DT, DX, UM = 0.01, 5.0, 30.0

# dhts.ops.macro_ckpt_plan(macro_desc(3, N, 0.01, 5.0, 30.0), 1000) as the parent commit's build returns it, in the order (waves, passes,
# segment, max_segment, checkpoints, fwd_lds_bytes, bwd_lds_bytes, bwd_groups_per_cu): the siblings' plan does not move
PARENT_PLAN = {
    1: (1, 1, 16, 2554, 63, 208, 1360, 120),
    2: (1, 1, 16, 1702, 63, 272, 1952, 83),
    63: (1, 1, 3, 77, 334, 4432, 12192, 13),
    64: (1, 1, 3, 75, 334, 4496, 12368, 13),
    65: (1, 2, 3, 74, 334, 4560, 12560, 13),
    130: (2, 2, 3, 36, 334, 8976, 24768, 6),
    300: (3, 2, 1, 14, 1000, 20544, 37472, 4),
    512: (4, 2, 2, 7, 500, 34960, 80176, 2),
    1000: (8, 2, 2, 2, 500, 68144, 156304, 1),
}


def rec_bytes(N):
    """The lane kernel's records: CellRec [N + 2] (48 B) | flux double2 [N + 1] | queue int [N + 2] | counters, rounded up to 16 B."""
    return (48 * (N + 2) + 16 * (N + 1) + 4 * (N + 2) + 16 + 15) & ~15


def fixed_bytes(N):
    """... and the six cotangent planes of N + 2 floats (rounded to 16 B) and the 48 B of parked pointers."""
    return rec_bytes(N) + 4 * ((6 * (N + 2) + 3) & ~3) + 48


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
        ints = [1, 2, 3 + names.index("ghost_is_sched")]
        assert [i for i, t in enumerate(_lib.SIGNATURES[name][1]) if t is C.c_int] == ints, name
    m = re.search(r"\bdhts_macro_ckpt_target_plan\s*\(([^;]*)\)\s*;", txt)
    assert m and [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == ["d", "T", "segment", "plan[8]"]
    assert len(_lib.SIGNATURES["dhts_macro_ckpt_target_plan"][1]) == 4 and lib.dhts_macro_ckpt_target_plan is not None
    comment = raw[raw.index("THE DENSE-FIT LOSS inside the checkpointed pair"):raw.index("int dhts_macro_ckpt_target_plan")]
    for cited in ("_macro_lane.py:83-146", "dmacro_lane.py:96-132", "dmacro_lane.py:277-309", "DHTS_E_INVALID", "[T][L][2][N]",
                  "[L][2] DOUBLE", "NaN", "exactly 0", "No atomics", "%d cells" % FIRST_THAT_DOES_NOT_FIT):
        assert cited in comment, cited
    for name in ("macro_rollout_fwd_ckpt_target", "macro_rollout_bwd_ckpt_target", "macro_ckpt_target_plan", "MacroRolloutTarget"):
        assert callable(getattr(ops, name))
    assert dhts.MacroRolloutTarget is ops.MacroRolloutTarget
    par = inspect.signature(dhts.macro_rollout).parameters
    # (in front of `checkpoint`, which tests/test_macro_ckpt.py holds in the last place; every call in the tree names both by keyword)
    assert par["target"].default is None and list(par)[-2:] == ["target", "checkpoint"]
    fwd = list(inspect.signature(ops.MacroRollout.forward).parameters)
    assert len(fwd) == 13 and fwd[-1] == "checkpoint", "MacroRollout keeps its signature"
    assert ops.MACRO_CKPT_TARGET_MAX_CELLS == FIRST_THAT_DOES_NOT_FIT - 1


def call_args(names, some, **kw):
    a = {n: some for n in names}
    a.update(stream=None, ghost_is_sched=0)
    a.update(kw)
    return [a[n] for n in names]


def test_bad_arguments_are_rejected_without_a_gpu():
    """DHTS_E_INVALID with nothing dereferenced: `some` is a pointer nobody may follow, and no device exists here to launch on."""
    from dhts import _lib
    lib = _lib.lib()
    ok = _lib.MacroDesc(4, 70, DT, DX, UM)
    some = C.c_void_p(64)
    fwd, bwd = lib.dhts_macro_rollout_fwd_ckpt_target, lib.dhts_macro_rollout_bwd_ckpt_target
    for fn, names, required in ((fwd, FWD, ("r", "y", "u", "ueq", "ghost", "r_out", "y_out", "u_out", "ueq_out", "target", "sse")),
                                (bwd, BWD, ("ckpt", "r", "y", "u", "ueq", "ghost", "g_r", "g_y", "target", "r_fin", "y_fin", "u_fin",
                                            "g_r_out", "g_y_out"))):
        for sched in (0, 1):
            for missing in required:
                assert fn(C.byref(ok), 5, 1, *call_args(names, some, ghost_is_sched=sched, **{missing: None})) == _lib.E_INVALID, \
                    (names is FWD, missing)
            for bad in (_lib.MacroDesc(4, 5000, DT, DX, UM), _lib.MacroDesc(0, 70, DT, DX, UM), _lib.MacroDesc(4, 70, 0.0, DX, UM),
                        _lib.MacroDesc(4, FIRST_THAT_DOES_NOT_FIT, DT, DX, UM)):
                assert fn(C.byref(bad), 5, 0, *call_args(names, some, ghost_is_sched=sched)) == _lib.E_INVALID
            assert fn(C.byref(ok), -1, 1, *call_args(names, some, ghost_is_sched=sched)) == _lib.E_INVALID
            assert fn(C.byref(ok), 5, -1, *call_args(names, some, ghost_is_sched=sched)) == _lib.E_INVALID
    # the per-step boundary cotangent goes with the schedule
    assert bwd(C.byref(ok), 5, 1, *call_args(BWD, some, ghost_is_sched=1, g_ghost=None)) == _lib.E_INVALID
    # a segment the reverse kernel's ring cannot hold -- the TARGET plan's, shorter than the siblings'
    plan, sib = (C.c_int32 * 8)(), (C.c_int32 * 8)()
    assert lib.dhts_macro_ckpt_target_plan(C.byref(ok), 5, 0, C.byref(plan)) == 0
    assert lib.dhts_macro_ckpt_plan(C.byref(ok), 5, 0, 0, C.byref(sib)) == 0
    assert 1 <= plan[3] < sib[3]
    assert bwd(C.byref(ok), 5, plan[3] + 1, *call_args(BWD, some)) == _lib.E_INVALID
    # ... also without a cotangent of the sums, where the plain sweep (whose own plan would take that segment) does the work
    assert bwd(C.byref(ok), 5, plan[3] + 1, *call_args(BWD, some, g_sse=None)) == _lib.E_INVALID
    assert fwd(C.byref(ok), 5, plan[3] + 1, *call_args(FWD, some)) == _lib.E_INVALID
    assert lib.dhts_macro_ckpt_target_plan(C.byref(ok), 5, plan[3] + 1, C.byref(sib)) == _lib.E_INVALID
    assert lib.dhts_macro_ckpt_target_plan(C.byref(ok), 5, 0, None) == _lib.E_INVALID
    assert lib.dhts_macro_ckpt_target_plan(C.byref(ok), -1, 0, C.byref(plan)) == _lib.E_INVALID


def test_every_value_error_is_raised_before_a_device_is_touched():
    """CPU tensors throughout: a call that reached a kernel wrapper would raise TypeError (not a CUDA tensor), not ValueError.  Before
    `target` existed the first call failed with TypeError: unexpected keyword argument 'target'."""
    import numpy as np
    import torch
    import dhts
    from dhts import ops
    L, N, T = 2, 5, 4
    r0, u0 = torch.full((L, N), 0.3), torch.full((L, N), 10.0)
    g = torch.full((L, 2), 0.3)
    gs = torch.full((T, L, 2), 0.3)
    target = torch.zeros(T, L, 2, N)

    def call(**kw):
        ghost = kw.pop("ghost", g)
        return dhts.macro_rollout(r0, u0, ghost, ghost, T, DT, DX, UM, **kw)
    with pytest.raises(ValueError, match="checkpoint=True"):
        call(target=target)
    with pytest.raises(ValueError, match="checkpoint=True"):
        call(target=target, checkpoint=False, ghost=gs)
    with pytest.raises(ValueError, match="does not take want_hist"):
        call(target=target, checkpoint=True, want_hist=True)
    with pytest.raises(ValueError, match="does not take detectors"):
        call(target=target, checkpoint=True, detectors=[0, 1])
    for bad in (torch.zeros(T + 1, L, 2, N), torch.zeros(T, L, 2, N + 1), torch.zeros(T, L, 3, N), torch.zeros(T, L, N, 2),
                torch.zeros(T, L, 2 * N), torch.zeros(T, L, 2, N, dtype=torch.float64), torch.zeros(T, L, 2, N, dtype=torch.float16),
                np.zeros((T, L, 2, N), np.float32)):
        for ghost in (g, gs):
            with pytest.raises(ValueError, match="target must be a float32 tensor of shape"):
                call(target=bad, checkpoint=True, ghost=ghost)
    with pytest.raises(ValueError, match="r0's device"):
        call(target=torch.zeros(T, L, 2, N, device="meta"), checkpoint=True)
    with pytest.raises(ValueError, match="must be contiguous"):
        call(target=torch.zeros(T, L, N, 2).transpose(2, 3), checkpoint=True)
    with pytest.raises(ValueError, match="must be contiguous"):
        call(target=torch.zeros(2 * T, L, 2, N)[::2], checkpoint=True)
    with pytest.raises(ValueError, match="not differentiable"):
        call(target=torch.zeros(T, L, 2, N, requires_grad=True), checkpoint=True)
    # the checkpoint argument, against the target forms' own plan
    with pytest.raises(ValueError, match="checkpoint must be"):
        call(target=target, checkpoint=-2)
    with pytest.raises(ValueError, match="max_segment of the target forms"):
        call(target=target, checkpoint=10 ** 6)
    desc = ops.macro_desc(L, N, DT, DX, UM)
    between = ops.macro_ckpt_target_plan(desc, T)["max_segment"] + 1
    assert between <= ops.macro_ckpt_plan(desc, T)["max_segment"]          # the siblings would take it
    with pytest.raises(ValueError, match="max_segment of the target forms"):
        call(target=target, checkpoint=between)
    # a lane the target form's reverse LDS cannot hold, which the siblings' still does
    M = FIRST_THAT_DOES_NOT_FIT
    assert ops.macro_ckpt_plan(ops.macro_desc(1, M, DT, DX, UM), T)["max_segment"] >= 1
    with pytest.raises(ValueError, match=r"lanes of %d cells do not fit.*target plan holds up to %d cells" % (M, M - 1)):
        dhts.macro_rollout(torch.zeros(1, M), torch.zeros(1, M), torch.zeros(1, 2), torch.zeros(1, 2), T, DT, DX, UM,
                           target=torch.zeros(T, 1, 2, M), checkpoint=True)
    # ... and the raw wrappers' own, which need no device either
    ck = torch.zeros(0)
    y = torch.zeros(L, N)
    gq = torch.zeros(L, 2, 4)
    with pytest.raises(ValueError, match="target must be a contiguous float32"):
        ops.macro_rollout_fwd_ckpt_target(desc, T, r0, y, u0, y, gq, None, target[:, :, :, :-1])
    with pytest.raises(ValueError, match="target must be a contiguous float32"):
        ops.macro_rollout_fwd_ckpt_target(desc, T, r0, y, u0, y, gq, None, target.double())
    with pytest.raises(ValueError, match="ckpt must be"):
        ops.macro_rollout_bwd_ckpt_target(desc, T, ck, r0, y, u0, y, gq, y, y, target)
    with pytest.raises(ValueError, match="ckpt must be"):
        ops.macro_rollout_bwd_ckpt_target(desc, T, None, r0, y, u0, y, gq, y, y, target)
    good = torch.zeros(ops.macro_ckpt_numel(desc, T, 2))
    with pytest.raises(ValueError, match="must have shape"):
        ops.macro_rollout_fwd_ckpt_target(desc, T, r0[:, :-1], y, u0, y, gq, good, target, segment=2)
    with pytest.raises(ValueError, match="g_sse needs final"):
        ops.macro_rollout_bwd_ckpt_target(desc, T, good, r0, y, u0, y, gq, y, y, target, g_sse=torch.zeros(L, 2, dtype=torch.float64), segment=2)
    with pytest.raises(ValueError, match="g_sse must be a float64"):
        ops.macro_rollout_bwd_ckpt_target(desc, T, good, r0, y, u0, y, gq, y, y, target, g_sse=torch.zeros(L, 2), final=(y, y, y), segment=2)
    with pytest.raises(TypeError, match="CUDA"):          # past every ValueError: the first thing that wants a device
        ops.macro_rollout_fwd_ckpt_target(desc, T, r0, y, u0, y, gq, good, target, segment=2)


def rule(N):
    """The plan's rule restated (csrc/macro_kernels.hip, macro_ckpt_plan): the lane mapping, max_segment by the 160 KB budget, the default
    segment the longest up to 16 that keeps 12 wavefronts resident on a CU -- or what a one-step ring leaves --, with the target step."""
    W = min((N + 127) // 128, 12)
    p = -(-N // (64 * W))
    W = -(-N // (64 * p))
    fixed, step = fixed_bytes(N), 32 * (N + 1) + 8 * N
    mx = (LDS_BUDGET - fixed) // step if fixed + step <= LDS_BUDGET and p <= 2 else 0
    by_regs = -(-12 // W)
    at_one = LDS_BUDGET // (fixed + step)
    groups = 1 if at_one < 1 else min(by_regs, at_one)
    room = LDS_BUDGET // groups - fixed
    S = max(min(room // step if room > 0 else 0, 16), 1)
    return W, p, min(S, mx), mx, fixed, step


def test_target_plan_by_the_rule():
    """dhts_macro_ckpt_target_plan at the shapes of the GPU tests and at every lane from 1000 cells to the first that does not fit: the
    rule, the LDS within 160 KB, max_segment consistent with the step size, a longer segment rejected, the checkpoint buffer."""
    from dhts import ops
    T = 1000
    first_bad = None
    for N in SHAPES + tuple(range(1001, FIRST_THAT_DOES_NOT_FIT + 2)):
        desc = ops.macro_desc(3, N, DT, DX, UM)
        W, p, S, M, fixed, step = rule(N)
        pl = ops.macro_ckpt_target_plan(desc, T)
        sib = ops.macro_ckpt_plan(desc, T)
        assert (pl["waves"], pl["passes"], pl["fwd_lds_bytes"]) == (W, p, rec_bytes(N)) == (sib["waves"], sib["passes"], sib["fwd_lds_bytes"])
        assert pl["max_segment"] == M, (N, pl)
        if M < 1:
            first_bad = first_bad or N
            assert pl["segment"] == 0 and pl["bwd_lds_bytes"] == 0 and fixed + step > LDS_BUDGET
            with pytest.raises(ValueError):
                ops.macro_ckpt_target_plan(desc, T, 1)
            continue
        assert first_bad is None, "a lane fits behind one that does not"
        assert 1 <= pl["segment"] == S <= M <= sib["max_segment"], (N, pl)
        assert pl["bwd_lds_bytes"] == fixed + S * step <= LDS_BUDGET and pl["checkpoints"] == -(-T // S)
        assert pl["bwd_groups_per_cu"] == LDS_BUDGET // pl["bwd_lds_bytes"] >= 1
        at_max = ops.macro_ckpt_target_plan(desc, T, M)
        assert at_max["segment"] == M and at_max["bwd_lds_bytes"] == fixed + M * step <= LDS_BUDGET < fixed + (M + 1) * step
        with pytest.raises(ValueError, match="max_segment of the target forms"):
            ops.macro_ckpt_target_plan(desc, T, M + 1)
        assert ops.macro_ckpt_numel(desc, T, S) == 2 * pl["checkpoints"] * 3 * N
    assert first_bad == FIRST_THAT_DOES_NOT_FIT


def test_the_siblings_plan_is_the_parents():
    from dhts import ops
    for N, want in PARENT_PLAN.items():
        got = ops.macro_ckpt_plan(ops.macro_desc(3, N, DT, DX, UM), 1000)
        assert tuple(got.values()) == want, (N, got)
    assert ops.macro_ckpt_plan(ops.macro_desc(3, 1319, DT, DX, UM), 1000)["max_segment"] == 1
    assert ops.macro_ckpt_plan(ops.macro_desc(3, 1320, DT, DX, UM), 1000)["max_segment"] == 0
    assert ops.MACRO_CKPT_MAX_CELLS == 1319


def test_resource_listing_keeps_every_existing_kernel():
    """profiles/macro_target_resources_parent.txt against profiles/macro_target_resources.txt (compiler output for gfx950, one line per
    kernel): every kernel of the parent is there with identical figures, and the new lines are the six target forms, none with scratch or
    a spill, none above the 168 VGPRs a block of 768 threads may use."""
    def read(name):
        rows = {}
        for line in open(os.path.join(ROOT, "profiles", name)).read().splitlines():
            kernel, figures = line.split(" SGPRs ")
            rows[kernel.strip()] = "SGPRs " + " ".join(figures.split())
        return rows
    parent, new = read("macro_target_resources_parent.txt"), read("macro_target_resources.txt")
    assert len(parent) == 173
    for k, figures in parent.items():
        assert new.get(k) == figures, k
    added = sorted(set(new) - set(parent))
    assert added == ["macro_rollout_ckpt_bwd_target_kernel<false>", "macro_rollout_ckpt_bwd_target_kernel<true>",
                     "macro_rollout_ckpt_fwd_target_kernel<1, false>", "macro_rollout_ckpt_fwd_target_kernel<1, true>",
                     "macro_rollout_ckpt_fwd_target_kernel<2, false>", "macro_rollout_ckpt_fwd_target_kernel<2, true>"]
    for k in added:
        assert " scratch 0 " in new[k] and " sgpr_spill 0 vgpr_spill 0 " in new[k], (k, new[k])
        assert int(re.search(r"VGPRs\s+(\d+)", new[k]).group(1)) <= 168, (k, new[k])
