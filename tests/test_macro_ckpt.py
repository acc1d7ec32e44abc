"""The checkpointed reverse mode of the ARZ rollout (dhts_macro_rollout_fwd_ckpt / _bwd_ckpt, dhts_macro_ckpt_plan / _bytes,
ops.macro_rollout_fwd_ckpt / _bwd_ckpt, dhts.macro_rollout(checkpoint=...)): the boundary of the library -- header, bindings, exports,
argument checks, the plan for every lane length, the operator's ValueErrors.  What it computes is held against the taped path bit for bit
in tests/test_macro_ckpt_gpu.py.  No GPU needed."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dhts_macro_ckpt_plan", "dhts_macro_ckpt_bytes", "dhts_macro_rollout_fwd_ckpt", "dhts_macro_rollout_bwd_ckpt")
FWD = ("r", "y", "u", "ueq", "ghost", "sched", "r_out", "y_out", "u_out", "ueq_out", "det", "n_det", "taps", "ckpt", "err", "stream")
FWD_REQUIRED = ("r", "y", "u", "ueq", "ghost", "r_out", "y_out", "u_out", "ueq_out", "ckpt")
BWD = ("ckpt", "r", "y", "u", "ueq", "ghost", "sched", "g_r", "g_y", "det", "n_det", "g_taps", "g_r_out", "g_y_out", "g_ghost", "err",
       "stream")
BWD_REQUIRED = ("ckpt", "r", "y", "u", "ueq", "ghost", "g_r", "g_y", "g_r_out", "g_y_out")
LDS_BUDGET = 160 * 1024
MAX_CELLS = 1319                     # the longest lane whose reverse LDS fits with a one-step ring


def rec_bytes(N):
    """The two-phase lane kernel's records: CellRec [N + 2] | flux double2 [N + 1] | queue int [N + 2] | counters, rounded up to 16."""
    return (48 * (N + 2) + 16 * (N + 1) + 4 * (N + 2) + 16 + 15) // 16 * 16


def fixed_bytes(N):
    """... with the parked pointers (48 B) and the six cotangent planes of N + 2 floats, padded to 16 B."""
    return 48 + rec_bytes(N) + (6 * (N + 2) + 3) // 4 * 4 * 4


def step_bytes(N):
    return 32 * (N + 1)               # (A, B) of the N + 1 interfaces: two float4


def default_segment(N):
    """the longest segment, up to 16, that leaves 12 wavefronts resident on a CU by LDS -- or, where a one-step ring already
    leaves fewer, as many workgroups as that one has."""
    W = min((N + 127) // 128, 12)
    p = -(-N // (64 * W))
    W = -(-N // (64 * p))
    groups = max(1, min(-(-12 // W), LDS_BUDGET // (fixed_bytes(N) + step_bytes(N))))
    S = (LDS_BUDGET // groups - fixed_bytes(N)) // step_bytes(N)
    top = (LDS_BUDGET - fixed_bytes(N)) // step_bytes(N)
    return min(max(min(S, 16), 1), top), W, p


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
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW] == [5, 3, 3 + len(FWD), 3 + len(BWD)]
    assert _lib.SIGNATURES[NEW[1]][0] is C.c_size_t
    comment = raw[raw.index("Reverse mode of the same rollout WITHOUT a tape in memory"):raw.index("int " + NEW[0])]
    for cited in ("_macro_lane.py:83-146", "dmacro_lane.py:96-132", ":277-309"):
        assert cited in comment, cited            # what dhts_macro_rollout_fwd / _bwd cite
    for name in ("macro_rollout_fwd_ckpt", "macro_rollout_bwd_ckpt", "macro_ckpt_plan", "macro_ckpt_numel"):
        assert callable(getattr(ops, name))
    assert inspect.signature(dhts.macro_rollout).parameters["checkpoint"].default is None, "the default stays the taped path"
    assert list(inspect.signature(dhts.macro_rollout).parameters)[-1] == "checkpoint"
    assert list(inspect.signature(ops.MacroRollout.forward).parameters)[-1] == "checkpoint"
    assert inspect.signature(ops.MacroRollout.forward).parameters["checkpoint"].default is None


def call_args(names, some, **kw):
    a = {n: some for n in names}
    a.update(stream=None, sched=0, n_det=2)
    a.update(kw)
    return [a[n] for n in names]


def test_bad_arguments_are_rejected_without_a_gpu():
    from dhts import _lib
    lib = _lib.lib()
    ok = _lib.MacroDesc(4, 70, 0.01, 5.0, 30.0)
    some = C.c_void_p(64)                      # a non-NULL pointer that is never dereferenced: the checks come first
    fwd, bwd, plan, size = (getattr(lib, n) for n in (NEW[2], NEW[3], NEW[0], NEW[1]))
    out = (C.c_int32 * 8)()
    assert plan(C.byref(ok), 3, 0, 0, C.byref(out)) == _lib.OK
    top = out[3]
    assert top >= 3
    plain = dict(det=None, taps=None, g_taps=None, err=None)
    for T in (0, 3):
        for sched in (0, 1):
            for missing in FWD_REQUIRED:
                if T == 0 and missing == "ckpt":
                    continue                   # (no checkpoint exists for T = 0: NULL is accepted, as the taped forward takes a NULL tape)
                assert fwd(C.byref(ok), T, 3, *call_args(FWD, some, sched=sched, **{missing: None})) == _lib.E_INVALID
                kw = {k: v for k, v in plain.items() if k in FWD}
                assert fwd(C.byref(ok), T, 0, *call_args(FWD, some, sched=sched, **dict(kw, **{missing: None}))) == _lib.E_INVALID
            for missing in BWD_REQUIRED:
                if T == 0 and missing == "ckpt":
                    continue
                assert bwd(C.byref(ok), T, 3, *call_args(BWD, some, sched=sched, **{missing: None})) == _lib.E_INVALID
                kw = {k: v for k, v in plain.items() if k in BWD}
                assert bwd(C.byref(ok), T, 0, *call_args(BWD, some, sched=sched, **dict(kw, **{missing: None}))) == _lib.E_INVALID
        # a schedule's gradient is per step: g_ghost is required with it
        assert bwd(C.byref(ok), T, 3, *call_args(BWD, some, sched=1, g_ghost=None)) == _lib.E_INVALID
        # det without taps resp. g_taps or the reverse; n_det outside 1 .. n_cells with det
        assert fwd(C.byref(ok), T, 3, *call_args(FWD, some, taps=None)) == _lib.E_INVALID
        assert fwd(C.byref(ok), T, 3, *call_args(FWD, some, det=None)) == _lib.E_INVALID
        assert bwd(C.byref(ok), T, 3, *call_args(BWD, some, g_taps=None)) == _lib.E_INVALID
        assert bwd(C.byref(ok), T, 3, *call_args(BWD, some, det=None)) == _lib.E_INVALID
        for n_det in (0, -1, 71):
            assert fwd(C.byref(ok), T, 3, *call_args(FWD, some, n_det=n_det)) == _lib.E_INVALID
            assert bwd(C.byref(ok), T, 3, *call_args(BWD, some, n_det=n_det)) == _lib.E_INVALID
        for n_det in (-1, 71):
            assert plan(C.byref(ok), T, n_det, 0, C.byref(out)) == _lib.E_INVALID
        # a segment outside 0 .. max_segment
        for seg in (-1, -7, top + 1, 1 << 30):
            assert fwd(C.byref(ok), T, seg, *call_args(FWD, some)) == _lib.E_INVALID
            assert bwd(C.byref(ok), T, seg, *call_args(BWD, some)) == _lib.E_INVALID
            assert size(C.byref(ok), T, seg) == 0
            assert plan(C.byref(ok), T, 0, seg, C.byref(out)) == _lib.E_INVALID
        assert plan(C.byref(ok), T, 0, top, C.byref(out)) == _lib.OK and out[2] == top
    assert fwd(C.byref(ok), -1, 3, *call_args(FWD, some)) == _lib.E_INVALID
    assert bwd(C.byref(ok), -1, 3, *call_args(BWD, some)) == _lib.E_INVALID
    assert size(C.byref(ok), -1, 3) == 0
    bad_descs = (_lib.MacroDesc(4, 5000, 0.01, 5.0, 30.0), _lib.MacroDesc(4, 0, 0.01, 5.0, 30.0), _lib.MacroDesc(0, 70, 0.01, 5.0, 30.0),
                 _lib.MacroDesc(4, 70, 0.0, 5.0, 30.0), _lib.MacroDesc(4, 70, 0.01, 0.0, 30.0), _lib.MacroDesc(4, 70, 0.01, 5.0, 0.0))
    for bad in bad_descs:
        assert fwd(C.byref(bad), 3, 1, *call_args(FWD, some)) == _lib.E_INVALID
        assert bwd(C.byref(bad), 3, 1, *call_args(BWD, some)) == _lib.E_INVALID
        assert plan(C.byref(bad), 3, 0, 1, C.byref(out)) == _lib.E_INVALID
        assert size(C.byref(bad), 3, 1) == 0
    # a lane beyond the bound: every segment is refused, the plan answers segment = 0 with max_segment = 0
    long = _lib.MacroDesc(4, MAX_CELLS + 1, 0.01, 5.0, 30.0)
    for seg in (0, 1):
        assert fwd(C.byref(long), 3, seg, *call_args(FWD, some)) == _lib.E_INVALID
        assert bwd(C.byref(long), 3, seg, *call_args(BWD, some)) == _lib.E_INVALID
        assert size(C.byref(long), 3, seg) == 0
    assert plan(C.byref(long), 3, 0, 1, C.byref(out)) == _lib.E_INVALID
    assert plan(C.byref(long), 3, 0, 0, C.byref(out)) == _lib.OK and out[3] == 0
    assert fwd(None, 3, 1, *call_args(FWD, some)) == _lib.E_INVALID
    assert bwd(None, 3, 1, *call_args(BWD, some)) == _lib.E_INVALID
    assert plan(None, 3, 0, 1, C.byref(out)) == _lib.E_INVALID
    assert plan(C.byref(ok), 3, 0, 1, None) == _lib.E_INVALID
    assert plan(C.byref(ok), -1, 0, 1, C.byref(out)) == _lib.E_INVALID
    assert size(None, 3, 1) == 0


def test_the_plan_for_every_lane_length():
    """N = 1 .. 1410: the lane mapping (two 64-cell passes per wavefront from 65 cells on, at most 12 wavefronts); the reverse kernel's LDS
    is the documented sum -- 48 B of parked pointers, the lane kernel's records, six cotangent planes of N + 2 floats, and per step of the
    segment 32 (N + 1) B of interface products -- within the 160 KB of a CU at the plan's segment, at max_segment, and no longer at
    max_segment + 1; C = ceil(T / S); the buffer is C x L x N x 8 bytes; an explicit segment comes back unchanged; the plan's own
    segment follows the documented rule; lanes beyond the bound report max_segment = 0."""
    from dhts import ops
    L = 3
    keys = {"waves", "passes", "segment", "max_segment", "checkpoints", "fwd_lds_bytes", "bwd_lds_bytes", "bwd_groups_per_cu"}
    bound = max(N for N in range(1, 1411) if fixed_bytes(N) + step_bytes(N) <= LDS_BUDGET)
    assert bound == MAX_CELLS == ops.MACRO_CKPT_MAX_CELLS
    for N in range(1, 1411):
        desc = ops.macro_desc(L, N, 0.01, 5.0, 30.0)
        fixed, per_step = fixed_bytes(N), step_bytes(N)
        for T in (0, 1, 1000) if N % 97 == 1 or N in (64, 512, 1024, bound) else (1000,):
            p = ops.macro_ckpt_plan(desc, T)
            assert set(p) == keys
            if N > bound:
                assert p["max_segment"] == 0 and p["segment"] == 0 and p["checkpoints"] == 0, (N, p)
                assert ops.macro_ckpt_numel(desc, T) == 0
                with pytest.raises(ValueError):
                    ops.macro_ckpt_plan(desc, T, 0, 1)
                continue
            S, top = p["segment"], p["max_segment"]
            want_S, W, passes = default_segment(N)
            assert (p["waves"], p["passes"]) == (W, passes) and passes in (1, 2) and 64 * W * passes >= N, (N, p)
            assert 1 <= S <= top and S == want_S, (N, p, want_S)
            assert p["fwd_lds_bytes"] == rec_bytes(N)
            assert p["bwd_lds_bytes"] == fixed + S * per_step <= LDS_BUDGET
            assert fixed + top * per_step <= LDS_BUDGET < fixed + (top + 1) * per_step
            assert p["bwd_groups_per_cu"] == LDS_BUDGET // p["bwd_lds_bytes"] >= 1
            assert p["checkpoints"] == -(-T // S)
            assert ops.macro_ckpt_numel(desc, T) * 4 == p["checkpoints"] * L * N * 8
            for seg in {1, 2, 3, S, top, max(1, top // 2)}:
                if seg > top:
                    continue
                e = ops.macro_ckpt_plan(desc, T, min(N, 4), seg)
                assert e["segment"] == seg and e["max_segment"] == top and e["checkpoints"] == -(-T // seg)
                assert e["bwd_lds_bytes"] == fixed + seg * per_step <= LDS_BUDGET
                assert ops.macro_ckpt_numel(desc, T, seg) * 4 == e["checkpoints"] * L * N * 8
            with pytest.raises(ValueError):
                ops.macro_ckpt_plan(desc, T, 0, top + 1)
            with pytest.raises(ValueError):
                ops.macro_ckpt_plan(desc, T, 0, -1)
    top = {N: ops.macro_ckpt_plan(ops.macro_desc(L, N, 0.01, 5.0, 30.0), 5)["max_segment"] for N in (64, 512, 1024)}
    assert top == {64: 75, 512: 7, 1024: 2}
    own = {N: ops.macro_ckpt_plan(ops.macro_desc(L, N, 0.01, 5.0, 30.0), 5)["segment"] for N in (64, 512, 1024)}
    assert own == {64: 3, 512: 2, 1024: 2}                                 # the fastest pairs of DESIGN 4f's tables at 64 and 512 cells
    assert ops.macro_ckpt_plan(ops.macro_desc(L, 512, 0.01, 5.0, 30.0), 5, 0, 2)["bwd_lds_bytes"] > 64 * 1024


def test_value_errors_come_before_any_device_use():
    """CPU tensors, no device in sight: a bad `checkpoint` is a ValueError (not the error a launch on them would be), whether or not
    anything requires grad, with both boundary forms and with detectors."""
    import torch
    import dhts
    from dhts import ops
    L, T = 2, 5
    for N, grads, sched, det in ((8, False, False, None), (8, True, True, [0, 7]), (1024, True, False, None)):
        r0, u0 = torch.full((L, N), 0.3, requires_grad=grads), torch.full((L, N), 10.0)
        gr = torch.full((T, L, 2) if sched else (L, 2), 0.3)
        gu = torch.full_like(gr, 10.0)
        top = ops.macro_ckpt_plan(ops.macro_desc(L, N, 0.01, 5.0, 30.0), T)["max_segment"]
        for bad in (0, -1, -5, 2.0, 2.5, "3", (3,), [2], top + 1, 1 << 40):
            with pytest.raises(ValueError):
                dhts.macro_rollout(r0, u0, gr, gu, T, 0.01, 5.0, 30.0, detectors=det, checkpoint=bad)
    r0, u0 = torch.full((L, 8), 0.3, requires_grad=True), torch.full((L, 8), 10.0)
    gr, gu = torch.full((L, 2), 0.3), torch.full((L, 2), 10.0)
    for ck in (True, 1, 3):
        with pytest.raises(ValueError, match="want_hist"):
            dhts.macro_rollout(r0, u0, gr, gu, T, 0.01, 5.0, 30.0, want_hist=True, checkpoint=ck)
    # a lane beyond the bound keeps the taped path: the message names the cells and checkpoint=None
    N = MAX_CELLS + 1
    r0, u0 = torch.full((L, N), 0.3, requires_grad=True), torch.full((L, N), 10.0)
    for ck in (True, 1):
        with pytest.raises(ValueError, match=r"%d cells.*checkpoint=None" % N):
            dhts.macro_rollout(r0, u0, gr, gu, T, 0.01, 5.0, 30.0, checkpoint=ck)
    # the raw wrappers check the buffer, the segment and the lane themselves
    N = 8
    desc = ops.macro_desc(L, N, 0.01, 5.0, 30.0)
    z, ghost = torch.zeros(L, N), torch.zeros(L, 2, 4)
    good = torch.zeros(ops.macro_ckpt_numel(desc, T, 2))
    assert good.numel() == 3 * L * N * 2
    with pytest.raises(ValueError):
        ops.macro_rollout_fwd_ckpt(desc, T, z, z, z, z, ghost, torch.zeros(3), segment=2)
    with pytest.raises(ValueError):
        ops.macro_rollout_fwd_ckpt(desc, T, z, z, z, z, ghost, good, segment=3)           # the buffer of another segment
    with pytest.raises(ValueError):
        ops.macro_rollout_fwd_ckpt(desc, T, z, z, z, z, ghost, good, segment=-2)
    with pytest.raises(ValueError):
        ops.macro_rollout_fwd_ckpt(desc, T, z, z, z, z, ghost, good.double(), segment=2)
    with pytest.raises(ValueError):
        ops.macro_rollout_bwd_ckpt(desc, T, torch.zeros(3), z, z, z, z, ghost, z, z, segment=2)
    with pytest.raises(ValueError):
        ops.macro_rollout_bwd_ckpt(desc, T, good, z, z, z, z, ghost, z, z, segment=1)
    with pytest.raises(ValueError):
        ops.macro_rollout_bwd_ckpt(desc, T, good, z, z, z, z, ghost, z, z, segment=2, det=torch.zeros(2, dtype=torch.int32))   # det without g_taps
    # ... in this order, with these texts: the detector pairing, the lane, the buffer, the state, the boundary cells; then the device
    bad_z, bad_ghost, taps = torch.zeros(L, N + 1), torch.zeros(T + 1, L, 2, 4), torch.zeros(T, L, 3, 2)
    with pytest.raises(ValueError, match="^taps without det$"):
        ops.macro_rollout_fwd_ckpt(desc, T, bad_z, z, z, z, ghost, torch.zeros(3), segment=2, taps=taps)
    for pair in (dict(det=torch.zeros(2, dtype=torch.int32)), dict(g_taps=taps)):
        with pytest.raises(ValueError, match="^det and g_taps go together$"):
            ops.macro_rollout_bwd_ckpt(desc, T, torch.zeros(3), bad_z, z, z, z, ghost, z, z, segment=2, **pair)
    for call in (lambda **kw: ops.macro_rollout_fwd_ckpt(desc, T, kw.get("r", z), z, z, kw.get("q", z), kw.get("ghost", ghost),
                                                         kw.get("ckpt", good), segment=2),
                 lambda **kw: ops.macro_rollout_bwd_ckpt(desc, T, kw.get("ckpt", good), kw.get("r", z), z, z, kw.get("q", z),
                                                         kw.get("ghost", ghost), bad_z, bad_z, segment=2)):
        with pytest.raises(ValueError, match=r"^ckpt must be a contiguous float32 \[macro_ckpt_numel\(desc, T, segment\)\]$"):
            call(ckpt=torch.zeros(3), r=bad_z)
        with pytest.raises(ValueError, match=r"^r must have shape \(2, 8\)$"):
            call(r=bad_z, q=bad_z, ghost=bad_ghost)
        with pytest.raises(ValueError, match=r"^ueq must have shape \(2, 8\)$"):
            call(q=bad_z, ghost=bad_ghost)
        with pytest.raises(ValueError, match=r"^ghost must have shape \(2, 2, 4\) or, a schedule, \(5, 2, 2, 4\)$"):
            call(ghost=bad_ghost)
        with pytest.raises(TypeError, match="^r must be a float32 CUDA tensor"):      # past these ValueErrors: the first thing that wants a device
            call()
    long = ops.macro_desc(L, MAX_CELLS + 1, 0.01, 5.0, 30.0)
    zl = torch.zeros(L, MAX_CELLS + 1)
    with pytest.raises(ValueError, match="checkpoint=None"):
        ops.macro_rollout_fwd_ckpt(long, T, zl, zl, zl, zl, ghost, torch.zeros(0))
    with pytest.raises(ValueError, match="checkpoint=None"):
        ops.macro_rollout_bwd_ckpt(long, T, torch.zeros(0), zl, zl, zl, zl, ghost, zl, zl)


def test_a_bad_descriptor_is_not_reported_as_a_bad_segment():
    """dhts_macro_ckpt_plan answers DHTS_E_INVALID for a bad descriptor and for a bad segment alike; the wrapper speaks of the segment
    only where the same arguments with the plan's own segment are accepted."""
    from dhts import _lib, ops
    good = ops.macro_desc(2, 64, 0.01, 5.0, 30.0)
    with pytest.raises(ValueError, match=r"max_segment \(75\)"):
        ops.macro_ckpt_plan(good, 5, 0, 76)
    for bad in (ops.MacroDesc(n_lanes=2, n_cells=5000, dt=0.01, dx=5.0, u_max=30.0), ops.MacroDesc(n_lanes=2, n_cells=64, dt=0.0, dx=5.0, u_max=30.0)):
        for segment in (0, 3):
            with pytest.raises(_lib.DhtsError) as e:
                ops.macro_ckpt_plan(bad, 5, 0, segment)
            assert e.value.status == _lib.E_INVALID and "segment" not in str(e.value)
    for T, n_det in ((-1, 0), (5, 65)):
        with pytest.raises(_lib.DhtsError) as e:
            ops.macro_ckpt_plan(good, T, n_det, 3)
        assert "segment" not in str(e.value)


def test_the_glue_of_a_checkpointed_backward_goes_over_t_in_parts_with_the_same_bits():
    """_glue_rows: at most 16 passes, none below 8192 elements.  _ghost_ry_to_ru in parts is _ghost_ry_to_ru at once, bit for bit (it is
    elementwise), a short last part included."""
    import torch
    from dhts import ops
    assert ops._glue_rows(20000, 2 * 4) == 1250 and ops._glue_rows(20000, 4) == 2048 and ops._glue_rows(37, 8) == 1024
    assert ops._glue_rows(1000, 4096 * 4) == 63 and ops._glue_rows(0, 8) == 1024 and ops._glue_rows(5, 1 << 20) == 1
    g = torch.Generator().manual_seed(3)
    T, L, um = 11, 3, 30.0
    gr = torch.rand(T, L, 2, generator=g)
    gr[2, 0, 0], gr[5, 1, 1] = 0.0, 3e-6
    gu = torch.rand(T, L, 2, generator=g) * um
    gq = um * (1 - gr.sqrt())
    g_ghost = torch.randn(T, L, 2, 2, generator=g, dtype=torch.float64)
    whole = ops._ghost_ry_to_ru(g_ghost, gr, gu, gq, um)
    for rows in (1, 3, 4, 11, 12):
        parts = ops._ghost_ry_to_ru(g_ghost, gr, gu, gq, um, rows=rows)
        for a, b in zip(parts, whole):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), rows
    sums = torch.randn(L, 2, 2, generator=g, dtype=torch.float64)       # the constant boundary: one row, taken at once
    for a, b in zip(ops._ghost_ry_to_ru(sums, gr[0], gu[0], gq[0], um, rows=1), ops._ghost_ry_to_ru(sums, gr[0], gu[0], gq[0], um)):
        assert torch.equal(a, b)
