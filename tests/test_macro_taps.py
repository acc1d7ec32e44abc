"""Detector taps of the fused ARZ rollout (dhts_macro_rollout_fwd_taps / _bwd_taps / dhts_macro_taps_plan and dhts.macro_rollout with
`detectors`): the boundary of the library -- header, bindings, exports, argument checks -- and the operator's ValueErrors, all of which
are raised before anything touches a device.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dhts_macro_rollout_fwd_taps", "dhts_macro_rollout_bwd_taps", "dhts_macro_taps_plan")


def test_header_library_and_bindings_hold_the_new_entry_points():
    from dhts import _lib, ops
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dhts.h")).read(), flags=re.S)
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), "include/dhts.h does not declare %s" % name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    # d, T + 16 resp. 12 further arguments, as the header declares them
    assert len(_lib.SIGNATURES[NEW[0]][1]) == 18 and len(_lib.SIGNATURES[NEW[1]][1]) == 14
    assert _lib.SIGNATURES[NEW[2]][1][1:3] == [C.c_int, C.c_int]
    for name in ("macro_rollout_fwd_taps", "macro_rollout_bwd_taps", "macro_taps_plan"):
        assert callable(getattr(ops, name))


def fwd_args(some, **kw):
    """(r, y, u, ueq, ghost, ghost_is_sched, r_out, y_out, u_out, ueq_out, tape, det, n_det, taps, err, stream)"""
    a = dict(r=some, y=some, u=some, ueq=some, ghost=some, ghost_is_sched=0, r_out=some, y_out=some, u_out=some, ueq_out=some, tape=some,
             det=some, n_det=4, taps=some, err=some, stream=None)
    a.update(kw)
    return list(a.values())


def bwd_args(some, **kw):
    """(tape, g_r, g_y, det, n_det, g_taps, g_r_out, g_y_out, g_ghost, ghost_is_sched, err, stream)"""
    a = dict(tape=some, g_r=some, g_y=some, det=some, n_det=4, g_taps=some, g_r_out=some, g_y_out=some, g_ghost=some, ghost_is_sched=0,
             err=some, stream=None)
    a.update(kw)
    return list(a.values())


def test_bad_arguments_are_rejected_without_a_gpu():
    from dhts import _lib
    lib = _lib.lib()
    N = 128
    ok = _lib.MacroDesc(n_lanes=4, n_cells=N, dt=0.01, dx=5.0, u_max=30.0)
    some = C.c_void_p(64)                      # a non-NULL pointer that is never dereferenced: the checks come first
    fwd, bwd, plan = lib.dhts_macro_rollout_fwd_taps, lib.dhts_macro_rollout_bwd_taps, lib.dhts_macro_taps_plan
    out = (C.c_int32 * 8)()
    for T in (0, 3):
        for sched in (0, 1):
            assert fwd(C.byref(ok), T, *fwd_args(some, det=None, ghost_is_sched=sched)) == _lib.E_INVALID
            assert fwd(C.byref(ok), T, *fwd_args(some, taps=None, ghost_is_sched=sched)) == _lib.E_INVALID
            assert bwd(C.byref(ok), T, *bwd_args(some, det=None, ghost_is_sched=sched)) == _lib.E_INVALID
            assert bwd(C.byref(ok), T, *bwd_args(some, g_taps=None, ghost_is_sched=sched)) == _lib.E_INVALID
            for n_det in (0, -1, N + 1):
                assert fwd(C.byref(ok), T, *fwd_args(some, n_det=n_det, ghost_is_sched=sched)) == _lib.E_INVALID
                assert bwd(C.byref(ok), T, *bwd_args(some, n_det=n_det, ghost_is_sched=sched)) == _lib.E_INVALID
    for n_det in (0, -1, N + 1):
        assert plan(C.byref(ok), 3, n_det, C.byref(out)) == _lib.E_INVALID
    for missing in ("r", "ueq", "ghost", "r_out", "ueq_out"):
        assert fwd(C.byref(ok), 3, *fwd_args(some, **{missing: None})) == _lib.E_INVALID
    for missing in ("tape", "g_r", "g_r_out"):
        assert bwd(C.byref(ok), 3, *bwd_args(some, **{missing: None})) == _lib.E_INVALID
    assert bwd(C.byref(ok), 3, *bwd_args(some, g_ghost=None, ghost_is_sched=1)) == _lib.E_INVALID     # required with a schedule
    bads = (_lib.MacroDesc(n_lanes=0, n_cells=N, dt=0.01, dx=5.0, u_max=30.0),
            _lib.MacroDesc(n_lanes=4, n_cells=0, dt=0.01, dx=5.0, u_max=30.0),
            _lib.MacroDesc(n_lanes=4, n_cells=_lib.MACRO_MAX_CELLS + 1, dt=0.01, dx=5.0, u_max=30.0),
            _lib.MacroDesc(n_lanes=4, n_cells=N, dt=0.0, dx=5.0, u_max=30.0),
            _lib.MacroDesc(n_lanes=4, n_cells=N, dt=0.01, dx=5.0, u_max=-1.0))
    for bad in bads:
        assert fwd(C.byref(bad), 3, *fwd_args(some)) == _lib.E_INVALID
        assert bwd(C.byref(bad), 3, *bwd_args(some)) == _lib.E_INVALID
        assert plan(C.byref(bad), 3, 1, C.byref(out)) == _lib.E_INVALID
    assert fwd(None, 3, *fwd_args(some)) == _lib.E_INVALID
    assert bwd(None, 3, *bwd_args(some)) == _lib.E_INVALID
    assert plan(None, 3, 1, C.byref(out)) == _lib.E_INVALID
    assert plan(C.byref(ok), 3, 1, None) == _lib.E_INVALID
    assert fwd(C.byref(ok), -1, *fwd_args(some)) == _lib.E_INVALID
    assert bwd(C.byref(ok), -1, *bwd_args(some)) == _lib.E_INVALID


def test_the_taps_plan_is_the_plan_without_a_history_but_for_the_two_cell_sweep():
    """dhts_macro_taps_plan needs no device: full lanes stay on the pair kernel with the same lanes per workgroup, N = block keeps the
    full reverse instantiation's block, and lanes of 1026 .. 2048 cells take the general reverse sweep (include/dhts.h)."""
    from dhts import ops
    for L, N, T in ((1024, 512, 1000), (4, 128, 5), (4, 256, 7), (2, 63, 9), (2, 65, 3), (1, 1000, 3), (1, 2500, 3), (3, 1, 6), (2, 64, 0)):
        d = ops.macro_desc(L, N, 0.01, 5.0, 30.0)
        plain, taps = ops.macro_rollout_plan(d, T, want_hist=False), ops.macro_taps_plan(d, T, 1)
        assert taps == plain, (L, N, T, plain, taps)
        assert ops.macro_taps_plan(d, T, N) == plain
    assert ops.macro_taps_plan(ops.macro_desc(1024, 512, 0.01, 5.0, 30.0), 1000, 8)["fwd_kernel"] == 2          # the pair kernel
    for N in (1026, 2048):
        d = ops.macro_desc(1, N, 0.01, 5.0, 30.0)
        plain, hist, taps = ops.macro_rollout_plan(d, 3), ops.macro_rollout_plan(d, 3, want_hist=True), ops.macro_taps_plan(d, 3, 2)
        assert plain["bwd_pipelined"] == 2 and hist["bwd_pipelined"] == 0 and taps["bwd_pipelined"] == 0
        assert taps["bwd_block"] == hist["bwd_block"]
        for k in ("fwd_kernel", "fwd_waves", "fwd_passes", "fwd_full_lane", "fwd_lanes_per_group"):
            assert taps[k] == plain[k], k


@pytest.mark.parametrize("bad", [[], [3, 2], [2, 2], [-1, 2], [0, 8], [0, 3, 3, 5], [7, 6, 5], [1.5, 2]], ids=str)
def test_bad_detectors_are_value_errors_before_anything_touches_a_device(bad):
    import torch
    import dhts
    r0, u0, g = torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(2, 2)
    with pytest.raises(ValueError):
        dhts.macro_rollout(r0, u0, g, g, 5, 0.01, 5.0, 30.0, detectors=bad)
    if bad and all(isinstance(b, int) for b in bad):
        with pytest.raises(ValueError):
            dhts.macro_rollout(r0, u0, g, g, 5, 0.01, 5.0, 30.0, detectors=torch.tensor(bad))
        with pytest.raises(ValueError):
            dhts.macro_rollout(r0, u0, torch.zeros(5, 2, 2), torch.zeros(5, 2, 2), 5, 0.01, 5.0, 30.0, detectors=torch.tensor(bad))


def test_other_value_errors_of_the_operator():
    import torch
    import dhts
    r0, u0, g = torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(2, 2)
    with pytest.raises(ValueError):                                            # the history holds every cell
        dhts.macro_rollout(r0, u0, g, g, 5, 0.01, 5.0, 30.0, want_hist=True, detectors=[1, 2])
    with pytest.raises(ValueError):
        dhts.macro_rollout(r0, u0, g, g, 5, 0.01, 5.0, 30.0, detectors=torch.tensor([0.0, 1.0]))
    with pytest.raises(ValueError):
        dhts.macro_rollout(r0, u0, g, g, 5, 0.01, 5.0, 30.0, detectors=torch.tensor([[0, 1]]))
    with pytest.raises(ValueError):
        dhts.macro_rollout(r0, u0, g, g, 5, 0.01, 5.0, 30.0, detectors=torch.tensor([], dtype=torch.int64))
