"""A closed ARZ lane on the two tape-free paths of the macro rollout (dhts_macro_rollout_fwd_ckpt_ring / _bwd_ckpt_ring /
_fwd_ckpt_target_ring / _bwd_ckpt_target_ring / _fwd_jvp_ring, the ops wrappers of the same names, dhts.macro_rollout(ring=True) and
dhts.macro_rollout_jvp(ring=True)): the boundary of the library -- header, bindings, exports, argument checks, every ValueError -- and
the validation of the yardstick tests/macro_ring_ref.py on the oracle alone: against an open lane of three copies of the state,
translation, mass, folded gradients.  What the kernels compute is held against existing device code and the yardstick in
tests/test_macro_ring_gpu.py.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import macro_sched_ref as S
from macro_ring_ref import FOLD_STEPS, ORACLE_CASES, SIZES, jump_state, ring_bwd, ring_fwd, seam_is_live
from util import TOL_GRAD, grad_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, DX, UM = 0.01, 5.0, 30.0
NEW = ("dhts_macro_rollout_fwd_ckpt_ring", "dhts_macro_rollout_bwd_ckpt_ring", "dhts_macro_rollout_fwd_ckpt_target_ring",
       "dhts_macro_rollout_bwd_ckpt_target_ring", "dhts_macro_rollout_fwd_jvp_ring")
SIBLING = {n: n[:-len("_ring")] for n in NEW}
GONE = ("ghost", "ghost_is_sched", "g_ghost", "t_ghost")


def declared(name):
    raw = open(os.path.join(ROOT, "include", "dhts.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, txt)
    assert m, "include/dhts.h does not declare %s" % name
    return [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]


def call_args(names, some, **kw):
    """Arguments 3.. of an entry point: `some` for every pointer, 1 for n_det, kw overrides by name."""
    return [kw[a] if a in kw else (1 if a == "n_det" else some) for a in names[3:]]


# =================================================================================================================
# 1, 2: the library's boundary
# =================================================================================================================
def test_header_library_and_bindings_hold_the_new_entry_points():
    import dhts
    from dhts import _lib, ops
    lib = _lib.lib()
    for name in NEW:
        ours, theirs = declared(name), declared(SIBLING[name])
        assert ours == [a for a in theirs if a not in GONE], "%s is its sibling without %s" % (name, ", ".join(GONE))
        assert getattr(lib, name) is not None
        sig, sib = _lib.SIGNATURES[name][1], _lib.SIGNATURES[SIBLING[name]][1]
        assert len(sig) == len(ours)
        assert list(sig) == [t for t, a in zip(sib, theirs) if a not in GONE], name
        assert callable(getattr(ops, name[len("dhts_"):]))
    assert issubclass(dhts.MacroRolloutRing, dhts.ops.torch.autograd.Function)
    assert issubclass(dhts.MacroRolloutRingTarget, dhts.ops.torch.autograd.Function)


def test_bad_arguments_are_rejected_without_a_gpu():
    """DHTS_E_INVALID with nothing dereferenced: `some` is a pointer nobody may follow, and no device exists here to launch on."""
    from dhts import _lib
    lib = _lib.lib()
    ok = _lib.MacroDesc(3, 100, DT, DX, UM)
    some = C.c_void_p(64)
    required = {NEW[0]: ("r", "y", "u", "ueq", "r_out", "y_out", "u_out", "ueq_out", "ckpt"),
                NEW[1]: ("ckpt", "r", "y", "u", "ueq", "g_r", "g_y", "g_r_out", "g_y_out"),
                NEW[2]: ("r", "y", "u", "ueq", "r_out", "y_out", "u_out", "ueq_out", "target", "sse"),
                NEW[3]: ("ckpt", "r", "y", "u", "ueq", "g_r", "g_y", "target", "g_r_out", "g_y_out"),
                NEW[4]: ("r", "y", "u", "ueq", "t_r", "t_y", "r_out", "y_out", "u_out", "ueq_out", "t_r_out", "t_y_out")}
    for name in NEW:
        fn, names = getattr(lib, name), declared(name)
        for missing in required[name]:
            assert fn(C.byref(ok), 5, 1, *call_args(names, some, **{missing: None})) == _lib.E_INVALID, (name, missing)
        for bad in (_lib.MacroDesc(0, 100, DT, DX, UM), _lib.MacroDesc(3, 0, DT, DX, UM), _lib.MacroDesc(3, 100, 0.0, DX, UM)):
            assert fn(C.byref(bad), 5, 1, *call_args(names, some)) == _lib.E_INVALID, name
        assert fn(C.byref(ok), -1, 1, *call_args(names, some)) == _lib.E_INVALID, name
    # detectors and their array: together or not at all, 1 .. n_cells of them
    for name, arr in ((NEW[0], "taps"), (NEW[1], "g_taps"), (NEW[4], "taps"), (NEW[4], "t_taps")):
        fn, names = getattr(lib, name), declared(name)
        assert fn(C.byref(ok), 5, 1, *call_args(names, some, **{arr: None})) == _lib.E_INVALID, (name, arr)
        assert fn(C.byref(ok), 5, 1, *call_args(names, some, det=None)) == _lib.E_INVALID, name
        assert fn(C.byref(ok), 5, 1, *call_args(names, some, n_det=0)) == _lib.E_INVALID, name
        assert fn(C.byref(ok), 5, 1, *call_args(names, some, n_det=101)) == _lib.E_INVALID, name
    # the siblings' plans hold: a segment beyond max_segment, and the siblings' cell limits
    plan = (C.c_int32 * 8)()
    assert lib.dhts_macro_ckpt_plan(C.byref(ok), 5, 0, 0, C.byref(plan)) == 0
    for name in NEW[:2]:
        assert getattr(lib, name)(C.byref(ok), 5, plan[3] + 1, *call_args(declared(name), some)) == _lib.E_INVALID, name
    assert lib.dhts_macro_ckpt_target_plan(C.byref(ok), 5, 0, C.byref(plan)) == 0
    for name in NEW[2:4]:
        assert getattr(lib, name)(C.byref(ok), 5, plan[3] + 1, *call_args(declared(name), some)) == _lib.E_INVALID, name
    for name, cells in ((NEW[0], 1320), (NEW[1], 1320), (NEW[2], 1240), (NEW[3], 1240), (NEW[4], 1411)):
        long = _lib.MacroDesc(1, cells, DT, DX, UM)
        assert getattr(lib, name)(C.byref(long), 5, 1 if name == NEW[4] else 0, *call_args(declared(name), some)) == _lib.E_INVALID, name
    assert lib.dhts_macro_rollout_fwd_jvp_ring(C.byref(ok), 5, 0, *call_args(declared(NEW[4]), some)) == _lib.E_INVALID       # n_dir < 1
    # the reverse target form: g_sse needs the forward's final state
    assert lib.dhts_macro_rollout_bwd_ckpt_target_ring(C.byref(ok), 5, 1, *call_args(declared(NEW[3]), some, r_fin=None)) == _lib.E_INVALID


def test_every_value_error_is_raised_before_a_device_is_touched():
    """CPU tensors throughout: a call that reached a kernel wrapper would raise TypeError (not a CUDA tensor), not ValueError."""
    import torch
    import dhts
    from dhts import ops
    L, N, T = 2, 6, 4
    r0, u0 = torch.full((L, N), 0.3), torch.full((L, N), 10.0)
    g = torch.zeros(L, 2)
    target = torch.zeros(T, L, 2, N)
    t_r0 = torch.zeros(3, L, N)

    def roll(*a, **kw):
        return dhts.macro_rollout(r0, u0, *a, T, DT, DX, UM, ring=True, **kw)

    def jvp(*a, **kw):
        return dhts.macro_rollout_jvp(r0, u0, *a, T, DT, DX, UM, ring=True, **kw)
    for kw in ({}, dict(checkpoint=False), dict(checkpoint=None, detectors=[0]), dict(target=target)):
        with pytest.raises(ValueError, match="checkpoint=True"):
            roll(None, None, **kw)
    for a in ((g, g), (g, None), (None, g)):
        with pytest.raises(ValueError, match="ghost_r and ghost_u must be None when ring"):
            roll(*a, checkpoint=True)
        with pytest.raises(ValueError, match="ghost_r and ghost_u must be None when ring"):
            roll(*a, checkpoint=True, target=target)
        with pytest.raises(ValueError, match="ghost_r and ghost_u must be None when ring"):
            jvp(*a, fused=True, t_r0=t_r0)
    with pytest.raises(ValueError, match=r"target= for the dense fit, or detectors=range\(N\)"):
        roll(None, None, checkpoint=True, want_hist=True)
    with pytest.raises(ValueError, match="checkpoint must be"):
        roll(None, None, checkpoint=-2)
    with pytest.raises(ValueError, match="segment must be"):
        roll(None, None, checkpoint=10 ** 6)
    with pytest.raises(ValueError, match="strictly ascending"):
        roll(None, None, checkpoint=True, detectors=[1, 0])
    with pytest.raises(ValueError, match="target does not take detectors"):
        roll(None, None, checkpoint=True, target=target, detectors=[0])
    with pytest.raises(ValueError, match="target must be a float32 tensor of shape"):
        roll(None, None, checkpoint=True, target=target[1:])
    with pytest.raises(ValueError, match="max_segment of the target forms"):
        roll(None, None, checkpoint=10 ** 6, target=target)
    # forward mode
    for kw in ({}, dict(fused=False)):
        with pytest.raises(ValueError, match="fused=True"):
            jvp(None, None, t_r0=t_r0, **kw)
    for kw in (dict(t_ghost_r=torch.zeros(3, L, 2)), dict(t_ghost_u=torch.zeros(3, L, 2))):
        with pytest.raises(ValueError, match="t_ghost_r and t_ghost_u must be None when ring"):
            jvp(None, None, fused=True, t_r0=t_r0, **kw)
    with pytest.raises(ValueError, match="at least one of"):
        jvp(None, None, fused=True)
    with pytest.raises(ValueError, match="must have shape"):
        jvp(None, None, fused=True, t_r0=t_r0, t_u0=torch.zeros(3, L, N + 1))
    with pytest.raises(ValueError, match="does not fit the fused"):
        dhts.macro_rollout_jvp(torch.zeros(1, 1411), torch.zeros(1, 1411), None, None, T, DT, DX, UM, ring=True, fused=True,
                               t_r0=torch.zeros(1, 1, 1411))
    # a mis-shaped u0 never reaches a kernel, and `ring` is a bool: `target` or `checkpoint` handed over by position lands there
    for bad in (torch.zeros(L, N + 1), torch.zeros(N)):
        with pytest.raises(ValueError, match="u0 must have its shape"):
            dhts.macro_rollout(r0, bad, None, None, T, DT, DX, UM, ring=True, checkpoint=True)
        with pytest.raises(ValueError, match="u0 must have its shape"):
            dhts.macro_rollout_jvp(r0, bad, None, None, T, DT, DX, UM, ring=True, fused=True, t_r0=t_r0)
    with pytest.raises(ValueError, match="ring must be True or False"):
        dhts.macro_rollout(r0, u0, g, g, T, DT, DX, UM, False, True, None, target, 2)
    with pytest.raises(ValueError, match="ring must be True or False"):
        dhts.macro_rollout(r0, u0, g, g, T, DT, DX, UM, ring=1)
    # without ring nothing is asked that was not asked before
    with pytest.raises(ValueError, match="ghost_r and ghost_u must have shape"):
        dhts.macro_rollout(r0, u0, g[:1], g[:1], T, DT, DX, UM)
    # ... and the raw wrappers' own, which need no device either
    desc, ck = ops.macro_desc(L, N, DT, DX, UM), torch.zeros(0)
    with pytest.raises(ValueError, match="ckpt must be"):
        ops.macro_rollout_fwd_ckpt_ring(desc, T, r0, r0, u0, u0, ck)
    with pytest.raises(ValueError, match="ckpt must be"):
        ops.macro_rollout_bwd_ckpt_ring(desc, T, ck, r0, r0, u0, u0, r0, r0)
    with pytest.raises(ValueError, match="det and g_taps go together"):
        ops.macro_rollout_bwd_ckpt_ring(desc, T, ck, r0, r0, u0, u0, r0, r0, det=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="target must be a contiguous float32"):
        ops.macro_rollout_fwd_ckpt_target_ring(desc, T, r0, r0, u0, u0, None, target[:, :, :, :-1])
    with pytest.raises(ValueError, match="ckpt must be"):
        ops.macro_rollout_bwd_ckpt_target_ring(desc, T, None, r0, r0, u0, u0, r0, r0, target)
    with pytest.raises(ValueError, match="must have shape"):
        ops.macro_rollout_fwd_jvp_ring(desc, T, r0, r0, u0, u0[:, 1:], t_r0, t_r0)
    with pytest.raises(ValueError, match="t_r and t_y must have shape"):
        ops.macro_rollout_fwd_jvp_ring(desc, T, r0, r0, u0, u0, t_r0[:, :1], t_r0)


def test_resource_listing_keeps_every_existing_kernel():
    """profiles/macro_ring_resources_parent.txt against profiles/macro_ring_resources.txt (compiler output for gfx950, one line per
    kernel of macro_kernels.hip): every kernel of the parent has identical figures -- the fifty-four tape-free ones with a boundary
    under the longer name the enum gives them, false = 0 (constant), true = 1 (a schedule) --; the new lines are the twenty-seven ring
    forms, none with scratch or a vector-register spill.  The issue asks for no spill in the ring forms: that holds for the nine
    checkpointed ones and for the fused kernel's nine without detectors.  The fused kernel's forms with detectors spill scalar
    registers into vector lanes in the parent already (the constant forms: six of nine, 20 .. 54), so there zero is out of reach and
    the bound is the constant-boundary sibling's figure, form by form -- an OPEN deviation from the issue, DESIGN 4l.  No ring form
    spills more, takes more scalar registers in the reverse kernels, or reaches a lower occupancy than its constant sibling."""
    def read(name):
        rows = {}
        for line in open(os.path.join(ROOT, "profiles", name)).read().splitlines():
            kernel, figures = line.split(" SGPRs ")
            rows[kernel.strip()] = "SGPRs " + " ".join(figures.split())
        return rows
    parent, new = read("macro_ring_resources_parent.txt"), read("macro_ring_resources.txt")
    bounded = {"macro_rollout_ckpt_fwd_kernel<": 1, "macro_rollout_ckpt_bwd_kernel<": 0, "macro_rollout_ckpt_fwd_target_kernel<": 1,
               "macro_rollout_ckpt_bwd_target_kernel<": 0, "macro_rollout_fwd_jvp_kernel<": 2}      # name: position of the boundary

    def renamed(k):
        for stem, pos in bounded.items():
            if k.startswith(stem):
                args = k[len(stem):-1].split(", ")
                args[pos] = "(dhts::MacroBoundary)%d" % (args[pos] == "true")
                return stem + ", ".join(args) + ">"
        return k

    def num(row, key):
        return int(re.search(r"%s\s+(\d+)" % key, row).group(1))
    assert len(parent) == 179 and sum(k.startswith(tuple(bounded)) for k in parent) == 54
    for k, figures in parent.items():
        assert new.get(renamed(k)) == figures, k
    added = sorted(set(new) - {renamed(k) for k in parent})
    assert len(added) == 27 and all(k.startswith(tuple(bounded)) and "(dhts::MacroBoundary)2" in k for k in added), added
    assert sum("fwd_jvp" in k for k in added) == 18 and sum("ckpt_bwd" in k for k in added) == 3
    for k in added:
        const = new[k.replace("Boundary)2", "Boundary)0")]
        assert " scratch 0 " in new[k] and " vgpr_spill 0 " in new[k], (k, new[k])
        assert num(new[k], "sgpr_spill") <= num(const, "sgpr_spill"), (k, new[k], const)
        assert num(new[k], "occupancy") >= num(const, "occupancy"), (k, new[k], const)
        if "ckpt" in k or k.endswith("false>"):
            assert " sgpr_spill 0 " in new[k], (k, new[k])
        if "ckpt_bwd" in k:
            assert num(new[k], "SGPRs") <= num(const, "SGPRs"), k


# =================================================================================================================
# 3 - 7: the yardstick on the oracle alone
# =================================================================================================================
CASES = [(1, 1, 1), (2, 2, 2), (1, 3, 3), (2, 7, 7), (1, 20, 13), (2, 65, 9)]      # (L, N, T <= N)


def tiled(O, r, u, T, seed=5):
    """The open lane of 3 N cells that holds the state three times, any boundary cells -> the chained oracle's run."""
    rng = np.random.default_rng(seed)
    L = r.shape[0]
    gr = np.broadcast_to(rng.uniform(0.1, 0.9, (1, L, 2)).astype(S.F), (T, L, 2))
    gu = np.broadcast_to(rng.uniform(0.0, UM, (1, L, 2)).astype(S.F), (T, L, 2))
    return S.sched_fwd(O, np.tile(r, (1, 3)), np.tile(u, (1, 3)), gr, gu, DT, DX, UM)


@pytest.mark.parametrize("L,N,T", CASES)
def test_ring_is_the_middle_copy_of_a_tiled_open_lane(oracle, L, N, T):
    """Information moves one cell per step, so for T <= N the open ends cannot reach the middle copy: bit for bit."""
    r, u = jump_state(L, N, seed=N)
    f, ft = ring_fwd(oracle, r, u, T, DT, DX, UM), tiled(oracle, r, u, T)
    for k in ("rT", "yT", "uT", "qT"):
        assert np.array_equal(f[k], ft[k][:, N:2 * N]), k
    for k in ("hist_r", "hist_y", "hist_u"):
        assert np.array_equal(f[k], ft[k][:, :, N:2 * N]), k
    if N > 1:
        assert not np.array_equal(ft["rT"][:, :N], ft["rT"][:, N:2 * N]), "the open end did not move the first copy: the case shows nothing"


@pytest.mark.parametrize("N,m", [(2, 1), (7, 3), (20, 13), (65, 64)])
def test_translation(oracle, N, m):
    T = 2 * N + 5
    r, u = jump_state(2, N, seed=N)
    f = ring_fwd(oracle, r, u, T, DT, DX, UM)
    fm = ring_fwd(oracle, np.roll(r, m, axis=1), np.roll(u, m, axis=1), T, DT, DX, UM)
    for k in ("rT", "yT", "uT", "qT"):
        assert np.array_equal(np.roll(f[k], m, axis=1), fm[k]), k
    assert np.array_equal(np.roll(f["hist_r"], m, axis=2), fm["hist_r"])


def mass_bound(f):
    T, (L, N) = f["T"], f["r0"].shape
    return T * N * 2.0 ** -24 * float(max(f["r0"].max(), f["hist_r"].max() if T else 0.0))


@pytest.mark.parametrize("N", [7, 20, 65])
def test_mass_is_conserved_and_the_bound_tells_an_open_lane_apart(oracle, N):
    T = 2 * N + 5
    r, u = jump_state(2, N, seed=N)
    f = ring_fwd(oracle, r, u, T, DT, DX, UM)
    drift = np.abs(f["rT"].astype(np.float64).sum(axis=1) - r.astype(np.float64).sum(axis=1))
    print("N = %d: mass drift %s, bound %.3e" % (N, drift, mass_bound(f)))
    assert np.all(drift <= mass_bound(f))
    # the interface at the seam carries both Jacobians in at least one step: its B block is d2 of cell N - 1, up to the factor -dt / dx
    assert all(seam_is_live(f, l) for l in range(2)), "interface 0 is trivial in every step"
    # the same inputs on an open lane fed the ring's own upstream cell but an emptier downstream one
    L = r.shape[0]
    gr = np.stack([np.stack([f["hist_r"][max(t - 1, 0), :, N - 1], np.full(L, 0.02, S.F)], axis=1) for t in range(T)])
    gu = np.stack([np.stack([f["hist_u"][max(t - 1, 0), :, N - 1], np.full(L, 25.0, S.F)], axis=1) for t in range(T)])
    fo = S.sched_fwd(oracle, r, u, gr, gu, DT, DX, UM)
    leak = np.abs(fo["rT"].astype(np.float64).sum(axis=1) - r.astype(np.float64).sum(axis=1))
    assert np.all(leak > mass_bound(f)), (leak, mass_bound(f))


@pytest.mark.parametrize("L,N,T", CASES)
@pytest.mark.parametrize("loss", ["final", "every"])
def test_gradients_are_the_folded_gradients_of_the_tiled_lane(oracle, L, N, T, loss):
    r, u = jump_state(L, N, seed=N)
    f, ft = ring_fwd(oracle, r, u, T, DT, DX, UM), tiled(oracle, r, u, T)
    rng = np.random.default_rng(N)

    def mid(a):
        z = np.zeros(a.shape[:-1] + (3 * N,), S.F)
        z[..., N:2 * N] = a
        return z
    if loss == "final":
        cot = dict(g_rT=rng.standard_normal((L, N)).astype(S.F), g_uT=rng.standard_normal((L, N)).astype(S.F))
    else:
        cot = dict(gh_r=rng.standard_normal((T, L, N)).astype(S.F), gh_y=rng.standard_normal((T, L, N)).astype(S.F),
                   gh_u=rng.standard_normal((T, L, N)).astype(S.F))
    b = ring_bwd(oracle, f, **cot)
    bt = S.sched_bwd(oracle, ft, **{k: mid(v) for k, v in cot.items()})
    for k in ("g_r0", "g_u0"):
        folded = bt[k].astype(np.float64).reshape(L, 3, N).sum(axis=1)
        assert grad_report("%s N=%d T=%d %s" % (k, N, T, loss), b[k], folded) <= TOL_GRAD


@pytest.mark.parametrize("L,N,T", sorted({(3, N, min(N, FOLD_STEPS)) for N in SIZES} | {(3, N, 1) for N in SIZES} | set(ORACLE_CASES) |
                                            {(3, N, min(2 * N + 5, 650)) for N in SIZES}))
def test_the_seam_is_live_in_every_shape_the_gpu_tests_run(oracle, L, N, T):
    """jump_state(seed=N), as tests/test_macro_ring_gpu.py calls it, at its sizes and step counts (one step included: the forward-bits
    cases): the chained oracle raises no CFL return code, and on every lane the seam interface is non-trivial in at least one step, so
    that the device comparisons carry both of its Jacobians.  One cell is its own neighbour: equal states, a trivial interface."""
    r, u = jump_state(L, N, seed=N)
    f = ring_fwd(oracle, r, u, T, DT, DX, UM)
    assert f["rc"] is None
    if N >= 2:
        assert all(seam_is_live(f, l) for l in range(L)), (L, N, T)


@pytest.mark.parametrize("N", [1, 2, 9])
def test_a_constant_state_stays_constant(oracle, N):
    r, u = np.full((2, N), 0.4, S.F), np.full((2, N), 7.0, S.F)
    f = ring_fwd(oracle, r, u, 2 * N + 5, DT, DX, UM)
    assert np.array_equal(f["rT"], r) and np.all(f["hist_r"] == S.F(0.4))
    assert np.all(f["hist_y"] == f["hist_y"][0, 0, 0]) and np.all(f["hist_u"] == f["hist_u"][0, 0, 0])


def test_one_cell_never_changes(oracle):
    r, u = np.array([[0.7]], S.F), np.array([[3.0]], S.F)
    f = ring_fwd(oracle, r, u, 6, DT, DX, UM)
    assert np.array_equal(f["rT"], r) and np.all(f["hist_r"] == r[0, 0])
