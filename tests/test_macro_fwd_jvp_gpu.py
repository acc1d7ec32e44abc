"""The tape-free fused rollout + tangent kernel of the ARZ rollout on the GPU (dhts_macro_rollout_fwd_jvp, dhts.macro_rollout_jvp(
fused=True)): bit for bit what the taped pair returns -- lane-kernel and pair-kernel tapes, constant boundary cells and a schedule,
with and without detectors, one masked launch and two launches --; the tangents against the float64 chain on the oracle's blocks; a
direction does not depend on K or on its slot; memory and index safety at the raw operator; the two fault records; nothing of size T;
the plan's refusal of a lane that does not fit; the example.  Shapes and inputs are those of tests/test_macro_jvp_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import macro_jvp_ref as J
import test_macro_jvp_gpu as TJ
from test_macro_jvp_gpu import edges, same_bits
from util import TOL_GRAD, grad_report, options

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, DX, UM = 0.01, 5.0, 30.0
GUARD, SENTINEL = 257, 12345.0

# id: (the case of tests/test_macro_jvp_gpu.py whose shape, inputs and tangents it takes, DHTS_OPT_MACRO_FWD_GROUP of the taped side)
SHAPES = {
    "1x5": ("gen1", 0), "2x7": ("fast2", 0), "63x5": ("fast63", 0), "64x1": ("fast64", 0), "65x12": ("fast65", 0), "130x5": ("fast130", 0),
    "300x2": ("fast300", 0), "1000x2": ("fast1000", 0), "128x5": ("pair128_g1", 0), "256x12": ("pair256_g1", 0), "64x0": ("fast64_t0", 0),
    # pair-kernel tapes with one and four lanes per workgroup (L = 4)
    "128x5_g1": ("pair128_g1", 1), "128x2_g4": ("pair128_g4", 4), "256x12_g1": ("pair256_g1", 1), "256x1_g4": ("pair256_g4", 4),
}
for _s, (_c, _g) in SHAPES.items():
    assert TJ.CASES[_c][3] == 0, "no case with DHTS_OPT_MACRO_FWD_VARIANT set"
assert sorted((TJ.CASES[c][:3]) for c, g in SHAPES.values() if g == 0) == sorted(
    [(3, 1, 5), (3, 2, 7), (2, 63, 5), (2, 64, 1), (2, 65, 12), (2, 130, 5), (2, 300, 2), (1, 1000, 2), (4, 128, 5), (4, 256, 12), (2, 64, 0)])


def leaves_and_tangents(cuda, case, sched, K, T=None):
    import torch
    leaves = list(TJ.inputs(case, sched))
    tans = [a[:K] for a in TJ.leaf_tangents(case, sched)]
    if T is not None and sched:                      # the first T rows of the schedule and of its tangents
        leaves[2:] = [a[:T] for a in leaves[2:]]
        tans[2:] = [a[:, :T] for a in tans[2:]]
    return [torch.tensor(a, device=cuda) for a in leaves], [torch.tensor(np.ascontiguousarray(a), device=cuda) for a in tans]


def run_both(leaves, tans, T, det, group=0, **kw):
    import dhts
    kw = dict(kw, t_r0=tans[0], t_u0=tans[1], t_ghost_r=tans[2], t_ghost_u=tans[3], detectors=det)
    fused = dhts.macro_rollout_jvp(*leaves, T, DT, DX, UM, fused=True, **kw)
    with options(0, group):
        taped = dhts.macro_rollout_jvp(*leaves, T, DT, DX, UM, fused=False, **kw)
    return fused, taped


def assert_same_structure_and_bits(fused, taped, tag):
    assert len(fused) == len(taped) == 2
    for f, t, part in zip(fused, taped, ("primal", "tangent")):
        assert len(f) == len(t), (tag, part)
        for j, (a, b) in enumerate(zip(f, t)):
            assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), (tag, part, j, tuple(a.shape), tuple(b.shape))
            assert same_bits(a.cpu().numpy(), b.cpu().numpy()), "%s: %s output %d differs from the taped path" % (tag, part, j)


# ---- 1. bit identity with the taped path -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", TJ.BOTH, ids=["const", "sched"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_fused_equals_the_taped_path_bit_for_bit(cuda, shape, sched):
    from dhts import ops
    case, group = SHAPES[shape]
    L, N, T = TJ.CASES[case][:3]
    desc = ops.macro_desc(L, N, DT, DX, UM)
    for K, launches in ((5, 2), (3, 1)):             # launches of 4 + 1; one masked launch of 4
        if N <= 512:                                 # (1000 cells: two directions per launch, 2 + 2 + 1 and 2 + 1)
            assert ops.macro_fwd_jvp_plan(desc, T, K)["launches"] == (launches if T else 0)
            assert ops.macro_fwd_jvp_plan(desc, T, K)["dirs_per_launch"] == 4
        else:
            assert ops.macro_fwd_jvp_plan(desc, T, K) == dict(waves=8, passes=2, dirs_per_launch=2, launches=3 if K == 5 else 2,
                                                              lds_bytes=ops.macro_fwd_jvp_plan(desc, T, 2)["lds_bytes"])
        leaves, tans = leaves_and_tangents(cuda, case, sched, K)
        for det in (edges(N), None):
            fused, taped = run_both(leaves, tans, T, det, group)
            assert len(fused[0]) == (5 if det else 4) and len(fused[1]) == (4 if det else 3)
            assert tuple(fused[1][0].shape) == (K, L, N)
            if det:
                assert tuple(fused[0][4].shape) == (T, L, 3, len(det)) and tuple(fused[1][3].shape) == (K, T, L, 3, len(det))
            assert_same_structure_and_bits(fused, taped, "%s %s K = %d %s" % (shape, "sched" if sched else "const", K, "det" if det else "plain"))


# ---- 2. not resting on the taped path alone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", TJ.BOTH, ids=["const", "sched"])
@pytest.mark.parametrize("case", ["fast64", "fast130", "fast300"])
def test_fused_tangents_against_the_oracle_chain(cuda, oracle, case, sched):
    import dhts
    L, N, T = TJ.CASES[case][:3]
    K, det = TJ.KMAX, edges(N)
    leaves, tans = leaves_and_tangents(cuda, case, sched, K)
    _, tang = dhts.macro_rollout_jvp(*leaves, T, DT, DX, UM, t_r0=tans[0], t_u0=tans[1], t_ghost_r=tans[2], t_ghost_u=tans[3], detectors=det,
                                     fused=True)
    f = TJ.oracle_chain(oracle, case, sched)
    tn = TJ.leaf_tangents(case, sched)
    for i in range(K):
        t_gr, t_gu = (tn[2][i], tn[3][i]) if sched else (np.tile(tn[2][i][None], (T, 1, 1)), np.tile(tn[3][i][None], (T, 1, 1)))
        o = J.jvp(f, t_r0=tn[0][i], t_u0=tn[1][i], t_gr=t_gr, t_gu=t_gu, det=det)
        for j, k in enumerate(("t_rT", "t_yT", "t_uT", "t_read")):
            assert np.abs(o[k]).max() > 0
            assert grad_report("fused %s %s direction %d %s" % (case, "sched" if sched else "const", i, k), tang[j][i].cpu().numpy(),
                               o[k]) <= TOL_GRAD


# ---- 3. a direction does not depend on K or on its slot ----------------------------------------------------------------------------------
def test_a_direction_does_not_depend_on_k_or_its_slot(cuda):
    import torch
    import dhts
    L, N, T, KK = 2, 65, 6, 9
    leaves, _ = leaves_and_tangents(cuda, "fast65", True, 1, T=T)
    rng = np.random.default_rng(65006)
    tans = [torch.tensor(rng.standard_normal(s).astype(np.float32), device=cuda)
            for s in ((KK, L, N), (KK, L, N), (KK, T, L, 2), (KK, T, L, 2))]
    det = edges(N)
    runs = {}
    for K in range(1, KK + 1):
        runs[K] = dhts.macro_rollout_jvp(*leaves, T, DT, DX, UM, t_r0=tans[0][:K], t_u0=tans[1][:K], t_ghost_r=tans[2][:K],
                                         t_ghost_u=tans[3][:K], detectors=det, fused=True)
    full = runs[KK]
    assert all(float(t.abs().max()) > 0 for t in full[1])
    for K in range(1, KK):
        for j, (a, b) in enumerate(zip(runs[K][0], full[0])):
            assert same_bits(a.cpu().numpy(), b.cpu().numpy()), "the primal output %d at K = %d" % (j, K)
        for j, (a, b) in enumerate(zip(runs[K][1], full[1])):
            for i in range(K):
                assert same_bits(a[i].cpu().numpy(), b[i].cpu().numpy()), "direction %d of output %d at K = %d" % (i, j, K)


# ---- 4. raw operator safety --------------------------------------------------------------------------------------------------------------
def raw(cuda, case, T, det, K=5, ghost=True, poison=None, dt=DT, leaves=None):
    """One call of ops.macro_rollout_fwd_jvp on the case's leaves (a schedule; `leaves`: others of the case's shape) with every output in
    the middle of a larger buffer: NaN where it belongs, a sentinel on both sides."""
    import torch
    from dhts import ops
    L, N = TJ.CASES[case][:2]
    r0, u0, gr, gu = TJ.inputs(case, True) if leaves is None else leaves
    gr, gu = gr[:T], gu[:T]
    rng = np.random.default_rng(4000 + sum(map(ord, case)))
    t_r, t_y = rng.standard_normal((2, K, L, N)).astype(np.float32)
    t_g = rng.standard_normal((K, T, L, 2, 2)).astype(np.float32)
    if poison is not None:
        t_r[poison] = np.nan
    desc = ops.macro_desc(L, N, dt, DX, UM)
    r, u = torch.tensor(r0, device=cuda), torch.tensor(u0, device=cuda)
    y, q = ops.macro_state_from_ru(r, u, UM)
    br, bu = torch.tensor(gr, device=cuda), torch.tensor(gu, device=cuda)
    by, bq = ops.macro_state_from_ru(br, bu, UM)
    ghost_q = torch.stack([br, by, bu, bq], dim=-1).contiguous()
    D = len(det)
    sizes = [L * N] * 4 + [K * L * N] * 2 + [T * L * 3 * D, K * T * L * 2 * D]
    bufs = [torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=cuda) for n in sizes]
    views = [b[GUARD:GUARD + n] for b, n in zip(bufs, sizes)]
    for v in views:
        v.fill_(float("nan"))
    out = tuple(v.view(L, N) for v in views[:4]) + tuple(v.view(K, L, N) for v in views[4:6])
    taps, t_taps = views[6].view(T, L, 3, D), views[7].view(K, T, L, 2, D)
    err, err_jvp = ops.new_error_record(cuda), ops.new_error_record(cuda)
    tg = None if not ghost else torch.tensor(t_g * (0 if ghost == "zero" else 1), device=cuda)
    res = ops.macro_rollout_fwd_jvp(desc, T, r, y, u, q, ghost_q, torch.tensor(t_r, device=cuda), torch.tensor(t_y, device=cuda), t_ghost=tg,
                                    det=torch.tensor(det, dtype=torch.int32, device=cuda), err=err, err_jvp=err_jvp, out=out, taps=taps,
                                    t_taps=t_taps)
    assert res[0][0].data_ptr() == out[0].data_ptr() and res[1][1].data_ptr() == out[5].data_ptr()
    assert res[0][4].data_ptr() == taps.data_ptr() and res[1][2].data_ptr() == t_taps.data_ptr()
    for b, n in zip(bufs, sizes):
        h = b.cpu().numpy()
        assert np.all(h[:GUARD] == SENTINEL) and np.all(h[GUARD + n:] == SENTINEL), "a store beside the outputs"
    names = ("r", "y", "u", "q", "t_r", "t_y")
    o = {k: v.cpu().numpy() for k, v in zip(names, out)}
    o.update(taps=taps.cpu().numpy(), t_taps=t_taps.cpu().numpy(), err=err.tolist(), err_jvp=err_jvp.tolist(),
             args=(desc, r, y, u, q, ghost_q, t_r, t_y, t_g))
    return o


KEYS = ("r", "y", "u", "q", "t_r", "t_y", "taps", "t_taps")


@pytest.mark.parametrize("case,T", [("fast65", 5), ("fast1000", 2)])
def test_raw_operator_writes_everything_and_nothing_else(cuda, case, T):
    N = TJ.CASES[case][1]
    a = raw(cuda, case, T, edges(N))
    assert a["err"] == [0, 0, 0, 0] and a["err_jvp"] == [0, 0, 0, 0]
    for k in KEYS:
        assert not np.isnan(a[k]).any(), "%d elements of %s were not written" % (int(np.isnan(a[k]).sum()), k)
    # an entry outside [0, N) is compared away before any address is formed: its column stays as it was, the others are unchanged
    good = raw(cuda, case, T, [2, N - 1])
    b = raw(cuda, case, T, [2, -1, N - 1, N])
    for k in ("taps", "t_taps"):
        assert same_bits(b[k][..., [0, 2]], good[k]), k
        assert np.isnan(b[k][..., [1, 3]]).all(), k
    for k in KEYS[:6]:
        assert same_bits(a[k], good[k]) and same_bits(b[k], good[k]), k
    # zero boundary tangents are the NULL ones
    z, n = raw(cuda, case, T, edges(N), ghost="zero"), raw(cuda, case, T, edges(N), ghost=False)
    for k in KEYS:
        assert same_bits(z[k], n[k]), k
    assert not same_bits(z["t_r"], a["t_r"])


# ---- 5. fault records --------------------------------------------------------------------------------------------------------------------
def test_a_nan_tangent_goes_on_the_tangent_record_alone(cuda):
    import torch
    from dhts import _lib, ops
    case, T, K = "fast65", 4, 3
    N = TJ.CASES[case][1]
    clean = raw(cuda, case, T, edges(N), K=K)
    a = raw(cuda, case, T, edges(N), K=K, poison=(1, 1, 7))
    # what the taped sweep records for the same input
    desc, r, y, u, q, ghost_q, t_r, t_y, t_g = a["args"]
    tape = torch.zeros(ops.macro_tape_numel(desc, T), dtype=torch.float32, device=cuda)
    ops.macro_rollout_fwd_sched(desc, T, r, y, u, q, ghost_q, tape=tape)
    err = ops.new_error_record(cuda)
    ops.macro_rollout_jvp(desc, T, tape, torch.tensor(t_r, device=cuda), torch.tensor(t_y, device=cuda), t_ghost=torch.tensor(t_g, device=cuda),
                          det=torch.tensor(edges(N), dtype=torch.int32, device=cuda), err=err)
    print("fused err_jvp", a["err_jvp"], "taped sweep", err.tolist())
    assert a["err_jvp"][:3] == [_lib.FAULT_NAN, 0, 1] and a["err_jvp"][3] in (6, 7, 8)
    assert a["err_jvp"] == err.tolist()
    assert a["err"] == [0, 0, 0, 0]
    for k in ("r", "y", "u", "q", "taps"):
        assert same_bits(a[k], clean[k]), "the primal output %s" % k
    assert np.isfinite(a["t_r"][[0, 2]]).all() and np.isnan(a["t_r"][1, 1]).any() and np.isfinite(a["t_r"][1, 0]).all()


def slow_traffic(L, N, T, fast=None):
    """Leaves that keep the CFL bound at dt = 1.0, dx = 5 (every characteristic speed inside (-5, 5): u in [1.5, 3], u - 15 sqrt(r) >= -3.5
    at r <= 0.08, middle states included; the float64 oracle steps them for four steps without a fault), and with `fast` = (step, lane)
    a downstream boundary cell at u = 20 in that row: interface N of that lane in that step is the ONE violation of the rollout."""
    rng = np.random.default_rng(6504)
    r0 = rng.uniform(0.02, 0.08, (L, N)).astype(np.float32)
    u0 = rng.uniform(1.5, 3.0, (L, N)).astype(np.float32)
    gr = rng.uniform(0.02, 0.08, (T, L, 2)).astype(np.float32)
    gu = rng.uniform(1.5, 3.0, (T, L, 2)).astype(np.float32)
    if fast is not None:
        gu[fast[0], fast[1], 1] = 20.0
    return r0, u0, gr, gu


def test_a_cfl_violation_goes_on_the_forward_record_and_raises_as_the_taped_path(cuda):
    """(2, 65, 4) at dt = 1.0.  A fault record is first-wins among the threads AND the lanes that fault (one compare-and-swap each, in
    every forward kernel), so an input in which both lanes violate the bound -- test_macro_jvp_gpu.inputs at dt = 1.0: every interface in
    step 0 -- has no record of its own: ops.macro_rollout_fwd leaves lane 0 in one run and lane 1 in the next.  The input here violates
    the bound at exactly one (step, lane, interface), the last step's downstream boundary of lane 1, so the forward's record is a
    function of the input and the fused kernel's must equal it, as must the text of the AssertionError."""
    import torch
    import dhts
    from dhts import _lib, ops
    case, T, K = "fast65", 4, 3
    L, N = TJ.CASES[case][:2]
    calm = raw(cuda, case, T, edges(N), K=K, dt=1.0, leaves=slow_traffic(L, N, T))
    assert calm["err"] == [0, 0, 0, 0] and calm["err_jvp"] == [0, 0, 0, 0], "the control: no violation without the fast boundary cell"
    leaves = slow_traffic(L, N, T, fast=(T - 1, 1))
    a = raw(cuda, case, T, edges(N), K=K, dt=1.0, leaves=leaves)
    desc, r, y, u, q, ghost_q = a["args"][:6]
    err = ops.new_error_record(cuda)
    ops.macro_rollout_fwd_sched(desc, T, r, y, u, q, ghost_q, err=err)
    print("fused err", a["err"], "forward", err.tolist(), "fused err_jvp", a["err_jvp"])
    assert err.tolist() == [_lib.FAULT_CFL, T - 1, 1, N]
    assert a["err"] == err.tolist()
    assert a["err_jvp"] == [0, 0, 0, 0]
    dev = [torch.tensor(x, device=cuda) for x in leaves]
    _, tans = leaves_and_tangents(cuda, case, True, K, T=T)
    kw = dict(t_r0=tans[0], t_u0=tans[1], t_ghost_r=tans[2], t_ghost_u=tans[3], detectors=edges(N))
    text = {}
    for fused in (False, True):
        with pytest.raises(AssertionError) as e:
            dhts.macro_rollout_jvp(*dev, T, 1.0, DX, UM, fused=fused, **kw)
        text[fused] = str(e.value)
        dhts.macro_rollout_jvp(*dev, T, 1.0, DX, UM, fused=fused, check_faults=False, **kw)       # neither raises
    print(text[True])
    assert "CFL" in text[True] and "(step %d, lane 1, interface %d)" % (T - 1, N) in text[True] and text[True] == text[False]


# ---- 6. nothing of size T is allocated ---------------------------------------------------------------------------------------------------
def test_nothing_of_size_t_is_allocated(cuda):
    """L, N, T = 2, 64, 5000: the tape of the taped path is T L 3200 B = 32.0 MB; the fused call's peak above its resident inputs stays
    below an eighth of that (its outputs, readings included, are about 1 MB).  The float64 oracle steps this input for 5000 steps without
    a CFL fault to a finite state (r in [0.29, 0.73], u in [6.3, 12.2])."""
    import torch
    import dhts
    from dhts import ops
    L, N, T, K, D = 2, 64, 5000, 2, 1
    k = np.arange(N)
    r0 = np.stack([0.3 + 0.2 * np.sin(2 * np.pi * k / N), 0.5 + 0.3 * np.cos(2 * np.pi * k / N)]).astype(np.float32)
    u0 = np.stack([np.full(N, 12.0), 8 + 4 * np.sin(2 * np.pi * k / N)]).astype(np.float32)
    gr, gu = np.array([[0.3, 0.3], [0.8, 0.2]], np.float32), np.array([[12, 12], [5, 20]], np.float32)
    rng = np.random.default_rng(6)
    leaves = [torch.tensor(a, device=cuda) for a in (r0, u0, gr, gu)]
    tg = [torch.tensor(rng.standard_normal((K, L, 2)).astype(np.float32), device=cuda) for _ in range(2)]
    kw = dict(t_ghost_r=tg[0], t_ghost_u=tg[1], detectors=[32])
    tape_bytes = T * L * 3200
    assert tape_bytes == ops.macro_tape_numel(ops.macro_desc(L, N, DT, DX, UM), T) * 4
    dhts.macro_rollout_jvp(*leaves, 2, DT, DX, UM, fused=True, **kw)              # (first-call allocations of the runtime are not the call's)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    resident = torch.cuda.memory_allocated()
    fused = dhts.macro_rollout_jvp(*leaves, T, DT, DX, UM, fused=True, **kw)      # check_faults: both records are read and empty
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - resident
    print("fused peak above the resident inputs: %d B (%.3f MB); the tape would be %.1f MB" % (peak, peak / 2 ** 20, tape_bytes / 1e6))
    assert peak < tape_bytes // 8
    taped = dhts.macro_rollout_jvp(*leaves, T, DT, DX, UM, fused=False, **kw)
    assert torch.cuda.max_memory_allocated() - resident >= tape_bytes, "the taped path holds the tape"
    assert_same_structure_and_bits(fused, taped, "T = 5000")
    assert all(bool(torch.isfinite(t).all()) for part in fused for t in part)
    # the raw operator with records of its own: both stay empty
    desc = ops.macro_desc(L, N, DT, DX, UM)
    y0, q0 = ops.macro_state_from_ru(leaves[0], leaves[1], UM)
    gy, gq = ops.macro_state_from_ru(leaves[2], leaves[3], UM)
    ghost = torch.stack([leaves[2], gy, leaves[3], gq], dim=-1).contiguous()
    err, err_jvp = ops.new_error_record(cuda), ops.new_error_record(cuda)
    t_g = torch.stack([tg[0], ops.macro_state_from_ru_jvp(leaves[2].expand(K, L, 2), leaves[3].expand(K, L, 2), tg[0], tg[1], UM)], dim=-1)
    z = torch.zeros(K, L, N, device=cuda)
    ops.macro_rollout_fwd_jvp(desc, T, leaves[0], y0, leaves[1], q0, ghost, z, z.clone(), t_ghost=t_g.contiguous(),
                              det=torch.tensor([32], dtype=torch.int32, device=cuda), err=err, err_jvp=err_jvp)
    assert err.tolist() == [0, 0, 0, 0] and err_jvp.tolist() == [0, 0, 0, 0]


# ---- 7. the plan and the ValueError on the device ----------------------------------------------------------------------------------------
def test_a_lane_that_does_not_fit_is_refused_and_the_taped_path_still_runs(cuda):
    import torch
    import dhts
    from dhts import _lib
    L, N, T = 1, _lib.MACRO_MAX_CELLS, 2
    rng = np.random.default_rng(7)
    leaves = [torch.tensor(rng.uniform(lo, hi, s).astype(np.float32), device=cuda)
              for lo, hi, s in ((0.2, 0.8, (L, N)), (5.0, 20.0, (L, N)), (0.2, 0.8, (L, 2)), (5.0, 20.0, (L, 2)))]
    t_r0 = torch.tensor(rng.standard_normal((2, L, N)).astype(np.float32), device=cuda)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError) as e:
        dhts.macro_rollout_jvp(*leaves, T, DT, DX, UM, t_r0=t_r0, fused=True)
    assert str(N) in str(e.value) and "fused=False" in str(e.value)
    assert torch.cuda.memory_allocated() == before, "refused before anything was allocated or launched"
    primal, tang = dhts.macro_rollout_jvp(*leaves, T, DT, DX, UM, t_r0=t_r0, fused=False)
    assert tuple(tang[0].shape) == (2, L, N) and bool(torch.isfinite(tang[0]).all()) and float(tang[0].abs().max()) > 0


def test_the_raw_tape_free_wrappers_keep_their_errors_texts_and_order(cuda):
    """What the raw wrappers of the tangent and checkpointed paths raise once their tensors are on the device (nothing is launched):
    each message word for word, and where two things are wrong the one that is reported."""
    import re
    import torch
    from dhts import ops
    L, N, T, K = 2, 8, 5, 3
    desc = ops.macro_desc(L, N, DT, DX, UM)
    f32 = dict(dtype=torch.float32, device=cuda)
    z, ghost, tr = torch.zeros(L, N, **f32), torch.zeros(L, 2, 4, **f32), torch.zeros(K, L, N, **f32)
    det = torch.tensor([0, 7], dtype=torch.int32, device=cuda)
    many = torch.arange(N + 1, dtype=torch.int32, device=cuda)
    taps, t_taps, g_taps = torch.zeros(T, L, 3, 2, **f32), torch.zeros(K, T, L, 2, 2, **f32), torch.zeros(T, L, 2, 2, **f32)
    ckpt = torch.zeros(ops.macro_ckpt_numel(desc, T, 2), **f32)
    target = torch.zeros(T, L, 2, N, **f32)
    six = [torch.zeros(L, N, **f32) for _ in range(4)] + [torch.zeros(K, L, N, **f32) for _ in range(2)]

    def raises(kind, text, call):
        with pytest.raises(kind, match="^" + re.escape(text) + "$"):
            call()

    def fused(**kw):
        return ops.macro_rollout_fwd_jvp(desc, T, z, z, z, z, ghost, tr, tr, **kw)

    def swept(**kw):
        return ops.macro_rollout_jvp(desc, T, kw.pop("tape", z), tr, tr, **kw)
    bad_tg = torch.zeros(K, T, L, 2, 2, **f32)            # a schedule's tangents beside constant boundary cells
    raises(ValueError, "t_ghost must have shape (3, 2, 2, 2): it follows the form of ghost", lambda: fused(t_ghost=bad_tg, det=many))
    raises(ValueError, "det must hold 1..8 cell indices (got 9)", lambda: fused(det=many, out=six[:5]))
    raises(ValueError, "det must be a one-dimensional int32 CUDA tensor", lambda: fused(det=det.long(), taps=taps[1:]))
    raises(ValueError, "taps must be a contiguous float32 CUDA tensor of shape (5, 2, 3, 2)", lambda: fused(det=det, taps=taps[1:], t_taps=t_taps[1:]))
    raises(ValueError, "t_taps must be a contiguous float32 CUDA tensor of shape (3, 5, 2, 2, 2)", lambda: fused(det=det, taps=taps, t_taps=t_taps.double()))
    for kw in (dict(taps=taps), dict(t_taps=t_taps)):
        raises(ValueError, "taps / t_taps without det", lambda: fused(out=six[:5], **kw))
    raises(ValueError, "out must be (r_out, y_out, u_out, ueq_out, t_r_out, t_y_out)", lambda: fused(out=six[:5]))
    raises(ValueError, "t_r_out must be a contiguous float32 CUDA tensor of shape (3, 2, 8)", lambda: fused(out=six[:4] + [six[0], six[0]]))
    raises(ValueError, "u_out must be a contiguous float32 CUDA tensor of shape (2, 8)", lambda: fused(out=six[:2] + [six[2].double()] + six[3:]))
    raises(ValueError, "t_ghost must have shape (3, 2, 2, 2) or (3, 5, 2, 2, 2)", lambda: swept(t_ghost=torch.zeros(K, L, 2, **f32), det=many))
    raises(ValueError, "det must hold 1..8 cell indices (got 9)", lambda: swept(det=many, tape=None))
    raises(ValueError, "t_taps must be a contiguous float32 CUDA tensor of shape (3, 5, 2, 2, 2)", lambda: swept(det=det, t_taps=t_taps[:, 1:], tape=None))
    raises(ValueError, "t_taps without det", lambda: swept(t_taps=t_taps, tape=None))
    raises(ValueError, "a sweep of T > 0 steps needs the rollout's tape", lambda: swept(tape=None, det=det))
    # the checkpointed pair and its target forms
    fwd = lambda **kw: ops.macro_rollout_fwd_ckpt(desc, T, z, z, z, z, ghost, ckpt, segment=2, **kw)      # noqa: E731
    bwd = lambda g_r=z, **kw: ops.macro_rollout_bwd_ckpt(desc, T, ckpt, z, z, z, z, ghost, g_r, z, segment=2, **kw)      # noqa: E731
    raises(ValueError, "det must hold 1..8 cell indices (got 9)", lambda: fwd(det=many, taps=taps[1:]))
    raises(ValueError, "taps must be a contiguous float32 CUDA tensor of shape (5, 2, 3, 2)", lambda: fwd(det=det, taps=taps[1:]))
    raises(ValueError, "det must be a one-dimensional int32 CUDA tensor", lambda: bwd(det=det.long(), g_taps=g_taps[1:]))
    raises(ValueError, "g_taps must have shape (5, 2, 2, 2)", lambda: bwd(g_r=tr, det=det, g_taps=g_taps[1:]))
    raises(ValueError, "g_r and g_y must have shape (2, 8)", lambda: bwd(g_r=tr, det=det, g_taps=g_taps))
    raises(ValueError, "g_r and g_y must have shape (2, 8)", lambda: bwd(g_r=tr))
    fit = lambda **kw: ops.macro_rollout_fwd_ckpt_target(desc, T, z, z, z, z, ghost, ckpt, kw.pop("target", target), segment=2, **kw)      # noqa: E731
    back = lambda g_r=z, **kw: ops.macro_rollout_bwd_ckpt_target(desc, T, ckpt, z, z, z, z, ghost, g_r, z, kw.pop("target", target),      # noqa: E731
                                                                 segment=2, **kw)
    raises(ValueError, "sse must be a contiguous float64 CUDA tensor of shape (2, 2)", lambda: fit(sse=torch.zeros(L, 2, **f32), target=target.cpu()))
    raises(TypeError, "target is not a CUDA tensor", lambda: fit(target=target.cpu()))
    raises(ValueError, "g_r and g_y must have shape (2, 8)", lambda: back(g_r=tr, target=target.cpu()))
    raises(TypeError, "target is not a CUDA tensor", lambda: back(target=target.cpu(), g_ghost=torch.zeros(L, 2, **f32)))
    raises(ValueError, "g_ghost must be a contiguous float64 tensor of shape (2, 2, 2)", lambda: back(g_ghost=torch.zeros(L, 2, **f32)))
    raises(TypeError, "final u must be a float32 CUDA tensor (got torch.float64 on %s)" % z.device,
           lambda: back(g_r=tr, g_sse=torch.zeros(L, 2, dtype=torch.float64, device=cuda), final=(z, z, z.double())))


# ---- 8. the example ----------------------------------------------------------------------------------------------------------------------
def test_fit_pulse_fused_writes_the_taped_run_s_trial_file(cuda, tmp_path):
    """Both runs take --seed 1: the example draws the pulse it hides from torch's generator, and two unseeded runs fit different pulses."""
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    texts = []
    for flags in ([], ["--fused"]):
        cwd = tmp_path / ("fused" if flags else "taped")
        cwd.mkdir()
        out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "fit_pulse.py"), "--method", "lm", "--n_cell", "64",
                              "--n_timestep", "40", "--n_episode", "4", "--seed", "1"] + flags, cwd=str(cwd), env=env, capture_output=True, text=True,
                             timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        files = [os.path.join(dp, f) for dp, _, fs in os.walk(str(cwd)) for f in fs if f.startswith("trial_") and f.endswith(".txt")]
        assert len(files) == 1, files
        texts.append(open(files[0]).read())
    assert len(texts[0].splitlines()) == 4 and texts[0] == texts[1]
