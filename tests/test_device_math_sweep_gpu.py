"""Sweep the device's interface solver and IDM step over a million seeded points per family, at the edge classes of
tests/sweep_inputs.py, against the C oracle's batch entries; adjudicate every disagreement in exact arithmetic (tests/hp_ref.py).

A disagreement is excused only as a tie: a case or clip decision whose margin lies within hp_ref's bound, or a float32 entry that both
sides round from values the bound allows.  Doubles are checked against the exact value on every disagreeing row and on a seeded
sample of each class.  Exceptions are capped per class: a high count is itself a systematic error.  Then the production rollout paths
(pair kernel, lane kernel, step operator; micro rollout kernel at every wave count) must reproduce the batch solver bit for bit.
Needs a real MI355X:  python -m pytest tests -m gpu"""
import numpy as np
import pytest

import hp_ref as H
import sweep_inputs as S

pytestmark = pytest.mark.gpu

N_ARZ = 80_000          # x 14 classes
N_IDM = 92_000          # x 11 classes
SAMPLE = 150            # rows per class whose doubles are checked against the exact value (besides every disagreeing row)
CAP = 2e-3              # ties allowed per class, as a fraction of its rows ...
# ... except in the classes built within a few double ulps of a clip threshold: half of acc_floor's rows sit there, and every row of
# sstar_0 forms s* by cancellation, so its float32 entries that scale with s*^2 have no relative accuracy (they are held to the bound)
CAP_EDGE = {"acc_floor": 0.5, "sstar_0": 1.0}
ARZ32 = ("dL", "dR", "fp")


def _t(a, dev):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device=dev)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def mm(a, b):
    """np.matmul of float32 2x2 blocks as the kernels and the reference form it: acc = a0 b0; acc = fma(a1, b1, acc)."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    o = np.empty_like(a)
    for i in range(2):
        for j in range(2):
            p0 = (a[:, i, 0] * b[:, 0, j]).astype(np.float32).astype(np.float64)
            o[:, i, j] = p0 + a[:, i, 1] * b[:, 1, j]
    return o.astype(np.float32)


def _sub(t, idx):
    return {k: v[idx] for k, v in t.items()}


def _distinct(dev, ref, keys):
    """Float32 exceptions counted once per distinct (entry, value, reference value): one tied quantity of a cell repeats on every row
    that holds the cell, and an edge class draws few distinct cells."""
    seen = set()
    for k in keys:
        a, b = dev[k].reshape(-1, 4), ref[k].reshape(-1, 4)
        i, j = np.nonzero((a != b) & ~(np.isnan(a) & np.isnan(b)))
        seen.update(zip([k] * len(i), j.tolist(), a[i, j].tolist(), b[i, j].tolist()))
    return len(seen)


# An itscp source ghost has y = 0, so d b0 / d r_L = 1 / (2 sqrt(r_L)) + u_eq'(r_L) / u_max cancels exactly: where it meets Q_M or Q_C,
# dL[0] and dL[2] are 0 exactly and every rounding of the noise is within the bound (and Q_M next to a speed 1e-5 away has y_0 ~ 0)
CAP_ARZ_EDGE = {"src_ghost": 0.5}


def _adjudicate_arz(name, inp, dt, dx, dev, ref, rng, report):
    """`dev` (one variant's outputs) against the oracle `ref`: equal, or a tie that hp_ref excuses."""
    n = len(inp)
    diff = dev["case"] != ref["case"]
    for k in ARZ32:
        diff |= np.any(dev[k].reshape(n, -1) != ref[k].reshape(n, -1), axis=1)
    rows = np.union1d(np.flatnonzero(diff), rng.choice(n, SAMPLE, replace=False))
    t_ref = H.arz_table(inp[rows], dt, dx)
    t_dev = H.arz_table(inp[rows], dt, dx, cases=dev["case"][rows])
    d = _sub(dev, rows)
    case_tie = d["case"] != t_ref["case"]
    assert np.all(t_ref["tie"][case_tie]), (name, "case outside its margin", inp[rows][case_tie & ~t_ref["tie"]][:3])
    worst = 0.0
    for k in ("q0", "flux"):
        ok, ratio = H.within64(d[k], t_dev, k)
        assert ok.all(), (name, k, inp[rows][~ok.all(1)][:3])
        worst = max(worst, float(np.nanmax(ratio)))
    for k in ARZ32:
        ok = H.within32(d[k], t_dev, k)
        assert ok.all(), (name, k, inp[rows][~ok.all(1)][:3])
    # the products are np.matmul of the row's own float32 factors
    assert np.array_equal(d["A"], mm(d["fp"], d["dL"])) and np.array_equal(d["B"], mm(d["fp"], d["dR"])), name
    n_case, n_f32 = int(case_tie.sum()), int(diff.sum() - case_tie.sum())
    n_exc = n_case + _distinct(_sub(dev, diff), _sub(ref, diff), ARZ32)
    report.append("%-14s %8d pts  case ties %4d  float32 ties %4d  (%d distinct)  max err %.3f bound"
                  % (name, n, n_case, n_f32, n_exc, worst))
    assert n_exc <= CAP_ARZ_EDGE.get(name, CAP) * n, (name, n_exc)


@pytest.mark.parametrize("variant", [1, 0])
def test_interface_solver_sweep(cuda, oracle, variant):
    """arz_interface_batch variant 1 (IEEE, reference order) and variant 0 (production) against the oracle on 1.12 M interfaces.
    Equal rows need no excuse; on the others every case, double and float32 entry must be one the exact solve allows.  The CFL
    flag must match the reference's assert wherever the exact speed is outside the bound of dx / dt."""
    from dhts import ops
    rng = np.random.default_rng(40 + variant)
    report = []
    for name, inp, dt, dx in S.arz_classes(N_ARZ, seed=variant + 1):
        ref = oracle.arz_batch(inp, dt, dx)
        dev = _np(ops.arz_interface_batch(_t(inp, cuda), dt=dt, dx=dx, variant=variant))
        _adjudicate_arz(name, inp, dt, dx, dev, ref, rng, report)
        # both variants keep the products exact where the factors agree
        same = np.all((dev["dL"] == ref["dL"]) & (dev["dR"] == ref["dR"]) & (dev["fp"] == ref["fp"]), axis=(1, 2))
        assert np.array_equal(dev["A"][same], ref["A"][same]) and np.array_equal(dev["B"][same], ref["B"][same]), name
        cfl = dev["cfl_bad"] != ref["cfl_bad"]
        if cfl.any():
            t = H.arz_table(inp[cfl], dt, dx)
            assert np.all(np.abs(t["cfl_m"]) <= t["cfl_e"]), (name, "CFL flag outside its margin", inp[cfl][:3])
        if variant == 1:
            # the IEEE variant keeps the reference's case logic exactly
            assert np.array_equal(dev["case"], ref["case"]), name
    print("\ninterface solver, variant %d:\n  " % variant + "\n  ".join(report))


@pytest.mark.parametrize("variant", [1, 0])
def test_idm_sweep(cuda, oracle, variant):
    """idm_batch variants 1 and 0 against the oracle on 1.01 M vehicle steps: flags, acc, s*, next_v and both Jacobians, adjudicated
    like the interface solver.  Zero gaps (the Jacobians divide by them) must give the oracle's non-finite values bit for bit, and
    under a settled acceleration clip the next speed is exactly 0 as in the reference."""
    from dhts import ops
    rng = np.random.default_rng(60 + variant)
    report = []
    for name, inp in S.idm_classes(N_IDM, seed=variant + 1):
        n = len(inp)
        ref = oracle.idm_batch(inp)
        dev = _np(ops.idm_batch(_t(inp, cuda), variant=variant))
        assert np.array_equal(dev["collided"], ref["collided"]), name
        flags = lambda o: np.stack([o["clipped_acc"], o["clipped_spacing"]], 1)
        diff = np.any(flags(dev) != flags(ref), axis=1) | (dev["next_v"].astype(np.float32) != ref["next_v"].astype(np.float32))
        for k in ("dEgo", "dLeading"):
            a, b = dev[k].reshape(n, -1), ref[k].reshape(n, -1)
            diff |= np.any((a != b) & ~(np.isnan(a) & np.isnan(b)), axis=1)
        rows = np.union1d(np.flatnonzero(diff), rng.choice(n, SAMPLE, replace=False))
        t_ref = H.idm_table(inp[rows])
        t_dev = H.idm_table(inp[rows], flags=flags(dev)[rows])
        d = _sub(dev, rows)
        for k, tk in (("clipped_acc", "tie_acc"), ("clipped_spacing", "tie_spacing")):
            off = d[k] != t_ref[k]
            assert np.all(t_ref[tk][off]), (name, k, "outside its margin", inp[rows][off & ~t_ref[tk]][:3])
        worst = 0.0
        for k in ("acc", "sstar"):
            ok, ratio = H.within64(d[k], t_dev, k)
            assert ok.all(), (name, k, inp[rows][~ok.reshape(-1)][:3])
            worst = max(worst, float(np.nanmax(ratio)))
        assert H.within32(d["next_v"], t_dev, "next_v").all(), name
        fin = t_dev["finite"]
        for k in ("dEgo", "dLeading"):
            ok = H.within32(d[k][fin], _sub(t_dev, fin), k)
            assert ok.all(), (name, k, inp[rows][fin][~ok.all(1)][:3])
            # a zero gap: the reference's Python floats raise ZeroDivisionError here, the oracle's C gives inf / nan.  The entries
            # that do not divide by the gap must agree; the IEEE variant keeps the oracle's values bit for bit; the production form
            # (no separate spacing-clip formulas) may turn a clipped row's 0 * inf into nan where the oracle has a finite value
            nf = ~fin
            a, b = d[k][nf], ref[k][rows][nf]
            assert np.array_equal(a[:, 0], b[:, 0], equal_nan=True), (name, k, "zero gap")
            if variant == 1:
                assert np.array_equal(a, b, equal_nan=True), (name, k, "zero gap")
            else:
                assert np.all(~np.isfinite(a[:, 1]) | (a[:, 1] == b[:, 1])), (name, k, "zero gap")
        settled_clip = ref["clipped_acc"] & (dev["clipped_acc"] == ref["clipped_acc"])
        assert np.all(dev["next_v"][settled_clip] == 0.0), (name, "a clipped vehicle must stop at exactly 0")
        zero = ~t_dev["finite"]
        n_exc = int(diff.sum()) - int(np.isin(np.flatnonzero(diff), rows[zero]).sum())
        ties = int((t_ref["tie_acc"] | t_ref["tie_spacing"]).sum())
        report.append("%-10s %8d pts  exceptions %5d  (clip ties %5d, zero-gap rows %5d)  max err %.3f bound"
                      % (name, n, n_exc, ties, int(zero.sum()), worst))
        assert n_exc <= CAP_EDGE.get(name, CAP) * n, (name, n_exc)
    print("\nIDM, variant %d:\n  " % variant + "\n  ".join(report))


def _lanes(rng, L, N, um):
    """Float32 lanes whose cells come from the sweep's edge values: vacuum, the neighbours of float32(eps), jams, equal speeds."""
    r = rng.uniform(0.0, 1.0, (L, N))
    u = rng.uniform(0.0, um, (L, N))
    pick = rng.integers(0, 8, (L, N))
    r = np.where(pick == 0, 0.0, r)
    r = np.where(pick == 1, S.nudge32(np.full((L, N), S.EPS32), rng.integers(-2, 3, (L, N))), r)
    r = np.where(pick == 2, rng.uniform(0.97, 1.0, (L, N)), r)
    u = np.where((pick == 3) | (pick == 0) & (rng.random((L, N)) < 0.5), np.roll(u, 1, axis=1), u)   # the left neighbour's speed
    u = np.where(pick == 4, np.roll(u, 1, axis=1) - rng.uniform(0, 1, (L, N)), u)                     # a hair slower than it
    dense = rng.random(L) < 0.5                                   # half the lanes hold no near-empty cell at all
    r[dense] = rng.uniform(0.02, 1.0, (int(dense.sum()), N))
    return S.cell(r, u, um)


def _step_from_batch(ops, dev, cells, ghost, dt, dx, um):
    """One step of every lane rebuilt from the batch solver (variant 0): new (r, y) = float32(x + (F_left - F_right) dt / dx), and
    the reference's three blocks per cell (dmacro_lane.py:56, the assembly of oracle_macro_step) from the interfaces' A and B."""
    L, N = cells[0].shape
    full = [np.concatenate([ghost[:, 0:1, j], cells[j], ghost[:, 1:2, j]], 1) for j in range(4)]     # [L][N+2]
    inp = np.stack([full[j][:, :-1] for j in range(4)] + [full[j][:, 1:] for j in range(4)] + [np.full((L, N + 1), um)], 2)
    b = _np(ops.arz_interface_batch(_t(inp.reshape(-1, 9), dev), dt=dt, dx=dx, variant=0))
    fl = b["flux"].reshape(L, N + 1, 2)
    c = dt / dx
    nr = (cells[0] + (fl[:, :-1, 0] - fl[:, 1:, 0]) * c).astype(np.float32)
    ny = (cells[1] + (fl[:, :-1, 1] - fl[:, 1:, 1]) * c).astype(np.float32)
    A, B = b["A"].reshape(L, N + 1, 4), b["B"].reshape(L, N + 1, 4)
    cf, ncf = np.float32(c), np.float32(-c)
    eye = np.array([1, 0, 0, 1], np.float32)
    d0 = ncf * (-A[:, :-1])
    d1 = eye - cf * (A[:, 1:] - B[:, :-1])
    d2 = ncf * B[:, 1:]
    return nr, ny, np.stack([d0, d1, d2], 2)                      # [L][N][3][4]


@pytest.mark.parametrize("N,group", [(128, 1), (256, 2), (512, 4)])
def test_macro_paths_equal_the_batch_solver(cuda, N, group):
    """One step through the pair kernel (full lanes of 128 W cells, 1, 2 or 4 lanes per workgroup), the lane kernel
    (DHTS_OPT_MACRO_FWD_VARIANT = 2) and the step operator: the new (r, y) and every block of the expanded tape must be what the batch
    solver's fluxes and products give, bit for bit.  Lanes with vacuum, float32(eps) neighbours and jams put interfaces on the
    queued phase-2 path and the dense phase-1 form; half the lanes hold no near-empty cell."""
    import torch
    from dhts import _lib, ops
    rng = np.random.default_rng(900 + N)
    L, dt, dx, um = 128 * group, 0.01, 5.0, 30.0
    cells = _lanes(rng, L, N, um)
    gcell = S.cell(rng.uniform(0, 1, (L, 2)), rng.uniform(0, um, (L, 2)), um)
    ghost = np.stack(gcell, 2).astype(np.float32)                 # [L][2][4]
    nr, ny, blocks = _step_from_batch(ops, cuda, cells, ghost.astype(np.float64), dt, dx, um)
    planes = [_t(c.astype(np.float32), cuda) for c in cells]
    g = _t(ghost, cuda)
    desc = ops.macro_desc(L, N, dt, dx, um)
    try:
        for variant, grp, kernel in ((0, group, 2), (2, 1, 0)):
            assert _lib.lib().dhts_set_option(_lib.OPT_MACRO_FWD_VARIANT, variant) == 0
            assert _lib.lib().dhts_set_option(_lib.OPT_MACRO_FWD_GROUP, grp) == 0
            assert ops.macro_rollout_plan(desc, 1)["fwd_kernel"] == kernel
            tape = torch.full((ops.macro_tape_numel(desc, 1),), float("nan"), device=cuda)
            out = ops.macro_rollout_fwd(desc, 1, *planes, g, tape=tape)
            assert np.array_equal(out[0].cpu().numpy(), nr) and np.array_equal(out[1].cpu().numpy(), ny), (variant, grp)
            ex = ops.macro_tape_expand(desc, 1, tape).cpu().numpy().reshape(L, 3, -1, 4)[:, :, :N]
            assert np.array_equal(ex.transpose(0, 2, 1, 3), blocks), (variant, grp)
    finally:
        _lib.lib().dhts_set_option(_lib.OPT_MACRO_FWD_GROUP, 0)
        _lib.lib().dhts_set_option(_lib.OPT_MACRO_FWD_VARIANT, 0)
    stape = torch.zeros(ops.macro_step_tape_numel(desc), device=cuda)
    out = ops.macro_step_fwd(desc, *planes, g, tape=stape)
    assert np.array_equal(out[0].cpu().numpy(), nr) and np.array_equal(out[1].cpu().numpy(), ny)
    Np = (N + 63) // 64 * 64
    st = stape.cpu().numpy().reshape(L, 3, Np, 4)[:, :, :N].transpose(0, 2, 1, 3)
    assert np.array_equal(st, blocks)


@pytest.mark.parametrize("waves", [0, 1, 2, 4])
def test_micro_rollout_step_equals_idm_batch(cuda, waves):
    """One step of the micro rollout kernel (wave count forced to 1, 2, 4, and 0 = the default the benchmark runs) on lanes whose head
    gaps are the sweep's gap values: the head vehicles' next speed must be idm_batch variant 0's bit for bit, and so must every
    follower's (its gap and speed difference recomputed as the lane computes them)."""
    import torch
    from dhts import _lib, ops
    rng = np.random.default_rng(70 + waves)
    L, V = 2048, 256
    gaps = np.concatenate([inp[:, 4] for _, inp in S.idm_classes(L // 8, seed=5) if _ in ("default", "gap_eps", "gap_1000", "acc_floor",
                                                                                        "sstar_0", "v0", "rv", "fast")])[:L]
    head_dv = np.concatenate([inp[:, 5] for _, inp in S.idm_classes(L // 8, seed=5) if _ in ("default", "gap_eps", "gap_1000", "acc_floor",
                                                                                          "sstar_0", "v0", "rv", "fast")])[:L]
    P = np.asarray(S.DEFAULT + (5.0,))
    params = np.broadcast_to(P[:, None, None], (6, L, V)).copy()
    p = np.cumsum(rng.uniform(6.0, 40.0, (L, V)), 1).astype(np.float32)
    v = rng.uniform(0, 30, (L, V)).astype(np.float32)
    head = np.stack([gaps, head_dv], 1)
    dt = 0.05
    desc = ops.micro_desc(L, V, dt)
    try:
        assert _lib.lib().dhts_set_option(_lib.OPT_MICRO_FWD_WAVES, waves) == 0
        out = ops.micro_rollout_fwd(desc, 1, _t(p, cuda), _t(v, cuda), _t(params, cuda), _t(head, cuda))
    finally:
        _lib.lib().dhts_set_option(_lib.OPT_MICRO_FWD_WAVES, 0)
    nv = out[1].cpu().numpy()
    pd, vd = p.astype(np.float64), v.astype(np.float64)
    dp = np.concatenate([np.abs(pd[:, 1:] - pd[:, :-1]) - 5.0, gaps[:, None]], 1)
    dv = np.concatenate([vd[:, :-1] - vd[:, 1:], head_dv[:, None]], 1)
    inp = np.stack([np.full((L, V), P[0]), np.full((L, V), P[1]), vd, np.full((L, V), P[2]), dp, dv, np.full((L, V), P[3]),
                    np.full((L, V), P[4]), np.full((L, V), dt)], 2).reshape(-1, 9)
    b = ops.idm_batch(_t(inp, cuda), variant=0)
    assert np.array_equal(nv.reshape(-1), b["next_v"].cpu().numpy().astype(np.float32))
