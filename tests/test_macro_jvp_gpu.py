"""Forward-mode tangent sweep of the fused ARZ rollout on the GPU (dhts_macro_rollout_jvp and dhts.macro_rollout_jvp): both kernels and
every number of directions per launch, on tapes of every forward kernel family, with constant boundary cells and with a schedule --
against the float64 chain of tests/macro_jvp_ref.py on the oracle's blocks and on the device's own, bit for bit against each other, by
the dot-product identity against the reverse sweep of the same tape; memory and index safety at the raw operator; primal parity; the
fault record; the example.  Shapes are the smallest that reach each plan entry and each wavefront boundary; every T <= 12."""
import os
import subprocess
import sys

import numpy as np
import pytest

import macro_jvp_ref as J
import macro_sched_ref as R
from util import TOL_GRAD, grad_report, options

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, DX, UM = 0.01, 5.0, 30.0
GENERAL, FAST = 0, 1                     # plan: kernel
KMAX = 5


def edges(N):
    """Cells 0 and N - 1 and both sides of every wavefront boundary."""
    return sorted({0, N - 1} | {c for b in range(64, N, 64) for c in (b - 1, b)})


# id: (L, N, T, forward variant, forward group, detectors, K of the operator-level checks, kernel, block)
CASES = {
    # the fast kernel on lane-kernel tapes
    "fast2": (3, 2, 7, 0, 0, [0, 1], 3, FAST, 64),
    "fast63": (2, 63, 5, 0, 0, edges(63), 5, FAST, 64),
    "fast64": (2, 64, 1, 0, 0, edges(64), 1, FAST, 64),
    "fast65": (2, 65, 12, 0, 0, edges(65), 4, FAST, 128),
    "fast65_onephase": (2, 65, 2, 1, 0, edges(65), 2, FAST, 128),          # every interface an exception: more of them than N = 64 + 1
    "fast64_onephase": (2, 64, 5, 1, 0, edges(64), 3, FAST, 64),           # ... and more than threads (65 > 64)
    "fast130": (2, 130, 5, 0, 0, edges(130), 2, FAST, 256),
    "fast300": (2, 300, 2, 0, 0, edges(300), 5, FAST, 512),
    "fast1000": (1, 1000, 2, 0, 0, edges(1000), 3, FAST, 1024),
    # ... on tapes the pair kernel wrote (other order of the exception lists), one and four lanes per workgroup
    "pair128_g1": (4, 128, 5, 0, 1, edges(128), 4, FAST, 128),
    "pair128_g4": (4, 128, 2, 0, 4, edges(128), 5, FAST, 128),
    "pair256_g1": (4, 256, 12, 0, 1, edges(256), 2, FAST, 256),
    "pair256_g4": (4, 256, 1, 0, 4, edges(256), 3, FAST, 256),
    # the general kernel
    "gen1": (3, 1, 5, 0, 0, [0], 5, GENERAL, 64),
    "gen1026": (1, 1026, 2, 0, 0, edges(1026), 3, GENERAL, 512),
    "gen2100": (1, 2100, 2, 0, 0, edges(2100), 4, GENERAL, 512),
    # T = 0: nothing to sweep
    "fast64_t0": (2, 64, 0, 0, 0, [3], 2, GENERAL, 64),
}
BOTH = [False, True]                     # constant boundary cells / a schedule
WIDEST = {1: 1, 2: 2, 3: 4, 4: 4, 5: 4}          # (three directions ride in a launch of four with one slot masked)
LAUNCHES = {1: 1, 2: 1, 3: 1, 4: 1, 5: 2}


class jvp_variant:
    """DHTS_OPT_MACRO_JVP_VARIANT for the length of a with-block."""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        from dhts import _lib
        assert _lib.lib().dhts_set_option(_lib.OPT_MACRO_JVP_VARIANT, self.v) == 0

    def __exit__(self, *exc):
        from dhts import _lib
        _lib.lib().dhts_set_option(_lib.OPT_MACRO_JVP_VARIANT, 0)


def check_plan(case, det=None):
    from dhts import ops
    L, N, T, _, _, cdet, _, kernel, block = CASES[case]
    desc = ops.macro_desc(L, N, DT, DX, UM)
    for K in range(1, KMAX + 1):
        p = ops.macro_jvp_plan(desc, T, K, len(cdet if det is None else det))
        assert p == dict(kernel=kernel, block=block, dirs_per_launch=WIDEST[K], launches=LAUNCHES[K] if T else 0), (case, K, p)


def inputs(case, sched):
    """tests/test_macro_sched_gpu.py's recipe (as tests/test_macro_taps_gpu.py draws it)."""
    L, N, T = CASES[case][:3]
    rng = np.random.default_rng(sum(map(ord, case)))
    r0 = rng.uniform(0.05, 0.95, (L, N)).astype(np.float32)
    u0 = rng.uniform(0.0, UM if T > 0 else 0.25, (L, N)).astype(np.float32)
    gr = rng.uniform(0.05, 0.95, (T, L, 2)).astype(np.float32)
    gu = rng.uniform(0.0, UM, (T, L, 2)).astype(np.float32)
    if T >= 2:
        gr[T // 2, 0, 0] = 3e-6
        gr[T - 1, L - 1, 1] = 0.0
        gr[0, 0, 1] = 8e-6
    cr = rng.uniform(0.05, 0.95, (L, 2)).astype(np.float32)
    cu = rng.uniform(0.0, UM, (L, 2)).astype(np.float32)
    return (r0, u0, gr, gu) if sched else (r0, u0, cr, cu)


def leaf_tangents(case, sched):
    """KMAX directions of tangents of the four leaves."""
    L, N, T = CASES[case][:3]
    rng = np.random.default_rng(2000 + sum(map(ord, case)))
    gshape = (KMAX, T, L, 2) if sched else (KMAX, L, 2)
    return (rng.standard_normal((KMAX, L, N)).astype(np.float32), rng.standard_normal((KMAX, L, N)).astype(np.float32),
            rng.standard_normal(gshape).astype(np.float32), rng.standard_normal(gshape).astype(np.float32))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---- (a), (f): the operator against the oracle chain, and its primal outputs -----------------------------------------------------------
_oracle_chain = {}


def oracle_chain(oracle, case, sched):
    key = (case, sched)
    if key not in _oracle_chain:
        T = CASES[case][2]
        r0, u0, gr, gu = inputs(case, sched)
        if not sched:
            gr, gu = np.tile(gr[None], (T, 1, 1)), np.tile(gu[None], (T, 1, 1))
        _oracle_chain[key] = R.sched_fwd(oracle, r0, u0, gr, gu, DT, DX, UM)
    return _oracle_chain[key]


@pytest.mark.parametrize("sched", BOTH, ids=["const", "sched"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_operator_against_the_oracle_chain_and_primal_parity(cuda, oracle, case, sched):
    import torch
    import dhts
    L, N, T, variant, group, det, K = CASES[case][:7]
    leaves = [torch.tensor(a, device=cuda) for a in inputs(case, sched)]
    tans = [torch.tensor(a[:K], device=cuda) for a in leaf_tangents(case, sched)]
    with options(variant, group):
        check_plan(case)
        primal, tang = dhts.macro_rollout_jvp(*leaves, T, DT, DX, UM, t_r0=tans[0], t_u0=tans[1], t_ghost_r=tans[2], t_ghost_u=tans[3],
                                              detectors=det)
        plain, tang_plain = dhts.macro_rollout_jvp(*leaves, T, DT, DX, UM, t_r0=tans[0], t_u0=tans[1], t_ghost_r=tans[2],
                                                   t_ghost_u=tans[3])
        ref = dhts.macro_rollout(*leaves, T, DT, DX, UM, detectors=det)
        ref_plain = dhts.macro_rollout(*leaves, T, DT, DX, UM)
    # (f) the primal outputs are dhts.macro_rollout's, bit for bit
    assert len(primal) == 5 and len(ref) == 5 and len(plain) == 4 and len(tang) == 4 and len(tang_plain) == 3
    for a, b in list(zip(primal, ref)) + list(zip(plain, ref_plain)):
        assert torch.equal(a, b)
    assert all(not t.requires_grad for t in tang)
    # the tangents without readings are those with readings
    for a, b in zip(tang_plain, tang):
        assert torch.equal(a, b)
    assert tuple(tang[0].shape) == (K, L, N) and tuple(tang[3].shape) == (K, T, L, 3, len(det))
    # (a) each output group on its own, direction by direction
    f = oracle_chain(oracle, case, sched)
    tn = leaf_tangents(case, sched)
    for i in range(K):
        t_gr, t_gu = (tn[2][i], tn[3][i]) if sched else (np.tile(tn[2][i][None], (T, 1, 1)), np.tile(tn[3][i][None], (T, 1, 1)))
        o = J.jvp(f, t_r0=tn[0][i], t_u0=tn[1][i], t_gr=t_gr, t_gu=t_gu, det=det)
        for j, k in enumerate(("t_rT", "t_yT", "t_uT")):
            assert np.abs(o[k]).max() > 0
            assert grad_report("%s %s direction %d %s" % (case, "sched" if sched else "const", i, k), tang[j][i].cpu().numpy(), o[k]) <= TOL_GRAD
        if T:
            assert np.abs(o["t_read"]).max() > 0
            assert grad_report("%s direction %d t_readings" % (case, i), tang[3][i].cpu().numpy(), o["t_read"]) <= TOL_GRAD


# ---- at the raw operator ---------------------------------------------------------------------------------------------------------------
GUARD, SENTINEL = 257, 12345.0
_forward = {}


def forward(cuda, case, sched, lanes=None):
    """One forward launch per (case, form, lanes): the tape, the device's own blocks and the raw tangents of KMAX directions."""
    import torch
    from dhts import ops
    key = (case, sched, None if lanes is None else tuple(lanes))
    if key in _forward:
        return _forward[key]
    L, N, T, variant, group = CASES[case][:5]
    r0, u0, gr, gu = inputs(case, sched)
    rng = np.random.default_rng(3000 + sum(map(ord, case)))
    t_r, t_y = rng.standard_normal((2, KMAX, L, N)).astype(np.float32)
    t_g = rng.standard_normal((KMAX, T, L, 2, 2) if sched else (KMAX, L, 2, 2)).astype(np.float32)
    if lanes is not None:
        r0, u0, t_r, t_y = r0[lanes], u0[lanes], t_r[:, lanes], t_y[:, lanes]
        gr, gu, t_g = (gr[:, lanes], gu[:, lanes], t_g[:, :, lanes]) if sched else (gr[lanes], gu[lanes], t_g[:, lanes])
        L = len(lanes)
    desc = ops.macro_desc(L, N, DT, DX, UM)
    r, u = torch.tensor(r0, device=cuda), torch.tensor(u0, device=cuda)
    y, q = ops.macro_state_from_ru(r, u, UM)
    tr, tu = torch.tensor(gr, device=cuda), torch.tensor(gu, device=cuda)
    gy, gq = ops.macro_state_from_ru(tr, tu, UM) if tr.numel() else (tr.clone(), tr.clone())
    ghost = torch.stack([tr, gy, tu, gq], dim=-1).contiguous()
    tape = torch.zeros(max(ops.macro_tape_numel(desc, T), 1), dtype=torch.float32, device=cuda)
    err = ops.new_error_record(cuda)
    with options(variant, group):
        fwd = ops.macro_rollout_fwd_sched if sched else ops.macro_rollout_fwd
        fwd(desc, T, r, y, u, q, ghost, tape=tape, err=err)
    assert err.tolist()[0] == 0, err.tolist()
    blocks = None
    if T:
        dqs = ops.macro_tape_expand(desc, T, tape).cpu().numpy()                       # [T][L][3][Np][4]
        blocks = dqs[:, :, :, :N].transpose(1, 0, 3, 2, 4).reshape(L, T, N, 3, 2, 2)
    _forward[key] = dict(desc=desc, tape=tape, blocks=blocks, t_r=t_r, t_y=t_y, t_g=t_g, L=L)
    return _forward[key]


def sweep(cuda, case, sched, dirs, general=False, lanes=None, det=None, ghost=True, poison=None):
    """One call of the raw operator on the directions `dirs` of the case's tangents.  Outputs and readings lie in the middle of larger
    buffers: NaN where they belong, a sentinel on both sides."""
    import torch
    from dhts import ops
    fw = forward(cuda, case, sched, lanes)
    N, T = CASES[case][1:3]
    det = CASES[case][5] if det is None else det
    L, K, D = fw["L"], len(dirs), len(det)
    t_r, t_y = fw["t_r"][dirs].copy(), fw["t_y"][dirs].copy()
    if poison is not None:
        t_r[poison] = np.nan
    n_s, n_t = K * L * N, K * T * L * 2 * D
    bufs = [torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=cuda) for n in (n_s, n_s, n_t)]
    views = [b[GUARD:GUARD + n] for b, n in zip(bufs, (n_s, n_s, n_t))]
    for v in views:
        v.fill_(float("nan"))
    out = (views[0].view(K, L, N), views[1].view(K, L, N))
    taps = views[2].view(K, T, L, 2, D)
    err = ops.new_error_record(cuda)
    with jvp_variant(1 if general else 0):
        if not general:
            check_plan(case, det)
        res = ops.macro_rollout_jvp(fw["desc"], T, fw["tape"] if T else None, torch.tensor(t_r, device=cuda), torch.tensor(t_y, device=cuda),
                                    t_ghost=torch.tensor(fw["t_g"][dirs] * (0 if ghost == "zero" else 1), device=cuda) if ghost else None,
                                    det=torch.tensor(det, dtype=torch.int32, device=cuda), err=err, out=out, t_taps=taps)
    assert res[0].data_ptr() == out[0].data_ptr() and res[2].data_ptr() == taps.data_ptr()
    for b, n in zip(bufs, (n_s, n_s, n_t)):
        h = b.cpu().numpy()
        assert np.all(h[:GUARD] == SENTINEL) and np.all(h[GUARD + n:] == SENTINEL), "a store beside the outputs"
    return dict(t_r=out[0].cpu().numpy(), t_y=out[1].cpu().numpy(), taps=taps.cpu().numpy(), err=err.tolist())


ALL = list(range(KMAX))


@pytest.mark.parametrize("sched", BOTH, ids=["const", "sched"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_raw_sweep_bits_chain_and_dot_product(cuda, case, sched):
    """(b) against the float64 chain on the device's own blocks; (c) the fast kernel equals the general one, direction i of a K-direction
    call equals a K = 1 call of it for every K, two runs give the same bits; (d) <g, J t> = <J^T g, t> with the reverse sweep of the same
    tape; (e) every element written (sweep() prefills with NaN and looks at the guard bands)."""
    import torch
    from dhts import ops
    L, N, T, _, _, det = CASES[case][:6]
    a = sweep(cuda, case, sched, ALL)
    assert a["err"] == [0, 0, 0, 0]
    for k in ("t_r", "t_y", "taps"):
        assert not np.isnan(a[k]).any(), "%d elements of %s were not written" % (int(np.isnan(a[k]).sum()), k)
    # (c)
    again, gen = sweep(cuda, case, sched, ALL), sweep(cuda, case, sched, ALL, general=True)
    for k in ("t_r", "t_y", "taps"):
        assert same_bits(a[k], again[k]), "two runs, %s" % k
        assert same_bits(a[k], gen[k]), "fast and general kernel, %s" % k
    for K in range(1, KMAX):                                   # K directions taken from the END of the five: other places in other launches
        part = sweep(cuda, case, sched, ALL[KMAX - K:])
        for k in ("t_r", "t_y", "taps"):
            assert same_bits(part[k], a[k][KMAX - K:]), "K = %d, %s" % (K, k)
    for i in ALL[:-1]:                                         # (the last one alone was K = 1 above)
        one = sweep(cuda, case, sched, [i])
        for k in ("t_r", "t_y", "taps"):
            assert same_bits(one[k][0], a[k][i]), "direction %d alone, %s" % (i, k)
    fw = forward(cuda, case, sched)
    if T == 0:
        assert same_bits(a["t_r"], fw["t_r"]) and same_bits(a["t_y"], fw["t_y"])
        return
    # (b)
    for i in ALL:
        ref = [J.chain(fw["blocks"][l], fw["t_r"][i, l], fw["t_y"][i, l], fw["t_g"][i][:, l] if sched else [fw["t_g"][i, l]] * T, det)
               for l in range(L)]
        for j, k in enumerate(("t_r", "t_y")):
            assert grad_report("%s direction %d %s" % (case, i, k), a[k][i], np.stack([x[j] for x in ref])) <= TOL_GRAD
        assert grad_report("%s direction %d taps" % (case, i), a["taps"][i], np.stack([x[2] for x in ref], axis=1)) <= TOL_GRAD
    # (d)
    rng = np.random.default_rng(7)
    g_r, g_y = rng.standard_normal((2, L, N)).astype(np.float32)
    g_t = rng.standard_normal((T, L, 2, len(det))).astype(np.float32)
    err = ops.new_error_record(cuda)
    g_r0, g_y0, g_ghost = ops.macro_rollout_bwd_taps(fw["desc"], T, fw["tape"], torch.tensor(g_r, device=cuda), torch.tensor(g_y, device=cuda),
                                                     torch.tensor(det, dtype=torch.int32, device=cuda), torch.tensor(g_t, device=cuda),
                                                     sched=sched, err=err)
    assert err.tolist()[0] == 0
    g_r0, g_y0, g_ghost = (x.cpu().numpy().astype(np.float64) for x in (g_r0, g_y0, g_ghost))
    for i in ALL:
        left = [g_r.astype(np.float64) * a["t_r"][i], g_y.astype(np.float64) * a["t_y"][i], g_t.astype(np.float64) * a["taps"][i]]
        right = [g_r0 * fw["t_r"][i], g_y0 * fw["t_y"][i], g_ghost * fw["t_g"][i]]
        lhs, rhs = sum(float(x.sum()) for x in left), sum(float(x.sum()) for x in right)
        scale = sum(float(np.abs(x).sum()) for x in left)
        print("%s direction %d: <g, J t> = %.9g, <J^T g, t> = %.9g, |d| / sum |products| = %.2e" % (case, i, lhs, rhs, abs(lhs - rhs) / scale))
        assert abs(lhs - rhs) <= TOL_GRAD * scale


@pytest.mark.parametrize("case", ["fast65", "pair128_g4", "gen1026"])
def test_null_boundary_tangents_are_zero_ones(cuda, case):
    a, b = sweep(cuda, case, False, ALL, ghost=False), sweep(cuda, case, False, ALL, ghost="zero")
    for k in ("t_r", "t_y", "taps"):
        assert same_bits(a[k], b[k]), k


@pytest.mark.parametrize("sched", BOTH, ids=["const", "sched"])
@pytest.mark.parametrize("case", ["fast65", "fast130", "pair128_g4", "gen1"])
def test_lanes_are_independent(cuda, case, sched):
    """(e) permuting the lanes permutes the results, bit for bit."""
    L = CASES[case][0]
    perm = list(range(L))[::-1]
    a, b = sweep(cuda, case, sched, ALL), sweep(cuda, case, sched, ALL, lanes=perm)
    assert same_bits(a["t_r"][:, perm], b["t_r"]) and same_bits(a["t_y"][:, perm], b["t_y"]) and same_bits(a["taps"][:, :, perm], b["taps"])


@pytest.mark.parametrize("general", [False, True], ids=["heuristic", "general"])
@pytest.mark.parametrize("case", ["fast65", "pair128_g1", "gen1026"])
def test_an_index_outside_the_lane_writes_nothing(cuda, case, general):
    """(e) an entry outside [0, N) is compared away before any address is formed: its column stays as it was, the others are those of a
    run without it."""
    N = CASES[case][1]
    good = sweep(cuda, case, True, ALL, general=general, det=[2, N - 1])
    a = sweep(cuda, case, True, ALL, general=general, det=[2, N - 1, N, N + 70000, -5])
    assert same_bits(a["taps"][..., :2], good["taps"])
    assert np.isnan(a["taps"][..., 2:]).all()
    assert same_bits(a["t_r"], good["t_r"]) and same_bits(a["t_y"], good["t_y"])


@pytest.mark.parametrize("general", [False, True], ids=["heuristic", "general"])
@pytest.mark.parametrize("case", ["fast65", "pair256_g1", "gen1026"])
def test_a_nan_tangent_is_on_record_with_its_lane_and_step_0(cuda, case, general):
    """(g) a NaN in one entry of the initial tangent reaches the cell and its neighbours in step 0."""
    from dhts import _lib
    L, N = CASES[case][:2]
    lane, cell = L - 1, N // 2
    a = sweep(cuda, case, False, [0, 1, 2], general=general, poison=(1, lane, cell))
    assert a["err"][:3] == [_lib.FAULT_NAN, 0, lane] and abs(a["err"][3] - cell) <= 1, a["err"]
    assert np.isfinite(a["t_r"][[0, 2]]).all() and np.isnan(a["t_r"][1, lane]).any()         # the other directions and lanes stay clean
    assert np.isfinite(a["t_r"][1, :lane]).all()


# ---- (h) the example -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["lm", "adam"])
def test_fit_pulse_example_lowers_its_loss(cuda, tmp_path, method):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "fit_pulse.py"), "--n_cell", "64", "--n_timestep", "60",
                          "--n_episode", "6", "--n_lane", "2", "--seed", "1", "--method", method], cwd=str(tmp_path), env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    files = [os.path.join(dp, f) for dp, _, fs in os.walk(str(tmp_path)) for f in fs if f == "trial_0.txt"]
    assert len(files) == 1, files
    losses = [float(line.split()[-1]) for line in open(files[0]).read().splitlines() if line.strip()]
    print("fit_pulse %s loss: first %.6g, last %.6g over %d iterations" % (method, losses[0], losses[-1], len(losses)))
    assert len(losses) == 6 and losses[0] > 0 and losses[-1] < losses[0]
