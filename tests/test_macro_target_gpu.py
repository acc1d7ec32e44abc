"""The dense-fit loss inside the checkpointed macro rollout on the GPU (dhts_macro_rollout_fwd_ckpt_target / _bwd_ckpt_target and
dhts.macro_rollout with `target`): number for number the taped want_hist=True call fed the dense cotangent G = 2 g (H - target) -- states
bit for bit, all four gradients np.array_equal, sse to the rounding of a double sum and the same bits at every segment --, the forward
without a leaf that requires grad, the memory of a long horizon, the chained oracle, the raw entry points, the example.  Shapes and leaves
are tests/test_macro_ckpt_gpu.py's RUNS (tests/test_macro_taps_gpu.py's CASES): 1 to 1000 cells, one and two passes, short last segments,
the pair kernel on the taped side, T = 0."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

import macro_sched_ref as R
from test_macro_ckpt_gpu import BOTH, GUARD, RUNS, SENTINEL, guarded, leaves_of, same_bits, shape, untouched
from test_macro_taps_gpu import CASES, DT, DX, UM, ghost_quads
from util import TOL_GRAD, TOL_STATE, grad_report, options, state_report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAN = F("nan")


@pytest.fixture(scope="module", autouse=True)
def device_memory_as_found():
    yield
    _taped.clear()
    gc.collect()


def plan_of(run):
    from dhts import ops
    _, L, N, T, _ = shape(run)
    return ops.macro_ckpt_target_plan(ops.macro_desc(L, N, DT, DX, UM), T)


def fits(run):
    return plan_of(run)["max_segment"] >= 1


ALL = sorted(r for r in RUNS)          # (every lane of RUNS is below the target plan's limit: asserted in test_every_run_fits)


def test_every_run_fits():
    assert all(fits(run) for run in ALL) and max(shape(run)[2] for run in ALL) == 1000


def segments(run):
    """1, 2, the target plan's, its max_segment, the smallest that does not divide T, one beyond T -- wherever max_segment allows."""
    T = shape(run)[3]
    plan = plan_of(run)
    mx = plan["max_segment"]
    odd = [s for s in range(2, 8) if T % s]
    want = {1, 2, plan["segment"], mx, T + 3} | set(odd[:1])
    return [True] + sorted(s for s in want if 1 <= s <= mx)


def weights_of(run):
    """c float64 [L][2], the weights of sse; wf float32 [2][L][N], those of (rT, uT)."""
    _, L, N, _, _ = shape(run)
    rng = np.random.default_rng(2000 + sum(map(ord, run)))
    return rng.uniform(0.5, 1.5, (L, 2)) * rng.choice([-1.0, 1.0], (L, 2)), rng.standard_normal((2, L, N)).astype(F)


_taped = {}


def taped_history(cuda, run, sched):
    """The history [T][L][3][N] of the taped want_hist=True call (numpy), once per (run, sched): the targets are cut from it."""
    import torch
    import dhts
    key = (run, sched)
    if key not in _taped:
        case, L, N, T, _ = shape(run)
        variant, group = CASES[case][3:5]
        leaves = [torch.tensor(a, device=cuda) for a in leaves_of(run, sched)]
        with options(variant, group):
            _taped[key] = dhts.macro_rollout(*leaves, T, DT, DX, UM, want_hist=True)[4].cpu().numpy()
    return _taped[key]


def target_of(cuda, run, sched, kind, S=1):
    """The observed field [T][L][2][N]: the taped history's density and speed plus noise, with the NaN pattern of `kind`."""
    _, L, N, T, _ = shape(run)
    H = taped_history(cuda, run, sched)
    rng = np.random.default_rng(3000 + sum(map(ord, run)) + int(sched))
    tgt = np.stack([H[:, :, 0], H[:, :, 2]], axis=2) + rng.standard_normal((T, L, 2, N)).astype(F) * F([0.05, 1.0])[None, None, :, None]
    tgt = np.ascontiguousarray(tgt, F)
    if kind == "all_nan":
        tgt[:] = NAN
    elif kind == "rows":                  # whole rows at s0 - 1, s0, s1 - 1 of the second segment, and T - 1
        for t in (S - 1, S, 2 * S - 1, T - 1):
            if 0 <= t < T:
                tgt[t] = NAN
    elif kind == "last_only":
        tgt[:max(T - 1, 0)] = NAN
    elif kind == "entries":
        tgt[rng.random(tgt.shape) < 0.3] = NAN
    elif kind == "no_speed":
        tgt[:, :, 1] = NAN
    else:
        assert kind == "dense"
    return tgt


KINDS = ("dense", "all_nan", "rows", "last_only", "entries", "no_speed")


def yardstick(cuda, run, sched, tgt):
    """The taped want_hist=True call with the loss (hist * G3).sum() + (rT * wf0).sum() + (uT * wf1).sum(), G3 = the dense cotangent
    where(isnan(target), 0, (2 c).float() * (H - target)) in the density and speed planes and 0 in the y plane; and the float64 sum of its
    own float32 residuals squared."""
    import torch
    import dhts
    case, L, N, T, _ = shape(run)
    variant, group = CASES[case][3:5]
    c, wf = weights_of(run)
    wf = torch.tensor(wf, device=cuda)
    g2 = (2.0 * torch.tensor(c, device=cuda)).float()
    t = torch.tensor(tgt, device=cuda)
    leaves = [torch.tensor(a, device=cuda, requires_grad=True) for a in leaves_of(run, sched)]
    with options(variant, group):
        out = dhts.macro_rollout(*leaves, T, DT, DX, UM, want_hist=True)
        H = out[4].detach()
        G3 = torch.zeros_like(H)
        res = []
        for plane, col in ((0, 0), (2, 1)):
            d = H[:, :, plane] - t[:, :, col]
            G3[:, :, plane] = torch.where(torch.isnan(t[:, :, col]), torch.zeros_like(d), g2[None, :, col, None] * d)
            res.append(torch.where(torch.isnan(t[:, :, col]), torch.zeros_like(d), d))
        loss = (out[4] * G3).sum() + (out[0] * wf[0]).sum() + (out[2] * wf[1]).sum()
        grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    sse = np.stack([(r.double() ** 2).sum(dim=(0, 2)).cpu().numpy() for r in res], axis=1)          # [L][2]
    return dict(state=[o.detach().cpu().numpy() for o in out[:4]], grads=[g.cpu().numpy() for g in grads], sse=sse)


def fitted(cuda, run, sched, tgt, S, grad=True):
    import torch
    import dhts
    _, L, N, T, _ = shape(run)
    c, wf = weights_of(run)
    wf = torch.tensor(wf, device=cuda)
    leaves = [torch.tensor(a, device=cuda, requires_grad=grad) for a in leaves_of(run, sched)]
    out = dhts.macro_rollout(*leaves, T, DT, DX, UM, checkpoint=S, target=torch.tensor(tgt, device=cuda))
    assert len(out) == 5 and tuple(out[4].shape) == (L, 2) and out[4].dtype == torch.float64
    res = dict(state=[o.detach().cpu().numpy() for o in out[:4]], sse=out[4].detach().cpu().numpy())
    if grad:
        loss = (out[4] * torch.tensor(c, device=cuda)).sum() + (out[0] * wf[0]).sum() + (out[2] * wf[1]).sum()
        res["grads"] = [g.cpu().numpy() for g in torch.autograd.grad(loss, leaves, allow_unused=True)]
    return res


# ---- 1. equals the dense yardstick ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", BOTH, ids=["const", "sched"])
@pytest.mark.parametrize("run", ALL)
def test_equals_the_dense_yardstick(cuda, run, sched):
    """rT .. qT bit for bit, the four gradients np.array_equal, sse within T N 2^-52 relative of the float64 sum of the yardstick's own
    float32 residuals squared (each term is exact in double: a rounding bound of the summation, not a measured tolerance), and the same
    sse bits on a second run and at every segment."""
    _, L, N, T, _ = shape(run)
    bad = []
    for kind in KINDS:
        per_target = {}
        for S in segments(run):
            Sk = S if (kind == "rows" and S is not True) else (plan_of(run)["segment"] if kind == "rows" else 0)
            key = (kind, Sk)
            if key not in per_target:
                tgt = target_of(cuda, run, sched, kind, Sk)
                per_target[key] = (tgt, yardstick(cuda, run, sched, tgt), [])
            tgt, ref, seen = per_target[key]
            got = fitted(cuda, run, sched, tgt, S)
            for k in range(4):
                if not same_bits(got["state"][k], ref["state"][k]):
                    bad.append((kind, S, "state %d" % k))
            for name, a, b in zip(("g_r0", "g_u0", "g_ghost_r", "g_ghost_u"), got["grads"], ref["grads"]):
                if a.shape != b.shape or not np.array_equal(a, b):
                    bad.append((kind, S, name, float(np.nanmax(np.abs(a.astype(np.float64) - b))) if a.size else 0.0))
            bound = T * N * 2.0 ** -52
            err = np.abs(got["sse"] - ref["sse"]) / np.maximum(np.abs(ref["sse"]), 1e-300)
            print("%s %s %s S=%s: sse %s rel. error %s (bound %.1e)" % (run, "sched" if sched else "const", kind, S,
                                                                         got["sse"].ravel()[:2], err.max() if err.size else 0, bound))
            if not np.all((err <= bound) | (got["sse"] == ref["sse"])):
                bad.append((kind, S, "sse", err.max()))
            if kind == "all_nan" or T == 0:
                assert np.all(got["sse"] == 0.0)
            if kind == "no_speed":
                assert np.all(got["sse"][:, 1] == 0.0)
            seen.append(got["sse"])
        for tgt, ref, seen in per_target.values():
            if not all(same_bits(s, seen[0]) for s in seen):
                bad.append((kind, "sse differs between segments"))
        again = fitted(cuda, run, sched, tgt, S)
        if not same_bits(again["sse"], got["sse"]) or not all(same_bits(a, b) for a, b in zip(again["grads"], got["grads"])):
            bad.append((kind, S, "a second run differs"))
    assert not bad, bad


# ---- 2. the forward nobody differentiates -----------------------------------------------------------------------------------------------
def test_no_grad_forward_returns_sse_and_keeps_no_checkpoints(cuda):
    """A line search's loss evaluation: the same sse bits, and above the inputs less than the checkpoint buffer would take (the allocator's
    peak): at L = 2, N = 64, T = 2000 the checkpoints are 1 MB with the plan's segment, everything else the forward makes 0.2 MB."""
    import torch
    import dhts
    from dhts import ops
    L, N, T = 2, 64, 2000
    rng = np.random.default_rng(11)
    mk = lambda a, g: torch.tensor(a.astype(F), device=cuda, requires_grad=g)      # noqa: E731
    data = [rng.uniform(0.2, 0.6, (L, N)), rng.uniform(5.0, 15.0, (L, N)), rng.uniform(0.2, 0.6, (T, L, 2)), rng.uniform(5.0, 15.0, (T, L, 2))]
    tgt = torch.tensor(rng.uniform(0.2, 0.6, (T, L, 2, N)).astype(F), device=cuda)
    desc = ops.macro_desc(L, N, DT, DX, UM)
    ck_bytes = ops.macro_ckpt_numel(desc, T, ops.macro_ckpt_target_plan(desc, T)["segment"]) * 4
    assert ck_bytes >= 1 << 19
    peaks, sse = {}, {}
    for grad in (False, True):
        leaves = [mk(a, grad) for a in data]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = dhts.macro_rollout(*leaves, T, DT, DX, UM, checkpoint=True, target=tgt)
        torch.cuda.synchronize()
        peaks[grad] = torch.cuda.max_memory_allocated() - base
        sse[grad] = out[4].detach().cpu().numpy()
        assert out[4].requires_grad == grad
        del out, leaves
    print("peak above the inputs: %d B without grad, %d B with; checkpoints %d B" % (peaks[False], peaks[True], ck_bytes))
    assert same_bits(sse[False], sse[True]) and np.all(sse[True] > 0)
    assert peaks[False] < ck_bytes // 2 and peaks[True] >= ck_bytes


# ---- 3. memory --------------------------------------------------------------------------------------------------------------------------
def test_a_long_horizon_fit_holds_neither_history_nor_tape(cuda):
    """L = 2, N = 64, T = 20 000 with a schedule.  Above the resident inputs (target among them), forward + backward may take the
    checkpoint buffer, 32 B per (step, lane, side) of boundary gradients, and 1 MB.  One [T][L][N] float plane is 10.24 MB and does not fit
    that allowance beside the checkpoints, so a hidden history (three planes), g_hist (two) or a tape fails this."""
    import torch
    import dhts
    from dhts import ops
    L, N, T = 2, 64, 20000
    rng = np.random.default_rng(5)
    mk = lambda a: torch.tensor(a.astype(F), device=cuda, requires_grad=True)      # noqa: E731
    desc = ops.macro_desc(L, N, DT, DX, UM)
    ck_bytes = ops.macro_ckpt_numel(desc, T, ops.macro_ckpt_target_plan(desc, T)["segment"]) * 4
    rest = 32 * T * L * 2 + (1 << 20)
    plane = T * L * N * 4
    assert plane == 10240000 and plane > rest
    leaves = [mk(rng.uniform(0.2, 0.6, (L, N))), mk(rng.uniform(5.0, 15.0, (L, N))), mk(rng.uniform(0.2, 0.6, (T, L, 2))),
              mk(rng.uniform(5.0, 15.0, (T, L, 2)))]
    tgt = torch.tensor(rng.uniform(0.2, 0.6, (T, L, 2, N)).astype(F), device=cuda)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = dhts.macro_rollout(*leaves, T, DT, DX, UM, checkpoint=True, target=tgt)
    (out[4].sum() + out[0].sum()).backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("checkpoints %d B; peak above the inputs %d B (allowed %d)" % (ck_bytes, peak, ck_bytes + rest))
    assert all(torch.isfinite(x.grad).all() for x in leaves)
    assert peak <= ck_bytes + rest


# ---- 4. the chained oracle --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", BOTH, ids=["const", "sched"])
@pytest.mark.parametrize("run", ["lane65_T37", "lane130", "lane300_T29"])
def test_against_the_chained_oracle(cuda, oracle, run, sched):
    """The oracle's rollout with the dense per-step cotangents gh_r, gh_u = (float32)(2 c) * (its own history - target), 0 at NaN."""
    _, L, N, T, _ = shape(run)
    r0, u0, gr, gu = leaves_of(run, sched)
    c, wf = weights_of(run)
    if sched:
        f = R.sched_fwd(oracle, r0, u0, gr, gu, DT, DX, UM)
    else:
        f = oracle.macro_rollout_fwd(r0, u0, gr, gu, T, DT, DX, UM, want_hist=True)
    rng = np.random.default_rng(4000 + sum(map(ord, run)))
    tgt = np.stack([f["hist_r"], f["hist_u"]], axis=2).astype(F) + rng.standard_normal((T, L, 2, N)).astype(F) * F([0.05, 1.0])[None, None, :, None]
    tgt = np.ascontiguousarray(tgt, F)
    tgt[rng.random(tgt.shape) < 0.2] = NAN
    tgt[T // 2] = NAN
    g2 = (2.0 * c).astype(F)
    d_r, d_u = (f["hist_r"] - tgt[:, :, 0]).astype(F), (f["hist_u"] - tgt[:, :, 1]).astype(F)
    gh_r = np.where(np.isnan(tgt[:, :, 0]), F(0), g2[None, :, 0, None] * d_r).astype(F)
    gh_u = np.where(np.isnan(tgt[:, :, 1]), F(0), g2[None, :, 1, None] * d_u).astype(F)
    sse = np.stack([(np.where(np.isnan(d), 0.0, d.astype(np.float64)) ** 2).sum(axis=(0, 2)) for d in (d_r, d_u)], axis=1)
    if sched:
        b = R.sched_bwd(oracle, f, g_rT=wf[0], g_uT=wf[1], gh_r=gh_r, gh_u=gh_u)
    else:
        b = oracle.macro_rollout_bwd(f, g_rT=wf[0], g_uT=wf[1], gh_r=gh_r, gh_y=np.zeros_like(gh_r), gh_u=gh_u)
    for S in (True, 4):
        got = fitted(cuda, run, sched, tgt, S)
        for j, k in enumerate(("rT", "yT", "uT")):
            assert state_report("%s S=%s %s" % (run, S, k), got["state"][j], f[k]) <= TOL_STATE
        assert state_report("%s S=%s sse" % (run, S), got["sse"], sse) <= TOL_STATE
        for k, g in zip(("g_r0", "g_u0", "g_ghost_r", "g_ghost_u"), got["grads"]):
            assert grad_report("%s S=%s %s" % (run, S, k), g, b[k]) <= TOL_GRAD


# ---- 5. the raw entry points ------------------------------------------------------------------------------------------------------------
def guarded64(cuda, n):
    """test_macro_ckpt_gpu.guarded for n doubles: 2 n float32 of NaN at an even offset of a larger buffer, the sentinel on both sides
    -> (buffer, the float32 view)."""
    import torch
    buf = torch.full((GUARD + 1 + 2 * n + GUARD,), SENTINEL, dtype=torch.float32, device=cuda)
    view = buf[GUARD + 1:GUARD + 1 + 2 * n]
    view.fill_(float("nan"))
    return buf, view


def untouched64(buf, n):
    b = buf.cpu().numpy()
    return bool(np.all(b[:GUARD + 1] == SENTINEL) and np.all(b[GUARD + 1 + 2 * n:] == SENTINEL))


def raw_run(cuda, run, sched, S, lanes=None):
    """One forward and one reverse launch at the raw operators, on all lanes or on `lanes` alone, into poisoned, guarded buffers."""
    import torch
    from dhts import ops
    _, L, N, T, _ = shape(run)
    r0, u0, gr, gu = leaves_of(run, sched)
    tgt = target_of(cuda, run, sched, "entries")
    rng = np.random.default_rng(7)
    g_r, g_y = rng.standard_normal((2, L, N)).astype(F)
    g_sse = rng.uniform(0.5, 1.5, (L, 2))
    if lanes is not None:
        r0, u0, g_r, g_y, g_sse, tgt = r0[lanes], u0[lanes], g_r[lanes], g_y[lanes], g_sse[lanes], np.ascontiguousarray(tgt[:, lanes])
        gr, gu = (gr[:, lanes], gu[:, lanes]) if sched else (gr[lanes], gu[lanes])
        L = len(lanes)
    desc = ops.macro_desc(L, N, DT, DX, UM)
    r, u = torch.tensor(r0, device=cuda), torch.tensor(u0, device=cuda)
    y, q = ops.macro_state_from_ru(r, u, UM)
    ghost = ghost_quads(cuda, gr, gu)
    t = torch.tensor(tgt, device=cuda)
    Sr = ops.macro_ckpt_target_plan(desc, T, S)["segment"]
    n_ck = ops.macro_ckpt_numel(desc, T, Sr)
    assert n_ck * 4 == -(-T // Sr) * L * N * 8
    n_gg = T * L * 4 if sched else L * 4
    bufs = {}
    for name, n in (("ckpt", n_ck), ("r", L * N), ("y", L * N), ("u", L * N), ("q", L * N), ("g_r", L * N), ("g_y", L * N)):
        bufs[name] = guarded(cuda, n) + (n,)
    for name, n in (("sse", L * 2), ("g_ghost", n_gg)):          # doubles
        bufs[name] = guarded64(cuda, n) + (n,)
    out = tuple(bufs[k][1].view(L, N) for k in ("r", "y", "u", "q"))
    sse = bufs["sse"][1].view(torch.float64).view(L, 2)
    err, err_b = ops.new_error_record(cuda), ops.new_error_record(cuda)
    state, sse_out = ops.macro_rollout_fwd_ckpt_target(desc, T, r, y, u, q, ghost, bufs["ckpt"][1], t, segment=S, sse=sse, err=err, out=out)
    assert sse_out.data_ptr() == sse.data_ptr() and state[0].data_ptr() == bufs["r"][1].data_ptr()
    no_ck = ops.macro_rollout_fwd_ckpt_target(desc, T, r, y, u, q, ghost, None, t, segment=S)
    assert all(torch.equal(a, b) for a, b in zip(no_ck[0], state)) and torch.equal(no_ck[1].view(torch.int64), sse.view(torch.int64))
    ck_fwd = bufs["ckpt"][1].clone()
    g_out = (bufs["g_r"][1].view(L, N), bufs["g_y"][1].view(L, N))
    g_ghost = bufs["g_ghost"][1].view(torch.float64).view((T, L, 2, 2) if sched else (L, 2, 2))
    res = ops.macro_rollout_bwd_ckpt_target(desc, T, bufs["ckpt"][1], r, y, u, q, ghost, torch.tensor(g_r, device=cuda),
                                            torch.tensor(g_y, device=cuda), t, g_sse=torch.tensor(g_sse, device=cuda), final=state[:3],
                                            segment=S, err=err_b, out=g_out, g_ghost=g_ghost)
    assert err.tolist() == [0, 0, 0, 0] and err_b.tolist() == [0, 0, 0, 0], (err.tolist(), err_b.tolist())
    assert torch.equal(ck_fwd.view(torch.int32), bufs["ckpt"][1].view(torch.int32)), "the reverse sweep wrote into the checkpoints"
    for name, (buf, view, n) in bufs.items():
        assert (untouched64 if name in ("sse", "g_ghost") else untouched)(buf, n), "a store beside %s" % name
        assert not torch.isnan(view).any(), "%d elements of %s were not written" % (int(torch.isnan(view).sum()), name)
    # without a cotangent of the sums the sweep is the siblings' plain one
    plain = ops.macro_rollout_bwd_ckpt_target(desc, T, bufs["ckpt"][1], r, y, u, q, ghost, torch.tensor(g_r, device=cuda),
                                              torch.tensor(g_y, device=cuda), t, segment=S)
    sib = ops.macro_rollout_bwd_ckpt(desc, T, bufs["ckpt"][1], r, y, u, q, ghost, torch.tensor(g_r, device=cuda), torch.tensor(g_y, device=cuda),
                                     segment=Sr)
    assert all(torch.equal(a, b) for a, b in zip(plain, sib))
    return dict(state=[s.cpu().numpy() for s in state], sse=sse.cpu().numpy(), ckpt=ck_fwd.cpu().numpy(), g_r0=res[0].cpu().numpy(),
                g_y0=res[1].cpu().numpy(), g_ghost=res[2].cpu().numpy())


@pytest.mark.parametrize("sched", BOTH, ids=["const", "sched"])
@pytest.mark.parametrize("run,S", [("lane65_T37", 5), ("lane130", 0), ("lane300_T29", 9), ("pair128_g2_T26", 3), ("lane1000", 1)])
def test_raw_operators_write_everything_repeat_and_keep_lanes_apart(cuda, run, sched, S):
    _, L, N, T, _ = shape(run)
    keep = L - 1
    a = raw_run(cuda, run, sched, S)
    b = raw_run(cuda, run, sched, S)
    c = raw_run(cuda, run, sched, S, lanes=[keep])
    for k in range(4):
        assert same_bits(a["state"][k], b["state"][k]) and same_bits(a["state"][k][keep:keep + 1], c["state"][k])
    for k in ("sse", "g_r0", "g_y0"):
        assert same_bits(a[k], b[k]) and same_bits(a[k][keep:keep + 1], c[k]), k
    assert same_bits(a["ckpt"], b["ckpt"]) and same_bits(a["g_ghost"], b["g_ghost"])
    assert same_bits(a["g_ghost"][:, keep:keep + 1] if sched else a["g_ghost"][keep:keep + 1], c["g_ghost"])
    assert np.all(a["sse"] > 0)


def test_raw_rejections_leave_the_outputs_alone_and_t0_copies(cuda):
    """Every rejected combination returns DHTS_E_INVALID and writes nothing; T = 0: state and cotangents as they went in, sse = 0."""
    import ctypes as C
    import torch
    from dhts import _lib, ops
    L, N, T = 2, 65, 6
    desc = ops.macro_desc(L, N, DT, DX, UM)
    lib = _lib.lib()
    P = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    rng = np.random.default_rng(3)
    r = torch.tensor(rng.uniform(0.2, 0.6, (L, N)).astype(F), device=cuda)
    u = torch.tensor(rng.uniform(5.0, 15.0, (L, N)).astype(F), device=cuda)
    y, q = ops.macro_state_from_ru(r, u, UM)
    ghost = ghost_quads(cuda, rng.uniform(0.2, 0.6, (L, 2)).astype(F), rng.uniform(5.0, 15.0, (L, 2)).astype(F))
    tgt = torch.zeros(T, L, 2, N, device=cuda)
    S = 2
    ck = torch.full((ops.macro_ckpt_numel(desc, T, S),), 7.0, device=cuda)
    outs = [torch.full((L, N), 7.0, device=cuda) for _ in range(4)]
    sse = torch.full((L, 2), 7.0, dtype=torch.float64, device=cuda)
    g_sse = torch.ones(L, 2, dtype=torch.float64, device=cuda)
    gg = torch.full((L, 2, 2), 7.0, dtype=torch.float64, device=cuda)
    mx = ops.macro_ckpt_target_plan(desc, T)["max_segment"]

    def fwd(T=T, S=S, target=tgt, sse=sse, r_out=outs[0]):
        return lib.dhts_macro_rollout_fwd_ckpt_target(C.byref(desc), T, S, P(r), P(y), P(u), P(q), P(ghost), 0, None if r_out is None else P(r_out),
                                                      P(outs[1]), P(outs[2]), P(outs[3]), P(ck), None if target is None else P(target),
                                                      None if sse is None else P(sse), None, None)

    def bwd(T=T, S=S, target=tgt, g=g_sse, fin=r, ckpt=ck, sched=0, g_ghost=gg):
        return lib.dhts_macro_rollout_bwd_ckpt_target(C.byref(desc), T, S, None if ckpt is None else P(ckpt), P(r), P(y), P(u), P(q), P(ghost), sched,
                                                      P(r), P(y), None if target is None else P(target), None if g is None else P(g),
                                                      None if fin is None else P(fin), P(y), P(u), P(outs[0]), P(outs[1]),
                                                      None if g_ghost is None else P(g_ghost), None, None)
    for call in (lambda: fwd(T=-1), lambda: fwd(S=-1), lambda: fwd(S=mx + 1), lambda: fwd(target=None), lambda: fwd(sse=None),
                 lambda: fwd(r_out=None), lambda: bwd(T=-1), lambda: bwd(S=mx + 1), lambda: bwd(target=None), lambda: bwd(fin=None),
                 lambda: bwd(ckpt=None), lambda: bwd(sched=1, g_ghost=None)):
        assert call() == _lib.E_INVALID
    torch.cuda.synchronize()
    for t in outs + [ck, sse, gg]:
        assert bool((t == 7.0).all()), "a rejected call wrote"
    # T = 0: no row of anything is addressed (target, ckpt NULL)
    assert fwd(T=0, target=None) == 0
    assert all(torch.equal(a, b) for a, b in zip(outs, (r, y, u, q))) and bool((sse == 0).all())
    assert bwd(T=0, target=None, ckpt=None, fin=None) == 0
    assert torch.equal(outs[0], r) and torch.equal(outs[1], y) and bool((gg == 0).all())
    # ... and through the operator, with both boundary forms
    import dhts
    for run in ("lane64_t0",):
        for sched in BOTH:
            _, L0, N0, T0, _ = shape(run)
            assert T0 == 0
            got = fitted(cuda, run, sched, np.zeros((0, L0, 2, N0), F), True)
            assert np.all(got["sse"] == 0) and got["grads"][0].shape == (L0, N0)
    assert dhts.MacroRolloutTarget is ops.MacroRolloutTarget


# ---- 6. the example ---------------------------------------------------------------------------------------------------------------------
def run_example(tmp_path, tag, extra):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    cwd = os.path.join(str(tmp_path), tag)
    os.makedirs(cwd)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "estimate_inflow.py"), "--n_cell", "48", "--n_timestep", "40",
                          "--n_episode", "2", "--seed", "1", "--readings", "field"] + extra, cwd=cwd, env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    files = [os.path.join(dp, f) for dp, _, fs in os.walk(cwd) for f in fs if f == "trial_0.txt"]
    assert len(files) == 1, files
    return [line.split() for line in open(files[0]).read().splitlines() if line.strip()]


def test_inflow_example_fits_the_field_with_and_without_the_fused_loss(cuda, tmp_path):
    """--readings field against --readings field --checkpoint --fused-loss at 48 cells, 40 steps, two episodes: the profile-error column
    is identical, the loss column within T N 2^-52 relative (both are double sums of the same exact terms)."""
    dense = run_example(tmp_path, "dense", [])
    fused = run_example(tmp_path, "fused", ["--checkpoint", "--fused-loss"])
    assert len(dense) == len(fused) == 2
    for a, b in zip(dense, fused):
        assert a[:-1] == b[:-1], (a, b)
        la, lb = float(a[-1]), float(b[-1])
        print("loss %r (torch, double) against %r (fused)" % (la, lb))
        assert abs(la - lb) <= 40 * 48 * 2.0 ** -52 * abs(la)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "estimate_inflow.py"), "--readings", "field", "--fused-loss"],
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 2 and "--fused-loss" in r.stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "estimate_inflow.py"), "--checkpoint", "--fused-loss"],
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 2 and "--fused-loss" in r.stderr
