"""Reverse mode of the fused ARZ rollout from checkpoints on the GPU (dhts_macro_rollout_fwd_ckpt / _bwd_ckpt and dhts.macro_rollout
with `checkpoint`): bit equality with the taped pair at the lane mapping's corner cases, with both boundary forms, with and without
detectors, at every kind of segment length; the oracle and a reference golden; the raw operators (every element written, nothing beside
them, repeatable, lanes independent); the two fault records; the memory a long horizon takes; the example.  Shapes and leaves are
tests/test_macro_taps_gpu.py's; two cases are also run for a few dozen steps so that several segments and a short last one occur."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

import macro_sched_ref as R
from test_macro_taps_gpu import CASES, DT, DX, UM, ghost_quads, inputs, weights
from util import TOL_GRAD, TOL_STATE, grad_report, meta_of, options, rel_elem, rel_max, state_report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (case of test_macro_taps_gpu.CASES, T; None = the case's own)
RUNS = {
    "lane1": ("lane1", None),
    "lane2": ("lane2", None),
    "lane63": ("lane63", None),
    "lane64": ("lane64", None),
    "lane65": ("lane65", None),
    "lane65_T37": ("lane65", 37),
    "lane130": ("lane130", None),
    "lane300": ("lane300", None),
    "lane300_T29": ("lane300", 29),
    "lane1000": ("lane1000", None),          # max_segment = 2
    "pair128_g2": ("pair128_g2", None),      # the taped side: the pair kernel and bwd_fast<.., full>
    "pair128_g2_T26": ("pair128_g2", 26),
    "pair512": ("pair512", None),
    "lane64_t0": ("lane64_t0", None),
}
BOTH = [False, True]


def shape(run):
    case, T = RUNS[run]
    L, N, T0 = CASES[case][:3]
    return case, L, N, (T0 if T is None else T), CASES[case][5]


def leaves_of(run, sched):
    """test_macro_taps_gpu.inputs; for another T the same recipe (random state, independent random boundary cells per step, on some
    steps a boundary density below 1e-5 or exactly 0)."""
    case, L, N, T, _ = shape(run)
    if T == CASES[case][2]:
        return inputs(case, sched)
    rng = np.random.default_rng(sum(map(ord, run)))
    r0 = rng.uniform(0.05, 0.95, (L, N)).astype(np.float32)
    u0 = rng.uniform(0.0, UM, (L, N)).astype(np.float32)
    gr = rng.uniform(0.05, 0.95, (T, L, 2)).astype(np.float32)
    gu = rng.uniform(0.0, UM, (T, L, 2)).astype(np.float32)
    gr[T // 2, 0, 0] = 3e-6
    gr[T - 1, L - 1, 1] = 0.0
    gr[0, 0, 1] = 8e-6
    cr = rng.uniform(0.05, 0.95, (L, 2)).astype(np.float32)
    cu = rng.uniform(0.0, UM, (L, 2)).astype(np.float32)
    return (r0, u0, gr, gu) if sched else (r0, u0, cr, cu)


def weights_of(run):
    """test_macro_taps_gpu.weights: the loss is sum of w * (r, y, u) at the detectors after every step plus wf * (rT, uT)."""
    case, L, N, T, det = shape(run)
    if T == CASES[case][2]:
        return weights(case)
    rng = np.random.default_rng(1000 + sum(map(ord, run)))
    return rng.standard_normal((T, L, 3, len(det))).astype(np.float32), rng.standard_normal((2, L, N)).astype(np.float32)


def segments(run):
    """1, 2, the plan's, max_segment, one that does not divide T, one beyond T -- wherever max_segment allows."""
    from dhts import ops
    _, L, N, T, _ = shape(run)
    plan = ops.macro_ckpt_plan(ops.macro_desc(L, N, DT, DX, UM), T)
    mx = plan["max_segment"]
    odd = [s for s in range(2, 8) if T % s]                 # the smallest segment that leaves a short last one
    want = {1, 2, plan["segment"], mx, T + 3} | set(odd[:1])
    return [True] + sorted(s for s in want if 1 <= s <= mx)


@pytest.fixture(scope="module", autouse=True)
def device_memory_as_found():
    """Nothing here outlives its test but what hangs in a reference cycle (a failing test's traceback, for one); that goes when the
    module's last test has run, so that the module leaves the allocator's count as it found it."""
    yield
    gc.collect()


def rollout(cuda, run, sched, dets, checkpoint):
    """Outputs and gradients of one dhts.macro_rollout call."""
    import torch
    import dhts
    case, L, N, T, det = shape(run)
    variant, group = CASES[case][3:5]
    w, wf = (torch.tensor(a, device=cuda) for a in weights_of(run))
    leaves = [torch.tensor(a, device=cuda, requires_grad=True) for a in leaves_of(run, sched)]
    with options(variant, group):
        out = dhts.macro_rollout(*leaves, T, DT, DX, UM, detectors=det if dets else None, checkpoint=checkpoint)
        loss = (out[0] * wf[0]).sum() + (out[2] * wf[1]).sum()
        if dets:
            assert tuple(out[4].shape) == (T, L, 3, len(det))
            loss = loss + (out[4] * w).sum()
        grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    res = dict(state=[o.detach() for o in out[:4]], read=out[4].detach() if dets else None, grads=grads)
    return res


@pytest.mark.parametrize("dets", BOTH, ids=["plain", "detectors"])
@pytest.mark.parametrize("sched", BOTH, ids=["const", "sched"])
@pytest.mark.parametrize("run", sorted(RUNS))
def test_checkpointed_equals_taped_bit_for_bit(cuda, run, sched, dets):
    """States, readings, g_r0, g_u0 and the boundary gradients (per step with a schedule) of the checkpointed call are the taped call's
    bits at every segment length.  The taped side runs whatever its plan picks (the pair kernel and the pipelined sweeps included): the
    project holds those bit-equal to the lane kernel and the general sweep, whose expressions the new kernels use.  Nothing is skipped."""
    import torch
    from dhts import ops
    case, L, N, T, det = shape(run)
    ref = rollout(cuda, run, sched, dets, None)
    plan = ops.macro_rollout_plan(ops.macro_desc(L, N, DT, DX, UM), T)
    print("%s: taped plan fwd_kernel %d bwd_pipelined %d; segments %s" % (run, plan["fwd_kernel"], plan["bwd_pipelined"], segments(run)))
    bad = []
    for S in segments(run):
        got = rollout(cuda, run, sched, dets, S)
        pairs = [("state %d" % k, ref["state"][k], got["state"][k]) for k in range(4)]
        if dets:
            pairs.append(("readings", ref["read"], got["read"]))
        pairs += list(zip(("g_r0", "g_u0", "g_ghost_r", "g_ghost_u"), ref["grads"], got["grads"]))
        for name, a, b in pairs:
            assert (a is None) == (b is None), name
            if a is None:
                continue
            assert a.shape == b.shape, name
            equal = torch.equal(a, b) if a.numel() else True
            print("%s %s %s S=%s %s: %s" % (run, "sched" if sched else "const", "det" if dets else "plain", S, name,
                                           "equal" if equal else "not bit-equal"))
            if not equal:
                bad.append((S, name))
    assert not bad, bad


@pytest.mark.parametrize("run,sched,dets", [("lane65_T37", True, True), ("lane130", False, False)])
def test_checkpointed_against_the_oracle(cuda, oracle, run, sched, dets):
    """As test_macro_taps_gpu.test_detectors_against_the_oracle: the oracle's history gathered at det, its reverse sweep with the weights
    scattered to det.  checkpoint=True and a segment that leaves a short last one."""
    case, L, N, T, det = shape(run)
    r0, u0, gr, gu = leaves_of(run, sched)
    w, wf = weights_of(run)
    gh = np.zeros((3, T, L, N), np.float32)
    if dets:
        gh[:, :, :, det] = w.transpose(2, 0, 1, 3)
    if sched:
        f = R.sched_fwd(oracle, r0, u0, gr, gu, DT, DX, UM)
        b = R.sched_bwd(oracle, f, g_rT=wf[0], g_uT=wf[1], gh_r=gh[0], gh_y=gh[1], gh_u=gh[2])
    else:
        f = oracle.macro_rollout_fwd(r0, u0, gr, gu, T, DT, DX, UM, want_hist=True)
        b = oracle.macro_rollout_bwd(f, g_rT=wf[0], g_uT=wf[1], gh_r=gh[0], gh_y=gh[1], gh_u=gh[2])
    for S in (True, 4):
        t = rollout(cuda, run, sched, dets, S)
        for j, k in enumerate(("rT", "yT", "uT")):
            assert state_report("%s S=%s %s" % (run, S, k), t["state"][j].cpu().numpy(), f[k]) <= TOL_STATE
        if dets:
            read = t["read"].cpu().numpy()
            for j, k in enumerate(("hist_r", "hist_y", "hist_u")):
                assert state_report("%s S=%s readings of %s" % (run, S, k), read[:, :, j], f[k][:, :, det]) <= TOL_STATE
        for k, g in zip(("g_r0", "g_u0", "g_ghost_r", "g_ghost_u"), t["grads"]):
            assert grad_report("%s S=%s %s" % (run, S, k), g.cpu().numpy(), b[k]) <= TOL_GRAD


@pytest.mark.parametrize("name", ["small", "x10"])
def test_macro_rollout_vs_golden_checkpointed(cuda, golden_dir, name):
    """test_gpu_parity.test_macro_rollout_vs_golden with checkpoint=3, at that test's limits.  The history it looks at excludes
    checkpoints, so every cell is a detector here: the readings are the history."""
    import torch
    import dhts
    g = np.load(os.path.join(golden_dir, "macro_rollout_%s.npz" % name))
    m = meta_of(g)

    def leaf(a):
        return torch.tensor(np.ascontiguousarray(a[None], dtype=np.float32), device=cuda, requires_grad=True)
    r0, u0, gr, gu = leaf(g["r0"]), leaf(g["u0"]), leaf(g["ghost_r"]), leaf(g["ghost_u"])
    N = r0.shape[1]
    rT, yT, uT, _, hist = dhts.macro_rollout(r0, u0, gr, gu, m["T"], m["dt"], m["dx"], m["u_max"], detectors=list(range(N)), checkpoint=3)
    loss = hist.sum() if m["tap"] == "every_sum" else (rT ** 2).sum() + (uT ** 2).sum()
    loss.backward()
    for a, k in ((rT, "rT"), (yT, "yT"), (uT, "uT")):
        assert rel_max(a.detach().cpu().numpy()[0], g[k]) <= TOL_STATE
    assert max(rel_elem(rT.detach().cpu().numpy()[0], g["rT"]), rel_elem(uT.detach().cpu().numpy()[0], g["uT"])) <= TOL_STATE
    h = hist.detach().cpu().numpy()
    for t in range(len(g["steps_r"])):
        for j, k in enumerate(("steps_r", "steps_y", "steps_u")):
            assert rel_max(h[t, 0, j], g[k][t]) <= TOL_STATE
    assert abs(float(loss) - float(g["loss"])) <= 2e-6 * abs(float(g["loss"]))
    assert grad_report("G4 %s (checkpointed) d loss / d r0" % name, r0.grad.cpu().numpy()[0], g["g_r0"]) <= TOL_GRAD
    assert grad_report("G4 %s (checkpointed) d loss / d u0" % name, u0.grad.cpu().numpy()[0], g["g_u0"]) <= TOL_GRAD
    assert rel_max(gr.grad.cpu().numpy()[0], g["g_ghost_r"]) <= TOL_GRAD
    assert rel_max(gu.grad.cpu().numpy()[0], g["g_ghost_u"]) <= TOL_GRAD


# ---- at the entry points ------------------------------------------------------------------------------------------------------------
GUARD, SENTINEL = 257, 12345.0


def guarded(cuda, n):
    """n float32 of NaN in the middle of a larger buffer with a sentinel on both sides -> (buffer, view)."""
    import torch
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=cuda)
    view = buf[GUARD:GUARD + n]
    view.fill_(float("nan"))
    return buf, view


def untouched(buf, n):
    b = buf.cpu().numpy()
    return bool(np.all(b[:GUARD] == SENTINEL) and np.all(b[GUARD + n:] == SENTINEL))


def raw_run(cuda, run, sched, S, lanes=None):
    """One forward and one reverse launch at the raw operators, on all lanes or on `lanes` alone; outputs, readings, checkpoints and
    gradients land in poisoned, guarded buffers."""
    import torch
    from dhts import ops
    case, L, N, T, det = shape(run)
    D = len(det)
    r0, u0, gr, gu = leaves_of(run, sched)
    rng = np.random.default_rng(7)
    g_r, g_y = rng.standard_normal((2, L, N)).astype(np.float32)
    g_t = rng.standard_normal((T, L, 2, D)).astype(np.float32)
    if lanes is not None:
        r0, u0, g_r, g_y, g_t = r0[lanes], u0[lanes], g_r[lanes], g_y[lanes], g_t[:, lanes]
        gr, gu = (gr[:, lanes], gu[:, lanes]) if sched else (gr[lanes], gu[lanes])
        L = len(lanes)
    desc = ops.macro_desc(L, N, DT, DX, UM)
    r, u = torch.tensor(r0, device=cuda), torch.tensor(u0, device=cuda)
    y, q = ops.macro_state_from_ru(r, u, UM)
    ghost = ghost_quads(cuda, gr, gu)
    n_ck = ops.macro_ckpt_numel(desc, T, S)
    assert n_ck * 4 == -(-T // ops.macro_ckpt_plan(desc, T, D, S)["segment"]) * L * N * 8
    bufs = {}
    for name, n in (("ckpt", n_ck), ("taps", T * L * 3 * D), ("r", L * N), ("y", L * N), ("u", L * N), ("q", L * N), ("g_r", L * N),
                    ("g_y", L * N)):
        bufs[name] = guarded(cuda, n) + (n,)
    out = tuple(bufs[k][1].view(L, N) for k in ("r", "y", "u", "q"))
    dt = torch.tensor(det, dtype=torch.int32, device=cuda)
    err, err_b = ops.new_error_record(cuda), ops.new_error_record(cuda)
    state, taps = ops.macro_rollout_fwd_ckpt(desc, T, r, y, u, q, ghost, bufs["ckpt"][1], segment=S, det=dt, err=err, out=out,
                                             taps=bufs["taps"][1].view(T, L, 3, D))
    assert taps.data_ptr() == bufs["taps"][1].data_ptr() and state[0].data_ptr() == bufs["r"][1].data_ptr()
    ck_fwd = bufs["ckpt"][1].clone()
    g_out = (bufs["g_r"][1].view(L, N), bufs["g_y"][1].view(L, N))
    g_r0, g_y0, g_ghost = ops.macro_rollout_bwd_ckpt(desc, T, bufs["ckpt"][1], r, y, u, q, ghost, torch.tensor(g_r, device=cuda),
                                                     torch.tensor(g_y, device=cuda), segment=S, det=dt, g_taps=torch.tensor(g_t, device=cuda),
                                                     err=err_b, out=g_out)
    assert err.tolist() == [0, 0, 0, 0] and err_b.tolist() == [0, 0, 0, 0], (err.tolist(), err_b.tolist())
    assert tuple(g_ghost.shape) == ((T, L, 2, 2) if sched else (L, 2, 2))
    assert torch.equal(ck_fwd.view(torch.int32), bufs["ckpt"][1].view(torch.int32)), "the reverse sweep wrote into the checkpoints"
    for name, (buf, view, n) in bufs.items():
        assert untouched(buf, n), "a store beside %s" % name
        assert not torch.isnan(view).any(), "%d elements of %s were not written" % (int(torch.isnan(view).sum()), name)
    # the taped pair on the same arguments
    tape = torch.zeros(ops.macro_tape_numel(desc, T), dtype=torch.float32, device=cuda)
    variant, group = CASES[case][3:5]
    with options(variant, group):
        t_state, t_taps = ops.macro_rollout_fwd_taps(desc, T, r, y, u, q, ghost, dt, tape=tape)
        t_g = ops.macro_rollout_bwd_taps(desc, T, tape, torch.tensor(g_r, device=cuda), torch.tensor(g_y, device=cuda), dt,
                                         torch.tensor(g_t, device=cuda), sched=sched)
    res = dict(state=[s.cpu().numpy() for s in state], taps=taps.cpu().numpy(), ckpt=ck_fwd.cpu().numpy(), g_r0=g_r0.cpu().numpy(),
               g_y0=g_y0.cpu().numpy(), g_ghost=g_ghost.cpu().numpy())
    ref = dict(state=[s.cpu().numpy() for s in t_state], taps=t_taps.cpu().numpy(), g_r0=t_g[0].cpu().numpy(), g_y0=t_g[1].cpu().numpy(),
               g_ghost=t_g[2].cpu().numpy())
    return res, ref


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("sched", BOTH, ids=["const", "sched"])
@pytest.mark.parametrize("run,S", [("lane65_T37", 5), ("lane130", 0), ("lane300_T29", 14), ("pair128_g2_T26", 3), ("lane1000", 2)])
def test_raw_operators_write_everything_repeat_and_keep_lanes_apart(cuda, run, sched, S):
    case, L, N, T, det = shape(run)
    keep = L - 1
    a, ref = raw_run(cuda, run, sched, S)
    b, _ = raw_run(cuda, run, sched, S)
    c, _ = raw_run(cuda, run, sched, S, lanes=[keep])
    for k in range(4):
        assert same_bits(a["state"][k], ref["state"][k]), "state %d against the taped forward" % k
        assert same_bits(a["state"][k], b["state"][k]) and same_bits(a["state"][k][keep:keep + 1], c["state"][k])
    assert same_bits(a["taps"], ref["taps"]) and same_bits(a["taps"], b["taps"]) and same_bits(a["taps"][:, keep:keep + 1], c["taps"])
    assert same_bits(a["ckpt"], b["ckpt"])
    C = a["ckpt"].size // (L * N * 2)
    assert same_bits(a["ckpt"].reshape(C, L, N, 2)[:, keep:keep + 1], c["ckpt"].reshape(C, 1, N, 2))
    r0 = leaves_of(run, sched)[0]
    assert same_bits(a["ckpt"].reshape(C, L, N, 2)[0, :, :, 0], r0), "row 0 holds the state the rollout starts from"
    for k in ("g_r0", "g_y0", "g_ghost"):
        assert same_bits(a[k], ref[k]), "%s against the taped sweep" % k
        assert same_bits(a[k], b[k])
    for k in ("g_r0", "g_y0"):
        assert same_bits(a[k][keep:keep + 1], c[k])
    assert same_bits(a["g_ghost"][:, keep:keep + 1] if sched else a["g_ghost"][keep:keep + 1], c["g_ghost"])


def test_an_index_outside_the_lane_matches_no_cell(cuda):
    """The index contract of the taps operators: an entry of det outside [0, N) forms no address -- its column of the readings stays as
    it was and its column of g_taps (NaN here) is not read."""
    import torch
    from dhts import ops
    L, N, T, S = 2, 65, 10, 3
    r0, u0, gr, gu = inputs("lane65", True)
    desc = ops.macro_desc(L, N, DT, DX, UM)
    r, u = torch.tensor(r0, device=cuda), torch.tensor(u0, device=cuda)
    y, q = ops.macro_state_from_ru(r, u, UM)
    ghost = ghost_quads(cuda, gr, gu)
    rng = np.random.default_rng(7)
    g_r, g_y = (torch.tensor(a, device=cuda) for a in rng.standard_normal((2, L, N)).astype(np.float32))
    res = {}
    for name, det in (("good", [2, N - 1]), ("bad", [2, N - 1, N, N + 70000, -5])):
        D = len(det)
        dt = torch.tensor(det, dtype=torch.int32, device=cuda)
        ck = torch.empty(ops.macro_ckpt_numel(desc, T, S), dtype=torch.float32, device=cuda)
        taps = torch.full((T, L, 3, D), float("nan"), dtype=torch.float32, device=cuda)
        g_t = rng.standard_normal((T, L, 2, D)).astype(np.float32) if name == "good" else np.concatenate(
            [res["good"][3], np.full((T, L, 2, 3), np.nan, np.float32)], axis=-1)
        ops.macro_rollout_fwd_ckpt(desc, T, r, y, u, q, ghost, ck, segment=S, det=dt, taps=taps)
        g = ops.macro_rollout_bwd_ckpt(desc, T, ck, r, y, u, q, ghost, g_r, g_y, segment=S, det=dt, g_taps=torch.tensor(g_t, device=cuda))
        res[name] = (taps.cpu().numpy(), [x.cpu().numpy() for x in g], None, g_t)
    assert same_bits(res["bad"][0][..., :2], res["good"][0]) and np.isnan(res["bad"][0][..., 2:]).all()
    for a, b in zip(res["bad"][1], res["good"][1]):
        assert same_bits(a, b)


# ---- the fault records ----------------------------------------------------------------------------------------------------------------
def test_a_cfl_violation_raises_the_taped_call_s_text_and_the_replay_adds_no_record(cuda):
    """test_macro_fwd_jvp_gpu.slow_traffic: at dt = 1.0 one (step, lane, interface) violates the bound -- the last step's downstream
    boundary of lane 1 -- so the record is a function of the input.  The checkpointed forward leaves the taped forward's record, the
    operator raises the same text, and the reverse sweep, which replays that step, leaves its own record clean."""
    import torch
    import dhts
    from dhts import _lib, ops
    from test_macro_fwd_jvp_gpu import slow_traffic
    L, N, T = 2, 65, 4
    leaves = slow_traffic(L, N, T, fast=(T - 1, 1))
    text = {}
    for ck in (None, 1, 3):
        dev = [torch.tensor(x, device=cuda, requires_grad=True) for x in leaves]
        with pytest.raises(AssertionError) as e:
            dhts.macro_rollout(*dev, T, 1.0, DX, UM, detectors=[0, 64], checkpoint=ck)
        text[ck] = str(e.value)
        del e                    # (it holds this frame through its traceback: a cycle around every tensor here)
    print(text)
    assert "step %d, lane 1, interface %d" % (T - 1, N) in text[None]
    assert text[1] == text[None] and text[3] == text[None]
    desc = ops.macro_desc(L, N, 1.0, DX, UM)
    r, u = torch.tensor(leaves[0], device=cuda), torch.tensor(leaves[1], device=cuda)
    y, q = ops.macro_state_from_ru(r, u, UM)
    ghost = ghost_quads(cuda, leaves[2], leaves[3])
    taped, err, err_b = (ops.new_error_record(cuda) for _ in range(3))
    ops.macro_rollout_fwd_sched(desc, T, r, y, u, q, ghost, err=taped)
    ck = torch.empty(ops.macro_ckpt_numel(desc, T, 3), dtype=torch.float32, device=cuda)
    ops.macro_rollout_fwd_ckpt(desc, T, r, y, u, q, ghost, ck, segment=3, err=err)
    g = torch.ones(L, N, device=cuda)
    ops.macro_rollout_bwd_ckpt(desc, T, ck, r, y, u, q, ghost, g, g, segment=3, err=err_b)
    assert taped.tolist() == [_lib.FAULT_CFL, T - 1, 1, N] and err.tolist() == taped.tolist()
    assert err_b.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("run,cell", [("lane2", 0), ("lane1", 0)])
def test_a_non_finite_cotangent_gives_the_taped_sweep_s_record(cuda, run, cell):
    """An inf in g_rT at one cell (data, through the loss weights).  Every cell of these lanes meets a non-finite cotangent in the
    sweep's first step, so whichever thread's report wins, the record is (DHTS_FAULT_NAN, T - 1, lane): a function of the input, and
    the AssertionError of the checkpointed call is the taped call's."""
    import torch
    import dhts
    from dhts import _lib, ops
    case, L, N, T, det = shape(run)
    lane = L - 1
    text = {}
    for ck in (None, 1, 2, True):
        leaves = [torch.tensor(a, device=cuda, requires_grad=True) for a in leaves_of(run, True)]
        rT = dhts.macro_rollout(*leaves, T, DT, DX, UM, checkpoint=ck)[0]
        w = torch.ones(L, N, device=cuda)
        w[lane, cell] = float("inf")
        with pytest.raises(AssertionError) as e:
            (rT * w).sum().backward()
        text[ck] = str(e.value)
        del e
    print(text)
    assert "step %d, lane %d" % (T - 1, lane) in text[None]
    assert all(t == text[None] for t in text.values())
    # the raw records
    desc = ops.macro_desc(L, N, DT, DX, UM)
    r0, u0, gr, gu = leaves_of(run, True)
    r, u = torch.tensor(r0, device=cuda), torch.tensor(u0, device=cuda)
    y, q = ops.macro_state_from_ru(r, u, UM)
    ghost = ghost_quads(cuda, gr, gu)
    g_r = torch.zeros(L, N, device=cuda)
    g_r[lane, cell] = float("inf")
    tape = torch.zeros(ops.macro_tape_numel(desc, T), dtype=torch.float32, device=cuda)
    ck = torch.empty(ops.macro_ckpt_numel(desc, T, 2), dtype=torch.float32, device=cuda)
    taped, err = ops.new_error_record(cuda), ops.new_error_record(cuda)
    ops.macro_rollout_fwd_sched(desc, T, r, y, u, q, ghost, tape=tape)
    ops.macro_rollout_bwd_sched(desc, T, tape, g_r, torch.zeros_like(g_r), err=taped)
    ops.macro_rollout_fwd_ckpt(desc, T, r, y, u, q, ghost, ck, segment=2)
    ops.macro_rollout_bwd_ckpt(desc, T, ck, r, y, u, q, ghost, g_r, torch.zeros_like(g_r), segment=2, err=err)
    assert taped.tolist()[:3] == [_lib.FAULT_NAN, T - 1, lane] and err.tolist()[:3] == taped.tolist()[:3]


# ---- memory ---------------------------------------------------------------------------------------------------------------------------
def test_a_long_horizon_takes_checkpoints_not_a_tape(cuda):
    """L = 2, N = 64, T = 20 000, four detectors, checkpoint=True.  Above what exists before the call, forward + backward may take: the
    checkpoint buffer; the readings and their cotangents; the gradients; 1 MB of allocator slack.  With R = the bytes of the readings
    [T][L][3][D]: the readings are R; their cotangents are the one autograd hands back (R) and the sweep's [T][L][2][D] form of it
    (2/3 R).  The gradients: per cell the cotangent planes (g_r, g_y in and out, g_u0, the two leaves' .grad: 28 B, taken as 32); per
    (step, lane, side) of the boundary schedule the sweep's float64 pair (16 B), the two float32 results (8 B) and the leaves' .grad
    (8 B): 32 B.  Nothing else is allowed for: the boundary quads and u_eq the replay reads (20 B per (step, lane, side), saved by the
    forward) and the temporaries of the glue, which goes over the T-sized cotangents a sixteenth at a time, have to fit into the slack
    and into the terms that are not alive yet when the sweep runs (the float32 results and the .grad)."""
    import torch
    import dhts
    from dhts import ops
    L, N, T, D = 2, 64, 20000, 4
    det = [0, 21, 42, 63]
    rng = np.random.default_rng(5)
    mk = lambda a: torch.tensor(a.astype(np.float32), device=cuda, requires_grad=True)      # noqa: E731
    w = torch.tensor(rng.standard_normal((T, L, 3, D)).astype(np.float32), device=cuda)
    desc = ops.macro_desc(L, N, DT, DX, UM)
    tape_bytes = ops.macro_tape_numel(desc, T) * 4
    ck_bytes = ops.macro_ckpt_numel(desc, T) * 4
    R_bytes = T * L * 3 * D * 4
    allowed = ck_bytes + (R_bytes + R_bytes + 2 * R_bytes // 3) + (32 * T * L * 2 + 32 * L * N) + (1 << 20)
    peaks = {}
    for ck in (True, None):
        leaves = [mk(rng.uniform(0.2, 0.6, (L, N))), mk(rng.uniform(5.0, 15.0, (L, N))), mk(rng.uniform(0.2, 0.6, (T, L, 2))),
                  mk(rng.uniform(5.0, 15.0, (T, L, 2)))]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = dhts.macro_rollout(*leaves, T, DT, DX, UM, detectors=det, checkpoint=ck)
        ((out[4] * w).sum() + out[0].sum()).backward()
        torch.cuda.synchronize()
        peaks[ck] = torch.cuda.max_memory_allocated() - base
        assert all(torch.isfinite(x.grad).all() for x in leaves)
        del out, leaves
    print("tape %d B, checkpoints %d B, readings %d B; peak above the inputs: checkpointed %d B (allowed %d), taped %d B" % (
        tape_bytes, ck_bytes, R_bytes, peaks[True], allowed, peaks[None]))
    assert peaks[True] <= allowed
    assert peaks[True] < tape_bytes / 4
    assert peaks[None] >= tape_bytes


# ---- the example ----------------------------------------------------------------------------------------------------------------------
def run_example(tmp_path, tag, extra):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    cwd = os.path.join(str(tmp_path), tag)
    os.makedirs(cwd)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "estimate_inflow.py"), "--n_cell", "64", "--n_timestep", "60",
                          "--n_episode", "5", "--seed", "1"] + extra, cwd=cwd, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    files = [os.path.join(dp, f) for dp, _, fs in os.walk(cwd) for f in fs if f == "trial_0.txt"]
    assert len(files) == 1, files
    return open(files[0]).read()


def test_inflow_example_logs_the_same_lines_with_and_without_checkpoints(cuda, tmp_path):
    taped = run_example(tmp_path, "taped", [])
    assert run_example(tmp_path, "plan", ["--checkpoint"]) == taped
    assert run_example(tmp_path, "seven", ["--checkpoint", "7"]) == taped
    losses = [float(line.split()[-1]) for line in taped.splitlines() if line.strip()]
    assert len(losses) == 5 and losses[0] > 0 and losses[-1] < losses[0]


def test_the_readings_cotangent_in_parts_has_the_same_bits(cuda):
    """What a checkpointed backward does at a long horizon: _per_step_cotangent over `rows` steps at a time is _per_step_cotangent at
    once, a short last part and a one-lane, one-detector shape (contiguous slices) included, and the cotangent it is given stays as it was."""
    import torch
    from dhts import ops
    g = torch.Generator().manual_seed(5)
    for T, L, D in ((11, 2, 4), (7, 1, 1)):
        steps = torch.rand(T, L, 3, D, generator=g).to(cuda)
        steps[:, :, 1] = steps[:, :, 0] * (5.0 + 20.0 * steps[:, :, 1])
        g_steps = torch.randn(T, L, 3, D, generator=g).to(cuda)
        kept = g_steps.clone()
        whole = ops._per_step_cotangent(steps, g_steps, UM)
        assert tuple(whole.shape) == (T, L, 2, D) and not torch.equal(whole, g_steps[:, :, :2])
        for rows in (1, 3, 4, T, T + 1):
            parts = ops._per_step_cotangent(steps, g_steps, UM, rows=rows)
            assert parts.is_contiguous() and torch.equal(parts.view(torch.int32), whole.view(torch.int32)), (T, L, D, rows)
        assert torch.equal(g_steps, kept)
