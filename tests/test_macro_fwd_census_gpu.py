"""The pair kernel's step loop after its instruction census (csrc/macro_fwd_pairs.inc, arz_interface_queued): phase 1's case logic and
the queue append on lane masks, the tape written through a buffer descriptor, phase 2's record addresses as 32-bit LDS offsets.  No
floating-point operation changed, so the yardstick is the lane kernel (DHTS_OPT_MACRO_FWD_VARIANT = 2), bit for bit: final state, the
blocks the tape expands to, the reverse sweep's gradients -- and an empty error record from every launch.

Shapes: 8 lanes, T = 40, the smallest at which the touched code takes each of its paths:
  (a) N = 128, one lane per workgroup (64 threads), a lane that queues more than 64 interfaces: phase 2's second round;
  (b) N = 256 with 2 and N = 512 with 4 lanes per workgroup: thread g solves entry g / G of lane g % G, rows of several lanes behind one
      descriptor;
  (c) speeds of 243 .. 249.5 with dx / dt = 500: every cell fails own_calm (|u| alone is past the threshold 234.9) and every interface
      the cheap bound of arz_interface_queued (|u_L| + |u_R| + u_max / 2 >= 501), yet every wave speed is below 500: the exact CFL tests
      run in every wavefront of phase 2 and raise nothing (the oracle's rc is 0 on these inputs: test_fast_inputs_are_legal, no GPU);
  (d) the scheduled, the detector-tap and the scheduled detector-tap instantiations at N = 128 and N = 512 on the inputs of (a)."""
import numpy as np
import pytest

from util import options

DT, DX, UM = 0.01, 5.0, 30.0
L, T = 8, 40
QUEUE_LANE = 5


def mixed_inputs(N):
    """tests/test_gpu_parity.py's lanes: vacuum stretches (the general form of phase 1), float32(eps), an idle lane, every other cell
    empty, a lane that queues every interface, an empty lane, vacuum across a wavefront's chunk boundary."""
    rng = np.random.default_rng(900 + N)
    r0 = rng.uniform(0.02, 1.0, (L, N)).astype(np.float32)
    r0[1, 10:20] = 0.0
    r0[2] = 0.4
    r0[3, 64] = np.float32(1e-5)
    r0[3, 65] = 1e-6
    r0[4, ::2] = 0.0
    r0[QUEUE_LANE] = 0.5                     # speeds 28, 2, 28, ...: a shock with s0 < 0 or a rarefaction with lambda_0(Q_L) < 0 at every interface
    r0[6] = 0.0
    r0[7, 126:130 if N > 128 else 128] = 0.0
    r0[L - 1, N - 3:] = 0.0
    u0 = rng.uniform(0.0, UM, (L, N)).astype(np.float32)
    u0[2] = 12.0
    u0[QUEUE_LANE, ::2], u0[QUEUE_LANE, 1::2] = 28.0, 2.0
    gr = rng.uniform(0.0, 1.0, (T, L, 2)).astype(np.float32)
    gu = rng.uniform(0.0, UM, (T, L, 2)).astype(np.float32)
    return r0, u0, gr, gu


def fast_inputs(N):
    """Case (c).  Lane 2 turns slow in its second half: a fast-to-slow junction, whose interfaces are not trivial."""
    rng = np.random.default_rng(700 + N)
    r0 = rng.uniform(0.05, 0.95, (L, N)).astype(np.float32)
    u0 = rng.uniform(243.0, 249.5, (L, N)).astype(np.float32)
    u0[2, N // 2:] = rng.uniform(0.0, UM, N - N // 2).astype(np.float32)
    gr = np.repeat(rng.uniform(0.05, 0.95, (1, L, 2)).astype(np.float32), T, axis=0)
    gu = np.repeat(rng.uniform(243.0, 249.5, (1, L, 2)).astype(np.float32), T, axis=0)
    return r0, u0, gr, gu


def fails_the_cheap_tests(r0, u0):
    """The float64 forms of own_calm's g and arz_interface_queued's bound at the given state: (cells with g >= threshold, interior
    interfaces with bound >= dx / dt)."""
    r, u = r0.astype(np.float64), u0.astype(np.float64)
    ueq = UM * (1.0 - np.sqrt(r + 1e-5))
    g = np.abs(u) + 0.5 * np.abs(ueq) + 0.5 * UM * np.sqrt(r)
    thr = 0.5 * (DX / DT) * (1.0 - 1e-4) - 0.002 * UM - 0.5 * UM
    bound = 0.5 * np.abs(ueq[:, :-1]) + np.abs(u[:, :-1]) + np.abs(u[:, 1:]) + 0.5 * UM * np.sqrt(r[:, :-1]) + 0.5 * UM
    return g >= thr, bound >= DX / DT


def test_fast_inputs_are_legal(oracle):
    """The inputs of case (c) on the CPU: the oracle steps them without a CFL violation (rc = 0), and at step 0 every cell of the fast
    lanes fails own_calm and every interface between two fast cells fails the cheap bound."""
    for N in (128, 512):
        r0, u0, gr, gu = fast_inputs(N)
        f = oracle.macro_rollout_fwd(r0, u0, gr[0], gu[0], T, DT, DX, UM, want_tape=False)
        assert f["rc"] == 0, (N, f["rc"])
        assert np.isfinite(f["rT"]).all() and np.isfinite(f["uT"]).all()
        not_calm, not_sure = fails_the_cheap_tests(r0, u0)
        fast = [l for l in range(L) if l != 2]
        assert not_calm[fast].all() and not_sure[fast].all()
        assert not_calm[2, :N // 2].all() and not_sure[2, :N // 2 - 1].all()


def run(cuda, N, variant, group, form, data):
    """One forward rollout with a tape and its reverse sweep.  form: plain | sched | taps | taps_sched."""
    import torch
    from dhts import ops
    r0, u0, gr, gu = (torch.tensor(a, device=cuda) for a in data)
    y0, q0 = ops.macro_state_from_ru(r0, u0, UM)
    gy, gq = ops.macro_state_from_ru(gr, gu, UM)
    sched = form in ("sched", "taps_sched")
    ghost = torch.stack([gr, gy, gu, gq], dim=-1).contiguous()      # [T][L][2][4]
    if not sched:
        ghost = ghost[0].contiguous()
    det = torch.tensor([0, 1, 63, 64, N // 2, N - 2, N - 1], dtype=torch.int32, device=cuda) if form.startswith("taps") else None
    desc = ops.macro_desc(L, N, DT, DX, UM)
    errs = [ops.new_error_record(cuda), ops.new_error_record(cuda)]
    res = {}
    with options(variant, group):
        plan = ops.macro_rollout_plan(desc, T) if det is None else ops.macro_taps_plan(desc, T, det.numel())
        assert plan["fwd_kernel"] == (2 if variant == 0 else 0) and plan["fwd_lanes_per_group"] == group, plan
        tape = torch.full((ops.macro_tape_numel(desc, T),), float("nan"), device=cuda)      # unwritten parts must never be read
        if det is not None:
            out, res["taps"] = ops.macro_rollout_fwd_taps(desc, T, r0, y0, u0, q0, ghost, det, tape=tape, err=errs[0])
        elif sched:
            out = ops.macro_rollout_fwd_sched(desc, T, r0, y0, u0, q0, ghost, tape=tape, err=errs[0])
        else:
            out = ops.macro_rollout_fwd(desc, T, r0, y0, u0, q0, ghost, tape=tape, err=errs[0])
        g_r, g_y = 2 * out[0], 0.5 * out[1]
        if det is not None:
            g_taps = torch.tensor(np.random.default_rng(5).standard_normal((T, L, 2, det.numel())).astype(np.float32), device=cuda)
            grads = ops.macro_rollout_bwd_taps(desc, T, tape, g_r, g_y, det, g_taps, sched=sched, err=errs[1])
        elif sched:
            grads = ops.macro_rollout_bwd_sched(desc, T, tape, g_r, g_y, err=errs[1])
        else:
            grads = ops.macro_rollout_bwd(desc, T, tape, g_r, g_y, err=errs[1])
        res.update(state=out, dqs=ops.macro_tape_expand(desc, T, tape), grads=grads, err=[e.tolist() for e in errs])
    s_f4 = ((3 * N + 3) // 4 + 7) // 8 * 8
    res["counts"] = tape.view(T, L, -1)[:, :, 4 * s_f4].contiguous().view(torch.int32)       # exceptions per (step, lane)
    return res


def same_bits(tag, pair, lane):
    import torch
    for res in (pair, lane):
        assert res["err"][0][0] == 0 and res["err"][1][0] == 0, (tag, res["err"])
    for name in ("state", "grads"):
        for j, (a, b) in enumerate(zip(pair[name], lane[name])):
            assert a.shape == b.shape and bool(torch.isfinite(a).all()), (tag, name, j)
            assert torch.equal(a, b), "%s %s[%d]: %d entries differ, max |d| %.3e" % (
                tag, name, j, int((a != b).sum()), float((a.double() - b.double()).abs().max()))
    assert bool(torch.isfinite(pair["dqs"]).all()), tag
    assert torch.equal(pair["dqs"], lane["dqs"]), "%s: %d entries of the expanded tape differ" % (tag, int((pair["dqs"] != lane["dqs"]).sum()))
    if "taps" in pair:
        assert torch.equal(pair["taps"], lane["taps"]), tag
    assert float(pair["grads"][0].abs().max()) > 0, tag


@pytest.mark.gpu
@pytest.mark.parametrize("N,group", [(128, 1), (256, 2), (512, 4)])
def test_mixed_lanes_equal_the_lane_kernel(cuda, N, group):
    """Cases (a) and (b)."""
    data = mixed_inputs(N)
    pair, lane = run(cuda, N, 0, group, "plain", data), run(cuda, N, 2, 1, "plain", data)
    same_bits("N %d group %d" % (N, group), pair, lane)
    # the lane that queues nearly every interface: more entries than a round of phase 2 has threads per lane (N / 2)
    assert int(pair["counts"][0, QUEUE_LANE]) > N // 2, pair["counts"][0]


@pytest.mark.gpu
@pytest.mark.parametrize("N,group", [(128, 1), (256, 2), (512, 4)])
def test_fast_lanes_run_the_exact_cfl_tests_and_raise_nothing(cuda, N, group):
    """Case (c)."""
    data = fast_inputs(N)
    pair, lane = run(cuda, N, 0, group, "plain", data), run(cuda, N, 2, 1, "plain", data)
    same_bits("fast N %d group %d" % (N, group), pair, lane)
    # nothing calm: every interface of the fast lanes is queued in step 0
    assert int(pair["counts"][0, 0]) == N + 1, pair["counts"][0]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["sched", "taps", "taps_sched"])
@pytest.mark.parametrize("N", [128, 512])
def test_scheduled_and_tapped_forms_equal_the_lane_kernel(cuda, N, form):
    """Case (d)."""
    data = mixed_inputs(N)
    pair, lane = run(cuda, N, 0, 1, form, data), run(cuda, N, 2, 1, form, data)
    same_bits("%s N %d" % (form, N), pair, lane)
