"""The tape-free fused rollout + tangent kernel on the device: dhts.micro_rollout_jvp(fused=True) and the raw
ops.micro_rollout_fwd_jvp against the taped path (forward with tapes + tangent sweep) bit for bit, against the float64 yardstick of
tests/micro_jvp_ref.py directly, and against itself: bit-identity across K, slots and runs, exact zeros and the clip, the two fault
records, guard bands, and the absence of any [T]-sized allocation.  Needs a real MI355X: python -m pytest tests -m gpu"""
import os
import subprocess
import sys

import numpy as np
import pytest

import micro_jvp_ref as J
from test_micro_jvp_gpu import CASES, DT, HEADS, IDS, LEAVES, case_inputs, device_jvp, directions, guarded, same_bits, stop_head, yard
from test_micro_params_gpu import lanes
from util import TOL_GRAD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("pT", "vT", "t_pT", "t_vT", "t_hist")


def fused_jvp(cuda, p0, v0, par, head, T, dt, count=None, want_hist=False, check_faults=True, **tang):
    """test_micro_jvp_gpu.device_jvp with fused=True: the same inputs through the one tape-free entry point."""
    import torch
    import dhts
    dt64 = {"t_head": torch.float64, "t_params": torch.float64}
    kw = {n: torch.tensor(a, device=cuda, dtype=dt64.get(n, torch.float32)) for n, a in tang.items() if a is not None}
    cnt = None if count is None else torch.tensor(count, device=cuda, dtype=torch.int32)
    prim, tan = dhts.micro_rollout_jvp(torch.tensor(p0, device=cuda), torch.tensor(v0, device=cuda),
                                       torch.tensor(par, device=cuda, dtype=torch.float64), torch.tensor(head, device=cuda, dtype=torch.float64),
                                       T, dt, count=cnt, want_hist=want_hist, check_faults=check_faults, fused=True, **kw)
    torch.cuda.synchronize()
    assert all(not x.requires_grad and x.grad_fn is None for x in prim + tan), "no autograd graph is recorded"
    n = lambda x: x.cpu().numpy()      # noqa: E731
    return dict(pT=n(prim[0]), vT=n(prim[1]), hist=n(prim[2]) if want_hist else None,
                t_pT=n(tan[0]), t_vT=n(tan[1]), t_hist=n(tan[2]) if want_hist else None)


def assert_same(tag, a, b, live=None):
    """Two result dicts bit for bit: the states, the tangents, their history, and hist at live slots (the forward leaves the rest of
    hist unwritten)."""
    for key in KEYS:
        if a[key] is None and b[key] is None:
            continue
        assert a[key].shape == b[key].shape, "%s: %s has shape %s against %s" % (tag, key, a[key].shape, b[key].shape)
        assert same_bits(a[key], b[key]), "%s: %s differs from the taped path" % (tag, key)
    if a["hist"] is not None:
        assert a["hist"].shape == b["hist"].shape
        T, L, _, V = a["hist"].shape
        lt = np.broadcast_to(live[None, :, None, :], (T, L, 2, V))
        assert same_bits(a["hist"][lt], b["hist"][lt]), "%s: hist differs from the taped path at a live slot" % tag


# =================================================================================================================
# 1. bit identity with the taped path, 2. the yardstick directly
# =================================================================================================================
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fused_equals_the_taped_path_bit_for_bit(cuda, case):
    """Every shape of the tangent sweep's own tests, the directions of LEAVES (K = 5: the t_params kernel, launches of 4 + 1) and of
    LEAVES[:3] (K = 4), with and without the histories: pT, vT, hist at live slots, t_pT, t_vT, t_hist are the taped path's bits.  The
    cases of 64, 130 and 1024 vehicles are also held against the float64 yardstick directly (TOL_GRAD, dead slots exactly 0), so that the
    check does not rest on the taped path alone."""
    L, V, T, count = case
    p0, v0, par, head, t = case_inputs(case)
    live = J.live_mask(L, V, count)
    for names in (LEAVES, LEAVES[:3]):
        d = directions(t, names)
        K = len(names) + 1
        for want_hist in (True, False):
            taped = device_jvp(cuda, p0, v0, par, head, T, DT, count=count, want_hist=want_hist, **d)
            fused = fused_jvp(cuda, p0, v0, par, head, T, DT, count=count, want_hist=want_hist, **d)
            assert fused["t_pT"].shape == (K, L, V)
            assert_same("%s K=%d hist=%s" % (IDS[CASES.index(case)], K, want_hist), fused, taped, live)
            if want_hist and V in (64, 130, 1024):
                ys = yard(case, names)
                for k in range(K):
                    got = dict(t_pT=fused["t_pT"][k], t_vT=fused["t_vT"][k], t_hist=fused["t_hist"][k])
                    J.compare("fused %s K=%d direction %d" % (IDS[CASES.index(case)], K, k), got, ys[k], count, TOL_GRAD)


# =================================================================================================================
# 3. a direction does not depend on K or its slot
# =================================================================================================================
@pytest.mark.parametrize("want_params", [False, True], ids=["state", "params"])
def test_a_direction_does_not_depend_on_k_or_slot(cuda, want_params):
    """Direction i of a K-direction call equals the K = 1 call of it, bit for bit, for K = 1 .. 9 (the masked 3, the splits 4 + 1,
    4 + 2, 4 + 4 + 1) and every window of the nine directions, so every direction visits every slot; two runs give the same bits."""
    L, V, T = 4, 130, 7
    count = [130, 0, 77, 1]
    N = 9
    rng = np.random.default_rng(19)
    p0, v0, par, head = lanes(rng, L, V)
    head[0], head[2], head[3] = HEADS[1], HEADS[2], HEADS[1]
    stop_head(par, head, 2, count[2])
    names = LEAVES if want_params else LEAVES[:3]
    shapes = dict(t_p0=(L, V), t_v0=(L, V), t_head=(L, 2), t_params=(6, L, V))
    full = {n: rng.standard_normal((N,) + shapes[n]).astype(np.float32 if n in ("t_p0", "t_v0") else np.float64) for n in names}
    keys = ("pT", "vT", "t_pT", "t_vT", "t_hist")
    single = [fused_jvp(cuda, p0, v0, par, head, T, DT, count=count, want_hist=True, **{n: full[n][i:i + 1] for n in names}) for i in range(N)]
    for K in range(1, N + 1):
        for first in range(0, N + 1 - K):
            o = fused_jvp(cuda, p0, v0, par, head, T, DT, count=count, want_hist=True, **{n: full[n][first:first + K] for n in names})
            assert same_bits(o["pT"], single[0]["pT"]) and same_bits(o["vT"], single[0]["vT"]), "the primal depends on K"
            for i in range(K):
                for key in keys[2:]:
                    assert same_bits(o[key][i], single[first + i][key][0]), "K=%d first=%d slot %d: %s differs from the K = 1 call" % (K, first, i, key)
    a = fused_jvp(cuda, p0, v0, par, head, T, DT, count=count, want_hist=True, **full)
    b = fused_jvp(cuda, p0, v0, par, head, T, DT, count=count, want_hist=True, **full)
    assert all(same_bits(a[key], b[key]) for key in keys), "two runs differ"


# =================================================================================================================
# 4. exact zeros, the state-only bits, the clip
# =================================================================================================================
def test_zeros_dead_slots_and_the_clip(cuda):
    """test_micro_jvp_gpu.test_zeros_dead_slots_and_the_clip with fused=True: a zero tangent gives exact zeros; t_params = 0 gives the
    bits of the state-only call; dead slots and empty lanes are exact zeros; under the acceleration clip the parameter term is absent."""
    L, V, T = 3, 70, 7
    count = [70, 0, 33]
    rng = np.random.default_rng(23)
    p0, v0, par, head = lanes(rng, L, V)
    head[0], head[2] = HEADS[1], HEADS[2]
    stop_head(par, head, 2, count[2])
    z = fused_jvp(cuda, p0, v0, par, head, T, DT, count=count, want_hist=True, t_p0=np.zeros((2, L, V), np.float32),
                  t_params=np.zeros((2, 6, L, V)), t_head=np.zeros((2, L, 2)))
    assert all(np.all(z[k] == 0) for k in ("t_pT", "t_vT", "t_hist"))
    t_p, t_v = rng.standard_normal((2, 2, L, V)).astype(np.float32)
    t_head = rng.standard_normal((2, L, 2))
    state = fused_jvp(cuda, p0, v0, par, head, T, DT, count=count, want_hist=True, t_p0=t_p, t_v0=t_v, t_head=t_head)
    zero_q = fused_jvp(cuda, p0, v0, par, head, T, DT, count=count, want_hist=True, t_p0=t_p, t_v0=t_v, t_head=t_head,
                       t_params=np.zeros((2, 6, L, V)))
    assert all(same_bits(state[k], zero_q[k]) for k in ("t_pT", "t_vT", "t_hist"))
    live = J.live_mask(L, V, count)
    for o in (state, zero_q):
        assert np.all(o["t_pT"][:, ~live] == 0) and np.all(o["t_vT"][:, ~live] == 0)
        assert np.all(o["t_hist"][:, :, ~live[:, None, :].repeat(2, 1)] == 0)
        assert same_bits(o["pT"][~live], p0[~live]) and same_bits(o["vT"][~live], v0[~live]), "dead slots pass the state through"
    # one step, head gap (0.5, 0): the head vehicle (slot count - 1) is under the clip, its follower is not
    one = [fused_jvp(cuda, p0, v0, par, head, 1, DT, count=count, want_hist=True, t_p0=t_p, t_v0=t_v, t_head=t_head, **kw)
           for kw in ({}, dict(t_params=rng.standard_normal((2, 6, L, V))))]
    assert one[0]["vT"][2, 32] == 0.0, "the head of lane 2 stops in its one step (acceleration clip)"
    assert same_bits(one[0]["t_vT"][:, 2, 32], one[1]["t_vT"][:, 2, 32]) and same_bits(one[0]["t_pT"], one[1]["t_pT"])
    assert np.all(one[1]["t_vT"][:, 2, 32] == 0)
    assert np.all(one[0]["t_vT"][:, 2, :32] != one[1]["t_vT"][:, 2, :32]) and np.all(one[0]["t_vT"][:, 0] != one[1]["t_vT"][:, 0])


# =================================================================================================================
# 5. the two fault records
# =================================================================================================================
def test_fault_records(cuda, capsys):
    """The caller's own records through ops.micro_rollout_fwd_jvp: a NaN in one initial tangent is on err_jvp as DHTS_FAULT_NAN with its
    lane and step 0 and leaves err clean (the operator raises); a collision is on err as DHTS_FAULT_COLLISION and leaves err_jvp clean
    (the operator prints and goes on), and the outputs are still the taped path's bits."""
    import torch
    from dhts import _lib, ops
    L, V, T = 4, 70, 5
    rng = np.random.default_rng(2)
    p0, v0, par, head = lanes(rng, L, V)
    desc = ops.micro_desc(L, V, DT)
    tp0, tv0 = torch.tensor(p0, device=cuda), torch.tensor(v0, device=cuda)
    tpar, thead = torch.tensor(par, device=cuda, dtype=torch.float64), torch.tensor(head, device=cuda, dtype=torch.float64)
    t_p = torch.zeros(2, L, V, device=cuda)
    t_p[1, 2, 40] = float("nan")
    t_v = torch.ones(2, L, V, device=cuda)
    err, err_jvp = ops.new_error_record(cuda), ops.new_error_record(cuda)
    prim, tan = ops.micro_rollout_fwd_jvp(desc, T, tp0, tv0, tpar, thead, t_p, t_v, err=err, err_jvp=err_jvp)
    code, step, lane, index = err_jvp.tolist()
    assert (code, step, lane) == (_lib.FAULT_NAN, 0, 2) and index in (39, 40)
    assert err.tolist()[0] == 0
    assert bool(torch.all(torch.isfinite(tan[0][0]))) and bool(torch.isnan(tan[0][1, 2, 40]))
    assert prim[2] is None and tan[2] is None
    with pytest.raises(AssertionError):
        fused_jvp(cuda, p0, v0, par, head, T, DT, t_p0=t_p.cpu().numpy())
    fused_jvp(cuda, p0, v0, par, head, T, DT, check_faults=False, t_p0=t_p.cpu().numpy())
    # a lane with two vehicles 1 m apart, the follower at 30 m/s
    count = [70, 2, 70, 70]
    p0[1, :2], v0[1, :2] = (0.0, 1.0), (30.0, 10.0)
    tp0, tv0 = torch.tensor(p0, device=cuda), torch.tensor(v0, device=cuda)
    cnt = torch.tensor(count, device=cuda, dtype=torch.int32)
    t_q = torch.tensor(rng.standard_normal((2, 6, L, V)), device=cuda)
    err, err_jvp = ops.new_error_record(cuda), ops.new_error_record(cuda)
    prim, tan = ops.micro_rollout_fwd_jvp(desc, T, tp0, tv0, tpar, thead, t_v, t_v, count=cnt, t_params=t_q, want_hist=True, err=err,
                                          err_jvp=err_jvp)
    code, step, lane, index = err.tolist()
    assert (code, step, lane, index) == (_lib.FAULT_COLLISION, 0, 1, 0)
    assert err_jvp.tolist()[0] == 0
    tang = dict(t_p0=t_v.cpu().numpy(), t_v0=t_v.cpu().numpy(), t_params=t_q.cpu().numpy())
    capsys.readouterr()
    taped = device_jvp(cuda, p0, v0, par, head, T, DT, count=count, want_hist=True, **tang)
    assert "Collision detected" in capsys.readouterr().out
    fused = fused_jvp(cuda, p0, v0, par, head, T, DT, count=count, want_hist=True, **tang)      # prints, does not raise
    assert "Collision detected between vehicles (step 0, lane 1, vehicle 0)" in capsys.readouterr().out
    live = J.live_mask(L, V, count)
    assert_same("collision", fused, taped, live)
    raw = dict(pT=prim[0].cpu().numpy(), vT=prim[1].cpu().numpy(), hist=prim[2].cpu().numpy(), t_pT=tan[0].cpu().numpy(),
               t_vT=tan[1].cpu().numpy(), t_hist=tan[2].cpu().numpy())
    assert_same("collision, raw operator", raw, taped, live)


# =================================================================================================================
# 6. guard bands
# =================================================================================================================
@pytest.mark.parametrize("case", [CASES[4], CASES[7]], ids=[IDS[4], IDS[7]])
def test_guard_bands(cuda, case):
    """All six outputs in the middle of NaN-prefilled buffers, K = 3 (one launch of four slots, one masked), state-only and with
    t_params: nothing outside them is written, every element of the states and the tangents is, and hist at every live slot."""
    import torch
    from dhts import ops
    L, V, T, count = case
    p0, v0, par, head, _ = case_inputs(case)
    K = 3
    rng = np.random.default_rng(5)
    t_p, t_v = rng.standard_normal((2, K, L, V)).astype(np.float32)
    t_head, t_par = rng.standard_normal((K, L, 2)), rng.standard_normal((K, 6, L, V))
    desc = ops.micro_desc(L, V, DT)
    cnt = torch.tensor(count, device=cuda, dtype=torch.int32)
    live = J.live_mask(L, V, count)
    for want_params in (False, True):
        bufs = [guarded(s, cuda) for s in ((L, V), (L, V), (K, L, V), (K, L, V), (T, L, 2, V), (K, T, L, 2, V))]
        err, err_jvp = ops.new_error_record(cuda), ops.new_error_record(cuda)
        prim, tan = ops.micro_rollout_fwd_jvp(desc, T, torch.tensor(p0, device=cuda), torch.tensor(v0, device=cuda),
                                              torch.tensor(par, device=cuda, dtype=torch.float64),
                                              torch.tensor(head, device=cuda, dtype=torch.float64), torch.tensor(t_p, device=cuda),
                                              torch.tensor(t_v, device=cuda), count=cnt, t_head=torch.tensor(t_head, device=cuda),
                                              t_params=torch.tensor(t_par, device=cuda) if want_params else None, err=err,
                                              err_jvp=err_jvp, out=[b[1] for b in bufs])
        torch.cuda.synchronize()
        assert err.tolist()[0] == 0 and err_jvp.tolist()[0] == 0
        assert all(o is b[1] for o, b in zip(prim[:2] + tan[:2] + (prim[2], tan[2]), bufs))
        for i, (buf, view) in enumerate(bufs):
            b = buf.cpu().numpy()
            assert np.all(np.isnan(b[:256])) and np.all(np.isnan(b[b.size - 256:])), "a guard band was written (output %d)" % i
            inner = b[256:b.size - 256].reshape(view.shape)
            if i == 4:           # hist: the forward writes live slots only
                lt = np.broadcast_to(live[None, :, None, :], (T, L, 2, V))
                assert np.all(np.isfinite(inner[lt])) and np.all(np.isnan(inner[~lt]))
            else:
                assert np.all(np.isfinite(inner)), "an element was not written (output %d)" % i


# =================================================================================================================
# 7. no [T]-sized memory
# =================================================================================================================
def test_fused_allocates_nothing_of_size_t(cuda):
    """20 000 steps of two lanes of 64 vehicles, K = 2 with t_params, free-road heads: the peak of the fused call above the resident
    inputs stays below one eighth of the tape alone (30.7 MB; the taped path allocates it and 20.5 MB of parameter tape), and the
    results are the taped call's bits at that T."""
    import torch
    import dhts
    from dhts import ops
    L, V, T, K = 2, 64, 20000, 2
    rng = np.random.default_rng(41)
    p0, v0, par, head = lanes(rng, L, V)
    args = (torch.tensor(p0, device=cuda), torch.tensor(v0, device=cuda), torch.tensor(par, device=cuda, dtype=torch.float64),
            torch.tensor(head, device=cuda, dtype=torch.float64), T, DT)
    t_q = torch.tensor(rng.standard_normal((K, 6, L, V)), device=cuda)
    tape_bytes = ops.micro_tape_numel(ops.micro_desc(L, V, DT), T) * 4
    assert tape_bytes == T * L * V * 12
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    resident = torch.cuda.memory_allocated()
    fused = dhts.micro_rollout_jvp(*args, t_params=t_q, check_faults=False, fused=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - resident
    print("fused peak above the resident inputs: %d bytes; the tape alone: %d bytes" % (peak, tape_bytes))
    assert peak < tape_bytes // 8
    taped = dhts.micro_rollout_jvp(*args, t_params=t_q, check_faults=False)
    torch.cuda.synchronize()
    for a, b in zip(fused[0] + fused[1], taped[0] + taped[1]):
        assert same_bits(a.cpu().numpy(), b.cpu().numpy())


# =================================================================================================================
# 8. the example
# =================================================================================================================
def test_calibration_example_writes_the_same_log_fused(cuda, tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    logs = []
    for extra in ([], ["--fused"]):
        cwd = tmp_path / ("fused" if extra else "taped")
        cwd.mkdir()
        out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "calibrate_idm.py"), "--method", "lm", "--n_lane", "2",
                              "--n_vehicle", "8", "--n_step", "40", "--n_episode", "6"] + extra, cwd=str(cwd), env=env,
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        files = [os.path.join(dp, f) for dp, _, fs in os.walk(str(cwd)) for f in fs if f.startswith("trial_") and f.endswith(".txt")]
        assert len(files) == 1, "one trial_k.txt per run"
        logs.append(open(files[0]).read())
    assert len(logs[0].splitlines()) == 6
    assert logs[0] == logs[1], "the fused run's loss lines differ:\n%s\nagainst\n%s" % (logs[1], logs[0])
