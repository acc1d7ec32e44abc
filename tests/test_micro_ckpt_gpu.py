"""The checkpointed reverse mode of the IDM rollout on the device: dhts.micro_rollout(checkpoint=...) and the raw
ops.micro_rollout_fwd_ckpt / _bwd_ckpt against the taped path bit for bit, against the reference's goldens directly, the two fault records,
the memory it does not allocate, guard bands, and the calibration example.  Needs a real MI355X: python -m pytest tests -m gpu"""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_micro_jvp_gpu import CASES, DT, IDS, case_inputs, guarded
from test_micro_params import GOLDENS, golden_case, per_plane, restated
from test_micro_params_gpu import lanes
from util import TOL_GRAD, TOL_STATE, grad_report, rel_elem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRADS = ("g_p0", "g_v0", "g_head", "g_params")


def bits(a):
    """The bit pattern of a float32 or float64 array."""
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def run(cuda, p0, v0, par, head, T, dt, count=None, want_params=True, g_pT=None, g_vT=None, g_hist=None, tap=None, checkpoint=None,
        check_faults=True):
    """dhts.micro_rollout + backward of the given cotangents (or of test_micro_params_gpu.device_run's `tap` losses) -> numpy arrays."""
    import torch
    import dhts
    tp0 = torch.tensor(p0, device=cuda, requires_grad=True)
    tv0 = torch.tensor(v0, device=cuda, requires_grad=True)
    tpar = torch.tensor(par, device=cuda, dtype=torch.float64, requires_grad=want_params)
    thead = torch.tensor(head, device=cuda, dtype=torch.float64, requires_grad=True)
    cnt = None if count is None else torch.tensor(count, device=cuda, dtype=torch.int32)
    want_hist = tap == "every_sum" or g_hist is not None
    out = dhts.micro_rollout(tp0, tv0, tpar, thead, T, dt, count=cnt, want_hist=want_hist, check_faults=check_faults, checkpoint=checkpoint)
    pT, vT = out[0], out[1]
    if tap is None:
        loss = (pT * torch.tensor(g_pT, device=cuda)).sum() + (vT * torch.tensor(g_vT, device=cuda)).sum()
        if g_hist is not None:
            loss = loss + (out[2] * torch.tensor(g_hist, device=cuda)).sum()
    else:
        loss = out[2].sum() if tap == "every_sum" else 1e-4 * (pT ** 2).sum() + (vT ** 2).sum()
    loss.backward()
    torch.cuda.synchronize()
    n = lambda t: None if t is None else t.detach().cpu().numpy()      # noqa: E731
    return dict(pT=n(pT), vT=n(vT), hist=n(out[2]) if want_hist else None, g_p0=n(tp0.grad), g_v0=n(tv0.grad), g_head=n(thead.grad),
                g_params=n(tpar.grad))


def assert_same(tag, got, ref, live):
    """Outputs, hist at live slots (the forward leaves the rest unwritten) and every gradient, bit for bit."""
    for key in ("pT", "vT") + GRADS:
        if got[key] is None and ref[key] is None:
            continue
        assert got[key] is not None and ref[key] is not None, "%s: %s is missing on one side" % (tag, key)
        assert same_bits(got[key], ref[key]), "%s: %s differs from the taped path" % (tag, key)
    if ref["hist"] is not None:
        T, L, _, V = ref["hist"].shape
        assert got["hist"].shape == ref["hist"].shape
        lt = np.broadcast_to(live[None, :, None, :], (T, L, 2, V))
        assert same_bits(got["hist"][lt], ref["hist"][lt]), "%s: hist differs from the taped path at a live slot" % tag


def live_mask(L, V, count):
    return np.arange(V)[None, :] < np.array([V] * L if count is None else count)[:, None]


# =================================================================================================================
# 1. bit identity with the taped path
# =================================================================================================================
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_checkpointed_equals_the_taped_path_bit_for_bit(cuda, case):
    """Every shape of the tangent sweep's tests x S in {1, 3, the plan's, max_segment, one >= T clipped to max_segment} x
    params.requires_grad x cotangents on (pT, vT) alone and with a random g_hist: pT, vT, hist at live slots, g_p0, g_v0, g_head and
    g_params are dhts.micro_rollout(checkpoint=None)'s bits.  The taped result of a (params, hist) setting is computed once.  With 1024
    vehicles max_segment needs more than 64 KB of LDS."""
    from dhts import ops
    L, V, T, count = case
    p0, v0, par, head, _ = case_inputs(case)
    live = live_mask(L, V, count)
    rng = np.random.default_rng(1000 + 31 * V + T)
    g_pT, g_vT = rng.standard_normal((2, L, V)).astype(np.float32)
    g_hist = rng.standard_normal((T, L, 2, V)).astype(np.float32)
    desc = ops.micro_desc(L, V, DT)
    for want_params in (False, True):
        plan = ops.micro_ckpt_plan(desc, T, want_params)
        top = plan["max_segment"]
        segments = [1, 3, True, top, min(max(T, 1) + 2, top)]
        assert 3 <= top, "S = 3 runs for every case"
        if V == 1024:
            assert ops.micro_ckpt_plan(desc, T, want_params, top)["bwd_lds_bytes"] > 64 * 1024
        for gh in (None, g_hist):
            kw = dict(count=count, want_params=want_params, g_pT=g_pT, g_vT=g_vT, g_hist=gh)
            taped = run(cuda, p0, v0, par, head, T, DT, **kw)
            assert (taped["g_params"] is not None) == want_params
            for S in segments:
                got = run(cuda, p0, v0, par, head, T, DT, checkpoint=S, **kw)
                assert_same("%s S=%s params=%s hist=%s" % (IDS[CASES.index(case)], S, want_params, gh is not None), got, taped, live)


# =================================================================================================================
# 2. not resting on the taped path alone: the reference's goldens
# =================================================================================================================
@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_as_lanes_of_one_launch_checkpointed(cuda, golden_dir, name):
    """test_micro_params_gpu.test_goldens_as_lanes_of_one_launch with checkpoint=3, at that test's tolerances: the golden as lane 2 of a
    ragged launch, lane 2 against the reference's numbers, all lanes against the restatement."""
    c = golden_case(golden_dir, name)
    g, T, dt, tap = c["g"], c["T"], c["dt"], c["tap"]
    V = c["p0"].shape[1]
    k = V - 3
    p0, v0 = np.tile(c["p0"], (4, 1)), np.tile(c["v0"], (4, 1))
    par, head = np.tile(c["params"], (1, 4, 1)), np.tile(c["head"], (4, 1))
    p0[0, :k], v0[0, :k], par[:, 0, :k] = c["p0"][0, 3:], c["v0"][0, 3:], c["params"][:, 0, 3:]
    par[:5, 3, :] *= np.random.default_rng(3).uniform(0.9, 1.1, (5, V))
    count = [k, 0, V, V]
    d = run(cuda, p0, v0, par, head, T, dt, count=count, tap=tap, checkpoint=3)
    r = restated(p0, v0, par, head, T, dt, tap, count=count)
    assert np.all(np.isfinite(d["g_params"]))
    assert np.all(d["g_params"][:, 1, :] == 0) and np.all(d["g_params"][:, 0, k:] == 0)
    assert max(rel_elem(d["pT"], r["pT"]), rel_elem(d["vT"], r["vT"])) <= TOL_STATE
    for lane in (0, 2, 3):
        assert per_plane("%s lane %d checkpointed vs restatement" % (name, lane), d["g_params"][:, lane], r["g_params"][:, lane]) <= TOL_GRAD
    live = live_mask(4, V, count)
    assert grad_report("%s checkpointed vs restatement d loss / d p0" % name, d["g_p0"] * live, r["g_p0"] * live) <= TOL_GRAD
    assert grad_report("%s checkpointed vs restatement d loss / d v0" % name, d["g_v0"] * live, r["g_v0"] * live) <= TOL_GRAD
    assert per_plane("%s checkpointed vs golden" % name, d["g_params"][:, 2, :], g["g_params"].T) <= TOL_GRAD


# =================================================================================================================
# 3. the fault records
# =================================================================================================================
def test_collision_record_of_the_forward(cuda, capsys):
    """The fused kernel's construction -- a lane with two vehicles 1 m apart, the follower at 30 m/s --: the checkpointed forward's
    record is the taped forward's DHTS_FAULT_COLLISION (step 0, lane 1, vehicle 0), the operator prints it and goes on, and outputs and
    gradients are still the taped path's bits (the replay raises nothing again: the reverse sweep's record stays clean)."""
    import torch
    from dhts import _lib, ops
    L, V, T = 4, 70, 5
    rng = np.random.default_rng(2)
    p0, v0, par, head = lanes(rng, L, V)
    count = [70, 2, 70, 70]
    p0[1, :2], v0[1, :2] = (0.0, 1.0), (30.0, 10.0)
    desc = ops.micro_desc(L, V, DT)
    tp0, tv0 = torch.tensor(p0, device=cuda), torch.tensor(v0, device=cuda)
    tpar, thead = torch.tensor(par, device=cuda, dtype=torch.float64), torch.tensor(head, device=cuda, dtype=torch.float64)
    cnt = torch.tensor(count, device=cuda, dtype=torch.int32)
    records = []
    for S in (None, 2):
        err = ops.new_error_record(cuda)
        if S is None:
            tape = torch.empty(ops.micro_tape_numel(desc, T), dtype=torch.float32, device=cuda)
            ops.micro_rollout_fwd(desc, T, tp0, tv0, tpar, thead, count=cnt, tape=tape, err=err)
        else:
            ckpt = torch.empty(ops.micro_ckpt_numel(desc, T, S), dtype=torch.float32, device=cuda)
            ops.micro_rollout_fwd_ckpt(desc, T, tp0, tv0, tpar, thead, ckpt, count=cnt, segment=S, err=err)
            err_bwd = ops.new_error_record(cuda)
            ops.micro_rollout_bwd_ckpt(desc, T, ckpt, tpar, thead, torch.ones(L, V, device=cuda), torch.ones(L, V, device=cuda), count=cnt,
                                       segment=S, err=err_bwd)
            assert err_bwd.tolist()[0] in (0, _lib.FAULT_NAN), "the replay raises no collision"
        records.append(err.tolist())
    assert records[0] == [_lib.FAULT_COLLISION, 0, 1, 0] == records[1]
    g_pT, g_vT = rng.standard_normal((2, L, V)).astype(np.float32)
    g_hist = rng.standard_normal((T, L, 2, V)).astype(np.float32)
    capsys.readouterr()
    taped = run(cuda, p0, v0, par, head, T, DT, count=count, g_pT=g_pT, g_vT=g_vT, g_hist=g_hist)
    assert "Collision detected" in capsys.readouterr().out
    got = run(cuda, p0, v0, par, head, T, DT, count=count, g_pT=g_pT, g_vT=g_vT, g_hist=g_hist, checkpoint=2)      # prints, does not raise
    assert "Collision detected between vehicles (step 0, lane 1, vehicle 0)" in capsys.readouterr().out
    assert_same("collision", got, taped, live_mask(L, V, count))


def test_non_finite_cotangent_record_of_the_reverse_sweep(cuda):
    """A NaN in g_hist at step 9 of 20 with S = 4 (segments of steps 16-19, 12-15, 8-11, ...: step 9 is in the third segment the sweep
    takes and on no boundary of one): ops.micro_bwd_fault() gives the taped path's (step, lane, vehicle) = (9, 1, 7), and the gradients
    are identical as integer views (NaN payloads included)."""
    for want_params in (False, True):      # the state-only sweep, then the one with the parameter gradient
        import warnings
        import torch
        import dhts
        from dhts import ops
        L, V, T, S = 3, 70, 20, 4
        step, lane, veh = 9, 1, 7
        assert step // S < (T - 1) // S and step % S not in (0, S - 1)
        rng = np.random.default_rng(77)
        p0, v0, par, head = lanes(rng, L, V)
        count = [70, 41, 5]
        g_pT, g_vT = rng.standard_normal((2, L, V)).astype(np.float32)
        g_hist = rng.standard_normal((T, L, 2, V)).astype(np.float32)
        g_hist[step, lane, 1, veh] = np.nan
        out = []
        for ck in (None, S):
            tp0 = torch.tensor(p0, device=cuda, requires_grad=True)
            tv0 = torch.tensor(v0, device=cuda, requires_grad=True)
            tpar = torch.tensor(par, device=cuda, dtype=torch.float64, requires_grad=want_params)
            thead = torch.tensor(head, device=cuda, dtype=torch.float64, requires_grad=True)
            pT, vT, hist = dhts.micro_rollout(tp0, tv0, tpar, thead, T, DT, count=torch.tensor(count, device=cuda, dtype=torch.int32),
                                              want_hist=True, checkpoint=ck)
            torch.autograd.backward([pT, vT, hist], [torch.tensor(g_pT, device=cuda), torch.tensor(g_vT, device=cuda),
                                                     torch.tensor(g_hist, device=cuda)])
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                where = ops.micro_bwd_fault()
            assert any(issubclass(x.category, RuntimeWarning) for x in w)
            out.append((where, [t.grad.cpu().numpy() for t in (tp0, tv0, thead) + ((tpar,) if want_params else ())]))
        assert out[0][0] == (step, lane, veh) == out[1][0]
        assert np.isnan(out[0][1][1][lane, veh]) and np.all(np.isfinite(out[0][1][1][0]))
        for a, b in zip(out[0][1], out[1][1]):
            assert same_bits(a, b)


# =================================================================================================================
# 4. memory
# =================================================================================================================
def test_checkpointed_allocates_no_tape(cuda):
    """20 000 steps of two lanes of 64 vehicles, params requiring grad, no hist, the plan's segment: the peak of forward + backward above
    the resident inputs stays below one eighth of tape + parameter tape (30.7 MB + 20.5 MB, which the taped call allocates); the
    gradients are the taped call's bits; a backward over the retained graph leaves torch.cuda.memory_allocated() where it was and
    returns the same bits again."""
    import torch
    import dhts
    from dhts import ops
    L, V, T = 2, 64, 20000
    rng = np.random.default_rng(41)
    p0, v0, par, head = lanes(rng, L, V)
    g_pT, g_vT = (torch.tensor(a, device=cuda) for a in rng.standard_normal((2, L, V)).astype(np.float32))
    desc = ops.micro_desc(L, V, DT)
    tapes = ops.micro_tape_numel(desc, T) * 4 + ops.micro_param_tape_numel(desc, T) * 4
    assert ops.micro_tape_numel(desc, T) * 4 == T * L * V * 12

    def leaves():
        return (torch.tensor(p0, device=cuda, requires_grad=True), torch.tensor(v0, device=cuda, requires_grad=True),
                torch.tensor(par, device=cuda, dtype=torch.float64, requires_grad=True),
                torch.tensor(head, device=cuda, dtype=torch.float64, requires_grad=True))

    x = leaves()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    resident = torch.cuda.memory_allocated()
    pT, vT = dhts.micro_rollout(*x, T, DT, check_faults=False, checkpoint=True)
    loss = (pT * g_pT).sum() + (vT * g_vT).sum()
    first = torch.autograd.grad(loss, x, retain_graph=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - resident
    print("checkpointed forward + backward, peak above the resident inputs: %d bytes; tape + parameter tape: %d bytes" % (peak, tapes))
    assert peak < tapes // 8
    # a backward over the retained graph: into gradients that exist already, so nothing it allocates may stay
    for t, g in zip(x, first):
        t.grad = g.clone()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    loss.backward(retain_graph=True)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    for t, g in zip(x, first):
        assert same_bits(t.grad.cpu().numpy(), (g + g).cpu().numpy())      # (x + x is exact: the second sweep returned the first one's bits)
    second = torch.autograd.grad(loss, x, retain_graph=True)
    for a, b in zip(first, second):
        assert same_bits(a.cpu().numpy(), b.cpu().numpy())
    y = leaves()
    pT2, vT2 = dhts.micro_rollout(*y, T, DT, check_faults=False)
    taped = torch.autograd.grad((pT2 * g_pT).sum() + (vT2 * g_vT).sum(), y)
    assert same_bits(pT.detach().cpu().numpy(), pT2.detach().cpu().numpy()) and same_bits(vT.detach().cpu().numpy(), vT2.detach().cpu().numpy())
    for a, b in zip(first, taped):
        assert same_bits(a.cpu().numpy(), b.cpu().numpy())


# =================================================================================================================
# 5. guard bands
# =================================================================================================================
def test_guard_bands(cuda):
    """The raw wrappers at V = 65, T = 7, S = 3 with ragged counts: the checkpoint buffer, the outputs of both kernels and g_params in the
    middle of NaN-prefilled buffers.  Nothing outside them is written; every element of the states, the gradients and g_params is, hist at
    every live slot, and every slot below V of every checkpoint row."""
    for want_params in (False, True):      # the state-only sweep, then the one with the parameter gradient
        import torch
        from dhts import ops
        L, V, T, S = 3, 65, 7, 3
        count = [65, 1, 64]
        rng = np.random.default_rng(5)
        p0, v0, par, head = lanes(rng, L, V)
        desc = ops.micro_desc(L, V, DT)
        cnt = torch.tensor(count, device=cuda, dtype=torch.int32)
        tpar, thead = torch.tensor(par, device=cuda, dtype=torch.float64), torch.tensor(head, device=cuda, dtype=torch.float64)
        live = live_mask(L, V, count)
        n_ck = ops.micro_ckpt_numel(desc, T, S)
        assert n_ck == 3 * L * 128 * 2
        ck_buf, ck = guarded((n_ck,), cuda)
        f_bufs = [guarded(s, cuda) for s in ((L, V), (L, V), (T, L, 2, V))]
        err = ops.new_error_record(cuda)
        pT, vT = ops.micro_rollout_fwd_ckpt(desc, T, torch.tensor(p0, device=cuda), torch.tensor(v0, device=cuda), tpar, thead, ck, count=cnt,
                                            segment=S, hist=f_bufs[2][1], err=err, out=(f_bufs[0][1], f_bufs[1][1]))
        assert pT is f_bufs[0][1] and vT is f_bufs[1][1]
        b_bufs = [guarded(s, cuda) for s in ((L, V), (L, V))]
        gq_buf = torch.full((6 * L * V + 64,), float("nan"), dtype=torch.float64, device=cuda)
        g_params = gq_buf[32:32 + 6 * L * V].view(6, L, V) if want_params else None
        g_head = torch.full((L, 2), float("nan"), dtype=torch.float64, device=cuda)
        err_bwd = ops.new_error_record(cuda)
        g_pT, g_vT = (torch.tensor(a, device=cuda) for a in rng.standard_normal((2, L, V)).astype(np.float32))
        g_hist = torch.tensor(rng.standard_normal((T, L, 2, V)).astype(np.float32), device=cuda)
        ops.micro_rollout_bwd_ckpt(desc, T, ck, tpar, thead, g_pT, g_vT, count=cnt, segment=S, g_hist=g_hist, err=err_bwd,
                                   out=(b_bufs[0][1], b_bufs[1][1]), g_head=g_head, g_params=g_params)
        torch.cuda.synchronize()
        assert err.tolist()[0] == 0 and err_bwd.tolist()[0] == 0
        for i, (buf, view) in enumerate([(ck_buf, ck)] + f_bufs + b_bufs):
            b = buf.cpu().numpy()
            assert np.all(np.isnan(b[:256])) and np.all(np.isnan(b[b.size - 256:])), "a guard band was written (buffer %d)" % i
            inner = b[256:b.size - 256].reshape(view.shape)
            if i == 0:               # rows [3][L][128] of (p, v): slots below V written, the padding of a row never
                rows = inner.reshape(3, L, 128, 2)
                assert np.all(np.isfinite(rows[:, :, :V])) and np.all(np.isnan(rows[:, :, V:]))
                assert same_bits(rows[0, :, :V, 0], p0) and same_bits(rows[0, :, :V, 1], v0), "row 0 is the initial state"
            elif i == 3:             # hist: the forward writes live slots only
                lt = np.broadcast_to(live[None, :, None, :], (T, L, 2, V))
                assert np.all(np.isfinite(inner[lt])) and np.all(np.isnan(inner[~lt]))
            else:
                assert np.all(np.isfinite(inner)), "an element was not written (buffer %d)" % i
        assert bool(torch.all(torch.isfinite(g_head)))
        q = gq_buf.cpu().numpy()
        if want_params:
            assert np.all(np.isnan(q[:32])) and np.all(np.isnan(q[-32:])) and np.all(np.isfinite(q[32:-32]))
        else:
            assert np.all(np.isnan(q))
        # and they are the taped pair's bits
        taped = run(cuda, p0, v0, par, head, T, DT, count=count, want_params=want_params, g_pT=g_pT.cpu().numpy(), g_vT=g_vT.cpu().numpy(),
                    g_hist=g_hist.cpu().numpy())
        got = dict(pT=pT.cpu().numpy(), vT=vT.cpu().numpy(), hist=f_bufs[2][1].cpu().numpy(), g_p0=b_bufs[0][1].cpu().numpy(),
                   g_v0=b_bufs[1][1].cpu().numpy(), g_head=g_head.cpu().numpy(), g_params=g_params.cpu().numpy() if want_params else None)
        assert_same("raw wrappers", got, taped, live)


# =================================================================================================================
# 6. the example
# =================================================================================================================
def test_calibration_example_writes_the_same_log_checkpointed(cuda, tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    logs = []
    for extra in ([], ["--checkpoint", "4"]):
        cwd = tmp_path / ("checkpointed" if extra else "taped")
        cwd.mkdir()
        out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "calibrate_idm.py"), "--seed", "1", "--n_lane", "8",
                              "--n_vehicle", "16", "--n_step", "50", "--n_episode", "5"] + extra, cwd=str(cwd), env=env,
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        files = [os.path.join(dp, f) for dp, _, fs in os.walk(str(cwd)) for f in fs if f.startswith("trial_") and f.endswith(".txt")]
        assert len(files) == 1, "one trial_k.txt per run"
        logs.append(open(files[0]).read())
    assert len(logs[0].splitlines()) == 5
    assert logs[0] == logs[1], "the checkpointed run's loss lines differ:\n%s\nagainst\n%s" % (logs[1], logs[0])
