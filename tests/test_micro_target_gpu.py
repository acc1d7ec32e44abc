"""The trajectory-fit loss inside the checkpointed micro rollout on the device: dhts.micro_rollout(target=, checkpoint=) returns
(pT, vT, sse) and differentiates sse without a dense history or a cotangent of one.  The yardstick everywhere is existing code on the
same inputs, never the code under test: dhts.micro_rollout(want_hist=True, checkpoint=S) -- with a recorded leader the existing lead
form with probes=range(V), every=1 -- whose dense history H carries the loss written in torch.  Then missing observations, the no-grad
forward, the memory that is not allocated, the float64 restatement, the raw entry points and the calibration example.
Needs a real MI355X: python -m pytest tests -m gpu"""
import os
import subprocess
import sys

import numpy as np
import pytest

from micro_lead_ref import lead_rollout
from test_micro_ckpt_gpu import live_mask, same_bits
from test_micro_jvp_gpu import CASES, DT, IDS, case_inputs
from test_micro_lead_gpu import moving_leaders
from test_micro_params import lane_rollout, per_plane
from test_micro_params_gpu import lanes
from util import TOL_GRAD, grad_report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the shapes of tests/test_micro_samples_gpu.py: wavefront edges, empty and one-vehicle lanes, several wavefronts per lane, the largest
# block, T = 0
SHAPES = [c for c in CASES if (c[0], c[1], c[2]) in ((3, 1, 3), (3, 2, 7), (3, 64, 50), (3, 65, 1), (5, 130, 50), (3, 1024, 20), (3, 70, 0))]
SHAPE_IDS = [IDS[CASES.index(c)] for c in SHAPES]
PATTERNS = ("dense", "all_nan", "steps", "entries")


def n(t):
    return None if t is None else t.detach().cpu().numpy()


def make_target(rng, hist, live, pattern):
    """An observed trajectory around the dense history `hist` [T][L][2][V] (numpy): the history plus noise, then the missing
    observations of `pattern`, then garbage (NaN and 1e30, alternating) at every slot at or beyond count, which nothing may read.
      dense     every live entry observed
      all_nan   nothing observed
      steps     whole steps missing: 0, 2, 3, 4 (around the boundaries of S = 3 and of S = 4), 7, 8, 12 (boundaries of 4, 8 and of the
                longer plans' segments), T - 2 and T - 1
      entries   a tenth of the (p, v) pairs missing, a tenth of the p alone and a tenth of the v alone"""
    T, L, _, V = hist.shape
    noise = rng.standard_normal(hist.shape).astype(np.float32)
    noise[:, :, 0] *= 5.0
    noise[:, :, 1] *= 2.0
    with np.errstate(all="ignore"):                  # (a history holds whatever its buffer held at slots at or beyond count)
        target = (hist + noise).astype(np.float32)
    if pattern == "all_nan":
        target[:] = np.nan
    elif pattern == "steps":
        for t in (0, 2, 3, 4, 7, 8, 12, T - 2, T - 1):
            if 0 <= t < T:
                target[t] = np.nan
    elif pattern == "entries":
        u = rng.uniform(size=(T, L, V))
        target[:, :, 0][u < 0.2] = np.nan
        target[:, :, 1][(u < 0.1) | ((u >= 0.2) & (u < 0.3))] = np.nan
    dead = np.broadcast_to(~live[None, :, None, :], target.shape)
    garbage = np.where((np.arange(target.size).reshape(target.shape) % 2) == 0, np.float32(np.nan), np.float32(1e30))
    return np.where(dead, garbage, target).astype(np.float32)


def expected_sse(hist, target, live):
    """sum over observed live entries of the float32 residual squared in double, per lane and component: [L][2] float64, and the
    number of terms the longest of the sums has."""
    with np.errstate(all="ignore"):
        r = (hist - target).astype(np.float32).astype(np.float64) ** 2
    seen = ~np.isnan(target) & live[None, :, None, :]
    return np.where(seen, r, 0.0).sum(axis=(0, 3)), seen


def assert_sse(tag, got, hist, target, live):
    """Each term is exact in double (a float32 squared has 48 bits), so only the order of the N = T V non-negative additions differs
    between two summations: |got - want| <= N 2^-52 want.  Exactly 0 where nothing is observed."""
    want, seen = expected_sse(hist, target, live)
    T, _, _, V = hist.shape
    assert got.shape == want.shape and got.dtype == np.float64, tag
    err = np.abs(got - want)
    bound = T * V * 2.0 ** -52 * want
    print("%s: sse max |got - want| / want = %.2e (bound %.2e)" % (tag, float(np.max(err / np.maximum(want, 1e-300))), T * V * 2.0 ** -52))
    assert np.all(err <= bound), "%s: sse %s against %s" % (tag, got, want)
    nothing = ~seen.any(axis=(0, 3))
    assert np.all(got[nothing] == 0), "%s: sse is not exactly 0 where nothing is observed" % tag


class Device:
    """The inputs of a case on the device, uploaded once, in the head form (a constant head gap) or with a recorded leader."""

    def __init__(self, cuda, case, with_lead):
        import torch
        self.L, self.V, self.T, self.count = case
        self.cuda, self.with_lead = cuda, with_lead
        self.p0, self.v0, self.par, self.head, _ = case_inputs(case)
        self.cnt = None if self.count is None else torch.tensor(self.count, device=cuda, dtype=torch.int32)
        self.live = live_mask(self.L, self.V, self.count)
        rng = np.random.default_rng(977 + 31 * self.V + self.T)
        self.lead = moving_leaders(rng, self.p0, self.count, self.V, self.T)
        self.lead_len = torch.tensor(rng.uniform(4.0, 7.0, self.L), device=cuda, dtype=torch.float64)
        boundary = torch.tensor(self.lead, device=cuda) if with_lead else torch.tensor(self.head, device=cuda, dtype=torch.float64)
        self.base = (torch.tensor(self.p0, device=cuda), torch.tensor(self.v0, device=cuda),
                     torch.tensor(self.par, device=cuda, dtype=torch.float64), boundary)

    def leaves(self, want_params, grad=True):
        return tuple(t.clone().requires_grad_(grad and (want_params or i != 2)) for i, t in enumerate(self.base))

    def call(self, x, checkpoint, target=None, dense=False):
        """-> (pT, vT, third): third is sse with target, the dense history H with dense, else absent."""
        import dhts
        p, v, par, b = x
        kw = dict(count=self.cnt, checkpoint=checkpoint)
        if self.with_lead:
            kw.update(lead=b, lead_length=self.lead_len)
            b = None
            if dense:
                kw.update(probes=list(range(self.V)), every=1)
        elif dense:
            kw.update(want_hist=True)
        if target is not None:
            kw.update(target=target)
        return dhts.micro_rollout(p, v, par, b, self.T, DT, **kw)

    def grads(self, x):
        return dict(g_p0=n(x[0].grad), g_v0=n(x[1].grad), g_params=n(x[2].grad), g_boundary=n(x[3].grad))

    def yardstick(self, want_params, S, g_pT, g_vT, g_sse, target):
        """Existing code alone: the dense history H of the checkpointed rollout and the loss written on it in torch with the dense
        cotangent G = where(isnan(target), 0, (2 g_sse).float()[l][c] (H - target)), zero at slots at or beyond count."""
        import torch
        x = self.leaves(want_params)
        pT, vT, H = self.call(x, S, dense=True)
        loss = (pT * g_pT).sum() + (vT * g_vT).sum()
        if target is not None:
            live = torch.tensor(self.live, device=self.cuda)[None, :, None, :]
            G = (2 * g_sse).float()[None, :, :, None] * (H.detach() - target)
            G = torch.where(torch.isnan(target) | ~live, torch.zeros((), device=self.cuda), G)
            loss = loss + (H * G).sum()
        loss.backward()
        return dict(pT=n(pT), vT=n(vT), hist=n(H), **self.grads(x))

    def fitted(self, want_params, S, g_pT, g_vT, g_sse, target):
        x = self.leaves(want_params)
        pT, vT, sse = self.call(x, S, target=target)
        ((pT * g_pT).sum() + (vT * g_vT).sum() + (sse * g_sse).sum()).backward()
        return dict(pT=n(pT), vT=n(vT), sse=n(sse), **self.grads(x))


def compare_with_the_yardstick(cuda, case, with_lead, patterns):
    import torch
    from dhts import ops
    d = Device(cuda, case, with_lead)
    L, V, T = d.L, d.V, d.T
    rng = np.random.default_rng(4000 + 31 * V + T + (7 if with_lead else 0))
    g_pT, g_vT = (torch.tensor(a, device=cuda) for a in rng.standard_normal((2, L, V)).astype(np.float32))
    g_sse = torch.tensor(rng.standard_normal((L, 2)), device=cuda)
    desc = ops.micro_desc(L, V, DT)
    hist = d.yardstick(False, True, g_pT, g_vT, g_sse, None)["hist"]
    assert hist.shape == (T, L, 2, V)
    for pattern in patterns:
        tgt = make_target(rng, hist, d.live, pattern)
        target = torch.tensor(tgt, device=cuda)
        for want_params in (False, True):
            plan = ops.micro_ckpt_target_plan(desc, T, want_params)
            top = plan["max_segment"]
            assert top >= 3
            want = d.yardstick(want_params, True, g_pT, g_vT, g_sse, target)
            m = np.broadcast_to(d.live[None, :, None, :], hist.shape)      # (the history is written at live slots only)
            assert same_bits(want["hist"][m], hist[m])
            first = None
            for S in (1, 3, True, top):
                tag = "%s%s %s params=%s S=%s" % (IDS[CASES.index(case)], " lead" if with_lead else "", pattern, want_params, S)
                got = d.fitted(want_params, S, g_pT, g_vT, g_sse, target)
                assert same_bits(got["pT"], want["pT"]) and same_bits(got["vT"], want["vT"]), tag
                assert_sse(tag, got["sse"], hist, tgt, d.live)
                if first is None:
                    first = got["sse"]
                    assert same_bits(d.fitted(want_params, S, g_pT, g_vT, g_sse, target)["sse"], first), "%s: two runs differ" % tag
                assert same_bits(got["sse"], first), "%s: sse depends on the segment" % tag
                assert (got["g_params"] is not None) == want_params
                for key in ("g_p0", "g_v0", "g_boundary", "g_params"):
                    if got[key] is not None:
                        assert got[key].shape == want[key].shape and got[key].dtype == want[key].dtype
                        assert np.array_equal(got[key], want[key]), "%s: %s differs from the dense yardstick" % (tag, key)
                if pattern == "all_nan":
                    assert np.all(got["sse"] == 0)
            if pattern == "all_nan":
                # nothing observed: the gradients of a call without target whose loss is on pT, vT alone
                x = d.leaves(want_params)
                pT, vT = d.call(x, 3)[:2]
                ((pT * g_pT).sum() + (vT * g_vT).sum()).backward()
                plain = d.grads(x)
                for key, a in plain.items():
                    if a is not None:
                        assert np.array_equal(got[key], a), "%s: %s differs from the call without target" % (tag, key)


# =================================================================================================================
# 1. - 4. state, sse, gradients and missing data against the dense yardstick
# =================================================================================================================
@pytest.mark.parametrize("case", SHAPES, ids=SHAPE_IDS)
def test_target_equals_the_dense_yardstick(cuda, case):
    """params.requires_grad x S in {1, 3, the plan's, max_segment} x every pattern of missing observations, random cotangents on pT,
    vT and sse, garbage in target at every slot at or beyond count: pT, vT bit for bit; sse within N 2^-52 of the float64 sum over
    the yardstick's history, the same bits in two runs and for every S; g_p0, g_v0, g_head and g_params equal the yardstick's as numbers
    (np.array_equal: a +0.0 that one path adds and the other does not can flip the sign of a zero and nothing else)."""
    compare_with_the_yardstick(cuda, case, False, PATTERNS)


@pytest.mark.parametrize("case", SHAPES, ids=SHAPE_IDS)
def test_target_with_a_recorded_leader_equals_the_dense_yardstick(cuda, case):
    """The same with lead= and lead_length=: the yardstick is the existing lead form observed at every slot and step; g_lead too."""
    compare_with_the_yardstick(cuda, case, True, ("dense", "all_nan", "entries"))


# =================================================================================================================
# 5. the forward that nobody differentiates
# =================================================================================================================
@pytest.mark.parametrize("with_lead", (False, True))
def test_forward_without_grad_keeps_no_checkpoint(cuda, with_lead):
    """No leaf requires grad: sse has the bits of the differentiated call, and what the call leaves allocated is its three outputs
    (pT, vT, sse) and its fault record -- less than the checkpoint buffer the differentiated call keeps."""
    import torch
    from dhts import ops
    case = SHAPES[4]
    d = Device(cuda, case, with_lead)
    L, V, T = d.L, d.V, d.T
    rng = np.random.default_rng(5)
    hist = d.yardstick(False, True, torch.zeros(L, V, device=cuda), torch.zeros(L, V, device=cuda), None, None)["hist"]
    tgt = make_target(rng, hist, d.live, "entries")
    target = torch.tensor(tgt, device=cuda)
    S = 2
    with_grad = d.call(d.leaves(True), S, target=target)
    x = d.leaves(False, grad=False)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    out = d.call(x, S, target=target)
    torch.cuda.synchronize()
    kept = torch.cuda.memory_allocated() - before
    assert all(o.grad_fn is None and not o.requires_grad for o in out)
    assert same_bits(n(out[2]), n(with_grad[2])) and same_bits(n(out[0]), n(with_grad[0])) and same_bits(n(out[1]), n(with_grad[1]))
    assert_sse("no grad", n(out[2]), hist, tgt, d.live)
    ckpt_bytes = 4 * ops.micro_ckpt_numel(ops.micro_desc(L, V, DT), T, S)
    print("no-grad forward keeps %d bytes; the checkpoint buffer would be %d" % (kept, ckpt_bytes))
    assert ckpt_bytes > 3 * 4096 and kept <= 2 * L * V * 4 + 3 * 4096 < ckpt_bytes        # (the allocator rounds small blocks up to 512 B)


# =================================================================================================================
# 6. memory
# =================================================================================================================
def test_target_allocates_no_history(cuda):
    """64 lanes of 256 vehicles, 400 steps, params requiring grad: one dense history is T L 2 V 4 = 52 MB.  The peak of forward +
    backward above the resident inputs (target among them: it is the data) stays under half of one history with target=; the
    yardstick -- want_hist=True, the loss in torch -- is above two."""
    import torch
    import dhts
    L, V, T = 64, 256, 400
    rng = np.random.default_rng(43)
    p0, v0, par, head = lanes(rng, L, V)
    dense = T * L * 2 * V * 4
    target = torch.tensor(rng.standard_normal((T, L, 2, V)).astype(np.float32), device=cuda)
    peaks = []
    for fused in (True, False):
        x = (torch.tensor(p0, device=cuda, requires_grad=True), torch.tensor(v0, device=cuda, requires_grad=True),
             torch.tensor(par, device=cuda, dtype=torch.float64, requires_grad=True),
             torch.tensor(head, device=cuda, dtype=torch.float64, requires_grad=True))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        resident = torch.cuda.memory_allocated()
        if fused:
            out = dhts.micro_rollout(*x, T, DT, check_faults=False, checkpoint=True, target=target)
            loss = out[2].sum() / target.numel()
        else:
            out = dhts.micro_rollout(*x, T, DT, check_faults=False, checkpoint=True, want_hist=True)
            loss = ((out[2] - target) ** 2).mean()
        loss.backward()
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - resident)
        assert all(bool(torch.all(torch.isfinite(t.grad))) for t in x)
        del out, loss, x
    print("forward + backward, peak above the resident inputs: target= %d bytes, want_hist %d bytes; one dense history %d bytes"
          % (peaks[0], peaks[1], dense))
    assert peaks[0] < dense // 2
    assert peaks[1] > 2 * dense


# =================================================================================================================
# 7. independent semantics: the float64 restatement
# =================================================================================================================
@pytest.mark.parametrize("with_lead", (False, True))
def test_gradient_of_sse_against_the_restated_rollout(cuda, with_lead):
    """loss = sse.sum() against tests/test_micro_params.py::lane_rollout (with a leader tests/micro_lead_ref.py::lead_rollout), the
    float64 torch restatements the CPU tests validate against the C oracle, differentiated by autograd on the CPU: gradients at
    TOL_GRAD, g_params plane by plane.  Collision-free lanes (test_micro_params_gpu.lanes), 20 steps: no vehicle meets a clip.  The
    observations lie 5 m and 2 m/s (one sigma) off the trajectory, so that a residual is large against the float32 spacing of the
    state it is formed from (6e-5 m at 1000 m) and both sides differentiate the same numbers."""
    import torch
    import dhts
    L, V, T = 3, 70, 20
    count = [70, 41, 5]
    rng = np.random.default_rng(71)
    p0, v0, par, head = lanes(rng, L, V)
    live = live_mask(L, V, count)
    lead = moving_leaders(rng, p0, count, V, T)
    lead_len = np.array([6.5, 4.0, 5.5])
    c = [torch.tensor(p0, requires_grad=True), torch.tensor(v0, requires_grad=True), torch.tensor(par, requires_grad=True),
         torch.tensor(lead if with_lead else head, requires_grad=True)]
    if with_lead:
        _, _, hist = lead_rollout(c[0], c[1], c[2], c[3], T, DT, count=count, lead_length=lead_len)
    else:
        _, _, hist = lane_rollout(c[0], c[1], c[2], c[3], T, DT, count=count)
    tgt = make_target(rng, hist.detach().numpy(), live, "entries")
    seen = torch.tensor(~np.isnan(tgt) & live[None, :, None, :])
    r = hist.double() - torch.tensor(np.where(np.isnan(tgt) | ~live[None, :, None, :], 0.0, tgt).astype(np.float64))
    ref_loss = (torch.where(seen, r, torch.zeros((), dtype=torch.float64)) ** 2).sum()
    ref_loss.backward()
    x = [t.detach().to(cuda).requires_grad_(True) for t in c]
    kw = dict(lead=x[3], lead_length=torch.tensor(lead_len, device=cuda)) if with_lead else {}
    pT, vT, sse = dhts.micro_rollout(x[0], x[1], x[2], None if with_lead else x[3], T, DT, checkpoint=3,
                                     count=torch.tensor(count, device=cuda, dtype=torch.int32), target=torch.tensor(tgt, device=cuda), **kw)
    sse.sum().backward()
    loss = float(sse.detach().sum())
    e_loss = abs(loss - float(ref_loss.detach())) / float(ref_loss.detach())
    print("lead=%s: loss %.9g against the restatement's %.9g (%.2e)" % (with_lead, loss, float(ref_loss.detach()), e_loss))
    assert e_loss <= TOL_GRAD
    assert grad_report("sse d loss / d p0", n(x[0].grad), c[0].grad.numpy()) <= TOL_GRAD
    assert grad_report("sse d loss / d v0", n(x[1].grad), c[1].grad.numpy()) <= TOL_GRAD
    assert grad_report("sse d loss / d %s" % ("lead" if with_lead else "head"), n(x[3].grad), c[3].grad.numpy()) <= TOL_GRAD
    assert per_plane("sse", n(x[2].grad), c[2].grad.numpy()) <= TOL_GRAD
    assert np.any(n(x[3].grad) != 0)


# =================================================================================================================
# 8. the raw entry points
# =================================================================================================================
def test_raw_entry_points_reject_and_launch(cuda):
    """DHTS_E_INVALID for each contradictory or missing argument, with real device buffers; a launch at T = 0 succeeds in both forms,
    copies the state, zeroes sse and leaves the gradients of a rollout of no steps."""
    import ctypes as C
    import torch
    from dhts import _lib, ops
    lib = _lib.lib()
    L, V, T, S = 3, 70, 5, 2
    rng = np.random.default_rng(3)
    p0, v0, par, head = lanes(rng, L, V)
    desc = ops.micro_desc(L, V, DT)
    tp0, tv0 = torch.tensor(p0, device=cuda), torch.tensor(v0, device=cuda)
    tpar, thead = torch.tensor(par, device=cuda, dtype=torch.float64), torch.tensor(head, device=cuda, dtype=torch.float64)
    lead = torch.tensor(moving_leaders(rng, p0, None, V, T), device=cuda)
    target = torch.zeros(T, L, 2, V, device=cuda)
    sse = torch.full((L, 2), -1.0, dtype=torch.float64, device=cuda)
    ckpt = torch.empty(ops.micro_ckpt_numel(desc, T, S), dtype=torch.float32, device=cuda)
    out = [torch.empty(L, V, device=cuda) for _ in range(4)]
    g_head, g_lead = torch.zeros(L, 2, dtype=torch.float64, device=cuda), torch.empty(T, L, 2, device=cuda)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    top = ops.micro_ckpt_target_plan(desc, T)["max_segment"]

    def fwd(T_, S_, head_, lead_, target_, sse_=sse):
        return lib.dhts_micro_rollout_fwd_ckpt_target(C.byref(desc), T_, S_, P(tp0), P(tv0), None, P(tpar), P(head_), P(lead_), None,
                                                      P(out[0]), P(out[1]), P(ckpt), P(target_), P(sse_), None, stream)

    def bwd(T_, S_, head_, lead_, target_, g_head_, g_lead_, ckpt_=ckpt):
        return lib.dhts_micro_rollout_bwd_ckpt_target(C.byref(desc), T_, S_, P(ckpt_), None, P(tpar), P(head_), P(lead_), None, P(tp0),
                                                      P(tv0), P(target_), None, P(out[2]), P(out[3]), P(g_head_), P(g_lead_), None, None,
                                                      stream)
    assert fwd(T, S, thead, lead, target) == _lib.E_INVALID            # both
    assert fwd(T, S, None, None, target) == _lib.E_INVALID             # neither
    assert fwd(T, S, thead, None, None) == _lib.E_INVALID              # no target with T > 0
    assert fwd(T, S, thead, None, target, None) == _lib.E_INVALID      # no sse
    assert fwd(T, top + 1, thead, None, target) == _lib.E_INVALID      # a segment the ring cannot hold
    assert bwd(T, S, thead, lead, target, g_head, None) == _lib.E_INVALID
    assert bwd(T, S, None, None, target, None, None) == _lib.E_INVALID
    assert bwd(T, S, thead, None, None, g_head, None) == _lib.E_INVALID
    assert bwd(T, S, thead, None, target, g_head, None, None) == _lib.E_INVALID      # no checkpoints with T > 0
    assert bwd(T, S, None, lead, target, None, None) == _lib.E_INVALID               # a leader without g_lead
    assert bwd(T, S, None, lead, target, g_head, g_lead) == _lib.E_INVALID           # a leader and g_head
    assert bwd(T, top + 1, thead, None, target, g_head, None) == _lib.E_INVALID
    torch.cuda.synchronize()
    assert bool(torch.all(sse == -1.0)), "a rejected call wrote"
    # T = 0: both forms launch
    for head_, lead_ in ((thead, None), (None, None)):
        sse.fill_(-1.0)
        assert fwd(0, 0, head_, lead_, None) == 0
        assert bwd(0, 0, head_, lead_, None, g_head if head_ is not None else None, None, None) == 0
        torch.cuda.synchronize()
        assert bool(torch.all(sse == 0)) and same_bits(n(out[0]), p0) and same_bits(n(out[1]), v0)
        assert same_bits(n(out[2]), p0) and same_bits(n(out[3]), v0)           # (the cotangents handed in were p0, v0)
    # ... and the wrappers run a short fit through both
    pT, vT, s = ops.micro_rollout_fwd_ckpt_target(desc, T, tp0, tv0, tpar, ckpt, target, head=thead, segment=S)
    g = ops.micro_rollout_bwd_ckpt_target(desc, T, ckpt, tpar, tp0, tv0, target, g_sse=torch.ones(L, 2, dtype=torch.float64, device=cuda),
                                          head=thead, segment=S)
    assert bool(torch.all(s > 0)) and all(bool(torch.all(torch.isfinite(t))) for t in g)


# =================================================================================================================
# 9. the example
# =================================================================================================================
@pytest.mark.parametrize("leader", (False, True), ids=("head_gap", "leader"))
def test_calibration_example_fits_with_the_fused_loss(cuda, tmp_path, leader):
    """examples/calibrate_idm.py --checkpoint with and without --fused-loss on a tiny problem, same seed.  The two runs differ in the
    summation of the loss alone -- float32 torch.mean against the kernels' float64 sums --, so (a) the first logged loss, taken at the
    same parameters, agrees within the bound of ANY order of a float32 sum of N = T L 2 V non-negative terms, (N + 2) 2^-24 relative
    (two roundings more for the float32 subtraction and square), and (b) the final parameter error agrees to the digits the example
    prints (three decimals).  The largest relative difference of any logged figure is printed, not asserted."""
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    logs, printed = [], []
    n_lane, n_vehicle, n_step = 8, 16, 50
    for extra in ([], ["--fused-loss"]):
        cwd = tmp_path / ("fused" if extra else "dense")
        cwd.mkdir()
        out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "calibrate_idm.py"), "--seed", "1", "--n_lane", str(n_lane),
                              "--n_vehicle", str(n_vehicle), "--n_step", str(n_step), "--n_episode", "5", "--checkpoint", "4"]
                             + (["--leader"] if leader else []) + extra, cwd=str(cwd), env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        files = [os.path.join(dp, f) for dp, _, fs in os.walk(str(cwd)) for f in fs if f.startswith("trial_") and f.endswith(".txt")]
        assert len(files) == 1, "one trial_k.txt per run"
        logs.append([[float(w) for w in line.split()] for line in open(files[0]).read().splitlines()])
        printed.append([line for line in out.stdout.splitlines() if line.startswith("Trial # 0")][0])
    assert len(logs[0]) == len(logs[1]) == 5 and all(len(a) == len(b) == 2 for a, b in zip(*logs))
    worst = max(abs(a - b) / max(abs(a), 1e-30) for la, lb in zip(*logs) for a, b in zip(la, lb))
    first = abs(logs[0][0][1] - logs[1][0][1]) / logs[0][0][1]
    print("leader=%s: first loss differs by %.2e relative; largest relative difference of a logged figure %.2e\n%s\n%s"
          % (leader, first, worst, printed[0], printed[1]))
    assert logs[0][0][0] == logs[1][0][0], "the first parameter error is the initial guess's"
    assert first <= (n_step * n_lane * 2 * n_vehicle + 2) * 2.0 ** -24
    final = [line.split("parameter error")[1].split("in")[0] for line in printed]
    assert final[0] == final[1], "the final parameter error as printed: %s against %s" % (printed[1], printed[0])
