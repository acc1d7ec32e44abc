"""Probe samples of the micro rollout on the device: dhts.micro_rollout(probes=, every=) with checkpoint= and
dhts.micro_rollout_jvp(probes=, every=, fused=True) write and read samples [T // every][L][2][P] from their kernels, without a dense
history.  The yardstick everywhere is the existing dense path -- want_hist=True on the same inputs, cut as hist[E - 1::E][..., probes],
the loss written on that cut -- never the code under test.  Then the taped paths' glue, guard bands and raw probe indices, the memory
that is not allocated, the fault records and the calibration example.  Needs a real MI355X: python -m pytest tests -m gpu"""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_micro_ckpt_gpu import live_mask, same_bits
from test_micro_jvp_gpu import CASES, DT, IDS, LEAVES, case_inputs, directions, guarded
from test_micro_params_gpu import lanes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# wavefront edges, empty and one-vehicle lanes, several wavefronts per lane, the largest block, T = 0
SHAPES = [c for c in CASES if (c[0], c[1], c[2]) in ((3, 1, 3), (3, 2, 7), (3, 64, 50), (3, 65, 1), (5, 130, 50), (3, 1024, 20), (3, 70, 0))]
SHAPE_IDS = [IDS[CASES.index(c)] for c in SHAPES]
GRADS = ("g_p0", "g_v0", "g_head", "g_params")


def everies(T):
    """1 and 2 (the reverse sweep's two rows of prefetch), 3 and 7 (no divisors of most T), T (one row), T + 1 (no row)."""
    return sorted(e for e in {1, 2, 3, 7, T, T + 1} if e >= 1)


def probe_lists(V):
    """Every slot without a list; the tail vehicle; the last slot; a list that has, on the ragged lanes, slots at or beyond count; every
    slot as a list."""
    out = [None, [0], [V - 1], sorted({0, V // 3, V // 2, V - 1}), list(range(V))]
    return [p for i, p in enumerate(out) if p not in out[:i]]


def settings(T, V):
    """(every, probes) of a sampled call: all of them but (1, None), which is the un-sampled call by definition."""
    return [(e, p) for e in everies(T) for p in probe_lists(V) if not (e == 1 and p is None)]


def cut(hist, probes, every):
    """The yardstick's samples of a dense numpy history [..][T][L][2][V]."""
    c = hist[..., every - 1::every, :, :, :]
    return c if probes is None else c[..., probes]


class Device:
    """The inputs of a case on the device, uploaded once; leaves are made per run."""

    def __init__(self, cuda, case):
        import torch
        self.L, self.V, self.T, self.count = case
        self.p0, self.v0, self.par, self.head, self.t = case_inputs(case)
        self.cuda = cuda
        self.cnt = None if self.count is None else torch.tensor(self.count, device=cuda, dtype=torch.int32)
        self.live = live_mask(self.L, self.V, self.count)
        self.base = (torch.tensor(self.p0, device=cuda), torch.tensor(self.v0, device=cuda),
                     torch.tensor(self.par, device=cuda, dtype=torch.float64), torch.tensor(self.head, device=cuda, dtype=torch.float64))

    def leaves(self, want_params):
        return tuple(t.clone().requires_grad_(want_params or i != 2) for i, t in enumerate(self.base))

    def reverse(self, want_params, g_pT, g_vT, g_samples, probes, every, checkpoint, dense):
        """dense: the yardstick -- dhts.micro_rollout(want_hist=True), the loss written on the cut of hist; else the sampled call.
        -> numpy arrays.  The cotangent is random at probe slots at or beyond count too: they must receive no gradient."""
        import torch
        import dhts
        x = self.leaves(want_params)
        if dense:
            pT, vT, hist = dhts.micro_rollout(*x, self.T, DT, count=self.cnt, want_hist=True)
            samples = hist[every - 1::every]
            if probes is not None:
                samples = samples[..., torch.tensor(probes, device=self.cuda)]
        else:
            pT, vT, samples = dhts.micro_rollout(*x, self.T, DT, count=self.cnt, checkpoint=checkpoint, probes=probes, every=every)
        ((pT * g_pT).sum() + (vT * g_vT).sum() + (samples * g_samples).sum()).backward()
        n = lambda t: None if t is None else t.detach().cpu().numpy()      # noqa: E731
        return dict(pT=n(pT), vT=n(vT), samples=n(samples), g_p0=n(x[0].grad), g_v0=n(x[1].grad), g_params=n(x[2].grad), g_head=n(x[3].grad))


def assert_samples(tag, got, want, live_probes, bitwise):
    """got [..][R][L][2][P] against the yardstick's cut at live probe slots; exactly 0 at the others."""
    assert got.shape == want.shape and got.dtype == np.float32, "%s: shape %s, expected %s" % (tag, got.shape, want.shape)
    m = np.broadcast_to(live_probes[:, None, :], got.shape)
    assert (same_bits if bitwise else np.array_equal)(got[m], want[m]), "%s: a live probe slot differs from the dense history" % tag
    assert np.all(got[~m] == 0), "%s: a probe slot at or beyond count is not 0" % tag


# =================================================================================================================
# 1. checkpointed reverse mode
# =================================================================================================================
@pytest.mark.parametrize("case", SHAPES, ids=SHAPE_IDS)
def test_checkpointed_samples_equal_the_dense_yardstick(cuda, case):
    """every x probes x params.requires_grad x S in {1, 3, the plan's, max_segment}, random cotangents on pT, vT and on samples: pT, vT,
    samples at live probe slots, g_p0, g_v0, g_head and g_params equal what the dense history gives, and probe slots at or beyond count
    are exactly 0.  Sampled steps fall on, before and after segment boundaries, with every a multiple of S and coprime to it.
    Compared as NUMBERS (np.array_equal), not as bit patterns: where the sampled sweep adds nothing, the yardstick adds the float32 +0.0
    that autograd scattered into its dense cotangent, which can turn a -0.0 into +0.0 and does nothing else.
    The yardstick of an (every, probes, params) setting is computed once for all S."""
    import torch
    from dhts import ops
    d = Device(cuda, case)
    L, V, T = d.L, d.V, d.T
    rng = np.random.default_rng(2000 + 31 * V + T)
    g_pT, g_vT = (torch.tensor(a, device=cuda) for a in rng.standard_normal((2, L, V)).astype(np.float32))
    g_dense = rng.standard_normal((T, L, 2, V)).astype(np.float32)
    desc = ops.micro_desc(L, V, DT)
    for want_params in (False, True):
        top = ops.micro_ckpt_plan(desc, T, want_params)["max_segment"]
        assert top >= 3
        for every, probes in settings(T, V):
            g_samples = torch.tensor(np.ascontiguousarray(cut(g_dense, probes, every)), device=cuda)
            assert g_samples.shape[0] == T // every
            want = d.reverse(want_params, g_pT, g_vT, g_samples, probes, every, None, dense=True)
            lp = d.live if probes is None else d.live[:, probes]
            for S in (1, 3, True, top):
                tag = "%s every=%d probes=%s params=%s S=%s" % (IDS[CASES.index(case)], every, "all" if probes is None else probes[:4],
                                                              want_params, S)
                got = d.reverse(want_params, g_pT, g_vT, g_samples, probes, every, S, dense=False)
                assert same_bits(got["pT"], want["pT"]) and same_bits(got["vT"], want["vT"]), tag
                assert_samples(tag, got["samples"], want["samples"], lp, bitwise=False)
                assert (got["g_params"] is not None) == want_params
                for key in GRADS:
                    if got[key] is not None:
                        assert np.array_equal(got[key], want[key]), "%s: %s differs from the dense yardstick" % (tag, key)


# =================================================================================================================
# 2. fused forward mode
# =================================================================================================================
@pytest.mark.parametrize("case", SHAPES, ids=SHAPE_IDS)
def test_fused_samples_are_the_cut_of_the_dense_histories(cuda, case):
    """every x probes x direction sets -- K = 5 (each leaf of LEAVES alone, then all together: the t_params kernel, two launch groups),
    K = 4 with t_params (its first four), K = 4 state-only (t_p0, t_v0, t_head alone and together), K = 1 both ways --: pT, vT, t_pT,
    t_vT, samples at live probe slots and all of t_samples are bit for bit those of micro_rollout_jvp(fused=True, want_hist=True), cut;
    dead probe slots are exactly 0 in both.  The dense call of a direction set is made once."""
    import torch
    import dhts
    d = Device(cuda, case)
    L, V, T = d.L, d.V, d.T
    five, three = directions(d.t, LEAVES), directions(d.t, LEAVES[:3])
    sets = [five, {n: a[:4] for n, a in five.items()}, three, {n: a[4:] for n, a in five.items()}, {n: a[3:] for n, a in three.items()}]
    dt64 = {"t_head": torch.float64, "t_params": torch.float64}
    base = d.base
    n = lambda t: t.cpu().numpy()      # noqa: E731
    for tang in sets:
        K = len(next(iter(tang.values())))
        kw = {name: torch.tensor(np.ascontiguousarray(a), device=cuda, dtype=dt64.get(name, torch.float32)) for name, a in tang.items()}
        (pT, vT, hist), (t_pT, t_vT, t_hist) = dhts.micro_rollout_jvp(*base, T, DT, count=d.cnt, want_hist=True, fused=True, **kw)
        dense = [n(x) for x in (pT, vT, hist, t_pT, t_vT, t_hist)]
        assert dense[5].shape == (K, T, L, 2, V)
        for every, probes in settings(T, V):
            tag = "%s K=%d params=%s every=%d probes=%s" % (IDS[CASES.index(case)], K, "t_params" in tang, every,
                                                            "all" if probes is None else probes[:4])
            prim, tan = dhts.micro_rollout_jvp(*base, T, DT, count=d.cnt, fused=True, probes=probes, every=every, **kw)
            assert len(prim) == 3 and len(tan) == 3 and all(x.grad_fn is None for x in prim + tan)
            for got, want in zip((prim[0], prim[1], tan[0], tan[1]), (dense[0], dense[1], dense[3], dense[4])):
                assert same_bits(n(got), want), tag
            lp = d.live if probes is None else d.live[:, probes]
            assert_samples(tag, n(prim[2]), cut(dense[2], probes, every), lp, bitwise=True)
            t_s = n(tan[2])
            assert t_s.shape == (K, T // every, L, 2, len(lp[0]))
            assert same_bits(t_s, np.ascontiguousarray(cut(dense[5], probes, every))), "%s: t_samples" % tag
            assert np.all(t_s[np.broadcast_to(~lp[:, None, :], t_s.shape)] == 0), "%s: a dead probe slot of t_samples" % tag


# =================================================================================================================
# 3. the taped paths' glue
# =================================================================================================================
@pytest.mark.parametrize("case", [SHAPES[1], SHAPES[2]], ids=[SHAPE_IDS[1], SHAPE_IDS[2]])
def test_taped_paths_cut_the_same_numbers_out_of_a_dense_history(cuda, case):
    """checkpoint=None and fused=False with sampling: the numbers of the tape-free paths (tests 1 and 2), zeros at dead probe slots
    included -- reverse mode compared as numbers, forward mode bit for bit."""
    import torch
    import dhts
    d = Device(cuda, case)
    L, V, T = d.L, d.V, d.T
    rng = np.random.default_rng(7)
    g_pT, g_vT = (torch.tensor(a, device=cuda) for a in rng.standard_normal((2, L, V)).astype(np.float32))
    g_dense = rng.standard_normal((T, L, 2, V)).astype(np.float32)
    five = directions(d.t, LEAVES)
    dt64 = {"t_head": torch.float64, "t_params": torch.float64}
    kw = {name: torch.tensor(a, device=cuda, dtype=dt64.get(name, torch.float32)) for name, a in five.items()}
    base = d.base
    for every, probes in ((1, sorted({0, V // 2, V - 1})), (3, None), (3, sorted({0, V // 2, V - 1}))):
        g_samples = torch.tensor(np.ascontiguousarray(cut(g_dense, probes, every)), device=cuda)
        for want_params in (False, True):
            free = d.reverse(want_params, g_pT, g_vT, g_samples, probes, every, True, dense=False)
            taped = d.reverse(want_params, g_pT, g_vT, g_samples, probes, every, None, dense=False)
            for key in ("pT", "vT", "samples") + GRADS:
                assert (free[key] is None) == (taped[key] is None)
                if free[key] is not None:
                    assert np.array_equal(free[key], taped[key]), "every=%d probes=%s %s" % (every, probes, key)
        outs = [dhts.micro_rollout_jvp(*base, T, DT, count=d.cnt, fused=fused, probes=probes, every=every, **kw) for fused in (True, False)]
        for a, b in zip(outs[0][0] + outs[0][1], outs[1][0] + outs[1][1]):
            assert same_bits(a.cpu().numpy(), b.cpu().numpy()), "every=%d probes=%s" % (every, probes)


# =================================================================================================================
# 4. guard bands and raw indices
# =================================================================================================================
def test_guard_bands_and_raw_probe_indices(cuda):
    """The three raw wrappers at V = 65, T = 7, S = 3, every = 2 with ragged counts and a raw CUDA probe tensor that holds -1 and V: every
    output in the middle of a NaN-prefilled buffer (the sample arrays zeroed inside it, as the wrappers allocate them).  Nothing outside
    the views is written; the columns of -1 and V stay 0 (and take no cotangent); every other column is the dense history's."""
    import torch
    import dhts
    from dhts import ops
    L, V, T, S, every, K = 3, 65, 7, 3, 2, 5
    count = [65, 1, 64]
    raw = [0, -1, 33, V, 64]
    valid = [i for i, s in enumerate(raw) if 0 <= s < V]
    slots = [raw[i] for i in valid]
    R, P = T // every, len(raw)
    rng = np.random.default_rng(11)
    p0, v0, par, head = lanes(rng, L, V)
    live = live_mask(L, V, count)
    desc = ops.micro_desc(L, V, DT)
    cnt = torch.tensor(count, device=cuda, dtype=torch.int32)
    probes = torch.tensor(raw, device=cuda, dtype=torch.int32)
    tp0, tv0 = torch.tensor(p0, device=cuda), torch.tensor(v0, device=cuda)
    tpar, thead = torch.tensor(par, device=cuda, dtype=torch.float64), torch.tensor(head, device=cuda, dtype=torch.float64)
    g_pT, g_vT = (torch.tensor(a, device=cuda) for a in rng.standard_normal((2, L, V)).astype(np.float32))
    g_samples = torch.tensor(rng.standard_normal((R, L, 2, P)).astype(np.float32), device=cuda)
    t_par = torch.tensor(rng.standard_normal((K, 6, L, V)), device=cuda)
    t_p, t_v = (torch.tensor(a, device=cuda) for a in rng.standard_normal((2, K, L, V)).astype(np.float32))

    # the dense yardstick: reverse mode with the cotangent of the valid columns, forward mode cut
    x = [t.clone().requires_grad_(True) for t in (tp0, tv0, tpar, thead)]
    pT, vT, hist = dhts.micro_rollout(*x, T, DT, count=cnt, want_hist=True)
    sel = hist[every - 1::every][..., torch.tensor(slots, device=cuda)]
    lp = live[:, slots]
    ((pT * g_pT).sum() + (vT * g_vT).sum() + (sel * g_samples[..., valid]).sum()).backward()
    (_, _, d_hist), (d_tp, d_tv, d_thist) = dhts.micro_rollout_jvp(tp0, tv0, tpar, thead, T, DT, t_p0=t_p, t_v0=t_v, t_params=t_par, count=cnt,
                                                                   want_hist=True, fused=True)

    def framed(shape, zero=False):
        buf, view = guarded(shape, cuda)
        if zero:
            view.zero_()
        return buf, view

    bufs = dict(ck=framed((ops.micro_ckpt_numel(desc, T, S),)), pT=framed((L, V)), vT=framed((L, V)), samples=framed((R, L, 2, P), True),
                g_p0=framed((L, V)), g_v0=framed((L, V)), jp=framed((L, V)), jv=framed((L, V)), jtp=framed((K, L, V)), jtv=framed((K, L, V)),
                jsamples=framed((R, L, 2, P), True), jt=framed((K, R, L, 2, P), True))
    gq_buf = torch.full((6 * L * V + 64,), float("nan"), dtype=torch.float64, device=cuda)
    g_params = gq_buf[32:32 + 6 * L * V].view(6, L, V)
    g_head = torch.full((L, 2), float("nan"), dtype=torch.float64, device=cuda)
    errs = [ops.new_error_record(cuda) for _ in range(4)]
    out = ops.micro_rollout_fwd_ckpt_samples(desc, T, tp0, tv0, tpar, thead, bufs["ck"][1], probes, every, count=cnt, segment=S,
                                             samples=bufs["samples"][1], err=errs[0], out=(bufs["pT"][1], bufs["vT"][1]))
    assert out[2] is bufs["samples"][1]
    ops.micro_rollout_bwd_ckpt_samples(desc, T, bufs["ck"][1], tpar, thead, g_pT, g_vT, probes, every, g_samples, count=cnt, segment=S,
                                       err=errs[1], out=(bufs["g_p0"][1], bufs["g_v0"][1]), g_head=g_head, g_params=g_params)
    ops.micro_rollout_fwd_jvp_samples(desc, T, tp0, tv0, tpar, thead, t_p, t_v, probes, every, count=cnt, t_params=t_par, err=errs[2],
                                      err_jvp=errs[3], out=tuple(bufs[k][1] for k in ("jp", "jv", "jtp", "jtv", "jsamples", "jt")))
    torch.cuda.synchronize()
    assert all(e.tolist()[0] == 0 for e in errs)
    host = {}
    for name, (buf, view) in bufs.items():
        b = buf.cpu().numpy()
        assert np.all(np.isnan(b[:256])) and np.all(np.isnan(b[b.size - 256:])), "a guard band was written (%s)" % name
        host[name] = b[256:b.size - 256].reshape(view.shape)
        if name != "ck":
            assert np.all(np.isfinite(host[name])), "an element was not written (%s)" % name
    q = gq_buf.cpu().numpy()
    assert np.all(np.isnan(q[:32])) and np.all(np.isnan(q[-32:])) and np.all(np.isfinite(q[32:-32])) and bool(torch.all(torch.isfinite(g_head)))
    n = lambda t: t.detach().cpu().numpy()      # noqa: E731
    for name in ("samples", "jsamples"):
        assert np.all(host[name][..., [1, 3]] == 0), "the column of a probe outside [0, V) was written (%s)" % name
        assert_samples(name, np.ascontiguousarray(host[name][..., valid]), cut(n(hist) if name == "samples" else n(d_hist), slots, every), lp,
                       bitwise=True)
    assert np.all(host["jt"][..., [1, 3]] == 0)
    assert same_bits(np.ascontiguousarray(host["jt"][..., valid]), np.ascontiguousarray(cut(n(d_thist), slots, every)))
    assert same_bits(host["pT"], n(pT)) and same_bits(host["vT"], n(vT)) and same_bits(host["jp"], n(pT)) and same_bits(host["jv"], n(vT))
    assert same_bits(host["jtp"], n(d_tp)) and same_bits(host["jtv"], n(d_tv))
    for got, want in ((host["g_p0"], x[0].grad), (host["g_v0"], x[1].grad), (n(g_params), x[2].grad), (n(g_head), x[3].grad)):
        assert np.array_equal(got, n(want))


# =================================================================================================================
# 5. memory
# =================================================================================================================
def test_checkpointed_samples_allocate_no_history(cuda):
    """64 lanes of 256 vehicles, 400 steps, checkpoint=4, four probes every 10 steps, params requiring grad: the peak of forward +
    backward above the resident inputs stays below half the bytes of the dense history (T L 2 V 4 = 52 MB; the checkpoint buffer is a
    quarter of it by construction, everything else is small).  The same call with want_hist=True exceeds the history's size: the test
    measures something."""
    import torch
    import dhts
    L, V, T = 64, 256, 400
    rng = np.random.default_rng(43)
    p0, v0, par, head = lanes(rng, L, V)
    dense = T * L * 2 * V * 4
    peaks = []
    for sampled in (True, False):
        x = (torch.tensor(p0, device=cuda, requires_grad=True), torch.tensor(v0, device=cuda, requires_grad=True),
             torch.tensor(par, device=cuda, dtype=torch.float64, requires_grad=True),
             torch.tensor(head, device=cuda, dtype=torch.float64, requires_grad=True))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        resident = torch.cuda.memory_allocated()
        kw = dict(probes=[10, 90, 170, 250], every=10) if sampled else dict(want_hist=True)
        out = dhts.micro_rollout(*x, T, DT, check_faults=False, checkpoint=4, **kw)
        if sampled:
            assert tuple(out[2].shape) == (T // 10, L, 2, 4)
        (1e-4 * (out[0] ** 2).sum() + (out[1] ** 2).sum() + (out[2] ** 2).sum()).backward()
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - resident)
        assert all(bool(torch.all(torch.isfinite(t.grad))) for t in x)
        del out, x
    print("forward + backward, peak above the resident inputs: sampled %d bytes, want_hist %d bytes; the dense history %d bytes"
          % (peaks[0], peaks[1], dense))
    assert peaks[0] < dense // 2
    assert peaks[1] > dense


# =================================================================================================================
# 6. the fault records
# =================================================================================================================
def test_collision_record_of_the_sampled_forwards(cuda, capsys):
    """test_micro_ckpt_gpu's construction -- a lane with two vehicles 1 m apart, the follower at 30 m/s --: the sampled checkpointed
    forward and the sampled fused kernel report the un-sampled checkpointed forward's DHTS_FAULT_COLLISION (step 0, lane 1, vehicle 0),
    and the operator prints it and goes on."""
    import torch
    import dhts
    from dhts import _lib, ops
    L, V, T, S = 4, 70, 5, 2
    rng = np.random.default_rng(2)
    p0, v0, par, head = lanes(rng, L, V)
    count = [70, 2, 70, 70]
    p0[1, :2], v0[1, :2] = (0.0, 1.0), (30.0, 10.0)
    desc = ops.micro_desc(L, V, DT)
    tp0, tv0 = torch.tensor(p0, device=cuda), torch.tensor(v0, device=cuda)
    tpar, thead = torch.tensor(par, device=cuda, dtype=torch.float64), torch.tensor(head, device=cuda, dtype=torch.float64)
    cnt = torch.tensor(count, device=cuda, dtype=torch.int32)
    probes = torch.tensor([0, 1, 69], device=cuda, dtype=torch.int32)
    errs = [ops.new_error_record(cuda) for _ in range(3)]
    ckpt = torch.empty(ops.micro_ckpt_numel(desc, T, S), dtype=torch.float32, device=cuda)
    ops.micro_rollout_fwd_ckpt(desc, T, tp0, tv0, tpar, thead, ckpt, count=cnt, segment=S, err=errs[0])
    ops.micro_rollout_fwd_ckpt_samples(desc, T, tp0, tv0, tpar, thead, ckpt, probes, 2, count=cnt, segment=S, err=errs[1])
    ops.micro_rollout_fwd_jvp_samples(desc, T, tp0, tv0, tpar, thead, tp0[None], tv0[None], probes, 2, count=cnt, err=errs[2])
    assert [e.tolist() for e in errs] == [[_lib.FAULT_COLLISION, 0, 1, 0]] * 3
    capsys.readouterr()
    out = dhts.micro_rollout(tp0, tv0, tpar, thead, T, DT, count=cnt, checkpoint=S, probes=[0, 1, 69], every=2)      # prints, does not raise
    assert "Collision detected between vehicles (step 0, lane 1, vehicle 0)" in capsys.readouterr().out
    assert tuple(out[2].shape) == (2, L, 2, 3)


def test_non_finite_cotangent_record_of_the_sampled_reverse_sweep(cuda):
    """test_micro_ckpt_gpu's construction: a NaN in the cotangent at step 9 of 20 with S = 4 (the third segment the sweep takes, on no
    boundary of one), here in the row of g_samples that every = 5 gives step 9 (row 1), at probe column 2 = vehicle 7 of lane 1.
    ops.micro_bwd_fault() gives (9, 1, 7) as the un-sampled checkpointed call with the dense g_hist does, state-only and with the
    parameter gradient, and the gradients are NaN in the same places."""
    import warnings
    import torch
    import dhts
    from dhts import ops
    L, V, T, S, every = 3, 70, 20, 4, 5
    step, lane, veh = 9, 1, 7
    probes = [0, 3, 7, 40]
    rng = np.random.default_rng(77)
    p0, v0, par, head = lanes(rng, L, V)
    count = [70, 41, 5]
    g_pT, g_vT = rng.standard_normal((2, L, V)).astype(np.float32)
    g_samples = rng.standard_normal((T // every, L, 2, len(probes))).astype(np.float32)
    assert (step + 1) % every == 0
    g_samples[(step + 1) // every - 1, lane, 1, probes.index(veh)] = np.nan
    g_hist = np.zeros((T, L, 2, V), np.float32)
    g_hist[every - 1::every][..., probes] = g_samples
    assert np.isnan(g_hist[step, lane, 1, veh]) and np.isnan(g_hist).sum() == 1
    for want_params in (False, True):
        out = []
        for sampled in (False, True):
            x = (torch.tensor(p0, device=cuda, requires_grad=True), torch.tensor(v0, device=cuda, requires_grad=True),
                 torch.tensor(par, device=cuda, dtype=torch.float64, requires_grad=want_params),
                 torch.tensor(head, device=cuda, dtype=torch.float64, requires_grad=True))
            kw = dict(probes=probes, every=every) if sampled else dict(want_hist=True)
            res = dhts.micro_rollout(*x, T, DT, count=torch.tensor(count, device=cuda, dtype=torch.int32), checkpoint=S, **kw)
            torch.autograd.backward(list(res), [torch.tensor(g_pT, device=cuda), torch.tensor(g_vT, device=cuda),
                                                torch.tensor(g_samples if sampled else g_hist, device=cuda)])
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                where = ops.micro_bwd_fault()
            assert any(issubclass(i.category, RuntimeWarning) for i in w)
            out.append((where, [t.grad.cpu().numpy() for t in x if t.grad is not None]))
        assert out[0][0] == (step, lane, veh) == out[1][0]
        assert len(out[0][1]) == len(out[1][1]) == (4 if want_params else 3)
        for a, b in zip(out[0][1], out[1][1]):
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])
        assert np.isnan(out[1][1][1][lane, veh]) and np.all(np.isfinite(out[1][1][1][0]))


# =================================================================================================================
# 7. the example
# =================================================================================================================
def test_calibration_example_observes_probes_the_same_checkpointed(cuda, tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    logs = []
    for extra in ([], ["--checkpoint", "4"]):
        cwd = tmp_path / ("checkpointed" if extra else "taped")
        cwd.mkdir()
        out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "calibrate_idm.py"), "--seed", "1", "--n_lane", "8",
                              "--n_vehicle", "16", "--n_step", "50", "--n_episode", "5", "--observe", "4,5"] + extra, cwd=str(cwd), env=env,
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        files = [os.path.join(dp, f) for dp, _, fs in os.walk(str(cwd)) for f in fs if f.startswith("trial_") and f.endswith(".txt")]
        assert len(files) == 1, "one trial_k.txt per run"
        logs.append(open(files[0]).read())
    assert len(logs[0].splitlines()) == 5
    assert logs[0] == logs[1], "the checkpointed run's loss lines differ:\n%s\nagainst\n%s" % (logs[1], logs[0])
