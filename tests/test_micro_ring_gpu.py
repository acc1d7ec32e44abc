"""A ring road on the two tape-free paths of the micro rollout, on the device: dhts.micro_rollout(ring=) with checkpoint= (and
target=) and dhts.micro_rollout_jvp(ring=, fused=True).  The yardsticks, in the order of trust:
  1. forward -- the existing lead= forms fed the ring run's own tail trajectory one circumference ahead: the same bits;
  2. reverse -- T chained one-step lead= calls under autograd, the single lead row built from the previous call's tail by torch ops, so
     that autograd hands g_lead back to the tail; the head's share of the tail's length gradient, which lead_length cannot carry, and
     the whole g_params once more against tests/micro_ring_ref.py::ring_rollout (validated on the CPU in tests/test_micro_ring.py);
  3. the target form against the sampled form with the squared error formed in torch;
  4. forward mode against chained one-step fused lead= calls, and a dot-product check between the new reverse and forward forms;
  5. a full lane of 1024 against ring_rollout.
Then the collision record of a ring too short, guard bands and empty rollouts, and the calibration example.
Needs a real MI355X: python -m pytest tests -m gpu"""
import os
import subprocess
import sys

import numpy as np
import pytest

from micro_lead_ref import trajectory_before_steps
from micro_ring_ref import restated_ring, tail_image
from test_micro_ckpt_gpu import live_mask, same_bits
from test_micro_jvp_gpu import DT, guarded
from test_micro_lead_gpu import cut, n, samplings, t32, t64
from test_micro_params import per_plane
from test_micro_params_gpu import lanes
from test_micro_target_gpu import assert_sse, make_target
from util import TOL_GRAD, TOL_STATE, grad_report, rel_elem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 5
WIDTHS = (1, 2, 5, 64, 65, 130)          # 64: tail and head in one wavefront; 65: in different ones
STEPS = (0, 1, 7, 37)                    # against segments 1, 3, the plan's and the longest: a multiple and not
SHAPES = [(V, T) for V in WIDTHS for T in STEPS]
SHAPE_IDS = ["V%d_T%d" % s for s in SHAPES]


def counts(V):
    """Per-lane count in {V, 0, 1, 2, V // 2}, one lane each."""
    return [min(c, V) for c in (V, 0, 1, 2, V // 2)]


def ring_inputs(V, T, count=None, lanes_=L):
    """Collision-free lanes with vehicle lengths of their own, and a circumference per lane that leaves the head 25 to 35 m of road
    to the image of the tail."""
    rng = np.random.default_rng(31 * V + T)
    p0, v0, par, _ = lanes(rng, lanes_, V)
    par[5] = rng.uniform(4.0, 6.0, par[5].shape)
    cnt = [V] * lanes_ if count is None else count
    ring = np.array([(p0[l, c - 1] - p0[l, 0] if c > 0 else 0.0) + rng.uniform(25.0, 35.0) for l, c in enumerate(cnt)])
    return rng, p0, v0, par, ring, cnt


def checkpoints(desc, T, want_params, target=False):
    from dhts import ops
    plan = ops.micro_ckpt_target_plan if target else ops.micro_ckpt_plan
    return (1, 3, True, plan(desc, T, want_params)["max_segment"])


def dense_ring_run(cuda, p0, v0, par, ring, cnt, T):
    """The ring form observed at every slot and step, no grad -> (pT, vT, samples [T][L][2][V]) as numpy."""
    import torch
    import dhts
    V = p0.shape[1]
    with torch.no_grad():
        out = dhts.micro_rollout(t32(p0, cuda), t32(v0, cuda), t64(par, cuda), None, T, DT, count=torch.tensor(cnt, device=cuda, dtype=torch.int32),
                                 checkpoint=True, ring=t64(ring, cuda), probes=list(range(V)), every=1)
    return tuple(n(x) for x in out)


def lead_of_tail(p0, v0, hist, ring):
    """[T][L][2] float32: what the head sees in step t -- the tail's state before the step, one circumference ahead."""
    return np.stack([tail_image(trajectory_before_steps(p0[:, 0], hist[:, :, 0, 0]), ring[None, :]),
                     trajectory_before_steps(v0[:, 0], hist[:, :, 1, 0])], -1).astype(np.float32)


# =================================================================================================================
# 1. forward against existing device code
# =================================================================================================================
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_forward_is_the_lead_form_fed_the_rings_own_tail(cuda, shape):
    """pT, vT and the samples of the checkpointed and of the fused kernel: the bits of the existing lead= call whose lead[t] is the
    ring run's tail before step t, (p.double() + ring).float(), and whose lead_length is the tail's length.  Slots at or beyond count
    read exactly 0 in the samples and pass through in the state.  checkpoint in {1, 3, True, max_segment} x five sampling settings."""
    import torch
    import dhts
    from dhts import ops
    V, T = shape
    rng, p0, v0, par, ring, cnt = ring_inputs(V, T, counts(V))
    live = live_mask(L, V, cnt)
    desc = ops.micro_desc(L, V, DT)
    t_cnt = torch.tensor(cnt, device=cuda, dtype=torch.int32)
    pT, vT, hist = dense_ring_run(cuda, p0, v0, par, ring, cnt, T)
    assert hist.shape == (T, L, 2, V)
    assert same_bits(pT[~live], p0[~live]) and same_bits(vT[~live], v0[~live]), "slots at or beyond count pass through"
    assert np.all(hist[np.broadcast_to(~live[None, :, None, :], hist.shape)] == 0)
    if T > 0:
        assert not np.array_equal(pT[live], p0[live])
    lead, lead_len = t32(lead_of_tail(p0, v0, hist, ring), cuda), t64(par[5, :, 0], cuda)
    t_ring = t64(ring, cuda)
    t_p0 = t32(rng.standard_normal((1, L, V)), cuda)
    runs = 0
    for sampling in samplings(T, V):
        kw = {} if sampling is None else dict(every=sampling[0], probes=sampling[1])
        want_rows = None if sampling is None else cut(hist, sampling)
        for ck in checkpoints(desc, T, False):
            for grad in (False, True):            # with a leaf that requires grad the forward keeps its checkpoints
                a = dhts.micro_rollout(t32(p0, cuda, grad), t32(v0, cuda), t64(par, cuda), None, T, DT, count=t_cnt, checkpoint=ck, ring=t_ring, **kw)
                b = dhts.micro_rollout(t32(p0, cuda, grad), t32(v0, cuda), t64(par, cuda), None, T, DT, count=t_cnt, checkpoint=ck, lead=lead,
                                       lead_length=lead_len, **kw)
                tag = "sampling %s, checkpoint %s" % (sampling and sampling[0], ck)
                assert len(a) == len(b) == (2 if sampling is None else 3), tag
                assert all(same_bits(n(x), n(y)) for x, y in zip(a, b)), tag
                assert same_bits(n(a[0]), pT) and same_bits(n(a[1]), vT), tag
                if sampling is not None:
                    assert same_bits(n(a[2]), np.ascontiguousarray(want_rows)), tag
                runs += 1
        prim, tang = dhts.micro_rollout_jvp(t32(p0, cuda), t32(v0, cuda), t64(par, cuda), None, T, DT, t_p0=t_p0, count=t_cnt, fused=True,
                                            ring=t_ring, **kw)
        prim_l, _ = dhts.micro_rollout_jvp(t32(p0, cuda), t32(v0, cuda), t64(par, cuda), None, T, DT, t_p0=t_p0, count=t_cnt, fused=True,
                                           lead=lead, lead_length=lead_len, **kw)
        assert len(prim) == len(tang) == (2 if sampling is None else 3)
        assert all(same_bits(n(x), n(y)) for x, y in zip(prim, prim_l)), "the fused kernel, sampling %s" % (sampling and sampling[0],)
        assert same_bits(n(prim[0]), pT) and same_bits(n(prim[1]), vT)
    assert runs == 5 * 4 * 2


# =================================================================================================================
# 2. reverse against chained one-step calls
# =================================================================================================================
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_reverse_against_chained_one_step_lead_calls(cuda, shape):
    """T calls of dhts.micro_rollout(T=1, checkpoint=1, lead=row, lead_length=the tail's length) under autograd, row = the previous
    call's tail one circumference ahead, formed by torch ops: autograd returns g_lead to the tail.  States: the same bits.  g_p0, g_v0,
    g_params planes 0 .. 4 and the length plane of every slot but 0: TOL_GRAD (printed: whether they are bit-equal).  The length plane
    of slot 0 -- the head's share -- and all of g_params once more: ring_rollout's autograd, TOL_GRAD."""
    import torch
    import dhts
    from dhts import ops
    V, T = shape
    rng, p0, v0, par, ring, cnt = ring_inputs(V, T, counts(V))
    live = live_mask(L, V, cnt)
    desc = ops.micro_desc(L, V, DT)
    t_cnt = torch.tensor(cnt, device=cuda, dtype=torch.int32)
    t_ring = t64(ring, cuda)
    every, probes = (3, sorted({0, V // 3, V // 2, V - 1})) if T >= 3 else (1, list(range(V)))
    R = T // every
    g_pT, g_vT = rng.standard_normal((2, L, V)).astype(np.float32)
    g_s = rng.standard_normal((R, L, 2, len(probes))).astype(np.float32)
    g_hist = np.zeros((T, L, 2, V), np.float32)
    if R:
        g_hist[every - 1::every][..., probes] = g_s              # (a view of g_hist: written in place)
    g_hist *= live[None, :, None, :]
    # ---- the chain ----
    c_p0, c_v0, c_par = t32(p0, cuda, True), t32(v0, cuda, True), t64(par, cuda, True)
    lead_len = t64(par[5, :, 0], cuda)
    zero, lp = torch.zeros((), device=cuda), torch.tensor(live[:, probes], device=cuda)
    p, v, rows = c_p0, c_v0, []
    for t in range(T):
        row = torch.stack([(p[:, 0].double() + t_ring).float(), v[:, 0]], -1)[None]
        p, v = dhts.micro_rollout(p, v, c_par, None, 1, DT, count=t_cnt, checkpoint=1, lead=row, lead_length=lead_len)
        if (t + 1) % every == 0:
            rows.append(torch.where(lp[:, None, :], torch.stack([p[:, probes], v[:, probes]], 1), zero))
    loss = (p * t32(g_pT, cuda)).sum() + (v * t32(g_vT, cuda)).sum()
    if rows:
        loss = loss + (torch.stack(rows) * t32(g_s, cuda)).sum()
    loss.backward()                                              # (T = 0: the cotangents pass through)
    c_samples = n(torch.stack(rows)) if rows else np.zeros((0, L, 2, len(probes)), np.float32)
    zeros = lambda t: n(t.grad) if t.grad is not None else np.zeros(tuple(t.shape), np.float32 if t.dtype == torch.float32 else np.float64)  # noqa: E731
    c_gp, c_gv, c_gq = zeros(c_p0) * live, zeros(c_v0) * live, zeros(c_par) * live[None]
    ref = restated_ring(p0, v0, par, ring, T, DT, count=cnt, g_pT=g_pT * live, g_vT=g_vT * live, g_hist=g_hist)
    not_tail = np.ones((6, L, V), bool)
    not_tail[5, :, 0] = False
    for want_params in (False, True):
        for ck in checkpoints(desc, T, want_params):
            y = (t32(p0, cuda, True), t32(v0, cuda, True), t64(par, cuda, want_params))
            pT, vT, samples = dhts.micro_rollout(*y, None, T, DT, count=t_cnt, checkpoint=ck, ring=t_ring, every=every, probes=probes)
            ((pT * t32(g_pT * live, cuda)).sum() + (vT * t32(g_vT * live, cuda)).sum() + (samples * t32(g_s, cuda)).sum()).backward()
            tag = "V %d T %d checkpoint %s params %s" % (V, T, ck, want_params)
            assert same_bits(n(pT), n(p)) and same_bits(n(vT), n(v)) and same_bits(n(samples), c_samples), tag
            gp, gv = n(y[0].grad), n(y[1].grad)
            assert np.all(gp[~live] == 0) and np.all(gv[~live] == 0), tag
            equal = [np.array_equal(gp, c_gp), np.array_equal(gv, c_gv)]
            if T > 0:
                assert grad_report(tag + ": g_p0 vs the chain", gp, c_gp) <= TOL_GRAD
                assert grad_report(tag + ": g_v0 vs the chain", gv, c_gv) <= TOL_GRAD
                assert grad_report(tag + ": g_p0 vs ring_rollout", gp, ref["g_p0"]) <= TOL_GRAD
                assert grad_report(tag + ": g_v0 vs ring_rollout", gv, ref["g_v0"]) <= TOL_GRAD
            else:
                assert equal == [True, True], tag
            if want_params:
                gq = n(y[2].grad)
                assert np.all(gq[~np.broadcast_to(live, (6, L, V))] == 0), tag
                equal.append(np.array_equal(gq[not_tail], c_gq[not_tail]))
                if T > 0:
                    assert per_plane(tag + ": g_params but the tail's length vs the chain", gq * not_tail, c_gq * not_tail) <= TOL_GRAD
                    assert per_plane(tag + ": g_params vs ring_rollout", gq, ref["g_params"]) <= TOL_GRAD
                    assert grad_report(tag + ": the tail's length vs ring_rollout", gq[5, :, 0], ref["g_params"][5, :, 0]) <= TOL_GRAD
                else:
                    assert np.all(gq == 0), tag
            print("%s: bit-equal to the chain: g_p0 %s, g_v0 %s%s" % (tag, equal[0], equal[1], ", g_params %s" % equal[2] if want_params else ""))
    if T >= 7 and V >= 2:
        # the head's share is there to be seen: the chain, which cannot carry it, differs in the tail's length
        full = [l for l, c in enumerate(cnt) if c >= 2]
        assert np.any(ref["g_params"][5, full, 0] != c_gq[5, full, 0])
        assert np.any(c_gp[:, 0] != 0)


# =================================================================================================================
# 3. the target form
# =================================================================================================================
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_target_on_a_ring_equals_the_sampled_form_with_the_loss_in_torch(cuda, shape):
    """ring= + target= against ring= + probes=range(V), every=1 with the squared error formed in torch, under the NaN-masked targets of
    tests/test_micro_target_gpu.py: pT, vT the same bits, sse as that file compares it, gradients at TOL_GRAD."""
    import torch
    import dhts
    from dhts import ops
    V, T = shape
    rng, p0, v0, par, ring, cnt = ring_inputs(V, T, counts(V))
    live = live_mask(L, V, cnt)
    desc = ops.micro_desc(L, V, DT)
    t_cnt, t_ring = torch.tensor(cnt, device=cuda, dtype=torch.int32), t64(ring, cuda)
    hist = dense_ring_run(cuda, p0, v0, par, ring, cnt, T)[2]
    g_pT, g_vT = (rng.standard_normal((2, L, V)) * live).astype(np.float32)
    w = rng.uniform(0.5, 2.0, (L, 2))
    for pattern in ("entries", "steps", "all_nan"):
        target = make_target(rng, hist, live, pattern)
        t_target = t32(target, cuda)
        x = (t32(p0, cuda, True), t32(v0, cuda, True), t64(par, cuda, True))
        d_pT, d_vT, d_s = dhts.micro_rollout(*x, None, T, DT, count=t_cnt, checkpoint=True, ring=t_ring, probes=list(range(V)), every=1)
        seen = ~torch.isnan(t_target) & torch.tensor(live, device=cuda)[None, :, None, :]
        r = torch.where(seen, d_s - torch.where(seen, t_target, torch.zeros((), device=cuda)), torch.zeros((), device=cuda))
        loss = ((r.double() ** 2).sum(dim=(0, 3)) * t64(w, cuda)).sum() + (d_pT * t32(g_pT, cuda)).sum() + (d_vT * t32(g_vT, cuda)).sum()
        loss.backward()
        for want_params in (False, True):
            for ck in checkpoints(desc, T, want_params, target=True):
                y = (t32(p0, cuda, True), t32(v0, cuda, True), t64(par, cuda, want_params))
                pT, vT, sse = dhts.micro_rollout(*y, None, T, DT, count=t_cnt, checkpoint=ck, ring=t_ring, target=t_target)
                ((sse * t64(w, cuda)).sum() + (pT * t32(g_pT, cuda)).sum() + (vT * t32(g_vT, cuda)).sum()).backward()
                tag = "V %d T %d %s checkpoint %s params %s" % (V, T, pattern, ck, want_params)
                assert same_bits(n(pT), n(d_pT)) and same_bits(n(vT), n(d_vT)), tag
                assert_sse(tag, n(sse), hist, target, live)
                if T > 0:
                    assert grad_report(tag + ": g_p0", n(y[0].grad), n(x[0].grad)) <= TOL_GRAD
                    assert grad_report(tag + ": g_v0", n(y[1].grad), n(x[1].grad)) <= TOL_GRAD
                    if want_params:
                        assert per_plane(tag, n(y[2].grad), n(x[2].grad)) <= TOL_GRAD
                else:
                    assert np.array_equal(n(y[0].grad), g_pT) and np.array_equal(n(y[1].grad), g_vT) and np.all(n(sse) == 0), tag


# =================================================================================================================
# 4. fused forward mode
# =================================================================================================================
def ring_directions(rng, K, V):
    t_p0, t_v0 = rng.standard_normal((2, K, L, V)).astype(np.float32)
    t_par = rng.standard_normal((K, 6, L, V))
    return t_p0, t_v0, t_par


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_tangents_against_chained_one_step_fused_lead_calls(cuda, shape):
    """K in {1, 4, 5}, with and without t_params: T calls of dhts.micro_rollout_jvp(T=1, fused=True, lead=row, t_lead=the tail's
    tangents) against one ring call.  The tail's length tangent is zero here (a recorded leader's length is a constant: the chain cannot
    carry it; the dot-product test below does), so every step is the same arithmetic: the same bits, primal, tangents and samples."""
    import torch
    import dhts
    V, T = shape
    rng, p0, v0, par, ring, cnt = ring_inputs(V, T, counts(V))
    live = live_mask(L, V, cnt)
    t_cnt, t_ring = torch.tensor(cnt, device=cuda, dtype=torch.int32), t64(ring, cuda)
    lead_len = t64(par[5, :, 0], cuda)
    every, probes = (3, sorted({0, V // 3, V // 2, V - 1})) if T >= 3 else (1, list(range(V)))
    base = (t32(p0, cuda), t32(v0, cuda), t64(par, cuda))
    for K in (1, 4, 5):
        t_p0, t_v0, t_par = ring_directions(rng, K, V)
        t_par[:, 5, :, 0] = 0.0
        for with_params in (False, True):
            tq = dict(t_params=t64(t_par, cuda)) if with_params else {}
            p, v, tp, tv = base[0], base[1], t32(t_p0, cuda), t32(t_v0, cuda)
            rows, t_rows = [], []
            for t in range(T):
                row = torch.stack([(p[:, 0].double() + t_ring).float(), v[:, 0]], -1)[None]
                t_row = torch.stack([tp[:, :, 0], tv[:, :, 0]], -1)[:, None]                     # [K][1][L][2]
                (p, v), (tp, tv) = dhts.micro_rollout_jvp(p, v, base[2], None, 1, DT, t_p0=tp, t_v0=tv, count=t_cnt, fused=True, lead=row,
                                                          lead_length=lead_len, t_lead=t_row.contiguous(), **tq)
                if (t + 1) % every == 0:
                    rows.append(torch.stack([p[:, probes], v[:, probes]], 1))
                    t_rows.append(torch.stack([tp[:, :, probes], tv[:, :, probes]], 2))
            prim, tang = dhts.micro_rollout_jvp(*base, None, T, DT, t_p0=t32(t_p0, cuda), t_v0=t32(t_v0, cuda), count=t_cnt, fused=True,
                                                ring=t_ring, every=every, probes=probes, **tq)
            tag = "V %d T %d K %d t_params %s" % (V, T, K, with_params)
            lk = np.broadcast_to(live, (K, L, V))
            assert same_bits(n(prim[0]), n(p)) and same_bits(n(prim[1]), n(v)), tag
            if T > 0:
                assert same_bits(n(tang[0])[lk], n(tp)[lk]) and same_bits(n(tang[1])[lk], n(tv)[lk]), tag
            else:
                zero = np.float32(0)             # (+0: a product with False would leave -0 under a negative tangent)
                assert same_bits(n(tang[0]), np.where(live[None], t_p0, zero)) and same_bits(n(tang[1]), np.where(live[None], t_v0, zero)), tag
            assert np.all(n(tang[0])[~lk] == 0) and np.all(n(tang[1])[~lk] == 0), tag
            if rows:
                m = np.broadcast_to(live[:, probes][:, None, :], prim[2].shape)
                mk = np.broadcast_to(m, tang[2].shape)
                assert same_bits(n(prim[2])[m], n(torch.stack(rows))[m]) and np.all(n(prim[2])[~m] == 0), tag
                assert same_bits(n(tang[2])[mk], n(torch.stack(t_rows, 1))[mk]) and np.all(n(tang[2])[~mk] == 0), tag
            else:
                assert prim[2].shape[0] == 0 and tang[2].shape[1] == 0, tag


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] > 0], ids=[i for s, i in zip(SHAPES, SHAPE_IDS) if s[1] > 0])
def test_new_reverse_and_forward_forms_are_adjoint(cuda, shape):
    """<g, J t> against <J^T g, t> on a ring: J t from dhts.micro_rollout_jvp(ring=, fused=True) with random t_p0, t_v0, t_params (the
    tail's length included), J^T g from the backward of dhts.micro_rollout(ring=, checkpoint=True) under random cotangents of pT, vT and
    the samples.  Both inner products summed in double; they agree within TOL_GRAD of the sum of the absolute terms."""
    import torch
    import dhts
    V, T = shape
    rng, p0, v0, par, ring, cnt = ring_inputs(V, T, counts(V))
    live = live_mask(L, V, cnt)
    t_cnt, t_ring = torch.tensor(cnt, device=cuda, dtype=torch.int32), t64(ring, cuda)
    every, probes = (3, sorted({0, V // 3, V // 2, V - 1})) if T >= 3 else (1, list(range(V)))
    K = 5
    t_p0, t_v0, t_par = ring_directions(rng, K, V)
    t_par[:, :5] *= 0.1
    _, (j_p, j_v, j_s) = dhts.micro_rollout_jvp(t32(p0, cuda), t32(v0, cuda), t64(par, cuda), None, T, DT, t_p0=t32(t_p0, cuda),
                                                t_v0=t32(t_v0, cuda), t_params=t64(t_par, cuda), count=t_cnt, fused=True, ring=t_ring,
                                                every=every, probes=probes)
    g_pT, g_vT = (rng.standard_normal((2, L, V)) * live).astype(np.float32)
    g_s = rng.standard_normal(tuple(j_s.shape[1:])).astype(np.float32)
    y = (t32(p0, cuda, True), t32(v0, cuda, True), t64(par, cuda, True))
    pT, vT, samples = dhts.micro_rollout(*y, None, T, DT, count=t_cnt, checkpoint=True, ring=t_ring, every=every, probes=probes)
    ((pT * t32(g_pT, cuda)).sum() + (vT * t32(g_vT, cuda)).sum() + (samples * t32(g_s, cuda)).sum()).backward()
    d = lambda a: np.asarray(a, np.float64)      # noqa: E731
    for k in range(K):
        fwd_terms = np.concatenate([(d(g_pT) * d(n(j_p)[k])).ravel(), (d(g_vT) * d(n(j_v)[k])).ravel(), (d(g_s) * d(n(j_s)[k])).ravel()])
        rev_terms = np.concatenate([(d(n(y[0].grad)) * d(t_p0[k])).ravel(), (d(n(y[1].grad)) * d(t_v0[k])).ravel(),
                                    (d(n(y[2].grad)) * d(t_par[k])).ravel()])
        a, b, scale = fwd_terms.sum(), rev_terms.sum(), np.abs(fwd_terms).sum()
        print("V %d T %d direction %d: <g, J t> %.9e  <J^T g, t> %.9e  |difference| / sum |terms| %.2e" % (V, T, k, a, b, abs(a - b) / scale))
        assert abs(a - b) <= TOL_GRAD * scale
    if V >= 2 and T >= 7:
        assert np.any(n(y[2].grad)[5, :, 0] != 0)


# =================================================================================================================
# 5. a full lane
# =================================================================================================================
def test_a_full_lane_of_1024_against_the_yardstick(cuda):
    """count = capacity = 1024, one lane: thread 1023 is the head and slot 1024 of the hand-over arrays the image of the tail.  Against
    ring_rollout: states at TOL_STATE, gradients at TOL_GRAD (g_params plane by plane); the fused kernel's primal is the same bits."""
    import dhts
    V, T = 1024, 20
    rng, p0, v0, par, ring, cnt = ring_inputs(V, T, lanes_=1)
    g_pT, g_vT = rng.standard_normal((2, 1, V)).astype(np.float32)
    g_hist = (0.1 * rng.standard_normal((T, 1, 2, V))).astype(np.float32)
    ref = restated_ring(p0, v0, par, ring, T, DT, g_pT=g_pT, g_vT=g_vT, g_hist=g_hist)
    y = (t32(p0, cuda, True), t32(v0, cuda, True), t64(par, cuda, True))
    pT, vT, samples = dhts.micro_rollout(*y, None, T, DT, checkpoint=True, ring=t64(ring, cuda), every=1, probes=list(range(V)))
    ((pT * t32(g_pT, cuda)).sum() + (vT * t32(g_vT, cuda)).sum() + (samples * t32(g_hist, cuda)).sum()).backward()
    e_s = max(rel_elem(n(pT), ref["pT"]), rel_elem(n(vT), ref["vT"]), rel_elem(n(samples), ref["hist"]))
    print("full ring of 1024: states vs ring_rollout %.2e" % e_s)
    assert e_s <= TOL_STATE
    assert grad_report("full ring d loss / d p0", n(y[0].grad), ref["g_p0"]) <= TOL_GRAD
    assert grad_report("full ring d loss / d v0", n(y[1].grad), ref["g_v0"]) <= TOL_GRAD
    assert per_plane("full ring", n(y[2].grad), ref["g_params"]) <= TOL_GRAD
    # the head sees the tail: on a longer ring it drives another trajectory
    other = dhts.micro_rollout(t32(p0, cuda), t32(v0, cuda), t64(par, cuda), None, T, DT, checkpoint=True, ring=t64(ring + 10.0, cuda))
    assert n(other[1])[0, V - 1] != n(vT)[0, V - 1] and same_bits(n(other[1])[0, :V - T - 1], n(vT)[0, :V - T - 1])
    t_p0 = rng.standard_normal((1, 1, V)).astype(np.float32)
    prim, tang = dhts.micro_rollout_jvp(t32(p0, cuda), t32(v0, cuda), t64(par, cuda), None, T, DT, t_p0=t32(t_p0, cuda), fused=True,
                                        ring=t64(ring, cuda))
    assert same_bits(n(prim[0]), n(pT)) and same_bits(n(prim[1]), n(vT))
    assert np.all(np.isfinite(n(tang[0]))) and np.all(np.isfinite(n(tang[1])))


# =================================================================================================================
# 6. the record
# =================================================================================================================
def test_collision_record_of_a_ring_shorter_than_its_platoon(cuda, capsys):
    """Lane 1's ring ends a metre in front of its head vehicle: the image of the tail stands inside the head (gap = |dp| - half_len <
    0) from step 0 on.  Both forwards leave DHTS_FAULT_COLLISION (step 0, lane 1, the head vehicle) in the library's record, nothing on
    the device faults, the outputs are finite and those of the yardstick, and the operator prints the record and goes on."""
    import torch
    import dhts
    from dhts import _lib, ops
    from micro_ring_ref import ring_rollout
    V, T, S = 70, 5, 2
    count = [70, 9, 70, 70]
    rng, p0, v0, par, ring, cnt = ring_inputs(V, T, count, lanes_=4)
    ring[1] = float(p0[1, 8] - p0[1, 0]) + 1.0
    desc = ops.micro_desc(4, V, DT)
    tp0, tv0, tpar, t_ring = t32(p0, cuda), t32(v0, cuda), t64(par, cuda), t64(ring, cuda)
    t_cnt = torch.tensor(count, device=cuda, dtype=torch.int32)
    errs = [ops.new_error_record(cuda) for _ in range(2)]
    ckpt = torch.empty(ops.micro_ckpt_numel(desc, T, S), dtype=torch.float32, device=cuda)
    a = ops.micro_rollout_fwd_ckpt_ring(desc, T, tp0, tv0, tpar, t_ring, ckpt, None, 1, count=t_cnt, segment=S, err=errs[0])
    b = ops.micro_rollout_fwd_jvp_ring(desc, T, tp0, tv0, tpar, t_ring, tp0[None], tv0[None], None, 1, count=t_cnt, err=errs[1])
    assert [e.tolist() for e in errs] == [[_lib.FAULT_COLLISION, 0, 1, 8]] * 2
    for t in (a[0], a[1], a[2], b[0][0], b[0][1], b[1][0], b[1][1], b[1][2]):
        assert bool(torch.all(torch.isfinite(t)))
    assert same_bits(n(a[0]), n(b[0][0])) and same_bits(n(a[1]), n(b[0][1]))
    pT, vT, hist = ring_rollout(torch.tensor(p0), torch.tensor(v0), torch.tensor(par), ring, T, DT, count)
    e_s = max(rel_elem(n(a[0]), pT.numpy()), rel_elem(n(a[1]), vT.numpy()), rel_elem(n(a[2]), hist.numpy() * live_mask(4, V, count)[None, :, None, :]))
    print("a ring too short: states vs ring_rollout %.2e" % e_s)
    assert e_s <= TOL_STATE
    assert n(a[2])[0, 1, 1, 8] < 0.01 * v0[1, 8], "the head braked to a stop at once (the acceleration clip), as a follower that collides does"
    capsys.readouterr()
    out = dhts.micro_rollout(tp0, tv0, tpar, None, T, DT, count=t_cnt, checkpoint=S, ring=t_ring, probes=[0, 8], every=2)      # prints, does not raise
    assert "Collision detected between vehicles (step 0, lane 1, vehicle 8)" in capsys.readouterr().out
    assert tuple(out[2].shape) == (2, 4, 2, 2)


# =================================================================================================================
# 7. guard bands
# =================================================================================================================
def test_guard_bands_and_empty_rollouts(cuda):
    """tests/test_micro_lead_gpu.py::test_guard_bands_and_empty_rollouts for the five ring entry points: V = 65, T = 7, S = 3, ragged
    counts with an empty lane, the dense history of the raw level and a probe list every 2 steps, every output in the middle of a
    NaN-prefilled buffer.  No byte outside the views changes and every element inside is written.  T = 0, and count all zero: the state
    passes through, the gradients are the cotangents at live slots (none: exactly 0), nothing outside the outputs is written."""
    import torch
    import dhts
    from dhts import ops
    V, T, S, K = 65, 7, 3, 5
    Lg, count = 3, [65, 0, 64]
    rng, p0, v0, par, ring, _ = ring_inputs(V, T, count, lanes_=Lg)
    desc = ops.micro_desc(Lg, V, DT)
    cnt = torch.tensor(count, device=cuda, dtype=torch.int32)
    tp0, tv0, tpar, t_ring = t32(p0, cuda), t32(v0, cuda), t64(par, cuda), t64(ring, cuda)
    g_pT, g_vT = (t32(a, cuda) for a in rng.standard_normal((2, Lg, V)))
    t_p, t_v = (t32(a, cuda) for a in rng.standard_normal((2, K, Lg, V)))
    t_par = t64(rng.standard_normal((K, 6, Lg, V)), cuda)
    live = live_mask(Lg, V, count)

    def framed(shape, fill=None):
        buf, view = guarded(shape, cuda)
        if fill is not None:
            view.fill_(fill)
        return buf, view

    def frames_hold(bufs, unwritten=()):
        host = {}
        for name, (buf, view) in bufs.items():
            b = buf.cpu().numpy()
            assert np.all(np.isnan(b[:256])) and np.all(np.isnan(b[b.size - 256:])), "a guard band was written (%s)" % name
            host[name] = b[256:b.size - 256].reshape(view.shape)
            if name not in unwritten:
                assert np.all(np.isfinite(host[name])), "an element was not written (%s)" % name
        return host

    for every, probe_list in ((1, None), (2, [0, 33, 64])):
        probes = None if probe_list is None else torch.tensor(probe_list, device=cuda, dtype=torch.int32)
        R, P = T // every, V if probe_list is None else len(probe_list)
        g_samples = t32(rng.standard_normal((R, Lg, 2, P)), cuda)
        bufs = dict(ck=framed((ops.micro_ckpt_numel(desc, T, S),)), pT=framed((Lg, V)), vT=framed((Lg, V)), samples=framed((R, Lg, 2, P), 0.0),
                    g_p0=framed((Lg, V)), g_v0=framed((Lg, V)), jp=framed((Lg, V)), jv=framed((Lg, V)), jtp=framed((K, Lg, V)),
                    jtv=framed((K, Lg, V)), jsamples=framed((R, Lg, 2, P), 0.0), jt=framed((K, R, Lg, 2, P), 0.0))
        g_params = torch.full((6, Lg, V), float("nan"), dtype=torch.float64, device=cuda)
        errs = [ops.new_error_record(cuda) for _ in range(4)]
        out = ops.micro_rollout_fwd_ckpt_ring(desc, T, tp0, tv0, tpar, t_ring, bufs["ck"][1], probes, every, count=cnt, segment=S,
                                              samples=bufs["samples"][1], err=errs[0], out=(bufs["pT"][1], bufs["vT"][1]))
        assert out[2] is bufs["samples"][1]
        res = ops.micro_rollout_bwd_ckpt_ring(desc, T, bufs["ck"][1], tpar, t_ring, g_pT, g_vT, probes, every, g_samples, count=cnt, segment=S,
                                              err=errs[1], out=(bufs["g_p0"][1], bufs["g_v0"][1]), g_params=g_params)
        assert len(res) == 2 and res[0] is bufs["g_p0"][1]
        ops.micro_rollout_fwd_jvp_ring(desc, T, tp0, tv0, tpar, t_ring, t_p, t_v, probes, every, count=cnt, t_params=t_par, err=errs[2],
                                       err_jvp=errs[3], out=tuple(bufs[k][1] for k in ("jp", "jv", "jtp", "jtv", "jsamples", "jt")))
        torch.cuda.synchronize()
        assert all(e.tolist()[0] == 0 for e in errs)
        host = frames_hold(bufs, unwritten=("ck",))
        assert same_bits(n(t_ring), ring) and same_bits(n(tp0), p0) and same_bits(n(tpar), par), "an input was written"
        assert bool(torch.all(torch.isfinite(g_params))) and bool(torch.all(g_params[:, 1] == 0))
        assert same_bits(host["jp"], host["pT"]) and same_bits(host["jv"], host["vT"]) and same_bits(host["jsamples"], host["samples"])
        assert np.all(host["jt"][:, :, 1] == 0) and np.all(host["samples"][:, 1] == 0) and np.all(host["g_p0"][1] == 0)
        # the same calls through the public operators: the same numbers
        y = (tp0.clone().requires_grad_(True), tv0.clone().requires_grad_(True), tpar.clone().requires_grad_(True))
        pub = dhts.micro_rollout(*y, None, T, DT, count=cnt, checkpoint=S, ring=t_ring, every=every,
                                 probes=list(range(V)) if probe_list is None else probe_list)
        ((pub[0] * g_pT).sum() + (pub[1] * g_vT).sum() + (pub[2] * g_samples).sum()).backward()
        assert same_bits(n(pub[2]), host["samples"]) and np.array_equal(n(y[0].grad), host["g_p0"]) and np.array_equal(n(y[2].grad), n(g_params))
    # the target pair, framed the same way (its own segment plan)
    St = min(S, ops.micro_ckpt_target_plan(desc, T, True)["max_segment"])
    target = t32(rng.standard_normal((T, Lg, 2, V)), cuda)
    bufs = dict(ck=framed((ops.micro_ckpt_numel(desc, T, St),)), pT=framed((Lg, V)), vT=framed((Lg, V)), g_p0=framed((Lg, V)), g_v0=framed((Lg, V)))
    g_params = torch.full((6, Lg, V), float("nan"), dtype=torch.float64, device=cuda)
    sse = torch.full((Lg, 2), float("nan"), dtype=torch.float64, device=cuda)
    errs = [ops.new_error_record(cuda) for _ in range(2)]
    ops.micro_rollout_fwd_ckpt_target_ring(desc, T, tp0, tv0, tpar, t_ring, bufs["ck"][1], target, count=cnt, segment=St, sse=sse, err=errs[0],
                                           out=(bufs["pT"][1], bufs["vT"][1]))
    ops.micro_rollout_bwd_ckpt_target_ring(desc, T, bufs["ck"][1], tpar, t_ring, g_pT, g_vT, target, g_sse=torch.ones_like(sse), count=cnt,
                                           segment=St, err=errs[1], out=(bufs["g_p0"][1], bufs["g_v0"][1]), g_params=g_params)
    torch.cuda.synchronize()
    assert all(e.tolist()[0] == 0 for e in errs)
    frames_hold(bufs, unwritten=("ck",))
    assert bool(torch.all(torch.isfinite(sse))) and bool(torch.all(sse[1] == 0)) and bool(torch.all(torch.isfinite(g_params)))
    # T = 0, and count all zero with T = 7: nothing happens
    for T0, cnt0 in ((0, cnt), (T, torch.zeros(Lg, device=cuda, dtype=torch.int32))):
        live0 = live if T0 == 0 else np.zeros((Lg, V), bool)
        R0 = T0
        bufs = dict(ck=framed((max(ops.micro_ckpt_numel(desc, T0, S), 1),)), pT=framed((Lg, V)), vT=framed((Lg, V)), samples=framed((R0, Lg, 2, V), 0.0),
                    g_p0=framed((Lg, V)), g_v0=framed((Lg, V)), jp=framed((Lg, V)), jv=framed((Lg, V)), jtp=framed((K, Lg, V)),
                    jtv=framed((K, Lg, V)), jsamples=framed((R0, Lg, 2, V), 0.0), jt=framed((K, R0, Lg, 2, V), 0.0))
        ck0 = bufs["ck"][1][:ops.micro_ckpt_numel(desc, T0, S)]
        g_params = torch.full((6, Lg, V), float("nan"), dtype=torch.float64, device=cuda)
        g_samples = t32(rng.standard_normal((R0, Lg, 2, V)), cuda)
        err = ops.new_error_record(cuda)
        ops.micro_rollout_fwd_ckpt_ring(desc, T0, tp0, tv0, tpar, t_ring, ck0, None, 1, count=cnt0, segment=S, samples=bufs["samples"][1], err=err,
                                        out=(bufs["pT"][1], bufs["vT"][1]))
        ops.micro_rollout_bwd_ckpt_ring(desc, T0, ck0, tpar, t_ring, g_pT, g_vT, None, 1, g_samples, count=cnt0, segment=S, err=err,
                                        out=(bufs["g_p0"][1], bufs["g_v0"][1]), g_params=g_params)
        ops.micro_rollout_fwd_jvp_ring(desc, T0, tp0, tv0, tpar, t_ring, t_p, t_v, None, 1, count=cnt0, t_params=t_par, err=err,
                                       out=tuple(bufs[k][1] for k in ("jp", "jv", "jtp", "jtv", "jsamples", "jt")))
        torch.cuda.synchronize()
        host = frames_hold(bufs, unwritten=("ck",))
        assert err.tolist()[0] == 0
        assert same_bits(host["pT"], p0) and same_bits(host["vT"], v0) and same_bits(host["jp"], p0) and same_bits(host["jv"], v0)
        assert np.array_equal(host["g_p0"], n(g_pT) * live0) and np.array_equal(host["g_v0"], n(g_vT) * live0)
        assert np.array_equal(host["jtp"], n(t_p) * live0[None]) and np.array_equal(host["jtv"], n(t_v) * live0[None])
        assert np.all(host["samples"] == 0) and np.all(host["jsamples"] == 0) and np.all(host["jt"] == 0)
        assert bool(torch.all(g_params == 0))


# =================================================================================================================
# 8. the example
# =================================================================================================================
@pytest.mark.parametrize("mode", (["--checkpoint"], ["--checkpoint", "--fused-loss"], ["--checkpoint", "--observe", "2,5"],
                                  ["--method", "lm", "--fused"]), ids=("adam_checkpoint", "fused_loss", "observe", "lm_fused"))
def test_calibration_example_on_a_ring(cuda, tmp_path, mode):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "calibrate_idm.py"), "--ring", "200", "--seed", "1", "--n_lane", "3",
                          "--n_vehicle", "9", "--n_step", "40", "--n_episode", "5"] + mode, cwd=str(tmp_path), env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    files = [os.path.join(dp, f) for dp, _, fs in os.walk(str(tmp_path)) for f in fs if f.startswith("trial_") and f.endswith(".txt")]
    assert len(files) == 1, "one trial_k.txt per run"
    losses = [float(line.split()[1]) for line in open(files[0]).read().splitlines()]
    print("calibrate_idm.py --ring 200 %s: loss %s" % (" ".join(mode), " ".join("%.6g" % x for x in losses)))
    assert len(losses) == 5 and all(np.isfinite(losses))
    assert losses[-1] < losses[0]
