"""A recorded leader on the two tape-free paths of the micro rollout, on the device: dhts.micro_rollout(lead=, lead_length=) with
checkpoint= and dhts.micro_rollout_jvp(lead=, lead_length=, t_lead=, fused=True).  Every yardstick is code that existed before them:
  1. the split identity -- the existing dense path (want_hist=True) on whole lanes; a lane cut behind vehicle j, with vehicle j's
     recorded trajectory as `lead` and its length as `lead_length`, must give the same bits for the vehicles behind it;
  2. g_lead / t_lead -- T chained one-step calls of the existing dhts.micro_rollout(T=1) / micro_rollout_jvp(T=1) on lanes that hold
     the leader in a slot of their own, lead[t] a fresh leaf per step;
  3. a full lane of 1024, whose leader has no slot in such a chain: tests/micro_lead_ref.py::lead_rollout (validated on the CPU in
     tests/test_micro_lead.py).
Then guard bands, the fault records, the memory that is not allocated and the calibration example.
Needs a real MI355X: python -m pytest tests -m gpu"""
import os
import subprocess
import sys

import numpy as np
import pytest

from micro_lead_ref import restated_lead, trajectory_before_steps
from test_micro_ckpt_gpu import live_mask, same_bits
from test_micro_jvp_gpu import CASES, DT, IDS, case_inputs, guarded
from test_micro_params import per_plane
from test_micro_params_gpu import lanes
from util import TOL_GRAD, TOL_STATE, grad_report, rel_elem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT = [c for c in CASES if (c[0], c[1], c[2]) in ((3, 2, 7), (3, 64, 50), (3, 65, 1), (5, 130, 50), (3, 1024, 20), (3, 70, 0))]
SPLIT_IDS = [IDS[CASES.index(c)] for c in SPLIT]
CHAIN = [c for c in CASES if (c[0], c[1], c[2]) in ((3, 1, 3), (3, 2, 7), (3, 64, 50), (5, 130, 50))] + [(3, 1024, 20, [1023, 1023, 1023])]
CHAIN_IDS = [IDS[CASES.index(c)] for c in CHAIN[:-1]] + ["L3_V1024_T20_count1023"]


def samplings(T, V):
    """(every, probes) of a call; None: no samples at all.  (1, None) is the dense history, which the public call spells
    probes=range(V), every=1 (probes=None with every=1 is the call without samples there; the raw wrappers take (1, None) as it is, in
    the guard-band test; so T + 1 = 1 at T = 0 is spelled with the list too)."""
    return [None, (1, list(range(V))), (2, [0]), (3, sorted({0, V // 3, V // 2, V - 1})), (T + 1, None if T else list(range(V)))]


def cut(hist, sampling):
    every, probes = sampling
    c = hist[..., every - 1::every, :, :, :]
    return c if probes is None else c[..., probes]


def split_points(count, V, L, i):
    """Split point of every lane for variant i of {1, count // 2, count - 1}; 0 (an empty lane) where no vehicle has a vehicle behind it."""
    cnt = [V] * L if count is None else count
    return [0 if c < 2 else max(1, (1, c // 2, c - 1)[i]) for c in cnt]


def lead_of(x0, hist_x, js):
    """[T][L] what vehicle js[l] of lane l is seen at in step t, from x0 [L][V] and the dense history's plane hist_x [T][L][V]."""
    L = x0.shape[0]
    return np.stack([trajectory_before_steps(x0[l, js[l]], hist_x[:, l, js[l]]) for l in range(L)], 1)


def t32(a, cuda, grad=False):
    import torch
    return torch.tensor(np.ascontiguousarray(a, np.float32), device=cuda, requires_grad=grad)


def t64(a, cuda, grad=False):
    import torch
    return torch.tensor(np.ascontiguousarray(a, np.float64), device=cuda, dtype=torch.float64, requires_grad=grad)


def n(t):
    return None if t is None else t.detach().cpu().numpy()


# =================================================================================================================
# 1. the split identity
# =================================================================================================================
@pytest.mark.parametrize("case", SPLIT, ids=SPLIT_IDS)
def test_reverse_mode_of_a_lane_cut_behind_a_recorded_vehicle(cuda, case):
    """pT, vT and the samples at live slots: the dense path's bits.  g_p0, g_v0, g_params of the vehicles behind the split:
    np.array_equal to the dense path's under cotangents that are zero from the split on.  checkpoint in {1, 3, True, max_segment} x
    params.requires_grad x five sampling settings x three split points."""
    import torch
    import dhts
    from dhts import ops
    L, V, T, count = case
    p0, v0, par, head, _ = case_inputs(case)
    rng = np.random.default_rng(5 * V + T)
    cnt = None if count is None else torch.tensor(count, device=cuda, dtype=torch.int32)
    desc = ops.micro_desc(L, V, DT)
    g_pT, g_vT = rng.standard_normal((2, L, V)).astype(np.float32)
    g_hist = rng.standard_normal((T, L, 2, V)).astype(np.float32)
    with torch.no_grad():
        _, _, hist = dhts.micro_rollout(t32(p0, cuda), t32(v0, cuda), t64(par, cuda), t64(head, cuda), T, DT, count=cnt, want_hist=True)
    hist = n(hist)
    runs = 0
    for i in range(3):
        js = split_points(count, V, L, i)
        behind = live_mask(L, V, js)                                  # the vehicles behind the split: what is compared
        lead = np.stack([lead_of(p0, hist[:, :, 0], js), lead_of(v0, hist[:, :, 1], js)], -1).astype(np.float32)       # [T][L][2]
        lead_len = np.array([par[5, l, js[l]] for l in range(L)])
        t_lead, t_len, t_cnt = t32(lead, cuda), t64(lead_len, cuda), torch.tensor(js, device=cuda, dtype=torch.int32)
        m_pT, m_vT = g_pT * behind, g_vT * behind
        for sampling in samplings(T, V):
            # the dense yardstick: the loss on the cut of hist, cotangents zero from the split on
            x = (t32(p0, cuda, True), t32(v0, cuda, True), t64(par, cuda, True), t64(head, cuda))
            d_pT, d_vT, d_hist = dhts.micro_rollout(*x, T, DT, count=cnt, want_hist=True)
            loss = (d_pT * t32(m_pT, cuda)).sum() + (d_vT * t32(m_vT, cuda)).sum()
            g_s = live_p = None
            if sampling is not None:
                every, probes = sampling
                cols = list(range(V)) if probes is None else probes
                live_p = behind[:, cols]
                g_s = np.ascontiguousarray(cut(g_hist, sampling) * live_p[:, None, :])
                d_samples = d_hist[every - 1::every]
                if probes is not None:
                    d_samples = d_samples[..., torch.tensor(probes, device=cuda)]
                loss = loss + (d_samples * t32(g_s, cuda)).sum()
            loss.backward()
            want = dict(pT=n(d_pT), vT=n(d_vT), g_p0=n(x[0].grad), g_v0=n(x[1].grad), g_params=n(x[2].grad))
            for want_params in (False, True):
                for ck in (1, 3, True, ops.micro_ckpt_plan(desc, T, want_params)["max_segment"]):
                    y = (t32(p0, cuda, True), t32(v0, cuda, True), t64(par, cuda, want_params))
                    kw = {} if sampling is None else dict(every=sampling[0], probes=sampling[1])
                    out = dhts.micro_rollout(*y, None, T, DT, count=t_cnt, checkpoint=ck, lead=t_lead, lead_length=t_len, **kw)
                    assert len(out) == (2 if sampling is None else 3)
                    loss = (out[0] * t32(m_pT, cuda)).sum() + (out[1] * t32(m_vT, cuda)).sum()
                    if sampling is not None:
                        loss = loss + (out[2] * t32(g_s, cuda)).sum()
                    loss.backward()
                    tag = "split %d, sampling %s, checkpoint %s, params %s" % (i, sampling and sampling[0], ck, want_params)
                    assert same_bits(n(out[0])[behind], want["pT"][behind]) and same_bits(n(out[1])[behind], want["vT"][behind]), tag
                    if sampling is not None:
                        got = n(out[2])
                        m = np.broadcast_to(live_p[:, None, :], got.shape)
                        assert same_bits(got[m], cut(hist, sampling)[m]), tag
                        assert np.all(got[~m] == 0), tag
                    assert np.array_equal(n(y[0].grad)[behind], want["g_p0"][behind]), tag
                    assert np.array_equal(n(y[1].grad)[behind], want["g_v0"][behind]), tag
                    assert np.all(n(y[0].grad)[~behind] == 0) and np.all(n(y[1].grad)[~behind] == 0), tag
                    if want_params:
                        bq = np.broadcast_to(behind, (6, L, V))
                        assert np.array_equal(n(y[2].grad)[bq], want["g_params"][bq]), tag
                        assert np.all(n(y[2].grad)[~bq] == 0), tag
                    runs += 1
    assert runs == 3 * 5 * 2 * 4


@pytest.mark.parametrize("case", SPLIT, ids=SPLIT_IDS)
def test_fused_forward_mode_of_a_lane_cut_behind_a_recorded_vehicle(cuda, case):
    """K in {1, 4, 5}, with and without t_params, t_lead the dense fused path's tangents of the split vehicle: t_pT, t_vT and t_samples
    (and the primal outputs) are the dense fused=True result's bits behind the split.  The recorded vehicle's length is a constant of
    the cut lane, so its tangent is zero in the dense call too."""
    import torch
    import dhts
    L, V, T, count = case
    p0, v0, par, head, _ = case_inputs(case)
    rng = np.random.default_rng(7 * V + T)
    cnt = None if count is None else torch.tensor(count, device=cuda, dtype=torch.int32)
    base = (t32(p0, cuda), t32(v0, cuda), t64(par, cuda))
    runs = 0
    for i, K in enumerate((1, 4, 5)):
        js = split_points(count, V, L, i)
        behind = live_mask(L, V, js)
        t_cnt = torch.tensor(js, device=cuda, dtype=torch.int32)
        t_len = t64([par[5, l, js[l]] for l in range(L)], cuda)
        t_p0, t_v0 = rng.standard_normal((2, K, L, V)).astype(np.float32)
        t_head = rng.standard_normal((K, L, 2))
        t_par = rng.standard_normal((K, 6, L, V))
        for l in range(L):
            t_par[:, 5, l, js[l]] = 0.0
        for with_params in (False, True):
            tq = dict(t_params=t64(t_par, cuda)) if with_params else {}
            (d_pT, d_vT, d_hist), (d_tp, d_tv, d_thist) = dhts.micro_rollout_jvp(
                *base, t64(head, cuda), T, DT, t_p0=t32(t_p0, cuda), t_v0=t32(t_v0, cuda), t_head=t64(t_head, cuda), count=cnt, want_hist=True,
                fused=True, **tq)
            d_hist, d_thist = n(d_hist), n(d_thist)
            lead = np.stack([lead_of(p0, d_hist[:, :, 0], js), lead_of(v0, d_hist[:, :, 1], js)], -1).astype(np.float32)
            t_lead = np.stack([np.stack([lead_of(t_p0[k], d_thist[k][:, :, 0], js), lead_of(t_v0[k], d_thist[k][:, :, 1], js)], -1)
                               for k in range(K)]).astype(np.float32)                                    # [K][T][L][2]
            for sampling in samplings(T, V):
                kw = {} if sampling is None else dict(every=sampling[0], probes=sampling[1])
                prim, tang = dhts.micro_rollout_jvp(*base, None, T, DT, t_p0=t32(t_p0, cuda), t_v0=t32(t_v0, cuda), count=t_cnt, fused=True,
                                                    lead=t32(lead, cuda), lead_length=t_len, t_lead=t32(t_lead, cuda), **tq, **kw)
                tag = "K %d, t_params %s, sampling %s" % (K, with_params, sampling and sampling[0])
                assert len(prim) == len(tang) == (2 if sampling is None else 3), tag
                assert same_bits(n(prim[0])[behind], n(d_pT)[behind]) and same_bits(n(prim[1])[behind], n(d_vT)[behind]), tag
                bk = np.broadcast_to(behind, (K, L, V))
                assert same_bits(n(tang[0])[bk], n(d_tp)[bk]) and same_bits(n(tang[1])[bk], n(d_tv)[bk]), tag
                assert np.all(n(tang[0])[~bk] == 0) and np.all(n(tang[1])[~bk] == 0), tag
                if sampling is not None:
                    cols = list(range(V)) if sampling[1] is None else sampling[1]
                    got, t_got = n(prim[2]), n(tang[2])
                    m = np.broadcast_to(behind[:, cols][:, None, :], got.shape)
                    mk = np.broadcast_to(m, t_got.shape)
                    assert same_bits(got[m], cut(d_hist, sampling)[m]) and np.all(got[~m] == 0), tag
                    assert same_bits(t_got[mk], cut(d_thist, sampling)[mk]) and np.all(t_got[~mk] == 0), tag
                runs += 1
    assert runs == 3 * 2 * 5


# =================================================================================================================
# 2. g_lead and t_lead against chained one-step calls of the existing operators
# =================================================================================================================
def moving_leaders(rng, p0, count, V, T):
    """A leader per lane some way in front of the head vehicle that speeds up and slows down: [T][L][2] float32."""
    L = p0.shape[0]
    cnt = [V] * L if count is None else count
    v = np.clip(14.0 + np.cumsum(rng.normal(0.0, 1.0, (T, L)), 0), 1.0, 28.0)
    start = np.array([p0[l, c - 1] + 22.0 if c > 0 else 10.0 for l, c in enumerate(cnt)])
    p = start[None, :] + np.concatenate([np.zeros((1, L)), np.cumsum(v[:-1] * DT, 0)], 0) if T else np.zeros((0, L))
    return np.stack([p, v], -1).astype(np.float32)


def chain_inputs(case):
    """The inputs of a chain case: the lanes of V1 slots that hold the leader in slot count, and the V-slot lanes of the new call."""
    L, V, T, count = case
    cnt = [V] * L if count is None else count
    V1 = V + 1 if max(cnt) == V else V
    rng = np.random.default_rng(13 * V + T)
    p1, v1, par1, head = lanes(rng, L, V1)
    lead = moving_leaders(rng, p1, cnt, V, T)
    lead_len = np.array([par1[5, l, c] for l, c in enumerate(cnt)]) + 1.5        # (not the head's own length)
    for l, c in enumerate(cnt):
        par1[5, l, c] = lead_len[l]
    sampling = (3, sorted({0, V // 3, V // 2, V - 1})) if T >= 3 else (1, None)
    return cnt, V1, rng, p1, v1, par1, head, lead, lead_len, sampling


@pytest.mark.parametrize("case", CHAIN, ids=CHAIN_IDS)
def test_g_lead_against_chained_one_step_rollouts(cuda, case):
    """T calls of dhts.micro_rollout(T=1) on lanes of count + 1 vehicles, slot count replaced by the fresh leaf lead[t] before each call
    and its output dropped (zero cotangent: a step's output of the leader is not part of lead).  Random cotangents on pT, vT and the
    samples.  pT, vT, samples: same bits; g_p0, g_v0, g_lead: np.array_equal, an empty lane's rows exactly 0; g_params plane by plane
    at TOL_GRAD (the chain folds the length sums once per call, the rollout once over the sums)."""
    import torch
    import dhts
    L, V, T, _ = case
    cnt, V1, rng, p1, v1, par1, head, lead, lead_len, sampling = chain_inputs(case)
    every, probes = sampling
    cols = list(range(V)) if probes is None else probes
    live = live_mask(L, V, cnt)
    R = T // every
    g_pT, g_vT = rng.standard_normal((2, L, V)).astype(np.float32)
    g_s = rng.standard_normal((R, L, 2, len(cols))).astype(np.float32)
    idx = torch.tensor(cnt, device=cuda, dtype=torch.int64)[:, None]
    live1 = torch.tensor(live_mask(L, V1, cnt), device=cuda)
    # ---- the chain ----
    c_p0, c_v0, c_par = t32(p1, cuda, True), t32(v1, cuda, True), t64(par1, cuda, True)
    c_head = t64(head, cuda)
    c_cnt = torch.tensor([c + 1 for c in cnt], device=cuda, dtype=torch.int32)
    leaves = [t32(lead[t], cuda, True) for t in range(T)]
    p, v, rows = c_p0, c_v0, []
    for t in range(T):
        p_in, v_in = p.scatter(1, idx, leaves[t][:, 0:1]), v.scatter(1, idx, leaves[t][:, 1:2])
        p, v = dhts.micro_rollout(p_in, v_in, c_par, c_head, 1, DT, count=c_cnt)
        if (t + 1) % every == 0:
            rows.append(torch.stack([p[:, cols], v[:, cols]], 1))
    zero = torch.zeros((), device=cuda)
    c_pT, c_vT = torch.where(live1, p, zero)[:, :V], torch.where(live1, v, zero)[:, :V]       # (the leader's output takes no cotangent)
    loss = (c_pT * t32(g_pT, cuda)).sum() + (c_vT * t32(g_vT, cuda)).sum()
    c_samples = torch.stack(rows) if rows else torch.zeros(0, L, 2, len(cols), device=cuda)
    lp = torch.tensor(live[:, cols], device=cuda)
    if rows:
        loss = loss + (torch.where(lp[:, None, :], c_samples, zero) * t32(g_s, cuda)).sum()
    loss.backward()
    c_g_lead = np.stack([n(x.grad) if x.grad is not None else np.zeros((L, 2), np.float32) for x in leaves]) if T else np.zeros((0, L, 2))
    # ---- the rollout with the recorded leader ----
    for ck in (1, 3, True):
        y = (t32(p1[:, :V], cuda, True), t32(v1[:, :V], cuda, True), t64(par1[:, :, :V], cuda, True))
        y_lead = t32(lead, cuda, True)
        pT, vT, samples = dhts.micro_rollout(*y, None, T, DT, count=torch.tensor(cnt, device=cuda, dtype=torch.int32), checkpoint=ck,
                                             lead=y_lead, lead_length=t64(lead_len, cuda), every=every,
                                             probes=cols if probes is not None or every == 1 else None)
        ((pT * t32(g_pT, cuda)).sum() + (vT * t32(g_vT, cuda)).sum() + (samples * t32(g_s, cuda)).sum()).backward()
        assert same_bits(n(pT)[live], n(c_pT)[live]) and same_bits(n(vT)[live], n(c_vT)[live])
        m = np.broadcast_to(live[:, cols][:, None, :], samples.shape)
        assert same_bits(n(samples)[m], n(c_samples)[m]) and np.all(n(samples)[~m] == 0)
        assert np.array_equal(n(y[0].grad)[live], n(c_p0.grad)[:, :V][live]) and np.all(n(y[0].grad)[~live] == 0)
        assert np.array_equal(n(y[1].grad)[live], n(c_v0.grad)[:, :V][live]) and np.all(n(y[1].grad)[~live] == 0)
        g_lead = n(y_lead.grad)
        assert g_lead.shape == (T, L, 2) and g_lead.dtype == np.float32
        assert np.array_equal(g_lead, c_g_lead), "checkpoint %s: g_lead differs from the chain's leaves" % (ck,)
        for l, c in enumerate(cnt):
            if c == 0:
                assert np.all(g_lead[:, l] == 0)
        assert T == 0 or np.any(g_lead != 0)
        got, ref = n(y[2].grad) * live[None], n(c_par.grad)[:, :, :V] * live[None]
        worst = per_plane("checkpoint %s: g_params against the chain" % (ck,), got, ref) if T else 0.0
        print("L %d V %d T %d checkpoint %s: g_params vs chained one-step calls, worst plane %.2e" % (L, V, T, ck, worst))
        assert worst <= TOL_GRAD
        assert np.all(n(y[2].grad)[~np.broadcast_to(live, (6, L, V))] == 0)


@pytest.mark.parametrize("case", CHAIN, ids=CHAIN_IDS)
def test_t_lead_against_chained_one_step_tangent_sweeps(cuda, case):
    """The same chain through dhts.micro_rollout_jvp(T=1), K = 5 (a launch of four and one of one), with t_params: direction k's t_lead[t]
    replaces the leader slot's tangents before each call.  Same bits for the primal outputs, t_pT, t_vT and t_samples."""
    import torch
    import dhts
    L, V, T, _ = case
    K = 5
    cnt, V1, rng, p1, v1, par1, head, lead, lead_len, sampling = chain_inputs(case)
    every, probes = sampling
    cols = list(range(V)) if probes is None else probes
    live = live_mask(L, V, cnt)
    t_p0, t_v0 = rng.standard_normal((2, K, L, V1)).astype(np.float32)
    t_par = rng.standard_normal((K, 6, L, V1))
    t_lead = rng.standard_normal((K, T, L, 2)).astype(np.float32)
    t_lead[1] = 0.0                                   # a direction without a leader tangent
    for l, c in enumerate(cnt):
        t_par[:, 5, l, c] = 0.0                       # the leader's length is a constant
    idx = torch.tensor(cnt, device=cuda, dtype=torch.int64)[:, None]
    idk = idx[None].expand(K, L, 1)
    c_cnt = torch.tensor([c + 1 for c in cnt], device=cuda, dtype=torch.int32)
    c_par, c_head, c_tpar = t64(par1, cuda), t64(head, cuda), t64(t_par, cuda)
    p, v, tp, tv = t32(p1, cuda), t32(v1, cuda), t32(t_p0, cuda), t32(t_v0, cuda)
    d_lead, d_tlead = t32(lead, cuda), t32(t_lead, cuda)
    rows, t_rows = [], []
    for t in range(T):
        p, v = p.scatter(1, idx, d_lead[t][:, 0:1]), v.scatter(1, idx, d_lead[t][:, 1:2])
        tp, tv = tp.scatter(2, idk, d_tlead[:, t, :, 0:1]), tv.scatter(2, idk, d_tlead[:, t, :, 1:2])
        (p, v), (tp, tv) = dhts.micro_rollout_jvp(p, v, c_par, c_head, 1, DT, t_p0=tp, t_v0=tv, t_params=c_tpar, count=c_cnt)
        if (t + 1) % every == 0:
            rows.append(torch.stack([p[:, cols], v[:, cols]], 1))
            t_rows.append(torch.stack([tp[:, :, cols], tv[:, :, cols]], 2))
    prim, tang = dhts.micro_rollout_jvp(t32(p1[:, :V], cuda), t32(v1[:, :V], cuda), t64(par1[:, :, :V], cuda), None, T, DT,
                                        t_p0=t32(t_p0[:, :, :V], cuda), t_v0=t32(t_v0[:, :, :V], cuda), t_params=t64(t_par[:, :, :, :V], cuda),
                                        count=torch.tensor(cnt, device=cuda, dtype=torch.int32), fused=True, lead=d_lead,
                                        lead_length=t64(lead_len, cuda), t_lead=d_tlead, every=every,
                                        probes=cols if probes is not None or every == 1 else None)
    lk = np.broadcast_to(live, (K, L, V))
    assert same_bits(n(prim[0])[live], n(p)[:, :V][live]) and same_bits(n(prim[1])[live], n(v)[:, :V][live])
    assert same_bits(n(tang[0])[lk], n(tp)[:, :, :V][lk]) and same_bits(n(tang[1])[lk], n(tv)[:, :, :V][lk])
    assert np.all(n(tang[0])[~lk] == 0) and np.all(n(tang[1])[~lk] == 0)
    if rows:
        m = np.broadcast_to(live[:, cols][:, None, :], prim[2].shape)
        mk = np.broadcast_to(m, tang[2].shape)
        assert same_bits(n(prim[2])[m], n(torch.stack(rows))[m])
        assert same_bits(n(tang[2])[mk], n(torch.stack(t_rows, 1))[mk]) and np.all(n(tang[2])[~mk] == 0)
        assert np.any(n(tang[2])[mk] != 0)
    else:
        assert prim[2].shape[0] == 0 and tang[2].shape[1] == 0


def test_a_full_lane_of_1024_against_the_restated_rollout(cuda):
    """count = capacity = 1024: thread 1023 is the head and slot 1024 of the hand-over arrays the leader -- no V + 1 chain holds it.
    Against tests/micro_lead_ref.py::lead_rollout: states at TOL_STATE, gradients at TOL_GRAD (g_params plane by plane)."""
    import torch
    import dhts
    L, V, T = 2, 1024, 20
    rng = np.random.default_rng(1024)
    p0, v0, par, _ = lanes(rng, L, V)
    lead = moving_leaders(rng, p0, None, V, T)
    lead_len = np.array([6.5, 4.0])
    g_pT, g_vT = rng.standard_normal((2, L, V)).astype(np.float32)
    g_hist = (0.1 * rng.standard_normal((T, L, 2, V))).astype(np.float32)
    ref = restated_lead(p0, v0, par, lead, T, DT, lead_length=lead_len, g_pT=g_pT, g_vT=g_vT, g_hist=g_hist)
    y = (t32(p0, cuda, True), t32(v0, cuda, True), t64(par, cuda, True))
    y_lead = t32(lead, cuda, True)
    pT, vT, samples = dhts.micro_rollout(*y, None, T, DT, checkpoint=True, lead=y_lead, lead_length=t64(lead_len, cuda), every=1,
                                         probes=list(range(V)))
    ((pT * t32(g_pT, cuda)).sum() + (vT * t32(g_vT, cuda)).sum() + (samples * t32(g_hist, cuda)).sum()).backward()
    e_s = max(rel_elem(n(pT), ref["pT"]), rel_elem(n(vT), ref["vT"]), rel_elem(n(samples), ref["hist"]))
    print("full lane of 1024: states vs lead_rollout %.2e" % e_s)
    assert e_s <= TOL_STATE
    assert grad_report("full lane d loss / d p0", n(y[0].grad), ref["g_p0"]) <= TOL_GRAD
    assert grad_report("full lane d loss / d v0", n(y[1].grad), ref["g_v0"]) <= TOL_GRAD
    assert grad_report("full lane d loss / d lead", n(y_lead.grad), ref["g_lead"]) <= TOL_GRAD
    assert per_plane("full lane", n(y[2].grad), ref["g_params"]) <= TOL_GRAD
    assert all(np.any(n(y_lead.grad)[:, l] != 0) for l in range(L)), "the head's thread wrote the rows"
    # the fused kernel: its primal is the checkpointed forward's bits, and a tangent of the leader alone reaches the head vehicle
    t_lead = rng.standard_normal((1, T, L, 2)).astype(np.float32)
    prim, tang = dhts.micro_rollout_jvp(t32(p0, cuda), t32(v0, cuda), t64(par, cuda), None, T, DT, t_lead=t32(t_lead, cuda), fused=True,
                                        lead=t32(lead, cuda), lead_length=t64(lead_len, cuda))
    assert same_bits(n(prim[0]), n(pT)) and same_bits(n(prim[1]), n(vT))
    assert np.all(np.isfinite(n(tang[0]))) and np.all(np.isfinite(n(tang[1]))) and np.all(n(tang[1])[0, :, V - 1] != 0)


# =================================================================================================================
# 3. guard bands
# =================================================================================================================
def test_guard_bands_and_empty_rollouts(cuda):
    """The three raw wrappers at V = 65, T = 7, S = 3 with ragged counts (an empty lane among them), probes = None / every = 1 -- the
    dense history of the raw level -- and a probe list every 2 steps: lead, t_lead and every output in the middle of NaN-prefilled
    buffers.  No byte outside the views changes, the inputs keep their bytes, g_lead is handed in as garbage and every row of it is
    written (the empty lane's exactly 0).  T = 0 launches, and g_lead is empty."""
    import torch
    from dhts import ops
    L, V, T, S, K = 3, 65, 7, 3, 5
    count = [65, 0, 64]
    rng = np.random.default_rng(17)
    p0, v0, par, _ = lanes(rng, L, V)
    desc = ops.micro_desc(L, V, DT)
    cnt = torch.tensor(count, device=cuda, dtype=torch.int32)
    tp0, tv0, tpar = t32(p0, cuda), t32(v0, cuda), t64(par, cuda)
    g_pT, g_vT = (t32(a, cuda) for a in rng.standard_normal((2, L, V)))
    t_p, t_v = (t32(a, cuda) for a in rng.standard_normal((2, K, L, V)))
    t_par = t64(rng.standard_normal((K, 6, L, V)), cuda)
    lead_np = moving_leaders(rng, p0, count, V, T)
    t_lead_np = rng.standard_normal((K, T, L, 2)).astype(np.float32)
    lead_len = t64([6.0, 5.0, 4.5], cuda)
    for every, probe_list in ((1, None), (2, [0, 33, 64])):
        probes = None if probe_list is None else torch.tensor(probe_list, device=cuda, dtype=torch.int32)
        R, P = T // every, V if probe_list is None else len(probe_list)
        g_samples = t32(rng.standard_normal((R, L, 2, P)), cuda)

        def framed(shape, fill=None):
            buf, view = guarded(shape, cuda)
            if fill is not None:
                view.copy_(torch.as_tensor(fill, device=cuda)) if not np.isscalar(fill) else view.fill_(fill)
            return buf, view

        bufs = dict(lead=framed((T, L, 2), lead_np), t_lead=framed((K, T, L, 2), t_lead_np), ck=framed((ops.micro_ckpt_numel(desc, T, S),)),
                    pT=framed((L, V)), vT=framed((L, V)), samples=framed((R, L, 2, P), 0.0), g_p0=framed((L, V)), g_v0=framed((L, V)),
                    g_lead=framed((T, L, 2)), jp=framed((L, V)), jv=framed((L, V)), jtp=framed((K, L, V)), jtv=framed((K, L, V)),
                    jsamples=framed((R, L, 2, P), 0.0), jt=framed((K, R, L, 2, P), 0.0))
        g_params = torch.full((6, L, V), float("nan"), dtype=torch.float64, device=cuda)
        errs = [ops.new_error_record(cuda) for _ in range(4)]
        lead, t_lead = bufs["lead"][1], bufs["t_lead"][1]
        out = ops.micro_rollout_fwd_ckpt_lead(desc, T, tp0, tv0, tpar, lead, bufs["ck"][1], probes, every, lead_length=lead_len, count=cnt,
                                              segment=S, samples=bufs["samples"][1], err=errs[0], out=(bufs["pT"][1], bufs["vT"][1]))
        assert out[2] is bufs["samples"][1]
        res = ops.micro_rollout_bwd_ckpt_lead(desc, T, bufs["ck"][1], tpar, lead, g_pT, g_vT, probes, every, g_samples, lead_length=lead_len,
                                              count=cnt, segment=S, err=errs[1], out=(bufs["g_p0"][1], bufs["g_v0"][1]),
                                              g_lead=bufs["g_lead"][1], g_params=g_params)
        assert res[2] is bufs["g_lead"][1]
        ops.micro_rollout_fwd_jvp_lead(desc, T, tp0, tv0, tpar, lead, t_p, t_v, probes, every, lead_length=lead_len, count=cnt, t_lead=t_lead,
                                       t_params=t_par, err=errs[2], err_jvp=errs[3],
                                       out=tuple(bufs[k][1] for k in ("jp", "jv", "jtp", "jtv", "jsamples", "jt")))
        torch.cuda.synchronize()
        assert all(e.tolist()[0] == 0 for e in errs)
        host = {}
        for name, (buf, view) in bufs.items():
            b = buf.cpu().numpy()
            assert np.all(np.isnan(b[:256])) and np.all(np.isnan(b[b.size - 256:])), "a guard band was written (%s)" % name
            host[name] = b[256:b.size - 256].reshape(view.shape)
            if name != "ck":
                assert np.all(np.isfinite(host[name])), "an element was not written (%s)" % name
        assert same_bits(host["lead"], lead_np) and same_bits(host["t_lead"], t_lead_np), "an input was written"
        assert np.all(host["g_lead"][:, 1] == 0) and np.any(host["g_lead"][:, 0] != 0) and np.any(host["g_lead"][:, 2] != 0)
        assert bool(torch.all(torch.isfinite(g_params)))
        assert same_bits(host["jp"], host["pT"]) and same_bits(host["jv"], host["vT"]) and same_bits(host["jsamples"], host["samples"])
        assert np.all(host["jt"][:, :, 1] == 0) and np.all(host["samples"][:, 1] == 0)
        # the same calls through the public operators: the same numbers
        y = (tp0.clone().requires_grad_(True), tv0.clone().requires_grad_(True), tpar.clone().requires_grad_(True))
        y_lead = t32(lead_np, cuda, True)
        import dhts
        pub = dhts.micro_rollout(*y, None, T, DT, count=cnt, checkpoint=S, lead=y_lead, lead_length=lead_len, every=every,
                                 probes=list(range(V)) if probe_list is None else probe_list)
        ((pub[0] * g_pT).sum() + (pub[1] * g_vT).sum() + (pub[2] * g_samples).sum()).backward()
        assert same_bits(n(pub[2]), host["samples"]) and np.array_equal(n(y_lead.grad), host["g_lead"])
        assert np.array_equal(n(y[0].grad), host["g_p0"]) and np.array_equal(n(y[2].grad), n(g_params))
    # T = 0
    empty = torch.zeros(0, L, 2, device=cuda)
    ck0 = torch.empty(ops.micro_ckpt_numel(desc, 0, S), dtype=torch.float32, device=cuda)
    err = ops.new_error_record(cuda)
    pT, vT, samples = ops.micro_rollout_fwd_ckpt_lead(desc, 0, tp0, tv0, tpar, empty, ck0, None, 1, count=cnt, segment=S, err=err)
    g0 = ops.micro_rollout_bwd_ckpt_lead(desc, 0, ck0, tpar, empty, g_pT, g_vT, None, 1, samples, count=cnt, segment=S, err=err)
    j0 = ops.micro_rollout_fwd_jvp_lead(desc, 0, tp0, tv0, tpar, empty, t_p, t_v, None, 1, count=cnt, err=err)
    torch.cuda.synchronize()
    live = live_mask(L, V, count)
    assert err.tolist()[0] == 0 and tuple(samples.shape) == (0, L, 2, V) and tuple(g0[2].shape) == (0, L, 2)
    assert same_bits(n(pT), p0) and same_bits(n(vT), v0) and same_bits(n(j0[0][0]), p0)
    assert np.array_equal(n(g0[0]), n(g_pT) * live) and np.array_equal(n(g0[1]), n(g_vT) * live)
    assert np.array_equal(n(j0[1][0]), n(t_p) * live[None])


# =================================================================================================================
# 4. the fault records
# =================================================================================================================
def test_collision_record_of_a_leader_behind_the_head(cuda, capsys):
    """A leader that in step 2 stands within a metre of lane 1's head vehicle (gap = |dp| - half_len < 0): both forwards raise
    DHTS_FAULT_COLLISION (step 2, lane 1, the head vehicle), the result stays finite as on the existing path, and the operator prints it
    and goes on."""
    import torch
    import dhts
    from dhts import _lib, ops
    L, V, T, S = 4, 70, 5, 2
    rng = np.random.default_rng(2)
    p0, v0, par, _ = lanes(rng, L, V)
    count = [70, 9, 70, 70]
    lead = moving_leaders(rng, p0, count, V, T)
    lead[2, 1, 0] = p0[1, 8] + 2 * DT * v0[1, 8]          # where the head is in step 2, give or take its acceleration: well inside 5 m
    desc = ops.micro_desc(L, V, DT)
    tp0, tv0, tpar, tlead = t32(p0, cuda), t32(v0, cuda), t64(par, cuda), t32(lead, cuda)
    cnt = torch.tensor(count, device=cuda, dtype=torch.int32)
    errs = [ops.new_error_record(cuda) for _ in range(2)]
    ckpt = torch.empty(ops.micro_ckpt_numel(desc, T, S), dtype=torch.float32, device=cuda)
    a = ops.micro_rollout_fwd_ckpt_lead(desc, T, tp0, tv0, tpar, tlead, ckpt, None, 1, count=cnt, segment=S, err=errs[0])
    b = ops.micro_rollout_fwd_jvp_lead(desc, T, tp0, tv0, tpar, tlead, tp0[None], tv0[None], None, 1, count=cnt, err=errs[1])
    assert [e.tolist() for e in errs] == [[_lib.FAULT_COLLISION, 2, 1, 8]] * 2
    live = live_mask(L, V, count)
    for t in (a[0], a[1], a[2], b[0][0], b[0][1], b[1][0], b[1][1], b[1][2]):
        assert bool(torch.all(torch.isfinite(t)))
    assert same_bits(n(a[0]), n(b[0][0])) and same_bits(n(a[1]), n(b[0][1]))
    assert n(a[2])[2, 1, 1, 8] < 0.01 * v0[1, 8], "the head braked to a stop in step 2 (the acceleration clip), as a follower that collides does"
    assert np.all(n(a[1])[live & (np.arange(V)[None, :] != 8)] > 0)
    capsys.readouterr()
    out = dhts.micro_rollout(tp0, tv0, tpar, None, T, DT, count=cnt, checkpoint=S, lead=tlead, probes=[0, 8], every=2)      # prints, does not raise
    assert "Collision detected between vehicles (step 2, lane 1, vehicle 8)" in capsys.readouterr().out
    assert tuple(out[2].shape) == (2, L, 2, 2)


def test_non_finite_cotangent_record_with_a_recorded_leader(cuda):
    """test_micro_samples_gpu's construction -- an inf in the row of g_samples that every = 5 gives step 9, at probe column 2 = vehicle 7
    of lane 1, S = 4 --: ops.micro_bwd_fault() gives (9, 1, 7) with a recorded leader as the sampled sweep with a constant head gap
    does, state-only and with the parameter gradient."""
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
    lead = moving_leaders(rng, p0, count, V, T)
    g_pT, g_vT = rng.standard_normal((2, L, V)).astype(np.float32)
    g_samples = rng.standard_normal((T // every, L, 2, len(probes))).astype(np.float32)
    g_samples[(step + 1) // every - 1, lane, 1, probes.index(veh)] = np.inf
    cnt = torch.tensor(count, device=cuda, dtype=torch.int32)
    for want_params in (False, True):
        where = []
        for with_lead in (False, True):
            x = (t32(p0, cuda, True), t32(v0, cuda, True), t64(par, cuda, want_params))
            kw = dict(lead=t32(lead, cuda, True)) if with_lead else {}
            res = dhts.micro_rollout(*x, None if with_lead else t64(head, cuda), T, DT, count=cnt, checkpoint=S, probes=probes, every=every, **kw)
            torch.autograd.backward(list(res), [t32(g_pT, cuda), t32(g_vT, cuda), t32(g_samples, cuda)])
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                where.append(ops.micro_bwd_fault())
            assert any(issubclass(i.category, RuntimeWarning) for i in w)
            assert not np.all(np.isfinite(n(x[1].grad)[lane, veh])) and np.all(np.isfinite(n(x[1].grad)[0]))
        assert where[0] == (step, lane, veh) == where[1]


# =================================================================================================================
# 5. memory
# =================================================================================================================
def test_checkpointed_rollout_with_a_leader_allocates_no_history(cuda):
    """test_checkpointed_samples_allocate_no_history with a recorded leader: 64 lanes of 256 vehicles, 400 steps, checkpoint=4, four
    probes every 10 steps, params and lead requiring grad.  The peak of forward + backward above the resident inputs stays below half
    the bytes of a dense history (T L 2 V 4 = 52 MB); the same call observing every slot at every step exceeds the history's size."""
    import torch
    import dhts
    L, V, T = 64, 256, 400
    rng = np.random.default_rng(43)
    p0, v0, par, _ = lanes(rng, L, V)
    lead = moving_leaders(rng, p0, None, V, T)
    dense = T * L * 2 * V * 4
    peaks = []
    for sampled in (True, False):
        x = (t32(p0, cuda, True), t32(v0, cuda, True), t64(par, cuda, True))
        x_lead = t32(lead, cuda, True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        resident = torch.cuda.memory_allocated()
        kw = dict(probes=[10, 90, 170, 250], every=10) if sampled else dict(probes=list(range(V)), every=1)
        out = dhts.micro_rollout(*x, None, T, DT, check_faults=False, checkpoint=4, lead=x_lead, **kw)
        if sampled:
            assert tuple(out[2].shape) == (T // 10, L, 2, 4)
        (1e-4 * (out[0] ** 2).sum() + (out[1] ** 2).sum() + (out[2] ** 2).sum()).backward()
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - resident)
        assert all(bool(torch.all(torch.isfinite(t.grad))) for t in x + (x_lead,))
        del out, x, x_lead
    print("forward + backward with a leader, peak above the resident inputs: probes %d bytes, every slot and step %d bytes; a dense "
          "history %d bytes" % (peaks[0], peaks[1], dense))
    assert peaks[0] < dense // 2
    assert peaks[1] > dense


# =================================================================================================================
# 6. the example
# =================================================================================================================
@pytest.mark.parametrize("mode", (["--checkpoint"], ["--method", "lm", "--fused"]), ids=("adam_checkpoint", "lm_fused"))
@pytest.mark.parametrize("observe", ([], ["--observe", "2,5"]), ids=("dense", "observe"))
def test_calibration_example_follows_a_recorded_leader(cuda, tmp_path, mode, observe):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "calibrate_idm.py"), "--leader", "--seed", "1", "--n_lane", "3",
                          "--n_vehicle", "9", "--n_step", "40", "--n_episode", "5"] + mode + observe, cwd=str(tmp_path), env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    files = [os.path.join(dp, f) for dp, _, fs in os.walk(str(tmp_path)) for f in fs if f.startswith("trial_") and f.endswith(".txt")]
    assert len(files) == 1, "one trial_k.txt per run"
    losses = [float(line.split()[1]) for line in open(files[0]).read().splitlines()]
    print("calibrate_idm.py --leader %s: loss %s" % (" ".join(mode + observe), " ".join("%.6g" % x for x in losses)))
    assert len(losses) == 5 and all(np.isfinite(losses))
    assert losses[-1] < losses[0]
