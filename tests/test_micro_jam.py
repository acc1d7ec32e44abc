"""Stop-and-go traffic for the IDM rollout: the cases of tests/micro_jam_cases.py meet the conditions the GPU tests of
tests/test_micro_jam_gpu.py rest on, and the yardstick those tests use -- autograd of the float64 restatement -- holds where the
clips fire: against the C oracle's analytic operator (states, g_p0, g_v0) and against its own forward mode (torch.func.jvp) by the
dot-product identity.  No GPU needed."""
import numpy as np
import pytest

import micro_jam_cases as M
import micro_jvp_ref as J
from util import TOL_GRAD, TOL_STATE, grad_report, rel_elem


# =================================================================================================================
# conditions on the inputs
# =================================================================================================================
@pytest.mark.parametrize("case", M.CLEAN, ids=M.CLEAN_IDS)
def test_a_clean_case_is_clean_and_jammed(case):
    """No collision and no raw gap below 1e-5; at least 30 acceleration-clip events on vehicles that are not the head; every decision
    margin at least 1e-4; V, T, L and the step size from the stated sets; an empty lane."""
    print(M.summary(case))
    c = M.census(case)
    L, V = case.p0.shape
    assert V in (5, 64, 65, 130) and case.T in (37, 150) and 3 <= L <= 5 and case.dt >= 0.1 and 0 in case.count
    assert not c["collided"].any() and not c["small_gap"].any()
    assert (c["clip_a"] & ~c["head"][None]).sum() >= 30
    assert c["margin_a"].min() >= M.MARGIN and c["margin_s"].min() >= M.MARGIN
    live = np.broadcast_to(M.live_mask(case)[None], c["stopped"].shape)
    assert np.array_equal(c["stopped"], c["clip_a"] & live), "a clipped vehicle stops at exactly 0, and no other vehicle stands"


def test_the_clean_cases_cover_the_regime():
    """Both clips occur; some vehicle stands at v == 0 for at least 10 consecutive steps and some vehicle moves again after a stop (in
    every kind of boundary: head gap, recorded leader, ring); in a case of V >= 65 clipped vehicles sit on both sides of a 64-slot
    boundary; every stated V and T occurs."""
    assert any(M.census(c)["clip_s"].any() for c in M.CLEAN) and all(M.census(c)["clip_a"].any() for c in M.CLEAN)
    for kind in ("head", "lead", "ring"):
        cases = [c for c in M.CLEAN if c.kind == kind]
        stand = [M.longest_standstill(c) for c in cases]
        print(kind, [(c.name,) + s for c, s in zip(cases, stand)])
        assert any(s[1] for s in stand), kind
    assert max(M.longest_standstill(c)[0] for c in M.CLEAN) >= 10
    assert any(M.census(c)["clip_s"].any() for c in M.RING), "a ring under the spacing clip"
    both = []
    for c in M.CLEAN:
        if c.p0.shape[1] >= 65:
            clipped = M.census(c)["clip_a"].any(0)
            both.append(bool((clipped[:, :64].any(1) & clipped[:, 64:].any(1)).any()))          # in ONE lane
    assert any(both)
    assert {c.p0.shape[1] for c in M.CLEAN} == {5, 64, 65, 130} and {c.T for c in M.CLEAN} == {37, 150}


@pytest.mark.parametrize("case", M.CLEAN, ids=M.CLEAN_IDS)
def test_the_yardstick_can_judge_a_tenth_of_its_own_error(case):
    """The restatement rounds the state's cotangents to float32 once per step (so does the device, in another order).  Against the same
    rollout with every cotangent carried in double, under the cotangents the GPU tests use: every plane of every lane -- g_p0, g_v0, the
    six parameter planes, each relative to its own maximum -- moves by at most TOL_GRAD / 10.  A case where a plane is a small
    difference of large sums fails this and cannot tell a wrong kernel from a rounded one at TOL_GRAD: another seed is drawn."""
    rows, same_forward = M.own_error(case)
    assert same_forward and len(rows) >= 16
    lane, name, worst = max(rows, key=lambda r: r[2])
    print("%s: the yardstick's own rounding, worst plane: lane %d %s %.2e" % (case.name, lane, name, worst))
    assert worst <= TOL_GRAD / 10


@pytest.mark.parametrize("case", M.CLEAN, ids=M.CLEAN_IDS)
def test_the_tangent_planes_held_against_the_loudest_lane_are_the_listed_ones(case):
    """LOUDEST_LANE_PLANES of tests/micro_jam_cases.py is exactly the set of non-zero tangent planes, over the four kinds of direction,
    that the yardstick's own float32 rounding of the tangents moves by more than TOL_GRAD / 10 of the lane's own maximum."""
    found = {(k, lane, name) for k in range(4) for (lane, name), how in M.tangent_criteria(case, k).items() if how == "loudest"}
    print("%s: %s" % (case.name, sorted(found)))
    assert found == M.LOUDEST_LANE_PLANES[case.name]


@pytest.mark.parametrize("case", M.COLLIDE, ids=M.COLLIDE_IDS)
def test_a_collision_case_collides(case):
    print(M.summary(case))
    c = M.census(case)
    vehicles = int(c["collided"].any(0).sum())
    assert c["collided"].sum() >= 100 and M.first_collision(case) is not None
    assert vehicles == (1 if "one" in case.name else 6)
    assert c["margin_a"].min() >= M.MARGIN and c["margin_s"].min() >= M.MARGIN


# =================================================================================================================
# the restatement against the oracle, under both clips
# =================================================================================================================
def oracle_lanes(oracle, case, cotangents):
    """The C oracle lane by lane (it takes one head gap per call and no count): the live vehicles of every non-empty lane.  Returns per
    lane (n, fwd, [bwd per cotangent])."""
    out = []
    for lane, n in enumerate(case.count):
        if n == 0:
            continue
        params = np.ascontiguousarray(case.params[:, lane, :n].T)[None]
        f = oracle.micro_rollout_fwd(case.p0[lane:lane + 1, :n], case.v0[lane:lane + 1, :n], params, case.T, case.dt,
                                     head_dp=case.boundary[lane, 0], head_dv=case.boundary[lane, 1], want_hist=True)
        b = [oracle.micro_rollout_bwd(f, g_pT=g_pT[lane:lane + 1, :n], g_vT=g_vT[lane:lane + 1, :n],
                                      gh_p=None if g_hist is None else np.ascontiguousarray(g_hist[:, lane:lane + 1, 0, :n]),
                                      gh_v=None if g_hist is None else np.ascontiguousarray(g_hist[:, lane:lane + 1, 1, :n]))
             for g_pT, g_vT, g_hist in cotangents]
        out.append((lane, n, f, b))
    return out


def cotangents_of(case, seed=0):
    """A final-state cotangent, and a random cotangent of the whole history."""
    rng = np.random.default_rng(1000 + seed)
    L, V = case.p0.shape
    g_pT, g_vT = rng.standard_normal((2, L, V)).astype(np.float32)
    g_hist = rng.standard_normal((case.T, L, 2, V)).astype(np.float32)
    zero = np.zeros((L, V), np.float32)
    return [(g_pT, g_vT, None), (zero, zero, g_hist)]


@pytest.mark.parametrize("case", M.HEAD, ids=[c.name for c in M.HEAD])
def test_restatement_against_the_oracle_under_both_clips(oracle, case):
    """Stop-wave and pull-away cases: the restatement's history within TOL_STATE of the oracle's, its autograd g_p0, g_v0 within
    TOL_GRAD of the oracle's analytic operator (dIDM's blocks under both clips), for a final-state cotangent and for a random history
    cotangent, lane by lane."""
    cots = cotangents_of(case)
    refs = [M.reference(case, *c) for c in cots]
    for lane, n, f, b in oracle_lanes(oracle, case, cots):
        e_s = max(rel_elem(refs[0]["hist"][:, lane, 0, :n], f["hist_p"][:, 0]), rel_elem(refs[0]["hist"][:, lane, 1, :n], f["hist_v"][:, 0]),
                  rel_elem(refs[0]["pT"][lane, :n], f["pT"][0]), rel_elem(refs[0]["vT"][lane, :n], f["vT"][0]))
        print("%s lane %d: restatement vs oracle states %.2e" % (case.name, lane, e_s))
        assert e_s <= TOL_STATE
        assert np.array_equal(refs[0]["hist"][:, lane, 1, :n] == 0, f["hist_v"][:, 0] == 0), "the same vehicle-steps stand"
        for which, r, g in zip(("final-state", "history"), refs, b):
            tag = "%s lane %d, %s cotangent" % (case.name, lane, which)
            assert np.abs(g["g_p0"]).max() > 0
            assert grad_report(tag + ": g_p0", r["g_p0"][lane, :n], g["g_p0"][0]) <= TOL_GRAD
            assert grad_report(tag + ": g_v0", r["g_v0"][lane, :n], g["g_v0"][0]) <= TOL_GRAD


@pytest.mark.parametrize("case", M.COLLIDE, ids=M.COLLIDE_IDS)
def test_restatement_states_against_the_oracle_where_vehicles_collide(oracle, case):
    """The collision family: only the states have a common definition (the oracle's blocks use the un-clamped gap, autograd the
    clamped forward)."""
    ref = M.reference(case)
    for lane, n, f, _ in oracle_lanes(oracle, case, []):
        e_s = max(rel_elem(ref["hist"][:, lane, 0, :n], f["hist_p"][:, 0]), rel_elem(ref["hist"][:, lane, 1, :n], f["hist_v"][:, 0]))
        print("%s lane %d: restatement vs oracle states %.2e" % (case.name, lane, e_s))
        assert e_s <= TOL_STATE


# =================================================================================================================
# forward mode against reverse mode of the same restatement
# =================================================================================================================
@pytest.mark.parametrize("case", M.CLEAN, ids=M.CLEAN_IDS)
def test_forward_mode_of_the_restatement_is_the_adjoint_of_its_reverse_mode(case):
    """<g, J t> = <J^T g, t> for torch.func.jvp and autograd of the same restatement, on jammed inputs, with random cotangents of pT,
    vT and the history: TOL_GRAD of the sum of the absolute terms (both sweeps round to float32 where the rollout stores its state).
    On the head-gap cases micro_jvp_ref.yardstick gives the same tangents."""
    live = M.live_mask(case)
    t_p0, t_v0, t_par, t_b = (None if t is None else t[0] for t in M.directions(case, 1))
    jt = M.reference_jvp(case, 0)
    if case.kind == "head":
        y = J.yardstick(case.p0, case.v0, case.params, case.boundary, case.T, case.dt, count=case.count, t_p0=t_p0, t_v0=t_v0,
                        t_params=t_par, t_head=t_b)
        assert all(np.array_equal(y[k], jt[k]) for k in ("t_pT", "t_vT", "t_hist"))
    g_pT, g_vT, g_hist = M.cotangents(case)
    r = M.reference(case, g_pT, g_vT, g_hist)
    lv = live.astype(np.float64)                     # (slots at or beyond count pass their tangents through: not part of J)
    a, b, scale = M.adjoint_gap((g_pT, g_vT, g_hist), (jt["t_pT"], jt["t_vT"], jt["t_hist"]),
                              (r["g_p0"] * lv, r["g_v0"] * lv, r["g_params"] * lv[None], r["g_boundary"]), (t_p0, t_v0, t_par, t_b))
    print("%s: <g, J t> %.9e  <J^T g, t> %.9e  |difference| / sum |terms| %.2e" % (case.name, a, b, abs(a - b) / scale))
    assert scale > 0 and abs(a - b) <= TOL_GRAD * scale
