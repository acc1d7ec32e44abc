"""The hand-built networks of tests/net_cases.py on the CPU: is every case what it was built to be, and is the oracle fit to judge the
device on it?  Per case: the launch plan the library answers (dhts_net_macro_plan) and the two device-side layout choices are the ones the
case names; oracle.net_macro runs it without a CFL fault and oracle.net_hybrid agrees on the all-macro hybrid tables; the gradient is not
trivial; the structural zeros are exact; and one float32 ulp of the action moves the oracle's own gradient by at most a tenth of the
tolerance the device is held to (tests/test_net_cases_gpu.py).  Run with -s for the per-case lines of profiles/net_layout_cases.log."""
import types

import numpy as np
import pytest

import net_cases as nc
from util import TOL_GRAD, TOL_STATE, grad_report, state_report


@pytest.mark.parametrize("name", nc.NAMES)
def test_case_reaches_the_layout_it_names(name):
    """The plan comes from the arguments the launches use (dhts_net_macro_plan); gb1 and sg_base are recomputed from the formulas of the
    kernels' comments (Case.layout) and compared with what the case was built for inside net_cases.case()."""
    from dhts import ops
    c = nc.case(name)
    shim = types.SimpleNamespace(n_lanes=c.L, n_cells=c.C, T=c.T, n_replica_tables=0)
    plan = ops.net_macro_plan(c.A, shim, c.sq, c.F, nc.DT, nc.U_MAX)
    print(c.describe())
    assert plan == c.plan
    lay = c.layout()
    assert lay["fwd"]["block"] == plan["fwd_block"] and lay["bwd"]["block"] == plan["bwd_block"]
    assert c.T <= 48 and c.L <= c.C and c.C + c.L <= 960 and c.A <= 960          # every device form accepts it


def test_plan_query_refuses_what_the_launches_refuse():
    from dhts import _lib, ops
    for L, C, A in ((100, 925, 4), (10, 5, 4), (10, 50, 1025)):          # more than 1024 cells + lanes, more lanes than cells, too many actions
        with pytest.raises(_lib.DhtsError) as e:
            ops.net_macro_plan(A, types.SimpleNamespace(n_lanes=L, n_cells=C, T=8, n_replica_tables=0), 1, 8, nc.DT, nc.U_MAX)
        assert e.value.status == _lib.E_INVALID


def test_the_table_of_layouts_is_covered():
    """Every launch-bounds instantiation the arithmetic can reach, both ghost layouts on both kernels, both signal-thread placements, the
    64 / 128 thread edge, a block sized by the action count, and a lane at the adjacency limit on both sides."""
    cases = [nc.case(n) for n in nc.NAMES]
    assert {(c.plan["loss_waves"], c.plan["fwd_bound"]) for c in cases} == {(True, 512), (True, 640), (True, 1024), (False, 640), (False, 1024)}
    assert {c.plan["bwd_bound"] for c in cases} == {512, 1024}
    for side in ("fwd", "bwd"):
        assert {c.layout()[side]["ghost_split"] for c in cases} == {True, False}
        assert any(c.layout()[side]["sg_base"] == 0 for c in cases) and any(c.layout()[side]["sg_base"] > 0 for c in cases)
    assert nc.case("edge_64").C + nc.case("edge_64").L == 64 and nc.case("edge_65").C + nc.case("edge_65").L == 65
    assert nc.case("ghost_split_fits").L == 64 and nc.case("ghost_fallback").L == 65
    w = nc.case("action_wide")
    assert w.A > w.C + w.L and w.plan["bwd_block"] == nc.pad64(w.A)
    assert nc.case("sq_65").sq == 65 and sorted(set(nc.case("sq_65").tab.inter[nc.case("sq_65").tab.sig_kind != 0])) == [0, 63, 64]
    f = nc.case("fan_4")
    assert f.max_in == 4 and f.max_out == 4 and f.n_red > 0 and (f.tab.right_src[0] == -1).any()
    assert (np.diff(f.tab.left_src[:, 4]) != 0).all()                 # the lane with four upstream lanes takes another one every step
    assert sorted(set(int(n) for n in nc.case("one_wave").tab.lane_ncell) & {1, 8, 9, 17}) == [1, 8, 9, 17]
    p = nc.case("phase_clamp")
    assert p.T == 5 * p.F and p.A == 2 * p.sq + 1


@pytest.mark.parametrize("name", nc.NAMES)
def test_oracle_runs_the_case_and_its_two_forms_agree(oracle, name):
    from dhts.network import group_routes
    c = nc.case(name)
    ref = nc.reference(name, oracle)
    routes, ptr = group_routes(c.routes, c.L)
    for an, a in c.actions.items():
        o, oe = ref[an]["train"], ref[an]["hard"]
        assert o["rc"] == 0 and oe["rc"] == 0, an
        h = oracle.net_hybrid(c.htab, routes, ptr, a, *c.args)
        assert h["rc"] == 0 and h["n_spawned"] == 0
        assert state_report("%s %s: oracle hybrid form vs macro form, queues" % (name, an), h["queue"], o["queue"]) <= TOL_STATE
        assert abs(h["reward"] - o["reward"]) <= 1e-5 * abs(o["reward"])
        assert grad_report("%s %s: oracle hybrid form vs macro form, d reward / d action" % (name, an), h["g_action"], o["g_action"]) <= TOL_GRAD
        he = oracle.net_hybrid(c.htab, routes, ptr, a, *c.args, hard=True)
        assert state_report("%s %s: oracle hybrid form vs macro form, evaluation queues" % (name, an), he["queue"], oe["queue"]) <= TOL_STATE


@pytest.mark.parametrize("name", nc.NAMES)
def test_gradient_is_not_trivial(oracle, name):
    """Two phase rows and two gating intersections (where the episode reaches two rows / the case has two such intersections) carry
    gradient under `plain`; signals sit inside and outside the sigmoid's open range (episodes of at least F steps); `edges` has steps
    with a == progress, where an evaluation episode shows neither light."""
    c = nc.case(name)
    ref = nc.reference(name, oracle)
    g = ref["plain"]["train"]["g_action"]
    G = np.abs(g[:c.rows() * c.sq]).reshape(c.rows(), c.sq)
    gating = sorted(set(int(q) for q, k in zip(c.tab.inter, c.tab.sig_kind) if k != 0))
    print("%s: rows with gradient %d of %d reached, intersections with gradient %d of %d gating" %
          (name, (G.max(axis=1) > 0).sum(), c.last_row_reached() + 1, (G.max(axis=0) > 0).sum(), len(gating)))
    for an, a in c.actions.items():
        inside, outside = c.sigmoid_range_counts(a)
        print("  %s: signals inside the sigmoid's open range %d, outside %d; a == progress %d" % (an, inside, outside, c.neither_light_steps(a)))
    assert nc.nontrivial_failures(name, oracle) == []


@pytest.mark.parametrize("name", nc.NAMES)
def test_structural_zeros_are_exact_in_the_oracle(oracle, name):
    c = nc.case(name)
    z = c.structural_zeros()
    for an in c.actions:
        g = nc.reference(name, oracle)[an]["train"]["g_action"]
        assert (g[z] == 0.0).all(), an
    if name == "phase_clamp":
        assert z[-1] and not z[:4].any()                       # the odd trailing entry; both rows are reached
        g = nc.reference(name, oracle)["plain"]["train"]["g_action"]
        assert np.abs(g[2:4]).max() > 0                         # steps past the last row accumulate there
    if name == "sq_65":
        assert z.sum() == 130 - 2 * 3
    if name == "action_wide":
        assert z.sum() == 130 - 6


def test_trailing_unused_actions_change_nothing_in_the_oracle(oracle):
    w, t = nc.reference("action_wide", oracle), nc.reference("action_wide_trim", oracle)
    n = nc.case("action_wide_trim").A
    for an in w:
        for k in ("train", "hard"):
            assert np.array_equal(w[an][k]["queue"], t[an][k]["queue"]) and w[an][k]["reward"] == t[an][k]["reward"]
        assert np.array_equal(w[an]["train"]["g_action"][:n], t[an]["train"]["g_action"]) and (w[an]["train"]["g_action"][n:] == 0).all()


@pytest.mark.parametrize("name", nc.NAMES)
def test_oracle_gradient_is_well_conditioned(oracle, name):
    """One float32 ulp on every action entry, up and down: the oracle's own gradient moves by at most 0.1 TOL_GRAD of its largest
    entry, and under `plain` at least 90 % of the rows with a gradient move by at most 0.1 TOL_GRAD of the row's own largest entry.  A
    condition on the INPUTS, settled here: a case that misses it gets another seed (net_cases.SEEDS)."""
    ref = nc.reference(name, oracle)
    for an, r in ref.items():
        nz = r["row_max"] > 0
        print("%s %s: ulp spread of the oracle's gradient %.2e of max |g| = %.3e; rows well conditioned %d of %d with a gradient (worst row %.2e)"
              % (name, an, r["spread"], np.abs(r["train"]["g_action"]).max(), r["well"].sum(), nz.sum(), r["row_spread"].max() if len(nz) else 0.0))
    assert nc.conditioning_failures(name, oracle) == []
