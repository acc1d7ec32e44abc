"""dhts/episode.py without a GPU: the capacity ladder, the path chosen from a network's sizes, and the host-side inputs of an episode
(shapes, order, and how much of np.random they consume)."""
import os

import numpy as np
import pytest

from dhts import _lib, ops
from dhts.episode import LANE_BY_LANE, Plan, episode_inputs, next_rung, plan_episode, sim_args
from test_oracle_golden import itscp_hybrid_tables, itscp_micro_tables, itscp_tables

FULL = ops.CapacityError("a lane is full")
FULL.index = 7
EVENTS = ops.CapacityError("the event list is full")
EVENTS.index = -2


def _refusal(status):
    e = _lib.DhtsError("a library call failed")
    e.status = status
    return e


def _climb(plan, error=FULL, **kw):
    seen = []
    while True:
        plan = next_rung(plan, error, **kw)
        if plan == LANE_BY_LANE:
            return seen
        seen.append((plan.path, plan.lane_capacity))


@pytest.mark.parametrize("mode", ["hybrid", "micro"])
def test_ladder_order(mode):
    """fused 16 -> fused 128 -> stepwise 32 -> 128 -> 1024 -> lane by lane; `fused_max_lane_capacity` removes the rungs above it."""
    start = Plan(mode, 0, True, 0)
    assert _climb(start) == [(mode, 128), ("stepwise", 32), ("stepwise", 128), ("stepwise", 1024)]
    assert _climb(Plan(mode, 16, True, 0)) == _climb(start)                         # (0 = the kernels' default 16)
    assert _climb(start, max_lane_capacity=16) == []                                # the first fault goes straight to lane by lane
    # At 128 the fused kernels stop at 128 and the rung of 1 024 is gone.  The stepwise rungs of 32 and 128 stay: the rule is
    # `capacity <= fused_max_lane_capacity` for every rung, as before this module existed.
    assert _climb(start, max_lane_capacity=128) == [(mode, 128), ("stepwise", 32), ("stepwise", 128)]
    assert next_rung(start, FULL, max_lane_capacity=128) == Plan(mode, 128, True, 0)
    # a stepwise start below 32 (the geometry's 8, or a pinned 1) climbs to 32
    for cap in (8, 1):
        assert _climb(Plan("stepwise", cap, True, 0)) == [("stepwise", 32), ("stepwise", 128), ("stepwise", 1024)]
    # what a rung carries for the stepwise path survives the climb
    assert next_rung(Plan(mode, 128, False, 77), FULL) == Plan("stepwise", 32, False, 77)


def test_event_list_overflow_grows_the_list_once():
    T, n_micro, n_caps = 40, 12, 3
    bound = T * (4 * n_micro + 2 * n_caps) + 64
    plan = Plan("stepwise", 32, True, 4)
    grown = next_rung(plan, EVENTS, event_bound=bound)
    assert grown == Plan("stepwise", 32, True, bound)                               # same lane capacity: more slots would not help
    assert next_rung(Plan("stepwise", 32, True, 0), EVENTS, event_bound=bound) == grown
    assert next_rung(grown, EVENTS, event_bound=bound) == Plan("stepwise", 128, True, bound)      # the bound in place: a capacity fault
    assert next_rung(Plan("hybrid", 0, True, 0), EVENTS, event_bound=bound) == Plan("hybrid", 128, True, 0)


def test_library_refusals():
    invalid = _refusal(_lib.E_INVALID)
    assert next_rung(Plan("stepwise", 8, True, 5), invalid) == Plan("stepwise", 8, False, 5)         # the persistent form does not fit
    assert next_rung(Plan("stepwise", 8, False, 5), invalid) is None                                 # ... nothing left: the caller's
    assert next_rung(Plan("hybrid", 128, True, 0), invalid) == Plan("stepwise", 32, True, 0)         # a fused LDS plan does not fit
    assert next_rung(Plan("micro", 0, True, 0), invalid) == Plan("micro", 128, True, 0)
    for status in (_lib.E_LAUNCH, _lib.E_NO_DEVICE, None):
        for path in ("macro", "batched", "hybrid", "micro", "stepwise"):
            assert next_rung(Plan(path, 0, True, 0), _refusal(status)) is None
    for path in ("macro", "batched"):                       # no error of the macro paths becomes a rung
        assert next_rung(Plan(path, 0, True, 0), invalid) is None
        assert next_rung(Plan(path, 0, True, 0), FULL) == LANE_BY_LANE
    assert next_rung(Plan("hybrid", 0, True, 0), RuntimeError("anything else")) is None


def _golden(golden_dir, name):
    return np.load(os.path.join(golden_dir, "itscp_%s.npz" % name))


def test_path_from_sizes(golden_dir):
    from dhts.stepwise import default_lane_capacity, persistent_form_pays
    t, m = itscp_tables(_golden(golden_dir, "macro_small"))
    assert plan_episode(t, "macro", {}, m["vehicle_length"]).path == "macro"
    assert plan_episode(t, "macro", {"fused": False}, m["vehicle_length"]) == LANE_BY_LANE
    t, m = itscp_tables(_golden(golden_dir, "macro_3x3x3"))
    assert t.n_lanes == 360
    assert plan_episode(t, "macro", {}, m["vehicle_length"]) == Plan("stepwise", 32, persistent_form_pays(t), 0)
    assert plan_episode(t, "macro", {"macro_path": "batched"}, m["vehicle_length"]).path == "batched"
    assert plan_episode([t, t], "macro", {"stepwise_persistent": False}, m["vehicle_length"]) == Plan("stepwise", 32, False, 0)
    t, m = itscp_hybrid_tables(_golden(golden_dir, "hybrid_short"))
    assert plan_episode(t, "hybrid", {}, m["vehicle_length"]) == Plan("hybrid", 0, True, 0)
    assert plan_episode(t, "hybrid", {}, m["vehicle_length"], Plan("fused", 128, True, 0)).lane_capacity == 128
    assert plan_episode(t, "hybrid", {}, m["vehicle_length"], Plan("fused", 1, True, 0)).path == "stepwise"       # no fused kernel of 1
    pinned = plan_episode(t, "hybrid", {}, m["vehicle_length"], Plan("stepwise", 32, False, 4))
    assert pinned == Plan("stepwise", 32, False, 4)
    t, m = itscp_hybrid_tables(_golden(golden_dir, "hybrid_n2l30"))
    assert default_lane_capacity(t, m["vehicle_length"]) == 8
    assert plan_episode(t, "hybrid", {}, m["vehicle_length"]) == Plan("stepwise", 8, True, 0)
    assert plan_episode(t, "hybrid", {"stepwise_lane_capacity": 64}, m["vehicle_length"]).lane_capacity == 64
    t, m = itscp_hybrid_tables(_golden(golden_dir, "hybrid_5x5"))
    assert plan_episode(t, "hybrid", {}, m["vehicle_length"]).path == "stepwise"
    t, m, _ = itscp_micro_tables(_golden(golden_dir, "micro_2x2"))
    try:
        t.check_kernel_limits()
        want = "micro"
    except ValueError:
        want = "stepwise"
    assert plan_episode(t, "micro", {}, m["vehicle_length"]).path == want


def _env(mode, n, seed=11):
    from example.control.itscp._env import ItscpEnv
    from example.control.itscp import problem as problems
    env = ItscpEnv()
    env.schedule_callback = problems.problem_1
    env.config.update(num_intersection=n, num_lane=1, lane_length=5.0, policy_length=4, signal_length=2, mode=mode, speed_limit=60.0,
                      random_seed=seed)
    env.reset()
    return env


@pytest.mark.parametrize("mode,n", [(mode, n) for mode in ("macro", "hybrid", "micro") for n in (1, 2)] + [("hybrid", 3)])      # (3 x 3: the smallest
def test_episode_inputs(mode, n, monkeypatch):                  # hybrid grid with an interior intersection, i.e. with spawn routes to draw)
    import torch
    from dhts import device
    monkeypatch.setattr(device, "_device", torch.device("cpu"))      # lane objects in host memory: only their sizes are read here
    env, twin = _env(mode, n), _env(mode, n)
    np.random.seed(123)
    one = episode_inputs(env)
    after = np.random.get_state()
    tab, routes = one.tables, one.routes
    assert one.args == sim_args(env) and len(one.args) == 6
    assert routes.dtype == np.int32 and routes.ndim == 2 and 2 <= routes.shape[1] <= 32
    pad = np.cumsum(routes < 0, axis=1) > 0
    assert np.array_equal(pad, routes == -1)                                        # a route, then nothing but -1
    sim = twin.simulator
    # the same draws by hand on the twin: np.random ends where episode_inputs left it
    np.random.seed(123)
    if mode == "hybrid":
        spawn = [l for l in range(tab.n_lanes) if tab.lane_macro[l] == 0 and any(tab.lane_macro[a] for a in tab.prev_lanes[l])]
        drawn = [list(sim.create_random_route(l).route) for l in spawn for _ in range(8)]
        assert routes.shape == ((len(drawn), 32) if drawn else (1, 2))
        for row, r in zip(routes, drawn):
            assert list(row[:len(r[:32])]) == r[:32] and (row[len(r[:32]):] == -1).all()
        assert one.n_draws == 0 and one.vehicle_params is None
        # routes that are known already are taken as they are, and nothing is drawn
        state = np.random.get_state()
        again = episode_inputs(env, routes=routes)
        assert np.array_equal(again.routes, routes) and np.array_equal(np.random.get_state()[1], state[1])
    elif mode == "micro":
        want = [list(r.route) for l in range(tab.n_lanes) for r in reversed(sim.lane_waiting_micro_route.get(l, []))]
        assert routes.shape == (len(want), 32) and len(want) > 0
        for row, r in zip(routes, want):                                            # reversed waiting-list order, lane by lane
            assert list(row[:len(r)]) == r and (row[len(r):] == -1).all()
        assert one.n_draws == env.num_timestep * int(tab.lane_source.sum()) > 0 and tab.draws.shape == (one.n_draws,)
        assert one.vehicle_params is None                                           # every waiting vehicle is the default one
        lane = next(l for l, w in env.simulator.lane_waiting_micro_vehicle.items() if w)
        env.simulator.lane_waiting_micro_vehicle[lane][-1].time_pref += 0.25         # ... until one is not
        own = episode_inputs(env).vehicle_params
        first = sum(len(env.simulator.lane_waiting_micro_route.get(l, [])) for l in range(lane))
        assert own.shape == (len(want), 6) and len(np.unique(own, axis=0)) == 2
        assert np.flatnonzero((own != own[(first + 1) % len(want)]).any(axis=1)).tolist() == [first]     # the list's end is admitted first
        env.simulator.lane_waiting_micro_vehicle[lane][-1].time_pref -= 0.25
    else:
        assert routes.tolist() == [[-1, -1]] and one.n_draws == 0 and one.vehicle_params is None
    assert np.array_equal(np.random.get_state()[1], after[1]) and np.random.get_state()[2] == after[2]
    # one environment or a list of one: the same arrays
    np.random.seed(123)
    many = episode_inputs([env])
    assert isinstance(many.tables, list) and len(many.tables) == 1
    assert np.array_equal(many.routes, routes) and many.n_draws == one.n_draws and many.args == one.args
    for name in ("schedule", "lane_ncell", "left_src", "right_src", "sig_kind", "inter"):
        assert np.array_equal(getattr(many.tables[0], name), getattr(tab, name)), name
    if mode != "macro":
        assert np.array_equal(many.tables[0].conv_next, tab.conv_next) and np.array_equal(many.tables[0].lane_macro, tab.lane_macro)
