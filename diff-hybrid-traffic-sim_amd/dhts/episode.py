"""Which device path an itscp episode takes, decided and run in one place for ItscpEnv.step (R = 1) and ReplicaBatch.rollout (R replicas):
episode_inputs (host arrays) -> plan_episode (a decision, nothing uploaded; next_rung after a sizing fault) -> Runner (the uploaded
tables and the one rollout); EpisodeState is what an ItscpEnv remembers of it, every field with its lifetime."""
import copy
import warnings
from collections import namedtuple

import numpy as np

from . import _lib, ops
from .network import HybridNetworkTables, MacroNetworkTables
from .stepwise import default_lane_capacity, persistent_form_pays

# path: "macro" / "hybrid" / "micro" = the fused kernels (one workgroup per replica), "stepwise" / "batched" = step by step on the device
# (dhts/stepwise.py, dhts/batched.py), "none" = lane by lane.  lane_capacity: vehicles a micro lane holds (0 = the default: 16 on the
# fused paths).  persistent, max_events: the stepwise path's form and hand-off event list (0 = sized from the network).  As a RUNG
# (plan_episode's argument, next_rung's result) only "stepwise" or not matters of `path`, and persistent = False rules that form out.
Plan = namedtuple("Plan", "path lane_capacity persistent max_events")
LANE_BY_LANE = Plan("none", 0, False, 0)
# (every rung the SAME episode; a network that starts on the stepwise path starts at default_lane_capacity and climbs from there)
LADDER = (("fused", 16), ("fused", 128), ("stepwise", 32), ("stepwise", 128), ("stepwise", 1024))
NO_ROUTES = np.asarray([[-1, -1]], dtype=np.int32)
EpisodeInputs = namedtuple("EpisodeInputs", "tables routes vehicle_params n_draws args")


def sim_args(env):
    """(n_inter_sq, frames_per_phase, dt, u_max, static_speed, vehicle_length) as every network entry point takes them."""
    return (env.num_intersection ** 2, env.config["signal_length"] * env.config["simulation_frequency"],
            1.0 / env.config["simulation_frequency"], env.simulator.speed_limit, env.config["static_speed"], env.simulator.vehicle_length)


def _vehicle_attributes(v, sim):
    """(accel_max, accel_pref, target_speed, min_space, time_pref, length) of a MicroVehicle; None = default_micro_vehicle(speed_limit)."""
    if v is None:
        from road.vehicle.micro_vehicle import MicroVehicle
        v = MicroVehicle.default_micro_vehicle(sim.speed_limit)
    return [float(v.accel_max), float(v.accel_pref), float(v.target_speed), float(v.min_space), float(v.time_pref), float(v.length)]


def _route_row(route):
    r = list(route.route)[:32]
    return r + [-1] * (32 - len(r))


def episode_inputs(envs, routes=None, vehicle_params=None):
    """The host-side inputs of an episode of one ItscpEnv (after reset()), or of a LIST of them that share the topology: `tables` is then a
    list, one per environment; routes and vehicle attributes are the first one's.  Host arrays: tools/probes/fuzz_env.py hands them to the CPU checker.
    routes: the spawn routes of a `hybrid` episode when they are known already ([n][<= 32], -1 padded); None draws 8 per spawn lane
    from create_random_route (np.random).  vehicle_params [routes][6] beside them, or None."""
    many = isinstance(envs, (list, tuple))
    e0 = envs[0] if many else envs
    mode, sim = e0.config["mode"], e0.simulator
    from_env = MacroNetworkTables.from_env if mode == "macro" else HybridNetworkTables.from_env
    tabs = [from_env(e) for e in (envs if many else [envs])]
    t0, n_draws = tabs[0], 0
    if mode == "macro":
        routes = NO_ROUTES
    elif mode == "micro":
        # every lane an IDM lane; source lanes admit their waiting vehicles against np.random draws (_simulator.py:153-174): the waiting
        # routes in admission order (the list is popped from its end) are the route rows; the draws are set per episode (set_draws)
        rows, vrows = [], []
        for l in range(t0.n_lanes):
            waiting = sim.lane_waiting_micro_vehicle.get(l, [])
            for k, r in enumerate(reversed(sim.lane_waiting_micro_route.get(l, []))):
                rows.append(_route_row(r))
                vrows.append(_vehicle_attributes(waiting[len(waiting) - 1 - k] if k < len(waiting) else None, sim))
        routes = np.asarray(rows, dtype=np.int32) if rows else NO_ROUTES
        # the waiting vehicles' own IDM attributes ride beside their routes (dhts_hybrid_tables::veh_params) unless every one of
        # them is the default vehicle the reference's reset() builds (_env.py:205-219)
        if any(v != _vehicle_attributes(None, sim) for v in vrows):
            vehicle_params = np.asarray(vrows, dtype=np.float64)
        n_draws = e0.num_timestep * max(1, int(t0.lane_source.sum()))
        for t in tabs:
            t.set_micro_sources(np.full(n_draws, 2.0))
    else:
        if routes is None:
            # hybrid: vehicle routes are pre-drawn per spawn lane (a micro lane fed by a macro lane) instead of at spawn time
            routes = [_route_row(sim.create_random_route(l)) for l in range(t0.n_lanes)
                      if t0.lane_macro[l] == 0 and any(t0.lane_macro[a] for a in t0.prev_lanes[l]) for _ in range(8)] or NO_ROUTES
        routes = np.asarray(routes, dtype=np.int32)
    return EpisodeInputs(tabs if many else t0, routes, vehicle_params, n_draws, sim_args(e0))


def plan_episode(tables, mode, config, vehicle_length, rung=None):
    """The device path of an episode from the tables' sizes (one table, or the first of a list), the itscp mode, the configuration
    (`fused`, `macro_path`, `stepwise_persistent`, `stepwise_lane_capacity`) and the rung the ladder has reached (None = the first)."""
    t = tables[0] if isinstance(tables, (list, tuple)) else tables
    rung = rung or Plan("fused", 0, True, 0)
    if not config.get("fused", True) or mode not in ("macro", "hybrid", "micro"):
        return LANE_BY_LANE
    if mode == "macro":
        if t.n_cells + t.n_lanes <= 1024:                   # one item per thread of one workgroup
            return Plan("macro", 0, True, 0)
        # beyond: the stepwise path (360 lanes: 6.9 ms per 120-step differentiable episode) unless round 4's batched one (11.4 ms) is asked for
        if config.get("macro_path", "stepwise") != "stepwise":
            return Plan("batched", 0, True, 0)
        lane_capacity = 32
    else:
        try:
            t.check_kernel_limits()                         # cells + lanes <= 960, <= 64 IDM lanes, <= 16 spawning lanes
            fits = True
        except ValueError:
            fits = False
        if fits and rung.path != "stepwise" and rung.lane_capacity in (0, 16, 32, 64, 128):
            return Plan(mode, rung.lane_capacity, rung.persistent, rung.max_events)      # (the last two: for the stepwise rungs above)
        lane_capacity = rung.lane_capacity or int(config.get("stepwise_lane_capacity", 0)) or default_lane_capacity(t, vehicle_length)
    # the persistent form (one kernel per direction) where it pays, unless the configuration or an earlier refusal says otherwise
    persistent = bool(rung.persistent) and bool(config.get("stepwise_persistent", persistent_form_pays(t)))
    return Plan("stepwise", lane_capacity, persistent, rung.max_events)


def next_rung(plan, error, event_bound=0, max_lane_capacity=1024):
    """The plan to run the same episode with after `plan` failed with `error`; LANE_BY_LANE past the last rung; None when the error is no
    sizing matter (a failed launch, a bad argument, any library error of the macro paths): a bug or a broken device, the caller's to raise."""
    sized = plan.path in ("hybrid", "micro", "stepwise")
    if isinstance(error, _lib.DhtsError):
        # two DHTS_E_INVALID sizing refusals have another way to run: the persistent form of a network whose scratch does not fit a
        # workgroup's LDS (-> the stepwise form), and a fused launch whose LDS plan does not fit at this lane capacity (-> next rung)
        if error.status != _lib.E_INVALID or not sized:
            return None
        if plan.path == "stepwise":
            return plan._replace(persistent=False) if plan.persistent else None
    elif not isinstance(error, ops.CapacityError):
        return None
    elif plan.path == "stepwise" and error.index == -2 and max(plan.max_events, 0) < event_bound:
        return plan._replace(max_events=event_bound)        # the event list, not a lane: more slots per lane would not help
    here = (plan.path == "stepwise", plan.lane_capacity or 16)
    for path, cap in LADDER if sized else ():
        if (path == "stepwise", cap) > here and cap <= max_lane_capacity:
            return plan._replace(path=path if path == "stepwise" else plan.path, lane_capacity=cap)
    return LANE_BY_LANE


class Runner:
    """The uploaded tables of one plan.  `inputs.tables` a list: one replica per entry (R = its length); one table: R = 1."""

    def __init__(self, plan, inputs=EpisodeInputs(None, None, None, 0, None), device=None, kept=None, batched_graph=True):
        """kept: the stepwise / batched Runner of the environment's earlier episodes; its network is updated in place (a captured
        graph stays valid) when the topology, the plan, the routes and the vehicle attributes are unchanged."""
        self.plan, self.args, self.n_draws = plan, inputs.args, inputs.n_draws
        tabs, routes, vp = inputs.tables, inputs.routes, inputs.vehicle_params
        self.R = len(tabs) if isinstance(tabs, (list, tuple)) else 0          # 0: one network, un-batched tables
        one = tabs[0] if self.R == 1 else tabs                               # (the fused kernels share a single table)
        self.tab = self.key = None
        self.batched_graph, self.graph_failed = bool(batched_graph), False
        if plan.path == "macro":
            self.tab = ops.DeviceNetTables(one, device)
        elif plan.path in ("hybrid", "micro"):
            self.tab = ops.DeviceHybridTables(one, routes, device, lane_capacity=plan.lane_capacity, vehicle_params=vp)
        elif plan.path in ("stepwise", "batched"):
            self.key = (plan, routes.shape, routes.tobytes(), None if vp is None else np.asarray(vp, dtype=np.float64).tobytes())
            try:
                if self.R or kept is None or kept.key != self.key:
                    raise ValueError
                kept.tab.update(tabs)
                self.tab, self.graph_failed = kept.tab, kept.graph_failed
            except ValueError:
                if plan.path == "batched":
                    from .batched import BatchedMacroNetwork
                    self.tab = BatchedMacroNetwork(tabs, device)
                else:
                    from .stepwise import StepwiseNetwork
                    self.tab = StepwiseNetwork(tabs, routes, device, lane_capacity=plan.lane_capacity, persistent=plan.persistent,
                                               max_events=plan.max_events, vehicle_params=vp)

    @property
    def event_bound(self):
        # the most a hand-off event list can need: every micro lane's head leaves (up to three deposit cells), every capacitor spawns, every step
        return self.tab.T * (4 * self.tab.n_micro + 2 * self.tab.n_caps) + 64 if self.plan.path == "stepwise" else 0

    def set_draws(self, draws):                             # draws [R][n_draws]: the admission draws of the next episode (`micro` mode)
        shared = self.R == 0 or (self.R == 1 and self.plan.path != "stepwise")
        self.tab.set_draws(draws[0] if shared else draws)

    def rollout(self, actions, differentiable=True):
        """actions [R][A] (device) -> (reward [R], queue [R][T][L], counts [R][4] or None).  differentiable=False: an evaluation episode."""
        path, tab, args = self.plan.path, self.tab, self.args
        if path == "batched":
            graph = self.batched_graph and not self.graph_failed    # the whole episode as one HIP graph (captured at the first call)
            try:
                reward, queue = (tab.graphed_rollout if graph else tab.rollout)(actions[0], *args, differentiable=differentiable)
            except RuntimeError as e:
                if not graph or isinstance(e, ops.CapacityError) or "capture" not in str(e).lower():
                    raise
                warnings.warn("ItscpEnv: HIP-graph capture of the batched episode failed (%s); running it eagerly" % e)
                self.graph_failed = True
                reward, queue = tab.rollout(actions[0], *args, differentiable=differentiable)
            return reward.reshape(1), queue.unsqueeze(0), None
        if path == "stepwise":
            cut, _, queue, counts = tab.rollout(actions if self.R else actions[0], *args, differentiable=differentiable)
            return (cut, queue, counts) if self.R else (cut.reshape(1), queue.unsqueeze(0), counts.unsqueeze(0))
        if path == "macro":
            reward, queue = ops.net_macro_rollout(actions, tab, *args) if differentiable else ops.net_macro_eval(actions, tab, *args)
            return reward, queue, None
        if differentiable:
            reward, _, queue, counts = ops.net_hybrid_rollout(actions, tab, *args)
        else:
            reward, queue, counts = ops.net_hybrid_eval(actions, tab, *args)
        return reward, queue, counts


class EpisodeState:
    """What an ItscpEnv remembers about its device path (env.device_path)."""

    def __init__(self):
        # ---- one episode: rewind() and reset() clear it
        self.done = False               # a device episode ran: the lane objects are still at their reset state
        # ---- the last episode that ran: overwritten by the next one, never cleared
        self.last_path = None           # "fused" / "stepwise" / "batched" / "lane-by-lane" (env.last_path)
        self.counts = None              # [4] vehicle counts of the last hybrid / micro / stepwise episode (env.fused_counts)
        # ---- until reset(): it depends on the schedules and routes reset() draws
        self.runner = None              # Runner of the plan in use
        # ---- the environment's life
        self.rung = None                # Plan the next plan_episode starts from: pin(), or where the ladder has climbed to
        self.routes_drawn = None        # hybrid spawn routes drawn by episode_inputs (drawn once, also across reset())
        self.kept = None                # the last stepwise / batched Runner: its network is updated in place after reset()
        self.overflowed = False         # an episode outgrew the last rung and ran lane by lane (env.fused_overflowed)
        self.overflow_warned = False    # ... and the warning was given

    def pin(self, path="fused", lane_capacity=0, max_events=0, persistent=True):
        """Start the ladder at a rung of the caller's choice ("fused" / "stepwise"), for the environment's life; it climbs on from there."""
        self.rung, self.runner = Plan(path, int(lane_capacity), bool(persistent), int(max_events)), None

    def new_episode(self, reset=False):
        self.done, self.runner = False, None if reset else self.runner

    def __deepcopy__(self, memo):
        twin = copy.copy(self)          # uploaded tables are shared -- but a kept network is updated in place: the copy builds its own
        twin.kept = None
        return twin
