"""ItscpEnv on the reference's import path (example.control.itscp._env; reference _env.py:24-962) without the
highway-env / gym / pygame dependencies: grid-of-intersections topology, inflow schedules, differentiable signal phases,
per-step queue-length loss.  Rendering is out of scope.

Topology (reference _env.py:221-439): every intersection (row, col) has, per side (south / west / north / east) and per
lane index, one approaching and one leaving lane of `lane_length`; inside the intersection each approaching lane gets a
straight connector to the opposite leaving lane and (right-most lane only) a right-turn connector; left turns are disabled.
Neighbouring intersections are joined leaving -> approaching.  Lane geometry is only used for lane LENGTHS; it is
reproduced with the same floating-point construction so that ceil(length / cell_length) gives the same cell counts.
"""
import copy
import itertools
import warnings

import numpy as np
import torch as th

from dhts import _lib, episode, ops
from dmath.operation import sigmoid
from example.common.rms import RunningMean
from example.control.itscp._env_config import default_config
from example.control.itscp._simulator import ItscpRoadNetwork as SimRoadNetwork
from road.lane.dmacro_lane import MacroLane, dMacroLane
from road.lane.dmicro_lane import MicroLane, dMicroLane

LANE_WIDTH = 4          # highway-env AbstractLane.DEFAULT_WIDTH


class LaneID:
    """(row, col) of the intersection, side `loc` ('south' / 'west' / 'north' / 'east' / 'mid'), for connectors the side
    they come from (`ploc`), direction and lane index (reference _env.py:24-60)."""

    def __init__(self, row, col, loc, ploc, approaching, lane_id):
        self.row, self.col, self.loc, self.ploc, self.approaching, self.lane_id = row, col, loc, ploc, approaching, lane_id

    def __str__(self):
        return "{}_{}_{}_{}_{}_{}".format(self.row, self.col, self.loc, self.ploc,
                                          "approaching" if self.approaching else "leaving", self.lane_id)

    def __eq__(self, o):
        return str(self) == str(o)

    def __hash__(self):
        return hash(str(self))


class _Segment:
    def __init__(self, start, end):
        self.start, self.end = np.array(start, dtype=float), np.array(end, dtype=float)
        self.length = float(np.linalg.norm(self.end - self.start))
        self.direction = (self.end - self.start) / self.length

    def position(self, s):
        return self.start + s * self.direction


class _Lane:
    def __init__(self, seg, sim_lane):
        self.env_lane, self.sim_lane = seg, sim_lane


def itscp_random_schedule(lane_id, num_timestep):
    """Five sessions of constant random inflow per lane (reference _env.py:62-92)."""
    per = num_timestep // 5
    schedule = {}
    for id in lane_id:
        cur = []
        for _ in range(5):
            r = np.random.random((1)).item()
            cur.extend([r] * per)
            cur = cur[:num_timestep]
        schedule[id] = cur
    return schedule


SIDE_OF_CORNER = (("south", "east"), ("west", "south"), ("north", "west"), ("east", "north"))   # (approaching, leaving)
STRAIGHT = {"north": "south", "west": "east", "east": "west", "south": "north"}
RIGHT = {"north": "west", "west": "south", "east": "north", "south": "east"}


class Box:
    """The three attributes of gym.spaces.Box the trainer reads (reference _env.py:170-173, trainer.py:26-36,182-187)."""

    def __init__(self, low, high, shape=None, dtype=np.float32):
        self.shape = tuple(shape) if shape is not None else np.shape(low)
        self.low = np.broadcast_to(np.asarray(low, dtype=dtype), self.shape).copy()
        self.high = np.broadcast_to(np.asarray(high, dtype=dtype), self.shape).copy()
        self.dtype = np.dtype(dtype)


class ItscpEnv:

    def __init__(self, schedule_callback=itscp_random_schedule):
        self.schedule_callback = schedule_callback
        self.config = dict(default_config)
        self.simulator = None
        self.lane = {}
        self.schedule = {}
        self.macro_route_schedule = []
        self.queue_length = {}
        self.flux = {}
        self.avg_speed = []
        self.is_static_rms = RunningMean(100_000)
        self.render_eval = False
        self.route_provider = None          # optional callable(lane_id) -> MicroRoute replacing create_random_route
        self.time = self.steps = 0
        # given by the caller instead of drawn: `hybrid` spawn routes [n][<= 32], their vehicles' attributes [n][6], `micro` admission draws
        self.fused_routes = self.fused_vehicle_params = self.fused_draws = None
        self.device_path = episode.EpisodeState()       # which device path the episodes take, and its uploaded tables

    fused_counts = property(lambda self: self.device_path.counts)
    fused_overflowed = property(lambda self: self.device_path.overflowed)
    last_path = property(lambda self: self.device_path.last_path)
    _fused_done = property(lambda self: self.device_path.done)      # (the flag's name before dhts/episode.py: tests and tools read it)

    def action_size(self):
        length = self.config["policy_length"] * self.config["duration"]
        return int(length / self.config["signal_length"]) * (self.num_intersection ** 2)

    def reset(self):
        if self.config["random_seed"] > 0:
            np.random.seed(self.config["random_seed"])
        self.num_intersection = self.config["num_intersection"]
        self.num_lane = self.config["num_lane"]
        self.num_timestep = self.config["policy_length"] * self.config["duration"] * self.config["simulation_frequency"]
        self._make_road()
        self.schedule = self.schedule_callback(list(self.lane.keys()), self.num_timestep)
        self.observation_space = Box(0, 1, shape=(self.config["num_schedule_obs"] * len(self.lane),))
        self.action_space = Box(self.config["action_min"], self.config["action_max"], shape=(self.action_size(),))
        self.time = self.steps = 0
        self.reward_queue_c = -1.0
        self.macro_route_schedule = [self.simulator.create_random_macro_route() for _ in range(self.num_timestep)]
        self._make_micro_route()
        self.device_path.new_episode(reset=True)        # (the uploaded tables depend on the schedules / routes drawn above)
        return self.observe()

    def rewind(self):
        """Episode state back to what reset() left, keeping the drawn schedules, routes and the uploaded kernel tables.
        Valid after fused episodes only (they never touch the lane objects); the reference deep-copies the environment
        per episode instead (trainer.py:172)."""
        if self.steps and not self.device_path.done:
            raise RuntimeError("rewind() after a lane-by-lane episode: the lane objects moved, call reset()")
        self.time = self.steps = 0
        self.device_path.new_episode()
        self.queue_length.clear()
        self.flux.clear()
        self.is_static_rms = RunningMean(100_000)

    def episode_copy(self):
        """A twin for ONE episode that must not disturb this environment (Trainer.evaluate; the reference deep-copies the
        environment, trainer.py:172): the episode state is its own, everything else is shared -- a fused episode never touches
        the lane objects.  Should the episode have to run lane by lane after all, the twin takes its own copy of the lanes first
        (step -> _own_lanes)."""
        twin = object.__new__(type(self))
        twin.__dict__.update(self.__dict__)
        twin.queue_length, twin.flux = {}, {}
        twin.config = dict(self.config)
        twin.is_static_rms = RunningMean(100_000)
        twin.device_path = copy.copy(self.device_path)         # (own fields, the same uploaded tables)
        twin._lanes_shared = True
        return twin

    def _own_lanes(self):
        if getattr(self, "_lanes_shared", False):
            memo = {}
            self.simulator = copy.deepcopy(self.simulator, memo)
            self.lane = copy.deepcopy(self.lane, memo)
            self._lanes_shared = False

    def __deepcopy__(self, memo):
        """Episode copy for the lane-by-lane path: everything is copied except the uploaded tables of the device paths
        (EpisodeState.__deepcopy__)."""
        twin = object.__new__(type(self))
        memo[id(self)] = twin
        # what an episode only reads is shared, not copied: the drawn inflow schedules (lanes x steps numpy scalars -- 86 000 objects
        # at config 4, 0.4 s per copy) and the per-step macro routes
        for k, v in self.__dict__.items():
            twin.__dict__[k] = v if k in ("schedule", "macro_route_schedule") else copy.deepcopy(v, memo)
        return twin

    def _make_micro_route(self):
        sim = self.simulator
        sim.lane_waiting_micro_vehicle.clear()
        sim.lane_waiting_micro_route.clear()
        for lid in sim.lane.keys():
            pairs = [sim.create_default_vehicle_with_random_route(lid) for _ in range(self.config["max_num_micro_vehicle_per_lane"])]
            sim.lane_waiting_micro_vehicle[lid] = [p[0] for p in pairs]
            sim.lane_waiting_micro_route[lid] = [p[1] for p in pairs]

    # ---- topology --------------------------------------------------------------------------------------------------
    def _make_road(self):
        n_int, n_lane = self.config["num_intersection"], self.config["num_lane"]
        outer = (LANE_WIDTH + 10) + LANE_WIDTH * (n_lane - 3 + 0.5)
        access = self.config["lane_length"]
        self.simulator = SimRoadNetwork(self.config["speed_limit"])
        if self.route_provider is not None:
            self.simulator.create_random_route = self.route_provider
        self.lane.clear()
        for row in range(n_int):
            for col in range(n_int):
                center = np.array([col * (outer + access), row * (outer + access)]) * 2.0
                approaching_ids = []
                for corner in range(4):
                    ang = np.radians(90 * corner)
                    rot = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
                    for approaching in (True, False):
                        loc = SIDE_OF_CORNER[corner][0 if approaching else 1]
                        for k in range(n_lane):
                            lid = LaneID(row, col, loc, None, approaching, k)
                            a = np.array([LANE_WIDTH * (k + 0.5), access + outer])
                            b = np.array([LANE_WIDTH * (k + 0.5), outer])
                            if not approaching:
                                a, b = np.flip(a, axis=0), np.flip(b, axis=0)
                            self._make_lane(lid, center + rot @ a, center + rot @ b)
                            if approaching:
                                approaching_ids.append(lid)
                idx = 0
                for lid in approaching_ids:
                    seg = self.lane[lid].env_lane
                    for turn in ("straight", "right"):
                        if turn == "right" and lid.lane_id != n_lane - 1:
                            continue
                        n_loc = (RIGHT if turn == "right" else STRAIGHT)[lid.loc]
                        nid = LaneID(row, col, n_loc, None, False, lid.lane_id)
                        nseg = self.lane[nid].env_lane
                        mid = LaneID(row, col, "mid", lid.loc, True, idx)
                        idx += 1
                        self._make_lane(mid, seg.position(seg.length), nseg.position(nseg.length))
                        self._connect(lid, mid)
                        self._connect(mid, nid)
        for row in range(n_int):
            for col in range(n_int):
                for side, other, dr, dc in (("north", "south", -1, 0), ("west", "east", 0, -1)):
                    if (side == "north" and row == 0) or (side == "west" and col == 0):
                        continue
                    for approaching in (True, False):
                        for k in range(n_lane):
                            cur = LaneID(row, col, side, None, approaching, k)
                            con = LaneID(row + dr, col + dc, other, None, not approaching, k)
                            if approaching:
                                self._connect(con, cur)
                            else:
                                self._connect(cur, con)

    def _make_lane(self, lid, start, end):
        seg = _Segment(start, end)
        n_int, sl, dx, mode = self.config["num_intersection"], self.config["speed_limit"], self.config["cell_length"], self.config["mode"]
        sid = len(self.simulator.lane)
        if mode == "macro":
            sim_lane = dMacroLane(sid, seg.length, sl, dx)
        elif mode == "micro":
            sim_lane = MicroLane(sid, seg.length, sl)
        else:       # hybrid: intersections on the border of the grid are macro, interior ones micro
            border = lid.row in (0, n_int - 1) or lid.col in (0, n_int - 1)
            sim_lane = dMacroLane(sid, seg.length, sl, dx) if border else dMicroLane(sid, seg.length, sl)
        self.simulator.add_lane(sim_lane)
        self.lane[lid] = _Lane(seg, sim_lane)

    def _connect(self, a, b):
        self.simulator.connect_lane(self.lane[a].sim_lane.id, self.lane[b].sim_lane.id)

    # ---- observation / step ------------------------------------------------------------------------------------------
    def observe(self):
        n_obs = self.config["num_schedule_obs"]
        obs = []
        for lid in self.lane.keys():
            sc = self.schedule[lid]
            t = len(sc) // n_obs
            for k in range(n_obs):
                if len(self.lane[lid].sim_lane.prev_lane) == 0:
                    t0, t1 = int(t * k), min(int(t * k + t), len(sc))
                    obs.append(sum(sc[t0:t1]) / (t1 - t0))
                else:
                    obs.append(0)
        return np.array(obs).astype(np.float32)

    def step(self, action, differentiable):
        self.steps += 1
        self.queue_length.clear()
        self.flux.clear()
        if self.device_path.done:
            raise NotImplementedError("the fused episode leaves the lane objects at their reset state: call reset() first, "
                                      "or set config['fused'] = False to step lane by lane")
        reward = self._step_fused(action, differentiable)
        if reward is None:
            self.device_path.last_path = "lane-by-lane"
            self._own_lanes()                       # (an episode_copy() twin: the lane-by-lane path moves the lane objects)
            self._simulate(action, differentiable)
            reward = self._reward(action)
        obs = self.observe()
        info = {"img": []}
        return obs, reward, self.steps >= self.config["duration"], info

    # ---- device episode: the whole differentiable rollout in two kernel launches (dhts_net_*_rollout_fwd / _bwd) ---------
    def _step_fused(self, action, differentiable=True):
        """First step after reset() in `macro` / `hybrid` / `micro` mode with config["fused"] (default on): reward (differentiable
        w.r.t. `action`) and the per-step queue terms from the device paths (dhts/episode.py) instead of one operator call per
        lane and step.  differentiable=False (an evaluation episode, Trainer.evaluate): the same episode with the reference's
        hard thresholds (dhts_net_*_rollout_eval), one launch, nothing kept for a reverse sweep.  Same numbers as the operator path in `macro` mode; in `hybrid` mode vehicle routes are pre-drawn
        per spawn lane (`fused_routes`, or 8 per lane from create_random_route) instead of being drawn at spawn time.
        Returns None when the network or the call is outside what the kernels cover (the operator path runs then)."""
        if (not self.config.get("fused", True) or self.config["mode"] not in ("macro", "hybrid", "micro") or self.steps != 1 or self.time != 0
                or not (isinstance(action, th.Tensor) and action.is_cuda)
                or any(sl.is_micro() and sl.num_vehicle() for sl in self.simulator.lane.values())):
            return None
        st = self.device_path
        draws = None            # the admission draws of THIS episode (`micro` mode): every rung of the ladder sees the same ones
        while True:
            runner = st.runner or self._build_runner(action.device)
            if runner.plan.path == "none":
                return None
            if (n := runner.n_draws) and draws is None:
                draws = np.random.random(n) if self.fused_draws is None else np.concatenate([np.asarray(self.fused_draws, dtype=np.float64), np.full(n, 2.0)])[:n]
            if draws is not None:
                runner.set_draws(draws[None])
            try:
                reward, queue, counts = runner.rollout(action.reshape(1, -1), differentiable)
                break
            except (_lib.DhtsError, ops.CapacityError) as e:
                # more than this launch was sized for, or a sizing that does not fit a workgroup's LDS; the attempt touched nothing on the host
                rung = episode.next_rung(runner.plan, e, runner.event_bound, int(self.config.get("fused_max_lane_capacity", 1024)))
                if rung is None:
                    raise
                if rung == episode.LANE_BY_LANE:
                    return self._fall_back_lane_by_lane(draws, e)
                st.rung, st.runner = rung, None
        st.counts = st.counts if counts is None else counts[0].tolist()
        st.last_path = "fused" if runner.plan.path in ("macro", "hybrid", "micro") else runner.plan.path
        q = np.ascontiguousarray(queue[0].detach().cpu().numpy().T)      # [L][T]
        for i, lid in enumerate(self.lane.keys()):
            self.queue_length[lid] = q[i].tolist()              # (Python floats like the lane-by-lane path's, converted in C)
            self.flux.setdefault(lid, [])
        self.time = self.num_timestep
        st.done = True
        return (-self.reward_queue_c) * reward[0]

    def _build_runner(self, device):
        """Plan the episode from where the ladder stands and upload its tables; any ValueError on the way = lane by lane."""
        st = self.device_path
        try:
            routes = self.fused_routes if self.fused_routes is not None else st.routes_drawn
            inputs = episode.episode_inputs(self, routes, self.fused_vehicle_params)
            if routes is None and self.config["mode"] == "hybrid":
                st.routes_drawn = inputs.routes                         # (a capacity retry is the same episode: the same routes)
            config = dict(self.config, stepwise_lane_capacity=0)        # (a key of ReplicaBatch: the environment ignores it)
            plan = episode.plan_episode(inputs.tables, self.config["mode"], config, self.simulator.vehicle_length, st.rung)
            st.runner = episode.Runner(plan, inputs, device, st.kept, self.config.get("batched_graph", True))
        except ValueError:
            st.runner = episode.Runner(episode.LANE_BY_LANE)
        if st.runner.key is not None:
            st.kept = st.runner                                         # (a stepwise / batched network survives reset())
        return st.runner

    def _fall_back_lane_by_lane(self, draws, e):
        # The reference has no capacity limits (_micro_lane.py:53-113): past the last rung the episode runs lane by lane (minutes, not
        # milliseconds).  In `micro` mode the admission draws the kernels were given are replayed: the episode that was asked for.
        st = self.device_path
        if not st.overflow_warned:
            warnings.warn("ItscpEnv: the device paths' capacity was exceeded (%s); this episode runs lane by lane" % e)
        self._own_lanes()                       # (an episode_copy() twin: from here on the lane objects are written to)
        if draws is not None:       # (and np.random once they run out)
            self.simulator.random_draw = itertools.chain(np.asarray(draws, dtype=np.float64).tolist(),
                                                         iter(lambda: float(np.random.random()), None)).__next__
        st.overflowed = st.overflow_warned = True
        return None

    def _simulate(self, action, differentiable):
        self.time = 0
        for _ in range(self.num_timestep):
            self._simulate_step(action, differentiable)
        return []

    def _is_static(self, speed, differentiable):
        """sigmoid(k (static_speed - speed)), k = 16 / |running mean of all (static_speed - speed) seen so far|, one
        sample at a time in visiting order (reference _env.py:586-618); `speed` is a 1-D tensor of one lane."""
        s0 = self.config["static_speed"]
        if not differentiable:
            return (speed < s0).float()
        with th.no_grad():
            means = self.is_static_rms.prefix_means((s0 - speed).detach().cpu().numpy())
            k = th.as_tensor(16.0 / np.abs(means), dtype=th.float32, device=speed.device)
        return th.sigmoid(th.clamp((s0 - speed) * k, -16.0, 16.0))

    def _simulate_step(self, action, differentiable):
        frame = self.time
        sim = self.simulator
        for lid in self.lane.keys():
            sl = self.lane[lid].sim_lane
            sim.lane_incoming[sl.id] = self.schedule[lid][frame] if len(sl.prev_lane) == 0 else -1
            sim.lane_signal[sl.id] = self.lane_signal_info(lid, action, frame, differentiable)[1]
        sim.macro_route = self.macro_route_schedule[frame]
        dt = 1.0 / self.config["simulation_frequency"]
        sim.forward(dt, differentiable)
        self.time += 1
        for lid in self.lane.keys():
            sl = self.lane[lid].sim_lane
            q = 0
            if isinstance(sl, MacroLane):
                r, _, u = sl.get_state_vector()
                q = (self._is_static(u, differentiable) * (r * sl.cell_length / sim.vehicle_length)).sum()
            elif isinstance(sl, MicroLane):
                if sl.num_vehicle():
                    _, v = sl.get_state_vector()
                    q = self._is_static(v, differentiable).sum()
            else:
                raise ValueError()
            self.queue_length.setdefault(lid, []).append((q ** 2.0) * dt)
            self.flux.setdefault(lid, [])

    def _reward(self, action):
        reward = 0
        for lid in self.lane.keys():
            for x in self.queue_length[lid]:
                reward = reward + self.reward_queue_c * x
        return reward

    # ---- signals -----------------------------------------------------------------------------------------------------
    def lane_signal_info(self, lane_id, action, curr_frame, differentiable):
        """(prev_signal, next_signal) of a lane (reference _env.py:885-962): within each signal phase the action value a
        of the lane's intersection splits the phase: west-east green while progress < a, north-south green afterwards."""
        frames = self.config["simulation_frequency"] * self.config["signal_length"]
        sq = self.num_intersection ** 2
        phase = min(curr_frame // frames, len(action) // sq - 1)
        a = action[phase * sq + lane_id.row * self.num_intersection + lane_id.col]
        if not isinstance(a, th.Tensor):
            a = th.tensor(a)
        progress = min((curr_frame % frames) / frames, 1.0)

        def we():
            return sigmoid(a - progress, constant=32) if differentiable else float(a > progress)

        def ns():
            return sigmoid(progress - a, constant=32) if differentiable else float(progress > a)

        if lane_id.loc == "mid":
            return (we() if lane_id.ploc in ("west", "east") else ns()), 1.0
        if not lane_id.approaching:
            return 1.0, 1.0
        return 1.0, (we() if lane_id.loc in ("west", "east") else ns())
