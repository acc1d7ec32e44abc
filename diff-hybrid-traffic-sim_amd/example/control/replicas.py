"""R itscp environments of ONE topology as one batch (this build only; the reference trains on one environment per episode,
example/control/trainer.py:168-205).

The fused network kernels run one workgroup per replica (dhts_net_macro_rollout_* / dhts_net_hybrid_rollout_*; BASELINE configs
4-5: 256 replicas per GPU), and a launch sized for 256 replicas takes as long as one for a single replica -- a trainer that runs
ONE environment per episode leaves 255 of 256 compute units idle and pays its host time per episode.  `ReplicaBatch` holds R
environments that share the topology and differ in what reset() draws (inflow schedules, per-step macro routes, admission draws):
their tables go to the device once as per-replica tables (dhts.ops.DeviceNetTables / DeviceHybridTables take a list), and an
"episode" of the batch is [R][A] actions -> [R] rewards in two launches.  Networks the fused kernels cannot hold run as R workgroups
of the stepwise path's persistent kernels (dhts/stepwise.py: StepwiseNetwork over a list of tables), same interface; only what
neither holds falls back to one ItscpEnv.step per replica.
"""
import copy

import numpy as np
import torch as th


class ReplicaBatch:

    def __init__(self, env, n_replica, device, seed_stride=1, seed_offset=0):
        """env: an ItscpEnv after reset().  Replica 0 is `env` itself; replica r > 0 is a copy reset with random_seed =
        env's seed + seed_offset + r * seed_stride when the environment is seeded (> 0), else with whatever np.random yields next."""
        self.device = th.device(device)
        self.R = int(n_replica)
        base = int(env.config.get("random_seed", 0))
        self.envs = [env]
        for r in range(1, self.R):
            e = copy.deepcopy(env)                      # (reset() below drops the copy's share of env's uploaded tables)
            if base > 0:
                e.config["random_seed"] = base + seed_offset + r * seed_stride      # (the copy's own dict)
            e.reset()
            self.envs.append(e)
        if base > 0 and seed_offset:
            # replica 0 of another rank draws its own episode too -- with the caller's configuration left as it was (a second
            # batch built from the same environment must not see an accumulated offset)
            env.config["random_seed"] = base + seed_offset
            try:
                env.reset()
            finally:
                env.config["random_seed"] = base
        self.fused_draws = self.last_draws = self._obs = None      # fused_draws [R][n]: a recorded stream of admission draws to replay
        self.kind, self.runner = self._build()

    def _build(self):
        from dhts import episode
        e0 = self.envs[0]
        mode, sim = e0.config["mode"], e0.simulator
        try:
            # ONE route table for the batch (the kernels share it between replicas): replica 0's.  Every replica environment is given the
            # same routes / waiting lists, so that the per-environment path of a comparison -- or of the fall-back -- runs the episode
            # the batch runs; what differs is what the kernels take per replica: inflow schedules, per-step macro routes, admission draws.
            inputs = episode.episode_inputs(self.envs, routes=e0.fused_routes)
            for e in self.envs[1:] if mode == "micro" else ():
                e.simulator.lane_waiting_micro_route = copy.deepcopy(sim.lane_waiting_micro_route)
            for e in self.envs if mode == "hybrid" else ():
                e.fused_routes = inputs.routes
            inputs = inputs._replace(vehicle_params=None)       # the batch ignores the vehicles' own attributes (ItscpEnv carries them)
            # the batch has no ladder (no rung), ignores `fused` and `macro_path`, is always persistent -- and reads `stepwise_lane_capacity`
            config = dict(e0.config, fused=True, macro_path="stepwise", stepwise_persistent=True)
            plan = episode.plan_episode(inputs.tables, mode, config, sim.vehicle_length)
            return plan.path, episode.Runner(plan, inputs, self.device)
        except ValueError:
            return "per-env", None

    def observe(self):
        """[R][n_obs].  ItscpEnv.observe() is a function of the drawn inflow schedules alone (reference _env.py:541-558), i.e. constant
        until the next reset(): evaluated once per replica (144 lanes x 5 windows of Python per call otherwise: 0.5 ms per replica)."""
        if self._obs is None:
            self._obs = np.stack([e.observe() for e in self.envs])
        return self._obs

    def rollout(self, actions, differentiable=True):
        """actions [R][A] (device) -> rewards [R] (reward_queue_c applied like ItscpEnv._reward); differentiable w.r.t. actions."""
        c = -self.envs[0].reward_queue_c
        if self.kind == "per-env":
            out = []
            for r, e in enumerate(self.envs):
                e.rewind() if e.device_path.done else None
                _, reward, _, _ = e.step(actions[r], differentiable)
                out.append(reward.reshape(()) if isinstance(reward, th.Tensor) else th.as_tensor(float(reward), device=self.device))
            return th.stack(out)
        if self.runner.n_draws:
            # itscp `micro` mode: fresh admission draws for every episode and replica, as ItscpEnv._step_fused draws them per episode
            d = self.fused_draws
            self.last_draws = np.random.random((self.R, self.runner.n_draws)) if d is None else np.asarray(d, dtype=np.float64)
            self.runner.set_draws(self.last_draws)
        reward, _, _ = self.runner.rollout(actions, differentiable)
        return c * reward

    @property
    def path(self):
        return "per-env" if self.kind == "per-env" else ("stepwise x%d" % self.R if self.kind == "stepwise" else "fused x%d" % self.R)
