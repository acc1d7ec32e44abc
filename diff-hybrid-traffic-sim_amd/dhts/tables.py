"""A network's host tables on the device, uploaded in ONE place and keyed by the C field names of include/dhts.h.

UploadedTables serves dhts.ops.DeviceNetTables, dhts.ops.DeviceHybridTables and dhts.stepwise.StepwiseNetwork: it owns the validation
(routes, per-replica topology, draws of source lanes), the padding (draws, empty CSR arrays) and the replica stride, and it fills
dhts_net_tables / dhts_hybrid_tables BY NAME from the binding's field lists, which tests/test_boundary.py pins to the header.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .network import group_routes

_FLOAT64 = ("lane_dx", "schedule", "lane_len", "draws", "veh_params")             # every other array is int32
_PER_REPLICA = ("left_src", "left_gate", "right_src", "schedule", "conv_next")    # [T][L] per table; the rest comes from table 0
_HOST_NAME = {"lane_len": "lane_length"}                                          # C field -> attribute of the host tables
NET_POINTERS = tuple(n for n, ty in _lib.NetTables._fields_ if ty is C.c_void_p)
HYBRID_POINTERS = tuple(n for n, ty in _lib.HybridTables._fields_ if ty is C.c_void_p)


class UploadedTables:
    """`tables`: one dhts.network.MacroNetworkTables / HybridNetworkTables (shared by all replicas) or a list of them (one per
    replica: same topology, own schedules / per-step routes / draws).  Hybrid tables come with `routes` [n_routes >= 1][stride <= 32]
    (int, -1 padded) and optionally `vehicle_params` [n_routes][6], rows as `routes`.  `overrides`: host arrays by C field name that
    replace table 0's (the stepwise path's group-major lane_off).

    .d                   the device tensors by C field name (lane_source / draws only with source lanes, veh_params only when given)
    .n_replica_tables    len(tables), or 0 for one shared table
    .replica_stride      dhts_net_tables::replica_stride: elements between the replicas' [T][L] tables (0 = shared)
    """

    def __init__(self, tables, device, routes=None, vehicle_params=None, overrides=None):
        many = isinstance(tables, (list, tuple))
        tabs = list(tables) if many else [tables]
        t = tabs[0]
        hybrid = hasattr(t, "lane_macro")
        fixed = ("lane_ncell", "lane_macro", "lane_source") if hybrid else ("lane_ncell",)
        for i, x in enumerate(tabs):
            if (x.n_lanes, x.n_cells, x.T) != (t.n_lanes, t.n_cells, t.T) or \
                    any(not np.array_equal(np.asarray(getattr(x, n)), np.asarray(getattr(t, n))) for n in fixed):
                raise ValueError("per-replica tables must share the topology of table 0 (lanes, cells, steps, lane kinds, source lanes): "
                                 "table %d differs" % i)
        self.device = device
        self.n_lanes, self.n_cells, self.T, self.n_edges = t.n_lanes, t.n_cells, t.T, t.n_edges
        self.n_replica_tables = len(tabs) if many else 0
        self.replica_stride = t.T * t.n_lanes if many else 0
        host = dict(overrides or {})
        for name in NET_POINTERS + (("lane_macro", "lane_len", "conv_next") if hybrid else ()):
            if name in _PER_REPLICA and many:
                host[name] = np.stack([getattr(x, name) for x in tabs])
            elif name not in host:
                host[name] = getattr(t, _HOST_NAME.get(name, name))
        if hybrid:
            self._hybrid(tabs, many, host, routes, vehicle_params)
        for name in ("nxt_idx", "prv_idx"):                   # (an empty CSR index array goes up as one zero: never pass a NULL pointer)
            host[name] = host[name] if len(host[name]) else np.zeros(1, dtype=np.int32)
        self.d = {name: self.upload(name, a) for name, a in host.items()}

    def _hybrid(self, tabs, many, host, routes, vehicle_params):
        t = tabs[0]
        routes = np.ascontiguousarray(routes, dtype=np.int32)
        if routes.ndim != 2 or routes.shape[0] < 1 or routes.shape[1] > 32:
            raise ValueError("routes must be [n_routes >= 1][stride <= 32]")
        if vehicle_params is not None:
            host["routes"], host["route_ptr"], host["veh_params"] = group_routes(routes, t.n_lanes, vehicle_params)
        else:
            host["routes"], host["route_ptr"] = group_routes(routes, t.n_lanes)
        self.n_routes, self.route_stride = (int(x) for x in host["routes"].shape)
        self.n_micro = int((np.asarray(t.lane_macro) == 0).sum())
        self.micro_tensor_ladder = bool(getattr(t, "micro_tensor_ladder", False))
        # micro source lanes (itscp `micro` mode): the lane flags and the host's admission draws (per replica when `tables` is a list)
        self.has_sources = bool(np.asarray(t.lane_source).any())
        self.n_draws, self.draws_stride = 0, 0
        if not self.has_sources:
            return
        for i, x in enumerate(tabs):
            if getattr(x, "draws", None) is None:
                raise ValueError("table %d has micro source lanes but no admission draws (HybridNetworkTables.set_micro_sources)" % i)
        if many:
            n = max(len(x.draws) for x in tabs)
            d = np.full((len(tabs), n), 2.0)                  # (a draw of 2.0 admits nobody)
            for i, x in enumerate(tabs):
                d[i, :len(x.draws)] = x.draws
            self.n_draws, self.draws_stride = n, n
        else:
            d = np.asarray(t.draws, dtype=np.float64)
            self.n_draws = len(d)
        host["lane_source"], host["draws"] = t.lane_source, d

    def upload(self, name, a):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64 if name in _FLOAT64 else torch.int32, device=self.device)

    def replace(self, name, a, in_place):
        """New per-episode data for d[name] (schedules, per-step routes, draws: same shape) -- the one rule for every user.
        in_place=True copies into the uploaded tensor: its address stays, so structs filled earlier and a captured HIP graph see the
        new data.  That is only sound where nothing still to run reads the OLD data; the fused kernels read these arrays in their
        forward launch alone.  in_place=False binds a NEW tensor: a stepwise rollout that has not run its reverse sweep yet keeps
        the tensors it was stepped with (several episodes summed before one backward(): Trainer.train_epoch with
        num_episode_per_epoch > 1), and its reverse sweep reads them again."""
        new = torch.as_tensor(np.ascontiguousarray(a), dtype=self.d[name].dtype)
        if new.shape != self.d[name].shape:
            raise ValueError("%s must keep the shape %s" % (name, tuple(self.d[name].shape)))
        if in_place:
            self.d[name].copy_(new)
        else:
            self.d[name] = new.to(self.device)

    def set_draws(self, draws, in_place):
        """A fresh stream of admission draws for the next episode (micro source lanes; same length as the uploaded one)."""
        if not self.has_sources:
            raise ValueError("the network has no micro source lanes")
        self.replace("draws", draws, in_place)

    def net_tables(self):
        d = self.d
        return _lib.NetTables(replica_stride=self.replica_stride, n_edges=self.n_edges, **{n: d[n].data_ptr() for n in NET_POINTERS})

    def hybrid_tables(self, net, **scalars):
        """dhts_hybrid_tables over `net` (net_tables(), or one built earlier while no tensor of it was rebound); `scalars`: the
        caller's records_per_step / loss_steps / lane_capacity / two_per_cu.  An array that was not uploaded stays NULL."""
        d = self.d
        return _lib.HybridTables(net=net, n_routes=self.n_routes, route_stride=self.route_stride, n_micro=self.n_micro,
                                 n_draws=self.n_draws, draws_stride=self.draws_stride, micro_tensor_ladder=int(self.micro_tensor_ladder),
                                 **{n: d[n].data_ptr() for n in HYBRID_POINTERS if n in d}, **scalars)
