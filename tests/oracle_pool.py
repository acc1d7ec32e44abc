"""Whole oracle episodes of network batches in a small process pool (tests/test_bench_batches_gpu.py: thousands of episodes).

The workers start with `spawn` and import numpy and the C oracle only -- never torch -- so that none of them opens the GPU;
each runs one OpenMP thread.  Tables travel as plain dicts of numpy arrays: the shared part once per pool, the inflow
schedule with each episode.
"""
import multiprocessing as mp
import os
import types
from concurrent.futures import ProcessPoolExecutor

import numpy as np

# the attributes oracle.net_hybrid / oracle.net_macro read from a table (dhts.network.HybridNetworkTables / MacroNetworkTables)
TABLE_KEYS = ("T", "n_lanes", "n_cells", "lane_macro", "lane_length", "lane_ncell", "lane_off", "lane_dx", "sig_kind", "inter",
              "left_src", "left_gate", "right_src", "conv_next", "lane_source", "draws", "micro_tensor_ladder")

_SHARED = None


def plain_tables(tab):
    """The oracle's view of `tab` without its schedule: a dict that pickles without importing the package."""
    out = {}
    for k in TABLE_KEYS:
        v = getattr(tab, k, None)
        if v is not None:
            out[k] = v if np.isscalar(v) or isinstance(v, (bool, int, float)) else np.asarray(v)
    return out


def workers():
    """min(8, CPUs this process may run on)."""
    return max(1, min(8, len(os.sched_getaffinity(0))))


def _init(shared):
    global _SHARED
    os.environ["OMP_NUM_THREADS"] = "1"
    _SHARED = shared


def _episode(job):
    from oracle import oracle as O
    r, sched, action = job
    s = _SHARED
    tab = types.SimpleNamespace(**s["tables"], schedule=sched)
    if s["kind"] == "hybrid":
        o = O.net_hybrid(tab, s["routes"], s["route_ptr"], action, *s["args"])
        return r, dict(rc=o["rc"], reward=o["reward"], queue=o["queue"], g_action=o["g_action"], n_spawned=o["n_spawned"],
                       n_deposits=o["n_deposits"])
    o = O.net_macro(tab, action, *s["args"])
    return r, dict(rc=o["rc"], reward=o["reward"], queue=o["queue"], g_action=o["g_action"])


def episodes(kind, tables, args, jobs, routes=None, route_ptr=None):
    """Yield (replica, oracle result) for every job (replica, schedule [T][L], action [A]) in job order.  kind: "hybrid"
    (oracle.net_hybrid with the grouped `routes`, `route_ptr`) or "macro" (oracle.net_macro); args: (n_inter_sq,
    frames_per_phase, dt, u_max).  A worker that dies raises BrokenProcessPool here (no silent wait)."""
    assert kind in ("hybrid", "macro")
    shared = {"kind": kind, "tables": plain_tables(tables), "args": tuple(args), "routes": routes, "route_ptr": route_ptr}
    old = os.environ.get("OMP_NUM_THREADS")
    os.environ["OMP_NUM_THREADS"] = "1"          # (the workers start on the first job and inherit it before numpy or OpenMP read it)
    try:
        with ProcessPoolExecutor(workers(), mp_context=mp.get_context("spawn"), initializer=_init, initargs=(shared,)) as pool:
            for item in pool.map(_episode, jobs, chunksize=4):
                yield item
    finally:
        if old is None:
            os.environ.pop("OMP_NUM_THREADS", None)
        else:
            os.environ["OMP_NUM_THREADS"] = old
