"""The batches bench.py times, replica by replica (lane by lane for config 3), against the CPU oracle.

bench.py's parity_check looks at replica 0 of a network batch (lanes 0 .. 15 of config 3); here every replica is held to
the oracle on its own schedule and action: the 2 048-replica hybrid batch of rank 0 (packed plan, replicas 256 .. 2047 on
constant-in-time schedules, tapes above 4 GiB), the 256-replica batches of ranks 1 .. 7, the macro and stepwise batches,
and lanes across the whole 4 096-lane micro launch.  The gradient is the RAW d loss / d action of the pass: nothing dropped.

Ulp rule (after tests/test_stepwise_gpu.py): these episodes are often ill-conditioned, so an entry outside its tolerance is
excused when the oracle cannot decide it -- when the oracle's own value, with the action nudged by +-1, 2, 4 and 8 ulps,
moves at least as far as the kernel-vs-oracle gap, or by more than a fifth of the tolerance (the stepwise test's stability
bound).  A replica whose whole episode (every entry, every count) is the oracle's at one of those nudged actions is
excused as a whole: the kernels took the neighbouring branch.  A single +1 ulp nudge is not enough: on the first MI355X
run seven gradient entries of rank 0's batch were 3 to 200 times the oracle's +1 ulp move, and 1 to 10 times short of its
move at +-2 .. 8 ulps.  At most MAX_EXCUSED_ENTRIES excused entries per replica and MAX_EXCUSED_REPLICAS replicas per
batch; the log lists every excused entry with the oracle's move.

The reward is compared in the reference's summation order (DHTS_OPT_REWARD_CHAIN on one more forward pass, as bench.py's
parity_check); the kernels' own order is 1.3e-5 from it at worst on rank 0's batch, and is printed.
"""
import time

import numpy as np
import pytest

from oracle_pool import episodes
from util import TOL_GRAD, TOL_STATE, rel_elem, rel_max

pytestmark = pytest.mark.gpu

TOL_REWARD = 1e-5
MAX_EXCUSED_ENTRIES = 2
# ... but for this replica, whose three excused gradient entries (7, 16, 17) each move 20 times their gap under the nudges
WIDER_EXCUSE = {("hybrid", 0, 2048): {289: 3}}
NUDGES = (1, -1, 2, -2, 4, -4, 8, -8)        # ulps
# replicas of a batch that may lean on the ulp rule: the MI355X runs needed 11 (rank 0 x 2048), at most 2 (ranks 1 .. 7 x 256)
# and 0 (macro, stepwise)
MAX_EXCUSED_REPLICAS = {"hybrid rank 0 x 2048": 12, "hybrid x 256": 3, "macro x 256": 1, "stepwise x 256": 1}
# replicas whose reverse sweep goes non-finite in the ORACLE (0 x inf on a head gap clamped to 0, dmacro_lane.py:308): the
# kernels must leave NaN / inf in exactly these rows, at exactly the oracle's entries (bench.py drops these rows)
NONFINITE = {("hybrid", 0, 2048): {442, 1945}, ("hybrid", 2, 256): {14}}
# ... except these entries of two of those rows, where the kernels' reverse sweep stays finite and the oracle's is NaN (stable
# under the nudges above; replica 442's rows agree entry for entry).  An open difference in how far NaN travels backwards,
# pinned here so that either side changing is seen.
NAN_ONLY_IN_ORACLE = {("hybrid", 0, 2048): {1945: {4, 13}}, ("hybrid", 2, 256): {14: {31, 39, 40}}}


def _field(o, what):
    """One replica's entries of `what` (queue, reward, g_action, n_spawned, n_deposits) as a flat float64 array."""
    return np.asarray(o[what], dtype=np.float64).ravel()


def _gaps(kern, ref):
    """(what, index, |kernel - oracle|, tolerance) of every entry of one replica outside its tolerance (a non-finite kernel value counts
    as outside); gradient entries the oracle has non-finite are compared by position elsewhere.  Also the replica's
    (queue, reward, gradient) relative gaps."""
    out, rel = [], {}
    for what in ("queue", "reward", "g_action", "n_spawned", "n_deposits"):
        if what not in ref:
            continue
        k, r = _field(kern, what), _field(ref, what)
        fin = np.isfinite(r)
        if what == "queue":
            tol = TOL_STATE * max(np.abs(r).max(), 1e-30)
        elif what == "reward":
            tol = TOL_REWARD * max(abs(r[0]), 1e-30)
        elif what == "g_action":
            tol = TOL_GRAD * max(np.abs(r[fin]).max() if fin.any() else 0.0, 1e-30)
        else:
            tol = 0.0
        d = np.where(fin, np.abs(k - np.where(fin, r, 0.0)), 0.0)
        if what in ("queue", "reward", "g_action"):
            rel[what] = float(np.max(d) / (tol / {"queue": TOL_STATE, "reward": TOL_REWARD, "g_action": TOL_GRAD}[what])) \
                if np.isfinite(d).all() else float("inf")
        for i in np.flatnonzero(~(d <= tol)):
            out.append((what, int(i), float(d[i]), tol))
    return out, rel


def _nudge(a, ulps):
    a = np.asarray(a, dtype=np.float32)
    for _ in range(abs(ulps)):
        a = np.nextafter(a, np.float32(1.0 if ulps > 0 else 0.0))
    return a


def check_batch(tag, kind, tables, args, scheds, actions, kern, replicas, routes=None, route_ptr=None, budget=None, nan_only_in_oracle=None,
                wider_excuse=None):
    """Every replica of `replicas` through the oracle (process pool) against the kernel's host arrays `kern`: reward [R],
    queue [R][T][L], g_action [R][A] (d reward / d action), n_spawned / n_deposits [R] (hybrid).  Returns (problems,
    oracle non-finite set, kernel non-finite set, excused {replica: [(what, index, gap, oracle move)]})."""
    t0 = time.time()
    budget = MAX_EXCUSED_REPLICAS[budget or tag]
    nan_only_in_oracle, wider_excuse = nan_only_in_oracle or {}, wider_excuse or {}
    problems, pending, worst = [], {}, {"queue": (0.0, -1), "reward": (0.0, -1), "g_action": (0.0, -1)}
    nonfin_ref, nonfin_kern = set(), set()
    jobs = ((r, scheds[r], actions[r]) for r in replicas)
    for r, ref in episodes(kind, tables, args, jobs, routes, route_ptr):
        if ref["rc"] != 0:
            problems.append("replica %d: the oracle's episode failed (rc %d)" % (r, ref["rc"]))
            continue
        k = {key: v[r] for key, v in kern.items()}
        bad_r, bad_k = ~np.isfinite(ref["g_action"]), ~np.isfinite(k["g_action"])
        if bad_r.any():
            nonfin_ref.add(r)
        if bad_k.any():
            nonfin_kern.add(r)
        expect_k = bad_r.copy()
        expect_k[sorted(nan_only_in_oracle.get(r, ()))] = False
        if not np.array_equal(expect_k, bad_k):
            problems.append("replica %d: non-finite gradient entries kernel %s, oracle %s"
                            % (r, np.flatnonzero(bad_k).tolist(), np.flatnonzero(bad_r).tolist()))
        gaps, rel = _gaps(k, ref)
        for what, e in rel.items():
            if e > worst[what][0]:
                worst[what] = (e, r)
        if gaps:
            pending[r] = (ref, gaps)
    excused = {}
    if pending:
        # the oracle's own spread at each missed entry under the nudges (only the replicas that missed run again)
        moves = {r: [0.0] * len(g) for r, (_, g) in pending.items()}
        neighbour = {}           # replica -> a nudge at which the kernel's episode is the oracle's within every tolerance
        jobs = (((r, u), scheds[r], _nudge(actions[r], u)) for r in sorted(pending) for u in NUDGES)
        for (r, u), nud in episodes(kind, tables, args, jobs, routes, route_ptr):
            ref, gaps = pending[r]
            for j, (what, i, _, _) in enumerate(gaps):
                m = abs(_field(nud, what)[i] - _field(ref, what)[i])
                moves[r][j] = max(moves[r][j], m if np.isfinite(m) else np.inf)
            if r not in neighbour and np.array_equal(np.isfinite(nud["g_action"]), np.isfinite(ref["g_action"])) \
                    and not _gaps({key: v[r] for key, v in kern.items()}, nud)[0]:
                neighbour[r] = u
        for r in sorted(pending):
            ref, gaps = pending[r]
            ex = [(w_, i, d, m) for (w_, i, d, tol), m in zip(gaps, moves[r])]
            stand = [e for e, (_, _, _, tol) in zip(ex, gaps) if not (e[3] >= e[2] or e[3] > 0.2 * tol)]
            if r in neighbour:
                print("%s: replica %d is the oracle's episode at %+d ulps within every tolerance (%d entries off at 0: %s)"
                      % (tag, r, neighbour[r], len(gaps), ", ".join("%s[%d] gap %.3g" % e[:3] for e in ex[:6])))
                excused[r] = ex
            elif stand:
                problems.append("replica %d: %d entries outside tolerance that the oracle decides (what, index, |kernel - oracle|, "
                                "oracle's move at +-1 .. 8 ulps): %s" % (r, len(stand), [(e[0], e[1], "%.3g" % e[2], "%.3g" % e[3])
                                                                                            for e in stand[:6]]))
            elif len(gaps) > wider_excuse.get(r, MAX_EXCUSED_ENTRIES):
                problems.append("replica %d: %d entries need the ulp excuse (at most %d): %s" % (
                    r, len(gaps), wider_excuse.get(r, MAX_EXCUSED_ENTRIES), ", ".join("%s[%d] gap %.3g, oracle moves %.3g" % e for e in ex[:6])))
            else:
                excused[r] = ex
    print("\n%s: %d replicas vs oracle in %.0f s; worst |d| / tol-scale (replica): queue %.2e (%d), reward %.2e (%d), "
          "gradient %.2e (%d)" % (tag, len(replicas), time.time() - t0, worst["queue"][0], worst["queue"][1], worst["reward"][0],
                                  worst["reward"][1], worst["g_action"][0], worst["g_action"][1]))
    print("%s: non-finite gradient rows: oracle %s, kernel %s" % (tag, sorted(nonfin_ref), sorted(nonfin_kern)))
    print("%s: %d replicas excused by the ulp rule (at most %d)%s" % (tag, len(excused), budget, "".join(
        "\n    replica %d: %s" % (r, ", ".join("%s[%d] gap %.3g, oracle moves %.3g" % e for e in ex)) for r, ex in sorted(excused.items()))))
    for p in problems[:20]:
        print("%s: %s" % (tag, p))
    if len(excused) > budget:
        problems.append("%d replicas needed the ulp excuse (at most %d)" % (len(excused), budget))
    if nonfin_ref != nonfin_kern:
        problems.append("non-finite gradient rows differ: kernel %s, oracle %s" % (sorted(nonfin_kern), sorted(nonfin_ref)))
    return problems, nonfin_ref, nonfin_kern, excused


# ------------------------------------------------------------------------------------------------------------------------
# the fused hybrid network (BASELINE configs 4 / 5)
# ------------------------------------------------------------------------------------------------------------------------
def _hybrid_pass(w):
    """One forward + reverse pass of the bench's batch as bench.py launches it, every output kept raw on the host."""
    import torch
    from dhts import ops
    dev = w.action.device
    err, err_bwd = ops.new_error_record(dev), ops.new_error_record(dev)
    a = w.action.detach().clone().requires_grad_(True)
    cut, _, queue, counts = ops.net_hybrid_rollout(a, w.tab, w.sq, w.F, w.dt, w.um, err=err, err_bwd=err_bwd)
    (-cut.sum()).backward()
    torch.cuda.synchronize()
    out = dict(reward=cut.detach().cpu().numpy(), queue=queue.cpu().numpy(), counts=counts.cpu().numpy(),
               grad=a.grad.cpu().numpy(), err=err.cpu().numpy(), err_bwd=err_bwd.cpu().numpy())
    del cut, queue, counts, a
    from dhts import _lib
    assert _lib.lib().dhts_set_option(_lib.OPT_REWARD_CHAIN, 1) == 0
    try:
        with torch.no_grad():
            _, chain, _, _ = ops.net_hybrid_rollout(w.action.detach(), w.tab, w.sq, w.F, w.dt, w.um, err=ops.new_error_record(dev))
            out["reward_chain"] = chain.cpu().numpy()
    finally:
        _lib.lib().dhts_set_option(_lib.OPT_REWARD_CHAIN, 0)
    torch.cuda.empty_cache()
    return out


def _hybrid_kern(p):
    """The pass' arrays as check_batch wants them (d reward / d action: the pass differentiates -sum reward; the reward in the
    reference's summation order)."""
    return dict(reward=p["reward_chain"], queue=p["queue"], g_action=-p["grad"], n_spawned=p["counts"][:, 0], n_deposits=p["counts"][:, 1])


def _plan(w, R):
    from dhts import ops
    return ops.net_hybrid_plan(R, w.action.shape[1], w.tab, w.sq, w.F, w.dt, w.um)


def _check_hybrid(w, p, rank, replicas):
    from dhts import _lib
    from dhts.network import group_routes
    R = w.action.shape[0]
    routes, ptr = group_routes(w.host_routes, w.host_tab.n_lanes)
    scheds = w.tab.schedules()
    assert scheds.shape == (R, w.T, w.n_lanes)
    assert np.array_equal(scheds[0], w.host_tab.schedule)
    actions = w.action.detach().cpu().numpy()
    tag = "hybrid rank %d x %d" % (rank, R)
    problems, nf_ref, nf_kern, _ = check_batch(tag, "hybrid", w.host_tab, (w.sq, w.F, w.dt, w.um), scheds, actions,
                                               _hybrid_kern(p), replicas, routes, ptr, budget=tag if R == 2048 else "hybrid x 256",
                                               nan_only_in_oracle=NAN_ONLY_IN_ORACLE.get(("hybrid", rank, R)),
                                               wider_excuse=WIDER_EXCUSE.get(("hybrid", rank, R)))
    order = np.abs(p["reward"].astype(np.float64) - p["reward_chain"]) / np.abs(p["reward_chain"].astype(np.float64))
    print("%s: reward in the kernels' own order vs the reference's: %.2e relative at worst (replica %d)"
          % (tag, order.max(), int(order.argmax())))
    print("%s: forward fault record %s, reverse %s" % (tag, p["err"].tolist(), p["err_bwd"].tolist()))
    if p["err"][0] not in (_lib.FAULT_NONE, _lib.FAULT_COLLISION):
        problems.append("forward fault record %s" % p["err"].tolist())
    code, _, rep, _ = p["err_bwd"].tolist()
    if nf_ref and (code != _lib.FAULT_NAN or rep not in nf_ref):
        problems.append("reverse fault record %s does not name a replica of the oracle's non-finite set" % p["err_bwd"].tolist())
    if not nf_ref and code != _lib.FAULT_NONE:
        problems.append("reverse fault record %s on a batch the oracle has finite" % p["err_bwd"].tolist())
    expect = NONFINITE.get(("hybrid", rank, R), set())
    if nf_ref != expect & set(replicas):
        problems.append("the oracle's non-finite set %s is not the pinned %s" % (sorted(nf_ref), sorted(expect)))
    assert not problems, "%s: %d problems, first: %s" % (tag, len(problems), problems[:3])
    return nf_ref


@pytest.fixture(scope="module")
def rank0_2048(cuda):
    """Config 4 / 5's largest batch: rank 0 at 2 048 replicas, one pass under the default plan."""
    import bench
    w = bench.make_workload("itscp_hybrid", cuda, 0, 2048)
    assert w.tab.two_per_cu == 0
    plan = _plan(w, 2048)
    print("\nrank 0 x 2048 plan: %s" % plan)
    assert plan["packed"] and 2048 > plan["cus"]
    return w, _hybrid_pass(w)


def test_hybrid_rank0_2048_every_replica_vs_oracle(rank0_2048):
    """Every one of the 2 048 replicas (the packed plan's second replica of each unit, the constant-in-time schedules of
    replicas 256 ..., tapes above 4 GiB): counts, queues, reward and the raw gradient against the oracle; the non-finite rows
    are the oracle's own, {442, 1945}."""
    w, p = rank0_2048
    nf = _check_hybrid(w, p, 0, range(2048))
    assert nf == {442, 1945}


def test_hybrid_packed_plan_is_bit_identical_at_full_size(rank0_2048):
    """The same 2 048 replicas with one replica per compute unit (the tables' own word), and the first 256 (a batch the
    default plan does not pack): reward, queues, counts and the raw gradient bit for bit, NaN positions included."""
    w, packed = rank0_2048
    try:
        w.tab.two_per_cu = -1
        assert not _plan(w, 2048)["packed"]
        one = _hybrid_pass(w)
    finally:
        w.tab.two_per_cu = 0
    w.restrict(256)
    assert not _plan(w, 256)["packed"]
    small = _hybrid_pass(w)
    for tag, o, n in (("one replica per unit", one, 2048), ("restrict(256)", small, 256)):
        for k in ("reward", "reward_chain", "queue", "counts", "grad"):
            a, b = packed[k][:n], o[k]
            same = np.array_equal(a, b, equal_nan=k != "counts")
            if not same:
                rows = sorted({int(i[0]) for i in np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))))}) if k != "counts" else \
                    sorted({int(i[0]) for i in np.argwhere(a != b)})
                pytest.fail("packed vs %s: %s differs on replicas %s" % (tag, k, rows[:20]))
    print("\npacked == one replica per unit (2048) == unpacked restrict(256): bit for bit")


@pytest.mark.parametrize("rank", [1, 2, 3, 4, 5, 6, 7])
def test_hybrid_rank_batches_vs_oracle(cuda, rank):
    """Config 5's per-rank batches (what an 8-GPU run times): all 256 replicas of ranks 1 .. 7 against the oracle."""
    import bench
    w = bench.make_workload("itscp_hybrid", cuda, rank, 256)
    _check_hybrid(w, _hybrid_pass(w), rank, range(256))


# ------------------------------------------------------------------------------------------------------------------------
# the macro and stepwise network batches
# ------------------------------------------------------------------------------------------------------------------------
def test_itscp_macro_batch_vs_oracle(cuda):
    """bench.py's itscp_macro batch: all 256 replicas through oracle.net_macro."""
    import torch
    import bench
    from dhts import _lib, ops
    w = bench.make_workload("itscp_macro", cuda, 0, 256)
    err = ops.new_error_record(cuda)
    a = w.action.detach().clone().requires_grad_(True)
    reward, queue = ops.net_macro_rollout(a, w.tab, w.sq, w.F, w.dt, w.um, err=err)
    (-reward.sum()).backward()
    torch.cuda.synchronize()
    assert err[0].item() == _lib.FAULT_NONE, err.tolist()
    kern = dict(reward=reward.detach().cpu().numpy(), queue=queue.cpu().numpy(), g_action=-a.grad.cpu().numpy())
    scheds = w.tab.schedule.cpu().numpy()
    assert scheds.shape == (256, w.T, w.n_lanes)
    problems, nf_ref, _, _ = check_batch("macro x 256", "macro", w.host_tab, (w.sq, w.F, w.dt, w.um), scheds,
                                         w.action.detach().cpu().numpy(), kern, range(256))
    assert not nf_ref
    assert not problems, problems[:3]


def test_itscp_stepwise_batch_vs_oracle(cuda):
    """bench.py's itscp_stepwise batch (252 lanes on the persistent kernels): all 256 replicas through oracle.net_hybrid."""
    import torch
    import bench
    from dhts.network import group_routes
    w = bench.make_workload("itscp_stepwise", cuda, 0, 256)
    sq, F = 9, 60
    assert (w.sq, w.F) == (sq, F)
    a = w.action.detach().clone().requires_grad_(True)
    cut, _, queue, counts = w.net.rollout(a, sq, F, w.dt, w.um, check_faults=False)
    (-cut.sum()).backward()
    torch.cuda.synchronize()
    counts = counts.cpu().numpy()
    kern = dict(reward=cut.detach().cpu().numpy(), queue=queue.cpu().numpy().reshape(256, w.T, w.n_lanes),
                g_action=-a.grad.cpu().numpy(), n_spawned=counts[:, 0], n_deposits=counts[:, 1])
    print("\nstepwise fault record %s" % w.net.err.tolist())
    scheds = np.stack([t.schedule for t in w.net.tabs])
    routes, ptr = group_routes(w.host_routes, w.host_tab.n_lanes)
    problems, _, _, _ = check_batch("stepwise x 256", "hybrid", w.net.tabs[0], (sq, F, w.dt, w.um), scheds,
                                    w.action.detach().cpu().numpy(), kern, range(256), routes, ptr)
    assert not problems, problems[:3]


# ------------------------------------------------------------------------------------------------------------------------
# config 3: the 4 096-lane micro launch
# ------------------------------------------------------------------------------------------------------------------------
def test_micro_config3_full_launch_lanes_vs_oracle(cuda, oracle):
    """bench.py's config 3 as it launches it (4 096 lanes x 256 vehicles x 1 000 steps, MicroWorkload.one_pass): final state
    and d loss / d (p0, v0) of lanes across the whole batch -- the first, the middle, the last workgroup's -- against the oracle."""
    import torch
    import bench
    from dhts import ops
    w = bench.make_workload("micro", cuda, 0)
    L, V, T, dt = w.L, w.V, w.T, w.dt
    assert (L, V, T) == (4096, 256, 1000)
    plan = ops.micro_rollout_plan(w.desc, T, has_count=False)
    assert plan == dict(fwd_waves=2, fwd_passes=2, fwd_full_lane=1, bwd_one_vehicle_per_thread=1, bwd_block=256)
    _, g_p0, g_v0 = w.one_pass()
    torch.cuda.synchronize()
    assert w.err[0].item() == 0, w.err.tolist()
    lanes = [0, 1, 1365, 2047, 2048, 3071, 4094, 4095]
    pT, vT = w.out[0][lanes].cpu().numpy(), w.out[1][lanes].cpu().numpy()
    g_p0, g_v0 = g_p0[lanes].cpu().numpy(), g_v0[lanes].cpu().numpy()
    p0b, v0b = (t.numpy() for t in bench.MicroWorkload.inputs(0, L, V))
    p0, v0 = np.ascontiguousarray(p0b[lanes], np.float32), np.ascontiguousarray(v0b[lanes], np.float32)
    assert np.array_equal(p0, w.p0[lanes].cpu().numpy()) and np.array_equal(v0, w.v0[lanes].cpu().numpy())
    par = np.tile(np.array(bench.MicroWorkload.PARAMS), (len(lanes), V, 1))
    f = oracle.micro_rollout_fwd(p0, v0, par, T, dt)
    assert f["rc"] == 0
    b = oracle.micro_rollout_bwd(f, g_pT=np.float32(2e-4) * f["pT"], g_vT=2 * f["vT"])
    rows = []
    for i, l in enumerate(lanes):
        rows.append((l, max(rel_elem(pT[i], f["pT"][i]), rel_elem(vT[i], f["vT"][i])),
                     max(rel_max(g_p0[i], b["g_p0"][i]), rel_max(g_v0[i], b["g_v0"][i]))))
    print("\nconfig 3 (4096 x 256 x 1000, bench launch) vs oracle, lane: state (element-wise), gradient\n    "
          + "\n    ".join("%4d: %.2e %.2e" % r for r in rows))
    assert all(s <= TOL_STATE and g <= TOL_GRAD for _, s, g in rows), rows
