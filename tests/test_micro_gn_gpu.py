"""The Gauss-Newton normal equations inside the fused micro rollout, on the device: dhts.micro_rollout_jvp(fused=True, target=).

The yardstick is existing device code: the same call without target= and with the samples on (probes=range(V), every=1 for the dense
fit), whose samples / t_samples are the very float32 values the new kernel holds.  The test forms the residual in float32, as the
kernel does, and sums the masked products in float64 on the host (tests/micro_gn_ref.py::expected).

Tolerance, derived: each term is exact in double and only the summation order differs, so |got - want| <= n 2^-52 sum|terms| per entry,
n the number of terms of the lane (each of the two sums is within (n - 1) 2^-53 sum|terms| of the exact one).  Every test prints the
largest ratio |got - want| / (n 2^-52 sum|terms|) it saw.  The state outputs are the sibling's bits, sse is the checkpointed target
form's bits (the same order), and the relations between calls -- symmetry, K = 4 inside K = 5 and 7, two runs, permuted directions --
are bit for bit.
Needs a real MI355X: python -m pytest tests -m gpu"""
import os
import subprocess
import sys

import numpy as np
import pytest

import micro_gn_ref as G
import micro_jam_cases as J
from test_micro_params_gpu import lanes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.01
L = 3
WIDTHS = (1, 5, 64, 65, 130)
STEPS = (1, 7, 37)
SHAPES = [(V, T) for V in WIDTHS for T in STEPS]
KINDS = ("head", "lead", "ring")
MASKS = ("dense", "all_nan", "plane", "entries")
WORST = {"ratio": 0.0}


def t32(a, cuda):
    import torch
    return torch.tensor(np.ascontiguousarray(a, np.float32), device=cuda)


def t64(a, cuda):
    import torch
    return torch.tensor(np.ascontiguousarray(a, np.float64), device=cuda, dtype=torch.float64)


def n(t):
    return t.detach().cpu().numpy()


def counts(V):
    """Ragged: a full lane, an empty one, and a lane cut short (count = V where V = 1)."""
    return [V, 0, max(1, V // 2 + 1 if V > 2 else V)]


class Case:
    """The inputs of one shape on the device, K directions of every tangent, and the three boundaries."""

    def __init__(self, cuda, V, T, K, cnt=None, lanes_=L, seed=0):
        import torch
        self.V, self.T, self.K, self.L, self.cuda = V, T, K, lanes_, cuda
        rng = self.rng = np.random.default_rng(1000 * V + 10 * T + K + seed)
        p0, v0, par, head = lanes(rng, lanes_, V)
        par[5] = rng.uniform(4.0, 6.0, par[5].shape)
        self.cnt = counts(V)[:lanes_] if cnt is None else cnt
        self.p0, self.v0, self.par = t32(p0, cuda), t32(v0, cuda), t64(par, cuda)
        self.count = torch.tensor(self.cnt, device=cuda, dtype=torch.int32)
        self.head = t64(head, cuda)
        vl = rng.uniform(12.0, 18.0, lanes_)
        start = np.array([float(p0[l, c - 1]) + 30.0 if c > 0 else 10.0 for l, c in enumerate(self.cnt)])
        self.lead = t32(np.stack([start[None, :] + vl[None, :] * DT * np.arange(T)[:, None], np.tile(vl[None, :], (T, 1))], -1), cuda)
        self.lead_length = t64(rng.uniform(4.0, 6.0, lanes_), cuda)
        self.ring = t64([(float(p0[l, c - 1]) - float(p0[l, 0]) if c > 0 else 0.0) + rng.uniform(25.0, 35.0) for l, c in enumerate(self.cnt)], cuda)
        self.t_p0, self.t_v0 = t32(rng.standard_normal((K, lanes_, V)), cuda), t32(rng.standard_normal((K, lanes_, V)), cuda)
        self.t_params = t64(rng.standard_normal((K, 6, lanes_, V)) * 0.1, cuda)
        self.t_head = t64(rng.standard_normal((K, lanes_, 2)), cuda)
        self.t_lead = t32(rng.standard_normal((K, T, lanes_, 2)), cuda)

    def kwargs(self, kind, with_params, dirs=None):
        """The keywords of dhts.micro_rollout_jvp for one boundary; dirs: the directions to pass, in that order (None: all)."""
        import torch
        idx = torch.arange(self.K, device=self.cuda) if dirs is None else torch.tensor(list(dirs), device=self.cuda)
        kw = dict(t_p0=self.t_p0[idx].contiguous(), t_v0=self.t_v0[idx].contiguous(), count=self.count, fused=True)
        if with_params:
            kw["t_params"] = self.t_params[idx].contiguous()
        if kind == "head":
            kw.update(t_head=self.t_head[idx].contiguous())
        elif kind == "lead":
            kw.update(lead=self.lead, lead_length=self.lead_length, t_lead=self.t_lead[idx].contiguous())
        else:
            kw.update(ring=self.ring)
        return kw

    def run(self, kind, with_params, dirs=None, **more):
        import dhts
        return dhts.micro_rollout_jvp(self.p0, self.v0, self.par, self.head if kind == "head" else None, self.T, DT,
                                      **self.kwargs(kind, with_params, dirs), **more)


def samplings(V, T):
    """(probes, every): the dense fit; every third step (T is no multiple of 3) at probes that include the tail, the head of the full
    lane and slots at or beyond the shorter lanes' count; every slot at every second step."""
    return [(None, 1), (sorted({0, V // 2, V - 1}), 3), (None, 2)]


def observed(sampling, V):
    """The keywords that switch the sibling's samples on at the same rows and columns (its dense history is probes=range(V), every=1)."""
    probes, every = sampling
    return dict(probes=list(range(V)) if probes is None and every == 1 else probes, every=every)


def make_target(rng, samples, live_cols, mask):
    """What was observed: the samples plus noise, the missing observations of `mask`, and garbage (NaN and 1e30, alternating) in
    every column whose slot is at or beyond count, which nothing may read."""
    target = (samples + rng.standard_normal(samples.shape).astype(np.float32) * np.float32(2.0)).astype(np.float32)
    if mask == "all_nan":
        target[:] = np.nan
    elif mask == "plane":
        target[:, :, int(rng.integers(2))] = np.nan
    elif mask == "entries":
        target[rng.uniform(size=target.shape) < 0.2] = np.nan
    garbage = np.where(np.arange(target.shape[3]) % 2 == 0, np.float32(np.nan), np.float32(1e30))
    dead = np.broadcast_to(~live_cols[None, :, None, :], target.shape)
    return np.where(dead, np.broadcast_to(garbage, target.shape), target).astype(np.float32)


def live_columns(cnt, probes, V):
    cols = np.arange(V) if probes is None else np.asarray(probes)
    return cols[None, :] < np.asarray(cnt)[:, None]


def check_sums(tag, got_prim, got_tang, want_prim, want_tang, target, live_cols, mask):
    """The state outputs: the sibling's bits.  sse, jtr, jtj: within the derived bound of the host sums over the sibling's samples."""
    import torch
    assert len(got_prim) == 3 and len(got_tang) == 4, tag
    assert torch.equal(got_prim[0], want_prim[0]) and torch.equal(got_prim[1], want_prim[1]), tag + ": pT, vT"
    assert torch.equal(got_tang[0], want_tang[0]) and torch.equal(got_tang[1], want_tang[1]), tag + ": t_pT, t_vT"
    sse, jtr, jtj = n(got_prim[2]), n(got_tang[2]), n(got_tang[3])
    K, lanes_ = want_tang[0].shape[0], want_prim[0].shape[0]
    assert sse.shape == (lanes_, 2) and jtr.shape == (lanes_, K) and jtj.shape == (lanes_, K, K), tag
    assert sse.dtype == jtr.dtype == jtj.dtype == np.float64, tag
    e = G.expected(n(want_prim[2]), n(want_tang[2]), target, live_cols)
    worst = 0.0
    for key, got in (("sse", sse), ("jtr", jtr), ("jtj", jtj)):
        ok, ratio = G.within_bound(got, e[key], e["abs_" + key], e["n"])
        worst = max(worst, ratio)
        assert ok, "%s: %s\n%s\nagainst\n%s" % (tag, key, got, e[key])
    assert np.array_equal(jtj, jtj.transpose(0, 2, 1)), tag + ": jtj is not bit-symmetric"
    if mask == "all_nan":
        assert not sse.any() and not jtr.any() and not jtj.any(), tag + ": nothing observed must give exactly 0"
    nothing = e["n"] == 0
    assert not sse[nothing].any() and not jtr[nothing].any() and not jtj[nothing].any(), tag + ": a lane without a term"
    WORST["ratio"] = max(WORST["ratio"], worst)
    return worst


# =================================================================================================================
# 1. against the sibling's samples, every shape, boundary, K, mask and sampling
# =================================================================================================================
@pytest.mark.parametrize("shape", SHAPES, ids=["V%d_T%d" % s for s in SHAPES])
def test_normal_equations_against_the_siblings_samples(cuda, shape):
    """K in {1, 2, 3, 4, 5, 7} x the three boundaries x with and without t_params.  The sampling follows (K's index + the boundary's)
    mod 3 and the mask (K's index + 2 t_params + the boundary's) mod 4, so that at every shape every (boundary, mask) pair and every
    (boundary, sampling, t_params) triple occurs, the dense fit with t_params at K >= 3 -- the widest kernel with the parameter
    term -- on every boundary among them; the test asserts that they did.  Dense fits also hold sse against
    dhts.micro_rollout(checkpoint=True, target=) bit for bit."""
    import torch
    import dhts
    V, T = shape
    worst, runs = 0.0, 0
    seen_masks, seen_samplings, wide_dense = set(), set(), set()
    for ki, K in enumerate((1, 2, 3, 4, 5, 7)):
        c = Case(cuda, V, T, K)
        for bi, kind in enumerate(KINDS):
            for with_params in (False, True):
                si = (ki + bi) % 3
                sampling = samplings(V, T)[si]
                mask = MASKS[(ki + 2 * int(with_params) + bi) % 4]
                seen_masks.add((kind, mask))
                seen_samplings.add((kind, si, with_params))
                if si == 0 and with_params and K >= 3:
                    wide_dense.add(kind)
                probes, every = sampling
                tag = "V %d T %d K %d %s params %d probes %s every %d mask %s" % (V, T, K, kind, with_params, probes, every, mask)
                want_prim, want_tang = c.run(kind, with_params, **observed(sampling, V))
                live_cols = live_columns(c.cnt, probes, V)
                target = make_target(c.rng, n(want_prim[2]), live_cols, mask)
                assert target.shape == (T // every, L, 2, V if probes is None else len(probes))
                t_target = t32(target, cuda)
                kw = {} if probes is None and every == 1 else dict(probes=probes, every=every)
                got_prim, got_tang = c.run(kind, with_params, target=t_target, **kw)
                worst = max(worst, check_sums(tag, got_prim, got_tang, want_prim, want_tang, target, live_cols, mask))
                if probes is None and every == 1:      # the checkpointed target form sums in the same order
                    with torch.no_grad():
                        ref = dhts.micro_rollout(c.p0, c.v0, c.par, c.head if kind == "head" else None, T, DT, count=c.count, checkpoint=True,
                                                 target=t_target, **{k: v for k, v in c.kwargs(kind, False).items()
                                                                     if k in ("lead", "lead_length", "ring")})
                    assert np.array_equal(n(got_prim[2]), n(ref[2])), tag + ": sse is not the checkpointed target form's"
                runs += 1
    print("V %d T %d: %d calls, largest |got - want| / (n 2^-52 sum|terms|) = %.3f" % (V, T, runs, worst))
    assert runs == 36
    assert seen_masks == {(k, m) for k in KINDS for m in MASKS}
    assert seen_samplings == {(k, s, w) for k in KINDS for s in range(3) for w in (False, True)}
    assert wide_dense == set(KINDS)


def test_full_lane_runs_the_narrower_width_and_the_pair_scheme(cuda):
    """V = 1024, T = 5 with t_params: the plan carries 2 directions per launch, K = 3 is three launches of the pair scheme and K = 5
    ten; without t_params the width is 4."""
    from dhts import ops
    V, T = 1024, 5
    desc = ops.micro_desc(L, V, DT)
    assert ops.micro_fwd_jvp_gn_plan(desc, T, 5, True)["dirs_per_launch"] == 2 and ops.micro_fwd_jvp_gn_plan(desc, T, 5, True)["launches"] == 10
    for K, with_params, kind in ((5, True, "head"), (3, True, "ring"), (5, False, "lead")):
        c = Case(cuda, V, T, K, cnt=[V, 0, 700])
        want_prim, want_tang = c.run(kind, with_params, probes=list(range(V)), every=1)
        live_cols = live_columns(c.cnt, None, V)
        target = make_target(c.rng, n(want_prim[2]), live_cols, "entries")
        got_prim, got_tang = c.run(kind, with_params, target=t32(target, cuda))
        r = check_sums("V 1024 K %d %s" % (K, kind), got_prim, got_tang, want_prim, want_tang, target, live_cols, "entries")
        print("V 1024 K %d %s params %d: ratio %.3f" % (K, kind, with_params, r))


# =================================================================================================================
# 2. relations between calls, bit for bit
# =================================================================================================================
@pytest.mark.parametrize("kind", KINDS)
def test_bit_relations_between_calls(cuda, kind):
    """Two runs are equal; the leading 4 x 4 block and the first four jtr of a K = 5 and of a K = 7 call are a K = 4 call's; permuting the
    directions permutes jtj and jtr exactly."""
    import torch
    V, T, K = 65, 7, 7
    c = Case(cuda, V, T, K)
    hist = n(c.run(kind, True, probes=list(range(V)), every=1)[0][2])
    target = t32(make_target(c.rng, hist, live_columns(c.cnt, None, V), "entries"), cuda)
    for with_params in (True, False):
        full = c.run(kind, with_params, target=target)
        again = c.run(kind, with_params, target=target)
        for a, b in zip(full[0] + full[1], again[0] + again[1]):
            assert torch.equal(a, b), "two runs of the same call differ"
        four = c.run(kind, with_params, dirs=range(4), target=target)
        for Kn in (5, 7):
            more = c.run(kind, with_params, dirs=range(Kn), target=target)
            assert torch.equal(more[1][3][:, :4, :4], four[1][3]) and torch.equal(more[1][2][:, :4], four[1][2]), Kn
            assert torch.equal(more[0][2], four[0][2]) and torch.equal(more[1][0][:4], four[1][0])
            assert torch.equal(more[1][3], more[1][3].transpose(1, 2))
        for perm in ((6, 5, 4, 3, 2, 1, 0), (2, 0, 6, 1, 5, 3, 4), (3, 1, 4), (1, 0)):
            p = torch.tensor(perm, device=cuda)
            got = c.run(kind, with_params, dirs=perm, target=target)
            assert torch.equal(got[1][3], full[1][3][:, p][:, :, p]), "jtj under the permutation %s" % (perm,)
            assert torch.equal(got[1][2], full[1][2][:, p]), "jtr under the permutation %s" % (perm,)
            assert torch.equal(got[0][2], full[0][2])


def test_empty_rollouts_and_empty_lanes_give_zeros(cuda):
    """T = 0, T < every (no row) and a call whose lanes are all empty: sse, jtr and jtj exactly 0, the state passes through."""
    import torch
    for V, T, every, cnt in ((5, 0, 1, None), (65, 2, 3, None), (65, 7, 1, [0, 0, 0])):
        c = Case(cuda, V, T, 3, cnt=cnt)
        for kind in KINDS:
            target = torch.full((T // every, L, 2, V), 3.0, device=cuda)
            prim, tang = c.run(kind, True, target=target, **({} if every == 1 else dict(every=every)))
            assert prim[2].shape == (L, 2) and tang[2].shape == (L, 3) and tang[3].shape == (L, 3, 3)
            assert not prim[2].any() and not tang[2].any() and not tang[3].any(), (V, T, kind)
            if T == 0 or cnt is not None:
                assert torch.equal(prim[0], c.p0) and torch.equal(prim[1], c.v0)


# =================================================================================================================
# 3. fault records
# =================================================================================================================
def test_collision_record_is_the_siblings(cuda):
    """A stop wave in which one vehicle runs into the standing queue: err holds what dhts_micro_rollout_fwd_jvp_samples reports, the
    tangents' record stays clear, and the sums are still those of the sibling's samples."""
    import torch
    from dhts import ops
    case = J.COLLIDE[0]
    assert case.kind == "head"
    lanes_, V = case.p0.shape
    K = 2
    rng = np.random.default_rng(3)
    desc = ops.micro_desc(lanes_, V, case.dt)
    p0, v0, par, head = t32(case.p0, cuda), t32(case.v0, cuda), t64(case.params, cuda), t64(case.boundary, cuda)
    count = torch.tensor(case.count, device=cuda, dtype=torch.int32)
    t_p, t_v = t32(rng.standard_normal((K, lanes_, V)), cuda), t32(rng.standard_normal((K, lanes_, V)), cuda)
    e1, j1, e2, j2 = (ops.new_error_record(cuda) for _ in range(4))
    want_prim, want_tang = ops.micro_rollout_fwd_jvp_samples(desc, case.T, p0, v0, par, head, t_p, t_v, None, 1, count=count, err=e1, err_jvp=j1)
    live_cols = live_columns(case.count, None, V)
    target = make_target(rng, n(want_prim[2]), live_cols, "entries")
    got_prim, got_tang = ops.micro_rollout_fwd_jvp_gn(desc, case.T, p0, v0, par, t_p, t_v, t32(target, cuda), head=head, count=count, err=e2,
                                                      err_jvp=j2)
    assert int(e1[0]) != 0, "the case collides"
    assert torch.equal(e1, e2) and torch.equal(j1, j2) and int(j2[0]) == 0
    check_sums("collision", got_prim, got_tang, want_prim, want_tang, target, live_cols, "entries")


def test_nan_tangents_raise_the_siblings_fault(cuda):
    import torch
    c = Case(cuda, 65, 7, 2)
    c.t_p0[1, 0, 3] = float("nan")
    raised = []
    for more in (dict(probes=list(range(65)), every=1), dict(target=torch.zeros(7, L, 2, 65, device=cuda))):
        with pytest.raises(Exception) as info:
            c.run("head", False, **more)
        raised.append((type(info.value), str(info.value)))
    assert raised[0] == raised[1], raised
    prim, tang = c.run("head", False, target=torch.zeros(7, L, 2, 65, device=cuda), check_faults=False)
    assert torch.isnan(tang[3][0, 1, 1]) and not torch.isnan(tang[3][0, 0, 0]) and not torch.isnan(tang[3][2]).any()


# =================================================================================================================
# 4. nothing of size T x V is allocated
# =================================================================================================================
def test_peak_memory_stays_below_one_history(cuda):
    """64 x 256 x 400, K = 5 with t_params: above the resident inputs (target among them: it is data) the call's peak stays below ONE
    history of 52 MB; the existing path holds six of them (hist and five directions of t_hist)."""
    import torch
    lanes_, V, T, K = 64, 256, 400, 5
    c = Case(cuda, V, T, K, cnt=[V] * lanes_, lanes_=lanes_)
    target = torch.zeros(T, lanes_, 2, V, device=cuda)
    one_history = T * lanes_ * 2 * V * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    prim, tang = c.run("head", True, target=target)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("peak above the resident inputs: %.2f MB (one history: %.1f MB)" % (peak / 1e6, one_history / 1e6))
    assert peak < one_history
    assert tang[3].shape == (lanes_, K, K)
    del prim, tang
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    c.run("head", True, want_hist=True)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base >= 6 * one_history


# =================================================================================================================
# 5. the example
# =================================================================================================================
def run_example(tmp_path, name, flags):
    """One run of the example at a small shape -> [(parameter error, loss)] per iteration, from its log."""
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    cmd = [sys.executable, os.path.join(ROOT, "examples", "calibrate_idm.py"), "--method", "lm", "--fused", "--seed", "1", "--n_lane", "3",
           "--n_vehicle", "9", "--n_step", "40", "--n_episode", "6", "--run_name", name] + list(flags)
    out = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    log = os.path.join(str(tmp_path), "result", "calibrate", name, "lm", "trial_0.txt")
    return [tuple(float(x) for x in line.split()) for line in open(log).read().splitlines()]


@pytest.mark.parametrize("flags", ((), ("--observe", "2,5"), ("--leader",), ("--ring", "200")), ids=["dense", "observe", "leader", "ring"])
def test_example_forms_the_normal_equations_in_the_kernel(cuda, tmp_path, flags):
    """calibrate_idm.py --method lm --fused --fused-loss: the first line's loss is the --fused run's to 1e-12 relative (the same exact
    terms in another order: float64 both ways).  The later lines pass through a linear solve, so the fit is only asked to converge to
    the same parameter error to three digits."""
    a, b = run_example(tmp_path, "torch", flags), run_example(tmp_path, "kernel", flags + ("--fused-loss",))
    assert len(a) == len(b) == 6
    print("calibrate_idm.py --method lm --fused %s" % " ".join(flags))
    for (ea, la), (eb, lb) in zip(a, b):
        print("  loss %.17g / %.17g (rel %.1e)   parameter error %.6e / %.6e" % (la, lb, abs(la - lb) / la, ea, eb))
    assert abs(a[0][1] - b[0][1]) <= 1e-12 * abs(a[0][1]), (a[0], b[0])
    assert b[-1][1] < b[0][1], "the fit does not lower the loss"
    assert abs(a[-1][0] - b[-1][0]) <= 5e-4 * abs(a[-1][0]), "the two fits end at different parameter errors: %r, %r" % (a[-1], b[-1])


@pytest.fixture(scope="module", autouse=True)
def report_the_largest_ratio_seen():
    """Prints, behind the module's last test, the largest ratio check_sums saw (each call has asserted its own bound)."""
    yield
    print("\nlargest |got - want| / (n 2^-52 sum|terms|) over this module's cases: %.3f" % WORST["ratio"])
