"""A ring road on the two tape-free paths of the micro rollout (dhts_micro_rollout_fwd_ckpt_ring / _bwd_ckpt_ring / _fwd_jvp_ring /
_fwd_ckpt_target_ring / _bwd_ckpt_target_ring, the ops wrappers of the same names, dhts.micro_rollout(ring=) and
dhts.micro_rollout_jvp(ring=)): the boundary of the library -- header, bindings, exports, argument checks, every ValueError -- and the
validation of the yardstick tests/micro_ring_ref.py::ring_rollout against lead_rollout and the C oracle.  What the kernels compute is
held against existing device code and the yardstick in tests/test_micro_ring_gpu.py.  No GPU needed."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from micro_lead_ref import lead_rollout, trajectory_before_steps
from micro_ring_ref import restated_ring, ring_rollout, tail_image
from test_micro_params import GOLDENS, golden_case
from util import TOL_GRAD, TOL_STATE, grad_report, rel_elem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dhts_micro_rollout_fwd_ckpt_ring", "dhts_micro_rollout_bwd_ckpt_ring", "dhts_micro_rollout_fwd_jvp_ring",
       "dhts_micro_rollout_fwd_ckpt_target_ring", "dhts_micro_rollout_bwd_ckpt_target_ring")
FWD = ("p", "v", "count", "params", "ring", "p_out", "v_out", "ckpt", "probes", "n_probes", "every", "samples", "err", "stream")
BWD = ("ckpt", "count", "params", "ring", "g_p", "g_v", "probes", "n_probes", "every", "g_samples", "g_p_out", "g_v_out", "g_params", "err",
       "stream")
JVP = ("p", "v", "count", "params", "ring", "t_p", "t_v", "t_params", "p_out", "v_out", "t_p_out", "t_v_out", "probes", "n_probes", "every",
       "samples", "t_samples", "err", "err_jvp", "stream")
FWD_T = ("p", "v", "count", "params", "ring", "p_out", "v_out", "ckpt", "target", "sse", "err", "stream")
BWD_T = ("ckpt", "count", "params", "ring", "g_p", "g_v", "target", "g_sse", "g_p_out", "g_v_out", "g_params", "err", "stream")
ARGS = dict(zip(NEW, (FWD, BWD, JVP, FWD_T, BWD_T)))
REQUIRED = {NEW[0]: ("p", "v", "params", "ring", "p_out", "v_out"),
            NEW[1]: ("ckpt", "params", "ring", "g_p", "g_v", "g_p_out", "g_v_out"),
            NEW[2]: ("p", "v", "params", "ring", "t_p", "t_v", "p_out", "v_out", "t_p_out", "t_v_out"),
            NEW[3]: ("p", "v", "params", "ring", "p_out", "v_out", "target", "sse"),
            NEW[4]: ("ckpt", "params", "ring", "g_p", "g_v", "target", "g_p_out", "g_v_out")}


def test_header_library_and_bindings_hold_the_new_entry_points():
    import dhts
    from dhts import _lib, ops
    raw = open(os.path.join(ROOT, "include", "dhts.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib.lib()
    for name, names in ARGS.items():
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, txt)
        assert m, "include/dhts.h does not declare %s" % name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
        assert len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1 == len(names) + 3, name        # d, T, segment / n_dir first
        declared = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
        assert declared[3:] == list(names), "the header's argument names of %s" % name
        ints = [i for i, t in enumerate(_lib.SIGNATURES[name][1]) if t is C.c_int]
        sampled = [3 + names.index("n_probes"), 3 + names.index("every")] if "every" in names else []
        assert ints == [1, 2] + sampled, name
        for gone in ("head", "t_head", "g_head", "lead", "lead_length", "g_lead", "t_lead"):
            assert gone not in names
    # each beside its lead sibling, in its argument order: ring where (lead, lead_length) stand, no g_lead / t_lead
    from test_micro_lead import BWD as L_BWD, FWD as L_FWD, JVP as L_JVP
    for ours, theirs in ((FWD, L_FWD), (BWD, L_BWD), (JVP, L_JVP)):
        want = [("ring" if a == "lead" else a) for a in theirs if a not in ("lead_length", "g_lead", "t_lead")]
        assert list(ours) == want
    comment = raw[raw.index("A RING ROAD on the two tape-free paths"):raw.index("int " + NEW[0])]
    for cited in ("_micro_lane.py:131-214", "dmicro_lane.py:230-298", ":130-153", "DHTS_E_INVALID", "UNWRAPPED", "(float)((double)p_tail + ring[l])",
                  "half_len = (length[slot 0] + length[head]) / 2", "gap >= 1e-5", "n = 1", "n = 0", "-0.5 (A[0] + A[n - 1])",
                  "-(t_len[head] + t_len[tail]) / 2", "DHTS_FAULT_COLLISION", "NOT differentiated"):
        assert cited in comment, cited
    for name in ("micro_rollout_fwd_ckpt_ring", "micro_rollout_bwd_ckpt_ring", "micro_rollout_fwd_jvp_ring",
                 "micro_rollout_fwd_ckpt_target_ring", "micro_rollout_bwd_ckpt_target_ring", "MicroRolloutRing", "MicroRolloutRingTarget",
                 "_micro_ring_checks"):
        assert callable(getattr(ops, name))
    assert dhts.MicroRolloutRing is ops.MicroRolloutRing and dhts.MicroRolloutRingTarget is ops.MicroRolloutRingTarget
    par = inspect.signature(dhts.micro_rollout).parameters
    assert par["ring"].default is None and list(par)[-3:] == ["lead_length", "ring", "target"]
    par = inspect.signature(dhts.micro_rollout_jvp).parameters
    assert par["ring"].default is None and par["ring"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(ops.MicroRollout.forward).parameters)[-1] == "checkpoint", "the existing operators keep their signatures"
    assert list(inspect.signature(ops.MicroRolloutSamples.forward).parameters)[-1] == "every"
    assert list(inspect.signature(ops.MicroRolloutLead.forward).parameters)[-1] == "observe"
    assert list(inspect.signature(ops.MicroRolloutTarget.forward).parameters)[-1] == "target"


def call_args(names, some, **kw):
    a = {n: some for n in names}
    a.update(stream=None, n_probes=4, every=2)
    a.update(kw)
    return [a[n] for n in names]


def test_bad_arguments_are_rejected_without_a_gpu():
    """DHTS_E_INVALID with nothing dereferenced: `some` is a pointer nobody may follow, and no device exists here to launch on."""
    from dhts import _lib
    lib = _lib.lib()
    ok = _lib.MicroDesc(4, 70, 0.01)
    some = C.c_void_p(64)
    for name, names in ARGS.items():
        fn = getattr(lib, name)
        for missing in REQUIRED[name]:
            assert fn(C.byref(ok), 5, 1, *call_args(names, some, **{missing: None})) == _lib.E_INVALID, (name, missing)
        for bad in (_lib.MicroDesc(4, 5000, 0.01), _lib.MicroDesc(0, 70, 0.01), _lib.MicroDesc(4, 70, 0.0)):
            assert fn(C.byref(bad), 5, 1, *call_args(names, some)) == _lib.E_INVALID
        assert fn(C.byref(ok), -1, 1, *call_args(names, some)) == _lib.E_INVALID
        assert fn(C.byref(ok), 0, 1, *call_args(names, some, ring=None)) == _lib.E_INVALID, "a NULL ring, T = 0 included"
        if "every" in names:
            assert fn(C.byref(ok), 5, 1, *call_args(names, some, every=0)) == _lib.E_INVALID
            assert fn(C.byref(ok), 5, 1, *call_args(names, some, n_probes=0)) == _lib.E_INVALID
            assert fn(C.byref(ok), 5, 1, *call_args(names, some, n_probes=71)) == _lib.E_INVALID
    # a segment the reverse kernels' ring of steps cannot hold: the siblings' plans hold for the ring forms
    plan = (C.c_int32 * 8)()
    for plan_fn, fwd, bwd in ((lib.dhts_micro_ckpt_plan, NEW[0], NEW[1]), (lib.dhts_micro_ckpt_target_plan, NEW[3], NEW[4])):
        for want_params, g_params in ((0, None), (1, some)):
            assert plan_fn(C.byref(ok), 5, want_params, 0, C.byref(plan)) == 0
            assert getattr(lib, bwd)(C.byref(ok), 5, plan[2] + 1, *call_args(ARGS[bwd], some, g_params=g_params)) == _lib.E_INVALID
        assert plan_fn(C.byref(ok), 5, 0, 0, C.byref(plan)) == 0
        assert getattr(lib, fwd)(C.byref(ok), 5, plan[2] + 1, *call_args(ARGS[fwd], some)) == _lib.E_INVALID
    # the fused kernel's sample arrays: both or neither
    assert lib.dhts_micro_rollout_fwd_jvp_ring(C.byref(ok), 5, 1, *call_args(JVP, some, samples=None)) == _lib.E_INVALID
    assert lib.dhts_micro_rollout_fwd_jvp_ring(C.byref(ok), 5, 1, *call_args(JVP, some, t_samples=None)) == _lib.E_INVALID
    assert lib.dhts_micro_rollout_fwd_jvp_ring(C.byref(ok), 5, 0, *call_args(JVP, some)) == _lib.E_INVALID       # n_dir < 1


def test_every_value_error_is_raised_before_a_device_is_touched():
    """CPU tensors throughout: a call that reached a kernel wrapper would raise TypeError (not a CUDA tensor), not ValueError."""
    import torch
    import dhts
    from dhts import ops
    L, V, T, dt = 2, 5, 4, 0.1
    p0, v0 = torch.zeros(L, V), torch.zeros(L, V)
    params = torch.ones(6, L, V, dtype=torch.float64)
    head = torch.zeros(L, 2, dtype=torch.float64)
    lead = torch.zeros(T, L, 2)
    ring = torch.full((L,), 100.0, dtype=torch.float64)
    target = torch.zeros(T, L, 2, V)
    with pytest.raises(ValueError, match="checkpoint=True"):
        dhts.micro_rollout(p0, v0, params, None, T, dt, ring=ring)
    with pytest.raises(ValueError, match="checkpoint=True"):
        dhts.micro_rollout(p0, v0, params, None, T, dt, ring=ring, checkpoint=False, probes=[0], every=2)
    with pytest.raises(ValueError, match=r"probes=range\(V\) with every=1"):
        dhts.micro_rollout(p0, v0, params, None, T, dt, ring=ring, checkpoint=True, want_hist=True)
    with pytest.raises(ValueError, match="head must be None when ring"):
        dhts.micro_rollout(p0, v0, params, head, T, dt, ring=ring, checkpoint=True)
    with pytest.raises(ValueError, match="lead / lead_length must be None when ring"):
        dhts.micro_rollout(p0, v0, params, None, T, dt, ring=ring, lead=lead, checkpoint=True)
    with pytest.raises(ValueError, match="lead / lead_length must be None when ring"):
        dhts.micro_rollout(p0, v0, params, None, T, dt, ring=ring, lead_length=torch.ones(L, dtype=torch.float64), checkpoint=True)
    for bad in (torch.ones(L), torch.ones(L + 1, dtype=torch.float64), torch.ones(L, 1, dtype=torch.float64), np.ones(L), 100.0):
        with pytest.raises(ValueError, match="ring must be a float64 tensor of shape"):
            dhts.micro_rollout(p0, v0, params, None, T, dt, ring=bad, checkpoint=True)
        with pytest.raises(ValueError, match="ring must be a float64 tensor of shape"):
            dhts.micro_rollout(p0, v0, params, None, T, dt, ring=bad, checkpoint=True, target=target)
        with pytest.raises(ValueError, match="ring must be a float64 tensor of shape"):
            dhts.micro_rollout_jvp(p0, v0, params, None, T, dt, t_p0=torch.zeros(1, L, V), ring=bad, fused=True)
    with pytest.raises(ValueError, match="ring is not differentiable"):
        dhts.micro_rollout(p0, v0, params, None, T, dt, ring=ring.clone().requires_grad_(), checkpoint=True)
    with pytest.raises(ValueError, match="checkpoint must be"):
        dhts.micro_rollout(p0, v0, params, None, T, dt, ring=ring, checkpoint=-2)
    with pytest.raises(ValueError, match="segment must be"):
        dhts.micro_rollout(p0, v0, params, None, T, dt, ring=ring, checkpoint=10 ** 6)
    with pytest.raises(ValueError, match="every must be"):
        dhts.micro_rollout(p0, v0, params, None, T, dt, ring=ring, checkpoint=True, every=0)
    with pytest.raises(ValueError, match="strictly ascending"):
        dhts.micro_rollout(p0, v0, params, None, T, dt, ring=ring, checkpoint=True, probes=[1, 0])
    # next to target: the ring's checks first, then the target's own
    with pytest.raises(ValueError, match="head must be None when ring"):
        dhts.micro_rollout(p0, v0, params, head, T, dt, ring=ring, checkpoint=True, target=target)
    with pytest.raises(ValueError, match="target does not take probes"):
        dhts.micro_rollout(p0, v0, params, None, T, dt, ring=ring, checkpoint=True, target=target, probes=[0])
    with pytest.raises(ValueError, match="target must be a float32 tensor of shape"):
        dhts.micro_rollout(p0, v0, params, None, T, dt, ring=ring, checkpoint=True, target=target[1:])
    with pytest.raises(ValueError, match="max_segment of the target forms"):
        dhts.micro_rollout(p0, v0, params, None, T, dt, ring=ring, checkpoint=10 ** 6, target=target)
    # forward mode
    t_p0 = torch.zeros(3, L, V)
    with pytest.raises(ValueError, match="fused=True"):
        dhts.micro_rollout_jvp(p0, v0, params, None, T, dt, t_p0=t_p0, ring=ring)
    with pytest.raises(ValueError, match="head and t_head must be None when ring"):
        dhts.micro_rollout_jvp(p0, v0, params, None, T, dt, t_p0=t_p0, t_head=torch.zeros(3, L, 2, dtype=torch.float64), ring=ring, fused=True)
    with pytest.raises(ValueError, match="head and t_head must be None when ring"):
        dhts.micro_rollout_jvp(p0, v0, params, head, T, dt, t_p0=t_p0, ring=ring, fused=True)
    with pytest.raises(ValueError, match="lead, lead_length and t_lead must be None when ring"):
        dhts.micro_rollout_jvp(p0, v0, params, None, T, dt, t_p0=t_p0, ring=ring, lead=lead, fused=True)
    with pytest.raises(ValueError, match="lead, lead_length and t_lead must be None when ring"):
        dhts.micro_rollout_jvp(p0, v0, params, None, T, dt, t_p0=t_p0, ring=ring, t_lead=torch.zeros(3, T, L, 2), fused=True)
    with pytest.raises(ValueError, match=r"probes=range\(V\) with every=1"):
        dhts.micro_rollout_jvp(p0, v0, params, None, T, dt, t_p0=t_p0, ring=ring, fused=True, want_hist=True)
    with pytest.raises(ValueError, match="at least one of"):
        dhts.micro_rollout_jvp(p0, v0, params, None, T, dt, ring=ring, fused=True)
    with pytest.raises(ValueError, match="every must be"):
        dhts.micro_rollout_jvp(p0, v0, params, None, T, dt, t_p0=t_p0, ring=ring, fused=True, every=0)
    # ... and the raw wrappers' own, which need no device either
    desc, ck = ops.micro_desc(L, V, dt), torch.zeros(0)
    with pytest.raises(ValueError, match="ring must be a contiguous float64"):
        ops.micro_rollout_fwd_ckpt_ring(desc, T, p0, v0, params, ring[:1], None)
    with pytest.raises(ValueError, match="ring must be a contiguous float64"):
        ops.micro_rollout_bwd_ckpt_ring(desc, T, ck, params, torch.ones(2 * L, dtype=torch.float64)[::2], p0, v0)
    with pytest.raises(ValueError, match="ring must be a contiguous float64"):
        ops.micro_rollout_fwd_jvp_ring(desc, T, p0, v0, params, None, t_p0, t_p0)
    with pytest.raises(ValueError, match="ring must be a contiguous float64"):
        ops.micro_rollout_fwd_ckpt_target_ring(desc, T, p0, v0, params, ring.float(), None, target)
    with pytest.raises(ValueError, match="ckpt must be"):
        ops.micro_rollout_bwd_ckpt_ring(desc, T, ck, params, ring, p0, v0)
    with pytest.raises(ValueError, match="ckpt must be"):
        ops.micro_rollout_bwd_ckpt_target_ring(desc, T, ck, params, ring, p0, v0, target)
    with pytest.raises(ValueError, match="target must be a contiguous float32"):
        ops.micro_rollout_fwd_ckpt_target_ring(desc, T, p0, v0, params, ring, None, target[:, :, :, :-1])


def test_resource_listing_keeps_every_existing_kernel():
    """profiles/micro_ring_resources_parent.txt against profiles/micro_ring_resources.txt (compiler output for gfx950, one line per
    kernel of micro_kernels.hip): every kernel of the parent has identical figures -- the twenty-four with a boundary under the longer
    name the enum gives them, false = 0 (the head gap), true = 1 (the leader) --, and the new lines are the twelve ring forms, none with
    scratch or a spill, none above the 128 VGPRs a block of 1024 threads may use."""
    def read(name):
        rows = {}
        for line in open(os.path.join(ROOT, "profiles", name)).read().splitlines():
            kernel, figures = line.split(" SGPRs ")
            rows[kernel.strip()] = "SGPRs " + " ".join(figures.split())
        return rows
    parent, new = read("micro_ring_resources_parent.txt"), read("micro_ring_resources.txt")
    bounded = ("micro_rollout_ckpt_fwd_samples_kernel<", "micro_rollout_ckpt_bwd_samples_kernel<", "micro_rollout_fwd_jvp_samples_kernel<",
               "micro_rollout_ckpt_fwd_target_kernel<", "micro_rollout_ckpt_bwd_target_kernel<")

    def renamed(k):
        if k.startswith(bounded):
            return re.sub(r"(true|false)>$", lambda m: "(dhts::MicroBoundary)%d>" % (m.group(1) == "true"), k)
        return k
    assert len(parent) == 137 and sum(k.startswith(bounded) for k in parent) == 24
    for k, figures in parent.items():
        assert new.get(renamed(k)) == figures, k
    added = sorted(set(new) - {renamed(k) for k in parent})
    assert len(added) == 12 and all(k.startswith(bounded) and k.endswith("(dhts::MicroBoundary)2>") for k in added), added
    assert sum("fwd_jvp_samples" in k for k in added) == 6 and sum("ckpt_bwd" in k for k in added) == 4
    for k in added:
        assert " scratch 0 " in new[k] and " sgpr_spill 0 vgpr_spill 0 " in new[k], (k, new[k])
        assert int(re.search(r"VGPRs\s+(\d+)", new[k]).group(1)) <= 128, (k, new[k])


# =================================================================================================================
# the yardstick, validated twice
# =================================================================================================================
def ring_of(c, slack):
    """A circumference for a golden platoon: its extent, the head's length and `slack` metres of road in front of the head."""
    return np.array([float(c["p0"][0, -1] - c["p0"][0, 0]) + float(c["g"]["params"][-1, 5]) + slack])


@pytest.mark.parametrize("name", GOLDENS)
@pytest.mark.parametrize("slack", (12.0, 60.0))
def test_ring_rollout_is_lead_rollout_fed_its_own_tail(golden_dir, name, slack):
    """The yardstick's own tail trajectory, one circumference ahead, as `lead`, the tail's length as lead_length: lead_rollout gives the
    same states after every step, bit for bit -- ring_rollout differs from it in where the leader comes from and in nothing else.  Also
    with a count below the width, one vehicle and none."""
    import torch
    c = golden_case(golden_dir, name)
    T, dt = min(c["T"], 80), c["dt"]
    V = c["p0"].shape[1]
    ring = ring_of(c, slack)
    p0, v0, par = torch.tensor(c["p0"]), torch.tensor(c["v0"]), torch.tensor(c["params"])
    for n in (V, V // 2, 2, 1, 0):
        count = [n]
        rg = ring if n == V else np.array([float(c["p0"][0, max(n - 1, 0)] - c["p0"][0, 0]) + 5.0 + slack])
        pT, vT, hist = ring_rollout(p0, v0, par, rg, T, dt, count)
        h = hist.numpy()
        lead = np.stack([tail_image(trajectory_before_steps(c["p0"][:, 0], h[:, :, 0, 0]), rg),
                         trajectory_before_steps(c["v0"][:, 0], h[:, :, 1, 0])], -1)                       # [T][1][2]
        qT, wT, hist_l = lead_rollout(p0, v0, par, torch.tensor(lead), T, dt, count, lead_length=c["params"][5, :, 0])
        assert np.array_equal(h, hist_l.numpy()), (name, n)
        assert np.array_equal(pT.numpy(), qT.numpy()) and np.array_equal(vT.numpy(), wT.numpy())
        assert np.array_equal(pT.numpy()[:, n:], c["p0"][:, n:]) and np.array_equal(vT.numpy()[:, n:], c["v0"][:, n:]), "slots beyond count"
        if n > 0:
            assert not np.array_equal(pT.numpy()[:, :n], c["p0"][:, :n])
    # the head does see the tail: another circumference, another trajectory of the head
    a = ring_rollout(p0, v0, par, ring, T, dt)[2].numpy()
    b = ring_rollout(p0, v0, par, ring + 3.0, T, dt)[2].numpy()
    assert not np.array_equal(a[:, :, :, -1], b[:, :, :, -1])


@pytest.mark.parametrize("name", GOLDENS)
def test_ring_rollout_against_a_chain_of_oracle_steps(golden_dir, oracle, name):
    """T single oracle.micro_step calls on n + 1 slots, slot n overwritten before every step with the image of slot 0 and given slot 0's
    length -- the head gap is recomputed from the tail every step.  States after every step; the cotangents through
    oracle.micro_step_bwd, slot n's input cotangent returned to slot 0 in the same step."""
    c = golden_case(golden_dir, name)
    g, dt = c["g"], c["dt"]
    T = min(c["T"], 60)
    n = c["p0"].shape[1]
    ring = ring_of(c, 12.0)
    rng = np.random.default_rng(13)
    par1 = np.concatenate([g["params"], g["params"][:1]], 0).copy()      # [n + 1][6]: slot n has the tail's length
    p, v = np.append(c["p0"][0], 0).astype(np.float32), np.append(c["v0"][0], 0).astype(np.float32)
    hist, tapes = [], []
    for t in range(T):
        p[n], v[n] = tail_image(p[0], ring[0]), v[0]
        o = oracle.micro_step(p, v, par1, 1000.0, 0.0, dt)
        assert o["rc"] == 0
        p, v = o["np"].copy(), o["nv"].copy()
        hist.append(np.stack([p[:n], v[:n]]))
        tapes.append(o["dqs"])
    hist = np.stack(hist)[:, None]                                          # [T][1][2][n]
    g_pT, g_vT = rng.normal(size=(1, n)).astype(np.float32), rng.normal(size=(1, n)).astype(np.float32)
    g_hist = (0.1 * rng.normal(size=hist.shape)).astype(np.float32)
    gp, gv = np.append(g_pT[0], 0).astype(np.float32), np.append(g_vT[0], 0).astype(np.float32)
    through_image = 0.0
    for t in reversed(range(T)):
        gp[:n] += g_hist[t, 0, 0]
        gv[:n] += g_hist[t, 0, 1]
        ip, iv = oracle.micro_step_bwd(tapes[t], gp, gv)
        gp, gv = np.append(ip[:n], 0).astype(np.float32), np.append(iv[:n], 0).astype(np.float32)
        gp[0] += ip[n]
        gv[0] += iv[n]
        through_image += abs(float(ip[n])) + abs(float(iv[n]))
    r = restated_ring(c["p0"], c["v0"], c["params"], ring, T, dt, g_pT=g_pT, g_vT=g_vT, g_hist=g_hist)
    e_s = rel_elem(r["hist"], hist)
    print("%s: ring_rollout vs oracle chain, states %.2e" % (name, e_s))
    assert e_s <= TOL_STATE
    assert rel_elem(r["pT"], hist[-1][:, 0]) <= TOL_STATE and rel_elem(r["vT"], hist[-1][:, 1]) <= TOL_STATE
    assert grad_report("%s ring_rollout vs oracle chain d loss / d p0" % name, r["g_p0"][0], gp[:n]) <= TOL_GRAD
    assert grad_report("%s ring_rollout vs oracle chain d loss / d v0" % name, r["g_v0"][0], gv[:n]) <= TOL_GRAD
    assert through_image > 0, "the head never felt the tail: the case shows nothing"
    assert np.any(r["g_params"][5, 0, 0] != 0)
