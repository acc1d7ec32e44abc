"""A recorded leader on the two tape-free paths of the micro rollout (dhts_micro_rollout_fwd_ckpt_lead / _bwd_ckpt_lead /
_fwd_jvp_lead, the ops wrappers of the same names, dhts.micro_rollout(lead=, lead_length=) and dhts.micro_rollout_jvp(lead=,
lead_length=, t_lead=)): the boundary of the library -- header, bindings, exports, argument checks, every ValueError, the plans -- and
the validation of the yardstick tests/micro_lead_ref.py::lead_rollout against the C oracle.  What the kernels compute is held against
existing device code in tests/test_micro_lead_gpu.py.  No GPU needed."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from micro_lead_ref import lead_rollout, restated_lead, trajectory_before_steps
from test_micro_params import GOLDENS, golden_case
from util import TOL_GRAD, TOL_STATE, grad_report, rel_elem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dhts_micro_rollout_fwd_ckpt_lead", "dhts_micro_rollout_bwd_ckpt_lead", "dhts_micro_rollout_fwd_jvp_lead")
FWD = ("p", "v", "count", "params", "lead", "lead_length", "p_out", "v_out", "ckpt", "probes", "n_probes", "every", "samples", "err", "stream")
BWD = ("ckpt", "count", "params", "lead", "lead_length", "g_p", "g_v", "probes", "n_probes", "every", "g_samples", "g_p_out", "g_v_out",
       "g_lead", "g_params", "err", "stream")
JVP = ("p", "v", "count", "params", "lead", "lead_length", "t_p", "t_v", "t_lead", "t_params", "p_out", "v_out", "t_p_out", "t_v_out", "probes",
       "n_probes", "every", "samples", "t_samples", "err", "err_jvp", "stream")
REQUIRED = {NEW[0]: ("p", "v", "params", "lead", "p_out", "v_out"),
            NEW[1]: ("ckpt", "params", "lead", "g_p", "g_v", "g_p_out", "g_v_out", "g_lead"),
            NEW[2]: ("p", "v", "params", "lead", "t_p", "t_v", "p_out", "v_out", "t_p_out", "t_v_out")}


def test_header_library_and_bindings_hold_the_new_entry_points():
    import dhts
    from dhts import _lib, ops
    raw = open(os.path.join(ROOT, "include", "dhts.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib.lib()
    for name, names in zip(NEW, (FWD, BWD, JVP)):
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, txt)
        assert m, "include/dhts.h does not declare %s" % name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
        assert len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1 == len(names) + 3, name        # d, T, segment / n_dir first
        declared = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
        assert declared[3:] == list(names), "the header's argument names of %s" % name
        ints = [i for i, t in enumerate(_lib.SIGNATURES[name][1]) if t is C.c_int]
        assert ints == [1, 2, 3 + names.index("n_probes"), 3 + names.index("every")], name
        assert "head" not in names and "t_head" not in names and "g_head" not in names
    comment = raw[raw.index("A RECORDED LEADER on the two tape-free paths"):raw.index("int " + NEW[0])]
    for cited in ("_micro_lane.py:131-214", "dmicro_lane.py:271-298", ":130-153", "DHTS_E_INVALID", "[T][L][2]", "[K][T][L][2]", "exactly 0"):
        assert cited in comment, cited
    for name in ("micro_rollout_fwd_ckpt_lead", "micro_rollout_bwd_ckpt_lead", "micro_rollout_fwd_jvp_lead", "MicroRolloutLead"):
        assert callable(getattr(ops, name))
    assert dhts.MicroRolloutLead is ops.MicroRolloutLead
    par = inspect.signature(dhts.micro_rollout).parameters
    assert par["lead"].default is None and par["lead_length"].default is None
    par = inspect.signature(dhts.micro_rollout_jvp).parameters
    assert par["lead"].default is None and par["lead_length"].default is None and par["t_lead"].default is None
    assert list(inspect.signature(ops.MicroRollout.forward).parameters)[-1] == "checkpoint", "the existing operators keep their signatures"
    assert list(inspect.signature(ops.MicroRolloutSamples.forward).parameters)[-1] == "every"


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
    for name, names in zip(NEW, (FWD, BWD, JVP)):
        fn = getattr(lib, name)
        for missing in REQUIRED[name]:
            assert fn(C.byref(ok), 5, 1, *call_args(names, some, **{missing: None})) == _lib.E_INVALID, (name, missing)
        for bad in (_lib.MicroDesc(4, 5000, 0.01), _lib.MicroDesc(0, 70, 0.01), _lib.MicroDesc(4, 70, 0.0)):
            assert fn(C.byref(bad), 5, 1, *call_args(names, some)) == _lib.E_INVALID
        assert fn(C.byref(ok), -1, 1, *call_args(names, some)) == _lib.E_INVALID
        assert fn(C.byref(ok), 5, 1, *call_args(names, some, every=0)) == _lib.E_INVALID
        assert fn(C.byref(ok), 5, 1, *call_args(names, some, n_probes=0)) == _lib.E_INVALID
        assert fn(C.byref(ok), 5, 1, *call_args(names, some, n_probes=71)) == _lib.E_INVALID
    # a segment the reverse kernel's ring cannot hold: the plan of the siblings holds for the lead forms
    plan = (C.c_int32 * 8)()
    for want_params, g_params in ((0, None), (1, some)):
        assert lib.dhts_micro_ckpt_plan(C.byref(ok), 5, want_params, 0, C.byref(plan)) == 0
        too_long = plan[2] + 1
        assert lib.dhts_micro_rollout_bwd_ckpt_lead(C.byref(ok), 5, too_long, *call_args(BWD, some, g_params=g_params)) == _lib.E_INVALID
    assert lib.dhts_micro_ckpt_plan(C.byref(ok), 5, 0, 0, C.byref(plan)) == 0
    assert lib.dhts_micro_rollout_fwd_ckpt_lead(C.byref(ok), 5, plan[2] + 1, *call_args(FWD, some)) == _lib.E_INVALID
    # the fused kernel's sample arrays: both or neither
    assert lib.dhts_micro_rollout_fwd_jvp_lead(C.byref(ok), 5, 1, *call_args(JVP, some, samples=None)) == _lib.E_INVALID
    assert lib.dhts_micro_rollout_fwd_jvp_lead(C.byref(ok), 5, 1, *call_args(JVP, some, t_samples=None)) == _lib.E_INVALID
    assert lib.dhts_micro_rollout_fwd_jvp_lead(C.byref(ok), 5, 0, *call_args(JVP, some)) == _lib.E_INVALID       # n_dir < 1


def test_every_value_error_is_raised_before_a_device_is_touched():
    """CPU tensors throughout: a call that reached a kernel wrapper would raise TypeError (not a CUDA tensor), not ValueError."""
    import torch
    import dhts
    L, V, T, dt = 2, 5, 4, 0.1
    p0, v0 = torch.zeros(L, V), torch.zeros(L, V)
    params = torch.ones(6, L, V, dtype=torch.float64)
    head = torch.zeros(L, 2, dtype=torch.float64)
    lead = torch.zeros(T, L, 2)
    with pytest.raises(ValueError, match="checkpoint=True"):
        dhts.micro_rollout(p0, v0, params, None, T, dt, lead=lead)
    with pytest.raises(ValueError, match="checkpoint=True"):
        dhts.micro_rollout(p0, v0, params, None, T, dt, lead=lead, checkpoint=False, probes=[0], every=2)
    with pytest.raises(ValueError, match="every=1"):
        dhts.micro_rollout(p0, v0, params, None, T, dt, lead=lead, checkpoint=True, want_hist=True)
    with pytest.raises(ValueError, match="head must be None"):
        dhts.micro_rollout(p0, v0, params, head, T, dt, lead=lead, checkpoint=True)
    with pytest.raises(ValueError, match="lead_length needs lead"):
        dhts.micro_rollout(p0, v0, params, head, T, dt, lead_length=torch.ones(L, dtype=torch.float64), checkpoint=True)
    for bad in (torch.zeros(T + 1, L, 2), torch.zeros(T, L, 2, dtype=torch.float64), torch.zeros(T, L), np.zeros((T, L, 2), np.float32)):
        with pytest.raises(ValueError, match="lead must be a float32 tensor"):
            dhts.micro_rollout(p0, v0, params, None, T, dt, lead=bad, checkpoint=True)
        with pytest.raises(ValueError, match="lead must be a float32 tensor"):
            dhts.micro_rollout_jvp(p0, v0, params, None, T, dt, t_p0=torch.zeros(1, L, V), lead=bad, fused=True)
    for bad in (torch.ones(L), torch.ones(L + 1, dtype=torch.float64)):
        with pytest.raises(ValueError, match="lead_length must be None or a float64"):
            dhts.micro_rollout(p0, v0, params, None, T, dt, lead=lead, lead_length=bad, checkpoint=True)
        with pytest.raises(ValueError, match="lead_length must be None or a float64"):
            dhts.micro_rollout_jvp(p0, v0, params, None, T, dt, t_p0=torch.zeros(1, L, V), lead=lead, lead_length=bad, fused=True)
    with pytest.raises(ValueError, match="not differentiable"):
        dhts.micro_rollout(p0, v0, params, None, T, dt, lead=lead, lead_length=torch.ones(L, dtype=torch.float64, requires_grad=True),
                           checkpoint=True)
    with pytest.raises(ValueError, match="checkpoint must be"):
        dhts.micro_rollout(p0, v0, params, None, T, dt, lead=lead, checkpoint=-2)
    with pytest.raises(ValueError, match="segment must be"):
        dhts.micro_rollout(p0, v0, params, None, T, dt, lead=lead, checkpoint=10 ** 6)
    with pytest.raises(ValueError, match="every must be"):
        dhts.micro_rollout(p0, v0, params, None, T, dt, lead=lead, checkpoint=True, every=0)
    with pytest.raises(ValueError, match="strictly ascending"):
        dhts.micro_rollout(p0, v0, params, None, T, dt, lead=lead, checkpoint=True, probes=[1, 0])
    # forward mode
    t_p0 = torch.zeros(3, L, V)
    with pytest.raises(ValueError, match="fused=True"):
        dhts.micro_rollout_jvp(p0, v0, params, None, T, dt, t_p0=t_p0, lead=lead)
    with pytest.raises(ValueError, match="need lead"):
        dhts.micro_rollout_jvp(p0, v0, params, head, T, dt, t_p0=t_p0, t_lead=torch.zeros(3, T, L, 2), fused=True)
    with pytest.raises(ValueError, match="t_head must be None"):
        dhts.micro_rollout_jvp(p0, v0, params, None, T, dt, t_p0=t_p0, t_head=torch.zeros(3, L, 2, dtype=torch.float64), lead=lead, fused=True)
    with pytest.raises(ValueError, match="head and t_head must be None"):
        dhts.micro_rollout_jvp(p0, v0, params, head, T, dt, t_p0=t_p0, lead=lead, fused=True)
    with pytest.raises(ValueError, match="every=1"):
        dhts.micro_rollout_jvp(p0, v0, params, None, T, dt, t_p0=t_p0, lead=lead, fused=True, want_hist=True)
    with pytest.raises(ValueError, match="t_lead must have shape"):
        dhts.micro_rollout_jvp(p0, v0, params, None, T, dt, t_p0=t_p0, t_lead=torch.zeros(3, T + 1, L, 2), lead=lead, fused=True)
    with pytest.raises(ValueError, match="t_lead must have shape"):
        dhts.micro_rollout_jvp(p0, v0, params, None, T, dt, t_p0=t_p0, t_lead=torch.zeros(2, T, L, 2), lead=lead, fused=True)
    with pytest.raises(ValueError, match="at least one of"):
        dhts.micro_rollout_jvp(p0, v0, params, None, T, dt, lead=lead, fused=True)


@pytest.mark.parametrize("L,V,T", [(3, 1, 3), (3, 70, 50), (5, 130, 50), (3, 1024, 20)])
def test_both_plans_are_the_siblings(L, V, T):
    """The lead forms launch on dhts_micro_ckpt_plan and dhts_micro_fwd_jvp_plan as they stand: the block, the segment, the dynamic LDS
    sizes are the documented functions of the shape alone (include/dhts.h), with no term for a leader -- its state travels in slot V of
    the hand-over arrays, which the layouts already hold."""
    from dhts import ops
    desc = ops.micro_desc(L, V, 0.01)
    Vp = (V + 63) // 64 * 64
    for want_params in (False, True):
        pl = ops.micro_ckpt_plan(desc, T, want_params)
        S = pl["segment"]
        assert pl["block"] == Vp and pl["fwd_lds_bytes"] == 8 * 2 * (V + 1)
        assert pl["bwd_lds_bytes"] == 8 * 2 * (V + 1) + 4 * 4 * (V + 2) + S * (12 * V + (8 * (V + 1) if want_params else 0))
        assert pl["checkpoints"] == (T + S - 1) // S
        assert pl["max_segment"] == (160 * 1024 - 8 * 2 * (V + 1) - 4 * 4 * (V + 2)) // (12 * V + (8 * (V + 1) if want_params else 0))
        for K in (1, 4, 5):
            pj = ops.micro_fwd_jvp_plan(desc, T, K, want_params)
            widest = min(4, 1 if K == 1 else 4)
            assert pj["block"] == Vp and pj["dirs_per_launch"] == widest, pj
            assert pj["lds_bytes"] == 8 * (2 + 2 * widest) * (V + 1) + 16 * widest


def test_resource_listing_keeps_every_existing_kernel():
    """profiles/micro_lead_resources_parent.txt against profiles/micro_lead_resources.txt (compiler output for gfx950, one line per
    kernel): every kernel of the parent has identical figures -- the nine sampled ones under the name their new template parameter
    gives them, kLead = false --, and the new lines are the nine kLead = true forms, none with scratch or a spill."""
    def read(name):
        rows = {}
        for line in open(os.path.join(ROOT, "profiles", name)).read().splitlines():
            kernel, figures = line.split(" SGPRs ")
            rows[kernel.strip()] = "SGPRs " + " ".join(figures.split())
        return rows
    parent, new = read("micro_lead_resources_parent.txt"), read("micro_lead_resources.txt")

    def renamed(k):
        if k == "dhts::micro_rollout_ckpt_fwd_samples_kernel":
            return "micro_rollout_ckpt_fwd_samples_kernel<false>"
        if k.startswith(("micro_rollout_ckpt_bwd_samples_kernel<", "micro_rollout_fwd_jvp_samples_kernel<")):
            return k[:-1] + ", false>"
        return k
    assert len(parent) == 122
    for k, figures in parent.items():
        assert new.get(renamed(k)) == figures, k
    added = sorted(set(new) - {renamed(k) for k in parent})
    assert len(added) == 9 and all(k.endswith("true>") and "_samples_kernel<" in k for k in added), added
    for k in added:
        assert " scratch 0 " in new[k] and " sgpr_spill 0 vgpr_spill 0 " in new[k], (k, new[k])


# =================================================================================================================
# the yardstick, validated twice
# =================================================================================================================
def moving_leader(rng, p_head, T, dt):
    """A leader some way in front of the head that speeds up and slows down: [T][2] float32."""
    v = np.clip(8.0 + np.cumsum(rng.normal(0.0, 1.5, T)), 0.5, 25.0)
    p = p_head + 25.0 + np.concatenate([[0.0], np.cumsum(v[:-1] * dt)])
    return np.stack([p, v], 1).astype(np.float32)


@pytest.mark.parametrize("name", GOLDENS)
@pytest.mark.parametrize("own_length", (False, True))
def test_lead_rollout_against_a_chain_of_oracle_steps(golden_dir, oracle, name, own_length):
    """(a) T single oracle.micro_step calls on n + 1 slots, slot n overwritten with lead[t] before every step: the followers' states
    after every step, and the cotangents through oracle.micro_step_bwd (slot n's output takes none: it is not part of lead)."""
    c = golden_case(golden_dir, name)
    g, dt = c["g"], c["dt"]
    T = min(c["T"], 60)
    n = c["p0"].shape[1]
    rng = np.random.default_rng(11)
    lead = moving_leader(rng, float(c["p0"][0, -1]), T, dt)
    len_lead = float(g["params"][-1, 5]) if own_length else 6.5
    par1 = np.concatenate([g["params"], g["params"][-1:]], 0).copy()      # [n + 1][6]
    par1[n, 5] = len_lead
    p, v = np.append(c["p0"][0], 0).astype(np.float32), np.append(c["v0"][0], 0).astype(np.float32)
    hist, tapes = [], []
    for t in range(T):
        p[n], v[n] = lead[t]
        o = oracle.micro_step(p, v, par1, 1000.0, 0.0, dt)
        assert o["rc"] == 0
        p, v = o["np"].copy(), o["nv"].copy()
        hist.append(np.stack([p[:n], v[:n]]))
        tapes.append(o["dqs"])
    hist = np.stack(hist)[:, None]                                          # [T][1][2][n]
    g_pT, g_vT = rng.normal(size=(1, n)).astype(np.float32), rng.normal(size=(1, n)).astype(np.float32)
    g_hist = (0.1 * rng.normal(size=hist.shape)).astype(np.float32)
    gp, gv = np.append(g_pT[0], 0).astype(np.float32), np.append(g_vT[0], 0).astype(np.float32)
    g_lead = np.zeros((T, 1, 2), np.float32)
    for t in reversed(range(T)):
        gp[:n] += g_hist[t, 0, 0]
        gv[:n] += g_hist[t, 0, 1]
        ip, iv = oracle.micro_step_bwd(tapes[t], gp, gv)
        g_lead[t, 0] = ip[n], iv[n]
        gp, gv = np.append(ip[:n], 0).astype(np.float32), np.append(iv[:n], 0).astype(np.float32)
    r = restated_lead(c["p0"], c["v0"], c["params"], lead[:, None], T, dt, lead_length=None if own_length else [len_lead], g_pT=g_pT,
                      g_vT=g_vT, g_hist=g_hist)
    e_s = rel_elem(r["hist"], hist)
    print("%s own_length=%s: lead_rollout vs oracle chain, states %.2e" % (name, own_length, e_s))
    assert e_s <= TOL_STATE
    assert rel_elem(r["pT"], hist[-1][:, 0]) <= TOL_STATE and rel_elem(r["vT"], hist[-1][:, 1]) <= TOL_STATE
    assert grad_report("%s lead_rollout vs oracle chain d loss / d p0" % name, r["g_p0"][0], gp[:n]) <= TOL_GRAD
    assert grad_report("%s lead_rollout vs oracle chain d loss / d v0" % name, r["g_v0"][0], gv[:n]) <= TOL_GRAD
    assert grad_report("%s lead_rollout vs oracle chain d loss / d lead" % name, r["g_lead"], g_lead) <= TOL_GRAD
    assert np.any(g_lead != 0)


@pytest.mark.parametrize("name", GOLDENS)
def test_lead_rollout_reproduces_a_rollout_split_at_a_vehicle(golden_dir, oracle, name):
    """(b) The oracle's full rollout with its history; vehicle j's trajectory as lead, its length as lead_length: vehicles 0 .. j - 1 of
    lead_rollout are those of the full rollout, after every step."""
    import torch
    c = golden_case(golden_dir, name)
    g, T, dt = c["g"], c["T"], c["dt"]
    n = c["p0"].shape[1]
    f = oracle.micro_rollout_fwd(c["p0"], c["v0"], g["params"][None], T, dt, head_dp=c["head"][0, 0], head_dv=c["head"][0, 1],
                                 want_tape=False, want_hist=True)
    assert f["rc"] == 0
    for j in sorted({1, n // 2, n - 1}):
        lead = np.stack([trajectory_before_steps(c["p0"][:, j], f["hist_p"][:, :, j]),
                         trajectory_before_steps(c["v0"][:, j], f["hist_v"][:, :, j])], -1).astype(np.float32)      # [T][1][2]
        pT, vT, hist = lead_rollout(torch.tensor(c["p0"][:, :j]), torch.tensor(c["v0"][:, :j]), torch.tensor(c["params"][:, :, :j]),
                                    torch.tensor(lead), T, dt, lead_length=c["params"][5, :, j])
        e_p, e_v = rel_elem(hist[:, :, 0].numpy(), f["hist_p"][:, :, :j]), rel_elem(hist[:, :, 1].numpy(), f["hist_v"][:, :, :j])
        print("%s split at %d of %d: p %.2e v %.2e" % (name, j, n, e_p, e_v))
        assert max(e_p, e_v) <= TOL_STATE
        assert rel_elem(pT.numpy(), f["pT"][:, :j]) <= TOL_STATE and rel_elem(vT.numpy(), f["vT"][:, :j]) <= TOL_STATE
