"""Every public form of dhts.macro_rollout and dhts.micro_rollout against the same computation driven by hand through the raw wrappers
(ops.macro_rollout_fwd_ckpt* / _bwd_ckpt*, ops.micro_rollout_fwd_ckpt* / _bwd_ckpt*, the taped ones) and the glue operators
(macro_state_from_ru, macro_state_from_ru_bwd, macro_u_tap_bwd, _per_step_cotangent, _ghost_ry_to_ru, cut_samples): every output and every
leaf gradient under .backward() bit for bit (torch.equal, no tolerance), and beside them what each form's autograd Function guarantees --
the tuple it returns, the leaves that get a gradient with dtype and shape, whether a call without a leaf that requires grad hands the raw
layer a checkpoint buffer, whether the context is released by backward (a second backward over a retained graph), and what backward
leaves allocated.  Where the forms differ in one of these, each is held to its own.

The shapes are the smallest at which the bookkeeping of a form can go wrong.  Macro: L = 2 lanes of N = 6 cells, T = 5 steps at a segment
of 2 (three segments, the last one short), detectors at both ends, ramps beside both ends, the staircase of tests/macro_ramp_ref.py at
the ramp cells.  Micro: L = 2 lanes of V = 5 slots with 5 and 3 vehicles, T = 5 at a segment of 2, probes at slots 0 and 4 every 2 steps
(the fifth step gives no row), the stop wave, the braking leader and the jammed ring of tests/micro_jam_cases.py.  One T = 0 case each."""
import collections
import functools

import numpy as np
import pytest

import macro_ramp_ref as R
import micro_jam_cases as J

pytestmark = pytest.mark.gpu

L, T, S = 2, 5, 2
N, DET, RAMPS = 6, [0, 5], [1, 4]
V, COUNT, PROBES, EVERY, MICRO_DT = 5, [5, 3], [0, 4], 2, 0.1
DT, DX, UM = R.DT, R.DX, R.UM
F = np.float32


def blk(n_bytes):
    """What torch's caching allocator accounts for a small tensor: its bytes rounded up to 512."""
    return -(-int(n_bytes) // 512) * 512 if n_bytes else 0


def weighted(out, w):
    """sum_k <w_k, out_k>."""
    return sum((o * g).sum().double() for o, g in zip(out, w))


def same(a, b, what):
    import torch
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), what


def backward_into_zeros(loss, leaves, retain=True):
    """loss.backward() into gradients that exist already -> the change of torch.cuda.memory_allocated() across it."""
    import torch
    for t in leaves:
        if t is not None and t.requires_grad and t.grad is None:
            t.grad = torch.zeros_like(t)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    loss.backward(retain_graph=retain)
    torch.cuda.synchronize()
    return torch.cuda.memory_allocated() - before


@pytest.fixture
def handed(monkeypatch):
    """One entry per checkpointed forward the raw layer runs: whether it was handed a checkpoint buffer (True) or None (False)."""
    from dhts import ops
    seen = []
    for name, at in (("_macro_ckpt_fwd", 8), ("_micro_ckpt_fwd", 6)):
        def spy(*a, _raw=getattr(ops, name), _at=at, **kw):
            seen.append((kw["ckpt"] if "ckpt" in kw else a[_at]) is not None)
            return _raw(*a, **kw)
        monkeypatch.setattr(ops, name, spy)
    return seen


# =================================================================================================================
# macro
# =================================================================================================================
MacroCase = collections.namedtuple("MacroCase", "r u gr gu inflow target w")
MACRO_BOUNDS, MACRO_OBS = ("const", "sched", "ring"), (None, "detectors", "target")
MACRO_FORMS = [(b, o, ramp) for b in MACRO_BOUNDS for o in MACRO_OBS for ramp in (False, True)]


@functools.lru_cache(None)
def macro_case(bound, steps=T):
    r, u = (a[:L].copy() for a in R.case_state(N, RAMPS))
    gr, gu = R.case_bounds(bound, steps)
    if gr is not None:
        gr, gu = (np.ascontiguousarray(a[..., :L, :]) for a in (gr, gu))
    rng = np.random.default_rng(5)
    w = {None: [rng.standard_normal((L, N)).astype(F) for _ in range(3)]}
    w["detectors"] = w[None] + [rng.standard_normal((steps, L, 3, len(DET))).astype(F)]
    w["hist"] = w[None] + [rng.standard_normal((steps, L, 3, N)).astype(F)]
    w["target"] = w[None] + [rng.standard_normal((L, 2))]
    return MacroCase(r, u, gr, gu, R.ramp_inflow(steps, L, len(RAMPS), DT, seed=N + steps),
                     np.ascontiguousarray(R.case_target(N, RAMPS, steps)[:, :L]), w)


def macro_class(bound, obs, ramp):
    if ramp:
        return "MacroRolloutRamp"
    fit = obs == "target"
    return ("MacroRolloutRingTarget" if fit else "MacroRolloutRing") if bound == "ring" else ("MacroRolloutTarget" if fit else "MacroRollout")


def macro_leaves(cuda, c, ramp, grad=True):
    import torch
    t = lambda a: None if a is None else torch.tensor(a, device=cuda, requires_grad=grad)      # noqa: E731
    return dict(r0=t(c.r), u0=t(c.u), ghost_r=t(c.gr), ghost_u=t(c.gu), inflow=t(c.inflow) if ramp else None)


def macro_api(cuda, x, c, obs, ramp, steps=T, checkpoint=S, want_hist=False):
    import torch
    import dhts
    kw = dict(checkpoint=checkpoint, ring=x["ghost_r"] is None, want_hist=want_hist)
    if ramp:
        kw.update(ramps=RAMPS, inflow=x["inflow"])
    if obs == "detectors":
        kw["detectors"] = DET
    if obs == "target":
        kw["target"] = torch.tensor(c.target, device=cuda)
    return dhts.macro_rollout(x["r0"], x["u0"], x["ghost_r"], x["ghost_u"], steps, DT, DX, UM, **kw)


def macro_by_hand(cuda, x, c, obs, ramp, w, steps=T, taped=False, want_hist=False):
    """The form through the raw wrappers and the glue -> (outputs, dict of the leaves' gradients)."""
    import torch
    from dhts import ops
    i32 = lambda cells: torch.tensor(cells, dtype=torch.int32, device=cuda)      # noqa: E731
    r0, u0 = x["r0"].detach(), x["u0"].detach()
    ring, fit = x["ghost_r"] is None, obs == "target"
    desc = ops.macro_desc(L, N, DT, DX, UM)
    y0, q0 = ops.macro_state_from_ru(r0, u0, UM)
    state = (r0, y0, u0, q0)
    gr = gu = gq = ghost = g_ghost = None
    if not ring:
        gr, gu = x["ghost_r"].detach(), x["ghost_u"].detach()
        gy, gq = ops.macro_state_from_ru(gr, gu, UM) if gr.numel() else (gr.clone(), gr.clone())
        ghost = torch.stack([gr, gy, gu, gq], dim=-1).contiguous()
    sched = ghost is not None and ghost.dim() == 4
    det = i32(DET) if obs == "detectors" else None
    tgt = torch.tensor(c.target, device=cuda) if fit else None
    if taped:
        tape = torch.empty(ops.macro_tape_numel(desc, steps), dtype=torch.float32, device=cuda)
        if det is not None:
            out, extra = ops.macro_rollout_fwd_taps(desc, steps, *state, ghost, det, tape=tape)
        else:
            extra = torch.empty(steps, L, 3, N, dtype=torch.float32, device=cuda) if want_hist else None
            out = (ops.macro_rollout_fwd_sched if sched else ops.macro_rollout_fwd)(desc, steps, *state, ghost, tape=tape, hist=extra)
    else:
        plan = ops.macro_ckpt_target_plan(desc, steps, S) if fit else ops.macro_ckpt_plan(desc, steps, 0 if det is None else len(DET), S)
        seg = plan["segment"]
        ckpt = torch.empty(ops.macro_ckpt_numel(desc, steps, seg), dtype=torch.float32, device=cuda)
        if ramp:
            ramps, inflow = i32(RAMPS), x["inflow"].detach()
            out, extra = ops.macro_rollout_fwd_ckpt_ramp(desc, steps, *state, ghost, ckpt, ramps, inflow, segment=seg, det=det, target=tgt)
        elif ring and fit:
            out, extra = ops.macro_rollout_fwd_ckpt_target_ring(desc, steps, *state, ckpt, tgt, segment=seg)
        elif ring:
            out, extra = ops.macro_rollout_fwd_ckpt_ring(desc, steps, *state, ckpt, segment=seg, det=det)
        elif fit:
            out, extra = ops.macro_rollout_fwd_ckpt_target(desc, steps, *state, ghost, ckpt, tgt, segment=seg)
        else:
            out, extra = ops.macro_rollout_fwd_ckpt(desc, steps, *state, ghost, ckpt, segment=seg, det=det)
    rT, yT, uT, qT = out
    g_r, g_y = w[0].clone(), w[1].clone()
    ops.macro_u_tap_bwd(rT, yT, w[2], g_r, g_y, UM)
    gs = g_sse = final = None
    if fit:
        g_sse, final = w[3], (rT, yT, uT)
    elif extra is not None and extra.numel():
        gs = ops._per_step_cotangent(extra, w[3], UM)
    taps = dict(det=det if gs is not None else None, g_taps=gs)
    if taped and gs is not None and det is not None:
        g_r0, g_y0, g_ghost = ops.macro_rollout_bwd_taps(desc, steps, tape, g_r, g_y, det, gs, sched=sched)
    elif taped:
        g_r0, g_y0, g_ghost = (ops.macro_rollout_bwd_sched if sched else ops.macro_rollout_bwd)(desc, steps, tape, g_r, g_y, g_hist=gs)
    elif ramp:
        g_r0, g_y0, g_ghost, g_inflow = ops.macro_rollout_bwd_ckpt_ramp(desc, steps, ckpt, *state, ghost, g_r, g_y, ramps, inflow, segment=seg,
                                                                        target=tgt, g_sse=g_sse, final=final, **taps)
    elif ring and fit:
        g_r0, g_y0 = ops.macro_rollout_bwd_ckpt_target_ring(desc, steps, ckpt, *state, g_r, g_y, tgt, g_sse=g_sse, final=final, segment=seg)
    elif ring:
        g_r0, g_y0 = ops.macro_rollout_bwd_ckpt_ring(desc, steps, ckpt, *state, g_r, g_y, segment=seg, **taps)
    elif fit:
        g_r0, g_y0, g_ghost = ops.macro_rollout_bwd_ckpt_target(desc, steps, ckpt, *state, ghost, g_r, g_y, tgt, g_sse=g_sse, final=final,
                                                                segment=seg)
    else:
        g_r0, g_y0, g_ghost = ops.macro_rollout_bwd_ckpt(desc, steps, ckpt, *state, ghost, g_r, g_y, segment=seg, **taps)
    g_u0 = ops.macro_state_from_ru_bwd(r0, u0, g_y0, g_r0, UM)                 # (g_r0 is completed in place)
    grads = dict(r0=g_r0, u0=g_u0, ghost_r=None, ghost_u=None, inflow=g_inflow if ramp else None)
    if not ring:
        grads["ghost_r"], grads["ghost_u"] = ops._ghost_ry_to_ru(g_ghost, gr, gu, gq, UM)
    return (rT, yT, uT, qT) + (() if extra is None else (extra,)), grads


def macro_held(cuda, bound, obs, ramp, steps=T, checkpoint=S, want_hist=False):
    """One form: the public call and its backward against macro_by_hand, and the tuple, dtypes and shapes the form promises."""
    import torch
    c = macro_case(bound, steps)
    w = [torch.tensor(a, device=cuda) for a in c.w["hist" if want_hist else obs]]
    x = macro_leaves(cuda, c, ramp)
    out = macro_api(cuda, x, c, obs, ramp, steps, checkpoint, want_hist)
    weighted(out[:3] + out[4:], w).backward()        # (the fourth output, the equilibrium speed, is not differentiable)
    want, g = macro_by_hand(cuda, x, c, obs, ramp, w, steps, taped=checkpoint is None, want_hist=want_hist)
    tag = (bound, obs, ramp, steps, checkpoint, want_hist)
    assert out[0].grad_fn.name() == macro_class(bound, obs, ramp) + "Backward", tag
    assert len(out) == len(want) == (4 if obs is None and not want_hist else 5), tag
    for k, (a, b) in enumerate(zip(out, want)):
        same(a.detach(), b, tag + ("output", k))
    assert all(o.dtype == torch.float32 and tuple(o.shape) == (L, N) for o in out[:4]) and not out[3].requires_grad, tag
    if len(out) == 5:
        shape = {None: (steps, L, 3, N), "detectors": (steps, L, 3, len(DET)), "target": (L, 2)}[obs]
        assert out[4].dtype == (torch.float64 if obs == "target" else torch.float32) and tuple(out[4].shape) == shape, tag
    for k, leaf in x.items():
        same(None if leaf is None else leaf.grad, g[k], tag + ("gradient", k))
        assert leaf is None or (leaf.grad.dtype == torch.float32 and leaf.grad.shape == leaf.shape), tag
    if ramp:
        assert tuple(x["inflow"].grad.shape) == (steps, L, len(RAMPS)), tag
    if bound == "sched":
        assert tuple(x["ghost_r"].grad.shape) == tuple(x["ghost_u"].grad.shape) == (steps, L, 2), tag


@pytest.mark.parametrize("bound,obs,ramp", MACRO_FORMS)
def test_macro_checkpointed_forms_are_the_raw_wrappers_and_the_glue(cuda, bound, obs, ramp):
    macro_held(cuda, bound, obs, ramp)


@pytest.mark.parametrize("bound", ("const", "sched"))
@pytest.mark.parametrize("obs,want_hist", [(None, False), (None, True), ("detectors", False)])
def test_macro_taped_forms_are_the_raw_wrappers_and_the_glue(cuda, bound, obs, want_hist):
    macro_held(cuda, bound, obs, False, checkpoint=None, want_hist=want_hist)


def test_macro_without_a_step(cuda):
    """T = 0 with a schedule, detectors and ramps: no row of anything, and the state goes through."""
    macro_held(cuda, "sched", "detectors", True, steps=0)
    macro_held(cuda, "ring", "target", False, steps=0)


@pytest.mark.parametrize("bound,obs,ramp", MACRO_FORMS)
def test_macro_checkpoint_without_grad(cuda, handed, bound, obs, ramp):
    """Without a leaf that requires grad: MacroRollout runs the taped kernels without a tape (no checkpointed forward at all), the two
    target Functions run theirs without a checkpoint, MacroRolloutRing and every form of MacroRolloutRamp allocate one all the same.
    With one, every form keeps a checkpoint."""
    import torch
    c = macro_case(bound)
    cls = macro_class(bound, obs, ramp)
    out = macro_api(cuda, macro_leaves(cuda, c, ramp, grad=False), c, obs, ramp)
    assert not any(o.requires_grad for o in out)
    want = {"MacroRollout": [], "MacroRolloutTarget": [False], "MacroRolloutRingTarget": [False], "MacroRolloutRing": [True],
            "MacroRolloutRamp": [True]}[cls]
    assert handed == want, (cls, handed)
    del handed[:]
    with_grad = macro_api(cuda, macro_leaves(cuda, c, ramp), c, obs, ramp)
    assert handed == [True], (cls, handed)
    for a, b in zip(out, with_grad):
        assert torch.equal(a, b.detach())


@pytest.mark.parametrize("bound,obs,ramp", MACRO_FORMS)
def test_macro_backward_and_the_context(cuda, bound, obs, ramp):
    """A backward over a retained graph into gradients that exist already.  MacroRollout's checkpointed branch keeps its context: nothing
    stays allocated, nothing is released, and a second backward returns the same bits.  The four other Functions release the checkpoint
    buffer and the replay inputs (y0, q0 and, on an open lane, the boundary block) -- exactly those leave the allocator's count, so
    nothing a backward makes stays -- and a second backward finds no context."""
    import torch
    from dhts import ops
    c = macro_case(bound)
    w = [torch.tensor(a, device=cuda) for a in c.w[obs]]
    cls = macro_class(bound, obs, ramp)

    def run():
        x = macro_leaves(cuda, c, ramp)
        out = macro_api(cuda, x, c, obs, ramp)
        return x, weighted(out[:3] + out[4:], w)
    run()[1].backward()                      # (whatever a first backward of the process sets up is there)
    x, loss = run()
    leaves = [t for t in x.values() if t is not None]
    change = backward_into_zeros(loss, leaves)
    first = [t.grad.clone() for t in leaves]
    if cls == "MacroRollout":
        assert change == 0, (cls, change)
        assert backward_into_zeros(loss, leaves) == 0
        for t, g in zip(leaves, first):
            assert torch.equal(t.grad, g + g)
        return
    desc = ops.macro_desc(L, N, DT, DX, UM)
    plan = ops.macro_ckpt_target_plan(desc, T, S) if obs == "target" else ops.macro_ckpt_plan(desc, T, len(DET) if obs else 0, S)
    ghost = 0 if bound == "ring" else (T if bound == "sched" else 1) * L * 2 * 4 * 4
    released = blk(4 * ops.macro_ckpt_numel(desc, T, plan["segment"])) + 2 * blk(4 * L * N) + blk(ghost)
    assert change == -released, (cls, change, released)
    with pytest.raises(TypeError):
        loss.backward()


# =================================================================================================================
# micro
# =================================================================================================================
MICRO_KINDS = ("head", "lead", "lead_length", "ring")
MICRO_FORMS = [(k, o) for k in MICRO_KINDS for o in (None, "hist", "probes", "target") if o != "hist" or k == "head"]


@functools.lru_cache(None)
def micro_case(kind, steps=T):
    """The builder's lanes with 5 and 3 vehicles (its own counts are 5 and 0): the ring's circumference and the leader's start are set for
    the second lane as the builder sets them for the first."""
    build = {"head": J.stop_wave, "lead": J.braking_leader, "ring": functools.partial(J.jammed_ring, pull=True)}[kind]
    c = build(3, L, V, steps, MICRO_DT)
    b = np.array(c.boundary)
    last = COUNT[1] - 1
    if kind == "ring":
        b[1] = float(c.p0[1, last]) - float(c.p0[1, 0]) + 0.5 * (c.params[5, 1, 0] + c.params[5, 1, last]) + 8.0
    if kind == "lead":
        b[:, 1, 0] += F(float(c.p0[1, last]) + 25.0 - 10.0)
    c = c._replace(boundary=b, count=COUNT)
    rng = np.random.default_rng(9)
    live = J.live_mask(c)
    w = {None: [(rng.standard_normal((L, V)) * live).astype(F) for _ in range(2)]}
    w["hist"] = w[None] + [(rng.standard_normal((steps, L, 2, V)) * live[None, :, None, :]).astype(F)]
    w["probes"] = w[None] + [rng.standard_normal((steps // EVERY, L, 2, len(PROBES))).astype(F)]
    w["target"] = w[None] + [rng.standard_normal((L, 2))]
    tg = np.stack([c.p0[None] + rng.uniform(0, 5, (steps, L, V)), c.v0[None] + rng.uniform(-2, 2, (steps, L, V))], axis=2).astype(F)
    tg[rng.uniform(size=tg.shape) < 0.2] = np.nan
    return c, w, tg, np.array([4.5, 5.5])


def micro_class(kind, obs):
    if obs == "target":
        return "MicroRolloutRingTarget" if kind == "ring" else "MicroRolloutTarget"
    if kind == "head":
        return "MicroRolloutSamples" if obs == "probes" else "MicroRollout"
    return "MicroRolloutRing" if kind == "ring" else "MicroRolloutLead"


def micro_leaves(cuda, c, kind, grad=True, want_params=True):
    import torch
    t = lambda a, dt, g: torch.tensor(np.asarray(a), dtype=dt, device=cuda, requires_grad=g)      # noqa: E731
    b = t(c.boundary, torch.float32, grad) if kind.startswith("lead") else t(c.boundary, torch.float64, grad and kind == "head")
    return dict(p0=t(c.p0, torch.float32, grad), v0=t(c.v0, torch.float32, grad), params=t(c.params, torch.float64, grad and want_params),
                boundary=b)


def micro_extras(cuda, kind, tg, ll):
    import torch
    return (torch.tensor(COUNT, dtype=torch.int32, device=cuda), torch.tensor(tg, device=cuda),
            torch.tensor(ll, device=cuda) if kind == "lead_length" else None)


def micro_api(cuda, x, kind, obs, steps=T, checkpoint=S):
    import dhts
    c, _, tg, ll = micro_case(kind.split("_")[0], steps)
    cnt, tg, ll = micro_extras(cuda, kind, tg, ll)
    kw = dict(count=cnt, checkpoint=checkpoint, want_hist=obs == "hist")
    if obs == "probes":
        kw.update(probes=PROBES, every=EVERY)
    if obs == "target":
        kw["target"] = tg
    if kind == "head":
        return dhts.micro_rollout(x["p0"], x["v0"], x["params"], x["boundary"], steps, MICRO_DT, **kw)
    if kind == "ring":
        kw.update(ring=x["boundary"])
    else:
        kw.update(lead=x["boundary"], lead_length=ll)
    return dhts.micro_rollout(x["p0"], x["v0"], x["params"], None, steps, MICRO_DT, **kw)


def micro_by_hand(cuda, x, kind, obs, w, steps=T, taped=False):
    """The form through the raw wrappers (the sampled taped form: the history, cut) -> (outputs, dict of the leaves' gradients)."""
    import torch
    from dhts import ops
    c, _, tg, ll = micro_case(kind.split("_")[0], steps)
    cnt, tg, ll = micro_extras(cuda, kind, tg, ll)
    p0, v0, par, b = (x[k].detach() for k in ("p0", "v0", "params", "boundary"))
    want_params = x["params"].requires_grad
    desc = ops.micro_desc(L, V, MICRO_DT)
    g_params = torch.empty(6, L, V, dtype=torch.float64, device=cuda) if want_params else None
    probes = torch.tensor(PROBES, dtype=torch.int32, device=cuda) if obs == "probes" else None
    every, sampled, fit = (EVERY if obs == "probes" else 1), obs == "probes", obs == "target"
    g_p, g_v, g_obs = w[0], w[1], (w[2] if len(w) == 3 else None)
    shared = dict(count=cnt)
    if taped:
        tape = torch.empty(ops.micro_tape_numel(desc, steps), dtype=torch.float32, device=cuda)
        ptape = torch.empty(ops.micro_param_tape_numel(desc, steps), dtype=torch.float32, device=cuda) if want_params else None
        hist = torch.empty(steps, L, 2, V, dtype=torch.float32, device=cuda) if obs else None
        pT, vT = ops.micro_rollout_fwd(desc, steps, p0, v0, par, b, tape=tape, hist=hist, ptape=ptape, **shared)
        third, g_hist = hist, g_obs
        if sampled:                          # the cotangent of the cut, scattered back into a dense one by autograd
            dense = hist.clone().requires_grad_()
            third = ops.cut_samples(dense, PROBES, EVERY, cnt)
            (third * g_obs).sum().backward()
            third, g_hist = third.detach(), dense.grad
        g_p0, g_v0, g_b = ops.micro_rollout_bwd(desc, steps, tape, g_p, g_v, g_hist=g_hist, ptape=ptape, params=par if want_params else None,
                                                g_params=g_params, **shared)
        return (pT, vT) + (() if third is None else (third,)), dict(p0=g_p0, v0=g_v0, params=g_params, boundary=g_b)
    seg = (ops.micro_ckpt_target_plan if fit else ops.micro_ckpt_plan)(desc, steps, want_params, S)["segment"]
    ckpt = torch.empty(ops.micro_ckpt_numel(desc, steps, seg), dtype=torch.float32, device=cuda)
    shared.update(segment=seg)
    head, lead, ring = (b if kind == k else None for k in ("head", "lead", "ring"))
    if kind == "lead_length":
        lead = b
    g_b = None
    if fit and ring is not None:
        pT, vT, third = ops.micro_rollout_fwd_ckpt_target_ring(desc, steps, p0, v0, par, ring, ckpt, tg, **shared)
        g_p0, g_v0 = ops.micro_rollout_bwd_ckpt_target_ring(desc, steps, ckpt, par, ring, g_p, g_v, tg, g_sse=g_obs, g_params=g_params, **shared)
    elif fit:
        pT, vT, third = ops.micro_rollout_fwd_ckpt_target(desc, steps, p0, v0, par, ckpt, tg, head=head, lead=lead, lead_length=ll, **shared)
        g_p0, g_v0, g_b = ops.micro_rollout_bwd_ckpt_target(desc, steps, ckpt, par, g_p, g_v, tg, g_sse=g_obs, head=head, lead=lead,
                                                            lead_length=ll, g_params=g_params, **shared)
    elif ring is not None:
        pT, vT, third = ops.micro_rollout_fwd_ckpt_ring(desc, steps, p0, v0, par, ring, ckpt, probes, every, observe=sampled, **shared)
        g_p0, g_v0 = ops.micro_rollout_bwd_ckpt_ring(desc, steps, ckpt, par, ring, g_p, g_v, probes, every, g_obs, g_params=g_params, **shared)
    elif lead is not None:
        pT, vT, third = ops.micro_rollout_fwd_ckpt_lead(desc, steps, p0, v0, par, lead, ckpt, probes, every, lead_length=ll, observe=sampled,
                                                        **shared)
        g_p0, g_v0, g_b = ops.micro_rollout_bwd_ckpt_lead(desc, steps, ckpt, par, lead, g_p, g_v, probes, every, g_obs, lead_length=ll,
                                                          g_params=g_params, **shared)
    elif sampled:
        pT, vT, third = ops.micro_rollout_fwd_ckpt_samples(desc, steps, p0, v0, par, head, ckpt, probes, every, **shared)
        g_p0, g_v0, g_b = ops.micro_rollout_bwd_ckpt_samples(desc, steps, ckpt, par, head, g_p, g_v, probes, every, g_obs, g_params=g_params,
                                                             **shared)
    else:
        third = torch.empty(steps, L, 2, V, dtype=torch.float32, device=cuda) if obs == "hist" else None
        pT, vT = ops.micro_rollout_fwd_ckpt(desc, steps, p0, v0, par, head, ckpt, hist=third, **shared)
        g_p0, g_v0, g_b = ops.micro_rollout_bwd_ckpt(desc, steps, ckpt, par, head, g_p, g_v, g_hist=g_obs, g_params=g_params, **shared)
    return (pT, vT) + (() if third is None else (third,)), dict(p0=g_p0, v0=g_v0, params=g_params, boundary=g_b)


def micro_held(cuda, kind, obs, want_params, steps=T, checkpoint=S):
    import torch
    c, w, _, _ = micro_case(kind.split("_")[0], steps)
    w = [torch.tensor(a, device=cuda) for a in w[obs]]
    x = micro_leaves(cuda, c, kind, want_params=want_params)
    out = micro_api(cuda, x, kind, obs, steps, checkpoint)
    weighted(out, w).backward()
    want, g = micro_by_hand(cuda, x, kind, obs, w, steps, taped=checkpoint is None)
    tag = (kind, obs, want_params, steps, checkpoint)
    if checkpoint is not None:
        assert out[0].grad_fn.name() == micro_class(kind, obs) + "Backward", tag
    assert len(out) == len(want) == (2 if obs is None else 3), tag
    live = torch.tensor(J.live_mask(c), device=cuda)
    for k, (a, b) in enumerate(zip(out, want)):
        if obs == "hist" and k == 2:         # (the forward leaves a history's slots at or beyond count unwritten)
            a, b = (torch.where(live[:, None, :], t.detach(), torch.zeros_like(t)) for t in (a, b))
        same(a.detach(), b, tag + ("output", k))
    assert all(o.dtype == torch.float32 and tuple(o.shape) == (L, V) for o in out[:2]), tag
    if obs is not None:
        shape = {"hist": (steps, L, 2, V), "probes": (steps // EVERY, L, 2, len(PROBES)), "target": (L, 2)}[obs]
        assert out[2].dtype == (torch.float64 if obs == "target" else torch.float32) and tuple(out[2].shape) == shape, tag
    for k, leaf in x.items():
        same(leaf.grad, g[k], tag + ("gradient", k))
        assert (leaf.grad is not None) == leaf.requires_grad and (leaf.grad is None or leaf.grad.dtype == leaf.dtype), tag
        assert leaf.grad is None or leaf.grad.shape == leaf.shape, tag
    assert (x["params"].grad is not None) == want_params and (x["boundary"].grad is None) == (kind == "ring"), tag
    if kind.startswith("lead"):
        assert x["boundary"].grad.dtype == torch.float32 and tuple(x["boundary"].grad.shape) == (steps, L, 2), tag


@pytest.mark.parametrize("want_params", (False, True))
@pytest.mark.parametrize("kind,obs", MICRO_FORMS)
def test_micro_checkpointed_forms_are_the_raw_wrappers(cuda, kind, obs, want_params):
    micro_held(cuda, kind, obs, want_params)


@pytest.mark.parametrize("want_params", (False, True))
@pytest.mark.parametrize("obs", (None, "hist", "probes"))
def test_micro_taped_forms_are_the_raw_wrappers(cuda, obs, want_params):
    micro_held(cuda, "head", obs, want_params, checkpoint=None)


def test_micro_without_a_step(cuda):
    micro_held(cuda, "head", "probes", True, steps=0)
    micro_held(cuda, "head", "target", True, steps=0)


@pytest.mark.parametrize("kind,obs", MICRO_FORMS)
def test_micro_checkpoint_without_grad(cuda, handed, kind, obs):
    """Without a leaf that requires grad MicroRollout runs the taped kernels without a tape, and every other Function runs its
    checkpointed forward without a checkpoint; with one, every form keeps a checkpoint."""
    import torch
    c = micro_case(kind.split("_")[0])[0]
    out = micro_api(cuda, micro_leaves(cuda, c, kind, grad=False), kind, obs)
    assert not any(o.requires_grad for o in out)
    assert handed == ([] if micro_class(kind, obs) == "MicroRollout" else [False]), (kind, obs, handed)
    del handed[:]
    with_grad = micro_api(cuda, micro_leaves(cuda, c, kind), kind, obs)
    assert handed == [True], (kind, obs, handed)
    for k, (a, b) in enumerate(zip(out, with_grad)):
        if not (obs == "hist" and k == 2):
            assert torch.equal(a, b.detach())


@pytest.mark.parametrize("kind,obs", MICRO_FORMS)
def test_micro_backward_and_the_context(cuda, kind, obs):
    """Every checkpointed micro form keeps its context and makes its buffers in forward: a backward over a retained graph into gradients
    that exist already leaves torch.cuda.memory_allocated() where it was, the first time and the second, and the second returns the
    first one's bits."""
    import torch
    c, w, _, _ = micro_case(kind.split("_")[0])
    w = [torch.tensor(a, device=cuda) for a in w[obs]]

    def run():
        x = micro_leaves(cuda, c, kind)
        return x, weighted(micro_api(cuda, x, kind, obs), w)
    from dhts import ops
    run()[1].backward()                      # (whatever a first backward of the process sets up is there)
    ops.MicroRollout.last_bwd_record = None  # (micro_bwd_fault()'s record of that sweep, which the next one would replace and so free)
    x, loss = run()
    leaves = list(x.values())
    assert backward_into_zeros(loss, leaves) == 0
    first = [t.grad.clone() for t in leaves if t.requires_grad]
    assert backward_into_zeros(loss, leaves) == 0
    for t, g in zip([t for t in leaves if t.requires_grad], first):
        assert torch.equal(t.grad, g + g)
