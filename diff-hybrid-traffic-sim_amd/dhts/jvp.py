"""Forward-mode differentiation of the fused rollouts: dhts.macro_rollout_jvp (ARZ) and dhts.micro_rollout_jvp (IDM), K Jacobian-vector
products in one pass over the rollout tape (dhts_macro_rollout_jvp, dhts_micro_rollout_jvp, include/dhts.h) or, with fused=True, in
one kernel that steps the rollout and its tangents together and has no tape (dhts_macro_rollout_fwd_jvp, dhts_micro_rollout_fwd_jvp).
The raw operators are in dhts.ops; MacroRollout and MicroRollout (reverse mode) are untouched."""
import torch

from . import ops


def _jvp_tangents(r0, ghost_r, T, t_r0, t_u0, t_ghost_r, t_ghost_u, t_inflow=None, n_ramp=0):
    """Shape checks of dhts.macro_rollout_jvp's tangents (ValueError, before anything touches a device).  Returns K.  t_inflow: the
    tangent of `inflow` [T][L][n_ramp], one more leaf."""
    given = [(n, t) for n, t in (("t_r0", t_r0), ("t_u0", t_u0), ("t_ghost_r", t_ghost_r), ("t_ghost_u", t_ghost_u), ("t_inflow", t_inflow))
             if t is not None]
    if not given:
        raise ValueError("macro_rollout_jvp needs at least one of t_r0, t_u0, t_ghost_r, t_ghost_u, t_inflow")
    if r0.dim() != 2:
        raise ValueError("r0 must be [L][N]")
    L, N = r0.shape
    for n, t in given:
        if not isinstance(t, torch.Tensor) or t.dim() < 1 or t.shape[0] < 1:
            raise ValueError("%s must be a tensor with a leading direction axis K >= 1" % n)
    K = int(given[0][1].shape[0])
    want_g = (K, int(T), L, 2) if ghost_r is not None and ghost_r.dim() == 3 else (K, L, 2)
    for n, t in given:
        want = (K, L, N) if n in ("t_r0", "t_u0") else ((K, int(T), L, n_ramp) if n == "t_inflow" else want_g)
        if tuple(t.shape) != want:
            raise ValueError("%s must have shape %s (got %s): all tangents share K = %d, boundary tangents follow the form of ghost_r"
                             % (n, want, tuple(t.shape), K))
    if t_inflow is not None and (t_inflow.dtype != torch.float32 or t_inflow.device != r0.device):
        raise ValueError("t_inflow must be a float32 tensor on r0's device (%s) (got %s on %s)" % (r0.device, t_inflow.dtype, t_inflow.device))
    return K


def macro_rollout_jvp(r0, u0, ghost_r, ghost_u, T, dt, dx, u_max, *, t_r0=None, t_u0=None, t_ghost_r=None, t_ghost_u=None,
                      detectors=None, check_faults=True, fused=False, ring=False, ramps=None, inflow=None, t_inflow=None):
    """dhts.macro_rollout and K Jacobian-vector products of it in one pass over its tape (forward mode).

    Returns ((rT, yT, uT, qT[, readings]), (t_rT, t_yT, t_uT[, t_readings])).  The primal outputs are those of
    dhts.macro_rollout(r0, u0, ghost_r, ghost_u, T, dt, dx, u_max, detectors=detectors) bit for bit.  The tangents carry a leading
    direction axis K: t_r0, t_u0 [K][L][N]; t_ghost_r, t_ghost_u [K][L][2], or [K][T][L][2] when ghost_r, ghost_u are a schedule
    [T][L][2].  At least one is given, all share K, a missing one is zero; anything else is a ValueError before anything touches a device.
    Direction i of the outputs is J applied to direction i of the inputs: t_rT, t_yT, t_uT [K][L][N] and, with detectors, t_readings
    [K][T][L][3][D], the tangent of (r, y, u) of cell detectors[j] after every step.  Nothing returned here is differentiable (no
    autograd graph is recorded; the inputs are read as constants): for gradients use dhts.macro_rollout.

    fused=True: the rollout and its tangents are stepped together by one kernel (dhts_macro_rollout_fwd_jvp) and no tape is allocated
    (17.3 B per cell-step: 9 GB at 1024 x 512 x 1000) -- same return values, bit for bit, and the same two fault checks in the same
    order (the forward's, then the tangent sweep's); nothing it allocates grows with T but the readings.  It runs up to four directions
    per launch and recomputes the primal in every launch, on the two-phase lane kernel's mapping with a larger LDS footprint, so it is
    NOT always the faster path.  Measured on one MI355X: at 1024 lanes x 512 cells x 1000 steps it is slower than
    fused=False for every K (1.04x, 1.08x at K = 1, 2; 1.8x at K = 3, 4; 2.4x at K = 8); at 4096 x 64 x 1000 with four detectors it
    takes 0.74, 0.79 of the taped time at K = 1, 2 and 1.16 .. 1.61 from K = 3 on (0.89 at K = 3, 4 at 3328 lanes, which
    a launch of four holds on the chip at once).  Choose it when the tape is what limits T, or for few directions on short lanes.
    Lanes of more than 1410 cells do not fit it (ValueError before anything is launched; fused=False covers them).

    ring=True (with fused=True only; ghost_r, ghost_u, t_ghost_r and t_ghost_u None): the lane is closed as in dhts.macro_rollout(ring=True)
    (dhts_macro_rollout_fwd_jvp_ring); the tangents of the two end cells are each other's boundary tangents.

    ramps / inflow / t_inflow (with fused=True only): dhts.macro_rollout's on-ramps -- `ramps` the cells, `inflow` float32 [T][L][R] the
    density rate cell ramps[j] of lane l gets in step t -- and t_inflow float32 [K][T][L][R], the tangent of `inflow`: one more leaf
    tangent, which counts as "at least one given" and shares K; None is zero, so ramps and inflow alone give the other leaves' tangents
    through a rollout with a source.  The primal outputs are dhts.macro_rollout(..., checkpoint=True, ramps=, inflow=)'s bit for bit, and
    with detectors the readings and t_readings are those after the source (dhts_macro_rollout_fwd_jvp_ramp / _ring_ramp).
    ramps without inflow (or the reverse), t_inflow without ramps, any of the three with fused=False, a wrong shape, dtype or device:
    ValueError before anything touches a device."""
    ops._macro_ring_checks(ring, ghost_r, ghost_u, t_ghost_r, t_ghost_u, fused=fused, r0=r0, u0=u0)
    if not ring and (ghost_r.dim() != ghost_u.dim() or ghost_r.dim() not in (2, 3)):
        raise ValueError("ghost_r and ghost_u must both be [L][2] or both [T][L][2]")
    T = int(T)
    if (ramps is None) != (inflow is None):
        raise ValueError("ramps and inflow go together: the cells, and inflow [T][L][R] with the rate each of them gets in every step")
    if t_inflow is not None and ramps is None:
        raise ValueError("t_inflow needs ramps and inflow: it is the tangent of inflow")
    if ramps is not None and not fused:
        raise ValueError("ramps, inflow and t_inflow live on the fused forward + tangent kernel only: pass fused=True")
    cells = ops._macro_ramp_checks(r0, T, ramps, inflow, False, True)
    n_ramp = 0 if cells is None else (cells.numel() if isinstance(cells, torch.Tensor) else len(cells))
    K = _jvp_tangents(r0, ghost_r, T, t_r0, t_u0, t_ghost_r, t_ghost_u, t_inflow, n_ramp)
    L, N = r0.shape
    sched = not ring and ghost_r.dim() == 3
    want = (T, L, 2) if sched else (L, 2)
    if ring and tuple(u0.shape) != (L, N):
        raise ValueError("u0 must have the shape of r0")
    if not ring and (tuple(ghost_r.shape) != want or tuple(ghost_u.shape) != want or tuple(u0.shape) != (L, N)):
        raise ValueError("u0 must have the shape of r0, ghost_r and ghost_u shape %s" % (want,))
    det = None if detectors is None else ops._detector_indices(detectors, N, r0.device)
    desc = ops.macro_desc(L, N, dt, dx, u_max)
    if fused and ops.macro_fwd_jvp_plan(desc, T, K)["dirs_per_launch"] < 1:
        raise ValueError("macro_rollout_jvp(fused=True): a lane of %d cells does not fit the fused forward + tangent kernel (its records, "
                         "the interface products and the tangent copies exceed the LDS of a workgroup); fused=False covers it" % N)
    with torch.no_grad():
        if ring:                             # no boundary cells: ghost None is the ring form of ops.macro_rollout_fwd_jvp
            r0c, u0c = ops._f32c(r0.detach(), "r0"), ops._f32c(u0.detach(), "u0")
            (y0, q0), ghost = ops.macro_state_from_ru(r0c, u0c, u_max), None
        else:
            r0c, u0c, gr, gu, _, y0, q0, ghost = ops._macro_leaves(r0, u0, ghost_r, ghost_u, u_max)
        readings = None
        if not fused:
            # the forward rollout with a tape, as MacroRollout.forward runs it
            tape = torch.empty(ops.macro_tape_numel(desc, T), dtype=torch.float32, device=r0c.device)
            err = ops.new_error_record(r0c.device)
            if det is not None:
                (rT, yT, uT, qT), readings = ops.macro_rollout_fwd_taps(desc, T, r0c, y0, u0c, q0, ghost, det, tape=tape, err=err)
            else:
                fwd = ops.macro_rollout_fwd_sched if sched else ops.macro_rollout_fwd
                rT, yT, uT, qT = fwd(desc, T, r0c, y0, u0c, q0, ghost, tape=tape, err=err)
            if check_faults:
                ops.raise_on_fault(err)
        # the leaves' tangents -> tangents of (r, y)
        dev = r0c.device

        def tan(t, shape):
            return torch.zeros(shape, dtype=torch.float32, device=dev) if t is None else ops._f32c(t.detach(), "tangent")

        tr0, tu0 = tan(t_r0, (K, L, N)), tan(t_u0, (K, L, N))
        ty0 = ops.macro_state_from_ru_jvp(r0c.expand(K, L, N), u0c.expand(K, L, N), tr0, tu0, u_max)
        t_ghost = None
        if (t_ghost_r is not None or t_ghost_u is not None) and gr.numel():
            tgr, tgu = tan(t_ghost_r, (K,) + want), tan(t_ghost_u, (K,) + want)
            tgy = ops.macro_state_from_ru_jvp(gr.expand((K,) + want), gu.expand((K,) + want), tgr, tgu, u_max)
            t_ghost = torch.stack([tgr, tgy], dim=-1).contiguous()          # [K][L][2][2], or [K][T][L][2][2]
        if fused:                            # one kernel, no tape
            err, err_jvp = ops.new_error_record(dev), ops.new_error_record(dev)
            ramp = {}
            if cells is not None:
                ramp = dict(ramps=cells if isinstance(cells, torch.Tensor) else torch.tensor(cells, dtype=torch.int32, device=dev),
                            inflow=ops._f32c(inflow.detach(), "inflow"),
                            t_inflow=None if t_inflow is None else ops._f32c(t_inflow.detach(), "t_inflow"))
            (rT, yT, uT, qT, readings), (t_rT, t_yT, t_taps) = ops.macro_rollout_fwd_jvp(desc, T, r0c, y0, u0c, q0, ghost, tr0, ty0,
                                                                                         t_ghost=t_ghost, det=det, err=err, err_jvp=err_jvp,
                                                                                         **ramp)
            if check_faults:                 # the pair's order: the forward's record first, then the tangents'
                ops.raise_on_fault(err)
                ops.raise_on_fault(err_jvp)
        else:
            err = ops.new_error_record(dev)
            t_rT, t_yT, t_taps = ops.macro_rollout_jvp(desc, T, tape if T > 0 else None, tr0, ty0, t_ghost=t_ghost, det=det, err=err)
            if check_faults:
                ops.raise_on_fault(err)
        t_uT = ops.macro_u_tap_jvp(rT.expand(K, L, N), yT.expand(K, L, N), t_rT, t_yT, u_max)
        primal = (rT, yT, uT, qT)
        if det is None:
            return primal, (t_rT, t_yT, t_uT)
        D = det.numel()
        if T > 0:
            sr, sy = readings[:, :, 0].expand(K, T, L, D), readings[:, :, 1].expand(K, T, L, D)
            tsr, tsy = t_taps[:, :, :, 0].contiguous(), t_taps[:, :, :, 1].contiguous()
            tsu = ops.macro_u_tap_jvp(sr, sy, tsr, tsy, u_max)
            t_readings = torch.stack([tsr, tsy, tsu], dim=3).contiguous()
        else:
            t_readings = torch.zeros(K, 0, L, 3, D, dtype=torch.float32, device=dev)
        return primal + (readings,), (t_rT, t_yT, t_uT, t_readings)


def _micro_jvp_tangents(p0, t_p0, t_v0, t_params, t_head, t_lead=None, T=0):
    """Shape checks of dhts.micro_rollout_jvp's tangents (ValueError, before anything touches a device).  Returns K."""
    given = [(n, t) for n, t in (("t_p0", t_p0), ("t_v0", t_v0), ("t_params", t_params), ("t_head", t_head), ("t_lead", t_lead))
             if t is not None]
    if not given:
        raise ValueError("micro_rollout_jvp needs at least one of t_p0, t_v0, t_params, t_head, t_lead")
    if p0.dim() != 2:
        raise ValueError("p0 must be [L][V]")
    L, V = p0.shape
    for n, t in given:
        if not isinstance(t, torch.Tensor) or t.dim() < 1 or t.shape[0] < 1:
            raise ValueError("%s must be a tensor with a leading direction axis K >= 1" % n)
    K = int(given[0][1].shape[0])
    want = dict(t_p0=(K, L, V), t_v0=(K, L, V), t_params=(K, 6, L, V), t_head=(K, L, 2), t_lead=(K, int(T), L, 2))
    for n, t in given:
        if tuple(t.shape) != want[n]:
            raise ValueError("%s must have shape %s (got %s): all tangents share K = %d" % (n, want[n], tuple(t.shape), K))
    return K


def _micro_gn_checks(target, fused, want_hist):
    """What target= rules out whatever the shapes are (ValueError, before anything touches a device)."""
    if not fused:
        raise ValueError("target lives in the fused kernel only: pass fused=True")
    if want_hist:
        raise ValueError("target and want_hist exclude each other: the fit is formed in the kernel so that no history exists")
    if not isinstance(target, torch.Tensor):
        raise ValueError("target must be a float32 tensor")


def _micro_gn_target(p0, T, dt, K, t_params, sampling, target):
    """target against the shape of the samples it takes the place of, and K against the plan of the Gauss-Newton form (ValueError, before
    anything touches a device)."""
    L, V = p0.shape
    slots, every = sampling if sampling is not None else (None, 1)
    n = V if slots is None else (int(slots.numel()) if isinstance(slots, torch.Tensor) else len(slots))
    shape = (T // every, L, 2, n)
    if target.dtype != torch.float32:
        raise ValueError("target must be float32 (got %s)" % target.dtype)
    if tuple(target.shape) != shape:
        raise ValueError("target must have shape %s (got %s): [T // every][L][2][P], the shape of samples" % (shape, tuple(target.shape)))
    if target.device != p0.device:
        raise ValueError("target must be on p0's device %s (got %s)" % (p0.device, target.device))
    if not target.is_contiguous():
        raise ValueError("target must be contiguous")
    if target.requires_grad:
        raise ValueError("target must not require grad: it is data (a gradient of sse is dhts.micro_rollout(checkpoint=True, target=)'s)")
    ops._gn_plan_carries(ops.micro_desc(L, V, dt), T, K, t_params is not None)


def micro_rollout_jvp(p0, v0, params, head, T, dt, *, t_p0=None, t_v0=None, t_params=None, t_head=None, count=None, want_hist=False,
                      check_faults=True, fused=False, probes=None, every=1, lead=None, lead_length=None, t_lead=None, ring=None,
                      target=None):
    """dhts.micro_rollout and K Jacobian-vector products of it in one pass over its tape (forward mode).

    Returns ((pT, vT[, hist]), (t_pT, t_vT[, t_hist])).  The primal outputs are those of dhts.micro_rollout(p0, v0, params, head, T, dt,
    count=count, want_hist=want_hist) bit for bit.  The tangents carry a leading direction axis K: t_p0, t_v0 [K][L][V]; t_params
    [K][6][L][V]; t_head [K][L][2].  At least one is given, all share K, a missing one is zero; anything else is a ValueError before
    anything touches a device.  Direction i of the outputs is J applied to direction i of the inputs: t_pT, t_vT [K][L][V] float32 and,
    with want_hist, t_hist [K][T][L][2][V]; slots at or beyond a lane's count are exactly 0.  The forward fills the parameter tape only
    when t_params is given.  fused=True: the rollout and its tangents are stepped together by one kernel (dhts_micro_rollout_fwd_jvp)
    and neither the tape nor the parameter tape is allocated -- same return values, bit for bit, and the same two fault checks in the
    same order (the forward's, then the tangent sweep's).  Nothing returned here is differentiable (no autograd graph is recorded; the
    inputs are read as constants): for gradients use dhts.micro_rollout.

    probes / every: as dhts.micro_rollout's (the same rules and ValueErrors; not together with want_hist).  With sampling on the call
    returns ((pT, vT, samples), (t_pT, t_vT, t_samples)): samples [T // every][L][2][P] and t_samples [K][T // every][L][2][P], row j
    = slot probes[i] after step (j + 1) every - 1, slots at or beyond count exactly 0 in both.  fused=True writes them from the kernel
    (dhts_micro_rollout_fwd_jvp_samples) and nothing of size T x V is allocated; with fused=False, the taped path, the samples are cut
    out of a dense history: ask for fused=True when memory matters.

    lead / lead_length / t_lead: as dhts.micro_rollout's `lead` (the head vehicle follows a recorded leader; `head` and t_head must be
    None), with t_lead float32 [K][T][L][2] the leader's tangents per direction (None: zero).  It lives on the fused path only:
    fused=True is required, want_hist is not accepted; t_lead without lead, or t_head together with lead, is a ValueError.  Without
    probes / every the call returns ((pT, vT), (t_pT, t_vT)).

    ring: as dhts.micro_rollout's `ring` (float64 [L]; the head vehicle follows the image of the tail one circumference ahead, whose
    tangents are the tail's; the tail's length tangent is in the head's gap).  It lives on the fused path only: fused=True is required,
    want_hist is not accepted, and head, t_head, lead (with lead_length) and t_lead must be None.  probes / every combine with it.

    target: the Gauss-Newton normal equations of a trajectory fit, formed inside the fused kernel (dhts_micro_rollout_fwd_jvp_gn; fused=True
    is required, want_hist is not accepted; every boundary and probes / every combine with it).  target is what was observed: float32,
    contiguous, on p0's device, not requiring grad, of the shape samples would have -- [T][L][2][V] without sampling,
    [T // every][L][2][P] with it; a NaN entry is not observed, a slot at or beyond count is never read.  The call returns
    ((pT, vT, sse), (t_pT, t_vT, jtr, jtj)) and allocates neither history nor samples: with r = x - target in float32 and t_a the
    float32 tangent of x in direction a, sse float64 [L][2] is dhts.micro_rollout(checkpoint=True, target=)'s (sum of r r per plane),
    jtr float64 [L][K] the sum of t_a r and jtj float64 [L][K][K] the sum of t_a t_b over the observed entries of both planes of a lane
    -- exact double products, summed in a fixed order (two runs give the same bits; jtj is bit-symmetric).  The loss is sse.sum(), its
    gradient along the directions 2 jtr.sum(0), the Gauss-Newton matrix 2 jtj.sum(0).  K directions beyond what a launch carries are
    run as one launch per pair of direction blocks (ops.micro_gn_launches); a K the lane's plan cannot carry is a ValueError."""
    T = int(T)
    if target is not None:
        _micro_gn_checks(target, fused, want_hist)
    if ring is not None:
        if lead is not None or lead_length is not None or t_lead is not None:
            raise ValueError("lead, lead_length and t_lead must be None when ring is given: the head vehicle follows the tail")
        return _micro_rollout_jvp_lead(p0, v0, params, head, T, dt, t_p0, t_v0, t_params, t_head, count, want_hist, check_faults, fused,
                                       probes, every, None, None, None, ring, target)
    if lead is None and (t_lead is not None or lead_length is not None):
        raise ValueError("t_lead and lead_length need lead")
    if lead is not None:
        return _micro_rollout_jvp_lead(p0, v0, params, head, T, dt, t_p0, t_v0, t_params, t_head, count, want_hist, check_faults, fused,
                                       probes, every, lead, lead_length, t_lead, None, target)
    K = _micro_jvp_tangents(p0, t_p0, t_v0, t_params, t_head)
    L, V = p0.shape
    sampling = ops.micro_sampling(probes, every, V, want_hist)
    if sampling is not None and not fused:       # the taped path: both histories, cut
        (pT, vT, hist), (t_pT, t_vT, t_hist) = micro_rollout_jvp(p0, v0, params, head, T, dt, t_p0=t_p0, t_v0=t_v0, t_params=t_params,
                                                                 t_head=t_head, count=count, want_hist=True, check_faults=check_faults)
        return (pT, vT, ops.cut_samples(hist, *sampling, count)), (t_pT, t_vT, ops.cut_samples(t_hist, *sampling, count))
    if tuple(v0.shape) != (L, V) or tuple(params.shape) != (6, L, V) or tuple(head.shape) != (L, 2):
        raise ValueError("v0 must have the shape of p0, params shape (6, %d, %d), head shape (%d, 2)" % (L, V, L))
    if count is not None and (count.dtype != torch.int32 or tuple(count.shape) != (L,)):
        raise ValueError("count must be int32 [L]")
    if T < 0:
        raise ValueError("T must be >= 0")
    if target is not None:
        _micro_gn_target(p0, T, dt, K, t_params, sampling, target)
    desc = ops.micro_desc(L, V, dt)
    with torch.no_grad():
        p0c, v0c = ops._f32c(p0.detach(), "p0"), ops._f32c(v0.detach(), "v0")
        dev = p0c.device
        par = params.detach().contiguous()

        def tan(t, shape, dtype):
            if t is None:
                return torch.zeros(shape, dtype=dtype, device=dev)
            return t.detach().to(device=dev, dtype=dtype).contiguous()

        tp, tv = tan(t_p0, (K, L, V), torch.float32), tan(t_v0, (K, L, V), torch.float32)
        th = None if t_head is None else tan(t_head, (K, L, 2), torch.float64)
        tq = None if t_params is None else tan(t_params, (K, 6, L, V), torch.float64)
        if fused:                            # one kernel, no tape
            err, err_jvp = ops.new_error_record(dev), ops.new_error_record(dev)
            if target is not None:           # the Gauss-Newton form: no history and no samples, the fit's sums instead
                slots, ev = sampling if sampling is not None else (None, 1)
                prim, tang = ops.micro_rollout_fwd_jvp_gn(desc, T, p0c, v0c, par, tp, tv, target, head=head.detach(),
                                                          probes=ops._device_slots(slots, dev), every=ev, count=count, t_head=th,
                                                          t_params=tq, err=err, err_jvp=err_jvp)
                if check_faults:
                    ops.raise_on_fault(err)
                    ops.raise_on_fault(err_jvp)
                return prim, tang
            if sampling is not None:         # the sampled kernel form: no history of either kind
                slots = ops._device_slots(sampling[0], dev)
                prim, tang = ops.micro_rollout_fwd_jvp_samples(desc, T, p0c, v0c, par, head.detach(), tp, tv, slots, sampling[1], count=count,
                                                               t_head=th, t_params=tq, err=err, err_jvp=err_jvp)
                if check_faults:
                    ops.raise_on_fault(err)
                    ops.raise_on_fault(err_jvp)
                return prim, tang
            (pT, vT, hist), (t_pT, t_vT, t_hist) = ops.micro_rollout_fwd_jvp(desc, T, p0c, v0c, par, head.detach(), tp, tv, count=count,
                                                                             t_head=th, t_params=tq, want_hist=want_hist, err=err,
                                                                             err_jvp=err_jvp)
            if check_faults:                 # the forward's record first (a collision is printed and tolerated), then the tangents'
                ops.raise_on_fault(err)
                ops.raise_on_fault(err_jvp)
            if want_hist:
                return (pT, vT, hist), (t_pT, t_vT, t_hist)
            return (pT, vT), (t_pT, t_vT)
        # the forward rollout with a tape, as MicroRollout.forward runs it
        tape = torch.empty(ops.micro_tape_numel(desc, T), dtype=torch.float32, device=dev)
        ptape = torch.empty(ops.micro_param_tape_numel(desc, T), dtype=torch.float32, device=dev) if t_params is not None else None
        hist = torch.empty(T, L, 2, V, dtype=torch.float32, device=dev) if want_hist else None
        err = ops.new_error_record(dev)
        pT, vT = ops.micro_rollout_fwd(desc, T, p0c, v0c, par, head.detach(), count=count, tape=tape, hist=hist, err=err, ptape=ptape)
        if check_faults:                 # a collision is printed like the reference does, and tolerated
            ops.raise_on_fault(err)
        err = ops.new_error_record(dev)
        t_pT, t_vT, t_hist = ops.micro_rollout_jvp(desc, T, tape if T > 0 else None, tp, tv, count=count, t_head=th, ptape=ptape,
                                                   params=par if tq is not None else None, t_params=tq, want_hist=want_hist, err=err)
        if check_faults:
            ops.raise_on_fault(err)
    if want_hist:
        return (pT, vT, hist), (t_pT, t_vT, t_hist)
    return (pT, vT), (t_pT, t_vT)


def _micro_rollout_jvp_lead(p0, v0, params, head, T, dt, t_p0, t_v0, t_params, t_head, count, want_hist, check_faults, fused, probes, every,
                            lead, lead_length, t_lead, ring=None, target=None):
    """dhts.micro_rollout_jvp with a recorded leader, or (ring given, lead None) on a ring road: every ValueError first, then the lead
    or the ring form of the fused kernel."""
    what, follows = ("lead", "`lead`") if ring is None else ("ring", "the tail")
    if head is not None or t_head is not None:
        raise ValueError("head and t_head must be None when %s is given: the head vehicle follows %s, no head gap exists" % (what, follows))
    if not fused:
        raise ValueError("%s lives on the tape-free path only: pass fused=True" % what)
    if want_hist:
        raise ValueError("%s does not take want_hist: the dense history is the sampled form, probes=range(V) with every=1" % what)
    K = _micro_jvp_tangents(p0, t_p0, t_v0, t_params, None, t_lead, T)
    L, V = p0.shape
    if T < 0:
        raise ValueError("T must be >= 0")
    if ring is not None and (not isinstance(ring, torch.Tensor) or ring.dtype != torch.float64 or tuple(ring.shape) != (L,)):
        raise ValueError("ring must be a float64 tensor of shape (L,) = (%d,)" % L)
    if ring is None and (not isinstance(lead, torch.Tensor) or lead.dtype != torch.float32 or tuple(lead.shape) != (T, L, 2)):
        raise ValueError("lead must be a float32 tensor of shape (T, L, 2) = (%d, %d, 2)" % (T, L))
    if lead_length is not None and (not isinstance(lead_length, torch.Tensor) or lead_length.dtype != torch.float64
                                    or tuple(lead_length.shape) != (L,)):
        raise ValueError("lead_length must be None or a float64 tensor of shape (L,) = (%d,)" % L)
    if tuple(v0.shape) != (L, V) or tuple(params.shape) != (6, L, V):
        raise ValueError("v0 must have the shape of p0, params shape (6, %d, %d)" % (L, V))
    if count is not None and (count.dtype != torch.int32 or tuple(count.shape) != (L,)):
        raise ValueError("count must be int32 [L]")
    sampling = ops.micro_sampling(probes, every, V, False)
    if target is not None:
        _micro_gn_target(p0, T, dt, K, t_params, sampling, target)
    desc = ops.micro_desc(L, V, dt)
    with torch.no_grad():
        p0c, v0c = ops._f32c(p0.detach(), "p0"), ops._f32c(v0.detach(), "v0")
        dev = p0c.device

        def tan(t, shape, dtype):
            if t is None:
                return torch.zeros(shape, dtype=dtype, device=dev)
            return t.detach().to(device=dev, dtype=dtype).contiguous()

        tp, tv = tan(t_p0, (K, L, V), torch.float32), tan(t_v0, (K, L, V), torch.float32)
        tl = None if t_lead is None else tan(t_lead, (K, T, L, 2), torch.float32)
        tq = None if t_params is None else tan(t_params, (K, 6, L, V), torch.float64)
        ll = None if lead_length is None else lead_length.detach().to(device=dev).contiguous()
        slots, ev = sampling if sampling is not None else (None, 1)
        slots = ops._device_slots(slots, dev)
        err, err_jvp = ops.new_error_record(dev), ops.new_error_record(dev)
        if target is not None:
            prim, tang = ops.micro_rollout_fwd_jvp_gn(desc, T, p0c, v0c, params.detach(), tp, tv, target,
                                                      lead=None if ring is not None else ops._f32c(lead.detach(), "lead"), lead_length=ll,
                                                      ring=None if ring is None else ring.detach().to(device=dev).contiguous(),
                                                      probes=slots, every=ev, count=count, t_lead=tl, t_params=tq, err=err,
                                                      err_jvp=err_jvp)
        elif ring is not None:
            prim, tang = ops.micro_rollout_fwd_jvp_ring(desc, T, p0c, v0c, params.detach(), ring.detach().to(device=dev).contiguous(), tp,
                                                        tv, slots, ev, count=count, t_params=tq, observe=sampling is not None, err=err,
                                                        err_jvp=err_jvp)
        else:
            prim, tang = ops.micro_rollout_fwd_jvp_lead(desc, T, p0c, v0c, params.detach(), ops._f32c(lead.detach(), "lead"), tp, tv, slots,
                                                        ev, lead_length=ll, count=count, t_lead=tl, t_params=tq,
                                                        observe=sampling is not None, err=err, err_jvp=err_jvp)
        if check_faults:                 # the forward's record first (a collision is printed and tolerated), then the tangents'
            ops.raise_on_fault(err)
            ops.raise_on_fault(err_jvp)
    if target is not None:
        return prim, tang
    if sampling is None:
        return prim[:2], tang[:2]
    return prim, tang

