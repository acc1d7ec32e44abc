"""Device-side operators over libdhts.so: raw calls on torch CUDA tensors + torch.autograd.Functions.

PyTorch is plumbing here (device memory, streams, autograd bookkeeping, the optimiser outside); every
per-step computation of the hot path is a hand-written HIP kernel behind the C ABI (include/dhts.h).

Mirrors the reference operators
    dMacroForwardLayer  road/lane/dmacro_lane.py:234-309
    dMicroForwardLayer  road/lane/dmicro_lane.py:228-298
batched over lanes and fused over time steps.
"""
import collections
import ctypes as C
import operator
import warnings

import torch

from . import _lib
from ._lib import MacroDesc, MicroDesc, call, check, raw
from .tables import UploadedTables

EPS = 1e-5  # model/macro/_arz.py:2


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32c(t, name):
    if t.dtype != torch.float32 or not t.is_cuda:
        raise TypeError("%s must be a float32 CUDA tensor (got %s on %s)" % (name, t.dtype, t.device))
    return t.contiguous()


# ---- what the raw wrappers of both models share: optional arrays, observation buffers, state outputs ----
def _data(t):
    """The address the library gets for an optional array: NULL for None and for a tensor without an element (it has no address)."""
    return None if t is None or not t.numel() else C.c_void_p(t.data_ptr())


def _obs_buffer(name, t, shape, device, new=torch.zeros):
    """An observation array handed in (checked), or one made by `new` (None: none).  Samples are zero-filled: the kernels write live
    probe slots only."""
    if t is None:
        return None if new is None else new(shape, dtype=torch.float32, device=device)
    if tuple(t.shape) != tuple(shape) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
        raise ValueError("%s must be a contiguous float32 CUDA tensor of shape %s" % (name, tuple(shape)))
    return t


def _state_out(names, out, likes):
    """The state buffers of `out` (checked against the inputs they mirror), or new ones."""
    if not out:
        return tuple(torch.empty_like(t) for t in likes)
    for name, t, like in zip(names, out, likes):
        if t.shape != like.shape or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
            raise ValueError("%s must be a contiguous float32 CUDA tensor of shape %s" % (name, tuple(like.shape)))
    return tuple(out[:len(likes)])


def new_error_record(device):
    """Device-side sticky fault record (dhts_error): int32 [code, step, lane, index]."""
    return torch.zeros(4, dtype=torch.int32, device=device)


class CapacityError(RuntimeError):
    """A fused network episode needed more than one of the kernels' fixed capacities (include/dhts.h: vehicles per micro lane,
    vehicles per episode, records per step).  Nothing was changed on the host: callers can run the episode another way
    (ItscpEnv.step falls back to the lane-by-lane path).  `.index` = the fault record's index field: -2 = the stepwise path's hand-off
    event list (dhts_netstep_tables::max_events), -3 = a reverse sweep whose plan is not its forward's, else 0 / a count."""
    index = 0


def raise_on_fault(err):
    """Read the record back (synchronises) and raise the way the reference asserts."""
    code, step, lane, index = err.tolist()
    if code == _lib.FAULT_CFL:
        # road/lane/_macro_lane.py:145-146
        raise AssertionError("Time step size does not meet CFL condition. Please try smaller delta_time. "
                             "(step %d, lane %d, interface %d)" % (step, lane, index))
    if code == _lib.FAULT_NAN:
        raise AssertionError("non-finite gradient in the reverse sweep (step %d, lane %d)" % (step, lane))   # dmacro_lane.py:308
    if code == _lib.FAULT_CAPACITY:
        e = CapacityError("hybrid network: a fixed capacity was exceeded (record stream / vehicles / lane list / routes / events); "
                          "index %d" % index)
        e.index = int(index)
        raise e
    if code == _lib.FAULT_COLLISION:
        # printed and tolerated in the reference (_micro_lane.py:155-160): the deltas of that vehicle are zeroed, the run goes on
        print("Collision detected between vehicles (step %d, lane %d, vehicle %d)" % (step, lane, index))
    return code


# ---------------------------------------------------------------------------------------------------------
# macro
# ---------------------------------------------------------------------------------------------------------
def macro_desc(L, N, dt, dx, u_max):
    if not (1 <= N <= _lib.MACRO_MAX_CELLS):
        raise ValueError("cells per lane must be in 1..%d" % _lib.MACRO_MAX_CELLS)
    return MacroDesc(n_lanes=int(L), n_cells=int(N), dt=float(dt), dx=float(dx), u_max=float(u_max))


def macro_tape_numel(desc, T):
    """float32 elements of the rollout tape (include/dhts.h: left-cell states + the compacted products of the exceptions)."""
    return raw("dhts_macro_tape_bytes", d=C.byref(desc), T=int(T)) // 4


def macro_step_tape_numel(desc):
    """float32 elements of the single-step operator's tape (the reference's per-cell blocks)."""
    return raw("dhts_macro_step_tape_bytes", d=C.byref(desc)) // 4


def macro_step_fwd(desc, r, y, u, ueq, ghost, tape=None, err=None):
    """One step of L lanes through the operator entry point (dqs-layout tape)."""
    r, y, u, ueq, ghost = (_f32c(t, n) for t, n in ((r, "r"), (y, "y"), (u, "u"), (ueq, "ueq"), (ghost, "ghost")))
    out = tuple(torch.empty_like(r) for _ in range(4))
    call("dhts_macro_step_fwd", d=C.byref(desc), r=_ptr(r), y=_ptr(y), u=_ptr(u), ueq=_ptr(ueq), ghost=_ptr(ghost), r_out=_ptr(out[0]),
         y_out=_ptr(out[1]), u_out=_ptr(out[2]), ueq_out=_ptr(out[3]), tape=_ptr(tape), err=_ptr(err), stream=_stream())
    return out


def macro_step_bwd(desc, tape, g_r, g_y, err=None):
    g_r, g_y = _f32c(g_r, "g_r"), _f32c(g_y, "g_y")
    out = (torch.empty_like(g_r), torch.empty_like(g_y))
    g_ghost = torch.zeros(desc.n_lanes, 2, 2, dtype=torch.float64, device=g_r.device)
    call("dhts_macro_step_bwd", d=C.byref(desc), tape=_ptr(tape), g_r=_ptr(g_r), g_y=_ptr(g_y), g_r_out=_ptr(out[0]), g_y_out=_ptr(out[1]),
         g_ghost=_ptr(g_ghost), err=_ptr(err), stream=_stream())
    return out[0], out[1], g_ghost


def macro_state_from_ru(r, u, u_max):
    r, u = _f32c(r, "r"), _f32c(u, "u")
    y, q = torch.empty_like(r), torch.empty_like(r)
    call("dhts_macro_state_from_ru", n=r.numel(), u_max=float(u_max), r=_ptr(r), u=_ptr(u), y=_ptr(y), ueq=_ptr(q), stream=_stream())
    return y, q


def macro_state_from_ru_bwd(r, u, g_y, g_r, u_max):
    """g_r is updated in place; returns g_u."""
    g_u = torch.empty_like(r)
    call("dhts_macro_state_from_ru_bwd", n=r.numel(), u_max=float(u_max), r=_ptr(r), u=_ptr(u), g_y=_ptr(g_y), g_r=_ptr(g_r),
         g_u=_ptr(g_u), stream=_stream())
    return g_u


def macro_u_tap_bwd(r, y, g_u, g_r, g_y, u_max):
    """g_r, g_y updated in place."""
    call("dhts_macro_u_tap_bwd", n=r.numel(), u_max=float(u_max), r=_ptr(r), y=_ptr(y), g_u=_ptr(g_u), g_r=_ptr(g_r), g_y=_ptr(g_y),
         stream=_stream())


def _det_i32(det, N):
    if not isinstance(det, torch.Tensor) or det.dtype != torch.int32 or not det.is_cuda or det.dim() != 1:
        raise ValueError("det must be a one-dimensional int32 CUDA tensor")
    if not 1 <= det.numel() <= N:
        raise ValueError("det must hold 1..%d cell indices (got %d)" % (N, det.numel()))
    return det.contiguous()


def _with_det(t, det):
    """The address of the array that goes with detectors (readings, their tangents or cotangents); the entry points want one even for
    T = 0, where the tensor has no element and no address, and read no row."""
    return None if t is None else C.c_void_p(t.data_ptr() or det.data_ptr())


def _empty_rows(shape, **kw):
    """torch.empty for [T][...] observations, a row allocated even for T = 0."""
    return torch.empty((max(shape[0], 1),) + tuple(shape[1:]), **kw)[:shape[0]]


def _macro_rollout_fwd(desc, T, r, y, u, ueq, ghost, ghost_name, sched, tape, err, out, hist=None, det=None, taps=None):
    """The forward rollout of every form (include/dhts.h): ghost [L][2][4], or with `sched` a schedule [T][L][2][4]; with `det` the
    detector form, which writes `taps` instead of `hist`.  Returns (out, taps)."""
    L, N, T = desc.n_lanes, desc.n_cells, int(T)
    for name, t in (("r", r), ("y", y), ("u", u), ("ueq", ueq)):
        if tuple(t.shape) != (L, N):
            raise ValueError("%s must have shape (%d, %d)" % (name, L, N))
    want = (T, L, 2, 4) if sched else (L, 2, 4)
    if tuple(ghost.shape) != want:
        raise ValueError("%s must have shape %s" % (ghost_name, want))
    if det is not None:
        det = _det_i32(det, N)
    r, y, u, ueq, ghost = (_f32c(t, n) for t, n in ((r, "r"), (y, "y"), (u, "u"), (ueq, "ueq"), (ghost, ghost_name)))
    if sched and T == 0:        # an empty tensor has no address; the entry point wants one and reads no row
        ghost = torch.zeros(1, L, 2, 4, dtype=torch.float32, device=r.device)
    if det is not None:
        D = det.numel()
        taps = _obs_buffer("taps", taps, (T, L, 3, D), r.device, new=_empty_rows)
    if out is None:
        out = tuple(torch.empty_like(r) for _ in range(4))
    args = dict(d=C.byref(desc), T=T, r=_ptr(r), y=_ptr(y), u=_ptr(u), ueq=_ptr(ueq), r_out=_ptr(out[0]), y_out=_ptr(out[1]),
                u_out=_ptr(out[2]), ueq_out=_ptr(out[3]), tape=_ptr(tape), err=_ptr(err), stream=_stream())
    args["ghost_sched" if sched and det is None else "ghost"] = _ptr(ghost)
    if det is not None:
        args.update(ghost_is_sched=int(sched), det=_ptr(det), n_det=D, taps=_with_det(taps, det))
    else:
        args["hist"] = _ptr(hist)
    call("dhts_macro_rollout_fwd" + ("_taps" if det is not None else "_sched" if sched else ""), args)
    return out, taps


def _macro_rollout_bwd(desc, T, tape, g_r, g_y, sched, err, out, g_hist=None, det=None, g_taps=None, g_ghost=None):
    """The reverse sweep of every form: per-step cotangents g_hist [T][L][2][N], or with `det` g_taps [T][L][2][D].  Returns
    (g_r0, g_y0, g_ghost): float64 [L][2][2] summed over the steps, or with `sched` per step [T][L][2][2]."""
    L, N, T = desc.n_lanes, desc.n_cells, int(T)
    if det is not None:
        det = _det_i32(det, N)
        D = det.numel()
        if tuple(g_taps.shape) != (T, L, 2, D):
            raise ValueError("g_taps must have shape (%d, %d, 2, %d)" % (T, L, D))
    g_r, g_y = _f32c(g_r, "g_r"), _f32c(g_y, "g_y")
    if det is not None:
        g_taps = _f32c(g_taps, "g_taps")
        if tuple(g_r.shape) != (L, N) or tuple(g_y.shape) != (L, N):
            raise ValueError("g_r and g_y must have shape (%d, %d)" % (L, N))
    if out is None:
        out = (torch.empty_like(g_r), torch.empty_like(g_y))
    if g_ghost is None and sched:
        g_ghost = torch.empty(max(T, 1), L, 2, 2, dtype=torch.float64, device=g_r.device)      # every row is written
    elif g_ghost is None:
        g_ghost = torch.zeros(L, 2, 2, dtype=torch.float64, device=g_r.device)
    args = dict(d=C.byref(desc), T=T, tape=_ptr(tape), g_r=_ptr(g_r), g_y=_ptr(g_y), g_r_out=_ptr(out[0]), g_y_out=_ptr(out[1]),
                err=_ptr(err), stream=_stream())
    args["g_ghost_sched" if sched and det is None else "g_ghost"] = _ptr(g_ghost)
    if det is not None:
        args.update(ghost_is_sched=int(bool(sched)), det=_ptr(det), n_det=D, g_taps=_with_det(g_taps, det))
    else:
        args["g_hist"] = _ptr(g_hist)
    call("dhts_macro_rollout_bwd" + ("_taps" if det is not None else "_sched" if sched else ""), args)
    return out[0], out[1], (g_ghost[:T] if sched else g_ghost)


def macro_rollout_fwd(desc, T, r, y, u, ueq, ghost, tape=None, hist=None, err=None, out=None):
    """state planes [L][N]; ghost [L][2][4]; returns (r, y, u, ueq) after T steps."""
    return _macro_rollout_fwd(desc, T, r, y, u, ueq, ghost, "ghost", False, tape, err, out, hist=hist)[0]


def macro_rollout_bwd(desc, T, tape, g_r, g_y, g_hist=None, err=None, out=None, g_ghost=None):
    """returns (g_r0, g_y0, g_ghost[L][2][2] float64)."""
    return _macro_rollout_bwd(desc, T, tape, g_r, g_y, False, err, out, g_hist=g_hist, g_ghost=g_ghost)


def macro_rollout_fwd_sched(desc, T, r, y, u, ueq, ghost_sched, tape=None, hist=None, err=None, out=None):
    """macro_rollout_fwd with a boundary schedule: ghost_sched [T][L][2][4], row t read by step t."""
    return _macro_rollout_fwd(desc, T, r, y, u, ueq, ghost_sched, "ghost_sched", True, tape, err, out, hist=hist)[0]


def macro_rollout_bwd_sched(desc, T, tape, g_r, g_y, g_hist=None, err=None, out=None):
    """returns (g_r0, g_y0, g_ghost_sched [T][L][2][2] float64): row t = the cotangent that reaches the boundary cells of step t."""
    return _macro_rollout_bwd(desc, T, tape, g_r, g_y, True, err, out, g_hist=g_hist)


def macro_rollout_fwd_taps(desc, T, r, y, u, ueq, ghost, det, tape=None, err=None, out=None, taps=None):
    """macro_rollout_fwd / _sched with detector taps instead of a history.  ghost [L][2][4], or a schedule [T][L][2][4]; det int32 CUDA
    [D]: cell indices, strictly ascending, in [0, N) (not looked at here: include/dhts.h, index contract).  Returns
    ((r, y, u, ueq) after T steps, taps [T][L][3][D] = (r, y, u) of cell det[j] after every step)."""
    if det is None:
        raise ValueError("det must be a one-dimensional int32 CUDA tensor")
    return _macro_rollout_fwd(desc, T, r, y, u, ueq, ghost, "ghost", ghost.dim() == 4, tape, err, out, det=det, taps=taps)


def macro_rollout_bwd_taps(desc, T, tape, g_r, g_y, det, g_taps, sched=False, err=None, out=None):
    """macro_rollout_bwd / _sched with g_taps [T][L][2][D], the cotangent of (r, y) of the cells det[j] after every step.  Returns
    (g_r0, g_y0, g_ghost): [L][2][2] float64, or the per-step [T][L][2][2] when sched."""
    if det is None:
        raise ValueError("det must be a one-dimensional int32 CUDA tensor")
    return _macro_rollout_bwd(desc, T, tape, g_r, g_y, sched, err, out, det=det, g_taps=g_taps)


_MACRO_PLAN_KEYS = ("fwd_kernel", "fwd_waves", "fwd_passes", "fwd_full_lane", "bwd_pipelined", "bwd_block", "hist", "fwd_lanes_per_group")


def macro_rollout_plan(desc, T, want_hist=False):
    """Which kernel instantiations dhts_macro_rollout_fwd / _bwd launch for this shape (include/dhts.h).
    fwd_kernel: 0 = two-phase lane kernel, 1 = one-phase, 2 = two-phase pair kernel."""
    plan = (C.c_int32 * 8)()
    call("dhts_macro_rollout_plan", d=C.byref(desc), T=int(T), want_hist=int(bool(want_hist)), plan=C.byref(plan))
    return dict(zip(_MACRO_PLAN_KEYS, list(plan)))


def macro_taps_plan(desc, T, n_det):
    """Which kernel instantiations dhts_macro_rollout_fwd_taps / _bwd_taps launch for this shape: the fields of macro_rollout_plan."""
    plan = (C.c_int32 * 8)()
    call("dhts_macro_taps_plan", d=C.byref(desc), T=int(T), n_det=int(n_det), plan=C.byref(plan))
    return dict(zip(_MACRO_PLAN_KEYS, list(plan)))


def macro_tape_expand(desc, T, tape):
    """The reference's blocks dqs (dmacro_lane.py:56) of all T steps from a rollout tape: float32 [T][L][3][Np][4]."""
    Np = raw("dhts_padded", n=desc.n_cells)
    dqs = torch.empty(int(T), desc.n_lanes, 3, Np, 4, dtype=torch.float32, device=tape.device)
    call("dhts_macro_tape_expand", d=C.byref(desc), T=int(T), tape=_ptr(tape), dqs_out=_ptr(dqs), stream=_stream())
    return dqs


def _ghost_ry_to_ru(g_ghost, gr, gu, gq, um, rows=None):
    """ghost (r, y) cotangents (sums over the steps, or per step) -> ghost (r, u) leaves, in double (the sum is ill-conditioned).
    rows (per step only): so many steps at a time into results allocated once -- the same bits, elementwise as it is, and the double
    copies and temporaries are of that many rows instead of T (the checkpointed backward, whose point is what it allocates)."""
    if rows is not None and g_ghost.dim() == 4 and g_ghost.shape[0] > rows:
        g_gr, g_gu = torch.empty_like(gr), torch.empty_like(gu)
        for t in range(0, g_ghost.shape[0], rows):
            g_gr[t:t + rows], g_gu[t:t + rows] = _ghost_ry_to_ru(g_ghost[t:t + rows], gr[t:t + rows], gu[t:t + rows], gq[t:t + rows], um)
        return g_gr, g_gu
    rr, uu, qq = gr.double(), gu.double(), gq.double()
    dueq = torch.where(rr < 0, torch.zeros_like(rr), -um * 0.5 / torch.sqrt(rr.clamp_min(0) + EPS))
    return (g_ghost[..., 0] + g_ghost[..., 1] * ((uu - qq) - rr * dueq)).float(), (g_ghost[..., 1] * rr).float()


def _per_step_cotangent(steps, g_steps, um, rows=None):
    """The cotangent of per-step states [T][L][3][X] (r, y, u; X = N: the history, X = D: detector readings) as the reverse sweep
    takes it, [T][L][2][X]: (r, y) directly, u through the float32 glue of the saved (r, y) of that step.
    rows: so many steps at a time into a result allocated once (the same bits; the five contiguous planes the glue kernel works on are
    of that many rows instead of T: the checkpointed backward)."""
    if rows is not None and steps.shape[0] > rows:
        gs = torch.empty(steps.shape[0], steps.shape[1], 2, steps.shape[3], dtype=torch.float32, device=steps.device)
        for t in range(0, steps.shape[0], rows):
            gs[t:t + rows] = _per_step_cotangent(steps[t:t + rows], g_steps[t:t + rows], um)
        return gs
    sr, sy = steps[:, :, 0].contiguous(), steps[:, :, 1].contiguous()
    g_sr, g_sy = g_steps[:, :, 0].contiguous().clone(), g_steps[:, :, 1].contiguous().clone()
    macro_u_tap_bwd(sr, sy, g_steps[:, :, 2].contiguous(), g_sr, g_sy, um)
    return torch.stack([g_sr, g_sy], dim=2).contiguous()


_GLUE_PASSES, _GLUE_ELEMS = 16, 8192


def _glue_rows(T, row_elems):
    """Steps per pass of the checkpointed backward's glue: at most _GLUE_PASSES passes (their launches stay a small part of a sweep's
    time), and no pass below _GLUE_ELEMS elements (a short rollout takes one).  The glue's temporaries shrink to 1 / 16 of their size."""
    return max(-(-int(T) // _GLUE_PASSES), -(-_GLUE_ELEMS // max(int(row_elems), 1)), 1)


class MacroRollout(torch.autograd.Function):
    """T fused differentiable steps of L independent straight ARZ lanes.

    (r0, u0 [L][N], ghost_r, ghost_u [L][2]) -> (rT, yT, uT, qT [L][N]) (+ hist [T][L][3][N] when asked).
    ghost_r, ghost_u [T][L][2] instead: a boundary schedule, row t set in front of step t; their gradients come back per step.
    det (int32 CUDA [D]): detector readings [T][L][3][D] as the fifth output instead of a history, readings[t][l][:][j] = (r, y, u) of
    cell det[j] after step t; nothing of size [T][L][N] is written, saved or read back then.
    What example/inverse/macro.py does with one dMacroLane in a RoadNetwork (macro.py:34-68,
    _inverse.py:91-99), for L lanes at once: state set by set_state_vector_u, ghosts by
    set_leftmost_cell / set_rightmost_cell, T x RoadNetwork.forward, state read by get_state_vector (at chosen cells: the readings).
    checkpoint (None / False: the taped path; True: the plan's segment length; a positive int: that one): keep (r, y) every so many steps
    instead of the tape, and let the reverse sweep replay one segment at a time with its interface products in LDS (macro_ckpt_plan) --
    the same outputs and gradients bit for bit, and the only buffer that grows with T besides the readings is 8 B per cell per segment.
    Not with want_hist, and not for lanes the reverse kernel's LDS cannot hold (ValueError).  A checkpointed call that requires grad is
    the "MacroRollout" row of _MACRO_CKPT_FORMS: the pair every checkpointed form shares runs it; the taped path is all here.
    """

    @staticmethod
    def forward(ctx, r0, u0, ghost_r, ghost_u, T, dt, dx, u_max, want_hist=False, check_faults=True, det=None, checkpoint=None):
        L, N = r0.shape
        sched = _macro_boundary_form(L, ghost_r, ghost_u, T)
        desc = macro_desc(L, N, dt, dx, u_max)
        segment = _macro_checkpoint_segment(checkpoint, desc, T, want_hist, 0 if det is None else int(det.numel()))
        need_grad = any(t.requires_grad for t in (r0, u0, ghost_r, ghost_u))
        if segment is not None and need_grad:
            return _macro_ckpt_forward(ctx, "MacroRollout", r0, u0, ghost_r, ghost_u, None, T, dt, dx, u_max, check_faults, det, checkpoint,
                                       None, None, segment=segment)
        r0c, u0c, gr, gu, gq, y0, q0, ghost = _macro_leaves(r0, u0, ghost_r, ghost_u, u_max)
        ctx.segment = None
        err = new_error_record(r0.device)
        tape = torch.empty(macro_tape_numel(desc, T), dtype=torch.float32, device=r0.device) if need_grad else None
        if det is not None:
            (rT, yT, uT, qT), steps = macro_rollout_fwd_taps(desc, T, r0c, y0, u0c, q0, ghost, det, tape=tape, err=err)
        else:
            steps = torch.empty(T, L, 3, N, dtype=torch.float32, device=r0.device) if want_hist else None
            fwd = macro_rollout_fwd_sched if sched else macro_rollout_fwd
            rT, yT, uT, qT = fwd(desc, T, r0c, y0, u0c, q0, ghost, tape=tape, hist=steps, err=err)
        if check_faults:
            raise_on_fault(err)
        ctx.sched = sched
        ctx.desc, ctx.T, ctx.u_max, ctx.tape, ctx.check_faults = desc, T, u_max, tape, check_faults
        ctx.save_for_backward(r0c, u0c, gr, gu, gq, rT, yT, steps, det)
        ctx.mark_non_differentiable(qT)
        return (rT, yT, uT, qT) if steps is None else (rT, yT, uT, qT, steps)

    @staticmethod
    def backward(ctx, g_rT, g_yT, g_uT, _g_qT, g_steps=None):
        if ctx.segment is not None:
            return _macro_ckpt_backward(ctx, g_rT, g_yT, g_uT, g_steps)
        r0, u0, gr, gu, gq, rT, yT, steps, det = ctx.saved_tensors
        desc, T, um = ctx.desc, ctx.T, ctx.u_max
        g_r, g_y = _macro_bwd_seeds(rT, yT, g_rT, g_yT, g_uT, um)
        gs = None
        if steps is not None and g_steps is not None and g_steps.numel():      # (T = 0: no row, and an empty tensor has no address)
            gs = _per_step_cotangent(steps, g_steps, um)                         # [T][L][2][N], with detectors [T][L][2][D]
        err = new_error_record(r0.device)
        if gs is not None and det is not None:
            g_r0, g_y0, g_ghost = macro_rollout_bwd_taps(desc, T, ctx.tape, g_r, g_y, det, gs, sched=ctx.sched, err=err)
        else:                            # (no readings to look at: the plain sweep over the same tape)
            bwd = macro_rollout_bwd_sched if ctx.sched else macro_rollout_bwd
            g_r0, g_y0, g_ghost = bwd(desc, T, ctx.tape, g_r, g_y, g_hist=gs, err=err)      # [L][2][2], or [T][L][2][2] per step
        return _macro_bwd_done(ctx, err, (r0, u0, gr, gu, gq), g_r0, g_y0, g_ghost, None) + (None,) * 8


# ---- the checkpointed forms: one row per autograd Function, one forward / backward pair for all of them -------------------
# What the Functions differ in is this table and nothing else.  boundary: "open" (ghost_r, ghost_u [L][2] or a schedule [T][L][2]),
# "ring" (no boundary arguments) or "either" (the call's: ghost_r None is a ring).  raw: the raw layer's form and with it the plan that
# gives the segment -- "plain" (detectors or nothing; macro_ckpt_plan), "target" (the dense fit; macro_ckpt_target_plan) or None (the
# call's: a target is the fit).  sweep_buffers: the reverse sweep's outputs (g_r0, g_y0, g_ghost) are made in forward.  idle_ckpt: the
# checkpoint buffer is allocated even when no leaf requires grad.  release: backward drops the checkpoint buffer and the replay inputs
# (a second backward over a retained graph then fails).  keep_uT: uT is saved for backward also without a fit, which alone reads it.
# nones: the backward's trailing Nones, one per argument of forward behind the leaves.
_MacroForm = collections.namedtuple("_MacroForm", "boundary raw ramps sweep_buffers idle_ckpt release keep_uT nones")
_MACRO_CKPT_FORMS = {
    "MacroRollout":           _MacroForm("open",   "plain",  False, False, False, False, False, 8),
    "MacroRolloutTarget":     _MacroForm("open",   "target", False, True,  False, True,  False, 7),
    "MacroRolloutRing":       _MacroForm("ring",   "plain",  False, False, True,  True,  False, 7),
    "MacroRolloutRingTarget": _MacroForm("ring",   "target", False, False, False, True,  False, 7),
    "MacroRolloutRamp":       _MacroForm("either", None,     True,  False, True,  True,  True,  9),
}


def _macro_ckpt_forward(ctx, name, r0, u0, ghost_r, ghost_u, inflow, T, dt, dx, u_max, check_faults, det, checkpoint, target, ramps,
                        segment=None):
    """The forward of every checkpointed form (name: its row of _MACRO_CKPT_FORMS): the leaves as the kernels read them, the checkpoint
    buffer, the one raw call, the fault check and what backward needs -> (rT, yT, uT, qT[, readings [T][L][3][D] | sse [L][2]]).
    segment: resolved already (MacroRollout, which needs it to choose its path)."""
    form = _MACRO_CKPT_FORMS[name]
    L, N = r0.shape
    ring, raw = ghost_r is None, form.raw or ("plain" if target is None else "target")
    sched = False if ring else _macro_boundary_form(L, ghost_r, ghost_u, T)
    desc = macro_desc(L, N, dt, dx, u_max)
    if segment is None:
        segment = _macro_segment(checkpoint, desc, T, raw, 0 if det is None else int(det.numel()))
    dev = r0.device
    gr = gu = gq = ghost = inf = None
    if ring:
        r0c, u0c = _f32c(r0.detach(), "r0"), _f32c(u0.detach(), "u0")
        y0, q0 = macro_state_from_ru(r0c, u0c, u_max)
    else:
        r0c, u0c, gr, gu, gq, y0, q0, ghost = _macro_leaves(r0, u0, ghost_r, ghost_u, u_max)
    if form.ramps:
        inf = _f32c(inflow.detach(), "inflow")
    need_grad = any(t is not None and t.requires_grad for t in (r0, u0, ghost_r, ghost_u, inflow))
    ckpt = torch.empty(macro_ckpt_numel(desc, T, segment), dtype=torch.float32, device=dev) if need_grad or form.idle_ckpt else None
    err = new_error_record(dev)
    (rT, yT, uT, qT), extra = _macro_ckpt_fwd(raw, desc, T, r0c, y0, u0c, q0, ghost, ckpt, segment, err, None, det, None, target, None,
                                              ramps, inf)
    fit = raw == "target"
    if check_faults:
        raise_on_fault(err)
    if need_grad:
        # the replay reads the forward's inputs again: (y0, q0, ghost) stay alive beside the checkpoints; no tape exists
        ctx.form, ctx.raw, ctx.ckpt, ctx.replay, ctx.target = form, raw, ckpt, (y0, q0, ghost), target
        ctx.desc, ctx.T, ctx.u_max, ctx.segment, ctx.check_faults = desc, T, u_max, segment, check_faults
        ctx.out_bwd = ctx.g_ghost = None
        if form.sweep_buffers:
            ctx.out_bwd = (torch.empty(L, N, dtype=torch.float32, device=dev), torch.empty(L, N, dtype=torch.float32, device=dev))
            if not ring:
                ctx.g_ghost = torch.empty((max(int(T), 1), L, 2, 2) if sched else (L, 2, 2), dtype=torch.float64, device=dev)
        ctx.save_for_backward(r0c, u0c, gr, gu, gq, rT, yT, uT if fit or form.keep_uT else None, None if fit else extra, det, ramps, inf)
    ctx.mark_non_differentiable(qT)
    return (rT, yT, uT, qT) if extra is None else (rT, yT, uT, qT, extra)


def _macro_ckpt_backward(ctx, g_rT, g_yT, g_uT, g_extra):
    """The backward of every checkpointed form: the seeds, the cotangent of the readings (its glue goes over the T-sized arrays a part at
    a time: _glue_rows) or of sse, the one raw call, the glue back to the leaves -> a gradient per argument of the form's forward."""
    form = ctx.form
    r0, u0, gr, gu, gq, rT, yT, uT, steps, det, ramps, inf = ctx.saved_tensors
    desc, T, um = ctx.desc, ctx.T, ctx.u_max
    L, fit = desc.n_lanes, ctx.raw == "target"
    g_r, g_y = _macro_bwd_seeds(rT, yT, g_rT, g_yT, g_uT, um)
    gs = g_sse = None
    if fit:
        g_sse = g_extra.contiguous() if g_extra is not None else None
    elif steps is not None and g_extra is not None and g_extra.numel():      # (T = 0: no row, and an empty tensor has no address)
        gs = _per_step_cotangent(steps, g_extra, um, rows=_glue_rows(T, L * steps.shape[3]))
    err = new_error_record(r0.device)
    y0, q0, ghost = ctx.replay
    g_r0, g_y0, g_ghost, *g_inflow = _macro_ckpt_bwd(
        ctx.raw, desc, T, ctx.ckpt, r0, y0, u0, q0, ghost, g_r, g_y, ctx.segment, err, ctx.out_bwd,
        det if gs is not None else None, gs, ctx.target, g_sse, (rT, yT, uT) if fit else None, ctx.g_ghost, ramps, inf)
    del gs, y0, q0, ghost                # (the sweep is enqueued on this stream: the allocator may hand the blocks to the glue below)
    if form.release:
        ctx.replay = ctx.ckpt = None
    grads = _macro_bwd_done(ctx, err, (r0, u0, gr, gu, gq), g_r0, g_y0, g_ghost, _glue_rows(T, 2 * L))
    if form.boundary == "either" and g_ghost is None:        # (a ring through a forward that has boundary arguments)
        grads += (None, None)
    return grads + tuple(g_inflow) + (None,) * form.nones


class MacroRolloutTarget(torch.autograd.Function):
    """MacroRollout's checkpointed call fitted to an observed space-time field inside the kernels: (r0, u0 [L][N], ghost_r, ghost_u [L][2]
    or a schedule [T][L][2]) -> (rT, yT, uT, qT, sse [L][2] float64), sse[l] = the sums over observed entries of target [T][L][2][N] of
    (x - target)^2 for the density and for the speed after every step (dhts_macro_rollout_fwd_ckpt_target / _bwd_ckpt_target).  No
    [T][L][3][N] history and no cotangent of one exists: the forward accumulates, the reverse sweep forms 2 g_sse (x - target) from the
    state it replays.  Every buffer of both directions is made in forward; without a leaf that requires grad none is."""

    @staticmethod
    def forward(ctx, r0, u0, ghost_r, ghost_u, T, dt, dx, u_max, check_faults, checkpoint, target):
        return _macro_ckpt_forward(ctx, "MacroRolloutTarget", r0, u0, ghost_r, ghost_u, None, T, dt, dx, u_max, check_faults, None,
                                   checkpoint, target, None)

    @staticmethod
    def backward(ctx, g_rT, g_yT, g_uT, _g_qT, g_sse):
        return _macro_ckpt_backward(ctx, g_rT, g_yT, g_uT, g_sse)


class MacroRolloutRing(torch.autograd.Function):
    """MacroRollout's checkpointed call on a closed lane: (r0, u0 [L][N]) -> (rT, yT, uT, qT[, readings [T][L][3][D]]) with cell N - 1 the
    left neighbour of cell 0 (dhts_macro_rollout_fwd_ckpt_ring / _bwd_ckpt_ring).  The dependence of each end on the other is inside the
    kernels: what the sweep sends through an end arrives at the other end in the same step; no boundary cell and no gradient of one
    exists."""

    @staticmethod
    def forward(ctx, r0, u0, T, dt, dx, u_max, check_faults, det, checkpoint):
        return _macro_ckpt_forward(ctx, "MacroRolloutRing", r0, u0, None, None, None, T, dt, dx, u_max, check_faults, det, checkpoint,
                                   None, None)

    @staticmethod
    def backward(ctx, g_rT, g_yT, g_uT, _g_qT, g_steps=None):
        return _macro_ckpt_backward(ctx, g_rT, g_yT, g_uT, g_steps)


class MacroRolloutRingTarget(torch.autograd.Function):
    """MacroRolloutTarget on a closed lane: (r0, u0 [L][N]) -> (rT, yT, uT, qT, sse [L][2] float64)
    (dhts_macro_rollout_fwd_ckpt_target_ring / _bwd_ckpt_target_ring)."""

    @staticmethod
    def forward(ctx, r0, u0, T, dt, dx, u_max, check_faults, checkpoint, target):
        return _macro_ckpt_forward(ctx, "MacroRolloutRingTarget", r0, u0, None, None, None, T, dt, dx, u_max, check_faults, None, checkpoint,
                                   target, None)

    @staticmethod
    def backward(ctx, g_rT, g_yT, g_uT, _g_qT, g_sse):
        return _macro_ckpt_backward(ctx, g_rT, g_yT, g_uT, g_sse)


class MacroRolloutRamp(torch.autograd.Function):
    """The checkpointed rollout with on-ramps (dhts_macro_rollout_*_ckpt_ramp), every form of it: (r0, u0 [L][N], ghost_r,
    ghost_u [L][2], a schedule [T][L][2] or None: a ring, inflow [T][L][R]) -> (rT, yT, uT, qT[, readings [T][L][3][D] | sse [L][2]]).
    inflow is a leaf like the others: its gradient comes back float32 [T][L][R], written by the reverse sweep itself."""

    @staticmethod
    def forward(ctx, r0, u0, ghost_r, ghost_u, inflow, T, dt, dx, u_max, check_faults, det, checkpoint, target, ramps):
        return _macro_ckpt_forward(ctx, "MacroRolloutRamp", r0, u0, ghost_r, ghost_u, inflow, T, dt, dx, u_max, check_faults, det, checkpoint,
                                   target, ramps)

    @staticmethod
    def backward(ctx, g_rT, g_yT, g_uT, _g_qT, g_extra=None):
        return _macro_ckpt_backward(ctx, g_rT, g_yT, g_uT, g_extra)


def _macro_ramp_checks(r0, T, ramps, inflow, want_hist, checkpoint):
    """Every ValueError of dhts.macro_rollout's `ramps` / `inflow`, raised before anything touches a device -> the cells (a list, or the
    CUDA tensor as it is), or None without ramps."""
    if (ramps is None) != (inflow is None):
        raise ValueError("ramps and inflow go together: the cells, and inflow [T][L][R] with the rate each of them gets in every step "
                         "(target= and checkpoint= are passed by keyword: they stay the last two arguments)")
    if ramps is None:
        return None
    if isinstance(inflow, (bool, int)) or (isinstance(ramps, torch.Tensor) and ramps.dim() == 4):
        # (what a caller gets who hands target and checkpoint over by position, where ramps and inflow now stand in front of them)
        raise ValueError("ramps must be cell indices and inflow a float32 tensor [T][L][R] (got %s and %s): target= and checkpoint= are "
                         "passed by keyword" % (type(ramps).__name__, type(inflow).__name__))
    if checkpoint is None or checkpoint is False:
        raise ValueError("ramps live on the checkpointed path only: pass checkpoint=True (or a segment length)")
    if want_hist:
        raise ValueError("ramps do not take want_hist: pass target= for the dense fit, or detectors= for the readings")
    if r0.dim() != 2:
        raise ValueError("r0 must be [L][N]")
    L, N = int(r0.shape[0]), int(r0.shape[1])
    cells = _detector_cells(ramps, N, "ramps")
    R = cells.numel() if isinstance(cells, torch.Tensor) else len(cells)
    if not isinstance(inflow, torch.Tensor) or inflow.dtype != torch.float32 or tuple(inflow.shape) != (int(T), L, R):
        raise ValueError("inflow must be a float32 tensor of shape (T, L, R) = (%d, %d, %d)" % (int(T), L, R))
    if inflow.device != r0.device:
        raise ValueError("inflow must live on r0's device (%s), not %s" % (r0.device, inflow.device))
    return cells


def _macro_ring_checks(ring, ghost_r, ghost_u, t_ghost_r=None, t_ghost_u=None, want_hist=False, checkpoint=None, fused=None, r0=None,
                       u0=None):
    """Every ValueError of `ring=True` of dhts.macro_rollout (fused None) and dhts.macro_rollout_jvp (checkpoint None), raised before
    anything touches a device.  Without `ring` nothing is checked here but `ring` itself: it is a bool (whoever hands `target` or
    `checkpoint` over by position, where `ring` now stands in front of them, is told so instead of getting another rollout)."""
    if not isinstance(ring, bool):
        raise ValueError("ring must be True or False (got %s): target= and checkpoint= are passed by keyword" % type(ring).__name__)
    if not ring:
        return
    if fused is None and (checkpoint is None or checkpoint is False):
        raise ValueError("ring lives on the checkpointed path only: pass checkpoint=True (or a segment length)")
    if fused is not None and not fused:
        raise ValueError("ring lives on the fused forward + tangent kernel only: pass fused=True")
    if ghost_r is not None or ghost_u is not None:
        raise ValueError("ghost_r and ghost_u must be None when ring: a closed lane has no boundary cells")
    if t_ghost_r is not None or t_ghost_u is not None:
        raise ValueError("t_ghost_r and t_ghost_u must be None when ring: a closed lane has no boundary cells")
    if want_hist:
        raise ValueError("ring does not take want_hist: pass target= for the dense fit, or detectors=range(N) for every cell's readings")
    if r0 is not None and (r0.dim() != 2 or tuple(u0.shape) != tuple(r0.shape)):
        raise ValueError("r0 must be [L][N] and u0 must have its shape (got %s and %s)" % (tuple(r0.shape), tuple(u0.shape)))


# ---- what the macro autograd Functions (and dhts.jvp.macro_rollout_jvp) share: the leaves, the backward's seeds and tail, the segment ----
def _macro_boundary_form(L, ghost_r, ghost_u, T):
    """-> whether (ghost_r, ghost_u) are a schedule [T][L][2] (else [L][2]); ValueError for anything else."""
    sched = ghost_r.dim() == 3
    if ghost_r.dim() != ghost_u.dim() or ghost_r.dim() not in (2, 3):
        raise ValueError("ghost_r and ghost_u must both be [L][2] or both [T][L][2]")
    want = (int(T), L, 2) if sched else (L, 2)
    if tuple(ghost_r.shape) != want or tuple(ghost_u.shape) != want:
        raise ValueError("ghost_r and ghost_u must have shape %s (got %s and %s)" % (want, tuple(ghost_r.shape), tuple(ghost_u.shape)))
    return sched


def _macro_leaves(r0, u0, ghost_r, ghost_u, u_max):
    """The leaves as the kernels read them -> (r0c, u0c, gr, gu, gq, y0, q0, ghost): detached contiguous float32, y and the equilibrium
    speed of the state and of the boundary cells, ghost = (r, y, u, ueq) stacked, [L][2][4] or [T][L][2][4]."""
    r0c, u0c = _f32c(r0.detach(), "r0"), _f32c(u0.detach(), "u0")
    gr, gu = _f32c(ghost_r.detach(), "ghost_r"), _f32c(ghost_u.detach(), "ghost_u")
    y0, q0 = macro_state_from_ru(r0c, u0c, u_max)
    gy, gq = macro_state_from_ru(gr, gu, u_max) if gr.numel() else (gr.clone(), gr.clone())
    return r0c, u0c, gr, gu, gq, y0, q0, torch.stack([gr, gy, gu, gq], dim=-1).contiguous()


def _macro_bwd_seeds(rT, yT, g_rT, g_yT, g_uT, um):
    """The cotangents of (rT, yT, uT) -> fresh (g_r, g_y) for the reverse sweep, uT's folded in through the speed's glue."""
    g_r = g_rT.contiguous().clone() if g_rT is not None else torch.zeros_like(rT)
    g_y = g_yT.contiguous().clone() if g_yT is not None else torch.zeros_like(rT)
    if g_uT is not None:
        macro_u_tap_bwd(rT, yT, g_uT.contiguous(), g_r, g_y, um)
    return g_r, g_y


def _macro_bwd_done(ctx, err, leaves, g_r0, g_y0, g_ghost, rows):
    """The fault check and the glue back to the leaves -> (g_r0, g_u0, g_ghost_r, g_ghost_u), or with g_ghost None (a ring: no boundary
    cells) (g_r0, g_u0); rows: _ghost_ry_to_ru's."""
    r0, u0, gr, gu, gq = leaves
    if ctx.check_faults:             # reading the record back synchronises: off inside HIP-graph capture
        raise_on_fault(err)
    g_u0 = macro_state_from_ru_bwd(r0, u0, g_y0, g_r0, ctx.u_max)
    if g_ghost is None:
        return g_r0, g_u0
    return (g_r0, g_u0) + _ghost_ry_to_ru(g_ghost, gr, gu, gq, ctx.u_max, rows=rows)


def _macro_segment(checkpoint, desc, T, form, n_det=0):
    """dhts.macro_rollout's `checkpoint` -> the segment length of the form's plan ("target": the target forms' own); ValueError otherwise."""
    def plan(segment):
        ask = (lambda sg: macro_ckpt_target_plan(desc, T, sg)) if form == "target" else (lambda sg: macro_ckpt_plan(desc, T, n_det, sg))
        if ask(0)["max_segment"] >= 1:
            return ask(segment)
        if form == "target":
            raise ValueError("lanes of %d cells do not fit the target forms of the checkpointed sweep (the reverse LDS of the target plan "
                             "holds up to %d cells): fit the want_hist=True history instead" % (desc.n_cells, MACRO_CKPT_TARGET_MAX_CELLS))
        raise ValueError("lanes of %d cells do not fit the checkpointed reverse sweep (its LDS holds up to %d cells): "
                         "use the taped path, checkpoint=None" % (desc.n_cells, MACRO_CKPT_MAX_CELLS))
    return _checkpoint_segment(checkpoint, plan)


def _macro_target_checks(r0, T, dt, dx, u_max, target, want_hist, detectors, checkpoint):
    """Every ValueError of dhts.macro_rollout's `target`, raised before anything touches a device."""
    if checkpoint is None or checkpoint is False:
        raise ValueError("target lives on the checkpointed path only: pass checkpoint=True (or a segment length)")
    if want_hist:
        raise ValueError("target does not take want_hist: the history is what target= does without")
    if detectors is not None:
        raise ValueError("target does not take detectors: it is the dense fit (NaN entries of target are the unobserved ones)")
    if r0.dim() != 2:
        raise ValueError("r0 must be [L][N]")
    L, N = int(r0.shape[0]), int(r0.shape[1])
    if not isinstance(target, torch.Tensor) or target.dtype != torch.float32 or tuple(target.shape) != (int(T), L, 2, N):
        raise ValueError("target must be a float32 tensor of shape (T, L, 2, N) = (%d, %d, 2, %d)" % (int(T), L, N))
    if target.device != r0.device:
        raise ValueError("target must live on r0's device (%s), not %s" % (r0.device, target.device))
    if not target.is_contiguous():
        raise ValueError("target must be contiguous: a copy of it is as large as the history it replaces")
    if target.requires_grad:
        raise ValueError("target is data and not differentiable: pass it detached")
    _macro_segment(checkpoint, macro_desc(L, N, float(dt), float(dx), float(u_max)), int(T), "target")


def _macro_checkpoint_segment(checkpoint, desc, T, want_hist, n_det):
    """dhts.macro_rollout's `checkpoint` -> None (the taped path) or the segment length; ValueError otherwise, before a device is touched."""
    if checkpoint is None or checkpoint is False:
        return None
    segment = _macro_segment(checkpoint, desc, T, "plain", n_det)
    if want_hist:
        raise ValueError("want_hist and checkpoint exclude each other: the history is of size T anyway (checkpoint=None keeps the tape)")
    return segment


def _detector_indices(detectors, N, device):
    """dhts.macro_rollout's `detectors` -> int32 CUDA [D].  A sequence of ints or a CPU integer tensor is validated (ValueError) before
    anything touches a device; a CUDA int32 tensor is used as it is."""
    cells = _detector_cells(detectors, N)
    return cells if isinstance(cells, torch.Tensor) else torch.tensor(cells, dtype=torch.int32, device=device)


def _detector_cells(detectors, N, name="detectors"):
    """The checks of _detector_indices without the upload -> the CUDA tensor as it is, or the list of cells.  name: what the messages call
    the argument (`ramps` of dhts.macro_rollout is a list of cells of the same kind)."""
    if isinstance(detectors, torch.Tensor) and detectors.is_cuda:
        if detectors.dtype != torch.int32 or detectors.dim() != 1 or not 1 <= detectors.numel() <= N:
            raise ValueError("a CUDA `%s` must be a one-dimensional int32 tensor of 1..%d entries" % (name, N))
        return detectors.contiguous()
    if isinstance(detectors, torch.Tensor):
        if detectors.dim() != 1 or detectors.dtype.is_floating_point or detectors.dtype.is_complex or detectors.dtype == torch.bool:
            raise ValueError("`%s` must be a one-dimensional integer tensor" % name)
        cells = detectors.tolist()
    else:
        cells = list(detectors)
        if any(isinstance(c, bool) or int(c) != c for c in cells):
            raise ValueError("`%s` must hold integers" % name)
        cells = [int(c) for c in cells]
    if not cells:
        raise ValueError("`%s` is empty" % name)
    if cells[0] < 0 or cells[-1] >= N or any(a >= b for a, b in zip(cells, cells[1:])) or any(not 0 <= c < N for c in cells):
        raise ValueError("`%s` must be strictly ascending cell indices in [0, %d) (got %s)" % (name, N, cells))
    return cells


def macro_rollout(r0, u0, ghost_r, ghost_u, T, dt, dx, u_max, want_hist=False, check_faults=True, detectors=None, ring=False,
                  ramps=None, inflow=None, target=None, checkpoint=None):
    """T fused differentiable steps of L straight ARZ lanes (MacroRollout): returns (rT, yT, uT, qT), with want_hist also hist [T][L][3][N].
    checkpoint=None: the taped reverse mode; True or a segment length: the checkpointed one (same bits, no tape; MacroRollout).

    detectors: cell indices at which the state is read after every step -- a sequence of ints or a CPU integer tensor (non-empty, strictly
    ascending, in [0, N): checked, ValueError otherwise, then uploaded), or a CUDA int32 tensor, which is used as it is so that a graph
    capture sees no upload and no synchronisation and which is therefore NOT validated: the kernels skip an index outside [0, N) (its
    column of the readings stays unwritten) and never form an address from one.  Returns (rT, yT, uT, qT, readings) then, readings
    [T][L][3][D] = (r, y, u) of cell detectors[j] after every step, differentiable in all three; no [T][L][N] history is written or
    read.  Not together with want_hist (ValueError): a caller who wants every cell has the history.

    target (with checkpoint only; not with want_hist or detectors): the observed field, float32 [T][L][2][N] on r0's device, contiguous,
    not requiring grad -- target[t][l][0][k] the density of cell k after step t (hist[t][l][0][k]), target[t][l][1][k] the speed
    (hist[t][l][2][k]), NaN = not observed.  Returns (rT, yT, uT, qT, sse) then: sse float64 [L][2], per lane the sum of the squared
    float32 density residuals and of the squared speed residuals, differentiable; the kernels read target themselves and neither a
    history nor its cotangent exists (MacroRolloutTarget).  The segment is that of macro_ckpt_target_plan.

    ring=True (with checkpoint only; ghost_r and ghost_u None; not with want_hist): the lane is closed, cell N - 1 is the left neighbour
    of cell 0 and the circumference is N dx (MacroRolloutRing, MacroRolloutRingTarget).  detectors and target as above.  The
    lane's mass sum_k r[k] is conserved up to the float32 store of each cell, and the gradient carries the dependence of each end on the
    other.

    ramps with inflow (with checkpoint only; not with want_hist; with ring=True or either boundary form, and with detectors, target or
    neither): on-ramps.  ramps: cell indices shared by all lanes, validated exactly as detectors are (a CUDA int32 tensor is used as it
    is; an index outside [0, N) then names no cell).  inflow: float32 [T][L][R] on r0's device, inflow[t][l][j] the density rate
    (normalised density per second) cell ramps[j] of lane l gets in step t, added behind the step's own float32 store as
    (float)((double)r + dt (double)inflow) with y unchanged; a negative entry is an off-ramp, nothing is clamped.  The
    return tuple is the form's own; inflow is a differentiable leaf and inflow.grad is float32 [T][L][R] (MacroRolloutRamp)."""
    # every form's checks, each ValueError where it has always stood and all of them before anything touches a device ...
    _macro_ring_checks(ring, ghost_r, ghost_u, want_hist=want_hist, checkpoint=checkpoint, r0=r0, u0=u0)
    cells = _macro_ramp_checks(r0, T, ramps, inflow, want_hist, checkpoint)
    desc = det = None
    if cells is not None:                # (the on-ramp forms look at the lane's size first)
        desc = macro_desc(int(r0.shape[0]), int(r0.shape[1]), float(dt), float(dx), float(u_max))
    if target is not None:               # (... which end with the segment of the target forms' plan)
        _macro_target_checks(r0, T, dt, dx, u_max, target, want_hist, detectors, checkpoint)
    else:
        if detectors is not None:
            if want_hist:
                raise ValueError("want_hist and detectors exclude each other: the history holds every cell")
            det = _detector_cells(detectors, int(r0.shape[-1]))
        if checkpoint is not None and checkpoint is not False and r0.dim() == 2:      # (ValueError before the detectors are uploaded)
            if desc is None:
                desc = macro_desc(int(r0.shape[0]), int(r0.shape[1]), float(dt), float(dx), float(u_max))
            _macro_checkpoint_segment(checkpoint, desc, int(T), want_hist, 0 if det is None else len(det))
    if cells is not None and not ring:
        _macro_boundary_form(int(r0.shape[0]), ghost_r, ghost_u, int(T))
    # ... the uploads, and the form's Function
    if isinstance(det, list):
        det = torch.tensor(det, dtype=torch.int32, device=r0.device)
    if isinstance(cells, list):
        cells = torch.tensor(cells, dtype=torch.int32, device=r0.device)
    size = (int(T), float(dt), float(dx), float(u_max))
    if cells is not None:
        return MacroRolloutRamp.apply(r0, u0, ghost_r, ghost_u, inflow, *size, check_faults, det, checkpoint, target, cells)
    if ring and target is not None:
        return MacroRolloutRingTarget.apply(r0, u0, *size, check_faults, checkpoint, target)
    if ring:
        return MacroRolloutRing.apply(r0, u0, *size, check_faults, det, checkpoint)
    if target is not None:
        return MacroRolloutTarget.apply(r0, u0, ghost_r, ghost_u, *size, check_faults, checkpoint, target)
    return MacroRollout.apply(r0, u0, ghost_r, ghost_u, *size, want_hist, check_faults, det, checkpoint)


# ---- forward mode: Jacobian-vector products over the rollout tape ---------------------------------------------------------------------
def macro_state_from_ru_jvp(r, u, t_r, t_u, u_max):
    """t_y = (dy/dr) t_r + (dy/du) t_u of y = r (u - u_eq(r)), elementwise; all four of one shape."""
    r, u, t_r, t_u = (_f32c(t, n) for t, n in ((r, "r"), (u, "u"), (t_r, "t_r"), (t_u, "t_u")))
    if not (r.shape == u.shape == t_r.shape == t_u.shape):
        raise ValueError("r, u, t_r and t_u must have one shape")
    t_y = torch.empty_like(r)
    call("dhts_macro_state_from_ru_jvp", n=r.numel(), u_max=float(u_max), r=_ptr(r), u=_ptr(u), t_r=_ptr(t_r), t_u=_ptr(t_u), t_y=_ptr(t_y),
         stream=_stream())
    return t_y


def macro_u_tap_jvp(r, y, t_r, t_y, u_max):
    """t_u = (du/dr) t_r + (du/dy) t_y of the speed tap u = y / max(r, eps) + u_eq(max(r, eps)), elementwise; all four of one shape."""
    r, y, t_r, t_y = (_f32c(t, n) for t, n in ((r, "r"), (y, "y"), (t_r, "t_r"), (t_y, "t_y")))
    if not (r.shape == y.shape == t_r.shape == t_y.shape):
        raise ValueError("r, y, t_r and t_y must have one shape")
    t_u = torch.empty_like(r)
    call("dhts_macro_u_tap_jvp", n=r.numel(), u_max=float(u_max), r=_ptr(r), y=_ptr(y), t_r=_ptr(t_r), t_y=_ptr(t_y), t_u=_ptr(t_u),
         stream=_stream())
    return t_u


def _macro_directions(desc, t_r, t_y):
    """The two tangent wrappers' check of (t_r, t_y) -> K."""
    L, N = desc.n_lanes, desc.n_cells
    if t_r.dim() != 3 or tuple(t_r.shape[1:]) != (L, N) or t_r.shape[0] < 1 or t_y.shape != t_r.shape:
        raise ValueError("t_r and t_y must have shape (K, %d, %d) with K >= 1" % (L, N))
    return int(t_r.shape[0])


def _macro_t_ghost(t_ghost, want, message):
    """... of t_ghost against the shape `want` (ValueError(message)) -> contiguous, or None: zero boundary tangents."""
    if t_ghost is None:
        return None
    if tuple(t_ghost.shape) != want:
        raise ValueError(message)
    t_ghost = _f32c(t_ghost, "t_ghost")
    return t_ghost if t_ghost.numel() else None          # (a schedule of no steps: no row, and an empty tensor has no address)


def _macro_readings(desc, T, K, det, device, without, t_taps, taps=None, primal=False):
    """... of det and the readings -> (det, D, taps, t_taps): with det t_taps [K][T][L][2][D] and, for `primal`, taps [T][L][3][D] are
    checked or made; without det, handing one in is ValueError(without)."""
    if det is None:
        if taps is not None or t_taps is not None:
            raise ValueError(without)
        return None, 0, None, None
    L, det = desc.n_lanes, _det_i32(det, desc.n_cells)
    D = det.numel()
    if primal:
        taps = _obs_buffer("taps", taps, (T, L, 3, D), device, new=torch.empty)
    return det, D, taps, _obs_buffer("t_taps", t_taps, (K, T, L, 2, D), device, new=torch.empty)


def macro_rollout_jvp(desc, T, tape, t_r, t_y, t_ghost=None, det=None, err=None, out=None, t_taps=None):
    """The tangent sweep over a rollout tape (include/dhts.h): t_r, t_y [K][L][N]; t_ghost None (zero), [K][L][2][2] (the same tangent in
    front of every step) or a schedule [K][T][L][2][2], (left, right) x (r, y); det int32 CUDA [D] or None.  Returns (t_rT, t_yT, t_taps):
    t_taps [K][T][L][2][D] = the tangent of (r, y) of cell det[j] after every step, None without det."""
    L, N, T = desc.n_lanes, desc.n_cells, int(T)
    K = _macro_directions(desc, t_r, t_y)
    t_r, t_y = _f32c(t_r, "t_r"), _f32c(t_y, "t_y")
    sched = t_ghost is not None and t_ghost.dim() == 5
    t_ghost = _macro_t_ghost(t_ghost, (K, T, L, 2, 2) if sched else (K, L, 2, 2),
                             "t_ghost must have shape (%d, %d, 2, 2) or (%d, %d, %d, 2, 2)" % (K, L, K, T, L))
    sched = sched and t_ghost is not None
    det, D, _, t_taps = _macro_readings(desc, T, K, det, t_r.device, "t_taps without det", t_taps)
    if T > 0 and tape is None:
        raise ValueError("a sweep of T > 0 steps needs the rollout's tape")
    if out is None:
        out = (torch.empty_like(t_r), torch.empty_like(t_y))
    call("dhts_macro_rollout_jvp", d=C.byref(desc), T=T, tape=_ptr(tape), n_dir=K, t_r=_ptr(t_r), t_y=_ptr(t_y), t_ghost=_ptr(t_ghost),
         ghost_is_sched=int(sched), t_r_out=_ptr(out[0]), t_y_out=_ptr(out[1]), det=_ptr(det), n_det=D, t_taps=_with_det(t_taps, det),
         err=_ptr(err), stream=_stream())
    return out[0], out[1], t_taps


_MACRO_JVP_PLAN_KEYS = ("kernel", "block", "dirs_per_launch", "launches")


def macro_jvp_plan(desc, T, n_dir, n_det=0):
    """What dhts_macro_rollout_jvp launches for this shape: kernel 0 = general, 1 = fast; its block; the directions of the widest launch;
    the number of launches (0 for T = 0)."""
    plan = (C.c_int32 * 8)()
    call("dhts_macro_jvp_plan", d=C.byref(desc), T=int(T), n_dir=int(n_dir), n_det=int(n_det), plan=C.byref(plan))
    return dict(zip(_MACRO_JVP_PLAN_KEYS, list(plan)))


_MACRO_FWD_JVP_PLAN_KEYS = ("waves", "passes", "dirs_per_launch", "launches", "lds_bytes")


def macro_rollout_fwd_jvp(desc, T, r, y, u, ueq, ghost, t_r, t_y, t_ghost=None, det=None, err=None, err_jvp=None, out=None, taps=None,
                          t_taps=None, ramps=None, inflow=None, t_inflow=None):
    """The rollout and K tangent directions of it in one kernel, no tape (dhts_macro_rollout_fwd_jvp, include/dhts.h): what
    macro_rollout_fwd / _fwd_sched / _fwd_taps followed by macro_rollout_jvp returns, bit for bit.  r, y, u, ueq [L][N]; ghost [L][2][4]
    or a schedule [T][L][2][4]; t_r, t_y [K][L][N]; t_ghost None (zero), [K][L][2][2], or [K][T][L][2][2] beside a schedule; det int32
    CUDA [D] or None.  err: the forward's fault record (CFL), err_jvp: the tangent sweep's (the earliest non-finite tangent); each may be
    None.  out: (r_out, y_out, u_out, ueq_out, t_r_out, t_y_out) buffers to fill; taps [T][L][3][D] and t_taps [K][T][L][2][D] are
    allocated with det unless handed in.  A lane the plan cannot take is a ValueError before anything is launched.
    ramps int32 CUDA [R] with inflow float32 [T][L][R]: DESIGN 4m's source behind every step (dhts_macro_rollout_fwd_jvp_ramp /
    _ring_ramp), and t_inflow None (zero) or float32 [K][T][L][R] its tangent per direction.
    Returns ((rT, yT, uT, qT, taps), (t_rT, t_yT, t_taps)), the readings None without det."""
    L, N, T = desc.n_lanes, desc.n_cells, int(T)
    if T < 0:
        raise ValueError("T must be >= 0")
    if (ramps is None) != (inflow is None):
        raise ValueError("ramps and inflow go together")
    if t_inflow is not None and ramps is None:
        raise ValueError("t_inflow without ramps")
    for name, t in (("r", r), ("y", y), ("u", u), ("ueq", ueq)):
        if tuple(t.shape) != (L, N):
            raise ValueError("%s must have shape (%d, %d)" % (name, L, N))
    ring = ghost is None             # (macro_rollout_fwd_jvp_ring)
    sched = not ring and ghost.dim() == 4
    want = (T, L, 2, 4) if sched else (L, 2, 4)
    if not ring and tuple(ghost.shape) != want:
        raise ValueError("ghost must have shape (%d, 2, 4) or (%d, %d, 2, 4)" % (L, T, L))
    if ring and t_ghost is not None:
        raise ValueError("a ring has no boundary cells and no t_ghost")
    K = _macro_directions(desc, t_r, t_y)
    if macro_fwd_jvp_plan(desc, T, K)["dirs_per_launch"] < 1:
        raise ValueError("a lane of %d cells does not fit the fused forward + tangent kernel (its records, the interface products and "
                         "the tangent copies exceed the LDS of a workgroup); fused=False, the taped pair, covers it" % N)
    r, y, u, ueq = (_f32c(t, n) for t, n in ((r, "r"), (y, "y"), (u, "u"), (ueq, "ueq")))
    ghost = None if ring else _f32c(ghost, "ghost")
    t_r, t_y = _f32c(t_r, "t_r"), _f32c(t_y, "t_y")
    if sched and T == 0:        # an empty tensor has no address; the entry point wants one and reads no row
        ghost = torch.zeros(1, L, 2, 4, dtype=torch.float32, device=r.device)
    want = (K, T, L, 2, 2) if sched else (K, L, 2, 2)
    t_ghost = _macro_t_ghost(t_ghost, want, "t_ghost must have shape %s: it follows the form of ghost" % (want,))
    det, D, taps, t_taps = _macro_readings(desc, T, K, det, r.device, "taps / t_taps without det", t_taps, taps, primal=True)
    if out is not None:
        out = tuple(out)
        if len(out) != 6:
            raise ValueError("out must be (r_out, y_out, u_out, ueq_out, t_r_out, t_y_out)")
    out = _state_out(("r_out", "y_out", "u_out", "ueq_out", "t_r_out", "t_y_out"), out, (r, y, u, ueq, t_r, t_y))
    if ramps is not None:
        ramps, R, inflow = _macro_ramp_args(desc, T, ramps, inflow)
        if t_inflow is not None:
            if not isinstance(t_inflow, torch.Tensor) or tuple(t_inflow.shape) != (K, T, L, R):
                raise ValueError("t_inflow must have shape (%d, %d, %d, %d): the directions of t_r, then the shape of inflow" % (K, T, L, R))
            t_inflow = _f32c(t_inflow, "t_inflow")
    args = dict(d=C.byref(desc), T=T, n_dir=K, r=_ptr(r), y=_ptr(y), u=_ptr(u), ueq=_ptr(ueq), t_r=_ptr(t_r), t_y=_ptr(t_y),
                r_out=_ptr(out[0]), y_out=_ptr(out[1]), u_out=_ptr(out[2]), ueq_out=_ptr(out[3]), t_r_out=_ptr(out[4]), t_y_out=_ptr(out[5]),
                det=_ptr(det), n_det=D, taps=_with_det(taps, det), t_taps=_with_det(t_taps, det), err=_ptr(err), err_jvp=_ptr(err_jvp),
                stream=_stream())
    if not ring:
        args.update(ghost=_ptr(ghost), ghost_is_sched=int(sched), t_ghost=_ptr(t_ghost))
    if ramps is not None:
        args.update(ramps=_ptr(ramps), n_ramp=R, inflow=_data(inflow), t_inflow=_data(t_inflow))
    call("dhts_macro_rollout_fwd_jvp" + ("_ring" if ring else "") + ("_ramp" if ramps is not None else ""), args)
    return (out[0], out[1], out[2], out[3], taps), (out[4], out[5], t_taps)


def macro_fwd_jvp_plan(desc, T, n_dir, n_det=0):
    """What dhts_macro_rollout_fwd_jvp launches for this shape: the lane kernel's wavefronts per lane and passes per wavefront, the
    direction slots of the widest launch (0: the lane does not fit), the number of launches (0 for T = 0 or when nothing fits) and the
    widest launch's dynamic LDS bytes.  Needs no device."""
    plan = (C.c_int32 * 8)()
    call("dhts_macro_fwd_jvp_plan", d=C.byref(desc), T=int(T), n_dir=int(n_dir), n_det=int(n_det), plan=C.byref(plan))
    return dict(zip(_MACRO_FWD_JVP_PLAN_KEYS, list(plan)))


# ---- reverse mode from checkpoints: the interface products of one segment at a time, in LDS -------------------------------------------
MACRO_CKPT_MAX_CELLS = 1319      # the longest lane whose records, planes and one ring step fit 160 KB (csrc/macro_ckpt.inc; the plan is the truth)
_MACRO_CKPT_PLAN_KEYS = ("waves", "passes", "segment", "max_segment", "checkpoints", "fwd_lds_bytes", "bwd_lds_bytes", "bwd_groups_per_cu")


def macro_ckpt_plan(desc, T, n_det=0, segment=0):
    """What dhts_macro_rollout_fwd_ckpt / _bwd_ckpt launch for this shape (include/dhts.h): the lane mapping's wavefronts and passes, the
    segment length used (the plan's own for segment = 0), the longest one the reverse kernel's LDS holds, the number of checkpoints
    ceil(T / segment), the dynamic LDS bytes of the two kernels and the reverse workgroups a CU holds by LDS.  A lane too long for the
    reverse kernel reports max_segment = 0 (and segment = 0).  ValueError: a segment outside 0 .. max_segment.  Needs no device."""
    return _macro_ckpt_plan("dhts_macro_ckpt_plan", "max_segment", desc, (T, n_det), segment)


def _macro_ckpt_plan(entry, forms, desc, shape, segment):
    """macro_ckpt_plan (shape = (T, n_det)) and macro_ckpt_target_plan (shape = (T,), forms "the max_segment of the target forms")."""
    plan = (C.c_int32 * 8)()
    if not 0 <= int(segment) <= 0x7fffffff:
        raise ValueError("segment must be 0 (the plan's choice) or a positive int")
    args = dict(zip(("T", "n_det"), (int(v) for v in shape)), d=C.byref(desc), plan=C.byref(plan))
    status = raw(entry, dict(args, segment=int(segment)))
    if status == _lib.E_INVALID and int(segment) and raw(entry, dict(args, segment=0)) == 0:
        # the plan's own segment is accepted, so the descriptor, T and n_det are good and it is the segment that is not
        raise ValueError("segment must be 0 (the plan's choice) or 1 .. %s (%d) for lanes of %d cells" % (forms, plan[3], desc.n_cells))
    check(status, entry)
    return dict(zip(_MACRO_CKPT_PLAN_KEYS, list(plan)))


def macro_ckpt_numel(desc, T, segment=0):
    """float32 elements of the checkpoint buffer (opaque: the float32 (r, y) of every cell every `segment` steps, include/dhts.h)."""
    return raw("dhts_macro_ckpt_bytes", d=C.byref(desc), T=int(T), segment=int(segment)) // 4


def _macro_ckpt_args(desc, T, segment, ckpt, r, y, u, ueq, ghost):
    """What both raw wrappers check of the arguments they share -> (sched, contiguous r, y, u, ueq, ghost).  ghost None: a ring (the
    _ring wrappers), which has no boundary cells; it comes back as None."""
    L, N, T = desc.n_lanes, desc.n_cells, int(T)
    if macro_ckpt_plan(desc, T, 0, segment)["max_segment"] < 1:
        raise ValueError("lanes of %d cells do not fit the checkpointed reverse sweep: use the taped path (checkpoint=None)" % N)
    if ckpt.dtype != torch.float32 or ckpt.numel() != macro_ckpt_numel(desc, T, segment) or not ckpt.is_contiguous():
        raise ValueError("ckpt must be a contiguous float32 [macro_ckpt_numel(desc, T, segment)]")
    for name, t in (("r", r), ("y", y), ("u", u), ("ueq", ueq)):
        if tuple(t.shape) != (L, N):
            raise ValueError("%s must have shape (%d, %d)" % (name, L, N))
    if ghost is None:
        return (False,) + tuple(_f32c(t, n) for t, n in ((r, "r"), (y, "y"), (u, "u"), (ueq, "ueq"))) + (None,)
    sched = ghost.dim() == 4
    want = (T, L, 2, 4) if sched else (L, 2, 4)
    if tuple(ghost.shape) != want:
        raise ValueError("ghost must have shape (%d, 2, 4) or, a schedule, (%d, %d, 2, 4)" % (L, T, L))
    r, y, u, ueq, ghost = (_f32c(t, n) for t, n in ((r, "r"), (y, "y"), (u, "u"), (ueq, "ueq"), (ghost, "ghost")))
    if sched and T == 0:        # an empty tensor has no address; the entry point wants one and reads no row
        ghost = torch.zeros(1, L, 2, 4, dtype=torch.float32, device=r.device)
    return sched, r, y, u, ueq, ghost


def _macro_ramp_args(desc, T, ramps, inflow, g_inflow=None, reverse=False):
    """What both raw wrappers check of the on-ramp arguments -> (ramps, R, inflow[, g_inflow]); g_inflow None: a new one."""
    L, N = desc.n_lanes, desc.n_cells
    if not isinstance(ramps, torch.Tensor) or ramps.dtype != torch.int32 or not ramps.is_cuda or ramps.dim() != 1:
        raise ValueError("ramps must be a one-dimensional int32 CUDA tensor")
    R = ramps.numel()
    if not 1 <= R <= N:
        raise ValueError("ramps must hold 1..%d cell indices (got %d)" % (N, R))
    if not isinstance(inflow, torch.Tensor) or tuple(inflow.shape) != (T, L, R):
        raise ValueError("inflow must have shape (%d, %d, %d)" % (T, L, R))
    ramps, inflow = ramps.contiguous(), _f32c(inflow, "inflow")
    if not reverse:
        return ramps, R, inflow
    if g_inflow is None:
        g_inflow = torch.empty(T, L, R, dtype=torch.float32, device=inflow.device)
    elif tuple(g_inflow.shape) != (T, L, R) or g_inflow.dtype != torch.float32 or not g_inflow.is_cuda or not g_inflow.is_contiguous():
        raise ValueError("g_inflow must be a contiguous float32 CUDA tensor of shape (%d, %d, %d)" % (T, L, R))
    return ramps, R, inflow, g_inflow


def _macro_ckpt_fwd(form, desc, T, r, y, u, ueq, ghost, ckpt, segment, err, out, det=None, taps=None, target=None, sse=None, ramps=None,
                    inflow=None):
    """The checkpointed forward of both forms ("plain": detectors or nothing, "target": the dense fit): checks, buffers and the one C call
    -> (out, taps or sse).  ckpt may be None (no checkpoint is kept) in the target form.  ghost None: the ring entry points.  ramps with
    inflow: the on-ramp entry points (dhts_macro_rollout_fwd_ckpt_ramp / _target_ramp), which take all three boundary forms."""
    L, N, T = desc.n_lanes, desc.n_cells, int(T)
    fit, keep = form == "target", ckpt
    if (ramps is None) != (inflow is None):
        raise ValueError("ramps and inflow go together")
    if fit:
        segment = _macro_target_args(desc, T, segment, ckpt, target, False)
        if ckpt is None:
            keep = torch.empty(macro_ckpt_numel(desc, T, segment), dtype=torch.float32, device="meta")
    elif det is None and taps is not None:
        raise ValueError("taps without det")
    sched, r, y, u, ueq, ghost = _macro_ckpt_args(desc, T, segment, keep, r, y, u, ueq, ghost)
    D = 0
    if det is not None:
        det = _det_i32(det, N)
        D = det.numel()
        taps = _obs_buffer("taps", taps, (T, L, 3, D), r.device, new=_empty_rows)
    if fit and sse is None:
        sse = torch.empty(L, 2, dtype=torch.float64, device=r.device)
    elif fit and (tuple(sse.shape) != (L, 2) or sse.dtype != torch.float64 or not sse.is_cuda or not sse.is_contiguous()):
        raise ValueError("sse must be a contiguous float64 CUDA tensor of shape (%d, 2)" % L)
    if fit and not target.is_cuda:
        raise TypeError("target is not a CUDA tensor")
    if out is None:
        out = tuple(torch.empty_like(r) for _ in range(4))
    ring = ghost is None
    if ramps is not None:
        ramps, R, inflow = _macro_ramp_args(desc, T, ramps, inflow)
    # the family's arguments by name, each group where a sibling takes it: the boundary cells, the fit or the detectors, the ramps
    args = dict(d=C.byref(desc), T=T, segment=int(segment), r=_ptr(r), y=_ptr(y), u=_ptr(u), ueq=_ptr(ueq), r_out=_ptr(out[0]),
                y_out=_ptr(out[1]), u_out=_ptr(out[2]), ueq_out=_ptr(out[3]), ckpt=_data(ckpt), err=_ptr(err), stream=_stream())
    if not ring or ramps is not None:
        args.update(ghost=_ptr(ghost), ghost_is_sched=int(sched))
    if fit:
        args.update(target=_data(target), sse=_ptr(sse))
    else:
        args.update(det=_ptr(det), n_det=D, taps=_with_det(taps, det))
    if ramps is not None:
        args.update(ramps=_ptr(ramps), n_ramp=R, inflow=_data(inflow), ring=int(ring))
    call("dhts_macro_rollout_fwd_ckpt" + ("_target" if fit else "") + ("_ramp" if ramps is not None else "_ring" if ring else ""), args)
    return out, (sse if fit else taps)


def _macro_ckpt_bwd(form, desc, T, ckpt, r, y, u, ueq, ghost, g_r, g_y, segment, err, out, det=None, g_taps=None, target=None, g_sse=None,
                    final=None, g_ghost=None, ramps=None, inflow=None, g_inflow=None):
    """The checkpointed reverse sweep of both forms, as above -> (g_r0, g_y0, g_ghost); g_ghost is None for a ring (ghost None).  ramps with
    inflow: the on-ramp entry points -> (g_r0, g_y0, g_ghost, g_inflow [T][L][R])."""
    L, N, T = desc.n_lanes, desc.n_cells, int(T)
    fit = form == "target"
    if (ramps is None) != (inflow is None):
        raise ValueError("ramps and inflow go together")
    if fit:
        segment = _macro_target_args(desc, T, segment, ckpt, target, True)
        if g_sse is not None:
            if tuple(g_sse.shape) != (L, 2) or g_sse.dtype != torch.float64:
                raise ValueError("g_sse must be a float64 tensor of shape (%d, 2)" % L)
            if final is None or len(final) != 3 or any(tuple(t.shape) != (L, N) for t in final):
                raise ValueError("g_sse needs final = the forward's (r, y, u) after T steps, each of shape (%d, %d)" % (L, N))
    elif (det is None) != (g_taps is None):
        raise ValueError("det and g_taps go together")
    sched, r, y, u, ueq, ghost = _macro_ckpt_args(desc, T, segment, ckpt, r, y, u, ueq, ghost)
    D = 0
    if det is not None:
        det = _det_i32(det, N)
        D = det.numel()
        if tuple(g_taps.shape) != (T, L, 2, D):
            raise ValueError("g_taps must have shape (%d, %d, 2, %d)" % (T, L, D))
        g_taps = _f32c(g_taps, "g_taps")
    if g_sse is not None:
        g_sse = g_sse.contiguous()
        final = tuple(_f32c(t, n) for t, n in zip(final, ("final r", "final y", "final u")))
    else:
        final = (None, None, None)
    g_r, g_y = _f32c(g_r, "g_r"), _f32c(g_y, "g_y")
    if tuple(g_r.shape) != (L, N) or tuple(g_y.shape) != (L, N):
        raise ValueError("g_r and g_y must have shape (%d, %d)" % (L, N))
    if fit and not target.is_cuda:
        raise TypeError("target is not a CUDA tensor")
    if out is None:
        out = (torch.empty_like(g_r), torch.empty_like(g_y))
    ring = ghost is None
    if ramps is not None:
        ramps, R, inflow, g_inflow = _macro_ramp_args(desc, T, ramps, inflow, g_inflow, True)
    if ring:
        if g_ghost is not None:
            raise ValueError("a ring has no boundary cells and no g_ghost")
    else:
        want = (max(T, 1), L, 2, 2) if sched else (L, 2, 2)
        if g_ghost is None:              # (a schedule's: every row is written; the sums are added to)
            g_ghost = (torch.empty if sched else torch.zeros)(want, dtype=torch.float64, device=g_r.device)
        elif tuple(g_ghost.shape) != want or g_ghost.dtype != torch.float64 or not g_ghost.is_contiguous():
            raise ValueError("g_ghost must be a contiguous float64 tensor of shape %s" % (want,))
        elif not sched:
            g_ghost.zero_()
    args = dict(d=C.byref(desc), T=T, segment=int(segment), ckpt=_data(ckpt), r=_ptr(r), y=_ptr(y), u=_ptr(u), ueq=_ptr(ueq), g_r=_ptr(g_r),
                g_y=_ptr(g_y), g_r_out=_ptr(out[0]), g_y_out=_ptr(out[1]), err=_ptr(err), stream=_stream())
    if not ring or ramps is not None:
        args.update(ghost=_ptr(ghost), ghost_is_sched=int(sched), g_ghost=_ptr(g_ghost))
    if fit:
        args.update(target=_data(target), g_sse=_ptr(g_sse), r_fin=_ptr(final[0]), y_fin=_ptr(final[1]), u_fin=_ptr(final[2]))
    else:
        args.update(det=_ptr(det), n_det=D, g_taps=_with_det(g_taps, det))
    if ramps is not None:
        args.update(ramps=_ptr(ramps), n_ramp=R, inflow=_data(inflow), g_inflow=_data(g_inflow), ring=int(ring))
    call("dhts_macro_rollout_bwd_ckpt" + ("_target" if fit else "") + ("_ramp" if ramps is not None else "_ring" if ring else ""), args)
    g_ghost = None if ring else g_ghost[:T] if sched else g_ghost
    return (out[0], out[1], g_ghost) + ((g_inflow,) if ramps is not None else ())


def macro_rollout_fwd_ckpt(desc, T, r, y, u, ueq, ghost, ckpt, segment=0, det=None, err=None, out=None, taps=None):
    """macro_rollout_fwd / _sched / _taps that fills the checkpoint buffer `ckpt` (float32 [macro_ckpt_numel(desc, T, segment)]) instead
    of a tape (dhts_macro_rollout_fwd_ckpt): the same state and readings, bit for bit.  ghost [L][2][4], or a schedule [T][L][2][4].
    Returns ((r, y, u, ueq) after T steps, taps [T][L][3][D] or None)."""
    return _macro_ckpt_fwd("plain", desc, T, r, y, u, ueq, ghost, ckpt, segment, err, out, det, taps)


def macro_rollout_bwd_ckpt(desc, T, ckpt, r, y, u, ueq, ghost, g_r, g_y, segment=0, det=None, g_taps=None, err=None, out=None):
    """Reverse sweep from the checkpoints of macro_rollout_fwd_ckpt -> (g_r0, g_y0, g_ghost): macro_rollout_bwd / _sched / _taps' bits.
    r, y, u, ueq, ghost, segment: the forward's.  det with g_taps [T][L][2][D], or neither.  g_ghost: float64 [L][2][2] summed over the
    steps, or beside a schedule per step [T][L][2][2]."""
    return _macro_ckpt_bwd("plain", desc, T, ckpt, r, y, u, ueq, ghost, g_r, g_y, segment, err, out, det, g_taps)


# ---- the dense-fit loss inside the checkpointed pair (dhts_macro_rollout_*_ckpt_target) ------------------------------------------------
MACRO_CKPT_TARGET_MAX_CELLS = 1239      # the longest lane the target forms' reverse LDS holds (one ring step of 32 (N + 1) + 8 N bytes; the plan is the truth)


def macro_ckpt_target_plan(desc, T, segment=0):
    """macro_ckpt_plan for dhts_macro_rollout_fwd_ckpt_target / _bwd_ckpt_target (include/dhts.h): the same keys; the reverse kernel's
    ring holds two more floats per cell-step, so max_segment and the default segment are shorter and fewer lanes fit (max_segment = 0).
    ValueError: a segment outside 0 .. max_segment.  Needs no device."""
    return _macro_ckpt_plan("dhts_macro_ckpt_target_plan", "the max_segment of the target forms", desc, (T,), segment)


def _macro_target_args(desc, T, segment, ckpt, target, need_ckpt):
    """What both raw target wrappers check of ckpt and target before _macro_ckpt_args -> the resolved segment."""
    L, N, T = desc.n_lanes, desc.n_cells, int(T)
    plan = macro_ckpt_target_plan(desc, T, segment)
    if plan["max_segment"] < 1:
        raise ValueError("lanes of %d cells do not fit the target forms of the checkpointed sweep (their LDS holds up to %d cells)"
                         % (N, MACRO_CKPT_TARGET_MAX_CELLS))
    if ckpt is None and need_ckpt:
        raise ValueError("ckpt must be a contiguous float32 [macro_ckpt_numel(desc, T, segment)]")
    if not isinstance(target, torch.Tensor) or target.dtype != torch.float32 or tuple(target.shape) != (T, L, 2, N) or \
            not target.is_contiguous():
        raise ValueError("target must be a contiguous float32 tensor of shape (%d, %d, 2, %d)" % (T, L, N))
    return plan["segment"]


def macro_rollout_fwd_ckpt_target(desc, T, r, y, u, ueq, ghost, ckpt, target, segment=0, sse=None, err=None, out=None):
    """macro_rollout_fwd_ckpt that reads the observed field `target` (float32 [T][L][2][N]: density and speed after every step, NaN = not
    observed) and returns the squared error (dhts_macro_rollout_fwd_ckpt_target): ((r, y, u, ueq) after T steps, sse float64 [L][2]).
    ckpt: float32 [macro_ckpt_numel(desc, T, S)] with S the resolved segment of macro_ckpt_target_plan, or None: no checkpoint is kept.
    segment 0: that plan's default."""
    return _macro_ckpt_fwd("target", desc, T, r, y, u, ueq, ghost, ckpt, segment, err, out, None, None, target, sse)


def macro_rollout_bwd_ckpt_target(desc, T, ckpt, r, y, u, ueq, ghost, g_r, g_y, target, g_sse=None, final=None, segment=0, err=None,
                                  out=None, g_ghost=None):
    """The reverse sweep of macro_rollout_fwd_ckpt_target (dhts_macro_rollout_bwd_ckpt_target) -> (g_r0, g_y0, g_ghost) as
    macro_rollout_bwd_ckpt.  g_sse float64 [L][2] or None (zero: the plain sweep): the cotangent of sse; the per-step cotangent
    (float)(2 g_sse) * (x - target), through the speed's glue, is formed in the kernel.  final: the forward's (r, y, u) after T steps,
    needed with g_sse.  r, y, u, ueq, ghost, target, segment: the forward's."""
    return _macro_ckpt_bwd("target", desc, T, ckpt, r, y, u, ueq, ghost, g_r, g_y, segment, err, out, None, None, target, g_sse, final, g_ghost)


# ---- ring roads on the tape-free paths (dhts_macro_rollout_*_ring): the lane is closed, there are no boundary cells ----------------------
def macro_rollout_fwd_ckpt_ring(desc, T, r, y, u, ueq, ckpt, segment=0, det=None, err=None, out=None, taps=None):
    """macro_rollout_fwd_ckpt of a ring (dhts_macro_rollout_fwd_ckpt_ring, include/dhts.h): cell N - 1 is the left neighbour of cell 0.
    Returns ((r, y, u, ueq) after T steps, taps [T][L][3][D] or None)."""
    return _macro_ckpt_fwd("plain", desc, T, r, y, u, ueq, None, ckpt, segment, err, out, det, taps)


def macro_rollout_bwd_ckpt_ring(desc, T, ckpt, r, y, u, ueq, g_r, g_y, segment=0, det=None, g_taps=None, err=None, out=None):
    """Reverse sweep from the checkpoints of macro_rollout_fwd_ckpt_ring -> (g_r0, g_y0): what leaves through an end of the lane arrives
    at the other end (dhts_macro_rollout_bwd_ckpt_ring)."""
    return _macro_ckpt_bwd("plain", desc, T, ckpt, r, y, u, ueq, None, g_r, g_y, segment, err, out, det, g_taps)[:2]


def macro_rollout_fwd_ckpt_target_ring(desc, T, r, y, u, ueq, ckpt, target, segment=0, sse=None, err=None, out=None):
    """macro_rollout_fwd_ckpt_target of a ring -> ((r, y, u, ueq) after T steps, sse float64 [L][2])."""
    return _macro_ckpt_fwd("target", desc, T, r, y, u, ueq, None, ckpt, segment, err, out, None, None, target, sse)


def macro_rollout_bwd_ckpt_target_ring(desc, T, ckpt, r, y, u, ueq, g_r, g_y, target, g_sse=None, final=None, segment=0, err=None, out=None):
    """The reverse sweep of macro_rollout_fwd_ckpt_target_ring -> (g_r0, g_y0), as macro_rollout_bwd_ckpt_target."""
    return _macro_ckpt_bwd("target", desc, T, ckpt, r, y, u, ueq, None, g_r, g_y, segment, err, out, None, None, target, g_sse, final)[:2]


# ---- on-ramp inflow at chosen cells of the checkpointed pair (dhts_macro_rollout_*_ckpt_ramp) ---------------------------------
def macro_rollout_fwd_ckpt_ramp(desc, T, r, y, u, ueq, ghost, ckpt, ramps, inflow, segment=0, det=None, target=None, err=None, out=None,
                                taps=None, sse=None):
    """macro_rollout_fwd_ckpt (target given: macro_rollout_fwd_ckpt_target) with a source in chosen cells: ramps int32 CUDA [R] cell
    indices shared by all lanes, inflow float32 [T][L][R] the density rate cell ramps[j] of lane l gets in step t, added behind the
    step's own float32 store as (float)((double)r + dt (double)inflow) (include/dhts.h).  ghost [L][2][4], a schedule [T][L][2][4], or
    None: a ring.  Returns ((r, y, u, ueq) after T steps, taps [T][L][3][D] or sse [L][2] or None)."""
    return _macro_ckpt_fwd("plain" if target is None else "target", desc, T, r, y, u, ueq, ghost, ckpt, segment, err, out, det, taps, target,
                           sse, ramps, inflow)


def macro_rollout_bwd_ckpt_ramp(desc, T, ckpt, r, y, u, ueq, ghost, g_r, g_y, ramps, inflow, segment=0, det=None, g_taps=None, target=None,
                                g_sse=None, final=None, err=None, out=None, g_ghost=None, g_inflow=None):
    """The reverse sweep of macro_rollout_fwd_ckpt_ramp -> (g_r0, g_y0, g_ghost or None for a ring, g_inflow float32 [T][L][R]):
    g_inflow[t][l][j] = (float)(dt (double)G_r) with G_r the cotangent of r at cell ramps[j] of the state after step t; the column of an
    index outside [0, N) is 0.  The other arguments as macro_rollout_bwd_ckpt resp. (target given) macro_rollout_bwd_ckpt_target."""
    return _macro_ckpt_bwd("plain" if target is None else "target", desc, T, ckpt, r, y, u, ueq, ghost, g_r, g_y, segment, err, out, det,
                           g_taps, target, g_sse, final, g_ghost, ramps, inflow, g_inflow)


def macro_rollout_fwd_jvp_ring(desc, T, r, y, u, ueq, t_r, t_y, det=None, err=None, err_jvp=None, out=None, taps=None, t_taps=None,
                               ramps=None, inflow=None, t_inflow=None):
    """macro_rollout_fwd_jvp of a ring (dhts_macro_rollout_fwd_jvp_ring; with ramps: dhts_macro_rollout_fwd_jvp_ring_ramp): no ghost and no
    t_ghost; the tangents of the two end cells are each other's boundary tangents.  Returns ((rT, yT, uT, qT, taps), (t_rT, t_yT, t_taps))."""
    return macro_rollout_fwd_jvp(desc, T, r, y, u, ueq, None, t_r, t_y, None, det, err, err_jvp, out, taps, t_taps, ramps, inflow, t_inflow)


# ---------------------------------------------------------------------------------------------------------
# micro
# ---------------------------------------------------------------------------------------------------------
def micro_desc(L, V, dt):
    if not (1 <= V <= _lib.MICRO_MAX_VEHICLES):
        raise ValueError("vehicle slots per lane must be in 1..%d" % _lib.MICRO_MAX_VEHICLES)
    return MicroDesc(int(L), int(V), float(dt))


def micro_tape_numel(desc, T):
    """float32 elements of the rollout tape (second rows of dEgo / dLeading)."""
    return raw("dhts_micro_tape_bytes", d=C.byref(desc), T=int(T)) // 4


def micro_param_tape_numel(desc, T):
    """float32 elements of the parameter tape of a rollout that is differentiated w.r.t. the driver parameters (opaque: a header, the
    head gaps and 8 bytes per vehicle-step, include/dhts.h)."""
    return raw("dhts_micro_param_tape_bytes", d=C.byref(desc), T=int(T)) // 4


def micro_step_tape_numel(desc):
    """float32 elements of the single-step operator's tape (the reference's dqs)."""
    return raw("dhts_micro_step_tape_bytes", d=C.byref(desc)) // 4


def micro_step_fwd(desc, p, v, params, head, count=None, tape=None, err=None, tensor_ladder=False, head_tensor=False):
    """One step of L lanes through the operator entry point (dqs-layout tape).  tensor_ladder: the float32 tensor arithmetic of the
    reference's plain MicroLane (dhts_micro_step_fwd_tensor) instead of the analytic operator's float64 ladder; head_tensor: only the
    lanes' head gaps are float32 tensors there (dMicroLane under a tensor gap: dhts_micro_step_fwd_tensor_head)."""
    p, v = _f32c(p, "p"), _f32c(v, "v")
    out = (torch.empty_like(p), torch.empty_like(v))
    entry = "dhts_micro_step_fwd" + ("_tensor" if tensor_ladder else "_tensor_head" if head_tensor else "")
    check(raw(entry, d=C.byref(desc), p=_ptr(p), v=_ptr(v), count=_ptr(count), params=_ptr(params), head=_ptr(head), p_out=_ptr(out[0]),
              v_out=_ptr(out[1]), tape=_ptr(tape), err=_ptr(err), stream=_stream()), "dhts_micro_step_fwd")
    return out


def micro_rollout_fwd(desc, T, p, v, params, head, count=None, tape=None, hist=None, err=None, out=None, ptape=None):
    """p, v [L][V] float32; params [6][L][V] float64; head [L][2] float64; count [L] int32 or None.
    ptape (float32 [micro_param_tape_numel]): also fill the parameter tape (dhts_micro_rollout_fwd_params; needs `tape`)."""
    L, V = desc.n_lanes, desc.capacity
    p, v = _f32c(p, "p"), _f32c(v, "v")
    if tuple(p.shape) != (L, V) or tuple(v.shape) != (L, V):
        raise ValueError("p, v must have shape (%d, %d)" % (L, V))
    if params.dtype != torch.float64 or tuple(params.shape) != (6, L, V):
        raise ValueError("params must be float64 [6][L][V]")
    if head.dtype != torch.float64 or tuple(head.shape) != (L, 2):
        raise ValueError("head must be float64 [L][2]")
    if count is not None and (count.dtype != torch.int32 or tuple(count.shape) != (L,)):
        raise ValueError("count must be int32 [L]")
    params, head = params.contiguous(), head.contiguous()
    if out is None:
        out = (torch.empty_like(p), torch.empty_like(v))
    if ptape is not None and (ptape.dtype != torch.float32 or ptape.numel() != micro_param_tape_numel(desc, T)):
        raise ValueError("ptape must be float32 [micro_param_tape_numel(desc, T)]")
    call("dhts_micro_rollout_fwd" + ("_params" if ptape is not None else ""),
         dict(d=C.byref(desc), T=int(T), p=_ptr(p), v=_ptr(v), count=_ptr(count), params=_ptr(params), head=_ptr(head), p_out=_ptr(out[0]),
              v_out=_ptr(out[1]), tape=_ptr(tape), ptape=_ptr(ptape), hist=_ptr(hist), err=_ptr(err), stream=_stream()))
    return out


def micro_rollout_bwd(desc, T, tape, g_p, g_v, count=None, g_hist=None, err=None, out=None, g_head=None,
                      ptape=None, params=None, g_params=None):
    """Reverse sweep -> (g_p0, g_v0, g_head).  With ptape, params (the forward's) and g_params (float64 [6][L][V], filled here) the
    sweep also sums the gradient w.r.t. the driver parameters (dhts_micro_rollout_bwd_params); the three go together."""
    g_p, g_v = _f32c(g_p, "g_p"), _f32c(g_v, "g_v")
    if out is None:
        out = (torch.empty_like(g_p), torch.empty_like(g_v))
    if g_head is None:
        g_head = torch.zeros(desc.n_lanes, 2, dtype=torch.float64, device=g_p.device)
    with_params = ptape is not None or params is not None or g_params is not None
    if with_params:
        L, V = desc.n_lanes, desc.capacity
        if ptape is None or params is None or g_params is None:
            raise ValueError("ptape, params and g_params go together")
        if ptape.dtype != torch.float32 or ptape.numel() != micro_param_tape_numel(desc, T):
            raise ValueError("ptape must be float32 [micro_param_tape_numel(desc, T)]")
        for name, t in (("params", params), ("g_params", g_params)):
            if t.dtype != torch.float64 or tuple(t.shape) != (6, L, V) or not t.is_contiguous():
                raise ValueError("%s must be a contiguous float64 [6][L][V]" % name)
    call("dhts_micro_rollout_bwd" + ("_params" if with_params else ""),
         dict(d=C.byref(desc), T=int(T), tape=_ptr(tape), ptape=_ptr(ptape), count=_ptr(count), params=_ptr(params), g_p=_ptr(g_p),
              g_v=_ptr(g_v), g_hist=_ptr(g_hist), g_p_out=_ptr(out[0]), g_v_out=_ptr(out[1]), g_head=_ptr(g_head), g_params=_ptr(g_params),
              err=_ptr(err), stream=_stream()))
    return out[0], out[1], g_head


def micro_rollout_plan(desc, T, has_count=False):
    """Which kernel instantiations dhts_micro_rollout_fwd / _bwd launch for this shape (include/dhts.h)."""
    plan = (C.c_int32 * 8)()
    call("dhts_micro_rollout_plan", d=C.byref(desc), T=int(T), has_count=int(bool(has_count)), plan=C.byref(plan))
    keys = ("fwd_waves", "fwd_passes", "fwd_full_lane", "bwd_one_vehicle_per_thread", "bwd_block")
    return dict(zip(keys, list(plan)[:5]))


def micro_param_plan(desc, T, has_count=False):
    """The same plan's entries for the rollout that is differentiated w.r.t. the driver parameters: bytes per vehicle-step of its
    parameter tape (8 = the pre-step state; the reverse sweep recomputes the partials) and the block size of its reverse sweep."""
    plan = (C.c_int32 * 8)()
    call("dhts_micro_rollout_plan", d=C.byref(desc), T=int(T), has_count=int(bool(has_count)), plan=C.byref(plan))
    return dict(param_tape_bytes=plan[5], param_bwd_block=plan[6])


# ---- forward mode: Jacobian-vector products over the rollout tape ---------------------------------------------------------------------
def micro_rollout_jvp(desc, T, tape, t_p, t_v, count=None, t_head=None, ptape=None, params=None, t_params=None, want_hist=False,
                      err=None, out=None, t_hist=None):
    """The tangent sweep over a rollout tape (include/dhts.h): t_p, t_v float32 [K][L][V]; t_head float64 [K][L][2] or None (zero);
    ptape, params (the forward's) and t_params float64 [K][6][L][V] go together or are all None; count int32 [L] or None.
    Returns (t_pT, t_vT, t_hist): t_hist [K][T][L][2][V] = the tangent of hist after every step, None unless want_hist (or t_hist, a
    buffer to fill, is given)."""
    L, V, T = desc.n_lanes, desc.capacity, int(T)
    if t_p.dim() != 3 or tuple(t_p.shape[1:]) != (L, V) or t_p.shape[0] < 1 or t_v.shape != t_p.shape:
        raise ValueError("t_p and t_v must have shape (K, %d, %d) with K >= 1" % (L, V))
    K = int(t_p.shape[0])
    t_p, t_v = _f32c(t_p, "t_p"), _f32c(t_v, "t_v")
    if count is not None and (count.dtype != torch.int32 or tuple(count.shape) != (L,)):
        raise ValueError("count must be int32 [L]")
    _dir_arg("t_head", t_head, torch.float64, (K, L, 2))
    if ptape is not None or params is not None or t_params is not None:
        if ptape is None or params is None or t_params is None:
            raise ValueError("ptape, params and t_params go together")
        if ptape.dtype != torch.float32 or ptape.numel() != micro_param_tape_numel(desc, T):
            raise ValueError("ptape must be float32 [micro_param_tape_numel(desc, T)]")
        if params.dtype != torch.float64 or tuple(params.shape) != (6, L, V) or not params.is_contiguous():
            raise ValueError("params must be a contiguous float64 [6][L][V]")
        _dir_arg("t_params", t_params, torch.float64, (K, 6, L, V))
    if T > 0 and tape is None:
        raise ValueError("a sweep of T > 0 steps needs the rollout's tape")
    if tape is not None and (tape.dtype != torch.float32 or tape.numel() != micro_tape_numel(desc, T)):
        raise ValueError("tape must be float32 [micro_tape_numel(desc, T)]")
    if t_hist is not None:
        if tuple(t_hist.shape) != (K, T, L, 2, V) or t_hist.dtype != torch.float32 or not t_hist.is_cuda or not t_hist.is_contiguous():
            raise ValueError("t_hist must be a contiguous float32 CUDA tensor of shape (%d, %d, %d, 2, %d)" % (K, T, L, V))
    elif want_hist:
        t_hist = torch.empty(K, T, L, 2, V, dtype=torch.float32, device=t_p.device)
    if out is None:
        out = (torch.empty_like(t_p), torch.empty_like(t_v))
    hist_ptr = None if t_hist is None or not t_hist.numel() else _ptr(t_hist)      # (T = 0: no row, and an empty tensor has no address)
    call("dhts_micro_rollout_jvp", d=C.byref(desc), T=T, n_dir=K, tape=_ptr(tape) if T > 0 else None, ptape=_ptr(ptape), count=_ptr(count),
         params=_ptr(params), t_p=_ptr(t_p), t_v=_ptr(t_v), t_head=_ptr(t_head), t_params=_ptr(t_params), t_p_out=_ptr(out[0]),
         t_v_out=_ptr(out[1]), t_hist=hist_ptr, err=_ptr(err), stream=_stream())
    return out[0], out[1], t_hist


_MICRO_JVP_PLAN_KEYS = ("block", "dirs_per_launch", "launches", "lds_bytes")


def micro_jvp_plan(desc, T, n_dir, want_params=False):
    """What dhts_micro_rollout_jvp launches for this shape: its block (one vehicle per thread), the direction slots of the widest launch,
    the number of launches and the widest launch's dynamic LDS bytes."""
    plan = (C.c_int32 * 8)()
    call("dhts_micro_jvp_plan", d=C.byref(desc), T=int(T), n_dir=int(n_dir), want_params=int(bool(want_params)), plan=C.byref(plan))
    return dict(zip(_MICRO_JVP_PLAN_KEYS, list(plan)))


def micro_rollout_fwd_jvp(desc, T, p, v, params, head, t_p, t_v, count=None, t_head=None, t_params=None, want_hist=False, err=None,
                          err_jvp=None, out=None):
    """The rollout and K tangent directions of it in one kernel, no tape (dhts_micro_rollout_fwd_jvp, include/dhts.h): what
    micro_rollout_fwd followed by micro_rollout_jvp returns, bit for bit.  p, v, params, head, count as micro_rollout_fwd; t_p, t_v
    float32 [K][L][V]; t_head float64 [K][L][2] or None (zero); t_params float64 [K][6][L][V] or None (no parameter term).
    err: the forward's fault record (collisions), err_jvp: the tangent sweep's (the earliest non-finite tangent); each may be None.
    out: (p_out, v_out, t_p_out, t_v_out[, hist, t_hist]) buffers to fill; hist [T][L][2][V] and t_hist [K][T][L][2][V] are allocated
    with want_hist unless handed in.  Returns ((pT, vT, hist), (t_pT, t_vT, t_hist)), the histories None unless asked for."""
    return _micro_fwd_jvp("hist", desc, T, p, v, params, t_p, t_v, count, t_params, err, err_jvp, out, head=head, t_head=t_head, want_hist=want_hist)


def micro_fwd_jvp_gn_plan(desc, T, n_dir, want_params=False):
    """What dhts_micro_rollout_fwd_jvp_gn launches for this shape (include/dhts.h): the keys of micro_jvp_plan -- dirs_per_launch the
    widest kernel held for the lane (no scratch, no spill), launches 0 where that width cannot carry n_dir -- then pair_block, the
    directions per block of the pair-of-blocks scheme, and block_bound, the block size the widest launch's kernel is compiled for."""
    plan = (C.c_int32 * 8)()
    call("dhts_micro_fwd_jvp_gn_plan", d=C.byref(desc), T=int(T), n_dir=int(n_dir), want_params=int(bool(want_params)), plan=C.byref(plan))
    return dict(zip(_MICRO_JVP_PLAN_KEYS + ("pair_block", "block_bound"), list(plan)))


def micro_gn_launches(n_dir, width):
    """The launches dhts_micro_rollout_fwd_jvp_gn takes for n_dir directions under launch width `width`, each a tuple of the directions it
    carries (the library's schedule restated: its count is micro_fwd_jvp_gn_plan's `launches`).  n_dir <= width: one launch.  Otherwise
    blocks of width // 2 directions and one launch per PAIR of blocks, so that every pair of directions meets in some launch; a width
    below 2 carries one direction only (an empty list: it cannot carry n_dir)."""
    n_dir, width = int(n_dir), int(width)
    if n_dir < 1 or width < 1 or (n_dir > width and width < 2):
        return []
    if n_dir <= width:
        return [tuple(range(n_dir))]
    h = width // 2
    blocks = [tuple(range(b, min(b + h, n_dir))) for b in range(0, n_dir, h)]
    return [blocks[i] + blocks[j] for i in range(len(blocks)) for j in range(i + 1, len(blocks))]


def micro_rollout_fwd_jvp_gn(desc, T, p, v, params, t_p, t_v, target, head=None, lead=None, lead_length=None, ring=None, probes=None, every=1,
                             count=None, t_head=None, t_lead=None, t_params=None, err=None, err_jvp=None, out=None):
    """The fused rollout + tangent call with the Gauss-Newton normal equations of a trajectory fit formed in the kernel
    (dhts_micro_rollout_fwd_jvp_gn, include/dhts.h), through the launch path of the sampled forms: exactly one of head, lead, ring names
    the boundary; target is a contiguous float32 [T // every][L][2][P] on p's device (the shape of samples; probes=None, every=1: [T][L][2][V]),
    NaN = not observed.  Neither samples nor t_samples exists.  Returns ((pT, vT, sse), (t_pT, t_vT, jtr, jtj)): sse float64 [L][2], jtr
    float64 [L][K], jtj float64 [L][K][K].  ValueError: a K the plan cannot carry (micro_fwd_jvp_gn_plan)."""
    if (head is not None) + (lead is not None) + (ring is not None) != 1:
        raise ValueError("exactly one of head, lead and ring must be given")
    if t_head is not None and head is None:
        raise ValueError("t_head needs head")
    if (t_lead is not None or lead_length is not None) and lead is None:
        raise ValueError("t_lead and lead_length need lead")
    if target is None:
        raise ValueError("target must be given")
    form = "samples" if head is not None else ("lead" if lead is not None else "ring")
    return _micro_fwd_jvp(form, desc, T, p, v, params, t_p, t_v, count, t_params, err, err_jvp, out, head=head, t_head=t_head, probes=probes,
                          every=every, lead=lead, lead_length=lead_length, t_lead=t_lead, ring=ring, target=target)


def micro_fwd_jvp_plan(desc, T, n_dir, want_params=False):
    """What dhts_micro_rollout_fwd_jvp launches for this shape: the keys of micro_jvp_plan."""
    plan = (C.c_int32 * 8)()
    call("dhts_micro_fwd_jvp_plan", d=C.byref(desc), T=int(T), n_dir=int(n_dir), want_params=int(bool(want_params)), plan=C.byref(plan))
    return dict(zip(_MICRO_JVP_PLAN_KEYS, list(plan)))


# ---- reverse mode from checkpoints: the tape of one segment at a time, in LDS ------------------------------------------------------------
_MICRO_CKPT_PLAN_KEYS = ("block", "segment", "max_segment", "checkpoints", "fwd_lds_bytes", "bwd_lds_bytes", "bwd_groups_per_cu")


def micro_ckpt_plan(desc, T, want_params=False, segment=0):
    """What dhts_micro_rollout_fwd_ckpt / _bwd_ckpt launch for this shape (include/dhts.h): the block, the segment length used (the plan's
    own for segment = 0), the longest one the reverse kernel's LDS holds (shorter with want_params), the number of checkpoints
    ceil(T / segment), the dynamic LDS bytes of the two kernels and the reverse workgroups a CU holds by LDS.  ValueError: a segment
    outside 0 .. max_segment."""
    return _micro_ckpt_plan("dhts_micro_ckpt_plan", "", desc, T, want_params, segment)


def micro_ckpt_numel(desc, T, segment=0):
    """float32 elements of the checkpoint buffer (opaque: the float32 (p, v) of every slot every `segment` steps, include/dhts.h)."""
    return raw("dhts_micro_ckpt_bytes", d=C.byref(desc), T=int(T), segment=int(segment)) // 4


# ---- the tape-free paths' raw layer: every check once, then _micro_ckpt_fwd / _micro_ckpt_bwd / _micro_fwd_jvp for every form -----------
# A form: "hist" (the dense history, a constant head gap), "samples" (probe samples in its place), "lead" (samples, the head follows a
# recorded leader), "ring" (samples, the head follows the lane's own tail one circumference ahead) or "target" (the trajectory fit of
# the checkpointed pair; head, lead or ring).


def _micro_ckpt_plan(entry, forms, desc, T, want_params, segment):
    """micro_ckpt_plan (forms "") and micro_ckpt_target_plan (" of the target forms")."""
    plan = (C.c_int32 * 8)()
    if not 0 <= int(segment) <= 0x7fffffff:
        raise ValueError("segment must be 0 (the plan's choice) or a positive int")
    status = raw(entry, d=C.byref(desc), T=int(T), want_params=int(bool(want_params)), segment=int(segment), plan=C.byref(plan))
    if status == _lib.E_INVALID and int(T) >= 0:
        raise ValueError("segment must be 0 (the plan's choice) or 1 .. max_segment%s for %d vehicle slots%s" %
                         (forms, desc.capacity, " with the parameter gradient" if want_params else ""))
    check(status, entry)
    return dict(zip(_MICRO_CKPT_PLAN_KEYS, list(plan)))


def _samples_shape(desc, T, probes, every):
    """The raw wrappers' checks of (probes, every) -> (rows, columns, n_probes for the C call).  probes: None (every slot) or a CUDA int32
    tensor of distinct slots, used as it is (include/dhts.h: an entry outside [0, V) is skipped by the kernels)."""
    V = desc.capacity
    if isinstance(every, bool) or not isinstance(every, int) or every < 1:
        raise ValueError("every must be an int >= 1, not %r" % (every,))
    if int(T) < 0:
        raise ValueError("T must be >= 0")
    if probes is None:
        return int(T) // every, V, 0
    if (not isinstance(probes, torch.Tensor) or not probes.is_cuda or probes.dtype != torch.int32 or probes.dim() != 1
            or not 1 <= probes.numel() <= V or not probes.is_contiguous()):
        raise ValueError("probes must be None or a contiguous one-dimensional CUDA int32 tensor of 1..%d slots" % V)
    return int(T) // every, int(probes.numel()), int(probes.numel())


def _lead_args(desc, T, lead, lead_length):
    """The raw wrappers' checks of (lead, lead_length): lead a contiguous float32 [T][L][2], lead_length None or a contiguous float64 [L]."""
    L = desc.n_lanes
    if int(T) < 0:
        raise ValueError("T must be >= 0")
    if (not isinstance(lead, torch.Tensor) or lead.dtype != torch.float32 or tuple(lead.shape) != (int(T), L, 2)
            or not lead.is_contiguous()):
        raise ValueError("lead must be a contiguous float32 tensor of shape (%d, %d, 2)" % (int(T), L))
    if lead_length is not None and (not isinstance(lead_length, torch.Tensor) or lead_length.dtype != torch.float64
                                    or tuple(lead_length.shape) != (L,) or not lead_length.is_contiguous()):
        raise ValueError("lead_length must be None or a contiguous float64 tensor of shape (%d,)" % L)


def _ring_arg(desc, ring):
    """The raw wrappers' check of ring: a contiguous float64 [L], the circumference of each lane's ring."""
    if (not isinstance(ring, torch.Tensor) or ring.dtype != torch.float64 or tuple(ring.shape) != (desc.n_lanes,)
            or not ring.is_contiguous()):
        raise ValueError("ring must be a contiguous float64 tensor of shape (%d,)" % desc.n_lanes)


def _head_arg(desc, head, contiguous):
    if head.dtype != torch.float64 or tuple(head.shape) != (desc.n_lanes, 2) or (contiguous and not head.is_contiguous()):
        raise ValueError("head must be %sfloat64 [L][2]" % ("a contiguous " if contiguous else ""))


def _target_args(desc, T, target, head, lead, ring=None):
    """What the target forms check first: head or lead, exactly one (neither on a ring), and target, a contiguous float32 [T][L][2][V]."""
    L, V = desc.n_lanes, desc.capacity
    if ring is not None:
        if head is not None or lead is not None:
            raise ValueError("ring takes neither head nor lead: the head vehicle follows the tail")
    elif (head is None) == (lead is None):
        raise ValueError("exactly one of head and lead must be given")
    if int(T) < 0:
        raise ValueError("T must be >= 0")
    if (not isinstance(target, torch.Tensor) or target.dtype != torch.float32 or tuple(target.shape) != (int(T), L, 2, V)
            or not target.is_contiguous()):
        raise ValueError("target must be a contiguous float32 tensor of shape (%d, %d, 2, %d)" % (int(T), L, V))


def _boundary_args(desc, T, head, lead, lead_length, contiguous, ring=None):
    """... and after ckpt: whichever of head, lead and ring the head vehicle follows."""
    if ring is not None:
        if lead_length is not None:
            raise ValueError("lead_length needs lead")
        _ring_arg(desc, ring)
    elif lead is not None:
        _lead_args(desc, T, lead, lead_length)
    elif lead_length is not None:
        raise ValueError("lead_length needs lead")
    else:
        _head_arg(desc, head, contiguous)


def _ckpt_args(form, desc, T, want_params, segment, ckpt, optional):
    """(segment, ckpt) against the form's segment plan -> the resolved segment.  ckpt: a contiguous float32
    [micro_ckpt_numel(desc, T, resolved segment)], or None where the forward may run without one."""
    S = (micro_ckpt_target_plan if form == "target" else micro_ckpt_plan)(desc, T, want_params, segment)["segment"]
    if ckpt is None and optional:
        return S
    if (ckpt is None and form == "target") or ckpt.dtype != torch.float32 or ckpt.numel() != micro_ckpt_numel(desc, T, S) \
            or not ckpt.is_contiguous():
        raise ValueError("ckpt must be %sa contiguous float32 [micro_ckpt_numel(desc, T, segment)]%s" %
                         ("None or " if optional else "", ", segment the target plan's" if form == "target" else ""))
    return S


def _state_args(desc, p, v, params, head, count, check_head=True):
    """(p, v, params, head, count) of a forward -> (p, v, params, head) as the library reads them; head None: the lead forms;
    check_head False: _boundary_args has checked it."""
    L, V = desc.n_lanes, desc.capacity
    p, v = _f32c(p, "p"), _f32c(v, "v")
    if tuple(p.shape) != (L, V) or tuple(v.shape) != (L, V):
        raise ValueError("p, v must have shape (%d, %d)" % (L, V))
    if params.dtype != torch.float64 or tuple(params.shape) != (6, L, V):
        raise ValueError("params must be float64 [6][L][V]")
    if head is not None and check_head:
        _head_arg(desc, head, False)
    if count is not None and (count.dtype != torch.int32 or tuple(count.shape) != (L,)):
        raise ValueError("count must be int32 [L]")
    return p, v, params.contiguous(), None if head is None else head.contiguous()


def _dir_arg(name, t, dtype, shape):
    """An optional per-direction tangent array: contiguous, of `dtype` and `shape`."""
    if t is not None and (t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous()):
        raise ValueError("%s must be a contiguous %s %s" % (name, str(dtype)[6:], "".join("[%d]" % s for s in shape)))


def _micro_ckpt_fwd(form, desc, T, p, v, params, ckpt, count, segment, err, out, head=None, hist=None, probes=None, every=1, samples=None,
                    observe=True, lead=None, lead_length=None, target=None, sse=None, ring=None):
    """The checkpointed forward of every form: checks, buffers and the one C call -> (out, samples or sse).  ckpt may be None (no
    checkpoint is kept) in every form but "hist"."""
    L = desc.n_lanes
    sampled = form in ("samples", "lead", "ring")
    if form == "target":
        _target_args(desc, T, target, head, lead, ring)
    if sampled:
        rows, n, n_probes = _samples_shape(desc, T, probes, every)
    if form == "lead":
        _lead_args(desc, T, lead, lead_length)
    if form == "ring":
        _ring_arg(desc, ring)
    S = _ckpt_args(form, desc, T, False, segment, ckpt, form != "hist")
    if form == "target":
        _boundary_args(desc, T, head, lead, lead_length, False, ring)
    p, v, params, head = _state_args(desc, p, v, params, head, count, form != "target")
    if sampled:
        samples = _obs_buffer("samples", samples, (rows, L, 2, n), p.device) if observe else None
    if form == "target":
        if sse is None:
            sse = torch.empty(L, 2, dtype=torch.float64, device=p.device)
        elif sse.dtype != torch.float64 or tuple(sse.shape) != (L, 2) or not sse.is_contiguous():
            raise ValueError("sse must be a contiguous float64 tensor of shape (%d, 2)" % L)
    if out is None:
        out = (torch.empty_like(p), torch.empty_like(v))
    # (a T = 0 call of the target form with lead: no row exists; the library takes the lead form from the NULL head)
    # the family's arguments by name, each group where a sibling takes it: what the head vehicle follows, what is observed
    on_ring = form == "ring" or (form == "target" and ring is not None)
    args = dict(d=C.byref(desc), T=int(T), segment=S, p=_ptr(p), v=_ptr(v), count=_ptr(count), params=_ptr(params), p_out=_ptr(out[0]),
                v_out=_ptr(out[1]), ckpt=_data(ckpt), err=_ptr(err), stream=_stream())
    if on_ring:
        args["ring"] = _ptr(ring)
    if not on_ring and form != "lead":
        args["head"] = _ptr(head)
    if form == "lead" or (form == "target" and not on_ring):
        args.update(lead=_data(lead), lead_length=_ptr(lead_length))
    if sampled:
        args.update(probes=_ptr(probes), n_probes=n_probes, every=every, samples=_data(samples))
    elif form == "target":
        args.update(target=_data(target), sse=_ptr(sse))
    else:
        args["hist"] = _data(hist)
    call("dhts_micro_rollout_fwd_ckpt" + ("" if form == "hist" else "_target_ring" if form == "target" and on_ring else "_" + form), args)
    return out, (sse if form == "target" else samples if sampled else None)


def _micro_ckpt_bwd(form, desc, T, ckpt, params, g_p, g_v, count, segment, err, out, g_params, head=None, g_head=None, g_hist=None,
                    probes=None, every=1, g_samples=None, lead=None, lead_length=None, g_lead=None, target=None, g_sse=None, ring=None):
    """The reverse sweep from checkpoints of every form -> (g_p0, g_v0, g_head or g_lead; None on a ring).  g_samples is required in
    the "samples" form and optional (None: nothing was observed) in the "lead" and "ring" forms."""
    L, V = desc.n_lanes, desc.capacity
    sampled = form in ("samples", "lead", "ring")
    if form == "target":
        _target_args(desc, T, target, head, lead, ring)
    if sampled:
        rows, n, n_probes = _samples_shape(desc, T, probes, every)
    if form == "lead":
        _lead_args(desc, T, lead, lead_length)
    if form == "ring":
        _ring_arg(desc, ring)
    S = _ckpt_args(form, desc, T, g_params is not None, segment, ckpt, False)
    if form == "target":
        _boundary_args(desc, T, head, lead, lead_length, True, ring)
    for name, t in (("params", params), ("g_params", g_params)):
        if t is not None and (t.dtype != torch.float64 or tuple(t.shape) != (6, L, V) or not t.is_contiguous()):
            raise ValueError("%s must be a contiguous float64 [6][L][V]" % name)
    if form in ("hist", "samples"):
        _head_arg(desc, head, True)
    if form == "samples" and g_samples is None:
        raise ValueError("g_samples is required: float32 [T // every][L][2][P]")
    if g_sse is not None and (g_sse.dtype != torch.float64 or tuple(g_sse.shape) != (L, 2) or not g_sse.is_contiguous()):
        raise ValueError("g_sse must be None or a contiguous float64 tensor of shape (%d, 2)" % L)
    g_p, g_v = _f32c(g_p, "g_p"), _f32c(g_v, "g_v")
    if g_samples is not None:
        g_samples = _obs_buffer("g_samples", g_samples, (rows, L, 2, n), g_p.device)
    if out is None:
        out = (torch.empty_like(g_p), torch.empty_like(g_v))
    if ring is not None:                 # the image's cotangent returns to the tail inside the sweep
        if g_head is not None or g_lead is not None:
            raise ValueError("a ring has neither g_head nor g_lead")
    elif lead is None:                   # the cotangent of whichever the head follows
        if g_lead is not None:
            raise ValueError("g_lead needs lead")
        if g_head is None:
            g_head = torch.zeros(L, 2, dtype=torch.float64, device=g_p.device)
    else:
        if g_head is not None:
            raise ValueError("g_head needs head")
        if g_lead is None:
            g_lead = torch.empty(int(T), L, 2, dtype=torch.float32, device=g_p.device)
        elif g_lead.dtype != torch.float32 or tuple(g_lead.shape) != (int(T), L, 2) or not g_lead.is_contiguous():
            raise ValueError("g_lead must be a contiguous float32 tensor of shape (%d, %d, 2)" % (int(T), L))
    on_ring = form == "ring" or (form == "target" and ring is not None)
    args = dict(d=C.byref(desc), T=int(T), segment=S, ckpt=_data(ckpt), count=_ptr(count), params=_ptr(params), g_p=_ptr(g_p), g_v=_ptr(g_v),
                g_p_out=_ptr(out[0]), g_v_out=_ptr(out[1]), g_params=_ptr(g_params), err=_ptr(err), stream=_stream())
    if on_ring:
        args["ring"] = _ptr(ring)
    if not on_ring and form != "lead":
        args.update(head=_ptr(head), g_head=_ptr(g_head))
    if form == "lead" or (form == "target" and not on_ring):
        args.update(lead=_data(lead), lead_length=_ptr(lead_length), g_lead=_data(g_lead))
    if sampled:
        args.update(probes=_ptr(probes), n_probes=n_probes, every=every, g_samples=_data(g_samples))
    elif form == "target":
        args.update(target=_data(target), g_sse=_ptr(g_sse))
    else:
        args["g_hist"] = _ptr(g_hist)
    call("dhts_micro_rollout_bwd_ckpt" + ("" if form == "hist" else "_target_ring" if form == "target" and on_ring else "_" + form), args)
    return out[0], out[1], (None if ring is not None else g_head if lead is None else g_lead)


def _gn_target_arg(target, shape, device):
    """The Gauss-Newton form's check of target: a contiguous float32 tensor of the shape of samples on the state's device, no grad."""
    if (not isinstance(target, torch.Tensor) or target.dtype != torch.float32 or tuple(target.shape) != tuple(shape)
            or target.device != device or not target.is_contiguous() or target.requires_grad):
        raise ValueError("target must be a contiguous float32 tensor of shape %s on %s that does not require grad" % (tuple(shape), device))


def _gn_plan_carries(desc, T, K, want_params):
    """The Gauss-Newton form's plan, or the ValueError for a K it cannot carry."""
    plan = micro_fwd_jvp_gn_plan(desc, T, K, want_params)
    if plan["launches"] == 0:
        raise ValueError("V = %d%s: a launch of the Gauss-Newton form carries %d direction%s (block %d, compiled for %d threads), which "
                         "cannot form the cross products of K = %d" % (desc.capacity, " with t_params" if want_params else "",
                                                                        plan["dirs_per_launch"], "" if plan["dirs_per_launch"] == 1 else "s",
                                                                        plan["block"], plan["block_bound"], K))
    return plan


def _micro_fwd_jvp(form, desc, T, p, v, params, t_p, t_v, count, t_params, err, err_jvp, out, head=None, t_head=None, want_hist=False,
                   probes=None, every=1, observe=True, lead=None, lead_length=None, t_lead=None, ring=None, target=None):
    """The fused rollout + tangent call of the "hist", "samples", "lead" and "ring" forms -> ((pT, vT, observed), (t_pT, t_vT, t_observed)),
    observed = the histories (None unless asked for or handed in) or the sample arrays (None with observe False).  target (the three
    sampled forms): the Gauss-Newton form, dhts_micro_rollout_fwd_jvp_gn -> ((pT, vT, sse), (t_pT, t_vT, jtr, jtj)); out holds the four
    state buffers only."""
    L, V, T = desc.n_lanes, desc.capacity, int(T)
    sampled = form != "hist"
    if sampled:
        rows, n, n_probes = _samples_shape(desc, T, probes, every)
    if target is not None:
        if not sampled:
            raise ValueError("target takes the place of the sample arrays: the dense fit is the sampled form with probes=None, every=1")
        _gn_target_arg(target, (rows, L, 2, n), p.device)
    if form == "lead":
        _lead_args(desc, T, lead, lead_length)
    if form == "ring":
        _ring_arg(desc, ring)
    p, v, params, head = _state_args(desc, p, v, params, head, count)
    if T < 0:
        raise ValueError("T must be >= 0")
    if t_p.dim() != 3 or tuple(t_p.shape[1:]) != (L, V) or t_p.shape[0] < 1 or t_v.shape != t_p.shape:
        raise ValueError("t_p and t_v must have shape (K, %d, %d) with K >= 1" % (L, V))
    K = int(t_p.shape[0])
    t_p, t_v = _f32c(t_p, "t_p"), _f32c(t_v, "t_v")
    _dir_arg("t_lead", t_lead, torch.float32, (K, T, L, 2))
    _dir_arg("t_head", t_head, torch.float64, (K, L, 2))
    _dir_arg("t_params", t_params, torch.float64, (K, 6, L, V))
    out = tuple(out) if out is not None else ()
    if target is not None:
        _gn_plan_carries(desc, T, K, t_params is not None)
        if len(out) not in (0, 4):
            raise ValueError("out must be (p_out, v_out, t_p_out, t_v_out)")
        state = _state_out(("p_out", "v_out", "t_p_out", "t_v_out"), out, (p, v, t_p, t_v))
        sse = torch.zeros(L, 2, dtype=torch.float64, device=p.device)
        jtr, jtj = torch.zeros(L, K, dtype=torch.float64, device=p.device), torch.zeros(L, K, K, dtype=torch.float64, device=p.device)
        observed = dict(target=_data(target), sse=_ptr(sse), jtr=_ptr(jtr), jtj=_ptr(jtj))
    else:
        names = ("samples", "t_samples") if sampled else ("hist", "t_hist")
        if len(out) not in (0, 4, 6) or (len(out) == 6 and not observe):
            raise ValueError("out must be (p_out, v_out, t_p_out, t_v_out[, %s, %s])" % names)
        shape = (rows, L, 2, n) if sampled else (T, L, 2, V)
        new = (torch.zeros if observe else None) if sampled else (torch.empty if want_hist else None)
        obs = [_obs_buffer(name, t, shp, p.device, new) for name, t, shp in zip(names, out[4:6] or (None, None), (shape, (K,) + shape))]
        state = _state_out(("p_out", "v_out", "t_p_out", "t_v_out"), out, (p, v, t_p, t_v))
        observed = {names[0]: _data(obs[0]), names[1]: _data(obs[1])}
    # the family's arguments by name, each group where a sibling takes it (the Gauss-Newton entry takes every boundary group)
    gn = target is not None
    args = dict(observed, d=C.byref(desc), T=T, n_dir=K, p=_ptr(p), v=_ptr(v), count=_ptr(count), params=_ptr(params), t_p=_ptr(t_p),
                t_v=_ptr(t_v), t_params=_ptr(t_params), p_out=_ptr(state[0]), v_out=_ptr(state[1]), t_p_out=_ptr(state[2]),
                t_v_out=_ptr(state[3]), err=_ptr(err), err_jvp=_ptr(err_jvp), stream=_stream())
    if gn or form in ("hist", "samples"):
        args.update(head=_ptr(head), t_head=_ptr(t_head))
    if gn or form == "lead":
        args.update(lead=_data(lead), lead_length=_ptr(lead_length), t_lead=_data(t_lead))
    if gn or form == "ring":
        args["ring"] = _ptr(ring)
    if sampled:
        args.update(probes=_ptr(probes), n_probes=n_probes, every=every)
    call("dhts_micro_rollout_fwd_jvp" + ("_gn" if gn else "" if form == "hist" else "_" + form), args)
    if gn:
        return (state[0], state[1], sse), (state[2], state[3], jtr, jtj)
    return (state[0], state[1], obs[0]), (state[2], state[3], obs[1])


def micro_rollout_fwd_ckpt(desc, T, p, v, params, head, ckpt, count=None, segment=0, hist=None, err=None, out=None):
    """micro_rollout_fwd that fills the checkpoint buffer `ckpt` (float32 [micro_ckpt_numel(desc, T, segment)]) instead of a tape
    (dhts_micro_rollout_fwd_ckpt): the same (pT, vT) and hist, bit for bit."""
    return _micro_ckpt_fwd("hist", desc, T, p, v, params, ckpt, count, segment, err, out, head=head, hist=hist)[0]


def micro_rollout_bwd_ckpt(desc, T, ckpt, params, head, g_p, g_v, count=None, segment=0, g_hist=None, err=None, out=None, g_head=None,
                           g_params=None):
    """Reverse sweep from the checkpoints of micro_rollout_fwd_ckpt -> (g_p0, g_v0, g_head): micro_rollout_bwd's bits.  params, head,
    count, segment: the forward's.  g_params (float64 [6][L][V], filled here): also the gradient w.r.t. the driver parameters."""
    return _micro_ckpt_bwd("hist", desc, T, ckpt, params, g_p, g_v, count, segment, err, out, g_params, head=head, g_head=g_head,
                           g_hist=g_hist)


# ---- probe samples on the two tape-free paths (dhts_micro_rollout_*_samples) ------------------------------------------------------------
def micro_rollout_fwd_ckpt_samples(desc, T, p, v, params, head, ckpt, probes, every, count=None, segment=0, samples=None, err=None, out=None):
    """micro_rollout_fwd_ckpt that writes, instead of a history, samples [T // every][L][2][P] (dhts_micro_rollout_fwd_ckpt_samples,
    include/dhts.h): row j = (p, v) of slot probes[i] after step (j + 1) every - 1.  probes: a CUDA int32 tensor of distinct slots (not
    validated: an entry outside [0, V) leaves its column as it is) or None = every slot.  samples: allocated zero-filled unless handed
    in (live probe slots only are written).  ckpt=None: no checkpoint is kept.  Returns (pT, vT, samples)."""
    out, samples = _micro_ckpt_fwd("samples", desc, T, p, v, params, ckpt, count, segment, err, out, head=head, probes=probes, every=every,
                                   samples=samples)
    return out[0], out[1], samples


def micro_rollout_bwd_ckpt_samples(desc, T, ckpt, params, head, g_p, g_v, probes, every, g_samples, count=None, segment=0, err=None,
                                   out=None, g_head=None, g_params=None):
    """micro_rollout_bwd_ckpt with the cotangent g_samples [T // every][L][2][P] of micro_rollout_fwd_ckpt_samples' samples in place of
    g_hist (dhts_micro_rollout_bwd_ckpt_samples): it enters the sweep at the sampled steps, at live probe slots.  probes, every,
    count, segment: the forward's.  Returns (g_p0, g_v0, g_head)."""
    return _micro_ckpt_bwd("samples", desc, T, ckpt, params, g_p, g_v, count, segment, err, out, g_params, head=head, g_head=g_head,
                           probes=probes, every=every, g_samples=g_samples)


def micro_rollout_fwd_jvp_samples(desc, T, p, v, params, head, t_p, t_v, probes, every, count=None, t_head=None, t_params=None, err=None,
                                  err_jvp=None, out=None):
    """micro_rollout_fwd_jvp that writes, instead of the histories, samples [T // every][L][2][P] and t_samples [K][T // every][L][2][P]
    (dhts_micro_rollout_fwd_jvp_samples): probes, every as micro_rollout_fwd_ckpt_samples.  out: (p_out, v_out, t_p_out, t_v_out[,
    samples, t_samples]); the sample arrays are allocated zero-filled unless handed in (samples: live probe slots only are written;
    t_samples: every probe slot, 0 at or beyond count).  Returns ((pT, vT, samples), (t_pT, t_vT, t_samples))."""
    return _micro_fwd_jvp("samples", desc, T, p, v, params, t_p, t_v, count, t_params, err, err_jvp, out, head=head, t_head=t_head,
                          probes=probes, every=every)


# ---- a recorded leader on the two tape-free paths (dhts_micro_rollout_*_lead) ------------------------------------------------------------
def micro_rollout_fwd_ckpt_lead(desc, T, p, v, params, lead, ckpt, probes=None, every=1, lead_length=None, count=None, segment=0,
                                samples=None, observe=True, err=None, out=None):
    """micro_rollout_fwd_ckpt_samples whose head vehicle follows a recorded leader (dhts_micro_rollout_fwd_ckpt_lead, include/dhts.h):
    lead float32 [T][L][2] = (p, v) of the vehicle in front of each lane's head as the head sees it in step t; lead_length float64 [L]
    or None (the head's own length).  observe=False: no samples at all (the kernel is handed NULL; the returned samples is None);
    probes=None, every=1 is the dense history.  Returns (pT, vT, samples)."""
    out, samples = _micro_ckpt_fwd("lead", desc, T, p, v, params, ckpt, count, segment, err, out, probes=probes, every=every,
                                   samples=samples, observe=observe, lead=lead, lead_length=lead_length)
    return out[0], out[1], samples


def micro_rollout_bwd_ckpt_lead(desc, T, ckpt, params, lead, g_p, g_v, probes=None, every=1, g_samples=None, lead_length=None, count=None,
                                segment=0, err=None, out=None, g_lead=None, g_params=None):
    """The reverse sweep of micro_rollout_fwd_ckpt_lead (dhts_micro_rollout_bwd_ckpt_lead) -> (g_p0, g_v0, g_lead): g_lead float32
    [T][L][2], row t the cotangent of lead[t] (every row written; exactly 0 for a lane without a vehicle); nothing is folded into the
    head.  g_samples=None: nothing was observed.  lead, lead_length, probes, every, count, segment: the forward's."""
    return _micro_ckpt_bwd("lead", desc, T, ckpt, params, g_p, g_v, count, segment, err, out, g_params, probes=probes, every=every,
                           g_samples=g_samples, lead=lead, lead_length=lead_length, g_lead=g_lead)


def micro_rollout_fwd_jvp_lead(desc, T, p, v, params, lead, t_p, t_v, probes=None, every=1, lead_length=None, count=None, t_lead=None,
                               t_params=None, observe=True, err=None, err_jvp=None, out=None):
    """micro_rollout_fwd_jvp_samples whose head vehicle follows a recorded leader (dhts_micro_rollout_fwd_jvp_lead): lead, lead_length
    as micro_rollout_fwd_ckpt_lead; t_lead float32 [K][T][L][2] or None (zero).  observe=False: no sample arrays (both returned as
    None).  Returns ((pT, vT, samples), (t_pT, t_vT, t_samples))."""
    return _micro_fwd_jvp("lead", desc, T, p, v, params, t_p, t_v, count, t_params, err, err_jvp, out, probes=probes, every=every,
                          observe=observe, lead=lead, lead_length=lead_length, t_lead=t_lead)


# ---- the trajectory-fit loss inside the checkpointed pair (dhts_micro_rollout_*_ckpt_target) ----------------------------------------------
def micro_ckpt_target_plan(desc, T, want_params=False, segment=0):
    """micro_ckpt_plan for dhts_micro_rollout_fwd_ckpt_target / _bwd_ckpt_target (include/dhts.h): the same keys; the reverse kernel's
    ring holds two more floats per vehicle-step, so max_segment and the default segment are shorter.  ValueError: a segment outside
    0 .. max_segment."""
    return _micro_ckpt_plan("dhts_micro_ckpt_target_plan", " of the target forms", desc, T, want_params, segment)


def micro_rollout_fwd_ckpt_target(desc, T, p, v, params, ckpt, target, head=None, lead=None, lead_length=None, count=None, segment=0,
                                  sse=None, err=None, out=None):
    """micro_rollout_fwd_ckpt (head given) or micro_rollout_fwd_ckpt_lead (lead given) -- exactly one of the two -- that reads the observed
    trajectory `target` (float32 [T][L][2][V], hist's indexing, NaN = not observed) and returns the squared error
    (dhts_micro_rollout_fwd_ckpt_target): (pT, vT, sse), sse float64 [L][2].  ckpt None: no checkpoint is kept.  segment 0: the default
    of micro_ckpt_target_plan."""
    out, sse = _micro_ckpt_fwd("target", desc, T, p, v, params, ckpt, count, segment, err, out, head=head, lead=lead,
                               lead_length=lead_length, target=target, sse=sse)
    return out[0], out[1], sse


def micro_rollout_bwd_ckpt_target(desc, T, ckpt, params, g_p, g_v, target, g_sse=None, head=None, lead=None, lead_length=None, count=None,
                                  segment=0, err=None, out=None, g_head=None, g_lead=None, g_params=None):
    """The reverse sweep of micro_rollout_fwd_ckpt_target (dhts_micro_rollout_bwd_ckpt_target) -> (g_p0, g_v0, g_head) with head, or
    (g_p0, g_v0, g_lead) with lead.  g_sse float64 [L][2] or None (zero): the cotangent of sse; the per-step cotangent
    (float)(2 g_sse) * (x - target) is formed in the kernel.  target, head / lead, lead_length, count, segment: the forward's."""
    return _micro_ckpt_bwd("target", desc, T, ckpt, params, g_p, g_v, count, segment, err, out, g_params, head=head, g_head=g_head,
                           lead=lead, lead_length=lead_length, g_lead=g_lead, target=target, g_sse=g_sse)


# ---- a ring road on the two tape-free paths (dhts_micro_rollout_*_ring) -------------------------------------------------------------------
def micro_rollout_fwd_ckpt_ring(desc, T, p, v, params, ring, ckpt, probes=None, every=1, count=None, segment=0, samples=None, observe=True,
                                err=None, out=None):
    """micro_rollout_fwd_ckpt_lead on a closed lane (dhts_micro_rollout_fwd_ckpt_ring, include/dhts.h): ring float64 [L] = the
    circumference of each lane's ring; the head vehicle follows the image of the tail (slot 0) one circumference ahead, positions stay
    unwrapped.  observe, probes, every, ckpt as micro_rollout_fwd_ckpt_lead.  Returns (pT, vT, samples)."""
    out, samples = _micro_ckpt_fwd("ring", desc, T, p, v, params, ckpt, count, segment, err, out, probes=probes, every=every,
                                   samples=samples, observe=observe, ring=ring)
    return out[0], out[1], samples


def micro_rollout_bwd_ckpt_ring(desc, T, ckpt, params, ring, g_p, g_v, probes=None, every=1, g_samples=None, count=None, segment=0, err=None,
                                out=None, g_params=None):
    """The reverse sweep of micro_rollout_fwd_ckpt_ring (dhts_micro_rollout_bwd_ckpt_ring) -> (g_p0, g_v0): the cotangent of the image
    returns to the tail inside the sweep; no g_head and no g_lead exist.  g_samples=None: nothing was observed.  With g_params the tail's
    length also collects the head's share of the gap.  ring, probes, every, count, segment: the forward's."""
    return _micro_ckpt_bwd("ring", desc, T, ckpt, params, g_p, g_v, count, segment, err, out, g_params, probes=probes, every=every,
                           g_samples=g_samples, ring=ring)[:2]


def micro_rollout_fwd_jvp_ring(desc, T, p, v, params, ring, t_p, t_v, probes=None, every=1, count=None, t_params=None, observe=True, err=None,
                               err_jvp=None, out=None):
    """micro_rollout_fwd_jvp_lead on a closed lane (dhts_micro_rollout_fwd_jvp_ring): the image's tangents are the tail's; no t_head and
    no t_lead exist.  Returns ((pT, vT, samples), (t_pT, t_vT, t_samples))."""
    return _micro_fwd_jvp("ring", desc, T, p, v, params, t_p, t_v, count, t_params, err, err_jvp, out, probes=probes, every=every,
                          observe=observe, ring=ring)


def micro_rollout_fwd_ckpt_target_ring(desc, T, p, v, params, ring, ckpt, target, count=None, segment=0, sse=None, err=None, out=None):
    """micro_rollout_fwd_ckpt_target on a closed lane (dhts_micro_rollout_fwd_ckpt_target_ring) -> (pT, vT, sse)."""
    out, sse = _micro_ckpt_fwd("target", desc, T, p, v, params, ckpt, count, segment, err, out, target=target, sse=sse, ring=ring)
    return out[0], out[1], sse


def micro_rollout_bwd_ckpt_target_ring(desc, T, ckpt, params, ring, g_p, g_v, target, g_sse=None, count=None, segment=0, err=None, out=None,
                                       g_params=None):
    """The reverse sweep of micro_rollout_fwd_ckpt_target_ring (dhts_micro_rollout_bwd_ckpt_target_ring) -> (g_p0, g_v0)."""
    return _micro_ckpt_bwd("target", desc, T, ckpt, params, g_p, g_v, count, segment, err, out, g_params, target=target, g_sse=g_sse,
                           ring=ring)[:2]


def _probe_slots(probes, V):
    """The `probes` argument of dhts.micro_rollout / micro_rollout_jvp, checked as macro_rollout checks `detectors` -> the CUDA int32
    tensor as it is (not validated), or the list of slots (non-empty, strictly ascending, in [0, V); ValueError otherwise)."""
    if isinstance(probes, torch.Tensor) and probes.is_cuda:
        if probes.dtype != torch.int32 or probes.dim() != 1 or not 1 <= probes.numel() <= V:
            raise ValueError("a CUDA `probes` must be a one-dimensional int32 tensor of 1..%d entries" % V)
        return probes.contiguous()
    if isinstance(probes, torch.Tensor):
        if probes.dim() != 1 or probes.dtype.is_floating_point or probes.dtype.is_complex or probes.dtype == torch.bool:
            raise ValueError("`probes` must be a one-dimensional integer tensor")
        slots = probes.tolist()
    else:
        slots = list(probes)
        if any(isinstance(c, bool) or int(c) != c for c in slots):
            raise ValueError("`probes` must hold integers")
        slots = [int(c) for c in slots]
    if not slots:
        raise ValueError("`probes` is empty")
    if any(a >= b for a, b in zip(slots, slots[1:])) or any(not 0 <= c < V for c in slots):
        raise ValueError("`probes` must be strictly ascending vehicle slots in [0, %d) (got %s)" % (V, slots))
    return slots


def micro_sampling(probes, every, V, want_hist):
    """The (probes, every) arguments of dhts.micro_rollout / micro_rollout_jvp -> None when sampling is off (probes is None and every is
    1), else (slots, every) with slots None (every slot), a list of ints or a CUDA int32 tensor.  Every ValueError of the two arguments
    is raised here, before anything touches a device."""
    if isinstance(every, bool) or not isinstance(every, int) or every < 1:
        raise ValueError("every must be an int >= 1, not %r" % (every,))
    if probes is None and every == 1:
        return None
    slots = None if probes is None else _probe_slots(probes, V)
    if want_hist:
        raise ValueError("want_hist and probes / every exclude each other: the history holds every vehicle and step")
    return slots, every


def cut_samples(hist, slots, every, count=None):
    """The samples of a dense history [..][T][L][2][V] (the taped paths: no sampled kernel form exists there): rows every - 1, 2 every - 1,
    ..., the probes' columns, exactly 0 at a slot at or beyond count (the forward leaves those of hist unwritten) and in the column of a
    raw CUDA entry outside [0, V).  Differentiable: autograd scatters the cotangent back into a dense one."""
    V = hist.shape[-1]
    cut = hist[..., every - 1::every, :, :, :]
    if count is not None:
        live = torch.arange(V, device=hist.device)[None, :] < count[:, None]
        cut = torch.where(live[:, None, :], cut, torch.zeros((), dtype=cut.dtype, device=cut.device))
    if slots is None:
        return cut.contiguous()
    idx = slots.long() if isinstance(slots, torch.Tensor) else torch.tensor(slots, dtype=torch.int64, device=hist.device)
    inside = (idx >= 0) & (idx < V)
    cut = cut.index_select(-1, idx.clamp(0, V - 1))
    return torch.where(inside, cut, torch.zeros((), dtype=cut.dtype, device=cut.device))


def _checkpoint_segment(checkpoint, plan):
    """The `checkpoint` argument of micro_rollout / macro_rollout -> None (the taped path) or the segment length to run with; ValueError
    otherwise.  plan(segment) -> the family's checkpoint plan (micro_ckpt_plan, macro_ckpt_plan), which raises for a segment it cannot run."""
    if checkpoint is None or checkpoint is False:
        return None
    if checkpoint is True:
        return plan(0)["segment"]
    try:
        segment = operator.index(checkpoint)
    except TypeError:
        segment = 0
    if segment < 1:
        raise ValueError("checkpoint must be None, False, True or a positive int (the segment length), not %r" % (checkpoint,))
    return plan(segment)["segment"]


def micro_step_bwd(desc, tape, g_p, g_v, count=None):
    """dMicroForwardLayer.backward for a batch of lanes: returns (g_p[L][V], g_v[L][V], g_virtual[L][2] float64),
    g_virtual = raw cotangent of the virtual leader slot (not folded into the head vehicle)."""
    g_p, g_v = _f32c(g_p, "g_p"), _f32c(g_v, "g_v")
    out = (torch.empty_like(g_p), torch.empty_like(g_v))
    g_virtual = torch.zeros(desc.n_lanes, 2, dtype=torch.float64, device=g_p.device)
    call("dhts_micro_step_bwd", d=C.byref(desc), tape=_ptr(tape), count=_ptr(count), g_p=_ptr(g_p), g_v=_ptr(g_v), g_p_out=_ptr(out[0]),
         g_v_out=_ptr(out[1]), g_head=_ptr(g_virtual), err=None, stream=_stream())
    return out[0], out[1], g_virtual


# ---- what the micro autograd Functions share: the segment, the backward's seeds and its fault record ------------------------------------
def _micro_segment(p0, params, T, dt, checkpoint, plan):
    """-> (desc, the segment `checkpoint` asks for or None): a ValueError before a device is touched."""
    L, V = p0.shape
    desc = micro_desc(L, V, dt)
    return desc, _checkpoint_segment(checkpoint, lambda sg: plan(desc, T, params.requires_grad, sg))


def _micro_bwd_seeds(ctx, g_pT, g_vT):
    """-> (g_p, g_v, the reverse sweep's record, cleared)."""
    L, V, dev = ctx.desc.n_lanes, ctx.desc.capacity, ctx.err_bwd.device
    g_p = g_pT.contiguous() if g_pT is not None else torch.zeros(L, V, device=dev)
    g_v = g_vT.contiguous() if g_vT is not None else torch.zeros(L, V, device=dev)
    ctx.err_bwd.zero_()                  # (first fault wins: a second backward with retain_graph must not report the first one's)
    return g_p, g_v, ctx.err_bwd


def _micro_bwd_done(ctx):
    # The record only feeds a warning (the reference's micro backward returns NaNs silently, dmicro_lane.py:271-298): it is not
    # read back here -- that would be a host synchronisation per reverse sweep -- unless the gradient that is being returned
    # anyway is non-finite, which the caller's next use of it would synchronise on as well.
    if ctx.check_faults and not torch.cuda.is_current_stream_capturing():
        MicroRollout.last_bwd_record = ctx.err_bwd           # (dhts.ops.micro_bwd_fault() reads it on demand)


# ---- the checkpointed forms: one row per autograd Function, one forward / backward pair for all of them -------------------
# boundary: what the head vehicle follows and which gradient the backward returns for it -- "head" (g_head), "lead" (g_lead), "head or
# lead" (exactly one is a tensor; a slot for each) or "ring" (data: none).  raw: the raw layer's form; observe: what the third output
# is -- "hist" (when asked), "samples" (unless observe is False) or "fit" (sse).  plan: which plan gives the segment.  sweep_buffers:
# the reverse sweep's outputs that are made in forward (the checkpoint buffer, g_params and both fault records always are).  nones: the
# backward's trailing Nones, one per argument of forward behind the leaves.  No form keeps a checkpoint without a leaf that requires
# grad and none releases its context after backward, so neither is a column here.
_MicroForm = collections.namedtuple("_MicroForm", "boundary raw observe plan sweep_buffers nones")
_MICRO_CKPT_FORMS = {
    "MicroRollout":           _MicroForm("head",         "hist",    "hist",    micro_ckpt_plan,        (),                          6),
    "MicroRolloutSamples":    _MicroForm("head",         "samples", "samples", micro_ckpt_plan,        (),                          7),
    "MicroRolloutLead":       _MicroForm("lead",         "lead",    "samples", micro_ckpt_plan,        ("g_lead",),                 9),
    "MicroRolloutTarget":     _MicroForm("head or lead", "target",  "fit",     micro_ckpt_target_plan, ("g_lead", "g_head", "out"), 7),
    "MicroRolloutRing":       _MicroForm("ring",         "ring",    "samples", micro_ckpt_plan,        (),                          9),
    "MicroRolloutRingTarget": _MicroForm("ring",         "target",  "fit",     micro_ckpt_target_plan, ("out",),                    7),
}


def _micro_ckpt_forward(ctx, name, p0, v0, params, count, T, dt, check_faults, checkpoint, head=None, lead=None, lead_length=None, ring=None,
                        want_hist=False, probes=None, every=1, observe=True, target=None, resolved=None):
    """The forward of every checkpointed form (name: its row of _MICRO_CKPT_FORMS): the segment, the boundary as the kernels read it,
    the one raw call and the fault check -> (pT, vT[, hist | samples | sse]).  Everything the pair needs is made here (no allocation
    inside backward but for a cotangent autograd does not hand over, i.e. none inside a graph capture of it): the checkpoint buffer --
    none when nothing requires grad --, g_params, the form's sweep_buffers and the two fault records; neither tape exists.
    resolved: (desc, segment) where they exist already (MicroRollout, which needs them to choose its path)."""
    form = _MICRO_CKPT_FORMS[name]
    desc, segment = resolved or _micro_segment(p0, params, T, dt, checkpoint, form.plan)
    leaf = head if lead is None else lead
    need_grad = p0.requires_grad or v0.requires_grad or params.requires_grad or (leaf is not None and leaf.requires_grad)
    p0c, v0c = _f32c(p0.detach(), "p0"), _f32c(v0.detach(), "v0")
    L, V, dev = desc.n_lanes, desc.capacity, p0c.device
    ctx.form, ctx.want_hist, ctx.probes, ctx.every, ctx.observe = form, want_hist, probes, every, observe
    ctx.desc, ctx.T, ctx.segment, ctx.count, ctx.check_faults = desc, T, segment, count, check_faults
    ctx.params = params.detach().contiguous()
    ctx.ckpt = torch.empty(micro_ckpt_numel(desc, T, segment), dtype=torch.float32, device=dev) if need_grad else None
    ctx.g_params = torch.empty(6, L, V, dtype=torch.float64, device=dev) if params.requires_grad else None
    err, ctx.err_bwd = new_error_record(dev), new_error_record(dev) if need_grad else None
    ctx.head = None if head is None else head.detach().contiguous()
    ctx.lead = None if lead is None else _f32c(lead.detach(), "lead")
    ctx.lead_length = None if lead_length is None else lead_length.detach().to(device=dev, dtype=torch.float64).contiguous()
    ctx.ring = None if ring is None else ring.detach().to(device=dev).contiguous()
    ctx.target = None if target is None else _f32c(target, "target")
    made = form.sweep_buffers if need_grad else ()
    ctx.g_lead = torch.empty(T, L, 2, dtype=torch.float32, device=dev) if "g_lead" in made and lead is not None else None
    ctx.g_head = torch.zeros(L, 2, dtype=torch.float64, device=dev) if "g_head" in made and lead is None else None
    ctx.out_bwd = (torch.empty_like(p0c), torch.empty_like(v0c)) if "out" in made else None
    hist = torch.empty(T, L, 2, V, dtype=torch.float32, device=dev) if want_hist else None
    out, third = _micro_ckpt_fwd(form.raw, desc, T, p0c, v0c, ctx.params, ctx.ckpt, count, segment, err, None, head=ctx.head, hist=hist,
                                 probes=probes, every=every, observe=observe, lead=ctx.lead, lead_length=ctx.lead_length, target=ctx.target,
                                 ring=ctx.ring)
    if check_faults:                     # a collision is printed like the reference does, and tolerated
        raise_on_fault(err)
    third = hist if form.observe == "hist" else third
    return out if third is None else out + (third,)


def _micro_ckpt_backward(ctx, g_pT, g_vT, g_third=None):
    """The backward of every checkpointed form: the seeds, the cotangent of the third output as the form's sweep takes it, the one raw
    call -> a gradient per argument of the form's forward."""
    form, desc, T = ctx.form, ctx.desc, ctx.T
    g_p, g_v, err = _micro_bwd_seeds(ctx, g_pT, g_vT)
    observed = g_third is not None and {"hist": ctx.want_hist, "samples": ctx.observe, "fit": True}[form.observe]
    g = {form.observe: g_third.contiguous() if observed else None}        # (None: nothing enters there; the fit's kernel takes zero)
    if form.raw == "samples" and not observed:                               # (its sweep alone wants the array)
        P = desc.capacity if ctx.probes is None else int(ctx.probes.numel())
        g["samples"] = torch.zeros(T // ctx.every, desc.n_lanes, 2, P, device=err.device)
    if ctx.g_head is not None:
        ctx.g_head.zero_()
    g_p0, g_v0, g_b = _micro_ckpt_bwd(form.raw, desc, T, ctx.ckpt, ctx.params, g_p, g_v, ctx.count, ctx.segment, err, ctx.out_bwd,
                                      ctx.g_params, head=ctx.head, g_head=ctx.g_head, g_hist=g.get("hist"), probes=ctx.probes,
                                      every=ctx.every, g_samples=g.get("samples"), lead=ctx.lead, lead_length=ctx.lead_length,
                                      g_lead=ctx.g_lead, target=ctx.target, g_sse=g.get("fit"), ring=ctx.ring)
    _micro_bwd_done(ctx)
    if form.boundary == "head or lead":
        g_b = (g_b, None) if ctx.lead is None else (None, g_b)
    else:
        g_b = () if form.boundary == "ring" else (g_b,)
    return (g_p0, g_v0, ctx.g_params) + g_b + (None,) * form.nones


class MicroRollout(torch.autograd.Function):
    """T fused differentiable IDM steps of L independent lanes with a fixed head gap.

    (p0, v0 [L][V]) -> (pT, vT) (+ hist [T][L][2][V]).  What example/inverse/micro.py does with one dMicroLane
    (micro.py:36-118): vehicles ordered tail -> head, head gap = lane defaults (1000, 0).
    The head gap is differentiable: `head` [L][2] float64 receives the cotangent of
    (head_position_delta, head_speed_delta).
    So are the driver parameters: when `params` [6][L][V] float64 requires grad, the forward also fills the parameter tape and the
    reverse sweep returns d loss / d params (what autograd of the reference's plain MicroLane gives for tensor attributes,
    _micro_lane.py:131-214 over _idm.py:30-49); outputs and the other gradients are bit for bit those of a call without it.
    checkpoint (None / False: the taped path; True: the plan's segment length; a positive int: that one): keep the state every so many
    steps instead of the tapes, and let the reverse sweep rebuild one segment of tape at a time in LDS (micro_ckpt_plan) -- the same
    outputs and gradients bit for bit, and the only buffer that grows with T is 8 B per vehicle per segment.  A checkpointed call that
    requires grad is the "MicroRollout" row of _MICRO_CKPT_FORMS: the pair every checkpointed form shares runs it.
    """

    @staticmethod
    def forward(ctx, p0, v0, params, head, count, T, dt, want_hist=False, check_faults=True, checkpoint=None):
        L, V = p0.shape
        desc, segment = _micro_segment(p0, params, T, dt, checkpoint, micro_ckpt_plan)
        want_params = params.requires_grad
        need_grad = p0.requires_grad or v0.requires_grad or head.requires_grad or want_params
        if segment is not None and need_grad:
            return _micro_ckpt_forward(ctx, "MicroRollout", p0, v0, params, count, T, dt, check_faults, checkpoint, head=head,
                                       want_hist=want_hist, resolved=(desc, segment))
        p0c, v0c = _f32c(p0.detach(), "p0"), _f32c(v0.detach(), "v0")
        ctx.segment = None
        tape = torch.empty(micro_tape_numel(desc, T), dtype=torch.float32, device=p0.device) if need_grad else None
        hist = torch.empty(T, L, 2, V, dtype=torch.float32, device=p0.device) if want_hist else None
        err = new_error_record(p0.device)
        # parameter gradient: its tape and its result buffer are made here (nothing is allocated inside backward)
        ctx.ptape = ctx.params = ctx.g_params = None
        if want_params:
            ctx.params = params.detach().contiguous()
            ctx.ptape = torch.empty(micro_param_tape_numel(desc, T), dtype=torch.float32, device=p0.device)
            ctx.g_params = torch.empty(6, L, V, dtype=torch.float64, device=p0.device)
        pT, vT = micro_rollout_fwd(desc, T, p0c, v0c, params.detach(), head.detach(), count=count, tape=tape, hist=hist, err=err,
                                   ptape=ctx.ptape)
        if check_faults:                 # a collision is printed like the reference does, and tolerated
            raise_on_fault(err)
        ctx.desc, ctx.T, ctx.tape, ctx.count, ctx.want_hist, ctx.check_faults = desc, T, tape, count, want_hist, check_faults
        # the reverse sweep's own record, made here (no allocation inside backward, i.e. inside a graph capture of it)
        ctx.err_bwd = new_error_record(p0.device) if need_grad else None
        if want_hist:
            return pT, vT, hist
        return pT, vT

    @staticmethod
    def backward(ctx, g_pT, g_vT, g_hist=None):
        if ctx.segment is not None:
            return _micro_ckpt_backward(ctx, g_pT, g_vT, g_hist)
        g_p, g_v, err = _micro_bwd_seeds(ctx, g_pT, g_vT)
        gh = g_hist.contiguous() if (ctx.want_hist and g_hist is not None) else None
        g_p0, g_v0, g_head = micro_rollout_bwd(ctx.desc, ctx.T, ctx.tape, g_p, g_v, count=ctx.count, g_hist=gh, err=err,
                                               ptape=ctx.ptape, params=ctx.params, g_params=ctx.g_params)
        _micro_bwd_done(ctx)
        return g_p0, g_v0, ctx.g_params, g_head, None, None, None, None, None, None


def micro_bwd_fault(warn=True):
    """Where the most recent micro reverse sweep first met a non-finite cotangent: (step, lane, vehicle) or None.  Reads the sweep's
    fault record back (a host synchronisation: call it once per so many iterations, or when a gradient looks wrong)."""
    rec = getattr(MicroRollout, "last_bwd_record", None)
    if rec is None:
        return None
    code, step, lane, index = rec.tolist()
    if code != _lib.FAULT_NAN:
        return None
    if warn:
        warnings.warn("non-finite gradient in the micro reverse sweep (step %d, lane %d, vehicle %d)" % (step, lane, index), RuntimeWarning)
    return step, lane, index


class MicroRolloutSamples(torch.autograd.Function):
    """MicroRollout's checkpointed call observed at probe slots: (p0, v0 [L][V]) -> (pT, vT, samples [T // every][L][2][P]), samples
    row j = (p, v) of slot probes[i] after step (j + 1) every - 1, exactly 0 at a slot at or beyond the lane's count.  The forward writes
    samples and the reverse sweep reads their cotangent directly (dhts_micro_rollout_fwd_ckpt_samples / _bwd_ckpt_samples): no
    [T][L][2][V] history and no cotangent of one exists, what grows with T is the checkpoint buffer and T // every rows of L 2 P floats.
    probes: None (every slot) or a CUDA int32 tensor; segment: the checkpoint segment length, as MicroRollout's `checkpoint`."""

    @staticmethod
    def forward(ctx, p0, v0, params, head, count, T, dt, check_faults, checkpoint, probes, every):
        return _micro_ckpt_forward(ctx, "MicroRolloutSamples", p0, v0, params, count, T, dt, check_faults, checkpoint, head=head,
                                   probes=probes, every=every)

    @staticmethod
    def backward(ctx, g_pT, g_vT, g_samples):
        return _micro_ckpt_backward(ctx, g_pT, g_vT, g_samples)


class MicroRolloutLead(torch.autograd.Function):
    """MicroRolloutSamples whose head vehicle follows a recorded leader: (p0, v0 [L][V], lead [T][L][2]) -> (pT, vT[, samples]).  No head
    gap exists; `lead` is differentiable, its gradient is the per-step cotangent of the slot in front of the head
    (dhts_micro_rollout_fwd_ckpt_lead / _bwd_ckpt_lead).  observe False: no samples are written or returned."""

    @staticmethod
    def forward(ctx, p0, v0, params, lead, lead_length, count, T, dt, check_faults, checkpoint, probes, every, observe):
        return _micro_ckpt_forward(ctx, "MicroRolloutLead", p0, v0, params, count, T, dt, check_faults, checkpoint, lead=lead,
                                   lead_length=lead_length, probes=probes, every=every, observe=observe)

    @staticmethod
    def backward(ctx, g_pT, g_vT, g_samples=None):
        return _micro_ckpt_backward(ctx, g_pT, g_vT, g_samples)


class MicroRolloutTarget(torch.autograd.Function):
    """MicroRollout's checkpointed call fitted to an observed trajectory inside the kernels: (p0, v0 [L][V], head [L][2] or lead
    [T][L][2]) -> (pT, vT, sse [L][2] float64), sse[l] = the sums over observed entries of target of (x - target)^2 for positions and for
    speeds (dhts_micro_rollout_fwd_ckpt_target / _bwd_ckpt_target).  No [T][L][2][V] history and no cotangent of one exists: the forward
    accumulates, the reverse sweep forms 2 g_sse (x - target) from the state it replays.  Exactly one of head and lead is a tensor."""

    @staticmethod
    def forward(ctx, p0, v0, params, head, lead, lead_length, count, T, dt, check_faults, checkpoint, target):
        return _micro_ckpt_forward(ctx, "MicroRolloutTarget", p0, v0, params, count, T, dt, check_faults, checkpoint, head=head, lead=lead,
                                   lead_length=lead_length, target=target)

    @staticmethod
    def backward(ctx, g_pT, g_vT, g_sse):
        return _micro_ckpt_backward(ctx, g_pT, g_vT, g_sse)


class MicroRolloutRing(torch.autograd.Function):
    """MicroRolloutLead on a closed lane: (p0, v0 [L][V]) -> (pT, vT[, samples]) with the head vehicle following the image of the tail one
    circumference `ring` [L] ahead (dhts_micro_rollout_fwd_ckpt_ring / _bwd_ckpt_ring).  The dependence of the head on the tail is inside
    the kernels: the image's cotangent returns to the tail in the sweep, and no head gap, leader row or gradient of one exists.  ring is
    data.  observe False: no samples are written or returned."""

    @staticmethod
    def forward(ctx, p0, v0, params, ring, count, T, dt, check_faults, checkpoint, probes, every, observe):
        return _micro_ckpt_forward(ctx, "MicroRolloutRing", p0, v0, params, count, T, dt, check_faults, checkpoint, ring=ring,
                                   probes=probes, every=every, observe=observe)

    @staticmethod
    def backward(ctx, g_pT, g_vT, g_samples=None):
        return _micro_ckpt_backward(ctx, g_pT, g_vT, g_samples)


class MicroRolloutRingTarget(torch.autograd.Function):
    """MicroRolloutTarget on a closed lane: (p0, v0 [L][V]) -> (pT, vT, sse [L][2] float64), the trajectory fit of MicroRolloutRing's
    rollout inside the kernels (dhts_micro_rollout_fwd_ckpt_target_ring / _bwd_ckpt_target_ring)."""

    @staticmethod
    def forward(ctx, p0, v0, params, ring, count, T, dt, check_faults, checkpoint, target):
        return _micro_ckpt_forward(ctx, "MicroRolloutRingTarget", p0, v0, params, count, T, dt, check_faults, checkpoint, ring=ring,
                                   target=target)

    @staticmethod
    def backward(ctx, g_pT, g_vT, g_sse):
        return _micro_ckpt_backward(ctx, g_pT, g_vT, g_sse)


def _micro_ring_checks(p0, head, T, ring, lead, lead_length, want_hist, checkpoint):
    """Every ValueError of dhts.micro_rollout's `ring`, raised before anything touches a device."""
    if head is not None:
        raise ValueError("head must be None when ring is given: the head vehicle follows the tail, no head gap exists")
    if lead is not None or lead_length is not None:
        raise ValueError("lead / lead_length must be None when ring is given: the head vehicle follows the tail")
    if want_hist:
        raise ValueError("ring does not take want_hist: the dense history is the sampled form, probes=range(V) with every=1")
    if checkpoint is None or checkpoint is False:
        raise ValueError("ring lives on the tape-free path only: pass checkpoint=True (or a segment length)")
    if p0.dim() != 2:
        raise ValueError("p0 must be [L][V]")
    L = int(p0.shape[0])
    if int(T) < 0:
        raise ValueError("T must be >= 0")
    if not isinstance(ring, torch.Tensor) or ring.dtype != torch.float64 or tuple(ring.shape) != (L,):
        raise ValueError("ring must be a float64 tensor of shape (L,) = (%d,)" % L)
    if ring.requires_grad:
        raise ValueError("ring is not differentiable: pass it detached")


def _micro_target_checks(p0, T, target, want_hist, checkpoint, probes, every):
    """Every ValueError of dhts.micro_rollout's `target`, raised before anything touches a device."""
    if checkpoint is None or checkpoint is False:
        raise ValueError("target lives on the checkpointed path only: pass checkpoint=True (or a segment length)")
    if want_hist:
        raise ValueError("target does not take want_hist: the history is what target= does without")
    if probes is not None or every != 1:
        raise ValueError("target does not take probes / every: it is the dense fit (NaN entries of target are the unobserved ones)")
    if p0.dim() != 2:
        raise ValueError("p0 must be [L][V]")
    L, V = int(p0.shape[0]), int(p0.shape[1])
    if not isinstance(target, torch.Tensor) or target.dtype != torch.float32 or tuple(target.shape) != (int(T), L, 2, V):
        raise ValueError("target must be a float32 tensor of shape (T, L, 2, V) = (%d, %d, 2, %d)" % (int(T), L, V))
    if target.device != p0.device:
        raise ValueError("target must live on p0's device (%s), not %s" % (p0.device, target.device))
    if not target.is_contiguous():
        raise ValueError("target must be contiguous: a copy of it is as large as the history it replaces")
    if target.requires_grad:
        raise ValueError("target is data and not differentiable: pass it detached")


def _micro_lead_checks(p0, head, T, lead, lead_length, want_hist, checkpoint):
    """Every ValueError of dhts.micro_rollout's `lead` / `lead_length`, raised before anything touches a device."""
    if head is not None:
        raise ValueError("head must be None when lead is given: the head vehicle follows `lead`, no head gap exists")
    if want_hist:
        raise ValueError("lead does not take want_hist: the dense history is the sampled form, probes=range(V) with every=1")
    if checkpoint is None or checkpoint is False:
        raise ValueError("lead lives on the tape-free path only: pass checkpoint=True (or a segment length)")
    if p0.dim() != 2:
        raise ValueError("p0 must be [L][V]")
    L = int(p0.shape[0])
    if not isinstance(lead, torch.Tensor) or lead.dtype != torch.float32 or tuple(lead.shape) != (int(T), L, 2):
        raise ValueError("lead must be a float32 tensor of shape (T, L, 2) = (%d, %d, 2)" % (int(T), L))
    if lead_length is not None and (not isinstance(lead_length, torch.Tensor) or lead_length.dtype != torch.float64
                                    or tuple(lead_length.shape) != (L,)):
        raise ValueError("lead_length must be None or a float64 tensor of shape (L,) = (%d,)" % L)
    if lead_length is not None and lead_length.requires_grad:
        raise ValueError("lead_length is not differentiable: pass it detached")


def _device_slots(slots, device):
    """The probes micro_sampling returned, uploaded where they are a checked list (after every ValueError of the call)."""
    return torch.tensor(slots, dtype=torch.int32, device=device) if isinstance(slots, list) else slots


def micro_rollout(p0, v0, params, head, T, dt, count=None, want_hist=False, check_faults=True, checkpoint=None, probes=None, every=1,
                  lead=None, lead_length=None, ring=None, target=None):
    """MicroRollout.  checkpoint=None: the taped reverse mode; True or a segment length: the checkpointed one (same bits, no tape).

    probes / every: observe the trajectory at a few vehicle slots every so many steps.  Sampling is on when probes is not None or
    every != 1, and the call then returns (pT, vT, samples), samples [T // every][L][2][P] float32: row j holds (p, v) of slot probes[i]
    after step (j + 1) every - 1; the trailing T mod every steps give no row (T < every: no row at all); a slot at or beyond a lane's
    count reads exactly 0 and receives no gradient.  samples is differentiable like hist: its cotangent enters the reverse sweep at the
    sampled steps only.  probes: None (every slot, P = V), a sequence of ints or a CPU integer tensor (non-empty, strictly ascending, in
    [0, V): checked, ValueError otherwise, before anything touches a device, then uploaded), or a CUDA int32 tensor, which is used as it
    is and NOT validated: its entries must be distinct, and the kernels never form an address from one outside [0, V) -- that column
    stays 0.  every: an int >= 1.  Not together with want_hist (ValueError): the history holds every vehicle and step.
    With checkpoint= the kernels write and read samples directly and nothing of size T x V is allocated (MicroRolloutSamples).  On the
    taped path (checkpoint=None) the samples are cut out of a dense history: ask for checkpoint= when memory matters.

    lead / lead_length: let the head vehicle of every lane follow a recorded leader instead of a constant head gap.  lead float32
    [T][L][2]: lead[t][l] = (p, v) of the vehicle in front of lane l's head as the head sees it in step t; the head is then an ordinary
    follower (the same gap, collision and clamp rules).  lead_length float64 [L] or None = the head's own length; not differentiable.
    `head` must be None.  lead may require grad: its gradient [T][L][2] is the per-step cotangent of that leader.  It lives on the
    checkpointed path only: checkpoint=True or a segment is required (ValueError otherwise), want_hist is not accepted (ValueError: the
    dense history is probes=range(V), every=1), probes / every work as above; without them the call returns (pT, vT).

    ring: close the lane.  ring float64 [L] = the circumference of each lane's ring in metres (data: not differentiable).  The lane's
    count vehicles drive on a ring road: the head (slot count - 1) follows the image of the tail (slot 0) one circumference ahead, with
    the gap, collision and clamp rules of every follower and half the sum of the tail's and its own length; the gradient flows from the
    head to the tail inside the kernels (MicroRolloutRing).  Positions stay unwrapped -- no modulo is taken, p keeps growing as on an open
    lane.  One vehicle follows its own image; an empty lane passes through.  A ring too short for its vehicles shows as the collision
    fault of every rollout.  `head`, lead and lead_length must be None; checkpoint=True or a segment is required (ValueError otherwise:
    the taped kernels have no ring form), want_hist is not accepted (the dense history is probes=range(V), every=1); probes / every and
    target work as above, and the call returns (pT, vT), (pT, vT, samples) or (pT, vT, sse).

    target: fit the whole trajectory without holding it.  target float32 [T][L][2][V], contiguous, on p0's device, not requiring grad:
    target[t][l][0 / 1][k] = the observed (p, v) of slot k after step t (hist's indexing); a NaN entry is not observed.  The call returns
    (pT, vT, sse), sse float64 [L][2]: per lane the sum over observed entries of (x - target)^2 for positions and for speeds -- the
    float32 difference hist - target, squared and summed in double in a fixed order (the same bits every run; slots at or beyond count
    are never read; T = 0 gives zeros).  sse is differentiable: mean((hist - target)^2) is sse.sum() / target.numel().  Neither hist nor
    its cotangent exists; the kernels read target once per direction (MicroRolloutTarget).  checkpoint=True or a segment is required
    (the segment plan is micro_ckpt_target_plan's: its reverse ring is wider), want_hist / probes / every are not accepted (ValueError),
    lead / lead_length and ring combine with it.  Without a leaf that requires grad no checkpoint is kept: a loss evaluation."""
    # every form's checks, each ValueError where it has always stood and all of them before anything touches a device ...
    fit, led = target is not None, lead is not None or lead_length is not None
    if ring is not None:
        _micro_ring_checks(p0, head, T, ring, lead, lead_length, want_hist, checkpoint)
    if fit:
        _micro_target_checks(p0, T, target, want_hist, checkpoint, probes, every)
    if led and ring is None:
        if lead is None:
            raise ValueError("lead_length needs lead")
        _micro_lead_checks(p0, head, T, lead, lead_length, want_hist, checkpoint)
    elif fit and ring is None and head is None:
        raise ValueError("head must be given (float64 [L][2]) unless lead is")
    sampling = None if fit else micro_sampling(probes, every, int(p0.shape[-1]), want_hist)
    checkpointed = checkpoint is not None and checkpoint is not False
    if (ring is not None or led or fit or (sampling is not None and checkpointed)) and p0.dim() == 2:
        # (a bad `checkpoint` is a ValueError before the probes are uploaded; the plain form's is raised by MicroRollout itself)
        _micro_segment(p0, params, int(T), float(dt), checkpoint, micro_ckpt_target_plan if fit else micro_ckpt_plan)
    # ... the upload, and the form's Function
    slots, ev = sampling if sampling is not None else (None, 1)
    run = (count, int(T), float(dt), bool(check_faults), checkpoint)
    if ring is not None and fit:
        return MicroRolloutRingTarget.apply(p0, v0, params, ring, *run, target)
    if ring is not None:
        return MicroRolloutRing.apply(p0, v0, params, ring, *run, _device_slots(slots, p0.device), ev, sampling is not None)
    if fit:
        return MicroRolloutTarget.apply(p0, v0, params, head, lead, lead_length, *run, target)
    if led:
        return MicroRolloutLead.apply(p0, v0, params, lead, lead_length, *run, _device_slots(slots, p0.device), ev, sampling is not None)
    if sampling is None:
        return MicroRollout.apply(p0, v0, params, head, count, int(T), float(dt), want_hist, bool(check_faults), checkpoint)
    if not checkpointed:                 # the taped path has no sampled kernel form: the samples are cut out of a dense history
        pT, vT, hist = MicroRollout.apply(p0, v0, params, head, count, int(T), float(dt), True, bool(check_faults), None)
        return pT, vT, cut_samples(hist, slots, ev, count)
    return MicroRolloutSamples.apply(p0, v0, params, head, *run, _device_slots(slots, p0.device), ev)


# ---------------------------------------------------------------------------------------------------------
# known-answer / scalar-surface entry points (model.macro._arz, model.macro.darz, model.micro._idm mirrors)
# ---------------------------------------------------------------------------------------------------------
def arz_interface_batch(inp, dt=0.01, dx=5.0, variant=0):
    """inp: float64 [n][9] = rL yL uL ueqL rR yR uR ueqR u_max (CUDA).  Returns a dict of CUDA tensors:
    case [n] int32, q0 [n][4] f64, flux [n][2] f64, dL/dR/fp/A/B [n][2][2] f32, cfl_bad [n] bool, speed [n][2] f64
    (speed0, speed1 of ARZ.riemann_solve)."""
    if inp.dtype != torch.float64 or not inp.is_cuda or inp.dim() != 2 or inp.shape[1] != 9:
        raise TypeError("inp must be a float64 CUDA tensor of shape [n][9]")
    n, dev = inp.shape[0], inp.device
    soa = inp.t().contiguous()
    case = torch.empty(n, dtype=torch.int32, device=dev)
    q0 = torch.empty(4, n, dtype=torch.float64, device=dev)
    flux = torch.empty(2, n, dtype=torch.float64, device=dev)
    f32 = [torch.empty(4, n, dtype=torch.float32, device=dev) for _ in range(5)]
    bad = torch.empty(n, dtype=torch.int32, device=dev)
    speed = torch.empty(2, n, dtype=torch.float64, device=dev)
    call("dhts_arz_interface_batch", n=n, variant=int(variant), dt=float(dt), dx=float(dx), case_ind=_ptr(case), q0=_ptr(q0), flux=_ptr(flux),
         dL=_ptr(f32[0]), dR=_ptr(f32[1]), fp=_ptr(f32[2]), A=_ptr(f32[3]), B=_ptr(f32[4]), cfl_bad=_ptr(bad), speed=_ptr(speed),
         stream=_stream(), **{"in": _ptr(soa)})
    m = [t.t().reshape(n, 2, 2) for t in f32]
    return dict(case=case, q0=q0.t().contiguous(), flux=flux.t().contiguous(), dL=m[0], dR=m[1], fp=m[2], A=m[3], B=m[4],
                cfl_bad=bad.bool(), speed=speed.t().contiguous())


def idm_batch(inp, variant=0):
    """inp: float64 [n][9] = a_max a_pref v v_target dp dv min_space time_pref dt (CUDA).
    Returns next_v (float32-rounded v + dt acc, as f64), acc, dEgo, dLeading [n][2][2] f32, collided [n] bool."""
    if inp.dtype != torch.float64 or not inp.is_cuda or inp.dim() != 2 or inp.shape[1] != 9:
        raise TypeError("inp must be a float64 CUDA tensor of shape [n][9]")
    n, dev = inp.shape[0], inp.device
    soa = inp.t().contiguous()
    nxt = torch.empty(2, n, dtype=torch.float64, device=dev)
    dE = torch.empty(4, n, dtype=torch.float32, device=dev)
    dLd = torch.empty(4, n, dtype=torch.float32, device=dev)
    col = torch.empty(n, dtype=torch.int32, device=dev)
    acs = torch.empty(2, n, dtype=torch.float64, device=dev)
    clips = torch.empty(2, n, dtype=torch.int32, device=dev)
    call("dhts_idm_batch", n=n, variant=int(variant), next_pv=_ptr(nxt), dEgo=_ptr(dE), dLeading=_ptr(dLd), collided=_ptr(col),
         acc_sstar=_ptr(acs), clips=_ptr(clips), stream=_stream(), **{"in": _ptr(soa)})
    return dict(next_p=nxt[0], next_v=nxt[1], dEgo=dE.t().reshape(n, 2, 2), dLeading=dLd.t().reshape(n, 2, 2),
                collided=col.bool(), acc=acs[0], sstar=acs[1], clipped_acc=clips[0].bool(), clipped_spacing=clips[1].bool())


def idm_jac_batch(inp):
    """inp: float64 [n][12] = a_max a_pref v v_target dp dv min_space time_pref optimal_spacing dt clipped_acceleration
    clipped_optimal_spacing (CUDA) -> dEgo, dLeading [n][2][2] float32: dIDM.compute_dEgo / compute_dLeading with the CALLER's
    optimal spacing and clip flags (reference didm.py:13-103)."""
    if inp.dtype != torch.float64 or not inp.is_cuda or inp.dim() != 2 or inp.shape[1] != 12:
        raise TypeError("inp must be a float64 CUDA tensor of shape [n][12]")
    n, dev = inp.shape[0], inp.device
    soa = inp.t().contiguous()
    dE = torch.empty(4, n, dtype=torch.float32, device=dev)
    dLd = torch.empty(4, n, dtype=torch.float32, device=dev)
    call("dhts_idm_jac_batch", n=n, dEgo=_ptr(dE), dLeading=_ptr(dLd), stream=_stream(), **{"in": _ptr(soa)})
    return dE.t().reshape(n, 2, 2), dLd.t().reshape(n, 2, 2)


def idm_param_jac_batch(inp):
    """inp: float64 [n][9] as idm_batch (a_max a_pref v v_target dp dv min_space time_pref dt, dp raw; CUDA) -> d acc / d (a_max, a_pref,
    v_target, min_space, time_pref, dp) [n][6] float64 of IDM.compute_acceleration as the lane's step executes it (reference
    _idm.py:30-49 under _micro_lane.py:151-166), clipped_acc, clipped_spacing [n] bool: the function the parameter reverse sweep calls."""
    if inp.dtype != torch.float64 or not inp.is_cuda or inp.dim() != 2 or inp.shape[1] != 9:
        raise TypeError("inp must be a float64 CUDA tensor of shape [n][9]")
    n, dev = inp.shape[0], inp.device
    soa = inp.t().contiguous()
    dacc = torch.empty(6, n, dtype=torch.float64, device=dev)
    clips = torch.empty(2, n, dtype=torch.int32, device=dev)
    call("dhts_idm_param_jac_batch", n=n, dacc=_ptr(dacc), clips=_ptr(clips), stream=_stream(), **{"in": _ptr(soa)})
    return dacc.t().contiguous(), clips[0].bool(), clips[1].bool()


# ---------------------------------------------------------------------------------------------------------
# macro road network with differentiable signals (itscp `macro` mode), replica batch
# ---------------------------------------------------------------------------------------------------------
def _net_desc(action, tables, n_inter_sq, frames_per_phase, dt, u_max, static_speed, vehicle_length):
    """(action [R][A] as a contiguous float32 tensor, the dhts_net_desc of R replicas of `tables`).  `action` may be the bare shape
    (R, A) instead -- a question about a batch size (net_hybrid_plan), not a launch: nothing is checked against the tables then."""
    a = None if isinstance(action, tuple) else _f32c(action.detach(), "action")
    R, A = action if a is None else a.shape
    if a is not None and tables.n_replica_tables not in (0, R):
        raise ValueError("per-replica tables must match the number of replicas")
    return a, _lib.NetDesc(n_replicas=int(R), n_lanes=tables.n_lanes, n_cells=tables.n_cells, n_steps=tables.T, n_inter_sq=int(n_inter_sq),
                           frames_per_phase=int(frames_per_phase), n_action=int(A), dt=float(dt), u_max=float(u_max),
                           static_speed=float(static_speed), vehicle_length=float(vehicle_length))


class _FaultRecord:
    """Whose dhts_error a network rollout writes, and who reads it (net_macro_rollout / net_hybrid_rollout say it for the caller).
    err = None: the record is ours -- a fresh one per direction, or `own`, one the front end keeps (StepwiseNetwork.err) -- and each
    direction reads it back and raises, unless check_faults is off: reading synchronises, which a HIP-graph capture cannot have.
    A caller's `err` is sticky across calls, is used by both directions and is read by the caller alone; a caller's `err_bwd` takes
    the reverse sweep's faults instead, so that sweep raises nothing either."""

    def __init__(self, device, check_faults=True, err=None, err_bwd=None, own=None):
        self.checked = bool(check_faults) and err is None
        self.fwd = err if err is not None else (own if own is not None else new_error_record(device))
        self._bwd = err_bwd if err_bwd is not None else (err if err is not None else own)
        self._bwd_checked = self.checked and err_bwd is None

    def after_forward(self):
        if self.checked:
            raise_on_fault(self.fwd)

    def for_reverse(self, device):
        return self._bwd if self._bwd is not None else new_error_record(device)

    def after_reverse(self, err):
        if self._bwd_checked:
            raise_on_fault(err)      # a NaN in the reverse sweep asserts like the reference (dmacro_lane.py:308)


class DeviceNetTables:
    """dhts.network.MacroNetworkTables uploaded once; `tables` may be one MacroNetworkTables (shared by all replicas)
    or a list of them (one per replica: same topology, own schedules / per-step routes)."""

    def __init__(self, tables, device):
        up = UploadedTables(tables, device)
        self.n_lanes, self.n_cells, self.T, self.n_replica_tables = up.n_lanes, up.n_cells, up.T, up.n_replica_tables
        self.__dict__.update(up.d)         # the tensors by C field name (dhts.batched.update copies into left_src, ..., schedule)
        self.c = up.net_tables()


class NetMacroRollout(torch.autograd.Function):
    """action [R][A] -> reward [R] of R replicas of a signalised macro network (ItscpEnv.step(action, True) of the
    reference in `macro` mode, reward = - sum of squared queue lengths); also returns the per-step queue terms."""

    @staticmethod
    def forward(ctx, action, dev_tables, n_inter_sq, frames_per_phase, dt, u_max, static_speed, vehicle_length, check_faults=True,
                err=None):
        a, d = _net_desc(action, dev_tables, n_inter_sq, frames_per_phase, dt, u_max, static_speed, vehicle_length)
        R = d.n_replicas
        hist_n, tape_n = raw("dhts_net_macro_hist_bytes", d=C.byref(d)) // 4, raw("dhts_net_macro_tape_bytes", d=C.byref(d)) // 4
        if hist_n == 0:
            raise ValueError("unsupported network size (need cells + lanes <= 1024 and lanes <= cells)")
        dev = a.device
        hist = torch.empty(hist_n, dtype=torch.float32, device=dev)
        tape = torch.empty(tape_n, dtype=torch.float32, device=dev)
        kc = torch.empty(R, dev_tables.T, dev_tables.n_cells, dtype=torch.float32, device=dev)
        queue = torch.empty(R, dev_tables.T, dev_tables.n_lanes, dtype=torch.float32, device=dev)
        reward = torch.empty(R, dtype=torch.float32, device=dev)
        ws = torch.zeros(R * dev_tables.T * 2 * dev_tables.n_lanes, dtype=torch.float32, device=dev)
        rec = _FaultRecord(dev, check_faults, err)
        call("dhts_net_macro_rollout_fwd", d=C.byref(d), t=C.byref(dev_tables.c), action=_ptr(a), hist=_ptr(hist), tape=_ptr(tape), kc=_ptr(kc),
             queue=_ptr(queue), reward=_ptr(reward), workspace=_ptr(ws), err=_ptr(rec.fwd), stream=_stream())
        rec.after_forward()
        ctx.d, ctx.tables, ctx.rec = d, dev_tables, rec
        ctx.save_for_backward(a, hist, tape, kc, queue, ws)
        ctx.mark_non_differentiable(queue)
        return reward, queue

    @staticmethod
    def backward(ctx, g_reward, _g_queue):
        a, hist, tape, kc, queue, ws = ctx.saved_tensors
        d = ctx.d
        g_action = torch.empty_like(a)
        err = ctx.rec.for_reverse(a.device)
        g = g_reward.contiguous().float()          # a named local: the (possibly fresh) tensor must outlive the launch
        call("dhts_net_macro_rollout_bwd", d=C.byref(d), t=C.byref(ctx.tables.c), action=_ptr(a), hist=_ptr(hist), tape=_ptr(tape),
             kc=_ptr(kc), queue=_ptr(queue), g_reward=_ptr(g), g_action=_ptr(g_action), workspace=_ptr(ws), err=_ptr(err), stream=_stream())
        ctx.rec.after_reverse(err)
        return g_action, None, None, None, None, None, None, None, None, None


def net_macro_rollout(action, dev_tables, n_inter_sq, frames_per_phase, dt, u_max, static_speed=0.2, vehicle_length=5.0,
                      check_faults=True, err=None):
    """Returns (reward [R], queue [R][T][L]).  check_faults=False: nothing is read back (no host sync; usable inside a
    HIP-graph capture); faults stay in the device record.  err: a caller-owned sticky fault record (new_error_record) used
    by both directions and read by the caller when it wants to (raise_on_fault)."""
    return NetMacroRollout.apply(action, dev_tables, int(n_inter_sq), int(frames_per_phase), float(dt), float(u_max),
                                 float(static_speed), float(vehicle_length), bool(check_faults), err)


def net_macro_eval(action, dev_tables, n_inter_sq, frames_per_phase, dt, u_max, static_speed=0.2, vehicle_length=5.0, err=None):
    """An evaluation episode (ItscpEnv.step(action, False) of the reference: hard signal / boundary / is_static thresholds,
    trainer.py:94-142) of R replicas of a macro network: returns (reward [R], queue [R][T][L]); nothing differentiable."""
    a, d = _net_desc(action, dev_tables, n_inter_sq, frames_per_phase, dt, u_max, static_speed, vehicle_length)
    R = d.n_replicas
    queue = torch.empty(R, dev_tables.T, dev_tables.n_lanes, dtype=torch.float32, device=a.device)
    reward = torch.empty(R, dtype=torch.float32, device=a.device)
    rec = _FaultRecord(a.device, err=err)
    call("dhts_net_macro_rollout_eval", d=C.byref(d), t=C.byref(dev_tables.c), action=_ptr(a), queue=_ptr(queue), reward=_ptr(reward),
         err=_ptr(rec.fwd), stream=_stream())
    rec.after_forward()
    return reward, queue


_NET_MACRO_PLAN_KEYS = ("fwd_block", "loss_waves", "fwd_bound", "bwd_block", "bwd_bound")


def net_macro_plan(n_action, dev_tables, n_inter_sq=1, frames_per_phase=1, dt=1.0 / 30.0, u_max=30.0):
    """What net_macro_rollout launches for this network (dhts_net_macro_plan): the forward kernel's block, whether it runs the loss on
    wavefronts of its own, its launch bound; the reverse sweep's block (net_macro_eval's too) and launch bound.  `dev_tables`: anything
    with n_lanes, n_cells, T and n_replica_tables (DeviceNetTables) -- nothing is launched."""
    _, d = _net_desc((1, n_action), dev_tables, n_inter_sq, frames_per_phase, dt, u_max, 0.2, 5.0)
    plan = (C.c_int32 * 8)()
    call("dhts_net_macro_plan", d=C.byref(d), plan=C.byref(plan))
    out = dict(zip(_NET_MACRO_PLAN_KEYS, [int(x) for x in plan]))
    out["loss_waves"] = bool(out["loss_waves"])
    return out


class DeviceHybridTables:
    """dhts.network.HybridNetworkTables plus the pre-drawn vehicle routes [n_routes][stride] (int, -1 padded; the k-th
    vehicle spawned onto a lane takes the k-th route starting there, cyclically), uploaded once.  `tables` may be one
    HybridNetworkTables (shared by all replicas) or a list of them (one per replica: same topology, own inflow schedules
    and per-step macro routes)."""

    def __init__(self, tables, routes, device, records_per_step=0, lane_capacity=0, vehicle_params=None):
        """vehicle_params [n_routes][6] (rows as `routes`): the IDM attributes of the vehicle that takes each route row
        (dhts_hybrid_tables::veh_params); None = every vehicle a default_micro_vehicle(speed_limit)."""
        if lane_capacity not in (0, 16, 32, 64, 128):
            raise ValueError("lane_capacity (vehicles a micro lane holds at once) must be 0 (= 16), 16, 32, 64 or 128")
        self.lane_capacity, self.records_per_step = int(lane_capacity), int(records_per_step)
        self.two_per_cu = 0                # dhts_hybrid_tables::two_per_cu: 0 = DHTS_OPT_HYB_PACK decides, 1 = packed, -1 = one replica per unit
        for x in tables if isinstance(tables, (list, tuple)) else [tables]:
            x.check_kernel_limits()
        up = self._up = UploadedTables(tables, device, routes, vehicle_params)
        for name in ("n_lanes", "n_cells", "T", "n_replica_tables", "n_micro", "has_sources", "micro_tensor_ladder"):
            setattr(self, name, getattr(up, name))
        self.net = up.net_tables()         # (filled once: nothing here rebinds a tensor, see set_draws)

    def first(self, n_replicas):
        """The same uploaded tables as a batch of the first `n_replicas` replicas (no copy: the per-replica arrays are
        replica-major, so a shorter batch reads a prefix of them)."""
        import copy
        if not 1 <= int(n_replicas) <= max(self.n_replica_tables, 1) and self.n_replica_tables:
            raise ValueError("tables hold %d replicas" % self.n_replica_tables)
        v = copy.copy(self)
        if self.n_replica_tables:
            v.n_replica_tables = int(n_replicas)
        return v

    def schedules(self):
        """The uploaded inflow schedules read back to the host: float64 [R][T][L], one per replica of this batch (a `first(n)`
        view gives its n), or [1][T][L] for tables shared by all replicas."""
        s = self._up.d["schedule"].cpu().numpy().reshape(-1, self.T, self.n_lanes)
        return s[:self.n_replica_tables] if self.n_replica_tables else s

    def set_draws(self, draws):
        """A fresh stream of admission draws for the next episode (micro source lanes; same length as the uploaded one), copied
        into the uploaded tensor (UploadedTables.replace says when that is sound)."""
        self._up.set_draws(draws, in_place=True)

    def c(self, loss_steps=0):
        return self._up.hybrid_tables(self.net, records_per_step=self.records_per_step, loss_steps=int(loss_steps),
                                      lane_capacity=self.lane_capacity, two_per_cu=int(self.two_per_cu))


def _hybrid_buffers(d, tc, dev):
    """What a fused hybrid rollout writes: (hist, tape, kc, queue [R][T][L], reward [R], counts [R][4], workspace)."""
    R, T = d.n_replicas, d.n_steps
    ws_n = raw("dhts_net_hybrid_workspace_bytes", d=C.byref(d), t=C.byref(tc))
    if ws_n == 0:
        raise ValueError("unsupported hybrid network size")
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)      # noqa: E731
    # (an all-micro network has no cells: the kernels' unconditional prefetches still want something to read)
    return (f32(max(R * (T + 1) * 4 * d.n_cells, 64)), f32(max(raw("dhts_net_hybrid_tape_bytes", d=C.byref(d)) // 4, 64)),
            f32(max(R * T * d.n_cells, 64)), f32(R, T, d.n_lanes), f32(R), torch.zeros(R, 4, dtype=torch.int32, device=dev),
            torch.empty(ws_n, dtype=torch.uint8, device=dev))


class NetHybridRollout(torch.autograd.Function):
    """action [R][A] -> reward [R] of R replicas of a signalised hybrid network (ItscpEnv.step(action, True) of the
    reference in `hybrid` mode); also returns the per-step queue terms and (spawned, deposited, records) per replica.
    loss_steps > 0 restricts the differentiated reward to the first loss_steps steps (second output `reward_cut`)."""

    @staticmethod
    def forward(ctx, action, dev_tables, n_inter_sq, frames_per_phase, dt, u_max, static_speed, vehicle_length, loss_steps,
                check_faults=True, err=None, err_bwd=None):
        t = dev_tables
        a, d = _net_desc(action, t, n_inter_sq, frames_per_phase, dt, u_max, static_speed, vehicle_length)
        R = d.n_replicas
        tc = t.c(loss_steps)
        dev = a.device
        hist, tape, kc, queue, reward, counts, ws = _hybrid_buffers(d, tc, dev)
        rec = _FaultRecord(dev, check_faults, err, err_bwd)

        def launch(tc):
            call("dhts_net_hybrid_rollout_fwd", d=C.byref(d), t=C.byref(tc), action=_ptr(a), hist=_ptr(hist), tape=_ptr(tape), kc=_ptr(kc),
                 queue=_ptr(queue), reward=_ptr(reward), counts=_ptr(counts), workspace=_ptr(ws), err=_ptr(rec.fwd), stream=_stream())
            rec.after_forward()
        try:
            launch(tc)
        except CapacityError:            # (raised only where the record is ours and check_faults is on)
            # two replicas per compute unit (more replicas than units) halve the record staging area: the same batch once more
            # with one replica per unit before the caller hears of it (the reverse sweep follows the tables it is given)
            plan = (C.c_int32 * 8)()
            call("dhts_net_hybrid_plan", d=C.byref(d), t=C.byref(tc), plan=plan)
            if not plan[0]:
                raise
            import copy
            t = copy.copy(t)
            t.two_per_cu = -1
            rec.fwd.zero_()
            counts.zero_()
            launch(t.c(loss_steps))
        # (a caller's record -- err, or err_bwd for the reverse sweep alone -- is the caller's to read: that is how a batch
        # tolerates one member's NaN)
        ctx.d, ctx.tables, ctx.loss_steps, ctx.rec = d, t, int(loss_steps), rec
        ctx.save_for_backward(a, hist, tape, kc, queue, ws)
        ctx.mark_non_differentiable(reward, queue, counts)
        if loss_steps and loss_steps > 0:
            # reference accumulation order: lanes outer, steps inner
            cut = -(queue[:, :int(loss_steps), :].transpose(1, 2).reshape(R, -1).sum(dim=1))
        else:
            cut = reward.clone()
        return cut, reward, queue, counts

    @staticmethod
    def backward(ctx, g_cut, _g_reward, _g_queue, _g_counts):
        a, hist, tape, kc, queue, ws = ctx.saved_tensors
        d = ctx.d
        tc = ctx.tables.c(ctx.loss_steps)
        g_action = torch.empty_like(a)
        err = ctx.rec.for_reverse(a.device)
        g = g_cut.contiguous().float()             # a named local: the (possibly fresh) tensor must outlive the launch
        call("dhts_net_hybrid_rollout_bwd", d=C.byref(d), t=C.byref(tc), action=_ptr(a), hist=_ptr(hist), tape=_ptr(tape), kc=_ptr(kc),
             queue=_ptr(queue), g_reward=_ptr(g), g_action=_ptr(g_action), workspace=_ptr(ws), err=_ptr(err), stream=_stream())
        ctx.rec.after_reverse(err)
        return g_action, None, None, None, None, None, None, None, None, None, None, None


class NetHybridStateRollout(torch.autograd.Function):
    """R replicas of a road network of ARZ and IDM lanes that starts from a GIVEN state, all T steps in one launch each way:
    (r0, u0 [R][C]) -> (rT, yT, uT [R][C], veh [R][128][4], events, counts).  With dev_tables built by
    HybridNetworkTables.plain(...) and plain = True this is T x RoadNetwork.forward(dt, True) of the reference on the network
    of example/inverse/hybrid.py (macro -> micro -> macro: flux-capacitor spawns, IDM steps, deposits; hybrid.py:37-146,
    _inverse.py:91-99) with its backward pass: cotangents of the final (r, u) of every cell and of the final (position, speed)
    of every vehicle go back to (r0, u0).  ghost0 [R][L][4] = stored (r, u) of each lane's upstream / downstream ghost
    (set_leftmost_cell / set_rightmost_cell), constants."""

    @staticmethod
    def forward(ctx, r0, u0, ghost0, dev_tables, dt, u_max, plain, vehicle_length, check_faults):
        t = dev_tables
        R, Cc = r0.shape
        if Cc != t.n_cells:
            raise ValueError("state must be [R][%d cells]" % t.n_cells)
        dev = r0.device
        r0c, u0c = _f32c(r0.detach(), "r0"), _f32c(u0.detach(), "u0")
        action = torch.full((R, 1), 0.5, dtype=torch.float32, device=dev)                # no signals: one dummy phase
        action, d = _net_desc(action, t, 1, max(int(t.T), 1), dt, u_max, 0.2, vehicle_length)
        y0, q0 = macro_state_from_ru(r0c, u0c, u_max)
        state0 = torch.stack([r0c, y0, u0c, q0], dim=1).contiguous()                       # [R][4][C]
        g0 = None if ghost0 is None else _f32c(ghost0.detach(), "ghost0")
        if g0 is not None and tuple(g0.shape) != (R, t.n_lanes, 4):
            raise ValueError("ghost0 must be [R][%d lanes][4]" % t.n_lanes)
        tc = t.c(0)
        hist, tape, kc, queue, reward, counts, ws = _hybrid_buffers(d, tc, dev)
        veh = torch.zeros(R, 128, 4, dtype=torch.float32, device=dev)
        veh[:, :, 0] = -1.0
        events = torch.full((R, 256, 2), -1, dtype=torch.int32, device=dev)
        err = new_error_record(dev)
        io = _lib.HybridStateIO(plain=1 if plain else 0, state0=_ptr(state0), ghost0=_ptr(g0), veh_out=_ptr(veh), events=_ptr(events))
        call("dhts_net_hybrid_state_rollout_fwd", d=C.byref(d), t=C.byref(tc), io=C.byref(io), action=_ptr(action), hist=_ptr(hist),
             tape=_ptr(tape), kc=_ptr(kc), queue=_ptr(queue), reward=_ptr(reward), counts=_ptr(counts), workspace=_ptr(ws), err=_ptr(err),
             stream=_stream())
        if check_faults:
            raise_on_fault(err)
        fin = hist[:R * (t.T + 1) * 4 * t.n_cells].view(R, t.T + 1, 4, t.n_cells)[:, t.T]
        rT, yT, uT = fin[:, 0].clone(), fin[:, 1].clone(), fin[:, 2].clone()
        ctx.d, ctx.tables, ctx.plain, ctx.u_max, ctx.check_faults = d, t, bool(plain), float(u_max), bool(check_faults)
        ctx.save_for_backward(action, hist, tape, kc, queue, ws, r0c, u0c, rT, yT)
        ctx.mark_non_differentiable(yT, events, counts)
        return rT, yT, uT, veh, events, counts

    @staticmethod
    def backward(ctx, g_rT, _g_yT, g_uT, g_veh, _g_ev, _g_counts):
        action, hist, tape, kc, queue, ws, r0c, u0c, rT, yT = ctx.saved_tensors
        d, t = ctx.d, ctx.tables
        R, Cc = r0c.shape
        dev = r0c.device
        z = lambda: torch.zeros(R, Cc, dtype=torch.float32, device=dev)      # noqa: E731
        g_r = g_rT.contiguous().float() if g_rT is not None else z()
        g_u = g_uT.contiguous().float() if g_uT is not None else z()
        g_stateT = torch.stack([g_r, z(), g_u], dim=1).contiguous()          # the kernel turns the speed's cotangent into (r, y)'s itself
        gv = None
        if g_veh is not None:
            gv = g_veh[:, :, 1:3].contiguous().float()                        # cotangent of (position, speed)
        g_reward = torch.zeros(R, dtype=torch.float32, device=dev)            # a pure state tap
        g_action = torch.empty_like(action)
        g_state0 = torch.empty(R, 3, Cc, dtype=torch.float32, device=dev)
        err = new_error_record(dev)
        tc = t.c(0)
        call("dhts_net_hybrid_state_rollout_bwd", d=C.byref(d), t=C.byref(tc), plain=1 if ctx.plain else 0, action=_ptr(action),
             hist=_ptr(hist), tape=_ptr(tape), kc=_ptr(kc), queue=_ptr(queue), g_reward=_ptr(g_reward), g_stateT=_ptr(g_stateT), g_veh=_ptr(gv),
             g_action=_ptr(g_action), g_state0=_ptr(g_state0), workspace=_ptr(ws), err=_ptr(err), stream=_stream())
        if ctx.check_faults:
            raise_on_fault(err)
        # initial (r, y, u) -> (r0, u0): y0 = r0 (u0 - u_eq(r0)) (FullQ.from_r_u), u0 itself where step 0 read the given speed
        g_r0 = g_state0[:, 0].contiguous()
        g_y0 = g_state0[:, 1].contiguous()
        g_u0 = macro_state_from_ru_bwd(r0c, u0c, g_y0, g_r0, ctx.u_max)
        g_u0 = g_u0 + g_state0[:, 2]
        return g_r0, g_u0, None, None, None, None, None, None, None


def net_hybrid_state_rollout(r0, u0, dev_tables, dt, u_max, ghost0=None, plain=True, vehicle_length=5.0, check_faults=True):
    """(rT, yT, uT [R][C], veh [R][128][4] = (lane or -1, position, speed, a) per spawned vehicle, events [R][256][2] = (step, kind),
    counts [R][4] = (spawned, deposited, records, events)); differentiable in r0, u0 through rT, uT and veh[..., 1:3]."""
    return NetHybridStateRollout.apply(r0, u0, ghost0, dev_tables, float(dt), float(u_max), bool(plain), float(vehicle_length),
                                       bool(check_faults))


def net_hybrid_plan(n_replicas, n_action, dev_tables, n_inter_sq=1, frames_per_phase=1, dt=1.0 / 30.0, u_max=30.0):
    """What net_hybrid_rollout would launch for a batch of `n_replicas` under the current DHTS_OPT_HYB_PACK (dhts_net_hybrid_plan):
    {"packed": two replicas per compute unit, "block", "stage_h", "lds_fwd", "lds_bwd", "loc_lanes", "max_step_records", "cus"}."""
    t = dev_tables
    _, d = _net_desc((n_replicas, n_action), t, n_inter_sq, frames_per_phase, dt, u_max, 0.2, 5.0)
    tc = t.c(0)
    plan = (C.c_int32 * 8)()
    call("dhts_net_hybrid_plan", d=C.byref(d), t=C.byref(tc), plan=plan)
    keys = ("packed", "block", "stage_h", "lds_fwd", "lds_bwd", "loc_lanes", "max_step_records", "cus")
    out = dict(zip(keys, [int(x) for x in plan]))
    out["packed"] = bool(out["packed"])
    return out


def net_hybrid_eval(action, dev_tables, n_inter_sq, frames_per_phase, dt, u_max, static_speed=0.2, vehicle_length=5.0, err=None):
    """An evaluation episode (hard thresholds, see net_macro_eval) of R replicas of a hybrid network: returns
    (reward [R], queue [R][T][L], counts [R][4] = vehicles spawned, vehicles deposited, 0, 0)."""
    t = dev_tables
    a, d = _net_desc(action, t, n_inter_sq, frames_per_phase, dt, u_max, static_speed, vehicle_length)
    R = d.n_replicas
    tc = t.c(0)
    queue = torch.empty(R, t.T, t.n_lanes, dtype=torch.float32, device=a.device)
    reward = torch.empty(R, dtype=torch.float32, device=a.device)
    counts = torch.zeros(R, 4, dtype=torch.int32, device=a.device)
    rec = _FaultRecord(a.device, err=err)
    call("dhts_net_hybrid_rollout_eval", d=C.byref(d), t=C.byref(tc), action=_ptr(a), queue=_ptr(queue), reward=_ptr(reward),
         counts=_ptr(counts), err=_ptr(rec.fwd), stream=_stream())
    rec.after_forward()
    return reward, queue, counts


def net_hybrid_rollout(action, dev_tables, n_inter_sq, frames_per_phase, dt, u_max, static_speed=0.2, vehicle_length=5.0,
                       loss_steps=0, check_faults=True, err=None, err_bwd=None):
    """Returns (reward restricted to the first loss_steps steps [differentiable], full reward, queue [R][T][L], counts [R][4]).
    check_faults=False: nothing is read back in either direction (no host sync; usable inside a HIP-graph capture), and a
    non-finite cotangent in the reverse sweep (the reference asserts on it, dmacro_lane.py:308; it
    happens e.g. when a head gap clamps to exactly 0 and the IDM Jacobian divides by it, didm.py:60-70) is left in the
    returned gradient of that replica instead of raising, so that a batch survives one bad member.
    err: a caller-owned sticky fault record (new_error_record) used by both directions instead of a fresh one per call; the
    caller reads it when it wants to (raise_on_fault) -- a training loop checks once per so many iterations, not twice per pass.
    err_bwd: a second caller-owned record for the reverse sweep alone, for callers that tolerate its NaN fault (a batch with one
    bad member) but not the forward's CFL / capacity faults: the first fault wins a record, so the two must not share one."""
    return NetHybridRollout.apply(action, dev_tables, int(n_inter_sq), int(frames_per_phase), float(dt), float(u_max),
                                  float(static_speed), float(vehicle_length), int(loss_steps), bool(check_faults), err, err_bwd)
