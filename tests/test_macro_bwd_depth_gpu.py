"""The reverse sweep without per-step cotangents (macro_rollout_bwd_fast_kernel, kHist = kTaps = false) loads every S entry once, hands
the right interface's entry over by DPP moves and a small LDS array at the wavefront boundaries, and rotates six S sets through a
six-step round.  The yardstick is the instantiation WITH per-step cotangents, which keeps the three-set code: the same call with
g_hist = zeros runs it, and both must give the same bits (adding zero changes no value; torch.equal compares values).

Shapes: 4 lanes; N over the masked and full forms, the wavefront boundary at 63 / 64 / 65 and a partly filled last wavefront; T over every
residue of the six-step round, rollouts shorter than the pipeline (T < 8) and both loop exits.  All T of one (input, N) run in one case."""
import numpy as np
import pytest

from util import options

pytestmark = pytest.mark.gpu
DT, DX, UM = 0.01, 5.0, 30.0
L = 4
NS = (2, 63, 64, 65, 128, 130, 256, 300, 512, 1024)
TS = (1, 2, 3, 5, 6, 7, 8, 11, 12, 13, 19, 25)
KINDS = ("bench", "smooth", "onephase")
FAST = 1                                  # plan: bwd_pipelined
_BENCH = {}


def lane_inputs(kind, N):
    """(r0, u0, ghost r, ghost u) as CPU tensors.  bench / onephase: bench.py's distribution (about half the interfaces are exceptions in the
    first steps), cut to N cells; smooth: one constant state, boundary cells included -- only the standing exceptions, every other block
    comes from S and so from the hand-over."""
    import torch
    if kind == "smooth":
        return (torch.full((L, N), 0.4), torch.full((L, N), 12.0), torch.full((L, 2), 0.4), torch.full((L, 2), 12.0))
    if not _BENCH:
        import bench
        _BENCH["t"] = bench.MacroWorkload.inputs(0, L, max(NS), UM)
    r0, u0, gr, gu = _BENCH["t"]
    return r0[:, :N].contiguous(), u0[:, :N].contiguous(), gr, gu


def forward(cuda, kind, N, T, sched):
    """One forward rollout; returns (desc, tape, g_r, g_y): the tape and the cotangent of a loss on the final state."""
    import torch
    from dhts import ops
    r0, u0, gr, gu = (t.to(cuda) for t in lane_inputs(kind, N))
    y0, q0 = ops.macro_state_from_ru(r0, u0, UM)
    gy, gq = ops.macro_state_from_ru(gr, gu, UM)
    ghost = torch.stack([gr, gy, gu, gq], dim=-1).contiguous()
    desc = ops.macro_desc(L, N, DT, DX, UM)
    tape = torch.zeros(ops.macro_tape_numel(desc, T), dtype=torch.float32, device=cuda)
    err = ops.new_error_record(cuda)
    with options(1 if kind == "onephase" else 0, 0):
        if sched:
            out = ops.macro_rollout_fwd_sched(desc, T, r0, y0, u0, q0, ghost[None].expand(T, L, 2, 4).contiguous(), tape=tape, err=err)
        else:
            out = ops.macro_rollout_fwd(desc, T, r0, y0, u0, q0, ghost, tape=tape, err=err)
    assert err.tolist()[0] == 0, err.tolist()
    return desc, tape, 2 * out[0], 0.5 * out[1]


def both_paths(cuda, desc, T, tape, g_r, g_y, sched):
    """(deep path, three-set path with zero per-step cotangents): each (g_r0, g_y0, g_ghost, error record)."""
    import torch
    from dhts import ops
    bwd = ops.macro_rollout_bwd_sched if sched else ops.macro_rollout_bwd
    zeros = torch.zeros(T, desc.n_lanes, 2, desc.n_cells, device=cuda)
    res = []
    for g_hist in (None, zeros):
        err = ops.new_error_record(cuda)
        res.append(tuple(bwd(desc, T, tape, g_r, g_y, g_hist=g_hist, err=err)) + (err.tolist(),))
    return res


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("kind", KINDS)
def test_same_bits_as_the_three_set_sweep(cuda, kind, N):
    import torch
    from dhts import ops
    for T in TS:
        desc = ops.macro_desc(L, N, DT, DX, UM)
        for hist in (False, True):
            assert ops.macro_rollout_plan(desc, T, want_hist=hist)["bwd_pipelined"] == FAST
        for sched in (False, True):
            desc, tape, g_r, g_y = forward(cuda, kind, N, T, sched)
            if kind == "onephase":        # every interface is an exception: N + 1 of them, more than the block's threads where N = block
                rows = tape.view(T * L, -1)
                s_f4 = ((3 * N + 3) // 4 + 7) // 8 * 8
                assert int(rows[:, 4 * s_f4].contiguous().view(torch.int32).min()) == N + 1
            deep, three = both_paths(cuda, desc, T, tape, g_r, g_y, sched)
            tag = "%s N %d T %d %s" % (kind, N, T, "sched" if sched else "plain")
            assert deep[3][0] == 0 and three[3][0] == 0, (tag, deep[3], three[3])
            for name, a, b in zip(("g_r0", "g_y0", "g_ghost"), deep, three):
                assert a.shape == b.shape and bool(torch.isfinite(a).all()), (tag, name)
                assert torch.equal(a, b), "%s %s: %d entries differ, max |d| %.3e" % (
                    tag, name, int((a != b).sum()), float((a.double() - b.double()).abs().max()))
            assert float(deep[0].abs().max()) > 0, tag


@pytest.mark.parametrize("N", (128, 130))
def test_nan_in_an_s_entry_leaves_the_same_fault_record(cuda, N):
    """NaN in the S entry of interface 64 -- the entry lane 63 of wavefront 0 takes from the LDS array and thread 64 holds itself.
    Step 0: the entry feeds d1 of cell 63 (its right interface) and d0 of cell 64 (its left one), whose product goes to cell 63, so
    after step 0 cell 63 alone is not finite and ONE thread reports: the record is a function of the input, (NaN, step 0, lane, 63).
    A NaN at a later step spreads one cell per step to both sides and several threads report, the first wins: there the record of
    either path must lie in that cone."""
    import torch
    from dhts import _lib
    T, lane = 13, 2
    desc, tape, g_r, g_y = forward(cuda, "smooth", N, T, False)
    for step in (0, 7):
        bad = tape.clone()
        rows = bad.view(T * L, -1)
        rows[step * L + lane, 3 * 64] = float("nan")
        deep, three = both_paths(cuda, desc, T, bad, g_r, g_y, False)
        print("N %d step %d: deep %s three-set %s" % (N, step, deep[3], three[3]))
        for rec in (deep[3], three[3]):
            assert rec[0] == _lib.FAULT_NAN and rec[2] == lane, rec
            assert 0 <= rec[1] <= step and 63 - (step - rec[1]) <= rec[3] <= 64 + (step - rec[1]), rec
        if step == 0:
            assert deep[3] == three[3] == [_lib.FAULT_NAN, 0, lane, 63]
        for a in deep[:2]:
            other = [i for i in range(L) if i != lane]
            assert bool(torch.isfinite(a[other]).all())
