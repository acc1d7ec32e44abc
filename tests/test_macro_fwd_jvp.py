"""The tape-free fused rollout + tangent kernel of the ARZ rollout (dhts_macro_rollout_fwd_jvp / dhts_macro_fwd_jvp_plan,
ops.macro_rollout_fwd_jvp, dhts.macro_rollout_jvp(fused=True)): the boundary of the library -- header, bindings, exports, argument
checks, the plan, the operator's ValueErrors.  What it computes is held against the taped path bit for bit in
tests/test_macro_fwd_jvp_gpu.py.  No GPU needed."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dhts_macro_rollout_fwd_jvp", "dhts_macro_fwd_jvp_plan")
# the arguments between (d, T) and stream, in the header's order; ints carry their value, pointers default to a non-NULL dummy
ARGS = ("n_dir", "r", "y", "u", "ueq", "ghost", "ghost_is_sched", "t_r", "t_y", "t_ghost", "r_out", "y_out", "u_out", "ueq_out",
        "t_r_out", "t_y_out", "det", "n_det", "taps", "t_taps", "err", "err_jvp", "stream")
INTS = dict(n_dir=3, ghost_is_sched=0, n_det=2)
REQUIRED = ("r", "y", "u", "ueq", "ghost", "t_r", "t_y", "r_out", "y_out", "u_out", "ueq_out", "t_r_out", "t_y_out")


def test_header_library_and_bindings_hold_the_new_entry_points():
    import dhts
    from dhts import _lib, ops
    raw = open(os.path.join(ROOT, "include", "dhts.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib.lib()
    for name in NEW:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, txt)
        assert m, "include/dhts.h does not declare %s" % name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
        assert len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name          # the header's argument count
    assert len(_lib.SIGNATURES[NEW[0]][1]) == 2 + len(ARGS) == 25 and len(_lib.SIGNATURES[NEW[1]][1]) == 5
    comment = raw[raw.index("The rollout AND n_dir = K tangent directions of it in one kernel, without a tape: what dhts_macro"):
                  raw.index("int " + NEW[0])]
    for cited in ("_macro_lane.py:83-146", "dmacro_lane.py:96-132", ":277-309"):      # what the pair it replaces cites
        assert cited in comment
    for name in ("macro_rollout_fwd_jvp", "macro_fwd_jvp_plan"):
        assert callable(getattr(ops, name))
    assert inspect.signature(dhts.macro_rollout_jvp).parameters["fused"].default is False, "the default stays the taped path"


def fused_args(some, **kw):
    a = {n: INTS.get(n, some) for n in ARGS}
    a["stream"] = None
    a.update(kw)
    return [a[n] for n in ARGS]


def test_bad_arguments_are_rejected_without_a_gpu():
    from dhts import _lib
    lib = _lib.lib()
    ok = _lib.MacroDesc(4, 70, 0.01, 5.0, 30.0)
    some = C.c_void_p(64)                      # a non-NULL pointer that is never dereferenced: the checks come first
    run, plan = lib.dhts_macro_rollout_fwd_jvp, lib.dhts_macro_fwd_jvp_plan
    out = (C.c_int32 * 8)()
    nodet = dict(det=None, taps=None, t_taps=None, n_det=0)
    long_lane = _lib.MacroDesc(4, _lib.MACRO_MAX_CELLS, 0.01, 5.0, 30.0)        # a valid descriptor whose lane does not fit (kmax = 0)
    for T in (0, 3):
        for n_dir in (0, -2):
            assert run(C.byref(ok), T, *fused_args(some, n_dir=n_dir)) == _lib.E_INVALID
        for missing in REQUIRED:
            assert run(C.byref(ok), T, *fused_args(some, **{missing: None})) == _lib.E_INVALID
            assert run(C.byref(ok), T, *fused_args(some, t_ghost=None, err=None, err_jvp=None, **dict(nodet, **{missing: None}))) == _lib.E_INVALID
        # det without both taps and t_taps, or the reverse
        for kw in (dict(taps=None), dict(t_taps=None), dict(taps=None, t_taps=None), dict(det=None), dict(det=None, taps=None),
                   dict(det=None, t_taps=None)):
            assert run(C.byref(ok), T, *fused_args(some, **kw)) == _lib.E_INVALID, kw
        for n_det in (0, -1, 71):
            assert run(C.byref(ok), T, *fused_args(some, n_det=n_det)) == _lib.E_INVALID
        assert run(C.byref(long_lane), T, *fused_args(some)) == _lib.E_INVALID
        assert run(C.byref(long_lane), T, *fused_args(some, **nodet)) == _lib.E_INVALID
        for bad in (_lib.MacroDesc(4, _lib.MACRO_MAX_CELLS + 1, 0.01, 5.0, 30.0), _lib.MacroDesc(4, 0, 0.01, 5.0, 30.0),
                    _lib.MacroDesc(0, 70, 0.01, 5.0, 30.0), _lib.MacroDesc(4, 70, 0.0, 5.0, 30.0), _lib.MacroDesc(4, 70, 0.01, 0.0, 30.0),
                    _lib.MacroDesc(4, 70, 0.01, 5.0, 0.0)):
            assert run(C.byref(bad), T, *fused_args(some)) == _lib.E_INVALID
            assert plan(C.byref(bad), T, 1, 0, C.byref(out)) == _lib.E_INVALID
        assert run(None, T, *fused_args(some)) == _lib.E_INVALID
        assert plan(None, T, 1, 0, C.byref(out)) == _lib.E_INVALID
        assert plan(C.byref(ok), T, 1, 0, None) == _lib.E_INVALID
        assert plan(C.byref(ok), T, 0, 0, C.byref(out)) == _lib.E_INVALID
        assert plan(C.byref(ok), T, 1, 71, C.byref(out)) == _lib.E_INVALID
    assert run(C.byref(ok), -1, *fused_args(some)) == _lib.E_INVALID
    assert plan(C.byref(ok), -1, 1, 0, C.byref(out)) == _lib.E_INVALID


def jvp_width(rem, kmax):
    """host_common.hpp: launches of 4, then 2, then 1; a remainder of 3 rides in one launch of 4."""
    if rem >= 3 and kmax >= 4:
        return 4
    k = min(kmax, 2)
    while k > rem:
        k >>= 1
    return k


def lds_bytes(N, k):
    """The lane kernel's records (48 B a cell record, 16 B a flux, 4 B a queue entry, 16 B of counters; to 16 B), two float4 products per
    interface, two float2 tangent copies per direction."""
    rec = (48 * (N + 2) + 16 * (N + 1) + 4 * (N + 2) + 16 + 15) // 16 * 16
    return rec + 32 * (N + 1) + 16 * k * (N + 2)


def test_the_plan_needs_no_device():
    from dhts import _lib, ops
    for N in (1, 64, 65, 512, 1000, 1024, _lib.MACRO_MAX_CELLS):
        for T in (0, 5):
            desc = ops.macro_desc(3, N, 0.01, 5.0, 30.0)
            kmax = ops.macro_fwd_jvp_plan(desc, 5, 9)["dirs_per_launch"]
            if N <= 512:
                assert kmax == 4
            elif N <= 1024:
                assert kmax >= 2
            elif N == _lib.MACRO_MAX_CELLS:
                assert kmax == 0
            # the widest launch is the widest whose LDS fits 160 KB
            assert kmax == max([k for k in (4, 2, 1) if lds_bytes(N, k) <= 160 * 1024], default=0)
            for K in range(1, 10):
                p = ops.macro_fwd_jvp_plan(desc, T, K)
                assert set(p) == {"waves", "passes", "dirs_per_launch", "launches", "lds_bytes"}
                assert p["lds_bytes"] <= 160 * 1024
                if kmax == 0:
                    assert p["dirs_per_launch"] == 0 and p["launches"] == 0 and p["lds_bytes"] == 0
                    continue
                assert p["waves"] >= 1 and p["passes"] >= 1 and 64 * p["waves"] * p["passes"] >= N > 64 * p["passes"] * (p["waves"] - 1)
                roll = ops.macro_rollout_plan(desc, T)
                assert (p["waves"], p["passes"]) == (roll["fwd_waves"], roll["fwd_passes"]), "W and p as macro_plan has them for the lane kernel"
                widths, rem = [], K
                while rem > 0:
                    widths.append(jvp_width(rem, kmax))
                    rem -= min(widths[-1], rem)
                assert p["dirs_per_launch"] == widths[0] and p["lds_bytes"] == lds_bytes(N, widths[0])
                assert p["launches"] == (len(widths) if T else 0), (N, T, K, p)
                if K >= 3 and N <= 512:
                    assert p["dirs_per_launch"] == 4
            assert ops.macro_fwd_jvp_plan(desc, 5, 3)["launches"] == (0 if kmax == 0 else (1 if kmax == 4 else 2))


def test_value_errors_of_the_operator_are_unchanged_with_fused():
    import torch
    import dhts
    L, N, T, K = 2, 8, 5, 3
    r0, u0 = torch.full((L, N), 0.3), torch.full((L, N), 10.0)
    gr, gu = torch.full((L, 2), 0.3), torch.full((L, 2), 10.0)
    sr, su = torch.full((T, L, 2), 0.3), torch.full((T, L, 2), 10.0)
    tr = torch.zeros(K, L, N)
    bad = [
        dict(),                                                       # no tangent at all
        dict(t_r0=torch.zeros(L, N)),                                 # no direction axis
        dict(t_r0=torch.zeros(0, L, N)),                              # K = 0
        dict(t_r0=tr, t_u0=torch.zeros(K + 1, L, N)),                 # two values of K
        dict(t_u0=torch.zeros(K, L, N + 1)),
        dict(t_r0=torch.zeros(K, L + 1, N)),
        dict(t_r0=tr, t_ghost_r=torch.zeros(K, L, 3)),
        dict(t_ghost_u=torch.zeros(K, L)),
        dict(t_r0=tr, t_ghost_r=torch.zeros(K, T, L, 2)),             # a schedule's tangent beside constant boundary cells
        dict(t_r0=tr, t_ghost_u=torch.zeros(K + 1, L, 2)),
        dict(t_r0=[[0.0]]),                                           # not a tensor
    ]
    for fused in (False, True):
        def run(*a, **kw):
            return dhts.macro_rollout_jvp(*a, fused=fused, **kw)

        for kw in bad:
            with pytest.raises(ValueError):
                run(r0, u0, gr, gu, T, 0.01, 5.0, 30.0, **kw)
        with pytest.raises(ValueError):
            run(r0, u0, sr, su, T, 0.01, 5.0, 30.0, t_r0=tr, t_ghost_r=torch.zeros(K, L, 2))      # constant tangent beside a schedule
        with pytest.raises(ValueError):
            run(r0, u0, sr, su, T, 0.01, 5.0, 30.0, t_r0=tr, t_ghost_r=torch.zeros(K, T + 1, L, 2))
        with pytest.raises(ValueError):
            run(r0, torch.zeros(L, N + 1), gr, gu, T, 0.01, 5.0, 30.0, t_r0=tr)
        with pytest.raises(ValueError):
            run(r0, u0, gr, su, T, 0.01, 5.0, 30.0, t_r0=tr)
        with pytest.raises(ValueError):
            run(r0, u0, sr[:T - 1], su[:T - 1], T, 0.01, 5.0, 30.0, t_r0=tr)
        with pytest.raises(ValueError):
            run(torch.zeros(N), torch.zeros(N), gr, gu, T, 0.01, 5.0, 30.0, t_r0=tr)
        with pytest.raises(TypeError):
            run(r0, u0, gr, gu, T, 0.01, 5.0, 30.0, tr)                 # tangents are keyword-only
    # the raw wrappers' own, in their order: the state, the boundary cells, the tangents; the readings only behind the device check
    from dhts import ops
    desc = ops.macro_desc(L, N, 0.01, 5.0, 30.0)
    z, ghost, taps = torch.zeros(L, N), torch.zeros(L, 2, 4), torch.zeros(T, L, 3, 2)

    def raw(r=z, q=z, ghost=ghost, t_r=tr, T=T, **kw):
        return ops.macro_rollout_fwd_jvp(desc, T, r, z, z, q, ghost, t_r, tr, **kw)
    with pytest.raises(ValueError, match="^T must be >= 0$"):
        raw(T=-1, r=torch.zeros(L, N + 1))
    with pytest.raises(ValueError, match=r"^r must have shape \(2, 8\)$"):
        raw(r=torch.zeros(L, N + 1), q=torch.zeros(L), ghost=torch.zeros(L, 2), taps=taps)
    with pytest.raises(ValueError, match=r"^ueq must have shape \(2, 8\)$"):
        raw(q=torch.zeros(L), ghost=torch.zeros(L, 2), taps=taps)
    with pytest.raises(ValueError, match=r"^ghost must have shape \(2, 2, 4\) or \(5, 2, 2, 4\)$"):
        raw(ghost=torch.zeros(T + 1, L, 2, 4), t_r=torch.zeros(L, N))
    for t_r in (torch.zeros(L, N), torch.zeros(0, L, N), torch.zeros(K + 1, L, N)):
        for call in (lambda: raw(t_r=t_r, taps=taps), lambda: ops.macro_rollout_jvp(desc, T, None, t_r, tr, t_taps=taps)):
            with pytest.raises(ValueError, match=r"^t_r and t_y must have shape \(K, 2, 8\) with K >= 1$"):
                call()
    for call in (lambda: raw(taps=taps), lambda: raw(t_ghost=torch.zeros(K, L, 2)),
                 lambda: ops.macro_rollout_jvp(desc, T, None, tr, tr, t_taps=taps),
                 lambda: ops.macro_rollout_jvp(desc, T, None, tr, tr, t_ghost=torch.zeros(K, L, 2))):
        with pytest.raises(TypeError, match="must be a float32 CUDA tensor"):
            call()


def test_a_lane_that_does_not_fit_is_a_value_error_before_any_device():
    """kmax = 0: the message names the number of cells and says fused=False covers it; CPU tensors, so nothing was launched."""
    import torch
    import dhts
    from dhts import _lib
    N = _lib.MACRO_MAX_CELLS
    r0, u0 = torch.full((1, N), 0.3), torch.full((1, N), 10.0)
    g = torch.full((1, 2), 0.3)
    with pytest.raises(ValueError) as e:
        dhts.macro_rollout_jvp(r0, u0, g, g, 2, 0.01, 5.0, 30.0, t_r0=torch.zeros(1, 1, N), fused=True)
    assert str(N) in str(e.value) and "fused=False" in str(e.value)
