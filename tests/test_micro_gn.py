"""The Gauss-Newton normal equations inside the fused micro rollout (dhts_micro_rollout_fwd_jvp_gn, dhts_micro_fwd_jvp_gn_plan,
ops.micro_rollout_fwd_jvp_gn, dhts.micro_rollout_jvp(fused=True, target=)): the numpy restatement against a brute-force J^T J, the
pair-of-blocks launch schedule, the plan, the boundary of the library and every ValueError.  What the kernels compute is held against
existing device code in tests/test_micro_gn_gpu.py.  No GPU needed."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import micro_gn_ref as G
from micro_jvp_ref import chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ("p", "v", "count", "params", "head", "lead", "lead_length", "ring", "t_p", "t_v", "t_head", "t_lead", "t_params", "p_out", "v_out",
        "t_p_out", "t_v_out", "probes", "n_probes", "every", "target", "sse", "jtr", "jtj", "err", "err_jvp", "stream")
LAUNCHES = {4: (1, 1, 1, 1, 3, 3, 6, 6), 2: (1, 1, 3, 6, 10, 15, 21, 28)}      # K = 1 .. 8 at launch widths 4 and 2


# =================================================================================================================
# the restatement
# =================================================================================================================
@pytest.mark.parametrize("n", (0, 1, 5, 9))
def test_restatement_against_a_brute_force_normal_matrix_of_the_chains_own_history(n):
    """K = 3 directions of micro_jvp_ref.chain on random tape blocks: J is the masked t_hist, one row per observed entry; J^T J and
    J^T r in float64 matrix products against the restatement's fsum, within n 2^-52 sum|terms| (the matrix product's own order)."""
    T, V, K = 11, 9, 3
    rng = np.random.default_rng(7 + n)
    dqs = rng.uniform(-1, 1, (T, V, 2, 2, 2)).astype(np.float32)
    dqs[:, :, 0, 0, 0], dqs[:, :, 0, 0, 1], dqs[:, :, 1, 0] = 1.0, 0.01, 0.0
    t = np.stack([chain(dqs, rng.standard_normal(V), rng.standard_normal(V), rng.standard_normal(2), n)[2] for _ in range(K)])
    x = rng.uniform(0, 100, (T, 2, V)).astype(np.float32)
    target = (x + rng.standard_normal(x.shape)).astype(np.float32)
    target[rng.uniform(size=x.shape) < 0.2] = np.nan
    target[:, :, n:] = np.nan if n % 2 else 1e30                 # garbage at slots at or beyond count
    live = np.arange(V) < n
    (sse, jtr, jtj), (terms, abs_jtr, abs_jtj) = G.normal_equations(x, t, target, live)
    seen = ~np.isnan(target) & live[None, None, :]
    assert terms == int(seen.sum())
    J = np.stack([t[a][seen] for a in range(K)], 1).astype(np.float64)          # [terms][K]
    r = (x - target).astype(np.float32)[seen].astype(np.float64)
    for got, want, mag in ((jtj, J.T @ J, abs_jtj), (jtr, J.T @ r, abs_jtr)):
        ok, ratio = G.within_bound(got[None], want[None], mag[None], [terms])
        assert ok, (got, want)
    for c in range(2):
        rc = (x - target).astype(np.float32)[:, c][seen[:, c]].astype(np.float64)
        assert abs(sse[c] - rc @ rc) <= max(terms, 1) * 2.0 ** -52 * sse[c]
    assert np.array_equal(jtj, jtj.T)
    if n == 0:
        assert not jtj.any() and not jtr.any() and not sse.any()
    # the vectorised form of the same sums (the GPU tests' yardstick) agrees within the same bound
    e = G.expected(x[:, None], t[:, :, None], target[:, None], live[None])
    for key, got in (("sse", sse), ("jtr", jtr), ("jtj", jtj)):
        assert G.within_bound(e[key], got[None], e["abs_" + key], e["n"])[0], key
    assert int(e["n"][0]) == terms


# =================================================================================================================
# the launch schedule and the plan
# =================================================================================================================
@pytest.mark.parametrize("width", (4, 2))
def test_pair_of_blocks_schedule_covers_every_pair_of_directions(width):
    from dhts import ops
    for K in range(1, 9):
        launches = ops.micro_gn_launches(K, width)
        assert len(launches) == LAUNCHES[width][K - 1], (K, width)
        assert all(1 <= len(d) <= width and len(set(d)) == len(d) and all(0 <= i < K for i in d) for d in launches)
        met = {(a, b) for d in launches for a in d for b in d}
        assert met == {(a, b) for a in range(K) for b in range(K)}, "K = %d, width %d: a pair of directions meets in no launch" % (K, width)
        if K <= width:
            assert launches == [tuple(range(K))]
    assert ops.micro_gn_launches(1, 1) == [(0,)] and ops.micro_gn_launches(2, 1) == [] and ops.micro_gn_launches(0, 4) == []


def test_plan_through_the_library():
    """Width 4 at V = 256 with parameters; never 0 at V <= 1024 for K = 1; the launch counts are the schedule's; the LDS is the sibling's."""
    from dhts import ops
    for V in (1, 5, 64, 65, 130, 256, 257, 512, 513, 1000, 1024):
        desc = ops.micro_desc(3, V, 0.01)
        for want_params in (False, True):
            one = ops.micro_fwd_jvp_gn_plan(desc, 1000, 1, want_params)
            assert one["launches"] == 1 and one["dirs_per_launch"] >= 1, (V, want_params)
            assert one["block"] == (V + 63) // 64 * 64 == ops.micro_fwd_jvp_plan(desc, 1000, 1, want_params)["block"]
            width = one["dirs_per_launch"]
            assert width in (1, 2, 4)
            if V <= 256:
                assert width == 4, "a lane of up to 256 vehicles carries 4 directions per launch, with t_params too"
            for K in range(1, 9):
                plan = ops.micro_fwd_jvp_gn_plan(desc, 1000, K, want_params)
                assert plan["dirs_per_launch"] == width and plan["block"] <= plan["block_bound"]
                assert plan["launches"] == len(ops.micro_gn_launches(K, width)) == LAUNCHES.get(width, (1,) + (0,) * 7)[K - 1]
                assert plan["pair_block"] == (K if K <= width else width // 2)
                widest = 4 if K >= 3 and width >= 4 else (2 if K >= 2 and width >= 2 else 1)
                assert plan["lds_bytes"] == 8 * (2 + 2 * widest) * (V + 1) + 16 * widest <= 160 * 1024
                assert plan["lds_bytes"] == ops.micro_fwd_jvp_plan(desc, 1000, widest, want_params)["lds_bytes"], "the sibling's bytes"
    assert ops.micro_fwd_jvp_gn_plan(ops.micro_desc(3, 256, 0.01), 1000, 5, True)["launches"] == 3
    assert ops.micro_fwd_jvp_gn_plan(ops.micro_desc(3, 1024, 0.01), 5, 5, True)["dirs_per_launch"] == 2


def test_no_gn_kernel_has_scratch_or_a_spill_and_the_parents_kernels_keep_their_figures():
    """The committed compiler listings: every kernel of the parent's listing stands in the new one with every field, and every new
    kernel is a Gauss-Newton instantiation with scratch 0 and no spill.  This compares two committed text files: it documents what
    the listings say and cannot notice a kernel that changes without a regenerated listing; it is no evidence about the compiled
    code, which the GPU tests and a fresh listing give."""
    def listing(name):
        rows = {}
        for line in open(os.path.join(ROOT, "profiles", name)):
            m = re.match(r"(.*?)\s+SGPRs\s", line)
            rows[m.group(1)] = line[m.end(1):].split()
        return rows
    parent, new = listing("micro_gn_resources_parent.txt"), listing("micro_gn_resources.txt")
    assert all(new.get(k) == v for k, v in parent.items()), [k for k, v in parent.items() if new.get(k) != v]
    added = sorted(set(new) - set(parent))
    assert added and all(k.startswith("micro_rollout_fwd_jvp_gn_kernel<") for k in added)
    for k in added:
        f = dict(zip(new[k][0::2], new[k][1::2]))
        assert f["scratch"] == "0" and f["sgpr_spill"] == "0" and f["vgpr_spill"] == "0", (k, f)
    assert any(k.startswith("micro_rollout_fwd_jvp_gn_kernel<4, true") for k in added)


# =================================================================================================================
# the boundary of the library
# =================================================================================================================
def test_header_library_and_bindings_hold_the_new_entry_points():
    import dhts
    from dhts import _lib, ops
    raw = open(os.path.join(ROOT, "include", "dhts.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib.lib()
    m = re.search(r"\bdhts_micro_rollout_fwd_jvp_gn\s*\(([^;]*)\)\s*;", txt)
    assert m and lib.dhts_micro_rollout_fwd_jvp_gn is not None
    declared = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert declared[3:] == list(ARGS) and len(_lib.SIGNATURES["dhts_micro_rollout_fwd_jvp_gn"][1]) == len(ARGS) + 3
    ints = [i for i, t in enumerate(_lib.SIGNATURES["dhts_micro_rollout_fwd_jvp_gn"][1]) if t is C.c_int]
    assert ints == [1, 2, 3 + ARGS.index("n_probes"), 3 + ARGS.index("every")]
    assert re.search(r"\bdhts_micro_fwd_jvp_gn_plan\s*\(", txt)
    assert _lib.SIGNATURES["dhts_micro_fwd_jvp_gn_plan"] == _lib.SIGNATURES["dhts_micro_fwd_jvp_plan"]
    comment = raw[raw.index("GAUSS-NEWTON NORMAL EQUATIONS"):raw.index("int dhts_micro_rollout_fwd_jvp_gn")]
    for cited in ("DHTS_E_INVALID", "[L][n_dir][n_dir] double", "NaN", "exactly 0", "no atomics", "PAIR", "plan[2]", "DHTS_FAULT_CAPACITY"):
        assert cited in comment, cited
    assert callable(ops.micro_rollout_fwd_jvp_gn) and callable(ops.micro_fwd_jvp_gn_plan)
    par = inspect.signature(dhts.micro_rollout_jvp).parameters
    assert par["target"].default is None and list(par)[-1] == "target" and par["target"].kind is inspect.Parameter.KEYWORD_ONLY


def test_bad_arguments_are_rejected_without_a_gpu():
    """DHTS_E_INVALID with nothing dereferenced: `some` is a pointer nobody may follow, and no device exists here to launch on."""
    from dhts import _lib
    lib = _lib.lib()
    ok = _lib.MicroDesc(4, 70, 0.01)
    some = C.c_void_p(64)

    def call(desc=ok, T=5, K=2, **kw):
        a = {k: some for k in ARGS}
        a.update(stream=None, lead=None, lead_length=None, ring=None, t_lead=None, probes=None, n_probes=0, every=1)
        a.update(kw)
        return lib.dhts_micro_rollout_fwd_jvp_gn(C.byref(desc), T, K, *[a[k] for k in ARGS])

    for name in ("p", "v", "params", "p_out", "v_out", "t_p", "t_v", "t_p_out", "t_v_out", "target", "sse", "jtr", "jtj"):
        assert call(**{name: None}) == _lib.E_INVALID, name
    assert call(head=None, t_head=None) == _lib.E_INVALID, "no boundary at all"
    assert call(lead=some) == _lib.E_INVALID and call(ring=some) == _lib.E_INVALID, "two boundaries"
    assert call(head=None, t_head=None, lead=some, ring=some) == _lib.E_INVALID
    assert call(head=None, ring=some) == _lib.E_INVALID, "t_head without head"
    assert call(t_lead=some) == _lib.E_INVALID and call(lead_length=some) == _lib.E_INVALID, "t_lead / lead_length without lead"
    assert call(head=None, t_head=None, ring=some, t_lead=some) == _lib.E_INVALID
    assert call(K=0) == _lib.E_INVALID and call(T=-1) == _lib.E_INVALID and call(every=0) == _lib.E_INVALID
    assert call(probes=some, n_probes=0) == _lib.E_INVALID and call(probes=some, n_probes=71) == _lib.E_INVALID
    assert call(desc=_lib.MicroDesc(4, 1025, 0.01)) == _lib.E_INVALID and call(desc=_lib.MicroDesc(0, 70, 0.01)) == _lib.E_INVALID
    plan = (C.c_int32 * 8)()
    assert lib.dhts_micro_fwd_jvp_gn_plan(C.byref(ok), 5, 0, 1, C.byref(plan)) == _lib.E_INVALID
    assert lib.dhts_micro_fwd_jvp_gn_plan(C.byref(ok), -1, 1, 1, C.byref(plan)) == _lib.E_INVALID
    assert lib.dhts_micro_fwd_jvp_gn_plan(C.byref(ok), 5, 1, 1, None) == _lib.E_INVALID
    assert lib.dhts_micro_fwd_jvp_gn_plan(None, 5, 1, 1, C.byref(plan)) == _lib.E_INVALID


# =================================================================================================================
# every ValueError of the public call, on CPU tensors: nothing is launched
# =================================================================================================================
def inputs(L=3, V=8, T=6, K=2):
    import torch
    p0 = torch.arange(V, dtype=torch.float32).repeat(L, 1) * 20.0
    v0 = torch.full((L, V), 10.0)
    par = torch.ones(6, L, V, dtype=torch.float64)
    head = torch.tensor([[1000.0, 0.0]] * L, dtype=torch.float64)
    return p0, v0, par, head, dict(t_p0=torch.ones(K, L, V))


def test_every_value_error_before_a_device_is_touched(monkeypatch):
    import torch
    import dhts
    from dhts import ops
    L, V, T, K = 3, 8, 6, 2
    p0, v0, par, head, tan = inputs(L, V, T, K)
    good = torch.zeros(T, L, 2, V)
    lead, ring = torch.zeros(T, L, 2), torch.full((L,), 500.0, dtype=torch.float64)

    def call(target, match, head_=head, T_=T, **kw):
        kw = dict(dict(fused=True), **kw)
        with pytest.raises(ValueError, match=match):
            dhts.micro_rollout_jvp(p0, v0, par, head_, T_, 0.01, target=target, **tan, **kw)

    call(good, "fused=True", fused=False)
    call(good, "want_hist", want_hist=True)
    call(good.double(), "float32")
    call(good.numpy(), "tensor")
    for shape in ((T, L, 2), (T + 1, L, 2, V), (T, L, 2, V + 1), (L, T, 2, V), (T // 2, L, 2, V)):
        call(torch.zeros(shape), "shape")
    call(torch.zeros(T // 2, L, 2, 3), "shape", probes=[0, 3, 7])                  # the rows of every = 1, not of every = 2 ...
    call(torch.zeros(T, L, 2, V), "shape", probes=[0, 3, 7], every=2)             # ... and the dense shape with sampling on
    call(torch.zeros(T, L, 2, V), "shape", every=4)
    call(torch.zeros(T, L, 2, V, device="meta"), "device")
    call(torch.zeros(T, L, V, 2).transpose(2, 3), "contiguous")
    call(torch.zeros(T, L, 2, V, requires_grad=True), "require grad")
    # the same checks on the other two boundaries
    for kw in (dict(lead=lead), dict(ring=ring)):
        call(good.double(), "float32", head_=None, **kw)
        call(torch.zeros(T, L, 2, V + 1), "shape", head_=None, **kw)
        call(good, "fused=True", head_=None, fused=False, **kw)
        call(torch.zeros(T // 3, L, 2, 2, requires_grad=True), "require grad", head_=None, probes=[1, 5], every=3, **kw)
    # a K the plan cannot carry: the kernels this library holds carry every K (width >= 2), so the plan is made to answer as a
    # library whose widest kernel for the lane holds one direction would
    real = ops.micro_fwd_jvp_gn_plan

    def narrow(desc, T_, n_dir, want_params=False):
        plan = real(desc, T_, n_dir, want_params)
        plan.update(dirs_per_launch=1, launches=1 if n_dir == 1 else 0, pair_block=1 if n_dir == 1 else 0)
        return plan
    monkeypatch.setattr(ops, "micro_fwd_jvp_gn_plan", narrow)
    call(good, r"V = 8.*carries 1 direction .*K = 2")
    monkeypatch.undo()
    # nothing above reached a device: a good call on CPU tensors stops where every fused call does, at the first upload check
    with pytest.raises(TypeError, match="CUDA"):
        dhts.micro_rollout_jvp(p0, v0, par, head, T, 0.01, target=good, fused=True, **tan)
    # the raw wrapper: its own checks
    desc = ops.micro_desc(L, V, 0.01)
    t = torch.zeros(K, L, V)
    with pytest.raises(ValueError, match="exactly one"):
        ops.micro_rollout_fwd_jvp_gn(desc, T, p0, v0, par, t, t, good)
    with pytest.raises(ValueError, match="exactly one"):
        ops.micro_rollout_fwd_jvp_gn(desc, T, p0, v0, par, t, t, good, head=head, ring=ring)
    with pytest.raises(ValueError, match="t_head needs head"):
        ops.micro_rollout_fwd_jvp_gn(desc, T, p0, v0, par, t, t, good, ring=ring, t_head=torch.zeros(K, L, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match="need lead"):
        ops.micro_rollout_fwd_jvp_gn(desc, T, p0, v0, par, t, t, good, head=head, t_lead=torch.zeros(K, T, L, 2))
    with pytest.raises(ValueError, match="contiguous float32 tensor of shape"):
        ops.micro_rollout_fwd_jvp_gn(desc, T, p0, v0, par, t, t, good[:, :, :, :4], head=head)
    with pytest.raises(ValueError, match="target must be given"):
        ops.micro_rollout_fwd_jvp_gn(desc, T, p0, v0, par, t, t, None, head=head)


def test_calls_without_target_are_untouched():
    """Without target= the keyword changes nothing: the same ValueErrors from the same places."""
    import dhts
    p0, v0, par, head, tan = inputs()
    with pytest.raises(ValueError, match="exclude each other"):
        dhts.micro_rollout_jvp(p0, v0, par, head, 6, 0.01, fused=True, want_hist=True, every=2, **tan)
    with pytest.raises(TypeError, match="CUDA"):
        dhts.micro_rollout_jvp(p0, v0, par, head, 6, 0.01, fused=True, **tan)
