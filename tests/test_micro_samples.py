"""Probe samples of the micro rollout (dhts_micro_rollout_fwd_ckpt_samples / _bwd_ckpt_samples / _fwd_jvp_samples, the ops wrappers of the
same names, dhts.micro_rollout(probes=, every=) and dhts.micro_rollout_jvp(probes=, every=)): the boundary of the library -- header,
bindings, exports, argument checks, the operators' ValueErrors and defaults.  What they compute is held against the dense history in
tests/test_micro_samples_gpu.py.  No GPU needed."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dhts_micro_rollout_fwd_ckpt_samples", "dhts_micro_rollout_bwd_ckpt_samples", "dhts_micro_rollout_fwd_jvp_samples")
FWD = ("p", "v", "count", "params", "head", "p_out", "v_out", "ckpt", "probes", "n_probes", "every", "samples", "err", "stream")
FWD_REQUIRED = ("p", "v", "params", "head", "p_out", "v_out")
BWD = ("ckpt", "count", "params", "head", "g_p", "g_v", "probes", "n_probes", "every", "g_samples", "g_p_out", "g_v_out", "g_head", "g_params",
       "err", "stream")
BWD_REQUIRED = ("ckpt", "params", "head", "g_p", "g_v", "g_p_out", "g_v_out")
JVP = ("p", "v", "count", "params", "head", "t_p", "t_v", "t_head", "t_params", "p_out", "v_out", "t_p_out", "t_v_out", "probes", "n_probes",
       "every", "samples", "t_samples", "err", "err_jvp", "stream")
JVP_REQUIRED = ("p", "v", "params", "head", "t_p", "t_v", "p_out", "v_out", "t_p_out", "t_v_out")
SAMPLE_BUFFERS = {NEW[0]: ("samples",), NEW[1]: ("g_samples",), NEW[2]: ("samples", "t_samples")}


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
    assert lib.dhts_version() == 100
    comment = raw[raw.index("PROBE SAMPLES on the two tape-free paths"):raw.index("int " + NEW[0])]
    for cited in ("dmicro_lane.py:230-269", "_micro_lane.py:131-214", ":87-127", "dmicro_lane.py:271-298", ":130-153", "_idm.py:30-49"):
        assert cited in comment, cited            # what the three siblings cite
    assert "DISTINCT" in comment, "the raw level's rule for the probe list is documented"
    for name in ("micro_rollout_fwd_ckpt_samples", "micro_rollout_bwd_ckpt_samples", "micro_rollout_fwd_jvp_samples", "MicroRolloutSamples"):
        assert callable(getattr(ops, name))
    for fn in (dhts.micro_rollout, dhts.micro_rollout_jvp):
        par = inspect.signature(fn).parameters
        assert par["probes"].default is None and par["every"].default == 1 and type(par["every"].default) is int
    assert list(inspect.signature(ops.MicroRollout.forward).parameters)[-1] == "checkpoint", "the existing operator keeps its signature"


def call_args(names, some, **kw):
    a = {n: some for n in names}
    a.update(stream=None, n_probes=4, every=2)
    a.update(kw)
    return [a[n] for n in names]


def test_bad_arguments_are_rejected_without_a_gpu():
    from dhts import _lib
    lib = _lib.lib()
    V = 70
    ok = _lib.MicroDesc(4, V, 0.01)
    some = C.c_void_p(64)                      # a non-NULL pointer that is never dereferenced: the checks come first
    entries = [(getattr(lib, NEW[0]), FWD, FWD_REQUIRED, 3), (getattr(lib, NEW[1]), BWD, BWD_REQUIRED, 3), (getattr(lib, NEW[2]), JVP, JVP_REQUIRED, 2)]
    for fn, names, required, third in entries:
        buffers = SAMPLE_BUFFERS[fn.__name__]
        for T in (0, 3):
            for missing in required:
                if T == 0 and missing == "ckpt":
                    continue                   # (no checkpoint exists for T = 0, as for the un-sampled pair)
                assert fn(C.byref(ok), T, third, *call_args(names, some, **{missing: None})) == _lib.E_INVALID, (fn.__name__, missing)
            for every in (0, -1, -(1 << 31)):
                assert fn(C.byref(ok), T, third, *call_args(names, some, every=every)) == _lib.E_INVALID
                assert fn(C.byref(ok), T, third, *call_args(names, some, every=every, probes=None)) == _lib.E_INVALID
            for n in (0, -1, V + 1, 1 << 30):  # with a list: 1 .. V
                assert fn(C.byref(ok), T, third, *call_args(names, some, n_probes=n)) == _lib.E_INVALID
        for T, every in ((3, 1), (3, 3), (7, 2)):        # T / every > 0: the sample buffers are required, with and without a list
            for b in buffers:
                assert fn(C.byref(ok), T, third, *call_args(names, some, every=every, **{b: None})) == _lib.E_INVALID
                assert fn(C.byref(ok), T, third, *call_args(names, some, every=every, probes=None, **{b: None})) == _lib.E_INVALID
        assert fn(C.byref(ok), -1, third, *call_args(names, some)) == _lib.E_INVALID
        for bad in (_lib.MicroDesc(4, 5000, 0.01), _lib.MicroDesc(4, 0, 0.01), _lib.MicroDesc(0, V, 0.01), _lib.MicroDesc(4, V, 0.0)):
            assert fn(C.byref(bad), 3, 1, *call_args(names, some)) == _lib.E_INVALID
        assert fn(None, 3, 1, *call_args(names, some)) == _lib.E_INVALID
    # the checkpointed pair: a segment outside 0 .. max_segment, as its siblings
    for fn, names, _, _ in entries[:2]:
        for seg in (-1, 1 << 30):
            assert fn(C.byref(ok), 3, seg, *call_args(names, some)) == _lib.E_INVALID
    assert entries[2][0](C.byref(ok), 3, 0, *call_args(JVP, some)) == _lib.E_INVALID           # n_dir < 1


def test_value_errors_come_before_any_device_use():
    """CPU tensors, no device in sight: every bad `probes`, `every` or combination with want_hist is a ValueError of both public functions
    (not the TypeError / RuntimeError a launch on CPU tensors would be), on the taped and on the tape-free paths alike."""
    import torch
    import dhts
    L, V, T = 2, 8, 5
    p0, v0 = torch.zeros(L, V), torch.zeros(L, V)
    par, head = torch.ones(6, L, V, dtype=torch.float64), torch.zeros(L, 2, dtype=torch.float64)
    t_p0 = torch.zeros(1, L, V)
    bad_probes = ([3, 1], [1, 1], [], [-1, 2], [0, V], [1.5], [True], (2.0, 3.5), torch.tensor([2, 1]), torch.tensor([], dtype=torch.int64),
                  torch.tensor([0.0, 1.0]), torch.tensor([[1, 2]]), torch.tensor([V]), torch.tensor([True, False]))
    bad_every = (0, -1, 1.5, True, False, "2", None, 2.0)
    for path in (dict(), dict(checkpoint=True), dict(checkpoint=2)):
        for probes in bad_probes:
            with pytest.raises(ValueError):
                dhts.micro_rollout(p0, v0, par, head, T, 0.01, probes=probes, **path)
        for every in bad_every:
            with pytest.raises(ValueError):
                dhts.micro_rollout(p0, v0, par, head, T, 0.01, every=every, **path)
            with pytest.raises(ValueError):
                dhts.micro_rollout(p0, v0, par, head, T, 0.01, probes=[1], every=every, **path)
        for kw in (dict(probes=[1, 2]), dict(every=2), dict(probes=[0], every=3)):
            with pytest.raises(ValueError, match="the history holds every vehicle and step"):
                dhts.micro_rollout(p0, v0, par, head, T, 0.01, want_hist=True, **kw, **path)
    # a bad checkpoint with good probes: still the ValueError of the checkpoint, nothing uploaded
    for bad in (0, -1, 2.5, "3"):
        with pytest.raises(ValueError):
            dhts.micro_rollout(p0, v0, par, head, T, 0.01, probes=[1], checkpoint=bad)
    for fused in (False, True):
        for probes in bad_probes:
            with pytest.raises(ValueError):
                dhts.micro_rollout_jvp(p0, v0, par, head, T, 0.01, t_p0=t_p0, probes=probes, fused=fused)
        for every in bad_every:
            with pytest.raises(ValueError):
                dhts.micro_rollout_jvp(p0, v0, par, head, T, 0.01, t_p0=t_p0, every=every, fused=fused)
        for kw in (dict(probes=[1, 2]), dict(every=2)):
            with pytest.raises(ValueError, match="the history holds every vehicle and step"):
                dhts.micro_rollout_jvp(p0, v0, par, head, T, 0.01, t_p0=t_p0, want_hist=True, fused=fused, **kw)


def test_the_raw_wrappers_check_probes_every_and_the_buffers():
    import torch
    from dhts import ops
    L, V, T = 2, 8, 5
    desc = ops.micro_desc(L, V, 0.01)
    z = torch.zeros(L, V)
    par, head = torch.ones(6, L, V, dtype=torch.float64), torch.zeros(L, 2, dtype=torch.float64)
    ck = torch.zeros(ops.micro_ckpt_numel(desc, T, 2))
    for every in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            ops.micro_rollout_fwd_ckpt_samples(desc, T, z, z, par, head, ck, None, every, segment=2)
        with pytest.raises(ValueError):
            ops.micro_rollout_bwd_ckpt_samples(desc, T, ck, par, head, z, z, None, every, torch.zeros(T, L, 2, V), segment=2)
        with pytest.raises(ValueError):
            ops.micro_rollout_fwd_jvp_samples(desc, T, z, z, par, head, z[None], z[None], None, every)
    for probes in ([1, 2], torch.tensor([1, 2]), torch.tensor([1, 2], dtype=torch.int32)):      # the raw level takes a CUDA int32 tensor only
        with pytest.raises(ValueError):
            ops.micro_rollout_fwd_ckpt_samples(desc, T, z, z, par, head, ck, probes, 1, segment=2)
        with pytest.raises(ValueError):
            ops.micro_rollout_bwd_ckpt_samples(desc, T, ck, par, head, z, z, probes, 1, torch.zeros(T, L, 2, 2), segment=2)
        with pytest.raises(ValueError):
            ops.micro_rollout_fwd_jvp_samples(desc, T, z, z, par, head, z[None], z[None], probes, 1)
    with pytest.raises(ValueError):
        ops.micro_rollout_fwd_ckpt_samples(desc, T, z, z, par, head, torch.zeros(3), None, 1, segment=2)
    with pytest.raises(ValueError):
        ops.micro_rollout_bwd_ckpt_samples(desc, T, ck, par, head, z, z, None, 2, None, segment=2)
    # the slots of a public call, as lists, and when sampling is off
    assert ops.micro_sampling(None, 1, V, False) is None and ops.micro_sampling(None, 1, V, True) is None
    assert ops.micro_sampling(None, 3, V, False) == (None, 3)
    assert ops.micro_sampling([0, 7], 1, V, False) == ([0, 7], 1)
    assert ops.micro_sampling(torch.tensor([2, 5]), 4, V, False) == ([2, 5], 4)


def test_cut_samples_is_the_documented_slice():
    """The taped paths' glue on a CPU tensor: rows every - 1, 2 every - 1, ...; the probes' columns; zeros at or beyond count; T // every
    rows for every T."""
    import torch
    from dhts import ops
    L, V = 3, 5
    count = torch.tensor([5, 0, 2], dtype=torch.int32)
    for T in (0, 1, 6, 7):
        hist = torch.arange(T * L * 2 * V, dtype=torch.float32).reshape(T, L, 2, V) + 1
        for every in (1, 2, 3, 7, 8):
            for slots in (None, [0], [1, 4]):
                cut = ops.cut_samples(hist, slots, every, count)
                cols = list(range(V)) if slots is None else slots
                assert tuple(cut.shape) == (T // every, L, 2, len(cols))
                for j in range(T // every):
                    for lane in range(L):
                        for i, c in enumerate(cols):
                            want = hist[(j + 1) * every - 1, lane, :, c] if c < int(count[lane]) else torch.zeros(2)
                            assert torch.equal(cut[j, lane, :, i], want)
