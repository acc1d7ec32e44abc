"""The exact-arithmetic adjudicator (tests/hp_ref.py) against the reference's known answers and the C oracle.  Runs without a GPU.

Every row of the reference's own tables must get the reference's case, and every double and float32 value the reference computed
must lie within hp_ref's bound; on seeded sweeps of every edge class of tests/sweep_inputs.py the oracle must agree the same way.
This is what lets tests/test_device_math_sweep_gpu.py excuse a kernel's difference as a tie."""
import os

import numpy as np

import hp_ref as H
import sweep_inputs as S


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def _check_arz(t, o, label):
    settled = ~t["tie"]
    assert np.array_equal(o["case"][settled], t["case"][settled]), label
    for k in ("q0", "speed"):
        if k not in o:
            continue
        ok, ratio = H.within64(o[k], t, k)
        assert ok.all(), (label, k, np.argwhere(~ok)[:5])
    for k in ("dL", "dR", "fp"):
        ok = H.within32(o[k], t, k)
        assert ok.all(), (label, k, np.argwhere(~ok)[:5])


def test_hp_ref_reproduces_the_interface_known_answers(golden_dir):
    for name in ("riemann_kat.npz", "riemann_kat_stale.npz"):
        g = load(golden_dir, name)
        t = H.arz_table(g["inp"])
        assert not t["tie"].any(), name                  # the reference's rows are far from every threshold
        assert np.array_equal(t["case"], g["case"]), name
        _check_arz(t, {k: g[k] for k in ("case", "q0", "speed", "dL", "dR", "fp") if k in g.files}, name)


def test_hp_ref_reproduces_the_idm_known_answers(golden_dir):
    for name in ("idm_kat.npz", "idm_kat_smallgap.npz"):
        g = load(golden_dir, name)
        t = H.idm_table(g["inp"])
        assert not (t["tie_acc"] | t["tie_spacing"]).any(), name
        assert np.array_equal(t["clipped_acc"], g["flags"][:, 0].astype(bool)), name
        assert np.array_equal(t["clipped_spacing"], g["flags"][:, 1].astype(bool)), name
        for k in ("acc", "sstar"):
            ok, _ = H.within64(g[k], t, k)
            assert ok.all(), (name, k)
        for k in ("dEgo", "dLeading"):
            assert H.within32(g[k], t, k).all(), (name, k)


def test_hp_ref_agrees_with_the_oracle_on_every_edge_class(oracle):
    """About 20 000 interfaces and 12 000 vehicle steps over every edge class of the sweep, against the C oracle's batch entries."""
    ties = {}
    for name, inp, dt, dx in S.arz_classes(1500, seed=11):
        o = oracle.arz_batch(inp, dt, dx)
        t = H.arz_table(inp, dt, dx)
        _check_arz(t, o, name)
        # the CFL assert: the oracle may only differ from the exact decision inside the bound
        settled = np.abs(t["cfl_m"]) > t["cfl_e"]
        assert np.array_equal(o["cfl_bad"][settled], (t["cfl_m"] <= 0)[settled]), name
        ties[name] = int(t["tie"].sum())
    for name, inp in S.idm_classes(1000, seed=11):
        o = oracle.idm_batch(inp)
        t = H.idm_table(inp)
        for k, tk in (("clipped_acc", "tie_acc"), ("clipped_spacing", "tie_spacing")):
            assert np.array_equal(o[k][~t[tk]], t[k][~t[tk]]), (name, k)
        agree = (o["clipped_acc"] == t["clipped_acc"]) & (o["clipped_spacing"] == t["clipped_spacing"])
        assert np.array_equal(o["collided"], t["collided"])
        for k in ("acc", "sstar"):
            ok, _ = H.within64(o[k], t, k)
            assert ok[agree].all(), (name, k)
        assert H.within32(o["next_v"], t, "next_v")[agree].all(), name
        fin = t["finite"] & agree
        for k in ("dEgo", "dLeading"):
            assert H.within32(o[k][fin], {kk: v[fin] for kk, v in t.items()}, k).all(), (name, k)
        # under the acceleration clip the reference's v + dt * (-v / dt) is exactly 0 (and its exact value is 0)
        clip = o["clipped_acc"] & ~t["tie_acc"]
        assert np.all(o["next_v"][clip] == 0.0), name
        ties[name] = int((t["tie_acc"] | t["tie_spacing"]).sum())
    print("rows whose case or clip decision is a tie:", ties)
