"""The hand-built networks of tests/net_cases.py through every device form that accepts a macro-only network -- the fused macro pair
(ops.net_macro_rollout / net_macro_eval), the fused hybrid pair on the all-macro hybrid tables, StepwiseNetwork stepwise and persistent,
BatchedMacroNetwork -- against ONE reference, oracle.net_macro.  Per case and form, three replicas (the `plain`, `edges` and `mixed`
actions) in one launch where the form has replicas, else one launch each:

* the launch plan is the one the case names (fused macro pair: ops.net_macro_plan; hybrid: the block of ops.net_hybrid_plan against
  Case.hybrid_plan, which records what these shapes reach there);
* queues <= TOL_STATE norm-relative and <= 10 TOL_STATE element-wise, reward <= 1e-5, the whole gradient <= TOL_GRAD of its largest
  entry, and every well-conditioned phase row (net_cases.reference: the oracle's own gradient moves by at most 0.1 TOL_GRAD of the row
  under one ulp of the action) <= TOL_GRAD of the ROW's largest entry -- a lost contribution to a late phase or a quiet intersection
  shows there; the rows left out as ill conditioned are printed;
* every structural zero of the oracle's gradient is an exact zero on the device;
* evaluation episodes (hard thresholds; under `edges` with steps where a == progress and neither light is on): queues and reward;
* two launches give the same bits, and a replica of the three-replica launch gives the bits of its single-replica launch;
* the fault records come back clean.

The NETCASE lines (pytest -s) are the second section of profiles/net_layout_cases.log.
"""
import numpy as np
import pytest

import net_cases as nc
from util import TOL_GRAD, TOL_STATE, grad_report, rel_elem, state_report

pytestmark = pytest.mark.gpu

FORMS = ["macro", "hybrid", "stepwise", "persistent", "batched"]
KINDS = ["plain", "edges", "mixed"]


class Runner:
    """One case on one device form.  run(acts [R][A], train) -> dict(queue [R][T][L], reward [R] float32, grad [R][A] or None); the
    forms without replicas (stepwise, batched) take the replicas one launch after the other."""

    def __init__(self, form, c, cuda):
        from dhts import ops
        self.form, self.c, self.cuda, self.ops = form, c, cuda, ops
        self.nets = {}
        if form == "macro":
            self.tab = ops.DeviceNetTables(c.tab, cuda)
        elif form == "hybrid":
            self.tab = ops.DeviceHybridTables(c.htab, c.routes, cuda)
        elif form == "stepwise":
            from dhts.stepwise import StepwiseNetwork
            self.net = StepwiseNetwork(c.htab, c.routes, cuda)
        elif form == "batched":
            from dhts.batched import BatchedMacroNetwork
            self.net = BatchedMacroNetwork(c.tab, cuda)

    def _persistent(self, R):
        from dhts.stepwise import StepwiseNetwork
        if R not in self.nets:
            self.nets[R] = StepwiseNetwork([self.c.htab] * R, self.c.routes, self.cuda, persistent=True)
        return self.nets[R]

    def run(self, acts, train):
        import torch
        ops, c, form = self.ops, self.c, self.form
        acts = np.ascontiguousarray(acts, dtype=np.float32)
        R = acts.shape[0]
        if form in ("macro", "hybrid", "persistent"):
            a = torch.tensor(acts, device=self.cuda, requires_grad=train)
            err = ops.new_error_record(self.cuda)
            if form == "macro":
                reward, queue = (ops.net_macro_rollout if train else ops.net_macro_eval)(a, self.tab, *c.args, err=err)
                cut = reward
            elif form == "hybrid":
                if train:
                    cut, reward, queue, _ = ops.net_hybrid_rollout(a, self.tab, *c.args, err=err)
                else:
                    reward, queue, _ = ops.net_hybrid_eval(a, self.tab, *c.args, err=err)
            else:
                net = self._persistent(R)
                cut, reward, queue, _ = net.rollout(a, *c.args, differentiable=train)
                err = net.err
            if train:
                cut.sum().backward()
            assert err.tolist() == [0, 0, 0, 0], "%s %s: fault record %s" % (c.name, form, err.tolist())
            return dict(queue=queue.detach().cpu().numpy(), reward=reward.detach().cpu().numpy(), grad=a.grad.cpu().numpy() if train else None)
        out = dict(queue=[], reward=[], grad=[])
        for r in range(R):
            a = torch.tensor(acts[r], device=self.cuda, requires_grad=train)
            if form == "stepwise":
                cut, reward, queue, _ = self.net.rollout(a, *c.args, differentiable=train)
            else:
                with torch.set_grad_enabled(train):
                    reward, queue = self.net.rollout(a, *c.args, differentiable=train)
                cut = reward
            if train:
                cut.backward()
            assert self.net.err.tolist() == [0, 0, 0, 0], "%s %s: fault record %s" % (c.name, form, self.net.err.tolist())
            out["queue"].append(queue.detach().cpu().numpy())
            out["reward"].append(np.float32(reward.detach().cpu().numpy()))
            out["grad"].append(a.grad.cpu().numpy() if train else None)
        return dict(queue=np.stack(out["queue"]), reward=np.array(out["reward"], dtype=np.float32), grad=np.stack(out["grad"]) if train else None)


def same_bits(x, y):
    return all((x[k] is None and y[k] is None) or np.array_equal(x[k], y[k]) for k in ("queue", "reward", "grad"))


def acts_of(c):
    return np.stack([c.actions[k] for k in KINDS])


def check_plan(form, c, runner):
    from dhts import ops
    if form == "macro":
        assert ops.net_macro_plan(c.A, runner.tab, c.sq, c.F, nc.DT, nc.U_MAX) == c.plan
        lay = c.layout()
        for side, want in c.want.items():
            for k, v in want.items():
                assert lay[side][k] == v
    if form == "hybrid":
        plan = ops.net_hybrid_plan(3, c.A, runner.tab, c.sq, c.F, nc.DT, nc.U_MAX)
        assert plan["block"] == c.hybrid_plan()["block"] and not plan["packed"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", nc.NAMES)
def test_case_on_device_form_vs_oracle(cuda, oracle, name, form):
    c = nc.case(name)
    ref = nc.reference(name, oracle)
    runner = Runner(form, c, cuda)
    check_plan(form, c, runner)
    acts = acts_of(c)
    tr, ev = runner.run(acts, True), runner.run(acts, False)
    zeros = c.structural_zeros()
    sq, rows = c.sq, c.rows()
    for r, kind in enumerate(KINDS):
        tag = "%s / %s / %s" % (name, form, kind)
        o, oe, rf = ref[kind]["train"], ref[kind]["hard"], ref[kind]
        e_q = state_report("%s: queues" % tag, tr["queue"][r], o["queue"])
        e_qe = rel_elem(tr["queue"][r], o["queue"])
        e_r = abs(float(tr["reward"][r]) - o["reward"]) / max(abs(o["reward"]), 1e-300)
        e_g = grad_report("%s: d reward / d action" % tag, tr["grad"][r], o["g_action"])
        d = np.abs(tr["grad"][r].astype(np.float64) - o["g_action"].astype(np.float64))[:rows * sq].reshape(rows, sq).max(axis=1)
        e_row = d / np.maximum(rf["row_max"], 1e-300)
        well, nz = rf["well"], rf["row_max"] > 0
        skipped = [int(i) for i in np.nonzero(nz & ~well)[0]]
        worst = float(e_row[well].max()) if well.any() else 0.0
        e_ev = state_report("%s: evaluation queues" % tag, ev["queue"][r], oe["queue"])
        e_eve = rel_elem(ev["queue"][r], oe["queue"])
        e_evr = abs(float(ev["reward"][r]) - oe["reward"]) / max(abs(oe["reward"]), 1e-300)
        print("NETCASE %s: queue %.2e (element-wise %.2e) reward %.2e gradient %.2e worst well-conditioned row %.2e (%d rows, ill-conditioned rows "
              "left out: %s) | evaluation queue %.2e (element-wise %.2e) reward %.2e, steps with neither light %d"
              % (tag, e_q, e_qe, e_r, e_g, worst, int(well.sum()), skipped or "none", e_ev, e_eve, e_evr, c.neither_light_steps(acts[r])))
        assert e_q <= TOL_STATE and e_qe <= 10 * TOL_STATE, tag
        assert e_r <= 1e-5, tag
        assert e_g <= TOL_GRAD, tag
        assert (e_row[well] <= TOL_GRAD).all(), "%s: rows %s" % (tag, np.nonzero(well & (e_row > TOL_GRAD))[0])
        if kind == "plain":
            assert len(skipped) <= 0.1 * nz.sum()
        assert (tr["grad"][r][zeros] == 0.0).all(), tag
        assert e_ev <= TOL_STATE and e_eve <= 10 * TOL_STATE, tag
        assert e_evr <= 1e-5, tag
    # two launches give the same bits; a replica of the three-replica launch gives the bits of its single-replica launch
    assert same_bits(tr, runner.run(acts, True)) and same_bits(ev, runner.run(acts, False))
    if form in ("macro", "hybrid", "persistent"):
        for r in range(len(KINDS)):
            one, one_e = runner.run(acts[r:r + 1], True), runner.run(acts[r:r + 1], False)
            for k in ("queue", "reward", "grad"):
                assert np.array_equal(one[k][0], tr[k][r]), (name, form, KINDS[r], k)
            assert np.array_equal(one_e["queue"][0], ev["queue"][r]) and np.array_equal(one_e["reward"][0], ev["reward"][r])


@pytest.mark.parametrize("form", FORMS)
def test_trailing_unused_actions_change_only_the_block_size(cuda, form):
    """action_wide (65 phase rows, 6 used: the fused macro pair's block is sized by the action count) and action_wide_trim (the 6 rows):
    bit-identical queues, reward and shared gradient entries, zeros in the rest -- training and evaluation episodes."""
    w, t = nc.case("action_wide"), nc.case("action_wide_trim")
    assert np.array_equal(acts_of(w)[:, :t.A], acts_of(t))
    rw, rt = Runner(form, w, cuda), Runner(form, t, cuda)
    a, b = rw.run(acts_of(w), True), rt.run(acts_of(t), True)
    assert np.array_equal(a["queue"], b["queue"]) and np.array_equal(a["reward"], b["reward"])
    assert np.array_equal(a["grad"][:, :t.A], b["grad"]) and (a["grad"][:, t.A:] == 0.0).all()
    a, b = rw.run(acts_of(w), False), rt.run(acts_of(t), False)
    assert np.array_equal(a["queue"], b["queue"]) and np.array_equal(a["reward"], b["reward"])
