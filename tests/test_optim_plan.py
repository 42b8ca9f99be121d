"""The fused optimizers' launch plans (rbm_amd.optim), on the CPU: FusedAdam / FusedSGD driven over a stand-in flat
buffer with the optimizer entries of rbm_amd.ops replaced by recorders (tests/optim_plan.py) must issue exactly the
launches stored in tests/golden/optim_plans.json -- entry, range, zero_grad / prepare / tbase / max_wg, the optional
pointers passed, marks -- which the revision before the optimizers moved into their own module produced.  And the
range planner on its own."""
import json
import os

import pytest

import optim_plan
from conftest import GOLDEN


def _golden():
    with open(os.path.join(GOLDEN, "optim_plans.json")) as fh:
        return json.load(fh)


def test_the_stored_plans_cover_every_case():
    assert list(_golden()) == list(optim_plan.CASES)


@pytest.mark.parametrize("name", list(optim_plan.CASES))
def test_launch_plan_equals_the_stored_one(name):
    got, want = optim_plan.run_case(name), _golden()[name]
    for i, (g, e) in enumerate(zip(got, want)):
        assert g == e, f"launch {i}: {g} != {e}"
    assert len(got) == len(want), f"{len(got)} launches, stored {len(want)}"


def test_planner_alone():
    from rbm_amd.optim import plan
    from rbm_amd.train_step import FusedAdam
    n, lst, cnt = optim_plan.NUMEL, None, None
    tables = [(64, 10, 5, lst, cnt), (1024, 3, 1, lst, cnt)]
    # today's FusedAdam._sparse_segments values (tests/test_adam_rows_ref.py), from the planner and through the name
    assert plan(n, sparse=tables) == [(0, 64, True), (128, 1024, True), (1088, 4096, True)]
    assert plan(n, sparse=[(0, 4096, 1, lst, cnt)]) == []
    opt = FusedAdam(optim_plan.flat())
    assert opt._sparse_segments(tables) == plan(n, sparse=tables)
    assert plan(n) == [(0, n, True)]
    assert plan(n, keep=(1024, 2048)) == [(0, 1024, True), (1024, 2048, False), (2048, n, True)]
    assert plan(n, keep=(1024, n)) == [(0, 1024, True), (1024, n, False)]
    # keep is ignored when ranges is given: the ranges are swept as they are, every gradient cleared
    rg = [(0, 512), (1024, n)]
    assert plan(n, ranges=rg, keep=(1024, 2048)) == plan(n, ranges=rg) == [(0, 512, True), (1024, n, True)]
    with pytest.raises(AssertionError):
        plan(n, keep=(1022, 2048))                       # keep must be 16-byte aligned
    for kw in (dict(ranges=rg), dict(keep=(64, 128))):
        with pytest.raises(ValueError, match="neither ranges nor keep"):
            plan(n, sparse=tables, **kw)
    with pytest.raises(ValueError, match="weight_decay"):
        plan(n, sparse=tables, weight_decay=0.01)
    with pytest.raises(ValueError, match="not a parameter"):
        plan(n, sparse=[(32, 10, 4, lst, cnt)])
    with pytest.raises(ValueError, match="overlap"):
        plan(n, sparse=[(0, 100, 4, lst, cnt), (64, 10, 4, lst, cnt)])


def test_complement():
    from rbm_amd.optim import complement
    assert complement([], 100) == [(0, 100)]
    assert complement([(40, 60), (0, 10)], 100) == [(10, 40), (60, 100)]
    assert complement([(0, 50), (50, 100)], 100) == []
    with pytest.raises(ValueError, match="overlap"):
        complement([(0, 50), (40, 60)], 100)
    with pytest.raises(ValueError, match="overlap"):
        complement([(10, 120)], 100)                     # past the end of the buffer


def test_sgd_refuses_sparse_tables_first():
    from rbm_amd.train_step import FusedSGD
    with pytest.raises(ValueError, match="lazy rule is Adam's"):
        FusedSGD(optim_plan.flat(), lr=0.1).step(sparse=[(0, 10, 4, None, None)], keep=(64, 128))


def test_checkpoint_surface():
    """What the trainer's delegations rely on: both optimizers expose state_dict / load_state_dict /
    moment_buffers, and the old names resolve to the moved classes."""
    import rbm_amd.optim as optim
    import rbm_amd.train_step as ts
    assert (ts.FusedAdam, ts.FusedSGD, ts.FusedStepLR) == (optim.FusedAdam, optim.FusedSGD, optim.FusedStepLR)
    assert ts.FusedTrainStep.SGD_STEP_KEY == optim.FusedSGD.SGD_STEP_KEY == "fused_step"
    f = optim_plan.flat()
    adam, sgd0, sgd = optim.FusedAdam(f), optim.FusedSGD(f, lr=0.1), optim.FusedSGD(f, lr=0.1, momentum=0.9)
    assert [b is x for b, x in zip(adam.moment_buffers(), (adam.m, adam.v))] == [True, True]
    assert sgd0.moment_buffers() == [] and sgd.moment_buffers()[0] is sgd.buf and len(sgd.moment_buffers()) == 1


# ------------------------------------------------------------------ the checkpoint formats, on the host
def _params(f):
    """Two parameters that are views of the stand-in buffer, as a model's are of FlatParams: [(parameter, offset)]."""
    import torch
    return [(torch.nn.Parameter(f.data[off:off + n].view(shape)), off) for off, n, shape in ((0, 12, (3, 4)),
                                                                                           (64, 5, (5,)))]


def test_adam_state_dict_is_torchs_and_round_trips():
    import torch
    from rbm_amd.optim import FusedAdam, FusedSGD
    f = optim_plan.flat()
    slices = _params(f)
    params = [p for p, _ in slices]
    opt = FusedAdam(f, lr=3e-3, weight_decay=0.01)
    assert opt.state_dict(params, slices)["state"] == {}              # no step yet: torch's empty state
    torch.manual_seed(0)
    opt.m.normal_(), opt.v.uniform_()
    opt.state[0] = 3
    sd = opt.state_dict(params, slices)
    assert list(sd["state"][0]) == ["step", "exp_avg", "exp_avg_sq"] and float(sd["state"][1]["step"]) == 3.0
    assert torch.equal(sd["state"][0]["exp_avg"], opt.m[0:12].view(3, 4))
    assert torch.equal(sd["state"][1]["exp_avg_sq"], opt.v[64:69])
    g = sd["param_groups"][0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"]) == (3e-3, (0.9, 0.999), 1e-8, 0.01)
    torch.optim.Adam(params).load_state_dict(sd)                      # torch takes it
    new = FusedAdam(optim_plan.flat())
    new.load_state_dict(sd, slices)
    assert torch.equal(new.hyper, opt.hyper) and new.weight_decay == 0.01 and float(new.state[0]) == 3.0
    for a, b in zip(new.moment_buffers(), opt.moment_buffers()):
        assert torch.equal(a[0:12], b[0:12]) and torch.equal(a[64:69], b[64:69])
        assert not a[12:64].any() and not a[69:].any()                # what no parameter covers is zero
    sd["state"][1]["step"] = torch.tensor(4.0)
    with pytest.raises(ValueError, match="step counts differ"):
        new.load_state_dict(sd, slices)
    with pytest.raises(ValueError, match="optimizer='sgd' cannot load"):
        FusedSGD(optim_plan.flat(), lr=0.1).load_state_dict(sd, slices)


def test_sgd_state_dict_is_torchs_and_round_trips():
    import torch
    from rbm_amd.optim import FusedAdam, FusedSGD
    f = optim_plan.flat()
    slices = _params(f)
    params = [p for p, _ in slices]
    opt = FusedSGD(f, lr=0.05, momentum=0.9, weight_decay=0.01)
    torch.manual_seed(0)
    opt.buf.normal_()
    opt.state[0] = 2
    sd = opt.state_dict(params, slices)
    g = sd["param_groups"][0]
    assert (g["lr"], g["momentum"], g["weight_decay"], g[FusedSGD.SGD_STEP_KEY]) == (0.05, 0.9, 0.01, 2.0)
    assert list(sd["state"][0]) == ["momentum_buffer"]
    assert torch.equal(sd["state"][1]["momentum_buffer"], opt.buf[64:69])
    torch.optim.SGD(params, lr=0.1).load_state_dict(sd)
    plain = FusedSGD(optim_plan.flat(), lr=0.1)                       # built without momentum: no buffer
    with pytest.raises(ValueError, match="captured step graphs were built with momentum=0.0"):
        plain.load_state_dict(sd, slices, captured=True)
    assert plain.buf is None
    plain.load_state_dict(sd, slices)
    assert plain.momentum == 0.9 and torch.equal(plain.hyper, opt.hyper) and float(plain.state[0]) == 2.0
    assert torch.equal(plain.buf[0:12], opt.buf[0:12]) and torch.equal(plain.buf[64:69], opt.buf[64:69])
    assert not plain.buf[12:64].any()
    # a checkpoint torch wrote has no count: 1 when it holds buffers, and momentum 0 drops the buffer
    del g[FusedSGD.SGD_STEP_KEY]
    plain.load_state_dict(sd, slices)
    assert float(plain.state[0]) == 1.0
    g["momentum"], sd["state"] = 0.0, {}
    plain.load_state_dict(sd, slices)
    assert plain.buf is None and plain.moment_buffers() == [] and float(plain.state[0]) == 0.0
    assert plain.state_dict(params, slices)["state"] == {}
    for key, bad in (("dampening", 0.1), ("nesterov", True), ("momentum", -1.0)):
        with pytest.raises(ValueError, match=key):
            plain.load_state_dict({"state": {}, "param_groups": [dict(g, **{key: bad})]}, slices)
    with pytest.raises(ValueError, match="no 'betas'"):
        FusedAdam(optim_plan.flat()).load_state_dict(sd, slices)
