"""CPU checks of the fused SGD's reference (tests/sgd_ref.py) against torch.optim.SGD, of the planted mistakes, of
FusedTrainStep's refusals around optimizer= / momentum=, and of rs_sgd_step's argument validation (no launch)."""
import argparse
import math

import numpy as np
import pytest
import torch

import sgd_ref as R

N, STEPS = 100_003, 20
LR = 0.05
CASES = [(0.9, 0.0), (0.9, 0.01), (0.0, 0.01), (0.0, 0.0)]


def torch_sgd(p0, grads, lr, momentum, wd, dtype, foreach=None, lrs=None):
    """torch.optim.SGD on CPU tensors of `dtype`: (p, momentum buffer or None) after the steps."""
    p = torch.tensor(np.asarray(p0), dtype=dtype, requires_grad=True)
    opt = torch.optim.SGD([p], lr=lr, momentum=momentum, weight_decay=wd, foreach=foreach)
    for k, g in enumerate(grads):
        if lrs is not None:
            opt.param_groups[0]["lr"] = lrs[k]
        opt.zero_grad()
        p.grad = torch.tensor(np.asarray(g), dtype=dtype)
        opt.step()
    buf = opt.state[p].get("momentum_buffer") if momentum else None
    return p.detach().numpy(), None if buf is None else buf.numpy()


@pytest.fixture(scope="module")
def data():
    return R.scenario(3, N, STEPS)


@pytest.mark.parametrize("momentum,wd", CASES)
def test_float64_form_is_torch_sgd(data, momentum, wd):
    p0, grads = data
    p0, grads = p0[:4099], [g[:4099] for g in grads[:5]]
    run = R.Run(p0, momentum != 0, np.float64)
    s = R.scalars(LR, momentum, wd, cast=False)
    for g in grads:
        run.step(g, s)
    p, buf = torch_sgd(p0, grads, LR, momentum, wd, torch.float64)
    assert np.abs(run.p - p).max() <= 1e-14 * np.abs(p).max()
    if momentum:
        assert np.abs(run.buf - buf).max() <= 1e-14 * np.abs(buf).max()
    else:
        assert run.buf is None and buf is None


def emulate(p0, grads, momentum, wd, mistake=None, lrs=None, divisor=None):
    run = R.Run(p0, momentum != 0, np.float32)
    for k, g in enumerate(grads):
        run.step(g, R.scalars(lrs[k] if lrs else LR, momentum, wd, divisor), mistake=mistake)
    return run


@pytest.fixture(scope="module")
def torch32(data):
    """torch's CPU float32 SGD on the 100,003-element scenario, once per case (read-only afterwards)."""
    p0, grads = data
    return {c: torch_sgd(p0, grads, LR, c[0], c[1], torch.float32) for c in CASES}


@pytest.mark.parametrize("momentum,wd", CASES)
def test_float32_emulation_equals_torch_on_every_element(data, torch32, momentum, wd):
    """20 steps, the first-step rule included (the buffer starts absent in torch, zero in the emulation)."""
    p0, grads = data
    run = emulate(p0, grads, momentum, wd)
    p, buf = torch32[(momentum, wd)]
    assert R.check_run(run, p, buf) == []
    # after ONE step too: buf = grad.clone() in torch
    one = emulate(p0, grads[:1], momentum, wd)
    p1, b1 = torch_sgd(p0, grads[:1], LR, momentum, wd, torch.float32)
    assert R.check_run(one, p1, b1) == []


def test_float32_emulation_equals_torch_single_tensor_path_and_changing_rate(data):
    p0, grads = data
    p0, grads = p0[:20_011], [g[:20_011] for g in grads]
    lrs = [LR * 0.5 ** (k // 3) for k in range(len(grads))]
    run = emulate(p0, grads, 0.9, 0.01, lrs=lrs)
    for foreach in (False, True):
        p, buf = torch_sgd(p0, grads, LR, 0.9, 0.01, torch.float32, foreach=foreach, lrs=lrs)
        assert R.check_run(run, p, buf) == []


@pytest.mark.parametrize("momentum,wd", CASES)
def test_emulation_with_a_gradient_scale_stays_inside_the_derived_bound(data, momentum, wd):
    """gs = 1 / 3 (data parallel): no torch yardstick in float32, so float64 with the same float-cast scalars and
    the per-step bound of sgd_ref's docstring."""
    p0, grads = data
    p0, grads = p0[:20_011], [g[:20_011] for g in grads]
    s = R.scalars(LR, momentum, wd, divisor=3.0)
    assert s["gs"] != 1.0
    ref, emu = R.Run(p0, momentum != 0, np.float64), R.Run(p0, momentum != 0, np.float32)
    bound = R.Bound(p0.size, momentum != 0)
    for g in grads:
        bound.step(ref, g, s)
        ref.step(g, s)
        emu.step(g, s)
        assert np.all(np.abs(emu.p.astype(np.float64) - ref.p) <= bound.eP)
        if momentum:
            assert np.all(np.abs(emu.buf.astype(np.float64) - ref.buf) <= bound.eB)
    # the bound is tight enough to mean something: a few float32 ulps of the largest parameter per step
    assert bound.eP.max() <= 4 * len(grads) * R.U32 * max(1.0, np.abs(ref.p).max())
    # and an emulation that drops the scale is far outside it
    wrong = R.Run(p0, momentum != 0, np.float32)
    wrong.step(grads[0], R.scalars(LR, momentum, wd))
    b1 = R.Bound(p0.size, momentum != 0)
    r1 = R.Run(p0, momentum != 0, np.float64)
    b1.step(r1, grads[0], s)
    r1.step(grads[0], s)
    assert not np.all(np.abs(wrong.p.astype(np.float64) - r1.p) <= b1.eP)


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_planted_mistakes_fail_the_check(data, torch32, mistake):
    p0, grads = data
    lrs = None
    if mistake == "lr_in_buf":      # with a constant rate only the buffer shows it; a changing one moves p too
        lrs = [LR * 0.5 ** (k // 3) for k in range(len(grads))]
        want = torch_sgd(p0, grads, LR, 0.9, 0.01, torch.float32, lrs=lrs)
    else:
        want = torch32[(0.9, 0.01)]
    assert R.check_run(emulate(p0, grads, 0.9, 0.01, lrs=lrs), *want) == []
    bad = R.check_run(emulate(p0, grads, 0.9, 0.01, mistake=mistake, lrs=lrs), *want)
    assert bad, mistake
    expect = {"no_clear": "gradient not cleared", "stale_bf16": "bf16 copy"}.get(mistake, "differs")
    assert any(expect in b for b in bad), (mistake, bad)
    assert R.MISTAKES == ("buf_fma", "decay_after", "lr_in_buf", "first_dampened", "no_clear", "stale_bf16")


# ================================================================ the refusals
def _sas_model(**kw):
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    return model_factory(argparse.Namespace(model_code="sas", num_items=30, max_len=8, device="cpu",
                                            sas_hidden_units=16, sas_num_blocks=1, sas_heads=2, sas_dropout=0.0,
                                            model_init_seed=0, **kw))


def _bert_model(**kw):
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    return model_factory(argparse.Namespace(model_code="bert", num_items=30, max_len=8, device="cpu",
                                            bert_hidden_units=16, bert_num_blocks=1, bert_num_heads=2,
                                            bert_dropout=0.0, bert_hidden_dropout=0.0, bert_mask_prob=0.2,
                                            model_init_seed=0, **kw))


def test_every_refusal_is_raised_before_the_device_is_touched():
    from rbm_amd.train_step import FusedTrainStep
    sas, bert = _sas_model(), _bert_model()
    with pytest.raises(ValueError, match="table_optim"):
        FusedTrainStep(sas, optimizer="sgd", momentum=0.9, table_optim="sparse")
    with pytest.raises(ValueError, match="shard_rows"):
        FusedTrainStep(sas, optimizer="SGD", momentum=0.9, shard_rows="on")
    with pytest.raises(ValueError, match="vocab_shard"):
        FusedTrainStep(bert, optimizer="sgd", momentum=0.9, vocab_shard=True)
    for m in (None, -0.1, math.nan, math.inf):
        with pytest.raises(ValueError, match="momentum"):
            FusedTrainStep(sas, optimizer="sgd", momentum=m)
    with pytest.raises(ValueError, match=r"momentum=None.*torch\.optim\.SGD raise"):
        FusedTrainStep(sas, optimizer="sgd", momentum=None)
    with pytest.raises(ValueError, match="momentum"):
        FusedTrainStep(sas, optimizer="adam", momentum=0.9)
    with pytest.raises(ValueError, match="momentum"):
        FusedTrainStep(sas, momentum=0.9)
    for o in ("rmsprop", "", None, 3):
        with pytest.raises(ValueError, match="optimizer"):
            FusedTrainStep(sas, optimizer=o)


def test_adam_ignores_the_references_default_momentum():
    """The reference's defaults are --optimizer Adam and --momentum None, and it reads momentum in its SGD branch only:
    optimizer=args.optimizer, momentum=args.momentum must pass the argument checks under Adam.  A CPU model then stops
    at the engine (the hot path has no CPU form), which is as far as a machine without a GPU gets; the construction
    itself is checked on the GPU (tests/test_sgd_step_gpu.py)."""
    from rbm_amd.train_step import FusedTrainStep
    for kw in ({"optimizer": "Adam", "momentum": None}, {"optimizer": "adam", "momentum": 0}, {"momentum": None},
               {"optimizer": "ADAM", "momentum": 0.0}):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            FusedTrainStep(_sas_model(), **kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            FusedTrainStep(_bert_model(), **kw)
    for m in (0.9, True, -1):
        with pytest.raises(ValueError, match="needs optimizer='sgd'"):
            FusedTrainStep(_sas_model(), optimizer="Adam", momentum=m)


# ================================================================ the C entry's argument checks
ARG = 1001
FAKE = 0x10000     # 16-byte aligned, points at nothing: every case below must be refused before any launch


def _sgd(**kw):
    import rbm_amd._lib as L
    a = dict(n=1024, p=FAKE, g=FAKE, buf=FAKE, p_bf16=None, state=FAKE, hyper=FAKE, zero_grad=1, prepare=1,
             grad_divisor=None, seed_base=None, tdesc=None, ntd=0, tbase=0, wT=None, loss_sum=None, loss_out=None,
             max_wg=0, stream=None)
    assert set(kw) <= set(a), kw
    a.update(kw)
    return L.lib().rs_sgd_step(*a.values())


def test_rs_sgd_step_rejects_bad_arguments_before_any_launch():
    for n in (0, -4):
        assert _sgd(n=n) == ARG
    for name in ("p", "g", "state", "hyper"):
        assert _sgd(**{name: None}) == ARG, name
    full = dict(ntd=1, p_bf16=FAKE, tdesc=FAKE, wT=FAKE)
    for name in ("p_bf16", "tdesc", "wT"):
        assert _sgd(**{**full, name: None}) == ARG, name
    assert _sgd(ntd=-1, p_bf16=FAKE, tdesc=FAKE, wT=FAKE) == ARG
    assert _sgd(loss_out=FAKE, loss_sum=None, grad_divisor=FAKE) == ARG
    assert _sgd(loss_out=FAKE, loss_sum=FAKE, grad_divisor=None) == ARG
    assert _sgd(max_wg=-1) == ARG
    # a base rs_adam_step would refuse: not 16-byte aligned
    for name in ("p", "g", "buf"):
        assert _sgd(**{name: FAKE + 4}) == ARG, name
    assert _sgd(p_bf16=FAKE + 2) == ARG
