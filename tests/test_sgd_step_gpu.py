"""FusedTrainStep(optimizer="sgd"): the reference's other optimizer (BS/trainers/base.py:229-233) behind every loss
of the step, at tiny shapes (SASRec V = 60, T = 16, d = 64, 2 blocks, B = 8; BERT4Rec the same with 2 heads; sampled
softmax over K = 16 candidates).

fp32 against the oracle: the float64 loss functions of oracle/sas.py / oracle/bert.py (and the tests' restatements of
the CE / sampled-softmax heads over them) differentiated by autograd and fed to torch.optim.SGD in float64.  Bars:
  loss      |loss - ref| < 1e-5 max(1, |ref|)            (FWD_TOL_F32 of tests/test_sas_gpu.py / tests/test_bert.py)
  gradient  ||g - ref|| < 1e-4 ||ref|| per tensor, the analytically zero key-bias gradients against the largest
            tensor's norm                                (GRAD_TOL_F32 and check_grads of the same files)
  parameter after n steps, per tensor: every step's gradient may be off by e = (gradient bar) x the largest reference
            gradient norm of the run; the momentum buffer passes a step-j error on to p with the weights 1, 1 + mu,
            ..., so after n steps ||p - ref|| <= lr e sum_{j <= n} (1 - mu^j) / (1 - mu), plus the float32 update's own
            rounding: the per-element bound of tests/sgd_ref.py (Bound) run on the reference's gradients.
The hyperparameters are float32-representable doubles, so the kernel's casts lose nothing against torch's doubles.
"""
import argparse
import io
import os
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import sgd_ref as R
from conftest import ROOT, rel

pytestmark = pytest.mark.gpu

V, T, D, L, B, K = 60, 16, 64, 2, 8, 16
HEADS = {"sas": 1, "bert": 2}
LR, MOM, WD = float(np.float32(0.05)), float(np.float32(0.9)), float(np.float32(0.01))
# The rate of the comparisons with a float64 TRAJECTORY (the 5-step oracle test, the 200-step curve): 2^-10, the power
# of two next to the 1e-3 the project's other step tests train at.  Both bars assume that rounding moves the run only
# through the update itself; a rate at which the training amplifies float32 rounding breaks that for ANY float32
# implementation.  Measured on the CPU with the reference's own arithmetic (the oracle in torch float32 + torch's
# float32 SGD against the same in float64, this shape, these batches, momentum 0.9, 200 steps): max |loss32 - loss64|
# is 1.1e-2 at 0.05 (step 13), 1.2e-1 at 2^-6, 4.7e-3 at 2^-7, 3.5e-3 at 2^-8, 2.7e-4 at 2^-9 and 1.8e-6 at 2^-10, where
# the float64 curve still falls from 5.2 to 1.4.
LR_REF = 2.0 ** -10
LOSS_TOL, GRAD_TOL = 1e-5, 1e-4
CASES = [("sas", "bce", False), ("sas", "ce", False), ("sas", "sampled_ce", False), ("sas", "sampled_ce", True),
         ("bert", None, False), ("bert", "sampled_ce", False), ("bert", "sampled_ce", True)]


def test_the_bars_are_the_adam_step_tests():
    import test_bert
    import test_sas_gpu
    assert (LOSS_TOL, GRAD_TOL) == (test_sas_gpu.FWD_TOL_F32, test_sas_gpu.GRAD_TOL_F32)
    assert (LOSS_TOL, GRAD_TOL) == (test_bert.FWD_TOL_F32, test_bert.GRAD_TOL_F32)


# ---------------------------------------------------------------- models, batches, the reference loss
def _model(kind, dtype="fp32", p=0.0, l2=0.0, seed=5):
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    torch.manual_seed(seed)
    if kind == "sas":
        a = argparse.Namespace(model_code="sas", num_items=V, max_len=T, device="cuda", sas_hidden_units=D,
                               sas_num_blocks=L, sas_heads=1, sas_dropout=p, l2_emb=l2, rs_dtype=dtype)
    else:
        a = argparse.Namespace(model_code="bert", num_items=V, max_len=T, device="cuda", bert_hidden_units=D,
                               bert_num_blocks=L, bert_num_heads=2, bert_dropout=p, bert_hidden_dropout=p,
                               bert_mask_prob=0.2, model_init_seed=seed, rs_dtype=dtype)
    m = model_factory(a)
    m.train()
    return m


def _logq():
    import test_sce_logq_gpu as tq
    return tq._logq(V)


def _step(kind, loss, logq=False, dtype="fp32", p=0.0, l2=0.0, wd=0.0, seed=5, lr=LR, **kw):
    from rbm_amd.train_step import FusedTrainStep
    m = _model(kind, dtype, p, l2, seed)
    kw.setdefault("optimizer", "sgd")
    if kw["optimizer"] == "sgd":
        kw.setdefault("momentum", MOM)
    q = _logq()[1] if logq else None
    return m, FusedTrainStep(m, lr=lr, weight_decay=wd, loss=loss, logq=q, **kw)


def _P(m):
    return {k: v.detach().cpu().double() for k, v in m.state_dict().items()}


def _cand(seed):
    rng = np.random.default_rng(100 + seed)
    c = rng.integers(1, V + 1, K)
    c[1], c[3], c[4] = 0, c[2], V          # a padding id, a duplicate, the largest id
    return c


def _batches(kind, loss, n, seed=4, rows=B):
    """n host batches (numpy int64 arrays): SAS (seq, pos, neg | cand), BERT (tokens, labels[, cand])"""
    import rbm_amd.data as synth
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if kind == "sas":
            seq, pos, neg = synth.sas_batch(rng, rows, T, V)
            out.append((seq, pos, _cand(i) if loss == "sampled_ce" else neg))
        else:
            tok, lab = synth.bert_batch(rng, rows, T, V, 0.3)
            out.append((tok, lab, _cand(i)) if loss == "sampled_ce" else (tok, lab))
    return out


def _dev(b):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in b)


def _ref_loss(kind, loss, logq=False, l2=0.0):
    """fn(P, host batch) -> the float64 loss (autograd-differentiable in P)"""
    import bert_sce_ref
    import sas_ce_ref
    import sas_sce_ref
    import sce_logq_ref
    from oracle import bert as obert
    from oracle import sas as osas
    q64 = _logq()[0] if logq else None
    h = HEADS[kind]

    def fn(P, b):
        b = [torch.from_numpy(np.ascontiguousarray(x)) for x in b]
        if kind == "sas" and loss == "bce":
            return osas.bce_loss(*osas.forward(P, b[0], b[1], b[2], L, h), b[1], P, l2)
        if kind == "sas" and loss == "ce":
            return sas_ce_ref.ce_loss(P, b[0], b[1], L, h, l2_emb=l2)
        if kind == "sas":
            if q64 is not None:
                return sce_logq_ref.sas_sce_loss(P, b[0], b[1], b[2], q64, L, h)
            return sas_sce_ref.sce_loss(P, b[0], b[1], b[2], L, h, l2_emb=l2)
        if loss is None:
            return obert.ce_loss(obert.forward(P, b[0], L, h), b[1])
        if q64 is not None:
            return sce_logq_ref.bert_sce_loss(P, b[0], b[1], b[2], q64, L, h)
        return bert_sce_ref.sce_loss(P, b[0], b[1], b[2], L, h)
    return fn


def _grads_of(fn, P, b):
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    loss = fn(leaves, b)
    loss.backward()
    return float(loss), {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in leaves.items()}


def _parts(kind, name, a):
    """[(label, sub-array, analytically-zero-gradient)] of a tensor: the attention key bias (the middle third of SAS's
    in_proj_bias, BERT's linear_layers.1.bias) has a zero gradient and is held against the global scale"""
    a = np.asarray(a)
    if kind == "sas" and name.endswith("in_proj_bias"):
        d = a.shape[0] // 3
        return [(name + "[q,v]", np.concatenate([a[:d], a[2 * d:]]), False), (name + "[k]", a[d:2 * d], True)]
    if kind == "bert" and "linear_layers.1.bias" in name:
        return [(name, a, True)]
    return [(name, a, False)]


def _flat_name(kind, k):
    return k[4:] if kind == "sas" else k      # the SAS flat buffer is built over model.sas


@pytest.mark.parametrize("kind,loss,logq,wd,l2", [c + (0.0, 0.0) for c in CASES] + [("sas", "bce", False, WD, 0.0),
                                                                                  ("sas", "bce", False, 0.0, 0.01)])
def test_fp32_steps_match_the_oracle_with_torch_sgd(kind, loss, logq, wd, l2):
    torch.set_num_threads(16)
    steps = 5
    m, tr = _step(kind, loss, logq, l2=l2, wd=wd, lr=LR_REF)
    assert type(tr.opt).__name__ == "FusedSGD" and tr.opt.marks is None and not tr._early_ok
    fn = _ref_loss(kind, loss, logq, l2)
    Pref = {k: v.clone().requires_grad_(True) for k, v in _P(m).items()}
    opt = torch.optim.SGD(list(Pref.values()), lr=LR_REF, momentum=MOM, weight_decay=wd)
    s = R.scalars(LR_REF, MOM, wd)
    assert (s["lr"], s["mom"], s["wd"]) == (LR_REF, MOM, wd)     # float32-representable: the casts lose nothing
    runs = {k: R.Run(v.detach().numpy().reshape(-1), True, np.float64) for k, v in Pref.items()}
    bounds = {k: R.Bound(v.numel(), True) for k, v in Pref.items()}
    gmax = {}
    for n, hb in enumerate(_batches(kind, loss, steps), 1):
        b = _dev(hb)
        # the step's loss and gradient against the reference AT THE STEP'S OWN parameters
        l64, g64 = _grads_of(fn, _P(m), hb)
        tr._compute(*tr._batch(b))
        tr._l2(tr.loss_out[2:3])
        torch.cuda.synchronize()
        lg = float(tr.loss_out[2].item())
        assert abs(lg - l64) < LOSS_TOL * max(1.0, abs(l64)), (n, lg, l64)
        scale = max(float(np.linalg.norm(v)) for v in g64.values())
        worst = (0.0, None)
        for k, r in g64.items():
            g = tr.flat.view(_flat_name(kind, k), tr.flat.grad).detach().cpu().numpy()
            for label, ga, zero in _parts(kind, k, g):
                ra = dict((x[0], x[1]) for x in _parts(kind, k, r))[label]
                if zero or not np.linalg.norm(ra):
                    assert np.linalg.norm(ga - ra) <= GRAD_TOL * scale, (n, label)
                else:
                    e = rel(ga, ra)
                    worst = max(worst, (e, label))
                    assert e < GRAD_TOL, (n, label, e)
        tr.flat.grad.zero_()
        # the step itself
        ls = float(tr.step(*b).item())
        assert ls == lg, (n, ls, lg)
        assert int(torch.count_nonzero(tr.flat.grad)) == 0
        # the reference trajectory
        opt.zero_grad()
        lr_ = fn(Pref, hb)
        lr_.backward()
        for k, v in Pref.items():
            g = (v.grad if v.grad is not None else torch.zeros_like(v)).numpy().reshape(-1)
            for label, ga, zero in _parts(kind, k, g.reshape(v.shape)):
                gmax[label] = max(gmax.get(label, 0.0), scale if zero else float(np.linalg.norm(ga)))
            bounds[k].step(runs[k], g, s)
            runs[k].step(g, s)
        opt.step()
        torch.cuda.synchronize()
        geo = sum((1.0 - MOM ** j) / (1.0 - MOM) for j in range(1, n + 1))
        got = _P(m)
        for k, v in Pref.items():
            assert np.abs(runs[k].p - v.detach().numpy().reshape(-1)).max() <= 1e-12      # Run tracks torch's SGD
            eP = bounds[k].eP.reshape(v.shape)
            for (label, pa, _), (_, ra, _), (_, ea, _) in zip(_parts(kind, k, got[k].numpy()),
                                                             _parts(kind, k, v.detach().numpy()),
                                                             _parts(kind, k, eP)):
                bar = LR_REF * GRAD_TOL * gmax[label] * geo + float(np.linalg.norm(ea))
                err = float(np.linalg.norm(pa - ra))
                assert err <= bar, (n, label, err, bar)
        print(kind, loss, logq, "step", n, "loss", lg, "ref", l64, "worst gradient", worst)
    assert float(tr.opt.state[0].item()) == steps


# ---------------------------------------------------------------- bitwise: step == composition == graph
def _manual_step(tr, b):
    """forward + backward, then rs_sgd_step driven by hand over the flat buffers"""
    from rbm_amd import ops
    tr._compute(*tr._batch(b))
    tr._l2(tr.loss_out[2:3])
    f, o, eng = tr.flat, tr.opt, tr.engine
    spec = eng.transposed_spec() if hasattr(eng, "transposed_spec") else None
    n = f.numel
    ops.sgd_step(f.data[:n], f.grad[:n], o.buf, f.bf16[:n] if f.bf16 is not None else None, o.state, o.hyper,
                 zero_grad=True, prepare=True,
                 seed_base=eng.seed_base, transposed=spec)
    return tr.loss_out[2:3]


# fp32 for SASRec only: BERT's fp32 token-table gradient is summed with float atomics (embedding.hip, embed_bwd; the
# inverted-index form is the bf16 path's, BERTEngine._det_table), so two fp32 BERT runs do not share their bits
# whatever the optimizer
@pytest.mark.parametrize("kind,loss,logq,dtype", [c + ("bf16",) for c in CASES] + [("sas", "bce", False, "fp32")])
def test_step_equals_composition_equals_captured_graph(kind, loss, logq, dtype):
    bs = [_dev(b) for b in _batches(kind, loss, 3)]
    runs = []
    for mode in ("step", "manual", "graph"):
        m, tr = _step(kind, loss, logq, dtype=dtype, p=0.2)
        tr.engine.seed_base.fill_(77)
        if mode == "graph":
            tr.capture(*bs[0], warmup=2)
            losses = [float(tr.replay(*b).item()) for b in bs]
        else:
            f = tr.step if mode == "step" else (lambda *b: _manual_step(tr, b))
            for _ in range(2):
                f(*bs[0])
            losses = [float(f(*b).item()) for b in bs]
        torch.cuda.synchronize()
        runs.append((losses, tr.flat.data.clone(), tr.opt.buf.clone(), int(tr.engine.seed_base.item()),
                     float(tr.opt.state[0].item()),
                     tr.flat.bf16.clone() if tr.flat.bf16 is not None else torch.zeros(1)))
    assert all(np.isfinite(runs[0][0])) and len(set(runs[0][0])) == 3
    assert runs[0][3] == 77 + 5 and runs[0][4] == 5
    for r in runs[1:]:
        assert r[0] == runs[0][0], (r[0], runs[0][0])
        assert torch.equal(r[1], runs[0][1]) and torch.equal(r[2], runs[0][2]) and torch.equal(r[5], runs[0][5])
        assert r[3:5] == runs[0][3:5]


def test_two_unrolled_steps_equal_two_single_steps():
    bs = [torch.stack(_dev(b)) for b in _batches("sas", "bce", 4)]
    m0, t0 = _step("sas", "bce", dtype="bf16", p=0.2)
    for _ in range(2):
        t0.step(*bs[0].unbind(0))
    want = [float(t0.step(*b.unbind(0)).item()) for b in bs]
    m1, t1 = _step("sas", "bce", dtype="bf16", p=0.2)
    t1.capture(*bs[0].unbind(0), warmup=2, steps_per_graph=2)
    got = []
    for r in range(2):
        got += t1.replay_packed(torch.stack(bs[2 * r:2 * r + 2])).tolist()
    torch.cuda.synchronize()
    assert got == want and all(np.isfinite(want))
    assert torch.equal(t0.flat.data, t1.flat.data) and torch.equal(t0.opt.buf, t1.opt.buf)
    assert float(t1.opt.state[0].item()) == 6


@pytest.mark.parametrize("kind,loss", [("sas", "bce"), ("sas", "sampled_ce"), ("bert", "sampled_ce")])
def test_capture_sampled_runs_under_sgd(kind, loss):
    import rbm_amd.data as synth
    from rbm_amd.dataloaders import DeviceBertMasker, DeviceWarpSampler
    hist = synth.user_histories(np.random.default_rng(3), 100, T, V)
    shared = K if loss == "sampled_ce" else None
    runs = []
    for _ in range(2):
        m, tr = _step(kind, loss, dtype="bf16", p=0.2)
        if kind == "sas":
            sampler = DeviceWarpSampler(hist, V, B, T, seed=9, **({"shared_negs": shared} if shared else {}))
        else:
            sampler = DeviceBertMasker(hist, V, B, T, 0.3, seed=9, shared_negs=shared)
        tr.capture_sampled(sampler, warmup=2)
        losses = [float(tr.replay_sampled().item()) for _ in range(3)]
        runs.append((losses, tr.flat.data.clone(), tr.opt.buf.clone()))
    assert runs[0][0] == runs[1][0] and all(np.isfinite(runs[0][0])) and len(set(runs[0][0])) == 3
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    assert float(tr.opt.state[0].item()) == 5


# ---------------------------------------------------------------- bf16: the compute copies
@pytest.mark.parametrize("kind,loss", [("sas", "bce"), ("bert", None)])
def test_bf16_copies_follow_the_masters(kind, loss):
    m, tr = _step(kind, loss, dtype="bf16", p=0.2)
    eng = tr.engine
    for b in _batches(kind, loss, 3):
        tr.step(*_dev(b))
        torch.cuda.synchronize()
        assert torch.equal(tr.flat.bf16, tr.flat.data.to(torch.bfloat16))
        if kind == "sas":
            assert eng.adam_transposes and eng._wT is not None
            got = eng._wT.clone()
            eng.adam_transposes = False
            eng._refresh_transposed()
            torch.cuda.synchronize()
            eng.adam_transposes = True
            assert torch.equal(got, eng._wT)
    assert float(tr.opt.buf.abs().sum()) > 0


# ---------------------------------------------------------------- StepLR
def test_step_lr_reaches_the_device_and_a_captured_graph():
    import rbm_amd  # noqa: F401
    from rbm_amd.train_step import FusedSGD, FusedStepLR
    n, wd = 50_003, 0.01
    p0, grads = R.scenario(2, n, 6)

    class _Flat:
        device = torch.device("cuda")
        numel = n
        data = torch.from_numpy(p0).cuda()
        grad = torch.zeros(n, device="cuda")
        bf16 = None
    fs = FusedSGD(_Flat, lr=LR, momentum=MOM, weight_decay=wd)
    sched = FusedStepLR(fs, step_size=2, gamma=0.5)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    topt = torch.optim.SGD([tp], lr=LR, momentum=MOM, weight_decay=wd)
    tsched = torch.optim.lr_scheduler.StepLR(topt, step_size=2, gamma=0.5)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    before = _Flat.data.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):       # captured before the first decay
        fs.step()
    torch.cuda.synchronize()
    assert torch.equal(_Flat.data, before) and float(fs.state[0].item()) == 0
    lrs = []
    for epoch in range(6):
        lrs.append(float(fs.hyper[0].item()))
        assert lrs[-1] == tsched.get_last_lr()[0] == topt.param_groups[0]["lr"]
        _Flat.grad.copy_(torch.from_numpy(grads[epoch]))
        graph.replay()
        tp.grad = torch.from_numpy(grads[epoch].copy())
        topt.step()
        sched.step()
        tsched.step()
        assert sched.get_last_lr() == tsched.get_last_lr()
    torch.cuda.synchronize()
    assert lrs == [LR, LR, LR * 0.5, LR * 0.5, LR * 0.25, LR * 0.25]
    emu = R.Run(p0, True, np.float32)
    for g, lr in zip(grads, lrs):
        emu.step(g, R.scalars(lr, MOM, wd))
    assert R.same_bits(_Flat.data.cpu().numpy(), emu.p) and R.same_bits(fs.buf.cpu().numpy(), emu.buf)
    assert R.check_run(emu, tp.detach().numpy(), topt.state[tp]["momentum_buffer"].numpy()) == []
    assert float(fs.state[0].item()) == 6 and int(torch.count_nonzero(_Flat.grad)) == 0


def test_step_lr_through_the_trainer_and_its_captured_graph():
    """FusedStepLR(step, ...) takes the trainer: its rate lands in the trainer's FusedSGD, a step graph captured
    before the first decay trains at each epoch's rate bit for bit as the eager twin, and the decay is no no-op."""
    from rbm_amd.train_step import FusedStepLR
    bs = [_dev(b) for b in _batches("sas", "bce", 6)]
    tp = torch.nn.Parameter(torch.zeros(1))
    tsched = torch.optim.lr_scheduler.StepLR(torch.optim.SGD([tp], lr=LR), step_size=2, gamma=0.5)
    want = []
    for _ in range(6):
        want.append(tsched.get_last_lr()[0])
        tsched.optimizer.step()
        tsched.step()
    runs = {}
    for mode in ("graph", "eager", "constant"):
        m, tr = _step("sas", "bce", dtype="bf16", p=0.2)
        sched = FusedStepLR(tr, step_size=2, gamma=0.5)
        assert sched.optimizer is tr.opt and type(tr.opt).__name__ == "FusedSGD"
        if mode == "graph":
            tr.capture(*bs[0], warmup=1)
        else:
            tr.step(*bs[0])
        snaps = []
        for epoch in range(6):
            if mode != "constant":
                assert float(tr.opt.hyper[0].item()) == want[epoch]
            (tr.replay if mode == "graph" else tr.step)(*bs[epoch])
            if mode != "constant":
                sched.step()
            snaps.append(tr.flat.data.clone())
        torch.cuda.synchronize()
        runs[mode] = snaps
    for x, y in zip(runs["graph"], runs["eager"]):
        assert torch.equal(x, y)
    assert torch.equal(runs["eager"][1], runs["constant"][1]) and not torch.equal(runs["eager"][3], runs["constant"][3])
    assert want == [LR, LR, LR * 0.5, LR * 0.5, LR * 0.25, LR * 0.25]


# ---------------------------------------------------------------- checkpoints
def _roundtrip(ck):
    buf = io.BytesIO()
    torch.save(ck, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=True)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_checkpoint_resumes_bit_for_bit_and_in_torch_sgd(dtype):
    from rbm_amd.losses import sampled_bce
    bs = [_dev(b) for b in _batches("sas", "bce", 5)]
    m, tr = _step("sas", "bce", dtype=dtype, wd=WD)
    assert tr.optimizer_state_dict()["state"] == {}                    # before the first step
    for b in bs[:2]:
        tr.step(*b)
    ck = _roundtrip(tr.checkpoint(epoch=1))
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "epoch"}
    sd = ck["optimizer_state_dict"]
    g = sd["param_groups"][0]
    want = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=LR).state_dict()["param_groups"][0]
    assert set(want) <= set(g) and set(g) - set(want) == {"fused_step"}          # torch's own keys + the count
    assert (g["lr"], g["momentum"], g["weight_decay"], g["dampening"], g["nesterov"]) == (LR, MOM, WD, 0, False)
    assert g["fused_step"] == 2.0
    params = list(m.parameters())
    assert sorted(sd["state"]) == list(range(len(params)))
    for i, p in enumerate(params):
        assert set(sd["state"][i]) == {"momentum_buffer"} and sd["state"][i]["momentum_buffer"].shape == p.shape

    # torch.optim.SGD on the CPU: loads it, and its own state_dict() gives it back
    cpu = [torch.nn.Parameter(v.detach().cpu().clone()) for v in params]
    topt = torch.optim.SGD(cpu, lr=1.0)
    topt.load_state_dict(_roundtrip(sd))
    back = topt.state_dict()
    assert back["param_groups"] == sd["param_groups"]
    assert sorted(back["state"]) == sorted(sd["state"])
    for i in sd["state"]:
        assert torch.equal(back["state"][i]["momentum_buffer"], sd["state"][i]["momentum_buffer"])

    # the run continues in torch.optim.SGD on the reference's loop ...
    m2 = _model("sas", dtype, seed=6)
    m2.load_state_dict(ck["model_state_dict"])
    opt2 = torch.optim.SGD(m2.parameters(), lr=1.0)
    opt2.load_state_dict(_roundtrip(sd))
    assert opt2.param_groups[0]["lr"] == LR and opt2.param_groups[0]["momentum"] == MOM
    opt2.zero_grad()
    pl, nl = m2(*bs[2])
    sampled_bce(pl, nl, bs[2][1]).backward()
    opt2.step()
    # ... and in a fresh fused trainer, bit for bit
    m3, tr3 = _step("sas", "bce", dtype=dtype, seed=6, lr=1.0, momentum=0.5)
    tr3.load_checkpoint(_roundtrip(ck))
    assert float(tr3.opt.state[0].item()) == 2 and float(tr3.opt.hyper[1].item()) == MOM
    l3 = [float(tr3.step(*b).item()) for b in bs[2:]]
    l1 = [float(tr.step(*b).item()) for b in bs[2:3]]
    torch.cuda.synchronize()
    p1 = torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    p2 = torch.cat([p.detach().reshape(-1) for p in m2.parameters()])
    r = ((p1 - p2).norm() / p1.norm()).item()
    assert r < (1e-6 if dtype == "fp32" else 1e-3), r
    l1 += [float(tr.step(*b).item()) for b in bs[3:]]
    torch.cuda.synchronize()
    assert l1 == l3
    assert torch.equal(tr.flat.data, tr3.flat.data) and torch.equal(tr.opt.buf, tr3.opt.buf)
    assert float(tr3.opt.state[0].item()) == 5
    if dtype == "bf16":
        assert torch.equal(tr.flat.bf16, tr3.flat.bf16)


def test_checkpoint_formats_without_momentum_from_torch_and_across_optimizers():
    bs = [_dev(b) for b in _batches("sas", "bce", 2)]
    # momentum = 0: an empty state, after a step too
    m0, t0 = _step("sas", "bce", momentum=0.0)
    assert t0.opt.buf is None
    t0.step(*bs[0])
    sd0 = t0.optimizer_state_dict()
    assert sd0["state"] == {} and sd0["param_groups"][0]["momentum"] == 0 and sd0["param_groups"][0]["fused_step"] == 1
    # a checkpoint torch.optim.SGD wrote (the reference's trainer): buffers loaded, the run continues bit for bit
    m1, t1 = _step("sas", "bce")
    t1.step(*bs[0])
    ck = t1.checkpoint()
    ref_sd = _roundtrip(ck["optimizer_state_dict"])
    del ref_sd["param_groups"][0]["fused_step"]                       # as torch itself writes it
    m2, t2 = _step("sas", "bce", seed=6)
    t2.load_checkpoint({"model_state_dict": ck["model_state_dict"], "optimizer_state_dict": ref_sd})
    assert torch.equal(t1.opt.buf, t2.opt.buf) and float(t2.opt.state[0].item()) == 1
    # a step built without momentum takes the buffer on when the load comes before any capture ...
    m3, t3 = _step("sas", "bce", seed=6, momentum=0.0)
    t3.load_checkpoint(_roundtrip(ck))
    assert t3.opt.buf is not None and torch.equal(t1.opt.buf, t3.opt.buf) and t3.momentum == MOM
    l1 = float(t1.step(*bs[1]).item())
    assert l1 == float(t2.step(*bs[1]).item()) == float(t3.step(*bs[1]).item())
    assert torch.equal(t1.flat.data, t2.flat.data) and torch.equal(t1.flat.data, t3.flat.data)
    # ... and is refused once graphs hold the buffer's pointer and the kernel chosen for it (both directions)
    t3.capture(*bs[0], warmup=1)
    with pytest.raises(ValueError, match="captured"):
        t3.load_optimizer_state_dict(sd0)
    t0.capture(*bs[0], warmup=1)
    with pytest.raises(ValueError, match="captured"):
        t0.load_optimizer_state_dict(_roundtrip(ck["optimizer_state_dict"]))
    assert t0.opt.buf is None and t3.opt.buf is not None
    t3.load_optimizer_state_dict(_roundtrip(ck["optimizer_state_dict"]))       # the same presence: accepted
    # the refusals
    ma, ta = _step("sas", "bce", optimizer="adam")
    ta.step(*bs[0])
    adam_sd, sgd_sd = ta.optimizer_state_dict(), t1.optimizer_state_dict()
    with pytest.raises(ValueError, match="optimizer='sgd'"):
        t1.load_optimizer_state_dict(adam_sd)
    with pytest.raises(ValueError, match="optimizer='adam'"):
        ta.load_optimizer_state_dict(sgd_sd)
    for key, val in (("dampening", 0.1), ("nesterov", True)):
        bad = _roundtrip(sgd_sd)
        bad["param_groups"][0][key] = val
        with pytest.raises(ValueError, match=key):
            t1.load_optimizer_state_dict(bad)


# ---------------------------------------------------------------- a curve
def test_fp32_curve_of_200_steps_follows_float64_torch_sgd():
    """|loss - reference| <= 1e-3 at every step: the bar tests/test_curves_gpu.py holds its fp32 curve to over its
    first 300 steps.  The reference curve itself must fall, so a flat one cannot pass."""
    torch.set_num_threads(16)
    steps = 200
    m, tr = _step("sas", "bce", lr=LR_REF)
    fn = _ref_loss("sas", "bce")
    P = {k: v.clone().requires_grad_(True) for k, v in _P(m).items()}
    opt = torch.optim.SGD(list(P.values()), lr=LR_REF, momentum=MOM)
    got, want = [], []
    for hb in _batches("sas", "bce", steps, seed=11):
        got.append(tr.step(*_dev(hb)).clone())
        opt.zero_grad()
        loss = fn(P, hb)
        loss.backward()
        opt.step()
        want.append(float(loss))
    got = np.array([float(x.item()) for x in got])
    want = np.array(want)
    assert np.mean(want[-10:]) < 0.5 * np.mean(want[:10]), (want[:10], want[-10:])
    err = np.abs(got - want)
    print("sgd curve fp32: max |dloss|", err.max(), "at", int(err.argmax()), "; first / last", want[0], want[-1])
    assert err.max() <= 1e-3, (err.max(), int(err.argmax()))


# ---------------------------------------------------------------- data parallel: two processes on one GPU, gloo
BR, DP_STEPS = 4, 3
DP_MODES = [(False, False), (False, True), (True, False), (True, True)]     # (graph, overlap)
CHILD_TIMEOUT = 240.0


def _dp_loss(kind):
    return "bce" if kind == "sas" else None


def _dp_batches(kind, world):
    bs = _batches(kind, _dp_loss(kind), DP_STEPS, seed=5, rows=world * BR)
    return [[tuple(x[r * BR:(r + 1) * BR] for x in b) for r in range(world)] for b in bs], bs


def _dp_worker(rank, world, rdzv, kind, out_dir):
    import sys
    sys.path.insert(0, ROOT)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=rdzv, rank=rank, world_size=world)
    try:
        from rbm_amd import dp as dpx
        local = [_dev(b[rank]) for b in _dp_batches(kind, world)[0]]
        out = {}
        for graph, overlap in DP_MODES:
            sparse = "on" if (kind == "bert" and overlap) else "auto"
            m, tr = _step(kind, _dp_loss(kind), dp=True, overlap=overlap, sparse_rows=sparse,
                          bucket_numel=None if overlap else 1 << 30,
                          max_labelled=BR * T if kind == "bert" else None)
            assert type(tr.opt).__name__ == "FusedSGD" and tr.rshard is None and tr.vshard is None
            sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
            if graph:
                tr.capture(*local[0])
                tr.model.load_state_dict(sd0)
                tr.masters_loaded()
                tr.opt.buf.zero_()
                tr.opt.state.zero_()
            losses, counts = [], []
            for b in local:
                losses.append(float((tr.replay(*b) if graph else tr.step(*b)).item()))
                counts.append(float(tr.flat.aux[dpx.COUNT].item()))
            torch.cuda.synchronize()
            out[f"{int(graph)}{int(overlap)}"] = {
                "losses": losses, "counts": counts, "equal": tr.replicas_equal(),
                "sparse": tr.sparse is not None, "step": float(tr.opt.state[0].item()),
                "sd": {k: v.detach().cpu().clone() for k, v in m.state_dict().items()},
                "buf": tr.opt.buf.cpu().clone()}
        torch.save(out, os.path.join(out_dir, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


def _spawn(fn, args, world):
    ctx = mp.spawn(fn, args=args, nprocs=world, join=False)
    deadline = time.monotonic() + CHILD_TIMEOUT
    try:
        while not ctx.join(timeout=5.0):
            if time.monotonic() > deadline:
                raise TimeoutError(f"a data-parallel child ran past {CHILD_TIMEOUT} s")
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
                p.join()


@pytest.mark.parametrize("kind", ["sas", "bert"])
def test_two_rank_sgd_step_equals_the_single_process_step(tmp_path, kind):
    """Two child processes hold the GPU for the exchange; the pytest process, which has held it since the first GPU
    test of the session and cannot let go of it, computes the single-process reference after they have exited.  So
    three processes have the GPU open while the children run (as in tests/test_dp_multirank_gpu.py), two of them
    started here."""
    import test_dp_multirank_gpu as td
    world = 2
    _spawn(_dp_worker, (world, td._rendezvous(tmp_path), kind, str(tmp_path)), world)
    split, whole = _dp_batches(kind, world)
    m, tr = _step(kind, _dp_loss(kind), max_labelled=world * BR * T if kind == "bert" else None)
    init = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    ref_losses = [float(tr.step(*_dev(b)).item()) for b in whole]
    torch.cuda.synchronize()
    ref = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    counts = [float((b[1] != 0).sum()) for b in whole]
    r0 = torch.load(tmp_path / "r0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "r1.pt", weights_only=True)
    loss_tol, upd_tol, upd_med_tol = 1e-5, 1e-3, 1e-5          # the fp32 bars of tests/test_dp_multirank_gpu.py
    assert sorted(r0) == ["00", "01", "10", "11"]
    for mode in r0:
        a, b = r0[mode], r1[mode]
        assert a["equal"] and b["equal"] and a["step"] == b["step"] == DP_STEPS, mode
        assert a["sparse"] == b["sparse"] == (kind == "bert" and mode[1] == "1"), mode
        assert a["counts"] == counts and b["counts"] == counts, (mode, a["counts"], counts)
        assert a["losses"] == b["losses"], mode
        assert np.allclose(a["losses"], ref_losses, rtol=loss_tol), (mode, a["losses"], ref_losses)
        assert torch.equal(a["buf"], b["buf"]), mode
        errs = {}
        for k in ref:
            assert torch.equal(a["sd"][k], b["sd"][k]), (mode, k)
            if td._skip_key(kind, k):
                continue
            errs[k] = td._update_err(kind, k, a["sd"][k], ref[k], init[k])
        worst = max(errs, key=errs.get)
        med = float(np.median(list(errs.values())))
        print(f"sgd {kind} {mode}: update error median {med:.3g}, max {errs[worst]:.3g} ({worst})")
        assert errs[worst] < upd_tol, (mode, worst, errs[worst])
        assert med < upd_med_tol, (mode, med)


# ---------------------------------------------------------------- the default has not moved
def test_adam_is_the_default_and_both_spellings_are_one_step():
    b = _dev(_batches("sas", "bce", 1)[0])
    outs = []
    # the last: the reference's own defaults (--optimizer Adam, --momentum None) through the documented binding
    for kw in ({}, {"optimizer": "adam"}, {"optimizer": "Adam", "momentum": 0.0}, {"optimizer": "Adam", "momentum": None}):
        from rbm_amd.train_step import FusedTrainStep
        m = _model("sas", "bf16", p=0.2)
        tr = FusedTrainStep(m, lr=1e-3, **kw)
        assert type(tr.opt).__name__ == "FusedAdam" and tr.optimizer == "adam"
        tr.engine.seed_base.fill_(77)
        loss = float(tr.step(*b).item())
        torch.cuda.synchronize()
        outs.append((loss, tr.flat.data.clone(), tr.opt.m.clone(), tr.opt.v.clone()))
    for o in outs[1:]:
        assert o[0] == outs[0][0] and all(torch.equal(x, y) for x, y in zip(o[1:], outs[0][1:]))
    m, tr = _step("sas", "bce", optimizer="SGD")
    assert type(tr.opt).__name__ == "FusedSGD" and tr.optimizer == "sgd"
