"""FusedTrainStep(max_grad_norm=): global gradient-norm clipping inside the fused step, at the tiny shapes of
tests/test_sgd_step_gpu.py (V = 60, T = 16, d = 64, 2 blocks, B = 8, K = 16; dropout 0 and fp32 unless a test says
otherwise) and its seven (model, loss, logq) cases, under both optimizers.

The step's record {grad_norm, clip_coef, effective divisor} is held to the bounds derived in tests/gradnorm_ref.py
against the extended-precision norm of the step's own gradient.  The update is then restated on the host over the flat
vector with divisor = THE STEP'S OWN effective divisor, by the modules the optimizers' own tests use, at their bars:
  sgd   tests/sgd_ref.py update in float32: bit for bit (p by bits, the momentum buffer by value), as
        tests/test_sgd_gpu.py compares rs_sgd_step;
  adam  tests/adam_rows_ref.py update in float64 from the GPU's own state before the step: v within 4 float32 ulps per
        element, m and p within 4 ulps of the tensor's largest magnitude (ULPS of that module, the bars of
        tests/test_adam_gpu.py / tests/test_adam_rows_gpu.py), per parameter tensor.
The step's gradient comes from a bare _compute (no update) on the same object right before the step, copied off and
cleared.  fp32 BERT is the exception: its token-table gradient is summed with float atomics (embedding.hip), so two
runs do not share their bits (tests/test_sgd_step_gpu.py says the same of its bitwise test); there the step is driven
as its own two halves, _compute(update=True) and _update(), and the gradient is read between them."""
import argparse

import numpy as np
import pytest
import torch

import adam_rows_ref as A
import gradnorm_ref as G
import sgd_ref as R
import test_sgd_step_gpu as S

pytestmark = pytest.mark.gpu

INF = float("inf")
LRS = {"adam": 1e-3, "sgd": S.LR}


def _mk(kind, loss, logq=False, opt="adam", **kw):
    kw.setdefault("lr", LRS[opt])
    if opt == "sgd":
        kw.setdefault("momentum", S.MOM)
    return S._step(kind, loss, logq, optimizer=opt, **kw)


def _reproducible(tr):
    return not (tr.kind == "bert" and tr.flat.bf16 is None)


def _bare_grad(tr, b):
    """the step's gradient (the regulariser's included) from a bare forward + backward, copied off and cleared"""
    tr._compute(*tr._batch(b))
    tr._l2(tr.loss_out[2:3])
    torch.cuda.synchronize()
    g = tr.flat.grad[:tr.flat.numel].cpu().numpy().copy()
    tr.flat.grad.zero_()
    return g


def _opt_state(tr):
    o = tr.opt
    names = ("m", "v") if tr.optimizer == "adam" else (("buf",) if o.buf is not None else ())
    out = {"p": tr.flat.data.cpu().numpy().copy()}
    out.update({n: getattr(o, n).cpu().numpy().copy() for n in names})
    return out


def _run_step(tr, b):
    """One step; returns (the gradient it applied, the state before it).  See the module docstring."""
    if _reproducible(tr):
        g = _bare_grad(tr, b)
        before = _opt_state(tr)
        tr.step(*b)
    else:
        _bare_grad(tr, b)
        before = _opt_state(tr)
        tr._compute(*tr._batch(b), update=True)
        torch.cuda.synchronize()
        g = tr.flat.grad[:tr.flat.numel].cpu().numpy().copy()
        tr._update()
    torch.cuda.synchronize()
    return g, before


def _record(tr):
    return tr._clip_rec[:3].cpu().numpy()


def _check_record(tr, g, mx, what):
    rec = _record(tr)
    ref = G.reference(G.sumsq(g), mx)
    print(what, "record", rec, "reference", ref)
    assert float(tr.grad_norm) == rec[0] and float(tr.clip_coef) == rec[1]
    assert G.check_record(rec, ref, g.size) == [], what
    return rec


def _check_update(tr, g, before, eff, touched=None, what=""):
    """the host restatement with the step's own effective divisor against the GPU state (bars: module docstring).
    touched: {table name: row ids} of sparse tables -- every other row of theirs must keep its bits."""
    f = tr.flat
    after = _opt_state(tr)
    live = np.ones(f.numel, bool)
    for name, rows in (touched or {}).items():
        shp = f.shapes[name]
        w = shp[1] if len(shp) > 1 else 1
        m = np.zeros(shp[0], bool)
        m[rows.cpu().numpy()] = True
        live[f.offsets[name]:f.offsets[name] + shp[0] * w] = np.repeat(m, w)
    for k in before:
        assert R.same_bits(before[k][~live], after[k][~live]), (what, k, "an untouched row changed")
    if tr.optimizer == "sgd":
        lr, mom, wd = tr.opt.hyper.cpu().tolist()
        s = R.scalars(lr, mom, wd, divisor=float(eff))
        P, Bf = R.update(before["p"], g, before.get("buf"), s, np.float32)
        assert R.same_bits(P, after["p"]), (what, "p", R.mismatches(P, after["p"]))
        if Bf is not None:
            assert R.mismatches(Bf, after["buf"]) == 0, (what, "buf")
        return
    hyper = tr.opt.hyper.cpu().tolist()
    s = A.step_scalars(float(tr.opt.state[0].item()), hyper, divisor=float(eff))
    assert float(tr.opt.state[3].item()) == float(s["gs"])          # the kernels' gradient scale is 1 / eff
    worst = {}
    for name in f.names:
        n = int(np.prod(f.shapes[name]))
        sl = slice(f.offsets[name], f.offsets[name] + n)
        lv = live[sl]
        if not lv.any():
            continue
        P, M, V = A.update(before["p"][sl][lv], g[sl][lv], before["m"][sl][lv], before["v"][sl][lv], s, np.float64)

        class _T:
            p, m, v = after["p"][sl][lv], after["m"][sl][lv], after["v"][sl][lv]

        class _Ref:
            p, m, v = P, M, V
        errs = A.state_errors(_T, _Ref)
        # v: the module's bar assumes gj carries one rounding.  With a divisor AND a decay, gj = fma(wd, p, fl(g gs))
        # keeps fl(g gs)'s absolute error 2^-24 |g gs| through a sum that may cancel, and v takes 2 (1 - b2) |gj| of it
        # (the derivative of (1 - b2) gj^2): that much is allowed on top, per element; zero whenever wd == 0 or gs == 1
        if float(s["wd"]) != 0.0 and float(s["gs"]) != 1.0:
            ggs = np.abs(g[sl][lv].astype(np.float64) * float(s["gs"]))
            gj = float(s["wd"]) * before["p"][sl][lv].astype(np.float64) + g[sl][lv].astype(np.float64) * float(s["gs"])
            extra = 2.0 * float(s["omb2"]) * np.abs(gj) * G.U32 * ggs
            dv = np.abs(_T.v.astype(np.float64) - V)
            errs["v"] = float(((dv - extra).clip(min=0) / A.EPS32 / np.maximum(np.abs(V), 1e-30)).max())
        for k, e in errs.items():
            worst[k] = max(worst.get(k, 0.0), e)
            assert e <= A.ULPS, (what, name, k, e)
    print(what, "adam restatement, worst ulps", worst)


CLIP_CASES = [c + (0.0, 0.0) for c in S.CASES] + [("sas", "bce", False, S.WD, 0.0), ("sas", "bce", False, 0.0, 0.01)]


@pytest.mark.parametrize("opt", ["adam", "sgd"])
@pytest.mark.parametrize("kind,loss,logq,wd,l2", CLIP_CASES)
def test_clipped_update(kind, loss, logq, wd, l2, opt):
    """4 steps on 4 batches, max_grad_norm = half the first step's norm.  wd != 0: the decay enters after the scale
    (outside the norm); l2 != 0: the regulariser's gradient is part of the gradient the norm is taken of."""
    m, tr = _mk(kind, loss, logq, opt, wd=wd, l2=l2, max_grad_norm=INF)
    assert not tr._early_ok and tr.grad_norm is not None
    mx, coefs, gaps = INF, [], []
    for n, hb in enumerate(S._batches(kind, loss, 4)):
        b = S._dev(hb)
        if n == 0:
            mx = 0.5 * float(np.sqrt(float(G.sumsq(_bare_grad(tr, b)))))
            tr.set_max_grad_norm(mx)
        if l2:      # the loss gradient alone, without the regulariser's part
            tr._compute(*tr._batch(b))
            torch.cuda.synchronize()
            bare = float(np.sqrt(float(G.sumsq(tr.flat.grad[:tr.flat.numel].cpu().numpy()))))
            tr.flat.grad.zero_()
        g, before = _run_step(tr, b)
        what = f"{kind} {loss} logq={logq} {opt} wd={wd} l2={l2} step {n + 1}"
        rec = _check_record(tr, g, mx, what)
        coefs.append(float(rec[1]))
        _check_update(tr, g, before, rec[2], what=what)
        if l2:
            gaps.append(abs(bare - float(rec[0])) / (G.norm_rel(g.size) * bare))
    if l2:          # the regulariser's part is inside the norm: without it the record misses its bound many times over
        print("l2: |loss gradient's own norm - record| in bounds, per step", gaps)
        assert max(gaps) > 10, gaps
    assert abs(coefs[0] - 0.5) < 1e-3 and min(coefs) < 1.0, coefs
    assert float(tr.opt.state[0].item()) == 4


@pytest.mark.parametrize("kind,loss,dtype,opt", [("sas", "bce", "fp32", "adam"), ("sas", "bce", "fp32", "sgd"),
                                                 ("sas", "sampled_ce", "fp32", "adam"), ("sas", "ce", "bf16", "adam"),
                                                 ("bert", None, "bf16", "adam"), ("bert", "sampled_ce", "bf16", "sgd")])
def test_inf_measures_and_changes_nothing(kind, loss, dtype, opt):
    bs = [S._dev(b) for b in S._batches(kind, loss, 3)]
    m0, t0 = _mk(kind, loss, False, opt, dtype=dtype)
    m1, t1 = _mk(kind, loss, False, opt, dtype=dtype, max_grad_norm=INF)
    assert t0.grad_norm is None and t0.max_grad_norm is None
    for n, b in enumerate(bs):
        l0 = float(t0.step(*b).item())
        g = _bare_grad(t1, b) if n == 2 else None
        l1 = float(t1.step(*b).item())
        assert l0 == l1
    torch.cuda.synchronize()
    s0, s1 = _opt_state(t0), _opt_state(t1)
    for k in s0:
        assert R.same_bits(s0[k], s1[k]), k
    if t0.flat.bf16 is not None:
        assert torch.equal(t0.flat.bf16, t1.flat.bf16)
    rec = _check_record(t1, g, INF, f"inf {kind} {loss} {dtype} {opt}")
    assert rec[1] == 1.0 and rec[2] == 1.0


# ---------------------------------------------------------------- captured graphs
def _eager_vs_graph(kind, loss, dtype, opt, p=0.2, **kw):
    """capture (2 warm-up steps) + replay on 3 batches against 5 eager steps: parameters, optimizer state and every
    step's record bit for bit; then a new bound between replays.  Returns the eager twin's records."""
    bs = [S._dev(b) for b in S._batches(kind, loss, 4)]
    m, probe = _mk(kind, loss, False, opt, dtype=dtype, p=p, max_grad_norm=INF, **kw)
    mx = 0.5 * float(np.sqrt(float(G.sumsq(_bare_grad(probe, bs[0])))))
    runs = []
    for mode in ("eager", "graph"):
        m, tr = _mk(kind, loss, False, opt, dtype=dtype, p=p, max_grad_norm=mx, **kw)
        tr.engine.seed_base.fill_(77)
        if mode == "graph":
            tr.capture(*bs[0], warmup=2)
            f = tr.replay
        else:
            f = tr.step
            f(*bs[0])
            f(*bs[0])
        recs = []
        for b in bs[:3]:
            f(*b)
            recs.append(_record(tr).copy())
        tr.set_max_grad_norm(0.25 * mx)               # takes effect without re-capture
        f(*bs[3])
        recs.append(_record(tr).copy())
        torch.cuda.synchronize()
        runs.append((recs, _opt_state(tr)))
    (re, se), (rg, sg) = runs
    for a, b in zip(re, rg):
        assert R.same_bits(a, b), (a, b)
    for k in se:
        assert R.same_bits(se[k], sg[k]), k
    assert re[0][1] < 1.0, re
    # the new bound: the last step's coefficient is 0.25 mx / (its norm + 1e-6)
    want = min(1.0, 0.25 * mx / (float(re[3][0]) + 1e-6))
    assert abs(float(re[3][1]) - want) <= 4 * 2.0 ** -24 * want, (re[3], want)
    return re


@pytest.mark.parametrize("kind,loss,dtype,opt", [("sas", "bce", "fp32", "adam"), ("sas", "bce", "bf16", "sgd"),
                                                 ("bert", None, "bf16", "adam"), ("sas", "sampled_ce", "bf16", "adam")])
def test_captured_equals_eager(kind, loss, dtype, opt):
    _eager_vs_graph(kind, loss, dtype, opt)


@pytest.mark.parametrize("kind,loss", [("sas", "bce"), ("bert", None)])
def test_bf16_norm_is_the_norm_of_the_runs_own_gradient(kind, loss):
    m, tr = _mk(kind, loss, False, "adam", dtype="bf16", max_grad_norm=INF)
    mx = INF
    for n, hb in enumerate(S._batches(kind, loss, 3)):
        b = S._dev(hb)
        if n == 0:
            mx = 0.5 * float(np.sqrt(float(G.sumsq(_bare_grad(tr, b)))))
            tr.set_max_grad_norm(mx)
        g, before = _run_step(tr, b)
        rec = _check_record(tr, g, mx, f"bf16 {kind} step {n + 1}")
        _check_update(tr, g, before, rec[2], what=f"bf16 {kind} step {n + 1}")
        assert torch.equal(tr.flat.bf16, tr.flat.data.to(torch.bfloat16))


def test_two_unrolled_steps_clip_each_and_keep_the_last_norm():
    bs = [torch.stack(S._dev(b)) for b in S._batches("sas", "bce", 4)]
    m, probe = _mk("sas", "bce", False, "adam", dtype="bf16", p=0.2, max_grad_norm=INF)
    mx = 0.5 * float(np.sqrt(float(G.sumsq(_bare_grad(probe, tuple(bs[0].unbind(0)))))))
    m0, t0 = _mk("sas", "bce", False, "adam", dtype="bf16", p=0.2, max_grad_norm=mx)
    for _ in range(2):
        t0.step(*bs[0].unbind(0))
    want, recs = [], []
    for b in bs:
        want.append(float(t0.step(*b.unbind(0)).item()))
        recs.append(_record(t0).copy())
    m1, t1 = _mk("sas", "bce", False, "adam", dtype="bf16", p=0.2, max_grad_norm=mx)
    t1.capture(*bs[0].unbind(0), warmup=2, steps_per_graph=2)
    got = []
    for r in range(2):
        got += t1.replay_packed(torch.stack(bs[2 * r:2 * r + 2])).tolist()
        assert R.same_bits(_record(t1), recs[2 * r + 1])          # the last unrolled step's record
    torch.cuda.synchronize()
    assert got == want and recs[0][1] < 1.0
    s0, s1 = _opt_state(t0), _opt_state(t1)
    for k in s0:
        assert R.same_bits(s0[k], s1[k]), k
    assert float(t1.opt.state[0].item()) == 6


def test_capture_sampled_clips():
    import rbm_amd.data as synth
    from rbm_amd.dataloaders import DeviceWarpSampler
    hist = synth.user_histories(np.random.default_rng(3), 100, S.T, S.V)
    runs = []
    for mode in ("graph", "eager"):
        m, tr = _mk("sas", "bce", False, "adam", dtype="bf16", p=0.2, max_grad_norm=0.05)
        sampler = DeviceWarpSampler(hist, S.V, S.B, S.T, seed=9)
        recs = []
        if mode == "graph":
            tr.capture_sampled(sampler, warmup=2)
            for _ in range(3):
                tr.replay_sampled()
                recs.append(_record(tr).copy())
        else:
            static = list(torch.zeros((3, S.B, S.T), dtype=torch.int64, device="cuda").unbind(0))
            for k in range(5):
                sampler.sample_into(*static)
                tr.step(*static)
                if k >= 2:
                    recs.append(_record(tr).copy())
        torch.cuda.synchronize()
        runs.append((recs, _opt_state(tr)))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert R.same_bits(a, b), (a, b)
    for k in runs[0][1]:
        assert R.same_bits(runs[0][1][k], runs[1][1][k]), k
    assert all(r[1] < 1.0 and np.isfinite(r).all() for r in runs[0][0]), runs[0][0]
    assert len({float(r[0]) for r in runs[0][0]}) == 3


# ---------------------------------------------------------------- sparse tables
@pytest.mark.parametrize("kind,loss,dtype", [("sas", "bce", "fp32"), ("sas", "sampled_ce", "fp32"),
                                             ("bert", "sampled_ce", "bf16")])
def test_sparse_tables(kind, loss, dtype):
    """The row-list norm equals the norm of the whole gradient (what the dense mode reads) within the bound; untouched
    rows of p / m / v keep their bits; the touched ones and the rest take the clipped update."""
    import test_sparse_tables_gpu as ST
    m, tr = _mk(kind, loss, False, "adam", dtype=dtype, table_optim="sparse", max_grad_norm=INF)
    m2, dense = _mk(kind, loss, False, "adam", dtype=dtype, max_grad_norm=INF)
    mx = INF
    for n, hb in enumerate(S._batches(kind, loss, 3)):
        b = S._dev(hb)
        if n == 0:
            mx = 0.5 * float(np.sqrt(float(G.sumsq(_bare_grad(tr, b)))))
            tr.set_max_grad_norm(mx)
            dense.set_max_grad_norm(mx)
        g, before = _run_step(tr, b)
        what = f"sparse {kind} {loss} step {n + 1}"
        rec = _check_record(tr, g, mx, what)
        sets = ST.touched(tr, tr._batch(b))
        print(what, "touched rows", {k: (len(r), tr.flat.shapes[k][0]) for k, r in sets.items()})
        _check_update(tr, g, before, rec[2], touched=sets, what=what)
        if n == 0:      # the dense twin on the same weights and batch: the same gradient, its norm by the dense sweep
            gd, _ = _run_step(dense, b)
            assert R.same_bits(g, gd)
            rd = _record(dense)
            assert G.check_record(rd, G.reference(G.sumsq(g), mx), g.size) == []
            assert abs(float(rd[0]) - float(rec[0])) <= 2 * G.norm_rel(g.size) * float(rec[0])


# ---------------------------------------------------------------- the regimes the tiny shape misses
def _big(kind, V, L, dtype, **kw):
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    from rbm_amd.train_step import FusedTrainStep
    torch.manual_seed(5)
    if kind == "sas":
        a = argparse.Namespace(model_code="sas", num_items=V, max_len=S.T, device="cuda", sas_hidden_units=S.D,
                               sas_num_blocks=L, sas_heads=1, sas_dropout=0.0, l2_emb=0.0, rs_dtype=dtype)
    else:
        a = argparse.Namespace(model_code="bert", num_items=V, max_len=S.T, device="cuda", bert_hidden_units=S.D,
                               bert_num_blocks=L, bert_num_heads=2, bert_dropout=0.0, bert_hidden_dropout=0.0,
                               bert_mask_prob=0.2, model_init_seed=5, rs_dtype=dtype)
    m = model_factory(a)
    m.train()
    return m, FusedTrainStep(m, lr=1e-3, **kw)


def _big_batch(kind, V, seed):
    import rbm_amd.data as synth
    rng = np.random.default_rng(seed)
    hb = synth.sas_batch(rng, S.B, S.T, V) if kind == "sas" else synth.bert_batch(rng, S.B, S.T, V, 0.3)
    return S._dev(hb)


@pytest.mark.parametrize("kind,V,L", [("sas", 20000, 2), ("bert", 262200, 1)])
def test_row_marked_and_unzeroed_regimes(kind, V, L):
    """SAS at V = 20000 >= ROW_MARKS_MIN: the row-marked sweeps.  BERT full CE at V d >= 2^24: the `keep` range (the
    head gradient overwritten, never cleared) and no early update.  Two steps each, the second on a gradient buffer
    the first has swept: the norm against the float64 norm of the whole gradient, the clipped update restated."""
    m0, plain = _big(kind, V, L, "bf16")
    m, tr = _big(kind, V, L, "bf16", max_grad_norm=INF)
    if kind == "sas":
        assert tr.opt.marks is not None and plain.opt.marks is not None
    else:
        assert tr.engine.overwritten_grads() is not None and plain._early_ok and not tr._early_ok
    del m0, plain
    mx = INF
    for n in range(2):
        b = _big_batch(kind, V, n)
        if n == 0:
            mx = 0.5 * float(np.sqrt(float(G.sumsq(_bare_grad(tr, b)))))
            tr.set_max_grad_norm(mx)
        g, before = _run_step(tr, b)
        rec = _check_record(tr, g, mx, f"regime {kind} step {n + 1}")
        if n == 1:      # the step on a buffer the first has swept, and Adam's second
            assert rec[1] < 1.0
            _check_update(tr, g, before, rec[2], what=f"regime {kind} step {n + 1}")


# ---------------------------------------------------------------- refusals
def test_refusals_come_before_any_launch():
    from rbm_amd.train_step import FusedTrainStep
    m = S._model("sas")
    before = m.sas.item_emb.weight.detach().clone()
    for bad in (0, 0.0, -1.0, float("nan"), True, False, "1.0", [1.0]):
        with pytest.raises(ValueError, match="max_grad_norm"):
            FusedTrainStep(m, max_grad_norm=bad)
    with pytest.raises(ValueError, match="single device"):
        FusedTrainStep(m, max_grad_norm=1.0, dp=True)
    mb = S._model("bert")
    with pytest.raises(ValueError, match="single device"):
        FusedTrainStep(mb, max_grad_norm=1.0, vocab_shard=True)
    with pytest.raises(ValueError, match="single device"):
        FusedTrainStep(mb, max_grad_norm=1.0, dp=True, vocab_shard=True)
    assert torch.equal(before, m.sas.item_emb.weight.detach())
    m1, t1 = _mk("sas", "bce", max_grad_norm=1.0)
    for bad in (0, -2.0, float("nan"), True, None):
        with pytest.raises(ValueError):
            t1.set_max_grad_norm(bad)
    m2, t2 = _mk("sas", "bce")
    with pytest.raises(ValueError):
        t2.set_max_grad_norm(1.0)
    t1.set_max_grad_norm(3)
    assert float(t1._clip_max.item()) == 3.0 and t1.max_grad_norm == 3.0
