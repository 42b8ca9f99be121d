"""Popularity-drawn candidates and the logQ correction of the sampled softmax, on the GPU.

* ``rs_alias_items`` against its host restatement, bit for bit, and against ``rs_uniform_items`` on a uniform table;
* the two head launches with the correction (rs_sce_head_logq_fwd / _bwd) directly, every output element against the
  float64 reference under the derived bounds of tests/sce_logq_ref.py (its docstring has the derivation), outputs
  NaN-filled and guarded, with and without a bias, on every sweep width and the plain kernel; logq = NULL bitwise
  against the entries without the argument;
* ``sampled_ce_loss(..., logq=)`` of both models against the float64 reference: fp32 at the fp32 bars of the existing
  sampled-CE model tests, bf16 SASRec against the BF16Storage emulation (conftest's bf16 bars), bf16 BERT4Rec -- for
  which the oracle has no storage emulation -- against float64 at tests/test_bert.py's bf16 bars, as the existing
  sampled-CE BERT test does;
* ``FusedTrainStep(loss="sampled_ce", logq=)``: against sampled_ce_loss + the fused Adam, eager against captured,
  a proposal-carrying sampler's logq adopted by capture_sampled, reproducibility; the V-free workspace; the errors.
Each head test prints its worst error / bar per output (pytest -s).
"""
import math

import numpy as np
import pytest
import torch

import sce_logq_ref as ref
import test_bert_sce_gpu as tb
import test_sas_sce_gpu as ts
from conftest import check_bf16_grads, rel
from test_bert import FWD_TOL_BF16 as B_FWD_BF16, FWD_TOL_F32 as B_FWD_F32, GRAD_TOL_BF16 as B_GRAD_BF16, \
    GRAD_TOL_F32 as B_GRAD_F32
from test_sas_gpu import FWD_TOL_BF16, GRAD_TOL_F32, check_grads

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
GUARD = 8
SENT = -7


def _nan(shape, dt=F32):
    return torch.full(shape, math.nan, dtype=dt, device="cuda")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _zipf_weights(V, seed=0):
    w = 1.0 / np.arange(1, V + 1)
    return np.concatenate([[0.0], w[np.random.default_rng(seed).permutation(V)]])


def _proposal(V, seed=0, uniform=False):
    from rbm_amd.dataloaders import ItemProposal
    return ItemProposal(np.concatenate([[0.0], np.ones(V)]) if uniform else _zipf_weights(V, seed))


# ================================================================ rs_alias_items
@pytest.mark.parametrize("V", [1, 2, 63, 1000, 54542])
def test_alias_items_equal_the_host_restatement(V):
    from rbm_amd import ops
    P = _proposal(V, seed=V)
    table = P.table.cpu().numpy()
    for seed_base, salt in ((1, 1234), (2 ** 40 + 3, 2 ** 61 + 5)):
        sb = torch.tensor([seed_base], dtype=torch.int64, device="cuda")
        for K in (1, 255, 256, 257, 4096):
            out = torch.full((K + GUARD,), SENT, dtype=torch.int64, device="cuda")
            ops.alias_items(sb, salt, P.table, out[:K])
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert (got[K:] == SENT).all()
            assert got[:K].min() >= 1 and got[:K].max() <= V
            assert (got[:K] == ref.alias_items_ref(seed_base, salt, table, V, K)).all(), (V, K, seed_base)
        assert int(sb.item()) == seed_base                            # it advances nothing


@pytest.mark.parametrize("V", [1, 63, 54542])
def test_uniform_table_gives_rs_uniform_items_draws(V):
    from rbm_amd import ops
    P = _proposal(V, uniform=True)
    sb = torch.tensor([77], dtype=torch.int64, device="cuda")
    a, b = (torch.zeros(4096, dtype=torch.int64, device="cuda") for _ in range(2))
    ops.alias_items(sb, 991, P.table, a)
    ops.uniform_items(sb, 991, V, b)
    assert torch.equal(a, b)


def test_alias_items_is_graph_capturable():
    from rbm_amd import ops
    V, K = 1000, 300
    P = _proposal(V)
    sb = torch.tensor([5], dtype=torch.int64, device="cuda")
    out = torch.zeros(K, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ops.alias_items(sb, 17, P.table, out)                         # warm up outside the capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            ops.alias_items(sb, 17, P.table, out)
    torch.cuda.synchronize()
    for seed in (5, 6):                                               # the replay reads the seed's current value
        sb.fill_(seed)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == ref.alias_items_ref(seed, 17, P.table.cpu().numpy(), V, K)).all()


# ================================================================ the head kernels
def _run_head(dt, d, rows, K, pattern, kind, with_bias, count=None):
    from rbm_amd import ops
    V, cap, hl, E, bias, logq, lab, cand = ref.head_problem(dt, d, rows, K, pattern, kind, seed=d + rows + K)
    count = rows if count is None else count
    hl_d, E_d, lab_d, cand_d, q_d = hl.cuda(), E.cuda(), _dev(lab), _dev(cand), logq.cuda()
    b_d = bias.cuda() if with_bias else None
    b64 = bias.numpy() if with_bias else None
    cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
    nvalid = int(((lab[:count] > 0) & (lab[:count] <= V)).sum())
    div = torch.tensor([float(max(nvalid, 1))], device="cuda")
    dloss = torch.tensor([0.75], device="cuda")
    nws = ops.sce_head_ws_numel(cap, K, d, dt, with_bias)
    ws, out = _nan((nws + GUARD,)), _nan((4,))
    ops.sce_head_fwd(hl_d, lab_d, cnt, cap, E_d, b_d, cand_d, div, ws[:nws], out, logq=q_d)
    ks = ops.sce_head_dh_splits(cap, K, d, dt)
    dh, coef = _nan((ks * cap + GUARD, d)), _nan((cap + GUARD,))
    src, dbc = _nan((cap + K + GUARD, d)), _nan((K + GUARD,))
    keys = torch.full((cap + K + GUARD,), SENT, dtype=torch.int64, device="cuda")
    ops.sce_head_bwd(hl_d, lab_d, cnt, cap, E_d, b_d, cand_d, div, dloss, ws[:nws], dh, coef, src[:cap],
                     src[cap:cap + K], dbc[:K] if with_bias else None, keys, logq=q_d)
    torch.cuda.synchronize()
    bars = ref.head_bars(dt, ks, hl.double().numpy(), lab, count, E.double().numpy(), b64, logq.numpy(), cand,
                         float(div.item()), 0.75)
    got = dict(lse=ws[:count].double().cpu().numpy(), z0=ws[cap:cap + count].double().cpu().numpy(),
               dh=dh[:ks * cap].view(ks, cap, d)[:, :count].double().sum(0).cpu().numpy(),
               coef=coef[:count].double().cpu().numpy(), pg=src[:count].double().cpu().numpy(),
               dEc=src[cap:cap + K].double().cpu().numpy(), out=out[:3].double().cpu().numpy())
    if with_bias:
        got["dbc"] = dbc[:K].double().cpu().numpy()
    res = ref.worst(got, bars)
    assert set(res) == set(bars) - {"keys"}
    # rows at or past the count, and the guards: untouched
    assert torch.isnan(ws[count:cap]).all() and torch.isnan(ws[cap + count:2 * cap]).all() and torch.isnan(ws[nws:]).all()
    assert torch.isnan(dh[:ks * cap].view(ks, cap, d)[:, count:]).all() and torch.isnan(dh[ks * cap:]).all()
    assert torch.isnan(coef[count:]).all()
    assert torch.isnan(src[count:cap]).all() and torch.isnan(src[cap + K:]).all()
    assert torch.isnan(dbc[K:]).all() and (with_bias or torch.isnan(dbc).all())
    assert torch.isnan(out[3])
    k = keys.cpu().numpy()
    assert (k[:cap + K] == bars["keys"]).all() and (k[cap + K:] == SENT).all()
    return res, (ks, nws, lab[:count], cand, V)


def _check(tag, res):
    print(tag, "err/bar:", ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
    bad = {k: v for k, v in res.items() if v > 1.0}
    assert not bad, (tag, bad)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("dt,d", ref.HEAD_WIDTHS)
def test_head_kernels_with_the_correction(dt, d, with_bias):
    """HEAD_ROWS x HEAD_K (tests/sce_logq_ref.py), the patterns (mixed: duplicates, id 0, an accidental hit, ids out
    of range; hits: rows whose candidates are all dead; big: z - logq = 100) and the two tables (Zipf; one reaching
    -40) rotating over them.  logq[0] is NaN in every problem: it is never read."""
    from rbm_amd import ops
    seen_ks, seen_sp, dead_rows, past88 = set(), set(), 0, 0
    for rows, K, pattern, kind in ref.head_cases():
        res, (ks, nws, lab, cand, V) = _run_head(dt, d, rows, K, pattern, kind, with_bias)
        _check(f"head {dt} d={d} bias={with_bias} rows={rows} K={K} {pattern} {kind}", res)
        seen_ks.add(ks > 1)
        cap = rows + 9
        seen_sp.add(ops.sce_head_ws_numel(cap, K, d, dt, True) > ops.sce_head_ws_numel(cap, K, d, dt, False))
        ok = (lab > 0) & (lab <= V)
        cc = np.where((cand <= 0) | (cand > V), 0, cand)
        live = (cc != 0)[None, :] & (cc[None, :] != lab[:, None])
        dead_rows += int((ok & ~live.any(-1)).sum())
        past88 += pattern == "big"
    assert seen_ks == {False, True}, "no shape with several candidate splits (rs_sce_head_dh_splits > 1)"
    assert seen_sp == {False, True}, "no shape with several row splits of the dEc launch"
    assert dead_rows > 0 and past88 > 0


@pytest.mark.parametrize("dt,d", [(F32, 50), (BF, 128), (BF, 256), (F32, 136)])
def test_head_kernels_with_no_row(dt, d):
    """*count = 0: the loss triple and dEc / dbc are zero, the keys hold the candidates alone, no per-row output is
    written."""
    for with_bias in (False, True):
        res, _ = _run_head(dt, d, 17, 65, "mixed", "zipf", with_bias, count=0)
        assert not any(res.values()), res


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("dt,d", [(BF, 64), (BF, 128), (BF, 256), (F32, 50), (F32, 128), (F32, 136), (BF, 264)])
def test_null_logq_gives_the_bits_of_the_entries_without_it(dt, d, with_bias):
    """rs_sce_head_logq_* with logq = NULL against rs_sce_head_*: every output and the whole workspace."""
    import rbm_amd._lib as L
    from rbm_amd import ops
    lib = L.lib()
    rows, K = 130, 257
    V, cap, hl, E, bias, logq, lab, cand = ref.head_problem(dt, d, rows, K, "mixed", "zipf", seed=d)
    hl_d, E_d, lab_d, cand_d = hl.cuda(), E.cuda(), _dev(lab), _dev(cand)
    b_d = bias.cuda() if with_bias else None
    cnt = torch.tensor([rows], dtype=torch.int32, device="cuda")
    div, dloss = torch.tensor([float(rows)], device="cuda"), torch.tensor([0.75], device="cuda")
    nws = ops.sce_head_ws_numel(cap, K, d, dt, with_bias)
    ks = ops.sce_head_dh_splits(cap, K, d, dt)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    code = L.BF16 if dt == BF else L.F32
    res = []
    for new in (False, True):
        ws, out = _nan((nws,)), _nan((4,))
        dh, coef, src, dbc = _nan((ks * cap, d)), _nan((cap,)), _nan((cap + K, d)), _nan((K,))
        keys = torch.full((cap + K,), SENT, dtype=torch.int64, device="cuda")
        db = dbc if with_bias else None
        if new:
            assert lib.rs_sce_head_logq_fwd(code, cap, d, p(hl_d), d, p(lab_d), p(cnt), p(E_d), p(b_d), None, V + 1,
                                            p(cand_d), K, p(div), p(ws), p(out), st) == 0
            assert lib.rs_sce_head_logq_bwd(code, cap, d, p(hl_d), d, p(lab_d), p(cnt), p(E_d), p(b_d), None, V + 1,
                                            p(cand_d), K, p(div), p(dloss), p(ws), p(dh), p(coef), p(src),
                                            p(src[cap:]), p(db), p(keys), st) == 0
        else:
            ops.sce_head_fwd(hl_d, lab_d, cnt, cap, E_d, b_d, cand_d, div, ws, out)
            ops.sce_head_bwd(hl_d, lab_d, cnt, cap, E_d, b_d, cand_d, div, dloss, ws, dh, coef, src[:cap], src[cap:],
                             db, keys)
        torch.cuda.synchronize()
        res.append([t.view(torch.int32) if t.dtype == F32 else t for t in (ws, out, dh, coef, src, dbc, keys)])
    for name, a, b in zip(("ws", "out", "dh", "coef", "src", "dbc", "keys"), *res):
        assert torch.equal(a, b), name                                # bit patterns (NaN fill included)
    assert not torch.isnan(res[0][1].view(F32)[:3]).any()


# ================================================================ the models
def _logq(V, seed=3):
    """(float64 [V + 1] on the host, the proposal's fp32 tensor on the device) of a Zipf proposal over V items."""
    P = _proposal(V, seed)
    return P.logq.double().cpu().numpy(), P.logq


SAS_SHAPE = (60, 16, 32, 2, 1, 4)


@pytest.mark.parametrize("K", [1, 50])
def test_sas_sampled_ce_loss_with_logq_fp32(K):
    V, T, d, L, h, B = SAS_SHAPE
    m = ts._model(V, T, d, L, h)
    seq, pos = ts._batch(V, T, B)
    cand = ts._cand(V, K)
    q64, q = _logq(V)
    m.zero_grad(set_to_none=True)
    loss = m.sampled_ce_loss(seq.numpy(), pos, cand, logq=q)
    loss.backward()
    torch.cuda.synchronize()
    loss, grads = float(loss.item()), {k: v.grad.detach().cpu().numpy() for k, v in m.named_parameters()}
    l64, g64 = ref.loss_and_grads(ref.sas_sce_loss, ts._P(m), seq, pos, cand, q64, L, h)
    plain = ts.ref.sce_loss(ts._P(m), seq, pos, cand, L, h).item()
    print((V, T, d, K), "loss", loss, "ref", l64.item(), "uncorrected", plain)
    assert abs(l64.item() - plain) > 1e-3                              # the correction is no rounding matter here
    assert abs(loss - l64.item()) < 1e-5 * max(1.0, abs(l64.item())), (loss, l64.item())
    r = {k: g64[k].numpy() for k in grads}
    check_grads(grads, r, d, GRAD_TOL_F32, max(np.linalg.norm(v) for v in r.values()))
    assert not grads["sas.item_emb.weight"][0].any()


@pytest.mark.parametrize("V,T,d,L,h,B", [SAS_SHAPE, (60, 16, 64, 2, 1, 4)])
def test_sas_sampled_ce_loss_with_logq_bf16_matches_the_storage_emulation(V, T, d, L, h, B):
    """d = 32 (the unfused blocks) and d = 64 (the fused row chains): every gradient against the BF16Storage
    emulation and the exact reference under conftest's bf16 bars."""
    from oracle import sas as osas
    m = ts._model(V, T, d, L, h, dtype="bf16", scale_items=0.1)
    seq, pos = ts._batch(V, T, B)
    cand = ts._cand(V, 50)
    q64, q = _logq(V)
    m.zero_grad(set_to_none=True)
    loss = m.sampled_ce_loss(seq, pos, cand, logq=q)
    loss.backward()
    torch.cuda.synchronize()
    loss, grads = float(loss.item()), {k: v.grad.detach().cpu().numpy() for k, v in m.named_parameters()}
    P = ts._P(m)
    le, ge = ref.loss_and_grads(ref.sas_sce_loss, P, seq, pos, cand, q64, L, h, emu=osas.BF16Storage())
    l64, g64 = ref.loss_and_grads(ref.sas_sce_loss, P, seq, pos, cand, q64, L, h)
    print((V, T, d), "loss", loss, "emulation", le.item(), "exact", l64.item())
    assert abs(loss - l64.item()) < FWD_TOL_BF16 * max(1.0, abs(l64.item())), (loss, l64.item())
    res = check_bf16_grads(lambda n: grads[n], ge, g64, d, kbias=lambda n: n.endswith("in_proj_bias"))
    print((V, T, d), "worst vs emulation", max(res.items(), key=lambda kv: kv[1][0]))
    assert not grads["sas.item_emb.weight"][0].any()


BERT_SHAPE = (50, 16, 64, 2, 2, 4)                                     # the bert_tiny golden's dimensions


@pytest.mark.parametrize("K", [1, 50])
def test_bert_sampled_ce_loss_with_logq_fp32(K):
    V, T, d, L, h, B = BERT_SHAPE
    m = tb._model(V, T, d, L, h)
    tok, lab = tb._batch(V, T, B)
    cand = tb._cand(V, K)
    q64, q = _logq(V)
    m.zero_grad(set_to_none=True)
    loss = m.sampled_ce_loss(tok.numpy(), lab, cand, logq=q)
    loss.backward()
    torch.cuda.synchronize()
    loss, grads = float(loss.item()), {k: v.grad.detach().cpu().numpy() for k, v in m.named_parameters()}
    l64, g64 = ref.loss_and_grads(ref.bert_sce_loss, tb._P(m), tok, lab, cand, q64, L, h)
    plain = tb.ref.sce_loss(tb._P(m), tok, lab, cand, L, h).item()
    print((V, T, d, K), "loss", loss, "ref", l64.item(), "uncorrected", plain)
    assert abs(l64.item() - plain) > 1e-3
    assert abs(loss - l64.item()) < B_FWD_F32 * max(1.0, abs(l64.item())), (loss, l64.item())
    tb._check_grads_f32(grads, g64, B_GRAD_F32)
    touched = set(lab.reshape(-1).tolist()) | set(cand.tolist())
    rest = [v for v in range(V + 1) if v not in touched or v == 0]
    assert not grads["out.weight"][rest].any() and not grads["out.bias"][rest].any()


def test_bert_fused_bf16_step_with_logq_matches_float64_reference():
    from rbm_amd.train_step import FusedTrainStep
    V, T, d, L, h, B = BERT_SHAPE
    m = tb._model(V, T, d, L, h, dtype="bf16", seed=1)
    tok, lab = tb._batch(V, T, B)
    cand = tb._cand(V, 50)
    q64, q = _logq(V)
    tr = FusedTrainStep(m, lr=0.0, loss="sampled_ce", logq=q)
    tr.flat.grad.zero_()
    tr._compute(tok.cuda(), lab.cuda(), cand.cuda())
    torch.cuda.synchronize()
    loss = float(tr.loss_out[2].item())
    l64, g64 = ref.loss_and_grads(ref.bert_sce_loss, tb._P(m), tok, lab, cand, q64, L, h)
    scale = max(float(g.norm()) for g in g64.values())
    worst = {}
    for k, r in g64.items():
        g = tr.flat.view(k, tr.flat.grad).cpu().double()
        if "linear_layers.1.bias" in k:
            assert float(g.norm()) <= 1e-2 * scale, k
            continue
        worst[k] = rel(g.numpy(), r.numpy())
    print("loss", loss, "ref", l64.item(), "worst", max(worst.items(), key=lambda kv: kv[1]))
    assert abs(loss - l64.item()) < B_FWD_BF16 * abs(l64.item()), (loss, l64.item())
    bad = {k: v for k, v in worst.items() if v >= B_GRAD_BF16}
    assert not bad, bad


# ================================================================ the fused step
def _step(kind, logq, **kw):
    mod = ts if kind == "sas" else tb
    return mod._step_model(logq=logq, **kw)


def _step_V(kind):
    return (ts.STEP if kind == "sas" else tb.STEP)[0]


@pytest.mark.parametrize("kind", ["sas", "bert"])
def test_fused_step_equals_sampled_ce_loss_with_logq_plus_fused_adam_bit_for_bit(kind):
    mod = ts if kind == "sas" else tb
    _, q = _logq(_step_V(kind))
    b = mod._step_batches(1)[0]
    m1, t1 = _step(kind, q)
    m2, t2 = _step(kind, q)
    m3, t3 = _step(kind, False)
    for t in (t1, t2, t3):
        t.engine.seed_base.fill_(77)
    l1 = float(t1.step(*b).item())
    loss = m2.sampled_ce_loss(*b, logq=q)
    loss.backward()
    for n, p in (m2.sas if kind == "sas" else m2).named_parameters():
        t2.flat.view(n, t2.flat.grad).copy_(p.grad)
    t2._update()
    l3 = float(t3.step(*b).item())
    torch.cuda.synchronize()
    assert l1 == float(loss.item()) and np.isfinite(l1)
    assert torch.equal(t1.flat.data, t2.flat.data)
    assert l3 != l1 and not torch.equal(t1.flat.data, t3.flat.data)   # logq=False: the uncorrected step


@pytest.mark.parametrize("kind", ["sas", "bert"])
def test_captured_replays_with_logq_equal_eager_steps(kind):
    mod = ts if kind == "sas" else tb
    _, q = _logq(_step_V(kind))
    bs = mod._step_batches(3)
    m0, t0 = _step(kind, q)
    for b in bs[:1] * 2:                                              # the capture's two warmup steps
        t0.step(*b)
    want = [float(t0.step(*b).item()) for b in bs]
    m1, t1 = _step(kind, q)
    t1.capture(*bs[0], warmup=2)
    got = [float(t1.replay(*b).item()) for b in bs]
    torch.cuda.synchronize()
    assert got == want and all(np.isfinite(want)), (got, want)
    assert torch.equal(t0.flat.data, t1.flat.data)


def _sampler(kind, V, B, T, K, proposal, seed=9):
    import rbm_amd.data as synth
    from rbm_amd.dataloaders import DeviceBertMasker, DeviceWarpSampler
    hist = synth.user_histories(np.random.default_rng(3), 100, T, V)
    if kind == "sas":
        return DeviceWarpSampler(hist, V, B, T, seed=seed, shared_negs=K, proposal=proposal)
    return DeviceBertMasker(hist, V, B, T, 0.3, seed=seed, shared_negs=K, proposal=proposal)


@pytest.mark.parametrize("kind", ["sas", "bert"])
def test_capture_sampled_adopts_the_proposals_logq(kind):
    """None adopts sampler.proposal.logq (the same bits as handing that tensor over), False never corrects (another
    loss on the same replayed batch), and two runs replay the same losses."""
    mod = ts if kind == "sas" else tb
    V, T, d, L, h, B = mod.STEP
    P = _proposal(V, seed=4)
    runs = {}
    for name, logq in (("adopted", None), ("again", None), ("given", P.logq), ("off", False)):
        m, t = _step(kind, logq)
        assert t.logq is (P.logq if name == "given" else None)
        s = _sampler(kind, V, B, T, mod.K_STEP, P)
        t.capture_sampled(s, warmup=2)
        assert t.logq is (None if name == "off" else P.logq)
        losses = [float(t.replay_sampled().item()) for _ in range(3)]
        torch.cuda.synchronize()
        seed = int((s.seed_base if kind == "sas" else s.state)[0].item())     # the step seed the last replay left
        cand = t.static[2].cpu().numpy()
        assert (cand == ref.alias_items_ref(seed, s.cand_salt, P.table.cpu().numpy(), V, mod.K_STEP)).all()
        runs[name] = (losses, t.flat.data.clone())
    assert runs["adopted"][0] == runs["again"][0] == runs["given"][0] and all(np.isfinite(runs["adopted"][0]))
    assert torch.equal(runs["adopted"][1], runs["again"][1]) and torch.equal(runs["adopted"][1], runs["given"][1])
    assert len(set(runs["adopted"][0])) == 3                          # fresh batches and candidates every replay
    assert all(a != b for a, b in zip(runs["adopted"][0], runs["off"][0]))


def test_a_sampler_without_a_proposal_leaves_the_step_uncorrected():
    V, T, d, L, h, B = ts.STEP
    m, t = ts._step_model()
    t.capture_sampled(ts._sampler(V, B, T, ts.K_STEP), warmup=1)
    assert t.logq is None


# ================================================================ memory, errors
@pytest.mark.parametrize("kind", ["sas", "bert"])
def test_workspace_is_not_shaped_by_the_catalogue_with_a_proposal(kind):
    T, d, L, h, B, K = 16, 64, 1, 2, 8, 100
    sizes = {}
    for V in (1000, 50000):
        P = _proposal(V)
        rng = np.random.default_rng(0)
        a = torch.from_numpy(rng.integers(1, 1001, (B, T)))
        lab = torch.from_numpy(np.where(rng.random((B, T)) < 0.3, rng.integers(1, 1001, (B, T)), 0))
        cand = torch.from_numpy(rng.integers(1, 1001, K))
        if kind == "sas":
            m = ts._model(V, T, d, L, h, dtype="bf16")
            eng = m.sas.engine()
        else:
            m = tb._model(V, T, d, L, h, dtype="bf16")
            eng = m.engine()
        loss = m.sampled_ce_loss(a, lab, cand, logq=P.logq)
        loss.backward()
        torch.cuda.synchronize()
        assert np.isfinite(float(loss.item()))
        sizes[V] = {k: (tuple(v.shape), v.numel() * v.element_size()) for k, v in eng.ws.bufs.items()
                    if k.startswith("sce_")}
        assert {"sce_ws", "sce_dh", "sce_src", "sce_keys", "sce_itemidx"} <= set(sizes[V])
    print(kind, "sce_* bytes", {V: sum(b for _, b in s.values()) for V, s in sizes.items()})
    assert sizes[1000] == sizes[50000]


def test_errors():
    import rbm_amd._lib as L
    from rbm_amd import ops
    from rbm_amd.train_step import FusedTrainStep
    lib = L.lib()
    st = torch.cuda.current_stream().cuda_stream
    # rs_alias_items: RS_ERR_ARG, nothing launched
    out = torch.full((16,), SENT, dtype=torch.int64, device="cuda")
    table = _proposal(5).table
    sb = torch.zeros(1, dtype=torch.int64, device="cuda")
    for item_num, K, tab, o in ((0, 4, table, out), (5, 0, table, out), (-1, 4, table, out), (5, -2, table, out),
                                (5, 4, None, out), (5, 4, table, None)):
        assert lib.rs_alias_items(sb.data_ptr(), 3, None if tab is None else tab.data_ptr(), item_num, K,
                                  None if o is None else o.data_ptr(), st) == 1001
    torch.cuda.synchronize()
    assert (out == SENT).all()
    # the models: a logq of another shape, dtype or device
    V, T, d, Lb, h, B = ts.STEP
    m = ts._model(V, T, d, Lb, h, dtype="bf16")
    seq, pos = ts._batch(V, T, B)
    cand = ts._cand(V, 8)
    for bad in (torch.zeros(V, device="cuda"), torch.zeros(V + 1, dtype=torch.float64, device="cuda"),
                torch.zeros(V + 1), torch.zeros(2 * (V + 1), device="cuda")[::2]):
        with pytest.raises(ValueError, match="logq"):
            m.sampled_ce_loss(seq, pos, cand, logq=bad)
    Vb, Tb, db, L2, hb, Bb = tb.STEP
    mb = tb._model(Vb, Tb, db, L2, hb, dtype="bf16")
    tok, lab = tb._batch(Vb, Tb, Bb)
    with pytest.raises(ValueError, match="logq"):
        mb.sampled_ce_loss(tok, lab, tb._cand(Vb, 8), logq=torch.zeros(Vb, device="cuda"))
    # the step: logq with another loss; a value that is neither a tensor, False nor None
    q = torch.zeros(V + 1, device="cuda")
    with pytest.raises(ValueError, match="sampled_ce"):
        FusedTrainStep(m, loss="bce", logq=q)
    with pytest.raises(ValueError, match="sampled_ce"):
        FusedTrainStep(m, loss="ce", logq=q)
    with pytest.raises(ValueError, match="sampled_ce"):
        FusedTrainStep(mb, logq=torch.zeros(Vb + 1, device="cuda"))
    with pytest.raises(ValueError, match="logq"):
        FusedTrainStep(m, loss="sampled_ce", logq=True)
    assert FusedTrainStep(m, loss="bce", logq=False).logq is None
    # the samplers
    from rbm_amd.dataloaders import DeviceBertMasker, DeviceWarpSampler
    hist = [[1, 2, 3], [2, 4]]
    P = _proposal(5)
    with pytest.raises(ValueError, match="shared_negs"):
        DeviceWarpSampler(hist, 5, 2, 4, proposal=P)
    with pytest.raises(ValueError, match="item_num"):
        DeviceWarpSampler(hist, 6, 2, 4, shared_negs=4, proposal=P)
    with pytest.raises(ValueError, match="shared_negs"):
        DeviceBertMasker(hist, 5, 2, 4, 0.2, proposal=P)
    with pytest.raises(ValueError, match="item_num"):
        DeviceBertMasker(hist, 4, 2, 4, 0.2, shared_negs=4, proposal=P)
    assert DeviceWarpSampler(hist, 5, 2, 4, shared_negs=4, proposal=P).proposal is P
    # ops: the fp32 / shape / contiguity check of logq
    with pytest.raises(AssertionError):
        ops._sce_head_logq(torch.zeros(7, device="cuda"), torch.zeros(6, 8, device="cuda"))
