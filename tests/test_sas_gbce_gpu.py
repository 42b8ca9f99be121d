"""SASRec training with N negatives per position and the gBCE loss, on the GPU.

* the two head launches of sas_gbce.hip directly (rs_sas_gbce_fwd / rs_sas_gbce_bwd) and rs_item_grad_weighted, every
  output element against float64 on the kernels' own inputs (tests/sas_gbce_ref.py) under the derived bounds stated
  there (rowchain_ref.bound_f32), outputs pre-filled with NaN / a sentinel and followed by guard rows;
* rs_sas_sample_negs against rs_sas_sample (bit for bit at j = 0) and the host restatement of its counter rule;
* ``SASModel.gbce_loss`` + autograd: the reference's golden at N = 1, beta = 1; fp32 against float64; the bf16 fused
  path against the bf16-storage emulation (dropout masks replayed);
* ``FusedTrainStep(loss="gbce")``: against gbce_loss + the fused Adam (bit for bit), graph capture against eager steps
  (bit for bit), reproducibility, a sampler with negs=N captured with the step, sparse tables, SGD, clipping, l2_emb;
* the all-padding batch and every refusal.
Each head test prints its worst error / bound per output (pytest -s)."""
import math

import numpy as np
import pytest
import torch

import sas_gbce_ref as ref
from conftest import check_bf16_grads, load_golden, rel
from test_sas_ce_gpu import BF16_STEP_SEED, _batch, _P, _rule_batch
from test_sas_gpu import FWD_TOL_BF16, FWD_TOL_F32, GRAD_TOL_F32, check_grads, make_model, sas_args

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
GUARD = 8
SENT = -777
G = ref.IDS_PER_PASS         # ids per wave pass of the head kernels


def _nan(shape, dt=F32):
    return torch.full(shape, math.nan, dtype=dt, device="cuda")


# ================================================================ the head kernels
def _run_head(inp):
    """Both launches on one case of sas_gbce_ref.head_inputs; returns check_head's ratios."""
    from rbm_amd import ops
    cap, N, d, count = inp["cap"], inp["N"], inp["d"], inp["count"]
    hl = inp["hl"].cuda()[:, :d]                                  # rows of stride ldh (wider than d where given)
    E, lab, neg = inp["E"].cuda(), inp["lab"].cuda(), inp["neg"].cuda().contiguous()
    idx = None if inp["idx"] is None else inp["idx"].cuda()
    cnt = None if inp["dense"] else torch.tensor([count], dtype=torch.int32, device="cuda")
    div = torch.tensor([inp["divisor"]], device="cuda")
    dloss = None if inp["dloss"] is None else torch.tensor([inp["dloss"]], device="cuda")
    nws = ops.sas_gbce_ws_numel(cap, N, d)
    ws, out = _nan((nws + GUARD,)), _nan((4,))
    ops.sas_gbce_fwd(hl, lab, idx, cnt, cap, E, neg, N, inp["beta"], div, ws[:nws], out)
    n1 = cap * (1 + N)
    dh, w = _nan((cap + GUARD, d)), _nan((n1 + GUARD,))
    keys = torch.full((n1 + GUARD,), SENT, dtype=torch.int64, device="cuda")
    ops.sas_gbce_bwd(hl, lab, idx, cnt, cap, E, neg, N, inp["beta"], div, dloss, ws[:nws], dh[:cap], w[:n1], keys[:n1])
    torch.cuda.synchronize()
    off = -(-4 * n1 // 16) * 16                                   # the partials: doubles after the logits
    nwg = -(-cap // ref.ROWS_PER_WG)
    parts = ws.view(torch.uint8)[off:off + 24 * nwg].view(torch.float64).view(nwg, 3).cpu()
    assert torch.isnan(ws[nws:]).all() and torch.isnan(dh[cap:]).all() and torch.isnan(w[n1:]).all()
    assert (keys[n1:] == SENT).all()
    assert torch.isnan(ws[n1:off // 4]).all()                     # the alignment gap between the two regions
    o = dict(z=ws[:n1].view(cap, 1 + N).cpu(), out=out.cpu(), parts=parts, w=w[:n1].view(cap, 1 + N).cpu(),
             dh=dh[:cap].cpu(), keys=keys[:n1].cpu())
    assert not torch.isnan(o["out"]).any() and not torch.isnan(parts).any()
    return ref.check_head(inp, o)


def _check(tag, res):
    print(tag, "err/bound:", ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
    bad = {k: v for k, v in res.items() if v > 1.0}
    assert not bad, (tag, bad)


CAPS = [1, 63, 65, 209]
NS = sorted({1, 3, 4, 5, 67, 256, G - 1, G, G + 1})


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("dt,d", [(BF, 64), (BF, 128), (BF, 256), (F32, 64), (F32, 128), (F32, 256)])
def test_head_kernels(dt, d, cap, N):
    """count in {0, 1, cap - 1, cap}, beta in {1, 0.07} (both betas at every count), V = 41, ~30 % id-0 negatives,
    ids > V and < 0 among them."""
    for count in sorted({0, 1, cap - 1, cap}):
        for beta in (1.0, 0.07):
            inp = ref.head_inputs(cap, N, d, dt, count, beta=beta)
            _check(f"head {dt} d={d} cap={cap} N={N} count={count} beta={beta}", _run_head(inp))


@pytest.mark.parametrize("N", [1, 5, 67])
@pytest.mark.parametrize("cap", [1, 63, 209])
def test_head_kernels_fp32_d50_dense_rows(cap, N):
    """d = 50 in fp32 with idx = NULL and count = NULL: every row is given, lab 0 marks no row (zeros written)."""
    for beta in (1.0, 0.07):
        inp = ref.head_inputs(cap, N, 50, F32, cap, beta=beta, dense=True)
        _check(f"head dense d=50 cap={cap} N={N} beta={beta}", _run_head(inp))


@pytest.mark.parametrize("dt,d", [(BF, 64), (F32, 128), (BF, 256), (F32, 50)])
def test_head_kernels_large_logits_dloss_and_wide_rows(dt, d):
    dense = d == 50
    big = ref.head_inputs(65, 5, d, dt, 65 if dense else 64, big=True, dense=dense, beta=0.07)
    zmax = float(ref.head_ref(big)["z"].abs().max())
    print("largest |z|", zmax)
    assert zmax > 60                                              # exp(|z|) alone would overflow a naive softplus' square
    _check(f"head big d={d}", _run_head(big))
    _check(f"head dloss d={d}", _run_head(ref.head_inputs(63, 4, d, dt, 63 if dense else 62, dloss=0.75, dense=dense)))
    if not dense:                                                 # a row pitch wider than the row (16-byte multiple)
        _check(f"head ldh d={d}", _run_head(ref.head_inputs(63, 3, d, dt, 62, ldh=d + 16)))


@pytest.mark.parametrize("dt,d", [(F32, 1024), (BF, 1024), (F32, 130), (BF, 136), (BF, 512)])
def test_head_kernels_other_widths(dt, d):
    _check(f"head wide d={d}", _run_head(ref.head_inputs(9, 5, d, dt, 8, beta=0.07)))


def test_head_kernels_unsupported_launch_nothing():
    import rbm_amd._lib as L
    lib = L.lib()
    s = torch.cuda.current_stream().cuda_stream

    def codes(dtype, d, tdt, N, Nbuf=None):
        cap = 8
        nb = Nbuf or max(N, 1)
        hl, E = torch.zeros(cap, d, dtype=tdt, device="cuda"), torch.zeros(20, d, dtype=tdt, device="cuda")
        lab = torch.ones(cap, dtype=torch.int64, device="cuda")
        neg = torch.ones(cap * nb, dtype=torch.int64, device="cuda")
        div = torch.ones(1, device="cuda")
        ws, out = _nan((4096,)), _nan((4,))
        dh, w = _nan((cap, d)), _nan((cap * (1 + nb),))
        keys = torch.full((cap * (1 + nb),), SENT, dtype=torch.int64, device="cuda")
        p = lambda t: t.data_ptr()  # noqa: E731
        a = lib.rs_sas_gbce_fwd(dtype, cap, d, p(hl), d, p(lab), None, None, p(E), 20, p(neg), N, 1.0, p(div), p(ws),
                                p(out), s)
        b = lib.rs_sas_gbce_bwd(dtype, cap, d, p(hl), d, p(lab), None, None, p(E), 20, p(neg), N, 1.0, p(div), None,
                                p(ws), p(dh), p(w), p(keys), s)
        torch.cuda.synchronize()
        for t in (ws, out, dh, w):
            assert torch.isnan(t).all()
        assert (keys == SENT).all()
        return a, b
    assert codes(7, 64, F32, 4) == (1002, 1002)                   # no such dtype
    assert codes(L.BF16, 50, BF, 4) == (1002, 1002)               # bf16 rows that are no multiple of 16 bytes
    assert codes(L.BF16, 1032, BF, 4) == (1002, 1002)
    assert codes(L.F32, 1025, F32, 4) == (1002, 1002)
    assert codes(L.BF16, 64, BF, 0) == (1002, 1002)
    assert codes(L.BF16, 64, BF, 1025, Nbuf=4) == (1002, 1002)


# ================================================================ rs_item_grad_weighted
def _run_weighted(inp):
    from rbm_amd import ops
    rows, per, d, R = inp["rows"], inp["per"], inp["d"], inp["table_rows"]
    keys, w, f = inp["keys"].cuda(), inp["w"].cuda(), inp["f"].cuda()
    iws = torch.zeros(ops.item_index_ws_bytes(1, rows * per, R, d), dtype=torch.uint8, device="cuda")
    outs = []
    for _ in range(2):
        t = torch.cat([inp["dtable0"], torch.full((GUARD, d), math.nan)]).cuda()
        ops.item_index_build([keys], R, d, iws)
        ops.item_grad_weighted(iws, rows, per, f, w, t[:R], table_rows=R)
        torch.cuda.synchronize()
        assert torch.isnan(t[R:]).all()
        outs.append(t[:R].cpu())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two runs differ in their bits"
    path = ops.item_index_view(1, rows * per, R, d, iws)[3]
    return ref.check_weighted(inp, outs[0]), path


@pytest.mark.parametrize("dt,d", [(F32, 64), (BF, 128), (F32, 50), (BF, 256)])
@pytest.mark.parametrize("table_rows", [41, 40000])
@pytest.mark.parametrize("rows,per,hot,edge", [(5000, 1, 0.7, False), (2500, 2, 0.7, False), (20, 258, 0.7, False),
                                               (64, 4, 0.0, True), (37, 2, 0.0, False)])
def test_item_grad_weighted(dt, d, table_rows, rows, per, hot, edge):
    """5,000 entries with one key owning 70 % (its run crosses ~100 chunks), runs ending exactly on a chunk edge, key 0
    present, per in {1, 2, 258}, a non-zero table (41 rows), the counting sort (41 rows) and the radix path (40,000),
    bf16 and fp32 f, two runs bit-identical."""
    inp = ref.weighted_inputs(rows, per, d, dt, table_rows, hot=hot, edge=edge)
    res, path = _run_weighted(inp)
    assert path == (0 if table_rows == 41 else 3)
    _check(f"weighted {dt} d={d} R={table_rows} rows={rows} per={per}", res)


# ================================================================ the sampler
def _histories(n_users=9, item_num=30, seed=2):
    rng = np.random.default_rng(seed)
    return [list(rng.permutation(np.arange(1, item_num + 1))[:int(rng.integers(2, 26))]) for _ in range(n_users)]


@pytest.mark.parametrize("N", [1, 3])
def test_sampler_negs(N):
    from rbm_amd.dataloaders import DeviceWarpSampler
    B, T, V = 5, 7, 30
    hist = _histories()
    s, plain = DeviceWarpSampler(hist, V, B, T, seed=4, negs=N), DeviceWarpSampler(hist, V, B, T, seed=4)
    assert s.n_outputs == 3 and s.salt == plain.salt
    for k in range(3):
        seq, pos, neg = s.sample()
        q = plain.sample()
        assert neg.shape == (B, T, N) and neg.dtype == torch.int64
        assert torch.equal(seq, q[0]) and torch.equal(pos, q[1]) and torch.equal(neg[:, :, 0], q[2])
        rs, rp, rn = ref.sample_negs_ref(hist, V, B, T, N, k + 1, s.salt)      # the step seed after k + 1 advances
        assert (seq.cpu().numpy() == rs).all() and (pos.cpu().numpy() == rp).all()
        assert (neg.cpu().numpy() == rn).all()
        sq, ps, ng = seq.cpu().numpy(), pos.cpu().numpy(), neg.cpu().numpy()
        pad = ps == 0
        assert (ng[pad] == 0).all() and pad.any()
        for b in range(B):
            win = set(sq[b][sq[b] != 0]) | set(ps[b][ps[b] != 0])
            assert not (set(ng[b][~pad[b]].reshape(-1)) & win)
    with pytest.raises(ValueError):
        s.sample_into(seq, pos, torch.zeros(B, T, dtype=torch.int64, device="cuda") if N > 1 else
                      torch.zeros(B, T, 2, dtype=torch.int64, device="cuda"))


# ================================================================ the model
def _gmodel(V, T, d, L, h, N, p=0.0, dtype="fp32", seed=None, l2=0.0, scale_items=None, t=0.0):
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    torch.manual_seed(V + T if seed is None else seed)
    a = sas_args(V, T, d, L, h, p=p, dtype=dtype)
    a.l2_emb, a.sas_loss, a.sas_negs, a.sas_gbce_t = l2, "gbce", N, t
    m = model_factory(a)
    if scale_items is not None:
        with torch.no_grad():
            m.sas.item_emb.weight.mul_(scale_items)
    m.train()
    return m


def _negs(V, B, T, N, seed=0):
    """(B, T, N) with id 0, duplicates and ids equal to a positive among them"""
    rng = np.random.default_rng(seed + N)
    neg = rng.integers(1, V + 1, (B, T, N))
    neg[rng.random((B, T, N)) < 0.2] = 0
    neg[:, :, -1] = neg[:, :, 0]
    neg[-1, -1, 0] = V                                             # _batch forces the label V in there
    return torch.from_numpy(neg)


def _autograd_step(m, seq, pos, neg, beta):
    m.zero_grad(set_to_none=True)
    loss = m.gbce_loss(seq.numpy(), pos, neg, beta=beta)         # numpy and tensor ids
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.item()), {k: q.grad.detach().cpu().numpy() for k, q in m.named_parameters()}


def test_one_negative_beta_one_reproduces_the_reference_golden_fp32():
    """sas_tiny.npz: the reference-generated loss and gradients, under the tolerances tests/test_sas_gpu.py applies to
    forward + BCE on that golden."""
    z = load_golden("sas_tiny")
    m = make_model(z, "fp32")
    m.train()
    seq, pos, neg = (torch.from_numpy(z[k]) for k in ("seq", "pos", "neg"))
    loss, grads = _autograd_step(m, seq, pos, neg[..., None], 1.0)
    assert abs(loss - float(z["loss"])) < FWD_TOL_F32 * max(1.0, abs(float(z["loss"])))
    r = {k: z["g/sas." + k[4:]] if k.startswith("sas.") else z["g/" + k] for k in grads}
    check_grads(grads, r, int(z["d"]), GRAD_TOL_F32, max(np.linalg.norm(v) for v in r.values()))
    l2, g2 = _autograd_step(m, seq, pos, neg, 1.0)                # (B, T) is N = 1: the same launches
    assert l2 == loss and all(np.array_equal(grads[k], g2[k]) for k in grads)


@pytest.mark.parametrize("N", [3, 17])
@pytest.mark.parametrize("V,T,d,L,h,B", [(50, 16, 32, 2, 2, 4), (50, 16, 50, 2, 2, 4)])
def test_gbce_loss_fp32_matches_float64_reference(V, T, d, L, h, B, N):
    m = _gmodel(V, T, d, L, h, N)
    seq, pos = _batch(V, T, B)
    neg = _negs(V, B, T, N)
    loss, grads = _autograd_step(m, seq, pos, neg, 0.3)
    l64, g64 = ref.gbce_loss_and_grads(_P(m), seq, pos, neg, 0.3, L, h)
    print((V, T, d, N), "loss", loss, "ref", l64.item())
    assert abs(loss - l64.item()) < 1e-5 * max(1.0, abs(l64.item())), (loss, l64.item())
    r = {k: g64[k].numpy() for k in grads}
    print((V, T, d, N), "worst gradient errors", sorted(((rel(grads[k], r[k]), k) for k in grads
                                                         if not k.endswith("in_proj_bias")), reverse=True)[:3])
    check_grads(grads, r, d, GRAD_TOL_F32, max(np.linalg.norm(v) for v in r.values()))
    assert not grads["sas.item_emb.weight"][0].any()


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("V,T,d,L,h,B", [(60, 16, 64, 2, 1, 4), (127, 16, 128, 1, 1, 2)])
def test_gbce_loss_bf16_fused_matches_reference(V, T, d, L, h, B, p):
    """The acceptance rule of test_sampled_ce_loss_bf16_fused_matches_reference, dropout on and off."""
    from oracle import sas as osas
    from test_dropout_parity_gpu import sas_masks
    N, beta = 5, 0.3
    m = _gmodel(V, T, d, L, h, N, p=p, dtype="bf16", scale_items=0.1)
    eng = m.sas.engine()
    assert eng.fused_head and eng.ce_rows_fused
    seq, pos = _batch(V, T, B)
    neg = _negs(V, B, T, N)
    eng.seed_base.fill_(BF16_STEP_SEED.get(V, 41) - 1)
    loss, grads = _autograd_step(m, seq, pos, neg, beta)
    assert all(k in eng.ws.bufs for k in ("gbce_ws", "gbce_dh", "gbce_w", "gbce_keys", "gbce_itemidx")), "the head ran"
    n1 = eng.ws.bufs["gbce_keys"].numel()
    assert not any(v.numel() >= n1 * d for k, v in eng.ws.bufs.items() if k.startswith("gbce_")), "no entries x d buffer"
    sb = eng.seed_base.clone()                    # the forward advanced the step seed once (p > 0)
    masks = {k: v.cpu().double() for k, v in sas_masks(eng, B, T, sb).items()} if p > 0 else None
    P = _P(m)
    le, ge = ref.gbce_loss_and_grads(P, seq, pos, neg, beta, L, h, p=p, masks=masks, emu=osas.BF16Storage())
    l64, g64 = ref.gbce_loss_and_grads(P, seq, pos, neg, beta, L, h, p=p, masks=masks)
    print((V, T, d, p), "loss", loss, "emulation", le.item(), "exact", l64.item())
    assert abs(loss - l64.item()) < FWD_TOL_BF16 * max(1.0, abs(l64.item())), (loss, l64.item())
    res = check_bf16_grads(lambda n: grads[n], ge, g64, d, kbias=lambda n: n.endswith("in_proj_bias"))
    print((V, T, d, p), "worst vs emulation", max(res.items(), key=lambda kv: kv[1][0]),
          "worst vs exact", max(res.items(), key=lambda kv: kv[1][1]))
    assert not grads["sas.item_emb.weight"][0].any()


def test_all_padding_batch_gives_zero_loss_gradients_and_step():
    from rbm_amd.train_step import FusedTrainStep
    for dtype in ("fp32", "bf16"):
        m = _gmodel(60, 16, 64, 1, 1, 3, dtype=dtype)
        z = torch.zeros(2, 16, dtype=torch.int64)
        neg = _negs(60, 2, 16, 3)
        loss, grads = _autograd_step(m, z, z, neg, 0.3)
        assert loss == 0.0
        assert all(not g.any() for g in grads.values()), dtype
        t = FusedTrainStep(m, lr=1e-3)
        before = t.flat.data.clone()
        l = t.step(z.cuda(), z.cuda(), neg.cuda())
        torch.cuda.synchronize()
        assert float(l.item()) == 0.0 and torch.equal(before, t.flat.data), dtype


# ================================================================ the fused step
STEP = (500, 37, 64, 2, 2, 3)
N_STEP = 5


def _step_model(dtype="bf16", p=0.2, l2=0.0, seed=1, N=N_STEP, **kw):
    from rbm_amd.train_step import FusedTrainStep
    V, T, d, L, h, B = STEP
    m = _gmodel(V, T, d, L, h, N, p=p, dtype=dtype, seed=seed, l2=l2, scale_items=0.1)
    return m, FusedTrainStep(m, lr=1e-3, **kw)


def _step_batches(n, N=N_STEP):
    V, T, d, L, h, B = STEP
    out = []
    for i in range(n):
        seq, pos = _batch(V, T, B, seed=100 + i)
        out.append((seq.cuda(), pos.cuda(), _negs(V, B, T, N, seed=i).cuda()))
    return out


def test_fused_step_equals_gbce_loss_plus_fused_adam_bit_for_bit():
    """Both forms run the same kernels on the same seeds: the parameters after one step are the same bits.  beta: the
    step's default is gbce_beta(N, V, t) from the model's args."""
    from rbm_amd.models.sas import gbce_beta
    V = STEP[0]
    b = _step_batches(1)[0]
    m1, t1 = _step_model(gbce_beta=None)
    m2, t2 = _step_model()
    assert t1.loss == "gbce" and t1.gbce_beta == 1.0               # t = 0
    m3 = _gmodel(*STEP[:5], N_STEP, dtype="bf16", t=0.75)
    from rbm_amd.train_step import FusedTrainStep
    assert FusedTrainStep(m3).gbce_beta == gbce_beta(N_STEP, V, 0.75) < 1.0
    m1, t1 = _step_model(gbce_beta=0.3)
    m2, t2 = _step_model(gbce_beta=0.3)
    assert t1.opt.marks is None and getattr(t1.engine, "row_marks", None) is None
    t1.engine.seed_base.fill_(77)
    t2.engine.seed_base.fill_(77)
    l1 = float(t1.step(*b).item())
    loss = m2.gbce_loss(*b, beta=0.3)
    loss.backward()
    for n, q in m2.sas.named_parameters():
        t2.flat.view(n, t2.flat.grad).copy_(q.grad)
    t2._update()
    torch.cuda.synchronize()
    assert l1 == float(loss.item())
    assert torch.equal(t1.flat.data, t2.flat.data)
    assert int(t1.engine.seed_base.item()) == int(t2.engine.seed_base.item()) == 78
    assert not m1.sas.item_emb.weight[0].any()


def test_captured_replays_equal_eager_steps():
    bs = _step_batches(3)
    m0, t0 = _step_model(gbce_beta=0.3)
    for b in bs[:1] * 2:                 # the capture's two warmup steps
        t0.step(*b)
    want = [float(t0.step(*b).item()) for b in bs]
    m1, t1 = _step_model(gbce_beta=0.3)
    t1.capture(*bs[0], warmup=2)
    got = [float(t1.replay(*b).item()) for b in bs]
    torch.cuda.synchronize()
    assert got == want, (got, want)
    assert torch.equal(t0.flat.data, t1.flat.data)
    assert all(np.isfinite(want))


def test_three_steps_are_reproducible_from_the_same_seeds():
    bs = _step_batches(3)
    runs = []
    for _ in range(2):
        m, t = _step_model()
        losses = [float(t.step(*b).item()) for b in bs]
        runs.append((losses, t.flat.data.clone()))
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1])


def _rule_histories(rng, V, n=600):
    hist = []
    for _ in range(n):                                             # chains of 10 .. 17 items: 0 .. 7 leading pads
        x = [int(rng.integers(1, V + 1))]
        for _ in range(int(rng.integers(9, 17))):
            x.append((7 * x[-1] + 3) % V + 1)
        hist.append(x)
    return hist


def test_sampled_capture_learns_a_deterministic_next_item_rule():
    """The rule task of test_it_learns_a_deterministic_next_item_rule (V = 200, T = 16, d = 64, 200 steps), every
    iteration one replay of capture_sampled(DeviceWarpSampler(negs=N)): sampling, the gBCE step and Adam in one graph."""
    from rbm_amd.dataloaders import DeviceWarpSampler
    from rbm_amd.train_step import FusedTrainStep
    V, T, d, L, h, B, N = 200, 16, 64, 1, 1, 16, 8
    rng = np.random.default_rng(0)
    sampler = DeviceWarpSampler(_rule_histories(rng, V), V, B, T, seed=0, negs=N)
    m = _gmodel(V, T, d, L, h, N, dtype="bf16", seed=0, t=0.5)
    t = FusedTrainStep(m, lr=1e-3)
    t.capture_sampled(sampler, warmup=2)
    assert t.packed is None and tuple(t.static[2].shape) == (B, T, N)
    losses = [t.replay_sampled().clone() for _ in range(200)]
    losses = [float(x.item()) for x in losses]
    sq, ps = t.static[0].cpu().numpy(), t.static[1].cpu().numpy()  # the batches follow the rule
    assert ((ps == (7 * sq + 3) % V + 1) | (sq == 0)).all()
    seq, pos = _rule_batch(rng, 256, T)
    m.eval()
    rank = m.full_rank(seq, pos[:, -1], exclude_seen=False)
    hr10 = float((rank < 10).float().mean().item())
    print("gbce learns: first / last loss", losses[0], losses[-1], "HR@10", hr10)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], (losses[0], losses[-1])
    assert hr10 >= 0.5, hr10


def test_sparse_tables_match_dense_on_the_touched_rows():
    """table_optim="sparse": the same loss and gradient bits as the dense twin; after the first step (equal moments,
    equal step count: the lazy rule of tests/adam_rows_ref.py is the dense rule on a touched row) the touched rows
    seq | pos | neg hold the dense twin's bits and every other row of the table is unchanged."""
    b = _step_batches(1)[0]
    res = {}
    for mode in ("sparse", "dense"):
        m, t = _step_model(table_optim=mode, gbce_beta=0.3)
        before = t.flat.view("item_emb.weight").clone()
        t._compute(*b)
        torch.cuda.synchronize()
        stats = (t.loss_out.clone(), t.flat.grad.clone())
        t.flat.grad.zero_()
        m, t = _step_model(table_optim=mode, gbce_beta=0.3)
        t.step(*b)
        torch.cuda.synchronize()
        res[mode] = stats + (t.flat.view("item_emb.weight").clone(), before, t.flat.data.clone())
    s, dn = res["sparse"], res["dense"]
    assert torch.equal(s[0], dn[0]) and torch.equal(s[1], dn[1]) and float(s[1].abs().sum()) > 0
    V1 = s[2].shape[0]
    ids = torch.cat([x.reshape(-1) for x in b])
    rows = torch.unique(ids[(ids >= 1) & (ids < V1)])
    rest = torch.ones(V1, dtype=torch.bool, device="cuda")
    rest[rows] = False
    assert torch.equal(s[2][rows], dn[2][rows]) and not torch.equal(s[2][rows], s[3][rows])
    assert torch.equal(s[2][rest], s[3][rest]) and rest.any()


def test_sgd_clipping_and_l2_run_with_gbce():
    """optimizer="sgd" and max_grad_norm: the step equals its eager composition (same kernels, same seeds); l2_emb in
    fp32: the loss and gradients against float64."""
    V, T, d, L, h, B = STEP
    b = _step_batches(1)[0]
    for kw in (dict(optimizer="sgd", momentum=0.9), dict(max_grad_norm=0.05)):
        runs = []
        for _ in range(2):
            m, t = _step_model(gbce_beta=0.3, **kw)
            losses = [float(t.step(*b).item()) for _ in range(2)]
            runs.append((losses, t.flat.data.clone()))
        m2, t2 = _step_model(gbce_beta=0.3, **kw)
        for _ in range(2):
            t2._compute(*b, update=True)
            t2._update()
        torch.cuda.synchronize()
        assert runs[0][0] == runs[1][0] and all(np.isfinite(runs[0][0]))
        assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][1], t2.flat.data)
        if "max_grad_norm" in kw:
            assert float(t.grad_norm.item()) > 0.05 and 0 < float(t.clip_coef.item()) < 1
    l2 = 1e-3
    m, t = _step_model(dtype="fp32", p=0.0, l2=l2, gbce_beta=0.3)
    assert t.l2 == l2
    t._compute(*b)
    t._l2(t.loss_out[2:3])
    torch.cuda.synchronize()
    loss = float(t.loss_out[2].item())
    l64, g64 = ref.gbce_loss_and_grads(_P(m), b[0].cpu(), b[1].cpu(), b[2].cpu(), 0.3, L, h, l2_emb=l2)
    assert abs(loss - l64.item()) < 1e-5 * max(1.0, abs(l64.item())), (loss, l64.item())
    grads = {k: t.flat.view(k[4:], t.flat.grad).cpu().numpy() for k in g64}
    r = {k: v.numpy() for k, v in g64.items()}
    check_grads(grads, r, d, GRAD_TOL_F32, max(np.linalg.norm(v) for v in r.values()))


# ================================================================ refusals
def test_refusals():
    from rbm_amd.dataloaders import DeviceWarpSampler
    from rbm_amd.models import model_factory
    from rbm_amd.train_step import FusedTrainStep
    from rbm_amd import ops
    V, T, d, L, h, B = STEP
    a = sas_args(V, T, d, L, h, dtype="bf16")
    a.sas_loss = "gbce"
    with pytest.raises(ValueError, match="sas_negs"):              # a missing N
        model_factory(a)
    a.sas_negs = N_STEP
    m = model_factory(a)
    t = FusedTrainStep(m, lr=1e-3)
    assert t.loss == "gbce"
    b = _step_batches(1)[0]
    launches = []
    real = ops.call
    ops.call = lambda name, *args: launches.append(name) or real(name, *args)
    n0 = 0
    try:
        with pytest.raises(ValueError, match="single device"):
            FusedTrainStep(m, dp=True)
        with pytest.raises(ValueError, match="shard_rows"):
            FusedTrainStep(m, shard_rows="on")
        with pytest.raises(ValueError, match="steps_per_graph"):
            t.capture(*b, warmup=1, steps_per_graph=2)
        hist = _rule_histories(np.random.default_rng(3), V, 20)
        with pytest.raises(ValueError, match="steps_per_graph"):
            t.capture_sampled(DeviceWarpSampler(hist, V, B, T, seed=1, negs=N_STEP), warmup=1, steps_per_graph=2)
        for bad in (DeviceWarpSampler(hist, V, B, T, seed=1), DeviceWarpSampler(hist, V, B, T, seed=1, negs=N_STEP + 1),
                    DeviceWarpSampler(hist, V, B, T, seed=1, shared_negs=8)):
            with pytest.raises(ValueError, match="negs"):
                t.capture_sampled(bad, warmup=1)
        with pytest.raises(ValueError, match="negs"):              # a batch with another N
            t.step(b[0], b[1], b[2][:, :, :2].contiguous())
        assert len(launches) == n0, launches[n0:]                  # every refusal before a launch
    finally:
        ops.call = real
    with pytest.raises(ValueError, match="negs"):
        DeviceWarpSampler(hist, V, B, T, negs=3, shared_negs=8)
    over = torch.ones(B, T, ops.sas_gbce_max_n() + 1, dtype=torch.int64)
    with pytest.raises(ValueError, match="negatives"):
        m.gbce_loss(b[0], b[1], over)
    with pytest.raises(ValueError, match=r"\(B, T, N\)"):
        m.gbce_loss(b[0], b[1], over[:, :5, :3])
    with pytest.raises(ValueError, match="fp32"):
        _gmodel(40, 8, 50, 1, 1, 3, dtype="bf16").gbce_loss(*_batch(40, 8, 2), _negs(40, 2, 8, 3))
