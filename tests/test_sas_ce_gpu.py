"""SASRec training with the tied full-catalogue softmax cross-entropy loss, on the GPU.

* the two row kernels of sas_ce.hip directly (rs_sas_ce_rows_fwd / rs_sas_ce_rows_bwd) against the float64
  reference (tests/sas_ce_ref.py) and against the composed launches they replace, outputs NaN-filled and guarded;
* ``SASModel.ce_loss`` + autograd in fp32 (the project's fp32 bars) and on the bf16 fused path (conftest's bf16 bars,
  dropout masks replayed into the reference);
* ``FusedTrainStep(loss="ce")``: against ce_loss + the fused Adam (bit for bit: both run the same kernels), graph
  capture / unrolled capture against eager steps (bit for bit), run-to-run reproducibility, neg=None, l2_emb;
* the row-marked optimizer sweep is off with CE; the fp32 loss curve against the CPU float64 reference + torch Adam;
  a deterministic next-item rule is learnt.

Each row-kernel test prints its worst error / bar per output (pytest -s).
"""
import math

import numpy as np
import pytest
import torch

import sas_ce_ref as ref
from conftest import EMU_TOL, check_bf16_grads, exact_bound, rel  # noqa: F401  (the project's own bf16 bars)
from test_sas_gpu import FWD_TOL_BF16, GRAD_TOL_F32, check_grads, sas_args

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
GUARD = 32
EPS = 1e-8
SENT = -7          # sentinel of the integer outputs


# ================================================================ the row kernels
def _labels(M, pattern, rng):
    lab = np.zeros(M, np.int64)
    if pattern == "all":
        lab[:] = rng.integers(1, 1000, M)
    elif pattern == "leftpad":                      # sequences of 13 positions, random numbers of leading pads
        T = 13
        for s in range(0, M, T):
            n = min(T, M - s)
            k = int(rng.integers(0, n + 1))
            lab[s + k:s + n] = rng.integers(1, 1000, n - k)
    elif pattern == "first":
        lab[0] = 5
    elif pattern == "last":
        lab[M - 1] = 7
    return lab


def _nan(shape, dt):
    return torch.full(shape, math.nan, dtype=dt, device="cuda")


def _rowerr(out, want, scale_rows=None):
    """worst over rows of max|out - want| / max|row of want| (scale_rows: another per-row magnitude)."""
    out, want = np.asarray(out, np.float64), np.asarray(want, np.float64)
    if out.size == 0:
        return 0.0
    if out.ndim == 1:
        out, want = out[:, None], want[:, None]
    sc = np.abs(want).max(-1) if scale_rows is None else np.asarray(scale_rows, np.float64)
    return float((np.abs(out - want).max(-1) / np.maximum(sc, 1e-30)).max())


def _run_rows(M, d, pattern, seed, cap=None, strided=False, splits=6):
    """Both row kernels and the composed launches on one problem; returns {output: (err, composed err, rounding)}."""
    from rbm_amd import ops
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    lab_np = _labels(M, pattern, rng)
    labels = torch.from_numpy(lab_np).cuda()
    cap = M if cap is None else cap
    if strided:
        wide = _nan((M, 2 * d), BF)
        wide[:, :d] = (torch.randn(M, d, device="cuda") * 1.5 + 0.3).to(BF)
        x = wide[:, :d]
    else:
        x = (torch.randn(M, d, device="cuda") * 1.5 + 0.3).to(BF)
    gamma = (1.0 + 0.2 * torch.randn(d, device="cuda")).float()
    beta = (0.1 * torch.randn(d, device="cuda")).float()

    # ---- forward: ours
    idx = torch.full((cap + GUARD,), SENT, dtype=torch.int32, device="cuda")
    rank = torch.full((M + GUARD,), SENT, dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), SENT, dtype=torch.int32, device="cuda")
    div = _nan((1,), F32)
    hl, lab = _nan((cap + GUARD, d), BF), torch.full((cap + GUARD,), SENT, dtype=torch.int64, device="cuda")
    mu, rs = _nan((cap + GUARD,), F32), _nan((cap + GUARD,), F32)
    ops.sas_ce_rows_fwd(x, labels, cap, gamma, beta, EPS, idx, rank, cnt, hl, lab, mu, rs, divisor=div)
    # ---- forward: the composed launches
    f, mu_f, rs_f = torch.empty(M, d, dtype=BF, device="cuda"), torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    ops.layernorm_fwd(x, gamma, beta, EPS, f, mu_f, rs_f, 0)
    idx_c = torch.full((cap,), SENT, dtype=torch.int32, device="cuda")
    rank_c = torch.full((M,), SENT, dtype=torch.int32, device="cuda")
    cnt_c = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.compact_rows(labels, cap, idx_c, rank_c, cnt_c)
    hl_c, lab_c = torch.empty(cap, d, dtype=BF, device="cuda"), torch.empty(cap, dtype=torch.int64, device="cuda")
    ops.gather_rows(f, idx_c, cnt_c, cap, hl_c, labels, lab_c)
    torch.cuda.synchronize()
    n = int(cnt.item())
    ridx, rrank, rn, rhl, rlab, rmu, rrs = ref.rows_fwd_ref(x.float().cpu().numpy(), lab_np, cap, gamma.cpu().numpy(),
                                                            beta.cpu().numpy(), EPS)
    # placement: exactly rs_compact_rows (and the reference)
    assert n == int(cnt_c.item()) == rn
    assert float(div.item()) == max(n, 1)
    assert torch.equal(idx[:cap], idx_c) and (idx[:cap].cpu().numpy() == ridx).all()
    assert torch.equal(rank[:M], rank_c) and (rank[:M].cpu().numpy() == rrank).all()
    assert torch.equal(lab[:n], lab_c[:n]) and (lab[:n].cpu().numpy() == rlab).all()
    # guards and the rows >= count: untouched
    assert (idx[cap:] == SENT).all() and (rank[M:] == SENT).all() and (lab[n:] == SENT).all()
    assert torch.isnan(hl[n:].float()).all() and torch.isnan(mu[n:]).all() and torch.isnan(rs[n:]).all()
    assert not torch.isnan(hl[:n].float()).any()
    if strided:
        assert torch.isnan(wide[:, d:].float()).all()
    res = {}
    sel = ridx[:n]
    xmax = np.abs(x.float().cpu().numpy()[sel]).max(-1) if n else np.zeros(0)
    res["hl"] = (_rowerr(hl[:n].float().cpu(), rhl), _rowerr(hl_c[:n].float().cpu(), rhl), 2.0 ** -8)
    res["mean"] = (_rowerr(mu[:n].cpu(), rmu, xmax), _rowerr(mu_f.cpu().numpy()[sel], rmu, xmax), d * 2.0 ** -23)
    res["rstd"] = (_rowerr(rs[:n].cpu(), rrs), _rowerr(rs_f.cpu().numpy()[sel], rrs), d * 2.0 ** -23)

    # ---- backward: the same inputs for both forms (the composed forward's statistics)
    slab = _nan((splits, cap, d), F32)
    slab[:, :n] = torch.randn(splits, n, d, device="cuda")
    mu_k, rs_k = _nan((cap,), F32), _nan((cap,), F32)
    if n:
        sel_t = torch.from_numpy(sel.astype(np.int64)).cuda()
        mu_k[:n], rs_k[:n] = mu_f[sel_t], rs_f[sel_t]
    nb = ops.sas_ce_rows_nparts(M)
    dx = _nan((M + GUARD, d), BF)
    part = _nan((nb + 1, 2, d), F32)
    ops.sas_ce_rows_bwd(slab, splits, cap, rank, x, gamma, mu_k, rs_k, dx[:M], part)
    df = torch.empty(M, d, dtype=BF, device="cuda")
    ops.splitk_scatter_rows(slab, splits, cap, rank_c, df)
    dx_c = torch.empty(M, d, dtype=BF, device="cuda")
    dg_c, db_c = torch.zeros(d, device="cuda"), torch.zeros(d, device="cuda")
    wln = torch.empty(2 * 512 * d, device="cuda")
    ops.layernorm_bwd(x, df, gamma, mu_f, rs_f, EPS, dx_c, dg_c, db_c, wln, 0)
    torch.cuda.synchronize()
    assert torch.isnan(dx[M:].float()).all() and torch.isnan(part[nb:]).all()
    assert not torch.isnan(dx[:M].float()).any() and not torch.isnan(part[:nb]).any()
    rdx, rpart = ref.rows_bwd_ref(slab[:, :max(n, 1)].cpu().numpy() if n else np.zeros((splits, 1, d), np.float32),
                                  rrank, x.float().cpu().numpy(), gamma.cpu().numpy(),
                                  mu_k.cpu().numpy(), rs_k.cpu().numpy(), nb, d)
    dxn = dx[:M].float().cpu().numpy()
    assert not dxn[rrank < 0].any()                                      # exactly 0 at the invalid rows
    res["dx"] = (_rowerr(dxn[sel], rdx[sel]), _rowerr(dx_c.float().cpu().numpy()[sel], rdx[sel]), 2.0 ** -8)
    pn = part[:nb].double().cpu().numpy()
    tot, rtot = pn.sum(0), rpart.sum(0)
    ctot = np.stack([dg_c.double().cpu().numpy(), db_c.double().cpu().numpy()])
    res["ln_total"] = (_rowerr(tot, rtot), _rowerr(ctot, rtot), d * 2.0 ** -23)
    empty = np.abs(rpart).max(-1) == 0
    assert not pn[empty].any()                                           # a set without valid rows: exactly 0
    live = ~empty
    res["ln_per_wg"] = (_rowerr(pn[live], rpart[live]), res["ln_total"][1], d * 2.0 ** -23)
    return res


def _check_rows(tag, res):
    line, bad = [], {}
    for k, (err, comp, rnd) in res.items():
        bar = max(2.0 * comp, rnd)
        line.append(f"{k} {err / bar:.3f}")
        if err > bar:
            bad[k] = (err, bar)
    print(tag, "err/bar:", ", ".join(line))
    assert not bad, bad


@pytest.mark.parametrize("pattern", ["none", "all", "leftpad", "first", "last"])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 16 * 43 - 11, 4135])
@pytest.mark.parametrize("d", [64, 128])
def test_row_kernels(d, M, pattern):
    _check_rows(f"rows d={d} M={M} {pattern}", _run_rows(M, d, pattern, seed=M + d))


@pytest.mark.parametrize("d", [64, 128])
def test_row_kernels_strided_input(d):
    _check_rows(f"rows strided d={d}", _run_rows(677, d, "leftpad", seed=3, strided=True))


@pytest.mark.parametrize("d,splits", [(64, 1), (128, 9)])
def test_row_kernels_cap_below_count_and_other_split_counts(d, splits):
    """cap < count: the rows past cap are dropped exactly as rs_compact_rows drops them; 1 and 9 slabs."""
    M = 4135
    n_all = int((_labels(M, "leftpad", np.random.default_rng(11)) != 0).sum())
    _check_rows(f"rows cap<count d={d}", _run_rows(M, d, "leftpad", seed=11, cap=n_all // 2, splits=splits))
    _check_rows(f"rows splits={splits} d={d}", _run_rows(65, d, "all", seed=12, splits=splits))


def test_row_kernels_unsupported_launch_nothing():
    import rbm_amd._lib as L
    lib = L.lib()
    s = torch.cuda.current_stream().cuda_stream

    def codes(dtype, d, tdt):
        M = 8
        x = torch.zeros(M, d, dtype=tdt, device="cuda")
        labels = torch.ones(M, dtype=torch.int64, device="cuda")
        g = torch.ones(d, device="cuda")
        idx = torch.full((M,), SENT, dtype=torch.int32, device="cuda")
        rank = torch.full((M,), SENT, dtype=torch.int32, device="cuda")
        cnt = torch.full((1,), SENT, dtype=torch.int32, device="cuda")
        hl, lab = _nan((M, d), tdt), torch.full((M,), SENT, dtype=torch.int64, device="cuda")
        mu, rs, dx, part = _nan((M,), F32), _nan((M,), F32), _nan((M, d), tdt), _nan((2 * d,), F32)
        slab = torch.zeros(M * d, device="cuda")
        p = lambda t: t.data_ptr()  # noqa: E731
        a = lib.rs_sas_ce_rows_fwd(dtype, M, d, p(x), d, p(labels), M, p(g), p(g), EPS, p(idx), p(rank), p(cnt), None,
                                   p(hl), d, p(lab), p(mu), p(rs), s)
        b = lib.rs_sas_ce_rows_bwd(dtype, M, d, p(slab), 1, M, p(rank), p(x), d, p(g), p(mu), p(rs), p(dx), d, p(part), s)
        torch.cuda.synchronize()
        assert (idx == SENT).all() and (rank == SENT).all() and (cnt == SENT).all() and (lab == SENT).all()
        for t in (hl, mu, rs, dx, part):
            assert torch.isnan(t.float()).all()
        return a, b
    assert codes(L.F32, 64, F32) == (1002, 1002)
    assert codes(L.BF16, 50, BF) == (1002, 1002)
    assert codes(L.BF16, 256, BF) == (1002, 1002)


# ================================================================ the model
SHAPES = [(60, 16, 64, 2, 1, 4), (500, 37, 64, 2, 2, 3), (300, 50, 50, 1, 2, 2), (127, 16, 128, 1, 1, 2),
          (128, 16, 128, 1, 1, 2), (20000, 8, 64, 1, 1, 2)]


def _model(V, T, d, L, h, p=0.0, dtype="fp32", seed=None, l2=0.0, scale_items=None):
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    torch.manual_seed(V + T if seed is None else seed)
    a = sas_args(V, T, d, L, h, p=p, dtype=dtype)
    a.l2_emb = l2
    m = model_factory(a)
    if scale_items is not None:
        with torch.no_grad():
            m.sas.item_emb.weight.mul_(scale_items)
    m.train()
    return m


def _batch(V, T, B, seed=0):
    """left-padded (seq, pos): one fully padded sequence and one with 3 leading pads (B >= 4), the label V forced in"""
    rng = np.random.default_rng(seed + T)
    seq = rng.integers(1, V + 1, (B, T))
    pos = rng.integers(1, V + 1, (B, T))
    seq[0, :3] = 0
    pos[0, :3] = 0
    if B >= 4:
        seq[2], pos[2] = 0, 0
    pos[-1, -1] = V
    pos[0, 5] = V
    return torch.from_numpy(seq), torch.from_numpy(pos)


def _P(m):
    return {k: v.detach().cpu().double() for k, v in m.state_dict().items()}


def _autograd_step(m, seq, pos):
    m.zero_grad(set_to_none=True)
    loss = m.ce_loss(seq.numpy(), pos)           # numpy and tensor ids
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.item()), {k: q.grad.detach().cpu().numpy() for k, q in m.named_parameters()}


# Weight seed of the fp32 case (500, 37): V + T + 1.  With V + T = 537 and this batch the fp32 gradient of block 0's
# conv1 is 1.6e-4 from the float64 one while every other tensor, and this tensor at the seeds 538 .. 542, is within
# 2.7e-6; the float64 reference moves by 3e-7 under 2^-24 relative noise on the parameters, and the BCE step through
# the same (unchanged) block kernels on that draw is 9.7e-3 off on the same tensor: one discontinuity of the network
# (a ReLU input within fp32 rounding of zero) falls on different sides in fp32 and float64 there.  The draw is chosen
# by those figures; the bar is the project's.
F32_SEED = {(500, 37): 538}


@pytest.mark.parametrize("V,T,d,L,h,B", SHAPES)
def test_ce_loss_fp32_matches_float64_reference(V, T, d, L, h, B):
    m = _model(V, T, d, L, h, seed=F32_SEED.get((V, T)))
    seq, pos = _batch(V, T, B)
    loss, grads = _autograd_step(m, seq, pos)
    l64, g64 = ref.ce_loss_and_grads(_P(m), seq, pos, L, h)
    print((V, T, d), "loss", loss, "ref", l64.item())
    assert abs(loss - l64.item()) < 1e-5 * max(1.0, abs(l64.item())), (loss, l64.item())
    r = {k: g64[k].numpy() for k in grads}
    print((V, T, d), "worst gradient errors", sorted(((rel(grads[k], r[k]), k) for k in grads
                                                      if not k.endswith("in_proj_bias")), reverse=True)[:3])
    check_grads(grads, r, d, GRAD_TOL_F32, max(np.linalg.norm(v) for v in r.values()))
    assert not grads["sas.item_emb.weight"][0].any()


# Step seed (= dropout draw) of the V = 20,000 case: it has B * T = 16 tokens, and at p = 0.2 the gradient of conv1
# hangs on a handful of kept activations.  The bf16-storage emulation's own distance to the exact math (a figure of
# the two float64 references alone) over the draws 40 .. 51: 0.007, 0.156, 0.108, 0.008, 0.007, 0.072, 0.018, 0.033,
# 0.041, 0.007, 0.007, 0.089 -- at 41 it is above the 0.15 cap of conftest.exact_bound, so nothing could pass there.
# Draw 43 (0.008) is used; the other shapes keep 41.
BF16_STEP_SEED = {20000: 43}


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("V,T,d,L,h,B", [s for s in SHAPES if s[2] in (64, 128)])
def test_ce_loss_bf16_fused_matches_reference(V, T, d, L, h, B, p):
    from oracle import sas as osas
    from test_dropout_parity_gpu import sas_masks
    m = _model(V, T, d, L, h, p=p, dtype="bf16", scale_items=0.1)
    eng = m.sas.engine()
    assert eng.fused_head and eng.ce_rows_fused
    seq, pos = _batch(V, T, B)
    eng.seed_base.fill_(BF16_STEP_SEED.get(V, 41) - 1)
    loss, grads = _autograd_step(m, seq, pos)
    sb = eng.seed_base.clone()                    # the forward advanced the step seed once (p > 0)
    masks = {k: v.cpu().double() for k, v in sas_masks(eng, B, T, sb).items()} if p > 0 else None
    P = _P(m)
    le, ge = ref.ce_loss_and_grads(P, seq, pos, L, h, p=p, masks=masks, emu=osas.BF16Storage())
    l64, g64 = ref.ce_loss_and_grads(P, seq, pos, L, h, p=p, masks=masks)
    print((V, T, d, p), "loss", loss, "emulation", le.item(), "exact", l64.item())
    assert abs(loss - l64.item()) < FWD_TOL_BF16 * max(1.0, abs(l64.item())), (loss, l64.item())
    out = check_bf16_grads(lambda n: grads[n], ge, g64, d, kbias=lambda n: n.endswith("in_proj_bias"))
    print((V, T, d, p), "worst vs emulation", max(out.items(), key=lambda kv: kv[1][0]),
          "worst vs exact", max(out.items(), key=lambda kv: kv[1][1]))
    assert not grads["sas.item_emb.weight"][0].any()


def test_ce_loss_bf16_other_width_needs_fp32_mode():
    m = _model(40, 8, 50, 1, 1, dtype="bf16")
    seq, pos = _batch(40, 8, 2)
    with pytest.raises(ValueError, match="fp32"):
        m.ce_loss(seq, pos)


def test_ce_loss_all_padding_batch():
    for dtype in ("fp32", "bf16"):
        m = _model(60, 16, 64, 1, 1, dtype=dtype)
        z = torch.zeros(2, 16, dtype=torch.int64)
        loss, grads = _autograd_step(m, z, z)
        assert loss == 0.0
        assert all(not g.any() for g in grads.values()), dtype


def test_reference_loop_with_torch_adam():
    """loss = model.ce_loss(seq, pos); loss.backward(); optimizer.step() -- the loss falls on a repeated batch."""
    m = _model(60, 16, 64, 1, 1, dtype="bf16", scale_items=0.1)
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    seq, pos = _batch(60, 16, 4)
    losses = []
    for _ in range(12):
        opt.zero_grad()
        loss = m.ce_loss(seq, pos)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < 0.7 * losses[0], losses
    assert not m.sas.item_emb.weight[0].any()


# ================================================================ the fused step
STEP = (500, 37, 64, 2, 2, 3)


def _step_model(loss="ce", dtype="bf16", p=0.2, l2=0.0, seed=1, **kw):
    from rbm_amd.train_step import FusedTrainStep
    V, T, d, L, h, B = STEP
    m = _model(V, T, d, L, h, p=p, dtype=dtype, seed=seed, l2=l2, scale_items=0.1)
    return m, FusedTrainStep(m, lr=1e-3, loss=loss, **kw)


def _step_batches(n):
    V, T, d, L, h, B = STEP
    out = []
    for i in range(n):
        seq, pos = _batch(V, T, B, seed=100 + i)
        out.append(torch.stack([seq, pos, pos.flip(0)]).cuda())     # a neg is carried and ignored
    return out


def test_fused_step_equals_ce_loss_plus_fused_adam_bit_for_bit():
    """Both forms run the same kernels on the same seeds: the parameters after one step are the same bits."""
    b = _step_batches(1)[0]
    m1, t1 = _step_model()
    m2, t2 = _step_model()
    assert t1.opt.marks is None
    t1.engine.seed_base.fill_(77)
    t2.engine.seed_base.fill_(77)
    l1 = float(t1.step(*b.unbind(0)).item())
    loss = m2.ce_loss(b[0], b[1])
    loss.backward()
    for n, q in m2.sas.named_parameters():
        t2.flat.view(n, t2.flat.grad).copy_(q.grad)
    t2._update()
    torch.cuda.synchronize()
    assert l1 == float(loss.item())
    assert torch.equal(t1.flat.data, t2.flat.data)
    assert int(t1.engine.seed_base.item()) == int(t2.engine.seed_base.item()) == 78


@pytest.mark.parametrize("S", [1, 2])
def test_captured_replays_equal_eager_steps(S):
    bs = _step_batches(3 * S)
    m0, t0 = _step_model()
    for b in bs[:1] * 2:                 # the capture's two warmup steps
        t0.step(*b.unbind(0))
    want = [float(t0.step(*b.unbind(0)).item()) for b in bs]
    m1, t1 = _step_model()
    t1.capture(*bs[0].unbind(0), warmup=2, steps_per_graph=S)
    got = []
    for r in range(3):
        if S == 1:
            got.append(float(t1.replay_packed(bs[r]).item()))
        else:
            got += t1.replay_packed(torch.stack(bs[r * S:(r + 1) * S])).tolist()
    torch.cuda.synchronize()
    assert got == want, (got, want)
    assert torch.equal(t0.flat.data, t1.flat.data)
    assert all(np.isfinite(want))


def test_three_steps_are_reproducible_from_the_same_seeds():
    bs = _step_batches(3)
    runs = []
    for _ in range(2):
        m, t = _step_model()
        losses = [float(t.step(*b.unbind(0)).item()) for b in bs]
        runs.append((losses, t.flat.data.clone()))
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1])


def test_neg_none_is_accepted():
    b = _step_batches(2)
    m1, t1 = _step_model()
    m2, t2 = _step_model()
    l1 = [float(t1.step(b[0][0], b[0][1], None).item()), float(t1.step(b[1][0], b[1][1]).item())]
    l2 = [float(t2.step(*x.unbind(0)).item()) for x in b]
    assert l1 == l2 and torch.equal(t1.flat.data, t2.flat.data)
    t1.capture(b[0][0], b[0][1], None, warmup=1)
    assert np.isfinite(float(t1.replay(b[1][0], b[1][1], None).item()))


def test_sampled_capture_runs_with_ce():
    from rbm_amd.dataloaders import DeviceWarpSampler
    import rbm_amd.data as synth
    V, T, d, L, h, B = STEP
    users = synth.user_histories(np.random.default_rng(3), 100, T, V)
    runs = []
    for S in (1, 2):
        m, t = _step_model()
        t.capture_sampled(DeviceWarpSampler(users, V, B, T, seed=9), warmup=2, steps_per_graph=S)
        losses = []
        for _ in range(2 // S):
            losses += t.replay_sampled().reshape(-1).tolist()
        runs.append((losses, t.flat.data.clone()))
    assert runs[0][0] == runs[1][0] and all(np.isfinite(runs[0][0]))
    assert torch.equal(runs[0][1], runs[1][1])


def test_l2_emb_with_ce_fp32():
    V, T, d, L, h, B = STEP
    l2 = 1e-3
    m, t = _step_model(dtype="fp32", p=0.0, l2=l2)
    assert t.l2 == l2
    b = _step_batches(1)[0]
    t._compute(*b.unbind(0))
    t._l2(t.loss_out[2:3])
    torch.cuda.synchronize()
    loss = float(t.loss_out[2].item())
    l64, g64 = ref.ce_loss_and_grads(_P(m), b[0].cpu(), b[1].cpu(), L, h, l2_emb=l2)
    assert abs(loss - l64.item()) < 1e-5 * max(1.0, abs(l64.item())), (loss, l64.item())
    grads = {k: t.flat.view(k[4:], t.flat.grad).cpu().numpy() for k in g64}
    r = {k: v.numpy() for k, v in g64.items()}
    check_grads(grads, r, d, GRAD_TOL_F32, max(np.linalg.norm(v) for v in r.values()))


def test_ce_uses_the_models_switch_and_rejects_data_parallel():
    from rbm_amd.train_step import FusedTrainStep
    V, T, d, L, h, B = STEP
    a = sas_args(V, T, d, L, h, dtype="bf16")
    a.sas_loss = "ce"
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    m = model_factory(a)
    assert FusedTrainStep(m).loss == "ce"
    assert FusedTrainStep(m, loss="bce").loss == "bce"
    with pytest.raises(ValueError, match="single device"):
        FusedTrainStep(m, loss="ce", dp=True)
    with pytest.raises(ValueError):
        FusedTrainStep(m, loss="softmax")


# ================================================================ row marks
def test_row_marked_sweep_is_off_with_ce():
    """V >= ROW_MARKS_MIN: with BCE the optimizer skips the unmarked rows; with CE every row has a gradient, so one
    step must move every non-padding row by a full first Adam step (this fails if the marks stay on)."""
    from oracle import sas as osas
    from rbm_amd.train_step import FusedTrainStep
    V, T, d, L, h, B = 20000, 8, 64, 1, 1, 2
    assert V + 1 >= FusedTrainStep.ROW_MARKS_MIN
    lr = 1e-3
    # item table x 0.1 as in the other bf16 cases: at the raw N(0, 1) init the softmax over 20,001 classes is so
    # sharp that most rows' gradients fall below Adam's eps = 1e-8 and their first update rounds to nothing in fp32
    m = _model(V, T, d, L, h, dtype="bf16", scale_items=0.1)
    assert FusedTrainStep(m, lr=lr, loss="bce").opt.marks is not None
    t = FusedTrainStep(m, lr=lr, loss="ce")
    assert t.opt.marks is None and getattr(t.engine, "row_marks", None) is None
    P = _P(m)
    seq, pos = _batch(V, T, B)
    before = m.sas.item_emb.weight.detach().clone()
    t.step(seq.cuda(), pos.cuda(), None)
    torch.cuda.synchronize()
    after = m.sas.item_emb.weight.detach()
    delta = (after - before).cpu().double()
    assert not delta[0].any()
    print("smallest largest-move of a row:", float(delta[1:].abs().amax(-1).min()), "lr", lr)
    assert delta[1:].ne(0).any(-1).all()                         # every non-padding row has changed
    # float64 reference + torch Adam
    tables = {}
    for tag, emu in (("emu", osas.BF16Storage()), ("exact", None)):
        _, g = ref.ce_loss_and_grads(P, seq, pos, L, h, emu=emu)
        w = P["sas.item_emb.weight"].clone().requires_grad_(True)
        opt = torch.optim.Adam([w], lr=lr)
        w.grad = g["sas.item_emb.weight"]
        opt.step()
        tables[tag] = w.detach()
    name = "sas.item_emb.weight"
    out = check_bf16_grads(lambda n: after.cpu().numpy(), {name: tables["emu"]}, {name: tables["exact"]}, d)
    de = (tables["exact"] - P[name]).numpy()
    print("updated table (vs emulation, vs exact, fmt):", out[name], "; update alone vs exact:", rel(delta.numpy(), de))


# ================================================================ curve, learning
def test_fp32_curve_matches_float64_reference_with_torch_adam():
    import rbm_amd.data as synth
    from rbm_amd.train_step import FusedTrainStep
    V, T, d, L, h, B = 60, 16, 64, 2, 1, 4
    m = _model(V, T, d, L, h)
    P = {k: v.clone().requires_grad_(True) for k, v in _P(m).items()}
    t = FusedTrainStep(m, lr=1e-3, loss="ce")
    opt = torch.optim.Adam(list(P.values()), lr=1e-3)
    rng = np.random.default_rng(4)
    got, want = [], []
    for _ in range(30):
        seq, pos, _ = (torch.from_numpy(a) for a in synth.sas_batch(rng, B, T, V))
        got.append(t.step(seq.cuda(), pos.cuda(), None).clone())
        opt.zero_grad()
        loss = ref.ce_loss(P, seq, pos, L, h)
        loss.backward()
        opt.step()
        want.append(loss.item())
    got = np.array([float(x.item()) for x in got])
    err = np.abs(got - np.array(want))
    print("ce curve fp32: max |dloss|", err.max(), "at", int(err.argmax()), "; first / last loss", want[0], want[-1])
    assert err.max() <= 1e-3, (err.max(), int(err.argmax()))


def _rule_batch(rng, B, T, V=200):
    x = np.zeros((B, T + 1), np.int64)
    x[:, 0] = rng.integers(1, V + 1, B)
    for t in range(T):
        x[:, t + 1] = (7 * x[:, t] + 3) % V + 1
    seq, pos = x[:, :-1].copy(), x[:, 1:].copy()
    for b in range(B):
        k = int(rng.integers(0, 8))
        seq[b, :k] = 0
        pos[b, :k] = 0
    return seq, pos


def test_it_learns_a_deterministic_next_item_rule():
    from rbm_amd.train_step import FusedTrainStep
    V, T, d, L, h, B = 200, 16, 64, 1, 1, 16
    m = _model(V, T, d, L, h, dtype="bf16", seed=0)
    t = FusedTrainStep(m, lr=1e-3, loss="ce")
    rng = np.random.default_rng(0)
    losses = []
    for _ in range(200):
        seq, pos = _rule_batch(rng, B, T)
        losses.append(t.step(torch.from_numpy(seq).cuda(), torch.from_numpy(pos).cuda(), None).clone())
    losses = [float(x.item()) for x in losses]
    seq, pos = _rule_batch(rng, 256, T)
    m.eval()
    rank = m.full_rank(seq, pos[:, -1], exclude_seen=False)
    # the history for the target pos[:, -1] is seq itself (pos is seq shifted by one)
    hr10 = float((rank < 10).float().mean().item())
    print("ce learns: first / last loss", losses[0], losses[-1], "ratio", losses[-1] / losses[0], "HR@10", hr10)
    assert losses[-1] <= 0.25 * losses[0], (losses[0], losses[-1])
    assert hr10 >= 0.8, hr10
