"""SASRec training with the sampled softmax over batch-shared candidates, on the GPU.

* the two head launches of sas_sce.hip directly (rs_sas_sce_fwd / rs_sas_sce_bwd), every output element against the
  float64 reference (tests/sas_sce_ref.py) under derived bounds, outputs NaN-filled and guarded;
* ``SASModel.sampled_ce_loss`` + autograd in fp32 (the project's fp32 bars) and on the bf16 fused path (conftest's
  bf16 bars, dropout masks replayed into the reference); the full-catalogue identity against ``ce_loss``;
* ``FusedTrainStep(loss="sampled_ce")``: against sampled_ce_loss + the fused Adam (bit for bit), graph capture against
  eager steps (bit for bit), run-to-run reproducibility, a sampler with shared_negs captured with the step;
* the errors, the V-free workspace, the sampler's candidates, and a deterministic next-item rule is learnt.

The bounds of the head kernels (u = 2^-24, the fp32 unit roundoff; every quantity on the right is computed in float64
from the kernels' own inputs):

    Z_rj   = sum_k |hl_rk| |E_jk|                     the magnitude a length-d fp32 accumulation's error scales with
    z_r0   : (d + 2) u Z_r0                           d fused multiply-adds and two cross-lane additions
    lse_r  : u ((d + 4) Zmax_r + nlive_r + 16 + splits + |lse_r|)
             the logits' error passes through the log-sum-exp with weights that sum to 1 ((d + 4) u Zmax_r covers it
             and the rounding of z - m, |z| <= Zmax); the sum of at most nlive + 1 terms, each exp within 2 u, carries
             (nlive + 16 + splits) u relative (the candidate splits' partial sums are merged in split order), which the
             logarithm turns into the same absolute error; one rounding of the result
    out    : the rows' bars summed (the sum itself is formed in double) + u |out|
    e_r    = 1.01 (lse bar + (d + 4) u Zmax_r + 4 u)  the exponent's error of p_rj = exp(z_rj - lse_r), hence p's relative
                                                      error (1.01: the second-order term, e_r < 2e-2)
    coef_r : |s| (p_r0 e_r + 4 u)                     (p_r0 - 1) s: p_r0's error, the subtraction, s = dloss / divisor
    pg_rc  : coef's bar |hl_rc| + u |pg_rc|
    dh_rc  : |s| (e_r + (K + 4 + splits) u + fmt) A_rc + coef's bar |E[pos_r]_c| + u |dh_rc|,   A_rc = sum_j p_rj |E[cand_j]_c|
    dEc_jc : |s| (sum_r p_rj e_r |hl_rc| + ((n + 68) u + fmt) B_jc) + u |dEc_jc|,      B_jc = sum_r p_rj |hl_rc|
             (n rows in a fixed order, up to 64 split slabs and the reduction)
    fmt    = 0 in fp32; 2^-7 in bf16: the probabilities enter the MFMA as bf16 operands (8 significant bits: rounding
             2^-8 relative), held to twice the format's rounding.
Each head test prints its worst error / bar per output (pytest -s).
"""
import math

import numpy as np
import pytest
import torch

import sas_ce_ref as ce_ref
import sas_sce_ref as ref
from conftest import check_bf16_grads, rel
from test_sas_ce_gpu import BF16_STEP_SEED, F32_SEED, SHAPES, STEP, _batch, _model, _P, _rule_batch
from test_sas_gpu import FWD_TOL_BF16, GRAD_TOL_F32, check_grads, sas_args

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
GUARD = 8
SENT = -7
U = 2.0 ** -24
TILE = 64          # the kernel's candidate-tile size (sas_sce.hip TS)


def _nan(shape, dt=F32):
    return torch.full(shape, math.nan, dtype=dt, device="cuda")


# ================================================================ the head kernels
def _head_problem(dt, d, rows, K, pattern, seed, dense=False):
    rng = np.random.default_rng(seed)
    V = 300
    cap = rows + 9
    big = pattern == "big"
    hl = torch.from_numpy(rng.standard_normal((cap, d))).to(dt)
    E = torch.from_numpy(rng.standard_normal((V + 1, d)) * ((36.0 if big else 1.0) / math.sqrt(d))).to(dt)
    E[0] = 0
    lab = rng.integers(1, V + 1, cap)
    if dense:
        lab[rng.random(cap) < 0.4] = 0                           # all rows given, lab 0 = no row
    if pattern == "hits":
        cand = lab[rng.integers(0, rows, K)]                      # every candidate is some row's positive
        if dense:
            cand = np.where(cand == 0, 1, cand)
    else:
        cand = rng.integers(1, V + 1, K)
        cand[rng.random(K) < 0.15] = 0                            # ignored slots
        if K > 3:
            cand[K // 2] = cand[0]                                # a duplicate for certain
    return V, cap, hl, E, lab, cand


def _run_head(dt, d, rows, K, pattern, seed, dense=False):
    from rbm_amd import ops
    V, cap, hl, E, lab, cand = _head_problem(dt, d, rows, K, pattern, seed, dense)
    count = cap if dense else rows
    fmt = 2.0 ** -7 if dt == BF else 0.0
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    hl_d, E_d, lab_d, cand_d = hl.cuda(), E.cuda(), dev(lab), dev(cand)
    cnt = None if dense else torch.tensor([rows], dtype=torch.int32, device="cuda")
    nvalid = int((lab[:count] != 0).sum())
    div = torch.tensor([float(max(nvalid, 1))], device="cuda")
    dloss = torch.tensor([0.75], device="cuda")
    nws = ops.sas_sce_ws_numel(cap, K, d)
    ws = _nan((nws + GUARD,))
    out = _nan((4,))
    ops.sas_sce_fwd(hl_d, lab_d, cnt, cap, E_d, cand_d, div, ws[:nws], out)
    ks = ops.sas_sce_dh_splits(cap, K, d)                         # dh: one slab per split of the candidates
    assert 1 <= ks <= max(1, -(-K // TILE))
    dh, coef = _nan((ks * cap + GUARD, d)), _nan((cap + GUARD,))
    src = _nan((cap + K + GUARD, d))
    keys = torch.full((cap + K + GUARD,), SENT, dtype=torch.int64, device="cuda")
    ops.sas_sce_bwd(hl_d, lab_d, cnt, cap, E_d, cand_d, div, dloss, ws[:nws], dh, coef, src[:cap], src[cap:cap + K],
                    keys)
    torch.cuda.synchronize()
    # ---- float64 on the kernels' own inputs
    hl64, E64 = hl.double().numpy(), E.double().numpy()
    lse, z0, rout = ref.head_fwd_ref(hl64, lab, count, E64, cand, float(div.item()))
    rdh, rcoef, rpg, rdEc, rkeys, mag = ref.head_bwd_ref(hl64, lab, count, E64, cand, float(div.item()), 0.75)
    s = 0.75 / float(div.item())
    valid = lab[:count] != 0
    zmax = np.maximum(mag["z0"], mag["z"].max(-1)) * valid
    bar_z0 = (d + 2) * U * mag["z0"] * valid
    bar_lse = U * ((d + 4) * zmax + mag["nlive"] + 16 + ks + np.abs(lse)) * valid
    e_r = 1.01 * (bar_lse + (d + 4) * U * zmax + 4 * U)
    assert e_r.max() < 2e-2
    bar_coef = abs(s) * (mag["p0"] * e_r + 4 * U) * valid
    Epos = np.abs(E64[np.where(valid, lab[:count], 0)])
    P = _probs(hl64, lab, count, E64, cand, lse)
    A = abs(s) * (P @ np.abs(E64[np.where((cand <= 0) | (cand > V), 0, cand)]))
    bar_dh = (e_r[:, None] + (K + 4 + ks) * U + fmt) * A + bar_coef[:, None] * Epos + U * np.abs(rdh)
    bar_pg = bar_coef[:, None] * np.abs(hl64[:count]) + U * np.abs(rpg)
    bar_dEc = abs(s) * ((P * e_r[:, None]).T @ np.abs(hl64[:count]) + ((count + 68) * U + fmt) * (P.T @ np.abs(hl64[:count]))) \
        + U * np.abs(rdEc)
    got = dict(lse=ws[:count].double().cpu().numpy(), z0=ws[cap:cap + count].double().cpu().numpy(),
               dh=dh[:ks * cap].view(ks, cap, d)[:, :count].double().sum(0).cpu().numpy(), coef=coef[:count].double().cpu().numpy(),
               pg=src[:count].double().cpu().numpy(), dEc=src[cap:cap + K].double().cpu().numpy())
    want = dict(lse=(lse, bar_lse), z0=(z0, bar_z0), dh=(rdh, bar_dh), coef=(rcoef, bar_coef), pg=(rpg, bar_pg),
                dEc=(rdEc, bar_dEc))
    res = {}
    for k, (w, bar) in want.items():
        err = np.abs(got[k] - w)
        assert np.isfinite(got[k]).all(), k
        res[k] = float((err / np.maximum(bar, 1e-30)).max()) if err.size else 0.0
        assert (err[bar == 0] == 0).all(), k                      # nothing to round: exact (a masked row's zeros)
    o = out.double().cpu().numpy()
    bar_sum = float((bar_lse + bar_z0).sum()) + U * abs(rout[0])
    res["out.sum"] = abs(o[0] - rout[0]) / max(bar_sum, 1e-30) if bar_sum else float(o[0] != rout[0])
    res["out.mean"] = abs(o[2] - rout[2]) / max(bar_sum / float(div.item()) + 2 * U * abs(rout[2]), 1e-30) \
        if bar_sum else float(o[2] != rout[2])
    assert o[1] == rout[1] == nvalid
    # ---- rows at or past the count, and the guards: untouched
    assert torch.isnan(ws[count:cap]).all() and torch.isnan(ws[cap + count:2 * cap]).all() and torch.isnan(ws[nws:]).all()
    assert torch.isnan(dh[:ks * cap].view(ks, cap, d)[:, count:]).all() and torch.isnan(dh[ks * cap:]).all()
    assert torch.isnan(coef[count:]).all()
    assert torch.isnan(src[count:cap]).all() and torch.isnan(src[cap + K:]).all()
    assert torch.isnan(out[3])
    k = keys.cpu().numpy()
    assert (k[:cap + K] == rkeys).all() and (k[cap + K:] == SENT).all()
    return res


def _probs(hl64, lab, count, E64, cand, lse):
    lab, cand = np.asarray(lab)[:count], np.asarray(cand)
    z = hl64[:count] @ E64[cand].T
    live = (cand != 0)[None, :] & (cand[None, :] != lab[:, None]) & (lab != 0)[:, None]
    return np.where(live, np.exp(np.where(live, z, 0.0) - lse[:, None]), 0.0)


def _check_head(tag, res):
    print(tag, "err/bar:", ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
    bad = {k: v for k, v in res.items() if v > 1.0}
    assert not bad, bad


ROWS = [1, 15, 16, 17, 127, 129, 1031]
KS = [1, 31, 128, 129, 257, 1000, TILE - 1, TILE, TILE + 1]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("d", [64, 128])
def test_head_kernels_bf16(d, rows, K):
    _check_head(f"head bf16 d={d} rows={rows} K={K}", _run_head(BF, d, rows, K, "mixed", seed=d + rows + K))


@pytest.mark.parametrize("pattern", ["hits", "big"])
@pytest.mark.parametrize("K", [31, 257, 1000])
@pytest.mark.parametrize("rows", [17, 129, 1031])
@pytest.mark.parametrize("d", [64, 128])
def test_head_kernels_bf16_hits_and_large_logits(d, rows, K, pattern):
    """hits: every candidate equals some row's positive (masked there, live elsewhere).  big: the largest |z| of
    every case is past 88, where exp(z) overflows fp32 unless the maximum is subtracted."""
    V, cap, hl, E, lab, cand = _head_problem(BF, d, rows, K, pattern, seed=rows + K)
    if pattern == "big":
        zmax = float((hl.double()[:rows] @ E.double()[cand].T).abs().max())
        print("largest |z|", zmax)
        assert zmax > 88                                          # exp(z) alone overflows fp32 there
    _check_head(f"head bf16 {pattern} d={d} rows={rows} K={K}", _run_head(BF, d, rows, K, pattern, seed=rows + K))


@pytest.mark.parametrize("pattern", ["mixed", "big"])
@pytest.mark.parametrize("K", [65, 257])
@pytest.mark.parametrize("rows", [17, 129])
@pytest.mark.parametrize("d", [50, 64, 128])
def test_head_kernels_fp32(d, rows, K, pattern):
    _check_head(f"head fp32 {pattern} d={d} rows={rows} K={K}", _run_head(F32, d, rows, K, pattern, seed=d + K))


@pytest.mark.parametrize("rows,K", [(1, 1), (17, 65), (129, 257)])
@pytest.mark.parametrize("dt,d,pattern", [(F32, 256, "mixed"), (F32, 256, "big"), (F32, 256, "hits"), (BF, 256, "mixed"),
                                          (BF, 256, "big"), (F32, 130, "mixed"), (BF, 136, "hits"), (F32, 1024, "mixed"),
                                          (BF, 1024, "hits")])
def test_head_kernels_wider_than_the_mfma_sweep(dt, d, rows, K, pattern):
    """128 < d <= 1024: the plain kernel with the same outputs (one workgroup per row / candidate), the same bounds.
    (No large-logit case at d = 1024: there the bound on the exponent's error leaves the first-order regime the
    bars are derived in.)"""
    _check_head(f"head wide {pattern} d={d} rows={rows} K={K}", _run_head(dt, d, rows, K, pattern, seed=d + rows + K))


@pytest.mark.parametrize("dt,d", [(BF, 64), (F32, 50), (BF, 72), (F32, 200), (BF, 256)])
def test_head_kernels_all_rows_with_lab_zero_as_no_row(dt, d):
    """count NULL (the fp32 path at widths the compaction does not take): every row is given, lab 0 marks the rows to
    skip -- loss, coefficient and gradient rows exactly 0 there; d = 72: a width padded inside the fragments."""
    _check_head(f"head dense d={d}", _run_head(dt, d, 129, 129, "mixed", seed=d, dense=True))
    _check_head(f"head dense hits d={d}", _run_head(dt, d, 129, 31, "hits", seed=d + 1, dense=True))


def test_head_kernels_unsupported_launch_nothing():
    import rbm_amd._lib as L
    from rbm_amd import ops
    lib = L.lib()
    s = torch.cuda.current_stream().cuda_stream
    kmax = ops.sas_sce_max_k()
    assert kmax >= 16384

    def codes(dtype, d, tdt, K, Kbuf=None):
        cap = 8
        hl, E = torch.zeros(cap, d, dtype=tdt, device="cuda"), torch.zeros(20, d, dtype=tdt, device="cuda")
        lab = torch.ones(cap, dtype=torch.int64, device="cuda")
        cand = torch.ones(Kbuf or max(K, 1), dtype=torch.int64, device="cuda")
        div = torch.ones(1, device="cuda")
        ws, out = _nan((4096,)), _nan((4,))
        dh, coef, pg, dEc = _nan((16 * cap, d)), _nan((cap,)), _nan((cap, d)), _nan((max(Kbuf or K, 1), d))
        keys = torch.full((cap + (Kbuf or max(K, 1)),), SENT, dtype=torch.int64, device="cuda")
        p = lambda t: t.data_ptr()  # noqa: E731
        a = lib.rs_sas_sce_fwd(dtype, cap, d, p(hl), d, p(lab), None, p(E), 20, p(cand), K, p(div), p(ws), p(out), s)
        b = lib.rs_sas_sce_bwd(dtype, cap, d, p(hl), d, p(lab), None, p(E), 20, p(cand), K, p(div), None, p(ws), p(dh),
                               p(coef), p(pg), p(dEc), p(keys), s)
        torch.cuda.synchronize()
        for t in (ws, out, dh, coef, pg, dEc):
            assert torch.isnan(t).all()
        assert (keys == SENT).all()
        return a, b
    assert codes(7, 64, F32, 4) == (1002, 1002)                   # no such dtype
    assert codes(L.BF16, 50, BF, 4) == (1002, 1002)               # bf16 rows that are no multiple of 16 bytes
    assert codes(L.BF16, 1032, BF, 4) == (1002, 1002)
    assert codes(L.F32, 1025, F32, 4) == (1002, 1002)
    assert codes(L.BF16, 64, BF, 0) == (1002, 1002)
    assert codes(L.BF16, 64, BF, kmax + 1, Kbuf=4) == (1002, 1002)


# ================================================================ the model
def _cand(V, K, seed=0):
    if K == V:
        return torch.arange(1, V + 1)
    rng = np.random.default_rng(seed + K)
    c = rng.integers(1, V + 1, K)
    if K > 4:
        c[1] = 0
        c[3] = c[2]
        c[4] = V                                                   # _batch forces the label V in: an accidental hit
    return torch.from_numpy(c)


def _autograd_step(m, seq, pos, cand):
    m.zero_grad(set_to_none=True)
    loss = m.sampled_ce_loss(seq.numpy(), pos, cand)              # numpy and tensor ids
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.item()), {k: q.grad.detach().cpu().numpy() for k, q in m.named_parameters()}


@pytest.mark.parametrize("Ksel", ["1", "50", "V"])
@pytest.mark.parametrize("V,T,d,L,h,B", SHAPES)
def test_sampled_ce_loss_fp32_matches_float64_reference(V, T, d, L, h, B, Ksel):
    K = V if Ksel == "V" else int(Ksel)
    m = _model(V, T, d, L, h, seed=F32_SEED.get((V, T)))
    seq, pos = _batch(V, T, B)
    cand = _cand(V, K)
    loss, grads = _autograd_step(m, seq, pos, cand)
    l64, g64 = ref.sce_loss_and_grads(_P(m), seq, pos, cand, L, h)
    print((V, T, d, K), "loss", loss, "ref", l64.item())
    assert abs(loss - l64.item()) < 1e-5 * max(1.0, abs(l64.item())), (loss, l64.item())
    r = {k: g64[k].numpy() for k in grads}
    print((V, T, d, K), "worst gradient errors", sorted(((rel(grads[k], r[k]), k) for k in grads
                                                         if not k.endswith("in_proj_bias")), reverse=True)[:3])
    check_grads(grads, r, d, GRAD_TOL_F32, max(np.linalg.norm(v) for v in r.values()))
    assert not grads["sas.item_emb.weight"][0].any()


@pytest.mark.parametrize("K", [1, 50, 300])
def test_sampled_ce_loss_fp32_at_256_hidden_units(K):
    """A width past the MFMA sweep (the BCE and CE objectives run there too): the plain head kernel in the model."""
    V, T, d, L, h, B = 300, 16, 256, 1, 2, 2
    m = _model(V, T, d, L, h)
    seq, pos = _batch(V, T, B)
    cand = _cand(V, K)
    loss, grads = _autograd_step(m, seq, pos, cand)
    l64, g64 = ref.sce_loss_and_grads(_P(m), seq, pos, cand, L, h)
    print((V, T, d, K), "loss", loss, "ref", l64.item())
    assert abs(loss - l64.item()) < 1e-5 * max(1.0, abs(l64.item())), (loss, l64.item())
    r = {k: g64[k].numpy() for k in grads}
    print((V, T, d, K), "worst gradient errors", sorted(((rel(grads[k], r[k]), k) for k in grads
                                                         if not k.endswith("in_proj_bias")), reverse=True)[:3])
    check_grads(grads, r, d, GRAD_TOL_F32, max(np.linalg.norm(v) for v in r.values()))
    assert not grads["sas.item_emb.weight"][0].any()


def test_sampled_ce_loss_bf16_at_256_hidden_units_runs_and_is_near_the_reference():
    """bf16 at d = 256 (unfused blocks, the plain head kernel): the loss within the bf16 forward bar of the exact one."""
    V, T, d, L, h, B = 300, 16, 256, 1, 2, 2
    m = _model(V, T, d, L, h, dtype="bf16", scale_items=0.1)
    seq, pos = _batch(V, T, B)
    cand = _cand(V, 50)
    loss, grads = _autograd_step(m, seq, pos, cand)
    l64 = ref.sce_loss(_P(m), seq, pos, cand, L, h).item()
    print((V, T, d), "loss", loss, "exact", l64)
    assert abs(loss - l64) < FWD_TOL_BF16 * max(1.0, abs(l64)), (loss, l64)
    assert all(np.isfinite(g).all() for g in grads.values()) and not grads["sas.item_emb.weight"][0].any()
    with pytest.raises(ValueError, match="1024"):
        _model(V, T, 1032, L, h, dtype="bf16").sampled_ce_loss(seq, pos, cand)


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("V,T,d,L,h,B", [s for s in SHAPES if s[2] in (64, 128)])
def test_sampled_ce_loss_bf16_fused_matches_reference(V, T, d, L, h, B, p):
    from oracle import sas as osas
    from test_dropout_parity_gpu import sas_masks
    m = _model(V, T, d, L, h, p=p, dtype="bf16", scale_items=0.1)
    eng = m.sas.engine()
    assert eng.fused_head and eng.ce_rows_fused
    seq, pos = _batch(V, T, B)
    cand = _cand(V, 50)
    eng.seed_base.fill_(BF16_STEP_SEED.get(V, 41) - 1)
    loss, grads = _autograd_step(m, seq, pos, cand)
    assert all(k in eng.ws.bufs for k in ("sce_ws", "sce_dh", "sce_src", "sce_keys", "sce_itemidx")), "the head ran"
    assert "ce_dlogits" not in eng.ws.bufs and "ce_lnp" in eng.ws.bufs     # no (cap, V) buffer; the fused row kernels
    sb = eng.seed_base.clone()                    # the forward advanced the step seed once (p > 0)
    masks = {k: v.cpu().double() for k, v in sas_masks(eng, B, T, sb).items()} if p > 0 else None
    P = _P(m)
    le, ge = ref.sce_loss_and_grads(P, seq, pos, cand, L, h, p=p, masks=masks, emu=osas.BF16Storage())
    l64, g64 = ref.sce_loss_and_grads(P, seq, pos, cand, L, h, p=p, masks=masks)
    print((V, T, d, p), "loss", loss, "emulation", le.item(), "exact", l64.item())
    assert abs(loss - l64.item()) < FWD_TOL_BF16 * max(1.0, abs(l64.item())), (loss, l64.item())
    res = check_bf16_grads(lambda n: grads[n], ge, g64, d, kbias=lambda n: n.endswith("in_proj_bias"))
    print((V, T, d, p), "worst vs emulation", max(res.items(), key=lambda kv: kv[1][0]),
          "worst vs exact", max(res.items(), key=lambda kv: kv[1][1]))
    assert not grads["sas.item_emb.weight"][0].any()


def test_sampled_ce_loss_bf16_other_width_needs_fp32_mode():
    m = _model(40, 8, 50, 1, 1, dtype="bf16")
    seq, pos = _batch(40, 8, 2)
    with pytest.raises(ValueError, match="fp32"):
        m.sampled_ce_loss(seq, pos, torch.arange(1, 9))


def test_all_padding_batch_and_rows_without_a_live_candidate():
    for dtype in ("fp32", "bf16"):
        m = _model(60, 16, 64, 1, 1, dtype=dtype)
        z = torch.zeros(2, 16, dtype=torch.int64)
        loss, grads = _autograd_step(m, z, z, torch.arange(1, 9))
        assert loss == 0.0
        assert all(not g.any() for g in grads.values()), dtype
        seq, pos = z.clone(), z.clone()
        seq[0, -2:], pos[0, -2:] = torch.tensor([3, 4]), torch.tensor([7, 7])
        loss, grads = _autograd_step(m, seq, pos, torch.tensor([7, 0, 7]))      # 0 or the rows' own positive only
        assert loss == 0.0
        assert all(not g.any() for g in grads.values()), dtype


@pytest.mark.parametrize("V,T,d,L,h,B", [SHAPES[0], SHAPES[2], SHAPES[3]])
def test_full_catalogue_identity_fp32(V, T, d, L, h, B):
    """sampled_ce_loss(seq, pos, arange(1, V + 1)) against ce_loss(seq, pos): each within the fp32 bar of its own
    float64 value, and the two float64 values apart by the padding class alone (class 0, logit exactly 0, which the
    full CE counts and a candidate list cannot name): mean over the valid rows of log(1 + exp(-lse_r))."""
    m = _model(V, T, d, L, h)
    seq, pos = _batch(V, T, B)
    cand = torch.arange(1, V + 1)
    ls, gs = _autograd_step(m, seq, pos, cand)
    m.zero_grad(set_to_none=True)
    lc = m.ce_loss(seq, pos)
    lc.backward()
    torch.cuda.synchronize()
    gc = {k: q.grad.detach().cpu().numpy() for k, q in m.named_parameters()}
    P = _P(m)
    l64s = ref.sce_loss(P, seq, pos, cand, L, h).item()
    l64c = ce_ref.ce_loss(P, seq, pos, L, h).item()
    f = ref.osas.log2feats(P, seq, L, h)
    lse, _, valid = ref.sce_rows(f, P["sas.item_emb.weight"], pos, cand, ref.osas.Exact())
    gap = float(((torch.logaddexp(lse, torch.zeros_like(lse)) - lse) * valid).sum() / int(valid.sum()))
    print((V, T, d), "sampled", ls, "ce", float(lc.item()), "float64", l64s, l64c, "class-0 term", gap)
    bar = 1e-5 * max(1.0, abs(l64c))
    assert abs(ls - l64s) < bar and abs(float(lc.item()) - l64c) < bar
    assert abs((l64c - l64s) - gap) < 1e-12 * max(1.0, abs(l64c))
    assert abs(ls - float(lc.item())) < 2 * bar + gap
    for k in gs:
        if not k.endswith("in_proj_bias"):
            assert rel(gs[k], gc[k]) < 2 * GRAD_TOL_F32 + 10 * gap, (k, rel(gs[k], gc[k]))


# ================================================================ the fused step
K_STEP = 50


def _step_model(dtype="bf16", p=0.2, l2=0.0, seed=1, **kw):
    from rbm_amd.train_step import FusedTrainStep
    V, T, d, L, h, B = STEP
    m = _model(V, T, d, L, h, p=p, dtype=dtype, seed=seed, l2=l2, scale_items=0.1)
    return m, FusedTrainStep(m, lr=1e-3, loss="sampled_ce", **kw)


def _step_batches(n):
    V, T, d, L, h, B = STEP
    out = []
    for i in range(n):
        seq, pos = _batch(V, T, B, seed=100 + i)
        out.append((seq.cuda(), pos.cuda(), _cand(V, K_STEP, seed=i).cuda()))
    return out


def test_fused_step_equals_sampled_ce_loss_plus_fused_adam_bit_for_bit():
    """Both forms run the same kernels on the same seeds: the parameters after one step are the same bits."""
    b = _step_batches(1)[0]
    m1, t1 = _step_model()
    m2, t2 = _step_model()
    assert t1.opt.marks is None and getattr(t1.engine, "row_marks", None) is None
    t1.engine.seed_base.fill_(77)
    t2.engine.seed_base.fill_(77)
    l1 = float(t1.step(*b).item())
    loss = m2.sampled_ce_loss(*b)
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
    m0, t0 = _step_model()
    for b in bs[:1] * 2:                 # the capture's two warmup steps
        t0.step(*b)
    want = [float(t0.step(*b).item()) for b in bs]
    m1, t1 = _step_model()
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


def _sampler(V, B, T, K, seed=9, users=100):
    from rbm_amd.dataloaders import DeviceWarpSampler
    import rbm_amd.data as synth
    hist = synth.user_histories(np.random.default_rng(3), users, T, V)
    return DeviceWarpSampler(hist, V, B, T, seed=seed, shared_negs=K)


def test_sampled_capture_runs_with_shared_negs():
    V, T, d, L, h, B = STEP
    runs = []
    for _ in range(2):
        m, t = _step_model()
        t.capture_sampled(_sampler(V, B, T, K_STEP), warmup=2)
        losses = [float(t.replay_sampled().item()) for _ in range(3)]
        runs.append((losses, t.flat.data.clone()))
    assert runs[0][0] == runs[1][0] and all(np.isfinite(runs[0][0]))
    assert len(set(runs[0][0])) == 3                              # fresh batches and candidates every replay
    assert t.packed is None                                       # no packed buffer that would leave cand stale
    assert torch.equal(runs[0][1], runs[1][1])


def test_l2_emb_with_sampled_ce_fp32():
    V, T, d, L, h, B = STEP
    l2 = 1e-3
    m, t = _step_model(dtype="fp32", p=0.0, l2=l2)
    assert t.l2 == l2
    b = _step_batches(1)[0]
    t._compute(*b)
    t._l2(t.loss_out[2:3])
    torch.cuda.synchronize()
    loss = float(t.loss_out[2].item())
    l64, g64 = ref.sce_loss_and_grads(_P(m), b[0].cpu(), b[1].cpu(), b[2].cpu(), L, h, l2_emb=l2)
    assert abs(loss - l64.item()) < 1e-5 * max(1.0, abs(l64.item())), (loss, l64.item())
    grads = {k: t.flat.view(k[4:], t.flat.grad).cpu().numpy() for k in g64}
    r = {k: v.numpy() for k, v in g64.items()}
    check_grads(grads, r, d, GRAD_TOL_F32, max(np.linalg.norm(v) for v in r.values()))


# ================================================================ errors, memory
def test_errors():
    from rbm_amd.models import model_factory
    from rbm_amd.train_step import FusedTrainStep
    from rbm_amd import ops
    V, T, d, L, h, B = STEP
    a = sas_args(V, T, d, L, h, dtype="bf16")
    a.sas_loss = "sampled_ce"
    with pytest.raises(ValueError, match="sas_shared_negs"):     # a missing K
        model_factory(a)
    a.sas_shared_negs = 16
    m = model_factory(a)
    assert FusedTrainStep(m).loss == "sampled_ce"
    with pytest.raises(ValueError, match="single device"):
        FusedTrainStep(m, dp=True)
    b = _step_batches(1)[0]
    t = FusedTrainStep(m, lr=1e-3)
    with pytest.raises(ValueError, match="steps_per_graph"):
        t.capture(*b, warmup=1, steps_per_graph=2)
    with pytest.raises(ValueError, match="steps_per_graph"):
        t.capture_sampled(_sampler(V, B, T, 16), warmup=1, steps_per_graph=2)
    from rbm_amd.dataloaders import DeviceWarpSampler
    import rbm_amd.data as synth
    hist = synth.user_histories(np.random.default_rng(3), 20, T, V)
    with pytest.raises(ValueError, match="shared_negs"):
        FusedTrainStep(m, lr=1e-3).capture_sampled(DeviceWarpSampler(hist, V, B, T, seed=1), warmup=1)
    over = torch.ones(ops.sas_sce_max_k() + 1, dtype=torch.int64)
    with pytest.raises(ValueError, match="candidates"):
        m.sampled_ce_loss(b[0], b[1], over)
    with pytest.raises(ValueError, match="candidates"):
        m.sampled_ce_loss(b[0], b[1], over[:0])


def test_workspace_is_not_shaped_by_the_catalogue():
    """The engine's sce_* buffers at V = 1,000 and V = 50,000, d = 64, the same batch shape and K: the same bytes."""
    T, d, L, h, B, K = 16, 64, 1, 1, 8, 100
    sizes = {}
    for V in (1000, 50000):
        m = _model(V, T, d, L, h, dtype="bf16", scale_items=0.1)
        rng = np.random.default_rng(0)
        seq, pos = (torch.from_numpy(rng.integers(1, 1001, (B, T))) for _ in range(2))
        _autograd_step(m, seq, pos, torch.from_numpy(rng.integers(1, 1001, K)))
        bufs = m.sas.engine().ws.bufs
        sizes[V] = {k: (tuple(v.shape), v.numel() * v.element_size()) for k, v in bufs.items() if k.startswith("sce_")}
        assert {"sce_ws", "sce_dh", "sce_coef", "sce_src", "sce_keys", "sce_itemidx"} <= set(sizes[V])
        assert not any(V + 1 in shape or V in shape for shape, _ in sizes[V].values())
    print("sce_* bytes", {V: sum(b for _, b in s.values()) for V, s in sizes.items()})
    assert sizes[1000] == sizes[50000]


# ================================================================ the sampler's candidates
def test_sampler_candidates():
    V, T, B, K = 50, 12, 16, 40
    s1, s2 = _sampler(V, B, T, K, seed=5), _sampler(V, B, T, K, seed=5)
    assert s1.n_outputs == 3
    a = [s1.sample() for _ in range(3)]
    b = [s2.sample() for _ in range(3)]
    plain = _sampler(V, B, T, K, seed=5)
    plain.shared_negs = None                                       # the same salt without candidates: seq / pos agree
    q = plain.sample()
    for (seq, pos, cand), (seq2, pos2, cand2) in zip(a, b):
        assert cand.shape == (K,) and cand.dtype == torch.int64
        assert int(cand.min()) >= 1 and int(cand.max()) <= V
        assert torch.equal(cand, cand2) and torch.equal(seq, seq2) and torch.equal(pos, pos2)
    assert torch.equal(a[0][0], q[0]) and torch.equal(a[0][1], q[1])
    assert not torch.equal(a[0][2], a[1][2]) and not torch.equal(a[1][2], a[2][2])
    # the host restatement of the draws (the step seed after the k-th advance is k)
    for k, (_, _, cand) in enumerate(a):
        assert (cand.cpu().numpy() == ref.uniform_items_ref(k + 1, s1.cand_salt, V, K)).all()
    # uniform: N = 200 K draws over 50 items, every count within 6 sigma of N / 50 (binomial)
    s = _sampler(V, B, T, 200 * K, seed=11)
    c = s.sample()[2].cpu().numpy()
    n, pr = c.size, 1.0 / V
    counts = np.bincount(c, minlength=V + 1)
    sigma = math.sqrt(n * pr * (1 - pr))
    print("candidate counts: worst deviation / sigma", float(np.abs(counts[1:] - n * pr).max() / sigma))
    assert counts[0] == 0 and np.abs(counts[1:] - n * pr).max() <= 6 * sigma
    with pytest.raises(ValueError):
        s.sample_into(a[0][0], a[0][1], torch.zeros(3, dtype=torch.int64, device="cuda"))


# ================================================================ learning
def test_it_learns_a_deterministic_next_item_rule():
    """The rule task of the CE test (V = 200, T = 16, d = 64, 200 steps), trained through
    DeviceWarpSampler(shared_negs=64): the users' histories are rule chains, every step's (seq, pos, cand) comes from
    the sampler.  HR@10 >= 0.5 on fresh rule sequences is 10 x the chance level 10 / V."""
    from rbm_amd.dataloaders import DeviceWarpSampler
    from rbm_amd.train_step import FusedTrainStep
    V, T, d, L, h, B, K = 200, 16, 64, 1, 1, 16, 64
    rng = np.random.default_rng(0)
    hist = []
    for _ in range(600):                                           # chains of 10 .. 17 items: 0 .. 7 leading pads
        x = [int(rng.integers(1, V + 1))]
        for _ in range(int(rng.integers(9, 17))):
            x.append((7 * x[-1] + 3) % V + 1)
        hist.append(x)
    sampler = DeviceWarpSampler(hist, V, B, T, seed=0, shared_negs=K)
    m = _model(V, T, d, L, h, dtype="bf16", seed=0)
    t = FusedTrainStep(m, lr=1e-3, loss="sampled_ce")
    losses = []
    for i in range(200):
        seq, pos, cand = sampler.sample()
        if i == 0:                                                 # the batches follow the rule
            sq, ps = seq.cpu().numpy(), pos.cpu().numpy()
            assert ((ps == (7 * sq + 3) % V + 1) | (sq == 0)).all() and (ps[sq == 0] == 0).sum() > 0
        losses.append(t.step(seq, pos, cand).clone())
    losses = [float(x.item()) for x in losses]
    seq, pos = _rule_batch(rng, 256, T)
    m.eval()
    rank = m.full_rank(seq, pos[:, -1], exclude_seen=False)
    hr10 = float((rank < 10).float().mean().item())
    print("sampled ce learns: first / last loss", losses[0], losses[-1], "HR@10", hr10)
    assert losses[-1] < losses[0], (losses[0], losses[-1])
    assert hr10 >= 0.5, hr10
