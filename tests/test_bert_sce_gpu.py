"""BERT4Rec training with the sampled softmax over batch-shared candidates, on the GPU.

* the two head launches with an output bias (rs_sce_head_fwd / rs_sce_head_bwd, sas_sce.hip) directly, every output
  element against the float64 reference (tests/bert_sce_ref.py) under derived bounds, outputs NaN-filled and guarded:
  the bf16 MFMA sweep at d = 256 (and a width padded inside its fragments), the narrower sweeps, the plain kernel;
  bias = NULL bitwise against the rs_sas_sce_* entries; the scattered bias gradient;
* ``BERTModel.sampled_ce_loss`` + autograd in fp32 (tests/test_bert.py's fp32 bars) and one fused bf16 step against the
  float64 reference with the step's dropout masks replayed (tests/test_bert.py's bf16 bars);
* ``FusedTrainStep(loss="sampled_ce")``: against sampled_ce_loss + the fused Adam (bit for bit), graph capture against
  eager steps (bit for bit), reproducibility, ``DeviceBertMasker(shared_negs=K)`` captured with the step;
* the default loss' step is unchanged, the gradient contract, the errors, the V-free workspace, and a deterministic
  next-item rule is learnt about as well as with the full cross-entropy.

The bounds of the head kernels are those of tests/test_sas_sce_gpu.py (its docstring has the derivation), with two
changes that the bias makes.  Every magnitude sum gains its |b| term (Z_rj = sum_k |h_rk| |E_jk| + |b_j|: the reference
computes them so), and every logit carries one more fp32 addition, hence one more rounding of a value bounded by Z:

    z_r0   : (d + 3) u Z_r0
    lse_r  : u ((d + 5) Zmax_r + nlive_r + 16 + splits + |lse_r|)
    e_r    = 1.01 (lse bar + (d + 5) u Zmax_r + 4 u)
    coef, pg, dh, dEc: as there, on these e_r
    dbc_j  : |s| (sum_r p_rj e_r + (n + 68) u P_j) + u |dbc_j|,   P_j = sum_r p_rj
             (p's relative error e_r; n rows summed in fp32 in a fixed order, up to 64 split slabs and the reduction;
             no bf16 term: the probabilities are summed before they are rounded for the MFMA)
Each head test prints its worst error / bar per output (pytest -s).
"""
import argparse
import math
import types

import numpy as np
import pytest
import torch

import bert_sce_ref as ref
from conftest import rel
from test_bert import FWD_TOL_BF16, FWD_TOL_F32, GRAD_TOL_BF16, GRAD_TOL_F32

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
GUARD = 8
SENT = -7
U = 2.0 ** -24
TILE = 64          # the kernel's tile size (sas_sce.hip TS)
V_HEAD = 300


def _nan(shape, dt=F32):
    return torch.full(shape, math.nan, dtype=dt, device="cuda")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ================================================================ the head kernels
def _head_problem(dt, d, rows, K, pattern, seed, dense=False, empty=False):
    """hl [cap][d], E [V + 1][d], bias [V + 1], lab [cap], cand [K].  Patterns: mixed (id-0 slots, a duplicate), hits
    (every candidate is 0 or row 0's label: that row and every row sharing the label has no live candidate, the others
    do; one row: a hit, an id-0 slot and a duplicated live candidate), big (|z| past 88), bias_big (|b| >> |<h, E>|)."""
    rng = np.random.default_rng(seed)
    V = V_HEAD
    cap = rows + 9
    hl = torch.from_numpy(rng.standard_normal((cap, d))).to(dt)
    E = torch.from_numpy(rng.standard_normal((V + 1, d)) * ((36.0 if pattern == "big" else 1.0) / math.sqrt(d))).to(dt)
    bias = rng.standard_normal(V + 1) * (25.0 if pattern == "bias_big" else 1.0)
    bias = torch.from_numpy(bias).float()
    lab = rng.integers(1, V + 1, cap)
    if dense:
        lab[rng.random(cap) < 0.4] = 0                           # all rows given, lab 0 = no row
        lab[0] = 5
    if empty:
        lab[:] = 0
    if pattern == "hits" and rows > 1:
        cand = np.where(rng.random(K) < 0.3, 0, lab[0])
        cand[0] = lab[0]
        if K > 1:
            cand[-1] = 0
    elif pattern == "hits":
        other = lab[0] % V + 1
        cand = np.array(([lab[0], 0, other, other] * K)[:K]) if K > 1 else np.array([other])
    else:
        cand = rng.integers(1, V + 1, K)
        cand[rng.random(K) < 0.15] = 0                            # ignored slots
        if K > 3:
            cand[K // 2] = cand[0]                                # a duplicate for certain
        if not (cand != 0).any():
            cand[0] = lab[0] % V + 1
    if pattern == "big":
        # a logit of 100 for certain, whatever the draw: one candidate's row along row 0 of hl (|z| = Z there, so the
        # bars stay in the first-order regime they are derived in)
        h0 = hl[0].double()
        E[int(cand[np.nonzero(cand)[0][0]])] = (h0 * (100.0 / float((h0 * h0).sum()))).to(dt)
    return V, cap, hl, E, bias, lab, cand


def _check_inputs(lab, count, cand, pattern, rows, empty):
    """A degenerate draw must not pass silently."""
    l = lab[:count]
    live = (cand != 0)[None, :] & (cand[None, :] != l[:, None]) & (l != 0)[:, None]
    if empty:
        assert not (l != 0).any()
        return
    assert (l != 0).any(), "no valid row"
    assert live.any(), "no live pair"
    if pattern == "hits" and rows > 1:
        assert ((l != 0) & ~live.any(-1)).any(), "no row without a live candidate"
        assert (cand == 0).any() or cand.size == 1
    if pattern == "hits":
        assert np.isin(cand, l).any() or cand.size == 1, "no candidate equal to a label"


def _run_head(dt, d, rows, K, pattern, seed, dense=False, empty=False, with_bias=True):
    from rbm_amd import ops
    V, cap, hl, E, bias, lab, cand = _head_problem(dt, d, rows, K, pattern, seed, dense, empty)
    count = cap if dense else rows
    _check_inputs(lab, count, cand, pattern, rows, empty)
    fmt = 2.0 ** -7 if dt == BF else 0.0
    hl_d, E_d, lab_d, cand_d = hl.cuda(), E.cuda(), _dev(lab), _dev(cand)
    b_d = bias.cuda() if with_bias else None
    cnt = None if dense else torch.tensor([rows], dtype=torch.int32, device="cuda")
    nvalid = int((lab[:count] != 0).sum())
    div = torch.tensor([float(max(nvalid, 1))], device="cuda")
    dloss = torch.tensor([0.75], device="cuda")
    nws = ops.sce_head_ws_numel(cap, K, d, dt, with_bias)
    ws = _nan((nws + GUARD,))
    out = _nan((4,))
    ops.sce_head_fwd(hl_d, lab_d, cnt, cap, E_d, b_d, cand_d, div, ws[:nws], out)
    ks = ops.sce_head_dh_splits(cap, K, d, dt)
    assert 1 <= ks <= max(1, -(-K // TILE))
    dh, coef = _nan((ks * cap + GUARD, d)), _nan((cap + GUARD,))
    src, dbc = _nan((cap + K + GUARD, d)), _nan((K + GUARD,))
    keys = torch.full((cap + K + GUARD,), SENT, dtype=torch.int64, device="cuda")
    ops.sce_head_bwd(hl_d, lab_d, cnt, cap, E_d, b_d, cand_d, div, dloss, ws[:nws], dh, coef, src[:cap],
                     src[cap:cap + K], dbc[:K] if with_bias else None, keys)
    torch.cuda.synchronize()
    # ---- float64 on the kernels' own inputs
    hl64, E64 = hl.double().numpy(), E.double().numpy()
    b64 = bias.double().numpy() if with_bias else None
    dv = float(div.item())
    lse, z0, rout = ref.head_fwd_ref(hl64, lab, count, E64, b64, cand, dv)
    rdh, rcoef, rpg, rdEc, rdbc, rkeys, mag = ref.head_bwd_ref(hl64, lab, count, E64, b64, cand, dv, 0.75)
    s = 0.75 / dv
    valid = lab[:count] != 0
    zmax = np.maximum(mag["z0"], mag["z"].max(-1)) * valid
    bar_z0 = (d + 3) * U * mag["z0"] * valid
    bar_lse = U * ((d + 5) * zmax + mag["nlive"] + 16 + ks + np.abs(lse)) * valid
    e_r = 1.01 * (bar_lse + (d + 5) * U * zmax + 4 * U)
    assert e_r.max() < 2e-2
    bar_coef = abs(s) * (mag["p0"] * e_r + 4 * U) * valid
    Epos = np.abs(E64[np.where(valid, lab[:count], 0)])
    cc = np.where((cand <= 0) | (cand > V), 0, cand)
    z = hl64[:count] @ E64[cc].T + (b64[cc][None, :] if with_bias else 0.0)
    live = (cc != 0)[None, :] & (cc[None, :] != lab[:count, None]) & valid[:, None]
    P = np.where(live, np.exp(np.where(live, z, 0.0) - lse[:, None]), 0.0)
    H = np.abs(hl64[:count])
    A = abs(s) * (P @ np.abs(E64[cc]))
    bar_dh = (e_r[:, None] + (K + 4 + ks) * U + fmt) * A + bar_coef[:, None] * Epos + U * np.abs(rdh)
    bar_pg = bar_coef[:, None] * H + U * np.abs(rpg)
    bar_dEc = abs(s) * ((P * e_r[:, None]).T @ H + ((count + 68) * U + fmt) * (P.T @ H)) + U * np.abs(rdEc)
    bar_dbc = abs(s) * ((P * e_r[:, None]).sum(0) + (count + 68) * U * P.sum(0)) + U * np.abs(rdbc)
    got = dict(lse=ws[:count].double().cpu().numpy(), z0=ws[cap:cap + count].double().cpu().numpy(),
               dh=dh[:ks * cap].view(ks, cap, d)[:, :count].double().sum(0).cpu().numpy(),
               coef=coef[:count].double().cpu().numpy(), pg=src[:count].double().cpu().numpy(),
               dEc=src[cap:cap + K].double().cpu().numpy())
    want = dict(lse=(lse, bar_lse), z0=(z0, bar_z0), dh=(rdh, bar_dh), coef=(rcoef, bar_coef), pg=(rpg, bar_pg),
                dEc=(rdEc, bar_dEc))
    if with_bias:
        got["dbc"] = dbc[:K].double().cpu().numpy()
        want["dbc"] = (rdbc, bar_dbc)
    res = {}
    for k, (w, bar) in want.items():
        err = np.abs(got[k] - w)
        assert np.isfinite(got[k]).all(), k
        res[k] = float((err / np.maximum(bar, 1e-30)).max()) if err.size else 0.0
        assert (err[bar == 0] == 0).all(), k                      # nothing to round: exact (a masked row's zeros)
    o = out.double().cpu().numpy()
    bar_sum = float((bar_lse + bar_z0).sum()) + U * abs(rout[0])
    res["out.sum"] = abs(o[0] - rout[0]) / max(bar_sum, 1e-30) if bar_sum else float(o[0] != rout[0])
    res["out.mean"] = abs(o[2] - rout[2]) / max(bar_sum / dv + 2 * U * abs(rout[2]), 1e-30) \
        if bar_sum else float(o[2] != rout[2])
    assert o[1] == rout[1] == nvalid
    # ---- rows at or past the count, and the guards: untouched
    assert torch.isnan(ws[count:cap]).all() and torch.isnan(ws[cap + count:2 * cap]).all() and torch.isnan(ws[nws:]).all()
    assert torch.isnan(dh[:ks * cap].view(ks, cap, d)[:, count:]).all() and torch.isnan(dh[ks * cap:]).all()
    assert torch.isnan(coef[count:]).all()
    assert torch.isnan(src[count:cap]).all() and torch.isnan(src[cap + K:]).all()
    assert torch.isnan(dbc[K:]).all() and (with_bias or torch.isnan(dbc).all())
    assert torch.isnan(out[3])
    k = keys.cpu().numpy()
    assert (k[:cap + K] == rkeys).all() and (k[cap + K:] == SENT).all()
    if dense or empty:                                            # lab 0 = no row: exactly-zero outputs there
        dead = ~valid
        for name in ("lse", "z0", "dh", "coef", "pg"):
            assert not got[name][dead].any(), name
    if empty:
        assert not o[:3].any() and not got["dEc"].any() and not got.get("dbc", np.zeros(1)).any()
    return res


def _check_head(tag, res):
    print(tag, "err/bar:", ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
    bad = {k: v for k, v in res.items() if v > 1.0}
    assert not bad, bad


def test_head_paths():
    from rbm_amd import ops
    assert [ops.sce_head_path(d, BF) for d in (64, 128, 136, 200, 256, 264)] == [1, 1, 1, 1, 1, 0]
    assert [ops.sce_head_path(d, F32) for d in (50, 64, 128, 256)] == [1, 1, 1, 0]


@pytest.mark.parametrize("pattern", ["mixed", "hits", "big", "bias_big"])
@pytest.mark.parametrize("K", [1, 65, 257])
@pytest.mark.parametrize("rows", [1, 17, 129])
def test_head_bf16_mfma_sweep_at_256(rows, K, pattern):
    """rows: a partial wave, a partial tile, 3 row tiles (row-split slabs of dEc / dbc); K: a partial tile, 2 tiles,
    5 tiles (candidate splits of the forward and dh).  big: the largest |z| is past 88, where exp(z) alone overflows
    fp32.  bias_big: |b| ~ 25 against |<h, E>| ~ 1, so a bias missing at the positive or at the candidates moves lse
    and every probability grossly, far past any rounding bar."""
    d = 256
    V, cap, hl, E, bias, lab, cand = _head_problem(BF, d, rows, K, pattern, seed=rows + K)
    zz = hl.double()[:rows] @ E.double()[cand].T
    if pattern == "big":
        assert float(zz.abs().max()) > 88
    if pattern == "bias_big":
        live_b = bias.double()[cand][cand != 0].abs()
        assert float(live_b.max()) > 10 * float(zz.abs().median()) and float(bias[lab[:rows]].abs().max()) > 5
    _check_head(f"head bf16 sweep256 {pattern} rows={rows} K={K}", _run_head(BF, d, rows, K, pattern, seed=rows + K))


@pytest.mark.parametrize("pattern", ["mixed", "hits"])
@pytest.mark.parametrize("d", [136, 200])
def test_head_bf16_mfma_sweep_width_padded_inside_the_fragments(d, pattern):
    _check_head(f"head bf16 sweep256 {pattern} d={d}", _run_head(BF, d, 129, 257, pattern, seed=d))
    _check_head(f"head bf16 sweep256 {pattern} d={d} small", _run_head(BF, d, 17, 65, pattern, seed=d + 1))


@pytest.mark.parametrize("rows,K", [(17, 65), (129, 257)])
@pytest.mark.parametrize("dt,d", [(BF, 64), (BF, 128), (F32, 50), (F32, 64), (F32, 128)])
def test_head_narrow_sweeps_with_bias(dt, d, rows, K):
    for pattern in ("mixed", "bias_big"):
        _check_head(f"head {dt} {pattern} d={d} rows={rows} K={K}", _run_head(dt, d, rows, K, pattern, seed=d + K))


@pytest.mark.parametrize("rows,K", [(1, 1), (17, 65)])
@pytest.mark.parametrize("dt,d", [(F32, 256), (BF, 264)])
def test_head_plain_kernel_with_bias(dt, d, rows, K):
    for pattern in ("mixed", "hits", "bias_big"):
        _check_head(f"head plain {dt} {pattern} d={d} rows={rows} K={K}",
                    _run_head(dt, d, rows, K, pattern, seed=d + rows + K))


@pytest.mark.parametrize("dt,d", [(BF, 64), (BF, 128), (F32, 50), (F32, 128)])
def test_head_without_bias_equals_the_tied_entries_bitwise(dt, d):
    """bias = NULL: every output and the whole workspace are the rs_sas_sce_* entries' bits."""
    from rbm_amd import ops
    rows, K = 129, 257
    V, cap, hl, E, bias, lab, cand = _head_problem(dt, d, rows, K, "mixed", seed=d)
    hl_d, E_d, lab_d, cand_d = hl.cuda(), E.cuda(), _dev(lab), _dev(cand)
    cnt = torch.tensor([rows], dtype=torch.int32, device="cuda")
    div, dloss = torch.tensor([float(rows)], device="cuda"), torch.tensor([0.75], device="cuda")
    nws = ops.sas_sce_ws_numel(cap, K, d)
    assert nws == ops.sce_head_ws_numel(cap, K, d, dt, False)
    ks = ops.sas_sce_dh_splits(cap, K, d)
    assert ks == ops.sce_head_dh_splits(cap, K, d, dt)
    res = []
    for new in (False, True):
        ws, out = _nan((nws,)), _nan((4,))
        dh, coef, src = _nan((ks * cap, d)), _nan((cap,)), _nan((cap + K, d))
        keys = torch.full((cap + K,), SENT, dtype=torch.int64, device="cuda")
        if new:
            ops.sce_head_fwd(hl_d, lab_d, cnt, cap, E_d, None, cand_d, div, ws, out)
            ops.sce_head_bwd(hl_d, lab_d, cnt, cap, E_d, None, cand_d, div, dloss, ws, dh, coef, src[:cap], src[cap:],
                             None, keys)
        else:
            ops.sas_sce_fwd(hl_d, lab_d, cnt, cap, E_d, cand_d, div, ws, out)
            ops.sas_sce_bwd(hl_d, lab_d, cnt, cap, E_d, cand_d, div, dloss, ws, dh, coef, src[:cap], src[cap:], keys)
        torch.cuda.synchronize()
        res.append([t.view(torch.int32) if t.dtype == F32 else t for t in (ws, out, dh, coef, src, keys)])
    for name, a, b in zip(("ws", "out", "dh", "coef", "src", "keys"), *res):
        assert torch.equal(a, b), name                            # bit patterns (NaN fill included)
    assert not torch.isnan(res[0][1].view(F32)[:3]).any()


@pytest.mark.parametrize("dt,d", [(BF, 256), (BF, 64), (F32, 50), (F32, 256)])
def test_head_all_rows_with_lab_zero_as_no_row(dt, d):
    """count NULL: every row is given, lab 0 marks the rows to skip -- exactly-zero outputs there."""
    _check_head(f"head dense d={d}", _run_head(dt, d, 129, 129, "mixed", seed=d, dense=True))


@pytest.mark.parametrize("dt,d", [(BF, 256), (F32, 64), (BF, 264)])
def test_head_batch_with_no_valid_row(dt, d):
    res = _run_head(dt, d, 17, 65, "mixed", seed=d, dense=True, empty=True)
    assert not any(res.values()), res


def test_head_unsupported_and_bad_arguments_launch_nothing():
    import rbm_amd._lib as L
    lib = L.lib()
    s = torch.cuda.current_stream().cuda_stream
    kmax = lib.rs_sas_sce_max_k()

    def codes(dtype, d, tdt, K, Kbuf=None, bias=True, dbc=True, ldh=None):
        cap = 8
        hl, E = torch.zeros(cap, d, dtype=tdt, device="cuda"), torch.zeros(20, d, dtype=tdt, device="cuda")
        lab = torch.ones(cap, dtype=torch.int64, device="cuda")
        cand = torch.ones(Kbuf or max(K, 1), dtype=torch.int64, device="cuda")
        div, b = torch.ones(1, device="cuda"), torch.zeros(20, device="cuda")
        ws, out = _nan((4096,)), _nan((4,))
        dh, coef, pg, dEc = _nan((16 * cap, d)), _nan((cap,)), _nan((cap, d)), _nan((max(Kbuf or K, 1), d))
        db = _nan((max(Kbuf or K, 1),))
        keys = torch.full((cap + (Kbuf or max(K, 1)),), SENT, dtype=torch.int64, device="cuda")
        p = lambda t: t.data_ptr()  # noqa: E731
        a = lib.rs_sce_head_fwd(dtype, cap, d, p(hl), ldh or d, p(lab), None, p(E), p(b) if bias else None, 20, p(cand),
                                K, p(div), p(ws), p(out), s)
        c = lib.rs_sce_head_bwd(dtype, cap, d, p(hl), ldh or d, p(lab), None, p(E), p(b) if bias else None, 20, p(cand),
                                K, p(div), None, p(ws), p(dh), p(coef), p(pg), p(dEc), p(db) if dbc else None, p(keys),
                                s)
        torch.cuda.synchronize()
        for t in (dh, coef, pg, dEc, db) + ((ws, out) if a else ()):
            assert torch.isnan(t).all()
        assert (keys == SENT).all()
        return a, c
    assert codes(7, 64, F32, 4) == (1002, 1002)                   # no such dtype
    assert codes(L.BF16, 50, BF, 4) == (1002, 1002)               # bf16 rows that are no multiple of 16 bytes
    assert codes(L.BF16, 1032, BF, 4) == (1002, 1002)
    assert codes(L.F32, 1025, F32, 4) == (1002, 1002)
    assert codes(L.BF16, 256, BF, 0) == (1002, 1002)
    assert codes(L.BF16, 256, BF, kmax + 1, Kbuf=4) == (1002, 1002)
    assert codes(L.BF16, 256, BF, 4, ldh=128) == (1001, 1001)     # rows narrower than d
    assert codes(L.BF16, 256, BF, 4, dbc=False) == (0, 1001)      # a bias without dbc (the forward is a valid call)
    assert codes(L.F32, 64, F32, 4, bias=False) == (0, 1001)      # dbc without a bias


@pytest.mark.parametrize("dt,d", [(BF, 256), (F32, 64)])
def test_scattered_bias_gradient(dt, d):
    """db[v] += the entries of {coef at lab_r, dbc at cand_j} keyed v, through the index built for the weights'
    scatter (rs_item_grad_f32 at d = 1): against float64 -- each entry's own bar summed, plus one rounding per added
    entry -- into a non-zero db, key 0 untouched, and the same bits on a second run."""
    from rbm_amd import ops
    from rbm_amd.models.bert_model.bert import SCE_INDEX_ROWS
    rows, K = 129, 257
    V, cap, hl, E, bias, lab, cand = _head_problem(dt, d, rows, K, "mixed", seed=11)
    cand[:40] = lab[:40]                                          # keys met as a label and as a candidate
    cand[40:44] = 0
    hl_d, E_d, b_d, lab_d, cand_d = hl.cuda(), E.cuda(), bias.cuda(), _dev(lab), _dev(cand)
    cnt = torch.tensor([rows], dtype=torch.int32, device="cuda")
    div = torch.tensor([float(rows)], device="cuda")
    ws = torch.zeros(ops.sce_head_ws_numel(cap, K, d, dt), device="cuda")
    out = torch.zeros(4, device="cuda")
    ks = ops.sce_head_dh_splits(cap, K, d, dt)
    trow = max(V + 1, SCE_INDEX_ROWS)
    runs = []
    for _ in range(2):
        dh, src = torch.zeros(ks, cap, d, device="cuda"), torch.zeros(cap + K, d, device="cuda")
        bsrc = torch.zeros(cap + K, device="cuda")
        keys = torch.zeros(cap + K, dtype=torch.int64, device="cuda")
        ops.sce_head_fwd(hl_d, lab_d, cnt, cap, E_d, b_d, cand_d, div, ws, out)
        ops.sce_head_bwd(hl_d, lab_d, cnt, cap, E_d, b_d, cand_d, div, None, ws, dh, bsrc[:cap], src[:cap], src[cap:],
                         bsrc[cap:], keys)
        iws = torch.zeros(ops.item_index_ws_bytes(1, cap + K, trow, d), dtype=torch.uint8, device="cuda")
        ops.item_index_build([keys], trow, d, iws)
        dW = torch.zeros(V + 1, d, device="cuda")
        db = torch.full((V + 1,), 0.5, device="cuda")
        sb = torch.zeros(1, dtype=torch.int64, device="cuda")
        ops.item_grad(iws, 1, cap + K, src, 1.0, 0.0, 0, sb, None, None, None, dW, table_rows=trow)
        ops.item_grad(iws, 1, cap + K, bsrc.view(-1, 1), 1.0, 0.0, 0, sb, None, None, None, db.view(-1, 1),
                      table_rows=trow)
        torch.cuda.synchronize()
        runs.append((db.clone(), dW.clone(), bsrc.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    hl64, E64, b64 = hl.double().numpy(), E.double().numpy(), bias.double().numpy()
    _, rcoef, rpg, rdEc, rdbc, rkeys, _ = ref.head_bwd_ref(hl64, lab, rows, E64, b64, cand, float(rows))
    want = ref.scatter_bias_grad(V + 1, cap, rkeys, rcoef, rdbc) + 0.5
    want[0] = 0.5
    # the entries' own errors (checked against their bars above; here: as measured) carried through the sums, plus one
    # fp32 rounding per addition of an entry, on the sum of the magnitudes
    ent = runs[0][2].double().cpu().numpy()
    ent_ref = np.concatenate([rcoef, np.zeros(cap - rows), rdbc])
    err_ent = ref.scatter_bias_grad(V + 1, cap, rkeys, np.abs(ent - ent_ref)[:rows], np.abs(ent - ent_ref)[cap:])
    n_ent = ref.scatter_bias_grad(V + 1, cap, rkeys, np.ones(rows), np.ones(K))
    mag = ref.scatter_bias_grad(V + 1, cap, rkeys, np.abs(rcoef), np.abs(rdbc)) + 0.5
    bar = err_ent + (n_ent + 1) * U * mag
    got = runs[0][0].double().cpu().numpy()
    err = np.abs(got - want)
    print(f"scattered db {dt} d={d}: worst err / bar", float((err / np.maximum(bar, 1e-30)).max()),
          "keys with several entries", int((n_ent > 1).sum()))
    assert (n_ent > 1).sum() >= 40 and got[0] == 0.5
    assert (err <= bar).all()
    dWr = np.zeros((V + 1, d))
    np.add.at(dWr, rkeys[:rows], rpg)
    np.add.at(dWr, rkeys[cap:], rdEc)
    dWr[0] = 0
    assert rel(runs[0][1].double().cpu().numpy(), dWr) < (1e-2 if dt == BF else 1e-5)


# ================================================================ the model
def _model(V, T, d, L, h, p=0.0, dtype="fp32", seed=0, **kw):
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    torch.manual_seed(V + T + seed)                               # the engine's dropout-site salts
    a = argparse.Namespace(model_code="bert", num_items=V, max_len=T, device="cuda", bert_hidden_units=d,
                           bert_num_blocks=L, bert_num_heads=h, bert_dropout=p, bert_hidden_dropout=p,
                           bert_mask_prob=0.2, model_init_seed=seed, rs_dtype=dtype, **kw)
    m = model_factory(a)
    with torch.no_grad():
        g = torch.Generator().manual_seed(seed + 1)
        m.out.bias.copy_(torch.randn(V + 1, generator=g) * 0.5)   # nn.Linear's bias init is tiny at these widths
    m.train()
    return m


def _P(m):
    return {k: v.detach().cpu().double() for k, v in m.state_dict().items()}


def _batch(V, T, B, seed=0, mask_prob=0.3):
    import rbm_amd.data as synth
    rng = np.random.default_rng(seed + T)
    tok, lab = synth.bert_batch(rng, B, T, V, mask_prob=mask_prob)
    lab[0, -1], tok[0, -1] = V, V + 1                             # the label V forced in
    assert (lab != 0).sum() >= 2
    return torch.from_numpy(tok), torch.from_numpy(lab)


def _cand(V, K, seed=0):
    if K == V + 1:
        return torch.arange(1, V + 2)                             # every item, and the id past out.weight's rows
    rng = np.random.default_rng(seed + K)
    c = rng.integers(1, V + 1, K)
    if K > 4:
        c[1] = 0
        c[3] = c[2]
        c[4] = V                                                  # _batch forces the label V in: an accidental hit
    return torch.from_numpy(c)


def _autograd_step(m, tok, lab, cand):
    m.zero_grad(set_to_none=True)
    loss = m.sampled_ce_loss(tok.numpy(), lab, cand)              # numpy and tensor ids
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.item()), {k: q.grad.detach().cpu().numpy() for k, q in m.named_parameters()}


def _check_grads_f32(grads, g64, tol):
    scale = max(float(v.norm()) for v in g64.values())
    for k, r in g64.items():
        g = grads[k]
        if "linear_layers.1.bias" in k or float(r.norm()) == 0:  # the key bias: analytically zero
            assert np.linalg.norm(g) <= 1e-5 * scale, k
            continue
        assert rel(g, r.numpy()) < tol, (k, rel(g, r.numpy()))


@pytest.mark.parametrize("Ksel", ["1", "50", "V+1"])
@pytest.mark.parametrize("V,T,d,L,h,B", [(60, 12, 32, 1, 2, 4), (500, 50, 64, 2, 2, 3)])
def test_sampled_ce_loss_fp32_matches_float64_reference(V, T, d, L, h, B, Ksel):
    K = V + 1 if Ksel == "V+1" else int(Ksel)
    m = _model(V, T, d, L, h)
    tok, lab = _batch(V, T, B)
    cand = _cand(V, K)
    loss, grads = _autograd_step(m, tok, lab, cand)
    l64, g64 = ref.sce_loss_and_grads(_P(m), tok, lab, cand, L, h)
    print((V, T, d, K), "loss", loss, "ref", l64.item(), "worst",
          sorted(((rel(grads[k], g64[k].numpy()), k) for k in grads if "linear_layers.1.bias" not in k), reverse=True)[:2])
    assert abs(loss - l64.item()) < FWD_TOL_F32 * max(1.0, abs(l64.item())), (loss, l64.item())
    _check_grads_f32(grads, g64, GRAD_TOL_F32)
    touched = set(lab.reshape(-1).tolist()) | set(cand.tolist())
    rest = [v for v in range(V + 1) if v not in touched or v == 0]
    assert not grads["out.weight"][rest].any() and not grads["out.bias"][rest].any()


def test_all_unlabelled_batch_gives_zero_loss_and_gradients():
    for dtype in ("fp32", "bf16"):
        m = _model(60, 12, 64, 1, 2, dtype=dtype)
        tok = torch.from_numpy(np.random.default_rng(0).integers(1, 61, (2, 12)))
        loss, grads = _autograd_step(m, tok, torch.zeros_like(tok), torch.arange(1, 9))
        assert loss == 0.0 and all(not g.any() for g in grads.values()), dtype


def test_sampled_ce_loss_bf16_other_width_needs_fp32_mode():
    m = _model(40, 8, 36, 1, 2, dtype="bf16")
    tok, lab = _batch(40, 8, 2)
    with pytest.raises(ValueError, match="fp32"):
        m.sampled_ce_loss(tok, lab, torch.arange(1, 9))


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("d", [64, 128, 256])
def test_fused_bf16_step_matches_float64_reference(d, p):
    """One fused bf16 step (FusedTrainStep._compute, before the optimizer) against the float64 reference with the
    step's dropout masks replayed, under the project's bars for the CE step."""
    from rbm_amd.train_step import FusedTrainStep
    from test_dropout_parity_gpu import bert_masks
    V, T, L, h, B, K = 500, 50, 1, 2, 8, 65
    m = _model(V, T, d, L, h, p=p, dtype="bf16", seed=1)
    tok, lab = _batch(V, T, B)
    cand = _cand(V, K)
    tr = FusedTrainStep(m, lr=0.0, loss="sampled_ce")
    seed = 4242
    tr.engine.seed_base.fill_(seed)
    tr.flat.grad.zero_()
    tr._compute(tok.cuda(), lab.cuda(), cand.cuda())
    torch.cuda.synchronize()
    loss = float(tr.loss_out[2].item())
    assert float(tr.loss_out[1].item()) == int((lab != 0).sum())
    from rbm_amd import ops
    assert ops.sce_head_path(d, BF) == 1 and "sce_ws" in tr.engine.ws.bufs and "dlogits" not in tr.engine.ws.bufs
    sb = torch.full((1,), seed, dtype=torch.int64, device="cuda")
    masks = {k: v.cpu().double() for k, v in bert_masks(tr.engine, B, T, sb).items()} if p > 0 else None
    l64, g64 = ref.sce_loss_and_grads(_P(m), tok, lab, cand, L, h, p=p, hp=p, masks=masks)
    scale = max(float(g.norm()) for g in g64.values())
    worst = {}
    for k, r in g64.items():
        g = tr.flat.view(k, tr.flat.grad).cpu().double()
        if "linear_layers.1.bias" in k:
            assert float(g.norm()) <= 1e-2 * scale, k
            continue
        worst[k] = rel(g.numpy(), r.numpy())
    print((d, p), "loss", loss, "ref", l64.item(), "worst", max(worst.items(), key=lambda kv: kv[1]))
    assert abs(loss - l64.item()) < FWD_TOL_BF16 * abs(l64.item()), (loss, l64.item())
    bad = {k: v for k, v in worst.items() if v >= GRAD_TOL_BF16}
    assert not bad, bad


# ================================================================ the fused step
STEP = (300, 24, 64, 1, 2, 8)
K_STEP = 50


def _step_model(dtype="bf16", p=0.1, seed=1, loss="sampled_ce", **kw):
    from rbm_amd.train_step import FusedTrainStep
    V, T, d, L, h, B = STEP
    m = _model(V, T, d, L, h, p=p, dtype=dtype, seed=seed)
    return m, FusedTrainStep(m, lr=1e-3, loss=loss, **kw)


def _step_batches(n):
    V, T, d, L, h, B = STEP
    out = []
    for i in range(n):
        tok, lab = _batch(V, T, B, seed=100 + i)
        out.append((tok.cuda(), lab.cuda(), _cand(V, K_STEP, seed=i).cuda()))
    return out


def test_fused_step_equals_sampled_ce_loss_plus_fused_adam_bit_for_bit():
    """Both forms run the same kernels on the same seeds: the parameters after one step are the same bits."""
    b = _step_batches(1)[0]
    m1, t1 = _step_model()
    m2, t2 = _step_model()
    assert t1.loss == "sampled_ce" and not t1._early_ok and t1.engine.overwritten_grads() is None
    t1.engine.seed_base.fill_(77)
    t2.engine.seed_base.fill_(77)
    l1 = float(t1.step(*b).item())
    loss = m2.sampled_ce_loss(*b)
    loss.backward()
    for n, q in m2.named_parameters():
        t2.flat.view(n, t2.flat.grad).copy_(q.grad)
    t2._update()
    torch.cuda.synchronize()
    assert l1 == float(loss.item()) and np.isfinite(l1)
    assert torch.equal(t1.flat.data, t2.flat.data)
    assert int(t1.engine.seed_base.item()) == int(t2.engine.seed_base.item()) == 78
    assert float(t1.flat.grad.abs().sum()) == 0                   # the whole buffer is zeroed again: no kept range


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


def _masker(V, B, T, K, seed=9, users=100):
    from rbm_amd.dataloaders import DeviceBertMasker
    import rbm_amd.data as synth
    hist = synth.user_histories(np.random.default_rng(3), users, T, V)
    return DeviceBertMasker(hist, V, B, T, 0.3, seed=seed, shared_negs=K)


def test_sampled_capture_runs_with_shared_negs():
    V, T, d, L, h, B = STEP
    runs = []
    for _ in range(2):
        m, t = _step_model()
        t.capture_sampled(_masker(V, B, T, K_STEP), warmup=2)
        losses = [float(t.replay_sampled().item()) for _ in range(3)]
        runs.append((losses, t.flat.data.clone()))
    assert runs[0][0] == runs[1][0] and all(np.isfinite(runs[0][0]))
    assert len(set(runs[0][0])) == 3                              # fresh batches and candidates every replay
    assert t.packed is None                                       # no packed buffer that would leave cand stale
    assert torch.equal(runs[0][1], runs[1][1])


def test_masker_candidates():
    V, T, B, K = 50, 12, 16, 40
    s1, s2 = _masker(V, B, T, K, seed=5), _masker(V, B, T, K, seed=5)
    assert s1.n_outputs == 3
    a = [s1.sample() for _ in range(3)]
    b = [s2.sample() for _ in range(3)]
    from rbm_amd.dataloaders import DeviceBertMasker
    import rbm_amd.data as synth
    plain = DeviceBertMasker(synth.user_histories(np.random.default_rng(3), 100, T, V), V, B, T, 0.3, seed=5)
    assert plain.n_outputs == 2 and plain.salt == s1.salt
    q = plain.sample()
    for (tok, lab, cand), (tok2, lab2, cand2) in zip(a, b):
        assert cand.shape == (K,) and cand.dtype == torch.int64
        assert int(cand.min()) >= 1 and int(cand.max()) <= V
        assert torch.equal(cand, cand2) and torch.equal(tok, tok2) and torch.equal(lab, lab2)
    assert torch.equal(a[0][0], q[0]) and torch.equal(a[0][1], q[1])       # the same tokens / labels without candidates
    assert not torch.equal(a[0][2], a[1][2]) and not torch.equal(a[1][2], a[2][2])
    # the host restatement of the draws (the step seed after the k-th advance is k)
    for k, (_, _, cand) in enumerate(a):
        assert int(s1.state[0].item()) == 3
        assert (cand.cpu().numpy() == ref.uniform_items_ref(k + 1, s1.cand_salt, V, K)).all()
    with pytest.raises(ValueError):
        s1.sample_into(a[0][0], a[0][1], torch.zeros(3, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        s1.sample_into(a[0][0], a[0][1])


# ================================================================ existing behaviour, contract, errors, memory
def test_default_loss_step_is_unchanged_by_the_argument():
    """A model built with bert_loss="ce" and one built without the argument: the same bits after three fused steps
    (the default path takes no new branch)."""
    import rbm_amd.data as synth
    from rbm_amd.train_step import FusedTrainStep
    V, T, d, L, h, B = STEP
    rng = np.random.default_rng(3)
    batches = [tuple(torch.from_numpy(t).cuda() for t in synth.bert_batch(rng, B, T, V, mask_prob=0.2)) for _ in range(3)]
    res = []
    for kw, loss in (({}, None), ({"bert_loss": "ce"}, None)):
        m = _model(V, T, d, L, h, p=0.1, dtype="bf16", seed=2, **kw)
        tr = FusedTrainStep(m, lr=1e-3, loss=loss)
        assert tr.loss is None and tr.engine.loss == "ce"
        tr.engine.seed_base.fill_(9)
        losses = [float(tr.step(*b).item()) for b in batches]
        torch.cuda.synchronize()
        res.append((losses, tr.flat.data.clone(), tr.opt.m.clone(), tr.opt.v.clone()))
        assert "sce_ws" not in tr.engine.ws.bufs
    for other in res[1:]:
        assert other[0] == res[0][0]
        assert all(torch.equal(a, b) for a, b in zip(res[0][1:], other[1:]))


def test_overwritten_grads_contract():
    """None under the sampled loss at any size; under CE unchanged: None below 2^24 head elements, the out.weight /
    out.bias range from there on -- checked on the method itself with the shape arithmetic alone (no 1M-row table)."""
    from rbm_amd.models.bert_model.bert import BERTEngine
    m, t = _step_model()
    assert t.engine.overwritten_grads() is None and t.engine.loss == "sampled_ce" and not t._early_ok
    m, t = _step_model(loss=None)
    assert t.engine.overwritten_grads() is None and t.engine.loss == "ce" and t._early_ok
    for V1, d, want in [(1_000_001, 256, (128, 999)), (65_536, 256, (128, 999)), (65_535, 256, None), (27_000, 256, None)]:
        for loss in ("ce", "sampled_ce"):
            stub = types.SimpleNamespace(V1=V1, d=d, loss=loss, head_grad_range=lambda: (128, 999))
            assert BERTEngine.overwritten_grads(stub) == (want if loss == "ce" else None), (V1, loss)


def test_errors():
    from rbm_amd import ops
    from rbm_amd.dataloaders import DeviceBertMasker
    from rbm_amd.train_step import FusedTrainStep
    import rbm_amd.data as synth
    V, T, d, L, h, B = STEP
    with pytest.raises(ValueError, match="bert_shared_negs"):     # a missing K
        _model(V, T, d, L, h, dtype="bf16", bert_loss="sampled_ce")
    with pytest.raises(ValueError, match="candidates"):           # K = 0
        _model(V, T, d, L, h, dtype="bf16", bert_loss="sampled_ce", bert_shared_negs=0)
    with pytest.raises(ValueError, match="candidates"):           # K > max
        _model(V, T, d, L, h, dtype="bf16", bert_loss="sampled_ce", bert_shared_negs=ops.sas_sce_max_k() + 1)
    m = _model(V, T, d, L, h, dtype="bf16", bert_loss="sampled_ce", bert_shared_negs=16)
    assert FusedTrainStep(m).loss == "sampled_ce"
    with pytest.raises(ValueError, match="single device"):
        FusedTrainStep(m, dp=True)
    with pytest.raises(ValueError, match="single device"):
        FusedTrainStep(m, vocab_shard=True)
    b = _step_batches(1)[0]
    t = FusedTrainStep(m, lr=1e-3)
    with pytest.raises(ValueError, match="steps_per_graph"):
        t.capture(*b, warmup=1, steps_per_graph=2)
    with pytest.raises(ValueError, match="steps_per_graph"):
        t.capture_sampled(_masker(V, B, T, 16), warmup=1, steps_per_graph=2)
    hist = synth.user_histories(np.random.default_rng(3), 20, T, V)
    with pytest.raises(ValueError, match="shared_negs"):          # a sampler without candidates
        FusedTrainStep(m, lr=1e-3).capture_sampled(DeviceBertMasker(hist, V, B, T, 0.3, seed=1), warmup=1)
    over = torch.ones(ops.sas_sce_max_k() + 1, dtype=torch.int64)
    with pytest.raises(ValueError, match="candidates"):
        m.sampled_ce_loss(b[0], b[1], over)
    with pytest.raises(ValueError, match="candidates"):
        m.sampled_ce_loss(b[0], b[1], over[:0])


def test_workspace_is_not_shaped_by_the_catalogue():
    """The engine's sce_* buffers at V = 1,000 and V = 50,000, d = 64, the same batch shape and K: the same bytes, and
    no other buffer of the step is shaped by V either."""
    T, d, L, h, B, K = 16, 64, 1, 2, 8, 100
    sizes = {}
    for V in (1000, 50000):
        m = _model(V, T, d, L, h, dtype="bf16")
        rng = np.random.default_rng(0)
        tok = torch.from_numpy(rng.integers(1, 1001, (B, T)))
        lab = torch.from_numpy(np.where(rng.random((B, T)) < 0.3, rng.integers(1, 1001, (B, T)), 0))
        _autograd_step(m, tok, lab, torch.from_numpy(rng.integers(1, 1001, K)))
        bufs = m.engine().ws.bufs
        sizes[V] = {k: (tuple(v.shape), v.numel() * v.element_size()) for k, v in bufs.items() if k.startswith("sce_")}
        assert {"sce_ws", "sce_dh", "sce_src", "sce_bsrc", "sce_keys", "sce_itemidx", "sce_div"} <= set(sizes[V])
        for k, v in bufs.items():
            if k != "tokidx":                                     # the token table's own index (the encoder's, as under CE)
                assert not any(n in tuple(v.shape) for n in (V, V + 1, V + 2, -(-(V + 1) // 64) * 64)), k
    print("sce_* bytes", {V: sum(b for _, b in s.values()) for V, s in sizes.items()})
    assert sizes[1000] == sizes[50000]


# ================================================================ learning
def test_it_learns_a_deterministic_next_item_rule_about_as_well_as_the_full_ce():
    """The rule x' = (7 x + 3) mod V + 1 on V = 200 items, T = 16, d = 64, 300 fused bf16 steps through
    DeviceBertMasker at batch 16: one model trained with the sampled softmax (K = 64 candidates per step) and its twin
    (same weights, data, masker seed and step count) with the full cross-entropy.  Full-rank HR@10 of the item that
    follows a fresh rule chain ([MASK] at the last position).

    Measured on an MI355X: HR@10 1.000 with the sampled softmax (loss 4.78 -> 1.10) and 1.000 with the full
    cross-entropy (loss 5.87 -> 1.70): both twins rank the rule's item first-ten on all 256 chains.  The allowed
    shortfall is 0.05 (13 of the 256 chains): room for a few borderline ranks, far from the 0.95 a model that had
    not learnt the rule would lose."""
    from rbm_amd.dataloaders import DeviceBertMasker
    from rbm_amd.train_step import FusedTrainStep
    V, T, d, L, h, B, K, steps = 200, 16, 64, 1, 2, 16, 64, 300
    rng = np.random.default_rng(0)
    hist = []
    for _ in range(600):
        x = [int(rng.integers(1, V + 1))]
        for _ in range(T - 1):
            x.append((7 * x[-1] + 3) % V + 1)
        hist.append(x)
    ev = np.zeros((256, T + 1), np.int64)
    ev[:, 0] = rng.integers(1, V + 1, 256)
    for t in range(T):
        ev[:, t + 1] = (7 * ev[:, t] + 3) % V + 1
    x_eval = ev[:, 1:].copy()
    target = torch.from_numpy(x_eval[:, -1].copy())
    x_eval[:, -1] = V + 1                                           # [MASK]
    hr = {}
    for loss in ("sampled_ce", "ce"):
        m = _model(V, T, d, L, h, dtype="bf16", seed=0)
        sampler = DeviceBertMasker(hist, V, B, T, 0.3, seed=0, shared_negs=K if loss == "sampled_ce" else None)
        t = FusedTrainStep(m, lr=1e-3, loss="sampled_ce" if loss == "sampled_ce" else None)
        losses = []
        for i in range(steps):
            if i % sampler.num_batch == 0:
                sampler.new_epoch()
            losses.append(t.step(*sampler.sample()).clone())
        losses = [float(x.item()) for x in losses]
        m.eval()
        rank = m.full_rank(torch.from_numpy(x_eval), target, exclude_seen=False)
        hr[loss] = float((rank < 10).float().mean().item())
        print(loss, "first / last loss", losses[0], losses[-1], "HR@10", hr[loss])
        assert losses[-1] < losses[0], (loss, losses[0], losses[-1])
    assert hr["ce"] >= 0.5, hr                                      # 10 x the chance level 10 / V: the task is learnable
    assert hr["sampled_ce"] >= hr["ce"] - SHORTFALL, hr


# HR@10 the sampled-softmax twin may lose against the CE twin (see the test's docstring)
SHORTFALL = 0.05
