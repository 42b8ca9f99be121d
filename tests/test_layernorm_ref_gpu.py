"""rs_layernorm_fwd / rs_layernorm_bwd / rs_layernorm_bwd_drop (layernorm.hip) per element against the float64
reference and derived bound of bert_rows_ref.py, in every launch regime: the vectorised kernels at every lanes-per-row
count (bf16 d = 32 .. 1024, fp32 d = 16 .. 512), the scalar kernels (d = 50, 96, 300, 1000 and a leading dimension
off the vector width), both variants (torch.nn.LayerNorm, sas.py:39,42,50; the BERT LayerNorm,
bert_modules/utils/layer_norm.py:14-17), accumulate off and on, the affine gradients as += into prefilled vectors
and as the per-workgroup partials (by the ownership model), row counts around every loop edge, one constant row.
Outputs live in NaN-filled buffers with a wider leading dimension and guard rows that must stay untouched."""
import math

import numpy as np
import pytest
import torch

import bert_rows_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
WS_SLABS = R.LN_BWD_BLOCKS            # the ABI's workspace: 2 * d * 512 floats


def _fmt(res):
    return {k: round(v, 3) for k, v in res.items()}


def _assert_inside(res, tag):
    print("err/bound", tag, _fmt(res))
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, (tag, bad)


def _nb(M, rpb, vec):
    return min(R.LN_BWD_BLOCKS, -(-M // (4 * rpb))) if vec else R.ln_scalar_nb(M)


def _forward(ops, i, x, M, d, pad, dtype, variant, eps):
    wy, y = R.guarded(M, d, pad, dtype)
    wm, mean = R.guarded_vec(M)
    wr, rinv = R.guarded_vec(M)
    ops.layernorm_fwd(x, i["gamma"], i["beta"], eps, y, mean, rinv, variant)
    torch.cuda.synchronize()
    assert R.guards_untouched(wy, (M, d)) and R.guards_untouched(wm, (M,)) and R.guards_untouched(wr, (M,))
    return y, mean, rinv


@pytest.mark.parametrize("dtype,d,pad", R.LN_VEC + R.LN_SCALAR,
                         ids=[f"{'bf16' if t == BF else 'fp32'}-d{d}-ld+{p}-{'vec' if R.ln_rpb(t, d, p)[1] else 'scalar'}"
                              for t, d, p in R.LN_VEC + R.LN_SCALAR])
def test_layernorm_every_element(dtype, d, pad):
    import rbm_amd  # noqa: F401
    from rbm_amd import ops
    rpb, vec = R.ln_rpb(dtype, d, pad)
    worst = {}
    for M in R.ln_rows(rpb, vec):
        i = R.ln_inputs(M, d, dtype, dev=DEV, const_row=0 if M > 1 else None)
        _, x = R.guarded_from(i["x"], pad)
        _, dy = R.guarded_from(i["dy"], pad)
        # the regime the case is named for, where the ABI exposes it
        nparts = ops.layernorm_bwd_nparts(x)
        nb = _nb(M, rpb, vec)
        assert (nparts != 0) == vec and (not vec or nparts == nb), (M, nparts, nb)
        for variant, eps in ((0, R.EPS0), (1, R.EPS1)):
            tag = f"M={M} variant {variant}"
            y, mean, rinv = _forward(ops, i, x, M, d, pad, dtype, variant, eps)
            res = R.check_ln_fwd(i["x"], i["gamma"], i["beta"], eps, variant, y, mean, rinv)
            if M > 1 and variant == 1:       # the constant row: std = 0 -> y = beta, rinv = 1 / eps exactly
                assert torch.equal(y[0], i["beta"].to(dtype)), tag
                assert float(rinv[0]) == float(np.float32(1.0) / np.float32(eps)) and float(mean[0]) == 0.5, tag
            for acc in (False, True):
                for given in (True, False):
                    if acc and not given:
                        continue
                    wdx, dx = R.guarded(M, d, pad, dtype)
                    if acc:
                        dx.copy_(i["old"])
                    wg, dg = R.guarded_vec(d, 7.0)
                    wb, db = R.guarded_vec(d, 7.0)
                    dg.copy_(i["g0"])
                    db.copy_(i["b0"])
                    ws = torch.full((WS_SLABS * 2 * d + 64,), float("nan"), device=DEV)
                    ops.layernorm_bwd(x, dy, i["gamma"], mean, rinv, eps, dx, dg if given else None,
                                      db if given else None, ws, variant, accumulate=acc)
                    torch.cuda.synchronize()
                    assert R.guards_untouched(wdx, (M, d)), tag
                    assert bool(torch.isnan(ws[nb * 2 * d:]).all()), tag       # no slab past the nb written
                    r = R.check_ln_bwd(i["x"], dy, i["gamma"], mean, rinv, eps, variant, rpb, nb, dx,
                                       old=i["old"] if acc else None, ws=ws[:nb * 2 * d].view(nb, 2, d),
                                       dgamma=dg if given else None, dbeta=db if given else None, g0=i["g0"],
                                       b0=i["b0"])
                    if given:
                        assert R.guards_untouched(wg, (d,), 7.0) and R.guards_untouched(wb, (d,), 7.0), tag
                    else:
                        assert torch.equal(dg, i["g0"]) and torch.equal(db, i["b0"]), tag
                    if M > 1:
                        assert bool(torch.isfinite(dx[0].float()).all()), tag      # the constant row's coef = 0 branch
                    res.update({f"{k}{' acc' if acc else ''}{'' if given else ' null'}": v for k, v in r.items()})
            _assert_inside(res, f"{dtype} d={d} {tag}")
            for k, v in res.items():
                worst[k.split(" ")[0]] = max(worst.get(k.split(" ")[0], 0.0), v)
    print("WORST err/bound", dtype, d, "vectorised" if vec else "scalar", _fmt(worst))


DROP_CASES = [(BF, 256, 8, True), (BF, 1024, 8, True), (BF, 32, 8, True), (F32, 64, 4, True),
              (BF, 50, 6, False), (F32, 50, 3, False), (BF, 256, 4, False)]


@pytest.mark.parametrize("dtype,d,pad,fused", DROP_CASES,
                         ids=[f"{'bf16' if t == BF else 'fp32'}-d{d}-ld+{p}-{'fused' if f else 'two-launches'}"
                              for t, d, p, f in DROP_CASES])
def test_layernorm_bwd_drop(dtype, d, pad, fused):
    """dX per element by the bound; out1 = round(dX as stored * m1) and out2 = round(out1 * m2) bit for bit from the
    stored dX with the HOST hash (index row * d + column), dense [M][d] -- whichever path ran: the fused kernel, or
    the LayerNorm backward and the dropout sites in two launches (d = 50; a leading dimension off the vector width).
    Regression: the two-launch path used to write out1 / out2 at dX's pitch and to refuse d % 8 != 0 with out2."""
    import rbm_amd  # noqa: F401
    from rbm_amd import ops
    rpb, vec = R.ln_rpb(dtype, d, pad)
    assert vec == fused
    base = (3 << 40) + 11
    sb = torch.tensor([base], dtype=torch.int64, device=DEV)
    for M in (4 * rpb * 2 + 2 * rpb + 3, rpb - 1 if rpb > 4 else 3):
        i = R.ln_inputs(M, d, dtype, dev=DEV)
        _, x = R.guarded_from(i["x"], pad)
        _, dy = R.guarded_from(i["dy"], pad)
        nb = _nb(M, rpb, vec)
        y, mean, rinv = _forward(ops, i, x, M, d, pad, dtype, 1, R.EPS1)
        for p in (0.0, 0.1):
            m1 = R.drop_mult(p, R.SALT1, base, M, d, d, DEV)
            m2 = R.drop_mult(p, R.SALT2, base, M, d, d, DEV)
            for two in (False, True):
                for acc in (False, True):
                    tag = f"M={M} p={p} out2={two} acc={acc}"
                    wdx, dx = R.guarded(M, d, pad, dtype)
                    if acc:
                        dx.copy_(i["old"])
                    w1, o1 = R.guarded(M, d, 0, dtype)
                    w2, o2 = R.guarded(M, d, 0, dtype)
                    dg, db = i["g0"].clone(), i["b0"].clone()
                    ws = torch.full((WS_SLABS * 2 * d + 64,), float("nan"), device=DEV)
                    ops.layernorm_bwd_drop(x, dy, i["gamma"], mean, rinv, R.EPS1, dx, dg, db, ws, 1, p, R.SALT1,
                                           R.SALT2, sb, o1, o2 if two else None, accumulate=acc)
                    torch.cuda.synchronize()
                    assert R.guards_untouched(wdx, (M, d)) and R.guards_untouched(w1, (M, d)), tag
                    assert R.guards_untouched(w2, (M, d)) if two else bool(torch.isnan(w2).all()), tag
                    res = R.check_ln_bwd(i["x"], dy, i["gamma"], mean, rinv, R.EPS1, 1, rpb, nb, dx,
                                         old=i["old"] if acc else None, ws=ws[:nb * 2 * d].view(nb, 2, d), dgamma=dg,
                                         dbeta=db, g0=i["g0"], b0=i["b0"])
                    _assert_inside(res, f"{dtype} d={d} {tag}")
                    e1, e2 = R.emu_drop2(dx.contiguous(), m1, m2 if two else None)
                    assert torch.equal(o1, e1), (tag, int((o1 != e1).sum()))
                    if two:
                        assert torch.equal(o2, e2), (tag, int((o2 != e2).sum()))
                    if p > 0:       # dropped elements are exactly 0
                        assert not o1[m1 == 0].any()
