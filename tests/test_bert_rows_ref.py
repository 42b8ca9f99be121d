"""The float64 reference of the BERT row kernels and its bound, checked without a GPU (bert_rows_ref.py): every stage
against torch autograd of the plain formula, the host dropout hash against its known properties, the bound against a
float32/bf16 emulation of the kernels at every shape of the GPU tests (a correct kernel passes) and against mutations
of that emulation (a wrong kernel does not)."""
import math

import numpy as np
import pytest
import torch

import bert_rows_ref as R

BF, F32 = torch.bfloat16, torch.float32


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------ the reference is right
@pytest.mark.parametrize("variant,eps", [(0, R.EPS0), (1, R.EPS1)])
def test_layernorm_stages_match_autograd(variant, eps):
    """s_ln_fwd / s_ln_bwd against autograd of the plain formula, dropout sites with injected masks behind the
    backward (out1 = dX m1, out2 = out1 m2).  Reached: <= 1e-13 (asserted 1e-12)."""
    M, d = 37, 50
    i = R.ln_inputs(M, d, F32, seed=3)
    x, g, b = (R.D(i[n]).clone().requires_grad_() for n in ("x", "gamma", "beta"))
    mu = x.mean(-1, keepdim=True)
    if variant == 0:
        y = (x - mu) / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + eps) * g + b
        rinv = 1 / torch.sqrt(x.var(-1, unbiased=False) + eps)
    else:
        y = g * (x - mu) / (x.std(-1, unbiased=True, keepdim=True) + eps) + b
        rinv = 1 / (x.std(-1, unbiased=True) + eps)
    dy = R.D(i["dy"])
    (y * dy).sum().backward()
    ry, rm, rr = R.s_ln_fwd(x.detach(), g.detach(), b.detach(), eps, variant)
    dx, tg, tb = R.s_ln_bwd(dy, x.detach(), g.detach(), rm, rr, eps, variant)
    m1 = R.D(R.drop_mult(0.1, 5, 7, M, d, d))
    m2 = R.D(R.drop_mult(0.1, 6, 7, M, d, d))
    xa = x.detach().clone().requires_grad_()      # the sites' forward: z = (xa m1) m2 -> their backward in turn
    (xa * m1 * m2 * dy).sum().backward()
    worst = {"y": _rel(ry, y.detach()), "mean": _rel(rm, mu.detach()[:, 0]), "rinv": _rel(rr, rinv.detach()),
             "dx": _rel(dx, x.grad), "dgamma": _rel(tg.sum(0), g.grad), "dbeta": _rel(tb.sum(0), b.grad),
             "drop2": _rel(dy * m2 * m1, xa.grad)}
    print("LayerNorm reference vs autograd, variant", variant, max(worst.items(), key=lambda kv: kv[1]))
    assert max(worst.values()) <= 1e-12, worst


def test_epilogue_stage_matches_autograd():
    """GELU (tanh form) and its derivative against autograd, and the whole chain against the plain expression.
    Reached: <= 1e-14 (asserted 1e-12)."""
    x = torch.linspace(-6, 6, 4001, dtype=torch.float64).requires_grad_()
    y = torch.nn.functional.gelu(x, approximate="tanh")
    y.sum().backward()
    worst = {"gelu": _rel(R.gelu(x.detach()), y.detach()), "gelu'": _rel(R.gelu_grad(x.detach()), x.grad)}
    M, N, K = 9, 16, 8
    inp = R.epi_inputs(M, N, K, seed=1)
    acc, absacc = R.products(inp["A"], inp["W"])
    kw = R.epi_ref_kw("BDRMPA", 2, inp, M, N, N + 2, F32, alpha=0.5)
    kw = {k: (R.D(v) if torch.is_tensor(v) else v) for k, v in kw.items()}
    r, _, pre, _ = R.s_epilogue(acc, absacc, K, bf16=False, **kw)
    plain = ((torch.nn.functional.gelu(0.5 * acc + kw["bias"], approximate="tanh") * kw["m1"] + kw["resid"])
             * kw["rowkeep"]) * kw["m2"] + kw["cold"]
    worst["chain"], worst["pre"] = _rel(r, plain), _rel(pre, 0.5 * acc + kw["bias"])
    kw4 = R.epi_ref_kw("D", 4, inp, M, N, N, F32)
    kw4 = {k: (R.D(v) if torch.is_tensor(v) else v) for k, v in kw4.items()}
    a = kw4["aux"].clone().requires_grad_()
    (torch.nn.functional.gelu(a, approximate="tanh") * kw4["m1"] * acc).sum().backward()   # d/da of the FFN1 output
    worst["gelu' chain"] = _rel(R.s_epilogue(acc, absacc, K, bf16=False, **kw4)[0], a.grad)
    print("epilogue reference vs autograd", worst)
    assert max(worst.values()) <= 1e-12, worst


# ------------------------------------------------------------------ the host hash
@pytest.mark.parametrize("p", [0.1, 0.2, 0.5])
def test_host_hash_properties(p):
    M, N = 512, 1024
    n = M * N
    keep, k = R.drop_site(p, R.SALT1, 7, M, N, N)
    q = 1 - math.floor(p * 65536) / 65536
    sig = math.sqrt(n * q * (1 - q))
    print(f"keep rate p = {p}: {keep.mean():.6f} expected {q:.6f}, {abs(keep.sum() - n * q) / sig:.2f} sigma")
    assert abs(keep.sum() - n * q) <= 5 * sig
    assert k == float(np.float32(1) / (np.float32(1) - np.float32(p)))
    # elements 2j, 2j + 1: the low / high half of ONE hash
    idx = np.arange(0, 4096, dtype=np.uint64)
    u = R.drop_u16(R.SALT1, 7, idx)
    h = R.pair_hash(R.seed32(R.eff_seed(R.SALT1, 7)), idx[::2]).astype(np.int64)
    assert np.array_equal(u[::2], h & 0xFFFF) and np.array_equal(u[1::2], h >> 16)
    # only seed_base changes -> another mask; only the salt changes -> another mask
    other, _ = R.drop_site(p, R.SALT1, 8, M, N, N)
    salt, _ = R.drop_site(p, R.SALT1 ^ 1, 7, M, N, N)
    for o in (other, salt):
        agree = (o == keep).mean()
        assert abs(agree - (q * q + (1 - q) ** 2)) < 0.01, agree       # independent draws agree at q^2 + (1-q)^2
    # a leading dimension that differs from N indexes m * ld + n
    wide, _ = R.drop_site(p, R.SALT1, 7, 4, N + 6, N)
    flat, _ = R.drop_site(p, R.SALT1, 7, 1, 4 * (N + 6), 4 * (N + 6))
    assert np.array_equal(wide, flat.reshape(4, N + 6)[:, :N])


def test_fast_gelu_term_covers_emulation():
    """E of the bound against the emulation's fast GELU / GELU' in float32 over the tests' input range (|x| <= 8:
    pre-activations are ~N(0, 1.1), aux ~N(0, 1.5)).  Measured: the emulation uses 0.43 of E for GELU and 0.40 for
    GELU' (printed)."""
    x = torch.linspace(-8, 8, 200001, dtype=torch.float32)
    xd = x.double()
    rg = ((R.emu_gelu_fast(x).double() - R.gelu(xd)).abs() / R.gelu_err(xd, True)).max()
    rd = ((R.emu_gelu_grad_fast(x).double() - R.gelu_grad(xd)).abs() / R.gelu_grad_err(xd, True)).max()
    print(f"fast GELU uses {float(rg):.3f} of E, fast GELU' {float(rd):.3f}")
    assert rg <= 1 and rd <= 1


# ------------------------------------------------------------------ the bound admits a correct kernel
def _ln_case(dtype, d, M, variant, old=True, mut=None, const_row=None, zero_beta=False):
    eps = R.EPS0 if variant == 0 else R.EPS1
    pad = 8 if dtype == BF else 4
    rpb, vec = R.ln_rpb(dtype, d, pad)
    nb = min(R.LN_BWD_BLOCKS, -(-M // (4 * rpb))) if vec else R.ln_scalar_nb(M)
    i = R.ln_inputs(M, d, dtype, const_row=const_row, zero_beta=zero_beta)
    y, mu, ri = R.emu_ln_fwd(i["x"], i["gamma"], i["beta"], eps, variant, mut=mut)
    res = R.check_ln_fwd(i["x"], i["gamma"], i["beta"], eps, variant, y, mu, ri)
    if mut in ("biased_v1", "eps_in_sqrt_v1"):
        return res
    o = R.emu_ln_bwd(i["dy"], i["x"], i["gamma"], mu, ri, eps, variant, old=i["old"] if old else None, rpb=rpb,
                     nb=nb, g0=i["g0"], b0=i["b0"], mut=mut)
    res.update(R.check_ln_bwd(i["x"], i["dy"], i["gamma"], mu, ri, eps, variant, rpb, nb, o["dx"],
                              old=i["old"] if old else None, ws=o["ws"], dgamma=o["dgamma"], dbeta=o["dbeta"],
                              g0=i["g0"], b0=i["b0"]))
    return res


@pytest.mark.parametrize("dtype,d,pad", R.LN_VEC + R.LN_SCALAR, ids=lambda v: str(v).replace("torch.", ""))
def test_layernorm_emulation_inside_bound(dtype, d, pad):
    rpb, vec = R.ln_rpb(dtype, d, pad)
    worst = {}
    rows = R.ln_rows(rpb, vec)
    for M in rows:
        big = M == rows[-1]
        for variant in ((1,) if big else (0, 1)):       # the large count once: the arithmetic per row is the same
            for k, v in _ln_case(dtype, d, M, variant, old=not big, const_row=0 if M > 1 else None).items():
                worst[k] = max(worst.get(k, 0.0), v)
    print("LayerNorm emulation err/bound", dtype, d, "vectorised" if vec else "scalar", rows,
          {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


def _epi_case(name, flags, act, M, N, K, out_dtype=BF, alpha=1.0, mut=None, drop_ld=None, dtype=BF, rows=None):
    inp = R.epi_inputs(M, N, K, dtype=dtype)
    acc, absacc = R.products(inp["A"], inp["W"])
    drop_ld = drop_ld or N
    kw = R.epi_ref_kw(flags, act, inp, M, N, drop_ld, out_dtype, alpha=alpha)
    ekw = dict(kw)
    if mut == "drop_ld_is_N" and "m1" in kw:
        ekw["m1_mut"] = R.drop_mult(R.EPI_P, R.SALT1, R.SEED_BASE, M, N, N)
    fast = dtype == BF
    C, aux_out = R.emu_epilogue(acc.float(), out_dtype=out_dtype, aux_dtype=dtype, fast=fast, mut=mut, **ekw)
    if rows is not None:        # rows_dev: the kernel leaves rows >= rows alone; the mutation writes them
        keepold = torch.full_like(C, 3.0)
        if mut != "rows_past_count":
            C = torch.where(torch.arange(M)[:, None] < rows, C, keepold)
        res = R.check_epilogue(acc[:rows], absacc[:rows], K, C[:rows], aux_out[:rows] if act in (1, 2) else None,
                               fast=fast, **{k: (v[:rows] if torch.is_tensor(v) and v.dim() == 2 and v.shape[0] == M
                                                 else v) for k, v in kw.items()})
        res["rows past count"] = 0.0 if bool((C[rows:] == 3.0).all()) else math.inf
        return res
    return R.check_epilogue(acc, absacc, K, C, aux_out if act in (1, 2) else None, fast=fast, **kw)


@pytest.mark.parametrize("M,N,K", R.EPI_SHAPES)
def test_epilogue_emulation_inside_bound(M, N, K):
    worst = {}
    for name, flags, act in R.EPI_CLASSES:
        for k, v in _epi_case(name, flags, act, M, N, K, F32 if "F" in flags else BF).items():
            worst[name + " " + k] = v
    worst["alpha bias_gelu_drop C"] = _epi_case("a", "BD", 2, M, N, K, alpha=0.5)["C"]
    worst["rows_dev C"] = max(_epi_case("r", "BR", 0, M, N, K, rows=M - 37).values())
    worst["fp32 bias_gelu_drop"] = max(_epi_case("f", "BD", 2, 70, 100, 50, F32, dtype=F32).values())
    worst["fp32 gelu_bwd_drop"] = max(_epi_case("f", "D", 4, 70, 100, 50, F32, dtype=F32).values())
    worst["fp32 bias_drop_resid_post"] = max(_epi_case("f", "BDRP", 0, 70, 100, 50, F32, dtype=F32).values())
    top = max(worst.items(), key=lambda kv: kv[1])
    print("epilogue emulation err/bound", (M, N, K), "worst", top[0], round(top[1], 3))
    assert top[1] <= 1.0, {k: v for k, v in worst.items() if v > 1}


# ------------------------------------------------------------------ and rejects wrong ones
def _drop_sites(mut):
    """bit equality of out1 / out2 with the emulation: a mutation is rejected when any bit differs (factor = the
    number of differing elements, the bound being 0)"""
    M, d = 43, 256
    i = R.ln_inputs(M, d, BF)
    y, mu, ri = R.emu_ln_fwd(i["x"], i["gamma"], i["beta"], R.EPS1, 1)
    o = R.emu_ln_bwd(i["dy"], i["x"], i["gamma"], mu, ri, R.EPS1, 1)
    a, u = R.D(ri)[:, None], R.D(i["x"]) - R.D(mu)[:, None]
    unr = R.s_ln_bwd(R.D(i["dy"]), R.D(i["x"]), R.D(i["gamma"]), R.D(mu), R.D(ri), R.EPS1, 1)[0].float()
    m1 = R.drop_mult(0.1, R.SALT1, 7, M, d, d)
    m2 = R.drop_mult(0.1, R.SALT2, 7, M, d, d)
    good = R.emu_drop2(o["dx"], m1, m2)
    bad = R.emu_drop2(o["dx"], m1, m2, mut=mut, unrounded=unr)
    n = sum(int((g != b).sum()) for g, b in zip(good, bad))
    return {"out1/out2 differing elements": float(n) if n else 0.0}


MUTATIONS = {
    # name: (callable -> {output: err/bound}, the outputs that must reject it)
    "biased variance in variant 1": (lambda: _ln_case(BF, 256, 43, 1, mut="biased_v1"), ("rinv",)),
    "eps inside the sqrt in variant 1": (lambda: _ln_case(F32, 16, 43, 1, mut="eps_in_sqrt_v1", const_row=0), ("rinv",)),
    "mean(g) divided by d - 1": (lambda: _ln_case(F32, 256, 43, 1, mut="mean_dm1"), ("dx",)),
    "coef term dropped": (lambda: _ln_case(BF, 256, 43, 1, mut="no_coef"), ("dx",)),
    "accumulate ignored": (lambda: _ln_case(BF, 256, 43, 0, mut="no_acc"), ("dx",)),
    "one row group missing from a partial": (lambda: _ln_case(BF, 256, 16 * 4 * 3 + 1, 1, mut="lost_group"), ("ws",)),
    "clamped row M - 1 added again": (lambda: _ln_case(BF, 256, 16 * 4 * 2 + 2 * 16 + 3, 1, mut="clamp_readd"), ("ws",)),
    "dgamma overwritten": (lambda: _ln_case(BF, 256, 43, 1, mut="dgamma_overwrite"), ("dgamma", "dbeta")),
    "site 2 drawn with site 1's salt": (lambda: _drop_sites("salt_reuse"), ("out1/out2 differing elements",)),
    "dropout applied to the unrounded dX": (lambda: _drop_sites("drop_unrounded"), ("out1/out2 differing elements",)),
    "post-dropout before the residual": (lambda: _epi_case("m", "BDRP", 0, 70, 128, 32, mut="post_before_resid"), ("C",)),
    "row mask before the residual": (lambda: _epi_case("m", "BDRM", 0, 70, 128, 32, mut="mask_before_resid"), ("C",)),
    "residual added before dropout": (lambda: _epi_case("m", "BDR", 0, 70, 128, 32, mut="resid_before_drop"), ("C",)),
    "alpha ignored": (lambda: _epi_case("m", "BD", 2, 70, 128, 32, alpha=0.5, mut="alpha_ignored"), ("C", "aux_out")),
    "bias added after the activation": (lambda: _epi_case("m", "BD", 2, 70, 128, 32, mut="bias_after_act"), ("C", "aux_out")),
    "act 4 given the rounded output for aux": (lambda: _epi_case("m", "D", 4, 70, 128, 32, mut="act4_rounded_out"), ("C",)),
    "GELU' with 0.044715 for 0.134145": (lambda: _epi_case("m", "D", 4, 70, 128, 32, mut="gelu_bwd_c3"), ("C",)),
    "dropout index using N for drop_ld": (lambda: _epi_case("m", "BD", 2, 70, 128, 32, drop_ld=130, mut="drop_ld_is_N"), ("C",)),
    "rows at or past rows_dev written": (lambda: _epi_case("m", "BR", 0, 70, 128, 32, rows=33, mut="rows_past_count"),
                                         ("rows past count",)),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_mutation_rejected(name):
    """Each wrong kernel exceeds the bound on at least one of the outputs named for it (the factor is printed).
    Biased variance in variant 1 is a 0.2 % relative error of the normalised term at d = 256: with beta = 0 the bf16
    y bound (2 * 2^-8 = 0.8 %) cannot see it -- asserted below; with a beta that cancels part of an element it can, but
    a test must not lean on that -- and the float32 rinv rejects it outright.  eps inside the sqrt moves rinv by 4e-7
    on a row of unit spread, under the bound (asserted); the constant row (rinv 1e3 for 1e6) rejects it."""
    fn, outs = MUTATIONS[name]
    res = fn()
    factors = {o: res[o] for o in outs}
    print(f"mutation '{name}': err/bound", {k: (round(v, 2) if math.isfinite(v) else v) for k, v in res.items()})
    assert max(factors.values()) > 1.0, (name, res)
    if name == "biased variance in variant 1":     # not visible in the bf16 output: why rinv is its own output
        assert _ln_case(BF, 256, 43, 1, mut="biased_v1", zero_beta=True)["y"] <= 1.0
    if name == "eps inside the sqrt in variant 1":
        assert _ln_case(F32, 16, 43, 1, mut="eps_in_sqrt_v1")["rinv"] <= 1.0
