"""rs_attn_fwd / rs_attn_bwd against the float64 reference of tests/attn_ref.py, EVERY element of every output
held to the derived per-element bound (the derivation: attn_ref's docstring), in every regime of the LDS-resident
kernels' launchers (attention_lds.hip) -- each case first proves, through the host-only rs_attn_lds_regime and
rs_attn_bwd_plan, that it runs the code it names.

The kernels are called as the models call them: q its own tensor, k / v the two halves of a [M][2d] tensor, dk / dv
the halves of another.  Every output (o, lse, dq, dk, dv, ws) is prefilled with NaN and has GUARD rows of NaN in
front and behind, which must stay NaN.  Each case runs without dropout, with dropout 0.2 (the kernels' own
multiplier, materialised through rs_dropout_rowmask), and with dropout and RS_ATTN_DELTA_IN (delta from
rs_attn_row_delta, O a tensor of NaN).  RS_ATTN_REF_LOG=<file> appends every case's ratios as JSON lines.

Worst err / bound measured on an MI355X (per regime: DESIGN.md, attention section): LDS kernels lse 0.038, o 0.461,
delta 0.023, dq 0.450, dk 0.470, dv 0.476; generic bf16 o 0.430, dq 0.394, dk 0.458, dv 0.456; fp32 mode <= 0.044.
The fp32-mode all-padding case (3, 2, 64, 37) is the regression test of the generic kernels' dS on filled keys.
"""
import json
import math
import os

import pytest
import torch

import attn_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
G = R.GUARD
SALT = 0x1234567


def guarded(rows, cols, dtype):
    """(whole, view): a NaN tensor with G guard rows (elements when cols is None) around the view the kernels get"""
    shape = (rows + 2 * G,) if cols is None else (rows + 2 * G, cols)
    big = torch.full(shape, math.nan, device=DEV, dtype=dtype)
    return big, big[G:G + rows]


def guards_intact(big, rows):
    return bool(torch.isnan(big[:G]).all() and torch.isnan(big[G + rows:]).all())


def kernel_mult(c, p, sb):
    """the kernels' dropout multiplier [BH][T][T]: rs_dropout_rowmask over (B*H*T, Tp) draws the same mask"""
    from rbm_amd import ops
    if p <= 0:
        return torch.ones(c.BH, c.T, c.T, device=DEV)
    ones = torch.ones(c.BH * c.T, c.Tp, device=DEV)
    mult = torch.empty_like(ones)
    ops.dropout_rowmask(ones, p, SALT, sb, None, mult)
    return mult[:, :c.T].reshape(c.BH, c.T, c.T)


def run(c, inp, p, delta_in, dtype=torch.bfloat16):
    """forward then backward through ops; returns (outputs, the guarded wholes, delta given to the backward)"""
    from rbm_amd import ops
    d, n = c.d, c.BH * c.T
    sb = torch.full((1,), 99, dtype=torch.int64, device=DEV)
    big = {}
    big["o"], o = guarded(c.M, d, dtype)
    big["lse"], lse = guarded(n, None, torch.float32)
    big["dq"], dq = guarded(c.M, d, dtype)
    big["dkv"], dkv = guarded(c.M, 2 * d, dtype)
    big["ws"], ws = guarded(n, None, torch.float32)
    q, kv, do, ids = inp["q"], inp["kv"], inp["do"], inp["ids"]
    ops.attn_fwd(c.B, c.T, c.H, c.Dh, q, kv[:, :d], kv[:, d:], o, lse, c.scale, c.mask_kind, ids, p, SALT, sb)
    given = None
    o_arg = o
    if delta_in:
        ops.attn_row_delta(c.B, c.T, c.H, c.Dh, do, o, ws)
        given = ws.clone()
        o_arg = torch.full_like(o, math.nan)             # O must not be read
    ops.attn_bwd(c.B, c.T, c.H, c.Dh, q, kv[:, :d], kv[:, d:], o_arg, do, lse, dq, dkv[:, :d], dkv[:, d:], c.scale,
                 c.mask_kind, ids, p, SALT, sb, ws, delta_in=delta_in)
    torch.cuda.synchronize()
    return {"o": o, "lse": lse, "dq": dq, "dkv": dkv, "ws": ws}, big, given, kernel_mult(c, p, sb)


def check(c, inp, p, delta_in, kind="lds", dtype=torch.bfloat16):
    """{output: worst err / bound}; asserts the guards, the bound on every element, and ws untouched when given"""
    out, big, given, m = run(c, inp, p, delta_in, dtype)
    rows = {"o": c.M, "dq": c.M, "dkv": c.M, "lse": c.BH * c.T, "ws": c.BH * c.T}
    for name, t in big.items():
        assert guards_intact(t, rows[name]), f"guard rows of {name} written"
    bf = dtype == torch.bfloat16
    res = R.check_fwd(c, inp, m, out, kind, bf)
    if given is not None:
        assert torch.equal(out["ws"], given), "the given delta was overwritten"
    res.update(R.check_bwd(c, inp, m, out["lse"], out["ws"], out, None if delta_in else out["o"], kind, bf))
    tag = f"{(c.B, c.H, c.Dh, c.T)} mask {c.mask_kind} p {p} delta_in {delta_in} {kind} {dtype}"
    print(tag, {k: round(r, 3) for k, (r, _) in res.items()})
    log = os.environ.get("RS_ATTN_REF_LOG")
    if log:
        with open(log, "a") as fh:
            fh.write(json.dumps({"case": tag, "regime": R.regime(c, 1 if bf else 0),
                                 **{k: r for k, (r, _) in res.items()}}) + "\n")
    bad = [f"{r:.3g} x bound at {R.where(c, k, i)}" for k, (r, i) in res.items() if not r <= 1.0]
    assert not bad, tag + ": " + "; ".join(bad)
    return out


VARIANTS = [(0.0, False), (0.2, False), (0.2, True)]
CASES = [(purpose, shape, mk, want, False) for purpose, shape, mks, want in R.SHAPES for mk in mks] + \
        [("all-padding sequence", shape, 1, None, True) for shape in R.ALL_PAD]


@pytest.mark.parametrize("purpose,shape,mask_kind,want,all_pad", CASES,
                         ids=[f"{s[0]}x{s[1]}x{s[2]}x{s[3]}-m{mk}{'-pad' if ap else ''}" for _, s, mk, _, ap in CASES])
def test_lds_attention_every_element(purpose, shape, mask_kind, want, all_pad):
    import rbm_amd  # noqa: F401
    c = R.Case(*shape, mask_kind)
    if want is not None:
        R.assert_regime(c, purpose, want)
    else:
        assert R.regime(c)[0] == 1
    inp = R.make_inputs(c, DEV, all_pad=all_pad)
    for p, delta_in in VARIANTS:
        out = check(c, inp, p, delta_in)
        if all_pad:          # P is uniform from the fill: dS is exactly 0 there, dV is not
            rows = slice(c.T, 2 * c.T)
            assert not out["dq"][rows].any() and not out["dkv"][rows, :c.d].any()
            dv = out["dkv"][rows, c.d:].float()
            assert torch.isfinite(dv).all() and dv.any()


@pytest.mark.parametrize("B,H,Dh,T,mask_kind,all_pad", R.TIER2_F32)
def test_fp32_mode_every_element(B, H, Dh, T, mask_kind, all_pad):
    """float32 storage (the generic kernels): the same reference, the bound without its bf16 terms"""
    import rbm_amd  # noqa: F401
    c = R.Case(B, H, Dh, T, mask_kind)
    assert R.regime(c, 0)[0] == 0
    inp = R.make_inputs(c, DEV, all_pad=all_pad, dtype=torch.float32)
    for p, delta_in in VARIANTS[:2]:
        out = check(c, inp, p, delta_in, "generic", torch.float32)
        if all_pad:
            rows = slice(c.T, 2 * c.T)
            assert not out["dq"][rows].any() and not out["dkv"][rows, :c.d].any()


@pytest.mark.parametrize("B,H,Dh,T,mask_kind,all_pad", R.TIER2_BF16)
def test_generic_bf16_every_element(B, H, Dh, T, mask_kind, all_pad):
    """bf16 shapes the LDS kernels do not take: the generic kernels round the same quantities (the unnormalised P
    instead of the normalised one, dS, P m; the same relative rounding), so the same P term holds"""
    import rbm_amd  # noqa: F401
    c = R.Case(B, H, Dh, T, mask_kind)
    assert R.regime(c)[0] == 0
    inp = R.make_inputs(c, DEV, all_pad=all_pad)
    for p, delta_in in VARIANTS[:2]:
        check(c, inp, p, delta_in, "generic")
