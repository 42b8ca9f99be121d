"""The fused GEMM epilogue (include/recsys_hip.h rs_epilogue) per element against the float64 chain and derived bound
of bert_rows_ref.py, with the dropout masks from the HOST hash: every compile-time class of GBF_EC_LIST and the runtime
fallback, on every GEMM body the dispatch can select (LDS-DMA 64- and 128-row tiles, register-staged 64x64 and
128x128), both storage orientations of B (forward X W^T and input gradient dY W), bf16 and fp32 C, accumulate, a device
row count, the fp32 kernel's libm GELU, and rs_gemm_ln staged on the h it stored.  (The bitwise tests of
test_gemm_dma_gpu.py pin the bodies to each other; these pin the shared epilogue source to the header.)
BERT's uses: bert_modules/utils/feed_forward.py:15-16, utils/sublayer.py:16-18, attention/multi_head.py:18-19,40."""
import os

import pytest
import torch

import bert_rows_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
BODIES = {"dma64": {"RS_GEMM_DMA": "1", "RS_GEMM_DMA_BM": "64"}, "dma128": {"RS_GEMM_DMA": "1", "RS_GEMM_DMA_BM": "128"},
          "reg": {"RS_GEMM_DMA": "0"}}


class _env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_cache = {}


def _inputs(M, N, K, dtype=BF):
    """inputs and the float64 products, computed once per shape and left unchanged"""
    key = (M, N, K, dtype)
    if key not in _cache:
        inp = R.epi_inputs(M, N, K, dev=DEV, dtype=dtype)
        inp["Wt"] = inp["W"].t().contiguous()
        inp["acc"], inp["absacc"] = R.products(inp["A"], inp["W"])
        _cache[key] = inp
    return _cache[key]


def run_case(ops, inp, M, N, K, flags, act, *, dgrad=False, out_dtype=BF, alpha=1.0, pad=8, respad=8, auxpad=8,
             bias_off=0, drop_ld=None, rows=None, dtype=BF, tag=""):
    """one GEMM call in guarded buffers + every check of its outputs; returns {output: err/bound}"""
    drop_ld = drop_ld or N
    kw = R.epi_ref_kw(flags, act, inp, M, N, drop_ld, out_dtype, alpha=alpha)
    sb = torch.tensor([R.SEED_BASE], dtype=torch.int64, device=DEV)
    ek = {"alpha": alpha, "act": act}
    if "B" in flags:
        buf = torch.full((N + 8,), float("nan"), device=DEV)
        ek["bias"] = buf[bias_off:bias_off + N]
        ek["bias"].copy_(inp["bias"])
    if act >= 3:
        ek["aux"] = R.guarded_from(inp["aux"], auxpad)[1]
    waux = aux_out = None
    if act in (1, 2):
        waux, aux_out = R.guarded(M, N, auxpad, dtype)
        ek["aux_out"] = aux_out
    if "D" in flags:
        ek.update(drop_p=R.EPI_P, drop_seed=R.SALT1, seed_base=sb, drop_ld=drop_ld)
    if "P" in flags:
        ek.update(post_drop_p=R.EPI_P, post_drop_seed=R.SALT2, seed_base=sb, drop_ld=drop_ld)
    if "R" in flags:
        ek["resid"] = R.guarded_from(inp["resid"], respad)[1]
    if "M" in flags:
        ek["rowmask_ids"] = inp["ids"]
    if "A" in flags:
        ek["accumulate"] = True
    if rows is not None:
        ek["rows_dev"] = torch.tensor([rows], dtype=torch.int32, device=DEV)
    wc, C = R.guarded(M, N, pad, out_dtype)
    if "A" in flags:
        C.copy_(kw["cold"])
    if dgrad:
        ops.linear_dgrad(inp["A"], inp["Wt"], C, **ek)
    else:
        ops.linear_fwd(inp["A"], inp["W"], C, **ek)
    torch.cuda.synchronize()
    assert R.guards_untouched(wc, (M, N)), tag
    if waux is not None:
        assert R.guards_untouched(waux, (M, N)), tag
    n = M if rows is None else rows
    if rows is not None:      # rows at or past the device count: untouched
        assert torch.equal(C[n:], kw["cold"][n:]) if "A" in flags else bool(torch.isnan(C[n:]).all()), tag
        assert aux_out is None or bool(torch.isnan(aux_out[n:]).all()), tag
    cut = {k: (v[:n] if torch.is_tensor(v) and v.dim() == 2 and v.shape[0] == M else v) for k, v in kw.items()}
    # bf16 operands whose leading dimensions are no multiple of 8 (here: dY W with N = 100) go to gemm.hip's kernel
    # and its libm GELU, like the fp32 dtype: rs_gemm's own dispatch rule, and the bound's E term follows it
    B = inp["Wt"] if dgrad else inp["W"]
    fast = dtype == BF and inp["A"].stride(0) % 8 == 0 and B.stride(0) % 8 == 0
    res = R.check_epilogue(inp["acc"][:n], inp["absacc"][:n], K, C[:n], None if aux_out is None else aux_out[:n],
                           fast=fast, **cut)
    # dropped elements: exactly 0, or exactly the residual where one is added behind the dropout
    if "D" in flags and "A" not in flags:
        dropped = cut["m1"] == 0
        if "M" in flags:
            dropped = dropped & (cut["rowkeep"] != 0)
        if "R" not in flags:
            assert not C[:n][dropped].any(), tag
        elif "P" not in flags:
            assert torch.equal(C[:n][dropped], inp["resid"][:n][dropped].to(out_dtype)), tag
    if "P" in flags and "A" not in flags:
        assert not C[:n][cut["m2"] == 0].any(), tag
    if "M" in flags and "A" not in flags:
        assert not C[:n][inp["ids"][:n] == 0].any(), tag
    return res


def _report(results, tag):
    top = max(results.items(), key=lambda kv: kv[1])
    print("err/bound", tag, "worst", top[0], round(top[1], 3))
    bad = {k: v for k, v in results.items() if not v <= 1.0}
    assert not bad, (tag, bad)


@pytest.mark.parametrize("body", list(BODIES))
@pytest.mark.parametrize("M,N,K", R.EPI_SHAPES, ids=[f"{m}x{n}x{k}" for m, n, k in R.EPI_SHAPES])
def test_every_class_on_every_body(M, N, K, body):
    """the 18 classes of GBF_EC_LIST (the four BERT uses among them) in both orientations, the class's own C dtype"""
    import rbm_amd  # noqa: F401
    from rbm_amd import ops
    inp = _inputs(M, N, K)
    results = {}
    with _env(BODIES[body]):
        for name, flags, act in R.EPI_CLASSES:
            for dgrad in (False, True):
                tag = f"{body} {name} {'dgrad' if dgrad else 'fwd'}"
                r = run_case(ops, inp, M, N, K, flags, act, dgrad=dgrad, out_dtype=F32 if "F" in flags else BF, tag=tag)
                results.update({f"{tag} {k}": v for k, v in r.items()})
        # a device row count and an fp32 / accumulating C on BERT's classes
        for name, flags, act, od in (("bias_gelu_drop", "BD", 2, BF), ("bias_drop_resid_post", "BDRP", 0, BF),
                                     ("gelu_bwd_drop", "D", 4, BF), ("bias_drop_resid f32 acc", "BDRAF", 0, F32),
                                     ("bias_resid acc", "BRA", 0, BF)):
            r = run_case(ops, inp, M, N, K, flags, act, out_dtype=od, rows=M - 37, tag=f"{body} {name} rows_dev")
            results.update({f"{body} {name} rows_dev {k}": v for k, v in r.items()})
    _report(results, f"{body} {M}x{N}x{K}")


FALLBACKS = {
    "alpha": dict(alpha=0.5),
    "ldc": dict(pad=4),
    "ldres": dict(respad=4),
    "ldaux": dict(auxpad=4),
    "bias+1": dict(bias_off=1),
    "odd drop_ld": dict(drop_ld_extra=1),      # regression: the typed classes paired the elements of odd rows wrongly
    "even drop_ld": dict(drop_ld_extra=2),
}


@pytest.mark.parametrize("why", list(FALLBACKS))
def test_runtime_fallback(why):
    """calls the typed classes cannot take (epi8, the runtime-flag epilogue) -- and drop_ld != N, which they can"""
    import rbm_amd  # noqa: F401
    from rbm_amd import ops
    M, N, K = 70, 128, 96
    inp = _inputs(M, N, K)
    opt = dict(FALLBACKS[why])
    extra = opt.pop("drop_ld_extra", 0)
    results = {}
    for name, flags, act in (("bias_gelu_drop", "BD", 2), ("bias_drop_resid_post", "BDRP", 0), ("gelu_bwd_drop", "D", 4),
                             ("bias_drop_resid_mask", "BDRM", 0), ("bias_relu_drop", "BD", 1), ("relu_bwd_drop", "D", 3)):
        for dgrad in (False, True):
            tag = f"{why} {name} {'dgrad' if dgrad else 'fwd'}"
            r = run_case(ops, inp, M, N, K, flags, act, dgrad=dgrad, drop_ld=N + extra if extra else None, tag=tag, **opt)
            results.update({f"{tag} {k}": v for k, v in r.items()})
    _report(results, why)


@pytest.mark.parametrize("M,N,K", [(70, 100, 96), (70, 192, 96), (200, 128, 40)], ids=["N100", "N192", "K40"])
def test_register_staged_reached_naturally(M, N, K):
    """N not a multiple of 128 (N = 100: a ragged last 8-column chunk, the fallback inside a typed class) and K not a
    multiple of 32 leave the DMA form by themselves"""
    import rbm_amd  # noqa: F401
    from rbm_amd import ops
    inp = _inputs(M, N, K)
    results = {}
    pad = 4 if N % 8 else 8
    for name, flags, act in R.EPI_CLASSES:
        for dgrad in (False, True):
            tag = f"{name} {'dgrad' if dgrad else 'fwd'}"
            r = run_case(ops, inp, M, N, K, flags, act, dgrad=dgrad, out_dtype=F32 if "F" in flags else BF, pad=pad,
                         respad=pad, auxpad=pad, tag=tag)
            results.update({f"{tag} {k}": v for k, v in r.items()})
    _report(results, f"{M}x{N}x{K}")


def test_register_staged_128x128():
    """512 tiles of 128 x 128 with the DMA form off: plain and bias + residual"""
    import rbm_amd  # noqa: F401
    from rbm_amd import ops
    M, N, K = 8192, 1024, 64
    inp = R.epi_inputs(M, N, K, dev=DEV)
    inp["Wt"] = inp["W"].t().contiguous()
    inp["acc"], inp["absacc"] = R.products(inp["A"], inp["W"])
    results = {}
    with _env(BODIES["reg"]):
        for name, flags in (("plain", ""), ("bias_resid", "BR")):
            for dgrad in (False, True):
                r = run_case(ops, inp, M, N, K, flags, 0, dgrad=dgrad, tag=name)
                results.update({f"{name} {'dgrad' if dgrad else 'fwd'} {k}": v for k, v in r.items()})
    _report(results, "128x128")


@pytest.mark.parametrize("name,flags,act", [("bias_gelu_drop", "BD", 2), ("gelu_bwd_drop", "D", 4),
                                            ("bias_drop_resid_post", "BDRP", 0)])
def test_fp32_kernel(name, flags, act):
    """gemm.hip (the exact f32 MFMA, libm tanhf) at the reference's default width: (70, 100, 50)"""
    import rbm_amd  # noqa: F401
    from rbm_amd import ops
    M, N, K = 70, 100, 50
    inp = _inputs(M, N, K, F32)
    results = {}
    for dgrad in (False, True):
        r = run_case(ops, inp, M, N, K, flags, act, dgrad=dgrad, out_dtype=F32, dtype=F32, pad=3, respad=3, auxpad=3,
                     tag=name)
        results.update({f"{name} {'dgrad' if dgrad else 'fwd'} {k}": v for k, v in r.items()})
    _report(results, "fp32 " + name)


@pytest.mark.parametrize("M", [37, 70, 1000])
@pytest.mark.parametrize("kind,N", [("qkv", 768), ("ffn1", 1024), ("ffn1_eval", 1024)])
def test_gemm_ln_staged(M, kind, N):
    """rs_gemm_ln: h, mean, rinv against the LayerNorm stage (variant 1), C and aux_out against the epilogue stage
    applied to the h the kernel stored"""
    import rbm_amd  # noqa: F401
    from rbm_amd import ops
    d = 256
    i = R.ln_inputs(M, d, BF, dev=DEV)
    e = R.epi_inputs(M, N, d, dev=DEV)
    _, x = R.guarded_from(i["x"], 8)
    wh, h = R.guarded(M, d, 8, BF)
    wm, mean = R.guarded_vec(M)
    wr, rinv = R.guarded_vec(M)
    wc, C = R.guarded(M, N, 8, BF)
    sb = torch.tensor([R.SEED_BASE], dtype=torch.int64, device=DEV)
    kw, ref = {}, {"bias": e["bias"], "act": 0}
    waux = aux = None
    if kind != "qkv":
        waux, aux = R.guarded(M, N, 8, BF)
        p = R.EPI_P if kind == "ffn1" else 0.0
        kw = dict(act=ops.ACT_GELU, aux_out=aux, drop_p=p, drop_seed=R.SALT1, seed_base=sb, drop_ld=N)
        ref["act"] = 2
        if p > 0:
            ref["m1"] = R.drop_mult(p, R.SALT1, R.SEED_BASE, M, N, N, DEV)
    assert ops.linear_fwd_ln(x, i["gamma"], i["beta"], R.EPS1, e["W"], C, h, mean, rinv, bias=e["bias"], **kw)
    torch.cuda.synchronize()
    for w, shape in ((wh, (M, d)), (wm, (M,)), (wr, (M,)), (wc, (M, N))) + (((waux, (M, N)),) if aux is not None else ()):
        assert R.guards_untouched(w, shape)
    res = R.check_ln_fwd(i["x"], i["gamma"], i["beta"], R.EPS1, 1, h, mean, rinv)
    acc, absacc = R.products(h, e["W"])
    res.update(R.check_epilogue(acc, absacc, d, C, aux, **ref))
    if "m1" in ref:
        assert not C[ref["m1"] == 0].any()
    _report(res, f"gemm_ln {kind} M={M}")


def test_gemm_ln_unsupported_leaves_outputs_alone():
    import rbm_amd  # noqa: F401
    from rbm_amd import ops
    M, N, d = 70, 768, 128
    i = R.ln_inputs(M, d, BF, dev=DEV)
    e = R.epi_inputs(M, N, d, dev=DEV)
    outs = [torch.full(s, float("nan"), device=DEV, dtype=t) for s, t in (((M, N), BF), ((M, d), BF), ((M,), F32), ((M,), F32))]
    assert ops.linear_fwd_ln(i["x"], i["gamma"], i["beta"], R.EPS1, e["W"], outs[0], outs[1], outs[2], outs[3],
                             bias=e["bias"]) is False
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs)
