"""float64 reference, error bounds, a float32/bf16 emulation and a host statement of the dropout hash for the BERT
row kernels: rs_layernorm_fwd / _bwd / _bwd_drop (layernorm.hip), rs_dropout_rowmask / rs_dropout2 (misc.hip), the
fused GEMM epilogue rs_epilogue (gemm_bf16_impl.h epi8 / epi8_t / epi_rows, gemm.hip epilogue_store) and rs_gemm_ln.

Reference.  One plain torch float64 function per stage, written from the formulas in include/recsys_hip.h
(LayerNorm variant 0: torch.nn.LayerNorm, BS/models/sas_model/sas.py:39,42,50; variant 1: the BERT LayerNorm,
BS/models/bert_modules/utils/layer_norm.py:14-17; GELU: bert_modules/utils/gelu.py:11-12; the sublayer / feed-forward
chains: utils/sublayer.py:16-18, utils/feed_forward.py:15-16).  The checkers apply them STAGED: the LayerNorm
backward continues from the mean / rinv the kernel stored, the fused dropout sites from the dX it stored, rs_gemm_ln's
product from the h it stored -- as the kernels do -- so errors do not compound and a failure names its stage.

Dropout hash.  drop_site() restates common.h's eff_seed, seed32, seed_mult, pair_hash, drop_thr, drop_mul, drop_mul2
in numpy integers: it, not rs_dropout_rowmask, is the mask source of every check here.

Bound (derived, not fitted), the form of rowchain_ref.py.  For a bf16 output with float64 reference r

    |hip - r| <= 2 * ( 2^-8 |r|  +  2^-8 P  +  K 2^-24 A  +  E )

  2^-8 |r|   the output's own rounding; float32 outputs drop it;
  K 2^-24 A  float32 arithmetic: A is the same map on absolute values (|x - mean| replaced by |x| + |mean| where the
             mean is formed in float32), K the number of float32 operations on the longest path, stated at each use;
  P          absolute-value propagation of an unstored bf16 rounding (none of the stages here has one: every value a
             kernel rounds it also stores, and the next stage starts from the stored value);
  E          the fast GELU of the bf16 epilogues (gelu_sig: __expf and v_rcp_f32), explicit, from the argument size:
             2u = 2k x (1 + 0.044715 x^2) is formed by 5 float32 operations, __expf multiplies it by log2(e) (one more
             rounding) and the exponent's absolute error |2u| * 7 * 2^-24 is a relative error of e^-2u; v_exp_f32
             and v_rcp_f32 are taken at 1 ulp (2^-23) each -- the figure of AMD's public CDNA3/CDNA4 ISA guides, which
             are not among this repository's documents -- and the add at 2^-24:  rel(s) <= 2^-24 (7 |2u| + 5).
             test_bert_rows_ref.py::test_fast_gelu_term_covers_emulation measures the emulation's fast GELU against
             float64 over the tests' input range and prints the fraction of E it uses (a property of reference and
             emulation, not of a kernel).  The fp32 path's libm tanhf is taken at 2 ulp (HIP's device math table).
The leading 2 is the only slack.  A bound of 0 (a dropped element, an untouched guard) demands the exact value.

Where a result is one float32 operation on stored inputs and one rounding (the dropout kernels, out1 / out2 of
rs_layernorm_bwd_drop given the stored dX) the checks are bit equality with the emulation, not a bound.

Partials.  rs_layernorm_bwd leaves ws[nb][2][d]; row r belongs to workgroup (r // RPB) % nb with RPB = 4 * (64 / LPR)
on the vectorised path and (r // 4) % min(512, ceil(M / 4)) on the scalar one (ln_owner).  They are checked summed
and workgroup by workgroup.

Emulation.  The same stages in float32 with bf16 rounding wherever the kernels round: a correct kernel as far as the
bound is concerned, and, through `mut`, a family of wrong ones the bound has to reject (test_bert_rows_ref.py).
"""
import math

import numpy as np
import torch

U8, U24 = 2.0 ** -8, 2.0 ** -24
EPS0, EPS1 = float(np.float32(1e-8)), float(np.float32(1e-6))
GUARD = 3                     # guard rows before and after every output
KG = 0.7978845608028654       # sqrt(2/pi)
GELU_LIP = 1.13               # max |gelu_tanh'| = 1.1289
M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
LN_BWD_BLOCKS = 512


def D(t):
    return t.double()


def rb(t):
    """round to bf16, keep the dtype"""
    return t.bfloat16().to(t.dtype)


def rt(t, dtype):
    """round a float32/64 tensor to the storage dtype and return it as float32"""
    return t.to(dtype).float()


# ------------------------------------------------------------------ the dropout hash on the host (common.h)
def eff_seed(salt, seed_base):
    return (salt ^ ((seed_base * 0xD1B54A32D192ED03) & M64)) & M64


def seed32(seed):
    return ((seed & M32) ^ (((seed >> 32) * 0x27D4EB2F) & M32)) & M32


def seed_mult(s32):
    return ((((s32 * 0x9E3779B9) & M32) ^ 0x7FEB352D) | 1) & M32


def pair_hash(s32, idx):
    """idx: numpy uint64 element indices -> the 32-bit hash of each element's PAIR (idx >> 1)"""
    x = ((idx >> np.uint64(1)) & np.uint64(M32)) ^ np.uint64(s32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(seed_mult(s32))) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x


def drop_thr(p):
    return int(min(np.float32(p) * np.float32(65536.0), np.float32(65535.0)))


def kmul(p):
    """the kernels' multiplier 1/(1-p), formed in float32"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def drop_u16(salt, seed_base, idx):
    """the 16-bit uniform of every element index: low half of the pair's hash for even idx, high half for odd"""
    h = pair_hash(seed32(eff_seed(salt, seed_base)), idx)
    return np.where(idx & np.uint64(1), h >> np.uint64(16), h & np.uint64(0xFFFF)).astype(np.int64)


def drop_site(p, salt, seed_base, M, ld, N, rows=None):
    """(keep mask bool [M, N] numpy, the float32 multiplier 1/(1-p) as a python float) of the dropout site
    (salt, seed_base) over elements m * ld + n; drop_mul = drop_mul2 (common.h).  p <= 0 keeps everything."""
    if p <= 0:
        return np.ones((M, N), bool), 1.0
    r = np.arange(M, dtype=np.uint64) if rows is None else np.asarray(rows, np.uint64)
    idx = r[:, None] * np.uint64(ld) + np.arange(N, dtype=np.uint64)[None, :]
    return drop_u16(salt, seed_base, idx) >= drop_thr(p), kmul(p)


def drop_mult(p, salt, seed_base, M, ld, N, dev="cpu"):
    """the site's multiplier tensor (0 or 1/(1-p)) in float32"""
    keep, k = drop_site(p, salt, seed_base, M, ld, N)
    return torch.from_numpy(keep).to(dev).float() * k


# ------------------------------------------------------------------ bound helpers
def bound(r, A, K, bf16, E=None):
    b = K * U24 * A
    if bf16:
        b = b + U8 * r.abs()
    if E is not None:
        b = b + E
    return 2.0 * b


def ratio(hip, r, b):
    """worst |hip - r| / bound over EVERY element; 0/0 counts as 0, a non-finite hip value or an error over a zero
    bound as inf"""
    err = (D(hip) - r).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / b)
    q = torch.where(torch.isfinite(D(hip)) & ~torch.isnan(q), q, torch.full_like(q, math.inf))
    return float(q.max()) if q.numel() else 0.0


# ------------------------------------------------------------------ LayerNorm, float64 stages
def s_ln_fwd(x, g, b, eps, variant):
    """(y, mean [M], rinv [M]).  variant 0: (x - mean) / sqrt(var_biased + eps) g + b; variant 1: g (x - mean) /
    (std_unbiased + eps) + b"""
    d = x.shape[-1]
    mu = x.mean(-1, keepdim=True)
    q = ((x - mu) ** 2).sum(-1, keepdim=True)
    rinv = 1.0 / torch.sqrt(q / d + eps) if variant == 0 else 1.0 / (torch.sqrt(q / (d - 1)) + eps)
    return (x - mu) * rinv * g + b, mu[:, 0], rinv[:, 0]


def b_ln_fwd(x, g, b, eps, variant, bf16):
    """bounds of (y, mean, rinv).  K = d + 8: the d-term sum behind mean and variance plus the handful of elementwise
    operations (divide, sqrt, add eps, reciprocal; subtract, two multiplies, fused add).  mean: A = mean|x|.
    rinv: the relative error of q = sum u^2 is (d + 1) 2^-24 from the sum and 2 sum|u| dmean / q from the float32
    mean, half of it reaches rinv: A = rinv (1 + mean|x| sum|u| / q) (a constant row, q = 0: A = rinv).
    y: A = |g| ((|x| + mean|x|) rinv + |u| A_rinv) + |b|."""
    d = x.shape[-1]
    y, mu, rinv = s_ln_fwd(x, g, b, eps, variant)
    u = (x - mu[:, None]).abs()
    ax = x.abs().mean(-1)
    q = (u ** 2).sum(-1)
    amp = torch.where(q > 0, ax * u.sum(-1) / q.clamp_min(1e-300), torch.zeros_like(q))
    A_r = rinv * (1 + amp)
    A_y = g.abs() * ((x.abs() + ax[:, None]) * rinv[:, None] + u * A_r[:, None]) + b.abs()
    K = d + 8
    return bound(y, A_y, K, bf16), bound(mu, ax, K, False), bound(rinv, A_r, K, False)


def s_ln_bwd(dy, x, g, mu, rinv, eps, variant):
    """(dx, dgamma terms [M, d], dbeta terms [M, d]) from the STORED statistics.  dx = a (gq - mean gq) - coef u,
    u = x - mean, gq = dy g; variant 0: coef = a^3 mean(gq u); variant 1: coef = a^2 sum(gq u) / ((d - 1) sd),
    sd = 1/a - eps the unbiased std (coef = 0 where sd <= 0 or the row is constant: the kernels' branch; the plain
    formula's autograd is NaN there)."""
    d = x.shape[-1]
    a = rinv[:, None]
    u = x - mu[:, None]
    gq = dy * g
    sgu = (gq * u).sum(-1, keepdim=True)
    if variant == 0:
        coef = a ** 3 * sgu / d
    else:
        sd = 1.0 / a - eps
        const = (u == 0).all(-1, keepdim=True)
        coef = torch.where((sd > 0) & ~const, a * a * sgu / ((d - 1) * sd.clamp_min(1e-300)), torch.zeros_like(a))
    return a * (gq - gq.mean(-1, keepdim=True)) - coef * u, dy * (u * a), dy


def b_ln_bwd_dx(dy, x, g, mu, rinv, eps, variant, old, bf16):
    """(dx reference incl. the accumulated old value, its bound).  K = d + 8: the two d-term sums and the elementwise
    operations; A = a (|gq| + mean|gq|) + |coef|_abs |u| + |old| with |coef|_abs the same formula on sum |gq| |u|."""
    d = x.shape[-1]
    dx, _, _ = s_ln_bwd(dy, x, g, mu, rinv, eps, variant)
    a = rinv[:, None]
    u = (x - mu[:, None]).abs()
    gq = (dy * g).abs()
    sgu = (gq * u).sum(-1, keepdim=True)
    if variant == 0:
        coef = a ** 3 * sgu / d
    else:
        sd = 1.0 / a - eps
        coef = torch.where((sd > 0) & (u.sum(-1, keepdim=True) > 0), a * a * sgu / ((d - 1) * sd.clamp_min(1e-300)),
                           torch.zeros_like(a))
    A = a * (gq + gq.mean(-1, keepdim=True)) + coef * u
    if old is not None:
        dx, A = dx + old, A + old.abs()
    return dx, bound(dx, A, d + 8, bf16)


# ---- ownership of the affine partials
def ln_regime(dtype, d, lds=(), ptrs=()):
    """(vectorised?, LPR, NCH): ln_bwd_t's choice.  lds: the leading dimensions, ptrs: the data pointers"""
    V = 8 if dtype == torch.bfloat16 else 4
    ok = d % V == 0 and all(l % V == 0 for l in lds) and all(p % 16 == 0 for p in ptrs)
    cpr = d // V if d % V == 0 else 0
    if ok and cpr in (4, 8, 16, 32, 64):
        return True, cpr, 1
    if ok and cpr == 128:
        return True, 64, 2
    return False, 0, 0


def ln_owner(M, rpb, nb, dev="cpu"):
    """workgroup of every row: (r // rpb) % nb"""
    return (torch.arange(M, device=dev) // rpb) % nb


def ln_scalar_nb(M):
    return min(LN_BWD_BLOCKS, -(-M // 4))


def wg_sum(terms, owner, nb):
    return torch.zeros(nb, terms.shape[1], dtype=terms.dtype, device=terms.device).index_add_(0, owner, terms)


def b_ln_partials(dy, x, mu, rinv, rpb, nb):
    """(ws reference [nb, 2, d], its bound, K) workgroup by workgroup.  K = rows of the longest per-lane chain (the
    iterations of the grid-stride loop times its unroll of 4; on the scalar path rpb = 4 rows per pass, one per
    wave) + the rpb row groups combined in LDS + 3 for the products dy (u a)."""
    M = x.shape[0]
    own = ln_owner(M, rpb, nb, x.device)
    u = x - mu[:, None]
    tg, tb = dy * (u * rinv[:, None]), dy
    ref = torch.stack([wg_sum(tg, own, nb), wg_sum(tb, own, nb)], 1)
    A = torch.stack([wg_sum(tg.abs(), own, nb), wg_sum(tb.abs(), own, nb)], 1)
    K = 4 * -(-M // (nb * rpb * 4)) + rpb + 3
    return ref, bound(ref, A, K, False), K


def b_ln_affine(dy, x, mu, rinv, rpb, nb, g0, b0):
    """(dgamma, dbeta) references as += into the prefilled g0 / b0 and their bounds; K = the partials' K + the nb
    slabs of the fixed-order reduce + 1."""
    u = x - mu[:, None]
    tg, tb = dy * (u * rinv[:, None]), dy
    K = 4 * -(-x.shape[0] // (nb * rpb * 4)) + rpb + 3 + nb + 1
    rg, rbt = g0 + tg.sum(0), b0 + tb.sum(0)
    return (rg, bound(rg, g0.abs() + tg.abs().sum(0), K, False)), (rbt, bound(rbt, b0.abs() + tb.abs().sum(0), K, False))


# ------------------------------------------------------------------ LayerNorm + dropout, emulation
def emu_ln_fwd(x, g, b, eps, variant, mut=None):
    """float32 forward, outputs rounded to x's dtype -> (y, mean, rinv)"""
    d = x.shape[-1]
    xf = x.float()
    mu = xf.sum(-1, keepdim=True) / d
    u = xf - mu
    q = (u * u).sum(-1, keepdim=True)
    e = torch.tensor(eps, dtype=torch.float32)
    if variant == 0:
        rinv = 1.0 / torch.sqrt(q / d + e)
    elif mut == "biased_v1":
        rinv = 1.0 / (torch.sqrt(q / d) + e)
    elif mut == "eps_in_sqrt_v1":
        rinv = 1.0 / torch.sqrt(q / (d - 1) + e)
    else:
        rinv = 1.0 / (torch.sqrt(q / (d - 1)) + e)
    y = u * rinv * g + b if variant == 0 else g * (u * rinv) + b
    return y.to(x.dtype), mu[:, 0], rinv[:, 0]


def emu_ln_bwd(dy, x, g, mu, rinv, eps, variant, old=None, rpb=4, nb=1, g0=None, b0=None, mut=None):
    """float32 backward from the stored statistics -> dict(dx, ws [nb, 2, d], dgamma, dbeta)"""
    M, d = x.shape
    a = rinv[:, None].float()
    u = x.float() - mu[:, None]
    dyf = dy.float()
    gq = dyf * g
    mg = gq.sum(-1, keepdim=True) / (d - 1 if mut == "mean_dm1" else d)
    sgu = (gq * u).sum(-1, keepdim=True)
    if variant == 0:
        coef = a * a * a * sgu / d
    else:
        sd = 1.0 / a - torch.tensor(eps, dtype=torch.float32)
        coef = torch.where(sd > 0, a * a * sgu / ((d - 1) * sd), torch.zeros_like(a))
    if mut == "no_coef":
        coef = torch.zeros_like(coef)
    t = a * (gq - mg) - coef * u
    if old is not None and mut != "no_acc":
        t = old.float() + t
    own = ln_owner(M, rpb, nb)
    tg, tb = dyf * (u * a), dyf
    if mut == "lost_group":       # row group 1 of workgroup 0 never reaches the LDS combine
        lost = ((own == 0) & (torch.arange(M) % rpb == min(1, rpb - 1)))[:, None]
        tg, tb = torch.where(lost, torch.zeros_like(tg), tg), torch.where(lost, torch.zeros_like(tb), tb)
    ws = torch.stack([wg_sum(tg, own, nb), wg_sum(tb, own, nb)], 1)
    if mut == "clamp_readd":      # invalid rows of the last unrolled iteration add the clamped row M - 1 again
        stride = nb * rpb
        for v in range(M, -(-M // (stride * 4)) * stride * 4):
            if v - ((v // stride) % 4) * stride < M:
                w = (v // rpb) % nb
                ws[w, 0] += tg[M - 1]
                ws[w, 1] += tb[M - 1]
    out = {"dx": t.to(x.dtype), "ws": ws}
    if g0 is not None:
        sg, sb = ws[:, 0].sum(0), ws[:, 1].sum(0)
        out["dgamma"], out["dbeta"] = (sg, sb) if mut == "dgamma_overwrite" else (g0 + sg, b0 + sb)
    return out


def emu_drop2(x, m1, m2=None, mut=None, unrounded=None):
    """out1 = round(x * m1), out2 = round(out1 * m2): float32 products of the STORED x; bit-exact model of
    rs_dropout2, rs_dropout_rowmask and the fused sites of rs_layernorm_bwd_drop"""
    src = unrounded if mut == "drop_unrounded" else x.float()
    o1 = (src * m1).to(x.dtype)
    if m2 is None:
        return o1, None
    return o1, (o1.float() * (m1 if mut == "salt_reuse" else m2)).to(x.dtype)


def emu_rowmask(x, ids, m):
    """rs_dropout_rowmask: v = x (0 on rows with id 0); out_masked = v; out = round(v * m)"""
    v = x.float() if ids is None else x.float() * (ids != 0).float()[:, None]
    return (v * m).to(x.dtype), v.to(x.dtype)


# ------------------------------------------------------------------ GELU (tanh form), float64 and its fast-form error
# 0.5 (1 + tanh u) = sigmoid(2u): the same function, written so that float64 keeps its relative accuracy in the
# negative tail (1 + tanh u cancels there)
def gelu(x):
    return x * torch.sigmoid(2 * KG * (x + 0.044715 * x ** 3))


def gelu_grad(x):
    s = torch.sigmoid(2 * KG * (x + 0.044715 * x ** 3))
    return s + x * s * (1 - s) * 2 * KG * (1 + 3 * 0.044715 * x * x)


def _sig_err(x, fast):
    """(s, absolute error bound of s) for s = 0.5 (1 + tanh u) = 1 / (1 + e^-2u) as the kernels form it"""
    u2 = 2 * KG * x * (1 + 0.044715 * x * x)
    s = torch.sigmoid(u2)
    if fast:    # docstring, term E: rel(s) <= 2^-24 (7 |2u| + 5)
        return s, s * U24 * (7 * u2.abs() + 5)
    t = 2 * s - 1   # libm: u by 5 operations, tanhf at 2 ulp = 4 * 2^-24 relative, then 1 + t and the halving
    return s, 0.5 * U24 * (4 * s * (1 - s) * 5 * (u2 / 2).abs() + 4 * t.abs() + 2 * s)


def gelu_err(x, fast):
    s, ds = _sig_err(x, fast)
    return x.abs() * ds + 2 * U24 * (x * s).abs()


def gelu_grad_err(x, fast):
    """gelu' = s + x s (1 - s) c(x), c = 2k (1 + 0.134145 x^2): ds reaches it times (1 + |x| c) (|1 - 2s| <= 1),
    plus 8 roundings of the second term and one of the sum"""
    s, ds = _sig_err(x, fast)
    c = 2 * KG * (1 + 3 * 0.044715 * x * x)
    return ds * (1 + x.abs() * c) + 8 * U24 * (x * s * (1 - s) * c).abs() + U24 * gelu_grad(x).abs()


def emu_gelu_sig(x):
    u2 = np.float32(1.5957691216057308) * x * (1.0 + np.float32(0.044715) * x * x)
    return 1.0 / (1.0 + torch.exp(-u2))


def emu_gelu_fast(x):
    return x * emu_gelu_sig(x)


def emu_gelu_grad_fast(x, c3=0.134145):
    s = emu_gelu_sig(x)
    return s + x * s * (1.0 - s) * np.float32(1.5957691216057308) * (1.0 + np.float32(c3) * x * x)


# ------------------------------------------------------------------ the epilogue chain
ACT_NONE, ACT_RELU, ACT_GELU, ACT_RELU_BWD, ACT_GELU_BWD = 0, 1, 2, 3, 4


def s_epilogue(acc, absacc, Kred, *, bias=None, alpha=1.0, act=0, aux=None, m1=None, resid=None, rowkeep=None,
               m2=None, cold=None, bf16=True, fast=True, aux_bf16=True):
    """The header's chain on float64 tensors: v = alpha acc + bias; act (1 relu, 2 gelu: pre-activation out; 3 relu',
    4 gelu' of aux); dropout m1; + resid; row mask; post dropout m2; + C.  acc = A B^T, absacc = |A| |B|^T, Kred the
    contraction length.  Returns (C reference, C bound, pre-activation reference, its bound).
    K = Kred + 8: the contraction and the at most 8 elementwise float32 operations behind it.  The error of the
    pre-activation passes relu unchanged, GELU times at most 1.13, GELU' times |gelu'(aux)|; E (module docstring) is
    the activation's own error and is scaled by every later factor."""
    K = Kred + 8
    v = alpha * acc
    A = abs(alpha) * absacc
    if bias is not None:
        v, A = v + bias, A + bias.abs()
    pre, bpre = v, bound(v, A, K, aux_bf16)
    E = torch.zeros_like(v)
    if act == ACT_RELU:
        v = torch.relu(v)
    elif act == ACT_GELU:
        E = gelu_err(v, fast)
        v, A = gelu(v), GELU_LIP * A
    elif act == ACT_RELU_BWD:
        k = (aux > 0).double()
        v, A = v * k, A * k
    elif act == ACT_GELU_BWD:
        gp = gelu_grad(aux)
        E = v.abs() * gelu_grad_err(aux, fast)
        v, A = v * gp, A * gp.abs()
    if m1 is not None:
        v, A, E = v * m1, A * m1, E * m1
    if resid is not None:
        v, A = v + resid, A + resid.abs()
    if rowkeep is not None:
        v, A, E = v * rowkeep, A * rowkeep, E * rowkeep
    if m2 is not None:
        v, A, E = v * m2, A * m2, E * m2
    if cold is not None:
        v, A = v + cold, A + cold.abs()
    return v, bound(v, A, K, bf16, E), pre, bpre


def emu_epilogue(acc, *, bias=None, alpha=1.0, act=0, aux=None, m1=None, resid=None, rowkeep=None, m2=None,
                 cold=None, out_dtype=torch.bfloat16, aux_dtype=torch.bfloat16, fast=True, mut=None, m1_mut=None):
    """float32 chain with the kernels' roundings: the stored C and aux_out, the single-rounding fmaf(x, m1, resid) of
    the drop + resid classes.  Returns (C, aux_out).  mut: one deliberate fault (test_bert_rows_ref.py)."""
    x = acc.float()
    if mut != "alpha_ignored":
        x = x * np.float32(alpha)
    if bias is not None and mut != "bias_after_act":
        x = x + bias
    pre = x
    aux_out = pre.to(aux_dtype)
    if act == ACT_RELU:
        x = torch.relu(x)
    elif act == ACT_GELU:
        x = emu_gelu_fast(x) if fast else 0.5 * x * (1 + torch.tanh(np.float32(KG) * (x + np.float32(0.044715) * x ** 3)))
    elif act == ACT_RELU_BWD:
        x = x * (aux > 0).float()
    elif act == ACT_GELU_BWD:
        a = aux.float()
        if mut == "act4_rounded_out":     # the rounded GELU output taken for the saved pre-activation
            a = emu_gelu_fast(a).to(aux.dtype).float()
        if mut == "gelu_bwd_c3":
            x = x * emu_gelu_grad_fast(a, 0.044715)
        elif fast:
            x = x * emu_gelu_grad_fast(a)
        else:
            x = x * gelu_grad(a.double()).float()
    if bias is not None and mut == "bias_after_act":
        x = x + bias
    if m1_mut is not None:
        m1 = m1_mut
    keep = None if rowkeep is None else rowkeep.float()
    if mut == "post_before_resid" and m2 is not None:
        x = (x if m1 is None else x * m1) * m2
        x = x if resid is None else x + resid.float()
        x = x if keep is None else x * keep
    elif mut == "mask_before_resid" and keep is not None:
        x = (x if m1 is None else x * m1) * keep
        x = x if resid is None else x + resid.float()
        x = x if m2 is None else x * m2
    elif mut == "resid_before_drop" and resid is not None:
        x = x + resid.float()
        x = x if m1 is None else x * m1
        x = x if keep is None else x * keep
        x = x if m2 is None else x * m2
    else:
        if m1 is not None and resid is not None:
            x = (x.double() * m1.double() + resid.double()).float()      # fmaf: one rounding
        elif m1 is not None:
            x = x * m1
        elif resid is not None:
            x = x + resid.float()
        x = x if keep is None else x * keep
        x = x if m2 is None else x * m2
    if cold is not None:
        x = x + cold.float()
    return x.to(out_dtype), aux_out


def products(A, B):
    """(A B^T, |A| |B|^T) in float64 for A [M, K], B [N, K]"""
    return D(A) @ D(B).t(), D(A).abs() @ D(B).abs().t()


# ------------------------------------------------------------------ inputs and shapes shared by the CPU and GPU tests
def ln_inputs(M, d, dtype, seed=0, dev="cpu", const_row=None, zero_beta=False):
    """x with a row offset, dy with a per-feature mean (column sums do not cancel), affine parameters, prefills"""
    g = torch.Generator().manual_seed(1000 * d + M + seed)
    x = (torch.randn(M, d, generator=g) * 1.5 + 0.3 + 0.5 * torch.randn(M, 1, generator=g)).to(dtype)
    if const_row is not None:
        x[const_row] = 0.5
    dy = (torch.randn(M, d, generator=g) * 0.5 + 0.25 * torch.randn(1, d, generator=g).sign()).to(dtype)
    out = {"x": x, "dy": dy, "gamma": 1.0 + 0.2 * torch.randn(d, generator=g),
           "beta": 0.1 * torch.randn(d, generator=g) * (0.0 if zero_beta else 1.0),
           "old": torch.randn(M, d, generator=g).to(dtype), "g0": torch.randn(d, generator=g),
           "b0": torch.randn(d, generator=g)}
    return {k: v.to(dev) for k, v in out.items()}


def ln_rows(rpb, vec=True):
    """row counts of one regime: 1, RPB - 1, one row past full unrolled iterations, a last iteration with 1-3 invalid
    rows per group, and one just past a full first trip of the grid-stride loop, so that a second, ragged one runs:
    512 * 4 * RPB rows vectorised (16,413 at d = 256 bf16, 8,205 at d = 1024), 512 * 4 on the scalar path (2,051)"""
    big = LN_BWD_BLOCKS * 4 * rpb + 3 * rpb + (5 if rpb == 8 else 1) if vec else LN_BWD_BLOCKS * 4 + 3
    return [1, max(2, rpb - 1), 4 * rpb * 3 + 1, 4 * rpb * 2 + 2 * rpb + 3, big]


# (dtype, d, leading-dimension pad) of every LayerNorm regime the GPU tests reach; pad keeps the vector alignment
# except where the case is the scalar path by leading dimension
LN_VEC = [(torch.bfloat16, d, 8) for d in (32, 64, 128, 256, 512, 1024)] + \
         [(torch.float32, d, 4) for d in (16, 64, 256, 512)]
LN_SCALAR = [(torch.bfloat16, 50, 6), (torch.float32, 50, 3), (torch.bfloat16, 96, 8), (torch.float32, 300, 4),
             (torch.bfloat16, 1000, 8), (torch.bfloat16, 256, 4), (torch.float32, 256, 2)]


def ln_rpb(dtype, d, pad):
    vec, lpr, _ = ln_regime(dtype, d, (d + pad,))
    return (4 * (64 // lpr), True) if vec else (4, False)


def epi_inputs(M, N, K, seed=0, dev="cpu", dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(7 * M + 3 * N + K + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    out = {"A": r(M, K).to(dtype), "W": (r(N, K) / math.sqrt(K)).to(dtype), "bias": 0.3 * r(N),
           "aux": (1.5 * r(M, N)).to(dtype), "resid": r(M, N).to(dtype), "cold": r(M, N),
           "ids": (torch.rand(M, generator=g) > 0.3).long()}
    return {k: v.to(dev) for k, v in out.items()}


# ------------------------------------------------------------------ checkers: {output: worst err / bound}
def check_ln_fwd(x, g, b, eps, variant, y, mean, rinv):
    bf = x.dtype == torch.bfloat16
    ry, rm, rr = s_ln_fwd(D(x), D(g), D(b), eps, variant)
    by, bm, br = b_ln_fwd(D(x), D(g), D(b), eps, variant, bf)
    return {"y": ratio(y, ry, by), "mean": ratio(mean, rm, bm), "rinv": ratio(rinv, rr, br)}


def check_ln_bwd(x, dy, g, mean, rinv, eps, variant, rpb, nb, dx, old=None, ws=None, dgamma=None, dbeta=None,
                 g0=None, b0=None):
    """staged on the stored mean / rinv; ws [nb, 2, d] workgroup by workgroup and summed; dgamma / dbeta as += into
    the prefills g0 / b0"""
    bf = x.dtype == torch.bfloat16
    X, DY, MU, RI = D(x), D(dy), D(mean), D(rinv)
    rdx, bdx = b_ln_bwd_dx(DY, X, D(g), MU, RI, eps, variant, None if old is None else D(old), bf)
    res = {"dx": ratio(dx, rdx, bdx)}
    zero = torch.zeros(x.shape[1], dtype=torch.float64, device=x.device)
    if ws is not None:
        rws, bws, _ = b_ln_partials(DY, X, MU, RI, rpb, nb)
        res["ws"] = ratio(ws, rws, bws)
        (rg, bg), (rbt, bb) = b_ln_affine(DY, X, MU, RI, rpb, nb, zero, zero)
        res["ws summed"] = max(ratio(D(ws)[:, 0].sum(0), rg, bg), ratio(D(ws)[:, 1].sum(0), rbt, bb))
    if dgamma is not None:
        (rg, bg), (rbt, bb) = b_ln_affine(DY, X, MU, RI, rpb, nb, D(g0), D(b0))
        res["dgamma"], res["dbeta"] = ratio(dgamma, rg, bg), ratio(dbeta, rbt, bb)
    return res


def check_epilogue(acc, absacc, Kred, C, aux_out=None, fast=True, **kw):
    """kw: s_epilogue's keyword tensors in any float dtype"""
    kw = {k: (D(v) if torch.is_tensor(v) else v) for k, v in kw.items()}
    aux_bf16 = aux_out is None or aux_out.dtype == torch.bfloat16
    r, b, pre, bpre = s_epilogue(acc, absacc, Kred, bf16=C.dtype == torch.bfloat16, fast=fast, aux_bf16=aux_bf16, **kw)
    res = {"C": ratio(C, r, b)}
    if aux_out is not None:
        res["aux_out"] = ratio(aux_out, pre, bpre)
    return res


# ------------------------------------------------------------------ the epilogue classes (GBF_EC_LIST, in its order)
# flags: B bias, D dropout, R residual, M row mask, P post dropout, A accumulate, F fp32 C; then the activation
EPI_CLASSES = [("plain", "", 0), ("bias", "B", 0), ("bias_resid", "BR", 0), ("bias_relu_drop", "BD", 1),
               ("bias_relu", "B", 1), ("bias_drop_resid_mask", "BDRM", 0), ("bias_resid_mask", "BRM", 0),
               ("bias_gelu_drop", "BD", 2),              # BERT FFN1 (with the pre-activation saved)
               ("bias_gelu", "B", 2),
               ("bias_drop_resid", "BDR", 0),            # BERT output projection
               ("bias_drop_resid_post", "BDRP", 0),      # BERT FFN2
               ("f32_bias", "BF", 0), ("resid", "R", 0), ("relu_bwd_drop", "D", 3), ("relu_bwd", "", 3),
               ("gelu_bwd_drop", "D", 4),                # BERT FFN2 input gradient
               ("gelu_bwd", "", 4), ("acc", "A", 0)]
EPI_SHAPES = [(70, 128, 32), (200, 384, 96), (70, 384, 160), (200, 128, 1024)]   # M, N, K
SALT1, SALT2 = 0xC0FFEE0000000007, 0x8000000100000003      # high bits set
SEED_BASE = (3 << 40) + 11
EPI_P = 0.1


def epi_ref_kw(flags, act, inp, M, N, drop_ld, out_dtype, alpha=1.0, p=EPI_P):
    """s_epilogue / emu_epilogue keywords of one class over the inputs of epi_inputs (the masks from the host hash)"""
    dev = inp["A"].device
    kw = {"act": act, "alpha": alpha}
    if "B" in flags:
        kw["bias"] = inp["bias"]
    if act >= 3:
        kw["aux"] = inp["aux"]
    if "D" in flags:
        kw["m1"] = drop_mult(p, SALT1, SEED_BASE, M, drop_ld, N, dev)
    if "R" in flags:
        kw["resid"] = inp["resid"]
    if "M" in flags:
        kw["rowkeep"] = (inp["ids"] != 0).float()[:, None]
    if "P" in flags:
        kw["m2"] = drop_mult(p, SALT2, SEED_BASE, M, drop_ld, N, dev)
    if "A" in flags:
        kw["cold"] = inp["cold"].to(out_dtype)
    return kw


# ------------------------------------------------------------------ guarded buffers of the GPU tests
def guarded(M, N, pad, dtype, fill=float("nan"), dev="cuda"):
    """(whole, view): an [M, N] view at leading dimension N + pad with GUARD rows above and below, all = fill"""
    whole = torch.full((M + 2 * GUARD, N + pad), fill, dtype=dtype, device=dev)
    return whole, whole[GUARD:GUARD + M, :N]


def guarded_from(t, pad, fill=float("nan")):
    """t copied into a guarded buffer (inputs whose padding must not be read as data, += targets with a sentinel)"""
    whole, view = guarded(t.shape[0], t.shape[1], pad, t.dtype, fill, t.device)
    view.copy_(t)
    return whole, view


def guarded_vec(n, fill=float("nan"), dev="cuda", dtype=torch.float32):
    """a length-n vector 16 bytes into a filled buffer, with GUARD + 1 spare elements behind it"""
    whole = torch.full((4 + n + GUARD + 1,), fill, dtype=dtype, device=dev)
    return whole, whole[4:4 + n]


def guards_untouched(whole, view_shape, fill=float("nan"), off=None):
    """every element of `whole` outside the [M, N] (or [n]) view still holds the fill"""
    g = whole.clone()
    if whole.dim() == 2:
        g[GUARD:GUARD + view_shape[0], :view_shape[1]] = fill
    else:
        g[4:4 + view_shape[0]] = fill
    return bool(torch.isnan(g).all()) if math.isnan(fill) else bool((g == fill).all())
