"""float64 reference, error bounds and a float32/bf16 emulation of the vocabulary-sharded head (vocab_head.hip:
rs_vocab_shard_lse, rs_vocab_shard_label_logits, rs_vocab_shard_combine, rs_vocab_head_bwd with voff) and of the
gradient glue behind it (rs_linear_wgrad into a slice of the full gradient, split-K rs_gemm + rs_reduce_slabs).

N shards of one vocabulary are the slices rbm_amd.vocab_parallel.shard_range gives; the reference is plain torch
float64 on the whole vocabulary (losshead_ref.vce_logits, logsumexp, F.cross_entropy), restricted to a shard's
columns where a kernel sees only those.  Every check is STAGED as in losshead_ref: the combine is fed the shard lse
the kernels stored and so is its reference, the backward the stored global lse, the glue the stored bf16 dlogits.
The combine is held end to end as well, against the float64 lse of the whole vocabulary.

Bounds: losshead_ref's (bound_f32 / bound_bf16 with K stated at every use, FAST_ULPS for the fast intrinsics); no
new constant.
  shard lse       vce_lse_bound on the shard's columns; label-0 rows exactly 0
  label logits    bound_f32(|h|.|E[label]| + |b|, d + 1); rows of label 0 or of another shard's label exactly 0
  combine         the kernel takes the max of the N partials, sums N fast exps of N differences and adds a fast log:
                  N + 2 float32 operations on values of magnitude max(|lse|, 1), bound_f32(max(|lse|, 1), N + 2), and
                  one more fold of the fast intrinsics, FAST_ULPS 2^-24 max(|lse|, 1).  End to end: a shard's error
                  moves the whole lse by its softmax weight exp(lse_q - lse), so the weighted mean of the shard bounds
                  is added
  out             as check_vce_fwd: per live row the lse's and the label logit's bound, then the sum: the row term (1),
                  ceil(R / 256) strided adds per thread, 6 shuffles, 4 waves.  The count is exact.  No live row: exactly
                  (0, 0, 0)
  dlogits         vce_grad_bound's formula on the shard's columns from the stored global lse, the one-hot only in the
                  shard that owns the label (grad_bound below; at N = 1 it is vce_grad_bound, which the CPU test holds
                  to equality)
  dW, db          bound_f32(|prefill| + |dlogits|^T |h|, R + splits): R products per element, over `splits` slabs
  dH              per shard ceil(V1s / splits) products and `splits` slabs; the shards are summed in float64

Emulation: the chain in float32 with bf16 dlogits, each `mut` planting one mistake (MUTATIONS).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import losshead_ref as L
from losshead_ref import BF, F32, FAST_ULPS, TINY, Guarded, Worst  # noqa: F401  (re-exported to the tests)
from rowchain_ref import D, U24, bound_bf16, bound_f32, ratio

# ------------------------------------------------------------------ the shape lists of the GPU tests
CHAIN_D, CHAIN_R = (64, 128, 256), (37, 130)
CHAIN_NV = ((1, 5001), (2, 200), (3, 257), (3, 5001))   # (3, 257): the last shard has one row
CHAIN_LONG = (2, 140001, 256, 37)                       # shards past 65,536 classes: persistent over vocabulary tiles
CHAIN_CASES = [(N, V1, d, R) for N, V1 in CHAIN_NV for d in CHAIN_D for R in CHAIN_R] + [CHAIN_LONG]
PATTERNS = ("boundary", "free", "dead", "big")
PATTERN_SHAPE = (2, 5001, 130)                          # (N, V1, R)
PATTERN_D = (64, 256)
MUTATIONS = {   # mut -> (pattern, N, V1, d, R): the smallest listed shape that exercises it
    "onehot_all": (None, 2, 200, 64, 37), "no_v0": (None, 2, 200, 64, 37), "drop_shard": (None, 2, 200, 64, 37),
    "local_max": (None, 2, 200, 64, 37), "dead_mul": ("big", 2, 5001, 64, 130)}
PP_FIXED = {64: 63488, 128: 88064, 256: 137216}        # pp::C<d, true>::FIXED of vocab_head.hip, restated below
LDS_MAX = 163840


def ranges(V1, N):
    from rbm_amd.vocab_parallel import shard_range
    return [shard_range(V1, N, q) for q in range(N)]


def pp_fixed_bytes(d, bwd):
    """pp::C<d, bwd>::FIXED restated: six 32-row h tiles, 8 waves' bias quarters, the forward's reduction slots or
    the backward's per-wave dlogits stage"""
    h_bytes = 6 * 32 * d * 2
    return h_bytes + 8 * 64 * 4 + (8 * 32 * (64 + 8) * 2 if bwd else 2 * 2 * 4 * 4 * 32 * 8)


def expected_form(bwd, R, V1, d, cus, pp=True):
    """(form, gridDim.x, gridDim.y, row tiles per y-group, LDS bytes): the launch rule restated from the file's
    constants (ping-pong: 256-class tiles, 32-row tiles, 8 bytes of metadata per row of the backward's range;
    lock-step: 128-row tiles, 256- (fwd) / 128-class (bwd) tiles, a fixed LDS image)"""
    cd = lambda a, b: -(-a // b)
    nvt, nmt = cd(V1, 256), cd(R, 32)
    gy = max(1, min(nmt, cus // nvt))
    lds = pp_fixed_bytes(d, bwd) + (8 * 32 * cd(nmt, gy) if bwd else 0)
    if pp and lds <= LDS_MAX:
        return 1, min(nvt, cus), gy, cd(nmt, gy), lds
    bv, bk = (128, 64) if bwd else (256, 32)
    nvt, nmt = cd(V1, bv), cd(R, 128)
    gy = max(1, min(nmt, cus // nvt))
    lds = (bv * d + 2 * 128 * bk + (128 * (bv + 8) if bwd else 0)) * 2 + 128 * 12 + 4 * 128 * 2 * 4
    return 0, min(nvt, cus), gy, cd(nmt, gy), lds


def pp_tile_limit(d):
    """most 32-row tiles per y-group the ping-pong backward holds metadata for"""
    return (LDS_MAX - pp_fixed_bytes(d, True)) // (8 * 32)


# ------------------------------------------------------------------ inputs
def shard_inputs(d, R, V1, N, dev, bias=True, pattern=None):
    """vce_inputs, then the label / scale pattern:
    boundary  for each shard boundary b rows labelled b - 1, b, b + 1, plus V1 - 1 and 1
    free      no label in the last shard
    dead      every label 0
    big       E scaled so that a live row and a label-0 row each have a logit above 89 (asserted by big_ok)"""
    inp = L.vce_inputs(d, R, V1, dev, bias=bias)
    lab = inp["labels"]
    rng = ranges(V1, N)
    if pattern == "boundary":
        vals = [v for v0, _ in rng[1:] for v in (v0 - 1, v0, v0 + 1) if v < V1] + [V1 - 1, 1]
        rows = [r for r in range(R) if r % 7][:len(vals)]
        lab[rows] = torch.tensor(vals, device=dev)
    elif pattern == "free":
        lab[lab != 0] = 1 + (lab[lab != 0] - 1) % (rng[-1][0] - 1)
    elif pattern == "dead":
        lab.zero_()
    elif pattern == "big":
        mx = (D(inp["h"]) @ D(inp["E"]).t()).max(1).values     # the bias is not scaled: left out here
        s = 95.0 / float(torch.minimum(mx[lab != 0].max(), mx[lab == 0].max()))
        inp["E"] = (inp["E"].float() * s).to(BF)
    else:
        assert pattern is None
    inp["N"], inp["ranges"] = N, rng
    return inp


def big_ok(inp, logits):
    x, lab = logits[0], inp["labels"]
    mx = x.max(1).values
    return float(mx[lab != 0].max()) > 89 and float(mx[lab == 0].max()) > 89 and float(x.abs().max()) > 88


# ------------------------------------------------------------------ reference and checks
def owned(lab, v0, v1):
    return (lab != 0) & (lab >= v0) & (lab < v1)


def check_shard_lse(inp, logits, q, lse_q):
    x, Ax = (t[:, slice(*inp["ranges"][q])] for t in logits)
    live = (inp["labels"] != 0).double()
    r = torch.logsumexp(x, 1)
    b = L.vce_lse_bound(x, Ax, r, inp["d"])
    return {"lse_q": ratio(lse_q, r * live, b * live)}


def check_label_logits(inp, logits, q, tgt_q):
    x, Ax = logits
    lab = inp["labels"]
    own = owned(lab, *inp["ranges"][q]).double()
    r, A = x.gather(1, lab[:, None])[:, 0] * own, Ax.gather(1, lab[:, None])[:, 0] * own
    return {"tgt_q": ratio(tgt_q, r, bound_f32(A, inp["d"] + 1))}


def fold_bound(r, N):
    m = r.abs().clamp(min=1.0)
    return bound_f32(m, N + 2) + FAST_ULPS * U24 * m


def lse_bound_from(pAx, lse, d):
    """losshead_ref.vce_lse_bound from the softmax-weighted sum pAx = sum_v p_v Ax_v (which may be formed in chunks)"""
    return bound_f32(pAx, d + 1) + FAST_ULPS * U24 * lse.abs().clamp(min=1.0)


def e2e_lse_bound(inp, logits):
    """(float64 lse of the whole vocabulary, the chain's bound on it): the softmax-weighted mean of the shard bounds
    plus the combine's fold"""
    x, Ax = logits
    rf = torch.logsumexp(x, 1)
    bq = 0.0
    for v0, v1 in inp["ranges"]:
        rq = torch.logsumexp(x[:, v0:v1], 1)
        bq = bq + L.vce_lse_bound(x[:, v0:v1], Ax[:, v0:v1], rq, inp["d"]) * torch.exp(rq - rf)
    return rf, bq + fold_bound(rf, inp["N"])


def loss_sum_bound(rf, b_lse, t, At, live, R, d):
    """as check_vce_fwd: per live row the lse's and the label logit's bound, then the row term, ceil(R / 256)
    strided adds, 6 shuffles, 4 waves"""
    return ((b_lse + bound_f32(At, d + 1)) * live).sum() + \
        bound_f32(((rf.abs() + t.abs()) * live).sum(), 1 + -(-R // 256) + 6 + 4)


def check_loss_out(out, rf, b_lse, t, At, live, R, d, zero_mean=True):
    """out = {sum of lse - label logit over the live rows, live count, mean}; t, At: the float64 label logits and
    their absolute-value map.  No live row: (0, 0) and, for the chain (zero_mean), a mean of exactly 0"""
    c = float(live.sum())
    res = {"count": L.exact(out[1], torch.tensor(c, device=out.device))}
    if c == 0:
        zero = torch.zeros((), device=out.device)
        res["sum"] = L.exact(out[0], zero)
        if zero_mean:
            res["mean"] = L.exact(out[2], zero)
        return res
    S = ((rf - t) * live).sum()
    b_S = loss_sum_bound(rf, b_lse, t, At, live, R, d)
    res["sum"] = ratio(out[0], S, b_S)
    res["mean"] = ratio(out[2], S / c, b_S / c + bound_f32(S.abs() / c, 1))
    return res


def check_combine(inp, logits, lse_parts, tgt, lse, out):
    """lse_parts [N][R], tgt [R] (summed over the shards), lse [R], out [3] as the kernels stored them"""
    x, Ax = logits
    lab, N, R, d = inp["labels"], inp["N"], inp["R"], inp["d"]
    live = (lab != 0).double()
    res = {}
    r = torch.logsumexp(D(lse_parts), 0)                                   # staged
    res["lse"] = ratio(lse, r * live, fold_bound(r, N) * live)
    rf, b_lse = e2e_lse_bound(inp, logits)                                 # end to end
    res["lse.e2e"] = ratio(lse, rf * live, b_lse * live)
    t, At = x.gather(1, lab[:, None])[:, 0], Ax.gather(1, lab[:, None])[:, 0]
    res.update(check_loss_out(out, rf, b_lse, t, At, live, R, d))
    return res


def grad_bound(x, Ax, Lg, live, onehot, r, d, sc):
    """losshead_ref.vce_grad_bound with the one-hot given as a tensor (a shard holds it only for its own labels)"""
    z = x - Lg[:, None]
    p = torch.exp(z)
    A = (p * (Ax + 1) + onehot) * live * sc
    return bound_bf16(r, A, d + 4) + p * live * sc * FAST_ULPS * U24 * z.abs().clamp(min=1.0) + TINY


def ref_shard_grad(x, lab, v0, v1, Lg, count, dloss):
    """(dlogits, one-hot) on columns [v0, v1) of the logits x given there, from the global lse"""
    own = owned(lab, v0, v1)
    oh = torch.zeros_like(x)
    oh[own, (lab - v0)[own]] = 1.0
    live = (lab != 0).double()[:, None]
    sc = dloss / count if count else 0.0
    return (torch.exp(x - Lg[:, None]) - oh) * live * sc, oh


def check_cols_bwd(inp, x, Ax, v0, v1, lse, count, dloss, dl, rows=None):
    """dl: the stored dlogits of vocabulary ids [v0, v1), whose float64 logits are x, Ax; lse: the stored global lse"""
    lab, Lg = L.ce_live(inp, rows), D(lse)
    r, oh = ref_shard_grad(x, lab, v0, v1, Lg, count, dloss)
    live = (lab != 0).double()[:, None]
    b = grad_bound(x, Ax, Lg, live, oh, r, inp["d"], abs(dloss / count) if count else 0.0)
    n = inp["R"] if rows is None else rows
    res = {"dlogits": ratio(dl[:n], r[:n], b[:n])}
    # exact zeros: label-0 rows; and no -1 where the label lives in another shard (every entry there is >= 0)
    dead = lab[:n] == 0
    res["dlogits.dead"] = 0.0 if float(dl[:n][dead].float().abs().sum()) == 0 else math.inf
    away = (lab[:n] != 0) & ~owned(lab[:n], v0, v1)
    sign = 1.0 if count and dloss / count >= 0 else -1.0
    res["dlogits.away"] = 0.0 if bool((dl[:n][away].float() * sign >= 0).all()) else math.inf
    return res


def check_shard_bwd(inp, logits, v0, v1, lse, count, dloss, dl, rows=None):
    """staged: from the global lse the combine stored; logits: the whole vocabulary's"""
    x, Ax = (t[:, v0:v1] for t in logits)
    return check_cols_bwd(inp, x, Ax, v0, v1, lse, count, dloss, dl, rows)


def check_wgrad(dl, h, W0, b0, W, b, v0, v1, splits):
    """W, b: the full-size gradients after rs_linear_wgrad accumulated dl^T h / colsum(dl) onto rows [v0, v1) of the
    prefill W0, b0; every other row bit for bit the prefill"""
    R = dl.shape[0]
    g, a = D(dl).t() @ D(h), D(dl).abs().t() @ D(h).abs()
    res = {"dW": ratio(W[v0:v1], D(W0[v0:v1]) + g, bound_f32(D(W0[v0:v1]).abs() + a, R + splits)),
           "db": ratio(b[v0:v1], D(b0[v0:v1]) + D(dl).sum(0), bound_f32(D(b0[v0:v1]).abs() + D(dl).abs().sum(0),
                                                                     R + splits))}
    same = torch.ones(W.shape[0], dtype=torch.bool, device=W.device)
    same[v0:v1] = False
    res["dW.outside"] = 0.0 if torch.equal(W[same], W0[same]) and torch.equal(b[same], b0[same]) else math.inf
    return res


def dh_bound(dl, Es, splits):
    return bound_f32(D(dl).abs() @ D(Es).abs(), -(-dl.shape[1] // splits) + splits)


# ------------------------------------------------------------------ emulation
def _emu_tile_lse(x):
    """per 128-column tile the (max, sum) pair, the pairs folded (as losshead_ref.emu_vce_fwd)"""
    V1 = x.shape[1]
    nt = -(-V1 // 128)
    xp = torch.full((x.shape[0], nt * 128), -math.inf)
    xp[:, :V1] = x
    xt = xp.view(-1, nt, 128)
    mx = xt.max(-1).values
    sm = torch.exp(xt - mx[..., None]).sum(-1)
    m = mx.max(-1).values
    return m + torch.log((sm * torch.exp(mx - m[:, None])).sum(-1))


def emu_chain(inp, count=None, dloss=1.0, mut=None):
    """the sharded chain in float32 (dlogits bf16) -> lse_parts [N][R], tgt_parts [N][R], lse, out, [dlogits]"""
    lab, R, rng = inp["labels"], inp["R"], inp["ranges"]
    x = inp["h"].float() @ inp["E"].float().t()
    if inp["bias"] is not None:
        x = x + inp["bias"]
    live = lab != 0
    lse_parts, tgt_parts = [], []
    for v0, v1 in rng:
        lse_parts.append(torch.where(live, _emu_tile_lse(x[:, v0:v1]), torch.zeros(())))
        own = owned(lab, v0, v1)
        col = (v0 + lab).clamp(max=v1 - 1) if mut == "no_v0" else lab
        tgt_parts.append(torch.where(own, x.gather(1, col[:, None])[:, 0], torch.zeros(())))
    lse_parts, tgt_parts = torch.stack(lse_parts), torch.stack(tgt_parts)
    parts = lse_parts[:-1] if mut == "drop_shard" else lse_parts
    mx = parts.max(0).values
    Lg = mx if mut == "local_max" else mx + torch.log(torch.exp(parts - mx).sum(0))
    Lg = torch.where(live, Lg, torch.zeros(()))
    tgt = tgt_parts.sum(0)
    S, c = ((Lg - tgt) * live).sum(), live.float().sum()
    out = torch.stack([S, c, S / c if c > 0 else torch.zeros(())])
    sc = np.float32(dloss) / np.float32(count if count is not None else float(c)) if (count or c > 0) else \
        np.float32(math.inf)
    dls = []
    for v0, v1 in rng:
        g = torch.exp(x[:, v0:v1] - Lg[:, None])
        own = live if mut == "onehot_all" else owned(lab, v0, v1)
        g[own, ((lab - v0) % (v1 - v0))[own]] -= 1.0
        if mut == "dead_mul":
            g = g * (live.float() * sc)[:, None]             # inf * 0 on a label-0 row with a logit past 88.7
        else:
            g = torch.where(live[:, None], g * sc, torch.zeros(()))
        dls.append(g.bfloat16())
    return {"lse_parts": lse_parts, "tgt_parts": tgt_parts, "lse": Lg, "out": out, "dl": dls}


def check_chain(inp, logits, got, count, dloss):
    """every check of the chain on what a run (kernels or emulation) stored; count: the divisor the backward took"""
    res = {}

    def worst(d_):
        for k, v in d_.items():
            res[k] = max(res.get(k, 0.0), v)

    for q, (v0, v1) in enumerate(inp["ranges"]):
        worst(check_shard_lse(inp, logits, q, got["lse_parts"][q]))
        worst(check_label_logits(inp, logits, q, got["tgt_parts"][q]))
        worst(check_shard_bwd(inp, logits, v0, v1, got["lse"], count, dloss, got["dl"][q]))
    worst(check_combine(inp, logits, got["lse_parts"], got["tgt_parts"].sum(0), got["lse"], got["out"]))
    return res
