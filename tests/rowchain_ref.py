"""float64 reference, error bounds and a float32/bf16 emulation of the fused SAS row-chain kernels (rowchain.hip).

Reference.  One plain torch float64 function per stage, written from the formulas in include/recsys_hip.h.  The
checkers below apply them STAGED: every stage is fed the tensor the kernel itself stored for the stage before
(the kernels continue from the bf16 value they just stored), so errors do not compound and a failure names
its stage.  Three intermediates are rounded to bf16 by the kernels without being stored (dxkv and dQ of
rs_sas_block_in_bwd, dz of rs_sas_block_out_bwd); the reference keeps them in float64 and their rounding enters
the bound as the term P.

Bound (derived, not fitted).  For a bf16 output with float64 reference r

    |hip - r| <= 2 * ( 2^-8 |r|  +  2^-8 P  +  2 K 2^-24 A )

  2^-8 |r|     the output's own rounding (bf16 keeps 8 significant bits);
  2 K 2^-24 A  the standard float32 bound of a length-K reduction, A = the same map on absolute values
               (|x| |W|^T + |b| + |resid|, or the absolute-value form of the LayerNorm row formulas, in which
               |x - mean| is replaced by |x| + |mean| so that the float32 error of the row mean is covered);
  P            the absolute-value propagation of a 2^-8 relative perturbation of the unstored rounded
               intermediates through the rest of the stage; through the LayerNorm backward, per row, with
               e = |intermediate * gamma|:  rstd (|e_k| + mean|e| + |u_k| mean(|e| |u|)), u = (x - mean) rstd.
float32 outputs drop the first term.  K is the reduction length plus the few elementwise float32 operations
around it, never more than 128 for a bf16 output; for the per-workgroup partial sums it is the number of float32
operations on the longest path to the sum (stated at each use).  The factor 2 in front is the only slack.

Partial sums (LayerNorm affine, BCE) are checked twice: summed over the workgroups against the float64 column sums,
and workgroup by workgroup against the float64 sum over exactly the rows that the dealing (wave_tiles) gives that
workgroup.  With 2-3 tiles per wave a workgroup sums 16-24 tiles, so one lost tile is 1/16 to 1/24 of its terms;
the gradient inputs carry a per-feature mean so that these sums do not cancel.

Emulation.  The same stages in float32 with a bf16 rounding at every point where the kernels round (stored or
not), in torch's summation order: a correct kernel as far as the bound is concerned.  tests/test_rowchain_ref.py
holds it to the bound on the CPU (so the bound admits a correct kernel) and checks that mutations of it are rejected.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

U8, U24 = 2.0 ** -8, 2.0 ** -24
TR, NW = 16, 8              # rows per wave tile, waves per workgroup
EPS = float(np.float32(1e-8))
GUARD = 32


def D(t):
    return t.double()


def rb(t):
    """round to bf16, keep the dtype"""
    return t.bfloat16().to(t.dtype)


def kmul(p):
    """the kernels' dropout multiplier 1/(1-p), formed in float32"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


# ------------------------------------------------------------------ tile dealing (model of tiles_of_wave)
def wave_tiles(M, ncu):
    """{(workgroup, wave): range of 16-row tiles} for M rows on a part with ncu compute units."""
    nt = -(-M // TR)
    G = min(nt, ncu)
    out = {}
    for w in range(G):
        for wave in range(NW):
            if G >= 8 and G % 8 == 0:
                x, Gx = w & 7, G >> 3
                first, step, end = x * nt // 8 + (w >> 3) + Gx * wave, Gx * NW, (x + 1) * nt // 8
            else:
                first, step, end = w + G * wave, G * NW, nt
            out[(w, wave)] = range(first, max(first, end), step)
    return out


def max_tiles_per_wave(M, ncu):
    return max(len(r) for r in wave_tiles(M, ncu).values())


@functools.lru_cache(maxsize=64)
def tile_owner(M, ncu):
    """(workgroup of tile t, the iteration of its wave's loop that runs it) as two tuples over the tiles"""
    nt = -(-M // TR)
    wg, it = [-1] * nt, [-1] * nt
    for (w, _), r in wave_tiles(M, ncu).items():
        for k, t in enumerate(r):
            assert wg[t] < 0
            wg[t], it[t] = w, k
    assert min(wg) >= 0
    return tuple(wg), tuple(it)


def row_owner(M, ncu, dev):
    return torch.tensor(tile_owner(M, ncu)[0], device=dev).repeat_interleave(TR)[:M]


def wg_sum(terms, owner, G):
    """float64 sums of per-row terms [M, n] over the rows of each workgroup -> [G, n]"""
    return torch.zeros(G, terms.shape[1], dtype=torch.float64, device=terms.device).index_add_(0, owner, terms)


# ------------------------------------------------------------------ float64 stages
def s_embed(E, Ptab, ids, T, scale, me):
    """x0 = (E[ids] scale + P[row % T]) * dropout * (ids != 0);  me: multiplier tensor (0 or 1/(1-p))"""
    t = torch.arange(ids.numel(), device=ids.device) % T
    return (D(E)[ids] * scale + D(Ptab)[t]) * me * (ids != 0).double()[:, None]


def s_stats(x, eps=EPS):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return mu, 1.0 / torch.sqrt(var + eps)


def s_ln(x, g, b, mu, rs):
    return (x - mu) * rs * g + b


def s_ln_abs(x, g, b, rs):
    ax = x.abs()
    return (ax + ax.mean(-1, keepdim=True)) * rs * g.abs() + b.abs()


def s_lin(x, W, b=None):
    y = x @ D(W).t()
    return y if b is None else y + D(b)


def s_lin_abs(x, W, b=None):
    y = x.abs() @ D(W).abs().t()
    return y if b is None else y + D(b).abs()


def s_ln_bwd(dy, x, g, mu, rs):
    """(dx, dgamma terms, dbeta terms): dx = rstd (dy g - mean(dy g) - u mean(dy g u)), u = (x - mean) rstd"""
    u = (x - mu) * rs
    gq = dy * g
    dx = rs * (gq - gq.mean(-1, keepdim=True) - u * (gq * u).mean(-1, keepdim=True))
    return dx, dy * u, dy


def s_ln_bwd_abs(ady, x, g, mu, rs, exact_u=False):
    """absolute-value form of s_ln_bwd's dx for |dy| = ady (exact_u: |u| itself, the closed form of P)"""
    u = ((x - mu) * rs).abs() if exact_u else (x.abs() + mu.abs()) * rs
    gq = ady * g.abs()
    return rs * (gq + gq.mean(-1, keepdim=True) + u * (gq * u).mean(-1, keepdim=True)), u


def softplus(z):
    return torch.clamp(z, min=0) + torch.log1p(torch.exp(-z.abs()))


# ------------------------------------------------------------------ bounds and the comparison
def bound_bf16(r, A, K, P=0.0):
    K = min(K, 128)
    return 2.0 * (U8 * r.abs() + U8 * P + 2.0 * K * U24 * A)


def bound_f32(A, K, P=0.0):
    return 2.0 * (U8 * P + 2.0 * K * U24 * A)


def ratio(hip, r, bound):
    """worst err / bound over the tensor (0 where both are 0; inf for a NaN or an error at a zero bound)"""
    err = (D(hip) - r).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(q.max()) if q.numel() else 0.0


def check_parts(res, name, part, terms, aterms, K, inp, pterms=None):
    """res[name]: the partial sets [G][n] summed over the workgroups against the float64 column sums of terms [M][n]
    (aterms: the same on absolute values, pterms: the P terms); res[name + "/wg"]: each workgroup's own set against
    the float64 sum over the rows dealt to it"""
    G = part.shape[0]
    zero = torch.zeros_like(terms)
    pterms = zero if pterms is None else pterms
    res[name] = ratio(D(part).sum(0), terms.sum(0), bound_f32(aterms.sum(0), K, pterms.sum(0)))
    own = row_owner(inp["M"], inp["ncu"], terms.device)
    res[name + "/wg"] = ratio(part, wg_sum(terms, own, G), bound_f32(wg_sum(aterms, own, G), K, wg_sum(pterms, own, G)))


def _kpart(inp):
    # LayerNorm affine partials: 4 operations form a term, 16 rows of a tile, the wave's tiles, 8 waves
    return 4 + TR + max_tiles_per_wave(inp["M"], inp["ncu"]) + NW


# ------------------------------------------------------------------ checkers: {tensor name: worst err / bound}
def check_embed(inp, out):
    me = D(inp["me"]) * kmul(inp["p"])
    r = s_embed(inp["E"], inp["Ptab"], inp["ids"], inp["T"], inp["scale"], me)
    t = torch.arange(inp["M"], device=r.device) % inp["T"]
    A = (D(inp["E"])[inp["ids"]].abs() * inp["scale"] + D(inp["Ptab"])[t].abs()) * me
    # K = 6: multiply, add, the multiplier's own two roundings, two multiplies
    return {"x0": ratio(out["x0"], r, bound_bf16(r, A, 6))}


def check_block_in(inp, out, x=None):
    x = D(inp["x"] if x is None else x)
    d = x.shape[1]
    g, b = D(inp["ln1w"]), D(inp["ln1b"])
    mu, rs = s_stats(x)
    res = {"mean": ratio(out["mean"], mu[:, 0], bound_f32(x.abs().mean(-1), d + 1)),
           "rstd": ratio(out["rstd"], rs[:, 0], bound_f32(rs[:, 0], d))}
    Qr = s_ln(x, g, b, mu, rs)
    res["Q"] = ratio(out["Q"], Qr, bound_bf16(Qr, s_ln_abs(x, g, b, rs), d))
    Qh = D(out["Q"])
    r = s_lin(Qh, inp["Wq"], inp["bq"])
    res["q"] = ratio(out["q"], r, bound_bf16(r, s_lin_abs(Qh, inp["Wq"], inp["bq"]), d))
    r = s_lin(x, inp["Wkv"], inp["bkv"])
    res["kv"] = ratio(out["kv"], r, bound_bf16(r, s_lin_abs(x, inp["Wkv"], inp["bkv"]), d))
    return res


def check_block_out(inp, out, head=False, divisor=None):
    o, Q = D(inp["o"]), D(inp["Q"])
    d = o.shape[1]
    k = kmul(inp["p"])
    m1, m2 = D(inp["m1"]) * k, D(inp["m2"]) * k
    keep = (inp["ids"] != 0).double()[:, None]
    res = {}
    r = Q + s_lin(o, inp["Wo"], inp["bo"])
    res["x1"] = ratio(out["x1"], r, bound_bf16(r, Q.abs() + s_lin_abs(o, inp["Wo"], inp["bo"]), d))
    x1 = D(out["x1"])
    g, b = D(inp["ln2w"]), D(inp["ln2b"])
    mu, rs = s_stats(x1)
    res["mean"] = ratio(out["mean"], mu[:, 0], bound_f32(x1.abs().mean(-1), d + 1))
    res["rstd"] = ratio(out["rstd"], rs[:, 0], bound_f32(rs[:, 0], d))
    r = s_ln(x1, g, b, mu, rs)
    res["z"] = ratio(out["z"], r, bound_bf16(r, s_ln_abs(x1, g, b, rs), d))
    z = D(out["z"])
    r = torch.relu(s_lin(z, inp["W1"], inp["b1"])) * m1
    res["h1"] = ratio(out["h1"], r, bound_bf16(r, s_lin_abs(z, inp["W1"], inp["b1"]) * m1, d + 3))
    h1 = D(out["h1"])
    r = (s_lin(h1, inp["W2"], inp["b2"]) * m2 + z) * keep
    A = (s_lin_abs(h1, inp["W2"], inp["b2"]) * m2 + z.abs()) * keep
    res["xn"] = ratio(out["xn"], r, bound_bf16(r, A, d + 3))
    if not head:
        return res
    xn = D(out["xn"])
    g, b = D(inp["lnlw"]), D(inp["lnlb"])
    mu, rs = s_stats(xn)
    r = s_ln(xn, g, b, mu, rs)
    res["f"] = ratio(out["f"], r, bound_bf16(r, s_ln_abs(xn, g, b, rs), d))
    f = D(out["f"])
    Ep, En = D(inp["E"])[inp["pos"]], D(inp["E"])[inp["neg"]]
    res["pl"] = ratio(out["pl"], (f * Ep).sum(-1), bound_f32((f.abs() * Ep.abs()).sum(-1), d))
    res["nl"] = ratio(out["nl"], (f * En).sum(-1), bound_f32((f.abs() * En.abs()).sum(-1), d))
    pl, nl = D(out["pl"]), D(out["nl"])
    valid = (inp["pos"] != 0).double()
    c = divisor if divisor is not None else float(valid.sum())
    sc = 1.0 / c if c else 0.0                              # no valid position: every gradient is zero
    # sigmoid in float32 from a fast exp: |error| <= (8 + |z|) 2^-24 in absolute terms, then the scale's rounding
    res["dpl"] = ratio(out["dpl"], (torch.sigmoid(pl) - 1) * sc * valid, bound_f32(sc * (1 + pl.abs()) * valid, 8))
    res["dnl"] = ratio(out["dnl"], torch.sigmoid(nl) * sc * valid, bound_f32(sc * (1 + nl.abs()) * valid, 8))
    dpl, dnl = D(out["dpl"])[:, None], D(out["dnl"])[:, None]
    df, adf = dpl * Ep + dnl * En, dpl.abs() * Ep.abs() + dnl.abs() * En.abs()
    r, tg, tb = s_ln_bwd(df, xn, g, mu, rs)
    A, ut = s_ln_bwd_abs(adf, xn, g, mu, rs)
    res["dx"] = ratio(out["dx"], r, bound_bf16(r, A, d + 4))
    K = _kpart(inp) + 3                                     # + the term's df = dpl E[pos] + dnl E[neg]
    check_parts(res, "lnpart.g", out["lnpart"][:, 0], tg, adf * ut, K + d, inp)   # u carries the row statistics
    check_parts(res, "lnpart.b", out["lnpart"][:, 1], tb, adf, K, inp)
    hp = D(out["part"]).sum(0)
    # loss partials: softplus to ~8 float32 operations, the wave's tiles, 6 butterfly steps, 8 waves
    K = 8 + max_tiles_per_wave(inp["M"], inp["ncu"]) + 6 + NW
    sp, sn = (softplus(-pl) * valid).sum(), (softplus(nl) * valid).sum()
    res["part.sp"] = ratio(hp[0], sp, bound_f32(sp, K))
    res["part.sn"] = ratio(hp[1], sn, bound_f32(sn, K))
    res["part.count"] = 0.0 if float(hp[2]) == float(valid.sum()) else math.inf
    own, G = row_owner(inp["M"], inp["ncu"], pl.device), out["part"].shape[0]
    t = wg_sum(torch.stack([softplus(-pl) * valid, softplus(nl) * valid, valid], 1), own, G)
    res["part.sp/wg"] = ratio(out["part"][:, 0], t[:, 0], bound_f32(t[:, 0], K))
    res["part.sn/wg"] = ratio(out["part"][:, 1], t[:, 1], bound_f32(t[:, 1], K))
    res["part.count/wg"] = 0.0 if torch.equal(D(out["part"][:, 2]), t[:, 2]) else math.inf
    return res


def check_block_out_bwd(inp, out):
    dxn, h1, x1 = D(inp["dxn"]), D(inp["h1"]), D(inp["x1"])
    d = dxn.shape[1]
    k = kmul(inp["p"])
    m1, m2 = D(inp["m1"]) * k, D(inp["m2"]) * k
    dzres = dxn * (inp["ids"] != 0).double()[:, None]
    res = {}
    r = dzres * m2
    res["dy2"] = ratio(out["dy2"], r, bound_bf16(r, r.abs(), 3))
    dy2 = D(out["dy2"])
    relu = (h1 > 0).double()
    r = s_lin(dy2, inp["W2T"]) * relu * m1
    res["da1"] = ratio(out["da1"], r, bound_bf16(r, s_lin_abs(dy2, inp["W2T"]) * relu * m1, d + 3))
    da1 = D(out["da1"])
    dz = s_lin(da1, inp["W1T"]) + dzres                    # rounded by the kernel, not stored: enters as P
    adz = s_lin_abs(da1, inp["W1T"]) + dzres.abs()
    g, mu, rs = D(inp["ln2w"]), D(inp["mean2"])[:, None], D(inp["rstd2"])[:, None]
    r, tg, tb = s_ln_bwd(dz, x1, g, mu, rs)
    A, ut = s_ln_bwd_abs(adz, x1, g, mu, rs)
    P, u = s_ln_bwd_abs(dz.abs(), x1, g, mu, rs, exact_u=True)
    res["dx1"] = ratio(out["dx1"], r, bound_bf16(r, A, 2 * d + 4, P))
    K = _kpart(inp) + d                                     # + dz's own reduction
    check_parts(res, "part.g", out["part"][:, 0], tg, adz * ut, K, inp, dz.abs() * u)
    check_parts(res, "part.b", out["part"][:, 1], tb, adz, K, inp, dz.abs())
    dx1 = D(out["dx1"])
    r = s_lin(dx1, inp["WoT"])
    res["dout"] = ratio(out["dout"], r, bound_bf16(r, s_lin_abs(dx1, inp["WoT"]), d))
    if "delta" in out:
        do, o = D(out["dout"]), D(inp["o"])
        res["delta"] = ratio(out["delta"], (do * o).sum(-1), bound_f32((do * o).abs().sum(-1), d))
    return res


def check_block_in_bwd(inp, out):
    dq, dkv, dx1, x = D(inp["dq"]), D(inp["dkv"]), D(inp["dx1b"]), D(inp["xb"])
    d = dq.shape[1]
    W = inp["WinT"]
    Wq, Wk, Wv = W[:, :d], W[:, d:2 * d], W[:, 2 * d:]
    dxkv = s_lin(dkv[:, :d], Wk) + s_lin(dkv[:, d:], Wv)    # rounded by the kernel, not stored: enters as P
    adxkv = s_lin_abs(dkv[:, :d], Wk) + s_lin_abs(dkv[:, d:], Wv)
    dQ = dx1 + s_lin(dq, Wq)                                # likewise
    adQ = dx1.abs() + s_lin_abs(dq, Wq)
    g, mu, rs = D(inp["ln1w"]), D(inp["mean1"])[:, None], D(inp["rstd1"])[:, None]
    t, tg, tb = s_ln_bwd(dQ, x, g, mu, rs)
    At, ut = s_ln_bwd_abs(adQ, x, g, mu, rs)
    Pt, u = s_ln_bwd_abs(dQ.abs(), x, g, mu, rs, exact_u=True)
    r = dxkv + t
    res = {"dx": ratio(out["dx"], r, bound_bf16(r, adxkv + At, 2 * d + 5, dxkv.abs() + Pt))}
    K = _kpart(inp) + d
    check_parts(res, "part.g", out["part"][:, 0], tg, adQ * ut, K, inp, dQ.abs() * u)
    check_parts(res, "part.b", out["part"][:, 1], tb, adQ, K, inp, dQ.abs())
    return res


# ------------------------------------------------------------------ inputs
def make_ids(M, V, gen, dev):
    """ids, pos, neg with a padded prefix, a whole 16-row tile of zeros (where M allows), a zero in the last row
    (ids and pos at different places, so every combination occurs) and zeros among neg"""
    def draw(lo):
        return torch.randint(lo, V, (M,), generator=gen, device=dev, dtype=torch.int64)
    ids, pos, neg = draw(1), draw(1), draw(0)
    ids[:min(5, M)] = 0
    pos[:min(7, M)] = 0
    if M >= 64:
        ids[32:48] = 0
        pos[16:32] = 0
    ids[M - 1] = 0
    pos[M - 1] = 0
    neg[::11] = 0
    return ids, pos, neg


def largest_divisor(M, cap=300):
    return max(t for t in range(1, min(M, cap) + 1) if M % t == 0)


def make_inputs(M, d, p, ncu, dev="cpu", seed=0, V=97):
    """Inputs of all six entry points for M rows at width d (dropout masks excluded: the caller adds the bool keep
    masks me, m1, m2).  Weights ~ 1/sqrt(d), non-zero biases, LayerNorm affine distinct per feature, activations
    distinct per row."""
    gen = torch.Generator(device=dev).manual_seed(seed * 1000003 + M * 131 + d)
    bf, f32 = torch.bfloat16, torch.float32

    def rn(*shape, s=1.0, dt=bf):
        return (torch.randn(*shape, generator=gen, device=dev, dtype=f32) * s).to(dt)

    def act(s=1.0, mean=0.0, phase=0.0):
        """mean: a per-feature mean of that size (in units of s), different per feature and per phase"""
        rows = torch.arange(M, device=dev, dtype=f32)[:, None]
        cols = torch.arange(d, device=dev, dtype=f32)[None, :]
        return (rn(M, d, dt=f32) * s + 0.25 * s * torch.sin(0.37 * rows) + mean * s * torch.cos(0.7 * cols + phase)).to(bf)

    def affine():
        c = torch.arange(d, device=dev, dtype=f32)
        return ((0.6 + 0.9 * c / d) * (1 - 2 * (c % 3 == 1).float())).contiguous(), (0.3 * torch.cos(1.3 * c) + 0.05)

    w = 1.0 / math.sqrt(d)
    inp = {"M": M, "d": d, "p": p, "ncu": ncu, "T": largest_divisor(M), "scale": float(np.float32(math.sqrt(d)))}
    inp["ids"], inp["pos"], inp["neg"] = make_ids(M, V, gen, dev)
    inp["E"], inp["Ptab"] = rn(V, d, s=w), rn(inp["T"], d, s=0.5)
    for n in ("ln1", "ln2", "lnl"):
        inp[n + "w"], inp[n + "b"] = affine()
    for n in ("Wq", "Wo", "W1", "W2"):
        inp[n] = rn(d, d, s=w)
    inp["Wkv"] = rn(2 * d, d, s=w)
    for n in ("bq", "bo", "b1", "b2"):
        inp[n] = rn(d, s=0.2, dt=f32)
    inp["bkv"] = rn(2 * d, s=0.2, dt=f32)
    inp["WinT"] = torch.cat([inp["Wq"], inp["Wkv"]], 0).t().contiguous()
    for n in ("Wo", "W1", "W2"):
        inp[n + "T"] = inp[n].t().contiguous()
    inp["x"], inp["o"], inp["Q"] = act(), act(0.7), act()
    # backward inputs: saved tensors with consistent statistics; the gradients and the LayerNorm inputs carry a
    # per-feature mean, so the affine partial sums grow with the row count instead of cancelling
    inp["dxn"], inp["x1"], inp["h1"] = act(0.05, 1.0), act(1.3, 1.0, 0.4), torch.relu(act()).to(bf)
    inp["dq"], inp["dx1b"], inp["xb"] = act(0.05, 1.0, 1.1), act(0.05, 1.0, 2.0), act(1.0, 1.0, 2.4)
    inp["dkv"] = torch.cat([act(0.05), act(0.05)], 1).contiguous()
    for x, mu, rs in (("x1", "mean2", "rstd2"), ("xb", "mean1", "rstd1")):
        a, b = s_stats(D(inp[x]))
        inp[mu], inp[rs] = a[:, 0].float().contiguous(), b[:, 0].float().contiguous()
    return inp


def random_masks(inp, seed=1):
    M, d, p = inp["M"], inp["d"], inp["p"]
    gen = torch.Generator().manual_seed(seed)
    for n in ("me", "m1", "m2"):
        inp[n] = (torch.rand(M, d, generator=gen) >= p) if p > 0 else torch.ones(M, d, dtype=torch.bool)
    return inp


# ------------------------------------------------------------------ float32 / bf16 emulation of the kernels
def _f(t):
    return t.float()


def _stats32(x):
    mu = x.mean(-1, keepdim=True)
    return mu, 1.0 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + np.float32(EPS))


def _ln_bwd32(dy, x, g, mu, rs):
    u = x - mu
    gq = dy * g
    dx = rs * (gq - gq.mean(-1, keepdim=True)) - rs ** 3 * (gq * u).mean(-1, keepdim=True) * u
    return dx, dy * (u * rs), dy


def _partials32(terms, ncu, skip_tile=None):
    """per-workgroup float32 sums of per-row terms [M, d]: 16-row tiles, then each tile to its workgroup"""
    M, d = terms.shape
    nt = -(-M // TR)
    G = min(nt, ncu)
    t = torch.zeros(nt * TR, d, dtype=terms.dtype)
    t[:M] = terms
    tiles = t.view(nt, TR, d).sum(1)
    if skip_tile is not None:
        tiles[skip_tile] = 0
    return torch.zeros(G, d, dtype=terms.dtype).index_add_(0, torch.tensor(tile_owner(M, ncu)[0]), tiles)


def _parts32(tg, tb, ncu, skip_tile=None):
    return torch.stack([_partials32(tg, ncu, skip_tile), _partials32(tb, ncu, skip_tile)], 1).contiguous()


def emu_embed(inp):
    me = _f(inp["me"]) * np.float32(kmul(inp["p"]))
    t = torch.arange(inp["M"]) % inp["T"]
    x = (_f(inp["E"])[inp["ids"]] * np.float32(inp["scale"]) + _f(inp["Ptab"])[t]) * me
    return {"x0": (x * (inp["ids"] != 0).float()[:, None]).bfloat16()}


def emu_block_in(inp, x=None):
    x = _f(inp["x"] if x is None else x)
    mu, rs = _stats32(x)
    Q = ((x - mu) * rs * inp["ln1w"] + inp["ln1b"]).bfloat16()
    q = F.linear(_f(Q), _f(inp["Wq"]), inp["bq"]).bfloat16()
    kv = F.linear(x, _f(inp["Wkv"]), inp["bkv"]).bfloat16()
    return {"Q": Q, "mean": mu[:, 0].clone(), "rstd": rs[:, 0].clone(), "q": q, "kv": kv}


def emu_block_out(inp, head=False, divisor=None, skip_tile=None):
    k = np.float32(kmul(inp["p"]))
    m1, m2 = _f(inp["m1"]) * k, _f(inp["m2"]) * k
    keep = (inp["ids"] != 0).float()[:, None]
    x1 = rb(_f(inp["Q"]) + F.linear(_f(inp["o"]), _f(inp["Wo"]), inp["bo"]))
    mu, rs = _stats32(x1)
    z = rb((x1 - mu) * rs * inp["ln2w"] + inp["ln2b"])
    h1 = rb(torch.relu(F.linear(z, _f(inp["W1"]), inp["b1"])) * m1)
    xn = rb((F.linear(h1, _f(inp["W2"]), inp["b2"]) * m2 + z) * keep)
    out = {"x1": x1.bfloat16(), "mean": mu[:, 0].clone(), "rstd": rs[:, 0].clone(), "z": z.bfloat16(),
           "h1": h1.bfloat16(), "xn": xn.bfloat16()}
    if not head:
        return out
    mu, rs = _stats32(xn)
    f = rb((xn - mu) * rs * inp["lnlw"] + inp["lnlb"])
    Ep, En = _f(inp["E"])[inp["pos"]], _f(inp["E"])[inp["neg"]]
    pl, nl = (f * Ep).sum(-1), (f * En).sum(-1)
    valid = (inp["pos"] != 0).float()
    c = divisor if divisor is not None else float(valid.sum())
    sc = np.float32(1.0) / np.float32(c) if c else np.float32(0.0)
    dpl, dnl = (torch.sigmoid(pl) - 1) * sc * valid, torch.sigmoid(nl) * sc * valid
    df = dpl[:, None] * Ep + dnl[:, None] * En
    dx, tg, tb = _ln_bwd32(df, xn, inp["lnlw"], mu, rs)
    ncu = inp["ncu"]
    part = torch.stack([_partials32((F.softplus(-pl) * valid)[:, None], ncu)[:, 0],
                        _partials32((F.softplus(nl) * valid)[:, None], ncu)[:, 0],
                        _partials32(valid[:, None], ncu)[:, 0]], 1).contiguous()
    out.update(f=f.bfloat16(), pl=pl, nl=nl, dpl=dpl, dnl=dnl, dx=dx.bfloat16(),
               lnpart=_parts32(tg, tb, ncu, skip_tile), part=part)
    return out


def emu_block_out_bwd(inp, delta=False, skip_tile=None):
    k = np.float32(kmul(inp["p"]))
    m1, m2 = _f(inp["m1"]) * k, _f(inp["m2"]) * k
    dzres = _f(inp["dxn"]) * (inp["ids"] != 0).float()[:, None]
    dy2 = rb(dzres * m2)
    da1 = rb(F.linear(dy2, _f(inp["W2T"])) * (_f(inp["h1"]) > 0).float() * m1)
    dz = rb(F.linear(da1, _f(inp["W1T"])) + dzres)
    dx1, tg, tb = _ln_bwd32(dz, _f(inp["x1"]), inp["ln2w"], inp["mean2"][:, None], inp["rstd2"][:, None])
    dx1 = rb(dx1)
    dout = rb(F.linear(dx1, _f(inp["WoT"])))
    out = {"dy2": dy2.bfloat16(), "da1": da1.bfloat16(), "dx1": dx1.bfloat16(), "dout": dout.bfloat16(),
           "part": _parts32(tg, tb, inp["ncu"], skip_tile)}
    if delta:
        out["delta"] = (dout * _f(inp["o"])).sum(-1)
    return out


def emu_block_in_bwd(inp, skip_tile=None):
    d = inp["d"]
    W, dkv = _f(inp["WinT"]), _f(inp["dkv"])
    dxkv = rb(F.linear(dkv[:, :d], W[:, d:2 * d]) + F.linear(dkv[:, d:], W[:, 2 * d:]))
    dQ = rb(_f(inp["dx1b"]) + F.linear(_f(inp["dq"]), W[:, :d]))
    t, tg, tb = _ln_bwd32(dQ, _f(inp["xb"]), inp["ln1w"], inp["mean1"][:, None], inp["rstd1"][:, None])
    return {"dx": (t + dxkv).bfloat16(), "part": _parts32(tg, tb, inp["ncu"], skip_tile)}


def case_rows(ncu):
    """The row counts of the kernel tests: {case: [M, ...]} for a part with ncu compute units."""
    return {1: [1, 16, 17], 2: [16 * 8 - 11], 3: [16 * 13 - 3], 4: [16 * (ncu + 3) - 9],
            5: [16 * (16 * ncu + 43) - 11]}
