"""float64 reference, error bounds and a float32/bf16 emulation of the embedding, loss-head and row-gather kernels
(embedding.hip, head.hip, loss.hip, vocab_ce.hip, rows.hip): the layer every model passes on its way in and out.

Reference.  One plain torch float64 function per entry point, written from the formulas in include/recsys_hip.h.
Where torch has the operation it is used in float64 (F.embedding(padding_idx=0), F.binary_cross_entropy_with_logits,
F.cross_entropy(ignore_index=0), autograd for the embedding and cross-entropy backward), so the reference does not
share a formula with the kernels.  The checks are STAGED as in rowchain_ref: a kernel that continues from a tensor
another kernel stored (rs_sas_head_bwd from pl, nl, mean, rstd and part; rs_ce_bwd and rs_vocab_ce_bwd from the row
log-sum-exp) is fed the stored tensor, and so is its reference.

Bounds (derived, not fitted): rowchain_ref.bound_bf16 / bound_f32, i.e. 2 (2^-8 |r| + 2 K 2^-24 A) with A the same
map on absolute values and K the number of float32 operations on the longest path, stated at every use.  Sums built
from float atomics (the table gradients) have no fixed order: their K is the number of contributions to that table
row (+ the operations that form a contribution).  Copies (rs_gather_rows, rs_scatter_rows) are held to equality.

The one measured constant.  vocab_ce.hip's epilogues and tile fold use the fast intrinsics __expf / __logf, whose
error is not a derivable multiple of 2^-24 and for which the ROCm tree used here carries no accuracy table.
FAST_ULPS states it: the error of one such evaluation in units of 2^-24 max(|argument or result|, 1).  It was
measured once on an MI355X as the worst |lse_hip - lse_fp64| over the cases of tests/test_vocab_ce_ref_gpu.py in units
of 2^-24 max(|lse|, 1) (the test prints it): MEASURED_FAST_ULPS = 2.534 (2.462 on the inputs as committed, 2.534 on an
earlier draw of the same shapes: the larger is kept), times the factor FAST_FACTOR = 4.  float32 underflow (TINY =
2^-126 per term where an exp may flush to zero) is the format's own.

Emulation.  The same stages in float32 with a bf16 rounding wherever the kernels round (head_fwd_kernel rounds f to
bf16 BEFORE the dot products), each with a `mut` switch that plants one specific mistake.  tests/test_losshead_ref.py
holds the emulation to the bounds on the CPU and checks that every mutation is rejected at the smallest shape of the
GPU lists below that exercises it.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from rowchain_ref import (D, EPS, GUARD, U24, bound_bf16, bound_f32, kmul, ratio, rb, s_ln, s_ln_abs, s_ln_bwd,
                          s_ln_bwd_abs, s_stats, softplus)

BF, F32 = torch.bfloat16, torch.float32
MEASURED_FAST_ULPS, FAST_FACTOR = 2.534, 4.0
FAST_ULPS = MEASURED_FAST_ULPS * FAST_FACTOR
RB = 64                     # rows per workgroup of head.hip
SENTINEL = -777             # pre-fill of integer outputs (no NaN there)
TINY = 2.0 ** -126          # float32's smallest normal number: what an exp that underflows may lose, per term

# ------------------------------------------------------------------ the shape lists of the GPU tests
EMBED_FWD_D = (64, 128, 50)                         # vector path, vector path, any-width path
EMBED_T, EMBED_B = 7, (1, 5, 37)
# positional sum: (dtype, d) -> (launch form, RG = batch groups per workgroup); U = 8 rows in flight per group
POS_FORMS = {(F32, 64): ("v16", 32), (BF, 128): ("v16", 32), (F32, 128): ("v32", 8), (BF, 256): ("v32", 8),
             (F32, 256): ("v64", 4), (BF, 512): ("v64", 4), (F32, 50): ("any", 4), (F32, 512): ("any", 4),
             (BF, 1024): ("any", 4)}
POS_T, POS_U = 3, 8
SAMPLED_D, SAMPLED_M = (50, 64, 200), (1, 4, 5, 259)
HEAD_D = (64, 128, 256)
HEAD_M = (1, 63, 64, 65, 64 * 3 + 17, 64 * 257 + 5)
BCE_M = (1, 255, 256, 257, 65536 + 300)
CE_R, CE_V1 = (1, 5), (7, 256, 257, 1000, 16384 + 77)
VCE_D, VCE_R, VCE_V1 = (64, 96, 256), (37, 130), (200, 20000, 70001)
ROWS_N, ROWS_D = (1, 1023, 1024, 1025, 2500), (64, 128)
CAND_D, CAND_B, CAND_C = (50, 64, 300), (1, 3), (1, 101)


def pos_batches(rg):
    return (1, rg - 1, rg * POS_U + 3)


def gen_for(dev, *key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator(device=dev).manual_seed(seed)


def rn(gen, dev, *shape, s=1.0, dt=F32):
    return (torch.randn(*shape, generator=gen, device=dev, dtype=F32) * s).to(dt)


def bound_out(dt, r, A, K):
    """the bound of an output stored as dt (bf16: its own rounding on top)"""
    return bound_bf16(r, A, K) if dt == BF else bound_f32(A, K)


def exact(hip, ref):
    return 0.0 if torch.equal(hip, ref.to(hip.dtype)) else math.inf


class Guarded:
    """An output pre-filled with NaN (integers: SENTINEL), followed by GUARD guard rows, optionally with a row pitch
    wider than the row and an element offset of the base.  .t is what the kernel gets (rows x cols view)."""

    def __init__(self, rows, cols=None, dt=F32, dev="cuda", pitch=None, offset=0):
        self.rows, self.cols, self.fill = rows, cols, (math.nan if dt.is_floating_point else SENTINEL)
        p = (pitch or cols) if cols else 1
        self.flat = torch.full(((rows + GUARD) * p + offset,), self.fill, dtype=dt, device=dev)
        body = self.flat[offset:]
        self.full = body.view(rows + GUARD, p) if cols else body
        self.t = self.full[:rows, :cols] if cols else self.full[:rows]

    def _is_fill(self, t):
        return torch.isnan(t) if math.isnan(self.fill) else t == self.fill

    def check(self, name, written=None, pads_zero_ok=False):
        """rows below `written` (default all) hold no fill value; guard rows, rows past `written`, pad columns and
        the offset elements are untouched (pads_zero_ok: a written row's pad columns may instead hold zeros)"""
        n = self.rows if written is None else written
        body = self.full[:n, :self.cols] if self.cols else self.full[:n]
        assert not self._is_fill(body).any(), f"{name}: elements below the row count left unwritten"
        assert self._is_fill(self.full[n:]).all(), f"{name}: store past the row count"
        if self.cols:
            pad = self.full[:n, self.cols:]
            assert (self._is_fill(pad) | ((pad == 0) & pads_zero_ok)).all(), f"{name}: store into the pad columns"
        assert self._is_fill(self.flat[:self.flat.numel() - self.full.numel()]).all(), f"{name}: store before the base"

    def untouched(self, name):
        assert self._is_fill(self.flat).all(), f"{name}: written by a call that must leave it alone"


class Worst(dict):
    """the worst err / bound per kernel and tensor over the cases of a module"""

    def report(self, kernel, key, res):
        print(f"\n{kernel} {key} err/bound:", {k: round(v, 4) for k, v in res.items()})
        for k, v in res.items():
            self[(kernel, k)] = max(self.get((kernel, k), 0.0), v)
        bad = {k: v for k, v in res.items() if not v <= 1.0 and not k.endswith(".ulps")}
        assert not bad, (kernel, key, bad)

    def dump(self):
        print("\nworst err / bound per kernel and output tensor")
        for (kernel, k), v in sorted(self.items()):
            print(f"{kernel:20s} {k:16s} {v:.4f}")


def vce_cross(inp, logits, lse_a, lse_b, dl_a, dl_b, count, dloss, rows=None):
    """two kernels of the same operation: apart by at most the sum of their two bounds"""
    x, Ax = logits
    lab, d = ce_live(inp, rows), inp["d"]
    live = (lab != 0).double()
    n = inp["R"] if rows is None else rows
    b_lse = vce_lse_bound(x, Ax, torch.logsumexp(x, 1), d) * live
    sc = abs(dloss / count)
    b = sum(vce_grad_bound(x, Ax, D(l), lab, ref_ce_grad(x, lab, D(l), count, dloss), d, sc) for l in (lse_a, lse_b))
    return {"lse": ratio(lse_a, D(lse_b), 2 * b_lse), "dlogits": ratio(dl_a[:n], D(dl_b[:n]), b[:n])}


# ====================================================================== embedding.hip
def rand_mask(gen, dev, rows, d, p):
    return torch.rand(rows, d, generator=gen, device=dev) >= p if p > 0 else torch.ones(rows, d, dtype=torch.bool,
                                                                                         device=dev)


def embed_inputs(dt, d, B, T, dev, V=23, seed=0):
    g = gen_for(dev, 11, d, B, T, seed)
    ids = torch.randint(1, V, (B * T,), generator=g, device=dev)
    ids[::5] = 0                                            # padding, the first row included
    return {"ids": ids, "T": T, "table": rn(g, dev, V, d, s=0.3, dt=dt), "ptab": rn(g, dev, T, d, s=0.5, dt=dt),
            "scale": float(np.float32(math.sqrt(d))), "dx": rn(g, dev, B * T, d, s=0.1, dt=dt),
            "dpos0": rn(g, dev, T, d, s=0.2), "dtable0": rn(g, dev, V, d, s=0.2), "V": V, "d": d}


def ref_embed_fwd(mode, ids, T, table, ptab, scale, mk):
    """mode 0 (SAS): ((E[ids] scale + P[t]) drop) [ids != 0];  mode 1 (BERT): (E[ids] + P[t]) drop;  mk = keep/(1-p)"""
    e = F.embedding(ids, D(table), padding_idx=0)
    p = D(ptab)[torch.arange(ids.numel(), device=ids.device) % T]
    if mode == 0:
        return (e * scale + p) * mk * (ids != 0).double()[:, None]
    return (e + p) * mk


def check_embed_fwd(mode, inp, keep, p, out):
    mk = D(keep) * kmul(p)
    r = ref_embed_fwd(mode, inp["ids"], inp["T"], inp["table"], inp["ptab"], inp["scale"], mk)
    A = ref_embed_fwd(mode, inp["ids"], inp["T"], inp["table"].abs(), inp["ptab"].abs(), inp["scale"], mk)
    # K = 6: one fma (or add), the multiplier's own two roundings, two multiplies, the padding select
    return {"x": ratio(out, r, bound_out(out.dtype, r, A, 6))}


def emu_embed_fwd(mode, inp, keep, p, mut=None):
    ids, T = inp["ids"], inp["T"]
    mk = keep.float() * np.float32(kmul(p))
    e, pt = inp["table"].float()[ids], inp["ptab"].float()[torch.arange(ids.numel()) % T]
    x = (e * np.float32(inp["scale"]) + pt if mode == 0 else e + pt) * mk
    if mode == 0 and mut != "nozero":
        x = x * (ids != 0).float()[:, None]
    return x.to(inp["table"].dtype)


def ref_embed_bwd(mode, inp, dx, mk):
    """(dtable, dpos) by autograd through the float64 forward (padding_idx=0: row 0 takes no gradient)"""
    V, T, d = inp["V"], inp["T"], inp["d"]
    tab = torch.zeros(V, d, dtype=torch.float64, device=dx.device, requires_grad=True)
    pt = torch.zeros(T, d, dtype=torch.float64, device=dx.device, requires_grad=True)
    ref_embed_fwd(mode, inp["ids"], T, tab, pt, inp["scale"] if mode == 0 else 1.0, mk).backward(D(dx))
    return tab.grad, pt.grad


def check_embed_bwd(mode, inp, keep, p, dtable=None, dpos=None, accumulate=False):
    """dtable: atomics on top of dtable0; dpos: the per-position sum over the batch (+ dpos0 when accumulating)"""
    mk = D(keep) * kmul(p)
    rt, rp = ref_embed_bwd(mode, inp, inp["dx"], mk)
    At, Ap = ref_embed_bwd(mode, inp, inp["dx"].abs(), mk)
    res = {}
    if dtable is not None:
        # K per table row: its contributions (rows of the batch with that id) + 3 to form one (scale, two for the
        # multiplier) + 1 for the value already there
        n = torch.bincount(inp["ids"], minlength=inp["V"]).double()[:, None] + 4
        t0 = D(inp["dtable0"])
        res["dtable"] = ratio(dtable, t0 + rt, bound_f32(t0.abs() + At, n))
        res["dtable.row0"] = exact(dtable[0], inp["dtable0"][0])
    if dpos is not None:
        p0 = D(inp["dpos0"]) if accumulate else 0.0
        # K: nb batch rows summed (in groups, then the groups: never a longer path than in order) + 2 for the
        # multiplier + 1 for the accumulate
        nb = inp["ids"].numel() // inp["T"]
        res["dpos"] = ratio(dpos, p0 + rp, bound_f32(Ap + (p0.abs() if accumulate else 0.0), nb + 3))
    return res


def emu_embed_bwd(mode, inp, keep, p, accumulate=False, mut=None):
    ids, T, d = inp["ids"], inp["T"], inp["d"]
    rows = ids.numel()
    mk = keep.float() * np.float32(kmul(p))
    dx = inp["dx"].float()
    g = dx * (np.float32(inp["scale"]) if mode == 0 and mut != "noscale" else np.float32(1.0)) * mk
    live = torch.ones(rows, dtype=torch.bool) if mut == "row0" else ids != 0
    dtable = inp["dtable0"].clone().index_add_(0, ids[live], g[live])
    mkp = mk.roll(1, 0) if mut == "maskrow" else mk           # the mask of the row before: index r*d + c of r - 1
    gp = dx * mkp * ((ids != 0).float()[:, None] if mode == 0 else 1.0)
    gp = gp.view(rows // T, T, d)
    if mut == "lastbatch":
        gp = gp[:-1]
    s = gp.sum(0)
    return dtable, (inp["dpos0"] + s if accumulate else s)


def zipf_ids(gen, dev, rows, V):
    """ids with P(v) ~ 1/v over 1..V-1 and ~10 % padding: the hottest row takes hundreds of contributions"""
    w = 1.0 / torch.arange(1, V, device=dev, dtype=torch.float64)
    ids = torch.multinomial(w, rows, replacement=True, generator=gen) + 1
    ids[::10] = 0
    return ids


# ---------------------------------------------------------------------- sampled logits
def sampled_inputs(dt, d, M, dev, V=19):
    g = gen_for(dev, 13, d, M)
    pos, neg = torch.randint(0, V, (M,), generator=g, device=dev), torch.randint(0, V, (M,), generator=g, device=dev)
    if M >= 4:
        pos[1], neg[2], pos[3], neg[3] = 0, 0, neg[0], neg[0]        # padding ids; one row with pos == neg
    dpl, dnl = rn(g, dev, M, s=0.3), rn(g, dev, M, s=0.3)
    dpl[::4] = 0                                                      # dpl == 0 rows (skipped atomics)
    return {"f": rn(g, dev, M, d, dt=dt), "E": rn(g, dev, V, d, s=0.3, dt=dt), "pos": pos, "neg": neg, "dpl": dpl,
            "dnl": dnl, "df0": rn(g, dev, M, d, s=0.5, dt=dt), "dE0": rn(g, dev, V, d, s=0.2), "V": V, "d": d, "M": M}


def k_lanes(d):
    """a lane-strided dot product of length d over 64 lanes: ceil(d/64) multiply-adds, then 6 butterfly steps"""
    return -(-d // 64) + 6


def check_sampled_fwd(inp, pl, nl):
    f, E = D(inp["f"]), D(inp["E"])
    res = {}
    for n, ids, hip in (("pl", inp["pos"], pl), ("nl", inp["neg"], nl)):
        e = F.embedding(ids, E)
        res[n] = ratio(hip, (f * e).sum(-1), bound_f32((f * e).abs().sum(-1), k_lanes(inp["d"])))
    return res


def emu_sampled_fwd(inp, mut=None):
    d = inp["d"]
    n = d - d % 64 if mut == "tail" else d
    f = inp["f"].float()[:, :n]
    return ((f * inp["E"].float()[inp["pos"]][:, :n]).sum(-1), (f * inp["E"].float()[inp["neg"]][:, :n]).sum(-1))


def check_sampled_bwd(inp, df, dE=None, accumulate=False):
    f, E = D(inp["f"]), D(inp["E"])
    gp, gn = D(inp["dpl"])[:, None], D(inp["dnl"])[:, None]
    ep, en = F.embedding(inp["pos"], E), F.embedding(inp["neg"], E)
    d0 = D(inp["df0"]) if accumulate else torch.zeros_like(f)
    r, A = gp * ep + gn * en + d0, (gp * ep).abs() + (gn * en).abs() + d0.abs()
    res = {"df": ratio(df, r, bound_out(df.dtype, r, A, 4))}       # K = 4: two products, two adds
    if dE is not None:
        V = inp["V"]
        e0 = D(inp["dE0"])
        rt, At, n = e0.clone(), e0.abs(), torch.zeros(V, dtype=torch.float64, device=f.device)
        for ids, g in ((inp["pos"], gp), (inp["neg"], gn)):
            live = (ids != 0).double()[:, None]
            rt.index_add_(0, ids, g * f * live)
            At.index_add_(0, ids, (g * f).abs() * live)
            n.index_add_(0, ids, live[:, 0])
        # K per table row: its contributions + 1 product each + the value already there
        res["dE"] = ratio(dE, rt, bound_f32(At, n[:, None] + 2))
        res["dE.row0"] = exact(dE[0], inp["dE0"][0])
    return res


def emu_sampled_bwd(inp, accumulate=False):
    f, E = inp["f"].float(), inp["E"].float()
    gp, gn = inp["dpl"][:, None], inp["dnl"][:, None]
    df = gp * E[inp["pos"]] + gn * E[inp["neg"]]
    if accumulate:
        df = df + inp["df0"].float()
    dE = inp["dE0"].clone()
    for ids, g in ((inp["pos"], gp), (inp["neg"], gn)):
        dE.index_add_(0, ids[ids != 0], (g * f)[ids != 0])
    return df.to(inp["f"].dtype), dE


# ====================================================================== head.hip
def head_np(d):
    """rows each thread handles: 8 columns per thread, 256 threads, 64 rows per workgroup"""
    return RB // (256 // (d // 8))


def head_inputs(d, M, dev, zeros=0.3, escale=1.0, V=41):
    g = gen_for(dev, 17, d, M, int(zeros * 10), int(escale))
    c = torch.arange(d, device=dev, dtype=F32)
    rows = torch.arange(M, device=dev, dtype=F32)[:, None]
    x = (rn(g, dev, M, d) * (1.0 + 0.5 * torch.sin(0.11 * rows)) + 0.4 * torch.cos(0.7 * c)).to(BF)
    pos, neg = torch.randint(1, V, (M,), generator=g, device=dev), torch.randint(0, V, (M,), generator=g, device=dev)
    pos[torch.rand(M, generator=g, device=dev) < zeros] = 0
    if zeros < 1:
        pos[0], pos[M - 1] = 0, 3                           # a padded first row (M > 1), a valid last row
    return {"M": M, "d": d, "x": x, "g": ((0.6 + 0.9 * c / d) * (1 - 2 * (c % 3 == 1).float())).contiguous(),
            "b": (0.3 * torch.cos(1.3 * c) + 0.05).contiguous(), "pos": pos, "neg": neg,
            "E": rn(g, dev, V, d, s=escale / math.sqrt(d), dt=BF), "dpl_in": rn(g, dev, M, s=0.01),
            "dnl_in": rn(g, dev, M, s=0.01)}


def blk_sum(t):
    """[M, n] -> [ceil(M/64), n]: the sum over each 64-row block"""
    M, n = t.shape
    nb = -(-M // RB)
    p = torch.zeros(nb * RB, n, dtype=t.dtype, device=t.device)
    p[:M] = t
    return p.view(nb, RB, n).sum(1)


def check_parts(res, name, part, terms, aterms, K):
    """block by block against the float64 sum over exactly that block's rows, and in total"""
    res[name + "/blk"] = ratio(part, blk_sum(terms), bound_f32(blk_sum(aterms), K))
    res[name] = ratio(D(part).sum(0), terms.sum(0), bound_f32(aterms.sum(0), K))


def check_head_fwd(inp, out):
    x, d = D(inp["x"]), inp["d"]
    g, b = D(inp["g"]), D(inp["b"])
    mu, rs = s_stats(x)
    # K as rowchain_ref: the row reduction (d) and the few operations around it
    res = {"mean": ratio(out["mean"], mu[:, 0], bound_f32(x.abs().mean(-1), d + 1)),
           "rstd": ratio(out["rstd"], rs[:, 0], bound_f32(rs[:, 0], d))}
    r = s_ln(x, g, b, mu, rs)
    res["f"] = ratio(out["f"], r, bound_bf16(r, s_ln_abs(x, g, b, rs), d))
    f = D(out["f"])                                         # the logits read the stored bf16 features
    ep, en = F.embedding(inp["pos"], D(inp["E"])), F.embedding(inp["neg"], D(inp["E"]))
    # K: 8 products per thread, log2(d/8) butterfly steps
    K = 8 + int(math.log2(d // 8))
    res["pl"] = ratio(out["pl"], (f * ep).sum(-1), bound_f32((f * ep).abs().sum(-1), K))
    res["nl"] = ratio(out["nl"], (f * en).sum(-1), bound_f32((f * en).abs().sum(-1), K))
    pl, nl = D(out["pl"]), D(out["nl"])
    valid = (inp["pos"] != 0).double()
    t = torch.stack([softplus(-pl) * valid, softplus(nl) * valid], 1)
    # K: softplus to ~8 float32 operations, the thread's rows, 6 butterfly steps, 4 waves
    check_parts(res, "part", out["part"][:, :2], t, t + TINY / U24 * valid[:, None], 8 + head_np(d) + 6 + 4)
    res["part.count"] = exact(out["part"][:, 2], blk_sum(valid[:, None])[:, 0])
    return res


def ref_head_stats(part, divisor):
    """out[0..3] = {sum of the BCE terms, valid count, pos mean + neg mean, neg sum} from the block partials"""
    sp, sn, c = D(part).sum(0)
    cc = c if divisor is None else divisor
    return torch.stack([sp + sn, c, sp / cc + sn / cc, sn]), torch.stack([sp + sn, c * 0, (sp + sn) / abs(cc), sn])


def check_head_stats(part, divisor, out):
    """staged: from the partials the forward stored.  K: ceil(nblk/256) strided adds, an 8-level tree, 3 to finish.
    No valid row and no divisor: out[2] = 0 / 0 = NaN, the reference's mean over an empty selection."""
    r, A = ref_head_stats(part, divisor)
    K = -(-part.shape[0] // 256) + 8 + 3
    res = {"out.count": exact(out[1], r[1])}
    if float(r[1]) == 0 and divisor is None:
        res["out"] = ratio(out[[0, 3]], r[[0, 3]], bound_f32(A[[0, 3]], K))
        res["out.mean"] = 0.0 if bool(torch.isnan(out[2])) else math.inf
    else:
        res["out"] = ratio(out[[0, 2, 3]], r[[0, 2, 3]], bound_f32(A[[0, 2, 3]], K))
    return res


def check_head_bwd(inp, fw, out, divisor=None, grads_in=False):
    """fw: what rs_sas_head_fwd stored (pl, nl, mean, rstd, part); out: dx, lnpart (+ dpl, dnl, out)"""
    d = inp["d"]
    x, g = D(inp["x"]), D(inp["g"])
    res = {}
    if grads_in:
        dpl, dnl = D(inp["dpl_in"]), D(inp["dnl_in"])
    else:
        res.update(check_head_stats(fw["part"], divisor, out["out"]))
        pl, nl = D(fw["pl"]), D(fw["nl"])
        valid = (inp["pos"] != 0).double()
        c = float(D(fw["part"])[:, 2].sum()) if divisor is None else divisor
        sc = 1.0 / c if c else 0.0                          # no valid row: every gradient is zero
        # the sigmoid in float32: |error| <= (8 + |z|) 2^-24 in absolute terms, then the scale's rounding (K = 8)
        res["dpl"] = ratio(out["dpl"], (torch.sigmoid(pl) - 1) * sc * valid, bound_f32(sc * (1 + pl.abs()) * valid, 8))
        res["dnl"] = ratio(out["dnl"], torch.sigmoid(nl) * sc * valid, bound_f32(sc * (1 + nl.abs()) * valid, 8))
        dpl, dnl = D(out["dpl"]), D(out["dnl"])
    ep, en = F.embedding(inp["pos"], D(inp["E"])), F.embedding(inp["neg"], D(inp["E"]))
    df = dpl[:, None] * ep + dnl[:, None] * en
    adf = (dpl[:, None] * ep).abs() + (dnl[:, None] * en).abs()
    mu, rs = D(fw["mean"])[:, None], D(fw["rstd"])[:, None]
    r, tg, tb = s_ln_bwd(df, x, g, mu, rs)
    A, ut = s_ln_bwd_abs(adf, x, g, mu, rs)
    res["dx"] = ratio(out["dx"], r, bound_bf16(r, A, d + 4) + TINY)     # TINY: gradients that underflow
    # K: 3 to form df, 2 more for its term, the thread's rows, the workgroup's 256/(d/8) row groups in LDS order;
    # the gamma term carries u = (x - mean) rstd: 2 more
    K = 3 + 2 + head_np(d) + 256 // (d // 8)
    check_parts(res, "lnpart.g", out["lnpart"][:, 0], tg, adf * ut, K + 2)
    check_parts(res, "lnpart.b", out["lnpart"][:, 1], tb, adf, K)
    return res


def _stats32(x):
    mu = x.mean(-1, keepdim=True)
    return mu, 1.0 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + np.float32(EPS))


def emu_head_fwd(inp):
    x = inp["x"].float()
    mu, rs = _stats32(x)
    f = rb((x - mu) * rs * inp["g"] + inp["b"])             # rounded before the dot products
    pl, nl = (f * inp["E"].float()[inp["pos"]]).sum(-1), (f * inp["E"].float()[inp["neg"]]).sum(-1)
    valid = (inp["pos"] != 0).float()
    part = blk_sum(torch.stack([F.softplus(-pl) * valid, F.softplus(nl) * valid, valid], 1))
    return {"f": f.bfloat16(), "mean": mu[:, 0].clone(), "rstd": rs[:, 0].clone(), "pl": pl, "nl": nl, "part": part}


def emu_head_stats(part, divisor, mut=None):
    p = part[1:] if mut == "statblk" else part
    sp, sn, c = p.sum(0)
    cc = c if divisor is None or mut == "nodivisor" else np.float32(divisor)
    return torch.stack([sp + sn, c, sp / cc + sn / cc, sn])


def emu_head_bwd(inp, fw, divisor=None, grads_in=False, mut=None):
    x, E = inp["x"].float(), inp["E"].float()
    out = {}
    if grads_in:
        dpl, dnl = inp["dpl_in"], inp["dnl_in"]
    else:
        out["out"] = emu_head_stats(fw["part"], divisor, mut)
        valid = (inp["pos"] != 0).float()
        c = float(fw["part"][:, 2].sum()) if divisor is None or mut == "nodivisor" else divisor
        sc = np.float32(1.0) / np.float32(c) if c else np.float32(0.0)
        dpl, dnl = (torch.sigmoid(fw["pl"]) - 1) * sc * valid, torch.sigmoid(fw["nl"]) * sc * valid
        out["dpl"], out["dnl"] = dpl, dnl
    df = dpl[:, None] * E[inp["pos"]] + dnl[:, None] * E[inp["neg"]]
    mu, rs = fw["mean"][:, None], fw["rstd"][:, None]
    u = x - mu
    gq = df * inp["g"]
    dx = rs * (gq - gq.mean(-1, keepdim=True)) - rs ** 3 * (gq * u).mean(-1, keepdim=True) * u
    lnpart = torch.stack([blk_sum(df * (u * rs)), blk_sum(df)], 1).contiguous()
    if mut == "lnblk":
        lnpart[-1] = 0
    out.update(dx=dx.bfloat16(), lnpart=lnpart)
    return out


# ====================================================================== loss.hip: BCE
def bce_inputs(M, dev, big=False):
    g = gen_for(dev, 19, M, int(big))
    pl, nl = rn(g, dev, M, s=2.0), rn(g, dev, M, s=2.0)
    if big:                                                 # |logit| past 100, every sign combination
        pl, nl = pl * 60 + 110 * torch.sign(pl), nl * 60 + 110 * torch.sign(nl)
    pos = torch.randint(1, 50, (M,), generator=g, device=dev)
    pos[torch.rand(M, generator=g, device=dev) < 0.3] = 0
    pos[0] = 3
    if M > 1:
        pos[M - 1] = 0
    return {"M": M, "pl": pl, "nl": nl, "pos": pos}


def k_bce(M):
    """softplus to ~8 operations, the grid-stride trips, 6 butterfly steps, 4 waves, the finish kernel's serial sum
    over the workgroups, 3 to finish"""
    return 8 + -(-M // 65536) + 6 + 4 + min(256, -(-M // 256)) + 3


def check_bce_fwd(inp, out, count_override=None):
    v = inp["pos"] != 0
    pl, nl = D(inp["pl"])[v], D(inp["nl"])[v]
    sp = F.binary_cross_entropy_with_logits(pl, torch.ones_like(pl), reduction="sum")
    sn = F.binary_cross_entropy_with_logits(nl, torch.zeros_like(nl), reduction="sum")
    c = float(v.sum())
    cc = c if count_override is None else count_override
    mean = (sp + sn) / cc if cc else torch.tensor(math.nan, dtype=torch.float64, device=sp.device)
    K = k_bce(inp["M"])
    u = TINY * c                                            # terms that underflow in float32
    res = {"sum": ratio(out[0], sp + sn, bound_f32(sp + sn, K) + 2 * u), "neg": ratio(out[3], sn, bound_f32(sn, K) + u),
           "count": exact(out[1], torch.tensor(c, device=out.device))}
    if cc:
        res["mean"] = ratio(out[2], mean, bound_f32(mean.abs(), K))
    else:
        res["mean"] = 0.0 if bool(torch.isnan(out[2])) else math.inf       # 0 / 0: the mean of no element
    return res


def emu_bce_fwd(inp, count_override=None, mut=None):
    v = (inp["pos"] != 0).float()
    sp = (F.softplus(-inp["pl"]) * v).sum()
    sn = (F.softplus(-inp["nl"] if mut == "negsign" else inp["nl"]) * v).sum()
    c = v.sum()
    cc = np.float32(count_override) if count_override is not None and mut != "nooverride" else c
    if mut == "padcount":
        cc = np.float32(inp["M"])
    return torch.stack([sp + sn, c, sp / cc + sn / cc, sn])


def check_bce_bwd(inp, count, dloss, dpl, dnl):
    """dpl, dnl = dloss (sigmoid(z) - y) / count on valid rows; the float64 gradient by autograd of the torch loss"""
    v = (inp["pos"] != 0).double()
    pl, nl = D(inp["pl"]).requires_grad_(), D(inp["nl"]).requires_grad_()
    loss = (F.binary_cross_entropy_with_logits(pl, torch.ones_like(pl), weight=v, reduction="sum") +
            F.binary_cross_entropy_with_logits(nl, torch.zeros_like(nl), weight=v, reduction="sum")) / count
    gp, gn = torch.autograd.grad(loss * dloss, (pl, nl))
    s = abs(dloss) / count
    # K = 10: the sigmoid's |error| <= (8 + |z|) 2^-24 as in the head, the scale's division and product
    return {"dpl": ratio(dpl, gp, bound_f32(s * (1 + pl.detach().abs()) * v, 10)),
            "dnl": ratio(dnl, gn, bound_f32(s * (1 + nl.detach().abs()) * v, 10))}


def emu_bce_bwd(inp, count, dloss, mut=None):
    v = (inp["pos"] != 0).float()
    s = np.float32(1.0 if mut == "nodloss" else dloss) / np.float32(count)
    return (torch.sigmoid(inp["pl"]) - 1) * s * v, torch.sigmoid(inp["nl"]) * s * v


# ====================================================================== loss.hip: cross entropy over stored logits
def ce_inputs(R, V1, dev, ldl=None, span=False):
    g = gen_for(dev, 23, R, V1, int(span))
    ldl = ldl or V1
    full = torch.full((R, ldl), math.nan, device=dev)
    full[:, :V1] = rn(g, dev, R, V1, s=2.0)
    if span:                                                # one row whose logits span +-150
        full[R - 1, :V1] = torch.linspace(-150, 150, V1, device=dev)[torch.randperm(V1, generator=g, device=dev)]
    lab = torch.randint(1, V1, (R,), generator=g, device=dev)
    if R > 1:
        lab[1] = 0
    return {"R": R, "V1": V1, "logits": full[:, :V1], "labels": lab}


def ce_live(inp, rows):
    lab = inp["labels"].clone()
    if rows is not None:
        lab[rows:] = 0
    return lab


def check_ce_fwd(inp, lse, out, count_override=None, rows=None):
    x, lab, V1 = D(inp["logits"]), ce_live(inp, rows), inp["V1"]
    live = lab != 0
    r = torch.logsumexp(x, 1) * live
    # K: every online step is ~4 operations (difference, exp, rescale, add); a thread takes ceil(V1/256) of them, the
    # block tree 8 more; + log and the last add.  A: the relative error of the sum moves lse by that much in
    # absolute terms (the sum is >= 1), the last add by 2^-24 |lse|
    K = 4 * (-(-V1 // 256) + 8) + 2
    b_lse = bound_f32((1 + r.abs()) * live, K)
    res = {"lse": ratio(lse, r, b_lse)}
    S = F.cross_entropy(x, lab, ignore_index=0, reduction="sum")
    tgt = x.gather(1, lab[:, None])[:, 0]
    # the row terms lse - x[label], then ceil(R/256) strided adds, 6 butterfly steps, 4 waves
    b_S = b_lse.sum() + bound_f32(((r.abs() + tgt.abs()) * live).sum(), 1 + -(-inp["R"] // 256) + 6 + 4)
    c = float(live.sum())
    cc = c if count_override is None else count_override
    res["sum"] = ratio(out[0], S, b_S)
    res["count"] = exact(out[1], torch.tensor(c, device=out.device))
    res["mean"] = ratio(out[2], S / cc, b_S / cc + bound_f32(S.abs() / cc, 1)) if cc else 0.0
    return res


def emu_ce_fwd(inp, count_override=None, rows=None, mut=None):
    x, lab = inp["logits"], ce_live(inp, rows)
    live = (lab != 0).float()
    lse = (torch.log(torch.exp(x).sum(1)) if mut == "nomax" else torch.logsumexp(x, 1)) * live
    S = ((lse - x.gather(1, lab[:, None])[:, 0]) * live).sum()
    c = live.sum()
    return lse, torch.stack([S, c, S / (c if count_override is None else np.float32(count_override))])


def ref_ce_grad(x, lab, lse, count, dloss):
    """dloss (softmax - onehot) / count on labelled rows from a given row log-sum-exp"""
    g = torch.exp(x - lse[:, None])
    g[torch.arange(x.shape[0], device=x.device), lab] -= 1.0
    return g * (lab != 0).double()[:, None] * (dloss / count)


def check_ce_bwd(inp, lse, count, dloss, dl, rows=None):
    """staged: from the row log-sum-exp the forward stored.  K = 6: difference, exp (2), one-hot, scale (2); the
    difference's rounding moves exp by |x - lse| 2^-24 in relative terms"""
    x, lab = D(inp["logits"]), ce_live(inp, rows)
    L = D(lse)
    r = ref_ce_grad(x, lab, L, count, dloss)
    p = torch.exp(x - L[:, None])
    live = (lab != 0).double()[:, None]
    A = (p * (1 + (x - L[:, None]).abs()) + F.one_hot(lab, inp["V1"])) * live * abs(dloss / count)
    n = inp["R"] if rows is None else rows
    return {"dlogits": ratio(dl[:n], r[:n], bound_out(dl.dtype, r[:n], A[:n], 6) + TINY)}


def emu_ce_bwd(inp, lse, count, dloss, dt=F32, mut=None):
    x, lab = inp["logits"], inp["labels"]
    g = torch.exp(x - lse[:, None])
    g[torch.arange(x.shape[0]), (lab + 1) % inp["V1"] if mut == "onehot+1" else lab] -= 1.0
    if mut != "lab0grad":
        g = g * (lab != 0).float()[:, None]
    return (g * (np.float32(1.0 if mut == "nodloss" else dloss) / np.float32(count))).to(dt)


# ====================================================================== vocab_ce.hip
def vce_inputs(d, R, V1, dev, bias=True):
    g = gen_for(dev, 29, d, R, V1)
    lab = torch.randint(1, V1, (R,), generator=g, device=dev)
    lab[::7] = 0
    lab[R - 1] = V1 - 1                                     # a label in the last, ragged tile
    return {"d": d, "R": R, "V1": V1, "h": rn(g, dev, R, d, dt=BF), "E": rn(g, dev, V1, d, s=0.6 / math.sqrt(d), dt=BF),
            "bias": rn(g, dev, V1, s=0.3) if bias else None, "labels": lab}


def vce_logits(inp):
    h, E = D(inp["h"]), D(inp["E"])
    b = D(inp["bias"]) if inp["bias"] is not None else 0.0
    return h @ E.t() + b, h.abs() @ E.abs().t() + (b.abs() if inp["bias"] is not None else 0.0)


def vce_lse_bound(x, Ax, lse, d):
    """the logits' float32 GEMM error (K = d + 1 with the bias) moves lse by at most its softmax-weighted mean; the
    fast exp / log of the tile pairs and their folds by FAST_ULPS 2^-24 max(|lse|, 1)"""
    p = torch.exp(x - lse[:, None])
    return bound_f32((p * Ax).sum(1), d + 1) + FAST_ULPS * U24 * lse.abs().clamp(min=1.0)


def check_vce_fwd(inp, lse, out, count_override=None, rows=None, logits=None):
    x, Ax = logits if logits is not None else vce_logits(inp)
    lab, d = ce_live(inp, rows), inp["d"]
    live = (lab != 0).double()
    r = torch.logsumexp(x, 1)
    b_lse = vce_lse_bound(x, Ax, r, d)
    res = {"lse": ratio(lse, r * live, b_lse * live)}
    err = (D(lse) - r * live).abs() / (U24 * r.abs().clamp(min=1.0))
    res["lse.ulps"] = float(err.max())                      # the measurement behind MEASURED_FAST_ULPS (no bar)
    S = F.cross_entropy(x, lab, ignore_index=0, reduction="sum")
    tgt, Atgt = x.gather(1, lab[:, None])[:, 0], Ax.gather(1, lab[:, None])[:, 0]
    b_S = ((b_lse + bound_f32(Atgt, d + 1)) * live).sum() + \
        bound_f32(((r.abs() + tgt.abs()) * live).sum(), 1 + -(-inp["R"] // 256) + 6 + 4)
    c = float(live.sum())
    cc = c if count_override is None else count_override
    res["sum"] = ratio(out[0], S, b_S)
    res["count"] = exact(out[1], torch.tensor(c, device=out.device))
    res["mean"] = ratio(out[2], S / cc, b_S / cc + bound_f32(S.abs() / cc, 1))
    return res


def vce_grad_bound(x, Ax, L, lab, r, d, sc):
    """bf16 output; K = d + 4: the logit's reduction and bias, difference, one-hot, scale (2); the logit's error moves
    exp by that much in relative terms, the fast exp by FAST_ULPS 2^-24 max(|x - lse|, 1)"""
    z = x - L[:, None]
    p = torch.exp(z)
    live = (lab != 0).double()[:, None]
    A = (p * (Ax + 1) + F.one_hot(lab, x.shape[1])) * live * sc
    return bound_bf16(r, A, d + 4) + p * live * sc * FAST_ULPS * U24 * z.abs().clamp(min=1.0) + TINY


def check_vce_bwd(inp, lse, count, dloss, dl, rows=None, logits=None):
    """staged: from the row log-sum-exp the forward stored"""
    x, Ax = logits if logits is not None else vce_logits(inp)
    lab, L = ce_live(inp, rows), D(lse)
    r = ref_ce_grad(x, lab, L, count, dloss)
    n = inp["R"] if rows is None else rows
    b = vce_grad_bound(x, Ax, L, lab, r, inp["d"], abs(dloss / count))
    return {"dlogits": ratio(dl[:n], r[:n], b[:n])}


def emu_vce_fwd(inp, count_override=None, rows=None, mut=None):
    """the logits in float32, per 128-column tile the (max, sum) pair, the pairs folded; mut 'tile' drops one pair"""
    x = inp["h"].float() @ inp["E"].float().t()
    if inp["bias"] is not None:
        x = x + inp["bias"]
    lab = ce_live(inp, rows)
    live = (lab != 0).float()
    V1 = inp["V1"]
    nt = -(-V1 // 128)
    xp = torch.full((x.shape[0], nt * 128), -math.inf)
    xp[:, :V1] = x
    xt = xp.view(-1, nt, 128)
    mx = xt.max(-1).values
    sm = torch.exp(xt - mx[..., None]).sum(-1)
    if mut == "tile":
        mx, sm = mx[:, :-1], sm[:, :-1]
    m = mx.max(-1).values
    lse = (m + torch.log((sm * torch.exp(mx - m[:, None])).sum(-1))) * live
    S = ((lse - x.gather(1, lab[:, None])[:, 0]) * live).sum()
    c = live.sum()
    return lse, torch.stack([S, c, S / (c if count_override is None else np.float32(count_override))]), x


def emu_vce_bwd(inp, x, lse, count, dloss, rows=None):
    lab = ce_live(inp, rows)
    g = torch.exp(x - lse[:, None])
    g[torch.arange(x.shape[0]), lab] -= 1.0
    return (g * (lab != 0).float()[:, None] * (np.float32(dloss) / np.float32(count))).bfloat16()


# ====================================================================== rows.hip
def ref_compact(labels, cap):
    """(idx, rank, count) of rs_compact_rows"""
    n = labels.numel()
    rows = torch.nonzero(labels != 0)[:, 0]
    cnt = min(rows.numel(), cap)
    idx = torch.full((cap,), -1, dtype=torch.int32, device=labels.device)
    idx[:cnt] = rows[:cnt].int()
    rank = torch.full((n,), -1, dtype=torch.int32, device=labels.device)
    rank[rows[:cnt]] = torch.arange(cnt, dtype=torch.int32, device=labels.device)
    return idx, rank, cnt


def ref_gather(src, labels, idx, cnt, cap):
    dst = torch.zeros(cap, src.shape[1], dtype=src.dtype, device=src.device)
    lab = torch.zeros(cap, dtype=torch.int64, device=src.device)
    dst[:cnt], lab[:cnt] = src[idx[:cnt].long()], labels[idx[:cnt].long()]
    return dst, lab


def ref_scatter(src, rank):
    dst = src[rank.clamp(min=0).long()].clone()
    dst[rank < 0] = 0
    return dst


def cand_inputs(dt, d, B, C_, dev, V=37, bias=True):
    g = gen_for(dev, 31, d, B, C_)
    ldh = d + 8
    return {"d": d, "V": V, "h": rn(g, dev, B, ldh, dt=dt)[:, :d], "E": rn(g, dev, V, d, s=0.3, dt=dt),
            "bias": rn(g, dev, V, s=0.3) if bias else None,
            "cand": torch.randint(0, V, (B, C_), generator=g, device=dev)}


def check_cand(inp, out, cand=None):
    """K: the lane-strided fma chain and butterfly, + the bias"""
    cand = inp["cand"] if cand is None else cand
    e = F.embedding(cand, D(inp["E"]))
    h = D(inp["h"])[:, None, :]
    b = D(inp["bias"])[cand] if inp["bias"] is not None else 0.0
    A = (h * e).abs().sum(-1) + (b.abs() if inp["bias"] is not None else 0.0)
    return {"scores": ratio(out, (h * e).sum(-1) + b, bound_f32(A, k_lanes(inp["d"]) + 1))}


def emu_cand(inp, mut=None):
    d = inp["d"]
    n = d - d % 64 if mut == "tail" else d
    s = (inp["h"].float()[:, None, :n] * inp["E"].float()[inp["cand"]][..., :n]).sum(-1)
    return s + inp["bias"][inp["cand"]] if inp["bias"] is not None else s
