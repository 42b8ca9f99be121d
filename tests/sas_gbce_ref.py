"""Float64 references for SASRec's BCE with N negatives per position / gBCE (TEST INFRASTRUCTURE ONLY).

The objective, on top of ``oracle.sas.log2feats``, for neg int64 (B, T, N):

    valid r : pos_r != 0,  n = #valid
    z_r0    = <f_r, E[pos_r]>,   z_rj = <f_r, E[neg_rj]>,  j = 1..N        E = item_emb.weight (tied)
    loss    = (1 / max(n, 1)) * sum_valid r [ beta * softplus(-z_r0) + sum_j softplus(z_rj) ]
    g_r0    = s * beta * (sigmoid(z_r0) - 1),   g_rj = s * sigmoid(z_rj),   s = dloss / max(n, 1)
    df_r    = g_r0 E[pos_r] + sum_j g_rj E[neg_rj]
    dE[v]  += sum over (r, j = 0..N) with id_rj = v, v != 0 of  g_rj f_r

The negatives are summed; a negative id 0 is the zero row (logit 0, softplus(0) in the loss, no table gradient);
nothing is masked; equal ids in a row are separate terms; an id outside [0, V] counts as 0; no valid row: loss 0.

``emu=oracle.sas.BF16Storage()`` rounds to bf16 where the HIP path stores bf16 (as tests/sas_sce_ref.py): the compact
LayerNorm output, the table's compute copy, the dh the LayerNorm backward reads.  The logits stay fp32.

Kernel level (sas_gbce.hip, rs_item_grad_weighted), on the kernels' own inputs: ``head_inputs`` draws a case,
``head_ref`` is float64, ``check_head`` holds a set of outputs to the derived bounds (rowchain_ref.bound_f32), and
``emu_head`` / ``emu_weighted`` restate the launches in float32 with bf16 storage and a `mut` switch that plants one
specific mistake.  ``sample_negs_ref`` is the host restatement of rs_sas_sample_negs' counter rule.

Bounds (every output is fp32; bf16 inputs are rounded before the reference sees them):
    logit           bound_f32(sum |f||E|, K = d)
    loss partial    bound_f32(sum over its terms of |term| + sum |f||E| (softplus is 1-Lipschitz: a logit's error
                    moves its term by at most as much), K = d + the number of terms summed)
    weight w        from the stored logit: K = 10 on s (1 + |z|) as losshead_ref.check_bce_bwd (the sigmoid's error is
                    at most (8 + |z|) 2^-24, the scale's division and products), + TINY for an exp that underflows
    dh element      bound_f32(sum_j |g_j||E[id_j]|, K = d + 2 + (1 + N))
    dtable element  bound_f32(|dtable0| + sum |w||f|, K = its number of contributions + 1)
The kernels use expf / log1pf, no fast intrinsic: no FAST_ULPS term.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import sas as osas
from rowchain_ref import bound_f32, ratio
from losshead_ref import TINY

ROWS_PER_WG = 4        # rows (waves) per workgroup of the head kernels: a loss partial covers that many rows
IDS_PER_PASS = 4       # ids per wave pass (one per 16-lane group)
MUTATIONS = ("beta_on_negs", "neg_mean", "drop_id0", "key0_grad", "g0_sign", "w_by_row", "past_count")


# ---------------------------------------------------------------- model level
def gbce_from_feats(f, E, pos, neg, beta, R):
    """f (B, T, d), E (V+1, d) the (possibly rounded) table, neg (B, T, N) -> the loss."""
    f = R.g(f)                                                       # R:G the dh the LayerNorm backward reads
    d = f.shape[-1]
    fr, tgt = f.reshape(-1, d), pos.reshape(-1)
    ng = neg.reshape(tgt.numel(), -1)
    V1 = E.shape[0]
    ng = torch.where((ng < 0) | (ng >= V1), torch.zeros_like(ng), ng)
    Eall = F.embedding(torch.arange(V1), E, padding_idx=0)           # a lookup: row 0 stays out of the gradient
    Eall = torch.cat([Eall[:1] * 0, Eall[1:]])                       # id 0 is the zero row: logit exactly 0
    z0 = (fr * Eall[tgt]).sum(-1)
    z = (fr[:, None, :] * Eall[ng]).sum(-1)                          # (M, N)
    valid = tgt != 0
    terms = beta * F.softplus(-z0) + F.softplus(z).sum(-1)
    return (terms * valid).sum() / max(int(valid.sum()), 1)


def gbce_loss(P, seq, pos, neg, beta, num_blocks, heads, p=0.0, masks=None, emu=None, l2_emb=0.0):
    R = emu or osas.Exact()
    f = osas.log2feats(P, seq, num_blocks, heads, p, masks, emu)
    neg = torch.as_tensor(neg)
    neg = neg[..., None] if neg.dim() == 2 else neg
    loss = gbce_from_feats(f, R.w(P["sas.item_emb.weight"]), torch.as_tensor(pos), neg, beta, R)
    if l2_emb:
        for t in P.values():
            loss = loss + l2_emb * torch.norm(t)
    return loss


def gbce_loss_and_grads(P, seq, pos, neg, beta, num_blocks, heads, p=0.0, masks=None, emu=None, l2_emb=0.0):
    """(loss, {name: gradient}) -- every parameter, zeros where the loss does not reach one."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    loss = gbce_loss(leaves, seq, pos, neg, beta, num_blocks, heads, p, masks, emu, l2_emb)
    loss.backward()
    return loss.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}


def torch_head(f, E, pos, neg, beta):
    """The plain-torch spelling of the head on features f (M, d): gather, BCE-with-logits sums over the valid rows."""
    tgt = pos.reshape(-1)
    rows = torch.nonzero(tgt != 0).reshape(-1)
    if rows.numel() == 0:
        return f.sum() * 0 + E.sum() * 0
    W = F.embedding(torch.arange(E.shape[0]), E, padding_idx=0)
    ng = neg.reshape(tgt.numel(), -1)[rows]
    zp = (f[rows] * W[tgt[rows]]).sum(-1)
    zn = (f[rows, None, :] * W[ng]).sum(-1)
    lp = F.binary_cross_entropy_with_logits(zp, torch.ones_like(zp), reduction="sum")
    ln = F.binary_cross_entropy_with_logits(zn, torch.zeros_like(zn), reduction="sum")
    return (beta * lp + ln) / rows.numel()


def closed_form_head(f, E, pos, neg, beta, dloss=1.0):
    """(loss, df (M, d), dE (V+1, d)) by the definition's closed-form gradients, float64; E[0] must be zero."""
    f, E = f.double(), E.double()
    tgt = pos.reshape(-1)
    ng = neg.reshape(tgt.numel(), -1)
    valid = (tgt != 0).double()
    n = max(int(valid.sum()), 1)
    ids = torch.cat([tgt[:, None], ng], 1)                            # (M, 1 + N)
    z = (f[:, None, :] * E[ids]).sum(-1)
    z = torch.where(ids == 0, torch.zeros_like(z), z)
    loss = ((beta * F.softplus(-z[:, 0]) + F.softplus(z[:, 1:]).sum(-1)) * valid).sum() / n
    s = dloss / n
    g = s * torch.sigmoid(z)
    g[:, 0] = s * beta * (torch.sigmoid(z[:, 0]) - 1.0)
    g = g * valid[:, None]
    df = (g[:, :, None] * E[ids]).sum(1)
    dE = torch.zeros_like(E).index_add_(0, ids.reshape(-1), (g[:, :, None] * f[:, None, :]).reshape(-1, f.shape[1]))
    dE[0] = 0
    return loss, df, dE


def gbce_beta_ref(n_negs, num_items, t):
    alpha = min(1.0, n_negs / (num_items - 1))
    return alpha * (t * (1.0 - 1.0 / alpha) + 1.0 / alpha)


# ---------------------------------------------------------------- the head kernels alone
def head_inputs(cap, N, d, dtype, count, V=41, seed=0, big=False, ldh=None, dense=False, beta=1.0, dloss=None):
    """One case of the head kernels on the CPU: hl [cap][ldh] (the first d columns are the rows), E [V+1][d] (row 0
    zero) in `dtype`, lab [cap], idx [cap] (None in the dense form, where lab 0 marks no row), neg [M][N] with about
    30 % id 0, a few ids > V and < 0, and V small so that duplicates and the positive among the negatives abound.
    big: logits near +-80."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * cap + 13 * N + d)
    V1 = V + 1
    M = cap if dense else cap + 7
    E = torch.randn(V1, d, generator=g)
    E[0] = 0
    hl = torch.randn(cap, ldh or d, generator=g)
    lab = torch.randint(1, V1, (cap,), generator=g)
    if big:                       # z_r0 = +-80: f along the positive's row, scaled; the negatives fall in between
        E = E / E.norm(dim=1, keepdim=True).clamp(min=1e-6) * math.sqrt(80.0)
        E[0] = 0
        sign = torch.where(torch.rand(cap, generator=g) < 0.5, -1.0, 1.0)
        hl[:, :d] = E[lab] * sign[:, None] + 0.05 * hl[:, :d]
    E, hl = E.to(dtype), hl.to(dtype)
    if dense:
        lab[torch.rand(cap, generator=g) < 0.3] = 0
        idx = None
        count = cap
    else:
        if count > 2:
            lab[1] = V1 + 2                                           # a label out of range: no row
        lab[count:] = -5                                              # rows past the count: never read
        idx = torch.randperm(M, generator=g)[:cap].to(torch.int32)
    neg = torch.randint(1, V1, (M, N), generator=g)
    u = torch.rand(M, N, generator=g)
    neg[u < 0.3] = 0
    neg[(u > 0.3) & (u < 0.33)] = V1 + 3
    neg[(u > 0.33) & (u < 0.36)] = -2
    nvalid = int(((lab[:count] > 0) & (lab[:count] < V1)).sum())
    return dict(cap=cap, N=N, d=d, dtype=dtype, count=count, V1=V1, M=M, hl=hl, E=E, lab=lab, idx=idx, neg=neg,
                beta=float(beta), divisor=float(max(nvalid, 1)), dloss=dloss, dense=dense)


def _ids(inp):
    """(count, 1 + N) ids as the kernels clamp them, and the valid rows."""
    c, V1 = inp["count"], inp["V1"]
    lab = inp["lab"][:c].clone()
    lab[(lab <= 0) | (lab >= V1)] = 0
    src = torch.arange(c) if inp["idx"] is None else inp["idx"][:c].long()
    ng = inp["neg"][src].clone()
    ng[(ng <= 0) | (ng >= V1)] = 0
    return torch.cat([lab[:, None], ng], 1), lab != 0


def head_ref(inp, z_stored=None):
    """float64 on the kernels' own inputs.  z_stored: the backward's input (the forward's fp32 logits), else the
    reference's own.  Returns z, terms, out, parts [workgroups][3], w, dh, keys and the magnitudes of the bounds."""
    c, cap, N, d = inp["count"], inp["cap"], inp["N"], inp["d"]
    hl, E = inp["hl"][:c, :d].double(), inp["E"].double()
    ids, valid = _ids(inp)
    E = E.clone()
    E[0] = 0                                   # id 0 is the zero row whatever the table holds there
    # every row against the whole (small) table once, then gathered by id: no (rows, 1 + N, d) tensor
    z = (hl @ E.T).gather(1, ids) * valid.double()[:, None]
    Az = (hl.abs() @ E.abs().T).gather(1, ids) * valid.double()[:, None]
    beta = inp["beta"]
    terms = F.softplus(z)
    terms[:, 0] = beta * F.softplus(-z[:, 0])
    terms = terms * valid.double()[:, None]
    nwg = -(-cap // ROWS_PER_WG)
    own = torch.arange(c) // ROWS_PER_WG
    parts = torch.zeros(nwg, 3, dtype=torch.float64)
    parts[:, 0].index_add_(0, own, terms.sum(-1))
    parts[:, 1].index_add_(0, own, valid.double())
    parts[:, 2].index_add_(0, own, terms[:, 1:].sum(-1))
    Aparts = torch.zeros(nwg, 3, dtype=torch.float64)
    Aparts[:, 0].index_add_(0, own, (terms + Az).sum(-1))
    Aparts[:, 2].index_add_(0, own, (terms + Az)[:, 1:].sum(-1))
    nterms = torch.zeros(nwg, dtype=torch.float64).index_add_(0, own, valid.double() * (1 + N))
    total, negs = float(terms.sum()), float(terms[:, 1:].sum())
    out = torch.tensor([total, float(valid.sum()), total / inp["divisor"], negs], dtype=torch.float64)
    zb = z if z_stored is None else z_stored[:c].double()
    s = (1.0 if inp["dloss"] is None else inp["dloss"]) / inp["divisor"]
    w = s * torch.sigmoid(zb)
    w[:, 0] = -s * beta * torch.sigmoid(-zb[:, 0])
    w = w * valid.double()[:, None]
    bw = torch.full_like(w, abs(s))
    bw[:, 0] = abs(s) * beta
    Aw = bw * (1 + zb.abs()) * valid.double()[:, None]
    dh = torch.zeros(c, inp["V1"], dtype=torch.float64).scatter_add_(1, ids, w) @ E
    Adh = torch.zeros(c, inp["V1"], dtype=torch.float64).scatter_add_(1, ids, w.abs()) @ E.abs()
    keys = torch.zeros(cap, 1 + N, dtype=torch.int64)
    keys[:c] = ids * valid[:, None]
    return dict(z=z, Az=Az, terms=terms, out=out, parts=parts, Aparts=Aparts, nterms=nterms, w=w, Aw=Aw, dh=dh,
                Adh=Adh, keys=keys.reshape(-1), valid=valid, ids=ids)


def _untouched(t, c):
    """rows at or past the count still hold their NaN / sentinel fill"""
    rest = t[c:]
    if rest.numel() == 0:
        return 0.0
    ok = torch.isnan(rest) if rest.is_floating_point() else rest == -777
    return 0.0 if bool(ok.all()) else math.inf


def check_head(inp, o, staged=True):
    """o: z [cap][1+N], out [4], parts [workgroups][3] (float64), w [cap][1+N], dh [cap][d], keys [cap*(1+N)], the
    per-row outputs pre-filled with NaN (keys: -777).  staged: w and dh against the logits o["z"] itself (what the
    backward read).  Returns {name: worst error / bound}; > 1 fails."""
    c, N, d = inp["count"], inp["N"], inp["d"]
    r = head_ref(inp, z_stored=o["z"] if staged else None)
    res = {"z": ratio(o["z"][:c], r["z"], bound_f32(r["Az"], d)),
           "z.past": _untouched(o["z"], c)}
    K = d + r["nterms"]
    res["part.sum"] = ratio(o["parts"][:, 0], r["parts"][:, 0], bound_f32(r["Aparts"][:, 0], K))
    res["part.neg"] = ratio(o["parts"][:, 2], r["parts"][:, 2], bound_f32(r["Aparts"][:, 2], K))
    res["part.n"] = 0.0 if torch.equal(o["parts"][:, 1].double(), r["parts"][:, 1]) else math.inf
    Kt = d + float(r["nterms"].sum()) + 2
    At = float(r["Aparts"][:, 0].sum())
    res["out.sum"] = ratio(o["out"][0], r["out"][0], bound_f32(At, Kt))
    res["out.n"] = 0.0 if float(o["out"][1]) == float(r["out"][1]) else math.inf
    res["out.mean"] = ratio(o["out"][2], r["out"][2], bound_f32(At / inp["divisor"], Kt + 1))
    res["out.neg"] = ratio(o["out"][3], r["out"][3], bound_f32(float(r["Aparts"][:, 2].sum()), Kt))
    res["w"] = ratio(o["w"][:c], r["w"], bound_f32(r["Aw"], 10) + TINY * r["valid"].double()[:, None])
    res["w.past"] = _untouched(o["w"], c)
    res["dh"] = ratio(o["dh"][:c, :d], r["dh"], bound_f32(r["Adh"], d + 2 + (1 + N)) + TINY)
    res["dh.past"] = _untouched(o["dh"], c)
    res["keys"] = 0.0 if torch.equal(o["keys"].reshape(-1), r["keys"]) else math.inf
    return res


def emu_head(inp, mut=None):
    """The two head launches in float32 (bf16 inputs as stored), outputs shaped and pre-filled as check_head takes
    them.  mut plants one mistake (MUTATIONS)."""
    c, cap, N, d = inp["count"], inp["cap"], inp["N"], inp["d"]
    f32 = torch.float32
    hl, E = inp["hl"][:c, :d].float(), inp["E"].float()
    ids, valid = _ids(inp)
    vf = valid.float()
    E = E.clone()
    E[0] = 0
    z = (hl @ E.T).gather(1, ids) * vf[:, None]
    beta = np.float32(inp["beta"])
    terms = F.softplus(z)
    terms[:, 0] = beta * F.softplus(-z[:, 0])
    if mut == "beta_on_negs":
        terms[:, 1:] = beta * terms[:, 1:]
    if mut == "neg_mean":
        terms[:, 1:] = terms[:, 1:] / N
    if mut == "drop_id0":
        terms[:, 1:] = terms[:, 1:] * (ids[:, 1:] != 0).float()
    terms = terms * vf[:, None]
    nwg = -(-cap // ROWS_PER_WG)
    own = torch.arange(c) // ROWS_PER_WG
    parts = torch.zeros(nwg, 3, dtype=torch.float64)
    parts[:, 0].index_add_(0, own, terms.double().sum(-1))
    parts[:, 1].index_add_(0, own, valid.double())
    parts[:, 2].index_add_(0, own, terms[:, 1:].double().sum(-1))
    tot = parts.sum(0)
    out = torch.tensor([tot[0], tot[1], tot[0] / inp["divisor"], tot[2]]).float()
    s = np.float32((1.0 if inp["dloss"] is None else inp["dloss"]) / inp["divisor"])
    w = s * torch.sigmoid(z)
    w[:, 0] = -(s * beta) * torch.sigmoid(-z[:, 0])
    if mut == "g0_sign":
        w[:, 0] = -w[:, 0]
    if mut == "beta_on_negs":
        w[:, 1:] = beta * w[:, 1:]
    if mut == "neg_mean":
        w[:, 1:] = w[:, 1:] / N
    w = w * vf[:, None]
    dh = torch.zeros(c, inp["V1"]).scatter_add_(1, ids, w) @ E
    rows = cap if mut == "past_count" else c

    def full(t, cols, fill=math.nan, dt=f32):
        o = torch.full((cap, cols), fill, dtype=dt)
        o[:c] = t
        o[c:rows] = 0
        return o
    keys = torch.zeros(cap, 1 + N, dtype=torch.int64)
    keys[:c] = ids * valid[:, None]
    return dict(z=full(z, 1 + N), out=out, parts=parts, w=full(w, 1 + N), dh=full(dh, d), keys=keys.reshape(-1))


# ---------------------------------------------------------------- rs_item_grad_weighted
def weighted_inputs(rows, per, d, dtype, table_rows, seed=0, hot=0.0, edge=False):
    """keys int64 [rows * per] (key 0 present; hot: that share of the entries on one key, so its run crosses many
    32-entry chunks; edge: runs that end exactly on a chunk edge), w fp32 [rows * per], f [rows][d], dtable0."""
    g = torch.Generator().manual_seed(31 * seed + rows + 7 * per + d)
    n = rows * per
    keys = torch.randint(0, table_rows, (n,), generator=g)
    if hot:
        keys[torch.rand(n, generator=g) < hot] = min(7, table_rows - 1)
    if edge:                                   # sorted position of key k's run: multiples of 32 entries for k = 1, 2, 3
        keys = torch.cat([torch.zeros(32, dtype=torch.int64), torch.full((64,), 1), torch.full((32,), 2),
                          torch.full((n - 128,), 3)])[torch.randperm(n, generator=g)]
    keys[:3] = 0
    w = torch.randn(n, generator=g)
    f = torch.randn(rows, d, generator=g).to(dtype)
    t0 = torch.randn(table_rows, d, generator=g) if table_rows <= 4096 else torch.zeros(table_rows, d)
    return dict(rows=rows, per=per, d=d, table_rows=table_rows, keys=keys, w=w, f=f, dtable0=t0)


def weighted_ref(inp):
    """(dtable float64, its magnitude, contributions per row)"""
    keys, per = inp["keys"], inp["per"]
    src = torch.arange(keys.numel()) // per
    live = (keys != 0).double()[:, None]
    c = inp["w"].double()[:, None] * inp["f"].double()[src] * live
    t = inp["dtable0"].double().clone().index_add_(0, keys, c)
    A = inp["dtable0"].double().abs().index_add_(0, keys, c.abs())
    n = torch.zeros(inp["table_rows"], dtype=torch.float64).index_add_(0, keys, live[:, 0])
    return t, A, n


def check_weighted(inp, dtable):
    t, A, n = weighted_ref(inp)
    touched = n > 0
    same = torch.equal(dtable[~touched], inp["dtable0"][~touched])        # rows without an entry, row 0: untouched bits
    return {"dtable": ratio(dtable, t, bound_f32(A, n[:, None] + 1)),
            "dtable.untouched": 0.0 if same else math.inf}


def emu_weighted(inp, mut=None):
    keys, per = inp["keys"], inp["per"]
    e = torch.arange(keys.numel())
    src = e // per
    w = inp["w"][src] if mut == "w_by_row" else inp["w"]
    live = torch.ones_like(w) if mut == "key0_grad" else (keys != 0).float()
    c = (w * live)[:, None] * inp["f"].float()[src]
    return inp["dtable0"].clone().index_add_(0, keys, c)


# ---------------------------------------------------------------- rs_sas_sample_negs on the host
_M64 = (1 << 64) - 1


def _splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def sample_negs_ref(histories, item_num, B, T, N, seed_base, salt):
    """(seq, pos, neg) of rs_sas_sample_negs for the step seed `seed_base` (the value AFTER the sampler advanced it):
    user = mulhi(splitmix64(seed ^ C (b + 1)), n_users); negative j of position (b, t) = the first of
    mulhi(splitmix64(base + (j << 8) + a), item_num + 1), a = 0..255, outside the row's window, base = seed +
    ((b T + t) << 20); then the linear scan (never reached in practice)."""
    seed = (salt ^ ((seed_base * 0xD1B54A32D192ED03) & _M64)) & _M64
    V1 = item_num + 1
    seq, pos = np.zeros((B, T), np.int64), np.zeros((B, T), np.int64)
    neg = np.zeros((B, T, N), np.int64)
    for b in range(B):
        u = (_splitmix64(seed ^ ((0xA0761D6478BD642F * (b + 1)) & _M64)) * len(histories)) >> 64
        win = list(histories[u])[-T:]
        n = len(win)
        pad = T - n + 1
        inwin = set(win)
        for t in range(T):
            o = t - pad
            if o < 0:
                continue
            seq[b, t], pos[b, t] = win[o], win[o + 1]
            for j in range(N):
                base = (seed + ((b * T + t) << 20) + (j << 8)) & _M64
                v = (_splitmix64(base) * V1) >> 64
                a = 1
                while a < 256 and v in inwin:
                    v = (_splitmix64((base + a) & _M64) * V1) >> 64
                    a += 1
                k = 0
                while k < V1 and v in inwin:
                    v, k = (v + 1) % V1, k + 1
                neg[b, t, j] = v
    return seq, pos, neg
