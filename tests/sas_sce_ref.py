"""Float64 references for the SASRec sampled softmax over batch-shared candidates (TEST INFRASTRUCTURE ONLY).

The objective, on top of ``oracle.sas.log2feats``:

    f_r   = last_layernorm(log2feats(seq))[r]          for every position r with pos_r != 0 ("valid")
    z_r0  = <f_r, E[pos_r]>                            E = item_emb.weight (tied)
    z_rj  = <f_r, E[cand_j]>,  j = 1..K                cand: int64 [K], ids in [0, V]
    live(r, j) = cand_j != 0 and cand_j != pos_r       id 0 = an ignored slot; accidental hits masked
    loss  = (1 / max(n, 1)) * sum_valid r [ log( exp(z_r0) + sum_{live j} exp(z_rj) ) - z_r0 ],   n = #valid

Duplicate ids in cand are separate classes; a row with no live candidate contributes 0; no valid row: loss 0.

``emu=oracle.sas.BF16Storage()`` additionally rounds to bf16 exactly where the HIP path stores bf16: the compact
LayerNorm output hl (log2feats' own last rounding), the table's compute copy, the dh the LayerNorm backward reads and
dx (the last block output's gradient rounding inside log2feats).  The probabilities are never stored.

``head_fwd_ref`` / ``head_bwd_ref``: the two head launches of sas_sce.hip alone, in float64 on the kernels' own inputs.
``uniform_items_ref``: the host restatement of rs_uniform_items' counter-based draws.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import sas as osas


def sce_rows(f, E, pos, cand, R):
    """Per position: (lse over {positive} + live candidates, z_r0, valid) -- the pieces of the loss."""
    f = R.g(f)                                                       # R:G the dh the LayerNorm backward reads
    d = f.shape[-1]
    fr, tgt = f.reshape(-1, d), pos.reshape(-1)
    cand = cand.reshape(-1)
    Eall = F.embedding(torch.arange(E.shape[0]), E, padding_idx=0)   # a lookup: row 0 stays out of the gradient
    z0 = (fr * Eall[tgt]).sum(-1)
    z = fr @ Eall[cand].T                                            # (M, K)
    live = (cand != 0)[None, :] & (cand[None, :] != tgt[:, None])
    z = z.masked_fill(~live, -float("inf"))
    return torch.logsumexp(torch.cat([z0[:, None], z], 1), 1), z0, tgt != 0


def sce_from_feats(f, E, pos, cand, R):
    """f (B, T, d), E (V+1, d) the (possibly rounded) table, cand (K,) -> the loss; R: oracle.sas.Exact / BF16Storage."""
    lse, z0, valid = sce_rows(f, E, pos, cand, R)
    return ((lse - z0) * valid).sum() / max(int(valid.sum()), 1)


def sce_loss(P, seq, pos, cand, num_blocks, heads, p=0.0, masks=None, emu=None, l2_emb=0.0):
    R = emu or osas.Exact()
    f = osas.log2feats(P, seq, num_blocks, heads, p, masks, emu)
    loss = sce_from_feats(f, R.w(P["sas.item_emb.weight"]), torch.as_tensor(pos), torch.as_tensor(cand), R)
    if l2_emb:
        for t in P.values():
            loss = loss + l2_emb * torch.norm(t)
    return loss


def sce_loss_and_grads(P, seq, pos, cand, num_blocks, heads, p=0.0, masks=None, emu=None, l2_emb=0.0):
    """(loss, {name: gradient}) -- every parameter, zeros where the loss does not reach one."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    loss = sce_loss(leaves, seq, pos, cand, num_blocks, heads, p, masks, emu, l2_emb)
    loss.backward()
    return loss.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}


def torch_definition(P, seq, pos, cand, num_blocks, heads):
    """The plain-torch spelling: gather the logits, mask with -inf, F.cross_entropy with target 0."""
    f = osas.log2feats(P, seq, num_blocks, heads)
    W = P["sas.item_emb.weight"]
    d = f.shape[-1]
    fr, tgt = f.reshape(-1, d), torch.as_tensor(pos).reshape(-1)
    cand = torch.as_tensor(cand).reshape(-1)
    rows = torch.nonzero(tgt != 0).reshape(-1)
    if rows.numel() == 0:
        return fr.sum() * 0
    ids = torch.cat([tgt[rows, None], cand[None, :].expand(rows.numel(), -1)], 1)       # (n, 1 + K)
    logits = (fr[rows, None, :] * W[ids]).sum(-1)
    dead = (ids == 0) | (ids == tgt[rows, None])
    dead[:, 0] = False
    logits = logits.masked_fill(dead, -float("inf"))
    return F.cross_entropy(logits, torch.zeros(rows.numel(), dtype=torch.int64))


# ---------------------------------------------------------------- the head kernels alone
def _head(hl, lab, count, E, cand):
    hl, E = np.asarray(hl, np.float64)[:count], np.asarray(E, np.float64)
    lab, cand = np.asarray(lab, np.int64)[:count], np.asarray(cand, np.int64)
    V1 = E.shape[0]
    lab = np.where((lab <= 0) | (lab >= V1), 0, lab)
    cand = np.where((cand <= 0) | (cand >= V1), 0, cand)
    valid = lab != 0
    z0 = (hl * E[lab]).sum(-1)
    z = hl @ E[cand].T
    live = (cand != 0)[None, :] & (cand[None, :] != lab[:, None]) & valid[:, None]
    return hl, E, lab, cand, valid, z0, z, live


def head_fwd_ref(hl, lab, count, E, cand, divisor):
    """-> lse [count], z0 [count] (both 0 on a row with lab 0), out = (loss sum, valid rows, sum / divisor)."""
    hl, E, lab, cand, valid, z0, z, live = _head(hl, lab, count, E, cand)
    m = np.maximum(z0, np.where(live, z, -np.inf).max(-1, initial=-np.inf)) if z.shape[1] else z0
    s = np.exp(z0 - m) + (np.exp(np.where(live, z - m[:, None], -np.inf))).sum(-1)
    lse = np.where(valid, m + np.log(s), 0.0)
    z0 = np.where(valid, z0, 0.0)
    total = float((lse - z0).sum())
    return lse, z0, (total, float(valid.sum()), total / float(divisor))


def head_bwd_ref(hl, lab, count, E, cand, divisor, dloss=1.0):
    """-> dh [count][d], coef [count], pg [count][d], dEc [K][d], keys [cap + K] in float64 / int64, and the
    magnitude sums the error bounds are built from: a dict of arrays shaped like the outputs."""
    cap = np.asarray(lab).shape[0]
    hl, E, lab, cand, valid, z0, z, live = _head(hl, lab, count, E, cand)
    lse, _, _ = head_fwd_ref(hl, lab, count, E, cand, 1.0)
    s = float(dloss) / float(divisor)
    p = np.where(live, np.exp(np.where(live, z, 0.0) - lse[:, None]), 0.0)
    p0 = np.where(valid, np.exp(z0 - lse), 1.0)
    coef = (p0 - 1.0) * s
    Ec = E[cand]
    dh = s * (p @ Ec) + coef[:, None] * E[lab]
    pg = coef[:, None] * hl
    dEc = s * (p.T @ hl)
    keys = np.zeros(cap + cand.shape[0], np.int64)
    keys[:count] = lab
    keys[cap:] = cand
    mag = dict(dh=abs(s) * (p @ np.abs(Ec)) + np.abs(coef)[:, None] * np.abs(E[lab]),
               dEc=abs(s) * (p.T @ np.abs(hl)), psum=p.sum(-1), p0=p0, z=np.abs(hl) @ np.abs(Ec).T,
               z0=(np.abs(hl) * np.abs(E[lab])).sum(-1), nlive=live.sum(-1))
    return dh, coef, pg, dEc, keys, mag


# ---------------------------------------------------------------- rs_uniform_items on the host
_M64 = (1 << 64) - 1


def _splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def uniform_items_ref(seed_base, salt, item_num, K):
    """The K draws of rs_uniform_items for the step seed `seed_base` (the value AFTER the sampler advanced it)."""
    seed = (salt ^ ((seed_base * 0xD1B54A32D192ED03) & _M64)) & _M64
    return np.array([1 + ((_splitmix64((seed + 0x632BE59BD9B4E019 * (j + 1)) & _M64) * item_num) >> 64)
                     for j in range(K)], np.int64)
