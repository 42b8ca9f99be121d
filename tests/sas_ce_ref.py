"""Float64 references for the SASRec tied full-catalogue cross-entropy loss (TEST INFRASTRUCTURE ONLY).

The objective, on top of ``oracle.sas.log2feats``:

    f      = last_layernorm(log2feats(seq))
    E      = item_emb(arange(V+1))            # a lookup: padding_idx=0 keeps row 0 out of the gradient
    logits = f @ E.T                          # (B, T, V+1); class 0 is the zero padding row
    loss   = cross_entropy(logits, pos, ignore_index=0)   # mean over pos != 0; 0 (not NaN) when there is none

``emu=oracle.sas.BF16Storage()`` additionally rounds to bf16 exactly where the HIP path stores bf16: the compact
LayerNorm output hl (log2feats' own last rounding), the table's compute copy, dlogits, the reduced dh and dx (the
last block output's gradient rounding inside log2feats).

``rows_fwd_ref`` / ``rows_bwd_ref``: the two row kernels of sas_ce.hip alone, in float64 on the kernels' own inputs.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import sas as osas


def ce_from_feats(f, E, pos, R):
    """f (B, T, d), E (V+1, d) the (possibly rounded) table -> the loss; R: oracle.sas.Exact / BF16Storage."""
    V1 = E.shape[0]
    f = R.g(f)                                                       # R:G the reduced dh
    Eall = F.embedding(torch.arange(V1), E, padding_idx=0)
    logits = R.g(f @ Eall.T)                                         # R:G dlogits
    tgt = pos.reshape(-1)
    n = int((tgt != 0).sum())
    total = F.cross_entropy(logits.reshape(-1, V1), tgt, ignore_index=0, reduction="sum")
    return total / max(n, 1)


def ce_loss(P, seq, pos, num_blocks, heads, p=0.0, masks=None, emu=None, l2_emb=0.0):
    R = emu or osas.Exact()
    f = osas.log2feats(P, seq, num_blocks, heads, p, masks, emu)
    loss = ce_from_feats(f, R.w(P["sas.item_emb.weight"]), pos, R)
    if l2_emb:
        for t in P.values():
            loss = loss + l2_emb * torch.norm(t)
    return loss


def ce_loss_and_grads(P, seq, pos, num_blocks, heads, p=0.0, masks=None, emu=None, l2_emb=0.0):
    """(loss, {name: gradient}) -- every parameter, zeros where the loss does not reach one."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    loss = ce_loss(leaves, seq, pos, num_blocks, heads, p, masks, emu, l2_emb)
    loss.backward()
    return loss.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}


def torch_definition(P, seq, pos, num_blocks, heads):
    """The issue's four-line definition spelled with plain torch ops (for checking ce_loss itself)."""
    f = osas.log2feats(P, seq, num_blocks, heads)
    W = P["sas.item_emb.weight"]
    V1 = W.shape[0]
    E = F.embedding(torch.arange(V1), W, padding_idx=0)
    logits = f @ E.T
    return F.cross_entropy(logits.view(-1, V1), pos.view(-1), ignore_index=0)


# ---------------------------------------------------------------- the row kernels alone
def compact_ref(labels, cap):
    """(idx [cap] (-1 past the valid rows), rank [M], count) as rs_compact_rows."""
    labels = np.asarray(labels).reshape(-1)
    rows = np.nonzero(labels != 0)[0]
    idx = np.full(cap, -1, np.int32)
    rank = np.full(labels.shape[0], -1, np.int32)
    n = min(len(rows), cap)
    idx[:n] = rows[:n]
    rank[rows[:n]] = np.arange(n, dtype=np.int32)
    return idx, rank, n


def rows_fwd_ref(x, labels, cap, gamma, beta, eps=1e-8):
    """x (M, d) float64 (the bf16 input's values) -> idx, rank, count, hl (count, d) unrounded, lab, mean, rstd."""
    idx, rank, n = compact_ref(labels, cap)
    xs = np.asarray(x, np.float64)[idx[:n]]
    mu = xs.mean(-1)
    var = ((xs - mu[:, None]) ** 2).mean(-1)
    rstd = 1.0 / np.sqrt(var + eps)
    hl = (xs - mu[:, None]) * rstd[:, None] * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
    return idx, rank, n, hl, np.asarray(labels).reshape(-1)[idx[:n]], mu, rstd


def reduced_dh(slab):
    """slab (splits, cap, d) float32 -> the bf16 value of its sum in split order, as float64.  The sum is the
    kernels' own sequence of fp32 additions (exact to reproduce), so the bf16 rounding falls on the same value."""
    acc = np.zeros(slab.shape[1:], np.float32)
    for z in range(slab.shape[0]):
        acc = (acc + slab[z]).astype(np.float32)
    return torch.from_numpy(acc).to(torch.bfloat16).double().numpy()


def rows_bwd_ref(slab, rank, x, gamma, mean, rstd, nparts, d):
    """-> dx (M, d) float64 (0 at rank < 0), part (nparts, 2, d): set b sums the rows r with (r // (2048 // d)) % nparts
    == b; mean / rstd per compact row (the kernel's fp32 inputs)."""
    x = np.asarray(x, np.float64)
    M = x.shape[0]
    g = np.asarray(gamma, np.float64)
    dh = reduced_dh(np.asarray(slab, np.float32))
    dx = np.zeros((M, d))
    part = np.zeros((nparts, 2, d))
    rpb = 2048 // d
    for r in range(M):
        k = int(rank[r])
        if k < 0:
            continue
        a, u = float(rstd[k]), x[r] - float(mean[k])
        dy = dh[k]
        gq = dy * g
        dx[r] = a * (gq - gq.mean()) - (a ** 3) * (gq * u).mean() * u
        b = (r // rpb) % nparts
        part[b, 0] += dy * u * a
        part[b, 1] += dy
    return dx, part
