"""Float64 references for BERT4Rec's sampled softmax over batch-shared candidates (TEST INFRASTRUCTURE ONLY).

The objective, on top of ``oracle.bert.encode`` with the untied output layer E = out.weight [V1][d], b = out.bias:

    h_r   = encode(tokens)[r]                            for every position r with labels_r != 0 ("labelled")
    z_r0  = <h_r, E[labels_r]> + b[labels_r]
    z_rj  = <h_r, E[cand_j]> + b[cand_j],  j = 1..K      cand: int64 [K]; an id outside [1, V1) counts as 0
    live(r, j) = cand_j != 0 and cand_j != labels_r      id 0 = an ignored slot; accidental hits masked
    loss  = (1 / max(n, 1)) * sum_r [ log( exp(z_r0) + sum_{live j} exp(z_rj) ) - z_r0 ],   n = #labelled

``head_fwd_ref`` / ``head_bwd_ref``: the two head launches (rs_sce_head_fwd / _bwd) alone, in float64 on the kernels'
own inputs.  They wrap the tied head's references of tests/sas_sce_ref.py through the identity

    <h, E[v]> + b[v] = <[h, 1], [E[v], b[v]]>

so every quantity of that file is computed on the biased logits, the magnitude sums gain their |b| terms (the
appended column contributes 1 * |b[v]|), pg's appended column is coef and dEc's is dbc[j] = s sum_r p_rj.
"""
import numpy as np
import torch
import torch.nn.functional as F

import sas_sce_ref as base
from oracle import bert as obert

uniform_items_ref = base.uniform_items_ref


# ---------------------------------------------------------------- the head kernels alone
def _aug(hl, E, bias):
    hl, E = np.asarray(hl, np.float64), np.asarray(E, np.float64)
    b = np.zeros(E.shape[0]) if bias is None else np.asarray(bias, np.float64)
    return np.concatenate([hl, np.ones((hl.shape[0], 1))], 1), np.concatenate([E, b[:, None]], 1)


def head_fwd_ref(hl, lab, count, E, bias, cand, divisor):
    """-> lse [count], z0 [count] (both 0 on a row with lab 0), out = (loss sum, valid rows, sum / divisor)."""
    h1, E1 = _aug(hl, E, bias)
    return base.head_fwd_ref(h1, lab, count, E1, cand, divisor)


def head_bwd_ref(hl, lab, count, E, bias, cand, divisor, dloss=1.0):
    """-> dh [count][d], coef [count], pg [count][d], dEc [K][d], dbc [K], keys [cap + K], and the magnitude sums
    (sas_sce_ref's, with the |b| terms in z / z0, plus dbc = |s| sum_r p_rj)."""
    h1, E1 = _aug(hl, E, bias)
    dh, coef, pg, dEc, keys, mag = base.head_bwd_ref(h1, lab, count, E1, cand, divisor, dloss)
    assert np.array_equal(pg[:, -1], coef)
    mag = dict(mag, dh=mag["dh"][:, :-1], dEc=mag["dEc"][:, :-1], dbc=mag["dEc"][:, -1])
    return dh[:, :-1], coef, pg[:, :-1], dEc[:, :-1], dEc[:, -1], keys, mag


def scatter_bias_grad(V1, cap, keys, coef, dbc):
    """db [V1]: the entries of {coef at lab_r, dbc at cand_j} summed per key; key 0 gets nothing."""
    db = np.zeros(V1)
    count = coef.shape[0]
    np.add.at(db, keys[:count], coef)
    np.add.at(db, keys[cap:], dbc)
    db[0] = 0.0
    return db


# ---------------------------------------------------------------- the model
def _ids(t, V1):
    t = torch.as_tensor(t).reshape(-1)
    return torch.where((t <= 0) | (t >= V1), torch.zeros_like(t), t)


def sce_rows(h, W, b, labels, cand):
    """Per position: (lse over {label} + live candidates, z_r0, labelled)."""
    d = h.shape[-1]
    hr = h.reshape(-1, d)
    lab, cand = _ids(labels, W.shape[0]), _ids(cand, W.shape[0])
    z0 = (hr * W[lab]).sum(-1) + b[lab]
    z = hr @ W[cand].T + b[cand]
    live = (cand != 0)[None, :] & (cand[None, :] != lab[:, None])
    z = z.masked_fill(~live, -float("inf"))
    return torch.logsumexp(torch.cat([z0[:, None], z], 1), 1), z0, lab != 0


def sce_from_hidden(h, W, b, labels, cand):
    lse, z0, valid = sce_rows(h, W, b, labels, cand)
    return ((lse - z0) * valid).sum() / max(int(valid.sum()), 1)


def sce_loss(P, tokens, labels, cand, num_blocks, heads, p=0.0, hp=0.0, masks=None):
    h = obert.encode(P, torch.as_tensor(tokens), num_blocks, heads, p, hp, masks)
    return sce_from_hidden(h, P["out.weight"], P["out.bias"], labels, cand)


def sce_loss_and_grads(P, tokens, labels, cand, num_blocks, heads, p=0.0, hp=0.0, masks=None):
    """(loss, {name: gradient}) -- every parameter, zeros where the loss does not reach one."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    loss = sce_loss(leaves, tokens, labels, cand, num_blocks, heads, p, hp, masks)
    loss.backward()
    return loss.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}


def torch_head_definition(h, W, b, labels, cand):
    """The plain-torch spelling on hidden rows h (n, d): gather the logits of {label} + candidates, mask the dead
    ones with -inf, F.cross_entropy with target 0 over the labelled rows."""
    lab, cand = _ids(labels, W.shape[0]), _ids(cand, W.shape[0])
    rows = torch.nonzero(lab != 0).reshape(-1)
    if rows.numel() == 0:
        return h.sum() * 0
    ids = torch.cat([lab[rows, None], cand[None, :].expand(rows.numel(), -1)], 1)         # (n, 1 + K)
    logits = (h.reshape(-1, h.shape[-1])[rows, None, :] * W[ids]).sum(-1) + b[ids]
    dead = (ids == 0) | (ids == lab[rows, None])
    dead[:, 0] = False
    logits = logits.masked_fill(dead, -float("inf"))
    return F.cross_entropy(logits, torch.zeros(rows.numel(), dtype=torch.int64))


def torch_definition(P, tokens, labels, cand, num_blocks, heads):
    h = obert.encode(P, torch.as_tensor(tokens), num_blocks, heads)
    return torch_head_definition(h, P["out.weight"], P["out.bias"], labels, cand)
