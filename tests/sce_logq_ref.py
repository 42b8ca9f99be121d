"""Float64 references for the logQ-corrected sampled softmax and its alias sampler (TEST INFRASTRUCTURE ONLY).

The definition (rs_sce_head_logq_fwd / _bwd, include/recsys_hip.h), on top of tests/sas_sce_ref.py and
tests/bert_sce_ref.py:

    z_r0 = <h_r, E[lab_r]>  + b[lab_r]  - logq[lab_r]
    z_rj = <h_r, E[cand_j]> + b[cand_j] - logq[cand_j]

and everything else -- live, the loss, lse, dh, coef, pg, dEc, dbc, keys -- on these logits exactly as there.  logq is
a constant (no gradient); entry 0 is never read; dbc exists with a bias alone.

The head references wrap the tied head's through the identity

    <h, E[v]> + b[v] - logq[v] = <[h, 1, 1], [E[v], b[v], -logq[v]]>

so that every magnitude sum of that file gains |b[v]| + |logq[v]| (the two appended columns contribute 1 * |b[v]| and
1 * |logq[v]|).  dEc's column under b is dbc; the one under -logq is the gradient logq would get, and is dropped.

Bounds of the head kernels (``head_bars``).  Those of tests/test_bert_sce_gpu.py (which are tests/test_sas_sce_gpu.py's
with the bias), widened by the rounding of the one fp32 subtraction the correction adds per logit.  The kernel forms
the per-id term t_v = fl(b_v - logq_v) once and adds it where it added b_v, so a logit carries, beyond the biased
head's roundings, the rounding of t_v:  |fl(b_v - logq_v) - (b_v - logq_v)| <= u |b_v - logq_v| <= u (|b_v| + |logq_v|)
<= u Z, with Z the logit's magnitude sum (which holds |b_v| + |logq_v| whole).  One more u Z per logit:

    z_r0   : (d + 4) u Z_r0                                                   (d + 3 there)
    lse_r  : u ((d + 6) Zmax_r + nlive_r + 16 + splits + |lse_r|)             (d + 5 there)
    e_r    = 1.01 (lse bar + (d + 6) u Zmax_r + 4 u)                          (d + 5 there)
    coef, pg, dh, dEc, dbc: as there, on these e_r

Underflow.  The bars above are relative to magnitudes; fp32 itself stops being relative below its smallest normal
number, TINY = 2^-126: a probability or a product under it is flushed to zero or rounded to a subnormal, an absolute
error of at most TINY per term.  Every bar of a sum of n such terms, each times a factor f, gains n TINY max(1, f):
dh (K candidates, f = |s| max|E|), dEc (count rows, f = |s| max|hl|), dbc (count rows, f = |s|), coef and pg (one
term, f = |s| max(1, max|hl|)).  It shows where z - logq spans a hundred units (the "big" problems), nowhere else.  A
bar that is exactly 0 -- a masked row, a dead slot -- stays 0: the output there must be 0.

Nothing in them comes from a kernel's output.  The same bars hold without a bias (t_v = -logq_v is then exact: the
bars are not tight there, and are not tightened).

``emu_head``: the head in float32 (bf16 probabilities where the MFMA takes them), with a ``mut`` switch that plants
one mistake; tests/test_sce_logq_ref.py holds the emulation inside the bars and every mistake outside them.

The alias sampler: ``alias_table_ref`` restates ItemProposal's build, ``realised_q_ref`` the distribution the draw
rule realises (exact integers), ``alias_items_ref`` rs_alias_items' draws.

Bound of the table (``table_bound``).  Let p_s = V w_s / sum(w) in exact arithmetic, keep_s / alias_s the float64
table before quantisation, M(v) = keep_(v-1) + sum over {s: alias_s = v} of (1 - keep_s) the mass (in slots) it gives
item v.  Quantisation: thr_s = max(1, floor(keep_s 2^32)) is within 1 of keep_s 2^32, and item v's count N(v) is a sum
of 1 + indegree(v) such terms, so |Qhat(v) - M(v) / V| <= (1 + indegree(v)) 2^-32 / V: the first term of the bound.
The float64 build (u64 = 2^-53): the initial p_s carries three roundings (the product, the correctly rounded sum, the
quotient): |fl(p_s) - p_s| <= 3.01 u64 pmax, and sum_s fl(p_s) is within 3.01 u64 V of V.  Each step of the loop
replaces p_l by fl(fl(p_l + p_s) - 1): two roundings of values below pmax + 1, an error <= 2.01 u64 (pmax + 1) in the
mass item l still has to place; item l is touched by at most V steps in all (one slot is settled per step).  A slot
settled inside the loop keeps exactly its current p.  A slot left over at the end keeps mass 1 instead of its current
p; the leftovers are all >= 1 or all < 1, so each one's |p - 1| is at most the sum of theirs, which is the total drift
of sum p from V: <= 3.01 u64 V + V 2.01 u64 (pmax + 1).  Together
    |M(v) - p_v| <= 3.01 u64 pmax + 3.01 u64 V + 2 V 2.01 u64 (pmax + 1),
and divided by V (pmax <= V):  |M(v) / V - Q(v)| <= u64 (3.01 + 3.01 + 4.02 (pmax + 1)) <= 8 u64 (pmax + 2): the
second term.
"""
import math

import numpy as np
import torch

import bert_sce_ref as bert_ref
import sas_sce_ref as base
from oracle import bert as obert
from oracle import sas as osas

U = 2.0 ** -24
TINY = 2.0 ** -126
U64 = 2.0 ** -53
uniform_items_ref = base.uniform_items_ref


# ---------------------------------------------------------------- the head kernels alone
def _aug(hl, E, bias, logq):
    hl, E = np.asarray(hl, np.float64), np.asarray(E, np.float64)
    b = np.zeros(E.shape[0]) if bias is None else np.asarray(bias, np.float64)
    q = np.zeros(E.shape[0]) if logq is None else np.asarray(logq, np.float64).copy()
    q[0] = 0.0                                                       # never read: whatever the caller left there
    one = np.ones((hl.shape[0], 2))
    return np.concatenate([hl, one], 1), np.concatenate([E, b[:, None], -q[:, None]], 1)


def head_fwd_ref(hl, lab, count, E, bias, logq, cand, divisor):
    """-> lse [count], z0 [count] (both 0 on a row with lab 0), out = (loss sum, valid rows, sum / divisor)."""
    h2, E2 = _aug(hl, E, bias, logq)
    return base.head_fwd_ref(h2, lab, count, E2, cand, divisor)


def head_bwd_ref(hl, lab, count, E, bias, logq, cand, divisor, dloss=1.0):
    """-> dh [count][d], coef [count], pg [count][d], dEc [K][d], dbc [K] (the column under b: meaningful with a bias),
    keys [cap + K], and sas_sce_ref's magnitude sums with the |b| + |logq| terms in z / z0, plus dbc."""
    h2, E2 = _aug(hl, E, bias, logq)
    dh, coef, pg, dEc, keys, mag = base.head_bwd_ref(h2, lab, count, E2, cand, divisor, dloss)
    mag = dict(mag, dh=mag["dh"][:, :-2], dEc=mag["dEc"][:, :-2], dbc=mag["dEc"][:, -2])
    return dh[:, :-2], coef, pg[:, :-2], dEc[:, :-2], dEc[:, -2], keys, mag


def head_bars(dt, ks, hl, lab, count, E, bias, logq, cand, divisor, dloss):
    """{name: (float64 value, bar)} for lse, z0, coef, pg, dh, dEc, dbc (with a bias), and "out" = ((sum, n, mean),
    (bar of the sum, 0, bar of the mean)); keys under "keys".  hl / E: the kernel's inputs (bf16 values included) as
    float64; ks: the candidate splits of the launch (rs_sce_head_dh_splits).  The docstring has the derivation."""
    hl64, E64 = np.asarray(hl, np.float64), np.asarray(E, np.float64)
    lab, cand = np.asarray(lab, np.int64), np.asarray(cand, np.int64)
    d, K, V1 = hl64.shape[1], cand.shape[0], E64.shape[0]
    fmt = 2.0 ** -7 if dt == torch.bfloat16 else 0.0
    dv = float(divisor)
    lse, z0, rout = head_fwd_ref(hl64, lab, count, E64, bias, logq, cand, dv)
    rdh, rcoef, rpg, rdEc, rdbc, rkeys, mag = head_bwd_ref(hl64, lab, count, E64, bias, logq, cand, dv, dloss)
    s = float(dloss) / dv
    labc = np.where((lab[:count] <= 0) | (lab[:count] >= V1), 0, lab[:count])
    valid = labc != 0
    zmax = np.maximum(mag["z0"], mag["z"].max(-1, initial=0.0)) * valid
    bar_z0 = (d + 4) * U * mag["z0"] * valid
    bar_lse = U * ((d + 6) * zmax + mag["nlive"] + 16 + ks + np.abs(lse)) * valid
    e_r = 1.01 * (bar_lse + (d + 6) * U * zmax + 4 * U)
    assert e_r.max(initial=0.0) < 2e-2                            # the first-order regime the bars are derived in
    bar_coef = abs(s) * (mag["p0"] * e_r + 4 * U) * valid
    Epos = np.abs(E64[labc])
    cc = np.where((cand <= 0) | (cand >= V1), 0, cand)
    h2, E2 = _aug(hl64, E64, bias, logq)
    z = h2[:count] @ E2[cc].T
    live = (cc != 0)[None, :] & (cc[None, :] != labc[:, None]) & valid[:, None]
    P = np.where(live, np.exp(np.where(live, z, 0.0) - lse[:, None]), 0.0)
    H = np.abs(hl64[:count])
    A = abs(s) * (P @ np.abs(E64[cc]))
    def under(bar, n, f):                                          # fp32 underflow, where there is a bar at all
        return bar + (bar > 0) * (n * TINY * max(1.0, f))
    hmax, emax = float(H.max(initial=0.0)), float(np.abs(E64).max())
    bars = dict(
        lse=(lse, bar_lse), z0=(z0, bar_z0), coef=(rcoef, under(bar_coef, 1, abs(s))),
        dh=(rdh, under((e_r[:, None] + (K + 4 + ks) * U + fmt) * A + bar_coef[:, None] * Epos + U * np.abs(rdh),
                       K + 1, abs(s) * emax)),
        pg=(rpg, under(bar_coef[:, None] * H + U * np.abs(rpg), 1, abs(s) * max(1.0, hmax))),
        dEc=(rdEc, under(abs(s) * ((P * e_r[:, None]).T @ H + ((count + 68) * U + fmt) * (P.T @ H)) + U * np.abs(rdEc),
                         count, abs(s) * hmax)))
    if bias is not None:
        bars["dbc"] = (rdbc, under(abs(s) * ((P * e_r[:, None]).sum(0) + (count + 68) * U * P.sum(0))
                                   + U * np.abs(rdbc), count, abs(s)))
    bar_sum = float((bar_lse + bar_z0).sum()) + U * abs(rout[0])
    bars["out"] = (np.array(rout), np.array([bar_sum, 0.0, bar_sum / dv + 2 * U * abs(rout[2])]))
    bars["keys"] = rkeys
    return bars


def worst(got, bars):
    """{name: worst |got - value| / bar}; where a bar is 0 (nothing to round) the output must be the value."""
    res = {}
    for k in bars:
        if k == "keys" or k not in got:
            continue
        w, bar = bars[k]
        g = np.asarray(got[k], np.float64)
        assert g.shape == np.asarray(w).shape, (k, g.shape, np.asarray(w).shape)
        if not np.isfinite(g).all():
            res[k] = math.inf
            continue
        err = np.abs(g - w)
        exact = bar == 0
        res[k] = max(float((err[~exact] / bar[~exact]).max(initial=0.0)), math.inf if (err[exact] != 0).any() else 0.0)
    return res


PATTERNS = ("mixed", "hits", "big")
LOGQ_KINDS = ("zipf", "deep")
V_HEAD = 300
# the shapes of the GPU head tests (tests/test_sce_logq_gpu.py) and of the emulation's checks on the CPU.  rows: a
# partial wave, a partial tile, a whole tile, three row tiles (the dEc launch's row splits exceed 1 from the second
# tile on); K: a partial tile, a tile less one, a tile, a tile and one, five tiles (the candidate splits of the
# forward and dh exceed 1 from the second tile on).  Widths: the fp32 sweeps (50 padded inside the fragments), the bf16
# sweeps of 64, 128 and 256, and the plain kernel (fp32 past 128, bf16 past 256).
HEAD_ROWS = (1, 17, 64, 130)
HEAD_K = (1, 63, 64, 65, 257)
HEAD_WIDTHS = ((torch.float32, 50), (torch.float32, 128), (torch.bfloat16, 64), (torch.bfloat16, 128),
               (torch.bfloat16, 256), (torch.float32, 136), (torch.bfloat16, 264))


def head_cases():
    """(rows, K, pattern, logq kind) over HEAD_ROWS x HEAD_K: the patterns and kinds rotate, so that every pair of
    them meets several shapes."""
    out = []
    for i, (rows, K) in enumerate((r, k) for r in HEAD_ROWS for k in HEAD_K):
        out.append((rows, K, PATTERNS[i % 3], LOGQ_KINDS[(i // 3) % 2]))
    return out


def zipf_logq(V, rng=None):
    """log Q of a Zipf(1) proposal over V items in a random (or the identity) order, entry 0 = 0: [V + 1] float32."""
    w = 1.0 / np.arange(1, V + 1)
    if rng is not None:
        w = w[rng.permutation(V)]
    return np.concatenate([[0.0], np.log(w / w.sum())]).astype(np.float32)


def head_problem(dt, d, rows, K, pattern, kind, seed):
    """hl [cap][d], E [V1][d], bias [V1], logq [V1] (fp32; entry 0 NaN: it must never be read), lab [cap], cand [K],
    cap = rows + 9, V1 = 301.
    mixed: id-0 slots, a duplicate, an accidental hit of row 0's label, ids outside [0, V1) among the candidates and
           in one label (they count as 0).
    hits:  every candidate is 0 or row 0's label: that row (and every row sharing the label) has no live candidate.
    big:   one candidate's row lies along hl[0] with <h, E> = 60 and has logq = -40: z - logq = 100 (plus its bias),
           past the 88 where exp alone overflows fp32.
    kind zipf: logq of a Zipf proposal in a random order (-1.8 .. -7.5); deep: the same stretched to reach -40."""
    rng = np.random.default_rng(seed)
    V = V_HEAD
    cap = rows + 9
    hl = torch.from_numpy(rng.standard_normal((cap, d))).to(dt)
    E = torch.from_numpy(rng.standard_normal((V + 1, d)) / math.sqrt(d)).to(dt)
    bias = torch.from_numpy(rng.standard_normal(V + 1)).float()
    logq = zipf_logq(V, rng)
    if kind == "deep":
        logq[1:] = logq[1:] * np.float32(40.0 / -logq[1:].min())
    lab = rng.integers(1, V + 1, cap)
    if pattern == "hits":
        cand = np.where(rng.random(K) < 0.3, 0, lab[0])
        cand[0] = lab[0]
        if K > 1:
            cand[-1] = 0
        if rows > 1:
            lab[1] = lab[0] % V + 1                                   # a row that does have a live candidate
    else:
        cand = rng.integers(1, V + 1, K)
        cand[rng.random(K) < 0.15] = 0                            # ignored slots
        if K > 3:
            cand[K // 2] = cand[0]                                # a duplicate for certain
            cand[1] = lab[0]                                      # an accidental hit
            cand[2] = 0
        if K > 8:
            cand[5], cand[6] = V + 1 + 5, -3                      # outside [0, V1): count as 0
        if rows > 4:
            lab[3] = V + 1 + 7                                    # a label outside: no row
        if not ((cand > 0) & (cand <= V) & (cand != lab[0])).any():
            cand[0] = lab[0] % V + 1
    if pattern == "big":
        j = int(np.nonzero((cand > 0) & (cand <= V) & (cand != lab[0]))[0][0])
        h0 = hl[0].double()
        E[int(cand[j])] = (h0 * (60.0 / float((h0 * h0).sum()))).to(dt)
        logq[int(cand[j])] = -40.0
    logq[0] = np.nan
    return V, cap, hl, E, bias, torch.from_numpy(logq), lab, cand


def emu_head(dt, hl, lab, count, E, bias, logq, cand, divisor, dloss, mut=None):
    """The head in float32 on the kernel's inputs: the per-id term t = fl(b - logq), z = fl(dot + t), a float32
    log-sum-exp, p = exp(z - lse), the probabilities rounded to bf16 where the MFMA takes them (bf16 inputs) -- every
    output of the two launches.  mut plants one mistake:
      plus       +logq in place of -logq
      pos        the positive left uncorrected
      slot       logq indexed by the candidate's slot j, not by its id
      zero_live  an id-0 slot made live, its term read from entry 0 (as if logq[0] were a class)
      dec        the correction applied in the forward and dh and dropped in the dEc role (dEc, dbc)"""
    f32 = np.float32
    V1, K = E.shape[0], len(cand)
    cap = len(lab)
    h = np.asarray(hl, np.float64)[:count].astype(f32)
    E = np.asarray(E, np.float64).astype(f32)
    lab = np.asarray(lab, np.int64)[:count]
    cand = np.asarray(cand, np.int64)
    lab = np.where((lab <= 0) | (lab >= V1), 0, lab)
    cc = np.where((cand <= 0) | (cand >= V1), 0, cand)
    b = np.zeros(V1, f32) if bias is None else np.asarray(bias, f32)
    q = np.asarray(logq, f32).copy()
    q[0] = f32(1.5) if mut == "zero_live" else f32(0)              # entry 0: read by that mistake alone
    sign = f32(-1) if mut == "plus" else f32(1)
    t = (b - sign * q).astype(f32)
    t_pos = b if mut == "pos" else t
    t_cand = (b[cc] - q[np.arange(K) % V1]).astype(f32) if mut == "slot" else t[cc]
    valid = lab != 0
    z0 = ((h * E[lab]).sum(-1, dtype=f32) + t_pos[lab]).astype(f32)
    dot = (h @ E[cc].T).astype(f32)
    z = (dot + t_cand[None, :]).astype(f32)
    live = (cc[None, :] != lab[:, None]) & valid[:, None]
    if mut != "zero_live":
        live &= (cc != 0)[None, :]
    zm = np.where(live, z, f32(-3e38))
    m = np.maximum(z0, zm.max(-1, initial=f32(-3e38))).astype(f32)
    ssum = (np.exp((z0 - m).astype(f32)) + np.where(live, np.exp((zm - m[:, None]).astype(f32)), f32(0)).sum(-1, dtype=f32))
    lse = np.where(valid, (m + np.log(ssum.astype(f32))).astype(f32), f32(0))
    z0 = np.where(valid, z0, f32(0))
    total = float((lse.astype(np.float64) - z0.astype(np.float64)).sum())
    s = f32(f32(dloss) / f32(divisor))
    p = np.where(live, np.exp((np.where(live, z, f32(0)) - lse[:, None]).astype(f32)), f32(0)).astype(f32)
    coef = np.where(valid, ((np.exp((z0 - lse).astype(f32)) - f32(1)) * s).astype(f32), f32(0))
    if mut == "dec":                                               # the dEc role sees the uncorrected logits
        z_dec = (dot + b[cc][None, :]).astype(f32)
        p_dec = np.where(live, np.exp((np.where(live, z_dec, f32(0)) - lse[:, None]).astype(f32)), f32(0)).astype(f32)
    else:
        p_dec = p
    rb = (lambda x: torch.from_numpy(x).bfloat16().float().numpy()) if dt == torch.bfloat16 else (lambda x: x)
    dh = (s * (rb(p) @ E[cc]).astype(f32) + coef[:, None] * E[lab]).astype(f32)
    pg = (coef[:, None] * h).astype(f32)
    dEc = (s * (rb(p_dec).T @ h).astype(f32)).astype(f32)
    dbc = (s * p_dec.sum(0, dtype=f32)).astype(f32)
    out = np.array([total, float(valid.sum()), total / float(divisor)])
    return dict(lse=lse, z0=z0, coef=coef, dh=dh, pg=pg, dEc=dEc, dbc=dbc, out=out)


# ---------------------------------------------------------------- the models
def sas_sce_loss(P, seq, pos, cand, logq, num_blocks, heads, p=0.0, masks=None, emu=None):
    """tests/sas_sce_ref.sce_loss with z_r0 -= logq[pos_r], z_rj -= logq[cand_j] (logq: float64 [V + 1], a constant)."""
    R = emu or osas.Exact()
    f = R.g(osas.log2feats(P, seq, num_blocks, heads, p, masks, emu))
    E = R.w(P["sas.item_emb.weight"])
    pos, cand = torch.as_tensor(pos), torch.as_tensor(cand).reshape(-1)
    q = torch.as_tensor(logq, dtype=torch.float64).clone()
    q[0] = 0.0
    d = f.shape[-1]
    fr, tgt = f.reshape(-1, d), pos.reshape(-1)
    Eall = torch.nn.functional.embedding(torch.arange(E.shape[0]), E, padding_idx=0)
    z0 = (fr * Eall[tgt]).sum(-1) - q[tgt]
    z = fr @ Eall[cand].T - q[cand]
    live = (cand != 0)[None, :] & (cand[None, :] != tgt[:, None])
    z = z.masked_fill(~live, -float("inf"))
    lse = torch.logsumexp(torch.cat([z0[:, None], z], 1), 1)
    valid = tgt != 0
    return ((lse - z0) * valid).sum() / max(int(valid.sum()), 1)


def bert_sce_loss(P, tokens, labels, cand, logq, num_blocks, heads, p=0.0, hp=0.0, masks=None):
    """tests/bert_sce_ref.sce_loss on the logits minus logq: the constant joins the bias' place, not its gradient."""
    h = obert.encode(P, torch.as_tensor(tokens), num_blocks, heads, p, hp, masks)
    q = torch.as_tensor(logq, dtype=torch.float64).clone()
    q[0] = 0.0
    return bert_ref.sce_from_hidden(h, P["out.weight"], P["out.bias"] - q, labels, cand)


def loss_and_grads(fn, P, *args, **kw):
    """(loss, {name: gradient}) of fn(P, *args, **kw) -- every parameter, zeros where the loss does not reach one."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    loss = fn(leaves, *args, **kw)
    loss.backward()
    return loss.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}


# ---------------------------------------------------------------- the alias table and its draws
def alias_table_ref(weights):
    """(thr uint32 [V], alias int64 [V]) for weights float64 [V + 1] (entry 0 ignored): ItemProposal's build, restated
    with Python floats and ints alone.  p_s = w_(s+1) V / fsum(w); smalls (p < 1) and larges on two stacks in
    ascending order; pop one of each, the small keeps p_s and is aliased to the large, whose p becomes (p_l + p_s) - 1;
    leftovers keep their whole mass (alias = own item, thr = 0).  thr = max(1, floor(keep 2^32)) otherwise."""
    w = [float(x) for x in np.asarray(weights, np.float64)[1:]]
    V = len(w)
    total = math.fsum(w)
    p = [x * float(V) / total for x in w]
    small = [s for s in range(V) if p[s] < 1.0]
    large = [s for s in range(V) if not p[s] < 1.0]
    thr, alias = [0] * V, list(range(1, V + 1))
    while small and large:
        s, l = small.pop(), large.pop()
        thr[s] = max(1, int(math.floor(p[s] * 4294967296.0)))
        alias[s] = l + 1
        p[l] = (p[l] + p[s]) - 1.0
        (small if p[l] < 1.0 else large).append(l)
    return np.array(thr, np.uint32), np.array(alias, np.int64)


def unpack_table(table):
    """(thr, alias) of a packed table (int64 / uint64 [V]: thr | alias << 32)."""
    t = np.asarray(table).view(np.uint64)
    return (t & np.uint64(0xFFFFFFFF)).astype(np.uint32), (t >> np.uint64(32)).astype(np.int64)


def realised_counts_ref(thr, alias):
    """N(v), v = 1..V, as Python ints: thr[v - 1] + sum over {s: alias[s] = v} of (2^32 - thr[s])."""
    n = [int(t) for t in thr]
    for s, a in enumerate(alias):
        n[int(a) - 1] += (1 << 32) - int(thr[s])
    return n


def realised_q_ref(table):
    """Qhat [V + 1] (float64, entry 0 = 0) of a packed table: N(v) / (V 2^32), each quotient correctly rounded."""
    thr, alias = unpack_table(table)
    n = realised_counts_ref(thr, alias)
    V = len(n)
    return np.array([0.0] + [x / (V << 32) for x in n])


def table_bound(weights, alias):
    """Per item: (1 + indegree(v)) 2^-32 / V + 8 u64 (pmax + 2), the docstring's bound on |Qhat(v) - Q(v)|."""
    w = np.asarray(weights, np.float64)[1:]
    V = w.shape[0]
    own = alias == np.arange(1, V + 1)
    indeg = np.bincount(alias[~own] - 1, minlength=V)
    pmax = float(w.max()) * V / math.fsum(w.tolist())
    return (1 + indeg) * 2.0 ** -32 / V + 8 * U64 * (pmax + 2), indeg


def alias_items_ref(seed_base, salt, table, V, K):
    """The K draws of rs_alias_items for the step seed `seed_base` (the value AFTER the sampler advanced it)."""
    thr, alias = unpack_table(table)
    assert len(thr) == V
    seed = (salt ^ ((seed_base * 0xD1B54A32D192ED03) & base._M64)) & base._M64
    if K <= 4096:                                                  # Python integers: the rule as the header writes it
        out = np.empty(K, np.int64)
        for j in range(K):
            r = base._splitmix64((seed + 0x632BE59BD9B4E019 * (j + 1)) & base._M64)
            prod = r * V
            s, frac = prod >> 64, (prod & base._M64) >> 32
            out[j] = s + 1 if frac < int(thr[s]) else int(alias[s])
        return out
    # many draws: the same rule in wrapping uint64 arithmetic, the 128-bit product from 32-bit halves (V < 2^32)
    u64 = np.uint64
    with np.errstate(over="ignore"):
        z = u64(seed) + u64(0x632BE59BD9B4E019) * np.arange(1, K + 1, dtype=u64) + u64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> u64(30))) * u64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u64(27))) * u64(0x94D049BB133111EB)
        r = z ^ (z >> u64(31))
        mid = (r >> u64(32)) * u64(V) + (((r & u64(0xFFFFFFFF)) * u64(V)) >> u64(32))    # (r * V) >> 32, < V 2^32
    s, frac = (mid >> u64(32)).astype(np.int64), (mid & u64(0xFFFFFFFF)).astype(np.uint32)
    return np.where(frac < thr[s], s + 1, alias[s])
