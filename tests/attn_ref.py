"""float64 reference, per-element error bounds and a float32/bf16 emulation of the LDS-resident attention kernels
(attention_lds.hip: rs_attn_fwd / rs_attn_bwd, bf16, T <= 256, Dh 32/64/128).  Conventions as rowchain_ref.py.

Reference.  Plain torch float64 from the formulas in include/recsys_hip.h on the values as stored, per
(sequence, head), tensors [B*H][T][.]:
    s = scale q k^T;  causal: s = -inf for key > query;  key padding: s = -1e9 where ids[key] == 0
    lse = logsumexp(s);  p = exp(s - lse);  o = (p m) v            m: the kernels' own dropout multiplier
The backward is STAGED: it is fed the lse and the delta (ws) the kernels themselves stored, so a forward error is
not charged twice and a failure names its pass:
    p = exp(s - lse_stored);  dP = dO v^T;  dS = p (dP m - delta_stored) scale, exactly 0 on -inf and -1e9 scores
    dq = dS k;  dk = dS^T q;  dv = (p m)^T dO;   delta = rowsum(dO o_stored) is checked on its own

Bound (derived, not fitted), per element, for a bf16 output with float64 reference r:

    |hip - r| <= 2 * ( U8 |r| + U8 P + K U24 A + S )

  U8 |r|   the output's own rounding;
  P        absolute-value propagation of the unstored bf16 roundings: p m is packed to bf16 before the second MFMA
           (forward, dV), dS likewise (dQ, dK):  P = |p m| |v|,  |dS| |k|,  |dS|^T |q|,  |p m|^T |dO|.  Where the
           backward's work plan splits a dK/dV tile, the writer's partial sum (its query chunks) goes through an
           LDS slot in bf16: P gains the same sum restricted to the writer's queries (read from rs_attn_bwd_plan);
           the dQ slots are float32 and add nothing;
  K U24 A  float32 accumulation and elementwise operations; A = the same map on absolute values (for dS:
           p (|dO| |v|^T m + |delta|) scale, which covers dP's own Dh-long accumulation).  K, stated at each use,
           is the reduction length plus the elementwise float32 operations on the path;
  S        propagation of the exponent's error through exp: the weight of each (query, key) pair in P's map times
           rho = expm1(es) + ULP, where es is the absolute error of the exponent and ULP = 2^-23 is the 1 ulp of
           v_exp_f32 / v_log_f32 (the CDNA ISA's stated accuracy for both).  With As = scale |q| |k|^T:
             forward   es = U24 ((Dh + 3) As + |s - max_row s|)          Dh accumulations, scale*log2(e) (its own
                       rounding and the product's) and the multiply; then the subtraction of the row maximum.  A
                       filled score is the constant itself (As = 0): its error is common to the row and cancels
                       in the normalisation.  The normalisation adds the p-weighted row mean of rho (rbar);
             backward  es = U24 ((Dh + 3) As + |s - lse| + 2 |lse|)      the same, the subtraction of lse and the
                       product lse*log2(e) with its constant; a filled key has As = 1e9 with K = 1 (the constant's
                       rounding).
lse, delta and float32 outputs drop the U8 terms.  lse:  2 (rbar + U24 (n + 2 |lse - max| + 3 |lse|)), n = live keys
(the sum), the log's ulp, the add and the product with ln 2 and its constant.

Second tier (kind = "generic": attention.hip, float32 storage and the bf16 shapes the LDS path does not take).  The
same reference and bound; these kernels work in natural units with an online softmax over 32-key chunks and round
to bf16 the unnormalised exp(s - running max) m, dS and p m -- the same relative roundings, so P is unchanged (no
split tiles).  The exponent's error becomes  es = U24 ((Dh + 1) As + 3 |s - max| + 6 R)  in the forward (the
subtraction and the fast exp's product with log2 e and its constant; the running maximum lies up to R = max - first
chunk's live maximum below the final one, and the rescalings exp(old max - new max), whose exponents sum to R, cost
3 each), one ULP and 3 operations per chunk on top, and  es = U24 ((Dh + 1) As + 3 |s - lse|)  in the backward; the
-1e9 fill is the exact constant there.

A row whose keys are ALL padding has lse = -1e9 + ln T, which float32 stores as -1e9 (spacing 64): the backward's
p = exp(-1e9 - lse_stored) is then whatever the roundings of two numbers near 1.4e9 leave, es ~ 180 and the bound
on that sequence's dV says nothing (the kernels give p = 1 there where the exact softmax has 1/T: a property of
carrying the row statistic as one float32 logsumexp, shared with the generic kernels, noted in DESIGN.md).  What
is exact there is asserted exactly: dS = 0, so dq = dk = 0, and dv is finite and not zero.

Emulation.  The same passes in float32 in the kernels' log2 domain with a bf16 rounding at every point where the
kernels round, the split-tile partials from the real plan included: a correct kernel as far as the bound is
concerned.  `mut` injects the faults of tests/test_attn_ref.py.
"""
import ctypes as C
import functools
import math

import numpy as np
import torch

from rowchain_ref import D, U8, U24, kmul, rb

ULP = 2.0 * U24
GUARD = 32
NW, PLAN_S, PLAN_I = 8, 4, 6
LOG2E = float(np.float32(1.4426950408889634))
LN2 = float(np.float32(0.6931471805599453))
MASK2 = float(np.float32(-1e9) * np.float32(LOG2E))
FILL = -1e9

# The shape matrix: (purpose, (B, H, Dh, T), mask kinds, (forward nsplit, backward nsplit, causal plan used)) -- the
# regime each row is there for, asserted against rs_attn_lds_regime (key padding: the same splits, never a plan).
# (3, 8, 64, 255) has B*H = 24, which pick_split_bwd gives 4 workgroups, not 2: it is the swizzled nsplit-4 plan.
SHAPES = [
    ("plan ns1, bench shape", (65, 1, 128, 200), (0, 1), (2, 1, 1)),
    ("plan ns1, BH % 8 == 0; key padding: round robin second item", (9, 8, 32, 200), (0, 1), (2, 1, 1)),
    ("plan ns1", (11, 7, 32, 200), (0, 1), (2, 1, 1)),
    ("plan ns2 swizzled", (8, 1, 128, 200), (0, 1), (2, 2, 1)),
    ("plan ns4 swizzled", (3, 8, 64, 255), (0, 1), (4, 4, 1)),
    ("plan ns4", (2, 4, 64, 256), (0, 1), (4, 4, 1)),
    ("plan ns4", (3, 1, 32, 241), (0, 1), (4, 4, 1)),
    ("boundary: 7 tiles, no plan", (9, 8, 32, 112), (0, 1), (1, 1, 0)),
    ("boundary: 8 tiles, plan", (9, 8, 32, 113), (0, 1), (2, 1, 1)),
    ("boundary: Dh 128 plan fits LDS", (65, 1, 128, 224), (0, 1), (2, 1, 1)),
    ("boundary: Dh 128 plan does not fit", (65, 1, 128, 225), (0, 1), (2, 1, 0)),
    ("round robin second item, causal", (72, 1, 128, 240), (0,), (2, 1, 0)),
    ("forward two tiles per wave", (32, 8, 32, 144), (0, 1), (1, 1, 1)),
    ("forward two tiles per wave", (37, 7, 32, 255), (0, 1), (1, 1, 1)),
    ("forward ns4 at 16 tiles", (3, 1, 64, 256), (0, 1), (4, 4, 1)),
    ("forward ns2 at 16 tiles", (16, 8, 32, 256), (0, 1), (2, 1, 1)),
] + [("edge", (3, 2, 64, T), (0, 1), (1, 1, 0)) for T in (1, 15, 16, 17, 31, 33)]
# key-padding cases with sequence 1's ids all 0: (B, H, Dh, T)
ALL_PAD = [(9, 8, 32, 200), (3, 2, 64, 37)]
# second tier: float32 mode (generic kernels) and the generic bf16 kernels, (B, H, Dh, T, mask kind, all-padding)
TIER2_F32 = [(3, 2, 64, 37, 1, True), (3, 2, 64, 33, 0, False), (8, 1, 128, 200, 0, False)]
TIER2_BF16 = [(2, 1, 50, 200, 0, False), (1, 2, 64, 300, 1, False), (2, 3, 100, 40, 0, False),
              (2, 3, 100, 40, 1, False)]


def expected_regime(c, want):
    plan = int(want[2] and c.mask_kind == 0)
    return (1, want[0], want[1], plan, plan)


def assert_regime(c, purpose, want):
    """the case runs the code it is there for (rs_attn_lds_regime calls the launchers' own host functions)"""
    reg = regime(c)
    assert reg == expected_regime(c, want), (purpose, reg, want)
    _, fwd_ns, bwd_ns, plan_q, _ = reg
    if purpose.startswith("forward two tiles"):          # a wave of the forward takes a second tile
        assert c.BH >= 256 and c.nq > NW * fwd_ns
    if "second item" in purpose and not plan_q:          # a wave of the round-robin backward takes a second tile
        assert c.nq > NW * bwd_ns
    if purpose.startswith("plan ns1") and plan_q:        # both roles in each pass, and a wave with >= 3 items
        most = 0
        for dkv in (False, True):
            items, ns = plan_items(c.B, c.T, c.H, dkv)
            assert ns == 1 and {1, 2} <= {it[6] for it in items}
            most = max([most] + [sum(1 for it in items if it[1] == w) for w in range(NW)])
        assert most >= 3, most


class Case:
    def __init__(self, B, H, Dh, T, mask_kind):
        self.B, self.H, self.Dh, self.T, self.mask_kind = B, H, Dh, T, mask_kind
        self.BH, self.M, self.d, self.Tp = B * H, B * T, H * Dh, T + (T & 1)
        self.scale = float(np.float32(1.0 / math.sqrt(Dh)))
        self.nq = -(-T // 16)


# ------------------------------------------------------------------ the host's regime and plan
def regime(c, dtype=1):
    """(LDS path, forward nsplit, backward nsplit, dQ plan, dK/dV plan) of rs_attn_lds_regime (dtype 1 = bf16)"""
    import rbm_amd._lib as L
    out = (C.c_int * 5)()
    rc = L.lib().rs_attn_lds_regime(dtype, c.B, c.T, c.H, c.Dh, c.mask_kind, out)
    assert rc == 0, rc
    return tuple(out)


@functools.lru_cache(maxsize=None)
def plan_items(B, T, H, dkv):
    """[(split, wave, item index, tile, chunk begin, chunk end, role, slot)] of rs_attn_bwd_plan, and nsplit"""
    import rbm_amd._lib as L
    buf = (C.c_uint32 * (PLAN_S * NW * PLAN_I))()
    ns = C.c_int()
    rc = L.lib().rs_attn_bwd_plan(B, T, H, int(dkv), buf, C.byref(ns))
    assert rc == 0, rc
    p = np.frombuffer(buf, dtype=np.uint32).reshape(PLAN_S, NW, PLAN_I)
    items = []
    for sp in range(ns.value):
        for w in range(NW):
            for it in range(PLAN_I):
                e = int(p[sp, w, it])
                if e >> 31:
                    items.append((sp, w, it, e & 255, (e >> 8) & 255, (e >> 16) & 255, (e >> 24) & 3, (e >> 26) & 15))
    return items, ns.value


def writer_pairs(c, dkv, dev="cpu"):
    """bool [T queries][T keys]: the (query, key) pairs whose contribution passes through a writer's LDS slot, for the
    dK/dV pass (dkv: key tiles, 32-query chunks) or the dQ pass (query tiles, 32-key chunks); None without a plan"""
    if not regime(c)[4 if dkv else 3]:
        return None
    T = c.T
    W = torch.zeros(T, T, dtype=torch.bool)
    for _, _, _, tile, cb, ce, role, _ in plan_items(c.B, T, c.H, dkv)[0]:
        if role == 1:
            if dkv:
                W[32 * cb:32 * ce, 16 * tile:16 * tile + 16] = True
            else:
                W[16 * tile:16 * tile + 16, 32 * cb:32 * ce] = True
    return W.to(dev)


def block_coords(BH, ns, lin, swizzled):
    """model of attention_lds.hip block_coords: (sequence-head, split) of workgroup lin; swizzled: the BH % 8 == 0
    branch, which deals the sequence-heads to the 8 XCDs"""
    if swizzled:
        xcd, slot = lin & 7, lin >> 3
        return xcd * (BH >> 3) + slot // ns, slot % ns
    return lin // ns, lin % ns


def plan_role(c, dkv, tile):
    """'round robin', 'whole' or 'split' for a tile of the pass"""
    if not regime(c)[4 if dkv else 3]:
        return "round robin"
    roles = {r for _, _, _, t, _, _, r, _ in plan_items(c.B, c.T, c.H, dkv)[0] if t == tile}
    return "split" if roles & {1, 2} else "whole"


# ------------------------------------------------------------------ inputs
def heads(x, c):
    return x.reshape(c.B, c.T, c.H, -1).permute(0, 2, 1, 3).reshape(c.BH, c.T, -1)


def unheads(x, c):
    return x.reshape(c.B, c.H, c.T, -1).permute(0, 2, 1, 3).reshape(c.M, -1)


def make_inputs(c, dev="cpu", seed=0, all_pad=False, dtype=torch.bfloat16):
    """bf16 q [M][d], kv [M][2d], dO [M][d] and ids [B][T].  q is scaled so that the scores have a standard deviation
    near 2 (a softmax that is not near-uniform), dO carries a per-feature mean so that delta does not cancel, the
    ids pad left by a different length per sequence; all_pad: sequence 1's ids are all 0."""
    gen = torch.Generator(device=dev).manual_seed(seed * 1000003 + c.M * 131 + c.d + c.mask_kind)
    f32 = torch.float32

    def rn(*shape, s=1.0):
        return torch.randn(*shape, generator=gen, device=dev, dtype=f32) * s

    cols = torch.arange(c.d, device=dev, dtype=f32)[None, :]
    inp = {"q": (rn(c.M, c.d, s=2.0)).to(dtype), "kv": rn(c.M, 2 * c.d).to(dtype),
           "do": (rn(c.M, c.d) + 0.7 * torch.cos(0.7 * cols)).to(dtype)}
    ids = torch.randint(1, 50, (c.B, c.T), generator=gen, device=dev)
    for b in range(c.B):
        ids[b, :(b * c.T) // (c.B + 1)] = 0
    if all_pad:
        ids[1] = 0
    inp["ids"] = ids
    return inp


def random_mult(c, p, dev="cpu", seed=1, pitch=None):
    """a dropout multiplier [BH][T][T] (0 or 1/(1-p)) read from a flat keep array at ((bh T + q) pitch + k), as the
    kernels index their hash; pitch defaults to the even Tp"""
    if p <= 0:
        return torch.ones(c.BH, c.T, c.T, device=dev)
    gen = torch.Generator().manual_seed(seed)
    flat = (torch.rand(c.BH * c.T * c.Tp + c.T, generator=gen) >= p).float() * kmul(p)
    pitch = pitch or c.Tp
    idx = (torch.arange(c.BH * c.T)[:, None] * pitch + torch.arange(c.T)[None, :]).view(c.BH, c.T, c.T)
    return flat[idx].to(dev)


def masks(c, ids, dev):
    """dead [BH or 1][T][T] (-inf scores), fill [BH or 1][1][T] (-1e9 scores)"""
    T = c.T
    if c.mask_kind == 0:
        r = torch.arange(T, device=dev)
        return (r[None, :] > r[:, None])[None], torch.zeros(1, 1, T, dtype=torch.bool, device=dev)
    fill = (ids == 0).view(c.B, 1, 1, T).expand(c.B, c.H, 1, T).reshape(c.BH, 1, T)
    return torch.zeros(1, T, T, dtype=torch.bool, device=dev), fill


# ------------------------------------------------------------------ float64 reference and bounds
def _scores(c, inp):
    dev = inp["q"].device
    q, k = D(heads(inp["q"], c)), D(heads(inp["kv"][:, :c.d], c))
    dead, fill = masks(c, inp["ids"], dev)
    s = c.scale * (q @ k.transpose(1, 2))
    As = c.scale * (q.abs() @ k.abs().transpose(1, 2))
    s = s.masked_fill(fill, FILL).masked_fill(dead, -math.inf)
    return s, As, dead, fill


def ref_fwd(c, inp, m):
    """the forward in float64, head-major [BH][T][.]: lse [BH][T][1], p, pm = p m, o (and the operands)"""
    s, As, dead, fill = _scores(c, inp)
    v, m = D(heads(inp["kv"][:, c.d:], c)), D(m)
    lse = torch.logsumexp(s, -1, keepdim=True)
    p = torch.exp(s - lse)
    return {"s": s, "As": As, "dead": dead, "fill": fill, "v": v, "m": m, "lse": lse, "p": p, "pm": p * m,
            "o": (p * m) @ v}


def ref_bwd(c, inp, m, lse, delta):
    """the staged backward in float64 from a given lse and delta (both [BH*T]), head-major: dS, dq, dk, dv"""
    s, As, dead, fill = _scores(c, inp)
    q, k, v = (D(heads(t, c)) for t in (inp["q"], inp["kv"][:, :c.d], inp["kv"][:, c.d:]))
    dO, m = D(heads(inp["do"], c)), D(m)
    lse, delta = D(lse).reshape(c.BH, c.T, 1), D(delta).reshape(c.BH, c.T, 1)
    p = torch.exp(s - lse)
    dS = (p * ((dO @ v.transpose(1, 2)) * m - delta) * c.scale).masked_fill(dead | fill, 0.0)
    return {"s": s, "As": As, "dead": dead, "fill": fill, "q": q, "k": k, "v": v, "dO": dO, "m": m, "lse": lse,
            "delta": delta, "p": p, "dS": dS, "dq": dS @ k, "dk": dS.transpose(1, 2) @ q,
            "dv": (p * m).transpose(1, 2) @ dO}


def _rho(es, dead):
    return torch.where(dead, torch.zeros_like(es), torch.expm1(es.clamp(max=700.0)) + ULP)


def _bound(r, P, A, K, S, bf16=True):
    return 2.0 * ((U8 * (r.abs() + P) if bf16 else 0.0) + K * U24 * A + S)


def worst(hip, r, bound):
    """(worst err / bound, its flat index): 0 where err is 0, inf for a NaN or an error at a zero bound"""
    err = (D(hip) - r).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    i = int(q.argmax())
    return float(q.reshape(-1)[i]), i


def _nch(c):
    return -(-c.T // 32)


def check_fwd(c, inp, m, out, kind="lds", bf16=True):
    """{name: (ratio, flat index)} for o [M][d] and lse [BH*T] of the forward (kind: "lds" or "generic" kernels)"""
    ref = ref_fwd(c, inp, m)
    s, As, dead, fill, v, m, lse, p = (ref[n] for n in ("s", "As", "dead", "fill", "v", "m", "lse", "p"))
    smax = s.max(-1, keepdim=True).values
    # the exponent's error: Dh accumulations + 3 (see the module docstring), then the subtraction of the maximum
    if kind == "lds":
        es, kx = U24 * ((c.Dh + 3) * As.masked_fill(fill, 0.0) + (s - smax).abs()), 0
    else:
        # generic kernels (online softmax over 32-key chunks): Dh accumulations and the scale; 3 |s - running max|
        # (the subtraction, and the fast exp's product with log2 e and its constant), the running maximum lying
        # up to R = max - (first chunk's max) below the final one; the rescalings exp(old max - new max), whose
        # exponents sum to R, at 3 each; one ULP per chunk's rescaling (in rho) and 3 operations per chunk (in K)
        # (R counts the rises among live scores only: exp(-1e9 - a live maximum) is exactly 0)
        cm = torch.nn.functional.pad(s.masked_fill(fill, -math.inf), (0, -c.T % 32), value=-math.inf)
        cm = cm.view(s.shape[0], c.T, -1, 32).max(-1).values
        first = cm.gather(-1, (cm > -math.inf).double().argmax(-1, keepdim=True))
        R = torch.where(first > -math.inf, smax - first, torch.zeros_like(first))
        es, kx = U24 * ((c.Dh + 1) * As.masked_fill(fill, 0.0) + 3 * (s - smax).abs() + 6 * R), _nch(c)
    rho = _rho(es, dead) + kx * ULP * D(~dead)
    rbar = (p * rho).sum(-1, keepdim=True)
    n = (~dead).sum(-1, keepdim=True).double().expand(s.shape[0], -1, -1)
    res = {"lse": worst(out["lse"].view(c.BH, c.T, 1), lse,
                        2.0 * (rbar + U24 * (n + 3 * kx + 2 * (lse - smax).abs() + 3 * lse.abs())))}
    pm, o = ref["pm"], ref["o"]
    Ao = pm @ v.abs()
    # K = 2 n + 6: the accumulation over the keys, the row sum's own n additions, the reciprocal (2: 1 ulp), the
    # products with it and with the dropout multiplier, the multiplier's own rounding
    S = (pm * (rho + rbar)) @ v.abs()
    res["o"] = worst(heads(out["o"], c), o, _bound(o, Ao, Ao, 2 * n + 6 + 3 * kx, S, bf16))
    return res


def check_bwd(c, inp, m, lse_st, delta_st, out, o_st=None, kind="lds", bf16=True):
    """{name: (ratio, flat index)} for dq [M][d], dkv [M][2d] and (o_st given: the kernels formed delta) delta [BH*T],
    staged on the stored lse and delta (both [BH*T])"""
    dev = inp["q"].device
    ref = ref_bwd(c, inp, m, lse_st, delta_st)
    s, As, dead, fill, q, k, v, dO, m, lse, delta, p, dS = (ref[n] for n in (
        "s", "As", "dead", "fill", "q", "k", "v", "dO", "m", "lse", "delta", "p", "dS"))
    res = {}
    if o_st is not None:
        t = dO * D(heads(o_st, c))
        # K = Dh + 2: the fma chain over the head's columns and the two cross-lane additions
        res["delta"] = worst(delta, t.sum(-1, keepdim=True), _bound(0, 0, t.abs().sum(-1, keepdim=True), c.Dh + 2, 0, False))
    AdP = dO.abs() @ v.abs().transpose(1, 2)
    AdS = (p * (AdP * m + delta.abs()) * c.scale).masked_fill(dead | fill, 0.0)
    if kind == "lds":
        Kmat = (c.Dh + 3) - (c.Dh + 2) * D(fill)
        es = U24 * (Kmat * As.masked_fill(fill, -FILL) + (s - lse).abs() + 2 * lse.abs())
    else:   # generic kernels: natural units, the fill is the exact constant; 3 |s - lse| as in the forward
        es = U24 * ((c.Dh + 1) * As.masked_fill(fill, 0.0) + 3 * (s - lse).abs())
    rho = _rho(es, dead)
    n = float(c.T)
    aS = dS.abs()
    # dq: K = T + Dh + 6: the accumulation over the keys, dP's over Dh (in A), and dS's elementwise operations
    r = dS @ k
    res["dq"] = worst(heads(out["dq"], c), r, _bound(r, aS @ k.abs(), AdS @ k.abs(), n + c.Dh + 6, (aS * rho) @ k.abs(), bf16))
    W = writer_pairs(c, True, dev) if kind == "lds" else None
    Wd = D(W)[None] if W is not None else None
    r = dS.transpose(1, 2) @ q
    P = aS.transpose(1, 2) @ q.abs()
    if W is not None:                                # the writer's partial, rounded to bf16 in the slot
        P = P + (aS * Wd).transpose(1, 2) @ q.abs()
    res["dk"] = worst(heads(out["dkv"][:, :c.d], c), r,
                      _bound(r, P, AdS.transpose(1, 2) @ q.abs(), n + c.Dh + 6, (aS * rho).transpose(1, 2) @ q.abs(), bf16))
    pm = p * m
    r = pm.transpose(1, 2) @ dO
    A = pm.transpose(1, 2) @ dO.abs()
    P = A + ((pm * Wd).transpose(1, 2) @ dO.abs() if W is not None else 0.0)
    # dv: K = T + 4: the accumulation over the queries, the product with the multiplier and its own rounding
    res["dv"] = worst(heads(out["dkv"][:, c.d:], c), r, _bound(r, P, A, n + 4, (pm * rho).transpose(1, 2) @ dO.abs(), bf16))
    return res


def where(c, name, i):
    """(b, h, row, column) of flat index i of the head-major view of output `name`, its tile and plan role"""
    w = 1 if name in ("lse", "delta") else c.Dh
    bh, row, col = i // (c.T * w), (i // w) % c.T, i % w
    role = plan_role(c, name in ("dk", "dv"), row // 16) if name in ("dq", "dk", "dv") else "-"
    return f"{name}: b {bh // c.H} h {bh % c.H} row {row} col {col} tile {row // 16} plan role {role}"


# ------------------------------------------------------------------ float32 / bf16 emulation of the kernels
def _f(t):
    return t.float()


def _score2(c, inp, mut, key):
    """log2-domain scores as the kernels form them, with dead / fill masks (mut[key]: a changed dead mask)"""
    q, k = _f(heads(inp["q"], c)), _f(heads(inp["kv"][:, :c.d], c))
    dead, fill = masks(c, inp["ids"], "cpu")
    dead = dead.expand(c.BH, -1, -1)
    if key in mut:
        dead = mut[key](dead.clone())
    sl2 = np.float32(c.scale) * np.float32(LOG2E)
    s2 = (q @ k.transpose(1, 2)) * sl2
    return s2, dead, fill


def emu_fwd(c, inp, m, mut={}):
    s2, dead, fill = _score2(c, inp, mut, "dead_fwd")
    v = _f(heads(inp["kv"][:, c.d:], c))
    m = _f(m)
    if mut.get("extra_keys"):       # keys past T (the staged copies of row T - 1) left unmasked
        nx = -c.T % 16
        s2 = torch.cat([s2, s2[:, :, -1:].expand(-1, -1, nx)], 2)
        v = torch.cat([v, v[:, -1:].expand(-1, nx, -1)], 1)
        m = torch.cat([m, m[:, :, -1:].expand(-1, -1, nx)], 2)
        dead = torch.cat([dead, dead[:, :, -1:].expand(-1, -1, nx)], 2)
        fill = torch.cat([fill, torch.zeros(fill.shape[0], 1, nx, dtype=torch.bool)], 2)
    s2 = s2.masked_fill(fill, MASK2).masked_fill(dead, -math.inf)
    mx = s2.max(-1, keepdim=True).values
    e = torch.exp2(s2 - mx)
    sm = e.sum(-1, keepdim=True)
    lse = (mx + torch.log2(sm)) * np.float32(LN2)
    if mut.get("lse_log2"):
        lse = mx + torch.log2(sm)
    o = (rb(e * (1.0 / sm) * m) @ v).bfloat16()
    o, lse = unheads(o, c), lse.reshape(-1).clone()
    for bh, tile in mut.get("skip_fwd", ()):          # tiles a wave never ran: the outputs keep their prefill
        rows = slice(16 * tile, 16 * tile + 16)
        ov = o.view(c.B, c.T, c.H, c.Dh)
        ov[bh // c.H, rows, bh % c.H] = math.nan
        lse.view(c.BH, c.T)[bh, rows] = math.nan
    return {"o": o, "lse": lse}


def emu_bwd(c, inp, m, lse, delta=None, o=None, mut={}):
    """delta given: as RS_ATTN_DELTA_IN; else formed from o.  Returns dq, dkv (and delta when formed here)"""
    q, k, v = (_f(heads(t, c)) for t in (inp["q"], inp["kv"][:, :c.d], inp["kv"][:, c.d:]))
    dO, m = _f(heads(inp["do"], c)), _f(m)
    out = {}
    if delta is None:
        delta = (dO * _f(heads(o, c))).sum(-1).reshape(-1)
        out["delta"] = delta.clone()
    lse, dl = lse.view(c.BH, c.T, 1), delta.view(c.BH, c.T, 1)
    if "row_perm" in mut:                              # lse / delta rows taken from another head
        which, perm = mut["row_perm"]
        if which == "lse":
            lse = lse[perm]
        else:
            dl = dl[perm]
    lq2 = lse * np.float32(LOG2E)
    sc = np.float32(c.scale)
    dP = dO @ v.transpose(1, 2)
    # dQ pass: P from the scores alone, dS zeroed wherever the score is not live
    s2, dead, fill = _score2(c, inp, mut, "dead_dq")
    live = ~(dead | fill)
    if mut.get("ds_fill"):                            # dS kept on -1e9 scores (P from the fill)
        live = ~dead
        s2 = s2.masked_fill(fill, MASK2)
    ds = torch.where(live, torch.exp2(s2 - lq2) * sc * (dP * m - dl), torch.zeros(()))
    if "skip_dq" in mut:
        ds = ds.masked_fill(mut["skip_dq"], 0.0)
    dq = unheads((rb(ds) @ k).bfloat16(), c)
    # dK/dV pass: P also on filled keys (from the fill), dS zeroed on dead and filled scores
    s2, dead, fill = _score2(c, inp, mut, "dead_dkv")
    p = torch.exp2(s2.masked_fill(fill, MASK2).masked_fill(dead, -math.inf) - lq2)
    ds = torch.where(dead | fill, torch.zeros(()), p * (dP * m - dl) * sc)
    pd = p * m
    if "skip_dkv" in mut:
        ds, pd = ds.masked_fill(mut["skip_dkv"], 0.0), pd.masked_fill(mut["skip_dkv"], 0.0)
    ds, pd = rb(ds), rb(pd)
    W = writer_pairs(c, True)
    if W is None:
        dk, dv = ds.transpose(1, 2) @ q, pd.transpose(1, 2) @ dO
    else:                                              # the writer's partial passes through a bf16 slot
        Wf = W.float()[None]
        dk = rb((ds * Wf).transpose(1, 2) @ q) + (ds * (1 - Wf)).transpose(1, 2) @ q
        dv = rb((pd * Wf).transpose(1, 2) @ dO) + (pd * (1 - Wf)).transpose(1, 2) @ dO
    dkv = torch.cat([unheads(dk.bfloat16(), c), unheads(dv.bfloat16(), c)], 1).contiguous()
    for name, t in (("skip_dq_tile", dq), ("skip_dkv_tile", dkv)):
        for bh, tile in mut.get(name, ()):
            tv = t.view(c.B, c.T, -1, c.Dh)
            for h in ((bh % c.H,) if t is dq else (bh % c.H, c.H + bh % c.H)):
                tv[bh // c.H, 16 * tile:16 * tile + 16, h] = math.nan
    out.update(dq=dq, dkv=dkv)
    return out
