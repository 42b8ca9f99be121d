"""float64 reference, error bounds and a float32 emulation of the gradient tail every SASRec / BERT4Rec step ends in:
the grouped weight-gradient launch and its grouped segment reduction (wgrad.hip), the fused rs_wgrad_grouped_pos /
_pos_stats launch (grad_tail.hip), rs_reduce_slabs(2) (reduce.hip), rs_colsum (misc.hip) and the split-K
rs_linear_wgrad (gemm.hip).

Reference.  One plain torch float64 function per entry point, written from include/recsys_hip.h: dW0 + dY^T X,
db0 + colsum(dY), out0 + sum_z src[z].  The positional gradient and the head statistics reuse losshead_ref's
references.  The operands are the bf16 values the kernels read; bf16 x bf16 is exact in float32, so the reference
shares no rounding with the kernels (the float32 forms of rs_linear_wgrad / rs_colsum round each product once: inside
the factor-four slack of bound_f32 at the same K).

Bounds (derived, not fitted): rowchain_ref.bound_f32(A, K) = 2 * 2 K 2^-24 A with A the same map on absolute values
(|dY|^T |X| + |dW0|, sum |src| + |out0|) and K the float32 additions on the longest path, stated at every use:
    a weight or bias element    rows of the problem + splits + 1 (the rows in any grouping, the splits, the old value)
    a reduced element           splits + 1
    rs_colsum                   rows + blocks + 1
No tolerance constant appears.

Operands are column slices of wider NaN-filled buffers (operand(): pitch > width, NaN rows after row M), outputs are
losshead_ref.Guarded: an over-read shows as a NaN in the result, a stray store in the guards.

Emulation.  Each kernel's summation structure in float32 (row splits; 64-row stages, 32-row ones for the 256 tile and
the generic GEMM; the reductions' split groups and tree; the positional body's batch groups), each with `mut`
switches that plant one specific mistake.  tests/test_gradtail_ref.py holds the emulation to the bounds on the CPU at
every shape of the GPU lists below and checks that every mutation is rejected at the smallest listed shape that
exercises it.
"""
import math

import numpy as np
import torch

import losshead_ref as L
from losshead_ref import BF, F32, check_embed_bwd, check_head_stats, gen_for, rn  # noqa: F401 (re-exported)
from rowchain_ref import D, GUARD, bound_f32, kmul, ratio

NAN = math.nan

# ------------------------------------------------------------------ the shape lists of the GPU tests
# grouped launch: the problem set (N, K) of each tile edge, and (set, max_tile) of every launch form
GROUP_SETS = {64: [(64, 64), (128, 64), (64, 192)], 128: [(128, 128), (256, 128)],
              256: [(256, 256), (512, 256), (256, 512)]}
GROUP_FORMS = [(64, 256), (128, 256), (256, 256), (256, 128), (256, 64)]
# (M, rows_per_split): checked loop only; ring nk = 1; a second split of one row; ring nk even / odd; an interior
# split + a ragged one; five splits
GROUP_ROWS = [(1, 64), (63, 64), (64, 64), (65, 64), (128, 128), (192, 192), (209, 128), (320, 64)]
# the 256 tile alone: fewer 32-row stages than the prefetch distance; tails of 31 rows, none, 1 row
GROUP_ROWS_256 = [(31, 64), (32, 64), (33, 64)]
EXTRA_SPLITS, EXTRA_N = 37, 64                              # the segment pair that rides along (tree, C = 16)

# segment reduction: form -> (split counts, lengths)
SEG_FORMS = {"col": ((1, 2, 3, 4, 5, 8, 31, 32), (4, 1020, 1024, 1028)),
             "four": ((1, 2, 3, 4), (65536, 65536 + 4, 65536 + 4 * 1023)),
             "tree16": ((33, 48, 49, 64), (4, 60, 68)),
             "tree4": ((65, 192, 193, 257, 400), (4, 60, 68))}
SLABS_N, SLABS_SPLITS = (4, 64, 68, 1024, 1028, 4100), (1, 4, 13, 25, 29, 49)
SLABS_SCALAR = (50, 6)                                      # n, n0 of the scalar kernel (+ an output off by a float)
FUSED_D, FUSED_T, FUSED_B, FUSED_P, FUSED_HB = (64, 128), (1, 3), (1, 15, 16, 17, 16 * 8 + 3), (0.0, 0.2), (1, 3, 257)
POS_RG_FUSED, POS_RG_ALONE = 16, 32                         # batch groups: embed_pos_body<bf16, 16, 256> / <16, 512>
LN_SETS = 5                                                 # rows of each LayerNorm partial set part[b][2][d]
LW_FORMS = [(BF, 64, 64, False), (BF, 130, 64, False), (BF, 64, 50, True), (F32, 64, 64, False), (F32, 50, 50, True)]
LW_M, LW_SPLITS, LW_ROWS_DEV = (1, 63, 65, 257), (1, 2, 3), (None, 0, 1, 64, 65)
COLSUM_N, COLSUM_M = (64, 128, 256, 50, 520), (1, 63, 65, 130, 4033, 4100)


def cdiv(a, b):
    return -(-a // b)


def operand(gen, dev, M, w, dt=BF, s=1.0, unaligned=False, live=None):
    """[M, w] random values as a column slice (offset 8) of a NaN-filled buffer of GUARD more rows; the pitch is a
    multiple of 8 elements past the slice (unaligned: w + 16 with w no multiple of 8: neither is the pitch); rows
    [live, M) NaN as well (the rows a device-side row count excludes)"""
    pitch = w + 16 if unaligned else cdiv(w, 8) * 8 + 16
    assert (pitch % 8 != 0) == unaligned and pitch > w + 8
    buf = torch.full((M + GUARD, pitch), NAN, dtype=dt, device=dev)
    buf[:M, 8:8 + w] = rn(gen, dev, M, w, s=s, dt=dt)
    if live is not None:
        buf[live:M, 8:8 + w] = NAN
    return buf[:M, 8:8 + w]


def one_more_row(t):
    """the operand with the (NaN) row at index M of its buffer"""
    return t.as_strided((t.shape[0] + 1, t.shape[1]), t.stride(), t.storage_offset())


def problem(gen, dev, M, N, K, dt=BF, bias=True, unaligned=False, live=None):
    return {"N": N, "K": K, "dY": operand(gen, dev, M, N, dt, 0.5, unaligned and N % 8 != 0, live),
            "X": operand(gen, dev, M, K, dt, 1.0, unaligned and K % 8 != 0, live), "dW0": rn(gen, dev, N, K),
            "db0": rn(gen, dev, N) if bias else None}


def group_inputs(shapes, M, dev):
    """the problems of one grouped launch (the last without a bias) and the extra segment pair"""
    g = gen_for(dev, 41, M, len(shapes), shapes[0][0])
    probs = [problem(g, dev, M, N, K, bias=i + 1 < len(shapes)) for i, (N, K) in enumerate(shapes)]
    part = rn(g, dev, EXTRA_SPLITS, 2, EXTRA_N)
    return probs, {"part": part, "out0": [rn(g, dev, EXTRA_N), rn(g, dev, EXTRA_N)]}


def extra_rows(extra, i):
    return extra["part"][:, i]


def seg_inputs(splits, n, dev, stride=None):
    """one reduce segment: `splits` rows of n floats at a stride of n + 8 in a NaN-filled buffer"""
    stride = stride or n + 8
    g = gen_for(dev, 47, splits, n)
    rows = rn(g, dev, splits, n)
    buf = torch.full((splits * stride,), NAN, device=dev)
    buf.view(splits, stride)[:, :n] = rows
    return {"src": buf, "stride": stride, "splits": splits, "n": n, "rows": rows, "out0": rn(g, dev, n)}


def lw_inputs(dt, N, K, unaligned, M, rows_dev, bias, dev):
    """one rs_linear_wgrad problem; with a device row count the rows from it on are NaN"""
    g = gen_for(dev, 53, N, K, M, -1 if rows_dev is None else rows_dev, int(bias))
    return problem(g, dev, M, N, K, dt, bias, unaligned, None if rows_dev is None else min(M, rows_dev))


# ====================================================================== reference and bounds
def ref_wgrad(p, rows, accumulate=True):
    """((dW, |.|), (db, |.|) or None) in float64 over the first `rows` rows"""
    y, x = D(p["dY"][:rows]), D(p["X"][:rows])
    w0 = D(p["dW0"]) if accumulate else torch.zeros_like(D(p["dW0"]))
    W = (w0 + y.t() @ x, w0.abs() + y.abs().t() @ x.abs())
    if p["db0"] is None:
        return W, None
    b0 = D(p["db0"]) if accumulate else torch.zeros_like(D(p["db0"]))
    return W, (b0 + y.sum(0), b0.abs() + y.abs().sum(0))


def wgrad_bounds(p, rows, splits, accumulate=True):
    """K = rows + splits + 1: the rows' products added in any grouping, the split partials, the old value"""
    W, b = ref_wgrad(p, rows, accumulate)
    K = rows + splits + 1
    return (W[0], bound_f32(W[1], K)), (None if b is None else (b[0], bound_f32(b[1], K)))


def check_wgrad(p, rows, splits, dW, db, accumulate=True, tag=""):
    (rW, bW), b = wgrad_bounds(p, rows, splits, accumulate)
    res = {tag + "dW": ratio(dW, rW, bW)}
    if b is not None:
        res[tag + "db"] = ratio(db, *b)
    return res


def cross_wgrad(p, rows, splits, a, b, tag=""):
    """two launch forms on the same inputs: apart by at most the sum of their two (equal) bounds"""
    (_, bW), bb = wgrad_bounds(p, rows, splits)
    res = {tag + "dW": ratio(a[0], D(b[0]), 2 * bW)}
    if bb is not None:
        res[tag + "db"] = ratio(a[1], D(b[1]), 2 * bb[1])
    return res


def check_reduce(rows, out0, accumulate, hip):
    """rows [splits][n]: out0 + sum_z rows[z]; K = splits + 1 (the splits in any grouping, the old value)"""
    r, A = D(rows).sum(0), D(rows).abs().sum(0)
    if accumulate:
        r, A = r + D(out0), A + D(out0).abs()
    return ratio(hip, r, bound_f32(A, rows.shape[0] + 1))


def colsum_blocks(M):
    return min(64, cdiv(M, 64))


def check_colsum(X, out0, accumulate, hip):
    """K = rows + blocks + 1: a block's rows in any grouping, the block partials, the old value"""
    r, A = D(X).sum(0), D(X).abs().sum(0)
    if accumulate:
        r, A = r + D(out0), A + D(out0).abs()
    return ratio(hip, r, bound_f32(A, X.shape[0] + colsum_blocks(X.shape[0]) + 1))


# ====================================================================== emulation: the grouped launch
def emu_partials(p, M, per_split, stage, splits, limit=None, mut=None):
    """slab [splits][N K + N] of one problem: each split's rows in stages of `stage` rows, the stage products added
    to the accumulator in row order.  limit: the device-side row count.  mut: 'droplast' the last row of a ragged
    split is not read; 'readM' the last split reads the row at index M; 'emptynan' an empty split writes nothing"""
    N, K = p["N"], p["K"]
    y, x = one_more_row(p["dY"]).float(), one_more_row(p["X"]).float()
    end = M if limit is None else min(M, limit)
    slab = torch.zeros(splits, N * K + N)
    for s in range(splits):
        kb = s * per_split
        ke = min(end, kb + per_split)
        if ke <= kb:
            if mut == "emptynan":
                slab[s] = NAN
            continue
        if mut == "droplast" and (ke - kb) % 64:
            ke -= 1
        if mut == "readM" and ke == M:
            ke += 1
        aw, ab = torch.zeros(N, K), torch.zeros(N)
        for k0 in range(kb, ke, stage):
            k1 = min(ke, k0 + stage)
            aw += y[k0:k1].t() @ x[k0:k1]
            ab += y[k0:k1].sum(0)
        slab[s, :N * K], slab[s, N * K:] = aw.reshape(-1), ab
    return slab


def seg_form(splits, n):
    """reduce_args' choice: column per thread up to 32 splits (four columns for large segments of at most 4
    splits), else split groups + LDS tree with C = 16 columns (G = 16 groups) or, past 64 splits, C = 4 (G = 64)"""
    if splits > 32:
        return "tree4" if splits > 64 else "tree16"
    return "four" if splits <= 4 and n // 4 >= 16384 else "col"


def group_sums(rows, G, unroll, mut=None):
    """[splits][n] -> [G][n]: group g adds the splits g, g + G, ... in order (the unrolled loop takes `unroll` at a
    time, a remainder loop the rest; mut 'remainder' skips that loop)"""
    splits, n = rows.shape
    red = torch.zeros(G, n)
    for g in range(min(G, splits)):
        zs = list(range(g, splits, G))
        if mut == "remainder":
            zs = zs[:len(zs) - len(zs) % unroll]
        for z in zs:
            red[g] += rows[z]
    return red


def emu_reduce(src, stride, splits, n, out0, accumulate=1, mut=None):
    """one segment of rs_reduce_segments: src flat float32, split z at src + z stride.  mut: 'stridelen' the stride
    taken as n; 'skipsplit' the last split left out; 'remainder'; 'noacc' accumulate ignored; 'old2' the four-column
    form adds the old value twice"""
    st = n if mut == "stridelen" else stride
    rows = torch.stack([src[z * st:z * st + n] for z in range(splits)])
    if mut == "skipsplit":
        rows = rows[:-1] if splits > 1 else torch.zeros(1, n)
    form = seg_form(splits, n)
    if form in ("col", "four"):
        acc = group_sums(rows, 1, 4, mut if form == "col" else None)[0]
    else:
        G = 64 if form == "tree4" else 16
        red = group_sums(rows, G, 4, mut)
        h = G // 2
        while h:
            red[:h] += red[h:2 * h]
            h //= 2
        acc = red[0]
    if accumulate and mut != "noacc":
        acc = acc + out0
        if form == "four" and mut == "old2":
            acc = acc + out0
    return acc


def emu_wgrad_grouped(probs, M, per_split, T, extra=None, mut=None):
    """rs_wgrad_grouped_max at tile edge T: [(dW, db)] and the extra pair's outputs.  mut (besides emu_partials' and
    emu_reduce's): 'biastile' the bias column sums formed in column tile 1 (never, for a problem of one column tile:
    its slab columns stay unwritten); 'adjbias' the bias partials of the next problem"""
    splits = cdiv(M, per_split)
    stage = 32 if T == 256 else 64
    slabs = [emu_partials(p, M, per_split, stage, splits, mut=mut) for p in probs]
    outs = []
    for i, p in enumerate(probs):
        N, K = p["N"], p["K"]
        slab = slabs[i].clone()
        if mut == "biastile" and K // T < 2:
            slab[:, N * K:] = NAN
        if mut == "adjbias":
            q = probs[(i + 1) % len(probs)]
            slab[:, N * K:] = slabs[(i + 1) % len(probs)][:, q["N"] * q["K"]:][:, torch.arange(N) % q["N"]]
        flat, stride = slab.reshape(-1), N * K + N
        dW = emu_reduce(flat, stride, splits, N * K, p["dW0"].reshape(-1), 1, mut).view(N, K)
        db = None if p["db0"] is None else emu_reduce(flat[N * K:], stride, splits, N, p["db0"], 1, mut)
        outs.append((dW, db))
    ex = []
    if extra is not None:
        flat = extra["part"].reshape(-1)
        ex = [emu_reduce(flat[i * EXTRA_N:], 2 * EXTRA_N, EXTRA_SPLITS, EXTRA_N, extra["out0"][i], 1, mut)
              for i in range(2)]
    return outs, ex


def group_tile(shapes, max_tile):
    """wgrad_tile: the largest of 256, 128, 64 (at most max_tile) dividing every N and K"""
    T = 256 if max_tile >= 256 else 128 if max_tile >= 128 else 64
    while any(N % T or K % T for N, K in shapes):
        T //= 2
    return T


# ====================================================================== emulation: reduce.hip, rs_colsum
def slabs_form(n, n0, aligned=True):
    """(C, G, unroll) of launch_reduce_slabs: float4 columns C = 16 / 32 / 64 by n, else the scalar kernel"""
    if n % 4 or n0 % 4 or not aligned:
        return 64, 4, 8
    n4 = n // 4
    C = 16 if n4 <= 16 else 32 if n4 <= 256 else 64
    return C, 256 // C, 4


def emu_reduce_slabs(slab, n0, out0, out1, accumulate, aligned=True, mut=None):
    """slab [splits][n]: the split groups' sums added in group order, then the old value; (out0 [n0], out1 [n - n0]),
    None where that output is null.  mut: 'remainder', 'skipsplit', 'noacc'"""
    splits, n = slab.shape
    _, G, unroll = slabs_form(n, n0, aligned)
    rows = slab if mut != "skipsplit" else (slab[:-1] if splits > 1 else torch.zeros(1, n))
    red = group_sums(rows, G, unroll, mut)
    t = red[0].clone()
    for g in range(1, G):
        t += red[g]
    res = []
    for old, sl in ((out0, slice(0, n0)), (out1, slice(n0, n))):
        res.append(None if old is None else (t[sl] + old if accumulate and mut != "noacc" else t[sl].clone()))
    return res


def colsum_form(dt, N):
    """row groups of colsum_partial: 16-byte chunk columns CPR = 16 / 32 / 64 (256 / CPR groups), else one thread
    per column over the block's rows in order"""
    V = 8 if dt == BF else 4
    cpr = N // V
    if N % V or cpr > 64:
        return 1
    return 256 // (16 if cpr <= 16 else 32 if cpr <= 32 else 64)


def emu_colsum(X, out0, accumulate, mut=None):
    """mut 'lastrow': the last row of the last block not read"""
    M, N = X.shape
    nblk = colsum_blocks(M)
    per = cdiv(M, nblk)
    RG = colsum_form(X.dtype, N)
    ws = torch.zeros(nblk, N)
    for b in range(nblk):
        r1 = min(M, (b + 1) * per) - (1 if mut == "lastrow" and b == nblk - 1 else 0)
        x = X[b * per:r1].float()
        if x.shape[0]:
            red = group_sums(x, RG, 1)
            for g in range(RG):
                ws[b] += red[g]
    return emu_reduce_slabs(ws, N, out0, None, accumulate, mut=mut if mut != "lastrow" else None)[0]


# ====================================================================== emulation: rs_linear_wgrad
def lw_direct(dt, K, splits, unaligned):
    return dt == BF and not unaligned and splits == 1 and K % 8 == 0


def emu_linear_wgrad(p, M, splits, rows_dev, accumulate, unaligned=False, mut=None):
    """one split (bf16, aligned): straight into dW / db; else split-K slabs of ceil(ceil(M / splits) / 64) 64 rows and
    one rs_reduce_slabs2 pass.  mut: 'rowsdev' the device row count ignored; emu_partials' and emu_reduce_slabs'"""
    N, K, dt = p["N"], p["K"], p["dY"].dtype
    limit = None if mut == "rowsdev" else rows_dev
    stage = 64 if dt == BF and not unaligned else 32
    if lw_direct(dt, K, splits, unaligned):
        s = emu_partials(p, M, M, stage, 1, limit, mut)[0]
        dW, db = s[:N * K].view(N, K), s[N * K:]
        if accumulate and mut != "noacc":
            dW, db = dW + p["dW0"], (db + p["db0"] if p["db0"] is not None else None)
        return dW, (db if p["db0"] is not None else None)
    slab = emu_partials(p, M, cdiv(cdiv(M, splits), 64) * 64, stage, splits, limit, mut)
    if p["db0"] is None:
        slab = slab[:, :N * K]
    dW, db = emu_reduce_slabs(slab, N * K, p["dW0"].reshape(-1), p["db0"], accumulate, mut=mut)
    return dW.view(N, K), db


# ====================================================================== emulation: the fused launch
def fused_inputs(d, T, B, dev, hb=None):
    """the SAS block's set at M = B T rows: five problems [(d, d) x 4, (2 d, d)], four LayerNorm partial set pairs,
    the positional sum's inputs (ids with padding, the last position all padding when T > 1), head partials"""
    M = B * T
    g = gen_for(dev, 43, d, T, B)
    probs = [problem(g, dev, M, N, d, bias=i != 2) for i, N in enumerate((d, d, d, d, 2 * d))]
    ln = [{"part": rn(g, dev, LN_SETS, 2, d, s=0.3), "out0": [rn(g, dev, d), rn(g, dev, d)]} for _ in range(4)]
    emb = L.embed_inputs(BF, d, B, T, dev)
    emb["ids"][0] = 3                                       # position 0 has a live row at every batch size
    # rows 2^-12 .. 2^12 apart: a float32 sum of bf16 values of one magnitude is exact in any order, and would hide
    # the order the batch rows are added in
    e = torch.randint(-12, 13, (M, 1), generator=g, device=dev)
    emb["dx"] = (emb["dx"].float() * torch.pow(2.0, e.float())).to(BF)
    if T > 1:
        emb["ids"].view(B, T)[:, T - 1] = 0
    head = None
    if hb:
        head = rn(g, dev, hb, 3, s=1.0).abs()
        head[:, 2] = torch.randint(0, 65, (hb,), generator=g, device=dev).float()
        head[0, 2] = 7.0
    return {"probs": probs, "ln": ln, "emb": emb, "head": head, "M": M, "d": d}


def emu_pos(inp, keep, p, RG, mut=None):
    """embed_pos_body in SAS mode, dpos +=: batch group g adds the sequences g, g + RG, ... in order, the groups are
    added in order, then the old value.  mut 'noh': the head-statistics workgroup's offset forgotten: position 0 is
    never summed"""
    ids, T, d = inp["ids"], inp["T"], inp["d"]
    nb = ids.numel() // T
    mk = keep.float() * np.float32(kmul(p))
    g = (inp["dx"].float() * mk * (ids != 0).float()[:, None]).view(nb, T * d)
    red = group_sums(g, RG, 8)
    s = red[0].clone()
    for i in range(1, RG):
        s += red[i]
    out = inp["dpos0"] + s.view(T, d)
    if mut == "noh":
        out[0] = inp["dpos0"][0]
    return out
