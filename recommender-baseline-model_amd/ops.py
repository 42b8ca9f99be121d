"""Thin tensor-level wrappers over the C ABI (librecsys_hip.so).

Every function launches HIP kernels on the current torch stream and returns
nothing; outputs are caller-allocated tensors (the C ABI allocates nothing).
2-D tensors are passed with their row stride as the leading dimension.
"""
import ctypes as C
import os

import torch

from . import _lib
from ._lib import BF16, F32, Epilogue, call, ptr, stream

ACT_NONE, ACT_RELU, ACT_GELU, ACT_RELU_BWD, ACT_GELU_BWD = (
    _lib.ACT_NONE, _lib.ACT_RELU, _lib.ACT_GELU, _lib.ACT_RELU_BWD, _lib.ACT_GELU_BWD)


# ------------------------------------------------------------------ kernel stamps
STAMP_KINDS = {1: "attn_bwd", 2: "wgrad_grouped", 3: "vocab_ce_fwd"}


def kernel_stamps(buf, step, kinds=()):
    """Enable (buf: int64 device tensor, step: the optimizer's float64 device step count, kinds: names from
    STAMP_KINDS) or disable (None, None) the in-kernel begin/end stamps of rs_attn_bwd / rs_wgrad_grouped
    launches (layout in include/recsys_hip.h).  Launches captured into a graph while enabled keep stamping
    on every replay."""
    mask = sum(1 << k for k, n in STAMP_KINDS.items() if n in kinds)
    call("rs_kernel_stamps", ptr(buf), ptr(step), mask)


def read_kernel_stamps(buf, khz):
    """[(mark, step slot, µs)] of every complete record in a stamp buffer (after the stamped work finished)."""
    import numpy as np
    h = buf.cpu().numpy().view(np.uint64)
    steps, marks, W = int(h[1]), int(h[2]), int(h[3])
    rec = h[4:4 + steps * marks * (1 + W)].reshape(steps, marks, 1 + W)
    out = []
    for st in range(steps):
        for m in range(marks):
            b, e = int(rec[st, m, 0]), int(rec[st, m, 1:].max())
            if b and e > b:
                out.append((m, st, (e - b) / khz * 1e3))
    return out


def kernel_stamp_kinds():
    """Kind name of every mark handed out since the last kernel_stamps(buf, step), in mark order."""
    n = _lib.lib().rs_kernel_stamp_count()
    arr = (C.c_int * max(n, 1))()
    call("rs_kernel_stamp_kinds", arr, n)
    return [STAMP_KINDS.get(arr[i], "?") for i in range(n)]


# ------------------------------------------------------------------ HIP-event launch timing
_EVENTS = {"kinds": (), "pairs": []}


def event_timing(kinds=()):
    """Bracket every launch of the named kinds (STAMP_KINDS names) with a pair of timing HIP events on the current
    stream (eager launches; bench.py's roofline leg).  Returns the list collecting (kind, begin event, end event);
    kinds=() disables."""
    _EVENTS["kinds"], _EVENTS["pairs"] = tuple(kinds), []
    return _EVENTS["pairs"]


def _ev_begin(kind):
    if kind not in _EVENTS["kinds"]:
        return None
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _EVENTS["pairs"].append((kind, e0, e1))
    return e1


def _ev_end(e1):
    if e1 is not None:
        e1.record()


def wall_clock_khz():
    k = C.c_int()
    call("rs_wall_clock_khz", C.byref(k))
    return k.value


def dtype_code(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported dtype {t.dtype}")


def ld(t):
    return t.stride(0) if t.dim() == 2 else t.shape[-1]


def epilogue(bias=None, alpha=1.0, act=ACT_NONE, aux=None, aux_out=None, drop_p=0.0, drop_seed=0,
             seed_base=None, drop_ld=0, resid=None, rowmask_ids=None, accumulate=False, post_drop_p=0.0,
             post_drop_seed=0, rows_dev=None):
    e = Epilogue()
    e.bias = ptr(bias)
    e.alpha = alpha
    e.act = act
    e.aux = ptr(aux)
    e.aux_out = ptr(aux_out)
    a = aux if aux is not None else aux_out
    e.ldaux = ld(a) if a is not None else 0
    e.drop_p = drop_p
    e.drop_seed = drop_seed
    e.seed_base = ptr(seed_base)
    e.drop_ld = drop_ld
    e.resid = ptr(resid)
    e.ldres = ld(resid) if resid is not None else 0
    e.rowmask_ids = ptr(rowmask_ids)
    e.accumulate = 1 if accumulate else 0
    e.post_drop_p = post_drop_p
    e.post_drop_seed = post_drop_seed
    e.rows_dev = ptr(rows_dev)
    return e


def gemm(A, B, Cout, M, N, K, a_kmajor=False, b_kmajor=False, epi=None, split_k=1, slab=None):
    """Cout[M,N] = epi(A . B^T) with the storage conventions of rs_gemm (C may be fp32 for bf16 A/B)."""
    assert A.dtype == B.dtype, "A and B must share the compute dtype"
    call("rs_gemm", dtype_code(A), int(a_kmajor), int(b_kmajor), M, N, K, ptr(A), ld(A), ptr(B), ld(B),
         ptr(Cout), ld(Cout), int(Cout.dtype == torch.float32),
         C.byref(epi) if epi is not None else None, split_k, ptr(slab), stream())


def linear_fwd(X, W, Y, bias=None, **epi_kw):
    """Y = X W^T (+ fused epilogue).  X [M,K], W [N,K], Y [M,N]."""
    M, K = X.shape
    N = W.shape[0]
    gemm(X, W, Y, M, N, K, False, False, epilogue(bias=bias, **epi_kw))


RS_ERR_UNSUPPORTED = 1002


def linear_fwd_ln(X, gamma, beta, eps, W, Y, h=None, mean=None, rinv=None, bias=None, **epi_kw):
    """Y = epi(LN(X) W^T) with the BERT LayerNorm (variant 1) in the GEMM's prologue (rs_gemm_ln); h / mean / rinv
    receive what rs_layernorm_fwd would write.  Returns False (nothing launched) when the shape or epilogue is not
    one the fused kernel covers -- the caller then runs layernorm_fwd + linear_fwd."""
    M, K = X.shape
    N = W.shape[0]
    e = epilogue(bias=bias, **epi_kw)
    rc = _lib.lib().rs_gemm_ln(M, N, K, ptr(X), ld(X), ptr(gamma), ptr(beta), eps, ptr(W), ld(W), ptr(Y), ld(Y),
                               C.byref(e), ptr(h), ld(h) if h is not None else 0, ptr(mean), ptr(rinv), stream())
    if rc == RS_ERR_UNSUPPORTED:
        return False
    if rc != 0:
        raise RuntimeError(f"rs_gemm_ln failed with code {rc}")
    return True


def linear_dgrad(dY, W, dX, **epi_kw):
    """dX = dY W (+ epilogue).  dY [M,N], W [N,K], dX [M,K]."""
    M, N = dY.shape
    K = W.shape[1]
    gemm(dY, W, dX, M, K, N, False, True, epilogue(**epi_kw))


def linear_dgrad_splitk(dY, W, dX, slab, splits, acc_f32=None, rows_dev=None):
    """dX = dY W for a long contraction (dY [M,N] with N >> M, e.g. the vocabulary gradient):
    split-K into fp32 slabs (rs_gemm with split_k) + one deterministic reduce (+ cast when dX is
    bf16, through ``acc_f32`` [M,K] fp32)."""
    M, N = dY.shape
    K = W.shape[1]
    assert slab.numel() >= splits * M * K
    gemm(dY, W, slab, M, K, N, False, True, epilogue(rows_dev=rows_dev), split_k=splits, slab=slab)
    out = dX if dX.dtype == torch.float32 else acc_f32
    assert out is not None and out.is_contiguous() and out.shape == (M, K)
    call("rs_reduce_slabs", ptr(slab), splits, M * K, ptr(out), 0, stream())
    if out is not dX:
        cast_bf16(out, dX)


def split_for(M_tok, n_out, k_in):
    """Split-K factor of the weight-gradient GEMM: ~1024 blocks of 64x64 output tiles, >= 256 rows each."""
    tiles = -(-n_out // 64) * -(-k_in // 64)
    return int(max(1, min(-(-1024 // tiles), -(-M_tok // 256))))


def wgrad_slab_numel(M_tok, n_out, k_in):
    return split_for(M_tok, n_out, k_in) * (n_out * k_in + n_out)


def linear_wgrad(dY, X, dW, slab, db=None, split_k=None, accumulate=True, rows_dev=None):
    """dW [N,K] (+)= dY^T X and db [N] (+)= colsum(dY) over M token rows (rs_linear_wgrad)."""
    M, N = dY.shape
    K = X.shape[1]
    s = split_k or split_for(M, N, K)
    direct = s == 1 and dY.dtype == torch.bfloat16 and K % 8 == 0 and dW.data_ptr() % 16 == 0  # no slab used
    assert direct or slab.numel() >= s * (N * K + N), "slab workspace too small"
    assert dY.dtype == X.dtype
    call("rs_linear_wgrad", dtype_code(dY), M, N, K, ptr(dY), ld(dY), ptr(X), ld(X), ptr(dW), ptr(db),
         int(accumulate), s, ptr(slab), ptr(rows_dev), stream())


def colsum(X, out, ws, accumulate=True):
    M, N = X.shape
    call("rs_colsum", dtype_code(X), ptr(X), M, N, ld(X), ptr(ws), ptr(out), int(accumulate), stream())


def layernorm_fwd(X, gamma, beta, eps, Y, mean, rinv, variant):
    M, d = X.shape
    call("rs_layernorm_fwd", dtype_code(X), variant, ptr(X), ld(X), M, d, ptr(gamma), ptr(beta), eps,
         ptr(Y), ld(Y), ptr(mean), ptr(rinv), stream())


def layernorm_bwd_nparts(X):
    """Partial count layernorm_bwd leaves in ws when called with dgamma = dbeta = None (0: not deferrable)."""
    M, d = X.shape
    ok = X.data_ptr() % 16 == 0 and ld(X) % (8 if X.dtype == torch.bfloat16 else 4) == 0
    return int(_lib.lib().rs_layernorm_bwd_nparts(dtype_code(X), M, d)) if ok else 0


def layernorm_bwd_drop(X, dY, gamma, mean, rinv, eps, dX, dgamma, dbeta, ws, variant, drop_p, salt1, salt2, seed_base,
                       out1, out2=None, accumulate=False):
    """layernorm_bwd, then out1 = drop(dX; salt1) (and out2 = drop(out1; salt2)) in the same launch."""
    M, d = X.shape
    assert out1.shape == (M, d) and out1.is_contiguous() and (out2 is None or out2.is_contiguous())
    call("rs_layernorm_bwd_drop", dtype_code(X), variant, ptr(X), ld(X), ptr(dY), ld(dY), M, d, ptr(gamma),
         ptr(mean), ptr(rinv), eps, ptr(dX), ld(dX), int(accumulate), ptr(dgamma), ptr(dbeta), ptr(ws), drop_p, salt1,
         salt2, ptr(seed_base), ptr(out1), ptr(out2), stream())


def layernorm_bwd(X, dY, gamma, mean, rinv, eps, dX, dgamma, dbeta, ws, variant, accumulate=False):
    M, d = X.shape
    call("rs_layernorm_bwd", dtype_code(X), variant, ptr(X), ld(X), ptr(dY), ld(dY), M, d, ptr(gamma),
         ptr(mean), ptr(rinv), eps, ptr(dX), ld(dX), int(accumulate), ptr(dgamma), ptr(dbeta), ptr(ws), stream())


def embed_fwd(mode, ids, T, table, pos, scale, drop_p, seed, seed_base, out):
    rows = ids.numel()
    d = table.shape[1]
    call("rs_embed_fwd", dtype_code(table), mode, ptr(ids), rows, T, ptr(table), ptr(pos), d, scale, drop_p,
         seed, ptr(seed_base), ptr(out), stream())


def embed_bwd(mode, ids, T, dx, scale, drop_p, seed, seed_base, dtable, dpos, accumulate_pos=True):
    rows = ids.numel()
    d = dx.shape[-1]
    call("rs_embed_bwd", dtype_code(dx), mode, ptr(ids), rows, T, ptr(dx), d, scale, drop_p, seed,
         ptr(seed_base), ptr(dtable), ptr(dpos), int(accumulate_pos), stream())


def attn_fwd(B, T, H, Dh, q, k, v, o, lse, scale, mask_kind, ids, drop_p, seed, seed_base):
    call("rs_attn_fwd", dtype_code(q), B, T, H, Dh, ptr(q), ld(q), ptr(k), ld(k), ptr(v), ld(v), ptr(o), ld(o),
         ptr(lse), scale, mask_kind, ptr(ids), drop_p, seed, ptr(seed_base), stream())


RS_ATTN_DELTA_IN = 0x100


def attn_row_delta(B, T, H, Dh, do, o, delta):
    """delta[(b*H+h)*T + t] = sum over head h's columns of do * o (the input of attn_bwd(delta_in=True))."""
    call("rs_attn_row_delta", dtype_code(do), B, T, H, Dh, ptr(do), ld(do), ptr(o), ld(o), ptr(delta), stream())


def attn_bwd(B, T, H, Dh, q, k, v, o, do, lse, dq, dk, dv, scale, mask_kind, ids, drop_p, seed, seed_base, ws,
             delta_in=False):
    """delta_in: ws already holds delta = rowsum(dO * O) per (b, h, t) (sas_block_out_bwd with o=)."""
    mk = mask_kind | (RS_ATTN_DELTA_IN if delta_in else 0)
    ev = _ev_begin("attn_bwd")
    call("rs_attn_bwd", dtype_code(q), B, T, H, Dh, ptr(q), ld(q), ptr(k), ld(k), ptr(v), ld(v), ptr(o), ld(o),
         ptr(do), ld(do), ptr(lse), ptr(dq), ld(dq), ptr(dk), ld(dk), ptr(dv), ld(dv), scale, mk, ptr(ids),
         drop_p, seed, ptr(seed_base), ptr(ws), stream())
    _ev_end(ev)


def sampled_logits_fwd(f, E, pos, neg, pl, nl):
    M, d = f.shape
    call("rs_sampled_logits_fwd", dtype_code(f), ptr(f), M, d, ptr(E), ptr(pos), ptr(neg), ptr(pl), ptr(nl),
         stream())


def sampled_logits_bwd(f, E, pos, neg, dpl, dnl, df, dE, accumulate_df=False):
    M, d = f.shape
    call("rs_sampled_logits_bwd", dtype_code(f), ptr(f), M, d, ptr(E), ptr(pos), ptr(neg), ptr(dpl), ptr(dnl),
         ptr(df), int(accumulate_df), ptr(dE), stream())


def bce_fwd(pl, nl, pos, ws, out, count_override=None):
    call("rs_bce_fwd", ptr(pl), ptr(nl), ptr(pos), pl.numel(), ptr(count_override), ptr(ws), ptr(out), stream())


def bce_bwd(pl, nl, pos, count, dloss, dpl, dnl):
    call("rs_bce_bwd", ptr(pl), ptr(nl), ptr(pos), pl.numel(), ptr(count), ptr(dloss), ptr(dpl), ptr(dnl),
         stream())


def ce_fwd(logits, labels, ws, out, count_override=None, rows_dev=None):
    R, V1 = logits.shape
    call("rs_ce_fwd", ptr(logits), R, V1, ld(logits), ptr(labels), ptr(count_override), ptr(ws), ptr(out),
         ptr(rows_dev), stream())


def ce_bwd(logits, labels, count, dloss, ws, dlogits, rows_dev=None):
    R, V1 = logits.shape
    call("rs_ce_bwd", dtype_code(dlogits), ptr(logits), R, V1, ld(logits), ptr(labels), ptr(count), ptr(dloss),
         ptr(ws), ptr(dlogits), ld(dlogits), ptr(rows_dev), stream())


def compact_rows(labels, cap, idx, rank, count):
    call("rs_compact_rows", ptr(labels), labels.numel(), cap, ptr(idx), ptr(rank), ptr(count), stream())


def gather_rows(src, idx, count, cap, dst, labels=None, lab_out=None):
    d = src.shape[1]
    call("rs_gather_rows", dtype_code(src), ptr(src), ld(src), d, ptr(idx), ptr(count), cap, ptr(dst), ld(dst),
         ptr(labels), ptr(lab_out), stream())


def scatter_rows(src, rank, dst):
    n, d = dst.shape
    call("rs_scatter_rows", dtype_code(src), ptr(src), ld(src), d, ptr(rank), n, ptr(dst), ld(dst), stream())


def reduce_slabs(slab, splits, out, accumulate=False):
    """out (+)= sum over the `splits` leading slabs of slab (fixed order)."""
    n = out.numel()
    call("rs_reduce_slabs", ptr(slab), splits, n, ptr(out), int(accumulate), stream())


def splitk_scatter_rows(slab, splits, cap, rank, dst):
    """dst[r] = sum_z slab[z][rank[r]] (0 where rank < 0): split-K reduce + cast + scatter, one launch."""
    n, d = dst.shape
    call("rs_splitk_scatter_rows", dtype_code(dst), ptr(slab), splits, cap, d, ptr(rank), n, ptr(dst), ld(dst),
         stream())


def adam_prepare(state, hyper, grad_divisor=None, seed_base=None):
    call("rs_adam_prepare", ptr(state), ptr(hyper), ptr(grad_divisor), ptr(seed_base), stream())


def row_marks_bytes(rows):
    """Size of a row-marks array (rs_item_grad_marked / rs_adam_*_marked): the rows' stamps, padding to 16 B + 16
    (the sweep's scalar mark loads run past the last row) and a 1 KB zero tail (the unstamped rows' gradient
    loads read it).  Allocate zeroed, 16-byte aligned."""
    return (rows + 15) // 16 * 16 + 16 + 1024


def adam_step(p, g, m, v, p_bf16, state, hyper, zero_grad=False, max_wg=None, marks=None):
    """marks: (row_marks u8, epoch u8, moff, rows, dshift) of a marked table inside this range (rs_adam_step_marked)."""
    if marks is not None:
        rm, ep, moff, rows, dshift = marks
        call("rs_adam_step_marked", p.numel(), ptr(p), ptr(g), ptr(m), ptr(v), ptr(p_bf16), ptr(state), ptr(hyper),
             int(zero_grad), int(max_wg or 8192), ptr(rm), ptr(ep), int(moff), int(rows), int(dshift), stream())
        return
    if max_wg:
        call("rs_adam_step_wg", p.numel(), ptr(p), ptr(g), ptr(m), ptr(v), ptr(p_bf16), ptr(state), ptr(hyper),
             int(zero_grad), int(max_wg), stream())
        return
    call("rs_adam_step", p.numel(), ptr(p), ptr(g), ptr(m), ptr(v), ptr(p_bf16), ptr(state), ptr(hyper),
         int(zero_grad), stream())


def adam_prepare_step(p, g, m, v, p_bf16, state, hyper, zero_grad=False, grad_divisor=None, seed_base=None,
                      transposed=None, loss_sum=None, loss_out=None, tbase=0, marks=None):
    """adam_prepare + adam_step in one launch (state: double[144]; state[7], state[16 + 16 k] arrival counters).
    transposed: (desc int64 device [n][6] as transpose_bf16's, its host copy, dst bf16 tensor) -- the bf16
    result of those matrices is also written transposed; the descriptors' offsets are flat-buffer elements and
    p[0] is element `tbase` of the flat buffer (every matrix must lie inside [tbase, tbase + p.numel()))."""
    if state.numel() < 144:
        raise ValueError("adam_prepare_step needs the 144-entry optimizer state")
    td, nt, wt = None, 0, None
    if transposed is not None:
        td, host, wt = transposed
        nt = len(host)
        for rows, cols, off, lds, doff, ldd in host:
            if lds % 4 or off % 4 or tbase % 4 or off < tbase or off + rows * lds > tbase + (p.numel() // 4) * 4 \
                    or doff + (cols - 1) * ldd + rows > wt.numel() or rows * lds >= 2 ** 31:
                raise ValueError("adam_prepare_step: transposed matrix outside the buffers or misaligned")
        if p_bf16 is None:
            raise ValueError("adam_prepare_step: transposed copies need the bf16 output")
    if marks is not None:      # a marked table inside the range (rs_adam_prepare_step_marked)
        rm, ep, moff, rows, dshift = marks
        call("rs_adam_prepare_step_marked", p.numel(), ptr(p), ptr(g), ptr(m), ptr(v), ptr(p_bf16), ptr(state),
             ptr(hyper), int(zero_grad), ptr(grad_divisor), ptr(seed_base), ptr(td), nt, int(tbase), ptr(wt),
             ptr(loss_sum), ptr(loss_out), ptr(rm), ptr(ep), int(moff), int(rows), int(dshift), stream())
        return
    if loss_out is not None:   # + loss_out = loss_sum / grad_divisor in the same launch
        call("rs_adam_prepare_step_loss", p.numel(), ptr(p), ptr(g), ptr(m), ptr(v), ptr(p_bf16), ptr(state),
             ptr(hyper), int(zero_grad), ptr(grad_divisor), ptr(seed_base), ptr(td), nt, int(tbase), ptr(wt), ptr(loss_sum),
             ptr(loss_out), stream())
        return
    call("rs_adam_prepare_step", p.numel(), ptr(p), ptr(g), ptr(m), ptr(v), ptr(p_bf16), ptr(state), ptr(hyper),
         int(zero_grad), ptr(grad_divisor), ptr(seed_base), ptr(td), nt, int(tbase), ptr(wt), stream())


def sgd_step(p, g, buf, p_bf16, state, hyper, zero_grad=False, prepare=False, grad_divisor=None, seed_base=None,
             transposed=None, tbase=0, loss_sum=None, loss_out=None, max_wg=8192):
    """torch.optim.SGD over a flat range in one launch (rs_sgd_step).  buf None: no momentum.  hyper: double[3] =
    {lr, momentum, weight_decay} on the device; state: double[>= 1], state[0] the step count.  prepare: the first
    range of a step (step count, seed, loss_out = loss_sum / grad_divisor).  transposed / tbase: as
    adam_prepare_step's.  max_wg: at most that many workgroups (0: unbounded)."""
    if hyper.dtype != torch.float64 or state.dtype != torch.float64 or hyper.numel() < 3 or state.numel() < 1:
        raise ValueError("sgd_step: state / hyper must be the optimizer's float64 device arrays")
    if max_wg is None or max_wg < 0:
        raise ValueError("sgd_step: max_wg must be >= 0")
    n = p.numel()
    if g.numel() != n or (buf is not None and buf.numel() != n) or (p_bf16 is not None and p_bf16.numel() != n):
        raise ValueError("sgd_step: p, g, buf and p_bf16 must have one length")
    td, nt, wt = None, 0, None
    if transposed is not None:
        td, host, wt = transposed
        nt = len(host)
        for rows, cols, off, lds, doff, ldd in host:
            if lds % 4 or cols % 4 or off % 4 or tbase % 4 or off < tbase or off + rows * lds > tbase + (n // 4) * 4 \
                    or doff < 0 or doff + (cols - 1) * ldd + rows > wt.numel() or rows * lds >= 2 ** 31 \
                    or cols > lds or rows <= 0 or cols <= 0 or ldd < rows:
                raise ValueError("sgd_step: transposed matrix outside the buffers or misaligned")
        if p_bf16 is None:
            raise ValueError("sgd_step: transposed copies need the bf16 output")
    call("rs_sgd_step", n, ptr(p), ptr(g), ptr(buf), ptr(p_bf16), ptr(state), ptr(hyper), int(zero_grad),
         int(prepare), ptr(grad_divisor), ptr(seed_base), ptr(td), nt, int(tbase), ptr(wt), ptr(loss_sum),
         ptr(loss_out), int(max_wg), stream())


L2_CHUNK = 16384


def l2_chunk_desc(flat, device):
    """rs_l2_penalty's chunk descriptor over a FlatParams buffer: one segment per parameter tensor (its exact
    elements, alignment padding excluded), cut into chunks of at most L2_CHUNK elements.  int64 [n][4]."""
    rows = []
    for n in flat.names:
        lo = flat.offsets[n]
        cnt = 1
        for s in flat.shapes[n]:
            cnt *= s
        first, nch = len(rows), max(1, -(-cnt // L2_CHUNK))
        for k in range(nch):
            rows.append([lo + k * L2_CHUNK, lo + min(cnt, (k + 1) * L2_CHUNK), first, nch])
    return torch.tensor(rows, dtype=torch.int64, device=device)


def l2_penalty(p, g, desc, l2, ws, loss=None, scale=None):
    """loss += l2 * sum ||p_seg||, g += scale * l2 * p / ||p_seg|| (BS/trainers/sas.py:51-52; rs_l2_penalty)."""
    assert ws.numel() >= 2 * desc.shape[0] and ws.dtype == torch.float32   # chunk sums + segment norms
    call("rs_l2_penalty", ptr(p), ptr(g), ptr(desc), desc.shape[0], float(l2), ptr(scale), ptr(ws), ptr(loss),
         stream())


def cast_bf16(src, dst):
    call("rs_cast_bf16", src.numel(), ptr(src), ptr(dst), stream())


def dropout_rowmask(x, drop_p, seed, seed_base, rowmask_ids, out, out_masked=None):
    M, N = x.shape
    call("rs_dropout_rowmask", dtype_code(x), ptr(x), M, N, ld(x), drop_p, seed, ptr(seed_base), N,
         ptr(rowmask_ids), ptr(out), ptr(out_masked), stream())


def dropout2(x, drop_p, salt1, salt2, seed_base, out1, out2):
    """out1 = drop(x; salt1), out2 = drop(out1; salt2): two stacked dropout sites' backward, one pass."""
    M, N = x.shape
    call("rs_dropout2", dtype_code(x), ptr(x), M, N, ld(x), drop_p, salt1, salt2, ptr(seed_base), N, ptr(out1),
         ptr(out2), stream())


# ---- BERT vocabulary head + cross entropy, logits not materialised (vocab_ce.hip) -----------
def vocab_ce_ws_numel(R, V1):
    n = _lib.lib().rs_vocab_ce_ws_numel(R, V1)
    if n < 0:
        raise RuntimeError("rs_vocab_ce_ws_numel: bad arguments")
    return n


def vocab_ce_fwd(h, E, bias, labels, ws, out, rows_dev=None, count_override=None):
    """out[0:3] = (loss sum, labelled count, mean) of CE(h E^T + bias, labels, ignore_index=0); ws keeps
    the row log-sum-exp for vocab_ce_bwd."""
    R, d = h.shape
    V1 = E.shape[0]
    call("rs_vocab_ce_fwd", R, V1, d, ptr(h), ld(h), ptr(E), ld(E), ptr(bias), ptr(labels), ptr(rows_dev),
         ptr(count_override), ptr(ws), ptr(out), stream())


def vocab_head_supported(d):
    return bool(_lib.lib().rs_vocab_head_supported(d))


def vocab_head_fwd(h, E, bias, labels, ws, out, rows_dev=None, count_override=None):
    """vocab_ce_fwd's result from the vocabulary-tile-stationary kernel (rs_vocab_head_fwd)."""
    R, d = h.shape
    V1 = E.shape[0]
    ev = _ev_begin("vocab_ce_fwd")
    call("rs_vocab_head_fwd", R, V1, d, ptr(h), ld(h), ptr(E), ld(E), ptr(bias), ptr(labels), ptr(rows_dev),
         ptr(count_override), ptr(ws), ptr(out), stream())
    _ev_end(ev)


def vocab_head_bwd(h, E, bias, labels, ws, count, dl, rows_dev=None, dloss=None, voff=0):
    """vocab_ce_bwd's dlogits from the vocabulary-tile-stationary kernel (rs_vocab_head_bwd); E may be a shard of
    the table starting at vocabulary id voff (labels stay absolute)."""
    R, d = h.shape
    V1 = E.shape[0]
    call("rs_vocab_head_bwd", R, V1, d, ptr(h), ld(h), ptr(E), ld(E), ptr(bias), ptr(labels), ptr(rows_dev),
         ptr(count), ptr(dloss), ptr(ws), ptr(dl), ld(dl), int(voff), stream())


def vocab_head_form(bwd, R, V1, d, cus=0):
    """(form: 1 ping-pong / 0 lock-step, gridDim.x, gridDim.y, row tiles per y-group, dynamic LDS bytes) of the
    vocab_head_fwd (bwd False) / vocab_head_bwd launch at these sizes (rs_vocab_head_form: host only; cus <= 0 asks
    the device; RS_VHEAD_PP is honoured)."""
    out = (C.c_int * 5)()
    call("rs_vocab_head_form", int(bool(bwd)), R, V1, d, int(cus), out)
    return tuple(out)


def vocab_shard_lse(h, E, bias, labels, ws, lse):
    R, d = h.shape
    call("rs_vocab_shard_lse", R, E.shape[0], d, ptr(h), ld(h), ptr(E), ld(E), ptr(bias), ptr(labels), ptr(ws),
         ptr(lse), stream())


def vocab_shard_label_logits(h, E, bias, labels, v0, v1, tgt):
    R, d = h.shape
    call("rs_vocab_shard_label_logits", R, d, ptr(h), ld(h), ptr(E), ld(E), ptr(bias), ptr(labels), int(v0), int(v1),
         ptr(tgt), stream())


def vocab_shard_combine(lse_parts, tgt, labels, lse, out):
    N, R = lse_parts.shape
    call("rs_vocab_shard_combine", N, R, ptr(lse_parts), ptr(tgt), ptr(labels), ptr(lse), ptr(out), stream())


def vocab_ce_bwd(h, E, bias, labels, ws, count, dl, rows_dev=None, dloss=None):
    """dl [R, V1] bf16 = (softmax(h E^T + bias) - onehot(labels)) * dloss / count."""
    R, d = h.shape
    V1 = E.shape[0]
    call("rs_vocab_ce_bwd", R, V1, d, ptr(h), ld(h), ptr(E), ld(E), ptr(bias), ptr(labels), ptr(rows_dev),
         ptr(count), ptr(dloss), ptr(ws), ptr(dl), ld(dl), stream())


def graph_upload(graph):
    """hipGraphUpload of a captured torch.cuda.CUDAGraph's executable (rs_graph_upload) on the current stream."""
    call("rs_graph_upload", C.c_void_p(int(graph.raw_cuda_graph_exec())), stream())


def seed_advance(seed_base):
    call("rs_seed_advance", ptr(seed_base), stream())


# ---- fused SAS sublayers (rowchain.hip) ----------------------------------------------------
def sas_block_fused_ok(d, dtype):
    """rs_sas_block_in/out cover bf16 with d in {64, 128}; anything else runs the unfused kernels."""
    return dtype == torch.bfloat16 and d in (64, 128)


def sas_block_grid(M):
    """Workgroups the row-chain kernels launch for M rows = per-workgroup partial sets (LayerNorm affine partials,
    BCE partials, valid-position counts) they write."""
    return int(_lib.lib().rs_sas_block_grid(M))


sas_block_parts = sas_block_in_count_parts = sas_block_grid      # the names the partial-set count had per kernel


def sas_block_boundary_fused(M, d):
    """True where the block-boundary entries below run their one-launch kernels (every wave owns at most one
    tile); they launch the two single-block kernels otherwise."""
    return bool(_lib.lib().rs_sas_block_boundary_fused(M, d))


# The C entries take argument structs (include/recsys_hip.h documents the fields).  The wrappers below keep their
# tensor-level signatures; each argument group is mapped to its struct's field names in exactly one place:
def _sas_args(cls, **fields):
    return cls(**{k: ptr(v) if isinstance(v, torch.Tensor) else v for k, v in fields.items() if v is not None})


def _sas_in(x, ln_w, ln_b, eps, Q, mean, rstd, Wq, bq, q, Wkv, bkv, kv, embed=None):
    return _sas_args(_lib.SasInArgs, M=x.shape[0], x=x, ldx=ld(x), ln_w=ln_w, ln_b=ln_b, eps=eps, Q=Q, mean=mean,
                     rstd=rstd, Wq=Wq, bq=bq, q=q, Wkv=Wkv, bkv=bkv, kv=kv, e=embed)


def _sas_out(o, Q, Wo, bo, x1, ln_w, ln_b, eps, z, mean, rstd, W1, b1, h1, W2, b2, xn, ids, drop_p, salt1, salt2,
             seed_base, head=None):
    return _sas_args(_lib.SasOutArgs, M=o.shape[0], o=o, Q=Q, Wo=Wo, bo=bo, x1=x1, ln_w=ln_w, ln_b=ln_b, eps=eps,
                     z=z, mean=mean, rstd=rstd, W1=W1, b1=b1, h1=h1, W2=W2, b2=b2, xn=xn, ids=ids, drop_p=drop_p,
                     salt1=salt1, salt2=salt2, seed_base=seed_base, h=head)


def _sas_head(M, d, E, pos, neg, ln_w, ln_b, count_parts, divisor, f, pl, nl, dpl, dnl, dx, lnpart, part):
    G = sas_block_grid(M)
    assert part.numel() == 3 * G and lnpart.numel() >= 2 * d * G and count_parts.dtype == torch.int32
    return _sas_args(_lib.SasHeadArgs, E=E, pos=pos, neg=neg, ln_w=ln_w, ln_b=ln_b, count_parts=count_parts,
                     ncount=count_parts.numel(), divisor=divisor, f=f, pl=pl, nl=nl, dpl=dpl, dnl=dnl, dx=dx,
                     lnpart=lnpart, part=part)


def _sas_out_bwd(M, dxn, ids, h1, x1, mean2, rstd2, ln_w, W2T, W1T, WoT, dy2, da1, dx1, dout, part, drop_p, salt1,
                 salt2, seed_base, o=None, delta=None):
    return _sas_args(_lib.SasOutBwdArgs, M=M, dxn=dxn, ids=ids, h1=h1, x1=x1, mean2=mean2, rstd2=rstd2, ln_w=ln_w,
                     W2T=W2T, W1T=W1T, WoT=WoT, dy2=dy2, da1=da1, dx1=dx1, dout=dout, part=part, drop_p=drop_p,
                     salt1=salt1, salt2=salt2, seed_base=seed_base, o=o, delta=delta)


def _sas_in_bwd(dq, dkv, dx1, x, mean1, rstd1, ln_w, WinT, dx, part):
    return _sas_args(_lib.SasInBwdArgs, M=dq.shape[0], dq=dq, dkv=dkv, dx1=dx1, x=x, mean1=mean1, rstd1=rstd1,
                     ln_w=ln_w, WinT=WinT, ldwt=ld(WinT), dx=dx, part=part)


def sas_block_in(x, ln_w, ln_b, eps, Q, mean, rstd, Wq, bq, q, Wkv, bkv, kv):
    a = _sas_in(x, ln_w, ln_b, eps, Q, mean, rstd, Wq, bq, q, Wkv, bkv, kv)
    call("rs_sas_block_in", x.shape[1], C.byref(a), stream())


def sas_block_in_embed(ids, T, item_emb, pos_emb, scale, drop_p, salt, seed_base, x0, count_ids, count_parts,
                       ln_w, ln_b, eps, Q, mean, rstd, Wq, bq, q, Wkv, bkv, kv):
    """embed_fwd(_counted) (mode 0) + sas_block_in in one launch (rowchain); x0 receives the embedding output."""
    M, d = x0.shape
    assert ids.numel() == M and item_emb.dtype == torch.bfloat16 and x0.dtype == torch.bfloat16
    if count_parts is not None:
        assert count_parts.dtype == torch.int32 and count_parts.numel() >= sas_block_grid(M)
    e = _sas_args(_lib.SasEmbedArgs, ids=ids, item_emb=item_emb, pos_emb=pos_emb, T=T, scale=scale, drop_p=drop_p,
                  salt=salt, seed_base=seed_base, x0=x0, count_ids=count_ids, count_parts=count_parts)
    a = _sas_in(x0, ln_w, ln_b, eps, Q, mean, rstd, Wq, bq, q, Wkv, bkv, kv, embed=e)
    call("rs_sas_block_in", d, C.byref(a), stream())


def sas_block_in_attn_nsplit(d, B, T):
    """Workgroups per sequence of sas_block_in_attn for (d, B, T); 0 where it does not cover the shape."""
    return int(_lib.lib().rs_sas_block_in_attn_nsplit(d, B, T))


def sas_block_in_attn(ids, T, item_emb, pos_emb, scale, drop_p, salt, seed_base, x0, count_ids, count_parts,
                      ln_w, ln_b, eps, Q, mean, rstd, Wq, bq, q, Wkv, bkv, kv, o, lse, attn_scale, attn_salt):
    """sas_block_in_embed(...) + attn_fwd(q, k, v -> o, lse; one head, causal, dropout drop_p with attn_salt) in one
    launch (block_in_attn.hip), bit for bit; every slot of count_parts is written."""
    M, d = x0.shape
    assert ids.numel() == M and M % T == 0 and item_emb.dtype == torch.bfloat16 and x0.dtype == torch.bfloat16
    if count_parts is not None:
        assert count_parts.dtype == torch.int32
    e = _sas_args(_lib.SasEmbedArgs, ids=ids, item_emb=item_emb, pos_emb=pos_emb, T=T, scale=scale, drop_p=drop_p,
                  salt=salt, seed_base=seed_base, x0=x0, count_ids=count_ids, count_parts=count_parts)
    a = _sas_in(x0, ln_w, ln_b, eps, Q, mean, rstd, Wq, bq, q, Wkv, bkv, kv, embed=e)
    k = _sas_args(_lib.SasInAttnArgs, B=M // T, o=o, lse=lse, scale=attn_scale, drop_p=drop_p, salt=attn_salt,
                  ncount=0 if count_parts is None else count_parts.numel(), **{"in": a})
    call("rs_sas_block_in_attn", d, C.byref(k), stream())


def sas_block_out_head(out_args, E, pos, neg, lnl_w, lnl_b, count_parts, divisor, f, pl, nl, dpl, dnl, dx, lnpart,
                       part):
    """sas_block_out(*out_args) for the last block with the SAS head in the same launch (rowchain);
    lnpart [G][2][d], part [G][3] with G = sas_block_grid(M)."""
    M, d = out_args[0].shape
    h = _sas_head(M, d, E, pos, neg, lnl_w, lnl_b, count_parts, divisor, f, pl, nl, dpl, dnl, dx, lnpart, part)
    a = _sas_out(*out_args, head=h)
    call("rs_sas_block_out", d, C.byref(a), stream())


def sas_block_out(o, Q, Wo, bo, x1, ln_w, ln_b, eps, z, mean, rstd, W1, b1, h1, W2, b2, xn, ids, drop_p,
                  salt1, salt2, seed_base):
    a = _sas_out(o, Q, Wo, bo, x1, ln_w, ln_b, eps, z, mean, rstd, W1, b1, h1, W2, b2, xn, ids, drop_p, salt1, salt2,
                 seed_base)
    call("rs_sas_block_out", o.shape[1], C.byref(a), stream())


def sas_block_out_bwd(dxn, ids, h1, x1, mean2, rstd2, ln_w, W2T, W1T, WoT, dy2, da1, dx1, dout, part, drop_p, salt1,
                      salt2, seed_base, o=None, delta=None):
    """part: fp32 >= 2*d*sas_block_grid(M), receives the LN2 affine partials (ln_partial_segments).  o, delta
    (one-head attention output [M, d] bf16, fp32 [M]): also delta = rowsum(dout * o) for attn_bwd(delta_in=True)."""
    M, d = dxn.shape
    a = _sas_out_bwd(M, dxn, ids, h1, x1, mean2, rstd2, ln_w, W2T, W1T, WoT, dy2, da1, dx1, dout, part, drop_p, salt1,
                     salt2, seed_base, o, delta)
    call("rs_sas_block_out_bwd_delta", d, C.byref(a), stream())


def sas_block_in_bwd(dq, dkv, dx1, x, mean1, rstd1, ln_w, WinT, dx, part):
    a = _sas_in_bwd(dq, dkv, dx1, x, mean1, rstd1, ln_w, WinT, dx, part)
    call("rs_sas_block_in_bwd", dq.shape[1], C.byref(a), stream())


def sas_block_out_in(out_args, ln1_w, ln1_b, eps1, Qn, mean1, rstd1, Wq, bq, q, Wkv, bkv, kv):
    """sas_block_out(*out_args) of block i, then sas_block_in(xn, ...) of block i+1 on the tile in registers: one
    launch (rowchain), bitwise the two calls' results."""
    a = _sas_out(*out_args)
    # block i+1's input side on the same rows: the entry sets its x / ldx to the first chain's xn / d
    b = _sas_args(_lib.SasInArgs, M=a.M, ln_w=ln1_w, ln_b=ln1_b, eps=eps1, Q=Qn, mean=mean1, rstd=rstd1, Wq=Wq,
                  bq=bq, q=q, Wkv=Wkv, bkv=bkv, kv=kv)
    call("rs_sas_block_out_in", out_args[0].shape[1], C.byref(a), C.byref(b), stream())


def sas_block_in_out_bwd(in_args, dx, part1, out_args):
    """sas_block_in_bwd(*in_args, dx, part1) of block i, then sas_block_out_bwd(dx, *out_args) of block i-1 on the
    tile in registers: one launch (rowchain), bitwise the two calls' results except that dx is not written.  dx: the
    scratch of the two-launch path, None allowed where sas_block_boundary_fused(M, d)."""
    M, d = in_args[0].shape
    a = _sas_in_bwd(*in_args, dx, part1)
    b = _sas_out_bwd(M, None, *out_args)
    call("rs_sas_block_in_out_bwd", d, C.byref(a), C.byref(b), stream())


def sas_block_out_head_bwd(out_args, head_args, W2T, W1T, WoT, dy2, da1, dx1, dout, part2, delta=None):
    """sas_block_out_head(out_args, *head_args) of the last block, then that block's sas_block_out_bwd(dx, ids, h1,
    x1, mean, rstd, ln_w, W2T, W1T, WoT, dy2, da1, dx1, dout, part2, ..., o, delta) on the tile in registers: one
    launch (rowchain), bitwise the two calls' results except that dx is not written.  head_args' dx: the scratch of
    the two-launch path, None allowed where sas_block_boundary_fused(M, d)."""
    M, d = out_args[0].shape
    assert part2.numel() >= 2 * d * sas_block_grid(M)
    a = _sas_out(*out_args, head=_sas_head(M, d, *head_args))
    # the entry takes the saved tensors, mask, seeds and o of the backward from the forward's arguments
    b = _sas_args(_lib.SasOutBwdArgs, M=M, W2T=W2T, W1T=W1T, WoT=WoT, dy2=dy2, da1=da1, dx1=dx1, dout=dout,
                  part=part2, delta=delta)
    call("rs_sas_block_out_head_bwd", d, C.byref(a), C.byref(b), stream())


# ---- union-of-touched-rows table-gradient exchange (sparse_rows.hip) -------------------------
def touched_rows_ws_numel(rows):
    return int(_lib.lib().rs_touched_rows_ws_numel(rows))


def touched_rows(ids, rows, flags, index, count, ws):
    """flags/index int32[rows]: index[v] = rank of table row v among the rows occurring in ids (ascending), else
    -1; count int32[1] = their number (device-side, no sync)."""
    call("rs_touched_rows", ptr(ids), ids.numel(), rows, ptr(flags), ptr(index), ptr(count), ptr(ws), stream())


def rows_pack(src, index, count, compact):
    """compact[index[v]] = src[v] for the touched rows; compact rows [count, cap) = 0.  src fp32 [rows, d]."""
    rows, d = src.shape
    call("rs_rows_pack", ptr(src), rows, d, ptr(index), ptr(count), ptr(compact), compact.shape[0], stream())


def rows_unpack(dst, index, compact):
    """dst[v] = compact[index[v]] for the touched rows (the others are left as they are)."""
    rows, d = dst.shape
    call("rs_rows_unpack", ptr(dst), rows, d, ptr(index), ptr(compact), stream())


# ---- sparse (touched-rows-only) Adam of a table (adam_rows.hip) ------------------------------
def unique_rows_ws_bytes(table_rows):
    n = int(_lib.lib().rs_unique_rows_ws_bytes(int(table_rows)))
    if n < 0:
        raise ValueError("rs_unique_rows_ws_bytes: table_rows must be positive")
    return n


def _i32(t, name, numel=None):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous int32 tensor")
    if numel is not None and t.numel() != numel:
        raise ValueError(f"{name} must hold {numel} element(s), got {t.numel()}")


def unique_rows(keys, table_rows, rows, count, ws):
    """rows[:count] (int32 [cap], count int32 [1], both on the device; no sync) = the ascending distinct ids in
    [1, table_rows) of the one to three int64 key tensors `keys`; ids of 0 or >= table_rows are dropped, entries past
    count are unspecified.  cap >= the keys' total length; ws: uint8 [unique_rows_ws_bytes(table_rows)]."""
    keys = list(keys)
    if not 1 <= len(keys) <= 3:
        raise ValueError(f"unique_rows takes one to three key tensors, got {len(keys)}")
    for k in keys:
        if not isinstance(k, torch.Tensor) or k.dtype != torch.int64 or not k.is_contiguous():
            raise ValueError("unique_rows: every key tensor must be contiguous int64")
    table_rows = int(table_rows)
    if not 0 < table_rows < 2 ** 31:
        raise ValueError(f"unique_rows: table_rows must be in [1, 2^31), got {table_rows}")
    _i32(rows, "rows")
    _i32(count, "count", 1)
    total = sum(k.numel() for k in keys)
    if rows.numel() < max(total, 1):
        raise ValueError(f"unique_rows: rows holds {rows.numel()} ids but the keys number {total}")
    if ws.dtype != torch.uint8 or ws.numel() < unique_rows_ws_bytes(table_rows):
        raise ValueError(f"unique_rows: ws must be uint8 with at least {unique_rows_ws_bytes(table_rows)} bytes")
    kp = [(ptr(k) if k.numel() else None, k.numel()) for k in keys] + [(None, 0)] * (3 - len(keys))
    call("rs_unique_rows", kp[0][0], kp[0][1], kp[1][0], kp[1][1], kp[2][0], kp[2][1], table_rows, ptr(rows),
         ptr(count), rows.numel(), ptr(ws), ws.numel(), stream())


def adam_rows(rows, count, p, g, m, v, p_bf16, state, hyper, zero_grad=False, max_wg=None):
    """rs_adam_step's update on the rows rows[:count] (unique_rows' list: distinct ids) of the table p / g / m / v
    (fp32 [R, d] or [R], contiguous views of the flat buffers; p_bf16 its bf16 copy or None) and on no other row.
    The step's scalars must be prepared (after adam_prepare / adam_prepare_step of this step, same stream)."""
    _i32(rows, "rows")
    _i32(count, "count", 1)
    if p.dim() not in (1, 2):
        raise ValueError("adam_rows: the table must be [R, d] or [R]")
    R, d = p.shape[0], (p.shape[1] if p.dim() == 2 else 1)
    for name, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        if t.dtype != torch.float32 or t.shape != p.shape or not t.is_contiguous():
            raise ValueError(f"adam_rows: {name} must be contiguous fp32 of the table's shape {tuple(p.shape)}")
    if p_bf16 is not None and (p_bf16.dtype != torch.bfloat16 or p_bf16.shape != p.shape or not p_bf16.is_contiguous()):
        raise ValueError("adam_rows: p_bf16 must be a contiguous bf16 tensor of the table's shape")
    if R < 1 or d < 1 or rows.numel() < 1:
        raise ValueError("adam_rows: empty table or list")
    if rows.numel() * d >= 2 ** 31:
        raise ValueError("adam_rows: list capacity * row width must stay below 2^31")
    if max_wg is not None and int(max_wg) < 1:
        raise ValueError("adam_rows: max_wg must be positive")
    if state.dtype != torch.float64 or state.numel() < 4 or hyper.dtype != torch.float64 or hyper.numel() < 5:
        raise ValueError("adam_rows: state / hyper must be the optimizer's float64 device arrays")
    call("rs_adam_rows", d, R, ptr(rows), ptr(count), rows.numel(), ptr(p), ptr(g), ptr(m), ptr(v), ptr(p_bf16),
         ptr(state), ptr(hyper), int(zero_grad), int(max_wg or 8192), stream())


# ---- global gradient norm and clip coefficient (gradnorm.hip) --------------------------------
def gradnorm_dense_parts(n):
    """Partial slots rs_gradnorm_dense writes for one range of n elements."""
    k = int(_lib.lib().rs_gradnorm_dense_parts(int(n)))
    if k < 0:
        raise ValueError(f"gradnorm_dense_parts: a range needs n > 0, got {n}")
    return k


def gradnorm_rows_parts(d, cap):
    """Partial slots rs_gradnorm_rows writes for a list of capacity cap over rows of width d."""
    k = int(_lib.lib().rs_gradnorm_rows_parts(int(d), int(cap)))
    if k < 0:
        raise ValueError(f"gradnorm_rows_parts: needs d >= 1, cap >= 1 and cap * d < 2^31, got d={d}, cap={cap}")
    return k


def _gradnorm_partials(partials, need, who):
    if not isinstance(partials, torch.Tensor) or partials.dtype != torch.float64 or not partials.is_contiguous():
        raise ValueError(f"{who}: partials must be a contiguous float64 tensor")
    if partials.numel() < need:
        raise ValueError(f"{who}: partials holds {partials.numel()} slots, the launch writes {need}")


def gradnorm_dense(g, ranges, partials, max_wg=8192):
    """Double partial sums of squares of g[lo:hi] for every (lo, hi) of `ranges` (at most 8; lo % 4 == 0) into
    partials[0:k], range after range; returns k = sum of gradnorm_dense_parts(hi - lo).  g: contiguous fp32, 1-D."""
    if not isinstance(g, torch.Tensor) or g.dtype != torch.float32 or g.dim() != 1 or not g.is_contiguous():
        raise ValueError("gradnorm_dense: g must be a contiguous 1-D fp32 tensor")
    ranges = [(int(lo), int(hi)) for lo, hi in ranges]
    if not 1 <= len(ranges) <= 8:
        raise ValueError(f"gradnorm_dense takes one to eight ranges, got {len(ranges)}")
    for lo, hi in ranges:
        if lo < 0 or lo % 4 or hi <= lo or hi > g.numel():
            raise ValueError(f"gradnorm_dense: range ({lo}, {hi}) is empty, outside g or starts off a multiple of 4")
    if max_wg is None or int(max_wg) < 1:
        raise ValueError("gradnorm_dense: max_wg must be positive")
    need = sum(gradnorm_dense_parts(hi - lo) for lo, hi in ranges)
    _gradnorm_partials(partials, need, "gradnorm_dense")
    arr = (_lib.i64 * (2 * len(ranges)))(*[x for r in ranges for x in r])
    call("rs_gradnorm_dense", ptr(g), arr, len(ranges), int(max_wg), ptr(partials), stream())
    return need


def gradnorm_rows(g, rows, count, partials, max_wg=8192):
    """Double partial sums of squares of the rows rows[:count] (unique_rows' list) of the table g (fp32 [R, d] or [R],
    contiguous) and of no other row, into ALL of partials[0:k] (zeros where the list is short); returns k =
    gradnorm_rows_parts(d, rows.numel())."""
    _i32(rows, "rows")
    _i32(count, "count", 1)
    if not isinstance(g, torch.Tensor) or g.dtype != torch.float32 or g.dim() not in (1, 2) or not g.is_contiguous():
        raise ValueError("gradnorm_rows: the table must be contiguous fp32 [R, d] or [R]")
    R, d = g.shape[0], (g.shape[1] if g.dim() == 2 else 1)
    if R < 1 or d < 1 or rows.numel() < 1:
        raise ValueError("gradnorm_rows: empty table or list")
    if rows.numel() * d >= 2 ** 31:
        raise ValueError("gradnorm_rows: list capacity * row width must stay below 2^31")
    if max_wg is None or int(max_wg) < 1:
        raise ValueError("gradnorm_rows: max_wg must be positive")
    need = gradnorm_rows_parts(d, rows.numel())
    _gradnorm_partials(partials, need, "gradnorm_rows")
    call("rs_gradnorm_rows", ptr(g), d, R, ptr(rows), ptr(count), rows.numel(), int(max_wg), ptr(partials), stream())
    return need


def gradnorm_finish(partials, nparts, max_norm, record, div=None):
    """record (fp32 [>= 3]) = {norm, coef, effective divisor} from partials[:nparts]: norm = sqrt(sum) / div, coef =
    min(1, max_norm / (norm + 1e-6)); max_norm: float64 [1] on the device; div: fp32 [1] or None (1)."""
    nparts = int(nparts)
    if nparts < 1:
        raise ValueError("gradnorm_finish: nparts must be positive")
    _gradnorm_partials(partials, nparts, "gradnorm_finish")
    if not isinstance(max_norm, torch.Tensor) or max_norm.dtype != torch.float64 or max_norm.numel() < 1:
        raise ValueError("gradnorm_finish: max_norm must be a float64 device tensor")
    if not isinstance(record, torch.Tensor) or record.dtype != torch.float32 or record.numel() < 3 \
            or not record.is_contiguous():
        raise ValueError("gradnorm_finish: record must be a contiguous fp32 tensor of at least 3 elements")
    if div is not None and (div.dtype != torch.float32 or div.numel() < 1):
        raise ValueError("gradnorm_finish: div must be an fp32 device tensor")
    call("rs_gradnorm_finish", ptr(partials), nparts, ptr(div), ptr(max_norm), ptr(record), stream())


def ln_partial_segments(part, M, d, dgamma, dbeta, nb=None):
    """The two reduce segments of a fused kernel's LayerNorm partials (part[b][2][d], b < nb; default: the
    SAS row-block backward kernels' set count)."""
    nb = sas_block_grid(M) if nb is None else nb
    return [(part, 2 * d, nb, d, dgamma), (part[d:], 2 * d, nb, d, dbeta)]


def _segments(segs):
    arr = (_lib.ReduceSegment * max(1, len(segs)))()
    for i, (src, stride, splits, n, out) in enumerate(segs):
        arr[i] = _lib.ReduceSegment(ptr(src), stride, splits, n, ptr(out))
    return arr


def wgrad_grouped(problems, M, rows_per_split, slab, extra=(), pos=None, max_tile=256):
    ev = _ev_begin("wgrad_grouped")
    _wgrad_grouped(problems, M, rows_per_split, slab, extra, pos, max_tile)
    _ev_end(ev)


def _wgrad_grouped(problems, M, rows_per_split, slab, extra=(), pos=None, max_tile=256):
    """problems: [(dY, X, dW, db|None)] with dW [N][K] fp32 (+=); extra: reduce segments
    (src, stride, splits, n, out) summed (+=) in the same reduction launch.  pos: (ids, T, dx, drop_p, salt, seed_base, dpos) -- the SAS positional
    table's gradient (embed_bwd mode 0, scale 1, +=) then rides in the reduction launch (rs_wgrad_grouped_pos);
    pos + (head_part, divisor, loss_out): the SAS head's loss statistics too (rs_wgrad_grouped_pos_stats)."""
    arr = (_lib.WgradProblem * len(problems))()
    for i, (dY, X, dW, db) in enumerate(problems):
        N, K = dY.shape[1], X.shape[1]
        assert dW.numel() == N * K and dY.shape[0] >= M and X.shape[0] >= M
        arr[i] = _lib.WgradProblem(ptr(dY), ld(dY), ptr(X), ld(X), N, K, ptr(dW), ptr(db) if db is not None else None)
    segs = _segments(list(extra))
    if pos is not None:
        assert max_tile == 256, "the positional form takes the default tiles"
        ids, T, dx, drop_p, salt, seed_base, dpos, *st = pos
        if st:
            hp, hdiv, lout, *aux = st
            call("rs_wgrad_grouped_pos_stats", len(problems), arr, M, rows_per_split, ptr(slab), slab.numel(),
                 len(extra), segs, ptr(ids), T, ptr(dx), dx.shape[-1], drop_p, salt, ptr(seed_base), ptr(dpos),
                 ptr(hp), hp.numel() // 3, ptr(hdiv), ptr(lout), ptr(aux[0] if aux else None), stream())
            return
        call("rs_wgrad_grouped_pos", len(problems), arr, M, rows_per_split, ptr(slab), slab.numel(), len(extra),
             segs, ptr(ids), T, ptr(dx), dx.shape[-1], drop_p, salt, ptr(seed_base), ptr(dpos), stream())
        return
    call("rs_wgrad_grouped_max", len(problems), arr, M, rows_per_split, ptr(slab), slab.numel(), len(extra), segs,
         int(max_tile), stream())


def wgrad_grouped_tile(shapes, max_tile=256):
    """Output tile edge rs_wgrad_grouped uses for problems of these (N, K) shapes (256, 128 or 64; at most
    max_tile)."""
    arr = (_lib.WgradProblem * len(shapes))()
    for i, (N, K) in enumerate(shapes):
        arr[i] = _lib.WgradProblem(None, 0, None, 0, N, K, None, None)
    t = int(_lib.lib().rs_wgrad_grouped_tile_max(len(shapes), arr, int(max_tile)))
    if t <= 0:
        raise RuntimeError("rs_wgrad_grouped_tile: bad arguments")
    return t


def wgrad_grouped_slab_numel(shapes, M, rows_per_split):
    """shapes: [(N, K)] of the problems."""
    splits = -(-M // rows_per_split)
    return sum(splits * (N * K + N) for N, K in shapes)


def reduce_segments(segs, accumulate=True):
    call("rs_reduce_segments", len(segs), _segments(list(segs)), int(accumulate), stream())


def transpose_bf16(desc, max_tiles, src, dst):
    """desc: int64 device tensor [nmat][6] (rows, cols, src_off, lds, dst_off, ldd)."""
    call("rs_transpose_bf16", desc.shape[0], ptr(desc), max_tiles, ptr(src), ptr(dst), stream())


# ---- item-table gradient by inverted index (itemgrad.hip) ----------------------------------
def item_index_ws_bytes(nsrc, rows, table_rows, d):
    n = _lib.lib().rs_item_index_ws_bytes(nsrc, rows, table_rows, d)
    if n < 0:
        raise RuntimeError("rs_item_index_ws_bytes: bad arguments")
    return n


def item_index_build(keys, table_rows, d, ws):
    """keys: 1-3 int64 device tensors of the same numel (ids, pos, neg)."""
    rows = keys[0].numel()
    kp = [ptr(k) for k in keys] + [None] * (3 - len(keys))
    call("rs_item_index_build", len(keys), kp[0], kp[1], kp[2], rows, table_rows, d, ptr(ws), ws.numel(), stream())


def item_index_view(nsrc, rows, table_rows, d, ws):
    """(sorted keys, sorted entries, start, sort path) of a built index: views into ws (tests and tools); start
    (first sorted position of each key) exists on the counting-sort path only, else None."""
    out = (_lib.i64 * 4)()
    call("rs_item_index_layout", nsrc, rows, table_rows, d, out)
    n = nsrc * rows
    sk = ws[out[0]:out[0] + 4 * n].view(torch.int32)
    sv = ws[out[1]:out[1] + 4 * n].view(torch.int32)
    start = ws[out[2]:out[2] + 4 * (table_rows + 1)].view(torch.int32) if out[2] >= 0 else None
    return sk, sv, start, int(out[3])


def item_grad(ws, nsrc, rows, dx, scale, drop_p, salt, seed_base, f, w1, w2, dtable, marks=None, table_rows=None):
    """marks: (row_marks u8 [table_rows], epoch u8 [1]) -- rs_item_grad_marked stamps the rows it writes (bf16).
    table_rows: the key range the index was built with, where that is not the table's row count."""
    d = dtable.shape[1]
    table_rows = dtable.shape[0] if table_rows is None else table_rows
    if marks is not None and dx.dtype != torch.float32:
        call("rs_item_grad_marked", ptr(ws), nsrc, rows, table_rows, d, ptr(dx), scale, drop_p, salt, ptr(seed_base),
             ptr(f) if f is not None else None, ptr(w1) if w1 is not None else None,
             ptr(w2) if w2 is not None else None, ptr(dtable), ptr(marks[0]), ptr(marks[1]), stream())
        return
    # fp32 (the parity path): chunk + span kernels at any width; bf16: the LDS chunk kernels (d in {64, 128, 256})
    call("rs_item_grad_f32" if dx.dtype == torch.float32 else "rs_item_grad", ptr(ws), nsrc, rows, table_rows, d,
         ptr(dx), scale, drop_p, salt, ptr(seed_base),
         ptr(f) if f is not None else None, ptr(w1) if w1 is not None else None,
         ptr(w2) if w2 is not None else None, ptr(dtable), stream())


def gemm_n256_splits(M, K):
    return int(_lib.lib().rs_gemm_n256_splits(M, K))


def gemm_n256(A, B, C, a_kmajor, M, K, split=False, colsum=None, rows_dev=None):
    """C[m, :256] = sum_k A(m, k) B(k, :) fp32 (rs_gemm_n256).  A: bf16 2-D view, A(m, k) = A[k, m] (a_kmajor) or
    A[m, k]; B: bf16 (K, 256) rows (row stride ld(B)); C: fp32 rows of 256 (ld(C)); split: C is a [splits, M, 256]
    slab (one k slice each, gemm_n256_splits(M, K) of them)."""
    cz = C[0].numel() if split else 0
    Cm = C[0] if split else C
    call("rs_gemm_n256", int(a_kmajor), M, K, ptr(A), ld(A), ptr(B), ld(B), ptr(C), ld(Cm), int(split), cz,
         ptr(colsum), ptr(rows_dev), stream())


def candidate_scores(h, E, cand, bias=None):
    """(B, C) fp32 scores <h[b], E[cand[b, c]]> (+ bias[cand[b, c]]): rs_candidate_scores.  h: (B, d) rows (row stride
    may exceed d), E: (V, d) in h's dtype, cand: (B, C) int64 on the device; raises on an id outside [0, V) like
    the reference's embedding / gather."""
    B, d = h.shape
    V = E.shape[0]
    cand = cand.contiguous()
    if bool(((cand < 0) | (cand >= V)).any()):
        raise IndexError("candidate id out of range")
    out = torch.empty(cand.shape, dtype=torch.float32, device=h.device)
    call("rs_candidate_scores", dtype_code(h), ptr(h), h.stride(0), B, d, ptr(E), ptr(bias), ptr(cand), cand.shape[1], V,
         ptr(out), stream())
    return out


# ---- fused SAS output head (head.hip) --------------------------------------------------------
def sas_head_fwd(x, ln_w, ln_b, eps, f, mean, rstd, E, pos, neg, pl, nl, part):
    M, d = x.shape
    call("rs_sas_head_fwd", M, d, ptr(x), ptr(ln_w), ptr(ln_b), eps, ptr(f), ptr(mean), ptr(rstd), ptr(E), ptr(pos),
         ptr(neg), ptr(pl), ptr(nl), ptr(part), stream())


def sas_head_bwd(part, divisor, out, pl, nl, dpl_in, dnl_in, dpl, dnl, pos, neg, E, x, ln_w, mean, rstd, dx, lnpart):
    M, d = x.shape
    call("rs_sas_head_bwd", M, d, ptr(part), ptr(divisor), ptr(out), ptr(pl), ptr(nl), ptr(dpl_in), ptr(dnl_in),
         ptr(dpl), ptr(dnl), ptr(pos), ptr(neg), ptr(E), ptr(x), ptr(ln_w), ptr(mean), ptr(rstd), ptr(dx),
         ptr(lnpart), stream())


# ---- SAS tied full-catalogue CE head: the row kernels (sas_ce.hip) --------------------------
def sas_ce_rows_ok(d, dtype):
    """The widths rs_sas_ce_rows_fwd / _bwd cover (the fused engine's: bf16, d in {64, 128})."""
    return dtype == torch.bfloat16 and d in (64, 128)


def sas_ce_rows_fwd(x, labels, cap, ln_w, ln_b, eps, idx, rank, count, hl, lab, mean, rstd, divisor=None):
    """compact_rows(labels) + the last LayerNorm on the valid rows of x only + gather, one launch: hl [cap][d],
    lab [cap], mean / rstd [cap] per compact row; rows >= count are left untouched.  divisor (fp32 [1]): receives
    max(count, 1), the CE mean's divisor."""
    M, d = x.shape
    assert labels.numel() == M and hl.shape[0] >= cap and rank.numel() >= M and idx.numel() >= cap
    call("rs_sas_ce_rows_fwd", dtype_code(x), M, d, ptr(x), ld(x), ptr(labels), cap, ptr(ln_w), ptr(ln_b), eps,
         ptr(idx), ptr(rank), ptr(count), ptr(divisor), ptr(hl), ld(hl), ptr(lab), ptr(mean), ptr(rstd), stream())


def sas_ce_rows_nparts(M):
    """LayerNorm affine partial sets sas_ce_rows_bwd leaves for M rows (host only)."""
    return int(_lib.lib().rs_sas_ce_rows_nparts(M))


def sas_ce_rows_bwd(slab, splits, cap, rank, x, ln_w, mean, rstd, dx, part):
    """Split-K sum of dh (slab fp32 [splits][cap][d], fixed order) + LayerNorm backward + scatter to all rows of dx
    (zeros at invalid rows); part [nparts][2][d]: the affine partials (ln_partial_segments(nb=nparts))."""
    M, d = x.shape
    assert slab.numel() >= splits * cap * d and part.numel() >= 2 * d * sas_ce_rows_nparts(M)
    assert dx.shape == (M, d) and rank.numel() >= M
    call("rs_sas_ce_rows_bwd", dtype_code(x), M, d, ptr(slab), splits, cap, ptr(rank), ptr(x), ld(x), ptr(ln_w),
         ptr(mean), ptr(rstd), ptr(dx), ld(dx), ptr(part), stream())


# ---- SAS sampled-softmax head over batch-shared candidates (sas_sce.hip) --------------------
def sas_sce_max_k():
    """Most candidates the sampled-softmax head takes (host only)."""
    return int(_lib.lib().rs_sas_sce_max_k())


def sas_sce_ok(d, dtype):
    """The dtypes / widths rs_sas_sce_fwd / _bwd cover: fp32 at any d <= 1024, bf16 at d % 8 == 0, d <= 1024 (the
    MFMA sweep up to d = 128, a plain kernel past it)."""
    return d <= 1024 and (dtype == torch.float32 or (dtype == torch.bfloat16 and d % 8 == 0))


def sas_sce_ws_numel(cap, K, d):
    """fp32 elements of the head's workspace (lse, z0, the dEc split slabs): a function of (cap, K, d) alone."""
    n = int(_lib.lib().rs_sas_sce_ws_bytes(cap, K, d))
    if n < 0:
        raise RuntimeError("rs_sas_sce_ws_bytes: bad arguments")
    return n // 4


def sas_sce_dh_splits(cap, K, d):
    """Slabs rs_sas_sce_bwd writes dh in (one per split of the candidates; host only)."""
    return int(_lib.lib().rs_sas_sce_dh_splits(cap, K, d))


def sas_sce_fwd(hl, lab, count, cap, E, cand, divisor, ws, out):
    """lse / z0 per compact row into ws, out = {loss sum, valid rows, sum / divisor} (rs_sas_sce_fwd)."""
    d, K = hl.shape[1], cand.numel()
    assert hl.shape[0] >= cap and lab.numel() >= cap and E.dtype == hl.dtype and E.shape[1] == d and E.is_contiguous()
    assert cand.dtype == torch.int64 and cand.is_contiguous() and ws.numel() >= sas_sce_ws_numel(cap, K, d)
    call("rs_sas_sce_fwd", dtype_code(hl), cap, d, ptr(hl), ld(hl), ptr(lab), ptr(count), ptr(E), E.shape[0], ptr(cand),
         K, ptr(divisor), ptr(ws), ptr(out), stream())


def sas_sce_bwd(hl, lab, count, cap, E, cand, divisor, dloss, ws, dh, coef, pg, dEc, keys=None):
    """dh fp32 [sas_sce_dh_splits][cap][d], coef [cap], pg = coef * hl [cap][d], dEc fp32 [K][d], keys int64
    [cap + K] (rs_sas_sce_bwd)."""
    d, K = hl.shape[1], cand.numel()
    assert dh.numel() >= sas_sce_dh_splits(cap, K, d) * cap * d and coef.numel() >= cap and pg.numel() >= cap * d and dEc.numel() >= K * d
    assert keys is None or (keys.numel() >= cap + K and keys.dtype == torch.int64)
    assert ws.numel() >= sas_sce_ws_numel(cap, K, d) and E.shape[1] == d and E.is_contiguous()
    call("rs_sas_sce_bwd", dtype_code(hl), cap, d, ptr(hl), ld(hl), ptr(lab), ptr(count), ptr(E), E.shape[0], ptr(cand),
         K, ptr(divisor), ptr(dloss), ptr(ws), ptr(dh), ptr(coef), ptr(pg), ptr(dEc), ptr(keys), stream())


# ---- the sampled-softmax head for an untied output layer with a bias (sas_sce.hip: rs_sce_head_*) -----------
def sce_head_path(d, dtype):
    """1: the MFMA sweep (fp32 d <= 128, bf16 d <= 256), 0: the plain kernel, < 0: unsupported (host only)."""
    return int(_lib.lib().rs_sce_head_path(_lib.BF16 if dtype == torch.bfloat16 else
                                           (_lib.F32 if dtype == torch.float32 else -1), d))


def sce_head_ws_numel(cap, K, d, dtype, has_bias=True):
    """fp32 elements of the head's workspace: a function of (dtype, cap, K, d, bias or not) alone (host only)."""
    n = int(_lib.lib().rs_sce_head_ws_bytes(_lib.BF16 if dtype == torch.bfloat16 else _lib.F32, cap, K, d,
                                            int(has_bias)))
    if n < 0:
        raise RuntimeError("rs_sce_head_ws_bytes: bad arguments")
    return n // 4


def sce_head_dh_splits(cap, K, d, dtype):
    """Slabs rs_sce_head_bwd writes dh in (one per split of the candidates; host only)."""
    return int(_lib.lib().rs_sce_head_dh_splits(_lib.BF16 if dtype == torch.bfloat16 else _lib.F32, cap, K, d))


def _sce_head_bias(bias, E):
    assert bias is None or (bias.dtype == torch.float32 and bias.shape == (E.shape[0],) and bias.is_contiguous())


def _sce_head_logq(logq, E):
    assert logq.dtype == torch.float32 and logq.shape == (E.shape[0],) and logq.is_contiguous()
    assert logq.device == E.device


def sce_head_fwd(hl, lab, count, cap, E, bias, cand, divisor, ws, out, logq=None):
    """sas_sce_fwd on the logits <h, E[.]> + bias[.] (bias fp32 [V1] or None): rs_sce_head_fwd.  logq (fp32 [V1]):
    the logits are <h, E[.]> + bias[.] - logq[.], the proposal's correction (rs_sce_head_logq_fwd)."""
    d, K = hl.shape[1], cand.numel()
    assert hl.shape[0] >= cap and lab.numel() >= cap and E.dtype == hl.dtype and E.shape[1] == d and E.is_contiguous()
    assert cand.dtype == torch.int64 and cand.is_contiguous()
    assert ws.numel() >= sce_head_ws_numel(cap, K, d, hl.dtype, bias is not None)
    _sce_head_bias(bias, E)
    if logq is not None:
        _sce_head_logq(logq, E)
        call("rs_sce_head_logq_fwd", dtype_code(hl), cap, d, ptr(hl), ld(hl), ptr(lab), ptr(count), ptr(E), ptr(bias),
             ptr(logq), E.shape[0], ptr(cand), K, ptr(divisor), ptr(ws), ptr(out), stream())
        return
    call("rs_sce_head_fwd", dtype_code(hl), cap, d, ptr(hl), ld(hl), ptr(lab), ptr(count), ptr(E), ptr(bias),
         E.shape[0], ptr(cand), K, ptr(divisor), ptr(ws), ptr(out), stream())


def sce_head_bwd(hl, lab, count, cap, E, bias, cand, divisor, dloss, ws, dh, coef, pg, dEc, dbc, keys=None,
                 logq=None):
    """sas_sce_bwd's outputs on those logits, and dbc fp32 [K] (with a bias; None without): rs_sce_head_bwd.  logq:
    as in sce_head_fwd (rs_sce_head_logq_bwd); it gets no gradient and does not change what dbc is tied to."""
    d, K = hl.shape[1], cand.numel()
    assert dh.numel() >= sce_head_dh_splits(cap, K, d, hl.dtype) * cap * d and coef.numel() >= cap
    assert pg.numel() >= cap * d and dEc.numel() >= K * d
    assert keys is None or (keys.numel() >= cap + K and keys.dtype == torch.int64)
    assert ws.numel() >= sce_head_ws_numel(cap, K, d, hl.dtype, bias is not None)
    assert E.shape[1] == d and E.is_contiguous() and E.dtype == hl.dtype
    _sce_head_bias(bias, E)
    assert (dbc is None) == (bias is None) and (dbc is None or (dbc.dtype == torch.float32 and dbc.numel() >= K))
    if logq is not None:
        _sce_head_logq(logq, E)
        call("rs_sce_head_logq_bwd", dtype_code(hl), cap, d, ptr(hl), ld(hl), ptr(lab), ptr(count), ptr(E), ptr(bias),
             ptr(logq), E.shape[0], ptr(cand), K, ptr(divisor), ptr(dloss), ptr(ws), ptr(dh), ptr(coef), ptr(pg),
             ptr(dEc), ptr(dbc), ptr(keys), stream())
        return
    call("rs_sce_head_bwd", dtype_code(hl), cap, d, ptr(hl), ld(hl), ptr(lab), ptr(count), ptr(E), ptr(bias),
         E.shape[0], ptr(cand), K, ptr(divisor), ptr(dloss), ptr(ws), ptr(dh), ptr(coef), ptr(pg), ptr(dEc), ptr(dbc),
         ptr(keys), stream())


def uniform_items(seed_base, salt, item_num, out):
    """out (int64, device): uniform draws with replacement over [1, item_num] from (seed_base, salt)."""
    call("rs_uniform_items", ptr(seed_base), salt, item_num, out.numel(), ptr(out), stream())


def alias_items(seed_base, salt, table, out):
    """out (int64, device): draws with replacement over [1, V] from the packed alias table (int64 [V], device:
    ItemProposal.table) and (seed_base, salt): rs_alias_items."""
    assert table.dtype == torch.int64 and table.dim() == 1 and table.is_contiguous() and table.device == out.device
    assert out.dtype == torch.int64 and out.is_contiguous()
    call("rs_alias_items", ptr(seed_base), salt, ptr(table), table.numel(), out.numel(), ptr(out), stream())


# ---- SAS head with N negatives per position: multi-negative BCE / gBCE (sas_gbce.hip) -----------------------
def sas_gbce_max_n():
    """Most negatives per position the head takes (rs_sas_gbce_max_n: 1024)."""
    return int(_lib.lib().rs_sas_gbce_max_n())


def sas_gbce_ok(d, dtype):
    """The dtypes / widths rs_sas_gbce_fwd / _bwd cover: fp32 at any d <= 1024, bf16 at d % 8 == 0, d <= 1024."""
    return 1 <= d <= 1024 and (dtype == torch.float32 or (dtype == torch.bfloat16 and d % 8 == 0))


def sas_gbce_ws_numel(cap, N, d):
    """fp32 elements of the head's workspace (the logits [cap][1 + N] and the loss partials; host only)."""
    n = int(_lib.lib().rs_sas_gbce_ws_bytes(cap, N, d))
    if n < 0:
        raise RuntimeError("rs_sas_gbce_ws_bytes: bad arguments")
    return -(-n // 4)


def _gbce_args(hl, lab, idx, count, cap, E, neg, N, ws):
    d = hl.shape[1]
    assert hl.shape[0] >= cap and lab.numel() >= cap and lab.dtype == torch.int64 and E.dtype == hl.dtype
    assert idx is None or (idx.dtype == torch.int32 and idx.numel() >= cap)
    assert neg.dtype == torch.int64 and neg.is_contiguous() and neg.numel() % N == 0
    assert idx is not None or neg.numel() >= cap * N
    assert ws.dtype == torch.float32 and ws.numel() >= sas_gbce_ws_numel(cap, N, d)
    assert E.shape[1] == d and E.is_contiguous()
    return d


def sas_gbce_fwd(hl, lab, idx, count, cap, E, neg, N, beta, divisor, ws, out):
    """The logits z [cap][1 + N] into ws, out = {loss sum, valid rows, sum / divisor, negative-term sum}
    (rs_sas_gbce_fwd).  neg: int64, N per source row, read as neg[idx[r] * N + j] (idx None: identity)."""
    d = _gbce_args(hl, lab, idx, count, cap, E, neg, N, ws)
    assert out.dtype == torch.float32 and out.numel() >= 4
    call("rs_sas_gbce_fwd", dtype_code(hl), cap, d, ptr(hl), ld(hl), ptr(lab), ptr(idx), ptr(count), ptr(E),
         E.shape[0], ptr(neg), N, float(beta), ptr(divisor), ptr(ws), ptr(out), stream())


def sas_gbce_bwd(hl, lab, idx, count, cap, E, neg, N, beta, divisor, dloss, ws, dh, w, keys):
    """dh fp32 [cap][d], the weights w fp32 [cap][1 + N], keys int64 [cap * (1 + N)] (rs_sas_gbce_bwd)."""
    d = _gbce_args(hl, lab, idx, count, cap, E, neg, N, ws)
    assert dh.dtype == torch.float32 and dh.is_contiguous() and dh.numel() >= cap * d
    assert w.dtype == torch.float32 and w.is_contiguous() and w.numel() >= cap * (1 + N)
    assert keys.dtype == torch.int64 and keys.is_contiguous() and keys.numel() >= cap * (1 + N)
    call("rs_sas_gbce_bwd", dtype_code(hl), cap, d, ptr(hl), ld(hl), ptr(lab), ptr(idx), ptr(count), ptr(E),
         E.shape[0], ptr(neg), N, float(beta), ptr(divisor), ptr(dloss), ptr(ws), ptr(dh), ptr(w), ptr(keys), stream())


def item_grad_weighted(ws, rows, per, f, w, dtable, table_rows=None):
    """dtable[key_e] += sum_e w[e] * f[e // per] over the index built on rows * per keys (item_index_build([keys], ...)):
    rs_item_grad_weighted.  f: fp32 / bf16 (rows, d) rows (row stride may exceed d), w fp32 [rows * per].
    table_rows: the key range the index was built with, where that is not the table's row count."""
    d = dtable.shape[1]
    assert f.shape[0] >= rows and f.shape[1] == d and f.stride(1) == 1
    assert w.dtype == torch.float32 and w.is_contiguous() and w.numel() >= rows * per
    assert dtable.dtype == torch.float32 and dtable.is_contiguous()
    call("rs_item_grad_weighted", ptr(ws), dtype_code(f), rows, per,
         dtable.shape[0] if table_rows is None else table_rows, d, ptr(f), ld(f), ptr(w), ptr(dtable), stream())


def sas_sample_negs(user_offsets, user_items, n_users, item_num, seed_base, salt, seq, pos, neg):
    """rs_sas_sample_negs: the next batch with neg int64 (batch, max_len, n_negs)."""
    B, T = seq.shape
    assert neg.dim() == 3 and neg.shape[:2] == (B, T) and neg.dtype == torch.int64 and neg.is_contiguous()
    call("rs_sas_sample_negs", ptr(user_offsets), ptr(user_items), n_users, item_num, B, T, ptr(seed_base), salt,
         neg.shape[2], ptr(seq), ptr(pos), ptr(neg), stream())


def sas_head_finish(part, divisor, out):
    """Loss statistics out[0..3] from the head's BCE partials part[nblk][3] (one workgroup)."""
    call("rs_sas_head_finish", part.numel() // 3, ptr(part), ptr(divisor), ptr(out), stream())


# ---- on-device sampler and ranking metrics (sampler.hip) -----------------------------------
def sas_sample(user_offsets, user_items, n_users, item_num, seed_base, salt, seq, pos, neg, draws=None):
    """draws (optional, tests): int64 (batch, 1 + 256 * max_len) record of the draws (rs_sas_sample_draws)."""
    B, T = seq.shape
    if draws is not None:
        call("rs_sas_sample_draws", ptr(user_offsets), ptr(user_items), n_users, item_num, B, T, ptr(seed_base), salt,
             ptr(seq), ptr(pos), ptr(neg), ptr(draws), stream())
        return
    call("rs_sas_sample", ptr(user_offsets), ptr(user_items), n_users, item_num, B, T, ptr(seed_base), salt,
         ptr(seq), ptr(pos), ptr(neg), stream())


def bert_mask(offsets, items, n_users, num_items, mask_prob, perm, state, salt, tokens, labels, draws=None):
    """rs_bert_mask: the next (tokens, labels) batch into (batch, max_len) int64 device tensors; draws (optional,
    tests): int64 (batch, 1 + 2 * max_len) record of the draws (rs_bert_mask_draws)."""
    B, T = tokens.shape
    if draws is not None:
        call("rs_bert_mask_draws", ptr(offsets), ptr(items), n_users, num_items, B, T, mask_prob, ptr(perm),
             ptr(state), salt, ptr(tokens), ptr(labels), ptr(draws), stream())
        return
    call("rs_bert_mask", ptr(offsets), ptr(items), n_users, num_items, B, T, mask_prob, ptr(perm), ptr(state), salt,
         ptr(tokens), ptr(labels), stream())


def rank_metrics(scores, labels, ks_dev, ws, out):
    R, C = scores.shape
    call("rs_rank_metrics", ptr(scores), ptr(labels), R, C, ks_dev.numel(), ptr(ks_dev), ptr(ws), ptr(out), stream())


# ---- evaluation loader: per-user negatives and eval batches (eval_loader.hip) ----------------
def eval_negs_max():
    return int(_lib.lib().rs_eval_negs_max())


def eval_negatives_max_draws():
    return int(_lib.lib().rs_eval_negatives_max_draws())


def eval_negatives(seen_offsets, seen_sorted, item_num, seed, negs, table=None, n_drawn=None, draws=None, user0=0,
                   count=None):
    """negs (int32 (n_users, n_neg), device) rows [user0, user0 + count) <- the seeded per-user negatives of
    rs_eval_negatives: seen_offsets int64 (n_users + 1,), seen_sorted int32 (each user's whole history, ascending,
    unique), table None (uniform) or ItemProposal.table, n_drawn int32 (n_users,) optional, draws (tests) int64
    (n_users, eval_negatives_max_draws()) record of the raw stream (rs_eval_negatives_draws)."""
    n_users, n_neg = negs.shape
    count = n_users - user0 if count is None else count
    assert seen_offsets.dtype == torch.int64 and seen_offsets.numel() == n_users + 1 and seen_offsets.is_contiguous()
    assert seen_sorted.dtype == torch.int32 and seen_sorted.is_contiguous()
    assert negs.dtype == torch.int32 and negs.is_contiguous() and 0 <= user0 and user0 + count <= n_users
    assert n_drawn is None or (n_drawn.dtype == torch.int32 and n_drawn.numel() == n_users and n_drawn.is_contiguous())
    assert table is None or (table.dtype == torch.int64 and table.numel() == item_num and table.is_contiguous())
    seed = int(seed) & (2 ** 64 - 1)
    if draws is not None:
        assert draws.dtype == torch.int64 and draws.is_contiguous()
        assert draws.shape == (n_users, eval_negatives_max_draws())
        call("rs_eval_negatives_draws", ptr(seen_offsets), ptr(seen_sorted), user0, count, item_num, n_neg, seed,
             ptr(table), ptr(negs), ptr(n_drawn), ptr(draws), stream())
        return
    call("rs_eval_negatives", ptr(seen_offsets), ptr(seen_sorted), user0, count, item_num, n_neg, seed, ptr(table),
         ptr(negs), ptr(n_drawn), stream())


def eval_batch(hist_offsets, hist_items, extra, answer, negs, user0, mask_token, seq, cand, labels):
    """rs_eval_batch: the rows of the users [user0, user0 + B) into seq (B, T), cand and labels (B, 1 + n_neg), int64
    device tensors.  extra None (validation) or the per-user validation item (test); mask_token 0 (SAS) or [MASK]."""
    n_users, n_neg = negs.shape
    B, T = seq.shape
    assert hist_offsets.dtype == torch.int64 and hist_offsets.numel() == n_users + 1 and hist_items.dtype == torch.int64
    assert answer.dtype == torch.int64 and answer.numel() == n_users and negs.dtype == torch.int32
    assert extra is None or (extra.dtype == torch.int64 and extra.numel() == n_users)
    assert 0 <= user0 and user0 + B <= n_users and cand.shape == (B, 1 + n_neg) and labels.shape == (B, 1 + n_neg)
    assert all(t.dtype == torch.int64 and t.is_contiguous() for t in (seq, cand, labels)) and negs.is_contiguous()
    call("rs_eval_batch", ptr(hist_offsets), ptr(hist_items), ptr(extra), ptr(answer), ptr(negs), user0, B, T, n_neg,
         mask_token, ptr(seq), ptr(cand), ptr(labels), stream())


# ---- full-catalogue ranking and top-K (fullrank.hip) ----------------------------------------
RS_TOPK_MAX = 128


def _full_args(h, E, bias, lo, hi, exclude):
    B, d = h.shape
    hi = E.shape[0] if hi is None else int(hi)
    lo = int(lo)
    if not 0 <= lo < hi <= E.shape[0]:
        raise ValueError(f"item range [{lo}, {hi}) outside the table's [0, {E.shape[0]})")
    if E.dtype != h.dtype or h.stride(1) != 1 or E.stride(1) != 1:
        raise TypeError("h and E: rows of one dtype with unit element stride")
    nx = 0
    if exclude is not None and exclude.numel():
        # the sweep binary-searches each row's list per vocabulary tile: sorted rows (rs_full_rank's contract)
        exclude = torch.sort(exclude.reshape(B, -1).to(torch.int64), dim=1).values.contiguous()
        nx = exclude.shape[1]
    else:
        exclude = None
    return B, d, lo, hi, exclude, nx


def full_ws(h, lo, hi, k):
    """uint8 workspace of rs_full_ws_bytes for h's (B, d) against the item range [lo, hi) (k = 0: full_rank)."""
    B, d = h.shape
    n = int(_lib.lib().rs_full_ws_bytes(dtype_code(h), B, d, hi - lo, k))
    return torch.empty(max(n, 256), dtype=torch.uint8, device=h.device)


def full_rank(h, E, target, bias=None, lo=1, hi=None, exclude=None, return_scores=False, check=True):
    """int32 (B,) rank of target[b] among the admissible items of [lo, hi) (hi: E's rows): the number of items v, not
    in exclude[b] (int64 (B, n); zeros and ids outside the range are ignored; the target itself always stays), with
    <h[b], E[v]> (+ bias[v]) above the target's score, or equal to it and v < target[b]: rs_full_rank.  h: (B, d)
    rows (row stride may exceed d), E: (V, d) in h's dtype.  Raises IndexError for a target outside [lo, hi); with
    check=False (no host read: inside a graph capture) such a row ranks -1 instead."""
    B, d, lo, hi, exclude, nx = _full_args(h, E, bias, lo, hi, exclude)
    target = target.to(torch.int64).contiguous()
    if check and bool(((target < lo) | (target >= hi)).any()):
        raise IndexError("target id outside the item range")
    ws = full_ws(h, lo, hi, 0)
    rank = torch.empty(B, dtype=torch.int32, device=h.device)
    ts = torch.empty(B, dtype=torch.float32, device=h.device) if return_scores else None
    call("rs_full_rank", dtype_code(h), ptr(h), h.stride(0), B, d, ptr(E), E.stride(0), ptr(bias), lo, hi,
         ptr(target), ptr(exclude), nx, nx, ptr(ws), ptr(rank), ptr(ts), stream())
    return (rank, ts) if return_scores else rank


def full_topk(h, E, k, bias=None, lo=1, hi=None, exclude=None):
    """(ids int64 (B, k), scores fp32 (B, k)): per row the k best admissible items of [lo, hi), by score descending
    and id ascending among equal scores: rs_full_topk.  Past the number of admissible items: id -1, score -inf."""
    k = int(k)
    if not 1 <= k <= RS_TOPK_MAX:
        raise ValueError(f"k must be in 1..{RS_TOPK_MAX}, got {k}")
    B, d, lo, hi, exclude, nx = _full_args(h, E, bias, lo, hi, exclude)
    ws = full_ws(h, lo, hi, k)
    ids = torch.empty((B, k), dtype=torch.int64, device=h.device)
    scores = torch.empty((B, k), dtype=torch.float32, device=h.device)
    call("rs_full_topk", dtype_code(h), ptr(h), h.stride(0), B, d, ptr(E), E.stride(0), ptr(bias), lo, hi,
         ptr(exclude), nx, nx, k, ptr(ws), ptr(ids), ptr(scores), stream())
    return ids, scores


def rank_to_metrics(rank, ks_dev, ws, out):
    """out[3q + {0, 1, 2}] = mean Recall / NDCG / MRR @ ks_dev[q] of int32 ranks (one positive per row; -1: a miss);
    ws: >= 3 * nk * rows floats (rs_rank_to_metrics)."""
    call("rs_rank_to_metrics", ptr(rank), rank.numel(), ks_dev.numel(), ptr(ks_dev), ptr(ws), ptr(out), stream())
