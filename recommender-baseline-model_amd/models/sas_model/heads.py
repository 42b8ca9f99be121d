"""The row heads of SASRec's tied losses (ce, sampled_ce, gbce): what a loss does between SASEngine._valid_rows_forward
(the blocks' forward, then the last LayerNorm on the compacted rows with pos != 0) and _valid_rows_backward.  Called by
SASEngine.rows_forward / rows_backward:

    extras(batch, logq) -> extra              the head's own tensors of a training step's batch (seq, pos, third)
    prepare(eng, ids, pos, *extra) -> extra   the refusals that need no row count, before the first launch (gBCE's
                                              rows * (1 + N) < 2^31: in forward, once cap is known); extras normalised
    forward(eng, c, extra, loss_out)          the launches on c (_valid_rows_forward's dict: cap, cnt, hl, lab, div ...);
                                              stores in c what backward (and tools/sas_*_bench.py) read
    backward(eng, s, grad, dloss)             the launches on the current stream, c = s["ce"]
        -> (slab_d, sk, table_grad)           dh on the compact rows, fp32 [sk][cap][d], and None or a zero-argument
                                              callable: the launches that depend on the head alone (its rows of the item
                                              table's gradient, by an inverted index of their own: one writer per row,
                                              fixed order).  _valid_rows_backward decides where they run.

packs_with_seq: True iff the batch's third tensor has seq's shape (one packed buffer; a graph may unroll steps); else it
has third_shape(batch shape, sampler) and steps_per_graph > 1 is refused with unroll_refusal.  The buffers are the
engine's workspace, sized by (cap, K or N, d) alone: nothing here allocates per step or reads the host."""
import math

import torch

from ... import ops
from ...engine_util import SCE_INDEX_ROWS, check_logq


def check_width(eng, display, ok=None):
    d, dt = eng.d, eng.dt
    if dt == torch.bfloat16 and d % 8:
        raise ValueError(f"the bf16 {display} head needs hidden units divisible by 8 (got {d}); "
                         "use fp32 mode (rs_dtype='fp32') at this width")
    if ok is not None and not ok(d, dt):
        raise ValueError(f"the {display} head covers hidden units up to 1024 (got {d})")


def index_rows(table_rows):
    """The key range of a head's own item index: at least past the counting sort's table limit, so that the radix path
    is taken and the workspace is sized by the entry count alone (the counting sort's histograms are sized by the
    table)."""
    return max(table_rows, SCE_INDEX_ROWS)


def gbce_beta(n_negs, num_items, t):
    """gSASRec's positive-term power for n_negs sampled negatives out of num_items items at calibration t:

        alpha = min(1, n_negs / (num_items - 1))        the sampling rate of the negatives
        beta  = alpha * (t * (1 - 1 / alpha) + 1 / alpha)

    t = 0 gives 1 (plain multi-negative BCE), t = 1 gives alpha (fully calibrated), and beta falls linearly from 1 to
    alpha in between.  n_negs >= num_items - 1 clamps alpha (and beta) to 1."""
    n_negs, num_items, t = int(n_negs), int(num_items), float(t)
    if n_negs < 1 or num_items < 2:
        raise ValueError("gbce_beta needs n_negs >= 1 and num_items >= 2")
    if not 0.0 <= t <= 1.0:
        raise ValueError(f"gbce_beta: t must lie in [0, 1], got {t}")
    alpha = min(1.0, n_negs / (num_items - 1))
    # the formula above with the product multiplied out, alpha t + (1 - t): exactly 1 at t = 0 and alpha at t = 1
    # (alpha * (1 / alpha) need not round to 1)
    return alpha * t + (1.0 - t)


class CEHead:
    """CrossEntropy(ignore_index=0) of the logits against the whole item table (tied; class 0 is the zero padding row),
    never materialised in bf16 (SAS.ce_loss has the definition).  The table's gradient is dense: dlogits^T f over all
    rows (rs_linear_wgrad's fixed-order split-K, row 0 cleared afterwards: the padding row gets no gradient), written
    on the main stream BEFORE the blocks' backward; no table_grad."""
    name, display, packs_with_seq = "ce", "cross-entropy", True

    def extras(self, batch, logq):
        return ()

    def prepare(self, eng, ids, pos):
        check_width(eng, self.display)
        return ()

    def forward(self, eng, c, extra, loss_out):
        f32, g = torch.float32, eng.ws.get
        cap, V1, cnt, hl, lab, div = (c[k] for k in ("cap", "V1", "cnt", "hl", "lab", "div"))
        E = eng.W("item_emb.weight")
        if eng.dt == torch.bfloat16:
            wce = g("ce_vce", (ops.vocab_ce_ws_numel(cap, V1),), f32)
            fwd = ops.vocab_head_fwd if ops.vocab_head_supported(eng.d) else ops.vocab_ce_fwd
            fwd(hl, E, None, lab, wce, loss_out, rows_dev=cnt, count_override=div)
            dl = None
        else:
            dl = g("ce_logits", (cap, c["V1p"]), f32)[:, :V1]          # the logits, then dlogits in place
            ops.linear_fwd(hl, E, dl, rows_dev=cnt)
            wce = g("ce_wce", (3 * cap,), f32)
            ops.ce_fwd(dl, lab, wce, loss_out, div, rows_dev=cnt)
        c.update(wce=wce, dl=dl)

    def backward(self, eng, s, grad, dloss):
        c = s["ce"]
        d, dt = eng.d, eng.dt
        f32, g = torch.float32, eng.ws.get
        cap, V1, cnt, hl, lab = c["cap"], c["V1"], c["cnt"], c["hl"], c["lab"]
        E = eng.W("item_emb.weight")
        if dt == torch.bfloat16:
            dl = g("ce_dlogits", (cap, c["V1p"]), dt)[:, :V1]     # the one (cap, V+1) buffer of the bf16 path
            bwd = ops.vocab_head_bwd if ops.vocab_head_supported(d) else ops.vocab_ce_bwd
            bwd(hl, E, None, lab, c["wce"], c["div"], dl, rows_dev=cnt, dloss=dloss)
        else:
            dl = c["dl"]
            ops.ce_bwd(dl, lab, c["div"], dloss, c["wce"], dl, rows_dev=cnt)
        GE = eng.flat.view("item_emb.weight", grad)
        slab = g("ce_slab_dE", (ops.wgrad_slab_numel(cap, V1, d),), f32)
        ops.linear_wgrad(dl, hl, GE, slab, rows_dev=cnt, accumulate=True)
        GE[0].zero_()                              # class 0 is the padding row: no gradient (padding_idx)
        # dh = dlogits E: a contraction over the whole catalogue with few rows -- split-K into fp32 slabs
        sk = int(max(1, min(64, -(-V1 // 2048))))
        slab_d = g("ce_slab_dh", (sk * cap * d,), f32)
        ops.gemm(dl, E, slab_d, cap, d, V1, False, True, ops.epilogue(rows_dev=cnt), split_k=sk, slab=slab_d)
        c.update(dlogits=dl, slab_dE=slab, slab_dh=slab_d, dh_splits=sk)
        return slab_d, sk, None


class SampledCEHead:
    """The softmax cross-entropy of the positive against K candidates shared by every row (sas_sce.hip; extras: cand
    int64 [K], id 0 and a row's own positive masked, and logq fp32 [V + 1] or None, the proposal's correction,
    subtracted from every logit by the rs_sce_head_logq_* entries; SAS.sampled_ce_loss has the definition).
    table_grad: coef_r f_r at row pos_r and dEc[j] at row cand_j, through rs_item_index_build over the cap + K keys
    and rs_item_grad_f32 (duplicates summed in sorted-entry order)."""
    name, display, packs_with_seq = "sampled_ce", "sampled-softmax", False
    unroll_refusal = ("loss='sampled_ce' needs steps_per_graph = 1: cand has another shape than seq / pos, "
                      "and the unrolled graph takes one packed buffer")

    def third_shape(self, shape, sampler):
        K = getattr(sampler, "shared_negs", None)
        if not K:
            raise ValueError("loss='sampled_ce' needs a sampler with shared_negs=K")
        return (K,)

    def extras(self, batch, logq):
        return batch[2], logq

    def prepare(self, eng, ids, pos, cand, logq=None):
        check_width(eng, self.display, ops.sas_sce_ok)
        cand = cand.reshape(-1).contiguous()
        K, kmax = cand.numel(), ops.sas_sce_max_k()
        if K < 1 or K > kmax:
            raise ValueError(f"the sampled-softmax head takes 1 .. {kmax} shared candidates, got {K}")
        return cand, check_logq(logq, eng.W("item_emb.weight"))

    def forward(self, eng, c, extra, loss_out):
        cand, logq = extra
        E = eng.W("item_emb.weight")
        ws = eng.ws.get("sce_ws", (ops.sas_sce_ws_numel(c["cap"], cand.numel(), eng.d),), torch.float32)
        if logq is None:
            ops.sas_sce_fwd(c["hl"], c["lab"], c["cnt"], c["cap"], E, cand, c["div"], ws, loss_out)
        else:                                           # the same workspace: rs_sce_head_ws_bytes without a bias
            ops.sce_head_fwd(c["hl"], c["lab"], c["cnt"], c["cap"], E, None, cand, c["div"], ws, loss_out, logq=logq)
        c.update(cand=cand, sce_ws=ws, logq=logq)

    def backward(self, eng, s, grad, dloss):
        c = s["ce"]
        d = eng.d
        f32, g = torch.float32, eng.ws.get
        cap, cnt, hl, lab, cand = c["cap"], c["cnt"], c["hl"], c["lab"], c["cand"]
        K = cand.numel()
        E, GE = eng.W("item_emb.weight"), eng.flat.view("item_emb.weight", grad)
        sk = ops.sas_sce_dh_splits(cap, K, d)          # one fp32 slab per split of the candidates
        dh, coef = g("sce_dh", (sk, cap, d), f32), g("sce_coef", (cap,), f32)
        src, keys = g("sce_src", (cap + K, d), f32), g("sce_keys", (cap + K,), torch.int64)
        if c["logq"] is None:
            ops.sas_sce_bwd(hl, lab, cnt, cap, E, cand, c["div"], dloss, c["sce_ws"], dh, coef, src[:cap], src[cap:],
                            keys)
        else:
            ops.sce_head_bwd(hl, lab, cnt, cap, E, None, cand, c["div"], dloss, c["sce_ws"], dh, coef, src[:cap],
                             src[cap:], None, keys, logq=c["logq"])
        rows = index_rows(GE.shape[0])
        iws = g("sce_itemidx", (ops.item_index_ws_bytes(1, cap + K, rows, d),), torch.uint8)
        c.update(dh=dh, coef=coef, src=src, keys=keys, iws=iws, index_rows=rows)

        def table_grad():
            ops.item_index_build([keys], rows, d, iws)
            ops.item_grad(iws, 1, cap + K, src, 1.0, 0.0, 0, s["sb"], None, None, None, GE, table_rows=rows)
        return dh, sk, table_grad


class GBCEHead:
    """The BCE of the positive (weighted by beta) and the row's own N negatives neg[b, t, :] (sas_gbce.hip; extra: neg
    int64 (B, T, N), or (B, T) as N = 1, read in place through the compaction's source-row index; SAS.gbce_loss has the
    definition).  loss_out[3] = the negative-term sum.  table_grad: g_rj f_r at rows pos_r and neg_rj, through
    rs_item_index_build over the cap * (1 + N) head entries and rs_item_grad_weighted (no [entries][d] buffer)."""
    name, display, packs_with_seq = "gbce", "gBCE", False
    unroll_refusal = ("loss='gbce' needs steps_per_graph = 1: neg has another shape than seq / pos, and the "
                      "unrolled graph takes one packed buffer")

    def __init__(self, beta, negs=None):
        """beta: the positive term's weight; negs: the N every batch must have (a training step's), None = any."""
        self.beta, self.negs = float(beta), negs

    @classmethod
    def for_step(cls, sas, beta):
        """A training step's head: N = the model's args.sas_negs; beta None = gbce_beta(N, num_items,
        args.sas_gbce_t)."""
        negs = int(getattr(sas, "sas_negs", 0) or 0)
        if negs < 1:
            raise ValueError("FusedTrainStep(loss='gbce') needs the model's args.sas_negs = N >= 1")
        if beta is None:
            beta = gbce_beta(negs, sas.item_num, getattr(sas, "sas_gbce_t", 0.0))
        if isinstance(beta, bool) or not isinstance(beta, (int, float)) or not math.isfinite(beta) or beta < 0:
            raise ValueError(f"gbce_beta must be a finite number >= 0, got {beta!r}")
        return cls(beta, negs)

    def third_shape(self, shape, sampler):
        return shape + (self.negs,)

    def extras(self, batch, logq):
        return (batch[2],)

    def prepare(self, eng, ids, pos, neg):
        B, T = ids.shape
        if self.negs is not None:
            if neg is None or neg.dim() not in (2, 3) or tuple(neg.shape[:2]) != (B, T):
                raise ValueError(f"loss='gbce' needs neg of shape (B, T, N) with (B, T) = {(B, T)}")
            n = 1 if neg.dim() == 2 else neg.shape[2]
            if n != self.negs:
                raise ValueError(f"loss='gbce': the batch has {n} negs per position, the model's sas_negs is "
                                 f"{self.negs}")
        check_width(eng, self.display, ops.sas_gbce_ok)
        if neg.dim() == 2:
            neg = neg.unsqueeze(-1)
        if neg.dim() != 3 or tuple(neg.shape[:2]) != (B, T):
            raise ValueError(f"neg must be (B, T, N) or (B, T) = {(B, T)}, got {tuple(neg.shape)}")
        N, nmax = neg.shape[2], ops.sas_gbce_max_n()
        if N < 1 or N > nmax:
            raise ValueError(f"the gBCE head takes 1 .. {nmax} negatives per position, got {N}")
        return (neg if neg.is_contiguous() else neg.contiguous(),)

    def forward(self, eng, c, extra, loss_out):
        neg, = extra
        cap, N = c["cap"], neg.shape[2]
        if cap * (1 + N) >= 2 ** 31:
            raise ValueError(f"the gBCE head needs rows * (1 + N) < 2^31 (got {cap} rows, N = {N})")
        # the compaction's source rows (rs_compact_rows' idx, which _valid_rows_forward filled); the dense fp32 form
        # runs on all rows: identity
        idx = None if c["dense"] else eng.ws.get("ce_idx", (cap,), torch.int32)
        ws = eng.ws.get("gbce_ws", (ops.sas_gbce_ws_numel(cap, N, eng.d),), torch.float32)
        ops.sas_gbce_fwd(c["hl"], c["lab"], idx, c["cnt"], cap, eng.W("item_emb.weight"), neg, N, self.beta, c["div"],
                         ws, loss_out)
        c.update(neg=neg, N=N, beta=self.beta, idx=idx, gbce_ws=ws)

    def backward(self, eng, s, grad, dloss):
        c = s["ce"]
        d = eng.d
        f32, g = torch.float32, eng.ws.get
        cap, N, hl = c["cap"], c["N"], c["hl"]
        n = cap * (1 + N)
        GE = eng.flat.view("item_emb.weight", grad)
        dh, w = g("gbce_dh", (1, cap, d), f32), g("gbce_w", (n,), f32)
        keys = g("gbce_keys", (n,), torch.int64)
        ops.sas_gbce_bwd(hl, c["lab"], c["idx"], c["cnt"], cap, eng.W("item_emb.weight"), c["neg"], N, c["beta"],
                         c["div"], dloss, c["gbce_ws"], dh, w, keys)
        rows = index_rows(GE.shape[0])
        iws = g("gbce_itemidx", (ops.item_index_ws_bytes(1, n, rows, d),), torch.uint8)
        c.update(dh=dh, w=w, keys=keys, iws=iws, index_rows=rows)

        def table_grad():
            ops.item_index_build([keys], rows, d, iws)
            ops.item_grad_weighted(iws, cap, 1 + N, hl, w, GE, table_rows=rows)
        return dh, 1, table_grad


HEADS = {"ce": CEHead, "sampled_ce": SampledCEHead, "gbce": GBCEHead}
