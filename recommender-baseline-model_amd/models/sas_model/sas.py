"""SASRec on the MI355X HIP path.

Same constructor arguments, parameter modules, initialisation and
``state_dict`` keys as the reference ``BS/models/sas_model/sas.py:23-57`` (the
torch modules below are only parameter containers and initialisers: they never
run), same ``forward``/``predict`` results (``sas.py:59-118``).  The math runs
as HIP kernels through the C ABI, orchestrated by :class:`SASEngine`:

bf16 fused step (FusedTrainStep, d in {64, 128}: the benchmarked path) -- per block two row-chain kernels per
direction (rowchain.hip: one workgroup per CU, the block's three d x d weights in LDS, each wave carrying 16-token
tiles through the sublayer chain in registers) around the LDS-resident attention (attention_lds.hip):
  x = emb*sqrt(d)+pos, drop, mask;  Q = LN1(x);      rs_sas_block_in (first block: with rs_sas_embed_args)
                                                     (one head, two or more attention workgroups per sequence: the
                                                     first block's chain and attention in rs_sas_block_in_attn)
  q = Q Wq^T+bq;  kv = x Wkv^T+bkv                   (same launch; sas.py:59-67, 73-76)
  o = attn(q, k, v) causal, dropout on P             rs_attn_fwd (mask_kind 0; sas.py:75)
  x1 = Q + o Wo^T + bo;  z = LN2(x1);                rs_sas_block_out (sas.py:75-84, PointWiseFeedForward)
  x = (drop(relu(drop(z W1^T+b1)) W2^T+b2) + z)*m    (same launch)
  f = LN(x); pl/nl = <f, E[pos/neg]>; BCE + grads   rs_sas_block_out with rs_sas_head_args (the last block)
backward: rs_sas_block_out_bwd_delta -> rs_attn_bwd (dQ and dK/dV workgroups in one launch) ->
rs_sas_block_in_bwd per block (between two blocks one launch carries both adjacent row chains: rs_sas_block_out_in
forward, rs_sas_block_in_out_bwd backward; in the fused training step the last block's output chain, the head and
that block's output-side backward are one launch too: rs_sas_block_out_head_bwd), then ONE grouped launch of every
weight / bias / LayerNorm-affine gradient
(rs_wgrad_grouped_pos_stats, with the positional table's gradient and the loss statistics) beside the item-table
gradient by inverted index (rs_item_index_build on a side stream during the forward, rs_item_grad), then the fused
Adam (rs_adam_prepare_step_loss).
The tied losses are row heads (heads.py) between rows_forward / rows_backward's shared halves.
loss="ce" (CEHead): the blocks without the in-block head, then on the rows with pos != 0 only
rs_sas_ce_rows_fwd -> rs_vocab_head_fwd / _bwd against the whole item table (tied) -> rs_linear_wgrad (dE) -> rs_gemm
(dh) -> rs_sas_ce_rows_bwd, and the blocks' backward with the item index over the input ids alone.
loss="sampled_ce" (SampledCEHead): the same, with the vocabulary kernels replaced by the sampled-softmax
head over K candidates shared by the batch (sas_sce.hip): rs_sas_sce_fwd -> rs_sas_sce_bwd (dh, the positives'
coefficients, dEc) -> rs_item_index_build + rs_item_grad_f32 over the cap + K head keys -> rs_sas_ce_rows_bwd.
loss="gbce" (GBCEHead): the same valid-row front and back halves around the per-row gather head for
N negatives per position (sas_gbce.hip): rs_sas_gbce_fwd -> rs_sas_gbce_bwd (dh, the weights w, the keys) ->
rs_item_index_build + rs_item_grad_weighted over the cap * (1 + N) head entries -> rs_sas_ce_rows_bwd.
fp32 parity mode and other widths run the generic unfused kernels: rs_embed_fwd, rs_layernorm_fwd/bwd (variant 0,
eps 1e-8), rs_gemm (MFMA, fused bias / ReLU / dropout / residual / row-mask epilogues), rs_attn_fwd/bwd,
rs_sampled_logits_fwd/bwd, rs_bce_*, split-K weight gradients.
"""
import math
import os

import torch
import torch.nn as nn

from ... import ops
from ...engine_util import (SCE_INDEX_ROWS, SideBranch, Workspace, as_ids, compute_dtype,  # noqa: F401 (re-exported)
                            neg_dist_args, require_cuda, site_salt)
from ...flat import FlatParams
from .heads import CEHead, GBCEHead, SampledCEHead, gbce_beta  # noqa: F401 (gbce_beta: re-exported)

LN_EPS = 1e-8
SAS_LOSSES = ("bce", "ce", "sampled_ce")
# losses with per-position negatives beyond the reference's one: accepted alongside SAS_LOSSES
SAS_NEG_LOSSES = ("gbce",)


class PointWiseFeedForward(nn.Module):
    """Parameter container mirroring ``sas.py:6-14`` (conv1 / conv2 = Conv1d(d, d, 1))."""

    def __init__(self, hidden_units, dropout_rate):
        super().__init__()
        self.conv1 = nn.Conv1d(hidden_units, hidden_units, kernel_size=1)
        self.conv2 = nn.Conv1d(hidden_units, hidden_units, kernel_size=1)
        self.dropout_rate = dropout_rate


class SAS(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.item_num = args.num_items
        self.device = args.device
        self.max_len = args.max_len
        self.hidden = args.sas_hidden_units
        self.num_blocks = args.sas_num_blocks
        self.heads = args.sas_heads
        self.dropout_rate = args.sas_dropout
        # the trainer's l2 regulariser weight (BS/trainers/sas.py:14,51-52), applied by FusedTrainStep
        self.l2_emb = float(getattr(args, "l2_emb", 0.0) or 0.0)
        # the training objective FusedTrainStep takes by default: "bce" (the reference's one sampled negative per
        # position), "ce" (softmax cross-entropy over the whole catalogue, the item table tied as output layer) or
        # "sampled_ce" (the same softmax over the positive and sas_shared_negs candidates shared by the batch)
        self.sas_loss = str(getattr(args, "sas_loss", None) or "bce")
        if self.sas_loss not in SAS_LOSSES and self.sas_loss not in SAS_NEG_LOSSES:
            raise ValueError(f"sas_loss must be one of {SAS_LOSSES + SAS_NEG_LOSSES}, got {self.sas_loss!r}")
        # sas_loss="gbce": sas_negs = N negatives per position (required), sas_gbce_t = the calibration t in [0, 1]
        # (0: plain multi-negative BCE, beta = 1; 1: beta = alpha; gbce_beta has the formula)
        self.sas_negs = int(getattr(args, "sas_negs", 0) or 0)
        self.sas_gbce_t = float(getattr(args, "sas_gbce_t", 0.0) or 0.0)
        if self.sas_loss == "gbce":
            if self.sas_negs < 1:
                raise ValueError("sas_loss='gbce' needs args.sas_negs = N >= 1 (the negatives per position)")
            if not 0.0 <= self.sas_gbce_t <= 1.0:
                raise ValueError(f"sas_gbce_t must lie in [0, 1], got {self.sas_gbce_t}")
        # sas_loss="sampled_ce": the number of candidates (negatives shared by the whole batch) per step
        self.sas_shared_negs = int(getattr(args, "sas_shared_negs", 0) or 0)
        if self.sas_loss == "sampled_ce" and self.sas_shared_negs < 1:
            raise ValueError("sas_loss='sampled_ce' needs args.sas_shared_negs = K > 0 (the shared candidates)")
        # the proposal the shared candidates are drawn from: "uniform", or "popular" (an ItemProposal over the
        # training counts ** sas_neg_alpha, handed to the sampler; the loss then takes its logq correction)
        self.sas_neg_dist, self.sas_neg_alpha = neg_dist_args(args, "sas", self.sas_loss)
        self.cdtype = compute_dtype(args)
        d = self.hidden
        if d % self.heads:
            raise ValueError("sas_hidden_units must be divisible by sas_heads")

        self.item_emb = nn.Embedding(self.item_num + 1, d, padding_idx=0)
        self.pos_emb = nn.Embedding(args.max_len, d)
        self.attention_layernorms = nn.ModuleList()
        self.attention_layers = nn.ModuleList()
        self.forward_layernorms = nn.ModuleList()
        self.forward_layers = nn.ModuleList()
        self.last_layernorm = nn.LayerNorm(d, eps=LN_EPS)
        for _ in range(self.num_blocks):
            self.attention_layernorms.append(nn.LayerNorm(d, eps=LN_EPS))
            self.attention_layers.append(nn.MultiheadAttention(d, self.heads, self.dropout_rate))
            self.forward_layernorms.append(nn.LayerNorm(d, eps=LN_EPS))
            self.forward_layers.append(PointWiseFeedForward(d, self.dropout_rate))

        self._flat = None
        self._engine = None
        if torch.device(self.device).type == "cuda":
            self.to(self.device)

    # ---- flat-buffer management ------------------------------------------------------
    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        p = next(self.parameters())
        self._flat = FlatParams(self, p.device) if p.device.type == "cuda" else None
        self._engine = None
        return self

    def engine(self):
        p = self.item_emb.weight
        require_cuda(p.device)
        if self._flat is None or not self._flat.is_bound(self):
            self._flat = FlatParams(self, p.device)
            self._engine = None
        if self._engine is None:
            self._engine = SASEngine(self, self._flat)
        return self._engine

    # ---- reference API ---------------------------------------------------------------
    def forward(self, log_seqs, pos_seqs, neg_seqs):
        eng = self.engine()
        dev = self._flat.device
        ids, pos, neg = as_ids(log_seqs, dev), as_ids(pos_seqs, dev), as_ids(neg_seqs, dev)
        params = [p for _, p in self.named_parameters()]
        return _SASFunction.apply(eng, ids, pos, neg, self.training, *params)

    def _rows_loss(self, head, log_seqs, pos_seqs, own_ids=(), rest=()):
        """A row head's loss (heads.py); own_ids: the head's own id tensors (cand / neg), rest: its other extras."""
        eng = self.engine()
        dev = self._flat.device
        ids, pos = as_ids(log_seqs, dev), as_ids(pos_seqs, dev)
        extra = (*(as_ids(x, dev) for x in own_ids), *rest)
        params = [p for _, p in self.named_parameters()]
        return _SASRowsFunction.apply(eng, head, ids, pos, extra, self.training, *params)

    def ce_loss(self, log_seqs, pos_seqs):
        """Scalar loss of the tied full-catalogue objective (differentiable; available whatever sas_loss says):

            f = last_layernorm(log2feats(seq));  logits = f @ item_emb.weight.T      # (B, T, V+1), class 0 = padding
            loss = F.cross_entropy(logits.view(-1, V+1), pos.view(-1), ignore_index=0)

        the mean over the positions with pos != 0.  The padding row of the item table gets no gradient.  A batch
        with no valid position gives loss 0 and all-zero gradients (torch gives NaN there).  The head's buffers are
        the engine's workspace: call backward() before the next ce_loss()."""
        return self._rows_loss(CEHead(), log_seqs, pos_seqs)

    def sampled_ce_loss(self, log_seqs, pos_seqs, cand, logq=None):
        """Scalar loss of the sampled softmax over batch-shared candidates (differentiable; available whatever
        sas_loss says).  cand: int64 (K,), ids in [0, V], shared by every position:

            f_r   = last_layernorm(log2feats(seq))[r]          for every position r with pos_r != 0 ("valid")
            z_r0  = <f_r, E[pos_r]>                            E = item_emb.weight (tied)
            z_rj  = <f_r, E[cand_j]>,  j = 1..K
            live(r, j) = cand_j != 0 and cand_j != pos_r       id 0 = an ignored slot; accidental hits masked
            loss  = (1 / max(n, 1)) * sum_valid r [ log(exp(z_r0) + sum_{live j} exp(z_rj)) - z_r0 ],   n = #valid

        Duplicate candidates count separately; with cand = arange(1, V + 1) it is
        ce_loss up to the padding class 0 (logit exactly 0), which ce_loss counts and no candidate list can name.
        A row with no live candidate, and a batch with no valid row, give loss 0 and zero gradients; row 0 of the
        item table gets no gradient.  Call backward() before the next loss call.

        logq: fp32 (V + 1,) on the device, the log of the distribution the candidates were drawn from
        (ItemProposal.logq): the logQ correction, z_r0 -= logq[pos_r] and z_rj -= logq[cand_j].  It is a constant
        of the loss (no gradient); entry 0 is never read.  None: no correction."""
        return self._rows_loss(SampledCEHead(), log_seqs, pos_seqs, (cand,), (logq,))

    def gbce_loss(self, log_seqs, pos_seqs, neg_seqs, beta=1.0):
        """Scalar loss of the reference's BCE with N negatives per position, the positive term weighted by beta
        (gSASRec's generalised BCE; differentiable; available whatever sas_loss says).  neg_seqs: int64 (B, T, N), ids
        in [0, V]; (B, T) is taken as N = 1:

            valid r : pos_r != 0,  n = #valid
            z_r0    = <f_r, E[pos_r]>,   z_rj = <f_r, E[neg_rj]>, j = 1..N      f = last_layernorm(log2feats(seq)),
                                                                                E = item_emb.weight (tied)
            loss    = (1 / max(n, 1)) * sum_valid r [ beta * softplus(-z_r0) + sum_j softplus(z_rj) ]

        The negatives are summed, not averaged: N = 1, beta = 1 is the reference's loss (forward + BCE) term for term.
        A negative id 0 is the zero row (logit 0: softplus(0) in the loss, no table gradient); nothing is masked; equal
        ids in a row are separate terms; a batch with no valid row gives loss 0 and zero gradients; row 0 of the item
        table gets no gradient.  beta is a plain float (gbce_beta gives gSASRec's).  Call backward() before the next
        loss call."""
        return self._rows_loss(GBCEHead(beta), log_seqs, pos_seqs, (neg_seqs,))

    def log2feats(self, log_seqs):
        eng = self.engine()
        ids = as_ids(log_seqs, self._flat.device)
        with torch.no_grad():
            return eng.features(ids).clone()

    @torch.no_grad()
    def predict(self, log_seqs, item_indices):
        eng = self.engine()
        dev = self._flat.device
        return eng.predict(as_ids(log_seqs, dev), as_ids(item_indices, dev))

    @torch.no_grad()
    def recommend(self, log_seqs, k, exclude_seen=True):
        """(ids int64 (B, k), scores fp32 (B, k)) on the device: the k best items of the whole catalogue for each
        history, best first (equal scores: lower id first), without the history's own items when exclude_seen."""
        eng = self.engine()
        return eng.topk(as_ids(log_seqs, self._flat.device), k, exclude_seen)

    @torch.no_grad()
    def full_rank(self, log_seqs, target, exclude_seen=True):
        """int32 (B,) rank of target[b] among all items (0 = first), seen items left out when exclude_seen."""
        eng = self.engine()
        dev = self._flat.device
        return eng.full_rank(as_ids(log_seqs, dev), as_ids(target, dev).reshape(-1), exclude_seen)


class _SASFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, engine, ids, pos, neg, training, *params):
        engine.sync_compute_weights()
        pl, nl, saved = engine.forward(ids, pos, neg, training)
        ctx.engine = engine
        ctx.saved = saved
        return pl, nl

    @staticmethod
    def backward(ctx, dpl, dnl):
        eng = ctx.engine
        grad = torch.zeros(eng.flat.numel, dtype=torch.float32, device=eng.flat.device)
        eng.backward(ctx.saved, dpl.contiguous().float(), dnl.contiguous().float(), grad)
        ctx.saved = None
        grads = [eng.flat.view(n, grad) for n in eng.flat.names]
        return (None, None, None, None, None, *grads)


class _SASRowsFunction(torch.autograd.Function):
    """The loss of a row head (heads.py) through SASEngine.rows_forward / rows_backward."""

    @staticmethod
    def forward(ctx, engine, head, ids, pos, extra, training, *params):
        engine.sync_compute_weights()
        out = torch.zeros(4, dtype=torch.float32, device=engine.dev)
        ctx.saved = engine.rows_forward(head, ids, pos, extra, training, out)
        ctx.engine = engine
        return out[2].clone()

    @staticmethod
    def backward(ctx, dloss):
        eng = ctx.engine
        grad = torch.zeros(eng.flat.numel, dtype=torch.float32, device=eng.flat.device)
        eng.rows_backward(ctx.saved, grad, dloss=dloss.contiguous().float().reshape(1))
        ctx.saved = None
        grads = [eng.flat.view(n, grad) for n in eng.flat.names]
        return (None, None, None, None, None, None, *grads)


class SASEngine:
    """Owns workspaces and issues the HIP kernels of one SAS model."""

    def __init__(self, model: SAS, flat: FlatParams):
        self.m = model
        self.flat = flat
        self.d = model.hidden
        self.L = model.num_blocks
        self.H = model.heads
        self.Dh = self.d // self.H
        self.p = float(model.dropout_rate)
        self.dt = model.cdtype
        self.dev = flat.device
        if self.dt == torch.bfloat16:
            flat.enable_bf16()
        self.ws = Workspace(self.dev)
        # the item index and the transposed weights beside the forward, the item table's gradient beside the grouped
        # weight gradients, the sampled-softmax head's table rows beside the blocks' backward
        self.side = SideBranch(self.dev)
        self._side_refreshed = False
        self.seed_base = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self.external_seed = False    # True: the fused train step's optimizer advances seed_base
        # True: the fused train step's optimizer also writes the transposed bf16 block weights (transposed_spec),
        # so the forward's side branch builds only the item index and the backward needs no join for it
        self.adam_transposes = False
        self._wT = None
        # the block-boundary launches (rs_sas_block_out_in, rs_sas_block_in_out_bwd: two adjacent row chains in one
        # kernel); RS_SAS_BOUNDARY_FUSE=0 selects the composed launches they replace (A/B timing, bitwise tests)
        self.boundary_fuse = os.environ.get("RS_SAS_BOUNDARY_FUSE", "1") != "0"
        # the forward/backward turnaround launch (rs_sas_block_out_head_bwd: the last block's output chain, the head
        # and that block's output-side backward in one kernel); RS_SAS_TURNAROUND_FUSE=0 selects the two launches
        self.turnaround_fuse = os.environ.get("RS_SAS_TURNAROUND_FUSE", "1") != "0"
        # block 0's input chain and attention forward in one launch (rs_sas_block_in_attn) where it applies;
        # RS_SAS_IN_ATTN_FUSE=0 selects the two launches
        self.in_attn_fuse = os.environ.get("RS_SAS_IN_ATTN_FUSE", "1") != "0"
        salt0 = int(torch.randint(0, 2 ** 62, (1,)).item())
        self.salt = {"emb": site_salt(salt0, 0)}
        for i in range(self.L):
            self.salt[f"attn{i}"] = site_salt(salt0, 1 + 4 * i)
            self.salt[f"ffn1_{i}"] = site_salt(salt0, 2 + 4 * i)
            self.salt[f"ffn2_{i}"] = site_salt(salt0, 3 + 4 * i)

    # compute-dtype weights
    def sync_compute_weights(self):
        f = self.flat
        if f.bf16 is not None:
            if not f.stale:
                ops.cast_bf16(f.data, f.bf16)
            else:   # the compute copy of stale master rows (a sharded item table) is the current one: keep it
                a = 0
                for lo, hi in sorted(f.stale) + [(f.numel, f.numel)]:
                    if lo > a:
                        ops.cast_bf16(f.data[a:lo], f.bf16[a:lo])
                    a = max(a, hi)
            if self._wT is not None:
                self._refresh_transposed()

    def transposed_spec(self):
        """(desc, host desc, destination) of the backward's transposed block weights, for an optimizer that
        writes them itself (rs_adam_prepare_step; adam_transposes=True), or None before they exist."""
        if not self.adam_transposes or self._wT is None:
            return None
        return self._wT_desc, self._wT_desc_host, self._wT

    def W(self, n):
        return self.flat.cview(n)

    def Wf(self, n):
        return self.flat.view(n)

    def _buf(self, name, shape, dtype=None):
        return torch.empty(shape, dtype=dtype or self.dt, device=self.dev)

    # ---- forward -------------------------------------------------------------------
    def forward(self, ids, pos, neg, training, need_logits=True, clone_seed=True, fuse_head=False,
                head_divisor=None, ce=False):
        """fuse_head (the fused training step, whose backward forms the BCE gradient itself): the head's forward
        and backward run as one pass per token inside the last block's output kernel (rs_sas_block_out with a head); the
        returned pl / nl are filled by then.  The first block's input kernel counts the valid positions (the BCE
        divisor) for it; head_divisor (device scalar, data parallel: 1) replaces that count and must be the divisor
        later passed to backward.  ce (rows_forward): the blocks only -- no last LayerNorm, no sampled head; the
        side branch indexes the input ids alone (neg plays no part)."""
        B, T = ids.shape
        M, d, H, Dh, L = B * T, self.d, self.H, self.Dh, self.L
        p = self.p if training else 0.0
        if p > 0 and not self.external_seed:
            ops.seed_advance(self.seed_base)
        # this step's masks, replayed by backward (the fused step runs backward before the next
        # advance, so it reads the live word; the autograd API may interleave forwards: snapshot)
        sb = self.seed_base.clone() if clone_seed else self.seed_base
        e = self._buf
        s = {"B": B, "T": T, "p": p, "ids": ids, "pos": pos, "neg": neg, "sb": sb,
             "x": [], "Q": [], "mu1": [], "r1": [], "q": [], "kv": [], "o": [], "lse": [],
             "x1": [], "z": [], "mu2": [], "r2": [], "h1": []}
        fused = ops.sas_block_fused_ok(d, self.dt)
        side = fused and training and pos is not None
        nsrc = 1 if ce else 3
        if side:
            fork = self.side.mark()
        x = e("x0", (M, d))
        # the fused training step: the head's forward and backward inside the last block's output kernel, the
        # embedding stage inside the first block's input kernel, which counts the valid positions (the BCE divisor)
        fuse_head = fuse_head and side and need_logits
        cntp = None
        if fuse_head:
            cntp = self.ws.get("cntp", (ops.sas_block_in_count_parts(M),), torch.int32)
            s["cntp"] = cntp
        emb = None
        if fused:
            emb = (ids, T, self.W("item_emb.weight"), self.W("pos_emb.weight"), math.sqrt(d), p, self.salt["emb"], sb,
                   x, pos if cntp is not None else None, cntp)
        else:
            ops.embed_fwd(0, ids, T, self.W("item_emb.weight"), self.W("pos_emb.weight"), math.sqrt(d), p,
                          self.salt["emb"], sb, x)

        def after_first():
            if side:     # issued after the first forward launch (SideBranch, rule 2)
                s["side"] = self._side_prologue(ids, pos, neg, after=fork, nsrc=nsrc)
        head = None
        if cntp is not None:
            # the head inside the last block's output kernel: its outputs, per-workgroup partials
            Gb = ops.sas_block_grid(M)
            f32 = torch.float32
            s.update(head_in_block=True, hdiv=head_divisor, f=e("f", (M, d)), pl=e("pl", (B, T), f32),
                     nl=e("nl", (B, T), f32), dpl=e("dpl", (B, T), f32), dnl=e("dnl", (B, T), f32),
                     hdx=e("dx", (M, d)), lnh=self.ws.get("lnh_blk", (2 * d * Gb,), f32),
                     headp=e("headp", (3 * Gb,), f32))
            head = (self.W("item_emb.weight"), pos, neg, self.Wf("last_layernorm.weight"),
                    self.Wf("last_layernorm.bias"), cntp, head_divisor, s["f"], s["pl"], s["nl"], s["dpl"], s["dnl"],
                    s["hdx"], s["lnh"], s["headp"])
        if fused:
            x = self._forward_blocks_fused(s, x, emb=emb, after_first=after_first, head=head)
        else:
            for i in range(L):
                pre = f"attention_layers.{i}."
                Q, mu1, r1 = e("Q", (M, d)), e("mu", (M,), torch.float32), e("r", (M,), torch.float32)
                Win, bin_ = self.W(pre + "in_proj_weight"), self.Wf(pre + "in_proj_bias")
                q, kv = e("q", (M, d)), e("kv", (M, 2 * d))
                o, lse = e("o", (M, d)), e("lse", (B * H * T,), torch.float32)
                x1 = e("x1", (M, d))
                z, mu2, r2 = e("z", (M, d)), e("mu", (M,), torch.float32), e("r", (M,), torch.float32)
                fw = f"forward_layers.{i}."
                h1, xn = e("h1", (M, d)), e("x", (M, d))
                ops.layernorm_fwd(x, self.Wf(f"attention_layernorms.{i}.weight"),
                                  self.Wf(f"attention_layernorms.{i}.bias"), LN_EPS, Q, mu1, r1, 0)
                ops.linear_fwd(Q, Win[:d], q, bias=bin_[:d])
                ops.linear_fwd(x, Win[d:], kv, bias=bin_[d:])
                ops.attn_fwd(B, T, H, Dh, q, kv[:, :d], kv[:, d:], o, lse, 1.0 / math.sqrt(Dh), 0, ids, p,
                             self.salt[f"attn{i}"], sb)
                ops.linear_fwd(o, self.W(pre + "out_proj.weight"), x1, bias=self.Wf(pre + "out_proj.bias"), resid=Q)
                ops.layernorm_fwd(x1, self.Wf(f"forward_layernorms.{i}.weight"),
                                  self.Wf(f"forward_layernorms.{i}.bias"), LN_EPS, z, mu2, r2, 0)
                ops.linear_fwd(z, self.W(fw + "conv1.weight").view(d, d), h1, bias=self.Wf(fw + "conv1.bias"),
                               act=ops.ACT_RELU, drop_p=p, drop_seed=self.salt[f"ffn1_{i}"], seed_base=sb, drop_ld=d)
                ops.linear_fwd(h1, self.W(fw + "conv2.weight").view(d, d), xn, bias=self.Wf(fw + "conv2.bias"),
                               drop_p=p, drop_seed=self.salt[f"ffn2_{i}"], seed_base=sb, drop_ld=d, resid=z,
                               rowmask_ids=ids)
                for k_, v_ in (("x", x), ("Q", Q), ("mu1", mu1), ("r1", r1), ("q", q), ("kv", kv), ("o", o),
                               ("lse", lse), ("x1", x1), ("z", z), ("mu2", mu2), ("r2", r2), ("h1", h1)):
                    s[k_].append(v_)
                x = xn
        if "head_in_block" in s:
            s.update(xL=x)
            return s["pl"], s["nl"], s
        if ce:
            s.update(xL=x)
            return None, None, s
        f, muf, rf = e("f", (M, d)), e("mu", (M,), torch.float32), e("r", (M,), torch.float32)
        s.update(xL=x, f=f, muf=muf, rf=rf)
        if fused and need_logits:
            # last LayerNorm + tied sampled logits + BCE partial sums in one kernel (head.hip)
            pl, nl = e("pl", (B, T), torch.float32), e("nl", (B, T), torch.float32)
            headp = e("headp", (3 * (-(-M // 64)),), torch.float32)
            ops.sas_head_fwd(x, self.Wf("last_layernorm.weight"), self.Wf("last_layernorm.bias"), LN_EPS, f, muf, rf,
                             self.W("item_emb.weight"), pos, neg, pl, nl, headp)
            s.update(pl=pl, nl=nl, headp=headp)
            return pl, nl, s
        ops.layernorm_fwd(x, self.Wf("last_layernorm.weight"), self.Wf("last_layernorm.bias"), LN_EPS, f, muf, rf, 0)
        if not need_logits:
            return None, None, s
        pl, nl = e("pl", (B, T), torch.float32), e("nl", (B, T), torch.float32)
        ops.sampled_logits_fwd(f, self.W("item_emb.weight"), pos, neg, pl, nl)
        return pl, nl, s

    def _forward_blocks_fused(self, s, x, emb=None, after_first=None, head=None):
        """SAS blocks' forward with the row-chain kernels (rowchain.hip) on each side of the attention core
        (rs_sas_block_in, rs_attn_fwd, rs_sas_block_out per block).  Fills s's per-block saved tensors; returns the
        last block's output.  emb: sas_block_in_embed's embedding arguments (x is then its x0 output, formed by the
        first launch); after_first(): called after the first launch; head: sas_block_out_head's head arguments
        (the last block's output kernel then also runs the SAS head)."""
        B, T, p, ids, sb = s["B"], s["T"], s["p"], s["ids"], s["sb"]
        M, d, H, Dh, L = B * T, self.d, self.H, self.Dh, self.L
        e = self._buf
        f32 = torch.float32
        lay = [dict(Q=e("Q", (M, d)), mu1=e("mu", (M,), f32), r1=e("r", (M,), f32), q=e("q", (M, d)),
                    kv=e("kv", (M, 2 * d)), o=e("o", (M, d)), lse=e("lse", (B * H * T,), f32), x1=e("x1", (M, d)),
                    z=e("z", (M, d)), mu2=e("mu", (M,), f32), r2=e("r", (M,), f32), h1=e("h1", (M, d)),
                    xn=e("x", (M, d))) for _ in range(L)]

        def in_args(i):
            pre = f"attention_layers.{i}."
            Win, bin_ = self.W(pre + "in_proj_weight"), self.Wf(pre + "in_proj_bias")
            b = lay[i]
            return (self.Wf(f"attention_layernorms.{i}.weight"), self.Wf(f"attention_layernorms.{i}.bias"),
                    b["Q"], b["mu1"], b["r1"], Win[:d], bin_[:d], b["q"], Win[d:], bin_[d:], b["kv"])

        def out_args(i):
            pre, fw, b = f"attention_layers.{i}.", f"forward_layers.{i}.", lay[i]
            return (b["o"], b["Q"], self.W(pre + "out_proj.weight"), self.Wf(pre + "out_proj.bias"), b["x1"],
                    self.Wf(f"forward_layernorms.{i}.weight"), self.Wf(f"forward_layernorms.{i}.bias"), LN_EPS,
                    b["z"], b["mu2"], b["r2"], self.W(fw + "conv1.weight"), self.Wf(fw + "conv1.bias"), b["h1"],
                    self.W(fw + "conv2.weight"), self.Wf(fw + "conv2.bias"), b["xn"], ids, p,
                    self.salt[f"ffn1_{i}"], self.salt[f"ffn2_{i}"], sb)

        ln_w, ln_b, Q, mu1, r1, Wq, bq, q, Wkv, bkv, kv = in_args(0)
        # block 0's input chain and its attention forward in one launch (rs_sas_block_in_attn) where the attention
        # launch would be the LDS kernel with two or more workgroups per sequence and the count slots cover its grid
        in_attn = False
        if emb is not None and self.in_attn_fuse and H == 1:
            ns = ops.sas_block_in_attn_nsplit(d, B, T)
            in_attn = ns >= 2 and (emb[-1] is None or emb[-1].numel() >= ns * B)
        if in_attn:
            ops.sas_block_in_attn(*emb, ln_w, ln_b, LN_EPS, Q, mu1, r1, Wq, bq, q, Wkv, bkv, kv, lay[0]["o"],
                                  lay[0]["lse"], 1.0 / math.sqrt(Dh), self.salt["attn0"])
        elif emb is not None:
            ops.sas_block_in_embed(*emb, ln_w, ln_b, LN_EPS, Q, mu1, r1, Wq, bq, q, Wkv, bkv, kv)
        else:
            ops.sas_block_in(x, ln_w, ln_b, LN_EPS, Q, mu1, r1, Wq, bq, q, Wkv, bkv, kv)
        if after_first is not None:
            after_first()
        xs = [x]
        for i in range(L):
            b = lay[i]
            if i > 0 or not in_attn:
                ops.attn_fwd(B, T, H, Dh, b["q"], b["kv"][:, :d], b["kv"][:, d:], b["o"], b["lse"],
                             1.0 / math.sqrt(Dh), 0, ids, p, self.salt[f"attn{i}"], sb)
            if i + 1 < L:
                ln_w, ln_b, Q, mu1, r1, Wq, bq, q, Wkv, bkv, kv = in_args(i + 1)
                if self.boundary_fuse:
                    # this block's output chain and the next block's input chain in one launch (xn in registers)
                    ops.sas_block_out_in(out_args(i), ln_w, ln_b, LN_EPS, Q, mu1, r1, Wq, bq, q, Wkv, bkv, kv)
                else:
                    ops.sas_block_out(*out_args(i))
                    ops.sas_block_in(b["xn"], ln_w, ln_b, LN_EPS, Q, mu1, r1, Wq, bq, q, Wkv, bkv, kv)
            elif head is not None and self.turnaround_fuse:
                # the fused training step: the backward is known to follow, and its first launch (this block's
                # output-side backward) is a row chain on the rows this launch holds -- one launch for both
                if self._side_refreshed:
                    # the side branch writes the transposed weights during this forward (otherwise the previous
                    # step's optimizer wrote them)
                    self.side.join(s["side"][0])
                tb = self._out_bwd_bufs(s, i)
                ops.sas_block_out_head_bwd(out_args(i), head, *tb["args"])
                s["turnaround"] = tb
            elif head is not None:
                ops.sas_block_out_head(out_args(i), *head)
            else:
                ops.sas_block_out(*out_args(i))
            xs.append(b["xn"])
        for i in range(L):
            b = lay[i]
            for k_ in ("Q", "mu1", "r1", "q", "kv", "o", "lse", "x1", "z", "mu2", "r2", "h1"):
                s[k_].append(b[k_])
            s["x"].append(xs[i])
        return xs[L]

    @property
    def fused_head(self):
        """True when forward/backward take the fused bf16 path (head.hip, rowchain.hip, itemgrad.hip)."""
        return ops.sas_block_fused_ok(self.d, self.dt)

    # ---- backward ------------------------------------------------------------------
    def backward(self, s, dpl, dnl, grad, loss_out=None, divisor=None, split=None, aux_out=None):
        """Accumulates every parameter gradient into the flat fp32 buffer ``grad``.  dpl/dnl: the
        logits' gradients; None (fused path only) = form the BCE gradient of the forward's logits here,
        writing the loss statistics to loss_out (divisor: device count, None = this batch's).  aux_out (data
        parallel, fused head): (loss sum, count) also written there by the same launch; returns True if it was."""
        B, T, p, ids = s["B"], s["T"], s["p"], s["ids"]
        M, d, H, Dh, L = B * T, self.d, self.H, self.Dh, self.L
        sb = s["sb"]
        e = self._buf
        G = lambda n: self.flat.view(n, grad)  # noqa: E731
        slab = self.ws.get("slab", (ops.wgrad_slab_numel(M, 2 * d, d),), torch.float32)
        wln = self.ws.get("ln", (2 * 512 * d,), torch.float32)
        wat = self.ws.get("attn", (B * H * T,), torch.float32)

        fused = ops.sas_block_fused_ok(d, self.dt)
        if fused:
            # the side-stream prologue of forward built the item index and the transposed weights; the head
            # backward needs neither, so the join waits until the blocks' backward
            ev, iws = s["side"] if "side" in s else self._side_prologue(ids, s["pos"], s["neg"])
        if fused:
            dx = e("dx", (M, d))
            lnh = self.ws.get("lnh", (2 * d * (-(-M // 64)),), torch.float32)
            E, gl = self.W("item_emb.weight"), self.Wf("last_layernorm.weight")
            stats = ()
            nb = -(-M // 64)
            assert dpl is None or "turnaround" not in s, "the forward already ran the backward of its own BCE gradient"
            if dpl is None and "head_in_block" in s:
                # the head ran inside the last block's output kernel (forward)
                assert s["hdiv"] is divisor, "backward's divisor must be the one forward's head used"
                dx, dpl, dnl, lnh = s["hdx"], s["dpl"], s["dnl"], s["lnh"]
                nb = s["headp"].numel() // 3
                if loss_out is not None:
                    stats = (s["headp"], divisor, loss_out) + ((aux_out,) if aux_out is not None else ())
            elif dpl is None:
                dpl, dnl = e("dpl", (B, T), torch.float32), e("dnl", (B, T), torch.float32)
                ops.sas_head_bwd(s["headp"], divisor, loss_out, s["pl"], s["nl"], None, None, dpl, dnl, s["pos"],
                                 s["neg"], E, s["xL"], gl, s["muf"], s["rf"], dx, lnh)
            else:
                ops.sas_head_bwd(None, None, None, None, None, dpl, dnl, None, None, s["pos"], s["neg"], E, s["xL"],
                                 gl, s["muf"], s["rf"], dx, lnh)
            segs = ops.ln_partial_segments(lnh, M, d, G("last_layernorm.weight"), G("last_layernorm.bias"), nb=nb)
            # the item table's gradient (rs_item_grad, ~40 us) runs on the side stream beside the grouped weight
            # gradients (both latency-bound; measured: inside those launches on one queue 0.367 vs 0.356 ms/step at
            # cfg2, the item chunks queue behind the weight-gradient tiles); the positional table's gradient and the
            # head's loss statistics ride in the grouped reduction's launch on the main one, so both branches end
            # together and the join's cross-queue latency is hidden
            if self._side_refreshed:
                # the blocks' backward reads the transposed weights the side branch wrote this step (otherwise
                # the previous step's optimizer wrote them)
                self.side.join(ev)

            def item_grads(dx):
                ops.item_grad(iws, 3, M, dx, math.sqrt(d), p, self.salt["emb"], sb, s["f"], dpl, dnl,
                              G("item_emb.weight"), marks=getattr(self, "row_marks", None))
            dx = self._backward_blocks_fused(s, dx, grad, segs, tail=item_grads,
                                             pos=lambda dx: (ids, T, dx, p, self.salt["emb"], sb,
                                                             G("pos_emb.weight")) + stats)
            self.side.join()
            if split is not None:
                split("dense")          # every parameter gradient is final (data-parallel overlap)
            return len(stats) > 3
        df = e("df", (M, d))
        # the item table's gradient (lookup + tied logits) by the inverted index after the blocks (rs_item_grad /
        # rs_item_grad_f32): one writer per table row in a fixed order, so the unfused (fp32 parity) step is
        # deterministic -- the float-atomic scatter made every fp32 curve its own chaotic draw
        by_index = self.dt == torch.float32 or d in (64, 128, 256)   # else (bf16, other d): atomic scatter
        ops.sampled_logits_bwd(s["f"], self.W("item_emb.weight"), s["pos"], s["neg"], dpl, dnl, df,
                               None if by_index else G("item_emb.weight"))
        dx = e("dx", (M, d))
        ops.layernorm_bwd(s["xL"], df, self.Wf("last_layernorm.weight"), s["muf"], s["rf"], LN_EPS, dx,
                          G("last_layernorm.weight"), G("last_layernorm.bias"), wln, 0)
        self._backward_blocks_unfused(s, dx, grad, by_index, [ids, s["pos"], s["neg"]], s["f"], dpl, dnl)

    def _backward_blocks_unfused(self, s, dx, grad, by_index, keys, f, w1, w2):
        """The generic (fp32 parity / other widths) blocks' backward from dx = the gradient at the last block's
        output, then the embedding tables' gradients.  by_index: the item table's by the inverted index over `keys`
        (the input ids, then the tied head's pos / neg with weights w1 / w2 on f); else the atomic scatter."""
        B, T, p, ids = s["B"], s["T"], s["p"], s["ids"]
        M, d, H, Dh, L = B * T, self.d, self.H, self.Dh, self.L
        sb = s["sb"]
        e = self._buf
        G = lambda n: self.flat.view(n, grad)  # noqa: E731
        slab = self.ws.get("slab", (ops.wgrad_slab_numel(M, 2 * d, d),), torch.float32)
        wln = self.ws.get("ln", (2 * 512 * d,), torch.float32)
        wat = self.ws.get("attn", (B * H * T,), torch.float32)
        for i in reversed(range(L)):
            pre = f"attention_layers.{i}."
            fw = f"forward_layers.{i}."
            # x_{i+1} = (drop2(h1 W2^T + b2) + z) * mask
            dy2, dzres = e("dy2", (M, d)), e("dzres", (M, d))
            ops.dropout_rowmask(dx, p, self.salt[f"ffn2_{i}"], sb, ids, dy2, dzres)
            ops.linear_wgrad(dy2, s["h1"][i], G(fw + "conv2.weight").view(d, d), slab, db=G(fw + "conv2.bias"))
            da1 = e("da1", (M, d))
            ops.linear_dgrad(dy2, self.W(fw + "conv2.weight").view(d, d), da1, act=ops.ACT_RELU_BWD,
                             aux=s["h1"][i], drop_p=p, drop_seed=self.salt[f"ffn1_{i}"], seed_base=sb, drop_ld=d)
            ops.linear_wgrad(da1, s["z"][i], G(fw + "conv1.weight").view(d, d), slab, db=G(fw + "conv1.bias"))
            dz = e("dz", (M, d))
            ops.linear_dgrad(da1, self.W(fw + "conv1.weight").view(d, d), dz, resid=dzres)
            dx1 = e("dx1", (M, d))
            ops.layernorm_bwd(s["x1"][i], dz, self.Wf(f"forward_layernorms.{i}.weight"), s["mu2"][i], s["r2"][i],
                              LN_EPS, dx1, G(f"forward_layernorms.{i}.weight"), G(f"forward_layernorms.{i}.bias"),
                              wln, 0)
            # x1 = Q + o Wo^T + bo
            ops.linear_wgrad(dx1, s["o"][i], G(pre + "out_proj.weight"), slab, db=G(pre + "out_proj.bias"))
            do = e("do", (M, d))
            ops.linear_dgrad(dx1, self.W(pre + "out_proj.weight"), do)
            dq, dkv = e("dq", (M, d)), e("dkv", (M, 2 * d))
            kv = s["kv"][i]
            ops.attn_bwd(B, T, H, Dh, s["q"][i], kv[:, :d], kv[:, d:], s["o"][i], do, s["lse"][i], dq,
                         dkv[:, :d], dkv[:, d:], 1.0 / math.sqrt(Dh), 0, ids, p, self.salt[f"attn{i}"], sb, wat)
            Gin, Gb = G(pre + "in_proj_weight"), G(pre + "in_proj_bias")
            Win = self.W(pre + "in_proj_weight")
            ops.linear_wgrad(dq, s["Q"][i], Gin[:d], slab, db=Gb[:d])
            ops.linear_wgrad(dkv, s["x"][i], Gin[d:], slab, db=Gb[d:])
            dQ = e("dQ", (M, d))
            ops.linear_dgrad(dq, Win[:d], dQ, resid=dx1)
            dxi = e("dxi", (M, d))
            ops.linear_dgrad(dkv, Win[d:], dxi)
            ops.layernorm_bwd(s["x"][i], dQ, self.Wf(f"attention_layernorms.{i}.weight"), s["mu1"][i], s["r1"][i],
                              LN_EPS, dxi, G(f"attention_layernorms.{i}.weight"),
                              G(f"attention_layernorms.{i}.bias"), wln, 0, accumulate=True)
            dx = dxi
        ops.embed_bwd(0, ids, T, dx, math.sqrt(d), p, self.salt["emb"], sb, None if by_index else G("item_emb.weight"),
                      G("pos_emb.weight"))
        if by_index:
            V1 = self.flat.shapes["item_emb.weight"][0]
            n = len(keys)
            iws = self.ws.get("itemidx", (ops.item_index_ws_bytes(n, M, V1, d),), torch.uint8)
            ops.item_index_build(keys, V1, d, iws)
            ops.item_grad(iws, n, M, dx, math.sqrt(d), p, self.salt["emb"], sb, f, w1, w2,
                          G("item_emb.weight"), marks=getattr(self, "row_marks", None) if n == 3 else None)

    # ---- the row heads (heads.py): ce, sampled_ce, gbce -----------------------------------
    @property
    def ce_rows_fused(self):
        """True when the CE head's row-local work runs in the two sas_ce.hip launches (bf16, d in {64, 128});
        RS_SAS_CE_ROWS=0 selects the composed launches they replace (A/B timing, tools/sas_ce_bench.py)."""
        return ops.sas_ce_rows_ok(self.d, self.dt) and os.environ.get("RS_SAS_CE_ROWS", "1") != "0"

    def _valid_rows_forward(self, s, pos, max_labelled):
        """The last LayerNorm on the rows with pos != 0, compacted (the front half of every row head): hl [cap][d],
        lab [cap], the device row count and the mean's divisor max(count, 1), in the engine's ce_* buffers."""
        d, dt = self.d, self.dt
        M = s["B"] * s["T"]
        f32 = torch.float32
        g = self.ws.get
        # fp32 rows that are no multiple of 16 bytes (the reference's d = 50): the compaction kernels do not take
        # them, so the head runs on all M rows (labels 0 are ignored by rs_ce_fwd / rs_ce_bwd: same loss, same
        # gradients)
        dense = dt == torch.float32 and d % 4 != 0
        cap = M if dense else int(max_labelled or M)
        V1 = self.flat.shapes["item_emb.weight"][0]
        V1p = -(-V1 // 64) * 64
        x, labels = s["xL"], pos.reshape(-1)
        idx, rank, cnt = g("ce_idx", (cap,), torch.int32), g("ce_rank", (M,), torch.int32), g("ce_cnt", (1,), torch.int32)
        if "ce_hl" not in self.ws.bufs or tuple(self.ws.bufs["ce_hl"].shape) != (cap, d):
            g("ce_hl", (cap, d), dt).zero_()      # rows past the live count are never written: start them finite
        hl, lab, div = g("ce_hl", (cap, d), dt), g("ce_lab", (cap,), torch.int64), g("ce_div", (1,), f32)
        gl, bl = self.Wf("last_layernorm.weight"), self.Wf("last_layernorm.bias")
        rows_fused = self.ce_rows_fused
        if dense:
            hl, mu, rs, lab, cnt = g("ce_f", (M, d), dt), g("ce_mu", (M,), f32), g("ce_rs", (M,), f32), labels, None
            ops.layernorm_fwd(x, gl, bl, LN_EPS, hl, mu, rs, 0)
            div.copy_(torch.count_nonzero(labels)).clamp_(min=1)
        elif rows_fused:
            mu, rs = g("ce_mu", (cap,), f32), g("ce_rs", (cap,), f32)
            ops.sas_ce_rows_fwd(x, labels, cap, gl, bl, LN_EPS, idx, rank, cnt, hl, lab, mu, rs, divisor=div)
        else:
            f, mu, rs = g("ce_f", (M, d), dt), g("ce_mu", (M,), f32), g("ce_rs", (M,), f32)
            ops.layernorm_fwd(x, gl, bl, LN_EPS, f, mu, rs, 0)
            ops.compact_rows(labels, cap, idx, rank, cnt)
            ops.gather_rows(f, idx, cnt, cap, hl, labels, lab)
            div.copy_(cnt).clamp_(min=1)          # the mean's divisor: max(count, 1)
        return dict(cap=cap, V1=V1, V1p=V1p, rank=rank, cnt=cnt, hl=hl, lab=lab, div=div, mu=mu, rs=rs,
                    rows_fused=rows_fused, dense=dense)

    def rows_forward(self, head, ids, pos, extra, training, loss_out, max_labelled=None, clone_seed=True):
        """Blocks' forward, then on the rows with pos != 0 only: the last LayerNorm and the row head's loss (heads.py;
        extra: the head's own batch tensors).  loss_out (fp32 [>= 3], device) = {loss sum, valid count, mean}; a batch
        without a valid row gives mean 0.  max_labelled: upper bound on the valid rows (sizes the compact buffers;
        default B*T; rows past it are dropped as rs_compact_rows does).  Returns the saved state for rows_backward.
        Buffers are the engine's workspace; nothing here allocates per step or reads the host."""
        extra = head.prepare(self, ids, pos, *extra)
        _, _, s = self.forward(ids, pos, None, training, need_logits=False, clone_seed=clone_seed, ce=True)
        c = self._valid_rows_forward(s, pos, max_labelled)
        c.update(head=head)
        head.forward(self, c, extra, loss_out)
        s.update(ce=c)
        return s

    def rows_backward(self, s, grad, dloss=None):
        """Accumulates every parameter gradient of rows_forward's loss (times *dloss, a device scalar, if given) into
        the flat fp32 buffer ``grad``: the head's backward, then the shared back half."""
        slab_d, sk, table_grad = s["ce"]["head"].backward(self, s, grad, dloss)
        self._valid_rows_backward(s, grad, slab_d, sk, table_grad)

    def _valid_rows_backward(self, s, grad, slab_d, sk, table_grad=None):
        """From dh on the compact rows (fp32 slab_d [sk][cap][d], summed in split order): the last LayerNorm's
        backward scattered to all rows, the blocks' backward and the lookup part of the item table's gradient by the
        inverted index over the input ids (the back half of every row head).  table_grad(): the head's own rows of that
        gradient, launches that depend on the head alone.  On the fused path they run on the side branch beside the
        LayerNorm and blocks' backward, forked before the LayerNorm backward and issued after it; the lookup part
        continues that branch after the blocks' backward and the step joins it once (SideBranch, rules 2 and 3): one
        writer at a time, fixed order, no float atomics.  Elsewhere they follow the LayerNorm backward on the main
        stream."""
        c = s["ce"]
        B, T, p, ids = s["B"], s["T"], s["p"], s["ids"]
        M, d = B * T, self.d
        sb, dt = s["sb"], self.dt
        f32 = torch.float32
        g = self.ws.get
        G = lambda n: self.flat.view(n, grad)  # noqa: E731
        cap = c["cap"]
        GE = G("item_emb.weight")
        gl = self.Wf("last_layernorm.weight")
        fused = ops.sas_block_fused_ok(d, dt)
        fork = self.side.mark() if table_grad is not None and fused and "side" in s else None
        dx = g("ce_dx", (M, d), dt)
        if c["rows_fused"]:
            nb = ops.sas_ce_rows_nparts(M)
            part = g("ce_lnp", (2 * d * nb,), f32)
            ops.sas_ce_rows_bwd(slab_d, sk, cap, c["rank"], s["xL"], gl, c["mu"], c["rs"], dx, part)
            segs = ops.ln_partial_segments(part, M, d, G("last_layernorm.weight"), G("last_layernorm.bias"), nb=nb)
            if not fused:
                ops.reduce_segments(segs)
        else:
            df = g("ce_df", (M, d), dt)
            if c["dense"]:
                ops.reduce_slabs(slab_d, sk, df)
            else:
                ops.splitk_scatter_rows(slab_d, sk, cap, c["rank"], df)
            wln = g("ln", (2 * 512 * d,), f32)
            ops.layernorm_bwd(s["xL"], df, gl, c["mu"], c["rs"], LN_EPS, dx, G("last_layernorm.weight"),
                              G("last_layernorm.bias"), wln, 0)
            segs = []
        if fork is not None:
            with self.side.run(after=fork, end=False):
                table_grad()
        elif table_grad is not None:
            table_grad()
        if not fused:
            by_index = dt == torch.float32 or d in (64, 128, 256)
            self._backward_blocks_unfused(s, dx, grad, by_index, [ids], None, None, None)
            return
        ev, iws = s["side"] if "side" in s else self._side_prologue(ids, None, None, nsrc=1)
        if self._side_refreshed:
            self.side.join(ev)

        def item_grads(dx):
            ops.item_grad(iws, 1, M, dx, math.sqrt(d), p, self.salt["emb"], sb, None, None, None, GE)
        self._backward_blocks_fused(s, dx, grad, segs, tail=item_grads,
                                    pos=lambda dx: (ids, T, dx, p, self.salt["emb"], sb, G("pos_emb.weight")))
        self.side.join()

    def enable_row_marks(self, min_rows=0):
        """Stamp the rows the inverted-index gradient writes (rs_item_grad_marked) so the optimizer can skip the
        gradient loads of the others: (table name, row marks u8 [rows], epoch u8 [1]), or None where that
        gradient is not the index path's alone (fp32 / other widths) or the table is below min_rows."""
        name = "item_emb.weight"
        rows, d = self.flat.shapes[name]
        if not (self.dt == torch.bfloat16 and d in (64, 128, 256)) or d & (d - 1) or rows < min_rows:
            self.row_marks = None
            return None
        self.row_marks = (torch.zeros(ops.row_marks_bytes(rows), dtype=torch.uint8, device=self.dev),
                          torch.zeros(1, dtype=torch.uint8, device=self.dev))
        return (name,) + self.row_marks

    def _side_prologue(self, ids, pos, neg, after=None, nsrc=3):
        """Work of the fused backward that depends only on the batch's keys and the weights, issued on a
        side branch so it overlaps the forward pass: the item-gradient index (rs_item_index_build) and
        the transposed block weights (rs_transpose_bf16).  Returns (the branch's end event, index workspace)."""
        B, T = ids.shape
        M, d = B * T, self.d
        V1 = self.flat.shapes["item_emb.weight"][0]
        with self.side.run(after=after):
            iws = self.ws.get("itemidx", (ops.item_index_ws_bytes(nsrc, M, V1, d),), torch.uint8)
            ops.item_index_build([ids, pos, neg][:nsrc], V1, d, iws)
            self._side_refreshed = not self.adam_transposes or self._wT is None
            if self._side_refreshed:
                self._refresh_transposed()
        return self.side.end, iws

    def _refresh_transposed(self):
        """bf16 [in][out] copies of the block weights for the fused backward's input-gradient
        GEMMs (rs_transpose_bf16, one launch); per layer: in_proj^T [d][3d], out_proj^T, conv1^T,
        conv2^T [d][d]."""
        d, L = self.d, self.L
        if self._wT is None:
            self._wT = torch.empty(L * 6 * d * d, dtype=torch.bfloat16, device=self.dev)
            desc = []
            for i in range(L):
                base = i * 6 * d * d
                pre, fw = f"attention_layers.{i}.", f"forward_layers.{i}."
                for name, rows, off in ((pre + "in_proj_weight", 3 * d, 0), (pre + "out_proj.weight", d, 3 * d * d),
                                        (fw + "conv1.weight", d, 4 * d * d), (fw + "conv2.weight", d, 5 * d * d)):
                    desc.append([rows, d, self.flat.offsets[name], d, base + off, rows])
            self._wT_desc = torch.tensor(desc, dtype=torch.int64, device=self.dev)
            self._wT_desc_host = desc
            self._wT_tiles = max(-(-r // 64) * -(-c // 64) for r, c, *_ in desc)
        ops.transpose_bf16(self._wT_desc, self._wT_tiles, self.flat.bf16, self._wT)
        return self._wT

    def _out_bwd_bufs(self, s, i):
        """Block i's output-side backward issued from the forward (the turnaround launch): its gradient buffers,
        and the arguments of ops.sas_block_out_head_bwd after the head's (the workspaces are those
        _backward_blocks_fused uses)."""
        B, T = s["B"], s["T"]
        M, d, H, L = B * T, self.d, self.H, self.L
        e = self._buf
        wT = self._wT.view(L, 6, d, d)
        lnp = self.ws.get("lnp", (L, 2, 2 * d * ops.sas_block_parts(M)), torch.float32)
        g = dict(dy2=e("dy2", (M, d)), da1=e("da1", (M, d)), dx1=e("dx1", (M, d)), do=e("do", (M, d)))
        dl = self.ws.get(f"attn_delta{i}", (B * H * T,), torch.float32) if H == 1 else None
        return dict(g=g, args=(wT[i, 5], wT[i, 4], wT[i, 3], g["dy2"], g["da1"], g["dx1"], g["do"], lnp[i, 0], dl))

    def _backward_blocks_fused(self, s, dx, grad, extra_segs=(), tail=None, pos=None):
        """SAS blocks' backward with rs_sas_block_out_bwd / rs_sas_block_in_bwd (rowchain.hip) for the
        row-local chains; then ALL ten weight gradients and the four LayerNorm affine partial sets in
        one grouped GEMM launch + one grouped reduction (rs_wgrad_grouped, wgrad.hip).  Returns the
        gradient at the embedding output.  tail(dx): work on that gradient alone (the item table's
        gradient), issued on the side branch so it runs beside the grouped weight-gradient launch (both are
        latency-bound); the caller joins the branch (self.side.join()).  pos(dx): the positional table's gradient (and
        the head's loss statistics) in the grouped reduction's launch (ops.wgrad_grouped pos=)."""
        B, T, p, ids, sb = s["B"], s["T"], s["p"], s["ids"], s["sb"]
        M, d, H, Dh, L = B * T, self.d, self.H, self.Dh, self.L
        e = self._buf
        G = lambda n: self.flat.view(n, grad)  # noqa: E731
        wT = self._wT.view(L, 6, d, d)              # refreshed by _side_prologue
        nb = ops.sas_block_parts(M)
        lnp = self.ws.get("lnp", (L, 2, 2 * d * nb), torch.float32)
        wat = self.ws.get("attn", (B * H * T,), torch.float32)
        probs, segs = [], list(extra_segs)
        # per block: the out-side backward's outputs (dy2, da1, dx1, do) and the attention backward's (dq, dkv)
        g = [dict(dy2=e("dy2", (M, d)), da1=e("da1", (M, d)), dx1=e("dx1", (M, d)), do=e("do", (M, d)),
                  dq=e("dq", (M, d)), dkv=e("dkv", (M, 2 * d))) for _ in range(L)]
        turn = s.get("turnaround")       # the forward's last launch already ran block L-1's output-side backward
        if turn is not None:
            g[L - 1].update(turn["g"])

        # one head: the out-side backward also forms the attention backward's row term delta = rowsum(dO * O)
        # (the attention kernels then read neither O nor recompute it)
        dl = [self.ws.get(f"attn_delta{i}", (B * H * T,), torch.float32) for i in range(L)] if H == 1 else None

        def out_bwd_args(i):
            return (ids, s["h1"][i], s["x1"][i], s["mu2"][i], s["r2"][i], self.Wf(f"forward_layernorms.{i}.weight"),
                    wT[i, 5], wT[i, 4], wT[i, 3], g[i]["dy2"], g[i]["da1"], g[i]["dx1"], g[i]["do"], lnp[i, 0], p,
                    self.salt[f"ffn1_{i}"], self.salt[f"ffn2_{i}"], sb, s["o"][i] if dl else None, dl[i] if dl else None)

        def in_bwd_args(i):
            return (g[i]["dq"], g[i]["dkv"], g[i]["dx1"], s["x"][i], s["mu1"][i], s["r1"][i],
                    self.Wf(f"attention_layernorms.{i}.weight"), wT[i, 0:3].reshape(d, 3 * d))

        if turn is None:
            ops.sas_block_out_bwd(dx, *out_bwd_args(L - 1))
        for i in reversed(range(L)):
            pre, fw = f"attention_layers.{i}.", f"forward_layers.{i}."
            dq, dkv, kv = g[i]["dq"], g[i]["dkv"], s["kv"][i]
            ops.attn_bwd(B, T, H, Dh, s["q"][i], kv[:, :d], kv[:, d:], s["o"][i], g[i]["do"], s["lse"][i], dq,
                         dkv[:, :d], dkv[:, d:], 1.0 / math.sqrt(Dh), 0, ids, p, self.salt[f"attn{i}"], sb,
                         dl[i] if dl else wat, delta_in=bool(dl))
            if i > 0 and self.boundary_fuse:
                # this block's input-side backward and the previous block's output-side backward in one launch: the
                # gradient between them stays in registers (a scratch only where the entry runs two launches)
                dxi = None if ops.sas_block_boundary_fused(M, d) else e("dxi", (M, d))
                ops.sas_block_in_out_bwd(in_bwd_args(i), dxi, lnp[i, 1], out_bwd_args(i - 1))
            else:
                dxi = e("dxi", (M, d))
                ops.sas_block_in_bwd(*in_bwd_args(i), dxi, lnp[i, 1])
                if i > 0:
                    ops.sas_block_out_bwd(dxi, *out_bwd_args(i - 1))
            dx = dxi
            Gin, Gb = G(pre + "in_proj_weight"), G(pre + "in_proj_bias")
            probs += [(g[i]["dy2"], s["h1"][i], G(fw + "conv2.weight"), G(fw + "conv2.bias")),
                      (g[i]["da1"], s["z"][i], G(fw + "conv1.weight"), G(fw + "conv1.bias")),
                      (g[i]["dx1"], s["o"][i], G(pre + "out_proj.weight"), G(pre + "out_proj.bias")),
                      (dq, s["Q"][i], Gin[:d], Gb[:d]),
                      (dkv, s["x"][i], Gin[d:], Gb[d:])]
            segs += ops.ln_partial_segments(lnp[i, 0], M, d, G(f"forward_layernorms.{i}.weight"),
                                            G(f"forward_layernorms.{i}.bias"))
            segs += ops.ln_partial_segments(lnp[i, 1], M, d, G(f"attention_layernorms.{i}.weight"),
                                            G(f"attention_layernorms.{i}.bias"))
        rows = self._wgrad_rows(M, 6 * L)
        wslab = self.ws.get("wslab", (ops.wgrad_grouped_slab_numel([(d, d)] * 4 * L + [(2 * d, d)] * L, M, rows),),
                            torch.float32)
        fork = self.side.mark() if tail is not None else None
        # the grouped launch is issued BEFORE the side branch (SideBranch, rule 2)
        ops.wgrad_grouped(probs, M, rows, wslab, extra=segs, pos=pos(dx) if pos is not None else None)
        if tail is not None:
            with self.side.run(after=fork):
                tail(dx)
        return dx

    @staticmethod
    def _wgrad_rows(M, tiles):
        """rows per split of the grouped weight-gradient launch: ~256 workgroups (the 128x128-tile kernel
        runs one per CU), fewer splits also shrink the partial slab the reduction reads."""
        splits = max(1, 256 // tiles)
        return max(64, -(-(-(-M // splits)) // 64) * 64)

    # ---- eval ----------------------------------------------------------------------
    def features(self, ids):
        self.sync_compute_weights()
        _, _, s = self.forward(ids, None, None, False, need_logits=False)
        B, T = ids.shape
        return s["f"].view(B, T, self.d)

    def predict(self, ids, cand):
        f = self.features(ids)[:, -1, :]                    # sas.py:110 (a strided view: row stride T*d)
        # candidate scores <f_b, item_emb[c]> (sas.py:112-114): one wave per (row, candidate), rs_candidate_scores
        return ops.candidate_scores(f, self.W("item_emb.weight"), cand)

    # full catalogue: the same hidden state against every item of [1, num_items + 1), no score matrix
    def full_rank(self, ids, target, exclude_seen=True):
        f = self.features(ids)[:, -1, :]
        return ops.full_rank(f, self.W("item_emb.weight"), target, lo=1, hi=self.m.item_num + 1,
                             exclude=ids if exclude_seen else None)

    def topk(self, ids, k, exclude_seen=True):
        f = self.features(ids)[:, -1, :]
        return ops.full_topk(f, self.W("item_emb.weight"), k, lo=1, hi=self.m.item_num + 1,
                             exclude=ids if exclude_seen else None)
