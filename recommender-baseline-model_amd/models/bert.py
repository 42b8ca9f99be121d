"""BERTModel -- same API as the reference ``BS/models/bert.py:6-16``.

``forward(x)`` returns the full-vocabulary logits (B, T, V+1) like the
reference; training through :class:`rbm_amd.train_step.FusedTrainStep` uses the
labelled-rows-only loss head instead (same loss and gradients).  ``predict(x,
candidates)`` gives the validation scores ``forward(x)[:, -1, :].gather(1,
candidates)`` (``BS/trainers/bert.py:43-49``) without forming the (B, T, V+1)
logits (51 GB fp32 at a 1M-item catalogue and B = 64).
"""
import torch
import torch.nn as nn

from ..engine_util import as_ids, compute_dtype, require_cuda
from .base import BaseModel
from .bert_model.bert import BERT, BERTEngine, _BERTFunction, _BERTSCEFunction, build_flat


class BERTModel(BaseModel):
    def __init__(self, args):
        super().__init__(args)
        self.bert = BERT(args)
        self.out = nn.Linear(self.bert.hidden, args.num_items + 1)
        self.cdtype = compute_dtype(args)
        self._flat = None
        self._engine = None
        if torch.device(getattr(args, "device", "cpu")).type == "cuda":
            self.to(args.device)

    @classmethod
    def code(cls):
        return 'bert'

    def _apply(self, fn, recurse=True):
        # (re)build the flat parameter buffer eagerly on .to(cuda), before any optimizer is created over
        # model.parameters() (the reference builds its Adam after model.to(device), base.py:21,38)
        super()._apply(fn, recurse)
        p = self.out.weight
        self._flat = build_flat(self, p.device) if p.device.type == "cuda" else None
        self._engine = None
        return self

    def engine(self):
        p = self.out.weight
        require_cuda(p.device)
        if self._flat is None or not self._flat.is_bound(self):
            self._flat = build_flat(self, p.device)
            self._engine = None
        if self._engine is None:
            self._engine = BERTEngine(self, self._flat)
        return self._engine

    @torch.no_grad()
    def predict(self, x, candidates):
        """(B, C) fp32 scores of the last position at ``candidates`` (long ids): the same values as
        ``self(x)[:, -1, :].gather(1, candidates)`` (the reference's calculate_metrics), eval-mode encoder."""
        eng = self.engine()
        dev = self._flat.device
        return eng.predict(as_ids(x, dev), as_ids(candidates, dev))

    @torch.no_grad()
    def recommend(self, x, k, exclude_seen=True):
        """(ids int64 (B, k), scores fp32 (B, k)) on the device: the k best items of the whole catalogue at the last
        position (x ends in [MASK], as for ``predict``), best first (equal scores: lower id first), without x's own
        items when exclude_seen; the padding id and [MASK] are never returned."""
        return self.engine().topk(as_ids(x, self._flat.device), k, exclude_seen)

    @torch.no_grad()
    def full_rank(self, x, target, exclude_seen=True):
        """int32 (B,) rank of target[b] among all items (0 = first), x's own items left out when exclude_seen."""
        dev = self._flat.device
        return self.engine().full_rank(as_ids(x, dev), as_ids(target, dev).reshape(-1), exclude_seen)

    def sampled_ce_loss(self, tokens, labels, cand, logq=None):
        """Scalar loss of the sampled softmax over batch-shared candidates (differentiable; available whatever
        bert_loss says).  cand: int64 (K,), shared by every position; with E = out.weight, b = out.bias:

            h_r   = BERT(tokens)[r]                            for every position r with labels_r != 0 ("labelled")
            z_r0  = <h_r, E[labels_r]> + b[labels_r]
            z_rj  = <h_r, E[cand_j]> + b[cand_j],  j = 1..K
            live(r, j) = cand_j != 0 and cand_j != labels_r    id 0 = an ignored slot; accidental hits masked
            loss  = (1 / max(n, 1)) * sum_r [ log(exp(z_r0) + sum_{live j} exp(z_rj)) - z_r0 ],   n = #labelled

        Duplicate candidates count separately; an id outside out.weight's rows counts as 0.  logq (fp32, one entry
        per row of out.weight, on the device: ItemProposal.logq) is the logQ correction, the log of the distribution
        the candidates were drawn from: z_r0 -= logq[labels_r], z_rj -= logq[cand_j]; a constant of the loss (no
        gradient, and out.bias's gradient is unchanged in form), entry 0 never read; None: no correction.  With
        cand = every item it is the
        reference's cross-entropy up to class 0, which that loss counts and no candidate list can name.  A row with
        no live candidate, and a batch with no labelled row, give loss 0 and zero gradients; rows of out.weight /
        out.bias outside the batch's labels and candidates get none.  Call backward() before the next loss call."""
        eng = self.engine()
        dev = self._flat.device
        ids, lab, cand = as_ids(tokens, dev), as_ids(labels, dev), as_ids(cand, dev)
        params = [p for _, p in self.named_parameters()]
        return _BERTSCEFunction.apply(eng, ids, lab, cand, logq, self.training, *params)

    def forward(self, x):
        eng = self.engine()
        ids = as_ids(x, self._flat.device)
        params = [p for _, p in self.named_parameters()]
        return _BERTFunction.apply(eng, ids, self.training, *params)
