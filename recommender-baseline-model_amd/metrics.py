"""Ranking metrics on the GPU: ``recalls_ndcgs_and_mrr_for_ks`` (BS/trainers/utils.py:28-57) through
rs_rank_metrics.  Same inputs (scores, labels: (B, C)) and the same dict keys; ranks follow a stable
descending sort (ties by candidate index)."""
import torch

from . import ops
from .engine_util import as_ids


def recalls_ndcgs_and_mrr_for_ks(scores, labels, ks):
    dev = scores.device
    if dev.type != "cuda":
        raise RuntimeError("rbm_amd.metrics runs on the GPU (rs_rank_metrics); there is no CPU fallback")
    ks = sorted(ks, reverse=True)
    s = scores.detach().float().contiguous()
    lab = labels.detach().to(device=dev, dtype=torch.float32).contiguous()
    R = s.shape[0]
    ks_dev = torch.tensor(ks, dtype=torch.int32, device=dev)
    ws = torch.empty(3 * len(ks) * R, dtype=torch.float32, device=dev)
    out = torch.empty(3 * len(ks), dtype=torch.float32, device=dev)
    ops.rank_metrics(s, lab, ks_dev, ws, out)
    v = out.cpu().tolist()
    res = {}
    for q, k in enumerate(ks):
        res["Recall@%d" % k] = v[3 * q]
        res["NDCG@%d" % k] = v[3 * q + 1]
        res["MRR@%d" % k] = v[3 * q + 2]
    return res


def calculate_metrics(model, batch, metric_ks):
    """The trainers' ``calculate_metrics`` (BS/trainers/sas.py:56-62, BS/trainers/bert.py:43-52) on the GPU: the
    model's scores at the candidates -- ``SASModel.predict`` / ``BERTModel.predict`` (the last position only, no
    (B, T, V+1) logits) -- ranked by rs_rank_metrics.  batch = (seqs, candidates, labels) as the eval loaders
    yield it."""
    seqs, candidates, labels = batch
    dev = model.engine().flat.device if hasattr(model, "engine") else next(model.parameters()).device
    with torch.no_grad():
        scores = model.predict(as_ids(seqs, dev), as_ids(candidates, dev))
    return recalls_ndcgs_and_mrr_for_ks(scores, torch.as_tensor(labels).to(dev), metric_ks)


def evaluate(model, loader, metric_ks):
    """The body of the reference's ``validate`` (BS/trainers/base.py:151-183): ``calculate_metrics`` on every batch of
    the loader (a DeviceEvalLoader, or anything that yields (seqs, candidates, labels)), averaged as AverageMeterSet
    does -- every batch's mean has weight one, the partial last batch included.  The per-batch results stay on the
    device: rs_rank_metrics writes batch i into row i of an (n_batches, 3 nk) fp32 buffer, the mean over the rows is
    taken in float64, and the host reads once at the end.  Same dict keys as ``recalls_ndcgs_and_mrr_for_ks``."""
    dev = model.engine().flat.device if hasattr(model, "engine") else next(model.parameters()).device
    if torch.device(dev).type != "cuda":
        raise RuntimeError("rbm_amd.metrics runs on the GPU (rs_rank_metrics); there is no CPU fallback")
    ks = sorted(metric_ks, reverse=True)
    n = len(loader)
    if n < 1:
        raise ValueError("the loader yields no batch")
    ks_dev = torch.tensor(ks, dtype=torch.int32, device=dev)
    rows = torch.zeros((n, 3 * len(ks)), dtype=torch.float32, device=dev)
    ws, i = None, 0
    with torch.no_grad():
        for seqs, candidates, labels in loader:
            if i >= n:
                raise ValueError("the loader yields more batches than len(loader)")
            scores = model.predict(as_ids(seqs, dev), as_ids(candidates, dev)).float().contiguous()
            lab = torch.as_tensor(labels).to(device=dev, dtype=torch.float32).contiguous()
            if ws is None or ws.numel() < 3 * len(ks) * scores.shape[0]:
                ws = torch.empty(3 * len(ks) * scores.shape[0], dtype=torch.float32, device=dev)
            ops.rank_metrics(scores, lab, ks_dev, ws, rows[i])
            i += 1
    if i != n:
        raise ValueError(f"the loader yielded {i} batches, len(loader) = {n}")
    v = rows.double().mean(dim=0).cpu().tolist()
    res = {}
    for q, k in enumerate(ks):
        res["Recall@%d" % k] = v[3 * q]
        res["NDCG@%d" % k] = v[3 * q + 1]
        res["MRR@%d" % k] = v[3 * q + 2]
    return res


def full_rank_metrics(model, batch, metric_ks, exclude_seen=True):
    """Exact full-rank Recall / NDCG / MRR @ k: the held-out item ranked against EVERY item of the catalogue (minus the
    row's own history when exclude_seen; the held-out item always stays), not against 100 sampled negatives.
    batch = (seqs, targets) -- seqs as ``predict`` takes them (BERT: ending in [MASK]), targets (B,) item ids.  The
    same dict keys as ``recalls_ndcgs_and_mrr_for_ks``; rs_full_rank + rs_rank_to_metrics, no (B, V) scores."""
    seqs, targets = batch
    dev = model.engine().flat.device if hasattr(model, "engine") else next(model.parameters()).device
    if torch.device(dev).type != "cuda":
        raise RuntimeError("rbm_amd.metrics runs on the GPU (rs_full_rank); there is no CPU fallback")
    ks = sorted(metric_ks, reverse=True)
    with torch.no_grad():
        rank = model.full_rank(as_ids(seqs, dev), as_ids(targets, dev).reshape(-1), exclude_seen)
    ks_dev = torch.tensor(ks, dtype=torch.int32, device=dev)
    ws = torch.empty(3 * len(ks) * rank.numel(), dtype=torch.float32, device=dev)
    out = torch.empty(3 * len(ks), dtype=torch.float32, device=dev)
    ops.rank_to_metrics(rank, ks_dev, ws, out)
    v = out.cpu().tolist()
    res = {}
    for q, k in enumerate(ks):
        res["Recall@%d" % k] = v[3 * q]
        res["NDCG@%d" % k] = v[3 * q + 1]
        res["MRR@%d" % k] = v[3 * q + 2]
    return res
