"""Union-of-touched-rows exchange of the BERT token table's gradient (dp.SparseRowExchange, sparse_rows.hip;
SURVEY.md §8(e)).  The kernels against a torch restatement, then two data-parallel ranks -- processes on ONE GPU,
gloo moving the tensors (the product uses RCCL) -- whose parameters after three steps equal, bit for bit, the same
ranks exchanging the dense table (two ranks: every element is a + b either way)."""
import argparse
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_touched_rows_pack_unpack():
    import rbm_amd  # noqa: F401
    from rbm_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    for rows, d, n in ((1000, 8, 300), (5003, 64, 4096), (100_000, 16, 50_000), (7, 4, 0)):
        ids = torch.randint(0, rows, (n,), device="cuda", generator=g)
        flags = torch.full((rows,), 7, dtype=torch.int32, device="cuda")
        index = torch.empty(rows, dtype=torch.int32, device="cuda")
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
        ws = torch.empty(ops.touched_rows_ws_numel(rows), dtype=torch.int32, device="cuda")
        ops.touched_rows(ids, rows, flags, index, count, ws)
        uniq = torch.unique(ids)
        ref = torch.full((rows,), -1, dtype=torch.int32, device="cuda")
        ref[uniq] = torch.arange(uniq.numel(), dtype=torch.int32, device="cuda")
        assert int(count.item()) == uniq.numel()
        assert torch.equal(index, ref)
        src = torch.randn(rows, d, device="cuda", generator=g)
        cap = max(1, min(rows, n + 5))
        compact = torch.full((cap, d), 3.0, device="cuda")
        ops.rows_pack(src, index, count, compact)
        assert torch.equal(compact[:uniq.numel()], src[uniq])
        assert not compact[uniq.numel():].any()
        dst = torch.zeros(rows, d, device="cuda")
        ops.rows_unpack(dst, index, compact * 2)
        assert torch.equal(dst[uniq], 2 * src[uniq])
        mask = torch.ones(rows, dtype=torch.bool, device="cuda")
        mask[uniq] = False
        assert not dst[mask].any()


V, T, D, BR = 20000, 50, 64, 4      # items, max_len, hidden, sequences per rank (2*200 ids << 20,002 rows)


def _rendezvous(d):
    """init_method of a file store inside the test's own directory: the ranks meet through it, so there is no port
    that another process could take between choosing it and binding it."""
    fd, path = tempfile.mkstemp(prefix="rdzv", dir=str(d))
    os.close(fd)
    return "file://" + path


def _model():
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    a = argparse.Namespace(model_code="bert", num_items=V, max_len=T, device="cuda", bert_hidden_units=D,
                           bert_num_blocks=1, bert_num_heads=2, bert_dropout=0.1, bert_hidden_dropout=0.1,
                           bert_mask_prob=0.2, model_init_seed=7, rs_dtype="bf16")
    return model_factory(a)


def _worker(rank, world, rdzv, graph, mode, out_dir):
    import sys
    sys.path.insert(0, ROOT)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=rdzv, rank=rank, world_size=world)
    try:
        import rbm_amd.data as synth
        from rbm_amd.train_step import FusedTrainStep
        m = _model()
        tr = FusedTrainStep(m, lr=1e-3, max_labelled=BR * T, sparse_rows=mode)
        rng = np.random.default_rng(3)
        batches = [[synth.bert_batch(rng, BR, T, V, mask_prob=0.3) for _ in range(world)] for _ in range(3)]
        batches = [tuple(torch.from_numpy(x).cuda() for x in b[rank]) for b in batches]
        if graph:
            tr.capture(*batches[0])
            m.load_state_dict(_model().state_dict())
            tr.engine.sync_compute_weights()
            tr.opt.m.zero_(); tr.opt.v.zero_(); tr.opt.state.zero_()
            tr.engine.seed_base.fill_(rank << 40)
        losses = [float((tr.replay(*b) if graph else tr.step(*b)).item()) for b in batches]
        torch.cuda.synchronize()
        sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        torch.save({"losses": losses, "sd": sd, "sparse": tr.sparse is not None},
                   os.path.join(out_dir, f"{mode}_r{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("graph", [False, True])
def test_sparse_token_exchange_equals_dense(tmp_path, graph):
    world = 2
    for mode in ("on", "off"):
        mp.spawn(_worker, args=(world, _rendezvous(tmp_path), graph, mode, str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        a = torch.load(tmp_path / f"on_r{r}.pt", weights_only=True)
        b = torch.load(tmp_path / f"off_r{r}.pt", weights_only=True)
        assert a["sparse"] and not b["sparse"]
        assert a["losses"] == b["losses"]
        for k in b["sd"]:
            assert torch.equal(a["sd"][k], b["sd"][k]), k
    r0 = torch.load(tmp_path / "on_r0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "on_r1.pt", weights_only=True)
    for k in r0["sd"]:
        assert torch.equal(r0["sd"][k], r1["sd"][k]), k        # the replicas stay identical


@pytest.mark.parametrize("n,cap,frac", [(1, 4, 1.0), (1000, 1000, 0.2), (12800, 12800, 0.2), (12800, 1000, 0.2),
                                        (70001, 70001, 0.5), (5000, 6000, 0.0)])
def test_compact_rows_matches_numpy(n, cap, frac):
    """rs_compact_rows (one 1024-row block per workgroup, wave ballots): the ordered labelled-row list capped at
    cap, the rank of every row (-1 unlabelled or past the cap), the capped count, -1 in the unused list slots."""
    from rbm_amd import ops
    rng = np.random.default_rng(n)
    lab = np.where(rng.random(n) < frac, rng.integers(1, 100, n), 0).astype(np.int64)
    labels = torch.from_numpy(lab).cuda()
    idx = torch.full((cap,), 7, dtype=torch.int32, device="cuda")
    rank = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.compact_rows(labels, cap, idx, rank, cnt)
    torch.cuda.synchronize()
    rows = np.nonzero(lab)[0]
    k = min(len(rows), cap)
    want_rank = np.full(n, -1, dtype=np.int32)
    want_rank[rows[:k]] = np.arange(k)
    assert int(cnt.item()) == k
    assert np.array_equal(idx.cpu().numpy()[:k], rows[:k])
    assert (idx.cpu().numpy()[len(rows):] == -1).all()
    assert np.array_equal(rank.cpu().numpy(), want_rank)
