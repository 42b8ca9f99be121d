"""FusedTrainStep(table_optim="sparse") on the GPU: the sparse (touched-rows-only) Adam of the embedding / output
tables through the whole training step (the reference's inner loop, BS/trainers/base.py:114-123, with its dense
torch.optim.Adam replaced by the lazy rule for those tables; tests/adam_rows_ref.py states the rule).

Tiny models (B 4, T 16, 2 blocks; SAS d 64 bf16 and d 50 fp32, BERT d 64 and 256) for SAS bce, SAS sampled_ce
(K = 8, with and without logq) and BERT sampled_ce: the fused step against its eager composition and its captured
graph (bit for bit), sparse against dense twins (same loss and gradients; the same bits altogether when every row is
touched every step), the rows outside the documented touched set (bit for bit unchanged, at V = 5,000 and over 300
sampled steps at V = 600), learning, checkpoints, the unrolled graph, and the refusals."""
import argparse

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, T, L, K = 4, 16, 2, 8
CONFIGS = [("sas_bce", 64, "bf16"), ("sas_bce", 50, "fp32"), ("sas_sce", 64, "bf16"), ("sas_sce", 50, "fp32"),
           ("sas_sce_logq", 64, "bf16"), ("sas_sce_logq", 50, "fp32"), ("bert_sce", 64, "bf16"),
           ("bert_sce", 256, "bf16")]
IDS = [f"{k}-d{d}-{dt}" for k, d, dt in CONFIGS]
cases = pytest.mark.parametrize("kind,d,dt", CONFIGS, ids=IDS)
TOKEN = "bert.embedding.token.weight"


def build(kind, d, dt, V, table_optim="sparse", p=0.2, seed=3, lr=1e-3):
    """(model, FusedTrainStep, logq or None): the same seed gives twins with the same weights and dropout salts."""
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    from rbm_amd.train_step import FusedTrainStep
    torch.manual_seed(seed)
    if kind.startswith("sas"):
        a = argparse.Namespace(model_code="sas", num_items=V, max_len=T, device="cuda", sas_hidden_units=d,
                               sas_num_blocks=L, sas_heads=1, sas_dropout=p, l2_emb=0.0, rs_dtype=dt)
        m = model_factory(a)
        with torch.no_grad():
            m.sas.item_emb.weight.mul_(0.1)
    else:
        a = argparse.Namespace(model_code="bert", num_items=V, max_len=T, device="cuda", bert_hidden_units=d,
                               bert_num_blocks=L, bert_num_heads=2, bert_dropout=p, bert_hidden_dropout=p,
                               bert_mask_prob=0.2, model_init_seed=seed, rs_dtype=dt)
        m = model_factory(a)
    m.train()
    q = None
    if kind.endswith("logq"):
        w = torch.rand(V + 1, generator=torch.Generator().manual_seed(5)) + 0.1
        q = torch.log(w / w.sum()).float().cuda()
    loss = "bce" if kind == "sas_bce" else "sampled_ce"
    return m, FusedTrainStep(m, lr=lr, loss=loss, logq=q, table_optim=table_optim), q


def batch(kind, V, seed, cover=False):
    """One batch on the device.  cover: every item id (and BERT's [MASK]) occurs in the lookup keys, every id in the
    head's keys too (V <= 40)."""
    import rbm_amd.data as synth
    rng = np.random.default_rng(seed)
    if kind.startswith("sas"):
        seq, pos, neg = synth.sas_batch(rng, B, T, V)
        third = neg if kind == "sas_bce" else rng.integers(1, V + 1, K)
        if kind != "sas_bce":
            third[1] = 0                                   # a masked candidate
        if cover:
            flat = seq.reshape(-1)
            flat[-V:] = rng.permutation(V) + 1             # the leading pads of row 0 stay
            pos.reshape(-1)[-V:] = rng.permutation(V) + 1
        out = (seq, pos, third)
    else:
        tok, lab = synth.bert_batch(rng, B, T, V, mask_prob=0.3)
        cand = rng.integers(1, V + 1, K)
        cand[1] = 0
        if cover:
            tok.reshape(-1)[-(V + 1):] = rng.permutation(V + 1) + 1
            lab.reshape(-1)[-(V + 1):] = np.where(tok.reshape(-1)[-(V + 1):] == V + 1, rng.integers(1, V + 1, V + 1), 0)
            cand = rng.permutation(V) + 1                  # K = V candidates: every output row
        out = (tok, lab, cand)
    return tuple(torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).cuda() for x in out)


def tables(tr):
    """{table name: the positions of its keys in the batch}"""
    return {"item_emb.weight": (0, 1, 2)} if tr.kind == "sas" else {TOKEN: (0,), "out.weight": (1, 2),
                                                                    "out.bias": (1, 2)}


def touched(tr, b):
    """{table: sorted distinct non-zero ids below the table's rows in its key tensors}: the documented set."""
    out = {}
    for name, pos in tables(tr).items():
        ids = torch.cat([b[i].reshape(-1) for i in pos])
        ids = ids[(ids >= 1) & (ids < tr.flat.shapes[name][0])]
        out[name] = torch.unique(ids)
    return out


def bufs(tr):
    return [x for x in (tr.flat.data, tr.flat.bf16, tr.opt.m, tr.opt.v) if x is not None]


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def snapshot(tr):
    return [x.clone() for x in bufs(tr)]


def equal_state(t1, t2):
    return all(same(a, b) for a, b in zip(bufs(t1), bufs(t2)))


def untouched_unchanged(tr, before, sets):
    """Every row outside `sets` of every sparse table keeps its bits in p / bf16 / m / v; returns the share of rows
    checked per table."""
    share = {}
    for name, rows in sets.items():
        R = tr.flat.shapes[name][0]
        rest = torch.ones(R, dtype=torch.bool, device="cuda")
        rest[rows] = False
        for old, new in zip(before, bufs(tr)):
            a, b = tr.flat.view(name, old), tr.flat.view(name, new)
            assert same(a[rest], b[rest]), (name, "a row outside the touched set changed")
        share[name] = float(rest.float().mean().item())
    return share


def composed_step(m, tr, q, b):
    """The step's eager composition: the loss call and backward() into the flat gradient, ops.unique_rows per union
    list, FusedAdam.step(sparse=...).  (SAS bce: the trainer's own forward + loss + backward, whose fused head is
    not the autograd path's.)  Returns the loss."""
    from rbm_amd import ops
    f = tr.flat
    if tr.loss == "bce":
        tr._compute(*b)
        loss = tr.loss_out[2].clone()
    else:
        net = m.sas if tr.kind == "sas" else m
        net.zero_grad(set_to_none=True)
        loss = m.sampled_ce_loss(*b, logq=q)
        loss.backward()
        for n, prm in net.named_parameters():
            f.view(n, f.grad).copy_(prm.grad)
    spec, lists = [], {}
    for name, pos in tables(tr).items():
        if pos not in lists:
            keys = [b[i].reshape(-1).contiguous() for i in pos]
            R = f.shapes[name][0]
            lst = torch.zeros(sum(k.numel() for k in keys), dtype=torch.int32, device="cuda")
            cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
            ops.unique_rows(keys, R, lst, cnt, torch.empty(ops.unique_rows_ws_bytes(R), dtype=torch.uint8,
                                                           device="cuda"))
            lists[pos] = (lst, cnt)
        shp = f.shapes[name]
        spec.append((f.offsets[name], shp[0], shp[1] if len(shp) > 1 else 1) + lists[pos])
    tspec = tr.engine.transposed_spec() if hasattr(tr.engine, "transposed_spec") else None
    tr.opt.step(seed_base=tr.engine.seed_base, transposed=tspec, sparse=spec)
    return loss


# ------------------------------------------------------------------ 1. fused == composed == captured
@cases
def test_fused_step_equals_its_eager_composition_and_its_graph(kind, d, dt):
    V = 300
    bs = [batch(kind, V, s) for s in range(3)]
    warm = [bs[0], bs[0]]                                  # the capture's two warmup steps
    m1, t1, q1 = build(kind, d, dt, V)
    want = [float(t1.step(*b).item()) for b in warm + bs]
    m2, t2, q2 = build(kind, d, dt, V)
    got = [float(composed_step(m2, t2, q2, b).item()) for b in warm + bs]
    assert got == want and all(np.isfinite(want)), (got, want)
    assert equal_state(t1, t2)
    assert int(t1.engine.seed_base.item()) == int(t2.engine.seed_base.item())
    m3, t3, _ = build(kind, d, dt, V)
    t3.capture(*bs[0], warmup=2)
    rep = [float(t3.replay(*b).item()) for b in bs]
    torch.cuda.synchronize()
    assert rep == want[2:], (rep, want[2:])
    assert equal_state(t1, t3)
    assert float(t1.flat.grad[:t1.flat.numel].abs().sum()) == 0        # every gradient row cleared again
    assert t1.opt.marks is None and getattr(t1.engine, "row_marks", None) is None


# ------------------------------------------------------------------ 2. only the optimizer differs
@cases
def test_first_step_of_sparse_and_dense_twins_has_the_same_loss_and_gradients(kind, d, dt):
    V = 300
    b = batch(kind, V, 7)
    res = []
    for mode in ("sparse", "dense"):
        m, t, _ = build(kind, d, dt, V, table_optim=mode)
        t._compute(*b)
        torch.cuda.synchronize()
        res.append((t.loss_out.clone(), t.flat.grad.clone()))
    assert same(res[0][0], res[1][0]) and same(res[0][1], res[1][1])
    assert float(res[0][1].abs().sum()) > 0


# ------------------------------------------------------------------ 3. V = 5,000: the rows outside the set
@cases
def test_rows_outside_the_touched_set_are_bitwise_unchanged(kind, d, dt):
    V = 5000
    m, t, _ = build(kind, d, dt, V)
    for s in range(3):
        b = batch(kind, V, 20 + s)
        sets = touched(t, b)
        for name, rows in sets.items():                          # lookup keys + head keys: B T + cap + K ids at most
            assert len(rows) <= (3 * B * T if kind == "sas_bce" else B * T + B * T + K), name
        before = snapshot(t)
        t.step(*b)
        torch.cuda.synchronize()
        share = untouched_unchanged(t, before, sets)
        assert min(share.values()) >= 0.9, share
        for name, rows in sets.items():                          # ... and the touched rows did move
            assert not same(t.flat.view(name, before[0])[rows], t.flat.view(name)[rows]), name


# ------------------------------------------------------------------ 4. every row touched: the dense step, bit for bit
@cases
def test_sparse_equals_dense_bitwise_when_every_row_is_touched(kind, d, dt):
    V = 40
    runs = []
    for mode in ("sparse", "dense"):
        m, t, _ = build(kind, d, dt, V, table_optim=mode)
        losses = []
        for s in range(5):
            b = batch(kind, V, 40 + s, cover=True)
            for name, rows in touched(t, b).items():             # rows 1 .. R - 1: all but the padding row
                assert rows.tolist() == list(range(1, t.flat.shapes[name][0])), name
            losses.append(float(t.step(*b).item()))
        torch.cuda.synchronize()
        runs.append((losses, t))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    assert equal_state(runs[0][1], runs[1][1])
    assert float(runs[0][1].opt.state[0].item()) == 5.0


# ------------------------------------------------------------------ 5. 300 sampled steps
@cases
def test_300_sampled_steps_leave_the_rows_outside_each_steps_set_unchanged(kind, d, dt):
    import rbm_amd.data as synth
    from rbm_amd.dataloaders import DeviceBertMasker, DeviceWarpSampler
    V = 600
    hist = synth.user_histories(np.random.default_rng(3), 100, T, V)
    if kind.startswith("sas"):
        sampler = DeviceWarpSampler(hist, V, B, T, seed=2, shared_negs=None if kind == "sas_bce" else K)
    else:
        sampler = DeviceBertMasker(hist, V, B, T, 0.3, seed=2, shared_negs=K)
    m, t, _ = build(kind, d, dt, V)
    moved = {name: torch.zeros(t.flat.shapes[name][0], dtype=torch.bool, device="cuda") for name in tables(t)}
    for i in range(300):
        if kind == "bert_sce" and i % sampler.num_batch == 0:
            sampler.new_epoch()
        b = sampler.sample()
        sets = touched(t, b)
        before = snapshot(t)
        t.step(*b)
        untouched_unchanged(t, before, sets)
        for name, rows in sets.items():
            moved[name][rows] = True
    torch.cuda.synchronize()
    assert float(t.opt.state[0].item()) == 300.0
    assert all(bool(v.any()) and not bool(v[0]) for v in moved.values())
    assert torch.isfinite(t.flat.data).all()


# ------------------------------------------------------------------ 6. it learns
def test_bert_sparse_twin_learns_the_rule_about_as_well_as_the_dense_sampled_softmax():
    """The rule, sizes, data, seeds and step count of test_bert_sce_gpu's
    test_it_learns_a_deterministic_next_item_rule_about_as_well_as_the_full_ce: a dense sampled-softmax twin and a
    sparse one; the sparse twin's full-rank HR@10 may fall short of the dense twin's by that test's SHORTFALL."""
    from rbm_amd.dataloaders import DeviceBertMasker
    from rbm_amd.train_step import FusedTrainStep
    from test_bert_sce_gpu import SHORTFALL, _model
    V, T_, d, L_, h, B_, K_, steps = 200, 16, 64, 1, 2, 16, 64, 300
    rng = np.random.default_rng(0)
    hist = []
    for _ in range(600):
        x = [int(rng.integers(1, V + 1))]
        for _ in range(T_ - 1):
            x.append((7 * x[-1] + 3) % V + 1)
        hist.append(x)
    ev = np.zeros((256, T_ + 1), np.int64)
    ev[:, 0] = rng.integers(1, V + 1, 256)
    for t in range(T_):
        ev[:, t + 1] = (7 * ev[:, t] + 3) % V + 1
    x_eval = ev[:, 1:].copy()
    target = torch.from_numpy(x_eval[:, -1].copy())
    x_eval[:, -1] = V + 1                                           # [MASK]
    hr = {}
    for mode in ("dense", "sparse"):
        m = _model(V, T_, d, L_, h, dtype="bf16", seed=0)
        sampler = DeviceBertMasker(hist, V, B_, T_, 0.3, seed=0, shared_negs=K_)
        tr = FusedTrainStep(m, lr=1e-3, loss="sampled_ce", table_optim=mode)
        losses = []
        for i in range(steps):
            if i % sampler.num_batch == 0:
                sampler.new_epoch()
            losses.append(tr.step(*sampler.sample()).clone())
        losses = [float(x.item()) for x in losses]
        m.eval()
        rank = m.full_rank(torch.from_numpy(x_eval), target, exclude_seen=False)
        hr[mode] = float((rank < 10).float().mean().item())
        print("bert", mode, "first / last loss", losses[0], losses[-1], "HR@10", hr[mode])
        assert losses[-1] < losses[0], (mode, losses[0], losses[-1])
    assert hr["dense"] >= 0.5, hr
    assert hr["sparse"] >= hr["dense"] - SHORTFALL, hr


def test_sas_sparse_twin_learns_the_rule_about_as_well_as_the_dense_sampled_softmax():
    """test_sas_sce_gpu's rule task (V = 200, T = 16, d = 64, 200 steps through DeviceWarpSampler(shared_negs=64)) for a
    dense and a sparse twin, the same margin between the twins."""
    from rbm_amd.dataloaders import DeviceWarpSampler
    from rbm_amd.train_step import FusedTrainStep
    from test_bert_sce_gpu import SHORTFALL
    from test_sas_ce_gpu import _model, _rule_batch
    V, T_, d, L_, h, B_, K_ = 200, 16, 64, 1, 1, 16, 64
    hr = {}
    for mode in ("dense", "sparse"):
        rng = np.random.default_rng(0)
        hist = []
        for _ in range(600):
            x = [int(rng.integers(1, V + 1))]
            for _ in range(int(rng.integers(9, 17))):
                x.append((7 * x[-1] + 3) % V + 1)
            hist.append(x)
        sampler = DeviceWarpSampler(hist, V, B_, T_, seed=0, shared_negs=K_)
        m = _model(V, T_, d, L_, h, dtype="bf16", seed=0)
        tr = FusedTrainStep(m, lr=1e-3, loss="sampled_ce", table_optim=mode)
        losses = [tr.step(*sampler.sample()).clone() for _ in range(200)]
        losses = [float(x.item()) for x in losses]
        seq, pos = _rule_batch(rng, 256, T_)
        m.eval()
        rank = m.full_rank(seq, pos[:, -1], exclude_seen=False)
        hr[mode] = float((rank < 10).float().mean().item())
        print("sas", mode, "first / last loss", losses[0], losses[-1], "HR@10", hr[mode])
        assert losses[-1] < losses[0], (mode, losses[0], losses[-1])
    assert hr["dense"] >= 0.5, hr
    assert hr["sparse"] >= hr["dense"] - SHORTFALL, hr


# ------------------------------------------------------------------ 7. checkpoint
@pytest.mark.parametrize("kind,d,dt", [CONFIGS[0], CONFIGS[3], CONFIGS[6]], ids=[IDS[0], IDS[3], IDS[6]])
def test_checkpoint_resumes_bit_for_bit(kind, d, dt):
    import io
    V = 300
    bs = [batch(kind, V, 60 + s) for s in range(5)]
    m1, t1, _ = build(kind, d, dt, V)
    for b in bs[:2]:
        t1.step(*b)
    buf = io.BytesIO()
    torch.save(t1.checkpoint(epoch=1), buf)
    seed = t1.engine.seed_base.clone()
    for b in bs[2:]:
        t1.step(*b)
    m2, t2, _ = build(kind, d, dt, V, lr=1.0)                # the same dropout salts; the rate comes from the checkpoint
    buf.seek(0)
    ck = torch.load(buf, weights_only=True)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "epoch"}
    assert set(ck["optimizer_state_dict"]["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    t2.load_checkpoint(ck)
    t2.engine.seed_base.copy_(seed)                          # the dropout step seed is not part of a checkpoint
    for b in bs[2:]:
        t2.step(*b)
    torch.cuda.synchronize()
    assert equal_state(t1, t2)


# ------------------------------------------------------------------ the unrolled graph
def test_unrolled_graph_of_sparse_bce_steps_equals_single_steps():
    kind, d, dt = CONFIGS[0]
    V, S = 300, 2
    bs = [batch(kind, V, 80 + s) for s in range(2 * S)]
    m1, t1, _ = build(kind, d, dt, V)
    for b in [bs[0]] * 2:
        t1.step(*b)
    want = [float(t1.step(*b).item()) for b in bs]
    m2, t2, _ = build(kind, d, dt, V)
    t2.capture(*bs[0], warmup=2, steps_per_graph=S)
    got = []
    for k in range(0, len(bs), S):
        got += t2.replay_packed(torch.stack([torch.stack(b) for b in bs[k:k + S]])).tolist()
    torch.cuda.synchronize()
    assert got == want, (got, want)
    assert equal_state(t1, t2)


# ------------------------------------------------------------------ 8. the refusals
def test_errors_name_their_reason_and_launch_nothing():
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    from rbm_amd.train_step import FusedTrainStep

    def sas(l2=0.0):
        return model_factory(argparse.Namespace(model_code="sas", num_items=50, max_len=T, device="cuda",
                                                sas_hidden_units=64, sas_num_blocks=1, sas_heads=1, sas_dropout=0.0,
                                                l2_emb=l2, rs_dtype="bf16"))

    def bert():
        return model_factory(argparse.Namespace(model_code="bert", num_items=50, max_len=T, device="cuda",
                                                bert_hidden_units=64, bert_num_blocks=1, bert_num_heads=2,
                                                bert_dropout=0.0, bert_hidden_dropout=0.0, bert_mask_prob=0.2,
                                                model_init_seed=0, rs_dtype="bf16"))
    refusals = [(sas, dict(loss="ce"), "every row"),
                (bert, dict(), "full cross-entropy"),
                (sas, dict(loss="bce", dp=True), "one rank"),
                (bert, dict(loss="sampled_ce", dp=True), "one rank"),
                (bert, dict(loss="sampled_ce", vocab_shard=True), "vocab_shard"),
                (sas, dict(loss="bce", weight_decay=0.01), "weight_decay"),
                (bert, dict(loss="sampled_ce", weight_decay=0.01), "weight_decay"),
                (lambda: sas(l2=1e-3), dict(loss="sampled_ce"), "l2_emb")]
    for make, kw, why in refusals:
        m = make()
        with pytest.raises(ValueError, match=why):
            FusedTrainStep(m, table_optim="sparse", **kw)
        assert (m.sas if hasattr(m, "sas") else m)._engine is None, (kw, "an engine was built before the refusal")
    with pytest.raises(ValueError, match="table_optim"):
        FusedTrainStep(sas(), table_optim="lazy")
    # a loaded optimizer state with a decay is refused too
    m = sas()
    t = FusedTrainStep(m, loss="bce", table_optim="sparse")
    sd = t.optimizer_state_dict()
    sd["param_groups"][0]["weight_decay"] = 0.01
    with pytest.raises(ValueError, match="weight_decay"):
        t.load_optimizer_state_dict(sd)
    assert FusedTrainStep(sas(), loss="bce").table_optim == "dense"
