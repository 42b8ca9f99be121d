"""The device evaluation loader on the GPU against its host restatement (tests/eval_loader_ref.py, pinned to the
reference by tests/test_eval_loader_ref.py): rs_eval_negatives / _draws bit for bit for both samplers, the bound and
the fallback, split invariance, rs_eval_batch and DeviceEvalLoader for SAS / BERT x val / test, from_samples, and
rbm_amd.metrics.evaluate against a Python loop of calculate_metrics."""
import argparse
import functools

import numpy as np
import pytest
import torch

import eval_loader_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"

# name -> (users, V, history lengths lo..hi, n_neg, zipf): the user counts are deliberately no multiples of 4
CASES = {"default": (301, 500, 3, 300, 100, True),          # the reference's default n_neg
         "mostly_rejected": (37, 130, 1, 25, 100, False),   # at most 103 admissible items for 100 slots
         "one": (64, 50, 1, 20, 1, False),                  # minimum n_neg
         "max": (10, 3000, 1, 100, R.NEGS_MAX, False)}      # maximum n_neg
SEED = 0x5EED0E7A1


@functools.lru_cache(maxsize=None)
def case(name):
    n, V, lo, hi, n_neg, zipf = CASES[name]
    train, val, test = R.make_users(np.random.default_rng(len(name) + n), n, V, lo, hi, zipf=zipf)
    return train, val, test, V, n_neg, R.seen_sets(train, val, test)


@functools.lru_cache(maxsize=None)
def fallback_case():
    """9 users who have each seen 2000 of 3000 items, n_neg = the 1000 left: 4096 raw draws never collect them all"""
    rng = np.random.default_rng(5)
    train, val, test = [], [], []
    for _ in range(9):
        p = rng.permutation(3000)[:2000] + 1
        train.append(p[:-2].tolist())
        val.append([int(p[-2])])
        test.append([int(p[-1])])
    return train, val, test, 3000, 1000, R.seen_sets(train, val, test)


def seen_csr(seen):
    off = np.zeros(len(seen) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in seen])
    flat = np.array([v for s in seen for v in sorted(s)], np.int32)
    return torch.from_numpy(off).to(DEV), torch.from_numpy(flat).to(DEV)


@functools.lru_cache(maxsize=None)
def proposal(name):
    """a popularity proposal over the case's items (smooth = 1: items nobody has seen keep a positive weight)"""
    from rbm_amd.dataloaders import ItemProposal
    train, val, test, V = (fallback_case() if name == "fallback" else case(name))[:4]
    return ItemProposal.from_histories([h + v + t for h, v, t in zip(train, val, test)], V, alpha=1.0, smooth=1.0,
                                       device=DEV)


@functools.lru_cache(maxsize=None)
def reference(name, sampler):
    train, val, test, V, n_neg, seen = fallback_case() if name == "fallback" else case(name)
    table = None
    if sampler == "popular":
        p = proposal(name)
        table = (p.thr, p.alias)
    negs, drawn = R.negatives_ref(seen, V, n_neg, SEED, table=table)
    negs.setflags(write=False)
    drawn.setflags(write=False)
    return negs, drawn


def run(seen, V, n_neg, table=None, draws=False, parts=None):
    from rbm_amd import ops
    n = len(seen)
    off, flat = seen_csr(seen)
    negs = torch.full((n, n_neg), -7, dtype=torch.int32, device=DEV)
    drawn = torch.full((n,), -7777, dtype=torch.int32, device=DEV)
    rec = torch.full((n, ops.eval_negatives_max_draws()), -7, dtype=torch.int64, device=DEV) if draws else None
    for u0, cnt in parts or [(0, n)]:
        ops.eval_negatives(off, flat, V, SEED, negs, table=table, n_drawn=drawn, draws=rec, user0=u0, count=cnt)
    torch.cuda.synchronize()
    return negs.cpu().numpy(), drawn.cpu().numpy(), None if rec is None else rec.cpu().numpy()


# ================================================================ rs_eval_negatives
@pytest.mark.parametrize("sampler", ["random", "popular"])
@pytest.mark.parametrize("name", list(CASES))
def test_negatives_equal_the_restatement(name, sampler):
    train, val, test, V, n_neg, seen = case(name)
    negs, drawn, _ = run(seen, V, n_neg, table=proposal(name).table if sampler == "popular" else None)
    ref_negs, ref_drawn = reference(name, sampler)
    R.check_negatives(negs, drawn, ref_negs, ref_drawn)
    R.check_properties(negs, seen, V)
    if sampler == "random":
        assert (drawn > 0).all()                  # the uniform stream fills these shapes well inside the bound


@pytest.mark.parametrize("sampler", ["random", "popular"])
def test_every_user_ends_in_the_fallback_when_n_neg_is_all_that_is_left(sampler):
    train, val, test, V, n_neg, seen = fallback_case()
    negs, drawn, _ = run(seen, V, n_neg, table=proposal("fallback").table if sampler == "popular" else None)
    ref_negs, ref_drawn = reference("fallback", sampler)
    assert (ref_drawn < 0).all()
    R.check_negatives(negs, drawn, ref_negs, ref_drawn)
    R.check_properties(negs, seen, V)
    for u in range(len(seen)):                    # all that is left, whatever the order
        assert set(negs[u].tolist()) == set(range(1, V + 1)) - seen[u]


def test_fallback_forced_by_a_proposal_whose_mass_sits_on_seen_items():
    from rbm_amd.dataloaders import ItemProposal
    V, n_neg, n = 200, 20, 13
    rng = np.random.default_rng(3)
    seen = [set(range(1, 11)) | set(rng.integers(11, V + 1, size=int(rng.integers(0, 30))).tolist()) for _ in range(n)]
    w = np.ones(V + 1)
    w[1:11] = 1e12                                 # an unseen item is drawn with probability ~ 2e-11 per draw
    p = ItemProposal(w, device=DEV)
    negs, drawn, _ = run(seen, V, n_neg, table=p.table)
    ref_negs, ref_drawn = R.negatives_ref(seen, V, n_neg, SEED, table=(p.thr, p.alias))
    assert (ref_drawn == -1 - n_neg).all()         # nothing kept from the stream
    R.check_negatives(negs, drawn, ref_negs, ref_drawn)
    R.check_properties(negs, seen, V)
    for u in range(n):
        assert negs[u].tolist() == [v for v in range(1, V + 1) if v not in seen[u]][:n_neg]


@pytest.mark.parametrize("sampler", ["random", "popular"])
@pytest.mark.parametrize("name", ["default", "mostly_rejected"])
def test_draws_form_records_the_stream_and_gives_the_same_negatives(name, sampler):
    train, val, test, V, n_neg, seen = case(name)
    p = proposal(name) if sampler == "popular" else None
    negs, drawn, rec = run(seen, V, n_neg, table=None if p is None else p.table, draws=True)
    plain, plain_drawn, _ = run(seen, V, n_neg, table=None if p is None else p.table)
    assert np.array_equal(negs, plain) and np.array_equal(drawn, plain_drawn)
    R.check_negatives(negs, drawn, *reference(name, sampler))
    for u in range(0, len(seen), 7):
        assert np.array_equal(rec[u], R.draws_np(SEED, u, 0, R.MAX_DRAWS, V, None if p is None else (p.thr, p.alias)))
    for u in np.nonzero(drawn > 0)[0]:            # the reference's loop on the recorded draws
        assert R.reference_loop(rec[u], seen[u], n_neg) == negs[u].tolist(), u
    assert (drawn > 0).sum() >= len(seen) // 2
    assert (rec >= 1).all() and (rec <= V).all()


def test_split_invariance():
    train, val, test, V, n_neg, seen = case("default")
    negs, drawn, _ = run(seen, V, n_neg, parts=[(150, 151), (0, 150)])
    R.check_negatives(negs, drawn, *reference("default", "random"))
    part, part_drawn, _ = run(seen, V, n_neg, parts=[(150, 151)])
    assert (part[:150] == -7).all() and (part_drawn[:150] == -7777).all()       # a call touches its own users only
    assert np.array_equal(part[150:], negs[150:])


# ================================================================ the Python classes
@pytest.mark.parametrize("sampler", ["random", "popular"])
def test_device_eval_negatives(sampler):
    from rbm_amd.dataloaders import DeviceEvalNegatives
    train, val, test, V, n_neg, seen = case("mostly_rejected")
    kw = dict(proposal=proposal("mostly_rejected")) if sampler == "popular" else {}
    neg = DeviceEvalNegatives(train, {u: v for u, v in enumerate(val)}, test, V, n_neg=n_neg, sampler=sampler, seed=4,
                              device=DEV, **kw)
    again = DeviceEvalNegatives(train, val, [t[0] for t in test], V, n_neg=n_neg, sampler=sampler, seed=4, device=DEV,
                                **kw)
    assert neg.seed == again.seed and torch.equal(neg.negs, again.negs)
    table = (kw["proposal"].thr, kw["proposal"].alias) if kw else None
    ref_negs, ref_drawn = R.negatives_ref(seen, V, n_neg, neg.seed, table=table)
    R.check_negatives(neg.negs.cpu().numpy(), neg.n_drawn.cpu().numpy(), ref_negs, ref_drawn)
    assert neg.negs.dtype == torch.int32 and neg.negs.shape == (len(train), n_neg)
    assert neg.fallback_users == int((ref_drawn < 0).sum())


def test_popular_default_proposal_counts_the_whole_history():
    from rbm_amd.dataloaders import DeviceEvalNegatives, ItemProposal
    V = 30
    train, val, test = R.make_users(np.random.default_rng(8), 64, V, 10, 20)
    allh = [h + v + t for h, v, t in zip(train, val, test)]
    assert len({i for h in allh for i in h}) == V                # every item occurs: smooth = 0 is legal here
    neg = DeviceEvalNegatives(train, val, test, V, n_neg=5, sampler="popular", seed=1, device=DEV)
    want = ItemProposal.from_histories(allh, V, alpha=1.0, smooth=0.0, device="cpu")
    assert np.array_equal(neg.proposal.thr, want.thr) and np.array_equal(neg.proposal.alias, want.alias)
    seen = R.seen_sets(train, val, test)
    ref_negs, ref_drawn = R.negatives_ref(seen, V, 5, neg.seed, table=(want.thr, want.alias))
    R.check_negatives(neg.negs.cpu().numpy(), neg.n_drawn.cpu().numpy(), ref_negs, ref_drawn)
    R.check_properties(neg.negs.cpu().numpy(), seen, V)


# ================================================================ rs_eval_batch / DeviceEvalLoader
@functools.lru_cache(maxsize=None)
def batch_users():
    """45 users; training histories of length 1, around every T of the tests, and longer than all of them"""
    rng = np.random.default_rng(21)
    V = 400
    lens = [1, 2, 6, 7, 8, 9, 48, 49, 50, 51, 198, 199, 200, 201, 300] + rng.integers(1, 260, size=30).tolist()
    train = [rng.integers(1, V + 1, size=n).tolist() for n in lens]
    val = [[int(x)] for x in rng.integers(1, V + 1, size=len(lens))]
    test = [[int(x)] for x in rng.integers(1, V + 1, size=len(lens))]
    negs = rng.integers(1, V + 1, size=(len(lens), 7))
    return train, val, test, V, negs


def _host(batches):
    return [tuple(t.cpu().numpy() for t in b) for b in batches]


@pytest.mark.parametrize("T", [8, 50, 200])
@pytest.mark.parametrize("mode", ["val", "test"])
@pytest.mark.parametrize("code", ["sas", "bert"])
def test_loader_batches_equal_the_restatement(code, mode, T):
    from rbm_amd.dataloaders import DeviceEvalLoader, DeviceEvalNegatives
    train, val, test, V, negs = batch_users()
    neg = DeviceEvalNegatives.from_samples(negs, device=DEV)
    loader = DeviceEvalLoader(train, val, test, V, batch_size=16, max_len=T, negatives=neg, mode=mode, model_code=code,
                              device=DEV)
    got = list(loader)
    assert len(loader) == 3 and [b[0].shape[0] for b in got] == [16, 16, 13]
    for seq, cand, labels in got:
        assert all(t.dtype == torch.int64 and t.is_cuda for t in (seq, cand, labels))
        assert seq.shape[1] == T and cand.shape[1] == labels.shape[1] == 8
    want = R.batches_ref(R.rows_ref(train, val, test, negs, T, mode, code, V), 16)
    R.check_batches(_host(got), want)
    R.check_batches(_host(list(loader)), want)              # a second pass gives the same batches


def test_eval_batch_entry_at_a_user_offset():
    from rbm_amd import ops
    from rbm_amd.dataloaders import DeviceEvalLoader, DeviceEvalNegatives
    train, val, test, V, negs = batch_users()
    neg = DeviceEvalNegatives.from_samples(negs, device=DEV)
    ld = DeviceEvalLoader(train, val, test, V, batch_size=16, max_len=50, negatives=neg, mode="test",
                          model_code="bert", device=DEV)
    seq = torch.full((5, 50), -1, dtype=torch.int64, device=DEV)
    cand, labels = (torch.full((5, 8), -1, dtype=torch.int64, device=DEV) for _ in range(2))
    ops.eval_batch(ld.offsets, ld.items, ld.extra, ld.answer, neg.negs, 11, V + 1, seq, cand, labels)
    rows = R.rows_ref(train, val, test, negs, 50, "test", "bert", V)
    R.check_batches(_host([(seq, cand, labels)]), [tuple(a[11:16] for a in rows)])


@pytest.mark.parametrize("mode", ["val", "test"])
@pytest.mark.parametrize("code", ["sas", "bert"])
def test_from_samples_round_trips_the_golden(code, mode):
    from rbm_amd.dataloaders import DeviceEvalLoader, DeviceEvalNegatives
    z = load_golden("eval_loader")
    off, U, V, T = z["train_off"], int(z["U"]), int(z["V"]), int(z["T"])
    train = {u: z["train_items"][off[u]:off[u + 1]].tolist() for u in range(U)}
    val, test = {u: [int(z["val"][u])] for u in range(U)}, {u: [int(z["test"][u])] for u in range(U)}
    neg = DeviceEvalNegatives.from_samples({u: z["negs"][u].tolist() for u in range(U)}, device=DEV)
    assert np.array_equal(neg.negs.cpu().numpy(), z["negs"]) and neg.fallback_users == 0
    loader = DeviceEvalLoader(train, val, test, V, batch_size=8, max_len=T, negatives=neg, mode=mode, model_code=code,
                              device=DEV)
    want = tuple(z[f"{code}_{mode}/{k}"] for k in ("seq", "cand", "labels"))
    R.check_batches(_host(list(loader)), R.batches_ref(want, 8))


def test_generated_negatives_match_the_golden_stream():
    """the golden's seed fed to the kernel: the reference's own sampler output on the recorded stream"""
    z = load_golden("eval_loader")
    off, U, V = z["train_off"], int(z["U"]), int(z["V"])
    train = [z["train_items"][off[u]:off[u + 1]].tolist() for u in range(U)]
    seen = R.seen_sets(train, z["val"], z["test"])
    from rbm_amd import ops
    soff, flat = seen_csr(seen)
    negs = torch.empty((U, int(z["n_neg"])), dtype=torch.int32, device=DEV)
    drawn = torch.empty(U, dtype=torch.int32, device=DEV)
    ops.eval_negatives(soff, flat, V, int(z["seed"]), negs, n_drawn=drawn)
    R.check_negatives(negs.cpu().numpy(), drawn.cpu().numpy(), z["negs"], z["n_drawn"])


# ================================================================ evaluate
KS = [1, 5, 10]


def _check_evaluate(m, V, T, code, n_neg, hi):
    from rbm_amd.dataloaders import DeviceEvalLoader, DeviceEvalNegatives
    from rbm_amd.metrics import calculate_metrics, evaluate
    train, val, test = R.make_users(np.random.default_rng(V), 45, V, 1, hi)
    neg = DeviceEvalNegatives(train, val, test, V, n_neg=n_neg, seed=2, device=DEV)
    for mode in ("val", "test"):
        loader = DeviceEvalLoader(train, val, test, V, batch_size=16, max_len=T, negatives=neg, mode=mode,
                                  model_code=code, device=DEV)
        per_batch = [calculate_metrics(m, b, KS) for b in loader]
        sizes = [b[0].shape[0] for b in loader]
        assert sizes == [16, 16, 13]
        want = R.average_ref(per_batch)
        got = evaluate(m, loader, KS)
        print(mode, got, want)
        R.check_average(got, want, tol=1e-9)
        assert list(got) == list(per_batch[0])
        assert 0.0 <= got["Recall@10"] <= 1.0
        with pytest.raises(AssertionError):                       # the comparison tells the weighting apart
            R.check_average(R.average_ref(per_batch, sizes=sizes, mistake="weight_by_size"), want, tol=1e-9)


def test_evaluate_sas():
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    z = load_golden("sas_curve")
    V, T, d, L, h = (int(z[k]) for k in ("V", "T", "d", "L", "h"))
    a = argparse.Namespace(model_code="sas", num_items=V, max_len=T, device="cuda", sas_hidden_units=d,
                           sas_num_blocks=L, sas_heads=h, sas_dropout=0.0, l2_emb=0.0, rs_dtype="fp32")
    m = model_factory(a)
    m.load_state_dict({k[6:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("final/")})
    m.eval()
    _check_evaluate(m, V, T, "sas", n_neg=20, hi=20)


def test_evaluate_bert():
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    z = load_golden("bert_mid")
    V, T, d, L, h = (int(z[k]) for k in ("V", "T", "d", "L", "h"))
    a = argparse.Namespace(model_code="bert", num_items=V, max_len=T, device="cuda", bert_hidden_units=d,
                           bert_num_blocks=L, bert_num_heads=h, bert_dropout=0.0, bert_hidden_dropout=0.0,
                           bert_mask_prob=0.2, model_init_seed=4, rs_dtype="fp32")
    m = model_factory(a)
    m.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p/")})
    m.eval()
    _check_evaluate(m, V, T, "bert", n_neg=100, hi=100)
