"""CPU checks of the evaluation loader: the host restatement (tests/eval_loader_ref.py) against the reference's own
sampler and datasets (tests/golden/eval_loader.npz, written by tools/gen_golden_eval.py), planted mistakes against the
comparison functions the GPU tests use, the law of the seeded streams, and every refusal that needs no device."""
import numpy as np
import pytest

import eval_loader_ref as R
from conftest import load_golden

MODES = [(m, c) for c in ("sas", "bert") for m in ("val", "test")]


@pytest.fixture(scope="module")
def gold():
    z = load_golden("eval_loader")
    off = z["train_off"]
    train = [z["train_items"][off[u]:off[u + 1]].tolist() for u in range(int(z["U"]))]
    val, test = [[int(v)] for v in z["val"]], [[int(t)] for t in z["test"]]
    return dict(z=z, train=train, val=val, test=test, V=int(z["V"]), n_neg=int(z["n_neg"]), T=int(z["T"]),
                seed=int(z["seed"]), seen=R.seen_sets(train, val, test))


# ================================================================ the restatement against the reference
def test_stream_in_python_integers_is_the_recorded_stream(gold):
    z, V, seed = gold["z"], gold["V"], gold["seed"]
    for u in (0, 5, 36):
        assert [R.draw(seed, u, c, V) for c in range(100)] == z["draws"][u, :100].tolist()
        assert np.array_equal(R.draws_np(seed, u, 0, z["draws"].shape[1], V), z["draws"][u])
    assert np.array_equal(R.draws_np(seed, 3, 64, 64, V), z["draws"][3, 64:128])        # any offset, same stream


def test_restatement_reproduces_the_reference_negatives(gold):
    z = gold["z"]
    negs, drawn = R.negatives_ref(gold["seen"], gold["V"], gold["n_neg"], gold["seed"])
    R.check_negatives(negs, drawn, z["negs"], z["n_drawn"])
    R.check_properties(negs, gold["seen"], gold["V"])
    for u in range(len(gold["train"])):                      # and so does the replayed loop
        assert R.reference_loop(z["draws"][u], gold["seen"][u], gold["n_neg"]) == z["negs"][u].tolist()


@pytest.mark.parametrize("mode,code", MODES)
def test_restatement_reproduces_the_reference_rows(gold, mode, code):
    z = gold["z"]
    rows = R.rows_ref(gold["train"], gold["val"], gold["test"], z["negs"], gold["T"], mode, code, gold["V"])
    want = tuple(z[f"{code}_{mode}/{k}"] for k in ("seq", "cand", "labels"))
    R.check_batches([rows], [want])
    R.check_batches(R.batches_ref(rows, 8), R.batches_ref(want, 8))
    assert [b[0].shape[0] for b in R.batches_ref(rows, 8)] == [8, 8, 8, 8, 5]


def test_alias_rule_is_rs_alias_items_rule():
    """a table whose slots keep their whole mass draws the uniform stream; a two-item table follows thr"""
    V = 97
    thr, alias = np.zeros(V, np.uint32), np.arange(1, V + 1, dtype=np.int64)
    assert np.array_equal(R.draws_np(9, 4, 0, 500, V, (thr, alias)), R.draws_np(9, 4, 0, 500, V))
    thr, alias = np.array([1 << 30, 0], np.uint32), np.array([2, 2], np.int64)     # item 1 keeps a quarter of slot 0
    x = R.draws_np(9, 4, 0, 4000, 2, (thr, alias))
    assert [R.draw(9, 4, c, 2, (thr, alias)) for c in range(200)] == x[:200].tolist()
    assert abs((x == 1).mean() - 0.125) < 0.03
    packed = (thr.astype(np.uint64) | (alias.astype(np.uint64) << np.uint64(32))).view(np.int64)
    t2, a2 = R.unpack_table(packed)
    assert np.array_equal(t2, thr) and np.array_equal(a2, alias)


def test_bound_and_fallback():
    """n_neg = V - |seen| with a large V: 4096 raw draws cannot collect every unseen item, the rest is filled
    ascending; a short max_draws shows the same on a small case"""
    V, seen = 40, set(range(1, 11))
    negs, drawn = R.filter_stream(lambda c0, n: R.draws_np(1, 0, c0, n, V), seen, 30, V, max_draws=64)
    assert drawn < 0 and sorted(negs) == list(range(11, 41))
    k = 30 - (-1 - drawn)                                          # kept from the stream, then ascending fill
    assert negs[k:] == sorted(negs[k:]) and len(set(negs)) == 30
    first = []
    for v in R.draws_np(1, 0, 0, 64, V).tolist():
        if v not in seen and v not in first:
            first.append(v)
    assert negs[:k] == first


# ================================================================ planted mistakes
def test_planted_sampler_mistakes_are_rejected(gold):
    z, V, n_neg, seed = gold["z"], gold["V"], gold["n_neg"], gold["seed"]
    window = R.seen_sets(gold["train"], gold["val"], gold["test"], mistake="window_seen", max_len=gold["T"])
    negs, drawn = R.negatives_ref(window, V, n_neg, seed)
    with pytest.raises(AssertionError):
        R.check_negatives(negs, drawn, z["negs"], z["n_drawn"])
    with pytest.raises(AssertionError):
        R.check_properties(negs, gold["seen"], V)
    negs, drawn = R.negatives_ref(gold["seen"], V, n_neg, seed, mistake="keep_repeats")
    with pytest.raises(AssertionError):
        R.check_negatives(negs, drawn, z["negs"], z["n_drawn"])
    with pytest.raises(AssertionError):
        R.check_properties(negs, gold["seen"], V)
    # id 0 drawable: the stream changes, and over many users a 0 shows up
    negs, drawn = R.negatives_ref(gold["seen"], V, n_neg, seed, mistake="zero_drawable")
    with pytest.raises(AssertionError):
        R.check_negatives(negs, drawn, z["negs"], z["n_drawn"])
    with pytest.raises(AssertionError):
        R.check_properties(negs, gold["seen"], V)


@pytest.mark.parametrize("mistake,mode,code", [("test_without_val", "test", "sas"), ("test_without_val", "test", "bert"),
                                               ("truncate_before_mask", "val", "bert"),
                                               ("truncate_before_mask", "test", "bert"),
                                               ("answer_last", "val", "sas"), ("answer_last", "test", "bert")])
def test_planted_row_mistakes_are_rejected(gold, mistake, mode, code):
    z = gold["z"]
    rows = R.rows_ref(gold["train"], gold["val"], gold["test"], z["negs"], gold["T"], mode, code, gold["V"],
                      mistake=mistake)
    want = tuple(z[f"{code}_{mode}/{k}"] for k in ("seq", "cand", "labels"))
    with pytest.raises(AssertionError):
        R.check_batches([rows], [want])


def test_planted_batching_and_averaging_mistakes_are_rejected(gold):
    z = gold["z"]
    want = tuple(z[f"sas_val/{k}"] for k in ("seq", "cand", "labels"))
    with pytest.raises(AssertionError):
        R.check_batches(R.batches_ref(want, 8, mistake="drop_partial"), R.batches_ref(want, 8))
    ms = [{"Recall@10": 0.5, "NDCG@10": 0.25}, {"Recall@10": 0.75, "NDCG@10": 0.5}, {"Recall@10": 1.0, "NDCG@10": 1.0}]
    right = R.average_ref(ms)
    assert right == {"Recall@10": 0.75, "NDCG@10": (0.25 + 0.5 + 1.0) / 3}
    R.check_average(R.average_ref(ms, sizes=[8, 8, 5]), right)
    with pytest.raises(AssertionError):
        R.check_average(R.average_ref(ms, sizes=[8, 8, 5], mistake="weight_by_size"), right)


# ================================================================ the law of the streams
LAW = dict(V=64, N=48_000, n_seen=16, n_neg=8, seed=12345)
CHI2_47_1M1E9 = 130.08          # the 1 - 1e-9 quantile of chi-square at 47 degrees of freedom


def _law_negs(table=None):
    seen = set(range(1, LAW["n_seen"] + 1))
    negs, drawn = R.negatives_ref([seen] * LAW["N"], LAW["V"], LAW["n_neg"], LAW["seed"], table=table)
    assert (drawn > 0).all()
    return negs, drawn


def _chi2(counts, p):
    e = p * counts.sum()
    return float(((counts - e) ** 2 / e).sum())


def test_law_uniform():
    """first slot uniform over the 48 unseen items (chi-square below the 1 - 1e-9 quantile at 47 degrees of freedom:
    measured 39.6, at most 27 raw draws per user); every unseen item's inclusion count within 6 sigma of N 8 / 48,
    sigma^2 = N p (1 - p) (measured maximum 1.63 sigma).  The bounds are conditions fixed before the run, the seed
    (12345) likewise; the GPU runs the same streams bit for bit (tests/test_eval_loader_gpu.py)."""
    V, N, ns, k = LAW["V"], LAW["N"], LAW["n_seen"], LAW["n_neg"]
    negs, drawn = _law_negs()
    first = np.bincount(negs[:, 0], minlength=V + 1)[ns + 1:]
    chi2 = _chi2(first, np.full(V - ns, 1.0 / (V - ns)))
    p = k / (V - ns)
    incl = np.bincount(negs.ravel(), minlength=V + 1)[ns + 1:]
    dev = np.abs(incl - N * p).max() / np.sqrt(N * p * (1 - p))
    print(f"uniform: chi2 {chi2:.1f}, max inclusion deviation {dev:.2f} sigma, max raw draws {drawn.max()}")
    assert first.sum() == N and chi2 < CHI2_47_1M1E9
    assert dev < 6.0


def test_law_popular():
    """w_v = v: the first slot follows Qhat(v) / (1 - Qhat(seen)), Qhat from ItemProposal.counts (the same chi-square
    bound; measured 33.2)"""
    from rbm_amd.dataloaders import ItemProposal
    V, N, ns = LAW["V"], LAW["N"], LAW["n_seen"]
    prop = ItemProposal(np.arange(V + 1, dtype=np.float64), device="cpu")
    q = prop.counts.astype(np.float64) / float(V << 32)            # Qhat(v), v = 1..V
    negs, drawn = _law_negs((prop.thr, prop.alias))
    first = np.bincount(negs[:, 0], minlength=V + 1)[ns + 1:]
    chi2 = _chi2(first, q[ns:] / q[ns:].sum())
    print(f"popular: chi2 {chi2:.1f}, max raw draws {drawn.max()}")
    assert first.sum() == N and chi2 < CHI2_47_1M1E9


# ================================================================ refusals
ARG = 1001
FAKE = 0x10000      # non-NULL, points at nothing: every case below must be refused by host-side validation


def test_c_abi_refuses_bad_arguments_before_any_launch():
    import rbm_amd._lib as L
    lib = L.lib()
    assert lib.rs_eval_negs_max() == R.NEGS_MAX and lib.rs_eval_negatives_max_draws() == R.MAX_DRAWS
    ok = dict(off=FAKE, seen=FAKE, user0=0, count=8, V=100, n_neg=10, seed=1, table=None, negs=FAKE, drawn=None)
    bad = [dict(off=None), dict(seen=None), dict(negs=None), dict(count=0), dict(count=-3), dict(user0=-1),
           dict(V=0), dict(V=1 << 31), dict(n_neg=0), dict(n_neg=R.NEGS_MAX + 1), dict(n_neg=101)]
    for ch in bad:
        a = {**ok, **ch}
        args = (a["off"], a["seen"], a["user0"], a["count"], a["V"], a["n_neg"], a["seed"], a["table"], a["negs"],
                a["drawn"])
        assert lib.rs_eval_negatives(*args, None) == ARG, ch
        assert lib.rs_eval_negatives_draws(*args, FAKE, None) == ARG, ch
    ok = dict(off=FAKE, items=FAKE, extra=None, answer=FAKE, negs=FAKE, user0=0, B=4, T=16, n_neg=10, mask=0,
              seq=FAKE, cand=FAKE, labels=FAKE)
    bad = [dict(off=None), dict(items=None), dict(answer=None), dict(negs=None), dict(seq=None), dict(cand=None),
           dict(labels=None), dict(user0=-1), dict(B=0), dict(B=-4), dict(T=0), dict(T=513), dict(n_neg=0),
           dict(n_neg=R.NEGS_MAX + 1), dict(mask=-1)]
    for ch in bad:
        a = {**ok, **ch}
        assert lib.rs_eval_batch(a["off"], a["items"], a["extra"], a["answer"], a["negs"], a["user0"], a["B"], a["T"],
                                 a["n_neg"], a["mask"], a["seq"], a["cand"], a["labels"], None) == ARG, ch


def test_python_classes_refuse_without_a_device():
    from rbm_amd.dataloaders import DeviceEvalLoader, DeviceEvalNegatives
    train, val, test = [[1, 2, 3], [2, 3, 4, 5]], [[4], [6]], [[5], [7]]
    with pytest.raises(ValueError, match="sampler"):
        DeviceEvalNegatives(train, val, test, 20, n_neg=5, sampler="zipf")
    for n_neg in (0, R.NEGS_MAX + 1):
        with pytest.raises(ValueError, match="n_neg"):
            DeviceEvalNegatives(train, val, test, 5000, n_neg=n_neg)
    with pytest.raises(ValueError, match="loop forever"):                 # user 1 has seen 6 of 10: 4 left
        DeviceEvalNegatives(train, val, test, 10, n_neg=5)
    with pytest.raises(ValueError, match="outside"):
        DeviceEvalNegatives(train, val, test, 6, n_neg=1)
    with pytest.raises(ValueError, match="exactly one"):
        DeviceEvalNegatives(train, [[4], [6, 7]], test, 20, n_neg=5)
    with pytest.raises(ValueError, match="exactly one"):
        DeviceEvalNegatives(train, val, [[5], []], 20, n_neg=5)
    with pytest.raises(ValueError, match="same"):
        DeviceEvalNegatives(train, val[:1], test, 20, n_neg=5)
    with pytest.raises(ValueError, match="strictly positive"):             # items 8..20 never occur: ItemProposal's own
        DeviceEvalNegatives(train, val, test, 20, n_neg=5, sampler="popular")
    with pytest.raises(ValueError):
        DeviceEvalNegatives.from_samples({0: [1, 2], 1: [3]})
    with pytest.raises(ValueError, match="n_neg"):
        DeviceEvalNegatives.from_samples(np.ones((2, R.NEGS_MAX + 1), np.int64))
    with pytest.raises(ValueError, match="outside"):
        DeviceEvalNegatives.from_samples([[1, 0], [2, 3]])
    for kw, pat in ((dict(mode="train"), "mode"), (dict(model_code="gru"), "model_code"), (dict(max_len=0), "max_len"),
                    (dict(max_len=513), "max_len"), (dict(batch_size=0), "batch_size")):
        with pytest.raises(ValueError, match=pat):
            DeviceEvalLoader(train, val, test, 20, **{**dict(batch_size=2, max_len=8, negatives=None), **kw})
    with pytest.raises(ValueError, match="exactly one"):
        DeviceEvalLoader(train, [[4, 5], [6]], test, 20, batch_size=2, max_len=8, negatives=None)
