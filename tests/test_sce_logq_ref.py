"""The logQ-corrected sampled softmax and its alias sampler, on the CPU: the proposal's table, the reference draws, the
reason for the correction, the references' identities, and the emulated kernel arithmetic against the derived bounds
with every planted mistake outside them (tests/sce_logq_ref.py has the definitions and the derivations)."""
import argparse
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bert_sce_ref
import sas_sce_ref
import sce_logq_ref as ref

BF, F32 = torch.bfloat16, torch.float32


def _weights(kind, V):
    if kind == "uniform":
        w = np.full(V, 3.7)
    elif kind == "zipf":
        w = 1.0 / np.arange(1, V + 1)
    else:                                                           # one weight 10^9 times the others
        w = np.ones(V)
        w[V // 2] = 1e9
    return np.concatenate([[0.0], w])


def _proposal(w):
    from rbm_amd.dataloaders import ItemProposal
    return ItemProposal(w, device="cpu")


# ================================================================ the table
@pytest.mark.parametrize("kind", ["uniform", "zipf", "spike"])
@pytest.mark.parametrize("V", [1, 2, 3, 63, 1000])
def test_alias_table(V, kind):
    w = _weights(kind, V)
    P = _proposal(w)
    assert P.item_num == V and P.table.shape == (V,) and P.table.dtype == torch.int64
    thr, alias = ref.unpack_table(P.table.numpy())
    rthr, ralias = ref.alias_table_ref(w)
    assert (thr == rthr).all() and (alias == ralias).all()          # the build is the documented one, bit for bit
    P2 = _proposal(w.copy())
    assert torch.equal(P.table, P2.table) and torch.equal(P.logq.view(torch.int32), P2.logq.view(torch.int32))
    assert alias.min() >= 1 and alias.max() <= V
    n = ref.realised_counts_ref(thr, alias)
    assert sum(n) == V << 32                                        # exactly: Python integers
    assert min(n) >= 1
    q = w[1:] / math.fsum(w[1:].tolist())
    qhat = ref.realised_q_ref(P.table.numpy())
    assert qhat[0] == 0 and (qhat == P.q).all()
    bound, indeg = ref.table_bound(w, alias)
    err = np.abs(qhat[1:] - q)
    print((V, kind), "worst |Qhat - Q| / bound", float((err / bound).max()), "largest indegree", int(indeg.max()))
    assert (err <= bound).all()
    # logq = log Qhat to fp32 rounding (2^-24 relative, of a float64 logarithm whose own error is far below that)
    D = V << 32                                                     # Python integers: x / D is correctly rounded
    want = np.array([math.log1p(-((D - x) / D)) if 2 * x > D else math.log(x / D) for x in n])
    got = P.logq.numpy().astype(np.float64)
    assert got[0] == 0.0 and P.logq.dtype == torch.float32 and P.logq.shape == (V + 1,)
    assert (np.abs(got[1:] - want) <= 2.0 ** -24 * np.abs(want)).all()
    if kind == "uniform":
        assert (alias == np.arange(1, V + 1)).all()                 # every slot keeps its whole mass
        assert (np.array(n) == 1 << 32).all()


def test_bad_weights_raise():
    from rbm_amd.dataloaders import ItemProposal
    good = np.array([0.0, 1.0, 2.0, 3.0])
    ItemProposal(good, device="cpu")
    ItemProposal(np.array([np.nan, 1.0, 2.0, 3.0]), device="cpu")    # entry 0 is ignored
    for bad in (np.array([0.0, 1.0, 0.0, 3.0]), np.array([0.0, 1.0, -2.0, 3.0]), np.array([0.0, 1.0, np.nan, 3.0]),
                np.array([0.0, 1.0, np.inf, 3.0]), np.array([0.0]), np.zeros((2, 3))):
        with pytest.raises(ValueError):
            ItemProposal(bad, device="cpu")


def test_samplers_check_the_proposal_before_touching_a_device():
    from rbm_amd.dataloaders import DeviceBertMasker, DeviceWarpSampler
    P = _proposal(_weights("zipf", 20))
    hist = [[1, 2, 3], [4, 5]]
    for make in (lambda **kw: DeviceWarpSampler(hist, 20, 2, 4, device="cpu", **kw),
                 lambda **kw: DeviceBertMasker(hist, 20, 2, 4, 0.2, device="cpu", **kw)):
        with pytest.raises(ValueError, match="shared_negs"):
            make(proposal=P)
        s = make(shared_negs=8, proposal=P)
        assert s.proposal is P and make(shared_negs=8).proposal is None
    with pytest.raises(ValueError, match="item_num"):
        DeviceWarpSampler(hist, 21, 2, 4, device="cpu", shared_negs=8, proposal=P)
    with pytest.raises(ValueError, match="item_num"):
        DeviceBertMasker(hist, 19, 2, 4, 0.2, device="cpu", shared_negs=8, proposal=P)


def test_from_histories_counts():
    from rbm_amd.dataloaders import ItemProposal
    hist = [[1, 2, 2, 5], [5, 5], [2]]                              # item 1: 1, 2: 3, 3: 0, 4: 0, 5: 3
    P = ItemProposal.from_histories(hist, 5, device="cpu")
    assert (P.weights == np.array([0, 2, 4, 1, 1, 4.0])).all()
    P = ItemProposal.from_histories(hist, 5, alpha=0.5, smooth=0.25, device="cpu")
    assert np.allclose(P.weights[1:], np.sqrt(np.array([1.25, 3.25, 0.25, 0.25, 3.25])), rtol=1e-15)
    P = ItemProposal.from_histories(hist, 5, alpha=0.0, device="cpu")
    assert (ref.unpack_table(P.table.numpy())[1] == np.arange(1, 6)).all()      # alpha = 0: uniform
    with pytest.raises(ValueError):
        ItemProposal.from_histories([[1, 6]], 5, device="cpu")
    with pytest.raises(ValueError):
        ItemProposal.from_histories(hist, 5, smooth=0.0, device="cpu")           # items 3 and 4 would have Q = 0


# ================================================================ the draws
@pytest.mark.parametrize("V,K", [(1, 5), (2, 300), (63, 4096), (1000, 5000), (54542, 257)])
def test_uniform_table_gives_the_uniform_draws(V, K):
    P = _proposal(_weights("uniform", V))
    for seed_base, salt in ((1, 1234), (7, 2 ** 61 + 5)):
        a = ref.alias_items_ref(seed_base, salt, P.table.numpy(), V, K)
        assert (a == ref.uniform_items_ref(seed_base, salt, V, K)).all()


def test_both_spellings_of_the_draw_rule_agree():
    P = _proposal(_weights("zipf", 63))
    a = ref.alias_items_ref(3, 99, P.table.numpy(), 63, 5000)       # wrapping uint64 arithmetic
    b = ref.alias_items_ref(3, 99, P.table.numpy(), 63, 4096)       # Python integers
    assert (a[:4096] == b).all() and a.min() >= 1 and a.max() <= 63


# the 1 - 10^-6 quantile of the chi-square distribution with 63 degrees of freedom
CHI2_63_Q = 131.3697
CHI2_SEED = (1, 20261020)          # (step seed, salt) of the draws below


def test_reference_draws_follow_the_realised_distribution():
    """2^20 draws at V = 64, Zipf s = 1, against Qhat: a fixed function of the seed, so the statistic is one number
    (68.20 with CHI2_SEED; the mean of chi-square(63) is 63)."""
    V, n = 64, 1 << 20
    P = _proposal(_weights("zipf", V))
    a = ref.alias_items_ref(CHI2_SEED[0], CHI2_SEED[1], P.table.numpy(), V, n)
    obs = np.bincount(a, minlength=V + 1)[1:]
    exp = n * P.q[1:]
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    print("chi-square", chi2)
    assert chi2 < CHI2_63_Q
    assert abs(chi2 - 68.20) < 0.005                                  # the value, pinned


# ================================================================ the reason for the feature
def test_the_correction_brings_the_sampled_gradient_to_the_full_softmax_gradient():
    """V = 200, d = 16, 32 rows, a Zipf s = 1 proposal, K = 512, the mean over 200 draws of the gradient with respect
    to the features against the full cross-entropy gradient (every item a candidate, no correction): the corrected
    mean is at least four times nearer than the uncorrected one on the same draws.  Features of unit variance against
    a table of variance 1 / d: logits of unit variance, the scale of the head problems on the GPU.  (0.011 against
    0.190 here; with logits four times as wide the sampled estimate's own variance at K = 512 dominates both.)"""
    V, d, rows, K, draws = 200, 16, 32, 512, 200
    rng = np.random.default_rng(0)
    hl, E = rng.standard_normal((rows, d)), rng.standard_normal((V + 1, d)) / math.sqrt(d)
    lab = rng.integers(1, V + 1, rows)
    P = _proposal(_weights("zipf", V))
    logq = P.logq.numpy().astype(np.float64)
    full = ref.head_bwd_ref(hl, lab, rows, E, None, None, np.arange(1, V + 1), float(rows))[0]
    g_c, g_u = np.zeros_like(full), np.zeros_like(full)
    for i in range(draws):
        cand = ref.alias_items_ref(i + 1, 4242, P.table.numpy(), V, K)
        g_c += ref.head_bwd_ref(hl, lab, rows, E, None, logq, cand, float(rows))[0]
        g_u += ref.head_bwd_ref(hl, lab, rows, E, None, None, cand, float(rows))[0]
    e_c = np.linalg.norm(g_c / draws - full) / np.linalg.norm(full)
    e_u = np.linalg.norm(g_u / draws - full) / np.linalg.norm(full)
    print("relative error of the mean gradient: corrected", e_c, "uncorrected", e_u)
    assert e_c <= e_u / 4


# ================================================================ identities in float64
def _small_head(seed=0, cap=40, count=33, d=24, V=50, K=70):
    rng = np.random.default_rng(seed)
    hl, E = rng.standard_normal((cap, d)) * 0.3, rng.standard_normal((V + 1, d)) * 0.3
    bias = rng.standard_normal(V + 1)
    lab, cand = rng.integers(1, V + 1, cap), rng.integers(0, V + 1, K)
    logq = np.concatenate([[0.0], np.log(rng.dirichlet(np.ones(V)))])
    return hl, E, bias, lab, cand, logq, cap, count, V, K


@pytest.mark.parametrize("with_bias", [False, True])
def test_a_constant_logq_changes_nothing(with_bias):
    hl, E, bias, lab, cand, logq, cap, count, V, K = _small_head()
    b = bias if with_bias else None
    const = np.full(V + 1, -3.25)
    got_f = ref.head_fwd_ref(hl, lab, count, E, b, const, cand, float(count))
    want_f = bert_sce_ref.head_fwd_ref(hl, lab, count, E, b, cand, float(count))
    assert np.abs(got_f[0] - 3.25 - want_f[0]).max() < 1e-12         # lse and z0 both move by the constant
    assert np.abs(got_f[1] - 3.25 - want_f[1]).max() < 1e-12
    assert abs(got_f[2][2] - want_f[2][2]) < 1e-12 and got_f[2][1] == want_f[2][1]
    got = ref.head_bwd_ref(hl, lab, count, E, b, const, cand, float(count), 0.75)
    want = bert_sce_ref.head_bwd_ref(hl, lab, count, E, b, cand, float(count), 0.75)
    for g, w in zip(got[:5], want[:5]):
        assert np.abs(g - w).max() < 1e-12
    assert (got[5] == want[5]).all()


def test_a_constant_logq_changes_nothing_in_the_models():
    import test_bert_sce_ref as tb
    import test_sas_ce_ref as ts
    rng = np.random.default_rng(1)
    V, T, d, L, h, B, K = 30, 8, 16, 1, 2, 3, 12
    const = np.full(V + 1, 1.75)
    cand = rng.integers(0, V + 1, K)
    P = ts.params(V, T, d, L, h)
    seq, pos = ts.batch(rng, B, T, V)
    l0, g0 = sas_sce_ref.sce_loss_and_grads(P, seq, pos, cand, L, h)
    l1, g1 = ref.loss_and_grads(ref.sas_sce_loss, P, seq, pos, cand, const, L, h)
    assert abs(l0.item() - l1.item()) < 1e-12
    assert all(float((g0[k] - g1[k]).abs().max()) < 1e-12 for k in g0)
    P = tb.params(V, T, d, L, h)
    tok, lab = tb.batch(rng, B, T, V)
    l0, g0 = bert_sce_ref.sce_loss_and_grads(P, tok, lab, cand, L, h)
    l1, g1 = ref.loss_and_grads(ref.bert_sce_loss, P, tok, lab, cand, const, L, h)
    assert abs(l0.item() - l1.item()) < 1e-12
    assert all(float((g0[k] - g1[k]).abs().max()) < 1e-12 for k in g0)


@pytest.mark.parametrize("with_bias", [False, True])
def test_every_item_as_candidate_is_cross_entropy_over_the_corrected_logits(with_bias):
    hl, E, bias, lab, _, logq, cap, count, V, K = _small_head(seed=3)
    b = bias if with_bias else np.zeros(V + 1)
    cand = np.arange(1, V + 1)
    lse, z0, out = ref.head_fwd_ref(hl, lab, count, E, b if with_bias else None, logq, cand, float(count))
    ht = torch.from_numpy(hl[:count]).requires_grad_(True)
    Et = torch.from_numpy(E).requires_grad_(True)
    bt = torch.from_numpy(b).requires_grad_(True)
    logits = ht @ Et.T + bt - torch.from_numpy(logq)                 # (count, V + 1); class 0 is left out below
    loss = F.cross_entropy(logits[:, 1:], torch.from_numpy(lab[:count]) - 1)
    assert abs(out[2] - loss.item()) < 1e-12
    loss.backward()
    dh, coef, pg, dEc, dbc, keys, _ = ref.head_bwd_ref(hl, lab, count, E, b if with_bias else None, logq, cand,
                                                       float(count))
    assert np.abs(dh - ht.grad.numpy()).max() < 1e-13
    dE = np.zeros_like(E)
    np.add.at(dE, keys[:count], pg)
    np.add.at(dE, keys[cap:], dEc)
    assert np.abs(dE - Et.grad.numpy()).max() < 1e-13
    if with_bias:
        db = bert_sce_ref.scatter_bias_grad(V + 1, cap, keys, coef, dbc)
        assert np.abs(db - bt.grad.numpy()).max() < 1e-13


def test_model_references_reduce_to_the_head_reference():
    """sas_sce_loss / bert_sce_loss are the uncorrected model references with the corrected head in place."""
    rng = np.random.default_rng(5)
    n, d, V, K = 14, 8, 20, 9
    h = torch.from_numpy(rng.standard_normal((1, n, d)))
    W, b = torch.from_numpy(rng.standard_normal((V + 1, d))), torch.from_numpy(rng.standard_normal(V + 1))
    lab = rng.integers(0, V + 1, n)
    cand = rng.integers(0, V + 1, K)
    logq = np.concatenate([[7.0], np.log(rng.dirichlet(np.ones(V)))])    # entry 0: whatever, never read
    q = torch.from_numpy(logq).clone()
    q[0] = 0
    got = bert_sce_ref.sce_from_hidden(h, W, b - q, lab[None], cand)
    _, _, out = ref.head_fwd_ref(h[0].numpy(), lab, n, W.numpy(), b.numpy(), logq, cand, float(max((lab != 0).sum(), 1)))
    assert abs(got.item() - out[2]) < 1e-12


# ================================================================ the emulated kernels and the planted mistakes
def _ks(cap, K, d, dt):
    from rbm_amd import ops
    return ops.sce_head_dh_splits(cap, K, d, dt)


def _emu_case(dt, d, rows, K, pattern, kind, with_bias, mut=None, count=None):
    V, cap, hl, E, bias, logq, lab, cand = ref.head_problem(dt, d, rows, K, pattern, kind, seed=d + rows + K)
    count = rows if count is None else count
    b = bias.numpy() if with_bias else None
    nvalid = int(((lab[:count] > 0) & (lab[:count] <= V)).sum())
    dv = float(max(nvalid, 1))
    hl64, E64 = hl.double().numpy(), E.double().numpy()
    bars = ref.head_bars(dt, _ks(cap, K, d, dt), hl64, lab, count, E64, b, logq.numpy(), cand, dv, 0.75)
    got = ref.emu_head(dt, hl64, lab, count, E64, b, logq.numpy(), cand, dv, 0.75, mut=mut)
    z_id0 = hl64[:count] @ E64[0] + (float(b[0]) if with_bias else 0.0) - 1.5     # emu_head's planted class
    with np.errstate(divide="ignore", invalid="ignore"):
        shift = np.exp(z_id0 - bars["lse"][0]) / bars["lse"][1]      # that class' weight in units of lse's bar
    return ref.worst(got, bars), (lab[:count], cand, V, shift)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("dt,d", ref.HEAD_WIDTHS)
def test_emulated_kernels_stay_inside_the_bounds(dt, d, with_bias):
    top = {}
    for rows, K, pattern, kind in ref.head_cases():
        res, _ = _emu_case(dt, d, rows, K, pattern, kind, with_bias)
        bad = {k: v for k, v in res.items() if v > 1.0}
        assert not bad, (rows, K, pattern, kind, bad)
        for k, v in res.items():
            top[k] = max(top.get(k, 0.0), v)
    res, _ = _emu_case(dt, d, 17, 65, "mixed", "zipf", with_bias, count=0)
    assert not any(res.values()), res
    print((dt, d, with_bias), "worst err / bar", {k: round(v, 3) for k, v in top.items()})


def _exercised(mut, lab, cand, V, p_id0):
    """Does the problem hold what the mistake needs to show?  An id-0 slot made live is one more class of logit ~ -1,
    and moves a row's lse by its weight p (log1p(n p) for n such slots).  Where a corrected logit of 40 or 100 carries
    the row's whole softmax (the deep table, the big pattern) p is exp(-40) and less, below every rounding.  The
    mistake is held to show wherever n p is past 4 bars of lse in some row: the emulation's own error is within one
    bar, so the mistaken lse is then at least 3 bars from the reference."""
    ok_l = (lab > 0) & (lab <= V)
    cc = np.where((cand <= 0) | (cand > V), 0, cand)
    live = (cc != 0)[None, :] & (cc[None, :] != lab[:, None]) & ok_l[:, None]
    if mut == "zero_live":
        return bool((cc == 0).any() and ((cc == 0).sum() * p_id0[ok_l] > 4.0).any())
    if mut == "slot":
        return bool(live.any() and (cc[cc != 0] != np.nonzero(cc)[0]).any())
    return bool(live.any())


# the outputs a mistake must push past its bar: the forward's (lse or z0) for the four that change the loss; dEc for
# the one that leaves the forward alone
MUTATIONS = {"plus": ("lse",), "pos": ("z0",), "slot": ("lse",), "zero_live": ("lse",), "dec": ("dEc",)}


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("mut", sorted(MUTATIONS))
def test_planted_mistakes_fall_outside_the_bounds(mut, with_bias):
    """At the GPU tests' shapes (fp32 at d = 50, bf16 at d = 128 and the plain kernel's d = 136), wherever the problem
    exercises the mistake: at least 10 of each width's 20 (3 for the id-0 class, which the deep table and the big pattern hide)."""
    for dt, d in ((F32, 50), (BF, 128), (F32, 136)):
        seen = 0
        for rows, K, pattern, kind in ref.head_cases():
            res, (lab, cand, V, p_id0) = _emu_case(dt, d, rows, K, pattern, kind, with_bias, mut=mut)
            if not _exercised(mut, lab, cand, V, p_id0):
                continue
            seen += 1
            assert any(res[k] > 1.0 for k in MUTATIONS[mut]), (mut, dt, d, rows, K, pattern, kind, res)
        assert seen >= (3 if mut == "zero_live" else 10), (mut, dt, d, seen)


# ================================================================ the arguments
def _sas_args(**kw):
    return argparse.Namespace(model_code="sas", num_items=30, max_len=8, device="cpu", sas_hidden_units=16,
                              sas_num_blocks=1, sas_heads=2, sas_dropout=0.0, model_init_seed=0, **kw)


def _bert_args(**kw):
    return argparse.Namespace(model_code="bert", num_items=30, max_len=8, device="cpu", bert_hidden_units=16,
                              bert_num_blocks=1, bert_num_heads=2, bert_dropout=0.0, bert_hidden_dropout=0.0,
                              bert_mask_prob=0.2, model_init_seed=0, **kw)


def test_models_read_and_validate_the_proposal_arguments():
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    m = model_factory(_sas_args())
    assert m.sas.sas_neg_dist == "uniform" and m.sas.sas_neg_alpha == 1.0
    m = model_factory(_sas_args(sas_loss="sampled_ce", sas_shared_negs=8, sas_neg_dist="popular", sas_neg_alpha=0.75))
    assert m.sas.sas_neg_dist == "popular" and m.sas.sas_neg_alpha == 0.75
    with pytest.raises(ValueError, match="sas_neg_dist"):
        model_factory(_sas_args(sas_loss="sampled_ce", sas_shared_negs=8, sas_neg_dist="zipf"))
    with pytest.raises(ValueError, match="sampled_ce"):
        model_factory(_sas_args(sas_neg_dist="popular"))
    m = model_factory(_bert_args())
    assert m.bert.bert_neg_dist == "uniform" and m.bert.bert_neg_alpha == 1.0
    m = model_factory(_bert_args(bert_loss="sampled_ce", bert_shared_negs=8, bert_neg_dist="popular"))
    assert m.bert.bert_neg_dist == "popular" and m.bert.bert_neg_alpha == 1.0
    with pytest.raises(ValueError, match="bert_neg_dist"):
        model_factory(_bert_args(bert_loss="sampled_ce", bert_shared_negs=8, bert_neg_dist="log"))
    with pytest.raises(ValueError, match="sampled_ce"):
        model_factory(_bert_args(bert_neg_dist="popular"))


def test_entries_reject_bad_arguments_before_any_launch():
    import rbm_amd._lib as L
    lib = L.lib()
    assert lib.rs_alias_items(None, 0, 8, 0, 4, 8, None) == 1001      # item_num < 1
    assert lib.rs_alias_items(None, 0, 8, 5, 0, 8, None) == 1001      # K < 1
    assert lib.rs_alias_items(None, 0, None, 5, 4, 8, None) == 1001   # no table
    assert lib.rs_alias_items(None, 0, 8, 5, 4, None, None) == 1001   # no output
    assert lib.rs_alias_items(None, 0, 8, 1 << 32, 4, 8, None) == 1001
    # the head entries keep the checks of rs_sce_head_*: a bias without dbc, an unsupported width
    a = lib.rs_sce_head_logq_bwd(L.F32, 8, 64, 8, 64, 8, None, 8, 8, 8, 20, 8, 4, 8, None, 16, 8, 8, 8, 8, None, None,
                                 None)
    assert a == 1001
    assert lib.rs_sce_head_logq_fwd(L.BF16, 8, 50, 8, 64, 8, None, 8, None, 8, 20, 8, 4, 8, 16, 8, None) == 1002
    assert lib.rs_sce_head_logq_fwd(L.F32, 8, 64, 8, 64, 8, None, 8, None, 8, 20, 8, 0, 8, 16, 8, None) == 1002
