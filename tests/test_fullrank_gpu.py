"""Full-catalogue ranking and top-K (rs_full_rank / rs_full_topk / rs_rank_to_metrics, fullrank.hip).

Kernel tests are EXACT: h and E hold integers in [-3, 3] and the bias multiples of 0.25 in [-2, 2], so every score is
exact in bf16 storage and in fp32 accumulation whatever the summation order, and a CPU reference (scores, then a
stable sort: score descending, id ascending) is the truth with no tolerance.  The small value set makes ties frequent,
which exercises the order rule.  Model tests use real-valued weights; there the ranks are bracketed by the derived
dot-product error bound of the two summation orders (and the bracket is asserted tight on at least 90 % of rows).
"""
import argparse

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
TD = {"fp32": torch.float32, "bf16": torch.bfloat16}


# ------------------------------------------------------------------------------------------- exact kernel tests
def _ints(rng, shape):
    return rng.integers(-3, 4, size=shape).astype(np.float32)


def _bias(rng, n):
    return (rng.integers(-8, 9, size=n) * 0.25).astype(np.float32)


def _scores(h, E, bias, lo, hi):
    S = h @ E[lo:hi].T                       # fp32 on integers: exact in any order
    return S + bias[lo:hi] if bias is not None else S


def _ref(S, lo, target, excl, K):
    """(rank, top-K ids, top-K scores) of the definition, from exact scores S (B, hi - lo)."""
    B, n = S.shape
    ids = np.arange(lo, lo + n)
    rank = np.full(B, -1, np.int64)
    tid = np.full((B, max(K, 1)), -1, np.int64)
    tsc = np.full((B, max(K, 1)), -np.inf, np.float32)
    for b in range(B):
        adm = np.ones(n, bool)
        if excl is not None:
            e = excl[b]
            adm[e[(e >= lo) & (e < lo + n)] - lo] = False
        if target is not None:
            t = int(target[b])
            st = S[b, t - lo]
            before = (S[b] > st) | ((S[b] == st) & (ids < t))
            rank[b] = int((adm & (ids != t) & before).sum())
        if K:
            cand = np.flatnonzero(adm)
            if cand.size > K:                # (only to keep the sort small at 1M items)
                kth = np.partition(S[b, cand], cand.size - K)[cand.size - K]
                cand = cand[S[b, cand] >= kth]
            o = cand[np.lexsort((cand, -S[b, cand]))][:K]      # stable: score descending, then id ascending
            tid[b, :o.size] = ids[o]
            tsc[b, :o.size] = S[b, o]
    return rank, tid, tsc


def _gpu(dtype, h, E, bias, lo, hi, target, excl, K, ldh=None):
    from rbm_amd import ops
    td = TD[dtype]
    B, d = h.shape
    hd = torch.from_numpy(h).cuda().to(td)
    if ldh:
        buf = torch.full((B, ldh), 7.0, dtype=td, device="cuda")      # a read past d would change every score
        buf[:, :d] = hd
        hd = buf[:, :d]
    Ed = torch.from_numpy(E).cuda().to(td)
    bd = torch.from_numpy(bias).cuda() if bias is not None else None
    ex = torch.from_numpy(excl).cuda() if excl is not None else None
    rank = None
    if target is not None:
        rank = ops.full_rank(hd, Ed, torch.from_numpy(target).cuda(), bias=bd, lo=lo, hi=hi, exclude=ex).cpu().numpy()
    ids = sc = None
    if K:
        ids, sc = ops.full_topk(hd, Ed, K, bias=bd, lo=lo, hi=hi, exclude=ex)
        ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
    return rank, ids, sc


def _excl_lists(rng, S, lo, hi, target):
    """Per row: zeros, ids outside the range on both sides, a duplicated id, the target itself (must stay), the item
    that would otherwise rank first, and a few random ids."""
    B, n = S.shape
    best = lo + np.argmax(S, axis=1)                 # first maximum = lowest id among the best
    dup = rng.integers(lo, hi, size=B)
    rnd = rng.integers(lo, hi, size=(B, 3))
    cols = [np.zeros(B, np.int64), np.zeros(B, np.int64), np.full(B, hi + 3), np.full(B, -2), np.full(B, hi), dup, dup,
            target, best, rnd[:, 0], rnd[:, 1], rnd[:, 2]]
    ex = np.stack(cols, axis=1).astype(np.int64)
    return ex[:, rng.permutation(ex.shape[1])]


def _check(dtype, rng, B, n, d, K, lo=1, tail=0, ldh=None, with_bias=True, with_excl=True, E=None):
    V1 = lo + n + tail                               # rows of the table; the range is [lo, lo + n)
    hi = lo + n
    h = _ints(rng, (B, d))
    E = _ints(rng, (V1, d)) if E is None else E
    bias = _bias(rng, V1) if with_bias else None
    S = _scores(h, E, bias, lo, hi)
    target = rng.integers(lo, hi, size=B)
    excl = _excl_lists(rng, S, lo, hi, target) if with_excl else None
    want = _ref(S, lo, target, excl, K)
    got = _gpu(dtype, h, E, bias, lo, hi if tail else None, target, excl, K, ldh)
    tag = (dtype, B, n, d, K, lo, tail, ldh)
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"rank {tag}")
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"ids {tag}")
    np.testing.assert_array_equal(got[2], want[2], err_msg=f"scores {tag}")
    return got, target


@pytest.mark.parametrize("d", [50, 64, 128, 256])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_rank_and_topk_equal_the_cpu_reference(dtype, d):
    """B in {1, 17, 130} (a partial row tile, a second row tile) x range sizes {1, 5, 255, 257, 1000} (below, across
    and beyond one 128-item tile; 1000: eight slices) x K in {1, 10, 128} (K > |A(b)| included: tail -1 / -inf),
    with a bias and exclusion lists holding zeros, out-of-range ids, duplicates, the target and the best item."""
    rng = np.random.default_rng(1000 + d)
    for B in (1, 17, 130):
        for n in (1, 5, 255, 257, 1000):
            for K in (1, 10, 128):
                _check(dtype, rng, B, n, d, K)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_row_pitch_and_sub_range(dtype):
    """ldh > d (16-byte-loadable and not), and a sub-range v_lo > 1, v_hi < V of a larger table."""
    rng = np.random.default_rng(7)
    for d, ldh in ((64, 72), (64, 67), (50, 61), (128, 4 * 128)):
        _check(dtype, rng, 17, 300, d, 10, ldh=ldh)
    for d in (50, 128):
        _check(dtype, rng, 130, 333, d, 10, lo=37, tail=20)
        _check(dtype, rng, 5, 100, d, 128, lo=129, tail=1, with_bias=False)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_all_zero_table_orders_by_id(dtype):
    rng = np.random.default_rng(11)
    B, n, d, K = 17, 300, 64, 10
    (rank, ids, sc), target = _check(dtype, rng, B, n, d, K, with_bias=False, E=np.zeros((n + 1, d), np.float32))
    assert (sc == 0).all() and (np.diff(ids, axis=1) > 0).all()
    (rank, ids, _), target = _check(dtype, rng, B, n, d, K, with_bias=False, with_excl=False,
                                    E=np.zeros((n + 1, d), np.float32))
    np.testing.assert_array_equal(ids, np.tile(np.arange(1, K + 1), (B, 1)))
    np.testing.assert_array_equal(rank, target - 1)


@pytest.mark.parametrize("d", [50, 128])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_identical_rows_in_different_tiles_tie_exactly(dtype, d):
    """REAL-valued weights: the table is seven distinct rows (and biases) repeated over 1000 ids, so equal items sit
    in different vocabulary tiles, lanes and slices.  Equal rows must score bit-identically -- the target's own score
    included -- so the order is: groups by score, then ids ascending; any id's rank follows from group sizes."""
    from rbm_amd import ops
    rng = np.random.default_rng(5)
    B, n, G, K = 17, 1000, 7, 128
    td = TD[dtype]
    base = torch.from_numpy(rng.standard_normal((G, d)).astype(np.float32)).to(td)
    bb = rng.standard_normal(G).astype(np.float32)
    h = torch.from_numpy(rng.standard_normal((B, d)).astype(np.float32)).to(td)
    grp = np.arange(n + 1) % G
    E = base[torch.from_numpy(grp)].cuda()
    bias = torch.from_numpy(bb[grp]).cuda()
    gs = h.double() @ base.double().T + torch.from_numpy(bb).double()          # (B, G) group scores, fp64
    gs = gs.numpy()
    gap = np.abs(gs[:, :, None] - gs[:, None, :])[:, ~np.eye(G, dtype=bool)].min()
    assert gap > 1e-3, gap                           # groups are far apart against fp32 / bf16-product rounding
    ids_all = np.arange(1, n + 1)
    target = rng.integers(1, n + 1, size=B)
    rank, ts = ops.full_rank(h.cuda(), E, torch.from_numpy(target).cuda(), bias=bias, return_scores=True)
    ids, sc = ops.full_topk(h.cuda(), E, K, bias=bias)
    rank, ts, ids, sc = (x.cpu().numpy() for x in (rank, ts, ids, sc))
    for b in range(B):
        order = np.lexsort((ids_all, -gs[b, grp[1:]]))          # group score descending, id ascending
        want = ids_all[order]
        np.testing.assert_array_equal(ids[b], want[:K])
        assert rank[b] == int(np.flatnonzero(want == target[b])[0])
        assert len(set(sc[b].tolist())) == len(set(grp[want[:K]].tolist()))    # one bit pattern per group
        same = grp[ids[b]] == grp[target[b]]
        assert not same.any() or (sc[b][same] == ts[b]).all()                  # the target's score is the sweep's


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_no_exclusion_equals_an_all_zero_list_and_rank_indexes_topk(dtype):
    rng = np.random.default_rng(13)
    B, n, d, K = 130, 700, 64, 128
    h, E, bias = _ints(rng, (B, d)), _ints(rng, (n + 1, d)), _bias(rng, n + 1)
    target = rng.integers(1, n + 1, size=B)
    a = _gpu(dtype, h, E, bias, 1, None, target, None, K)
    z = _gpu(dtype, h, E, bias, 1, None, target, np.zeros((B, 6), np.int64), K)
    for x, y in zip(a, z):
        np.testing.assert_array_equal(x, y)
    # consistency (exclusions that do not hold the target): rank < K  =>  ids[b][rank[b]] == target[b]
    excl = rng.integers(1, n + 1, size=(B, 20))
    excl[excl == target[:, None]] = 0
    rank, ids, _ = _gpu(dtype, h, E, bias, 1, None, target, excl, K)
    hit = rank < K
    assert hit.sum() > B // 8
    np.testing.assert_array_equal(ids[hit, rank[hit]], target[hit])
    assert not (ids[~hit] == target[~hit, None]).any()


def test_rank_to_metrics_matches_the_formulas():
    from rbm_amd import ops
    rng = np.random.default_rng(3)
    rank = rng.integers(0, 40, size=1000).astype(np.int32)
    rank[::17] = -1                                   # targets outside the range: misses
    rank[5] = 0
    ks = np.array([20, 10, 5, 1], np.int32)
    out = torch.empty(3 * len(ks), dtype=torch.float32, device="cuda")
    ws = torch.empty(3 * len(ks) * rank.size, dtype=torch.float32, device="cuda")
    ops.rank_to_metrics(torch.from_numpy(rank).cuda(), torch.from_numpy(ks).cuda(), ws, out)
    out = out.cpu().numpy().astype(np.float64)
    r = rank.astype(np.float64)
    for q, k in enumerate(ks):
        hit = (rank >= 0) & (rank < k)
        want = [hit.mean(), np.where(hit, 1.0 / np.log2(np.where(hit, r, 0) + 2.0), 0.0).mean(),
                np.where(hit, 1.0 / (np.where(hit, r, 0) + 1.0), 0.0).mean()]
        np.testing.assert_allclose(out[3 * q:3 * q + 3], want, rtol=0, atol=1e-6)


def test_bad_arguments():
    from rbm_amd import _lib, ops
    h = torch.zeros((4, 64), dtype=torch.bfloat16, device="cuda")
    E = torch.zeros((100, 64), dtype=torch.bfloat16, device="cuda")
    for t in (0, 100):
        with pytest.raises(IndexError):
            ops.full_rank(h, E, torch.tensor([1, 2, t, 3], device="cuda"))
    with pytest.raises(RuntimeError, match="1002"):                       # d > 256: RS_ERR_UNSUPPORTED
        ops.full_topk(torch.zeros((4, 264), device="cuda"), torch.zeros((100, 264), device="cuda"), 5)
    # the C call itself: a target outside [v_lo, v_hi) ranks -1 (and the other rows are unaffected)
    tgt = torch.tensor([1, 99, 0, 100], device="cuda")
    rank = torch.empty(4, dtype=torch.int32, device="cuda")
    ws = ops.full_ws(h, 1, 100, 0)
    _lib.call("rs_full_rank", _lib.BF16, h.data_ptr(), 64, 4, 64, E.data_ptr(), 64, None, 1, 100, tgt.data_ptr(), None,
              0, 0, ws.data_ptr(), rank.data_ptr(), None, _lib.stream())
    assert rank.tolist() == [0, 98, -1, -1]


def test_one_million_items_without_a_score_matrix():
    """V = 1,000,001 rows, d = 64, B = 64, K = 10, bf16, integer inputs (so ties are everywhere): results equal the
    CPU reference, and the peak allocation stays under one eighth of a B x V fp32 score matrix."""
    from rbm_amd import ops
    rng = np.random.default_rng(99)
    V1, d, B, K = 1_000_001, 64, 64, 10
    h, E, bias = _ints(rng, (B, d)), _ints(rng, (V1, d)), _bias(rng, V1)
    target = rng.integers(1, V1, size=B)
    excl = rng.integers(0, V1 + 5, size=(B, 8))
    excl[:, 0] = 0
    S = _scores(h, E, bias, 1, V1)
    excl[:, 1] = 1 + np.argmax(S, axis=1)
    want = _ref(S, 1, target, excl, K)
    hd, Ed = torch.from_numpy(h).cuda().bfloat16(), torch.from_numpy(E).cuda().bfloat16()
    bd, td, ex = torch.from_numpy(bias).cuda(), torch.from_numpy(target).cuda(), torch.from_numpy(excl).cuda()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    rank = ops.full_rank(hd, Ed, td, bias=bd, exclude=ex)
    ids, sc = ops.full_topk(hd, Ed, K, bias=bd, exclude=ex)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < B * V1 * 4 // 8, peak
    np.testing.assert_array_equal(rank.cpu().numpy(), want[0])
    np.testing.assert_array_equal(ids.cpu().numpy(), want[1])
    np.testing.assert_array_equal(sc.cpu().numpy(), want[2])


def test_topk_replays_in_a_captured_graph():
    from rbm_amd import ops
    rng = np.random.default_rng(21)
    B, n, d, K = 17, 700, 64, 10
    E = torch.from_numpy(_ints(rng, (n + 1, d))).cuda().bfloat16()
    h0, h1 = (torch.from_numpy(_ints(rng, (B, d))).cuda().bfloat16() for _ in range(2))
    h = h0.clone()
    ops.full_topk(h, E, K)                            # first use outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ids, sc = ops.full_topk(h, E, K)
    h.copy_(h1)
    g.replay()
    torch.cuda.synchronize()
    ids1, sc1 = ops.full_topk(h1, E, K)
    assert torch.equal(ids, ids1) and torch.equal(sc, sc1)
    ids0, _ = ops.full_topk(h0, E, K)
    assert not torch.equal(ids0, ids1)


# ------------------------------------------------------------------------------------------------- model level
def _sas_trained(dtype):
    from rbm_amd.models import model_factory
    z = load_golden("sas_curve")
    V, T, d, L, hd = (int(z[k]) for k in ("V", "T", "d", "L", "h"))
    a = argparse.Namespace(model_code="sas", num_items=V, max_len=T, device="cuda", sas_hidden_units=d,
                           sas_num_blocks=L, sas_heads=hd, sas_dropout=0.0, l2_emb=0.0, rs_dtype=dtype)
    m = model_factory(a)
    m.load_state_dict({k[6:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("final/")})
    return m, V, T, 64, 123


def _sas_random(dtype):
    from rbm_amd.models import model_factory
    torch.manual_seed(5)
    V, T, d = 777, 20, 50
    a = argparse.Namespace(model_code="sas", num_items=V, max_len=T, device="cuda", sas_hidden_units=d,
                           sas_num_blocks=2, sas_heads=1, sas_dropout=0.0, l2_emb=0.0, rs_dtype=dtype)
    return model_factory(a), V, T, 33, 17


def _bert_mid(dtype):
    from rbm_amd.models import model_factory
    z = load_golden("bert_mid")
    V, T, d, L, hd = (int(z[k]) for k in ("V", "T", "d", "L", "h"))
    a = argparse.Namespace(model_code="bert", num_items=V, max_len=T, device="cuda", bert_hidden_units=d,
                           bert_num_blocks=L, bert_num_heads=hd, bert_dropout=0.0, bert_hidden_dropout=0.0,
                           bert_mask_prob=0.2, model_init_seed=4, rs_dtype=dtype)
    m = model_factory(a)
    m.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p/")})
    return m, V, T, 64, 7


MODELS = {"sas_trained": _sas_trained, "bert_mid": _bert_mid, "sas_random": _sas_random}


def _hidden_and_weights(m, ids):
    """The engine's own last-position hidden state and stored head weights (fp64 copies) and the bias (or None)."""
    if hasattr(m, "sas"):
        eng = m.sas.engine()
        return eng.features(ids)[:, -1, :].double(), eng.W("item_emb.weight").double(), None
    eng = m.engine()
    return eng._last_hidden(ids).double(), eng.W("out.weight").double(), eng.Wf("out.bias").double()


@pytest.mark.parametrize("exclude_seen", [True, False])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(MODELS))
def test_models_rank_and_recommend_within_the_summation_bound(name, dtype, exclude_seen):
    """Reference scores S = predict(seq, every item) (rs_candidate_scores: the same hidden state and stored weights, a
    different summation order).  tol(b, v) = 2 (d + 2) 2^-24 (sum_k |h_k| |E_vk| + |bias_v|): the gamma_d dot-product
    bound once per computation -- derived, not measured.  Then lo <= rank <= hi with lo = #{S_v > S_t + tol}, hi =
    #{S_v >= S_t - tol} over admissible v != t, the top-K checks below, and lo == hi on >= 90 % of rows."""
    import rbm_amd.data as synth
    from rbm_amd import metrics
    m, V, T, B, seed = MODELS[name](dtype)
    m.eval()
    rng = np.random.default_rng(seed)
    seq, pos, _ = synth.sas_batch(rng, B, T, V, zipf=synth.ZipfItems(V))
    target = pos[:, -1]
    if hasattr(m, "bert"):
        seq = np.concatenate([seq[:, 1:], np.full((B, 1), V + 1)], axis=1)       # eval appends [MASK]
    seq_t = torch.from_numpy(seq).cuda()
    items = torch.arange(1, V + 1, device="cuda")
    with torch.no_grad():
        S = m.predict(seq_t, items.expand(B, V).contiguous()).double()           # (B, V): column v - 1 = item v
        hcur, W, bias = _hidden_and_weights(m, seq_t)
    d = hcur.shape[1]
    mag = hcur.abs() @ W[1:V + 1].abs().T + (bias[1:V + 1].abs() if bias is not None else 0.0)
    tol = 2.0 * (d + 2) * 2.0 ** -24 * mag
    tgt = torch.from_numpy(target).cuda()
    adm = torch.ones((B, V), dtype=torch.bool, device="cuda")
    if exclude_seen:
        for b in range(B):
            s = seq_t[b][(seq_t[b] >= 1) & (seq_t[b] <= V)]
            adm[b, s - 1] = False
    rows = torch.arange(B, device="cuda")
    St = S[rows, tgt - 1][:, None]
    other = adm.clone()
    other[rows, tgt - 1] = False                      # v != t (and the target is never excluded)
    lo = (other & (S > St + tol)).sum(1)
    hi = (other & (S >= St - tol)).sum(1)
    tight = lo == hi
    assert tight.double().mean() >= 0.9, (int(tight.sum()), B)

    rank = m.full_rank(seq_t, tgt, exclude_seen).long()
    assert bool(((lo <= rank) & (rank <= hi)).all()), (lo.tolist(), rank.tolist(), hi.tolist())

    K = 10
    ids, sc = m.recommend(seq_t, K, exclude_seen)
    assert ids.shape == (B, K) and ids.dtype == torch.int64 and sc.dtype == torch.float32
    assert bool(((ids >= 1) & (ids <= V)).all())                                  # never 0, never [MASK] = V + 1
    assert all(len(set(r)) == K for r in ids.tolist())                            # distinct
    assert bool(adm.gather(1, ids - 1).all())                                     # admissible (never a seen item)
    assert bool(((sc.double() - S.gather(1, ids - 1)).abs() <= tol.gather(1, ids - 1)).all())
    assert bool((sc[:, 1:] <= sc[:, :-1]).all())                                  # non-increasing
    kept = torch.zeros((B, V), dtype=torch.bool, device="cuda")
    kept[rows[:, None], ids - 1] = True
    kth = sc[:, -1:].double()
    assert not bool((adm & ~kept & (S > kth + tol)).any())                        # nothing better was left out

    # full_rank_metrics: equal to the dense route (rs_rank_metrics over every admissible item) on the tight rows
    ks = [1, 5, 10]
    Sa = torch.where(other, S.float(), torch.full_like(S, -1e30, dtype=torch.float32))
    Sa[rows, tgt - 1] = S[rows, tgt - 1].float()
    onehot = torch.zeros((B, V), device="cuda")
    onehot[rows, tgt - 1] = 1.0
    got_t = metrics.full_rank_metrics(m, (seq_t[tight], tgt[tight]), ks, exclude_seen)
    want_t = metrics.recalls_ndcgs_and_mrr_for_ks(Sa[tight], onehot[tight], ks)
    assert got_t == want_t, (got_t, want_t)
    got = metrics.full_rank_metrics(m, (seq, target), ks, exclude_seen)
    want = metrics.recalls_ndcgs_and_mrr_for_ks(Sa, onehot, ks)
    assert set(got) == set(want)
    for k in want:
        assert abs(got[k] - want[k]) <= float((~tight).sum()) / B + 1e-7, (k, got[k], want[k])
