"""CPU checks of tests/vocab_shard_ref.py and of the host-side rules behind the sharded vocabulary head:
  * the float64 reference of the sharded chain against torch float64 autograd of F.cross_entropy(ignore_index=0) on
    the concatenated vocabulary;
  * the float32/bf16 emulation of the chain within every bound at the GPU tests' shape list and patterns, and every
    planted mistake (vocab_shard_ref.MUTATIONS) rejected at the smallest listed shape that exercises it;
  * vocab_parallel.shard_range: 128-aligned, disjoint, covering; an empty shard is VocabShard's ValueError;
  * rs_vocab_head_form (host only, cus = 256) against a restatement of the LDS budget: the backward flips to the
    lock-step form exactly one 32-row tile past the limit (104 tiles at d = 256, 296 at d = 128, 392 at d = 64), the
    forward never, RS_VHEAD_PP=0 gives the lock-step form everywhere, bad arguments are refused."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import losshead_ref as L
import vocab_shard_ref as S

CPU = "cpu"


def ok(res):
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, bad


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("N,V1,d,R", [(2, 200, 64, 37), (3, 257, 64, 37), (3, 5001, 128, 130)])
@pytest.mark.parametrize("pattern", [None, "boundary"])
def test_reference_is_cross_entropy_on_the_concatenated_vocabulary(N, V1, d, R, pattern):
    inp = S.shard_inputs(d, R, V1, N, CPU, pattern=pattern)
    lab = inp["labels"]
    x = L.vce_logits(inp)[0].requires_grad_()
    count, dloss = float((lab != 0).sum()), 0.37
    loss = F.cross_entropy(x, lab, ignore_index=0, reduction="sum")
    (g,) = torch.autograd.grad(loss * dloss / count, x)
    xd = x.detach()
    # the chain in float64: per-shard lse, owned label logits, combine, per-shard gradient
    lse_q = torch.stack([torch.logsumexp(xd[:, v0:v1], 1) for v0, v1 in inp["ranges"]])
    Lg = torch.logsumexp(lse_q, 0)
    tgt = sum(xd.gather(1, lab[:, None])[:, 0] * S.owned(lab, v0, v1) for v0, v1 in inp["ranges"])
    assert torch.allclose(((Lg - tgt) * (lab != 0)).sum(), loss.detach(), rtol=1e-12, atol=0)
    gs = torch.cat([S.ref_shard_grad(xd[:, v0:v1], lab, v0, v1, Lg, count, dloss)[0] for v0, v1 in inp["ranges"]], 1)
    assert torch.allclose(gs, g, rtol=1e-10, atol=1e-15)
    # every label's one-hot in exactly one shard
    oh = torch.cat([S.ref_shard_grad(xd[:, v0:v1], lab, v0, v1, Lg, count, dloss)[1] for v0, v1 in inp["ranges"]], 1)
    assert torch.equal(oh.sum(1), (lab != 0).double()) and torch.equal(oh.argmax(1)[lab != 0], lab[lab != 0])


def test_grad_bound_is_vce_grad_bound_on_one_shard():
    inp = S.shard_inputs(64, 37, 200, 1, CPU)
    x, Ax = L.vce_logits(inp)
    lab = inp["labels"]
    Lg = torch.logsumexp(x, 1)
    r, oh = S.ref_shard_grad(x, lab, 0, 200, Lg, 11.0, 0.5)
    assert torch.equal(r, L.ref_ce_grad(x, lab, Lg, 11.0, 0.5))
    pAx = (torch.exp(x - Lg[:, None]) * Ax).sum(1)
    assert torch.equal(S.lse_bound_from(pAx, Lg, 64), L.vce_lse_bound(x, Ax, Lg, 64))
    live = (lab != 0).double()[:, None]
    assert torch.equal(S.grad_bound(x, Ax, Lg, live, oh, r, 64, 0.5 / 11), L.vce_grad_bound(x, Ax, Lg, lab, r, 64, 0.5 / 11))


# ------------------------------------------------------------------ the emulation and the mutations
def emu_res(inp, mut=None, dloss=1.0):
    logits = L.vce_logits(inp)
    got = S.emu_chain(inp, dloss=dloss, mut=mut)
    return S.check_chain(inp, logits, got, float(got["out"][1]), dloss), logits


@pytest.mark.parametrize("N,V1,d,R", S.CHAIN_CASES)
def test_emulation_within_every_bound(N, V1, d, R):
    for bias in (True, False):
        ok(emu_res(S.shard_inputs(d, R, V1, N, CPU, bias=bias))[0])


@pytest.mark.parametrize("d", S.PATTERN_D)
@pytest.mark.parametrize("pattern", S.PATTERNS)
def test_emulation_within_every_bound_on_the_patterns(pattern, d):
    N, V1, R = S.PATTERN_SHAPE
    inp = S.shard_inputs(d, R, V1, N, CPU, pattern=pattern)
    res, logits = emu_res(inp, dloss=0.37)
    ok(res)
    lab, (v0, v1) = inp["labels"], inp["ranges"][-1]
    if pattern == "boundary":
        assert {v0 - 1, v0, v0 + 1, V1 - 1, 1} <= set(lab.tolist())
    if pattern == "free":
        assert int((lab != 0).sum()) > 0 and not S.owned(lab, v0, v1).any()
    if pattern == "dead":
        got = S.emu_chain(inp)
        assert not lab.any() and not got["out"].any() and not got["lse"].any() and not any(t.any() for t in got["dl"])
    if pattern == "big":
        assert S.big_ok(inp, logits)


@pytest.mark.parametrize("mut", list(S.MUTATIONS))
def test_every_mutation_is_rejected(mut):
    pattern, N, V1, d, R = S.MUTATIONS[mut]
    inp = S.shard_inputs(d, R, V1, N, CPU, pattern=pattern)
    ok(emu_res(inp)[0])                                     # the unmutated chain passes at this very shape
    res = emu_res(inp, mut=mut)[0]
    key = {"onehot_all": "dlogits.away", "no_v0": "tgt_q", "drop_shard": "lse", "local_max": "lse",
           "dead_mul": "dlogits.dead"}[mut]
    assert res[key] > 1.0, (mut, res)
    if mut in ("drop_shard", "local_max"):                  # (dlogits is staged: it follows the stored lse)
        assert res["lse.e2e"] > 1.0, res


# ------------------------------------------------------------------ shard_range
@pytest.mark.parametrize("V1", [257, 5001, 70001, 1000001])
def test_shard_range_is_aligned_disjoint_and_covering(V1):
    from rbm_amd.vocab_parallel import ALIGN, shard_range
    for world in range(1, 9):
        rng = [shard_range(V1, world, r) for r in range(world)]
        assert rng[0][0] == 0 and max(v1 for _, v1 in rng) == V1
        for (a0, a1), (b0, b1) in zip(rng, rng[1:]):
            assert a1 == b0 and a0 <= a1                    # disjoint, in order, no gap
        assert all(v0 % ALIGN == 0 for v0, v1 in rng if v1 > v0)        # (an empty shard is [V1, V1))
        assert all(v1 % ALIGN == 0 or v1 == V1 for _, v1 in rng)
        sizes = [v1 - v0 for v0, v1 in rng]
        assert sizes == sorted(sizes, reverse=True) and sizes[0] - (V1 + world - 1) // world < ALIGN


def test_empty_shard_is_a_value_error(monkeypatch):
    import torch.distributed as dist
    from rbm_amd.vocab_parallel import VocabShard, shard_range
    assert shard_range(257, 4, 3) == (257, 257)             # three shards of 128 hold all 257 rows
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 4)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 3)
    with pytest.raises(ValueError, match="too small for 4 shards of 128"):
        VocabShard(257)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 2)
    vs = VocabShard(257)
    assert (vs.v0, vs.v1) == (256, 257)


def test_dh_split_helper():
    from rbm_amd.models.bert_model.bert import head_dh_splits
    assert [head_dh_splits(v) for v in (1, 2048, 2049, 5001, 131072, 131073, 1000001)] == [1, 1, 2, 3, 64, 64, 64]


# ------------------------------------------------------------------ rs_vocab_head_form
CUS = 256


def form(bwd, R, V1, d, cus=CUS):
    from rbm_amd import ops
    return ops.vocab_head_form(bwd, R, V1, d, cus)


def test_lds_budget_restatement():
    assert {d: S.pp_fixed_bytes(d, True) for d in S.PP_FIXED} == S.PP_FIXED
    assert {d: S.pp_tile_limit(d) for d in (256, 128, 64)} == {256: 104, 128: 296, 64: 392}


@pytest.mark.parametrize("d", [64, 128, 256])
def test_form_equals_the_restated_budget(d, monkeypatch):
    monkeypatch.delenv("RS_VHEAD_PP", raising=False)
    lim = S.pp_tile_limit(d)
    for V1 in (200, 5001, 26745, 128 * 256, 128 * 256 + 1, 33025, 70001, 1000001):
        for R in (1, 37, 130, 1750, 3584, 32 * lim, 32 * lim + 1, 64 * lim, 64 * lim + 1, 20000):
            for bwd in (0, 1):
                assert form(bwd, R, V1, d) == S.expected_form(bwd, R, V1, d, CUS), (bwd, R, V1, d)
                assert form(0, R, V1, d)[0] == 1                   # the forward never flips
    # one y-group (more than half as many 256-class tiles as CUs): exactly one row tile past the limit
    V1 = 128 * 256 + 1
    assert form(1, 32 * lim, V1, d)[:4] == (1, 129, 1, lim) and form(1, 32 * lim, V1, d)[4] <= S.LDS_MAX
    assert form(1, 32 * lim + 1, V1, d)[0] == 0
    # two y-groups: twice the rows
    assert form(1, 64 * lim, V1 - 1, d)[:4] == (1, 128, 2, lim) and form(1, 64 * lim + 1, V1 - 1, d)[0] == 0
    # the sharded cfg5 step on two ranks: 2 x 1,792 rows against half of 1M + 1 classes
    assert form(1, 3584, 500096, d)[0] == (0 if d == 256 else 1)
    # fewer CUs, and the device's own count is not asked for when one is given
    assert form(1, 130, 5001, d, cus=8) == S.expected_form(1, 130, 5001, d, 8)


def test_form_honours_rs_vhead_pp(monkeypatch):
    monkeypatch.setenv("RS_VHEAD_PP", "0")
    for d in (64, 128, 256):
        for R, V1 in ((37, 200), (130, 5001), (3584, 500096)):
            for bwd in (0, 1):
                assert form(bwd, R, V1, d) == S.expected_form(bwd, R, V1, d, CUS, pp=False)
                assert form(bwd, R, V1, d)[0] == 0
    monkeypatch.setenv("RS_VHEAD_PP", "1")
    assert form(1, 130, 5001, 256)[0] == 1


def test_form_refuses_bad_arguments():
    import rbm_amd._lib as lib
    out = (ctypes.c_int * 5)()
    f = lib.lib().rs_vocab_head_form
    assert f(1, 130, 5001, 256, CUS, out) == 0
    for args in ((1, 130, 5001, 96, CUS, out), (1, 0, 5001, 256, CUS, out), (1, 130, 0, 256, CUS, out),
                 (2, 130, 5001, 256, CUS, out), (-1, 130, 5001, 256, CUS, out), (1, 130, 5001, 256, CUS, None)):
        assert f(*args) == 1001, args[:5]
