"""CPU checks of BERT4Rec's sampled softmax over batch-shared candidates (no GPU): the float64 head reference against
the plain-torch spelling and its autograd, the scattered bias gradient, the full-catalogue identity against the oracle's
cross-entropy, the host-only parts of the C ABI, and every argument error that needs no device."""
import argparse
import re

import numpy as np
import pytest
import torch

import bert_sce_ref as ref
from oracle import bert as obert
from test_sas_ce_ref import HEADER

NEW = ["rs_sce_head_ws_bytes", "rs_sce_head_dh_splits", "rs_sce_head_path", "rs_sce_head_fwd", "rs_sce_head_bwd"]
ARG, UNSUPPORTED = 1001, 1002
# A 16-byte aligned non-NULL address that points at nothing: every call below that passes it must be rejected by the
# entry's host-side validation (tests/test_abi.py has the rule), so none of them is a valid call.
FAKE = 0x10000


def bert_args(V=60, T=12, d=32, L=1, h=2, device="cpu", seed=0, **kw):
    return argparse.Namespace(model_code="bert", num_items=V, max_len=T, device=device, bert_hidden_units=d,
                              bert_num_blocks=L, bert_num_heads=h, bert_dropout=0.0, bert_hidden_dropout=0.0,
                              bert_mask_prob=0.2, model_init_seed=seed, rs_dtype="fp32", **kw)


def params(V, T, d, L, h, seed=0):
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    m = model_factory(bert_args(V, T, d, L, h, seed=seed))
    P = {k: v.detach().double().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(seed + 1)
    P["out.bias"] = torch.randn(P["out.bias"].shape, generator=g, dtype=torch.float64)     # a bias that matters
    P["out.weight"] = P["out.weight"] * 4
    return P


def batch(rng, B, T, V):
    tok = rng.integers(1, V + 1, (B, T))
    lab = np.where(rng.random((B, T)) < 0.4, rng.integers(1, V + 1, (B, T)), 0)
    tok[0, :3], lab[0, :3] = 0, 0                                   # padding
    tok[lab != 0] = V + 1                                           # [MASK]
    lab[-1, -1] = V
    return torch.from_numpy(tok), torch.from_numpy(lab)


def _head_case(seed=0, cap=40, count=33, d=24, V=50, K=70):
    rng = np.random.default_rng(seed)
    hl, E = rng.standard_normal((cap, d)) * 0.3, rng.standard_normal((V + 1, d)) * 0.3
    bias = rng.standard_normal(V + 1)
    lab = rng.integers(1, V + 1, cap)
    lab[5] = 0                                                       # a row that is none
    cand = rng.integers(0, V + 1, K)                                 # id-0 slots and duplicates for certain (K > V)
    cand[:4] = [lab[0], lab[1], 0, lab[0]]                           # hits
    assert (cand == 0).sum() >= 1 and len(set(cand.tolist())) < K
    return cap, count, d, V, K, hl, E, bias, lab, cand


def test_head_references_agree_with_the_torch_spelling_and_its_autograd():
    cap, count, d, V, K, hl, E, bias, lab, cand = _head_case()
    nvalid = int((lab[:count] != 0).sum())
    lse, z0, out = ref.head_fwd_ref(hl, lab, count, E, bias, cand, float(nvalid))
    ht = torch.from_numpy(hl[:count]).requires_grad_(True)
    Et, bt = torch.from_numpy(E).requires_grad_(True), torch.from_numpy(bias).requires_grad_(True)
    labt, candt = torch.from_numpy(lab[:count]), torch.from_numpy(cand)
    loss = ref.torch_head_definition(ht, Et, bt, labt, candt)
    assert abs(out[2] - loss.item()) < 1e-12 and out[1] == nvalid
    assert abs(ref.sce_from_hidden(ht, Et, bt, labt, candt).item() - loss.item()) < 1e-12
    loss.backward()
    dh, coef, pg, dEc, dbc, keys, mag = ref.head_bwd_ref(hl, lab, count, E, bias, cand, float(nvalid))
    assert np.abs(dh - ht.grad.numpy()).max() < 1e-12
    dE = np.zeros_like(E)
    np.add.at(dE, keys[:count], pg)
    np.add.at(dE, keys[cap:], dEc)
    dE[0] = 0                                                        # key 0: no table row
    assert np.abs(dE - Et.grad.numpy()).max() < 1e-12
    # coef and dbc each against autograd: the bias gradient of a class reached only as a label / only as a candidate
    db = ref.scatter_bias_grad(V + 1, cap, keys, coef, dbc)
    assert np.abs(db - bt.grad.numpy()).max() < 1e-12
    assert np.abs(pg - coef[:, None] * hl[:count]).max() < 1e-12 and not keys[count:cap].any()
    only_label = [v for v in set(lab[:count].tolist()) - set(cand.tolist()) if v]
    only_cand = [v for v in set(cand.tolist()) - set(lab[:count].tolist()) if v]
    assert only_label and only_cand
    for v in only_label:
        assert abs(coef[lab[:count] == v].sum() - bt.grad[v].item()) < 1e-12
    for v in only_cand:
        assert abs(dbc[cand == v].sum() - bt.grad[v].item()) < 1e-12
    assert coef[5] == 0 and not dh[5].any() and not pg[5].any()     # lab 0: no row
    # the magnitude sums carry the |b| terms
    Ec = np.abs(E[cand])
    assert np.allclose(mag["z"], np.abs(hl[:count]) @ Ec.T + np.abs(bias[cand])[None, :], rtol=0, atol=1e-12)
    assert np.allclose(mag["z0"], (np.abs(hl[:count]) * np.abs(E[lab[:count]])).sum(-1) + np.abs(bias[lab[:count]]),
                       rtol=0, atol=1e-12)


def test_a_missing_bias_changes_the_reference():
    cap, count, d, V, K, hl, E, bias, lab, cand = _head_case(seed=3)
    a = ref.head_fwd_ref(hl, lab, count, E, bias, cand, 1.0)[2][0]
    b = ref.head_fwd_ref(hl, lab, count, E, None, cand, 1.0)[2][0]
    import sas_sce_ref as tied
    assert b == tied.head_fwd_ref(hl, lab, count, E, cand, 1.0)[2][0]
    assert abs(a - b) > 1e-3 * abs(b)


@pytest.mark.parametrize("V,T,d,L,h,B,K", [(60, 12, 32, 1, 2, 4, 1), (60, 12, 32, 1, 2, 4, 23), (37, 9, 24, 2, 2, 2, 90)])
def test_model_reference_matches_the_plain_torch_spelling(V, T, d, L, h, B, K):
    P = params(V, T, d, L, h)
    rng = np.random.default_rng(V + K)
    tok, lab = batch(rng, B, T, V)
    cand = torch.from_numpy(rng.integers(0, V + 2, K))               # zeros, duplicates, hits and the id past out's rows
    loss, g = ref.sce_loss_and_grads(P, tok, lab, cand, L, h)
    leaves = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    want = ref.torch_definition(leaves, tok, lab, cand, L, h)
    want.backward()
    assert abs(loss.item() - want.item()) <= 1e-12 * abs(want.item())
    scale = max(torch.linalg.norm(v).item() for v in g.values())
    for k, v in leaves.items():
        w = v.grad if v.grad is not None else torch.zeros_like(v)
        # the attention key bias has an analytically zero gradient (softmax shift invariance): rounding noise only
        size = scale if "linear_layers.1.bias" in k else max(torch.linalg.norm(w).item(), 1e-30)
        assert torch.linalg.norm(g[k] - w) <= 1e-12 * size, k


@pytest.mark.parametrize("V,T,d,L,h,B", [(60, 12, 32, 1, 2, 4), (37, 9, 24, 2, 2, 2)])
def test_all_items_as_candidates_is_the_full_cross_entropy(V, T, d, L, h, B):
    """cand = arange(1, V + 2) (the last id is past out.weight's rows: an ignored slot) against oracle.bert's
    CrossEntropyLoss(ignore_index=0) over all V + 1 classes.  The label's own duplicate is masked and every other item
    is live; the full loss has one class more, class 0, which no candidate list can name.  Put back in closed form:
    ce_r = log(exp(lse_r) + exp(<h_r, E[0]> + b[0])) - z_r0 with lse_r the sampled loss' own log-sum."""
    P = params(V, T, d, L, h)
    tok, lab = batch(np.random.default_rng(V), B, T, V)
    cand = torch.arange(1, V + 2)
    hid = obert.encode(P, tok, L, h)
    W, b = P["out.weight"], P["out.bias"]
    lse, z0, valid = ref.sce_rows(hid, W, b, lab, cand)
    n = int(valid.sum())
    assert n > 0
    plain = ref.sce_loss(P, tok, lab, cand, L, h).item()
    assert abs(((lse - z0) * valid).sum().item() / n - plain) < 1e-12
    zc0 = hid.reshape(-1, d) @ W[0] + b[0]
    back = ((torch.logaddexp(lse, zc0) - z0) * valid).sum().item() / n
    want = obert.ce_loss(obert.forward(P, tok, L, h), lab).item()
    assert abs(back - want) <= 1e-12 * abs(want)
    assert want > plain                                              # and the class-0 term is what separates them


def test_empty_batch_and_rows_without_a_live_candidate_are_zero():
    V, T, d, L, h = 30, 8, 16, 1, 2
    P = params(V, T, d, L, h)
    tok = torch.zeros(1, T, dtype=torch.int64)
    lab = torch.zeros(1, T, dtype=torch.int64)
    tok[0, -2:], lab[0, -2:] = V + 1, 7
    loss, g = ref.sce_loss_and_grads(P, tok, lab, torch.tensor([7, 0, 7, V + 1]), L, h)
    assert loss.item() == 0.0 and all(not v.any() for v in g.values())
    z = torch.zeros(2, T, dtype=torch.int64)
    loss, g = ref.sce_loss_and_grads(P, z + 3, z, torch.tensor([5, 6]), L, h)
    assert loss.item() == 0.0 and all(not v.any() for v in g.values())


# ================================================================ the C ABI, host only
def test_header_declares_and_lib_binds_the_head():
    syms = set(re.findall(r"^(?:int|int64_t) (rs_\w+)\(", open(HEADER).read(), flags=re.M))
    import rbm_amd._lib as L
    from rbm_amd import ops
    for s in NEW:
        assert s in syms, s
        assert s in L.SIGNATURES, s
    assert L.RESTYPES["rs_sce_head_ws_bytes"] is L.C.c_int64 and L.RESTYPES["rs_sce_head_dh_splits"] is L.C.c_int64
    for name in ("sce_head_ws_numel", "sce_head_dh_splits", "sce_head_path", "sce_head_fwd", "sce_head_bwd"):
        assert callable(getattr(ops, name))
    assert L.lib().rs_abi_version() == 2


def test_head_path_by_dtype_and_width():
    import rbm_amd._lib as L
    lib = L.lib()
    for d in (64, 128, 136, 256):
        assert lib.rs_sce_head_path(L.BF16, d) == 1, d               # the MFMA sweep, padded to 64 / 128 / 256
    assert lib.rs_sce_head_path(L.F32, 256) == 0                     # the fp32 tile would not fit: the plain kernel
    assert lib.rs_sce_head_path(L.BF16, 264) == 0
    assert lib.rs_sce_head_path(L.BF16, 50) < 0                      # bf16 rows that are no multiple of 16 bytes
    assert lib.rs_sce_head_path(L.F32, 50) == 1 and lib.rs_sce_head_path(L.F32, 128) == 1
    assert lib.rs_sce_head_path(L.F32, 1024) == 0 and lib.rs_sce_head_path(L.F32, 1025) < 0
    assert lib.rs_sce_head_path(7, 64) < 0
    from rbm_amd import ops
    assert ops.sce_head_path(256, torch.bfloat16) == 1 and ops.sce_head_path(256, torch.float32) == 0


def test_workspace_is_sized_by_dtype_cap_k_d_and_bias_alone():
    """By signature the sizing function cannot see V.  Without a bias and at d <= 128 it is the tied head's size; with
    one it grows by exactly the dbc row-split slabs (K floats per split of the rows, none when the rows are not
    split)."""
    import rbm_amd._lib as L
    from rbm_amd import ops
    from rbm_amd.models.bert_model.bert import SCE_INDEX_ROWS
    lib = L.lib()
    assert len(L.SIGNATURES["rs_sce_head_ws_bytes"]) == 5 and len(L.SIGNATURES["rs_sce_head_dh_splits"]) == 4
    grew = 0
    for dt in (L.F32, L.BF16):
        for cap, K, d in [(1, 1, 64), (1031, 257, 128), (1792, 4096, 64), (25600, 4096, 64), (6400, 16384, 128)]:
            n0, n1 = lib.rs_sce_head_ws_bytes(dt, cap, K, d, 0), lib.rs_sce_head_ws_bytes(dt, cap, K, d, 1)
            assert n0 == lib.rs_sas_sce_ws_bytes(cap, K, d) and n0 > 0
            extra = n1 - n0
            assert extra >= 0 and extra % (4 * K) < 16 and extra // (4 * K) <= 64       # whole slabs (+ alignment)
            grew += extra > 0
            assert lib.rs_sce_head_dh_splits(dt, cap, K, d) == lib.rs_sas_sce_dh_splits(cap, K, d)
    assert grew
    for cap, K in [(1792, 256), (1792, 16384)]:
        n = lib.rs_sce_head_ws_bytes(L.BF16, cap, K, 256, 1)
        assert n > 0 and n == lib.rs_sce_head_ws_bytes(L.BF16, cap, K, 256, 1)
        assert ops.sce_head_ws_numel(cap, K, 256, torch.bfloat16) == n // 4
        a, b = (ops.item_index_ws_bytes(1, cap + K, max(V + 1, SCE_INDEX_ROWS), 256) for V in (1000, 30000))
        assert a == b
    assert lib.rs_sce_head_ws_bytes(L.BF16, 8, 8, 50, 1) < 0 and lib.rs_sce_head_ws_bytes(L.F32, 0, 8, 64, 1) < 0
    assert lib.rs_sce_head_dh_splits(7, 8, 8, 64) < 0


def test_entries_reject_bad_arguments_before_any_launch():
    import rbm_amd._lib as L
    lib = L.lib()

    def fwd(dtype=L.BF16, cap=8, d=64, hl=FAKE, ldh=64, lab=FAKE, E=FAKE, bias=FAKE, V1=20, cand=FAKE, K=4, div=FAKE,
            ws=FAKE, out=FAKE):
        return lib.rs_sce_head_fwd(dtype, cap, d, hl, ldh, lab, None, E, bias, V1, cand, K, div, ws, out, None)

    def bwd(dtype=L.BF16, cap=8, d=64, hl=FAKE, ldh=64, lab=FAKE, E=FAKE, bias=FAKE, V1=20, cand=FAKE, K=4, div=FAKE,
            ws=FAKE, dh=FAKE, coef=FAKE, pg=FAKE, dEc=FAKE, dbc=FAKE):
        return lib.rs_sce_head_bwd(dtype, cap, d, hl, ldh, lab, None, E, bias, V1, cand, K, div, None, ws, dh, coef, pg,
                                   dEc, dbc, None, None)
    kmax = lib.rs_sas_sce_max_k()
    for f in (fwd, bwd):
        assert f(dtype=7) == UNSUPPORTED and f(d=50) == UNSUPPORTED and f(d=1032) == UNSUPPORTED
        assert f(dtype=L.F32, d=1025) == UNSUPPORTED and f(K=0) == UNSUPPORTED and f(K=kmax + 1) == UNSUPPORTED
        assert f(cap=0) == ARG and f(V1=0) == ARG and f(ldh=32) == ARG and f(ws=FAKE + 4) == ARG
        for name in ("hl", "lab", "E", "cand", "div", "ws"):
            assert f(**{name: None}) == ARG, name
    assert fwd(out=None) == ARG
    for name in ("dh", "coef", "pg", "dEc"):
        assert bwd(**{name: None}) == ARG, name
    assert bwd(dbc=None) == ARG                                      # a bias needs dbc
    assert bwd(bias=None) == ARG                                     # and dbc needs a bias
    assert bwd(bias=None, dbc=None, d=50) == UNSUPPORTED and bwd(dbc=None, d=50) == UNSUPPORTED


# ================================================================ the public switch, as far as it runs without a device
def test_model_factory_takes_the_switch_and_needs_k_in_range():
    import rbm_amd  # noqa: F401
    from rbm_amd import ops
    from rbm_amd.models import model_factory
    from rbm_amd.models.bert_model.bert import BERT_LOSSES
    assert BERT_LOSSES == ("ce", "sampled_ce")
    assert model_factory(bert_args()).bert.bert_loss == "ce"
    assert model_factory(bert_args(bert_loss="ce")).bert.bert_loss == "ce"
    m = model_factory(bert_args(bert_loss="sampled_ce", bert_shared_negs=64))
    assert m.bert.bert_loss == "sampled_ce" and m.bert.bert_shared_negs == 64
    with pytest.raises(ValueError, match="bert_loss"):
        model_factory(bert_args(bert_loss="bce"))
    for bad in ({}, {"bert_shared_negs": None}):
        with pytest.raises(ValueError, match="bert_shared_negs"):    # a missing K
            model_factory(bert_args(bert_loss="sampled_ce", **bad))
    for bad in (0, -3, ops.sas_sce_max_k() + 1):
        with pytest.raises(ValueError, match="candidates"):          # K outside [1, max]
            model_factory(bert_args(bert_loss="sampled_ce", bert_shared_negs=bad))
    assert callable(model_factory(bert_args()).sampled_ce_loss)      # whatever bert_loss says
    z = np.zeros((1, 12), np.int64)
    with pytest.raises(RuntimeError):                                # no CPU fallback: the engine needs a device
        m.sampled_ce_loss(z, z, np.arange(1, 5))
    # the same weights whatever the loss says
    sd0, sd1 = model_factory(bert_args()).state_dict(), m.state_dict()
    assert sorted(sd0) == sorted(sd1) and all(torch.equal(sd0[k], sd1[k]) for k in sd0)


def test_fused_train_step_validates_before_touching_a_device():
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    from rbm_amd.train_step import FusedTrainStep
    with pytest.raises(ValueError, match="single device"):
        FusedTrainStep(model_factory(bert_args()), loss="sampled_ce", dp=True)
    with pytest.raises(ValueError, match="single device"):
        FusedTrainStep(model_factory(bert_args(bert_loss="sampled_ce", bert_shared_negs=8)), dp=True)
    with pytest.raises(ValueError, match="single device"):
        FusedTrainStep(model_factory(bert_args()), loss="sampled_ce", dp=False, vocab_shard=True)
    with pytest.raises(ValueError, match="loss"):
        FusedTrainStep(model_factory(bert_args()), loss="bce")


def test_masker_validates_shared_negs_before_touching_a_device():
    from rbm_amd.dataloaders import DeviceBertMasker
    for bad in (0, -1):
        with pytest.raises(ValueError, match="shared_negs"):
            DeviceBertMasker([[1, 2, 3]], 10, 1, 4, 0.2, shared_negs=bad)
