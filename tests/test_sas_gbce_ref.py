"""CPU checks of SASRec's BCE with N negatives per position / gBCE (no GPU): the float64 reference against the
reference's own goldens at N = 1, beta = 1; the closed-form head backward against torch autograd of the plain-torch
spelling; gbce_beta; the float32 / bf16-storage emulation of the head launches and of the weighted table gradient held
to the derived bounds, with every planted mistake rejected at the smallest GPU shape; the host restatement of the
N-negative sampler; and the parts of the C ABI and of the public switch that need no device."""
import re

import numpy as np
import pytest
import torch

import sas_gbce_ref as ref
from conftest import golden_params, load_golden
from oracle import sas as osas
from test_sas_ce_ref import HEADER, batch, params, sas_args

NEW = ["rs_sas_gbce_fwd", "rs_sas_gbce_bwd", "rs_sas_gbce_ws_bytes", "rs_sas_gbce_max_n", "rs_item_grad_weighted",
       "rs_sas_sample_negs"]
BF, F32 = torch.bfloat16, torch.float32


def _close(a, b, tol=1e-12):
    return torch.linalg.norm(a - b) <= tol * max(torch.linalg.norm(b).item(), 1e-30)


# ---------------------------------------------------------------- the definition
def test_one_negative_and_beta_one_is_the_reference_loss_on_its_golden():
    """sas_tiny.npz: gbce at N = 1, beta = 1 equals oracle.sas.bce_loss / loss_and_grads, loss and every gradient to
    1e-12 relative -- and the golden's reference-generated loss to the golden's own (float32) precision."""
    z = load_golden("sas_tiny")
    P = {k: v.double() for k, v in golden_params(z).items()}
    L, h = int(z["L"]), int(z["h"])
    seq, pos, neg = (torch.from_numpy(z[k]) for k in ("seq", "pos", "neg"))
    want, _, _, gw = osas.loss_and_grads(P, seq, pos, neg, L, h)
    loss, g = ref.gbce_loss_and_grads(P, seq, pos, neg[..., None], 1.0, L, h)
    assert abs(loss.item() - want.item()) <= 1e-12 * abs(want.item())
    for k, v in gw.items():
        assert _close(g[k], v if v is not None else torch.zeros_like(g[k])), k
    assert abs(loss.item() - float(z["loss"])) < 1e-5 * max(1.0, abs(float(z["loss"])))
    l2, _ = ref.gbce_loss_and_grads(P, seq, pos, neg, 1.0, L, h)                 # (B, T) is N = 1
    assert l2.item() == loss.item()


def _head_case(N, M=23, d=16, V=12, seed=0, all_pad=False):
    g = torch.Generator().manual_seed(seed + N)
    f = torch.randn(M, d, generator=g, dtype=torch.float64)
    E = torch.randn(V + 1, d, generator=g, dtype=torch.float64)
    E[0] = 0
    pos = torch.randint(1, V + 1, (M,), generator=g)
    pos[::5] = 0
    neg = torch.randint(0, V + 1, (M, N), generator=g)
    neg[1, 0] = 0                                   # an id-0 negative
    neg[2, :] = neg[2, 0]                           # duplicates
    neg[3, -1] = pos[3]                             # a negative equal to the positive
    if all_pad:
        pos[:] = 0
    return f, E, pos, neg


@pytest.mark.parametrize("beta", [1.0, 0.3])
@pytest.mark.parametrize("N", [1, 3, 17])
def test_closed_form_head_backward_is_torch_autograd_of_the_plain_spelling(N, beta):
    for all_pad in (False, True):
        f, E, pos, neg = _head_case(N, all_pad=all_pad)
        ft, Et = f.clone().requires_grad_(True), E.clone().requires_grad_(True)
        want = ref.torch_head(ft, Et, pos, neg, beta)
        want.backward()
        loss, df, dE = ref.closed_form_head(f, E, pos, neg, beta)
        assert abs(loss.item() - want.item()) <= 1e-12 * max(abs(want.item()), 1e-30)
        assert _close(df, ft.grad) and _close(dE, Et.grad)
        assert not dE[0].any()
        if all_pad:
            assert loss.item() == 0.0 and not df.any() and not dE.any()
        # and the model-level reference's head is the same function
        l2 = ref.gbce_from_feats(f[None], E, pos[None], neg[None], beta, osas.Exact())
        assert abs(l2.item() - want.item()) <= 1e-12 * max(abs(want.item()), 1e-30)


def test_negatives_are_summed_and_an_id_zero_negative_counts_softplus_zero():
    f, E, pos, neg = _head_case(3)
    base, _, _ = ref.closed_form_head(f, E, pos, neg, 1.0)
    more, _, _ = ref.closed_form_head(f, E, pos, torch.cat([neg, torch.zeros_like(neg[:, :1])], 1), 1.0)
    assert abs((more - base).item() - np.log(2.0)) < 1e-12          # one more id-0 negative per valid row: + log 2
    twice, _, _ = ref.closed_form_head(f, E, pos, torch.cat([neg, neg], 1), 1.0)
    onlyp, _, _ = ref.closed_form_head(f, E, pos, neg[:, :0], 1.0)
    assert abs((twice - onlyp).item() - 2 * (base - onlyp).item()) < 1e-12


def test_model_reference_matches_the_closed_form_through_the_network():
    V, T, d, L, h, B, N = 37, 9, 50, 1, 2, 2, 3
    P = params(V, T, d, L, h)
    rng = np.random.default_rng(V)
    seq, pos = batch(rng, B, T, V)
    neg = torch.from_numpy(rng.integers(0, V + 1, (B, T, N)))
    loss, g = ref.gbce_loss_and_grads(P, seq, pos, neg, 0.3, L, h)
    f = osas.log2feats(P, seq, L, h).reshape(-1, d)
    want, _, dE = ref.closed_form_head(f, P["sas.item_emb.weight"], pos, neg, 0.3)
    assert abs(loss.item() - want.item()) <= 1e-12 * abs(want.item())
    assert not g["sas.item_emb.weight"][0].any()
    z = torch.zeros(B, T, dtype=torch.int64)
    loss, g = ref.gbce_loss_and_grads(P, z, z, neg, 0.3, L, h)
    assert loss.item() == 0.0 and all(not v.any() for v in g.values())


# ---------------------------------------------------------------- gbce_beta
def test_gbce_beta_pins_its_values():
    import rbm_amd  # noqa: F401
    from rbm_amd.models.sas import gbce_beta
    assert "alpha * (t * (1 - 1 / alpha) + 1 / alpha)" in gbce_beta.__doc__
    for n, V in [(1, 3416), (16, 3416), (256, 54542), (7, 9)]:
        alpha = min(1.0, n / (V - 1))
        assert gbce_beta(n, V, 0.0) == 1.0
        assert abs(gbce_beta(n, V, 1.0) - alpha) <= 1e-15
        ts = np.linspace(0, 1, 11)
        b = [gbce_beta(n, V, float(t)) for t in ts]
        assert all(x >= y for x, y in zip(b, b[1:]))                  # monotone in t, from 1 down to alpha
        assert all(abs(x - ref.gbce_beta_ref(n, V, float(t))) <= 1e-15 for x, t in zip(b, ts))
    for n in (40, 41, 100):                                           # N >= V - 1: alpha clamps to 1
        assert gbce_beta(n, 41, 0.5) == 1.0 and gbce_beta(n, 41, 1.0) == 1.0
    with pytest.raises(ValueError):
        gbce_beta(4, 100, 1.5)


# ---------------------------------------------------------------- emulation under the bounds, mutations rejected
HEAD_CASES = [(BF, 64, 1, 1, 1), (BF, 64, 63, 3, 62), (BF, 128, 65, 4, 65), (F32, 64, 65, 5, 1), (BF, 128, 63, 67, 0),
              (F32, 256, 9, 17, 9)]


@pytest.mark.parametrize("dt,d,cap,N,count", HEAD_CASES)
@pytest.mark.parametrize("beta", [1.0, 0.07])
def test_head_emulation_is_within_the_bounds(dt, d, cap, N, count, beta):
    inp = ref.head_inputs(cap, N, d, dt, count, beta=beta, dloss=0.75)
    res = ref.check_head(inp, ref.emu_head(inp))
    assert max(res.values()) <= 1.0, res
    dense = ref.head_inputs(cap, N, 50, F32, cap, beta=beta, dense=True)
    res = ref.check_head(dense, ref.emu_head(dense))
    assert max(res.values()) <= 1.0, res
    big = ref.head_inputs(cap, N, d, dt, count, beta=beta, big=True)
    res = ref.check_head(big, ref.emu_head(big))
    assert max(res.values()) <= 1.0, res


def test_large_logit_case_reaches_eighty():
    inp = ref.head_inputs(63, 5, 64, BF, 63, big=True)
    z = ref.head_ref(inp)["z"].abs().max().item()
    assert 60 < z < 110, z


@pytest.mark.parametrize("mut", ["beta_on_negs", "neg_mean", "drop_id0", "g0_sign", "past_count"])
def test_planted_head_mistakes_are_rejected_at_the_smallest_shape(mut):
    """cap 63, N = 3 (N = 1 cannot tell a mean from a sum), beta = 0.07, count = cap - 1 (a row past the count)."""
    inp = ref.head_inputs(63, 3, 64, BF, 62, beta=0.07)
    assert max(ref.check_head(inp, ref.emu_head(inp)).values()) <= 1.0
    res = ref.check_head(inp, ref.emu_head(inp, mut=mut))
    assert max(res.values()) > 1.0, (mut, res)


W_CASES = [(F32, 64, 50, 1, 41, 0.0, False), (BF, 64, 40, 2, 41, 0.7, False), (F32, 50, 5, 258, 41, 0.0, False),
           (BF, 128, 64, 4, 41, 0.0, True)]


@pytest.mark.parametrize("dt,d,rows,per,table_rows,hot,edge", W_CASES)
def test_weighted_gradient_emulation_is_within_the_bounds(dt, d, rows, per, table_rows, hot, edge):
    inp = ref.weighted_inputs(rows, per, d, dt, table_rows, hot=hot, edge=edge)
    assert (inp["keys"] == 0).any()
    res = ref.check_weighted(inp, ref.emu_weighted(inp))
    assert max(res.values()) <= 1.0, res


@pytest.mark.parametrize("mut", ["key0_grad", "w_by_row"])
def test_planted_weighted_gradient_mistakes_are_rejected_at_the_smallest_shape(mut):
    inp = ref.weighted_inputs(40, 2, 64, BF, 41)                      # per = 1 cannot tell a row from an entry
    res = ref.check_weighted(inp, ref.emu_weighted(inp, mut=mut))
    assert max(res.values()) > 1.0, (mut, res)


def test_every_mutation_has_a_test():
    assert set(ref.MUTATIONS) == {"beta_on_negs", "neg_mean", "drop_id0", "g0_sign", "past_count", "key0_grad",
                                  "w_by_row"}


# ---------------------------------------------------------------- the sampler's counter rule on the host
def _histories(n_users=9, item_num=30, seed=2):
    rng = np.random.default_rng(seed)
    return [list(rng.permutation(np.arange(1, item_num + 1))[:int(rng.integers(2, 26))]) for _ in range(n_users)]


def test_host_restatement_of_the_n_negative_counter_rule():
    B, T, N, V = 5, 7, 3, 30
    hist = _histories()
    seq, pos, neg = ref.sample_negs_ref(hist, V, B, T, N, 1, 1234)
    s1, p1, n1 = ref.sample_negs_ref(hist, V, B, T, 1, 1, 1234)
    assert (seq == s1).all() and (pos == p1).all() and (neg[:, :, 0] == n1[:, :, 0]).all()     # j = 0: the N = 1 stream
    assert neg.min() >= 0 and neg.max() <= V
    pad = pos == 0
    assert (neg[pad] == 0).all() and (seq[pad] == 0).all() and pad.any() and (~pad).any()
    for b in range(B):
        win = set(seq[b][seq[b] != 0]) | set(pos[b][pos[b] != 0])
        assert not (set(neg[b][~pad[b]].reshape(-1)) & win)             # no negative in its row's window
    assert (neg[:, :, 0] != neg[:, :, 1])[~pad].any()                   # another counter block, another draw
    other = ref.sample_negs_ref(hist, V, B, T, N, 2, 1234)[2]
    assert (other != neg).any()


# ---------------------------------------------------------------- ABI and arguments without a device
def test_header_declares_and_lib_exports_the_new_entries():
    import ctypes
    syms = set(re.findall(r"^(?:int|int64_t) (rs_\w+)\(", open(HEADER).read(), flags=re.M))
    import rbm_amd._lib as L
    from rbm_amd import ops
    h = ctypes.CDLL(L.LIB_PATH)
    for s in NEW:
        assert s in syms, s
        assert s in L.SIGNATURES, s
        assert getattr(h, s) is not None
    assert L.RESTYPES["rs_sas_gbce_ws_bytes"] is L.C.c_int64 and L.RESTYPES["rs_sas_gbce_max_n"] is L.C.c_int64
    for name in ("sas_gbce_fwd", "sas_gbce_bwd", "sas_gbce_ws_numel", "sas_gbce_max_n", "item_grad_weighted",
                 "sas_sample_negs"):
        assert callable(getattr(ops, name))
    assert L.lib().rs_abi_version() == 2
    text = open(HEADER).read()
    assert "beta * softplus(-z_r0) + sum_j softplus(z_rj)" in text


def test_workspace_grows_with_cap_n_and_not_with_the_catalogue():
    import rbm_amd._lib as L
    from rbm_amd import ops
    from rbm_amd.models.sas_model.sas import SCE_INDEX_ROWS
    assert len(L.SIGNATURES["rs_sas_gbce_ws_bytes"]) == 3             # (cap, N, d): no argument for V
    assert ops.sas_gbce_max_n() == 1024
    lib = L.lib()
    for cap, N, d in [(63, 1, 64), (209, 67, 128), (25600, 16, 128), (6400, 256, 128)]:
        n = lib.rs_sas_gbce_ws_bytes(cap, N, d)
        assert n >= 4 * cap * (1 + N)
        assert n <= 4 * cap * (1 + N) + 16 + 8 * 3 * (cap // 4 + 1)   # the logits and the partials: never cap * N * d
        assert lib.rs_sas_gbce_ws_bytes(cap, N, 2 * d) == n
        assert lib.rs_sas_gbce_ws_bytes(2 * cap, N, d) > n and lib.rs_sas_gbce_ws_bytes(cap, 2 * N, d) > n
        a, b = (ops.item_index_ws_bytes(1, cap * (1 + N), max(V + 1, SCE_INDEX_ROWS), d) for V in (1000, 30000))
        assert a == b
    assert lib.rs_sas_gbce_ws_bytes(8, 1025, 64) == -1 and lib.rs_sas_gbce_ws_bytes(8, 0, 64) == -1
    assert lib.rs_sas_gbce_ws_bytes(1 << 22, 1024, 64) == -1          # cap * (1 + N) >= 2^31


def test_model_factory_takes_gbce_and_needs_sas_negs():
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    from rbm_amd.models.sas_model.sas import SAS_LOSSES, SAS_NEG_LOSSES
    assert SAS_LOSSES == ("bce", "ce", "sampled_ce") and SAS_NEG_LOSSES == ("gbce",)
    m = model_factory(sas_args(sas_loss="gbce", sas_negs=16))
    assert m.sas.sas_loss == "gbce" and m.sas.sas_negs == 16 and m.sas.sas_gbce_t == 0.0
    assert model_factory(sas_args(sas_loss="gbce", sas_negs=4, sas_gbce_t=0.75)).sas.sas_gbce_t == 0.75
    for bad in ({}, {"sas_negs": 0}, {"sas_negs": None}, {"sas_negs": -3}):
        with pytest.raises(ValueError, match="sas_negs"):
            model_factory(sas_args(sas_loss="gbce", **bad))
    with pytest.raises(ValueError, match="sas_gbce_t"):
        model_factory(sas_args(sas_loss="gbce", sas_negs=4, sas_gbce_t=2.0))
    assert callable(model_factory(sas_args()).gbce_loss)              # whatever sas_loss says
    z = np.zeros((1, 16), np.int64)
    with pytest.raises(RuntimeError):                                 # no CPU fallback: the engine needs a device
        m.gbce_loss(z, z, np.zeros((1, 16, 16), np.int64))


def test_fused_train_step_refuses_before_touching_a_device():
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    from rbm_amd.train_step import FusedTrainStep
    m = model_factory(sas_args(sas_loss="gbce", sas_negs=8))
    with pytest.raises(ValueError, match="single device"):
        FusedTrainStep(m, dp=True)
    with pytest.raises(ValueError, match="single device"):
        FusedTrainStep(model_factory(sas_args(sas_negs=8)), loss="gbce", dp=True)
    with pytest.raises(ValueError, match="shard_rows"):
        FusedTrainStep(m, shard_rows="on", dp=False)
    with pytest.raises(ValueError, match="sas_negs"):
        FusedTrainStep(model_factory(sas_args()), loss="gbce", dp=False)
    with pytest.raises(ValueError, match="gbce_beta"):
        FusedTrainStep(m, dp=False, gbce_beta=-1.0)
    with pytest.raises(ValueError, match="gbce_beta"):
        FusedTrainStep(model_factory(sas_args()), loss="bce", dp=False, gbce_beta=0.5)


def test_sampler_refuses_negs_with_shared_negs_or_a_proposal():
    import rbm_amd  # noqa: F401
    from rbm_amd.dataloaders import DeviceWarpSampler
    hist = _histories()
    with pytest.raises(ValueError, match="negs"):
        DeviceWarpSampler(hist, 30, 4, 7, device="cpu", negs=3, shared_negs=8)
    with pytest.raises(ValueError, match="negs"):
        DeviceWarpSampler(hist, 30, 4, 7, device="cpu", negs=3, proposal=object())
    with pytest.raises(ValueError, match="negs"):
        DeviceWarpSampler(hist, 30, 4, 7, device="cpu", negs=0)
    with pytest.raises(ValueError, match="negs"):
        DeviceWarpSampler(hist, 30, 4, 7, device="cpu", negs=1025)
