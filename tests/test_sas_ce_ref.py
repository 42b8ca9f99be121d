"""CPU checks of the SASRec tied full-catalogue cross-entropy loss (no GPU): the float64 reference helper against
plain torch autograd of the definition, the public switch (args.sas_loss, FusedTrainStep(loss=)) as far as it runs
without a device, and the C-ABI boundary of the new row kernels."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

import sas_ce_ref as ref
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "recsys_hip.h")
NEW = ["rs_sas_ce_rows_fwd", "rs_sas_ce_rows_bwd", "rs_sas_ce_rows_nparts"]


def sas_args(V=60, T=16, d=64, L=2, h=1, device="cpu", **kw):
    return argparse.Namespace(model_code="sas", num_items=V, max_len=T, device=device, sas_hidden_units=d,
                              sas_num_blocks=L, sas_heads=h, sas_dropout=0.0, l2_emb=0.0, rs_dtype="fp32", **kw)


def params(V, T, d, L, h, seed=0):
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    torch.manual_seed(seed)
    m = model_factory(sas_args(V, T, d, L, h))
    return {k: v.detach().double() for k, v in m.state_dict().items()}


def batch(rng, B, T, V, pads=(0, 3)):
    seq = rng.integers(1, V + 1, (B, T))
    pos = rng.integers(1, V + 1, (B, T))
    for b, n in enumerate(pads):
        seq[b, :n] = 0
        pos[b, :n] = 0
    return torch.from_numpy(seq), torch.from_numpy(pos)


@pytest.mark.parametrize("V,T,d,L,h,B", [(60, 16, 64, 2, 1, 4), (37, 9, 50, 1, 2, 2)])
def test_helper_matches_torch_autograd_of_the_definition(V, T, d, L, h, B):
    P = params(V, T, d, L, h)
    seq, pos = batch(np.random.default_rng(V), B, T, V)
    loss, g = ref.ce_loss_and_grads(P, seq, pos, L, h)
    leaves = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    want = ref.torch_definition(leaves, seq, pos, L, h)
    want.backward()
    assert abs(loss.item() - want.item()) <= 1e-12 * abs(want.item())
    for k, v in leaves.items():
        w = v.grad if v.grad is not None else torch.zeros_like(v)
        assert torch.linalg.norm(g[k] - w) <= 1e-12 * max(torch.linalg.norm(w).item(), 1e-30), k
    assert not g["sas.item_emb.weight"][0].any()                 # the padding row: exactly zero
    assert g["sas.item_emb.weight"][1:].abs().sum(-1).gt(0).all()   # every other row is reached


def test_all_padding_batch_gives_zero_loss_and_gradients():
    V, T, d, L, h = 30, 8, 64, 1, 1
    P = params(V, T, d, L, h)
    z = torch.zeros(2, T, dtype=torch.int64)
    loss, g = ref.ce_loss_and_grads(P, z, z, L, h)
    assert loss.item() == 0.0
    assert all(not v.any() for v in g.values())


def test_emulation_stays_near_the_exact_math():
    """The bf16-storage emulation is the same objective: its loss is within the bf16 forward bar of the exact one
    (item table scaled by 0.1 as in the GPU cases)."""
    from oracle import sas as osas
    V, T, d, L, h = 60, 16, 64, 2, 1
    P = params(V, T, d, L, h)
    P["sas.item_emb.weight"] = P["sas.item_emb.weight"] * 0.1
    seq, pos = batch(np.random.default_rng(3), 4, T, V)
    le, _ = ref.ce_loss_and_grads(P, seq, pos, L, h, emu=osas.BF16Storage())
    lx, _ = ref.ce_loss_and_grads(P, seq, pos, L, h)
    assert abs(le.item() - lx.item()) < 3e-2 * max(1.0, abs(lx.item()))


def test_model_factory_takes_the_loss_switch():
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    assert model_factory(sas_args()).sas.sas_loss == "bce"
    assert model_factory(sas_args(sas_loss="bce")).sas.sas_loss == "bce"
    assert model_factory(sas_args(sas_loss="ce")).sas.sas_loss == "ce"
    assert model_factory(sas_args(sas_loss=None)).sas.sas_loss == "bce"
    with pytest.raises(ValueError):
        model_factory(sas_args(sas_loss="x"))


def test_ce_loss_is_part_of_the_model_api():
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    m = model_factory(sas_args())
    assert callable(m.ce_loss)
    z = np.zeros((1, 16), np.int64)
    with pytest.raises(RuntimeError):         # no CPU fallback: the engine needs a device
        m.ce_loss(z, z)


def test_fused_train_step_validates_loss_before_touching_a_device():
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    from rbm_amd.train_step import FusedTrainStep
    m = model_factory(sas_args())
    with pytest.raises(ValueError, match="loss"):
        FusedTrainStep(m, loss="x")
    with pytest.raises(ValueError, match="single device"):
        FusedTrainStep(m, loss="ce", dp=True)
    with pytest.raises(ValueError, match="single device"):
        FusedTrainStep(model_factory(sas_args(sas_loss="ce")), dp=True)     # loss=None takes the model's


def test_fused_train_step_ce_needs_a_sas_model():
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    from rbm_amd.train_step import FusedTrainStep
    a = argparse.Namespace(model_code="bert", num_items=40, max_len=8, device="cpu", bert_hidden_units=64,
                           bert_num_blocks=1, bert_num_heads=2, bert_dropout=0.0, bert_hidden_dropout=0.0,
                           model_init_seed=0, rs_dtype="fp32")
    with pytest.raises(ValueError, match="SAS"):
        FusedTrainStep(model_factory(a), loss="ce")


def test_header_declares_and_lib_binds_the_row_kernels():
    syms = set(re.findall(r"^(?:int|int64_t) (rs_\w+)\(", open(HEADER).read(), flags=re.M))
    import rbm_amd._lib as L
    from rbm_amd import ops
    for s in NEW:
        assert s in syms, s
        assert s in L.SIGNATURES, s
    assert L.RESTYPES["rs_sas_ce_rows_nparts"] is L.C.c_int64
    for name in ("sas_ce_rows_fwd", "sas_ce_rows_bwd", "sas_ce_rows_nparts"):
        assert callable(getattr(ops, name))


def test_nparts_is_host_only():
    from rbm_amd import ops
    assert ops.sas_ce_rows_nparts(1) == 1
    assert ops.sas_ce_rows_nparts(16) == 1 and ops.sas_ce_rows_nparts(17) == 2
    assert ops.sas_ce_rows_nparts(4135) == 259
    assert ops.sas_ce_rows_nparts(25600) == 512                  # bounded: one partial set per workgroup
    assert ops.sas_ce_rows_nparts(0) == 0


def test_row_kernel_references_agree_with_torch_layernorm():
    """rows_fwd_ref / rows_bwd_ref against torch autograd of LayerNorm on the gathered rows."""
    rng = np.random.default_rng(0)
    M, d, cap = 45, 64, 64
    x = rng.standard_normal((M, d))
    labels = (rng.random(M) < 0.4) * rng.integers(1, 9, M)
    gamma, beta = rng.standard_normal(d), rng.standard_normal(d)
    idx, rank, n, hl, lab, mu, rstd = ref.rows_fwd_ref(x, labels, cap, gamma, beta)
    assert n == int((labels != 0).sum()) and (lab == labels[labels != 0]).all()
    xt = torch.from_numpy(x[idx[:n]]).requires_grad_(True)
    gt, bt = torch.from_numpy(gamma).requires_grad_(True), torch.from_numpy(beta).requires_grad_(True)
    y = torch.nn.functional.layer_norm(xt, (d,), gt, bt, eps=1e-8)
    assert np.abs(y.detach().numpy() - hl).max() < 1e-12
    slab = rng.standard_normal((3, cap, d)).astype(np.float32)
    dh = torch.from_numpy(ref.reduced_dh(slab)[:n])
    y.backward(dh)
    nparts = 2
    dx, part = ref.rows_bwd_ref(slab, rank, x, gamma, mu, rstd, nparts, d)
    assert np.abs(dx[idx[:n]] - xt.grad.numpy()).max() < 1e-10
    assert not dx[rank < 0].any()
    assert np.abs(part[:, 0].sum(0) - gt.grad.numpy()).max() < 1e-10
    assert np.abs(part[:, 1].sum(0) - bt.grad.numpy()).max() < 1e-10
