"""CPU checks of tests/losshead_ref.py: the float32/bf16 emulation of every stage stays within the derived bounds (so
the bounds admit a correct kernel), and every planted mistake is rejected (ratio > 1) at the smallest shape of the
GPU tests' lists that exercises it.  No GPU, no native library."""
import math

import pytest
import torch
import torch.nn.functional as F

import losshead_ref as L

BF, F32 = torch.bfloat16, torch.float32
CPU = "cpu"


def ok(res):
    bad = {k: v for k, v in res.items() if not v <= 1.0 and k != "lse.ulps"}
    assert not bad, bad


def rejected(res, *keys):
    assert any(res[k] > 1.0 for k in keys), {k: res[k] for k in keys}


def keep_mask(inp, p, seed=5):
    return L.rand_mask(torch.Generator().manual_seed(seed), CPU, inp["ids"].numel(), inp["d"], p)


# ------------------------------------------------------------------ embedding
@pytest.mark.parametrize("dt", [BF, F32])
@pytest.mark.parametrize("mode,p", [(0, 0.0), (0, 0.2), (1, 0.2)])
def test_embed_fwd_emulation_and_mutation(dt, mode, p):
    for d in L.EMBED_FWD_D:
        for B in L.EMBED_B:
            inp = L.embed_inputs(dt, d, B, L.EMBED_T, CPU)
            keep = keep_mask(inp, p)
            ok(L.check_embed_fwd(mode, inp, keep, p, L.emu_embed_fwd(mode, inp, keep, p)))
    # the smallest shape: one sequence of T rows at d = 50, whose first id is 0
    inp = L.embed_inputs(dt, 50, 1, L.EMBED_T, CPU)
    keep = keep_mask(inp, p)
    if mode == 0:
        rejected(L.check_embed_fwd(0, inp, keep, p, L.emu_embed_fwd(0, inp, keep, p, mut="nozero")), "x")


@pytest.mark.parametrize("dt,d", list(L.POS_FORMS))
def test_embed_bwd_emulation(dt, d):
    rg = L.POS_FORMS[(dt, d)][1]
    for nb in L.pos_batches(rg):
        for mode, p, acc in ((0, 0.0, False), (0, 0.2, True), (1, 0.2, False)):
            inp = L.embed_inputs(dt, d, nb, L.POS_T, CPU)
            keep = keep_mask(inp, p)
            dtab, dpos = L.emu_embed_bwd(mode, inp, keep, p, acc)
            ok(L.check_embed_bwd(mode, inp, keep, p, dtab, dpos, acc))


@pytest.mark.parametrize("mut,key,p", [("lastbatch", "dpos", 0.0), ("maskrow", "dpos", 0.2), ("noscale", "dtable", 0.0),
                                       ("row0", "dtable.row0", 0.0)])
def test_embed_bwd_mutations(mut, key, p):
    """at the smallest case that has them: fp32 d = 50 (the fallback form, RG = 4) with nb = RG - 1 = 3 sequences
    (the batch sum has a last element and a wrong row's mask exists); scale and row 0 at nb = 1"""
    nb = 1 if mut in ("noscale", "row0") else L.pos_batches(L.POS_FORMS[(F32, 50)][1])[1]
    inp = L.embed_inputs(F32, 50, nb, L.POS_T, CPU)
    keep = keep_mask(inp, p)
    dtab, dpos = L.emu_embed_bwd(0, inp, keep, p, False, mut=mut)
    rejected(L.check_embed_bwd(0, inp, keep, p, dtab, dpos, False), key)


def test_embed_bwd_zipf_table():
    """hundreds of contributions to one table row: the emulation's index_add order against the per-row K"""
    g = torch.Generator().manual_seed(3)
    inp = L.embed_inputs(F32, 64, 400, 5, CPU, V=50)
    inp["ids"] = L.zipf_ids(g, CPU, 2000, 50)
    assert int(torch.bincount(inp["ids"])[1:].max()) >= 200
    keep = keep_mask(inp, 0.2)
    dtab, dpos = L.emu_embed_bwd(0, inp, keep, 0.2)
    ok(L.check_embed_bwd(0, inp, keep, 0.2, dtab, dpos))


@pytest.mark.parametrize("dt", [BF, F32])
def test_sampled_logits_emulation_and_tail(dt):
    for d in L.SAMPLED_D:
        for M in L.SAMPLED_M:
            inp = L.sampled_inputs(dt, d, M, CPU)
            ok(L.check_sampled_fwd(inp, *L.emu_sampled_fwd(inp)))
            for acc in (False, True):
                df, dE = L.emu_sampled_bwd(inp, acc)
                ok(L.check_sampled_bwd(inp, df, dE, acc))
    for d in (50, 200):                                     # the last d % 64 features dropped, at M = 1
        inp = L.sampled_inputs(dt, d, 1, CPU)
        rejected(L.check_sampled_fwd(inp, *L.emu_sampled_fwd(inp, mut="tail")), "pl", "nl")


@pytest.mark.parametrize("dt", [BF, F32])
def test_candidate_scores_emulation_and_tail(dt):
    for d in L.CAND_D:
        for B in L.CAND_B:
            for C_ in L.CAND_C:
                inp = L.cand_inputs(dt, d, B, C_, CPU)
                ok(L.check_cand(inp, L.emu_cand(inp)))
    inp = L.cand_inputs(dt, 50, 1, 1, CPU)
    rejected(L.check_cand(inp, L.emu_cand(inp, mut="tail")), "scores")


# ------------------------------------------------------------------ head
@pytest.mark.parametrize("d", L.HEAD_D)
def test_head_emulation(d):
    for M in L.HEAD_M:
        for zeros, esc in ((0.3, 1.0), (1.0, 1.0), (0.3, 300.0)):
            if M == L.HEAD_M[-1] and (zeros == 1.0 or d != 64):
                continue                                    # the long case once per variant is enough on the CPU
            inp = L.head_inputs(d, M, CPU, zeros, esc)
            fw = L.emu_head_fwd(inp)
            ok(L.check_head_fwd(inp, fw))
            for div in (None, 77.0):
                ok(L.check_head_bwd(inp, fw, L.emu_head_bwd(inp, fw, div), div))
            ok(L.check_head_bwd(inp, fw, L.emu_head_bwd(inp, fw, None, grads_in=True), None, grads_in=True))


def test_head_large_logits_and_all_padding():
    inp = L.head_inputs(64, 65, CPU, 0.3, 300.0)
    fw = L.emu_head_fwd(inp)
    assert float(fw["pl"].abs().max()) > 100 and float(fw["nl"].abs().max()) > 100
    assert torch.isfinite(fw["part"]).all()
    inp = L.head_inputs(64, 65, CPU, 1.0)
    fw = L.emu_head_fwd(inp)
    bw = L.emu_head_bwd(inp, fw)
    assert all(float(bw[k].float().abs().max()) == 0 for k in ("dpl", "dnl", "dx", "lnpart"))
    assert float(bw["out"][1]) == 0 and math.isnan(float(bw["out"][2]))


@pytest.mark.parametrize("mut,keys,div", [("statblk", ("out", "out.count"), None), ("lnblk", ("lnpart.b/blk",), None),
                                          ("nodivisor", ("out", "dpl"), 77.0)])
def test_head_mutations(mut, keys, div):
    """M = 65: the smallest row count with a second 64-row block; the divisor at M = 1"""
    M = 1 if mut == "nodivisor" else 65
    inp = L.head_inputs(64, M, CPU)
    fw = L.emu_head_fwd(inp)
    res = L.check_head_bwd(inp, fw, L.emu_head_bwd(inp, fw, div, mut=mut), div)
    rejected(res, *keys)
    if mut == "lnblk":
        rejected(res, "lnpart.b"), rejected(res, "lnpart.g/blk")


# ------------------------------------------------------------------ BCE
def test_bce_emulation():
    for M in L.BCE_M:
        for big in (False, True):
            inp = L.bce_inputs(M, CPU, big)
            for co in (None, 123.0):
                ok(L.check_bce_fwd(inp, L.emu_bce_fwd(inp, co), co))
            c = max(float((inp["pos"] != 0).sum()), 1.0)
            for dl in (1.0, 0.37):
                ok(L.check_bce_bwd(inp, c, dl, *L.emu_bce_bwd(inp, c, dl)))


@pytest.mark.parametrize("mut,key", [("negsign", "neg"), ("padcount", "mean"), ("nooverride", "mean")])
def test_bce_fwd_mutations(mut, key):
    """M = 255 (the smallest with padded rows; M = 1 has one valid row and nothing to miscount)"""
    M = 1 if mut == "negsign" else 255
    inp = L.bce_inputs(M, CPU)
    co = 123.0 if mut == "nooverride" else None
    rejected(L.check_bce_fwd(inp, L.emu_bce_fwd(inp, co, mut=mut), co), key)


def test_bce_bwd_dloss_ignored():
    inp = L.bce_inputs(1, CPU)
    rejected(L.check_bce_bwd(inp, 1.0, 0.37, *L.emu_bce_bwd(inp, 1.0, 0.37, mut="nodloss")), "dpl", "dnl")


# ------------------------------------------------------------------ cross entropy over stored logits
def test_ce_reference_is_autograd():
    """the staged gradient formula equals autograd through F.cross_entropy when fed the exact log-sum-exp"""
    inp = L.ce_inputs(5, 257, CPU)
    x = inp["logits"].double().requires_grad_()
    (F.cross_entropy(x, inp["labels"], ignore_index=0, reduction="sum") * 0.37 / 3.0).backward()
    r = L.ref_ce_grad(x.detach(), inp["labels"], torch.logsumexp(x.detach(), 1), 3.0, 0.37)
    assert torch.allclose(r, x.grad, rtol=1e-12, atol=1e-15)


def test_ce_emulation():
    for R in L.CE_R:
        for V1 in L.CE_V1:
            for span in (False, True):
                inp = L.ce_inputs(R, V1, CPU, ldl=V1 + 3, span=span)
                for co, rows in ((None, None), (9.0, None), (None, R - 1)):
                    if rows == 0:
                        continue
                    lse, out = L.emu_ce_fwd(inp, co, rows)
                    ok(L.check_ce_fwd(inp, lse, out, co, rows))
                    for dt in (F32, BF):
                        ok(L.check_ce_bwd(inp, lse, 4.0, 0.37, L.emu_ce_bwd(inp, lse, 4.0, 0.37, dt), rows))


def test_ce_mutations():
    """R = 1, V1 = 7 for the one-hot and dloss; R = 5 (the smallest with a label-0 row) for that row's gradient; the
    row spanning +-150 for the missing max subtraction"""
    inp = L.ce_inputs(1, 7, CPU)
    lse, _ = L.emu_ce_fwd(inp)
    for mut in ("onehot+1", "nodloss"):
        rejected(L.check_ce_bwd(inp, lse, 4.0, 0.37, L.emu_ce_bwd(inp, lse, 4.0, 0.37, mut=mut)), "dlogits")
    inp = L.ce_inputs(5, 7, CPU)
    lse, _ = L.emu_ce_fwd(inp)
    rejected(L.check_ce_bwd(inp, lse, 4.0, 0.37, L.emu_ce_bwd(inp, lse, 4.0, 0.37, mut="lab0grad")), "dlogits")
    inp = L.ce_inputs(1, 7, CPU, span=True)
    lse, out = L.emu_ce_fwd(inp, mut="nomax")
    rejected(L.check_ce_fwd(inp, lse, out), "lse")


# ------------------------------------------------------------------ vocabulary head
@pytest.mark.parametrize("d,R,V1", [(64, 37, 200), (96, 37, 200), (256, 130, 200), (96, 130, 20000), (64, 37, 70001)])
def test_vocab_ce_emulation(d, R, V1):
    inp = L.vce_inputs(d, R, V1, CPU, bias=d != 96)
    logits = L.vce_logits(inp)
    for co, rows in ((None, None), (11.0, R - 5)):
        lse, out, x = L.emu_vce_fwd(inp, co, rows)
        ok(L.check_vce_fwd(inp, lse, out, co, rows, logits=logits))
        ok(L.check_vce_bwd(inp, lse, 9.0, 0.37, L.emu_vce_bwd(inp, x, lse, 9.0, 0.37, rows), rows, logits=logits))


def test_vocab_ce_tile_dropped():
    """V1 = 200: two tiles, the smallest fold"""
    inp = L.vce_inputs(64, 37, 200, CPU)
    lse, out, _ = L.emu_vce_fwd(inp, mut="tile")
    rejected(L.check_vce_fwd(inp, lse, out), "lse")


# ------------------------------------------------------------------ rows
def test_rows_reference():
    lab = torch.tensor([0, 4, 0, 0, 9, 2, 0, 1])
    idx, rank, cnt = L.ref_compact(lab, 6)
    assert cnt == 4 and idx.tolist() == [1, 4, 5, 7, -1, -1] and rank.tolist() == [-1, 0, -1, -1, 1, 2, -1, 3]
    src = torch.arange(16.0).view(8, 2)
    dst, lo = L.ref_gather(src, lab, idx, cnt, 6)
    assert dst[:4].tolist() == src[[1, 4, 5, 7]].tolist() and float(dst[4:].abs().sum()) == 0
    assert lo.tolist() == [4, 9, 2, 1, 0, 0]
    back = L.ref_scatter(dst, rank)
    assert torch.equal(back, src * (lab != 0)[:, None])
    idx, rank, cnt = L.ref_compact(lab, 3)                  # cap below the count: the rest ranks -1
    assert cnt == 3 and rank.tolist() == [-1, 0, -1, -1, 1, 2, -1, -1]
