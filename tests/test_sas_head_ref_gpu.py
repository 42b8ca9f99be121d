"""Kernel-level checks of head.hip: rs_sas_head_fwd, rs_sas_head_bwd and rs_sas_head_finish called through the C
ABI, every stored element held to the float64 reference and derived bound of tests/losshead_ref.py.  The backward is
checked staged: it is fed the pl, nl, mean, rstd and part the forward kernel stored.

d = 64, 128, 256 (2, 4 and 8 rows per thread); M = 1, 63, 64, 65, 64*3 + 17 and 64*257 + 5 (258 block partials: the
statistics loop's second trip).  Outputs are pre-filled with NaN and followed by guard rows."""
import pytest
import torch

import losshead_ref as L
from rowchain_ref import EPS

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DEV = "cuda"
WORST = L.Worst()


def _ops():
    from rbm_amd import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    WORST.dump()


def run_fwd(inp):
    ops = _ops()
    M, d = inp["M"], inp["d"]
    nblk = -(-M // L.RB)
    b = {"f": L.Guarded(M, d, BF), "mean": L.Guarded(M), "rstd": L.Guarded(M), "pl": L.Guarded(M), "nl": L.Guarded(M),
         "part": L.Guarded(nblk, 3)}
    ops.sas_head_fwd(inp["x"], inp["g"], inp["b"], EPS, b["f"].t, b["mean"].t, b["rstd"].t, inp["E"], inp["pos"],
                     inp["neg"], b["pl"].t, b["nl"].t, b["part"].t)
    torch.cuda.synchronize()
    for k, v in b.items():
        v.check(k)
    return {k: v.t for k, v in b.items()}


def check_stats_written(out):
    """out[0..3] written, nothing past them (out[2] may itself be NaN: the mean over no valid row)"""
    assert not torch.isnan(out.t[[0, 1, 3]]).any() and torch.isnan(out.full[4:]).all(), "out[0..3]"


def run_bwd(inp, fw, divisor=None, grads_in=False):
    ops = _ops()
    M, d = inp["M"], inp["d"]
    nblk = -(-M // L.RB)
    b = {"out": L.Guarded(4), "dpl": L.Guarded(M), "dnl": L.Guarded(M), "dx": L.Guarded(M, d, BF),
         "lnpart": L.Guarded(nblk, 2 * d)}
    div = None if divisor is None else torch.full((1,), divisor, dtype=F32, device=DEV)
    part0 = fw["part"].clone()
    ops.sas_head_bwd(fw["part"], div, b["out"].t, fw["pl"], fw["nl"], inp["dpl_in"] if grads_in else None,
                     inp["dnl_in"] if grads_in else None, b["dpl"].t, b["dnl"].t, inp["pos"], inp["neg"], inp["E"],
                     inp["x"], inp["g"], fw["mean"], fw["rstd"], b["dx"].t, b["lnpart"].t)
    torch.cuda.synchronize()
    assert torch.equal(fw["part"], part0), "the forward's partials are an input"
    for k, v in b.items():
        if grads_in and k in ("out", "dpl", "dnl"):
            v.untouched(k)                                  # the caller's gradients: no statistics, no dpl / dnl
        elif k == "out":
            check_stats_written(v)
        else:
            v.check(k)
    out = {k: v.t for k, v in b.items()}
    out["lnpart"] = out["lnpart"].view(nblk, 2, d)
    return out


def finish(part, divisor=None):
    ops = _ops()
    out = L.Guarded(4)
    div = None if divisor is None else torch.full((1,), divisor, dtype=F32, device=DEV)
    ops.sas_head_finish(part, div, out.t)
    torch.cuda.synchronize()
    check_stats_written(out)
    return out.t


@pytest.mark.parametrize("d", L.HEAD_D)
@pytest.mark.parametrize("M", L.HEAD_M)
def test_head_fwd_bwd(d, M):
    """pos about 30 % zeros; both divisors (the forward's count, a device divisor different from it); both gradient
    sources; rs_sas_head_finish on the forward's partials equals the backward's statistics bit for bit"""
    inp = L.head_inputs(d, M, DEV)
    fw = run_fwd(inp)
    WORST.report("sas_head_fwd", (d, M), L.check_head_fwd(inp, fw))
    for div in (None, 77.0):
        bw = run_bwd(inp, fw, div)
        WORST.report("sas_head_bwd", (d, M, div), L.check_head_bwd(inp, fw, bw, div))
        valid = inp["pos"] != 0
        assert float(bw["dpl"][~valid].abs().sum()) == 0 and float(bw["dnl"][~valid].abs().sum()) == 0
        fin = finish(fw["part"], div)
        assert torch.equal(fin, bw["out"]), (fin, bw["out"])
        WORST.report("sas_head_finish", (d, M, div), L.check_head_stats(fw["part"], div, fin))
    bw = run_bwd(inp, fw, None, grads_in=True)
    WORST.report("sas_head_bwd", (d, M, "grads in"), L.check_head_bwd(inp, fw, bw, None, grads_in=True))


@pytest.mark.parametrize("d", L.HEAD_D)
def test_head_large_logits(d):
    """|pl|, |nl| past 100 (E scaled): finite softplus sums, the sigmoid terms at their 0 and -1/count limits"""
    inp = L.head_inputs(d, 64 * 3 + 17, DEV, escale=300.0)
    fw = run_fwd(inp)
    assert float(fw["pl"].abs().max()) > 100 and float(fw["nl"].abs().max()) > 100
    assert torch.isfinite(fw["part"]).all()
    WORST.report("sas_head_fwd", (d, "large"), L.check_head_fwd(inp, fw))
    bw = run_bwd(inp, fw)
    assert all(torch.isfinite(bw[k].float()).all() for k in bw)
    WORST.report("sas_head_bwd", (d, "large"), L.check_head_bwd(inp, fw, bw))
    c = float(bw["out"][1])
    valid = inp["pos"] != 0
    hi, lo = valid & (fw["pl"] > 100), valid & (fw["pl"] < -100)
    ulp = 2.0 ** -23 / c                                    # the scale 1 / count is one float32 division
    assert float(bw["dpl"][hi].abs().sum()) == 0 and bool(((bw["dpl"][lo].double() + 1.0 / c).abs() <= ulp).all())
    hi, lo = valid & (fw["nl"] > 100), valid & (fw["nl"] < -100)
    assert bool(((bw["dnl"][hi].double() - 1.0 / c).abs() <= ulp).all()) and float(bw["dnl"][lo].abs().sum()) == 0


@pytest.mark.parametrize("d", L.HEAD_D)
@pytest.mark.parametrize("M", [65, 64 * 3 + 17])
def test_head_all_padding(d, M):
    """no valid row: every gradient exactly zero without a NaN, count 0, and the mean loss 0 / 0 = NaN as
    include/recsys_hip.h states (the reference's mean over an empty selection); with a divisor it is 0"""
    inp = L.head_inputs(d, M, DEV, zeros=1.0)
    assert int((inp["pos"] != 0).sum()) == 0
    fw = run_fwd(inp)
    WORST.report("sas_head_fwd", (d, M, "all padding"), L.check_head_fwd(inp, fw))
    assert float(fw["part"].abs().sum()) == 0
    for div in (None, 77.0):
        bw = run_bwd(inp, fw, div)
        for k in ("dpl", "dnl", "dx", "lnpart"):
            assert not torch.isnan(bw[k].float()).any() and float(bw[k].float().abs().max()) == 0, k
        assert float(bw["out"][0]) == 0 and float(bw["out"][1]) == 0 and float(bw["out"][3]) == 0
        assert torch.isnan(bw["out"][2]) if div is None else float(bw["out"][2]) == 0
        fin = finish(fw["part"], div)
        assert torch.equal(fin.isnan(), bw["out"].isnan()) and torch.equal(fin.nan_to_num(), bw["out"].nan_to_num())
        WORST.report("sas_head_bwd", (d, M, "all padding", div), L.check_head_bwd(inp, fw, bw, div))
