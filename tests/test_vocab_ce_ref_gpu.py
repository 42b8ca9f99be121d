"""Kernel-level checks of vocab_ce.hip: rs_vocab_ce_fwd / rs_vocab_ce_bwd (the GEMM-epilogue vocabulary head: the path
of every bf16 width the tile-stationary head does not take, e.g. d = 96) called through the C ABI.  The per-row
log-sum-exp, the loss sum / count / mean and every element of dlogits are held to the float64 reference and the bounds
of tests/losshead_ref.py; the backward is checked staged, from the log-sum-exp the forward stored.

R = 37, 130: below and across one 128-row tile.  V1 = 200, 20000, 70001: 2 tiles (fewer than a wave), 157 tiles (the
tail loop only) and 547 tiles (one unrolled 8-deep fold plus a tail on lanes 0..34).  At d = 64, 256 the result is
also compared with rs_vocab_head_fwd / _bwd on the same inputs, within the sum of the two bounds (on top of the
float64 check, never instead of it).

The module prints the worst |lse_hip - lse_fp64| in units of 2^-24 max(|lse|, 1): the measurement behind
losshead_ref.MEASURED_FAST_ULPS."""
import pytest
import torch

import losshead_ref as L

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
    print(f"worst lse error over the cases: {WORST.get(('vocab_ce_fwd', 'lse.ulps'), 0.0):.3f} x 2^-24 max(|lse|, 1)"
          f"  (MEASURED_FAST_ULPS = {L.MEASURED_FAST_ULPS}, factor {L.FAST_FACTOR})")


def scalar(v, dt=F32):
    return None if v is None else torch.full((1,), v, dtype=dt, device=DEV)


def run(fwd, bwd, inp, co, rows, dloss, pads_zero_ok=False):
    """forward + backward of one of the two heads -> (lse, out, dl, count)"""
    ops = _ops()
    R, V1 = inp["R"], inp["V1"]
    ntn = -(-V1 // 128)
    n = ops.vocab_ce_ws_numel(R, V1)
    ws, out = L.Guarded(n), L.Guarded(3)
    rd = scalar(rows, torch.int32)
    fwd(inp["h"], inp["E"], inp["bias"], inp["labels"], ws.t, out.t, rows_dev=rd, count_override=scalar(co))
    torch.cuda.synchronize()
    out.check("out")
    assert torch.isnan(ws.full[n:]).all(), "store past the workspace"
    lse = ws.t[R * ntn * 2 + R: R * ntn * 2 + 2 * R]
    count = float(out.t[1]) if co is None else co
    dl = L.Guarded(R, V1, BF, pitch=-(-V1 // 8) * 8)
    bwd(inp["h"], inp["E"], inp["bias"], inp["labels"], ws.t, scalar(count), dl.t, rows_dev=rd, dloss=scalar(dloss))
    torch.cuda.synchronize()
    dl.check("dlogits", written=rows, pads_zero_ok=pads_zero_ok)
    return lse, out.t, dl.t, count


@pytest.mark.parametrize("d", L.VCE_D)
@pytest.mark.parametrize("R", L.VCE_R)
@pytest.mark.parametrize("V1", L.VCE_V1)
def test_vocab_ce(d, R, V1):
    ops = _ops()
    # (bias, count_override, rows_dev, dloss): the plain call, then every option at once
    for bias, co, rows, dloss in ((True, None, None, None), (False, 11.0, R - 5, 0.37)):
        inp = L.vce_inputs(d, R, V1, DEV, bias=bias)
        assert int((inp["labels"] == 0).sum()) > 0
        logits = L.vce_logits(inp)
        lse, out, dl, count = run(ops.vocab_ce_fwd, ops.vocab_ce_bwd, inp, co, rows, dloss)
        key = (d, R, V1, bias, co, rows, dloss)
        assert not torch.isnan(lse).any()
        WORST.report("vocab_ce_fwd", key, L.check_vce_fwd(inp, lse, out, co, rows, logits=logits))
        dl_ = 1.0 if dloss is None else dloss
        WORST.report("vocab_ce_bwd", key, L.check_vce_bwd(inp, lse, count, dl_, dl, rows, logits=logits))
        lab = L.ce_live(inp, rows)
        n = R if rows is None else rows
        assert float(lse[lab == 0].abs().sum()) == 0, "label-0 rows and rows past rows_dev: lse = 0"
        assert float(dl[:n][lab[:n] == 0].float().abs().sum()) == 0, "label-0 rows take no gradient"
        if d in (64, 256):
            assert ops.vocab_head_supported(d)
            # (rs_vocab_head_bwd's 16-byte stores may zero a written row's pad columns up to lddl: its contract)
            lse2, out2, dl2, count2 = run(ops.vocab_head_fwd, ops.vocab_head_bwd, inp, co, rows, dloss,
                                          pads_zero_ok=True)
            assert count2 == count
            zero = torch.zeros_like(lse)
            WORST.report("vocab_ce|vocab_head", key,
                         L.vce_cross(inp, logits, torch.where(lab != 0, lse, zero), torch.where(lab != 0, lse2, zero),
                                     dl, dl2, count, dl_, rows))
