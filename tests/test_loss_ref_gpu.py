"""Kernel-level checks of loss.hip: rs_bce_fwd / rs_bce_bwd and rs_ce_fwd / rs_ce_bwd called through the C ABI, every
stored element held to the float64 reference (torch's own BCE-with-logits and cross entropy in float64) and the
derived bounds of tests/losshead_ref.py.  Outputs are pre-filled with NaN and followed by guard rows; pad columns of
a pitched output must survive."""
import math

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


def scalar(v, dt=F32):
    return None if v is None else torch.full((1,), v, dtype=dt, device=DEV)


# ------------------------------------------------------------------ BCE
@pytest.mark.parametrize("M", L.BCE_M)
@pytest.mark.parametrize("big", [False, True], ids=["unit", "large"])
def test_bce(M, big):
    """M = 65536 + 300 reaches past 256 workgroups x 256 threads: the grid-stride loop's second trip"""
    ops = _ops()
    inp = L.bce_inputs(M, DEV, big)
    if big:
        assert float(inp["pl"].abs().min()) > 100
    valid = inp["pos"] != 0
    for co in (None, 123.0):
        ws, out = L.Guarded(3 * 256), L.Guarded(4)
        ops.bce_fwd(inp["pl"], inp["nl"], inp["pos"], ws.t, out.t, count_override=scalar(co))
        torch.cuda.synchronize()
        out.check("out")
        assert torch.isnan(ws.full[3 * 256:]).all() and torch.isfinite(out.t).all()
        WORST.report("bce_fwd", (M, big, co), L.check_bce_fwd(inp, out.t, co))
    c = float(valid.sum())
    for count, dloss in ((c, None), (123.0, 0.37)):
        dpl, dnl = L.Guarded(M), L.Guarded(M)
        ops.bce_bwd(inp["pl"], inp["nl"], inp["pos"], scalar(count), scalar(dloss), dpl.t, dnl.t)
        torch.cuda.synchronize()
        dpl.check("dpl"), dnl.check("dnl")
        assert float(dpl.t[~valid].abs().sum()) == 0 and float(dnl.t[~valid].abs().sum()) == 0
        WORST.report("bce_bwd", (M, big, count, dloss),
                     L.check_bce_bwd(inp, count, 1.0 if dloss is None else dloss, dpl.t, dnl.t))


# ------------------------------------------------------------------ cross entropy over stored logits
@pytest.mark.parametrize("R", L.CE_R)
@pytest.mark.parametrize("V1", L.CE_V1)
@pytest.mark.parametrize("span", [False, True], ids=["unit", "span150"])
def test_ce(R, V1, span):
    """ldl > V1 with NaN in the input's pad columns, lddl > V1 with NaN pad columns that must survive; label-0 rows;
    rows_dev below R; fp32 and bf16 dlogits; V1 = 16384 + 77 exceeds 64 workgroups x 256: the backward's second trip"""
    ops = _ops()
    inp = L.ce_inputs(R, V1, DEV, ldl=V1 + 3, span=span)
    assert inp["logits"].stride(0) == V1 + 3
    for co, rows in ((None, None), (9.0, None), (None, R - 1)):
        if rows == 0:
            continue
        ws, out = L.Guarded(3 * R), L.Guarded(3)
        ops.ce_fwd(inp["logits"], inp["labels"], ws.t, out.t, count_override=scalar(co),
                   rows_dev=scalar(rows, torch.int32))
        torch.cuda.synchronize()
        ws.check("ws"), out.check("out")
        lse = ws.t[:R]
        if rows is not None:
            assert float(lse[rows:].abs().sum()) == 0 and float(ws.t[R + 2 * rows:].abs().sum()) == 0
        WORST.report("ce_fwd", (R, V1, span, co, rows), L.check_ce_fwd(inp, lse, out.t, co, rows))
        lab = L.ce_live(inp, rows)
        for dt in (F32, BF):
            count, dloss = (float(out.t[1]), None) if co is None else (co, 0.37)
            dl = L.Guarded(R, V1, dt, pitch=V1 + 5)
            ops.ce_bwd(inp["logits"], inp["labels"], scalar(count), scalar(dloss), ws.t, dl.t,
                       rows_dev=scalar(rows, torch.int32))
            torch.cuda.synchronize()
            dl.check("dlogits", written=rows)               # rows past rows_dev stay untouched
            n = R if rows is None else rows
            assert float(dl.t[:n][lab[:n] == 0].float().abs().sum()) == 0, "label-0 rows take no gradient"
            WORST.report("ce_bwd", (R, V1, span, co, rows, dt),
                         L.check_ce_bwd(inp, lse, count, 1.0 if dloss is None else dloss, dl.t, rows))
    assert not math.isnan(float(out.t[0]))
