"""Kernel-level checks of rows.hip: rs_gather_rows / rs_scatter_rows (copies: held to equality, with the index from
rs_compact_rows) and rs_candidate_scores (held to the float64 reference and derived bound of tests/losshead_ref.py),
called through the C ABI.  Outputs are pre-filled with NaN (integers: a sentinel) and followed by guard rows; source
and destination pitches are wider than the row and the pad columns must survive."""
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


def compact(labels, cap):
    ops = _ops()
    n = labels.numel()
    idx, rank, count = L.Guarded(cap, dt=torch.int32), L.Guarded(n, dt=torch.int32), L.Guarded(1, dt=torch.int32)
    ops.compact_rows(labels, cap, idx.t, rank.t, count.t)
    torch.cuda.synchronize()
    idx.check("idx"), rank.check("rank"), count.check("count")
    ri, rr, rc = L.ref_compact(labels, cap)
    assert int(count.t[0]) == rc and torch.equal(rank.t, rr) and torch.equal(idx.t, ri)
    return idx.t, rank.t, count.t, rc


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("d", L.ROWS_D)
@pytest.mark.parametrize("n", L.ROWS_N)
def test_gather_scatter_rows(dt, d, n):
    """n around the 1024-row block of rs_compact_rows; cap above the count (zero rows and label 0 there), cap below it
    (the rows left out rank -1 and scatter back as zeros), an all-zero label vector"""
    ops = _ops()
    g = L.gen_for(DEV, 37, d, n)
    src = L.rn(g, DEV, n, d + 8, dt=dt)[:, :d]
    labels = torch.randint(1, 90, (n,), generator=g, device=DEV)
    labels[torch.rand(n, generator=g, device=DEV) < 0.6] = 0
    for lab, cap in ((labels, n), (labels, max(1, int((labels != 0).sum()) // 2)), (torch.zeros_like(labels), n)):
        idx, rank, count, cnt = compact(lab, cap)
        dst, lab_out = L.Guarded(cap, d, dt, pitch=d + 8), L.Guarded(cap, dt=torch.int64)
        ops.gather_rows(src, idx, count, cap, dst.t, labels=lab, lab_out=lab_out.t)
        torch.cuda.synchronize()
        dst.check("dst"), lab_out.check("lab_out")
        rd, rl = L.ref_gather(src, lab, idx, cnt, cap)
        assert torch.equal(dst.t, rd) and torch.equal(lab_out.t, rl)
        assert float(dst.t[cnt:].float().abs().sum()) == 0 and int(lab_out.t[cnt:].abs().sum()) == 0
        nolab = L.Guarded(cap, d, dt, pitch=d + 8)          # labels / lab_out are optional
        ops.gather_rows(src, idx, count, cap, nolab.t)
        back = L.Guarded(n, d, dt, pitch=d + 8)
        ops.scatter_rows(dst.t, rank, back.t)
        torch.cuda.synchronize()
        nolab.check("dst"), back.check("scattered")
        assert torch.equal(nolab.t, rd)
        assert torch.equal(back.t, L.ref_scatter(rd, rank))
        live = rank >= 0
        assert torch.equal(back.t[live], src[live]) and float(back.t[~live].float().abs().sum()) == 0


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("d", L.CAND_D)
def test_candidate_scores(dt, d):
    """one wave per (row, candidate), lanes strided over d (50: one trip with a tail, 300: five with a tail); ldh > d;
    an id equal to V or negative scores NaN, and only there"""
    from rbm_amd import _lib
    ops = _ops()
    for B in L.CAND_B:
        for C_ in L.CAND_C:
            for bias in (True, False):
                inp = L.cand_inputs(dt, d, B, C_, DEV, bias=bias)
                assert inp["h"].stride(0) > d
                out = ops.candidate_scores(inp["h"], inp["E"], inp["cand"], bias=inp["bias"])
                torch.cuda.synchronize()
                WORST.report("candidate_scores", (dt, d, B, C_, bias), L.check_cand(inp, out))
                # the C ABI itself with ids outside [0, V)
                cand, V = inp["cand"].clone(), inp["V"]
                bad = torch.zeros_like(cand, dtype=torch.bool)
                bad.view(-1)[0] = True
                cand.view(-1)[0] = V
                if B * C_ > 1:
                    bad.view(-1)[-1] = True
                    cand.view(-1)[-1] = -1
                raw = L.Guarded(B, C_, F32)
                _lib.call("rs_candidate_scores", ops.dtype_code(inp["h"]), _lib.ptr(inp["h"]), inp["h"].stride(0), B, d,
                          _lib.ptr(inp["E"]), _lib.ptr(inp["bias"]), _lib.ptr(cand), C_, V, _lib.ptr(raw.t),
                          _lib.stream())
                torch.cuda.synchronize()
                assert torch.isnan(raw.full[B:]).all(), "store past the rows"
                assert torch.equal(torch.isnan(raw.t), bad), "NaN exactly at the ids outside [0, V)"
                # everywhere else the scores of the valid ids (at the NaN places: the first call's)
                WORST.report("candidate_scores", (dt, d, B, C_, bias, "raw"),
                             L.check_cand(inp, torch.where(bad, out, raw.t)))
