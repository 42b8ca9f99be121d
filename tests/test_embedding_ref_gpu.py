"""Kernel-level checks of embedding.hip: rs_embed_fwd, rs_embed_bwd (positional sum in all four launch forms, table
scatter by float atomics), rs_sampled_logits_fwd / _bwd, each called through the C ABI and every stored element held
to the float64 reference and derived bound of tests/losshead_ref.py.  Dropout keep masks come from the kernels' own
hash (rs_dropout_rowmask, anchored by test_dropout_hash_gpu.py).

Every output is pre-filled with NaN and followed by guard rows: no NaN may remain below the row count and nothing
may be stored past it.  The module prints its worst err / bound per kernel and tensor; any ratio above 1 fails."""
import pytest
import torch

import losshead_ref as L

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
SALT, SEED = 0x1234_5678_9ABC_DEF1, 977
DEV = "cuda"
WORST = L.Worst()


def _ops():
    from rbm_amd import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    WORST.dump()


def _sb():
    return torch.full((1,), SEED, dtype=torch.int64, device=DEV)


def _mask(rows, d, p, sb):
    """keep mask of the dropout site with element index r*d + c (the kernels' own hash, through the C ABI)"""
    ops = _ops()
    if p == 0:
        return torch.ones(rows, d, dtype=torch.bool, device=DEV)
    ones = torch.ones(rows, d, dtype=F32, device=DEV)
    out = torch.empty_like(ones)
    ops.dropout_rowmask(ones, p, SALT, sb, None, out)
    return out > 0


def _offset(t):
    """the same values at a base one element past a 16-byte boundary"""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)[1:]
    flat.copy_(t.reshape(-1))
    return flat.view(t.shape)


# ------------------------------------------------------------------ rs_embed_fwd
@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_embed_fwd(dt, mode, p):
    ops = _ops()
    sb = _sb()
    # d = 64, 128: the 16-byte vector path; 50: any width; 64 with the table or the output one element off 16 bytes
    for d, off in [(d, None) for d in L.EMBED_FWD_D] + [(64, "table"), (64, "out")]:
        for B in L.EMBED_B:
            inp = L.embed_inputs(dt, d, B, L.EMBED_T, DEV)
            rows = B * L.EMBED_T
            assert int((inp["ids"] == 0).sum()) > 0
            keep = _mask(rows, d, p, sb)
            out = L.Guarded(rows, d, dt, offset=1 if off == "out" else 0)
            table = _offset(inp["table"]) if off == "table" else inp["table"]
            assert (table.data_ptr() % 16 != 0) == (off == "table") and (out.t.data_ptr() % 16 != 0) == (off == "out")
            ops.embed_fwd(mode, inp["ids"], L.EMBED_T, table, inp["ptab"], inp["scale"], p, SALT, sb, out.t)
            torch.cuda.synchronize()
            out.check("out")
            if mode == 0:
                assert float(out.t[inp["ids"] == 0].float().abs().max()) == 0, "padded rows must be exactly zero"
            WORST.report("embed_fwd", (dt, mode, p, d, off, B), L.check_embed_fwd(mode, inp, keep, p, out.t))


# ------------------------------------------------------------------ rs_embed_bwd: the positional sum
@pytest.mark.parametrize("dt,d", list(L.POS_FORMS),
                         ids=[f"{'bf16' if t == BF else 'fp32'}-{d}" for t, d in L.POS_FORMS])
def test_embed_bwd_pos(dt, d):
    """<16, 512>, <32>, <64> and the fallback kernel; nb = 1, RG - 1 and RG U + 3 sequences (the last runs the 8-row
    unrolled loop a second time with its clamped out-of-range rows)"""
    ops = _ops()
    sb = _sb()
    rg = L.POS_FORMS[(dt, d)][1]
    T = L.POS_T
    for nb in L.pos_batches(rg):
        inp = L.embed_inputs(dt, d, nb, T, DEV)
        assert inp["dx"].data_ptr() % 16 == 0
        for mode, p, acc in ((0, 0.0, False), (0, 0.2, True), (1, 0.2, False), (1, 0.0, True)):
            keep = _mask(nb * T, d, p, sb)
            dpos = L.Guarded(T, d, F32)
            if acc:
                dpos.t.copy_(inp["dpos0"])
            ops.embed_bwd(mode, inp["ids"], T, inp["dx"], inp["scale"], p, SALT, sb, None, dpos.t, accumulate_pos=acc)
            torch.cuda.synchronize()
            dpos.check("dpos")
            WORST.report("embed_bwd", (dt, d, nb, mode, p, acc),
                         L.check_embed_bwd(mode, inp, keep, p, None, dpos.t, acc))


@pytest.mark.parametrize("dt,d", [(BF, 128), (F32, 64)], ids=["bf16-128", "fp32-64"])
def test_embed_bwd_pos_misaligned_dx(dt, d):
    """dx one element off a 16-byte boundary: the fallback kernel at a width the vector forms would take"""
    ops = _ops()
    sb = _sb()
    T, nb, p = L.POS_T, 35, 0.2
    inp = L.embed_inputs(dt, d, nb, T, DEV)
    inp["dx"] = _offset(inp["dx"])
    assert inp["dx"].data_ptr() % 16 != 0
    keep = _mask(nb * T, d, p, sb)
    dpos = L.Guarded(T, d, F32)
    ops.embed_bwd(0, inp["ids"], T, inp["dx"], inp["scale"], p, SALT, sb, None, dpos.t, accumulate_pos=False)
    torch.cuda.synchronize()
    dpos.check("dpos")
    WORST.report("embed_bwd", (dt, d, "dx off"), L.check_embed_bwd(0, inp, keep, p, None, dpos.t, False))


# ------------------------------------------------------------------ rs_embed_bwd: the table scatter
@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("d", [64, 50])
def test_embed_bwd_table_zipf(dt, d):
    """Zipf ids: one table row takes hundreds of atomic contributions; row 0 stays bit for bit; dtable = None and
    dpos = None each launch only the other half"""
    ops = _ops()
    sb = _sb()
    V, T, B = 50, 5, 400
    inp = L.embed_inputs(dt, d, B, T, DEV, V=V)
    inp["ids"] = L.zipf_ids(L.gen_for(DEV, 3, d), DEV, B * T, V)
    assert int(torch.bincount(inp["ids"])[1:].max()) >= 200 and int((inp["ids"] == 0).sum()) > 0
    for mode, p in ((0, 0.0), (0, 0.2), (1, 0.2)):
        keep = _mask(B * T, d, p, sb)
        dtable, dpos = L.Guarded(V, d, F32), L.Guarded(T, d, F32)
        dtable.t.copy_(inp["dtable0"])
        ops.embed_bwd(mode, inp["ids"], T, inp["dx"], inp["scale"], p, SALT, sb, dtable.t, None)
        torch.cuda.synchronize()
        dtable.check("dtable"), dpos.untouched("dpos")
        WORST.report("embed_bwd", (dt, d, "zipf", mode, p), L.check_embed_bwd(mode, inp, keep, p, dtable.t, None))
        both = L.Guarded(V, d, F32)
        both.t.copy_(inp["dtable0"])
        ops.embed_bwd(mode, inp["ids"], T, inp["dx"], inp["scale"], p, SALT, sb, both.t, dpos.t, accumulate_pos=False)
        torch.cuda.synchronize()
        both.check("dtable"), dpos.check("dpos")
        WORST.report("embed_bwd", (dt, d, "zipf both", mode, p),
                     L.check_embed_bwd(mode, inp, keep, p, both.t, dpos.t, False))


# ------------------------------------------------------------------ rs_sampled_logits_fwd / _bwd
@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("d", L.SAMPLED_D)
def test_sampled_logits(dt, d):
    """one wave per row, lanes strided over d: 1 trip with a tail (50), exactly 1 (64), 4 with a tail (200); M = 1,
    a full workgroup of 4 rows, one more, and 259"""
    ops = _ops()
    for M in L.SAMPLED_M:
        inp = L.sampled_inputs(dt, d, M, DEV)
        V = inp["V"]
        pl, nl = L.Guarded(M), L.Guarded(M)
        ops.sampled_logits_fwd(inp["f"], inp["E"], inp["pos"], inp["neg"], pl.t, nl.t)
        torch.cuda.synchronize()
        pl.check("pl"), nl.check("nl")
        WORST.report("sampled_logits_fwd", (dt, d, M), L.check_sampled_fwd(inp, pl.t, nl.t))
        for acc in (False, True):
            df, dE = L.Guarded(M, d, dt), L.Guarded(V, d, F32)
            dE.t.copy_(inp["dE0"])
            if acc:
                df.t.copy_(inp["df0"])
            ops.sampled_logits_bwd(inp["f"], inp["E"], inp["pos"], inp["neg"], inp["dpl"], inp["dnl"], df.t, dE.t,
                                   accumulate_df=acc)
            torch.cuda.synchronize()
            df.check("df"), dE.check("dE")
            WORST.report("sampled_logits_bwd", (dt, d, M, acc), L.check_sampled_bwd(inp, df.t, dE.t, acc))
        # dE = None: the table gradient is left to rs_item_grad, df is the same
        df = L.Guarded(M, d, dt)
        ops.sampled_logits_bwd(inp["f"], inp["E"], inp["pos"], inp["neg"], inp["dpl"], inp["dnl"], df.t, None)
        torch.cuda.synchronize()
        df.check("df")
        WORST.report("sampled_logits_bwd", (dt, d, M, "no dE"), L.check_sampled_bwd(inp, df.t, None, False))
