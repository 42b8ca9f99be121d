"""CPU checks of tests/gradtail_ref.py: the float32 emulation of every kernel of the gradient tail stays within the
derived bounds at every shape of the GPU lists (so the bounds admit a correct kernel), and every planted mistake is
rejected (ratio > 1) at the smallest listed shape that exercises it.  No GPU, no native library."""
import pytest
import torch

import gradtail_ref as G
import losshead_ref as L

BF, F32 = torch.bfloat16, torch.float32
CPU = "cpu"


def ok(res):
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, bad


def rejected(res, *keys):
    assert any(res[k] > 1.0 for k in keys), {k: res[k] for k in keys}


# ------------------------------------------------------------------ the grouped launch
def group_check(probs, extra, M, per, outs, ex):
    splits = G.cdiv(M, per)
    res = {}
    for i, (p, (dW, db)) in enumerate(zip(probs, outs)):
        res.update(G.check_wgrad(p, M, splits, dW, db, tag=f"p{i}."))
    for i, o in enumerate(ex):
        res[f"extra{i}"] = G.check_reduce(G.extra_rows(extra, i), extra["out0"][i], 1, o)
    return res


@pytest.mark.parametrize("tset", list(G.GROUP_SETS))
def test_group_emulation(tset):
    """every (M, rows_per_split) at every tile edge the set can take; the forms agree within the two bounds"""
    shapes = G.GROUP_SETS[tset]
    for M, per in G.GROUP_ROWS + (G.GROUP_ROWS_256 if tset == 256 else []):
        probs, extra = G.group_inputs(shapes, M, CPU)
        got = {}
        for s, mt in G.GROUP_FORMS:
            if s != tset:
                continue
            T = G.group_tile(shapes, mt)
            assert T == min(tset, mt)
            outs, ex = G.emu_wgrad_grouped(probs, M, per, T, extra)
            ok(group_check(probs, extra, M, per, outs, ex))
            got[T] = outs
        for T in got:
            for i, p in enumerate(probs):
                ok(G.cross_wgrad(p, M, G.cdiv(M, per), got[T][i], got[tset][i]))


@pytest.mark.parametrize("mut,M,per,keys", [
    ("droplast", 1, 64, ("p0.dW", "p0.db")),                # M = 1: the smallest ragged split
    ("readM", 1, 64, ("p0.dW",)),
    ("skipsplit", 1, 64, ("p0.dW", "extra0")),              # one split, left out: the old value alone
    ("biastile", 1, 64, ("p0.db",)),                        # problems 0 and 1 have a single column tile
    ("adjbias", 1, 64, ("p0.db",)),
    ("noacc", 1, 64, ("p2.dW",))])
def test_group_mutations(mut, M, per, keys):
    probs, extra = G.group_inputs(G.GROUP_SETS[64], M, CPU)
    outs, ex = G.emu_wgrad_grouped(probs, M, per, 64, extra, mut=mut)
    res = group_check(probs, extra, M, per, outs, ex)
    rejected(res, *keys)
    if mut in ("biastile", "adjbias"):                      # the weights are untouched by a bias mistake
        ok({k: v for k, v in res.items() if k.endswith("dW")})


def test_group_ragged_split_mutation_at_second_split():
    """(65, 64): the second split holds the one row a dropped last row loses"""
    probs, extra = G.group_inputs(G.GROUP_SETS[64], 65, CPU)
    outs, ex = G.emu_wgrad_grouped(probs, 65, 64, 64, extra, mut="droplast")
    rejected(group_check(probs, extra, 65, 64, outs, ex), "p1.dW")


# ------------------------------------------------------------------ rs_reduce_segments
@pytest.mark.parametrize("form", list(G.SEG_FORMS))
def test_reduce_segments_emulation(form):
    splits_l, n_l = G.SEG_FORMS[form]
    for splits in splits_l:
        for n in n_l:
            assert G.seg_form(splits, n) == form
            s = G.seg_inputs(splits, n, CPU)
            for acc in (0, 1):
                out = G.emu_reduce(s["src"], s["stride"], splits, n, s["out0"], acc)
                ok({"out": G.check_reduce(s["rows"], s["out0"], acc, out)})


@pytest.mark.parametrize("mut,splits,n", [
    ("remainder", 1, 4), ("remainder", 5, 4),               # column form: all remainder; one past the unrolled four
    ("remainder", 33, 4), ("remainder", 49, 4),             # tree C = 16: remainder only; the first unrolled trip
    ("remainder", 65, 4), ("remainder", 193, 4),            # tree C = 4
    ("skipsplit", 1, 4), ("skipsplit", 33, 4), ("skipsplit", 65, 4), ("skipsplit", 1, 65536),
    ("noacc", 1, 4), ("noacc", 33, 4), ("noacc", 65, 4), ("noacc", 1, 65536),
    ("stridelen", 2, 4), ("stridelen", 33, 4), ("stridelen", 65, 4), ("stridelen", 2, 65536),
    ("old2", 1, 65536)])
def test_reduce_segments_mutations(mut, splits, n):
    """the smallest listed (splits, n) of each form that has the mistake's ingredient (a second split for the stride)"""
    s = G.seg_inputs(splits, n, CPU)
    out = G.emu_reduce(s["src"], s["stride"], splits, n, s["out0"], 1, mut=mut)
    rejected({"out": G.check_reduce(s["rows"], s["out0"], 1, out)}, "out")


# ------------------------------------------------------------------ rs_reduce_slabs(2)
def slabs_case(n, splits, n0=None, seed=0):
    g = G.gen_for(CPU, 59, n, splits, seed)
    n0 = n if n0 is None else n0
    return G.rn(g, CPU, splits, n), G.rn(g, CPU, n0), G.rn(g, CPU, n - n0), n0


def slabs_check(slab, o0, o1, n0, acc, got):
    res = {}
    for k, old, sl, out in (("out0", o0, slice(0, n0), got[0]), ("out1", o1, slice(n0, None), got[1])):
        if out is not None and out.numel():
            res[k] = G.check_reduce(slab[:, sl], old, acc, out)
    return res


def test_reduce_slabs_emulation():
    assert {G.slabs_form(n, n)[0] for n in G.SLABS_N} == {16, 32, 64}
    for n in G.SLABS_N + (G.SLABS_SCALAR[0],):
        for splits in G.SLABS_SPLITS:
            for n0 in (n, G.SLABS_SCALAR[1] if n % 4 else n // 2 // 4 * 4):
                slab, o0, o1, n0 = slabs_case(n, splits, n0)
                for acc in (0, 1):
                    for a, b in ((o0, o1), (None, o1), (o0, None)):
                        ok(slabs_check(slab, a, b, n0, acc, G.emu_reduce_slabs(slab, n0, a, b, acc)))


@pytest.mark.parametrize("mut,n,splits", [("remainder", 4, 1), ("remainder", 4, 49), ("remainder", 64, 25),
                                          ("remainder", 1028, 13), ("remainder", 50, 29), ("skipsplit", 4, 1),
                                          ("noacc", 4, 1)])
def test_reduce_slabs_mutations(mut, n, splits):
    """n = 4: the smallest length; the unrolled loops at the first split count that enters each (C = 16: 49, C = 32:
    25, C = 64: 13, scalar: 29), where the remainder is what is left after one unrolled trip"""
    slab, o0, _, n0 = slabs_case(n, splits)
    got = G.emu_reduce_slabs(slab, n0, o0, None, 1, mut=mut)
    rejected(slabs_check(slab, o0, None, n0, 1, got), "out0")


# ------------------------------------------------------------------ rs_colsum
@pytest.mark.parametrize("dt", [BF, F32])
def test_colsum_emulation_and_mutation(dt):
    assert {G.colsum_form(dt, N) for N in G.COLSUM_N} >= {1, 8} and G.colsum_form(BF, 128) == 16
    for N in G.COLSUM_N:
        for M in G.COLSUM_M:
            g = G.gen_for(CPU, 61, N, M)
            X, out0 = G.operand(g, CPU, M, N, dt), G.rn(g, CPU, N)
            for acc in (0, 1):
                ok({"out": G.check_colsum(X, out0, acc, G.emu_colsum(X, out0, acc))})
    g = G.gen_for(CPU, 61, 64, 1)                           # M = 1, N = 64: the smallest case
    X, out0 = G.operand(g, CPU, 1, 64, dt), G.rn(g, CPU, 64)
    for mut in ("lastrow", "noacc"):
        rejected({"out": G.check_colsum(X, out0, 1, G.emu_colsum(X, out0, 1, mut=mut))}, "out")


# ------------------------------------------------------------------ rs_linear_wgrad
def lw_check(p, M, splits, rows_dev, acc, got):
    rows = M if rows_dev is None else min(M, rows_dev)
    return G.check_wgrad(p, rows, splits, got[0], got[1], accumulate=acc)


@pytest.mark.parametrize("dt,N,K,unal", G.LW_FORMS)
def test_linear_wgrad_emulation(dt, N, K, unal):
    for M in G.LW_M:
        for splits in G.LW_SPLITS:
            for rd in G.LW_ROWS_DEV:
                for bias in (True, False):
                    p = G.lw_inputs(dt, N, K, unal, M, rd, bias, CPU)
                    for acc in (0, 1):
                        got = G.emu_linear_wgrad(p, M, splits, rd, acc, unal)
                        ok(lw_check(p, M, splits, rd, acc, got))
                        if rd == 0:                         # every split empty: the old values, or zeros
                            assert torch.equal(got[0], p["dW0"] if acc else torch.zeros_like(p["dW0"]))


@pytest.mark.parametrize("mut,M,splits,rd", [("emptynan", 1, 2, None), ("emptynan", 65, 3, None),
                                             ("rowsdev", 1, 1, 0), ("rowsdev", 65, 2, 64), ("droplast", 1, 1, None),
                                             ("readM", 1, 1, None), ("skipsplit", 65, 2, None), ("noacc", 1, 1, None),
                                             ("noacc", 1, 2, None)])
def test_linear_wgrad_mutations(mut, M, splits, rd):
    """M = 1 with two splits: the smallest case with an empty split; (65, 3): the issue's; rows_dev = 0 at M = 1"""
    p = G.lw_inputs(BF, 64, 64, False, M, rd, True, CPU)
    got = G.emu_linear_wgrad(p, M, splits, rd, 1, False, mut=mut)
    rejected(lw_check(p, M, splits, rd, 1, got), "dW", "db")


# ------------------------------------------------------------------ the fused launch
def keep_mask(inp, p):
    return L.rand_mask(torch.Generator().manual_seed(5), CPU, inp["ids"].numel(), inp["d"], p)


def fused_check(inp, keep, p, outs, lnout, dpos):
    M = inp["M"]
    res = {}
    for i, (q, (dW, db)) in enumerate(zip(inp["probs"], outs)):
        res.update(G.check_wgrad(q, M, G.cdiv(M, 64), dW, db, tag=f"p{i}."))
    for i, (s, pair) in enumerate(zip(inp["ln"], lnout)):
        for j in range(2):
            res[f"ln{i}.{j}"] = G.check_reduce(s["part"][:, j], s["out0"][j], 1, pair[j])
    res.update(G.check_embed_bwd(0, inp["emb"], keep, p, None, dpos, True))
    return res


def emu_fused(inp, keep, p, RG, mut=None):
    d = inp["d"]
    T = G.group_tile([(q["N"], q["K"]) for q in inp["probs"]], 256)
    outs, _ = G.emu_wgrad_grouped(inp["probs"], inp["M"], 64, T)
    lnout = [[G.emu_reduce(s["part"].reshape(-1)[j * d:], 2 * d, G.LN_SETS, d, s["out0"][j]) for j in range(2)]
             for s in inp["ln"]]
    return outs, lnout, G.emu_pos(inp["emb"], keep, p, RG, mut=mut)


@pytest.mark.parametrize("d", G.FUSED_D)
@pytest.mark.parametrize("T", G.FUSED_T)
def test_fused_emulation(d, T):
    """16 batch groups (the fused launch) and 32 (rs_embed_bwd) both meet the bound; the same bits up to 16
    sequences, where every group holds at most one"""
    differ = 0
    for B in G.FUSED_B:
        inp = G.fused_inputs(d, T, B, CPU, hb=3)
        assert int((inp["emb"]["ids"] == 0).sum()) > 0 or B * T == 1
        for p in G.FUSED_P:
            keep = keep_mask(inp["emb"], p)
            outs, lnout, dpos = emu_fused(inp, keep, p, G.POS_RG_FUSED)
            ok(fused_check(inp, keep, p, outs, lnout, dpos))
            alone = G.emu_pos(inp["emb"], keep, p, G.POS_RG_ALONE)
            ok(G.check_embed_bwd(0, inp["emb"], keep, p, None, alone, True))
            if B <= G.POS_RG_FUSED:
                assert torch.equal(dpos, alone)
            else:
                differ += int(not torch.equal(dpos, alone))
    assert differ > 0, "the two groupings add more than 16 sequences in different orders: some bits differ"


def test_fused_head_stats_emulation():
    for hb in G.FUSED_HB:
        part = G.fused_inputs(64, 1, 1, CPU, hb=hb)["head"]
        for div in (None, 77.0):
            ok(G.check_head_stats(part, div, L.emu_head_stats(part, div)))
    part = G.fused_inputs(64, 1, 1, CPU, hb=3)["head"]      # three blocks: the smallest with one to lose
    rejected(G.check_head_stats(part, None, L.emu_head_stats(part, None, mut="statblk")), "out", "out.count")


def test_fused_position_0_skipped():
    """d = 64, T = 1, one sequence: the smallest case; position 0's row is live there"""
    inp = G.fused_inputs(64, 1, 1, CPU)
    keep = keep_mask(inp["emb"], 0.0)
    assert int(inp["emb"]["ids"][0]) != 0
    rejected(G.check_embed_bwd(0, inp["emb"], keep, 0.0, None, G.emu_pos(inp["emb"], keep, 0.0, 16, mut="noh"), True),
             "dpos")
