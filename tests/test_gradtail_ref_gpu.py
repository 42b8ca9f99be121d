"""Kernel-level checks of the gradient tail: rs_wgrad_grouped_max and its grouped reduction (wgrad.hip), the fused
rs_wgrad_grouped_pos / _pos_stats launch (grad_tail.hip), rs_reduce_segments, rs_reduce_slabs(2) (reduce.hip),
rs_colsum (misc.hip) and the split-K rs_linear_wgrad (gemm.hip), called through ops and the C ABI, every stored
element held to the float64 reference and derived bound of tests/gradtail_ref.py.

Every output is a losshead_ref.Guarded (NaN pre-fill, guard rows, store-before-base check), every operand a column
slice of a wider NaN-filled buffer with NaN rows after row M, every slab NaN-pre-filled; every launch runs twice and
must give the same bits.  The module prints its worst err / bound per kernel and tensor; any ratio above 1 fails."""
import pytest
import torch

import gradtail_ref as G
import losshead_ref as L

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
SALT, SEED = 0x1234_5678_9ABC_DEF1, 977
DEV = "cuda"
ERR_ARG, ERR_UNSUPPORTED = 1001, 1002
WORST = L.Worst()


def _ops():
    from rbm_amd import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    WORST.dump()


def guarded(t0, fill=True, offset=0):
    """a Guarded float32 output of t0's shape, holding t0's values (fill) or NaN (a call that must not accumulate)"""
    g = L.Guarded(t0.shape[0], t0.shape[1] if t0.dim() == 2 else None, F32, DEV, offset=offset)
    if fill:
        g.t.copy_(t0)
    return g


def same_bits(a, b):
    return torch.equal(a.flat.view(torch.int32), b.flat.view(torch.int32))


def twice(run):
    """run() -> {name: Guarded}: two runs give the same bits everywhere (guards and pads included)"""
    a, b = run(), run()
    for k in a:
        assert same_bits(a[k], b[k]), f"{k}: two runs differ"
    return a


def nan_slab(n):
    return torch.full((max(n, 4),), G.NAN, device=DEV)


# ------------------------------------------------------------------ the grouped launch
def extra_segs(extra):
    flat = extra["part"].reshape(-1)
    return [(flat[i * G.EXTRA_N:], 2 * G.EXTRA_N, G.EXTRA_SPLITS, G.EXTRA_N, extra["out0"][i]) for i in range(2)]


def group_run(probs, segs, M, per, slab_short=0, **kw):
    """one ops.wgrad_grouped call on fresh Guarded outputs; segs: [(src, stride, splits, n, out0)]"""
    ops = _ops()
    out = {}
    for i, p in enumerate(probs):
        out[f"p{i}.dW"] = guarded(p["dW0"])
        if p["db0"] is not None:
            out[f"p{i}.db"] = guarded(p["db0"])
    for i, s in enumerate(segs):
        out[f"seg{i}"] = guarded(s[4])
    plist = [(p["dY"], p["X"], out[f"p{i}.dW"].t, out[f"p{i}.db"].t if p["db0"] is not None else None)
             for i, p in enumerate(probs)]
    slab = nan_slab(ops.wgrad_grouped_slab_numel([(p["N"], p["K"]) for p in probs], M, per) - slab_short)
    ops.wgrad_grouped(plist, M, per, slab, extra=[s[:4] + (out[f"seg{i}"].t,) for i, s in enumerate(segs)], **kw)
    torch.cuda.synchronize()
    return out


def group_check(probs, segs, M, per, out):
    splits = G.cdiv(M, per)
    res = {}
    for i, p in enumerate(probs):
        db = out[f"p{i}.db"].t if p["db0"] is not None else None
        res.update(G.check_wgrad(p, M, splits, out[f"p{i}.dW"].t, db, tag=f"p{i}."))
    for i, (src, stride, sp, n, out0) in enumerate(segs):
        rows = torch.stack([src[z * stride:z * stride + n] for z in range(sp)])
        res[f"seg{i}"] = G.check_reduce(rows, out0, 1, out[f"seg{i}"].t)
    for k, g in out.items():
        g.check(k)
    return res


@pytest.mark.parametrize("tset", list(G.GROUP_SETS))
def test_wgrad_grouped(tset):
    """the 64 / 128 tiles' checked loop and ring (nk = 1, 2, 3), the 256 tile with fewer stages than its prefetch
    distance and tails of 31, 0 and 1 rows, the capped forms of the 256 set; 1 .. 5 splits (workgroup counts on both
    sides of the XCD remap); the tile forms agree within the sum of their bounds"""
    shapes = G.GROUP_SETS[tset]
    ops = _ops()
    for M, per in G.GROUP_ROWS + (G.GROUP_ROWS_256 if tset == 256 else []):
        probs, extra = G.group_inputs(shapes, M, DEV)
        segs = extra_segs(extra)
        got = {}
        for s, mt in G.GROUP_FORMS:
            if s != tset:
                continue
            T = G.group_tile(shapes, mt)
            assert ops.wgrad_grouped_tile(shapes, mt) == T == min(tset, mt)
            out = twice(lambda: group_run(probs, segs, M, per, max_tile=mt))
            WORST.report(f"wgrad_grouped/{T}", (tset, M, per), group_check(probs, segs, M, per, out))
            got[T] = out
        for T, out in got.items():
            if T == tset:
                continue
            res = {}
            for i, p in enumerate(probs):
                pair = [(o[f"p{i}.dW"].t, o[f"p{i}.db"].t if p["db0"] is not None else None) for o in (out, got[tset])]
                res.update(G.cross_wgrad(p, M, G.cdiv(M, per), pair[0], pair[1], tag=f"p{i}."))
            WORST.report(f"wgrad_grouped/{T}~{tset}", (tset, M, per), res)


@pytest.mark.parametrize("case,code", [("17 problems", ERR_ARG), ("rows 96", ERR_ARG), ("N 96", ERR_UNSUPPORTED),
                                       ("pitch N+4", ERR_UNSUPPORTED), ("slab short", ERR_ARG),
                                       ("65 extra", ERR_ARG)])
def test_wgrad_grouped_argument_errors(case, code):
    """each returns its error and leaves every output as it was"""
    M, per = 65, 64
    g = G.gen_for(DEV, 67)
    shapes = [(64, 64)] * (17 if case == "17 problems" else 2)
    probs = [G.problem(g, DEV, M, N, K) for N, K in shapes]
    segs = extra_segs(G.group_inputs(G.GROUP_SETS[64], M, DEV)[1])
    if case == "65 extra":
        segs = (segs * 33)[:65]
    if case == "rows 96":
        per = 96
    if case == "N 96":
        probs[1] = G.problem(g, DEV, M, 96, 64)
    if case == "pitch N+4":
        probs[1]["dY"] = torch.full((M, 64 + 4), 0.5, dtype=BF, device=DEV)[:, :64]
        assert probs[1]["dY"].data_ptr() % 16 == 0
    ops = _ops()
    out = {}
    for i, p in enumerate(probs):
        out[f"p{i}.dW"], out[f"p{i}.db"] = guarded(p["dW0"], fill=False), guarded(p["db0"], fill=False)
    for i, s in enumerate(segs):
        out[f"seg{i}"] = guarded(s[4], fill=False)
    plist = [(p["dY"], p["X"], out[f"p{i}.dW"].t, out[f"p{i}.db"].t) for i, p in enumerate(probs)]
    slab = nan_slab(ops.wgrad_grouped_slab_numel([(p["N"], p["K"]) for p in probs], M, per) -
                    (1 if case == "slab short" else 0))
    with pytest.raises(RuntimeError, match=f"rs_wgrad_grouped_max failed with code {code}$"):
        ops.wgrad_grouped(plist, M, per, slab, extra=[s[:4] + (out[f"seg{i}"].t,) for i, s in enumerate(segs)])
    torch.cuda.synchronize()
    for k, o in out.items():
        o.untouched(k)
    assert torch.isnan(slab).all()


# ------------------------------------------------------------------ rs_reduce_segments
def seg_run(segs, acc):
    ops = _ops()
    out = {i: guarded(s["out0"], fill=bool(acc)) for i, s in enumerate(segs)}
    ops.reduce_segments([(s["src"], s["stride"], s["splits"], s["n"], out[i].t) for i, s in enumerate(segs)],
                        accumulate=bool(acc))
    torch.cuda.synchronize()
    for i, o in out.items():
        o.check(f"seg{i}")
    return out


def seg_report(name, key, segs, acc, out):
    WORST.report(name, key, {f"{s['splits']}x{s['n']}": G.check_reduce(s["rows"], s["out0"], acc, out[i].t)
                             for i, s in enumerate(segs)})


@pytest.mark.parametrize("form", list(G.SEG_FORMS))
def test_reduce_segments(form):
    """every (splits, n) of the form alone and all of them in one launch (the same bits): a stride above n, both
    accumulate modes, each form's unrolled loop and remainder, lengths on both sides of a workgroup's columns"""
    splits_l, n_l = G.SEG_FORMS[form]
    segs = [G.seg_inputs(sp, n, DEV) for sp in splits_l for n in n_l]
    assert all(G.seg_form(s["splits"], s["n"]) == form and s["stride"] > s["n"] for s in segs)
    for acc in (0, 1):
        together = twice(lambda: seg_run(segs, acc))
        seg_report(f"reduce_segments/{form}", ("all", acc), segs, acc, together)
        for i, s in enumerate(segs):
            alone = seg_run([s], acc)
            assert same_bits(alone[0], together[i]), (s["splits"], s["n"])


def test_reduce_segments_mixed_and_two_launches():
    """one launch holding all four forms; 70 segments in one call (two launches)"""
    mixed = [G.seg_inputs(sp, n, DEV) for sp, n in ((5, 1028), (3, 65536 + 4), (49, 68), (193, 60))]
    assert {G.seg_form(s["splits"], s["n"]) for s in mixed} == set(G.SEG_FORMS)
    many = [G.seg_inputs(sp, n, DEV) for sp, n in (((5, 1028), (49, 68), (193, 60), (1, 4), (32, 1020)) * 14)]
    assert len(many) == 70
    for name, segs in (("mixed", mixed), ("70", many)):
        for acc in (0, 1):
            out = twice(lambda: seg_run(segs, acc))
            seg_report(f"reduce_segments/{name}", (acc,), segs, acc, out)


@pytest.mark.parametrize("case", ["n 6", "out misaligned", "splits 0"])
def test_reduce_segments_argument_errors(case):
    ops = _ops()
    s = G.seg_inputs(3, 8, DEV)
    out = guarded(s["out0"], fill=False, offset=1 if case == "out misaligned" else 0)
    n = 6 if case == "n 6" else 8
    with pytest.raises(RuntimeError, match=f"rs_reduce_segments failed with code {ERR_ARG}$"):
        ops.reduce_segments([(s["src"], s["stride"], 0 if case == "splits 0" else 3, n, out.t[:n])], accumulate=False)
    torch.cuda.synchronize()
    out.untouched("out")


# ------------------------------------------------------------------ rs_reduce_slabs / rs_reduce_slabs2
def slabs_run(slab, splits, n, n0, o0, o1, acc, two, off=0):
    from rbm_amd import _lib
    out = {}
    if o0 is not None:
        out["out0"] = guarded(o0, fill=bool(acc), offset=off)
    if o1 is not None:
        out["out1"] = guarded(o1, fill=bool(acc), offset=off)
    p0, p1 = (_lib.ptr(out[k].t) if k in out else None for k in ("out0", "out1"))
    if two:
        _lib.call("rs_reduce_slabs2", _lib.ptr(slab), splits, n0, p0, n - n0, p1, acc, _lib.stream())
    else:
        _lib.call("rs_reduce_slabs", _lib.ptr(slab), splits, n, p0, acc, _lib.stream())
    torch.cuda.synchronize()
    for k, o in out.items():
        o.check(k)
    return out


def slabs_case(n, splits, n0):
    g = G.gen_for(DEV, 59, n, splits, n0)
    buf = nan_slab(splits * n + 64)                         # NaN after the last slab
    buf[:splits * n] = G.rn(g, DEV, splits * n)
    return buf, buf[:splits * n].view(splits, n), G.rn(g, DEV, max(n0, 1))[:n0], G.rn(g, DEV, max(n - n0, 1))[:n - n0]


@pytest.mark.parametrize("n", G.SLABS_N + (G.SLABS_SCALAR[0],))
def test_reduce_slabs(n):
    """float4 columns C = 16, 32, 64 by n (n = 50: the scalar kernel, n0 = 6), the split counts that first enter each
    unrolled loop, out0 or out1 null, both accumulate modes, outputs one float off 16 bytes (the scalar kernel)"""
    scalar = n % 4 != 0
    for splits in G.SLABS_SPLITS:
        n0 = G.SLABS_SCALAR[1] if scalar else n // 2 // 4 * 4
        buf, slab, o0, o1 = slabs_case(n, splits, n0)
        full0 = torch.cat([o0, o1])
        for acc in (0, 1):
            res = {}
            out = twice(lambda: slabs_run(buf, splits, n, n, full0, None, acc, two=False))
            res["one"] = G.check_reduce(slab, full0, acc, out["out0"].t)
            out = twice(lambda: slabs_run(buf, splits, n, n, full0, None, acc, two=False, off=1))
            res["one.off"] = G.check_reduce(slab, full0, acc, out["out0"].t)
            for a, b, tag in ((o0, o1, "both"), (None, o1, "no0"), (o0, None, "no1")):
                if (a is None or not a.numel()) and (b is None or not b.numel()):
                    continue
                out = twice(lambda: slabs_run(buf, splits, n, n0, a if a is not None and a.numel() else None,
                                              b if b is not None and b.numel() else None, acc, two=True))
                for k, old, sl in (("out0", o0, slice(0, n0)), ("out1", o1, slice(n0, None))):
                    if k in out:
                        res[f"{tag}.{k}"] = G.check_reduce(slab[:, sl], old, acc, out[k].t)
            WORST.report("reduce_slabs", (n, splits, acc), res)


# ------------------------------------------------------------------ rs_colsum
@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("N", G.COLSUM_N)
def test_colsum(dt, N):
    """the three chunk-column forms and the one-thread-per-column form (N = 50, 520), 1 .. 64 row blocks, pitch > N"""
    ops = _ops()
    for M in G.COLSUM_M:
        g = G.gen_for(DEV, 61, N, M)
        X, out0 = G.operand(g, DEV, M, N, dt), G.rn(g, DEV, N)
        assert X.stride(0) > N
        for acc in (0, 1):
            def run():
                out = guarded(out0, fill=bool(acc))
                ops.colsum(X, out.t, nan_slab(64 * N), accumulate=bool(acc))
                torch.cuda.synchronize()
                out.check("out")
                return {"out": out}
            WORST.report("colsum", (dt, N, M, acc), {"out": G.check_colsum(X, out0, acc, twice(run)["out"].t)})


# ------------------------------------------------------------------ rs_linear_wgrad
@pytest.mark.parametrize("dt,N,K,unal", G.LW_FORMS,
                         ids=[f"{'bf16' if f[0] == BF else 'fp32'}-{f[1]}x{f[2]}" for f in G.LW_FORMS])
def test_linear_wgrad(dt, N, K, unal):
    """the direct form, the split-K bf16 / fp32 / unaligned forms with 1 .. 3 splits (an empty third split at M =
    65), a device row count (0: every split empty) whose excluded rows are NaN, with and without the bias, both
    accumulate modes; the slab is NaN-pre-filled"""
    ops = _ops()
    for M in G.LW_M:
        for splits in G.LW_SPLITS:
            for rd in G.LW_ROWS_DEV:
                rows = M if rd is None else min(M, rd)
                rows_dev = None if rd is None else torch.tensor([rd], dtype=torch.int32, device=DEV)
                for bias in (True, False):
                    p = G.lw_inputs(dt, N, K, unal, M, rd, bias, DEV)
                    aligned = p["dY"].stride(0) % 8 == 0 and p["X"].stride(0) % 8 == 0
                    assert aligned != unal and p["dY"].data_ptr() % 16 == 0 and p["X"].data_ptr() % 16 == 0
                    for acc in (0, 1):
                        def run():
                            out = {"dW": guarded(p["dW0"], fill=bool(acc))}
                            if bias:
                                out["db"] = guarded(p["db0"], fill=bool(acc))
                            ops.linear_wgrad(p["dY"], p["X"], out["dW"].t, nan_slab(splits * (N * K + N)),
                                             db=out["db"].t if bias else None, split_k=splits, accumulate=bool(acc),
                                             rows_dev=rows_dev)
                            torch.cuda.synchronize()
                            for k, o in out.items():
                                o.check(k)
                            return out
                        out = twice(run)
                        WORST.report("linear_wgrad", (dt, N, K, M, splits, rd, bias, acc),
                                     G.check_wgrad(p, rows, splits, out["dW"].t, out["db"].t if bias else None,
                                                   accumulate=bool(acc)))
                        if rows == 0:
                            assert torch.equal(out["dW"].t, p["dW0"] if acc else torch.zeros_like(p["dW0"]))


# ------------------------------------------------------------------ the fused launch
def _sb():
    return torch.full((1,), SEED, dtype=torch.int64, device=DEV)


def _mask(rows, d, p, sb):
    """keep mask of the dropout site with element index r*d + c (the kernels' own hash, through the C ABI)"""
    if p == 0:
        return torch.ones(rows, d, dtype=torch.bool, device=DEV)
    ones = torch.ones(rows, d, dtype=F32, device=DEV)
    out = torch.empty_like(ones)
    _ops().dropout_rowmask(ones, p, SALT, sb, None, out)
    return out > 0


def ln_segs(inp):
    d = inp["d"]
    return [(s["part"].reshape(-1)[j * d:], 2 * d, s["part"].shape[0], d, s["out0"][j])
            for s in inp["ln"] for j in range(2)]


def fused_run(inp, segs, p, sb, div, per=64):
    """the pos= form of ops.wgrad_grouped (with the head statistics when the inputs have head partials)"""
    emb = inp["emb"]

    def run():
        dpos, loss, aux = guarded(emb["dpos0"]), L.Guarded(4), L.Guarded(2)
        pos = (emb["ids"], emb["T"], emb["dx"], p, SALT, sb, dpos.t)
        if inp["head"] is not None:
            pos += (inp["head"], div, loss.t, aux.t)
        out = group_run(inp["probs"], segs, inp["M"], per, pos=pos)
        out.update(dpos=dpos)
        if inp["head"] is not None:
            out.update(loss=loss, aux=aux)
        return out
    return twice(run)


def alone_run(inp, segs, p, sb, div, per=64):
    """the functions one after the other: rs_wgrad_grouped, rs_embed_bwd's positional part, rs_sas_head_finish"""
    ops = _ops()
    emb = inp["emb"]
    out = group_run(inp["probs"], segs, inp["M"], per)
    out["dpos"] = guarded(emb["dpos0"])
    ops.embed_bwd(0, emb["ids"], emb["T"], emb["dx"], 1.0, p, SALT, sb, None, out["dpos"].t, accumulate_pos=True)
    if inp["head"] is not None:
        out["loss"] = L.Guarded(4)
        ops.sas_head_finish(inp["head"], div, out["loss"].t)
    torch.cuda.synchronize()
    return out


def fused_compare(inp, segs, p, sb, div, dpos_bits):
    """the fused launch against the bounds and against the functions one after the other: weights, biases, segment
    outputs and loss statistics bit for bit; dpos bit for bit where dpos_bits, and within its bound always"""
    emb = inp["emb"]
    keep = _mask(inp["M"], inp["d"], p, sb)
    fused, alone = fused_run(inp, segs, p, sb, div), alone_run(inp, segs, p, sb, div)
    dpos = fused.pop("dpos")
    dpos.check("dpos")
    res = group_check(inp["probs"], segs, inp["M"], 64, {k: v for k, v in fused.items() if k not in ("loss", "aux")})
    res.update(L.check_embed_bwd(0, emb, keep, p, None, dpos.t, True))
    res["dpos.alone"] = L.check_embed_bwd(0, emb, keep, p, None, alone["dpos"].t, True)["dpos"]
    if inp["head"] is not None:
        fused["loss"].check("loss"), fused["aux"].check("aux")
        res.update(L.check_head_stats(inp["head"], None if div is None else float(div), fused["loss"].t))
        assert torch.equal(fused["aux"].t, fused["loss"].t[:2]), "aux_out = (loss sum, count)"
    for k, o in fused.items():
        if k != "aux":
            assert same_bits(o, alone[k]), f"{k}: the fused launch and the functions one after the other differ"
    if dpos_bits:
        assert same_bits(dpos, alone["dpos"]), "dpos: the fused launch and rs_embed_bwd differ"
    else:
        print("\ndpos, fused launch against rs_embed_bwd:", "same bits" if same_bits(dpos, alone["dpos"]) else
              "bits differ (another grouping of the batch rows)")
    return res


@pytest.mark.parametrize("d", G.FUSED_D)
@pytest.mark.parametrize("T", G.FUSED_T)
def test_fused_pos_stats(d, T):
    """the SAS block's set with the positional sum (ids with padding, an all-padding position, dropout from the
    kernels' own hash) and, for three block counts, the head statistics riding in the reduction launch.  The
    contract: weights, biases, segment outputs and loss statistics equal the functions one after the other bit for
    bit; dpos equals rs_embed_bwd's bit for bit up to 16 sequences (16 batch groups here, 32 there: past 16 the
    batch rows are added in another grouping) and agrees with it within the two bounds beyond"""
    sb = _sb()
    for B in G.FUSED_B:
        for p in G.FUSED_P:
            for hb in (None,) + G.FUSED_HB:
                inp = G.fused_inputs(d, T, B, DEV, hb=hb)
                assert T == 1 or int((inp["emb"]["ids"].view(B, T)[:, T - 1] != 0).sum()) == 0
                div = torch.full((1,), 77.0, device=DEV) if hb and p > 0 else None
                res = fused_compare(inp, ln_segs(inp), p, sb, div, dpos_bits=B <= G.POS_RG_FUSED)
                WORST.report("wgrad_grouped_pos" + ("_stats" if hb else ""), (d, T, B, p, hb), res)


@pytest.mark.parametrize("case", ["d 256", "65 segments"])
def test_fused_fallbacks(case):
    """d = 256 (wider than the fused positional body) and 16 problems with 65 segments (more than one reduction
    launch holds): the unfused branch, every output the same bits as the functions one after the other"""
    sb = _sb()
    if case == "d 256":
        inp = G.fused_inputs(256, 3, 17, DEV, hb=3)
        segs = ln_segs(inp)
    else:
        inp = G.fused_inputs(64, 3, 17, DEV, hb=3)
        g = G.gen_for(DEV, 71)
        inp["probs"] = [G.problem(g, DEV, inp["M"], 64, 64) for _ in range(16)]
        segs = (ln_segs(inp) * 5)[:33]
        assert 2 * len(inp["probs"]) + len(segs) == 65
    div = torch.full((1,), 77.0, device=DEV)
    p = 0.2
    keep = _mask(inp["M"], inp["d"], p, sb)
    fused, alone = fused_run(inp, segs, p, sb, div), alone_run(inp, segs, p, sb, div)
    for k, o in fused.items():
        o.check(k)
        if k != "aux":
            assert same_bits(o, alone[k]), k
    assert torch.equal(fused["aux"].t, fused["loss"].t[:2])
    res = L.check_embed_bwd(0, inp["emb"], keep, p, None, fused["dpos"].t, True)
    res.update(L.check_head_stats(inp["head"], 77.0, fused["loss"].t))
    WORST.report("wgrad_grouped_pos_stats/unfused", (case,), res)
