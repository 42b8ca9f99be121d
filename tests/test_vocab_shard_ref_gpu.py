"""Kernel-level float64 checks of the vocabulary-sharded head and of the vocabulary head's two forms (vocab_head.hip)
through the C ABI, against tests/vocab_shard_ref.py: per element, with derived bounds, in ONE process -- the N shards
of a vocabulary are slices of E and the bias by vocab_parallel.shard_range.

  chain      rs_vocab_shard_lse, rs_vocab_shard_label_logits, rs_vocab_shard_combine and rs_vocab_head_bwd(voff) at
             vocab_shard_ref.CHAIN_CASES, with and without bias: every shard's lse and label logits, the combined lse
             (staged and end to end), out = {sum, count, mean}, every element of every shard's dlogits; label-0 rows
             exactly 0; a row whose label lives in another shard has a label logit of exactly 0 and no one-hot
  identity   one shard: the chain's lse and out against rs_vocab_head_fwd, within the sum of the two bounds
  patterns   boundary labels, a label-free shard, an all-dead batch, logits past 88 on live and label-0 rows; the last
             two also through rs_vocab_head_fwd / _bwd and rs_vocab_ce_fwd / _bwd on the whole table
  voff       a shard start that is neither 128- nor 8-aligned (the header does not restrict voff)
  fallback   the smallest (R, V1) at d = 256 whose backward leaves the ping-pong form because its per-row metadata
             does not fit LDS, taken from rs_vocab_head_form on the device; one row tile fewer is still ping-pong;
             forward and every element of dlogits with rows_dev = R - 5, float64 in class chunks of 4,096; again as
             shard 1 of 2
  glue       the engine's op sequence behind the sharded head: rs_linear_wgrad into the [v0, v1) slice of a prefilled
             full-size gradient (the other rows bit for bit unchanged), split-K rs_gemm + rs_reduce_slabs for dH

Every case runs in the ping-pong (RS_VHEAD_PP=1) and the lock-step (RS_VHEAD_PP=0) form and first asserts through
rs_vocab_head_form that it runs the form it names.  Every output is prefilled with NaN and guarded.

Bit identity of the concatenated shards' dlogits with a whole-table call fed the same lse is printed, not asserted:
each element is the same sequence of operations in both calls (bias, the k steps in order, one fma, exp2 or exp, the
one-hot, the scale), but a shard start that is an odd multiple of 128 moves a column to another wave quarter of the
256-class tile, and that the matrix unit rounds alike in every lane position is not something the source shows.

It was 0 of 650,130 elements in both forms.

Fallback thresholds (row tiles of 32 per y-group the ping-pong backward holds): 392 / 296 / 104 at d = 64 / 128 / 256;
on 256 CUs the test's shape is R = 3,329, V1 = 32,769.

Measured on an MI355X, worst err / bound per output, ping-pong | lock-step (also DESIGN.md, vocabulary-head section):
shard lse 0.026 | 0.026, label logits 0.003 | 0.003, combined lse staged 0.042 | 0.042, end to end 0.022 | 0.022, sum
0.005 | 0.005, mean 0.005 | 0.004, dlogits 0.494 | 0.494; voff dlogits 0.485 | 0.485; one shard against
rs_vocab_head_fwd lse 0.008; fallback lse 0.005, sum 0.0001, dlogits 0.486; big logits lse 0.004 | 0.009 (vocab_ce
0.007), dlogits 0.429; glue dW 0.013, db 0.002, dH 0.003.

Kernel fix these tests brought: the lock-step backward multiplied a label-0 row's exp(x - 0) by a zero scale, NaN for a
logit above 88.7; test_patterns[big-*-0] fails on the library before the fix.
"""
import pytest
import torch

import losshead_ref as L
import vocab_shard_ref as S
from rowchain_ref import D, bound_f32, ratio

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DEV = "cuda"
WORST = L.Worst()
FORMS = (1, 0)
NAME = {1: "pp", 0: "lockstep"}


def _ops():
    from rbm_amd import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    WORST.dump()


def scalar(v, dt=F32):
    return None if v is None else torch.full((1,), v, dtype=dt, device=DEV)


def ceil8(n):
    return -(-n // 8) * 8


def assert_form(form, R, V1, d):
    """both launches of these sizes take the form the case names"""
    for bwd in (0, 1):
        assert _ops().vocab_head_form(bwd, R, V1, d)[0] == form, (form, bwd, R, V1, d)


def lse_slot(ws, R, V1):
    ntn = -(-V1 // 128)
    return ws.t[R * ntn * 2 + R:R * ntn * 2 + 2 * R]


def run_chain(inp, form, dloss=None):
    """the sharded chain as the engine runs it, every shard in this process -> (stored tensors, count)"""
    ops = _ops()
    R, d, N, lab = inp["R"], inp["d"], inp["N"], inp["labels"]
    lse_parts, tgt_parts = L.Guarded(N, R), L.Guarded(N, R)
    shards = []
    for q, (v0, v1) in enumerate(inp["ranges"]):
        assert_form(form, R, v1 - v0, d)
        Es, bs = inp["E"][v0:v1], None if inp["bias"] is None else inp["bias"][v0:v1]
        n = ops.vocab_ce_ws_numel(R, v1 - v0)
        ws = L.Guarded(n)
        ops.vocab_shard_lse(inp["h"], Es, bs, lab, ws.t, lse_parts.t[q])
        ops.vocab_shard_label_logits(inp["h"], Es, bs, lab, v0, v1, tgt_parts.t[q])
        shards.append((v0, v1, Es, bs, ws, n))
    torch.cuda.synchronize()
    lse_parts.check("lse_parts")
    tgt_parts.check("tgt_parts")
    tgt = tgt_parts.t.sum(0)                 # the all-reduce: one shard's value and N - 1 exact zeros
    got = {"lse_parts": lse_parts.t, "tgt_parts": tgt_parts.t, "dl": []}
    for v0, v1, Es, bs, ws, n in shards:
        lse, out = lse_slot(ws, R, v1 - v0), L.Guarded(3)
        ops.vocab_shard_combine(lse_parts.t, tgt, lab, lse, out.t)
        dl = L.Guarded(R, v1 - v0, BF, pitch=ceil8(v1 - v0))
        ops.vocab_head_bwd(inp["h"], Es, bs, lab, ws.t, out.t[1:2], dl.t, dloss=scalar(dloss), voff=v0)
        torch.cuda.synchronize()
        out.check("out")
        dl.check("dlogits", pads_zero_ok=True)
        assert torch.isnan(ws.full[n:]).all(), "store past the workspace"
        if "lse" in got:                     # every rank holds the same lse and loss
            assert torch.equal(lse, got["lse"]) and torch.equal(out.t, got["out"])
        else:
            got["lse"], got["out"] = lse.clone(), out.t
        got["dl"].append(dl.t)
    return got, float(got["out"][1])


def run_whole(fwd, bwd, inp, dloss=None, rows=None):
    """forward + backward of a whole-table head -> (lse, out, dlogits, count)"""
    ops = _ops()
    R, V1 = inp["R"], inp["V1"]
    n = ops.vocab_ce_ws_numel(R, V1)
    ws, out = L.Guarded(n), L.Guarded(3)
    rd = scalar(rows, torch.int32)
    fwd(inp["h"], inp["E"], inp["bias"], inp["labels"], ws.t, out.t, rows_dev=rd)
    torch.cuda.synchronize()
    if inp["labels"].any():
        out.check("out")
    else:       # no live row: the whole-table entries' mean is 0 / 0, which the NaN prefill cannot tell from unwritten
        assert not torch.isnan(out.t[:2]).any() and torch.isnan(out.full[3:]).all()
    assert torch.isnan(ws.full[n:]).all(), "store past the workspace"
    dl = L.Guarded(R, V1, BF, pitch=ceil8(V1))
    bwd(inp["h"], inp["E"], inp["bias"], inp["labels"], ws.t, out.t[1:2], dl.t, rows_dev=rd, dloss=scalar(dloss))
    torch.cuda.synchronize()
    dl.check("dlogits", written=rows, pads_zero_ok=True)
    return lse_slot(ws, R, V1), out.t, dl.t, float(out.t[1])


# ---------------------------------------------------------------------- 1. the chain
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("N,V1,d,R", S.CHAIN_CASES)
def test_shard_chain(N, V1, d, R, form, monkeypatch):
    monkeypatch.setenv("RS_VHEAD_PP", str(form))
    for bias, dloss in ((True, None), (False, 0.37)):
        inp = S.shard_inputs(d, R, V1, N, DEV, bias=bias)
        assert int((inp["labels"] == 0).sum()) > 0
        logits = L.vce_logits(inp)
        got, count = run_chain(inp, form, dloss)
        WORST.report("chain." + NAME[form], (N, V1, d, R, bias, dloss),
                     S.check_chain(inp, logits, got, count, 1.0 if dloss is None else dloss))


# ---------------------------------------------------------------------- 2. one shard is the whole-table head
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("d", S.CHAIN_D)
@pytest.mark.parametrize("R", S.CHAIN_R)
def test_one_shard_is_the_whole_table_head(d, R, form, monkeypatch):
    monkeypatch.setenv("RS_VHEAD_PP", str(form))
    ops = _ops()
    V1 = 5001
    inp = S.shard_inputs(d, R, V1, 1, DEV)
    logits = L.vce_logits(inp)
    x, Ax = logits
    lab = inp["labels"]
    live = (lab != 0).double()
    got, count = run_chain(inp, form)
    lse2, out2, _, count2 = run_whole(ops.vocab_head_fwd, ops.vocab_head_bwd, inp)
    assert count2 == count
    rf, b1 = S.e2e_lse_bound(inp, logits)
    b2 = L.vce_lse_bound(x, Ax, rf, d)
    t, At = x.gather(1, lab[:, None])[:, 0], Ax.gather(1, lab[:, None])[:, 0]
    bS = S.loss_sum_bound(rf, b1, t, At, live, R, d) + S.loss_sum_bound(rf, b2, t, At, live, R, d)
    Sr = ((rf - t) * live).sum().abs()
    WORST.report("chain|head." + NAME[form], (d, R), {
        "lse": ratio(got["lse"], D(lse2) * live, (b1 + b2) * live), "sum": ratio(got["out"][0], D(out2[0]), bS),
        "mean": ratio(got["out"][2], D(out2[2]), bS / count + 2 * bound_f32(Sr / count, 1))})


# ---------------------------------------------------------------------- 3. the patterns
def check_whole(name, key, inp, logits, fwd, bwd, dloss):
    lab = inp["labels"]
    lse, out, dl, count = run_whole(fwd, bwd, inp, dloss)
    assert float(lse[lab == 0].abs().sum()) == 0, "label-0 rows: lse = 0"
    res = {"dlogits.dead": 0.0 if float(dl[lab == 0].float().abs().sum()) == 0 else float("inf")}
    if lab.any():
        res.update(L.check_vce_fwd(inp, lse, out, logits=logits))
        res.update(L.check_vce_bwd(inp, lse, count, dloss, dl, logits=logits))
    else:                                    # no live row (the mean of no element is left to the entry point)
        assert float(out[0]) == 0 and float(out[1]) == 0 and count == 0
    WORST.report(name, key, res)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("d", S.PATTERN_D)
@pytest.mark.parametrize("pattern", S.PATTERNS)
def test_patterns(pattern, d, form, monkeypatch):
    monkeypatch.setenv("RS_VHEAD_PP", str(form))
    ops = _ops()
    N, V1, R = S.PATTERN_SHAPE
    dloss = 0.37
    inp = S.shard_inputs(d, R, V1, N, DEV, pattern=pattern)
    lab = inp["labels"]
    logits = L.vce_logits(inp)
    got, count = run_chain(inp, form, dloss)
    WORST.report(f"{pattern}.{NAME[form]}", (d,), S.check_chain(inp, logits, got, count, dloss))
    v0, v1 = inp["ranges"][-1]
    if pattern == "boundary":
        assert {v0 - 1, v0, v0 + 1, V1 - 1, 1} <= set(lab.tolist())
    if pattern == "free":
        assert not S.owned(lab, v0, v1).any() and not got["tgt_parts"][-1].any()
        assert bool((got["dl"][-1].float() >= 0).all())
    if pattern == "dead":
        assert not lab.any() and not got["out"].any() and not got["lse"].any()
        assert not any(t.float().abs().sum() != 0 for t in got["dl"])
    if pattern == "big":
        assert S.big_ok(inp, logits)
    if pattern in ("big", "dead"):           # the whole-table heads on the same inputs
        assert_form(form, R, V1, d)
        check_whole(f"{pattern}.head.{NAME[form]}", (d,), inp, logits, ops.vocab_head_fwd, ops.vocab_head_bwd, dloss)
        if form == 1:                        # (vocab_ce.hip has one form)
            check_whole(f"{pattern}.vocab_ce", (d,), inp, logits, ops.vocab_ce_fwd, ops.vocab_ce_bwd, dloss)


# ---------------------------------------------------------------------- 4. voff is any vocabulary id
@pytest.mark.parametrize("form", FORMS)
def test_voff_need_not_be_aligned(form, monkeypatch):
    monkeypatch.setenv("RS_VHEAD_PP", str(form))
    ops = _ops()
    d, R, V1, v0, v1 = 256, 130, 5001, 1237, 3790
    assert v0 % 8 and (v1 - v0) % 8
    assert_form(form, R, v1 - v0, d)
    inp = S.shard_inputs(d, R, V1, 1, DEV)
    lab = inp["labels"]
    lab[1:5] = torch.tensor([v0 - 1, v0, v1 - 1, v1], device=DEV)
    logits = L.vce_logits(inp)
    live = lab != 0
    count, dloss = float(live.sum()), 0.37
    n = ops.vocab_ce_ws_numel(R, v1 - v0)
    ws = L.Guarded(n)
    lse = lse_slot(ws, R, v1 - v0)
    lse.copy_(torch.where(live, torch.logsumexp(logits[0], 1), torch.zeros((), device=DEV, dtype=torch.float64)))
    dl = L.Guarded(R, v1 - v0, BF, pitch=ceil8(v1 - v0))
    ops.vocab_head_bwd(inp["h"], inp["E"][v0:v1], inp["bias"][v0:v1], lab, ws.t, scalar(count), dl.t,
                       dloss=scalar(dloss), voff=v0)
    torch.cuda.synchronize()
    dl.check("dlogits", pads_zero_ok=True)
    res = S.check_shard_bwd(inp, logits, v0, v1, lse, count, dloss, dl.t)
    # the one-hot sits where the reference has it: rows 2 and 3 own columns 0 and v1 - v0 - 1, rows 1 and 4 none
    assert float(dl.t[2, 0]) < 0 and float(dl.t[3, v1 - v0 - 1]) < 0 and bool((dl.t[[1, 4]].float() >= 0).all())
    WORST.report("voff." + NAME[form], (d, R, v0, v1), res)


# ---------------------------------------------------------------------- bit identity (printed)
@pytest.mark.parametrize("form", FORMS)
def test_shards_against_the_whole_table(form, monkeypatch):
    """the concatenated shards' dlogits and one whole-table call fed the same lse and count: both within the bound;
    the number of elements whose bits differ is printed (module docstring)"""
    monkeypatch.setenv("RS_VHEAD_PP", str(form))
    ops = _ops()
    (N, V1, R), d, dloss = S.PATTERN_SHAPE, 256, 0.37
    inp = S.shard_inputs(d, R, V1, N, DEV, pattern="boundary")
    logits = L.vce_logits(inp)
    got, count = run_chain(inp, form, dloss)
    assert_form(form, R, V1, d)
    ws = L.Guarded(ops.vocab_ce_ws_numel(R, V1))
    lse_slot(ws, R, V1).copy_(got["lse"])
    dl = L.Guarded(R, V1, BF, pitch=ceil8(V1))
    ops.vocab_head_bwd(inp["h"], inp["E"], inp["bias"], inp["labels"], ws.t, scalar(count), dl.t, dloss=scalar(dloss))
    torch.cuda.synchronize()
    dl.check("dlogits", pads_zero_ok=True)
    WORST.report("whole." + NAME[form], (d, R, V1), S.check_shard_bwd(inp, logits, 0, V1, got["lse"], count, dloss, dl.t))
    cat = torch.cat(got["dl"], 1)
    ndiff = int((cat.contiguous().view(torch.int16) != dl.t.contiguous().view(torch.int16)).sum())
    print(f"\n{NAME[form]}: {ndiff} of {cat.numel()} dlogits differ in bits between the shards and the whole table")


# ---------------------------------------------------------------------- 5. the fallback
def chunks(v0, v1, step=4096):
    return [(c, min(c + step, v1)) for c in range(v0, v1, step)]


def logits_cols(inp, c0, c1):
    return L.vce_logits(dict(inp, E=inp["E"][c0:c1], bias=None if inp["bias"] is None else inp["bias"][c0:c1]))


def big_case(name, inp, v0, v1, rows, dloss):
    """E[v0:v1] as the table (voff = v0), rows_dev = rows.  The whole table: rs_vocab_head_fwd, then the backward from
    the lse it stored; a shard: the backward from the float64 lse of the whole vocabulary rounded to float32"""
    ops = _ops()
    R, d, V1 = inp["R"], inp["d"], inp["V1"]
    whole = (v0, v1) == (0, V1)
    lab = L.ce_live(inp, rows)
    live = (lab != 0).double()
    lse64 = torch.full((R,), -float("inf"), dtype=torch.float64, device=DEV)
    for c0, c1 in chunks(0, V1):
        lse64 = torch.logaddexp(lse64, torch.logsumexp(logits_cols(inp, c0, c1)[0], 1))
    Es, bs = inp["E"][v0:v1], inp["bias"][v0:v1]
    n = ops.vocab_ce_ws_numel(R, v1 - v0)
    ws, out, rd = L.Guarded(n), L.Guarded(3), scalar(rows, torch.int32)
    slot = lse_slot(ws, R, v1 - v0)
    if whole:
        ops.vocab_head_fwd(inp["h"], Es, bs, inp["labels"], ws.t, out.t, rows_dev=rd)
        torch.cuda.synchronize()
        out.check("out")
        count, cnt = float(out.t[1]), out.t[1:2]
    else:
        slot.copy_(lse64 * live)
        count = float(live.sum())
        cnt = scalar(count)
    lse = slot.clone()
    dl = L.Guarded(R, v1 - v0, BF, pitch=ceil8(v1 - v0))
    ops.vocab_head_bwd(inp["h"], Es, bs, inp["labels"], ws.t, cnt, dl.t, rows_dev=rd, dloss=scalar(dloss), voff=v0)
    torch.cuda.synchronize()
    dl.check("dlogits", written=rows, pads_zero_ok=True)
    assert torch.isnan(ws.full[n:]).all(), "store past the workspace"
    res, pAx = {}, torch.zeros(R, dtype=torch.float64, device=DEV)
    for c0, c1 in chunks(v0, v1):
        x, Ax = logits_cols(inp, c0, c1)
        pAx += (torch.exp(x - lse64[:, None]) * Ax).sum(1)
        for k, v in S.check_cols_bwd(inp, x, Ax, c0, c1, lse, count, dloss, dl.t[:, c0 - v0:c1 - v0], rows).items():
            res[k] = max(res.get(k, 0.0), v)
    if whole:
        b_lse = S.lse_bound_from(pAx, lse64, d)
        res["lse"] = ratio(lse, lse64 * live, b_lse * live)
        e = D(inp["E"])[lab]
        t = (D(inp["h"]) * e).sum(1) + D(inp["bias"])[lab]
        At = (D(inp["h"]) * e).abs().sum(1) + D(inp["bias"])[lab].abs()
        res.update(S.check_loss_out(out.t, lse64, b_lse, t, At, live, R, d, zero_mean=False))
    WORST.report(name, (d, R, v0, v1, rows), res)


def test_backward_fallback_to_lock_step(monkeypatch):
    monkeypatch.delenv("RS_VHEAD_PP", raising=False)
    ops = _ops()
    form = ops.vocab_head_form
    d = 256
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # one y-group needs more than half as many 256-class tiles as CUs; with two the limit is at twice the rows
    V1 = 256 * (cus // 2) + 1
    assert form(1, 64, V1, d)[2] == 1 and form(1, 64, V1 - 1, d)[2] == 2
    t = 1
    while form(1, 32 * t + 1, V1, d)[0] == 1:
        t += 1
    R = 32 * t + 1                                          # t + 1 row tiles of 32
    assert t == S.pp_tile_limit(d) and form(1, R, V1, d) == S.expected_form(1, R, V1, d, cus)
    assert form(1, R, V1, d)[0] == 0 and form(1, R - 1, V1, d)[:4] == (1, cus // 2 + 1, 1, t)
    assert form(0, R, V1, d)[0] == 1                        # the forward stays ping-pong
    print(f"\nfallback at d = {d}, {cus} CUs: R = {R}, V1 = {V1}: {form(1, R, V1, d)}")
    big_case("fallback.whole", L.vce_inputs(d, R, V1, DEV), 0, V1, R - 5, 0.37)
    # shard 1 of 2 of a vocabulary whose second shard is at least that long
    Vt = 2 * V1
    while S.ranges(Vt, 2)[1][1] - S.ranges(Vt, 2)[1][0] < V1:
        Vt += 1
    v0, v1 = S.ranges(Vt, 2)[1]
    assert v0 > 0 and form(1, R, v1 - v0, d)[0] == 0 and form(1, R - 1, v1 - v0, d)[0] == 1
    big_case("fallback.shard", L.vce_inputs(d, R, Vt, DEV), v0, v1, R - 5, 0.37)


# ---------------------------------------------------------------------- 6. the gradient glue
def test_gradient_glue(monkeypatch):
    monkeypatch.delenv("RS_VHEAD_PP", raising=False)
    from rbm_amd.models.bert_model.bert import head_dh_splits
    ops = _ops()
    (N, V1, R), d, dloss = S.PATTERN_SHAPE, 256, 0.37
    inp = S.shard_inputs(d, R, V1, N, DEV, pattern="boundary")
    got, _ = run_chain(inp, 1, dloss)
    g = L.gen_for(DEV, 37, d, R, V1)
    W0, b0 = L.rn(g, DEV, V1, d, s=0.01), L.rn(g, DEV, V1, s=0.01)
    W, b = W0.clone(), b0.clone()
    H = inp["h"]
    dH, bH = 0.0, 0.0
    for (v0, v1), dl in zip(inp["ranges"], got["dl"]):
        Wb, bb = W.clone(), b.clone()
        splits = ops.split_for(R, v1 - v0, d)
        slab = torch.full((ops.wgrad_slab_numel(R, v1 - v0, d),), float("nan"), device=DEV)
        ops.linear_wgrad(dl, H, W[v0:v1], slab, db=b[v0:v1])
        torch.cuda.synchronize()
        WORST.report("glue.wgrad", (v0, v1), S.check_wgrad(dl, H, Wb, bb, W, b, v0, v1, splits))
        Es = inp["E"][v0:v1]
        sk = head_dh_splits(v1 - v0)
        slab_d = torch.full((sk * R * d,), float("nan"), device=DEV)
        ops.gemm(dl, Es, slab_d, R, d, v1 - v0, False, True, ops.epilogue(), split_k=sk, slab=slab_d)
        dHq = L.Guarded(R, d)
        ops.reduce_slabs(slab_d, sk, dHq.t)
        torch.cuda.synchronize()
        dHq.check("dH")
        dH, bH = dH + D(dHq.t), bH + S.dh_bound(dl, Es, sk)
    full = torch.cat([D(t) for t in got["dl"]], 1)
    WORST.report("glue.dH", (N, V1, R, d), {"dH": ratio(dH, full @ D(inp["E"]), bH)})
