"""The float64 reference of the fused SAS row-chain kernels and its bound, checked without a GPU (rowchain_ref.py):
the reference against torch autograd, the bound against a float32/bf16 emulation of the kernels at every shape
of tests/test_rowchain_gpu.py (a correct kernel passes), and against mutations of that emulation (a wrong kernel
does not)."""
import math

import pytest
import torch
import torch.nn.functional as F

import rowchain_ref as R

NCU = 256   # the shapes of the kernel tests on a 256-CU part


# ------------------------------------------------------------------ the reference is right
def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("p", [0.0, 0.2])
def test_reference_matches_autograd(p):
    M, d = 37, 64
    inp = R.random_masks(R.make_inputs(M, d, p, NCU, seed=3), seed=5)
    D, k = R.D, R.kmul(p)
    me, m1, m2 = (D(inp[n]) * k for n in ("me", "m1", "m2"))
    ids, pos, neg = inp["ids"], inp["pos"], inp["neg"]
    keep, valid = (ids != 0).double()[:, None], (pos != 0).double()
    cnt = float(valid.sum())

    # ---- the stages chained in float64 with no rounding
    x0 = R.s_embed(inp["E"], inp["Ptab"], ids, inp["T"], inp["scale"], me)
    mu1, rs1 = R.s_stats(x0)
    Q = R.s_ln(x0, D(inp["ln1w"]), D(inp["ln1b"]), mu1, rs1)
    q, kv = R.s_lin(Q, inp["Wq"], inp["bq"]), R.s_lin(x0, inp["Wkv"], inp["bkv"])
    o = D(inp["o"])
    x1 = Q + R.s_lin(o, inp["Wo"], inp["bo"])
    mu2, rs2 = R.s_stats(x1)
    z = R.s_ln(x1, D(inp["ln2w"]), D(inp["ln2b"]), mu2, rs2)
    h1 = torch.relu(R.s_lin(z, inp["W1"], inp["b1"])) * m1
    xn = (R.s_lin(h1, inp["W2"], inp["b2"]) * m2 + z) * keep
    mul, rsl = R.s_stats(xn)
    f = R.s_ln(xn, D(inp["lnlw"]), D(inp["lnlb"]), mul, rsl)
    Ep, En = D(inp["E"])[pos], D(inp["E"])[neg]
    pl, nl = (f * Ep).sum(-1), (f * En).sum(-1)
    dpl, dnl = (torch.sigmoid(pl) - 1) / cnt * valid, torch.sigmoid(nl) / cnt * valid
    hdx, hg, hb = R.s_ln_bwd(dpl[:, None] * Ep + dnl[:, None] * En, xn, D(inp["lnlw"]), mul, rsl)
    loss = ((R.softplus(-pl) + R.softplus(nl)) * valid).sum() / cnt
    dzres = hdx * keep
    dy2 = dzres * m2
    da1 = R.s_lin(dy2, inp["W2T"]) * (h1 > 0).double() * m1
    dz = R.s_lin(da1, inp["W1T"]) + dzres
    dx1, g2, b2 = R.s_ln_bwd(dz, x1, D(inp["ln2w"]), mu2, rs2)
    dout = R.s_lin(dx1, inp["WoT"])
    delta = (dout * o).sum(-1)
    dq, dkv = D(inp["dq"]), D(inp["dkv"])
    W = inp["WinT"]
    dQ = dx1 + R.s_lin(dq, W[:, :d])
    t, g1, b1 = R.s_ln_bwd(dQ, x0, D(inp["ln1w"]), mu1, rs1)
    dx = R.s_lin(dkv[:, :d], W[:, d:2 * d]) + R.s_lin(dkv[:, d:], W[:, 2 * d:]) + t

    # ---- the same block written plainly, differentiated by autograd
    leaf = {n: D(inp[n]).clone().requires_grad_() for n in ("ln1w", "ln1b", "ln2w", "ln2b", "lnlw", "lnlb", "o")}
    tpos = torch.arange(M) % inp["T"]
    ax0 = ((D(inp["E"])[ids] * inp["scale"] + D(inp["Ptab"])[tpos]) * me * keep).requires_grad_()
    aQ = F.layer_norm(ax0, (d,), leaf["ln1w"], leaf["ln1b"], R.EPS)
    aq = F.linear(aQ, D(inp["Wq"]), D(inp["bq"]))
    akv = F.linear(ax0, D(inp["Wkv"]), D(inp["bkv"]))
    ax1 = aQ + F.linear(leaf["o"], D(inp["Wo"]), D(inp["bo"]))
    az = F.layer_norm(ax1, (d,), leaf["ln2w"], leaf["ln2b"], R.EPS)
    ah1 = torch.relu(F.linear(az, D(inp["W1"]), D(inp["b1"])) * m1)
    axn = (F.linear(ah1, D(inp["W2"]), D(inp["b2"])) * m2 + az) * keep
    af = F.layer_norm(axn, (d,), leaf["lnlw"], leaf["lnlb"], R.EPS)
    apl, anl = (af * Ep).sum(-1), (af * En).sum(-1)
    vi = pos != 0
    aloss = (F.binary_cross_entropy_with_logits(apl[vi], torch.ones_like(apl[vi]), reduction="sum")
             + F.binary_cross_entropy_with_logits(anl[vi], torch.zeros_like(anl[vi]), reduction="sum")) / cnt
    for tsr in (ax1, axn, apl, anl):
        tsr.retain_grad()
    # the attention core is not part of the kernels: its gradients dq, dkv enter as given cotangents
    total = aloss + (aq * dq).sum() + (akv * dkv).sum()
    total.backward()

    pairs = {"x0": (x0, ax0), "Q": (Q, aQ), "q": (q, aq), "kv": (kv, akv), "x1": (x1, ax1), "z": (z, az),
             "h1": (h1, ah1), "xn": (xn, axn), "f": (f, af), "pl": (pl, apl), "nl": (nl, anl), "loss": (loss, aloss),
             "head dpl": (dpl, apl.grad), "head dnl": (dnl, anl.grad), "head dx": (hdx, axn.grad),
             "lnl dgamma": (hg.sum(0), leaf["lnlw"].grad), "lnl dbeta": (hb.sum(0), leaf["lnlb"].grad),
             "dx1": (dx1, ax1.grad), "dout": (dout, leaf["o"].grad), "delta": (delta, (leaf["o"].grad * o).sum(-1)),
             "ln2 dgamma": (g2.sum(0), leaf["ln2w"].grad), "ln2 dbeta": (b2.sum(0), leaf["ln2b"].grad),
             "dx": (dx, ax0.grad), "ln1 dgamma": (g1.sum(0), leaf["ln1w"].grad),
             "ln1 dbeta": (b1.sum(0), leaf["ln1b"].grad),
             "mean": (mu2[:, 0], ax1.mean(-1)), "rstd": (rs2[:, 0], 1 / torch.sqrt(ax1.var(-1, unbiased=False) + R.EPS))}
    worst = {n: _rel(a, b.detach()) for n, (a, b) in pairs.items()}
    print("reference vs autograd, p =", p, max(worst.items(), key=lambda kv: kv[1]))
    assert max(worst.values()) <= 1e-12, {n: v for n, v in worst.items() if v > 1e-12}


# ------------------------------------------------------------------ tile dealing
@pytest.mark.parametrize("ncu", [256, 304, 64, 20])
def test_dealing_model_owns_every_tile_once(ncu):
    for M in [m for ms in R.case_rows(ncu).values() for m in ms]:
        nt = -(-M // 16)
        seen = sorted(t for r in R.wave_tiles(M, ncu).values() for t in r)
        assert seen == list(range(nt)), (M, ncu)
    counts = [len(r) for r in R.wave_tiles(R.case_rows(ncu)[5][0], ncu).values()]
    assert min(counts) >= 2 and max(counts) >= 3, (ncu, min(counts), max(counts))


# ------------------------------------------------------------------ the bound admits a correct kernel
def _emulate_and_check(inp, every_form=True):
    res = {}
    x0 = R.emu_embed(inp)
    res["in_embed"] = {**R.check_embed(inp, x0), **R.check_block_in(inp, R.emu_block_in(inp, x0["x0"]), x0["x0"])}
    res["out_head"] = R.check_block_out(inp, R.emu_block_out(inp, head=True), head=True)
    if every_form:      # the same stages again: from a given x, without the head, with a given divisor
        res["in"] = R.check_block_in(inp, R.emu_block_in(inp))
        res["out"] = R.check_block_out(inp, R.emu_block_out(inp))
        res["out_head_div"] = R.check_block_out(inp, R.emu_block_out(inp, head=True, divisor=3.0), head=True,
                                                divisor=3.0)
    res["out_bwd"] = R.check_block_out_bwd(inp, R.emu_block_out_bwd(inp, delta=True))
    res["in_bwd"] = R.check_block_in_bwd(inp, R.emu_block_in_bwd(inp))
    return res


def _cases():
    rows = R.case_rows(NCU)
    small = [m for c in (1, 2, 3, 4) for m in rows[c]]
    return [(M, d, p) for d in (64, 128) for M in small for p in (0.0, 0.2)] + [(rows[5][0], d, 0.2) for d in (64, 128)]


@pytest.mark.parametrize("M,d,p", _cases())
def test_bound_admits_the_emulation(M, d, p):
    inp = R.random_masks(R.make_inputs(M, d, p, NCU, seed=1))
    res = _emulate_and_check(inp, every_form=M < 10000)
    worst = {k: max(v.items(), key=lambda kv: kv[1]) for k, v in res.items()}
    print("emulation err/bound", (M, d, p), worst)
    bad = {(k, n): v for k, r in res.items() for n, v in r.items() if not v <= 1.0}
    assert not bad, bad


# ------------------------------------------------------------------ the bound rejects a wrong kernel
@pytest.fixture(scope="module")
def mut():
    M, d = 16 * 13 - 3, 64
    return R.random_masks(R.make_inputs(M, d, 0.2, NCU, seed=2))


def _fails(res):
    return [n for n, v in res.items() if not v <= 1.0]


def test_rejects_swapped_rows(mut):
    for n in ("Q", "q", "kv"):
        out = R.emu_block_in(mut)
        assert not _fails(R.check_block_in(mut, out))
        out[n][[60, 61]] = out[n][[61, 60]]
        assert n in _fails(R.check_block_in(mut, out)), n
    for n in ("x1", "z", "h1", "xn", "f", "dx"):
        out = R.emu_block_out(mut, head=True)
        out[n][[60, 61]] = out[n][[61, 60]]
        assert n in _fails(R.check_block_out(mut, out, head=True)), n
    for n in ("dy2", "da1", "dx1", "dout"):
        out = R.emu_block_out_bwd(mut)
        out[n][[60, 61]] = out[n][[61, 60]]
        assert n in _fails(R.check_block_out_bwd(mut, out)), n
    out = R.emu_block_in_bwd(mut)
    out["dx"][[60, 61]] = out["dx"][[61, 60]]
    assert "dx" in _fails(R.check_block_in_bwd(mut, out))


def test_rejects_flipped_dropout_bit_in_last_row(mut):
    row = mut["M"] - 1
    base = dict(mut)
    base["ids"] = mut["ids"].clone()
    base["ids"][row] = 5                  # a last row that the padding mask leaves visible
    for site, fn, chk, name in (("m1", R.emu_block_out, R.check_block_out, "h1"),
                                ("m2", R.emu_block_out, R.check_block_out, "xn"),
                                ("m2", R.emu_block_out_bwd, R.check_block_out_bwd, "dy2"),
                                ("m1", R.emu_block_out_bwd, R.check_block_out_bwd, "da1"),
                                ("me", R.emu_embed, R.check_embed, "x0")):
        good = fn(base)[name]
        assert not _fails(chk(base, fn(base)))
        # the first column where the flip shows (h1 / da1 are zero either way where the relu is inactive)
        col = next(c for c in range(mut["d"]) if good[row, c] != 0)
        wrong = dict(base)
        wrong[site] = base[site].clone()
        wrong[site][row, col] = ~wrong[site][row, col]
        out = fn(wrong)
        assert not torch.equal(out[name], good)
        assert name in _fails(chk(base, out)), (site, name)


def test_rejects_tile_left_out_of_partials(mut):
    assert any(n.startswith("lnpart") for n in _fails(
        R.check_block_out(mut, R.emu_block_out(mut, head=True, skip_tile=7), head=True)))
    assert any(n.startswith("part") for n in _fails(
        R.check_block_out_bwd(mut, R.emu_block_out_bwd(mut, skip_tile=7))))
    assert any(n.startswith("part") for n in _fails(R.check_block_in_bwd(mut, R.emu_block_in_bwd(mut, skip_tile=7))))


@pytest.fixture(scope="module")
def big():
    rows = R.case_rows(NCU)
    return {c: R.random_masks(R.make_inputs(rows[c][0], 64, 0.2, NCU, seed=2)) for c in (4, 5)}


@pytest.mark.parametrize("kernel", ["out_bwd", "in_bwd", "out_head"])
@pytest.mark.parametrize("case,iteration", [(4, 0), (5, 1), (5, 2)])
def test_rejects_tile_left_out_at_the_multi_tile_shapes(big, kernel, case, iteration):
    """one tile of a wave's first (case 4), second and third (case 5) loop iteration missing from the LayerNorm
    partials: the per-workgroup comparison rejects it where the sum over all workgroups hides it"""
    inp = big[case]
    it = R.tile_owner(inp["M"], NCU)[1]
    assert max(it) == (0 if case == 4 else 2)
    cand = [t for t, k in enumerate(it) if k == iteration]
    tile = cand[len(cand) // 2]
    emu, chk, names = {"out_bwd": (R.emu_block_out_bwd, R.check_block_out_bwd, ("part.g/wg", "part.b/wg")),
                       "in_bwd": (R.emu_block_in_bwd, R.check_block_in_bwd, ("part.g/wg", "part.b/wg")),
                       "out_head": (lambda i, **k: R.emu_block_out(i, head=True, **k),
                                    lambda i, o: R.check_block_out(i, o, head=True),
                                    ("lnpart.g/wg", "lnpart.b/wg"))}[kernel]
    res = chk(inp, emu(inp, skip_tile=tile))
    print(kernel, inp["M"], "tile", tile, "iteration", iteration, {n: round(res[n], 2) for n in names})
    assert all(n in _fails(res) for n in names), {n: res[n] for n in names}


def test_rejects_exchanged_weight_rows(mut):
    """two weight rows exchanged while staging = two output features exchanged in every row"""
    for W, fn, chk, name in (("Wq", R.emu_block_in, R.check_block_in, "q"),
                             ("Wkv", R.emu_block_in, R.check_block_in, "kv"),
                             ("Wo", R.emu_block_out, R.check_block_out, "x1"),
                             ("W1", R.emu_block_out, R.check_block_out, "h1"),
                             ("W2", R.emu_block_out, R.check_block_out, "xn"),
                             ("W2T", R.emu_block_out_bwd, R.check_block_out_bwd, "da1"),
                             ("W1T", R.emu_block_out_bwd, R.check_block_out_bwd, "dx1"),
                             ("WoT", R.emu_block_out_bwd, R.check_block_out_bwd, "dout"),
                             ("WinT", R.emu_block_in_bwd, R.check_block_in_bwd, "dx")):
        wrong = dict(mut)
        wrong[W] = mut[W].clone()
        wrong[W][[9, 10]] = wrong[W][[10, 9]]
        assert name in _fails(chk(mut, fn(wrong))), W


def test_rejects_skipped_padding_mask(mut):
    row = 33                                         # ids == 0 there (the zero tile)
    assert mut["ids"][row] == 0
    wrong = dict(mut)
    wrong["ids"] = mut["ids"].clone()
    wrong["ids"][row] = 1
    out, good = R.emu_block_out(wrong), R.emu_block_out(mut)
    out = {**good, "xn": torch.cat([good["xn"][:row], out["xn"][row:row + 1], good["xn"][row + 1:]])}
    assert _fails(R.check_block_out(mut, out)) == ["xn"]     # the last stage: nothing reads it
    out, good = R.emu_block_out_bwd(wrong), R.emu_block_out_bwd(mut)
    out = {**good, "dy2": torch.cat([good["dy2"][:row], out["dy2"][row:row + 1], good["dy2"][row + 1:]])}
    assert "dy2" in _fails(R.check_block_out_bwd(mut, out))     # (its reader da1 fails with it)
    out, good = R.emu_embed(wrong), R.emu_embed(mut)
    assert _fails(R.check_embed(mut, out)) == ["x0"]


def test_rejects_two_ulps(mut):
    """one element moved by 2 bf16 ulps.  The bound is 2 x 2^-8 |r| plus the accumulation term, and 2 ulps are
    2^-6 / m of |r| for a significand m in [1, 2): an element with m < 1.25 is outside it by a factor of ~1.5."""
    out = R.emu_block_in(mut)
    Q = out["Q"].float()
    m = Q.abs() / 2.0 ** torch.floor(torch.log2(Q.abs()))
    i, j = (t[0].item() for t in torch.nonzero((m < 1.25) & (Q.abs() > 0.5), as_tuple=True))
    bits = out["Q"].view(torch.int16)
    bits[i, j] += 2
    assert abs(float(out["Q"][i, j]) - float(Q[i, j])) == 2 * 2.0 ** (math.floor(math.log2(abs(float(Q[i, j])))) - 7)
    assert "Q" in _fails(R.check_block_in(mut, out))                # (its reader q fails with it)
