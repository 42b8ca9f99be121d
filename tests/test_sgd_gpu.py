"""rs_sgd_step on the GPU against the float32 emulation of tests/sgd_ref.py (which equals torch's CPU float32 SGD bit
for bit: tests/test_sgd_ref.py).  Every comparison is bitwise.  Every buffer the kernel writes sits between NaN
guards that must stay NaN; pure outputs (the bf16 copy, the transposed copies) are prefilled with NaN."""
import numpy as np
import pytest
import torch

import sgd_ref as R

pytestmark = pytest.mark.gpu

LR, GUARD, U = 0.05, 64, 2


def guarded(n, dtype=torch.float32):
    """(whole, view): n elements between two NaN guards; the view starts 16-byte aligned."""
    whole = torch.full((GUARD + n + GUARD,), float("nan"), dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def guards_intact(whole, n):
    return bool(torch.isnan(whole[:GUARD]).all()) and bool(torch.isnan(whole[GUARD + n:]).all())


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def emulate(p0, grads, mom, wd, div, lr=LR):
    s = R.scalars(lr, mom, wd, div)
    p, b = np.array(p0, np.float32), (np.zeros(len(p0), np.float32) if mom else None)
    for g in grads:
        p, b = R.update(p, g, b, s, np.float32)
    return p, b


def run_case(n, mom=0.9, wd=0.01, zero_grad=True, div=None, bf16=True, max_wg=0, steps=2, seed=0):
    import rbm_amd  # noqa: F401
    from rbm_amd import ops
    p0, grads = R.scenario(seed + n, n, steps)
    grads[-1][::7] = -0.0      # signed zeros are zeros too
    wp, p = guarded(n)
    wg, g = guarded(n)
    wb, b = guarded(n) if mom else (None, None)
    wpb, pb = guarded(n, torch.bfloat16) if bf16 else (None, None)
    p.copy_(torch.from_numpy(p0))
    if mom:
        b.zero_()
    state = torch.zeros(8, dtype=torch.float64, device="cuda")
    hyper = torch.tensor([LR, mom, wd], dtype=torch.float64, device="cuda")
    dv = torch.tensor([div], device="cuda") if div is not None else None
    for k, gr in enumerate(grads):
        g.copy_(torch.from_numpy(gr))
        ops.sgd_step(p, g, b, pb, state, hyper, zero_grad=zero_grad, prepare=True, grad_divisor=dv, max_wg=max_wg)
        torch.cuda.synchronize()
        if zero_grad:
            assert int(torch.count_nonzero(g)) == 0 and not bool(torch.isnan(g).any())
        else:
            assert torch.equal(bits(g), bits(torch.from_numpy(gr)))
    ep, eb = emulate(p0, grads, mom, wd, div)
    assert torch.equal(bits(p), bits(torch.from_numpy(ep))), "p"
    if mom:
        assert torch.equal(bits(b), bits(torch.from_numpy(eb))), "buf"
    if bf16:
        assert torch.equal(bits(pb.float()), bits(torch.from_numpy(R.bf16_round(ep)))), "bf16"
    for w in (wp, wg, wb, wpb):
        assert w is None or guards_intact(w, n)
    assert float(state[0].item()) == steps


@pytest.mark.parametrize("n,max_wg", [(1, 0), (3, 0), (4, 0), (7, 0), (4 * 256 * U + 5, 1), (4096 + 3, 0),
                                      (662_019, 0), (662_019, 1)])
def test_sizes(n, max_wg):
    """one float4 and less, both loops and the tail in one workgroup, several workgroups, cfg2's flat size"""
    run_case(n, max_wg=max_wg)


@pytest.mark.parametrize("max_wg", [0, 1, 7])
@pytest.mark.parametrize("mom", [0.0, 0.9])
def test_every_variation(mom, max_wg):
    for wd in (0.0, 0.01):
        for zero_grad in (True, False):
            for div in (None, 3.0):
                for bf16 in (True, False):
                    run_case(4096 + 3, mom=mom, wd=wd, zero_grad=zero_grad, div=div, bf16=bf16, max_wg=max_wg)


def test_prepare_counts_the_step_advances_the_seed_and_forms_the_loss():
    import rbm_amd  # noqa: F401
    from rbm_amd import ops
    n = 4096 + 3
    p = torch.randn(n, device="cuda")
    b = torch.zeros(n, device="cuda")
    state = torch.zeros(8, dtype=torch.float64, device="cuda")
    hyper = torch.tensor([LR, 0.9, 0.0], dtype=torch.float64, device="cuda")
    seed = torch.tensor([41], dtype=torch.int64, device="cuda")
    div = torch.tensor([3.0], device="cuda")
    lsum = torch.zeros(1, device="cuda")
    lout = torch.full((3,), float("nan"), device="cuda")
    for k in range(1, 4):
        lsum.fill_(0.7 * k)
        ops.sgd_step(p, torch.randn(n, device="cuda"), b, None, state, hyper, zero_grad=True, prepare=True,
                     grad_divisor=div, seed_base=seed, loss_sum=lsum, loss_out=lout[1:2])
        torch.cuda.synchronize()
        assert float(state[0].item()) == k and int(seed.item()) == 41 + k
        assert float(lout[1].item()) == float((lsum / div).item())
        assert bool(torch.isnan(lout[0])) and bool(torch.isnan(lout[2]))
    assert not bool(state[1:].any())
    before = p.clone()
    lout.fill_(float("nan"))
    ops.sgd_step(p, torch.randn(n, device="cuda"), b, None, state, hyper, zero_grad=True, prepare=False,
                 grad_divisor=div, seed_base=seed, loss_sum=lsum, loss_out=lout[1:2])
    torch.cuda.synchronize()
    assert float(state[0].item()) == 3 and int(seed.item()) == 44 and bool(torch.isnan(lout).all())
    assert not torch.equal(p, before)      # the range itself was updated


@pytest.mark.parametrize("graph", [False, True])
def test_transposed_copies_equal_a_fresh_transpose(graph):
    """two matrices inside one buffer (8 x 12 with lds 12, 64 x 128), other elements before, between and after them
    (a ragged tail among them), tbase != 0"""
    import rbm_amd  # noqa: F401
    from rbm_amd import ops
    tbase = 64
    offA, offB = tbase + 16, tbase + 16 + 96 + 20
    n = (offB - tbase) + 64 * 128 + 37
    dstB = 128
    host = [(8, 12, offA, 12, 0, 8), (64, 128, offB, 128, dstB, 64)]
    desc = torch.tensor(host, dtype=torch.int64, device="cuda")
    local = torch.tensor([(r, c, o - tbase, l, do, ld) for r, c, o, l, do, ld in host], dtype=torch.int64,
                         device="cuda")
    nT = dstB + 128 * 64
    wwT, wT = guarded(nT, torch.bfloat16)
    p0, grads = R.scenario(5, n, 3)
    wp, p = guarded(n)
    wpb, pb = guarded(n, torch.bfloat16)
    p.copy_(torch.from_numpy(p0))
    b = torch.zeros(n, device="cuda")
    g = torch.zeros(n, device="cuda")
    gsrc = torch.zeros(n, device="cuda")
    state = torch.zeros(8, dtype=torch.float64, device="cuda")
    hyper = torch.tensor([LR, 0.9, 0.01], dtype=torch.float64, device="cuda")

    def step():
        g.copy_(gsrc)
        ops.sgd_step(p, g, b, pb, state, hyper, zero_grad=True, prepare=True, transposed=(desc, host, wT),
                     tbase=tbase)
    gr = None
    if graph:
        gsrc.copy_(torch.from_numpy(grads[0]))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        gr = torch.cuda.CUDAGraph()
        state_before = (p.clone(), b.clone(), state.clone())
        with torch.cuda.graph(gr, stream=side):
            step()
        torch.cuda.synchronize()
        # a capture runs nothing
        assert torch.equal(p, state_before[0]) and torch.equal(b, state_before[1])
        assert torch.equal(state, state_before[2])
    for k in range(3):
        gsrc.copy_(torch.from_numpy(grads[k]))
        gr.replay() if graph else step()
    torch.cuda.synchronize()
    ep, _ = emulate(p0, grads, 0.9, 0.01, None)
    assert torch.equal(bits(p), bits(torch.from_numpy(ep)))
    assert torch.equal(bits(pb.float()), bits(torch.from_numpy(R.bf16_round(ep))))
    wfresh, fresh = guarded(nT, torch.bfloat16)
    ops.transpose_bf16(local, 2, pb, fresh)
    torch.cuda.synchronize()
    assert torch.equal(bits(wwT), bits(wfresh))        # the gap between the two copies and the guards: still NaN
    assert not bool(torch.isnan(wT[:96]).any()) and not bool(torch.isnan(wT[dstB:]).any())
    assert bool(torch.isnan(wT[96:dstB]).all())
    assert guards_intact(wp, n) and guards_intact(wpb, n) and guards_intact(wwT, nT)
    assert float(state[0].item()) == 3


def test_nontemporal_form_equals_the_cached_form():
    """the smallest range that takes the nontemporal loads and stores (64M elements) against a second copy of the same
    data updated as two ranges of 32M (the cached form): every element of p, buf, the bf16 copy and the gradient is
    compared, over two steps, the first on a 256-workgroup grid (the grid-stride loop's many rounds)"""
    import rbm_amd  # noqa: F401
    from rbm_amd import ops
    n = 64 << 20
    h = n // 2
    g0 = torch.Generator(device="cuda").manual_seed(7)
    p = torch.randn(n, generator=g0, device="cuda")
    p2 = p.clone()
    b, b2 = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    pb = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    pb2 = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    hyper = torch.tensor([LR, 0.9, 0.01], dtype=torch.float64, device="cuda")
    div = torch.tensor([2.0], device="cuda")
    st_big = torch.zeros(8, dtype=torch.float64, device="cuda")
    st_small = torch.zeros(8, dtype=torch.float64, device="cuda")
    for step in range(2):
        g = torch.randn(n, generator=g0, device="cuda")
        g[: n // 64] = 0.0
        g2 = g.clone()
        ops.sgd_step(p, g, b, pb, st_big, hyper, zero_grad=True, prepare=True, grad_divisor=div,
                     max_wg=256 if step == 0 else 8192)
        for lo, hi in ((0, h), (h, n)):
            ops.sgd_step(p2[lo:hi], g2[lo:hi], b2[lo:hi], pb2[lo:hi], st_small, hyper, zero_grad=True,
                         prepare=lo == 0, grad_divisor=div)
        assert int(torch.count_nonzero(g)) == 0 and int(torch.count_nonzero(g2)) == 0
        del g, g2
    torch.cuda.synchronize()
    assert torch.equal(p, p2) and torch.equal(b, b2) and torch.equal(pb, pb2)
    assert not bool(torch.isnan(p).any()) and float(b.abs().max()) > 0
    assert float(st_big[0].item()) == float(st_small[0].item()) == 2


@pytest.mark.parametrize("k", [4, 2048, 4096])
def test_a_range_split_equals_one_launch(k):
    import rbm_amd  # noqa: F401
    from rbm_amd import ops
    n = 4096 + 3
    p0, grads = R.scenario(9, n, 2)
    hyper = torch.tensor([LR, 0.9, 0.01], dtype=torch.float64, device="cuda")
    outs = []
    for split in (False, True):
        p, b = torch.from_numpy(p0).cuda(), torch.zeros(n, device="cuda")
        pb = torch.full((n,), float("nan"), dtype=torch.bfloat16, device="cuda")
        state = torch.zeros(8, dtype=torch.float64, device="cuda")
        for gr in grads:
            g = torch.from_numpy(gr).cuda()
            if split:
                ops.sgd_step(p[:k], g[:k], b[:k], pb[:k], state, hyper, zero_grad=True, prepare=True)
                ops.sgd_step(p[k:], g[k:], b[k:], pb[k:], state, hyper, zero_grad=True, prepare=False)
            else:
                ops.sgd_step(p, g, b, pb, state, hyper, zero_grad=True, prepare=True)
            assert int(torch.count_nonzero(g)) == 0
        torch.cuda.synchronize()
        outs.append((p, b, pb, state))
    for x, y in zip(*outs):
        assert torch.equal(bits(x) if x.dtype != torch.float64 else x.cpu(), bits(y) if y.dtype != torch.float64
                           else y.cpu())
    assert float(outs[0][3][0].item()) == 2
    ep, eb = emulate(p0, grads, 0.9, 0.01, None)
    assert torch.equal(bits(outs[1][0]), bits(torch.from_numpy(ep)))
    assert torch.equal(bits(outs[1][1]), bits(torch.from_numpy(eb)))
