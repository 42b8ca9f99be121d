"""The dropout kernels against the HOST statement of the hash (bert_rows_ref.drop_site: common.h's eff_seed, seed32,
seed_mult, pair_hash, drop_thr, drop_mul / drop_mul2 in numpy integers) -- every other dropout test of the suite draws
its masks from rs_dropout_rowmask itself -- and, bit for bit, against the float32 emulation of their one multiply and
one rounding (rs_dropout_rowmask with row ids and out_masked, rs_dropout2: bert_modules/utils/sublayer.py:18 and
transformer.py:32 backward), in guarded buffers with a leading dimension wider than the rows."""
import pytest
import torch

import bert_rows_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SALT = 0xC0FFEE0000000007        # high bits set: seed32 folds the upper word in


def _sb(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("M,N", [(5, 64), (33, 50), (7, 1023)])
def test_rowmask_over_ones_is_the_host_hash(M, N):
    """even N on the 8-column kernel, even and odd N on the element kernel (drop_ld = N: odd rows start on an odd
    index); the keep mask AND the multiplier, bit for bit"""
    import rbm_amd  # noqa: F401
    from rbm_amd import ops
    ones = torch.ones(M, N, device=DEV)
    for p in (0.1, 0.2, 0.5):
        for base in (0, 7, (3 << 40) + 11):
            for salt in (SALT, 5):
                whole, out = R.guarded(M, N, 0, torch.float32)
                ops.dropout_rowmask(ones, p, salt, _sb(base), None, out)
                torch.cuda.synchronize()
                keep, k = R.drop_site(p, salt, base, M, N, N)
                want = torch.from_numpy(keep).to(DEV).float() * k
                assert torch.equal(out, want), (p, base, hex(salt), int((out != want).sum()))
                assert R.guards_untouched(whole, (M, N))
    whole, out = R.guarded(M, N, 0, torch.float32)       # a null device seed word is seed_base = 0
    ops.dropout_rowmask(ones, 0.2, SALT, None, None, out)
    assert torch.equal(out, R.drop_mult(0.2, SALT, 0, M, N, N, DEV))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("M,N,pad", [(37, 256, 8), (70, 64, 24), (33, 50, 6), (9, 1024, 0)])
def test_dropout_kernels_equal_the_emulation(dtype, M, N, pad):
    """out = round(v m), out_masked = v with v = x or 0 on rows whose id is 0; out1 = round(x m1), out2 = round(out1
    m2): one float32 product of stored values and one rounding each, so equality is exact.  p = 0 copies."""
    import rbm_amd  # noqa: F401
    from rbm_amd import ops
    g = torch.Generator().manual_seed(M * N)
    x = torch.randn(M, N, generator=g).to(dtype).to(DEV)
    ids = (torch.rand(M, generator=g) > 0.3).long().to(DEV)
    _, xs = R.guarded_from(x, pad)
    base = (3 << 40) + 11
    for p in (0.0, 0.1, 0.5):
        m1 = R.drop_mult(p, SALT, base, M, N, N, DEV)
        m2 = R.drop_mult(p, SALT ^ 0xFF, base, M, N, N, DEV)
        for use_ids, masked in ((False, False), (True, True), (True, False)):
            wo, out = R.guarded(M, N, pad, dtype)
            wm, om = R.guarded(M, N, pad, dtype)
            ops.dropout_rowmask(xs, p, SALT, _sb(base), ids if use_ids else None, out, om if masked else None)
            torch.cuda.synchronize()
            eo, ev = R.emu_rowmask(x, ids if use_ids else None, m1)
            assert torch.equal(out, eo), (p, use_ids, int((out != eo).sum()))
            assert R.guards_untouched(wo, (M, N))
            if masked:
                assert torch.equal(om, ev) and R.guards_untouched(wm, (M, N))
            else:
                assert bool(torch.isnan(wm).all())
        if N % 8 == 0:        # rs_dropout2 takes whole 8-column chunks
            w1, o1 = R.guarded(M, N, pad, dtype)
            w2, o2 = R.guarded(M, N, pad, dtype)
            ops.dropout2(xs, p, SALT, SALT ^ 0xFF, _sb(base), o1, o2)
            torch.cuda.synchronize()
            e1, e2 = R.emu_drop2(x, m1, m2)
            assert torch.equal(o1, e1) and torch.equal(o2, e2), (p, int((o1 != e1).sum()), int((o2 != e2).sum()))
            assert R.guards_untouched(w1, (M, N)) and R.guards_untouched(w2, (M, N))
            if p > 0:
                assert not torch.equal(o1, o2)
