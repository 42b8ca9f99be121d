"""The float64 reference of the attention kernels and its per-element bound, checked without a GPU (attn_ref.py):
the reference against torch autograd, the regime of every row of the shape matrix (rs_attn_lds_regime, host only),
the bound against a float32/bf16 emulation of the LDS kernels at every shape of tests/test_attention_ref_gpu.py (a
correct kernel passes) and against mutations of that emulation (a wrong kernel does not).

Emulation, worst err / bound over the whole matrix (dropout 0 and 0.2, with and without a given delta):
    lse 0.035   o 0.47   delta 0.029   dq 0.47   dk 0.47   dv 0.48
(0.5 is a bf16 output's own worst rounding under the factor 2.)

Mutations: the factor by which each breaks the bound (inf: a NaN prefill left in place, or an error where the
bound is 0), and whether the whole-tensor criterion of tests/test_attention_gpu.py (rel < 2e-2 for o, < 4e-2 for a
gradient, against the exact reference) would have accepted the mutant.  At (3, 2, 64, 33) one tile is 1/18 of the
tensor, so that criterion sees most faults; in one late tile of the bench shape (65, 1, 128, 200) it sees none:
     1  causal diagonal off by one in one tile, (3, 2, 64, 33) tile 1:
            forward +1: 1.7e3 (old: rejects)   -1: 7.3e3 (rejects)      dQ +1: 48 (ACCEPTS)   -1: 53 (rejects)
            dK/dV   +1: 3.9e3 (ACCEPTS)        -1: 64 (rejects)
        the same in tile 11 of (65, 1, 128, 200):
            forward +1: 86 (ACCEPTS)           -1: 38 (ACCEPTS)         dQ +1: 32 (ACCEPTS)   -1: 4.2 (ACCEPTS)
            dK/dV   +1: 1.1e3 (ACCEPTS)        -1: 53 (ACCEPTS)
     2  dQ reader without the writer's slot, (9, 8, 32, 113)       61 (ACCEPTS)
     3  dK/dV reader without the writer's slot, (9, 8, 32, 113)    40 (rejects)
     4  a wave's second tile not run: forward (32, 8, 32, 144), dQ and dK/dV (9, 8, 32, 200) key padding
                                                                   inf each (rejects: a NaN in the norm)
     5  dropout pitch T at odd T, (3, 2, 64, 33)                   inf (rejects)
     6  keys >= T not masked, (3, 2, 64, 17) key padding           3.1e4 (rejects)
     7  lse / delta of the neighbouring head, (3, 2, 64, 33)       lse 1.1e4, delta 2.3e4 (rejects both)
     8  workgroup -> (b, h) of the other branch, (8, 1, 128, 200)  an equivalent mutant, see the test; its harmful
                                                                   variant: inf (rejects)
     9  dS kept on -1e9 keys, all-padding sequence, (3, 2, 64, 37) inf (rejects)
    10  lse in log2 units, (3, 2, 64, 17)                          2.9e4 on lse itself, which the old test never
                                                                   read (it rejects the emulation's gradients, which
                                                                   take the stored value for a natural logarithm)
"""
import math

import pytest
import torch

import attn_ref as R
from conftest import rel

MATRIX = [(purpose, shape, mk, want) for purpose, shape, mks, want in R.SHAPES for mk in mks]
IDS = [f"{s[0]}x{s[1]}x{s[2]}x{s[3]}-m{mk}" for _, s, mk, _ in MATRIX]


# ------------------------------------------------------------------ the reference is right
@pytest.mark.parametrize("mask_kind", [0, 1])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_reference_matches_autograd(mask_kind, p):
    c = R.Case(3, 2, 32, 37, mask_kind)
    inp = R.make_inputs(c, seed=3)
    m = R.random_mult(c, p, seed=5).double()
    q, k, v = (R.D(R.heads(t, c)).requires_grad_() for t in (inp["q"], inp["kv"][:, :c.d], inp["kv"][:, c.d:]))
    s = c.scale * (q @ k.transpose(1, 2))
    if mask_kind == 0:
        s = s.masked_fill(torch.triu(torch.ones(c.T, c.T, dtype=torch.bool), 1), -math.inf)
    else:
        s = s.masked_fill((inp["ids"] == 0).view(c.B, 1, 1, c.T).expand(-1, c.H, -1, -1).reshape(c.BH, 1, c.T), -1e9)
    o = (torch.softmax(s, -1) * m) @ v
    dO = R.D(R.heads(inp["do"], c))
    o.backward(dO)
    f = R.ref_fwd(c, inp, m)
    b = R.ref_bwd(c, inp, m, f["lse"], (dO * f["o"]).sum(-1))
    pairs = {"o": (f["o"], o), "lse": (f["lse"][..., 0], torch.logsumexp(s, -1)), "dq": (b["dq"], q.grad),
             "dk": (b["dk"], k.grad), "dv": (b["dv"], v.grad)}
    worst = {n: float((a - r.detach()).abs().max() / r.detach().abs().max()) for n, (a, r) in pairs.items()}
    print("reference vs autograd", mask_kind, p, worst)
    assert max(worst.values()) <= 1e-12, worst


# ------------------------------------------------------------------ every row of the matrix is in its regime
@pytest.mark.parametrize("purpose,shape,mask_kind,want", MATRIX, ids=IDS)
def test_regime_of_the_shape_matrix(purpose, shape, mask_kind, want):
    R.assert_regime(R.Case(*shape, mask_kind), purpose, want)


def test_regime_of_the_other_cases():
    for shape in R.ALL_PAD:
        assert R.regime(R.Case(*shape, 1))[0] == 1
    for B, H, Dh, T, mk, _ in R.TIER2_F32:
        assert R.regime(R.Case(B, H, Dh, T, mk), 0) == (0, 0, 0, 0, 0)
    for B, H, Dh, T, mk, _ in R.TIER2_BF16:
        assert R.regime(R.Case(B, H, Dh, T, mk)) == (0, 0, 0, 0, 0)
    # the plan / no-plan boundaries lie where the matrix puts them
    assert [R.regime(R.Case(9, 8, 32, T, 0))[3] for T in (112, 113)] == [0, 1]
    assert [R.regime(R.Case(65, 1, 128, T, 0))[3:] for T in (224, 225)] == [(1, 1), (0, 0)]


# ------------------------------------------------------------------ the bound admits a correct kernel
def emulate_and_check(c, inp, m, mut={}, m_emu=None, given_delta=False):
    """{output: worst err / bound} of the emulation (with the faults of mut) and its outputs"""
    me = m if m_emu is None else m_emu
    f = R.emu_fwd(c, inp, me, mut)
    res = R.check_fwd(c, inp, m, f)
    if given_delta:
        delta = (R.heads(inp["do"], c).float() * R.heads(f["o"], c).float()).sum(-1).reshape(-1)
        b = R.emu_bwd(c, inp, me, f["lse"], delta=delta, mut=mut)
        res.update(R.check_bwd(c, inp, m, f["lse"], delta, b))
    else:
        b = R.emu_bwd(c, inp, me, f["lse"], o=f["o"], mut=mut)
        res.update(R.check_bwd(c, inp, m, f["lse"], b["delta"], b, o_st=f["o"]))
    return {k: r for k, (r, _) in res.items()}, {**f, **b}


@pytest.mark.parametrize("purpose,shape,mask_kind,want", MATRIX, ids=IDS)
def test_emulation_is_inside_the_bound(purpose, shape, mask_kind, want):
    c = R.Case(*shape, mask_kind)
    inp = R.make_inputs(c)
    for p, given in ((0.0, False), (0.2, False), (0.2, True)):
        res, _ = emulate_and_check(c, inp, R.random_mult(c, p), given_delta=given)
        print(shape, mask_kind, p, given, {k: round(r, 3) for k, r in res.items()})
        assert max(res.values()) <= 1.0, res


@pytest.mark.parametrize("shape", R.ALL_PAD)
def test_emulation_of_an_all_padding_sequence(shape):
    c = R.Case(*shape, 1)
    inp = R.make_inputs(c, all_pad=True)
    res, out = emulate_and_check(c, inp, R.random_mult(c, 0.2))
    assert max(res.values()) <= 1.0, res
    rows = slice(c.T, 2 * c.T)
    assert not out["dq"][rows].any() and not out["dkv"][rows, :c.d].any()
    assert out["dkv"][rows, c.d:].any()


# ------------------------------------------------------------------ the bound rejects a wrong kernel
def old_criterion_accepts(c, inp, m, out):
    """tests/test_attention_gpu.py's criterion on the mutant's outputs: rel < 2e-2 for o, < 4e-2 for a gradient"""
    f = R.ref_fwd(c, inp, m)
    b = R.ref_bwd(c, inp, m, f["lse"], (R.D(R.heads(inp["do"], c)) * f["o"]).sum(-1))
    pairs = [(out["o"], f["o"], 2e-2), (out["dq"], b["dq"], 4e-2), (out["dkv"][:, :c.d], b["dk"], 4e-2),
             (out["dkv"][:, c.d:], b["dv"], 4e-2)]
    return all(rel(R.heads(a, c).double().numpy(), r.numpy()) < tol for a, r, tol in pairs)


def reject(name, c, inp, m, mut, m_emu=None):
    res, out = emulate_and_check(c, inp, m, mut, m_emu)
    base, _ = emulate_and_check(c, inp, m)
    assert max(base.values()) <= 1.0, base
    factor = max(res.values())
    print(f"mutation {name}: {factor:.3g} x bound ({max(res, key=res.get)}); the old criterion "
          f"{'ACCEPTS' if old_criterion_accepts(c, inp, m, out) else 'rejects'} it")
    assert factor >= 4.0, (name, res)


def _one_tile(c, bh, tile, which, step):
    """a causal mask wrong by one in one tile: step +1 lets key q + 1 through, -1 blocks the diagonal; which: the tile is
    of queries (forward, dQ pass) or of keys (dK/dV pass)"""
    r = torch.arange(c.T)
    wrong = (r[None, :] > r[:, None] + step)

    def f(dead):
        sl = slice(16 * tile, 16 * tile + 16)
        if which == "keys":
            dead[bh, :, sl] = wrong[:, sl]
        else:
            dead[bh, sl, :] = wrong[sl, :]
        return dead
    return f


@pytest.mark.parametrize("step", [1, -1])
@pytest.mark.parametrize("where", ["dead_fwd", "dead_dq", "dead_dkv"])
@pytest.mark.parametrize("shape,tile", [((3, 2, 64, 33), 1), ((65, 1, 128, 200), 11)])
def test_mutation_1_causal_diagonal_off_by_one_in_one_tile(shape, tile, where, step):
    """at the smallest shape that shows it, and in a late tile of the bench shape, where the whole-tensor criterion
    no longer sees it"""
    c = R.Case(*shape, 0)
    inp = R.make_inputs(c)
    mut = {where: _one_tile(c, 3, tile, "keys" if where == "dead_dkv" else "queries", step)}
    reject(f"1 {shape} {where} {step:+d}", c, inp, R.random_mult(c, 0.0), mut)


def _writer_item(c, dkv):
    return next(it for it in R.plan_items(c.B, c.T, c.H, dkv)[0] if it[6] == 1)


@pytest.mark.parametrize("dkv", [False, True])
def test_mutation_2_3_reader_stores_without_the_writers_slot(dkv):
    c = R.Case(9, 8, 32, 113, 0)                      # the smallest shape with a plan
    assert R.regime(c)[3:] == (1, 1)
    inp = R.make_inputs(c)
    _, _, _, tile, cb, ce, _, _ = _writer_item(c, dkv)
    skip = torch.zeros(c.BH, c.T, c.T, dtype=torch.bool)
    if dkv:
        skip[5, 32 * cb:32 * ce, 16 * tile:16 * tile + 16] = True
    else:
        skip[5, 16 * tile:16 * tile + 16, 32 * cb:32 * ce] = True
    reject("3" if dkv else "2", c, inp, R.random_mult(c, 0.0), {"skip_dkv" if dkv else "skip_dq": skip})


@pytest.mark.parametrize("which", ["skip_fwd", "skip_dq_tile", "skip_dkv_tile"])
def test_mutation_4_a_waves_second_tile_not_run(which):
    # forward: B*H >= 256 and 9 tiles; backward: key padding (no plan) and 13 tiles; tile 8 is wave 0's second
    c = R.Case(32, 8, 32, 144, 1) if which == "skip_fwd" else R.Case(9, 8, 32, 200, 1)
    assert c.nq > R.NW * R.regime(c)[1 if which == "skip_fwd" else 2] and R.regime(c)[3] == 0
    inp = R.make_inputs(c)
    reject(f"4 {which}", c, inp, R.random_mult(c, 0.0), {which: [(c.BH - 3, 8)]})


def test_mutation_5_dropout_pitch_T_at_odd_T():
    c = R.Case(3, 2, 64, 33, 0)
    inp = R.make_inputs(c)
    reject("5", c, inp, R.random_mult(c, 0.2), {}, m_emu=R.random_mult(c, 0.2, pitch=c.T))


def test_mutation_6_keys_past_T_not_masked():
    c = R.Case(3, 2, 64, 17, 1)                       # key padding: a causal mask would hide the keys past T
    inp = R.make_inputs(c)
    reject("6", c, inp, R.random_mult(c, 0.0), {"extra_keys": True})


@pytest.mark.parametrize("which", ["lse", "delta"])
def test_mutation_7_row_statistic_of_the_neighbouring_head(which):
    c = R.Case(3, 2, 64, 33, 0)
    inp = R.make_inputs(c)
    reject(f"7 {which}", c, inp, R.random_mult(c, 0.0), {"row_perm": (which, torch.arange(c.BH) ^ 1)})


def test_mutation_8_workgroup_to_sequence_head_mapping():
    """As stated -- the plain branch of block_coords taken where BH % 8 == 0 -- the mutation changes no output: both
    branches map the workgroups one to one onto the (sequence-head, split) pairs, and a workgroup's work depends on
    the pair alone, so this is asserted as an equivalence.  Its harmful variant, the sequence-head of one branch with
    the split of the other, leaves pairs without a workgroup, and their tiles keep the NaN prefill."""
    c = R.Case(8, 1, 128, 200, 0)
    ns = R.regime(c)[2]
    assert c.BH % 8 == 0 and ns == 2
    pairs = {(bh, sp) for bh in range(c.BH) for sp in range(ns)}
    for swz in (False, True):
        assert {R.block_coords(c.BH, ns, lin, swz) for lin in range(c.BH * ns)} == pairs
    hybrid = {(R.block_coords(c.BH, ns, lin, False)[0], R.block_coords(c.BH, ns, lin, True)[1])
              for lin in range(c.BH * ns)}
    lost = sorted(pairs - hybrid)
    assert lost
    inp = R.make_inputs(c)
    reject("8 (hybrid)", c, inp, R.random_mult(c, 0.0),
           {"skip_dq_tile": [(bh, t) for bh, sp in lost for t in range(sp, c.nq, ns)]})


def test_mutation_9_dS_kept_on_filled_keys_of_an_all_padding_sequence():
    c = R.Case(3, 2, 64, 37, 1)
    inp = R.make_inputs(c, all_pad=True)
    reject("9", c, inp, R.random_mult(c, 0.0), {"ds_fill": True})


def test_mutation_10_lse_in_log2_units():
    c = R.Case(3, 2, 64, 17, 0)
    inp = R.make_inputs(c)
    reject("10", c, inp, R.random_mult(c, 0.0), {"lse_log2": True})
