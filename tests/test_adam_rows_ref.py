"""CPU checks of the sparse (touched-rows-only) Adam: the float32 emulation of tests/adam_rows_ref.py is held to the
GPU tests' bounds against the float64 reference, the same checks reject every planted mistake, the ops wrappers
validate their arguments before any launch, and the entries exist in the header and the ctypes mirror."""
import os
import re

import numpy as np
import pytest
import torch

import adam_rows_ref as R
from conftest import ROOT

HYPER = (1e-3, 0.9, 0.999, 1e-8, 0.0)


def run(steps_data, init, dtype, mistake=None, check_each=False):
    """The scenario through sparse_step; returns (final table, per-step touched rows, problems found on the way)."""
    p, m, v = init
    tab = R.Table(p, np.zeros_like(p), m, v, dtype)
    problems, touched = [], []
    for t, (lists, g, lr) in enumerate(steps_data, 1):
        ids = np.concatenate(lists)
        rows = np.unique(ids[(ids >= 1) & (ids < p.shape[0])])
        tab.g[rows] = g[rows]
        before = tab.copy() if check_each else None
        R.sparse_step(tab, lists, t, (lr,) + HYPER[1:], mistake=mistake)
        touched.append(rows)
        if check_each:
            problems += R.check_untouched(before, tab, rows)
            if np.count_nonzero(tab.g[rows]):
                problems.append("gradient of a touched row not cleared")
    return tab, touched, problems


LONG = R.LONG


def test_fp32_emulation_holds_the_bounds_against_fp64():
    init, data = R.scenario(**LONG)
    ref, _, _ = run(data, init, np.float64)
    emu, touched, problems = run(data, init, np.float32, check_each=True)
    errs = R.state_errors(emu, ref)
    print("fp32 emulation vs fp64 after 300 steps (ulps):", errs,
          "max updates of a row:", int(np.bincount(np.concatenate(touched)).max()))
    assert not problems, problems[:5]
    assert not R.check_state(emu, ref), (R.check_state(emu, ref), errs)


def test_fp32_emulation_holds_the_bounds_with_two_lists_and_tiny_moments():
    init, data = R.scenario(seed=5, R=97, d=12, steps=6, per_step=9, tiny_cols=4, lists=2)
    ref, _, _ = run(data, init, np.float64)
    emu, _, problems = run(data, init, np.float32, check_each=True)
    assert not problems and not R.check_state(emu, ref), (problems, R.check_state(emu, ref), R.state_errors(emu, ref))


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_the_checks_reject_a_planted_mistake(mistake):
    """Each mistake, planted into the float32 emulation, fails at least one of the checks the GPU tests apply (and
    the unplanted emulation of the same scenario passes them: the test above)."""
    init, data = R.scenario(seed=5, R=97, d=12, steps=6, per_step=9, tiny_cols=4, lists=2)
    ref, _, _ = run(data, init, np.float64)
    emu, touched, problems = run(data, init, np.float32, mistake=mistake, check_each=True)
    problems += R.check_state(emu, ref)
    print(mistake, "->", sorted(set(problems)), R.state_errors(emu, ref))
    assert problems, mistake
    want = {"decay_untouched": "untouched rows changed", "no_clear": "not cleared", "stale_bf16": "bf16 copy",
            "twice": "ulps", "per_row_step": "ulps", "eps_sparse_adam": "ulps"}[mistake]
    assert any(want in x for x in problems), (mistake, problems)


def test_touched_set_is_by_id_not_by_value():
    """A listed row whose gradient is exactly zero is still updated (m decays, p moves); an unlisted one is not."""
    rng = np.random.default_rng(0)
    p, m = rng.standard_normal((5, 4)).astype(np.float32), rng.standard_normal((5, 4)).astype(np.float32)
    v = rng.random((5, 4)).astype(np.float32)
    tab = R.Table(p, np.zeros_like(p), m, v, np.float32)
    before = tab.copy()
    rows = R.sparse_step(tab, [np.array([3, 3, 0, 9])], 1, HYPER)
    assert rows.tolist() == [3]
    assert not R.check_untouched(before, tab, rows)
    assert not R.same_bits(before.m[3], tab.m[3]) and not R.same_bits(before.p[3], tab.p[3])


def test_bf16_round_matches_torch():
    x = np.random.default_rng(1).standard_normal(4096).astype(np.float32) * 37.0
    assert R.same_bits(R.bf16_round(x), torch.from_numpy(x).bfloat16().float().numpy())


# ------------------------------------------------------------------ the boundary
def test_symbols_in_header_and_lib():
    import rbm_amd._lib as L
    text = open(os.path.join(ROOT, "include", "recsys_hip.h")).read()
    for name in ("rs_unique_rows", "rs_unique_rows_ws_bytes", "rs_adam_rows"):
        assert re.search(rf"^(?:int|int64_t) {name}\(", text, flags=re.M), name
        assert name in L.SIGNATURES
        assert hasattr(L.lib(), name)
    assert L.RESTYPES["rs_unique_rows_ws_bytes"] is L.C.c_int64
    assert L.lib().rs_abi_version() == 2
    assert L.lib().rs_unique_rows_ws_bytes(1_000_000) == 4 * (1_000_000 + 2 * 489)
    assert L.lib().rs_unique_rows_ws_bytes(0) < 0


def test_ops_wrappers_validate_before_any_launch():
    """Every refusal is a ValueError raised on the host from CPU tensors: nothing reaches the library."""
    from rbm_amd import ops
    i64 = lambda n: torch.zeros(n, dtype=torch.int64)  # noqa: E731
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)  # noqa: E731
    ws = torch.zeros(ops.unique_rows_ws_bytes(100), dtype=torch.uint8)
    bad = [
        lambda: ops.unique_rows([], 100, i32(8), i32(1), ws),                          # no keys
        lambda: ops.unique_rows([i64(2)] * 4, 100, i32(8), i32(1), ws),                # four sources
        lambda: ops.unique_rows([i32(4)], 100, i32(8), i32(1), ws),                    # int32 keys
        lambda: ops.unique_rows([i64(8)[::2]], 100, i32(8), i32(1), ws),               # strided keys
        lambda: ops.unique_rows([i64(4), i64(5)], 100, i32(8), i32(1), ws),            # cap < n0 + n1
        lambda: ops.unique_rows([i64(4)], 100, i64(8), i32(1), ws),                    # int64 list
        lambda: ops.unique_rows([i64(4)], 100, i32(8), i32(2), ws),                    # count of two
        lambda: ops.unique_rows([i64(4)], 100, i32(8), i32(1), ws[:-1]),               # short workspace
        lambda: ops.unique_rows([i64(4)], 0, i32(8), i32(1), ws),                      # no table
        lambda: ops.unique_rows([i64(4)], 2 ** 31, i32(8), i32(1), ws),                # ids past int32
        lambda: ops.unique_rows_ws_bytes(0),
    ]
    f = lambda *s: torch.zeros(*s)  # noqa: E731
    st, hy = torch.zeros(144, dtype=torch.float64), torch.zeros(5, dtype=torch.float64)
    ok = dict(rows=i32(8), count=i32(1), p=f(10, 4), g=f(10, 4), m=f(10, 4), v=f(10, 4), p_bf16=None, state=st,
              hyper=hy)

    def adam(**kw):
        a = dict(ok, **kw)
        return lambda: ops.adam_rows(a["rows"], a["count"], a["p"], a["g"], a["m"], a["v"], a["p_bf16"], a["state"],
                                     a["hyper"], zero_grad=True, max_wg=a.get("max_wg"))
    bad += [adam(rows=i64(8)), adam(count=i32(2)), adam(g=f(10, 5)), adam(m=f(10, 4).double()),
            adam(v=f(10, 8)[:, ::2]), adam(p_bf16=f(10, 4)), adam(p_bf16=f(9, 4).bfloat16()),
            adam(p=f(2, 5, 2), g=f(2, 5, 2), m=f(2, 5, 2), v=f(2, 5, 2)), adam(rows=i32(0)),
            adam(state=torch.zeros(144)), adam(hyper=torch.zeros(4, dtype=torch.float64)), adam(max_wg=0),
            adam(rows=i32(2 ** 20), p=f(3, 2048), g=f(3, 2048), m=f(3, 2048), v=f(3, 2048))]   # cap * d = 2^31
    for k, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail(f"case {k} was accepted")


def test_fused_adam_refuses_what_the_sparse_rule_cannot_mean():
    """weight_decay != 0, ranges / keep beside sparse tables, a table outside the buffer or overlapping another:
    ValueError before the first launch (CPU tensors never reach a kernel)."""
    from rbm_amd.train_step import FusedAdam

    class Flat:
        device = torch.device("cpu")
        numel = 4096
    lst, cnt = torch.zeros(8, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="weight_decay"):
        FusedAdam(Flat(), weight_decay=0.01).step(sparse=[(0, 10, 4, lst, cnt)])
    opt = FusedAdam(Flat())
    for kw in (dict(ranges=[(0, 64)]), dict(keep=(64, 128))):
        with pytest.raises(ValueError, match="neither ranges nor keep"):
            opt.step(sparse=[(0, 10, 4, lst, cnt)], **kw)
    with pytest.raises(ValueError, match="not a parameter"):
        opt.step(sparse=[(32, 10, 4, lst, cnt)])           # not on an alignment boundary
    with pytest.raises(ValueError, match="not a parameter"):
        opt.step(sparse=[(4032, 100, 4, lst, cnt)])        # runs past the buffer
    with pytest.raises(ValueError, match="overlap"):
        opt.step(sparse=[(0, 100, 4, lst, cnt), (64, 10, 4, lst, cnt)])
    assert opt._sparse_segments([(64, 10, 5, lst, cnt), (1024, 3, 1, lst, cnt)]) == \
        [(0, 64, True), (128, 1024, True), (1088, 4096, True)]
    assert opt._sparse_segments([(0, 4096, 1, lst, cnt)]) == []
