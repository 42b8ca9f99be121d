"""rs_adam_rows / rs_unique_rows on the GPU (adam_rows.hip): the sparse Adam of a table is the dense sweep
(rs_adam_step, which replaces the reference's torch.optim.Adam, BS/trainers/base.py:225-228) on the listed rows, bit
for bit, and nothing at all on the others; 300 steps against the float64 reference of tests/adam_rows_ref.py; the
row list against numpy.unique."""
import numpy as np
import pytest
import torch

import adam_rows_ref as R

pytestmark = pytest.mark.gpu

HYPER = (1e-3, 0.9, 0.999, 1e-8, 0.0)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def make(R_, d, seed, bf16=True, offset=0):
    """p / g / m / v (+ bf16 copy) of a table [R_][d] as views `offset` floats into their allocations (offset 1: a
    base that is not 16-byte aligned), g all NaN."""
    gen = torch.Generator().manual_seed(seed)
    n = R_ * d

    def buf(x):
        full = torch.zeros(n + 8, dtype=x.dtype)
        full[offset:offset + n] = x
        return full.cuda()[offset:offset + n].view(R_, d)
    p = buf(torch.randn(n, generator=gen))
    m = buf(0.1 * torch.randn(n, generator=gen))
    v = buf(0.01 * torch.randn(n, generator=gen) ** 2 + 1e-6)
    g = buf(torch.full((n,), float("nan")))
    pb = buf(torch.zeros(n).bfloat16() + 3.0) if bf16 else None     # a stale copy: 3.0 everywhere
    return p, g, m, v, pb


def prepared(steps=3, lr=HYPER[0]):
    """Optimizer state after `steps` rs_adam_prepare launches: the scalars of step `steps` in state[1..3]."""
    from rbm_amd import ops
    st = torch.zeros(144, dtype=torch.float64, device="cuda")
    hy = torch.tensor((lr,) + HYPER[1:], dtype=torch.float64, device="cuda")
    for _ in range(steps):
        ops.adam_prepare(st, hy)
    return st, hy


def listed(rows, cap, R_):
    """int32 list [cap]: rows, then out-of-range ids and -1 past the count."""
    junk = torch.tensor([R_, -1, R_ + 5, 2 ** 31 - 1, -(2 ** 31)], dtype=torch.int64).repeat(cap // 5 + 1)
    lst = torch.cat([torch.as_tensor(rows, dtype=torch.int64), junk])[:cap].to(torch.int32).cuda()
    return lst, torch.tensor([len(rows)], dtype=torch.int32, device="cuda")


def dense_twin(tab, grad, st, hy, zero_grad):
    """rs_adam_step on aligned clones of the table with the gradient `grad`: (p, g, m, v, bf16) after the step."""
    from rbm_amd import ops
    p, _, m, v, pb = tab
    c = [x.clone().view(-1) for x in (p, grad, m, v)]
    cb = torch.empty(p.numel(), dtype=torch.bfloat16, device="cuda") if pb is not None else None
    ops.adam_step(c[0], c[1], c[2], c[3], cb, st, hy, zero_grad=zero_grad)
    return [x.view(p.shape) for x in c] + [cb.view(p.shape) if cb is not None else None]


def run_case(R_, d, rows, seed, bf16=True, offset=0, zero_grad=True, max_wg=None):
    """rs_adam_rows over `rows` against the dense twin: listed rows equal the dense result bit for bit (p, m, v,
    bf16, g cleared or kept); every other row -- the NaNs of its gradient included -- keeps its bits."""
    from rbm_amd import ops
    tab = make(R_, d, seed, bf16, offset)
    p, g, m, v, pb = tab
    assert (p.data_ptr() % 16 != 0) == (offset % 4 != 0)
    rows = np.asarray(rows, dtype=np.int64)
    grad = torch.randn(R_, d, generator=torch.Generator().manual_seed(seed + 1)).cuda()
    if len(rows) > 2:
        grad[rows[1]] = 0.0                    # a touched row whose gradient is exactly zero is still updated
        grad[rows[2], : max(1, d // 2)] = -0.0
    idx = torch.from_numpy(rows).cuda()
    g[idx] = grad[idx]                         # NaN stays in the gradient of every unlisted row
    before = [x.clone() if x is not None else None for x in tab]
    st, hy = prepared()
    dp, dg, dm, dv, dpb = dense_twin(tab, grad, st, hy, zero_grad)
    lst, cnt = listed(rows, len(rows) + 5, R_)
    ops.adam_rows(lst, cnt, p.view(R_, d) if d > 1 else p.view(R_), g.view(R_, d) if d > 1 else g.view(R_),
                  m.view(R_, d) if d > 1 else m.view(R_), v.view(R_, d) if d > 1 else v.view(R_),
                  (pb.view(R_, d) if d > 1 else pb.view(R_)) if pb is not None else None, st, hy,
                  zero_grad=zero_grad, max_wg=max_wg)
    torch.cuda.synchronize()
    rest = torch.ones(R_, dtype=torch.bool, device="cuda")
    rest[idx] = False
    for name, got, dense, old in (("p", p, dp, before[0]), ("g", g, dg, before[1]), ("m", m, dm, before[2]),
                                  ("v", v, dv, before[3]), ("bf16", pb, dpb, before[4])):
        if got is None:
            continue
        assert same(got[idx], dense[idx]), (name, "listed rows differ from the dense sweep", R_, d)
        assert same(got[rest], old[rest]), (name, "an unlisted row changed", R_, d)
    if len(rows):
        assert int(torch.count_nonzero(g[idx])) == 0 if zero_grad else same(g[idx], grad[idx])


# ------------------------------------------------------------------ 1. the whole table listed
@pytest.mark.parametrize("R_", [1, 17, 1000])
@pytest.mark.parametrize("d", [1, 4, 50, 64, 128, 256, 264, 1024])
def test_whole_table_listed_is_the_dense_sweep_bitwise(d, R_):
    import rbm_amd  # noqa: F401
    rows = np.random.default_rng(d * 1009 + R_).permutation(R_)
    run_case(R_, d, rows, seed=d + R_)


@pytest.mark.parametrize("variant", ["unaligned_d50", "unaligned_d64", "max_wg_1", "keep_grad", "fp32_d50", "fp32_d64",
                                     "keep_grad_fp32_d1"])
def test_whole_table_listed_variants(variant):
    import rbm_amd  # noqa: F401
    kw = {"unaligned_d50": dict(d=50, offset=1), "unaligned_d64": dict(d=64, offset=1),
          "max_wg_1": dict(d=64, max_wg=1), "keep_grad": dict(d=128, zero_grad=False),
          "fp32_d50": dict(d=50, bf16=False), "fp32_d64": dict(d=64, bf16=False),
          "keep_grad_fp32_d1": dict(d=1, bf16=False, zero_grad=False)}[variant]
    d = kw.pop("d")
    for R_ in (17, 1000):
        run_case(R_, d, np.random.default_rng(R_).permutation(R_), seed=R_, **kw)


# ------------------------------------------------------------------ 2. partial lists
@pytest.mark.parametrize("d", [1, 50, 64, 264])
@pytest.mark.parametrize("frac", ["0", "1", "third", "all"])
def test_partial_list_updates_the_listed_rows_and_nothing_else(d, frac):
    import rbm_amd  # noqa: F401
    R_ = 1000
    n = {"0": 0, "1": 1, "third": R_ // 3, "all": R_}[frac]
    rows = np.sort(np.random.default_rng(d + n).permutation(R_)[:n])
    run_case(R_, d, rows, seed=7 * d + n)
    run_case(R_, d, rows, seed=7 * d + n + 1, max_wg=1, bf16=False)


# ------------------------------------------------------------------ 3. 300 steps against float64
def test_300_steps_of_fresh_touched_sets_against_the_fp64_reference():
    """300 steps (past the 256 a one-byte epoch stamp repeats after), a fresh random touched set per step through
    rs_unique_rows, a learning rate that changes every step: v within 4 ulps, m and p within 4 ulps of the tensor's
    largest magnitude (tests/test_adam_gpu.py's bars for the dense sweep) of the float64 reference.  R = 1000 rows,
    10 fresh ids per step: a row takes about 3 updates, at most 10 -- about the 5 steps those bars were set at (each
    update may add up to ~1 ulp to v; the float32 emulation of this very scenario is held to the same bars on the CPU,
    tests/test_adam_rows_ref.py).  Every step: the rows outside the set keep their bits, NaN gradients included."""
    import rbm_amd  # noqa: F401
    from rbm_amd import ops
    (p0, m0, v0), data = R.scenario(**R.LONG)
    R_, d = p0.shape
    ref = R.Table(p0, np.zeros_like(p0), m0, v0, np.float64)
    p, m, v = (torch.from_numpy(x).cuda() for x in (p0, m0, v0))
    g = torch.full((R_, d), float("nan"), device="cuda")
    pb = p.bfloat16()
    st = torch.zeros(144, dtype=torch.float64, device="cuda")
    hy = torch.tensor(HYPER, dtype=torch.float64, device="cuda")
    cap = sum(x.size for x in data[0][0])
    lst = torch.full((cap,), -3, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.unique_rows_ws_bytes(R_), dtype=torch.uint8, device="cuda")
    ever = np.zeros(R_, dtype=bool)
    for t, (lists, grad, lr) in enumerate(data, 1):
        ids = np.concatenate(lists)
        rows = np.unique(ids[(ids >= 1) & (ids < R_)])
        ref.g[rows] = grad[rows]
        R.sparse_step(ref, lists, t, (lr,) + HYPER[1:])
        idx = torch.from_numpy(rows).cuda()
        g[idx] = torch.from_numpy(grad[rows]).cuda()
        before = [x.clone() for x in (p, g, m, v, pb)]
        hy[0] = lr
        ops.adam_prepare(st, hy)
        ops.unique_rows([torch.from_numpy(x).cuda() for x in lists], R_, lst, cnt, ws)
        ops.adam_rows(lst, cnt, p, g, m, v, pb, st, hy, zero_grad=True)
        rest = torch.ones(R_, dtype=torch.bool, device="cuda")
        rest[idx] = False
        assert int(cnt.item()) == len(rows) and lst[:len(rows)].cpu().numpy().tolist() == rows.tolist(), t
        for name, old, new in zip("pgmvb", before, (p, g, m, v, pb)):
            assert same(old[rest], new[rest]), (t, name, "a row outside the step's set changed")
        ever[rows] = True
    assert float(st[0].item()) == 300.0

    class Got:
        pass
    got = Got()
    got.p, got.g, got.m, got.v = (x.cpu().numpy() for x in (p, g, m, v))
    got.bf16 = pb.float().cpu().numpy()
    errs = R.state_errors(got, ref)
    print("rs_adam_rows vs fp64 after 300 steps (ulps):", errs)
    assert not R.check_state(got, ref, cleared_rows=np.nonzero(ever)[0]), (R.check_state(got, ref), errs)
    assert np.isnan(got.g[~ever]).all() and (~ever).any()        # never listed: never read, never written


# ------------------------------------------------------------------ 4. rs_unique_rows against numpy.unique
def unique(keys, V, cap=None):
    from rbm_amd import ops
    total = sum(k.numel() for k in keys)
    lst = torch.full((cap or max(total, 1),), -9, dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    ws = torch.full((ops.unique_rows_ws_bytes(V),), 0xFF, dtype=torch.uint8, device="cuda")   # no initialisation needed
    ops.unique_rows(keys, V, lst, cnt, ws)
    torch.cuda.synchronize()
    n = int(cnt.item())
    return lst[:n].cpu().numpy().astype(np.int64), lst


def expect(keys, V):
    ids = np.concatenate([k.cpu().numpy().reshape(-1) for k in keys])
    return np.unique(ids[(ids >= 1) & (ids < V)])


@pytest.mark.parametrize("V", [2, 300, 70_000])
@pytest.mark.parametrize("n", [1, 63, 4097, 30_000])
@pytest.mark.parametrize("nsrc", [1, 2, 3])
def test_unique_rows_matches_numpy_unique(nsrc, n, V):
    import rbm_amd  # noqa: F401
    rng = np.random.default_rng(nsrc * 7 + n + V)
    # ids from 0 to a little past the table: padding, the last row and ids >= table_rows among them
    keys = [torch.from_numpy(rng.integers(0, V + 3, size=max(1, n // (k + 1)))).cuda() for k in range(nsrc)]
    keys[-1][-1] = V - 1
    got, _ = unique(keys, V)
    assert got.tolist() == expect(keys, V).tolist()
    again, _ = unique(keys, V, cap=sum(k.numel() for k in keys) + 11)
    assert again.tolist() == got.tolist()


@pytest.mark.parametrize("case", ["zeros", "duplicates", "each_once", "last_row", "outside", "negative", "empty_source"])
def test_unique_rows_edge_cases(case):
    import rbm_amd  # noqa: F401
    V = 5000
    rng = np.random.default_rng(3)
    keys = {"zeros": [np.zeros(777, np.int64)],
            "duplicates": [np.full(4097, 17, np.int64), rng.integers(15, 19, size=30_000)],
            "each_once": [rng.permutation(V)],
            "last_row": [np.full(65, V - 1, np.int64)],
            "outside": [np.arange(V, V + 300), np.array([V - 1, 2 ** 40, 2 ** 31, 2 ** 32 + 5])],
            "negative": [np.array([-1, -5000, 4, -(2 ** 40), 4])],
            "empty_source": [np.zeros(0, np.int64), np.array([9, 3, 9]), np.zeros(0, np.int64)]}[case]
    keys = [torch.from_numpy(np.asarray(k, dtype=np.int64)).cuda() for k in keys]
    got, _ = unique(keys, V)
    want = expect(keys, V)
    assert got.tolist() == want.tolist()
    assert {"zeros": 0, "duplicates": 4, "each_once": V - 1, "last_row": 1, "outside": 1, "negative": 1,
            "empty_source": 2}[case] == len(got)


def test_unique_rows_eager_and_captured_agree():
    """No host synchronisation: the build captures into a graph, and every replay lists the keys then in its static
    inputs -- what the eager call gives for them."""
    import rbm_amd  # noqa: F401
    from rbm_amd import ops
    V, n = 70_000, 4097
    rng = np.random.default_rng(8)
    static = [torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(63, dtype=torch.int64, device="cuda")]
    lst = torch.zeros(n + 63, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.unique_rows_ws_bytes(V), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.unique_rows(static, V, lst, cnt, ws)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ops.unique_rows(static, V, lst, cnt, ws)
    for k in range(3):
        fresh = [torch.from_numpy(rng.integers(0, V + 2 if k else 50, size=s.numel())).cuda() for s in static]
        for s, f in zip(static, fresh):
            s.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
        captured = lst[:int(cnt.item())].cpu().numpy().tolist()
        eager, _ = unique(fresh, V)
        assert captured == eager.tolist() == expect(fresh, V).tolist()
