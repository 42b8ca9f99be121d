"""CPU checks of tests/gradnorm_ref.py: the emulation of the gradient-norm kernels' partial order holds the derived
bounds against the extended-precision reference, every planted mistake is rejected by at least one case, and the C
entry points' host-side validation and slot counts agree with the restatement (no launch: no GPU here)."""
import ctypes

import numpy as np
import pytest

import gradnorm_ref as G

DENSE_N = [1, 3, 4, 5, 255, 256, 257, 4099, 2 ** 20 + 3]
INF = float("inf")


def _g(n, seed=0, scale=1.0):
    return (scale * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def test_slot_counts():
    ns = (1, 3, 4, 4096, 4097, 4100, 2 ** 20 + 3, 2 ** 28)
    assert [G.dense_parts(n) for n in ns] == [1, 1, 1, 1, 1, 2, 256, 2048]
    assert [G.rows_parts(d, c) for d, c in ((1, 1), (64, 1000), (256, 1000), (64, 2 ** 24))] == [1, 16, 63, 1024]


@pytest.mark.parametrize("n", DENSE_N)
def test_dense_emulation_holds_the_bounds(n):
    g = _g(n, n)
    ss = G.sumsq(g)
    parts = G.emulate_dense(g, [(0, n)])
    assert parts.size == G.dense_parts(n)
    for mx, div in ((INF, None), (0.5 * float(np.sqrt(float(ss))), None), (0.1, 3.0)):
        rec = G.emulate_finish(parts, mx, div)
        assert G.check_record(rec, G.reference(ss, mx, div), n) == [], (n, mx, div)


def test_two_and_three_ranges_in_one_call():
    g = _g(9000, 3)
    for ranges in ([(0, 4099), (4100, 9000)], [(0, 255), (256, 4103), (4104, 8999)]):
        parts = G.emulate_dense(g, ranges)
        assert parts.size == sum(G.dense_parts(hi - lo) for lo, hi in ranges)
        ss = G.sumsq(*[g[lo:hi] for lo, hi in ranges])
        n = sum(hi - lo for lo, hi in ranges)
        assert G.check_record(G.emulate_finish(parts, 1.0), G.reference(ss, 1.0), n) == []


@pytest.mark.parametrize("d", [1, 32, 64, 256])
def test_row_list_emulation_holds_the_bounds_and_ignores_unlisted_rows(d):
    R, cap = 1000, 40
    rng = np.random.default_rng(d)
    ws = None
    for count in (1, 7, cap, 3):                     # the last: a shorter list on the same workspace
        table = np.full((R, d), 1e30, np.float32)    # poison: an unlisted row that contributed would be seen
        rows = np.sort(rng.choice(np.arange(1, R), cap, replace=False)).astype(np.int32)
        table[rows[:count]] = rng.standard_normal((count, d)).astype(np.float32)
        ws = G.emulate_rows(table, rows, count, cap, ws)
        assert ws.size == G.rows_parts(d, cap)
        ss = G.sumsq(table[rows[:count]])
        assert G.check_record(G.emulate_finish(ws, 1.0), G.reference(ss, 1.0), count * d) == [], (d, count)
    if d % 4 == 0:      # the scalar path (a misaligned base) gives a sum inside the same bound
        alt = G.emulate_rows(table, rows, 3, cap, vec=False)
        assert G.check_record(G.emulate_finish(alt, 1.0), G.reference(ss, 1.0), 3 * d) == []


def test_finish_cases():
    g = np.array([3.0, 4.0], np.float32)             # norm 5 exactly
    parts = G.emulate_dense(g, [(0, 2)])
    for mx in (2.0, 2.5, 3.0, INF):                  # div = 2: the norm is 2.5
        rec = G.emulate_finish(parts, mx, 2.0)
        ref = G.reference(G.sumsq(g), mx, 2.0)
        assert G.check_record(rec, ref, 2) == [], mx
        if mx in (3.0, INF):                         # not clipping: exactly 1, the divisor untouched
            assert rec[1] == 1.0 and rec[2] == 2.0 and ref[1:] == (1.0, 2.0)
        else:
            assert rec[1] < 1.0 and rec[2] > 2.0
    assert G.emulate_finish(parts, 5.0)[1] < 1.0     # norm == max_norm clips by the eps
    # a finite value whose square overflows float32 but not float64: the correct finite norm
    big = np.full(5, 1e30, np.float32)
    rec = G.emulate_finish(G.emulate_dense(big, [(0, 5)]), 1.0)
    ref = G.reference(G.sumsq(big), 1.0)
    assert np.isfinite(rec).all() and G.check_record(rec, ref, 5) == []
    assert abs(float(rec[0]) / (float(np.float32(1e30)) * 5 ** 0.5) - 1) < 1e-6
    # a non-finite norm: coefficient 0 (the gradient is scaled to nothing), or NaN, applied
    rec = G.emulate_finish(np.array([np.inf]), 1.0)
    assert rec[0] == np.inf and rec[1] == 0.0 and rec[2] == np.inf
    assert G.check_record(rec, G.reference(np.inf, 1.0), 1) == []
    rec = G.emulate_finish(np.array([np.nan]), 1.0)
    assert np.isnan(rec).all() and G.check_record(rec, G.reference(np.nan, 1.0), 1) == []


# ------------------------------------------------------------------ a sparse BERT-like step and the planted mistakes
def _sparse_step(seed=1, counts=(20, 9)):
    """flat gradient = dense [0, 4099 + pad) | token table [300][32] | dense | out.weight [300][32] | out.bias [300],
    lists of capacity 24 / 12; unlisted rows zero, as the sparse tables' contract has it"""
    rng = np.random.default_rng(seed)
    R, d = 300, 32
    lay, off = {}, 0
    for name, n in (("a", 4099), ("tok", R * d), ("b", 517), ("ow", R * d), ("ob", R)):
        lay[name] = off
        off += -(-n // 64) * 64
    g = np.zeros(off, np.float32)
    g[lay["a"]:lay["a"] + 4099] = rng.standard_normal(4099)
    g[lay["b"]:lay["b"] + 517] = rng.standard_normal(517)
    lists = []
    for cap, cnt in zip((24, 12), counts):
        lst = np.zeros(cap, np.int32)
        lst[:cnt] = np.sort(rng.choice(np.arange(1, R), cnt, replace=False))
        lst[cnt:] = rng.integers(1, R, cap - cnt)       # past the count: unspecified ids
        lists.append((lst, cnt))
    for name, (lst, cnt), w in (("tok", lists[0], d), ("ow", lists[1], d), ("ob", lists[1], 1)):
        for r in lst[:cnt]:
            g[lay[name] + r * w:lay[name] + (r + 1) * w] = rng.standard_normal(w)
    segs = [(lay["a"], lay["tok"]), (lay["b"], lay["ow"])]
    tables = [(lay["tok"], R, d, lists[0][0], lists[0][1]), (lay["ow"], R, d, lists[1][0], lists[1][1]),
              (lay["ob"], R, 1, lists[1][0], lists[1][1])]
    return g, segs, tables


def _cases():
    """(name, g, segs, tables, max_norm, div, workspace left by an earlier launch)"""
    out = []
    g, segs, tables = _sparse_step()
    nrm = float(np.sqrt(float(G.sumsq(g))))
    out.append(("sparse_clip", g, segs, tables, 0.5 * nrm, None, None))
    out.append(("sparse_noclip", g, segs, tables, 2.0 * nrm, 4.0, None))
    out.append(("sparse_div", g, segs, tables, 0.1 * nrm, 4.0, None))
    # unlisted rows past the count carry a stale gradient the list must keep out
    g2 = g.copy()
    lo, R, d, lst, cnt = tables[0]
    for r in lst[cnt:]:
        g2[lo + r * d:lo + (r + 1) * d] = 7.0
    out.append(("past_count", g2, segs, tables, 0.5 * nrm, None, None))
    # a dense range with a tail; a tiny gradient, where the eps decides the coefficient
    t = _g(4099, 5)
    out.append(("tail", t, [(0, 4099)], [], 1.0, None, None))
    out.append(("tiny", _g(7, 6, 1e-7), [(0, 7)], [], 1e-7, None, None))
    return out, None


def _check(case, mistake=None, ws=None):
    name, g, segs, tables, mx, div, _ = case
    rec, ws = G.emulate_step(g, segs, tables, mx, div, mistake, ws)
    listed = [g[lo:hi] for lo, hi in segs]
    for lo, R, d, lst, cnt in tables:
        listed += [g[lo + r * d:lo + (r + 1) * d] for r in lst[:cnt]]
    n = sum(x.size for x in listed)
    return G.check_record(rec, G.reference(G.sumsq(*listed), mx, div), n), ws


def _stale_case(mistake=None):
    """rows of 128 over a capacity of 200: 7 virtual workgroups; a 150-row launch, then a 3-row one on its workspace"""
    rng = np.random.default_rng(8)
    R, d, cap = 400, 128, 200
    table = rng.standard_normal((R, d)).astype(np.float32)
    rows = np.sort(rng.choice(np.arange(1, R), cap, replace=False)).astype(np.int32)
    ws = G.emulate_rows(table, rows, 150, cap, None, mistake)
    assert G.rows_parts(d, cap) == 7 and np.count_nonzero(ws) == 7
    ws = G.emulate_rows(table, rows, 3, cap, ws, mistake)
    return G.check_record(G.emulate_finish(ws, 1.0), G.reference(G.sumsq(table[rows[:3]]), 1.0), 3 * d)


def test_the_emulated_step_holds_the_bounds():
    cases, _ = _cases()
    for c in cases:
        assert _check(c)[0] == [], c[0]
    assert _stale_case() == []


@pytest.mark.parametrize("mistake", G.MISTAKES)
def test_every_planted_mistake_is_rejected(mistake):
    cases, _ = _cases()
    caught = [c[0] for c in cases if _check(c, mistake)[0]]
    if mistake == "stale_partials":
        caught += ["stale"] if _stale_case(mistake) else []
    print(mistake, "rejected by", caught)
    assert caught, mistake


def test_the_reference_is_torchs_clip_grad_norm():
    import torch
    rng = np.random.default_rng(2)
    ps = [torch.nn.Parameter(torch.zeros(s, dtype=torch.float64)) for s in ((40, 8), (17,), (3, 5, 2))]
    for mx in (0.5, 100.0):
        for p in ps:
            p.grad = torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(np.float32)).double()
        flat = np.concatenate([p.grad.numpy().reshape(-1) for p in ps])
        ref = G.reference(G.sumsq(flat), mx)
        total = float(torch.nn.utils.clip_grad_norm_(ps, mx))
        assert abs(total - ref[0]) <= 1e-14 * ref[0]
        after = np.concatenate([p.grad.numpy().reshape(-1) for p in ps])
        assert np.allclose(after, flat * ref[1], rtol=1e-14, atol=0) and np.allclose(after, flat / ref[2], rtol=1e-14,
                                                                                       atol=0)


# ------------------------------------------------------------------ the C entry points, without a launch
ARG = 1001
FAKE = 0x10000        # 16-byte aligned, points at nothing: every call below must be refused before any launch


def test_entry_points_reject_bad_arguments_before_any_launch():
    import rbm_amd._lib as L
    lib = L.lib()
    for n in (1, 3, 4, 4097, 2 ** 20 + 3, 2 ** 28):
        assert lib.rs_gradnorm_dense_parts(n) == G.dense_parts(n)
    for d, cap in ((1, 1), (64, 1000), (256, 1000), (50, 33), (64, 2 ** 24)):
        assert lib.rs_gradnorm_rows_parts(d, cap) == G.rows_parts(d, cap)
    assert lib.rs_gradnorm_dense_parts(0) == -1 and lib.rs_gradnorm_dense_parts(-4) == -1
    assert lib.rs_gradnorm_rows_parts(0, 8) == -1 and lib.rs_gradnorm_rows_parts(8, 0) == -1
    assert lib.rs_gradnorm_rows_parts(64, 2 ** 25) == -1

    def dense(g=FAKE, ranges=((0, 8),), nr=None, max_wg=64, partials=FAKE):
        arr = (ctypes.c_int64 * max(2 * len(ranges), 2))(*[x for r in ranges for x in r])
        return lib.rs_gradnorm_dense(g, arr, len(ranges) if nr is None else nr, max_wg, partials, None)
    assert dense(g=None) == ARG and dense(g=FAKE + 4) == ARG                       # null, misaligned
    assert dense(ranges=((0, 0),)) == ARG and dense(ranges=((8, 4),)) == ARG       # n <= 0
    assert dense(ranges=((2, 8),)) == ARG and dense(ranges=((-4, 8),)) == ARG      # a start off the 16-byte grid
    assert dense(max_wg=0) == ARG and dense(partials=None) == ARG and dense(partials=FAKE + 4) == ARG
    assert dense(nr=0) == ARG and dense(ranges=((0, 8),) * 9) == ARG
    assert lib.rs_gradnorm_dense(FAKE, None, 1, 64, FAKE, None) == ARG

    def rows(g=FAKE, d=64, R=100, lst=FAKE, cnt=FAKE, cap=10, max_wg=64, partials=FAKE):
        return lib.rs_gradnorm_rows(g, d, R, lst, cnt, cap, max_wg, partials, None)
    assert rows(g=None) == ARG and rows(g=FAKE + 2) == ARG
    assert rows(d=0) == ARG and rows(cap=0) == ARG and rows(R=0) == ARG and rows(max_wg=0) == ARG
    assert rows(d=64, cap=2 ** 25) == ARG and rows(d=2 ** 31, cap=1) == ARG        # cap * d >= 2^31
    assert rows(lst=None) == ARG and rows(cnt=None) == ARG and rows(partials=None) == ARG

    def finish(partials=FAKE, n=4, div=None, mx=FAKE, rec=FAKE):
        return lib.rs_gradnorm_finish(partials, n, div, mx, rec, None)
    assert finish(partials=None) == ARG and finish(n=0) == ARG and finish(mx=None) == ARG and finish(rec=None) == ARG
    assert finish(mx=FAKE + 4) == ARG and finish(div=FAKE + 2) == ARG and finish(rec=FAKE + 2) == ARG
