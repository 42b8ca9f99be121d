"""rs_gradnorm_dense / rs_gradnorm_rows / rs_gradnorm_finish on the GPU, through the C ABI's wrappers, against the
extended-precision reference of tests/gradnorm_ref.py with the bounds derived there (norm: 2^-24 + (n + 4) 2^-53
relative; coefficient and effective divisor two and three double roundings more).  The kernels' arithmetic is fixed
by the lengths alone, so the record must also equal the numpy restatement of their partial order bit for bit, for
every max_wg and on every launch."""
import numpy as np
import pytest
import torch

import gradnorm_ref as G

pytestmark = pytest.mark.gpu

INF = float("inf")
DENSE_N = [1, 3, 4, 5, 255, 256, 257, 4099, 2 ** 20 + 3]


def _bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _finish(ws, k, mx, div=None):
    from rbm_amd import ops
    rec = torch.full((4,), -7.0, device="cuda")
    mxt = torch.tensor([mx], dtype=torch.float64, device="cuda")
    dvt = None if div is None else torch.tensor([div], dtype=torch.float32, device="cuda")
    ops.gradnorm_finish(ws, k, mxt, rec, div=dvt)
    torch.cuda.synchronize()
    assert float(rec[3]) == -7.0                       # three floats and no more
    return rec[:3].cpu().numpy()


def _dense(g, ranges, max_wg=8192):
    from rbm_amd import ops
    need = sum(ops.gradnorm_dense_parts(hi - lo) for lo, hi in ranges)
    ws = torch.full((need + 2,), -3.0, dtype=torch.float64, device="cuda")      # a guard slot behind the partials
    k = ops.gradnorm_dense(g, ranges, ws, max_wg=max_wg)
    torch.cuda.synchronize()
    assert k == need and float(ws[need]) == -3.0
    return ws, k


@pytest.mark.parametrize("n", DENSE_N)
def test_dense_ranges(n):
    rng = np.random.default_rng(n)
    host = rng.standard_normal(n + 8).astype(np.float32)
    host[n:] = 1e30                                     # past the range: must not be read into the sum
    g = torch.from_numpy(host).cuda()
    ss = G.sumsq(host[:n])
    out = {}
    for max_wg in (1, 8192):
        ws, k = _dense(g, [(0, n)], max_wg)
        assert k == G.dense_parts(n)
        out[max_wg] = (ws[:k].cpu().numpy(), _finish(ws, k, 0.5 * float(np.sqrt(float(ss)))))
    assert np.array_equal(_bits(out[1][0]), _bits(out[8192][0])) and np.array_equal(_bits(out[1][1]),
                                                                                     _bits(out[8192][1]))
    mx = 0.5 * float(np.sqrt(float(ss)))
    rec = out[8192][1]
    print("dense", n, "record", rec, "reference", G.reference(ss, mx))
    assert G.check_record(rec, G.reference(ss, mx), n) == []
    emu = G.emulate_dense(host, [(0, n)])
    assert np.array_equal(_bits(out[8192][0]), _bits(emu))
    assert np.array_equal(_bits(rec), _bits(G.emulate_finish(emu, mx)))
    ws, k = _dense(g, [(0, n)])                         # the same launch again: the same bits
    assert np.array_equal(_bits(ws[:k]), _bits(out[8192][0]))
    assert np.array_equal(_bits(_finish(ws, k, mx)), _bits(rec))


@pytest.mark.parametrize("ranges", [[(0, 4099), (4100, 9000)], [(0, 255), (256, 4103), (4104, 8999)],
                                    [(64, 2 ** 20 + 67), (2 ** 20 + 128, 2 ** 20 + 131)]])
def test_several_ranges_in_one_call(ranges):
    end = ranges[-1][1]
    host = np.random.default_rng(end).standard_normal(end + 4).astype(np.float32)
    keep = np.zeros(end + 4, bool)
    for lo, hi in ranges:
        keep[lo:hi] = True
    host[~keep] = 1e30                                  # the gaps between the ranges
    g = torch.from_numpy(host).cuda()
    n = int(keep.sum())
    ss = G.sumsq(host[keep])
    recs = []
    for max_wg in (1, 8192):
        ws, k = _dense(g, ranges, max_wg)
        recs.append(_finish(ws, k, 1.0, 3.0))
        assert np.array_equal(_bits(ws[:k]), _bits(G.emulate_dense(host, ranges)))
    print("ranges", ranges, "record", recs[1], "reference", G.reference(ss, 1.0, 3.0))
    assert np.array_equal(_bits(recs[0]), _bits(recs[1]))
    assert G.check_record(recs[1], G.reference(ss, 1.0, 3.0), n) == []


@pytest.mark.parametrize("d,shift", [(1, 0), (32, 0), (64, 0), (256, 0), (32, 1)])
def test_row_lists(d, shift):
    """R = 1000, a list of capacity 200; count 1, 7, cap, then 3 on the same workspace.  Unlisted rows hold 1e30.
    shift = 1: the table starts 4 bytes off the 16-byte grid (the element-by-element path at d % 4 == 0)."""
    from rbm_amd import ops
    R, cap = 1000, 200
    rng = np.random.default_rng(10 * d + shift)
    k = ops.gradnorm_rows_parts(d, cap)
    assert k == G.rows_parts(d, cap)
    ws = torch.full((k + 1,), -3.0, dtype=torch.float64, device="cuda")
    buf = torch.zeros(R * d + 4, device="cuda")
    for count in (1, 7, cap, 3):
        table = np.full((R, d), 1e30, np.float32)
        rows = np.sort(rng.choice(np.arange(1, R), cap, replace=False)).astype(np.int32)
        table[rows[:count]] = rng.standard_normal((count, d)).astype(np.float32)
        if count == 7:
            rows[2] = R + 5                             # an id outside the table is skipped
        listed = [r for r in rows[:count] if r < R]
        buf[shift:shift + R * d].copy_(torch.from_numpy(table.reshape(-1)))
        tv = buf[shift:shift + R * d]
        tv = tv.view(R, d) if d > 1 else tv
        lst, cnt = torch.from_numpy(rows).cuda(), torch.tensor([count], dtype=torch.int32, device="cuda")
        for max_wg in (1, 8192):
            assert ops.gradnorm_rows(tv, lst, cnt, ws, max_wg=max_wg) == k
            rec = _finish(ws, k, 1.0)
            assert float(ws[k]) == -3.0
            ss = G.sumsq(table[listed])
            ref = G.reference(ss, 1.0)
            print("rows", d, shift, count, max_wg, "record", rec, "reference", ref)
            assert G.check_record(rec, ref, len(listed) * d) == [], (count, max_wg)
            emu = G.emulate_rows(table, rows, count, cap, vec=(d % 4 == 0 and shift == 0))
            assert np.array_equal(_bits(ws[:k]), _bits(emu)), (count, max_wg)
    # a negative or oversized count is clamped to [0, cap]
    cnt.fill_(-4)
    ops.gradnorm_rows(tv, lst, cnt, ws)
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(ws[:k])) == 0


def test_finish():
    g = torch.tensor([3.0, 4.0, 0.0, 0.0], device="cuda")            # norm 5 (2.5 under div = 2)
    ws, k = _dense(g, [(0, 2)])
    ss = G.sumsq([3.0, 4.0])
    for mx in (2.0, 2.5, 3.0, INF):
        rec = _finish(ws, k, mx, 2.0)
        ref = G.reference(ss, mx, 2.0)
        print("finish", mx, rec, ref)
        assert G.check_record(rec, ref, 2) == [], mx
        if mx in (3.0, INF):
            assert rec[1] == 1.0 and rec[2] == 2.0                   # exactly 1, the divisor untouched
        else:
            assert rec[1] < 1.0 and rec[2] > 2.0
        assert np.array_equal(_bits(rec), _bits(G.emulate_finish(ws[:k].cpu().numpy(), mx, 2.0)))
    assert _finish(ws, k, 5.0)[1] < 1.0                              # norm == max_norm: the eps clips
    rec = _finish(ws, k, INF)
    assert rec[0] == 5.0 and rec[1] == 1.0 and rec[2] == 1.0         # no div: 1
    # a finite value whose square overflows float32 but not float64
    big = torch.full((8,), 1e30, device="cuda")
    ws, k = _dense(big, [(0, 5)])
    rec = _finish(ws, k, 1.0)
    ref = G.reference(G.sumsq(np.full(5, 1e30, np.float32)), 1.0)
    print("large", rec, ref)
    assert np.isfinite(rec).all() and G.check_record(rec, ref, 5) == []
    # a non-finite gradient: the norm is reported, the coefficient 0 (or NaN) is what the optimizer gets
    bad = torch.tensor([1.0, INF, 2.0, 0.0], device="cuda")
    ws, k = _dense(bad, [(0, 4)])
    rec = _finish(ws, k, 1.0)
    assert rec[0] == np.inf and rec[1] == 0.0 and rec[2] == np.inf
    bad[1] = float("nan")
    ws, k = _dense(bad, [(0, 4)])
    assert np.isnan(_finish(ws, k, 1.0)).all()
    # many partials: more than one slot per thread of the finish
    n = 4096 * 700 + 5
    host = np.random.default_rng(1).standard_normal(n).astype(np.float32)
    ws, k = _dense(torch.from_numpy(host).cuda(), [(0, n)])
    assert k == 701
    rec = _finish(ws, k, 7.0, 0.5)
    assert G.check_record(rec, G.reference(G.sumsq(host), 7.0, 0.5), n) == []
    assert np.array_equal(_bits(rec), _bits(G.emulate_finish(ws[:k].cpu().numpy(), 7.0, 0.5)))


def test_wrappers_refuse_bad_arguments():
    from rbm_amd import ops
    g = torch.zeros(64, device="cuda")
    ws = torch.zeros(8, dtype=torch.float64, device="cuda")
    lst, cnt = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    for bad in ([(0, 0)], [(2, 8)], [(0, 65)], [], [(0, 8)] * 9):
        with pytest.raises(ValueError):
            ops.gradnorm_dense(g, bad, ws)
    with pytest.raises(ValueError):
        ops.gradnorm_dense(g, [(0, 64)], ws, max_wg=0)
    with pytest.raises(ValueError):
        ops.gradnorm_dense(g, [(0, 64)], ws[:0])
    with pytest.raises(ValueError):
        ops.gradnorm_dense(g.double(), [(0, 64)], ws)
    with pytest.raises(ValueError):
        ops.gradnorm_rows(g.view(8, 8), lst.long(), cnt, ws)
    with pytest.raises(ValueError):
        ops.gradnorm_rows(g.view(8, 8), lst, cnt, ws, max_wg=0)
    with pytest.raises(ValueError):
        ops.gradnorm_rows(g.view(8, 8), lst, cnt, ws.float())
    with pytest.raises(ValueError):
        ops.gradnorm_finish(ws, 0, ws[:1], g)
    with pytest.raises(ValueError):
        ops.gradnorm_finish(ws, 4, g[:1], g)                          # max_norm must be a double
    with pytest.raises(ValueError):
        ops.gradnorm_finish(ws, 4, ws[:1], g[:2])
