"""Kernel-level checks of the fused SAS row-chain kernels (rowchain.hip): every entry point called directly, every
stored tensor held elementwise to the float64 reference and derived bound of tests/rowchain_ref.py, at row counts
that reach both tile-dealing regimes, ragged last tiles and the per-wave tile loop's second and third iteration.

Every output is pre-filled with NaN and followed by 32 guard rows: after the launch no NaN may remain below M
(every tile has an owner) and every guard row must still be NaN (no store past M).  Each test prints its worst
err / bound per output tensor; any ratio above 1 fails."""
import functools
import math

import pytest
import torch

import rowchain_ref as R

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
SALT_E, SALT_1, SALT_2, SEED = 0x1234_5678_9ABC_DEF1, 0x0F0F_1111_2222_3333, 0x7A7A_4444_5555_6666, 977
WORST = {}

# case label -> (case of the table, index): M from the part's CU count (rowchain_ref.case_rows)
CASES = {"1a": (1, 0), "1b": (1, 1), "1c": (1, 2), "2": (2, 0), "3": (3, 0), "4": (4, 0), "5": (5, 0)}
# (rs_sas_block_in and rs_sas_block_in_bwd have no dropout site: they run once per shape)
PARAMS = [(c, d, p) for d in (64, 128) for c in CASES for p in (0.0, 0.2) if not (c == "5" and p == 0.0)]


def _ops():
    from rbm_amd import ops
    return ops


def ncu():
    return _ops().sas_block_grid(10 ** 9)


def rows_of(case):
    c, i = CASES[case]
    return R.case_rows(ncu())[c][i]


def _mask(M, d, p, salt, sb):
    """keep mask of a dropout site with element index m*d + n (the kernels' own hash, through the C ABI)"""
    if p == 0:
        return torch.ones(M, d, dtype=torch.bool, device="cuda")
    ones = torch.ones(M, d, dtype=F32, device="cuda")
    out = torch.empty_like(ones)
    _ops().dropout_rowmask(ones, p, salt, sb, None, out)
    return out > 0


@functools.lru_cache(maxsize=3)
def problem(case, d, p):
    M = rows_of(case)
    inp = R.make_inputs(M, d, p, ncu(), dev="cuda", seed=7)
    inp["sb"] = torch.full((1,), SEED, dtype=torch.int64, device="cuda")
    for n, salt in (("me", SALT_E), ("m1", SALT_1), ("m2", SALT_2)):
        inp[n] = _mask(M, d, p, salt, inp["sb"])
    assert _ops().sas_block_grid(M) == min(-(-M // 16), ncu()) == _ops().sas_block_parts(M)
    return inp


class Bufs:
    """NaN-filled outputs with guard rows; [name] is the full buffer (what the kernel gets), .out the rows below M"""

    def __init__(self, M):
        self.M, self.full, self.rows = M, {}, {}

    def add(self, name, cols=None, dt=BF, rows=None):
        n = self.M if rows is None else rows
        shape = (n + R.GUARD,) if cols is None else (n + R.GUARD, cols)
        self.full[name], self.rows[name] = torch.full(shape, math.nan, dtype=dt, device="cuda"), n
        return self.full[name]

    def __getitem__(self, name):
        return self.full[name]

    @property
    def out(self):
        return {k: v[:self.rows[k]] for k, v in self.full.items()}

    def check_written(self):
        torch.cuda.synchronize()
        for k, v in self.full.items():
            n = self.rows[k]
            assert not torch.isnan(v[:n]).any(), f"{k}: rows below M left unwritten"
            assert torch.isnan(v[n:]).all(), f"{k}: store past M"

    def check_untouched(self):
        torch.cuda.synchronize()
        for k, v in self.full.items():
            assert torch.isnan(v).all(), f"{k}: written by a call that must not launch"


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    """after the module's tests: the worst err / bound per kernel and output tensor over the cases that ran"""
    yield
    print("\nworst err / bound per kernel and output tensor")
    for (kernel, k), v in sorted(WORST.items()):
        print(f"{kernel:18s} {k:14s} {v:.4f}")


def report(kernel, key, res):
    print(f"\n{kernel} {key} err/bound:", {k: round(v, 4) for k, v in res.items()})
    for k, v in res.items():
        WORST[(kernel, k)] = max(WORST.get((kernel, k), 0.0), v)
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, (kernel, key, bad)


# ------------------------------------------------------------------ launches
def in_bufs(M, d):
    b = Bufs(M)
    b.add("Q", d), b.add("mean", dt=F32), b.add("rstd", dt=F32), b.add("q", d), b.add("kv", 2 * d)
    return b


def run_in(inp, b, x):
    _ops().sas_block_in(x, inp["ln1w"], inp["ln1b"], R.EPS, b["Q"], b["mean"], b["rstd"], inp["Wq"], inp["bq"], b["q"],
                        inp["Wkv"], inp["bkv"], b["kv"])


def run_in_embed(inp, b, cnt, ids=None, x0=None):
    M = inp["M"]
    _ops().sas_block_in_embed(inp["ids"] if ids is None else ids, inp["T"], inp["E"], inp["Ptab"], inp["scale"],
                              inp["p"], SALT_E, inp["sb"], b["x0"][:M] if x0 is None else x0, inp["pos"], cnt,
                              inp["ln1w"], inp["ln1b"], R.EPS, b["Q"], b["mean"], b["rstd"], inp["Wq"], inp["bq"],
                              b["q"], inp["Wkv"], inp["bkv"], b["kv"])


def out_bufs(M, d, head, grid):
    b = Bufs(M)
    b.add("x1", d), b.add("z", d), b.add("mean", dt=F32), b.add("rstd", dt=F32), b.add("h1", d), b.add("xn", d)
    if head:
        b.add("f", d), b.add("dx", d)
        for n in ("pl", "nl", "dpl", "dnl"):
            b.add(n, dt=F32)
        b.add("lnpart", 2 * d, dt=F32, rows=grid), b.add("part", 3, dt=F32, rows=grid)
    return b


def out_args(inp, b, o=None):
    return (inp["o"] if o is None else o, inp["Q"], inp["Wo"], inp["bo"], b["x1"], inp["ln2w"], inp["ln2b"], R.EPS,
            b["z"], b["mean"], b["rstd"], inp["W1"], inp["b1"], b["h1"], inp["W2"], inp["b2"], b["xn"], inp["ids"],
            inp["p"], SALT_1, SALT_2, inp["sb"])


def run_out_head(inp, b, grid, cnt, divisor, o=None):
    _ops().sas_block_out_head(out_args(inp, b, o), inp["E"], inp["pos"], inp["neg"], inp["lnlw"], inp["lnlb"], cnt,
                              divisor, b["f"], b["pl"], b["nl"], b["dpl"], b["dnl"], b["dx"], b["lnpart"],
                              b["part"][:grid])


def out_bwd_bufs(M, d, grid, delta):
    b = Bufs(M)
    for n in ("dy2", "da1", "dx1", "dout"):
        b.add(n, d)
    b.add("part", 2 * d, dt=F32, rows=grid)
    if delta:
        b.add("delta", dt=F32)
    return b


def run_out_bwd(inp, b, dxn=None, o=None, delta=None):
    _ops().sas_block_out_bwd(inp["dxn"] if dxn is None else dxn, inp["ids"], inp["h1"], inp["x1"], inp["mean2"],
                             inp["rstd2"], inp["ln2w"], inp["W2T"], inp["W1T"], inp["WoT"], b["dy2"], b["da1"],
                             b["dx1"], b["dout"], b["part"], inp["p"], SALT_1, SALT_2, inp["sb"], o=o, delta=delta)


def run_out_bwd_plain(inp, b):
    """the exported rs_sas_block_out_bwd itself (ops.sas_block_out_bwd always enters the _delta form)"""
    from rbm_amd import _lib
    M, d = inp["dxn"].shape
    t = [inp[n] for n in ("dxn", "ids", "h1", "x1", "mean2", "rstd2", "ln2w", "W2T", "W1T", "WoT")]
    t += [b[n] for n in ("dy2", "da1", "dx1", "dout", "part")]
    _lib.call("rs_sas_block_out_bwd", M, d, *(_lib.ptr(x) for x in t), inp["p"], SALT_1, SALT_2,
              _lib.ptr(inp["sb"]), _lib.stream())


def in_bwd_bufs(M, d, grid):
    b = Bufs(M)
    b.add("dx", d), b.add("part", 2 * d, dt=F32, rows=grid)
    return b


def run_in_bwd(inp, b, dq=None):
    _ops().sas_block_in_bwd(inp["dq"] if dq is None else dq, inp["dkv"], inp["dx1b"], inp["xb"], inp["mean1"],
                            inp["rstd1"], inp["ln1w"], inp["WinT"], b["dx"], b["part"])


def parts3(out, name, grid, d):
    """[grid][2d] partial rows -> [grid][2][d]"""
    return {**out, name: out[name].view(grid, 2, d)}


# ------------------------------------------------------------------ the tests
def test_large_case_runs_the_tile_loop_two_to_three_times():
    """case 5 on THIS part: every wave carries at least 2 tiles and some wave 3 (so the reload paths, the
    multi-tile partial sums and the second tile's prefetch run), from the launch grid the library reports"""
    ops = _ops()
    M = rows_of("5")
    assert ops.sas_block_grid(M) == ncu()
    counts = [len(r) for r in R.wave_tiles(M, ops.sas_block_grid(M)).values()]
    print("\ncase 5: M =", M, "CUs =", ncu(), "tiles per wave min/max =", min(counts), max(counts))
    assert len(counts) == 8 * ncu() and min(counts) >= 2 and max(counts) >= 3
    assert sum(counts) == -(-M // 16)
    # the other cases sit in the regime the table names
    for case, xcd in (("1c", False), ("2", True), ("3", False), ("4", True)):
        g = ops.sas_block_grid(rows_of(case))
        assert (g >= 8 and g % 8 == 0) == xcd, (case, g)
    assert -(-rows_of("4") // 16) % 8 != 0


@pytest.mark.parametrize("case,d,p", [q for q in PARAMS if q[2] == 0.2])
def test_block_in(case, d, p):
    inp = problem(case, d, p)
    b = in_bufs(inp["M"], d)
    run_in(inp, b, inp["x"])
    b.check_written()
    report("block_in", (inp["M"], d), R.check_block_in(inp, b.out))


@pytest.mark.parametrize("case,d", [(c, d) for d in (64, 128) for c in ("1c", "3", "4")])
def test_block_in_strided_input(case, d):
    """x as a strided view (ldx = 2d): same results, bit for bit, as from the contiguous copy"""
    inp = problem(case, d, 0.2)
    M = inp["M"]
    wide = torch.full((M, 2 * d), math.nan, dtype=BF, device="cuda")
    wide[:, :d] = inp["x"]
    b, c = in_bufs(M, d), in_bufs(M, d)
    run_in(inp, b, wide[:, :d])
    run_in(inp, c, inp["x"])
    b.check_written()
    report("block_in(ldx=2d)", (M, d), R.check_block_in(inp, b.out))
    for k in b.full:
        assert torch.equal(b.out[k], c.out[k]), k


@pytest.mark.parametrize("case,d,p", PARAMS)
def test_block_in_embed(case, d, p):
    ops = _ops()
    inp = problem(case, d, p)
    M = inp["M"]
    grid = ops.sas_block_in_count_parts(M)
    b = in_bufs(M, d)
    b.add("x0", d)
    cnt = torch.full((grid + 8,), -7, dtype=torch.int32, device="cuda")
    run_in_embed(inp, b, cnt)
    b.check_written()
    assert int(cnt[:grid].sum()) == int((inp["pos"] != 0).sum()) and bool((cnt[grid:] == -7).all())
    assert bool((cnt[:grid] >= 0).all())
    x0 = torch.empty(M, d, dtype=BF, device="cuda")
    ops.embed_fwd(0, inp["ids"], inp["T"], inp["E"], inp["Ptab"], inp["scale"], p, SALT_E, inp["sb"], x0)
    assert torch.equal(b.out["x0"].view(torch.int16), x0.view(torch.int16))
    res = {**R.check_embed(inp, b.out), **R.check_block_in(inp, b.out, x=b.out["x0"])}
    report("block_in_embed", (M, d, p), res)


@pytest.mark.parametrize("case,d,p", PARAMS)
def test_block_out(case, d, p):
    inp = problem(case, d, p)
    b = out_bufs(inp["M"], d, False, 0)
    _ops().sas_block_out(*out_args(inp, b))
    b.check_written()
    report("block_out", (inp["M"], d, p), R.check_block_out(inp, b.out))


@pytest.mark.parametrize("form", ["divisor", "count_parts"])
@pytest.mark.parametrize("case,d,p", PARAMS)
def test_block_out_head(case, d, p, form):
    ops = _ops()
    inp = problem(case, d, p)
    M = inp["M"]
    grid = ops.sas_block_grid(M)
    count = int((inp["pos"] != 0).sum())
    # the valid count as the first block's input kernel hands it over: integer partials, here split unevenly
    cnt = torch.zeros(5, dtype=torch.int32, device="cuda")
    cnt[1], cnt[4] = count // 3, count - count // 3
    div = None if form == "count_parts" else float(count + 3)
    divisor = None if div is None else torch.full((1,), div, dtype=F32, device="cuda")
    b = out_bufs(M, d, True, grid)
    run_out_head(inp, b, grid, cnt, divisor)
    b.check_written()
    out = parts3(b.out, "lnpart", grid, d)
    zero = inp["pos"] == 0
    assert bool((out["dpl"][zero] == 0).all()) and bool((out["dnl"][zero] == 0).all())
    report("block_out_head", (M, d, p, form), R.check_block_out(inp, out, head=True, divisor=div))


@pytest.mark.parametrize("case,d,p", PARAMS)
def test_block_out_bwd(case, d, p):
    ops = _ops()
    inp = problem(case, d, p)
    M = inp["M"]
    grid = ops.sas_block_parts(M)
    b, c, e = out_bwd_bufs(M, d, grid, True), out_bwd_bufs(M, d, grid, False), out_bwd_bufs(M, d, grid, False)
    run_out_bwd(inp, b, o=inp["o"], delta=b["delta"])
    run_out_bwd(inp, c)
    run_out_bwd_plain(inp, e)
    for x in (b, c, e):
        x.check_written()
    for k in c.full:                                        # with and without delta, either entry point: the same bits
        assert torch.equal(b.out[k], c.out[k]) and torch.equal(b.out[k], e.out[k]), k
    report("block_out_bwd", (M, d, p), R.check_block_out_bwd(inp, parts3(b.out, "part", grid, d)))


@pytest.mark.parametrize("case,d,p", [q for q in PARAMS if q[2] == 0.2])
def test_block_in_bwd(case, d, p):
    inp = problem(case, d, p)
    M = inp["M"]
    grid = _ops().sas_block_parts(M)
    b = in_bwd_bufs(M, d, grid)
    run_in_bwd(inp, b)
    b.check_written()
    report("block_in_bwd", (M, d), R.check_block_in_bwd(inp, parts3(b.out, "part", grid, d)))


def test_error_codes_launch_nothing(monkeypatch):
    """unsupported width, M = 0, o without delta (and the reverse), ldx not a multiple of 8: the documented code,
    and no launch (every output still holds its sentinel)"""
    from rbm_amd import _lib
    ops = _ops()
    ARG, UNSUPPORTED = 1001, 1002
    codes = []
    monkeypatch.setattr(ops, "call", lambda name, *a: codes.append((name, getattr(_lib.lib(), name)(*a))))

    def code(fn):
        codes.clear()
        fn()
        assert len(codes) == 1
        return codes[0][1]

    M = 17
    cnt = torch.ones(4, dtype=torch.int32, device="cuda")
    one = torch.ones(1, dtype=F32, device="cuda")
    bufs = []

    # ---- d = 256
    inp = R.make_inputs(M, 256, 0.0, 256, dev="cuda", seed=1)
    inp["sb"] = torch.full((1,), SEED, dtype=torch.int64, device="cuda")
    grid = ops.sas_block_grid(M)
    b = in_bufs(M, 256)
    b.add("x0", 256)
    assert code(lambda: run_in(inp, b, inp["x"])) == UNSUPPORTED
    assert code(lambda: run_in_embed(inp, b, cnt)) == ARG            # documented: d in {64, 128}, else RS_ERR_ARG
    c = out_bufs(M, 256, True, grid)
    assert code(lambda: ops.sas_block_out(*out_args(inp, c))) == UNSUPPORTED
    assert code(lambda: run_out_head(inp, c, grid, cnt, one)) == UNSUPPORTED
    e = out_bwd_bufs(M, 256, grid, True)
    assert code(lambda: run_out_bwd(inp, e, o=inp["o"], delta=e["delta"])) == UNSUPPORTED
    f = in_bwd_bufs(M, 256, grid)
    assert code(lambda: run_in_bwd(inp, f)) == UNSUPPORTED
    bufs += [b, c, e, f]

    # ---- M = 0, o / delta unpaired, ldx % 8 != 0 at a supported width
    inp = R.make_inputs(M, 64, 0.0, 256, dev="cuda", seed=1)
    inp["sb"] = torch.full((1,), SEED, dtype=torch.int64, device="cuda")
    b = in_bufs(M, 64)
    b.add("x0", 64)
    assert code(lambda: run_in(inp, b, inp["x"][:0])) == ARG
    assert code(lambda: run_in_embed(inp, b, cnt, ids=inp["ids"][:0], x0=b["x0"][:0])) == ARG
    odd = torch.zeros(M, 64 + 4, dtype=BF, device="cuda")
    assert code(lambda: run_in(inp, b, odd[:, :64])) == ARG
    c = out_bufs(M, 64, True, grid)
    assert code(lambda: ops.sas_block_out(*out_args(inp, c, o=inp["o"][:0]))) == ARG
    assert code(lambda: run_out_head(inp, c, 0, cnt, one, o=inp["o"][:0])) == ARG
    e = out_bwd_bufs(M, 64, grid, True)
    assert code(lambda: run_out_bwd(inp, e, dxn=inp["dxn"][:0])) == ARG
    assert code(lambda: run_out_bwd(inp, e, o=inp["o"])) == ARG
    assert code(lambda: run_out_bwd(inp, e, delta=e["delta"])) == ARG
    f = in_bwd_bufs(M, 64, grid)
    assert code(lambda: run_in_bwd(inp, f, dq=inp["dq"][:0])) == ARG
    bufs += [b, c, e, f]
    for x in bufs:
        x.check_untouched()
