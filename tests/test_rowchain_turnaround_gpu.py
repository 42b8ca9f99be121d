"""The forward/backward turnaround launch of rowchain.hip (rs_sas_block_out_head_bwd): the last block's output chain,
the SAS head and that block's output-side backward in one kernel, dx_L / h1 / x1 / o / mean2 / rstd2 handed over in
registers.  The criterion is BIT EQUALITY with the two composed launches it replaces (rs_sas_block_out_head, then
rs_sas_block_out_bwd_delta on the tensors the first one stored), for every stored tensor, both LayerNorm partial sets
and the BCE partials, at row counts on both sides of the one-tile-per-wave limit (above it the entry runs the two
kernels itself), with and without delta, with a given divisor and with the counted one; at M = 205, d = 128 the fused
results are also held to the float64 reference of tests/rowchain_ref.py under its own bounds.  Outputs are pre-filled
with NaN and carry guard rows (test_rowchain_gpu.Bufs); the buffers are compared whole, guards included, as integers.

Model level: five training steps of a small bf16 SASRec with the launch on and off (RS_SAS_TURNAROUND_FUSE), eager and
as a captured two-step graph: the same losses and parameters, bit for bit; also with the transposed weights written
by the forward's side branch instead of the optimizer, and with the block-boundary launches off."""
import argparse
import functools
import math

import numpy as np
import pytest
import torch

import rowchain_ref as R
import test_rowchain_gpu as RC

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
ARG, UNSUPPORTED = 1001, 1002


def _ops():
    from rbm_amd import ops
    return ops


def row_counts():
    """label -> M (G = the part's CU count): one tile; 7 tiles (grid < 8: the non-XCD dealing); 13 tiles with a
    ragged last one; the last size at which every wave has at most one tile; the first that needs two launches;
    a size that is no multiple of 128"""
    G = RC.ncu()
    return {"1": 1, "100": 100, "205": 205, "last_fused": 16 * 8 * G - 11, "first_split": 16 * 8 * G + 1,
            "4135": 4135}


LABELS = ("1", "100", "205", "last_fused", "first_split", "4135")
PARAMS = [(m, d, p) for d in (64, 128) for m in LABELS for p in (0.0, 0.2)]


@functools.lru_cache(maxsize=2)
def problem(label, d, p):
    M = row_counts()[label]
    inp = R.make_inputs(M, d, p, RC.ncu(), dev="cuda", seed=13)
    inp["sb"] = torch.full((1,), RC.SEED, dtype=torch.int64, device="cuda")
    assert bool((inp["ids"] == 0).any()) and bool((inp["pos"] == 0).any())     # padding ids and pos == 0 rows
    if M > 16:
        assert bool((inp["ids"] != 0).any()) and bool((inp["pos"] != 0).any())
    return inp


def bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def same_bits(a, b, what, skip=()):
    for k in a.full:
        if k not in skip:
            assert torch.equal(bits(a[k]), bits(b[k])), (what, k)


def counts(inp):
    """the valid count as the first block's input kernel hands it over (integer partials, split unevenly) and a
    divisor that differs from it"""
    count = int((inp["pos"] != 0).sum())
    cnt = torch.zeros(5, dtype=torch.int32, device="cuda")
    cnt[1], cnt[4] = count // 3, count - count // 3
    return cnt, torch.full((1,), float(count + 3), dtype=F32, device="cuda"), count


def head_args(inp, b, grid, cnt, divisor, dx="buf"):
    return (inp["E"], inp["pos"], inp["neg"], inp["lnlw"], inp["lnlb"], cnt, divisor, b["f"], b["pl"], b["nl"],
            b["dpl"], b["dnl"], b["dx"] if dx == "buf" else dx, b["lnpart"], b["part"][:grid])


def run_fused(inp, fo, fb, grid, cnt, divisor, delta, dx="buf"):
    _ops().sas_block_out_head_bwd(RC.out_args(inp, fo), head_args(inp, fo, grid, cnt, divisor, dx), inp["W2T"],
                                  inp["W1T"], inp["WoT"], fb["dy2"], fb["da1"], fb["dx1"], fb["dout"], fb["part"],
                                  fb["delta"] if delta else None)


def run_composed_bwd(inp, co, cb, delta):
    """rs_sas_block_out_bwd_delta on what the composed forward stored (not the table's own backward inputs)"""
    M = inp["M"]
    _ops().sas_block_out_bwd(co["dx"][:M], inp["ids"], co["h1"][:M], co["x1"][:M], co["mean"][:M], co["rstd"][:M],
                             inp["ln2w"], inp["W2T"], inp["W1T"], inp["WoT"], cb["dy2"], cb["da1"], cb["dx1"],
                             cb["dout"], cb["part"], inp["p"], RC.SALT_1, RC.SALT_2, inp["sb"],
                             o=inp["o"] if delta else None, delta=cb["delta"] if delta else None)


def check_fused_written(fo, fb, one_launch):
    """every output written below M and nothing past it; dx only by the two-launch path"""
    torch.cuda.synchronize()
    dx = fo.full.pop("dx")
    try:
        fo.check_written(), fb.check_written()
    finally:
        fo.full["dx"] = dx
    if one_launch:
        assert bool(torch.isnan(dx).all()), "the one-launch kernel must not write the dx scratch"
    else:
        assert not torch.isnan(dx[:fo.M]).any() and bool(torch.isnan(dx[fo.M:]).all())


def test_row_counts_sit_on_both_sides_of_the_limit():
    ops = _ops()
    G, rows = RC.ncu(), row_counts()
    for d in (64, 128):
        assert ops.sas_block_boundary_fused(rows["last_fused"], d) and -(-rows["last_fused"] // 16) == 8 * G
        assert not ops.sas_block_boundary_fused(rows["first_split"], d)
        for k in ("1", "100", "205"):
            assert ops.sas_block_boundary_fused(rows[k], d)
    assert ops.sas_block_grid(100) == 7 and ops.sas_block_grid(205) == 13
    assert ops.sas_block_grid(rows["last_fused"]) == G


@pytest.mark.parametrize("label,d,p", PARAMS)
def test_block_out_head_bwd_equals_composed(label, d, p):
    ops = _ops()
    inp = problem(label, d, p)
    M = inp["M"]
    grid = ops.sas_block_grid(M)
    assert grid == ops.sas_block_parts(M)
    one_launch = ops.sas_block_boundary_fused(M, d)
    cnt, div, _ = counts(inp)
    for divisor in (div, None):
        co = RC.out_bufs(M, d, True, grid)
        RC.run_out_head(inp, co, grid, cnt, divisor)
        co.check_written()
        for delta in (True, False):
            cb = RC.out_bwd_bufs(M, d, grid, delta)
            run_composed_bwd(inp, co, cb, delta)
            cb.check_written()
            fo, fb = RC.out_bufs(M, d, True, grid), RC.out_bwd_bufs(M, d, grid, delta)
            run_fused(inp, fo, fb, grid, cnt, divisor, delta)
            check_fused_written(fo, fb, one_launch)
            what = f"divisor={'given' if divisor is not None else 'counted'} delta={delta}"
            same_bits(fo, co, "forward " + what, skip=("dx",) if one_launch else ())
            same_bits(fb, cb, "backward " + what)
    if one_launch:                                           # no scratch: allowed exactly where the path is certain
        fo, fb = RC.out_bufs(M, d, True, grid), RC.out_bwd_bufs(M, d, grid, False)
        run_fused(inp, fo, fb, grid, cnt, None, False, dx=None)
        check_fused_written(fo, fb, True)
        same_bits(fo, co, "forward, no scratch", skip=("dx",))
        same_bits(fb, cb, "backward, no scratch")


def test_fused_results_against_the_float64_reference():
    """M = 205, d = 128, dropout 0.2: every output of the one-launch kernel against the float64 reference of
    rowchain_ref under its own bounds, so equality with the composed launches is not the only witness.  The hand-off
    dx_L exists only in registers: its reference check and the backward chain's reference input take the composed
    launch's dx, which is itself held to the reference here; the backward's other inputs (h1, x1, the row statistics)
    are the fused launch's own stored outputs."""
    ops = _ops()
    d, p = 128, 0.2
    inp = dict(problem("205", d, p))
    M = inp["M"]
    for n, salt in (("m1", RC.SALT_1), ("m2", RC.SALT_2)):
        inp[n] = RC._mask(M, d, p, salt, inp["sb"])
    assert ops.sas_block_boundary_fused(M, d)
    grid = ops.sas_block_grid(M)
    cnt, div, count = counts(inp)
    co = RC.out_bufs(M, d, True, grid)
    RC.run_out_head(inp, co, grid, cnt, div)
    co.check_written()
    fo, fb = RC.out_bufs(M, d, True, grid), RC.out_bwd_bufs(M, d, grid, True)
    run_fused(inp, fo, fb, grid, cnt, div, True)
    check_fused_written(fo, fb, True)
    out = RC.parts3({**fo.out, "dx": co.out["dx"]}, "lnpart", grid, d)
    res = {"fwd." + k: v for k, v in R.check_block_out(inp, out, head=True, divisor=float(count + 3)).items()}
    inp2 = {**inp, "dxn": co.out["dx"].clone(), "h1": fo.out["h1"], "x1": fo.out["x1"], "mean2": fo.out["mean"],
            "rstd2": fo.out["rstd"]}
    res.update({"bwd." + k: v for k, v in R.check_block_out_bwd(inp2, RC.parts3(fb.out, "part", grid, d)).items()})
    RC.report("block_out_head_bwd", (M, d, p), res)


def test_error_codes_launch_nothing(monkeypatch):
    """no dx scratch where two launches are needed, M = 0, a missing head argument, another width: the documented
    code and no launch"""
    from rbm_amd import _lib
    ops = _ops()
    codes = []
    monkeypatch.setattr(ops, "call", lambda name, *a: codes.append(getattr(_lib.lib(), name)(*a)))
    M, d = row_counts()["first_split"], 64
    inp = problem("first_split", d, 0.0)
    grid = ops.sas_block_grid(M)
    cnt, div, _ = counts(inp)
    fo, fb = RC.out_bufs(M, d, True, grid), RC.out_bwd_bufs(M, d, grid, True)
    run_fused(inp, fo, fb, grid, cnt, div, True, dx=None)                      # two launches need the scratch
    empty = dict(inp, o=inp["o"][:0])
    run_fused(empty, fo, fb, 0, cnt, div, True)                                # M = 0
    run_fused(dict(inp, E=None), fo, fb, grid, cnt, div, True)                 # no item table
    run_fused(dict(inp, pos=None), fo, fb, grid, cnt, div, True)
    assert codes == [ARG, ARG, ARG, ARG]
    wide = R.make_inputs(17, 256, 0.0, 256, dev="cuda", seed=1)
    wide["sb"] = inp["sb"]
    g17 = ops.sas_block_grid(17)
    wo, wb = RC.out_bufs(17, 256, True, g17), RC.out_bwd_bufs(17, 256, g17, True)
    codes.clear()
    run_fused(wide, wo, wb, g17, cnt, div, True)
    assert codes == [UNSUPPORTED]
    for b in (fo, fb, wo, wb):
        b.check_untouched()


# ------------------------------------------------------------------ model level
def _model(L, d):
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    torch.manual_seed(0)
    a = argparse.Namespace(model_code="sas", num_items=500, max_len=20, device="cuda", sas_hidden_units=d,
                           sas_num_blocks=L, sas_heads=1, sas_dropout=0.2, l2_emb=0.0, rs_dtype="bf16")
    return model_factory(a)


@functools.lru_cache(maxsize=1)
def _batches():
    import rbm_amd.data as synth
    rng = np.random.default_rng(5)
    return [torch.stack([torch.from_numpy(x) for x in synth.sas_batch(rng, 4, 20, 500)]).cuda() for _ in range(5)]


class _Calls:
    """counts the launches of the turnaround and of the two it replaces"""
    NAMES = ("sas_block_out_head_bwd", "sas_block_out_head", "sas_block_out_bwd")

    def __init__(self, monkeypatch):
        self.n = dict.fromkeys(self.NAMES, 0)
        ops = _ops()
        for name in self.NAMES:
            monkeypatch.setattr(ops, name, self._count(name, getattr(ops, name)))

    def _count(self, name, fn):
        def wrapped(*a, **k):
            self.n[name] += 1
            return fn(*a, **k)
        return wrapped

    def reset(self):
        self.n.update(dict.fromkeys(self.NAMES, 0))


def _run(L, d, captured, adam_transposes=True):
    """five steps (the first is the capture's warmup step): the four losses after it and every parameter"""
    from rbm_amd.train_step import FusedTrainStep
    bs = _batches()
    st = FusedTrainStep(_model(L, d), lr=1e-3)
    st.engine.adam_transposes = adam_transposes
    if captured:
        st.capture(*bs[0].unbind(0), warmup=1, steps_per_graph=2)
        losses = []
        for r in range(2):
            losses += st.replay_packed(torch.stack(bs[1 + 2 * r:3 + 2 * r])).tolist()
    else:
        losses = [st.step(*b.unbind(0)).item() for b in bs][1:]
    torch.cuda.synchronize()
    assert len(losses) == 4 and all(math.isfinite(x) for x in losses)
    return st, (losses, st.flat.data.clone())


def _same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    assert torch.equal(a[1], b[1]), what


@pytest.mark.parametrize("L,d", [(L, d) for d in (64, 128) for L in (1, 2, 3)])
def test_training_steps_equal_with_the_switch_on_and_off(L, d, monkeypatch):
    calls = _Calls(monkeypatch)
    runs = {}
    for switch in ("1", "0"):
        for captured in (False, True):
            monkeypatch.setenv("RS_SAS_TURNAROUND_FUSE", switch)
            calls.reset()
            st, runs[(switch, captured)] = _run(L, d, captured)
            assert st.engine.turnaround_fuse == (switch == "1") and st.engine.adam_transposes
            n = calls.n
            if switch == "1":                                # the one launch, and neither of the two it replaces
                assert n["sas_block_out_head"] == 0 and n["sas_block_out_head_bwd"] > 0, n
                assert n["sas_block_out_bwd"] == 0, n        # the other blocks' ride in the boundary launches
                assert captured or n["sas_block_out_head_bwd"] == 5
            else:
                assert n["sas_block_out_head_bwd"] == 0 and n["sas_block_out_head"] == n["sas_block_out_bwd"] > 0, n
    for k, r in runs.items():
        _same(r, runs[("0", False)], k)


@pytest.mark.parametrize("captured", [False, True])
def test_transposed_weights_from_the_side_branch(captured, monkeypatch):
    """adam_transposes off: every step's transposed weights are written by the forward's side branch, which the
    turnaround launch has to wait for (with the optimizer writing them it waits only in the first step)"""
    calls = _Calls(monkeypatch)
    runs = {}
    for switch in ("1", "0"):
        monkeypatch.setenv("RS_SAS_TURNAROUND_FUSE", switch)
        calls.reset()
        st, runs[switch] = _run(2, 128, captured, adam_transposes=False)
        assert st.engine._side_refreshed and (calls.n["sas_block_out_head_bwd"] > 0) == (switch == "1")
    _same(runs["1"], runs["0"], "side-refreshed")
    monkeypatch.setenv("RS_SAS_TURNAROUND_FUSE", "0")
    st, ref = _run(2, 128, captured)                         # and the optimizer-written ones give the same step
    assert not st.engine._side_refreshed
    _same(runs["1"], ref, "side-refreshed against optimizer-written")


def test_turnaround_with_the_boundary_launches_off(monkeypatch):
    calls = _Calls(monkeypatch)
    monkeypatch.setenv("RS_SAS_BOUNDARY_FUSE", "0")
    runs = {}
    for switch in ("1", "0"):
        monkeypatch.setenv("RS_SAS_TURNAROUND_FUSE", switch)
        calls.reset()
        st, runs[switch] = _run(3, 128, False)
        assert not st.engine.boundary_fuse and st.engine.turnaround_fuse == (switch == "1")
        # composed boundaries: blocks 1 and 0 launch their own output-side backward, block 2's is in the turnaround
        assert calls.n["sas_block_out_bwd"] == 5 * (2 if switch == "1" else 3), calls.n
    _same(runs["1"], runs["0"], "boundary launches off")
