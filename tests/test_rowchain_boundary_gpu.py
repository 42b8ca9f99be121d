"""The block-boundary launches of rowchain.hip (rs_sas_block_out_in, rs_sas_block_in_out_bwd): two adjacent row
chains in one kernel, the tensor between them in registers.  The criterion is BIT EQUALITY with the two composed
launches they replace (same operations on the same rounded values in the same order), for every stored tensor and
both LayerNorm partial sets, at row counts on both sides of the one-tile-per-wave limit (above it the entries run
the two single-block kernels themselves); at M = 205, d = 128 the fused results are also held to the float64
reference of tests/rowchain_ref.py under its own bounds.  Outputs are pre-filled with NaN and carry guard rows
(test_rowchain_gpu.Bufs); the buffers are compared whole, guards included, as integers.

Model level: five training steps of a small bf16 SASRec with the launches on and off (RS_SAS_BOUNDARY_FUSE), eager
and as a captured two-step graph: the same losses and parameters, bit for bit; with one block nothing is fused."""
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
ARG = 1001


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
    inp = R.make_inputs(M, d, p, RC.ncu(), dev="cuda", seed=11)
    inp["sb"] = torch.full((1,), RC.SEED, dtype=torch.int64, device="cuda")
    assert bool((inp["ids"] == 0).any()) or M == 1          # padding ids present
    return inp


def bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def same_bits(a, b, what):
    for k in a.full:
        assert torch.equal(bits(a[k]), bits(b[k])), (what, k)


def in_args(inp, b):
    return (inp["ln1w"], inp["ln1b"], R.EPS, b["Q"], b["mean"], b["rstd"], inp["Wq"], inp["bq"], b["q"], inp["Wkv"],
            inp["bkv"], b["kv"])


def run_fwd_fused(inp, bo, bi):
    _ops().sas_block_out_in(RC.out_args(inp, bo), *in_args(inp, bi))


def run_fwd_composed(inp, bo, bi):
    M = inp["M"]
    _ops().sas_block_out(*RC.out_args(inp, bo))
    RC.run_in(inp, bi, bo["xn"][:M])


def bwd_in_args(inp):
    return (inp["dq"], inp["dkv"], inp["dx1b"], inp["xb"], inp["mean1"], inp["rstd1"], inp["ln1w"], inp["WinT"])


def bwd_out_args(inp, b, delta):
    return (inp["ids"], inp["h1"], inp["x1"], inp["mean2"], inp["rstd2"], inp["ln2w"], inp["W2T"], inp["W1T"],
            inp["WoT"], b["dy2"], b["da1"], b["dx1"], b["dout"], b["part"], inp["p"], RC.SALT_1, RC.SALT_2, inp["sb"],
            inp["o"] if delta else None, b["delta"] if delta else None)


def test_row_counts_sit_on_both_sides_of_the_limit():
    ops = _ops()
    G, rows = RC.ncu(), row_counts()
    for d in (64, 128):
        assert ops.sas_block_boundary_fused(rows["last_fused"], d) and -(-rows["last_fused"] // 16) == 8 * G
        assert not ops.sas_block_boundary_fused(rows["first_split"], d)
        for k in ("1", "100", "205"):
            assert ops.sas_block_boundary_fused(rows[k], d)
    assert not ops.sas_block_boundary_fused(205, 256)
    g = ops.sas_block_grid(100)
    assert g == 7 and ops.sas_block_grid(205) == 13
    assert ops.sas_block_grid(rows["last_fused"]) == G      # a multiple of 8 on this part: the XCD-dealing branch


@pytest.mark.parametrize("label,d,p", PARAMS)
def test_block_out_in_equals_composed(label, d, p):
    inp = problem(label, d, p)
    M = inp["M"]
    fo, fi = RC.out_bufs(M, d, False, 0), RC.in_bufs(M, d)
    co, ci = RC.out_bufs(M, d, False, 0), RC.in_bufs(M, d)
    run_fwd_fused(inp, fo, fi)
    run_fwd_composed(inp, co, ci)
    for b in (fo, fi, co, ci):
        b.check_written()
    same_bits(fo, co, "out")
    same_bits(fi, ci, "in")


@pytest.mark.parametrize("label,d,p", PARAMS)
def test_block_in_out_bwd_equals_composed(label, d, p):
    ops = _ops()
    inp = problem(label, d, p)
    M = inp["M"]
    grid = ops.sas_block_parts(M)
    fused = ops.sas_block_boundary_fused(M, d)
    ci = RC.in_bwd_bufs(M, d, grid)
    RC.run_in_bwd(inp, ci)
    ci.check_written()
    dx = ci["dx"][:M]
    composed = {}
    for delta in (True, False):
        co = composed[delta] = RC.out_bwd_bufs(M, d, grid, delta)
        RC.run_out_bwd(inp, co, dxn=dx, o=inp["o"] if delta else None, delta=co["delta"] if delta else None)
        fi, fo = RC.in_bwd_bufs(M, d, grid), RC.out_bwd_bufs(M, d, grid, delta)
        ops.sas_block_in_out_bwd(bwd_in_args(inp), fi["dx"], fi["part"], bwd_out_args(inp, fo, delta))
        co.check_written(), fo.check_written()
        same_bits(fo, co, f"out delta={delta}")
        assert torch.equal(bits(fi["part"]), bits(ci["part"])), "LN1 partials"
        torch.cuda.synchronize()
        if fused:
            assert bool(torch.isnan(fi["dx"]).all()), "the one-launch kernel must not write the dx scratch"
        else:
            assert torch.equal(bits(fi["dx"]), bits(ci["dx"]))
    if fused:                                                # no scratch: allowed exactly where the path is certain
        fi, fo = RC.in_bwd_bufs(M, d, grid), RC.out_bwd_bufs(M, d, grid, True)
        ops.sas_block_in_out_bwd(bwd_in_args(inp), None, fi["part"], bwd_out_args(inp, fo, True))
        fo.check_written()
        same_bits(fo, composed[True], "out, no scratch")
        assert torch.equal(bits(fi["part"]), bits(ci["part"]))


def test_fused_results_against_the_float64_reference():
    """M = 205, d = 128, dropout 0.2: every output of the two one-launch kernels against the float64 reference of
    rowchain_ref under its own bounds, so equality with the composed launches is not the only witness.  The backward's
    hand-off dx exists only in registers: the reference of block i-1's chain is formed from the composed launch's dx,
    which is itself held to the reference here."""
    ops = _ops()
    d, p = 128, 0.2
    inp = dict(problem("205", d, p))
    M = inp["M"]
    for n, salt in (("m1", RC.SALT_1), ("m2", RC.SALT_2)):
        inp[n] = RC._mask(M, d, p, salt, inp["sb"])
    assert ops.sas_block_boundary_fused(M, d)
    fo, fi = RC.out_bufs(M, d, False, 0), RC.in_bufs(M, d)
    run_fwd_fused(inp, fo, fi)
    fo.check_written(), fi.check_written()
    RC.report("block_out_in", (M, d, p), {**{"out." + k: v for k, v in R.check_block_out(inp, fo.out).items()},
                                          **{"in." + k: v for k, v in
                                             R.check_block_in(inp, fi.out, x=fo.out["xn"]).items()}})
    grid = ops.sas_block_parts(M)
    ci = RC.in_bwd_bufs(M, d, grid)
    RC.run_in_bwd(inp, ci)
    ci.check_written()
    bi, bo = RC.in_bwd_bufs(M, d, grid), RC.out_bwd_bufs(M, d, grid, True)
    ops.sas_block_in_out_bwd(bwd_in_args(inp), bi["dx"], bi["part"], bwd_out_args(inp, bo, True))
    bo.check_written()
    torch.cuda.synchronize()
    res = R.check_block_in_bwd(inp, RC.parts3({"dx": ci.out["dx"], "part": bi.out["part"]}, "part", grid, d))
    res = {"in." + k: v for k, v in res.items()}
    inp2 = {**inp, "dxn": ci.out["dx"].clone()}
    res.update({"out." + k: v for k, v in R.check_block_out_bwd(inp2, RC.parts3(bo.out, "part", grid, d)).items()})
    RC.report("block_in_out_bwd", (M, d, p), res)


def test_error_codes_launch_nothing(monkeypatch):
    """no dx scratch where two launches are needed, M = 0, o without delta, another width: the documented code and
    no launch"""
    from rbm_amd import _lib
    ops = _ops()
    codes = []
    monkeypatch.setattr(ops, "call", lambda name, *a: codes.append(getattr(_lib.lib(), name)(*a)))
    M, d = row_counts()["first_split"], 64
    inp = problem("first_split", d, 0.0)
    grid = ops.sas_block_parts(M)
    fi, fo = RC.in_bwd_bufs(M, d, grid), RC.out_bwd_bufs(M, d, grid, True)
    ops.sas_block_in_out_bwd(bwd_in_args(inp), None, fi["part"], bwd_out_args(inp, fo, True))
    a = list(bwd_out_args(inp, fo, True))
    a[-1] = None
    ops.sas_block_in_out_bwd(bwd_in_args(inp), fi["dx"], fi["part"], tuple(a))
    empty = tuple(t[:0] if i == 0 else t for i, t in enumerate(bwd_in_args(inp)))
    ops.sas_block_in_out_bwd(empty, fi["dx"], fi["part"], bwd_out_args(inp, fo, True))
    assert codes == [ARG, ARG, ARG]
    bo, bi = RC.out_bufs(M, d, False, 0), RC.in_bufs(M, d)
    codes.clear()
    oa = list(RC.out_args(inp, bo))
    oa[0] = oa[0][:0]
    ops.sas_block_out_in(tuple(oa), *in_args(inp, bi))
    assert codes == [ARG]
    wide = R.make_inputs(17, 256, 0.0, 256, dev="cuda", seed=1)
    wide["sb"] = inp["sb"]
    wo, wi = RC.out_bufs(17, 256, False, 0), RC.in_bufs(17, 256)
    codes.clear()
    ops.sas_block_out_in(RC.out_args(wide, wo), *in_args(wide, wi))
    assert codes == [1002]
    for b in (fi, fo, bo, bi, wo, wi):
        b.check_untouched()


# ------------------------------------------------------------------ model level
def _model(L):
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    torch.manual_seed(0)
    a = argparse.Namespace(model_code="sas", num_items=500, max_len=50, device="cuda", sas_hidden_units=128,
                           sas_num_blocks=L, sas_heads=1, sas_dropout=0.2, l2_emb=0.0, rs_dtype="bf16")
    return model_factory(a)


@functools.lru_cache(maxsize=1)
def _batches():
    import rbm_amd.data as synth
    rng = np.random.default_rng(5)
    return [torch.stack([torch.from_numpy(x) for x in synth.sas_batch(rng, 4, 50, 500)]).cuda() for _ in range(5)]


@pytest.mark.parametrize("L", [1, 2, 3])
def test_training_steps_equal_with_the_switch_on_and_off(L, monkeypatch):
    """five steps (the first is the capture's warmup step), eager and as a captured graph of two steps per replay"""
    from rbm_amd.train_step import FusedTrainStep
    ops = _ops()
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = ops.sas_block_out_in, ops.sas_block_in_out_bwd

    def count(name, fn):
        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(ops, "sas_block_out_in", count("fwd", fwd))
    monkeypatch.setattr(ops, "sas_block_in_out_bwd", count("bwd", bwd))
    bs = _batches()
    runs = {}
    for switch in ("1", "0"):
        for captured in (False, True):
            monkeypatch.setenv("RS_SAS_BOUNDARY_FUSE", switch)
            calls.update(fwd=0, bwd=0)
            st = FusedTrainStep(_model(L), lr=1e-3)
            assert st.engine.boundary_fuse == (switch == "1")
            if captured:
                st.capture(*bs[0].unbind(0), warmup=1, steps_per_graph=2)
                losses = []
                for r in range(2):
                    losses += st.replay_packed(torch.stack(bs[1 + 2 * r:3 + 2 * r])).tolist()
            else:
                losses = [st.step(*b.unbind(0)).item() for b in bs][1:]
            torch.cuda.synchronize()
            runs[(switch, captured)] = (losses, st.flat.data.clone())
            if switch == "0" or L == 1:
                assert calls == {"fwd": 0, "bwd": 0}, (switch, L, calls)
            else:                                            # eager: L - 1 boundaries per direction and step
                assert calls["fwd"] == calls["bwd"] > 0
                if not captured:
                    assert calls["fwd"] == 5 * (L - 1)
    ref = runs[("0", False)]
    assert len(ref[0]) == 4 and all(math.isfinite(x) for x in ref[0])
    for k, r in runs.items():
        assert r[0] == ref[0], (k, r[0], ref[0])
        assert torch.equal(r[1], ref[1]), k
