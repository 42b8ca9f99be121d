"""rs_sas_block_in_attn (block_in_attn.hip): the first SAS block's embed-form input chain and its attention forward in
one launch.

Kernel level: the per-tile code is the two launches' own, so every tensor either of them writes (x0, Q, mean, rstd, q,
kv, o, lse) must equal rs_sas_block_in (embed form) + rs_attn_fwd on the same inputs and seeds bit for bit, and the
position counts must sum to (pos != 0).sum() over EVERY slot of count_parts (the entry writes them all).  Shapes: one
tile (T = 16), a ragged last tile (T = 37), 13 tiles with two unequal splits and image rows past T (T = 200); B = 3, 8
and 9 (B % 8 zero and non-zero: the XCD remap of the grid); ids with a padded prefix, a whole 16-row tile of zeros, a
zero in the last row and one all-padding sequence.  T = 16 and 37 run one workgroup per sequence (the engine's gate
keeps such shapes on the two launches; here the entry is called directly).  Outputs are pre-filled with NaN and
followed by guard rows that must stay NaN.

One case holds every output per element to the float64 references of rowchain_ref / attn_ref under their own bounds,
so equality with the two launches is not the only witness.  Model level: training steps of a small bf16 SASRec with
RS_SAS_IN_ATTN_FUSE on and off, eager and captured, bit for bit."""
import argparse
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import attn_ref as A
import rowchain_ref as R

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
SALT_E, SALT_A, SEED = 0x1234_5678_9ABC_DEF1, 0x2B2B_7777_8888_9999, 977
ARG, UNSUPPORTED = 1001, 1002
NAMES = ("x0", "Q", "mean", "rstd", "q", "kv", "o", "lse")
SHAPES = [(B, T) for T in (16, 37, 200) for B in (3, 8, 9)]
PARAMS = [(B, T, d, p) for d in (64, 128) for (B, T) in SHAPES for p in (0.0, 0.2)]


def _ops():
    from rbm_amd import ops
    return ops


@functools.lru_cache(maxsize=4)
def problem(B, T, d, p):
    M = B * T
    inp = R.make_inputs(M, d, p, 256, dev="cuda", seed=11)      # ids: padded prefix, a zero tile, a zero last row
    inp["T"], inp["B"], inp["Ptab"] = T, B, inp["Ptab"][:T].contiguous()
    inp["ids"][T:2 * T] = 0                                     # one all-padding sequence
    inp["pos"][T:2 * T] = 0
    inp["sb"] = torch.full((1,), SEED, dtype=torch.int64, device="cuda")
    return inp


def bufs(M, d):
    cols = {"x0": d, "Q": d, "mean": None, "rstd": None, "q": d, "kv": 2 * d, "o": d, "lse": None}
    return {n: torch.full((M + R.GUARD,) if c is None else (M + R.GUARD, c), math.nan,
                          dtype=F32 if c is None else BF, device="cuda") for n, c in cols.items()}


def check_written(b, M):
    torch.cuda.synchronize()
    for n, t in b.items():
        assert not torch.isnan(t[:M]).any(), f"{n}: rows below M left unwritten"
        assert torch.isnan(t[M:]).all(), f"{n}: store past M"


def _chain_args(inp, b, cnt):
    M = inp["M"]
    return (inp["ids"], inp["T"], inp["E"], inp["Ptab"], inp["scale"], inp["p"], SALT_E, inp["sb"], b["x0"][:M],
            inp["pos"], cnt, inp["ln1w"], inp["ln1b"], R.EPS, b["Q"], b["mean"], b["rstd"], inp["Wq"], inp["bq"],
            b["q"], inp["Wkv"], inp["bkv"], b["kv"])


def run_two(inp, b, cnt):
    ops, (B, T, d, M) = _ops(), (inp["B"], inp["T"], inp["d"], inp["M"])
    ops.sas_block_in_embed(*_chain_args(inp, b, cnt))
    ops.attn_fwd(B, T, 1, d, b["q"][:M], b["kv"][:M, :d], b["kv"][:M, d:], b["o"][:M], b["lse"], 1.0 / math.sqrt(d), 0,
                 inp["ids"], inp["p"], SALT_A, inp["sb"])


def run_fused(inp, b, cnt):
    _ops().sas_block_in_attn(*_chain_args(inp, b, cnt), b["o"], b["lse"], 1.0 / math.sqrt(inp["d"]), SALT_A)


def fused_counts(inp):
    """count slots for the fused entry: its grid and three more, holding garbage that must be overwritten"""
    ns = _ops().sas_block_in_attn_nsplit(inp["d"], inp["B"], inp["T"])
    assert ns >= 1
    return torch.full((ns * inp["B"] + 3,), 12345, dtype=torch.int32, device="cuda"), ns


@pytest.mark.parametrize("B,T,d,p", PARAMS)
def test_fused_equals_the_two_launches(B, T, d, p):
    ops = _ops()
    inp = problem(B, T, d, p)
    M = inp["M"]
    ref, got = bufs(M, d), bufs(M, d)
    rcnt = torch.zeros(ops.sas_block_grid(M), dtype=torch.int32, device="cuda")
    gcnt, ns = fused_counts(inp)
    assert ns == (2 if T == 200 else 1)        # the split regime this shape is here for
    run_two(inp, ref, rcnt)
    run_fused(inp, got, gcnt)
    check_written(ref, M)
    check_written(got, M)
    for n in NAMES:
        r, g = ref[n][:M], got[n][:M]
        same = torch.equal(r.view(torch.int16 if r.dtype == BF else torch.int32),
                           g.view(torch.int16 if g.dtype == BF else torch.int32))
        assert same, (n, int((r.float() != g.float()).sum()), "elements differ")
    valid = int((inp["pos"] != 0).sum())
    assert int(rcnt.sum()) == valid and int(gcnt.sum()) == valid, (int(rcnt.sum()), int(gcnt.sum()), valid)


def _mask(rows, cols, p, salt, sb):
    """keep multiplier of a dropout site with element index row * cols + col (the kernels' own hash)"""
    ones = torch.ones(rows, cols, dtype=F32, device="cuda")
    out = torch.empty_like(ones)
    _ops().dropout_rowmask(ones, p, salt, sb, None, out)
    return out


def test_fused_results_against_the_float64_references():
    """d = 128, T = 37, B = 3, dropout 0.2: the chain's outputs under rowchain_ref's bounds (x0 from the tables, the
    rest staged on the stored x0), the attention's under attn_ref's (staged on the stored q, kv)"""
    B, T, d, p = 3, 37, 128, 0.2
    inp = dict(problem(B, T, d, p))
    M = inp["M"]
    inp["me"] = _mask(M, d, p, SALT_E, inp["sb"]) > 0
    got = bufs(M, d)
    gcnt, _ = fused_counts(inp)
    run_fused(inp, got, gcnt)
    check_written(got, M)
    out = {n: t[:M] for n, t in got.items()}
    res = {**R.check_embed(inp, out), **R.check_block_in(inp, out, x=out["x0"])}
    c = A.Case(B, 1, d, T, 0)
    m = _mask(B * T, c.Tp, p, SALT_A, inp["sb"])[:, :T].reshape(B, T, T)
    ares = A.check_fwd(c, {"q": out["q"], "kv": out["kv"], "ids": inp["ids"].view(B, T)}, m,
                       {"o": out["o"], "lse": out["lse"]})
    res.update({k: v[0] for k, v in ares.items()})
    print("\nblock_in_attn err/bound:", {k: round(v, 4) for k, v in res.items()})
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, bad


def test_bad_arguments_launch_nothing():
    """M != B T, a NULL output, count_ids without count_parts, too few count slots: RS_ERR_ARG; another width, a
    sequence longer than the LDS attention takes: RS_ERR_UNSUPPORTED; and nothing is written"""
    import rbm_amd._lib as L
    ops = _ops()
    B, T, d = 8, 200, 64
    inp = problem(B, T, d, 0.0)
    M = inp["M"]
    b = bufs(M, d)
    cnt, ns = fused_counts(inp)

    def args(**set_):
        a = ops._sas_args(L.SasEmbedArgs, ids=inp["ids"], item_emb=inp["E"], pos_emb=inp["Ptab"], T=T,
                          scale=inp["scale"], drop_p=0.0, salt=SALT_E, seed_base=inp["sb"], x0=b["x0"],
                          count_ids=inp["pos"], count_parts=cnt)
        i = ops._sas_in(b["x0"][:M], inp["ln1w"], inp["ln1b"], R.EPS, b["Q"], b["mean"], b["rstd"], inp["Wq"],
                        inp["bq"], b["q"], inp["Wkv"], inp["bkv"], b["kv"], embed=a)
        k = ops._sas_args(L.SasInAttnArgs, B=B, o=b["o"], lse=b["lse"], scale=0.125, drop_p=0.0, salt=SALT_A,
                          ncount=cnt.numel(), **{"in": i})
        for name, v in set_.items():
            obj = k
            *path, leaf = name.split("__")
            for q in path:
                obj = getattr(obj, q)
            setattr(obj, leaf, v)
        return k

    def code(width, **set_):
        return L.lib().rs_sas_block_in_attn(width, C.byref(args(**set_)), None)

    assert code(d, B=B + 1) == ARG
    assert code(d, in__M=0) == ARG
    assert code(d, o=None) == ARG
    assert code(d, lse=None) == ARG
    assert code(d, in__kv=None) == ARG
    assert code(d, in__e__item_emb=None) == ARG
    assert code(d, in__e__count_parts=None) == ARG                      # count_ids without count_parts
    assert code(d, ncount=ns * B - 1) == ARG
    assert code(d, in__e__x0=b["x0"].data_ptr() + 2) == ARG             # misaligned
    assert L.lib().rs_sas_block_in_attn(d, None, None) == ARG
    assert code(96) == UNSUPPORTED
    assert code(d, in__e__T=400, B=M // 400) == UNSUPPORTED             # T beyond the LDS attention's 256
    assert ops.sas_block_in_attn_nsplit(96, B, T) == 0 and ops.sas_block_in_attn_nsplit(d, B, 400) == 0
    torch.cuda.synchronize()
    for n, t in b.items():
        assert torch.isnan(t).all(), f"{n}: written by a call that must not launch"
    assert bool((cnt == 12345).all())


# ------------------------------------------------------------------ model level
MB, MT, MV = 8, 128, 500      # 8 tiles per sequence: two workgroups per sequence, the engine's gate is on


def _model(d):
    import rbm_amd  # noqa: F401
    from rbm_amd.models import model_factory
    torch.manual_seed(0)
    a = argparse.Namespace(model_code="sas", num_items=MV, max_len=MT, device="cuda", sas_hidden_units=d,
                           sas_num_blocks=2, sas_heads=1, sas_dropout=0.2, l2_emb=0.0, rs_dtype="bf16")
    return model_factory(a)


@functools.lru_cache(maxsize=1)
def _batches():
    import rbm_amd.data as synth
    rng = np.random.default_rng(5)
    return [torch.stack([torch.from_numpy(x) for x in synth.sas_batch(rng, MB, MT, MV)]).cuda() for _ in range(3)]


def _run(d, captured):
    """three steps (the first is the capture's warmup step): the two losses after it and every parameter"""
    from rbm_amd.train_step import FusedTrainStep
    bs = _batches()
    st = FusedTrainStep(_model(d), lr=1e-3)
    if captured:
        st.capture(*bs[0].unbind(0), warmup=1, steps_per_graph=2)
        losses = st.replay_packed(torch.stack(bs[1:3])).tolist()
    else:
        losses = [st.step(*b.unbind(0)).item() for b in bs][1:]
    torch.cuda.synchronize()
    assert len(losses) == 2 and all(math.isfinite(x) for x in losses)
    return st, (losses, st.flat.data.clone())


def test_training_steps_equal_with_the_switch_on_and_off(monkeypatch):
    ops = _ops()
    d = 64
    assert ops.sas_block_in_attn_nsplit(d, MB, MT) >= 2
    n = {"fused": 0, "embed": 0}

    def count(name, key):
        fn = getattr(ops, name)

        def wrapped(*a, **k):
            n[key] += 1
            return fn(*a, **k)
        monkeypatch.setattr(ops, name, wrapped)
    count("sas_block_in_attn", "fused")
    count("sas_block_in_embed", "embed")
    runs = {}
    for switch in ("1", "0"):
        for captured in (False, True):
            monkeypatch.setenv("RS_SAS_IN_ATTN_FUSE", switch)
            n.update(fused=0, embed=0)
            st, runs[(switch, captured)] = _run(d, captured)
            assert st.engine.in_attn_fuse == (switch == "1")
            assert (n["fused"] > 0, n["embed"] > 0) == ((True, False) if switch == "1" else (False, True)), n
    ref = runs[("0", False)]
    for key, r in runs.items():
        assert r[0] == ref[0], (key, r[0], ref[0])
        assert torch.equal(r[1], ref[1]), key
