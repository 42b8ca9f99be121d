#!/usr/bin/env python
"""Times SASRec training with the tied full-catalogue cross-entropy loss against the sampled BCE step (GPU only).

    python tools/sas_ce_bench.py [--reps 50] [--rounds 3] [--out profiles/sas_ce_bench.json] [--configs cfg2,cfg4]

At the cfg2 head shape (B 128, T 200, V 3,416, d 128) and the cfg4 one (B 128, T 50, V 54,542, d 128, Beauty-shaped
history lengths from rbm_amd.data), bf16, 2 blocks, dropout 0.2, one JSON line per shape:
  * ms/step of the captured fused step (median over --reps graph replays, each between its own pair of HIP events,
    in --rounds interleaved rounds) with loss="ce" -- the two sas_ce.hip row kernels (RS_SAS_CE_ROWS=1, default) and
    the composed launches they replace (RS_SAS_CE_ROWS=0) -- and with loss="bce";
  * device time of each launch of the CE head on that step's own buffers (graph replay of the one launch);
  * the row kernels' A/B: rs_sas_ce_rows_fwd against rs_layernorm_fwd + rs_compact_rows + rs_gather_rows, and
    rs_sas_ce_rows_bwd against rs_splitk_scatter_rows + rs_layernorm_bwd.
No pass / fail.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rbm_amd  # noqa: E402,F401
import rbm_amd.data as synth  # noqa: E402
from rbm_amd import ops  # noqa: E402
from rbm_amd.models import model_factory  # noqa: E402
from rbm_amd.models.sas_model.heads import CEHead  # noqa: E402
from rbm_amd.models.sas_model.sas import LN_EPS  # noqa: E402
from rbm_amd.train_step import FusedTrainStep  # noqa: E402

CONFIGS = {"cfg2": dict(V=3416, T=200, d=128, L=2, h=1, p=0.2, B=128, shape="ml-1m"),
           "cfg4": dict(V=54542, T=50, d=128, L=2, h=1, p=0.2, B=128, shape="beauty")}


def replay_us(g, reps, warmup=5):
    for _ in range(warmup):
        g.replay()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        g.replay()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev)


def launch_us(fn, reps):
    """Median device time of fn's launches replayed as one graph."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return round(replay_us(g, reps), 2)


def model(cfg, seed=0):
    torch.manual_seed(seed)
    a = argparse.Namespace(model_code="sas", num_items=cfg["V"], max_len=cfg["T"], device="cuda",
                           sas_hidden_units=cfg["d"], sas_num_blocks=cfg["L"], sas_heads=cfg["h"],
                           sas_dropout=cfg["p"], l2_emb=0.0, rs_dtype="bf16")
    m = model_factory(a)
    m.train()
    return m


def step_graph(cfg, batch, loss, rows):
    os.environ["RS_SAS_CE_ROWS"] = rows
    t = FusedTrainStep(model(cfg), lr=1e-3, loss=loss)
    t.capture(*batch, warmup=3)
    os.environ.pop("RS_SAS_CE_ROWS")
    return t


def head_launches(cfg, batch, reps):
    """Device time of each launch of the CE head, on the buffers of one eager forward + backward."""
    os.environ.pop("RS_SAS_CE_ROWS", None)
    m = model(cfg)
    eng = m.sas.engine()
    eng.sync_compute_weights()
    out = torch.zeros(4, device="cuda")
    grad = torch.zeros(eng.flat.numel, device="cuda")
    seq, pos = batch[0], batch[1]
    s = eng.rows_forward(CEHead(), seq, pos, (), True, out)
    eng.rows_backward(s, grad)
    torch.cuda.synchronize()
    c, g = s["ce"], eng.ws.get
    M, d, cap, V1 = seq.numel(), eng.d, c["cap"], c["V1"]
    f32, bf = torch.float32, torch.bfloat16
    x, labels = s["xL"], pos.reshape(-1)
    E, gl, bl = eng.W("item_emb.weight"), eng.Wf("last_layernorm.weight"), eng.Wf("last_layernorm.bias")
    idx, rank, cnt, hl, lab, div = g("ce_idx", (cap,), torch.int32), c["rank"], c["cnt"], c["hl"], c["lab"], c["div"]
    mu, rs, wce = c["mu"], c["rs"], c["wce"]
    dl, slab, sk, slab_d = c["dlogits"], c["slab_dE"], c["dh_splits"], c["slab_dh"]
    GE = eng.flat.view("item_emb.weight", grad)
    dx, part = g("ce_dx", (M, d), bf), g("ce_lnp", (2 * d * ops.sas_ce_rows_nparts(M),), f32)
    f, mu_f, rs_f = torch.empty(M, d, dtype=bf, device="cuda"), torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    df, wln = torch.empty(M, d, dtype=bf, device="cuda"), torch.empty(2 * 512 * d, device="cuda")
    dg, db = torch.zeros(d, device="cuda"), torch.zeros(d, device="cuda")
    ops.layernorm_fwd(x, gl, bl, LN_EPS, f, mu_f, rs_f, 0)

    def comp_fwd():
        ops.layernorm_fwd(x, gl, bl, LN_EPS, f, mu_f, rs_f, 0)
        ops.compact_rows(labels, cap, idx, rank, cnt)
        ops.gather_rows(f, idx, cnt, cap, hl, labels, lab)

    def comp_bwd():
        ops.splitk_scatter_rows(slab_d, sk, cap, rank, df)
        ops.layernorm_bwd(x, df, gl, mu_f, rs_f, LN_EPS, dx, dg, db, wln, 0)
    r = {"valid_rows": int(cnt.item()), "rows": M, "dh_splits": sk}
    r["rows_fwd_us"] = launch_us(lambda: ops.sas_ce_rows_fwd(x, labels, cap, gl, bl, LN_EPS, idx, rank, cnt, hl, lab,
                                                             mu, rs, divisor=div), reps)
    r["rows_fwd_composed_us"] = launch_us(comp_fwd, reps)
    r["vocab_head_fwd_us"] = launch_us(lambda: ops.vocab_head_fwd(hl, E, None, lab, wce, out, rows_dev=cnt,
                                                                  count_override=div), reps)
    r["vocab_head_bwd_us"] = launch_us(lambda: ops.vocab_head_bwd(hl, E, None, lab, wce, div, dl, rows_dev=cnt), reps)
    r["dE_wgrad_us"] = launch_us(lambda: ops.linear_wgrad(dl, hl, GE, slab, rows_dev=cnt, accumulate=True), reps)
    r["dh_gemm_us"] = launch_us(lambda: ops.gemm(dl, E, slab_d, cap, d, V1, False, True, ops.epilogue(rows_dev=cnt),
                                                 split_k=sk, slab=slab_d), reps)
    r["rows_bwd_us"] = launch_us(lambda: ops.sas_ce_rows_bwd(slab_d, sk, cap, rank, x, gl, mu, rs, dx, part), reps)
    r["rows_bwd_composed_us"] = launch_us(comp_bwd, reps)
    r["head_us"] = round(sum(r[k] for k in ("rows_fwd_us", "vocab_head_fwd_us", "vocab_head_bwd_us", "dE_wgrad_us",
                                            "dh_gemm_us", "rows_bwd_us")), 2)
    r["dlogits_bytes"] = cap * c["V1p"] * 2
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--configs", default="cfg2,cfg4")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sas_ce_bench needs a GPU"
    lines = []
    for name in a.configs.split(","):
        cfg = CONFIGS[name]
        rng = np.random.default_rng(0)
        zipf = synth.ZipfItems(cfg["V"])
        batch = [torch.from_numpy(x).cuda() for x in
                 synth.sas_batch(rng, cfg["B"], cfg["T"], cfg["V"], shape=cfg["shape"], zipf=zipf)]
        r = {"config": name, **{k: cfg[k] for k in ("B", "T", "V", "d", "L", "p")}, "dtype": "bf16", "reps": a.reps}
        steps = {"ce": step_graph(cfg, batch, "ce", "1"), "ce_composed_rows": step_graph(cfg, batch, "ce", "0"),
                 "bce": step_graph(cfg, batch, "bce", "1")}
        packed = torch.stack(batch)
        ms = {k: [] for k in steps}
        for _ in range(a.rounds):                 # interleaved rounds
            for k, t in steps.items():
                t.packed.copy_(packed)
                ms[k].append(round(replay_us(t.g_compute, a.reps) / 1e3, 4))
        for k, v in ms.items():
            r[f"step_ms_{k}"] = v
        r["ce_over_bce"] = round(statistics.median(ms["ce"]) / statistics.median(ms["bce"]), 2)
        del steps
        r.update(head_launches(cfg, batch, a.reps))
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
