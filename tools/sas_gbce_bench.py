#!/usr/bin/env python
"""Times SASRec training with N negatives per position (loss="gbce") against the unchanged one-negative BCE step
(GPU only).

    python tools/sas_gbce_bench.py [--reps 50] [--rounds 3] [--out profiles/sas_gbce_bench.json] [--configs cfg2,cfg4]
                                   [--ns 1,16,256]

At the cfg2 head shape (B 128, T 200, V 3,416, d 128) and the cfg4 one (B 128, T 50, V 54,542, d 128, Beauty-shaped
history lengths from rbm_amd.data), bf16, 2 blocks, dropout 0.2, one JSON line per shape:
  * ms/step of the captured fused step (median over --reps graph replays, each between its own pair of HIP events,
    in --rounds interleaved rounds: every version is replayed in turn inside one call) with loss="bce" and with
    loss="gbce" at every N, and each gbce time over the bce time of the same call;
  * device time of the new head's launches alone on that step's own buffers (graph replay of the launches):
    rs_sas_gbce_fwd, rs_sas_gbce_bwd, and the head's table-gradient launches (rs_item_index_build +
    rs_item_grad_weighted), with the gather bytes each head launch needs -- valid rows x (1 + N) x d x 2 table bytes, the
    rows themselves and the logits / weights / keys it writes, counted from the shapes -- and the achieved bytes/s over
    the HBM peak (8.0 TB/s, the part's specification);
  * the bytes of the engine's gbce_* buffers.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rbm_amd  # noqa: E402,F401
import rbm_amd.data as synth  # noqa: E402
from rbm_amd import ops  # noqa: E402
from rbm_amd.models import model_factory  # noqa: E402
from rbm_amd.models.sas_model.heads import GBCEHead  # noqa: E402
from rbm_amd.train_step import FusedTrainStep  # noqa: E402
from sas_ce_bench import CONFIGS, launch_us, model, replay_us  # noqa: E402

HBM_PEAK = 8.0e12       # bytes/s, the MI355X's specified HBM3E bandwidth


def gbce_model(cfg, N, seed=0):
    torch.manual_seed(seed)
    a = argparse.Namespace(model_code="sas", num_items=cfg["V"], max_len=cfg["T"], device="cuda",
                           sas_hidden_units=cfg["d"], sas_num_blocks=cfg["L"], sas_heads=cfg["h"],
                           sas_dropout=cfg["p"], l2_emb=0.0, rs_dtype="bf16", sas_loss="gbce", sas_negs=N)
    m = model_factory(a)
    m.train()
    return m


def head_launches(cfg, batch, neg, reps):
    """Device time of the gBCE head's launches, on the buffers of one eager forward + backward."""
    N = neg.shape[2]
    m = gbce_model(cfg, N)
    eng = m.sas.engine()
    eng.sync_compute_weights()
    out = torch.zeros(4, device="cuda")
    grad = torch.zeros(eng.flat.numel, device="cuda")
    s = eng.rows_forward(GBCEHead(1.0), batch[0], batch[1], (neg,), True, out)
    eng.rows_backward(s, grad)
    torch.cuda.synchronize()
    c = s["ce"]
    cap, d = c["cap"], eng.d
    E, GE = eng.W("item_emb.weight"), eng.flat.view("item_emb.weight", grad)
    keys, w, iws, rows = c["keys"], c["w"], c["iws"], c["index_rows"]
    n = int(c["cnt"].item())

    def table():
        ops.item_index_build([keys], rows, d, iws)
        ops.item_grad_weighted(iws, cap, 1 + N, c["hl"], w, GE, table_rows=rows)
    r = {"valid_rows": n}
    r["gbce_fwd_us"] = launch_us(lambda: ops.sas_gbce_fwd(c["hl"], c["lab"], c["idx"], c["cnt"], cap, E, neg, N, 1.0,
                                                          c["div"], c["gbce_ws"], out), reps)
    r["gbce_bwd_us"] = launch_us(lambda: ops.sas_gbce_bwd(c["hl"], c["lab"], c["idx"], c["cnt"], cap, E, neg, N, 1.0,
                                                          c["div"], None, c["gbce_ws"], c["dh"], w, keys), reps)
    r["gbce_table_grad_us"] = launch_us(table, reps)
    r["gbce_head_us"] = round(r["gbce_fwd_us"] + r["gbce_bwd_us"] + r["gbce_table_grad_us"], 2)
    # bytes from the shapes: the table rows gathered (bf16), the ids read, the row itself, the per-entry outputs
    e = n * (1 + N)
    fwd = e * d * 2 + n * N * 8 + n * d * 2 + e * 4
    bwd = e * d * 2 + n * N * 8 + e * 4 + e * (4 + 8) + n * d * 4
    r["gbce_fwd_bytes"], r["gbce_bwd_bytes"] = fwd, bwd
    r["gbce_fwd_TBps"] = round(fwd / r["gbce_fwd_us"] / 1e6, 3)
    r["gbce_bwd_TBps"] = round(bwd / r["gbce_bwd_us"] / 1e6, 3)
    r["gbce_fwd_over_hbm_peak"] = round(fwd / (r["gbce_fwd_us"] * 1e-6) / HBM_PEAK, 3)
    r["gbce_bwd_over_hbm_peak"] = round(bwd / (r["gbce_bwd_us"] * 1e-6) / HBM_PEAK, 3)
    r["gbce_bytes"] = sum(c[k].numel() * c[k].element_size() for k in ("gbce_ws", "dh", "w", "keys", "iws"))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--configs", default="cfg2,cfg4")
    ap.add_argument("--ns", default="1,16,256")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sas_gbce_bench needs a GPU"
    ns = [int(k) for k in a.ns.split(",")]
    lines = []
    for name in a.configs.split(","):
        cfg = CONFIGS[name]
        rng = np.random.default_rng(0)
        zipf = synth.ZipfItems(cfg["V"])
        batch = [torch.from_numpy(x).cuda() for x in
                 synth.sas_batch(rng, cfg["B"], cfg["T"], cfg["V"], shape=cfg["shape"], zipf=zipf)]
        negs = {N: torch.from_numpy(rng.integers(1, cfg["V"] + 1, (cfg["B"], cfg["T"], N))).cuda() for N in ns}
        r = {"config": name, **{k: cfg[k] for k in ("B", "T", "V", "d", "L", "p")}, "dtype": "bf16", "reps": a.reps,
             "hbm_peak_TBps": HBM_PEAK / 1e12}
        steps = {"bce": FusedTrainStep(model(cfg), lr=1e-3, loss="bce").capture(*batch, warmup=3)}
        for N in ns:
            steps[f"gbce_n{N}"] = FusedTrainStep(gbce_model(cfg, N), lr=1e-3).capture(batch[0], batch[1], negs[N],
                                                                                      warmup=3)
        ms = {k: [] for k in steps}
        for _ in range(a.rounds):                 # interleaved rounds
            for k, t in steps.items():
                ms[k].append(round(replay_us(t.g_compute, a.reps) / 1e3, 4))
        for k, v in ms.items():
            r[f"step_ms_{k}"] = v
        med = {k: statistics.median(v) for k, v in ms.items()}
        for N in ns:
            r[f"gbce_n{N}_over_bce"] = round(med[f"gbce_n{N}"] / med["bce"], 3)
        del steps
        for N in ns:
            r[f"n{N}"] = head_launches(cfg, batch, negs[N], a.reps)
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
