#!/usr/bin/env python
"""Times SASRec training with the sampled softmax over batch-shared candidates against the full-catalogue
cross-entropy step and the sampled BCE step (GPU only).

    python tools/sas_sce_bench.py [--reps 50] [--rounds 3] [--out profiles/sas_sce_bench.json] [--configs cfg2,cfg4]
                                  [--ks 256,1024,4096] [--proposal zipf]

At the cfg2 head shape (B 128, T 200, V 3,416, d 128) and the cfg4 one (B 128, T 50, V 54,542, d 128, Beauty-shaped
history lengths from rbm_amd.data), bf16, 2 blocks, dropout 0.2, one JSON line per shape:
  * ms/step of the captured fused step (median over --reps graph replays, each between its own pair of HIP events,
    in --rounds interleaved rounds) with loss="sampled_ce" at every K, loss="ce" and loss="bce";
  * device time of the new head's launches alone on that step's own buffers (graph replay of the launches):
    rs_sas_sce_fwd, rs_sas_sce_bwd, and the head's item-gradient launches (rs_item_index_build + rs_item_grad_f32);
  * the bytes of the engine's sce_* buffers beside the bytes of the CE step's (cap, V + 1) ce_dlogits.
--proposal zipf adds the popularity leg: the candidates come from an ItemProposal over Zipf(1) weights
(rs_alias_items), "logq_step_ms_k{K}" (the step without and with its logq, captured in turn on ONE step object each
round: two step objects of a process differ by more than the correction does, see toggled_step_ms) and the head launches "sce_logq_fwd_us" / "sce_logq_bwd_us" carry its
logq (rs_sce_head_logq_*), and "alias_items_us" / "uniform_items_us" time the two samplers' launches at each K.
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
from rbm_amd.dataloaders import ItemProposal  # noqa: E402
from rbm_amd.models.sas_model.heads import SampledCEHead  # noqa: E402
from rbm_amd.train_step import FusedTrainStep  # noqa: E402
from sas_ce_bench import CONFIGS, launch_us, model, replay_us  # noqa: E402


def head_launches(cfg, batch, cand, reps, proposal=None):
    """Device time of the sampled head's launches, on the buffers of one eager forward + backward."""
    m = model(cfg)
    eng = m.sas.engine()
    eng.sync_compute_weights()
    out = torch.zeros(4, device="cuda")
    grad = torch.zeros(eng.flat.numel, device="cuda")
    s = eng.rows_forward(SampledCEHead(), batch[0], batch[1], (cand,), True, out)
    eng.rows_backward(s, grad)
    torch.cuda.synchronize()
    c = s["ce"]
    cap, d, K = c["cap"], eng.d, cand.numel()
    E, GE = eng.W("item_emb.weight"), eng.flat.view("item_emb.weight", grad)
    src, keys, iws, rows = c["src"], c["keys"], c["iws"], c["index_rows"]

    def table():
        ops.item_index_build([keys], rows, d, iws)
        ops.item_grad(iws, 1, cap + K, src, 1.0, 0.0, 0, s["sb"], None, None, None, GE, table_rows=rows)
    r = {"valid_rows": int(c["cnt"].item())}
    r["sce_fwd_us"] = launch_us(lambda: ops.sas_sce_fwd(c["hl"], c["lab"], c["cnt"], cap, E, cand, c["div"],
                                                        c["sce_ws"], out), reps)
    r["sce_bwd_us"] = launch_us(lambda: ops.sas_sce_bwd(c["hl"], c["lab"], c["cnt"], cap, E, cand, c["div"], None,
                                                        c["sce_ws"], c["dh"], c["coef"], src[:cap], src[cap:],
                                                        keys), reps)
    r["sce_table_grad_us"] = launch_us(table, reps)
    if proposal is not None:
        q, sb = proposal.logq, torch.ones(1, dtype=torch.int64, device="cuda")
        r["sce_logq_fwd_us"] = launch_us(lambda: ops.sce_head_fwd(c["hl"], c["lab"], c["cnt"], cap, E, None, cand,
                                                                  c["div"], c["sce_ws"], out, logq=q), reps)
        r["sce_logq_bwd_us"] = launch_us(lambda: ops.sce_head_bwd(c["hl"], c["lab"], c["cnt"], cap, E, None, cand,
                                                                  c["div"], None, c["sce_ws"], c["dh"], c["coef"],
                                                                  src[:cap], src[cap:], None, keys, logq=q), reps)
        draws = torch.empty_like(cand)
        r["alias_items_us"] = launch_us(lambda: ops.alias_items(sb, 7, proposal.table, draws), reps)
        r["uniform_items_us"] = launch_us(lambda: ops.uniform_items(sb, 7, proposal.item_num, draws), reps)
    r["sce_head_us"] = round(r["sce_fwd_us"] + r["sce_bwd_us"] + r["sce_table_grad_us"], 2)
    r["sce_bytes"] = sum(c[k].numel() * c[k].element_size() for k in ("sce_ws", "dh", "coef", "src", "keys", "iws"))
    return r


def toggled_step_ms(t, batch, logq, reps, rounds):
    """ms/step of one FusedTrainStep captured without and with logq in turn, every round: the same model, buffers and
    streams on both sides.  (Two step objects of one process are no such pair: at the 1M-item BERT shape five
    objects built alike measured 3.77 .. 4.45 ms by their place in the process alone.)"""
    ms = {"plain": [], "logq": []}
    for _ in range(rounds):
        for name, q in (("plain", None), ("logq", logq)):
            t.logq = q
            t.capture(*batch, warmup=1)
            ms[name].append(round(replay_us(t.g_compute, reps) / 1e3, 4))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--configs", default="cfg2,cfg4")
    ap.add_argument("--ks", default="256,1024,4096")
    ap.add_argument("--proposal", default="", choices=["", "zipf"])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sas_sce_bench needs a GPU"
    ks = [int(k) for k in a.ks.split(",")]
    lines = []
    for name in a.configs.split(","):
        cfg = CONFIGS[name]
        rng = np.random.default_rng(0)
        zipf = synth.ZipfItems(cfg["V"])
        batch = [torch.from_numpy(x).cuda() for x in
                 synth.sas_batch(rng, cfg["B"], cfg["T"], cfg["V"], shape=cfg["shape"], zipf=zipf)]
        cands = {K: torch.from_numpy(rng.integers(1, cfg["V"] + 1, K)).cuda() for K in ks}
        prop = None
        if a.proposal:
            prop = ItemProposal(np.concatenate([[0.0], 1.0 / np.arange(1, cfg["V"] + 1)]))
            sb = torch.ones(1, dtype=torch.int64, device="cuda")
            for K in ks:
                ops.alias_items(sb, K, prop.table, cands[K])
        r = {"config": name, **{k: cfg[k] for k in ("B", "T", "V", "d", "L", "p")}, "dtype": "bf16", "reps": a.reps,
             "proposal": a.proposal or "uniform"}
        steps = {}
        for loss in ("ce", "bce"):
            steps[loss] = FusedTrainStep(model(cfg), lr=1e-3, loss=loss).capture(*batch, warmup=3)
        for K in ks:
            steps[f"sampled_ce_k{K}"] = FusedTrainStep(model(cfg), lr=1e-3, loss="sampled_ce").capture(
                batch[0], batch[1], cands[K], warmup=3)
        ms = {k: [] for k in steps}
        for _ in range(a.rounds):                 # interleaved rounds
            for k, t in steps.items():
                ms[k].append(round(replay_us(t.g_compute, a.reps) / 1e3, 4))
        for k, v in ms.items():
            r[f"step_ms_{k}"] = v
        med = {k: statistics.median(v) for k, v in ms.items()}
        for K in ks:
            r[f"sampled_k{K}_over_ce"] = round(med[f"sampled_ce_k{K}"] / med["ce"], 3)
            r[f"sampled_k{K}_over_bce"] = round(med[f"sampled_ce_k{K}"] / med["bce"], 3)
        ce_bufs = steps["ce"].engine.ws.bufs
        r["ce_dlogits_bytes"] = ce_bufs["ce_dlogits"].numel() * ce_bufs["ce_dlogits"].element_size()
        if prop is not None:
            for K in ks:
                r[f"logq_step_ms_k{K}"] = toggled_step_ms(steps[f"sampled_ce_k{K}"], (batch[0], batch[1], cands[K]),
                                                          prop.logq, a.reps, a.rounds)
        del steps
        for K in ks:
            r[f"k{K}"] = head_launches(cfg, batch, cands[K], a.reps, prop)
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
