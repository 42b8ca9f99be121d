#!/usr/bin/env python
"""Times BERT4Rec's sampled-softmax head and training step against the plain head kernel and the full-vocabulary
cross-entropy step (GPU only).

    python tools/bert_sce_bench.py [--reps 30] [--rounds 3] [--out profiles/bert_sce_bench.json]
                                   [--configs cfg3,cfg5] [--ks 256,1024,4096,16384] [--parts head,step] [--proposal zipf]

bf16, graph replays (median over --reps replays, each between its own pair of HIP events), --rounds interleaved
rounds, one JSON line per shape (cfg3: V 26,744; cfg5: V 1,000,000; both B 64, T 200, d 256, 4 blocks, 2 heads,
dropout 0.1, labelled-row cap 1,792):
  * head: the head's forward and backward launches alone at d = 256 on cap rows and K candidates -- the MFMA sweep
    through rs_sce_head_fwd / _bwd (without and with the bias) against the plain kernel through rs_sas_sce_fwd / _bwd at
    the same arguments (those entries keep d = 256 on the plain kernel, as the parent commit ran it);
  * step: ms/step of the captured fused step with loss="sampled_ce" at every K and with the default cross-entropy,
    the device time of the sampled step's index launches, and the bytes of the engine's sce_* buffers beside the CE
    step's (cap, V + 1) dlogits.
--proposal zipf adds the popularity leg: the candidates come from an ItemProposal over Zipf(1) weights
(rs_alias_items), "sweep_bias_logq_fwd" / "_bwd" are the head's launches with its logq beside the bias
(rs_sce_head_logq_*), "logq_step_ms_k{K}" the step without and with it captured in turn on one step object
(sas_sce_bench.toggled_step_ms), "alias_items" / "uniform_items" the samplers' launches.
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
from rbm_amd.models import model_factory  # noqa: E402
from rbm_amd.train_step import FusedTrainStep  # noqa: E402
from sas_ce_bench import launch_us, replay_us  # noqa: E402

CONFIGS = {"cfg3": dict(V=26744, T=200, d=256, L=4, h=2, p=0.1, B=64, cap=1792, shape="ml-1m", mask=0.2),
           "cfg5": dict(V=1000000, T=200, d=256, L=4, h=2, p=0.1, B=64, cap=1792, shape="ml-1m", mask=0.2)}
BF = torch.bfloat16


def model(cfg, seed=0):
    torch.manual_seed(seed)
    a = argparse.Namespace(model_code="bert", num_items=cfg["V"], max_len=cfg["T"], device="cuda",
                           bert_hidden_units=cfg["d"], bert_num_blocks=cfg["L"], bert_num_heads=cfg["h"],
                           bert_dropout=cfg["p"], bert_hidden_dropout=cfg["p"], bert_mask_prob=cfg["mask"],
                           model_init_seed=seed, rs_dtype="bf16")
    m = model_factory(a)
    m.train()
    return m


def zipf_proposal(V):
    return ItemProposal(np.concatenate([[0.0], 1.0 / np.arange(1, V + 1)]))


def head_alone(cfg, ks, reps, rounds, prop=None):
    """The head's launches on random rows: cap valid rows of width d against a [V + 1][d] table."""
    V, d, cap = cfg["V"], cfg["d"], cfg["cap"]
    g = torch.Generator(device="cuda").manual_seed(0)
    hl = torch.randn(cap, d, device="cuda", generator=g).to(BF)
    E = (torch.randn(V + 1, d, device="cuda", generator=g) / d ** 0.5).to(BF)
    bias = torch.randn(V + 1, device="cuda", generator=g) * 0.1
    lab = torch.randint(1, V + 1, (cap,), device="cuda", generator=g)
    cnt = torch.tensor([cap], dtype=torch.int32, device="cuda")
    div = torch.tensor([float(cap)], device="cuda")
    out = torch.zeros(4, device="cuda")
    r = {}
    for K in ks:
        cand = torch.randint(1, V + 1, (K,), device="cuda", generator=g)
        sb = torch.ones(1, dtype=torch.int64, device="cuda")
        if prop is not None:
            ops.alias_items(sb, K, prop.table, cand)
        sk = ops.sce_head_dh_splits(cap, K, d, BF)
        ws = torch.zeros(ops.sce_head_ws_numel(cap, K, d, BF, True), device="cuda")
        dh, coef = torch.zeros(sk, cap, d, device="cuda"), torch.zeros(cap, device="cuda")
        src, dbc = torch.zeros(cap + K, d, device="cuda"), torch.zeros(K, device="cuda")
        keys = torch.zeros(cap + K, dtype=torch.int64, device="cuda")
        fns = {
            "plain_fwd": lambda: ops.sas_sce_fwd(hl, lab, cnt, cap, E, cand, div, ws, out),
            "plain_bwd": lambda: ops.sas_sce_bwd(hl, lab, cnt, cap, E, cand, div, None, ws, dh, coef, src[:cap],
                                                 src[cap:], keys),
            "sweep_fwd": lambda: ops.sce_head_fwd(hl, lab, cnt, cap, E, None, cand, div, ws, out),
            "sweep_bwd": lambda: ops.sce_head_bwd(hl, lab, cnt, cap, E, None, cand, div, None, ws, dh, coef, src[:cap],
                                                  src[cap:], None, keys),
            "sweep_bias_fwd": lambda: ops.sce_head_fwd(hl, lab, cnt, cap, E, bias, cand, div, ws, out),
            "sweep_bias_bwd": lambda: ops.sce_head_bwd(hl, lab, cnt, cap, E, bias, cand, div, None, ws, dh, coef,
                                                       src[:cap], src[cap:], dbc, keys),
        }
        if prop is not None:
            q, draws = prop.logq, torch.empty_like(cand)
            fns.update({
                "sweep_bias_logq_fwd": lambda: ops.sce_head_fwd(hl, lab, cnt, cap, E, bias, cand, div, ws, out, logq=q),
                "sweep_bias_logq_bwd": lambda: ops.sce_head_bwd(hl, lab, cnt, cap, E, bias, cand, div, None, ws, dh,
                                                                coef, src[:cap], src[cap:], dbc, keys, logq=q),
                "alias_items": lambda: ops.alias_items(sb, 7, prop.table, draws),
                "uniform_items": lambda: ops.uniform_items(sb, 7, V, draws)})
        us = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                us[k].append(launch_us(fn, reps))
        med = {k: statistics.median(v) for k, v in us.items()}
        r[f"k{K}"] = dict(dh_splits=sk, us=us,
                          sweep_over_plain_fwd=round(med["sweep_fwd"] / med["plain_fwd"], 3),
                          sweep_over_plain_bwd=round(med["sweep_bwd"] / med["plain_bwd"], 3))
    return r


def whole_step(cfg, ks, reps, rounds, prop=None):
    rng = np.random.default_rng(0)
    zipf = synth.ZipfItems(cfg["V"])
    batch = [torch.from_numpy(x).cuda() for x in
             synth.bert_batch(rng, cfg["B"], cfg["T"], cfg["V"], mask_prob=cfg["mask"], shape=cfg["shape"], zipf=zipf)]
    assert int((batch[1] != 0).sum()) <= cfg["cap"]
    cands = {K: torch.from_numpy(rng.integers(1, cfg["V"] + 1, K)).cuda() for K in ks}
    if prop is not None:
        for K in ks:
            ops.alias_items(torch.ones(1, dtype=torch.int64, device="cuda"), K, prop.table, cands[K])
    steps = {"ce": FusedTrainStep(model(cfg), lr=1e-3, max_labelled=cfg["cap"]).capture(*batch, warmup=3)}
    for K in ks:
        steps[f"sampled_ce_k{K}"] = FusedTrainStep(model(cfg), lr=1e-3, max_labelled=cfg["cap"],
                                                   loss="sampled_ce").capture(*batch, cands[K], warmup=3)
    ms = {k: [] for k in steps}
    for _ in range(rounds):                       # interleaved rounds
        for k, t in steps.items():
            ms[k].append(round(replay_us(t.g_compute, reps) / 1e3, 4))
    med = {k: statistics.median(v) for k, v in ms.items()}
    r = {"labelled_rows": int((batch[1] != 0).sum()), "step_ms": ms}
    for K in ks:
        r[f"sampled_k{K}_over_ce"] = round(med[f"sampled_ce_k{K}"] / med["ce"], 3)
    dl = steps["ce"].engine.ws.bufs["dlogits"]
    r["ce_dlogits_bytes"] = dl.numel() * dl.element_size()
    for K in ks:
        t = steps[f"sampled_ce_k{K}"]
        eng, b = t.engine, t.engine.ws.bufs
        cap, d = cfg["cap"], cfg["d"]
        rows = max(eng.V1, 32769)
        GW, Gb = t.flat.view("out.weight", t.flat.grad), t.flat.view("out.bias", t.flat.grad)
        sb = eng.seed_base

        def index():
            ops.item_index_build([b["sce_keys"]], rows, d, b["sce_itemidx"])
            ops.item_grad(b["sce_itemidx"], 1, cap + K, b["sce_src"], 1.0, 0.0, 0, sb, None, None, None, GW,
                          table_rows=rows)
            ops.item_grad(b["sce_itemidx"], 1, cap + K, b["sce_bsrc"].view(-1, 1), 1.0, 0.0, 0, sb, None, None, None,
                          Gb.view(-1, 1), table_rows=rows)
        r[f"k{K}"] = {"sce_index_launches_us": launch_us(index, reps),
                      "sce_bytes": {k: v.numel() * v.element_size() for k, v in b.items() if k.startswith("sce_")}}
        r[f"k{K}"]["sce_bytes_total"] = sum(r[f"k{K}"]["sce_bytes"].values())
        t.flat.grad.zero_()
    # the optimizer alone (the two 1M-row tables dominate it at cfg5): its share of the sampled step
    t = steps[f"sampled_ce_k{ks[0]}"]
    r["adam_us"] = launch_us(lambda: t._update(), reps)
    if prop is not None:
        from sas_sce_bench import toggled_step_ms
        for K in ks:
            r[f"logq_step_ms_k{K}"] = toggled_step_ms(steps[f"sampled_ce_k{K}"], (*batch, cands[K]), prop.logq, reps,
                                                      rounds)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--configs", default="cfg3,cfg5")
    ap.add_argument("--ks", default="256,1024,4096,16384")
    ap.add_argument("--parts", default="head,step")
    ap.add_argument("--proposal", default="", choices=["", "zipf"])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bert_sce_bench needs a GPU"
    ks = [int(k) for k in a.ks.split(",")]
    lines = []
    for name in a.configs.split(","):
        cfg = CONFIGS[name]
        r = {"config": name, **{k: cfg[k] for k in ("B", "T", "V", "d", "L", "cap", "p")}, "dtype": "bf16",
             "reps": a.reps, "rounds": a.rounds, "proposal": a.proposal or "uniform"}
        prop = zipf_proposal(cfg["V"]) if a.proposal else None
        if "head" in a.parts:
            r["head"] = head_alone(cfg, ks, a.reps, a.rounds, prop)
        if "step" in a.parts:
            r["step"] = whole_step(cfg, ks, a.reps, a.rounds, prop)
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
