#!/usr/bin/env python
"""Times the training step and its optimizer with table_optim="dense" against table_optim="sparse" (GPU only).

    python tools/sparse_adam_bench.py [--reps 30] [--rounds 3] [--out profiles/sparse_adam_bench.json]
                                      [--shapes bert_cfg5,bert_cfg3,sas_cfg4,sas_cfg2] [--ks 256,4096] [--big 0]

bf16, graph replays (median over --reps replays, each between its own pair of HIP events), --rounds interleaved
rounds, one JSON line per shape and K:
  * bert_cfg5 (V 1,000,000) and bert_cfg3 (V 26,744): B 64, T 200, d 256, 4 blocks, loss="sampled_ce" at every K;
  * sas_cfg4 (V 54,542, B 128, T 50, d 128): loss="sampled_ce", K = 256; sas_cfg2 (V 3,416, B 128, T 200, d 128):
    loss="bce", where nearly every row is touched;
  * --big N (optional): a BERT shape with N items beside bert_cfg5, to show the scaling.
Per line: "step_ms" of the dense and the sparse step, "sparse_over_dense" (medians of the same run), "adam_us" -- the
optimizer's launches alone replayed as one graph (dense: FusedAdam.step over the whole buffer; sparse: the dense
ranges and one rs_adam_rows per table on the lists of the last step) --, "adam_share" of the step, "lists_us" (the
rs_unique_rows launches), the touched rows per table, and the bytes of the lists and their flag workspaces.
The two steps are two objects of one process (a step object's place in the process moves its time by a few percent
at the 1M-item shape: tools/sas_sce_bench.py toggled_step_ms), so differences of that size say nothing.
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
from rbm_amd.train_step import FusedTrainStep  # noqa: E402
import bert_sce_bench as bb  # noqa: E402
import sas_ce_bench as sb  # noqa: E402
from sas_ce_bench import launch_us, replay_us  # noqa: E402


def shapes(big):
    out = {"bert_cfg5": ("bert", bb.CONFIGS["cfg5"], "sampled_ce"), "bert_cfg3": ("bert", bb.CONFIGS["cfg3"], "sampled_ce"),
           "sas_cfg4": ("sas", sb.CONFIGS["cfg4"], "sampled_ce"), "sas_cfg2": ("sas", sb.CONFIGS["cfg2"], "bce")}
    if big:
        out[f"bert_{big}"] = ("bert", dict(bb.CONFIGS["cfg5"], V=big), "sampled_ce")
    return out


def make_batch(kind, cfg, loss, K, rng):
    zipf = synth.ZipfItems(cfg["V"])
    if kind == "bert":
        b = list(synth.bert_batch(rng, cfg["B"], cfg["T"], cfg["V"], mask_prob=cfg["mask"], shape=cfg["shape"], zipf=zipf))
    else:
        b = list(synth.sas_batch(rng, cfg["B"], cfg["T"], cfg["V"], shape=cfg["shape"], zipf=zipf))
        if loss == "sampled_ce":
            b = b[:2]
    if loss == "sampled_ce":
        b.append(rng.integers(1, cfg["V"] + 1, K))
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in b]


def sparse_spec(t):
    return [(lo, rows, d, lst, cnt) for (_, tabs), (lst, cnt, _) in zip(t._sparse_tables, t._sparse_bufs)
            for lo, rows, d in tabs]


def optimizer_alone(t):
    """The optimizer's launches of one step (it leaves the gradient zero, so it replays on its own)."""
    if t.table_optim != "sparse":
        return lambda: t._update()
    tr = t.engine.transposed_spec() if hasattr(t.engine, "transposed_spec") else None
    spec = sparse_spec(t)
    return lambda: t.opt.step(seed_base=t.engine.seed_base, transposed=tr, sparse=spec)


def one(kind, cfg, loss, K, reps, rounds):
    rng = np.random.default_rng(0)
    batch = make_batch(kind, cfg, loss, K, rng)
    make = bb.model if kind == "bert" else sb.model
    kw = dict(max_labelled=cfg["cap"]) if kind == "bert" else {}
    steps = {mode: FusedTrainStep(make(cfg), lr=1e-3, loss=loss, table_optim=mode, **kw).capture(*batch, warmup=3)
             for mode in ("dense", "sparse")}
    ms = {k: [] for k in steps}
    for _ in range(rounds):                       # interleaved rounds
        for k, t in steps.items():
            ms[k].append(round(replay_us(t.g_compute, reps) / 1e3, 4))
    med = {k: statistics.median(v) for k, v in ms.items()}
    r = {"step_ms": ms, "sparse_over_dense": round(med["sparse"] / med["dense"], 3), "adam_us": {}, "adam_share": {}}
    for k, t in steps.items():
        us = [launch_us(optimizer_alone(t), reps) for _ in range(rounds)]
        r["adam_us"][k] = us
        r["adam_share"][k] = round(statistics.median(us) / 1e3 / med[k], 3)
    t = steps["sparse"]
    keys = [[t.static[i].reshape(-1) for i in pos] for pos, _ in t._sparse_tables]

    def lists():
        for ks, (_, tabs), (lst, cnt, ws) in zip(keys, t._sparse_tables, t._sparse_bufs):
            ops.unique_rows(ks, tabs[0][1], lst, cnt, ws)
    r["lists_us"] = launch_us(lists, reps)
    torch.cuda.synchronize()
    names = {o: n for n, o in t.flat.offsets.items()}
    r["touched_rows"] = {names[tabs[0][0]]: [int(cnt.item()), tabs[0][1]]
                         for (_, tabs), (lst, cnt, _) in zip(t._sparse_tables, t._sparse_bufs)}
    r["list_bytes"] = sum(lst.numel() * 4 + 4 for lst, _, _ in t._sparse_bufs)
    r["list_workspace_bytes"] = sum(ws.numel() for _, _, ws in t._sparse_bufs)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--shapes", default="bert_cfg5,bert_cfg3,sas_cfg4,sas_cfg2")
    ap.add_argument("--ks", default="256,4096")
    ap.add_argument("--big", type=int, default=0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sparse_adam_bench needs a GPU"
    table = shapes(a.big)
    names = a.shapes.split(",") + ([f"bert_{a.big}"] if a.big else [])
    lines = []
    for name in names:
        kind, cfg, loss = table[name]
        ks = [int(k) for k in a.ks.split(",")] if kind == "bert" else [256 if loss == "sampled_ce" else 0]
        for K in ks:
            r = {"shape": name, "loss": loss, "K": K, **{k: cfg[k] for k in ("B", "T", "V", "d", "L")},
                 "dtype": "bf16", "reps": a.reps, "rounds": a.rounds}
            r.update(one(kind, cfg, loss, K, a.reps, a.rounds))
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
            if a.out:                     # written as it grows: a long run leaves what it finished
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
