#!/usr/bin/env python
"""Times the device evaluation loader (recorded, not gated).

    python tools/eval_bench.py [--out profiles/eval_loader_bench.json] [--reps 20] [--passes 5]     # on the GPU
    python tools/eval_bench.py --reference-cpu [--out ...]                                       # container-only

On the GPU, two things, each after a warm-up, each repeated, median and spread (min, max) reported:
  * "negatives": rs_eval_negatives at an ML-20M-like shape -- 138,493 users, V = 26,744, synthetic histories with the
    ML length distribution of rbm_amd.data (Zipf items), n_neg = 100, both samplers -- the launch alone between a pair
    of events, and the one-off host preparation of DeviceEvalNegatives (sorted unique seen lists, the alias table) by
    the host clock around the constructor (which ends in a host read);
  * "evaluate": a full rbm_amd.metrics.evaluate pass over a DeviceEvalLoader at the cfg2 (SASRec, 6,040 users) and
    cfg3 (BERT4Rec, 20,000 users) model shapes in bf16, against the only route the tree had before: the same batches
    built on the host (the restatement's rule, vectorised in numpy), fed to calculate_metrics one by one and averaged
    on the host.  The two routes alternate, the host clock runs around each pass and every pass ends in a host read.
    Both routes score the same candidates; their results are compared.
--reference-cpu times the reference's own Python samplers (RandomNegativeSampler, PopularNegativeSampler) on the first
2,000 users of the same data on this machine's CPU; it needs the reference tree and never runs on the GPU machine.
Each mode updates its own section of --out and leaves the other in place.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rbm_amd.data as synth  # noqa: E402

USERS, V, T, N_NEG, DATA_SEED = 138_493, 26_744, 200, 100, 20
REF = "/root/reference/NerualNetwork/bert4rec&sas4rec"


def make_data(n_users, num_items, max_len, seed=DATA_SEED):
    """(train, val, test): train as rbm_amd.data.user_histories gives it, one Zipf item each for val and test"""
    rng = np.random.default_rng(seed)
    zipf = synth.ZipfItems(num_items)
    train = synth.user_histories(rng, n_users, max_len, num_items, zipf=zipf)
    val = [[int(x)] for x in zipf.sample(rng, n_users)]
    test = [[int(x)] for x in zipf.sample(rng, n_users)]
    return train, val, test


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def update(path, section, value):
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc[section] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


# ---------------------------------------------------------------- the GPU side
def bench_negatives(reps):
    import torch
    from rbm_amd import ops
    from rbm_amd.dataloaders import DeviceEvalNegatives, ItemProposal
    t0 = time.perf_counter()
    train, val, test = make_data(USERS, V, T)
    out = {"users": USERS, "V": V, "n_neg": N_NEG, "data_seconds": round(time.perf_counter() - t0, 2),
           "interactions": int(sum(len(h) for h in train) + 2 * USERS)}
    for sampler in ("random", "popular"):
        kw, note = {}, "default proposal (smooth = 0)"
        if sampler == "popular":
            try:
                ItemProposal.from_histories(train + val + test, V, alpha=1.0, smooth=0.0, device="cpu")
            except ValueError:
                kw = {"proposal": ItemProposal.from_histories(train + val + test, V, alpha=1.0, smooth=1.0)}
                note = "some item never occurs: proposal with smooth = 1"
        t0 = time.perf_counter()
        neg = DeviceEvalNegatives(train, val, test, V, n_neg=N_NEG, sampler=sampler, seed=1, **kw)
        first = time.perf_counter() - t0
        table = None if neg.proposal is None else neg.proposal.table
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for _ in range(3):
            ops.eval_negatives(neg.seen_offsets, neg.seen_sorted, V, neg.seed, neg.negs, table=table,
                               n_drawn=neg.n_drawn)
        for a, b in ev:
            a.record()
            ops.eval_negatives(neg.seen_offsets, neg.seen_sorted, V, neg.seed, neg.negs, table=table,
                               n_drawn=neg.n_drawn)
            b.record()
        torch.cuda.synchronize()
        drawn = neg.n_drawn.cpu().numpy()
        out[sampler] = {"kernel_ms": spread([round(a.elapsed_time(b), 4) for a, b in ev]),
                        "constructor_seconds_host_prep_and_launch": round(first, 2), "note": note,
                        "fallback_users": neg.fallback_users, "raw_draws_mean": float(drawn[drawn > 0].mean()),
                        "raw_draws_max": int(drawn.max())}
        print(sampler, json.dumps(out[sampler]), flush=True)
    return out


def host_batches(off, flat, extra, answer, negs, batch_size, max_len, mask_token):
    """the loader's batches built on the host: rows_ref's rule (tests/eval_loader_ref.py), vectorised per batch"""
    n = len(off) - 1
    t = np.arange(max_len)
    for u0 in range(0, n, batch_size):
        u = np.arange(u0, min(n, u0 + batch_size))
        L = off[u + 1] - off[u]
        full = L + (extra is not None) + (mask_token > 0)
        j = (full - max_len)[:, None] + t[None, :]                   # position in the extended history
        seq = flat[np.clip(off[u][:, None] + np.minimum(j, (L - 1)[:, None]), 0, len(flat) - 1)]
        if extra is not None:
            seq = np.where(j == L[:, None], extra[u][:, None], seq)
        if mask_token > 0:
            seq = np.where(j == (full - 1)[:, None], mask_token, seq)
        seq = np.where(j < 0, 0, seq)
        cand = np.concatenate([answer[u][:, None], negs[u]], axis=1)
        labels = np.zeros_like(cand)
        labels[:, 0] = 1
        yield seq, cand, labels


def bench_evaluate(passes):
    import torch
    import bench
    from rbm_amd.dataloaders import DeviceEvalLoader, DeviceEvalNegatives
    from rbm_amd.metrics import calculate_metrics, evaluate
    ks, out = [1, 5, 10, 20], {}
    for name, users, bs in (("cfg2", 6040, 128), ("cfg3", 20000, 128)):
        cfg = bench.CONFIGS[name]
        code = cfg["model"]
        m = bench.make_model(cfg, "bf16")
        m.eval()
        train, val, test = make_data(users, cfg["V"], cfg["T"], seed=DATA_SEED + 1)
        neg = DeviceEvalNegatives(train, val, test, cfg["V"], n_neg=N_NEG, seed=1)
        loader = DeviceEvalLoader(train, val, test, cfg["V"], bs, cfg["T"], neg, mode="test", model_code=code)
        off, flat = loader.offsets.cpu().numpy(), loader.items.cpu().numpy()
        extra, answer = loader.extra.cpu().numpy(), loader.answer.cpu().numpy()
        negs = neg.negs.cpu().numpy().astype(np.int64)

        def device_pass():
            return evaluate(m, loader, ks)

        def host_pass():
            ms = [calculate_metrics(m, b, ks)
                  for b in host_batches(off, flat, extra, answer, negs, bs, cfg["T"], loader.mask_token)]
            return {k: float(np.mean([x[k] for x in ms])) for k in ms[0]}

        got, want = device_pass(), host_pass()                       # warm-up of both, and the comparison
        first = next(iter(loader))
        hb = next(host_batches(off, flat, extra, answer, negs, bs, cfg["T"], loader.mask_token))
        same_batches = all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(first, hb))
        td, th = [], []
        for _ in range(passes):
            for fn, acc in ((host_pass, th), (device_pass, td)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                acc.append(round((time.perf_counter() - t0) * 1e3, 3))
        out[name] = {"model": code, "users": users, "batch_size": bs, "batches": len(loader), "T": cfg["T"],
                     "V": cfg["V"], "d": cfg["d"], "n_neg": N_NEG, "dtype": "bf16", "mode": "test",
                     "device_loader_evaluate_ms": spread(td), "host_batches_calculate_metrics_ms": spread(th),
                     "speedup_of_medians": round(statistics.median(th) / statistics.median(td), 2),
                     "first_batch_identical": bool(same_batches),
                     "max_abs_metric_difference": max(abs(got[k] - want[k]) for k in want)}
        print(name, json.dumps(out[name]), flush=True)
        del m
    return out


# ---------------------------------------------------------------- the reference's samplers on the CPU
def bench_reference_cpu(n_users=2000):
    if not os.path.isdir(REF):
        raise SystemExit("eval_bench --reference-cpu: the reference tree is absent (container-only)")
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    from dataloaders.negative_samplers import PopularNegativeSampler, RandomNegativeSampler  # (reference)
    train, val, test = make_data(USERS, V, T)
    train, val, test = train[:n_users], val[:n_users], test[:n_users]
    out = {"users": n_users, "of_users": USERS, "V": V, "n_neg": N_NEG, "cpu": "this container's CPU, one process"}
    for name, cls in (("random", RandomNegativeSampler), ("popular", PopularNegativeSampler)):
        s = cls(train, val, test, n_users, V, N_NEG, 0, ".", "bench")
        np.random.seed(0)
        t0 = time.perf_counter()
        res = s.generate_negative_samples()
        dt = time.perf_counter() - t0
        assert len(res) == n_users and all(len(v) == N_NEG for v in res.values())
        out[name] = {"seconds": round(dt, 2), "ms_per_user": round(dt / n_users * 1e3, 3),
                     "extrapolated_seconds_all_users": round(dt / n_users * USERS, 1),
                     "note": "the last figure is an extrapolation (linear in the user count), not a measurement"}
        print(name, json.dumps(out[name]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_loader_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--reference-cpu", action="store_true")
    a = ap.parse_args()
    if a.reference_cpu:
        update(a.out, "reference_cpu", bench_reference_cpu())
        return
    import torch
    assert torch.cuda.is_available(), "eval_bench needs a GPU (no timing is taken on the CPU)"
    update(a.out, "gpu", {"device": torch.cuda.get_device_name(0), "negatives": bench_negatives(a.reps),
                          "evaluate": bench_evaluate(a.passes)})


if __name__ == "__main__":
    main()
