"""bench.py --dump-outputs and the plain (no --full) run.

CPU: dump_outputs writes float32 arrays -- every entry whole within the budget, a fixed sample (the same indices on
every call) of the entries that exceed their share of it.  GPU: a plain run prints the result line with null
roofline / cpu_baseline, and its dump holds the last timed step's loss and every parameter of the model."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import bench


def _state():
    g = torch.Generator().manual_seed(3)
    return {"big.weight": torch.randn(1000, 7, generator=g), "small.bias": torch.randn(5, generator=g),
            "mid.weight": torch.randn(40, 10, generator=g).double()}


def test_dump_outputs_whole(tmp_path):
    st, loss = _state(), torch.tensor([0.5, 0.25])
    bench.dump_outputs(str(tmp_path), loss, st)
    assert sorted(os.listdir(tmp_path)) == ["loss.npy"] + sorted(f"param.{k}.npy" for k in st)
    assert np.array_equal(np.load(tmp_path / "loss.npy"), np.float32([0.5, 0.25]))
    for k, v in st.items():
        a = np.load(tmp_path / f"param.{k}.npy")
        assert a.dtype == np.float32 and a.shape == tuple(v.shape) and np.array_equal(a, v.float().numpy())


def test_dump_outputs_samples_past_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 300)         # 5 whole, then (300 - 5) // 2 = 147 for each of the others
    st = _state()
    bench.dump_outputs(str(tmp_path / "a"), torch.zeros(1), st)
    bench.dump_outputs(str(tmp_path / "b"), torch.zeros(1), {k: v + 1 for k, v in st.items()})
    total = 0
    for k, v in st.items():
        a, b = np.load(tmp_path / "a" / f"param.{k}.npy"), np.load(tmp_path / "b" / f"param.{k}.npy")
        total += a.size
        assert a.dtype == np.float32 and a.shape == b.shape
        np.testing.assert_allclose(b, a + 1, rtol=0, atol=1e-6)          # the same indices in both dumps
        if v.numel() <= 147:
            assert np.array_equal(a, v.float().numpy())                   # within its share: whole
        else:
            assert a.ndim == 1 and 100 <= a.size <= 147
            assert np.isin(a, v.float().numpy().reshape(-1)).all()
    assert total <= 300


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2",
                        "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=300,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 4 and d["ms_per_step"] > 0 and d["unit"] == "sequences/s" and d["dtype"] == "bf16"
    assert abs(d["value"] - d["config"]["per_gpu_batch"] / (d["ms_per_step"] * 1e-3)) < 0.01 * d["value"]
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["config"]["full"] is False
    files = {f: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64e6
    loss = files["loss.npy"]
    assert loss.shape == (d["config"]["steps_per_graph"],) and abs(float(loss[-1]) - d["final_loss"]) < 1e-4
    model = bench.make_model(bench.CONFIGS["cfg2"], "fp32", device="cpu")
    assert {f"param.{k}.npy": tuple(v.shape) for k, v in model.state_dict().items()} == \
        {f: a.shape for f, a in files.items() if f != "loss.npy"}
