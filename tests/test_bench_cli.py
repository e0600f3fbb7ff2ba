"""bench.py's plain run and --dump-outputs: the plain line carries the headline fields and nothing that --full measures,
--steps sets the timed steps, and the dumped outputs of the last timed step are float32 arrays that the HIP-graph replay and
the eager issue of the same step agree on."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_dump_outputs_writes_float32_and_keeps_within_the_cap(tmp_path):
    bench = _bench_module()
    torch.manual_seed(0)
    m = torch.nn.Linear(300, 200)
    m(torch.randn(4, 300)).sum().backward()
    res = (torch.tensor(0.25), None, torch.randn(100, dtype=torch.float64))
    bench.dump_outputs(str(tmp_path / "all"), res, m.named_parameters())
    files = sorted(os.listdir(tmp_path / "all"))
    assert files == ["grad.bias.npy", "grad.weight.npy", "loss.npy", "q.npy"]
    w = np.load(tmp_path / "all" / "grad.weight.npy")
    assert w.dtype == np.float32 and np.array_equal(w, m.weight.grad.numpy())
    assert np.load(tmp_path / "all" / "q.npy").dtype == np.float32
    # above the cap: the same seeded sample every time, a subset of the full array, within the byte budget
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), res, m.named_parameters(), cap_bytes=20000)
    total = 0
    for f in files:
        a, b = np.load(tmp_path / "s1" / f), np.load(tmp_path / "s2" / f)
        assert np.array_equal(a, b)
        total += a.nbytes
    assert total <= 20000
    assert np.isin(np.load(tmp_path / "s1" / "grad.weight.npy"), w.reshape(-1)).all()


def _run(args, timeout=540):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_run_dumps_the_last_step(tmp_path):
    out = _run(["--gpus", "1", "--steps", "7", "--warmup", "2", "--preheat-ms", "20",
                "--dump-outputs", str(tmp_path / "graph")])
    assert out["steps"] == 7 and out["metric"] == "board-graphs/sec fwd+bwd" and out["unit"] == "graphs/s"
    assert out["higher_is_better"] is True and out["dtype"] == "f32"
    assert abs(out["value"] - 256 / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
    for k in ("sustained", "roofline", "cpu_baseline", "split_precision_mode", "other_configs"):
        assert out[k] is None, k
    eager = _run(["--gpus", "1", "--steps", "7", "--warmup", "2", "--preheat-ms", "20", "--eager",
                  "--dump-outputs", str(tmp_path / "eager")])
    assert eager["steps"] == 7
    files = sorted(os.listdir(tmp_path / "graph"))
    assert files == sorted(os.listdir(tmp_path / "eager"))
    assert {"loss.npy", "td.npy", "q.npy"} <= set(files) and sum(f.startswith("grad.") for f in files) > 10
    for f in files:
        a, b = np.load(tmp_path / "graph" / f), np.load(tmp_path / "eager" / f)
        assert a.dtype == np.float32 and np.isfinite(a).all(), f
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-5, f
    assert np.abs(np.load(tmp_path / "graph" / "q.npy")).max() > 0
