"""CPU suite: what ``bench.py --dump-outputs DIR`` writes (dtypes, names, the size limit, the fixed samples) and the argument
checks of the options a plain run and a ``--full`` run share."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_fixed_sample_is_the_same_every_time():
    a, b = bench.fixed_sample(10_000_000, 1 << 16), bench.fixed_sample(10_000_000, 1 << 16)
    assert torch.equal(a, b)
    assert a.numel() > (1 << 16) * 0.99 and bool((a[1:] > a[:-1]).all()) and int(a[-1]) < 10_000_000
    assert torch.equal(bench.fixed_sample(100, 1 << 16), torch.arange(100))


def test_write_outputs_dtypes_and_values(tmp_path):
    w = torch.randn(3, 50, generator=torch.Generator().manual_seed(0)).bfloat16()
    bench.write_outputs(str(tmp_path), {"w": w, "ids": torch.tensor([1, 5, 2**40], dtype=torch.int64),
                                        "x64": torch.tensor([0.1], dtype=torch.float64), "loss": 2.5})
    got = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert sorted(got) == ["ids", "loss", "w", "x64"]
    assert got["w"].dtype == np.float32 and np.array_equal(got["w"], w.float().numpy())      # bf16 is exact in float32
    assert got["ids"].dtype == np.float64 and got["ids"].tolist() == [1, 5, 2**40]
    assert got["x64"].dtype == np.float64 and got["x64"][0] == 0.1
    assert got["loss"].dtype == np.float32 and got["loss"] == 2.5


def test_write_outputs_refuses_more_than_the_limit(tmp_path):
    with pytest.raises(SystemExit):
        bench.write_outputs(str(tmp_path / "d"), {"big": torch.zeros(bench.DUMP_LIMIT // 4 + 1)})
    assert not os.path.exists(tmp_path / "d")                    # nothing written


def test_model_outputs_names():
    class Sampler:
        exp3_weights = torch.ones(3, 1000, dtype=torch.bfloat16)

    model = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.Linear(3, 2))
    sizes = [dict(S=7, E=9, C=3, K=11, B=20), dict(S=2, E=4, C=1, K=7, B=5)]
    arr = bench.model_outputs(model, torch.tensor(0.75), sizes, Sampler())
    assert set(arr) == {"loss", "param.0.weight", "param.0.bias", "param.1.weight", "param.1.bias", "block_sizes",
                        "exp3_weights_sample", "exp3_sample_edge_ids"}
    assert arr["block_sizes"].tolist() == [[7, 9, 3, 11, 20], [2, 4, 1, 7, 5]]
    assert arr["exp3_weights_sample"].shape == (3, 1000) and torch.equal(arr["exp3_sample_edge_ids"], torch.arange(1000))
    assert set(bench.model_outputs(model, 1.0)) == {"loss", "param.0.weight", "param.0.bias", "param.1.weight", "param.1.bias"}


def _run(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=env, capture_output=True, text=True,
                          timeout=120)


def test_new_options_parse_and_steps_must_be_positive(tmp_path):
    r = _run("--dry-run", "--full", "--dump-outputs", str(tmp_path), "--steps", "5", "--warmup", "0")
    assert r.returncode == 0, r.stderr[-2000:]
    r = _run("--dry-run", "--steps", "0")
    assert r.returncode != 0 and "--steps" in r.stderr
