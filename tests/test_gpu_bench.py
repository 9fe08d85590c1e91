"""bench.py as it is run for every change: a plain run (no --full) takes its steps and prints the headline line only,
and --dump-outputs writes what the last timed step computed, the same from run to run up to rounding."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--n-tx", "20000", "--n-bd", "200", "--dump-outputs", str(out_dir)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {p: np.load(os.path.join(out_dir, p)) for p in os.listdir(out_dir)}


def test_plain_bench_run_is_the_headline_alone_and_dumps_its_last_step(cuda, tmp_path):
    line, out = _plain_run(tmp_path / "a")
    assert line["metric"] == "edges scored/sec (tx->cell) fwd+bwd" and line["unit"] == "edges/s"
    assert line["higher_is_better"] is True and line["dtype"] == "bf16" and line["steps"] == 2 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and line["value"] > 0
    for k in ("roofline", "cpu_baseline", "auroc", "untimed_setup", "predict", "f32", "strong"):
        assert not line.get(k), (k, line.get(k))             # secondary records are --full only
    from segger_amd import LitISTEncoder
    m = LitISTEncoder(n_genes=256, in_channels=128)
    m.model._materialize_bd(128, "cpu")                        # as bench.py does (SyntheticSpec.bd_dim)
    names = [n for n, _ in m.named_parameters()]
    assert set(out) == {"loss.npy"} | {"param." + re.sub(r"[^A-Za-z0-9_.-]", "_", n) + ".npy" for n in names}
    assert sum(a.nbytes for a in out.values()) <= 64 * 2 ** 20
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in out.values())
    assert float(out["loss.npy"]) == pytest.approx(line["loss"], rel=1e-5)
    # same arguments -> same outputs: every step starts from the seed-0 weights, so the forward (atomic-free) repeats the
    # loss, and the weights differ only by the rounding the loss-head backward's fp32 atomics leave, through Adam
    # (C2, 25 steps: up to 3e-4 of a file's largest entry)
    line2, out2 = _plain_run(tmp_path / "b")
    assert line2["loss"] == line["loss"]
    assert float(out2["loss.npy"]) == pytest.approx(float(out["loss.npy"]), rel=1e-6)
    for f, a in out.items():
        d = np.abs(a.astype(np.float64) - out2[f]).max()
        assert d <= 1e-3 * np.abs(a).max() + 1e-9, (f, d)
