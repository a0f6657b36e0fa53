"""bench.py as every later change runs it: a plain `--gpus 1 --steps N --warmup W` run times
exactly N steps and prints the headline only; `--dump-outputs DIR` writes what the last timed
step returned.  One short run (3 steps) in a fresh process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "dominant_kernel", "hot_kernel", "hbm_roofline", "cpu_baseline", "variant_bf16_gemm",
             "extras")


@pytest.mark.gpu
def test_plain_run_headline_and_dump(tmp_path):
    import bench
    c = bench.CFG
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "dump")], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["n_gpus"] == 1 and rec["full"] is False
    assert "timed 3 steps" in r.stderr
    assert rec["unit"] == "samples/s" and rec["higher_is_better"] is True and rec["dtype"] == "fp32"
    assert rec["metric"].startswith("DSTAGNN_block fwd+bwd samples/sec")
    assert rec["ms_per_step"] > 0
    # value and ms_per_step are the same measurement (each rounded on its own)
    assert rec["value"] == pytest.approx(c["B"] / (rec["ms_per_step"] * 1e-3), rel=1e-3)
    assert not [k for k in FULL_ONLY if k in rec], rec.keys()

    files = sorted(os.listdir(tmp_path / "dump"))
    arrs = {f[:-4]: np.load(tmp_path / "dump" / f) for f in files}
    assert all(f.endswith(".npy") for f in files)
    assert sum(os.path.getsize(tmp_path / "dump" / f) for f in files) <= 64 << 20
    assert arrs["out"].shape == (c["B"], c["N"], c["C"], c["T"])
    assert arrs["re_at"].shape == (c["B"], c["C"], c["n_heads"], c["T"], c["T"])
    with torch.random.fork_rng(devices=[]):  # build_block seeds the global RNG
        shapes = {"grad." + n: tuple(p.shape) for n, p in bench.build_block("cpu")[0].named_parameters()}
    grads = {k: a.shape for k, a in arrs.items() if k.startswith("grad.")}
    assert grads and set(arrs) == {"out", "re_at"} | set(grads), files
    assert all(shapes.get(k) == s for k, s in grads.items()), grads  # parameter gradients, whole
    for k, a in arrs.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), k
    assert np.abs(arrs["out"]).max() > 0 and np.abs(arrs["re_at"]).max() > 0
