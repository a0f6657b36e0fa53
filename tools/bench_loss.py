#!/usr/bin/env python
"""What the on-device criterion and test-set scoring cost, A/B in one process:

  (1) forward + backward of nn.SmoothL1Loss against HipLoss('smooth_l1') on the head shapes
      (B, N, P) of PEMS08 (32, 170, 12), GAMBIA (4, 2139, 12) and SYN (32, 4096, 12): after a
      warm-up, windows of --iters (2000; at least 200) iterations between two device events,
      --rounds (3) windows of each variant, alternating, so a difference can be held against the
      spread.  At these sizes an iteration is a handful of launches: the figure is the host's
      issue rate as much as the kernels' time;
  (2) evaluate_on_test_mstgcn (scores accumulated on the device, one table copied back) against
      the host-copy path of predict_and_save_results_mstgcn (every prediction copied to the host,
      sklearn) with its file write taken out, over 64 batches of a PEMS08-shaped model
      (make_model nb_block=4, B=32): host clock around work that ends in a device synchronise.

    python tools/bench_loss.py --out profiles/loss_ab.json

The JSON carries the library stamp (dstagnn_drought_amd._lib.build_stamp).  There is no fallback:
without a HIP device the tool fails."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"PEMS08": (32, 170, 12), "GAMBIA": (4, 2139, 12), "SYN": (32, 4096, 12)}


def time_losses(torch, dev, shape, iters, rounds, warmup):
    from dstagnn_drought_amd import HipLoss
    gen = torch.Generator(device=dev).manual_seed(3)
    t = 3.0 * torch.randn(shape, device=dev, generator=gen)
    y = (t + torch.randn(shape, device=dev, generator=gen)).requires_grad_(True)
    crits = {"torch": torch.nn.SmoothL1Loss().to(dev), "hip": HipLoss("smooth_l1")}

    def step(c):
        y.grad = None
        c(y, t).backward()

    for c in crits.values():
        for _ in range(warmup):
            step(c)
    torch.cuda.synchronize()
    runs = {k: [] for k in crits}
    for _ in range(rounds):
        for k, c in crits.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                step(c)
            e1.record()
            e1.synchronize()
            runs[k].append(round(e0.elapsed_time(e1) / iters * 1e3, 3))
    med = {k: statistics.median(r) for k, r in runs.items()}
    with torch.no_grad():
        agree = abs(float(crits["torch"](y, t)) - float(crits["hip"](y, t)))
    return {"shape": list(shape), "us_per_fwd_bwd_runs": runs, "median_us": med,
            "hip_over_torch": round(med["hip"] / med["torch"], 4),
            "spread": {k: round((max(r) - min(r)) / med[k], 4) for k, r in runs.items()},
            "abs_loss_difference": agree}


def time_scoring(torch, dev, batches, rounds):
    import numpy as np
    import bench
    import dstagnn_drought_amd as D
    from dstagnn_drought_amd import train as TR
    c = bench.CFG
    B, N, T, K, h, Dm, dk, C = c["B"], c["N"], c["T"], c["K"], c["n_heads"], c["d_model"], c["d_k"], c["C"]
    tmd, pa = bench.synth_graph(N)
    torch.manual_seed(1)
    net = D.make_model(dev, 1, 4, 1, K, C, C, 1, tmd, pa, tmd, T, T, N, Dm, dk, dk, h).eval()
    gen = torch.Generator(device=dev).manual_seed(5)
    loader = [(torch.randn(B, N, 1, T, device=dev, generator=gen), torch.randn(B, N, T, device=dev, generator=gen))
              for _ in range(batches)]
    target = torch.cat([yb for _, yb in loader], 0)
    mean, std = np.zeros((1, 1, 1, 1), np.float32), np.ones((1, 1, 1, 1), np.float32)
    savez = TR.np.savez

    def device_path():
        with contextlib.redirect_stdout(io.StringIO()):
            return TR.evaluate_on_test_mstgcn(net, loader, target, None, 0, mean, std)

    def host_path():  # the real function, its np.savez call made a no-op
        TR.np.savez = lambda *a, **k: None
        try:
            return TR.predict_and_save_results_mstgcn(net, loader, target, 0, mean, std, ".", "test")
        finally:
            TR.np.savez = savez

    variants = {"device": device_path, "host": host_path}
    lists = {k: f() for k, f in variants.items()}  # warm-up, and the two lists for comparison
    torch.cuda.synchronize()
    runs = {k: [] for k in variants}
    for _ in range(rounds):
        for k, f in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            runs[k].append(round((time.perf_counter() - t0) * 1e3, 3))
    med = {k: statistics.median(r) for k, r in runs.items()}
    worst = max(abs(a - b) / max(abs(b), 1e-30) for a, b in zip(lists["device"], lists["host"]))
    return {"model": "make_model nb_block=4, PEMS08 shape", "batches": batches, "batch_size": B,
            "ms_per_pass_runs": runs, "median_ms": med, "device_over_host": round(med["device"] / med["host"], 4),
            "spread": {k: round((max(r) - min(r)) / med[k], 4) for k, r in runs.items()},
            "worst_relative_difference_of_the_lists": worst}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000, help="iterations per window (>= 200)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_ab.json"))
    a = ap.parse_args()
    if a.iters < 200:
        ap.error("--iters must be at least 200")
    import torch
    from dstagnn_drought_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss.py measures on the GPU only: no HIP device")
    dev = torch.device("cuda:0")
    rec = {"what": "criterion forward + backward, us per iteration between device events, "
                   f"{a.rounds} alternating windows x {a.iters} iterations; test-set scoring, ms per pass over "
                   f"{a.batches} batches (tools/bench_loss.py)",
           "variants": {"torch": "nn.SmoothL1Loss", "hip": "HipLoss('smooth_l1')",
                        "device": "evaluate_on_test_mstgcn (ForecastMetrics)",
                        "host": "predict_and_save_results_mstgcn without its np.savez"},
           "stamp": _lib.build_stamp(),
           "loss": {name: time_losses(torch, dev, shape, a.iters, a.rounds, a.warmup)
                    for name, shape in SHAPES.items()},
           "scoring": time_scoring(torch, dev, a.batches, a.rounds)}
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
