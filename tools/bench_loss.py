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

  (3) --mode metrics: a test-set scoring pass (reset, one ForecastMetrics.update per batch over
      --batches (64) batches of head outputs already on the device, compute()) on the three shapes,
      for the unmasked object (metrics_accum_kernel, the baseline), the masked one
      (metrics_masked_kernel, NaN marker on 30 % of the targets) and the masked one with the node
      table: windows of --passes (300) passes on the host clock (a pass ends in compute()'s
      synchronising copy), --rounds windows of each variant, alternating; median and spread.

    python tools/bench_loss.py --mode metrics --out profiles/metrics_masked_ab.json

  (4) --mode quantile: the pinball criterion (forward + backward, timed as (1)) and one calibration
      update (QuantileMetrics.update against the same sums written as torch tensor expressions,
      --iters updates between two device events) at the head shapes (B, N, P, Q) of PEMS08
      (32, 170, 12, 3) and GAMBIA (4, 2139, 12, 3), NaN marker on 30 % of the targets.  The torch
      side is what a user writes today: tensor expressions on the GPU, no host copy.  Also the full
      training step of the PEMS08-shaped model (nb_block=4, B=32), point head against quantile head.

    python tools/bench_loss.py --mode quantile --out profiles/quantile_ab.json

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


def time_metrics(torch, dev, shape, batches, passes, rounds):
    from dstagnn_drought_amd import ForecastMetrics
    B, N, P = shape
    gen = torch.Generator(device=dev).manual_seed(7)
    data = []
    for _ in range(batches):
        t = 3.0 * torch.randn(shape, device=dev, generator=gen)
        y = t + torch.randn(shape, device=dev, generator=gen)
        t[torch.rand(shape, device=dev, generator=gen) < 0.3] = float("nan")
        data.append((y, t))
    objs = {"unmasked": ForecastMetrics(P, 0.0, dev),
            "masked": ForecastMetrics(P, 0.0, dev, missing_value=float("nan")),
            "masked_nodes": ForecastMetrics(P, 0.0, dev, missing_value=float("nan"), num_nodes=N)}

    def one_pass(m):
        m.reset()
        for y, t in data:
            m.update(y, t)
        return m.compute()

    for m in objs.values():
        for _ in range(3):
            one_pass(m)
    torch.cuda.synchronize()
    runs = {k: [] for k in objs}
    for _ in range(rounds):
        for k, m in objs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(passes):
                one_pass(m)
            runs[k].append(round((time.perf_counter() - t0) / passes * 1e3, 4))
    med = {k: statistics.median(r) for k, r in runs.items()}
    return {"shape": list(shape), "batches": batches, "passes_per_window": passes, "ms_per_pass_runs": runs,
            "median_ms": med, "us_per_update": {k: round(v / batches * 1e3, 3) for k, v in med.items()},
            "over_unmasked": {k: round(med[k] / med["unmasked"], 4) for k in ("masked", "masked_nodes")},
            "spread": {k: round((max(r) - min(r)) / med[k], 4) for k, r in runs.items()}}


QUANTILES = (0.1, 0.5, 0.9)


def _windows(torch, variants, iters, rounds):
    """--rounds alternating windows of --iters calls between two device events: us per call."""
    runs = {k: [] for k in variants}
    for _ in range(rounds):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            e1.synchronize()
            runs[k].append(round(e0.elapsed_time(e1) / iters * 1e3, 3))
    med = {k: statistics.median(r) for k, r in runs.items()}
    return runs, med, {k: round((max(r) - min(r)) / med[k], 4) for k, r in runs.items()}


def time_quantile(torch, dev, shape, iters, rounds, warmup):
    from dstagnn_drought_amd import QuantileLoss, QuantileMetrics
    B, N, P = shape
    Q = len(QUANTILES)
    gen = torch.Generator(device=dev).manual_seed(11)
    t = 3.0 * torch.randn(shape, device=dev, generator=gen)
    y = (t[..., None] + torch.randn(B, N, P, Q, device=dev, generator=gen)
         + torch.linspace(-1.0, 1.0, Q, device=dev)).requires_grad_(True)
    t[torch.rand(shape, device=dev, generator=gen) < 0.3] = float("nan")
    tau = torch.tensor(QUANTILES, dtype=torch.float32, device=dev)
    omt = 1.0 - tau
    hip = QuantileLoss(QUANTILES, null_val=float("nan"))

    def torch_loss(y, t):  # the masked pinball mean as tensor expressions (no boolean indexing: no sync)
        valid = ~torch.isnan(t)
        d = y - torch.where(valid, t, torch.zeros_like(t))[..., None]
        term = torch.where(d > 0, omt * d, tau * -d)
        return torch.where(valid[..., None], term, torch.zeros_like(term)).sum() / (valid.sum() * Q).clamp(min=1)

    def step(c):
        y.grad = None
        c(y, t).backward()

    for c in (torch_loss, hip):
        for _ in range(warmup):
            step(c)
    torch.cuda.synchronize()
    runs, med, spread = _windows(torch, {"torch": lambda: step(torch_loss), "hip": lambda: step(hip)}, iters, rounds)
    with torch.no_grad():
        agree = abs(float(torch_loss(y, t)) - float(hip(y, t)))
    out = {"shape": [B, N, P, Q], "fwd_bwd": {"us_per_fwd_bwd_runs": runs, "median_us": med, "spread": spread,
                                              "hip_over_torch": round(med["hip"] / med["torch"], 4),
                                              "abs_loss_difference": agree}}

    # one calibration update: the (P, 2 + 3 Q) and (N, 2 + 3 Q) running tables
    yd = y.detach()
    qm = QuantileMetrics(P, QUANTILES, missing_value=float("nan"), num_nodes=N, device=dev)
    ht = torch.zeros(P, 2 + 3 * Q, dtype=torch.float64, device=dev)
    nt = torch.zeros(N, 2 + 3 * Q, dtype=torch.float64, device=dev)

    def torch_update():
        valid = ~torch.isnan(t)
        tz = torch.where(valid, t, torch.zeros_like(t))
        d = yd - tz[..., None]
        v3 = valid[..., None]
        term = torch.where(v3 & (d != 0), torch.where(d > 0, omt * d, tau * -d), torch.zeros_like(d)).double()
        hit = (v3 & (tz[..., None] <= yd)).double()
        sy = torch.where(v3, yd, torch.zeros_like(yd)).double()
        cross = (valid & (yd[..., 1:] < yd[..., :-1]).any(-1)).double()
        cols = torch.cat([valid.double()[..., None], cross[..., None],
                          torch.stack([term, hit, sy], -1).reshape(B, N, P, 3 * Q)], -1)
        ht.add_(cols.sum((0, 1)))
        nt.add_(cols.sum((0, 2)))

    for _ in range(max(warmup // 10, 10)):
        torch_update()
        qm.update(yd, t)
    torch.cuda.synchronize()
    qm.reset(), ht.zero_(), nt.zero_()
    torch_update()
    qm.update(yd, t)
    diff = float((qm.table - ht).abs().max() / ht.abs().max())
    runs, med, spread = _windows(torch, {"torch": torch_update, "hip": lambda: qm.update(yd, t)}, iters, rounds)
    out["metrics_update"] = {"us_per_update_runs": runs, "median_us": med, "spread": spread,
                             "hip_over_torch": round(med["hip"] / med["torch"], 4),
                             "worst_table_difference_relative_to_its_largest_entry": diff}
    return out


def time_model_step(torch, dev, rounds, steps=40, warmup=10):
    """The full training step (forward, criterion, backward, HipAdam) of the PEMS08-shaped model
    (make_model nb_block=4, B=32): the point model with the driver's default nn.SmoothL1Loss
    against the quantile model (final_fc 12 -> 36 columns) with QuantileLoss."""
    import bench
    import dstagnn_drought_amd as D
    from dstagnn_drought_amd import train as TR
    c = bench.CFG
    B, N, T, K, h, Dm, dk, C = c["B"], c["N"], c["T"], c["K"], c["n_heads"], c["d_model"], c["d_k"], c["C"]
    tmd, pa = bench.synth_graph(N)
    gen = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(B, N, 1, T, device=dev, generator=gen)
    t = torch.randn(B, N, T, device=dev, generator=gen)
    variants = {}
    for name, q in (("point", None), ("quantile", QUANTILES)):
        torch.manual_seed(1)
        net = D.set_direct_grads(D.make_model(dev, 1, 4, 1, K, C, C, 1, tmd, pa, tmd, T, T, N, Dm, dk, dk, h,
                                              quantiles=q).train())
        crit = torch.nn.SmoothL1Loss().to(dev) if q is None else D.QuantileLoss(q)
        opt = TR.make_adam(net.parameters(), 1e-3)

        def step(net=net, crit=crit, opt=opt):
            opt.zero_grad()
            crit(net(x), t).backward()
            opt.step()
        variants[name] = step
    for f in variants.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    runs, med, spread = _windows(torch, variants, steps, rounds)
    return {"model": "make_model nb_block=4, PEMS08 shape, B=32, train mode, HipAdam", "steps_per_window": steps,
            "us_per_step_runs": runs, "median_us": med, "spread": spread,
            "quantile_over_point": round(med["quantile"] / med["point"], 4)}


def main_quantile(a):
    import torch
    from dstagnn_drought_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss.py measures on the GPU only: no HIP device")
    dev = torch.device("cuda:0")
    rec = {"what": f"pinball criterion forward + backward and one calibration update at Q = {len(QUANTILES)}, NaN marker "
                   f"on 30 % of the targets, us per call between device events, {a.rounds} alternating windows x "
                   f"{a.iters} calls (tools/bench_loss.py --mode quantile)",
           "variants": {"torch": "the same quantities as torch tensor expressions on the GPU",
                        "hip": "QuantileLoss (pinball_fwd_kernel + pinball_bwd_kernel) / QuantileMetrics.update with the "
                               "node table (metrics_quantile_kernel)"},
           "quantiles": list(QUANTILES), "stamp": _lib.build_stamp(),
           "quantile": {name: time_quantile(torch, dev, SHAPES[name], a.iters, a.rounds, a.warmup)
                        for name in ("PEMS08", "GAMBIA")},
           "model_step": time_model_step(torch, dev, a.rounds)}
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


def main_metrics(a):
    import torch
    from dstagnn_drought_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss.py measures on the GPU only: no HIP device")
    dev = torch.device("cuda:0")
    rec = {"what": f"test-set scoring pass over {a.batches} batches of head outputs on the device (reset, one update "
                   f"per batch, compute()), ms per pass on the host clock, {a.rounds} alternating windows x "
                   f"{a.passes} passes (tools/bench_loss.py --mode metrics)",
           "variants": {"unmasked": "ForecastMetrics(P) (metrics_accum_kernel)",
                        "masked": "ForecastMetrics(P, missing_value=nan) (metrics_masked_kernel)",
                        "masked_nodes": "ForecastMetrics(P, missing_value=nan, num_nodes=N)"},
           "stamp": _lib.build_stamp(),
           "metrics": {name: time_metrics(torch, dev, shape, a.batches, a.passes, a.rounds)
                       for name, shape in SHAPES.items()}}
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("loss", "metrics", "quantile"), default="loss",
                    help="loss: (1) and (2) above; metrics: (3), the masked scoring pass; quantile: (4), the pinball "
                         "criterion and one calibration update")
    ap.add_argument("--passes", type=int, default=300, help="--mode metrics: passes per window")
    ap.add_argument("--iters", type=int, default=2000, help="iterations per window (>= 200)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--out", default=None,
                    help="default: profiles/loss_ab.json (profiles/metrics_masked_ab.json with --mode metrics, "
                         "profiles/quantile_ab.json with --mode quantile)")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", {"metrics": "metrics_masked_ab.json",
                                                "quantile": "quantile_ab.json"}.get(a.mode, "loss_ab.json"))
    if a.mode == "quantile":
        if a.iters < 200:
            ap.error("--iters must be at least 200")
        return main_quantile(a)
    if a.mode == "metrics":
        if a.passes < 1 or a.rounds < 3:
            ap.error("--mode metrics needs --passes >= 1 and --rounds >= 3")
        return main_metrics(a)
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
