#!/usr/bin/env python
"""What feeding a batch from the raw series costs against cutting it from materialised tensors,
A/B in one process, at the two geometries the issue is about:

  PEMS08  series (17856, 170, 1) fp32, one hour-window of 12, B = 32   (x[b]: 8 KB)
  GAMBIA  series (4000, 2139, 4) fp32, twelve hour-windows of 12 (Tin = 144), B = 4   (x[b]: 4.9 MB)

  gather        WindowedSeries.batch(): ONE dstagnn::window_gather launch -> (x, y)
  index_select  the parent path: x.index_select(0, idx), y.index_select(0, idx) from tensors that
                hold the same samples materialised (built here by the gather itself, and compared
                with it bit for bit)

Both walk the same shuffled index tensor batch by batch.  After a warm-up, windows of --iters
batches between two device events, --rounds windows of each variant, alternating; the figure is
us per batch as the loop sees it (launch issue included: at PEMS08 a batch is 0.5 MB and either
path is launch-bound).  The step the batch feeds is timed in the same process
(tools/bench_configs.run: one inner block forward + backward at the configuration's batch), and
the acceptance figure is (gather - index_select) / step <= 1 %.

    python tools/bench_windows.py --out profiles/windows_ab.json

With --missing-rate R (off by default) the tool measures the gap-aware path instead: a seeded
fraction R of the series is set to NaN and the masked gather (``fill='mean'`` and
``fill='ffill'``: dstagnn::window_gather_masked) is timed beside the plain gather of the intact
series in the same alternating-window protocol at both geometries (and the masked gather of the
intact series: the select alone); the one-time
dstagnn::window_fill_forward and dstagnn::window_stats_masked (beside dstagnn::window_stats) are
timed once each, after one warm call.  The three move the same bytes; the figure to read is the
masked medians against the spread the plain variant's own windows show.

    python tools/bench_windows.py --missing-rate 0.2      (writes profiles/windows_gaps_ab.json)

The JSON carries the library stamp (dstagnn_drought_amd._lib.build_stamp).  There is no fallback:
without a HIP device the tool fails."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_SPEC = 8.0e12      # B/s, datasheet
HBM_COPY = 6.29e12     # B/s, a float4 copy kernel on this chip
# name: (L, N, F, hours, num_for_predict, points_per_hour, B, materialised samples)
GEOMETRIES = {"PEMS08": (17856, 170, 1, 1, 12, 12, 32, 4096), "GAMBIA": (4000, 2139, 4, 12, 12, 12, 4, 64)}


def time_config(torch, name, iters, rounds, warmup):
    import numpy as np
    from dstagnn_drought_amd import WindowedSeries
    L, N, F, nh, P, pph, B, S = GEOMETRIES[name]
    rng = np.random.default_rng(1)
    series = (rng.standard_normal((L, N, F), dtype=np.float32) + 2.0)
    ws = WindowedSeries(series, 0, 0, nh, P, points_per_hour=pph)  # statistics from window_stats
    dev, Tin = ws.device, ws.Tin
    n_train = len(ws.labels["train"])
    gen = torch.Generator().manual_seed(2)
    pick = torch.randperm(n_train, generator=gen)[:S].to(dev)  # the samples both paths cut from
    parts = [ws.batch("train", pick[i:i + 4 * B]) for i in range(0, S, 4 * B)]
    mx, my = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    del parts
    order = torch.randperm(S, generator=gen).to(dev)  # positions in the materialised tensors
    sidx = pick[order]                                # the same samples as positions in the split
    nb = S // B

    def gather(i):
        return ws.batch("train", sidx[i * B:(i + 1) * B])

    def select(i):
        idx = order[i * B:(i + 1) * B]
        return mx.index_select(0, idx), my.index_select(0, idx)

    for i in range(nb):  # the two paths give the same bits
        (xa, ya), (xb, yb) = gather(i), select(i)
        assert torch.equal(xa.view(torch.int32), xb.view(torch.int32)) and torch.equal(ya, yb), (name, i)
    variants = {"gather": gather, "index_select": select}
    for f in variants.values():
        for i in range(warmup):
            f(i % nb)
    torch.cuda.synchronize()
    runs = {k: [] for k in variants}
    for _ in range(rounds):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(iters):
                f(i % nb)
            e1.record()
            e1.synchronize()
            runs[k].append(round(e0.elapsed_time(e1) / iters * 1e3, 3))
    med = {k: statistics.median(r) for k, r in runs.items()}
    item = series.dtype.itemsize
    moved = B * N * (Tin * F * item + P * item + F * Tin * 4 + P * 4)  # rows read + x, y written
    out = {"series": [L, N, F], "dtype": str(series.dtype), "Tin": Tin, "B": B, "tile_nodes": ws.tile_nodes(),
           "materialised_samples": S, "us_per_batch_runs": runs, "median_us": med,
           "spread": {k: round((max(r) - min(r)) / med[k], 4) for k, r in runs.items()},
           "bytes_moved_per_batch": moved,
           "gather_fraction_of_hbm_spec_8TBs": round(moved / (med["gather"] * 1e-6) / HBM_SPEC, 4),
           "gather_fraction_of_hbm_copy_6_29TBs": round(moved / (med["gather"] * 1e-6) / HBM_COPY, 4),
           "index_select_fraction_of_hbm_spec_8TBs": round(moved / (med["index_select"] * 1e-6) / HBM_SPEC, 4),
           "series_bytes": int(series.nbytes),
           "one_sample_bytes": N * F * Tin * 4,
           "bits_equal_to_index_select": True}
    del ws, mx, my
    torch.cuda.empty_cache()
    return out


def time_gaps(torch, name, rate, iters, rounds, warmup):
    """The masked gather (both fills) beside the plain one, and the one-time fill / statistics."""
    import numpy as np
    from dstagnn_drought_amd import WindowedSeries
    from dstagnn_drought_amd import windows as W
    L, N, F, nh, P, pph, B, S = GEOMETRIES[name]
    rng = np.random.default_rng(1)
    series = (rng.standard_normal((L, N, F), dtype=np.float32) + 2.0)
    gapped = series.copy()
    gapped[rng.random(series.shape) < rate] = np.nan
    nan = float("nan")
    plain = WindowedSeries(series, 0, 0, nh, P, points_per_hour=pph)
    owners = {"gather": plain,
              "gather_masked_mean": WindowedSeries(gapped, 0, 0, nh, P, points_per_hour=pph, missing_value=nan),
              "gather_masked_ffill": WindowedSeries(gapped, 0, 0, nh, P, points_per_hour=pph, missing_value=nan,
                                                    fill="ffill"),
              # the masked kernel where nothing is missing: the cost of the select alone
              "gather_masked_intact": WindowedSeries(series, 0, 0, nh, P, points_per_hour=pph, missing_value=nan)}
    ops, dev, Tin = plain._ops, plain.device, plain.Tin
    gen = torch.Generator().manual_seed(2)
    sidx = torch.randperm(len(plain.labels["train"]), generator=gen)[:S].to(dev)
    nb = S // B
    variants = {k: (lambda i, ws=ws: ws.batch("train", sidx[i * B:(i + 1) * B])) for k, ws in owners.items()}
    for k, f in variants.items():
        x, y = f(0)
        assert bool(torch.isfinite(x).all()), k  # (the plain one reads the intact series)
        for i in range(warmup):
            f(i % nb)
    torch.cuda.synchronize()
    runs = {k: [] for k in variants}
    for _ in range(rounds):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(iters):
                f(i % nb)
            e1.record()
            e1.synchronize()
            runs[k].append(round(e0.elapsed_time(e1) / iters * 1e3, 3))
    med = {k: statistics.median(r) for k, r in runs.items()}

    def once(f):  # one warm call, then one timed call
        f()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        return round(e0.elapsed_time(e1) * 1e3, 1)

    gws = owners["gather_masked_ffill"]
    w = W.window_weights(L, plain.labels["train"], plain.rel)
    wd, wtotal = torch.from_numpy(w).to(dev), float(N) * float(w.astype(np.int64).sum())
    one_time = {"window_fill_forward_us": once(lambda: ops.window_fill_forward(gws.series, nan, 0)),
                "window_stats_masked_us": once(lambda: ops.window_stats_masked(gws.series, wd, nan)),
                "window_stats_us": once(lambda: ops.window_stats(plain.series, wd, wtotal))}
    item = series.dtype.itemsize
    moved = B * N * (Tin * F * item + P * item + F * Tin * 4 + P * 4)
    spread = {k: round((max(r) - min(r)) / med[k], 4) for k, r in runs.items()}
    out = {"series": [L, N, F], "dtype": str(series.dtype), "Tin": Tin, "B": B, "missing_rate": rate,
           "missing_per_feature": gws.missing_count.tolist(), "filled_per_feature": gws.filled_count.tolist(),
           "us_per_batch_runs": runs, "median_us": med, "spread": spread,
           "masked_over_plain": {k: round(med[k] / med["gather"] - 1.0, 4) for k in med if k != "gather"},
           "inside_plain_spread": {k: bool(abs(med[k] - med["gather"]) <= max(runs["gather"]) - min(runs["gather"]))
                                   for k in med if k != "gather"},
           "bytes_moved_per_batch": moved, "one_time_us": one_time, "series_bytes": int(series.nbytes)}
    del owners, plain, gws
    torch.cuda.empty_cache()
    return out


def main_gaps(a, torch, _lib):
    rec = {"what": f"the masked gather (missing inputs imputed in the launch; fill = mean / ffill) beside the plain "
                   f"gather of the intact series, us per batch between device events, {a.rounds} alternating windows x "
                   f"{a.iters} batches; NaN at a seeded fraction {a.missing_rate} of the series; the one-time "
                   "window_fill_forward / window_stats_masked / window_stats: one timed call after a warm one "
                   "(tools/bench_windows.py --missing-rate)",
           "stamp": _lib.build_stamp(), "configs": {}}
    for name in GEOMETRIES:
        rec["configs"][name] = time_gaps(torch, name, a.missing_rate, a.iters, a.rounds, a.warmup)
        print(f"[windows gaps] {name}: {rec['configs'][name]}", file=sys.stderr, flush=True)
    print(json.dumps(rec))
    out = a.out or os.path.join(ROOT, "profiles", "windows_gaps_ab.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000, help="batches per window (>= 100)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--step-steps", type=int, default=50, help="steps of the block timing per configuration")
    ap.add_argument("--missing-rate", type=float, default=None,
                    help="measure the gap-aware path instead: this fraction of the series is NaN "
                         "(writes profiles/windows_gaps_ab.json unless --out is given)")
    ap.add_argument("--out", default=None,
                    help="default: profiles/windows_ab.json (profiles/windows_gaps_ab.json with --missing-rate)")
    a = ap.parse_args()
    if a.iters < 100:
        ap.error("--iters must be at least 100")
    if a.missing_rate is not None and not 0.0 < a.missing_rate < 1.0:
        ap.error("--missing-rate must lie in (0, 1)")
    import torch
    from dstagnn_drought_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_windows.py measures on the GPU only: no HIP device")
    torch.cuda.set_device(0)
    if a.missing_rate is not None:
        return main_gaps(a, torch, _lib)
    a.out = a.out or os.path.join(ROOT, "profiles", "windows_ab.json")
    import bench_configs
    rec = {"what": f"one batch cut from the raw series (gather) vs from materialised tensors (index_select), us per "
                   f"batch between device events, {a.rounds} alternating windows x {a.iters} batches; the step is one "
                   f"inner block forward + backward (tools/bench_configs.run, {a.step_steps} steps) in the same process "
                   "(tools/bench_windows.py)",
           "criterion": "(gather - index_select) / step <= 0.01",
           "stamp": _lib.build_stamp(), "configs": {}}
    for name in GEOMETRIES:
        r = time_config(torch, name, a.iters, a.rounds, a.warmup)
        step = bench_configs.run(name, steps=a.step_steps, warmup=10)
        r["step_ms"] = step["ms_per_step"]
        r["extra_us_per_batch"] = round(r["median_us"]["gather"] - r["median_us"]["index_select"], 3)
        r["extra_over_step"] = round(r["extra_us_per_batch"] * 1e-3 / step["ms_per_step"], 5)
        r["within_1_percent"] = bool(r["extra_over_step"] <= 0.01)
        rec["configs"][name] = r
        print(f"[windows] {name}: {r}", file=sys.stderr, flush=True)
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
