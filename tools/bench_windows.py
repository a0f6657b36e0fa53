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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000, help="batches per window (>= 100)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--step-steps", type=int, default=50, help="steps of the block timing per configuration")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "windows_ab.json"))
    a = ap.parse_args()
    if a.iters < 100:
        ap.error("--iters must be at least 100")
    import torch
    from dstagnn_drought_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_windows.py measures on the GPU only: no HIP device")
    torch.cuda.set_device(0)
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
