#!/usr/bin/env python
"""What the drought event scores cost, A/B in one process:

  (1) one EventScores.update (events_kernel: the (P, 2 + (K + 1)^2) and (N, ...) running contingency
      tables in one launch) against the same counts written as torch tensor expressions on the GPU
      (what a user writes today: K compares and a sum per class, a select for the NaN predictions and
      the masked targets, one torch.bincount per table; no prediction goes to the host, but bincount
      itself reads its largest index back), at the head shapes (B, N, P) of PEMS08 (32, 170, 12) and
      GAMBIA (4, 2139, 12), K = 3 thresholds (-1, -1.5, -2), NaN marker on 15 % of the targets:
      after a warm-up, windows of --iters updates between two device events, --rounds windows of
      each variant, alternating, so a difference can be held against the spread.  At these sizes an
      update is a dozen launches on the torch side and one on ours: the figure is the host's issue
      rate as much as the kernels' time;
  (2) train.score_batches over a PEMS08-shaped test split (make_model nb_block=4, B=32) with and
      without ``events=``: host clock around a pass that ends in a device synchronise, --rounds
      alternating passes.

    python tools/bench_events.py --out profiles/events_ab.json

Both sides must give equal tables (they are integers): the tool fails otherwise.  The JSON carries
the library stamp (dstagnn_drought_amd._lib.build_stamp).  There is no fallback: without a HIP device
the tool fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"PEMS08": (32, 170, 12), "GAMBIA": (4, 2139, 12)}
THRESHOLDS = (-1.0, -1.5, -2.0)
NAN = float("nan")


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


def _pair(torch, dev, shape, seed):
    """SPI-like targets (standard normal, 15 % NaN) and a forecast with unit-variance error, 1 % NaN."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    t = torch.randn(shape, device=dev, generator=gen)
    y = 0.8 * t + 0.6 * torch.randn(shape, device=dev, generator=gen)
    t = torch.where(torch.rand(shape, device=dev, generator=gen) < 0.15, torch.full_like(t, NAN), t)
    y = torch.where(torch.rand(shape, device=dev, generator=gen) < 0.01, torch.full_like(y, NAN), y)
    return y, t


def time_update(torch, dev, shape, iters, rounds, warmup):
    from dstagnn_drought_amd import EventScores
    B, N, P = shape
    K = len(THRESHOLDS)
    K1, cols = K + 1, 2 + (K + 1) ** 2
    ev = EventScores(P, THRESHOLDS, missing_value=NAN, num_nodes=N, device=dev)
    y, t = _pair(torch, dev, shape, 11)
    thr = torch.tensor(THRESHOLDS, dtype=torch.float32, device=dev)
    ht = torch.zeros(P, cols, dtype=torch.float64, device=dev)
    nt = torch.zeros(N, cols, dtype=torch.float64, device=dev)
    prow = (torch.arange(P, device=dev) * (cols + 1))[None, None, :]
    nrow = (torch.arange(N, device=dev) * (cols + 1))[None, :, None]

    def torch_update():  # no boolean indexing; one dump column (cols) for the masked targets
        valid = ~torch.isnan(t)
        co = (t[..., None] <= thr).sum(-1)
        cf = (y[..., None] <= thr).sum(-1)
        cell = torch.where(torch.isnan(y), torch.ones_like(co), 2 + co * K1 + cf)
        cell = torch.where(valid, cell, torch.full_like(cell, cols))
        h = torch.bincount((prow + cell).reshape(-1), minlength=P * (cols + 1)).view(P, cols + 1)
        n = torch.bincount((nrow + cell).reshape(-1), minlength=N * (cols + 1)).view(N, cols + 1)
        ht[:, 1:].add_(h[:, 1:cols])
        nt[:, 1:].add_(n[:, 1:cols])
        ht[:, 0].add_(valid.sum((0, 1)))
        nt[:, 0].add_(valid.sum((0, 2)))

    def hip_update():
        ev.update(y, t)

    for _ in range(max(warmup // 10, 10)):
        torch_update()
        hip_update()
    torch.cuda.synchronize()
    ev.reset(), ht.zero_(), nt.zero_()
    torch_update()
    hip_update()
    equal = bool(torch.equal(ev.table, ht)) and bool(torch.equal(ev.node_table, nt))
    if not equal:
        raise SystemExit(f"bench_events.py: the two sides give different tables at {shape}")
    runs, med, spread = _windows(torch, {"torch": torch_update, "hip": hip_update}, iters, rounds)
    return {"shape": [B, N, P], "K": K, "thresholds": list(THRESHOLDS), "us_per_update_runs": runs, "median_us": med,
            "spread": spread, "hip_over_torch": round(med["hip"] / med["torch"], 4), "tables_equal": equal,
            "counted_entries": int(ev.table[:, 0].sum().item())}


def time_scoring(torch, dev, rounds):
    import bench
    import dstagnn_drought_amd as D
    from dstagnn_drought_amd import train as TR
    c = bench.CFG
    B, N, T, K, h, Dm, dk, C = c["B"], c["N"], c["T"], c["K"], c["n_heads"], c["d_model"], c["d_k"], c["C"]
    tmd, pa = bench.synth_graph(N)
    torch.manual_seed(1)
    net = D.make_model(dev, 1, 4, 1, K, C, C, 1, tmd, pa, tmd, T, T, N, Dm, dk, dk, h).eval()
    S = 64 * B
    gen = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(S, N, 1, T, device=dev, generator=gen)
    _, y = _pair(torch, dev, (S, N, T), 6)
    ev = D.EventScores(T, THRESHOLDS, missing_value=NAN, num_nodes=N, device=dev)

    def without():
        return TR.score_batches(net, x, y, B, NAN, True)

    def with_events():
        ev.reset()
        return TR.score_batches(net, x, y, B, NAN, True, events=ev)

    variants = {"without": without, "with_events": with_events}
    for f in variants.values():
        f()
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
    batches = -(-S // B)
    return {"model": "make_model nb_block=4, PEMS08 shape", "batches": batches, "batch_size": B,
            "ms_per_pass_runs": runs, "median_ms": med, "with_over_without": round(med["with_events"] / med["without"], 4),
            "us_per_batch_added": round((med["with_events"] - med["without"]) / batches * 1e3, 3),
            "spread": {k: round((max(r) - min(r)) / med[k], 4) for k, r in runs.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000, help="updates per window (>= 200)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "events_ab.json"))
    a = ap.parse_args()
    if a.iters < 200 or a.rounds < 3:
        ap.error("--iters must be at least 200 and --rounds at least 3")
    import torch
    from dstagnn_drought_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_events.py measures on the GPU only: no HIP device")
    dev = torch.device("cuda:0")
    rec = {"what": "one drought-event update (contingency counts per horizon and per node, K = 3, NaN marker on 15 % of "
                   f"the targets), us per call between device events, {a.rounds} alternating windows x {a.iters} calls; "
                   "score_batches with and without events=, ms per pass on the host clock (tools/bench_events.py)",
           "variants": {"torch": "the same counts as torch tensor expressions on the GPU (compare, sum, bincount)",
                        "hip": "EventScores.update with the node table (events_kernel)"},
           "stamp": _lib.build_stamp(),
           "update": {name: time_update(torch, dev, SHAPES[name], a.iters, a.rounds, a.warmup) for name in SHAPES},
           "scoring": time_scoring(torch, dev, a.rounds)}
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
