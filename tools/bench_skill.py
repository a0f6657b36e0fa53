#!/usr/bin/env python
"""What the baseline skill scores cost, A/B in one process:

  (1) one BaselineSkill.update (skill_kernel: the (P, 13) and (N, 13) running tables, both baselines
      read out of the series inside the launch) against the same 13 sums written as torch tensor
      expressions on the GPU (what a user writes today: gathers of the persistence and climatology
      values, boolean selects, two reductions; no host copy), at the head shapes (B, N, P) of PEMS08
      (32, 170, 12) and GAMBIA (4, 2139, 12), NaN marker on 15 % of the series: after a warm-up,
      windows of --iters updates between two device events, --rounds windows of each variant,
      alternating, so a difference can be held against the spread.  At these sizes an update is a
      handful of launches on the torch side and one on ours: the figure is the host's issue rate as
      much as the kernels' time;
  (2) train.score_batches over the test split of a PEMS08-shaped streamed series (make_model
      nb_block=4, B=32) with and without ``skill=``: host clock around a pass that ends in a device
      synchronise, --rounds alternating passes.

    python tools/bench_skill.py --out profiles/skill_ab.json

The JSON carries the library stamp (dstagnn_drought_amd._lib.build_stamp).  There is no fallback:
without a HIP device the tool fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"PEMS08": (32, 170, 12), "GAMBIA": (4, 2139, 12)}
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


def _series(np, L, N, period, gaps, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(L)[:, None, None]
    s = (10.0 + 3.0 * np.sin(2 * np.pi * t / period + np.arange(N)[None, :, None]) + rng.normal(0, 1, (L, N, 1)))
    s = s.astype(np.float32)
    if gaps:
        s[rng.random(s.shape) < gaps] = NAN
    return s


def time_update(torch, dev, shape, period, iters, rounds, warmup):
    import numpy as np
    from dstagnn_drought_amd import BaselineSkill, WindowedSeries
    B, N, P = shape
    L = 40 * P + 5 * B
    ws = WindowedSeries(_series(np, L, N, period, 0.15, 3), 0, 0, 1, P, points_per_hour=P, device=dev,
                        missing_value=NAN)
    sk = BaselineSkill(ws, period, missing_value=NAN, num_nodes=N)
    _, t = ws.batch("test", slice(0, B))
    assert t.shape[0] == B
    gen = torch.Generator(device=dev).manual_seed(11)
    y = torch.where(torch.isnan(t), torch.ones_like(t), t) + torch.randn(shape, device=dev, generator=gen)
    pos = ws._labels["test"][:B]
    src, clim, cnt = sk._pers, sk._clim, sk._cnt
    ht = torch.zeros(P, 13, dtype=torch.float64, device=dev)
    nt = torch.zeros(N, 13, dtype=torch.float64, device=dev)
    steps = torch.arange(P, device=dev)

    def torch_update():  # no boolean indexing: no sync
        valid = ~torch.isnan(t)
        tz = torch.where(valid, t, torch.zeros_like(t))
        q = src[pos - 1, :, -1]                                   # (B, N): the forward-filled series
        sp = valid & ~torch.isnan(q)[:, :, None]
        q = torch.nan_to_num(q)[:, :, None]
        ph = (pos[:, None] + steps[None, :]) % period             # (B, P)
        sc = valid & (cnt[ph] > 0).transpose(1, 2)
        c = torch.nan_to_num(clim[ph]).transpose(1, 2).float()    # (B, N, P)
        em, ep, ec, af, ao = y - tz, q - tz, c - tz, y - c, tz - c
        em2, ema, one = (em * em).double(), em.abs().double(), torch.ones_like(em, dtype=torch.float64)
        zero = torch.zeros_like(one)
        af, ao = af.double(), ao.double()
        cols = [(sp, one), (sp, em2), (sp, (ep * ep).double()), (sp, ema), (sp, ep.abs().double()),
                (sc, one), (sc, em2), (sc, (ec * ec).double()), (sc, ema), (sc, ec.abs().double()),
                (sc, af * ao), (sc, af * af), (sc, ao * ao)]
        terms = torch.stack([torch.where(sel, v, zero) for sel, v in cols], -1)
        ht.add_(terms.sum((0, 1)))
        nt.add_(terms.sum((0, 2)))

    def hip_update():
        sk.update(y, t, "test", slice(0, B))

    for _ in range(max(warmup // 10, 10)):
        torch_update()
        hip_update()
    torch.cuda.synchronize()
    sk.reset(), ht.zero_(), nt.zero_()
    torch_update()
    hip_update()
    diff = float((sk.table - ht).abs().max() / ht.abs().max())
    counts_equal = bool(torch.equal(sk.table[:, [0, 5]], ht[:, [0, 5]]))
    runs, med, spread = _windows(torch, {"torch": torch_update, "hip": hip_update}, iters, rounds)
    return {"shape": [B, N, P], "period": period, "series": [L, N, 1], "us_per_update_runs": runs, "median_us": med,
            "spread": spread, "hip_over_torch": round(med["hip"] / med["torch"], 4),
            "worst_table_difference_relative_to_its_largest_entry": diff, "counts_equal": counts_equal}


def time_scoring(torch, dev, rounds, period=12):
    import numpy as np
    import bench
    import dstagnn_drought_amd as D
    from dstagnn_drought_amd import train as TR
    c = bench.CFG
    B, N, T, K, h, Dm, dk, C = c["B"], c["N"], c["T"], c["K"], c["n_heads"], c["d_model"], c["d_k"], c["C"]
    tmd, pa = bench.synth_graph(N)
    torch.manual_seed(1)
    net = D.make_model(dev, 1, 4, 1, K, C, C, 1, tmd, pa, tmd, T, T, N, Dm, dk, dk, h).eval()
    ws = D.WindowedSeries(_series(np, 10240, N, period, 0.15, 5), 0, 0, 1, T, points_per_hour=T, device=dev,
                          missing_value=NAN)
    sp = ws.split("test")
    sk = D.BaselineSkill(ws, period, missing_value=NAN, num_nodes=N)

    def without():
        return TR.score_batches(net, sp.x, sp.y, B, NAN, True)

    def with_skill():
        sk.reset()
        return TR.score_batches(net, sp.x, sp.y, B, NAN, True, skill=sk)

    variants = {"without": without, "with_skill": with_skill}
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
    batches = -(-sp.x.shape[0] // B)
    return {"model": "make_model nb_block=4, PEMS08 shape", "batches": batches, "batch_size": B,
            "ms_per_pass_runs": runs, "median_ms": med, "with_over_without": round(med["with_skill"] / med["without"], 4),
            "us_per_batch_added": round((med["with_skill"] - med["without"]) / batches * 1e3, 3),
            "spread": {k: round((max(r) - min(r)) / med[k], 4) for k, r in runs.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000, help="updates per window (>= 200)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skill_ab.json"))
    a = ap.parse_args()
    if a.iters < 200 or a.rounds < 3:
        ap.error("--iters must be at least 200 and --rounds at least 3")
    import torch
    from dstagnn_drought_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_skill.py measures on the GPU only: no HIP device")
    dev = torch.device("cuda:0")
    rec = {"what": "one baseline-skill update (13 sums per horizon and per node, NaN marker on 15 % of the series), us "
                   f"per call between device events, {a.rounds} alternating windows x {a.iters} calls; score_batches "
                   "with and without skill=, ms per pass on the host clock (tools/bench_skill.py)",
           "variants": {"torch": "the same sums as torch tensor expressions on the GPU",
                        "hip": "BaselineSkill.update with the node table (skill_kernel)"},
           "stamp": _lib.build_stamp(),
           "update": {name: time_update(torch, dev, SHAPES[name], 12, a.iters, a.rounds, a.warmup) for name in SHAPES},
           "scoring": time_scoring(torch, dev, a.rounds)}
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
