#!/usr/bin/env python
"""What gradient clipping costs on the PEMS08 model step (make_model nb_block=4, B=32, train:
forward, SmoothL1, backward, optimiser), three ways, interleaved in one process:

    (a) HipAdam as the driver builds it (no clipping)             one adam_step launch
    (b) torch.nn.utils.clip_grad_norm_ + HipAdam                  the only way to clip before
    (c) HipAdam(max_grad_norm=)                                   grad_sumsq + adam_step_ex

    python tools/bench_clip.py --out profiles/adam_clip_ab.json          # 3 rounds x 100 steps each
    rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- \
        python tools/bench_clip.py --rounds 1 --steps 20 --out ''           # kernel durations, a run of its own
    python tools/bench_clip.py --kernel-stats DIR/.../run_kernel_stats.csv --out profiles/adam_clip_ab.json

A round times `--steps` steps of each variant between two device synchronisations (host clock);
the rounds alternate the variants, so a difference can be held against the round-to-round spread.
The JSON carries the library stamp (dstagnn_drought_amd._lib.build_stamp), ms per step of every
round, the medians, (b) - (a), (c) - (a) and (c) / (b); --kernel-stats adds the average
duration of the optimiser's kernels from a rocprofv3 --stats run."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("grad_sumsq_kernel", "adam_ex_kernel", "adam_kernel", "grad_scale_kernel")


def merge_kernel_stats(path, out):
    with open(out) as f:
        rec = json.load(f)
    found = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                if f"::{k}(" in row["Name"] or row["Name"].startswith(k + "("):
                    found[k] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 3),
                                "min_us": round(float(row["MinNs"]) / 1e3, 3),
                                "max_us": round(float(row["MaxNs"]) / 1e3, 3)}
    rec["kernel_us"] = {"what": "rocprofv3 --kernel-trace --stats over a run of its own (adam_kernel: variants a "
                                "and b; grad_sumsq_kernel, adam_ex_kernel: variant c)", **found}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec["kernel_us"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--max-norm", type=float, default=0.1, help="below the model's gradient norm (~0.3): it clips")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_clip_ab.json"))
    ap.add_argument("--kernel-stats", default=None, help="merge a rocprofv3 kernel_stats.csv into --out and exit")
    a = ap.parse_args()
    if a.kernel_stats:
        return merge_kernel_stats(a.kernel_stats, a.out)
    import torch
    import bench
    import dstagnn_drought_amd as D
    from dstagnn_drought_amd import _lib
    from dstagnn_drought_amd.train import HipAdam
    assert torch.cuda.is_available(), "bench_clip.py measures on the GPU only"
    c = bench.CFG
    B, N, T, K, h, Dm, dk, C = c["B"], c["N"], c["T"], c["K"], c["n_heads"], c["d_model"], c["d_k"], c["C"]
    dev = torch.device("cuda:0")
    tmd, pa = bench.synth_graph(N)
    torch.manual_seed(1)
    net = D.make_model(dev, 1, 4, 1, K, C, C, 1, tmd, pa, tmd, T, T, N, Dm, dk, dk, h)
    D.set_direct_grads(net).train()
    params = list(net.parameters())
    crit = torch.nn.SmoothL1Loss().to(dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    xm = torch.randn(B, N, 1, T, device=dev, generator=gen)
    ym = torch.randn(B, N, T, device=dev, generator=gen)
    opts = {"a": HipAdam(params, lr=1e-4), "b": HipAdam(params, lr=1e-4),
            "c": HipAdam(params, lr=1e-4, max_grad_norm=a.max_norm)}

    def step(v):
        opt = opts[v]
        opt.zero_grad(set_to_none=True)
        crit(net(xm), ym).backward()
        if v == "b":
            torch.nn.utils.clip_grad_norm_(params, a.max_norm)
        opt.step()

    variants = ["a", "b", "c"]
    for v in variants:
        for _ in range(a.warmup):
            step(v)
    torch.cuda.synchronize()
    runs = {v: [] for v in variants}
    for _ in range(a.rounds):
        for v in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step(v)
            torch.cuda.synchronize()
            runs[v].append(round((time.perf_counter() - t0) / a.steps * 1e3, 4))
    med = {v: statistics.median(r) for v, r in runs.items()}
    rec = {"what": "PEMS08 model step (make_model nb_block=4, B=32, train: forward, SmoothL1, backward, optimiser), "
                   f"ms per step; {a.rounds} rounds x {a.steps} steps per variant, rounds interleaved in one process "
                   "(tools/bench_clip.py)",
           "variants": {"a": "HipAdam, no clipping", "b": "torch.nn.utils.clip_grad_norm_ + HipAdam",
                        "c": "HipAdam(max_grad_norm=)"},
           "stamp": _lib.build_stamp(), "max_norm": a.max_norm, "parameters": len(params),
           "elements": sum(p.numel() for p in params),
           "grad_norm_last_step": float(opts["c"].grad_norm), "ms_per_step_runs": runs, "median": med,
           "b_minus_a_ms": round(med["b"] - med["a"], 4), "c_minus_a_ms": round(med["c"] - med["a"], 4),
           "c_over_b": round(med["c"] / med["b"], 4),
           "spread": {v: round((max(r) - min(r)) / med[v], 4) for v, r in runs.items()}}
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
